"""Added backward time of differentiable hidden-state taps at the c2 shape (bs 256, 36 boxes, seq 20, 12 layers), device
events around `loss.backward()`: a tapped call whose taps stay detached against one whose loss reads 1 / all 25 hidden
states (alternating steps; autograd's assembly of the tap gradients is part of the figure).
`python tools/diff_taps_bench.py` on the MI355X."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clg_vqa_amd.config import GQA_TASK_CFG as TASK_CFG  # noqa: E402
from clg_vqa_amd.config import BertConfig, uc2_base_config  # noqa: E402
from clg_vqa_amd.encoders import BertForVLTasks  # noqa: E402
from clg_vqa_amd.optim import FusedAdamW  # noqa: E402
from clg_vqa_amd.synthetic import make_batch  # noqa: E402

dev = torch.device("cuda", 0)
torch.manual_seed(1234)
config = BertConfig.from_dict(uc2_base_config())
model = BertForVLTasks(config, TASK_CFG, ["TASK15"]).to(dev)
model.train()
opt = FusedAdamW(model, base_lr=4e-5, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-6, correct_bias=True, max_grad_norm=1.0,
                 warmup_steps=100, t_total=100000)
batches = [tuple(t.to(dev) for t in make_batch(256, seed=1234 + 1000 * i)) for i in range(4)]
MODES = (("taps detached", False, ()), ("1 hidden state in the loss", True, (12,)), ("all 25 in the loss", True, tuple(range(25))))


def step(i, diff, used):
    feats, spat, imask, q, target, tmask, seg = batches[i % 4][:7]
    model.differentiable_encoded_layers = diff
    out = model(q, feats, spat, "TASK15", seg, tmask, imask, output_all_encoded_layers=True)
    loss = torch.nn.functional.cross_entropy(out[0], target.argmax(1))
    for k in used:
        loss = loss + 1e-3 * (out[4][k].square().mean() + out[5][k].square().mean())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss.backward()
    e1.record()
    opt.step()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for i in range(6):
    step(i, *MODES[i % 3][1:])
t = {m[0]: [] for m in MODES}
for i in range(60):
    m = MODES[i % 3]
    t[m[0]].append(step(i, *m[1:]))
for name, v in t.items():
    v = sorted(v)
    print("backward, %s: median %.3f ms  min %.3f  max %.3f (n=%d)" % (name, v[len(v) // 2], v[0], v[-1], len(v)))
