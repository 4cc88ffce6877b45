"""Added backward time of the input-gradient path at the c2 shape (bs 256, 36 boxes, seq 20, 12 layers), device events:
`python tools/input_grad_bench.py` on the MI355X."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clg_vqa_amd import ops, task_utils  # noqa: E402
from clg_vqa_amd.config import GQA_TASK_CFG as TASK_CFG  # noqa: E402
from clg_vqa_amd.config import BertConfig, uc2_base_config  # noqa: E402
from clg_vqa_amd.encoders import BertForVLTasks  # noqa: E402
from clg_vqa_amd.engine import input_grad_feats, input_grad_locs  # noqa: E402
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
crit = torch.nn.CrossEntropyLoss()


def step(i, want):
    b = list(batches[i % 4])
    b[0] = b[0].detach().requires_grad_(want)
    b[1] = b[1].detach().requires_grad_(want)
    loss, _ = task_utils.ForwardModelsTrain(config, TASK_CFG, dev, "TASK15", tuple(b), model, crit)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss.backward()
    e1.record()
    opt.step()
    torch.cuda.synchronize()
    if want:
        assert b[0].grad is not None and b[1].grad is not None
    return e0.elapsed_time(e1)


for i in range(6):
    step(i, i % 2 == 1)
t = {False: [], True: []}
for i in range(40):
    want = i % 2 == 1
    t[want].append(step(i, want))
for want in (False, True):
    v = sorted(t[want])
    print("backward, input grads %s: median %.3f ms  min %.3f  max %.3f (n=%d)" % (want, v[len(v) // 2], v[0], v[-1], len(v)))

# the two products alone at c2's BV = 9216
BV, H, F, L = 9216, 768, 2048, 7
g = torch.Generator().manual_seed(0)
dloc = torch.randn(BV, H, generator=g).to(dev)
wl = torch.randn(H, L, generator=g).to(dev)
d16 = torch.randn(BV, H, generator=g).to(dev).to(torch.bfloat16)
w_hi = torch.randn(H, F, generator=g).to(dev).to(torch.bfloat16)
filler = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
for name, fn in (("loc_linear_bwd_input", lambda: input_grad_locs(dloc, wl)), ("transpose + 1-pass GEMM", lambda: input_grad_feats(d16, w_hi))):
    for cold in (False, True):
        ts = []
        for _ in range(20):
            if cold:
                filler.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = sorted(ts[3:])
        print("%s %s: median %.1f us  min %.1f us" % (name, "cold" if cold else "warm", ts[len(ts) // 2], ts[0]))
