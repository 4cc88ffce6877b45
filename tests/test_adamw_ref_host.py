"""tests/adamw_ref.py (the fp64 restatement the GPU tests hold the fused step to) against
oracle.adamw_oracle.ReferenceAdamW, on the CPU: parameter groups with both learning rates and both decays, warm-up,
clip active / inactive / off, a parameter that never has a gradient and one that misses the first step."""
import pytest
import torch

from adamw_ref import adamw_step
from oracle.adamw_oracle import NO_DECAY, ReferenceAdamW, warmup_linear

SHAPES = [("bert.encoder.layer.0.output.dense.weight", (13, 7)),
          ("bert.encoder.layer.0.output.dense.bias", (13,)),
          ("bert.encoder.layer.0.output.LayerNorm.weight", (7,)),
          ("bert.embeddings.task_embeddings.weight", (5, 6)),      # never receives a gradient
          ("vil_prediction.logit_fc.0.weight", (9, 13)),
          ("vil_prediction.logit_fc.0.bias", (9,)),
          ("bert.t_pooler.dense.weight", (3, 3)),                  # misses the first step: its own step count
          ("vil_logit.weight", (1, 11))]
NEVER, LATE = 3, 6
BASE_LR, WD, B1, B2, EPS = 4e-5, 1e-2, 0.9, 0.999, 1e-6
WARMUP, T_TOTAL, STEPS = 2, 10, 3


# the gradient norm of these steps is between 3 and 6: 0.5 always clips, 100 never does
@pytest.mark.parametrize("max_grad_norm", [0.5, 100.0, None], ids=["clip", "noclip", "off"])
@pytest.mark.parametrize("correct_bias", [True, False])
def test_fp64_restatement_equals_the_oracle_optimizer(max_grad_norm, correct_bias):
    gen = torch.Generator().manual_seed(11)
    params = [(n, torch.nn.Parameter(torch.randn(*s, generator=gen))) for n, s in SHAPES]
    opt = ReferenceAdamW(params, BASE_LR, WD, betas=(B1, B2), eps=EPS, correct_bias=correct_bias, warmup_steps=WARMUP,
                         t_total=T_TOTAL, max_grad_norm=max_grad_norm)
    lrs = [g["lr"] for g in opt.groups]
    wds = [g["wd"] for g in opt.groups]
    assert sorted(set(lrs)) == [BASE_LR, 1e-4] and sorted(set(wds)) == [0.0, WD]
    assert all((wd == 0.0) == any(nd in n for nd in NO_DECAY) for (n, _), wd in zip(SHAPES, wds))
    # the flat arena: 4-aligned segments, pad elements zero
    sizes = [p.numel() for _, p in params]
    offs, total = [], 0
    for s in sizes:
        offs.append(total)
        total += (s + 3) // 4 * 4
    ends = offs[1:] + [total]
    p = torch.zeros(total, dtype=torch.float64)
    for (_, q), o, s in zip(params, offs, sizes):
        p[o:o + s] = q.detach().double().view(-1)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    seg_steps = [0] * len(params)
    # every element keeps the sign of its gradient over the steps, so that b1 m + (1 - b1) g does not cancel and a pure
    # relative bound can hold against the oracle's fp32 arithmetic
    signs = [torch.where(torch.rand(*s, generator=gen) < 0.5, -1.0, 1.0) for _, s in SHAPES]
    seen = set()
    for step in range(1, STEPS + 1):
        g = torch.zeros(total, dtype=torch.float64)
        has = []
        for i, ((_, q), o, s) in enumerate(zip(params, offs, sizes)):
            has.append(i != NEVER and not (i == LATE and step == 1))
            if has[-1]:
                q.grad = signs[i] * (0.05 + torch.rand(*q.shape, generator=gen))
                g[o:o + s] = q.grad.double().view(-1)
                seg_steps[i] += 1
        mult = warmup_linear(step - 1, WARMUP, T_TOTAL)
        sumsq = (g * g).sum()
        norm = opt.step()
        kw = dict(grad_scale=1.0) if max_grad_norm is None else dict(sumsq=sumsq, max_norm=max_grad_norm, post=1.0)
        p, m, v, gs = adamw_step(p, g, m, v, ends, [lr if h else -1.0 for lr, h in zip(lrs, has)], wds, B1, B2, EPS, step,
                                 correct_bias, mult, seg_step=seg_steps, **kw)
        if max_grad_norm is None:
            assert norm is None and gs.item() == 1.0
        else:
            torch.testing.assert_close(norm.double(), sumsq.sqrt(), rtol=1e-6, atol=0.0)
            seen.add(bool(gs.item() < 1.0))
            assert (gs.item() < 1.0) == (norm.item() > max_grad_norm)
        for grp, o, s in zip(opt.groups, offs, sizes):
            assert grp["p"].grad is None
            for name, mine, theirs in (("p", p, grp["p"]), ("m", m, grp["m"]), ("v", v, grp["v"])):
                torch.testing.assert_close(mine[o:o + s], theirs.detach().double().view(-1), rtol=1e-6, atol=0.0,
                                           msg=lambda t, n=name, g_=grp: "%s of %s at step %d: %s" % (n, g_["name"], step, t))
        assert [grp["step"] for grp in opt.groups] == seg_steps
    assert seen == ({True} if max_grad_norm == 0.5 else {False} if max_grad_norm == 100.0 else set())
    assert seg_steps[NEVER] == 0 and seg_steps[LATE] == STEPS - 1
    untouched = params[NEVER][1].detach().double().view(-1)
    assert torch.equal(p[offs[NEVER]:offs[NEVER] + sizes[NEVER]], untouched)  # never moved, not even by decay
