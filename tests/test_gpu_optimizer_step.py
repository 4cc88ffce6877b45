"""The fused clip + AdamW step (vl_adamw, FusedAdamW.step) against the fp64 restatement of tests/adamw_ref.py, which
tests/test_adamw_ref_host.py pins to oracle/adamw_oracle.py.  Adam's update m / (sqrt(v) + eps) hides a constant factor on
the gradient, so every test here reads the moments: exp_avg is linear in the applied scale, exp_avg_sq quadratic.  The
tests write the fp32 device scalar sum(g^2) themselves and the restatement reads the same value: no reduction order enters.

Bounds, from the fp32 unit roundoff 6e-8: after one step from zero moments rtol 1e-6 on m (<= 8 roundings through the
scale and the product) and 2e-6 on v (<= 16, the square); over several steps also atol 1e-6 * max|g * gs| on m
(b1 m + c1 g can cancel) and its square on v; p: rtol 1e-6 plus atol 1e-5 * lr * bias correction (m / (sqrt(v) + eps) is
O(1) and carries the relative errors of m and v).  Needs a real MI355X."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adamw_ref import adamw_step, bias_correction  # noqa: E402
from clg_vqa_amd import ops  # noqa: E402

DEV = "cuda"
# vl_adamw takes its betas as floats: the kernel tests hand the restatement the values that arrive, fl(0.9) and fl(0.999),
# like the fp32 segment tables and the fp32 sum of squares; the step() test gives the same two values to FusedAdamW and to
# the oracle optimizer.  (With the decimal 0.999 the kernel's 1.f - fl(0.999) is 1.3e-5 below the reference's 0.001f, an
# offset of exp_avg_sq that DESIGN.md states; the bias correction uses the same fl(0.999), so the parameters do not see it.)
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), 1e-6
RTOL_M, RTOL_V, RTOL_P = 1e-6, 2e-6, 1e-6


def _rand(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _dev(vals, dtype=torch.float32):
    return torch.tensor(vals, dtype=dtype, device=DEV)


def _close(name, got, ref, rtol, atol=0.0):
    """|got - ref| <= atol + rtol * |ref| elementwise (atol: number or per-element tensor); NaN only where ref has it."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "%s: NaN pattern differs" % name
    ok = ~torch.isnan(ref)
    err = (got - ref).abs()[ok]
    bound = (torch.as_tensor(atol, dtype=torch.float64) + rtol * ref.abs()).expand_as(ref)[ok]
    worst = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: max err / bound = %.3f  (max abs err %.3e)" % (name, worst, err.max().item() if err.numel() else 0.0))
    assert bool((err <= bound).all()), "%s: error is %.3f x the bound" % (name, worst)


def _p_atol(n, seg_end, seg_lr, lr_mult, step, seg_step=None):
    """1e-5 * (lr * lr_mult * bias correction) of every element's segment."""
    out, lo = torch.zeros(n, dtype=torch.float64), 0
    for i, (hi, lr) in enumerate(zip(seg_end, seg_lr)):
        t = step if seg_step is None else max(int(seg_step[i]), 1)
        out[lo:hi] = 1e-5 * abs(lr) * lr_mult * bias_correction(B1, B2, t)
        lo = hi
    return out


# three segments, both learning rates of the model and one large enough that the decay 1 - lr * wd is not 1.0f
N = 4096
SEG_END, SEG_LR, SEG_WD = [1000, 1004, N], [4e-5, 1e-4, 1e-3], [1e-4, 0.0, 1e-2]
LR_MULT, STEP = 0.75, 3


def _arena(seed=70, zero_grad_values=False):
    p, g = _rand(N, seed), _rand(N, seed + 1)
    if zero_grad_values:
        g.zero_()
    return p, g, torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)


def _launch(p, g, m, v, seg_lr=SEG_LR, step=STEP, **kw):
    ops.adamw(p, g, m, v, _dev(SEG_END, torch.int64), _dev(seg_lr), _dev(SEG_WD), B1, B2, EPS, step, True, LR_MULT, **kw)


def _ref(p, g, m, v, seg_lr=SEG_LR, step=STEP, **kw):
    # the restatement reads the segment tables the kernel reads: the fp32 values
    return adamw_step(p, g, m, v, SEG_END, _dev(seg_lr).cpu(), _dev(SEG_WD).cpu(), B1, B2, EPS, step, True, LR_MULT, **kw)


def _f32(x):
    return float(np.float32(x))


def _sumsq_for(norm_times_post, post):
    """fp32 sum(g^2) for which the kernel's sqrtf(sumsq) * post is `norm_times_post` (post is a power of two)."""
    return _f32((np.float64(norm_times_post) / post) ** 2)


ONE_BELOW, ONE_ABOVE = float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2)))


@pytest.mark.parametrize("post", [1.0, 0.5, 0.125])
@pytest.mark.parametrize("norm", [7.3, 0.2, ONE_BELOW, 1.0, ONE_ABOVE], ids=["clipped", "clamped", "ulp_below", "at", "ulp_above"])
def test_clip_coefficient_reaches_the_moments(norm, post):
    """max_norm = 1: the coefficient well below 1, clamped at 1, and with the norm within one ulp of max_norm, each with
    the 1/world factors 1, 1/2 and 1/8."""
    s = _sumsq_for(norm, post)
    kernel_norm = float(np.sqrt(np.float32(s)) * np.float32(post))  # what the kernel computes, in fp32
    if norm in (ONE_BELOW, 1.0, ONE_ABOVE):
        assert kernel_norm == norm, (kernel_norm, norm)
    p, g, m, v = _arena()
    sumsq = _dev([s])
    rp, rm, rv, gs = _ref(p, g, m, v, sumsq=sumsq.cpu(), max_norm=1.0, post=post)
    expect = min(1.0, 1.0 / (norm + 1e-6)) * post
    assert abs(gs.item() - expect) <= 1e-6 * expect
    _launch(p, g, m, v, sumsq=sumsq, max_norm=1.0, post=post)
    _close("exp_avg", m, rm, RTOL_M)
    _close("exp_avg_sq", v, rv, RTOL_V)
    _close("param", p, rp, RTOL_P, _p_atol(N, SEG_END, SEG_LR, LR_MULT, STEP))
    assert (rm != 0).all() and (rv != 0).all()


def test_zero_gradient_gives_coefficient_one_and_decay_only():
    p, g, m, v = _arena(zero_grad_values=True)
    p0 = p.clone()
    sumsq = _dev([0.0])
    rp, rm, rv, gs = _ref(p, g, m, v, sumsq=sumsq.cpu(), max_norm=1.0, post=0.5)
    assert gs.item() == 0.5  # coefficient 1, times post
    _launch(p, g, m, v, sumsq=sumsq, max_norm=1.0, post=0.5)
    assert (m == 0).all() and (v == 0).all()
    _close("param", p, rp, RTOL_P, _p_atol(N, SEG_END, SEG_LR, LR_MULT, STEP))
    assert torch.equal(p[1000:1004], p0[1000:1004])                        # wd = 0: nothing moves
    assert not torch.equal(p[1004:], p0[1004:]) and (p[1004:].abs() <= p0[1004:].abs()).all()  # decay shrinks


@pytest.mark.parametrize("post", [1.0, 0.5])
def test_no_clipping_max_norm_equals_the_constant_scale_path(post):
    """max_norm = 3.0e38 is what step() passes for "no clipping"; with a norm of 1e-3 the quotient overflows to inf, the
    coefficient is 1 and the bits are those of grad_scale = post."""
    res = []
    for kw in (dict(sumsq=_dev([_sumsq_for(1e-3, post)]), max_norm=3.0e38, post=post), dict(grad_scale=post)):
        p, g, m, v = _arena()
        _launch(p, g, m, v, **kw)
        res.append((p, m, v))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    p, g, m, v = _arena()
    rp, rm, rv, gs = _ref(p, g, m, v, grad_scale=post)
    _close("exp_avg", res[0][1], rm, RTOL_M)
    _close("exp_avg_sq", res[0][2], rv, RTOL_V)


def test_gradient_scale_sources_and_the_next_accumulator():
    gs = 0.37
    res = []
    for kw in (dict(grad_scale=gs), dict(grad_scale_dev=_dev([gs])),
               dict(grad_scale_dev=_dev([gs]), grad_scale=123.0)):  # the device scalar wins over the constant
        p, g, m, v = _arena()
        _launch(p, g, m, v, **kw)
        res.append((p, m, v))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
    p, g, m, v = _arena()
    rp, rm, rv, _ = _ref(p, g, m, v, grad_scale=_f32(gs))
    _close("exp_avg", res[0][1], rm, RTOL_M)
    _close("exp_avg_sq", res[0][2], rv, RTOL_V)
    # with sumsq set, both other sources are ignored
    s = _sumsq_for(7.3, 0.5)
    res = []
    for kw in (dict(), dict(grad_scale_dev=_dev([55.0]), grad_scale=-3.0)):
        p, g, m, v = _arena()
        _launch(p, g, m, v, sumsq=_dev([s]), max_norm=1.0, post=0.5, **kw)
        res.append((p, m, v))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # sumsq_next becomes exactly 0.0 from a NaN fill, sumsq itself is only read; zero_grad clears the active segments only
    p, g, m, v = _arena()
    g0 = g.clone()
    acc = _dev([s, float("nan")])
    _launch(p, g, m, v, seg_lr=[4e-5, -1.0, 1e-3], sumsq=acc[0:1], max_norm=1.0, post=0.5, sumsq_next=acc[1:2], zero_grad=True)
    assert acc[1].item() == 0.0 and math.copysign(1.0, acc[1].item()) == 1.0 and acc[0].item() == s
    assert (g[:1000] == 0).all() and (g[1004:] == 0).all() and torch.equal(g[1000:1004], g0[1000:1004])
    for a, b in zip((p, m, v), res[0]):  # and neither changes the update of the active segments
        assert torch.equal(a[:1000], b[:1000]) and torch.equal(a[1004:], b[1004:])
    # without sumsq_next nothing is written there, without zero_grad the gradient stays
    p, g, m, v = _arena()
    acc = _dev([s, float("nan")])
    _launch(p, g, m, v, sumsq=acc[0:1], max_norm=1.0, post=0.5)
    assert math.isnan(acc[1].item()) and torch.equal(g, g0)


def _moments(seed=80):
    # moments as earlier steps leave them behind: |m| / sqrt(v) is O(1)
    m = _rand(N, seed, 0.01)
    return m, m * m * (0.5 + torch.rand(N, generator=torch.Generator().manual_seed(seed + 1)).to(DEV))


def test_infinite_norm_gives_coefficient_zero():
    p, g, _, _ = _arena()
    m, v = _moments()
    sumsq = _dev([float("inf")])
    rp, rm, rv, gs = _ref(p, g, m, v, sumsq=sumsq.cpu(), max_norm=1.0, post=0.5)
    assert gs.item() == 0.0
    _launch(p, g, m, v, sumsq=sumsq, max_norm=1.0, post=0.5)
    _close("exp_avg", m, rm, RTOL_M)     # b1 * m, (the gradient contributes exact zeros: atol 1e-6 * max|g * gs| = 0)
    _close("exp_avg_sq", v, rv, RTOL_V)
    _close("param", p, rp, RTOL_P, _p_atol(N, SEG_END, SEG_LR, LR_MULT, STEP))


def test_nan_norm_poisons_every_active_segment():
    """torch.clamp(NaN, max=1) is NaN: the reference step turns every parameter that has a gradient into NaN, and a run
    cannot continue unnoticed on partly poisoned weights.  Segments without a gradient are not touched."""
    p, g, _, _ = _arena()
    m, v = _moments()
    g[5] = float("nan")  # where the NaN norm came from
    seg_lr = [4e-5, -1.0, 1e-3]
    before = [t.clone() for t in (p, m, v)]
    sumsq = _dev([float("nan")])
    rp, rm, rv, gs = _ref(p, g, m, v, seg_lr=seg_lr, sumsq=sumsq.cpu(), max_norm=1.0, post=1.0)
    assert math.isnan(gs.item())
    _launch(p, g, m, v, seg_lr=seg_lr, sumsq=sumsq, max_norm=1.0, post=1.0)
    for name, t, r, t0 in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), (rp, rm, rv), before):
        assert torch.isnan(r[:1000]).all() and torch.isnan(r[1004:]).all()
        n_nan = int(torch.isnan(t[:1000]).sum()) + int(torch.isnan(t[1004:]).sum())
        print("%s: %d of %d active elements are NaN" % (name, n_nan, N - 4))
        assert n_nan == N - 4, "%s: %d of %d active elements are NaN" % (name, n_nan, N - 4)
        assert torch.equal(t[1000:1004], t0[1000:1004])


# ---- grid-stride loop, binary search over many segments, flagged table in the middle of the arena ----------------------
BIG_N = 3_145_728                 # 1.5 x the grid cap of 2048 workgroups x 256 float4
CAP_ELEMS = 2048 * 256 * 4
ROWS, ROW_LEN, TABLE_AT = 4096, 64, 400_004
LONG_END = CAP_ELEMS + 900_000


def _big_layout():
    """301 segments: the flagged table, a segment that ends exactly at float4 index 524 288, a very long one behind it,
    several of length 4, the rest uneven."""
    rng = np.random.RandomState(7)
    table_end = TABLE_AT + ROWS * ROW_LEN
    cuts = {TABLE_AT, table_end, CAP_ELEMS, LONG_END, 1000, 1004, 1008, 3_000_000, 3_000_004, BIG_N - 4}
    regions = [(4, TABLE_AT), (table_end + 4, CAP_ELEMS), (LONG_END + 4, BIG_N - 4)]
    while len(cuts) < 300:
        lo, hi = regions[rng.randint(len(regions))]
        cuts.add(int(rng.randint(lo // 4, hi // 4)) * 4)
    ends = sorted(cuts) + [BIG_N]
    begins = [0] + ends[:-1]
    lens = [e - b for b, e in zip(begins, ends)]
    assert len(ends) == 301 and all(x > 0 and x % 4 == 0 for x in lens)
    assert sum(1 for x in lens if x == 4) >= 4 and max(lens) == LONG_END - CAP_ELEMS and CAP_ELEMS // 4 == 524_288
    ti = begins.index(TABLE_AT)
    assert ends[ti] == table_end and 0 < ti < 300
    lr = rng.choice([4e-5, 1e-4, 1e-3], size=301)
    wd = rng.choice([0.0, 1e-4, 1e-2], size=301)
    lr[rng.rand(301) < 0.1] = -1.0
    steps = rng.randint(1, 10, size=301)
    lr[ti], wd[ti] = 1e-3, 1e-2    # 1 - lr * wd = 1 - 1e-5 is not 1.0f: the decay-only branch does real work
    li = begins.index(CAP_ELEMS)
    lr[li] = 1e-4
    lr[li - 1] = 4e-5              # the segment that ends at the grid cap is active as well
    assert np.float32(1) - np.float32(1e-3) * np.float32(1e-2) != np.float32(1)
    assert 20 <= int((lr < 0).sum()) <= 45
    return begins, ends, [float(x) for x in lr], [float(x) for x in wd], [int(x) for x in steps], ti


def test_grid_stride_many_segments_and_a_flagged_table_in_the_middle():
    begins, ends, lr, wd, steps, ti = _big_layout()
    gen = torch.Generator().manual_seed(90)
    p0, g = torch.randn(BIG_N, generator=gen), torch.randn(BIG_N, generator=gen)
    flags = (torch.rand(ROWS, generator=gen) < 1.0 / 3.0).to(torch.uint8)
    assert 1200 < int(flags.sum()) < 1530
    g[TABLE_AT:TABLE_AT + ROWS * ROW_LEN].view(ROWS, ROW_LEN)[flags == 0] = 0.0  # untouched rows: g = m = v = 0
    seg_end, seg_lr, seg_wd = _dev(ends, torch.int64), _dev(lr), _dev(wd)
    lr32 = seg_lr.cpu()
    fl = dict(row_flags=flags.to(DEV), flag_begin=TABLE_AT, flag_rows=ROWS, flag_row_len=ROW_LEN)
    post, max_norm, lr_mult = 0.5, 1.0, 0.6
    # the clip acts: the norm of the averaged gradient is ~ 850 and ~ 1200
    sums = [_f32((g.double() ** 2).sum().item()), _f32(2.0 * (g.double() ** 2).sum().item())]
    results = {}
    for mode in ("flagged", "dense"):
        p, m, v = p0.to(DEV), torch.zeros(BIG_N, device=DEV), torch.zeros(BIG_N, device=DEV)
        gd = g.to(DEV)
        rp, rm, rv = p0.double(), torch.zeros(BIG_N, dtype=torch.float64), torch.zeros(BIG_N, dtype=torch.float64)
        st = list(steps)
        for k, s in enumerate(sums):
            st = [t + 1 if l >= 0 else t for t, l in zip(st, lr)] if k else st
            kw = dict(sumsq=_dev([s]), max_norm=max_norm, post=post)
            ops.adamw(p, gd, m, v, seg_end, seg_lr, seg_wd, B1, B2, EPS, 9 + k, True, lr_mult,
                      seg_step=_dev(st, torch.int64), **kw, **(fl if mode == "flagged" else {}))
            if mode == "dense":
                continue
            rp, rm, rv, gs = adamw_step(rp, g, rm, rv, ends, lr32, seg_wd.cpu(), B1, B2, EPS, 9 + k, True, lr_mult,
                                        sumsq=torch.tensor([s]), max_norm=max_norm, post=post, seg_step=st,
                                        row_flags=flags, flag_begin=TABLE_AT, flag_rows=ROWS, flag_row_len=ROW_LEN)
            assert gs.item() < 0.01 * post
            amax = (g.double() * gs).abs().max().item()
            _close("step %d exp_avg" % (k + 1), m, rm, RTOL_M, 1e-6 * amax if k else 0.0)
            _close("step %d exp_avg_sq" % (k + 1), v, rv, RTOL_V, (1e-6 * amax) ** 2 if k else 0.0)
            _close("step %d param" % (k + 1), p, rp, RTOL_P, _p_atol(BIG_N, ends, lr, lr_mult, 9 + k, st))
        results[mode] = (p, m, v)
        assert torch.equal(gd.cpu(), g)  # zero_grad was not asked for
    # skipped segments are untouched, the unflagged rows only decayed
    p, m, v = (t.cpu() for t in results["flagged"])
    for b, e, l in zip(begins, ends, lr):
        if l < 0:
            assert torch.equal(p[b:e], p0[b:e]) and not m[b:e].any() and not v[b:e].any()
    rows_p = p[TABLE_AT:TABLE_AT + ROWS * ROW_LEN].view(ROWS, ROW_LEN)
    rows_0 = p0[TABLE_AT:TABLE_AT + ROWS * ROW_LEN].view(ROWS, ROW_LEN)
    assert not torch.equal(rows_p[flags == 0], rows_0[flags == 0])
    # the flagged form is the dense update, bit for bit
    for a, b in zip(results["flagged"], results["dense"]):
        assert torch.equal(a, b)


# ---- FusedAdamW.step() on a plain module (no engine): its own sum of squares, schedule, per-segment step counts ---------
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.dense = torch.nn.Linear(139, 263)
        self.LayerNorm = torch.nn.LayerNorm(263)
        self.vil_prediction = torch.nn.Linear(263, 101)
        self.embeddings = torch.nn.Embedding(37, 139)
        self.vil_logit = torch.nn.Linear(101, 1)
        self.scale = torch.nn.Parameter(torch.randn(3, 5, 7))


def test_fused_step_follows_the_oracle_optimizer_moment_by_moment():
    from clg_vqa_amd.optim import FusedAdamW
    from oracle.adamw_oracle import ReferenceAdamW
    torch.manual_seed(21)
    cpu = _Tiny()
    dev = copy.deepcopy(cpu).to(DEV)
    names = [n for n, _ in cpu.named_parameters()]
    assert len(names) == 10 and 65_000 < sum(p.numel() for p in cpu.parameters()) < 75_000
    assert any(p.numel() % 4 for p in cpu.parameters())
    base_lr, wd, max_norm = 4e-5, 1e-2, 1.0
    kw = dict(base_lr=base_lr, weight_decay=wd, betas=(B1, B2), eps=EPS, correct_bias=True, max_grad_norm=max_norm,
              warmup_steps=1, t_total=10)
    ref = ReferenceAdamW(list(cpu.named_parameters()), **kw)
    opt = FusedAdamW(dev, **kw)
    opt.return_norm = True
    assert {g["lr"] for g in ref.groups} == {base_lr, 1e-4} and {g["wd"] for g in ref.groups} == {0.0, wd}
    assert [g[0] for g in opt.groups] == [g["name"] for g in ref.groups] == names
    late = names.index("scale")
    gen = torch.Generator().manual_seed(22)
    clipped = []
    for step, gscale in enumerate((1e-2, 1e-4, 1e-2, 1e-3), 1):  # gradient norms ~ 2.6, 0.026, 2.6, 0.26 around max_norm = 1
        grads = []
        for i, (pc, pd) in enumerate(zip(cpu.parameters(), dev.parameters())):
            if i == late and step == 1:
                grads.append(None)
                continue  # this parameter joins at step 2: its own step count from then on
            gr = torch.randn(pc.shape, generator=gen) * gscale
            pc.grad, pd.grad = gr.clone(), gr.to(DEV)
            grads.append(gr)
        lr_mult = opt.lr_mult()
        norm_ref = ref.step()
        norm = opt.step()
        torch.cuda.synchronize()
        torch.testing.assert_close(norm.cpu().view(()), norm_ref.view(()), rtol=1e-5, atol=0.0)
        clipped.append(norm.item() > max_norm)
        gs = min(1.0, max_norm / (norm_ref.item() + 1e-6))
        assert (opt._seg_step_dev is not None) == (step >= 2)
        for i, (grp, off, gr) in enumerate(zip(ref.groups, opt.arena.offsets, grads)):
            n = grp["p"].numel()
            amax = 0.0 if gr is None else gr.abs().max().item() * gs
            where = "step %d %s " % (step, grp["name"])
            _close(where + "exp_avg", opt.exp_avg[off:off + n], grp["m"].view(-1), RTOL_M + 1e-5, 1e-6 * amax)
            _close(where + "exp_avg_sq", opt.exp_avg_sq[off:off + n], grp["v"].view(-1), RTOL_V + 1e-5, (1e-6 * amax) ** 2)
            t = max(grp["step"], 1)
            _close(where + "param", opt.arena.param[off:off + n], grp["p"].detach().view(-1), RTOL_P,
                   1e-5 * grp["lr"] * lr_mult * bias_correction(B1, B2, t))
            assert opt.seg_steps[i] == grp["step"]
        assert not opt.arena.grad.any()
        assert all(p.grad is None for p in dev.parameters())
        # the two accumulators alternate: the one of the next step reads 0.0, the one just used holds this step's sum
        assert opt._sumsq[opt.opt_step % 2].item() == 0.0
        torch.testing.assert_close(opt._sumsq[(opt.opt_step - 1) % 2].sqrt().cpu(), norm.cpu().view(()), rtol=1e-6, atol=0.0)
    assert clipped == [True, False, True, False]
    assert ref.groups[late]["step"] == 3 and opt.opt_step == 4
