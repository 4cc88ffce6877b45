"""One comparison for every gradient that is held against an oracle: per tensor AND per row, column, element and scale.

The backward pass runs single-pass bf16 products, so every gradient tensor carries 0.5-1.2 % of honest rounding noise and the
whole-tensor bound has to be 4e-2.  A whole-tensor norm at that bound cannot see a zeroed row or column of a 768-wide weight
gradient (1 / sqrt(768) = 3.6e-2), one wrong element of a bias gradient, or a 2 % scale error -- the shapes a ragged tile, a
dropped column-sum partial, a row map off by one or a wrong 1 / (1 - p) take.  The statistics below separate them from the
noise.  Tensors with two or more dims are viewed as [prod(shape[:-1]), shape[-1]]; everything is float64 on the CPU.

    tensor    ||g - r|| / ||r||
    scale     |<g, r> / <r, r> - 1|
    row       max_i ||(g - r)[i, :]|| / max(||r[i, :]||, ||r|| / sqrt(nrows))          2-D views
    column    the same over columns                                                      2-D views
    element   max_j |g_j - r_j| / max(|r_j|, ||r|| / sqrt(n))                           1-D tensors

The floor at the typical slice norm keeps slices that are exactly zero on both sides (untouched embedding rows, SFT-masked
entries) at 0 and stops a tiny reference slice from inflating the ratio.  0 / 0 counts as 0, x / 0 as infinity, a NaN fails.

Where the bounds come from: `python tests/precision_study.py --slices` (the reference-side noise model: the oracle with the
engine's rounding points restated -- 3-term bf16 forward incl. the attention core; bf16 operands of every backward product, which
is where dctx, P, dS and the LayerNorm backward's bf16 output enter; GELU' kept as bf16 and multiplied into a bf16 result), the
worst value of each statistic over all parameter gradients and both input gradients at (layers, B, T, V) in {(2,8,20,36), (2,3,7,9), (2,2,20,100), (2,1,6,4), (12,8,20,36)} and the
c1 config, two seeds each, times a margin, rounded to one significant digit (DESIGN.md section 5 quotes the output):

    statistic   worst of the noise model                                              margin   bound
    tensor      9.90e-03  c1, spatials.grad                                           -        4e-2 (the existing bound)
    scale       4.72e-03  12 layers, layer.2.attention_self.query.bias               3x       1e-2 (a 2 % scale error: 2e-2)
    row         4.57e-02  12 layers, layer.20.attention_self.query.weight[653]       4x       2e-1 (a zeroed row: 0.46-1)
    column      2.28e-02  (2,1,6,4), features.grad[158]                               4x       9e-2 (a zeroed column: ~1)
    element     4.69e-02  (2,2,20,100), embeddings.image_layer_norm.weight[674]      4x       2e-1 (a wrong element: >= 1)

The engine's own measured figures never set or widen a bound."""
import math

import torch

GRAD_REL_L2 = 4e-2   # per tensor: the bound every oracle gradient comparison of the suite has used
GRAD_SCALE = 1e-2
GRAD_ROW = 2e-1
GRAD_COLUMN = 9e-2
GRAD_ELEMENT = 2e-1
BOUNDS = dict(tensor=GRAD_REL_L2, scale=GRAD_SCALE, row=GRAD_ROW, column=GRAD_COLUMN, element=GRAD_ELEMENT)
ZERO_GRAD_ABS = 1e-2  # key biases: |g| against the query bias's gradient norm (softmax is shift invariant: dL / d key.bias = 0)
STATS = ("tensor", "scale", "row", "column", "element")


def _f64(t):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    return t.detach().to("cpu", torch.float64)


def _ratio(num, den):
    """num / den elementwise with 0 / 0 = 0 and x / 0 = inf (NaN stays NaN)."""
    out = num / den
    zero = den == 0
    if zero.any():
        out = torch.where(zero, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)), out)
    return out


def _worst(x):
    """(max, its index), a NaN winning over everything."""
    bad = torch.isnan(x)
    if bad.any():
        return math.nan, int(bad.nonzero()[0])
    i = int(x.argmax())
    return float(x[i]), i


def old_rel_l2(got, ref):
    """The per-tensor formula the suite used before (kept so that tests can show what it lets through)."""
    g, r = _f64(got), _f64(ref)
    return (g - r).norm().item() / max(r.norm().item(), 1e-12)


def grad_stats(got, ref):
    """The five statistics of `got` against `ref` (statistics that do not apply to the tensor's rank are 0.0) and, under
    "where", for row / column / element the index of the worst slice with both slice norms."""
    g, r = _f64(got), _f64(ref)
    assert g.shape == r.shape, "shapes differ: %s vs %s" % (tuple(g.shape), tuple(r.shape))
    assert g.numel() > 0
    d = g - r
    rn = r.norm()
    out = dict(tensor=float(_ratio(d.norm(), rn)), scale=0.0, row=0.0, column=0.0, element=0.0, where={})
    rr = float((r * r).sum())
    out["scale"] = abs(float((g * r).sum()) / rr - 1.0) if rr > 0 else (0.0 if not g.any() else math.inf)
    if bool(torch.isnan(g).any()):
        out["scale"] = math.nan
    if g.dim() >= 2:
        g2, r2, d2 = (t.reshape(-1, t.shape[-1]) for t in (g, r, d))
        for name, dim in (("row", 1), ("column", 0)):
            rs = r2.norm(dim=dim)
            floor = rn / math.sqrt(rs.numel())
            val, i = _worst(_ratio(d2.norm(dim=dim), torch.clamp(rs, min=float(floor))))
            out[name] = val
            out["where"][name] = (i, float(g2.norm(dim=dim)[i]), float(rs[i]))
    else:
        g1, r1, d1 = g.reshape(-1), r.reshape(-1), d.reshape(-1)
        floor = rn / math.sqrt(r1.numel())
        val, i = _worst(_ratio(d1.abs(), torch.clamp(r1.abs(), min=float(floor))))
        out["element"] = val
        out["where"]["element"] = (i, float(g1[i].abs()), float(r1[i].abs()))
    return out


def violations(stats, bounds=None):
    """[(statistic, value, bound)] of the statistics that exceed their bound (a NaN exceeds every bound)."""
    b = dict(BOUNDS)
    if bounds:
        assert set(bounds) <= set(BOUNDS), sorted(set(bounds) - set(BOUNDS))
        b.update(bounds)
    return [(k, stats[k], b[k]) for k in STATS if not stats[k] <= b[k]]


def within(stats, bounds=None):
    return not violations(stats, bounds)


def grad_check(name, got, ref, bounds=None):
    """Assert all five statistics of one tensor; returns them.  `bounds` replaces constants (a tighter per-tensor bound,
    the kernel-level bounds of the attention backward); there is no way to leave slices out."""
    st = grad_stats(got, ref)
    bad = violations(st, bounds)
    if bad:
        k, v, b = bad[0]
        w = st["where"].get(k)
        at = " at %s %d (slice norm %.3e, reference %.3e)" % ((k,) + w) if w else ""
        rn = _f64(ref).norm().item()
        raise AssertionError("%s: %s statistic %.3e exceeds %.1e%s; tensor %s, reference norm %.3e; all: %s" % (
            name, k, v, b, at, tuple(_f64(ref).shape), rn, fmt(st)))
    return st


def fmt(st):
    return " ".join("%s %.2e" % (k, st[k]) for k in STATS)


def is_zero_grad_name(n):
    """Parameters whose gradient is mathematically zero: the key bias of an attention (UC2 / M3P names)."""
    return n.endswith("attention_self.key.bias") or n.endswith("k_lin.bias")


def _query_name(n):
    return n.replace("key.bias", "query.bias") if n.endswith("key.bias") else n.replace("k_lin.bias", "q_lin.bias")


class Worst(dict):
    """{statistic: (value, tensor name)} of the worst value seen."""

    def __init__(self):
        super().__init__((k, (0.0, None)) for k in STATS)

    def add(self, name, st):
        for k in STATS:
            if not st[k] <= self[k][0]:
                self[k] = (st[k], name)

    def __str__(self):
        return "worst " + ", ".join("%s %.2e at %s" % (k, self[k][0], self[k][1]) for k in STATS if self[k][1] is not None)


def check_grads(got, ref, what="", bounds=None, check=True):
    """Every tensor of the dict `got` against `ref[name]`.  Key biases (mathematically zero) are held to ZERO_GRAD_ABS of the
    query bias's reference gradient norm instead.  With check=False nothing is asserted (negative controls read the result).
    Returns a Worst."""
    worst = Worst()
    assert got, what
    for n, g in got.items():
        assert g is not None, "%s %s: no gradient" % (what, n)
        if is_zero_grad_name(n):
            qn = _f64(ref[_query_name(n)]).norm().item()
            gn = _f64(g).norm().item()
            if check:
                assert gn <= ZERO_GRAD_ABS * qn, "%s %s: |g| %.3e against |d query bias| %.3e" % (what, n, gn, qn)
            continue
        st = grad_check((what + " " + n).strip(), g, ref[n], bounds) if check else grad_stats(g, ref[n])
        worst.add(n, st)
    return worst
