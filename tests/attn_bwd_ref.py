"""The attention backward restated in float64 with the kernel's rounding points, and the per-block / per-row bounds the kernel
tests (tests/test_gpu_kernels.py, tests/test_gpu_dropout.py) hold `vl_attn2_bwd` to.

attention2.hip's backward reads the bf16 halves of q, k, v, a bf16 dO and the forward's lse, and feeds the matrix pipe with
    P  = exp(s - lse),  s from the single-pass bf16 product of the hi halves, lse from the forward's 3-term product
    Pd = bf16(P * keep)                                                                          dV = Pd^T dO
    dS = bf16(P * (keep * dP - delta) * scale),  dP = dO V^T,  delta = rowsum(P * keep * dP)     dQ = dS K,  dK = dS^T Q
and stores dqkv as bf16.  `attn_bwd_restated(..., rounded=False)` is plain autograd of softmax attention (a CPU test holds it
to torch's autograd).  With rounded=True, P and dS are rounded as above, and with `lse` given P is taken against that lse
instead of its own row sum: the reference of the kernel tests.  out_bf16=True also rounds the result as the kernel's store does.

The lse point is the large one.  The scores of the hi halves differ from the forward's by ~2^-9 |s| per key, so a row of the
recomputed P is off by a common factor exp(lse(hi) - lse(hi + lo)) (up to 2e-2 at the tests' operand scale of 1.5) and no longer
sums to 1.  Where a row's softmax is peaked, dS = P (dP - delta) is a difference of nearly equal numbers and that factor does
not cancel: rows of dQ come out up to 5-9 % of the typical row norm off (13 % of their own, small, norm), while rounding P and dS
alone moves a row by 5e-3.  Found by the per-row check on the MI355X, reproduced on the CPU by this restatement.

Bounds.  The kernel is compared with the restatement that has the same lse, P and dS points (not the store rounding).  The lse
point is deterministic and shared by both sides; what may still differ is rounding: bf16 ties of P / dS, the bf16 store, fp32
accumulation.  So the bound is, per case, ATTN_MARGIN (4) x the deviation that the P / dS / store rounding alone gives the
restatement against the unrounded autograd at the same bf16-rounded operands and the case's own inputs -- computed on the CPU in
float64 by `deviation()` -- for the relative L2 error of a (q / k / v, head) block viewed [B S, dh] (deviation 2.4-3.3e-3) and for
the row statistic of grad_check within a block (3.7-5.1e-3).  With the lse point the restatement itself deviates 4-11e-3 per
block and 2-16e-2 per row (S = 2: 0.25 / 0.5); a bound from that would be no tighter than the whole-tensor 2e-2 and is not used.
`python tests/attn_bwd_ref.py` prints both deviations of every case.  Measured on the MI355X: block <= 2.1e-3, row <= 6.0e-3.
"""
import math

import torch

BF16 = torch.bfloat16
ATTN_MARGIN = 4.0

# the attention backward cases of the kernel tests: (B, T, V) at 12 heads of 64 / (B, S) at 4 heads of 32
FWD_BWD_CASES = [(3, 20, 36), (2, 40, 36), (2, 20, 100), (2, 40, 100), (1, 13, 20), (1, 60, 100), (2, 1, 1), (1, 30, 50)]
DH32_CASES = [(3, 56), (2, 120), (1, 10), (2, 140), (1, 156)]
# both sides of the S thresholds between kernel instances (64 / 80 / 128 / 144), which the lists above lack: (B, S, dh)
EDGE_CASES = [(2, 64, 64), (2, 65, 64), (1, 81, 64), (2, 128, 64), (2, 129, 64), (1, 144, 64), (2, 145, 64), (2, 65, 32),
              (2, 129, 32)]
DROPOUT_CASES = [(2, 56, 64, False), (2, 120, 64, False), (1, 160, 64, False), (2, 140, 32, False), (3, 16, 32, False),
                 (2, 56, 64, True), (2, 140, 64, True)]


def _bf(x, on):
    return x.to(BF16).to(x.dtype) if on else x


def _heads(x, B, S, nh, dh):
    return [t.view(B, S, nh, dh).permute(0, 2, 1, 3) for t in x.view(B, S, 3 * nh * dh).split(nh * dh, dim=-1)]


def lse_of(qkv, addmask, B, S, nh, dh):
    """[B, nh, S, 1] log-sum-exp of the masked, scaled scores of qkv (float64): what the forward saves, at its operands."""
    q, k, _ = _heads(qkv.double(), B, S, nh, dh)
    return torch.logsumexp(q @ k.transpose(-1, -2) / math.sqrt(dh) + addmask.double().view(B, 1, 1, S), dim=-1, keepdim=True)


def attn_bwd_restated(qkv, addmask, dO, B, S, nh, dh, keep=None, nq1=False, rounded=True, out_bf16=False, lse=None):
    """qkv [B S, 3 H] (the bf16-rounded operands as float64), addmask [B, S] additive key mask, dO [B S, H] (or [B, H] with
    nq1: only query row 0 of every sample is live), keep [B, nh, S, S] keep-scales (0 or 1 / (1 - p)) or None, lse [B, nh, S, 1]
    (lse_of the forward's operands) or None = the scores' own.  Returns dqkv [B S, 3 H] float64."""
    H = nh * dh
    qkv = qkv.double()
    q, k, v = _heads(qkv, B, S, nh, dh)
    scale = 1.0 / math.sqrt(dh)
    if nq1:
        full = torch.zeros(B, S, H, dtype=torch.float64, device=qkv.device)
        full[:, 0] = dO.double().view(B, H)
        dO = full
    do = dO.double().view(B, S, nh, dh).permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) * scale + addmask.double().view(B, 1, 1, S)
    p = torch.softmax(s, dim=-1) if lse is None else torch.exp(s - lse.double())
    kp = torch.ones_like(p) if keep is None else keep.double()
    pd = p * kp
    dv = _bf(pd, rounded).transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    delta = (pd * dp).sum(-1, keepdim=True)
    ds = _bf(p * (kp * dp - delta) * scale, rounded)
    dq, dk = ds @ k, ds.transpose(-1, -2) @ q
    out = torch.cat([t.permute(0, 2, 1, 3).reshape(B * S, H) for t in (dq, dk, dv)], dim=-1)
    return _bf(out, out_bf16)


def blocks(dqkv, B, S, nh, dh):
    """[(name, [B S, dh] view)] of the 3 nh column blocks of a dqkv [B S, 3 H]."""
    H = nh * dh
    return [("d%s head %d" % ("qkv"[i], h), dqkv[:, i * H + h * dh:i * H + (h + 1) * dh]) for i in range(3) for h in range(nh)]


def _block_stats(got, ref, B, S, nh, dh):
    import grad_check as G
    return [(bn, G.grad_stats(g, r)) for (bn, g), (_, r) in zip(blocks(got, B, S, nh, dh), blocks(ref, B, S, nh, dh))]


def deviation(hi, lo, addmask, d16, B, S, nh, dh, keep=None, nq1=False):
    """((worst block rel-L2, worst row statistic) of the restatement with the P / dS / store rounding against the unrounded
    autograd, the same with the lse point added, the restatement the kernel is compared with).  hi, lo: the bf16 halves the
    kernels read (any float dtype), d16: the bf16 dO."""
    h64, d64 = hi.double(), d16.double()
    lse = lse_of(h64 + lo.double(), addmask, B, S, nh, dh)
    exact = attn_bwd_restated(h64, addmask, d64, B, S, nh, dh, keep, nq1, rounded=False)
    ref = attn_bwd_restated(h64, addmask, d64, B, S, nh, dh, keep, nq1, lse=lse)
    out = []
    for noisy in (attn_bwd_restated(h64, addmask, d64, B, S, nh, dh, keep, nq1, out_bf16=True), _bf(ref, True)):
        stats = _block_stats(noisy, exact, B, S, nh, dh)
        out.append((max(st["tensor"] for _, st in stats), max(st["row"] for _, st in stats)))
    return out[0], out[1], ref


def check_blocks(name, dqkv, hi, lo, addmask, d16, B, S, nh, dh, keep=None, nq1=False):
    """grad_check of every (q / k / v, head) block of the kernel's dqkv -- the block as a whole and every sequence row of it
    -- against the restatement with the kernel's lse / P / dS points, within ATTN_MARGIN x the rounding deviation (see the
    module's docstring) on these inputs.  Prints before it asserts.  Returns the worst (block rel-L2, row statistic)."""
    import grad_check as G
    dev, with_lse, ref = deviation(hi, lo, addmask, d16, B, S, nh, dh, keep, nq1)
    bounds = dict(tensor=ATTN_MARGIN * dev[0], row=ATTN_MARGIN * dev[1])
    stats = _block_stats(dqkv, ref, B, S, nh, dh)
    worst = (max(st["tensor"] for _, st in stats), max(st["row"] for _, st in stats))
    print("%s: worst (q / k / v, head) block rel-L2 %.3e (bound %.3e = 4 x the rounding deviation; with the lse point the "
          "restatement deviates %.3e), worst row of a block %.3e (bound %.3e; %.3e)" % (
              name, worst[0], bounds["tensor"], with_lse[0], worst[1], bounds["row"], with_lse[1]))
    for (bn, g), (_, r) in zip(blocks(dqkv, B, S, nh, dh), blocks(ref, B, S, nh, dh)):
        G.grad_check("%s %s" % (name, bn), g, r, bounds=bounds)
    return worst


def case_inputs(B, S, nh, dh, seed, mask_kind, p=0.0, nq1=False, device="cpu"):
    """Host-side inputs of a case: (qkv fp32 [B S, 3 H], dO fp32, additive mask [B, S]).  mask_kind: "text" = five padded
    tokens in sample 0 (as in test_attention2_forward_backward), "tail0" = the last two keys of sample 0
    (test_attention2_head_dim_32), "edge" = a padded key tail in the LAST sample plus region positions in the middle of the
    sequence of sample 0 (test_attention2_dispatch_edges takes its inputs from here), "dropout" = the masks of
    test_attention_dropout_values_against_fp64."""
    g = torch.Generator().manual_seed(seed)
    H = nh * dh
    qkv = torch.randn(B * S, 3 * H, generator=g) * 1.5
    dO = torch.randn(B if nq1 else B * S, H, generator=torch.Generator().manual_seed(seed + 1))
    m = torch.ones(B, S)
    if mask_kind == "text" and S > 26:
        m[0, 15:20] = 0
    elif mask_kind == "tail0":
        m[0, S - 2:] = 0
    elif mask_kind == "edge":
        m[-1, S - 7:] = 0
        m[0, S // 2 - 3:S // 2 + 2] = 0
    elif mask_kind == "dropout":
        m[0, S - 5:] = 0
        m[-1, 3:6] = 0
    return qkv.to(device), dO.to(device), ((1 - m) * -10000.0).to(device)


def all_cases():
    cases = [(B, T + V, 12, 64, "text", 0.0, False) for B, T, V in FWD_BWD_CASES]
    cases += [(B, S, 4, 32, "tail0", 0.0, False) for B, S in DH32_CASES]
    cases += [(B, S, 4, dh, "edge", 0.0, False) for B, S, dh in EDGE_CASES]
    return cases + [(B, S, 4, dh, "dropout", 0.1, nq1) for B, S, dh, nq1 in DROPOUT_CASES]


def case_deviation(i, case):
    """deviation() of a case at host-made inputs (a Bernoulli keep mask stands in for the engine's at the dropout cases) and the
    same with the P / dS / store rounding alone, i.e. without the lse point."""
    B, S, nh, dh, kind, p, nq1 = case
    qkv, dO, addmask = case_inputs(B, S, nh, dh, 100 + i, kind, p, nq1)
    hi = qkv.to(BF16)
    lo = (qkv - hi.float()).to(BF16)
    keep = (torch.rand(B, nh, S, S, generator=torch.Generator().manual_seed(i)) >= p).double() / (1 - p) if p else None
    plain, dev, _ = deviation(hi, lo, addmask, dO.to(BF16), B, S, nh, dh, keep, nq1)
    return dev, plain


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    print("| B | S | heads x dh | p | nq | block rel-L2: P, dS, store | + lse | row: P, dS, store | + lse |")
    print("|---|---|---|---|---|---|---|---|---|")
    for i, c in enumerate(all_cases()):
        dev, plain = case_deviation(i, c)
        print("| %d | %d | %d x %d | %.1f | %s | %.2e | %.2e | %.2e | %.2e |" % (
            c[0], c[1], c[2], c[3], c[5], "1" if c[6] else "S", plain[0], dev[0], plain[1], dev[1]))
