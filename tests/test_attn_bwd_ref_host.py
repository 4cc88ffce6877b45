"""tests/attn_bwd_ref.py on the CPU: the restatement without rounding is torch's float64 autograd of softmax attention (with
and without a keep mask, all query rows and query row 0 only); giving it the scores' own lse changes nothing; the forward's lse
is the largest of the restated rounding points, as measured on the kernel."""
import math

import pytest
import torch

import attn_bwd_ref as A


@pytest.mark.parametrize("B,S,nh,dh,p,nq1", [(2, 13, 3, 32, 0.0, False), (2, 21, 2, 64, 0.1, False), (3, 9, 2, 32, 0.1, True)])
def test_unrounded_restatement_is_autograd(B, S, nh, dh, p, nq1):
    H = nh * dh
    qkv, dO, addmask = A.case_inputs(B, S, nh, dh, 5, "edge", p, nq1)
    keep = (torch.rand(B, nh, S, S, generator=torch.Generator().manual_seed(1)) >= p).double() / (1 - p) if p else None
    x = qkv.double().requires_grad_(True)
    q, k, v = [t.view(B, S, nh, dh).permute(0, 2, 1, 3) for t in x.view(B, S, 3 * H).split(H, dim=-1)]
    pr = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh) + addmask.double().view(B, 1, 1, S), dim=-1)
    ctx = ((pr * keep if p else pr) @ v).permute(0, 2, 1, 3).reshape(B, S, H)
    (ctx[:, 0] if nq1 else ctx.reshape(B * S, H)).backward(dO.double())
    got = A.attn_bwd_restated(qkv.double(), addmask, dO, B, S, nh, dh, keep, nq1, rounded=False)
    torch.testing.assert_close(got, x.grad, rtol=1e-11, atol=1e-12)
    assert (got[:, :H].view(B, S, H)[:, 1:] == 0).all() == nq1  # dQ of the dead query rows
    noisy = A.attn_bwd_restated(qkv.double(), addmask, dO, B, S, nh, dh, keep, nq1, rounded=True)
    rel = (noisy - got).norm().item() / got.norm().item()
    assert 1e-4 < rel < 1e-2, rel  # the rounding is there and is bf16-sized


def test_own_lse_changes_nothing_and_the_forwards_lse_is_the_large_point():
    """B = 2, S = 120, 12 heads of 64 (a case of test_attention2_forward_backward)."""
    case = A.all_cases()[2]
    B, S, nh, dh = case[:4]
    assert (B, S, nh, dh) == (2, 120, 12, 64)
    qkv, dO, addmask = A.case_inputs(B, S, nh, dh, 102, "text")
    hi = qkv.to(A.BF16).double()
    a = A.attn_bwd_restated(hi, addmask, dO.double(), B, S, nh, dh)
    b = A.attn_bwd_restated(hi, addmask, dO.double(), B, S, nh, dh, lse=A.lse_of(hi, addmask, B, S, nh, dh))
    assert (a - b).norm().item() <= 1e-5 * a.norm().item()  # only bf16 ties of P / dS can move
    dev, plain = A.case_deviation(2, case)
    print("block rel-L2 %.2e -> %.2e, row %.2e -> %.2e with the forward's lse" % (plain[0], dev[0], plain[1], dev[1]))
    assert 1e-3 < plain[0] < 5e-3 and 2e-3 < plain[1] < 1e-2   # P, dS and the bf16 store: 2^-9 each
    assert dev[0] > 1.2 * plain[0] and dev[1] > 3 * plain[1]    # the lse point dominates the rows
    assert dev[0] < 2e-2                                        # and still sits inside the whole-tensor bound of the kernel tests
