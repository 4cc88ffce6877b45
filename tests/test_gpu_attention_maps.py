"""Per-layer hidden states and attention maps of the UC2 trunk on the MI355X: the emitting attention kernel
(vl_attn2_fwd_probs) against fp64 math, the stack's taps and the model surface (output_all_encoded_layers /
output_all_attention_masks) against the real reference's fixture and the hook-based oracle helper."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_maps_ref as AR  # noqa: E402
import dropout_masks as DM  # noqa: E402
from helpers import TASK_CFG, golden_config, load_golden, uc2_cfg_dict  # noqa: E402
from oracle import uc2_oracle as O  # noqa: E402
from clg_vqa_amd import _lib, ops  # noqa: E402
from clg_vqa_amd.config import BertConfig  # noqa: E402
from clg_vqa_amd.encoders import BertForVLTasks  # noqa: E402
from clg_vqa_amd.ops import BF16  # noqa: E402
from clg_vqa_amd.synthetic import make_batch, seeded_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOGIT_TOL = 1e-3  # the project's forward contract (tests/test_gpu_model.py); all tensors compared here are O(1)
P_TOL = 3e-5      # the bound test_gpu_kernels.py holds ctx to against fp64; P <= 1
GUARD, SENTINEL = 1024, -7.0
BASE_SEED = 0x5EED ^ 20261016
MAP_KEYS = ("intra_attn", "inter_attn", "queries", "keys")


# ---------------------------------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------------------------------
def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _kernel_case(B, S, nh, dh, seed):
    H = nh * dh
    qkv = _rand(B * S, 3 * H, seed=seed)
    hi, lo = torch.empty_like(qkv, dtype=BF16), torch.empty_like(qkv, dtype=BF16)
    ops.split_f32(qkv.contiguous(), hi, lo)
    mask = torch.zeros(B, S)
    n = max(1, S // 8)
    mask[0, S - n:] = -10000.0                       # sample 0: a tail of padded keys the UC2 way ...
    if S - 2 * n >= 1:
        mask[0, S - 2 * n:S - n] = -float("inf")     # ... and a block masked the M3P way before it
    if B > 1:
        mask[1, 1] = -float("inf")
        if S > 2:
            mask[1, S - 1] = -10000.0
    return hi, lo, mask.reshape(-1).contiguous().to(DEV)


def _softmax64(hi, lo, addmask, B, S, nh, dh):
    H = nh * dh
    x = (hi.double() + lo.double()).view(B, S, 3, nh, dh)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh) + addmask.double().view(B, 1, 1, S)
    assert H == nh * dh
    return torch.softmax(s, dim=-1)


def _emit(hi, lo, addmask, B, S, nh, dh, p, seed, nq=None):
    """(probs buffer incl. guard, ctx_hi, ctx_lo, lse) of vl_attn2_fwd_probs and (ctx_hi, ctx_lo, lse) of vl_attn2_fwd."""
    H, n = nh * dh, S if nq is None else nq
    buf = torch.full((B * nh * S * S + GUARD,), SENTINEL, device=DEV)
    outs = []
    for emit in (True, False):
        ch, cl = torch.zeros(B * n, H, dtype=BF16, device=DEV), torch.zeros(B * n, H, dtype=BF16, device=DEV)
        lse = torch.zeros(B * nh * S, device=DEV)
        if emit:
            ops.attn2_fwd_probs(hi, lo, addmask, ch, cl, lse, buf, B, S, nh, dh, p, seed, nq=nq)
        else:
            ops.attn2_fwd(hi, lo, addmask, ch, cl, lse, B, S, nh, dh, p, seed, nq=nq)
        outs.append((ch, cl, lse))
    torch.cuda.synchronize()
    return buf, outs[0], outs[1]


@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("S", [2, 7, 56, 76, 120, 140, 160])
def test_emitted_probabilities_against_fp64(S, dh):
    B, nh = 2, 3
    hi, lo, addmask = _kernel_case(B, S, nh, dh, seed=40 + S)
    buf, em, plain = _emit(hi, lo, addmask, B, S, nh, dh, 0.0, 1)
    n = B * nh * S * S
    P = buf[:n].view(B, nh, S, S)
    ref = _softmax64(hi, lo, addmask, B, S, nh, dh)
    err = (P.double() - ref).abs().max().item()
    rows = (P.double().sum(-1) - 1.0).abs().max().item()
    print("emitted P S=%d dh=%d: max |P - fp64| %.2e, max |row sum - 1| %.2e (bound %.2e)" % (S, dh, err, rows, S * 2.0 ** -23))
    assert torch.isfinite(P).all()
    assert err <= P_TOL, err
    assert rows <= S * 2.0 ** -23, rows
    m = addmask.view(B, 1, 1, S).expand(B, nh, S, S)
    assert (P[m == -float("inf")] == 0).all()
    assert (P[m == -10000.0] < 1e-30).all()
    assert (m == -float("inf")).any() and (m == -10000.0).any()
    for a, b in zip(em, plain):  # the same arithmetic in the same order: only stores were added
        assert torch.equal(a, b)
    assert (buf[n:] == SENTINEL).all(), "the kernel wrote past the end of probs"
    # nq < S: only the rows of queries [0, nq) are written, with the values of the full call
    for nq in sorted({1, (S + 1) // 2}):
        if nq >= S:
            continue
        buf2, em2, plain2 = _emit(hi, lo, addmask, B, S, nh, dh, 0.0, 1, nq=nq)
        P2 = buf2[:n].view(B, nh, S, S)
        assert torch.equal(P2[:, :, :nq], P[:, :, :nq])
        assert (P2[:, :, nq:] == SENTINEL).all() and (buf2[n:] == SENTINEL).all()
        for a, b in zip(em2, plain2):
            assert torch.equal(a, b)


@pytest.mark.parametrize("S,dh", [(7, 64), (56, 64), (140, 64), (76, 32)])
def test_emitted_probabilities_under_dropout(S, dh):
    B, nh, p, seed = 2, 3, 0.1, 77
    hi, lo, addmask = _kernel_case(B, S, nh, dh, seed=90 + S)
    n = B * nh * S * S
    buf0, _, _ = _emit(hi, lo, addmask, B, S, nh, dh, 0.0, seed)
    buf, em, plain = _emit(hi, lo, addmask, B, S, nh, dh, p, seed)
    for a, b in zip(em, plain):
        assert torch.equal(a, b)
    assert (buf[n:] == SENTINEL).all()
    keep = DM.attn_mask(seed, B, nh, S, p)
    P0 = buf0[:n].view(B, nh, S, S).cpu().numpy()
    P = buf[:n].view(B, nh, S, S).cpu().numpy()
    want = P0 * keep  # fp32: (e * inv) * keep; the kernel forms e * (inv * keep)
    dropped = keep == 0
    assert dropped.any() and (S < 56 or 0.05 < dropped.mean() < 0.15)
    assert (P[dropped] == 0).all()
    ulps = np.abs(P - want)[~dropped] / np.spacing(np.abs(want[~dropped]).astype(np.float32))
    print("emitted P under dropout S=%d dh=%d: max %.1f ulp from (eval P) x mask" % (S, dh, ulps.max()))
    assert ulps.max() <= 4, ulps.max()


def test_emitting_entry_points_reject_bad_arguments():
    B, S, nh, dh = 2, 20, 3, 64
    hi, lo, addmask = _kernel_case(B, S, nh, dh, seed=3)
    H = nh * dh
    ch, cl = torch.zeros(B * S, H, dtype=BF16, device=DEV), torch.zeros(B * S, H, dtype=BF16, device=DEV)
    lse = torch.zeros(B * nh * S, device=DEV)
    buf = torch.full((B * nh * S * S + GUARD,), SENTINEL, device=DEV)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    bad = [dict(S=161), dict(S=0), dict(dh=48), dict(nq=S + 1), dict(nq=0), dict(p_drop=1.0), dict(probs=p(buf) + 4)]
    for kw in bad:
        a = dict(S=S, dh=dh, nq=S, p_drop=0.0, probs=p(buf))
        a.update(kw)
        rc = L.vl_attn2_fwd_probs(p(hi), p(lo), p(addmask), p(ch), p(cl), p(lse), a["probs"], B, a["S"], nh, a["dh"], a["nq"],
                                  a["p_drop"], 1, st)
        assert rc < 0 and L.vl_last_error().decode(), kw
        assert "vl_attn2_fwd_probs" in L.vl_last_error().decode()
        xh, xl = torch.zeros(B * S, H, dtype=BF16, device=DEV), torch.zeros(B * S, H, dtype=BF16, device=DEV)
        wh, wl = torch.zeros(3 * H, H, dtype=BF16, device=DEV), torch.zeros(3 * H, H, dtype=BF16, device=DEV)
        bias = torch.zeros(3 * H, device=DEV)
        rc = L.vl_qkv_attention_fwd_probs(p(xh), p(xl), p(wh), p(wl), p(bias), p(addmask), p(hi), p(lo), p(ch), p(cl), p(lse),
                                          a["probs"], B, a["S"], nh, a["dh"], a["nq"], a["p_drop"], 1, st)
        assert rc < 0 and "vl_qkv_attention_fwd_probs" in L.vl_last_error().decode(), kw
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (ch == 0).all() and (lse == 0).all()  # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# model surface
# ---------------------------------------------------------------------------------------------------------------------
def _build(config, seed, with_oracle=True):
    model = BertForVLTasks(config, TASK_CFG, ["TASK15"])
    sd = seeded_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd, strict=True)
    oracle = None
    if with_oracle:
        oracle = O.OracleUC2ForVLTasks(config, TASK_CFG, ["TASK15"])
        oracle.load_state_dict(sd, strict=True)
    return model.cuda(), oracle


def _inputs(B, T, V, vocab, seed):
    """(question, features, spatials, segment_ids, input_mask, image_mask) with padded text (make_batch) and boxes."""
    feats, spat, imask, q, _, tmask, seg, _, _, _ = make_batch(B, seq_len=T, num_boxes=V, vocab_size=vocab, seed=seed)
    imask = imask.clone()
    imask[0, V - 3:] = 0
    if tmask.all():
        q, tmask = q.clone(), tmask.clone()
        q[B - 1, T - 2] = 2
        q[B - 1, T - 1] = 1
        tmask[B - 1, T - 1] = 0
    return q, feats, spat, seg, tmask, imask


def _call(model, inputs, **flags):
    q, feats, spat, seg, tmask, imask = (t.cuda() for t in inputs)
    return model(q, feats, spat, "TASK15", seg, tmask, imask, **flags)


def _check_structure(out, n_layers, B, T, V, H, nh, maps=True):
    assert isinstance(out, tuple) and len(out) == 6
    logits, vis, ling, (maps_t, maps_v), hs_t, hs_v = out
    assert vis is None and ling is None
    n = 1 + 2 * n_layers
    assert len(hs_t) == len(hs_v) == len(maps_t) == len(maps_v) == n
    for h_t, h_v in zip(hs_t, hs_v):
        assert h_t.shape == (B, T, H) and h_v.shape == (B, V, H)
        for t in (h_t, h_v):
            assert t.dtype == torch.float32 and t.is_cuda and not t.requires_grad and t.grad_fn is None
    for lst, nq, nk in ((maps_t, T, V), (maps_v, V, T)):
        assert lst[0] is None
        for i in range(1, n):
            if i % 2 == 0 or not maps:  # feed-forward sub-layers; attention sub-layers without config.visualization
                assert lst[i] is None
                continue
            assert sorted(lst[i]) == sorted(MAP_KEYS)
            assert lst[i]["intra_attn"].shape == (B, nh, nq, nq) and lst[i]["inter_attn"].shape == (B, nh, nq, nk)
            assert lst[i]["queries"].shape == lst[i]["keys"].shape == (B, nh, nq, H // nh)
            for t in lst[i].values():
                assert t.dtype == torch.float32 and t.is_cuda and not t.requires_grad and t.grad_fn is None


def _compare(out, ref_hs_t, ref_hs_v, ref_maps_t, ref_maps_v, what):
    """max abs errors {hidden, intra_attn, ...}; the reference lists hold one dict per attention sub-layer."""
    _, _, _, (maps_t, maps_v), hs_t, hs_v = out
    worst = {}

    def upd(k, got, ref):
        ref = torch.as_tensor(ref)
        assert tuple(got.shape) == tuple(ref.shape), (k, got.shape, ref.shape)
        worst[k] = max(worst.get(k, 0.0), (got.detach().double().cpu() - ref.double()).abs().max().item())

    for i in range(len(hs_t)):
        upd("hidden", hs_t[i], ref_hs_t[i])
        upd("hidden", hs_v[i], ref_hs_v[i])
    for j in range(len(ref_maps_t)):
        for k in MAP_KEYS:
            upd(k, maps_t[2 * j + 1][k], ref_maps_t[j][k])
            upd(k, maps_v[2 * j + 1][k], ref_maps_v[j][k])
    print("%s: max abs error %s" % (what, {k: "%.2e" % v for k, v in sorted(worst.items())}))
    return worst


def test_model_matches_the_reference_maps_fixture():
    g = load_golden("uc2_maps.npz")
    config = golden_config(g)
    model, _ = _build(config, seed=int(g["seed"]), with_oracle=False)
    model.eval()
    t = torch.from_numpy
    B, T = g["question"].shape
    V = g["features"].shape[1]
    inputs = (t(g["question"].astype(np.int64)), t(g["features"].astype(np.float32)), t(g["spatials"].astype(np.float32)),
              torch.zeros(B, T, dtype=torch.int64), t(g["input_mask"].astype(np.int64)), t(g["image_mask"].astype(np.int64)))
    with torch.no_grad():
        out = _call(model, inputs, output_all_encoded_layers=True, output_all_attention_masks=True)
    _check_structure(out, 2, B, T, V, 128, 2)
    ref_t = [{k: g["%s_t_%d" % (k, i)] for k in MAP_KEYS} for i in (1, 3)]
    ref_v = [{k: g["%s_v_%d" % (k, i)] for k in MAP_KEYS} for i in (1, 3)]
    worst = _compare(out, [g["hidden_t_%d" % i] for i in range(5)], [g["hidden_v_%d" % i] for i in range(5)], ref_t, ref_v,
                     "model vs reference fixture (uc2_maps.npz)")
    err = (out[0].cpu() - t(g["logits"])).abs().max().item()
    print("  logits: max abs error %.2e" % err)
    assert err <= LOGIT_TOL
    for k, v in worst.items():
        assert v <= LOGIT_TOL, (k, v)


@pytest.mark.parametrize("n_layers", [2, 12])
@pytest.mark.parametrize("B,T,V", [(8, 20, 36), (3, 7, 9), (2, 20, 100)])
def test_full_width_against_the_oracle_helper(n_layers, B, T, V):
    cfg = uc2_cfg_dict(n_layers=n_layers, vocab=2000)
    cfg["visualization"] = True
    config = BertConfig.from_dict(cfg)
    model, oracle = _build(config, seed=20 + n_layers)
    model.eval()
    oracle.eval()
    inputs = _inputs(B, T, V, 2000, seed=500 + B)
    with torch.no_grad():
        out = _call(model, inputs, output_all_encoded_layers=True, output_all_attention_masks=True)
    _check_structure(out, n_layers, B, T, V, 768, 12)
    rec = AR.oracle_maps(oracle, inputs, double=True)
    worst = _compare(out, *AR.split_maps(rec, T), what="model vs fp64 oracle helper L=%d B=%d T=%d V=%d" % (n_layers, B, T, V))
    assert (out[0].double().cpu() - rec["logits"]).abs().max().item() <= LOGIT_TOL
    for k, v in worst.items():
        assert v <= LOGIT_TOL, (k, v)


def test_logits_with_the_flags_equal_the_dense_run():
    cfg = uc2_cfg_dict(n_layers=3, vocab=800)
    cfg["visualization"] = True
    model, _ = _build(BertConfig.from_dict(cfg), seed=29, with_oracle=False)
    model.eval()
    inputs = _inputs(8, 20, 36, 800, seed=308)
    with torch.no_grad():
        pooled = _call(model, inputs)[0].clone()
        on = _call(model, inputs, output_all_encoded_layers=True, output_all_attention_masks=True)[0].clone()
        assert model.engine.stack.pooled_only  # the option held for that call only
        model.engine.stack.pooled_only = False
        dense = _call(model, inputs)[0].clone()
    assert torch.equal(on, dense)
    torch.testing.assert_close(on, pooled, rtol=0, atol=5e-5)


def test_without_visualization_the_maps_are_none_and_no_probabilities_are_stored():
    cfg = uc2_cfg_dict(n_layers=2, vocab=800)
    assert not BertConfig.from_dict(cfg).visualization
    model, _ = _build(BertConfig.from_dict(cfg), seed=31, with_oracle=False)
    model.eval()
    B, T, V = 8, 20, 136
    inputs = _inputs(B, T, V, 800, seed=309)
    peaks = {}
    with torch.no_grad():
        for maps in (False, True, False, True):
            out = _call(model, inputs, output_all_encoded_layers=True, output_all_attention_masks=maps)
            del out
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = _call(model, inputs, output_all_encoded_layers=True, output_all_attention_masks=maps)
            torch.cuda.synchronize()
            peaks[maps] = torch.cuda.max_memory_allocated() - base
            if maps:
                _check_structure(out, 2, B, T, V, 768, 12, maps=False)
            else:
                assert out[3] == ([None], [None])
            del out
        mask_only = _call(model, inputs, output_all_attention_masks=True)
    assert len(mask_only) == 4 and mask_only[3] == ([None] * 5, [None] * 5)
    probs_bytes = 4 * B * 12 * (T + V) ** 2  # one layer's [B, nh, S, S] fp32
    print("peak extra bytes: hidden only %d, hidden + maps asked (visualization off) %d; one probability buffer = %d"
          % (peaks[False], peaks[True], probs_bytes))
    assert peaks[True] - peaks[False] < probs_bytes // 2


def test_training_step_with_the_flags_leaves_the_gradients_alone():
    cfg = uc2_cfg_dict(n_layers=2, vocab=2000)
    cfg["visualization"] = True
    config = BertConfig.from_dict(cfg)
    model, oracle = _build(config, seed=13)
    B, T, V, nh = 8, 20, 36, 12
    inputs = _inputs(B, T, V, 2000, seed=208)
    labels = torch.arange(B, device=DEV) * 7 % 1842
    eng = model.engine
    eng.base_seed = BASE_SEED
    eng.stack.pooled_only = False
    model.train()
    runs = {}
    for flags in (True, False):
        eng.calls = 0
        torch.manual_seed(5)
        model.zero_grad()
        out = _call(model, inputs, output_all_encoded_layers=flags, output_all_attention_masks=flags)
        loss = torch.nn.functional.cross_entropy(out[0], labels)
        loss.backward()
        torch.cuda.synchronize()
        assert eng.calls == 1
        runs[flags] = (out, float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    out = runs[True][0]
    _check_structure(out, 2, B, T, V, 768, nh)  # (detached: no grad_fn, requires_grad False)
    assert out[0].requires_grad and len(runs[False][0]) == 4
    assert runs[True][1] == runs[False][1] and torch.equal(runs[True][0][0], runs[False][0][0])
    assert runs[True][2].keys() == runs[False][2].keys() and len(runs[True][2]) > 30
    for n, gr in runs[True][2].items():
        assert torch.equal(gr, runs[False][2][n]), n
    # the emitted (post-dropout) probabilities against the helper under the engine's own masks of call 1
    masks = DM.StepMasks("uc2", BASE_SEED, 1, B, T, V, nh, config.hidden_dropout_prob, config.attention_probs_dropout_prob, 0.1)
    O.set_mask_provider(oracle, masks)
    try:
        oracle.train()
        rec = AR.oracle_maps(oracle, inputs, double=True,
                             attn_keep=AR.engine_attn_keep(BASE_SEED, 1, config.attention_probs_dropout_prob))
    finally:
        O.set_mask_provider(oracle, None)
    worst = _compare(out, *AR.split_maps(rec, T), what="train(): model vs fp64 oracle helper with the engine's masks")
    P = torch.cat([torch.cat([out[3][0][1]["intra_attn"], out[3][0][1]["inter_attn"]], -1),
                   torch.cat([out[3][1][1]["inter_attn"], out[3][1][1]["intra_attn"]], -1)], 2)
    live = torch.cat([inputs[4], inputs[5]], 1).bool().to(DEV)[:, None, None, :].expand_as(P)  # (padded keys underflow to 0)
    assert 0.05 < (P[live] == 0).float().mean().item() < 0.15  # dropout really is in the emitted tensor
    assert worst["intra_attn"] <= LOGIT_TOL and worst["inter_attn"] <= LOGIT_TOL


def test_ordinary_call_after_a_tapped_call_and_memory_of_repeated_tapped_calls():
    cfg = uc2_cfg_dict(n_layers=2, vocab=800)
    cfg["visualization"] = True
    config = BertConfig.from_dict(cfg)
    model, _ = _build(config, seed=33, with_oracle=False)
    fresh, _ = _build(config, seed=33, with_oracle=False)
    model.eval()
    fresh.eval()
    inputs = _inputs(4, 20, 36, 800, seed=310)
    with torch.no_grad():
        out = _call(model, inputs, output_all_encoded_layers=True, output_all_attention_masks=True)
        del out
        after = _call(model, inputs)[0].clone()
        want = _call(fresh, inputs)[0].clone()
        assert torch.equal(after, want)  # the descriptor went back: pooled-row mode, no taps
        mem = []
        for _ in range(4):
            out = _call(model, inputs, output_all_encoded_layers=True, output_all_attention_masks=True)
            del out
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated())
    assert mem[2] <= mem[1] and mem[3] <= mem[1], mem


def test_stack_rejects_a_tap_on_a_pooled_row_layer():
    from clg_vqa_amd.engine import VL
    cfg = uc2_cfg_dict(n_layers=2, vocab=800)
    model, _ = _build(BertConfig.from_dict(cfg), seed=35, with_oracle=False)
    model.eval()
    inputs = _inputs(4, 20, 36, 800, seed=311)
    with torch.no_grad():
        _call(model, inputs)
    torch.cuda.synchronize()
    ar = model.engine._last_arena
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    tap = torch.full((4 * 56, 768), SENTINEL, device=DEV)
    x_before = ar.x32.clone()
    last = VL["VL_ST_FIELDS"] + 1 * VL["VL_LY_FIELDS"]
    for field in ("VL_LY_TAP_PROBS", "VL_LY_TAP_X1", "VL_LY_TAP_OUT"):
        d = ar.desc.copy()
        assert d[VL["VL_ST_POOLED_ONLY"]] == 1
        d[last + VL[field]] = tap.data_ptr()
        rc = L.vl_stack_fwd(d.ctypes.data, 0, 2, st, None)
        msg = L.vl_last_error().decode()
        assert rc < 0 and "pooled" in msg and "vl_stack_fwd" in msg, (field, rc, msg)
    torch.cuda.synchronize()
    assert (tap == SENTINEL).all() and torch.equal(ar.x32, x_before)  # nothing was launched
