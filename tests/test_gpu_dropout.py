"""Training mode (dropout on) against the oracle, with the oracle handed exactly the engine's masks.

Every dropout mask of the HIP path is a pure function of a counter-based hash of (seed, site, element); tests/dropout_masks.py
restates the generators on the host.  Here (1) the restatement is checked bit for bit against the masks the kernels draw
(read back through inputs that make the output equal to the keep-scale), (2) the kernels' values with dropout on are checked
against fp64 math with the host mask, and (3) whole training steps of the model are checked against the oracle running in
train() with the restated masks, at the bounds of the eval-mode parity tests.  Negative controls show that the mask of
the neighbouring seed at any one site kind breaks those bounds.  Needs a real MI355X: ``pytest -m gpu``."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_bwd_ref as AR  # noqa: E402
import dropout_masks as DM  # noqa: E402
import grad_check as G  # noqa: E402
from grad_check import GRAD_REL_L2  # noqa: E402
from helpers import TASK_CFG, golden_config, load_golden, uc2_cfg_dict  # noqa: E402
from oracle import m3p_oracle as Mo  # noqa: E402
from oracle import uc2_oracle as O  # noqa: E402
from clg_vqa_amd import ops, task_utils  # noqa: E402
from clg_vqa_amd.config import BertConfig  # noqa: E402
from clg_vqa_amd.encoders import BertForVLTasks  # noqa: E402
from clg_vqa_amd.m3p import M3PForVLTasks  # noqa: E402
from clg_vqa_amd.ops import BF16  # noqa: E402
from clg_vqa_amd.synthetic import make_batch, seeded_state_dict  # noqa: E402

DEV = "cuda"
LOGIT_TOL = 1e-3
LOSS_REL = 2e-4


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _split(x):
    hi, lo = torch.empty_like(x, dtype=BF16), torch.empty_like(x, dtype=BF16)
    ops.split_f32(x.contiguous(), hi, lo)
    return hi, lo


def _t(a):
    return torch.from_numpy(a).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm: p_pre (dropout of the sub-layer output before the residual add) and p_post (embeddings: after the LayerNorm)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("pooled", [False, True])
def test_layernorm_pre_dropout_mask_and_values(H, pooled):
    """p_pre with orig_row_stride 1 (dense) and S (the compact pooled rows of the last layer): the saved z of y = 1 is the
    keep-scale itself and must equal the restated mask; then output, z, dz, dpre, dgamma, dbeta, dbias against fp64 math
    with that mask, at the bounds of test_layernorm_forward_backward."""
    B, S, p, seed, eps = 5, 56, 0.1, 777 * 4096 + 4, 1e-5
    stride = S if pooled else 1
    M = B if pooled else B * S
    mask = _t(DM.ln_pre_mask(seed, M, H, p, orig_row_stride=stride))
    gamma, beta = 1 + 0.1 * _rand(H, seed=20), 0.1 * _rand(H, seed=21)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    z = torch.ones(M, H, device=DEV)
    out = torch.empty(M, H, device=DEV)
    ops.ln_fwd(z, None, None, gamma, beta, eps, out, None, None, mean, rstd, M, H, p_pre=p, seed=seed,
               orig_row_stride=stride)
    assert torch.equal(z, mask)
    assert abs((mask == 0).float().mean().item() - p) < 0.03
    y, resid = _rand(M, H, seed=17), _rand(M, H, seed=18)
    z = y.clone()
    hi, lo = torch.empty(M, H, dtype=BF16, device=DEV), torch.empty(M, H, dtype=BF16, device=DEV)
    ops.ln_fwd(z, resid, None, gamma, beta, eps, out, hi, lo, mean, rstd, M, H, p_pre=p, seed=seed, orig_row_stride=stride)
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    zr = y64 * mask.double() + resid.double()
    u = zr.mean(-1, keepdim=True)
    s = (zr - u).pow(2).mean(-1, keepdim=True)
    ref = g64 * ((zr - u) / torch.sqrt(s + eps)) + b64
    zr.retain_grad()
    torch.testing.assert_close(z.double(), zr.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(out.double(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(hi.double() + lo.double(), ref.detach(), rtol=1e-4, atol=1e-4)
    dy = _rand(M, H, seed=22)
    ref.backward(dy.double())
    dz, dpre = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV)
    dg, db, dbias = torch.empty(H, device=DEV), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    ops.ln_bwd(dy, z, mean, rstd, gamma, dz, None, dpre, dg, db, dbias, ops.ln_bwd_ws(M, H, DEV), M, H, p_pre=p, seed=seed,
               orig_row_stride=stride)
    torch.testing.assert_close(dz.double(), zr.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dpre.double(), y64.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dg.double(), g64.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(db.double(), b64.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dbias.double(), y64.grad.sum(0), rtol=1e-4, atol=1e-4)


# (name, rows per sample of the call, rows before them in the [B, S] output, row_pre) -- the embedding LayerNorms
EMBED_ROW_MAPS = [("uc2_text", 20, 0, False), ("uc2_box", 36, 20, False), ("m3p_image", 36, 0, True),
                  ("m3p_text", 20, 36, True), ("m3p_image_ln", None, None, False)]


@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("name,G,off,row_pre", EMBED_ROW_MAPS)
def test_layernorm_post_dropout_mask_and_values(H, name, G, off, row_pre):
    """p_post under the row maps of the embeddings (group / out_stride / out_off, M3P's row_pre length mask): the output
    with dropout against the p = 0 output times the restated mask of the INPUT row (bit-equal), then output and gradients
    against fp64 math with that mask."""
    B, S, p, seed, eps = 3, 56, 0.1, 31337 * 4096 + 2, 1e-5
    Gr = G or 36
    M = B * Gr
    grp = dict(group=G, out_stride=S, out_off=off) if G else {}
    Mout = B * S if G else M
    rows = torch.arange(M, device=DEV)
    orow = (rows // G) * S + off + rows % G if G else rows
    rp = (torch.rand(M, generator=torch.Generator().manual_seed(3)) > 0.25).float().to(DEV) if row_pre else None
    mask = _t(DM.ln_post_mask(seed, M, H, p))
    y = _rand(M, H, seed=40)
    gamma, beta = 1 + 0.1 * _rand(H, seed=41), 0.1 * _rand(H, seed=42)
    outs = {}
    for pp in (0.0, p):
        out = torch.zeros(Mout, H, device=DEV)
        mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        z = y.clone()
        ops.ln_fwd(z, None, None, gamma, beta, eps, out, None, None, mean, rstd, M, H, p_post=pp, seed=seed, row_pre=rp, **grp)
        outs[pp] = (out, z, mean, rstd)
    out, z, mean, rstd = outs[p]
    assert torch.equal(out[orow], outs[0.0][0][orow] * mask)
    # values: out[orow] = dropout(LN(y * row_pre))
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    zr = y64 * (rp.double()[:, None] if row_pre else 1.0)
    ref = torch.nn.functional.layer_norm(zr, (H,), g64, b64, eps) * mask.double()
    torch.testing.assert_close(out[orow].double(), ref.detach(), rtol=1e-5, atol=1e-5)
    dy = _rand(Mout, H, seed=43)
    ref.backward(dy[orow].double())
    dz = torch.empty(M, H, device=DEV)
    dg, db, dbias = torch.empty(H, device=DEV), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    ops.ln_bwd(dy, z, mean, rstd, gamma, dz, None, None, dg, db, dbias, ops.ln_bwd_ws(M, H, DEV), M, H, p_post=p, seed=seed,
               row_pre=rp, **grp)
    torch.testing.assert_close(dz.double(), y64.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dg.double(), g64.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(db.double(), b64.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dbias.double(), y64.grad.sum(0), rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _attn_ref(qkv, addmask, B, S, nh, dh, keep=None):
    H = nh * dh
    q, k, v = [t.view(B, S, nh, dh).permute(0, 2, 1, 3) for t in qkv.view(B, S, 3 * H).split(H, dim=-1)]
    s = q @ k.transpose(-1, -2) / math.sqrt(dh) + addmask.view(B, 1, 1, S)
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep
    return (p @ v).permute(0, 2, 1, 3).reshape(B * S, H)


@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("S", [16, 56, 120, 140, 160])
@pytest.mark.parametrize("nq1", [False, True])
def test_attention_dropout_mask_equals_restatement(S, dh, nq1):
    """One-hot V (window w of ceil(S / dh): V[key] = e_(key - w dh)) and Q = 0 (uniform P = 1 / S, no padded keys): ctx[q, d]
    * S = the keep-scale of (q, w dh + d).  Every key of every (sample, head, query row) -- or of query row 0 at nq = 1 --
    against the restated mask."""
    B, nh, p = 2, 4, 0.1
    H = nh * dh
    seed = 4242 * 4096 + 16 * 3 + 3
    ref = DM.attn_mask(seed, B, nh, S, p)  # [b, h, q, k]
    addmask = torch.zeros(B * S, device=DEV)
    nq = 1 if nq1 else S
    got = np.zeros((B, nh, nq, S), np.float32)
    for w in range((S + dh - 1) // dh):
        z = torch.zeros(B, S, 3, nh, dh, device=DEV)
        keys = torch.arange(w * dh, min(S, (w + 1) * dh), device=DEV)
        z[:, keys, 2, :, keys - w * dh] = 1.0
        zh, zl = _split(z.view(B * S, 3 * H))
        rows = B if nq1 else B * S
        ch, cl = torch.empty(rows, H, dtype=BF16, device=DEV), torch.empty(rows, H, dtype=BF16, device=DEV)
        lse = torch.empty(B * nh * S, device=DEV)
        ops.attn2_fwd(zh, zl, addmask, ch, cl, lse, B, S, nh, dh, p, seed, nq=nq)
        c = ((ch.double() + cl.double()) * S).view(B, nq, nh, dh).permute(0, 2, 1, 3).cpu().numpy()
        got[..., w * dh:w * dh + len(keys)] = c[..., :len(keys)]
    exp = ref[:, :, :nq]
    np.testing.assert_allclose(got, exp, rtol=2e-4, atol=1e-4)
    assert np.array_equal(got > 0.5, exp > 0)


@pytest.mark.parametrize("B,S,dh,nq1", AR.DROPOUT_CASES)
def test_attention_dropout_values_against_fp64(B, S, dh, nq1):
    """attn2_fwd / attn2_bwd with dropout (p 0.1, padded keys) against fp64 attention with the restated keep mask: forward
    within 3e-5 at the (hi + lo) operands, backward within 2e-2 rel-L2 at the bf16-rounded operands (the p = 0 bounds)."""
    nh, p = 4, 0.1
    H = nh * dh
    seed = 99991 * 4096 + 16 + 3
    qkv = _rand(B * S, 3 * H, seed=12, scale=1.5)
    hi, lo = _split(qkv)
    m = torch.ones(B, S, device=DEV)
    m[0, S - 5:] = 0
    m[-1, 3:6] = 0
    addmask = ((1 - m) * -10000.0).reshape(-1).contiguous()
    keep = torch.from_numpy(DM.attn_mask(seed, B, nh, S, p)).double().to(DEV)
    nq = 1 if nq1 else S
    rows = B if nq1 else B * S
    ctx_hi = torch.full((rows, H), float("nan"), dtype=BF16, device=DEV)
    ctx_lo = torch.full_like(ctx_hi, float("nan"))
    lse = torch.empty(B * nh * S, device=DEV)
    ops.attn2_fwd(hi, lo, addmask, ctx_hi, ctx_lo, lse, B, S, nh, dh, p, seed, nq=nq)
    ref = _attn_ref(hi.double() + lo.double(), addmask.double(), B, S, nh, dh, keep).view(B, S, H)
    ref = ref[:, :1].reshape(rows, H) if nq1 else ref.reshape(rows, H)
    got = ctx_hi.double() + ctx_lo.double()
    err = (got - ref).abs().max().item()
    assert err < 3e-5 * max(1.0, ref.abs().max().item()), err
    d16 = _rand(rows, H, seed=13).to(BF16)
    qh = hi.double().clone().requires_grad_(True)
    r = _attn_ref(qh, addmask.double(), B, S, nh, dh, keep).view(B, S, H)
    (r[:, :1].reshape(rows, H) if nq1 else r.reshape(rows, H)).backward(d16.double())
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=BF16, device=DEV)
    ops.attn2_bwd(hi, addmask, d16, lse, dqkv, B, S, nh, dh, p, seed, nq=nq)
    g = qh.grad
    assert torch.isfinite(dqkv.float()).all()
    rel = (dqkv.double() - g).norm().item() / g.norm().item()
    print("attn dropout B=%d S=%d dh=%d nq=%d: fwd max err %.2e, bwd rel-L2 %.3e" % (B, S, dh, nq, err, rel))
    assert rel <= 2e-2, rel
    # per (q / k / v, head) block and per sequence row of a block, against the restatement with the kernel's lse / P / dS points
    AR.check_blocks("attn dropout B=%d S=%d dh=%d nq=%d" % (B, S, dh, nq), dqkv, hi, lo, addmask.view(B, S), d16, B, S, nh, dh,
                    keep, nq1)
    # the same call without the mask in the reference must miss: the bounds do see the mask
    assert (got - _attn_ref(hi.double() + lo.double(), addmask.double(), B, S, nh, dh).view(B, S, H)[:, :1 if nq1 else S]
            .reshape(rows, H)).abs().max().item() > 100 * 3e-5


# ---------------------------------------------------------------------------------------------------------------------
# head activation kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,p", [(8, 768, 0.1), (64, 128, 0.5), (3, 1536, 0.25)])
def test_head_dropout_mask_equals_restatement(M, N, p):
    seed = DM.site_seed(DM.seed0_of(0x5EED ^ 7, 5), DM.HEAD_SITE)
    mask = torch.empty(M, N, device=DEV)
    ops.act_fwd(torch.ones(M, N, device=DEV), M, N, ops.ACT_NONE, p, seed, out32=mask)
    assert torch.equal(mask, _t(DM.head_mask(seed, M, N, p)))


# ---------------------------------------------------------------------------------------------------------------------
# the model: a training step against the oracle with the engine's masks
# ---------------------------------------------------------------------------------------------------------------------
BASE_SEED = 0x5EED ^ 20261016


def _uc2_build(config, seed):
    model = BertForVLTasks(config, TASK_CFG, ["TASK15"])
    sd = seeded_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd, strict=True)
    oracle = O.OracleUC2ForVLTasks(config, TASK_CFG, ["TASK15"])
    oracle.load_state_dict(sd, strict=True)
    return model.cuda(), oracle


def _m3p_build(config, seed):
    model = M3PForVLTasks(config, TASK_CFG, ["TASK15"])
    sd = seeded_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd, strict=True)
    oracle = Mo.OracleM3PForVLTasks(config, TASK_CFG, ["TASK15"])
    oracle.load_state_dict({k: v for k, v in sd.items() if k in oracle.state_dict()}, strict=True)
    return model.cuda(), oracle


def _native_step(model, batch, train, call):
    """One training forward + backward as the `call`-th forward of the engine; logits of the same call (same masks)."""
    eng = model.engine
    eng.base_seed = BASE_SEED
    eng.calls = call - 1
    model.train(train)
    model.zero_grad()
    loss, _ = task_utils.ForwardModelsTrain(model.config, TASK_CFG, "cuda", "TASK15", batch, model, torch.nn.CrossEntropyLoss())
    loss.backward()
    assert eng.calls == call
    grads = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
    eng.calls = call - 1
    with torch.no_grad():
        b = tuple(t.cuda() for t in batch)
        logits = model(b[3], b[0], b[1], "TASK15", b[6], b[5], b[2])[0].cpu()
    eng.calls = call
    return float(loss.detach()), logits, grads


def _oracle_step(oracle, batch, provider):
    O.set_mask_provider(oracle, provider)
    try:
        oracle.train(provider is not None)
        oracle.zero_grad()
        loss, _, logits = O.forward_train(oracle, batch)
        loss.backward()
    finally:
        O.set_mask_provider(oracle, None)
    return float(loss.detach()), logits.detach(), {n: p.grad for n, p in oracle.named_parameters() if p.grad is not None}


def _errors(native, ref):
    """(max |logit err|, loss rel err, worst gradient rel-L2 error, its name).  Nothing is asserted here: the negative
    controls read the same figures."""
    loss, logits, grads = native
    oloss, ologits, ograds = ref
    err = (logits - ologits).abs().max().item()
    lrel = abs(loss - oloss) / abs(oloss)
    assert grads
    both = {n: g for n, g in grads.items() if ograds.get(n) is not None}  # (M3P: parameters the oracle does not build)
    worst = G.check_grads(both, ograds, check=False)
    return err, lrel, worst["tensor"][0], worst["tensor"][1]


def _within(e):
    return e[0] <= LOGIT_TOL and e[1] <= LOSS_REL and e[2] <= GRAD_REL_L2


def _assert_grads(native, ref, what):
    """The asserting form: every gradient through grad_check (per tensor, scale, row, column, element; key biases by their
    absolute rule)."""
    both = {n: g for n, g in native[2].items() if ref[2].get(n) is not None}
    return G.check_grads(both, ref[2], what)


def _parity(kind, model, oracle, batch, nh, call=1, p_head=0.1, negative=False, also_eval=True):
    B, T = batch[3].shape
    V = batch[0].shape[1]
    cfg = model.config
    p_hid = cfg.dropout if kind == "m3p" else cfg.hidden_dropout_prob
    p_att = cfg.attention_dropout if kind == "m3p" else cfg.attention_probs_dropout_prob
    masks = DM.StepMasks(kind, BASE_SEED, call, B, T, V, nh, p_hid, p_att, p_head)
    native = _native_step(model, batch, True, call)
    ref = _oracle_step(oracle, batch, masks)
    e = _errors(native, ref)
    res = dict(train_logit=e[0], train_loss=e[1], train_grad=e[2], train_grad_at=e[3])
    if also_eval:
        native_eval, ref_eval = _native_step(model, batch, False, call + 1000), _oracle_step(oracle, batch, None)
        ev = _errors(native_eval, ref_eval)
        res.update(eval_logit=ev[0], eval_grad=ev[2])
    print("%s B=%d S=%d call %d: train max|dlogit| %.2e (eval %s), loss rel %.1e, worst grad rel-L2 %.2e at %s (eval %s)" % (
        kind, B, T + V, call, e[0], "%.2e" % res["eval_logit"] if also_eval else "-", e[1], e[2], e[3],
        "%.2e" % res["eval_grad"] if also_eval else "-"))
    assert e[0] <= LOGIT_TOL, e
    assert e[1] <= LOSS_REL, e
    assert e[2] <= GRAD_REL_L2, e
    print("  train gradients: %s" % _assert_grads(native, ref, "%s train()" % kind))
    if also_eval:
        assert e[0] <= max(10 * res["eval_logit"], 1e-4), (e[0], res["eval_logit"])
        print("  eval gradients: %s" % _assert_grads(native_eval, ref_eval, "%s eval()" % kind))
    if negative:  # the mask of the neighbouring seed at one site kind: the same comparison must fail
        for wrong in DM.SITE_KINDS:
            bad = DM.StepMasks(kind, BASE_SEED, call, B, T, V, nh, p_hid, p_att, p_head, wrong=wrong)
            eb = _errors(native, _oracle_step(oracle, batch, bad))
            print("  negative control (%s from the neighbouring seed): max|dlogit| %.2e, loss rel %.1e, worst grad %.2e at %s"
                  % ((wrong,) + eb))
            assert not _within(eb), wrong
    return res


def _pad(batch, V):
    batch = list(batch)
    batch[2] = batch[2].clone()
    batch[2][0, V - 3:] = 0  # padded boxes in sample 0 (padded text comes with make_batch)
    return tuple(batch)


@pytest.mark.parametrize("n_layers,B,T,V", [(2, 8, 20, 36), (1, 3, 7, 9), (2, 2, 20, 100), (1, 2, 60, 100)])
def test_uc2_training_step_matches_oracle_with_engine_masks(n_layers, B, T, V):
    config = BertConfig.from_dict(uc2_cfg_dict(n_layers=n_layers, vocab=2000))
    model, oracle = _uc2_build(config, seed=11 + n_layers)
    batch = _pad(make_batch(B, seq_len=T, num_boxes=V, vocab_size=2000, seed=200 + B), V)
    _parity("uc2", model, oracle, batch, 12, negative=(n_layers, B, T, V) == (2, 8, 20, 36))


def test_uc2_c1_config_training_step():
    """hidden 128, 4 heads (head dim 32), I 512: the H = 128 LayerNorm and the dh = 32 attention instances."""
    config = BertConfig.from_dict(uc2_cfg_dict(hidden=128, heads=4, inter=512, n_layers=2, vocab=1000))
    model, oracle = _uc2_build(config, seed=7)
    _parity("uc2", model, oracle, _pad(make_batch(4, seq_len=20, num_boxes=36, vocab_size=1000, seed=8), 36), 4, negative=True)


def test_uc2_twelve_layers_training_step():
    config = BertConfig.from_dict(uc2_cfg_dict(n_layers=12, vocab=2000))
    model, oracle = _uc2_build(config, seed=12)
    _parity("uc2", model, oracle, _pad(make_batch(2, seq_len=20, num_boxes=36, vocab_size=2000, seed=9), 36), 12)


def test_uc2_dense_last_layer_training_step():
    """pooled_only off: the last layer runs every row (dense counters, nq = S) instead of the pooled rows."""
    config = BertConfig.from_dict(uc2_cfg_dict(n_layers=2, vocab=2000))
    model, oracle = _uc2_build(config, seed=13)
    model.engine.stack.pooled_only = False
    _parity("uc2", model, oracle, _pad(make_batch(4, seq_len=20, num_boxes=36, vocab_size=2000, seed=10), 36), 12)


def test_uc2_large_dropout_probabilities():
    cfgd = uc2_cfg_dict(n_layers=2, vocab=2000)
    cfgd["hidden_dropout_prob"], cfgd["attention_probs_dropout_prob"] = 0.3, 0.25
    config = BertConfig.from_dict(cfgd)
    model, oracle = _uc2_build(config, seed=14)
    model.dropout.p = 0.5
    oracle.p_pool = 0.5
    _parity("uc2", model, oracle, _pad(make_batch(4, seq_len=20, num_boxes=36, vocab_size=2000, seed=11), 36), 12, p_head=0.5)


def test_uc2_sft_masks_with_100_boxes_training_step():
    """SFT masks (prune.CustomFromMask on every prunable Linear) and the 100-box stream, dropout on: masked weight
    gradients exactly zero, the rest at the parity bounds."""
    from torch.nn.utils import prune
    config = BertConfig.from_dict(uc2_cfg_dict(n_layers=2, vocab=500))
    model, oracle = _uc2_build(config, seed=23)
    names = O.uc2_prunable_names(n_sublayers=4)
    gen = torch.Generator().manual_seed(4321)
    mods, omods = dict(model.named_modules()), dict(oracle.named_modules())
    masks = {}
    for n in names:
        masks[n] = (torch.rand(mods[n].weight.shape, generator=gen) < 0.59).float()
        mods[n].weight.data.mul_(masks[n].cuda())
        omods[n].weight.data.mul_(masks[n])
        prune.CustomFromMask.apply(mods[n], "weight", mask=masks[n].cuda())
        prune.CustomFromMask.apply(omods[n], "weight", mask=masks[n])
    batch = _pad(make_batch(4, seq_len=20, num_boxes=100, vocab_size=500, seed=33), 100)
    _parity("uc2", model, oracle, batch, 12)
    for n in names:
        assert torch.all(mods[n].weight_orig.grad.cpu()[masks[n] == 0] == 0), n


def test_uc2_consecutive_calls_use_their_own_masks():
    """Two forward / backward calls on one model without resetting the call count: each against the masks of its own
    call (the (base seed, call count) schedule that checkpoints store and restore)."""
    config = BertConfig.from_dict(uc2_cfg_dict(n_layers=2, vocab=2000))
    model, oracle = _uc2_build(config, seed=15)
    batch = _pad(make_batch(4, seq_len=20, num_boxes=36, vocab_size=2000, seed=12), 36)
    eng = model.engine
    eng.base_seed, eng.calls = BASE_SEED, 0
    model.train()
    for call in (1, 2):
        model.zero_grad()
        loss, _ = task_utils.ForwardModelsTrain(config, TASK_CFG, "cuda", "TASK15", batch, model, torch.nn.CrossEntropyLoss())
        loss.backward()
        assert eng.calls == call
        grads = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
        masks = DM.StepMasks("uc2", BASE_SEED, call, 4, 20, 36, 12, 0.1, 0.1, 0.1)
        oloss, ologits, ograds = _oracle_step(oracle, batch, masks)
        e = _errors((float(loss.detach()), ologits, grads), (oloss, ologits, ograds))
        print("consecutive call %d: loss rel %.1e, worst grad rel-L2 %.2e at %s" % (call, e[1], e[2], e[3]))
        assert e[1] <= LOSS_REL and e[2] <= GRAD_REL_L2, e
        print("  %s" % _assert_grads((None, None, grads), (None, None, ograds), "consecutive call %d" % call))
        other = DM.StepMasks("uc2", BASE_SEED, 3 - call, 4, 20, 36, 12, 0.1, 0.1, 0.1)
        assert not _within(_errors((float(loss.detach()), ologits, grads), _oracle_step(oracle, batch, other)))


@pytest.mark.parametrize("T,V", [(20, 36), (40, 100)])
def test_m3p_training_step_matches_oracle_with_engine_masks(T, V):
    g = load_golden("m3p_small.npz")
    config = golden_config(g, m3p=True)
    model, oracle = _m3p_build(config, seed=9)
    batch = make_batch(3, seq_len=T, num_boxes=V, vocab_size=config.n_words, num_locs=5, l2_normalize=True, seed=77)
    _parity("m3p", model, oracle, batch, config.n_heads, negative=(T, V) == (20, 36))
