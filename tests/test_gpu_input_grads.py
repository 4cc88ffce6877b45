"""Gradients with respect to the region features and the box locations on the HIP path: the fp32 location product
(vl_loc_linear_bwd_input) against fp64, the feature product (the single-pass bf16 GEMM on a transposed weight image), and the
model surface -- ``features.requires_grad_(True)`` / ``spatials.requires_grad_(True)`` before ``ForwardModelsTrain`` +
``loss.backward()`` -- against the fixture of the real reference and the oracles.  Needs a real MI355X: ``pytest -m gpu``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_check as G  # noqa: E402
import input_grads_ref as R  # noqa: E402
from helpers import TASK_CFG, uc2_cfg_dict  # noqa: E402
from grad_check import GRAD_REL_L2  # noqa: E402  (the project's bound for any gradient tensor behind the bf16 backward)
from oracle import m3p_oracle as Mo  # noqa: E402
from oracle import uc2_oracle as O  # noqa: E402
from clg_vqa_amd import _lib, ops, task_utils  # noqa: E402
from clg_vqa_amd.config import BertConfig  # noqa: E402
from clg_vqa_amd.encoders import BertForVLTasks  # noqa: E402
from clg_vqa_amd.engine import input_grad_feats  # noqa: E402
from clg_vqa_amd.m3p import M3PForVLTasks  # noqa: E402
from clg_vqa_amd.ops import BF16  # noqa: E402
from clg_vqa_amd.synthetic import make_batch, seeded_state_dict  # noqa: E402

DEV = "cuda"
BASE_SEED = 0x5EED ^ 20261017
SENTINEL, GUARD = -777.0, 1024


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,L,H", [(1, 7, 128), (7, 5, 768), (65, 7, 768), (300, 8, 256)])
def test_loc_linear_bwd_input_against_fp64(R_, L, H):
    """dloc[r,l] = sum_h dy[r,h] w[h,l] in fp32 against fp64.  Bound: the error of an fp32 sum of H products is at most
    (number of roundings on the longest path) * 2^-24 * sum_h |dy w| -- here ceil(H / 256) fused quads + 6 butterfly steps,
    under 3e-6 of that sum at H = 768 -- and tests/test_gpu_kernels.py bounds vl_loc_linear_fwd / _bwd with the relative
    constant 1e-5: the same constant, applied to the sum of magnitudes (which is what a relative bound of a summation refers
    to; exact zeros have a zero bound).  One row of dy is zero.  Repeatable to the bit; a guard region behind the output stays
    untouched."""
    dy, w = _rand(R_, H, seed=60 + R_), _rand(H, L, seed=61 + R_)
    dy[R_ // 2] = 0.0
    outs = []
    for rep in range(2):
        buf = torch.full((R_ * L + GUARD,), SENTINEL, device=DEV)
        ops.loc_linear_bwd_input(dy, w, buf, R_, L, H)
        outs.append(buf)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert (outs[0][R_ * L:] == SENTINEL).all()
    got = outs[0][:R_ * L].view(R_, L).double()
    ref = dy.double() @ w.double()
    bound = 1e-5 * (dy.double().abs() @ w.double().abs())
    err = (got - ref).abs()
    print("loc input grad R=%d L=%d H=%d: max err / bound %.3e" % (R_, L, H, (err / bound.clamp_min(1e-300)).max().item()))
    assert torch.isfinite(got).all() and (err <= bound).all()
    assert (got[R_ // 2] == 0).all()


def test_loc_linear_bwd_input_rejects_bad_arguments():
    L_ = _lib.lib()
    dy, w, out = _rand(4, 8, seed=1), _rand(8, 8, seed=2), torch.full((4 * 9,), SENTINEL, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    for args, word in (((dy.data_ptr(), w.data_ptr(), out.data_ptr(), 4, 9, 8), "L <= 8"),
                       ((dy.data_ptr(), w.data_ptr(), out.data_ptr(), 4, 7, 6), "multiple of 4"),
                       ((None, w.data_ptr(), out.data_ptr(), 4, 7, 8), "null"),
                       ((dy.data_ptr(), w.data_ptr(), None, 4, 7, 8), "null")):
        rc = L_.vl_loc_linear_bwd_input(*args, st)
        msg = L_.vl_last_error().decode()
        assert rc < 0 and "vl_loc_linear_bwd_input" in msg and word in msg, (args[3:], rc, msg)
    with pytest.raises(RuntimeError, match="vl_loc_linear_bwd_input"):
        ops.loc_linear_bwd_input(dy, w, out, 4, 9, 8)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()  # nothing was launched


@pytest.mark.parametrize("BV", [6, 300, 2400])
def test_feature_product_against_fp64(BV):
    """dfeats = d(img) . W_img through the engine's helper (transposed bf16 image + the 1-pass GEMM).  The library sends
    products of fewer than 100 tiles (ceil(M / 256) * ceil(N / 192)) through the small-M kernel: BV = 6 (one ragged 64-row
    tile) and BV = 300 (a ragged fifth row tile) both take it; BV = 2400 -- the row count from which F = 2048 reaches the main
    ping-pong kernel is 2305 -- takes the main path with a ragged last row tile (2400 = 9 * 256 + 96).  Against the fp64
    product of the same bf16-rounded operands, with the bound tests/test_gpu_kernels.py uses for a 1-pass vl_gemm_nt
    (products of bf16 values are exact in fp32; only the accumulation differs), at K = 768."""
    F, H = 2048, 768
    assert _lib.lib().vl_gemm_nt_path(BV, F, H, 1, 1) == (2 if BV == 2400 else 3)
    d16, w_hi = _rand(BV, H, seed=70).to(BF16), _rand(H, F, seed=71).to(BF16)
    got = input_grad_feats(d16, w_hi)
    again = input_grad_feats(d16, w_hi)
    torch.cuda.synchronize()
    assert got.shape == (BV, F) and got.dtype == torch.float32 and torch.equal(got, again)
    ref = (d16.double() @ w_hi.double()).float()
    torch.testing.assert_close(got, ref, rtol=2e-5, atol=2e-4 * math.sqrt(H / 256))


# ---------------------------------------------------------------------------------------------------------------------
# model surface
# ---------------------------------------------------------------------------------------------------------------------
def _build(kind, config, seed, with_oracle=True):
    m3p = kind == "m3p"
    model = (M3PForVLTasks if m3p else BertForVLTasks)(config, TASK_CFG, ["TASK15"])
    sd = seeded_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd, strict=True)
    oracle = None
    if with_oracle:
        oracle = (Mo.OracleM3PForVLTasks if m3p else O.OracleUC2ForVLTasks)(config, TASK_CFG, ["TASK15"])
        oracle.load_state_dict({k: v for k, v in sd.items() if k in oracle.state_dict()}, strict=True)
        oracle.eval()
    return model.cuda(), oracle


def _train_step(model, batch, want_feats=True, want_locs=True):
    """The reference's recipe: requires_grad_ on the batch tensors, ForwardModelsTrain, loss.backward()."""
    b = [t.cuda() for t in batch]
    b[0].requires_grad_(want_feats)
    b[1].requires_grad_(want_locs)
    model.zero_grad()
    loss, _ = task_utils.ForwardModelsTrain(model.config, TASK_CFG, "cuda", "TASK15", tuple(b), model, torch.nn.CrossEntropyLoss())
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), b[0].grad, b[1].grad


def _call_step(model, batch, labels, want_feats=False, want_locs=False, **flags):
    """model(...) -> cross entropy -> backward, as the `eng.calls + 1`-th call.  Returns (logits, loss, d features,
    d locations, parameter gradients, (loss tensor, model output))."""
    feats, spat, imask, q, _, tmask, seg = (t.cuda() for t in batch[:7])
    feats.requires_grad_(want_feats)
    spat.requires_grad_(want_locs)
    model.zero_grad()
    out = model(q, feats, spat, "TASK15", seg, tmask, imask, **flags)
    loss = torch.nn.functional.cross_entropy(out[0], labels)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return out[0].detach().clone(), float(loss.detach()), feats.grad, spat.grad, grads, (loss, out)


def _check_input_grad(got, like, ref, what):
    assert got is not None, "%s: .grad is None" % what
    assert got.shape == like.shape and got.dtype == torch.float32 and got.is_cuda, what
    assert torch.isfinite(got).all(), what
    st = G.grad_check(what, got, ref)  # [B, V, F] viewed as [B V, F]: rows = (sample, box)
    rel = st["tensor"]
    print("%s: relative L2 error %.3e (bound %.1e); %s" % (what, rel, GRAD_REL_L2, G.fmt(st)))
    return rel


@pytest.mark.parametrize("kind", ["uc2", "m3p"])
def test_model_input_gradients_match_reference_fixture_and_oracle(kind):
    """eval(): features.grad / spatials.grad have the inputs' shapes, fp32, and lie within GRAD_REL_L2 of the gradients the
    real reference produced (fixture) and of the oracle's (UC2: fp64; M3P: fp32, its oracle casts to float like the
    reference).  The pooled-row mode of the last layer is on (the shipped configuration)."""
    g = R.load_case(kind)
    model, oracle = _build(kind, R.case_config(g, kind == "m3p"), int(g["seed"]))
    assert model.engine.stack.pooled_only
    model.eval()
    batch = R.case_batch(g)
    loss, dfeats, dlocs = _train_step(model, batch)
    assert abs(loss - float(g["loss"])) <= 2e-4 * abs(float(g["loss"]))
    _, _, of, ol = R.oracle_input_grads(oracle, batch, double=kind != "m3p")
    for name, got, like, oref in (("features", dfeats, batch[0], of), ("spatials", dlocs, batch[1], ol)):
        _check_input_grad(got, like, g[name + "_grad"], "%s %s.grad vs the reference fixture" % (kind, name))
        _check_input_grad(got, like, oref, "%s %s.grad vs the oracle" % (kind, name))
    if kind == "m3p":  # rows beyond len_img + len_txt are multiplied by the row mask: exactly zero
        assert not dfeats[1, 6:].any() and not dlocs[1, 6:].any() and dfeats[1, :6].any(dim=-1).all()


def _uc2_small(seed, n_layers=2, vocab=800):
    return _build("uc2", BertConfig.from_dict(uc2_cfg_dict(hidden=128, heads=4, inter=512, n_layers=n_layers, vocab=vocab)), seed,
                  with_oracle=False)[0]


def test_nothing_else_moves_in_a_training_step_with_dropout():
    """train(), dropout on, same seed and call count: with and without requires_grad on the inputs the logits, the loss and
    every parameter gradient are bit-equal."""
    model = _uc2_small(seed=41)
    B, T, V = 5, 9, 11
    batch = make_batch(B, seq_len=T, num_boxes=V, vocab_size=800, seed=400)
    batch[2][0, V - 2:] = 0
    labels = torch.arange(B, device=DEV) * 7 % 1842
    eng = model.engine
    eng.base_seed = BASE_SEED
    model.train()
    runs = {}
    for want in (True, False):
        eng.calls = 0
        runs[want] = _call_step(model, batch, labels, want_feats=want, want_locs=want)
        assert eng.calls == 1
    (lg1, ls1, f1, l1, g1, _), (lg0, ls0, f0, l0, g0, _) = runs[True], runs[False]
    assert f0 is None and l0 is None and f1 is not None and l1 is not None
    assert f1.shape == (B, V, 2048) and l1.shape == (B, V, 7) and f1.abs().sum() > 0 and l1.abs().sum() > 0
    assert torch.equal(lg1, lg0) and ls1 == ls0
    assert g1.keys() == g0.keys() and len(g1) > 30
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n
    # dropout really was on: the same call in eval() gives other logits
    model.eval()
    assert not torch.equal(_call_step(model, batch, labels)[0], lg1)


@pytest.mark.parametrize("kind", ["uc2", "m3p"])
def test_frozen_model_and_single_input_requests(kind):
    """All parameters frozen and only one input requiring a gradient: backward runs, that gradient equals the one of the
    unfrozen run with both requested bit for bit, the other stays None."""
    g = R.load_case(kind)
    model, _ = _build(kind, R.case_config(g, kind == "m3p"), int(g["seed"]), with_oracle=False)
    model.eval()
    batch = R.case_batch(g)
    labels = torch.arange(batch[0].shape[0], device=DEV) * 7 % 1842
    _, _, f_all, l_all, grads, _ = _call_step(model, batch, labels, want_feats=True, want_locs=True)
    assert len(grads) > 20
    _, _, f_only, l_none, _, _ = _call_step(model, batch, labels, want_feats=True)     # unfrozen, features only
    _, _, f_none, l_only, _, _ = _call_step(model, batch, labels, want_locs=True)      # unfrozen, locations only
    assert l_none is None and f_none is None
    assert torch.equal(f_only, f_all) and torch.equal(l_only, l_all)
    for p in model.parameters():
        p.requires_grad_(False)
    _, _, f_frozen, l_none, grads, _ = _call_step(model, batch, labels, want_feats=True)
    assert not grads and l_none is None and torch.equal(f_frozen, f_all)
    _, _, f_none, l_frozen, grads, _ = _call_step(model, batch, labels, want_locs=True)
    assert not grads and f_none is None and torch.equal(l_frozen, l_all)
    # nothing requires a gradient at all: an inference call, no graph
    feats, spat, imask, q, _, tmask, seg = (t.cuda() for t in batch[:7])
    assert not model(q, feats, spat, "TASK15", seg, tmask, imask)[0].requires_grad


def test_padded_boxes():
    """image_mask with zeros.  M3P masks its [image ; text] stream by length: with len_img + len_txt < V the boxes beyond that
    length are multiplied by the row mask and their gradient rows are exactly zero (padded boxes inside the length keep a
    gradient, as in the reference).  UC2 keeps masked boxes as rows of the stream: compared with the oracle."""
    g = R.load_case("m3p")
    config = R.case_config(g, True)
    model, oracle = _build("m3p", config, seed=7)
    model.eval()
    B, T, V = 3, 7, 9
    batch = list(make_batch(B, seq_len=T, num_boxes=V, vocab_size=config.n_words, num_locs=5, l2_normalize=True, seed=78,
                            full_length=True))
    batch[2][1, 2:] = 0                                   # sample 1: 2 boxes ...
    batch[3][1, 3:], batch[3][1, 2] = 1, 2                # ... and 3 tokens: length 5 < V
    batch[5] = (batch[3] != 1).long()
    batch[2][2, V - 4:] = 0                               # sample 2: 5 boxes + 7 tokens = 12 >= V: every box row is live
    _, dfeats, dlocs = _train_step(model, batch)
    assert not dfeats[1, 5:].any() and not dlocs[1, 5:].any()
    assert dfeats[1, :5].any(dim=-1).all() and dfeats[2].any(dim=-1).all() and dlocs[2].any(dim=-1).all()
    _, _, of, ol = R.oracle_input_grads(oracle, batch, double=False)
    assert not of[1, 5:].any() and not ol[1, 5:].any()
    _check_input_grad(dfeats, batch[0], of, "m3p padded: features.grad vs the oracle")
    _check_input_grad(dlocs, batch[1], ol, "m3p padded: spatials.grad vs the oracle")

    g = R.load_case("uc2")
    model, oracle = _build("uc2", R.case_config(g, False), seed=8)
    model.eval()
    batch = make_batch(B, seq_len=T, num_boxes=V, vocab_size=1000, seed=79)
    batch[2][0, V - 3:] = 0
    batch[2][2, 1:4] = 0
    _, dfeats, dlocs = _train_step(model, batch)
    _, _, of, ol = R.oracle_input_grads(oracle, batch)
    _check_input_grad(dfeats, batch[0], of, "uc2 padded: features.grad vs the fp64 oracle")
    _check_input_grad(dlocs, batch[1], ol, "uc2 padded: spatials.grad vs the fp64 oracle")


def test_sft_mask_on_the_feature_projection():
    """A pruning mask on image_embeddings: the gradient is that of the masked model (the prepared weight image the forward
    pass used), as in the reference with prune applied -- against the fp64 oracle with the same mask."""
    from torch.nn.utils import prune
    g = R.load_case("uc2")
    model, oracle = _build("uc2", R.case_config(g, False), seed=9)
    name = "bert.embeddings.image_embeddings"
    mod, omod = dict(model.named_modules())[name], dict(oracle.named_modules())[name]
    mask = (torch.rand(mod.weight.shape, generator=torch.Generator().manual_seed(4321)) < 0.59).float()
    mod.weight.data.mul_(mask.cuda())
    omod.weight.data.mul_(mask)
    prune.CustomFromMask.apply(mod, "weight", mask=mask.cuda())
    prune.CustomFromMask.apply(omod, "weight", mask=mask)
    # the masked-out weights are made non-zero again: only the mask keeps them out of the product
    mod.weight_orig.data.add_((1 - mask.cuda()) * 0.05)
    omod.weight_orig.data.add_((1 - mask) * 0.05)
    model.eval()
    batch = make_batch(3, seq_len=7, num_boxes=9, vocab_size=1000, seed=80)
    _, dfeats, dlocs = _train_step(model, batch)
    _, _, of, ol = R.oracle_input_grads(oracle, batch)
    _check_input_grad(dfeats, batch[0], of, "SFT: features.grad vs the fp64 oracle with the same mask")
    _check_input_grad(dlocs, batch[1], ol, "SFT: spatials.grad vs the fp64 oracle with the same mask")
    gw = mod.weight_orig.grad
    assert gw is not None and (gw[mask.cuda() == 0] == 0).all()


def test_composition_with_per_layer_outputs_and_retain_graph_error():
    """output_all_encoded_layers=True with features.requires_grad gives the same features.grad bits as without the flag (both
    dense: a tapped call runs the last layer dense, so the plain call is made dense too, as in
    tests/test_gpu_attention_maps.py); a second backward through the same graph still raises the retain_graph error."""
    model = _uc2_small(seed=43)
    model.eval()
    model.engine.stack.pooled_only = False
    B, T, V = 3, 7, 9
    batch = make_batch(B, seq_len=T, num_boxes=V, vocab_size=800, seed=401)
    labels = torch.arange(B, device=DEV) * 7 % 1842
    feats, spat, imask, q, _, tmask, seg = (t.cuda() for t in batch[:7])
    feats.requires_grad_(True)
    spat.requires_grad_(True)
    model.zero_grad()
    out = model(q, feats, spat, "TASK15", seg, tmask, imask, output_all_encoded_layers=True)
    assert len(out) == 6 and not out[4][0].requires_grad
    loss = torch.nn.functional.cross_entropy(out[0], labels)
    loss.backward(retain_graph=True)  # (torch keeps its own nodes; the native trunk releases its activations regardless)
    lg1, ls1, f1, l1 = out[0].detach().clone(), float(loss.detach()), feats.grad.clone(), spat.grad.clone()
    with pytest.raises(RuntimeError, match="retain_graph / double backward are not supported"):
        loss.backward()
    torch.cuda.synchronize()
    lg0, ls0, f0, l0, _, _ = _call_step(model, batch, labels, want_feats=True, want_locs=True)
    assert torch.equal(lg1, lg0) and ls1 == ls0
    assert torch.equal(f1, f0) and torch.equal(l1, l0) and f0.abs().sum() > 0


def test_fused_adamw_with_its_word_gradient_sink():
    """FusedAdamW installs its word-gradient sink and per-layer gradient sinks: the input gradients are the same bits as
    without the optimizer, and the step still runs."""
    from clg_vqa_amd.optim import FusedAdamW
    plain, fused = _uc2_small(seed=45), _uc2_small(seed=45)
    plain.eval()
    fused.eval()
    opt = FusedAdamW(fused, base_lr=1e-3, weight_decay=0.1, correct_bias=True, max_grad_norm=1.0)
    assert fused.engine.word_grad_sink is not None
    B, T, V = 4, 9, 11
    batch = make_batch(B, seq_len=T, num_boxes=V, vocab_size=800, seed=402)
    _, fp, lp = _train_step(plain, batch)
    b = [t.cuda() for t in batch]
    b[0].requires_grad_(True)
    b[1].requires_grad_(True)
    loss, _ = task_utils.ForwardModelsTrain(fused.config, TASK_CFG, "cuda", "TASK15", tuple(b), fused, torch.nn.CrossEntropyLoss())
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(b[0].grad, fp) and torch.equal(b[1].grad, lp)
    assert torch.isfinite(loss)


def test_unsupported_location_width_raises_in_forward():
    model = _uc2_small(seed=47)
    model.eval()
    B, T, V = 2, 6, 4
    feats, spat, imask, q, _, tmask, seg = (t.cuda() for t in make_batch(B, seq_len=T, num_boxes=V, vocab_size=800, seed=403)[:7])
    loc9 = torch.rand(B, V, 9, device=DEV).requires_grad_(True)
    calls = model.engine.calls
    with pytest.raises(ValueError, match="box locations"):
        model(q, feats, loc9, "TASK15", seg, tmask, imask)
    assert model.engine.calls == calls  # refused before anything was launched
    # non-contiguous inputs: the gradient comes back in the input's own shape
    wide = torch.zeros(B, V, 2 * 2048, device=DEV)
    wide[..., ::2] = feats
    wide.requires_grad_(True)
    spat_t = spat.transpose(0, 1).contiguous().requires_grad_(True)
    f_nc, s_nc = wide[..., ::2], spat_t.transpose(0, 1)
    assert not f_nc.is_contiguous() and not s_nc.is_contiguous()
    labels = torch.arange(B, device=DEV)
    loss = torch.nn.functional.cross_entropy(model(q, f_nc, s_nc, "TASK15", seg, tmask, imask)[0], labels)
    loss.backward()
    fc, sc = feats.clone().requires_grad_(True), spat.clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(model(q, fc, sc, "TASK15", seg, tmask, imask)[0], labels).backward()
    assert wide.grad.shape == wide.shape and torch.equal(wide.grad[..., ::2], fc.grad) and not wide.grad[..., 1::2].any()
    assert spat_t.grad.shape == spat_t.shape and torch.equal(spat_t.grad.transpose(0, 1), sc.grad)
