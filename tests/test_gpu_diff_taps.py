"""Differentiable per-layer hidden states (``model.differentiable_encoded_layers``) on the HIP path: the LayerNorm backward
with a second addend (vl_ln_bwd_add) against its own unfused form and fp64 math, and losses on ``encoded_layers_t`` /
``encoded_layers_v`` through ``loss.backward()`` against the float64 autograd of the unmodified oracle
(tests/diff_taps_ref.py).  Needs a real MI355X: ``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import diff_taps_ref as R  # noqa: E402
import dropout_masks as DM  # noqa: E402
import grad_check as G  # noqa: E402
from helpers import TASK_CFG, uc2_cfg_dict  # noqa: E402
from grad_check import GRAD_REL_L2  # noqa: E402  (the project's bound for any gradient tensor behind the bf16 backward)
from oracle import uc2_oracle as O  # noqa: E402
from clg_vqa_amd import ops  # noqa: E402
from clg_vqa_amd.config import BertConfig  # noqa: E402
from clg_vqa_amd.encoders import BertForVLTasks  # noqa: E402
from clg_vqa_amd.ops import BF16  # noqa: E402
from clg_vqa_amd.synthetic import make_batch, seeded_state_dict  # noqa: E402

DROPOUT_GRAD_REL_L2 = GRAD_REL_L2  # the dropout-on parity tests use the same bound
DEV = "cuda"
BASE_SEED = 0x5EED ^ 20261018


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# kernel: vl_ln_bwd_add against vl_ln_bwd of the pre-added gradient, and against fp64
# ---------------------------------------------------------------------------------------------------------------------
LN_SEED = 4242 * 4096 + 4
# (name, keyword arguments of the forward / backward call, rows of the dy buffer or None = R)
LN_FORMS = [("plain", {}, None),
            ("dropout", dict(p_pre=0.1, seed=LN_SEED), None),
            ("strided", dict(p_pre=0.1, seed=LN_SEED, orig_row_stride=12), None),  # the compact rows of a pooled layer
            ("rowmap", dict(p_post=0.1, seed=LN_SEED, group=37, out_stride=50, out_off=13), 50)]  # the embeddings' row map


def _ln_bwd(fn, lead, z, mean, rstd, gamma, Rr, H, kw):
    dz, d16, d32 = torch.empty(Rr, H, device=DEV), torch.empty(Rr, H, dtype=BF16, device=DEV), torch.empty(Rr, H, device=DEV)
    dg, db, dbias = torch.empty(H, device=DEV), torch.empty(H, device=DEV), torch.empty(H, device=DEV)
    fn(*lead, z, mean, rstd, gamma, dz, d16, d32, dg, db, dbias, ops.ln_bwd_ws(Rr, H, DEV), Rr, H, **kw)
    return dict(dz=dz, dt=d16, dpre32=d32, dgamma=dg, dbeta=db, dbias=dbias)


@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("form,kw,dy_rows", LN_FORMS, ids=[f[0] for f in LN_FORMS])
def test_ln_bwd_add_equals_the_unfused_form_and_fp64(H, form, kw, dy_rows):
    """R = 37 rows (10 workgroups of 4 waves, the last one ragged; 4 rows per trip and wave never fill).  vl_ln_bwd_add(dy, add)
    is bit-equal in dz, the bf16 dt, the fp32 dpre and the reduced dgamma / dbeta / bias gradient to vl_ln_bwd(dy + add) with the
    sum taken in fp32 by torch; with a null addend it is bit-equal to vl_ln_bwd(dy).  Forms: no dropout, p_pre = 0.1, the same on
    strided rows (orig_row_stride 12), and the embeddings' row map with p_post = 0.1 (dy and the addend are read through the map).
    Then against fp64 math with the restated masks, at the tolerances of test_layernorm_forward_backward
    (tests/test_gpu_kernels.py) / test_layernorm_pre_dropout_mask_and_values (tests/test_gpu_dropout.py)."""
    Rr, eps = 37, 1e-5
    Mout = dy_rows or Rr
    y, resid = _rand(Rr, H, seed=17), _rand(Rr, H, seed=18)
    gamma, beta = 1 + 0.1 * _rand(H, seed=20), 0.1 * _rand(H, seed=21)
    z, out = y.clone(), torch.zeros(Mout, H, device=DEV)
    mean, rstd = torch.empty(Rr, device=DEV), torch.empty(Rr, device=DEV)
    ops.ln_fwd(z, resid, None, gamma, beta, eps, out, None, None, mean, rstd, Rr, H, **kw)
    dy, add = _rand(Mout, H, seed=22), _rand(Mout, H, seed=23, scale=0.7)
    add[Mout // 2] = 0.0
    fused = _ln_bwd(ops.ln_bwd_add, (dy, add), z, mean, rstd, gamma, Rr, H, kw)
    unfused = _ln_bwd(ops.ln_bwd, (dy + add,), z, mean, rstd, gamma, Rr, H, kw)
    null = _ln_bwd(ops.ln_bwd_add, (dy, None), z, mean, rstd, gamma, Rr, H, kw)
    plain = _ln_bwd(ops.ln_bwd, (dy,), z, mean, rstd, gamma, Rr, H, kw)
    torch.cuda.synchronize()
    for k in fused:
        assert torch.equal(fused[k], unfused[k]), "%s: vl_ln_bwd_add(dy, add) != vl_ln_bwd(dy + add)" % k
        assert torch.equal(null[k], plain[k]), "%s: vl_ln_bwd_add(dy, NULL) != vl_ln_bwd(dy)" % k
    assert not torch.equal(fused["dz"], plain["dz"])  # the addend does arrive
    # fp64
    p_pre, p_post, os_ = kw.get("p_pre", 0.0), kw.get("p_post", 0.0), kw.get("orig_row_stride", 1)
    m_pre = torch.from_numpy(DM.ln_pre_mask(kw.get("seed", 0), Rr, H, p_pre, orig_row_stride=os_)).to(DEV).double()
    m_post = torch.from_numpy(DM.ln_post_mask(kw.get("seed", 0), Rr, H, p_post)).to(DEV).double()
    rows = torch.arange(Rr, device=DEV)
    orow = (rows // kw["group"]) * kw["out_stride"] + kw["out_off"] + rows % kw["group"] if "group" in kw else rows
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    zr = y64 * m_pre + resid.double()
    zr.retain_grad()
    ref = torch.nn.functional.layer_norm(zr, (H,), g64, b64, eps) * m_post
    torch.testing.assert_close(out[orow].double(), ref.detach(), rtol=1e-5, atol=1e-5)
    ref.backward((dy.double() + add.double())[orow])
    torch.testing.assert_close(fused["dz"].double(), zr.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(fused["dpre32"].double(), y64.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(fused["dt"].float(), fused["dpre32"], rtol=2 ** -7, atol=1e-6)
    torch.testing.assert_close(fused["dgamma"].double(), g64.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(fused["dbeta"].double(), b64.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(fused["dbias"].double(), y64.grad.sum(0), rtol=1e-4, atol=1e-4)


def test_ln_bwd_add_rejects_a_misaligned_addend():
    Rr, H = 8, 128
    t = torch.zeros(Rr * H + 4, device=DEV)
    z, mean, rstd, gamma = torch.zeros(Rr, H, device=DEV), torch.zeros(Rr, device=DEV), torch.ones(Rr, device=DEV), torch.ones(H, device=DEV)
    dz = torch.full((Rr, H), -777.0, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.ln_bwd_add(t[:Rr * H].view(Rr, H), t[1:Rr * H + 1].view(Rr, H), z, mean, rstd, gamma, dz, None, None, None, None, None,
                       ops.ln_bwd_ws(Rr, H, DEV), Rr, H)
    torch.cuda.synchronize()
    assert (dz == -777.0).all()  # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# model: losses on the hidden states against the oracle's autograd
# ---------------------------------------------------------------------------------------------------------------------
B_, T_, V_, H_, NH_, NL_ = 3, 5, 7, 128, 4, 2   # S = 12: no multiple of 8 or 16; 1 + 2 * 2 = 5 hidden states
S_, NHID_ = T_ + V_, 1 + 2 * NL_
VOCAB = 800


def _config():
    return BertConfig.from_dict(uc2_cfg_dict(hidden=H_, heads=NH_, inter=512, n_layers=NL_, vocab=VOCAB))


def _build(seed, with_oracle=True):
    config = _config()
    model = BertForVLTasks(config, TASK_CFG, ["TASK15"])
    sd = seeded_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd, strict=True)
    oracle = None
    if with_oracle:
        oracle = O.OracleUC2ForVLTasks(config, TASK_CFG, ["TASK15"])
        oracle.load_state_dict(sd, strict=True)
        oracle.eval()
    return model.cuda(), oracle


def _inputs(seed=500):
    """(question, features, spatials, segment_ids, input_mask, image_mask): sample 1 has padded text, sample 2 padded boxes."""
    feats, spat, imask, q, _, _, seg = make_batch(B_, seq_len=T_, num_boxes=V_, vocab_size=VOCAB, seed=seed)[:7]
    q, imask = q.clone(), imask.clone()
    q[1, 2], q[1, 3:] = 2, 1          # </s> then pad
    tmask = (q != 1).long()
    imask[2, V_ - 2:] = 0
    assert tmask[1].sum() == 3 and imask[2].sum() == V_ - 2
    return q, feats, spat, seg, tmask, imask


def _native(model, inputs, E, c, taps=None, diff=True, flags=True, retain_hidden0=False, use_logits=True):
    """One forward + tap_loss + backward.  Returns dict(loss, logits, params {name: grad}, features, spatials, hidden0, out)."""
    q, feats, spat, seg, tmask, imask = (t.cuda() for t in inputs)
    feats.requires_grad_(True)
    spat.requires_grad_(True)
    model.differentiable_encoded_layers = diff
    model.zero_grad()
    out = model(q, feats, spat, "TASK15", seg, tmask, imask, **(dict(output_all_encoded_layers=True) if flags else {}))
    if flags and diff and retain_hidden0:
        out[4][0].retain_grad()
    if flags and diff and taps != ():
        loss = R.tap_loss(out[0], out[4], out[5], E, c if use_logits else torch.zeros_like(c), T_, taps)
    else:
        loss = (out[0] * c.to(out[0])).sum()
    loss.backward()
    torch.cuda.synchronize()
    seen, params = set(), {}
    for n, p in model.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            params[n] = p.grad
    return dict(loss=float(loss.detach()), logits=out[0].detach(), params=params, features=feats.grad, spatials=spat.grad,
                hidden0=out[4][0].grad if flags and diff and retain_hidden0 else None, out=out)


def _is_key_bias(n):
    return n.endswith("attention_self.key.bias")


def _compare(got, ref, bound, what, structurally_unused=()):
    """Every parameter gradient + features.grad + spatials.grad of `got` against the oracle's through grad_check: within `bound`
    per tensor (relative L2) and within its scale / row / column / element bounds (rows of features.grad and spatials.grad are
    (sample, box)).  Tensors whose oracle gradient is EXACTLY zero -- asserted to be the `structurally_unused` parameters and
    nothing else -- must be exactly zero in the engine too (grad_check: 0 / 0 = 0, x / 0 = inf).  The key biases: no hidden
    state and no logit depends on them (softmax is shift invariant), so the oracle's float64 value is its own rounding noise
    (asserted: below 1e-12 of the query bias's) and there is nothing to be relative to; they are held to the absolute bound
    grad_check uses for them, 1e-2 of the query bias's gradient norm."""
    excluded = set()
    tensors = dict(got["params"])
    tensors["features.grad"], tensors["spatials.grad"] = got["features"], got["spatials"]
    refs = dict(ref["params"])
    refs["features.grad"], refs["spatials.grad"] = ref["features"], ref["spatials"]
    for n, g in tensors.items():
        r = refs[n].double()
        assert g is not None, "%s: %s is None" % (what, n)
        assert g.shape == r.shape and torch.isfinite(g).all(), n
        if _is_key_bias(n):
            qn = refs[n.replace("key.bias", "query.bias")].double().norm().item()
            assert r.norm().item() <= 1e-12 * max(qn, 1e-300), (n, r.norm().item(), qn)
        elif not r.any():
            excluded.add(n)
            assert not g.any(), "%s: %s: the oracle's gradient is exactly zero, the engine's is not" % (what, n)
    assert excluded == set(structurally_unused), (what, sorted(excluded ^ set(structurally_unused)))
    stats = G.check_grads(tensors, refs, what, bounds=dict(tensor=bound))
    worst = stats["tensor"]
    print("%s: %d tensors, worst relative L2 error %.3e at %s (bound %.1e); exactly zero: %d" % (
        what, len(tensors), worst[0], worst[1], bound, len(excluded)))
    print("%s: %s" % (what, stats))
    return worst


@pytest.fixture(scope="module")
def case():
    """Model + oracle + inputs + coefficients, and the oracle's gradients of the full loss (computed once)."""
    model, oracle = _build(seed=21)
    model.eval()
    inputs = _inputs()
    E, c = R.coefficients(B_, S_, H_, NHID_, 1842, seed=77)
    return dict(model=model, oracle=oracle, inputs=inputs, E=E, c=c, ref=R.oracle_tap_grads(oracle, inputs, E, c))


def test_loss_on_every_hidden_state_matches_the_oracle(case):
    """eval(): loss = sum_k <C_k, hs_t[k]> + <D_k, hs_v[k]> + <c, logits> over all 5 hidden states.  Every parameter gradient,
    features.grad and spatials.grad within GRAD_REL_L2 of the oracle's float64 autograd; the hidden states themselves and
    the logits are those of the oracle.  Nothing is structurally unused by this loss."""
    got = _native(case["model"], case["inputs"], case["E"], case["c"])
    ref = case["ref"]
    hs = [torch.cat([t, v], dim=1) for t, v in zip(got["out"][4], got["out"][5])]
    assert len(hs) == NHID_ and all(h.requires_grad and h.shape == (B_, S_, H_) for h in hs)
    for k, h in enumerate(hs):
        assert (h.detach().double().cpu() - ref["hidden"][k]).abs().max().item() <= 1e-3, k
    assert (got["logits"].double().cpu() - ref["logits"]).abs().max().item() <= 1e-3
    assert abs(got["loss"] - float(ref["loss"])) <= 2e-4 * abs(float(ref["loss"])) + 1e-2
    _compare(got, ref, GRAD_REL_L2, "all taps")
    # the attention maps stay detached, and a second backward still raises
    with pytest.raises(RuntimeError, match="retain_graph / double backward are not supported"):
        got["out"][4][2].sum().backward()


@pytest.mark.parametrize("k", [2, 3])
def test_single_tap_in_the_middle_leaves_the_layers_above_exactly_zero(case, k):
    """c = 0 and one hidden state k: 2 = output of layer 0 (its gradient enters LayerNorm 2 of layer 0 through VL_LY_TAP_GRAD_OUT
    while the stack's own gradient there is zero), 3 = output of layer 1's attention sub-layer (VL_LY_TAP_GRAD_X1).  Everything
    above k -- the sub-layers after it, the pooler, the classifier -- receives exactly zero, as in the oracle; what is below
    matches the oracle."""
    ref = R.oracle_tap_grads(case["oracle"], case["inputs"], case["E"], torch.zeros_like(case["c"]), taps=(k,))
    got = _native(case["model"], case["inputs"], case["E"], case["c"], taps=(k,), use_logits=False)
    above = ["bert.encoder.layer.%d." % i for i in range(k, 2 * NL_)] + ["bert.t_pooler.", "clfs_dict."]
    unused = [n for n in got["params"] if n.startswith(tuple(above)) and not _is_key_bias(n)]
    assert len(unused) >= 10 and any(n.startswith("bert.encoder.layer.3.") for n in unused)
    _compare(got, ref, GRAD_REL_L2, "single tap %d" % k, structurally_unused=unused)
    for n, g in got["params"].items():  # (the key bias above k too: exactly zero, not just small)
        if n.startswith(tuple(above)):
            assert not g.any(), n


def test_loss_without_the_logits_term(case):
    """The loss reads hidden states only (no <c, logits> term at all): the trunk's own output receives no gradient, the
    top tap's gradient is the stack's dy.  Same bound."""
    q, feats, spat, seg, tmask, imask = (t.cuda() for t in case["inputs"])
    model = case["model"]
    model.differentiable_encoded_layers = True
    model.zero_grad()
    out = model(q, feats, spat, "TASK15", seg, tmask, imask, output_all_encoded_layers=True)
    e4, e1 = case["E"][4].cuda(), case["E"][1].cuda()
    ((out[4][4] * e4[:, :T_]).sum() + (out[5][4] * e4[:, T_:]).sum() + (out[5][1] * e1[:, T_:]).sum()).backward()
    torch.cuda.synchronize()
    E = case["E"].clone()
    E[1][:, :T_] = 0
    ref = R.oracle_tap_grads(case["oracle"], case["inputs"], E, torch.zeros_like(case["c"]), taps=(1, 4))
    for n in ("bert.encoder.layer.3.output.dense.weight", "bert.encoder.layer.0.attention_self.query.weight",
              "bert.embeddings.image_embeddings.weight", "bert.embeddings.word_embeddings.weight"):
        st = G.grad_check("taps only: " + n, dict(model.named_parameters())[n].grad, ref["params"][n])
        print("taps only: %s relative L2 error %.3e; %s" % (n, st["tensor"], G.fmt(st)))
    assert model.bert.t_pooler.dense.weight.grad is None  # nothing reached the head


def test_training_mode_with_the_engines_masks():
    """train(), dropout on (hidden 0.1, attention 0.1, pooled 0.1): the oracle is fed the masks of the engine's call
    (tests/dropout_masks.py, as tests/test_gpu_dropout.py does), the full loss, the bound of that file."""
    model, oracle = _build(seed=22)
    inputs = _inputs(seed=501)
    E, c = R.coefficients(B_, S_, H_, NHID_, 1842, seed=78)
    call = 3
    eng = model.engine
    eng.base_seed, eng.calls = BASE_SEED, call - 1
    model.train()
    got = _native(model, inputs, E, c)
    assert eng.calls == call
    cfg = model.config
    masks = DM.StepMasks("uc2", BASE_SEED, call, B_, T_, V_, NH_, cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob, 0.1)
    O.set_mask_provider(oracle, masks)
    oracle.train()
    ref = R.oracle_tap_grads(oracle, inputs, E, c)
    assert ("attn_out", 1) in masks.calls and ("emb_box", 0) in masks.calls and ("pooled", 0) in masks.calls
    assert (got["logits"].double().cpu() - ref["logits"]).abs().max().item() <= 1e-3
    _compare(got, ref, DROPOUT_GRAD_REL_L2, "train() with the engine's masks")
    # dropout really was on: the eval() oracle misses the bound
    O.set_mask_provider(oracle, None)
    oracle.eval()
    ref_eval = R.oracle_tap_grads(oracle, inputs, E, c)
    n = "bert.encoder.layer.1.intermediate.dense.weight"
    g = got["params"][n].double().cpu()
    assert (g - ref_eval["params"][n]).norm().item() > DROPOUT_GRAD_REL_L2 * ref_eval["params"][n].norm().item()


def test_token_saliency(case):
    """hs_t[0].retain_grad() + backward: hs_t[0].grad is the [B, T, H] gradient of the loss with respect to the summed token
    embeddings (the embedding output), within GRAD_REL_L2 of the oracle's -- as a whole and on the padded positions of
    sample 1 alone (they are query rows like any other: their gradient is not zero)."""
    got = _native(case["model"], case["inputs"], case["E"], case["c"], retain_hidden0=True)
    sal = got["hidden0"]
    assert sal is not None and sal.shape == (B_, T_, H_) and sal.dtype == torch.float32 and sal.is_cuda
    ref = case["ref"]["hidden0"][:, :T_]
    sal = sal.double().cpu()
    pad = case["inputs"][4][1] == 0
    assert pad.sum() == 2 and ref[1][pad].abs().sum() > 0
    for what, g, r in (("all token positions", sal, ref), ("padded positions", sal[1][pad], ref[1][pad])):
        st = G.grad_check("token saliency, " + what, g, r)  # rows = (sample, token)
        print("token saliency, %s: relative L2 error %.3e (bound %.1e); %s" % (what, st["tensor"], GRAD_REL_L2, G.fmt(st)))


# ---------------------------------------------------------------------------------------------------------------------
# nothing moves when the feature is off
# ---------------------------------------------------------------------------------------------------------------------
def test_nothing_moves_when_the_taps_are_off_or_unused():
    """train(), dropout on, same seed and call count.  A call without the flags (last layer dense, as a tapped call runs it),
    a tapped call with the attribute False, and a tapped call with the attribute True whose loss reads the logits only: the
    logits, the loss, every parameter gradient and both input gradients are bit-equal.  With the attribute False the taps
    have no graph; with it True they do, and under no_grad they do not."""
    model, _ = _build(seed=23, with_oracle=False)
    inputs = _inputs(seed=502)
    E, c = R.coefficients(B_, S_, H_, NHID_, 1842, seed=79)
    eng = model.engine
    eng.base_seed = BASE_SEED
    eng.stack.pooled_only = False
    model.train()
    assert BertForVLTasks.differentiable_encoded_layers is False
    runs = {}
    for name, kw in (("plain", dict(flags=False, diff=False)), ("attribute off", dict(diff=False)),
                     ("attribute on, taps unused", dict(diff=True, taps=()))):
        eng.calls = 0
        runs[name] = _native(model, inputs, E, c, **kw)
        assert eng.calls == 1
    assert not runs["attribute off"]["out"][4][2].requires_grad and not runs["attribute off"]["out"][5][0].requires_grad
    assert runs["attribute on, taps unused"]["out"][4][2].requires_grad
    ref = runs["plain"]
    assert len(ref["params"]) > 40 and all(g is not None for g in ref["params"].values())
    for name in ("attribute off", "attribute on, taps unused"):
        r = runs[name]
        assert torch.equal(r["logits"], ref["logits"]) and r["loss"] == ref["loss"], name
        assert torch.equal(r["features"], ref["features"]) and torch.equal(r["spatials"], ref["spatials"]), name
        for n, g in ref["params"].items():
            assert torch.equal(r["params"][n], g), (name, n)
    # the taps of a used-tap call are the same tensors' values; its gradients differ
    eng.calls = 0
    used = _native(model, inputs, E, c)
    assert torch.equal(used["logits"], ref["logits"])
    assert not torch.equal(used["params"]["bert.encoder.layer.1.output.dense.weight"],
                           ref["params"]["bert.encoder.layer.1.output.dense.weight"])
    model.differentiable_encoded_layers = True
    with torch.no_grad():
        q, feats, spat, seg, tmask, imask = (t.cuda() for t in inputs)
        out = model(q, feats, spat, "TASK15", seg, tmask, imask, output_all_encoded_layers=True)
    assert not out[4][1].requires_grad and not out[0].requires_grad


def test_tap_gradients_reach_the_fused_optimizer_through_its_sinks():
    """FusedAdamW with its per-layer gradient sinks (overlap_reduce=True: the stack writes into the optimizer's arena during
    backward) against the route through autograd's .grad (overlap_reduce=False), one step on the full tap loss: the
    updated parameters are bit-equal, as the existing comparison of the two routes demands
    (test_gradient_exchange_during_backward_is_bit_identical_to_the_plain_path); a step on the logits alone ends elsewhere."""
    from clg_vqa_amd.optim import FusedAdamW
    inputs = _inputs(seed=503)
    E, c = R.coefficients(B_, S_, H_, NHID_, 1842, seed=80)
    after = {}
    for name, overlap, taps in (("sinks", True, None), ("autograd", False, None), ("sinks, logits only", True, ())):
        model, _ = _build(seed=24, with_oracle=False)
        model.eval()
        opt = FusedAdamW(model, base_lr=1e-3, weight_decay=0.1, correct_bias=True, max_grad_norm=1.0, overlap_reduce=overlap)
        assert (model.engine.stack.layer_done_hook is not None) == overlap
        q, feats, spat, seg, tmask, imask = (t.cuda() for t in inputs)
        model.differentiable_encoded_layers = True
        out = model(q, feats, spat, "TASK15", seg, tmask, imask, output_all_encoded_layers=True)
        loss = R.tap_loss(out[0], out[4], out[5], E, c, T_, taps)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        after[name] = opt.arena.param.clone()
        assert torch.isfinite(after[name]).all()
    assert torch.equal(after["sinks"], after["autograd"]), int((after["sinks"] != after["autograd"]).sum())
    assert not torch.equal(after["sinks"], after["sinks, logits only"])
