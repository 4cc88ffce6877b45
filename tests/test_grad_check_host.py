"""tests/grad_check.py on the CPU: faults planted into the oracle's own gradients pass the per-tensor 4e-2 the suite used to
apply and fail grad_check; the gradients of the reference-side noise model (tests/precision_study.py: engine_noise_model) pass
every bound; exact zeros on both sides score 0 and a NaN fails."""
import math

import pytest
import torch

import grad_check as G
import precision_study as PS
from clg_vqa_amd.synthetic import make_batch

SHAPES = [(3, 7, 9), (8, 20, 36)]
FFN1 = "bert.encoder.layer.1.intermediate.dense.weight"   # 3072 x 768
FFN2 = "bert.encoder.layer.3.output.dense.weight"         # 768 x 3072
BIAS = "bert.encoder.layer.2.attention_output.dense.bias"  # 768
WORD = "bert.embeddings.word_embeddings.weight"


@pytest.fixture(scope="module", params=SHAPES, ids=["B%d_T%d_V%d" % s for s in SHAPES])
def grads(request):
    """(oracle gradients, noise model gradients) at 2 layers, hidden 768; computed once per shape and never modified."""
    B, T, V = request.param
    torch.manual_seed(0)
    model = PS.build(2, 2000, 40)
    batch = make_batch(B, seq_len=T, num_boxes=V, vocab_size=2000, seed=500)
    batch[2][0, V - 3:] = 0
    return PS.noise_model_grads(model, batch)


def _rejected(name, bad, ref, statistic):
    """The planted fault passes the old per-tensor check and fails grad_check on `statistic`."""
    old = G.old_rel_l2(bad, ref)
    st = G.grad_stats(bad, ref)
    print("%s: old per-tensor rel-L2 %.2e (passes 4e-2); %s" % (name, old, G.fmt(st)))
    assert old <= G.GRAD_REL_L2, (name, old)
    assert statistic in [v[0] for v in G.violations(st)], (name, statistic, G.fmt(st))
    with pytest.raises(AssertionError, match=statistic + " statistic"):
        G.grad_check(name, bad, ref)
    return st


def test_planted_faults_pass_the_old_check_and_fail_grad_check(grads):
    ref, _ = grads
    assert ref[FFN1].shape == (3072, 768) and ref[FFN2].shape == (768, 3072) and ref[BIAS].shape == (768,)
    # a ragged last tile / an epilogue lane that is not stored
    bad = ref[FFN1].clone()
    bad[-1] = 0
    st = _rejected("last row of a 3072 x 768 weight gradient zeroed", bad, ref[FFN1], "row")
    assert st["where"]["row"][0] == 3071
    bad = ref[FFN2].clone()
    bad[:, -1] = 0
    st = _rejected("last column of a 768 x 3072 weight gradient zeroed", bad, ref[FFN2], "column")
    assert st["where"]["column"][0] == 3071
    # a row map off by one
    bad = ref[FFN1].clone()
    bad[[17, 18]] = bad[[18, 17]]
    _rejected("two rows of a 3072-row gradient swapped", bad, ref[FFN1], "row")
    # a dropped column-sum partial
    r = ref[BIAS]
    rms = r.double().norm().item() / math.sqrt(r.numel())
    # (|r_j| <= rms / 2: negating it moves the tensor by 2 |r_j| / ||r|| <= 1 / sqrt(768), which the old check lets through)
    j = int(torch.where(r.abs() <= 0.5 * rms, r.abs(), torch.zeros_like(r)).argmax())
    assert 0.25 * rms < abs(float(r[j])) <= 0.5 * rms
    bad = r.clone()
    bad[j] = -bad[j]
    st = _rejected("one element of a 768-long bias gradient negated", bad, r, "element")
    assert st["where"]["element"][0] == j
    # a 1 / (1 - p) or C / B factor that is slightly wrong
    _rejected("a bias gradient x 0.98", ref[BIAS] * 0.98, ref[BIAS], "scale")
    _rejected("a weight gradient x 1.02", ref[FFN1] * 1.02, ref[FFN1], "scale")


def test_planted_fault_in_a_feature_gradient():
    """One (sample, box) row of a [B, V, 2048] feature gradient zeroed; B V = 800 rows, so the old check sees 1 / sqrt(800) = 3.5e-2."""
    r = torch.randn(8, 100, 2048, generator=torch.Generator().manual_seed(3))
    bad = r.clone()
    bad[5, 97] = 0
    st = _rejected("one (sample, box) row of a feature gradient zeroed", bad, r, "row")
    assert st["where"]["row"][0] == 5 * 100 + 97


def test_noise_model_gradients_pass_every_bound(grads):
    """The bounds are not so tight that honest rounding fails them."""
    ref, noisy = grads
    assert set(noisy) == set(ref) and len(ref) > 50
    worst = G.check_grads(noisy, ref, "noise model")
    print(worst)
    assert worst["tensor"][0] > 1e-3 and worst["row"][0] > 5e-3  # the model does round


def test_exact_zeros_score_zero_and_nan_fails(grads):
    ref, _ = grads
    r = ref[WORD]
    untouched = ~r.any(dim=1)
    assert untouched.sum() > 1000 and (~untouched).sum() > 5  # most rows of the table saw no token
    st = G.grad_check("identical", r.clone(), r)
    assert all(st[k] == 0.0 for k in G.STATS)
    # an SFT-masked gradient: exact zeros on both sides stay at 0, whatever else the tensor holds
    mask = (torch.rand(ref[FFN1].shape, generator=torch.Generator().manual_seed(1)) < 0.59).double()
    st = G.grad_check("masked", ref[FFN1] * mask, ref[FFN1] * mask)
    assert st["row"] == 0.0 and st["column"] == 0.0
    mask[7] = 0  # a whole row masked away
    st = G.grad_check("masked row", ref[FFN1] * mask, ref[FFN1] * mask)
    assert st["row"] == 0.0
    # all zero on both sides / all zero in the reference only
    z = torch.zeros(4, 5)
    assert G.within(G.grad_stats(z, z))
    nz = z.clone()
    nz[1, 2] = 1e-30
    assert not G.within(G.grad_stats(nz, z))
    # something in an untouched row
    bad = r.clone()
    bad[int(untouched.nonzero()[0]), 3] = float(r.abs().max())
    assert "row" in [v[0] for v in G.violations(G.grad_stats(bad, r))]
    with pytest.raises(AssertionError, match="written into an untouched row"):
        G.grad_check("written into an untouched row", bad, r)
    # NaN anywhere: a 2-D and a 1-D tensor
    for name, t in ((FFN1, ref[FFN1]), (BIAS, ref[BIAS])):
        bad = t.clone()
        bad.view(-1)[11] = float("nan")
        with pytest.raises(AssertionError):
            G.grad_check(name, bad, t)
        assert len(G.violations(G.grad_stats(bad, t))) >= 3
    # the key bias goes by its absolute rule, in both naming schemes
    q = {"a.attention_self.key.bias": torch.full((8,), 1e-3), "a.attention_self.query.bias": torch.ones(8),
         "b.k_lin.bias": torch.zeros(8), "b.q_lin.bias": torch.ones(8)}
    G.check_grads(q, {k: torch.zeros(8) if "key" in k or "k_lin" in k else v for k, v in q.items()})
    q["b.k_lin.bias"] = torch.full((8,), 0.1)
    with pytest.raises(AssertionError, match="k_lin.bias"):
        G.check_grads(q, {k: torch.zeros(8) if "key" in k or "k_lin" in k else v for k, v in q.items()})
