"""Record -> batch on the device (csrc/collate.hip through records.pack_records / collate_on_device / data.RecordPrefetcher)
against the host routine records.collate_records, which tests/test_records.py pins bit for bit to the real reference
preprocessing (tests/golden/records.npz).  Needs a real MI355X: ``pytest -m gpu``.

Contract: every tensor of the 10-tuple is BIT-EQUAL to the host's, except the L2-normalised features of norm_embeddings.
Those are held to the exact quotient r64 = x / max(||x||, 1e-12) in float64: |dev - r64| <= 3 * 2^-24 * |r64| (derived: one
rounding of the norm + one of the quotient = 2 * 2^-24; the third unit is margin for the fp64 sum's own rounding), padded rows
exactly 0, and against the torch fp32 result |dev - ref| <= (e_ref + 3 * 2^-24) * |r64| with e_ref the reference's own largest
relative distance from r64, computed here."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import TASK_CFG, load_golden, uc2_cfg_dict  # noqa: E402
from clg_vqa_amd import _lib, ops, records, synthetic  # noqa: E402

U = 2.0 ** -24
NAMES = ("feats", "loc", "image_mask", "ids", "target", "input_mask", "segment_ids", "qid", "ix", "dist")


def _fixture_records(g):
    out = []
    for i in range(3):
        w, h = g["rec%d_wh" % i]
        out.append(dict(features=g["rec%d_features" % i].astype(np.float32), boxes=g["rec%d_boxes" % i], img_w=w, img_h=h,
                        tokens=g["rec%d_tokens" % i].tolist(), labels=[int(g["rec%d_label" % i])], scores=[1.0],
                        question_id=7000 + i))
    return out


@functools.lru_cache(maxsize=None)
def _fixture():
    g = load_golden("records.npz")
    C = int(g["num_labels"])
    sem = {(int(j), int(t)): float(v) for (j, t), v in zip(g["semantic_pairs"], g["semantic_vals"])}
    return g, _fixture_records(g), int(g["seq_len"]), int(g["region_len"]), C, records.prior_table(sem, C)


def _on_device(recs, T, V, L, C, norm, prior, F=2048, batch_index=0):
    blob, meta = records.pack_records(recs, T, V, L, C, feat_dim=F, batch_index=batch_index)
    p32 = None if prior is None else records.prior_table_device(prior, "cuda")
    out = records.collate_on_device((blob[:meta["nbytes"]].cuda(), meta), T, V, L, C, padding_index=1, norm_embeddings=norm,
                                    prior32=p32)
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    """the bits, NaN rows included"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                       b.reshape(-1).contiguous().view(torch.uint8))


def _check_layout(dev, host):
    assert len(dev) == len(host) == 10
    for name, d, h in zip(NAMES, dev, host):
        assert d.is_cuda and d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape), name


def _check_normalised_feats(dev_feats, raw_feats, ref_feats, tag):
    """dev_feats / ref_feats [B, V, F] fp32 numpy (device result / torch's CPU F.normalize), raw_feats the padded raw rows."""
    x = raw_feats.astype(np.float64)
    r64 = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
    err = np.abs(dev_feats.astype(np.float64) - r64)
    nz = r64 != 0
    worst = (err[nz] / np.abs(r64[nz])).max() / U
    e_ref = (np.abs(ref_feats.astype(np.float64) - r64)[nz] / np.abs(r64[nz])).max()
    print("%s: normalised features: worst |dev - r64| / |r64| = %.3f * 2^-24 (reference's own: %.3f * 2^-24)"
          % (tag, worst, e_ref / U))
    assert (err <= 3 * U * np.abs(r64)).all(), worst          # (r64 == 0: padded rows and all-zero live rows are exactly 0)
    assert (np.abs(dev_feats.astype(np.float64) - ref_feats.astype(np.float64)) <= (e_ref + 3 * U) * np.abs(r64)).all()
    dead = ~x.any(-1)
    assert dead.any() and (dev_feats[dead] == 0).all() and not np.signbit(dev_feats[dead]).any()


def _check_equal(dev, host, norm, raw_feats=None, tag=""):
    _check_layout(dev, host)
    for name, d, h in zip(NAMES, dev, host):
        if name == "feats" and norm:
            _check_normalised_feats(d.cpu().numpy(), raw_feats, h.numpy(), tag)
        else:
            np.testing.assert_array_equal(d.cpu().numpy(), h.numpy(), err_msg=name)  # (NaN rows compare equal)


def test_fixture_uc2_mode_is_bit_equal_to_the_reference_preprocessing():
    g, recs, T, V, C, prior = _fixture()
    dev = _on_device(recs, T, V, 7, C, False, prior)
    host = records.collate_records(recs, T, V, 7, C, padding_index=1, norm_embeddings=False, prior=prior)
    _check_layout(dev, host)
    d = dict(zip(NAMES, (t.cpu().numpy() for t in dev)))
    np.testing.assert_array_equal(d["feats"], g["uc2_image_feat"])
    np.testing.assert_array_equal(d["loc"], g["uc2_image_loc"])
    np.testing.assert_array_equal(d["image_mask"], g["uc2_image_mask"])
    np.testing.assert_array_equal(d["ids"], g["uc2_input_ids"])
    np.testing.assert_array_equal(d["input_mask"], g["uc2_input_mask"])
    np.testing.assert_array_equal(d["segment_ids"], g["uc2_segment_ids"])
    np.testing.assert_array_equal(d["qid"], g["uc2_question_id"])
    np.testing.assert_array_equal(d["dist"], g["uc2_distances"].astype(np.float32))
    np.testing.assert_array_equal(d["target"], host[4].numpy())
    assert d["ix"].shape == () and int(d["ix"]) == 0


def test_fixture_m3p_mode():
    g, recs, T, V, C, prior = _fixture()
    dev = _on_device(recs, T, V, 5, C, True, prior)
    host = records.collate_records(recs, T, V, 5, C, padding_index=1, norm_embeddings=True, prior=prior)
    _check_layout(dev, host)
    d = dict(zip(NAMES, (t.cpu().numpy() for t in dev)))
    assert np.isnan(g["m3p_image_loc"][1, 4:]).all()  # the short record's padded rows: 0 / 0, reproduced
    np.testing.assert_array_equal(d["loc"], g["m3p_image_loc"])
    np.testing.assert_array_equal(d["image_mask"], g["m3p_image_mask"])
    np.testing.assert_array_equal(d["ids"], g["m3p_input_ids"])
    np.testing.assert_array_equal(d["input_mask"], g["m3p_input_mask"])
    np.testing.assert_array_equal(d["segment_ids"], g["m3p_segment_ids"])
    np.testing.assert_array_equal(d["qid"], g["m3p_question_id"])
    np.testing.assert_array_equal(d["dist"], g["m3p_distances"].astype(np.float32))
    np.testing.assert_array_equal(d["target"], host[4].numpy())
    _check_normalised_feats(d["feats"], g["uc2_image_feat"], g["m3p_image_feat"], "fixture")  # (uc2_image_feat: the raw rows)


@functools.lru_cache(maxsize=None)
def _ragged(C, F):
    """B 5, V 6, T 8: box counts {0, 1, 3, 6, 6}, token counts {2, 5, 8, 9, 30}, two distinct labels per record, one all-zero
    feature row in a live record; + a dense random prior table."""
    recs = synthetic.make_records(5, seq_len=8, num_boxes=6, num_labels=C, vocab_size=1000, feat_dim=F, seed=21,
                                  box_counts=(0, 1, 3, 6, 6), token_counts=(2, 5, 8, 9, 30), labels_per_record=2)
    recs[3]["features"][2, :] = 0.0
    prior = np.random.RandomState(4).uniform(0.05, 1.0, size=(C, C))
    np.fill_diagonal(prior, 0.0)
    raw = records.collate_records(recs, 8, 6, 7, C, feat_dim=F)[0].numpy()
    return recs, prior, raw


@pytest.mark.parametrize("C,F", [(1842, 2048), (41, 64)])
@pytest.mark.parametrize("L,norm", [(7, False), (5, True)])
def test_ragged_batch_matches_the_host_collate(C, F, L, norm):
    recs, prior, raw = _ragged(C, F)
    assert [len(r["boxes"]) for r in recs] == [0, 1, 3, 6, 6] and [len(r["tokens"]) for r in recs] == [2, 5, 8, 9, 30]
    host = records.collate_records(recs, 8, 6, L, C, norm_embeddings=norm, prior=prior, batch_index=3, feat_dim=F)
    dev = _on_device(recs, 8, 6, L, C, norm, prior, F=F, batch_index=3)
    _check_equal(dev, host, norm, raw, "ragged C %d F %d" % (C, F))
    assert (dev[0][3, 2] == 0).all() and raw[3, 3].any()  # the all-zero live row stays exactly 0 (F.normalize gives 0 there)
    assert int(dev[4].count_nonzero()) == 10  # two distinct labels per record
    # without a prior table: an all-zero dist, everything else unchanged
    dev0 = _on_device(recs, 8, 6, L, C, norm, None, F=F, batch_index=3)
    assert dev0[9].shape == (5, C) and int(dev0[9].count_nonzero()) == 0 and not torch.isnan(dev0[9]).any()
    for name, a, b in zip(NAMES[:9], dev0, dev):
        assert _same_bits(a, b), name


def _guarded(shape, dtype):
    """An output pre-filled with a pattern (NaN / -1) that has 64 guard elements behind it: (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), float("nan") if dtype.is_floating_point else -1, dtype=dtype, device="cuda")
    return buf[:n].view(shape), buf


def _pattern(t):
    return torch.isnan(t) if t.dtype.is_floating_point else t == -1


@pytest.mark.parametrize("C,F", [(1842, 2048), (41, 64)])
def test_every_output_element_is_written_and_nothing_behind_it(C, F):
    recs, prior, _ = _ragged(C, F)
    B, V, T, L = 5, 6, 8, 7
    blob, meta = records.pack_records(recs, T, V, L, C, feat_dim=F)
    v = records.packed_views((blob[:meta["nbytes"]].cuda(), meta))
    p32 = records.prior_table_device(prior, "cuda")
    f32, i64 = torch.float32, torch.int64
    outs = dict(feats=_guarded((B, V, F), f32), loc=_guarded((B, V, L), f32), image_mask=_guarded((B, V), i64),
                ids=_guarded((B, T), i64), input_mask=_guarded((B, T), i64), segment_ids=_guarded((B, T), i64),
                target=_guarded((B, C), f32), dist=_guarded((B, C), f32))
    o = {k: t for k, (t, _) in outs.items()}
    # (UC2 mode: no output holds a NaN of its own, and no id / mask is -1)
    ops.collate_regions(v["feats"], v["boxes"], v["row_off"], v["whp"], o["feats"], o["loc"], o["image_mask"], False)
    ops.collate_text(v["tok"], v["tok_off"], o["ids"], o["input_mask"], o["segment_ids"], 1)
    ops.collate_targets(v["labels"], v["scores"], p32, o["target"], o["dist"])
    torch.cuda.synchronize()
    for name, (t, buf) in outs.items():
        assert not _pattern(t).any(), "%s: the pre-fill pattern survives" % name
        assert _pattern(buf[t.numel():]).all(), "%s: guard elements were written" % name
    host = records.collate_records(recs, T, V, L, C, prior=prior, feat_dim=F)
    for name, i in (("feats", 0), ("loc", 1), ("image_mask", 2), ("ids", 3), ("target", 4), ("input_mask", 5),
                    ("segment_ids", 6), ("dist", 9)):
        np.testing.assert_array_equal(o[name].cpu().numpy(), host[i].numpy(), err_msg=name)
    # prior32 = None writes the zeros as well
    dist, buf = _guarded((B, C), f32)
    ops.collate_targets(v["labels"], v["scores"], None, o["target"], dist)
    torch.cuda.synchronize()
    assert int(dist.count_nonzero()) == 0 and not torch.isnan(dist).any() and torch.isnan(buf[dist.numel():]).all()


@pytest.mark.parametrize("L,norm", [(7, False), (5, True)])
def test_two_calls_give_the_same_bits(L, norm):
    recs, prior, _ = _ragged(1842, 2048)
    blob, meta = records.pack_records(recs, 8, 6, L, 1842)
    packed = (blob[:meta["nbytes"]].cuda(), meta)
    p32 = records.prior_table_device(prior, "cuda")
    a = records.collate_on_device(packed, 8, 6, L, 1842, norm_embeddings=norm, prior32=p32)
    b = records.collate_on_device(packed, 8, 6, L, 1842, norm_embeddings=norm, prior32=p32)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, a, b):
        assert _same_bits(x, y), name


def test_record_prefetcher_hands_out_what_the_collate_alone_gives_and_feeds_a_training_step():
    from clg_vqa_amd import task_utils
    from clg_vqa_amd.config import BertConfig
    from clg_vqa_amd.data import RecordPrefetcher
    from clg_vqa_amd.encoders import BertForVLTasks
    from clg_vqa_amd.synthetic import seeded_state_dict
    C, V, T, L = 1842, 36, 20, 7
    prior = np.random.RandomState(9).uniform(0.05, 1.0, size=(C, C))
    np.fill_diagonal(prior, 0.0)
    batches = [synthetic.make_records(4, seq_len=T, num_boxes=V, num_labels=C, vocab_size=1000, seed=100 + i)
               for i in range(3)]
    handed = list(RecordPrefetcher(iter(batches), "cuda", depth=2, seq_len=T, region_len=V, num_locs=L, num_labels=C,
                                   prior=prior))
    torch.cuda.synchronize()
    assert len(handed) == 3
    for i, (recs, dev) in enumerate(zip(batches, handed)):
        alone = _on_device(recs, T, V, L, C, False, prior, batch_index=i)
        for name, x, y in zip(NAMES, dev, alone):
            assert x.is_cuda and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (i, name)
    # one tuple through the model: the inputs are bit-equal to the host path's, so the step is too
    config = BertConfig.from_dict(uc2_cfg_dict(hidden=128, heads=4, inter=512, n_layers=2, vocab=1000))
    model = BertForVLTasks(config, TASK_CFG, ["TASK15"])
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=2))
    model = model.cuda().eval()
    crit = torch.nn.CrossEntropyLoss()
    host = records.collate_records(batches[1], T, V, L, C, prior=prior, batch_index=1)
    _check_equal(handed[1], host, False)
    loss_h, score_h = task_utils.ForwardModelsTrain(config, TASK_CFG, "cuda", "TASK15", tuple(t.to("cuda") for t in host),
                                                    model, crit)
    loss_d, score_d = task_utils.ForwardModelsTrain(config, TASK_CFG, "cuda", "TASK15", handed[1], model, crit)
    torch.cuda.synchronize()
    print("prefetcher step: loss %.6f (host path %.6f)  score %.4f (%.4f)" % (loss_d.item(), loss_h.item(), float(score_d),
                                                                           float(score_h)))
    assert torch.isfinite(loss_d) and torch.equal(loss_d.detach(), loss_h.detach())
    assert torch.equal(torch.as_tensor(score_d), torch.as_tensor(score_h))


def test_unsupported_arguments_are_rejected_and_leave_the_outputs_alone():
    recs, prior, _ = _ragged(41, 64)
    B, V, T, L, C, F = 5, 6, 8, 7, 41, 64
    blob, meta = records.pack_records(recs, T, V, L, C, feat_dim=F)
    v = records.packed_views((blob[:meta["nbytes"]].cuda(), meta))
    lib = _lib.lib()
    feats, _ = _guarded((B, V, 4096 + 64), torch.float32)  # (large enough for whatever a wrongly accepted call would write)
    loc, _ = _guarded((B, V, 16), torch.float32)
    imask, _ = _guarded((B, V), torch.int64)
    ids, _ = _guarded((B, T), torch.int64)
    target, _ = _guarded((B, 8192), torch.float32)
    dist, _ = _guarded((B, 8192), torch.float32)
    p = lambda t: t.data_ptr()  # noqa: E731

    def regions(B_=B, V_=V, F_=F, L_=L):
        return lib.vl_collate_regions(p(v["feats"]), p(v["boxes"]), p(v["row_off"]), p(v["whp"]), p(feats), p(loc), p(imask),
                                      B_, V_, F_, L_, meta["n_rows"], 0, None)

    def targets(B_=B, C_=C):
        return lib.vl_collate_targets(p(v["labels"]), p(v["scores"]), None, p(target), p(dist), B_, meta["Lb"], C_, None)

    def text(B_=B, T_=T):
        return lib.vl_collate_text(p(v["tok"]), p(v["tok_off"]), p(ids), p(ids), p(ids), B_, T_, 1, meta["n_tok"], None)

    for what, call, word in (("F % 4 != 0", lambda: regions(F_=62), "vl_collate_regions"),
                             ("F > 4096", lambda: regions(F_=4100), "vl_collate_regions"),
                             ("L > 8", lambda: regions(L_=9), "vl_collate_regions"),
                             ("B <= 0 (regions)", lambda: regions(B_=0), "vl_collate_regions"),
                             ("C > 4096", lambda: targets(C_=4097), "vl_collate_targets"),
                             ("B <= 0 (targets)", lambda: targets(B_=0), "vl_collate_targets"),
                             ("B <= 0 (text)", lambda: text(B_=-1), "vl_collate_text")):
        rc = call()
        msg = lib.vl_last_error().decode()
        assert rc == -1 and word in msg, (what, rc, msg)
    torch.cuda.synchronize()
    for name, t in (("feats", feats), ("loc", loc), ("image_mask", imask), ("ids", ids), ("target", target), ("dist", dist)):
        assert _pattern(t).all(), "%s was written by a rejected call" % name
