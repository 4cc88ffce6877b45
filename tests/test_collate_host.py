"""Host side of the device collate (clg_vqa_amd.records.pack_records, synthetic.make_records, the parsed binding of the
three vl_collate_* entry points).  CPU only; the kernels themselves are tested in test_gpu_collate.py."""
import copy
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from helpers import load_golden
from clg_vqa_amd import _lib, records, synthetic


def fixture_records(g):
    out = []
    for i in range(3):
        w, h = g["rec%d_wh" % i]
        out.append(dict(features=g["rec%d_features" % i].astype(np.float32), boxes=g["rec%d_boxes" % i], img_w=w, img_h=h,
                        tokens=g["rec%d_tokens" % i].tolist(), labels=[int(g["rec%d_label" % i])], scores=[1.0],
                        question_id=7000 + i))
    return out


def _pack(recs, g, **kw):
    return records.pack_records(recs, int(g["seq_len"]), int(g["region_len"]), 7, int(g["num_labels"]), **kw)


def test_pack_records_lays_the_fixture_records_out_bit_for_bit():
    g = load_golden("records.npz")
    recs = fixture_records(g)
    blob, meta = _pack(recs, g, batch_index=5)
    assert blob.dtype == torch.uint8 and blob.dim() == 1 and blob.numel() >= meta["nbytes"]
    names = ["feats", "boxes", "row_off", "whp", "tok", "tok_off", "labels", "scores", "qid"]
    assert list(meta["offsets"]) == names
    offs = [meta["offsets"][n] for n in names]
    assert all(o % 256 == 0 for o in offs) and meta["nbytes"] % 256 == 0
    assert offs == sorted(offs) and offs[0] == 0 and offs[-1] + 8 * 3 <= meta["nbytes"]
    v = {k: t.numpy() for k, t in records.packed_views((blob, meta)).items()}
    n = [len(r["boxes"]) for r in recs]
    nt = [len(r["tokens"]) for r in recs]
    assert (meta["B"], meta["n_rows"], meta["n_tok"], meta["Lb"], meta["feat_dim"], meta["batch_index"]) == (
        3, sum(n), sum(nt), 1, 2048, 5)
    np.testing.assert_array_equal(v["row_off"], np.concatenate([[0], np.cumsum(n)]))
    np.testing.assert_array_equal(v["tok_off"], np.concatenate([[0], np.cumsum(nt)]))
    assert v["row_off"].dtype == np.int64 and v["tok"].dtype == np.int64 and v["feats"].dtype == np.float32
    np.testing.assert_array_equal(v["feats"], np.concatenate([r["features"] for r in recs]))
    np.testing.assert_array_equal(v["boxes"], np.concatenate([np.asarray(r["boxes"], dtype=np.float32) for r in recs]))
    np.testing.assert_array_equal(v["tok"], np.concatenate([r["tokens"] for r in recs]))
    w64 = np.array([float(r["img_w"]) for r in recs], dtype=np.float64)
    h64 = np.array([float(r["img_h"]) for r in recs], dtype=np.float64)
    np.testing.assert_array_equal(v["whp"][:, 0], w64.astype(np.float32))
    np.testing.assert_array_equal(v["whp"][:, 1], h64.astype(np.float32))
    np.testing.assert_array_equal(v["whp"][:, 2], (w64 * h64).astype(np.float32))
    np.testing.assert_array_equal(v["labels"], [[r["labels"][0]] for r in recs])
    np.testing.assert_array_equal(v["scores"], np.ones((3, 1), dtype=np.float32))
    np.testing.assert_array_equal(v["qid"], [7000, 7001, 7002])
    assert v["feats"].shape == (sum(n), 2048) and v["boxes"].shape == (sum(n), 4) and v["whp"].shape == (3, 3)


def test_whp_keeps_the_double_product_rounded_once():
    """w * h is formed in double and rounded to fp32 once (box_locations); fl32(w) * fl32(h) in fp32 would differ here."""
    g = load_golden("records.npz")
    recs = copy.deepcopy(fixture_records(g))
    recs[0]["img_w"], recs[0]["img_h"] = 16777217.0 / 4096.0, 4099.0
    w, h = np.float64(recs[0]["img_w"]), np.float64(recs[0]["img_h"])
    assert np.float32(w * h) != np.float32(w) * np.float32(h)  # the case distinguishes the two
    v = records.packed_views(_pack(recs, g))
    assert v["whp"][0, 2].item() == np.float32(w * h)


def test_pack_records_reuses_a_blob_that_is_large_enough():
    g = load_golden("records.npz")
    recs = fixture_records(g)
    blob, meta = _pack(recs, g)
    blob2, meta2 = _pack(recs[:2], g, out=blob)
    assert blob2.data_ptr() == blob.data_ptr() and meta2["nbytes"] < meta["nbytes"]
    small = torch.empty(16, dtype=torch.uint8)
    blob3, meta3 = _pack(recs, g, out=small)
    assert blob3.numel() >= meta3["nbytes"] and blob3.data_ptr() != small.data_ptr()
    for k, t in records.packed_views((blob3, meta3)).items():
        np.testing.assert_array_equal(t.numpy(), records.packed_views(_pack(recs, g))[k].numpy())


def _broken(g, what):
    recs = copy.deepcopy(fixture_records(g))
    V = int(g["region_len"])
    r = recs[1]
    if what == "too many boxes":
        r["boxes"] = np.zeros((V + 1, 4), dtype=np.float32)
        r["features"] = np.zeros((V + 1, 2048), dtype=np.float32)
    elif what == "one token":
        r["tokens"] = [0]
    elif what == "no tokens":
        r["tokens"] = []
    elif what == "label too large":
        r["labels"] = [int(g["num_labels"])]
    elif what == "negative label":
        r["labels"] = [-1]
    elif what == "unequal label lists":
        r["labels"], r["scores"] = [1, 2], [1.0, 0.5]
    elif what == "feature row length":
        r["features"] = np.zeros((len(r["boxes"]), 2044), dtype=np.float32)
    return recs


@pytest.mark.parametrize("what", ["too many boxes", "one token", "no tokens", "label too large", "negative label",
                                  "unequal label lists", "feature row length"])
def test_pack_records_refuses_what_a_kernel_must_never_see(what):
    g = load_golden("records.npz")
    with pytest.raises(ValueError, match="pack_records"):
        _pack(_broken(g, what), g)


def test_a_record_without_boxes_packs():
    g = load_golden("records.npz")
    recs = copy.deepcopy(fixture_records(g))
    recs[1]["boxes"] = np.zeros((0, 4), dtype=np.float32)
    recs[1]["features"] = np.zeros((0, 2048), dtype=np.float32)
    blob, meta = _pack(recs, g)
    v = records.packed_views((blob, meta))
    n0, n2 = len(recs[0]["boxes"]), len(recs[2]["boxes"])
    assert v["row_off"].tolist() == [0, n0, n0, n0 + n2] and meta["n_rows"] == n0 + n2
    np.testing.assert_array_equal(v["feats"].numpy(), np.concatenate([recs[0]["features"], recs[2]["features"]]))
    # ... and a batch of nothing but such records
    blob, meta = _pack([recs[1]], g)
    assert meta["n_rows"] == 0 and records.packed_views((blob, meta))["feats"].shape == (0, 2048)


def test_collate_entry_points_are_bound_from_the_header():
    P, I64 = c_void_p, c_int64
    assert _lib._SIGS["vl_collate_regions"] == (c_int, [P, P, P, P, P, P, P, I64, I64, I64, I64, I64, c_int, P])
    assert _lib._SIGS["vl_collate_text"] == (c_int, [P, P, P, P, P, I64, I64, I64, I64, P])
    assert _lib._SIGS["vl_collate_targets"] == (c_int, [P, P, P, P, P, I64, I64, I64, P])
    for name in ("vl_collate_regions", "vl_collate_text", "vl_collate_targets"):
        assert all(t in (c_void_p, c_int64, c_int) for t in _lib._SIGS[name][1]), name
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().vl_version() == 100


def test_make_records_is_a_pure_function_of_its_seed():
    a = synthetic.make_records(7, seq_len=8, num_boxes=6, num_labels=41, vocab_size=500, feat_dim=64, seed=11)
    b = synthetic.make_records(7, seq_len=8, num_boxes=6, num_labels=41, vocab_size=500, feat_dim=64, seed=11)
    c = synthetic.make_records(7, seq_len=8, num_boxes=6, num_labels=41, vocab_size=500, feat_dim=64, seed=12)
    assert len(a) == 7
    for ra, rb in zip(a, b):
        assert sorted(ra) == sorted(rb)
        for k in ra:
            np.testing.assert_array_equal(np.asarray(ra[k]), np.asarray(rb[k]))
    assert any(ra["tokens"] != rc["tokens"] for ra, rc in zip(a, c))
    n = [len(r["boxes"]) for r in a]
    nt = [len(r["tokens"]) for r in a]
    assert 0 in n and 6 in n and any(0 < x < 6 for x in n)          # empty, full and short box lists
    assert 2 in nt and any(x > 8 for x in nt) and any(2 < x <= 8 for x in nt)  # short, over-long and ordinary questions
    assert all(len(r["labels"]) == 1 and len(r["scores"]) == 1 for r in a)
    assert all(r["features"].shape == (len(r["boxes"]), 64) and r["features"].dtype == np.float32 for r in a)
    d = synthetic.make_records(5, seq_len=8, num_boxes=6, num_labels=41, feat_dim=64, seed=3, box_counts=(0, 1, 3, 6, 6),
                               token_counts=(2, 5, 8, 9, 30), labels_per_record=2)
    assert [len(r["boxes"]) for r in d] == [0, 1, 3, 6, 6] and [len(r["tokens"]) for r in d] == [2, 5, 8, 9, 30]
    assert all(len(set(r["labels"])) == 2 for r in d)


@pytest.mark.parametrize("num_locs,norm", [(7, False), (5, True)])
def test_make_records_feed_the_host_collate(num_locs, norm):
    recs = synthetic.make_records(8, seq_len=8, num_boxes=6, num_labels=41, vocab_size=500, feat_dim=64, seed=5)
    batch = records.collate_records(recs, 8, 6, num_locs, 41, norm_embeddings=norm, feat_dim=64)
    assert [tuple(t.shape) for t in batch[:7]] == [(8, 6, 64), (8, 6, num_locs), (8, 6), (8, 8), (8, 41), (8, 8), (8, 8)]
    feats, loc, imask = batch[0].numpy(), batch[1].numpy(), batch[2].numpy()
    assert np.isfinite(feats).all() and all(torch.isfinite(t.double()).all() for t in batch[3:])
    if norm:  # the documented quirk: the location rows of padding are 0 / 0 -- and nothing else is
        assert np.isnan(loc[imask == 0]).all() and np.isfinite(loc[imask == 1]).all() and (imask == 0).any()
    else:
        assert np.isfinite(loc).all()
    # and the same records pack
    blob, meta = records.pack_records(recs, 8, 6, num_locs, 41, feat_dim=64)
    assert meta["n_rows"] == int(imask.sum())


def test_the_threaded_feature_copy_writes_the_same_blob():
    recs = synthetic.make_records(40, seq_len=8, num_boxes=6, num_labels=41, vocab_size=500, feat_dim=64, seed=8)
    one, meta1 = records.pack_records(recs, 8, 6, 7, 41, feat_dim=64)
    many, meta4 = records.pack_records(recs, 8, 6, 7, 41, feat_dim=64, threads=4)
    assert meta1 == meta4
    for k, t in records.packed_views((one, meta1)).items():
        np.testing.assert_array_equal(t.numpy(), records.packed_views((many, meta4))[k].numpy(), err_msg=k)
