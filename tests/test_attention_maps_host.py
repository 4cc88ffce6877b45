"""Per-layer outputs / attention maps, host side: the oracle helper against the fixture of the real reference
(tests/golden/make_golden_maps.py), and the C ABI of the emitting attention entry points and the stack's taps.  CPU only."""
import ctypes
import re

import numpy as np
import torch

import attention_maps_ref as AR
from helpers import TASK_CFG, golden_config, load_golden
from oracle import uc2_oracle as O
from clg_vqa_amd import _lib
from clg_vqa_amd.synthetic import seeded_state_dict

MAP_KEYS = ("intra_attn", "inter_attn", "queries", "keys")


def maps_inputs(g):
    t = torch.from_numpy
    B, T = g["question"].shape
    return (t(g["question"].astype(np.int64)), t(g["features"].astype(np.float32)), t(g["spatials"].astype(np.float32)),
            torch.zeros(B, T, dtype=torch.int64), t(g["input_mask"].astype(np.int64)), t(g["image_mask"].astype(np.int64)))


def test_oracle_helper_reproduces_the_reference_maps_fixture():
    """Hidden states, probabilities, queries and keys of the hook-based helper against BertForVLTasks(...,
    output_all_encoded_layers=True, output_all_attention_masks=True) of the real reference, to the bound
    test_oracle_golden.py holds the oracle's logits to."""
    g = load_golden("uc2_maps.npz")
    config = golden_config(g)
    assert config.visualization and config.num_attention_heads == 2 and config.hidden_size == 128
    assert g["input_mask"][1].sum() < g["input_mask"].shape[1] and g["image_mask"][1].sum() < g["image_mask"].shape[1]
    oracle = O.OracleUC2ForVLTasks(config, TASK_CFG, ["TASK15"])
    oracle.load_state_dict(seeded_state_dict(oracle.state_dict(), seed=int(g["seed"])), strict=True)
    oracle.eval()
    rec = AR.oracle_maps(oracle, maps_inputs(g))
    T = g["question"].shape[1]
    hs_t, hs_v, maps_t, maps_v = AR.split_maps(rec, T)
    assert len(hs_t) == len(hs_v) == 5 and len(maps_t) == len(maps_v) == 2
    worst = {}

    def check(name, got, ref):
        got = got.numpy()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        worst[name.split("_")[0]] = max(worst.get(name.split("_")[0], 0.0), float(np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-5, err_msg=name)

    check("logits", rec["logits"], g["logits"])
    for i in range(5):
        check("hidden_t_%d" % i, hs_t[i], g["hidden_t_%d" % i])
        check("hidden_v_%d" % i, hs_v[i], g["hidden_v_%d" % i])
    for j, i in enumerate((1, 3)):
        for k in MAP_KEYS:
            check("%s_t_%d" % (k, i), maps_t[j][k], g["%s_t_%d" % (k, i)])
            check("%s_v_%d" % (k, i), maps_v[j][k], g["%s_v_%d" % (k, i)])
    print("helper vs reference fixture, max abs error:", {k: "%.2e" % v for k, v in worst.items()})


def test_emitting_entry_points_and_tap_fields_are_part_of_the_abi():
    names = ("vl_attn2_fwd_probs", "vl_qkv_attention_fwd_probs")
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = _lib.header_symbols()
    for n in names:
        assert hasattr(handle, n), "%s is not exported by the library" % n
        assert n in declared, "%s is not declared in vlhip.h" % n
        assert n in _lib._SIGS, "%s is not bound in _lib.py" % n
    # the new entry points = the old ones + one pointer (float* probs) after lse
    assert len(_lib._SIGS["vl_attn2_fwd_probs"][1]) == len(_lib._SIGS["vl_attn2_fwd"][1]) + 1
    assert len(_lib._SIGS["vl_qkv_attention_fwd_probs"][1]) == len(_lib._SIGS["vl_qkv_attention_fwd"][1]) + 1
    assert len(_lib._SIGS["vl_attn2_fwd"][1]) == 14 and len(_lib._SIGS["vl_qkv_attention_fwd"][1]) == 19  # unchanged
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert re.search(r"encoders\.py:286-311, 343-359", header)
    VL = _lib.header_constants()
    taps = [VL["VL_LY_TAP_PROBS"], VL["VL_LY_TAP_X1"], VL["VL_LY_TAP_OUT"]]
    assert len(set(taps)) == 3 and all(84 <= v <= 95 for v in taps)
    others = {v for k, v in VL.items() if k.startswith("VL_LY_") and not k.startswith("VL_LY_TAP_") and k != "VL_LY_FIELDS"}
    assert not others & set(taps)
    assert max(others) == 83  # (VL_LY_EV_READY: the last field before the taps)
    assert VL["VL_LY_FIELDS"] == 96 and VL["VL_ST_FIELDS"] == 48
    lib = _lib.lib()
    for L in (1, 2, 12):
        assert lib.vl_stack_desc_len(L) == 48 + 96 * L
