"""Gradients with respect to the region features and the box locations: the oracles (fp64) against the fixture produced by
the real reference (tests/golden/make_golden_input_grads.py), and the ABI entry point of the new product.  CPU only."""
import numpy as np
import pytest

import input_grads_ref as R
from helpers import TASK_CFG
from clg_vqa_amd import _lib
from clg_vqa_amd.synthetic import seeded_state_dict


def _oracle(tag, g):
    if tag == "m3p":
        from oracle import m3p_oracle as M
        model = M.OracleM3PForVLTasks(R.case_config(g, True), TASK_CFG, ["TASK15"])
    else:
        from oracle import uc2_oracle as O
        model = O.OracleUC2ForVLTasks(R.case_config(g, False), TASK_CFG, ["TASK15"])
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=int(g["seed"])), strict=True)
    return model.eval()


@pytest.mark.parametrize("tag", ["uc2", "m3p"])
def test_oracle_input_gradients_match_reference_fixture(tag):
    """features.grad / spatials.grad of the oracle (UC2 in fp64; M3P in fp32, see input_grads_ref.oracle_input_grads) = the
    reference's own autograd (fp32 eager), to the tolerances tests/test_oracle_golden.py uses for the parameter gradients
    of its fixtures."""
    g = R.load_case(tag)
    loss, logits, dfeats, dlocs = R.oracle_input_grads(_oracle(tag, g), R.case_batch(g), double=tag != "m3p")
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=1e-4, atol=2e-5)
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    for name, got in (("features_grad", dfeats), ("spatials_grad", dlocs)):
        ref = g[name]
        assert got.shape == ref.shape == g[name[:-5]].shape
        norm = float(np.linalg.norm(ref.astype(np.float64)))
        assert norm > 0
        scale = max(norm, 1e-3)
        np.testing.assert_allclose(got.numpy(), ref, rtol=2e-4, atol=2e-5 * scale, err_msg=name)
        assert abs(float(got.norm()) - norm) <= 1e-4 * scale, name
    pad = g["image_mask"] == 0
    assert pad[1].any() and not pad[0].any()
    if tag == "m3p":
        # M3P masks the [image ; text] stream by length (len_img + len_txt = 6 < V in sample 1): boxes 6 and 7 are multiplied
        # by zero and receive no gradient; the padded boxes 2..5 lie inside the length and keep theirs
        assert int(g["image_mask"][1].sum() + g["input_mask"][1].sum()) == 6
        for name in ("features_grad", "spatials_grad"):
            assert not g[name][1, 6:].any() and g[name][1, 2:6].any(axis=-1).all(), name
    else:  # UC2: padded boxes are masked as keys (the -10000 underflows in the soft-max): nothing reaches the loss from them
        assert not g["features_grad"][pad].any() and g["features_grad"][~pad].any(axis=-1).all()


def test_abi_table_has_the_location_input_gradient():
    assert "vl_loc_linear_bwd_input" in _lib.header_symbols()
    res, args = _lib._SIGS["vl_loc_linear_bwd_input"]
    assert res is _lib.c_int and len(args) == 7
    assert hasattr(_lib.lib(), "vl_loc_linear_bwd_input")
