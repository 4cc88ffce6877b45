"""Host side of the differentiable hidden-state taps (no GPU): the two tap-gradient fields of the stack descriptor in the
header, the library and the descriptor builder; the model attribute; the two autograd nodes' handling of the hidden states'
gradients (which one a loss touched, how the text / box views' gradients are assembled, the whole gradient of entry 0, the
second-backward error) around a stand-in engine; M3P still refuses per-layer outputs."""
import numpy as np
import pytest
import torch

import diff_taps_ref as R
from helpers import TASK_CFG, golden_config, load_golden, uc2_cfg_dict
from clg_vqa_amd import _lib, engine as E
from clg_vqa_amd.config import BertConfig
from clg_vqa_amd.encoders import BertForVLTasks


def test_descriptor_fields_agree_between_header_library_and_builder():
    VL = _lib.header_constants()
    assert VL is not E.VL and VL == E.VL  # the builder indexes with the header's own numbers
    x1, out, fields = VL["VL_LY_TAP_GRAD_X1"], VL["VL_LY_TAP_GRAD_OUT"], VL["VL_LY_FIELDS"]
    taken = {v + i for k, v in VL.items() if k.startswith("VL_LY_") and k not in ("VL_LY_FIELDS", "VL_LY_TAP_GRAD_X1", "VL_LY_TAP_GRAD_OUT")
             for i in range(16 if k == "VL_LY_GRAD0" else 6 if k == "VL_LY_MASK0" else 1)}
    assert x1 != out and {x1, out}.isdisjoint(taken) and max(x1, out) < fields
    L = _lib.lib()
    for n in (1, 2, 12):
        assert L.vl_stack_desc_len(n) == VL["VL_ST_FIELDS"] + n * fields == E._layer_off(n)
        assert E._layer_off(n - 1) + max(x1, out) < L.vl_stack_desc_len(n)
    # the library reads the fields where the builder writes them: a tap gradient on a layer that runs in the pooled-row
    # mode is refused by name before anything is launched (argument checks only: no device is touched)
    for name in ("VL_LY_TAP_GRAD_X1", "VL_LY_TAP_GRAD_OUT"):
        d = np.zeros(E._layer_off(2), dtype=np.int64)
        d[VL["VL_ST_MAGIC"]] = VL["VL_ST_MAGIC_VALUE"]
        for k, v in (("B", 2), ("S", 12), ("H", 128), ("I", 512), ("NH", 4), ("NLAYERS", 2), ("POOLED_ONLY", 1), ("ROWS0", 64)):
            d[VL["VL_ST_" + k]] = v
        d[E._layer_off(1) + VL[name]] = 64
        rc = L.vl_stack_bwd(d.ctypes.data, 2, 1, None, None)
        msg = L.vl_last_error().decode()
        assert rc != 0 and "VL_LY_TAP_GRAD" in msg and "pooled-row" in msg, (name, rc, msg)


def test_attribute_defaults_to_false():
    assert BertForVLTasks.differentiable_encoded_layers is False
    model = BertForVLTasks(BertConfig.from_dict(uc2_cfg_dict(hidden=128, heads=4, inter=512, n_layers=1, vocab=64)), TASK_CFG,
                           ["TASK15"])
    assert model.differentiable_encoded_layers is False
    model.differentiable_encoded_layers = True
    assert BertForVLTasks.differentiable_encoded_layers is False and "differentiable_encoded_layers" not in model.state_dict()


def test_m3p_still_refuses_per_layer_outputs():
    from clg_vqa_amd.m3p import M3PForVLTasks
    g = load_golden("m3p_small.npz")
    model = M3PForVLTasks(golden_config(g, m3p=True), TASK_CFG, ["TASK15"])
    model.differentiable_encoded_layers = True
    z = torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="output_all_encoded_layers"):
        model(z, torch.zeros(1, 3, 2048), torch.zeros(1, 3, 5), "TASK15", output_all_encoded_layers=True)


class _Arena(object):
    in_flight, ticket = False, None


class _Stack(object):
    def __init__(self, L):
        self.specs, self.seen = [None] * L, []

    def backward(self, ar, pw_layers, dy, p_hid, p_att, seed0, dtaps=None, dx0_out=None):
        self.seen.append((dy.clone(), dtaps))
        dx0_out.fill_(0.5)
        return dx0_out, [[torch.ones(2)] * 16 for _ in self.specs]

    def join(self):
        pass


class _StandInEngine(object):
    """What the two nodes of engine.differentiable_trunk need of an engine: forward fills the tap request like
    UC2Engine.forward; the stack's and the embeddings' halves of backward record what they are handed."""
    H = 8

    def __init__(self, B, S, L):
        self.B, self.S, self.grad_mode, self.stack = B, S, True, _Stack(L)
        self.tap_request = dict(hidden=True, probs=False)
        self.embed_seen = []

    def forward(self, ids, feats, locs, seg, tmask, imask, training, need_grad=True):
        taps, self.tap_request = self.tap_request, None
        mk = lambda k: torch.full((self.B, self.S, self.H), float(k))  # noqa: E731
        L = len(self.stack.specs)
        taps["embed"] = mk(0)
        taps["x1"], taps["out"] = [mk(2 * l + 1) for l in range(L)], [mk(2 * l + 2) for l in range(L)]
        ar = _Arena()
        ar.x32 = torch.zeros(1)
        return mk(-1), dict(arena=ar, B=self.B, S=self.S, T=ids.shape[1], pw=dict(layers=None), p_hid=0.0, p_att=0.0, seed0=0)

    def embed_backward(self, sv, dy, layer_grads, want_feats=False, want_locs=False, dy_v=None):
        self.embed_seen.append((dy.clone(), dy_v.clone()))
        return [torch.ones(3)], None, None


@pytest.fixture
def no_device_stream(monkeypatch):
    class _S(object):
        cuda_stream = 0
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _S())


def _apply(eng, params):
    B, T, V = eng.B, 2, eng.S - 2
    return E.differentiable_trunk(eng, False, torch.zeros(B, T, dtype=torch.int64), torch.zeros(B, V, 4), torch.zeros(B, V, 7), None,
                                  None, None, params)


def test_autograd_nodes_route_the_hidden_state_gradients(no_device_stream):
    B, S, L, T = 2, 5, 2, 2
    w_emb = torch.zeros(3, requires_grad=True)
    w_lay = [torch.zeros(2, requires_grad=True) for _ in range(16 * L)]
    eng = _StandInEngine(B, S, L)
    x, (hs_t0, hs_v0), later = _apply(eng, [w_emb] + w_lay)
    hs = [None] + later
    assert len(later) == 2 * L and x.requires_grad and all(h.requires_grad and h.shape == (B, S, 8) for h in later)
    assert hs_t0.requires_grad and hs_v0.requires_grad and hs_t0.shape == (B, T, 8) and hs_v0.shape == (B, S - T, 8)
    assert [float(h.detach().flatten()[0]) for h in [x, hs_t0, hs_v0] + later] == [-1.0, 0.0, 0.0, 1.0, 2.0, 3.0, 4.0]
    coef, _ = R.coefficients(B, S, 8, 1 + 2 * L, 4, seed=5)
    # the loss reads the text view of hidden state 1, both views of 3 and the text view of 0 -- not the trunk's output
    hs_t0.retain_grad()
    loss = (hs[1][:, :T] * coef[1][:, :T]).sum() + (hs[3][:, :T] * coef[3][:, :T]).sum() + (hs[3][:, T:] * coef[3][:, T:]).sum() \
        + (hs_t0 * coef[0][:, :T]).sum()
    loss.backward(retain_graph=True)
    # the stack's half: no gradient of the output (zeros stand in), None for the untouched hidden states 2 and 4, the
    # assembled [B,S,H] gradients of 1 (box rows zero) and 3
    (dy, (dx1, dout)), = eng.stack.seen
    assert not dy.any() and dy.shape == (B * S, 8)
    assert dout == [None, None] and dx1[0] is not None and dx1[1] is not None
    want1 = coef[1].clone()
    want1[:, T:] = 0
    assert torch.equal(dx1[0], want1) and torch.equal(dx1[1], coef[3])
    # the embeddings' half receives what autograd collected for hidden state 0: the stack's dX0 (0.5), for the text rows +
    # the direct term
    (d_t, d_v), = eng.embed_seen
    assert torch.equal(d_t.view(B, T, 8), 0.5 + coef[0][:, :T]) and torch.equal(d_v, torch.full((B * (S - T), 8), 0.5))
    # ... and so does the retained tensor: the token saliency
    assert torch.equal(hs_t0.grad, 0.5 + coef[0][:, :T])
    assert torch.equal(w_emb.grad, torch.ones(3)) and all(torch.equal(w.grad, torch.ones(2)) for w in w_lay)
    # the activations were released by that backward: a second one raises the engine's own error
    with pytest.raises(RuntimeError, match="retain_graph / double backward are not supported"):
        hs[2].sum().backward()
    # a loss on the top hidden state alone: its gradient IS the stack's dy, no tap gradient is left
    eng = _StandInEngine(B, S, L)
    x, _, later = _apply(eng, [w_emb] + w_lay)
    (later[3] * coef[4]).sum().backward()
    (dy, (dx1, dout)), = eng.stack.seen
    assert torch.equal(dy.view(B, S, 8), coef[4]) and dx1 == [None, None] and dout == [None, None]
    # without grad mode at the call site nothing carries a graph and the taps stay with the request
    eng = _StandInEngine(B, S, L)
    eng.grad_mode = False
    x, hs0, later = _apply(eng, [w_emb] + w_lay)
    assert hs0 is None and later is None and not x.requires_grad
