"""Per-layer hidden states and attention data from the UNMODIFIED oracle (test infrastructure).

Forward hooks on ``bert.embeddings`` and ``bert.encoder.layer[i]`` record the hidden states; the attention data of an
attention sub-layer is re-evaluated from the hooked sub-layer input and its ``query`` / ``key`` Linear modules:
P = softmax(Q K^T / sqrt(dh) + mask), times a keep-scale when the caller supplies one (``train()``: the masks of
tests/dropout_masks.py).  In the reference's layout (encoders.py:343-355, 863-885): hidden states [B, S, H] with text rows
first, P [B, nh, S, S], queries / keys [B, nh, S, dh].  ``double=True`` runs a float64 copy of the oracle.
"""
import copy
import math

import torch

import dropout_masks as DM


def oracle_maps(oracle, inputs, double=False, attn_keep=None):
    """inputs = (question, features, spatials, segment_ids, input_mask, image_mask), CPU tensors.  attn_keep: None or
    callable(layer, B, nh, S) -> [B, nh, S, S] keep-scale array.  Returns dict(logits, hidden [1 + 2 L], probs / queries /
    keys [L])."""
    q, feats, spat, seg, tmask, imask = inputs
    if double:
        training, provider = oracle.training, getattr(oracle, "mask_provider", None)
        oracle = copy.deepcopy(oracle).double()
        oracle.train(training)
        for m in oracle.modules():
            m.mask_provider = provider
        feats, spat = feats.double(), spat.double()
    rec = dict(hidden=[], probs=[], queries=[], keys=[])
    hooks = []

    def emb_hook(mod, args, out):
        rec["hidden"].append(torch.cat(out, dim=1).detach())

    def layer_hook(i):
        def hook(mod, args, out):
            rec["hidden"].append(out.detach())
            if i % 2 == 0:
                x, add_mask = args
                B, S, H = x.shape
                nh = mod.nh
                dh = H // nh
                a = mod.attention_self
                with torch.no_grad():
                    qq = a.query(x).view(B, S, nh, dh).permute(0, 2, 1, 3)
                    kk = a.key(x).view(B, S, nh, dh).permute(0, 2, 1, 3)
                    P = torch.softmax(torch.matmul(qq, kk.transpose(-1, -2)) / math.sqrt(dh) + add_mask, dim=-1)
                    if attn_keep is not None:
                        P = P * torch.as_tensor(attn_keep(i // 2, B, nh, S)).to(P.dtype)
                rec["probs"].append(P)
                rec["queries"].append(qq)
                rec["keys"].append(kk)
        return hook

    hooks.append(oracle.bert.embeddings.register_forward_hook(emb_hook))
    for i, layer in enumerate(oracle.bert.encoder.layer):
        hooks.append(layer.register_forward_hook(layer_hook(i)))
    try:
        with torch.no_grad():
            rec["logits"] = oracle(q, feats, spat, "TASK15", seg, tmask, imask)[0].detach()
    finally:
        for h in hooks:
            h.remove()
    return rec


def engine_attn_keep(base_seed, call, p_att):
    """attn_keep of the engine's `call`-th forward (EngineBase.next_seed; attention site of layer l = 16 l + 3)."""
    seed0 = DM.seed0_of(base_seed, call)

    def keep(layer, B, nh, S):
        return DM.attn_mask(DM.site_seed(seed0, DM.stack_sites(layer)[0]), B, nh, S, p_att)
    return keep


def split_maps(rec, T):
    """The reference's return layout from the single-stream record: (hidden_t, hidden_v, maps_t, maps_v), the map lists
    holding one dict per ATTENTION sub-layer."""
    hs_t = [h[:, :T] for h in rec["hidden"]]
    hs_v = [h[:, T:] for h in rec["hidden"]]
    maps_t, maps_v = [], []
    for P, q, k in zip(rec["probs"], rec["queries"], rec["keys"]):
        maps_t.append(dict(intra_attn=P[:, :, :T, :T], inter_attn=P[:, :, :T, T:], queries=q[:, :, :T], keys=k[:, :, :T]))
        maps_v.append(dict(intra_attn=P[:, :, T:, T:], inter_attn=P[:, :, T:, :T], queries=q[:, :, T:], keys=k[:, :, T:]))
    return hs_t, hs_v, maps_t, maps_v
