"""Losses on the per-layer hidden states, and their gradients from the UNMODIFIED UC2 oracle in float64 (test infrastructure
shared by tests/test_gpu_diff_taps.py and tests/test_diff_taps_host.py).

The oracle's forward is plain torch: forward hooks on ``bert.embeddings`` and ``bert.encoder.layer[i]`` hand out its hidden
states WITH their graph (tests/attention_maps_ref.py records the same tensors detached), so autograd differentiates a loss on
them like any other.  Hidden state k of 1 + 2 L: 0 = embedding output, 2 l + 1 / 2 l + 2 = attention / feed-forward sub-layer
output of layer l, [B, S, H] with the T text rows first.
"""
import copy

import torch


def coefficients(B, S, H, n_hidden, n_labels, seed):
    """Fixed random coefficients of the loss: E [n_hidden, B, S, H] (C_k = E[k][:, :T], D_k = E[k][:, T:]) and c [B, n_labels]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_hidden, B, S, H, generator=g), torch.randn(B, n_labels, generator=g)


def tap_loss(logits, hs_t, hs_v, E, c, T, taps=None):
    """sum_k <C_k, hs_t[k]> + <D_k, hs_v[k]> over the hidden states `taps` (None = all) + <c, logits>."""
    loss = (logits * c.to(logits)).sum()
    for k in (range(len(hs_t)) if taps is None else taps):
        e = E[k].to(logits)
        loss = loss + (hs_t[k] * e[:, :T]).sum() + (hs_v[k] * e[:, T:]).sum()
    return loss


def oracle_tap_grads(oracle, inputs, E, c, taps=None):
    """inputs = (question, features, spatials, segment_ids, input_mask, image_mask), CPU tensors.  Runs a float64 copy of
    `oracle` (its mode and dropout-mask provider kept), builds tap_loss on its hooked hidden states and differentiates.
    Returns dict(loss, logits, params {name: grad, zeros where autograd left None}, features, spatials, hidden0 = the
    gradient of the embedding output [B, S, H])."""
    q, feats, spat, seg, tmask, imask = inputs
    training, provider = oracle.training, getattr(oracle, "mask_provider", None)
    o64 = copy.deepcopy(oracle).double()
    o64.train(training)
    for m in o64.modules():
        m.mask_provider = provider
    feats, spat = feats.double().clone().requires_grad_(True), spat.double().clone().requires_grad_(True)
    hidden, hooks = [], []

    def emb_hook(mod, args, out):
        x = torch.cat(out, dim=1)
        x.retain_grad()
        hidden.append(x)
        T = out[0].shape[1]
        return x[:, :T], x[:, T:]  # (the oracle's stream is rebuilt from these: x is the node every later use goes through)

    hooks.append(o64.bert.embeddings.register_forward_hook(emb_hook))
    for layer in o64.bert.encoder.layer:
        hooks.append(layer.register_forward_hook(lambda mod, args, out: hidden.append(out)))
    try:
        logits = o64(q, feats, spat, "TASK15", seg, tmask, imask)[0]
    finally:
        for h in hooks:
            h.remove()
    T = q.shape[1]
    loss = tap_loss(logits, [h[:, :T] for h in hidden], [h[:, T:] for h in hidden], E.double(), c.double(), T, taps)
    o64.zero_grad()
    loss.backward()
    params = {n: (torch.zeros_like(p) if p.grad is None else p.grad) for n, p in o64.named_parameters()}
    return dict(loss=loss.detach(), logits=logits.detach(), params=params, features=feats.grad, spatials=spat.grad,
                hidden0=hidden[0].grad, hidden=[h.detach() for h in hidden])
