"""Input gradients (region features, box locations) from the UNMODIFIED oracles in float64, and the fixture produced by the
real reference (tests/golden/make_golden_input_grads.py).  Test infrastructure shared by the CPU and the GPU tests."""
import copy

import torch

from helpers import golden_batch, golden_config, load_golden
from oracle import uc2_oracle as O

FIXTURE = "uc2_input_grads.npz"


def load_case(tag):
    """One case of the fixture ("uc2" / "m3p") as the dict a model fixture is: config, seed, batch fields, results."""
    g = load_golden(FIXTURE)
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + "_")}


def case_config(g, m3p):
    return golden_config(g, m3p=m3p)


def case_batch(g):
    return golden_batch(g)


def oracle_input_grads(oracle, batch, double=True):
    """(loss, logits, d loss / d features, d loss / d spatials) of a float64 copy of `oracle` (its mode and dropout-mask
    provider kept), CPU tensors.  double=False keeps float32: the M3P oracle casts its attention scores to float32 like the
    reference (m3p_transformer.py:201), so it cannot run in float64 as it stands."""
    training, provider = oracle.training, getattr(oracle, "mask_provider", None)
    dt = torch.float64 if double else torch.float32
    for m in oracle.modules():
        # torch.nn.utils.prune leaves `weight = weight_orig * weight_mask` behind as a plain non-leaf attribute, which
        # deepcopy refuses; the pruning pre-hook recomputes it on every forward, so a detached one copies just as well
        if "weight_orig" in m._parameters and "weight" in m.__dict__:
            m.__dict__["weight"] = m.__dict__["weight"].detach()
    o64 = copy.deepcopy(oracle).to(dt)
    o64.train(training)
    if provider is not None:
        for m in o64.modules():
            m.mask_provider = provider
    batch = list(batch)
    for i in (0, 1, 4, 9):  # features, spatials, target, distances
        batch[i] = batch[i].to(dt)
    feats, spat = batch[0].clone().requires_grad_(True), batch[1].clone().requires_grad_(True)
    batch[0], batch[1] = feats, spat
    loss, _, logits = O.forward_train(o64, tuple(batch))
    loss.backward()
    return loss.detach(), logits.detach(), feats.grad, spat.grad


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    return (got - ref).norm().item() / max(ref.norm().item(), 1e-30)
