"""CPU checks of the dropout-mask restatement (tests/dropout_masks.py) and of the oracles' mask hook: the GPU tests in
test_gpu_dropout.py hand the oracle the engine's masks through that hook, so it must reach every dropout of the oracle,
and the vectorised restatement must agree with a plain scalar one."""
import numpy as np
import pytest
import torch

import dropout_masks as DM
from helpers import TASK_CFG, golden_config, load_golden, uc2_cfg_dict
from oracle import m3p_oracle as M
from oracle import uc2_oracle as O
from clg_vqa_amd.config import BertConfig
from clg_vqa_amd.synthetic import make_batch


def _ones(calls):
    def provider(site, layer, shape):
        calls.append((site, layer))
        return torch.ones(shape)
    return provider


def _step(oracle, batch):
    oracle.zero_grad()
    loss, _, logits = O.forward_train(oracle, batch)
    loss.backward()
    return logits.detach().clone(), {n: p.grad.clone() for n, p in oracle.named_parameters() if p.grad is not None}


def _uc2():
    torch.manual_seed(3)
    config = BertConfig.from_dict(uc2_cfg_dict(hidden=128, heads=4, inter=512, n_layers=2, vocab=300))
    return O.OracleUC2ForVLTasks(config, TASK_CFG, ["TASK15"]), make_batch(3, seq_len=7, num_boxes=9, vocab_size=300, seed=4)


def _m3p():
    torch.manual_seed(3)
    config = golden_config(load_golden("m3p_small.npz"), m3p=True)
    oracle = M.OracleM3PForVLTasks(config, TASK_CFG, ["TASK15"])
    batch = make_batch(3, seq_len=7, num_boxes=9, vocab_size=config.n_words, num_locs=5, l2_normalize=True, seed=4)
    return oracle, batch, config.n_layers


@pytest.mark.parametrize("kind", ["uc2", "m3p"])
def test_all_ones_mask_provider_in_train_mode_equals_eval(kind):
    """With a provider that keeps everything, train() must equal eval() (logits bit for bit): every dropout of the
    oracle goes through the hook (one that did not would draw a torch mask and change the result).  Without a provider
    train() must differ (dropout really is on in these configs)."""
    if kind == "uc2":
        oracle, batch = _uc2()
        n_layers = 2
        emb = [("emb_text", 0), ("emb_box", 0)]
    else:
        oracle, batch, n_layers = _m3p()
        emb = [("emb_image", 0), ("emb_joint", 0)]
    oracle.eval()
    ref_logits, ref_grads = _step(oracle, batch)
    calls = []
    O.set_mask_provider(oracle, _ones(calls))
    oracle.train()
    logits, grads = _step(oracle, batch)
    assert torch.equal(logits, ref_logits)
    assert set(grads) == set(ref_grads)
    for n, g in grads.items():
        # (bit-equal, except that `* 1` hands the embedding LayerNorms a contiguous copy of a torch.cat slice of the
        # gradient: their bias reductions then add the same rows in another order -- measured 1e-7 relative)
        rel = (g.double() - ref_grads[n].double()).norm().item() / max(ref_grads[n].double().norm().item(), 1e-30)
        assert torch.equal(g, ref_grads[n]) or (n.endswith("LayerNorm.bias") and rel <= 1e-6), (n, rel)
    expect = emb + [(s, l) for l in range(n_layers) for s in ("attn_probs", "attn_out", "ffn_out")] + [("pooled", 0)]
    assert sorted(calls) == sorted(expect)
    O.set_mask_provider(oracle, None)
    torch.manual_seed(0)
    logits2, _ = _step(oracle, batch)
    assert not torch.equal(logits2, ref_logits)


def test_vectorised_restatement_equals_scalar_restatement():
    rng = np.random.default_rng(7)
    for seed in (0, 12345 * 4096 + 3, (0x7FFFFFFFFFFF * 4096 + 4090) & DM.MASK64, 0xFFFFFFFFFFFFFFFF):
        for p in (0.1, 0.25, 0.5):
            ctr = np.concatenate([np.arange(1000), rng.integers(0, 1 << 40, 1000)]).astype(np.int64)
            v4 = DM.scale4(seed, ctr, p)
            v1 = DM.scale1(seed, ctr, p)
            for i in range(0, len(ctr), 3):
                e = int(ctr[i])
                assert float(v4[i]) == DM.scalar_scale4(seed, e, p)
                assert float(v1[i]) == DM.scalar_scale1(seed, e, p)
            for kind, v in (("4", v4), ("1", v1)):
                assert abs((v == 0).mean() - p) < 0.04, (kind, seed, p)
    B, nh = 2, 3
    for S in (16, 56, 70, 120, 140, 160):
        for seed, p in ((5, 0.1), (2 ** 63 + 11, 0.25)):
            m = DM.attn_mask(seed, B, nh, S, p)
            idx = rng.integers(0, [B, nh, S, S], size=(300, 4))
            for b, h, q, k in idx:
                assert float(m[b, h, q, k]) == DM.scalar_attn(seed, B, nh, S, p, int(b), int(h), int(q), int(k))
            assert abs((m == 0).mean() - p) < 0.03


def test_restated_masks_keep_their_structure():
    """The counters of the LayerNorm sites: p_post is the p_pre mask of seed ^ POST_SALT; the compact rows of the pooled
    last layer (orig_row_stride S) are rows b * S of the dense mask; keep-scale values are 0 or float32(1 / (1 - p))."""
    B, S, H, p, seed = 3, 20, 128, 0.1, 99 * 4096 + 4
    dense = DM.ln_pre_mask(seed, B * S, H, p)
    assert np.array_equal(DM.ln_pre_mask(seed, B, H, p, orig_row_stride=S), dense.reshape(B, S, H)[:, 0])
    assert np.array_equal(DM.ln_post_mask(seed, B * S, H, p), DM.ln_pre_mask(seed ^ DM.POST_SALT, B * S, H, p))
    assert set(np.unique(dense).tolist()) == {0.0, float(np.float32(1) / np.float32(0.9))}
    assert not np.array_equal(DM.ln_post_mask(seed, B * S, H, p), dense)
    # seed schedule: next_seed / last_seed of engine.py
    s0 = DM.seed0_of(0x5EED ^ 42, 3)
    assert s0 == ((0x5EED ^ 42) * 0x9E3779B1 + 3 * 0x10001) & 0x7FFFFFFFFFFF
    assert DM.site_seed(s0, DM.stack_sites(2)[2]) == s0 * 4096 + 16 * 2 + 5
