#!/usr/bin/env python3
"""Golden per-layer outputs from the REAL reference: ``BertForVLTasks(..., output_all_encoded_layers=True,
output_all_attention_masks=True)`` with ``config.visualization`` set (volta/volta/encoders.py:1202-1259, :848-892, :343-359).

Run in the build container only (the reference does not travel), with the stubs and the weight / input recipe of
make_golden.py:

    python tests/golden/make_golden_maps.py

Writes uc2_maps.npz (data only): a UC2 config with hidden 128, 2 heads (head dim 64), intermediate 512, 2 layers,
visualization=True, all dropout probabilities 0; B = 2, T = 12 (sample 1 has 3 padded tokens), V = 20 (sample 1 has 5 padded
boxes); the inputs, the logits, the 5 + 5 hidden states (embedding output, then every sub-layer's output) and
intra_attn / inter_attn / queries / keys of both attention sub-layers for text and vision, from the model in eval().
Weights are not stored: ``seeded_state_dict(seed=SEED)``.  The archive is written with fixed member timestamps, so a second
run reproduces the file bit for bit.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

SEED, VOCAB, B, T, V = 5, 1000, 2, 12, 20
PAD_T, PAD_V = 3, 5  # padded tokens / boxes of sample 1


def make_inputs():
    from clg_vqa_amd.synthetic import PAD_ID, make_batch
    feats, spat, imask, q, _, tmask, seg, _, _, _ = make_batch(B, seq_len=T, num_boxes=V, vocab_size=VOCAB, seed=100 + SEED,
                                                               fp16_exact=True, full_length=True)
    q[1, T - PAD_T - 1] = 2  # </s>, then pad
    q[1, T - PAD_T:] = PAD_ID
    tmask = (q != PAD_ID).long()
    imask[1, V - PAD_V:] = 0
    return feats, spat, imask, q, tmask, seg


def save_npz_deterministic(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    BertConfig, BertForVLTasks, _ = MG.import_reference()
    from clg_vqa_amd.synthetic import seeded_state_dict
    cfg = MG.uc2_cfg_dict(128, 2, 512, 2, VOCAB)
    cfg.update(visualization=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
               v_attention_probs_dropout_prob=0.0)
    config = BertConfig.from_dict(cfg)
    torch.manual_seed(0)
    model = BertForVLTasks(config, MG.TASK_CFG, ["TASK15"])
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=SEED), strict=True)
    model.eval()
    feats, spat, imask, q, tmask, seg = make_inputs()
    with torch.no_grad():
        out = model(q, feats, spat, "TASK15", seg, tmask, imask, output_all_encoded_layers=True,
                    output_all_attention_masks=True)
    logits, _, _, (maps_t, maps_v), hs_t, hs_v = out
    assert len(hs_t) == len(hs_v) == 5 and len(maps_t) == len(maps_v) == 5
    arrays = dict(
        cfg_json=np.frombuffer(json.dumps(cfg, sort_keys=True).encode(), dtype=np.uint8),
        seed=np.int64(SEED), vocab=np.int64(VOCAB),
        features=feats.numpy().astype(np.float16), spatials=spat.numpy().astype(np.float16),
        image_mask=imask.numpy().astype(np.int8), question=q.numpy().astype(np.int32),
        input_mask=tmask.numpy().astype(np.int8), logits=logits.numpy())
    for i in range(5):
        arrays["hidden_t_%d" % i] = hs_t[i].numpy()
        arrays["hidden_v_%d" % i] = hs_v[i].numpy()
        for tag, m in (("t", maps_t[i]), ("v", maps_v[i])):
            if i in (1, 3):
                for k in ("intra_attn", "inter_attn", "queries", "keys"):
                    arrays["%s_%s_%d" % (k, tag, i)] = m[k].contiguous().numpy()
            else:
                assert m is None, (i, tag)
    path = os.path.join(HERE, "uc2_maps.npz")
    save_npz_deterministic(path, arrays)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
