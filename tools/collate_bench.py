"""Record -> device batch, host time per batch of the two input paths and device time of the collate kernels:
`python tools/collate_bench.py [--steps 20] [--rounds 3]` on the MI355X.

  (a) records.collate_records (host, one Python thread + torch's intra-op threads) -> data.DevicePrefetcher
  (b) data.RecordPrefetcher: records.pack_records -> one copy -> csrc/collate.hip on the copy stream

at the c2 shape (B 256, T 20, V 36, 7 locs) and the c4 shape (B 256, V 100, 5 locs, norm_embeddings), 16 threads.  The
consumer does nothing, so a figure is what the input side alone sustains: wall time of `steps` batches, ending in a device
synchronise, over `steps`.  The two paths alternate, `rounds` times each, after a warm-up round; the median and the range are
printed.  The kernels are timed with device events on a resident blob (warm: the blob fits the 256 MB L3 at c2)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clg_vqa_amd import ops, records  # noqa: E402
from clg_vqa_amd.data import DevicePrefetcher, RecordPrefetcher  # noqa: E402
from clg_vqa_amd.synthetic import make_records  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--distinct", type=int, default=4, help="distinct record batches per shape (cycled)")
args = ap.parse_args()

assert torch.cuda.is_available(), "collate_bench needs the MI355X"
torch.set_num_threads(16)
dev = torch.device("cuda", 0)
C, T, B = 1842, 20, args.batch
prior = np.random.RandomState(7).uniform(0.05, 1.0, size=(C, C))
np.fill_diagonal(prior, 0.0)
prior32 = records.prior_table_device(prior, dev)


def cycle(batches, n):
    for i in range(n):
        yield batches[i % len(batches)]


def run_a(batches, n, kw):
    def host_batches():
        for i, recs in enumerate(cycle(batches, n)):
            yield records.collate_records(recs, T, kw["region_len"], kw["num_locs"], C, norm_embeddings=kw["norm_embeddings"],
                                          prior=prior, batch_index=i)
    t0 = time.perf_counter()
    k = sum(1 for _ in DevicePrefetcher(host_batches(), dev, depth=2))
    torch.cuda.synchronize()
    assert k == n
    return (time.perf_counter() - t0) * 1e3 / n


def run_b(batches, n, kw):
    t0 = time.perf_counter()
    k = sum(1 for _ in RecordPrefetcher(cycle(batches, n), dev, depth=2, seq_len=T, num_labels=C, prior32=prior32, **kw))
    torch.cuda.synchronize()
    assert k == n
    return (time.perf_counter() - t0) * 1e3 / n


def kernel_times(recs, kw, reps=30):
    V, L, norm = kw["region_len"], kw["num_locs"], kw["norm_embeddings"]
    blob, meta = records.pack_records(recs, T, V, L, C)
    v = records.packed_views((blob[:meta["nbytes"]].to(dev), meta))
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    feats, loc, imask = torch.empty((B, V, 2048), **f32), torch.empty((B, V, L), **f32), torch.empty((B, V), **i64)
    ids, tmask, seg = (torch.empty((B, T), **i64) for _ in range(3))
    target, dist = torch.empty((B, C), **f32), torch.empty((B, C), **f32)
    calls = (("vl_collate_regions", lambda: ops.collate_regions(v["feats"], v["boxes"], v["row_off"], v["whp"], feats, loc,
                                                                imask, norm),
              4 * 2048 * (meta["n_rows"] + B * V)),
             ("vl_collate_text", lambda: ops.collate_text(v["tok"], v["tok_off"], ids, tmask, seg, 1), 8 * (3 * B * T)),
             ("vl_collate_targets", lambda: ops.collate_targets(v["labels"], v["scores"], prior32, target, dist),
              4 * 3 * B * C))
    out = {}
    for name, fn, nbytes in calls:
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = sorted(ts[5:])
        out[name] = ts[len(ts) // 2]
        print("  %-20s median %8.1f us  min %8.1f us  (%.0f GB/s of the bytes it must move)"
              % (name, out[name], ts[0], nbytes / out[name] / 1e3))
    return out, meta["nbytes"]


SHAPES = (("c2", dict(region_len=36, num_locs=7, norm_embeddings=False)),
          ("c4", dict(region_len=100, num_locs=5, norm_embeddings=True)))
for tag, kw in SHAPES:
    V = kw["region_len"]
    # mostly full box lists (the extractors emit a fixed number of boxes); ragged questions
    batches = [make_records(B, seq_len=T, num_boxes=V, num_labels=C, seed=500 + i, box_counts=(V, V, V, V - 4))
               for i in range(args.distinct)]
    print("%s: B %d  T %d  V %d  locs %d  norm_embeddings %s  (%d steps x %d rounds, %d torch threads)"
          % (tag, B, T, V, kw["num_locs"], kw["norm_embeddings"], args.steps, args.rounds, torch.get_num_threads()))
    run_a(batches, 4, kw)
    run_b(batches, 4, kw)  # warm-up: pinned buffers, code objects
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(run_a(batches, args.steps, kw))
        tb.append(run_b(batches, args.steps, kw))
    for name, ts in (("(a) collate_records -> DevicePrefetcher", ta), ("(b) RecordPrefetcher", tb)):
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        print("  %-42s %8.2f ms / batch  (range %.2f .. %.2f)  %7.1f batches/s  %9.0f samples/s"
              % (name, med, ts[0], ts[-1], 1e3 / med, 1e3 / med * B))
    print("  host time per batch, (a) / (b): %.2f" % (sorted(ta)[len(ta) // 2] / sorted(tb)[len(tb) // 2]))
    _, nbytes = kernel_times(batches[0], kw)
    print("  packed blob: %.1f MB per batch" % (nbytes / 1e6))
