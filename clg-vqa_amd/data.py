"""Host -> HBM staging of the reference's batch tuple.

The reference moves every batch with a blocking ``t.cuda(device=device, non_blocking=True)`` on pageable memory inside
the step (``volta/task_utils.py:309``: features ``[B,V,2048]`` fp32 = 75.5 MB at bs 256).  At > 10 k samples/s that
copy (~1.3 ms over PCIe when it overlaps nothing) has to leave the step: ``DevicePrefetcher`` wraps any iterable of
batch tuples (the reference's loaders yield 10-tuples of CPU tensors, ``gqa_dataset_semantic_code_mix.py:440-452``),
stages each tuple through pinned buffers on its own HIP stream ``depth`` batches ahead, and hands out device tuples
whose copies the consumer stream has been made to wait for.  ``ForwardModelsTrain/Val`` accept the device tuples
unchanged (their ``.to(device)`` is then a no-op).
"""
import collections

import torch


class DevicePrefetcher(object):
    def __init__(self, iterable, device, depth=2):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("clg_vqa_amd.DevicePrefetcher: the target must be the MI355X (no CPU path)")
        self.it = iter(iterable)
        self.depth = depth
        self.stream = torch.cuda.Stream(device=self.device)
        self.queue = collections.deque()
        self._pinned = {}  # (slot, position) -> pinned staging buffer, reused while shapes stay the same
        self._slot_done = {}  # slot -> event of the last copy that read its staging buffers
        self._slot = 0

    def _stage(self, slot, pos, t):
        if not torch.is_tensor(t) or t.is_cuda:
            return t
        if t.is_pinned():
            return t
        key = (slot, pos)
        buf = self._pinned.get(key)
        if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
            buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            self._pinned[key] = buf
        buf.copy_(t)
        return buf

    def _enqueue(self):
        try:
            batch = next(self.it)
        except StopIteration:
            return False
        slot = self._slot
        self._slot = (self._slot + 1) % (self.depth + 1)
        prev = self._slot_done.get(slot)
        if prev is not None:
            prev.synchronize()  # the host may run several steps ahead of the GPU: never rewrite a buffer a DMA still reads
        staged = [self._stage(slot, i, t) for i, t in enumerate(batch)]
        with torch.cuda.stream(self.stream):
            dev = tuple(t.to(self.device, non_blocking=True) if torch.is_tensor(t) else t for t in staged)
            done = torch.cuda.Event()
            done.record(self.stream)
        self._slot_done[slot] = done
        self.queue.append((dev, done))
        return True

    def __iter__(self):
        return self

    def __next__(self):
        while len(self.queue) < self.depth and self._enqueue():
            pass
        if not self.queue:
            raise StopIteration
        dev, done = self.queue.popleft()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(done)
        for t in dev:  # the consumer stream uses memory that the copy stream allocated
            if torch.is_tensor(t):
                t.record_stream(cur)
        self._enqueue()  # keep `depth` copies in flight while the consumer computes
        return dev


class RecordPrefetcher(object):
    """``DevicePrefetcher``'s contract for batches that are still LISTS OF RECORDS: the record -> batch work runs on the
    device (``records.pack_records`` -> one copy -> ``records.collate_on_device``, csrc/collate.hip) instead of on the host.

    Iterates over ``record_batches`` (each a list of the record dicts of ``records.collate_records``).  Per batch the host
    writes the records once, ragged, into a pinned blob that is reused per prefetch slot, ONE ``non_blocking`` copy takes it
    to HBM on this object's own stream, and the three collate kernels run on that same stream; the consumer stream is made
    to wait for the event behind them.  A blob is never rewritten while a DMA may still read it.  ``collate_kwargs``:
    ``seq_len, region_len, num_locs, num_labels`` and optionally ``padding_index, norm_embeddings, feat_dim`` as in
    ``collate_records``, plus ``prior`` (the dense table of ``records.prior_table``, moved to the device once) or
    ``prior32`` (``records.prior_table_device``).  ``pack_threads``: host threads of the record -> blob copy.
    ``ForwardModelsTrain/Val`` accept the tuples unchanged."""

    def __init__(self, record_batches, device, depth=2, pack_threads=8, **collate_kwargs):
        from . import records
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("clg_vqa_amd.RecordPrefetcher: the target must be the MI355X (no CPU path)")
        kw = dict(collate_kwargs)
        try:
            self.shape = tuple(kw.pop(k) for k in ("seq_len", "region_len", "num_locs", "num_labels"))
        except KeyError as e:
            raise TypeError("RecordPrefetcher: missing collate argument %s" % e) from None
        self.feat_dim = kw.pop("feat_dim", 2048)
        self.padding_index = kw.pop("padding_index", 1)
        self.norm_embeddings = kw.pop("norm_embeddings", False)
        prior, self.prior32 = kw.pop("prior", None), kw.pop("prior32", None)
        if kw:
            raise TypeError("RecordPrefetcher: unknown collate arguments %s" % sorted(kw))
        if prior is not None and self.prior32 is None:
            self.prior32 = records.prior_table_device(prior, self.device)
        self.it = iter(record_batches)
        self.depth = depth
        self.pack_threads = pack_threads
        self.stream = torch.cuda.Stream(device=self.device)
        self.queue = collections.deque()
        self._blob = {}  # slot -> pinned blob, reused (and grown) batch after batch
        self._slot_done = {}  # slot -> event behind the copy and the kernels that read the slot's blob
        self._slot = 0
        self._index = 0

    def _enqueue(self):
        from . import ops, records
        try:
            recs = next(self.it)
        except StopIteration:
            return False
        slot = self._slot
        self._slot = (self._slot + 1) % (self.depth + 1)
        prev = self._slot_done.get(slot)
        if prev is not None:
            prev.synchronize()  # the host may run several steps ahead of the GPU: never rewrite a blob a DMA still reads
        blob, meta = records.pack_records(recs, *self.shape, feat_dim=self.feat_dim, batch_index=self._index,
                                          out=self._blob.get(slot), threads=self.pack_threads)
        self._blob[slot] = blob
        self._index += 1
        with torch.cuda.stream(self.stream):
            blob_dev = blob[:meta["nbytes"]].to(self.device, non_blocking=True)
            with ops.launching(self.stream.cuda_stream):
                dev = records.collate_on_device((blob_dev, meta), *self.shape, padding_index=self.padding_index,
                                                norm_embeddings=self.norm_embeddings, prior32=self.prior32)
            done = torch.cuda.Event()
            done.record(self.stream)
        self._slot_done[slot] = done
        self.queue.append((dev, done))
        return True

    def __iter__(self):
        return self

    def __next__(self):
        while len(self.queue) < self.depth and self._enqueue():
            pass
        if not self.queue:
            raise StopIteration
        dev, done = self.queue.popleft()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(done)
        for t in dev:  # the consumer stream uses memory that the copy stream allocated (qid is a view of the device blob)
            t.record_stream(cur)
        self._enqueue()  # keep `depth` batches in flight while the consumer computes
        return dev
