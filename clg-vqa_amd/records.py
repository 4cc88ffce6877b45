"""Record -> batch on the host: the input side of the hot path.

Restates, vectorised over the whole batch, what the reference does per sample in Python:

* ``BertPreprocessBatch.__call__`` (volta/volta/datasets/gqa_dataset_semantic_code_mix.py:564-651): box-location
  features from pixel boxes -- area first, on the RAW coordinates ``(y2-y1)(x2-x1)/(w h)`` (:586-591), then
  ``x/w, y/h`` (:594-597), then for ``num_locs > 5`` width and height of the NORMALISED box in columns 4, 5 (:599-601)
  => UC2 7-d ``[x1,y1,x2,y2,w,h,area]``, M3P 5-d ``[x1,y1,x2,y2,area]``; with ``norm_embeddings`` (M3P) the feature
  rows are L2-normalised with ``F.normalize`` (eps 1e-12) and the location rows divided by their plain L2 norm (:603-606:
  an all-zero padded row becomes NaN there, Appendix B quirk 4 -- reproduced, the 100-box extractor never pads);
  token truncation ``[t0] + t[1:-1][:seq_len-2] + [t-1]`` and padding with ``padding_index`` (:622-623, :691-700).
* ``GQAClassificationLoader.__iter__`` (:386-452): ``target.scatter_(1, labels, scores)``, the 10-tuple.
* ``get_embeddingdist`` (:371-381): the ``[B, num_labels]`` prior-distance rows, a 1842-iteration Python loop per
  sample over a ``(j, t)``-keyed dict in the reference; here ONE row gather from a dense ``[C, C]`` table built once
  (``prior_table``).

The tokenizer (question string -> ids) and the LMDB / tensorpack reader stay outside: a record carries ``tokens``.
Batches come out as CPU tensors in the reference's 10-tuple layout, ready for ``clg_vqa_amd.data.DevicePrefetcher``.
"""
import numpy as np
import torch


def prior_table(semantic_dict, num_labels):
    """Dense table T with T[t, j] = semantic_dict[(j, t)] for j != t and 0 on the diagonal, so that the reference's
    ``get_embeddingdist(labels)[i] == T[labels[i][-1]]`` (gqa_dataset_semantic_code_mix.py:371-381).  fp64 like the
    reference's ``np.zeros(..., dtype=float)`` (the loader casts the rows to fp32 afterwards)."""
    T = np.zeros((num_labels, num_labels), dtype=np.float64)
    for (j, t), v in semantic_dict.items():
        if j != t:
            T[t, j] = v
    return T


def box_locations(boxes, img_w, img_h, num_locs):
    """boxes [..., 4] pixel (x1, y1, x2, y2) (zero rows = padding), img_w / img_h broadcastable to boxes[..., 0]
    -> [..., num_locs] float32, the reference's arithmetic in float32 and in its order of operations."""
    boxes = np.asarray(boxes, dtype=np.float32)
    loc = np.zeros(boxes.shape[:-1] + (num_locs,), dtype=np.float32)
    loc[..., :4] = boxes
    # the reference divides float32 arrays by python floats: the scalar (w, h, or the DOUBLE product w*h) is rounded
    # to float32 and the division itself is a float32 one
    w64 = np.asarray(img_w, dtype=np.float64)
    h64 = np.asarray(img_h, dtype=np.float64)
    w, h, wh = w64.astype(np.float32), h64.astype(np.float32), (w64 * h64).astype(np.float32)
    if num_locs >= 5:
        loc[..., -1] = (loc[..., 3] - loc[..., 1]) * (loc[..., 2] - loc[..., 0]) / wh
    loc[..., 0] = loc[..., 0] / w
    loc[..., 1] = loc[..., 1] / h
    loc[..., 2] = loc[..., 2] / w
    loc[..., 3] = loc[..., 3] / h
    if num_locs > 5:
        loc[..., 4] = loc[..., 2] - loc[..., 0]
        loc[..., 5] = loc[..., 3] - loc[..., 1]
    return loc


def collate_records(records, seq_len, region_len, num_locs, num_labels, padding_index=1, norm_embeddings=False,
                    prior=None, batch_index=0, feat_dim=2048):
    """records: dicts with ``features`` [n, feat_dim] f32, ``boxes`` [n, 4] f32 (pixels), ``img_w``, ``img_h``,
    ``tokens`` (ids incl. <s> ... </s>), ``labels`` [L] int, ``scores`` [L] float, ``question_id``.
    prior: the dense table of ``prior_table`` (or None: zeros).  Returns the reference's 10-tuple of CPU tensors."""
    B = len(records)
    feats = np.zeros((B, region_len, feat_dim), dtype=np.float32)
    boxes = np.zeros((B, region_len, 4), dtype=np.float32)
    image_mask = np.zeros((B, region_len), dtype=np.int64)
    ids = np.full((B, seq_len), padding_index, dtype=np.int64)
    input_mask = np.zeros((B, seq_len), dtype=np.int64)
    w = np.empty((B, 1), dtype=np.float64)
    h = np.empty((B, 1), dtype=np.float64)
    for b, r in enumerate(records):  # ragged parts only: copies, no arithmetic
        n = len(r["boxes"])
        f = np.asarray(r["features"], dtype=np.float32).reshape(-1, feat_dim)
        if norm_embeddings:
            f = torch.nn.functional.normalize(torch.from_numpy(f.copy()), dim=-1).numpy()
        feats[b, :n] = f
        boxes[b, :n] = np.asarray(r["boxes"], dtype=np.float32).reshape(-1, 4)
        image_mask[b, :n] = 1
        t = list(r["tokens"])
        t = [t[0]] + t[1:-1][:seq_len - 2] + [t[-1]]
        ids[b, :len(t)] = t
        input_mask[b, :len(t)] = 1
        w[b, 0], h[b, 0] = float(r["img_w"]), float(r["img_h"])
    loc = box_locations(boxes, w, h, num_locs)
    if norm_embeddings:
        with np.errstate(invalid="ignore", divide="ignore"):
            loc = loc / np.linalg.norm(loc, 2, -1, keepdims=True)
    labels = np.stack([np.asarray(r["labels"], dtype=np.int64) for r in records])
    scores = np.stack([np.asarray(r["scores"], dtype=np.float32) for r in records])
    target = torch.zeros((B, num_labels), dtype=torch.float32)
    target.scatter_(1, torch.from_numpy(labels), torch.from_numpy(scores))
    if prior is not None:
        dist = torch.from_numpy(np.ascontiguousarray(prior[labels[:, -1]])).to(torch.float32)  # one row gather
    else:
        dist = torch.zeros((B, num_labels), dtype=torch.float32)
    qid = torch.tensor([int(r["question_id"]) for r in records])
    return (torch.from_numpy(feats), torch.from_numpy(loc.astype(np.float32)), torch.from_numpy(image_mask),
            torch.from_numpy(ids), target, torch.from_numpy(input_mask), torch.zeros((B, seq_len), dtype=torch.int64),
            qid, torch.tensor(batch_index), dist)


# ---- record -> batch on the device (csrc/collate.hip) ------------------------------------------
# The host writes every record ONCE, ragged, into one pinned blob; one copy takes the blob to HBM; three kernels pad it
# into the same 10-tuple and do the arithmetic above (box locations, norm_embeddings, truncation, target scatter, prior
# row gather) there.  ``collate_records`` stays as it is: it is the yardstick of the device path.

PACK_ALIGN = 256  # every section of the blob starts on a 256-byte boundary
# section -> (dtype, trailing shape as a function of the batch's sizes); in blob order
_SECTIONS = (("feats", np.float32), ("boxes", np.float32), ("row_off", np.int64), ("whp", np.float32), ("tok", np.int64),
             ("tok_off", np.int64), ("labels", np.int64), ("scores", np.float32), ("qid", np.int64))


def _section_shapes(B, n_rows, n_tok, Lb, feat_dim):
    return {"feats": (n_rows, feat_dim), "boxes": (n_rows, 4), "row_off": (B + 1,), "whp": (B, 3), "tok": (n_tok,),
            "tok_off": (B + 1,), "labels": (B, Lb), "scores": (B, Lb), "qid": (B,)}


_pack_pools = {}  # threads -> ThreadPoolExecutor of the feature copy (numpy releases the GIL while it copies)


def _copy_rows(dst, parts, offs, threads):
    """dst[offs[j]:offs[j+1]] = parts[j] for every j, split over `threads` threads."""
    def work(k):
        for j in range(k, len(parts), threads):
            dst[offs[j]:offs[j + 1]] = parts[j]
    if threads <= 1 or len(parts) < 2 * threads:
        for j in range(len(parts)):
            dst[offs[j]:offs[j + 1]] = parts[j]
        return
    pool = _pack_pools.get(threads)
    if pool is None:
        from concurrent.futures import ThreadPoolExecutor
        pool = _pack_pools[threads] = ThreadPoolExecutor(threads, thread_name_prefix="pack_records")
    list(pool.map(work, range(threads)))


def pack_records(records, seq_len, region_len, num_locs, num_labels, feat_dim=2048, batch_index=0, out=None, threads=1):
    """The record dicts of ``collate_records`` -> ``(blob, meta)``: one ``uint8`` blob (pinned when a GPU is present; pass
    the previous blob of a prefetch slot as ``out`` and it is reused when large enough) holding the sections

        feats [N, F] f32 | boxes [N, 4] f32 | row_off [B+1] i64 | whp [B, 3] f32 | tok [sum len] i64 | tok_off [B+1] i64 |
        labels [B, Lb] i64 | scores [B, Lb] f32 | qid [B] i64          (N = sum of the box counts)

    each on a 256-byte boundary, and ``meta``: ``offsets`` (section -> byte offset), ``nbytes``, ``B``, ``n_rows``,
    ``n_tok``, ``Lb``, ``feat_dim``, ``batch_index``.  No arithmetic on features or boxes: only ``whp`` = {fl32(w), fl32(h),
    fl32(double(w) * double(h))}, the three scalars ``box_locations`` rounds on the host.  Raises ValueError for what a
    kernel must never see: more than ``region_len`` boxes, fewer than 2 tokens, a label outside [0, num_labels), label
    lists of unequal length, a feature row length other than ``feat_dim``.  A record with 0 boxes is legal.
    ``threads`` > 1 splits the one pass over the features (record -> blob) over that many threads."""
    B = len(records)
    if B < 1:
        raise ValueError("pack_records: an empty batch")
    if seq_len < 2 or not 4 <= num_locs <= 8:
        raise ValueError("pack_records: need seq_len >= 2 and 4 <= num_locs <= 8")
    feats, boxes, toks = [], [], []
    row_off = np.zeros(B + 1, dtype=np.int64)
    tok_off = np.zeros(B + 1, dtype=np.int64)
    w64 = np.empty(B, dtype=np.float64)
    h64 = np.empty(B, dtype=np.float64)
    Lb = len(records[0]["labels"])
    if Lb < 1:
        raise ValueError("pack_records: a record needs at least one label")
    labels = np.empty((B, Lb), dtype=np.int64)
    scores = np.empty((B, Lb), dtype=np.float32)
    qid = np.empty(B, dtype=np.int64)
    for b, r in enumerate(records):
        bx = np.asarray(r["boxes"], dtype=np.float32).reshape(-1, 4)
        n = len(bx)
        if n > region_len:
            raise ValueError("pack_records: record %d has %d boxes, region_len is %d" % (b, n, region_len))
        f = np.asarray(r["features"], dtype=np.float32)
        if n == 0 and f.size == 0:
            f = f.reshape(0, feat_dim)
        if f.ndim != 2 or f.shape[1] != feat_dim:
            raise ValueError("pack_records: record %d: feature rows of shape %s, feat_dim is %d" % (b, f.shape, feat_dim))
        if f.shape[0] != n:
            raise ValueError("pack_records: record %d: %d feature rows for %d boxes" % (b, f.shape[0], n))
        t = np.asarray(r["tokens"], dtype=np.int64).reshape(-1)
        if len(t) < 2:
            raise ValueError("pack_records: record %d has %d tokens (need <s> ... </s>: at least 2)" % (b, len(t)))
        lab = np.asarray(r["labels"], dtype=np.int64).reshape(-1)
        sc = np.asarray(r["scores"], dtype=np.float32).reshape(-1)
        if len(lab) != Lb or len(sc) != Lb:
            raise ValueError("pack_records: record %d has %d labels / %d scores, record 0 has %d" % (b, len(lab), len(sc), Lb))
        feats.append(f)
        boxes.append(bx)
        toks.append(t)
        row_off[b + 1] = row_off[b] + n
        tok_off[b + 1] = tok_off[b] + len(t)
        w64[b], h64[b] = float(r["img_w"]), float(r["img_h"])
        labels[b], scores[b], qid[b] = lab, sc, int(r["question_id"])
    bad = np.nonzero(((labels < 0) | (labels >= num_labels)).any(1))[0]
    if len(bad):
        raise ValueError("pack_records: record %d: label outside [0, %d)" % (bad[0], num_labels))
    n_rows, n_tok = int(row_off[-1]), int(tok_off[-1])
    shapes = _section_shapes(B, n_rows, n_tok, Lb, feat_dim)
    offsets, pos = {}, 0
    for name, dt in _SECTIONS:
        offsets[name] = pos
        pos += int(np.prod(shapes[name])) * np.dtype(dt).itemsize
        pos = (pos + PACK_ALIGN - 1) // PACK_ALIGN * PACK_ALIGN
    nbytes = pos
    if out is None or out.numel() < nbytes:
        # (grow with headroom: a ragged stream's blobs differ in size from batch to batch)
        cap = nbytes if out is None else max(nbytes, 2 * out.numel())
        out = torch.empty(cap, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    meta = dict(offsets=offsets, nbytes=nbytes, B=B, n_rows=n_rows, n_tok=n_tok, Lb=Lb, feat_dim=feat_dim,
                batch_index=int(batch_index))
    v = {k: t.numpy() for k, t in packed_views((out, meta)).items()}
    if n_rows:
        _copy_rows(v["feats"], feats, row_off, threads)  # the one pass over the features: record -> blob
        np.concatenate(boxes, axis=0, out=v["boxes"])
    np.concatenate(toks, out=v["tok"])
    v["row_off"][:], v["tok_off"][:] = row_off, tok_off
    v["whp"][:, 0], v["whp"][:, 1], v["whp"][:, 2] = w64, h64, w64 * h64  # rounded to fp32 by the assignment
    v["labels"][:], v["scores"][:], v["qid"][:] = labels, scores, qid
    return out, meta


def packed_views(packed):
    """``(blob, meta)`` (host or device blob) -> {section: typed tensor view of the blob}."""
    blob, meta = packed
    shapes = _section_shapes(meta["B"], meta["n_rows"], meta["n_tok"], meta["Lb"], meta["feat_dim"])
    out = {}
    for name, dt in _SECTIONS:
        shape = shapes[name]
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        o = meta["offsets"][name]
        tdt = torch.float32 if dt is np.float32 else torch.int64
        out[name] = blob[o:o + n].view(tdt).view(shape)
    return out


def prior_table_device(T, device):
    """The dense fp64 table of ``prior_table`` as the fp32 device table the collate kernel gathers rows from (cast once: the
    reference casts every gathered row to fp32; 13.6 MB at 1842 labels)."""
    return torch.from_numpy(np.ascontiguousarray(T, dtype=np.float64)).to(torch.float32).to(device).contiguous()


def collate_on_device(packed_dev, seq_len, region_len, num_locs, num_labels, padding_index=1, norm_embeddings=False,
                      prior32=None):
    """``packed_dev``: ``(blob on the device, meta)`` of ``pack_records``.  Three native launches on the current launch
    stream (``ops.launching``) -> the 10-tuple of ``collate_records`` on the device: same order, shapes and dtypes
    (``ix`` the 0-dim ``batch_index`` tensor).  Bit-equal to ``collate_records`` except the L2-normalised features of
    ``norm_embeddings``, which are within 2 * 2^-24 relative of the exact quotient (torch's CPU result is ~4 * 2^-24 off)."""
    from . import ops
    blob, meta = packed_dev
    if not blob.is_cuda:
        raise RuntimeError("clg_vqa_amd.records.collate_on_device: the blob must be on the MI355X (no CPU path; the host "
                           "routine is collate_records)")
    dev, B, F = blob.device, meta["B"], meta["feat_dim"]
    if prior32 is not None and (prior32.dtype != torch.float32 or tuple(prior32.shape) != (num_labels, num_labels)):
        raise ValueError("collate_on_device: prior32 must be the fp32 [num_labels, num_labels] table of prior_table_device")
    v = packed_views(packed_dev)
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    feats = torch.empty((B, region_len, F), **f32)
    loc = torch.empty((B, region_len, num_locs), **f32)
    image_mask = torch.empty((B, region_len), **i64)
    ids = torch.empty((B, seq_len), **i64)
    input_mask = torch.empty((B, seq_len), **i64)
    segment_ids = torch.empty((B, seq_len), **i64)
    target = torch.empty((B, num_labels), **f32)
    dist = torch.empty((B, num_labels), **f32)
    ops.collate_regions(v["feats"], v["boxes"], v["row_off"], v["whp"], feats, loc, image_mask, norm_embeddings)
    ops.collate_text(v["tok"], v["tok_off"], ids, input_mask, segment_ids, padding_index)
    ops.collate_targets(v["labels"], v["scores"], prior32, target, dist)
    ix = torch.full((), meta["batch_index"], dtype=torch.int64, device=dev)
    return (feats, loc, image_mask, ids, target, input_mask, segment_ids, v["qid"], ix, dist)
