"""Host restatement of every dropout mask the native engine draws (test infrastructure; numpy, wrapping uint64 / uint32).

Each mask is a pure function of a counter-based hash of (seed, element), so the oracle can be handed exactly the masks
of a training step.  Conventions, all read off the kernel sources:

- seed schedule: ``EngineBase.next_seed`` / ``last_seed`` (engine.py): seed0 from (base_seed, call count), site s draws
  from seed0 * 4096 + s.  Sites: embeddings 1, 2 (M3P: 1, 2, 3), layer l: 16 l + 3 attention, 16 l + 4 LayerNorm 1,
  16 l + 5 LayerNorm 2 (stack.hip seed_of), pooled vector 4090 (head.py HEAD_SEED_SITE).
- LayerNorm (layernorm.hip, common.h vl_dropout_scale4): one splitmix64 per aligned group of 4 elements, element t of
  the group uses bits [16 t, 16 t + 16), threshold round(p * 65536).  p_pre: counter r * orig_row_stride * H + c;
  p_post: seed ^ POST_SALT, counter of the INPUT row (r * orig_row_stride * H + c), not of the mapped output row.
- attention (attention2.hip drop_bits / fill_common): the seed is mixed by one splitmix64 on the host into
  (seed_lo, seed_hi); one hash32 per (row, key pair), row = (b * nh + h) * S + q, pairs per row = Spad / 2 with Spad the
  padded key count of the kernel instance; even key = low 16 bits, odd key = high 16 bits.
- head activation kernel (head.hip, common.h vl_dropout_scale): one splitmix64 per element e = m * N + n, 24-bit draw.
"""
import numpy as np

U64 = np.uint64
U32 = np.uint32
MASK64 = (1 << 64) - 1
POST_SALT = 0x5BD1E9955BD1E995
GOLDEN64 = 0x9E3779B97F4A7C15
HEAD_SITE = 4090


# ---- seed schedule --------------------------------------------------------------------------------------------------
def seed0_of(base_seed, call):
    """seed0 of the `call`-th forward (call counts from 1: next_seed increments before it draws)."""
    return (base_seed * 0x9E3779B1 + call * 0x10001) & 0x7FFFFFFFFFFF


def site_seed(seed0, site):
    return (seed0 * 4096 + site) & MASK64


def stack_sites(layer):
    """(attention, LayerNorm 1 / attention output, LayerNorm 2 / FFN output) sites of one layer."""
    s3 = 16 * layer + 3
    return s3, s3 + 1, s3 + 2


# ---- generators -----------------------------------------------------------------------------------------------------
def _mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def _splitmix(seed, idx):
    with np.errstate(over="ignore"):
        return _mix64(U64(seed & MASK64) + np.asarray(idx, dtype=U64) * U64(GOLDEN64))


def _inv_keep(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def _thr16(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))  # (uint32)(p * 65536.0f + 0.5f)


def scale4(seed, counter, p):
    """vl_dropout_scale4 at element counters `counter` (any shape, int64): keep-scale float32."""
    counter = np.asarray(counter, dtype=np.int64)
    if p <= 0:
        return np.ones(counter.shape, np.float32)
    z = _splitmix(seed, (counter >> 2).astype(U64))
    bits = (z >> (U64(16) * (counter & 3).astype(U64))) & U64(0xFFFF)
    return np.where(bits >= U64(_thr16(p)), _inv_keep(p), np.float32(0.0)).astype(np.float32)


def scale1(seed, counter, p):
    """vl_dropout_scale (24-bit draw per element)."""
    counter = np.asarray(counter, dtype=np.int64)
    if p <= 0:
        return np.ones(counter.shape, np.float32)
    u = (_splitmix(seed, counter.astype(U64)) >> U64(32)) >> U64(8)
    keep = u.astype(np.float64) / 16777216.0 >= float(np.float32(p))
    return np.where(keep, _inv_keep(p), np.float32(0.0)).astype(np.float32)


def ln_pre_mask(seed, M, H, p, orig_row_stride=1):
    """[M, H] keep-scale of vl_ln_fwd's p_pre (rows r of the call = rows r * orig_row_stride of the full problem)."""
    r = np.arange(M, dtype=np.int64)[:, None]
    c = np.arange(H, dtype=np.int64)[None, :]
    return scale4(seed, r * orig_row_stride * H + c, p)


def ln_post_mask(seed, M, H, p, orig_row_stride=1):
    """[M, H] keep-scale of vl_ln_fwd's p_post, indexed by the INPUT row of the call (the row map only moves the store)."""
    return ln_pre_mask(seed ^ POST_SALT, M, H, p, orig_row_stride)


def attn_spad(S):
    """Padded key count of the attention kernel instance that serves S (attention2.hip dispatch_fwd / dispatch_bwd)."""
    for lim, nt in ((64, 4), (80, 5), (128, 8), (144, 9), (160, 10)):
        if S <= lim:
            return 16 * nt
    raise ValueError("S must be <= 160")


def _hash32(x):
    with np.errstate(over="ignore"):
        x = x ^ (x >> U32(16))
        x = x * U32(0x7FEB352D)
        x = x ^ (x >> U32(15))
        x = x * U32(0x846CA68B)
        return x ^ (x >> U32(16))


def attn_mask(seed, B, nh, S, p):
    """[B, nh, S(query), S(key)] keep-scale of vl_attn2_fwd / vl_attn2_bwd (the same mask for nq = S and nq = 1)."""
    if p <= 0:
        return np.ones((B, nh, S, S), np.float32)
    z = int(_mix64(np.array([(seed + GOLDEN64) & MASK64], dtype=U64))[0])
    lo, hi = U32(z & 0xFFFFFFFF), U32(z >> 32)
    ppr = attn_spad(S) // 2
    row = np.arange(B * nh * S, dtype=np.int64).reshape(B, nh, S, 1)
    key = np.arange(S, dtype=np.int64).reshape(1, 1, 1, S)
    ctr = ((row * ppr + (key >> 1)) & 0xFFFFFFFF).astype(U32)
    with np.errstate(over="ignore"):
        bits = _hash32((ctr * U32(0x9E3779B1) + lo) ^ hi)
    u = np.where((key & 1) == 1, bits >> U32(16), bits & U32(0xFFFF))
    return np.where(u >= U32(_thr16(p)), _inv_keep(p), np.float32(0.0)).astype(np.float32)


def head_mask(seed, M, N, p):
    """[M, N] keep-scale of vl_act_fwd / vl_act_bwd (the pooled-vector dropout of the task head)."""
    return scale1(seed, np.arange(M * N, dtype=np.int64).reshape(M, N), p)


# ---- scalar pure-Python versions (cross-check of the vectorised ones) ------------------------------------------------
def scalar_splitmix(seed, idx):
    z = (seed + idx * GOLDEN64) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def scalar_scale4(seed, e, p):
    z = scalar_splitmix(seed, e >> 2)
    bits = (z >> (16 * (e & 3))) & 0xFFFF
    return float(_inv_keep(p)) if bits >= _thr16(p) else 0.0


def scalar_scale1(seed, e, p):
    u = (scalar_splitmix(seed, e) >> 32) >> 8
    return float(_inv_keep(p)) if u / 16777216.0 >= float(np.float32(p)) else 0.0


def scalar_attn(seed, B, nh, S, p, b, h, q, k):
    z = scalar_splitmix(seed, 1)  # seed + 1 * GOLDEN64: the host mix of fill_common
    lo, hi = z & 0xFFFFFFFF, z >> 32
    row = (b * nh + h) * S + q
    x = ((((row * (attn_spad(S) // 2) + (k >> 1)) * 0x9E3779B1) + lo) & 0xFFFFFFFF) ^ hi
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    u = x >> 16 if k & 1 else x & 0xFFFF
    return float(_inv_keep(p)) if u >= _thr16(p) else 0.0


# ---- the masks of one training step, as the oracle's mask provider -------------------------------------------------
SITE_KINDS = ("emb", "attn_probs", "attn_out", "ffn_out", "pooled")


class StepMasks(object):
    """provider(site, layer, shape) for oracle.set_mask_provider: the keep-scales the engine draws in its `call`-th forward.

    kind "uc2": sites emb_text / emb_box (seeds 1, 2); kind "m3p": emb_image (seed 1), emb_joint (image rows seed 2, text
    rows seed 3).  `wrong`: one site kind of SITE_KINDS whose masks are drawn from the neighbouring seed (site + 1) instead:
    a negative control."""

    def __init__(self, kind, base_seed, call, B, T, V, nh, p_hid, p_att, p_head, wrong=None):
        self.kind, self.B, self.T, self.V, self.nh = kind, B, T, V, nh
        self.p_hid, self.p_att, self.p_head = p_hid, p_att, p_head
        self.seed0 = seed0_of(base_seed, call)
        self.wrong = wrong
        self.calls = []

    def _seed(self, kind, site):
        return site_seed(self.seed0, site + (1 if kind == self.wrong else 0))

    def masks(self, site, layer, shape):
        B, T, V, nh = self.B, self.T, self.V, self.nh
        S = T + V
        H = shape[-1]
        if site == "emb_text":
            return ln_post_mask(self._seed("emb", 1), B * T, H, self.p_hid).reshape(shape)
        if site == "emb_box":
            return ln_post_mask(self._seed("emb", 2), B * V, H, self.p_hid).reshape(shape)
        if site == "emb_image":
            return ln_post_mask(self._seed("emb", 1), B * V, H, self.p_hid).reshape(shape)
        if site == "emb_joint":
            im = ln_post_mask(self._seed("emb", 2), B * V, H, self.p_hid).reshape(B, V, H)
            tx = ln_post_mask(self._seed("emb", 3), B * T, H, self.p_hid).reshape(B, T, H)
            return np.concatenate([im, tx], axis=1).reshape(shape)
        sa, s1, s2 = stack_sites(layer)
        if site == "attn_probs":
            return attn_mask(self._seed("attn_probs", sa), B, nh, S, self.p_att).reshape(shape)
        if site == "attn_out":
            return ln_pre_mask(self._seed("attn_out", s1), B * S, H, self.p_hid).reshape(shape)
        if site == "ffn_out":
            return ln_pre_mask(self._seed("ffn_out", s2), B * S, H, self.p_hid).reshape(shape)
        if site == "pooled":
            return head_mask(self._seed("pooled", HEAD_SITE), shape[0], shape[1], self.p_head)
        raise KeyError(site)

    def __call__(self, site, layer, shape):
        import torch
        self.calls.append((site, layer))
        return torch.from_numpy(self.masks(site, layer, tuple(shape)))
