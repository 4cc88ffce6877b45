// vl_collate_regions / vl_collate_text / vl_collate_targets: record -> batch on the device.
//
// The host writes every record once, ragged, into one pinned blob (clg_vqa_amd/records.py::pack_records); one copy takes the
// blob to HBM; these three streaming kernels pad it into the reference's batch tuple and do the arithmetic the reference does
// per sample in Python (volta/volta/datasets/gqa_dataset_semantic_code_mix.py:564-651 BertPreprocessBatch.__call__, :386-452
// the loader's target scatter, :371-381 get_embeddingdist).  No atomics, every output element has exactly one writer and one
// fixed order of operations: two calls give the same bits.  Padding is WRITTEN (zeros / pad id), never assumed.
//
// Rounding.  The box-location features are pinned bit for bit to the reference's numpy float32 arithmetic, so every product,
// sum, quotient and square root there must round to fp32 on its own.  In this toolchain HIP's __fmul_rn / __fadd_rn / __fsub_rn
// / __fdiv_rn are the plain operators (the compiler may still contract them into an FMA after inlining) and __fsqrt_rn is the
// native, not correctly rounded, square root.  So: (1) contraction is switched off for this whole file with the pragma below,
// and (2) the operations that are pinned go through rn_mul / rn_add / rn_sub / rn_div / rn_sqrt, which compute in fp64 and
// round the result to fp32 once: for fp32 operands that IS the correctly rounded fp32 operation (53 >= 2 * 24 + 2 bits: the
// double rounding is innocuous for + - * / sqrt), whatever the fast-math or division flags of the build are.  They run on at
// most 8 lanes per region row.
#include "common.h"
#include "../../include/vlhip.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float rn_mul(float a, float b) { return (float)((double)a * (double)b); }
__device__ __forceinline__ float rn_add(float a, float b) { return (float)((double)a + (double)b); }
__device__ __forceinline__ float rn_sub(float a, float b) { return (float)((double)a - (double)b); }
__device__ __forceinline__ float rn_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float rn_sqrt(float a) { return (float)sqrt((double)a); }

constexpr int CL_MAXL = 8;

// One wave per output row (b, v); lane c holds the 16-byte chunks c, c + 64, ... of the feature row (NCH of them: the row is
// read once and stays in registers between the sum of squares and the scaling).  Lanes 0 .. L-1 also write the location row.
template <int NCH>
__global__ __launch_bounds__(256) void collate_regions_kernel(const float* __restrict__ feats_packed,
                                                              const float* __restrict__ boxes_packed,
                                                              const int64_t* __restrict__ row_off, const float* __restrict__ whp,
                                                              float* __restrict__ feats, float* __restrict__ loc,
                                                              int64_t* __restrict__ image_mask, int64_t B, int V, int F, int L,
                                                              int64_t n_rows, int normalize) {
  const int lane = threadIdx.x & 63;
  const int nch = F >> 2;
  const int64_t rows = B * V;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t b = row / V;
    const int v = (int)(row - b * V);
    const int64_t r0 = row_off[b], n = row_off[b + 1] - r0, src = r0 + v;
    const bool in_record = v < n;                               // the reference's image_mask[b, :n] = 1
    const bool live = in_record && src >= 0 && src < n_rows;    // (wave-uniform) never read outside the packed sections
    f32x4 x[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) x[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
      const f32x4* s = reinterpret_cast<const f32x4*>(feats_packed + src * F);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int c = lane + 64 * j;
        if (c < nch) x[j] = s[c];
      }
      if (normalize) {
        // F.normalize: x / max(||x||_2, 1e-12).  Sum of squares in fp64 (the products of fp32 values are exact there; the
        // 2048 additions lose ~1e-13 relative), a fixed butterfly across the lanes, the norm rounded to fp32 ONCE, then one
        // fp32 division per element.
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc = fma((double)x[j][k], (double)x[j][k], acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        const float d = fmaxf((float)sqrt(acc), 1e-12f);
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k) x[j][k] = x[j][k] / d;
      }
    }
    f32x4* dst = reinterpret_cast<f32x4*>(feats + row * F);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int c = lane + 64 * j;
      if (c < nch) dst[c] = x[j];
    }
    if (lane == 0) image_mask[row] = in_record ? 1 : 0;
    if (lane < L) {
      // records.box_locations operation by operation (a dead row: the same arithmetic on a zero box)
      f32x4 bx = f32x4{0.f, 0.f, 0.f, 0.f};
      if (live) bx = reinterpret_cast<const f32x4*>(boxes_packed)[src];
      const float w = whp[b * 3], h = whp[b * 3 + 1], wh = whp[b * 3 + 2];
      float q[CL_MAXL];
#pragma unroll
      for (int i = 0; i < CL_MAXL; ++i) q[i] = 0.f;
      if (L >= 5) {  // area of the RAW pixel box over the image area, into the last column
        const float area = rn_div(rn_mul(rn_sub(bx[3], bx[1]), rn_sub(bx[2], bx[0])), wh);
#pragma unroll
        for (int i = 4; i < CL_MAXL; ++i)
          if (i == L - 1) q[i] = area;
      }
      q[0] = rn_div(bx[0], w);
      q[1] = rn_div(bx[1], h);
      q[2] = rn_div(bx[2], w);
      q[3] = rn_div(bx[3], h);
      if (L > 5) {  // width and height of the NORMALISED box
        q[4] = rn_sub(q[2], q[0]);
        q[5] = rn_sub(q[3], q[1]);
      }
      if (normalize) {
        // numpy's np.linalg.norm(loc, 2, -1) for rows shorter than 8: ((s0 + s1) + s2) + ..., every s_i = fl(x_i * x_i);
        // a zero row gives 0 / 0 = NaN (the reference's quirk, reproduced)
        float s = rn_mul(q[0], q[0]);
#pragma unroll
        for (int i = 1; i < CL_MAXL; ++i)
          if (i < L) s = rn_add(s, rn_mul(q[i], q[i]));
        const float nrm = rn_sqrt(s);
#pragma unroll
        for (int i = 0; i < CL_MAXL; ++i) q[i] = rn_div(q[i], nrm);
      }
      float mine = q[0];
#pragma unroll
      for (int i = 1; i < CL_MAXL; ++i)
        if (lane == i) mine = q[i];
      loc[row * L + lane] = mine;
    }
  }
}

// one thread per (b, t): [t0] + t[1:-1][:T-2] + [t_last], padded with pad_id
__global__ __launch_bounds__(256) void collate_text_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ tok_off,
                                                           int64_t* __restrict__ ids, int64_t* __restrict__ input_mask,
                                                           int64_t* __restrict__ segment_ids, int64_t B, int T, int64_t pad_id,
                                                           int64_t n_tok) {
  const int64_t total = B * T;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / T;
    const int t = (int)(i - b * T);
    const int64_t o = tok_off[b], len = tok_off[b + 1] - o;
    const int64_t kept = len < T ? len : T;
    const int64_t src = o + (t == kept - 1 ? len - 1 : t);
    const bool on = t < kept && src >= 0 && src < n_tok;
    ids[i] = on ? tok[src] : pad_id;
    input_mask[i] = on ? 1 : 0;
    segment_ids[i] = 0;
  }
}

template <int VEC>
struct alignas(4 * VEC) ClVec { float v[VEC]; };

// one thread per VEC consecutive classes of one sample (VEC divides C, so a group never crosses a row and every group is
// 4 * VEC-byte aligned: C = 1842 runs with 8-byte accesses, an odd C with 4-byte ones)
template <int VEC>
__global__ __launch_bounds__(256) void collate_targets_kernel(const int64_t* __restrict__ labels, const float* __restrict__ scores,
                                                              const float* __restrict__ prior32, float* __restrict__ target,
                                                              float* __restrict__ dist, int Lb, int C) {
  const int64_t b = blockIdx.y;
  const int c0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (c0 >= C) return;
  ClVec<VEC> t, d;
#pragma unroll
  for (int k = 0; k < VEC; ++k) t.v[k] = d.v[k] = 0.f;
  for (int l = 0; l < Lb; ++l) {  // ascending: for a repeated label the highest l wins
    const int64_t lab = labels[b * Lb + l];
    const float sc = scores[b * Lb + l];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (lab == c0 + k) t.v[k] = sc;
  }
  const int64_t last = labels[b * Lb + Lb - 1];
  if (prior32 && last >= 0 && last < C) d = *reinterpret_cast<const ClVec<VEC>*>(prior32 + last * C + c0);
  *reinterpret_cast<ClVec<VEC>*>(target + b * C + c0) = t;
  *reinterpret_cast<ClVec<VEC>*>(dist + b * C + c0) = d;
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int vl_collate_regions(const float* feats_packed, const float* boxes_packed, const int64_t* row_off, const float* whp,
                                  float* feats, float* loc, int64_t* image_mask, int64_t B, int64_t V, int64_t F, int64_t L,
                                  int64_t n_rows, int normalize, void* stream) {
  VL_CHECK_ARG(feats_packed && boxes_packed && row_off && whp && feats && loc && image_mask,
               "vl_collate_regions: null pointer");
  VL_CHECK_ARG(B >= 1 && V >= 1 && n_rows >= 0 && B * V < (1ll << 31),
               "vl_collate_regions: need B >= 1, V >= 1, n_rows >= 0; got B %lld V %lld n_rows %lld", (long long)B,
               (long long)V, (long long)n_rows);
  VL_CHECK_ARG(F >= 4 && F % 4 == 0 && F <= 4096, "vl_collate_regions: F must be a multiple of 4, at most 4096; got %lld",
               (long long)F);
  VL_CHECK_ARG(L >= 4 && L <= CL_MAXL, "vl_collate_regions: L (num_locs) must be in [4, 8]; got %lld", (long long)L);
  VL_CHECK_ARG(aligned_to(feats_packed, 16) && aligned_to(boxes_packed, 16) && aligned_to(feats, 16) && aligned_to(row_off, 8) &&
                   aligned_to(image_mask, 8) && aligned_to(whp, 4) && aligned_to(loc, 4),
               "vl_collate_regions: feats_packed / boxes_packed / feats must be 16-byte aligned, the int64 arrays 8-byte");
  const int64_t rows = B * V;
  const unsigned grid = (unsigned)((rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048);
  const int per_lane = (int)((F / 4 + 63) / 64);
  hipStream_t s = (hipStream_t)stream;
#define CL_LAUNCH(NCH)                                                                                                      \
  hipLaunchKernelGGL(collate_regions_kernel<NCH>, dim3(grid), dim3(256), 0, s, feats_packed, boxes_packed, row_off, whp, feats, \
                     loc, image_mask, B, (int)V, (int)F, (int)L, n_rows, normalize)
  if (per_lane <= 1) CL_LAUNCH(1);
  else if (per_lane <= 4) CL_LAUNCH(4);
  else if (per_lane <= 8) CL_LAUNCH(8);
  else CL_LAUNCH(16);
#undef CL_LAUNCH
  VL_CHECK_LAUNCH("vl_collate_regions");
  return 0;
}

extern "C" int vl_collate_text(const int64_t* tok, const int64_t* tok_off, int64_t* ids, int64_t* input_mask,
                               int64_t* segment_ids, int64_t B, int64_t T, int64_t pad_id, int64_t n_tok, void* stream) {
  VL_CHECK_ARG(tok && tok_off && ids && input_mask && segment_ids, "vl_collate_text: null pointer");
  VL_CHECK_ARG(B >= 1 && T >= 2 && T <= 65536 && n_tok >= 0 && B * T < (1ll << 31),
               "vl_collate_text: need B >= 1, 2 <= T <= 65536, n_tok >= 0; got B %lld T %lld n_tok %lld", (long long)B,
               (long long)T, (long long)n_tok);
  VL_CHECK_ARG(aligned_to(tok, 8) && aligned_to(tok_off, 8) && aligned_to(ids, 8) && aligned_to(input_mask, 8) &&
                   aligned_to(segment_ids, 8), "vl_collate_text: int64 arrays must be 8-byte aligned");
  const int64_t blocks = (B * T + 255) / 256;
  hipLaunchKernelGGL(collate_text_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream,
                     tok, tok_off, ids, input_mask, segment_ids, B, (int)T, pad_id, n_tok);
  VL_CHECK_LAUNCH("vl_collate_text");
  return 0;
}

extern "C" int vl_collate_targets(const int64_t* labels, const float* scores, const float* prior32, float* target, float* dist,
                                  int64_t B, int64_t Lb, int64_t C, void* stream) {
  VL_CHECK_ARG(labels && scores && target && dist, "vl_collate_targets: null pointer");
  VL_CHECK_ARG(B >= 1 && B <= 65535 && Lb >= 1 && Lb <= 4096,
               "vl_collate_targets: need 1 <= B <= 65535 and 1 <= Lb <= 4096; got B %lld Lb %lld", (long long)B, (long long)Lb);
  VL_CHECK_ARG(C >= 1 && C <= 4096, "vl_collate_targets: C (num_labels) must be in [1, 4096]; got %lld", (long long)C);
  VL_CHECK_ARG(aligned_to(labels, 8) && aligned_to(scores, 4) && aligned_to(prior32, 4) && aligned_to(target, 4) &&
                   aligned_to(dist, 4), "vl_collate_targets: misaligned pointer");
  // the widest access every row start allows: rows are C * 4 bytes apart
  const bool base16 = aligned_to(prior32, 16) && aligned_to(target, 16) && aligned_to(dist, 16);
  const bool base8 = aligned_to(prior32, 8) && aligned_to(target, 8) && aligned_to(dist, 8);
  const int vec = (C % 4 == 0 && base16) ? 4 : (C % 2 == 0 && base8) ? 2 : 1;
  const dim3 grid((unsigned)((C / vec + 255) / 256), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
#define CL_LAUNCH(VEC) \
  hipLaunchKernelGGL(collate_targets_kernel<VEC>, grid, dim3(256), 0, s, labels, scores, prior32, target, dist, (int)Lb, (int)C)
  if (vec == 4) CL_LAUNCH(4);
  else if (vec == 2) CL_LAUNCH(2);
  else CL_LAUNCH(1);
#undef CL_LAUNCH
  VL_CHECK_LAUNCH("vl_collate_targets");
  return 0;
}
