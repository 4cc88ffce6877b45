// Device helpers shared by the LDS-DMA tile kernels (gemm.hip, dw.hip, attention2.hip): one definition each.
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void* lds_ptr_t;        // global_load_lds destination
typedef const __attribute__((address_space(1))) void* glb_ptr_t;  // ... and source
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// Bank swizzle of the ping-pong kernels' 128-byte LDS rows (XOR on the 16-byte chunk index, applied on the DMA source
// address and undone by the reads): conflict-free both for 16 consecutive rows and for the permuted rows
// {0-3, 8-11, 16-19, 24-27} + 4*(j&1) that the paired n-tiles of the 16-bit epilogues read.
__device__ __forceinline__ int swz3(int row) {
  return ((row >> 1) & 1) | (((row >> 3) & 1) << 1) | ((((row >> 4) ^ (row >> 2)) & 1) << 2);
}

// XCD-contiguous work order: workgroup `bid` of `nwg` runs on XCD bid % 8 (round-robin dispatch); the returned index gives
// every XCD one contiguous range of the work list (bijective for any nwg), so neighbours in the list -- tiles that share
// an operand panel -- sit behind one L2.
__device__ __forceinline__ int xcd_tile(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// s_waitcnt vmcnt(N) with a compile-time count: at most N vector-memory operations (LDS-DMA loads) still outstanding
template <int N> __device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Transposing fragment read: 8 k-values (rows p0.., p1.. of a [k][column] LDS image, 4 each) of column (lane & 15) of a
// 16-column block, as two ds_read_b64_tr_b16.  (dw.hip's K loop has its own inline-assembly form, see there.)
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p0, const unsigned char* p1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p1);
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// ---- host side: launch of a kernel that needs more dynamic LDS than the 64 KB default -------------------------------
// `lds` is a constant of the kernel instantiation, so the opt-in is set once per kernel (idempotent: a race only repeats
// the call).  Returns 0 or the vl_set_error code.
template <auto Kernel, class Args>
int launch_dyn_lds(const char* what, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args& args) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return vl_set_error(-3, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
    attr_set = true;
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args);
  VL_CHECK_LAUNCH(what);
  return 0;
}
