// mm_epilogue.h -- how a C block leaves the wave that summed it: the one epilogue of the fp64 kernels that give a wave a whole C block of
// compile-time size (cblock_f64_exact in mm_numeric_f64.h, cblock_f64_classes and mm_class_stream_body in mm_exact.h, cblock_f64_dma in
// mm_dma.h, mm_numeric_f64_group in mm_group64.hip), and the 64-lane sum every kernel of the library reduces with.
//
//   wave_sum        x summed over the 64 lanes, in lane 0
//   acc_norm2       ||alpha * acc||^2 over the M x N valid elements, in every lane: the announced final filter's early-out
//   stage_c_block   alpha * acc into the wave's LDS slice, laid out as C stores the block
//   store_c_block   slice (+ beta * C_in) -> C in whole 1 KiB pieces, the stored block's squared norm -> *norm_out
//
// mm_numeric_f64_mid (run-time extents, an accumulator visitor) keeps a body of its own and follows the same rules.
// Plain on purpose: this text is also handed to hiprtc (mm_jit.hip) with mm_exact.h.
#ifndef DBCSR_AMD_MM_EPILOGUE_H
#define DBCSR_AMD_MM_EPILOGUE_H
#include "mm_types.h"
#include "smm_core.h"

namespace dbcsr_amd {

template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;  // (lane 0's is the sum)
}

// A filtered multiply whose final block filter is known (dbcsr_amd_mm_expect_filter; drop_below = its eps^2): a NEW block (no C_in: the usual case of a sparse
// product) has its norm in the accumulators.  The caller forms it with this BEFORE anything touches LDS, writes it to its norm_out (the double the filter
// compares: filter_flags), and a block the filter is going to drop (norm < drop_below) is neither staged nor written.  Nobody reads it.
template <int M, int N, int MA, int NC>
__device__ __forceinline__ double acc_norm2(const double (&acc)[MA][NC], double alpha, const LaneMap& L) {
  double s2 = 0.0;
#pragma unroll
  for (int a = 0; a < MA; ++a)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int row = 8 * a + L.rowd, col = 8 * c + L.coll;
      const double v = alpha * acc[a][c];
      if (row < M && col < N) s2 += v * v;
    }
  return __shfl(wave_sum(s2), 0, 64);
}

// C epilogue through LDS, first half: the block is laid out as stored (column-major, contiguous) in the wave's slice (M * N doubles, rounded up to 1 KiB)
template <int M, int N, int MA, int NC>
__device__ __forceinline__ void stage_c_block(double* lds_c, const double (&acc)[MA][NC], double alpha, const LaneMap& L) {
#pragma unroll
  for (int a = 0; a < MA; ++a)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int row = 8 * a + L.rowd, col = 8 * c + L.coll;
      if (row < M && col < N) lds_c[row + M * col] = alpha * acc[a][c];
    }
}

// ... second half: the staged block leaves in whole 1 KiB pieces -- 16 B per lane, full cache lines except at the two ends of the block -- with the
// streaming hint, so that the 8.6 GB of C that config 2 writes do not push the A block-rows out of L2 / the B panel out of the Infinity Cache.
// (Non-temporal on scattered 8-byte stores doubled WRITE_SIZE: partial lines are not combined.)  c_blk: the block in C_out; cin_blk: the block in C_in
// (beta * C_in is added per element) or nullptr for a new block; norm_out (or nullptr): receives the squared Frobenius norm of the block AS STORED, which
// the final block filter of a filtered multiply reads instead of C.  It is summed AFTER the stores, from the pieces still in registers: summed inside the
// piece loop, the arithmetic was if-converted in front of the stores (config 4's shape: + 0.8 ms, profiles/epilogue_shared.txt).
// streaming = false: plain stores (the lab's DBCSR_AMD_MM_DBG bit 16; a constant true everywhere else).
//
// THE STORE-DATA HAZARD.  The 16-byte stores below carry their piece offset in the VECTOR / immediate offset, never in the scalar offset: a buffer store of
// more than 64 bits whose soffset is an SGPR is NOT covered by the compiler's store-data hazard rule (it assumes none), yet on gfx950 a VALU write to the data
// registers right behind such a store reaches the store: the class (9, 32) kernel returned 16 elements per block with the low dword 0x100 (the next
// instruction's constant) in 0.2 % of the blocks (round 6, profiles/r06_store_data_hazard.txt).  Every wide buffer store of the library obeys this.
template <int M, int N>
__device__ __forceinline__ void store_c_block(const char* lds_c, double* c_blk, const double* cin_blk, double beta, int lane, double* norm_out,
                                              bool streaming = true) {
  constexpr int CC = (M * N * 8 + 1023) / 1024;
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  const int voff = lane * 16;
  const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc((void*)c_blk, 0, M * N * 8, 0x00020000);
  f64x2 v[CC];
  auto store = [&](int c) {
    if (streaming)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v[c]), rsc, voff + c * 1024, 0, 2);
    else
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v[c]), rsc, voff + c * 1024, 0, 0);
  };
  if (cin_blk) {
    const __amdgpu_buffer_rsrc_t rsi = __builtin_amdgcn_make_buffer_rsrc((void*)cin_blk, 0, M * N * 8, 0x00020000);
    u32x4 ci[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) ci[c] = __builtin_amdgcn_raw_buffer_load_b128(rsi, voff, c * 1024, 0);
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      v[c] = *reinterpret_cast<const f64x2*>(lds_c + c * 1024 + voff);
      const f64x2 w = __builtin_bit_cast(f64x2, ci[c]);
      v[c][0] += beta * w[0];
      v[c][1] += beta * w[1];
      store(c);
    }
  } else {
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      v[c] = *reinterpret_cast<const f64x2*>(lds_c + c * 1024 + voff);
      store(c);
    }
  }
  if (norm_out) {  // (the final values, per lane in piece order, then over the lanes: the pieces are still in registers, no second pass over the slice)
    double ss = 0.0;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      const int idx = c * 128 + 2 * lane;
      if (idx < M * N) ss += v[c][0] * v[c][0];
      if (idx + 1 < M * N) ss += v[c][1] * v[c][1];
    }
    ss = wave_sum(ss);
    if (lane == 0) *norm_out = ss;
  }
}

}  // namespace dbcsr_amd
#endif
