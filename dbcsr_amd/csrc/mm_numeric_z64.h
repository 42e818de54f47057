// mm_numeric_z64.h -- complex_8 block products: ONE WAVE per C block, two fp64 accumulator sets, operands in slabs of 8 inner indices
// Part of the device-resident multiply engine: included by mm_engine.hip after the fp64 / fp32 kernels.
//
// A complex product is four real ones on the same fragments: per 4-deep k step and 8 x 8 tile
//   accR += Ar * Br;  accR += (-Ai) * Bi;  accI += Ar * Bi;  accI += Ai * Br          (v_mfma_f64_4x4x4_4b, in this order, always)
// for MA + NC fragment reads of 16 bytes -- one ds_read_b128 yields (re, im) of a fragment element -- against the MA + NC reads of 8 bytes that feed
// MA * NC instructions in the real kernels: twice the MFMA work per LDS byte and per fabric byte.  -Ai is formed once per fragment read (a sign flip).
// No 3-multiplication form: it changes the rounding and saves work on a pipe that does not bound these kernels.
//   * dataflow of the fp64 kernels: all products of the block summed in ascending k in the accumulators (LaneMap of smm_core.h), C read at most once and
//     written once, no atomics: bitwise reproducible;
//   * a product is consumed in slabs of 8 inner indices, one element (16 bytes) per lane and load: A's slab is the (8 MA) x 8 piece of the block's rows
//     from row0 on (contiguous in memory when the tile starts at row 0 and the block has 8 MA rows), B's slab 8 NC runs of 8 elements.  The loads are raw
//     buffer loads whose descriptor covers exactly the block; an element past the k extent, past the block's last row / column is asked for beyond the
//     descriptor and comes back as zero: the k tail and the padding rows / columns contribute exact zeros.  The next slab is in flight in registers while
//     the current one is multiplied; one LDS buffer is enough (a wave's LDS operations complete in order);
//   * in LDS a column of A's slab has a pitch of 8 MA + 1 elements and a column of B's slab of 9: the granule of a lane is a whole element, so the pad
//     costs 16 bytes per column and nothing else.  The slice of <4, 4> is 8832 bytes per wave;
//   * one instance per (MA, NC), MA, NC = 1 ... 4: a multiply launches the instance of its LARGEST C block (MA = ceil(min(max_m, 32) / 8), NC likewise) and
//     smaller blocks run in it with zero rows / columns that are never stored -- the padding waste on mixed sizes is accepted for this first kernel.  A
//     block dimension above 32 is covered in tiles of 8 MA x 8 NC (then MA / NC = 4), one after the other in the same wave, each tile walking the
//     product list again;
//   * epilogue: C = alpha * acc + beta * C_in in complex arithmetic per element, one 16-byte store per lane and tile (plain stores: the store-data hazard
//     of mm_epilogue.h concerns wide BUFFER stores with a scalar offset).  No norms are left: the block filter computes them.
#ifndef DBCSR_AMD_MM_NUMERIC_Z64_H
#define DBCSR_AMD_MM_NUMERIC_Z64_H

#include "mm_complex.h"
#include "mm_types.h"
#include "smm_core.h"

namespace dbcsr_amd {

// flags: bit 0: C blocks without products stay as they are (in-place accumulation).  order: the launch order (npos positions, -1 = padding) or null: one
// wave per C block in index order.
template <int MA, int NC>
__global__ void __launch_bounds__(256) mm_numeric_z64(const Desc* __restrict__ descs, int64_t nblk, const Entry* __restrict__ entries,
                                                      const z64* __restrict__ a_data, const z64* __restrict__ b_data, z64* __restrict__ c_out,
                                                      const z64* __restrict__ c_in, double alpha_re, double alpha_im, double beta_re, double beta_im,
                                                      int flags, const int* __restrict__ order, int64_t npos) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TR = 8 * MA, TC = 8 * NC;      // rows / columns of a tile
  constexpr int PA = TR + 1, PB = 9;           // column pitch of the two slabs in LDS, in elements
  constexpr int ABYTES = 8 * PA * 16, SLICE = ABYTES + TC * PB * 16;
  static_assert(SLICE == z64_slice_bytes(MA, NC), "the launcher sizes the dynamic LDS with z64_slice_bytes");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t pos = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  int64_t cb = pos;
  if (order) {
    if (pos >= npos) return;
    cb = order[pos];
  }
  if (cb < 0 || cb >= nblk) return;
  const Desc d = descs[cb];
  const int cnt = __builtin_amdgcn_readfirstlane(d.prod_cnt);
  if ((flags & 1) && cnt == 0) return;
  const int m = __builtin_amdgcn_readfirstlane((int)d.m), n = __builtin_amdgcn_readfirstlane((int)d.n);
  const Entry* e = entries + d.prod_start;
  char* slice = smem + wave * SLICE;
  const f64x2* la = reinterpret_cast<const f64x2*>(slice);
  const f64x2* lb = reinterpret_cast<const f64x2*>(slice + ABYTES);
  const LaneMap L(lane);
  const bool has_in = d.cin_off >= 0;
  const f64x2* Ci = reinterpret_cast<const f64x2*>(c_in) + (has_in ? d.cin_off : 0);
  f64x2* C = reinterpret_cast<f64x2*>(c_out) + d.c_off;
  auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };

  for (int col0 = 0; col0 < n; col0 += TC) {
    for (int row0 = 0; row0 < m; row0 += TR) {
      double accR[MA][NC], accI[MA][NC];
#pragma unroll
      for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int c = 0; c < NC; ++c) accR[a][c] = 0.0, accI[a][c] = 0.0;
      u32x4 ga[MA], gb[NC];
      // the slab [k0, k0 + 8) of the product (a_lo, b_lo, w): element r * 64 + lane of A's piece (row fastest) and of B's (k fastest)
      auto issue = [&](uint32_t a_lo, uint32_t b_lo, uint32_t w, int k0) __attribute__((always_inline)) {
        const int ks = (int)(w & 0xffffu);
        const uint64_t a_off = (uint64_t)a_lo | ((uint64_t)((w >> 16) & 0xffu) << 32), b_off = (uint64_t)b_lo | ((uint64_t)(w >> 24) << 32);
        const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)(a_data + a_off), 0, m * ks * 16, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc((void*)(b_data + b_off), 0, ks * n * 16, 0x00020000);
#pragma unroll
        for (int r = 0; r < MA; ++r) {
          const int i = r * 64 + lane, kk = i / TR, row = row0 + i % TR;
          const int off = (row < m && k0 + kk < ks) ? ((k0 + kk) * m + row) * 16 : 0x7ffffff0;   // (past the descriptor: zero)
          ga[r] = __builtin_amdgcn_raw_buffer_load_b128(rsa, off, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < NC; ++r) {
          const int i = r * 64 + lane, kk = i & 7, col = col0 + (i >> 3);
          const int off = (col < n && k0 + kk < ks) ? (col * ks + k0 + kk) * 16 : 0x7ffffff0;
          gb[r] = __builtin_amdgcn_raw_buffer_load_b128(rsb, off, 0, 0);
        }
      };
      auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < MA; ++r) {
          const int i = r * 64 + lane;
          *reinterpret_cast<u32x4*>(slice + ((i / TR) * PA + i % TR) * 16) = ga[r];
        }
#pragma unroll
        for (int r = 0; r < NC; ++r) {
          const int i = r * 64 + lane;
          *reinterpret_cast<u32x4*>(slice + ABYTES + ((i >> 3) * PB + (i & 7)) * 16) = gb[r];
        }
      };
      // the current product and its successor as plain scalars (a record handed to the lambda would land in scratch)
      uint32_t ea = 0, eb = 0, ew = 0;
      if (cnt > 0) {
        ea = uni(e[0].a_lo), eb = uni(e[0].b_lo), ew = uni(e[0].w);
        issue(ea, eb, ew, 0);
      }
      int p = 0, k0 = 0;
      while (p < cnt) {
        const int ks = (int)(ew & 0xffffu);
        const int rem = (ks - k0 + 3) >> 2;   // k steps of this slab: 0 (an empty product), 1 or 2
        stage();
        int p2 = p, k2 = k0 + 8;
        if (k2 >= ks) {
          p2 = p + 1, k2 = 0;
          if (p2 < cnt) ea = uni(e[p2].a_lo), eb = uni(e[p2].b_lo), ew = uni(e[p2].w);
        }
        if (p2 < cnt) issue(ea, eb, ew, k2);   // in flight while this slab is multiplied
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (s < rem) {
            double ar[MA], ai[MA], an[MA], br[NC], bi[NC];
#pragma unroll
            for (int a = 0; a < MA; ++a) {
              const f64x2 v = la[(4 * s + L.kq) * PA + 8 * a + L.rowl];
              ar[a] = v[0], ai[a] = v[1], an[a] = -v[1];
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              const f64x2 v = lb[(8 * c + L.coll) * PB + 4 * s + L.kq];
              br[c] = v[0], bi[c] = v[1];
            }
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
              for (int c = 0; c < NC; ++c) {
                accR[a][c] = __builtin_amdgcn_mfma_f64_4x4x4f64(ar[a], br[c], accR[a][c], 0, 0, 0);
                accR[a][c] = __builtin_amdgcn_mfma_f64_4x4x4f64(an[a], bi[c], accR[a][c], 0, 0, 0);
                accI[a][c] = __builtin_amdgcn_mfma_f64_4x4x4f64(ar[a], bi[c], accI[a][c], 0, 0, 0);
                accI[a][c] = __builtin_amdgcn_mfma_f64_4x4x4f64(ai[a], br[c], accI[a][c], 0, 0, 0);
              }
          }
        }
        p = p2, k0 = k2;
      }
      // C = alpha * acc + beta * C_in, one element per lane and tile
#pragma unroll
      for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int row = row0 + 8 * a + L.rowd, col = col0 + 8 * c + L.coll;
          if (row < m && col < n) {
            const size_t idx = row + (size_t)m * col;
            f64x2 v;
            v[0] = alpha_re * accR[a][c] - alpha_im * accI[a][c];
            v[1] = alpha_re * accI[a][c] + alpha_im * accR[a][c];
            if (has_in) {
              const f64x2 w = Ci[idx];
              v[0] += beta_re * w[0] - beta_im * w[1];
              v[1] += beta_re * w[1] + beta_im * w[0];
            }
            C[idx] = v;
          }
        }
    }
  }
}

}  // namespace dbcsr_amd
#endif
