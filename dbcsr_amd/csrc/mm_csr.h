// mm_csr.h -- element CSR <-> block-sparse on the device: dbcsr_amd_bcsr_to_csr_count / _to_csr_apply (csr_row_slots, csr_slot_widths, csr_count, csr_crow,
// csr_emit), dbcsr_amd_bcsr_from_csr (csr_scatter) and dbcsr_amd_bcsr_csr_name_blocks (csr_name_blocks).  Part of the device-resident multiply engine:
// included by mm_engine.hip after mm_dense.h, whose tile (kDenseTile, dense_pitch) and whose pitch argument it takes over unchanged.
//
// The reference library has this conversion (dbcsr_csr_create_from_dbcsr, dbcsr_convert_dbcsr_to_csr, dbcsr_convert_csr_to_dbcsr, dbcsr_to_csr_filter in
// src/ops/dbcsr_csr_conversions.F); its source could not be consulted here, so the rule of the eps filter below -- an element is DROPPED iff |x| <= eps --
// is the semantics of this library.
//
// The CSR form: crow[n_rows + 1] int64 (positions pass 2^31 on matrices that fit one GPU), col[nnz] int32, 0-based element columns ascending inside a row,
// values[nnz] of the matrix' type.  A block is column by column at an element offset of its data area (blk_p); CSR is row by row with a position per
// element that depends on the data (with eps) or on the index alone (without): a transposing move, as dense_gather is, with a compaction behind it.
//   count   a slot per (element row, stored block of its block row), row by row: slot(i, b) = base[R] + p nb_R + (b - row_p[R]), p the row inside block row
//           R and nb_R the blocks of that block row.  The slot holds the number of kept elements of that row piece: the block's column count without eps
//           (csr_slot_widths: the index alone, no element is read), the count over the tile with eps (csr_count).  ONE exclusive scan in 64 bits over
//           the slots gives every row piece its CSR position; crow[i] is the scanned value of row i's first slot (csr_crow).
//   emit    one workgroup per (block row, every S-th block of it).  The block is read by the walk of mm_block_walk.h (16 bytes per lane, aligned on the
//           block) tile by tile of up to 32 x 32 through LDS at the odd pitch of mm_dense.h.  The CSR side takes a row piece of the tile per half wave,
//           consecutive lanes on consecutive columns q: the kept flag, a ballot, the popcount of the lanes below for the rank; the lane stores
//           col = col_start[C] + q and the value at pos + rank -- consecutive lanes write consecutive addresses within a row piece.  Blocks of any
//           dimension: the loops run over tiles, the pieces of one row of a block wider than a tile follow each other (a running count per row).
//   scatter the same split.  Per tile two binary searches per row give the CSR run of that row inside the tile's column range; the tile in LDS is
//           cleared, the run is dropped into it, the walk drains it to the block: every element of the block is stored once, zeros included.
// No atomics, the same bits on every call; every offset into the data area, col and values is formed in 64 bits; every position formed from crow is
// clamped to [0, nnz], and an emit never stores at or behind the position of the next row piece (a data area that changed between count and emit
// gives wrong values, never an access outside col / values).
#ifndef DBCSR_AMD_MM_CSR_H
#define DBCSR_AMD_MM_CSR_H
#include "mm_dense.h"

namespace dbcsr_amd {

// the eps filter: an element is dropped iff |x| <= eps -- real types compare in their own precision, complex ones hypot(re, im) in double; a NaN stays
__device__ __forceinline__ bool csr_kept(double x, double eps) { return !(fabs(x) <= eps); }
__device__ __forceinline__ bool csr_kept(float x, double eps) { return !(fabsf(x) <= (float)eps); }
__device__ __forceinline__ bool csr_kept(z64 x, double eps) { return !(hypot(x.re, x.im) <= eps); }

// tile[p P + q] <- blk[(p0 + p) + (q0 + q) mb], p < tp, q < tq: the block side of dense_put_transposing
template <typename T>
__device__ __forceinline__ void csr_tile_in(const T* __restrict__ blk, int64_t off, int mb, int p0, int tp, int q0, int tq, T* tile, int tid, int vec_ok) {
  constexpr int P = dense_pitch();
  if (mb <= kDenseTile) {   // (p0 = 0, tp = mb: the tile's columns are one run)
    const int run = q0 * mb;
    walk_block_values<T>(blk + run, off + run, mb * tq, tid, 256, vec_ok, [&](int e, T x) {
      const int q = e / mb;
      tile[(e - q * mb) * P + q] = x;
    });
  } else {
    for (int q = tid >> 6; q < tq; q += 4) {
      const int run = (q0 + q) * mb + p0;
      walk_block_values<T>(blk + run, off + run, tp, tid & 63, 64, vec_ok, [&](int e, T x) { tile[e * P + q] = x; });
    }
  }
}

// blk[(p0 + p) + (q0 + q) mb] <- tile[p P + q]: the block side of dense_take_transposing
template <typename T>
__device__ __forceinline__ void csr_tile_out(T* __restrict__ blk, int64_t off, int mb, int p0, int tp, int q0, int tq, const T* tile, int tid, int vec_ok) {
  constexpr int P = dense_pitch();
  if (mb <= kDenseTile) {
    const int run = q0 * mb;
    T* dst = blk + run;
    auto at = [&](int e) {
      const int q = e / mb;
      return tile[(e - q * mb) * P + q];
    };
    walk_block<T>(
        off + run, mb * tq, tid, 256, vec_ok, [&](int e) { dst[e] = at(e); },
        [&](int e) {
          Pack16<T> x;
#pragma unroll
          for (int u = 0; u < Pack16<T>::V; ++u) x.v[u] = at(e + u);
          *reinterpret_cast<Pack16<T>*>(dst + e) = x;
        });
  } else {
    for (int q = tid >> 6; q < tq; q += 4) {
      const int run = (q0 + q) * mb + p0;
      T* dst = blk + run;
      walk_block<T>(
          off + run, tp, tid & 63, 64, vec_ok, [&](int e) { dst[e] = tile[e * P + q]; },
          [&](int e) {
            Pack16<T> x;
#pragma unroll
            for (int u = 0; u < Pack16<T>::V; ++u) x.v[u] = tile[(e + u) * P + q];
            *reinterpret_cast<Pack16<T>*>(dst + e) = x;
          });
    }
  }
}

// rows of a tile per half wave: half h of the eight takes the rows h, h + 8, h + 16, h + 24
constexpr int kCsrRowsPerHalf = kDenseTile / 8;

// the half wave's 32 bits of a ballot
__device__ __forceinline__ unsigned csr_half_mask(unsigned long long mask, int tid) { return (tid & 32) ? (unsigned)(mask >> 32) : (unsigned)mask; }

// ---- count -----------------------------------------------------------------------------------------------------------------------------------------------
// slots of a block row: rows times blocks (saturated: the host refuses a total above 2^31 - 1)
__global__ void __launch_bounds__(256) csr_row_slots(const int* __restrict__ row_p, const int* __restrict__ rs, int nbr, int* __restrict__ out) {
  const int R = blockIdx.x * blockDim.x + threadIdx.x;
  if (R >= nbr) return;
  const int64_t v = (int64_t)rs[R] * (int64_t)(row_p[R + 1] - row_p[R]);
  out[R] = v > 0x7fffffff ? 0x7fffffff : (v < 0 ? 0 : (int)v);
}

// without eps: every row piece keeps the block's columns -- the index alone, no element of the data area is read.  One workgroup per (block row, sub of S)
__global__ void __launch_bounds__(256) csr_slot_widths(const int* __restrict__ row_p, const int* __restrict__ col_i, const int* __restrict__ rs,
                                                       const int* __restrict__ cs, const int64_t* __restrict__ base, int nbr, int S,
                                                       int* __restrict__ slots) {
  const int R = (int)(blockIdx.x / (unsigned)S), sub = (int)(blockIdx.x - (unsigned)R * (unsigned)S);
  if (R >= nbr) return;
  const int first = row_p[R], nb = row_p[R + 1] - first;
  if (nb <= 0) return;
  const int64_t n = (int64_t)rs[R] * nb, bR = base[R];
  for (int64_t t = (int64_t)sub * 256 + threadIdx.x; t < n; t += (int64_t)S * 256) slots[bR + t] = cs[col_i[first + (int)t % nb]];   // (n is below 2^31)
}

// with eps: the kept elements of every row piece, counted over the tile.  One workgroup per (block row, every S-th block of it)
template <typename T>
__global__ void __launch_bounds__(256) csr_count(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                 const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs,
                                                 const int64_t* __restrict__ base, int nbr, int S, double eps, int vec_ok, int* __restrict__ slots) {
  __shared__ T tile[kDenseTile * dense_pitch()];
  constexpr int P = dense_pitch();
  const int tid = threadIdx.x, half = tid >> 5, hq = tid & 31;
  const int R = (int)(blockIdx.x / (unsigned)S), sub = (int)(blockIdx.x - (unsigned)R * (unsigned)S);
  if (R >= nbr) return;
  const int m = rs[R], first = row_p[R], nb = row_p[R + 1] - first;
  const int64_t bR = base[R];
  for (int b = first + sub; b < first + nb; b += S) {
    const int n = cs[col_i[b]];
    const int64_t off = blk_p[b];
    for (int p0 = 0; p0 < m; p0 += kDenseTile) {
      const int tp = min(kDenseTile, m - p0);
      int run[kCsrRowsPerHalf];
#pragma unroll
      for (int k = 0; k < kCsrRowsPerHalf; ++k) run[k] = 0;
      for (int q0 = 0; q0 < n; q0 += kDenseTile) {
        const int tq = min(kDenseTile, n - q0);
        csr_tile_in<T>(data + off, off, m, p0, tp, q0, tq, tile, tid, vec_ok);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kCsrRowsPerHalf; ++k) {
          const int p = half + 8 * k;
          const bool kept = p < tp && hq < tq && csr_kept(tile[p * P + hq], eps);
          run[k] += __popc(csr_half_mask(__ballot(kept), tid));
        }
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < kCsrRowsPerHalf; ++k) {
        const int p = half + 8 * k;
        if (hq == 0 && p < tp) slots[bR + (int64_t)(p0 + p) * nb + (b - first)] = run[k];
      }
    }
  }
}

// crow[i] = the position of row i's first slot; a block row without blocks has none: its rows take the position of what follows.  One workgroup per block row
__global__ void __launch_bounds__(256) csr_crow(const int* __restrict__ row_p, const int* __restrict__ rs, const int64_t* __restrict__ roff,
                                                const int64_t* __restrict__ base, const int64_t* __restrict__ pos, int nbr, int64_t* __restrict__ crow) {
  const int R = blockIdx.x;
  if (R >= nbr) return;
  const int m = rs[R], nb = row_p[R + 1] - row_p[R];
  const int64_t r0 = roff[R], bR = base[R];
  for (int p = threadIdx.x; p < m; p += 256) crow[r0 + p] = pos[bR + (int64_t)p * nb];
  if (R == nbr - 1 && threadIdx.x == 0) crow[roff[nbr]] = pos[base[nbr]];
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) csr_emit(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs,
                                                const int64_t* __restrict__ coff, const int64_t* __restrict__ base, const int64_t* __restrict__ pos,
                                                int nbr, int S, int use_eps, double eps, int vec_ok, int32_t* __restrict__ col, T* __restrict__ values) {
  __shared__ T tile[kDenseTile * dense_pitch()];
  constexpr int P = dense_pitch();
  const int tid = threadIdx.x, half = tid >> 5, hq = tid & 31;
  const int R = (int)(blockIdx.x / (unsigned)S), sub = (int)(blockIdx.x - (unsigned)R * (unsigned)S);
  if (R >= nbr) return;
  const int m = rs[R], first = row_p[R], nb = row_p[R + 1] - first;
  const int64_t bR = base[R];
  for (int b = first + sub; b < first + nb; b += S) {
    const int Cb = col_i[b], n = cs[Cb], c0 = (int)coff[Cb];
    const int64_t off = blk_p[b];
    for (int p0 = 0; p0 < m; p0 += kDenseTile) {
      const int tp = min(kDenseTile, m - p0);
      int run[kCsrRowsPerHalf];
#pragma unroll
      for (int k = 0; k < kCsrRowsPerHalf; ++k) run[k] = 0;
      for (int q0 = 0; q0 < n; q0 += kDenseTile) {
        const int tq = min(kDenseTile, n - q0);
        csr_tile_in<T>(data + off, off, m, p0, tp, q0, tq, tile, tid, vec_ok);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kCsrRowsPerHalf; ++k) {
          const int p = half + 8 * k;
          const bool in = p < tp && hq < tq;
          const T x = in ? tile[p * P + hq] : dense_zero<T>();
          const bool kept = in && (!use_eps || csr_kept(x, eps));
          const unsigned mine = csr_half_mask(__ballot(kept), tid);
          if (kept) {
            const int64_t slot = bR + (int64_t)(p0 + p) * nb + (b - first);
            const int64_t at = pos[slot] + run[k] + __popc(mine & ((1u << hq) - 1u));
            if (at < pos[slot + 1]) {
              col[at] = c0 + q0 + hq;
              values[at] = x;
            }
          }
          run[k] += __popc(mine);
        }
        __syncthreads();
      }
    }
  }
}

// ---- CSR -> blocks ---------------------------------------------------------------------------------------------------------------------------------------
// first position in [lo, hi) whose column is not below c (columns ascend inside a row: the contract)
__device__ __forceinline__ int64_t csr_lower_bound(const int32_t* __restrict__ col, int64_t lo, int64_t hi, int c) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (col[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t csr_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Every element of every block the index names <- the CSR value at its (row, column), +0.0 where the CSR has none; nothing else of the data area is
// written.  One workgroup per (block row, every S-th block of it).
template <typename T>
__global__ void __launch_bounds__(256) csr_scatter(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                   T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs,
                                                   const int64_t* __restrict__ roff, const int64_t* __restrict__ coff, int nbr, int S, int vec_ok,
                                                   const int64_t* __restrict__ crow, const int32_t* __restrict__ col, const T* __restrict__ values,
                                                   int64_t nnz) {
  __shared__ T tile[kDenseTile * dense_pitch()];
  constexpr int P = dense_pitch();
  const int tid = threadIdx.x, half = tid >> 5, hq = tid & 31;
  const int R = (int)(blockIdx.x / (unsigned)S), sub = (int)(blockIdx.x - (unsigned)R * (unsigned)S);
  if (R >= nbr) return;
  const int m = rs[R];
  const int64_t r0 = roff[R];
  const T zero = dense_zero<T>();
  for (int b = row_p[R] + sub; b < row_p[R + 1]; b += S) {
    const int Cb = col_i[b], n = cs[Cb], c0 = (int)coff[Cb];
    const int64_t off = blk_p[b];
    for (int q0 = 0; q0 < n; q0 += kDenseTile) {
      const int tq = min(kDenseTile, n - q0);
      for (int p0 = 0; p0 < m; p0 += kDenseTile) {
        const int tp = min(kDenseTile, m - p0);
        for (int t = tid; t < tp * tq; t += 256) {
          const int p = t / tq;
          tile[p * P + (t - p * tq)] = zero;
        }
        // the run of every row of the tile: in each wave lane l < 32 searches the first entry of row l at or behind the tile's first column, lane l + 32
        // the first one behind its last column -- the 2 x 32 searches of a tile side by side, one chain of dependent loads instead of eight
        int64_t bound = 0;
        if (hq < tp) {
          const int64_t i = r0 + p0 + hq;
          const int64_t s = csr_clamp(crow[i], 0, nnz), e = csr_clamp(crow[i + 1], s, nnz);
          bound = csr_lower_bound(col, s, e, c0 + q0 + ((tid & 32) ? tq : 0));
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kCsrRowsPerHalf; ++k) {
          const int p = half + 8 * k;
          const int64_t lo = __shfl(bound, p, 64), hi = __shfl(bound, p + 32, 64);
          if (p < tp) {
            for (int64_t t = lo + hq; t < hi; t += 32) {
              const int q = col[t] - (c0 + q0);
              if ((unsigned)q < (unsigned)tq) tile[p * P + q] = values[t];   // (a CSR that breaks the contract: never outside the tile)
            }
          }
        }
        __syncthreads();
        csr_tile_out<T>(data + off, off, m, p0, tp, q0, tq, tile, tid, vec_ok);
        __syncthreads();
      }
    }
  }
}

// ---- the blocks of a CSR -----------------------------------------------------------------------------------------------------------------------------------
// the block of element index x: the last k in [0, n) with off[k] <= x (off ascends, off[n] the full length; blocks of no element are passed over), -1 outside
__device__ __forceinline__ int csr_block_of(const int64_t* __restrict__ off, int n, int64_t x) {
  if (n <= 0 || x < 0 || x >= off[n]) return -1;
  int lo = 0, hi = n;   // off[lo] <= x < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// rows[t], cols[t] <- the block of CSR entry t.  One wave per element row: the row's block is searched once, a lane per entry searches the column's.
// Entries outside the block structure are named (-1, -1); so stays every entry that no row of crow covers (the host fills both lists with -1 first).
__global__ void __launch_bounds__(256) csr_name_blocks(const int64_t* __restrict__ crow, const int32_t* __restrict__ col, int64_t nnz, int64_t n_rows,
                                                       const int64_t* __restrict__ roff, const int64_t* __restrict__ coff, int nbr, int nbc,
                                                       int32_t* __restrict__ rows, int32_t* __restrict__ cols) {
  const int lane = threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (i >= n_rows) return;
  const int64_t s = csr_clamp(crow[i], 0, nnz), e = csr_clamp(crow[i + 1], s, nnz);
  if (s >= e) return;
  const int R = csr_block_of(roff, nbr, i);
  for (int64_t t = s + lane; t < e; t += 64) {
    const int Cb = R >= 0 ? csr_block_of(coff, nbc, (int64_t)col[t]) : -1;
    rows[t] = Cb >= 0 ? R : -1;
    cols[t] = Cb;
  }
}

}  // namespace dbcsr_amd
#endif
