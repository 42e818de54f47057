// mm_dense.h -- dense <-> block-sparse on the device: dbcsr_amd_bcsr_to_dense (dense_gather), dbcsr_amd_bcsr_from_dense_apply (dense_scatter) and the count
// half of dbcsr_create_from_dense (dense_block_norms, dense_emit).  Part of the device-resident multiply engine: included by mm_engine.hip after
// mm_block_inverse.h.
//
// A block is column by column at an element offset of its data area (blk_p): element (p, q) of an mb x nb block is blk[p + q mb].  The dense matrix is
// element (i, j) at dense[i sr + j sc] with (sr, sc) = (ld, 1), row by row as torch lays a tensor out, or (1, ld), column by column as a Fortran full
// matrix.  Every dense offset is formed in 64 bits (row times ld passes 2^31 at ordinary sizes).  Each side is walked along its own contiguous direction:
//   straight     the block's columns lie along the dense side's contiguous direction (a stored block into a column-by-column matrix; the twin of a stored
//                block into a row-by-row one, whose rows are the block's columns): one walk over the block (walk_block: 16 bytes per lane where the data
//                area allows), element e -> column q = e / mb, place p = e - q mb, dense[p + q ld].  Consecutive lanes meet consecutive addresses on both sides.
//   transposing  the block's columns lie across it (a stored block into a row-by-row matrix; the twin into a column-by-column one): tiles of up to
//                32 x 32 elements go through LDS.  The block side fills or drains the tile by the same walk, the dense side by runs along q.  The tile is
//                tile[p P + q] with P = dense_pitch() = 33 elements: the walk along q (consecutive q, the dense side) meets consecutive words, and the walk
//                along p (consecutive p, the block side: stride P elements) meets every bank once, since P is odd -- 4-byte elements 32 lanes over 32 banks,
//                8-byte elements 16 lanes (stores) or 32 lanes (loads: 64 banks) at a stride of 2 P words, 16-byte elements 8 or 16 lanes at 4 P words.
//                (A lane that holds a 16-byte pack of V elements stores them V places apart from its neighbour's: those stores meet V-fold.  The tile
//                moves each element once in and once out, a small fraction of what LDS delivers while HBM is waited for.)
//                A block of more than 32 rows is cut into pieces of 32 rows, one wave per column piece; a block of up to 32 rows is walked as whole runs of
//                columns by the workgroup.
// dense_gather writes every element of the window exactly once: one workgroup per (block row, group of block columns) looks every tile up in row_p / col_i
// (binary search in the ascending col_i of the row) and writes the stored block, or -- of a stored triangle -- the twin of the block stored at the mirrored
// place, or zeros.  Nothing outside the window is written, no memset is needed, nothing is written twice.  dense_scatter walks the stored blocks (one
// workgroup per block row and sub) and writes only inside them.  No atomics on data.
#ifndef DBCSR_AMD_MM_DENSE_H
#define DBCSR_AMD_MM_DENSE_H
#include "mm_algebra.h"

namespace dbcsr_amd {

constexpr int kDenseTile = 32;   // rows and columns of the LDS tile of the transposing moves
__host__ __device__ constexpr int dense_pitch() { return kDenseTile | 1; }

template <typename T> __device__ __forceinline__ T dense_zero() { return T(0); }
template <> __device__ __forceinline__ z64 dense_zero<z64>() { return z64(0.0, 0.0); }

// |x|^2 in double
__device__ __forceinline__ double dense_abs2(double x) { return x * x; }
__device__ __forceinline__ double dense_abs2(float x) { return (double)x * (double)x; }
__device__ __forceinline__ double dense_abs2(z64 x) { return x.re * x.re + x.im * x.im; }

// the element as it is (kind < 0) or as the element of the twin block (kind 0 ... 3: twin_of)
template <typename T>
__device__ __forceinline__ T dense_value(T x, int kind) { return kind < 0 ? x : twin_of(x, kind); }

// position of block (r, c) in the index, -1 when the matrix does not store it: col_i ascends inside a row
__device__ __forceinline__ int dense_find(const int* __restrict__ row_p, const int* __restrict__ col_i, int r, int c) {
  const int end = row_p[r + 1];
  int lo = row_p[r], hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (col_i[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && col_i[lo] == c ? lo : -1;
}

// ---- block -> dense ------------------------------------------------------------------------------------------------------------------------------------
// straight: dense[p + q ldq] <- value(blk[p + q mb]); `dense` is the tile's first element
template <typename T>
__device__ __forceinline__ void dense_put_straight(const T* __restrict__ blk, int64_t off, int mb, int nb, T* __restrict__ dense, int64_t ldq, int kind,
                                                   int tid, int vec_ok) {
  walk_block_values<T>(blk, off, mb * nb, tid, 256, vec_ok, [&](int e, T x) {
    const int q = e / mb;
    dense[(int64_t)q * ldq + (e - q * mb)] = dense_value(x, kind);
  });
}

// transposing: dense[p ldp + q] <- value(blk[p + q mb]) through the tile
template <typename T>
__device__ __forceinline__ void dense_put_transposing(const T* __restrict__ blk, int64_t off, int mb, int nb, T* __restrict__ dense, int64_t ldp, int kind,
                                                      T* tile, int tid, int vec_ok) {
  constexpr int P = dense_pitch();
  const int lane = tid & 63, wave = tid >> 6;
  for (int q0 = 0; q0 < nb; q0 += kDenseTile) {
    const int tq = min(kDenseTile, nb - q0);
    for (int p0 = 0; p0 < mb; p0 += kDenseTile) {
      const int tp = min(kDenseTile, mb - p0);
      if (mb <= kDenseTile) {   // (p0 = 0, tp = mb: the tile's columns are one run)
        const int run = q0 * mb;
        walk_block_values<T>(blk + run, off + run, mb * tq, tid, 256, vec_ok, [&](int e, T x) {
          const int q = e / mb;
          tile[(e - q * mb) * P + q] = dense_value(x, kind);
        });
      } else {
        for (int q = wave; q < tq; q += 4) {
          const int run = (q0 + q) * mb + p0;
          walk_block_values<T>(blk + run, off + run, tp, lane, 64, vec_ok, [&](int e, T x) { tile[e * P + q] = dense_value(x, kind); });
        }
      }
      __syncthreads();
      for (int t = tid; t < tp * tq; t += 256) {
        const int p = t / tq, q = t - p * tq;
        dense[(int64_t)(p0 + p) * ldp + (q0 + q)] = tile[p * P + q];
      }
      __syncthreads();
    }
  }
}

// The window [n_rows, n_cols] of `dense` (element (i, j) at i sr + j sc: col_major ? (1, ld) : (ld, 1)) <- the matrix.  kind < 0: the stored blocks and
// zeros.  kind 0 ... 3: a stored triangle (square block structure) -- tile (R, C) is the block stored there, else the twin of the block stored at (C, R),
// else zeros; a diagonal block is taken in full as stored.  One workgroup per (block row R, G block columns from g G on).
template <typename T>
__global__ void __launch_bounds__(256) dense_gather(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                    const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs,
                                                    const int64_t* __restrict__ roff, const int64_t* __restrict__ coff, int nbr, int nbc, int G, int NG,
                                                    int kind, int col_major, int vec_ok, T* __restrict__ dense, int64_t ld) {
  __shared__ T tile[kDenseTile * dense_pitch()];
  const int tid = threadIdx.x;
  const int R = (int)(blockIdx.x / (unsigned)NG), g = (int)(blockIdx.x - (unsigned)R * (unsigned)NG);
  if (R >= nbr) return;
  const int m = rs[R];
  const int64_t r0 = roff[R], sr = col_major ? 1 : ld, sc = col_major ? ld : 1;
  const int cend = min(nbc, (g + 1) * G);
  for (int Cb = g * G; Cb < cend; ++Cb) {
    const int n = cs[Cb];
    T* out = dense + r0 * sr + coff[Cb] * sc;
    int b = dense_find(row_p, col_i, R, Cb);
    if (b >= 0) {   // the stored block: m x n, its columns are dense columns
      const int64_t off = blk_p[b];
      if (col_major) dense_put_straight<T>(data + off, off, m, n, out, ld, -1, tid, vec_ok);
      else dense_put_transposing<T>(data + off, off, m, n, out, ld, -1, tile, tid, vec_ok);
      continue;
    }
    if (kind >= 0 && Cb != R && rs[Cb] == n && cs[R] == m) b = dense_find(row_p, col_i, Cb, R);   // (row sizes that are not the column sizes: no twin fits)
    if (b >= 0) {   // the twin of the n x m block stored at (Cb, R): its columns are dense rows
      const int64_t off = blk_p[b];
      if (col_major) dense_put_transposing<T>(data + off, off, n, m, out, ld, kind, tile, tid, vec_ok);
      else dense_put_straight<T>(data + off, off, n, m, out, ld, kind, tid, vec_ok);
      continue;
    }
    const T zero = dense_zero<T>();
    if (col_major) {
      for (int t = tid; t < m * n; t += 256) {
        const int j = t / m;
        out[(int64_t)j * ld + (t - j * m)] = zero;
      }
    } else {
      for (int t = tid; t < m * n; t += 256) {
        const int i = t / n;
        out[(int64_t)i * ld + (t - i * n)] = zero;
      }
    }
  }
}

// ---- dense -> block ------------------------------------------------------------------------------------------------------------------------------------
// straight: blk[p + q mb] <- dense[p + q ldq], 16 bytes per store where the data area allows
template <typename T>
__device__ __forceinline__ void dense_take_straight(T* __restrict__ blk, int64_t off, int mb, int nb, const T* __restrict__ dense, int64_t ldq, int tid,
                                                    int vec_ok) {
  auto at = [&](int e) {
    const int q = e / mb;
    return dense[(int64_t)q * ldq + (e - q * mb)];
  };
  walk_block<T>(
      off, mb * nb, tid, 256, vec_ok, [&](int e) { blk[e] = at(e); },
      [&](int e) {
        Pack16<T> x;
#pragma unroll
        for (int u = 0; u < Pack16<T>::V; ++u) x.v[u] = at(e + u);
        *reinterpret_cast<Pack16<T>*>(blk + e) = x;
      });
}

// transposing: blk[p + q mb] <- dense[p ldp + q] through the tile
template <typename T>
__device__ __forceinline__ void dense_take_transposing(T* __restrict__ blk, int64_t off, int mb, int nb, const T* __restrict__ dense, int64_t ldp, T* tile,
                                                       int tid, int vec_ok) {
  constexpr int P = dense_pitch();
  const int lane = tid & 63, wave = tid >> 6;
  for (int q0 = 0; q0 < nb; q0 += kDenseTile) {
    const int tq = min(kDenseTile, nb - q0);
    for (int p0 = 0; p0 < mb; p0 += kDenseTile) {
      const int tp = min(kDenseTile, mb - p0);
      for (int t = tid; t < tp * tq; t += 256) {
        const int p = t / tq, q = t - p * tq;
        tile[p * P + q] = dense[(int64_t)(p0 + p) * ldp + (q0 + q)];
      }
      __syncthreads();
      if (mb <= kDenseTile) {   // (p0 = 0, tp = mb: the tile's columns are one run)
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
        for (int q = wave; q < tq; q += 4) {
          const int run = (q0 + q) * mb + p0;
          T* dst = blk + run;
          walk_block<T>(
              off + run, tp, lane, 64, vec_ok, [&](int e) { dst[e] = tile[e * P + q]; },
              [&](int e) {
                Pack16<T> x;
#pragma unroll
                for (int u = 0; u < Pack16<T>::V; ++u) x.v[u] = tile[(e + u) * P + q];
                *reinterpret_cast<Pack16<T>*>(dst + e) = x;
              });
        }
      }
      __syncthreads();
    }
  }
}

// Every block the index names <- the dense elements at its place; nothing else of the data area is written.  One workgroup per (block row, sub of S).
template <typename T>
__global__ void __launch_bounds__(256) dense_scatter(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                     T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs,
                                                     const int64_t* __restrict__ roff, const int64_t* __restrict__ coff, int nbr, int S, int col_major,
                                                     int vec_ok, const T* __restrict__ dense, int64_t ld) {
  __shared__ T tile[kDenseTile * dense_pitch()];
  const int tid = threadIdx.x;
  const int R = (int)(blockIdx.x / (unsigned)S), sub = (int)(blockIdx.x - (unsigned)R * (unsigned)S);
  if (R >= nbr) return;
  const int m = rs[R];
  const int64_t r0 = roff[R], sr = col_major ? 1 : ld, sc = col_major ? ld : 1;
  for (int b = row_p[R] + sub; b < row_p[R + 1]; b += S) {
    const int Cb = col_i[b], n = cs[Cb];
    const int64_t off = blk_p[b];
    const T* in = dense + r0 * sr + coff[Cb] * sc;
    if (col_major) dense_take_straight<T>(data + off, off, m, n, in, ld, tid, vec_ok);
    else dense_take_transposing<T>(data + off, off, m, n, in, ld, tile, tid, vec_ok);
  }
}

// ---- the count half of dbcsr_create_from_dense -----------------------------------------------------------------------------------------------------------
// One wave per tile (R, C) of the block structure: ||tile||_F^2 in double -- lane l sums the elements l, l + 64, ... of the tile counted along the dense
// side's contiguous direction, the 64 sums go through wave_sum's fixed butterfly: one partial per wave, the same bits on every call.  The filter's rule
// (filter_flags of mm_aux.h) is the DROP: keep = !(norm^2 < eps^2), so a NaN norm stays and eps = 0 keeps every tile.
template <typename T>
__global__ void __launch_bounds__(256) dense_block_norms(const T* __restrict__ dense, int64_t ld, int col_major, const int* __restrict__ rs,
                                                         const int* __restrict__ cs, const int64_t* __restrict__ roff, const int64_t* __restrict__ coff,
                                                         int nbr, int nbc, int64_t ntiles, int64_t n_rows, int64_t n_cols, double eps2,
                                                         int* __restrict__ keep, int* __restrict__ nze) {
  const int lane = threadIdx.x & 63;
  const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (t >= ntiles) return;
  const int R = (int)(t / nbc), Cb = (int)(t - (int64_t)R * nbc);
  const int m = rs[R], n = cs[Cb];
  if (roff[nbr] != n_rows || coff[nbc] != n_cols) {   // the window is not that of the block sizes: nothing of it is read, the host refuses the call
    if (lane == 0) keep[t] = nze[t] = 0;
    return;
  }
  const T* in = dense + (col_major ? roff[R] + coff[Cb] * ld : roff[R] * ld + coff[Cb]);
  const int fast = col_major ? m : n;
  double s = 0.0;
  for (int e = lane; e < m * n; e += 64) {
    const int slow = e / fast;
    s += dense_abs2(in[(int64_t)slow * ld + (e - slow * fast)]);
  }
  s = wave_sum(s);
  if (lane == 0) {
    const int k = !(s < eps2) ? 1 : 0;
    keep[t] = k;
    nze[t] = k ? m * n : 0;
  }
}

// the index of the kept tiles: pos = exclusive scan of keep (pos[ntiles] the total), off = exclusive scan of nze
__global__ void __launch_bounds__(256) dense_emit(const int* __restrict__ keep, const int* __restrict__ pos, const int64_t* __restrict__ off, int nbr, int nbc,
                                                  int64_t ntiles, int* __restrict__ dst_row_p, int* __restrict__ dst_col_i, int64_t* __restrict__ dst_blk_p) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntiles) return;
  const int R = (int)(t / nbc), Cb = (int)(t - (int64_t)R * nbc);
  if (Cb == 0) dst_row_p[R] = pos[t];
  if (t == 0) dst_row_p[nbr] = pos[ntiles];
  if (keep[t]) {
    dst_col_i[pos[t]] = Cb;
    dst_blk_p[pos[t]] = off[t];
  }
}

}  // namespace dbcsr_amd
#endif
