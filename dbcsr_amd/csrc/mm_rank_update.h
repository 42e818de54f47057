// mm_rank_update.h -- rank-k update on the stored pattern, A_IJ <- beta A_IJ + alpha X_I op(Y_J) for every stored block (I, J) and nothing else
// (dbcsr_amd_bcsr_rank_update): the opposite direction of mm_multivec.h, what cp_dbcsr_plus_fm_fm_t with keep_sparsity does.
// Part of the device-resident multiply engine: included by mm_engine.hip after mm_multivec.h, whose scalings (matvec_scaled / _wide / _narrow) it shares.
//
// X is n_x x nrhs, Y is n_y x nrhs, row by row: element (i, v) at i ld + v, so both operands of the product are contiguous along the summed index.
// Dataflow: a wave owns the blocks sub, sub + S, ... of one block row (algebra_rank_update_blocks) and covers each of them in tiles of 16 x 16 elements,
// at most two tiles of one strip of 16 element rows at a time.  One v_mfma_f64_16x16x4_f64 per tile and four summed indices computes the TRANSPOSED tile
// D = Y_tile X_tile^T: its A operand is Y (lane l: row l & 15 of the tile's columns of the block, k slot l >> 4), its B operand X (row l & 15 of the strip,
// k slot l >> 4), so a lane's four results are elements (i, j) = (l & 15, (l >> 4) + 4 reg) of the tile -- for every reg sixteen CONSECUTIVE elements of
// a column of the column-major block per quarter wave.  The sum over nrhs does not care about its order: the lane of k slot g takes the C consecutive
// indices v0 + g C ... v0 + g C + C - 1 of its row (C = 4, complex data 2: 16 / 32 bytes of a row, 16-byte loads where the tensor allows) and feeds them
// to C consecutive MFMAs; X and Y use the same assignment, so no operand passes through LDS.  fp32 data is converted on load (its products are exact in
// double); complex data is four real MFMA chains per tile (re: y_r x_r, y_i (-x_i); im: y_r x_i, y_i x_r), the conjugation of Y a sign on y_i.
// A row outside the block, a row of X / Y at or behind n_x / n_y and an index at or behind nrhs enter as TRUE zeros: they are not loaded (what lies there
// may be Inf, NaN or not mapped).  alpha and beta are applied in double, one rounding to the data's type per element; every element has one owner: no
// atomics, the same bits on every call.  Every write stays inside the blocks the index names.
#ifndef DBCSR_AMD_MM_RANK_UPDATE_H
#define DBCSR_AMD_MM_RANK_UPDATE_H
#include "mm_algebra.h"

namespace dbcsr_amd {

typedef double rank_update_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kRankUpdateTile = 16;    // the MFMA's tile: element rows of a strip, element columns of a tile
constexpr int kRankUpdateTiles = 2;    // tiles of one strip a wave holds accumulators for
template <typename T> struct RankUpdateRun { static constexpr int C = 4; };     // consecutive summed indices a lane loads per step: a step covers 4 C
template <> struct RankUpdateRun<z64> { static constexpr int C = 2; };

// C entries v ... v + C - 1 of one row of X / Y as doubles (re, im); zeros -- without a load -- when the row is not there (!ok) or the index is at or
// behind nrhs.  vec: the row starts on a 16-byte boundary (v is a multiple of C, C elements are a multiple of 16 bytes)
template <typename T, int C>
__device__ __forceinline__ void rank_update_run(const T* __restrict__ row, bool ok, int v, int nrhs, int vec, double (&re)[C], double (&im)[C]) {
  constexpr int V = Pack16<T>::V;
#pragma unroll
  for (int u = 0; u < C; ++u) re[u] = im[u] = 0.0;
  if (!ok || v >= nrhs) return;
  if (vec && v + C <= nrhs) {
    const Pack16<T>* p = reinterpret_cast<const Pack16<T>*>(row + v);
#pragma unroll
    for (int q = 0; q < C / V; ++q) {
      const Pack16<T> a = p[q];
#pragma unroll
      for (int u = 0; u < V; ++u) re[q * V + u] = re_of(a.v[u]), im[q * V + u] = im_of(a.v[u]);
    }
  } else {
#pragma unroll
    for (int u = 0; u < C; ++u)
      if (v + u < nrhs) {
        const T a = row[v + u];
        re[u] = re_of(a), im[u] = im_of(a);
      }
  }
}

// NT tiles (element columns j0 + 16 t ... of the block) of the strip of element rows i0 ... i0 + 15 of one m x n block at `blk`
template <typename T, int NT>
__device__ __forceinline__ void rank_update_tiles(T* __restrict__ blk, int m, int n, int i0, int j0, const T* __restrict__ x, int64_t xrow, int64_t n_x,
                                                  int64_t ldx, int xvec, const T* __restrict__ y, int64_t yrow, int64_t n_y, int64_t ldy, int yvec, int nrhs,
                                                  int conj, typename MatvecAcc<T>::type alpha, typename MatvecAcc<T>::type beta, int beta_zero, int lane) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr int C = RankUpdateRun<T>::C;
  constexpr bool Z = sizeof(T) == 16;
  const int q = lane & 15, g = lane >> 4;
  const bool xok = i0 + q < m && xrow + i0 + q < n_x;
  const T* __restrict__ xr = x + (xok ? (xrow + i0 + q) * ldx : 0);
  bool yok[NT];
  const T* __restrict__ yr[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = j0 + kRankUpdateTile * t + q;
    yok[t] = j < n && yrow + j < n_y;
    yr[t] = y + (yok[t] ? (yrow + j) * ldy : 0);
  }
  rank_update_f64x4 acc_re[NT], acc_im[Z ? NT : 1];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc_re[t] = rank_update_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < (Z ? NT : 1); ++t) acc_im[t] = rank_update_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int v0 = 0; v0 < nrhs; v0 += 4 * C) {
    const int v = v0 + g * C;
    double xre[C], xim[C], yre[NT][C], yim[NT][C];
    rank_update_run<T, C>(xr, xok, v, nrhs, xvec, xre, xim);
#pragma unroll
    for (int t = 0; t < NT; ++t) rank_update_run<T, C>(yr[t], yok[t], v, nrhs, yvec, yre[t], yim[t]);
#pragma unroll
    for (int u = 0; u < C; ++u) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc_re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(yre[t][u], xre[u], acc_re[t], 0, 0, 0);
        if (Z) {
          const double yi = conj ? -yim[t][u] : yim[t][u];   // (the conjugation of Y is a sign)
          acc_re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(yi, -xim[u], acc_re[t], 0, 0, 0);
          acc_im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(yre[t][u], xim[u], acc_im[t], 0, 0, 0);
          acc_im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(yi, xre[u], acc_im[t], 0, 0, 0);
        }
      }
    }
  }
  // the lane's results: element row i0 + q, element columns j0 + 16 t + g + 4 r.  An element whose row of X or of Y is not there is not written.
  if (!xok) return;
  const int i = i0 + q;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + kRankUpdateTile * t + g + 4 * r;
      if (j < n && yrow + j < n_y) {
        T* __restrict__ out = blk + (int64_t)j * m + i;
        Acc s;
        if constexpr (Z) s = z64(acc_re[t][r], acc_im[t][r]);
        else s = acc_re[t][r];
        Acc res = alpha * s;
        if (!beta_zero) res = res + beta * matvec_wide(*out);
        *out = matvec_narrow<T>(res);
      }
    }
  }
}

// A_IJ <- beta A_IJ + alpha X_I op(Y_J) for the blocks sub, sub + S, ... of block row `row`: wave (row S + sub).  xoff / yoff: the first full row of
// every block row / block column.  beta_zero: A's values are not read.
template <typename T>
__global__ void __launch_bounds__(256)
algebra_rank_update_blocks(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, T* __restrict__ data,
                           const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ xoff, const int64_t* __restrict__ yoff, int nbr,
                           int S, int conj, int beta_zero, const T* __restrict__ x, int64_t n_x, int64_t ldx, int xvec, const T* __restrict__ y, int64_t n_y,
                           int64_t ldy, int yvec, int nrhs, typename MatvecAcc<T>::type alpha, typename MatvecAcc<T>::type beta) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0) return;
  const int64_t xrow = xoff[row];
  if (xrow >= n_x) return;   // (no row of X for this block row: nothing of it is written)
  const int b1 = row_p[row + 1];
  for (int b = row_p[row] + sub; b < b1; b += S) {
    const int c = col_i[b];
    const int n = cs[c];
    const int64_t yrow = yoff[c];
    T* __restrict__ blk = data + blk_p[b];
    for (int i0 = 0; i0 < m; i0 += kRankUpdateTile) {
      for (int j0 = 0; j0 < n; j0 += kRankUpdateTiles * kRankUpdateTile) {
        if (n - j0 > kRankUpdateTile)   // (wave-uniform)
          rank_update_tiles<T, 2>(blk, m, n, i0, j0, x, xrow, n_x, ldx, xvec, y, yrow, n_y, ldy, yvec, nrhs, conj, alpha, beta, beta_zero, lane);
        else
          rank_update_tiles<T, 1>(blk, m, n, i0, j0, x, xrow, n_x, ldx, xvec, y, yrow, n_y, ldy, yvec, nrhs, conj, alpha, beta, beta_zero, lane);
      }
    }
  }
}

// alpha == 0 or nrhs == 0: A_IJ <- beta A_IJ in the data's own precision (matvec_scaled; zeros for beta == 0 without reading A), block by block of the
// index, for the elements the update itself would write: wave (row S + sub), a lane per element.  X and Y are not read.
template <typename T>
__global__ void __launch_bounds__(256)
algebra_rank_update_scale(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, T* __restrict__ data,
                          const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ xoff, const int64_t* __restrict__ yoff, int nbr,
                          int S, int beta_zero, int64_t n_x, int64_t n_y, T beta) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0) return;
  const int64_t xrow = xoff[row];
  const int b1 = row_p[row + 1];
  for (int b = row_p[row] + sub; b < b1; b += S) {
    const int c = col_i[b];
    const int ne = m * cs[c];
    const int64_t yrow = yoff[c];
    T* __restrict__ blk = data + blk_p[b];
    for (int e = lane; e < ne; e += 64) {
      const int j = e / m, i = e - j * m;
      if (xrow + i < n_x && yrow + j < n_y) blk[e] = beta_zero ? T(0) : matvec_scaled(beta, blk[e]);
    }
  }
}

}  // namespace dbcsr_amd
#endif
