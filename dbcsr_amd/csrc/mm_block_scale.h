// mm_block_scale.h -- a block diagonal applied to a matrix in place (dbcsr_amd_bcsr_block_diag_multiply): A_IJ <- alpha op(D_I) A_IJ (block_scale_left)
// or A_IJ <- alpha A_IJ op(D_J) (block_scale_right) for every stored block (I, J) of A and nothing else, D_I the diagonal block (I, I) that `diag` stores:
// D^-1 A of a block-Jacobi preconditioner, X0 S of a Hotelling / Newton-Schulz inverse, and -- as two passes -- a block congruence D A D^T.  Part of the
// device-resident multiply engine: included by mm_engine.hip after mm_block_inverse.h.
//
// The update is in place, so the unit of ownership is a STRIP of a block: 16 consecutive element columns for left (a result element (i, j) reads the whole
// column j of its block), 16 consecutive element rows for right (it reads the whole row i).  A wave owns the blocks sub, sub + S, ... of one block row and
// takes their strips one after the other; for a strip it holds accumulators for ALL ceil(d / 16) <= 6 tiles along the diagonal block's dimension d, and
// the sum over d runs in steps of 4 with one v_mfma_f64_16x16x4_f64 per tile and step (the core of mm_rank_update.h).  Every load of the strip has been
// fed to the accumulators before the first store: the stores depend on the accumulators, the accumulators on every load -- a data dependence, not a
// promise about aliasing (the block pointer carries no __restrict__).  No two waves share a strip.
// The tile is computed TRANSPOSED, Dout[jj][ii] = sum_k P[jj][k] Q[k][ii], so that a lane's four results are elements (i, j) = (q, g + 4 reg) of the tile
// (q = lane & 15, g = lane >> 4): for every reg sixteen consecutive elements of a column of the column-major block per quarter wave.
//   left:   P = the strip's A^T (lane: A(k0 + g, j0 + q), one load per step for all tiles),   Q = op(D)^T of tile t (lane: op(D)(16 t + q, k0 + g))
//   right:  P = op(D)^T of tile t (lane: op(D)(k0 + g, 16 t + q)),                          Q = the strip's A^T (lane: A(i0 + q, k0 + g), one load per step)
// op = T is an index swap on the loads of D, the conjugation of D a sign on its imaginary part; complex data is four real MFMA chains per tile.  D comes
// straight from global memory: it is shared by a whole block row (left) or block column (right) and stays in L2.  Rows, columns and summed indices outside
// the block enter as TRUE zeros without a load.  fp32 data is converted on load; alpha is applied in double, one rounding to the data's type per element;
// every element has one owner: no atomics, the same bits on every call.  A block whose D is not stored becomes +0.0 without being read (the zero block of
// a multiply with beta = 0); block_scale_zero does that to every block for alpha == 0.  Every write stays inside the blocks the index names.
#ifndef DBCSR_AMD_MM_BLOCK_SCALE_H
#define DBCSR_AMD_MM_BLOCK_SCALE_H
#include "mm_rank_update.h"

namespace dbcsr_amd {

constexpr int kBlockScaleTile = 16;     // the MFMA's tile; the width of a strip
constexpr int kBlockScaleMaxTiles = 6;  // accumulator tiles of a strip: diagonal blocks of up to 96 (what can be inverted can be applied)
constexpr int kBlockScaleMaxDim = kBlockScaleTile * kBlockScaleMaxTiles;

// element (r, c) of op(D) as doubles, D a d x d column-major block; a true zero outside the block: the lane then loads element 0 of the block -- an
// address that is there -- and drops what it got, so the loads of a step carry no branch and go out together
template <typename T>
__device__ __forceinline__ void block_scale_d(const T* __restrict__ D, int d, int r, int c, int tr, int conj, double& re, double& im) {
  const bool ok = r < d && c < d;
  const T x = D[(unsigned)(ok ? (tr ? r * d + c : c * d + r) : 0)];   // (32-bit offsets from a wave-uniform base: d <= 96)
  re = ok ? re_of(x) : 0.0;
  im = ok ? (conj ? -im_of(x) : im_of(x)) : 0.0;
}

// One strip of the m x n column-major block at blk against the d x d block D, nt = ceil(d / 16) <= NT tiles.  LEFT: d == m, the strip is the element
// columns s0 ... s0 + 15; otherwise d == n and it is the element rows s0 ... s0 + 15.  One accumulator set for every d: the tiles at and behind nt are
// skipped by a wave-uniform branch around their MFMAs and stores (their loads of D are off in every lane as it is).  A switch over bodies of 1 ... 6 tiles
// would keep all six accumulator sets alive across it.
template <typename T, bool LEFT>
__device__ __forceinline__ void block_scale_strip(T* blk, int m, int n, int s0, const T* __restrict__ D, int d, int nt, int tr, int conj,
                                                  typename MatvecAcc<T>::type alpha, int lane) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr bool Z = sizeof(T) == 16;
  constexpr int NT = kBlockScaleMaxTiles;
  const int q = lane & 15, g = lane >> 4;
  const int s = s0 + q;                          // the lane's column (left) / row (right) of the strip, as an operand
  const bool sok = s < (LEFT ? n : m);
  rank_update_f64x4 acc_re[NT], acc_im[Z ? NT : 1];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc_re[t] = rank_update_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < (Z ? NT : 1); ++t) acc_im[t] = rank_update_f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < d; k0 += 4) {
    const int k = k0 + g;
    const bool aok = sok && k < d;
    const T a = blk[(unsigned)(aok ? (LEFT ? s * m + k : k * m + s) : 0)];   // (inside the block: below m n, an int as everywhere; 0: see block_scale_d)
    const double ar = aok ? re_of(a) : 0.0, ai = aok ? im_of(a) : 0.0;
    double dr[NT], di[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int e = kBlockScaleTile * t + q;
      if constexpr (LEFT) block_scale_d<T>(D, d, e, k, tr, conj, dr[t], di[t]);
      else block_scale_d<T>(D, d, k, e, tr, conj, dr[t], di[t]);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t >= nt) break;   // (wave-uniform)
      // Dout = P Q: left P = A^T, Q = op(D)^T; right P = op(D)^T, Q = A^T
      const double pr = LEFT ? ar : dr[t], pi = LEFT ? ai : di[t], qr = LEFT ? dr[t] : ar, qi = LEFT ? di[t] : ai;
      acc_re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr, qr, acc_re[t], 0, 0, 0);
      if constexpr (Z) {
        acc_re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pi, -qi, acc_re[t], 0, 0, 0);
        acc_im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr, qi, acc_im[t], 0, 0, 0);
        acc_im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pi, qr, acc_im[t], 0, 0, 0);
      }
    }
  }
  // the lane's results.  left: element rows 16 t + q, element columns s0 + g + 4 r; right: element rows s0 + q, element columns 16 t + g + 4 r
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= nt) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = LEFT ? kBlockScaleTile * t + q : s0 + q;
      const int j = LEFT ? s0 + g + 4 * r : kBlockScaleTile * t + g + 4 * r;
      if (i < m && j < n) {
        Acc sum;
        if constexpr (Z) sum = z64(acc_re[t][r], acc_im[t][r]);
        else sum = acc_re[t][r];
        blk[(unsigned)(j * m + i)] = matvec_narrow<T>(alpha * sum);
      }
    }
  }
}

// every strip of one block; d <= kBlockScaleMaxDim (the caller looked)
template <typename T, bool LEFT>
__device__ __forceinline__ void block_scale_block(T* blk, int m, int n, const T* __restrict__ D, int d, int tr, int conj,
                                                  typename MatvecAcc<T>::type alpha, int lane) {
  const int len = LEFT ? n : m, nt = (d + kBlockScaleTile - 1) / kBlockScaleTile;   // (wave-uniform)
  for (int s0 = 0; s0 < len; s0 += kBlockScaleTile) {
    block_scale_strip<T, LEFT>(blk, m, n, s0, D, d, nt, tr, conj, alpha, lane);
  }
}

// +0.0 to every element of one block, a lane per element; nothing is read
template <typename T>
__device__ __forceinline__ void block_scale_clear(T* blk, int ne, int lane) {
  for (int e = lane; e < ne; e += 64) blk[e] = T(0);
}

// A_IJ <- alpha op(D_I) A_IJ for the blocks sub, sub + S, ... of block row `row`: wave (row S + sub).  D_I is looked up once per block row; without it
// the blocks become +0.0 unread.  A block row whose dimension exceeds kBlockScaleMaxDim is left alone (the entry refuses such a max_dim).
template <typename T>
__global__ void __launch_bounds__(256, 2)
block_scale_left(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, T* data, const int* __restrict__ rs,
                 const int* __restrict__ cs, const int* __restrict__ d_row_p, const int* __restrict__ d_col_i, const int64_t* __restrict__ d_blk_p,
                 const T* __restrict__ d_data, int nbr, int S, int tr, int conj, typename MatvecAcc<T>::type alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (in scalar registers, and all that follows from it)
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0 || m > kBlockScaleMaxDim) return;
  const int b0 = row_p[row] + sub, b1 = row_p[row + 1];
  if (b0 >= b1) return;
  const int at = __builtin_amdgcn_readfirstlane(find_diag_block(d_row_p, d_col_i, row, lane));
  const T* __restrict__ D = d_data + (at >= 0 ? d_blk_p[at] : 0);
  for (int b = b0; b < b1; b += S) {
    const int n = cs[col_i[b]];
    T* blk = data + blk_p[b];
    if (at < 0) block_scale_clear<T>(blk, m * n, lane);
    else block_scale_block<T, true>(blk, m, n, D, m, tr, conj, alpha, lane);
  }
}

// A_IJ <- alpha A_IJ op(D_J), the same walk; D_J is looked up once per block, through col_i.
template <typename T>
__global__ void __launch_bounds__(256, 2)
block_scale_right(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, T* data, const int* __restrict__ rs,
                  const int* __restrict__ cs, const int* __restrict__ d_row_p, const int* __restrict__ d_col_i, const int64_t* __restrict__ d_blk_p,
                  const T* __restrict__ d_data, int nbr, int S, int tr, int conj, typename MatvecAcc<T>::type alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (in scalar registers, and all that follows from it)
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0) return;
  const int b1 = row_p[row + 1];
  for (int b = row_p[row] + sub; b < b1; b += S) {
    const int c = col_i[b];
    const int n = cs[c];
    if (n <= 0 || n > kBlockScaleMaxDim) continue;
    T* blk = data + blk_p[b];
    const int at = __builtin_amdgcn_readfirstlane(find_diag_block(d_row_p, d_col_i, c, lane));
    if (at < 0) block_scale_clear<T>(blk, m * n, lane);
    else block_scale_block<T, false>(blk, m, n, d_data + d_blk_p[at], n, tr, conj, alpha, lane);
  }
}

// alpha == 0: every element of every stored block <- +0.0, a lane per element; neither operand's data is read
template <typename T>
__global__ void __launch_bounds__(256)
block_scale_zero(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, T* data, const int* __restrict__ rs,
                 const int* __restrict__ cs, int nbr, int S) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (in scalar registers, and all that follows from it)
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0) return;
  const int b1 = row_p[row + 1];
  for (int b = row_p[row] + sub; b < b1; b += S) block_scale_clear<T>(data + blk_p[b], m * cs[col_i[b]], lane);
}

}  // namespace dbcsr_amd
#endif
