// mm_spmm.h -- block-sparse matrix times a dense matrix on the MFMA, Y <- alpha op(A) X + beta Y (dbcsr_amd_bcsr_multiply_dense): the forward direction
// of mm_rank_update.h, what cp_dbcsr_sm_fm_multiply does (H C and S C of an SCF step), for dense operands with hundreds of columns.
// Part of the device-resident multiply engine: included by mm_engine.hip after mm_rank_update.h, whose MFMA lane assignment, runs (RankUpdateRun) and
// accumulator type it shares, with the passes (matvec_passes) and scalings (matvec_scaled / _wide / _narrow) of mm_algebra.h.
//
// X is n_x x ncol, Y is n_y x ncol, both ROW BY ROW (layout 0: element (i, v) at i ld + v) or both COLUMN BY COLUMN (layout 1: at i + v ld, a Fortran
// full matrix).  Dataflow: one workgroup of four waves owns block row I of op(A) and 64 columns of Y, wave w the 16 columns 64 t + 16 w ... of them and
// ALL element rows of the block row: 64 rows at a time (four strips of 16 rows, one f64x4 accumulator each; complex data two), a taller block row in
// chunks of 64.  The walk is fixed: first the stored blocks (I, J) of row I (the row pass of matvec_passes), then the entries of block column I's list
// (the column pass: the block is read transposed), both into the same registers.  A block -- or a piece of it that fits 24 KB -- is copied ONCE into the
// LDS by all 256 threads (walk_block_values: aligned 16-byte loads where the data area allows) exactly as it lies in memory: element (i, k) of the
// operand of a row-pass piece is at k pitch + i, of a column-pass piece at i pitch + k, so neither pass transposes on the way in.  X goes from global
// memory straight into the MFMA operand.  One v_mfma_f64_16x16x4_f64 multiplies a strip by four summed indices: the lane l holds row / column l & 15
// of its operand and the k slot l >> 4, its four results are D[(l >> 4) + 4 r][l & 15].  As in the rank update the order of the summed index is free:
// the lane of k slot g takes the C consecutive indices k0 + g C ... (C = 4, complex data 2) and feeds them to C consecutive MFMAs, the block and X
// alike.  Layout 0: the block is the A operand, X the B operand -- a quarter wave loads 16 consecutive columns of one row of X and stores 16 consecutive
// columns of one row of Y.  Layout 1: X^T is the A operand, the block's transpose the B operand (the tile is computed transposed) -- a lane loads C
// consecutive rows of one column of X (16-byte loads where the address allows), a quarter wave stores 16 consecutive rows of one column of Y.
// fp32 data is converted on load (its products are exact in double); complex data is four real chains per strip; conjugation and sign of a pass are
// applied when the block's operand is formed (sign flips: exact).  A row or column outside the block or the piece, a row of X at or behind n_x and a
// column at or behind ncol enter as TRUE zeros: they are not loaded.  alpha and beta are applied in double in the epilogue, one rounding per element;
// a block row whose walk met no block gets beta y, formed in double like every other row (+0 for beta == 0).  Every element of the window has one owner and is
// written once: no atomics, no partial matrices, the same bits on every call; a column's bits depend neither on its position nor on its company.
#ifndef DBCSR_AMD_MM_SPMM_H
#define DBCSR_AMD_MM_SPMM_H
#include <type_traits>
#include "mm_rank_update.h"

namespace dbcsr_amd {

constexpr int kSpmmTile = 16;                            // columns of Y per wave: the MFMA's tile
constexpr int kSpmmWaves = 4;                            // waves of a workgroup: they share the staged block
constexpr int kSpmmCols = kSpmmTile * kSpmmWaves;        // columns of Y per workgroup
constexpr int kSpmmStrips = 4;                           // strips of 16 element rows a wave holds accumulators for
constexpr int kSpmmRows = kSpmmStrips * kSpmmTile;       // element rows of a chunk
constexpr int kSpmmStageBytes = 24576;                   // LDS of a workgroup: the staged piece
constexpr int kSpmmRowsOn = 1, kSpmmSkipDiag = 2, kSpmmConj = 4, kSpmmNegate = 8;   // a pass of matvec_passes as bits
static_assert(kSpmmStageBytes <= 32768, "at most 32 KB of LDS per workgroup");
static_assert(kSpmmStageBytes / 16 >= kSpmmRows, "a piece holds at least one column of a chunk of any data type");

// `len` elements at d (element `off` of a 16-byte aligned area) -> lds[0 ... len), by the 256 threads: aligned 16-byte loads where vec_ok
template <typename T>
__device__ __forceinline__ void spmm_stage(const T* __restrict__ d, int64_t off, int len, int tid, int vec_ok, T* lds) {
  walk_block_values(d, off, len, tid, 256, vec_ok, [&](int e, T v) { lds[e] = v; });
}

// `count` runs of `h` elements, `step` elements apart, from d on -> lds[run h + i]: a part of a block that is not one piece of memory
template <typename T>
__device__ __forceinline__ void spmm_stage_runs(const T* __restrict__ d, int step, int h, int count, int tid, T* lds) {
  const int len = count * h;
  for (int e = tid; e < len; e += 256) {
    const int run = e / h;
    lds[e] = d[(int64_t)run * step + (e - run * h)];
  }
}

// The C entries of X this lane feeds to the next C MFMAs: rows row ... row + C - 1 of column col, as doubles (re, im).  An entry at or behind `cnt` (the
// rows the piece and n_x leave) and an entry of a column that is not there (!colok) is a TRUE zero: nothing of it is loaded -- the lane reads element
// (0, 0) of X in its place, which exists whenever a product is formed, and drops it.  No branch in layout 0; in layout 1 one, for the 16-byte loads.
template <typename T, int C, int LAYOUT>
__device__ __forceinline__ void spmm_x_run(const T* __restrict__ x, int64_t row, int cnt, int64_t col, bool colok, int64_t ld, double (&re)[C],
                                           double (&im)[C]) {
  constexpr int V = Pack16<T>::V;
  if (!colok) cnt = 0;
  const int64_t first = LAYOUT == 0 ? row * ld + col : col * ld + row, step = LAYOUT == 0 ? ld : 1;
  if constexpr (LAYOUT == 1 && V > 1) {
    if (cnt >= C && (reinterpret_cast<uintptr_t>(x + first) & 15u) == 0) {
#pragma unroll
      for (int w = 0; w < C / V; ++w) {
        const Pack16<T> a = reinterpret_cast<const Pack16<T>*>(x + first)[w];
#pragma unroll
        for (int u = 0; u < V; ++u) re[w * V + u] = re_of(a.v[u]), im[w * V + u] = im_of(a.v[u]);
      }
      return;
    }
  }
#pragma unroll
  for (int u = 0; u < C; ++u) {
    const bool ok = u < cnt;
    const T a = x[ok ? first + u * step : 0];
    re[u] = ok ? re_of(a) : 0.0, im[u] = ok ? im_of(a) : 0.0;
  }
}

// The products of one staged piece: acc += op(piece) X[xrow0 ... xrow0 + kc).  Element (i, k) of the piece' operand is lds[k pitch + i] (row pass) or
// lds[i pitch + k] (COLPASS: the block is read transposed), i below mrv (the element rows of the chunk this piece has), k below kc; NS strips of 16
// rows are at work.  An element outside the piece is a true zero: the lane reads lds[0] in its place and drops it.  The loop has no branch.
template <typename T, int LAYOUT, bool COLPASS, int NS>
__device__ __forceinline__ void spmm_piece(const T* lds, int pitch, int mrv, int kc, const T* __restrict__ x, int64_t xrow0, int64_t n_x, int64_t ldx,
                                           int col0, int ncol, int conj, int negate, int lane, rank_update_f64x4 (&acc_re)[NS],
                                           rank_update_f64x4 (&acc_im)[NS]) {
  constexpr int C = RankUpdateRun<T>::C;
  constexpr bool Z = sizeof(T) == 16;
  const int q = lane & 15, g = lane >> 4;
  const bool colok = col0 + q < ncol;
  const int64_t left = n_x - xrow0;   // (a term whose row of X lies at n_x or behind is not formed)
  const int kcx = left < kc ? (left > 0 ? (int)left : 0) : kc;
  for (int kb = 0; kb < kcx; kb += 4 * C) {
    const int k = kb + g * C;
    double xre[C], xim[C];
    spmm_x_run<T, C, LAYOUT>(x, xrow0 + k, kcx - k, col0 + q, colok, ldx, xre, xim);
    const int at = COLPASS ? q * pitch + k : k * pitch + q;
#pragma unroll
    for (int u = 0; u < C; ++u) {
      const bool kok = k + u < kcx;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const bool ok = kok && kSpmmTile * s + q < mrv;
        const T a = lds[ok ? at + (COLPASS ? kSpmmTile * s * pitch + u : u * pitch + kSpmmTile * s) : 0];
        double are = ok ? re_of(a) : 0.0, aim = ok ? im_of(a) : 0.0;
        if (Z && conj) aim = -aim;
        if (negate) are = -are, aim = -aim;
        if constexpr (LAYOUT == 0) {
          acc_re[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, xre[u], acc_re[s], 0, 0, 0);
          if (Z) {
            acc_re[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, -xim[u], acc_re[s], 0, 0, 0);
            acc_im[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(are, xim[u], acc_im[s], 0, 0, 0);
            acc_im[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(aim, xre[u], acc_im[s], 0, 0, 0);
          }
        } else {
          acc_re[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xre[u], are, acc_re[s], 0, 0, 0);
          if (Z) {
            acc_re[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xim[u], aim, acc_re[s], 0, 0, 0);
            acc_im[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xim[u], are, acc_im[s], 0, 0, 0);
            acc_im[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xre[u], aim, acc_im[s], 0, 0, 0);
          }
        }
      }
    }
  }
}

// f(NS) for the NS = 1 ... 4 strips a chunk of mr rows needs (workgroup-uniform)
template <typename F>
__device__ __forceinline__ void spmm_by_strips(int ns, F&& f) {
  switch (ns) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{});
  }
}

// Y[yoff(I) + i][v] <- alpha (sum over the walk of block row I of op(A)) + beta Y[...] for every element row i of block row I and the 64 columns of
// tile group blockIdx.x % G: workgroup blockIdx.x = I G + tile group.  rows / cols: the two passes as bits (kSpmmRowsOn: the pass is on).  With the row
// pass on I is a block row of A (lengths rs, offsets roff), otherwise a block column (cs, coff); a stored triangle has both and a square structure.
template <typename T, int LAYOUT>
__global__ void __launch_bounds__(256, 4)   // (four waves per SIMD: 128 registers)
spmm_product(const int* __restrict__ row_p, const int* __restrict__ col_i, const int* __restrict__ col_p, const int* __restrict__ list,
             const int64_t* __restrict__ blk_p, const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs,
             const int64_t* __restrict__ roff, const int64_t* __restrict__ coff, int nb, int G, int rows, int cols, int vec_ok, const T* __restrict__ x,
             int64_t n_x, int64_t ldx, T* __restrict__ y, int64_t n_y, int64_t ldy, int ncol, typename MatvecAcc<T>::type alpha,
             typename MatvecAcc<T>::type beta, int beta_zero) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr bool Z = sizeof(T) == 16;
  constexpr int cap = kSpmmStageBytes / (int)sizeof(T);
  __shared__ __align__(16) unsigned char spmm_lds[kSpmmStageBytes];
  T* as = reinterpret_cast<T*>(spmm_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 15, g = lane >> 4;
  const int I = (int)(blockIdx.x / G);
  if (I >= nb) return;   // (the whole workgroup, as every return in front of the walk)
  const bool rows_on = (rows & kSpmmRowsOn) != 0, cols_on = (cols & kSpmmRowsOn) != 0;
  const int m = rows_on ? rs[I] : cs[I];
  const int64_t base = rows_on ? roff[I] : coff[I];
  if (m <= 0 || base >= n_y) return;
  const int col0 = ((int)(blockIdx.x % G) * kSpmmWaves + wave) * kSpmmTile;
  const bool live = col0 < ncol;   // (a wave without columns still stages, and reaches every barrier)
  for (int r0 = 0; r0 < m; r0 += kSpmmRows) {
    const int mr = m - r0 < kSpmmRows ? m - r0 : kSpmmRows;
    auto chunk = [&](auto strips) {   // (the whole chunk per count of strips: the accumulators never cross a branch between the forms)
    constexpr int NS = decltype(strips)::value;
    rank_update_f64x4 acc_re[NS], acc_im[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc_re[s] = acc_im[s] = rank_update_f64x4{0.0, 0.0, 0.0, 0.0};
    int nterms = 0;   // blocks the walk met (workgroup-uniform)
    if (rows_on) {
      const int b1 = row_p[I + 1], cols_per = cap / mr;
      for (int b = row_p[I]; b < b1; ++b) {
        const int c = col_i[b];
        if ((rows & kSpmmSkipDiag) && c == I) continue;
        const int n = cs[c];
        if (n <= 0) continue;
        ++nterms;
        const int64_t off = blk_p[b], xb = coff[c];
        for (int ja = 0; ja < n; ja += cols_per) {
          const int kc = n - ja < cols_per ? n - ja : cols_per;
          if (m <= kSpmmRows) spmm_stage(data + off + (int64_t)ja * m, off + (int64_t)ja * m, kc * m, tid, vec_ok, as);   // whole columns: one piece of memory
          else spmm_stage_runs(data + off + (int64_t)ja * m + r0, m, mr, kc, tid, as);                                     // the chunk's rows of every column
          __syncthreads();
          if (live)
            spmm_piece<T, LAYOUT, false, NS>(as, mr, mr, kc, x, xb + ja, n_x, ldx, col0, ncol, rows & kSpmmConj, rows & kSpmmNegate, lane, acc_re, acc_im);
          __syncthreads();   // (the next piece overwrites the LDS)
        }
      }
    }
    const int left = cols_on ? cs[I] - r0 : 0, nj = left < mr ? (left > 0 ? left : 0) : mr;   // (the owner's rows are the block's columns)
    if (nj > 0) {
      const int t1 = col_p[I + 1];
      for (int t = col_p[I]; t < t1; ++t) {
        const int r = list[2 * (size_t)t + 1];
        if ((cols & kSpmmSkipDiag) && r == I) continue;
        const int mk = rs[r];
        if (mk <= 0) continue;
        ++nterms;
        const int64_t off = blk_p[list[2 * (size_t)t]] + (int64_t)r0 * mk, xb = roff[r];
        const int rows_per = nj * mk <= cap ? mk : cap / nj;   // the whole part, or as many rows of its nj columns as a piece holds
        for (int ia = 0; ia < mk; ia += rows_per) {
          const int h = mk - ia < rows_per ? mk - ia : rows_per;
          if (h == mk) spmm_stage(data + off, off, nj * mk, tid, vec_ok, as);
          else spmm_stage_runs(data + off + ia, mk, h, nj, tid, as);
          __syncthreads();
          if (live)
            spmm_piece<T, LAYOUT, true, NS>(as, h, nj, h, x, xb + ia, n_x, ldx, col0, ncol, cols & kSpmmConj, cols & kSpmmNegate, lane, acc_re, acc_im);
          __syncthreads();
        }
      }
    }
    if (!live) return;   // (the chunk; every barrier of it is behind)
    // the lane's results, D[g + 4 r][q] of every strip: layout 0 (row 16 s + g + 4 r, column q), layout 1 (row 16 s + q, column g + 4 r)
    int gw = g, qw = q;
    asm volatile("" : "+v"(gw), "+v"(qw));   // (keeps the sixteen addresses of the write-out from being formed, and held, in front of the walk)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = kSpmmTile * s + (LAYOUT == 0 ? gw + 4 * r : qw), v = col0 + (LAYOUT == 0 ? qw : gw + 4 * r);
        const int64_t row = base + r0 + i;
        if (i < mr && row < n_y && v < ncol) {
          T* __restrict__ out = y + (LAYOUT == 0 ? row * ldy + v : (int64_t)v * ldy + row);
          if (nterms == 0) {   // nothing stored for this block row: beta y in double, one rounding to the data's type; +0 for beta == 0.  (For
                               // float64 and complex128 that IS the data's own precision, every operation rounded on its own: matvec_scaled.)
            *out = beta_zero ? T(0) : matvec_narrow<T>(matvec_scaled(beta, matvec_wide(*out)));
          } else {
            Acc sum;
            if constexpr (Z) sum = z64(acc_re[s][r], acc_im[s][r]);
            else sum = acc_re[s][r];
            Acc res = alpha * sum;
            if (!beta_zero) res = res + beta * matvec_wide(*out);
            *out = matvec_narrow<T>(res);
          }
        }
      }
    }
    };
    spmm_by_strips((mr + kSpmmTile - 1) / kSpmmTile, chunk);
  }
}

// The modes without a product (kMatvecNoProduct: alpha == 0 or an empty matrix): Y[i][v] <- beta Y[i][v] in the data's own precision, zeros for beta == 0
// without reading Y, for i below n_y and below *total (the full rows of op(A), on the device) and v below ncol.  A and X are not read.  A thread per
// element, consecutive threads along the contiguous direction of the layout.
template <typename T>
__global__ void __launch_bounds__(256)
spmm_scale(T* __restrict__ y, int64_t n_y, int ncol, int64_t ldy, int layout, const int64_t* __restrict__ total, T beta, int beta_zero) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = n_y < *total ? n_y : *total;
  if (n <= 0) return;
  int64_t i, v;
  if (layout == 0) i = t / ncol, v = t - i * ncol;
  else v = t / n, i = t - v * n;
  if (i >= n || v >= ncol) return;
  T* __restrict__ out = y + (layout == 0 ? i * ldy + v : v * ldy + i);
  *out = beta_zero ? T(0) : matvec_scaled(beta, *out);
}

}  // namespace dbcsr_amd
#endif
