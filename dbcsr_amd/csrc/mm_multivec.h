// mm_multivec.h -- block-sparse matrix times several dense vectors, Y <- alpha op(A) X + beta Y (dbcsr_amd_bcsr_multivec): the matrix-vector product
// of mm_algebra.h with nrhs right-hand sides handled together, so that A is read once and every element of it is used nrhs times.
// Part of the device-resident multiply engine: included by mm_engine.hip after mm_algebra.h, whose passes (matvec_passes), terms (matvec_term, MatvecAcc)
// and scalings (matvec_scaled / _wide / _narrow / _signed) it shares.
//
// X is n_x x nrhs, Y is n_y x nrhs, row by row: element (i, v) at i ld + v, so the nrhs entries one element of A meets are consecutive in memory.
// Dataflow: a workgroup of W <= 4 waves owns one block row (algebra_multivec_rows) or one block column (algebra_multivec_cols, over the per-column lists)
// and W tiles of 16 right-hand sides, one tile per wave.  Lane 16 g + v holds column v of its tile and every fourth row (column pass: column) of the
// block in 16 register accumulators: 64 rows at a time, a taller block row in chunks of 64.  A piece of the block -- whole element columns -- is loaded
// by ALL waves of the workgroup (walk_block of mm_block_walk.h over the workgroup's threads: aligned 16-byte loads where the data area allows) into the
// workgroup's LDS, ONCE for its W tiles; each wave stages the
// X rows of its own tile that the piece meets (one coalesced 16-entry read per row), and after a barrier multiplies: per element column j one LDS read
// of x and one per owned row of a_ij.  W = 1 (nrhs <= 16) is the form with independent waves (measured against sharing: profiles/matrix_multivec.txt).  LDS is sized at the launch: W x 8 KB.
// Partial results go to S_r + S_c compact n_y x nrhs matrices (one per wave of a block row / column, as the matvec's partial vectors);
// algebra_multivec_combine adds them in a fixed order and applies alpha, beta and the signs: no atomics, the same bits on every call.
// Every read of X stays in rows below n_x and columns below nrhs, every write of Y in rows below n_y and columns below nrhs.
#ifndef DBCSR_AMD_MM_MULTIVEC_H
#define DBCSR_AMD_MM_MULTIVEC_H
#include <type_traits>
#include "mm_algebra.h"

namespace dbcsr_amd {

constexpr int kMultivecTile = 16;                               // right-hand sides per wave
constexpr int kMultivecWaves = 4;                               // waves (tiles) of a workgroup at most: they share the staged block
constexpr int kMultivecABytes = 5120, kMultivecXBytes = 3072;   // LDS per wave: its share of the staged piece of A; the X rows of its tile
constexpr int kMultivecRows = 64;                               // element rows (column pass: columns) a wave's accumulators cover
static_assert(kMultivecWaves * (kMultivecABytes + kMultivecXBytes) <= 32768, "at most 32 KB of LDS per workgroup");
static_assert(kMultivecABytes / 16 >= kMultivecRows, "a piece holds at least one column of a chunk of any data type");

// len elements at d (element `off` of a 16-byte aligned area) -> lds[0 ... len), by the nt threads of the workgroup: aligned 16-byte loads where vec_ok
template <typename T>
__device__ __forceinline__ void multivec_stage(const T* __restrict__ d, int64_t off, int len, int tid, int nt, int vec_ok, T* lds) {
  walk_block_values(d, off, len, tid, nt, vec_ok, [&](int e, T x) { lds[e] = x; });
}

// The column pass' piece, transposed on the way into the LDS so that the lanes of both passes read it alike: element (i, j) of an m x nj column-major
// part -> lds[i nj + j].  whole: the part is one contiguous piece of memory, e = j m + i (16-byte loads where vec_ok; i and j of a load from one
// multiplication by 1 / m, corrected by one where it rounds across a column: e < 2^24 is exact in float).  Otherwise the h rows from row ia on of every
// column, element by element: thread t takes (i, j) = (t mod P, t / P), P the power of two at or above h.
template <typename T>
__device__ __forceinline__ void multivec_stage_transposed(const T* __restrict__ d, int64_t off, int m, int nj, int ia, int h, int tid, int nt, int vec_ok,
                                                          T* lds) {
  constexpr int V = Pack16<T>::V;
  if (h < m) {
    const int lg = 32 - __clz(h - 1), total = nj << lg;   // (h == 1: lg = 0)
    for (int t = tid; t < total; t += nt) {
      const int i = t & ((1 << lg) - 1), j = t >> lg;
      if (i < h) lds[i * nj + j] = d[(int64_t)j * m + ia + i];
    }
    return;
  }
  const int len = nj * m;
  const float rm = 1.0f / (float)m;
  auto one = [&](int e) {
    int j = (int)((float)e * rm), i = e - j * m;
    if (i < 0) i += m, --j;
    else if (i >= m) i -= m, ++j;
    lds[i * nj + j] = d[e];
  };
  walk_block<T>(off, len, tid, nt, vec_ok, one, [&](int e) {
    const Pack16<T> a = *reinterpret_cast<const Pack16<T>*>(d + e);
    int j = (int)((float)e * rm), i = e - j * m;
    if (i < 0) i += m, --j;
    else if (i >= m) i -= m, ++j;
#pragma unroll
    for (int u = 0; u < V; ++u) {
      lds[i * nj + j] = a.v[u];
      if (++i == m) i = 0, ++j;
    }
  });
}

// the X rows first ... first + nx - 1 of one tile -> xs[16 r + v] (zero for an entry at or behind row n_x or column nrhs: never read)
template <typename T>
__device__ __forceinline__ void multivec_stage_x(const T* __restrict__ x, int64_t first, int nx, int col0, int lane, int64_t n_x, int64_t ldx, int nrhs, T* xs) {
  const int v = lane & (kMultivecTile - 1);
  for (int q = lane; q < nx * kMultivecTile; q += 64) {
    const int64_t r = first + (q >> 4);
    xs[q] = (r < n_x && col0 + v < nrhs) ? x[r * ldx + col0 + v] : T(0);
  }
}

// The products of a staged piece, KM = 4, 8, 12 or 16 accumulators of a lane at work (the count the chunk needs, rounded up to a multiple of four: the
// kernels choose it with one wave-uniform switch per chunk, multivec_by_count).  Every one of the KM updates is unconditional -- an update under a per-lane condition makes
// the compiler carry the whole accumulator array through every branch.  An accumulator whose row (column pass: column) the chunk does not have takes
// whatever the LDS holds there and is never written out: at most 15 elements behind the piece are read, inside the workgroup's LDS (the X rows lie behind
// the pieces).  a: the lane's first element of the piece' first column (column pass: row), `step` elements from one to the next.  The elements of A
// are taken B at a time, and the LDS reads of the next B -- of this column or of the next -- are issued in front of the products of the current ones.
template <typename T, int KM>
__device__ __forceinline__ void multivec_terms(const T* a, int step, const T* xv_at, int count, int conj,
                                                   typename MatvecAcc<T>::type (&acc)[KM]) {
  constexpr int B = sizeof(T) > 8 ? 2 : (KM % 8 == 0 ? 8 : 4);   // elements of A a lane holds at once, twice over (B divides KM): at most 32 registers
  if (count <= 0) return;
  T xv = xv_at[0];
  T av[B];
#pragma unroll
  for (int k = 0; k < B; ++k) av[k] = a[4 * k];
#pragma unroll 2
  for (int jj = 0; jj < count; ++jj) {
    // the LDS reads of the next column are issued in front of this column's products: the loop is bound by its multiply-adds, not by LDS latency
    const T* an = a + (jj + 1 < count ? step : 0);
    const T xn = xv_at[(jj + 1 < count ? jj + 1 : jj) * kMultivecTile];
#pragma unroll
    for (int k0 = 0; k0 < KM; k0 += B) {
      T nv[B];
      const T* src = k0 + B < KM ? a : an;   // (the next group of this column, or the first group of the next)
      const int first = k0 + B < KM ? k0 + B : 0;
#pragma unroll
      for (int k = 0; k < B; ++k) nv[k] = src[4 * (first + k)];
#pragma unroll
      for (int k = 0; k < B; ++k) acc[k0 + k] = acc[k0 + k] + matvec_term(av[k], xv, conj);
#pragma unroll
      for (int k = 0; k < B; ++k) av[k] = nv[k];
    }
    a = an;
    xv = xn;
  }
}

// f(KM) for the KM = 4, 8, 12 or 16 that covers kmax accumulators (wave-uniform)
template <typename F>
__device__ __forceinline__ void multivec_by_count(int kmax, F&& f) {
  switch ((kmax + 3) >> 2) {
    case 1: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 8>{}); break;
    case 3: f(std::integral_constant<int, 12>{}); break;
    default: f(std::integral_constant<int, 16>{});
  }
}

// partials[(sub n_y + yoff[row] + r) nrhs + v] = sum over the blocks sub, sub + S, ... of block row `row` of sum_j g(a_rj) X[xoff[c] + j][v], for every
// element row r of the block row and every right-hand side v (zero when the wave met no block).  Workgroup blockIdx.x = (row S + sub) G + tile group;
// its wave w has tile (tile group) W + w.  skip_diag: blocks on the block diagonal do not count (the twin part of a stored triangle).
template <typename T>
__global__ void __launch_bounds__(256, 4)   // (four waves per SIMD: 128 registers)
algebra_multivec_rows(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const T* __restrict__ data,
                      const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ yoff, const int64_t* __restrict__ xoff, int nbr,
                      int S, int G, int conj, int skip_diag, int vec_ok, const T* __restrict__ x, int64_t n_x, int64_t ldx, int nrhs, int64_t n_y,
                      typename MatvecAcc<T>::type* __restrict__ partials) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr int XR = kMultivecXBytes / (int)sizeof(T) / kMultivecTile;
  extern __shared__ __align__(16) unsigned char multivec_lds[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, W = nt >> 6;
  const int g = lane >> 4, v = lane & (kMultivecTile - 1);
  const int64_t unit = blockIdx.x / G;
  const int row = (int)(unit / S), sub = (int)(unit % S);
  if (row >= nbr) return;   // (the whole workgroup)
  const int m = rs[row];
  if (m <= 0) return;
  const int col0 = ((int)(blockIdx.x % G) * W + wave) * kMultivecTile;
  const bool live = col0 < nrhs;   // (a wave without a tile still helps to load the block)
  T* as = reinterpret_cast<T*>(multivec_lds);
  T* xs = reinterpret_cast<T*>(multivec_lds + (size_t)W * kMultivecABytes + (size_t)wave * kMultivecXBytes);
  const int capA = W * (kMultivecABytes / (int)sizeof(T));
  const int64_t base = yoff[row];
  Acc* __restrict__ mine = partials + (size_t)sub * n_y * nrhs;
  const int b0 = row_p[row] + sub, b1 = row_p[row + 1];
  for (int r0 = 0; r0 < m; r0 += kMultivecRows) {
    const int mr = m - r0 < kMultivecRows ? m - r0 : kMultivecRows;
    const int kmax = (mr + 3) >> 2, nk = mr > g ? (mr - g + 3) >> 2 : 0;   // rows g, g + 4, ... of the chunk: nk of them are this lane's
    const int cols_per = capA / mr;
    auto chunk = [&](auto km) {   // (the whole chunk per count of accumulators: the array never crosses a branch between the forms)
    constexpr int KM = decltype(km)::value;
    Acc acc[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[k] = Acc(0.0);
    for (int b = b0; b < b1; b += S) {
      const int c = col_i[b];
      if (skip_diag && c == row) continue;
      const int n = cs[c];
      const int64_t off = blk_p[b], xb = xoff[c];
      for (int ja = 0; ja < n; ja += cols_per) {
        const int jb = ja + cols_per < n ? ja + cols_per : n;
        const int len = (jb - ja) * mr;
        if (m <= kMultivecRows) {   // whole columns: one contiguous piece of memory
          multivec_stage(data + off + (int64_t)ja * m, off + (int64_t)ja * m, len, tid, nt, vec_ok, as);
        } else {                    // the chunk's rows of every column
          const T* d = data + off + (int64_t)ja * m + r0;
          for (int e = tid; e < len; e += nt) {
            const int jj = e / mr;
            as[e] = d[(int64_t)jj * m + (e - jj * mr)];
          }
        }
        for (int jx = ja; jx < jb; jx += XR) {
          const int nx = jb - jx < XR ? jb - jx : XR;
          if (live) multivec_stage_x(x, xb + jx, nx, col0, lane, n_x, ldx, nrhs, xs);
          __syncthreads();
          if (live) {
            const int64_t left = n_x - (xb + jx);   // (a term whose row of X lies at n_x or behind is not formed)
            const int count = left < nx ? (left > 0 ? (int)left : 0) : nx;
            const T* a = as + (jx - ja) * mr + g;
            multivec_terms<T, KM>(a, mr, xs + v, count, conj, acc);
          }
          __syncthreads();   // (the next piece and the next rows of X overwrite the LDS)
        }
      }
    }
    if (live && col0 + v < nrhs) {
      int gw = g;
      asm volatile("" : "+v"(gw));   // (keeps the KM row indices and addresses of the write-out from being formed, and held, in front of the walk)
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        const int64_t i = base + r0 + gw + 4 * k;
        if (k < nk && i < n_y) mine[i * nrhs + col0 + v] = acc[k];
      }
    }
    };
    multivec_by_count(kmax, chunk);
  }
}

// partials[(sub n_y + yoff[c] + j) nrhs + v] = sum over the entries sub, sub + S, ... of block column c's list of sum_i g(a_ij) X[xoff[r] + i][v]: the row
// pass with the roles of i and j exchanged -- the lane owns every fourth COLUMN of the block, 64 columns at a time, and walks the element rows.  A
// piece is the whole 64-column part of the block where it fits, else as many element rows of its columns as fit; it is transposed on its way into the LDS
// (multivec_stage_transposed), and the products are the row pass' (multivec_terms).
template <typename T>
__global__ void __launch_bounds__(256, 4)
algebra_multivec_cols(const int* __restrict__ col_p, const int* __restrict__ list, const int64_t* __restrict__ blk_p, const T* __restrict__ data,
                      const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ yoff, const int64_t* __restrict__ xoff, int nbc,
                      int S, int G, int conj, int skip_diag, int vec_ok, const T* __restrict__ x, int64_t n_x, int64_t ldx, int nrhs, int64_t n_y,
                      typename MatvecAcc<T>::type* __restrict__ partials) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr int XR = kMultivecXBytes / (int)sizeof(T) / kMultivecTile;
  extern __shared__ __align__(16) unsigned char multivec_lds[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, W = nt >> 6;
  const int g = lane >> 4, v = lane & (kMultivecTile - 1);
  const int64_t unit = blockIdx.x / G;
  const int c = (int)(unit / S), sub = (int)(unit % S);
  if (c >= nbc) return;   // (the whole workgroup)
  const int n = cs[c];
  if (n <= 0) return;
  const int col0 = ((int)(blockIdx.x % G) * W + wave) * kMultivecTile;
  const bool live = col0 < nrhs;
  T* as = reinterpret_cast<T*>(multivec_lds);
  T* xs = reinterpret_cast<T*>(multivec_lds + (size_t)W * kMultivecABytes + (size_t)wave * kMultivecXBytes);
  const int capA = W * (kMultivecABytes / (int)sizeof(T));
  const int64_t base = yoff[c];
  Acc* __restrict__ mine = partials + (size_t)sub * n_y * nrhs;
  const int t0 = col_p[c] + sub, t1 = col_p[c + 1];
  for (int j0 = 0; j0 < n; j0 += kMultivecRows) {
    const int nj = n - j0 < kMultivecRows ? n - j0 : kMultivecRows;
    const int kmax = (nj + 3) >> 2;
    auto chunk = [&](auto km) {
    constexpr int KM = decltype(km)::value;
    Acc acc[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[k] = Acc(0.0);
    for (int t = t0; t < t1; t += S) {
      const int r = list[2 * (size_t)t + 1];
      if (skip_diag && r == c) continue;
      const int m = rs[r];
      if (m <= 0) continue;
      const int64_t off = blk_p[list[2 * (size_t)t]] + (int64_t)j0 * m, xb = xoff[r];
      const int rows_per = nj * m <= capA ? m : capA / nj;   // the whole part, or as many rows of its nj columns as a piece holds
      for (int ia = 0; ia < m; ia += rows_per) {
        const int h = m - ia < rows_per ? m - ia : rows_per;
        multivec_stage_transposed(data + off, off, m, nj, ia, h, tid, nt, vec_ok, as);
        for (int ix = ia; ix < ia + h; ix += XR) {
          const int nx = ia + h - ix < XR ? ia + h - ix : XR;
          if (live) multivec_stage_x(x, xb + ix, nx, col0, lane, n_x, ldx, nrhs, xs);
          __syncthreads();
          if (live) {
            const int64_t left = n_x - (xb + ix);   // (a term whose row of X lies at n_x or behind is not formed)
            const int count = left < nx ? (left > 0 ? (int)left : 0) : nx;
            const T* a = as + (ix - ia) * nj + g;
            multivec_terms<T, KM>(a, nj, xs + v, count, conj, acc);
          }
          __syncthreads();   // (the next piece and the next rows of X overwrite the LDS)
        }
      }
    }
    if (live && col0 + v < nrhs) {
      int gw = g;
      asm volatile("" : "+v"(gw));   // (as in the row pass)
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        const int j = gw + 4 * k;
        const int64_t i = base + j0 + j;
        if (j < nj && i < n_y) mine[i * nrhs + col0 + v] = acc[k];
      }
    }
    };
    multivec_by_count(kmax, chunk);
  }
}

// Y[i][v] = alpha (row_sign * sum_k row partial k + col_sign * sum_k column partial k) + beta Y[i][v] for i below n_y and below *total (the full length,
// on the device) and v below nrhs: algebra_matvec_combine per element of the compact n_y x nrhs partial matrices, the same order (rows 0 ... S_r - 1,
// then columns 0 ... S_c - 1), the same modes.  Y has the leading dimension ldy: its padding columns are not written, nor anything else.
template <typename T>
__global__ void __launch_bounds__(256)
algebra_multivec_combine(const typename MatvecAcc<T>::type* __restrict__ partials, int S_r, int S_c, double row_sign, double col_sign, int64_t n_y, int nrhs,
                         int64_t ldy, const int64_t* __restrict__ total, typename MatvecAcc<T>::type alpha, typename MatvecAcc<T>::type beta, int mode,
                         T* __restrict__ y) {
  using Acc = typename MatvecAcc<T>::type;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = t / nrhs;
  if (i >= n_y || i >= *total) return;
  T* __restrict__ out = y + i * ldy + (t - i * nrhs);
  if (mode & kMatvecNoProduct) {
    *out = (mode & kMatvecBetaZero) ? T(0) : matvec_scaled(matvec_narrow<T>(beta), *out);
    return;
  }
  const size_t plane = (size_t)n_y * nrhs;
  Acc s = Acc(0.0);
  for (int k = 0; k < S_r; ++k) s = s + matvec_signed(partials[(size_t)k * plane + t], row_sign);
  for (int k = 0; k < S_c; ++k) s = s + matvec_signed(partials[(size_t)(S_r + k) * plane + t], col_sign);
  Acc r = alpha * s;
  if (!(mode & kMatvecBetaZero)) r = r + beta * matvec_wide(*out);
  *out = matvec_narrow<T>(r);
}

}  // namespace dbcsr_amd
#endif
