// mm_algebra.h -- matrix algebra between multiplies (src/ops/dbcsr_operations.F: dbcsr_add, dbcsr_add_on_diag, dbcsr_trace, dbcsr_dot,
// dbcsr_frobenius_norm): the union pattern of two matrices, the numeric add per block and flat, the diagonal helpers and the reductions.
// Part of the device-resident multiply engine: included by mm_engine.hip after mm_aux.h.
//
// Every kernel goes by the index (row_p, col_i, blk_p), never by the extent of a data area: an operand may have holes (the result of an in-place filter).
// ASSUMPTION, shared with the symbolic phase (fill_products / emit_index look a block of C_in up the same way): the block columns of a block row are
// stored in ascending order, so the position of block (i, j) inside row i is the number of blocks of that row with a column below j -- the bitmap rank
// row_p[i] + pre[i][j / 32] + popc(word & below) of the add, the binary search of the dot.  Every matrix this library makes has that order.
//
// All of them stream memory: 16-byte accesses where the addresses allow (a block of a matrix with 1 x 1 or odd blocks starts at any element), enough waves
// per block row (row_split) to fill the chip, no atomics on data, no floating-point atomics at all -- the reductions write one partial per wave and
// checksum_final (mm_aux.h) sums the partials in a fixed order, so a result is the same bits on every call.
// Every kernel that goes through a block element by element does it with walk_block / walk_block_values (mm_block_walk.h: the head in front of the
// first 16-byte boundary, the whole packs, the tail, in one fixed order per thread); the row passes (row_sum_slots, matvec_row_slots) walk slots at a
// stride instead and share their geometry, their dispatch on the block's shift and their hand-over (row_slots_of, DBCSR_AMD_BY_SHIFT, row_handover), the column
// passes the rotated add of a lane's run (add_run_rotated).
#ifndef DBCSR_AMD_MM_ALGEBRA_H
#define DBCSR_AMD_MM_ALGEBRA_H
#include "mm_block_walk.h"  // Pack16, Pack16U, walk_block
#include "mm_complex.h"
#include "mm_epilogue.h"  // wave_sum

namespace dbcsr_amd {

// bits of `mode`: the scalar is exactly 1 and the operand is taken as it is (bit-identical, NaN and -0 included)
constexpr int kAlphaIsOne = 1, kBetaIsOne = 2;

template <typename T>
__device__ __forceinline__ T scaled_by(T x, T s, bool is_one) { return is_one ? x : s * x; }

template <typename T>
__device__ __forceinline__ T axpby(T a, T b, T alpha, T beta, int mode) {
  return scaled_by(a, alpha, mode & kAlphaIsOne) + scaled_by(b, beta, mode & kBetaIsOne);
}

// |x|^2 and the parts of x in double (fp32 data converted first: its products are exact in double)
__device__ __forceinline__ double abs2_of(double x) { return x * x; }
__device__ __forceinline__ double abs2_of(float x) { return (double)x * (double)x; }
__device__ __forceinline__ double abs2_of(z64 x) { return x.re * x.re + x.im * x.im; }
__device__ __forceinline__ double re_of(double x) { return x; }
__device__ __forceinline__ double re_of(float x) { return (double)x; }
__device__ __forceinline__ double re_of(z64 x) { return x.re; }
__device__ __forceinline__ double im_of(double) { return 0.0; }
__device__ __forceinline__ double im_of(float) { return 0.0; }
__device__ __forceinline__ double im_of(z64 x) { return x.im; }

// ---- same pattern? ---------------------------------------------------------------------------------------------------
// S waves per block row of A (both matrices have nblks blocks: the host checked).  flags: bit 0 row_p or col_i differ, bit 1 blk_p differs,
// bit 2 A is not packed (blk_p is not the running sum of the block sizes).  *nze_out: end of A's last block = its element count when packed.
__global__ void __launch_bounds__(256) algebra_compare(const int* __restrict__ a_row_p, const int* __restrict__ a_col_i, const int64_t* __restrict__ a_blk_p,
                                                       const int* __restrict__ b_row_p, const int* __restrict__ b_col_i, const int64_t* __restrict__ b_blk_p,
                                                       const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S, int64_t nblks,
                                                       int* __restrict__ flags, int64_t* __restrict__ nze_out) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int b0 = a_row_p[row], b1 = a_row_p[row + 1];
  int bad = (b0 != b_row_p[row] || b1 != b_row_p[row + 1]) ? 1 : 0;
  if (b0 < 0 || b1 > nblks || b1 < b0) bad |= 1;   // (an index that does not belong to these arrays: never read outside them)
  if (!bad) {
    const int m = rs[row];
    for (int b = b0 + sub * 64 + lane; b < b1; b += S * 64) {
      const int c = a_col_i[b];
      const int64_t p = a_blk_p[b], end = p + (int64_t)m * cs[c];
      if (c != b_col_i[b]) bad |= 1;
      if (p != b_blk_p[b]) bad |= 2;
      if (b == 0 && p != 0) bad |= 4;
      if (b + 1 < nblks) {
        if (a_blk_p[b + 1] != end) bad |= 4;
      } else {
        *nze_out = end;
      }
    }
  }
  if (bad) atomicOr(flags, bad);
}

// ---- union pattern ----------------------------------------------------------------------------------------------------
// thread per (row, word): the union bitmap (b_bm == nullptr: A's pattern alone, the add with beta == 0)
__global__ void __launch_bounds__(256) algebra_union(const uint32_t* __restrict__ a_bm, const uint32_t* __restrict__ b_bm, int64_t nwords,
                                                     uint32_t* __restrict__ c_bm) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nwords) c_bm[t] = a_bm[t] | (b_bm ? b_bm[t] : 0u);
}

// thread per (row, word), in the manner of emit_index: the result's col_i / blk_p and, per result block, the offsets of its sources in A's and B's data
// areas (src[2 cb], src[2 cb + 1]; -1: the operand has no such block)
__global__ void __launch_bounds__(256)
algebra_emit(const int* __restrict__ a_row_p, const int64_t* __restrict__ a_blk_p, const uint32_t* __restrict__ a_bm, const int* __restrict__ a_pre,
             const int* __restrict__ b_row_p, const int64_t* __restrict__ b_blk_p, const uint32_t* __restrict__ b_bm, const int* __restrict__ b_pre,
             const uint32_t* __restrict__ c_bm, const int* __restrict__ c_pre, const int* __restrict__ c_row_p, const int64_t* __restrict__ c_blk_p_ws,
             int nbr, int W, int* __restrict__ c_col_i, int64_t* __restrict__ c_blk_p, int64_t* __restrict__ src) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nbr * W) return;
  const int i = (int)(t / W), w = (int)(t % W);
  uint32_t v = c_bm[t];
  if (!v) return;
  int cb = c_row_p[i] + c_pre[t];
  const uint32_t aw = a_bm[t], bw = b_bm ? b_bm[t] : 0u;
  while (v) {
    const int bit = __ffs(v) - 1;
    v &= v - 1;
    const uint32_t below = (1u << bit) - 1u;
    c_col_i[cb] = 32 * w + bit;
    c_blk_p[cb] = c_blk_p_ws[cb];
    src[2 * (size_t)cb] = ((aw >> bit) & 1u) ? a_blk_p[a_row_p[i] + a_pre[t] + __popc(aw & below)] : -1;
    src[2 * (size_t)cb + 1] = ((bw >> bit) & 1u) ? b_blk_p[b_row_p[i] + b_pre[t] + __popc(bw & below)] : -1;
    ++cb;
  }
}

// ---- numeric add ------------------------------------------------------------------------------------------------------
// dst block = alpha * a block + beta * b block, by block row with S waves per row (wave s takes the result blocks s mod S), lanes over the elements.  A block
// present in one operand only is alpha * a or beta * b; a scalar that is exactly 1 multiplies nothing.  16-byte accesses when dst's area is 16-byte aligned
// (vec_ok): the stores are aligned -- the elements in front of dst's first boundary and behind its last whole 16 bytes go one by one --, the loads take the
// same elements from wherever the source blocks start (Pack16U).  dst aliases neither operand (the host refuses it).
template <typename T>
__global__ void __launch_bounds__(256)
algebra_add_blocks(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const int64_t* __restrict__ src,
                   const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S, const T* __restrict__ a_data, const T* __restrict__ b_data,
                   T* __restrict__ d_data, T alpha, T beta, int mode, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  for (int t = row_p[row] + sub; t < row_p[row + 1]; t += S) {
    const int ne = m * cs[col_i[t]];
    const int64_t ao = src[2 * (size_t)t], bo = src[2 * (size_t)t + 1], dof = blk_p[t];
    const T* a = a_data + (ao >= 0 ? ao : 0);
    const T* b = b_data + (bo >= 0 ? bo : 0);
    T* d = d_data + dof;
    const int have = (ao >= 0 ? 1 : 0) | (bo >= 0 ? 2 : 0);   // (wave-uniform)
    auto one = [&](int e) {
      if (have == 3) d[e] = axpby(a[e], b[e], alpha, beta, mode);
      else if (have == 1) d[e] = scaled_by(a[e], alpha, mode & kAlphaIsOne);
      else d[e] = scaled_by(b[e], beta, mode & kBetaIsOne);
    };
    walk_block<T>(dof, ne, lane, 64, vec_ok, one, [&](int e) {   // (aligned on dst's block)
      Pack16<T> r;
      if (have == 3) {
        const Pack16U<T> x = *reinterpret_cast<const Pack16U<T>*>(a + e), y = *reinterpret_cast<const Pack16U<T>*>(b + e);
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = axpby(x.v[u], y.v[u], alpha, beta, mode);
      } else if (have == 1) {
        const Pack16U<T> x = *reinterpret_cast<const Pack16U<T>*>(a + e);
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = scaled_by(x.v[u], alpha, mode & kAlphaIsOne);
      } else {
        const Pack16U<T> y = *reinterpret_cast<const Pack16U<T>*>(b + e);
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = scaled_by(y.v[u], beta, mode & kBetaIsOne);
      }
      *reinterpret_cast<Pack16<T>*>(d + e) = r;
    });
  }
}

// Same pattern, same block offsets, A packed: one flat pass over the n elements of the data areas, dst[i] = alpha * a[i] + beta * b[i].  dst may be a (in
// place: a lane loads its elements before it stores them, and nobody else touches them).  One 16-byte access per operand and lane, one workgroup per 4 KiB
// of each area and no loop: on 8.6 GB per area (a += beta * b, float64) this form ran 4.39 ... 4.50 ms where grid-stride loops over 2048 workgroups with 1 ... 8
// accesses in flight per lane ran 4.6 ... 5.4 ms and torch.add 4.6 ms (tools/ubench/ubench_flat_add.hip, profiles/matrix_ops.txt).  The last n mod V elements
// go one by one.
template <typename T>
__global__ void __launch_bounds__(256) algebra_add_flat(const T* a, const T* b, T* dst, int64_t n, T alpha, T beta, int mode, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!vec_ok) {
    if (i < n) dst[i] = axpby(a[i], b[i], alpha, beta, mode);
    return;
  }
  const int64_t nv = n / V;
  if (i < nv) {
    const Pack16<T> x = reinterpret_cast<const Pack16<T>*>(a)[i], y = reinterpret_cast<const Pack16<T>*>(b)[i];
    Pack16<T> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = axpby(x.v[k], y.v[k], alpha, beta, mode);
    reinterpret_cast<Pack16<T>*>(dst)[i] = r;
  } else {
    const int64_t e = nv * V + (i - nv);
    if (e < n) dst[e] = axpby(a[e], b[e], alpha, beta, mode);
  }
}

// ---- the diagonal (dbcsr_add_on_diag) -----------------------------------------------------------------------------------
// position of the diagonal block of block row `row` in the index, or -1 (every lane gets the answer; any column order)
__device__ __forceinline__ int find_diag_block(const int* __restrict__ row_p, const int* __restrict__ col_i, int row, int lane) {
  int found = -1;
  for (int base = row_p[row]; base < row_p[row + 1] && found < 0; base += 64) {
    const int b = base + lane;
    const unsigned long long hit = __ballot(b < row_p[row + 1] && col_i[b] == row);
    if (hit) found = base + (__ffsll((long long)hit) - 1);
  }
  return found;
}

// one wavefront per block row: need[row] = 1 and blk_nze[row] = m * m when the row has no diagonal block, 0 otherwise
__global__ void __launch_bounds__(256) diag_missing(const int* __restrict__ row_p, const int* __restrict__ col_i, const int* __restrict__ rs, int nbr,
                                                    int* __restrict__ need, int* __restrict__ blk_nze) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= nbr) return;
  const int at = find_diag_block(row_p, col_i, row, lane);
  if (lane == 0) {
    need[row] = at < 0 ? 1 : 0;
    blk_nze[row] = at < 0 ? rs[row] * rs[row] : 0;
  }
}

// thread per block row: the index entries of the missing diagonal blocks (d_row_p is the scan of need[], off[] the scan of blk_nze[])
__global__ void __launch_bounds__(256) diag_emit(const int* __restrict__ need, const int* __restrict__ d_row_p, const int64_t* __restrict__ off, int nbr,
                                                 int* __restrict__ d_col_i, int64_t* __restrict__ d_blk_p) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nbr || !need[row]) return;
  d_col_i[d_row_p[row]] = row;
  d_blk_p[d_row_p[row]] = off[row];
}

// one wavefront per block row of a matrix of diagonal blocks: block = alpha * identity
template <typename T>
__global__ void __launch_bounds__(256) diag_fill(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                 const int* __restrict__ rs, int nbr, T alpha, T* __restrict__ data) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= nbr) return;
  const int m = rs[row];
  for (int b = row_p[row]; b < row_p[row + 1]; ++b) {
    if (col_i[b] != row) continue;   // (not a diagonal block: not this kernel's)
    T* d = data + blk_p[b];
    for (int e = lane; e < m * m; e += 64) d[e] = (e % m == e / m) ? alpha : T(0);
  }
}

// one wavefront per block row, in place: alpha is added to the diagonal elements of the diagonal block the row has (nothing else is written)
template <typename T>
__global__ void __launch_bounds__(256) diag_shift(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                  const int* __restrict__ rs, const int* __restrict__ cs, int nbr, T alpha, T* __restrict__ data) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= nbr) return;
  const int at = find_diag_block(row_p, col_i, row, lane);
  if (at < 0) return;
  const int m = rs[row];
  if (cs[row] != m) return;   // (not a square block: the caller's sizes are not those of a square matrix; never write outside the block)
  T* d = data + blk_p[at];
  for (int e = lane; e < m; e += 64) d[(size_t)e * (m + 1)] = d[(size_t)e * (m + 1)] + alpha;
}

// ---- reductions ---------------------------------------------------------------------------------------------------------
// Each writes one pair of doubles per wave (partials[2 wave], partials[2 wave + 1]); checksum_final sums the pairs in a fixed order.

// trace: one wavefront per block row, the diagonal elements of its diagonal block (real part, imaginary part)
template <typename T>
__global__ void __launch_bounds__(256) algebra_trace(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                     const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs, int nbr,
                                                     double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= nbr) return;
  double sr = 0.0, si = 0.0;
  const int at = find_diag_block(row_p, col_i, row, lane);
  if (at >= 0) {
    const int m = rs[row], n = cs[row], k = m < n ? m : n;
    const T* d = data + blk_p[at];
    for (int e = lane; e < k; e += 64) {
      const T x = d[(size_t)e * (m + 1)];
      sr += re_of(x);
      si += im_of(x);
    }
  }
  sr = wave_sum(sr);
  si = wave_sum(si);
  if (lane == 0) {
    partials[2 * (size_t)row] = sr;
    partials[2 * (size_t)row + 1] = si;
  }
}

// squared Frobenius norm: S waves per block row; with `symmetric` a block off the diagonal counts twice (it stands for its twin too)
template <typename T>
__global__ void __launch_bounds__(256) algebra_norm2(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                     const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S,
                                                     int symmetric, int vec_ok, double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  double acc = 0.0;
  for (int b = row_p[row] + sub; b < row_p[row + 1]; b += S) {
    const int c = col_i[b], ne = m * cs[c];
    const int64_t off = blk_p[b];
    double s = 0.0;
    walk_block_values(data + off, off, ne, lane, 64, vec_ok, [&](int, T x) { s += abs2_of(x); });
    acc += (symmetric && c != row) ? 2.0 * s : s;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    partials[2 * (size_t)wv] = acc;
    partials[2 * (size_t)wv + 1] = 0.0;
  }
}

// dot (real data): sum a_ij b_ij over the blocks both matrices store.  S waves per block row of A; B's block (row, c) is found by a binary search of B's
// row (ascending columns, see the head of this file): no work area, nothing a saved plan depends on is touched.
template <typename T>
__global__ void __launch_bounds__(256)
algebra_dot(const int* __restrict__ a_row_p, const int* __restrict__ a_col_i, const int64_t* __restrict__ a_blk_p, const T* __restrict__ a_data,
            const int* __restrict__ b_row_p, const int* __restrict__ b_col_i, const int64_t* __restrict__ b_blk_p, const T* __restrict__ b_data,
            const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S, int symmetric, int vec_ok, double* __restrict__ partials) {
  constexpr int V = Pack16<T>::V;
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  const int q0 = b_row_p[row], q1 = b_row_p[row + 1];
  double acc = 0.0;
  for (int b = a_row_p[row] + sub; b < a_row_p[row + 1]; b += S) {
    const int c = a_col_i[b];
    int lo = q0, hi = q1;   // first position of B's row with a column >= c
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (b_col_i[mid] < c) lo = mid + 1; else hi = mid;
    }
    if (lo >= q1 || b_col_i[lo] != c) continue;   // (wave-uniform)
    const int ne = m * cs[c];
    const int64_t ao = a_blk_p[b], bo = b_blk_p[lo];
    const T* x = a_data + ao;
    const T* y = b_data + bo;
    double s = 0.0;
    walk_block<T>(   // (aligned on A's block; B's is read from wherever it starts)
        ao, ne, lane, 64, vec_ok, [&](int e) { s += (double)x[e] * (double)y[e]; },
        [&](int e) {
          const Pack16<T> p = *reinterpret_cast<const Pack16<T>*>(x + e);
          const Pack16U<T> r = *reinterpret_cast<const Pack16U<T>*>(y + e);
#pragma unroll
          for (int u = 0; u < V; ++u) s += (double)p.v[u] * (double)r.v[u];
        });
    acc += (symmetric && c != row) ? 2.0 * s : s;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    partials[2 * (size_t)wv] = acc;
    partials[2 * (size_t)wv + 1] = 0.0;
  }
}

// ---- norms and vectors (dbcsr_norm, dbcsr_gershgorin_norm, dbcsr_maxabs_norm, dbcsr_get_diag / _set_diag, dbcsr_scale_by_vector) --------------------
// A result or an operand per FULL row or column of the matrix: a kernel must know where an element sits inside its column-major block (element row e % m,
// element column e / m), and the element offset of its block row / column (roff / coff: exclusive scans of the block sizes, formed on the device).  Sums are
// carried in double and written once per wave (S partial vectors); algebra_vec_combine adds the partial vectors in a fixed order.  No atomics.

// what == 0: |x|, what == 1: |x|^2, in double (fp32 data converted first; |z| as the root of re^2 + im^2)
__device__ __forceinline__ double absval_of(double x, int what) { return what ? x * x : fabs(x); }
__device__ __forceinline__ double absval_of(float x, int what) { return what ? (double)x * (double)x : fabs((double)x); }
__device__ __forceinline__ double absval_of(z64 x, int what) { const double s = x.re * x.re + x.im * x.im; return what ? s : sqrt(s); }

// Hand-over of values between the lanes of ONE wave through its own LDS slice: the hardware keeps a wave's LDS operations in order; the fences keep the
// compiler from moving the LDS accesses of one side across to the other (release what was written, acquire before reading), the barrier its scheduler.
__device__ __forceinline__ void wave_lds_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the larger of two values, NaN if either is one (a plain maximum would drop it: a matrix that holds a NaN must not report a finite norm)
__device__ __forceinline__ double max_or_nan(double a, double b) { return b != b ? b : (a < b ? b : a); }

constexpr int kStageElems = 1024;   // doubles of LDS per wave (column sums: one piece of a block; row sums: the lanes' accumulators at the end of a row)

// ---- what the row passes share (algebra_row_sums, algebra_matvec_rows) ---------------------------------------------------------------------------------
// The 16-byte slots of a block row with m element rows: p = m / gcd(V, m) lanes are one period of the element rows, P = the largest multiple of p that 64
// lanes hold (0 when p > 64: the slot form is not used)
struct RowSlots {
  int p, P;
};
template <int V>
__device__ __forceinline__ RowSlots row_slots_of(int m) {
  const int g = V == 1 ? 1 : (m % V == 0 ? V : (m % 2 == 0 ? 2 : 1));   // gcd(V, m), V = 1, 2 or 4
  const int p = m / g;
  return RowSlots{p, (64 / p) * p};
}

// F<T, A>(...) for the wave-uniform shift a = 0 ... V - 1 of a block against a 16-byte boundary, A the same value as a compile-time constant (T and V: the
// caller's; 1 % V ... keep a type with a smaller V from instantiating a shift it does not have).  A macro, so that the calls stand in the kernel as they
// would by hand: through a function that takes a callable the compiler laid the branches of algebra_matvec_rows<double> out differently, a product and
// its sum ended up in different blocks and were no longer contracted -- other bits.
#define DBCSR_AMD_BY_SHIFT(F, a, ...)               \
  do {                                              \
    if (V == 1 || (a) == 0) F<T, 0>(__VA_ARGS__);   \
    else if ((a) == 1) F<T, 1 % V>(__VA_ARGS__);    \
    else if ((a) == 2) F<T, 2 % V>(__VA_ARGS__);    \
    else F<T, 3 % V>(__VA_ARGS__);                  \
  } while (0)

// The end of a block row: the 2 V - 1 accumulators of every lane go through the wave's LDS slice (64 per accumulator), and lane r = lane, lane + 64, ...
// below m hands store(r, sum) the sum of those that belong to element row r -- accumulator k of lane l belongs to row (V l + k - (V - 1)) mod m -- in the
// order (k, then l = l0, l0 + p, ... below P).
template <int V, typename Acc, typename Store>
__device__ __forceinline__ void row_handover(const Acc (&acc)[2 * V - 1], Acc* slice, int lane, int m, RowSlots sl, Store&& store) {
  constexpr int K = 2 * V - 1;
#pragma unroll
  for (int k = 0; k < K; ++k) slice[k * 64 + lane] = acc[k];
  wave_lds_handover();   // (the slice is this wave's alone)
  for (int r = lane; r < m; r += 64) {
    Acc sum = Acc(0.0);
    for (int k = 0; k < K; ++k) {
      // the lanes l with (V l + k - (V - 1)) mod m == r: the first one below the period p (found without touching LDS), then every p-th
      int cur = ((k - (V - 1)) % m + m) % m, l0 = 0;
      while (l0 < sl.p && cur != r) {
        ++l0;
        cur += V;
        if (cur >= m) cur -= m;
        if (cur >= m) cur %= m;   // (m < V)
      }
      if (l0 < sl.p)
        for (int l = l0; l < sl.P; l += sl.p) sum = sum + slice[k * 64 + l];
    }
    store(r, sum);
  }
}

// Row sums, the elements of one block through the lanes of a wave.  A lane takes the 16-byte slots s = lane, lane + P, ... of the block; slot s holds the
// elements V s - A ... V s - A + V - 1 (A = elements by which the block starts behind a 16-byte boundary, so every whole slot is one aligned access; the
// first and the last slot may be cut by the block's ends and go element by element).  With V P a multiple of m the element rows a lane meets never change
// inside a block row: accumulator k of lane l belongs to element row (V l + k - (V - 1)) mod m whatever A is, k = 0 ... 2 V - 2.
template <typename T, int A>
__device__ __forceinline__ void row_sum_slots(const T* __restrict__ d, int ne, int lane, int P, int vec_ok, int what, double (&acc)[2 * Pack16<T>::V - 1]) {
  constexpr int V = Pack16<T>::V;
  const int nslots = (ne + A + V - 1) / V;
  for (int s = lane; s < nslots; s += P) {
    const int e0 = V * s - A;
    if (vec_ok && e0 >= 0 && e0 + V <= ne) {
      const Pack16<T> x = *reinterpret_cast<const Pack16<T>*>(d + e0);
#pragma unroll
      for (int u = 0; u < V; ++u) acc[V - 1 - A + u] += absval_of(x.v[u], what);
    } else {
#pragma unroll
      for (int u = 0; u < V; ++u)
        if (e0 + u >= 0 && e0 + u < ne) acc[V - 1 - A + u] += absval_of(d[e0 + u], what);
    }
  }
}

// sum_j f(a_ij) per full row: S waves per block row, wave (row, sub) takes the blocks sub, sub + S, ... of the row and writes partials[sub * n_out + roff[row] + r]
// for every element row r of the block row (zero when it met no block).  Every element is read once.  m / gcd(V, m) <= 64: the slot form above with
// P = the largest multiple of m / gcd(V, m) that 64 lanes hold (23 x 23 doubles: 46 lanes, 16 bytes each); at the end of the row the accumulators go
// through the wave's LDS slice and lane r adds those of its row in the order (k, lane).  Taller blocks: 64 element rows at a time, a lane per row, the
// columns of every block one after the other (consecutive lanes read consecutive elements).
template <typename T>
__global__ void __launch_bounds__(256)
algebra_row_sums(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const T* __restrict__ data,
                 const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ roff, int nbr, int S, int what, int vec_ok,
                 int64_t n_out, double* __restrict__ partials) {
  constexpr int V = Pack16<T>::V, K = 2 * V - 1;
  __shared__ double red[4][K * 64];
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0) return;
  const int64_t base = roff[row];
  double* __restrict__ mine = partials + (size_t)sub * n_out;
  const int b0 = row_p[row] + sub, b1 = row_p[row + 1];
  const RowSlots sl = row_slots_of<V>(m);
  if (sl.p > 64) {
    for (int r0 = 0; r0 < m; r0 += 64) {
      const int r = r0 + lane;
      double acc = 0.0;
      if (r < m)
        for (int b = b0; b < b1; b += S) {
          const int n = cs[col_i[b]];
          const T* d = data + blk_p[b] + r;
          for (int j = 0; j < n; ++j) acc += absval_of(d[(size_t)m * j], what);
        }
      if (r < m && base + r < n_out) mine[base + r] = acc;
    }
    return;
  }
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  if (lane < sl.P)
    for (int b = b0; b < b1; b += S) {
      const int ne = m * cs[col_i[b]];
      const int64_t off = blk_p[b];
      const T* d = data + off;
      const int a = vec_ok ? (int)(off & (V - 1)) : 0;   // (wave-uniform)
      DBCSR_AMD_BY_SHIFT(row_sum_slots, a, d, ne, lane, sl.P, vec_ok, what, acc);
    }
  row_handover<V>(acc, red[threadIdx.x >> 6], lane, m, sl, [&](int r, double sum) {
    if (base + r < n_out) mine[base + r] = sum;
  });
}

// out[i] = the sum of the S partial vectors in the order 0 ... S - 1, for i below *total (the full length, on the device); zero behind it
__global__ void __launch_bounds__(256) algebra_vec_combine(const double* __restrict__ partials, int S, int64_t n_out, const int64_t* __restrict__ total,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  double s = 0.0;
  if (i < *total)
    for (int k = 0; k < S; ++k) s += partials[(size_t)k * n_out + i];
  out[i] = s;
}

// The blocks of every block column in ascending block-row order, built as the transpose builds its index (transpose_mark, row_prefix, the bitmap rank of
// transpose_fill): list[2 t] = position of the source block in the matrix' index, list[2 t + 1] = its block row.  One wavefront per source block row.
__global__ void __launch_bounds__(256) algebra_col_list(const int* __restrict__ row_p, const int* __restrict__ col_i, int nbr, int Wt,
                                                        const uint32_t* __restrict__ t_bm, const int* __restrict__ t_pre, const int* __restrict__ col_p,
                                                        int* __restrict__ list) {
  const int lane = threadIdx.x & 63;
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= nbr) return;
  for (int b = row_p[r] + lane; b < row_p[r + 1]; b += 64) {
    const size_t w = (size_t)col_i[b] * Wt + (r >> 5);
    const int t = col_p[col_i[b]] + t_pre[w] + __popc(t_bm[w] & ((1u << (r & 31)) - 1u));
    list[2 * (size_t)t] = b;
    list[2 * (size_t)t + 1] = r;
  }
}

// len <= kStageElems elements at d (element `off` of a 16-byte aligned area) -> f of them in lds[0 ... len), with aligned 16-byte loads where vec_ok
template <typename T>
__device__ __forceinline__ void stage_absval(const T* __restrict__ d, int64_t off, int len, int lane, int vec_ok, int what, double* lds) {
  walk_block_values(d, off, len, lane, 64, vec_ok, [&](int e, T x) { lds[e] = absval_of(x, what); });
}

// the same loads, f summed per lane in a register (the lab build's ablation of the column sums without LDS)
template <typename T>
__device__ __forceinline__ double sum_absval(const T* __restrict__ d, int64_t off, int len, int lane, int vec_ok, int what) {
  double s = 0.0;
  walk_block_values(d, off, len, lane, 64, vec_ok, [&](int, T x) { s += absval_of(x, what); });
  return s;
}

// What the column passes share (algebra_col_sums, algebra_matvec_cols): the staged piece holds the elements c0 ... c0 + len - 1 of the part, the lane's run
// is run0 ... run0 + m - 1.  A lane that owns a column adds what the piece holds of its run, starting at element lane mod (that count) of it and wrapping
template <typename Acc>
__device__ __forceinline__ void add_run_rotated(const Acc* lds, int c0, int len, int run0, int m, int lane, bool owns, Acc& acc) {
  const int lo = run0 > c0 ? run0 : c0, hi = run0 + m < c0 + len ? run0 + m : c0 + len;
  if (owns && lo < hi) {
    const int cnt = hi - lo;
    const Acc* run = lds + (lo - c0);
    int i = lane % cnt;
    for (int k = 0; k < cnt; ++k) {
      acc = acc + run[i];
      if (++i == cnt) i = 0;
    }
  }
}

// sum_i f(a_ij) per full column: S waves per block column walk its list (wave sub takes the entries sub, sub + S, ...); a block is one contiguous piece of
// memory, column j of it the run j m ... j m + m - 1.  Lane j owns column j (64 columns at a time: of a wider block the wave reads, per pass, only the
// part that holds its 64 columns, so every element is still read once).  A piece of up to kStageElems elements is loaded with coalesced 16-byte accesses,
// f of it staged in the wave's LDS slice, and lane j adds what the piece holds of its run -- starting at element j mod (run length) of it and wrapping, so
// that lanes whose runs lie a multiple of the bank count apart do not meet in one bank; the order is fixed all the same.  skip_diag: blocks on the block
// diagonal do not count (the twin part of the Gershgorin sum of a stored triangle).
// VARIANT 0 is what ships.  The others exist in the lab build only (DBCSR_AMD_ALG_COLSUMS, profiles/matrix_norms.txt): 1 stages a piece and reads one value
// of it per lane (no add loop), 2 loads and adds in registers as algebra_norm2 does (no LDS), 3 walks no block at all (the list build, the launch and the sum
// of the partial vectors remain) -- ablations, their results are not column sums --, 4 is the lane-per-column form without staging: lane j reads its run
// from global memory element by element (a correct result, measured against 0).
template <typename T, int VARIANT = 0>
__global__ void __launch_bounds__(256)
algebra_col_sums(const int* __restrict__ col_p, const int* __restrict__ list, const int64_t* __restrict__ blk_p, const T* __restrict__ data,
                 const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ coff, int nbc, int S, int what, int skip_diag,
                 int vec_ok, int64_t n_out, double* __restrict__ partials) {
  __shared__ double stage[4][kStageElems];
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int c = (int)(wv / S), sub = (int)(wv % S);
  if (c >= nbc) return;
  const int n = cs[c];
  const int64_t base = coff[c];
  double* __restrict__ mine = partials + (size_t)sub * n_out;
  double* lds = stage[threadIdx.x >> 6];
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int nj = n - j0 < 64 ? n - j0 : 64;
    double acc = 0.0;
    for (int t = col_p[c] + sub; t < col_p[c + 1]; t += S) {
      const int r = list[2 * (size_t)t + 1];
      if (skip_diag && r == c) continue;
      const int m = rs[r];
      const int64_t off = blk_p[list[2 * (size_t)t]] + (int64_t)j0 * m;
      const int total = nj * m, run0 = lane * m;   // the part of the block with this pass' columns; lane's run inside it
      if constexpr (VARIANT == 3) continue;
      if constexpr (VARIANT == 4) {
        if (lane < nj) {
          const T* run = data + off + run0;
          for (int i = 0; i < m; ++i) acc += absval_of(run[i], what);
        }
        continue;
      }
      for (int c0 = 0; c0 < total; c0 += kStageElems) {
        const int len = total - c0 < kStageElems ? total - c0 : kStageElems;
        if constexpr (VARIANT == 2) {
          acc += sum_absval(data + off + c0, off + c0, len, lane, vec_ok, what);
          continue;
        }
        stage_absval(data + off + c0, off + c0, len, lane, vec_ok, what, lds);
        wave_lds_handover();   // (the slice is this wave's alone)
        if constexpr (VARIANT == 1) {
          if (lane < len) acc += lds[lane];
        } else {
          add_run_rotated(lds, c0, len, run0, m, lane, lane < nj, acc);
        }
        wave_lds_handover();   // (the next piece overwrites the slice)
      }
    }
    if (lane < nj && base + j0 + lane < n_out) mine[base + j0 + lane] = acc;
  }
}

template <typename T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = max_or_nan(x, __shfl_down(x, off, 64));
  return x;  // (lane 0's is the maximum; NaN if any lane's is)
}

// max |x| over the blocks the index names (holes do not count): as algebra_norm2, one partial per wave.  Real data: |x| itself, exact; complex data:
// |x|^2, the root is taken once at the end (algebra_max_final).  A NaN among the elements comes out as NaN (max_or_nan), as it does of the sums
__device__ __forceinline__ double maxterm_of(double x) { return fabs(x); }
__device__ __forceinline__ double maxterm_of(float x) { return fabs((double)x); }
__device__ __forceinline__ double maxterm_of(z64 x) { return x.re * x.re + x.im * x.im; }

template <typename T>
__global__ void __launch_bounds__(256) algebra_maxabs(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                      const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S,
                                                      int vec_ok, double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  double acc = 0.0;
  for (int b = row_p[row] + sub; b < row_p[row + 1]; b += S) {
    const int ne = m * cs[col_i[b]];
    const int64_t off = blk_p[b];
    walk_block_values(data + off, off, ne, lane, 64, vec_ok, [&](int, T x) { acc = max_or_nan(acc, maxterm_of(x)); });
  }
  acc = wave_max(acc);
  if (lane == 0) partials[wv] = acc;
}

// one workgroup: *out = max_i (v[i] + w[i]) over n non-negative values (w == nullptr: v alone), its root with `root`; 0 for n == 0
__global__ void __launch_bounds__(256) algebra_max_final(const double* __restrict__ v, const double* __restrict__ w, int64_t n, int root,
                                                         double* __restrict__ out) {
  __shared__ double best[256];
  double x = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) x = max_or_nan(x, v[i] + (w ? w[i] : 0.0));
  best[threadIdx.x] = x;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) best[threadIdx.x] = max_or_nan(best[threadIdx.x], best[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = root ? sqrt(best[0]) : best[0];
}

// The diagonal as a vector of the full-row length: one wavefront per block row.  get: the diagonal elements of the diagonal block the row has, zero where
// it has none (or one that is not square: left alone, as diag_shift leaves it); one wavefront more writes zero behind the last row, so that every one of
// the n elements is written.  set: the other way, onto the diagonal blocks present; nothing else is written.  Reads and writes of the vector stay below n.
template <typename T>
__global__ void __launch_bounds__(256) diag_get(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs,
                                                const int64_t* __restrict__ roff, int nbr, T* __restrict__ out, int64_t n) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row > nbr) return;
  if (row == nbr) {
    for (int64_t i = roff[nbr] + lane; i < n; i += 64) out[i] = T(0);
    return;
  }
  const int at = find_diag_block(row_p, col_i, row, lane);
  const int m = rs[row];
  const bool have = at >= 0 && cs[row] == m;
  const T* d = data + (have ? blk_p[at] : 0);
  const int64_t base = roff[row];
  for (int e = lane; e < m; e += 64)
    if (base + e < n) out[base + e] = have ? d[(size_t)e * (m + 1)] : T(0);
}

template <typename T>
__global__ void __launch_bounds__(256) diag_set(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ roff, int nbr,
                                                const T* __restrict__ vec, int64_t n, T* __restrict__ data) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= nbr) return;
  const int at = find_diag_block(row_p, col_i, row, lane);
  if (at < 0) return;
  const int m = rs[row];
  if (cs[row] != m) return;   // (not a square block: never write outside the block)
  T* d = data + blk_p[at];
  const int64_t base = roff[row];
  for (int e = lane; e < m; e += 64)
    if (base + e < n) d[(size_t)e * (m + 1)] = vec[base + e];
}

// in place: a_ij <- a_ij * v[coff(c) + j] (side 1, right: `offs` = coff) or a_ij * v[roff(r) + i] (side 0, left: `offs` = roff).  By block row with S waves
// per row as algebra_add_blocks, lanes over the elements with aligned 16-byte accesses; the position inside the block comes from one division per access.
// An element whose entry of the vector would lie at n or behind stays as it is.
template <typename T>
__global__ void __launch_bounds__(256)
algebra_scale_by_vector(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const int* __restrict__ rs,
                        const int* __restrict__ cs, const int64_t* __restrict__ offs, int nbr, int S, int side, const T* __restrict__ vec, int64_t n,
                        T* __restrict__ data, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0) return;
  for (int t = row_p[row] + sub; t < row_p[row + 1]; t += S) {
    const int c = col_i[t], ne = m * cs[c];
    const int64_t off = blk_p[t], vb = side ? offs[c] : offs[row];
    T* d = data + off;
    auto one = [&](int e) {
      const int64_t idx = vb + (side ? e / m : e % m);
      if (idx < n) d[e] = d[e] * vec[idx];
    };
    walk_block<T>(off, ne, lane, 64, vec_ok, one, [&](int e) {
      int i = e % m, j = e / m;
      Pack16<T> x = *reinterpret_cast<Pack16<T>*>(d + e);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int64_t idx = vb + (side ? j : i);
        if (idx < n) x.v[u] = x.v[u] * vec[idx];
        if (++i == m) i = 0, ++j;
      }
      *reinterpret_cast<Pack16<T>*>(d + e) = x;
    });
  }
}

// ---- matrix-vector product (y <- alpha op(A) x + beta y) -----------------------------------------------------------------------------------------------
// The two passes above with the term g(a_e) x[...] in place of f(a_e) (g: identity or conjugate): algebra_matvec_rows is algebra_row_sums' walk with
// x taken per element COLUMN, algebra_matvec_cols is algebra_col_sums' with x taken per element ROW.  Sums are carried in double / complex double
// (MatvecAcc), one partial vector per wave of a block row / column; algebra_matvec_combine adds the partial vectors of both passes in a fixed order and
// applies alpha and beta.  Every read of x stays below n_x (a term whose entry of x would lie behind it is not formed), every write of y below n_y.
template <typename T> struct MatvecAcc { using type = double; };
template <> struct MatvecAcc<z64> { using type = z64; };

__device__ __forceinline__ double matvec_term(double a, double x, int) { return a * x; }
__device__ __forceinline__ double matvec_term(float a, float x, int) { return (double)a * (double)x; }   // (exact in double)
__device__ __forceinline__ z64 matvec_term(z64 a, z64 x, int conj) { return z64(a.re, conj ? -a.im : a.im) * x; }

// Row pass, the elements of one block through the lanes of a wave: the slots of row_sum_slots.  xc = x at the block column's first element, nx the number
// of entries x has from there.  Slot s starts at element e0 = V s - A = i + m j of the column-major block; a lane's stride V P is a multiple of m, so from
// one slot to the next i stays and j grows by q = V P / m: one division per block and lane.  x is read straight from global memory: a wave's 16-byte loads
// cover V P consecutive elements, that is q (23 x 23 doubles: 4) consecutive entries of x, one cache line that stays in L1 / L2 (x is small next to A) --
// and an entry is loaded again only where a slot crosses into the next column.
template <typename T, int A>
__device__ __forceinline__ void matvec_row_slots(const T* __restrict__ d, int ne, int m, int lane, int P, int vec_ok, int conj, const T* __restrict__ xc,
                                                 int64_t nx, typename MatvecAcc<T>::type (&acc)[2 * Pack16<T>::V - 1]) {
  constexpr int V = Pack16<T>::V;
  const int nslots = (ne + A + V - 1) / V, q = V * P / m;
  int e0 = V * lane - A;
  int j = e0 >= 0 ? e0 / m : -((-e0 + m - 1) / m);   // (floor: the slot in front of the block's first element)
  const int i = e0 - j * m;
  for (int s = lane; s < nslots; s += P, e0 += V * P, j += q) {
    int iu = i, ju = j;
    bool ok = ju >= 0 && ju < nx;
    T xv = ok ? xc[ju] : T(0);
    auto next = [&]() {
      if (++iu == m) {
        iu = 0, ++ju;
        ok = ju >= 0 && ju < nx;
        xv = ok ? xc[ju] : T(0);
      }
    };
    if (vec_ok && e0 >= 0 && e0 + V <= ne) {
      const Pack16<T> a = *reinterpret_cast<const Pack16<T>*>(d + e0);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        if (ok) acc[V - 1 - A + u] = acc[V - 1 - A + u] + matvec_term(a.v[u], xv, conj);
        if (u + 1 < V) next();
      }
    } else {
#pragma unroll
      for (int u = 0; u < V; ++u) {
        if (e0 + u >= 0 && e0 + u < ne && ok) acc[V - 1 - A + u] = acc[V - 1 - A + u] + matvec_term(d[e0 + u], xv, conj);
        if (u + 1 < V) next();
      }
    }
  }
}

// partials[sub * n_y + yoff[row] + r] = sum over the blocks sub, sub + S, ... of block row `row` of sum_j g(a_rj) x[xoff[c] + j], for every element row r of
// the block row (zero when the wave met no block): algebra_row_sums with another term.  skip_diag: blocks on the block diagonal do not count (the twin part
// of the transposed product of a stored triangle).
template <typename T>
__global__ void __launch_bounds__(256)
algebra_matvec_rows(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const T* __restrict__ data,
                    const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ yoff, const int64_t* __restrict__ xoff, int nbr, int S,
                    int conj, int skip_diag, int vec_ok, const T* __restrict__ x, int64_t n_x, int64_t n_y,
                    typename MatvecAcc<T>::type* __restrict__ partials) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr int V = Pack16<T>::V, K = 2 * V - 1;
  __shared__ Acc red[4][K * 64];
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  if (m <= 0) return;
  const int64_t base = yoff[row];
  Acc* __restrict__ mine = partials + (size_t)sub * n_y;
  const int b0 = row_p[row] + sub, b1 = row_p[row + 1];
  const RowSlots sl = row_slots_of<V>(m);
  if (sl.p > 64) {
    for (int r0 = 0; r0 < m; r0 += 64) {
      const int r = r0 + lane;
      Acc acc = Acc(0.0);
      if (r < m)
        for (int b = b0; b < b1; b += S) {
          const int c = col_i[b];
          if (skip_diag && c == row) continue;
          const int n = cs[c];
          const T* d = data + blk_p[b] + r;
          const int64_t xb = xoff[c];
          for (int j = 0; j < n; ++j)
            if (xb + j < n_x) acc = acc + matvec_term(d[(size_t)m * j], x[xb + j], conj);
        }
      if (r < m && base + r < n_y) mine[base + r] = acc;
    }
    return;
  }
  Acc acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = Acc(0.0);
  if (lane < sl.P)
    for (int b = b0; b < b1; b += S) {
      const int c = col_i[b];
      if (skip_diag && c == row) continue;   // (wave-uniform)
      const int ne = m * cs[c];
      const int64_t off = blk_p[b], xb = xoff[c];
      const T* d = data + off;
      const T* xc = x + xb;
      const int64_t nx = n_x - xb;
      const int a = vec_ok ? (int)(off & (V - 1)) : 0;   // (wave-uniform)
      DBCSR_AMD_BY_SHIFT(matvec_row_slots, a, d, ne, m, lane, sl.P, vec_ok, conj, xc, nx, acc);
    }
  row_handover<V>(acc, red[threadIdx.x >> 6], lane, m, sl, [&](int r, Acc sum) {
    if (base + r < n_y) mine[base + r] = sum;
  });
}

// elements of a staged piece: a workgroup's four slices stay within the 32 KB of kStageElems doubles per wave (a complex term is two doubles)
template <typename T>
constexpr int kMatvecPiece = kStageElems * (int)sizeof(double) / (int)sizeof(typename MatvecAcc<T>::type);

// len <= kMatvecPiece elements at d (element `off` of a 16-byte aligned area; element `first` of a part of a column-major block that starts with a whole
// column of m elements) -> g(a_e) x[row of e] of them in lds[0 ... len), with aligned 16-byte loads where vec_ok: stage_absval with another term.  xr = x
// at the block row's first element, nx the number of entries x has from there (zero is staged for a term that is not formed)
template <typename T>
__device__ __forceinline__ void stage_matvec(const T* __restrict__ d, int64_t off, int len, int first, int m, int lane, int vec_ok, int conj,
                                             const T* __restrict__ xr, int64_t nx, typename MatvecAcc<T>::type* lds) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr int V = Pack16<T>::V;
  auto one = [&](int e) {
    const int i = (first + e) % m;
    lds[e] = i < nx ? matvec_term(d[e], xr[i], conj) : Acc(0.0);
  };
  walk_block<T>(off, len, lane, 64, vec_ok, one, [&](int e) {
    const Pack16<T> a = *reinterpret_cast<const Pack16<T>*>(d + e);
    int i = (first + e) % m;
#pragma unroll
    for (int u = 0; u < V; ++u) {
      lds[e + u] = i < nx ? matvec_term(a.v[u], xr[i], conj) : Acc(0.0);
      if (++i == m) i = 0;
    }
  });
}

// partials[sub * n_y + yoff[c] + j] = sum over the entries sub, sub + S, ... of block column c's list of sum_i g(a_ij) x[xoff[r] + i]: the staged form of
// algebra_col_sums with another term (lane j owns column j, 64 columns at a time; a piece is staged in the wave's LDS slice and lane j adds what the piece
// holds of its run in the rotated, fixed order).  skip_diag: blocks on the block diagonal do not count (the twin part of the product of a stored triangle).
template <typename T>
__global__ void __launch_bounds__(256)
algebra_matvec_cols(const int* __restrict__ col_p, const int* __restrict__ list, const int64_t* __restrict__ blk_p, const T* __restrict__ data,
                    const int* __restrict__ rs, const int* __restrict__ cs, const int64_t* __restrict__ yoff, const int64_t* __restrict__ xoff, int nbc, int S,
                    int conj, int skip_diag, int vec_ok, const T* __restrict__ x, int64_t n_x, int64_t n_y,
                    typename MatvecAcc<T>::type* __restrict__ partials) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr int kPiece = kMatvecPiece<T>;
  __shared__ Acc stage[4][kPiece];
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int c = (int)(wv / S), sub = (int)(wv % S);
  if (c >= nbc) return;
  const int n = cs[c];
  const int64_t base = yoff[c];
  Acc* __restrict__ mine = partials + (size_t)sub * n_y;
  Acc* lds = stage[threadIdx.x >> 6];
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int nj = n - j0 < 64 ? n - j0 : 64;
    Acc acc = Acc(0.0);
    for (int t = col_p[c] + sub; t < col_p[c + 1]; t += S) {
      const int r = list[2 * (size_t)t + 1];
      if (skip_diag && r == c) continue;
      const int m = rs[r];
      if (m <= 0) continue;
      const int64_t off = blk_p[list[2 * (size_t)t]] + (int64_t)j0 * m, xb = xoff[r];
      const int total = nj * m, run0 = lane * m;   // the part of the block with this pass' columns; lane's run inside it
      for (int c0 = 0; c0 < total; c0 += kPiece) {
        const int len = total - c0 < kPiece ? total - c0 : kPiece;
        stage_matvec(data + off + c0, off + c0, len, c0, m, lane, vec_ok, conj, x + xb, n_x - xb, lds);
        wave_lds_handover();   // (the slice is this wave's alone)
        add_run_rotated(lds, c0, len, run0, m, lane, lane < nj, acc);
        wave_lds_handover();   // (the next piece overwrites the slice)
      }
    }
    if (lane < nj && base + j0 + lane < n_y) mine[base + j0 + lane] = acc;
  }
}

// beta * y in the data's own precision, every operation rounded on its own: what alpha == 0 leaves of the product.  (The library is compiled with
// contraction into fused multiply-adds allowed; the pragma takes it from the complex product, whose bits would otherwise depend on the compiler.)
__device__ __forceinline__ double matvec_scaled(double b, double y) { return b * y; }
__device__ __forceinline__ float matvec_scaled(float b, float y) { return b * y; }
__device__ __forceinline__ z64 matvec_scaled(z64 b, z64 y) {
#pragma clang fp contract(off)
  const double rr = b.re * y.re, ii = b.im * y.im, ri = b.re * y.im, ir = b.im * y.re;
  return z64(rr - ii, ri + ir);
}
__device__ __forceinline__ double matvec_signed(double v, double sign) { return sign * v; }
__device__ __forceinline__ z64 matvec_signed(z64 v, double sign) { return z64(sign * v.re, sign * v.im); }
__device__ __forceinline__ double matvec_wide(double v) { return v; }
__device__ __forceinline__ double matvec_wide(float v) { return (double)v; }
__device__ __forceinline__ z64 matvec_wide(z64 v) { return v; }
template <typename T> __device__ __forceinline__ T matvec_narrow(typename MatvecAcc<T>::type v) { return (T)v; }
template <> __device__ __forceinline__ z64 matvec_narrow<z64>(z64 v) { return v; }

// bits of `mode`: alpha == 0 (no pass ran: y <- beta y in the data's precision, S_r = S_c = 0), beta == 0 (y is not read)
constexpr int kMatvecNoProduct = 1, kMatvecBetaZero = 2;

// y[i] = alpha (row_sign * sum_k row partial k + col_sign * sum_k column partial k) + beta y[i] for i below n_y and below *total (the full length, on the
// device): the partial vectors in the order rows 0 ... S_r - 1, then columns 0 ... S_c - 1 (the column partials lie behind the row partials; a sign of +-1 is
// exact), alpha and beta applied in double, one rounding to the data's type.  Nothing else is written.
template <typename T>
__global__ void __launch_bounds__(256)
algebra_matvec_combine(const typename MatvecAcc<T>::type* __restrict__ partials, int S_r, int S_c, double row_sign, double col_sign, int64_t n_y,
                       const int64_t* __restrict__ total, typename MatvecAcc<T>::type alpha, typename MatvecAcc<T>::type beta, int mode, T* __restrict__ y) {
  using Acc = typename MatvecAcc<T>::type;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_y || i >= *total) return;
  if (mode & kMatvecNoProduct) {
    y[i] = (mode & kMatvecBetaZero) ? T(0) : matvec_scaled(matvec_narrow<T>(beta), y[i]);
    return;
  }
  Acc s = Acc(0.0);
  for (int k = 0; k < S_r; ++k) s = s + matvec_signed(partials[(size_t)k * n_y + i], row_sign);
  for (int k = 0; k < S_c; ++k) s = s + matvec_signed(partials[(size_t)(S_r + k) * n_y + i], col_sign);
  Acc r = alpha * s;
  if (!(mode & kMatvecBetaZero)) r = r + beta * matvec_wide(y[i]);
  y[i] = matvec_narrow<T>(r);
}

#undef DBCSR_AMD_BY_SHIFT

}  // namespace dbcsr_amd
#endif
