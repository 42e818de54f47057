// mm_elementwise.h -- element-wise operations on two patterns (src/ops/dbcsr_operations.F: dbcsr_hadamard_product, dbcsr_copy with keep_sparsity,
// dbcsr_function_of_elements): a kernel walks the blocks of one matrix and finds the same block in another matrix with another pattern.
// Part of the device-resident multiply engine: included by mm_engine.hip after mm_algebra.h, whose conventions hold here -- every kernel goes by the index
// (row_p, col_i, blk_p), never by the extent of a data area, and the block columns of a block row ascend (the ASSUMPTION at the head of mm_algebra.h), so
// the partner of a block is found by a binary search of the other matrix' row, as algebra_dot finds it.
//
// The result of an intersection is a subset of A's blocks: no bitmap, no work area of the symbolic phase.  elementwise_match marks A's blocks and counts
// the kept ones per row, exclusive_scan turns the counts into row_p and the kept blocks' sizes into data offsets, elementwise_emit writes col_i, blk_p and
// the two source offsets per result block, elementwise_mul_blocks multiplies.  With A's index in B (algebra_compare) elementwise_mul_flat does it in one
// flat pass, in place if asked.  elementwise_copy_onto searches from the destination's side inside the kernel that copies; elementwise_function works on
// one matrix in place.  The numeric kernels stream memory as the add's do: walk_block aligned on the block that is written, the other source through
// Pack16U from wherever it starts, 64-bit offsets, no atomics on data, no LDS, and a lane loads all it needs of an element before it stores it.
#ifndef DBCSR_AMD_MM_ELEMENTWISE_H
#define DBCSR_AMD_MM_ELEMENTWISE_H
#include "mm_algebra.h"

namespace dbcsr_amd {

// partner[b] of a block of A: B's block position (>= 0), or one of these
constexpr int kPartnerNone = -1, kPartnerAssumed = -2;

// position of the block with column c among the positions [q0, q1) of col_i (ascending columns), or -1
__device__ __forceinline__ int find_block(const int* __restrict__ col_i, int q0, int q1, int c) {
  int lo = q0, hi = q1;   // first position with a column >= c
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (col_i[mid] < c) lo = mid + 1; else hi = mid;
  }
  return (lo < q1 && col_i[lo] == c) ? lo : -1;
}

__device__ __forceinline__ int clamped(int x, int64_t n) { return x < 0 ? 0 : (x > n ? (int)n : x); }

// ---- the pattern of the product -----------------------------------------------------------------------------------------------------------------------
// S waves per block row of A, a lane per block of A (wave sub takes the blocks sub 64 ... sub 64 + 63, then S 64 further): partner[b] = the position of
// the same block in B, kPartnerNone, or kPartnerAssumed where B lacks it and counts as filled with a value; blk_nze[b] = the block's element count when
// it is kept, 0 otherwise; row_cnt[row] += the kept blocks the wave met, by ballot and popcount (the caller zeroed row_cnt: the waves of a row add their
// counts).  A row_p entry outside [0, nblks] is clamped: nothing is read outside the index arrays.
__global__ void __launch_bounds__(256)
elementwise_match(const int* __restrict__ a_row_p, const int* __restrict__ a_col_i, const int* __restrict__ b_row_p, const int* __restrict__ b_col_i,
                  const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S, int64_t na, int64_t nb, int b_assumed, int* __restrict__ partner,
                  int* __restrict__ blk_nze, int* __restrict__ row_cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int b0 = clamped(a_row_p[row], na), b1 = clamped(a_row_p[row + 1], na);
  const int q0 = clamped(b_row_p[row], nb), q1 = clamped(b_row_p[row + 1], nb);
  const int m = rs[row];
  int kept = 0;
  for (int base = b0 + sub * 64; base < b1; base += S * 64) {   // (wave-uniform: every lane takes part in the ballot)
    const int b = base + lane;
    int p = kPartnerNone;
    if (b < b1) {
      const int c = a_col_i[b];
      p = find_block(b_col_i, q0, q1, c);
      if (p < 0) p = b_assumed ? kPartnerAssumed : kPartnerNone;
      partner[b] = p;
      blk_nze[b] = p != kPartnerNone ? m * cs[c] : 0;
    }
    kept += __popcll(__ballot(p != kPartnerNone));
  }
  if (lane == 0 && kept) atomicAdd(row_cnt + row, kept);   // (a count, not data: the sum is the same in any order)
}

// One wave per block row of A, 64 blocks at a time: kept block b is result block t = c_row_p[row] + (kept blocks of the row in front of it) -- the rank
// by ballot and popcount again --, c_col_i[t] its column, c_blk_p[t] = off[b] (the scan of blk_nze), src[2 t] = its offset in A's data area,
// src[2 t + 1] = its partner's offset in B's, -1 where B's block is assumed.  Nothing is written at or behind result block nres.
__global__ void __launch_bounds__(256)
elementwise_emit(const int* __restrict__ a_row_p, const int* __restrict__ a_col_i, const int64_t* __restrict__ a_blk_p, const int64_t* __restrict__ b_blk_p,
                 const int* __restrict__ partner, const int64_t* __restrict__ off, const int* __restrict__ c_row_p, int nbr, int64_t na, int64_t nres,
                 int* __restrict__ c_col_i, int64_t* __restrict__ c_blk_p, int64_t* __restrict__ src) {
  const int lane = threadIdx.x & 63;
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= nbr) return;
  const int b0 = clamped(a_row_p[row], na), b1 = clamped(a_row_p[row + 1], na);
  int64_t t = c_row_p[row];
  for (int base = b0; base < b1; base += 64) {
    const int b = base + lane;
    const int p = b < b1 ? partner[b] : kPartnerNone;
    const unsigned long long keep = __ballot(p != kPartnerNone);
    const int64_t at = t + __popcll(keep & ((1ull << lane) - 1ull));
    if (p != kPartnerNone && at >= 0 && at < nres) {
      c_col_i[at] = a_col_i[b];
      c_blk_p[at] = off[b];
      src[2 * (size_t)at] = a_blk_p[b];
      src[2 * (size_t)at + 1] = p >= 0 ? b_blk_p[p] : -1;
    }
    t += __popcll(keep);
  }
}

// ---- the product ----------------------------------------------------------------------------------------------------------------------------------------
// dst block = a block * b block element by element, by block row with S waves per row as algebra_add_blocks (wave s takes the result blocks s mod S), lanes
// over the elements.  Where B's block is assumed (src[2 t + 1] < 0) it is a block * bval, and with a value that is exactly 1 A's block as it is, bit for
// bit.  Real data: one multiplication per element; complex data: re = ar br - ai bi, im = ar bi + ai br (z64's operator *).  dst aliases neither
// operand (the host refuses it).
template <typename T>
__global__ void __launch_bounds__(256)
elementwise_mul_blocks(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const int64_t* __restrict__ src,
                       const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S, const T* __restrict__ a_data, const T* __restrict__ b_data,
                       T* __restrict__ d_data, T bval, int bval_is_one, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  for (int t = row_p[row] + sub; t < row_p[row + 1]; t += S) {
    const int ne = m * cs[col_i[t]];
    const int64_t ao = src[2 * (size_t)t], bo = src[2 * (size_t)t + 1], dof = blk_p[t];
    const T* a = a_data + ao;
    const T* b = b_data + (bo >= 0 ? bo : 0);
    T* d = d_data + dof;
    const int how = bo >= 0 ? 0 : (bval_is_one ? 2 : 1);   // (wave-uniform) 0: a * b, 1: a * bval, 2: a
    auto one = [&](int e) { d[e] = how == 0 ? a[e] * b[e] : (how == 1 ? a[e] * bval : a[e]); };
    walk_block<T>(dof, ne, lane, 64, vec_ok, one, [&](int e) {   // (aligned on dst's block)
      Pack16<T> r;
      const Pack16U<T> x = *reinterpret_cast<const Pack16U<T>*>(a + e);
      if (how == 0) {
        const Pack16U<T> y = *reinterpret_cast<const Pack16U<T>*>(b + e);
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = x.v[u] * y.v[u];
      } else {
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = how == 1 ? x.v[u] * bval : x.v[u];
      }
      *reinterpret_cast<Pack16<T>*>(d + e) = r;
    });
  }
}

// Same pattern, same block offsets, A packed: one flat pass over the n elements of the data areas, dst[i] = a[i] * b[i], in the form of algebra_add_flat
// (one 16-byte access per operand and lane, no loop; the last n mod V elements one by one).  dst may be a or b: a lane loads its elements before it stores
// them, and nobody else touches them.
template <typename T>
__global__ void __launch_bounds__(256) elementwise_mul_flat(const T* a, const T* b, T* dst, int64_t n, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!vec_ok) {
    if (i < n) dst[i] = a[i] * b[i];
    return;
  }
  const int64_t nv = n / V;
  if (i < nv) {
    const Pack16<T> x = reinterpret_cast<const Pack16<T>*>(a)[i], y = reinterpret_cast<const Pack16<T>*>(b)[i];
    Pack16<T> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = x.v[k] * y.v[k];
    reinterpret_cast<Pack16<T>*>(dst)[i] = r;
  } else {
    const int64_t e = nv * V + (i - nv);
    if (e < n) dst[e] = a[e] * b[e];
  }
}

// ---- copy onto a pattern (dbcsr_copy, keep_sparsity) ---------------------------------------------------------------------------------------------------
// Every block the destination's index names = the source's block, bit for bit (values are moved, nothing is computed), or +0.0 where the source has
// none.  By block row of dst with S waves per row; the wave finds its block in the source's row itself (a wave-uniform binary search: no intermediate
// array, no count step).  Elements of dst's data area that its index does not name are not written.  The data areas do not overlap (the host checks).
template <typename T>
__global__ void __launch_bounds__(256)
elementwise_copy_onto(const int* __restrict__ s_row_p, const int* __restrict__ s_col_i, const int64_t* __restrict__ s_blk_p, const T* __restrict__ s_data,
                      const int* __restrict__ d_row_p, const int* __restrict__ d_col_i, const int64_t* __restrict__ d_blk_p, T* __restrict__ d_data,
                      const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S, int64_t ns, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  const int q0 = clamped(s_row_p[row], ns), q1 = clamped(s_row_p[row + 1], ns);
  for (int t = d_row_p[row] + sub; t < d_row_p[row + 1]; t += S) {
    const int c = d_col_i[t], ne = m * cs[c];
    const int p = find_block(s_col_i, q0, q1, c);   // (wave-uniform)
    const int64_t dof = d_blk_p[t];
    const T* s = s_data + (p >= 0 ? s_blk_p[p] : 0);
    T* d = d_data + dof;
    auto one = [&](int e) { d[e] = p >= 0 ? s[e] : T(0.0); };
    walk_block<T>(dof, ne, lane, 64, vec_ok, one, [&](int e) {   // (aligned on dst's block)
      Pack16<T> r;
      if (p >= 0) {
        const Pack16U<T> x = *reinterpret_cast<const Pack16U<T>*>(s + e);
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = x.v[u];
      } else {
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = T(0.0);
      }
      *reinterpret_cast<Pack16<T>*>(d + e) = r;
    });
  }
}

// ---- functions of elements (dbcsr_function_of_elements) -------------------------------------------------------------------------------------------------
// the function codes: dbcsr_func_* of include/dbcsr_amd_mm.h, the twelve functions whose definitions are beyond doubt (5, 6 and 14 are the three left out)
__host__ __device__ __forceinline__ bool function_known(int func) {
  return (func >= dbcsr_func_inverse && func <= dbcsr_func_artanh) || (func >= dbcsr_func_sin && func <= dbcsr_func_ddcos);
}

// f(y), y = a1 x + a0, in double, FUNC a compile-time constant.  1 - tanh^2 y is formed as 1 / cosh^2 y: the same function without the cancellation of
// the difference near |tanh y| = 1 (at y = 4 the difference loses ten bits).
template <int FUNC>
__device__ __forceinline__ double function_value(double x, double a0, double a1) {
  const double y = a1 * x + a0;
  if constexpr (FUNC == dbcsr_func_inverse) return 1.0 / y;
  else if constexpr (FUNC == dbcsr_func_tanh) return tanh(y);
  else if constexpr (FUNC == dbcsr_func_dtanh) { const double ch = cosh(y); return a1 / (ch * ch); }
  else if constexpr (FUNC == dbcsr_func_ddtanh) { const double ch = cosh(y); return -2.0 * a1 * a1 * tanh(y) / (ch * ch); }
  else if constexpr (FUNC == dbcsr_func_artanh) return atanh(y);
  else if constexpr (FUNC == dbcsr_func_sin) return sin(y);
  else if constexpr (FUNC == dbcsr_func_dsin) return a1 * cos(y);
  else if constexpr (FUNC == dbcsr_func_ddsin) return -(a1 * a1) * sin(y);
  else if constexpr (FUNC == dbcsr_func_asin) return asin(y);
  else if constexpr (FUNC == dbcsr_func_cos) return cos(y);
  else if constexpr (FUNC == dbcsr_func_dcos) return -a1 * sin(y);
  else return -(a1 * a1) * cos(y);   // dbcsr_func_ddcos
}

// the blocks sub, sub + S, ... of a block row through one function: aligned 16-byte loads and stores of the same elements (a lane loads a pack, applies f,
// stores it)
template <typename T, int FUNC>
__device__ __forceinline__ void function_of_row(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                const int* __restrict__ cs, int row, int sub, int S, int m, int lane, double a0, double a1,
                                                T* __restrict__ data, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  for (int t = row_p[row] + sub; t < row_p[row + 1]; t += S) {
    const int ne = m * cs[col_i[t]];
    const int64_t off = blk_p[t];
    T* d = data + off;
    auto one = [&](int e) { d[e] = (T)function_value<FUNC>((double)d[e], a0, a1); };
    walk_block<T>(off, ne, lane, 64, vec_ok, one, [&](int e) {
      Pack16<T> x = *reinterpret_cast<Pack16<T>*>(d + e);
#pragma unroll
      for (int u = 0; u < V; ++u) x.v[u] = (T)function_value<FUNC>((double)x.v[u], a0, a1);
      *reinterpret_cast<Pack16<T>*>(d + e) = x;
    });
  }
}

// in place on every element the index names: x <- f(a1 x + a0), formed in double and rounded once to the data's type.  By block row with S waves per
// row.  One kernel per data type: the function is chosen once per wave, outside the walk -- with the choice inside it (one switch per element) every
// element paid for the dispatch and the kernel held the registers of all twelve functions at once (129 against 3 waves per SIMD; tanh on config 2's
// product ran 7.90 ms against torch.tanh_'s 5.31, profiles/elementwise.txt).  The host refuses every code that is not one of the twelve.
template <typename T>
__global__ void __launch_bounds__(256)
elementwise_function(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const int* __restrict__ rs,
                     const int* __restrict__ cs, int nbr, int S, int func, double a0, double a1, T* __restrict__ data, int vec_ok) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
#define DBCSR_AMD_FUNCTION_CASE(F) \
  case F: function_of_row<T, F>(row_p, col_i, blk_p, cs, row, sub, S, m, lane, a0, a1, data, vec_ok); break
  switch (func) {   // (wave-uniform: a kernel argument)
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_inverse);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_tanh);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_dtanh);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_ddtanh);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_artanh);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_sin);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_dsin);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_ddsin);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_asin);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_cos);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_dcos);
    DBCSR_AMD_FUNCTION_CASE(dbcsr_func_ddcos);
    default: break;
  }
#undef DBCSR_AMD_FUNCTION_CASE
}

}  // namespace dbcsr_amd
#endif
