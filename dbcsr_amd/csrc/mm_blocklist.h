// mm_blocklist.h -- a matrix built and edited through a coordinate list of blocks (src/block/dbcsr_block_access.F: dbcsr_reserve_blocks, dbcsr_put_block
// with summation and scale, dbcsr_get_block_p; the merge of the work matrices in dbcsr_finalize): entry i of a list names block (rows[i], cols[i]), in any
// order, duplicates allowed, and for put and get a window of a flat tensor at an element offset of its own.
// Part of the device-resident multiply engine: included by mm_engine.hip after mm_elementwise.h, whose conventions hold here -- every kernel goes by the
// index (row_p, col_i, blk_p), never by the extent of a data area, the block columns of a block row ascend (find_block), 64-bit offsets, no atomics on
// data and no floating-point atomics at all, no LDS, and a lane loads all it needs of an element before it stores it.
//
// reserve: blocklist_mark sets the bit of every listed block the matrix lacks in a bitmap of the feature's own (an integer atomicOr: idempotent, so
// order and duplicates do not matter; the lane that finds the bit clear counts the block and its size), blocklist_named_nze adds up the sizes of the
// blocks the matrix names.  From there the union add's kernels form the pattern and elementwise_copy_onto fills it.
// put: blocklist_locate finds every entry's block and counts the entries per block, exclusive_scan turns the counts into segments, blocklist_slot drops
// the entry numbers into their block's segment, blocklist_order puts every segment into ascending entry order, blocklist_put walks the touched blocks
// and applies each block's segment in that order.  The integer atomics count and hand out slots; what they decide is put right by the ordering pass, so
// the result is the same bits on every call.
// get: blocklist_get, one kernel, a wave per entry.
#ifndef DBCSR_AMD_MM_BLOCKLIST_H
#define DBCSR_AMD_MM_BLOCKLIST_H
#include "mm_elementwise.h"

namespace dbcsr_amd {

// counters[] of blocklist_mark / blocklist_named_nze
constexpr int kListNew = 0, kListInvalid = 1, kListNewNze = 2, kListNamedNze = 3;

// is (r, c) a block the matrix can store?  upper_only: a matrix with symmetry stores the triangle c >= r
__device__ __forceinline__ bool block_in_range(int r, int c, int nbr, int nbc, int upper_only) {
  return r >= 0 && r < nbr && c >= 0 && c < nbc && !(upper_only && c < r);
}

// ---- reserve --------------------------------------------------------------------------------------------------------------------------------------------
// A lane per list entry.  An entry outside the matrix (or below the diagonal with upper_only) is counted in counters[kListInvalid] and does nothing else.
// An entry whose block the matrix lacks sets bit (r, c) of bm[nbr][W]; the ONE lane that finds it clear adds 1 to counters[kListNew] and the block's
// element count to counters[kListNewNze].  Sums of integers: the same in any order.  A row_p entry outside [0, nblks] is clamped.
__global__ void __launch_bounds__(256)
blocklist_mark(const int* __restrict__ row_p, const int* __restrict__ col_i, const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int nbc,
               int W, int64_t nblks, const int* __restrict__ rows, const int* __restrict__ cols, int64_t n, int upper_only, uint32_t* __restrict__ bm,
               unsigned long long* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = rows[i], c = cols[i];
  if (!block_in_range(r, c, nbr, nbc, upper_only)) {
    atomicAdd(counters + kListInvalid, 1ull);
    return;
  }
  if (find_block(col_i, clamped(row_p[r], nblks), clamped(row_p[r + 1], nblks), c) >= 0) return;
  const uint32_t bit = 1u << (c & 31);
  if (atomicOr(&bm[(size_t)r * W + (c >> 5)], bit) & bit) return;   // (an earlier entry named the block)
  atomicAdd(counters + kListNew, 1ull);
  atomicAdd(counters + kListNewNze, (unsigned long long)((int64_t)rs[r] * cs[c]));
}

// One wavefront per block row: counters[kListNamedNze] += the element counts of the blocks the index names (what a packed copy of them holds).
__global__ void __launch_bounds__(256)
blocklist_named_nze(const int* __restrict__ row_p, const int* __restrict__ col_i, const int* __restrict__ rs, const int* __restrict__ cs, int nbr,
                    int64_t nblks, unsigned long long* __restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= nbr) return;
  const int b0 = clamped(row_p[row], nblks), b1 = clamped(row_p[row + 1], nblks);
  int64_t cols_sum = 0;
  for (int b = b0 + lane; b < b1; b += 64) cols_sum += cs[col_i[b]];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cols_sum += __shfl_down(cols_sum, off, 64);
  if (lane == 0 && cols_sum) atomicAdd(counters + kListNamedNze, (unsigned long long)(cols_sum * rs[row]));
}

// ---- put ------------------------------------------------------------------------------------------------------------------------------------------------
// (a) A lane per list entry: hit[i] = the position of block (rows[i], cols[i]) in the index, -1 where the matrix stores no such block or the coordinate
// is outside it; cnt[position] += 1 (the caller zeroed cnt).
__global__ void __launch_bounds__(256)
blocklist_locate(const int* __restrict__ row_p, const int* __restrict__ col_i, int nbr, int nbc, int64_t nblks, const int* __restrict__ rows,
                 const int* __restrict__ cols, int64_t n, int* __restrict__ hit, int* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = rows[i], c = cols[i];
  int p = -1;
  if (block_in_range(r, c, nbr, nbc, 0)) p = find_block(col_i, clamped(row_p[r], nblks), clamped(row_p[r + 1], nblks), c);
  hit[i] = p;
  if (p >= 0) atomicAdd(cnt + p, 1);
}

// (b) A lane per list entry: entry i takes one of the cnt[hit[i]] places of its block's segment seg[hit[i]] ... seg[hit[i] + 1) of `slots` (cnt counts
// down: which place an entry gets depends on the order the lanes arrive in -- blocklist_order removes that).
__global__ void __launch_bounds__(256)
blocklist_slot(const int* __restrict__ hit, const int* __restrict__ seg, int64_t n, int* __restrict__ cnt, int* __restrict__ slots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = hit[i];
  if (p >= 0) slots[seg[p] + atomicAdd(cnt + p, -1) - 1] = (int)i;
}

// One wavefront per 64 blocks of the index, a lane per block: order[seg[b] ... seg[b + 1]) = the entry numbers of slots[] in ascending order.  A segment
// of one entry -- almost all of them -- is copied by its lane.  A longer one, of any length, is ranked by the whole wave: the lanes take its entries 64 at
// a time, and the rank of an entry is the number of entries of the segment below it (the numbers of a segment differ).  Nothing is written outside a
// segment; a segment that does not lie inside [0, n] is left alone.
__global__ void __launch_bounds__(256)
blocklist_order(const int* __restrict__ seg, const int* __restrict__ slots, int64_t nblks, int64_t n, int* __restrict__ order) {
  const int lane = threadIdx.x & 63;
  const int64_t base = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64;
  if (base >= nblks) return;
  const int64_t b = base + lane;
  int s0 = 0, s1 = 0;
  if (b < nblks) {
    s0 = seg[b], s1 = seg[b + 1];
    if (s0 < 0 || s1 > n || s1 < s0) s1 = s0 = 0;
  }
  if (s1 - s0 == 1) order[s0] = slots[s0];
  unsigned long long longer = __ballot(s1 - s0 > 1);
  while (longer) {   // (wave-uniform)
    const int src = __ffsll((long long)longer) - 1;
    longer &= longer - 1;
    const int t0 = __shfl(s0, src, 64), t1 = __shfl(s1, src, 64);
    for (int k = t0 + lane; k < t1; k += 64) {
      const int mine = slots[k];
      int rank = 0;
      for (int j = t0; j < t1; ++j) rank += slots[j] < mine ? 1 : 0;
      order[t0 + rank] = mine;
    }
  }
}

// what a contribution adds: alpha * x, or x itself where alpha is exactly 1 (nothing is multiplied: bit for bit)
template <typename T>
__device__ __forceinline__ T put_term(T x, T alpha, int alpha_is_one) { return alpha_is_one ? x : alpha * x; }

// (c) The blocks of the index whose segment is not empty, by block row with S waves per row as algebra_add_blocks, lanes over the elements with
// walk_block aligned on the block that is written; entry k's window src + src_off[k] is read through Pack16U from wherever it starts.  The segment runs
// in ascending entry order: with summation v = old, then v = v + alpha x_k for every entry; without it v = alpha x of the LAST entry (the others are not
// read).  Blocks without an entry, holes and every index array are not touched.  The windows do not overlap the matrix' data area (the host's contract).
template <typename T>
__global__ void __launch_bounds__(256)
blocklist_put(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const int* __restrict__ rs,
              const int* __restrict__ cs, int nbr, int S, int64_t nblks, const int* __restrict__ seg, const int* __restrict__ order,
              const int64_t* __restrict__ src_off, const T* __restrict__ src, T alpha, int alpha_is_one, int summation, T* __restrict__ data, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int lane = threadIdx.x & 63;
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int row = (int)(wv / S), sub = (int)(wv % S);
  if (row >= nbr) return;
  const int m = rs[row];
  const int b1 = clamped(row_p[row + 1], nblks);
  for (int t = clamped(row_p[row], nblks) + sub; t < b1; t += S) {
    const int s1 = seg[t + 1];
    const int s0 = summation ? seg[t] : s1 - 1;   // (wave-uniform; an overwrite: the last entry alone)
    if (s1 <= seg[t]) continue;
    const int ne = m * cs[col_i[t]];
    const int64_t dof = blk_p[t];
    T* d = data + dof;
    auto one = [&](int e) {
      if (summation) {
        T v = d[e];
        for (int k = s0; k < s1; ++k) v = v + put_term(src[src_off[order[k]] + e], alpha, alpha_is_one);
        d[e] = v;
      } else {
        d[e] = put_term(src[src_off[order[s0]] + e], alpha, alpha_is_one);
      }
    };
    walk_block<T>(dof, ne, lane, 64, vec_ok, one, [&](int e) {   // (aligned on the matrix' block)
      Pack16<T> r;
      if (summation) {
        r = *reinterpret_cast<const Pack16<T>*>(d + e);
        for (int k = s0; k < s1; ++k) {
          const Pack16U<T> x = *reinterpret_cast<const Pack16U<T>*>(src + src_off[order[k]] + e);
#pragma unroll
          for (int u = 0; u < V; ++u) r.v[u] = r.v[u] + put_term(x.v[u], alpha, alpha_is_one);
        }
      } else {
        const Pack16U<T> x = *reinterpret_cast<const Pack16U<T>*>(src + src_off[order[s0]] + e);
#pragma unroll
        for (int u = 0; u < V; ++u) r.v[u] = put_term(x.v[u], alpha, alpha_is_one);
      }
      *reinterpret_cast<Pack16<T>*>(d + e) = r;
    });
  }
}

// ---- get ------------------------------------------------------------------------------------------------------------------------------------------------
// A wave per list entry: the window dst + dst_off[i] of rs[r] * cs[c] elements = block (r, c) bit for bit and found[i] = 1, or +0.0 and found[i] = 0 where
// the matrix stores no such block.  An entry outside the matrix has no window: nothing but found[i] = 0 is written.  The block is found by a
// wave-uniform binary search; the walk is aligned on the window, the block is read through Pack16U from wherever it starts.  Every element of a window
// is written exactly once, nothing outside the windows.
template <typename T>
__global__ void __launch_bounds__(256)
blocklist_get(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, const T* __restrict__ data,
              const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int nbc, int64_t nblks, const int* __restrict__ rows,
              const int* __restrict__ cols, const int64_t* __restrict__ dst_off, int64_t n, T* __restrict__ dst, int* __restrict__ found, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int lane = threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (i >= n) return;
  const int r = rows[i], c = cols[i];
  if (!block_in_range(r, c, nbr, nbc, 0)) {   // (wave-uniform)
    if (lane == 0) found[i] = 0;
    return;
  }
  const int p = find_block(col_i, clamped(row_p[r], nblks), clamped(row_p[r + 1], nblks), c);
  if (lane == 0) found[i] = p >= 0 ? 1 : 0;
  const int ne = rs[r] * cs[c];
  const int64_t dof = dst_off[i];
  const T* s = data + (p >= 0 ? blk_p[p] : 0);
  T* d = dst + dof;
  auto one = [&](int e) { d[e] = p >= 0 ? s[e] : T(0.0); };
  walk_block<T>(dof, ne, lane, 64, vec_ok, one, [&](int e) {   // (aligned on the window)
    Pack16<T> x;
    if (p >= 0) {
      const Pack16U<T> y = *reinterpret_cast<const Pack16U<T>*>(s + e);
#pragma unroll
      for (int u = 0; u < V; ++u) x.v[u] = y.v[u];
    } else {
#pragma unroll
      for (int u = 0; u < V; ++u) x.v[u] = T(0.0);
    }
    *reinterpret_cast<Pack16<T>*>(d + e) = x;
  });
}

}  // namespace dbcsr_amd
#endif
