// mm_submatrix.h -- the data movement of the submatrix method on the device: dbcsr_amd_bcsr_submatrix_gather (submatrix_gather) and
// dbcsr_amd_bcsr_submatrix_scatter (submatrix_scatter).  Part of the device-resident multiply engine: included by mm_engine.hip after mm_dense.h, whose
// moves (dense_put_straight, dense_put_transposing, dense_take_transposing, dense_find) these kernels use behind one indirection.
//
// A submatrix g is an ascending set S_g of block rows of a square block structure: set_idx[set_ptr[g] ... set_ptr[g + 1]) are its members, set_off the
// element offset of each member inside the dense principal submatrix A[S_g, S_g] (the running sum of the members' block sizes), sub_dim[g] its side.  A
// batch holds one window of n x n elements per slot, row by row: element (i, j) of slot t at dense[t batch_stride + i ld + j], every offset in 64 bits.
//   submatrix_gather   tile (a, b) of slot t <- block (set_idx[a], set_idx[b]) of the matrix, found in row_p / col_i as dense_gather finds it: the stored
//                      block (through the LDS tile: its columns lie across the window's rows), else -- kind 0 ... 3 -- the twin of the block stored at the
//                      mirrored place (straight), else zeros.  Around the n_g x n_g submatrix the window is blockdiag(A[S, S], pad I): +0.0, and pad on
//                      the diagonal.  One workgroup per (slot, member row a, group of G member columns); the NG workgroups of a member row share the
//                      right-hand padding of its rows, the workgroups with a >= |S_g| share the bottom padding rows.  The grid has max_members + 1 member
//                      rows, so every slot has at least NG workgroups for its bottom rows.  Every element of the window is written exactly once.
//   submatrix_scatter  every stored block (R, C) whose block column has an owner g = owner[C] with a slot t = sub_slot[g] >= 0, and whose block row is a
//                      member of S_g (binary search in the ascending set), <- the window's elements at (set_off[pos R], set_off[pos C]) of slot t.  One
//                      workgroup per (block row, sub of S), as dense_scatter.  Nothing else is written.
// A plan that does not fit the matrix gives wrong values, never an access outside the window: a member whose index is outside the block structure or whose
// run set_off + size passes n is skipped whole, a submatrix id outside 0 ... nsub - 1 counts as an empty set.  No atomics, no scratch, no memset; the
// same bits on every call.
#ifndef DBCSR_AMD_MM_SUBMATRIX_H
#define DBCSR_AMD_MM_SUBMATRIX_H
#include "mm_dense.h"

namespace dbcsr_amd {

template <typename T> __host__ __device__ __forceinline__ T submatrix_pad(double pad) { return (T)pad; }
template <> __host__ __device__ __forceinline__ z64 submatrix_pad<z64>(double pad) { return z64(pad, 0.0); }

// position of block row r among the members [lo, end) of a set (ascending), -1 when it is none
__device__ __forceinline__ int submatrix_member(const int* __restrict__ set_idx, int lo, int end, int r) {
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (set_idx[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && set_idx[lo] == r ? lo : -1;
}

// grid: x = (member rows AR) * NG, y = slots of this launch (slot0 + blockIdx.y)
template <typename T>
__global__ void __launch_bounds__(256) submatrix_gather(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                        const T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs, int nb, int kind,
                                                        int vec_ok, int nsub, const int* __restrict__ set_ptr, const int* __restrict__ set_idx,
                                                        const int* __restrict__ set_off, const int* __restrict__ sub_dim,
                                                        const int* __restrict__ slot_sub, int slot0, int G, int NG, T* __restrict__ dense, int n,
                                                        int64_t ld, int64_t batch_stride, double pad_diag) {
  __shared__ T tile[kDenseTile * dense_pitch()];
  const int tid = threadIdx.x;
  const int slot = slot0 + (int)blockIdx.y;
  const int a = (int)(blockIdx.x / (unsigned)NG), g = (int)(blockIdx.x - (unsigned)a * (unsigned)NG), AR = (int)(gridDim.x / (unsigned)NG);
  const int sub = slot_sub ? slot_sub[slot] : slot;
  int p0 = 0, cnt = 0, ng = 0;
  if (sub >= 0 && sub < nsub) {
    p0 = set_ptr[sub];
    cnt = max(set_ptr[sub + 1] - p0, 0);
    ng = min(max(sub_dim[sub], 0), n);
  }
  T* win = dense + (int64_t)slot * batch_stride;
  const T zero = dense_zero<T>();
  if (a >= cnt) {   // the rows below the submatrix, dealt round over the workgroups that have no member row
    const int w = (a - cnt) * NG + g, W = (AR - cnt) * NG;
    for (int i = ng + w; i < n; i += W) {
      T* row = win + (int64_t)i * ld;
      for (int j = tid; j < n; j += 256) row[j] = submatrix_pad<T>(j == i ? pad_diag : 0.0);
    }
    return;
  }
  const int R = set_idx[p0 + a], ro = set_off[p0 + a];
  if ((unsigned)R >= (unsigned)nb || ro < 0) return;
  const int m = rs[R];
  if (m < 0 || (int64_t)ro + m > n) return;
  T* rows = win + (int64_t)ro * ld;
  const int bend = min(cnt, (g + 1) * G);
  for (int b = g * G; b < bend; ++b) {
    const int Cb = set_idx[p0 + b], co = set_off[p0 + b];
    if ((unsigned)Cb >= (unsigned)nb || co < 0) continue;
    const int w = cs[Cb];
    if (w < 0 || (int64_t)co + w > n) continue;
    T* out = rows + co;
    int blk = dense_find(row_p, col_i, R, Cb);
    if (blk >= 0) {   // the stored block: m x w, its columns lie across the window's rows
      const int64_t off = blk_p[blk];
      dense_put_transposing<T>(data + off, off, m, w, out, ld, -1, tile, tid, vec_ok);
      continue;
    }
    if (kind >= 0 && Cb != R && rs[Cb] == w && cs[R] == m) blk = dense_find(row_p, col_i, Cb, R);
    if (blk >= 0) {   // the twin of the w x m block stored at (Cb, R): its columns are the window's rows
      const int64_t off = blk_p[blk];
      dense_put_straight<T>(data + off, off, w, m, out, ld, kind, tid, vec_ok);
      continue;
    }
    for (int t = tid; t < m * w; t += 256) {
      const int i = t / w;
      out[(int64_t)i * ld + (t - i * w)] = zero;
    }
  }
  // right of the submatrix: the columns ng ... n - 1 of this member's rows, shared by the NG workgroups of the member row (never on the diagonal)
  const int wp = n - ng;
  for (int i = 0; i < m; ++i) {
    T* row = rows + (int64_t)i * ld + ng;
    for (int j = g * 256 + tid; j < wp; j += NG * 256) row[j] = zero;
  }
}

// grid: x = block rows * S
template <typename T>
__global__ void __launch_bounds__(256) submatrix_scatter(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p,
                                                         T* __restrict__ data, const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int S,
                                                         int vec_ok, int nsub, const int* __restrict__ set_ptr, const int* __restrict__ set_idx,
                                                         const int* __restrict__ set_off, const int* __restrict__ owner,
                                                         const int* __restrict__ sub_slot, const T* __restrict__ dense, int n, int64_t ld,
                                                         int64_t batch_stride) {
  __shared__ T tile[kDenseTile * dense_pitch()];
  const int tid = threadIdx.x;
  const int R = (int)(blockIdx.x / (unsigned)S), sub = (int)(blockIdx.x - (unsigned)R * (unsigned)S);
  if (R >= nbr) return;
  const int m = rs[R];
  for (int b = row_p[R] + sub; b < row_p[R + 1]; b += S) {
    const int Cb = col_i[b];
    if ((unsigned)Cb >= (unsigned)nbr) continue;
    const int g = owner[Cb];
    if (g < 0 || g >= nsub) continue;
    const int slot = sub_slot[g];
    if (slot < 0) continue;
    const int p0 = set_ptr[g], p1 = set_ptr[g + 1];
    const int pr = submatrix_member(set_idx, p0, p1, R);
    if (pr < 0) continue;
    const int pc = submatrix_member(set_idx, p0, p1, Cb);
    if (pc < 0) continue;
    const int ro = set_off[pr], co = set_off[pc], w = cs[Cb];
    if (ro < 0 || co < 0 || (int64_t)ro + m > n || (int64_t)co + w > n) continue;
    const int64_t off = blk_p[b];
    const T* in = dense + (int64_t)slot * batch_stride + (int64_t)ro * ld + co;
    dense_take_transposing<T>(data + off, off, m, w, in, ld, tile, tid, vec_ok);
  }
}

}  // namespace dbcsr_amd
#endif
