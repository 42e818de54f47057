// mm_tensor.h -- the re-folding of block-sparse tensors on the device: dbcsr_amd_tensor_permute_blocks (tensor_permute_blocks).  Part of the
// device-resident multiply engine: included by mm_engine.hip after mm_csr.h.
//
// A tensor block is a Fortran array of up to four dimensions at an element offset of a flat area.  One launch moves a list of blocks: entry b is the array
// of extents ext[b][0 ... 3] (source order, padded with 1) at src + src_off[b], and it is written at dst + dst_off[b] with its dimensions permuted by one
// `perm` for the whole launch: dimension j of the written array is dimension perm[j] of the read one.  A pure move: bits are loaded and stored, nothing is
// computed with them.
//
// Every workgroup first reduces the move of its block (uniform integer work on four numbers): in the order of the written array each dimension is
// (extent, stride in the source); extents of 1 drop out, and a dimension whose source stride is the previous one's stride times its extent -- adjacent on
// both sides, in the same order -- joins the previous one.  What is left decides the move:
//   straight     nothing left, or the fastest dimension is the same on both sides (its source stride is 1): the written window is walked in its own
//                order, in slabs of kTensorSlab elements cut at 16-byte boundaries of the written side (walk_block: 16 bytes per lane where the area
//                allows).  A lane turns the place of its pack into the source offset (at most three divisions; none for a plain copy) and, where the pack
//                does not leave the run of the fastest dimension, loads its 16 bytes in one piece from wherever they start (Pack16U); a pack that crosses
//                runs steps through the dimensions with carries.  Consecutive lanes meet consecutive addresses on both sides.
//   transposing  the fastest dimension of the source (p, source stride 1) is another one than the fastest of the written array (q, written stride 1):
//                tiles of up to 32 x 32 elements of the plane (p, q) go through LDS, one tile per step, for every place of the other dimensions.  The tile is
//                filled along p -- consecutive lanes read consecutive source elements, and where the source rows of the plane are adjacent the runs
//                join -- and drained along q, consecutive lanes writing consecutive elements.  tile[q P + p], P = 33: the fill meets consecutive words, the
//                drain a stride of P elements, which meets every bank once for 4-, 8- and 16-byte elements (mm_dense.h has the count).
// Neither side is ever walked with a stride on its global accesses.  Workgroups go per (block, sub of S): slabs and tiles sub, sub + S, ... of the block,
// so a block of 23^3 elements occupies several workgroups and the launch is no chain per block.  No atomics, no scratch, no memset; LDS is the one tile.
//
// A block is skipped as a whole -- nothing of it is read or written -- when an extent is below 1, when it has 2^31 elements or more (block sizes are 32-bit
// everywhere in this library), or when one of its windows does not lie inside [0, src_len) / [0, dst_len).  Offsets are 64-bit element offsets; places
// inside a block are 32-bit.
#ifndef DBCSR_AMD_MM_TENSOR_H
#define DBCSR_AMD_MM_TENSOR_H
#include "mm_algebra.h"

namespace dbcsr_amd {

constexpr int kTensorTile = 32;      // rows and columns of the LDS tile of the transposing move
constexpr int kTensorSlab = 4096;    // elements of a slab of the straight move (a multiple of every pack)
__host__ __device__ constexpr int tensor_pitch() { return kTensorTile | 1; }

// `perm` of a launch, by value: dimension j of the written array is dimension p[j] of the read one (the identity from `rank` on)
struct TensorPerm {
  int p[4];
};

// x[i] of four values without an indexed array (an indexed array in registers would go to scratch)
__device__ __forceinline__ int tensor_pick(int x0, int x1, int x2, int x3, int i) { return i == 0 ? x0 : i == 1 ? x1 : i == 2 ? x2 : x3; }

// the reduced move: n dimensions in the order of the written array, extent d and source stride t each; slots from n on are (1, 0)
struct TensorMove {
  int n;
  int d0, d1, d2, d3;
  int t0, t1, t2, t3;
};

__device__ __forceinline__ void tensor_set(TensorMove& m, int k, int d, int t) {
  m.d0 = k == 0 ? d : m.d0, m.d1 = k == 1 ? d : m.d1, m.d2 = k == 2 ? d : m.d2, m.d3 = k == 3 ? d : m.d3;
  m.t0 = k == 0 ? t : m.t0, m.t1 = k == 1 ? t : m.t1, m.t2 = k == 2 ? t : m.t2, m.t3 = k == 3 ? t : m.t3;
}

// e0 ... e3: the extents in source order (each >= 1, product below 2^31)
__device__ __forceinline__ TensorMove tensor_reduce(int e0, int e1, int e2, int e3, const TensorPerm& perm) {
  const int s0 = 1, s1 = e0, s2 = e0 * e1, s3 = e0 * e1 * e2;   // the source strides
  TensorMove m = {0, 1, 1, 1, 1, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = tensor_pick(e0, e1, e2, e3, perm.p[j]), t = tensor_pick(s0, s1, s2, s3, perm.p[j]);
    if (d == 1) continue;
    const int ld = tensor_pick(m.d0, m.d1, m.d2, m.d3, m.n - 1), lt = tensor_pick(m.t0, m.t1, m.t2, m.t3, m.n - 1);
    if (m.n > 0 && t == lt * ld) {
      tensor_set(m, m.n - 1, ld * d, lt);
    } else {
      tensor_set(m, m.n, d, t);
      ++m.n;
    }
  }
  return m;
}

// the place of element e of the written window, dimension by dimension
struct TensorPlace {
  int i0, i1, i2, i3;
};

__device__ __forceinline__ TensorPlace tensor_place(const TensorMove& m, int e) {
  TensorPlace x = {e, 0, 0, 0};
  if (m.n > 1) {
    int q = e / m.d0;
    x.i0 = e - q * m.d0;
    x.i1 = q;
    if (m.n > 2) {
      const int r = q / m.d1;
      x.i1 = q - r * m.d1;
      x.i2 = r;
      if (m.n > 3) {
        x.i3 = r / m.d2;
        x.i2 = r - x.i3 * m.d2;
      }
    }
  }
  return x;
}

__device__ __forceinline__ int tensor_source(const TensorMove& m, const TensorPlace& x) {
  return m.n > 1 ? x.i0 * m.t0 + x.i1 * m.t1 + x.i2 * m.t2 + x.i3 * m.t3 : x.i0;
}

// the next element of the written window
__device__ __forceinline__ void tensor_step(const TensorMove& m, TensorPlace& x) {
  if (++x.i0 < m.d0 || m.n <= 1) return;
  x.i0 = 0;
  if (++x.i1 < m.d1) return;
  x.i1 = 0;
  if (++x.i2 < m.d2) return;
  x.i2 = 0;
  ++x.i3;
}

// straight: dst[e] <- src[source of e] for the slabs sub, sub + S, ... of the window of n elements that starts at element doff of its area
template <typename T>
__device__ __forceinline__ void tensor_move_straight(const TensorMove& m, const T* __restrict__ src, T* __restrict__ dst, int64_t doff, int n, int sub, int S,
                                                     int tid, int vec_ok) {
  constexpr int V = Pack16<T>::V;
  const int h = head_of<T>(doff), head = h < n ? h : n;
  const int64_t nslab = n > head ? ((int64_t)(n - head) + kTensorSlab - 1) / kTensorSlab : 1;   // slab 0 takes the head with it
  for (int64_t c = sub; c < nslab; c += S) {
    const int64_t lo64 = c == 0 ? 0 : head + c * kTensorSlab, hi64 = head + (c + 1) * kTensorSlab;
    const int lo = (int)lo64, hi = hi64 < n ? (int)hi64 : n;
    T* d = dst + lo;
    walk_block<T>(
        doff + lo, hi - lo, tid, 256, vec_ok, [&](int e) { d[e] = src[tensor_source(m, tensor_place(m, lo + e))]; },
        [&](int e) {
          TensorPlace x = tensor_place(m, lo + e);
          Pack16<T> r;
          if (m.n <= 1 || x.i0 + V <= m.d0) {   // the pack stays inside one run of the fastest dimension
            const Pack16U<T> y = *reinterpret_cast<const Pack16U<T>*>(src + tensor_source(m, x));
#pragma unroll
            for (int u = 0; u < V; ++u) r.v[u] = y.v[u];
          } else {
#pragma unroll
            for (int u = 0; u < V; ++u) {
              r.v[u] = src[tensor_source(m, x)];
              tensor_step(m, x);
            }
          }
          *reinterpret_cast<Pack16<T>*>(d + e) = r;
        });
  }
}

// transposing: the tiles sub, sub + S, ... of the block.  k: the slot whose source stride is 1 (1 ... 3)
template <typename T>
__device__ __forceinline__ void tensor_move_transposing(const TensorMove& m, int k, const T* __restrict__ src, T* __restrict__ dst, int sub, int S, int tid,
                                                        T* tile) {
  constexpr int P = tensor_pitch();
  // the written strides of the slots; a and b: the two slots of 1 ... 3 that are not k
  const int w1 = m.d0, w2 = m.d0 * m.d1, w3 = w2 * m.d2;
  const int a = k == 1 ? 2 : 1, b = k == 3 ? 2 : 3;
  const int np = tensor_pick(1, m.d1, m.d2, m.d3, k), nq = m.d0, tq0 = m.t0, wk = tensor_pick(1, w1, w2, w3, k);
  const int da = tensor_pick(1, m.d1, m.d2, m.d3, a), ta = tensor_pick(0, m.t1, m.t2, m.t3, a), wa = tensor_pick(1, w1, w2, w3, a);
  const int tb = tensor_pick(0, m.t1, m.t2, m.t3, b), wb = tensor_pick(1, w1, w2, w3, b), db = tensor_pick(1, m.d1, m.d2, m.d3, b);
  const int ntp = (np + kTensorTile - 1) / kTensorTile, ntq = (nq + kTensorTile - 1) / kTensorTile;
  const unsigned ntiles = (unsigned)ntp * (unsigned)ntq * (unsigned)da * (unsigned)db;   // (no more than the block has elements: below 2^31)
  for (unsigned u = (unsigned)sub; u < ntiles; u += (unsigned)S) {
    const unsigned r = u / (unsigned)ntq;
    const int q0 = (int)(u - r * (unsigned)ntq) * kTensorTile;
    const unsigned r2 = r / (unsigned)ntp;
    const int p0 = (int)(r - r2 * (unsigned)ntp) * kTensorTile;
    const int ib = (int)(r2 / (unsigned)da), ia = (int)r2 - ib * da;
    const int tp = min(kTensorTile, np - p0), tq = min(kTensorTile, nq - q0);
    const T* s = src + ((int64_t)ia * ta + (int64_t)ib * tb + p0 + (int64_t)q0 * tq0);
    T* d = dst + ((int64_t)ia * wa + (int64_t)ib * wb + q0 + (int64_t)p0 * wk);
    for (int t = tid; t < tp * tq; t += 256) {
      const int q = t / tp, p = t - q * tp;
      tile[q * P + p] = s[(int64_t)q * tq0 + p];
    }
    __syncthreads();
    for (int t = tid; t < tp * tq; t += 256) {
      const int p = t / tq, q = t - p * tq;
      d[(int64_t)p * wk + q] = tile[q * P + p];
    }
    __syncthreads();
  }
}

// One workgroup per (entry b of the list, sub of S): see the head of this file.
template <typename T>
__global__ void __launch_bounds__(256) tensor_permute_blocks(int64_t nblk, int S, int rank, TensorPerm perm, const int32_t* __restrict__ ext,
                                                             const int64_t* __restrict__ src_off, const int64_t* __restrict__ dst_off,
                                                             const T* __restrict__ src, int64_t src_len, T* __restrict__ dst, int64_t dst_len, int vec_ok) {
  __shared__ T tile[kTensorTile * tensor_pitch()];
  const int tid = threadIdx.x;
  const int64_t b = (int64_t)(blockIdx.x / (unsigned)S);
  const int sub = (int)(blockIdx.x - (unsigned)b * (unsigned)S);
  if (b >= nblk) return;
  const int e0 = ext[4 * b], e1 = ext[4 * b + 1], e2 = rank > 2 ? ext[4 * b + 2] : 1, e3 = rank > 3 ? ext[4 * b + 3] : 1;
  if (e0 < 1 || e1 < 1 || e2 < 1 || e3 < 1) return;
  const int64_t n01 = (int64_t)e0 * e1, n23 = (int64_t)e2 * e3;   // (each below 2^62)
  if (n01 > INT32_MAX || n23 > INT32_MAX || n01 * n23 > INT32_MAX) return;
  const int n = (int)(n01 * n23);
  const int64_t so = src_off[b], dof = dst_off[b];
  if (so < 0 || dof < 0 || so > src_len - n || dof > dst_len - n) return;   // (a window that leaves its area: the entry is skipped)
  const TensorMove m = tensor_reduce(e0, e1, e2, e3, perm);
  if (m.n == 0 || m.t0 == 1) {
    tensor_move_straight<T>(m, src + so, dst + dof, dof, n, sub, S, tid, vec_ok);
  } else {
    const int k = m.t1 == 1 ? 1 : m.t2 == 1 ? 2 : 3;
    tensor_move_transposing<T>(m, k, src + so, dst + dof, sub, S, tid, tile);
  }
}

}  // namespace dbcsr_amd
#endif
