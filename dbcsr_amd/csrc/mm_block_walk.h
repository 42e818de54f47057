// mm_block_walk.h -- the walk over one contiguous run of elements (a block, or a piece of one) by the threads of a wave or a workgroup, 16 bytes per
// access where the addresses allow: what the streaming kernels of mm_algebra.h and mm_multivec.h do with every block they touch.  Included by
// mm_algebra.h (and through it by mm_multivec.h and mm_rank_update.h); host-compiled code only, it does not travel to hiprtc.
//
// A block of a matrix with 1 x 1 or odd blocks starts at any element of its data area, so a run has up to V - 1 elements in front of its first 16-byte
// boundary (the head) and up to V - 1 behind its last whole 16 bytes (the tail).  This is the one place that knows where they are: a walk that is off
// by one reads outside the block or counts an element twice.
#ifndef DBCSR_AMD_MM_BLOCK_WALK_H
#define DBCSR_AMD_MM_BLOCK_WALK_H
#include <stdint.h>

namespace dbcsr_amd {

// 16 bytes of elements: what a lane moves per access where the addresses allow
template <typename T>
struct alignas(16) Pack16 {
  static constexpr int V = 16 / (int)sizeof(T);
  T v[V];
};

// ... the same 16 bytes at an address that is only element-aligned: a source block whose start is not congruent to its destination's modulo 16 bytes
// (blocks of 23 x 23 doubles start at odd elements half of the time) is still read 16 bytes per lane, as one unaligned access or two halves
template <typename T>
struct alignas(alignof(T) < 16 ? alignof(T) : 16) Pack16U {
  T v[Pack16<T>::V];
};

// elements in front of the first 16-byte boundary of a block that starts at element `off` of a 16-byte aligned area
template <typename T>
__device__ __forceinline__ int head_of(int64_t off) {
  constexpr int V = Pack16<T>::V;
  return (int)((V - (off & (V - 1))) & (V - 1));
}

// The elements 0 ... len - 1 of a run that starts at element `off` of its data area, by thread `tid` of nt.  one(e): element e, alone.  pack(e): the
// V = 16 / sizeof(T) elements e ... e + V - 1, and (area + off + e) is 16-byte aligned when the area is.  `off` is the offset of the ONE operand the
// caller aligns on; what it reads of other operands at e it reads from wherever they start (Pack16U).
// THE ORDER IS PART OF THE RESULT (the kernels sum per thread and promise the same bits on every call).  With head = min(head_of(off), len),
// nv = (len - head) / V and done = head + nv V, thread tid does, in this order:
//   V > 1 and vec_ok:   one(tid) if tid < head;   pack(head + q V) for q = tid, tid + nt, ... below nv;   one(done + tid) if done + tid < len
//   otherwise:          one(e) for e = tid, tid + nt, ... below len
// (head < V and len - done < V: both are below nt.)  Every element is visited exactly once, none outside [0, len).
template <typename T, typename One, typename Pack>
__device__ __forceinline__ void walk_block(int64_t off, int len, int tid, int nt, int vec_ok, One&& one, Pack&& pack) {
  constexpr int V = Pack16<T>::V;
  if constexpr (V > 1) {
    if (vec_ok) {
      const int h = head_of<T>(off), head = h < len ? h : len, nv = (len - head) / V, done = head + nv * V;
      if (tid < head) one(tid);
      for (int q = tid; q < nv; q += nt) pack(head + q * V);
      if (done + tid < len) one(done + tid);
      return;
    }
  }
  for (int e = tid; e < len; e += nt) one(e);
}

// The same walk over the run at d for a caller that does one thing to every element however it arrives: f(e, d[e]), with aligned 16-byte loads where the
// walk has packs; within a pack in ascending e.
template <typename T, typename F>
__device__ __forceinline__ void walk_block_values(const T* __restrict__ d, int64_t off, int len, int tid, int nt, int vec_ok, F&& f) {
  walk_block<T>(
      off, len, tid, nt, vec_ok, [&](int e) { f(e, d[e]); },
      [&](int e) {
        const Pack16<T> x = *reinterpret_cast<const Pack16<T>*>(d + e);
#pragma unroll
        for (int u = 0; u < Pack16<T>::V; ++u) f(e + u, x.v[u]);
      });
}

}  // namespace dbcsr_amd
#endif
