// mm_engine_tensor.h -- part of mm_engine.hip (included inside extern "C", after mm_engine_csr.h; it uses the helpers of mm_engine_algebra.h and ends the
// life of DBCSR_AMD_BY_TYPE): the C-ABI entry of the block-sparse tensors -- dbcsr_amd_tensor_permute_blocks.  Kernel: mm_tensor.h.  It holds no state and
// works in no buffer of the engine: no saved plan is touched, no work area is written, nothing synchronises.
#ifndef DBCSR_AMD_MM_ENGINE_TENSOR_H
#define DBCSR_AMD_MM_ENGINE_TENSOR_H

extern "C++" {
// workgroups per block: the slabs and tiles of a block of average size, and enough of them to fill the device when the list is short.  The extents live on
// the device; the two lengths bound what a block holds on average.  A sub that finds no slab or tile of its block left ends at once.
static int tensor_split(int64_t nblk, int64_t src_len, int64_t dst_len) {
  const int64_t avg = std::max<int64_t>(1, std::min(src_len, dst_len) / nblk);
  const int64_t by_size = (avg + kTensorSlab - 1) / kTensorSlab, pieces = (avg + kTensorTile * kTensorTile - 1) / (kTensorTile * kTensorTile);
  const int64_t to_fill = std::min(pieces, (2048 + nblk - 1) / nblk);
  return (int)std::min<int64_t>(1024, std::max<int64_t>(1, std::max(by_size, to_fill)));
}

template <typename T>
static void tensor_permute_launch(hipStream_t st, int64_t nblk, int S, int rank, TensorPerm perm, const int32_t* ext, const int64_t* src_off,
                                  const int64_t* dst_off, const void* src, int64_t src_len, void* dst, int64_t dst_len) {
  hipLaunchKernelGGL((tensor_permute_blocks<T>), dim3((unsigned)(nblk * S)), dim3(256), 0, st, nblk, S, rank, perm, ext, src_off, dst_off,
                     static_cast<const T*>(src), src_len, static_cast<T*>(dst), dst_len, aligned16(dst));
}
}  // extern "C++"

int dbcsr_amd_tensor_permute_blocks(void* handle, libsmm_acc_data_t datatype, int64_t nblk, int rank, const int* perm, const int32_t* ext,
                                    const int64_t* src_off, const int64_t* dst_off, const void* src, int64_t src_len, void* dst, int64_t dst_len,
                                    void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !perm || nblk < 0 || src_len < 0 || dst_len < 0 || rank < 2 || rank > 4) return -1;
  TensorPerm p = {{0, 1, 2, 3}};
  int seen = 0;
  for (int j = 0; j < rank; ++j) {
    if (perm[j] < 0 || perm[j] >= rank || (seen >> perm[j]) & 1) return -1;   // (not a permutation of 0 ... rank - 1)
    seen |= 1 << perm[j];
    p.p[j] = perm[j];
  }
  if (!algebra_type(datatype)) return -10;
  if (nblk == 0) return 0;
  if (!ext || !src_off || !dst_off || !src || !dst) return -1;
  const size_t esize = algebra_esize(datatype);
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  if (src_len > 0 && dst_len > 0 && s0 < d0 + esize * (size_t)dst_len && d0 < s0 + esize * (size_t)src_len) return -1;   // the two areas must not overlap
  const int S = tensor_split(nblk, src_len, dst_len);
  if (nblk > INT32_MAX / S) return -1;   // (the grid)
  engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  DBCSR_AMD_BY_TYPE(tensor_permute_launch, st, nblk, S, rank, p, ext, src_off, dst_off, src, src_len, dst, dst_len);
  return check(hipGetLastError(), "dbcsr_amd_tensor_permute_blocks", __FILE__, __LINE__);
}
#undef DBCSR_AMD_BY_TYPE

#endif
