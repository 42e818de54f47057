// mm_engine_elementwise.h -- part of mm_engine.hip (included inside extern "C", after mm_engine_algebra.h, whose helpers it uses): the C-ABI entries of the
// element-wise operations on two patterns -- dbcsr_amd_bcsr_hadamard_count / _hadamard_apply, dbcsr_amd_bcsr_copy_onto and
// dbcsr_amd_bcsr_function_of_elements.  Kernels: mm_elementwise.h.  They work in Engine::alg_i32 / alg_i64 (the scalars of a count), Engine::ew_* and
// the scan's scratch: no work area of the symbolic phase is touched and plan_invalidate is not called -- a multiply afterwards reuses its plan.
#ifndef DBCSR_AMD_MM_ENGINE_ELEMENTWISE_H
#define DBCSR_AMD_MM_ENGINE_ELEMENTWISE_H

extern "C++" {
template <typename T>
static void mul_flat_launch(hipStream_t st, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, dbcsr_amd_bcsr* dst, int64_t n) {
  const int vec_ok = aligned16(a->data) & aligned16(b->data) & aligned16(dst->data);
  const int64_t V = Pack16<T>::V, lanes = vec_ok ? n / V + n % V : n;   // one 16-byte access per lane, the last n mod V elements one lane each
  hipLaunchKernelGGL((elementwise_mul_flat<T>), grid_for(lanes), dim3(256), 0, st, static_cast<const T*>(a->data), static_cast<const T*>(b->data),
                     static_cast<T*>(dst->data), n, vec_ok);
}

// Waves per block row of the numeric kernels: algebra_split's four blocks per wave.  These passes move the bytes of the add's per-block form (two loads
// and a store per element at most), so its measured choice is taken over (profiles/elementwise.txt has what it gives here).
template <typename T>
static void mul_blocks_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, dbcsr_amd_bcsr* dst, const int64_t* src,
                              const double b_value[2], int b_value_is_one) {
  const int nbr = dst->nblkrows;
  const int S = algebra_split(nbr, E->had_nblks);
  const int vec_ok = aligned16(dst->data);   // (the sources are read from wherever their blocks start)
  hipLaunchKernelGGL((elementwise_mul_blocks<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, dst->row_p, dst->col_i, dst->blk_p, src,
                     dst->row_blk_size, dst->col_blk_size, nbr, S, static_cast<const T*>(a->data), static_cast<const T*>(b->data),
                     static_cast<T*>(dst->data), algebra_scalar<T>(b_value), b_value_is_one, vec_ok);
}

template <typename T>
static void copy_onto_launch(hipStream_t st, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst) {
  const int nbr = dst->nblkrows, S = algebra_split(nbr, dst->nblks);
  hipLaunchKernelGGL((elementwise_copy_onto<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, src->row_p, src->col_i, src->blk_p,
                     static_cast<const T*>(src->data), dst->row_p, dst->col_i, dst->blk_p, static_cast<T*>(dst->data), dst->row_blk_size,
                     dst->col_blk_size, nbr, S, src->nblks, aligned16(dst->data));
}

template <typename T>
static void function_launch(hipStream_t st, dbcsr_amd_bcsr* m, int func, double a0, double a1) {
  const int nbr = m->nblkrows, S = algebra_split(nbr, m->nblks);
  hipLaunchKernelGGL((elementwise_function<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, m->row_blk_size,
                     m->col_blk_size, nbr, S, func, a0, a1, static_cast<T*>(m->data), aligned16(m->data));
}
}  // extern "C++"

int dbcsr_amd_bcsr_hadamard_count(void* handle, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int b_assumed, int32_t* dst_row_p, int64_t* nblks,
                                  int64_t* nze, int* same_pattern, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !a || !b || !dst_row_p || !nblks || !nze || !same_pattern) return -1;
  if (a->nblkrows != b->nblkrows || a->nblkcols != b->nblkcols) return -1;
  hipStream_t st = stream_of(stream);
  const int nbr = a->nblkrows;
  const int64_t na = a->nblks, nb = b->nblks;
  E->had_mode = 0;
  E->had_assumed = b_assumed ? 1 : 0;
  E->had_nblks_a = na, E->had_nblks_b = nb;
  *nblks = *nze = 0;
  *same_pattern = 0;
  if (na > INT32_MAX || nb > INT32_MAX) return -1;   // (block positions are 32-bit, as row_p is)
  if (E->alg_i32.ensure(4) || E->alg_i64.ensure(8)) return -1;
  // 1. the same pattern at the same offsets, A packed?  (the add's check)
  if (na == nb) {
    int flags = 0;
    int64_t packed_nze = 0;
    if (same_index_packed(E, st, a, b, &flags, &packed_nze)) return -1;
    if (flags == 0) {
      if (dst_row_p != a->row_p) ACC_CHECK(hipMemcpyAsync(dst_row_p, a->row_p, sizeof(int32_t) * ((size_t)nbr + 1), hipMemcpyDeviceToDevice, st));
      E->had_mode = 1;
      *nblks = E->had_nblks = na;
      *nze = E->had_nze = packed_nze;
      *same_pattern = 1;
      return check(hipGetLastError(), "dbcsr_amd_bcsr_hadamard_count", __FILE__, __LINE__);
    }
  }
  // 2. the blocks of A that B has too (or all of them, with b_assumed): marked per block of A, counted per row, both scanned
  if (E->ew_i32.ensure(2 * (size_t)na + (size_t)nbr + 4) || E->ew_i64.ensure(3 * (size_t)na + 4)) return -1;
  int* partner = E->ew_i32.p;
  int* blk_nze = partner + na;
  int* row_cnt = blk_nze + na;
  if (nbr > 0) ACC_CHECK(hipMemsetAsync(row_cnt, 0, sizeof(int) * (size_t)nbr, st));
  if (nbr > 0 && na > 0) {
    const int S = std::max(1, row_split(nbr, na / 64));   // (a lane per block: a wave covers 64 of them)
    hipLaunchKernelGGL(elementwise_match, grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, a->row_p, a->col_i, b->row_p, b->col_i, a->row_blk_size,
                       a->col_blk_size, nbr, S, na, nb, E->had_assumed, partner, blk_nze, row_cnt);
  }
  if (exclusive_scan<int32_t>(E, row_cnt, nbr, dst_row_p, E->alg_i64.p + 0, true, st)) return -1;
  if (exclusive_scan<int64_t>(E, blk_nze, nbr > 0 ? na : 0, E->ew_i64.p, E->alg_i64.p + 1, false, st)) return -1;
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, E->alg_i64.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  E->had_mode = 2;
  *nblks = E->had_nblks = E->host_scalars[0];
  *nze = E->had_nze = E->host_scalars[1];
  return check(hipGetLastError(), "dbcsr_amd_bcsr_hadamard_count", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_hadamard_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, const double b_value[2],
                                  dbcsr_amd_bcsr* dst, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !a || !b || !dst) return -1;
  if (!algebra_type(datatype)) return -10;
  const int pending = E->had_mode;
  E->had_mode = 0;
  engine_writes_values(E);
  if (!pending || a->nblks != E->had_nblks_a || b->nblks != E->had_nblks_b || (b_value != nullptr) != (E->had_assumed != 0) ||
      a->nblkrows != b->nblkrows || a->nblkcols != b->nblkcols || dst->nblkrows != a->nblkrows || dst->nblkcols != a->nblkcols)
    return -1;
  hipStream_t st = stream_of(stream);
  dst->nblks = E->had_nblks;
  if (pending == 1) {   // same pattern: one flat pass, in place when dst is a or b (the index is then not touched at all)
    if (E->had_nblks == 0) return 0;
    if (dst->col_i != a->col_i && dst->col_i != b->col_i)
      ACC_CHECK(hipMemcpyAsync(dst->col_i, a->col_i, sizeof(int32_t) * (size_t)a->nblks, hipMemcpyDeviceToDevice, st));
    if (dst->blk_p != a->blk_p && dst->blk_p != b->blk_p)
      ACC_CHECK(hipMemcpyAsync(dst->blk_p, a->blk_p, sizeof(int64_t) * (size_t)a->nblks, hipMemcpyDeviceToDevice, st));
    DBCSR_AMD_BY_TYPE(mul_flat_launch, st, a, b, dst, E->had_nze);
    return check(hipGetLastError(), "dbcsr_amd_bcsr_hadamard_apply", __FILE__, __LINE__);
  }
  if (E->had_nblks == 0) return 0;
  if (dst->data == a->data || dst->data == b->data) return -1;   // two patterns: not done in place
  const int nbr = a->nblkrows;
  const int64_t* off = E->ew_i64.p;
  int64_t* src = E->ew_i64.p + a->nblks + 2;   // (the count sized the buffer for a result with all of A's blocks)
  hipLaunchKernelGGL(elementwise_emit, grid_for((int64_t)nbr * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, b->blk_p, E->ew_i32.p, off, dst->row_p,
                     nbr, (int64_t)a->nblks, E->had_nblks, dst->col_i, dst->blk_p, src);
  const double one[2] = {1.0, 0.0};   // (no assumed value: no block takes it)
  const double* v = b_value ? b_value : one;
  DBCSR_AMD_BY_TYPE(mul_blocks_launch, E, st, a, b, dst, src, v, algebra_is_one(datatype, v) ? 1 : 0);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_hadamard_apply", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_copy_onto(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !src || !dst || src->nblkrows != dst->nblkrows || src->nblkcols != dst->nblkcols) return -1;
  if (!algebra_type(datatype)) return -10;
  if (src->nblks > INT32_MAX) return -1;   // (block positions are 32-bit, as row_p is)
  engine_writes_values(E);
  if (dst->nblkrows == 0 || dst->nblks == 0) return 0;
  hipStream_t st = stream_of(stream);
  DBCSR_AMD_BY_TYPE(copy_onto_launch, st, src, dst);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_copy_onto", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_function_of_elements(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, int func, double a0, double a1, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !function_known(func)) return -1;
  if (datatype != dbcsr_type_real_8 && datatype != dbcsr_type_real_4) return -10;   // (complex data: not offered, see the header)
  engine_writes_values(E);
  if (m->nblkrows == 0 || m->nblks == 0) return 0;
  hipStream_t st = stream_of(stream);
  if (datatype == dbcsr_type_real_8) function_launch<double>(st, m, func, a0, a1);
  else function_launch<float>(st, m, func, a0, a1);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_function_of_elements", __FILE__, __LINE__);
}

#endif
