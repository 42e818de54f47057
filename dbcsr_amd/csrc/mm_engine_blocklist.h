// mm_engine_blocklist.h -- part of mm_engine.hip (included inside extern "C", after mm_engine_elementwise.h, whose helpers it uses): the C-ABI entries on
// a coordinate list of blocks -- dbcsr_amd_bcsr_reserve_count / _reserve_apply / _reserve_apply_index, dbcsr_amd_bcsr_put_blocks and
// dbcsr_amd_bcsr_get_blocks.  Kernels: mm_blocklist.h.  Put, get and the first half of a reserve count work in Engine::bl_* and the scan's scratch
// alone: no work area of the symbolic phase is touched and plan_invalidate is not called.  Only a reserve that creates blocks goes on into the work
// areas, as the union add does.
#ifndef DBCSR_AMD_MM_ENGINE_BLOCKLIST_H
#define DBCSR_AMD_MM_ENGINE_BLOCKLIST_H

extern "C++" {
template <typename T>
static void put_launch(Engine* E, hipStream_t st, dbcsr_amd_bcsr* m, const int* seg, const int* order, const int64_t* src_off, const void* src,
                       const double alpha[2], int alpha_is_one, int summation) {
  const int nbr = m->nblkrows, S = algebra_split(nbr, m->nblks);
  hipLaunchKernelGGL((blocklist_put<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, m->row_blk_size,
                     m->col_blk_size, nbr, S, (int64_t)m->nblks, seg, order, src_off, static_cast<const T*>(src), algebra_scalar<T>(alpha), alpha_is_one,
                     summation, static_cast<T*>(m->data), aligned16(m->data));
}

template <typename T>
static void get_launch(hipStream_t st, const dbcsr_amd_bcsr* m, int64_t n, const int32_t* rows, const int32_t* cols, const int64_t* dst_off, void* dst,
                       int32_t* found) {
  hipLaunchKernelGGL((blocklist_get<T>), grid_for(n * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, static_cast<const T*>(m->data),
                     m->row_blk_size, m->col_blk_size, m->nblkrows, m->nblkcols, (int64_t)m->nblks, rows, cols, dst_off, n, static_cast<T*>(dst), found,
                     aligned16(dst));
}
}  // extern "C++"

int dbcsr_amd_bcsr_reserve_count(void* handle, const dbcsr_amd_bcsr* m, int64_t n, const int32_t* rows, const int32_t* cols, int upper_only,
                                 int32_t* dst_row_p, int64_t* nblks, int64_t* nze, int64_t* n_new, int64_t* n_invalid, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || n < 0 || (n > 0 && (!rows || !cols)) || !dst_row_p || !nblks || !nze || !n_new || !n_invalid) return -1;
  if (upper_only && m->nblkrows != m->nblkcols) return -1;
  hipStream_t st = stream_of(stream);
  const int nbr = m->nblkrows, nbc = m->nblkcols;
  const int64_t na = m->nblks;
  E->rsv_pending = false;
  *nblks = na;
  *nze = *n_new = *n_invalid = 0;
  if (na > INT32_MAX || n > INT32_MAX) return -1;   // (block positions are 32-bit, as row_p is)
  if (n == 0) return 0;
  // 1. which listed blocks does the matrix lack?  In buffers of the feature's own: with none lacking, nothing else was touched
  const int W = (nbc + 31) / 32;
  const size_t nw = (size_t)nbr * W;
  if (E->bl_bm.ensure(nw + 1) || E->bl_cnt.ensure(4)) return -1;
  ACC_CHECK(hipMemsetAsync(E->bl_cnt.p, 0, 4 * sizeof(unsigned long long), st));
  if (nw > 0) ACC_CHECK(hipMemsetAsync(E->bl_bm.p, 0, sizeof(uint32_t) * nw, st));
  hipLaunchKernelGGL(blocklist_mark, grid_for(n), dim3(256), 0, st, m->row_p, m->col_i, m->row_blk_size, m->col_blk_size, nbr, nbc, W, na, rows, cols, n,
                     upper_only ? 1 : 0, E->bl_bm.p, E->bl_cnt.p);
  if (nbr > 0 && na > 0)
    hipLaunchKernelGGL(blocklist_named_nze, grid_for((int64_t)nbr * 64), dim3(256), 0, st, m->row_p, m->col_i, m->row_blk_size, m->col_blk_size, nbr, na,
                       E->bl_cnt.p);
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, E->bl_cnt.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  *n_invalid = E->host_scalars[kListInvalid];
  if (*n_invalid > 0) return check(hipGetLastError(), "dbcsr_amd_bcsr_reserve_count", __FILE__, __LINE__);   // (nothing to apply: the caller refuses the list)
  *n_new = E->host_scalars[kListNew];
  if (*n_new == 0) return check(hipGetLastError(), "dbcsr_amd_bcsr_reserve_count", __FILE__, __LINE__);
  const int64_t cap = na + *n_new, total = E->host_scalars[kListNamedNze] + E->host_scalars[kListNewNze];
  if (cap > INT32_MAX) return -1;
  // 2. the union of the matrix' pattern and the marked blocks, in the symbolic phase's work areas: the add's count path with the list's bitmap as B's
  plan_invalidate(E);
  E->valid = false;
  engine_takes_work_areas(E);
  if (E->cin_bm.ensure(nw + 1) || E->c_bm.ensure(nw + 1) || E->cin_pre.ensure(nw + 1) || E->c_pre.ensure(nw + 1) || E->row_nnz.ensure((size_t)nbr + 1) ||
      E->blk_nze.ensure((size_t)cap + 1) || E->c_blk_p_ws.ensure((size_t)cap + 1))
    return -1;
  ACC_CHECK(hipMemsetAsync(E->cin_bm.p, 0, sizeof(uint32_t) * nw, st));
  if (na > 0) hipLaunchKernelGGL(bitmap_from_index, grid_for((int64_t)nbr * 64), dim3(256), 0, st, m->row_p, m->col_i, nbr, W, E->cin_bm.p);
  hipLaunchKernelGGL(algebra_union, grid_for((int64_t)nw), dim3(256), 0, st, E->cin_bm.p, (const uint32_t*)E->bl_bm.p, (int64_t)nw, E->c_bm.p);
  hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, st, E->cin_bm.p, nbr, W, E->cin_pre.p, (int*)nullptr);
  hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, st, E->c_bm.p, nbr, W, E->c_pre.p, E->row_nnz.p);
  if (exclusive_scan<int32_t>(E, E->row_nnz.p, nbr, dst_row_p, nullptr, true, st)) return -1;
  hipLaunchKernelGGL(block_sizes_rows, grid_for((int64_t)nw), dim3(256), 0, st, E->c_bm.p, E->c_pre.p, dst_row_p, m->row_blk_size, m->col_blk_size, nbr, W,
                     E->blk_nze.p);
  if (exclusive_scan<int64_t>(E, E->blk_nze.p, cap, E->c_blk_p_ws.p, nullptr, false, st)) return -1;
  E->rsv_pending = true;
  E->rsv_row_p = m->row_p;
  E->rsv_nblkrows = nbr, E->rsv_nblkcols = nbc;
  E->rsv_nblks_a = na;
  *nblks = E->rsv_nblks = cap;
  *nze = E->rsv_nze = total;
  return check(hipGetLastError(), "dbcsr_amd_bcsr_reserve_count", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_reserve_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, dbcsr_amd_bcsr* dst, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !dst) return -1;
  if (!algebra_type(datatype)) return -10;
  const bool pending = E->rsv_pending;
  E->rsv_pending = false;
  if (!pending || m->row_p != E->rsv_row_p || m->nblks != E->rsv_nblks_a || m->nblkrows != E->rsv_nblkrows || m->nblkcols != E->rsv_nblkcols ||
      dst->nblkrows != m->nblkrows || dst->nblkcols != m->nblkcols || !dst->row_p || !dst->col_i || !dst->blk_p || (E->rsv_nze > 0 && !dst->data) ||
      dst->data == m->data)
    return -1;
  engine_writes_values(E);
  plan_invalidate(E);  // this call uses the engine's work areas: the next multiply runs its own symbolic phase
  hipStream_t st = stream_of(stream);
  const int nbr = m->nblkrows, W = (m->nblkcols + 31) / 32;
  if (E->prod_start.ensure(2 * (size_t)E->rsv_nblks + 2)) return -1;
  dst->nblks = E->rsv_nblks;
  // the result's col_i and blk_p by the add's kernel, B absent; then every block the result names = the matrix' block or +0.0 (the copy onto a pattern)
  hipLaunchKernelGGL(algebra_emit, grid_for((int64_t)nbr * W), dim3(256), 0, st, m->row_p, m->blk_p, E->cin_bm.p, E->cin_pre.p, m->row_p, m->blk_p,
                     (const uint32_t*)nullptr, E->cin_pre.p, E->c_bm.p, E->c_pre.p, dst->row_p, E->c_blk_p_ws.p, nbr, W, dst->col_i, dst->blk_p,
                     E->prod_start.p);
  DBCSR_AMD_BY_TYPE(copy_onto_launch, st, m, dst);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_reserve_apply", __FILE__, __LINE__);
}

// _reserve_apply without the data pass (the "Re-blocking" section of the header): col_i and blk_p of the counted union, nothing else -- for a caller
// that writes every element of the new data area itself.  The same pending-state rules; no value is written, so announced block norms stay.
int dbcsr_amd_bcsr_reserve_apply_index(void* handle, const dbcsr_amd_bcsr* m, dbcsr_amd_bcsr* dst, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !dst) return -1;
  const bool pending = E->rsv_pending;
  E->rsv_pending = false;
  if (!pending || m->row_p != E->rsv_row_p || m->nblks != E->rsv_nblks_a || m->nblkrows != E->rsv_nblkrows || m->nblkcols != E->rsv_nblkcols ||
      dst->nblkrows != m->nblkrows || dst->nblkcols != m->nblkcols || !dst->row_p || !dst->col_i || !dst->blk_p)
    return -1;
  plan_invalidate(E);  // this call uses the engine's work areas: the next multiply runs its own symbolic phase
  hipStream_t st = stream_of(stream);
  const int nbr = m->nblkrows, W = (m->nblkcols + 31) / 32;
  if (E->prod_start.ensure(2 * (size_t)E->rsv_nblks + 2)) return -1;
  dst->nblks = E->rsv_nblks;
  hipLaunchKernelGGL(algebra_emit, grid_for((int64_t)nbr * W), dim3(256), 0, st, m->row_p, m->blk_p, E->cin_bm.p, E->cin_pre.p, m->row_p, m->blk_p,
                     (const uint32_t*)nullptr, E->cin_pre.p, E->c_bm.p, E->c_pre.p, dst->row_p, E->c_blk_p_ws.p, nbr, W, dst->col_i, dst->blk_p,
                     E->prod_start.p);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_reserve_apply_index", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_put_blocks(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, int64_t n, const int32_t* rows, const int32_t* cols,
                              const int64_t* src_off, const void* src, const double alpha[2], int summation, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !alpha || n < 0 || (n > 0 && (!rows || !cols || !src_off))) return -1;
  if (!algebra_type(datatype)) return -10;
  if (m->nblks > INT32_MAX - 1 || n > INT32_MAX) return -1;   // (block positions and entry numbers are 32-bit)
  engine_writes_values(E);
  if (n == 0 || m->nblkrows == 0 || m->nblks == 0) return 0;
  hipStream_t st = stream_of(stream);
  const size_t nb = (size_t)m->nblks;
  if (E->bl_i32.ensure(3 * (size_t)n + 2 * nb + 4)) return -1;
  int* hit = E->bl_i32.p;
  int* slots = hit + n;
  int* order = slots + n;
  int* cnt = order + n;
  int* seg = cnt + nb + 1;
  ACC_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * nb, st));
  hipLaunchKernelGGL(blocklist_locate, grid_for(n), dim3(256), 0, st, m->row_p, m->col_i, m->nblkrows, m->nblkcols, (int64_t)m->nblks, rows, cols, n, hit,
                     cnt);
  if (exclusive_scan<int32_t>(E, cnt, (int64_t)nb, seg, nullptr, true, st)) return -1;
  hipLaunchKernelGGL(blocklist_slot, grid_for(n), dim3(256), 0, st, hit, seg, n, cnt, slots);
  hipLaunchKernelGGL(blocklist_order, grid_for(((int64_t)nb + 63) / 64 * 64), dim3(256), 0, st, seg, slots, (int64_t)nb, n, order);
  DBCSR_AMD_BY_TYPE(put_launch, E, st, m, seg, order, src_off, src, alpha, algebra_is_one(datatype, alpha) ? 1 : 0, summation ? 1 : 0);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_put_blocks", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_get_blocks(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int64_t n, const int32_t* rows, const int32_t* cols,
                              const int64_t* dst_off, void* dst, int32_t* found, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || n < 0 || (n > 0 && (!rows || !cols || !dst_off || !found))) return -1;
  if (!algebra_type(datatype)) return -10;
  if (m->nblks > INT32_MAX || n > INT32_MAX) return -1;
  if (n == 0) return 0;
  hipStream_t st = stream_of(stream);
  DBCSR_AMD_BY_TYPE(get_launch, st, m, n, rows, cols, dst_off, dst, found);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_get_blocks", __FILE__, __LINE__);
}
// (DBCSR_AMD_BY_TYPE stays defined for mm_engine_csr.h and mm_engine_tensor.h, which follow this file; the last one ends its life)

#endif
