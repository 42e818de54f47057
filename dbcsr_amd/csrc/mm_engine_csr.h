// mm_engine_csr.h -- part of mm_engine.hip (included inside extern "C", after mm_engine_blocklist.h; it uses the helpers of mm_engine_algebra.h): the
// C-ABI entries of the element CSR form -- dbcsr_amd_bcsr_to_csr_count / _to_csr_apply, dbcsr_amd_bcsr_from_csr and
// dbcsr_amd_bcsr_csr_name_blocks.  Kernels: mm_csr.h.  They work in Engine::csr_* and the scan's scratch alone: no work area of the symbolic phase is
// touched and plan_invalidate is not called -- a multiply afterwards reuses its plan.  What a count leaves for its apply (the offsets of the block rows
// and columns, the slot bases, the scanned positions) lives in csr_off / csr_pos, which no other entry writes: _from_csr and _csr_name_blocks scan their
// offsets into csr_aux.
#ifndef DBCSR_AMD_MM_ENGINE_CSR_H
#define DBCSR_AMD_MM_ENGINE_CSR_H

extern "C++" {
// element offsets of the block rows and columns (roff[nbr] / coff[nbc]: the full lengths) at the front of `buf`, `extra` more words behind them
static int csr_offsets(Engine* E, hipStream_t st, DevBuf<int64_t>& buf, const int32_t* rs, const int32_t* cs, int nbr, int nbc, size_t extra,
                       const int64_t** roff, const int64_t** coff) {
  if (buf.ensure((size_t)nbr + (size_t)nbc + 2 + extra)) return -1;
  int64_t* r = buf.p;
  int64_t* c = r + nbr + 1;
  if (exclusive_scan<int64_t>(E, rs, (int64_t)nbr, r, nullptr, true, st)) return -1;
  if (exclusive_scan<int64_t>(E, cs, (int64_t)nbc, c, nullptr, true, st)) return -1;
  *roff = r;
  *coff = c;
  return 0;
}

static Engine::CsrLen* csr_len_find(Engine* E, const dbcsr_amd_bcsr* m) {
  if (m->index_stamp == 0) return nullptr;
  for (Engine::CsrLen& k : E->csr_len)
    if (k.stamp == m->index_stamp && k.row_p == m->row_p && k.rs == m->row_blk_size && k.cs == m->col_blk_size && k.nbr == m->nblkrows &&
        k.nbc == m->nblkcols && k.nblks == m->nblks)
      return &k;
  return nullptr;
}

static Engine::CsrLen* csr_len_add(Engine* E, const dbcsr_amd_bcsr* m, int64_t nslots) {
  if (m->index_stamp == 0) return nullptr;
  Engine::CsrLen& k = E->csr_len[E->csr_len_next];
  E->csr_len_next = (E->csr_len_next + 1) % Engine::kCsrLens;
  k.row_p = m->row_p, k.rs = m->row_blk_size, k.cs = m->col_blk_size, k.stamp = m->index_stamp, k.nbr = m->nblkrows, k.nbc = m->nblkcols;
  k.nblks = m->nblks, k.nslots = nslots, k.nze = -1;
  return &k;
}

template <typename T>
static void csr_count_launch(hipStream_t st, const dbcsr_amd_bcsr* m, const int64_t* base, int S, double eps, int* slots) {
  hipLaunchKernelGGL((csr_count<T>), dim3((unsigned)((int64_t)m->nblkrows * S)), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p,
                     static_cast<const T*>(m->data), m->row_blk_size, m->col_blk_size, base, m->nblkrows, S, eps, aligned16(m->data), slots);
}

template <typename T>
static void csr_emit_launch(hipStream_t st, const dbcsr_amd_bcsr* m, const int64_t* coff, const int64_t* base, const int64_t* pos, int S, int use_eps,
                            double eps, int32_t* col, void* values) {
  hipLaunchKernelGGL((csr_emit<T>), dim3((unsigned)((int64_t)m->nblkrows * S)), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p,
                     static_cast<const T*>(m->data), m->row_blk_size, m->col_blk_size, coff, base, pos, m->nblkrows, S, use_eps, eps, aligned16(m->data),
                     col, static_cast<T*>(values));
}

template <typename T>
static void csr_scatter_launch(hipStream_t st, dbcsr_amd_bcsr* m, const int64_t* roff, const int64_t* coff, int S, const int64_t* crow, const int32_t* col,
                               const void* values, int64_t nnz) {
  hipLaunchKernelGGL((csr_scatter<T>), dim3((unsigned)((int64_t)m->nblkrows * S)), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p,
                     static_cast<T*>(m->data), m->row_blk_size, m->col_blk_size, roff, coff, m->nblkrows, S, aligned16(m->data), crow, col,
                     static_cast<const T*>(values), nnz);
}
}  // extern "C++"

int dbcsr_amd_bcsr_to_csr_count(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int use_eps, double eps, int64_t* crow, int64_t* nnz,
                                void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !crow || !nnz) return -1;
  if (use_eps && !(eps >= 0.0)) return -1;   // (negative, or NaN)
  if (!algebra_type(datatype)) return -10;
  E->csr_pending = false;
  *nnz = 0;
  if (m->nblks < 0 || m->nblks > INT32_MAX) return -1;   // (block positions are 32-bit, as row_p is)
  hipStream_t st = stream_of(stream);
  const int nbr = m->nblkrows, nbc = m->nblkcols;
  const int64_t *roff = nullptr, *coff = nullptr;
  int64_t rows = 0, cols = 0;
  if (csr_offsets(E, st, E->csr_off, m->row_blk_size, m->col_blk_size, nbr, nbc, (size_t)nbr + 1, &roff, &coff) ||
      dense_lengths(E, st, m, roff, coff, &rows, &cols))
    return -1;
  if (cols > INT32_MAX) return -1;   // (col is 32-bit)
  int64_t* base = E->csr_off.p + (size_t)nbr + (size_t)nbc + 2;
  // the slots: rows times blocks per block row, scanned; their number is the index's own, remembered with it
  if (E->csr_rows.ensure((size_t)nbr + 1)) return -1;
  if (nbr > 0) hipLaunchKernelGGL(csr_row_slots, grid_for(nbr), dim3(256), 0, st, m->row_p, m->row_blk_size, nbr, E->csr_rows.p);
  if (exclusive_scan<int64_t>(E, E->csr_rows.p, (int64_t)nbr, base, nullptr, true, st)) return -1;
  Engine::CsrLen* known = csr_len_find(E, m);
  int64_t nslots = 0;
  if (known) {
    nslots = known->nslots;
  } else {
    ACC_CHECK(hipMemcpyAsync(E->host_scalars + 8, base + nbr, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipStreamSynchronize(st));
    nslots = E->host_scalars[8];
    known = csr_len_add(E, m, nslots);
  }
  if (nslots < 0 || nslots > INT32_MAX - 8) return -1;
  const int S = algebra_split(nbr, m->nblks);
  if ((int64_t)nbr * S > INT32_MAX) return -1;   // (the grid)
  if (use_eps && nslots > 0 && !m->data) return -1;
  if (E->csr_slots.ensure((size_t)nslots + 1) || E->csr_pos.ensure((size_t)nslots + 2)) return -1;
  if (nslots > 0) {
    if (use_eps) {
      DBCSR_AMD_BY_TYPE(csr_count_launch, st, m, base, S, eps, E->csr_slots.p);
    } else {
      hipLaunchKernelGGL(csr_slot_widths, dim3((unsigned)((int64_t)nbr * S)), dim3(256), 0, st, m->row_p, m->col_i, m->row_blk_size, m->col_blk_size,
                         base, nbr, S, E->csr_slots.p);
    }
  }
  if (exclusive_scan<int64_t>(E, E->csr_slots.p, nslots, E->csr_pos.p, nullptr, true, st)) return -1;
  if (nbr > 0) hipLaunchKernelGGL(csr_crow, dim3((unsigned)nbr), dim3(256), 0, st, m->row_p, m->row_blk_size, roff, base, E->csr_pos.p, nbr, crow);
  else ACC_CHECK(hipMemsetAsync(crow, 0, sizeof(int64_t), st));
  if (!use_eps && known && known->nze >= 0) {   // the index alone decides, and it is a known one: nothing synchronises
    *nnz = known->nze;
  } else {
    ACC_CHECK(hipMemcpyAsync(E->host_scalars + 9, E->csr_pos.p + nslots, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipStreamSynchronize(st));
    *nnz = E->host_scalars[9];
    if (!use_eps && known) known->nze = *nnz;
  }
  E->csr_pending = true;
  E->csr_row_p = m->row_p, E->csr_rs = m->row_blk_size, E->csr_cs = m->col_blk_size;
  E->csr_nblkrows = nbr, E->csr_nblkcols = nbc, E->csr_datatype = (int)datatype, E->csr_use_eps = use_eps ? 1 : 0;
  E->csr_nblks = m->nblks, E->csr_nnz = *nnz, E->csr_nslots = nslots;
  E->csr_eps = eps;
  return check(hipGetLastError(), "dbcsr_amd_bcsr_to_csr_count", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_to_csr_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int32_t* col, void* values, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m) return -1;
  if (!algebra_type(datatype)) return -10;
  const bool pending = E->csr_pending;
  E->csr_pending = false;
  if (!pending || m->row_p != E->csr_row_p || m->row_blk_size != E->csr_rs || m->col_blk_size != E->csr_cs || m->nblkrows != E->csr_nblkrows ||
      m->nblkcols != E->csr_nblkcols || m->nblks != E->csr_nblks || (int)datatype != E->csr_datatype)
    return -1;
  if (E->csr_nnz > 0 && (!col || !values || !m->data)) return -1;
  if (E->csr_nnz == 0 || E->csr_nslots == 0) return 0;
  hipStream_t st = stream_of(stream);
  const int nbr = m->nblkrows, S = algebra_split(nbr, m->nblks);
  const int64_t* coff = E->csr_off.p + (size_t)nbr + 1;
  const int64_t* base = coff + (size_t)m->nblkcols + 1;
  DBCSR_AMD_BY_TYPE(csr_emit_launch, st, m, coff, base, E->csr_pos.p, S, E->csr_use_eps, E->csr_eps, col, values);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_to_csr_apply", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_from_csr(void* handle, libsmm_acc_data_t datatype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* crow, const int32_t* col,
                            const void* values, dbcsr_amd_bcsr* m, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !crow || n_rows < 0 || n_cols < 0 || nnz < 0 || (nnz > 0 && (!col || !values))) return -1;
  if (n_cols > INT32_MAX) return -1;   // (col is 32-bit)
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  const int64_t *roff = nullptr, *coff = nullptr;
  int64_t rows = 0, cols = 0;
  if (csr_offsets(E, st, E->csr_aux, m->row_blk_size, m->col_blk_size, m->nblkrows, m->nblkcols, 0, &roff, &coff) ||
      dense_lengths(E, st, m, roff, coff, &rows, &cols))
    return -1;
  if (rows != n_rows || cols != n_cols) return -1;
  engine_writes_values(E);
  if (n_rows == 0 || n_cols == 0 || m->nblks == 0) return 0;
  if (!m->data) return -1;
  const int S = algebra_split(m->nblkrows, m->nblks);
  if ((int64_t)m->nblkrows * S > INT32_MAX) return -1;   // (the grid)
  DBCSR_AMD_BY_TYPE(csr_scatter_launch, st, m, roff, coff, S, crow, col, values, nnz);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_from_csr", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_csr_name_blocks(void* handle, int64_t n_rows, int64_t nnz, const int64_t* crow, const int32_t* col, const int32_t* row_blk_size,
                                   const int32_t* col_blk_size, int nblkrows, int nblkcols, int32_t* rows, int32_t* cols, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !crow || n_rows < 0 || nnz < 0 || nblkrows < 0 || nblkcols < 0 || (nblkrows > 0 && !row_blk_size) || (nblkcols > 0 && !col_blk_size) ||
      (nnz > 0 && (!col || !rows || !cols)))
    return -1;
  if ((n_rows + 3) / 4 > INT32_MAX) return -1;   // (the grid: a wave per element row)
  if (nnz == 0) return 0;
  hipStream_t st = stream_of(stream);
  const int64_t *roff = nullptr, *coff = nullptr;
  if (csr_offsets(E, st, E->csr_aux, row_blk_size, col_blk_size, nblkrows, nblkcols, 0, &roff, &coff)) return -1;
  ACC_CHECK(hipMemsetAsync(rows, 0xff, sizeof(int32_t) * (size_t)nnz, st));   // (-1, -1): what no row of crow covers stays so
  ACC_CHECK(hipMemsetAsync(cols, 0xff, sizeof(int32_t) * (size_t)nnz, st));
  if (n_rows > 0)
    hipLaunchKernelGGL(csr_name_blocks, grid_for(n_rows * 64), dim3(256), 0, st, crow, col, nnz, n_rows, roff, coff, nblkrows, nblkcols, rows, cols);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_csr_name_blocks", __FILE__, __LINE__);
}
// (DBCSR_AMD_BY_TYPE stays defined for mm_engine_reblock.h and mm_engine_tensor.h, which follow this file; the last one ends its life)

#endif
