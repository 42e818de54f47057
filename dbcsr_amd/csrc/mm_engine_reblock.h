// mm_engine_reblock.h -- part of mm_engine.hip (included inside extern "C", after mm_engine_csr.h, whose csr_offsets it uses, and before
// mm_engine_tensor.h, which ends the life of DBCSR_AMD_BY_TYPE): the C-ABI entries of re-blocking -- dbcsr_amd_bcsr_reblock_name_blocks and
// dbcsr_amd_bcsr_reblock_gather.  Kernels: mm_reblock.h.  (The third entry of the section, dbcsr_amd_bcsr_reserve_apply_index, stands beside its twin in
// mm_engine_blocklist.h.)  Both work in Engine::rb_* and the scan's scratch alone and keep nothing pending: no work area of the symbolic phase is
// touched and plan_invalidate is not called -- a multiply afterwards reuses its plan.
#ifndef DBCSR_AMD_MM_ENGINE_REBLOCK_H
#define DBCSR_AMD_MM_ENGINE_REBLOCK_H

extern "C++" {
// the running sums of two block structures side by side in rb_off: the source's (sroff[nbr], scoff[nbc] the full lengths) and the new one's
static int reblock_offsets(Engine* E, hipStream_t st, const int32_t* rs, const int32_t* cs, int nbr, int nbc, const int32_t* nrs, const int32_t* ncs, int nnbr,
                           int nnbc, const int64_t** sroff, const int64_t** scoff, const int64_t** nroff, const int64_t** ncoff) {
  if (E->rb_off.ensure((size_t)nbr + (size_t)nbc + (size_t)nnbr + (size_t)nnbc + 4)) return -1;
  int64_t* a = E->rb_off.p;
  int64_t* b = a + nbr + 1;
  int64_t* c = b + nbc + 1;
  int64_t* d = c + nnbr + 1;
  if (exclusive_scan<int64_t>(E, rs, (int64_t)nbr, a, nullptr, true, st) || exclusive_scan<int64_t>(E, cs, (int64_t)nbc, b, nullptr, true, st) ||
      exclusive_scan<int64_t>(E, nrs, (int64_t)nnbr, c, nullptr, true, st) || exclusive_scan<int64_t>(E, ncs, (int64_t)nnbc, d, nullptr, true, st))
    return -1;
  *sroff = a, *scoff = b, *nroff = c, *ncoff = d;
  return 0;
}

// tiles of a new block per workgroup column of the grid: the tiles of a block of average size, fewer where the grid would not hold them
static int reblock_split(int64_t rows, int64_t cols, int nbr, int nbc, int64_t nblks) {
  const int64_t tr = (rows / nbr + kReblockTile - 1) / kReblockTile, tc = (cols / nbc + kReblockTile - 1) / kReblockTile;
  const int64_t T = std::max<int64_t>(1, std::min<int64_t>(tr * tc, 4096));
  return (int)std::max<int64_t>(1, std::min<int64_t>(T, INT32_MAX / std::max<int64_t>(1, nblks)));
}

template <typename T>
static void reblock_gather_launch(hipStream_t st, const dbcsr_amd_bcsr* s, const dbcsr_amd_bcsr* d, const int64_t* sroff, const int64_t* scoff,
                                  const int64_t* droff, const int64_t* dcoff, int split) {
  hipLaunchKernelGGL((reblock_gather<T>), dim3((unsigned)(d->nblks * split)), dim3(256), 0, st, s->row_p, s->col_i, s->blk_p,
                     static_cast<const T*>(s->data), s->row_blk_size, s->col_blk_size, sroff, scoff, s->nblkrows, s->nblkcols, d->row_p, d->col_i, d->blk_p,
                     static_cast<T*>(d->data), d->row_blk_size, d->col_blk_size, droff, dcoff, d->nblkrows, d->nblkcols, (int64_t)d->nblks, split,
                     aligned16(d->data));
}
}  // extern "C++"

int dbcsr_amd_bcsr_reblock_name_blocks(void* handle, const dbcsr_amd_bcsr* src, const int32_t* new_row_blk_size, const int32_t* new_col_blk_size,
                                       int new_nblkrows, int new_nblkcols, int64_t* n_pieces, int32_t* rows, int32_t* cols, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !src || !n_pieces || new_nblkrows < 0 || new_nblkcols < 0 || (new_nblkrows > 0 && !new_row_blk_size) ||
      (new_nblkcols > 0 && !new_col_blk_size) || (rows == nullptr) != (cols == nullptr))
    return -1;
  if (src->nblks < 0 || src->nblks > INT32_MAX) return -1;   // (block positions are 32-bit, as row_p is)
  const bool lists = rows != nullptr;
  const int64_t cap = lists ? *n_pieces : 0;
  if (cap < 0 || cap > INT32_MAX) return -1;
  const int nbr = src->nblkrows, nbc = src->nblkcols;
  const int64_t nb = src->nblks;
  if (nb == 0 || nbr == 0 || nbc == 0 || new_nblkrows == 0 || new_nblkcols == 0 || (lists && cap == 0)) {
    if (!lists) *n_pieces = 0;
    return 0;
  }
  hipStream_t st = stream_of(stream);
  const int64_t *sroff = nullptr, *scoff = nullptr, *nroff = nullptr, *ncoff = nullptr;
  if (reblock_offsets(E, st, src->row_blk_size, src->col_blk_size, nbr, nbc, new_row_blk_size, new_col_blk_size, new_nblkrows, new_nblkcols, &sroff,
                      &scoff, &nroff, &ncoff))
    return -1;
  if (E->rb_i32.ensure(4 * (size_t)nb + 4) || E->rb_pos.ensure((size_t)nb + 2)) return -1;
  int* cnt = E->rb_i32.p;
  int* first = cnt + nb;
  ACC_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * 4 * (size_t)nb, st));   // (a block that no row of row_p covers names nothing)
  hipLaunchKernelGGL(reblock_count_pieces, grid_for((int64_t)nbr * 64), dim3(256), 0, st, src->row_p, src->col_i, sroff, scoff, nbr, nbc, nroff, ncoff,
                     new_nblkrows, new_nblkcols, nb, cnt, first);
  if (exclusive_scan<int64_t>(E, cnt, nb, E->rb_pos.p, nullptr, true, st)) return -1;
  if (!lists) {
    ACC_CHECK(hipMemcpyAsync(E->host_scalars + 10, E->rb_pos.p + nb, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipStreamSynchronize(st));
    const int64_t total = E->host_scalars[10];
    if (total < 0 || total >= INT32_MAX) return -1;   // (the list is 32-bit; a saturated count is refused with the rest)
    *n_pieces = total;
  } else {
    hipLaunchKernelGGL(reblock_name_pieces, grid_for(cap), dim3(256), 0, st, (const int64_t*)E->rb_pos.p, (const int*)first, nb, cap, rows, cols);
  }
  return check(hipGetLastError(), "dbcsr_amd_bcsr_reblock_name_blocks", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_reblock_gather(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !src || !dst) return -1;
  if (!algebra_type(datatype)) return -10;
  if (src->nblks < 0 || src->nblks > INT32_MAX || dst->nblks < 0 || dst->nblks > INT32_MAX) return -1;
  if (src->data && src->data == dst->data) return -1;
  hipStream_t st = stream_of(stream);
  const int64_t *sroff = nullptr, *scoff = nullptr, *droff = nullptr, *dcoff = nullptr;
  int64_t srows = 0, scols = 0, drows = 0, dcols = 0;
  if (reblock_offsets(E, st, src->row_blk_size, src->col_blk_size, src->nblkrows, src->nblkcols, dst->row_blk_size, dst->col_blk_size, dst->nblkrows,
                      dst->nblkcols, &sroff, &scoff, &droff, &dcoff) ||
      dense_lengths(E, st, src, sroff, scoff, &srows, &scols) || dense_lengths(E, st, dst, droff, dcoff, &drows, &dcols))
    return -1;
  if (srows != drows || scols != dcols) return -1;
  engine_writes_values(E);
  if (dst->nblks == 0 || dst->nblkrows == 0 || dst->nblkcols == 0) return 0;
  if (!dst->data || !dst->col_i || !dst->blk_p || (src->nblks > 0 && (!src->data || !src->col_i || !src->blk_p))) return -1;
  const int split = reblock_split(drows, dcols, dst->nblkrows, dst->nblkcols, dst->nblks);
  DBCSR_AMD_BY_TYPE(reblock_gather_launch, st, src, dst, sroff, scoff, droff, dcoff, split);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_reblock_gather", __FILE__, __LINE__);
}
// (DBCSR_AMD_BY_TYPE stays defined for mm_engine_tensor.h, which follows this file and ends its life)

#endif
