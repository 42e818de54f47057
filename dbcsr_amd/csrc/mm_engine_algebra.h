// mm_engine_algebra.h -- part of mm_engine.hip (included inside extern "C", after mm_engine_ops.h): the C-ABI operations between multiplies --
// dbcsr_amd_bcsr_add_count / _add_apply, the pieces of dbcsr_add_on_diag (dbcsr_amd_bcsr_diag_count / _diag_fill / _diag_shift), dbcsr_amd_bcsr_trace,
// _dot, _norm2, and the norms and vectors: dbcsr_amd_bcsr_maxabs, _row_sums, _col_sums, _gershgorin, _get_diag, _set_diag, _scale_by_vector, _matvec, _multivec, _rank_update, _multiply_dense,
// the block diagonal: dbcsr_amd_bcsr_block_diag_count / _apply / _invert / _multiply, and the dense conversion: dbcsr_amd_bcsr_to_dense / _from_dense_apply /
// _from_dense_count, and the submatrix method: dbcsr_amd_bcsr_submatrix_gather / _submatrix_scatter.
// Kernels: mm_algebra.h, mm_multivec.h, mm_rank_update.h, mm_spmm.h, mm_block_inverse.h, mm_block_scale.h, mm_dense.h, mm_submatrix.h. The reductions, the diagonal pieces, the same-pattern add and the norms and vectors use buffers of their own (Engine::alg_*) and the
// scan's scratch, which no saved plan depends on (the checksum uses it the same way): they do NOT invalidate the plan.  The union add borrows the
// symbolic phase's bitmaps and prefix arrays and invalidates it, as filter and crop do.
#ifndef DBCSR_AMD_MM_ENGINE_ALGEBRA_H
#define DBCSR_AMD_MM_ENGINE_ALGEBRA_H

extern "C++" {
template <typename T> static inline T algebra_scalar(const double s[2]);
template <> inline double algebra_scalar<double>(const double s[2]) { return s[0]; }
template <> inline float algebra_scalar<float>(const double s[2]) { return (float)s[0]; }   // (the imaginary part of a scalar is ignored for real data)
template <> inline z64 algebra_scalar<z64>(const double s[2]) { return z64(s[0], s[1]); }

static inline bool algebra_is_one(libsmm_acc_data_t datatype, const double s[2]) { return s[0] == 1.0 && (datatype != dbcsr_type_complex_8 || s[1] == 0.0); }
static inline bool algebra_is_zero(libsmm_acc_data_t datatype, const double s[2]) { return s[0] == 0.0 && (datatype != dbcsr_type_complex_8 || s[1] == 0.0); }
static inline int aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 ? 1 : 0; }
static inline bool algebra_type(libsmm_acc_data_t datatype) {
  return datatype == dbcsr_type_real_8 || datatype == dbcsr_type_real_4 || datatype == dbcsr_type_complex_8;
}

// F<element type>(...) for a `datatype` that algebra_type() accepted (an expression: it has F's value where F returns one).  The one place of this file
// that turns a data type into an element type; dbcsr_amd_bcsr_dot, which offers two of the three, chooses for itself.
#define DBCSR_AMD_BY_TYPE(F, ...)                                  \
  (datatype == dbcsr_type_real_8   ? F<double>(__VA_ARGS__)        \
   : datatype == dbcsr_type_real_4 ? F<float>(__VA_ARGS__)         \
                                   : F<z64>(__VA_ARGS__))

template <typename T> static inline size_t algebra_sizeof() { return sizeof(T); }
static inline size_t algebra_esize(libsmm_acc_data_t datatype) { return DBCSR_AMD_BY_TYPE(algebra_sizeof); }

// `mode` of the matvec family (matvec, multivec, rank update): *product = alpha != 0 and there is something to multiply (`operands`); without a product
// the operands are not read and the result is beta times what was there
static inline int product_mode(libsmm_acc_data_t datatype, const double alpha[2], const double beta[2], bool operands, bool* product) {
  *product = !algebra_is_zero(datatype, alpha) && operands;
  return (*product ? 0 : kMatvecNoProduct) | (algebra_is_zero(datatype, beta) ? kMatvecBetaZero : 0);
}

// the `trans` and `kind` arguments of matvec and multivec: an operation N, T or C; no symmetry (-1) or the stored triangle of a square matrix (0 ... 3)
static inline bool matvec_args_ok(char trans, int kind, const dbcsr_amd_bcsr* a) {
  return (trans == 'N' || trans == 'T' || trans == 'C') && kind >= -1 && kind <= 3 && (kind < 0 || a->nblkrows == a->nblkcols);
}

// waves per block row of the per-block add: about four result blocks per wave (config 2's shape at 50 % overlap: 3.35 ms, against 3.52 ms with row_split's
// 65536 waves; the reductions keep row_split -- every wave they add is a partial more for the one workgroup that sums them)
static inline int algebra_split(int64_t nbr, int64_t nblks) {
  if (nbr <= 0) return 1;
  return (int)std::max<int64_t>(1, std::min<int64_t>(nblks / nbr / 4, 1024));
}

template <typename T>
static void add_flat_launch(hipStream_t st, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, dbcsr_amd_bcsr* dst, int64_t n, const double alpha[2],
                            const double beta[2], int mode) {
  const int vec_ok = aligned16(a->data) & aligned16(b->data) & aligned16(dst->data);
  const int64_t V = Pack16<T>::V, lanes = vec_ok ? n / V + n % V : n;   // one 16-byte access per lane, the last n mod V elements one lane each
  hipLaunchKernelGGL((algebra_add_flat<T>), grid_for(lanes), dim3(256), 0, st, static_cast<const T*>(a->data), static_cast<const T*>(b->data),
                     static_cast<T*>(dst->data), n, algebra_scalar<T>(alpha), algebra_scalar<T>(beta), mode, vec_ok);
}

template <typename T>
static void add_blocks_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, dbcsr_amd_bcsr* dst, const double alpha[2],
                              const double beta[2], int mode) {
  const int nbr = dst->nblkrows;
  const int S = algebra_split(nbr, E->add_nblks);
  const int vec_ok = aligned16(dst->data);   // (the sources are read from wherever their blocks start)
  hipLaunchKernelGGL((algebra_add_blocks<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, dst->row_p, dst->col_i, dst->blk_p, E->prod_start.p,
                     dst->row_blk_size, dst->col_blk_size, nbr, S, static_cast<const T*>(a->data), static_cast<const T*>(b->data),
                     static_cast<T*>(dst->data), algebra_scalar<T>(alpha), algebra_scalar<T>(beta), mode, vec_ok);
}

template <typename T>
static void diag_launch(hipStream_t st, bool fill, const dbcsr_amd_bcsr* m, const double alpha[2]) {
  if (fill)
    hipLaunchKernelGGL((diag_fill<T>), grid_for((int64_t)m->nblkrows * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, m->row_blk_size, m->nblkrows,
                       algebra_scalar<T>(alpha), static_cast<T*>(m->data));
  else
    hipLaunchKernelGGL((diag_shift<T>), grid_for((int64_t)m->nblkrows * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, m->row_blk_size, m->col_blk_size, m->nblkrows,
                       algebra_scalar<T>(alpha), static_cast<T*>(m->data));
}

// what: 0 trace, 1 norm^2; returns the number of partial pairs written to E->alg_sums
template <typename T>
static int64_t reduce_launch(Engine* E, hipStream_t st, int what, const dbcsr_amd_bcsr* a, int symmetric) {
  const int nbr = a->nblkrows;
  const int S = what == 0 ? 1 : row_split(nbr, a->nblks);
  const int64_t nw = (int64_t)nbr * S;
  if (E->alg_sums.ensure(2 * (size_t)nw + 2)) return -1;
  if (what == 0)
    hipLaunchKernelGGL((algebra_trace<T>), grid_for(nw * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, static_cast<const T*>(a->data),
                       a->row_blk_size, a->col_blk_size, nbr, E->alg_sums.p);
  else
    hipLaunchKernelGGL((algebra_norm2<T>), grid_for(nw * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, static_cast<const T*>(a->data),
                       a->row_blk_size, a->col_blk_size, nbr, S, symmetric, aligned16(a->data), E->alg_sums.p);
  return nw;
}

template <typename T>
static int64_t dot_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int symmetric) {
  const int nbr = a->nblkrows;
  const int S = row_split(nbr, a->nblks);
  const int64_t nw = (int64_t)nbr * S;
  if (E->alg_sums.ensure(2 * (size_t)nw + 2)) return -1;
  hipLaunchKernelGGL((algebra_dot<T>), grid_for(nw * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, static_cast<const T*>(a->data), b->row_p,
                     b->col_i, b->blk_p, static_cast<const T*>(b->data), a->row_blk_size, a->col_blk_size, nbr, S, symmetric,
                     aligned16(a->data), E->alg_sums.p);
  return nw;
}

// the partial pairs summed in a fixed order by one workgroup, the two sums brought to the host (synchronises)
static int reduce_finish(Engine* E, hipStream_t st, int64_t nw, double out2[2], const char* what) {
  if (nw < 0) return -1;
  hipLaunchKernelGGL(checksum_final, dim3(1), dim3(256), 0, st, E->alg_sums.p, (int)nw, E->alg_sums.p + 2 * (size_t)nw);
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 4, E->alg_sums.p + 2 * (size_t)nw, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  memcpy(out2, E->host_scalars + 4, 2 * sizeof(double));
  return check(hipGetLastError(), what, __FILE__, __LINE__);
}

// Do A and B, both with na blocks, have the same pattern at the same offsets, and is A packed?  algebra_compare's flags (0: yes) and the end of A's last
// block, brought to the host (one small kernel, one flag; synchronises; a saved plan is not touched).  The callers made alg_i32 hold 4 and alg_i64 8 entries.
static int same_index_packed(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int* flags, int64_t* packed_nze) {
  const int nbr = a->nblkrows;
  const int64_t na = a->nblks;
  *flags = 0;
  *packed_nze = 0;
  if (na <= 0 || nbr <= 0) return 0;
  ACC_CHECK(hipMemsetAsync(E->alg_i32.p, 0, sizeof(int), st));
  ACC_CHECK(hipMemsetAsync(E->alg_i64.p, 0, sizeof(int64_t), st));
  const int S = std::max(1, row_split(nbr, na / 64));   // (a lane per block: a wave covers 64 of them)
  hipLaunchKernelGGL(algebra_compare, grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, b->row_p, b->col_i, b->blk_p,
                     a->row_blk_size, a->col_blk_size, nbr, S, na, E->alg_i32.p, E->alg_i64.p);
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, E->alg_i32.p, sizeof(int), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 1, E->alg_i64.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  *flags = *reinterpret_cast<const int*>(E->host_scalars);
  *packed_nze = E->host_scalars[1];
  return 0;
}
}  // extern "C++"

int dbcsr_amd_bcsr_add_count(void* handle, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int beta_is_zero, int32_t* dst_row_p, int64_t* nblks,
                             int64_t* nze, int* same_pattern, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !a || !b || !dst_row_p || !nblks || !nze || !same_pattern) return -1;
  if (a->nblkrows != b->nblkrows || a->nblkcols != b->nblkcols) return -1;
  hipStream_t st = stream_of(stream);
  const int nbr = a->nblkrows, nbc = a->nblkcols;
  const int64_t na = a->nblks, nb = beta_is_zero ? 0 : b->nblks;
  E->add_mode = 0;
  E->add_beta_zero = beta_is_zero ? 1 : 0;
  E->add_nblks_a = a->nblks, E->add_nblks_b = b->nblks;
  *nblks = *nze = 0;
  *same_pattern = 0;
  if (E->alg_i32.ensure(4) || E->alg_i64.ensure(8)) return -1;
  // 1. the same pattern at the same offsets, A packed?  (one small kernel, one flag; a saved plan is not touched)
  if (!beta_is_zero && na == nb) {
    int flags = 0;
    int64_t packed_nze = 0;
    if (same_index_packed(E, st, a, b, &flags, &packed_nze)) return -1;
    if (flags == 0) {
      if (dst_row_p != a->row_p) ACC_CHECK(hipMemcpyAsync(dst_row_p, a->row_p, sizeof(int32_t) * ((size_t)nbr + 1), hipMemcpyDeviceToDevice, st));
      E->add_mode = 1;
      *nblks = E->add_nblks = na;
      *nze = E->add_nze = packed_nze;
      *same_pattern = 1;
      return check(hipGetLastError(), "dbcsr_amd_bcsr_add_count", __FILE__, __LINE__);
    }
  }
  // 2. the union pattern, in the symbolic phase's work areas
  plan_invalidate(E);
  E->valid = false;
  engine_takes_work_areas(E);
  const int W = (nbc + 31) / 32;
  const size_t nw = (size_t)nbr * W;
  const int64_t cap = na + nb;   // (no more blocks than both operands have)
  if (E->cin_bm.ensure(nw + 1) || E->b_bm.ensure(nw + 1) || E->c_bm.ensure(nw + 1) || E->cin_pre.ensure(nw + 1) || E->b_pre.ensure(nw + 1) ||
      E->c_pre.ensure(nw + 1) || E->row_nnz.ensure((size_t)nbr + 1) || E->blk_nze.ensure((size_t)cap + 1) || E->c_blk_p_ws.ensure((size_t)cap + 1) ||
      E->dev_scalars.ensure(16))
    return -1;
  int64_t* dsc = reinterpret_cast<int64_t*>(E->dev_scalars.p);
  ACC_CHECK(hipMemsetAsync(dsc, 0, 16 * sizeof(int64_t), st));
  if (nw > 0) {
    ACC_CHECK(hipMemsetAsync(E->cin_bm.p, 0, sizeof(uint32_t) * nw, st));
    if (na > 0) hipLaunchKernelGGL(bitmap_from_index, grid_for((int64_t)nbr * 64), dim3(256), 0, st, a->row_p, a->col_i, nbr, W, E->cin_bm.p);
    if (!beta_is_zero) {
      ACC_CHECK(hipMemsetAsync(E->b_bm.p, 0, sizeof(uint32_t) * nw, st));
      if (nb > 0) hipLaunchKernelGGL(bitmap_from_index, grid_for((int64_t)nbr * 64), dim3(256), 0, st, b->row_p, b->col_i, nbr, W, E->b_bm.p);
      hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, st, E->b_bm.p, nbr, W, E->b_pre.p, (int*)nullptr);
    }
    hipLaunchKernelGGL(algebra_union, grid_for((int64_t)nw), dim3(256), 0, st, E->cin_bm.p, beta_is_zero ? (const uint32_t*)nullptr : E->b_bm.p,
                       (int64_t)nw, E->c_bm.p);
    hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, st, E->cin_bm.p, nbr, W, E->cin_pre.p, (int*)nullptr);
    hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, st, E->c_bm.p, nbr, W, E->c_pre.p, E->row_nnz.p);
  } else if (nbr > 0) {
    ACC_CHECK(hipMemsetAsync(E->row_nnz.p, 0, sizeof(int) * (size_t)nbr, st));
  }
  if (exclusive_scan<int32_t>(E, E->row_nnz.p, nbr, dst_row_p, dsc + 0, true, st)) return -1;
  if (cap > 0 && nw > 0) {
    ACC_CHECK(hipMemsetAsync(E->blk_nze.p, 0, sizeof(int) * (size_t)cap, st));   // (the scan runs over cap entries: those behind the last block count nothing)
    hipLaunchKernelGGL(block_sizes_rows, grid_for((int64_t)nw), dim3(256), 0, st, E->c_bm.p, E->c_pre.p, dst_row_p, a->row_blk_size, a->col_blk_size, nbr,
                       W, E->blk_nze.p);
    if (exclusive_scan<int64_t>(E, E->blk_nze.p, cap, E->c_blk_p_ws.p, dsc + 1, false, st)) return -1;
  }
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, dsc, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  E->add_mode = 2;
  *nblks = E->add_nblks = E->host_scalars[0];
  *nze = E->add_nze = E->host_scalars[1];
  return check(hipGetLastError(), "dbcsr_amd_bcsr_add_count", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_add_apply(void* handle, libsmm_acc_data_t datatype, const double alpha[2], const dbcsr_amd_bcsr* a, const double beta[2],
                             const dbcsr_amd_bcsr* b, dbcsr_amd_bcsr* dst, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !alpha || !a || !beta || !b || !dst) return -1;
  if (!algebra_type(datatype)) return -10;
  const int pending = E->add_mode;
  E->add_mode = 0;
  engine_writes_values(E);
  if (!pending || a->nblks != E->add_nblks_a || b->nblks != E->add_nblks_b || a->nblkrows != b->nblkrows || a->nblkcols != b->nblkcols ||
      dst->nblkrows != a->nblkrows || dst->nblkcols != a->nblkcols)
    return -1;
  hipStream_t st = stream_of(stream);
  const int mode = (algebra_is_one(datatype, alpha) ? kAlphaIsOne : 0) | (algebra_is_one(datatype, beta) ? kBetaIsOne : 0);
  dst->nblks = E->add_nblks;
  if (pending == 1) {   // same pattern: one flat pass, in place when dst is a (the index is then not touched at all)
    if (E->add_nblks == 0) return 0;
    if (dst->col_i != a->col_i) ACC_CHECK(hipMemcpyAsync(dst->col_i, a->col_i, sizeof(int32_t) * (size_t)a->nblks, hipMemcpyDeviceToDevice, st));
    if (dst->blk_p != a->blk_p) ACC_CHECK(hipMemcpyAsync(dst->blk_p, a->blk_p, sizeof(int64_t) * (size_t)a->nblks, hipMemcpyDeviceToDevice, st));
    DBCSR_AMD_BY_TYPE(add_flat_launch, st, a, b, dst, E->add_nze, alpha, beta, mode);
    return check(hipGetLastError(), "dbcsr_amd_bcsr_add_apply", __FILE__, __LINE__);
  }
  plan_invalidate(E);  // this call uses the engine's work areas: the next multiply runs its own symbolic phase
  if (E->add_nblks == 0) return 0;
  if (dst->data == a->data || (!E->add_beta_zero && dst->data == b->data)) return -1;   // the union add is not done in place
  const int nbr = a->nblkrows, W = (a->nblkcols + 31) / 32;
  if (E->prod_start.ensure(2 * (size_t)E->add_nblks + 2)) return -1;
  hipLaunchKernelGGL(algebra_emit, grid_for((int64_t)nbr * W), dim3(256), 0, st, a->row_p, a->blk_p, E->cin_bm.p, E->cin_pre.p, b->row_p, b->blk_p,
                     E->add_beta_zero ? (const uint32_t*)nullptr : E->b_bm.p, E->b_pre.p, E->c_bm.p, E->c_pre.p, dst->row_p, E->c_blk_p_ws.p, nbr, W,
                     dst->col_i, dst->blk_p, E->prod_start.p);
  DBCSR_AMD_BY_TYPE(add_blocks_launch, E, st, a, b, dst, alpha, beta, mode);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_add_apply", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_diag_count(void* handle, const dbcsr_amd_bcsr* m, int32_t* dst_row_p, int32_t* dst_col_i, int64_t* dst_blk_p, int64_t* nblks,
                              int64_t* nze, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !dst_row_p || !nblks || !nze || m->nblkrows != m->nblkcols) return -1;
  hipStream_t st = stream_of(stream);
  const int nbr = m->nblkrows;
  *nblks = *nze = 0;
  if (nbr > 0 && (!dst_col_i || !dst_blk_p)) return -1;
  if (E->alg_i32.ensure(4 + 2 * (size_t)nbr) || E->alg_i64.ensure(8 + (size_t)nbr + 1)) return -1;
  int* need = E->alg_i32.p + 4;
  int* sizes = need + nbr;
  int64_t* off = E->alg_i64.p + 8;
  ACC_CHECK(hipMemsetAsync(E->alg_i64.p, 0, 2 * sizeof(int64_t), st));
  if (nbr > 0)
    hipLaunchKernelGGL(diag_missing, grid_for((int64_t)nbr * 64), dim3(256), 0, st, m->row_p, m->col_i, m->row_blk_size, nbr, need, sizes);
  if (exclusive_scan<int32_t>(E, need, nbr, dst_row_p, E->alg_i64.p + 0, true, st)) return -1;
  if (exclusive_scan<int64_t>(E, sizes, nbr, off, E->alg_i64.p + 1, false, st)) return -1;
  if (nbr > 0) hipLaunchKernelGGL(diag_emit, grid_for(nbr), dim3(256), 0, st, need, dst_row_p, off, nbr, dst_col_i, dst_blk_p);
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, E->alg_i64.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  *nblks = E->host_scalars[0];
  *nze = E->host_scalars[1];
  return check(hipGetLastError(), "dbcsr_amd_bcsr_diag_count", __FILE__, __LINE__);
}

static int diag_any(void* handle, libsmm_acc_data_t datatype, bool fill, const double alpha[2], const dbcsr_amd_bcsr* m, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !alpha || !m || m->nblkrows != m->nblkcols) return -1;
  if (!algebra_type(datatype)) return -10;
  engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  if (m->nblkrows == 0 || m->nblks == 0) return 0;
  DBCSR_AMD_BY_TYPE(diag_launch, st, fill, m, alpha);
  return check(hipGetLastError(), fill ? "dbcsr_amd_bcsr_diag_fill" : "dbcsr_amd_bcsr_diag_shift", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_diag_fill(void* handle, libsmm_acc_data_t datatype, const double alpha[2], dbcsr_amd_bcsr* dst, void* stream) {
  return diag_any(handle, datatype, true, alpha, dst, stream);
}

int dbcsr_amd_bcsr_diag_shift(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, const double alpha[2], void* stream) {
  return diag_any(handle, datatype, false, alpha, m, stream);
}

int dbcsr_amd_bcsr_trace(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, double out[2], void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !out || m->nblkrows != m->nblkcols) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  out[0] = out[1] = 0.0;
  if (m->nblkrows == 0 || m->nblks == 0) return 0;
  const int64_t nw = DBCSR_AMD_BY_TYPE(reduce_launch, E, st, 0, m, 0);
  return reduce_finish(E, st, nw, out, "dbcsr_amd_bcsr_trace");
}

int dbcsr_amd_bcsr_norm2(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int symmetric, double out[1], void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !out) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  out[0] = 0.0;
  if (m->nblkrows == 0 || m->nblks == 0) return 0;
  const int64_t nw = DBCSR_AMD_BY_TYPE(reduce_launch, E, st, 1, m, symmetric ? 1 : 0);
  double two[2] = {0.0, 0.0};
  const int rc = reduce_finish(E, st, nw, two, "dbcsr_amd_bcsr_norm2");
  out[0] = two[0];
  return rc;
}

int dbcsr_amd_bcsr_dot(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int symmetric, double out[1],
                       void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !a || !b || !out || a->nblkrows != b->nblkrows || a->nblkcols != b->nblkcols) return -1;
  if (datatype != dbcsr_type_real_8 && datatype != dbcsr_type_real_4) return -10;   // (complex data: not offered, see the header)
  hipStream_t st = stream_of(stream);
  out[0] = 0.0;
  if (a->nblkrows == 0 || a->nblks == 0 || b->nblks == 0) return 0;
  const int sym = symmetric ? 1 : 0;
  const int64_t nw = datatype == dbcsr_type_real_8 ? dot_launch<double>(E, st, a, b, sym) : dot_launch<float>(E, st, a, b, sym);
  double two[2] = {0.0, 0.0};
  const int rc = reduce_finish(E, st, nw, two, "dbcsr_amd_bcsr_dot");
  out[0] = two[0];
  return rc;
}

// ---- norms and vectors ---------------------------------------------------------------------------------------------------------------------------
// Everything here works in Engine::alg_* and the scan's scratch: no entry invalidates the plan or writes a work area a saved plan depends on.
extern "C++" {
// element offsets of the block rows and columns (roff[nblkrows] / coff[nblkcols]: the full lengths), scanned on the device into alg_i64
static int vector_offsets(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* m, const int64_t** roff, const int64_t** coff) {
  const size_t nbr = (size_t)m->nblkrows, nbc = (size_t)m->nblkcols;
  if (E->alg_i64.ensure(8 + nbr + nbc + 2)) return -1;
  int64_t* r = E->alg_i64.p + 8;
  int64_t* c = r + nbr + 1;
  if (exclusive_scan<int64_t>(E, m->row_blk_size, (int64_t)nbr, r, nullptr, true, st)) return -1;
  if (exclusive_scan<int64_t>(E, m->col_blk_size, (int64_t)nbc, c, nullptr, true, st)) return -1;
  *roff = r;
  *coff = c;
  return 0;
}

// the blocks of every block column in ascending block-row order (alg_col_p, alg_list), as transpose_any forms a transposed index -- in buffers of the algebra
static int col_list_build(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a) {
  const int nbr = a->nblkrows, nbc = a->nblkcols, Wt = (nbr + 31) / 32;
  const size_t nw = (size_t)nbc * Wt;
  if (E->alg_bm.ensure(nw + 1) || E->alg_pre.ensure(nw + 1) || E->alg_cnt.ensure((size_t)nbc + 1) || E->alg_col_p.ensure((size_t)nbc + 2) ||
      E->alg_list.ensure(2 * (size_t)a->nblks + 2))
    return -1;
  ACC_CHECK(hipMemsetAsync(E->alg_bm.p, 0, sizeof(uint32_t) * (nw + 1), st));
  hipLaunchKernelGGL(transpose_mark, grid_for((int64_t)nbr * 64), dim3(256), 0, st, a->row_p, a->col_i, nbr, Wt, E->alg_bm.p);
  hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbc * 64), dim3(256), 0, st, E->alg_bm.p, nbc, Wt, E->alg_pre.p, E->alg_cnt.p);
  if (exclusive_scan<int32_t>(E, E->alg_cnt.p, nbc, E->alg_col_p.p, nullptr, true, st)) return -1;
  hipLaunchKernelGGL(algebra_col_list, grid_for((int64_t)nbr * 64), dim3(256), 0, st, a->row_p, a->col_i, nbr, Wt, E->alg_bm.p, E->alg_pre.p,
                     E->alg_col_p.p, E->alg_list.p);
  return 0;
}

// (the callers made alg_sums hold S * n_out doubles)
template <typename T>
static void row_sums_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, int what, const int64_t* roff, double* out, int64_t n_out) {
  const int nbr = a->nblkrows, S = row_split(nbr, a->nblks);
  hipLaunchKernelGGL((algebra_row_sums<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p,
                     static_cast<const T*>(a->data), a->row_blk_size, a->col_blk_size, roff, nbr, S, what, aligned16(a->data), n_out, E->alg_sums.p);
  hipLaunchKernelGGL(algebra_vec_combine, grid_for(n_out), dim3(256), 0, st, E->alg_sums.p, S, n_out, roff + nbr, out);
}

template <typename T>
static void col_sums_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, int what, int skip_diag, const int64_t* coff, double* out, int64_t n_out) {
  const int nbc = a->nblkcols, S = row_split(nbc, a->nblks);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid_for((int64_t)nbc * S * 64), dim3(256), 0, st, E->alg_col_p.p, E->alg_list.p, a->blk_p, static_cast<const T*>(a->data),
                       a->row_blk_size, a->col_blk_size, coff, nbc, S, what, skip_diag, aligned16(a->data), n_out, E->alg_sums.p);
  };
#ifdef DBCSR_AMD_EXPERIMENTS
  switch (E->ls.alg_col_variant) {   // DBCSR_AMD_ALG_COLSUMS: ablations and the lane-per-column form (mm_algebra.h)
    case 1: launch(algebra_col_sums<T, 1>); break;
    case 2: launch(algebra_col_sums<T, 2>); break;
    case 3: launch(algebra_col_sums<T, 3>); break;
    case 4: launch(algebra_col_sums<T, 4>); break;
    default: launch(algebra_col_sums<T, 0>);
  }
#else
  launch(algebra_col_sums<T, 0>);
#endif
  hipLaunchKernelGGL(algebra_vec_combine, grid_for(n_out), dim3(256), 0, st, E->alg_sums.p, S, n_out, coff + nbc, out);
}

template <typename T>
static void maxabs_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, int S) {
  const int nbr = a->nblkrows;
  hipLaunchKernelGGL((algebra_maxabs<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, static_cast<const T*>(a->data),
                     a->row_blk_size, a->col_blk_size, nbr, S, aligned16(a->data), E->alg_sums.p);
}

template <typename T>
static void diag_vector_launch(hipStream_t st, bool set, const dbcsr_amd_bcsr* m, const int64_t* roff, void* vec, int64_t n) {
  const int nbr = m->nblkrows;
  if (set)
    hipLaunchKernelGGL((diag_set<T>), grid_for((int64_t)nbr * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, m->row_blk_size, m->col_blk_size, roff, nbr,
                       static_cast<const T*>(vec), n, static_cast<T*>(m->data));
  else
    hipLaunchKernelGGL((diag_get<T>), grid_for(((int64_t)nbr + 1) * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, static_cast<const T*>(m->data),
                       m->row_blk_size, m->col_blk_size, roff, nbr, static_cast<T*>(vec), n);
}

template <typename T>
static void scale_by_vector_launch(hipStream_t st, const dbcsr_amd_bcsr* m, const int64_t* offs, int side, const void* vec, int64_t n) {
  const int nbr = m->nblkrows, S = algebra_split(nbr, m->nblks);
  hipLaunchKernelGGL((algebra_scale_by_vector<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, m->row_blk_size,
                     m->col_blk_size, offs, nbr, S, side, static_cast<const T*>(vec), n, static_cast<T*>(m->data), aligned16(m->data));
}

// one double on the device brought to the host (synchronises)
static int scalar_finish(Engine* E, hipStream_t st, const double* dev, double out[1], const char* what) {
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 4, dev, sizeof(double), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  memcpy(out, E->host_scalars + 4, sizeof(double));
  return check(hipGetLastError(), what, __FILE__, __LINE__);
}
}  // extern "C++"

int dbcsr_amd_bcsr_maxabs(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, double out[1], void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !out) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  out[0] = 0.0;
  if (m->nblkrows == 0 || m->nblks == 0) return 0;
  const int S = row_split(m->nblkrows, m->nblks);
  const int64_t nw = (int64_t)m->nblkrows * S;
  if (E->alg_sums.ensure((size_t)nw + 2)) return -1;
  DBCSR_AMD_BY_TYPE(maxabs_launch, E, st, m, S);
  hipLaunchKernelGGL(algebra_max_final, dim3(1), dim3(256), 0, st, E->alg_sums.p, (const double*)nullptr, nw, datatype == dbcsr_type_complex_8 ? 1 : 0,
                     E->alg_sums.p + nw);
  return scalar_finish(E, st, E->alg_sums.p + nw, out, "dbcsr_amd_bcsr_maxabs");
}

int dbcsr_amd_bcsr_row_sums(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int what, double* out, int64_t n_out, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || n_out < 0 || (n_out > 0 && !out) || (what != 0 && what != 1)) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  if (n_out == 0) return 0;
  if (m->nblkrows == 0 || m->nblks == 0) {
    ACC_CHECK(hipMemsetAsync(out, 0, sizeof(double) * (size_t)n_out, st));
    return 0;
  }
  const int64_t *roff = nullptr, *coff = nullptr;
  if (E->alg_sums.ensure((size_t)row_split(m->nblkrows, m->nblks) * n_out + 2) || vector_offsets(E, st, m, &roff, &coff)) return -1;
  DBCSR_AMD_BY_TYPE(row_sums_launch, E, st, m, what, roff, out, n_out);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_row_sums", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_col_sums(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int what, int skip_diagonal_blocks, double* out,
                            int64_t n_out, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || n_out < 0 || (n_out > 0 && !out) || (what != 0 && what != 1)) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  if (n_out == 0) return 0;
  if (m->nblkrows == 0 || m->nblkcols == 0 || m->nblks == 0) {
    ACC_CHECK(hipMemsetAsync(out, 0, sizeof(double) * (size_t)n_out, st));
    return 0;
  }
  const int64_t *roff = nullptr, *coff = nullptr;
  if (E->alg_sums.ensure((size_t)row_split(m->nblkcols, m->nblks) * n_out + 2) || vector_offsets(E, st, m, &roff, &coff) || col_list_build(E, st, m))
    return -1;
  DBCSR_AMD_BY_TYPE(col_sums_launch, E, st, m, what, skip_diagonal_blocks ? 1 : 0, coff, out, n_out);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_col_sums", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_gershgorin(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int symmetric, double out[1], void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !out || (symmetric && m->nblkrows != m->nblkcols)) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  out[0] = 0.0;
  if (m->nblkrows == 0 || m->nblkcols == 0 || m->nblks == 0) return 0;
  const int64_t *roff = nullptr, *coff = nullptr;
  if (vector_offsets(E, st, m, &roff, &coff)) return -1;
  // the full row count sizes the vectors: known from an earlier call with these block sizes, fetched otherwise (then this call synchronises twice)
  int64_t n = -1;
  if (m->index_stamp != 0)
    for (const Engine::AlgLen& k : E->alg_len)
      if (k.stamp == m->index_stamp && k.rs == m->row_blk_size && k.cs == m->col_blk_size && k.nbr == m->nblkrows && k.nbc == m->nblkcols) n = k.rows;
  if (n < 0) {
    ACC_CHECK(hipMemcpyAsync(E->host_scalars + 6, roff + m->nblkrows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipStreamSynchronize(st));
    n = E->host_scalars[6];
    if (m->index_stamp != 0) {
      Engine::AlgLen& k = E->alg_len[E->alg_len_next];
      E->alg_len_next = (E->alg_len_next + 1) % Engine::kAlgLens;
      k.rs = m->row_blk_size, k.cs = m->col_blk_size, k.stamp = m->index_stamp, k.nbr = m->nblkrows, k.nbc = m->nblkcols, k.rows = n, k.cols = -1;
    }
  }
  if (n <= 0) return 0;
  const int S = std::max(row_split(m->nblkrows, m->nblks), symmetric ? row_split(m->nblkcols, m->nblks) : 1);
  if (E->alg_vec.ensure(2 * (size_t)n + 2) || E->alg_sums.ensure((size_t)S * n + 2)) return -1;
  double* rows = E->alg_vec.p;
  double* cols = symmetric ? rows + n : nullptr;
  if (symmetric && col_list_build(E, st, m)) return -1;
  DBCSR_AMD_BY_TYPE(row_sums_launch, E, st, m, 0, roff, rows, n);
  if (symmetric) DBCSR_AMD_BY_TYPE(col_sums_launch, E, st, m, 0, 1, coff, cols, n);   // the twins of the stored blocks off the diagonal
  hipLaunchKernelGGL(algebra_max_final, dim3(1), dim3(256), 0, st, rows, (const double*)cols, n, 0, rows + 2 * n);
  return scalar_finish(E, st, rows + 2 * n, out, "dbcsr_amd_bcsr_gershgorin");
}

static int diag_vector(void* handle, libsmm_acc_data_t datatype, bool set, const dbcsr_amd_bcsr* m, void* vec, int64_t n, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || n < 0 || (n > 0 && !vec) || m->nblkrows != m->nblkcols) return -1;
  if (!algebra_type(datatype)) return -10;
  if (set) engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  if (n == 0) return 0;
  if (m->nblkrows == 0 || m->nblks == 0) {
    if (!set) ACC_CHECK(hipMemsetAsync(vec, 0, algebra_esize(datatype) * (size_t)n, st));
    return 0;
  }
  const int64_t *roff = nullptr, *coff = nullptr;
  if (vector_offsets(E, st, m, &roff, &coff)) return -1;
  DBCSR_AMD_BY_TYPE(diag_vector_launch, st, set, m, roff, vec, n);
  return check(hipGetLastError(), set ? "dbcsr_amd_bcsr_set_diag" : "dbcsr_amd_bcsr_get_diag", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_get_diag(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, void* diag, int64_t n, void* stream) {
  return diag_vector(handle, datatype, false, m, diag, n, stream);
}

int dbcsr_amd_bcsr_set_diag(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, const void* diag, int64_t n, void* stream) {
  return diag_vector(handle, datatype, true, m, const_cast<void*>(diag), n, stream);
}

int dbcsr_amd_bcsr_scale_by_vector(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, const void* vec, int64_t n, int side, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || n < 0 || (n > 0 && !vec) || (side != 0 && side != 1)) return -1;
  if (!algebra_type(datatype)) return -10;
  engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  if (n == 0 || m->nblkrows == 0 || m->nblks == 0) return 0;
  const int64_t *roff = nullptr, *coff = nullptr;
  if (vector_offsets(E, st, m, &roff, &coff)) return -1;
  DBCSR_AMD_BY_TYPE(scale_by_vector_launch, st, m, side ? coff : roff, side, vec, n);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_scale_by_vector", __FILE__, __LINE__);
}
// ---- matrix-vector product ---------------------------------------------------------------------------------------------------------------------------
extern "C++" {
// one pass over the stored blocks: by block row (y per row of A, x per column) or by block column (y per column of A, x per row)
struct MatvecPass {
  int on, skip_diag, conj;
  double sign;
};

// The passes of y <- op(F) x, F the matrix the index stands for.  No symmetry (kind -1): F = A, one pass.  A stored triangle (kind = bit 0 negates, bit 1
// conjugates the twin: S 0, A 1, H 2, K 3; g = conjugate with bit 1, s = -1 with bit 0): block (r, c), r != c, stands for F_rc = a and F_cr = s g(a)^T,
// a diagonal block for itself.
//            rows: y_r += ... x_c                   cols: y_c += ... x_r
//   op N     a            every block               s g(a)^T     off the diagonal
//   op T     s g(a)       off the diagonal          a^T          every block
//   op C     s conj g(a)  off the diagonal          conj(a)^T    every block
static void matvec_passes(int kind, char op, MatvecPass* rows, MatvecPass* cols) {
  const int g = kind >= 0 ? (kind >> 1) & 1 : 0;
  const double s = kind >= 0 && (kind & 1) ? -1.0 : 1.0;
  const MatvecPass off = {0, 0, 0, 1.0};
  if (op == 'N') {
    *rows = MatvecPass{1, 0, 0, 1.0};
    *cols = kind >= 0 ? MatvecPass{1, 1, g, s} : off;
  } else {
    const int c = op == 'C' ? 1 : 0;
    *cols = MatvecPass{1, 0, c, 1.0};
    *rows = kind >= 0 ? MatvecPass{1, 1, g ^ c, s} : off;
  }
}

// (the caller made alg_sums hold (S_r + S_c) n_y sums, the column list when the column pass is on, and the offsets)
template <typename T>
static void matvec_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const MatvecPass& rp, const MatvecPass& cp, int S_r, int S_c,
                          const int64_t* roff, const int64_t* coff, const int64_t* total, const double alpha[2], const double beta[2], int mode,
                          const void* x, int64_t n_x, void* y, int64_t n_y) {
  using Acc = typename MatvecAcc<T>::type;
  Acc* sums = reinterpret_cast<Acc*>(E->alg_sums.p);
  const int nbr = a->nblkrows, nbc = a->nblkcols, vec_ok = aligned16(a->data);
  if (S_r > 0)
    hipLaunchKernelGGL((algebra_matvec_rows<T>), grid_for((int64_t)nbr * S_r * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p,
                       static_cast<const T*>(a->data), a->row_blk_size, a->col_blk_size, roff, coff, nbr, S_r, rp.conj, rp.skip_diag, vec_ok,
                       static_cast<const T*>(x), n_x, n_y, sums);
  if (S_c > 0)
    hipLaunchKernelGGL((algebra_matvec_cols<T>), grid_for((int64_t)nbc * S_c * 64), dim3(256), 0, st, E->alg_col_p.p, E->alg_list.p, a->blk_p,
                       static_cast<const T*>(a->data), a->row_blk_size, a->col_blk_size, coff, roff, nbc, S_c, cp.conj, cp.skip_diag, vec_ok,
                       static_cast<const T*>(x), n_x, n_y, sums + (size_t)S_r * n_y);
  hipLaunchKernelGGL((algebra_matvec_combine<T>), grid_for(n_y), dim3(256), 0, st, sums, S_r, S_c, rp.sign, cp.sign, n_y, total,
                     algebra_scalar<Acc>(alpha), algebra_scalar<Acc>(beta), mode, static_cast<T*>(y));
}
}  // extern "C++"

int dbcsr_amd_bcsr_matvec(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], const dbcsr_amd_bcsr* a, int kind, const void* x,
                          int64_t n_x, const double beta[2], void* y, int64_t n_y, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !alpha || !a || !beta || n_x < 0 || n_y < 0 || (n_x > 0 && !x) || (n_y > 0 && !y)) return -1;
  if (!matvec_args_ok(trans, kind, a)) return -1;
  if (!algebra_type(datatype)) return -10;
  const size_t esize = algebra_esize(datatype);
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
  if (n_x > 0 && n_y > 0 && x0 < y0 + esize * (size_t)n_y && y0 < x0 + esize * (size_t)n_x) return -1;   // x and y must not overlap
  hipStream_t st = stream_of(stream);
  if (n_y == 0 || a->nblkrows == 0 || a->nblkcols == 0) return 0;   // (no full row: nothing to write)
  const bool zc = datatype == dbcsr_type_complex_8;
  bool product = false;   // alpha == 0: A and x are not read; an empty matrix: y <- beta y
  const int mode = product_mode(datatype, alpha, beta, a->nblks > 0, &product);
  MatvecPass rp = {0, 0, 0, 1.0}, cp = rp;
  if (product) matvec_passes(kind, trans, &rp, &cp);
  const int S_r = rp.on ? row_split(a->nblkrows, a->nblks) : 0, S_c = cp.on ? row_split(a->nblkcols, a->nblks) : 0;
  const int64_t *roff = nullptr, *coff = nullptr;
  if (E->alg_sums.ensure((size_t)(S_r + S_c) * (size_t)n_y * (zc ? 2 : 1) + 2) || vector_offsets(E, st, a, &roff, &coff)) return -1;
  if (cp.on && col_list_build(E, st, a)) return -1;
  const int64_t* total = trans == 'N' ? roff + a->nblkrows : coff + a->nblkcols;   // the full rows of op(A)
  DBCSR_AMD_BY_TYPE(matvec_launch, E, st, a, rp, cp, S_r, S_c, roff, coff, total, alpha, beta, mode, x, n_x, y, n_y);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_matvec", __FILE__, __LINE__);
}

// ---- matrix times several dense vectors (kernels: mm_multivec.h) ---------------------------------------------------------------------------------------
extern "C++" {
// Waves per block row / column of the multivec passes.  A unit of (block row, sub) already brings one wave per tile of 16 right-hand sides, so row_split's
// S is divided by the tile count: the number of waves stays near row_split's target, and with it the volume of the partial matrices (S n_y nrhs sums:
// config 2's product, fp64, 47 partials at nrhs 16, 12 at nrhs 64 -- about 200 MB either way, 2.3 % of A's bytes, where 47 at nrhs 64 would be 9 %).
static inline int multivec_split(int64_t nb, int64_t nblks, int ntiles) {
  return std::max(1, (row_split(nb, nblks) + ntiles - 1) / ntiles);
}

// (the caller made alg_sums hold (S_r + S_c) n_y nrhs sums, the column list when the column pass is on, and the offsets)
template <typename T>
static void multivec_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const MatvecPass& rp, const MatvecPass& cp, int S_r, int S_c,
                            const int64_t* roff, const int64_t* coff, const int64_t* total, const double alpha[2], const double beta[2], int mode,
                            int nrhs, const void* x, int64_t n_x, int64_t ldx, void* y, int64_t n_y, int64_t ldy) {
  using Acc = typename MatvecAcc<T>::type;
  Acc* sums = reinterpret_cast<Acc*>(E->alg_sums.p);
  const int nbr = a->nblkrows, nbc = a->nblkcols, vec_ok = aligned16(a->data);
  int wmax = kMultivecWaves;
#ifdef DBCSR_AMD_EXPERIMENTS
  if (E->ls.multivec_waves >= 1 && E->ls.multivec_waves <= kMultivecWaves) wmax = E->ls.multivec_waves;   // DBCSR_AMD_MULTIVEC_WAVES (1: independent waves)
#endif
  const int ntiles = (nrhs + kMultivecTile - 1) / kMultivecTile, W = std::min(ntiles, wmax), G = (ntiles + W - 1) / W;
  const size_t lds = (size_t)W * (kMultivecABytes + kMultivecXBytes);
  if (S_r > 0)
    hipLaunchKernelGGL((algebra_multivec_rows<T>), dim3((unsigned)((int64_t)nbr * S_r * G)), dim3(64 * W), lds, st, a->row_p, a->col_i, a->blk_p,
                       static_cast<const T*>(a->data), a->row_blk_size, a->col_blk_size, roff, coff, nbr, S_r, G, rp.conj, rp.skip_diag, vec_ok,
                       static_cast<const T*>(x), n_x, ldx, nrhs, n_y, sums);
  if (S_c > 0)
    hipLaunchKernelGGL((algebra_multivec_cols<T>), dim3((unsigned)((int64_t)nbc * S_c * G)), dim3(64 * W), lds, st, E->alg_col_p.p, E->alg_list.p, a->blk_p,
                       static_cast<const T*>(a->data), a->row_blk_size, a->col_blk_size, coff, roff, nbc, S_c, G, cp.conj, cp.skip_diag, vec_ok,
                       static_cast<const T*>(x), n_x, ldx, nrhs, n_y, sums + (size_t)S_r * (size_t)n_y * nrhs);
  hipLaunchKernelGGL((algebra_multivec_combine<T>), grid_for(n_y * nrhs), dim3(256), 0, st, sums, S_r, S_c, rp.sign, cp.sign, n_y, nrhs, ldy, total,
                     algebra_scalar<Acc>(alpha), algebra_scalar<Acc>(beta), mode, static_cast<T*>(y));
}
}  // extern "C++"

int dbcsr_amd_bcsr_multivec(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], const dbcsr_amd_bcsr* a, int kind, int nrhs,
                            const void* x, int64_t n_x, int64_t ldx, const double beta[2], void* y, int64_t n_y, int64_t ldy, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !alpha || !a || !beta || n_x < 0 || n_y < 0 || nrhs < 0 || ldx < nrhs || ldy < nrhs) return -1;
  if (nrhs > 0 && ((n_x > 0 && !x) || (n_y > 0 && !y))) return -1;
  if (!matvec_args_ok(trans, kind, a)) return -1;
  if (!algebra_type(datatype)) return -10;
  const size_t esize = algebra_esize(datatype);
  if (nrhs > 0 && n_x > 0 && n_y > 0) {   // the element ranges of X and Y must not overlap
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
    const uintptr_t x1 = x0 + esize * ((size_t)(n_x - 1) * (size_t)ldx + (size_t)nrhs), y1 = y0 + esize * ((size_t)(n_y - 1) * (size_t)ldy + (size_t)nrhs);
    if (x0 < y1 && y0 < x1) return -1;
  }
  hipStream_t st = stream_of(stream);
  if (nrhs == 0 || n_y == 0 || a->nblkrows == 0 || a->nblkcols == 0) return 0;   // (no element of Y below the full length: nothing to write)
  const bool zc = datatype == dbcsr_type_complex_8;
  bool product = false;   // alpha == 0: A and X are not read; an empty matrix: Y <- beta Y
  const int mode = product_mode(datatype, alpha, beta, a->nblks > 0, &product);
  MatvecPass rp = {0, 0, 0, 1.0}, cp = rp;
  if (product) matvec_passes(kind, trans, &rp, &cp);
  const int ntiles = (nrhs + kMultivecTile - 1) / kMultivecTile, G = ntiles;   // (workgroups per block row and sub: at most one per tile)
  const int S_r = rp.on ? multivec_split(a->nblkrows, a->nblks, ntiles) : 0, S_c = cp.on ? multivec_split(a->nblkcols, a->nblks, ntiles) : 0;
  if ((int64_t)std::max(a->nblkrows, a->nblkcols) * std::max(S_r, S_c) * G > INT32_MAX || n_y > (int64_t)INT32_MAX * 256 / nrhs) return -1;   // (the grids)
  const int64_t *roff = nullptr, *coff = nullptr;
  if (E->alg_sums.ensure((size_t)(S_r + S_c) * (size_t)n_y * (size_t)nrhs * (zc ? 2 : 1) + 2) || vector_offsets(E, st, a, &roff, &coff)) return -1;
  if (cp.on && col_list_build(E, st, a)) return -1;
  const int64_t* total = trans == 'N' ? roff + a->nblkrows : coff + a->nblkcols;   // the full rows of op(A)
  DBCSR_AMD_BY_TYPE(multivec_launch, E, st, a, rp, cp, S_r, S_c, roff, coff, total, alpha, beta, mode, nrhs, x, n_x, ldx, y, n_y, ldy);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_multivec", __FILE__, __LINE__);
}

// ---- rank-k update on the stored pattern (kernels: mm_rank_update.h) ------------------------------------------------------------------------------------
extern "C++" {
// 16-byte loads of a row-by-row tensor: its first element and every row start on a 16-byte boundary
template <typename T>
static inline int rank_update_vec_ok(const void* p, int64_t ld) {
  return aligned16(p) && (ld * (int64_t)sizeof(T)) % 16 == 0 ? 1 : 0;
}

template <typename T>
static void rank_update_launch(hipStream_t st, dbcsr_amd_bcsr* a, const int64_t* roff, const int64_t* coff, int conj, const double alpha[2],
                               const double beta[2], int mode, int nrhs, const void* x, int64_t n_x, int64_t ldx, const void* y, int64_t n_y, int64_t ldy) {
  using Acc = typename MatvecAcc<T>::type;
  const int nbr = a->nblkrows, S = algebra_split(nbr, a->nblks), beta_zero = (mode & kMatvecBetaZero) ? 1 : 0;
  if (mode & kMatvecNoProduct)
    hipLaunchKernelGGL((algebra_rank_update_scale<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p,
                       static_cast<T*>(a->data), a->row_blk_size, a->col_blk_size, roff, coff, nbr, S, beta_zero, n_x, n_y, algebra_scalar<T>(beta));
  else
    hipLaunchKernelGGL((algebra_rank_update_blocks<T>), grid_for((int64_t)nbr * S * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p,
                       static_cast<T*>(a->data), a->row_blk_size, a->col_blk_size, roff, coff, nbr, S, conj, beta_zero, static_cast<const T*>(x), n_x, ldx,
                       rank_update_vec_ok<T>(x, ldx), static_cast<const T*>(y), n_y, ldy, rank_update_vec_ok<T>(y, ldy), nrhs, algebra_scalar<Acc>(alpha),
                       algebra_scalar<Acc>(beta));
}
}  // extern "C++"

int dbcsr_amd_bcsr_rank_update(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], int nrhs, const void* x, int64_t n_x,
                               int64_t ldx, const void* y, int64_t n_y, int64_t ldy, const double beta[2], dbcsr_amd_bcsr* a, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !alpha || !a || !beta || n_x < 0 || n_y < 0 || nrhs < 0 || ldx < nrhs || ldy < nrhs) return -1;
  if (trans != 'T' && trans != 'C') return -1;
  if (!algebra_type(datatype)) return -10;
  bool product = false;   // alpha == 0 or no column: X and Y are not read, A <- beta A
  const int mode = product_mode(datatype, alpha, beta, nrhs > 0, &product);
  if (product && ((n_x > 0 && !x) || (n_y > 0 && !y))) return -1;
  engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  if (a->nblkrows == 0 || a->nblkcols == 0 || a->nblks == 0) return 0;   // an empty matrix: nothing to write
  if (n_x == 0 || n_y == 0) return 0;                                      // (no element has both its rows)
  if (!product && algebra_is_one(datatype, beta)) return 0;               // A <- A: nothing is launched
  const int64_t *roff = nullptr, *coff = nullptr;
  if (vector_offsets(E, st, a, &roff, &coff)) return -1;
  DBCSR_AMD_BY_TYPE(rank_update_launch, st, a, roff, coff, datatype == dbcsr_type_complex_8 && trans == 'C' ? 1 : 0, alpha, beta, mode, nrhs, x, n_x, ldx, y, n_y, ldy);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_rank_update", __FILE__, __LINE__);
}

// ---- matrix times a dense matrix on the MFMA (kernels: mm_spmm.h) ----------------------------------------------------------------------------------------
extern "C++" {
static inline int spmm_pass_bits(const MatvecPass& p) {
  return (p.on ? kSpmmRowsOn : 0) | (p.skip_diag ? kSpmmSkipDiag : 0) | (p.conj ? kSpmmConj : 0) | (p.sign < 0.0 ? kSpmmNegate : 0);
}

// (the caller built the offsets, and the column list when the column pass is on)
template <typename T>
static void spmm_launch(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const MatvecPass& rp, const MatvecPass& cp, const int64_t* roff,
                        const int64_t* coff, const int64_t* total, const double alpha[2], const double beta[2], int mode, int ncol, const void* x,
                        int64_t n_x, int64_t ldx, void* y, int64_t n_y, int64_t ldy, int layout) {
  using Acc = typename MatvecAcc<T>::type;
  const int beta_zero = (mode & kMatvecBetaZero) ? 1 : 0;
  if (mode & kMatvecNoProduct) {
    hipLaunchKernelGGL((spmm_scale<T>), grid_for(n_y * ncol), dim3(256), 0, st, static_cast<T*>(y), n_y, ncol, ldy, layout, total, algebra_scalar<T>(beta),
                       beta_zero);
    return;
  }
  const int nb = rp.on ? a->nblkrows : a->nblkcols, G = (ncol + kSpmmCols - 1) / kSpmmCols;
  const int* col_p = cp.on ? E->alg_col_p.p : nullptr;
  const int* list = cp.on ? E->alg_list.p : nullptr;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((int64_t)nb * G)), dim3(256), 0, st, a->row_p, a->col_i, col_p, list, a->blk_p, static_cast<const T*>(a->data),
                       a->row_blk_size, a->col_blk_size, roff, coff, nb, G, spmm_pass_bits(rp), spmm_pass_bits(cp), aligned16(a->data),
                       static_cast<const T*>(x), n_x, ldx, static_cast<T*>(y), n_y, ldy, ncol, algebra_scalar<Acc>(alpha), algebra_scalar<Acc>(beta),
                       beta_zero);
  };
  if (layout == 0) launch(spmm_product<T, 0>);
  else launch(spmm_product<T, 1>);
}
}  // extern "C++"

int dbcsr_amd_bcsr_multiply_dense(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], const dbcsr_amd_bcsr* a, int kind, int ncol,
                                  const void* x, int64_t n_x, int64_t ldx, const double beta[2], void* y, int64_t n_y, int64_t ldy, int layout,
                                  void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !alpha || !a || !beta || n_x < 0 || n_y < 0 || ncol < 0 || (layout != 0 && layout != 1)) return -1;
  if (layout == 0 ? (ldx < ncol || ldy < ncol) : (ldx < n_x || ldy < n_y)) return -1;
  if (ncol > 0 && ((n_x > 0 && !x) || (n_y > 0 && !y))) return -1;
  if (!matvec_args_ok(trans, kind, a)) return -1;
  if (!algebra_type(datatype)) return -10;
  const size_t esize = algebra_esize(datatype);
  if (ncol > 0 && n_x > 0 && n_y > 0) {   // the element ranges of X and Y must not overlap
    const size_t ex = layout == 0 ? (size_t)(n_x - 1) * (size_t)ldx + (size_t)ncol : (size_t)(ncol - 1) * (size_t)ldx + (size_t)n_x;
    const size_t ey = layout == 0 ? (size_t)(n_y - 1) * (size_t)ldy + (size_t)ncol : (size_t)(ncol - 1) * (size_t)ldy + (size_t)n_y;
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
    if (x0 < y0 + esize * ey && y0 < x0 + esize * ex) return -1;
  }
  hipStream_t st = stream_of(stream);
  if (ncol == 0 || n_y == 0 || a->nblkrows == 0 || a->nblkcols == 0) return 0;   // (no element of Y below the full length: nothing to write)
  bool product = false;   // alpha == 0: A and X are not read; an empty matrix: Y <- beta Y
  const int mode = product_mode(datatype, alpha, beta, a->nblks > 0, &product);
  MatvecPass rp = {0, 0, 0, 1.0}, cp = rp;
  if (product) matvec_passes(kind, trans, &rp, &cp);
  const int64_t G = ((int64_t)ncol + kSpmmCols - 1) / kSpmmCols;
  if ((int64_t)std::max(a->nblkrows, a->nblkcols) * G > INT32_MAX || n_y > (int64_t)INT32_MAX * 256 / ncol) return -1;   // (the grids)
  const int64_t *roff = nullptr, *coff = nullptr;
  if (vector_offsets(E, st, a, &roff, &coff)) return -1;
  if (cp.on && col_list_build(E, st, a)) return -1;
  const int64_t* total = trans == 'N' ? roff + a->nblkrows : coff + a->nblkcols;   // the full rows of op(A)
  DBCSR_AMD_BY_TYPE(spmm_launch, E, st, a, rp, cp, roff, coff, total, alpha, beta, mode, ncol, x, n_x, ldx, y, n_y, ldy, layout);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_multiply_dense", __FILE__, __LINE__);
}
// ---- block diagonal (kernels: mm_block_inverse.h) ---------------------------------------------------------------------------------------------------------
extern "C++" {
template <typename T>
static void block_diag_copy_launch(hipStream_t st, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst) {
  hipLaunchKernelGGL((block_diag_copy<T>), grid_for((int64_t)src->nblkrows * 64), dim3(256), 0, st, src->row_p, src->col_i, src->blk_p,
                     static_cast<const T*>(src->data), dst->row_p, dst->col_i, dst->blk_p, static_cast<T*>(dst->data), src->row_blk_size, src->col_blk_size,
                     src->nblkrows, aligned16(dst->data));
}

// more than 64 KB of dynamic LDS needs the attribute, once per kernel
template <typename K>
static int block_inverse_allow_lds(K kernel, size_t bytes, bool* done) {
  if (*done || bytes <= 65536) return 0;
  ACC_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  *done = true;
  return 0;
}

// the wave kernel over every block row (it also counts the skipped blocks), and the workgroup kernel when a block above 32 may be there
template <typename T>
static int block_inverse_launch(hipStream_t st, dbcsr_amd_bcsr* m, int max_dim, unsigned long long* info) {
  using Acc = typename MatvecAcc<T>::type;
  static bool wave_lds = false, wide_lds = false;
  const int nbr = m->nblkrows, vec_ok = aligned16(m->data);
  const int nmax = std::max(1, std::min(max_dim, kBlockInverseWaveDim));
  if (block_inverse_allow_lds(block_inverse_wave<T>, 4 * block_inverse_lds_bytes<Acc>(kBlockInverseWaveDim), &wave_lds)) return -1;
  hipLaunchKernelGGL((block_inverse_wave<T>), grid_for((int64_t)nbr * 64), dim3(256), 4 * block_inverse_lds_bytes<Acc>(nmax), st, m->row_p, m->col_i,
                     m->blk_p, static_cast<T*>(m->data), m->row_blk_size, m->col_blk_size, nbr, nmax, max_dim, vec_ok, info);
  if (max_dim > kBlockInverseWaveDim) {
    if (block_inverse_allow_lds(block_inverse_wide<T>, block_inverse_lds_bytes<Acc>(kBlockInverseMaxDim), &wide_lds)) return -1;
    hipLaunchKernelGGL((block_inverse_wide<T>), dim3((unsigned)nbr), dim3(256), block_inverse_lds_bytes<Acc>(max_dim), st, m->row_p, m->col_i, m->blk_p,
                       static_cast<T*>(m->data), m->row_blk_size, m->col_blk_size, nbr, max_dim, vec_ok, info);
  }
  return 0;
}
}  // extern "C++"

int dbcsr_amd_bcsr_block_diag_count(void* handle, const dbcsr_amd_bcsr* m, int32_t* dst_row_p, int32_t* dst_col_i, int64_t* dst_blk_p, int64_t* nblks,
                                    int64_t* nze, int32_t* max_dim, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || !dst_row_p || !nblks || !nze || !max_dim || m->nblkrows != m->nblkcols) return -1;
  hipStream_t st = stream_of(stream);
  const int nbr = m->nblkrows;
  *nblks = *nze = 0;
  *max_dim = 0;
  if (nbr > 0 && (!dst_col_i || !dst_blk_p)) return -1;
  if (E->alg_i32.ensure(4 + 2 * (size_t)nbr) || E->alg_i64.ensure(8 + (size_t)nbr + 1)) return -1;
  int* have = E->alg_i32.p + 4;
  int* sizes = have + nbr;
  int64_t* off = E->alg_i64.p + 8;
  ACC_CHECK(hipMemsetAsync(E->alg_i64.p, 0, 2 * sizeof(int64_t), st));
  ACC_CHECK(hipMemsetAsync(E->alg_i32.p, 0, sizeof(int), st));
  if (nbr > 0)
    hipLaunchKernelGGL(block_diag_find, grid_for((int64_t)nbr * 64), dim3(256), 0, st, m->row_p, m->col_i, m->row_blk_size, m->col_blk_size, nbr, have, sizes,
                       E->alg_i32.p);
  if (exclusive_scan<int32_t>(E, have, nbr, dst_row_p, E->alg_i64.p + 0, true, st)) return -1;
  if (exclusive_scan<int64_t>(E, sizes, nbr, off, E->alg_i64.p + 1, false, st)) return -1;
  if (nbr > 0) hipLaunchKernelGGL(diag_emit, grid_for(nbr), dim3(256), 0, st, have, dst_row_p, off, nbr, dst_col_i, dst_blk_p);
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, E->alg_i64.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 2, E->alg_i32.p, sizeof(int), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  *nblks = E->host_scalars[0];
  *nze = E->host_scalars[1];
  *max_dim = *reinterpret_cast<const int*>(E->host_scalars + 2);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_block_diag_count", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_block_diag_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !src || !dst || src->nblkrows != src->nblkcols || dst->nblkrows != src->nblkrows || dst->nblkcols != src->nblkcols) return -1;
  if (!algebra_type(datatype)) return -10;
  if (dst->nblks > 0 && dst->data == src->data) return -1;   // (a copy between two data areas)
  engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  if (src->nblkrows == 0 || src->nblks == 0 || dst->nblks == 0) return 0;
  DBCSR_AMD_BY_TYPE(block_diag_copy_launch, st, src, dst);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_block_diag_apply", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_block_diag_invert(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, int max_dim, int64_t info[3], void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || m->nblkrows != m->nblkcols || max_dim < 0) return -1;
  if (!algebra_type(datatype)) return -10;
  if (max_dim > kBlockInverseMaxDim) return -11;
  if (info) info[0] = 0, info[1] = -1, info[2] = 0;
  engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  if (m->nblkrows == 0 || m->nblks == 0) return 0;
  if (E->alg_i64.ensure(8)) return -1;
  // [0] singular blocks, [1] the first of their block rows (all ones: none yet), [2] skipped blocks
  unsigned long long* dev = reinterpret_cast<unsigned long long*>(E->alg_i64.p);
  ACC_CHECK(hipMemsetAsync(dev, 0, 3 * sizeof(int64_t), st));
  ACC_CHECK(hipMemsetAsync(dev + 1, 0xff, sizeof(int64_t), st));
  if (DBCSR_AMD_BY_TYPE(block_inverse_launch, st, m, max_dim, dev)) return -1;
  if (info) {
    ACC_CHECK(hipMemcpyAsync(E->host_scalars, dev, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipStreamSynchronize(st));
    info[0] = E->host_scalars[0];
    info[1] = E->host_scalars[0] > 0 ? E->host_scalars[1] : -1;
    info[2] = E->host_scalars[2];
  }
  return check(hipGetLastError(), "dbcsr_amd_bcsr_block_diag_invert", __FILE__, __LINE__);
}
// ---- block diagonal times matrix (kernels: mm_block_scale.h) -------------------------------------------------------------------------------------------------
extern "C++" {
// waves per block row: about one stored block per wave (a block is ceil(len / 16) strips of up to six MFMA tiles each -- work enough for a wave)
static inline int block_scale_split(int64_t nbr, int64_t nblks) {
  if (nbr <= 0) return 1;
  return (int)std::max<int64_t>(1, std::min<int64_t>((nblks + nbr - 1) / nbr, 1024));
}

template <typename T>
static void block_scale_launch(hipStream_t st, const dbcsr_amd_bcsr* diag, dbcsr_amd_bcsr* m, int left, int tr, int conj, bool zero, const double alpha[2]) {
  using Acc = typename MatvecAcc<T>::type;
  const int nbr = m->nblkrows, S = block_scale_split(nbr, m->nblks);
  const dim3 grid = grid_for((int64_t)nbr * S * 64);
  if (zero)
    hipLaunchKernelGGL((block_scale_zero<T>), grid, dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, static_cast<T*>(m->data), m->row_blk_size,
                       m->col_blk_size, nbr, S);
  else if (left)
    hipLaunchKernelGGL((block_scale_left<T>), grid, dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, static_cast<T*>(m->data), m->row_blk_size,
                       m->col_blk_size, diag->row_p, diag->col_i, diag->blk_p, static_cast<const T*>(diag->data), nbr, S, tr, conj,
                       algebra_scalar<Acc>(alpha));
  else
    hipLaunchKernelGGL((block_scale_right<T>), grid, dim3(256), 0, st, m->row_p, m->col_i, m->blk_p, static_cast<T*>(m->data), m->row_blk_size,
                       m->col_blk_size, diag->row_p, diag->col_i, diag->blk_p, static_cast<const T*>(diag->data), nbr, S, tr, conj,
                       algebra_scalar<Acc>(alpha));
}
}  // extern "C++"

int dbcsr_amd_bcsr_block_diag_multiply(void* handle, libsmm_acc_data_t datatype, char side, char trans, const double alpha[2], const dbcsr_amd_bcsr* diag,
                                       dbcsr_amd_bcsr* m, int max_dim, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !alpha || !diag || !m || max_dim < 0 || diag->nblkrows != diag->nblkcols) return -1;
  if (side != 'L' && side != 'R') return -1;
  if (trans != 'N' && trans != 'T' && trans != 'C' && trans != 'J') return -1;
  if (diag->nblkrows != (side == 'L' ? m->nblkrows : m->nblkcols)) return -1;
  if (!algebra_type(datatype)) return -10;
  if (max_dim > kBlockScaleMaxDim) return -11;
  if (m->nblks > 0 && diag->nblks > 0 && diag->data == m->data) return -1;   // (in place on m: the operand is another data area)
  engine_writes_values(E);
  hipStream_t st = stream_of(stream);
  if (m->nblkrows == 0 || m->nblkcols == 0 || m->nblks == 0) return 0;   // an empty matrix: nothing to write
  const bool zc = datatype == dbcsr_type_complex_8;
  const int tr = trans == 'T' || trans == 'C' ? 1 : 0, conj = zc && (trans == 'C' || trans == 'J') ? 1 : 0;
  DBCSR_AMD_BY_TYPE(block_scale_launch, st, diag, m, side == 'L' ? 1 : 0, tr, conj, algebra_is_zero(datatype, alpha), alpha);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_block_diag_multiply", __FILE__, __LINE__);
}
// ---- dense conversion (kernels: mm_dense.h) -----------------------------------------------------------------------------------------------------------------
// Everything here works in Engine::alg_i32 / alg_i64 and the scan's scratch: no entry invalidates the plan or writes a work area of the symbolic phase.
extern "C++" {
// The full row and column counts of m's block sizes, which only the device knows: remembered per set of block sizes as dbcsr_amd_bcsr_gershgorin remembers
// its row count (same size arrays, same non-zero index_stamp), fetched otherwise -- then, and only then, the call synchronises.
static int dense_lengths(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* m, const int64_t* roff, const int64_t* coff, int64_t* rows, int64_t* cols) {
  if (m->index_stamp != 0)
    for (const Engine::AlgLen& k : E->alg_len)
      if (k.stamp == m->index_stamp && k.rs == m->row_blk_size && k.cs == m->col_blk_size && k.nbr == m->nblkrows && k.nbc == m->nblkcols && k.cols >= 0) {
        *rows = k.rows, *cols = k.cols;
        return 0;
      }
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 6, roff + m->nblkrows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 7, coff + m->nblkcols, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  *rows = E->host_scalars[6], *cols = E->host_scalars[7];
  if (m->index_stamp != 0) {
    Engine::AlgLen& k = E->alg_len[E->alg_len_next];
    E->alg_len_next = (E->alg_len_next + 1) % Engine::kAlgLens;
    k.rs = m->row_blk_size, k.cs = m->col_blk_size, k.stamp = m->index_stamp, k.nbr = m->nblkrows, k.nbc = m->nblkcols, k.rows = *rows, k.cols = *cols;
  }
  return 0;
}

// what the three entries ask of a window: 0 fine, -1 refused
static inline int dense_window_args(const void* dense, int64_t n_rows, int64_t n_cols, int64_t ld, int col_major) {
  if (n_rows < 0 || n_cols < 0 || ld < (col_major ? n_rows : n_cols)) return -1;
  if (n_rows > 0 && n_cols > 0 && !dense) return -1;   // (a null tensor: only with an empty window)
  return 0;
}

// block columns per workgroup of dense_gather: about 8192 elements of the window, at most 64 tiles
static inline int dense_group(int64_t n_rows, int64_t n_cols, int nbr, int nbc) {
  const int64_t tile = std::max<int64_t>(1, (n_rows / nbr) * (n_cols / nbc));
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(8192 / tile, 64), nbc));
}

template <typename T>
static void dense_gather_launch(hipStream_t st, const dbcsr_amd_bcsr* m, const int64_t* roff, const int64_t* coff, int G, int NG, int kind, int col_major,
                                void* dense, int64_t ld) {
  hipLaunchKernelGGL((dense_gather<T>), dim3((unsigned)((int64_t)m->nblkrows * NG)), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p,
                     static_cast<const T*>(m->data), m->row_blk_size, m->col_blk_size, roff, coff, m->nblkrows, m->nblkcols, G, NG, kind, col_major,
                     aligned16(m->data), static_cast<T*>(dense), ld);
}

template <typename T>
static void dense_scatter_launch(hipStream_t st, dbcsr_amd_bcsr* m, const int64_t* roff, const int64_t* coff, int S, int col_major, const void* dense,
                                 int64_t ld) {
  hipLaunchKernelGGL((dense_scatter<T>), dim3((unsigned)((int64_t)m->nblkrows * S)), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p,
                     static_cast<T*>(m->data), m->row_blk_size, m->col_blk_size, roff, coff, m->nblkrows, S, col_major, aligned16(m->data),
                     static_cast<const T*>(dense), ld);
}

template <typename T>
static void dense_norms_launch(hipStream_t st, const void* dense, int64_t ld, int col_major, const int* rs, const int* cs, const int64_t* roff,
                               const int64_t* coff, int nbr, int nbc, int64_t nt, int64_t n_rows, int64_t n_cols, double eps2, int* keep, int* nze) {
  hipLaunchKernelGGL((dense_block_norms<T>), grid_for(nt * 64), dim3(256), 0, st, static_cast<const T*>(dense), ld, col_major, rs, cs, roff, coff, nbr, nbc,
                     nt, n_rows, n_cols, eps2, keep, nze);
}
}  // extern "C++"

int dbcsr_amd_bcsr_to_dense(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int kind, void* dense, int64_t n_rows, int64_t n_cols,
                            int64_t ld, int col_major, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || kind < -1 || kind > 3 || (kind >= 0 && m->nblkrows != m->nblkcols)) return -1;
  if (dense_window_args(dense, n_rows, n_cols, ld, col_major)) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  const int64_t *roff = nullptr, *coff = nullptr;
  int64_t rows = 0, cols = 0;
  if (vector_offsets(E, st, m, &roff, &coff) || dense_lengths(E, st, m, roff, coff, &rows, &cols)) return -1;
  if (rows != n_rows || cols != n_cols) return -1;
  if (n_rows == 0 || n_cols == 0) return 0;
  const int G = dense_group(n_rows, n_cols, m->nblkrows, m->nblkcols), NG = (m->nblkcols + G - 1) / G;
  if ((int64_t)m->nblkrows * NG > INT32_MAX) return -1;   // (the grid)
  DBCSR_AMD_BY_TYPE(dense_gather_launch, st, m, roff, coff, G, NG, kind, col_major ? 1 : 0, dense, ld);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_to_dense", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_from_dense_apply(void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n_rows, int64_t n_cols, int64_t ld, int col_major,
                                    dbcsr_amd_bcsr* m, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m) return -1;
  if (dense_window_args(dense, n_rows, n_cols, ld, col_major)) return -1;
  if (!algebra_type(datatype)) return -10;
  hipStream_t st = stream_of(stream);
  const int64_t *roff = nullptr, *coff = nullptr;
  int64_t rows = 0, cols = 0;
  if (vector_offsets(E, st, m, &roff, &coff) || dense_lengths(E, st, m, roff, coff, &rows, &cols)) return -1;
  if (rows != n_rows || cols != n_cols) return -1;
  engine_writes_values(E);
  if (n_rows == 0 || n_cols == 0 || m->nblks == 0) return 0;
  const int S = algebra_split(m->nblkrows, m->nblks);
  if ((int64_t)m->nblkrows * S > INT32_MAX) return -1;   // (the grid)
  DBCSR_AMD_BY_TYPE(dense_scatter_launch, st, m, roff, coff, S, col_major ? 1 : 0, dense, ld);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_from_dense_apply", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_from_dense_count(void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n_rows, int64_t n_cols, int64_t ld, int col_major,
                                    const int32_t* row_blk_size, const int32_t* col_blk_size, int nblkrows, int nblkcols, double eps, int32_t* dst_row_p,
                                    int32_t* dst_col_i, int64_t* dst_blk_p, int64_t* nblks, int64_t* nze, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !dst_row_p || !nblks || !nze || nblkrows < 0 || nblkcols < 0 || (nblkrows > 0 && !row_blk_size) || (nblkcols > 0 && !col_blk_size)) return -1;
  if (!(eps >= 0.0)) return -1;   // (negative, or NaN)
  if (dense_window_args(dense, n_rows, n_cols, ld, col_major)) return -1;
  if (!algebra_type(datatype)) return -10;
  *nblks = *nze = 0;
  const int64_t nt = (int64_t)nblkrows * nblkcols;
  if (nt > INT32_MAX - 8 || (nt > 0 && (!dst_col_i || !dst_blk_p))) return -1;
  hipStream_t st = stream_of(stream);
  dbcsr_amd_bcsr sizes = {};   // (vector_offsets reads the block sizes and their counts)
  sizes.nblkrows = nblkrows, sizes.nblkcols = nblkcols, sizes.row_blk_size = row_blk_size, sizes.col_blk_size = col_blk_size;
  const size_t noff = (size_t)nblkrows + (size_t)nblkcols + 2;
  if (E->alg_i32.ensure(4 + 3 * (size_t)nt + 2) || E->alg_i64.ensure(8 + noff + (size_t)nt + 2)) return -1;
  const int64_t *roff = nullptr, *coff = nullptr;
  if (vector_offsets(E, st, &sizes, &roff, &coff)) return -1;   // (in alg_i64 behind its eight scalars: the ensure above holds it)
  int* keep = E->alg_i32.p + 4;
  int* tile_nze = keep + nt;
  int* pos = tile_nze + nt;
  int64_t* off = E->alg_i64.p + 8 + noff;
  // The block-size sums are known on the device alone.  dense_block_norms compares them with the window itself and reads nothing of dense when they
  // differ (every tile is then dropped), so the one synchronisation at the end brings the sums along with the counts.
  if (nt > 0) {
    DBCSR_AMD_BY_TYPE(dense_norms_launch, st, dense, ld, col_major ? 1 : 0, row_blk_size, col_blk_size, roff, coff, nblkrows, nblkcols, nt, n_rows, n_cols,
                      eps * eps, keep, tile_nze);
    if (exclusive_scan<int32_t>(E, keep, nt, pos, E->alg_i64.p + 0, true, st)) return -1;
    if (exclusive_scan<int64_t>(E, tile_nze, nt, off, E->alg_i64.p + 1, false, st)) return -1;
    hipLaunchKernelGGL(dense_emit, grid_for(nt), dim3(256), 0, st, keep, pos, off, nblkrows, nblkcols, nt, dst_row_p, dst_col_i, dst_blk_p);
  } else {
    ACC_CHECK(hipMemsetAsync(dst_row_p, 0, sizeof(int32_t) * ((size_t)nblkrows + 1), st));
    ACC_CHECK(hipMemsetAsync(E->alg_i64.p, 0, 2 * sizeof(int64_t), st));
  }
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, E->alg_i64.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 6, roff + nblkrows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipMemcpyAsync(E->host_scalars + 7, coff + nblkcols, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  if (E->host_scalars[6] != n_rows || E->host_scalars[7] != n_cols) return -1;
  *nblks = E->host_scalars[0];
  *nze = E->host_scalars[1];
  return check(hipGetLastError(), "dbcsr_amd_bcsr_from_dense_count", __FILE__, __LINE__);
}
// ---- submatrix method (kernels: mm_submatrix.h) ---------------------------------------------------------------------------------------------------------------
// Pure data movement by the caller's index sets: no buffer of the engine is used, no saved plan is touched, nothing synchronises.
extern "C++" {
// member columns per workgroup of submatrix_gather: about 8192 elements of the window, at most 64 tiles (dense_group's rule, with the mean member size
// n / max_members for the mean block size)
static inline int submatrix_group(int64_t n, int max_members) {
  if (max_members <= 0) return 1;
  const int64_t side = std::max<int64_t>(1, n / max_members), tile = side * side;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(8192 / tile, 64), max_members));
}

constexpr int kSubmatrixSlotsPerLaunch = 65535;   // (gridDim.y)

template <typename T>
static void submatrix_gather_launch(hipStream_t st, const dbcsr_amd_bcsr* m, int kind, int nsub, const int32_t* set_ptr, const int32_t* set_idx,
                                    const int32_t* set_off, const int32_t* sub_dim, int nslot, const int32_t* slot_sub, int max_members, void* dense,
                                    int64_t n, int64_t ld, int64_t batch_stride, double pad_diag) {
  const int G = submatrix_group(n, max_members), NG = std::max(1, (max_members + G - 1) / G);
  const unsigned gx = (unsigned)(((int64_t)max_members + 1) * NG);
  for (int slot0 = 0; slot0 < nslot; slot0 += kSubmatrixSlotsPerLaunch)
    hipLaunchKernelGGL((submatrix_gather<T>), dim3(gx, (unsigned)std::min(nslot - slot0, kSubmatrixSlotsPerLaunch)), dim3(256), 0, st, m->row_p, m->col_i,
                       m->blk_p, static_cast<const T*>(m->data), m->row_blk_size, m->col_blk_size, m->nblkrows, kind, aligned16(m->data), nsub, set_ptr,
                       set_idx, set_off, sub_dim, slot_sub, slot0, G, NG, static_cast<T*>(dense), (int)n, ld, batch_stride, pad_diag);
}

template <typename T>
static void submatrix_scatter_launch(hipStream_t st, dbcsr_amd_bcsr* m, int S, int nsub, const int32_t* set_ptr, const int32_t* set_idx,
                                     const int32_t* set_off, const int32_t* owner, const int32_t* sub_slot, const void* dense, int64_t n, int64_t ld,
                                     int64_t batch_stride) {
  hipLaunchKernelGGL((submatrix_scatter<T>), dim3((unsigned)((int64_t)m->nblkrows * S)), dim3(256), 0, st, m->row_p, m->col_i, m->blk_p,
                     static_cast<T*>(m->data), m->row_blk_size, m->col_blk_size, m->nblkrows, S, aligned16(m->data), nsub, set_ptr, set_idx, set_off, owner,
                     sub_slot, static_cast<const T*>(dense), (int)n, ld, batch_stride);
}
}  // extern "C++"

int dbcsr_amd_bcsr_submatrix_gather(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int kind, int nsub, const int32_t* set_ptr,
                                    const int32_t* set_idx, const int32_t* set_off, const int32_t* sub_dim, int nslot, const int32_t* slot_sub,
                                    int max_members, void* dense, int64_t n, int64_t ld, int64_t batch_stride, double pad_diag, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || kind < -1 || kind > 3 || m->nblkrows != m->nblkcols) return -1;
  if (nsub < 0 || nslot < 0 || max_members < 0 || n < 0 || n > INT32_MAX || ld < n) return -1;
  if (nslot > 1 && (batch_stride < 0 || (n > 0 && batch_stride / n < ld))) return -1;   // (batch_stride < n ld, without forming the product)
  if (nslot > 0 && n > 0) {   // (a null tensor: only with an empty batch)
    if (!dense || (nsub > 0 && (!set_ptr || !sub_dim)) || (max_members > 0 && (!set_idx || !set_off))) return -1;
    if (m->nblks > 0 && (!m->row_p || !m->col_i || !m->blk_p || !m->data)) return -1;
  }
  if (!algebra_type(datatype)) return -10;
  if (nslot == 0 || n == 0) return 0;
  hipStream_t st = stream_of(stream);
  const int G = submatrix_group(n, max_members);
  if (((int64_t)max_members + 1) * std::max(1, (max_members + G - 1) / G) > INT32_MAX) return -1;   // (the grid)
  DBCSR_AMD_BY_TYPE(submatrix_gather_launch, st, m, kind, nsub, set_ptr, set_idx, set_off, sub_dim, nslot, slot_sub, max_members, dense, n, ld, batch_stride,
                    pad_diag);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_submatrix_gather", __FILE__, __LINE__);
}

int dbcsr_amd_bcsr_submatrix_scatter(void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n, int64_t ld, int64_t batch_stride, int nsub,
                                     const int32_t* set_ptr, const int32_t* set_idx, const int32_t* set_off, const int32_t* owner, const int32_t* sub_slot,
                                     dbcsr_amd_bcsr* m, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !m || m->nblkrows != m->nblkcols) return -1;
  if (nsub < 0 || n < 0 || n > INT32_MAX || ld < n || batch_stride < 0) return -1;
  const bool work = n > 0 && nsub > 0 && m->nblks > 0 && m->nblkrows > 0;
  if (work && (!dense || !set_ptr || !set_idx || !set_off || !owner || !sub_slot)) return -1;   // (a null tensor: only with nothing to move)
  if (!algebra_type(datatype)) return -10;
  engine_writes_values(E);
  if (!work) return 0;
  hipStream_t st = stream_of(stream);
  const int S = algebra_split(m->nblkrows, m->nblks);
  if ((int64_t)m->nblkrows * S > INT32_MAX) return -1;   // (the grid)
  DBCSR_AMD_BY_TYPE(submatrix_scatter_launch, st, m, S, nsub, set_ptr, set_idx, set_off, owner, sub_slot, dense, n, ld, batch_stride);
  return check(hipGetLastError(), "dbcsr_amd_bcsr_submatrix_scatter", __FILE__, __LINE__);
}
// (DBCSR_AMD_BY_TYPE stays defined for mm_engine_elementwise.h, which follows this file and ends its life)

#endif
