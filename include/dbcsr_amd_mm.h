/*
 * dbcsr_amd_mm.h -- device-resident local multiply of DBCSR, C-ABI.
 *
 * Replaces, for one rank and one Cannon tick, the host-driven chain
 *   dbcsr_mm_multrec_multiply -> dbcsr_mm_csr_multiply_low -> flush_stacks ->
 *   dbcsr_mm_sched_process -> dbcsr_mm_accdrv_process -> libsmm_acc_process,
 *   then dbcsr_mm_multrec_finalize / dbcsr_finalize
 *   (/root/reference/src/mm/dbcsr_mm_multrec.F:263-335, dbcsr_mm_csr.F:178-359,
 *    dbcsr_mm_sched.F:266-382, dbcsr_mm_accdrv.F:433-541,
 *    src/work/dbcsr_work_operations.F:749+)
 * by two calls that keep panels, index and result in HBM:
 *   dbcsr_amd_mm_symbolic : the CSR x CSR symbolic product on the GPU
 *                           (C index = sorted BCSR, what dbcsr_finalize emits)
 *   dbcsr_amd_mm_numeric  : C_out = beta*C_in + alpha*A*B, one wavefront per
 *                           C block, all its products summed in MFMA
 *                           accumulators, each C block written once.
 *
 * A matrix is passed as the reference's BCSR index (core/dbcsr_types.F:376-385:
 * row_p / col_i / blk_p + one data area), 0-based, 64-bit block offsets,
 * blocks column-major.  ALL POINTERS ARE DEVICE POINTERS.
 *
 * Data types: dbcsr_type_real_8, dbcsr_type_real_4 and dbcsr_type_complex_8 (COMPLEX(real_8): (re, im) pairs of doubles,
 * interleaved; an element offset in blk_p counts complex elements).  Every entry with a datatype argument takes complex_8 unless
 * it says otherwise below; the entries whose scalars are real doubles read them as x + 0i for complex data, and the _z entries
 * take complex scalars as const double[2] = {re, im}.  Matrices with symmetry: all four kinds (symmetric, antisymmetric, hermitian, antihermitian;
 * dbcsr_amd_bcsr_twin_*, _desymmetrize_*, _desymmetrized) for every type, and a complex_8 product matrix with symmetry through
 * dbcsr_amd_multiply_symmetric_c_z.  NOT offered for complex_8 (they return -10, as every entry does for dbcsr_type_complex_4): libsmm_acc_process /
 * _transpose (the reference's accelerator path returns -10 for complex stacks too), dbcsr_amd_bcsr_checksum, and the multiplies with real scalars,
 * dbcsr_amd_multiply and dbcsr_amd_multiply_symmetric_c / _klimits (see dbcsr_amd_multiply_z and dbcsr_amd_multiply_symmetric_c_z).
 *
 * Return: 0 ok, non-zero error (message on stderr).  Streams use the handle
 * convention of dbcsr_acc.h (pointer to hipStream_t, NULL = null stream).
 */
#ifndef DBCSR_AMD_MM_H
#define DBCSR_AMD_MM_H

#include <stdint.h>

#include "dbcsr_acc_libsmm.h"

#if defined(__cplusplus)
extern "C" {
#endif

typedef struct dbcsr_amd_bcsr {
  int32_t nblkrows, nblkcols;
  const int32_t* row_blk_size; /* [nblkrows] */
  const int32_t* col_blk_size; /* [nblkcols] */
  int32_t* row_p;              /* [nblkrows+1] */
  int32_t* col_i;              /* [nblks], ascending inside a row */
  int64_t* blk_p;              /* [nblks], element offset of each block in data */
  void* data;                  /* fp64, fp32 or complex_8 (re, im) elements */
  int64_t nblks;
  uint64_t index_stamp;        /* generation of the index arrays above: 0 = unknown; a caller that owns them may set a value that it
                                  changes whenever it writes, frees or re-allocates one of them (see dbcsr_amd_mm_trust_plan).  Set to
                                  0 by the library in every matrix it hands out. */
} dbcsr_amd_bcsr;

typedef struct dbcsr_amd_mm_counts {
  int64_t c_nblks;   /* blocks of C_out */
  int64_t c_nze;     /* elements of C_out */
  int64_t nproducts; /* block products A(i,k)*B(k,j) */
  int64_t flop;      /* sum 2*m*n*k over products == dbcsr_multiply's flop (dbcsr_mm_csr.F:350) */
} dbcsr_amd_mm_counts;

/* Per-(m, n, k) statistics of a multiply: what dbcsr_mm_sched keeps per stack (src/mm/dbcsr_mm_sched.F:392-461, the
 * "flops m x n x k" table of dbcsr_print_statistics); here every product runs on the accelerator. */
typedef struct dbcsr_amd_mnk_stat {
  int32_t m, n, k, reserved;
  int64_t nproducts; /* block products of this size ("matmuls") */
  int64_t flop;      /* 2*m*n*k*nproducts */
} dbcsr_amd_mnk_stat;

int dbcsr_amd_mm_create(void** handle);
int dbcsr_amd_mm_destroy(void* handle);

/* Symbolic product.  c_in may have nblks == 0.  retain_sparsity: C_out keeps
 * exactly C_in's pattern (dbcsr_mm_csr.F:319).  Writes c_out_row_p
 * [nblkrows+1] (device) and *counts (host; the call synchronises `stream`
 * once to deliver them).  The pattern is kept in the handle for the numeric
 * call that must follow with the same A, B, C_in index arrays. */
int dbcsr_amd_mm_symbolic(void* handle, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, const dbcsr_amd_bcsr* c_in,
  int retain_sparsity, int32_t* c_out_row_p, dbcsr_amd_mm_counts* counts, void* stream);

/* Symbolic product with on-the-fly filtering (dbcsr_mm_csr.F:276, dbcsr_mm_cannon.F:1040-1113): a product
 * A(i,k)*B(k,j) is skipped when ||A(i,k)||^2 * ||alpha*B(k,j)||^2 < (filter_eps / max(1, #blocks of A row i))^2
 * (single precision, as the reference); new C blocks are created only by surviving products.  Needs the data
 * areas of a and b (norms) and the alpha of the numeric call that follows.  filter_eps <= 0: same as above.
 * complex_8: block norm^2 = sum re^2 + im^2, and `alpha` is |alpha| of the numeric call (the rule uses ||alpha*B||). */
int dbcsr_amd_mm_symbolic_filtered(void* handle, libsmm_acc_data_t datatype, double alpha, double filter_eps, const dbcsr_amd_bcsr* a,
  const dbcsr_amd_bcsr* b, const dbcsr_amd_bcsr* c_in, int retain_sparsity, int32_t* c_out_row_p, dbcsr_amd_mm_counts* counts,
  void* stream);

/* Final block filter of a multiply (dbcsr_mm_multrec.F:694-748) / dbcsr_filter: blocks with sum x^2 < eps^2 are
 * dropped.  _count writes new_row_p [nblkrows+1] (device) and the new block/element counts (host, synchronises);
 * _apply then compacts index and data into caller-allocated dst arrays (dst->row_p = new_row_p).
 * complex_8: sum x^2 is sum re^2 + im^2.
 * The two halves belong together (so do those of the crop and of the union add below): the count leaves its answer in work areas that the
 * symbolic phase of a multiply, every other _count, the transpose and the twin moves use too.  Any of those between a _count and its _apply ends the
 * pending count -- the _apply then returns -1 and writes nothing; count again.  (A reduction, a norm, a vector operation or a flat add in between is
 * harmless: the algebra has buffers of its own.  A crop count is also ended by dbcsr_amd_bcsr_scale_window and dbcsr_amd_bcsr_checksum.)
 * Block norms left by a multiply: the exact-size, slab and class kernels of a FILTERED fp64 multiply (dbcsr_amd_mm_symbolic_filtered with filter_eps > 0)
 * leave every C block's squared norm behind, and a _filter_count on that C -- same data pointer, same block count -- uses them instead of a pass over C.
 * The engine forgets them in the next symbolic phase, numeric phase or filter count, and in every entry that writes a matrix's values (init_c, scale_window,
 * add_apply, the diagonal entries, set_diag, scale_by_vector, rank_update, block_diag_apply / _invert, from_dense_apply, fill_random, crop / filter apply, transpose, twin moves).  It cannot see a write
 * made outside it: the norms are good only while nobody else writes C -- or frees it and allocates another matrix there -- between the numeric phase and
 * the filter. */
int dbcsr_amd_bcsr_filter_count(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, double eps, int32_t* new_row_p,
  int64_t* new_nblks, int64_t* new_nze, void* stream);
int dbcsr_amd_bcsr_filter_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);

/* Index-only form of dbcsr_amd_bcsr_filter_apply, after dbcsr_amd_bcsr_filter_count on the same handle and src:
 * dst->row_p = the new_row_p of the count, dst->col_i / dst->blk_p caller-allocated [new_nblks], dst->data MUST be src->data
 * (anything else: -1; so is a call without a count before it, or with a src whose nblks is not the counted one).  No element is
 * moved: kept blocks keep their offsets, the dropped blocks' space stays allocated and unreferenced.  Works for real_8 and real_4
 * alike (no datatype argument: no element is touched).
 * What comes back is an UNPACKED matrix: blk_p is strictly increasing but no longer the running sum of the block sizes, and the
 * index refers to new_nze elements of a larger data area.  Everything that reaches a block through blk_p takes it (operands A and
 * B, C_in out of place, transpose, desymmetrize / twin, crop, scale_window, checksum).  The one rule it brings: it must not be the
 * aliased c_in / c_out of an in-place dbcsr_amd_mm_numeric (see there: that needs a packed C_in).  A packed copy needs no function
 * of its own: dbcsr_amd_bcsr_crop_count / _apply with all four bounds negative is a packing copy, and the only thing besides
 * releasing the matrix that gives the dropped blocks' memory back.
 * dbcsr_amd_mm_set_filter_in_place(handle, 1): the final filter inside dbcsr_amd_multiply (and dbcsr_amd_multiply_symmetric_c /
 * _klimits, which call it) uses this form: c_out then owns the product's data area together with the new index arrays (the
 * product's own index arrays are freed before the call returns), and dbcsr_amd_bcsr_release frees it as any other result.
 * 0 (the default) switches back to the copying form. */
int dbcsr_amd_bcsr_filter_apply_index(void* handle, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);
int dbcsr_amd_mm_set_filter_in_place(void* handle, int on);

/* Submatrix limits of dbcsr_multiply (first_row ... last_k, src/mm/dbcsr_mm.F:631-709): dbcsr_crop_matrix
 * (src/ops/dbcsr_operations.F:1652-1833) keeps the blocks that intersect the window [row_lo, row_hi] x [col_lo, col_hi]
 * (0-based inclusive ELEMENT indices of the full matrix; a negative bound = no bound) and clears the parts of the
 * boundary blocks outside it.  Same two-step protocol as the filter: _count writes new_row_p and the new counts
 * (synchronises), _apply compacts into caller-allocated dst arrays.  _scale_window is dbcsr_scale with limits: in place,
 * only the elements inside the window are multiplied by beta. */
int dbcsr_amd_bcsr_crop_count(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int64_t row_lo, int64_t row_hi,
  int64_t col_lo, int64_t col_hi, int32_t* new_row_p, int64_t* new_nblks, int64_t* new_nze, void* stream);
int dbcsr_amd_bcsr_crop_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);
int dbcsr_amd_bcsr_scale_window(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, double beta, int64_t row_lo,
  int64_t row_hi, int64_t col_lo, int64_t col_hi, void* stream);
/* ... of a complex_8 matrix with a complex beta = {re, im} */
int dbcsr_amd_bcsr_scale_window_z(void* handle, dbcsr_amd_bcsr* m, const double beta[2], int64_t row_lo, int64_t row_hi, int64_t col_lo,
  int64_t col_hi, void* stream);

/* Numeric phase.  c_out->row_p is the array written by the symbolic call;
 * col_i [c_nblks], blk_p [c_nblks] and data [c_nze] are allocated by the caller
 * and filled here (blocks laid out in index order).  c_out->data may alias
 * c_in->data only when retain_sparsity was set (same pattern, in place) AND c_in's blocks are already laid out
 * packed in index order (blk_p = running sum of the block sizes) -- which is how every matrix produced by this
 * library is laid out; a C_in with another placement must not be aliased (c_out->blk_p is rewritten to the packed
 * offsets).
 * datatype: dbcsr_type_real_8, dbcsr_type_real_4 or dbcsr_type_complex_8 (alpha + 0i, beta + 0i).  Asynchronous on stream. */
int dbcsr_amd_mm_numeric(void* handle, libsmm_acc_data_t datatype, double alpha, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b,
  double beta, const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out, void* stream);
/* The numeric phase of a complex_8 multiply with complex scalars {re, im}: C_out = beta*C_in + alpha*A*B in complex arithmetic (kernel
 * family mm_numeric_z64<MA,NC>: every block is written, an announced final filter -- dbcsr_amd_mm_expect_filter -- is ignored).
 * In-place accumulation (c_out aliasing c_in after a retain_sparsity symbolic phase) leaves blocks without products untouched when
 * beta == 1 + 0i. */
int dbcsr_amd_mm_numeric_z(void* handle, const double alpha[2], const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, const double beta[2],
  const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out, void* stream);

/* Structure-only companion of the symbolic call, for multiplies whose products arrive in
 * several passes (the Cannon ticks of dbcsr_mm_cannon.F:1347-1704): emits C_out's index
 * (col_i, blk_p; row_p came from the symbolic call) and sets C_out = beta*C_in on the
 * blocks C_in has, 0 on the new ones.  The passes then call symbolic(retain_sparsity=1) +
 * numeric with c_out aliasing c_in and beta = 1: blocks that get no product in a pass are
 * not touched. */
int dbcsr_amd_mm_init_c(void* handle, libsmm_acc_data_t datatype, double beta, const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out,
  void* stream);
/* ... of a complex_8 product with a complex beta = {re, im} */
int dbcsr_amd_mm_init_c_z(void* handle, const double beta[2], const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out, void* stream);

/* Transposed copy of a BCSR matrix on the device (dbcsr_new_transposed,
 * src/ops/dbcsr_transformations.F): dst index arrays/data are caller-allocated
 * with src's nblks / nze; dst->row_blk_size/col_blk_size must already hold the
 * swapped size arrays. */
int dbcsr_amd_bcsr_transpose(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);
/* The conjugate transpose (complex_8; for real types the same as dbcsr_amd_bcsr_transpose): what 'C' means in dbcsr_multiply. */
int dbcsr_amd_bcsr_transpose_conj(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);

/* Checksums of dbcsr_checksum (src/dist/dbcsr_dist_util.F:432-577) on the
 * device: out[0] = sum x^2, out[1] = sum x*ln|row*col| (1-based global element
 * coordinates).  Synchronises stream.  Real types only: -10 for complex_8. */
int dbcsr_amd_bcsr_checksum(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, double* out2, void* stream);

/* Synthetic block values of the reference's test generator
 * (src/ops/dbcsr_test_methods.F:423-429 + LAPACK dlarnv/slarnv idist=1): block b of the
 * index gets larnv(seed(row+1, nblkrows, col+1, nblkcols, counter)).  Used by the
 * benchmark to create inputs directly in HBM.  complex_8: LAPACK zlarnv(idist = 1) -- the block's 2*m*n doubles are the dlarnv stream
 * of the block's seed, re, im, re, im, ... */
int dbcsr_amd_bcsr_fill_random(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int counter, void* stream);

/* Same for one rank's part of a distributed matrix: row_gid/col_gid (device, may be NULL)
 * map local block rows/columns to global ones, nblkrows_global is the global row count
 * that enters the seed (values are a pure function of the GLOBAL block coordinates, as in
 * the reference, so any process grid generates the same matrix). */
int dbcsr_amd_bcsr_fill_random_dist(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int counter,
  const int32_t* row_gid, const int32_t* col_gid, int32_t nblkrows_global, void* stream);

/* dbcsr_multiply for one rank as one call (src/dbcsr_api.F:1411-1433 -> src/mm/dbcsr_mm.F:336 dbcsr_multiply_generic):
 *   C_out = beta*C + alpha*op(A)*op(B)
 * transa/transb 'N' | 'T' | 'C' (real data: 'C' == 'T'); limits = {first_row, last_row, first_column, last_column, first_k,
 * last_k}, 1-based inclusive full-matrix indices, 0 = not given, NULL = no limits (inside the window beta scales C, outside it C
 * is unchanged); retain_sparsity and filter_eps as in the reference.  c_out: row_p / col_i / blk_p / data are allocated by the
 * library (its caching device allocator) and belong to the caller afterwards -- ONLY dbcsr_amd_bcsr_release frees them; the size arrays are borrowed
 * from matrix_c.  *flop (may be NULL) receives the reference's flop count.  Returns when the result is complete. */
int dbcsr_amd_multiply(void* handle, char transa, char transb, libsmm_acc_data_t datatype, double alpha, const dbcsr_amd_bcsr* matrix_a,
  const dbcsr_amd_bcsr* matrix_b, double beta, const dbcsr_amd_bcsr* matrix_c, const int64_t* limits, int retain_sparsity,
  double filter_eps, dbcsr_amd_bcsr* c_out, int64_t* flop, void* stream);
/* The same for complex_8 matrices with complex scalars {re, im}: 'C' is the conjugate transpose, 'T' the plain one; beta == 0 means both
 * parts are zero; *flop stays sum 2*m*n*k, as the reference counts it for every type.  Complex multiplies run in one pass over k.
 * (dbcsr_amd_multiply itself keeps answering -10 for dbcsr_type_complex_8, as it always did: hosts written against the real-only
 * library rely on that answer to leave a complex multiply to the reference path.  This entry is how a complex multiply is asked for.) */
int dbcsr_amd_multiply_z(void* handle, char transa, char transb, const double alpha[2], const dbcsr_amd_bcsr* matrix_a, const dbcsr_amd_bcsr* matrix_b,
  const double beta[2], const dbcsr_amd_bcsr* matrix_c, const int64_t* limits, int retain_sparsity, double filter_eps,
  dbcsr_amd_bcsr* c_out, int64_t* flop, void* stream);
int dbcsr_amd_bcsr_release(dbcsr_amd_bcsr* m);

/* HIP-event timing of the last dbcsr_amd_mm_numeric call on this handle, taken
 * on the stream the kernels were launched on: ms_fill = product-list/index
 * emission kernel, ms_numeric = the block-GEMM kernel.  Waits for that call to
 * finish.  Used by bench.py for the roofline figure. */
int dbcsr_amd_mm_timing(void* handle, float* ms_fill, float* ms_numeric);

/* Symbol name of the dominant kernel, for profile look-up. */
/* Matrices with symmetry (src/core/dbcsr_types.F: matrix_type 'S' symmetric, 'A' antisymmetric, 'H' hermitian, 'K' antihermitian): square block
 * structure, ONE block stored per pair (r, c) / (c, r), diagonal blocks stored in full and taken as they are (nobody checks that they have the symmetry).
 * The twin at (c, r) of a stored block X at (r, c), r != c, by `kind`:
 *     0 symmetric      X^T           1 antisymmetric  -X^T
 *     2 hermitian      conj(X)^T     3 antihermitian  -conj(X)^T
 * (bit 0 negates, bit 1 conjugates; sign flips and copies: every result below is defined bit for bit; any other value: -1).  Real data: conjugation is the
 * identity, kinds 2 / 3 behave as 0 / 1.  All data types, complex_8 with all four kinds.
 *
 * Operands (the reference desymmetrizes them while it builds the multiplication images, src/mm/dbcsr_mm_cannon.F:284, 351-379): src holds one block per
 * pair (any mix of upper and lower blocks); the full matrix gets block (c, r) = twin(block (r, c)) in addition.  _count writes dst_row_p [nblkrows+1]
 * (device) and the block / element counts (host, synchronises); _apply fills caller-allocated dst arrays (dst->row_p = that row_p), blocks packed in index
 * order.  An operand is desymmetrized BEFORE op() is applied: 'N', 'T' and 'C' all stay meaningful for a hermitian operand.
 * _apply: -1 when no count of this matrix and mode is pending (none since the handle was made, or a symbolic phase, a transpose or another pair's count
 * -- filter, crop, union add -- has run since: they write the areas the count left its answer in), for a src with another nblks / nblkrows than the
 * counted one, and -- dbcsr_amd_bcsr_twin_apply -- for another mode than the counted one.  A refused _apply launches nothing and writes nothing.  The
 * count stays pending after an _apply: the same src may be filled again. */
int dbcsr_amd_bcsr_desymmetrize_count(void* handle, const dbcsr_amd_bcsr* src, int32_t* dst_row_p, int64_t* nblks, int64_t* nze, void* stream);
int dbcsr_amd_bcsr_desymmetrize_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, int kind, dbcsr_amd_bcsr* dst, void* stream);

/* Product matrix WITH symmetry.  The reference puts the index of such a product matrix into canonical (checkerboard) form before the multiplication
 * (src/mm/dbcsr_mm.F:711-719, dbcsr_make_index_canonical), its local multiply computes block (i, j) only when that is the stored one of the pair
 * (i, j) / (j, i) (src/mm/dbcsr_mm_csr.F:280-292, checker_tr of src/dist/dbcsr_dist_operations.F:65-75), and the result is returned as the stored
 * triangle.  The pieces:
 *   dbcsr_amd_bcsr_twin_{count,apply}  mode 0: desymmetrize (= the two calls above); mode 1: stored triangle (row <= column) -> canonical form; mode 2:
 *     canonical form -> stored triangle.  A block that changes sides becomes its twin.  Same calling convention as desymmetrize_{count,apply}.
 *   dbcsr_amd_mm_set_canonical_product(handle, 1): the following symbolic phases of this handle leave out the products of blocks that are not stored in
 *     canonical form (blocks of C_in are kept wherever they are); 0 switches it off again.
 *   dbcsr_amd_multiply_symmetric_c: the whole sequence in one call; matrix_c and c_out hold the stored triangle (row <= column), no limits (the
 *     reference's own tests run symmetric products with full limits only, tests/dbcsr_test_multiply.F:196-200).
 * With P = op(A) * op(B), a stored block X at (r, c) therefore becomes beta * X + alpha * P(r, c) when it stays where it is in canonical form, and
 * twin(beta * twin(X) + alpha * P(c, r)) when it moves -- hermitian: conj(beta) * X + conj(alpha) * conj(P(c, r))^T.  Both agree when P has the symmetry
 * and alpha, beta are real (the caller's contract, as for real data); for other inputs this formula IS what the call computes. */
/* desymmetrize in one call: dst's arrays are allocated by the library (dbcsr_amd_bcsr_release frees them), size arrays borrowed from src */
int dbcsr_amd_bcsr_desymmetrized(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, int kind, dbcsr_amd_bcsr* dst, void* stream);
/* (_twin_apply: -1 when no count of this matrix and mode is pending, as for desymmetrize_apply above) */
int dbcsr_amd_bcsr_twin_count(void* handle, const dbcsr_amd_bcsr* src, int mode, int32_t* dst_row_p, int64_t* nblks, int64_t* nze, void* stream);
int dbcsr_amd_bcsr_twin_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, int mode, int kind, dbcsr_amd_bcsr* dst,
  void* stream);
int dbcsr_amd_mm_set_canonical_product(void* handle, int on);
/* (real scalars: dbcsr_type_real_8 / _real_4; -10 for complex_8, whose entry is dbcsr_amd_multiply_symmetric_c_z) */
int dbcsr_amd_multiply_symmetric_c(void* handle, char transa, char transb, libsmm_acc_data_t datatype, double alpha,
  const dbcsr_amd_bcsr* matrix_a, const dbcsr_amd_bcsr* matrix_b, double beta, const dbcsr_amd_bcsr* matrix_c, int kind,
  int retain_sparsity, double filter_eps, dbcsr_amd_bcsr* c_out, int64_t* flop, void* stream);
/* the same with limits on the inner dimension (dbcsr_multiply's first_k / last_k: 1-based inclusive element indices, 0 = not given) -- what the
   reference's own tests of products with symmetry use (tests/dbcsr_test_multiply.F:196-200: full row / column limits, any k limits) */
int dbcsr_amd_multiply_symmetric_c_klimits(void* handle, char transa, char transb, libsmm_acc_data_t datatype, double alpha,
  const dbcsr_amd_bcsr* matrix_a, const dbcsr_amd_bcsr* matrix_b, double beta, const dbcsr_amd_bcsr* matrix_c, int kind,
  int64_t first_k, int64_t last_k, int retain_sparsity, double filter_eps, dbcsr_amd_bcsr* c_out, int64_t* flop, void* stream);
/* ... for complex_8 matrices with complex scalars {re, im}: the three steps around dbcsr_amd_multiply_z ('C' conjugates); first_k / last_k as above */
int dbcsr_amd_multiply_symmetric_c_z(void* handle, char transa, char transb, const double alpha[2], const dbcsr_amd_bcsr* matrix_a,
  const dbcsr_amd_bcsr* matrix_b, const double beta[2], const dbcsr_amd_bcsr* matrix_c, int kind, int64_t first_k, int64_t last_k,
  int retain_sparsity, double filter_eps, dbcsr_amd_bcsr* c_out, int64_t* flop, void* stream);

/* Statistics of the last dbcsr_amd_mm_numeric of this handle, by (m, n, k): at most max_entries records are written to
 * `out` (host memory), *n_entries receives the number of distinct triples (larger than max_entries = truncated).
 * Counted on the device from the product lists of that call; synchronises `stream`. */
int dbcsr_amd_mm_stats(void* handle, dbcsr_amd_mnk_stat* out, int max_entries, int* n_entries, void* stream);

const char* dbcsr_amd_mm_kernel_name(libsmm_acc_data_t datatype);
/* name (with its template arguments) of the block-product kernel the last dbcsr_amd_mm_numeric of this handle launched */
const char* dbcsr_amd_mm_last_kernel(void* handle);
/* what the last symbolic phase of this handle chose, one line: "bitmap=plain|filtered|rows_filtered count=word|grid|rows W=<bitmap words per row>
   NP=<column panels> PW=<words per panel> classes=0|1 rowp_chunks=<chunks of the scan that made row_p> plan=miss|hit" (plan=hit: the saved plan of the
   previous multiply was reused, the other fields are that plan's).  Read-only; the text lives in the handle until the next call. */
const char* dbcsr_amd_mm_last_symbolic(void* handle);
/* name of the stack kernel the calling thread's last libsmm_acc_process (fp64, homogeneous stack) launched: "smm_stack_f64_exact<m,n,k>" (compiled
   for the triplet at run time, as libsmm_acc.cpp:90-195 does), "smm_stack_f64_lds(...)" (run-time sizes), "smm_stack_f64_big(...)" (blocks of 33 ... 80) */
const char* dbcsr_amd_smm_last_kernel(void);

/* Plan reuse: a multiply whose A, B and C_in have exactly the index arrays (row_p, col_i, blk_p, block sizes) of the previous
 * multiply of this handle -- every SCF step of a CP2K run -- skips its symbolic phase: the engine keeps device copies of the last
 * call's index arrays and compares the incoming ones on the device (one small kernel, one flag).  Multiplies with filter_eps > 0
 * never reuse (their pattern depends on the values).  DBCSR_AMD_MM_PLAN=0 switches it off.  Counters since the handle was made: */
/* Plan reuse without the comparison: while `on`, operands whose twelve index arrays (row_p / col_i / blk_p of A, B, C_in, the three
   block-size arrays) sit at the ADDRESSES the saved plan saw AND carry the non-zero index_stamp values the plan was saved with are
   taken as unchanged -- no comparison kernel, no synchronisation of the stream in dbcsr_amd_mm_symbolic.  The stamp is what makes the
   address test safe: an operand that was freed and allocated again at the same addresses with another pattern has another stamp (or
   none: 0 is never trusted) and is compared on the device as always.  For callers that own these arrays (the panels of a distributed
   multiply, dbcsr_amd/cannon.py; the benchmark's operands). */
int dbcsr_amd_mm_trust_plan(void* handle, int on);

/* A filtered multiply (reference: src/mm/dbcsr_mm_multrec.F:373-383 -- the product of a multiply with filter_eps is filtered with the same eps before it is
   finalized): announce the final block filter of the NEXT dbcsr_amd_mm_numeric of this handle.  Its product kernels form a block's squared norm before they write it
   and leave a block with ||blk||^2 < eps^2 UNWRITTEN -- the block filter is going to drop it (same double, same comparison), nobody may read it before.  The C that
   comes back is therefore only good for dbcsr_amd_bcsr_filter_count / _apply with an eps that is not smaller (a smaller one is refused: -3, nothing is counted), and
   that filter comes before any other call that writes C.  Ignored by
   complex_8 multiplies (every block is written).  On products with many
   dropped blocks the dropped share of C's write traffic is saved.  Without this call every block is written.  Call it AFTER the symbolic phase of the
   multiply it is meant for (a symbolic phase cancels an announcement that was never consumed).  fp64; ignored for retain_sparsity and in-place accumulation. */
int dbcsr_amd_mm_expect_filter(void* handle, double eps);
int dbcsr_amd_mm_plan_stats(void* handle, int64_t* reused, int64_t* built);

/* Matrix algebra between multiplies (src/ops/dbcsr_operations.F: dbcsr_add, dbcsr_scale, dbcsr_add_on_diag, dbcsr_trace, dbcsr_dot, dbcsr_frobenius_norm) on
 * device-resident matrices, for dbcsr_type_real_8, dbcsr_type_real_4 and dbcsr_type_complex_8 (any other type code: -10; the dot: real types only).  Every
 * operation goes by the index (row_p, col_i, blk_p), never by the extent of a data area: the result of an in-place filter is an operand like any other.
 * The block columns of every block row must be in ascending order (as in every matrix this library makes): the position of a block inside its row is found
 * from the number of blocks with a smaller column, the same convention by which the multiply finds a block of C_in.  NULL arguments and matrices whose
 * nblkrows / nblkcols differ: -1.  Complex scalars are double[2] = {re, im}; the imaginary part is ignored for real data.
 *
 * dbcsr_add: A <- alpha*A + beta*B.  The result's pattern is the union of both patterns, blocks packed in index order; a block one operand lacks counts as
 * zero there (the block is alpha*a or beta*b, and with a scalar that is exactly 1 it is bit-identical to its source); blocks of A stay stored with
 * alpha == 0.  beta_is_zero: B's pattern is NOT merged -- the result is alpha*A on A's pattern and B is never read.  Matrices with symmetry are added on
 * their stored triangles as they are (the caller checks that both have the same symmetry).  Two steps, as filter and crop:
 *   _add_count   writes dst_row_p [nblkrows + 1] (device) and the block / element counts of the result (host; synchronises).  *same_pattern = 1: A and B have
 *     the same row_p, col_i AND blk_p and A is packed -- compared on the device, with buffers no saved plan depends on.  Otherwise the union pattern is
 *     formed in the work areas of the symbolic phase: the handle's saved plan is invalidated, as by a filter or a crop.
 *   _add_apply   fills dst (dst->row_p = that row_p; col_i, blk_p [nblks], data [nze] allocated by the caller).  When _count reported same_pattern, dst may be
 *     a itself: one flat pass over the data area in place, no index array is written (a multiply with A as operand afterwards still reuses its plan).
 *     Otherwise a dst whose data area is a's or b's is refused (-1).  One _apply per _count.  Asynchronous on stream.
 * With alpha == beta == 1 on the same pattern the result is a + b in the data's own precision, bit for bit. */
int dbcsr_amd_bcsr_add_count(void* handle, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int beta_is_zero, int32_t* dst_row_p, int64_t* nblks,
  int64_t* nze, int* same_pattern, void* stream);
int dbcsr_amd_bcsr_add_apply(void* handle, libsmm_acc_data_t datatype, const double alpha[2], const dbcsr_amd_bcsr* a, const double beta[2],
  const dbcsr_amd_bcsr* b, dbcsr_amd_bcsr* dst, void* stream);
/* dbcsr_scale of the whole matrix is dbcsr_amd_bcsr_scale_window / _scale_window_z with no bounds (all four negative).
 *
 * dbcsr_add_on_diag (square matrix, row_blk_size == col_blk_size): alpha is added to every diagonal element; diagonal blocks the matrix lacks are created.
 *   _diag_shift  in place: adds alpha to the diagonal elements of the diagonal blocks m HAS; nothing else is written, no index array is touched.
 *   _diag_count  the index of the block-diagonal matrix of the diagonal blocks m LACKS: dst_row_p [nblkrows + 1], dst_col_i / dst_blk_p [nblkrows] (device,
 *     the first *nblks entries are written), *nblks and *nze on the host (synchronises).  No saved plan is touched.
 *   _diag_fill   every diagonal block of dst = alpha * identity.
 * add_on_diag is _diag_shift, and when blocks are missing the add (alpha = beta = 1) of the matrix made by _diag_count / _diag_fill: old elements off the
 * diagonal stay bit-identical, new blocks are alpha * I. */
int dbcsr_amd_bcsr_diag_count(void* handle, const dbcsr_amd_bcsr* m, int32_t* dst_row_p, int32_t* dst_col_i, int64_t* dst_blk_p, int64_t* nblks,
  int64_t* nze, void* stream);
int dbcsr_amd_bcsr_diag_fill(void* handle, libsmm_acc_data_t datatype, const double alpha[2], dbcsr_amd_bcsr* dst, void* stream);
int dbcsr_amd_bcsr_diag_shift(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, const double alpha[2], void* stream);
/* Reductions.  Sums are formed in double (fp32 data converted first), one partial per wave, the partials summed in a fixed order by one workgroup: no
 * floating-point atomics, the same bits on every call.  They use buffers of their own: a saved plan stays.  Each synchronises stream.
 *   _trace  out = {re, im} of the sum of the diagonal elements of the diagonal blocks present (square block structure; im = 0 for real data).
 *   _dot    out[0] = sum a_ij * b_ij over the blocks BOTH matrices store = trace(A^T B).  symmetric != 0 (both matrices symmetric, stored triangles): blocks
 *           off the diagonal count twice.  Real types only, -10 for complex_8: whether the reference conjugates one operand could not be checked against its
 *           sources, so the complex dot is not offered rather than guessed.
 *   _norm2  out[0] = sum |x|^2, the SQUARED Frobenius norm.  symmetric != 0 (any of the four symmetries): blocks off the diagonal count twice. */
int dbcsr_amd_bcsr_trace(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, double out[2], void* stream);
int dbcsr_amd_bcsr_dot(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int symmetric, double out[1],
  void* stream);
int dbcsr_amd_bcsr_norm2(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int symmetric, double out[1], void* stream);

/* Norms and vectors (src/ops/dbcsr_operations.F: dbcsr_norm / dbcsr_gershgorin_norm / dbcsr_maxabs_norm, dbcsr_get_diag, dbcsr_set_diag,
 * dbcsr_scale_by_vector; and the product of the matrix with a dense vector): a result or an operand per FULL row or column of the matrix.  Same types,
 * same answers as above (-10, -1; 0 for an empty matrix: scalar outputs are then 0, the vector outputs of the sums and of _get_diag all zero).  out, diag and vec are DEVICE memory.  A vector over the rows has
 * sum(row_blk_size) elements, one over the columns sum(col_blk_size), in the order of the dense matrix; the element offsets of the block rows / columns are
 * formed on the device.  Sums are carried in double, one partial vector per wave of a block row / column, the partial vectors added in a fixed order: no
 * floating-point atomics, the same bits on every call.  All go by the index, use buffers of their own and leave a saved plan alone.
 *   _maxabs     out[0] = max |x| over the blocks the index names (complex data: the modulus).  Synchronises.  A NaN among the elements gives NaN, here
 *               and in _gershgorin, as it does in the sums.
 *   _row_sums   out[i] = sum_j f(a_ij), f = |x| (what == 0) or |x|^2 (what == 1; any other value: -1), over the STORED blocks.  Asynchronous on stream.
 *   _col_sums   out[j] = sum_i f(a_ij); skip_diagonal_blocks != 0: blocks on the block diagonal do not count.  Asynchronous.
 *   _gershgorin out[0] = max_i sum_j |a_ij|.  symmetric != 0 (a stored triangle of any of the four symmetries; nblkrows == nblkcols, else -1): a stored
 *               block off the diagonal also adds its column sums to the rows of its twin.  Composed on the device of _row_sums, _col_sums and a maximum;
 *               synchronises once.  It sizes its vectors by the full row count, which it fetches (one more synchronisation) when a matrix' block-size
 *               arrays and non-zero index_stamp are not among the last eight it saw; a matrix with index_stamp == 0 pays that every time.  A caller that sets
 *               index_stamp itself must give every set of block-size arrays a stamp of its own: the same stamp at reused addresses with other
 *               sizes would be taken for the remembered count.
 *   _get_diag   diag[i] = a_ii from the diagonal blocks present, ZERO where a block row has no diagonal block; every one of the n elements is written.
 *   _set_diag   a_ii = diag[i] on the diagonal blocks present; nothing else is written and no block is created (dbcsr_add_on_diag with 0 creates them).
 *               Both: square block structure (nblkrows == nblkcols, else -1), diag has the matrix' data type; a diagonal block that is not square is
 *               left alone (get: zeros).  Asynchronous.
 *   _scale_by_vector  in place, side 1 (right): a_ij <- a_ij * vec[j]; side 0 (left): a_ij <- a_ij * vec[i]; any other side: -1.  vec has the matrix'
 *               data type.  Real data: one rounding per element.  Asynchronous.
 * n / n_out is the length of the vector: every read and write of it stays below, so a wrong length never touches memory outside the vector (elements whose
 * entry would lie behind it are not produced / not scaled; elements of a longer out / diag behind the full length are zero). */
int dbcsr_amd_bcsr_maxabs(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, double out[1], void* stream);
int dbcsr_amd_bcsr_row_sums(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int what, double* out, int64_t n_out, void* stream);
int dbcsr_amd_bcsr_col_sums(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int what, int skip_diagonal_blocks, double* out,
  int64_t n_out, void* stream);
int dbcsr_amd_bcsr_gershgorin(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int symmetric, double out[1], void* stream);
int dbcsr_amd_bcsr_get_diag(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, void* diag, int64_t n, void* stream);
int dbcsr_amd_bcsr_set_diag(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, const void* diag, int64_t n, void* stream);
int dbcsr_amd_bcsr_scale_by_vector(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, const void* vec, int64_t n, int side, void* stream);
/*   _matvec     y <- alpha op(A) x + beta y with dense DEVICE vectors x and y of the matrix' data type; trans 'N', 'T' or 'C' (conjugate transpose; real
 *               data: 'T'), any other: -1.  x has one element per full column of op(A), y one per full row, in the order of the dense matrix.  kind -1: the
 *               stored blocks only.  kind 0 ... 3 (S A H K; any other kind: -1): a stored triangle with a square block structure (nblkrows == nblkcols,
 *               else -1), the product is that of the desymmetrized matrix -- a stored block (r, c), r != c, gives a x[c] to the rows of r and its twin
 *               (a^T, -a^T, conj(a)^T, -conj(a)^T) x[r] to the rows of c; diagonal blocks are stored in full and count once; H and K on real data are S
 *               and A.  Composed on the device of a pass by block row and a pass by block column (the latter for 'T' / 'C' and for the twins), as
 *               _gershgorin is.  beta == 0: y is not read (a NaN in it does not reach the result).  alpha == 0: A and x are not read, y <- beta y in the
 *               data's own precision; so for an empty matrix (0).  Every element of y below the full length is written, a full row that no stored
 *               block touches gets beta y[i]; elements of a longer y behind the full length are left alone.  x and y must not overlap: -1 when
 *               [x, x + n_x) and [y, y + n_y) intersect.  Products and sums in double / complex double (fp32 products are exact), alpha and beta applied in
 *               double, one rounding to the data's type.  Every read of x stays below n_x, every write of y below n_y: a term whose entry of x would lie
 *               behind n_x is not formed, an element of y at or behind n_y is not produced.  Asynchronous, no synchronisation. */
int dbcsr_amd_bcsr_matvec(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], const dbcsr_amd_bcsr* a,
  int kind /* -1: no symmetry; 0 ... 3: S A H K */, const void* x, int64_t n_x, const double beta[2], void* y, int64_t n_y, void* stream);
/*   _multivec   Y <- alpha op(A) X + beta Y with nrhs right-hand sides handled together: A is read once for all of them.  X is n_x x nrhs, Y is
 *               n_y x nrhs, dense DEVICE matrices of the matrix' data type stored ROW BY ROW: element (i, v) at i ld + v, ld >= nrhs (a contiguous
 *               (n, nrhs) array has ld = nrhs, a column slice of a wider basis a larger ld) -- the layout in which the nrhs entries one element of A
 *               meets are consecutive.  trans, kind and every rule of _matvec hold per column: products and sums in double / complex double, one
 *               rounding to the data's type; beta == 0: Y is not read; alpha == 0 or an empty matrix: A and X are not read, Y <- beta Y in the data's
 *               own precision; a full row that no stored block touches gets beta y; no floating-point atomics, the same bits on every call;
 *               asynchronous, no synchronisation; buffers of its own, a saved plan stays.  -1 for a null argument, a bad trans or kind, kind >= 0 with
 *               nblkrows != nblkcols, nrhs < 0, ldx < nrhs or ldy < nrhs, and when the element ranges [x, x + (n_x - 1) ldx + nrhs) and
 *               [y, y + (n_y - 1) ldy + nrhs) intersect; -10 for a data type the algebra does not know; 0 with nothing written for nrhs == 0 or
 *               n_y == 0.  Every read of X stays in rows below n_x and columns below nrhs (a term whose row of X would lie behind n_x is not formed),
 *               every write of Y in rows below n_y and below the full row count of op(A) and in columns below nrhs: the padding columns
 *               nrhs ... ld - 1 of Y are never written.  One column (nrhs == 1) is served by the same kernels, not by _matvec. */
int dbcsr_amd_bcsr_multivec(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], const dbcsr_amd_bcsr* a,
  int kind /* -1; 0 ... 3: S A H K */, int nrhs, const void* x, int64_t n_x, int64_t ldx, const double beta[2], void* y, int64_t n_y, int64_t ldy,
  void* stream);
/*   _rank_update  A_IJ <- beta A_IJ + alpha X_I op(Y_J) for every block (I, J) the index of A names, in place, and nothing else: the pattern never
 *               changes, no index array is written (what cp_dbcsr_plus_fm_fm_t with keep_sparsity does).  op: trans 'T' (transpose) or 'C' (conjugate
 *               transpose; real data: 'T'), any other: -1.  X is n_x x nrhs, Y is n_y x nrhs, dense DEVICE matrices of the matrix' data type in
 *               _multivec's layout (row by row, element (i, v) at i ld + v, ld >= nrhs); X_I are the rows of X of block row I, Y_J the rows of Y of
 *               block column J.  y == x is legal, and so is any overlap of the two: both are only read; neither may overlap A's data area.  Products
 *               and sums in double / complex double (fp32 data converted first: its products are exact), alpha and beta applied in double, one
 *               rounding to the data's type per element; every element has one owner: no floating-point atomics, the same bits on every call.
 *               beta == 0: A's values are not read (a NaN in A does not reach the result).  alpha == 0 or nrhs == 0: X and Y are not read,
 *               A <- beta A in the data's own precision; with beta == 1 as well nothing is launched.  It goes by the index, never by the extent of
 *               the data area: the holes of an unpacked matrix keep their bits.  A stored triangle is updated block by block like any other matrix;
 *               which X, Y, trans and scalars keep its symmetry is the caller's business (Python: dbcsr_rank_update).  Buffers of its own, a saved
 *               plan stays; asynchronous, no synchronisation.  -1 for a null handle, matrix or scalar, a bad trans, nrhs < 0, n_x < 0 or n_y < 0,
 *               ldx < nrhs or ldy < nrhs, and a null x / y when they would be read (alpha != 0, nrhs > 0 and rows to read); -10 for a data type the
 *               algebra does not know; 0 with nothing written for an empty matrix.  Every read of X stays in rows below n_x and columns below nrhs,
 *               every read of Y in rows below n_y and columns below nrhs: rows outside a block, rows behind the tensors and padding columns are never
 *               loaded, they enter as true zeros.  An element of A whose row of X or of Y would lie at or behind n_x / n_y is not written at all; every
 *               write stays inside the blocks that the index names. */
int dbcsr_amd_bcsr_rank_update(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], int nrhs, const void* x, int64_t n_x,
  int64_t ldx, const void* y, int64_t n_y, int64_t ldy, const double beta[2], dbcsr_amd_bcsr* a, void* stream);
/*   _multiply_dense  Y <- alpha op(A) X + beta Y with a dense operand of many columns, on the matrix cores: the forward direction of _rank_update, what
 *               cp_dbcsr_sm_fm_multiply does (H C, S C).  X is n_x x ncol, Y is n_y x ncol, dense DEVICE matrices of the matrix' data type in the SAME
 *               layout: layout 0 row by row (element (i, v) at i ld + v, ld >= ncol: _multivec's), layout 1 column by column (element (i, v) at
 *               i + v ld, ld >= n_x / n_y: a Fortran full matrix or a window of one).  trans, kind, alpha == 0, beta == 0 and the empty matrix are
 *               _multivec's.  One workgroup owns a block row of op(A) and 64 columns of Y from the first block to the epilogue: no partial matrices,
 *               no floating-point atomics, the same bits on every call; within one layout the bits of a column depend neither on its position nor
 *               on the other columns.  Products and sums in double / complex double (fp32 data converted first), alpha and beta applied in double,
 *               one rounding per element.  Every element of Y in rows below n_y and below the full row count of op(A) and in columns below ncol is
 *               written exactly once -- a block row that stores nothing gets beta y (in double, one rounding), +0 for beta == 0 -- and nothing
 *               else is written.  Every read of X stays in rows below n_x and columns below ncol; rows and columns outside a block are never
 *               loaded, they enter as true zeros: an Inf or NaN in row r of X reaches only the rows of Y whose row of op(A) stores an element in
 *               column r.  Buffers of its own (the offsets and the per-column lists of the algebra; no sums), a saved plan stays; asynchronous, no
 *               synchronisation.  -1 for a null argument, a bad trans, kind or layout, kind >= 0 with nblkrows != nblkcols, ncol < 0, n_x < 0 or
 *               n_y < 0, ld below ncol (layout 0) or below n_x / n_y (layout 1), when the element ranges of X and Y intersect, and for grids above
 *               INT32_MAX; -10 for a data type the algebra does not know; 0 with nothing written for ncol == 0 or n_y == 0. */
int dbcsr_amd_bcsr_multiply_dense(void* handle, libsmm_acc_data_t datatype, char trans, const double alpha[2], const dbcsr_amd_bcsr* a,
  int kind /* -1; 0 ... 3: S A H K */, int ncol, const void* x, int64_t n_x, int64_t ldx, const double beta[2], void* y, int64_t n_y, int64_t ldy,
  int layout /* 0: row by row; 1: column by column */, void* stream);

/* Block diagonal: dbcsr_get_block_diag of the reference, and the batched inversion of the diagonal blocks that CP2K does on the host with an iterator and
 * invmat -- the initial guess X0 = blockdiag(S)^-1 of a Hotelling / Newton-Schulz inverse, and the block-Jacobi preconditioner blockdiag(A)^-1 that
 * _multivec then applies.  Same types and answers as the algebra above (-10 for another type code; -1 for a null handle or matrix and for
 * nblkrows != nblkcols).  A diagonal block is the block (r, r) the index names; of a stored triangle it is stored in full and taken as it is.  All three
 * use buffers of their own (and the scan's scratch): no saved plan is touched, no work area of the symbolic phase is written.
 *   _block_diag_count   the whole index of the matrix of the diagonal blocks m STORES, in block-row order and packed: dst_row_p [nblkrows + 1], dst_col_i /
 *     dst_blk_p [nblkrows] (device; the first *nblks entries are written, blk_p the running sum of the block sizes), and on the host *nblks, *nze and
 *     *max_dim, the largest dimension of such a block (0 when there is none).  A block row without a diagonal block has none in the result.  Synchronises
 *     once, as _diag_count does.
 *   _block_diag_apply   dst's diagonal blocks = src's diagonal blocks, bit for bit, found by both indices (dst: the index _block_diag_count made, data [nze]
 *     allocated by the caller and not src's).  Reads src only at its diagonal blocks, writes dst only inside its blocks.  Asynchronous on stream.
 *   _block_diag_invert  in place: every diagonal block m stores is replaced by its inverse; blocks off the diagonal, the holes of an unpacked matrix and
 *     everything else of the data area keep their bits; no index array is written.  Gauss-Jordan with partial (row) pivoting on a copy of the block in
 *     LDS, in double / complex double for all three types (real_4: converted on load, rounded once on store).  The pivot of a column is the largest |x|
 *     (complex data: |re| + |im|) at or below the diagonal, the lowest row on ties, compared with > so that a NaN never wins.  The bits of an inverse depend
 *     on the block's values, dimension and type alone -- not on where the block lies, on the alignment of the data area, on the other blocks or on the
 *     call; no atomics on data.  A block with a pivot column that is exactly zero (or all NaN) is SINGULAR: it is not written at all, it is counted, and
 *     every other block is still inverted.  A block that holds Inf or NaN gets no promise about its own values; the writes stay inside it.
 *     max_dim is the caller's bound on the dimension of a diagonal block (it sizes the LDS of the launch): one wave inverts a block of up to 32, one
 *     workgroup of 256 a block of 33 ... 96, both kinds in one call.  A diagonal block whose dimension exceeds max_dim (or that is not square) is SKIPPED:
 *     left untouched and counted, never a fault.  info may be NULL: then nothing synchronises.  Otherwise (host; synchronises once) info[0] = the number
 *     of singular blocks, info[1] = the first such block row or -1, info[2] = the number of skipped blocks.  -1 also for max_dim < 0; -11 for max_dim
 *     above 96, the supported limit (96 x 97 complex doubles fill the LDS of a compute unit), with nothing launched; 0 with nothing written for an empty
 *     matrix (info = {0, -1, 0}). */
int dbcsr_amd_bcsr_block_diag_count(void* handle, const dbcsr_amd_bcsr* m, int32_t* dst_row_p, int32_t* dst_col_i, int64_t* dst_blk_p,
  int64_t* nblks, int64_t* nze, int32_t* max_dim, void* stream);
int dbcsr_amd_bcsr_block_diag_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);
int dbcsr_amd_bcsr_block_diag_invert(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, int max_dim, int64_t info[3], void* stream);

/* Block diagonal times matrix: the block analogue of _scale_by_vector, in place on every block the index of m names and on nothing else -- D^-1 A of a
 * block-Jacobi preconditioner, X0 S of a Hotelling / Newton-Schulz inverse, and as two calls a block congruence D A D^T -- without a symbolic phase, a
 * plan or a second matrix: the product has the pattern of m itself.
 *   _block_diag_multiply  side 'L': A_IJ <- alpha op(D_I) A_IJ; side 'R': A_IJ <- alpha A_IJ op(D_J); D_I the diagonal block (I, I) that diag stores.
 *     Blocks of diag off the diagonal are never read: the operand is blockdiag(diag).  A block row of diag without a stored diagonal block counts as a zero
 *     block: the blocks of m in that block row (L) or block column (R) become +0.0 and their old values are not read.  op: trans 'N', 'T' (transpose),
 *     'C' (conjugate transpose; real data: 'T') or 'J' (the conjugate, not transposed; real data: 'N' -- the second pass of a congruence with op = T).
 *     diag has a square block structure whose block sizes are m's row block sizes (L) or column block sizes (R): the caller's contract, as is that the
 *     two data areas do not overlap (-1 when they start at the same address).  max_dim is the caller's bound on the dimension of a diagonal block; the
 *     other dimension of a block of m is not limited.  Products and sums in double / complex double (real_4 converted on load), alpha applied in double,
 *     one rounding to the data's type per element; a strip of 16 element columns (L) or rows (R) of a block is read completely before any of it is
 *     stored and has one owner: no atomics, the same bits on every call.  alpha == 0: every element of every stored block becomes +0.0 and neither
 *     operand's data is read.  No index array is written; the holes of an unpacked matrix and everything around the blocks keep their bits; buffers
 *     of the symbolic phase are not touched, a saved plan stays.  Asynchronous on stream, no synchronisation.  -1 for a null handle, scalar or matrix,
 *     a bad side or trans, max_dim < 0, diag->nblkrows != diag->nblkcols or != m's block rows (L) / block columns (R); -10 for a data type the algebra
 *     does not know; -11 for max_dim above 96 (what _block_diag_invert can invert can be applied), with nothing launched; 0 with nothing written for
 *     an empty matrix. */
int dbcsr_amd_bcsr_block_diag_multiply(void* handle, libsmm_acc_data_t datatype, char side /* 'L' 'R' */, char trans, const double alpha[2],
  const dbcsr_amd_bcsr* diag, dbcsr_amd_bcsr* m, int max_dim, void* stream);

/* Dense conversion: dbcsr_to_dense_local of the reference and CP2K's copy_dbcsr_to_fm / copy_fm_to_dbcsr(keep_sparsity), between a matrix and a dense
 * device tensor, without leaving the device.  `dense` is the window [n_rows, n_cols] of elements of the data type, element (i, j) at i * ld + j
 * (col_major 0: row by row, as a torch tensor or a column slice of a wider one; ld >= n_cols) or at i + j * ld (col_major != 0: column by column, as a
 * Fortran full matrix; ld >= n_rows).  Offsets into it are formed in 64 bits.  Same types as the algebra above (-10 for another type code).  -1 for a null
 * handle or matrix, a negative n_rows / n_cols, an ld below the window's contiguous extent, n_rows / n_cols that are not the sums of the row / column block
 * sizes, and a null dense with a window that has elements (a null dense is legal with an empty window: 0, nothing written).  The sums are known on the
 * device alone: _to_dense and _from_dense_apply remember them per set of block sizes (same size arrays and the same non-zero index_stamp) and synchronise
 * once when they meet a set they do not know -- otherwise they are asynchronous on stream and synchronise nothing.  All three work in buffers of the
 * algebra (and the scan's scratch): no saved plan is touched, no work area of the symbolic phase is written.  No atomics on data; the same bits on every
 * call.  The tensor must not overlap the data area of m (the caller's contract, as for _rank_update).
 *   _to_dense          every element of the window is written exactly once: a stored block at its place, bit for bit, +0.0 everywhere else; nothing outside
 *     the window is written (the padding between the window's extent and ld keeps its bits).  kind -1: the stored blocks only.  kind 0 ... 3 (S A H K; any
 *     other kind, or nblkrows != nblkcols: -1): a stored triangle is expanded as _desymmetrized does -- where (r, c) is not stored and (c, r) is, the tile
 *     is the twin of that block (transposed; bit 0 of kind negates, bit 1 conjugates: sign flips, exact); a diagonal block is taken in full as stored.
 *     m is only read.
 *   _from_dense_apply  every block the index of m names <- the window's elements at its place, bit for bit, and nothing else: no index array is written,
 *     the holes of an unpacked matrix and everything around the blocks keep their bits.  No symmetry is applied: of a stored triangle the blocks stored are
 *     taken from where they lie, the other triangle of the window is not read.  The norms a numeric phase announced are forgotten.
 *   _from_dense_count  the count half of "a new packed matrix of the tiles of the window that the block filter keeps" (the apply half is
 *     _from_dense_apply with the index made here): a tile of the block structure row_blk_size [nblkrows] x col_blk_size [nblkcols] (device) is DROPPED iff
 *     ||tile||_F^2 < eps^2 (filter_count's rule: a NaN norm stays, eps == 0 keeps every tile), norms summed in double in a fixed order.  Writes dst_row_p
 *     [nblkrows + 1], dst_col_i / dst_blk_p [nblkrows * nblkcols] (device; the first *nblks entries are written: ascending columns inside a row, blk_p the
 *     running sum of the block sizes) and *nblks, *nze on the host.  Synchronises once.  -1 also for eps < 0 or NaN and for a block structure of more than
 *     2^31 - 9 tiles; when the sums do not match, nothing of the window has been read. */
int dbcsr_amd_bcsr_to_dense(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int kind /* -1, or 0 ... 3: S A H K */, void* dense,
  int64_t n_rows, int64_t n_cols, int64_t ld, int col_major, void* stream);
int dbcsr_amd_bcsr_from_dense_apply(void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n_rows, int64_t n_cols, int64_t ld, int col_major,
  dbcsr_amd_bcsr* m, void* stream);
int dbcsr_amd_bcsr_from_dense_count(void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n_rows, int64_t n_cols, int64_t ld, int col_major,
  const int32_t* row_blk_size, const int32_t* col_blk_size, int nblkrows, int nblkcols, double eps, int32_t* dst_row_p, int32_t* dst_col_i,
  int64_t* dst_blk_p, int64_t* nblks, int64_t* nze, void* stream);

/* Submatrix method: the data movement of "a dense function of a large sparse matrix, one small dense principal submatrix per block column (or group of
 * block columns) at a time" -- batched windows out of the matrix and back onto its pattern, without leaving the device.  Not a mirror of a routine of the
 * reference.  m has a square block structure whose row block sizes are its column block sizes (nblkrows != nblkcols: -1; equal sizes are the caller's
 * contract).  The index sets are the caller's (device, int32): submatrix g = 0 ... nsub - 1 is the ascending set of block rows set_idx[set_ptr[g] ...
 * set_ptr[g + 1]), set_off [as set_idx] the element offset of each member inside the submatrix (the running sum of the members' block sizes), sub_dim
 * [nsub] its side n_g; owner [nblkcols] the submatrix that block column belongs to, -1 for none.  `dense` is a batch of windows of n x n elements of the
 * data type, one per slot, row by row: element (i, j) of slot t at t * batch_stride + i * ld + j, every offset formed in 64 bits.  Same types as the
 * algebra above (-10 for another type code).  -1 for a null handle or matrix, a negative count, n above 2^31 - 1, ld < n, batch_stride < n * ld with
 * more than one slot (_gather; _scatter: batch_stride < 0), a kind outside -1 ... 3, and a null tensor with a non-empty batch; 0 with nothing written for
 * nslot == 0 or n == 0 (_scatter: also nsub == 0 or a matrix without blocks).  Both are asynchronous on stream and synchronise nothing; they use no
 * buffer of the engine, no saved plan is touched.  No atomics, no memset; the same bits on every call.  The tensor must not overlap the data area of m
 * (the caller's contract).  Sets that do not fit the matrix give wrong values but never an access outside the windows: a member outside the block
 * structure, or whose run set_off + size passes n, is skipped whole, and a submatrix id outside 0 ... nsub - 1 counts as an empty set.
 *   _submatrix_gather   slot t = 0 ... nslot - 1 holds submatrix g = slot_sub[t] (slot_sub null: g = t).  Its window receives every tile (a, b) of
 *     S_g x S_g that m stores at (set_off[a], set_off[b]), bit for bit; for kind 0 ... 3 (S A H K) the twin of the block stored at (b, a) where (a, b) is
 *     not stored (transposed; bit 0 of kind negates, bit 1 conjugates: sign flips, exact), a diagonal block taken in full as stored -- _to_dense's
 *     reading; +0.0 everywhere else inside n_g x n_g; outside n_g x n_g and inside n x n, +0.0 off the diagonal and pad_diag on it (complex:
 *     (pad_diag, 0)), so that the window is blockdiag(A[S, S], pad_diag I).  Every element of every window is written exactly once per call, a window
 *     of a set without members included; nothing outside a window is written: the columns n ... ld - 1 and whatever lies between two windows keep
 *     their bits.  max_members: the largest number of members among the submatrices of the batch (or of all).  m is only read.
 *   _submatrix_scatter  every block (R, C) the index of m names with g = owner[C] >= 0, t = sub_slot[g] >= 0 (sub_slot [nsub]: the slot that holds
 *     submatrix g, -1 for none) and R a member of S_g (binary search) <- the elements at (set_off[pos R], set_off[pos C]) of window t, bit for bit.
 *     Everything else keeps its bits: blocks of block columns without an owner or whose submatrix has no slot, blocks whose row is no member, the holes
 *     of an unpacked matrix, every index array.  No symmetry is applied: of a stored triangle the blocks stored are taken from where they lie.  The
 *     norms a numeric phase announced are forgotten. */
int dbcsr_amd_bcsr_submatrix_gather(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int kind, int nsub, const int32_t* set_ptr,
  const int32_t* set_idx, const int32_t* set_off, const int32_t* sub_dim, int nslot, const int32_t* slot_sub, int max_members, void* dense, int64_t n,
  int64_t ld, int64_t batch_stride, double pad_diag, void* stream);
int dbcsr_amd_bcsr_submatrix_scatter(void* handle, libsmm_acc_data_t datatype, const void* dense, int64_t n, int64_t ld, int64_t batch_stride, int nsub,
  const int32_t* set_ptr, const int32_t* set_idx, const int32_t* set_off, const int32_t* owner, const int32_t* sub_slot, dbcsr_amd_bcsr* m,
  void* stream);

/* Element-wise operations on two patterns (src/ops/dbcsr_operations.F: dbcsr_hadamard_product, dbcsr_copy with keep_sparsity,
 * dbcsr_function_of_elements), for the types of the algebra above (any other type code: -10; the functions: real types only).  Every operation goes by the
 * index, never by the extent of a data area, and relies on ascending block columns per block row as the algebra does: the partner of a block in the
 * other matrix is found by a binary search of that matrix' row.  NULL arguments and matrices whose nblkrows / nblkcols differ: -1.  They use buffers of
 * their own: the work areas of the symbolic phase are not touched and a saved plan stays, for two patterns as well.
 *
 * dbcsr_hadamard_product: C <- A o B, element by element.  The result has the blocks BOTH operands store, in A's order, packed; with b_assumed / b_value
 * it has every block of A, and a block B lacks counts as filled with b_value (a b_value of exactly 1 copies A's block bit for bit).  Real data: one
 * multiplication per element, a * b in the data's precision bit for bit; complex data: re = ar br - ai bi, im = ar bi + ai br in double.  Matrices with
 * symmetry are multiplied on their stored triangles as they are (the caller checks that the product keeps the symmetry class).  The reference's source
 * could not be consulted for the pattern of the result: this is the semantics of this library.  Two steps, as the add:
 *   _hadamard_count  writes dst_row_p [nblkrows + 1] (device) and the block / element counts of the result (host; synchronises).  *same_pattern = 1: A and
 *     B have the same row_p, col_i AND blk_p and A is packed (the add's check).  b_assumed != 0: the _apply will be given a b_value.
 *   _hadamard_apply  fills dst (dst->row_p = that row_p; col_i, blk_p [nblks], data [nze] allocated by the caller).  b_value NULL: the intersection; it must
 *     be given exactly when _count was told b_assumed.  When _count reported same_pattern, dst may be a or b itself: one flat pass over the data area in
 *     place, no index array is written; a dst with index arrays of its own receives copies of a's.  Otherwise a dst whose data area is a's or b's is
 *     refused (-1).  One _apply per _count: an _apply without a pending _count, or with operands whose block counts differ from the counted ones, is
 *     refused (-1) and writes nothing.  What is pending lives in fields and buffers of its own: an add, a norm or a multiply between the two halves does
 *     not disturb it and is not disturbed by it.  Asynchronous on stream. */
int dbcsr_amd_bcsr_hadamard_count(void* handle, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, int b_assumed, int32_t* dst_row_p, int64_t* nblks,
  int64_t* nze, int* same_pattern, void* stream);
int dbcsr_amd_bcsr_hadamard_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b,
  const double b_value[2] /* NULL: intersection */, dbcsr_amd_bcsr* dst, void* stream);
/* dbcsr_copy with keep_sparsity: every block the index of dst names <- src's block (r, c) bit for bit, +0.0 in every element where src stores no such
 * block.  Only dst's data area is written, and of it only the elements its index names: the holes of an unpacked dst and every index array keep their
 * bits.  No count step, nothing synchronises: asynchronous on stream.  The blocks of src and dst must not overlap (the caller's
 * contract). */
int dbcsr_amd_bcsr_copy_onto(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);
/* dbcsr_function_of_elements: in place, x <- f(a1 * x + a0) on every element the index of m names (holes keep their bits), formed in double and rounded
 * once for real_4.  With y = a1 * x + a0: _inverse 1 / y, _tanh tanh y, _dtanh a1 (1 - tanh^2 y), _ddtanh -2 a1^2 tanh y (1 - tanh^2 y), _artanh atanh y,
 * _sin sin y, _dsin a1 cos y, _ddsin -a1^2 sin y, _asin asin y, _cos cos y, _dcos -a1 sin y, _ddcos -a1^2 cos y.  The reference has three functions more
 * (inverse_special, spread_from_zero, truncate: codes 5, 6, 14) and a third parameter; their definitions could not be checked and are not guessed: any
 * other func is refused (-1).  Complex types: -10.  Asynchronous on stream. */
enum {
  dbcsr_func_inverse = 0, dbcsr_func_tanh = 1, dbcsr_func_dtanh = 2, dbcsr_func_ddtanh = 3, dbcsr_func_artanh = 4, dbcsr_func_sin = 7,
  dbcsr_func_dsin = 8, dbcsr_func_ddsin = 9, dbcsr_func_asin = 10, dbcsr_func_cos = 11, dbcsr_func_dcos = 12, dbcsr_func_ddcos = 13
};
int dbcsr_amd_bcsr_function_of_elements(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, int func, double a0, double a1, void* stream);

/* Block lists (src/block/dbcsr_block_access.F: dbcsr_reserve_blocks, dbcsr_put_block with summation and scale, dbcsr_get_block_p; the merge of the work
 * matrices in dbcsr_finalize), for the types of the algebra above (any other type code: -10).  A list is rows[n], cols[n] (int32, device): entry i names
 * block (rows[i], cols[i]); any order, duplicates allowed.  Put and get move the blocks through ONE flat area of the matrix' type: entry i's window starts
 * at element off[i] (int64, device) of it and holds rs[rows[i]] * cs[cols[i]] elements, column-major as the library stores blocks.  Every operation goes by
 * the index and relies on ascending block columns per block row.  A matrix with symmetry is served on its stored triangle as it is: a block below the
 * diagonal is not transposed onto its twin.  NULL arguments, n < 0, more than 2^31 - 1 entries or blocks: -1.
 *
 * dbcsr_reserve_blocks: the pattern grows to the union of the matrix' pattern and the list.  Every block the matrix stores keeps its bits, every new block
 * is +0.0, the result is packed with ascending block columns per row.  Two steps, as add / filter / crop:
 *   _reserve_count  counts (host; synchronises once): *n_invalid entries outside [0, nblkrows) x [0, nblkcols), or with upper_only != 0 (square matrices
 *     only: the stored triangle of a matrix with symmetry) below the diagonal -- with any of them nothing is pending and the caller refuses the list;
 *     *n_new blocks the list names and the matrix lacks (a block named twice counts once).  *n_new == 0: there is nothing to apply, and no work area
 *     of the symbolic phase and no saved plan was touched -- a multiply afterwards reuses its plan.  Otherwise *nblks / *nze are the counts of the
 *     result, dst_row_p [nblkrows + 1] (device) receives its row_p, and the call has taken the symbolic phase's work areas and invalidated the saved
 *     plan, as the union add does.
 *   _reserve_apply  fills dst (dst->row_p = that row_p; col_i, blk_p [nblks], data [nze] allocated by the caller; dst's data area is not m's).
 *     Asynchronous on stream.  One _apply per _count: an _apply without a pending _count, after anything else took the work areas, or for a matrix
 *     other than the counted one (row_p, sizes, block count) is refused (-1) and writes nothing.  What is pending lives in fields of its own; a put, a get
 *     or a norm between the two halves disturbs nothing.
 *
 * dbcsr_put_block: per entry A_rc <- A_rc + alpha X (summation != 0) or A_rc <- alpha X.  Entries out of range or whose block the matrix does not store
 * are skipped.  Contributions to one block are applied IN LIST ORDER: with summation all of them are added in that order, without it the last one of the
 * list wins.  With alpha exactly 1 nothing is multiplied: an overwrite is bit for bit, a sum is the type's own addition.  The same bits on every call; no
 * floating-point atomics.  Only elements the index names are written (holes keep their bits), no index array is written, nothing synchronises, no work
 * area of the symbolic phase and no saved plan is touched: asynchronous on stream.  The windows must lie inside src and src must not overlap the matrix'
 * data area (the caller's contract).
 *
 * dbcsr_get_block_p: every window <- the block bit for bit and found[i] = 1, or +0.0 and found[i] = 0 where the matrix stores no such block; an entry out
 * of range has no window (found[i] = 0, nothing else written).  Every element of every window is written exactly once, nothing outside.  The windows
 * must lie inside dst and must not overlap each other or the matrix' data area (the caller's contract).  No saved plan, no work area: asynchronous. */
int dbcsr_amd_bcsr_reserve_count(void* handle, const dbcsr_amd_bcsr* m, int64_t n, const int32_t* rows, const int32_t* cols, int upper_only,
  int32_t* dst_row_p, int64_t* nblks, int64_t* nze, int64_t* n_new, int64_t* n_invalid, void* stream);
int dbcsr_amd_bcsr_reserve_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, dbcsr_amd_bcsr* dst, void* stream);
int dbcsr_amd_bcsr_put_blocks(void* handle, libsmm_acc_data_t datatype, dbcsr_amd_bcsr* m, int64_t n, const int32_t* rows, const int32_t* cols,
  const int64_t* src_off, const void* src, const double alpha[2], int summation, void* stream);
int dbcsr_amd_bcsr_get_blocks(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int64_t n, const int32_t* rows, const int32_t* cols,
  const int64_t* dst_off, void* dst, int32_t* found, void* stream);

/* Element CSR: the reference's conversion between a matrix and the element-wise CSR form (src/ops/dbcsr_csr_conversions.F: dbcsr_csr_create_from_dbcsr,
 * dbcsr_convert_dbcsr_to_csr, dbcsr_convert_csr_to_dbcsr, dbcsr_to_csr_filter; what CP2K hands to PEXSI and writes with KS_CSR_WRITE), without leaving
 * the device.  The reference's source could not be consulted: the rule of the eps filter stated below is the semantics of this library.  The CSR form of
 * this library: crow[n_rows + 1] int64 with crow[0] = 0 (positions pass 2^31 on matrices that fit one GPU), col[nnz] int32, 0-based element columns
 * ascending inside a row, values[nnz] of the matrix' type; all three on the device.  Same types as the algebra above (-10 for another type code).  -1 for a
 * null handle, matrix or array, negative sizes, and more than 2^31 - 1 element columns; 0 with nothing but crow written for a matrix without blocks.  The
 * index is served as it is: a stored triangle is not expanded (dbcsr_amd_bcsr_desymmetrized does that first).  Everything goes by the index: the holes of
 * an unpacked matrix are never read or written.  All four work in buffers of their own (and the scan's scratch): no saved plan is touched, no work area of
 * the symbolic phase is written.  No atomics on data; the same bits on every call; every offset into the data area, col and values is formed in 64 bits.
 *   _to_csr_count  writes crow [n_rows + 1] (device) and *nnz (host).  use_eps == 0: every element the index names is an entry -- crow and *nnz come from
 *     the index alone and NO element of the data area is read (m->data may point anywhere).  use_eps != 0 (eps >= 0; negative or NaN: -1): an element is
 *     DROPPED iff |x| <= eps -- real types compare in their own precision, complex ones hypot(re, im) in double -- so eps = 0 drops exactly +-0 and a NaN
 *     stays.  Synchronises once, for *nnz; once more when it meets an index it does not know (same row_p and size arrays, same non-zero index_stamp), for
 *     the number of row pieces it works on, as _to_dense does for the lengths; with use_eps == 0 and a known index it synchronises nothing.  -1 also for
 *     more than 2^31 - 9 row pieces (element rows times stored blocks of their block row, summed).
 *   _to_csr_apply  fills col and values [nnz], bit for bit.  Asynchronous on stream.  One _apply per _count: an _apply without a pending _count, a second
 *     one, or one for a matrix other than the counted one (row_p, the size arrays, the block counts, the type) is refused (-1) and writes nothing.  What is
 *     pending lives in fields and buffers of its own: an add, a norm, a put or a multiply between the two halves does not disturb it and is not
 *     disturbed by it.  With eps the data area must be the counted one; one that changed gives wrong entries, never a store outside col / values[0, nnz).
 *   _from_csr      the mirror of _from_dense_apply: every element of every block the index of m names is written exactly once -- the CSR value at its
 *     (row, column), or +0.0 where the CSR has none -- and nothing else: no index array, no hole of an unpacked matrix.  CSR entries whose block m does not
 *     store are ignored, as are entries with a column outside [0, n_cols).  Contract: columns ascend strictly inside a row (what _to_csr_apply and
 *     torch's to_sparse_csr() produce); a CSR that breaks it gives wrong values, never an access outside col / values[0, nnz) -- every position formed
 *     from crow is clamped -- or outside the blocks.  -1 for n_rows / n_cols that are not the sums of the block sizes (remembered per set of block sizes
 *     as _to_dense remembers them: one synchronisation the first time, none afterwards).  No symmetry is applied.  The norms a numeric phase announced
 *     are forgotten.  Asynchronous on stream.
 *   _csr_name_blocks  rows[t], cols[t] (int32 [nnz], device) <- the block (R, C) of the structure row_blk_size [nblkrows] x col_blk_size [nblkcols] (device)
 *     that holds CSR entry t, found by binary searches in the running sums of the block sizes; (-1, -1) for an entry outside the structure (or one that
 *     no row of crow[0 ... n_rows] covers), which _reserve_count then reports as invalid.  The list is what _reserve_count takes to build the pattern of
 *     "a new matrix of the blocks that hold at least one CSR entry".  Asynchronous on stream. */
int dbcsr_amd_bcsr_to_csr_count(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int use_eps, double eps, int64_t* crow, int64_t* nnz,
  void* stream);
int dbcsr_amd_bcsr_to_csr_apply(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* m, int32_t* col, void* values, void* stream);
int dbcsr_amd_bcsr_from_csr(void* handle, libsmm_acc_data_t datatype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* crow, const int32_t* col,
  const void* values, dbcsr_amd_bcsr* m, void* stream);
int dbcsr_amd_bcsr_csr_name_blocks(void* handle, int64_t n_rows, int64_t nnz, const int64_t* crow, const int32_t* col, const int32_t* row_blk_size,
  const int32_t* col_blk_size, int nblkrows, int nblkcols, int32_t* rows, int32_t* cols, void* stream);

/* Re-blocking: a matrix under another block structure, without leaving the device and without leaving the block-sparse form (dbcsr_amd/reblock.py).
 * The reference has the capability in dbcsr_complete_redistribute (a copy between matrices of different blockings: CP2K goes from atomic to molecular or
 * clustered blocks with it) and, for tensors, in dbcsr_t_split_blocks; their sources could not be consulted: the two rules below are the semantics of
 * this library.  A is a matrix without symmetry (a stored triangle is served as the blocks it stores: dbcsr_amd_bcsr_desymmetrized expands it first),
 * (rs', cs') a second block structure whose sizes are >= 1 and have the same sums.
 *   pattern  a new block (I, J) is stored iff its element rectangle intersects the rectangle of at least one block that A's index names.  Values play no
 *            part: a stored block full of zeros counts, the holes of an unpacked data area are never read.
 *   values   an element of a stored new block is the element of A at the same (row, column), bit for bit (-0.0, NaN and +-Inf included), where A's index
 *            names a block there, and +0.0 elsewhere.
 * Blocks are column-major as everywhere.  Same types as the algebra above.  The three entries work in buffers of their own (and the scan's scratch): no
 * saved plan and no work area of the symbolic phase is touched by _reblock_name_blocks and _reblock_gather.
 *   _reblock_name_blocks  the counterpart of _csr_name_blocks.  A source block covers a span of new block rows and a span of new block columns, found by
 *     binary searches in the running sums of the new sizes (new_row_blk_size [new_nblkrows], new_col_blk_size [new_nblkcols], device); it names
 *     rowspan x colspan pieces.  Two calls.  With rows == cols == NULL: *n_pieces (host) <- the total; synchronises once.  With both lists (int32
 *     [*n_pieces], device; *n_pieces is then read as their length): rows[t], cols[t] <- the new block of piece t, the pieces of one source block
 *     together; nothing is stored at or behind *n_pieces; asynchronous on stream.  The list names a new block once per source block that meets it; it
 *     is what _reserve_count takes on an empty matrix of the new structure.  A source block outside the new structure or of no element names nothing.
 *     -1 for null arguments, one list without the other, and a total of 2^31 - 1 pieces or more.
 *   _reserve_apply_index  _reserve_apply without the data pass: of what the pending _reserve_count counted it writes dst->col_i and dst->blk_p only (and
 *     sets dst->nblks), as _filter_apply_index stands beside _filter_apply -- so that a caller who writes every element of the new data area itself
 *     need not have it zero-filled first.  dst->data is not read.  The same pending-state rules: an apply without a pending count, a second one, one
 *     after anything else took the work areas, or one for another matrix than the counted one is refused (-1) and writes nothing.
 *   _reblock_gather  the move.  For every block the index of dst names, every element is written exactly once by the values rule with src as A, and
 *     nothing else: no index array, no hole of an unpacked dst.  dst may be any pattern of any structure with the same sums: the new matrix that the
 *     two entries above made, or an existing one (the keep_sparsity form and the way back).  One workgroup per (new block, tile of at most 32 x 32
 *     elements); a lookup table in LDS holds the data offset of every source block that crosses the tile; 16-byte stores aligned on dst; no atomics, no
 *     scratch, no memset; every offset is formed in 64 bits; the same bits on every call.  It synchronises nothing, except when it meets a set of block
 *     sizes for the first time, for their sums, as _to_dense remembers them.  The block norms a numeric phase announced are forgotten.
 *     -1 for null arguments, sums that differ and src->data == dst->data; -10 for other type codes; 0 with nothing done for a dst without blocks. */
int dbcsr_amd_bcsr_reblock_name_blocks(void* handle, const dbcsr_amd_bcsr* src, const int32_t* new_row_blk_size, const int32_t* new_col_blk_size,
  int new_nblkrows, int new_nblkcols, int64_t* n_pieces, int32_t* rows, int32_t* cols, void* stream);
int dbcsr_amd_bcsr_reserve_apply_index(void* handle, const dbcsr_amd_bcsr* m, dbcsr_amd_bcsr* dst, void* stream);
int dbcsr_amd_bcsr_reblock_gather(void* handle, libsmm_acc_data_t datatype, const dbcsr_amd_bcsr* src, dbcsr_amd_bcsr* dst, void* stream);

/* Tensors: the one device primitive under the block-sparse tensor interface (dbcsr_amd/tensor.py, the dbcsr_t_* of the reference's src/tensors).  A tensor
 * is stored as a matrix without symmetry: a mapping (map1 | map2) folds its dimensions into block rows and block columns, the first entry of each tuple
 * running fastest, for the block index and inside a block alike; a stored block is the Fortran array of the tensor block with its dimensions in the order
 * map1 ++ map2.  The reference's sources could not be consulted: the layout is the one stated here and in DESIGN 3.19, checked against dense numpy.
 * Changing the mapping of a tensor -- and with it every contraction whose operands are not folded the way the multiply needs them -- is index work on
 * nblks integers plus one move that permutes the inside of every block.  The move is this call; everything else is the matrix interface above.
 *   _tensor_permute_blocks  moves a list of nblk blocks in one launch.  Entry b is the Fortran array of extents ext[4 b ... 4 b + 3] (int32, device; in the
 *     order the source stores them; entries from `rank` on are not read and count as 1) at src + src_off[b]; it is written at dst + dst_off[b] with its
 *     dimensions permuted: dimension j of the written array is dimension perm[j] of the read one (numpy.transpose's convention; perm: `rank` entries on
 *     the HOST, one permutation for the whole launch).  Offsets are int64 ELEMENT offsets (device), src_len / dst_len the element counts of the two areas;
 *     every address is formed in 64 bits.  Bit for bit: elements of 4, 8 or 16 bytes are loaded and stored, never computed with.  Every element of every
 *     written window is written exactly once, nothing else of dst is written, src is never written.  An entry is skipped on the device as a whole -- not
 *     read, not written -- when one of its windows does not lie inside [0, src_len) / [0, dst_len), when an extent is below 1, or when it has 2^31
 *     elements or more (a block's element count is 32-bit everywhere in this library).  Written windows that overlap each other are the caller's error.
 *     Dimensions that are adjacent on both sides in the same order are moved as one, extents of 1 drop out; what is left with the same fastest dimension
 *     on both sides is copied in runs with 16-byte accesses aligned on the written side, anything else goes through a 32 x 33 LDS tile so that both
 *     sides are walked along their contiguous direction.  No atomics, no scratch, no memset, no buffer of the engine, no saved plan, no
 *     synchronisation: asynchronous on stream.  The block norms a numeric phase announced are forgotten (dst may be a data area).
 *     0 on success and for nblk == 0; -1 for a null handle or array, negative counts, a rank outside 2 ... 4, a perm that is no permutation of
 *     0 ... rank - 1, [src, src + src_len) overlapping [dst, dst + dst_len), and a list too long for one grid; -10 for complex_4 and unknown type codes. */
int dbcsr_amd_tensor_permute_blocks(void* handle, libsmm_acc_data_t datatype, int64_t nblk, int rank, const int* perm, const int32_t* ext,
  const int64_t* src_off, const int64_t* dst_off, const void* src, int64_t src_len, void* dst, int64_t dst_len, void* stream);

/* Measurement helper (bench.py, roofline.fabric): what the L2 <-> Infinity-Cache fabric of the current device delivers, in TB/s -- a
 * plain streaming read of a 160 MB window by all CUs, and the block gather of the block-product dataflow (4232-byte blocks from
 * pseudo-random places of the window into LDS, whole 128-byte lines counted).  Takes well under a second; synchronises the device. */
int dbcsr_amd_fabric_probe(double* stream_tb_per_s, double* gather_tb_per_s);

#if defined(__cplusplus)
}
#endif
#endif
