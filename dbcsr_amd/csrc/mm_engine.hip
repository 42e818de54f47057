// mm_engine.hip -- device-resident local multiply (include/dbcsr_amd_mm.h).
//
// Symbolic phase (integer, HBM/L2-bound): block-level bitmaps.
//   Bbm[k][w]  : bit j set iff B(k,j) present                 (bitmap_from_index)
//   Cbm[i][w]  = Cin_bm[i][w] | OR_{k in A-row(i)} Bbm[k][w]  (c_bitmap)
//   row prefix popcounts give, without any hashing, the sorted column index of
//   C (what dbcsr_finalize produces, work/dbcsr_work_operations.F:749+) and the
//   rank of any block inside its row (row_prefix).
//   For every C block the list of products (a_off, b_off, k) is emitted in
//   ascending k: deterministic, no atomics (count_products / fill_products).
// This restates WHAT dbcsr_mm_csr_multiply_low computes (mm/dbcsr_mm_csr.F:
// 257-357: which C blocks exist, which (A,B) pairs feed each) with a data-
// parallel algorithm instead of its per-thread hash tables and 30000-entry
// parameter stacks.
//
// Numeric phase (fp64/fp32 MFMA): one wavefront per C block, all products of
// the block accumulated in registers, C written exactly once (no atomics, no
// zero-fill pass, bitwise reproducible).  Kernels, chosen per launch by choose_numeric (mm_choose.h):
//   mm_numeric_f64_hot<M,N,K> / mm_numeric_f32_hot<M,N,K>  exact-size kernels, one (m, n, k) dominates (cubes 9..32)
//   mm_numeric_f64_tiny                                    C blocks of at most 4 x 4: four C blocks per wave
//   mm_numeric_f64_small<D>                                every block dimension at most 8: one 8 x 8 tile per wave, whole blocks per 8-byte load (mm_numeric_f64_small.h)
//   mm_numeric_f64_lds<MAXT> / mm_numeric_f64_pipe<MAXT>   any sizes up to 32 (pipe: mixed sizes, few products per block)
//   mm_numeric_f32_lds                                     fp32, any sizes up to 32
//   mm_numeric_f64 / mm_numeric_f32                        blocks above 32 (32 x 32 tiles, fragments from global memory)
//   mm_numeric_z64<MA,NC>                                  complex_8, any sizes: two accumulator sets, operands in slabs of 8 inner indices (mm_numeric_z64.h)
// Around them: transpose, checksum, synthetic fill, norm filter, crop / window scale (submatrix limits), and the algebra between multiplies
// (mm_algebra.h: add, add_on_diag, trace, dot, Frobenius norm, the norms and vectors, the matrix-vector product; mm_multivec.h; mm_rank_update.h; the walk
// over the elements of a block that they share: mm_block_walk.h).
//
// Files of this translation unit (included below, inside namespace dbcsr_amd unless they open it themselves):
//   mm_choose.h          WHICH kernel runs: SizeFacts / Switches / LabSwitches -> NumericChoice, the instance lists and their predicates (plain C++, no HIP)
//   mm_mid.h             NumericArgs (the operands every launcher takes) and the launcher of the slab kernels (their own translation unit, mm_mid.hip)
//   mm_engine_state.h    struct Engine: work areas, the SizeFacts carried from symbolic to numeric, switches, plan, the lab build's LabState
//   mm_engine_env.h      the environment switches, read once per engine
//   mm_engine_launch.h   launch dispatchers (sizes -> template instance)
//   mm_engine_plan.h     plan reuse
//   mm_engine_lab.h      lab build: hosts of the experimental dataflows and their family switch
//   mm_engine_ops.h      init_c, crop, filter, checksum, fill, transpose, twin moves, statistics
//   mm_engine_algebra.h  add (count / apply), add_on_diag pieces, trace, dot, norm, norms and vectors, matvec, multivec, rank update, multiply_dense (kernels:
//                        mm_algebra.h, mm_multivec.h, mm_rank_update.h, mm_spmm.h, over the block walk of mm_block_walk.h), the block diagonal (mm_block_inverse.h), its product with a
//                        matrix (mm_block_scale.h), the dense conversion (mm_dense.h) and the submatrix method (mm_submatrix.h)
//   mm_engine_csr.h      the element CSR form (kernels: mm_csr.h)
//   mm_engine_reblock.h  a matrix under another block structure (kernels: mm_reblock.h)
//   mm_engine_tensor.h   block-sparse tensors: the permuting move (kernel: mm_tensor.h)
// This file: create / destroy, the symbolic phase, and the numeric phase as a sequence -- product lists, choice, set-up, launch, plan bookkeeping.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/dbcsr_amd_mm.h"
#include "common.h"
#include "smm_core.h"
#include "mm_types.h"
#include "mm_complex.h"   // z64 and the per-element helpers of the type-generic kernels
#include "mm_jit.h"

#include "mm_workspace.h"
#include "mm_symbolic.h"
#include "mm_numeric_f64.h"
#include "mm_numeric_f64_big.h"
#include "mm_numeric_f64_small.h"
#include "mm_mid.h"   // the one-wave slab kernels of the blocks of 25 ... 40 (mm_numeric_f64_mid.h, mm_mid.hip)
#include "mm_numeric_f32.h"
#include "mm_numeric_z64.h"   // complex_8: one family for every block size
#include "mm_aux.h"
#include "mm_algebra.h"   // add, add_on_diag, trace, dot, norm: the operations between multiplies (brings mm_block_walk.h: Pack16, walk_block)
#include "mm_elementwise.h"  // element-wise operations on two patterns: hadamard product, copy onto a pattern, functions of elements
#include "mm_blocklist.h"  // a coordinate list of blocks: reserve, put and get
#include "mm_multivec.h"  // the matrix times several dense vectors
#include "mm_rank_update.h"  // the rank-k update on the stored pattern
#include "mm_spmm.h"  // the matrix times a dense matrix on the MFMA
#include "mm_block_inverse.h"  // the block diagonal: its copy and the batched inverse of its blocks
#include "mm_block_scale.h"  // a block diagonal applied to a matrix in place
#include "mm_dense.h"  // dense <-> block-sparse: to_dense, from_dense and the count half of create_from_dense
#include "mm_submatrix.h"  // the submatrix method: batched dense principal submatrices out of the matrix and back onto its pattern
#include "mm_csr.h"  // element CSR <-> block-sparse: to_csr (count, emit), from_csr and the blocks of a CSR
#include "mm_reblock.h"  // a matrix under another block structure: the pieces of the source blocks and the gather
#include "mm_tensor.h"  // block-sparse tensors: the permuting move of a list of blocks
// The library comes in two builds (Makefile): the SHIPPING one holds what a multiply can run by itself -- the kernels listed above, their
// symbolic phases, plan reuse -- and the LAB one (-DDBCSR_AMD_EXPERIMENTS, libdbcsr_acc_amd_lab.so) adds every dataflow and variant that
// was built, made parity-green and measured but does not win: the LDS-DMA ring kernels (mm_dma.h), XCD-wide C tiles (mm_tile.*), CU-wide
// C tiles with B shared in LDS (mm_band.*), the persistent form and the ablation / keep-alive variants of the exact-size kernel, the
// G-block bodies and stream spreading of the class kernels, the occupancy and row-group knobs.  Their switches exist in the lab build only.
#ifdef DBCSR_AMD_EXPERIMENTS
#include "mm_lab_api.h"
#include "mm_group.h"
#include "mm_group64.h"
#include "mm_dma.h"
#include "mm_tile_index.h"
#include "mm_band_index.h"
#endif
namespace dbcsr_amd {

#include "mm_engine_state.h"    // plan_compare, struct Engine, helpers
#include "mm_engine_env.h"      // engine_read_env: the environment switches, read once per engine
#include "mm_engine_launch.h"   // kernel tables and launch dispatchers
#include "mm_engine_plan.h"     // plan reuse
#ifdef DBCSR_AMD_EXPERIMENTS
#include "mm_engine_lab.h"      // host side of the experimental dataflows
#endif

// ---- the numeric phase, step by step (numeric_phase below: dbcsr_amd_mm_numeric and dbcsr_amd_mm_numeric_z) ----

// Product lists, C block descriptors and C's index.  Plan reuse: those of the previous multiply stand; C's index is copied from the saved one.
static int build_product_lists(Engine* E, bool reuse, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out,
                               hipStream_t st) {
  const int nbr = E->facts.nbr, W = E->W, nbc = b->nblkcols, nJ = (nbc + 63) / 64;
  const int64_t nblk = E->facts.c_nblks;
  const uint32_t* cin_bm = E->have_cin ? E->cin_bm.p : nullptr;
  const int* cin_pre = E->have_cin ? E->cin_pre.p : nullptr;
  if (reuse) {
    ACC_CHECK(hipMemcpyAsync(c_out->col_i, E->plan_c_col_i.p, sizeof(int32_t) * (size_t)nblk, hipMemcpyDeviceToDevice, st));
    ACC_CHECK(hipMemcpyAsync(c_out->blk_p, E->plan_c_blk_p.p, sizeof(int64_t) * (size_t)nblk, hipMemcpyDeviceToDevice, st));
  } else if (E->rows_kernels) {
    if (E->tmp_i32.ensure((size_t)nblk + 1)) return -1;
    ACC_CHECK(hipMemsetAsync(E->tmp_i32.p, 0, sizeof(int) * (size_t)nblk, st));
    hipLaunchKernelGGL(fill_products_rows, grid_for((int64_t)nbr * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, a->col_blk_size, b->row_p,
                       b->col_i, b->blk_p, E->c_bm.p, E->c_pre.p, c_out->row_p, E->prod_start.p, nbr, W, E->tmp_i32.p, E->entries.p, E->filter);
    hipLaunchKernelGGL(finish_descs_grid, grid_for((int64_t)nbr * nJ * 64), dim3(256), 0, st, c_in->row_p, c_in->blk_p, c_out->row_blk_size,
                       c_out->col_blk_size, cin_bm, cin_pre, E->c_bm.p, E->c_pre.p, c_out->row_p, E->c_blk_p_ws.p, E->prod_start.p,
                       E->prod_cnt.p, nbr, W, nJ, c_out->col_i, c_out->blk_p, E->descs.p);
  } else if (E->grid_kernels) {
    hipLaunchKernelGGL(fill_products_grid, grid_for((int64_t)nbr * nJ * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, b->row_p,
                       b->blk_p, c_in->row_p, c_in->blk_p, a->row_blk_size, a->col_blk_size, b->col_blk_size, E->b_bm.p, E->b_pre.p,
                       cin_bm, cin_pre, E->c_bm.p, E->c_pre.p, c_out->row_p, E->prod_start.p, E->c_blk_p_ws.p, nbr, nbc, W, nJ, c_out->col_i,
                       c_out->blk_p, E->descs.p, E->entries.p, E->filter);
  } else {
    hipLaunchKernelGGL(fill_products, grid_for((int64_t)nbr * W), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p, b->row_p, b->blk_p,
                       c_in->row_p, c_in->blk_p, a->row_blk_size, a->col_blk_size, b->col_blk_size, E->b_bm.p, E->b_pre.p,
                       cin_bm, cin_pre, E->c_bm.p, E->c_pre.p, c_out->row_p, E->prod_start.p, E->c_blk_p_ws.p, nbr, W, c_out->col_i, c_out->blk_p,
                       E->descs.p, E->entries.p);
  }
  return 0;
}

template <typename T>
static NumericArgs<T> numeric_args(Engine* E, hipStream_t st, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, const dbcsr_amd_bcsr* c_in,
                                   const dbcsr_amd_bcsr* c_out, T alpha, T beta, const Work* work, double* norms, bool reuse) {
  return NumericArgs<T>{st, E->descs.p, E->facts.c_nblks, E->entries.p, static_cast<const T*>(a->data), static_cast<const T*>(b->data),
                        static_cast<T*>(c_out->data), static_cast<const T*>(c_in->data), alpha, beta, E->facts.skip_empty, E->order.p, work, norms,
                        a, b, c_out, reuse};
}

// fp64 multiply of mixed sizes: one launch per (m, n) class on its segment of order[].  Which kernel a class gets is decided here, at run time: the slab
// kernel where the choice allows it (c.mid_class_mode), else the run-time compiled exact-size kernel of the class (mm_exact.h, mm_jit.hip), else -- class 9
// (other sizes) and the classes hiprtc could not serve -- the generic LDS kernel.  Writes last_kernel (the launch counts are part of it).
static int launch_classes_f64(Engine* E, const NumericArgs<double>& p, const NumericChoice& c) {
  const SizeFacts& F = E->facts;
  int njit = 0, ngen = 0, nmid = 0, jit_mask = 0, nlaunch = 0;
  const int nside = E->lab.class_streams > 1 ? E->lab.class_streams - 1 : 0;
  if (nside) {
    if (!E->fork_ev) ACC_CHECK(hipEventCreateWithFlags(&E->fork_ev, hipEventDisableTiming));
    ACC_CHECK(hipEventRecord(E->fork_ev, p.st));
    for (int i = 0; i < nside; ++i) {
      if (!E->side_stream[i]) {
        ACC_CHECK(hipStreamCreateWithFlags(&E->side_stream[i], hipStreamNonBlocking));
        ACC_CHECK(hipEventCreateWithFlags(&E->join_ev[i], hipEventDisableTiming));
      }
      ACC_CHECK(hipStreamWaitEvent(E->side_stream[i], E->fork_ev, 0));
    }
  }
  for (int k = 0; k < kNumClasses; ++k) {
    if (E->cls_len[k] == 0) continue;
    NumericArgs<double> q = p.segment(E->cls_off[k]);
    const int slot = nlaunch++ % (nside + 1);
    if (slot) q.st = E->side_stream[slot - 1];
    const unsigned npos = (unsigned)(8 * E->cls_len[k]);
    const int cm = k < 9 ? F.cls_m[k / 3] : 0, cn = k < 9 ? F.cls_n[k % 3] : 0;
    ClassKernel ck;
    if (k < 9 && c.mid_class_mode && mid_f64_serves(cm, cn, c.mid_class_mode)) {
      if (!launch_mid_f64(q, (cm + 3) / 4, (cn + 3) / 4, false, npos, (std::max(cm, cn) + 3) / 4)) return -1;
      ++nmid;
      jit_mask |= 1 << k;   // (the class left its norms, as the run-time compiled kernels do: block_norms_unserved_classes passes it by)
    } else if (k < 9 && cm > 0 && cn > 0 && jit_class_kernel(cm, cn, F.cls_k[0], F.cls_k[1], F.cls_k[2], E->lab.class_g, &ck) == 0) {
      long nblk_l = (long)q.nblk;
      void* args[] = {&q.descs, &nblk_l, &q.entries, &q.a, &q.b, &q.c_out, &q.c_in, &q.alpha, &q.beta, &q.skip_empty, &q.order, &q.work, &q.norms};
      const unsigned cw = E->lab.class_g == 1 ? (unsigned)c.ww : 4u;  // waves per workgroup (the G-block stream body keeps 4)
      ACC_CHECK(hipModuleLaunchKernel(ck.fn, npos / cw / (unsigned)E->lab.class_g, 1, 1, 64 * cw, 1, 1, (unsigned)(cw * ck.wave_lds), q.st, args, nullptr));
      ++njit;
      jit_mask |= 1 << k;
    } else {
      launch_lds_f64(q, c, (unsigned)(8 * E->cls_len[k] / 4) * 4u / (unsigned)c.ww);
      ++ngen;
    }
  }
  for (int i = 0; i < nside; ++i) {
    ACC_CHECK(hipEventRecord(E->join_ev[i], E->side_stream[i]));
    ACC_CHECK(hipStreamWaitEvent(p.st, E->join_ev[i], 0));
  }
  if (p.norms) {  // the blocks the generic kernel handled did not leave their norm
    ClassSet cs;
    for (int r = 0; r < 3; ++r) cs.m[r] = F.cls_m[r], cs.n[r] = F.cls_n[r];
    cs.jit_mask = jit_mask;
    hipLaunchKernelGGL(block_norms_unserved_classes, grid_for(p.nblk * 64), dim3(256), 0, p.st, p.descs, p.nblk, p.c_out, cs, p.norms);
  }
  char slab[24] = "";
  if (nmid > 0) snprintf(slab, sizeof slab, "%d slab + ", nmid);
  snprintf(E->last_kernel, sizeof E->last_kernel, "%s%d jit + %s%d generic launches; m {%d,%d,%d} n {%d,%d,%d} k {%d,%d,%d}]", c.name, njit, slab, ngen,
           F.cls_m[0], F.cls_m[1], F.cls_m[2], F.cls_n[0], F.cls_n[1], F.cls_n[2], F.cls_k[0], F.cls_k[1], F.cls_k[2]);
  return 0;
}

// Launch what the choice says and note it (last_kernel, whose norms norms64[] now holds).  0 = done, < 0 = error.  The choice asked the instance lists
// before it named a family, so a launcher without an instance is an error here, never a fall-through to another family.  (lab: the switches the
// choice was made with; nothing to read in the shipping build.)
static int launch_f64(Engine* E, const NumericChoice& c, const NumericArgs<double>& p, const LabSwitches& lab) {
  const SizeFacts& F = E->facts;
  const int64_t npos = 8 * F.order_len;
  snprintf(E->last_kernel, sizeof E->last_kernel, "%s", c.name);
  if (p.norms && c.leaves_norms) E->norms_data = p.c_out, E->norms_nblks = p.nblk;
  switch (c.family) {
    case Family::f64_tiny:
      if (c.grid > 0) launch_tiny_f64(p, c, F.max_k <= 4);
      return 0;
    case Family::f64_small8:
      if (c.grid > 0) launch_small_f64(p, c, npos);
      return 0;
    case Family::f64_mid:
      return launch_mid_f64(p, c.mid_rb, c.mid_cb, F.min_m != F.max_m || F.min_n != F.max_n, c.grid, (std::max(F.max_m, F.max_n) + 3) / 4) ? 0 : -1;
    case Family::f64_classes: return launch_classes_f64(E, p, c);
    case Family::f64_hot: return launch_hot_f64(p, c, F.hot_m, F.hot_n, F.hot_k, c.flags, c.variant) ? 0 : -1;
    case Family::f64_pipe: launch_pipe_f64(p, c, npos); return 0;
    case Family::f64_lds: launch_lds_f64(p, c, c.grid); return 0;
    case Family::f64_big: return launch_big_f64(p, c, big_tiles(F.max_m), big_tiles(F.max_n)) ? 0 : -1;
    case Family::f64_generic:
      hipLaunchKernelGGL(mm_numeric_f64, dim3(c.grid), dim3(256), 0, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.flags);
      return 0;
#ifdef DBCSR_AMD_EXPERIMENTS
    case Family::f64_group: case Family::f64_tile: case Family::f64_band: case Family::f64_dma: case Family::f64_persistent: return launch_lab_f64(E, c, p, lab);
#endif
    default: return -1;
  }
}

static int launch_f32(Engine* E, const NumericChoice& c, const NumericArgs<float>& p) {
  const SizeFacts& F = E->facts;
  snprintf(E->last_kernel, sizeof E->last_kernel, "%s", c.name);
  switch (c.family) {
    case Family::f32_classes:
      for (int k = 0; k < kNumClasses; ++k)
        if (E->cls_len[k] != 0) launch_lds_f32(p.segment(E->cls_off[k]), c, (unsigned)(8 * E->cls_len[k] / c.ww));
      return 0;
    case Family::f32_direct: return launch_hot_f32_direct(p, c, F.hot_m, F.hot_n, F.hot_k, c.flags, c.slim) ? 0 : -1;
    case Family::f32_hot: return launch_hot_f32(p, c, F.hot_m, F.hot_n, F.hot_k) ? 0 : -1;
    case Family::f32_lds: launch_lds_f32(p, c, c.grid); return 0;
    case Family::f32_generic:
      hipLaunchKernelGGL(mm_numeric_f32, dim3(c.grid), dim3(256), 0, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.flags);
      return 0;
#ifdef DBCSR_AMD_EXPERIMENTS
    case Family::f32_group: {
      const int rc = run_group_f32(E, p, c.group_R);
      // the C blocks of other sizes (tail block row / column): the one-wave-per-block kernel, told to leave the dominant size alone
      if (rc == 0 && F.other_sizes()) launch_hot_f32_direct(p, c, F.hot_m, F.hot_n, F.hot_k, c.flags | 2, false);
      if (rc != 1) return rc;
      LabSwitches lab = E->lab;   // it does not apply after all (B's blocks not in ascending order ...): the choice without it
      lab.f32_group = 0;
      return launch_f32(E, choose_numeric(F, E->sw, lab), p);
    }
#endif
    default: return -1;
  }
}

// complex_8: the one family (mm_numeric_z64.h)
static int launch_z64_family(Engine* E, const NumericChoice& c, const NumericArgs<z64>& p) {
  const SizeFacts& F = E->facts;
  snprintf(E->last_kernel, sizeof E->last_kernel, "%s", c.name);
  if (c.family != Family::z64) return -1;
  return launch_z64(p, c, z64_tiles(F.max_m), z64_tiles(F.max_n), 8 * F.order_len) ? 0 : -1;
}

// The numeric phase for every element type; the scalars are (re, im) pairs whose imaginary parts are zero for real data.
static int numeric_phase(void* handle, libsmm_acc_data_t datatype, const double alpha[2], const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b,
                         const double beta[2], const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out, void* stream);

}  // namespace dbcsr_amd

using namespace dbcsr_amd;

extern "C" {

int dbcsr_amd_mm_create(void** handle) {
  if (!handle) return -1;
  Engine* E = new (std::nothrow) Engine();
  if (!E) return -1;
  hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&E->host_scalars), 16 * sizeof(int64_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    delete E;
    return check(e, "hipHostMalloc", __FILE__, __LINE__);
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&E->cls_host_hist), 3 * 33 * sizeof(int), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&E->cls_host_lens), (2 * kNumClasses + 1) * sizeof(int64_t), hipHostMallocDefault) != hipSuccess)
    return -1;
  if (hipHostMalloc(reinterpret_cast<void**>(&E->plan_host_flag), sizeof(int), hipHostMallocDefault) != hipSuccess) return -1;
  engine_read_env(E);
  for (int i = 0; i < 3; ++i) {
    e = hipEventCreate(&E->ev[i]);
    if (e != hipSuccess) return check(e, "hipEventCreate", __FILE__, __LINE__);
  }
  *handle = E;
  return 0;
}

int dbcsr_amd_mm_timing(void* handle, float* ms_fill, float* ms_numeric) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !E->timed) return -1;
  ACC_CHECK(hipEventSynchronize(E->ev[2]));
  float f = 0.f, n = 0.f;
  ACC_CHECK(hipEventElapsedTime(&f, E->ev[0], E->ev[1]));
  ACC_CHECK(hipEventElapsedTime(&n, E->ev[1], E->ev[2]));
  if (ms_fill) *ms_fill = f;
  if (ms_numeric) *ms_numeric = n;
  return 0;
}

int dbcsr_amd_mm_destroy(void* handle) {
  if (!handle) return 0;
  Engine* E = static_cast<Engine*>(handle);
  if (E->host_scalars) (void)hipHostFree(E->host_scalars);
  if (E->plan_host_flag) (void)hipHostFree(E->plan_host_flag);
  if (E->cls_host_hist) (void)hipHostFree(E->cls_host_hist);
  if (E->cls_host_lens) (void)hipHostFree(E->cls_host_lens);
  for (int i = 0; i < 3; ++i)
    if (E->ev[i]) (void)hipEventDestroy(E->ev[i]);
  for (int i = 0; i < 3; ++i) {
    if (E->side_stream[i]) (void)hipStreamDestroy(E->side_stream[i]);
    if (E->join_ev[i]) (void)hipEventDestroy(E->join_ev[i]);
  }
  if (E->fork_ev) (void)hipEventDestroy(E->fork_ev);
  delete E;   // (the work areas, the lab build's included, free themselves: DevBuf)
  return 0;
}

int dbcsr_amd_mm_symbolic(void* handle, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, const dbcsr_amd_bcsr* c_in,
                          int retain_sparsity, int32_t* c_out_row_p, dbcsr_amd_mm_counts* counts, void* stream) {
  return dbcsr_amd_mm_symbolic_filtered(handle, dbcsr_type_real_8, 1.0, 0.0, a, b, c_in, retain_sparsity, c_out_row_p, counts, stream);
}

int dbcsr_amd_mm_symbolic_filtered(void* handle, libsmm_acc_data_t datatype, double alpha, double filter_eps, const dbcsr_amd_bcsr* a,
                                   const dbcsr_amd_bcsr* b, const dbcsr_amd_bcsr* c_in, int retain_sparsity, int32_t* c_out_row_p,
                                   dbcsr_amd_mm_counts* counts, void* stream) {
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !a || !b || !c_in || !c_out_row_p || !counts) return -1;
  E->drop_pending = 0.0;   // (an announced final filter belongs to ONE numeric phase: a new symbolic phase cancels whatever an abandoned multiply left)
  engine_takes_work_areas(E);
  const bool filtering = filter_eps > 0.0;
  if (filtering && datatype != dbcsr_type_real_8 && datatype != dbcsr_type_real_4 && datatype != dbcsr_type_complex_8) return -10;
  if (a->nblkcols != b->nblkrows || a->nblkrows != c_in->nblkrows || b->nblkcols != c_in->nblkcols) {
    fprintf(stderr, "dbcsr_amd_mm_symbolic: incompatible block dimensions\n");
    return -2;
  }
  hipStream_t st = stream_of(stream);
  const int nbr = a->nblkrows, nbk = a->nblkcols, nbc = b->nblkcols;
  const int W = (nbc + 31) / 32;
  // same index arrays as the previous multiply of this engine: its plan stands (no on-the-fly filter: that one depends on the values)
  if (!filtering) {
    const int hit = plan_matches(E, a, b, c_in, retain_sparsity ? 1 : 0, st);
    if (hit < 0) return -1;
    if (hit) {
      long long off = 0;
      const void* ptr[12];
      long long n[12];
      plan_segments(a, b, c_in, ptr, n);
      for (int i = 0; i < 12; ++i) off += n[i];
      ACC_CHECK(hipMemcpyAsync(c_out_row_p, E->plan_words.p + off, sizeof(int32_t) * ((size_t)nbr + 1), hipMemcpyDeviceToDevice, st));
      *counts = E->plan_counts;
      E->norms_data = nullptr;
      E->filter = FilterArgs{nullptr, nullptr, 0.0f};
      E->valid = true;
      E->plan_hit = true;
      ++E->plan_hits;
      return 0;
    }
  }
  plan_invalidate(E);
  E->valid = false;
  E->facts.nbr = nbr;
  E->facts.nbc = nbc;
  E->W = W;
  E->facts.retain = retain_sparsity != 0;
  E->norms_data = nullptr;  // block norms left by an earlier numeric phase belong to that product only
  E->have_cin = c_in->nblks > 0;
  if (E->b_bm.ensure((size_t)nbk * W + 1) || E->b_pre.ensure((size_t)nbk * W + 1) || E->c_bm.ensure((size_t)nbr * W + 1) ||
      E->c_pre.ensure((size_t)nbr * W + 1) || E->row_nnz.ensure((size_t)nbr + 1) || E->dev_scalars.ensure(16))
    return -1;
  if (E->have_cin && (E->cin_bm.ensure((size_t)nbr * W + 1) || E->cin_pre.ensure((size_t)nbr * W + 1))) return -1;
  ACC_CHECK(hipMemsetAsync(E->dev_scalars.p, 0, 16 * sizeof(unsigned long long), st));
  {  // the "negated min" slots start at the most negative value
    static const int init[6] = {0, -0x7fffffff, 0, -0x7fffffff, 0, -0x7fffffff};
    ACC_CHECK(hipMemcpyAsync(E->dev_scalars.p + 4, init, sizeof(init), hipMemcpyHostToDevice, st));
  }
  if (nbr == 0 || nbc == 0) {
    ACC_CHECK(hipMemsetAsync(c_out_row_p, 0, sizeof(int32_t) * ((size_t)nbr + 1), st));
    ACC_CHECK(hipStreamSynchronize(st));
    counts->c_nblks = counts->c_nze = counts->nproducts = counts->flop = 0;
    E->facts.c_nblks = 0;
    E->facts.nproducts = 0;
    E->grid_kernels = E->rows_kernels = false;
    E->facts.cls_mode = false;
    E->sym_bitmap = -1;
    E->sym_NP = E->sym_PW = E->sym_rowp_chunks = 0;
    E->valid = true;
    return 0;
  }
  // 1. bitmaps of B (and C_in)
  ACC_CHECK(hipMemsetAsync(E->b_bm.p, 0, sizeof(uint32_t) * (size_t)nbk * W, st));
  if (nbk > 0) {
    hipLaunchKernelGGL(bitmap_from_index, grid_for((int64_t)nbk * 64), dim3(256), 0, st, b->row_p, b->col_i, nbk, W, E->b_bm.p);
    hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbk * 64), dim3(256), 0, st, E->b_bm.p, nbk, W, E->b_pre.p, (int*)nullptr);
  }
  if (E->have_cin) {
    ACC_CHECK(hipMemsetAsync(E->cin_bm.p, 0, sizeof(uint32_t) * (size_t)nbr * W, st));
    hipLaunchKernelGGL(bitmap_from_index, grid_for((int64_t)nbr * 64), dim3(256), 0, st, c_in->row_p, c_in->col_i, nbr, W,
                       E->cin_bm.p);
    hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, st, E->cin_bm.p, nbr, W, E->cin_pre.p, (int*)nullptr);
  }
  // on-the-fly filter: block norms of A and alpha*B (fp32 values of fp64 sums)
  E->filter = FilterArgs{nullptr, nullptr, 0.0f};
  if (filtering) {
    if (E->a_norms.ensure((size_t)a->nblks + 1) || E->b_norms.ensure((size_t)b->nblks + 1)) return -1;
    const int sa = row_split(nbr, a->nblks), sb = row_split(nbk, b->nblks);
    if (datatype == dbcsr_type_real_8) {
      hipLaunchKernelGGL((bcsr_block_norms<double>), grid_for((int64_t)nbr * sa * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p,
                         static_cast<const double*>(a->data), a->row_blk_size, a->col_blk_size, nbr, sa, 1.0, E->a_norms.p, (double*)nullptr);
      hipLaunchKernelGGL((bcsr_block_norms<double>), grid_for((int64_t)nbk * sb * 64), dim3(256), 0, st, b->row_p, b->col_i, b->blk_p,
                         static_cast<const double*>(b->data), b->row_blk_size, b->col_blk_size, nbk, sb, alpha, E->b_norms.p, (double*)nullptr);
    } else if (datatype == dbcsr_type_complex_8) {   // (alpha is |alpha| here: the rule uses ||alpha * B||)
      hipLaunchKernelGGL((bcsr_block_norms<z64>), grid_for((int64_t)nbr * sa * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p,
                         static_cast<const z64*>(a->data), a->row_blk_size, a->col_blk_size, nbr, sa, 1.0, E->a_norms.p, (double*)nullptr);
      hipLaunchKernelGGL((bcsr_block_norms<z64>), grid_for((int64_t)nbk * sb * 64), dim3(256), 0, st, b->row_p, b->col_i, b->blk_p,
                         static_cast<const z64*>(b->data), b->row_blk_size, b->col_blk_size, nbk, sb, alpha, E->b_norms.p, (double*)nullptr);
    } else {
      hipLaunchKernelGGL((bcsr_block_norms<float>), grid_for((int64_t)nbr * sa * 64), dim3(256), 0, st, a->row_p, a->col_i, a->blk_p,
                         static_cast<const float*>(a->data), a->row_blk_size, a->col_blk_size, nbr, sa, 1.0, E->a_norms.p, (double*)nullptr);
      hipLaunchKernelGGL((bcsr_block_norms<float>), grid_for((int64_t)nbk * sb * 64), dim3(256), 0, st, b->row_p, b->col_i, b->blk_p,
                         static_cast<const float*>(b->data), b->row_blk_size, b->col_blk_size, nbk, sb, alpha, E->b_norms.p, (double*)nullptr);
    }
    E->filter = FilterArgs{E->a_norms.p, E->b_norms.p, (float)filter_eps};
  }
  // 2. pattern of C_out, its row prefix and row pointer
  // expected number of products against the number of (row, column) candidates: product-driven kernels for a sparse product
  SymbolicSizes sizes;
  sizes.nbr = nbr, sizes.nbk = nbk, sizes.nbc = nbc, sizes.a_nblks = a->nblks, sizes.b_nblks = b->nblks;
  sizes.filtering = filtering, sizes.retain = retain_sparsity != 0, sizes.forced = E->force_symbolic;
  SymbolicChoice sym = choose_symbolic_pattern(sizes);   // (mm_choose.h)
  if (sym.bitmap_rows) {
    if (E->have_cin)
      ACC_CHECK(hipMemcpyAsync(E->c_bm.p, E->cin_bm.p, sizeof(uint32_t) * (size_t)nbr * W, hipMemcpyDeviceToDevice, st));
    else
      ACC_CHECK(hipMemsetAsync(E->c_bm.p, 0, sizeof(uint32_t) * (size_t)nbr * W, st));
    hipLaunchKernelGGL(c_bitmap_rows_filtered, grid_for((int64_t)nbr * 64), dim3(256), 0, st, a->row_p, a->col_i, b->row_p, b->col_i, nbr, W,
                       E->facts.canonical_c, E->filter, E->c_bm.p);
  } else if (filtering)
    hipLaunchKernelGGL(c_bitmap_filtered, grid_for((int64_t)nbr * ((nbc + 63) / 64) * 64), dim3(256), 0, st, a->row_p, a->col_i, b->row_p,
                       E->b_bm.p, E->b_pre.p, E->have_cin ? E->cin_bm.p : (const uint32_t*)nullptr, nbr, nbc, W, (nbc + 63) / 64,
                       retain_sparsity ? 1 : 0, E->facts.canonical_c, E->filter, E->c_bm.p);
  else
    hipLaunchKernelGGL(c_bitmap, grid_for((int64_t)nbr * W), dim3(256), 0, st, a->row_p, a->col_i, E->b_bm.p,
                       E->have_cin ? E->cin_bm.p : (const uint32_t*)nullptr, nbr, W, retain_sparsity ? 1 : 0, E->facts.canonical_c, E->c_bm.p);
  hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, st, E->c_bm.p, nbr, W, E->c_pre.p, E->row_nnz.p);
  int64_t* dsc = reinterpret_cast<int64_t*>(E->dev_scalars.p);
  if (exclusive_scan<int32_t>(E, E->row_nnz.p, nbr, c_out_row_p, dsc + 0, true, st)) return -1;
  // block-size maxima (LDS slice size / kernel choice of the numeric phase), the most frequent block size per dimension (choice of an exact-size kernel), the most
  // frequent size in units of 4 of C's rows and columns (the slab kernels' exact launch when no size dominates) and the histograms of the sizes 1 ... 32 (the
  // (m, n) classes of a mixed-size multiply): one launch (block_size_stats)
  if (E->sw.use_classes > 0 && E->cls_hist.ensure(3 * 33)) return -1;
  hipLaunchKernelGGL(block_size_stats, dim3(3), dim3(256), 0, st, a->row_blk_size, nbr, a->col_blk_size, nbk, b->col_blk_size, nbc,
                     reinterpret_cast<int*>(E->dev_scalars.p + 4), reinterpret_cast<int*>(E->dev_scalars.p + 8), reinterpret_cast<int*>(E->dev_scalars.p + 11),
                     E->sw.use_classes > 0 ? E->cls_hist.p : (int*)nullptr);
  if (E->sw.use_classes > 0) ACC_CHECK(hipMemcpyAsync(E->cls_host_hist, E->cls_hist.p, 3 * 33 * sizeof(int), hipMemcpyDeviceToHost, st));
  // need c_nblks (and the block-size extrema) on the host to size per-block work arrays
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, dsc, 13 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  const int64_t c_nblks = E->host_scalars[0];
  {
    const int* mx = reinterpret_cast<const int*>(E->host_scalars + 4);
    E->facts.max_m = mx[0]; E->facts.min_m = -mx[1];
    E->facts.max_k = mx[2]; E->facts.min_k = -mx[3];
    E->facts.max_n = mx[4]; E->facts.min_n = -mx[5];
    if (E->facts.max_k > 0xffff || E->facts.max_m > 0x7fff || E->facts.max_n > 0x7fff) {
      fprintf(stderr, "dbcsr_amd_mm_symbolic: block sizes above 32767 (m, n) / 65535 (k) are not supported (packed 16-bit extents)\n");
      return -1;
    }
    // exact-size kernel: only when one (m, n, k) covers at least 90 % of the block rows / columns of each dimension
    const int* md = reinterpret_cast<const int*>(E->host_scalars + 8);
    const bool dominant = 10ll * md[1] >= 9ll * nbr && 10ll * md[3] >= 9ll * nbk && 10ll * md[5] >= 9ll * nbc;
    E->facts.hot_m = dominant ? md[0] : 0;
    E->facts.hot_k = dominant ? md[2] : 0;
    E->facts.hot_n = dominant ? md[4] : 0;
    E->facts.hot_cnt_m = md[1], E->facts.hot_cnt_k = md[3], E->facts.hot_cnt_n = md[5];
    const int* um = reinterpret_cast<const int*>(E->host_scalars + 11);
    E->facts.units_m = um[0], E->facts.units_cnt_m = um[1], E->facts.units_n = um[2], E->facts.units_cnt_n = um[3];
  }
  // (m, n) classes of a mixed-size multiply (mm_choose.h): is this one, and its three most frequent sizes per dimension
  E->facts.c_nblks = c_nblks;
  choose_classes(&E->facts, E->sw, E->cls_host_hist);
  // processing order of the numeric phase: column panels sized for the Infinity Cache, rows dealt to XCDs
  // size of B from the mean block sizes when the histograms are at hand (mixed sizes: the maxima overestimate it 2x on
  // BASELINE config 3, which doubled the number of panels and with it the compulsory re-reads of the A block-rows)
  double mean_k = E->facts.max_k, mean_n = E->facts.max_n;
  if (E->sw.use_classes > 0 && E->facts.max_k <= 32 && E->facts.max_n <= 32 && E->facts.min_k >= 1 && E->facts.min_n >= 1) {
    double sk = 0, ck = 0, sn = 0, cn = 0;
    for (int sz = 1; sz <= 32; ++sz) {
      sn += (double)sz * E->cls_host_hist[33 + sz];
      cn += E->cls_host_hist[33 + sz];
      sk += (double)sz * E->cls_host_hist[66 + sz];
      ck += E->cls_host_hist[66 + sz];
    }
    if (ck > 0 && cn > 0) mean_k = sk / ck, mean_n = sn / cn;
  }
  const int64_t b_bytes_est = (int64_t)((double)b->nblks * mean_k * mean_n * (double)sizeof(double));
  int NP = 1, PW = W;
  choose_panels(W, b_bytes_est, E->panel_bytes, &NP, &PW);
  const int R = (nbr + 7) / 8;
  // rows walked together per XCD.  Measured on config 2 (DBCSR_AMD_MM_ROW_GROUP = 1/2/4/6/8: 22.7/22.8/23.5/25.2/26.3 ms):
  // the B reuse it buys (10 % fill: 14 % fewer B fetches at 4 rows) does not pay for the extra A rows in L2 -> default 1.
  int RG = E->lab.row_group > 0 ? E->lab.row_group : 1;
  RG = std::max(1, std::min(RG, R));
  const int NG = (R + RG - 1) / RG;
  const int nkeys = (E->facts.cls_mode ? kNumClasses : 1) * 8 * NP * (E->facts.cls_mode ? R : NG);
  if (E->order_cnt.ensure((size_t)nkeys + 1) || E->order_base.ensure((size_t)nkeys + 1)) return -1;
  if (E->facts.cls_mode) {
    if (E->cls_row.ensure((size_t)nbr + 1) || E->cls_col.ensure((size_t)nbc + 1) || E->cls_col_bm.ensure((size_t)4 * W + 1) ||
        E->cls_lens.ensure(2 * kNumClasses + 1) || E->cls_vpos.ensure((size_t)nbr + 1) || E->cls_vrow.ensure((size_t)nbr + 1))
      return -1;
    hipLaunchKernelGGL(class_ids, grid_for(nbr), dim3(256), 0, st, a->row_blk_size, nbr, E->facts.cls_m[0], E->facts.cls_m[1], E->facts.cls_m[2], E->cls_row.p);
    hipLaunchKernelGGL(class_ids, grid_for(nbc), dim3(256), 0, st, b->col_blk_size, nbc, E->facts.cls_n[0], E->facts.cls_n[1], E->facts.cls_n[2], E->cls_col.p);
    hipLaunchKernelGGL(class_col_bitmaps, grid_for(W), dim3(256), 0, st, E->cls_col.p, nbc, W, E->cls_col_bm.p);
    hipLaunchKernelGGL(class_row_deal, dim3(1), dim3(256), 0, st, E->cls_row.p, nbr, E->cls_vpos.p, E->cls_vrow.p);
    hipLaunchKernelGGL(order_count_cls, grid_for(nkeys), dim3(256), 0, st, E->c_bm.p, E->cls_row.p, E->cls_col_bm.p, E->cls_vrow.p, nbr, W, PW, NP, R,
                       E->order_cnt.p);
    if (exclusive_scan<int64_t>(E, E->order_cnt.p, nkeys, E->order_base.p, nullptr, false, st)) return -1;
    hipLaunchKernelGGL(order_len_cls, dim3(1), dim3(1), 0, st, E->order_base.p, c_nblks, NP, R, E->cls_lens.p);
    ACC_CHECK(hipMemcpyAsync(E->cls_host_lens, E->cls_lens.p, (2 * kNumClasses + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  } else {
  hipLaunchKernelGGL(order_count, grid_for(nkeys), dim3(256), 0, st, E->c_pre.p, E->row_nnz.p, nbr, W, PW, NP, NG, RG, E->order_cnt.p);
  if (exclusive_scan<int64_t>(E, E->order_cnt.p, nkeys, E->order_base.p, nullptr, false, st)) return -1;
  hipLaunchKernelGGL(order_len, dim3(1), dim3(1), 0, st, E->order_base.p, c_nblks, NP, NG, dsc + 7);
  }
  if (E->prod_cnt.ensure((size_t)c_nblks + 1) || E->blk_nze.ensure((size_t)c_nblks + 1) || E->prod_start.ensure((size_t)c_nblks + 1) ||
      E->c_blk_p_ws.ensure((size_t)c_nblks + 1))
    return -1;
  // 3. per C block: number of products, size; flop
  // one lane per (row, column) candidate unless C is extremely sparse (then one thread per bitmap word); a sparse C with enough block rows to fill the
  // chip: product-driven kernels (choose_symbolic_count, mm_choose.h)
  const int nJ = (nbc + 63) / 64;
  sym = choose_symbolic_count(sizes, sym, c_nblks);
  E->grid_kernels = sym.grid_kernels;
  E->rows_kernels = sym.rows_kernels;
  E->sym_bitmap = sym.bitmap_rows ? 2 : (filtering ? 1 : 0);
  E->sym_NP = NP, E->sym_PW = PW;
  E->sym_rowp_chunks = (int)(((int64_t)nbr + kScanChunk - 1) / kScanChunk);
  if (E->rows_kernels) {
    ACC_CHECK(hipMemsetAsync(E->prod_cnt.p, 0, sizeof(int) * (size_t)c_nblks, st));
    hipLaunchKernelGGL(block_sizes_rows, grid_for((int64_t)nbr * W), dim3(256), 0, st, E->c_bm.p, E->c_pre.p, c_out_row_p, a->row_blk_size,
                       b->col_blk_size, nbr, W, E->blk_nze.p);
    hipLaunchKernelGGL(count_products_rows, grid_for((int64_t)nbr * 64), dim3(256), 0, st, a->row_p, a->col_i, a->row_blk_size, a->col_blk_size,
                       b->col_blk_size, b->row_p, b->col_i, E->c_bm.p, E->c_pre.p, c_out_row_p, nbr, W, E->prod_cnt.p, E->dev_scalars.p + 3,
                       E->filter);
  } else if (E->grid_kernels)
    hipLaunchKernelGGL(count_products_grid, grid_for((int64_t)nbr * nJ * 64), dim3(256), 0, st, a->row_p, a->col_i, a->row_blk_size,
                       a->col_blk_size, b->col_blk_size, E->b_bm.p, E->c_bm.p, E->c_pre.p, c_out_row_p, nbr, nbc, W, nJ,
                       E->prod_cnt.p, E->blk_nze.p, E->dev_scalars.p + 3, b->row_p, E->b_pre.p, E->filter);
  else
    hipLaunchKernelGGL(count_products, grid_for((int64_t)nbr * W), dim3(256), 0, st, a->row_p, a->col_i, a->row_blk_size,
                       a->col_blk_size, b->col_blk_size, E->b_bm.p, E->c_bm.p, E->c_pre.p, c_out_row_p, nbr, W, E->prod_cnt.p,
                       E->blk_nze.p, E->dev_scalars.p + 3);
  if (exclusive_scan<int64_t>(E, E->prod_cnt.p, c_nblks, E->prod_start.p, dsc + 2, false, st)) return -1;
  if (exclusive_scan<int64_t>(E, E->blk_nze.p, c_nblks, E->c_blk_p_ws.p, dsc + 1, false, st)) return -1;
  ACC_CHECK(hipMemcpyAsync(E->host_scalars, dsc, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  E->facts.order_len = E->host_scalars[7];
  if (E->facts.cls_mode) {
    for (int c = 0; c < kNumClasses; ++c) {
      E->cls_len[c] = E->cls_host_lens[c];
      E->cls_off[c] = E->cls_host_lens[kNumClasses + c];
    }
    const int64_t total = E->cls_host_lens[2 * kNumClasses];
    E->facts.order_len = total / 8;  // (only its product with 8 is used below: the size of order[])
    if (E->order.ensure((size_t)total + 64)) return -1;
    if (total > 0) {
      ACC_CHECK(hipMemsetAsync(E->order.p, 0xff, sizeof(int) * ((size_t)total + 64), st));
      hipLaunchKernelGGL(order_fill_cls, grid_for((int64_t)nbr * W), dim3(256), 0, st, E->c_bm.p, E->c_pre.p, c_out_row_p, E->cls_row.p,
                         E->cls_col_bm.p, E->order_base.p, E->cls_lens.p, E->cls_vpos.p, nbr, W, PW, NP, R, E->order.p);
    }
  } else {
  if (E->order.ensure((size_t)(8 * E->facts.order_len) + 64)) return -1;
  if (E->facts.order_len > 0) {
    ACC_CHECK(hipMemsetAsync(E->order.p, 0xff, sizeof(int) * ((size_t)(8 * E->facts.order_len) + 64), st));  // padding included
    hipLaunchKernelGGL(order_fill, grid_for((int64_t)nbr * W), dim3(256), 0, st, E->c_bm.p, E->c_pre.p, E->row_nnz.p, c_out_row_p,
                       E->order_base.p, nbr, W, PW, NP, NG, RG, E->facts.order_len, E->order.p);
  }
  }
  counts->c_nblks = E->host_scalars[0];
  counts->c_nze = E->host_scalars[1];
  counts->nproducts = E->host_scalars[2];
  counts->flop = E->host_scalars[3];
  E->facts.c_nblks = counts->c_nblks;
  E->facts.nproducts = counts->nproducts;
  E->valid = true;
  ++E->plan_misses;
  if (!filtering) {
    if (plan_save(E, a, b, c_in, retain_sparsity ? 1 : 0, c_out_row_p, *counts, st)) return -1;
  } else {
    plan_invalidate(E);
  }
  return check(hipGetLastError(), "dbcsr_amd_mm_symbolic", __FILE__, __LINE__);
}

int dbcsr_amd_mm_numeric(void* handle, libsmm_acc_data_t datatype, double alpha, const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b,
                         double beta, const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out, void* stream) {
  const double al[2] = {alpha, 0.0}, be[2] = {beta, 0.0};   // (complex_8: the scalars mean x + 0i)
  return numeric_phase(handle, datatype, al, a, b, be, c_in, c_out, stream);
}

int dbcsr_amd_mm_numeric_z(void* handle, const double alpha[2], const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b, const double beta[2],
                           const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out, void* stream) {
  if (!alpha || !beta) return -1;
  return numeric_phase(handle, dbcsr_type_complex_8, alpha, a, b, beta, c_in, c_out, stream);
}

#include "mm_engine_ops.h"   // init_c, crop, filter, checksum, fill, transpose, twin moves, statistics
#include "mm_engine_algebra.h"   // add, add_on_diag, trace, dot, norm
#include "mm_engine_elementwise.h"   // hadamard product, copy onto a pattern, functions of elements
#include "mm_engine_blocklist.h"   // reserve, put and get blocks through a coordinate list
#include "mm_engine_csr.h"   // the element CSR form: to_csr (count / apply), from_csr, the blocks of a CSR
#include "mm_engine_reblock.h"   // re-blocking: the pieces of the source blocks, the gather
#include "mm_engine_tensor.h"   // block-sparse tensors: the permuting move of a list of blocks

}  // extern "C"

namespace dbcsr_amd {

static int numeric_phase(void* handle, libsmm_acc_data_t datatype, const double alpha_z[2], const dbcsr_amd_bcsr* a, const dbcsr_amd_bcsr* b,
                         const double beta_z[2], const dbcsr_amd_bcsr* c_in, dbcsr_amd_bcsr* c_out, void* stream) {
  const double alpha = alpha_z[0], beta = beta_z[0];
  Engine* E = static_cast<Engine*>(handle);
  if (!E || !E->valid || !a || !b || !c_in || !c_out) {
    fprintf(stderr, "dbcsr_amd_mm_numeric: no valid symbolic phase for this handle\n");
    return -1;
  }
  if (datatype != dbcsr_type_real_8 && datatype != dbcsr_type_real_4 && datatype != dbcsr_type_complex_8) return -10;
  hipStream_t st = stream_of(stream);
  SizeFacts& F = E->facts;
  const int64_t nblk = F.c_nblks;
  if (nblk == 0) return 0;
  // 1. product lists (plan reuse: product lists, descriptors and launch order of the previous multiply stand)
  const bool reuse = E->plan_hit && E->plan_numeric;
  if (!reuse) {
    E->work_built = false;
#ifdef DBCSR_AMD_EXPERIMENTS
    E->ls.forget_plan();
#endif
  }
  if (E->entries.ensure((size_t)F.nproducts + 1) || E->descs.ensure((size_t)nblk + 1)) return -1;
  ACC_CHECK(hipEventRecord(E->ev[0], st));
  if (int rc = build_product_lists(E, reuse, a, b, c_in, c_out, st)) return rc;
  // 2. the choice (mm_choose.h), from the symbolic phase's facts and those of this call
  F.nbc = b->nblkcols;
  F.fp64 = datatype == dbcsr_type_real_8;
  F.cplx = datatype == dbcsr_type_complex_8;
  F.filter_active = E->filter.a_norms != nullptr;
  // in-place accumulation (Cannon ticks after the first): C blocks without products in this call are left untouched
  F.skip_empty = (c_out->data == c_in->data && F.retain && beta == 1.0 && beta_z[1] == 0.0) ? 1 : 0;
  const NumericChoice ch = choose_numeric(F, E->sw, E->lab);
  // 3. what the choice wants set up: launch-order work records (descriptor + first product in one read) ...
  const Work* work = nullptr;
  if (ch.work) {
    const int64_t npos = 8 * F.order_len;
    if (!(reuse && E->work_built)) {
      if (E->work.ensure((size_t)npos + 1)) return -1;
      hipLaunchKernelGGL(build_work, grid_for(npos), dim3(256), 0, st, E->order.p, npos, E->descs.p, nblk, E->entries.p, E->work.p);
      E->work_built = true;
    }
    work = E->work.p;
  }
  // ... and the norms a filtered multiply's kernels leave behind (dbcsr_amd_bcsr_filter_count then skips its pass over C).  The final block filter
  // announced for this numeric phase (dbcsr_amd_mm_expect_filter): its eps^2 rides behind the norms, norms64[nblk], where the exact-size and class
  // kernels pick it up -- a block below it is not written
  double* norms = nullptr;
  E->norms_data = nullptr;
  if (ch.norms) {
    if (E->norms64.ensure((size_t)nblk + 1)) return -1;
    norms = E->norms64.p;
  }
  const double drop = norms ? E->drop_pending : 0.0;
  E->drop_pending = 0.0;
  E->unwritten_below = 0.0;
  if (norms) {
    hipLaunchKernelGGL(store_scalar_f64, dim3(1), dim3(1), 0, st, norms + nblk, drop);
    E->unwritten_below = drop;
  }
  ACC_CHECK(hipEventRecord(E->ev[1], st));
  // 4. the launch
  if ((F.cplx ? launch_z64_family(E, ch, numeric_args<z64>(E, st, a, b, c_in, c_out, z64(alpha, alpha_z[1]), z64(beta, beta_z[1]), work, norms, reuse))
       : F.fp64 ? launch_f64(E, ch, numeric_args<double>(E, st, a, b, c_in, c_out, alpha, beta, work, norms, reuse), E->lab)
                : launch_f32(E, ch, numeric_args<float>(E, st, a, b, c_in, c_out, (float)alpha, (float)beta, work, norms, reuse))) != 0) {
    fprintf(stderr, "dbcsr_amd_mm_numeric: launching %s failed\n", E->last_kernel);
    return -1;
  }
  ACC_CHECK(hipEventRecord(E->ev[2], st));
  // 5. plan bookkeeping
  E->timed = true;
  c_out->nblks = nblk;
  if (E->plan_saved && !E->plan_numeric) {  // first numeric phase of a saved plan: keep C's index for the multiplies that reuse it
    if (E->plan_c_col_i.ensure((size_t)nblk + 1) || E->plan_c_blk_p.ensure((size_t)nblk + 1)) return -1;
    ACC_CHECK(hipMemcpyAsync(E->plan_c_col_i.p, c_out->col_i, sizeof(int32_t) * (size_t)nblk, hipMemcpyDeviceToDevice, st));
    ACC_CHECK(hipMemcpyAsync(E->plan_c_blk_p.p, c_out->blk_p, sizeof(int64_t) * (size_t)nblk, hipMemcpyDeviceToDevice, st));
    E->plan_numeric = true;
  }
  return check(hipGetLastError(), "dbcsr_amd_mm_numeric", __FILE__, __LINE__);
}

}  // namespace dbcsr_amd
