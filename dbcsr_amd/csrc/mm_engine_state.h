// mm_engine_state.h -- part of mm_engine.hip (included inside namespace dbcsr_amd): the plan-comparison kernel, struct Engine (buffers, the SizeFacts carried
// from the symbolic to the numeric phase, Switches / LabSwitches, the saved plan, the lab build's LabState) and the small host helpers everything else uses.
#ifndef DBCSR_AMD_MM_ENGINE_STATE_H
#define DBCSR_AMD_MM_ENGINE_STATE_H

// ---- plan reuse ------------------------------------------------------------------------------------------------------
// A multiply whose operands have the SAME index arrays (patterns, block sizes, block offsets) as the previous multiply of the
// engine -- every SCF step of a CP2K run, every repetition of the performance driver -- needs no new symbolic phase: the engine
// keeps device copies of the last call's index arrays and compares the incoming ones word by word (one small kernel, one flag).
struct PlanSegs {
  const int32_t* a[12];
  const int32_t* b[12];
  long long n[12];  // 32-bit words per segment
  int nseg;
};
__global__ void __launch_bounds__(256) plan_compare(PlanSegs S, int* __restrict__ differs) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  bool bad = false;
  for (int g = 0; g < S.nseg; ++g)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S.n[g]; i += stride) bad |= S.a[g][i] != S.b[g][i];
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(differs, 1);
}

#ifdef DBCSR_AMD_EXPERIMENTS
// Everything only the lab build's dataflows touch (mm_engine_lab.h, the lab families of dbcsr_amd_mm_numeric, the statistics calls): buffers, flags, knobs.
// (Its buffers, like all of the engine's, free themselves when dbcsr_amd_mm_destroy deletes the engine: DevBuf, mm_workspace.h.)
struct LabState {
  // group kernels (mm_group.h, mm_group64.h)
  int group_R = 0;
  bool group_built = false, b_monotone = false;
  int64_t group_panel_bytes = 0;   // DBCSR_AMD_MM_GROUP_PANEL_MB: target size of a B column panel of the group launch (unset: panel_bytes; at least 1 MB)
  DevBuf<int> groups, group_flag, group_cnt;
  DevBuf<GWork> group_work;
  DevBuf<GEntry> group_entries;
  DevBuf<int64_t> group_start;
  // XCD-wide C tiles in registers (mm_tile.h): DBCSR_AMD_MM_TILE_WINDOW = k window of the team (inner blocks; 0: no throttle);
  // DBCSR_AMD_MM_TILE_RDV = 1: unpaired fragment reads
  int tile_shape = 0;  // DBCSR_AMD_MM_TILE_SHAPE: 0 = 3 x 3 C blocks per wave, two waves per SIMD; 1 = 4 x 3, one wave per SIMD, four-slot ring (mm_tile.h)
  int tile_window = 256, tile_rdv = 0, tile_pub = 1, tile_prefetch = 0, tile_knobs = 0;  // DBCSR_AMD_MM_TILE_PUB: progress stores written through (0) / left in L2 (1)
  bool tile_built = false, band_built = false;
  DevBuf<uint32_t> a_bm, bt_bm, tile_prog;
  DevBuf<unsigned long long> tile_times;
  DevBuf<int> a_pre, tile_rows, tile_cols, tile_cnt, tile_flags;
  DevBuf<int64_t> tile_start;
  DevBuf<TileDesc> tdescs;
  DevBuf<TileEntry> tentries;
  TileGeom tile_geom = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // CU-wide C tiles, B shared in an LDS ring (mm_band.h): DBCSR_AMD_MM_BAND_DEPTH = slots of the ring (12 | 16 | 20 | 22);
  // DBCSR_AMD_MM_BAND_BPOL = 1: B copies with the nt hint; DBCSR_AMD_MM_BAND_KNOBS bit 0: where the waves' time goes (printed by dbcsr_amd_mm_band_stats)
  // DBCSR_AMD_MM_BAND_WINDOW = k window of an XCD's waves (inner blocks; 0: no throttle)
  // DBCSR_AMD_MM_BAND_SHAPE: 0 = 8 waves x (3 x 3 C blocks), 1 = 16 waves x (2 x 2)
  int band_shape = 1, band_depth = 20, band_bpol = 0, band_knobs = 0, band_window = 384;
  int64_t band_nlist = 0, band_nrem = 0;
  DevBuf<unsigned> band_prog;
  BandGeom band_geom = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  DevBuf<BandDesc> band_descs_buf;
  DevBuf<BandEntry> band_entries;
  DevBuf<BandRem> band_rem;
  DevBuf<int> band_cnt_list, band_cnt_b, band_cnt_rem, band_sub_cnt, band_flags;
  DevBuf<int64_t> band_list_off, band_seq_off, band_rem_start;
  DevBuf<unsigned long long> band_times;
  // the persistent form of the 23^3 kernel
  unsigned hot_xcd_mask = 0xffu;  // DBCSR_AMD_MM_HOT_XCDS: XCDs the persistent form runs on (experiments: the others' C blocks are NOT computed)
  DevBuf<unsigned> hot_counters;

  // norms and vectors: DBCSR_AMD_ALG_COLSUMS = 1 ... 4, the ablations of algebra_col_sums and its lane-per-column form (mm_algebra.h)
  int alg_col_variant = 0;
  // matrix times several vectors: DBCSR_AMD_MULTIVEC_WAVES = 1 ... 4, the waves (tiles of 16 right-hand sides) of a workgroup that share a staged
  // block; 1: independent waves, every tile loads the block itself (mm_multivec.h; profiles/matrix_multivec.txt)
  int multivec_waves = 0;

  void forget_plan() { tile_built = band_built = group_built = false; }
};
#endif

struct Engine {
  // ---- work areas ----
  DevBuf<uint32_t> b_bm, c_bm, cin_bm;
  DevBuf<int> b_pre, c_pre, cin_pre, row_nnz, prod_cnt, blk_nze, tmp_i32;
  DevBuf<int64_t> prod_start, c_blk_p_ws, partial, off_a, off_b;
  DevBuf<Entry> entries;
  DevBuf<Desc> descs;
  DevBuf<double> row_sums, norms64;
  DevBuf<float> a_norms, b_norms;
  DevBuf<int> keep;
  DevBuf<int> order, order_cnt;
  DevBuf<int64_t> order_base;
  DevBuf<Work> work;  // launch-order records of the exact-size fp64 kernels (DBCSR_AMD_MM_WORK=0: the class kernels read order[] -> descs[] -> entries[] instead)
  DevBuf<unsigned long long> dev_scalars, stat_table;
  int64_t* host_scalars = nullptr;  // pinned: [0]=c_nblks [1]=c_nze [2]=nproducts [3]=flop
  DevBuf<int> cls_hist;
  DevBuf<unsigned char> cls_row, cls_col;
  DevBuf<int> cls_vpos, cls_vrow;   // class mode: the rows numbered again class after class (class_row_deal, mm_symbolic.h) and the inverse
  DevBuf<uint32_t> cls_col_bm;
  DevBuf<int64_t> cls_lens;
  int* cls_host_hist = nullptr;       // pinned: 3 x 33 size histograms
  int64_t* cls_host_lens = nullptr;   // pinned: 10 lengths, 10 offsets, total
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // around fill_products and the numeric kernel
  // class launches spread over streams (lab: DBCSR_AMD_MM_CLASS_STREAMS)
  hipStream_t side_stream[3] = {nullptr, nullptr, nullptr};
  hipEvent_t fork_ev = nullptr, join_ev[3] = {nullptr, nullptr, nullptr};

  // ---- state carried from symbolic to numeric ----
  SizeFacts facts;      // block sizes, counts, the (m, n) classes: what the numeric phase's choice reads (mm_choose.h)
  int W = 0;
  bool have_cin = false, valid = false;
  bool rows_kernels = false;  // product-driven symbolic kernels (sparse C); DBCSR_AMD_MM_SYMBOLIC=rows forces, =grid / =word exclude
  bool grid_kernels = false;
  // what the symbolic phase chose (mm_choose.h: choose_symbolic_pattern / _count, choose_panels), for dbcsr_amd_mm_last_symbolic: the pattern kernel
  // (-1 none: no block row or column, 0 c_bitmap, 1 c_bitmap_filtered, 2 c_bitmap_rows_filtered), the column panels, the chunks of the scan that made row_p
  int sym_bitmap = -1, sym_NP = 0, sym_PW = 0, sym_rowp_chunks = 0;
  char last_symbolic[160] = "";
  int64_t cls_len[kNumClasses] = {0}, cls_off[kNumClasses] = {0};
  FilterArgs filter = {nullptr, nullptr, 0.0f};
  double drop_pending = 0.0;       // dbcsr_amd_mm_expect_filter: eps^2 of the final block filter announced for the next numeric phase (0: none)
  bool work_built = false;

  // ---- what the last numeric phase / the operations after it left ----
  const void* norms_data = nullptr;  // norms64[] holds the block norms of the matrix with this data pointer (left by the numeric kernel)
  int64_t norms_nblks = 0;
  double unwritten_below = 0.0;    // the C of the last numeric phase lacks the blocks with ||blk||^2 below this (their norms are in norms64)
  char last_kernel[96] = "";  // name of the numeric kernel of the last dbcsr_amd_mm_numeric (dbcsr_amd_mm_last_kernel)
  bool timed = false;
  int64_t flt_nblks = 0;
  int64_t flt_new_nblks = -1;  // blocks the last dbcsr_amd_bcsr_filter_count kept (-1: no count since the handle was made / since a crop count)
  int filter_in_place = 0;     // dbcsr_amd_mm_set_filter_in_place: dbcsr_amd_multiply's final filter rewrites C's index only
  Window crop_win = {0, 0, 0, 0};       // window of the last dbcsr_amd_bcsr_crop_count
  bool crop_pending = false;
  bool flt_pending = false;    // a dbcsr_amd_bcsr_filter_count succeeded and nothing has taken the work areas since: keep / prod_start / c_blk_p_ws are a filter's
  // the last dbcsr_amd_bcsr_twin_count that succeeded and still owns c_bm / c_pre / c_blk_p_ws: its mode (-1: none pending) and its matrix
  int twin_mode = -1, twin_nblkrows = 0;
  int64_t twin_nblks = 0;
  KPassMemo kpass_memo;  // dbcsr_amd_multiply's k-pass decision for the last stamped A operand (mm_api.hip)

  // ---- matrix algebra (mm_engine_algebra.h): buffers of its own, nothing a saved plan depends on.  Only the general (union) add borrows the symbolic
  // work areas, and invalidates the plan ----
  DevBuf<double> alg_sums;    // reductions: one pair of doubles per wave, the result behind them; norms and vectors: S partial vectors of n doubles / one maximum per wave
  DevBuf<int> alg_i32;        // [0] flags of algebra_compare; diag: need[nbr], blk_nze[nbr]
  DevBuf<int64_t> alg_i64;    // [0 ... 7] scalars; diag: offsets of the missing diagonal blocks; norms and vectors: element offsets of block rows / columns
  // norms and vectors: the per-column block lists (a transposed index: bitmap, prefix, counts, column pointers, (block, row) pairs) and Gershgorin's vectors
  DevBuf<uint32_t> alg_bm;
  DevBuf<int> alg_pre, alg_cnt, alg_col_p, alg_list;
  DevBuf<double> alg_vec;     // Gershgorin: row sums [n], column sums [n], the result
  // dbcsr_amd_bcsr_gershgorin sizes its vectors by the full row count, which only the device knows: the counts of the last few sets of block sizes it saw
  // (same size arrays, same non-zero index_stamp), so that an iteration over a few matrices fetches each count once
  struct AlgLen {
    const void* rs = nullptr;
    const void* cs = nullptr;
    uint64_t stamp = 0;
    int nbr = 0, nbc = 0;
    int64_t rows = 0;
    int64_t cols = -1;   // the full column count, where an entry of the dense conversion fetched it (-1: not known)
  };
  static constexpr int kAlgLens = 8;
  AlgLen alg_len[kAlgLens];
  int alg_len_next = 0;
  int add_mode = 0;           // what the last dbcsr_amd_bcsr_add_count found: 0 nothing pending, 1 same pattern (flat pass), 2 union pattern
  int add_beta_zero = 0;
  int64_t add_nblks_a = 0, add_nblks_b = 0, add_nblks = 0, add_nze = 0;

  // ---- element-wise operations on two patterns (mm_engine_elementwise.h): what dbcsr_amd_bcsr_hadamard_count leaves for its _apply, in buffers and fields
  // that no other entry writes -- an add, a norm or a multiply between the two halves changes nothing here, and these change nothing of theirs ----
  DevBuf<int> ew_i32;         // partner[nblks of A], blk_nze[nblks of A], row_cnt[nblkrows]
  DevBuf<int64_t> ew_i64;     // off[nblks of A]: the result offset of every kept block of A; behind it src[2 * nblks of the result] (sized for all of A)
  int had_mode = 0;           // what the last dbcsr_amd_bcsr_hadamard_count found: 0 nothing pending, 1 same pattern (flat pass), 2 two patterns
  int had_assumed = 0;
  int64_t had_nblks_a = 0, had_nblks_b = 0, had_nblks = 0, had_nze = 0;

  // ---- block lists (mm_engine_blocklist.h): reserve, put and get through a coordinate list of blocks, in buffers and fields that no other entry writes --
  // a put between the two halves of an add, a hadamard product, a filter or a twin move changes nothing of theirs, and these change nothing here.  A
  // reserve count that found blocks to create has gone on into the symbolic phase's work areas (cin_bm, c_bm, cin_pre, c_pre, c_blk_p_ws), as the union
  // add does: engine_takes_work_areas ends it ----
  DevBuf<uint32_t> bl_bm;     // reserve: the bits of the listed blocks the matrix lacks [nblkrows][W]
  DevBuf<unsigned long long> bl_cnt;   // reserve: blocks to create, invalid entries, elements of the new blocks, elements the matrix names
  DevBuf<int> bl_i32;         // put: hit[n], slots[n], order[n], cnt[nblks + 1], seg[nblks + 1]
  bool rsv_pending = false;   // a dbcsr_amd_bcsr_reserve_count found blocks to create and nothing has taken the work areas since
  const void* rsv_row_p = nullptr;   // ... for the matrix with this row_p, these sizes and this many blocks
  int rsv_nblkrows = 0, rsv_nblkcols = 0;
  int64_t rsv_nblks_a = 0, rsv_nblks = 0, rsv_nze = 0;

  // ---- element CSR (mm_engine_csr.h): what dbcsr_amd_bcsr_to_csr_count leaves for its _apply, in buffers and fields that no other entry writes -- an
  // add, a norm, a put or a multiply between the two halves changes nothing here, and these change nothing of theirs ----
  DevBuf<int64_t> csr_off;    // of the counted matrix: roff[nblkrows + 1], coff[nblkcols + 1], base[nblkrows + 1] (the first slot of every block row)
  DevBuf<int64_t> csr_pos;    // pos[nslots + 1]: the CSR position of every row piece, the total behind them
  DevBuf<int> csr_slots;      // slots[nslots]: the kept elements of every row piece
  DevBuf<int> csr_rows;       // the slots of every block row [nblkrows]: what base is the scan of
  DevBuf<int64_t> csr_aux;    // _from_csr and _csr_name_blocks: roff, coff of their block sizes (nothing is pending in it)
  bool csr_pending = false;   // a dbcsr_amd_bcsr_to_csr_count succeeded and no _apply has served it
  const void *csr_row_p = nullptr, *csr_rs = nullptr, *csr_cs = nullptr;   // ... for the matrix with this row_p, these size arrays,
  int csr_nblkrows = 0, csr_nblkcols = 0, csr_datatype = 0, csr_use_eps = 0;   // these counts, this type and this filter
  int64_t csr_nblks = 0, csr_nnz = 0, csr_nslots = 0;
  double csr_eps = 0.0;
  // the slot count of an index (and its element count, the nnz without eps), which only the device knows: remembered per index as alg_len remembers
  // the lengths (same row_p and size arrays, same non-zero index_stamp), fetched otherwise -- then, and only then, a count synchronises for them
  struct CsrLen {
    const void* row_p = nullptr;
    const void* rs = nullptr;
    const void* cs = nullptr;
    uint64_t stamp = 0;
    int nbr = 0, nbc = 0;
    int64_t nblks = 0, nslots = 0;
    int64_t nze = -1;   // the elements the index names, where a count without eps fetched them (-1: not known)
  };
  static constexpr int kCsrLens = 8;
  CsrLen csr_len[kCsrLens];
  int csr_len_next = 0;

  // ---- re-blocking (mm_engine_reblock.h): buffers that no other entry writes; nothing is pending in them between two calls ----
  DevBuf<int64_t> rb_off;     // the running sums of the source's block sizes and of the new ones: roff, coff, new roff, new coff
  DevBuf<int64_t> rb_pos;     // _reblock_name_blocks: the place of every source block's first piece [nblks + 1]
  DevBuf<int> rb_i32;         // _reblock_name_blocks: per source block its pieces [nblks], then (first new block row, first new block column, column span)

  // ---- switches (mm_engine_env.h) ----
  Switches sw;      // the numeric phase's kernel families (mm_choose.h)
  LabSwitches lab;  // lab build only: no state in the shipping build
  int use_plan = 1;  // DBCSR_AMD_MM_PLAN=0: every multiply runs its symbolic phase
  int force_symbolic = 0;     // DBCSR_AMD_MM_SYMBOLIC: 0 automatic, 1 word (the per-word kernels), 2 grid, 3 rows (SymbolicSizes::forced, mm_choose.h)
  int64_t panel_bytes = 256ll << 20;  // DBCSR_AMD_MM_PANEL_MB: target size of a B column panel (config 2, round 3: 160 / 200 / 256 / 320 / 400 MB ->
                                      // 18.97 / 18.76 / 18.63 / 18.95 / 19.04 ms, profiles/r03_panel_wgwaves_sweep.txt)

  // ---- plan reuse (plan_compare): device copies of the index arrays the last symbolic phase saw, C's index as the numeric phase emitted it ----
  bool plan_saved = false, plan_hit = false, plan_numeric = false;
  int plan_dims[3] = {0, 0, 0}, plan_retain = 0, plan_canonical = 0, plan_datatype = 0;
  int64_t plan_nblks[3] = {0, 0, 0};
  // dbcsr_amd_mm_trust_plan: index arrays at the ADDRESSES the saved plan saw are taken as unchanged (no comparison on the device, no
  // synchronisation): for callers that own their operands' index and never write it in place
  bool plan_trusted = false;
  const void* plan_ptrs[12] = {nullptr};
  uint64_t plan_stamps[3] = {0, 0, 0};  // index_stamp of A, B, C_in when the plan was saved (0: unknown generation, never trusted)
  DevBuf<int32_t> plan_words, plan_c_col_i;
  DevBuf<int64_t> plan_c_blk_p;
  DevBuf<int> plan_flag;
  int* plan_host_flag = nullptr;  // pinned
  dbcsr_amd_mm_counts plan_counts = {0, 0, 0, 0};
  long long plan_hits = 0, plan_misses = 0;

#ifdef DBCSR_AMD_EXPERIMENTS
  LabState ls;
#endif
};

// Every entry that writes a matrix's values passes through here before it launches: the block norms a numeric kernel left (norms_data, norms64) are those
// of the values before the write, so dbcsr_amd_bcsr_filter_count must form them again.  (The engine does not know which matrix is written through a view
// or another descriptor of the same data area: any write forgets them.)
static inline void engine_writes_values(Engine* E) { E->norms_data = nullptr; }

// The count halves of the two-call protocols (filter, crop, union add, twin / desymmetrize) leave their answer in work areas that the symbolic phase, each
// other's count and the transpose write too.  Whoever is about to write those areas calls this first: a count that is still pending is over, and its
// apply half then refuses (-1) and writes nothing instead of compacting by what this call left there.  Every apply half asks for a pending count of ITS
// OWN pair (flt_pending, crop_pending, add_mode, twin_mode, rsv_pending), never for a block count alone: a crop count of a matrix with as many blocks as the filter's
// ends the filter's count like any other.  The filter's and the twin's counts stay pending after an apply (the apply may be repeated); a count of a twin
// is pending for one matrix shape (nblks, nblkrows) and one mode.
static inline void engine_takes_work_areas(Engine* E) {
  E->flt_nblks = -1;
  E->flt_new_nblks = -1;
  E->flt_pending = false;
  E->crop_pending = false;
  E->twin_mode = -1;
  if (E->add_mode == 2) E->add_mode = 0;
  E->rsv_pending = false;
}

KPassMemo* engine_kpass_memo(void* handle) { return handle ? &static_cast<Engine*>(handle)->kpass_memo : nullptr; }
int engine_filter_in_place(void* handle) { return handle ? static_cast<Engine*>(handle)->filter_in_place : 0; }

// waves per block row for the kernels that stream whole blocks (norms, compaction): enough waves to keep the memory system busy
static inline int row_split(int64_t nbr, int64_t nblks) {
  if (nbr <= 0) return 1;
  const int64_t per_row = nblks / nbr;
  int64_t S = (65536 + nbr - 1) / nbr;
  if (S > per_row) S = per_row;
  return (int)std::max<int64_t>(1, std::min<int64_t>(S, 64));
}

template <typename TO>
static int exclusive_scan(Engine* E, const int* in, int64_t n, TO* out, int64_t* total_dev, bool write_total_at_n, hipStream_t st) {
  const int nb = (int)((n + kScanChunk - 1) / kScanChunk);
  if (E->partial.ensure((size_t)(nb > 0 ? nb : 1))) return -1;
  if (n <= 0) {
    if (total_dev) ACC_CHECK(hipMemsetAsync(total_dev, 0, sizeof(int64_t), st));
    if (write_total_at_n) ACC_CHECK(hipMemsetAsync(out, 0, sizeof(TO), st));
    return 0;
  }
  hipLaunchKernelGGL(scan_reduce, dim3(nb), dim3(kScanThreads), 0, st, in, n, E->partial.p);
  hipLaunchKernelGGL(scan_partials, dim3(1), dim3(kScanThreads), 0, st, E->partial.p, nb, total_dev);
  hipLaunchKernelGGL((scan_apply<TO>), dim3(nb), dim3(kScanThreads), 0, st, in, n, E->partial.p, out, write_total_at_n ? 1 : 0);
  return check(hipGetLastError(), "exclusive_scan", __FILE__, __LINE__);
}

static inline dim3 grid_for(int64_t nthreads) { return dim3((unsigned)((nthreads + 255) / 256)); }

#endif
