// mm_choose.h -- which numeric kernel a multiply runs, as a pure function of what the symbolic phase learned and of the switches.  Nothing of HIP in here: the
// header compiles with a plain C++ compiler, so the rules are tested without a GPU (tests/test_numeric_choice.py).  mm_engine.hip fills SizeFacts / Switches /
// LabSwitches, calls choose_numeric and launches what the NumericChoice says; the kernel instance lists live here, beside the predicates that answer "is there
// an instance" (the launchers in mm_engine_launch.h / mm_mid.hip expand the same lists).
#ifndef DBCSR_AMD_MM_CHOOSE_H
#define DBCSR_AMD_MM_CHOOSE_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace dbcsr_amd {

// ---- instance lists ----------------------------------------------------------------------------------------------------------------------------------------
// Exact-size kernels are instantiated for every cube from 9 to 32 (the reference compiles one kernel per (m, n, k) at run
// time; here the list is fixed at build time and every other case -- mixed sizes, blocks above 32 -- runs the generic kernels; measured on 4 x 4 blocks the generic kernel is 7 % faster, so sizes
// up to 8 are left to it).
#define DBCSR_AMD_HOT_SIZES(X) \
  X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#define DBCSR_AMD_DMA_SIZES(X) X(13) X(16) X(23) X(32)
// the direct form of the fp32 exact-size kernel: cubes whose k is a multiple of 8
#define DBCSR_AMD_F32_DIRECT_SIZES(X) X(16) X(24) X(32)
// the one-wave slab kernels (mm_numeric_f64_mid.h): (rows, columns) in units of 4
#define DBCSR_AMD_MID_SHAPES(X)                                                                             \
  X(6, 8) X(6, 9) X(6, 10) X(6, 11) X(6, 12)                                                                \
  X(7, 9) X(7, 10) X(7, 11) X(7, 12)                                                                        \
  X(8, 6) X(8, 8) X(8, 9) X(8, 10) X(8, 11) X(8, 12)                                                        \
  X(9, 6) X(9, 7) X(9, 8) X(9, 9) X(9, 10) X(9, 11) X(9, 12)                                                \
  X(10, 6) X(10, 7) X(10, 8) X(10, 9) X(10, 10) X(10, 11) X(10, 12)                                         \
  X(11, 6) X(11, 7) X(11, 8) X(11, 9) X(11, 10) X(11, 11) X(11, 12)                                         \
  X(12, 6) X(12, 7) X(12, 8) X(12, 9) X(12, 10) X(12, 11) X(12, 12)

#define DBCSR_AMD_IS_(S_) || s == S_
static inline bool hot_f64_has(int m, int n, int k) { const int s = m; return m == n && m == k && (false DBCSR_AMD_HOT_SIZES(DBCSR_AMD_IS_)); }
static inline bool dma_f64_has(int stages, int m, int n, int k) { const int s = m; return stages >= 2 && stages <= 4 && m == n && m == k && (false DBCSR_AMD_DMA_SIZES(DBCSR_AMD_IS_)); }
static inline bool f32_direct_has(int m, int n, int k) { const int s = m; return m == n && m == k && (false DBCSR_AMD_F32_DIRECT_SIZES(DBCSR_AMD_IS_)); }
#undef DBCSR_AMD_IS_
// mm_numeric_f64_big<TM, TN>: every pair of 2 ... 5
static inline bool big_f64_has(int tm, int tn) { return tm >= 2 && tm <= 5 && tn >= 2 && tn <= 5; }
static inline int big_tiles(int size) { return std::max(2, ((size + 7) / 8 + 1) / 2); }   // ... tiles of 8 per wave for blocks of that many rows / columns
// mm_numeric_z64<MA, NC> (complex_8, mm_numeric_z64.h): every pair of 1 ... 4; tiles of 8 rows / columns of the instance that serves blocks of that size
// (a dimension above 32 is covered in several tiles of 32), and the per-wave LDS slice: A's slab of 8 columns of 8 MA + 1 elements, B's 8 NC runs of 9
static inline bool z64_has(int ma, int nc) { return ma >= 1 && ma <= 4 && nc >= 1 && nc <= 4; }
static inline int z64_tiles(int size) { return std::max(1, (std::min(size, 32) + 7) / 8); }
static inline constexpr int z64_slice_bytes(int ma, int nc) { return 8 * (8 * ma + 1) * 16 + 8 * nc * 9 * 16; }
static inline bool mid_f64_has(int rb, int cb) {
#define DBCSR_AMD_IS_(A_, B_) || (rb == A_ && cb == B_)
  return false DBCSR_AMD_MID_SHAPES(DBCSR_AMD_IS_);
#undef DBCSR_AMD_IS_
}

// Which shapes the slab kernel should take (class_mode: 0 = the dominant size of a multiply, 1 = an (m, n) class of a mixed-size multiply, 3: as 1 without
// the classes of 21 ... 24 in one dimension).  Every shape it answers yes for has an instance (mid_f64_has).  Measured (profiles/r06_slab_kernel.txt):
//  * a dimension beyond 32 (9 / 10 units): the alternative is the workgroup kernel, which it beats (33^3 0.29 -> 0.36, 40^3 0.46 -> 0.55 of the fp64 peak);
//  * uniform blocks of 25 ... 32: the exact-size kernels win or tie (28^3 0.43 against 0.39, 30^3 0.49 / 0.42; 32^3 0.55 / 0.53 once hot<32,32,32>
//    stages with a padded pitch) -- not taken;
//  * the (32, 32), (32, 23), (23, 32) CLASSES of a mixed-size multiply with few products per C block (config 3: 3.6): the class kernels stage whole
//    blocks in 15-18 KB per wave, two waves per SIMD; with the slab kernel on these three classes config 3 takes 7.15 instead of 7.6 ms -- taken
//    (DBCSR_AMD_MM_MID=3: only (32, 32)).
//  * a dimension of 41 ... 48 (11 / 12 units; session r06_24): a tie with the workgroup kernel on cubes (41^3 0.40 / 0.40, 44^3 0.48 / 0.47, 45^3 0.45 / 0.46,
//    48^3 0.60 / 0.56 -- 0.31 / 0.33 at 5 % fill), a clear win when the other dimension is at most 40 (48 x 36 x 23: 0.51 against 0.43) -- taken then,
//    and for multiples of 4 in both (no padding inside the units).
static inline bool mid_f64_serves(int m, int n, int class_mode) {
  const int rb = (m + 3) / 4, cb = (n + 3) / 4;
  const int lo = rb < cb ? rb : cb, hi = rb < cb ? cb : rb;
  if (lo < 6 || hi > 12 || hi < 8) return false;
  if (hi >= 11) return lo <= 10 || (m % 4 == 0 && n % 4 == 0);
  if (hi >= 9) return true;
  return class_mode > 0 && (lo == 8 || (lo == 6 && class_mode != 3));
}

// ---- what the choice reads -----------------------------------------------------------------------------------------------------------------------------------
// What the symbolic phase learned about the multiply (the engine keeps it from the symbolic to the numeric phase), plus four facts of the numeric call itself.
struct SizeFacts {
  int max_m = 0, max_k = 0, max_n = 0, min_m = 0, min_k = 0, min_n = 0;
  int hot_m = 0, hot_n = 0, hot_k = 0;              // dominant block sizes (0: none covers 90 % of every dimension)
  int hot_cnt_m = 0, hot_cnt_k = 0, hot_cnt_n = 0;  // block rows / inner blocks / block columns of the most frequent size
  int units_m = 0, units_cnt_m = 0, units_n = 0, units_cnt_n = 0;   // most frequent size of C's rows / columns in units of 4 (sizes up to 48) and how often (block_size_stats)
  int nbr = 0, nbc = 0;
  int64_t c_nblks = 0, nproducts = 0, order_len = 0;
  bool cls_mode = false;                            // (m, n) classes (mixed block sizes, see order_count_cls)
  int cls_m[3] = {0, 0, 0}, cls_n[3] = {0, 0, 0}, cls_k[3] = {0, 0, 0};
  bool retain = false;
  int canonical_c = 0;   // dbcsr_amd_mm_set_canonical_product: the product matrix has symmetry, its index is in canonical form
  // of the numeric call
  bool filter_active = false;   // the symbolic phase filtered on the fly (block norms of A and B are at hand)
  bool fp64 = true;
  int skip_empty = 0;           // in-place accumulation: C blocks without products are left untouched
  bool cplx = false;            // complex_8 data: the one complex family serves every size (mm_numeric_z64.h)

  bool sizes_within(int s) const { return max_m <= s && max_k <= s && max_n <= s && min_m >= 1 && min_k >= 1 && min_n >= 1; }
  bool no_empty_dim() const { return min_m >= 1 && min_n >= 1 && min_k >= 1; }
  bool dominant_cube() const { return hot_m > 0 && hot_m == hot_n && hot_m == hot_k; }
  bool other_sizes() const { return hot_cnt_m < nbr || hot_cnt_n < nbc; }   // C blocks outside the dominant size (tail block row / column)
};

// The shipping switches (mm_engine_env.h reads them once per engine).
struct Switches {
  int use_lds = 1;     // DBCSR_AMD_MM_KERNEL=direct selects the v1 kernel (A/B experiments)
  int use_pipe = -1, pipe_g = 8;  // multi-block pipelined kernel: -1 automatic (short product lists only), DBCSR_AMD_MM_KERNEL=pipe|lds1 forces; DBCSR_AMD_MM_PIPE_G = blocks per wave
  int use_hot = 1;     // DBCSR_AMD_MM_HOT=0: never use the exact-size kernels
  int use_tiny = 1;    // DBCSR_AMD_MM_TINY=0: no packed kernel for blocks of at most 4 x 4
  int use_small = 2;   // DBCSR_AMD_MM_SMALL=0: no one-tile kernel for multiplies whose block dimensions are all <= 8 (mm_numeric_f64_small.h); 2 (default) / 3 / 4 / 6 / 8: products in flight per wave
  int small_group = 0; // DBCSR_AMD_MM_SMALL_G: C blocks a wave of the small-block kernel takes one after the other (0: eight when the lists are short, else one)
  int use_mid = 1;     // DBCSR_AMD_MM_MID=0: blocks of 33 ... 40 through the workgroup kernel mm_numeric_f64_big instead of the one-wave kernel mm_numeric_f64_mid
  int use_big = 1;     // DBCSR_AMD_MM_BIG=0: blocks above 32 through the one-wave-per-block kernel of rounds 1-4 (mm_numeric_f64) instead of mm_numeric_f64_big
  int use_work = 1;    // DBCSR_AMD_MM_WORK=0: the class kernels read order[] -> descs[] -> entries[] instead of the launch-order records
  int use_classes = 1; // DBCSR_AMD_MM_CLASSES = 0 never, 1 automatic, 2 always when the sizes allow
  int wg_waves = 0;    // DBCSR_AMD_MM_WG_WAVES = 1 | 2 | 4: waves per workgroup of the one-wave-per-C-block kernels (0: by list length).  A workgroup's LDS is
                       // released when its LAST wave ends, so with product lists of uneven length fewer waves per workgroup keep
                       // more of the CU's wave slots busy (config 3: kernel 8.93 / 8.09 / 7.51 ms for 4 / 2 / 1, config 2: 23.6 / 22.7 /
                       // 22.6, config 4: 30.1 / 28.8 / 28.4 on the same box, profiles/r02_wg_waves_bench_lines.txt)
  int f32_direct = 1;  // (2: + the slim-LDS launch when every C block has the dominant size -- more waves per CU, measured 0-4 % slower: the
                       // kernel is fabric-bound, round 5 session 17 --, 1: never slim) DBCSR_AMD_MM_F32_DIRECT=0: the fp32 exact-size kernel that stages both operands in LDS (rounds 1-4) instead of the direct form
};

// The lab build's switches (-DDBCSR_AMD_EXPERIMENTS): every one selects something that was measured and does not win.  The shipping build has no such state:
// the names are constants at their defaults there, and every condition on them folds away.  (Two layouts under one name: every function of this header
// has internal linkage, so that the two libraries, which may live in one process, never share a copy.)
struct LabSwitches {
#ifdef DBCSR_AMD_EXPERIMENTS
#define DBCSR_AMD_LAB_INT_ int
#else
#define DBCSR_AMD_LAB_INT_ static constexpr int
#endif
  DBCSR_AMD_LAB_INT_ dbg = 0;             // DBCSR_AMD_MM_DBG: ablation switches of the LDS kernel (profiling only; the exact-size kernel honours them in its VAR = 1 build)
  DBCSR_AMD_LAB_INT_ dma_stages = 0;      // DBCSR_AMD_MM_KERNEL=dma2|dma3|dma4: LDS-DMA exact-size kernel with that many ring slots (0: off)
  DBCSR_AMD_LAB_INT_ hot_persistent = 0;  // DBCSR_AMD_MM_HOT_PERSISTENT=1: the 23^3 kernel as persistent waves with a work counter per XCD (mm_numeric_f64.h)
  DBCSR_AMD_LAB_INT_ hot_variant = 0;     // DBCSR_AMD_MM_HOT_VARIANT: 2 = exact-size kernel with unpaired ds_read_b64 fragment reads (23^3 only)
  DBCSR_AMD_LAB_INT_ lds_pad = 0;         // DBCSR_AMD_MM_LDS_PAD: extra LDS bytes per workgroup (occupancy experiments)
  DBCSR_AMD_LAB_INT_ class_g = 1;         // DBCSR_AMD_MM_CLASS_G: C blocks per wave in the class kernels (1, 2, 4, 8)
  // DBCSR_AMD_MM_CLASS_STREAMS: the class launches of one multiply touch disjoint C blocks; with n > 1 they are spread over n streams
  // (the caller's + n - 1 of the engine's, forked / joined with events) so that the tail of one launch overlaps the body of the next
  DBCSR_AMD_LAB_INT_ class_streams = 1;
  DBCSR_AMD_LAB_INT_ row_group = 0;       // DBCSR_AMD_MM_ROW_GROUP: rows walked together per XCD (0 = automatic)
  // fp32: a wave owns R C blocks of one block column and shares B among them (mm_group.h).  DBCSR_AMD_MM_F32_GROUP = 2 / 3 / 4: that R
  // whenever the kernel applies; -1: R = 4 when C blocks have at least 16 products on average; 0 / unset: off -- measured (round 5, session 4:
  // 32768^2 at 20 % fill 32.1 ms against 28.6 for one wave per block, config 5 2125 against 1836 ms) it trades B blocks over the fabric for
  // A rows that no longer fit the XCD's L2 and for occupancy (3 waves per SIMD instead of 5), and loses
  DBCSR_AMD_LAB_INT_ f32_group = 0;
  // fp64 (round 6, mm_group64.h): DBCSR_AMD_MM_F64_GROUP = 2 ... 6: a wave owns that many C blocks of one block column whenever the kernel
  // applies; 0 / unset: off
  DBCSR_AMD_LAB_INT_ f64_group = 0;
  DBCSR_AMD_LAB_INT_ use_tile = 0;        // XCD-wide C tiles in registers (mm_tile.h): DBCSR_AMD_MM_TILE = 0 never, 1 automatic, 2 whenever the sizes allow
  DBCSR_AMD_LAB_INT_ use_band = 0;        // CU-wide C tiles, B shared in an LDS ring (mm_band.h): DBCSR_AMD_MM_BAND = 0 never, 1 automatic, 2 whenever the sizes allow
#undef DBCSR_AMD_LAB_INT_
  // an ablation switch, a ring kernel, the persistent form or a variant of the exact-size kernel was asked for: the other kernel families stand back
  bool variant_active() const { return (dbg & ~32) != 0 || dma_stages != 0 || hot_persistent != 0 || hot_variant != 0; }
};

// ---- (m, n) classes: the decision of the symbolic phase ------------------------------------------------------------------------------------------------------
// the three most frequent sizes of a histogram over 1 ... 32 (0: fewer than that many sizes occur)
static inline void top3_sizes(const int* hist, int* out) {
  int used[3] = {-1, -1, -1};
  for (int r = 0; r < 3; ++r) {
    int best = 0, bc = 0;
    for (int sz = 1; sz <= 32; ++sz)
      if (hist[sz] > bc && sz != used[0] && sz != used[1]) best = sz, bc = hist[sz];
    out[r] = best;
    used[r] = best ? best : -1;
  }
}
// (m, n) classes: blocks of at most 32 in every dimension, no single dominant size (that case has its ahead-of-time
// kernel), not the packed 4 x 4 case, and enough C blocks to pay for compiling the class kernels (forced with
// DBCSR_AMD_MM_CLASSES=2)
// (a dominant triplet that is NOT a cube of 9 ... 32 has no ahead-of-time kernel: uniform rectangular blocks -- 5 x 13 x 23, 23 x 23 x 5 -- took the
//  run-time-size kernel until round 6, session 43; they are one class with one inner size)
// hist: the 3 x 33 histograms of the sizes of m, n, k.  Sets cls_mode and, when the sizes allow classes at all, cls_m / cls_n / cls_k.
static inline void choose_classes(SizeFacts* f, const Switches& sw, const int* hist) {
  f->cls_mode = false;
  const bool hot_cube = f->hot_m >= 9 && f->dominant_cube();
  if (sw.use_classes > 0 && f->sizes_within(32) && !(f->max_m <= 4 && f->max_n <= 4) && (sw.use_classes > 1 || (!hot_cube && f->c_nblks >= 200000))) {
    top3_sizes(hist, f->cls_m);
    top3_sizes(hist + 33, f->cls_n);
    top3_sizes(hist + 66, f->cls_k);
    f->cls_mode = f->cls_m[0] > 0 && f->cls_n[0] > 0 && f->cls_k[0] > 0;
  }
}

// ---- the numeric phase's choice ------------------------------------------------------------------------------------------------------------------------------
enum class Family {
  f64_tiny, f64_small8, f64_mid, f64_classes, f64_hot, f64_pipe, f64_lds, f64_big, f64_generic, f32_classes, f32_direct, f32_hot, f32_lds, f32_generic,
  f64_group, f64_tile, f64_band, f64_dma, f64_persistent, f32_group,  // lab build only
  z64                                                                 // complex_8
};

struct NumericChoice {
  Family family = Family::f64_generic;
  char name[96] = "";    // what dbcsr_amd_mm_last_kernel reports (the class families append their launch counts at run time)
  int ww = 4;            // waves per workgroup of the one-wave-per-C-block kernels
  // work: the kernels read launch-order work records (build_work).  norms: the norm area is set up -- kernels that can leave every C block's squared norm
  // behind do (and skip the blocks below the announced filter); leaves_norms: ... and the chosen family is one of those
  bool work = false, norms = false, leaves_norms = false;
  unsigned grid = 0;     // workgroups (the class families: per class, from the class's length)
  size_t lds_bytes = 0;  // dynamic LDS per workgroup
  int flags = 0;         // the kernel's flag word (skip_empty / dbg argument)
  int lds_a = 0, lds_wave = 0, maxt = 0;   // per-wave LDS slice of the kernels that stage whole blocks (doubles), MAXT of the generic LDS / pipe kernels
  // slab kernel: the exact launch's shape in units of 4 (0: not the slab kernel); class family: mid_f64_serves' mode for the classes that may take the
  // slab kernel (0: none does)
  int mid_rb = 0, mid_cb = 0, mid_class_mode = 0;
  int depth = 0, group = 0;                // small-block kernel: products in flight, C blocks per wave; pipe kernel: C blocks per wave
  bool slim = false;                       // fp32 direct kernel: LDS for the B images only
  int variant = 0, group_R = 0;            // lab: variant of the exact-size kernel, C blocks per wave of the group kernels
};

// Waves per workgroup of the one-wave-per-C-block kernels.  A workgroup's LDS is released when its LAST wave ends: with short,
// uneven product lists one wave per workgroup keeps more wave slots busy (config 3: kernel 8.93 -> 7.51 ms, generic LDS kernel
// 12.3 -> 9.2, config 2: -5 %, config 4: -6 %); with long lists four waves per workgroup are faster (config 5, 164 products per
// block: 2.03 s against 2.27 s)
static inline int choose_wg_waves(const SizeFacts& f, const Switches& sw) { return sw.wg_waves > 0 ? sw.wg_waves : (f.nproducts <= 32 * f.c_nblks ? 1 : 4); }

// The one-wave slab kernel (mm_numeric_f64_mid.h): fp64 C blocks whose dominant (else largest) size has a dimension of 33 ... 40 and the other of
// 21 ... 40 (mid_f64_serves), any inner dimension; its second launch takes the blocks of another size.  Mixed-size multiplies (cls_mode) ask per class.
static inline void choose_mid_shape(const SizeFacts& f, const Switches& sw, const LabSwitches& lab, int* mid_rb, int* mid_cb) {
  *mid_rb = *mid_cb = 0;
  if (!(f.fp64 && sw.use_big && sw.use_mid && sw.use_lds && !f.cls_mode && f.max_m <= 48 && f.max_n <= 48 && f.no_empty_dim() && f.order_len > 0 &&
        !lab.variant_active() && sw.use_hot && sw.use_pipe != 1))
    return;
  // (without a dominant size -- the size statistics stop at 32 -- the largest size is multiplied exactly when the blocks go beyond 32, where the
  // alternative is the workgroup kernel, or when every block is in the range: the second launch pads the others to 40 x 40)
  const bool dom = f.hot_m > 0 && f.hot_n > 0, all_in = (f.min_m > 24 && f.min_n > 24) || f.max_m > 32 || f.max_n > 32;
  const int dm = dom ? f.hot_m : (all_in ? f.max_m : 0), dn = dom ? f.hot_n : (all_in ? f.max_n : 0);
  if (dm > 0 && dn > 0 && mid_f64_serves(dm, dn, 0)) *mid_rb = (dm + 3) / 4, *mid_cb = (dn + 3) / 4;
  if (*mid_rb && !dom) {
    // No dominant size: the exact launch would serve a minority and the second launch -- the largest shape, 10 x 10 or 12 x 12 units -- pads everything
    // else (30 / 36 mixed: 43 ms against 29 through the workgroup kernel, session r06_47).  The slab kernel stays when ONE launch serves every block -- the
    // largest blocks ARE the largest shape (30 / 40, 34 / 40, 23 / 40: +14-17 %) -- or when at least 80 % of C's rows and of its columns have the exact
    // launch's units (33 / 36: +17 %; 36 with a tail block).
    const int mu = (std::max(f.max_m, f.max_n) + 3) / 4, fb = (mu > 10 || *mid_rb > 10 || *mid_cb > 10) ? 12 : 10;
    const bool single = *mid_rb == fb && *mid_cb == fb;
    const bool most = 10ll * f.units_cnt_m >= 8ll * f.nbr && 10ll * f.units_cnt_n >= 8ll * f.nbc && mid_f64_serves(4 * f.units_m, 4 * f.units_n, 0);
    if (most)
      *mid_rb = f.units_m, *mid_cb = f.units_n;   // (the exact launch takes the most frequent shape, the second launch the rest)
    else if (!single)
      *mid_rb = *mid_cb = 0;
  }
}

// The rules, in the order that decides: complex data has its one family (z64); tiny -> small8 -> mid -> classes -> (lab: group, tile, band, dma, persistent) -> hot -> pipe / lds -> big -> generic
// for fp64, classes -> (lab: group) -> direct -> hot -> lds -> generic for fp32.  `work` and `norms` are decided BEFORE the family, as the set-up steps they
// stand for run before the launch.  Two reachable combinations set something up that the family then does not use, both kept as they always were:
//  * a dominant cube of at most 8 (no exact-size instance) with the small-block kernel switched off builds work records and arms the norms, then runs the
//    generic LDS / pipe kernel;
//  * a mixed-size multiply in class mode with DBCSR_AMD_MM_KERNEL=direct and an on-the-fly filter arms the norms (the class arm of `norms`), then runs the
//    plain kernel mm_numeric_f64.
// Neither kernel leaves norms (leaves_norms stays false: the filter computes them), both write every block although unwritten_below names the announced
// threshold -- for a follow-up.
static inline NumericChoice choose_numeric(const SizeFacts& f, const Switches& sw, const LabSwitches& lab) {
  NumericChoice c;
  const int64_t nblk = f.c_nblks, npos = 8 * f.order_len;
  const int skip = f.skip_empty, hm = f.hot_m, hn = f.hot_n, hk = f.hot_k;
  const int dbg_flags = lab.dbg | (skip ? 32 : 0);
  const bool small = f.sizes_within(32);
  c.ww = choose_wg_waves(f, sw);
  const unsigned per_wave = (unsigned)(npos / c.ww), per_block = (unsigned)npos, quads = (unsigned)((nblk + 3) / 4);   // grids: a wave / a workgroup per position, four blocks per workgroup
  auto pick = [&c](Family fam, unsigned grid, int flags, const char* fmt, int a = 0, int b = 0, int d = 0, int e = 0) {
    c.family = fam, c.grid = grid, c.flags = flags;
    c.leaves_norms = c.norms && (fam == Family::f64_mid || fam == Family::f64_classes || fam == Family::f64_hot || fam == Family::f64_persistent);
    snprintf(c.name, sizeof c.name, fmt, a, b, d, e);
    return c;
  };
  if (f.cplx) {
    // complex_8: one wave per C block in the instance of the multiply's largest block; no work records, no norms (the block filter computes them)
    const int ma = z64_tiles(f.max_m), nc = z64_tiles(f.max_n);
    c.lds_bytes = (size_t)c.ww * (size_t)z64_slice_bytes(ma, nc);
    const unsigned waves = (unsigned)(f.order_len > 0 ? npos : nblk);
    return pick(Family::z64, (waves + (unsigned)c.ww - 1) / (unsigned)c.ww, skip, "mm_numeric_z64<%d,%d>", ma, nc);
  }
  if (!f.fp64) {
    if (!(small && sw.use_lds)) return pick(Family::f32_generic, quads, skip, "mm_numeric_f32");
    if (f.cls_mode) return pick(Family::f32_classes, per_wave, skip, "mm_numeric_f32_lds[per class segment]");
    // lab: a wave per R C blocks of one block column (mm_group.h): one dominant cube the direct kernel serves, no tail in the inner dimension
    if (sw.use_hot && f.dominant_cube() && sw.f32_direct && lab.f32_group != 0 && f.min_k == f.max_k && f.max_k == hk &&
        (lab.f32_group > 0 || (f.nproducts >= 16 * nblk && nblk >= 1024))) {
      c.group_R = lab.f32_group > 0 ? lab.f32_group : 4;
      return pick(Family::f32_group, per_wave, skip, "mm_numeric_f32_group<%d,%d,%d;%d>", hm, hn, hk, c.group_R);
    }
    c.slim = sw.f32_direct >= 2 && f.hot_cnt_m == f.nbr && f.hot_cnt_n == f.nbc;
    if (sw.use_hot && hm > 0 && sw.f32_direct && f32_direct_has(hm, hn, hk)) return pick(Family::f32_direct, per_wave, skip, "mm_numeric_f32_direct<%d,%d,%d>", hm, hn, hk);
    if (sw.use_hot && hm > 0 && hot_f64_has(hm, hn, hk)) return pick(Family::f32_hot, per_wave, skip, "mm_numeric_f32_hot<%d,%d,%d>", hm, hn, hk);
    return pick(Family::f32_lds, per_wave, skip, "mm_numeric_f32_lds");
  }

  // ---- fp64: what is set up before the launch ----
  choose_mid_shape(f, sw, lab, &c.mid_rb, &c.mid_cb);
  // every block dimension at most 8 (and not the packed 4 x 4 case): one 8 x 8 tile per wave, several products in flight (mm_numeric_f64_small.h)
  const bool tiny4 = sw.use_tiny && f.max_m <= 4 && f.max_n <= 4;
  const bool small8 = sw.use_small > 0 && sw.use_lds && !tiny4 && f.sizes_within(8) && !lab.variant_active() && sw.use_pipe < 0;  // (DBCSR_AMD_MM_KERNEL=lds1 | pipe ask for those kernels)
  // the exact-size kernel may run (the instance list is asked below, after the set-up, as it always was)
  const bool hot_allowed = sw.use_hot && sw.use_pipe != 1 && hm > 0;
  // launch-order work records for the exact-size fp64 kernels (one wave per C block): descriptor + first product in one read
  // (the ahead-of-time exact-size kernel reads nothing else; the class kernels keep the order[] -> descs[] path for DBCSR_AMD_MM_WORK=0)
  const bool exact = f.cls_mode ? (lab.class_g == 1 && sw.use_work) : (hot_allowed && lab.dma_stages == 0 && f.dominant_cube());
  c.work = ((sw.use_lds && small && !tiny4 && !small8 && exact) || c.mid_rb || (small8 && sw.use_work)) && npos > 0;
  // a filtered multiply ends with the block filter on C's norms: the exact-size kernel leaves them behind (dbcsr_amd_bcsr_filter_count
  // then skips its pass over C)
  // (lab, dbg & 8: profiling epilogue of the exact-size kernel: it leaves no norms, the filter then computes them)
  c.norms = (c.work || (f.cls_mode && lab.class_g == 1)) && !small8 && f.filter_active && !skip && !f.retain && !(lab.dbg & 8);

  // ---- fp64: the family ----
  // four C blocks per wave, one per MFMA sub-block; order[] is padded to a multiple of 4 per XCD stream, so a wave's
  // four positions never straddle two streams only if the stream length is a multiple of 16: the tail positions hold -1
  if (sw.use_tiny && f.max_m <= 4 && f.max_n <= 4 && f.no_empty_dim()) return pick(Family::f64_tiny, (unsigned)((npos + 15) / 16), skip, "mm_numeric_f64_tiny");
  if (small8) {
    // C blocks per wave (DBCSR_AMD_MM_SMALL_G; 0 = by the list length): with one or two products per C block a wave lives for a microsecond and the launch is
    // bound by the rate at which waves start (5 x 5 blocks at 1 % fill, 14 M C blocks: 4.96 ms with one block per wave, 4.2 with eight); with fourteen it is not
    c.group = sw.small_group > 0 ? sw.small_group : (f.nproducts < 4 * nblk ? 8 : 1);
    c.depth = sw.use_small == 3 || sw.use_small == 4 || sw.use_small == 6 || sw.use_small == 8 ? sw.use_small : 2;
    return pick(Family::f64_small8, (unsigned)((npos + 4 * (int64_t)c.group - 1) / (4 * (int64_t)c.group)), skip, "mm_numeric_f64_small<%d>", c.depth);
  }
  if (c.mid_rb) {
    // blocks of 25 ... 40 in both dimensions: one wave per C block, operands in slabs (mm_numeric_f64_mid.h); the dominant size (else the largest)
    // multiplied exactly, the blocks of another size by the second launch.  Every block leaves its norm to a filtered multiply (round 6, session 56).
    return pick(Family::f64_mid, per_block, skip, "mm_numeric_f64_mid<%d,%d>", c.mid_rb, c.mid_cb);
  }
  if (!(small && sw.use_lds)) {
    // blocks of 33 ... 80 (or an inner dimension above 32): one workgroup per C block, operand slabs shared through LDS (mm_numeric_f64_big.h)
    if (sw.use_big && sw.use_lds && f.max_m <= 80 && f.max_n <= 80 && f.no_empty_dim() && !f.cls_mode && f.order_len > 0 &&
        (f.max_m > 32 || f.max_n > 32 || ((f.max_m + 7) / 8) * ((f.max_n + 7) / 8) >= 4) && big_f64_has(big_tiles(f.max_m), big_tiles(f.max_n)))
      return pick(Family::f64_big, per_block, skip | (sw.use_big == 2 ? 4 : 0), "mm_numeric_f64_big<%d,%d>", big_tiles(f.max_m), big_tiles(f.max_n));
    return pick(Family::f64_generic, quads, skip, "mm_numeric_f64");
  }
  // Blocks of at most 32, whole blocks staged in a per-wave LDS slice.  Staging writes whole 1 KiB chunks (128 doubles), A's chunks first, then B's: the B
  // part may start right after A's (zero-padded) block -- the tail of A's last chunk is simply overwritten by B's first chunk
  // (one wave, in-order LDS queue) -- and only B's part is rounded up to whole chunks.  For 23x23 blocks this is
  // 9.5 KB per wave instead of 10 KB, which is what lets a 4th workgroup (16 waves) fit the CU's 160 KB.
  int lds_b = ((f.max_k * f.max_n + 127) / 128) * 128;
  c.lds_a = (f.max_m * ((f.max_k + 3) & ~3) + 1) & ~1;
  if (!f.cls_mode && f.dominant_cube() && hm % 8 == 0) {
    // the exact-size kernel stages columns of 16 / 32 doubles (B: 24 too) with a pitch of + 2 (mm_numeric_f64.h: cblock_f64_exact): its A image has
    // hot_m + 2 rows per column, its B image 16 more bytes per column (128 per KiB piece at most)
    if (hm % 16 == 0) c.lds_a = std::max(c.lds_a, (hm + 2) * hm);
    lds_b = std::max(lds_b, ((hm * hm * 8 + 1023) / 1024) * (1024 + 128) / 8 + 2);
  }
  c.lds_wave = c.lds_a + lds_b;
  c.maxt = std::min(4, (std::max(f.max_m, f.max_n) + 7) / 8);
  const size_t wave_bytes = (size_t)c.lds_wave * sizeof(double);
  c.lds_bytes = c.ww * wave_bytes + (size_t)lab.lds_pad;   // one wave per C block: ww waves per workgroup, each with its LDS slice
  const unsigned lds_grid = (unsigned)(npos / 4) * 4u / (unsigned)c.ww;
  if (f.cls_mode) {
    // one launch per (m, n) class on its segment of order[]: the run-time compiled exact-size kernel of the class
    // (mm_exact.h, mm_jit.hip), the generic LDS kernel for class 9 (other sizes) and for classes hiprtc could not serve;
    // classes of 29 ... 32 rows and columns, or 21 ... 24 in one of them (DBCSR_AMD_MM_MID=3: not those): the one-wave slab kernel -- half the LDS of
    // the class kernel, which stages whole blocks (17.9 KB per wave for (32, 32), 15 KB for (32, 23): two waves per SIMD)
    c.lds_bytes = c.ww * wave_bytes;
    c.mid_class_mode = (sw.use_mid && sw.use_big && lab.class_g == 1) ? (sw.use_mid == 3 ? 3 : 1) : 0;
    return pick(Family::f64_classes, lds_grid, dbg_flags, "mm_numeric_f64_class[");
  }
  // lab: a wave per R C blocks of one block column, B shared inside the wave (mm_group64.h): one dominant cube size the kernel is built for, no
  // block norms to leave behind (filtered multiplies), no symmetric product.  Its launch for the C blocks of other sizes is told to leave the dominant
  // size alone (64), as is the one after the tile / band kernels.
  const bool plain_cube = c.work && hot_allowed && lab.dma_stages == 0 && f.dominant_cube() && !c.norms && !f.canonical_c && !(lab.dbg & ~32);
  c.group_R = lab.f64_group;
  if (lab.f64_group >= 2 && plain_cube && !lab.hot_persistent)
    return pick(Family::f64_group, per_wave, 64 | (skip ? 32 : 0), "mm_numeric_f64_group<%d,%d,%d;%d>", hm, hn, hk, c.group_R);
  // lab: XCD-wide C tiles (mm_tile.h) / CU-wide C tiles, B shared in LDS (mm_band.h): 23^3, a C dense enough that sub-tiles of 3 x 3 blocks have long
  // product lists, no on-the-fly filter, no in-place accumulation; band: and no retain_sparsity (its lists take C's pattern from the operands)
  const bool tiles_ok = plain_cube && hm == 23 && !f.filter_active && !skip, dense = f.nproducts >= 8 * nblk && nblk >= 200000;
  if (lab.use_tile > 0 && tiles_ok && (lab.use_tile > 1 || dense)) return pick(Family::f64_tile, per_wave, 64, "mm_numeric_f64_tile<%d,%d,%d>", hm, hn, hk);
  if (lab.use_band > 0 && tiles_ok && !f.retain && !lab.hot_persistent && (lab.use_band > 1 || dense))
    return pick(Family::f64_band, per_wave, 64, "mm_numeric_f64_band<%d,%d,%d>", hm, hn, hk);
  if (hot_allowed && lab.dma_stages > 0 && dma_f64_has(lab.dma_stages, hm, hn, hk))
    return pick(Family::f64_dma, per_block, skip, "mm_numeric_f64_dma<%d,%d,%d,%d>", hm, hn, hk, lab.dma_stages);
  if (lab.hot_persistent && hot_allowed && f.dominant_cube() && hm == 23 && c.work && !(lab.dbg & ~32)) {
    // persistent waves, one counter per XCD (an experiment: see the kernel); 16 one-wave workgroups per CU is what the LDS slice allows
    c.lds_bytes = wave_bytes + (size_t)lab.lds_pad;
    return pick(Family::f64_persistent, 0, skip ? 32 : 0, "mm_numeric_f64_hot_persistent<%d,%d,%d>", hm, hn, hk);
  }
  // C blocks of the dominant size take the exact-size path, the others the generic one; both leave their norms
  c.variant = (lab.dbg & ~32) ? 1 : lab.hot_variant;
  if (hot_allowed && hot_f64_has(hm, hn, hk)) return pick(Family::f64_hot, per_wave, dbg_flags, "mm_numeric_f64_hot<%d,%d,%d>", hm, hn, hk);
  // measured: the pipelined kernel wins when C blocks have few products (config 3: 3.7 per block, 10.4 vs 11.8 ms) and
  // loses when they have many (config 2: 14.4 per block, 32 vs 22 ms)
  if (sw.use_pipe == 1 || (sw.use_pipe < 0 && f.nproducts < 6 * nblk && f.nproducts > nblk + nblk / 2)) {
    c.group = sw.pipe_g;
    c.lds_bytes = 4 * wave_bytes + (size_t)lab.lds_pad;
    return pick(Family::f64_pipe, (unsigned)((npos + 4 * (int64_t)c.group - 1) / (4 * (int64_t)c.group)), skip, "mm_numeric_f64_pipe<%d>", c.maxt);
  }
  return pick(Family::f64_lds, lds_grid, dbg_flags, "mm_numeric_f64_lds<%d>", c.maxt);
}

// ---- the symbolic phase's choices ------------------------------------------------------------------------------------------------------------------------------
// Which kernels build C's pattern, count and list the block products, and how C is cut into column panels: pure functions of the block counts, the forced
// mode and the panel size (tests/test_symbolic_scale_cpu.py).  The number of C blocks is known only after the pattern kernels ran, so the choice comes in
// two steps: choose_symbolic_pattern before, choose_symbolic_count after.  dbcsr_amd_mm_last_symbolic reports what they chose.
struct SymbolicSizes {
  int nbr = 0, nbk = 0, nbc = 0;        // block rows of A / C, inner blocks, block columns of B / C
  int64_t a_nblks = 0, b_nblks = 0;
  bool filtering = false, retain = false;
  int forced = 0;                       // DBCSR_AMD_MM_SYMBOLIC: 0 automatic, 1 word, 2 grid, 3 rows
};

struct SymbolicChoice {
  bool sparse_guess = false;            // fewer products expected than 60 % of the (row, column) candidates, enough block rows to fill the chip
  bool bitmap_rows = false;             // C's pattern under the on-the-fly filter by the product-driven kernel (c_bitmap_rows_filtered)
  bool grid_kernels = false, rows_kernels = false;   // count / fill: one lane per candidate, one wave per block row (neither: one thread per bitmap word)
};

// before C's pattern: expected number of products against the number of (row, column) candidates
static inline SymbolicChoice choose_symbolic_pattern(const SymbolicSizes& s) {
  SymbolicChoice c;
  const double prod_est = (double)s.a_nblks * ((double)s.b_nblks / (double)std::max(s.nbk, 1));
  c.sparse_guess = s.forced == 3 || (s.forced == 0 && s.nbr >= 2048 && prod_est < 0.6 * (double)s.nbr * (double)s.nbc);
  c.bitmap_rows = s.filtering && c.sparse_guess && !s.retain;
  return c;
}

// after C's pattern: one lane per (row, column) candidate unless C is extremely sparse (then one thread per bitmap word); a sparse C (less than 60 % of the
// candidates are blocks) with enough block rows to fill the chip: the product-driven kernels
static inline SymbolicChoice choose_symbolic_count(const SymbolicSizes& s, SymbolicChoice c, int64_t c_nblks) {
  const int nJ = (s.nbc + 63) / 64;
  c.grid_kernels = s.filtering || (((int64_t)s.nbr * nJ * 64 <= 256 * std::max<int64_t>(c_nblks, 1)) && s.forced != 1);
  c.rows_kernels = s.forced == 3 || (s.forced == 0 && s.nbr >= 2048 && 10 * c_nblks < 6 * (int64_t)s.nbr * s.nbc);
  if (c.rows_kernels) c.grid_kernels = false;
  return c;
}

// column panels of C sized so that B's panel stays in the Infinity Cache: NP panels of PW bitmap words (the last one may be narrower; W % PW need not be 0)
static inline void choose_panels(int W, int64_t b_bytes_est, int64_t panel_bytes, int* NP_out, int* PW_out) {
  int NP = (int)std::min<int64_t>((b_bytes_est + panel_bytes - 1) / panel_bytes, (int64_t)W);
  if (NP < 1) NP = 1;
  const int PW = (W + NP - 1) / NP;
  *NP_out = (W + PW - 1) / PW;
  *PW_out = PW;
}

// DBCSR_AMD_MM_PANEL_MB / DBCSR_AMD_MM_GROUP_PANEL_MB in bytes: at least 1 MB (choose_panels divides by it)
static inline int64_t panel_bytes_of_mb(long long mb) { return (int64_t)std::max<long long>(mb, 1) << 20; }

}  // namespace dbcsr_amd
#endif
