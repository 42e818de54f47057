// mm_engine_lab.h -- part of mm_engine.hip, LAB build only (included inside namespace dbcsr_amd): host side of the experimental dataflows (group, tile,
// band kernels): built, parity-green, measured slower; DESIGN.md section 6.
#ifndef DBCSR_AMD_MM_ENGINE_LAB_H
#define DBCSR_AMD_MM_ENGINE_LAB_H

#ifdef DBCSR_AMD_EXPERIMENTS
// compute units of the current device (asked once), <= 0 on error
static int device_cu_count() {
  static int n_cu = 0;
  int dev = 0;
  if (n_cu == 0 && (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)) n_cu = 0;
  return n_cu;
}

// the group kernels read B's blocks in the order of its index: are the block offsets ascending?  (synchronises the stream)  < 0 on error
static int group_b_ascending(Engine* E, const dbcsr_amd_bcsr* b, hipStream_t st) {
  if (E->ls.group_flag.ensure(4)) return -1;
  ACC_CHECK(hipMemsetAsync(E->ls.group_flag.p, 0, sizeof(int), st));
  group_check_ascending(st, static_cast<const int64_t*>(b->blk_p), (int64_t)b->nblks, E->ls.group_flag.p);
  int* hflag = reinterpret_cast<int*>(E->host_scalars + 12);
  ACC_CHECK(hipMemcpyAsync(hflag, E->ls.group_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  ACC_CHECK(hipStreamSynchronize(st));
  return *hflag == 0;
}

// the group launches' geometry: B in column panels of about panel_bytes
static GroupGeom group_geom(int nbc, int ng, int ngx, int64_t b_bytes, int64_t panel_bytes) {
  GroupGeom G;
  G.nbc = nbc, G.ng = ng, G.ngx = ngx;
  const int np = (int)std::min<int64_t>(std::max<int64_t>(1, (b_bytes + panel_bytes - 1) / panel_bytes), (int64_t)nbc);
  G.pw = (nbc + np - 1) / np;
  G.np = (nbc + G.pw - 1) / G.pw;
  return G;
}

// fp32 group kernel: 0 = launched, 1 = does not apply here (the caller runs the one-wave-per-block kernel), < 0 = error
static int run_group_f32(Engine* E, const NumericArgs<float>& p, int R) {
  const hipStream_t st = p.st;
  const dbcsr_amd_bcsr *b = p.B, *c_out = p.C;
  const int S = E->facts.hot_m, nbr = E->facts.nbr, nbc = b->nblkcols;
  if (!(S == 16 || S == 24 || S == 32) || R < 2 || R > 4 || nbr <= 0 || nbc <= 0) return 1;
  const int ng = (nbr + R - 1) / R, ngx = (ng + 7) / 8;
  if ((int64_t)ngx * nbc >= (1ll << 30)) return 1;
  if (!(p.reuse && E->ls.group_built && E->ls.group_R == R)) {
    if (E->ls.groups.ensure((size_t)ng * nbc * R + 1)) return -1;
    const int asc = group_b_ascending(E, b, st);
    if (asc < 0) return -1;
    E->ls.b_monotone = asc == 1;
    E->ls.group_R = R;
    E->ls.group_built = true;
    if (E->ls.b_monotone) group_build_table(st, c_out->row_p, c_out->col_i, E->descs.p, nbr, nbc, R, S, E->ls.groups.p);
  }
  if (!E->ls.b_monotone) return 1;
  const GroupGeom G = group_geom(nbc, ng, ngx, (int64_t)b->nblks * S * S * (int64_t)sizeof(float), E->panel_bytes);
  const unsigned nwg = 8u * (unsigned)(((int64_t)ngx * nbc + 3) / 4);
  return group_f32_launch(S, R, nwg, st, p.descs, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, p.skip_empty, E->ls.groups.p, G);
}

// fp64 group kernel (mm_group64.h): 0 = launched, 1 = does not apply here (the caller runs the one-wave-per-block kernel), < 0 = error
static int run_group_f64(Engine* E, const NumericArgs<double>& p, int R) {
  const hipStream_t st = p.st;
  const dbcsr_amd_bcsr *b = p.B, *c_out = p.C;
  const int S = E->facts.hot_m, nbr = E->facts.nbr, nbc = b->nblkcols;
  if (!group64_has_kernel(S, R) || nbr <= 0 || nbc <= 0) return 1;
  const int ng = (nbr + R - 1) / R, ngx = (ng + 7) / 8;
  const int64_t ngj = (int64_t)ng * nbc;
  if ((int64_t)ngx * nbc >= (1ll << 28)) return 1;
  if (!(p.reuse && E->ls.group_built && E->ls.group_R == R)) {
    if (E->ls.groups.ensure((size_t)ngj * R + 1) || E->ls.group_cnt.ensure((size_t)ngj + 1) || E->ls.group_work.ensure((size_t)ngj + 1) ||
        E->ls.group_start.ensure((size_t)ngj + 2))
      return -1;
    const int asc = group_b_ascending(E, b, st);
    if (asc < 0) return -1;
    E->ls.b_monotone = asc == 1;
    E->ls.group_R = R;
    E->ls.group_built = true;
    if (E->ls.b_monotone) {
      // the merged lists hold at most as many records as there are products
      if (E->ls.group_entries.ensure((size_t)E->facts.nproducts + 4)) return -1;
      group_build_table(st, c_out->row_p, c_out->col_i, E->descs.p, nbr, nbc, R, S, E->ls.groups.p);
      group64_count(st, E->ls.groups.p, E->descs.p, ngj, R, E->ls.group_cnt.p);
      if (exclusive_scan<int64_t>(E, E->ls.group_cnt.p, ngj, E->ls.group_start.p, nullptr, true, st)) return -1;
      group64_merge(st, E->ls.groups.p, E->descs.p, E->entries.p, ngj, R, S, E->ls.group_start.p, E->ls.group_work.p, E->ls.group_entries.p);
    }
  }
  if (!E->ls.b_monotone) return 1;
  const GroupGeom G = group_geom(nbc, ng, ngx, (int64_t)b->nblks * S * S * (int64_t)sizeof(double),
                                 E->ls.group_panel_bytes > 0 ? E->ls.group_panel_bytes : E->panel_bytes);
  const int has_tail = (E->facts.min_k != E->facts.max_k || E->facts.max_k != S) ? 1 : 0;
  return group64_launch(S, R, st, p.descs, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, p.skip_empty, has_tail, E->ls.group_work.p,
                        E->ls.group_entries.p, G);
}

// Index work the tile and band dataflows share: bitmaps of A and of B transposed, A's row prefix, the block rows / columns of the dominant size S.
static int build_tile_index(Engine* E, const NumericArgs<double>& p, int S) {
  const dbcsr_amd_bcsr *a = p.A, *b = p.B;
  const int nbr = a->nblkrows, nbk = a->nblkcols, nbc = b->nblkcols, Wk = (nbk + 31) / 32;
  if (E->ls.a_bm.ensure((size_t)nbr * Wk + 1) || E->ls.a_pre.ensure((size_t)nbr * Wk + 1) || E->ls.bt_bm.ensure((size_t)nbc * Wk + 1) ||
      E->ls.tile_rows.ensure((size_t)nbr + 1) || E->ls.tile_cols.ensure((size_t)nbc + 1))
    return -1;
  ACC_CHECK(hipMemsetAsync(E->ls.a_bm.p, 0, sizeof(uint32_t) * (size_t)nbr * Wk, p.st));
  ACC_CHECK(hipMemsetAsync(E->ls.bt_bm.p, 0, sizeof(uint32_t) * (size_t)nbc * Wk, p.st));
  hipLaunchKernelGGL(bitmap_from_index, grid_for((int64_t)nbr * 64), dim3(256), 0, p.st, a->row_p, a->col_i, nbr, Wk, E->ls.a_bm.p);
  hipLaunchKernelGGL(row_prefix, grid_for((int64_t)nbr * 64), dim3(256), 0, p.st, E->ls.a_bm.p, nbr, Wk, E->ls.a_pre.p, (int*)nullptr);
  hipLaunchKernelGGL(tile_bitmap_transposed, grid_for((int64_t)nbk * 64), dim3(256), 0, p.st, b->row_p, b->col_i, nbk, Wk, E->ls.bt_bm.p);
  hipLaunchKernelGGL(tile_select, dim3(1), dim3(64), 0, p.st, a->row_blk_size, nbr, S, E->ls.tile_rows.p, nbr);
  hipLaunchKernelGGL(tile_select, dim3(1), dim3(64), 0, p.st, b->col_blk_size, nbc, S, E->ls.tile_cols.p, nbc);
  return 0;
}

// The tile dataflow (mm_tile.h) for the C blocks of the dominant size: index work (bitmaps of A and of B transposed, sub-tile
// descriptors, k-sorted product lists), the persistent tile kernel, the products with inner blocks of another size.  The caller
// then runs the exact-size kernel over the C blocks of the other sizes.  descs[] and C_out's index are already filled.
template <int S_>
static int run_tile_f64(Engine* E, const NumericArgs<double>& p) {
  const hipStream_t st = p.st;
  const dbcsr_amd_bcsr *a = p.A, *b = p.B, *c_out = p.C;
  const int nbk = a->nblkcols, W = E->W, Wk = (nbk + 31) / 32;
  const int n_cu = device_cu_count();
  if (n_cu <= 0) return -1;
  const int cu_per_xcd = std::min(32, std::max(2, n_cu / 8));
  TileGeom G;
  G.nfr = E->facts.hot_cnt_m;
  G.nfc = E->facts.hot_cnt_n;
  if (!tile_shape(E->ls.tile_shape, &G.tr, &G.tc, &G.wg_waves)) return 1;
  G.nTR = (G.nfr + G.tr - 1) / G.tr;
  G.nTC = (G.nfc + G.tc - 1) / G.tc;
  G.team_rows = std::max(1, cu_per_xcd * G.wg_waves / kTeamCols);
  G.nSR = (G.nTR + G.team_rows - 1) / G.team_rows;
  G.nSC = (G.nTC + kTeamCols - 1) / kTeamCols;
  G.nseq = (G.nSR * G.nSC + 7) / 8;
  G.kspan = nbk + 1;
  if ((int64_t)G.nseq * G.kspan >= 0x7ff00000ll) return 1;  // progress counter would overflow: not a tile case
  const int64_t nT = (int64_t)G.nTR * G.nTC;
  const bool reuse = E->plan_hit && E->plan_numeric && E->ls.tile_built;
  if (E->ls.tile_prog.ensure(8 * 256) || E->ls.tile_flags.ensure(4)) return -1;
  ACC_CHECK(hipMemsetAsync(E->ls.tile_prog.p, 0, sizeof(uint32_t) * 8 * 256, st));
  ACC_CHECK(hipMemsetAsync(E->ls.tile_flags.p, 0, sizeof(int) * 4, st));
  if (!reuse) {
  if (build_tile_index(E, p, S_) || E->ls.tdescs.ensure((size_t)nT + 1) || E->ls.tile_cnt.ensure((size_t)nT + 1) || E->ls.tile_start.ensure((size_t)nT + 1) ||
      E->ls.tentries.ensure((size_t)E->facts.nproducts + 1))
    return -1;
  hipLaunchKernelGGL(tile_descs, grid_for(nT * 16), dim3(256), 0, st, G, E->ls.tile_rows.p, E->ls.tile_cols.p, E->c_bm.p, E->c_pre.p, c_out->row_p, W,
                     E->descs.p, E->ls.tdescs.p, E->ls.tile_cnt.p);
  if (exclusive_scan<int64_t>(E, E->ls.tile_cnt.p, nT, E->ls.tile_start.p, nullptr, false, st)) return -1;
  hipLaunchKernelGGL(tile_lists, grid_for(nT * 64), dim3(256), 0, st, G, E->ls.tile_rows.p, E->ls.tile_cols.p, nbk, Wk, E->ls.a_bm.p, E->ls.a_pre.p, a->row_p,
                     a->blk_p, E->ls.bt_bm.p, W, E->b_bm.p, E->b_pre.p, b->row_p, b->blk_p, a->col_blk_size, S_, E->ls.tile_start.p, E->ls.tile_cnt.p,
                     E->ls.tdescs.p, E->ls.tentries.p, E->ls.tile_flags.p + 1);
  E->ls.tile_built = true;
  }
  TileArgs P;
  P.tdescs = E->ls.tdescs.p;
  P.entries = E->ls.tentries.p;
  P.a_data = p.a;
  P.b_data = p.b;
  P.c_out = p.c_out;
  P.c_in = p.c_in;
  P.alpha = p.alpha;
  P.beta = p.beta;
  P.prog = E->ls.tile_prog.p;
  P.flags = E->ls.tile_flags.p;
  P.G = G;
  P.window = E->ls.tile_window;
  P.pub_policy = E->ls.tile_pub;
  P.prefetch = E->ls.tile_prefetch;
  P.knobs = E->ls.tile_knobs;
  P.times = nullptr;
  if (E->ls.tile_knobs & 32) {
    if (E->ls.tile_times.ensure(8)) return -1;
    ACC_CHECK(hipMemsetAsync(E->ls.tile_times.p, 0, 8 * sizeof(unsigned long long), st));
    P.times = E->ls.tile_times.p;
  }
  ACC_CHECK(hipEventRecord(E->ev[1], st));  // the timed numeric launch starts here (the index work above counts as fill time)
  if (tile_launch(S_, S_, S_, E->ls.tile_rdv, E->ls.tile_shape, (unsigned)(8 * cu_per_xcd), st, P)) return -1;
  if (tile_launch_remainder(S_, S_, st, G, E->ls.tdescs.p, E->ls.tentries.p, P.a_data, P.b_data, P.c_out, p.alpha)) return -1;
  return check(hipGetLastError(), "run_tile_f64", __FILE__, __LINE__);
}

// The band dataflow (mm_band.h) for the C blocks of the dominant size: bitmaps of A and of B transposed, sub-tile descriptors, the
// product lists in sweep order (count, scan, fill), the persistent kernel, the products with inner blocks of another size.  The
// caller then runs the exact-size kernel over the C blocks of the other sizes.  descs[] and C_out's index are already filled.
template <int S_>
static int run_band_f64(Engine* E, const NumericArgs<double>& p) {
  const hipStream_t st = p.st;
  const dbcsr_amd_bcsr *a = p.A, *b = p.B, *c_out = p.C;
  const int nbk = a->nblkcols, W = E->W, Wk = (nbk + 31) / 32;
  const int n_cu = device_cu_count();
  if (n_cu <= 0) return -1;
  if (band_lds_bytes(S_, S_, S_, E->ls.band_shape, E->ls.band_depth) == 0) return 1;
  BandGeom G;
  G.nfr = E->facts.hot_cnt_m;
  G.nfc = E->facts.hot_cnt_n;
  if (G.nfr <= 0 || G.nfc <= 0 || !band_shape(E->ls.band_shape, &G.waves, &G.tr, &G.tc)) return 1;
  G.nBR = (G.nfr + G.waves * G.tr - 1) / (G.waves * G.tr);
  G.nBC = (G.nfc + G.tc - 1) / G.tc;
  if ((int64_t)G.nBR * G.nBC > 0x3fffffff) return 1;
  G.ntiles = G.nBR * G.nBC;
  G.cu_per_xcd = std::min(32, std::max(1, n_cu / 8));
  G.max_i = 1;
  for (int x = 0; x < 8; ++x) G.max_i = std::max(G.max_i, (int)((G.lo(x + 1) - G.lo(x) + G.cu_per_xcd - 1) / G.cu_per_xcd));
  G.kshift = 0;
  while ((nbk >> G.kshift) >= 4096) ++G.kshift;
  G.kspan = (nbk >> G.kshift) + 1;
  if ((int64_t)(G.max_i + 1) * G.kspan >= 0x7ff00000ll) return 1;  // sweep positions would overflow: not a band case
  const int nwg = 8 * G.cu_per_xcd;
  const int64_t nsub = (int64_t)G.waves * G.ntiles, npl = (int64_t)nwg * G.waves * G.max_i, nps = (int64_t)nwg * G.max_i;
  const bool reuse = E->plan_hit && E->plan_numeric && E->ls.band_built && E->ls.band_geom.waves == G.waves && E->ls.band_geom.ntiles == G.ntiles;
  if (E->ls.band_flags.ensure(4) || E->ls.band_prog.ensure(8 * 512)) return -1;
  ACC_CHECK(hipMemsetAsync(E->ls.band_flags.p, 0, sizeof(int) * 4, st));
  ACC_CHECK(hipMemsetAsync(E->ls.band_prog.p, 0, sizeof(unsigned) * 8 * 512, st));
  if (!reuse) {
    E->ls.band_built = false;
    if (build_tile_index(E, p, S_) || E->ls.band_descs_buf.ensure((size_t)nsub + 1) || E->ls.band_sub_cnt.ensure((size_t)nsub + 1) ||
        E->ls.band_cnt_rem.ensure((size_t)nsub + 1) || E->ls.band_rem_start.ensure((size_t)nsub + 2) || E->ls.band_cnt_list.ensure((size_t)npl + 1) ||
        E->ls.band_list_off.ensure((size_t)npl + 2) || E->ls.band_cnt_b.ensure((size_t)nps + 1) || E->ls.band_seq_off.ensure((size_t)nps + 2))
      return -1;
    ACC_CHECK(hipMemsetAsync(E->ls.band_cnt_list.p, 0, sizeof(int) * (size_t)npl, st));
    ACC_CHECK(hipMemsetAsync(E->ls.band_cnt_b.p, 0, sizeof(int) * (size_t)nps, st));
    hipLaunchKernelGGL(band_descs, grid_for(nsub * 16), dim3(256), 0, st, G, E->ls.tile_rows.p, E->ls.tile_cols.p, E->c_bm.p, E->c_pre.p, c_out->row_p, W,
                       E->descs.p, E->ls.band_descs_buf.p, E->ls.band_sub_cnt.p);
    hipLaunchKernelGGL((band_lists<false>), grid_for(nsub * 64), dim3(256), 0, st, G, E->ls.tile_rows.p, E->ls.tile_cols.p, nbk, Wk, E->ls.a_bm.p, E->ls.a_pre.p,
                       a->row_p, a->blk_p, E->ls.bt_bm.p, W, E->b_bm.p, E->b_pre.p, b->row_p, b->blk_p, a->col_blk_size, S_, E->ls.band_cnt_list.p,
                       E->ls.band_cnt_b.p, E->ls.band_cnt_rem.p, (const int64_t*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr,
                       E->ls.band_sub_cnt.p, (BandEntry*)nullptr, (BandRem*)nullptr, E->ls.band_flags.p + 1);
    if (exclusive_scan<int64_t>(E, E->ls.band_cnt_list.p, npl, E->ls.band_list_off.p, nullptr, true, st)) return -1;
    if (exclusive_scan<int64_t>(E, E->ls.band_cnt_b.p, nps, E->ls.band_seq_off.p, nullptr, true, st)) return -1;
    if (exclusive_scan<int64_t>(E, E->ls.band_cnt_rem.p, nsub, E->ls.band_rem_start.p, nullptr, true, st)) return -1;
    hipLaunchKernelGGL(band_max_seq, grid_for(nwg), dim3(256), 0, st, G, nwg, E->ls.band_seq_off.p, E->ls.band_flags.p + 2);
    // list sizes to the host (once per plan: a multiply that reuses the plan comes nowhere near this)
    ACC_CHECK(hipMemcpyAsync(E->host_scalars + 8, E->ls.band_list_off.p + npl, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipMemcpyAsync(E->host_scalars + 9, E->ls.band_rem_start.p + nsub, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipMemcpyAsync(E->host_scalars + 10, E->ls.band_flags.p + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    ACC_CHECK(hipStreamSynchronize(st));
    E->ls.band_nlist = E->host_scalars[8];
    E->ls.band_nrem = E->host_scalars[9];
    const int max_seq = *reinterpret_cast<const int*>(E->host_scalars + 10);
    if (max_seq >= (1 << 23) - 64) return 1;  // the entries carry 23 bits of the sequence number: not a band case
    if (E->ls.band_entries.ensure((size_t)E->ls.band_nlist + 1) || E->ls.band_rem.ensure((size_t)E->ls.band_nrem + 1)) return -1;
    hipLaunchKernelGGL((band_lists<true>), grid_for(nsub * 64), dim3(256), 0, st, G, E->ls.tile_rows.p, E->ls.tile_cols.p, nbk, Wk, E->ls.a_bm.p, E->ls.a_pre.p,
                       a->row_p, a->blk_p, E->ls.bt_bm.p, W, E->b_bm.p, E->b_pre.p, b->row_p, b->blk_p, a->col_blk_size, S_, (int*)nullptr,
                       (int*)nullptr, (int*)nullptr, E->ls.band_list_off.p, E->ls.band_seq_off.p, E->ls.band_rem_start.p, E->ls.band_sub_cnt.p,
                       E->ls.band_entries.p, E->ls.band_rem.p, E->ls.band_flags.p + 1);
    E->ls.band_geom = G;
    E->ls.band_built = true;
  }
  BandArgs P;
  P.descs = E->ls.band_descs_buf.p;
  P.entries = E->ls.band_entries.p;
  P.list_off = E->ls.band_list_off.p;
  P.a_data = p.a;
  P.b_data = p.b;
  P.c_out = p.c_out;
  P.c_in = p.c_in;
  P.alpha = p.alpha;
  P.beta = p.beta;
  P.G = G;
  P.flags = E->ls.band_flags.p;
  P.prog = E->ls.band_prog.p;
  P.window = E->ls.band_window > 0 ? std::max(1, E->ls.band_window >> G.kshift) : 0;
  P.knobs = E->ls.band_knobs;
  P.times = nullptr;
  if (E->ls.band_knobs & 1) {
    if (E->ls.band_times.ensure(16)) return -1;
    ACC_CHECK(hipMemsetAsync(E->ls.band_times.p, 0, 16 * sizeof(unsigned long long), st));
    P.times = E->ls.band_times.p;
  }
  ACC_CHECK(hipEventRecord(E->ev[1], st));  // the timed numeric launch starts here (the index work above counts as fill time)
  if (band_launch(S_, S_, S_, E->ls.band_shape, E->ls.band_depth, E->ls.band_bpol, (unsigned)nwg, st, P)) return -1;
  if (E->ls.band_nrem > 0 &&
      band_launch_remainder(S_, S_, st, nsub, E->ls.band_descs_buf.p, E->ls.band_rem_start.p, E->ls.band_rem.p, P.a_data, P.b_data, P.c_out, p.alpha))
    return -1;
  return check(hipGetLastError(), "run_band_f64", __FILE__, __LINE__);
}
// persistent waves, one counter per XCD (an experiment: see the kernel); 16 one-wave workgroups per CU is what the LDS slice allows
static int run_persistent_f64(Engine* E, const NumericArgs<double>& p, const NumericChoice& c) {
  const int n_cu_p = device_cu_count();
  if (n_cu_p <= 0 || E->ls.hot_counters.ensure(8 * 32)) return -1;
  const int per_cu = std::max(1, (int)((160 * 1024) / c.lds_bytes));
  ACC_CHECK(hipMemsetAsync(E->ls.hot_counters.p, 0, 8 * 32 * sizeof(unsigned), p.st));
  hipLaunchKernelGGL((mm_numeric_f64_hot_persistent<23, 23, 23>), dim3((unsigned)(n_cu_p * per_cu)), dim3(64), c.lds_bytes, p.st, p.entries, p.a, p.b, p.c_out,
                     p.c_in, p.alpha, p.beta, c.lds_a, c.flags, p.work, (long)E->facts.order_len, E->ls.hot_counters.p, E->ls.hot_xcd_mask, p.norms);
  if (p.norms)
    hipLaunchKernelGGL(block_norms_other_sizes, grid_for(p.nblk * 64), dim3(256), 0, p.st, p.descs, p.nblk, p.c_out, E->facts.hot_m, E->facts.hot_n, p.norms);
  return 0;
}

static int launch_f64(Engine* E, const NumericChoice& c, const NumericArgs<double>& p, const LabSwitches& lab);   // (mm_engine.hip)

// The lab families of the numeric phase (0 = launched, < 0 = error).  After group / tile / band: the exact-size kernel over the C blocks of the other
// sizes (tail block row / column), told to leave the dominant size alone (c.flags); tile / band computed the products with inner blocks of another size
// themselves.  A dataflow that does not apply to this multiply after all (its host returns 1: B's blocks not in ascending order, counters that would
// overflow ...) is struck from `lab` and the choice made again: the next family in the order takes the multiply (work records and norms do not
// depend on those switches).
static int launch_lab_f64(Engine* E, const NumericChoice& c, const NumericArgs<double>& p, LabSwitches lab) {
  const SizeFacts& F = E->facts;
  if (c.family == Family::f64_dma) return launch_dma_f64(p, c, lab.dma_stages, F.hot_m, F.hot_n, F.hot_k) ? 0 : -1;
  if (c.family == Family::f64_persistent) return run_persistent_f64(E, p, c);
  const int rc = c.family == Family::f64_group ? run_group_f64(E, p, c.group_R) : c.family == Family::f64_tile ? run_tile_f64<23>(E, p) : run_band_f64<23>(E, p);
  if (rc == 0 && (c.family != Family::f64_group || F.other_sizes())) launch_hot_f64(p, c, F.hot_m, F.hot_n, F.hot_k, c.flags, 0);
  if (rc != 1) return rc;
  (c.family == Family::f64_group ? lab.f64_group : c.family == Family::f64_tile ? lab.use_tile : lab.use_band) = 0;
  return launch_f64(E, choose_numeric(F, E->sw, lab), p, lab);
}
#endif  // DBCSR_AMD_EXPERIMENTS

#endif
