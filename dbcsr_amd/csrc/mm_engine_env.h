// mm_engine_env.h -- part of mm_engine.hip (included inside namespace dbcsr_amd, after struct Engine): every environment switch of the engine, read ONCE
// per engine, when it is created (dbcsr_amd_mm_create) -- nothing on the multiply path calls getenv.  Shipping build: the switches that select among
// kernels that ship (A / B measurements, tests that force a kernel family) -- those the numeric phase's choice reads land in E->sw (Switches, mm_choose.h),
// the plan / symbolic-phase ones in Engine itself; lab build: + the switches of the experimental dataflows -- E->lab (LabSwitches, mm_choose.h: what the
// choice reads) and E->ls (LabState: the knobs of the tile / band / group / persistent hosts).
#ifndef DBCSR_AMD_MM_ENGINE_ENV_H
#define DBCSR_AMD_MM_ENGINE_ENV_H

static void engine_read_env(Engine* E) {
  if (const char* k = getenv("DBCSR_AMD_MM_KERNEL")) {
    E->sw.use_lds = strcmp(k, "direct") != 0;
    E->sw.use_pipe = strcmp(k, "pipe") == 0 ? 1 : (strcmp(k, "lds1") == 0 ? 0 : -1);
#ifdef DBCSR_AMD_EXPERIMENTS
    if (strncmp(k, "dma", 3) == 0 && k[3] >= '2' && k[3] <= '4') E->lab.dma_stages = k[3] - '0';
#endif
  }
  if (const char* k = getenv("DBCSR_AMD_MM_PIPE_G")) E->sw.pipe_g = std::max(1, atoi(k));
  if (const char* k = getenv("DBCSR_AMD_MM_CLASSES")) E->sw.use_classes = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_WORK")) E->sw.use_work = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_WG_WAVES")) {
    const int w = atoi(k);
    if (w == 1 || w == 2 || w == 4) E->sw.wg_waves = w;
  }
  if (const char* k = getenv("DBCSR_AMD_MM_PLAN")) E->use_plan = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_HOT")) E->sw.use_hot = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_TINY")) E->sw.use_tiny = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_SMALL")) E->sw.use_small = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_SMALL_G")) E->sw.small_group = std::min(64, std::max(0, atoi(k)));
  if (const char* k = getenv("DBCSR_AMD_MM_F32_DIRECT")) E->sw.f32_direct = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_BIG")) E->sw.use_big = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_MID")) E->sw.use_mid = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_SYMBOLIC")) {
    E->force_symbolic = strcmp(k, "word") == 0 ? 1 : (strcmp(k, "grid") == 0 ? 2 : (strcmp(k, "rows") == 0 ? 3 : 0));
  }
  if (const char* k = getenv("DBCSR_AMD_MM_PANEL_MB")) E->panel_bytes = panel_bytes_of_mb(atoll(k));   // (at least 1 MB: choose_panels divides by it)
#ifdef DBCSR_AMD_EXPERIMENTS
  // ---- the lab build's switches (every one selects something that was measured and does not win; see the top of this file) ----
  if (const char* k = getenv("DBCSR_AMD_MM_F32_GROUP")) {
    const int r = atoi(k);
    E->lab.f32_group = (r >= 2 && r <= 4) ? r : (r < 0 ? -1 : 0);
  }
  if (const char* k = getenv("DBCSR_AMD_MM_F64_GROUP")) E->lab.f64_group = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_GROUP_PANEL_MB")) E->ls.group_panel_bytes = panel_bytes_of_mb(atoll(k));
  if (const char* k = getenv("DBCSR_AMD_MM_CLASS_G")) {
    const int g = atoi(k);
    E->lab.class_g = (g == 2 || g == 4 || g == 8) ? g : 1;
  }
  if (const char* k = getenv("DBCSR_AMD_MM_DBG")) E->lab.dbg = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_ALG_COLSUMS")) E->ls.alg_col_variant = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MULTIVEC_WAVES")) E->ls.multivec_waves = atoi(k);
  {
    const char* k = getenv("DBCSR_AMD_MM_POISON");  // (process-wide: the engines created from now on)
    g_devbuf_poison = k ? (atoi(k) & 255) : -1;
  }
  if (const char* k = getenv("DBCSR_AMD_MM_HOT_VARIANT")) E->lab.hot_variant = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_HOT_PERSISTENT")) E->lab.hot_persistent = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_HOT_XCDS")) E->ls.hot_xcd_mask = (unsigned)strtoul(k, nullptr, 0) & 0xffu;
  if (const char* k = getenv("DBCSR_AMD_MM_TILE")) E->lab.use_tile = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_TILE_WINDOW")) E->ls.tile_window = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_TILE_RDV")) E->ls.tile_rdv = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_TILE_PUB")) E->ls.tile_pub = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_TILE_PREFETCH")) E->ls.tile_prefetch = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_TILE_KNOBS")) E->ls.tile_knobs = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_TILE_SHAPE")) E->ls.tile_shape = atoi(k) == 1 ? 1 : 0;
  if (const char* k = getenv("DBCSR_AMD_MM_BAND")) E->lab.use_band = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_BAND_DEPTH")) E->ls.band_depth = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_BAND_BPOL")) E->ls.band_bpol = atoi(k) == 1 ? 1 : 0;
  if (const char* k = getenv("DBCSR_AMD_MM_BAND_KNOBS")) E->ls.band_knobs = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_BAND_WINDOW")) E->ls.band_window = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_BAND_SHAPE")) E->ls.band_shape = atoi(k) == 0 ? 0 : 1;
  if (const char* k = getenv("DBCSR_AMD_MM_LDS_PAD")) E->lab.lds_pad = atoi(k);
  if (const char* k = getenv("DBCSR_AMD_MM_CLASS_STREAMS")) E->lab.class_streams = std::min(4, std::max(1, atoi(k)));
  if (const char* k = getenv("DBCSR_AMD_MM_ROW_GROUP")) E->lab.row_group = atoi(k);
#endif
}

#endif
