// mm_engine_launch.h -- part of mm_engine.hip (one translation unit; included inside namespace dbcsr_amd): the table of exact-size kernel instantiations,
// the norm kernels beside them and the launch dispatchers (block size -> template instance) of the numeric kernels.
#ifndef DBCSR_AMD_MM_ENGINE_LAUNCH_H
#define DBCSR_AMD_MM_ENGINE_LAUNCH_H

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
// (the instance lists -- DBCSR_AMD_HOT_SIZES and their like -- and the predicates that answer for them are in mm_choose.h)

// one wave per C block, only the blocks that are NOT m x n: their squared Frobenius norm (the exact-size kernel wrote the others')
__global__ void __launch_bounds__(256) block_norms_other_sizes(const Desc* __restrict__ descs, int64_t nblk, const double* __restrict__ c_data,
                                                               int m, int n, double* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t cb = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (cb >= nblk) return;
  const Desc d = descs[cb];
  if (d.m == m && d.n == n) return;
  const double* x = c_data + d.c_off;
  double ss = 0.0;
  for (int e = lane; e < d.m * d.n; e += 64) ss += x[e] * x[e];
  ss = wave_sum(ss);
  if (lane == 0) norms[cb] = ss;
}

// the same for a multiply of mixed sizes: the blocks whose (m, n) class had no run-time compiled kernel (class 9 = other sizes, or hiprtc failed)
struct ClassSet {
  int m[3], n[3], jit_mask;
};
__global__ void __launch_bounds__(256) block_norms_unserved_classes(const Desc* __restrict__ descs, int64_t nblk, const double* __restrict__ c_data,
                                                                    ClassSet cs, double* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t cb = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (cb >= nblk) return;
  const Desc d = descs[cb];
  int rm = 3, rn = 3;
#pragma unroll
  for (int q = 2; q >= 0; --q) {
    if (cs.m[q] > 0 && d.m == cs.m[q]) rm = q;
    if (cs.n[q] > 0 && d.n == cs.n[q]) rn = q;
  }
  if (rm < 3 && rn < 3 && ((cs.jit_mask >> (3 * rm + rn)) & 1)) return;  // its class kernel wrote the norm
  const double* x = c_data + d.c_off;
  double ss = 0.0;
  for (int e = lane; e < d.m * d.n; e += 64) ss += x[e] * x[e];
  ss = wave_sum(ss);
  if (lane == 0) norms[cb] = ss;
}

// Every launcher takes the call's operands (NumericArgs, mm_mid.h) and its geometry, mostly as the NumericChoice made (mm_choose.h); each returns false
// when it has no instance for the sizes -- the choice asked the predicate beside the instance list first, so for the caller that is an error.

// exact-size kernel: flags / variant are the caller's (the launches that leave the dominant size alone pass their own)
static bool launch_hot_f64(const NumericArgs<double>& p, const NumericChoice& c, int m, int n, int k, int flags, int variant) {
  if (!hot_f64_has(m, n, k)) return false;
  const dim3 grid(c.grid), block(64 * c.ww);
#ifdef DBCSR_AMD_EXPERIMENTS
  // profiling variants exist for the benchmark's block size only (ablation switches; unpaired fragment reads)
  if (m == 23 && variant >= 1 && variant <= 6) {
    auto kern = variant == 1 ? mm_numeric_f64_hot<23, 23, 23, 1> : variant == 2 ? mm_numeric_f64_hot<23, 23, 23, 2> : variant == 3 ? mm_numeric_f64_hot<23, 23, 23, 3> :
                variant == 4 ? mm_numeric_f64_hot<23, 23, 23, 4> : variant == 5 ? mm_numeric_f64_hot<23, 23, 23, 5> : mm_numeric_f64_hot<23, 23, 23, 6>;
    hipLaunchKernelGGL(kern, grid, block, c.lds_bytes, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.lds_a, c.lds_wave, flags,
                       p.order, p.work, p.norms);
    return true;
  }
#else
  (void)variant;
#endif
  switch (m) {
#define DBCSR_HOT_CASE(S_)                                                                                                                          \
  case S_:                                                                                                                                          \
    hipLaunchKernelGGL((mm_numeric_f64_hot<S_, S_, S_, 0>), grid, block, c.lds_bytes, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in,  \
                       p.alpha, p.beta, c.lds_a, c.lds_wave, flags, p.order, p.work, p.norms);                                                     \
    return true;
    DBCSR_AMD_HOT_SIZES(DBCSR_HOT_CASE)
#undef DBCSR_HOT_CASE
    default: return false;
  }
}

#ifdef DBCSR_AMD_EXPERIMENTS
// LDS-DMA variant of the exact-size kernel (mm_dma.h): S ring slots per wave, one wave per workgroup
static bool launch_dma_f64(const NumericArgs<double>& p, const NumericChoice& c, int S, int m, int n, int k) {
  if (!dma_f64_has(S, m, n, k)) return false;
  switch (S * 64 + m) {
#define DBCSR_DMA_CASE(R_, S_)                                                                                                               \
  case R_ * 64 + S_:                                                                                                                          \
    hipLaunchKernelGGL((mm_numeric_f64_dma<S_, S_, S_, R_>), dim3(c.grid), dim3(64), (DmaRing<S_, S_, S_, R_>::BYTES), p.st, p.descs, p.nblk, \
                       p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.flags, p.order);                                              \
    return true;
#define DBCSR_DMA_RINGS(S_) DBCSR_DMA_CASE(2, S_) DBCSR_DMA_CASE(3, S_) DBCSR_DMA_CASE(4, S_)
    DBCSR_AMD_DMA_SIZES(DBCSR_DMA_RINGS)
#undef DBCSR_DMA_RINGS
#undef DBCSR_DMA_CASE
    default: return false;
  }
}
#endif

static bool launch_hot_f32(const NumericArgs<float>& p, const NumericChoice& c, int m, int n, int k) {
  if (!hot_f64_has(m, n, k)) return false;   // (the same cubes as fp64)
  switch (m) {
#define DBCSR_HOT_CASE(S_)                                                                                                                          \
  case S_:                                                                                                                                          \
    hipLaunchKernelGGL((mm_numeric_f32_hot<S_, S_, S_>), dim3(c.grid), dim3(64 * c.ww), f32_lds_bytes(c.ww), p.st, p.descs, p.nblk, p.entries, p.a, \
                       p.b, p.c_out, p.c_in, p.alpha, p.beta, c.flags, p.order);                                                                    \
    return true;
    DBCSR_AMD_HOT_SIZES(DBCSR_HOT_CASE)
#undef DBCSR_HOT_CASE
    default: return false;
  }
}

// the direct form of the fp32 exact-size kernel (mm_numeric_f32.h, round 5): cubes whose k is a multiple of 8
static bool launch_hot_f32_direct(const NumericArgs<float>& p, const NumericChoice& c, int m, int n, int k, int flags, bool slim) {
  if (!f32_direct_has(m, n, k)) return false;
  switch (m) {   // slim: every C block has the dominant size, LDS for the B images only
#define DBCSR_DIRECT_CASE(S_)                                                                                                                      \
  case S_:                                                                                                                                         \
    hipLaunchKernelGGL((slim ? mm_numeric_f32_direct_slim<S_, S_, S_> : mm_numeric_f32_direct<S_, S_, S_>), dim3(c.grid), dim3(64 * c.ww),         \
                       slim ? (size_t)c.ww * f32d_wave_floats(S_) * sizeof(float) : f32_lds_bytes(c.ww), p.st, p.descs, p.nblk, p.entries, p.a, p.b, \
                       p.c_out, p.c_in, p.alpha, p.beta, flags, p.order);                                                                          \
    return true;
    DBCSR_AMD_F32_DIRECT_SIZES(DBCSR_DIRECT_CASE)
#undef DBCSR_DIRECT_CASE
    default: return false;
  }
}

// fp32, any sizes up to 32, on the positions of `p.order` that `grid` workgroups of c.ww waves cover
static void launch_lds_f32(const NumericArgs<float>& p, const NumericChoice& c, unsigned grid) {
  hipLaunchKernelGGL(mm_numeric_f32_lds, dim3(grid), dim3(64 * c.ww), f32_lds_bytes(c.ww), p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in,
                     p.alpha, p.beta, c.flags, p.order);
}

// blocks of 33 ... 80: sub-blocks of TM x TN tiles per wave, 2 x 2 waves per C block (mm_numeric_f64_big.h)
static bool launch_big_f64(const NumericArgs<double>& p, const NumericChoice& c, int tm, int tn) {
  if (!big_f64_has(tm, tn) || c.grid == 0) return false;
  switch (tm * 8 + tn) {
#define DBCSR_BIG_CASE(A_, B_)                                                                                                                  \
  case A_ * 8 + B_:                                                                                                                             \
    hipLaunchKernelGGL((mm_numeric_f64_big<A_, B_>), dim3(c.grid), dim3(256), (size_t)big_lds_bytes(A_, B_), p.st, p.descs, p.nblk, p.entries,  \
                       p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.flags, p.order);                                                           \
    return true;
    DBCSR_BIG_CASE(2, 2) DBCSR_BIG_CASE(2, 3) DBCSR_BIG_CASE(2, 4) DBCSR_BIG_CASE(2, 5)
    DBCSR_BIG_CASE(3, 2) DBCSR_BIG_CASE(3, 3) DBCSR_BIG_CASE(3, 4) DBCSR_BIG_CASE(3, 5)
    DBCSR_BIG_CASE(4, 2) DBCSR_BIG_CASE(4, 3) DBCSR_BIG_CASE(4, 4) DBCSR_BIG_CASE(4, 5)
    DBCSR_BIG_CASE(5, 2) DBCSR_BIG_CASE(5, 3) DBCSR_BIG_CASE(5, 4) DBCSR_BIG_CASE(5, 5)
#undef DBCSR_BIG_CASE
    default: return false;
  }
}

// any sizes up to 32, one wave per C block, whole blocks staged in the wave's LDS slice; `grid` workgroups of c.ww waves
static void launch_lds_f64(const NumericArgs<double>& p, const NumericChoice& c, unsigned grid) {
  auto kern = c.maxt == 1 ? mm_numeric_f64_lds<1> : c.maxt == 2 ? mm_numeric_f64_lds<2> : c.maxt == 3 ? mm_numeric_f64_lds<3> : mm_numeric_f64_lds<4>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * c.ww), c.lds_bytes, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.lds_a,
                     c.lds_wave, c.flags, p.order);
}

// the same with c.group C blocks per wave, the next block's operands in flight (mixed sizes, few products per block)
static void launch_pipe_f64(const NumericArgs<double>& p, const NumericChoice& c, int64_t npos) {
  auto kern = c.maxt == 1 ? mm_numeric_f64_pipe<1> : c.maxt == 2 ? mm_numeric_f64_pipe<2> : c.maxt == 3 ? mm_numeric_f64_pipe<3> : mm_numeric_f64_pipe<4>;
  hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), c.lds_bytes, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.lds_a,
                     c.lds_wave, c.flags, p.order, npos, c.group);
}

// C blocks of at most 4 x 4: four per wave
static void launch_tiny_f64(const NumericArgs<double>& p, const NumericChoice& c, bool k4) {   // k4: the inner dimension is at most 4 too
  auto kern = k4 ? mm_numeric_f64_tiny<true> : mm_numeric_f64_tiny<false>;
  hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), 0, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.flags, p.order);
}

// every block dimension at most 8: one 8 x 8 tile per wave, c.depth products in flight, c.group C blocks per wave (mm_numeric_f64_small.h)
static void launch_small_f64(const NumericArgs<double>& p, const NumericChoice& c, int64_t npos) {
  const int d = c.depth;
  auto kern = p.work ? (d == 2 ? mm_numeric_f64_small<2, true> : d == 3 ? mm_numeric_f64_small<3, true> : d == 4 ? mm_numeric_f64_small<4, true> :
                        d == 6 ? mm_numeric_f64_small<6, true> : mm_numeric_f64_small<8, true>)
                     : (d == 2 ? mm_numeric_f64_small<2, false> : d == 3 ? mm_numeric_f64_small<3, false> : d == 4 ? mm_numeric_f64_small<4, false> :
                        d == 6 ? mm_numeric_f64_small<6, false> : mm_numeric_f64_small<8, false>);
  hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), 0, p.st, p.descs, p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, c.flags, p.order,
                     p.work, c.group, npos);
}

// complex_8: one wave per C block (launch position), c.ww waves per workgroup, the instance of the multiply's largest block (mm_numeric_z64.h)
static bool launch_z64(const NumericArgs<z64>& p, const NumericChoice& c, int ma, int nc, int64_t npos) {
  if (!z64_has(ma, nc) || c.grid == 0) return false;
  const int* order = npos > 0 ? p.order : nullptr;
  switch (ma * 8 + nc) {
#define DBCSR_Z64_CASE(A_, B_)                                                                                                                  \
  case A_ * 8 + B_:                                                                                                                             \
    hipLaunchKernelGGL((mm_numeric_z64<A_, B_>), dim3(c.grid), dim3(64 * c.ww), c.lds_bytes, p.st, p.descs, p.nblk, p.entries, p.a, p.b,        \
                       p.c_out, p.c_in, p.alpha.re, p.alpha.im, p.beta.re, p.beta.im, c.flags, order, npos);                                    \
    return true;
    DBCSR_Z64_CASE(1, 1) DBCSR_Z64_CASE(1, 2) DBCSR_Z64_CASE(1, 3) DBCSR_Z64_CASE(1, 4)
    DBCSR_Z64_CASE(2, 1) DBCSR_Z64_CASE(2, 2) DBCSR_Z64_CASE(2, 3) DBCSR_Z64_CASE(2, 4)
    DBCSR_Z64_CASE(3, 1) DBCSR_Z64_CASE(3, 2) DBCSR_Z64_CASE(3, 3) DBCSR_Z64_CASE(3, 4)
    DBCSR_Z64_CASE(4, 1) DBCSR_Z64_CASE(4, 2) DBCSR_Z64_CASE(4, 3) DBCSR_Z64_CASE(4, 4)
#undef DBCSR_Z64_CASE
    default: return false;
  }
}

#endif
