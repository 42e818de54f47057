// ubench_flat_add.hip -- which launch shape the flat pass of the same-pattern add should have (algebra_add_flat, dbcsr_amd/csrc/mm_algebra.h):
// a[i] = a[i] + beta * b[i] in place over the 1424^2 * 529 doubles of config 2's product (8.6 GB per area), 16 bytes per lane and access.  Variants: U accesses
// in flight per lane, taken nthreads apart (stride) or inside one contiguous chunk per workgroup (chunk), plain or non-temporal stores, grids of 2048 / 4096 /
// 8192 workgroups with a grid-stride loop or one workgroup per chunk and no loop (grid=0).  All variants alternate in one process, three launches per sample.
//   hipcc -O3 --offload-arch=gfx950 ubench_flat_add.hip -o ubench_flat_add && ./ubench_flat_add
// Result (profiles/matrix_ops.txt): no loop and U = 1 is the fastest.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
typedef double f64x2 __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

// variant 0: grid-stride, U accesses nthreads apart
template <int U, bool NT>
__global__ void __launch_bounds__(256) v_stride(const f64x2* a, const f64x2* b, f64x2* d, long nv, double beta) {
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, nt = (long)gridDim.x * 256;
  for (long base = tid; base < nv; base += U * nt) {
    f64x2 x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) if (base + u * nt < nv) { x[u] = a[base + u * nt]; y[u] = b[base + u * nt]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (base + u * nt < nv) {
      f64x2 r = x[u] + beta * y[u];
      if (NT) __builtin_nontemporal_store(r, &d[base + u * nt]); else d[base + u * nt] = r;
    }
  }
}
// variant 1: a workgroup takes contiguous chunks of 256 * U vectors, chunks grid-strided
template <int U, bool NT>
__global__ void __launch_bounds__(256) v_chunk(const f64x2* a, const f64x2* b, f64x2* d, long nv, double beta) {
  const long nchunks = (nv + 256 * U - 1) / (256 * U);
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long base = c * 256 * U + threadIdx.x;
    f64x2 x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) if (base + u * 256 < nv) { x[u] = a[base + u * 256]; y[u] = b[base + u * 256]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (base + u * 256 < nv) {
      f64x2 r = x[u] + beta * y[u];
      if (NT) __builtin_nontemporal_store(r, &d[base + u * 256]); else d[base + u * 256] = r;
    }
  }
}
template <int U, bool NT>
static void launch_u(int kind, long grid, double* a, double* b, long nv) {
  if (kind == 0) hipLaunchKernelGGL((v_stride<U, NT>), dim3((unsigned)grid), dim3(256), 0, 0, (const f64x2*)a, (const f64x2*)b, (f64x2*)a, nv, 1e-3);
  else hipLaunchKernelGGL((v_chunk<U, NT>), dim3((unsigned)grid), dim3(256), 0, 0, (const f64x2*)a, (const f64x2*)b, (f64x2*)a, nv, 1e-3);
}
static void launch(int kind, int U, int nt, long grid, double* a, double* b, long nv) {
  if (nt) { if (U == 1) launch_u<1, true>(kind, grid, a, b, nv); else if (U == 2) launch_u<2, true>(kind, grid, a, b, nv); else if (U == 4) launch_u<4, true>(kind, grid, a, b, nv); else launch_u<8, true>(kind, grid, a, b, nv); }
  else { if (U == 1) launch_u<1, false>(kind, grid, a, b, nv); else if (U == 2) launch_u<2, false>(kind, grid, a, b, nv); else if (U == 4) launch_u<4, false>(kind, grid, a, b, nv); else launch_u<8, false>(kind, grid, a, b, nv); }
}
int main() {
  const long n = 1424L * 1424 * 529, nv = n / 2;
  double *a, *b;
  CK(hipMalloc(&a, n * 8)); CK(hipMalloc(&b, n * 8));
  CK(hipMemset(a, 0, n * 8)); CK(hipMemset(b, 0, n * 8));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  struct V { const char* name; int kind, U, nt; long grid; };
  std::vector<V> vs;
  for (long g : {2048L, 8192L, 0L}) for (int U : {1, 2, 4, 8}) for (int nt : {0, 1}) { vs.push_back({"stride", 0, U, nt, g}); vs.push_back({"chunk", 1, U, nt, g}); }
  std::vector<std::vector<float>> t(vs.size());
  for (int round = 0; round < 6; ++round)
    for (size_t i = 0; i < vs.size(); ++i) {
      const V& v = vs[i];
      long grid = v.grid ? v.grid : (nv + 256L * v.U - 1) / (256L * v.U);
      CK(hipEventRecord(e0));
      for (int r = 0; r < 3; ++r) {
        launch(v.kind, v.U, v.nt, grid, a, b, nv);
      }
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (round) t[i].push_back(ms / 3);
    }
  for (size_t i = 0; i < vs.size(); ++i) {
    std::sort(t[i].begin(), t[i].end());
    printf("%-6s U=%d nt=%d grid=%-7ld median %.4f ms min %.4f max %.4f  %.0f GB/s\n", vs[i].name, vs[i].U, vs[i].nt, vs[i].grid, t[i][t[i].size() / 2], t[i].front(), t[i].back(),
           24e-6 * n / t[i][t[i].size() / 2]);
  }
  return 0;
}
