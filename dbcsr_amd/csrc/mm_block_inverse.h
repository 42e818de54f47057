// mm_block_inverse.h -- the block diagonal on the device: the index and the copy of dbcsr_get_block_diag (block_diag_find, block_diag_copy) and the batched
// inversion of the diagonal blocks in place (block_inverse_wave, block_inverse_wide; dbcsr_amd_bcsr_block_diag_invert) -- the initial guess of a
// Hotelling / Newton-Schulz inverse and the block-Jacobi preconditioner.  Part of the device-resident multiply engine: included by mm_engine.hip after
// mm_rank_update.h.
//
// The inversion is Gauss-Jordan in place with partial (row) pivoting on a copy of the block in LDS, in double / complex double for all three data types
// (float32 converted on load, rounded once on store).  The copy is column by column with a pitch of P = n | 1 elements (block_inverse_pitch).  Step k:
//   a. every wave reads column k (lane = row), finds the pivot row p -- the largest |x| (complex: |re| + |im|) among the rows k ... n - 1, compared with >
//      against 0 so that a NaN never wins and a zero column has no pivot, the lowest row on ties -- by a butterfly over the wave; the first wave stages
//      f = column k as it stands after the row exchange (f[p] = the old a_kk; f[k] is not used).  1 / a_pk is formed by every thread alike.
//   b. thread j < n: r[j] = a_pj / a_pk (r[k] = 1 / a_pk) and, the exchange, a_pj <- a_kj for j != k.
//   c. element (i, j): a_kj <- r[j];  a_ij <- a_ij - f[i] r[j] for i != k, where column k counts as zero (a_ik <- -f[i] r[k]).
// A thread owns the same elements in every step: row i = tid mod W of the columns tid / W, tid / W + G, ... (W the power of two >= n, G W = threads), so
// f[i] is read once per step and the reads of a column are consecutive.  Nobody writes column k before c, so a and b need no barrier between them: two
// hand-overs per step (after b, after c), of a wave (n <= 32: wave_lds_handover, no workgroup barrier) or of the workgroup (33 ... 96: __syncthreads).
// The row exchanges leave the inverse with its columns permuted: final column c is working column s_{n-1}(... s_0(c)), s_k the exchange (k p_k) -- thread c
// follows its own index through the steps in a register, and the store reads column src[c].
// A block without a pivot in some step is singular: nothing of it is stored, it is counted (integer atomics on info[0], info[1]) and every other block is
// still inverted.  Load and store go through walk_block: who moves which element depends on the block's place, what is computed does not -- the bits of an
// inverse depend on the block's values, dimension and type alone.  No atomics on data; every store stays inside the block.
#ifndef DBCSR_AMD_MM_BLOCK_INVERSE_H
#define DBCSR_AMD_MM_BLOCK_INVERSE_H
#include "mm_algebra.h"

namespace dbcsr_amd {

constexpr int kBlockInverseWaveDim = 32;   // up to this dimension a wave inverts a block, above it a workgroup of 256
constexpr int kBlockInverseMaxDim = 96;    // 96 x 97 complex doubles + f, r, src: 152 448 bytes of the 160 KiB of LDS

// elements between two columns of the LDS copy of an n x n block: odd, so that the walk along a row (b: stride P) meets every bank once -- 8-byte elements
// in groups of 32 lanes over 64 banks of 4 bytes, 16-byte elements in groups of 16 -- and the walk down a column (a, c) is consecutive
__host__ __device__ constexpr int block_inverse_pitch(int n) { return n | 1; }

// LDS bytes of one block of dimension up to nmax: the copy, f, r (Acc) and src (int), a multiple of 16
template <typename Acc>
__host__ __device__ constexpr size_t block_inverse_lds_bytes(int nmax) {
  return (((size_t)nmax * block_inverse_pitch(nmax) + 2 * (size_t)nmax) * sizeof(Acc) + (size_t)nmax * sizeof(int) + 15) & ~(size_t)15;
}

// |x| for the pivot search: complex data LAPACK's cabs1
__device__ __forceinline__ double block_inverse_abs(double x) { return fabs(x); }
__device__ __forceinline__ double block_inverse_abs(z64 x) { return fabs(x.re) + fabs(x.im); }

// 1 / x; complex data scaled by a power of two first (exact), so that the squares neither overflow nor vanish where x itself does not: conj(x) / |x|^2
// with three roundings per part
__device__ __forceinline__ double block_inverse_recip(double x) { return 1.0 / x; }
__device__ __forceinline__ z64 block_inverse_recip(z64 x) {
  int e;
  (void)frexp(fabs(x.re) + fabs(x.im), &e);
  const double a = ldexp(x.re, -e), b = ldexp(x.im, -e), d = a * a + b * b;
  return z64(ldexp(a / d, -e), ldexp(-b / d, -e));
}

__device__ __forceinline__ double block_inverse_fnma(double old, double f, double r) { return old - f * r; }
__device__ __forceinline__ z64 block_inverse_fnma(z64 old, z64 f, z64 r) {
  return z64(old.re - (f.re * r.re - f.im * r.im), old.im - (f.re * r.im + f.im * r.re));
}

// c ? a : b, part by part (a choice between two complex values as a whole goes through memory)
__device__ __forceinline__ double block_inverse_pick(bool c, double a, double b) { return c ? a : b; }
__device__ __forceinline__ z64 block_inverse_pick(bool c, z64 a, z64 b) { return z64(c ? a.re : b.re, c ? a.im : b.im); }

constexpr int kBlockInverseNoRow = 0x7fffffff;

// (value, row) of the better pivot candidate: the larger value, the lower row on ties; kBlockInverseNoRow: no candidate (its value is 0)
__device__ __forceinline__ void block_inverse_better(double& v, int& at, double w, int wat) {
  if (w > v || (w == v && wat < at)) v = w, at = wat;
}

template <bool GROUP>
__device__ __forceinline__ void block_inverse_handover() {
  if constexpr (GROUP) __syncthreads();
  else wave_lds_handover();
}

// The n x n block at blk (element offset `off` of its data area) inverted in place by NT = 64 (one wave) or 256 (the workgroup) threads; lds: their
// block_inverse_lds_bytes(n) bytes.  Returns false -- and has stored nothing -- when the block is singular.  Every thread of the NT gets the same answer.
template <typename T, bool GROUP>
__device__ __forceinline__ bool block_inverse_run(T* __restrict__ blk, int64_t off, int n, char* lds, int tid, int vec_ok) {
  using Acc = typename MatvecAcc<T>::type;
  constexpr int NT = GROUP ? 256 : 64;
  const int lane = tid & 63, P = block_inverse_pitch(n);
  Acc* a = reinterpret_cast<Acc*>(lds);   // (LDS that the threads hand to each other: no __restrict__ on these)
  Acc* f = a + (size_t)n * P;
  Acc* r = f + n;
  int* src = reinterpret_cast<int*>(r + n);
  // the copy (element e of the block is row e mod n of column e / n)
  walk_block_values<T>(blk, off, n * n, tid, NT, vec_ok, [&](int e, T x) {
    const int j = e / n;
    a[(e - j * n) + j * P] = matvec_wide(x);
  });
  block_inverse_handover<GROUP>();
  int shift = 0;
  while ((1 << shift) < n) ++shift;
  const int i = tid & ((1 << shift) - 1), jg = tid >> shift, G = NT >> shift;
  int mine = tid;   // the working column that ends as column tid
  bool singular = false;
  for (int k = 0; k < n; ++k) {
    // a. the pivot of column k (every wave for itself)
    const Acc* colk = a + (size_t)k * P;
    const Acc v0 = colk[lane < n ? lane : 0], v1 = colk[GROUP && lane + 64 < n ? lane + 64 : 0];   // (rows that are not there: an address that is)
    double best = 0.0;
    int p = kBlockInverseNoRow;
    {
      const double w = block_inverse_abs(v0);
      if (lane < n && lane >= k && w > 0.0) best = w, p = lane;
    }
    if constexpr (GROUP) {
      const double w = block_inverse_abs(v1);
      if (lane + 64 < n && lane + 64 >= k && w > best) best = w, p = lane + 64;   // (a higher row: only when larger)
    }
#pragma unroll
    for (int o = GROUP ? 32 : 16; o > 0; o >>= 1) block_inverse_better(best, p, __shfl_xor(best, o, 64), __shfl_xor(p, o, 64));
    p = __builtin_amdgcn_readfirstlane(p);
    if (p == kBlockInverseNoRow) {
      singular = true;
      break;
    }
    const Acc vk = colk[k], pinv = block_inverse_recip(colk[p]);
    if (tid < 64) {
      if (lane < n) f[lane] = block_inverse_pick(lane == p, vk, v0);
      if constexpr (GROUP) {
        if (lane + 64 < n) f[lane + 64] = block_inverse_pick(lane + 64 == p, vk, v1);
      }
    }
    // b. the scaled pivot row, and row k to where the pivot row was (column k is left to c)
    if (tid < n) {
      const int j = tid;
      Acc* colj = a + (size_t)j * P;
      r[j] = block_inverse_pick(j == k, pinv, colj[p] * pinv);
      if (p != k && j != k) colj[p] = colj[k];
      mine = mine == k ? p : (mine == p ? k : mine);
    }
    block_inverse_handover<GROUP>();
    // c. the elimination
    if (i < n) {
      const Acc fi = f[i];
      for (int j = jg; j < n; j += G) {
        Acc* x = a + i + (size_t)j * P;
        const Acc rj = r[j];
        *x = block_inverse_pick(i == k, rj, block_inverse_fnma(block_inverse_pick(j == k, Acc(0.0), *x), fi, rj));
      }
    }
    block_inverse_handover<GROUP>();
  }
  if (singular) return false;
  if (tid < n) src[tid] = mine;
  block_inverse_handover<GROUP>();
  auto at = [&](int e) {
    const int j = e / n;
    return matvec_narrow<T>(a[(e - j * n) + (size_t)src[j] * P]);
  };
  walk_block<T>(
      off, n * n, tid, NT, vec_ok, [&](int e) { blk[e] = at(e); },
      [&](int e) {
        Pack16<T> x;
#pragma unroll
        for (int u = 0; u < Pack16<T>::V; ++u) x.v[u] = at(e + u);
        *reinterpret_cast<Pack16<T>*>(blk + e) = x;
      });
  return true;
}

// info[0] += 1, info[1] = min(info[1], row): a singular block; info[2] += 1: a block that was skipped
__device__ __forceinline__ void block_inverse_report(unsigned long long* __restrict__ info, bool skipped, int row) {
  if (skipped) {
    atomicAdd(info + 2, 1ull);
  } else {
    atomicAdd(info + 0, 1ull);
    atomicMin(info + 1, (unsigned long long)row);
  }
}

// One wave per block row: the diagonal block of dimension <= nmax (<= 32; nmax sized the LDS slice of every wave) is inverted.  This kernel also counts
// the blocks nobody inverts: a dimension above max_dim, or a diagonal block that is not square.
template <typename T>
__global__ void __launch_bounds__(256)
block_inverse_wave(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, T* __restrict__ data,
                   const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int nmax, int max_dim, int vec_ok, unsigned long long* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Acc = typename MatvecAcc<T>::type;
  const int lane = threadIdx.x & 63;
  const int64_t row64 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row64 >= nbr) return;
  const int row = (int)row64;
  const int at = find_diag_block(row_p, col_i, row, lane);
  if (at < 0) return;
  const int n = rs[row];
  if (n <= 0) return;
  if (cs[row] != n || n > max_dim) {
    if (lane == 0) block_inverse_report(info, true, row);
    return;
  }
  if (n > nmax) return;   // (the workgroup kernel's)
  const int64_t off = blk_p[at];
  char* lds = smem + (size_t)(threadIdx.x >> 6) * block_inverse_lds_bytes<Acc>(nmax);
  if (!block_inverse_run<T, false>(data + off, off, n, lds, lane, vec_ok) && lane == 0) block_inverse_report(info, false, row);
}

// One workgroup of 256 per block row: the diagonal block of dimension 33 ... max_dim is inverted.
template <typename T>
__global__ void __launch_bounds__(256)
block_inverse_wide(const int* __restrict__ row_p, const int* __restrict__ col_i, const int64_t* __restrict__ blk_p, T* __restrict__ data,
                    const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int max_dim, int vec_ok, unsigned long long* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int row = blockIdx.x;
  if (row >= nbr) return;
  const int n = rs[row];
  if (n <= kBlockInverseWaveDim || n > max_dim || cs[row] != n) return;   // (workgroup-uniform)
  const int at = find_diag_block(row_p, col_i, row, threadIdx.x & 63);
  if (at < 0) return;
  const int64_t off = blk_p[at];
  if (!block_inverse_run<T, true>(data + off, off, n, smem, threadIdx.x, vec_ok) && threadIdx.x == 0) block_inverse_report(info, false, row);
}

// ---- dbcsr_get_block_diag ------------------------------------------------------------------------------------------------------------------------------
// one wavefront per block row: have[row] = 1 and blk_nze[row] = the elements of its diagonal block when the row stores one, 0 otherwise; *max_dim = the
// largest dimension of such a block (integer atomicMax)
__global__ void __launch_bounds__(256) block_diag_find(const int* __restrict__ row_p, const int* __restrict__ col_i, const int* __restrict__ rs,
                                                       const int* __restrict__ cs, int nbr, int* __restrict__ have, int* __restrict__ blk_nze,
                                                       int* __restrict__ max_dim) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= nbr) return;
  const int at = find_diag_block(row_p, col_i, row, lane);
  if (lane == 0) {
    have[row] = at >= 0 ? 1 : 0;
    blk_nze[row] = at >= 0 ? rs[row] * cs[row] : 0;
    if (at >= 0) atomicMax(max_dim, rs[row] > cs[row] ? rs[row] : cs[row]);
  }
}

// one wavefront per block row: the diagonal block of dst = the diagonal block of src, bit for bit (rows where either has none: nothing).  Aligned on
// dst's block; the source is read from wherever its block starts.
template <typename T>
__global__ void __launch_bounds__(256)
block_diag_copy(const int* __restrict__ s_row_p, const int* __restrict__ s_col_i, const int64_t* __restrict__ s_blk_p, const T* __restrict__ s_data,
                const int* __restrict__ d_row_p, const int* __restrict__ d_col_i, const int64_t* __restrict__ d_blk_p, T* __restrict__ d_data,
                const int* __restrict__ rs, const int* __restrict__ cs, int nbr, int vec_ok) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= nbr) return;
  const int sa = find_diag_block(s_row_p, s_col_i, row, lane);
  if (sa < 0) return;
  const int da = find_diag_block(d_row_p, d_col_i, row, lane);
  if (da < 0) return;
  const int64_t dof = d_blk_p[da];
  const T* __restrict__ s = s_data + s_blk_p[sa];
  T* __restrict__ d = d_data + dof;
  walk_block<T>(
      dof, rs[row] * cs[row], lane, 64, vec_ok, [&](int e) { d[e] = s[e]; },
      [&](int e) {
        const Pack16U<T> x = *reinterpret_cast<const Pack16U<T>*>(s + e);
        Pack16<T> y;
#pragma unroll
        for (int u = 0; u < Pack16<T>::V; ++u) y.v[u] = x.v[u];
        *reinterpret_cast<Pack16<T>*>(d + e) = y;
      });
}

}  // namespace dbcsr_amd
#endif
