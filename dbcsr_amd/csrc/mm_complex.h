// mm_complex.h -- the complex_8 element (dbcsr_type_complex_8: COMPLEX(real_8), (re, im) interleaved) and the few per-element helpers through which the
// type-generic kernels around the multiply (norms, transpose, crop, filter, init_c, scale_window) serve real and complex data alike.  For double / float
// every helper is the expression the kernels held before: real data takes exactly the arithmetic it always took.
#ifndef DBCSR_AMD_MM_COMPLEX_H
#define DBCSR_AMD_MM_COMPLEX_H
#include <hip/hip_runtime.h>

namespace dbcsr_amd {

struct alignas(16) z64 {
  double re, im;
  z64() = default;
  __host__ __device__ constexpr z64(double r, double i = 0.0) : re(r), im(i) {}
};
__host__ __device__ __forceinline__ z64 operator*(z64 a, z64 b) { return z64(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
__host__ __device__ __forceinline__ z64 operator+(z64 a, z64 b) { return z64(a.re + b.re, a.im + b.im); }
__host__ __device__ __forceinline__ z64& operator*=(z64& a, z64 b) { return a = a * b; }

// |scale * x|^2 (block norms: the on-the-fly filter and the final block filter)
__device__ __forceinline__ double scaled_norm2(double scale, double x) { const double y = scale * x; return y * y; }
__device__ __forceinline__ double scaled_norm2(double scale, float x) { const double y = scale * (double)x; return y * y; }
__device__ __forceinline__ double scaled_norm2(double scale, z64 x) { const double yr = scale * x.re, yi = scale * x.im; return yr * yr + yi * yi; }

// conjugate (dbcsr_amd_bcsr_transpose_conj; real data: the value itself)
__device__ __forceinline__ double conj_of(double x) { return x; }
__device__ __forceinline__ float conj_of(float x) { return x; }
__device__ __forceinline__ z64 conj_of(z64 x) { return z64(x.re, -x.im); }

// element of the twin block of a matrix with symmetry (dbcsr_amd_bcsr_twin_apply; the transposition is the caller's).  kind: bit 0 negates, bit 1
// conjugates -- 0 symmetric, 1 antisymmetric, 2 hermitian, 3 antihermitian.  Sign flips only: exact, and an involution bit for bit.  Real data: conjugation
// is the identity
__device__ __forceinline__ double twin_of(double x, int kind) { return (kind & 1) ? -x : x; }
__device__ __forceinline__ float twin_of(float x, int kind) { return (kind & 1) ? -x : x; }
__device__ __forceinline__ z64 twin_of(z64 x, int kind) { return z64((kind & 1) ? -x.re : x.re, (((kind >> 1) ^ kind) & 1) ? -x.im : x.im); }

}  // namespace dbcsr_amd
#endif
