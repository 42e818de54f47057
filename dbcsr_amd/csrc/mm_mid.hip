// mm_mid.hip -- the instantiations of mm_numeric_f64_mid (one wave per C block, operands in slabs through 6-13 KB of LDS) and their launcher.
// Slabs of 16 inner indices while the block has at most 8 units of 4 x 4 per dimension (32 x 32: 130 registers, three waves per SIMD), of 8 above
// (40 x 40 with 16 would need 40 staging registers more than three waves per SIMD leave).
// The list of shapes (DBCSR_AMD_MID_SHAPES) and the rule for which of them a multiply should take (mid_f64_serves, with the measurements behind it) are in
// mm_choose.h, where the kernel choice is made.
#include "mm_mid.h"

#include "smm_core.h"
#include "mm_numeric_f64_mid.h"

namespace dbcsr_amd {

bool launch_mid_f64(const NumericArgs<double>& p, int rb, int cb, bool other_sizes, unsigned npos, int max_units) {
  if (npos == 0 || rb < 6 || cb < 6 || rb > 12 || cb > 12) return false;
  // the shape that covers every block of the multiply (the second launch; the only one when the dominant size is that shape)
  const int fb = (max_units > 10 || rb > 10 || cb > 10) ? 12 : 10;
  const bool single = rb == fb && cb == fb;
  const int flags = (p.skip_empty & 1) | (single ? 32 : 0);
  switch (rb * 16 + cb) {
#define DBCSR_MID_CASE(A_, B_)                                                                                                                   \
  case A_ * 16 + B_: {                                                                                                                           \
    constexpr int KSL = (A_ <= 8 && B_ <= 8) ? 16 : 8;                                                                                           \
    hipLaunchKernelGGL((mm_numeric_f64_mid<A_, B_, KSL>), dim3(npos), dim3(64), (size_t)mid_lds_bytes((A_ + 1) / 2, (B_ + 1) / 2, KSL), p.st, p.descs,   \
                       p.nblk, p.entries, p.a, p.b, p.c_out, p.c_in, p.alpha, p.beta, flags, p.order, p.work, p.norms);                          \
  } break;
    DBCSR_AMD_MID_SHAPES(DBCSR_MID_CASE)
#undef DBCSR_MID_CASE
    default: return false;
  }
  if (!single && other_sizes) {
    const int f2 = (p.skip_empty & 1) | 16 | (rb << 8) | (cb << 12);
    if (fb == 12)
      hipLaunchKernelGGL((mm_numeric_f64_mid<12, 12, 8>), dim3(npos), dim3(64), (size_t)mid_lds_bytes(6, 6, 8), p.st, p.descs, p.nblk, p.entries, p.a, p.b,
                         p.c_out, p.c_in, p.alpha, p.beta, f2, p.order, p.work, p.norms);
    else
      hipLaunchKernelGGL((mm_numeric_f64_mid<10, 10, 8>), dim3(npos), dim3(64), (size_t)mid_lds_bytes(5, 5, 8), p.st, p.descs, p.nblk, p.entries, p.a, p.b,
                         p.c_out, p.c_in, p.alpha, p.beta, f2, p.order, p.work, p.norms);
  }
  return true;
}

}  // namespace dbcsr_amd
