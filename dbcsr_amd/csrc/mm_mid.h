// mm_mid.h -- the operand bundle of the numeric launchers (NumericArgs) and the launcher of the one-wave slab kernels (mm_numeric_f64_mid.h), which are
// compiled in a translation unit of their own (mm_mid.hip)
#ifndef DBCSR_AMD_MM_MID_H
#define DBCSR_AMD_MM_MID_H
#include <hip/hip_runtime.h>

#include "../../include/dbcsr_amd_mm.h"
#include "mm_choose.h"   // mid_f64_serves, mid_f64_has, DBCSR_AMD_MID_SHAPES
#include "mm_types.h"

namespace dbcsr_amd {

// What every numeric kernel is handed, filled once per dbcsr_amd_mm_numeric call.  HOST side only: each launcher unpacks it again into the kernel's scalar
// arguments (a struct passed into the exact-size kernel once cost config 2 fifteen per cent through scratch memory, tests/test_kernel_resources.py).
template <typename T>
struct NumericArgs {
  hipStream_t st;
  const Desc* descs;
  int64_t nblk;
  const Entry* entries;
  const T *a, *b;
  T* c_out;
  const T* c_in;
  T alpha, beta;
  int skip_empty;
  const int* order;
  const Work* work;   // launch-order records (null: the kernels read order[] -> descs[] -> entries[])
  double* norms;      // (may be null): every block's squared Frobenius norm as stored
  const dbcsr_amd_bcsr *A, *B, *C;   // the operands' and C_out's index (the lab dataflows build lists of their own from it)
  bool reuse;         // the plan of the previous multiply stands
  // the same operands on a segment of the launch order that starts at position off (an (m, n) class)
  NumericArgs segment(int64_t off) const {
    NumericArgs s = *this;
    s.order = order + off;
    s.work = work ? work + off : nullptr;
    return s;
  }
};

// C blocks of rb x cb units of 4 x 4 (6 ... 12 per dimension, the larger at least 8: 21 ... 48 rows / columns with at least one dimension above 28) on the
// launch-order positions order[0 .. npos): one wave per block.  other_sizes: positions may hold blocks of another size -- a second launch of the
// largest shape (<10, 10> up to 40, <12, 12> up to 48) takes them.  max_units: the largest block dimension of the launch, in units of 4.
// false: no kernel for this shape (mid_f64_has) or no position; nothing was launched.
bool launch_mid_f64(const NumericArgs<double>& p, int rb, int cb, bool other_sizes, unsigned npos, int max_units);

}  // namespace dbcsr_amd
#endif
