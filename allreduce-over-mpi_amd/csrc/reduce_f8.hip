// The fp8 half of the production dispatch (launch_reduce hands every FTAR_FLOAT8_E4M3 / _E5M2 fold over):
// traits and kernels in reduce_impl.h.  A translation unit of its own because its kernels compile for as long as
// two thirds of reduce_kernels.hip's: side by side, a parallel build stays at the length it had.
#include "reduce_impl.h"

namespace ftar {

namespace {
// HOT = 8, as for the other 1-byte types and not the 16-bit floats' 16: k = 9..16 (the one-round folds of 9 to 16
// ranks, more than a node holds) run on the runtime-k register kernel, and the eight further unrolled LDS
// kernels of every trait would lengthen this file's compile by a quarter.
constexpr int kHot = 8;
template <class F>
ftar_status_t fold(const FoldCall& f) {
  if (f.amax) return launch_sum<F8SumT<F>, F8SumHopT<F>, F8SumHopPreT<F>, kHot, kFinAmax>(f);
  // a scaled k = 1 is a scaled copy through the runtime-k kernel; a plain one is a copy
  if (f.scale) return launch_sum<F8SumT<F>, F8SumHopT<F>, F8SumHopPreT<F>, kHot, kFinScaled>(f);
  if (f.k == 1) return launch_copy(f.srcs[0], f.dst, f.count, f.stream);
  hipError_t e = hipErrorInvalidValue;
  switch (f.op) {
    case FTAR_SUM: return launch_sum<F8SumT<F>, F8SumHopT<F>, F8SumHopPreT<F>, kHot, kFinPlain>(f);
    case FTAR_MAX: e = launch_tr<F8MinMax<F, true>, kHot>(launch_of(f), f.count, f.lds); break;
    case FTAR_MIN: e = launch_tr<F8MinMax<F, false>, kHot>(launch_of(f), f.count, f.lds); break;
    default: return FTAR_ERR_UNSUPPORTED;  // BAND and AVG: refused by launch_reduce before this
  }
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}
}  // namespace

ftar_status_t launch_reduce_f8(const FoldCall& f) {
  return f.dt == FTAR_FLOAT8_E5M2 ? fold<E5M2Fmt>(f) : fold<E4M3Fmt>(f);
}

}  // namespace ftar
