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
template <class Tr, int SC = kFinPlain>
hipError_t tr(bool lds, const void* const* srcs, int k, void* dst, size_t count, hipStream_t s, double r = 1.0,
              unsigned* am = nullptr) {
  return lds ? launch_tr<Tr, kHot, SC>(srcs, k, dst, count, s, r, am)
             : launch_tr<Tr, 0, SC>(srcs, k, dst, count, s, r, am);
}
// One format's sum, nested or flat, in one of the three finishes (float_sum of reduce_kernels.hip): a one-round
// ring fold (round_each, k > 2) rounds after every add, under a scaled or an amax finish before each add instead.
template <class F, int SC>
ftar_status_t sum(const void* const* srcs, int k, void* dst, size_t count, hipStream_t s, bool round_each,
                  const int* shape, int nlevels, bool lds, double r, unsigned* am = nullptr) {
  hipError_t e = hipErrorInvalidValue;
  if (nlevels > 1 && k > 1) {
    TreeCode tc;
    if (!shape || !make_tree_code(shape, nlevels, k, &tc)) return FTAR_ERR_INVALID_ARG;
    e = launch_tree<F8SumT<F>, SC>(srcs, k, tc, shape, nlevels, dst, count, s, lds, r, am);
  } else if (round_each && k > 2) {
    e = tr<std::conditional_t<SC != kFinPlain, F8SumHopPreT<F>, F8SumHopT<F>>, SC>(lds, srcs, k, dst, count, s, r, am);
  } else {
    e = tr<F8SumT<F>, SC>(lds, srcs, k, dst, count, s, r, am);
  }
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}
}  // namespace

ftar_status_t launch_reduce_f8(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dt, ftar_op_t op,
                               hipStream_t s, bool round_each, const int* shape, int nlevels, bool lds,
                               const double* scale, unsigned* amax) {
  const bool e5m2 = dt == FTAR_FLOAT8_E5M2;
  if (amax)  // launch_reduce checked that a scale comes with it
    return e5m2 ? sum<E5M2Fmt, kFinAmax>(srcs, k, dst, count, s, round_each, shape, nlevels, lds, *scale, amax)
                : sum<E4M3Fmt, kFinAmax>(srcs, k, dst, count, s, round_each, shape, nlevels, lds, *scale, amax);
  // a scaled k = 1 is a scaled copy through the runtime-k kernel; a plain one is a copy
  if (scale)
    return e5m2 ? sum<E5M2Fmt, kFinScaled>(srcs, k, dst, count, s, round_each, shape, nlevels, lds, *scale)
                : sum<E4M3Fmt, kFinScaled>(srcs, k, dst, count, s, round_each, shape, nlevels, lds, *scale);
  if (k == 1) return launch_copy(srcs[0], dst, count, s);
  hipError_t e = hipErrorInvalidValue;
  switch (op) {
    case FTAR_SUM:
      return e5m2 ? sum<E5M2Fmt, kFinPlain>(srcs, k, dst, count, s, round_each, shape, nlevels, lds, 1.0)
                  : sum<E4M3Fmt, kFinPlain>(srcs, k, dst, count, s, round_each, shape, nlevels, lds, 1.0);
    case FTAR_MAX:
      e = e5m2 ? tr<F8MinMax<E5M2Fmt, true>>(lds, srcs, k, dst, count, s)
               : tr<F8MinMax<E4M3Fmt, true>>(lds, srcs, k, dst, count, s);
      break;
    case FTAR_MIN:
      e = e5m2 ? tr<F8MinMax<E5M2Fmt, false>>(lds, srcs, k, dst, count, s)
               : tr<F8MinMax<E4M3Fmt, false>>(lds, srcs, k, dst, count, s);
      break;
    default: return FTAR_ERR_UNSUPPORTED;  // BAND and AVG: refused by launch_reduce before this
  }
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}

}  // namespace ftar
