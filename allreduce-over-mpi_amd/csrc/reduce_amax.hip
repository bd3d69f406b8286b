// The amax finish of f32, bf16 and fp16 (launch_reduce hands every fold with an amax word over; fp8's is in
// reduce_f8.hip): traits and kernels in reduce_impl.h.  A translation unit of its own, as reduce_f8.hip is: its
// kernels are a third set beside the plain and the scaled ones, and side by side a parallel build stays at the
// length it had.
#include "reduce_impl.h"

namespace ftar {

namespace {
template <class Tr>
hipError_t tr(bool lds, const void* const* srcs, int k, void* dst, size_t count, hipStream_t s, double r,
              unsigned* am) {
  return lds ? launch_tr<Tr, 16, kFinAmax>(srcs, k, dst, count, s, r, am)
             : launch_tr<Tr, 0, kFinAmax>(srcs, k, dst, count, s, r, am);
}
// One dtype's sum, nested or flat (float_sum of reduce_kernels.hip under a scaled finish): Sum its trait, HopPre
// the one of a one-round ring fold (round_each, k > 2), which rounds before each add.
template <class Sum, class HopPre>
hipError_t sum(const void* const* srcs, int k, void* dst, size_t count, hipStream_t s, bool hop, const TreeCode* tc,
               const int* shape, int nlevels, bool lds, double r, unsigned* am) {
  if (tc) return launch_tree<Sum, kFinAmax>(srcs, k, *tc, shape, nlevels, dst, count, s, lds, r, am);
  return hop ? tr<HopPre>(lds, srcs, k, dst, count, s, r, am) : tr<Sum>(lds, srcs, k, dst, count, s, r, am);
}
}  // namespace

ftar_status_t launch_reduce_amax(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dt,
                                 hipStream_t s, bool round_each, const int* shape, int nlevels, bool lds, double r,
                                 unsigned* amax) {
  TreeCode code;
  const TreeCode* tc = nullptr;
  if (nlevels > 1 && k > 1) {
    if (!shape || !make_tree_code(shape, nlevels, k, &code)) return FTAR_ERR_INVALID_ARG;
    tc = &code;
  }
  const bool hop = round_each && k > 2;
  hipError_t e = hipErrorInvalidValue;
  switch (dt) {
    case FTAR_FLOAT32: e = sum<F32Sum, F32Sum>(srcs, k, dst, count, s, false, tc, shape, nlevels, lds, r, amax); break;
    case FTAR_FLOAT16:
      e = sum<F16Sum, F16SumHopPre>(srcs, k, dst, count, s, hop, tc, shape, nlevels, lds, r, amax);
      break;
    case FTAR_BFLOAT16:
      e = sum<BF16Sum, BF16SumHopPre>(srcs, k, dst, count, s, hop, tc, shape, nlevels, lds, r, amax);
      break;
    default: return FTAR_ERR_UNSUPPORTED;
  }
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}

}  // namespace ftar
