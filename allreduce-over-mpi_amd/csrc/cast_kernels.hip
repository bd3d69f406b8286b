// The scaled casts of ftar_cast_scaled (wide <-> fp8, cast_impl.h) in the layout production runs.  A translation
// unit of its own, as reduce_f8.hip and reduce_amax.hip are: its kernels compile beside the folds'.
#include "cast_impl.h"

namespace ftar {

bool cast_pair_supported(ftar_dtype_t src, ftar_dtype_t dst) {
  return (is_cast_wide(src) && is_f8(dst)) || (is_f8(src) && is_cast_wide(dst));
}

ftar_status_t launch_cast_scaled(const void* src, ftar_dtype_t src_dt, void* dst, ftar_dtype_t dst_dt, size_t count,
                                 const float* scale, unsigned* amax, hipStream_t s) {
  if (!cast_pair_supported(src_dt, dst_dt)) return FTAR_ERR_UNSUPPORTED;
  if (count == 0) return FTAR_SUCCESS;
  if (!src || !dst) return FTAR_ERR_INVALID_ARG;
  FTAR_CHECK_HIP((launch_cast_any<kCastU16, kCastU32, kCastLayout>(src, src_dt, dst, dst_dt, count, scale, amax, s)));
  return FTAR_SUCCESS;
}

bool cast_sr_pair_supported(ftar_dtype_t src, ftar_dtype_t dst) { return is_cast_wide(src) && is_f8(dst); }

ftar_status_t launch_cast_scaled_sr(const void* src, ftar_dtype_t src_dt, void* dst, ftar_dtype_t dst_dt,
                                    size_t count, const float* scale, const unsigned long long* seed,
                                    unsigned long long offset, unsigned* amax, hipStream_t s) {
  if (!cast_sr_pair_supported(src_dt, dst_dt)) return FTAR_ERR_UNSUPPORTED;
  if (count == 0) return FTAR_SUCCESS;
  if (!src || !dst || !seed) return FTAR_ERR_INVALID_ARG;
  FTAR_CHECK_HIP((launch_cast_any<kCastU16, kCastU32, kCastLayout, SrGen>(src, src_dt, dst, dst_dt, count, scale, amax,
                                                                          s, SrGen::Arg{seed, offset})));
  return FTAR_SUCCESS;
}

}  // namespace ftar
