// The scaled casts of ftar_cast_scaled (wide <-> fp8, cast_impl.h) in the layout production runs.  A translation
// unit of its own, as reduce_f8.hip and reduce_amax.hip are: its kernels compile beside the folds'.
#include "cast_impl.h"

namespace ftar {

namespace {
// The layout and the fp8 vectors per lane and pass, measured cold on 256 MiB of wide data (tools/cast_rates.py;
// DESIGN §4 has every candidate's rate, profiles/cast/ the logs): lane-contiguous 16-byte wide accesses with 4- /
// 8-byte fp8 accesses won or tied every pair against the lane-owned vectors, staged through LDS or not (whose
// lane-strided wide stores ran f8 -> f32 at 1.5 TB/s); f8 -> f32 gained 8 % from 4 vectors per lane over 2.
constexpr int kCastLayout = kLayWide;
constexpr int kCastU16 = 2, kCastU32 = 4;
}  // namespace

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

}  // namespace ftar
