// The MX block-scaled casts of ftar_mx_scales / ftar_mx_quantize / ftar_mx_quantize_sr / ftar_mx_dequantize
// (mx_impl.h).  A translation unit of its own, as cast_kernels.hip is: its kernels compile beside the casts', whose
// code does not change.  The stochastic quantize (SrGen) is instantiated here for kMxCompute and kMxGiven; the
// words-array form (SrWords) only in the bench library.
#include "mx_impl.h"

namespace ftar {

bool mx_pair_supported(ftar_dtype_t wide, ftar_dtype_t f8) { return is_cast_wide(wide) && is_f8(f8); }

namespace {
// MODE: kMxScales (dst unused), kMxCompute, kMxGiven; the caller has refused what the header refuses
template <int MODE>
ftar_status_t mx_quant(const void* src, ftar_dtype_t src_dt, void* dst, ftar_dtype_t f8_dt, size_t count,
                       int headroom, unsigned char* scales, hipStream_t s) {
  if (!mx_pair_supported(src_dt, f8_dt)) return FTAR_ERR_UNSUPPORTED;
  if (count == 0) return FTAR_SUCCESS;
  if (!src || !scales || (!dst && MODE != kMxScales)) return FTAR_ERR_INVALID_ARG;
  FTAR_CHECK_HIP(mx_with_pair(src_dt, f8_dt, [&](auto w, auto f) {
    return launch_mx_quant_pair<decltype(w), decltype(f), MODE>(src, dst, scales, count, headroom, s);
  }));
  return FTAR_SUCCESS;
}
}  // namespace

ftar_status_t launch_mx_quantize_sr(const void* src, ftar_dtype_t src_dt, void* dst, ftar_dtype_t f8_dt, size_t count,
                                    bool given, int headroom, unsigned char* scales, const unsigned long long* seed,
                                    unsigned long long offset, hipStream_t s) {
  if (!mx_pair_supported(src_dt, f8_dt)) return FTAR_ERR_UNSUPPORTED;
  if (!seed) return FTAR_ERR_INVALID_ARG;
  if (count == 0) return FTAR_SUCCESS;
  if (!src || !scales || !dst) return FTAR_ERR_INVALID_ARG;
  const SrGen::Arg rnd{seed, offset};
  FTAR_CHECK_HIP(mx_with_pair(src_dt, f8_dt, [&](auto w, auto f) {
    using W = decltype(w);
    using F = decltype(f);
    return given ? launch_mx_quant_pair<W, F, kMxGiven, SrGen>(src, dst, scales, count, headroom, s, rnd)
                 : launch_mx_quant_pair<W, F, kMxCompute, SrGen>(src, dst, scales, count, headroom, s, rnd);
  }));
  return FTAR_SUCCESS;
}

ftar_status_t launch_mx_scales(const void* src, ftar_dtype_t src_dt, ftar_dtype_t f8_dt, size_t count, int headroom,
                               unsigned char* scales, hipStream_t s) {
  return mx_quant<kMxScales>(src, src_dt, nullptr, f8_dt, count, headroom, scales, s);
}

ftar_status_t launch_mx_quantize(const void* src, ftar_dtype_t src_dt, void* dst, ftar_dtype_t f8_dt, size_t count,
                                 bool given, int headroom, unsigned char* scales, hipStream_t s) {
  return given ? mx_quant<kMxGiven>(src, src_dt, dst, f8_dt, count, headroom, scales, s)
               : mx_quant<kMxCompute>(src, src_dt, dst, f8_dt, count, headroom, scales, s);
}

ftar_status_t launch_mx_dequantize(const void* src, ftar_dtype_t f8_dt, const unsigned char* scales, void* dst,
                                   ftar_dtype_t dst_dt, size_t count, hipStream_t s) {
  if (!mx_pair_supported(dst_dt, f8_dt)) return FTAR_ERR_UNSUPPORTED;
  if (count == 0) return FTAR_SUCCESS;
  if (!src || !scales || !dst) return FTAR_ERR_INVALID_ARG;
  FTAR_CHECK_HIP(mx_with_pair(dst_dt, f8_dt, [&](auto w, auto f) {
    return launch_mx_dequant_pair<decltype(f), decltype(w)>(src, scales, dst, count, s);
  }));
  return FTAR_SUCCESS;
}

}  // namespace ftar
