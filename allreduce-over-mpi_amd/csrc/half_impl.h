// Stochastic rounding of f32 to the two 16-bit floats for gfx950 (MI355X): ftar_cast_half_sr (include/ftar.h), the
// sending end of a bf16 / fp16 gradient wire.
//
//   dst[i] = sr16(mul_rn_f32(src[i], r), U(*seed, offset + i)),  r = scale ? *scale : 1.0f
//
// The product is cast_mul's (one correctly rounded multiply in a register of its own); the word is SrGen's (or
// SrWords', the bench library's hook), indexed by the call's element index whichever kernel, tile or lane stores it.
//
// Shape.  A tile family of its own: cast_tile takes fp8 as one side (16 elements per 16-byte vector).  Here one
// 16-byte destination vector holds 8 elements and takes two 16-byte f32 source vectors.  `head` elements (0..7)
// bring dst to 16-byte alignment; if src + head is then 16-byte aligned too the vector kernel runs, workgroup 0 doing
// the head and the tail element-wise in the same launch; otherwise the element-wise kernel runs.  Two layouts of the
// vector kernel (DESIGN §4 has the A/B):
//   kHalfWide  lane-contiguous 16-byte f32 loads, 8-byte 16-bit stores: source vector q is 4 elements of its own;
//   kHalfOwn   each lane owns one destination vector and its 32 contiguous source bytes: 16-byte accesses on both
//              sides, the source side lane-strided.
// Included by cast_kernels.hip (production: kHalfLayout) and bench_kernels.hip (the words hook, the A/B, the sweep).
#pragma once
#include "cast_impl.h"

namespace ftar {
namespace {

constexpr int kHalfWide = 0, kHalfOwn = 1;
// how a 16-bit value is narrowed: the contract in integers everywhere, or the instruction fed the word as it is
// with the contract beside it in the range where the two differ (below SrH16::kMinNormal)
constexpr int kSrInt = 0, kSrHw = 1;

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// sr16(p, U) (ftar.h): BF = bf16 (m = 7, emin = -126), else IEEE binary16 (m = 10, emin = -14).
//
// In integers, on a = |p|'s bits.  bf16 shares f32's exponent range, so 16 bits are dropped over the whole finite
// range, f32 subnormals included: the encoding is a >> 16 plus the carry of (a << 16) + U, which runs from the
// largest finite encoding into inf's; inf has no dropped bits and stays; a NaN is answered apart, because its
// carry could run through 0x7fff into -0.  f16 drops 13 bits from 2^-14 on: the encoding is (a - (112 << 23)) >> 13
// plus the carry of (a << 19) + U, capped at inf's (65536 and above, inf included, land there before the carry).
// Below 2^-14 the ulp stays 2^-24: |p| x 2^24 is exact and lies in [0, 2^10), its integer part is the encoding, its
// fraction times 2^32, truncated, is F, and the carry of F + U adds one (SrFmt::sub's construction).
//
// The instructions v_cvt_sr_bf16_f32 / v_cvt_sr_f16_f32 (op_sel: the half written), fed U as it is, held against
// that on all 2^32 inputs under the words 0, 2^32 - 1, the input's threshold and the threshold minus one, in both
// halves (tools/sr_sweep.py --half): v_cvt_sr_bf16_f32 IS the contract everywhere -- fp32 subnormals, the
// carry into inf, inf and NaN included -- so bf16 runs it bare.  v_cvt_sr_f16_f32 is the contract from 2^-14 on (the
// band up to 65536, everything above, inf and NaN included) and below 2^-56, where both store a signed zero; between
// them, f16's subnormal range, it keeps fewer bits of the fraction than the contract's 32 (it rounds down under
// 2^32 - 1 and under the threshold word where the contract rounds up).  Fed U >> (32 - d) either instruction misses
// in every binade.  kSrHw runs the instruction and computes the integer form beside it for the lanes below 2^-14.
template <bool BF>
struct SrH16 {
  static constexpr int kM = BF ? 7 : 10, kDrop = 23 - kM;
  static constexpr unsigned kNan = BF ? 0x7fc0u : 0x7e00u, kInf = BF ? 0x7f80u : 0x7c00u;
  static constexpr unsigned kMinNormal = BF ? 0u : 0x38800000u;     // fp32 bits of f16's 2^-14; kSrHw: the integer
                                                                    // form answers |p| below it

  __device__ static unsigned soft(float p, unsigned u) {   // the 16-bit encoding
    const unsigned b = __float_as_uint(p), a = b & 0x7fffffffu, sign = (b >> 16) & 0x8000u;
    unsigned enc;
    if constexpr (BF) {
      const unsigned lo = a << 16;
      enc = (a >> 16) + (lo + u < lo ? 1u : 0u);
    } else {
      const unsigned lo = a << 19;
      const unsigned up = ((a - 0x38000000u) >> 13) + (lo + u < lo ? 1u : 0u), nrm = up < kInf ? up : kInf;
      const float y = __uint_as_float(a < kMinNormal ? a : 0u) * 16777216.0f;   // exact, in [0, 2^10)
      const unsigned f = (unsigned)(__builtin_amdgcn_fractf(y) * 4294967296.0f);
      const unsigned sub = (unsigned)y + (f + u < f ? 1u : 0u);
      enc = a >= kMinNormal ? nrm : sub;
    }
    return sign | (a > 0x7f800000u ? kNan : enc);
  }
  template <int HI>
  __device__ static unsigned hw(float p, unsigned u, unsigned old) {   // into half HI of old
    if constexpr (BF) return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_sr_bf16_f32(__builtin_bit_cast(bf16x2, old), p, u, HI != 0));
    else return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_sr_f16_f32(__builtin_bit_cast(f16x2, old), p, u, HI != 0));
  }
  template <int MODE, int HI>
  __device__ static unsigned put(float p, unsigned u, unsigned old) {
    constexpr unsigned keep = HI ? 0x0000ffffu : 0xffff0000u;
    if constexpr (MODE == kSrInt) {
      return (old & keep) | (soft(p, u) << (16 * HI));
    } else {
      const unsigned w = hw<HI>(p, u, old), a = __float_as_uint(p) & 0x7fffffffu;
      if (a >= kMinNormal) return w;
      return (w & keep) | (soft(p, u) << (16 * HI));
    }
  }
  template <int MODE>
  __device__ static unsigned short narrow(float p, unsigned u) { return (unsigned short)put<MODE, 0>(p, u, 0u); }
  template <int MODE>
  __device__ static u32x2 pack(f32x4 v, u32x4 u) {
    return u32x2{put<MODE, 1>(v.y, u.y, put<MODE, 0>(v.x, u.x, 0u)), put<MODE, 1>(v.w, u.w, put<MODE, 0>(v.z, u.z, 0u))};
  }
};

// The destination as the amax finish sees it (reduce_impl.h: two u16 lanes of |encoding| per word).
template <bool BF>
using HalfKey = H16SumT<std::conditional_t<BF, Bf16Fmt<kHwBf16>, HalfFmt>>;

template <bool BF, class Am>
__device__ __forceinline__ void half_note(Am& am, u32x2 o) {
  if constexpr (!std::is_same_v<Am, NoAmax>) am.key = HalfKey<BF>::key_max(am.key, HalfKey<BF>::v_key(u32x4{o.x, o.y, 0u, 0u}));
}
// four elements, the first at call index e: the product, then sr16 on each element's word
template <bool BF, int MODE, class Rd>
__device__ __forceinline__ u32x2 half_put4(u32x4 in, float r, const Rd& rd, size_t e) {
  return SrH16<BF>::template pack<MODE>(cast_mul(__builtin_bit_cast(f32x4, in), r),
                                        u32x4{rd.word(e), rd.word(e + 1), rd.word(e + 2), rd.word(e + 3)});
}
template <bool BF, int MODE, class Am, class Rd>
__device__ __forceinline__ void half_elem(const float* src, unsigned short* dst, size_t e, float r, Am& am, const Rd& rd) {
  const unsigned short o = SrH16<BF>::template narrow<MODE>(cast_mul(__builtin_nontemporal_load(src + e), r), rd.word(e));
  __builtin_nontemporal_store(o, dst + e);
  if constexpr (!std::is_same_v<Am, NoAmax>) am.key = HalfKey<BF>::key_max(am.key, HalfKey<BF>::s_key(o));
}

// One workgroup tile of U x BS destination vectors starting at vector t0 (s, d: the vectorised range's first
// source / destination vector); GUARD: the one partial tile.  head: the call index of vector 0's first element.
template <bool BF, int MODE, int U, int BS, int LAY, bool GUARD, class Am, class Rd>
__device__ __forceinline__ void half_tile(const u32x4* s, u32x4* d, size_t t0, size_t nvec, float r, Am& am,
                                          const Rd& rd, size_t head) {
  if constexpr (LAY == kHalfWide) {
    const size_t q0 = t0 * 2, nq = nvec * 2;        // source vectors: 4 elements, 8 destination bytes each
    u32x4 in[U * 2];
#pragma unroll
    for (int i = 0; i < U * 2; ++i) {
      const size_t q = q0 + (size_t)i * BS + threadIdx.x;
      in[i] = (GUARD && q >= nq) ? u32x4{0, 0, 0, 0} : ld16<true>(s + q);
    }
#pragma unroll
    for (int i = 0; i < U * 2; ++i) {
      const size_t q = q0 + (size_t)i * BS + threadIdx.x;
      if (GUARD && q >= nq) continue;
      const u32x2 out = half_put4<BF, MODE>(in[i], r, rd, head + q * 4);
      half_note<BF>(am, out);
      __builtin_nontemporal_store(out, reinterpret_cast<u32x2*>(d) + q);
    }
  } else {
    u32x4 in[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = t0 + (size_t)u * BS + threadIdx.x;
#pragma unroll
      for (int j = 0; j < 2; ++j) in[u][j] = (GUARD && v >= nvec) ? u32x4{0, 0, 0, 0} : ld16<true>(s + v * 2 + j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = t0 + (size_t)u * BS + threadIdx.x;
      if (GUARD && v >= nvec) continue;
      const u32x2 lo = half_put4<BF, MODE>(in[u][0], r, rd, head + v * 8);
      const u32x2 hi = half_put4<BF, MODE>(in[u][1], r, rd, head + v * 8 + 4);
      half_note<BF>(am, lo);
      half_note<BF>(am, hi);
      st16<true>(d + v, u32x4{lo.x, lo.y, hi.x, hi.y});
    }
  }
}

// Element range [head, head + nvec * 8) is vectorised, tile by tile of U x BS destination vectors (grid-stride
// beyond the grid's cap); workgroup 0 also does the `head` leading and `tail` trailing elements element-wise.
template <bool BF, int MODE, int U, int BS, int LAY, class Am, class Rd>
__device__ __forceinline__ void half_vec_body(const float* src, unsigned short* dst, size_t nvec, int head, int tail,
                                              const float* scale, Am am, const Rd rd) {
  const float r = scale ? *scale : 1.0f;
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * 8 + (threadIdx.x - head);
    half_elem<BF, MODE>(src, dst, e, r, am, rd);
  }
  const u32x4* s = reinterpret_cast<const u32x4*>(src + head);
  u32x4* d = reinterpret_cast<u32x4*>(dst + head);
  constexpr size_t T = (size_t)U * BS;
  const size_t full = nvec / T, tiles = (nvec + T - 1) / T;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform over the workgroup
    if (t < full) half_tile<BF, MODE, U, BS, LAY, false>(s, d, t * T, nvec, r, am, rd, (size_t)head);
    else half_tile<BF, MODE, U, BS, LAY, true>(s, d, t * T, nvec, r, am, rd, (size_t)head);
  }
  if constexpr (!std::is_same_v<Am, NoAmax>) amax_flush(am);
}
template <class Rd, bool BF, int MODE, int U, int BS, int LAY>
__global__ void __launch_bounds__(BS)
    half_vec_sr_kernel(const float* src, unsigned short* dst, size_t nvec, int head, int tail, const float* scale,
                       typename Rd::Arg rnd) {
  half_vec_body<BF, MODE, U, BS, LAY>(src, dst, nvec, head, tail, scale, NoAmax{}, Rd(rnd));
}
template <class Rd, bool BF, int MODE, int U, int BS, int LAY>
__global__ void __launch_bounds__(BS)
    half_vec_sr_amax_kernel(const float* src, unsigned short* dst, size_t nvec, int head, int tail, const float* scale,
                            typename Rd::Arg rnd, unsigned* amax) {
  half_vec_body<BF, MODE, U, BS, LAY>(src, dst, nvec, head, tail, scale, AmaxFin<HalfKey<BF>>{1.0f, amax}, Rd(rnd));
}

// element-wise: a pair whose pointers are not co-aligned
template <bool BF, int MODE, class Am, class Rd>
__device__ __forceinline__ void half_elem_body(const float* src, unsigned short* dst, size_t n, const float* scale,
                                               Am am, const Rd rd) {
  const float r = scale ? *scale : 1.0f;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) half_elem<BF, MODE>(src, dst, e, r, am, rd);
  if constexpr (!std::is_same_v<Am, NoAmax>) amax_flush(am);
}
template <class Rd, bool BF, int MODE>
__global__ void __launch_bounds__(kThreads)
    half_elem_sr_kernel(const float* src, unsigned short* dst, size_t n, const float* scale, typename Rd::Arg rnd) {
  half_elem_body<BF, MODE>(src, dst, n, scale, NoAmax{}, Rd(rnd));
}
template <class Rd, bool BF, int MODE>
__global__ void __launch_bounds__(kThreads)
    half_elem_sr_amax_kernel(const float* src, unsigned short* dst, size_t n, const float* scale, typename Rd::Arg rnd,
                             unsigned* amax) {
  half_elem_body<BF, MODE>(src, dst, n, scale, AmaxFin<HalfKey<BF>>{1.0f, amax}, Rd(rnd));
}

// `head` elements up to dst's first 16-byte aligned address, 8 elements per vector; co_aligned if src + head is
// 16-byte aligned there too (both pointers element-aligned: the caller's contract).
inline Split16 split_half(const void* src, const void* dst, size_t count) {
  size_t head = ((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / 2;
  if ((reinterpret_cast<uintptr_t>(dst) & 1) || ((reinterpret_cast<uintptr_t>(src) + head * 4) & 15)) return {false};
  if (head > count) head = count;
  const size_t nvec = (count - head) / 8;
  return {true, (int)head, (int)(count - head - nvec * 8), nvec};
}

template <class Rd, bool BF, int MODE, int U, int LAY>
hipError_t launch_half_sr(const void* src_, void* dst_, size_t count, const float* scale, unsigned* amax, hipStream_t s,
                          typename Rd::Arg rnd) {
  const float* src = static_cast<const float*>(src_);
  unsigned short* dst = static_cast<unsigned short*>(dst_);
  const Split16 sp = split_half(src, dst, count);
  if (!sp.co_aligned) {
    if (amax) FTAR_LAUNCH((half_elem_sr_amax_kernel<Rd, BF, MODE>), dim3(elem_blocks(count)), dim3(kThreads), 0, s, src,
                          dst, count, scale, rnd, amax);
    else FTAR_LAUNCH((half_elem_sr_kernel<Rd, BF, MODE>), dim3(elem_blocks(count)), dim3(kThreads), 0, s, src, dst, count,
                     scale, rnd);
    return hipGetLastError();
  }
  constexpr size_t T = (size_t)U * kCastThreads;
  size_t blocks = (sp.nvec + T - 1) / T;
  if (blocks == 0) blocks = 1;  // head / tail only
  if (blocks > 0x7fffffffull) blocks = 0x7fffffffull;
  if (amax) FTAR_LAUNCH((half_vec_sr_amax_kernel<Rd, BF, MODE, U, kCastThreads, LAY>), dim3((unsigned)blocks),
                        dim3(kCastThreads), 0, s, src, dst, sp.nvec, sp.head, sp.tail, scale, rnd, amax);
  else FTAR_LAUNCH((half_vec_sr_kernel<Rd, BF, MODE, U, kCastThreads, LAY>), dim3((unsigned)blocks), dim3(kCastThreads),
                   0, s, src, dst, sp.nvec, sp.head, sp.tail, scale, rnd);
  return hipGetLastError();
}

inline bool half_sr_pair(ftar_dtype_t src, ftar_dtype_t dst) {
  return src == FTAR_FLOAT32 && (dst == FTAR_BFLOAT16 || dst == FTAR_FLOAT16);
}

// What production runs (cast_kernels.hip; the bench library's words hook runs the same): the narrowing (the sweep
// above), the layout and the destination vectors per lane and pass, measured cold on 256 MiB of f32
// (tools/cast_rates.py --half; DESIGN §4 has every candidate's rate): lane-contiguous f32 loads at 2 vectors per lane
// won both destinations (bf16 6.35 TB/s against 6.16 for the lane-owned vectors, f16 5.89 against 5.76), and the
// instruction beat the integer form by 5 % (bf16) and 8 % (f16).  The other candidates stay in the bench library.
constexpr int kHalfSrMode = kSrHw;
constexpr int kHalfLayout = kHalfWide;
constexpr int kHalfU = 2;

template <class Rd, int MODE = kHalfSrMode, int U = kHalfU, int LAY = kHalfLayout>
hipError_t launch_half_sr_any(const void* src, void* dst, ftar_dtype_t ddt, size_t count, const float* scale,
                              unsigned* amax, hipStream_t s, typename Rd::Arg rnd) {
  return ddt == FTAR_BFLOAT16 ? launch_half_sr<Rd, true, MODE, U, LAY>(src, dst, count, scale, amax, s, rnd)
                              : launch_half_sr<Rd, false, MODE, U, LAY>(src, dst, count, scale, amax, s, rnd);
}

}  // namespace
}  // namespace ftar
