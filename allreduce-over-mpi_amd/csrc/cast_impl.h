// Scaled casts for gfx950 (MI355X): wide (f32, bf16, f16) <-> OCP fp8 (e4m3, e5m2), times a scale held in device
// memory, optionally with the abs-max of what is stored (ftar_cast_scaled, include/ftar.h).
//
//   dst[i] = cvt_dst(mul_rn_f32(widen(src[i]), r)),  r = scale ? *scale : 1.0f
//
// Widening is exact; the product is one correctly rounded fp32 multiply (subnormal products kept) that lands in
// a register of its own before any narrowing reads it (the guard of H16SumT::s_scale: no v_fma_mix* may fuse
// the two roundings into one); the narrowing is the folds' own (F8Fmt::narrow2, pack_f16, pack_bf16): torch's
// (src.to(float32) * r).to(dst_dtype) bit for bit, no saturation.
//
// Shape: one narrow-side 16-byte vector is 16 elements, 64 B on an f32 side and 32 B on a 16-bit side.  `head`
// elements bring the fp8 pointer to 16-byte alignment; if the wide pointer is then 16-byte aligned too the pair
// is co-aligned and the vector kernel runs, workgroup 0 doing the head and the tail element-wise in the same
// launch; otherwise the element-wise kernel runs.  Three layouts of the vector kernel (DESIGN §4 has the A/B):
//   kLayOwn   each lane owns one fp8 vector and its 64 / 32 contiguous wide bytes: 16-byte accesses on both
//             sides, the wide side lane-strided;
//   kLayLds   the same ownership, the wide side moved lane-contiguously and transposed through LDS;
//   kLayWide  lane-contiguous 16-byte wide accesses, 4- / 8-byte fp8 accesses.
// Included by cast_kernels.hip (production: kCastLayout) and bench_kernels.hip (the A/B hook).
#pragma once
#include "reduce_impl.h"

namespace ftar {
namespace {

constexpr int kLayOwn = 0, kLayLds = 1, kLayWide = 2;
constexpr int kCastThreads = 256;

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// One format as a cast sees it: S the element, kVecs the 16-byte vectors 16 elements take, Key the trait whose
// amax keys read the stored bits, widen / narrow one element, get / put chunk c (4 elements) of 16 in w[kVecs].
struct CastF32 {
  using S = float;
  using Key = F32Sum;
  static constexpr int kVecs = 4;
  __device__ static float widen(S x) { return x; }
  __device__ static S narrow(float p) { return p; }
  __device__ static f32x4 get(const u32x4* w, int c) { return __builtin_bit_cast(f32x4, w[c]); }
  __device__ static void put(u32x4* w, int c, f32x4 v) { w[c] = __builtin_bit_cast(u32x4, v); }
};
template <class F>
struct CastH16 {
  using S = unsigned short;
  using Key = H16SumT<F>;
  static constexpr int kVecs = 2;
  __device__ static float widen(S x) { return F::widen(x); }
  __device__ static S narrow(float p) { return (S)F::pack(p, p); }
  __device__ static f32x4 get(const u32x4* w, int c) {
    const u32x4 x = w[c >> 1];
    return (c & 1) ? F::unpack(x.z, x.w) : F::unpack(x.x, x.y);
  }
  __device__ static void put(u32x4* w, int c, f32x4 v) {
    const unsigned lo = F::pack(v.x, v.y), hi = F::pack(v.z, v.w);
    if (c & 1) {
      w[c >> 1].z = lo;
      w[c >> 1].w = hi;
    } else {
      w[c >> 1].x = lo;
      w[c >> 1].y = hi;
    }
  }
};
using CastBf16 = CastH16<Bf16Fmt<kHwBf16>>;
using CastF16 = CastH16<HalfFmt>;
template <bool E5M2>
struct CastF8 {
  using F = F8Fmt<E5M2>;
  using S = unsigned char;
  using Key = F8SumT<F>;
  static constexpr int kVecs = 1;
  __device__ static float widen(S x) { return F::widen(x); }
  __device__ static S narrow(float p) { return F::narrow(p); }
  __device__ static f32x4 get(const u32x4* w, int c) { return F::unpack(w[0][c]); }
  __device__ static void put(u32x4* w, int c, f32x4 v) { w[0][c] = F::pack(v); }
};
using CastE4M3 = CastF8<false>;
using CastE5M2 = CastF8<true>;

// the product, a value of its own in registers before the narrowing reads it
__device__ __forceinline__ f32x4 cast_mul(f32x4 a, float r) {
  f32x4 p = mul_rn(a, r);
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ float cast_mul(float a, float r) {
  float p = mul_rn(a, r);
  asm volatile("" : "+v"(p));
  return p;
}
// chunks [C0, C0 + NC) of 16 elements: in[] -> out[]
template <class Src, class Dst, int C0 = 0, int NC = 4>
__device__ __forceinline__ void cast_chunks(const u32x4* in, u32x4* out, float r) {
#pragma unroll
  for (int c = C0; c < C0 + NC; ++c) Dst::put(out, c, cast_mul(Src::get(in, c), r));
}

// The running key of the amax finish (AmaxFin's state and flush, reduce_impl.h), or nothing.
struct NoAmax {};
template <class Dst, class Am>
__device__ __forceinline__ void cast_note(Am& am, const u32x4* out, int nvecs) {
  if constexpr (!std::is_same_v<Am, NoAmax>) {
    using K = typename Dst::Key;
    for (int j = 0; j < nvecs; ++j) am.key = K::key_max(am.key, K::v_key(out[j]));
  }
}
template <class Src, class Dst, class Am>
__device__ __forceinline__ void cast_elem(const void* src, void* dst, size_t e, float r, Am& am) {
  const typename Dst::S o = Dst::narrow(cast_mul(Src::widen(static_cast<const typename Src::S*>(src)[e]), r));
  static_cast<typename Dst::S*>(dst)[e] = o;
  if constexpr (!std::is_same_v<Am, NoAmax>) am.key = Dst::Key::key_max(am.key, Dst::Key::s_key(o));
}

// One workgroup tile of U x BS fp8 vectors starting at vector t0; GUARD: the one partial tile.
template <class Src, class Dst, int U, int BS, int LAY, bool GUARD, class Am>
__device__ __forceinline__ void cast_tile(const u32x4* s, u32x4* d, size_t t0, size_t nvec, float r, Am& am,
                                          u32x4* stage) {
  constexpr int SV = Src::kVecs, DV = Dst::kVecs;
  constexpr bool kQuant = DV == 1;            // fp8 is the destination
  constexpr int WV = kQuant ? SV : DV;        // 16-byte vectors of the wide side per fp8 vector
  if constexpr (LAY == kLayWide) {
    // wide vector q holds 16 / WV elements: chunks [0, 4 / WV) of a 16-element group of its own
    constexpr int NC = 4 / WV;
    using N = std::conditional_t<NC == 1, unsigned, u32x2>;   // the fp8 side's 4- / 8-byte access
    const size_t q0 = t0 * WV, nq = nvec * WV;
    u32x4 in[U * WV];
#pragma unroll
    for (int i = 0; i < U * WV; ++i) {
      const size_t q = q0 + (size_t)i * BS + threadIdx.x;
      in[i] = u32x4{0, 0, 0, 0};
      if (GUARD && q >= nq) continue;
      if constexpr (kQuant) {
        in[i] = ld16<true>(s + q);
      } else {
        const N x = __builtin_nontemporal_load(reinterpret_cast<const N*>(s) + q);
        if constexpr (NC == 1) in[i].x = x;
        else {
          in[i].x = x.x;
          in[i].y = x.y;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < U * WV; ++i) {
      const size_t q = q0 + (size_t)i * BS + threadIdx.x;
      if (GUARD && q >= nq) continue;
      u32x4 out = {0, 0, 0, 0};
      if constexpr (kQuant && SV == 2) {       // a 16-bit source vector: chunks 0-1 of its own array
        cast_chunks<Src, Dst, 0, 2>(&in[i], &out, r);
      } else if constexpr (kQuant) {           // an f32 source vector: chunk 0
        Dst::put(&out, 0, cast_mul(__builtin_bit_cast(f32x4, in[i]), r));
      } else if constexpr (DV == 2) {
        cast_chunks<Src, Dst, 0, 2>(&in[i], &out, r);
      } else {
        out = __builtin_bit_cast(u32x4, cast_mul(Src::get(&in[i], 0), r));
      }
      cast_note<Dst>(am, &out, 1);
      if constexpr (!kQuant) {
        st16<true>(d + q, out);
      } else if constexpr (NC == 1) {
        __builtin_nontemporal_store(out.x, reinterpret_cast<unsigned*>(d) + q);
      } else {
        __builtin_nontemporal_store(u32x2{out.x, out.y}, reinterpret_cast<u32x2*>(d) + q);
      }
    }
  } else {
    u32x4 in[U][SV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = t0 + (size_t)u * BS + threadIdx.x;
      if constexpr (LAY == kLayLds && kQuant) {
        // the wave's 64 x WV wide vectors, lane-contiguous into LDS, each lane's own WV back out
        const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const size_t w0 = (t0 + (size_t)u * BS + wave * 64) * WV;
        u32x4* my = stage + wave * 64 * WV;
        __syncthreads();   // the previous pass has read its vectors
#pragma unroll
        for (int j = 0; j < WV; ++j) {
          const size_t q = w0 + j * 64 + lane;
          my[j * 64 + lane] = (GUARD && q >= nvec * WV) ? u32x4{0, 0, 0, 0} : ld16<true>(s + q);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WV; ++j) in[u][j] = my[lane * WV + j];
      } else {
#pragma unroll
        for (int j = 0; j < SV; ++j)
          in[u][j] = (GUARD && v >= nvec) ? u32x4{0, 0, 0, 0} : ld16<true>(s + v * SV + j);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = t0 + (size_t)u * BS + threadIdx.x;
      u32x4 out[DV];
      cast_chunks<Src, Dst>(in[u], out, r);
      if (!(GUARD && v >= nvec)) cast_note<Dst>(am, out, DV);
      if constexpr (LAY == kLayLds && !kQuant) {
        const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const size_t w0 = (t0 + (size_t)u * BS + wave * 64) * WV;
        u32x4* my = stage + wave * 64 * WV;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WV; ++j) my[lane * WV + j] = out[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WV; ++j) {
          const size_t q = w0 + j * 64 + lane;
          if (!(GUARD && q >= nvec * WV)) st16<true>(d + q, my[j * 64 + lane]);
        }
      } else {
        if (GUARD && v >= nvec) continue;
#pragma unroll
        for (int j = 0; j < DV; ++j) st16<true>(d + v * DV + j, out[j]);
      }
    }
  }
}

// Element range [head, head + nvec * 16) is vectorised, tile by tile of U x BS fp8 vectors (grid-stride beyond
// the grid's cap); workgroup 0 also does the `head` leading and `tail` trailing elements element-wise.
template <class Src, class Dst, int U, int BS, int LAY, class Am>
__device__ __forceinline__ void cast_vec_body(const void* src, void* dst, size_t nvec, int head, int tail,
                                              const float* scale, Am am) {
  constexpr int WV = Src::kVecs > Dst::kVecs ? Src::kVecs : Dst::kVecs;
  __shared__ u32x4 stage[LAY == kLayLds ? BS * WV : 1];
  const float r = scale ? *scale : 1.0f;
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * 16 + (threadIdx.x - head);
    cast_elem<Src, Dst>(src, dst, e, r, am);
  }
  const u32x4* s = reinterpret_cast<const u32x4*>(static_cast<const typename Src::S*>(src) + head);
  u32x4* d = reinterpret_cast<u32x4*>(static_cast<typename Dst::S*>(dst) + head);
  constexpr size_t T = (size_t)U * BS;
  const size_t full = nvec / T, tiles = (nvec + T - 1) / T;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform over the workgroup
    if (t < full) cast_tile<Src, Dst, U, BS, LAY, false>(s, d, t * T, nvec, r, am, stage);
    else cast_tile<Src, Dst, U, BS, LAY, true>(s, d, t * T, nvec, r, am, stage);
  }
  if constexpr (!std::is_same_v<Am, NoAmax>) amax_flush(am);
}
template <class Src, class Dst, int U, int BS, int LAY>
__global__ void __launch_bounds__(BS)
    cast_vec_kernel(const void* src, void* dst, size_t nvec, int head, int tail, const float* scale) {
  cast_vec_body<Src, Dst, U, BS, LAY>(src, dst, nvec, head, tail, scale, NoAmax{});
}
template <class Src, class Dst, int U, int BS, int LAY>
__global__ void __launch_bounds__(BS)
    cast_vec_amax_kernel(const void* src, void* dst, size_t nvec, int head, int tail, const float* scale,
                         unsigned* amax) {
  cast_vec_body<Src, Dst, U, BS, LAY>(src, dst, nvec, head, tail, scale, AmaxFin<typename Dst::Key>{1.0f, amax});
}

// element-wise: a pair whose pointers are not co-aligned
template <class Src, class Dst, class Am>
__device__ __forceinline__ void cast_elem_body(const void* src, void* dst, size_t n, const float* scale, Am am) {
  const float r = scale ? *scale : 1.0f;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) cast_elem<Src, Dst>(src, dst, e, r, am);
  if constexpr (!std::is_same_v<Am, NoAmax>) amax_flush(am);
}
template <class Src, class Dst>
__global__ void __launch_bounds__(kThreads) cast_elem_kernel(const void* src, void* dst, size_t n, const float* scale) {
  cast_elem_body<Src, Dst>(src, dst, n, scale, NoAmax{});
}
template <class Src, class Dst>
__global__ void __launch_bounds__(kThreads)
    cast_elem_amax_kernel(const void* src, void* dst, size_t n, const float* scale, unsigned* amax) {
  cast_elem_body<Src, Dst>(src, dst, n, scale, AmaxFin<typename Dst::Key>{1.0f, amax});
}

// split16's rule on two element sizes: `head` elements up to the fp8 side's first aligned address, co_aligned if
// the wide side is 16-byte aligned there too.
inline Split16 split_cast(const void* narrow, const void* wide, size_t wide_esz, size_t count) {
  size_t head = (16 - (reinterpret_cast<uintptr_t>(narrow) & 15)) & 15;
  if (head > count) head = count;
  if ((reinterpret_cast<uintptr_t>(wide) + head * wide_esz) & 15) return {false};
  const size_t nvec = (count - head) / 16;
  return {true, (int)head, (int)(count - head - nvec * 16), nvec};
}

template <class Src, class Dst, int U, int LAY>
hipError_t launch_cast_pair(const void* src, void* dst, size_t count, const float* scale, unsigned* amax,
                            hipStream_t s) {
  constexpr bool kQuant = Dst::kVecs == 1;
  const Split16 sp = kQuant ? split_cast(dst, src, sizeof(typename Src::S), count)
                            : split_cast(src, dst, sizeof(typename Dst::S), count);
  if (!sp.co_aligned) {
    if (amax) FTAR_LAUNCH((cast_elem_amax_kernel<Src, Dst>), dim3(elem_blocks(count)), dim3(kThreads), 0, s, src, dst,
                          count, scale, amax);
    else FTAR_LAUNCH((cast_elem_kernel<Src, Dst>), dim3(elem_blocks(count)), dim3(kThreads), 0, s, src, dst, count, scale);
    return hipGetLastError();
  }
  constexpr size_t T = (size_t)U * kCastThreads;
  size_t blocks = (sp.nvec + T - 1) / T;
  if (blocks == 0) blocks = 1;  // head / tail only
  if (blocks > 0x7fffffffull) blocks = 0x7fffffffull;
  if (amax) FTAR_LAUNCH((cast_vec_amax_kernel<Src, Dst, U, kCastThreads, LAY>), dim3((unsigned)blocks),
                        dim3(kCastThreads), 0, s, src, dst, sp.nvec, sp.head, sp.tail, scale, amax);
  else FTAR_LAUNCH((cast_vec_kernel<Src, Dst, U, kCastThreads, LAY>), dim3((unsigned)blocks), dim3(kCastThreads), 0, s,
                   src, dst, sp.nvec, sp.head, sp.tail, scale);
  return hipGetLastError();
}

inline bool is_f8(ftar_dtype_t dt) { return dt == FTAR_FLOAT8_E4M3 || dt == FTAR_FLOAT8_E5M2; }
inline bool is_cast_wide(ftar_dtype_t dt) { return dt == FTAR_FLOAT32 || dt == FTAR_BFLOAT16 || dt == FTAR_FLOAT16; }

// the 12 pairs; anything else: hipErrorInvalidValue (refused by the caller before).  U16 / U32: the fp8 vectors per
// lane and pass of the pairs whose wide side is 16-bit / f32.
template <int U16, int U32, int LAY>
hipError_t launch_cast_any(const void* src, ftar_dtype_t sdt, void* dst, ftar_dtype_t ddt, size_t count,
                           const float* scale, unsigned* amax, hipStream_t s) {
  auto with_f8 = [&](auto wide, bool quant, bool e5m2) {
    using W = decltype(wide);
    constexpr int U = W::kVecs == 4 ? U32 : U16;
    if (quant)
      return e5m2 ? launch_cast_pair<W, CastE5M2, U, LAY>(src, dst, count, scale, amax, s)
                  : launch_cast_pair<W, CastE4M3, U, LAY>(src, dst, count, scale, amax, s);
    return e5m2 ? launch_cast_pair<CastE5M2, W, U, LAY>(src, dst, count, scale, amax, s)
                : launch_cast_pair<CastE4M3, W, U, LAY>(src, dst, count, scale, amax, s);
  };
  const bool quant = is_f8(ddt);
  const ftar_dtype_t wide = quant ? sdt : ddt, f8 = quant ? ddt : sdt;
  if (!is_f8(f8) || !is_cast_wide(wide)) return hipErrorInvalidValue;
  const bool e5m2 = f8 == FTAR_FLOAT8_E5M2;
  switch (wide) {
    case FTAR_FLOAT32: return with_f8(CastF32{}, quant, e5m2);
    case FTAR_BFLOAT16: return with_f8(CastBf16{}, quant, e5m2);
    default: return with_f8(CastF16{}, quant, e5m2);
  }
}

}  // namespace
}  // namespace ftar
