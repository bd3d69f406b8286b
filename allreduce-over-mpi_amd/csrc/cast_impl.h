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

// ---- the narrowing's rounding: RNE as above (RneRound, an empty policy: the kernels compile as without it), or
// stochastic (ftar_cast_scaled_sr, include/ftar.h): sr_dst(p, U) with one 32-bit word U per element, a pure
// function of the device seed and the global element index (SrGen), or read from an array (SrWords: the bench
// library's hook for the sweep and the edge tests).
//
// Above the format's smallest normal value the instruction v_cvt_sr_fp8_f32 / v_cvt_sr_bf8_f32 IS the contract,
// fed U as it is: it adds the top 23 - m bits of its operand under the dropped mantissa bits, lets the carry run
// into the next encoding and past the largest finite one into NaN (e4m3) / inf (e5m2), and turns inf and NaN into
// what the contract names -- all 2^32 inputs x six words, the input's own thresholds among them
// (tools/sr_sweep.py).  Below it the instruction keeps fewer bits of the fraction than the contract's
// 32 (it rounds down under 2^32 - 1 and under the threshold word where the contract rounds up), so that range,
// zero included, is computed beside it for the lanes that need it: |p| x 2^(m - emin) is exact and lies in
// [0, 2^m), its integer part is the encoding, its fraction times 2^32, truncated, is F, and the carry of F + U
// adds one.
template <bool E5M2>
struct SrFmt {
  static constexpr int kM = E5M2 ? 2 : 3, kBias = E5M2 ? 15 : 7, kDrop = 23 - kM;
  static constexpr unsigned kMinNormal = (unsigned)(127 + 1 - kBias) << 23;   // fp32 bits of 2^emin
  template <int BYTE>
  __device__ static unsigned hw(float p, unsigned u, unsigned old) {   // into byte BYTE of old
    if constexpr (E5M2) return __builtin_amdgcn_cvt_sr_bf8_f32(p, u, old, BYTE);
    else return __builtin_amdgcn_cvt_sr_fp8_f32(p, u, old, BYTE);
  }
  __device__ static unsigned sub(float p, unsigned u) {                // |p| < 2^emin: the byte
    const float y = __builtin_fabsf(p) * __uint_as_float((unsigned)(127 + kM - 1 + kBias) << 23);
    const unsigned f = (unsigned)(__builtin_amdgcn_fractf(y) * 4294967296.0f);
    return ((__float_as_uint(p) >> 24) & 0x80u) | ((unsigned)y + (f + u < f ? 1u : 0u));
  }
  template <int BYTE>
  __device__ static unsigned put(float p, unsigned u, unsigned old) {
    const unsigned w = hw<BYTE>(p, u, old);
    if ((__float_as_uint(p) & 0x7fffffffu) >= kMinNormal) return w;
    return (w & ~(0xffu << (8 * BYTE))) | (sub(p, u) << (8 * BYTE));
  }
  __device__ static unsigned char narrow(float p, unsigned u) { return (unsigned char)put<0>(p, u, 0u); }
  __device__ static unsigned pack(f32x4 v, u32x4 u) {
    return put<3>(v.w, u.w, put<2>(v.z, u.z, put<1>(v.y, u.y, put<0>(v.x, u.x, 0u))));
  }
};

struct RneRound {
  static constexpr bool kSr = false;
  struct Arg {};
  __device__ explicit RneRound(Arg) {}
};
// U(seed, g), g = offset + the call's element index (ftar.h writes it out; tests/sr_ref.py restates it): two
// keys from the 64-bit seed through the splitmix64 finaliser, once per lane and call; per element a two-multiply
// 32-bit hash of the low index word, the second key and the high index word entering between its rounds.
struct SrGen {
  static constexpr bool kSr = true;
  struct Arg {
    const unsigned long long* seed;
    unsigned long long offset;
  };
  unsigned ka, kb;
  unsigned long long base;
  __device__ explicit SrGen(Arg a) : base(a.offset) {
    unsigned long long z = *a.seed + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    ka = (unsigned)z;
    kb = (unsigned)(z >> 32);
  }
  __device__ unsigned word(size_t e) const {
    const unsigned long long g = base + e;
    unsigned x = (unsigned)g ^ ka;
    x = (x ^ (x >> 16)) * 0x7feb352du;
    x += kb ^ ((unsigned)(g >> 32) * 0x9E3779B9u);
    x = (x ^ (x >> 15)) * 0x846ca68bu;
    return x ^ (x >> 16);
  }
};
struct SrWords {
  static constexpr bool kSr = true;
  struct Arg {
    const unsigned* words;
    size_t count;
  };
  Arg a;
  __device__ explicit SrWords(Arg a_) : a(a_) {}
  __device__ unsigned word(size_t e) const { return e < a.count ? a.words[e] : 0u; }   // a guarded tile's spare lanes
};

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
// chunk c (4 elements, the first at call index e) into out[]: the format's own RNE, or sr_dst on the element's word
template <class Dst, class Rd>
__device__ __forceinline__ void cast_put(u32x4* out, int c, f32x4 p, const Rd& rd, size_t e) {
  if constexpr (Rd::kSr) {
    static_assert(Dst::kVecs == 1, "stochastic rounding narrows to fp8 only");
    out[0][c] = SrFmt<std::is_same_v<Dst, CastE5M2>>::pack(p, u32x4{rd.word(e), rd.word(e + 1), rd.word(e + 2), rd.word(e + 3)});
  } else {
    Dst::put(out, c, p);
  }
}
// chunks [C0, C0 + NC) of 16 elements: in[] -> out[]; e0: the call index of chunk 0's first element
template <class Src, class Dst, int C0 = 0, int NC = 4, class Rd = RneRound>
__device__ __forceinline__ void cast_chunks(const u32x4* in, u32x4* out, float r, const Rd& rd, size_t e0) {
#pragma unroll
  for (int c = C0; c < C0 + NC; ++c) cast_put<Dst>(out, c, cast_mul(Src::get(in, c), r), rd, e0 + 4 * c);
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
template <class Src, class Dst, class Am, class Rd>
__device__ __forceinline__ void cast_elem(const void* src, void* dst, size_t e, float r, Am& am, const Rd& rd) {
  const float p = cast_mul(Src::widen(static_cast<const typename Src::S*>(src)[e]), r);
  typename Dst::S o;
  if constexpr (Rd::kSr) o = SrFmt<std::is_same_v<Dst, CastE5M2>>::narrow(p, rd.word(e));
  else o = Dst::narrow(p);
  static_cast<typename Dst::S*>(dst)[e] = o;
  if constexpr (!std::is_same_v<Am, NoAmax>) am.key = Dst::Key::key_max(am.key, Dst::Key::s_key(o));
}

// One workgroup tile of U x BS fp8 vectors starting at vector t0; GUARD: the one partial tile.  head: the call
// index of vector 0's first element (what the rounding's words are indexed by).
template <class Src, class Dst, int U, int BS, int LAY, bool GUARD, class Am, class Rd>
__device__ __forceinline__ void cast_tile(const u32x4* s, u32x4* d, size_t t0, size_t nvec, float r, Am& am,
                                          u32x4* stage, const Rd& rd, size_t head) {
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
        cast_chunks<Src, Dst, 0, 2>(&in[i], &out, r, rd, head + q * 8);
      } else if constexpr (kQuant) {           // an f32 source vector: chunk 0
        cast_put<Dst>(&out, 0, cast_mul(__builtin_bit_cast(f32x4, in[i]), r), rd, head + q * 4);
      } else if constexpr (DV == 2) {
        cast_chunks<Src, Dst, 0, 2>(&in[i], &out, r, rd, head + q * 8);
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
      cast_chunks<Src, Dst>(in[u], out, r, rd, head + v * 16);
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
template <class Src, class Dst, int U, int BS, int LAY, class Am, class Rd = RneRound>
__device__ __forceinline__ void cast_vec_body(const void* src, void* dst, size_t nvec, int head, int tail,
                                              const float* scale, Am am, const Rd rd = Rd{typename Rd::Arg{}}) {
  constexpr int WV = Src::kVecs > Dst::kVecs ? Src::kVecs : Dst::kVecs;
  __shared__ u32x4 stage[LAY == kLayLds ? BS * WV : 1];
  const float r = scale ? *scale : 1.0f;
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * 16 + (threadIdx.x - head);
    cast_elem<Src, Dst>(src, dst, e, r, am, rd);
  }
  const u32x4* s = reinterpret_cast<const u32x4*>(static_cast<const typename Src::S*>(src) + head);
  u32x4* d = reinterpret_cast<u32x4*>(static_cast<typename Dst::S*>(dst) + head);
  constexpr size_t T = (size_t)U * BS;
  const size_t full = nvec / T, tiles = (nvec + T - 1) / T;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform over the workgroup
    if (t < full) cast_tile<Src, Dst, U, BS, LAY, false>(s, d, t * T, nvec, r, am, stage, rd, (size_t)head);
    else cast_tile<Src, Dst, U, BS, LAY, true>(s, d, t * T, nvec, r, am, stage, rd, (size_t)head);
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

// the stochastic twins: the same bodies, the words' source (Rd: SrGen / SrWords) built from its argument
template <class Rd, class Src, class Dst, int U, int BS, int LAY>
__global__ void __launch_bounds__(BS)
    cast_vec_sr_kernel(const void* src, void* dst, size_t nvec, int head, int tail, const float* scale,
                       typename Rd::Arg rnd) {
  cast_vec_body<Src, Dst, U, BS, LAY>(src, dst, nvec, head, tail, scale, NoAmax{}, Rd(rnd));
}
template <class Rd, class Src, class Dst, int U, int BS, int LAY>
__global__ void __launch_bounds__(BS)
    cast_vec_sr_amax_kernel(const void* src, void* dst, size_t nvec, int head, int tail, const float* scale,
                            typename Rd::Arg rnd, unsigned* amax) {
  cast_vec_body<Src, Dst, U, BS, LAY>(src, dst, nvec, head, tail, scale, AmaxFin<typename Dst::Key>{1.0f, amax}, Rd(rnd));
}

// element-wise: a pair whose pointers are not co-aligned
template <class Src, class Dst, class Am, class Rd = RneRound>
__device__ __forceinline__ void cast_elem_body(const void* src, void* dst, size_t n, const float* scale, Am am,
                                               const Rd rd = Rd{typename Rd::Arg{}}) {
  const float r = scale ? *scale : 1.0f;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) cast_elem<Src, Dst>(src, dst, e, r, am, rd);
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

template <class Rd, class Src, class Dst>
__global__ void __launch_bounds__(kThreads)
    cast_elem_sr_kernel(const void* src, void* dst, size_t n, const float* scale, typename Rd::Arg rnd) {
  cast_elem_body<Src, Dst>(src, dst, n, scale, NoAmax{}, Rd(rnd));
}
template <class Rd, class Src, class Dst>
__global__ void __launch_bounds__(kThreads)
    cast_elem_sr_amax_kernel(const void* src, void* dst, size_t n, const float* scale, typename Rd::Arg rnd,
                             unsigned* amax) {
  cast_elem_body<Src, Dst>(src, dst, n, scale, AmaxFin<typename Dst::Key>{1.0f, amax}, Rd(rnd));
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

template <class Src, class Dst, int U, int LAY, class Rd = RneRound>
hipError_t launch_cast_pair(const void* src, void* dst, size_t count, const float* scale, unsigned* amax,
                            hipStream_t s, typename Rd::Arg rnd = {}) {
  constexpr bool kQuant = Dst::kVecs == 1;
  const Split16 sp = kQuant ? split_cast(dst, src, sizeof(typename Src::S), count)
                            : split_cast(src, dst, sizeof(typename Dst::S), count);
  if constexpr (Rd::kSr) {   // the same split and grids, the stochastic twins
    if (!sp.co_aligned) {
      if (amax) FTAR_LAUNCH((cast_elem_sr_amax_kernel<Rd, Src, Dst>), dim3(elem_blocks(count)), dim3(kThreads), 0, s,
                            src, dst, count, scale, rnd, amax);
      else FTAR_LAUNCH((cast_elem_sr_kernel<Rd, Src, Dst>), dim3(elem_blocks(count)), dim3(kThreads), 0, s, src, dst,
                       count, scale, rnd);
      return hipGetLastError();
    }
    constexpr size_t T = (size_t)U * kCastThreads;
    size_t blocks = (sp.nvec + T - 1) / T;
    if (blocks == 0) blocks = 1;
    if (blocks > 0x7fffffffull) blocks = 0x7fffffffull;
    if (amax) FTAR_LAUNCH((cast_vec_sr_amax_kernel<Rd, Src, Dst, U, kCastThreads, LAY>), dim3((unsigned)blocks),
                          dim3(kCastThreads), 0, s, src, dst, sp.nvec, sp.head, sp.tail, scale, rnd, amax);
    else FTAR_LAUNCH((cast_vec_sr_kernel<Rd, Src, Dst, U, kCastThreads, LAY>), dim3((unsigned)blocks),
                     dim3(kCastThreads), 0, s, src, dst, sp.nvec, sp.head, sp.tail, scale, rnd);
    return hipGetLastError();
  }
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
template <int U16, int U32, int LAY, class Rd = RneRound>
hipError_t launch_cast_any(const void* src, ftar_dtype_t sdt, void* dst, ftar_dtype_t ddt, size_t count,
                           const float* scale, unsigned* amax, hipStream_t s, typename Rd::Arg rnd = {}) {
  auto with_f8 = [&](auto wide, bool quant, bool e5m2) {
    using W = decltype(wide);
    constexpr int U = W::kVecs == 4 ? U32 : U16;
    if (quant)
      return e5m2 ? launch_cast_pair<W, CastE5M2, U, LAY, Rd>(src, dst, count, scale, amax, s, rnd)
                  : launch_cast_pair<W, CastE4M3, U, LAY, Rd>(src, dst, count, scale, amax, s, rnd);
    if constexpr (Rd::kSr) return hipErrorInvalidValue;   // quantize pairs only
    else return e5m2 ? launch_cast_pair<CastE5M2, W, U, LAY>(src, dst, count, scale, amax, s)
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

// What production runs (cast_kernels.hip; the bench library's words hook runs the same): the layout and the fp8
// vectors per lane and pass, measured cold on 256 MiB of wide data (tools/cast_rates.py; DESIGN §4 has every
// candidate's rate, profiles/cast/ the logs): lane-contiguous 16-byte wide accesses with 4- / 8-byte fp8 accesses
// won or tied every pair against the lane-owned vectors, staged through LDS or not (whose lane-strided wide stores
// ran f8 -> f32 at 1.5 TB/s); f8 -> f32 gained 8 % from 4 vectors per lane over 2.
constexpr int kCastLayout = kLayWide;
constexpr int kCastU16 = 2, kCastU32 = 4;

}  // namespace
}  // namespace ftar
