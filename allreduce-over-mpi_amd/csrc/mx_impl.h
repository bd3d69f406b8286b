// MX block-scaled casts for gfx950 (MI355X): wide (f32, bf16, f16) <-> OCP fp8 (e4m3, e5m2) with one E8M0 scale
// byte per block of FTAR_MX_BLOCK = 32 elements (ftar_mx_scales, ftar_mx_quantize, ftar_mx_dequantize;
// include/ftar.h has the contract in integers).
//
//   a    = max over the block of bits(widen(src[i])) & 0x7fffffff
//   s    = a >= 0x7f800000 ? 255 : min(254, max(0, (a >> 23) - emax + (mantissa(a) > 0x600000)) + headroom)
//   dst  = cvt_fp8(mul_rn_f32(widen(src[i]), q(s)))          quantize,   q(s) = 2^(127 - s), q(255) = 1
//   dst  = round_to_dst(mul_rn_f32(widen(src[i]), d(s)))     dequantize, d(s) = 2^(s - 127), d(255) = NaN
//
// The widening, the multiply (a value of its own in a register: cast_mul) and the narrowing are the scaled casts'
// (cast_impl.h: CastF32, CastH16, CastF8), so every block equals ftar_cast_scaled on that block with r = q(s) or
// d(s).  The power-of-two scale goes through that multiply, not through gfx950's v_cvt_scalef32_* conversions:
// their rounding and saturation are not measured here.
//
// Shape: kLayWide's.  Lane q of a pass owns wide vector q (16 bytes: 4 f32 or 8 16-bit elements) and its 4 or 8
// fp8 bytes, so a block is 8 neighbouring lanes (f32) or 4 (16-bit) and a wave's pass covers 8 or 16 whole blocks.
// The block's peak is an unsigned max of sign-cleared keys -- the fp32 bits, or the 16-bit encodings, which order
// as their widened values do and are widened once, after the max -- across those lanes by DPP (quad_perm for
// lanes ^ 1 and ^ 2, row_half_mirror for the other quad of 8): no LDS, no barrier.  The wave's 8 or 16 scale bytes
// are gathered into the lanes whose byte starts a store of the widest size the scales pointer's alignment allows
// (mx_store_scales: f32 one 8-byte store per wave and pass, 16-bit four dwords from one store instruction; 4, 2
// or 1 bytes at a time on a pointer aligned so).  The last workgroup tile is guarded: its lanes past the end hold
// zeros (the max's identity), the lane on the partial last vector moves its elements one by one, and its scale
// bytes go out one per group leader.  The vector kernels need src and dst 16-byte aligned (a block then starts a vector); any other
// call runs the element-wise kernels, one block per lane, which store the same bits.
//
// ftar_mx_quantize_sr: the quantize side's narrowing takes cast_impl.h's rounding policy (RneRound, SrGen, SrWords);
// the stochastic kernels (mx_quant_vec_sr_kernel, mx_quant_elem_sr_kernel; kMxCompute and kMxGiven) hash the call
// index of every element they store, so the word of element i is U(*seed, offset + i) in either family, any tile
// and any lane.  The scale bytes are computed before the narrowing and do not depend on it.
#pragma once
#include "cast_impl.h"

namespace ftar {
namespace {

constexpr int kMxBlock = FTAR_MX_BLOCK;
constexpr int kMxScales = 0, kMxCompute = 1, kMxGiven = 2;   // a quantize-side kernel: scales only / both / payload only
constexpr int kMxThreads = 256;

// ---- the contract's three integer functions ---------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned mx_scale_of(unsigned a, int emax, int headroom) {
  int e = (int)(a >> 23) - emax + ((a & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = (e < 0 ? 0 : e) + headroom;
  return a >= 0x7f800000u ? 255u : (unsigned)(e > 254 ? 254 : e);
}
__host__ __device__ __forceinline__ unsigned mx_q_bits(unsigned s) {
  return s <= 253u ? (254u - s) << 23 : s == 254u ? 0x00400000u : 0x3f800000u;
}
__host__ __device__ __forceinline__ unsigned mx_d_bits(unsigned s) {
  return s == 0u ? 0x00400000u : s == 255u ? 0x7fc00000u : s << 23;
}

// ---- a block's peak: a key per element that orders as |widen(x)| does, and the fp32 bits of the winning key
template <class Src>
struct MxPeak;
template <>
struct MxPeak<CastF32> {
  __device__ static unsigned s_key(float x) { return __float_as_uint(x) & 0x7fffffffu; }
  __device__ static unsigned v_key(u32x4 x) {
    x &= 0x7fffffffu;
    return umax(umax(x.x, x.y), umax(x.z, x.w));
  }
  __device__ static unsigned bits(unsigned k) { return k; }
};
template <class F>
struct MxPeak<CastH16<F>> {
  __device__ static unsigned s_key(unsigned short x) { return x & 0x7fffu; }
  __device__ static unsigned v_key(u32x4 x) {
    x &= 0x7fff7fffu;
    const unsigned m = pk_umax16(pk_umax16(x.x, x.y), pk_umax16(x.z, x.w));
    return umax(m & 0xffffu, m >> 16);
  }
  __device__ static unsigned bits(unsigned k) { return __float_as_uint(F::widen((unsigned short)k)); }
};

// the max over LANES (4 or 8) neighbouring lanes, in every one of them; a lane the exec mask has off gives 0
template <int LANES>
__device__ __forceinline__ unsigned mx_group_max(unsigned k) {
  static_assert(LANES == 4 || LANES == 8, "a block is 4 or 8 lanes");
  k = umax(k, (unsigned)__builtin_amdgcn_update_dpp(0, (int)k, 0xB1, 0xF, 0xF, false));     // quad_perm [1,0,3,2]
  k = umax(k, (unsigned)__builtin_amdgcn_update_dpp(0, (int)k, 0x4E, 0xF, 0xF, false));     // quad_perm [2,3,0,1]
  if constexpr (LANES == 8)
    k = umax(k, (unsigned)__builtin_amdgcn_update_dpp(0, (int)k, 0x141, 0xF, 0xF, false));  // row_half_mirror
  return k;
}

// The widest power-of-two store (bytes), at most `cap`, that a pointer's alignment allows.
inline int mx_store_width(const void* p, int cap) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  int w = 1;
  while (w < cap && !(a & (uintptr_t)(2 * w - 1))) w *= 2;
  return w;
}

// The widest store (bytes) of a wave's scale bytes a pointer's alignment allows: up to 8 (LPB = 8) or 4 (LPB = 4).
template <int LPB>
inline int mx_scale_store_width(const void* p) { return mx_store_width(p, LPB == 8 ? 8 : 4); }

// The wave's 64 / LPB scale bytes (byte j in every lane of group j), stored W at a time at p[0 .. 64 / LPB).
//   LPB = 8 (f32): the 8 bytes are read out of the group leaders (v_readlane) into two scalar words, and the lanes
//     whose byte starts a W-byte run store it: one 8-byte store per wave and pass when the pointer is aligned so.
//   LPB = 4 (16-bit): a DPP row of 16 lanes is 4 blocks, so the row's first lane collects its 4 bytes by row_shl
//     4 / 8 / 12 -- VALU only -- and stores a dword: 16 contiguous bytes per wave and pass from four lanes of one
//     store instruction.  Collecting all 16 in one lane by 16 v_readlane and their scalar packing ran
//     ftar_mx_scales at 4.87 TB/s where this runs it at the rate DESIGN §4 gives.
template <int LPB>
__device__ __forceinline__ void mx_store_scales(unsigned char* p, unsigned s, int W) {
  const unsigned lane = threadIdx.x & 63, j = lane / LPB;
  if (W == 1) {
    if (lane % LPB == 0) p[j] = (unsigned char)s;
    return;
  }
  if constexpr (LPB == 4) {
    // row_shl:n (dpp_ctrl 0x100 + n): lane i reads lane i + n of its row
    const unsigned lo = s | ((unsigned)__builtin_amdgcn_update_dpp(0, (int)s, 0x104, 0xF, 0xF, false) << 8);
    if (W == 2) {
      if (lane % 8 == 0) *reinterpret_cast<unsigned short*>(p + j) = (unsigned short)lo;
    } else {
      const unsigned w = lo | ((unsigned)__builtin_amdgcn_update_dpp(0, (int)s, 0x108, 0xF, 0xF, false) << 16) |
                         ((unsigned)__builtin_amdgcn_update_dpp(0, (int)s, 0x10C, 0xF, 0xF, false) << 24);
      if (lane % 16 == 0) *reinterpret_cast<unsigned*>(p + j) = w;
    }
  } else {
    unsigned w[2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
      w[d] = (unsigned)__builtin_amdgcn_readlane((int)s, (4 * d) * LPB) |
             ((unsigned)__builtin_amdgcn_readlane((int)s, (4 * d + 1) * LPB) << 8) |
             ((unsigned)__builtin_amdgcn_readlane((int)s, (4 * d + 2) * LPB) << 16) |
             ((unsigned)__builtin_amdgcn_readlane((int)s, (4 * d + 3) * LPB) << 24);
    if (lane % (LPB * W) != 0) return;
    const unsigned mine = j >> 2 ? w[1] : w[0];
    if (W == 2) *reinterpret_cast<unsigned short*>(p + j) = (unsigned short)(mine >> (8 * (j & 3)));
    else if (W == 4) *reinterpret_cast<unsigned*>(p + j) = mine;
    else *reinterpret_cast<u32x2*>(p + j) = u32x2{w[0], w[1]};
  }
}

// the first m (< 16 / sizeof(S)) elements of a 16-byte vector, one by one; the rest zero
template <class S>
__device__ __forceinline__ u32x4 mx_load_part(const S* p, int m) {
  constexpr int EPV = 16 / sizeof(S);
  struct {
    S e[EPV];
  } t;
#pragma unroll
  for (int j = 0; j < EPV; ++j) t.e[j] = j < m ? p[j] : S{};
  return __builtin_bit_cast(u32x4, t);
}
template <class S>
__device__ __forceinline__ void mx_store_part(S* p, u32x4 v, int m) {
  constexpr int EPV = 16 / sizeof(S);
  struct T {
    S e[EPV];
  };
  const T t = __builtin_bit_cast(T, v);
#pragma unroll
  for (int j = 0; j < EPV; ++j)
    if (j < m) p[j] = t.e[j];
}

// ---- quantize side: one workgroup tile of NI x BS wide vectors starting at vector q0 ------------------------
// rd: the narrowing's rounding (cast_impl.h); its words are indexed by the call index of each chunk's first element,
// q * EPV for vector q's chunk 0 -- in the unguarded and the guarded tile, on the partial last vector (whose spare
// elements' words are computed and dropped with their bytes) and in every pass of the grid-stride loop alike.
template <class Src, class Dst, int NI, int BS, int MODE, bool GUARD, class Rd = RneRound>
__device__ __forceinline__ void mx_quant_tile(const typename Src::S* src, unsigned char* dst, unsigned char* scales,
                                              size_t q0, size_t count, int headroom, int W,
                                              const Rd& rd = Rd{typename Rd::Arg{}}) {
  using S = typename Src::S;
  constexpr int EPV = 16 / sizeof(S);        // elements of a wide vector: 4 / 8
  constexpr int LPB = kMxBlock / EPV;        // lanes of a block: 8 / 4
  constexpr int NC = EPV / 4;                // fp8 dwords of a wide vector
  constexpr int kEmax = std::is_same_v<Dst, CastE5M2> ? 15 : 8;
  const size_t nfull = count / EPV;
  const int rem = (int)(count % EPV);
  const u32x4* sv = reinterpret_cast<const u32x4*>(src);
  u32x4 in[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const size_t q = q0 + (size_t)i * BS + threadIdx.x;
    in[i] = u32x4{0, 0, 0, 0};
    if (!GUARD || q < nfull) {
      in[i] = ld16<true>(sv + q);
    } else if (q == nfull) {
      in[i] = mx_load_part<S>(src + q * EPV, rem);
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const size_t q = q0 + (size_t)i * BS + threadIdx.x;
    const bool live = !GUARD || q * EPV < count;   // the vector holds an element
    unsigned s;
    if constexpr (MODE == kMxGiven) {
      s = live ? scales[q / LPB] : 0u;
    } else {   // every lane of the wave takes part: the lanes past the end hold zeros
      s = mx_scale_of(MxPeak<Src>::bits(mx_group_max<LPB>(MxPeak<Src>::v_key(in[i]))), kEmax, headroom);
      if constexpr (GUARD) {
        if (live && threadIdx.x % LPB == 0) scales[q / LPB] = (unsigned char)s;
      } else {
        mx_store_scales<LPB>(scales + (q0 + (size_t)i * BS + (threadIdx.x & ~63u)) / LPB, s, W);
      }
    }
    if constexpr (MODE != kMxScales) {
      const float r = __uint_as_float(mx_q_bits(s));
      u32x4 out = {0, 0, 0, 0};
      if constexpr (NC == 2) cast_chunks<Src, Dst, 0, 2>(&in[i], &out, r, rd, q * EPV);
      else cast_put<Dst>(&out, 0, cast_mul(__builtin_bit_cast(f32x4, in[i]), r), rd, q * EPV);
      if (!GUARD || q < nfull) {
        if constexpr (NC == 1) __builtin_nontemporal_store(out.x, reinterpret_cast<unsigned*>(dst) + q);
        else __builtin_nontemporal_store(u32x2{out.x, out.y}, reinterpret_cast<u32x2*>(dst) + q);
      } else if (q == nfull) {
        mx_store_part<unsigned char>(dst + q * EPV, out, rem);
      }
    }
  }
}

// All of a call whose src and dst are 16-byte aligned: tiles of NI x BS wide vectors (grid-stride beyond the grid's
// cap), the last one guarded when the count does not fill it.
template <class Src, class Dst, int NI, int BS, int MODE>
__global__ void __launch_bounds__(BS)
    mx_quant_vec_kernel(const void* src, void* dst, unsigned char* scales, size_t count, int headroom, int W) {
  using S = typename Src::S;
  constexpr size_t EPV = 16 / sizeof(S), T = (size_t)NI * BS;
  const size_t nq = (count + EPV - 1) / EPV, full = (count / EPV) / T, tiles = (nq + T - 1) / T;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform over the workgroup
    if (t < full)
      mx_quant_tile<Src, Dst, NI, BS, MODE, false>(static_cast<const S*>(src), static_cast<unsigned char*>(dst), scales,
                                                   t * T, count, headroom, W);
    else
      mx_quant_tile<Src, Dst, NI, BS, MODE, true>(static_cast<const S*>(src), static_cast<unsigned char*>(dst), scales,
                                                  t * T, count, headroom, W);
  }
}
// The stochastic twin (kMxCompute, kMxGiven): the same loop over the same tiles, the words' source (Rd: SrGen /
// SrWords) built from its argument as cast_vec_sr_kernel's is.  A kernel of its own and not a shared body: the
// round-to-nearest kernel above keeps its symbol, its arguments and, instruction for instruction, its code (a
// shared always-inline body between the two changed its block order and address arithmetic).
template <class Rd, class Src, class Dst, int NI, int BS, int MODE>
__global__ void __launch_bounds__(BS)
    mx_quant_vec_sr_kernel(const void* src, void* dst, unsigned char* scales, size_t count, int headroom, int W,
                           typename Rd::Arg rnd) {
  static_assert(MODE != kMxScales, "scale bytes do not depend on the rounding");
  using S = typename Src::S;
  constexpr size_t EPV = 16 / sizeof(S), T = (size_t)NI * BS;
  const size_t nq = (count + EPV - 1) / EPV, full = (count / EPV) / T, tiles = (nq + T - 1) / T;
  const Rd rd(rnd);
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // uniform over the workgroup
    if (t < full)
      mx_quant_tile<Src, Dst, NI, BS, MODE, false>(static_cast<const S*>(src), static_cast<unsigned char*>(dst), scales,
                                                   t * T, count, headroom, W, rd);
    else
      mx_quant_tile<Src, Dst, NI, BS, MODE, true>(static_cast<const S*>(src), static_cast<unsigned char*>(dst), scales,
                                                  t * T, count, headroom, W, rd);
  }
}

// element-wise: one block per lane
template <class Src, class Dst, int MODE>
__global__ void __launch_bounds__(kThreads)
    mx_quant_elem_kernel(const void* src, void* dst, unsigned char* scales, size_t count, int headroom) {
  using S = typename Src::S;
  constexpr int kEmax = std::is_same_v<Dst, CastE5M2> ? 15 : 8;
  const S* s = static_cast<const S*>(src);
  unsigned char* d = static_cast<unsigned char*>(dst);
  const size_t nblocks = (count + kMxBlock - 1) / kMxBlock, stride = (size_t)gridDim.x * kThreads;
  for (size_t b = (size_t)blockIdx.x * kThreads + threadIdx.x; b < nblocks; b += stride) {
    const size_t e0 = b * kMxBlock;
    const int m = count - e0 < (size_t)kMxBlock ? (int)(count - e0) : kMxBlock;
    unsigned sb;
    if constexpr (MODE == kMxGiven) {
      sb = scales[b];
    } else {
      unsigned k = 0;
      for (int j = 0; j < m; ++j) k = umax(k, MxPeak<Src>::s_key(s[e0 + j]));
      sb = mx_scale_of(MxPeak<Src>::bits(k), kEmax, headroom);
      scales[b] = (unsigned char)sb;
    }
    if constexpr (MODE != kMxScales) {
      const float r = __uint_as_float(mx_q_bits(sb));
      for (int j = 0; j < m; ++j) d[e0 + j] = Dst::narrow(cast_mul(Src::widen(s[e0 + j]), r));
    }
  }
}
// its stochastic twin, a kernel of its own for the reason above
template <class Rd, class Src, class Dst, int MODE>
__global__ void __launch_bounds__(kThreads)
    mx_quant_elem_sr_kernel(const void* src, void* dst, unsigned char* scales, size_t count, int headroom,
                            typename Rd::Arg rnd) {
  static_assert(MODE != kMxScales, "scale bytes do not depend on the rounding");
  using S = typename Src::S;
  constexpr int kEmax = std::is_same_v<Dst, CastE5M2> ? 15 : 8;
  const S* s = static_cast<const S*>(src);
  unsigned char* d = static_cast<unsigned char*>(dst);
  const Rd rd(rnd);
  const size_t nblocks = (count + kMxBlock - 1) / kMxBlock, stride = (size_t)gridDim.x * kThreads;
  for (size_t b = (size_t)blockIdx.x * kThreads + threadIdx.x; b < nblocks; b += stride) {
    const size_t e0 = b * kMxBlock;
    const int m = count - e0 < (size_t)kMxBlock ? (int)(count - e0) : kMxBlock;
    unsigned sb;
    if constexpr (MODE == kMxGiven) {
      sb = scales[b];
    } else {
      unsigned k = 0;
      for (int j = 0; j < m; ++j) k = umax(k, MxPeak<Src>::s_key(s[e0 + j]));
      sb = mx_scale_of(MxPeak<Src>::bits(k), kEmax, headroom);
      scales[b] = (unsigned char)sb;
    }
    const float r = __uint_as_float(mx_q_bits(sb));
    for (int j = 0; j < m; ++j)   // element e0 + j of the call takes word e0 + j
      d[e0 + j] = SrFmt<std::is_same_v<Dst, CastE5M2>>::narrow(cast_mul(Src::widen(s[e0 + j]), r), rd.word(e0 + j));
  }
}

// ---- dequantize side --------------------------------------------------------------------------------------
template <class Src, class Dst, int NI, int BS, bool GUARD>
__device__ __forceinline__ void mx_dequant_tile(const unsigned char* src, const unsigned char* scales,
                                                typename Dst::S* dst, size_t q0, size_t count) {
  using S = typename Dst::S;
  constexpr int EPV = 16 / sizeof(S), LPB = kMxBlock / EPV, NC = EPV / 4;
  using N = std::conditional_t<NC == 1, unsigned, u32x2>;   // the fp8 side's 4- / 8-byte access
  const size_t nfull = count / EPV;
  const int rem = (int)(count % EPV);
  u32x4 in[NI];
  unsigned sb[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const size_t q = q0 + (size_t)i * BS + threadIdx.x;
    in[i] = u32x4{0, 0, 0, 0};
    sb[i] = 0;
    if (!GUARD || q < nfull) {
      const N x = __builtin_nontemporal_load(reinterpret_cast<const N*>(src) + q);
      if constexpr (NC == 1) in[i].x = x;
      else {
        in[i].x = x.x;
        in[i].y = x.y;
      }
    } else if (q == nfull) {
      in[i] = mx_load_part<unsigned char>(src + q * EPV, rem);
    }
    if (!GUARD || q * EPV < count) sb[i] = scales[q / LPB];
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const size_t q = q0 + (size_t)i * BS + threadIdx.x;
    if (GUARD && q * EPV >= count) continue;
    const float r = __uint_as_float(mx_d_bits(sb[i]));
    const RneRound rd{RneRound::Arg{}};
    u32x4 out = {0, 0, 0, 0};
    if constexpr (NC == 2) cast_chunks<Src, Dst, 0, 2>(&in[i], &out, r, rd, 0);
    else out = __builtin_bit_cast(u32x4, cast_mul(Src::get(&in[i], 0), r));
    if (!GUARD || q < nfull) st16<true>(reinterpret_cast<u32x4*>(dst) + q, out);
    else mx_store_part<S>(dst + q * EPV, out, rem);
  }
}
template <class Src, class Dst, int NI, int BS>
__global__ void __launch_bounds__(BS)
    mx_dequant_vec_kernel(const void* src, const unsigned char* scales, void* dst, size_t count) {
  using S = typename Dst::S;
  constexpr size_t EPV = 16 / sizeof(S), T = (size_t)NI * BS;
  const size_t nq = (count + EPV - 1) / EPV, full = (count / EPV) / T, tiles = (nq + T - 1) / T;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (t < full)
      mx_dequant_tile<Src, Dst, NI, BS, false>(static_cast<const unsigned char*>(src), scales, static_cast<S*>(dst),
                                               t * T, count);
    else
      mx_dequant_tile<Src, Dst, NI, BS, true>(static_cast<const unsigned char*>(src), scales, static_cast<S*>(dst),
                                              t * T, count);
  }
}
template <class Src, class Dst>
__global__ void __launch_bounds__(kThreads)
    mx_dequant_elem_kernel(const void* src, const unsigned char* scales, void* dst, size_t count) {
  const unsigned char* s = static_cast<const unsigned char*>(src);
  typename Dst::S* d = static_cast<typename Dst::S*>(dst);
  const size_t nblocks = (count + kMxBlock - 1) / kMxBlock, stride = (size_t)gridDim.x * kThreads;
  for (size_t b = (size_t)blockIdx.x * kThreads + threadIdx.x; b < nblocks; b += stride) {
    const size_t e0 = b * kMxBlock;
    const int m = count - e0 < (size_t)kMxBlock ? (int)(count - e0) : kMxBlock;
    const float r = __uint_as_float(mx_d_bits(scales[b]));
    for (int j = 0; j < m; ++j) d[e0 + j] = Dst::narrow(cast_mul(Src::widen(s[e0 + j]), r));
  }
}

// ---- launchers --------------------------------------------------------------------------------------------
inline bool mx_aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }
inline unsigned mx_vec_blocks(size_t count, size_t elems_per_tile) {
  size_t blocks = (count + elems_per_tile - 1) / elems_per_tile;
  if (blocks > 0x7fffffffull) blocks = 0x7fffffffull;
  return (unsigned)(blocks ? blocks : 1);
}

// Wide vectors per lane and pass (NI): 4 for both widths -- 16 f32 or 32 16-bit elements in flight per lane.
constexpr int kMxNI = 4;

template <class Src, class Dst, int MODE, class Rd = RneRound>
hipError_t launch_mx_quant_pair(const void* src, void* dst, unsigned char* scales, size_t count, int headroom,
                                hipStream_t s, typename Rd::Arg rnd = {}) {
  constexpr size_t EPV = 16 / sizeof(typename Src::S);
  if constexpr (Rd::kSr) {   // the same choice of family and the same grids, the stochastic twins
    if (mx_aligned16(src) && mx_aligned16(dst)) {
      FTAR_LAUNCH((mx_quant_vec_sr_kernel<Rd, Src, Dst, kMxNI, kMxThreads, MODE>),
                  dim3(mx_vec_blocks(count, kMxNI * kMxThreads * EPV)), dim3(kMxThreads), 0, s, src, dst, scales, count,
                  headroom, mx_scale_store_width<kMxBlock / (int)EPV>(scales), rnd);
    } else {
      FTAR_LAUNCH((mx_quant_elem_sr_kernel<Rd, Src, Dst, MODE>), dim3(elem_blocks((count + kMxBlock - 1) / kMxBlock)),
                  dim3(kThreads), 0, s, src, dst, scales, count, headroom, rnd);
    }
  } else if (mx_aligned16(src) && (MODE == kMxScales || mx_aligned16(dst))) {
    FTAR_LAUNCH((mx_quant_vec_kernel<Src, Dst, kMxNI, kMxThreads, MODE>),
                dim3(mx_vec_blocks(count, kMxNI * kMxThreads * EPV)), dim3(kMxThreads), 0, s, src, dst, scales, count,
                headroom, mx_scale_store_width<kMxBlock / (int)EPV>(scales));
  } else {
    FTAR_LAUNCH((mx_quant_elem_kernel<Src, Dst, MODE>), dim3(elem_blocks((count + kMxBlock - 1) / kMxBlock)),
                dim3(kThreads), 0, s, src, dst, scales, count, headroom);
  }
  return hipGetLastError();
}
template <class Src, class Dst>
hipError_t launch_mx_dequant_pair(const void* src, const unsigned char* scales, void* dst, size_t count,
                                  hipStream_t s) {
  constexpr size_t EPV = 16 / sizeof(typename Dst::S);
  if (mx_aligned16(src) && mx_aligned16(dst)) {
    FTAR_LAUNCH((mx_dequant_vec_kernel<Src, Dst, kMxNI, kMxThreads>),
                dim3(mx_vec_blocks(count, kMxNI * kMxThreads * EPV)), dim3(kMxThreads), 0, s, src, scales, dst, count);
  } else {
    FTAR_LAUNCH((mx_dequant_elem_kernel<Src, Dst>), dim3(elem_blocks((count + kMxBlock - 1) / kMxBlock)),
                dim3(kThreads), 0, s, src, scales, dst, count);
  }
  return hipGetLastError();
}

// the wide format and the fp8 format of a supported pair, as types
template <class Fn>
hipError_t mx_with_pair(ftar_dtype_t wide, ftar_dtype_t f8, Fn&& fn) {
  auto with_f8 = [&](auto w) {
    return f8 == FTAR_FLOAT8_E5M2 ? fn(w, CastE5M2{}) : fn(w, CastE4M3{});
  };
  switch (wide) {
    case FTAR_FLOAT32: return with_f8(CastF32{});
    case FTAR_BFLOAT16: return with_f8(CastBf16{});
    default: return with_f8(CastF16{});
  }
}

}  // namespace
}  // namespace ftar
