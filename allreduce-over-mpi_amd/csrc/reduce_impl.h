// k-way element-wise reduce for gfx950 (MI355X).
//
// Replaces FlexTree::reduce_sum<T>/reduce_band<T> (allreduce_over_mpi/mpi_mod.hpp:812-1251)
// and the reference's never-wired GPU twin reduce_sum_1..20 (vector_add/reduce_sum_gpu.h:4-316).
//
//   dst[i] = src0[i] OP src1[i] OP ... OP src{k-1}[i]      strictly left to right
//
// Design (bandwidth-bound: (k+1)*n*sizeof(T) bytes, ~0 flops per byte, no MFMA):
//   * 16 B per lane per access, one wave instruction = 1 KiB contiguous per
//     source: fully coalesced;
//   * k = 2..16 for fp32/bf16/fp16, k = 2..8 for the other types: reduce_lds_kernel stages
//     U tiles of every source per wave through LDS with LDS-DMA
//     (global_load_lds_dwordx4, nontemporal) and folds tile by tile as each
//     tile lands (counted vmcnt); stores are nontemporal too (cold data: every
//     piece of an AllReduce is new); (U, waves per workgroup) per k below;
//   * other k / types: reduce_vec_kernel, registers, 2 vectors of every source
//     per lane in flight, runtime k up to FTAR_MAX_K;
//   * one-shot grids (>> 256 CUs); source pointers travel in the kernarg
//     segment (no device-side pointer table);
//   * unaligned heads/tails (block offsets need not be 16-B aligned) are done
//     element-wise by workgroup 0 in the same launch; sources whose alignment
//     differs from dst's take an element-wise kernel instead;
//   * dst may alias a source (the ring folds in place, mpi_mod.hpp:1699):
//     every lane loads its element of every source before it stores that
//     element, so no pointer is declared __restrict__;
//   * arithmetic follows the reference's C++ semantics bit for bit:
//       float/double in their own precision (no FMA: pure adds),
//       narrow integers wrap (promotion + truncating store == modular add),
//       bool sum = OR of non-zero;
//   * extensions (no reference): bf16, fp16 and OCP fp8 (e4m3, e5m2) sums = fp32 accumulate + one RNE per
//     reduce; MAX / MIN = signed or unsigned integer compare, IEEE 754-2019
//     maximum / minimum on floats (exact: every fold order gives the same bits); the scaled float sums
//     (AVG's root fold, ftar_reduce_scaled): the accumulator times r before the fold's one rounding --
//     one body per kernel family, two finishes (PlainFin / ScaledFin below).
#pragma once
// Internal: the reduce kernels, their traits and launchers, included by reduce_kernels.hip and reduce_f8.hip (the
// production dispatch, libftar.so) and bench_kernels.hip (the A/B harness, libftar_bench.so);
// anonymous namespace: each TU instantiates what it uses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "ftar_internal.h"

namespace ftar {

// The kernel the launchers below launched last on this thread (its host-side handle):
// ftar_debug_last_kernel names it, so bench.py reports PMC traffic only for the kernel it timed.
inline thread_local const void* g_last_kernel = nullptr;
#define FTAR_LAUNCH(KERNEL, ...)                                         \
  do {                                                                   \
    ::ftar::g_last_kernel = reinterpret_cast<const void*>(KERNEL);       \
    hipLaunchKernelGGL(KERNEL, __VA_ARGS__);                             \
  } while (0)
// A fold family in one of its finishes (PlainFin / ScaledFin / AmaxFin below), by SC (kFinPlain / kFinScaled /
// kFinAmax): NAME_kernel<TARGS>(args...), its twin NAME_scaled_kernel<TARGS>(args..., SCALE), or
// NAME_amax_kernel<TARGS>(args..., SCALE, AMAX).  TARGS is parenthesised; only the kernel launched is
// instantiated, so traits without a scaled or an amax finish never name one.
#define FTAR_TARGS(...) __VA_ARGS__
#define FTAR_LAUNCH_FIN(SC, SCALE, AMAX, NAME, TARGS, ...)                                                    \
  do {                                                                                                        \
    if constexpr ((SC) == 2) FTAR_LAUNCH((NAME##_amax_kernel<FTAR_TARGS TARGS>), __VA_ARGS__, SCALE, AMAX);   \
    else if constexpr ((SC) == 1) FTAR_LAUNCH((NAME##_scaled_kernel<FTAR_TARGS TARGS>), __VA_ARGS__, SCALE);  \
    else FTAR_LAUNCH((NAME##_kernel<FTAR_TARGS TARGS>), __VA_ARGS__);                                         \
  } while (0)

namespace {

constexpr int kFinPlain = 0, kFinScaled = 1, kFinAmax = 2;  // FTAR_LAUNCH_FIN's SC
constexpr int kThreads = 256;
constexpr int kTreeLevels = kMaxFoldLevels;
// Measured on MI355X with COLD data (tools/kbench_cold.py: launches rotate over
// 4 disjoint buffer sets, so nothing is left in the 256 MB Infinity Cache from
// the previous launch -- the AllReduce's situation, where every piece is new
// data; DESIGN.md §3, profiles/r01/kbench_cold*.log):
//  * nontemporal loads AND stores (f32 k = 2: 6.55 TB/s vs 6.09 with plain
//    stores; rewriting the same destination back to back -- the reference
//    harness's loop -- favours plain stores instead, because the MALL absorbs
//    part of the writes, a regime the hot path never sees);
//  * k = 2..16: staged through LDS (LDS-DMA, no VGPR landing zone) -- f32
//    +1 % at k = 2 and +3-5 % at k = 4..8 over the best register variant
//    (round 1); folding each tile as it lands instead of after all K x U
//    loads: +0.5-2 % for f32, up to +8 % for bf16 at k = 8 (round 2);
//  * larger k (runtime k): registers, 2 vectors per lane, 512-thread workgroups.
constexpr int kUnroll = 2;
constexpr int kVecThreads = 512;
constexpr bool kNtLoads = true, kNtStores = true;
#ifndef KHW_BF16_DEFAULT
#define KHW_BF16_DEFAULT true
#endif
#ifndef KLDS_DEEP_BF16
#define KLDS_DEEP_BF16 true
#endif
// Tiles per wave (U) and waves per workgroup (W) of the LDS-staged kernel by
// element size and k, from a cold-data sweep of 14 (U, W) shapes x k = 2..16
// x {f32, bf16} on MI355X (tools/kbench_cold.py variants 40-53,
// profiles/r02/kbench_cold_prog_shapes.log).  Up to k = 4 deep per-wave
// queues win (U = 3-4); from k = 5 on, two workgroups per CU of 2-6 waves.
// Round 2 added one-wave and two-wave workgroups of 1-4 tiles (variants 54-59,
// profiles/r02/kbench_cold_small_wg.log, kbench_k2_shape_ab.log): for 4-byte
// k = 2, U = 1 x W = 2 (4 KiB of LDS, up to 16 workgroups per CU) measured
// +0.6 / +1.3 / +1.8 % over U = 4 x W = 4 in three runs; elsewhere the table held.
// The fp16 sum and the MAX / MIN traits take the shapes of the sums of their width.  The 2-byte MAX / MIN on
// packed instructions (fp16, i16, u16: one VALU op per dword and source) run 0.5-1 % under the 2-byte sums at
// k = 8, at the rate of the 4-byte folds that are as light; a sweep of these shapes for them and an
// integer-key formulation gave no gain that held through the production dispatch (DESIGN §4,
// profiles/f16_minmax/).
template <class Tr, int K>
constexpr int kLdsTiles = sizeof(typename Tr::S) >= 4 ? (K == 2 ? 1 : K <= 4 ? 3 : K <= 6 ? 2 : K <= 10 ? 4 : 2)
                                                     : (K <= 4 ? 4 : K == 5 ? 2 : K == 6 ? 5 : K <= 10 ? 4 : 2);
template <class Tr, int K>
constexpr int kLdsWaves = sizeof(typename Tr::S) >= 4 ? (K == 2 ? 2 : K <= 6 ? 6 : K <= 10 ? 2 : 4)
                                                     : (K <= 4 ? 4 : K == 5 ? 5 : K <= 10 ? 2 : 4);
// LDS per workgroup = W waves x K x U x 1 KiB (<= 160 KiB): k = 16 at U = 2 stages 128 KiB

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ u32x4 ld16(const u32x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ void st16(u32x4* p, u32x4 v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
// RNE to bf16; NaN stays NaN (quieted, sign and top payload kept).  Written as
// a select, not an early return: a per-element NaN branch compiles to exec-mask
// save/restore around every conversion.
__device__ __forceinline__ unsigned bf16_round_bits(float f) {  // result in the high half
  const unsigned u = __float_as_uint(f);
  const unsigned rne = u + 0x7fffu + ((u >> 16) & 1u);
  return ((u & 0x7fffffffu) > 0x7f800000u ? (u | 0x00400000u) : rne) & 0xffff0000u;
}
__device__ __forceinline__ unsigned short f32_to_bf16(float f) { return (unsigned short)(bf16_round_bits(f) >> 16); }

// a * r rounded in a's own precision, whatever follows: with contraction allowed (hipcc's default) the
// compiler fuses an fp32 multiply into the conversion after it (v_fma_mixlo_f16: the exact product rounded
// once, to fp16), which is not the scaled finish's fp32 product followed by the fold's RNE
template <class A, class R>
__device__ __forceinline__ A mul_rn(A a, R r) {
#pragma clang fp contract(off)
  return a * r;
}

// The amax finish's keys (AmaxFin below): |encoding| as an unsigned integer is monotone in |value| in every float
// format here and every NAN encoding sorts above every number, so the running maximum is an integer max on
// the stored bits -- a u32 for fp32, two u16 lanes of a dword (v_pk_max_u16) for the 16- and 8-bit formats.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned pk_umax16(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned,
                            __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// ---------------------------------------------------------------------------
// element traits: scalar (S*) and 16-byte vector (V*) forms of one (dtype, op)
// ---------------------------------------------------------------------------
struct F32Sum {
  using S = float;
  using SA = float;
  using VA = f32x4;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return a + x; }
  __device__ static S s_fin(SA a) { return a; }
  __device__ static VA v_init(u32x4 x) { return __builtin_bit_cast(f32x4, x); }
  __device__ static VA v_comb(VA a, u32x4 x) { return a + __builtin_bit_cast(f32x4, x); }
  __device__ static u32x4 v_fin(VA a) { return __builtin_bit_cast(u32x4, a); }
  __device__ static SA s_add(SA a, SA b) { return a + b; }
  __device__ static SA s_rnd(SA a) { return a; }
  __device__ static VA v_add(VA a, VA b) { return a + b; }
  __device__ static VA v_rnd(VA a) { return a; }
  using SC = float;  // scaled finish (ScaledFin): one multiply in the accumulator's precision
  __device__ static SA s_scale(SA a, SC r) { return mul_rn(a, r); }
  __device__ static VA v_scale(VA a, SC r) { return mul_rn(a, r); }
  // amax finish (AmaxFin): the key of a stored vector / element, the max of two keys, a key as fp32 bits
  __device__ static unsigned v_key(u32x4 o) {
    const u32x4 m = o & 0x7fffffffu;
    return umax(umax(m.x, m.y), umax(m.z, m.w));
  }
  __device__ static unsigned s_key(S o) { return __float_as_uint(o) & 0x7fffffffu; }
  __device__ static unsigned key_max(unsigned a, unsigned b) { return umax(a, b); }
  __device__ static unsigned key_f32(unsigned k) { return k; }
};
struct F64Sum {
  using S = double;
  using SA = double;
  using VA = f64x2;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return a + x; }
  __device__ static S s_fin(SA a) { return a; }
  __device__ static VA v_init(u32x4 x) { return __builtin_bit_cast(f64x2, x); }
  __device__ static VA v_comb(VA a, u32x4 x) { return a + __builtin_bit_cast(f64x2, x); }
  __device__ static u32x4 v_fin(VA a) { return __builtin_bit_cast(u32x4, a); }
  __device__ static SA s_add(SA a, SA b) { return a + b; }
  __device__ static SA s_rnd(SA a) { return a; }
  __device__ static VA v_add(VA a, VA b) { return a + b; }
  __device__ static VA v_rnd(VA a) { return a; }
  using SC = double;
  __device__ static SA s_scale(SA a, SC r) { return mul_rn(a, r); }
  __device__ static VA v_scale(VA a, SC r) { return mul_rn(a, r); }
};
// bf16 rounding of two floats at once.  HW: gfx950's v_cvt_pk_bf16_f32 (RNE); every one of the 2^32
// float bit patterns converts to the same bf16 bits as bf16_round_bits, NaNs included
// (ftar_debug_bf16_cvt_check, tests/test_gpu_reduce.py), so the two are interchangeable.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
template <bool HW>
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  if constexpr (HW) return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
  else return (bf16_round_bits(lo) >> 16) | bf16_round_bits(hi);
}
// IEEE binary16 <-> fp32 through the compiler's conversions: v_cvt_f32_f16 (exact, subnormals included)
// and, two floats at once, v_cvt_pk_f16_f32 (RNE: overflow to inf, gradual underflow).  Both directions
// are checked over every bit pattern against integer code (ftar_debug_f16_cvt_check).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_f16(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, f16x2));
}
__device__ __forceinline__ f32x2 unpack_f16(unsigned x) {
  return __builtin_convertvector(__builtin_bit_cast(f16x2, x), f32x2);
}
// The two 16-bit float formats as the sum traits below see them: widen one element / a pair of packed
// words, pack two floats (one RNE each), round a float to the format and back (rnd, rnd4).
template <bool HW>
struct Bf16Fmt {
  __device__ static float widen(unsigned short h) { return bf16_to_f32(h); }
  __device__ static unsigned short narrow(float f) { return f32_to_bf16(f); }
  __device__ static f32x4 unpack(unsigned a, unsigned b) {
    f32x4 r;
    r.x = __uint_as_float(a << 16);
    r.y = __uint_as_float(a & 0xffff0000u);
    r.z = __uint_as_float(b << 16);
    r.w = __uint_as_float(b & 0xffff0000u);
    return r;
  }
  __device__ static unsigned pack(float lo, float hi) { return pack_bf16<HW>(lo, hi); }
  __device__ static float rnd(float f) { return __uint_as_float(bf16_round_bits(f)); }
  __device__ static f32x4 rnd4(f32x4 v) {
    if constexpr (HW) return unpack(pack(v.x, v.y), pack(v.z, v.w));
    else return f32x4{rnd(v.x), rnd(v.y), rnd(v.z), rnd(v.w)};
  }
};
struct HalfFmt {
  __device__ static float widen(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
  __device__ static unsigned short narrow(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  __device__ static f32x4 unpack(unsigned a, unsigned b) {
    const f32x2 lo = unpack_f16(a), hi = unpack_f16(b);
    return f32x4{lo.x, lo.y, hi.x, hi.y};
  }
  __device__ static unsigned pack(float lo, float hi) { return pack_f16(lo, hi); }
  __device__ static float rnd(float f) { return (float)(_Float16)f; }
  __device__ static f32x4 rnd4(f32x4 v) { return unpack(pack(v.x, v.y), pack(v.z, v.w)); }
};
// 16-bit float sums (extensions): fp32 accumulate, one RNE to the format per reduce call
template <class F>
struct H16SumT {
  using S = unsigned short;
  using SA = float;
  struct VA {
    f32x4 lo, hi;
  };
  __device__ static SA s_init(S x) { return F::widen(x); }
  __device__ static SA s_comb(SA a, S x) { return a + F::widen(x); }
  __device__ static S s_fin(SA a) { return F::narrow(a); }
  __device__ static VA v_init(u32x4 x) { return {F::unpack(x.x, x.y), F::unpack(x.z, x.w)}; }
  __device__ static VA v_comb(VA a, u32x4 x) {
    VA b = v_init(x);
    return {a.lo + b.lo, a.hi + b.hi};
  }
  __device__ static u32x4 v_fin(VA a) {
    return u32x4{F::pack(a.lo.x, a.lo.y), F::pack(a.lo.z, a.lo.w), F::pack(a.hi.x, a.hi.y), F::pack(a.hi.z, a.hi.w)};
  }
  // nested folds: an inner node's value is stored in the 16-bit format by the
  // staged schedule, so it is rounded before its parent adds it
  __device__ static SA s_add(SA a, SA b) { return a + b; }
  __device__ static SA s_rnd(SA a) { return F::rnd(a); }
  __device__ static VA v_add(VA a, VA b) { return {a.lo + b.lo, a.hi + b.hi}; }
  __device__ static VA v_rnd(VA a) { return {F::rnd4(a.lo), F::rnd4(a.hi)}; }
  using SC = float;  // the fp32 accumulator times r (v_pk_mul_f32), then the fold's one RNE
  __device__ static SA s_scale(SA a, SC r) {  // head / tail elements: the product lands in a register first,
    float p = mul_rn(a, r);                   // so the narrowing after it is a conversion of its own (never one
    asm volatile("" : "+v"(p));               // v_fma_mixlo_f16 of the unrounded product)
    return p;
  }
  __device__ static VA v_scale(VA a, SC r) { return {mul_rn(a.lo, r), mul_rn(a.hi, r)}; }
  // amax finish: two u16 lanes of |encoding|; the winner widens exactly (v_cvt_f32_f16, << 16)
  __device__ static unsigned v_key(u32x4 o) {
    const u32x4 m = o & 0x7fff7fffu;
    return pk_umax16(pk_umax16(m.x, m.y), pk_umax16(m.z, m.w));
  }
  __device__ static unsigned s_key(S o) { return o & 0x7fffu; }
  __device__ static unsigned key_max(unsigned a, unsigned b) { return pk_umax16(a, b); }
  __device__ static unsigned key_f32(unsigned k) {
    return __float_as_uint(F::widen((unsigned short)umax(k & 0xffffu, k >> 16)));
  }
};
// folded hop by hop: every add rounds to the format (the one-round ring fold has
// to reproduce the staged ring, which rounds once per hop)
template <class F>
struct H16SumHopT : H16SumT<F> {
  using B = H16SumT<F>;
  using typename B::S;
  using typename B::SA;
  using typename B::VA;
  __device__ static SA s_comb(SA a, S x) { return F::rnd(a + F::widen(x)); }
  __device__ static VA v_comb(VA a, u32x4 x) {
    VA b = B::v_init(x);
    const f32x4 lo = a.lo + b.lo, hi = a.hi + b.hi;
    return {F::rnd4(lo), F::rnd4(hi)};
  }
};
// the hop fold under a scaled finish: the staged ring's last hop is a plain k = 2 fold that rounds
// (a + b) * r once, so here the accumulator is rounded BEFORE each add (a no-op on the first operand,
// already in the format) and the last sum reaches the finisher unrounded
template <class F>
struct H16SumHopPreT : H16SumT<F> {
  using B = H16SumT<F>;
  using typename B::S;
  using typename B::SA;
  using typename B::VA;
  __device__ static SA s_comb(SA a, S x) { return F::rnd(a) + F::widen(x); }
  __device__ static VA v_comb(VA a, u32x4 x) {
    VA b = B::v_init(x);
    return {F::rnd4(a.lo) + b.lo, F::rnd4(a.hi) + b.hi};
  }
};
constexpr bool kHwBf16 = KHW_BF16_DEFAULT;
// bf16 nested folds of three and four levels (2,2,2), (2,2,2,2) on the LDS-staged kernel: with the
// integer RNE their per-level rounds made them ALU-bound there (round 2: -2 to -25 %); with
// v_cvt_pk_bf16_f32 rounding they gain +6.6 % and +3.6 % over the register kernel (cold,
// profiles/r02/s4/kbench_nested_bf16_lds.log).  Runtime-coded bf16 shapes still lose there (2,3: -11 %,
// 3,3: -4 %) and keep the register kernel.  fp16 rounds in hardware too and follows bf16's choices.
constexpr bool kLdsDeepBf16 = KLDS_DEEP_BF16;
using BF16Sum = H16SumT<Bf16Fmt<kHwBf16>>;
using BF16SumHop = H16SumHopT<Bf16Fmt<kHwBf16>>;
using F16Sum = H16SumT<HalfFmt>;
using F16SumHop = H16SumHopT<HalfFmt>;
using BF16SumHopPre = H16SumHopPreT<Bf16Fmt<kHwBf16>>;
using F16SumHopPre = H16SumHopPreT<HalfFmt>;
// The two OCP fp8 formats (extensions): e4m3fn (bias 7, no inf, NaN = 0x7f / 0xff, max 448) and e5m2 (bias 15,
// IEEE-like, max 57344), four elements to a dword, through gfx950's packed conversions.  Widening
// (v_cvt_pk_f32_fp8 / _bf8, SDWA WORD_1 for bytes 2-3) is exact, subnormals included.  Narrowing
// (v_cvt_pk_fp8_f32 / _bf8_f32, op_sel for the high half, no clamp) is RNE on the encoding with the mantissa
// carry running into the next encoding and no saturation: e5m2 overflows to +-inf at |A| >= 61440, e4m3 to NaN
// at |A| > 464 (and for +-inf), NaN stays NaN -- torch's float32 -> float8 cast.  The bare instructions are
// used as they are: both directions equal the integer reference on every bit pattern (2^32 floats, 2^8 bytes;
// ftar_debug_f8_cvt_check in bench_kernels.hip, tests/test_gpu_f8.py), so no select sits around them.
template <bool E5M2>
struct F8Fmt {
  template <bool HI>
  __device__ static f32x2 widen2(unsigned w) {  // bytes 0-1 (HI: 2-3) of w
    if constexpr (E5M2) return __builtin_amdgcn_cvt_pk_f32_bf8(w, HI);
    else return __builtin_amdgcn_cvt_pk_f32_fp8(w, HI);
  }
  template <bool HI>
  __device__ static unsigned narrow2(float a, float b, unsigned old) {  // into bytes 0-1 (HI: 2-3) of old
    if constexpr (E5M2) return __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, HI);
    else return __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, HI);
  }
  __device__ static float widen(unsigned char b) { return widen2<false>(b).x; }
  __device__ static unsigned char narrow(float f) { return (unsigned char)narrow2<false>(f, f, 0u); }
  __device__ static f32x4 unpack(unsigned w) {
    const f32x2 lo = widen2<false>(w), hi = widen2<true>(w);
    return f32x4{lo.x, lo.y, hi.x, hi.y};
  }
  __device__ static unsigned pack(f32x4 v) { return narrow2<true>(v.z, v.w, narrow2<false>(v.x, v.y, 0u)); }
  __device__ static float rnd(float f) { return widen(narrow(f)); }
  __device__ static f32x4 rnd4(f32x4 v) { return unpack(pack(v)); }
};
using E4M3Fmt = F8Fmt<false>;
using E5M2Fmt = F8Fmt<true>;
// fp8 sums: the 16-bit floats' rules (fp32 accumulate, one RNE to the format per reduce call) on 16 elements
// per 16-byte vector.  A family of its own beside H16SumT: that one's two-f32x4 accumulator and pair-of-words
// unpack are spelled out in its bodies, and its generated code stays as it is.
template <class F>
struct F8SumT {
  using S = unsigned char;
  using SA = float;
  struct VA {
    f32x4 a, b, c, d;  // the four dwords of the vector, widened
  };
  __device__ static SA s_init(S x) { return F::widen(x); }
  __device__ static SA s_comb(SA a, S x) { return a + F::widen(x); }
  __device__ static S s_fin(SA a) { return F::narrow(a); }
  __device__ static VA v_init(u32x4 x) { return {F::unpack(x.x), F::unpack(x.y), F::unpack(x.z), F::unpack(x.w)}; }
  __device__ static VA v_comb(VA a, u32x4 x) { return v_add(a, v_init(x)); }
  __device__ static u32x4 v_fin(VA a) { return u32x4{F::pack(a.a), F::pack(a.b), F::pack(a.c), F::pack(a.d)}; }
  // nested folds: an inner node is stored in the format by the staged schedule, so it is rounded
  __device__ static SA s_add(SA a, SA b) { return a + b; }
  __device__ static SA s_rnd(SA a) { return F::rnd(a); }
  __device__ static VA v_add(VA a, VA b) { return {a.a + b.a, a.b + b.b, a.c + b.c, a.d + b.d}; }
  __device__ static VA v_rnd(VA a) { return {F::rnd4(a.a), F::rnd4(a.b), F::rnd4(a.c), F::rnd4(a.d)}; }
  using SC = float;  // the fp32 accumulator times r, then the fold's one RNE
  __device__ static SA s_scale(SA a, SC r) {  // as H16SumT::s_scale: the product is a value of its own in a
    float p = mul_rn(a, r);                   // register before the conversion reads it
    asm volatile("" : "+v"(p));
    return p;
  }
  __device__ static VA v_scale(VA a, SC r) { return {mul_rn(a.a, r), mul_rn(a.b, r), mul_rn(a.c, r), mul_rn(a.d, r)}; }
  // amax finish: byte keys |b| <= 0x7f, the even and the odd bytes of a dword as two u16 lanes each (there is
  // no packed u8 max); the winner widens exactly (v_cvt_f32_fp8 / _bf8; e4m3's 0x7f is its NAN)
  __device__ static unsigned v_key(u32x4 o) {
    const u32x4 e = o & 0x007f007fu, d = (o >> 8) & 0x007f007fu;
    return pk_umax16(pk_umax16(pk_umax16(e.x, e.y), pk_umax16(e.z, e.w)),
                     pk_umax16(pk_umax16(d.x, d.y), pk_umax16(d.z, d.w)));
  }
  __device__ static unsigned s_key(S o) { return o & 0x7fu; }
  __device__ static unsigned key_max(unsigned a, unsigned b) { return pk_umax16(a, b); }
  __device__ static unsigned key_f32(unsigned k) {
    // the sign masked off: v_cvt_f32_fp8 / _bf8 widen a NaN byte to 0xffc00000, which is no non-negative float's
    // pattern -- the AllReduce's second round (a signed integer MAX of the ranks' words) dropped it for a 0
    return __float_as_uint(F::widen((unsigned char)umax(k & 0xffffu, k >> 16))) & 0x7fffffffu;
  }
};
// the ring's one-round fold: rounded after every add (H16SumHopT), or, under a scaled finish, before each add
// (H16SumHopPreT)
template <class F>
struct F8SumHopT : F8SumT<F> {
  using B = F8SumT<F>;
  using typename B::S;
  using typename B::SA;
  using typename B::VA;
  __device__ static SA s_comb(SA a, S x) { return F::rnd(a + F::widen(x)); }
  __device__ static VA v_comb(VA a, u32x4 x) { return B::v_rnd(B::v_add(a, B::v_init(x))); }
};
template <class F>
struct F8SumHopPreT : F8SumT<F> {
  using B = F8SumT<F>;
  using typename B::S;
  using typename B::SA;
  using typename B::VA;
  __device__ static SA s_comb(SA a, S x) { return F::rnd(a) + F::widen(x); }
  __device__ static VA v_comb(VA a, u32x4 x) { return B::v_add(B::v_rnd(a), B::v_init(x)); }
};
using E4M3Sum = F8SumT<E4M3Fmt>;
using E5M2Sum = F8SumT<E5M2Fmt>;
// modular integer sums on packed lanes (SWAR for 8/16-bit lanes)
template <class S_, unsigned HI>
struct SwarSum {
  using S = S_;
  using SA = S_;
  using VA = u32x4;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return (S)(a + x); }
  __device__ static S s_fin(SA a) { return a; }
  __device__ static VA v_init(u32x4 x) { return x; }
  __device__ static VA v_comb(VA a, u32x4 b) {
    const u32x4 lo = (a & ~HI) + (b & ~HI);  // carries stay inside each lane
    return lo ^ ((a ^ b) & HI);
  }
  __device__ static u32x4 v_fin(VA a) { return a; }
};
using U8Sum = SwarSum<unsigned char, 0x80808080u>;
using U16Sum = SwarSum<unsigned short, 0x80008000u>;
struct U32Sum {
  using S = unsigned;
  using SA = unsigned;
  using VA = u32x4;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return a + x; }
  __device__ static S s_fin(SA a) { return a; }
  __device__ static VA v_init(u32x4 x) { return x; }
  __device__ static VA v_comb(VA a, u32x4 x) { return a + x; }
  __device__ static u32x4 v_fin(VA a) { return a; }
};
struct U64Sum {
  using S = unsigned long long;
  using SA = unsigned long long;
  using VA = u64x2;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return a + x; }
  __device__ static S s_fin(SA a) { return a; }
  __device__ static VA v_init(u32x4 x) { return __builtin_bit_cast(u64x2, x); }
  __device__ static VA v_comb(VA a, u32x4 x) { return a + __builtin_bit_cast(u64x2, x); }
  __device__ static u32x4 v_fin(VA a) { return __builtin_bit_cast(u32x4, a); }
};
// bool "sum": the reference adds 0/1 ints and stores sum != 0 -> logical OR
struct BoolSum {
  using S = unsigned char;
  using SA = unsigned char;
  using VA = u32x4;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return a | x; }
  __device__ static S s_fin(SA a) { return a != 0; }
  __device__ static VA v_init(u32x4 x) { return x; }
  __device__ static VA v_comb(VA a, u32x4 x) { return a | x; }
  __device__ static u32x4 v_fin(VA a) {
    const u32x4 nz = ((a & 0x7f7f7f7fu) + 0x7f7f7f7fu) | a;  // bit 7 of each byte = byte != 0
    return (nz >> 7) & 0x01010101u;
  }
};
template <class S_>
struct Band {
  using S = S_;
  using SA = S_;
  using VA = u32x4;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return (S)(a & x); }
  __device__ static S s_fin(SA a) { return a; }
  __device__ static VA v_init(u32x4 x) { return x; }
  __device__ static VA v_comb(VA a, u32x4 x) { return a & x; }
  __device__ static u32x4 v_fin(VA a) { return a; }
};

// MAX / MIN (extensions): exact, associative and commutative, so one flat fold serves every schedule.
// Integers compare by the dtype's signedness (v_pk_max_i16 and kin; 8-bit lanes are unpacked by the
// compiler; 64-bit lanes compare and select).  Floats follow IEEE 754-2019 maximum / minimum
// (v_maximum3_f32, v_pk_maximum3_f16, v_max_f64 plus a NaN select): -0 < +0, subnormals kept, any NaN
// source makes the lane NaN, and a non-NaN result is one of the sources bit for bit.
template <class T>
constexpr bool kIsFloat = std::is_same_v<T, float> || std::is_same_v<T, double> || std::is_same_v<T, _Float16>;
template <bool MAX, bool FLT, class V>  // V: a scalar or an ext-vector
__device__ __forceinline__ V min_max(V a, V b) {
  if constexpr (FLT) {
    if constexpr (MAX) return __builtin_elementwise_maximum(a, b);
    else return __builtin_elementwise_minimum(a, b);
  } else {
    if constexpr (MAX) return __builtin_elementwise_max(a, b);
    else return __builtin_elementwise_min(a, b);
  }
}
template <class T, bool MAX>
struct MinMax {
  using S = T;
  using SA = T;
  typedef T V __attribute__((ext_vector_type(16 / sizeof(T))));
  using VA = V;
  __device__ static SA s_init(S x) { return x; }
  __device__ static SA s_comb(SA a, S x) { return min_max<MAX, kIsFloat<T>>(a, x); }
  __device__ static S s_fin(SA a) { return a; }
  __device__ static VA v_init(u32x4 x) { return __builtin_bit_cast(V, x); }
  __device__ static VA v_comb(VA a, u32x4 x) { return min_max<MAX, kIsFloat<T>>(a, __builtin_bit_cast(V, x)); }
  __device__ static u32x4 v_fin(VA a) { return __builtin_bit_cast(u32x4, a); }
};
// bf16 has no native maximum: widening is a 16-bit shift, the fp32 maximum of two widened values is one
// of them (or a NaN, whose high half is a bf16 NaN), and its high half is the bf16 answer, exactly.
template <bool MAX>
struct BF16MinMax {
  using S = unsigned short;
  using SA = float;
  struct VA {
    f32x4 lo, hi;
  };
  using F = Bf16Fmt<false>;
  __device__ static SA s_init(S x) { return F::widen(x); }
  __device__ static SA s_comb(SA a, S x) { return min_max<MAX, true>(a, F::widen(x)); }
  __device__ static S s_fin(SA a) { return (S)(__float_as_uint(a) >> 16); }
  __device__ static VA v_init(u32x4 x) { return {F::unpack(x.x, x.y), F::unpack(x.z, x.w)}; }
  __device__ static VA v_comb(VA a, u32x4 x) {
    VA b = v_init(x);
    return {min_max<MAX, true>(a.lo, b.lo), min_max<MAX, true>(a.hi, b.hi)};
  }
  __device__ static unsigned pack(float lo, float hi) {
    return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
  }
  __device__ static u32x4 v_fin(VA a) {
    return u32x4{pack(a.lo.x, a.lo.y), pack(a.lo.z, a.lo.w), pack(a.hi.x, a.hi.y), pack(a.hi.z, a.hi.w)};
  }
};
// fp8 MAX / MIN, production: widen, fp32 maximum / minimum (v_maximum3_f32: two sources per instruction),
// narrow.  The round trip is exact (every fp8 value is an fp32 value and narrows back to its own byte), an
// fp32 NaN narrows to a NaN of the format, and e5m2's infs are ordinary values on both sides.
template <class F, bool MAX>
struct F8MinMax {
  using B = F8SumT<F>;
  using S = unsigned char;
  using SA = float;
  using VA = typename B::VA;
  __device__ static SA s_init(S x) { return F::widen(x); }
  __device__ static SA s_comb(SA a, S x) { return min_max<MAX, true>(a, F::widen(x)); }
  __device__ static S s_fin(SA a) { return F::narrow(a); }
  __device__ static VA v_init(u32x4 x) { return B::v_init(x); }
  __device__ static VA v_comb(VA a, u32x4 x) {
    const VA b = B::v_init(x);
    return {min_max<MAX, true>(a.a, b.a), min_max<MAX, true>(a.b, b.b), min_max<MAX, true>(a.c, b.c),
            min_max<MAX, true>(a.d, b.d)};
  }
  __device__ static u32x4 v_fin(VA a) { return B::v_fin(a); }
};
// The other formulation, kept as the A/B variant (bench_kernels.hip; DESIGN §4 has the rates): monotone
// unsigned keys on the bytes -- negatives all bits flipped, non-negatives the sign bit set -- four to a dword
// (SWAR), reduced as unsigned bytes; NaN sources (e4m3: |b| == 0x7f, e5m2: |b| > 0x7c) are collected apart
// in bit 7 of their byte and turn the lane into 0x7f / 0xff at the end.
template <bool E5M2, bool MAX>
struct F8KeyMinMax {
  using S = unsigned char;
  using SA = unsigned;  // bits 0-7 the key, bit 8 a NaN seen
  typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));
  struct VA {
    u32x4 key, nan;
  };
  static constexpr unsigned kNanAdd = E5M2 ? 0x03u : 0x01u;  // (|b| + kNanAdd) reaches bit 7 exactly for a NaN
  __device__ static SA s_init(S x) {
    const unsigned b = x;
    return ((b & 0x80u) ? (~b & 0xffu) : (b | 0x80u)) | ((((b & 0x7fu) + kNanAdd) & 0x80u) << 1);
  }
  __device__ static SA s_comb(SA a, S x) {
    const SA b = s_init(x);
    const unsigned ka = a & 0xffu, kb = b & 0xffu;
    return ((a | b) & 0x100u) | (MAX ? (ka > kb ? ka : kb) : (ka < kb ? ka : kb));
  }
  __device__ static S s_fin(SA a) {
    const unsigned k = a & 0xffu, b = (k & 0x80u) ? (k ^ 0x80u) : (~k & 0xffu);
    return (S)((a & 0x100u) ? (b | 0x7fu) : b);
  }
  // x ^ (0xff where the byte's `neg` bit (bit 0) is set, 0x80 elsewhere): bits -> key with neg = the sign, key ->
  // bits with neg = the key's top bit inverted
  __device__ static u32x4 flip(u32x4 x, u32x4 neg) { return x ^ (((neg << 8) - neg) | 0x80808080u); }
  __device__ static VA v_init(u32x4 x) {
    return {flip(x, (x >> 7) & 0x01010101u), ((x & 0x7f7f7f7fu) + kNanAdd * 0x01010101u) & 0x80808080u};
  }
  __device__ static VA v_comb(VA a, u32x4 x) {
    const VA b = v_init(x);
    const u8x16 ka = __builtin_bit_cast(u8x16, a.key), kb = __builtin_bit_cast(u8x16, b.key);
    return {__builtin_bit_cast(u32x4, min_max<MAX, false>(ka, kb)), a.nan | b.nan};
  }
  __device__ static u32x4 v_fin(VA a) {
    const u32x4 n = a.nan >> 7;  // a NaN byte: 0x7f ORed in
    return flip(a.key, (~a.key >> 7) & 0x01010101u) | ((n << 7) - n);
  }
};

// The finish of a fold: how the accumulator becomes the stored value.  One *_body per kernel family, three finishes:
//   PlainFin: the trait's own v_fin / s_fin (every op and dtype);
//   ScaledFin (AVG's root fold, ftar_reduce_scaled; the float sums): out = round_to_dtype(A * r), one multiply
//     in the accumulator's precision (fp32 for bf16 / fp16; subnormal products kept), then the fold's single
//     rounding.  A nested fold hands it the root unrounded (kRawRoot, tree_push).
//   AmaxFin (ftar_reduce_amax, the root folds of ftar_allreduce_amax; f32, bf16, fp16, fp8): ScaledFin's value
//     (SUM passes r = 1: the multiply is exact), and a per-lane running maximum of the stored values'
//     |encoding| (the traits' keys).  When the body ends, flush() widens each lane's winner to fp32 bits
//     (the bit pattern of a non-negative float is its own key), maxes them over the wave (__shfl_xor) and over
//     the workgroup's waves (one LDS word each), and one lane issues ONE no-return agent-scope atomicMax on
//     the caller's word: zeroed before the first launch, it holds the answer once the last launch has ended.
//     The state and the flush exist only under `if constexpr (kIsAmax<Fin>)`: the other kernels are unchanged.
// A family's __global__ kernels, NAME_kernel(args), NAME_scaled_kernel(args, scale) and NAME_amax_kernel(args,
// scale, unsigned* amax), are two-line wrappers over its body: profiles and tools key on those names and
// argument lists.  (The register kernels reduce_vec_kernel and reduce_tree_kernel are the exception, see there:
// their plain kernel is a copy of the body's loop.)
template <class Tr>
struct PlainFin {
  static constexpr bool kRawRoot = false;
  __device__ static typename Tr::S s(typename Tr::SA a) { return Tr::s_fin(a); }
  __device__ static u32x4 v(typename Tr::VA a) { return Tr::v_fin(a); }
};
template <class Tr>
struct ScaledFin {
  static constexpr bool kRawRoot = true;
  typename Tr::SC r;
  __device__ typename Tr::S s(typename Tr::SA a) const { return Tr::s_fin(Tr::s_scale(a, r)); }
  __device__ u32x4 v(typename Tr::VA a) const { return Tr::v_fin(Tr::v_scale(a, r)); }
};
template <class Tr>
struct AmaxFin {
  static constexpr bool kRawRoot = true;
  typename Tr::SC r;
  unsigned* word;
  unsigned key = 0;
  __device__ typename Tr::S s(typename Tr::SA a) {
    const typename Tr::S o = Tr::s_fin(Tr::s_scale(a, r));
    key = Tr::key_max(key, Tr::s_key(o));
    return o;
  }
  __device__ u32x4 v(typename Tr::VA a) {
    const u32x4 o = Tr::v_fin(Tr::v_scale(a, r));
    key = Tr::key_max(key, Tr::v_key(o));
    return o;
  }
  // every lane of the workgroup, once, after its last store; wave w's word is slots[w * stride] (LDS)
  __device__ void flush(unsigned* slots, unsigned stride) {
    unsigned m = Tr::key_f32(key);
#pragma unroll
    for (int o = 32; o; o >>= 1) m = umax(m, (unsigned)__shfl_xor((int)m, o));
    const unsigned nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) slots[(threadIdx.x >> 6) * stride] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (unsigned w = 1; w < nw; ++w) m = umax(m, slots[w * stride]);
      // One address takes about 88 atomics per microsecond, returning or not: a launch of 131,072 two-wave
      // workgroups (f32 k = 2 on 256 MiB) spent 1.5 ms in them against 0.12 ms of memory traffic.
      // The word only grows while a call runs, so a workgroup whose maximum is not above what it reads there
      // (an L2 read, which one address serves far faster) has nothing to add: after the first few workgroups
      // nearly all of them skip the atomic.  A value read stale is smaller, and only costs an atomic.  The
      // read sits here, last: issued before the reduction the 2-byte k = 2 launch took 0.148 ms against 0.137
      // (profiles/amax/).
      if (m > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)__hip_atomic_fetch_max(word, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
};
template <class Fin>
constexpr bool kIsAmax = false;
template <class Tr>
constexpr bool kIsAmax<AmaxFin<Tr>> = true;
// the flush of a kernel that stages nothing through LDS: one word per wave of its own
template <class Fin>
__device__ __forceinline__ void amax_flush(Fin& fin) {
  if constexpr (kIsAmax<Fin>) {
    __shared__ unsigned slots[16];
    fin.flush(slots, 1);
  }
}

template <int K>
struct Srcs {
  const void* p[K];
};
template <int K>
Srcs<K> pack_srcs(const void* const* srcs, int k) {
  Srcs<K> a{};
  for (int j = 0; j < k; ++j) a.p[j] = srcs[j];
  return a;
}

// ---------------------------------------------------------------------------
// vector kernel: K sources (K == 0: runtime k <= FTAR_MAX_K), U vectors per lane.
// Element range [head, head + nvec*VE) is vectorised; workgroup 0 also does the
// `head` leading and `tail` trailing elements element-wise.
// ---------------------------------------------------------------------------
template <class Tr, int K, int U, bool NTL, bool NTS, int BS = kThreads>
__global__ void __launch_bounds__(BS)
    reduce_vec_kernel(Srcs<(K > 0 ? K : FTAR_MAX_K)> src, int kr, void* dst, size_t nvec, int head,
                      int tail) {
  using S = typename Tr::S;
  constexpr int KK = K > 0 ? K : FTAR_MAX_K;
  const int k = K > 0 ? K : kr;
  constexpr int VE = 16 / sizeof(S);
  constexpr int kThreads = BS;
  const size_t tile_stride = (size_t)gridDim.x * (U * kThreads);
  size_t v0 = (size_t)blockIdx.x * (U * kThreads) + threadIdx.x;

  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {  // unaligned head / short tail
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * VE + (threadIdx.x - head);
    typename Tr::SA a = Tr::s_init(static_cast<const S*>(src.p[0])[e]);
    for (int j = 1; j < k; ++j) a = Tr::s_comb(a, static_cast<const S*>(src.p[j])[e]);
    static_cast<S*>(dst)[e] = Tr::s_fin(a);
  }

  const u32x4* s0 = reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[0]) + head);
  u32x4* d = reinterpret_cast<u32x4*>(static_cast<S*>(dst) + head);
  for (; v0 + (U - 1) * kThreads < nvec; v0 += tile_stride) {  // full tiles: no per-vector guards
    typename Tr::VA acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = Tr::v_init(ld16<NTL>(s0 + v0 + u * kThreads));
    if constexpr (K > 0) {
      u32x4 x[KK > 1 ? KK - 1 : 1][U];
#pragma unroll
      for (int j = 1; j < KK; ++j) {
        const u32x4* sj = reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head);
#pragma unroll
        for (int u = 0; u < U; ++u) x[j - 1][u] = ld16<NTL>(sj + v0 + u * kThreads);
      }
#pragma unroll
      for (int j = 1; j < KK; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = Tr::v_comb(acc[u], x[j - 1][u]);
    } else {
      for (int j = 1; j < k; ++j) {
        const u32x4* sj = reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head);
        u32x4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = ld16<NTL>(sj + v0 + u * kThreads);
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = Tr::v_comb(acc[u], x[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st16<NTS>(d + v0 + u * kThreads, Tr::v_fin(acc[u]));
  }
  // the one partial tile (if any): guarded
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t v = v0 + u * kThreads;
    if (v >= nvec) break;
    typename Tr::VA a = Tr::v_init(ld16<NTL>(s0 + v));
    for (int j = 1; j < k; ++j)
      a = Tr::v_comb(a, ld16<NTL>(reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head) + v));
    st16<NTS>(d + v, Tr::v_fin(a));
  }
}

// The scaled twin: reduce_vec_kernel's loop again, with a ScaledFin finish.  The two register families (this one
// and reduce_tree_kernel) keep two copies of their loop -- a fix to one goes into both.  Behind a shared body
// the compiler optimises the body before it inlines it into the kernel and hoists every kernarg pointer load
// to the kernel's entry: the static-K instantiations (the A/B variants of bench_kernels.hip) came out
// different, a dozen of them with more VGPRs and an occupancy step lost (tools/asm_diff.py, profiles/README.md).
template <class Tr, int K, int U, bool NTL, bool NTS, int BS, class Fin>
__device__ __forceinline__ void reduce_vec_body(const Srcs<(K > 0 ? K : FTAR_MAX_K)>& src, int kr, void* dst,
                                                size_t nvec, int head, int tail, Fin fin) {
  using S = typename Tr::S;
  constexpr int KK = K > 0 ? K : FTAR_MAX_K;
  const int k = K > 0 ? K : kr;
  constexpr int VE = 16 / sizeof(S);
  constexpr int kThreads = BS;
  const size_t tile_stride = (size_t)gridDim.x * (U * kThreads);
  size_t v0 = (size_t)blockIdx.x * (U * kThreads) + threadIdx.x;

  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {  // unaligned head / short tail
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * VE + (threadIdx.x - head);
    typename Tr::SA a = Tr::s_init(static_cast<const S*>(src.p[0])[e]);
    for (int j = 1; j < k; ++j) a = Tr::s_comb(a, static_cast<const S*>(src.p[j])[e]);
    static_cast<S*>(dst)[e] = fin.s(a);
  }

  const u32x4* s0 = reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[0]) + head);
  u32x4* d = reinterpret_cast<u32x4*>(static_cast<S*>(dst) + head);
  for (; v0 + (U - 1) * kThreads < nvec; v0 += tile_stride) {  // full tiles: no per-vector guards
    typename Tr::VA acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = Tr::v_init(ld16<NTL>(s0 + v0 + u * kThreads));
    if constexpr (K > 0) {
      u32x4 x[KK > 1 ? KK - 1 : 1][U];
#pragma unroll
      for (int j = 1; j < KK; ++j) {
        const u32x4* sj = reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head);
#pragma unroll
        for (int u = 0; u < U; ++u) x[j - 1][u] = ld16<NTL>(sj + v0 + u * kThreads);
      }
#pragma unroll
      for (int j = 1; j < KK; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = Tr::v_comb(acc[u], x[j - 1][u]);
    } else {
      for (int j = 1; j < k; ++j) {
        const u32x4* sj = reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head);
        u32x4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = ld16<NTL>(sj + v0 + u * kThreads);
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = Tr::v_comb(acc[u], x[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st16<NTS>(d + v0 + u * kThreads, fin.v(acc[u]));
  }
  // the one partial tile (if any): guarded
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t v = v0 + u * kThreads;
    if (v >= nvec) break;
    typename Tr::VA a = Tr::v_init(ld16<NTL>(s0 + v));
    for (int j = 1; j < k; ++j)
      a = Tr::v_comb(a, ld16<NTL>(reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head) + v));
    st16<NTS>(d + v, fin.v(a));
  }
  amax_flush(fin);
}

template <class Tr, int K, int U, bool NTL, bool NTS, int BS = kThreads>
__global__ void __launch_bounds__(BS)
    reduce_vec_scaled_kernel(Srcs<(K > 0 ? K : FTAR_MAX_K)> src, int kr, void* dst, size_t nvec, int head,
                             int tail, typename Tr::SC scale) {
  reduce_vec_body<Tr, K, U, NTL, NTS, BS>(src, kr, dst, nvec, head, tail, ScaledFin<Tr>{scale});
}
template <class Tr, int K, int U, bool NTL, bool NTS, int BS = kThreads>
__global__ void __launch_bounds__(BS)
    reduce_vec_amax_kernel(Srcs<(K > 0 ? K : FTAR_MAX_K)> src, int kr, void* dst, size_t nvec, int head,
                           int tail, typename Tr::SC scale, unsigned* amax) {
  reduce_vec_body<Tr, K, U, NTL, NTS, BS>(src, kr, dst, nvec, head, tail, AmaxFin<Tr>{scale, amax});
}

// LDS-staged reduce: the production kernel for k = 2..16 (launch_k; A/B
// variants in tools/kbench_cold.py).  Each wave streams U tiles of every
// source into LDS with LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave
// instruction, nontemporal, no VGPR destination); every lane reads its own
// 16 B back with ds_read_b128 and folds.  Nothing is shared between lanes in
// an element-wise sum, so LDS serves as the landing zone of the loads: K x U
// KiB in flight per wave without spending VGPRs on them.
//   PROG (production): the loads are issued tile-major and tile u is folded
// and stored as soon as its K loads have landed (counted vmcnt: loads return
// in order, so the stores also in the count can only make a wait longer),
// while tiles u+1.. are still in flight.  !PROG waits for all K x U loads
// first (the round-1 kernel, kept as an A/B variant).
// Workgroup 0 also does the `head` leading and `tail` trailing elements
// element-wise, as reduce_vec_kernel does.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "gfx9 vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The staging and tile loop shared by the flat and the nested fold: `fold(get)`
// combines the K values get(0..K-1) of one 16-B vector slot (get(j) = source
// j's vector, from LDS or, on the partial tile, from memory), `elem(e)` folds
// element e alone (unaligned head / short tail, workgroup 0).
// Returns the staging LDS (wave w's region starts kLdsWaveWords<K, U> words after wave w - 1's): the amax
// finish leaves each wave's word in its own region once the wave has read its last tile back.
template <int K, int U>
constexpr unsigned kLdsWaveWords = U * K * 64 * 4;
template <class Tr, int K, int U, int W, int AUX, bool PROG, class Fold, class Elem>
__device__ __forceinline__ unsigned* lds_staged(const Srcs<K>& src, void* dst, size_t nvec, int head, int tail,
                                                Fold fold, Elem elem) {
  static_assert(W * U * K <= 160, "LDS per workgroup = W x U x K KiB <= 160 KiB");
  using S = typename Tr::S;
  constexpr int VE = 16 / sizeof(S);
  __shared__ u32x4 lds[W][U][K][64];
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {  // unaligned head / short tail
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * VE + (threadIdx.x - head);
    static_cast<S*>(dst)[e] = elem(e);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t base = ((size_t)blockIdx.x * W + wave) * (U * 64);
  u32x4* d = reinterpret_cast<u32x4*>(static_cast<S*>(dst) + head);
  auto sp = [&](int j) { return reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head); };
  if (base + U * 64 <= nvec) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const u32x4* g = sp(j) + base + u * 64 + lane;
        __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)g,
                                         (__attribute__((address_space(3))) void*)&lds[wave][u][j][0], 16, 0, AUX);
      }
    if constexpr (!PROG) wait_vmcnt<0>();
    auto tile = [&](auto uc) {
      constexpr int u = decltype(uc)::value;
      // the K loads of tile u have landed (a count above 63 waits for more: still exact)
      if constexpr (PROG) wait_vmcnt<((U - 1 - u) * K > 63 ? 63 : (U - 1 - u) * K)>();
      st16<kNtStores>(d + base + u * 64 + lane, fold([&](int j) { return lds[wave][u][j][lane]; }));
    };
    [&]<int... I>(std::integer_sequence<int, I...>) { (tile(std::integral_constant<int, I>{}), ...); }
    (std::make_integer_sequence<int, U>{});
  } else {
    for (int u = 0; u < U; ++u) {
      const size_t v = base + u * 64 + lane;
      if (v >= nvec) break;
      st16<kNtStores>(d + v, fold([&](int j) { return ld16<kNtLoads>(sp(j) + v); }));
    }
  }
  return reinterpret_cast<unsigned*>(&lds[0][0][0][0]);
}

template <class Tr, int K, int U, int W, int AUX, bool PROG, class Fin>
__device__ __forceinline__ void reduce_lds_body(const Srcs<K>& src, void* dst, size_t nvec, int head, int tail,
                                                Fin fin) {
  using S = typename Tr::S;
  unsigned* const lds = lds_staged<Tr, K, U, W, AUX, PROG>(
      src, dst, nvec, head, tail,
      [&](auto get) {
        typename Tr::VA a = Tr::v_init(get(0));
#pragma unroll
        for (int j = 1; j < K; ++j) a = Tr::v_comb(a, get(j));
        return fin.v(a);
      },
      [&](size_t e) {
        typename Tr::SA a = Tr::s_init(static_cast<const S*>(src.p[0])[e]);
        for (int j = 1; j < K; ++j) a = Tr::s_comb(a, static_cast<const S*>(src.p[j])[e]);
        return fin.s(a);
      });
  if constexpr (kIsAmax<Fin>) fin.flush(lds, kLdsWaveWords<K, U>);
  else (void)lds;
}
template <class Tr, int K, int U, int W, int AUX, bool PROG>
__global__ void __launch_bounds__(W * 64)
    reduce_lds_kernel(Srcs<K> src, void* dst, size_t nvec, int head, int tail) {
  reduce_lds_body<Tr, K, U, W, AUX, PROG>(src, dst, nvec, head, tail, PlainFin<Tr>{});
}
template <class Tr, int K, int U, int W, int AUX, bool PROG>
__global__ void __launch_bounds__(W * 64)
    reduce_lds_scaled_kernel(Srcs<K> src, void* dst, size_t nvec, int head, int tail, typename Tr::SC scale) {
  reduce_lds_body<Tr, K, U, W, AUX, PROG>(src, dst, nvec, head, tail, ScaledFin<Tr>{scale});
}
template <class Tr, int K, int U, int W, int AUX, bool PROG>
__global__ void __launch_bounds__(W * 64)
    reduce_lds_amax_kernel(Srcs<K> src, void* dst, size_t nvec, int head, int tail, typename Tr::SC scale,
                           unsigned* amax) {
  reduce_lds_body<Tr, K, U, W, AUX, PROG>(src, dst, nvec, head, tail, AmaxFin<Tr>{scale, amax});
}

// element-wise fallback for sources not co-aligned with dst
template <class Tr, class Fin>
__device__ __forceinline__ void reduce_elem_body(const Srcs<FTAR_MAX_K>& src, int k, void* dst, size_t n, Fin fin) {
  using S = typename Tr::S;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) {
    typename Tr::SA a = Tr::s_init(static_cast<const S*>(src.p[0])[e]);
    for (int j = 1; j < k; ++j) a = Tr::s_comb(a, static_cast<const S*>(src.p[j])[e]);
    static_cast<S*>(dst)[e] = fin.s(a);
  }
  amax_flush(fin);
}
template <class Tr>
__global__ void __launch_bounds__(kThreads)
    reduce_elem_kernel(Srcs<FTAR_MAX_K> src, int k, void* dst, size_t n) {
  reduce_elem_body<Tr>(src, k, dst, n, PlainFin<Tr>{});
}
template <class Tr>
__global__ void __launch_bounds__(kThreads)
    reduce_elem_scaled_kernel(Srcs<FTAR_MAX_K> src, int k, void* dst, size_t n, typename Tr::SC scale) {
  reduce_elem_body<Tr>(src, k, dst, n, ScaledFin<Tr>{scale});
}
template <class Tr>
__global__ void __launch_bounds__(kThreads)
    reduce_elem_amax_kernel(Srcs<FTAR_MAX_K> src, int k, void* dst, size_t n, typename Tr::SC scale, unsigned* amax) {
  reduce_elem_body<Tr>(src, k, dst, n, AmaxFin<Tr>{scale, amax});
}

// ---------------------------------------------------------------------------
// nested-fold kernel: the one-round reduce-scatter of a multi-stage tree.
// The k sources are the P copies of one block in depth-first leaf order of the
// block's mixed-radix fold tree (schedule.cpp tree_leaves), so every inner
// node folds a run of consecutive values: level 0 folds leaves w0 at a time,
// level 1 folds those results w1 at a time, ...  Per leaf j the host packs one
// code byte (make_tree_code): bits 0-2 = how many levels complete after leaf
// j, bit 3+l = the value entering level l opens a new node.  The codes are
// uniform across the grid (kernarg, scalar branches); accumulators are indexed
// only by unrolled loop counters, so they stay in VGPRs.  Float sums only:
// integer sums and AND are associative, the flat kernel is exact for them.
// ---------------------------------------------------------------------------
struct TreeCode {
  unsigned char c[FTAR_MAX_K];
};

// Code byte of leaf j of a nested fold with bottom-up widths w[0..L): bits 0-2
// = levels completed after leaf j, bit 3+l = the value entering level l opens
// a new node (level L's bit marks the root slot, written but never read).
__host__ __device__ constexpr unsigned leaf_code(const int* w, int L, int j) {
  int prod[kTreeLevels] = {};
  int p = 1;
  for (int l = 0; l < L; ++l) {
    p *= w[l];
    prod[l] = p;
  }
  unsigned done = 0;
  while (done < (unsigned)L && (j + 1) % prod[done] == 0) ++done;
  unsigned code = done;
  if (j % w[0] == 0) code |= 1u << 3;
  for (unsigned l = 1; l <= done && l < (unsigned)L; ++l)
    if (((j + 1) / prod[l - 1] - 1) % w[l] == 0) code |= 1u << (3 + l);
  if (done == (unsigned)L && L < kTreeLevels) code |= 1u << (3 + L);
  return code;
}

// The common shapes at compile time: with the leaf codes constant after
// unrolling, every select and level branch of tree_push folds away and the
// nested fold is straight-line adds (and bf16 rounds).
template <int... W>
struct StaticShape {
  static constexpr int L = sizeof...(W);
  static constexpr int K = (W * ... * 1);
  __device__ static constexpr unsigned code(int j) {
    constexpr int w[L] = {W...};
    return leaf_code(w, L, j);
  }
};
struct RuntimeShape {};

template <class Tr, bool VEC>
struct TreeOps;
template <class Tr>
struct TreeOps<Tr, true> {
  using A = typename Tr::VA;
  __device__ static A add(A a, A b) { return Tr::v_add(a, b); }
  __device__ static A rnd(A a) { return Tr::v_rnd(a); }
};
template <class Tr>
struct TreeOps<Tr, false> {
  using A = typename Tr::SA;
  __device__ static A add(A a, A b) { return Tr::s_add(a, b); }
  __device__ static A rnd(A a) { return Tr::s_rnd(a); }
};

// push leaf values v[0..U) (one per vector slot) up the tree; on the last leaf v ends up holding the
// root.  Inner nodes are rounded as they close (the staged schedule stores them in the dtype); RAW (the
// finish's kRawRoot) leaves the root as its level's accumulator holds it, unrounded, for the finish to scale
// and round once: the last leaf (`last`) completes every level (done = L), so the root is the node that
// closes at level done - 1.  Without RAW `last` is dead and compiles to nothing.
template <bool RAW, class O, int U>
__device__ __forceinline__ void tree_push(typename O::A (&acc)[kTreeLevels][U], typename O::A (&v)[U], unsigned code,
                                          bool last) {
  const unsigned done = code & 7u;
#pragma unroll
  for (int l = 0; l < kTreeLevels; ++l) {
    const bool fresh = (code >> (3 + l)) & 1u;
#pragma unroll
    for (int u = 0; u < U; ++u) acc[l][u] = fresh ? v[u] : O::add(acc[l][u], v[u]);
    if (done <= (unsigned)l) break;
    const bool root = RAW && last && done == (unsigned)l + 1;
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = root ? acc[l][u] : O::rnd(acc[l][u]);
  }
}

template <class Tr, class Fin>
__device__ __forceinline__ typename Tr::S tree_elem(const void* const* p, int k, const TreeCode& tc, size_t e,
                                                    Fin&& fin) {  // by reference: the amax finish keeps state
  using S = typename Tr::S;
  using O = TreeOps<Tr, false>;
  typename O::A acc[kTreeLevels][1], v[1];
  for (int j = 0; j < k; ++j) {
    v[0] = Tr::s_init(static_cast<const S*>(p[j])[e]);
    tree_push<std::remove_reference_t<Fin>::kRawRoot, O, 1>(acc, v, tc.c[j], j == k - 1);
  }
  return fin.s(v[0]);
}

// The nested fold in registers (round 1): f64, the 2-byte runtime-coded shapes, k outside the LDS set, and
// the A/B reference of ftar_debug_reduce_nested_lds.  Like reduce_vec_kernel it keeps its scaled loop as a second
// copy (reduce_tree_body below) -- a fix to one goes into both: behind a shared body all 41 plain instantiations
// compile differently (kernarg loads hoisted to the entry), and on cold data f64 (2,3) lost 1.7 % against the
// kernel as written here while f32 (3,3) gained 3.5 % (profiles/fold_bodies/).
template <class Tr, int K, int U, class Sh = RuntimeShape>
__global__ void __launch_bounds__(kThreads)
    reduce_tree_kernel(Srcs<(K > 0 ? K : FTAR_MAX_K)> src, int kr, TreeCode tc, void* dst, size_t nvec,
                       int head, int tail) {
  using S = typename Tr::S;
  using O = TreeOps<Tr, true>;
  const int k = K > 0 ? K : kr;
  constexpr int VE = 16 / sizeof(S);
  const size_t tile_stride = (size_t)gridDim.x * (U * kThreads);
  size_t v0 = (size_t)blockIdx.x * (U * kThreads) + threadIdx.x;

  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * VE + (threadIdx.x - head);
    static_cast<S*>(dst)[e] = tree_elem<Tr>(src.p, k, tc, e, PlainFin<Tr>{});
  }
  auto sp = [&](int j) { return reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head); };
  u32x4* d = reinterpret_cast<u32x4*>(static_cast<S*>(dst) + head);
  for (; v0 + (U - 1) * kThreads < nvec; v0 += tile_stride) {
    typename O::A acc[kTreeLevels][U], v[U];
    if constexpr (K > 0) {  // every source in flight before the first add
      u32x4 x[K][U];
#pragma unroll
      for (int j = 0; j < K; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) x[j][u] = ld16<kNtLoads>(sp(j) + v0 + u * kThreads);
#pragma unroll
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = Tr::v_init(x[j][u]);
        if constexpr (std::is_same_v<Sh, RuntimeShape>) tree_push<false, O, U>(acc, v, tc.c[j], false);
        else tree_push<false, O, U>(acc, v, Sh::code(j), false);
      }
    } else {
      for (int j = 0; j < k; ++j) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = Tr::v_init(ld16<kNtLoads>(sp(j) + v0 + u * kThreads));
        tree_push<false, O, U>(acc, v, tc.c[j], false);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st16<kNtStores>(d + v0 + u * kThreads, Tr::v_fin(v[u]));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {  // the one partial tile (if any)
    const size_t vi = v0 + u * kThreads;
    if (vi >= nvec) break;
    typename O::A acc[kTreeLevels][1], v[1];
    for (int j = 0; j < k; ++j) {
      v[0] = Tr::v_init(ld16<kNtLoads>(sp(j) + vi));
      tree_push<false, O, 1>(acc, v, tc.c[j], false);
    }
    d[vi] = Tr::v_fin(v[0]);
  }
}

template <class Tr, int K, int U, class Sh, class Fin>
__device__ __forceinline__ void reduce_tree_body(const Srcs<(K > 0 ? K : FTAR_MAX_K)>& src, int kr,
                                                 const TreeCode& tc, void* dst, size_t nvec, int head, int tail,
                                                 Fin fin) {
  using S = typename Tr::S;
  using O = TreeOps<Tr, true>;
  constexpr bool RAW = Fin::kRawRoot;
  const int k = K > 0 ? K : kr;
  constexpr int VE = 16 / sizeof(S);
  const size_t tile_stride = (size_t)gridDim.x * (U * kThreads);
  size_t v0 = (size_t)blockIdx.x * (U * kThreads) + threadIdx.x;

  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(head + tail)) {
    const size_t e = threadIdx.x < (unsigned)head ? threadIdx.x : (size_t)head + nvec * VE + (threadIdx.x - head);
    static_cast<S*>(dst)[e] = tree_elem<Tr>(src.p, k, tc, e, fin);
  }
  auto sp = [&](int j) { return reinterpret_cast<const u32x4*>(static_cast<const S*>(src.p[j]) + head); };
  u32x4* d = reinterpret_cast<u32x4*>(static_cast<S*>(dst) + head);
  for (; v0 + (U - 1) * kThreads < nvec; v0 += tile_stride) {
    typename O::A acc[kTreeLevels][U], v[U];
    if constexpr (K > 0) {  // every source in flight before the first add
      u32x4 x[K][U];
#pragma unroll
      for (int j = 0; j < K; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) x[j][u] = ld16<kNtLoads>(sp(j) + v0 + u * kThreads);
#pragma unroll
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = Tr::v_init(x[j][u]);
        if constexpr (std::is_same_v<Sh, RuntimeShape>) tree_push<RAW, O, U>(acc, v, tc.c[j], j == K - 1);
        else tree_push<RAW, O, U>(acc, v, Sh::code(j), j == K - 1);
      }
    } else {
      for (int j = 0; j < k; ++j) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = Tr::v_init(ld16<kNtLoads>(sp(j) + v0 + u * kThreads));
        tree_push<RAW, O, U>(acc, v, tc.c[j], j == k - 1);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st16<kNtStores>(d + v0 + u * kThreads, fin.v(v[u]));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {  // the one partial tile (if any)
    const size_t vi = v0 + u * kThreads;
    if (vi >= nvec) break;
    typename O::A acc[kTreeLevels][1], v[1];
    for (int j = 0; j < k; ++j) {
      v[0] = Tr::v_init(ld16<kNtLoads>(sp(j) + vi));
      tree_push<RAW, O, 1>(acc, v, tc.c[j], j == k - 1);
    }
    d[vi] = fin.v(v[0]);
  }
  amax_flush(fin);
}
template <class Tr, int K, int U, class Sh = RuntimeShape>
__global__ void __launch_bounds__(kThreads)
    reduce_tree_scaled_kernel(Srcs<(K > 0 ? K : FTAR_MAX_K)> src, int kr, TreeCode tc, void* dst, size_t nvec,
                              int head, int tail, typename Tr::SC scale) {
  reduce_tree_body<Tr, K, U, Sh>(src, kr, tc, dst, nvec, head, tail, ScaledFin<Tr>{scale});
}
template <class Tr, int K, int U, class Sh = RuntimeShape>
__global__ void __launch_bounds__(kThreads)
    reduce_tree_amax_kernel(Srcs<(K > 0 ? K : FTAR_MAX_K)> src, int kr, TreeCode tc, void* dst, size_t nvec,
                            int head, int tail, typename Tr::SC scale, unsigned* amax) {
  reduce_tree_body<Tr, K, U, Sh>(src, kr, tc, dst, nvec, head, tail, AmaxFin<Tr>{scale, amax});
}

// element-wise, for sources not co-aligned with dst
template <class Tr, class Fin>
__device__ __forceinline__ void reduce_tree_elem_body(const Srcs<FTAR_MAX_K>& src, int k, const TreeCode& tc,
                                                      void* dst, size_t n, Fin fin) {
  using S = typename Tr::S;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride)
    static_cast<S*>(dst)[e] = tree_elem<Tr>(src.p, k, tc, e, fin);
  amax_flush(fin);
}
template <class Tr>
__global__ void __launch_bounds__(kThreads)
    reduce_tree_elem_kernel(Srcs<FTAR_MAX_K> src, int k, TreeCode tc, void* dst, size_t n) {
  reduce_tree_elem_body<Tr>(src, k, tc, dst, n, PlainFin<Tr>{});
}
template <class Tr>
__global__ void __launch_bounds__(kThreads)
    reduce_tree_elem_scaled_kernel(Srcs<FTAR_MAX_K> src, int k, TreeCode tc, void* dst, size_t n,
                                   typename Tr::SC scale) {
  reduce_tree_elem_body<Tr>(src, k, tc, dst, n, ScaledFin<Tr>{scale});
}
template <class Tr>
__global__ void __launch_bounds__(kThreads)
    reduce_tree_elem_amax_kernel(Srcs<FTAR_MAX_K> src, int k, TreeCode tc, void* dst, size_t n,
                                 typename Tr::SC scale, unsigned* amax) {
  reduce_tree_elem_body<Tr>(src, k, tc, dst, n, AmaxFin<Tr>{scale, amax});
}

// The nested fold on the LDS-staged tile loop (lds_staged): the production
// path for the multi-stage trees' one-round reduce-scatter up to 16 ranks.
// Compile-time shapes (Sh = StaticShape) fold to straight-line adds; other
// shapes read the leaf codes from the kernarg.
template <class Tr, int K, int U, int W, class Sh, class Fin>
__device__ __forceinline__ void reduce_tree_lds_body(const Srcs<K>& src, const TreeCode& tc, void* dst, size_t nvec,
                                                     int head, int tail, Fin fin) {
  using O = TreeOps<Tr, true>;
  unsigned* const lds = lds_staged<Tr, K, U, W, 2, true>(
      src, dst, nvec, head, tail,
      [&](auto get) {
        typename O::A acc[kTreeLevels][1], v[1];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          v[0] = Tr::v_init(get(j));
          if constexpr (std::is_same_v<Sh, RuntimeShape>) tree_push<Fin::kRawRoot, O, 1>(acc, v, tc.c[j], j == K - 1);
          else tree_push<Fin::kRawRoot, O, 1>(acc, v, Sh::code(j), j == K - 1);
        }
        return fin.v(v[0]);
      },
      [&](size_t e) { return tree_elem<Tr>(src.p, K, tc, e, fin); });
  if constexpr (kIsAmax<Fin>) fin.flush(lds, kLdsWaveWords<K, U>);
  else (void)lds;
}
template <class Tr, int K, int U, int W, class Sh>
__global__ void __launch_bounds__(W * 64)
    reduce_tree_lds_kernel(Srcs<K> src, TreeCode tc, void* dst, size_t nvec, int head, int tail) {
  reduce_tree_lds_body<Tr, K, U, W, Sh>(src, tc, dst, nvec, head, tail, PlainFin<Tr>{});
}
template <class Tr, int K, int U, int W, class Sh>
__global__ void __launch_bounds__(W * 64)
    reduce_tree_lds_scaled_kernel(Srcs<K> src, TreeCode tc, void* dst, size_t nvec, int head, int tail,
                                  typename Tr::SC scale) {
  reduce_tree_lds_body<Tr, K, U, W, Sh>(src, tc, dst, nvec, head, tail, ScaledFin<Tr>{scale});
}
template <class Tr, int K, int U, int W, class Sh>
__global__ void __launch_bounds__(W * 64)
    reduce_tree_lds_amax_kernel(Srcs<K> src, TreeCode tc, void* dst, size_t nvec, int head, int tail,
                                typename Tr::SC scale, unsigned* amax) {
  reduce_tree_lds_body<Tr, K, U, W, Sh>(src, tc, dst, nvec, head, tail, AmaxFin<Tr>{scale, amax});
}

// ---------------------------------------------------------------------------
// multi-segment copy: the peer-direct all-gather pulls every rank's final block
// (over xGMI) into the caller's buffer in ONE launch.  Workgroup w copies
// piece w / m of segment w % m: consecutive workgroups -- the ones resident
// at the same time -- pull from different ranks, so every link streams at
// once (a grid.y = segment layout would dispatch segment 0's workgroups
// first and drive one link at a time).  16 B per lane per access when source and destination
// share their address mod 16 (always, in the all-gather: both sit at the same
// block offset of 256-B aligned buffers); bytes otherwise.
// ---------------------------------------------------------------------------
struct SegArgs {
  const char* src[FTAR_MAX_K];
  char* dst[FTAR_MAX_K];
  size_t bytes[FTAR_MAX_K];
};

template <bool NT>
__device__ __forceinline__ void gather_body(const SegArgs& a, int m) {
  const int sgi = (int)(blockIdx.x % (unsigned)m);
  const size_t bid = blockIdx.x / (unsigned)m, nb = gridDim.x / (unsigned)m;
  const char* src = a.src[sgi];
  char* dst = a.dst[sgi];
  const size_t n = a.bytes[sgi];
  const size_t tid = bid * kThreads + threadIdx.x, nthr = nb * kThreads;
  const uintptr_t ms = reinterpret_cast<uintptr_t>(src) & 15, md = reinterpret_cast<uintptr_t>(dst) & 15;
  if (ms != md) {
    for (size_t i = tid; i < n; i += nthr) dst[i] = src[i];
    return;
  }
  size_t head = ms ? 16 - ms : 0;
  if (head > n) head = n;
  const size_t nvec = (n - head) / 16, tail_at = head + nvec * 16;
  if (tid < head) dst[tid] = src[tid];
  if (tid < n - tail_at) dst[tail_at + tid] = src[tail_at + tid];
  const u32x4* s4 = reinterpret_cast<const u32x4*>(src + head);
  u32x4* d4 = reinterpret_cast<u32x4*>(dst + head);
  size_t v = bid * (2 * kThreads) + threadIdx.x;
  const size_t stride = nb * (2 * kThreads);
  for (; v + kThreads < nvec; v += stride) {  // streaming both ways (cold copy: 6.3 vs 5.5 TB/s for the DMA blit)
    const u32x4 x0 = ld16<NT>(s4 + v), x1 = ld16<NT>(s4 + v + kThreads);
    st16<NT>(d4 + v, x0);
    st16<NT>(d4 + v + kThreads, x1);
  }
  if (v < nvec) st16<NT>(d4 + v, ld16<NT>(s4 + v));
}

template <bool NT, bool REL = false>
__global__ void __launch_bounds__(kThreads) gather_kernel(SegArgs a, int m) {
  gather_body<NT>(a, m);
  if constexpr (REL) __threadfence_system();  // this workgroup's stores reach memory before it retires
}

// Diagnostic (engine_host.cpp FTAR_DEBUG_HOST_GATHER_LOG): the gather, and when every wave of
// the workgroup has issued its stores, one record of where and when it ran in host memory (fine-grained, not
// held in the GPU caches) {0x80000000 | XCD, HW_ID (CU, SIMD, queue, pipe), wall clock at start, at end}, and
// two device-scope atomics on its workgroup id's pair of words in device memory: how many times a workgroup
// with this id ran (0: never; 2: the id handed out twice) and the set of XCDs it ran on (bit x: XCD x).
template <bool NT>
__global__ void __launch_bounds__(kThreads) gather_logged_kernel(SegArgs a, int m, unsigned* host_log,
                                                                 unsigned* dev_log) {
  const unsigned t0 = (unsigned)wall_clock64();
  gather_body<NT>(a, m);
  __syncthreads();
  if (threadIdx.x == 0) {
    // s_getreg: HW_REG_XCC_ID (20) bits [3:0], HW_REG_HW_ID (4) whole
    const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (15 << 11)) & 15u;
    const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));
    const unsigned t1 = (unsigned)wall_clock64();
    unsigned* h = host_log + 4 * (size_t)blockIdx.x;
    h[0] = 0x80000000u | xcc;
    h[1] = hw;
    h[2] = t0;
    h[3] = t1;
    atomicAdd(dev_log + 2 * (size_t)blockIdx.x, 1u);
    atomicOr(dev_log + 2 * (size_t)blockIdx.x + 1, 1u << xcc);
  }
}

// ---------------------------------------------------------------------------
// host-side launch
// ---------------------------------------------------------------------------

// What every launcher below takes of one fold, beside the geometry it launches on: the k sources, the
// destination, the stream, and the two arguments of the finishes (r: the scale of the scaled and the amax finish;
// am: the amax word of the latter; a plain launch reads neither).
struct Launch {
  const void* const* srcs;
  int k;
  void* dst;
  hipStream_t s;
  double r = 1.0;
  unsigned* am = nullptr;
};
inline Launch launch_of(const FoldCall& f) {
  return {f.srcs, f.k, f.dst, f.stream, f.scale ? *f.scale : 1.0, f.amax};
}

// How `count` elements of `esz` bytes at dst split for 16-byte access (launch_tr, launch_tree, launch_copy):
// `head` elements up to dst's first aligned address, nvec vectors, `tail` elements (head and tail are workgroup
// 0's, element-wise, in the same launch).  co_aligned: dst is element-aligned and every source sits at dst's
// address mod 16; otherwise the caller takes an element-wise kernel and the rest stays 0.
struct Split16 {
  bool co_aligned;
  int head = 0, tail = 0;
  size_t nvec = 0;
};
inline Split16 split16(const void* const* srcs, int k, const void* dst, size_t count, size_t esz) {
  const uintptr_t mis = reinterpret_cast<uintptr_t>(dst) & 15;
  bool co_aligned = (mis % esz) == 0;
  for (int j = 0; j < k && co_aligned; ++j) co_aligned = (reinterpret_cast<uintptr_t>(srcs[j]) & 15) == mis;
  if (!co_aligned) return {false};
  size_t head = mis ? (16 - mis) / esz : 0;
  if (head > count) head = count;
  const size_t nvec = (count - head) / (16 / esz);
  return {true, (int)head, (int)(count - head - nvec * (16 / esz)), nvec};
}
// grid of the element-wise kernels: grid-stride beyond 8192 workgroups
inline unsigned elem_blocks(size_t count) { return (unsigned)std::min<size_t>((count + kThreads - 1) / kThreads, 8192); }

template <class Tr, int K, int U, int W = 4, int AUX = 2, bool PROG = true, int SC = kFinPlain>
hipError_t launch_lds(const Launch& c, const Split16& sp) {
  if constexpr (W * U * K > 160) {
    return hipErrorInvalidValue;
  } else {
    const size_t per_block = (size_t)W * U * 64;
    const size_t blocks = (sp.nvec + per_block - 1) / per_block;
    const dim3 grid((unsigned)(blocks ? blocks : 1));
    FTAR_LAUNCH_FIN(SC, (typename Tr::SC)c.r, c.am, reduce_lds, (Tr, K, U, W, AUX, PROG), grid, dim3(W * 64), 0, c.s,
                    pack_srcs<K>(c.srcs, K), c.dst, sp.nvec, sp.head, sp.tail);
    return hipGetLastError();
  }
}

template <class Tr, int K, int U, bool NTL, bool NTS, int BS, int SC = kFinPlain>
hipError_t launch_cfg(const Launch& c, const Split16& sp, size_t max_blocks = 0) {
  constexpr int KK = K > 0 ? K : FTAR_MAX_K;
  const size_t per_block = (size_t)U * BS;
  size_t blocks = (sp.nvec + per_block - 1) / per_block;
  if (blocks == 0) blocks = 1;  // head/tail only
  if (max_blocks && blocks > max_blocks) blocks = max_blocks;  // grid-stride over the rest
  if (blocks > 0x7fffffffull) blocks = 0x7fffffffull;
  FTAR_LAUNCH_FIN(SC, (typename Tr::SC)c.r, c.am, reduce_vec, (Tr, K, U, NTL, NTS, BS), dim3((unsigned)blocks), dim3(BS), 0,
                  c.s, pack_srcs<KK>(c.srcs, c.k), c.k, c.dst, sp.nvec, sp.head, sp.tail);
  return hipGetLastError();
}

template <class Tr, int K, int SC = kFinPlain>
hipError_t launch_k(const Launch& c, const Split16& sp) {
  // the amax finish ends every workgroup with a reduction and one L2 read: the 4-byte k = 2 shape of two-wave,
  // one-tile workgroups (131,072 of them on 256 MiB) pays it eight times as often as 4 x 4, the 2-byte shape
  constexpr bool kWide = SC == kFinAmax && K == 2 && sizeof(typename Tr::S) >= 4;
  if constexpr (K >= 2)
    return launch_lds<Tr, K, (kWide ? 4 : kLdsTiles<Tr, K>), (kWide ? 4 : kLdsWaves<Tr, K>), 2, true, SC>(c, sp);
  else
    return launch_cfg<Tr, K, kUnroll, kNtLoads, kNtStores, kVecThreads, SC>(c, sp);
}

// Leaf codes of a nested fold with bottom-up widths shape[0..nlevels) over k
// leaves (see reduce_tree_kernel).
bool make_tree_code(const int* shape, int nlevels, int k, TreeCode* tc) {
  if (nlevels < 1 || nlevels > kTreeLevels || k > FTAR_MAX_K) return false;
  size_t prod = 1;
  for (int l = 0; l < nlevels; ++l) {
    if (shape[l] < 1) return false;
    prod *= (size_t)shape[l];
  }
  if (prod != (size_t)k) return false;
  for (int j = 0; j < k; ++j) tc->c[j] = (unsigned char)leaf_code(shape, nlevels, j);
  return true;
}
// A nested fold on the host: its widths (launch_tree picks the compile-time shapes by them) and the leaf codes
// make_tree_code made of them (the kernels' argument).
struct Tree {
  const int* shape;
  int nlevels;
  TreeCode code;
};

template <class Tr, int K, int U, class Sh = RuntimeShape, int SC = kFinPlain>
hipError_t launch_tree_k(const Launch& c, const Tree& t, const Split16& sp) {
  constexpr int KK = K > 0 ? K : FTAR_MAX_K;
  size_t blocks = (sp.nvec + (size_t)U * kThreads - 1) / ((size_t)U * kThreads);
  if (blocks == 0) blocks = 1;
  if (blocks > 0x7fffffffull) blocks = 0x7fffffffull;
  FTAR_LAUNCH_FIN(SC, (typename Tr::SC)c.r, c.am, reduce_tree, (Tr, K, U, Sh), dim3((unsigned)blocks), dim3(kThreads), 0,
                  c.s, pack_srcs<KK>(c.srcs, c.k), c.k, t.code, c.dst, sp.nvec, sp.head, sp.tail);
  return hipGetLastError();
}

template <class Tr, int K, class Sh = RuntimeShape, int SC = kFinPlain>
hipError_t launch_tree_lds(const Launch& c, const Tree& t, const Split16& sp) {
  constexpr int U = kLdsTiles<Tr, K>, W = kLdsWaves<Tr, K>;
  const size_t per_block = (size_t)W * U * 64;
  const size_t blocks = (sp.nvec + per_block - 1) / per_block;
  FTAR_LAUNCH_FIN(SC, (typename Tr::SC)c.r, c.am, reduce_tree_lds, (Tr, K, U, W, Sh), dim3((unsigned)(blocks ? blocks : 1)),
                  dim3(W * 64), 0, c.s, pack_srcs<K>(c.srcs, K), t.code, c.dst, sp.nvec, sp.head, sp.tail);
  return hipGetLastError();
}

template <class Tr, int SC = kFinPlain>
hipError_t launch_tree(const Launch& c, const Tree& t, size_t count, bool lds) {
  using S = typename Tr::S;
  const Split16 sp = split16(c.srcs, c.k, c.dst, count, sizeof(S));
  if (!sp.co_aligned) {
    FTAR_LAUNCH_FIN(SC, (typename Tr::SC)c.r, c.am, reduce_tree_elem, (Tr), dim3(elem_blocks(count)), dim3(kThreads), 0,
                    c.s, pack_srcs<FTAR_MAX_K>(c.srcs, c.k), c.k, t.code, c.dst, count);
    return hipGetLastError();
  }
  auto is = [&](std::initializer_list<int> w) {
    return (int)w.size() == t.nlevels && std::equal(w.begin(), w.end(), t.shape);
  };
  // the multi-stage trees of 4, 8 and 16 ranks: compile-time shapes.
  // LDS-staged (production, round 2): cold A/B against the register kernel
  // (profiles/r02/kbench_cold_nested_lds.log): fp32 +4 to +10 % on every
  // shape; bf16 +4 to +8 % on the two-level shapes, and since bf16 rounds with
  // v_cvt_pk_bf16_f32 (kLdsDeepBf16) on (2,2,2) and (2,2,2,2) too; its
  // runtime-coded folds still lose there and keep the register kernel.
  if (lds) {
    if (is({2, 2})) return launch_tree_lds<Tr, 4, StaticShape<2, 2>, SC>(c, t, sp);
    if (is({2, 4})) return launch_tree_lds<Tr, 8, StaticShape<2, 4>, SC>(c, t, sp);
    if (is({4, 2})) return launch_tree_lds<Tr, 8, StaticShape<4, 2>, SC>(c, t, sp);
    if (is({4, 4})) return launch_tree_lds<Tr, 16, StaticShape<4, 4>, SC>(c, t, sp);
  }
  if (lds && (sizeof(S) >= 4 || kLdsDeepBf16)) {
    if (is({2, 2, 2})) return launch_tree_lds<Tr, 8, StaticShape<2, 2, 2>, SC>(c, t, sp);
    if (is({2, 2, 2, 2})) return launch_tree_lds<Tr, 16, StaticShape<2, 2, 2, 2>, SC>(c, t, sp);
  }
  if (lds && sizeof(S) >= 4) {
    switch (c.k) {  // other shapes: runtime leaf codes
      case 4: return launch_tree_lds<Tr, 4, RuntimeShape, SC>(c, t, sp);
      case 6: return launch_tree_lds<Tr, 6, RuntimeShape, SC>(c, t, sp);
      case 8: return launch_tree_lds<Tr, 8, RuntimeShape, SC>(c, t, sp);
      case 9: return launch_tree_lds<Tr, 9, RuntimeShape, SC>(c, t, sp);
      case 12: return launch_tree_lds<Tr, 12, RuntimeShape, SC>(c, t, sp);
      case 16: return launch_tree_lds<Tr, 16, RuntimeShape, SC>(c, t, sp);
      default: break;
    }
    return launch_tree_k<Tr, 0, 2, RuntimeShape, SC>(c, t, sp);
  }
  // registers (round 1; the A/B reference of ftar_debug_reduce_nested_lds)
  if (is({2, 2})) return launch_tree_k<Tr, 4, 2, StaticShape<2, 2>, SC>(c, t, sp);
  if (is({2, 4})) return launch_tree_k<Tr, 8, 2, StaticShape<2, 4>, SC>(c, t, sp);
  if (is({4, 2})) return launch_tree_k<Tr, 8, 2, StaticShape<4, 2>, SC>(c, t, sp);
  if (is({2, 2, 2})) return launch_tree_k<Tr, 8, 2, StaticShape<2, 2, 2>, SC>(c, t, sp);
  if (is({4, 4})) return launch_tree_k<Tr, 16, 1, StaticShape<4, 4>, SC>(c, t, sp);
  if (is({2, 2, 2, 2})) return launch_tree_k<Tr, 16, 1, StaticShape<2, 2, 2, 2>, SC>(c, t, sp);
  switch (c.k) {  // other shapes: runtime leaf codes; 16 sources fit one vector per lane
    case 4: return launch_tree_k<Tr, 4, 2, RuntimeShape, SC>(c, t, sp);
    case 6: return launch_tree_k<Tr, 6, 2, RuntimeShape, SC>(c, t, sp);
    case 8: return launch_tree_k<Tr, 8, 2, RuntimeShape, SC>(c, t, sp);
    case 16: return launch_tree_k<Tr, 16, 1, RuntimeShape, SC>(c, t, sp);
    default: return launch_tree_k<Tr, 0, 2, RuntimeShape, SC>(c, t, sp);
  }
}

// The flat fold.  HOT: the largest k with an unrolled LDS-staged kernel (fp32/bf16/fp16 16, the other types, fp8
// included, 8); larger k take the runtime-k register kernel, and so does every k > 2 when lds is false (the peer
// forms' ":vec" A/B).  The other types gained 4-6 % at k = 8 on the LDS kernel (tools/dtype_rates.py,
// profiles/r02/s4/dtype_rates*.log).
template <class Tr, int HOT, int SC = kFinPlain>
hipError_t launch_tr(const Launch& c, size_t count, bool lds = true) {
  static_assert(HOT >= 2);
  const Split16 sp = split16(c.srcs, c.k, c.dst, count, sizeof(typename Tr::S));
  if (!sp.co_aligned) {
    FTAR_LAUNCH_FIN(SC, (typename Tr::SC)c.r, c.am, reduce_elem, (Tr), dim3(elem_blocks(count)), dim3(kThreads), 0, c.s,
                    pack_srcs<FTAR_MAX_K>(c.srcs, c.k), c.k, c.dst, count);
    return hipGetLastError();
  }
  hipError_t e = hipErrorInvalidValue;
  bool done = false;
  [&]<int... I>(std::integer_sequence<int, I...>) {  // k = 2 .. HOT, unrolled
    ((c.k == I + 2 && (I + 2 == 2 || lds) ? (e = launch_k<Tr, I + 2, SC>(c, sp), done = true) : false), ...);
  }(std::make_integer_sequence<int, HOT - 1>{});
  if (done) return e;
  return launch_k<Tr, 0, SC>(c, sp);
}

// One dtype's SUM in the finish SC, nested or flat -- the one place that decides between the nested kernels, a
// one-round ring hop and the flat fold.  Sum: the dtype's trait; Hop: the one of a one-round ring fold
// (round_each, k > 2), which rounds to the format after every add; HopPre: its form under a scaled or an amax
// finish, which rounds before each add instead, so the last sum reaches the finish unrounded, as the staged
// ring's last hop (a plain k = 2 fold) hands it over.  f32 and f64, which round nowhere, pass Sum for both.  Only
// the hop trait of this finish is named, so only its kernels are instantiated: a plain launch never names a
// HopPre kernel, nor a scaled or amax one a Hop kernel.  TREE_LDS false (f64): nested folds stay on the register
// kernels.
template <class Sum, class Hop, class HopPre, int HOT, int SC, bool TREE_LDS = true>
ftar_status_t launch_sum(const FoldCall& f) {
  const Launch c = launch_of(f);
  hipError_t e;
  if (f.nlevels > 1 && f.k > 1) {
    Tree t{f.shape, f.nlevels, {}};
    if (!f.shape || !make_tree_code(f.shape, f.nlevels, f.k, &t.code)) return FTAR_ERR_INVALID_ARG;
    e = launch_tree<Sum, SC>(c, t, f.count, f.lds && TREE_LDS);
  } else if (f.round_each && f.k > 2) {
    e = launch_tr<std::conditional_t<SC != kFinPlain, HopPre, Hop>, HOT, SC>(c, f.count, f.lds);
  } else {
    e = launch_tr<Sum, HOT, SC>(c, f.count, f.lds);
  }
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}

}  // namespace
}  // namespace ftar
