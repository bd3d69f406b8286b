// libftar_bench.so: the A/B harness of the reduce kernels and kernel-level test hooks, kept OUT of the
// product library (libftar.so holds only the kernels launch_reduce / launch_tree / launch_copy /
// launch_gather dispatch).  Not part of ftar.h; loaded by tools/kbench*.py, the bf16 conversion test and the
// kernel-edge tests (ftar_debug_reduce_ex, ftar_debug_reduce_amax_ex, ftar_debug_gather) through ftar.bench_lib().  Shape, cache-policy and dtype variants of the production kernels in
// reduce_impl.h are instantiated here from the same templates; launch_gather (variant 90) and
// launch_reduce (the nested-fold A/B) are the product's own, linked from libftar.so.
#include "cast_impl.h"
#include "mx_impl.h"
#include "reduce_impl.h"

namespace ftar {

// ---------------------------------------------------------------------------
// A/B variants for tools/kbench.py (not part of ftar.h): (U, NT loads, NT
// stores, workgroup size, grid cap) for fp32 and bf16 sums, k in {2, 4, 8}.
// ---------------------------------------------------------------------------
namespace {
// progressive LDS-staged kernel: (tiles per wave U, waves per workgroup W)
template <class Tr, int K>
hipError_t variant_prog(int v, const Launch& c, const Split16& sp) {
  switch (v) {
    case 40: return launch_lds<Tr, K, 4, 4>(c, sp);
    case 41: return launch_lds<Tr, K, 3, 4>(c, sp);
    case 42: return launch_lds<Tr, K, 2, 4>(c, sp);
    case 43: return launch_lds<Tr, K, 4, 2>(c, sp);
    case 44: return launch_lds<Tr, K, 3, 6>(c, sp);
    case 45: return launch_lds<Tr, K, 2, 6>(c, sp);
    case 46: return launch_lds<Tr, K, 2, 8>(c, sp);
    case 47: return launch_lds<Tr, K, 1, 8>(c, sp);
    case 48: return launch_lds<Tr, K, 3, 2>(c, sp);
    case 49: return launch_lds<Tr, K, 6, 2>(c, sp);
    case 50: return launch_lds<Tr, K, 2, 2>(c, sp);
    case 51: return launch_lds<Tr, K, 1, 4>(c, sp);
    case 52: return launch_lds<Tr, K, 5, 2>(c, sp);
    case 53: return launch_lds<Tr, K, 2, 5>(c, sp);
    // small workgroups, many per CU (round 2: tools/kexp/k8_exp.hip found U1 W2 / U2 W1 ahead at k = 2..9)
    case 54: return launch_lds<Tr, K, 1, 2>(c, sp);
    case 55: return launch_lds<Tr, K, 1, 1>(c, sp);
    case 56: return launch_lds<Tr, K, 2, 1>(c, sp);
    case 57: return launch_lds<Tr, K, 1, 3>(c, sp);
    case 58: return launch_lds<Tr, K, 3, 1>(c, sp);
    case 59: return launch_lds<Tr, K, 4, 1>(c, sp);
    // load cache policy (the aux operand of global_load_lds) at the production shape: 2 = nt (production)
    case 60: return launch_lds<Tr, K, kLdsTiles<Tr, K>, kLdsWaves<Tr, K>, 1>(c, sp);
    case 61: return launch_lds<Tr, K, kLdsTiles<Tr, K>, kLdsWaves<Tr, K>, 3>(c, sp);
    case 62: return launch_lds<Tr, K, kLdsTiles<Tr, K>, kLdsWaves<Tr, K>, 2>(c, sp);
  }
  return hipErrorInvalidValue;
}
template <class Tr, int K>
hipError_t variant_k(int v, const Launch& c, const Split16& sp) {
  switch (v) {
    case 0: return launch_cfg<Tr, K, 2, true, false, 256>(c, sp);
    case 1: return launch_cfg<Tr, K, 1, true, false, 256>(c, sp);
    case 2: return launch_cfg<Tr, K, 4, true, false, 256>(c, sp);
    case 3: return launch_cfg<Tr, K, 1, true, false, 512>(c, sp);
    case 4: return launch_cfg<Tr, K, 2, true, false, 512>(c, sp);
    case 5: return launch_cfg<Tr, K, 1, true, false, 1024>(c, sp);
    case 6: return launch_cfg<Tr, K, 2, true, false, 128>(c, sp);
    case 7: return launch_cfg<Tr, K, 2, false, false, 256>(c, sp);
    case 8: return launch_cfg<Tr, K, 1, true, false, 256>(c, sp, 2048);
    case 9: return launch_cfg<Tr, K, 2, true, false, 256>(c, sp, 4096);
    case 10: return launch_cfg<Tr, K, 1, true, false, 128>(c, sp);
    case 11: return launch_cfg<Tr, K, 4, true, false, 128>(c, sp);
    case 12: return launch_cfg<Tr, K, 2, true, true, 256>(c, sp);   // nt stores
    case 13: return launch_cfg<Tr, K, 1, true, true, 256>(c, sp);
    case 14: return launch_cfg<Tr, K, 4, true, true, 256>(c, sp);
    case 15: return launch_cfg<Tr, K, 2, false, true, 256>(c, sp);
    case 16: return launch_cfg<Tr, K, 2, true, true, 512>(c, sp);
    case 17: return launch_cfg<Tr, K, 4, true, false, 256>(c, sp, 4096);
    case 18: return launch_cfg<Tr, K, 2, true, true, 256>(c, sp, 8192);
    case 19: return launch_cfg<Tr, K, 4, true, true, 512>(c, sp);
    case 23: return launch_cfg<Tr, K, 4, true, true, 128>(c, sp);
    case 24: return launch_cfg<Tr, K, 8, true, true, 256>(c, sp);
    case 25: return launch_cfg<Tr, K, 2, true, true, 128>(c, sp);
    case 26: return launch_cfg<Tr, K, 1, true, true, 512>(c, sp);
    case 31: return launch_lds<Tr, K, (K <= 4 ? 4 : 2), 4, 2, false>(c, sp);
    case 32: return launch_lds<Tr, K, (K <= 4 ? 4 : (K <= 6 ? 3 : 2)), 4, 2, false>(c, sp);
    case 33: return launch_lds<Tr, K, 1, 4, 2, false>(c, sp);
    case 27: return launch_cfg<Tr, 0, 2, true, true, 512>(c, sp);  // runtime-k loop
    case 28: return launch_cfg<Tr, 0, 4, true, true, 256>(c, sp);
    case 29: return launch_cfg<Tr, 0, 1, true, true, 512>(c, sp);
    case 30: return launch_cfg<Tr, 0, 2, true, true, 256>(c, sp);
    case 20: return launch_lds<Tr, K, 2, 4, 2, false>(c, sp);  // LDS-DMA, nt, wait for all
    case 21: return launch_lds<Tr, K, 4, 4, 2, false>(c, sp);
    case 22: return launch_lds<Tr, K, 2, 4, 0, false>(c, sp);  // LDS-DMA, default policy
  }
  return variant_prog<Tr, K>(v, c, sp);
}
// k = 1 (a copy, vector_add/reduce_sum.h:36-47): variant 90 = production (the streaming copy kernel,
// launch_gather), 40-62 = the LDS-DMA-staged kernel with K = 1 (load to LDS, store from LDS)
template <class Tr>
hipError_t variant_copy(int v, const Launch& c, const Split16& sp) {
  if (v == 90) {
    const Segment seg{c.srcs[0], c.dst, sp.nvec * 16};
    return launch_gather(&seg, 1, c.s) == FTAR_SUCCESS ? hipSuccess : hipErrorInvalidValue;
  }
  return variant_prog<Tr, 1>(v, c, sp);
}

template <class Tr>
hipError_t variant_tr(int v, const Launch& c, const Split16& sp) {
  switch (c.k) {
    case 1: return variant_copy<Tr>(v, c, sp);
    case 2: return variant_k<Tr, 2>(v, c, sp);
    case 3: return variant_k<Tr, 3>(v, c, sp);
    case 4: return variant_k<Tr, 4>(v, c, sp);
    case 5: return variant_prog<Tr, 5>(v, c, sp);
    case 6: return variant_k<Tr, 6>(v, c, sp);
    case 7: return variant_prog<Tr, 7>(v, c, sp);
    case 8: return variant_k<Tr, 8>(v, c, sp);
    case 10: return variant_prog<Tr, 10>(v, c, sp);
    case 12: return variant_prog<Tr, 12>(v, c, sp);
    case 16: return variant_prog<Tr, 16>(v, c, sp);
  }
  return hipErrorInvalidValue;
}
}  // namespace

hipError_t hop_variant(int v, const Launch& c, const Split16& sp) {
  switch (c.k) {
    case 2: return variant_prog<BF16SumHop, 2>(v, c, sp);
    case 4: return variant_prog<BF16SumHop, 4>(v, c, sp);
    case 8: return variant_prog<BF16SumHop, 8>(v, c, sp);
    case 16: return variant_prog<BF16SumHop, 16>(v, c, sp);
  }
  return hipErrorInvalidValue;
}

// the fp8 A/B (profiles/f8/): the (U, W) shapes 40-62 at k = 2 and 8 for one fp8 trait
template <class Tr>
hipError_t f8_variant(int v, const Launch& c, const Split16& sp) {
  switch (c.k) {
    case 2: return variant_prog<Tr, 2>(v, c, sp);
    case 8: return variant_prog<Tr, 8>(v, c, sp);
  }
  return hipErrorInvalidValue;
}

}  // namespace ftar

extern "C" ftar_status_t ftar_debug_reduce_variant(int variant, int dtype, const void* const* srcs, int k, void* dst,
                                                   size_t count, void* stream) {
  if (reinterpret_cast<uintptr_t>(dst) & 15) return FTAR_ERR_INVALID_ARG;
  const ftar::Launch c{srcs, k, dst, static_cast<hipStream_t>(stream)};
  auto vecs = [&](size_t per) { return ftar::Split16{true, 0, 0, count / per}; };  // whole vectors, aligned: no head or tail
  hipError_t e;
  if (dtype == FTAR_FLOAT32 && count % 4 == 0) e = ftar::variant_tr<ftar::F32Sum>(variant, c, vecs(4));
  else if (dtype == FTAR_BFLOAT16 && count % 8 == 0)
    e = ftar::variant_tr<ftar::BF16Sum>(variant, c, vecs(8));
  // 100 + bf16: the ring's hop fold (rounds after every add), production shape (variant 62), k = 2, 4, 8, 16.
  // (The round-2 A/B of the two bf16 conversions, profiles/r02/s4/kbench_bf16_cvt.log, also built
  // 200 + bf16 / 300 + bf16 for the flat and hop folds with the integer RNE; dropped to keep build time.)
  else if (dtype == 100 + FTAR_BFLOAT16 && count % 8 == 0)
    e = ftar::hop_variant(variant, c, vecs(8));
  // (The A/B of the 2-byte MAX traits, profiles/f16_minmax/kbench_2byte_max.log, also built the shape sweep
  // (variants 40-62, k = 2 and 8) for fp16 SUM, u16 SUM, 200 + f16 / 200 + i16 = MAX, and 300 + f16 = fp16 MAX by
  // integer keys (sign-magnitude flipped to two's complement per packed half, v_pk_max_i16, NaN lanes collected
  // apart); dropped to keep build time.)
  // e4m3 (e5m2 runs the same instructions under other opcodes): the SUM, 200 + e4m3 = MAX as production does it
  // (widen, fp32 maximum, narrow), 300 + e4m3 = MAX by integer keys on the bytes (F8KeyMinMax); k = 2 and 8
  else if (dtype == FTAR_FLOAT8_E4M3 && count % 16 == 0)
    e = ftar::f8_variant<ftar::E4M3Sum>(variant, c, vecs(16));
  else if (dtype == 200 + FTAR_FLOAT8_E4M3 && count % 16 == 0)
    e = ftar::f8_variant<ftar::F8MinMax<ftar::E4M3Fmt, true>>(variant, c, vecs(16));
  else if (dtype == 300 + FTAR_FLOAT8_E4M3 && count % 16 == 0)
    e = ftar::f8_variant<ftar::F8KeyMinMax<false, true>>(variant, c, vecs(16));
  else return FTAR_ERR_INVALID_ARG;
  return e == hipSuccess ? FTAR_SUCCESS : FTAR_ERR_HIP;
}

// A/B of the nested fold: lds = 1 the LDS-staged kernel (production), 0 the
// register kernel of round 1 (tools/kbench_cold.py --shapes).
extern "C" ftar_status_t ftar_debug_reduce_nested_lds(int lds, const void* const* srcs, int k, void* dst, size_t count,
                                                      int dtype, const int* shape, int nlevels, void* stream) {
  ftar::FoldCall f;
  f.srcs = srcs; f.k = k; f.dst = dst; f.count = count; f.dt = (ftar_dtype_t)dtype;
  f.stream = static_cast<hipStream_t>(stream);
  f.shape = shape; f.nlevels = nlevels; f.lds = lds != 0;
  return ftar::launch_reduce(f);
}

// Test hooks of the kernel-edge tests (tests/kernel_edges.py): the product's own launchers with every argument
// the engine can give them, each passed to launch_reduce unchanged (round_each: the hop folds; lds = 0: the peer
// forms' ":vec" dispatch and the register tree kernels; scale may be NULL, and launch_reduce refuses an amax
// without one).  The amax word is NOT zeroed here: what it holds before the launch is the caller's to decide, as
// it is the engine's, whose pieces max into one word launch after launch.
extern "C" ftar_status_t ftar_debug_reduce_amax_ex(const void* const* srcs, int k, void* dst, size_t count, int dtype,
                                                   int op, int round_each, const int* shape, int nlevels, int lds,
                                                   const double* scale, unsigned* amax, void* stream) {
  ftar::FoldCall f;
  f.srcs = srcs; f.k = k; f.dst = dst; f.count = count; f.dt = (ftar_dtype_t)dtype;
  f.op = (ftar_op_t)op; f.stream = static_cast<hipStream_t>(stream); f.round_each = round_each != 0;
  f.shape = shape; f.nlevels = nlevels; f.lds = lds != 0; f.scale = scale; f.amax = amax;
  return ftar::launch_reduce(f);
}
// The same without an amax word.
extern "C" ftar_status_t ftar_debug_reduce_ex(const void* const* srcs, int k, void* dst, size_t count, int dtype, int op,
                                              int round_each, const int* shape, int nlevels, int lds,
                                              const double* scale, void* stream) {
  return ftar_debug_reduce_amax_ex(srcs, k, dst, count, dtype, op, round_each, shape, nlevels, lds, scale, nullptr, stream);
}

// launch_gather on dsts[i][0..bytes[i]) = srcs[i][0..bytes[i]), i < nsegs (zero-byte segments included: the
// launcher packs them out); nsegs outside 0..FTAR_MAX_K is the launcher's to refuse.
extern "C" ftar_status_t ftar_debug_gather(const void* const* srcs, void* const* dsts, const size_t* bytes, int nsegs,
                                           int nt, size_t max_wg_per_seg, int release_system, void* stream) {
  if (nsegs < 0 || nsegs > FTAR_MAX_K) return FTAR_ERR_INVALID_ARG;
  if (nsegs && (!srcs || !dsts || !bytes)) return FTAR_ERR_INVALID_ARG;
  ftar::Segment segs[FTAR_MAX_K];
  for (int i = 0; i < nsegs; ++i) segs[i] = ftar::Segment{srcs[i], dsts[i], bytes[i]};
  return ftar::launch_gather(segs, nsegs, static_cast<hipStream_t>(stream), nt != 0, max_wg_per_seg,
                             release_system != 0);
}

namespace ftar {
namespace {
// every float bit pattern u (lo half) and u ^ 0x80000001 (hi half) through both bf16 conversions
__global__ void __launch_bounds__(256) bf16_cvt_check_kernel(unsigned long long* bad, unsigned* first) {
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  unsigned long long mine = 0;
  unsigned first_mine = 0xffffffffu;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < (1ull << 32); i += stride) {
    const unsigned u = (unsigned)i, v = u ^ 0x80000001u;
    const float lo = __uint_as_float(u), hi = __uint_as_float(v);
    if (pack_bf16<true>(lo, hi) != pack_bf16<false>(lo, hi)) {
      ++mine;
      first_mine = first_mine < u ? first_mine : u;
    }
  }
  if (mine) {
    atomicAdd(bad, mine);
    atomicMin(first, first_mine);
  }
}
}  // namespace
}  // namespace ftar

// Test hook (not in ftar.h): how many of the 2^32 float bit patterns convert to different bf16 bits
// through v_cvt_pk_bf16_f32 than through the bit-exact RNE (bf16_round_bits); the first such pattern.
extern "C" ftar_status_t ftar_debug_bf16_cvt_check(unsigned long long* mismatches, unsigned* first) {
  if (!mismatches || !first) return FTAR_ERR_INVALID_ARG;
  unsigned long long* d_bad = nullptr;
  unsigned* d_first = nullptr;
  ftar_status_t st = FTAR_SUCCESS;  // both buffers are freed on every path below
  if (hipMalloc(&d_bad, sizeof *d_bad) != hipSuccess || hipMalloc(&d_first, sizeof *d_first) != hipSuccess)
    st = FTAR_ERR_NO_MEMORY;
  if (st == FTAR_SUCCESS &&
      (hipMemset(d_bad, 0, sizeof *d_bad) != hipSuccess || hipMemset(d_first, 0xff, sizeof *d_first) != hipSuccess))
    st = FTAR_ERR_HIP;
  if (st == FTAR_SUCCESS) {
    hipLaunchKernelGGL(ftar::bf16_cvt_check_kernel, dim3(8192), dim3(256), 0, nullptr, d_bad, d_first);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(mismatches, d_bad, sizeof *d_bad, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(first, d_first, sizeof *d_first, hipMemcpyDeviceToHost) != hipSuccess)
      st = FTAR_ERR_HIP;
  }
  ftar::hip_ignore(hipFree(d_bad));
  ftar::hip_ignore(hipFree(d_first));
  return st;
}

namespace ftar {
namespace {
// fp32 -> binary16 round-to-nearest-even in integer arithmetic: overflow to inf, gradual underflow, NaN
// to a quiet NaN of the same sign (which NaN is outside the contract: the check compares NaN-ness)
__host__ __device__ constexpr unsigned f16_rne_bits(unsigned u) {
  const unsigned sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7e00u;
  if (a >= 0x47800000u) return sign | 0x7c00u;  // |x| >= 65536 (or inf)
  if (a >= 0x38800000u) {                       // |x| >= 2^-14: a normal half, unless the rounding carries to inf
    const unsigned r = a - 0x38000000u;         // exponent rebias 127 -> 15
    return sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);  // a carry out of the mantissa bumps the exponent
  }
  const unsigned e = a >> 23, m = (a & 0x7fffffu) | 0x800000u;  // value = m x 2^(e - 150), half ulp = 2^-24
  const unsigned shift = 126u - e;                              // e <= 112: shift >= 14
  if (e == 0 || shift > 24u) return sign;  // below 2^-25 (fp32 subnormals included): rounds to zero
  const unsigned h = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  return sign | (h + ((rem > half || (rem == half && (h & 1u))) ? 1u : 0u));
}
// binary16 -> fp32 by integer expansion (exact)
__host__ __device__ constexpr unsigned f16_widen_bits(unsigned h) {
  const unsigned sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 31u) return sign | 0x7f800000u | (m << 13);
  if (e) return sign | ((e + 112u) << 23) | (m << 13);
  if (!m) return sign;
  int p = 9;  // the leading one of a subnormal: value = m x 2^-24 = 2^(p - 24) x (m / 2^p)
  while (!((m >> p) & 1u)) --p;
  return sign | ((unsigned)(p + 103) << 23) | ((m << (23 - p)) & 0x7fffffu);
}
static_assert(f16_rne_bits(0x3f800000u) == 0x3c00u && f16_rne_bits(0x477ff000u) == 0x7c00u &&
              f16_rne_bits(0x477fefffu) == 0x7bffu && f16_rne_bits(0x33000000u) == 0u &&
              f16_rne_bits(0x33000001u) == 1u && f16_rne_bits(0x33c00000u) == 2u && f16_rne_bits(0xb8800000u) == 0x8400u &&
              f16_rne_bits(0x387fffffu) == 0x0400u && f16_rne_bits(0x3f801000u) == 0x3c00u &&
              f16_rne_bits(0x3f803000u) == 0x3c02u);
static_assert(f16_widen_bits(0x3c00u) == 0x3f800000u && f16_widen_bits(1u) == 0x33800000u &&
              f16_widen_bits(0x83ffu) == 0xb87fc000u && f16_widen_bits(0xfc00u) == 0xff800000u);

__device__ __forceinline__ bool f16_bits_differ(unsigned got, unsigned want) {  // 16-bit patterns
  const bool ng = (got & 0x7fffu) > 0x7c00u, nw = (want & 0x7fffu) > 0x7c00u;
  return ng != nw || (!nw && got != want);
}
// every float bit pattern u (lo half) and u ^ 0x80000001 (hi half) through the production packing
// (pack_f16: the v_fin of the fp16 traits) and the scalar narrowing (their s_fin) against the integer RNE
__global__ void __launch_bounds__(256) f16_narrow_check_kernel(unsigned long long* bad, unsigned* first) {
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  unsigned long long mine = 0;
  unsigned first_mine = 0xffffffffu;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < (1ull << 32); i += stride) {
    const unsigned u = (unsigned)i, v = u ^ 0x80000001u;
    const unsigned got = pack_f16(__uint_as_float(u), __uint_as_float(v));
    const unsigned one = HalfFmt::narrow(__uint_as_float(u));
    if (f16_bits_differ(got & 0xffffu, f16_rne_bits(u)) || f16_bits_differ(got >> 16, f16_rne_bits(v)) ||
        f16_bits_differ(one, f16_rne_bits(u))) {
      ++mine;
      first_mine = first_mine < u ? first_mine : u;
    }
  }
  if (mine) {
    atomicAdd(bad, mine);
    atomicMin(first, first_mine);
  }
}
// every half bit pattern h (lo) and h ^ 0x8001 (hi) through the production widening (unpack_f16: the
// v_init of the fp16 traits; HalfFmt::widen: their s_init) against the integer expansion
__global__ void __launch_bounds__(256) f16_widen_check_kernel(unsigned long long* bad, unsigned* first) {
  const unsigned h = blockIdx.x * 256 + threadIdx.x, g = h ^ 0x8001u;
  if (h >= 0x10000u) return;
  const f32x2 w = unpack_f16(h | (g << 16));
  auto differ = [](float got, unsigned want) {
    const unsigned gb = __float_as_uint(got);
    const bool ng = (gb & 0x7fffffffu) > 0x7f800000u, nw = (want & 0x7fffffffu) > 0x7f800000u;
    return ng != nw || (!nw && gb != want);
  };
  if (differ(w.x, f16_widen_bits(h)) || differ(w.y, f16_widen_bits(g)) ||
      differ(HalfFmt::widen((unsigned short)h), f16_widen_bits(h))) {
    atomicAdd(bad, 1ull);
    atomicMin(first, h);
  }
}
}  // namespace
}  // namespace ftar

// Test hook (not in ftar.h), the sibling of ftar_debug_bf16_cvt_check: mismatches[0] = how many of the 2^32
// float bit patterns the production fp32 -> fp16 conversion (v_cvt_pk_f16_f32, and the scalar one of the
// element-wise paths) rounds differently from an integer round-to-nearest-even; mismatches[1] = how many of
// the 2^16 half bit patterns widen differently from an integer expansion; first[0..1] = the first such
// pattern of each direction (0xffffffff: none).  NaNs compare as NaN or not.
extern "C" ftar_status_t ftar_debug_f16_cvt_check(unsigned long long* mismatches, unsigned* first) {
  if (!mismatches || !first) return FTAR_ERR_INVALID_ARG;
  unsigned long long* d_bad = nullptr;
  unsigned* d_first = nullptr;
  ftar_status_t st = FTAR_SUCCESS;  // both buffers are freed on every path below
  if (hipMalloc(&d_bad, 2 * sizeof *d_bad) != hipSuccess || hipMalloc(&d_first, 2 * sizeof *d_first) != hipSuccess)
    st = FTAR_ERR_NO_MEMORY;
  if (st == FTAR_SUCCESS && (hipMemset(d_bad, 0, 2 * sizeof *d_bad) != hipSuccess ||
                             hipMemset(d_first, 0xff, 2 * sizeof *d_first) != hipSuccess))
    st = FTAR_ERR_HIP;
  if (st == FTAR_SUCCESS) {
    hipLaunchKernelGGL(ftar::f16_narrow_check_kernel, dim3(8192), dim3(256), 0, nullptr, d_bad, d_first);
    hipLaunchKernelGGL(ftar::f16_widen_check_kernel, dim3(256), dim3(256), 0, nullptr, d_bad + 1, d_first + 1);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(mismatches, d_bad, 2 * sizeof *d_bad, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(first, d_first, 2 * sizeof *d_first, hipMemcpyDeviceToHost) != hipSuccess)
      st = FTAR_ERR_HIP;
  }
  ftar::hip_ignore(hipFree(d_bad));
  ftar::hip_ignore(hipFree(d_first));
  return st;
}

namespace ftar {
namespace {
// fp32 -> OCP fp8 in integer arithmetic, the specification of the fp8 sums' rounding (ftar.h): RNE on the
// encoding with MB mantissa bits and exponent bias BIAS (e4m3: 3, 7; e5m2: 2, 15), the mantissa carry running
// into the next encoding, no saturation.  What lies above the largest finite encoding after rounding is the
// format's overflow: e5m2's inf (0x7c), e4m3's NaN (0x7f) -- for an fp32 inf too; a NaN gives 0x7f.
template <int MB, int BIAS>
__host__ __device__ constexpr unsigned f8_rne_bits(unsigned u) {
  const unsigned sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
  constexpr unsigned kOver = MB == 3 ? 0x7fu : 0x7cu;  // the encoding right above the largest finite one
  if (a > 0x7f800000u) return sign | 0x7fu;
  constexpr int sh = 23 - MB;                                     // mantissa bits dropped
  constexpr unsigned min_normal = (unsigned)(127 - BIAS + 1) << 23;  // 2^(1 - BIAS)
  if (a >= min_normal) {
    if (a >= 0x7f800000u) return sign | kOver;
    const unsigned r = a - ((unsigned)(127 - BIAS) << 23);       // exponent rebias
    const unsigned q = (r + ((1u << (sh - 1)) - 1u) + ((r >> sh) & 1u)) >> sh;  // a carry bumps the exponent
    return sign | (q >= kOver ? kOver : q);
  }
  const unsigned e = a >> 23, m = (a & 0x7fffffu) | 0x800000u;  // value = m x 2^(e - 150); one ulp = 2^(1 - BIAS - MB)
  const unsigned shift = (unsigned)(151 - BIAS - MB) - e;        // h = value / ulp = m >> shift
  if (e == 0 || shift > 25u) return sign;                        // below half the smallest subnormal: zero
  const unsigned h = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  return sign | (h + ((rem > half || (rem == half && (h & 1u))) ? 1u : 0u));
}
// OCP fp8 -> fp32 by integer expansion (exact); e5m2's all-ones exponent is inf / NaN, e4m3's only NaN is 0x7f
template <int MB, int BIAS>
__host__ __device__ constexpr unsigned f8_widen_bits(unsigned b) {
  const unsigned sign = (b & 0x80u) << 24, e = (b & 0x7fu) >> MB, m = b & ((1u << MB) - 1u);
  if (MB == 3 ? (b & 0x7fu) == 0x7fu : e == 31u) return sign | 0x7f800000u | (m << (23 - MB));
  if (e) return sign | ((e + 127u - BIAS) << 23) | (m << (23 - MB));
  if (!m) return sign;
  int p = MB - 1;  // the leading one of a subnormal: value = m x 2^(1 - BIAS - MB)
  while (!((m >> p) & 1u)) --p;
  return sign | ((unsigned)(p + 128 - BIAS - MB) << 23) | ((m << (23 - p)) & 0x7fffffu);
}
// 16 + 1 -> 16 and 18 + 1 -> 20 (ties to even), 448, 464 -> 448 (a tie: 448's mantissa is even), 464 + -> NaN,
// inf -> NaN, the smallest subnormal 2^-9 and half of it (a tie to zero), the carry from the subnormals into
// the normals
static_assert(f8_rne_bits<3, 7>(0x41880000u) == 0x58u && f8_rne_bits<3, 7>(0x41980000u) == 0x5au &&
              f8_rne_bits<3, 7>(0x43e00000u) == 0x7eu && f8_rne_bits<3, 7>(0x43e7ffffu) == 0x7eu &&
              f8_rne_bits<3, 7>(0x43e80000u) == 0x7eu && f8_rne_bits<3, 7>(0x43e80001u) == 0x7fu &&
              f8_rne_bits<3, 7>(0xff800000u) == 0xffu &&
              f8_rne_bits<3, 7>(0x3b000000u) == 0x01u && f8_rne_bits<3, 7>(0x3a800000u) == 0x00u &&
              f8_rne_bits<3, 7>(0x3a800001u) == 0x01u && f8_rne_bits<3, 7>(0x3c780000u) == 0x08u &&
              f8_rne_bits<3, 7>(0x3f800000u) == 0x38u);
// e5m2: 57344, 61440 - -> 57344, 61440 -> inf, inf -> inf, 1, the smallest subnormal 2^-16, half of it -> 0
static_assert(f8_rne_bits<2, 15>(0x47600000u) == 0x7bu && f8_rne_bits<2, 15>(0x476fffffu) == 0x7bu &&
              f8_rne_bits<2, 15>(0x47700000u) == 0x7cu && f8_rne_bits<2, 15>(0x7f800000u) == 0x7cu &&
              f8_rne_bits<2, 15>(0x3f800000u) == 0x3cu && f8_rne_bits<2, 15>(0x37800000u) == 0x01u &&
              f8_rne_bits<2, 15>(0x37000000u) == 0x00u && f8_rne_bits<2, 15>(0xb7000001u) == 0x81u);
static_assert(f8_widen_bits<3, 7>(0x38u) == 0x3f800000u && f8_widen_bits<3, 7>(0x01u) == 0x3b000000u &&
              f8_widen_bits<3, 7>(0x7eu) == 0x43e00000u && f8_widen_bits<3, 7>(0x87u) == 0xbc600000u &&
              f8_widen_bits<2, 15>(0x3cu) == 0x3f800000u && f8_widen_bits<2, 15>(0x01u) == 0x37800000u &&
              f8_widen_bits<2, 15>(0xfcu) == 0xff800000u && f8_widen_bits<2, 15>(0x7bu) == 0x47600000u);

template <bool E5M2>
__device__ __forceinline__ bool f8_is_nan(unsigned b) {
  return E5M2 ? (b & 0x7fu) > 0x7cu : (b & 0x7fu) == 0x7fu;
}
template <bool E5M2>
__device__ __forceinline__ bool f8_bits_differ(unsigned got, unsigned want) {  // 8-bit patterns
  const bool ng = f8_is_nan<E5M2>(got), nw = f8_is_nan<E5M2>(want);
  return ng != nw || (!nw && got != want);
}
// every float bit pattern u, in each of the four byte positions of the production packing (F8Fmt::pack: the
// v_fin of the fp8 traits; the other three positions hold u ^ 0x80000001 and two neighbours) and through the
// scalar narrowing (their s_fin), against the integer RNE
template <bool E5M2>
__global__ void __launch_bounds__(256) f8_narrow_check_kernel(unsigned long long* bad, unsigned* first) {
  using F = F8Fmt<E5M2>;
  constexpr int MB = E5M2 ? 2 : 3, BIAS = E5M2 ? 15 : 7;
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  unsigned long long mine = 0;
  unsigned first_mine = 0xffffffffu;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < (1ull << 32); i += stride) {
    const unsigned u = (unsigned)i, v[4] = {u, u ^ 0x80000001u, u + 1u, u ^ 0x00400000u};
    const unsigned got = F::pack(f32x4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                                       __uint_as_float(v[3])});
    bool differ = f8_bits_differ<E5M2>(F::narrow(__uint_as_float(u)), f8_rne_bits<MB, BIAS>(u));
#pragma unroll
    for (int j = 0; j < 4; ++j) differ |= f8_bits_differ<E5M2>((got >> (8 * j)) & 0xffu, f8_rne_bits<MB, BIAS>(v[j]));
    if (differ) {
      ++mine;
      first_mine = first_mine < u ? first_mine : u;
    }
  }
  if (mine) {
    atomicAdd(bad, mine);
    atomicMin(first, first_mine);
  }
}
// every byte b, in each of the four byte positions of the production widening (F8Fmt::unpack: the v_init of the
// fp8 traits) and through the scalar one (their s_init), against the integer expansion
template <bool E5M2>
__global__ void __launch_bounds__(256) f8_widen_check_kernel(unsigned long long* bad, unsigned* first) {
  using F = F8Fmt<E5M2>;
  constexpr int MB = E5M2 ? 2 : 3, BIAS = E5M2 ? 15 : 7;
  const unsigned b = threadIdx.x, v[4] = {b, b ^ 0x81u, (b + 1u) & 0xffu, b ^ 0x40u};
  const f32x4 w = F::unpack(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24));
  auto differ = [](float got, unsigned want) {
    const unsigned gb = __float_as_uint(got);
    const bool ng = (gb & 0x7fffffffu) > 0x7f800000u, nw = (want & 0x7fffffffu) > 0x7f800000u;
    return ng != nw || (!nw && gb != want);
  };
  if (differ(w.x, f8_widen_bits<MB, BIAS>(v[0])) || differ(w.y, f8_widen_bits<MB, BIAS>(v[1])) ||
      differ(w.z, f8_widen_bits<MB, BIAS>(v[2])) || differ(w.w, f8_widen_bits<MB, BIAS>(v[3])) ||
      differ(F::widen((unsigned char)b), f8_widen_bits<MB, BIAS>(b))) {
    atomicAdd(bad, 1ull);
    atomicMin(first, b);
  }
}
}  // namespace
}  // namespace ftar

// Test hook (not in ftar.h), the sibling of ftar_debug_f16_cvt_check for the two OCP fp8 formats.  mismatches[0]
// / [1] = how many of the 2^32 float bit patterns the production narrowing to e4m3 / e5m2 (v_cvt_pk_fp8_f32 /
// v_cvt_pk_bf8_f32 in every byte position, and the scalar form of the element-wise paths) converts differently
// from the integer RNE above; mismatches[2] / [3] = how many of the 2^8 bytes of e4m3 / e5m2 widen differently
// from the integer expansion; first[0..3] = the first such pattern of each (0xffffffff: none).  NaNs compare as
// NaN or not.
extern "C" ftar_status_t ftar_debug_f8_cvt_check(unsigned long long* mismatches, unsigned* first) {
  if (!mismatches || !first) return FTAR_ERR_INVALID_ARG;
  unsigned long long* d_bad = nullptr;
  unsigned* d_first = nullptr;
  ftar_status_t st = FTAR_SUCCESS;  // both buffers are freed on every path below
  if (hipMalloc(&d_bad, 4 * sizeof *d_bad) != hipSuccess || hipMalloc(&d_first, 4 * sizeof *d_first) != hipSuccess)
    st = FTAR_ERR_NO_MEMORY;
  if (st == FTAR_SUCCESS && (hipMemset(d_bad, 0, 4 * sizeof *d_bad) != hipSuccess ||
                             hipMemset(d_first, 0xff, 4 * sizeof *d_first) != hipSuccess))
    st = FTAR_ERR_HIP;
  if (st == FTAR_SUCCESS) {
    hipLaunchKernelGGL(ftar::f8_narrow_check_kernel<false>, dim3(8192), dim3(256), 0, nullptr, d_bad, d_first);
    hipLaunchKernelGGL(ftar::f8_narrow_check_kernel<true>, dim3(8192), dim3(256), 0, nullptr, d_bad + 1, d_first + 1);
    hipLaunchKernelGGL(ftar::f8_widen_check_kernel<false>, dim3(1), dim3(256), 0, nullptr, d_bad + 2, d_first + 2);
    hipLaunchKernelGGL(ftar::f8_widen_check_kernel<true>, dim3(1), dim3(256), 0, nullptr, d_bad + 3, d_first + 3);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(mismatches, d_bad, 4 * sizeof *d_bad, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(first, d_first, 4 * sizeof *d_first, hipMemcpyDeviceToHost) != hipSuccess)
      st = FTAR_ERR_HIP;
  }
  ftar::hip_ignore(hipFree(d_bad));
  ftar::hip_ignore(hipFree(d_first));
  return st;
}

// ---------------------------------------------------------------------------
// Rehearsal hook of bench.py: a stream that really never drains while the RCCL preflight is
// waited for.  One wave spins on a host flag (a system-scope atomic load, vector memory) until the host
// releases it or `seconds` pass -- every wave reaches that exit, so the stream always drains in the end.
// ---------------------------------------------------------------------------
namespace {
__global__ void block_stream_kernel(int* flag, unsigned long long limit_ticks) {
  const unsigned long long t0 = wall_clock64();
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0 &&
         wall_clock64() - t0 < limit_ticks)
    __builtin_amdgcn_s_sleep(8);
}
}  // namespace

// Enqueues the spinning wave on `stream`; returns the host flag to release (ftar_debug_unblock), or NULL.
extern "C" void* ftar_debug_block_stream(void* stream, double seconds) {
  int* flag = nullptr;
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&flag), sizeof(int), hipHostMallocCoherent | hipHostMallocMapped) !=
          hipSuccess)
    return nullptr;
  __atomic_store_n(flag, 0, __ATOMIC_SEQ_CST);
  const unsigned long long ticks = (unsigned long long)(seconds * 1e3 * khz);
  hipLaunchKernelGGL(block_stream_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), flag, ticks);
  if (hipGetLastError() != hipSuccess) return nullptr;
  return flag;
}

// Releases a stream blocked by ftar_debug_block_stream (the 4-byte flag stays allocated).
extern "C" void ftar_debug_unblock(void* flag) {
  if (flag) __atomic_store_n(static_cast<int*>(flag), 1, __ATOMIC_SEQ_CST);
}

// The layout candidates of the scaled cast (cast_impl.h; tools/cast_rates.py): layout 0 = each lane owns one fp8
// vector and its wide bytes, 1 = the same with the wide side transposed through LDS, 2 = lane-contiguous wide
// vectors with 4- / 8-byte fp8 accesses; u = fp8 vectors per lane and pass (1, 2 or 4).  No amax, no memset.
extern "C" ftar_status_t ftar_debug_cast_variant(int layout, int u, const void* src, int src_dtype, void* dst,
                                                 int dst_dtype, size_t count, const float* scale, void* stream) {
  using namespace ftar;
  if (!cast_pair_supported((ftar_dtype_t)src_dtype, (ftar_dtype_t)dst_dtype)) return FTAR_ERR_UNSUPPORTED;
  if (!src || !dst || !count) return FTAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipErrorInvalidValue;
#define FTAR_CAST_VARIANT(L, U_)                                                                                  \
  if (layout == (L) && u == (U_))                                                                                 \
    e = launch_cast_any<U_, U_, L>(src, (ftar_dtype_t)src_dtype, dst, (ftar_dtype_t)dst_dtype, count, scale, nullptr, s);
  FTAR_CAST_VARIANT(kLayOwn, 1)
  FTAR_CAST_VARIANT(kLayOwn, 2)
  FTAR_CAST_VARIANT(kLayLds, 1)
  FTAR_CAST_VARIANT(kLayLds, 2)
  FTAR_CAST_VARIANT(kLayWide, 1)
  FTAR_CAST_VARIANT(kLayWide, 2)
  FTAR_CAST_VARIANT(kLayWide, 4)
#undef FTAR_CAST_VARIANT
  if (e == hipErrorInvalidValue) return FTAR_ERR_INVALID_ARG;
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}

// ---------------------------------------------------------------------------
// Stochastic rounding (ftar_cast_scaled_sr): the hooks of tools/sr_sweep.py and tests/test_gpu_cast_sr.py.
// ---------------------------------------------------------------------------
// The production stochastic cast (same kernels, layout and narrowing device function) on an explicit array of
// words, words[i] for element i, in place of the generator.  Quantize pairs only; no amax.
extern "C" ftar_status_t ftar_bench_cast_sr_words(const void* src, int src_dtype, void* dst, int dst_dtype,
                                                  size_t count, const float* scale, const unsigned* words,
                                                  void* stream) {
  using namespace ftar;
  if (!is_cast_wide((ftar_dtype_t)src_dtype) || !is_f8((ftar_dtype_t)dst_dtype)) return FTAR_ERR_UNSUPPORTED;
  if (!src || !dst || !words || !count) return FTAR_ERR_INVALID_ARG;
  FTAR_CHECK_HIP((launch_cast_any<kCastU16, kCastU32, kCastLayout, SrWords>(
      src, (ftar_dtype_t)src_dtype, dst, (ftar_dtype_t)dst_dtype, count, scale, nullptr,
      static_cast<hipStream_t>(stream), SrWords::Arg{words, count})));
  return FTAR_SUCCESS;
}

// The production stochastic MX quantize (mx_impl.h: same kernels, family choice and grids) on an explicit array of
// words, words[i] for element i of the call, in place of the generator: tests/test_gpu_mx_sr.py.  mode: ftar_mx_mode_t.
extern "C" ftar_status_t ftar_bench_mx_quantize_sr_words(const void* src, int src_dtype, void* dst, int dst_dtype,
                                                         size_t count, int mode, int headroom, unsigned char* scales,
                                                         const unsigned* words, void* stream) {
  using namespace ftar;
  if (!is_cast_wide((ftar_dtype_t)src_dtype) || !is_f8((ftar_dtype_t)dst_dtype)) return FTAR_ERR_UNSUPPORTED;
  if (mode != FTAR_MX_COMPUTE && mode != FTAR_MX_GIVEN) return FTAR_ERR_INVALID_ARG;
  if (headroom < 0 || headroom > 31 || (mode == FTAR_MX_GIVEN && headroom != 0)) return FTAR_ERR_INVALID_ARG;
  if (!src || !dst || !scales || !words || !count) return FTAR_ERR_INVALID_ARG;
  const SrWords::Arg rnd{words, count};
  hipStream_t s = static_cast<hipStream_t>(stream);
  FTAR_CHECK_HIP(mx_with_pair((ftar_dtype_t)src_dtype, (ftar_dtype_t)dst_dtype, [&](auto w, auto f) {
    using W = decltype(w);
    using F = decltype(f);
    return mode == FTAR_MX_GIVEN
               ? launch_mx_quant_pair<W, F, kMxGiven, SrWords>(src, dst, scales, count, headroom, s, rnd)
               : launch_mx_quant_pair<W, F, kMxCompute, SrWords>(src, dst, scales, count, headroom, s, rnd);
  }));
  return FTAR_SUCCESS;
}

namespace ftar {
namespace {
// The contract of ftar.h's stochastic-rounding paragraph in integers, step by step as written there (e, ulp, lo,
// F, the carry): what SrFmt (the instruction, and float arithmetic below the smallest normal) is held against.
// *f_out: F.
template <bool E5M2>
__device__ unsigned sr_contract(unsigned bits, unsigned u, unsigned* f_out) {
  constexpr int M = E5M2 ? 2 : 3, BIAS = E5M2 ? 15 : 7, EMIN = 1 - BIAS;
  const unsigned a = bits & 0x7fffffffu, sign = (bits >> 24) & 0x80u;
  *f_out = 0;
  if (a > 0x7f800000u) return sign | 0x7fu;
  if (a == 0x7f800000u) return sign | (E5M2 ? 0x7cu : 0x7fu);
  if (a == 0) return sign;
  const int ee = (a >> 23) ? (int)(a >> 23) : 1;
  const unsigned long long sig = (a & 0x7fffffu) | ((a >> 23) ? 0x800000u : 0u);   // a = sig * 2^(ee - 150)
  const int e = ee - 127, q = (e > EMIN ? e : EMIN) - M;                            // ulp = 2^q
  const int k = q - (ee - 150);                                                     // a / ulp = sig / 2^k, k >= 20
  const unsigned long long lo = k < 64 ? sig >> k : 0, rem = k < 64 ? sig & ((1ull << k) - 1) : sig;
  unsigned long long F;
  if (k <= 32) F = rem << (32 - k);
  else F = (k - 32) < 64 ? rem >> (k - 32) : 0;
  *f_out = (unsigned)F;
  const unsigned long long units = lo + (((unsigned long long)u + F) >> 32);
  unsigned enc;
  if (e < EMIN) enc = (unsigned)units;                                               // subnormal range
  else enc = ((unsigned)(e + BIAS) << M) + (unsigned)(units - (1u << M));
  constexpr unsigned TOP = E5M2 ? 0x7cu : 0x7fu;
  return sign | (enc < TOP ? enc : TOP);
}
constexpr int kSweepModes = 3, kSweepWords = 6;
// modes: 0 the production narrowing (SrFmt::pack in every byte position and SrFmt::narrow), 1 the bare
// instruction fed U, 2 the bare instruction fed U >> (32 - d), d = 23 - m.  words: 0, 1, 2^31, 2^32 - 1, the
// input's threshold 2^32 - F and 2^32 - F - 1.  bad[mode][word][fp32 exponent field], ex[mode][exponent][4] =
// {input bits, word, got, want} of one mismatch (ex[..][0] == 0xffffffff: none yet).
template <bool E5M2>
__global__ void __launch_bounds__(256) sr_sweep_kernel(unsigned long long first, unsigned long long count,
                                                       unsigned long long* bad, unsigned* ex) {
  using F = SrFmt<E5M2>;
  constexpr int SH = 32 - F::kDrop;
  __shared__ unsigned bins[kSweepModes * kSweepWords * 256];
  for (int j = threadIdx.x; j < kSweepModes * kSweepWords * 256; j += 256) bins[j] = 0;
  __syncthreads();
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
    const unsigned b = (unsigned)(first + i), ebin = (b >> 23) & 0xffu;
    const float p = __uint_as_float(b);
    unsigned f;
    sr_contract<E5M2>(b, 0u, &f);
    const unsigned w[kSweepWords] = {0u, 1u, 0x80000000u, 0xffffffffu, 0u - f, 0u - f - 1u};
    const unsigned pk0 = F::pack(f32x4{p, p, p, p}, u32x4{w[0], w[1], w[2], w[3]});
    const unsigned pk1 = F::pack(f32x4{p, p, p, p}, u32x4{w[4], w[5], w[0], w[1]});
#pragma unroll
    for (int j = 0; j < kSweepWords; ++j) {
      unsigned dummy;
      const unsigned want = sr_contract<E5M2>(b, w[j], &dummy);
      unsigned got[kSweepModes];
      got[0] = j < 4 ? (pk0 >> (8 * j)) & 0xffu : (pk1 >> (8 * (j - 4))) & 0xffu;
      if (f8_bits_differ<E5M2>(F::narrow(p, w[j]), want)) got[0] = 0x100u | F::narrow(p, w[j]);
      if (j < 2 && f8_bits_differ<E5M2>((pk1 >> (8 * (j + 2))) & 0xffu, want)) got[0] = 0x200u | ((pk1 >> (8 * (j + 2))) & 0xffu);
      if constexpr (E5M2) {
        got[1] = __builtin_amdgcn_cvt_sr_bf8_f32(p, w[j], 0u, 0) & 0xffu;
        got[2] = __builtin_amdgcn_cvt_sr_bf8_f32(p, w[j] >> SH, 0u, 0) & 0xffu;
      } else {
        got[1] = __builtin_amdgcn_cvt_sr_fp8_f32(p, w[j], 0u, 0) & 0xffu;
        got[2] = __builtin_amdgcn_cvt_sr_fp8_f32(p, w[j] >> SH, 0u, 0) & 0xffu;
      }
#pragma unroll
      for (int m = 0; m < kSweepModes; ++m) {
        if (got[m] > 0xffu || f8_bits_differ<E5M2>(got[m], want)) {
          atomicAdd(&bins[(m * kSweepWords + j) * 256 + ebin], 1u);
          unsigned* slot = ex + (m * 256 + ebin) * 4;
          if (atomicCAS(slot, 0xffffffffu, b) == 0xffffffffu) {
            slot[1] = w[j];
            slot[2] = got[m];
            slot[3] = want;
          }
        }
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kSweepModes * kSweepWords * 256; j += 256)
    if (bins[j]) atomicAdd(bad + j, (unsigned long long)bins[j]);
}
}  // namespace
}  // namespace ftar

// tools/sr_sweep.py's hook: the fp32 bit patterns [first, first + count) through the stochastic narrowing to e4m3
// (e5m2 != 0: e5m2) in the three modes and six words of sr_sweep_kernel, against the contract in integers.
// mismatches: 3 x 6 x 256 counts, added to; examples: 3 x 256 x 4 words, 0xffffffff where none was seen (both host
// arrays the caller initialises).  NaNs compare as NaN or not.  An input whose stored pattern 0xffffffff would be
// taken for "none" is a NaN, whose exponent bin 255 then only shows in the counts.
extern "C" ftar_status_t ftar_bench_sr_sweep(int e5m2, unsigned long long first, unsigned long long count,
                                             unsigned long long* mismatches, unsigned* examples) {
  using namespace ftar;
  if (!mismatches || !examples || first + count > (1ull << 32)) return FTAR_ERR_INVALID_ARG;
  constexpr size_t NB = (size_t)kSweepModes * kSweepWords * 256 * sizeof(unsigned long long);
  constexpr size_t NE = (size_t)kSweepModes * 256 * 4 * sizeof(unsigned);
  unsigned long long* d_bad = nullptr;
  unsigned* d_ex = nullptr;
  ftar_status_t st = FTAR_SUCCESS;
  if (hipMalloc(&d_bad, NB) != hipSuccess || hipMalloc(&d_ex, NE) != hipSuccess) st = FTAR_ERR_NO_MEMORY;
  if (st == FTAR_SUCCESS && (hipMemcpy(d_bad, mismatches, NB, hipMemcpyHostToDevice) != hipSuccess ||
                             hipMemcpy(d_ex, examples, NE, hipMemcpyHostToDevice) != hipSuccess))
    st = FTAR_ERR_HIP;
  if (st == FTAR_SUCCESS && count) {
    if (e5m2) hipLaunchKernelGGL(sr_sweep_kernel<true>, dim3(4096), dim3(256), 0, nullptr, first, count, d_bad, d_ex);
    else hipLaunchKernelGGL(sr_sweep_kernel<false>, dim3(4096), dim3(256), 0, nullptr, first, count, d_bad, d_ex);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) st = FTAR_ERR_HIP;
  }
  if (st == FTAR_SUCCESS && (hipMemcpy(mismatches, d_bad, NB, hipMemcpyDeviceToHost) != hipSuccess ||
                             hipMemcpy(examples, d_ex, NE, hipMemcpyDeviceToHost) != hipSuccess))
    st = FTAR_ERR_HIP;
  hip_ignore(hipFree(d_bad));
  hip_ignore(hipFree(d_ex));
  return st;
}
