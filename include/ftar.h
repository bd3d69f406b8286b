/*
 * ftar.h — C ABI of the MI355X-native FlexTree AllReduce (libftar.so).
 *
 * Plain pointers, sizes and enums only: no torch, no C++ types.  Every entry
 * point returns an ftar_status_t instead of exit()ing like the reference.
 * Device buffers are HBM pointers on the communicator's device; streams are
 * hipStream_t passed as void* so this header needs no HIP include.
 *
 * What each entry point replaces in the reference (DictXiong/AllReduce-Over-MPI):
 *
 *   ftar_reduce            FlexTree::reduce_sum<T> / reduce_band<T>
 *                            allreduce_over_mpi/mpi_mod.hpp:812-1031, :1034-1251
 *                          reduce_sum_gpu<T> + reduce_sum_1..20 kernels
 *                            vector_add/reduce_sum_gpu.h:4-316
 *   ftar_topo_parse        FlexTree::get_stages (FT_TOPO / FT_LONELY)
 *                            allreduce_over_mpi/mpi_mod.hpp:1419-1486
 *   ftar_topo_choose       cost_model getWidth + CostModel (argmin width list)
 *                            cost_model/GetWidth.h:42-47, cost_model/CostModel.h:82-120
 *   ftar_comm_init_rank    the MPI communicator the reference runs on (MPI_Comm_size/
 *                            rank, mpi_mod.hpp:781-809); transport = RCCL p2p
 *   ftar_allreduce         MPI_Allreduce_FT / static MPI_Allreduce
 *                            allreduce_over_mpi/mpi_mod.hpp:1723-1778
 *                          (ring_allreduce :1673-1719, tree_allreduce :1510-1671)
 *   ftar_schedule_json     Send/Recv_Operations + FMA_Send/Recv_Operations
 *                            allreduce_over_mpi/mpi_mod.hpp:258-766 (introspection)
 *
 * Results are bit-identical to the reference's CPU path for the same inputs
 * and FT_TOPO/FT_LONELY (same association order), see DESIGN.md §Parity.
 */
#ifndef FTAR_H
#define FTAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTAR_VERSION_MAJOR 0
#define FTAR_VERSION_MINOR 1
#define FTAR_MAX_STAGES 16
#define FTAR_MAX_K 64 /* max sources of one reduce (reference: 20, mpi_mod.hpp:811) */

typedef enum {
  FTAR_UINT8 = 0,   /* MPI_UINT8_T */
  FTAR_INT8 = 1,    /* MPI_INT8_T */
  FTAR_UINT16 = 2,  /* MPI_UINT16_T */
  FTAR_INT16 = 3,   /* MPI_INT16_T */
  FTAR_INT32 = 4,   /* MPI_INT32_T */
  FTAR_INT64 = 5,   /* MPI_INT64_T, MPI_LONG_LONG(_INT) */
  FTAR_FLOAT32 = 6, /* MPI_FLOAT */
  FTAR_FLOAT64 = 7, /* MPI_DOUBLE */
  FTAR_BOOL = 8,    /* MPI_C_BOOL: sum of bools == logical OR */
  FTAR_BFLOAT16 = 9, /* extension: fp32 accumulate, one RNE rounding per reduce */
  FTAR_FLOAT16 = 10, /* extension: IEEE binary16, bf16's rules (see below) */
  /* 11 is unassigned and stays invalid: ftar_dtype_size(11) == 0 and every entry point refuses it */
  FTAR_FLOAT8_E4M3 = 12, /* extension: OCP e4m3fn (bias 7, no inf, NaN = 0x7f / 0xff, max 448), see below */
  FTAR_FLOAT8_E5M2 = 13  /* extension: OCP e5m2 (bias 15, IEEE-like, max 57344), see below */
} ftar_dtype_t;

typedef enum {
  FTAR_SUM = 0,  /* MPI_SUM */
  FTAR_BAND = 1, /* MPI_BAND (integer types only, as in the reference) */
  FTAR_MAX = 2,  /* extension: every dtype but FTAR_BOOL (see below) */
  FTAR_MIN = 3,  /* extension: every dtype but FTAR_BOOL */
  FTAR_AVG = 4   /* extension: the mean, f32 f64 bf16 f16 f8e4m3 f8e5m2, the AllReduce entry points only (see below) */
} ftar_op_t;

/* Which (dtype, op) pairs run; the rest return FTAR_ERR_UNSUPPORTED before any device work.
 *
 *                  SUM   BAND   MAX   MIN   AVG
 *   u8 i8 u16 i16   x     x      x     x     -
 *   i32 i64         x     x      x     x     -
 *   f32 f64         x     -      x     x     x     (AVG: ftar_allreduce, _group, _host, _host_group;
 *   bf16 f16        x     -      x     x     x      ftar_reduce / ftar_reduce_nested refuse it)
 *   f8e4m3 f8e5m2   x     -      x     x     x
 *   bool            x(OR) -      -     -     -     (MPI defines no MAX/MIN on logical types either)
 *
 *   amax (ftar_reduce_amax, ftar_allreduce_amax, _amax_group): SUM and AVG of f32 bf16 f16 f8e4m3 f8e5m2;
 *   every other dtype (f64 included: its amax does not fit the word) and every other op is refused.
 *   cast (ftar_cast_scaled): f32 bf16 f16 -> f8e4m3 f8e5m2 and back, times a device scale; every other pair is refused.
 *   stochastic cast (ftar_cast_scaled_sr): f32 bf16 f16 -> f8e4m3 f8e5m2 only; the way back and every other pair is refused.
 *   MX casts (ftar_mx_scales, ftar_mx_quantize: f32 bf16 f16 -> f8e4m3 f8e5m2; ftar_mx_dequantize: the way back); every other pair is refused.
 *   stochastic MX quantize (ftar_mx_quantize_sr): f32 bf16 f16 -> f8e4m3 f8e5m2, both modes; every other pair is refused.
 *
 * The 16-bit floats (no reference; bf16 and IEEE binary16 follow the same rules): a SUM accumulates in fp32,
 * left to right, and rounds once to nearest even per reduce call -- once for a flat fold, once per hop on the
 * ring, once per node of a multi-stage tree.  For binary16 that rounding overflows to +-inf, keeps results
 * in the subnormal range (gradual underflow), and reads subnormal inputs exactly.  A lane is NaN exactly
 * where that fold has a NaN; which NaN is not specified.
 *
 * The two OCP fp8 formats (FTAR_FLOAT8_E4M3 = torch.float8_e4m3fn, FTAR_FLOAT8_E5M2 = torch.float8_e5m2; not
 * MI300X's fnuz encodings) follow the same rules with the same rounding points: a SUM accumulates in fp32,
 * left to right, and rounds once to nearest even per reduce call -- once for a flat fold, once per hop on the
 * ring, once per node of a multi-stage tree and of ftar_reduce_nested.  Widening is exact, subnormal inputs are
 * read exactly and results in the subnormal range are kept.  The rounding is torch's float32 -> float8 cast:
 * RNE on the encoding, the mantissa carry running into the next encoding, and no saturation.  e5m2 overflows
 * to +-inf at |A| >= 61440 (a tie that goes to the even encoding, inf's).  e4m3 has no inf encoding, so its
 * overflow rounds to NaN: |A| <= 464 rounds to at most 448 (464 is a tie and 448's mantissa is even), anything
 * above (an inf included) gives NaN.  That is deliberate: an overflow stays visible to the
 * caller, as fp16's inf does, where a saturated 448 would be silent.  So a lane is NaN where its fold has a
 * NaN, an inf - inf, or (e4m3 only) a rounding that overflows; which NaN pattern comes out is unspecified.
 * RCCL's fp8 conversion may saturate instead, so ftar_rccl_allreduce (the yardstick) can differ there.
 *
 * MAX / MIN: integers compare by the dtype's signedness (the first place u8/i8 and u16/i16 differ; SUM and
 * BAND treat them alike).  Floats follow IEEE 754-2019 maximum / minimum: -0 < +0, subnormals are not
 * flushed, a non-NaN result is bit for bit one of the sources, and any NaN source makes the lane NaN
 * (payload unspecified); the fp8 formats alike (e5m2's infs are ordinary values, e4m3 has none).  Both are
 * exact, associative and commutative, so every topology, form, piece size and buffer kind gives the same
 * bits, and a nested shape (ftar_reduce_nested) has no effect on them.
 *
 * AVG (ncclAvg, torch's ReduceOp.AVG) is SUM's schedule, unchanged, except at the root fold of each block:
 * the one reduce that produces the block's final value on the rank that owns it after the reduce-scatter.
 * That fold finishes as out = round_to_dtype(A x r): A is its accumulator before its rounding (fp32 for
 * bf16 / f16 / fp8, the dtype itself for f32 / f64) and r = 1.0f / (float)P (f64: 1.0 / (double)P) -- one
 * multiply by the reciprocal (as NCCL and torch's scalar division on the GPU do; not a division), correctly
 * rounded in the accumulator's precision, subnormal products kept; for the 16-bit and 8-bit floats the root's
 * single round to nearest even follows.  Inner nodes and earlier hops round exactly as under SUM; P = 1 is SUM's
 * copy; a lane with a NaN or an inf - inf stays NaN (payload unspecified).  For one topology every form
 * (stages, direct, collective all-gather, peer read, peer write), piece size and buffer kind gives the same
 * bits.  In the one-round forms a 16-bit or 8-bit mean is therefore summed in fp32, scaled and rounded once: an
 * fp16 mean stays finite where the fp16 sum is inf, an e4m3 mean where the e4m3 sum is NaN.  The staged forms
 * round partial sums between hops, where a partial sum can still overflow.  Integers and bool return FTAR_ERR_UNSUPPORTED before any device work.
 * A one-device reduce has no P: ftar_reduce and ftar_reduce_nested refuse FTAR_AVG (FTAR_ERR_UNSUPPORTED,
 * before touching a pointer); the one-device surface is ftar_reduce_scaled.
 *
 * amax (the *_amax entry points): the result's abs-max, taken in the root fold of each block, where the final
 * values sit in registers just before they are stored -- no extra pass over the bucket.  `amax` is one float
 * in device memory on the communicator's device (ftar_reduce_amax: the current device), 4-byte aligned, written
 * on the call's stream.  After the call it holds, on every rank, the IEEE 754-2019 maximum of |recvbuf[i]| over
 * all `count` elements AS STORED: after the fold's one rounding, and after the 1/P multiply under AVG, widened
 * exactly to fp32.  Any NaN element makes it a NaN (which NaN is unspecified); an inf element makes it +inf;
 * subnormals are not flushed; all zeros (-0 included) or count == 0 give +0.0 (bits 0x00000000).  The word is
 * overwritten, not accumulated into.  Non-NaN results are bit-identical on every rank, and for one topology
 * across every form, piece size and buffer layout, because the result is.  SUM and AVG of f32, bf16, f16,
 * f8e4m3 and f8e5m2; any other dtype (f64 included: its amax does not fit the word) or op returns
 * FTAR_ERR_UNSUPPORTED, a NULL or misaligned amax FTAR_ERR_INVALID_ARG, and ftar_allreduce_amax / _amax_group
 * under stream capture FTAR_ERR_UNSUPPORTED with a message (ftar_reduce_amax captures): every refusal comes
 * before any device work and leaves recvbuf and *amax untouched.  The host-buffer entry points
 * (ftar_allreduce_host, _host_group) and the MPI drop-in have no amax variant.
 *
 * Scaled casts (ftar_cast_scaled): the two ends of an fp8 wire.  src in {f32, bf16, f16} to dst in {f8e4m3,
 * f8e5m2} (quantize) and the reverse (dequantize), 12 pairs; every other pair (the same dtype twice, f32 <-> f16,
 * f64, integers, bool, the unassigned id 11) returns FTAR_ERR_UNSUPPORTED, and that check comes first.  Per
 * element dst[i] = cvt_dst(widen(src[i]) x r): the widening to fp32 is exact; r is the float at `scale`, read by
 * the kernel from device memory on the stream (NULL: 1.0f, an exact multiply) and never by the host, so it may be
 * any bit pattern (0, negative, inf, NaN, subnormal) and the result is what IEEE multiplication gives; the product
 * is one correctly rounded fp32 multiply, subnormal products kept; cvt_dst is the rounding of the paragraphs above
 * for that format (f32: the product itself).  That is (src.to(float32) * r).to(dst_dtype) of torch bit for bit:
 * TWO roundings when dst is narrower than fp32, never one fused one, and no saturation -- e4m3 overflow gives
 * NaN, e5m2 and f16 overflow +-inf.  amax (optional) is the amax paragraph's word for dst: the IEEE 754-2019
 * maximum of |dst[i]| as stored, widened exactly to fp32 -- NaN wins, inf is +inf, subnormals kept, all zeros or
 * count == 0 give bits 0, the word is overwritten.  NULL src or dst with count > 0, or a scale or amax that is not
 * 4-byte aligned, returns FTAR_ERR_INVALID_ARG; every refusal comes before any device work and leaves dst and
 * *amax untouched.  src and dst must not overlap.
 *
 * Stochastic rounding (ftar_cast_scaled_sr): the six quantize pairs of the scaled cast with another narrowing,
 * dst[i] = sr_dst(mul_rn_f32(widen(src[i]), r), U(seed, offset + i)).  Widening, r and the multiply are exactly
 * ftar_cast_scaled's (exact; NULL scale is 1.0f; one correctly rounded fp32 multiply in a register of its own).
 * sr_dst(p, U), U a 32-bit word: a NaN p gives NaN (which pattern is unspecified); +-0 gives +-0, and the sign is
 * kept also when a non-zero p rounds down to zero; +-inf gives e5m2 +-inf and e4m3 NaN.  Otherwise, with a = |p|,
 * m = 3 (e4m3) or 2 (e5m2), emin = -6 or -14, e = floor(log2 a), ulp = 2^(max(e, emin) - m),
 * lo = floor(a / ulp) x ulp, frac = (a - lo) / ulp in [0, 1) and F = floor(frac x 2^32), the magnitude stored is
 * lo + ulp if U + F >= 2^32, else lo.  In integers: the dropped mantissa bits are aligned under the TOP of U and
 * the carry decides -- with d = 23 - m dropped bits in the normal range, ((bits & (2^d - 1)) << (32 - d)) + U >= 2^32;
 * in the subnormal range d grows and bits below 2^-32 ulp are dropped.  So a representable p is stored unchanged
 * for every U, U = 0 truncates toward zero, and the stored value's expectation over a uniform U is p (to 2^-32 ulp).
 * No saturation: the carry runs into the next encoding -- an e4m3 magnitude in (448, 480) becomes NaN with
 * probability frac and from 480 on always; an e5m2 magnitude in (57344, 65536) becomes +-inf with probability
 * frac and from 65536 on always -- so an overflow stays visible to amax.
 * The word is a pure function of two inputs: the 64-bit value s at `seed` (device memory, 8-byte aligned, read by
 * the kernel on the stream, never by the host) and the global element index g = offset + i (mod 2^64).  It does
 * not depend on pointer alignment, on the kernel or layout that ran, on the grid, or on how a range was split
 * into calls: casting [0, n) in one call stores the bits of casting [0, a) and [a, n) with offset = a.  Exactly,
 * in unsigned arithmetic of the stated widths:
 *   z = s + 0x9E3779B97F4A7C15            (64-bit; then the splitmix64 finaliser)
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
 *   ka = low 32 bits of z, kb = high 32 bits of z;  gl = low 32 bits of g, gh = high 32 bits of g
 *   x = gl ^ ka                           (32-bit from here)
 *   x = (x ^ (x >> 16)) * 0x7feb352d
 *   x = x + (kb ^ (gh * 0x9E3779B9))
 *   x = (x ^ (x >> 15)) * 0x846ca68b
 *   U = x ^ (x >> 16)
 * Both keys change with every bit of s, and kb enters between the two rounds, so the streams of two seeds (s and
 * s + 1 included) are neither shifts nor index permutations of each other.  amax is ftar_cast_scaled's.  A
 * dequantize pair, or any pair ftar_cast_scaled refuses, returns FTAR_ERR_UNSUPPORTED, and that check comes first;
 * a NULL seed, a seed not 8-byte aligned, a scale or amax not 4-byte aligned, or a NULL src or dst with
 * count > 0 returns FTAR_ERR_INVALID_ARG; every refusal comes before any device work and leaves dst and *amax
 * untouched.  count == 0 succeeds, and a non-NULL amax then holds +0.0.
 *
 * MX block-scaled casts (ftar_mx_scales, ftar_mx_quantize, ftar_mx_dequantize): an fp8 wire with one power-of-two
 * scale byte (OCP E8M0) per block of FTAR_MX_BLOCK = 32 elements.  Block b of a call covers the call's indices
 * [32b, min(32b + 32, count)), counted from element 0 of that call; the last block may be partial;
 * nblocks = ceil(count / 32).  A scale byte s means 2^(s - 127) for s in 0..254; s = 255 is NaN.  Wide dtypes are
 * f32, bf16 and f16, fp8 dtypes f8e4m3 (emax = 8) and f8e5m2 (emax = 15): the 6 + 6 pairs of ftar_cast_scaled,
 * every other pair refused as there (FTAR_ERR_UNSUPPORTED, that check first).  All in integers:
 *   The block's scale (the "fit" rule).  a = the unsigned maximum over the block's own elements of
 *   bits(widen(src[i])) & 0x7fffffff, the widening exact.  If a >= 0x7f800000 (an inf or a NaN in the block)
 *   s = 255; otherwise
 *     s = min(254, max(0, (a >> 23) - emax + (((a & 0x7fffff) > 0x600000) ? 1 : 0)) + headroom).
 *   Both formats' largest finite value is 1.75 x 2^emax (448, 57344), so s is the smallest exponent at which the
 *   block's largest magnitude times 2^(127 - s) is at most that value: the block's scaled peak lies in
 *   (0.875 x 2^emax, 1.75 x 2^emax] x 2^-headroom unless s was clamped at 0 (stored, it may round down onto the
 *   interval's lower end, which fp8 holds exactly), and no stored element of a finite
 *   block is NaN or inf -- which matters because these casts do not saturate.  An all-zero block (-0 included)
 *   gives s = headroom.  headroom (0..31) leaves that many binades free above the block's peak: the staged
 *   AllReduce forms round partial sums to fp8 between hops and need it.  This is the ROUND-UP variant of the MX
 *   scale: it differs from OCP's floor rule (s = floor(log2 peak) - emax) exactly in the blocks whose peak
 *   mantissa exceeds 1.75, where OCP saturates the top eighth of the binade and this rule takes the next scale.
 *   Quantize.  dst[i] = cvt_fp8(mul_rn_f32(widen(src[i]), q(s))), s the scale byte of i's block;
 *   q(s) = 2^(127 - s): bits (254 - s) << 23 for s <= 253, 0x00400000 for s = 254; q(255) = 1.0f, so the payload of
 *   a NaN block is the plain cast and the block is NaN through its scale.  The multiply and the narrowing are
 *   ftar_cast_scaled's (subnormal products kept, RNE, no saturation): every block equals ftar_cast_scaled on that
 *   block with r = q(s).  With given scales an element may exceed the format and becomes NaN (e4m3) / +-inf (e5m2).
 *   Dequantize.  dst[i] = round_to_dst(mul_rn_f32(widen(src[i]), d(s))); d(s) has bits s << 23 for s in 1..254 and
 *   0x00400000 for s = 0; for s = 255 every element of the block is a NaN of unspecified pattern.  An f32
 *   destination holds the product itself; bf16 and f16 take the one RNE of ftar_cast_scaled's dequantizes (f16 may
 *   overflow to +-inf).
 * ftar_mx_quantize(FTAR_MX_COMPUTE) stores exactly what ftar_mx_scales followed by ftar_mx_quantize(FTAR_MX_GIVEN)
 * stores.  After the pair check, FTAR_ERR_INVALID_ARG: a NULL src / dst / scales with count > 0, a mode outside the
 * enum, a headroom outside 0..31, a headroom != 0 with FTAR_MX_GIVEN; every refusal comes before any device work
 * and leaves every buffer untouched.  count == 0 succeeds and writes nothing.  Pointers need only their element's
 * alignment and scales none: a call whose src and dst are both 16-byte aligned runs the vector kernels, any other
 * an element-wise family (one block per lane) that stores the same bits.  Each call enqueues kernels only -- no
 * memset, no host read, no synchronisation -- so it captures into a HIP graph and the scales may come from an
 * earlier kernel on the stream.  Splitting [0, n) at a multiple of 32 into two calls stores the same bits.  src,
 * dst and scales must not overlap.
 *   Stochastic quantize (ftar_mx_quantize_sr): ftar_mx_quantize with the narrowing of the stochastic-rounding
 *   paragraph above.  Element i of the call stores sr_dst(mul_rn_f32(widen(src[i]), q(s)), U(*seed, offset + i)), s
 *   the scale byte of i's block, sr_dst and U exactly those of that paragraph: block b of a call stores what
 *   ftar_cast_scaled_sr stores for that block with r = q(s_b) and offset + 32b.  Everything else is
 *   ftar_mx_quantize's -- scale bytes, q(s), modes, headroom, the six pairs.  The scale bytes do not depend on the
 *   rounding: FTAR_MX_COMPUTE writes the bytes ftar_mx_scales writes, and stores the payload that ftar_mx_scales
 *   followed by ftar_mx_quantize_sr(FTAR_MX_GIVEN) stores given the same seed and offset.  A block with s = 255
 *   (q = 1.0f) has the stochastic plain cast as its payload.  Under FTAR_MX_COMPUTE a finite block still stores no
 *   NaN and no inf, for every word: its scaled peak is at most the format's largest finite value, which is
 *   representable and so stored unchanged, and the carry of a smaller magnitude cannot pass it.  FTAR_MX_GIVEN with
 *   foreign scales may overflow as the RNE quantize does, with ftar_cast_scaled_sr's probabilities.  The word
 *   depends only on *seed (device memory, 8-byte aligned, read by the kernel on the stream, never by the host) and
 *   on offset + i (mod 2^64): not on alignment, on the vector or element-wise family that ran, on the grid or the
 *   tile, or on how the call was split -- splitting [0, n) at a multiple of 32 into two calls, the second with
 *   offset + cut, stores the one-call bits.  Refusals, in this order, all before any device work and leaving every
 *   buffer untouched: an unsupported pair FTAR_ERR_UNSUPPORTED; then FTAR_ERR_INVALID_ARG for a mode outside the
 *   enum; a headroom outside 0..31 or != 0 with FTAR_MX_GIVEN; a NULL seed or one not 8-byte aligned (at count == 0
 *   too, as in ftar_cast_scaled_sr); a NULL src / dst / scales with count > 0.  count == 0 otherwise succeeds and
 *   writes nothing.  The call enqueues kernels only, so it captures into a HIP graph, and a replay follows whatever
 *   the seed word, the source and the scales hold on the device at that time.
 * MXFP6 / MXFP4 are not covered.
 * The MPI drop-in (ftar_mpi.h) keeps the reference's datatype and op list: none of these extensions. */

typedef enum {
  FTAR_SUCCESS = 0,
  FTAR_ERR_INVALID_ARG = 1,
  FTAR_ERR_UNSUPPORTED = 2,   /* dtype/op pair the reference rejects too */
  FTAR_ERR_INVALID_TOPO = 3,  /* reference: "invalid FT_TOPO" + exit(1) */
  FTAR_ERR_HIP = 4,
  FTAR_ERR_RCCL = 5,
  FTAR_ERR_INTERNAL = 6,
  FTAR_ERR_TIMEOUT = 7,
  FTAR_ERR_NO_MEMORY = 8      /* a device allocation (scratch, staging, exchange buffer) failed */
} ftar_status_t;

/* Topology = FT_TOPO stage widths (bottom-up) + FT_LONELY count.  ring != 0
 * selects the ring schedule (reference: any width 1 in FT_TOPO). */
typedef struct {
  int nstages;
  int stages[FTAR_MAX_STAGES];
  int lonely;
  int ring;
} ftar_topo_t;

typedef struct ftar_comm* ftar_comm_t;
typedef struct {
  char internal[128];
} ftar_unique_id_t; /* == ncclUniqueId */

const char* ftar_version(void);
const char* ftar_status_string(ftar_status_t s);
/* Detail of the last failure on the calling thread ("" if none). */
const char* ftar_last_error(void);
size_t ftar_dtype_size(ftar_dtype_t dt);

/* ---- L3: k-way element-wise reduce on one device -------------------------
 * dst[i] = srcs[0][i] OP srcs[1][i] OP ... left to right, i < count; OP is
 * + (SUM), & (BAND), max or min (the support matrix is at ftar_op_t above).
 * srcs: HOST array of k device pointers; dst may be the same address as any
 * one source (in place: every element of every source is read before that
 * element is written); a dst that partly overlaps a source is undefined.
 * k == 1 copies (vector_add/reduce_sum.h:36-47).  stream: hipStream_t. */
ftar_status_t ftar_reduce(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dtype,
                          ftar_op_t op, void* stream);
/* Nested fold (extension; the one-round reduce-scatter of a multi-stage tree):
 * the k sources are the leaves, in depth-first order, of a mixed-radix tree
 * with bottom-up widths shape[0..nlevels) (product == k, nlevels <= 4).  Level
 * 0 folds shape[0] consecutive leaves, level 1 folds shape[1] consecutive
 * level-0 results, ... each node left to right; bf16, fp16 and fp8 inner nodes
 * are rounded to their format (what a staged tree stores between its stages).
 * Integer sums, AND, MAX and MIN are associative: the result equals
 * ftar_reduce's (the flat kernel runs).  nlevels <= 1 is ftar_reduce.  dst
 * may be the same address as any one source, as for ftar_reduce. */
ftar_status_t ftar_reduce_nested(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dtype,
                                 ftar_op_t op, const int* shape, int nlevels, void* stream);
/* Scaled SUM (extension; AVG's root fold on one device) of f32, f64, bf16, f16 or fp8: flat for nlevels <= 1,
 * nested as ftar_reduce_nested otherwise, finishing as dst = round_to_dtype(A x scale) -- A the fold's
 * accumulator before its one rounding (fp32 for bf16 / f16 / fp8; a nested fold's root, its inner nodes rounded
 * as ever), scale cast to float unless the dtype is f64, one correctly rounded multiply, subnormal products
 * kept.  k == 1 is a scaled copy; dst may be the same address as any one source (partial overlap is
 * undefined).  A non-finite scale returns FTAR_ERR_INVALID_ARG,
 * other dtypes FTAR_ERR_UNSUPPORTED, both before any device work. */
ftar_status_t ftar_reduce_scaled(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dtype,
                                 double scale, const int* shape, int nlevels, void* stream);
/* ftar_reduce_scaled plus the amax of what it stored (extension; the amax paragraph above): *amax = the
 * maximum of |dst[i]| over the count elements as stored, as a float.  scale == 1.0 gives the plain SUM's bits
 * (the multiply is exact).  f64 is refused (FTAR_ERR_UNSUPPORTED).  Enqueues a 4-byte memset of *amax and one
 * kernel, so it captures into a HIP graph as those two nodes. */
ftar_status_t ftar_reduce_amax(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dtype,
                               double scale, const int* shape, int nlevels, float* amax, void* stream);
/* Scaled cast between a wide float and an fp8 format (extension; the scaled-casts paragraph above):
 * dst[i] = round_to_dst(fp32(src[i]) x *scale) for i < count, one streaming kernel on `stream`.  scale: one float
 * in device memory on the current device, 4-byte aligned, read by the kernel (NULL: 1.0).  amax: as in
 * ftar_reduce_amax, or NULL; with it the call enqueues a 4-byte memset of *amax and the kernel, and captures into
 * a HIP graph as those two nodes (without it: the kernel alone, storing the same bits).  count == 0 succeeds and a
 * non-NULL amax then holds +0.0.  Pointers need no alignment beyond their element's: pairs whose 16-byte
 * alignments do not fit each other run an element-wise kernel. */
ftar_status_t ftar_cast_scaled(const void* src, ftar_dtype_t src_dtype, void* dst, ftar_dtype_t dst_dtype,
                               size_t count, const float* scale, float* amax, void* stream);
/* ftar_cast_scaled's quantize with stochastic rounding (extension; the stochastic-rounding paragraph above):
 * dst[i] = sr_dst(fp32(src[i]) x *scale, U(*seed, offset + i)), src in {f32, bf16, f16}, dst in {f8e4m3, f8e5m2}.
 * seed: one uint64_t in device memory on the current device, 8-byte aligned, read by the kernel; offset: the
 * global index of element 0, so consecutive calls with a running offset never reuse a word.  scale, amax, count
 * == 0, pointer alignment and graph capture (a 4-byte memset and one kernel with amax, the kernel alone without)
 * as for ftar_cast_scaled. */
ftar_status_t ftar_cast_scaled_sr(const void* src, ftar_dtype_t src_dtype, void* dst, ftar_dtype_t dst_dtype,
                                  size_t count, const float* scale, const uint64_t* seed, uint64_t offset,
                                  float* amax, void* stream);
/* MX block-scaled casts (extension; the MX paragraph above): fp8 elements plus one E8M0 scale byte per 32. */
#define FTAR_MX_BLOCK 32
typedef enum { FTAR_MX_COMPUTE = 0, FTAR_MX_GIVEN = 1 } ftar_mx_mode_t;
/* scales[b], b < ceil(count / 32), of a wide src for the fp8 format fp8_dtype: reads src once, writes nblocks bytes. */
ftar_status_t ftar_mx_scales(const void* src, ftar_dtype_t src_dtype, ftar_dtype_t fp8_dtype, size_t count,
                             int headroom, uint8_t* scales, void* stream);
/* FTAR_MX_COMPUTE: one pass over src that writes scales[] and dst[]; FTAR_MX_GIVEN: reads scales[] (device memory,
 * possibly written by an earlier kernel on the stream; headroom must be 0) and writes dst[]. */
ftar_status_t ftar_mx_quantize(const void* src, ftar_dtype_t src_dtype, void* dst, ftar_dtype_t dst_dtype,
                               size_t count, int mode, int headroom, uint8_t* scales, void* stream);
/* ftar_mx_quantize with stochastic rounding (the MX paragraph's stochastic quantize): element i takes the word
 * U(*seed, offset + i).  seed: one uint64_t in device memory on the current device, 8-byte aligned, read by the
 * kernel; offset: the global index of element 0 -- a running offset over consecutive calls never reuses a word. */
ftar_status_t ftar_mx_quantize_sr(const void* src, ftar_dtype_t src_dtype, void* dst, ftar_dtype_t dst_dtype,
                                  size_t count, int mode, int headroom, uint8_t* scales,
                                  const uint64_t* seed, uint64_t offset, void* stream);
/* dst[i] = round_to_dst(fp32(src[i]) x 2^(scales[i / 32] - 127)), src fp8, dst f32 / bf16 / f16. */
ftar_status_t ftar_mx_dequantize(const void* src, ftar_dtype_t src_dtype, const uint8_t* scales, void* dst,
                                 ftar_dtype_t dst_dtype, size_t count, void* stream);

/* ---- topology ------------------------------------------------------------
 * ftar_topo_parse: FT_TOPO / FT_LONELY strings (NULL = unset) for nranks.
 * Unlike the reference (mpi_mod.hpp:1447-1475, which exit(1)s when FT_TOPO
 * is unset and P > 1), an unset FT_TOPO returns FTAR_ERR_INVALID_TOPO so the
 * caller can fall back to ftar_topo_choose. */
ftar_status_t ftar_topo_parse(const char* ft_topo, const char* ft_lonely, int nranks, ftar_topo_t* out);
/* FT_TOPO/FT_LONELY from the environment, else ftar_topo_choose(nranks, bytes). */
ftar_status_t ftar_topo_from_env(int nranks, size_t bytes, ftar_topo_t* out);
/* The topology the execution model (below) chooses among all ordered
 * factorizations of nranks (plus the ring) at the default data movement (the
 * one-round direct forms, the best piece): the reference's own question
 * (cost_model/CostModel.h:82-120).  FTAR_COST_MODEL=reference: the
 * reference's scores instead. */
ftar_status_t ftar_topo_choose(int nranks, size_t bytes, ftar_topo_t* out);
/* The candidate set the cost model scores, in the reference's getWidth order
 * (cost_model/GetWidth.h:42-47; its [1,P]/[P,1] entries = the ring), plus the
 * single-stage width-P tree right after the ring (getWidth omits it; FT_TOPO=P
 * is valid).  Writes up to max_out entries, returns the total count (<0 = error). */
int ftar_topo_candidates(int nranks, ftar_topo_t* out, int max_out);
/* Predicted seconds of one topology for a bucket of `bytes` at that default
 * data movement (direct forms, the model's piece). */
double ftar_topo_cost(const ftar_topo_t* topo, int nranks, size_t bytes);
/* Three of the execution model's constants (ftar_cost_set sets them all):
 * alpha = one p2p group's latency (us), link = one peer's one-direction
 * bandwidth (GB/s), hbm = the reduce kernel's rate (GB/s).  Process-wide; a
 * value <= 0 restores the default; the environment (FTAR_COST_ALPHA_US /
 * _LINK_GBPS / _HBM_GBPS) overrides both. */
ftar_status_t ftar_cost_set_params(double alpha_us, double link_gbps, double hbm_gbps);
ftar_status_t ftar_cost_get_params(double* alpha_us, double* link_gbps, double* hbm_gbps);

/* ---- execution model: (topology, data-movement form, pipeline piece) -------
 * The role of the reference's CostModel (cost_model/CostModel.h:82-120: a
 * width list chosen for a chunk size), re-derived for one MI355X node.  With
 * the one-round forms every topology moves tree(P)'s bytes, so what varies on
 * a node is the form and the piece size; the model prices both:
 *   per piece of a round: r(x) = max(alpha + x / link, issue)  (x = bytes per
 *   link), a fold of k sources (k + 1) * c / hbm on the reduce stream, the
 *   fill / drain of that two-stream pipeline simulated piece by piece; peer
 *   forms: barriers, xGMI loads / stores and their local copy pass.
 * Forms (ftar_comm_set_form; the env FTAR_FORM=auto|direct|stages|collective|
 * peer-read|peer-write at init): */
typedef enum {
  FTAR_FORM_AUTO = -1,       /* the model chooses per call (the default) */
  FTAR_FORM_DIRECT = 0,      /* one-round reduce-scatter + all-gather, RCCL p2p */
  FTAR_FORM_STAGES = 1,      /* the reference's rounds both ways, RCCL p2p */
  FTAR_FORM_COLLECTIVE = 2,  /* one-round reduce-scatter + ncclAllGather */
  FTAR_FORM_PEER_READ = 3,   /* IPC peer-direct read (FTAR_PEER_READ) */
  FTAR_FORM_PEER_WRITE = 4   /* IPC peer-direct write (FTAR_PEER_WRITE) */
} ftar_form_t;
/* The model's constants, SI-like units as named.  A field <= 0 in
 * ftar_cost_set restores its default; FTAR_COST_<FIELD> in the environment
 * (ALPHA_US, LINK_GBPS, HBM_GBPS, ISSUE_US, BARRIER_US, PEER_READ_GBPS,
 * PEER_WRITE_GBPS, COPY_GBPS, COLL_GBPS) overrides both.  peer_*_gbps and
 * coll_gbps default to 0 = unmeasured: those forms are then never chosen.
 * Process-wide; every rank must hold the same values (compared at a
 * communicator's first call). */
typedef struct {
  double alpha_us;        /* one p2p group (one piece of one round): launch + handshake */
  double link_gbps;       /* RCCL p2p, one peer, one direction */
  double hbm_gbps;        /* the fold's rate, algorithmic bytes ((k+1) x piece) per second */
  double issue_us;        /* host time to enqueue one piece of one round (groups, events, fold) */
  double barrier_us;      /* one stream-ordered barrier of the peer forms */
  double peer_read_gbps;  /* one peer, kernel loads over xGMI (0 = unmeasured) */
  double peer_write_gbps; /* one peer, kernel stores over xGMI (0 = unmeasured) */
  double copy_gbps;       /* local copy, algorithmic bytes (read + written) per second */
  double coll_gbps;       /* ncclAllGather: bytes each rank receives per second (0 = unmeasured) */
} ftar_cost_params_t;
ftar_status_t ftar_cost_set(const ftar_cost_params_t* params);
ftar_status_t ftar_cost_get(ftar_cost_params_t* params);
/* Calibration files: the constants a run on the node fitted (bench.py --save-cost), so every later
 * MPI_Allreduce_FT on that node prices with them.  One "<field> <value>" per line ('#' comments), the
 * fields named as in ftar_cost_params_t, values > 0; fields left out keep their defaults.  Precedence:
 * FTAR_COST_<FIELD> > ftar_cost_set > FTAR_COST_FILE's file > ftar_cost_load's file > the defaults.
 * FTAR_COST_FILE=<path> loads one (re-read when the variable changes; an unreadable or malformed file
 * leaves the constants as they were and fails communicator bring-up with FTAR_ERR_INVALID_ARG; unsetting
 * the variable drops its file's constants, not ftar_cost_load's).  ftar_cost_load(NULL) forgets the loaded
 * constants; a malformed file loads nothing.  ftar_cost_save writes the constants in effect. */
ftar_status_t ftar_cost_load(const char* path);
ftar_status_t ftar_cost_save(const char* path);
/* Predicted seconds of one AllReduce of `bytes` per rank: topology, form
 * (not AUTO), piece size (0 = whole blocks); registered != 0 prices the peer
 * forms on registered buffers (no local pass).  < 0: not runnable that way. */
double ftar_cost_predict(const ftar_topo_t* topo, int form, size_t chunk_bytes, int nranks, size_t bytes,
                         int registered);
typedef struct {
  ftar_topo_t topo;
  int form;            /* ftar_form_t */
  size_t chunk_bytes;  /* pipeline piece (the one-round and staged forms); 0 for the peer forms */
  double seconds;      /* predicted */
  int tied;            /* candidates priced equal to the choice (within 1e-9), the choice included:
                          1 = a strict argmin; > 1 = the model could not tell them apart */
  int tie_broken_by;   /* ftar_tie_t: the highest-ranked rule that set the choice apart from a tied one */
} ftar_exec_t;
/* Tie rules of ftar_exec_choose, in the order they apply. */
typedef enum {
  FTAR_TIE_NONE = 0,    /* no tie */
  FTAR_TIE_STAGES = 1,  /* the fewest stages (the ring last: the flat fold rounds bf16 once) */
  FTAR_TIE_FORM = 2,    /* the simpler form (ftar_form_t order) */
  FTAR_TIE_PIECE = 3    /* the larger piece (fewer p2p groups; whole blocks first) */
} ftar_tie_t;
#define FTAR_CHOOSE_TOPO 1  /* the topology is free (else inout->topo is used) */
#define FTAR_CHOOSE_FORM 2  /* the form is free (else inout->form) */
#define FTAR_CHOOSE_CHUNK 4 /* the piece size is free (else inout->chunk_bytes) */
#define FTAR_CHOOSE_PEER 8  /* the peer forms may be chosen (their rates permitting) */
/* The model's argmin over what `flags` leaves free; ties keep the fewest
 * stages, then the simpler form, then the larger piece, and the result says
 * how many candidates tied and which rule decided (tied, tie_broken_by): in
 * the direct form every one-round topology moves tree(P)'s bytes over the
 * same links, so those price alike and the stage count picks tree(P). */
ftar_status_t ftar_exec_choose(int nranks, size_t bytes, int flags, ftar_exec_t* inout);

/* The reference's own cost model, restated bit for bit
 * (cost_model/CostModel.h:1-120; tests/golden/costmodel.jsonl holds its
 * output).  ftar_topo_choose uses it instead of the xGMI model when
 * FTAR_COST_MODEL=reference (chunk = FTAR_COST_REF_CHUNK, default 100 as in
 * cost_model/main.cpp:23).
 *   ftar_cost_reference       score of one getWidth-style width list (a width
 *                             1 = the ring's [1,P]/[P,1]); < 0 where the
 *                             reference has no case (height 0 or > 9)
 *   ftar_topo_choose_reference its argmin over getWidth(P), first minimum wins
 *                             (CostModel.h:97); *index = position in that list
 *   ftar_cost_reference_candidates getWidth(P) (GetWidth.h:42-47) flattened:
 *                             returns the number of lists, their lengths in
 *                             lengths[], their widths concatenated in widths[] */
double ftar_cost_reference(const int* widths, int nwidths, int nranks, double chunk);
ftar_status_t ftar_topo_choose_reference(int nranks, double chunk, ftar_topo_t* out, int* index);
int ftar_cost_reference_candidates(int nranks, int* widths, int max_widths, int* lengths, int max_lists);
/* Writes "w0,w1,..+L" / "ring" into buf; returns needed length. */
int ftar_topo_format(const ftar_topo_t* topo, char* buf, size_t buflen);

/* ---- communicators -------------------------------------------------------- */
ftar_status_t ftar_get_unique_id(ftar_unique_id_t* id);
/* One process per GPU over RCCL p2p (xGMI). Collective across nranks. */
ftar_status_t ftar_comm_init_rank(ftar_comm_t* comm, int nranks, ftar_unique_id_t id, int rank, int device);
/* nranks communicators inside ONE process (thread transport: stream-ordered
 * device copies).  All ranks may share one device (test mode on a 1-GPU box).
 * Each ftar_allreduce on them must be issued from its own host thread, or via
 * ftar_allreduce_group. */
ftar_status_t ftar_comm_init_local(ftar_comm_t* comms, int nranks, const int* devices);
/* One process per rank, bootstrapped by the caller's own host collective (MPI,
 * gloo, ...): `allgather` copies `bytes` from `mine` into slot `rank` of `all`
 * on every rank and returns 0 on success.  Data moves only by the peer-direct
 * forms (IPC-mapped exchange or registered buffers; set FTAR_PEER_READ or
 * FTAR_PEER_WRITE): p2p transfers are FTAR_ERR_UNSUPPORTED, so staged and
 * lonely plans cannot run on it.  Barriers synchronize the stream and then
 * the host collective (blocking).  Ranks may share a device. */
typedef int (*ftar_host_allgather_fn)(const void* mine, void* all, size_t bytes, void* user);
ftar_status_t ftar_comm_init_host(ftar_comm_t* comm, int nranks, int rank, int device, ftar_host_allgather_fn allgather,
                                  void* user);
ftar_status_t ftar_comm_destroy(ftar_comm_t comm);
ftar_status_t ftar_comm_rank(ftar_comm_t comm, int* rank);
ftar_status_t ftar_comm_size(ftar_comm_t comm, int* size);
ftar_status_t ftar_comm_device(ftar_comm_t comm, int* device);
/* The communicator's transport: "rccl", "local" (in-process group) or "host" (ftar_comm_init_host). */
const char* ftar_comm_transport(ftar_comm_t comm);
/* Pipelining granularity of the transfers (bytes, rounded to 256 B); 0 = the
 * execution model's piece for each call (the default; FTAR_CHUNK_BYTES at
 * init fixes it).  get: 0 while the model chooses. */
ftar_status_t ftar_comm_set_chunk_bytes(ftar_comm_t comm, size_t bytes);
ftar_status_t ftar_comm_get_chunk_bytes(ftar_comm_t comm, size_t* bytes);
/* The data-movement form (ftar_form_t).  FTAR_FORM_AUTO (the default): the
 * execution model chooses per call among the forms the communicator can run
 * (peer forms only once their rates are set, ftar_cost_set); any other value
 * fixes it, as do ftar_comm_set_allgather / _reduce_scatter / _peer_direct
 * (get then reports the form those describe, or -2 for a mix no form names).
 * A host-bootstrapped communicator keeps its peer form.
 * ftar_comm_last_exec: what the last call on this communicator ran -- the
 * topology, the form of the path actually taken (host buffers on an RCCL
 * communicator run the pipelined p2p path whatever peer form is set; a ring
 * or host buffers replace the collective all-gather with the direct one; -2
 * for a mix no form names), the piece it ran in bytes (host buffers: the
 * host piece; 0: whole blocks, or a peer form on device buffers), and the
 * model's predicted seconds (-1: unpriced). */
ftar_status_t ftar_comm_set_form(ftar_comm_t comm, int form);
ftar_status_t ftar_comm_get_form(ftar_comm_t comm, int* form);
ftar_status_t ftar_comm_last_exec(ftar_comm_t comm, ftar_exec_t* out);
/* How the all-gather phase is moved.  After the reduce-scatter stages every
 * rank holds exactly one fully reduced block (block r on trees, lonely ranks
 * included; block (r+1) mod P on the ring), so the phase only delivers final
 * values and every form gives bit-identical results:
 *   FTAR_AG_STAGES      the reference's rounds (ring: P-1 neighbour steps,
 *                       tree: the k stages reversed, mpi_mod.hpp:1620-1644, :1705-1715)
 *   FTAR_AG_DIRECT      one p2p group: each rank sends its block to all P-1
 *                       peers at once (every xGMI link busy; default)
 *   FTAR_AG_COLLECTIVE  one ncclAllGather (non-lonely trees with P | count;
 *                       otherwise DIRECT)
 * Default: FTAR_ALLGATHER=stages|direct|collective at init, else DIRECT. */
typedef enum { FTAR_AG_STAGES = 0, FTAR_AG_COLLECTIVE = 1, FTAR_AG_DIRECT = 2 } ftar_allgather_t;
ftar_status_t ftar_comm_set_allgather(ftar_comm_t comm, ftar_allgather_t mode);
ftar_status_t ftar_comm_get_allgather(ftar_comm_t comm, ftar_allgather_t* mode);
/* How the ring's reduce-scatter is moved.  The ring folds block b as
 * x_b + x_{b+1} + ... + x_{b+P-1} (left to right, indices mod P; the reference's
 * own+recv per hop is that fold since IEEE addition commutes), finishing on rank
 * b-1 (mpi_mod.hpp:1689-1703):
 *   FTAR_RS_STAGES  the reference's P-1 neighbour steps (one xGMI link per rank)
 *   FTAR_RS_DIRECT  rank b-1 gathers every rank's block b in ONE round over all
 *                   links and folds them in that order with one k=P reduce
 *                   (bf16, fp16, fp8: rounded after every add, i.e. once per hop, as staged)
 * Identical results.  Multi-stage trees without lonely ranks (at most 4
 * stages) likewise: FTAR_RS_DIRECT gathers the P copies of block r on rank r
 * in one round and folds them as the tree would (ftar_reduce_nested), bit for
 * bit; lonely layouts and single-stage trees keep their stages.
 * Default: FTAR_REDUCE_SCATTER=stages|direct, else DIRECT. */
typedef enum { FTAR_RS_STAGES = 0, FTAR_RS_DIRECT = 1 } ftar_reduce_scatter_t;
ftar_status_t ftar_comm_set_reduce_scatter(ftar_comm_t comm, ftar_reduce_scatter_t mode);
ftar_status_t ftar_comm_get_reduce_scatter(ftar_comm_t comm, ftar_reduce_scatter_t* mode);

/* Peer-direct data movement (extension; default off, FTAR_PEER_DIRECT=1|read
 * or 2|write at init).  For one-round plans (the ring, and trees without
 * lonely ranks, under FTAR_RS_DIRECT-or-single-stage + FTAR_AG_DIRECT), the
 * blocks move by kernel loads/stores through IPC-mapped, comm-owned exchange
 * buffers over xGMI instead of RCCL p2p into scratch:
 *   FTAR_PEER_READ   each rank's fold reads the other ranks' copies of its
 *                    block from their exchange buffers, and the all-gather
 *                    pulls every final block (three stream-ordered barriers);
 *   FTAR_PEER_WRITE  each rank pushes its copy of every peer's block into that
 *                    peer's buffer, folds locally, and pushes its final block
 *                    to every peer (three barriers: the last keeps
 *                    my exchange buffer until my copy-out has read it).
 * The plan's fold is executed unchanged: same bits.  Other plans keep RCCL p2p. */
typedef enum { FTAR_PEER_OFF = 0, FTAR_PEER_READ = 1, FTAR_PEER_WRITE = 2 } ftar_peer_mode_t;
ftar_status_t ftar_comm_set_peer_direct(ftar_comm_t comm, int mode);
ftar_status_t ftar_comm_get_peer_direct(ftar_comm_t comm, int* mode);
/* Registered (symmetric) buffers for the peer forms, like RCCL's user-buffer
 * registration.  Collective: every rank registers its own buffer of the same
 * role in the same call order; *reg is the same id on every rank.  A call
 * whose buffers lie in registrations -- on EVERY rank, at the SAME offsets
 * -- skips the peer forms' local pass: READ (sendbuf and recvbuf registered)
 * reads the peers' inputs and final blocks in place, three barriers, no
 * copy; WRITE (recvbuf registered) pushes final blocks straight into the
 * peers' outputs, two barriers, no copy.  Mixing registered and unregistered
 * buffers across ranks in one call is undefined.  deregister is local; the
 * buffer must not be freed before it (or before the calls using it ended).
 * The buffer must not be written while it is being registered: every peer
 * verifies its mapping against the owner's current first 16 bytes.
 * Under HIP runtimes older than 7.2 an allocation whose size has bit 31 set
 * cannot be registered (FTAR_ERR_HIP on every rank): those runtimes block in
 * hipIpcOpenMemHandle for such sizes.  FTAR_IPC_SIZE_GUARD=0|1 overrides. */
ftar_status_t ftar_comm_register(ftar_comm_t comm, void* buf, size_t bytes, int* reg);
ftar_status_t ftar_comm_deregister(ftar_comm_t comm, int reg);

/* ---- AllReduce (device resident) -------------------------------------------
 * sendbuf == NULL or == recvbuf: in place (MPI_IN_PLACE).  topo == NULL:
 * FT_TOPO/FT_LONELY read from the environment at THIS call, as get_stages is
 * on every MPI_Allreduce_FT call (mpi_mod.hpp:1732); both unset: the cost
 * model's choice; set but invalid for the communicator's size:
 * FTAR_ERR_INVALID_TOPO before anything is enqueued (the reference exit(1)s,
 * :1471-1475), 1-rank communicators included.  Enqueued on `stream`; returns
 * once enqueued. */
ftar_status_t ftar_allreduce(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dtype, ftar_op_t op,
                             const ftar_topo_t* topo, ftar_comm_t comm, void* stream);
/* Drive every rank of an ftar_comm_init_local group from this one call
 * (pooled host threads, one per rank at once); returns once every rank's
 * work is enqueued on its stream (streams == NULL: each device's NULL
 * stream), like ftar_allreduce -- synchronize the streams before reading
 * the results from the host.  ftar_allreduce_host_group returns once the
 * host buffers hold the result.
 * Under stream capture pass the capture stream itself for every rank (the
 * call is then captured serially, one graph chain); streams forked per rank
 * from the capture are refused with FTAR_ERR_UNSUPPORTED, as HIP's
 * hipStreamEndCapture recurses without end on them. */
ftar_status_t ftar_allreduce_group(const void* const* sendbufs, void* const* recvbufs, size_t count,
                                   ftar_dtype_t dtype, ftar_op_t op, const ftar_topo_t* topo, ftar_comm_t* comms,
                                   int nranks, void* const* streams);
/* ftar_allreduce / ftar_allreduce_group and the amax of the result (the amax paragraph at ftar_op_t above): the
 * same AllReduce, same bits, whose root folds also keep the largest |stored value| of the block they finish; a
 * second, internal AllReduce of one word per rank (an exact integer MAX on the fp32 bit patterns) and a 4-byte
 * write to *amax follow on the same stream.  amaxes: one device float per rank, on that rank's device. */
ftar_status_t ftar_allreduce_amax(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dtype, ftar_op_t op,
                                  const ftar_topo_t* topo, ftar_comm_t comm, float* amax, void* stream);
ftar_status_t ftar_allreduce_amax_group(const void* const* sendbufs, void* const* recvbufs, size_t count,
                                        ftar_dtype_t dtype, ftar_op_t op, const ftar_topo_t* topo, ftar_comm_t* comms,
                                        int nranks, float* const* amaxes, void* const* streams);

/* ---- AllReduce of HOST buffers (the reference's own setting) ---------------
 * Replaces MPI_Allreduce_FT's host-memory contract (mpi_mod.hpp:1723-1778).
 * sendbuf/recvbuf are host memory (sendbuf == NULL or == recvbuf: in place);
 * page-lock them (hipHostRegister / hipHostMalloc) or the copies are not
 * asynchronous.  The bucket moves through a grow-only device staging buffer in
 * pieces of host_chunk_bytes per block: H2D of later pieces, the exchange and
 * reduce of the current ones, and D2H of finished ones run at once (stage s+1
 * trails stage s by one piece), so PCIe in and out overlap.  Same blocks,
 * same fold order, same bits as ftar_allreduce.  Enqueued on `stream`; the
 * host buffers must stay untouched until it completes. */
ftar_status_t ftar_allreduce_host(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dtype,
                                  ftar_op_t op, const ftar_topo_t* topo, ftar_comm_t comm, void* stream);
ftar_status_t ftar_allreduce_host_group(const void* const* sendbufs, void* const* recvbufs, size_t count,
                                        ftar_dtype_t dtype, ftar_op_t op, const ftar_topo_t* topo,
                                        ftar_comm_t* comms, int nranks, void* const* streams);
/* Co-scheduling of the fold with the transport: the reduce stream runs on
 * `cus` of the device's CUs (spread evenly; 0 = all, the default), so the
 * comm stream's kernels (RCCL p2p, copies) always find free CUs while a
 * piece's fold runs (FTAR_REDUCE_CUS at init).  Same bits either way.
 * In-process (local) and host-bootstrapped communicators only: on an RCCL
 * communicator any cus other than 0 returns FTAR_ERR_UNSUPPORTED, and
 * FTAR_REDUCE_CUS fails ftar_comm_init_rank the same way.  The CU-masked
 * stream is a blocking stream on a hardware queue of its own, and over RCCL
 * two stress runs stalled ranks with it. */
ftar_status_t ftar_comm_set_reduce_cus(ftar_comm_t comm, int cus);
ftar_status_t ftar_comm_get_reduce_cus(ftar_comm_t comm, int* cus);
/* Host-mode piece size per block (bytes, rounded to 256 B); 0 = auto: 16 MiB,
 * at least 1/64 of a block (FTAR_HOST_CHUNK_BYTES at init). */
ftar_status_t ftar_comm_set_host_chunk_bytes(ftar_comm_t comm, size_t bytes);
ftar_status_t ftar_comm_get_host_chunk_bytes(ftar_comm_t comm, size_t* bytes);

/* ---- diagnostics ---------------------------------------------------------------
 * RCCL's own ncclAllReduce on the communicator's RCCL comm (ring/tree of the
 * vendor library, reduction inside RCCL): the yardstick bench.py reports next
 * to ftar at N > 1.  FTAR_ERR_UNSUPPORTED on local (in-process) groups, for
 * the types RCCL lacks (u16, i16, bool) and for BAND.  SUM, MAX, MIN and AVG map to
 * ncclSum / ncclMax / ncclMin / ncclAvg, fp16 to ncclFloat16, the fp8 formats to ncclFloat8e4m3 / ncclFloat8e5m2
 * (an RCCL built without them: FTAR_ERR_UNSUPPORTED): the arithmetic is RCCL's, so its NaN and signed-zero rules
 * for max / min, where it rounds a mean, and what its fp8 conversion does on overflow (it may saturate) may
 * differ from ftar's. */
ftar_status_t ftar_rccl_allreduce(const void* sendbuf, void* recvbuf, size_t count, ftar_dtype_t dtype, ftar_op_t op,
                                  ftar_comm_t comm, void* stream);
/* xGMI calibration (collective; every rank calls it): GB/s seen by this rank
 * for copy kernels through the peer-direct exchange buffers, all ranks running
 * the same pattern at once -- gbps[0] local HBM copy, [1] read from one peer
 * (ring neighbour), [2] read from all peers at once (aggregate), [3] write to
 * one peer, [4] write to all peers at once (aggregate), all by copy kernels;
 * [5] read from / [6] write to all peers by the DMA engines (one
 * hipMemcpyAsync per peer, each on its own stream).  bytes_per_peer per
 * copy, `iters` timed launches; grows the exchange buffer to 2*P*bytes. */
ftar_status_t ftar_xgmi_probe(ftar_comm_t comm, size_t bytes_per_peer, int iters, double* gbps, int n);
/* Phase timing of the last call on this communicator (diagnostic; off by
 * default): timing events at the phase boundaries -- per stage "moved" (comm
 * stream) and "reduced" (reduce stream) for the p2p executor in device mode,
 * every copy/fold/barrier for the peer forms.  ftar_comm_phase_json waits for
 * them and writes [["start", 0.0], [name, ms since start], ...]; returns the
 * needed length or < 0 on error. */
ftar_status_t ftar_comm_set_phase_timing(ftar_comm_t comm, int enable);
long ftar_comm_phase_json(ftar_comm_t comm, char* buf, size_t buflen);

/* ---- introspection (tests) -------------------------------------------------
 * FMA-level schedule of `rank` (same JSON shape as the reference dump in
 * tests/golden/schedules.jsonl). Returns needed length, or <0 on error. */
long ftar_schedule_json(const ftar_topo_t* topo, int nranks, int rank, size_t count, char* buf, size_t buflen);
/* Executable plan of `rank` (JSON): stages of transfers/reduces, scratch size,
 * and the forms actually used. */
long ftar_plan_json(const ftar_topo_t* topo, int nranks, int rank, size_t count, ftar_allgather_t allgather,
                    ftar_reduce_scatter_t reduce_scatter, char* buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* FTAR_H */
