// Production dispatch of the k-way reduce (ftar_reduce, the engine's folds) and the streaming copy;
// kernels and traits in reduce_impl.h.  Replaces FlexTree::reduce_sum<T>/reduce_band<T>
// (allreduce_over_mpi/mpi_mod.hpp:812-1251) and reduce_sum_gpu (vector_add/reduce_sum_gpu.h:205).
#include "reduce_impl.h"

#include <cxxabi.h>

#include <cstdlib>
#include <cstring>

namespace ftar {

size_t dtype_size(ftar_dtype_t dt) {
  switch (dt) {
    case FTAR_UINT8: case FTAR_INT8: case FTAR_BOOL: case FTAR_FLOAT8_E4M3: case FTAR_FLOAT8_E5M2: return 1;
    case FTAR_UINT16: case FTAR_INT16: case FTAR_BFLOAT16: case FTAR_FLOAT16: return 2;
    case FTAR_INT32: case FTAR_FLOAT32: return 4;
    case FTAR_INT64: case FTAR_FLOAT64: return 8;
  }
  return 0;
}

bool dtype_scalable(ftar_dtype_t dt) {
  return dt == FTAR_FLOAT32 || dt == FTAR_FLOAT64 || dt == FTAR_BFLOAT16 || dt == FTAR_FLOAT16 ||
         dt == FTAR_FLOAT8_E4M3 || dt == FTAR_FLOAT8_E5M2;
}

bool dtype_has_amax(ftar_dtype_t dt) { return dtype_scalable(dt) && dt != FTAR_FLOAT64; }

bool dtype_op_supported(ftar_dtype_t dt, ftar_op_t op) {
  if (dtype_size(dt) == 0) return false;
  switch (op) {
    case FTAR_SUM: return true;
    case FTAR_BAND:  // mpi_mod.hpp:1389-1396: integer types only
      return dt == FTAR_UINT8 || dt == FTAR_INT8 || dt == FTAR_UINT16 || dt == FTAR_INT16 || dt == FTAR_INT32 ||
             dt == FTAR_INT64;
    case FTAR_MAX: case FTAR_MIN: return dt != FTAR_BOOL;  // MPI defines no MAX / MIN on logical types either
    case FTAR_AVG: return dtype_scalable(dt);  // the AllReduce entry points only (the engine: SUM + a scaled root)
  }
  return false;
}

namespace {
// the segments with bytes, packed, and the grid: workgroups per segment to cover the largest in one pass
// (at most 65535, then grid-stride; max_wg_per_seg caps it), times the segments
GatherGeom pack_segments(const Segment* segs, int nsegs, size_t max_wg_per_seg, SegArgs* a) {
  GatherGeom g;
  size_t most = 0;
  for (int i = 0; i < nsegs; ++i) {
    if (!segs[i].bytes) continue;
    a->src[g.nsegs] = static_cast<const char*>(segs[i].src);
    a->dst[g.nsegs] = static_cast<char*>(segs[i].dst);
    a->bytes[g.nsegs] = segs[i].bytes;
    most = std::max(most, segs[i].bytes);
    ++g.nsegs;
  }
  if (!g.nsegs) return g;
  size_t bx = (most / 16 + 2 * kThreads - 1) / (2 * kThreads);
  bx = std::max<size_t>(1, std::min<size_t>(bx, 65535));  // per segment; grid-stride beyond
  if (max_wg_per_seg) bx = std::min(bx, max_wg_per_seg);
  g.grid = (unsigned)(bx * (size_t)g.nsegs);
  g.tile_bytes = 2 * kThreads * 16;
  return g;
}
}  // namespace

GatherGeom gather_geometry(const Segment* segs, int nsegs, size_t max_wg_per_seg) {
  if (nsegs < 0 || nsegs > FTAR_MAX_K) return GatherGeom{};
  SegArgs a{};
  return pack_segments(segs, nsegs, max_wg_per_seg, &a);
}

ftar_status_t launch_gather(const Segment* segs, int nsegs, hipStream_t stream, bool nt, size_t max_wg_per_seg,
                            bool release_system) {
  if (nsegs < 0 || nsegs > FTAR_MAX_K) return FTAR_ERR_INVALID_ARG;
  SegArgs a{};
  const GatherGeom g = pack_segments(segs, nsegs, max_wg_per_seg, &a);
  if (!g.nsegs) return FTAR_SUCCESS;
  const int m = (int)g.nsegs;
  const dim3 grid(g.grid);
  if (release_system && nt)
    FTAR_LAUNCH((gather_kernel<true, true>), grid, dim3(kThreads), 0, stream, a, m);
  else if (release_system)
    FTAR_LAUNCH((gather_kernel<false, true>), grid, dim3(kThreads), 0, stream, a, m);
  else if (nt)
    FTAR_LAUNCH(gather_kernel<true>, grid, dim3(kThreads), 0, stream, a, m);
  else
    FTAR_LAUNCH(gather_kernel<false>, grid, dim3(kThreads), 0, stream, a, m);
  FTAR_CHECK_HIP(hipGetLastError());
  return FTAR_SUCCESS;
}

ftar_status_t launch_gather_logged(const Segment* segs, int nsegs, hipStream_t stream, bool nt,
                                   size_t max_wg_per_seg, unsigned* host_log, unsigned* dev_log, size_t cap_wg) {
  if (nsegs < 0 || nsegs > FTAR_MAX_K || !host_log || !dev_log) return FTAR_ERR_INVALID_ARG;
  SegArgs a{};
  const GatherGeom g = pack_segments(segs, nsegs, max_wg_per_seg, &a);
  if (!g.nsegs) return FTAR_SUCCESS;
  if (g.grid > cap_wg) return FTAR_ERR_INVALID_ARG;  // one record per workgroup must fit
  const int m = (int)g.nsegs;
  if (nt)
    FTAR_LAUNCH(gather_logged_kernel<true>, dim3(g.grid), dim3(kThreads), 0, stream, a, m, host_log, dev_log);
  else
    FTAR_LAUNCH(gather_logged_kernel<false>, dim3(g.grid), dim3(kThreads), 0, stream, a, m, host_log, dev_log);
  FTAR_CHECK_HIP(hipGetLastError());
  return FTAR_SUCCESS;
}

namespace {
__global__ void noop_kernel() {}
}  // namespace

ftar_status_t launch_noop(hipStream_t stream) {
  FTAR_LAUNCH(noop_kernel, dim3(1), dim3(64), 0, stream);
  FTAR_CHECK_HIP(hipGetLastError());
  return FTAR_SUCCESS;
}

namespace {
// the LDS-staged kernel up to k = HOT, or (lds == false: the peer forms' ":vec" A/B) only at k = 2
template <class Tr, int HOT, bool SC = false>
hipError_t tr(bool lds, const void* const* srcs, int k, void* dst, size_t count, hipStream_t s, double r = 1.0) {
  return lds ? launch_tr<Tr, HOT, SC>(srcs, k, dst, count, s, r) : launch_tr<Tr, 0, SC>(srcs, k, dst, count, s, r);
}
// MAX / MIN of one dtype; HOT as the SUM of the same element width
template <bool MAX>
hipError_t tr_min_max(ftar_dtype_t dt, bool lds, const void* const* srcs, int k, void* dst, size_t count,
                      hipStream_t s) {
  switch (dt) {
    case FTAR_UINT8: return tr<MinMax<unsigned char, MAX>, 8>(lds, srcs, k, dst, count, s);
    case FTAR_INT8: return tr<MinMax<signed char, MAX>, 8>(lds, srcs, k, dst, count, s);
    case FTAR_UINT16: return tr<MinMax<unsigned short, MAX>, 8>(lds, srcs, k, dst, count, s);
    case FTAR_INT16: return tr<MinMax<short, MAX>, 8>(lds, srcs, k, dst, count, s);
    case FTAR_INT32: return tr<MinMax<int, MAX>, 8>(lds, srcs, k, dst, count, s);
    case FTAR_INT64: return tr<MinMax<long long, MAX>, 8>(lds, srcs, k, dst, count, s);
    case FTAR_FLOAT32: return tr<MinMax<float, MAX>, 16>(lds, srcs, k, dst, count, s);
    case FTAR_FLOAT64: return tr<MinMax<double, MAX>, 8>(lds, srcs, k, dst, count, s);
    case FTAR_BFLOAT16: return tr<BF16MinMax<MAX>, 16>(lds, srcs, k, dst, count, s);
    case FTAR_FLOAT16: return tr<MinMax<_Float16, MAX>, 16>(lds, srcs, k, dst, count, s);
    case FTAR_FLOAT8_E4M3: case FTAR_FLOAT8_E5M2: break;  // launch_reduce_f8
    case FTAR_BOOL: break;
  }
  return hipErrorInvalidValue;
}
// The float sums, nested or flat, in either finish: SC = the scaled finish (AVG's root folds,
// ftar_reduce_scaled) with the scale r.  A one-round ring fold (round_each, k > 2) of a 16-bit format rounds
// after every add; under a scaled finish it rounds before each add instead (H16SumHopPreT), so the last sum
// reaches the finish unrounded, as the staged ring's last hop (a plain k = 2 fold) hands it over.
template <bool SC>
ftar_status_t float_sum(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dt, hipStream_t s,
                        bool round_each, const int* shape, int nlevels, bool lds, double r) {
  hipError_t e = hipErrorInvalidValue;
  const bool hop = round_each && k > 2;
  if (nlevels > 1 && k > 1) {
    TreeCode tc;
    if (!shape || !make_tree_code(shape, nlevels, k, &tc)) return FTAR_ERR_INVALID_ARG;
    switch (dt) {
      case FTAR_FLOAT32: e = launch_tree<F32Sum, SC>(srcs, k, tc, shape, nlevels, dst, count, s, lds, r); break;
      case FTAR_FLOAT64: e = launch_tree<F64Sum, SC>(srcs, k, tc, shape, nlevels, dst, count, s, false, r); break;
      case FTAR_FLOAT16: e = launch_tree<F16Sum, SC>(srcs, k, tc, shape, nlevels, dst, count, s, lds, r); break;
      default: e = launch_tree<BF16Sum, SC>(srcs, k, tc, shape, nlevels, dst, count, s, lds, r); break;
    }
  } else {
    switch (dt) {
      case FTAR_FLOAT32: e = tr<F32Sum, 16, SC>(lds, srcs, k, dst, count, s, r); break;
      case FTAR_FLOAT64: e = tr<F64Sum, 8, SC>(lds, srcs, k, dst, count, s, r); break;
      case FTAR_FLOAT16:
        e = hop ? tr<std::conditional_t<SC, F16SumHopPre, F16SumHop>, 16, SC>(lds, srcs, k, dst, count, s, r)
                : tr<F16Sum, 16, SC>(lds, srcs, k, dst, count, s, r);
        break;
      default:
        e = hop ? tr<std::conditional_t<SC, BF16SumHopPre, BF16SumHop>, 16, SC>(lds, srcs, k, dst, count, s, r)
                : tr<BF16Sum, 16, SC>(lds, srcs, k, dst, count, s, r);
        break;
    }
  }
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}
}  // namespace

// The LDS-staged kernel with K = 1 on one-wave workgroups of one tile (U = 1, W = 1; byte traits, so any
// dtype): 6,530 vs 6,012 GB/s for the multi-segment copy kernel on cold 256 MiB buffers, the best of 17
// (U, W) shapes (tools/kbench_cold.py --ks 1, profiles/r03/kbench_copy.log).  Sources and destinations
// whose 16-byte alignments differ take the copy kernel, which handles any alignment.
ftar_status_t launch_copy(const void* src, void* dst, size_t bytes, hipStream_t s) {
  if (!bytes || src == dst) return FTAR_SUCCESS;
  const void* srcs[1] = {src};
  const Split16 sp = split16(srcs, 1, dst, bytes, 1);
  if (!sp.co_aligned) {
    const Segment seg{src, dst, bytes};
    return launch_gather(&seg, 1, s);
  }
  FTAR_CHECK_HIP((launch_lds<U8Sum, 1, 1, 1>(srcs, dst, sp.nvec, s, sp.head, sp.tail)));
  return FTAR_SUCCESS;
}

ftar_status_t launch_reduce(const void* const* srcs, int k, void* dst, size_t count, ftar_dtype_t dt, ftar_op_t op,
                            hipStream_t s, bool round_each, const int* shape, int nlevels, bool lds,
                            const double* scale, unsigned* amax) {
  if (k < 1 || k > FTAR_MAX_K || !srcs || !dst) return FTAR_ERR_INVALID_ARG;
  if (op == FTAR_AVG || !dtype_op_supported(dt, op)) return FTAR_ERR_UNSUPPORTED;  // AVG: the engine's SUM + scale
  if (scale && (op != FTAR_SUM || !dtype_scalable(dt))) return FTAR_ERR_UNSUPPORTED;
  if (amax && (!scale || !dtype_has_amax(dt))) return FTAR_ERR_UNSUPPORTED;
  if (count == 0) return FTAR_SUCCESS;
  for (int j = 0; j < k; ++j)
    if (!srcs[j]) return FTAR_ERR_INVALID_ARG;
  if (dt == FTAR_FLOAT8_E4M3 || dt == FTAR_FLOAT8_E5M2)  // every fp8 fold: reduce_f8.hip
    return launch_reduce_f8(srcs, k, dst, count, dt, op, s, round_each, shape, nlevels, lds, scale, amax);
  if (amax)  // the amax finish of f32, bf16 and fp16: reduce_amax.hip
    return launch_reduce_amax(srcs, k, dst, count, dt, s, round_each, shape, nlevels, lds, *scale, amax);
  // a scaled k = 1 is a scaled copy through the runtime-k kernel; a plain one is a copy
  if (scale) return float_sum<true>(srcs, k, dst, count, dt, s, round_each, shape, nlevels, lds, *scale);
  if (k == 1)  // vector_add/reduce_sum.h:36-47: a copy (a streaming kernel, not the DMA blit)
    return launch_copy(srcs[0], dst, count * dtype_size(dt), s);
  if (op == FTAR_SUM && dtype_scalable(dt))
    return float_sum<false>(srcs, k, dst, count, dt, s, round_each, shape, nlevels, lds, 1.0);
  hipError_t e = hipErrorInvalidValue;
  switch (op) {
  case FTAR_SUM:
    switch (dt) {
      case FTAR_FLOAT32: case FTAR_FLOAT64: case FTAR_BFLOAT16: case FTAR_FLOAT16: break;  // float_sum above
      case FTAR_FLOAT8_E4M3: case FTAR_FLOAT8_E5M2: break;  // launch_reduce_f8 above
      case FTAR_UINT8: case FTAR_INT8: e = tr<U8Sum, 8>(lds, srcs, k, dst, count, s); break;
      case FTAR_UINT16: case FTAR_INT16: e = tr<U16Sum, 8>(lds, srcs, k, dst, count, s); break;
      case FTAR_INT32: e = tr<U32Sum, 8>(lds, srcs, k, dst, count, s); break;
      case FTAR_INT64: e = tr<U64Sum, 8>(lds, srcs, k, dst, count, s); break;
      case FTAR_BOOL: e = tr<BoolSum, 8>(lds, srcs, k, dst, count, s); break;
    }
    break;
  case FTAR_BAND:
    switch (dt) {
      case FTAR_UINT8: case FTAR_INT8: e = tr<Band<unsigned char>, 8>(lds, srcs, k, dst, count, s); break;
      case FTAR_UINT16: case FTAR_INT16: e = tr<Band<unsigned short>, 8>(lds, srcs, k, dst, count, s); break;
      case FTAR_INT32: e = tr<Band<unsigned>, 8>(lds, srcs, k, dst, count, s); break;
      case FTAR_INT64: e = tr<Band<unsigned long long>, 8>(lds, srcs, k, dst, count, s); break;
      default: return FTAR_ERR_UNSUPPORTED;
    }
    break;
  case FTAR_MAX: e = tr_min_max<true>(dt, lds, srcs, k, dst, count, s); break;
  case FTAR_MIN: e = tr_min_max<false>(dt, lds, srcs, k, dst, count, s); break;
  case FTAR_AVG: break;  // refused above
  }
  FTAR_CHECK_HIP(e);
  return FTAR_SUCCESS;
}

}  // namespace ftar

// The kernel the reduce/copy launchers last launched on the calling thread, demangled the way rocprofv3
// prints kernel names ("void ftar::(anonymous namespace)::reduce_lds_kernel<...>(...)"); bench.py
// ties the PMC traffic it reports to this symbol.  Returns the length needed (excluding the NUL), or
// -1 when nothing was launched on this thread.
extern "C" long ftar_debug_last_kernel(char* buf, size_t buflen) {
  const void* k = ftar::g_last_kernel;
  if (!k) return -1;
  const char* raw = hipKernelNameRefByPtr(k, nullptr);
  if (!raw) return -1;
  int status = 0;
  char* dem = abi::__cxa_demangle(raw, nullptr, nullptr, &status);
  const char* name = status == 0 && dem ? dem : raw;
  const size_t need = strlen(name);
  if (buf && buflen) {
    const size_t m = need < buflen - 1 ? need : buflen - 1;
    memcpy(buf, name, m);
    buf[m] = 0;
  }
  free(dem);
  return (long)need;
}
