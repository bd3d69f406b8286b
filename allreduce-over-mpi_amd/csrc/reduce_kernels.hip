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
// MAX / MIN of one dtype; HOT as the SUM of the same element width
template <bool MAX>
hipError_t min_max(const FoldCall& f) {
  const Launch c = launch_of(f);
  switch (f.dt) {
    case FTAR_UINT8: return launch_tr<MinMax<unsigned char, MAX>, 8>(c, f.count, f.lds);
    case FTAR_INT8: return launch_tr<MinMax<signed char, MAX>, 8>(c, f.count, f.lds);
    case FTAR_UINT16: return launch_tr<MinMax<unsigned short, MAX>, 8>(c, f.count, f.lds);
    case FTAR_INT16: return launch_tr<MinMax<short, MAX>, 8>(c, f.count, f.lds);
    case FTAR_INT32: return launch_tr<MinMax<int, MAX>, 8>(c, f.count, f.lds);
    case FTAR_INT64: return launch_tr<MinMax<long long, MAX>, 8>(c, f.count, f.lds);
    case FTAR_FLOAT32: return launch_tr<MinMax<float, MAX>, 16>(c, f.count, f.lds);
    case FTAR_FLOAT64: return launch_tr<MinMax<double, MAX>, 8>(c, f.count, f.lds);
    case FTAR_BFLOAT16: return launch_tr<BF16MinMax<MAX>, 16>(c, f.count, f.lds);
    case FTAR_FLOAT16: return launch_tr<MinMax<_Float16, MAX>, 16>(c, f.count, f.lds);
    case FTAR_FLOAT8_E4M3: case FTAR_FLOAT8_E5M2: break;  // launch_reduce_f8
    case FTAR_BOOL: break;
  }
  return hipErrorInvalidValue;
}
// The float sums (fp8's: reduce_f8.hip) in the plain or the scaled finish (AVG's root folds, ftar_reduce_scaled)
template <int SC>
ftar_status_t float_sum(const FoldCall& f) {
  switch (f.dt) {
    case FTAR_FLOAT32: return launch_sum<F32Sum, F32Sum, F32Sum, 16, SC>(f);
    case FTAR_FLOAT64: return launch_sum<F64Sum, F64Sum, F64Sum, 8, SC, false>(f);
    case FTAR_FLOAT16: return launch_sum<F16Sum, F16SumHop, F16SumHopPre, 16, SC>(f);
    default: return launch_sum<BF16Sum, BF16SumHop, BF16SumHopPre, 16, SC>(f);
  }
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
  FTAR_CHECK_HIP((launch_lds<U8Sum, 1, 1, 1>(Launch{srcs, 1, dst, s}, sp)));
  return FTAR_SUCCESS;
}

ftar_status_t launch_reduce(const FoldCall& f) {
  if (f.k < 1 || f.k > FTAR_MAX_K || !f.srcs || !f.dst) return FTAR_ERR_INVALID_ARG;
  if (f.op == FTAR_AVG || !dtype_op_supported(f.dt, f.op)) return FTAR_ERR_UNSUPPORTED;  // AVG: the engine's SUM + scale
  if (f.scale && (f.op != FTAR_SUM || !dtype_scalable(f.dt))) return FTAR_ERR_UNSUPPORTED;
  if (f.amax && (!f.scale || !dtype_has_amax(f.dt))) return FTAR_ERR_UNSUPPORTED;
  if (f.count == 0) return FTAR_SUCCESS;
  for (int j = 0; j < f.k; ++j)
    if (!f.srcs[j]) return FTAR_ERR_INVALID_ARG;
  if (f.dt == FTAR_FLOAT8_E4M3 || f.dt == FTAR_FLOAT8_E5M2) return launch_reduce_f8(f);  // every fp8 fold: reduce_f8.hip
  if (f.amax) return launch_reduce_amax(f);  // the amax finish of f32, bf16 and fp16: reduce_amax.hip
  // a scaled k = 1 is a scaled copy through the runtime-k kernel; a plain one is a copy
  if (f.scale) return float_sum<kFinScaled>(f);
  if (f.k == 1)  // vector_add/reduce_sum.h:36-47: a copy (a streaming kernel, not the DMA blit)
    return launch_copy(f.srcs[0], f.dst, f.count * dtype_size(f.dt), f.stream);
  if (f.op == FTAR_SUM && dtype_scalable(f.dt)) return float_sum<kFinPlain>(f);
  const Launch c = launch_of(f);
  hipError_t e = hipErrorInvalidValue;
  switch (f.op) {
  case FTAR_SUM:
    switch (f.dt) {
      case FTAR_FLOAT32: case FTAR_FLOAT64: case FTAR_BFLOAT16: case FTAR_FLOAT16: break;  // float_sum above
      case FTAR_FLOAT8_E4M3: case FTAR_FLOAT8_E5M2: break;  // launch_reduce_f8 above
      case FTAR_UINT8: case FTAR_INT8: e = launch_tr<U8Sum, 8>(c, f.count, f.lds); break;
      case FTAR_UINT16: case FTAR_INT16: e = launch_tr<U16Sum, 8>(c, f.count, f.lds); break;
      case FTAR_INT32: e = launch_tr<U32Sum, 8>(c, f.count, f.lds); break;
      case FTAR_INT64: e = launch_tr<U64Sum, 8>(c, f.count, f.lds); break;
      case FTAR_BOOL: e = launch_tr<BoolSum, 8>(c, f.count, f.lds); break;
    }
    break;
  case FTAR_BAND:
    switch (f.dt) {
      case FTAR_UINT8: case FTAR_INT8: e = launch_tr<Band<unsigned char>, 8>(c, f.count, f.lds); break;
      case FTAR_UINT16: case FTAR_INT16: e = launch_tr<Band<unsigned short>, 8>(c, f.count, f.lds); break;
      case FTAR_INT32: e = launch_tr<Band<unsigned>, 8>(c, f.count, f.lds); break;
      case FTAR_INT64: e = launch_tr<Band<unsigned long long>, 8>(c, f.count, f.lds); break;
      default: return FTAR_ERR_UNSUPPORTED;
    }
    break;
  case FTAR_MAX: e = min_max<true>(f); break;
  case FTAR_MIN: e = min_max<false>(f); break;
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
