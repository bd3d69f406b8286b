// The amax finish of f32, bf16 and fp16 (launch_reduce hands every fold with an amax word over; fp8's is in
// reduce_f8.hip): traits and kernels in reduce_impl.h.  A translation unit of its own, as reduce_f8.hip is: its
// kernels are a third set beside the plain and the scaled ones, and side by side a parallel build stays at the
// length it had.
#include "reduce_impl.h"

namespace ftar {

ftar_status_t launch_reduce_amax(const FoldCall& f) {
  switch (f.dt) {
    case FTAR_FLOAT32: return launch_sum<F32Sum, F32Sum, F32Sum, 16, kFinAmax>(f);
    case FTAR_FLOAT16: return launch_sum<F16Sum, F16SumHop, F16SumHopPre, 16, kFinAmax>(f);
    case FTAR_BFLOAT16: return launch_sum<BF16Sum, BF16SumHop, BF16SumHopPre, 16, kFinAmax>(f);
    default: return FTAR_ERR_UNSUPPORTED;
  }
}

}  // namespace ftar
