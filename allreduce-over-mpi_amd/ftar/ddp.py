"""ftar as the gradient AllReduce of torch DistributedDataParallel (a DDP communication hook).

The data-parallel caller of the hot path: DDP packs gradients into buckets and hands each bucket to a hook
once its gradients are ready; the hook below reduces the bucket in place with ftar_allreduce on the stream the
backward pass runs on (the FlexTree schedule of FT_TOPO / FT_LONELY or `topo`, else the cost model; RCCL p2p
over xGMI, the reduce kernel on ftar's own stream).  No host synchronisation: the AllReduce and every later
use of the bucket are ordered on that stream.

The mean, two ways (HookState's `average`):

  * "divide" (the default): the bucket is divided by the world size first, as DDP's own allreduce hook does,
    then summed, so the mean rounds as DDP's does and keeps its overflow headroom in every form.  The division
    is a torch kernel of its own: one more read and write of the whole bucket, and one more rounding per
    element of an fp16 / bf16 bucket.
  * "fused": no division; the AllReduce runs op="avg" (FTAR_AVG, include/ftar.h), which multiplies by 1 / P
    inside the last fold of each block, where the sum still sits in its fp32 accumulator.  In the one-round
    forms (the default) the P copies are summed in fp32, scaled and rounded once: one rounding instead of
    P + 1, and an fp16 mean stays finite where the fp16 sum would be inf.  The staged 16-bit forms round
    partial sums between hops, so there a partial sum can overflow: they lose the pre-division's headroom.

    comm = ftar.dist.init_comm()                       # one rank per GPU, RCCL over the DDP process group's ids
    model = DistributedDataParallel(model, device_ids=[local_rank])
    model.register_comm_hook(ftar.ddp.HookState(comm), ftar.ddp.allreduce_hook)

The bucket's dtype is the tensor's own: fp32, bf16 and fp16 gradient buckets all work (mixed-precision
training, or DDP's fp16 / bf16 compression wrappers around this hook).  The 16-bit sums accumulate in fp32 and
round once per reduce call (include/ftar.h); an fp16 sum that overflows becomes inf, which a loss scaler sees.
What such training needs next to the sum -- an overflow flag for the loss scaler, the inf-norm for clipping,
the amax of delayed fp8 scaling -- comes out of the same AllReduce: with `track_amax=True` the hook calls
ftar_allreduce_amax, whose last fold of each block also keeps the largest |value| it stores (no pass of
`torch.isfinite(bucket).all()` or `bucket.abs().max()` over the bucket), and the state keeps the running
maximum over the buckets in `state.amax`; `state.found_inf()` is the GradScaler-style flag, on the device.
Values of the caller's own (a loss scale to agree on) still go through `comm.allreduce_tensor(t, op="max")` /
`op="min"`.

The reference reduces MPI buffers (MPI_Allreduce_FT, mpi_mod.hpp:1723-1778); a DDP bucket is the same call on
a device tensor, in place (`sendbuf = MPI_IN_PLACE`).
"""
import torch

import ftar


class HookState:
    """What the hook needs: the ftar communicator, optionally a fixed topology (FT_TOPO syntax), and how the
    mean is taken: average="divide" (div_ by the world size, then op="sum") or "fused" (op="avg": no division
    pass; rounded once in the one-round forms and no overflow there, but the staged 16-bit forms round partial
    sums between hops and lose the pre-division's headroom).
    track_amax=True: every bucket goes through ftar_allreduce_amax (with average="divide" the div_ stays and the
    op is SUM), and `amax`, a 1-element fp32 tensor on the bucket's device, holds the torch.maximum of the reduced
    buckets' abs-max since the last reset_amax() -- NAN once a bucket held a NAN, inf once one overflowed; the
    same on every rank.  found_inf() is 1.0 where it is not finite.  No host synchronisation anywhere."""

    def __init__(self, comm, topo=None, lonely=0, average="divide", track_amax=False):
        if average not in ("divide", "fused"):
            raise ValueError(f"average must be 'divide' or 'fused', not {average!r}")
        if not isinstance(track_amax, bool):
            raise ValueError(f"track_amax must be True or False, not {track_amax!r}")
        self.comm, self.topo, self.lonely, self.average = comm, topo, lonely, average
        self.track_amax = track_amax
        self.amax = None      # created on the first bucket's device
        self._bucket_amax = None
        self.calls = 0

    def _amax_on(self, device):
        if self.amax is None:
            self.amax = torch.zeros(1, dtype=torch.float32, device=device)
            self._bucket_amax = torch.zeros(1, dtype=torch.float32, device=device)
        return self._bucket_amax

    def reset_amax(self):
        """Start a new running maximum (e.g. once per optimizer step, after the scaler has read found_inf())."""
        if self.amax is not None:
            self.amax.zero_()

    def found_inf(self):
        """A 1-element fp32 device tensor: 1.0 where `amax` is inf or NAN, else 0.0 (what GradScaler keeps per
        optimizer); computed on the device, no host synchronisation."""
        if not self.track_amax:
            raise RuntimeError("found_inf() needs HookState(..., track_amax=True)")
        if self.amax is None:
            raise RuntimeError("found_inf() before the first bucket")
        return (~torch.isfinite(self.amax)).to(torch.float32)


def allreduce_hook(state, bucket):
    """DDP comm hook: the bucket / world size (first, as torch's default hook divides before it reduces), then
    its in-place FlexTree AllReduce -- or, with average="fused", the AllReduce alone with op="avg"; returns a
    completed future whose tensor the reducer copies back into the gradients on the same stream."""
    t = bucket.buffer()
    stream = torch.cuda.current_stream(t.device)
    fused = state.average == "fused"
    if not fused:
        t.div_(state.comm.nranks)
    if state.track_amax:
        a = state._amax_on(t.device)
        state.comm.allreduce(None, t, t.numel(), ftar._dt(str(t.dtype)), "avg" if fused else "sum",
                             topo_=state.topo, lonely=state.lonely, stream=stream, amax=a)
        torch.maximum(state.amax, a, out=state.amax)   # NAN-propagating, on the same stream
    else:
        state.comm.allreduce(None, t, t.numel(), ftar._dt(str(t.dtype)), "avg" if fused else "sum",
                             topo_=state.topo, lonely=state.lonely, stream=stream)
    state.calls += 1
    fut = torch.futures.Future(devices=[t.device])
    fut.set_result(t)
    return fut
