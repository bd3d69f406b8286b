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

fp8_compress_hook (with Fp8CompressState, at the end of this module) reduces the same buckets on an fp8 wire:
quantize with a power-of-two scale (ftar_cast_scaled, or with rounding="stochastic" ftar_cast_scaled_sr), AllReduce
with op="avg" and amax, dequantize; the scale follows the amax one step behind (next_fp8_scale), on the device.
mx_compress_hook (with MxCompressState) is the block-scaled (MX) form of that wire: one power-of-two scale byte per
32 elements, agreed among the ranks in the same step by a MAX AllReduce of the bytes, so small layers of a bucket
keep their bits and no step overflows the wire; no scale policy to run.  It takes rounding="stochastic" too
(ftar_mx_quantize_sr), with Fp8CompressState's seed and offset.

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


# ---- the fp8 wire ---------------------------------------------------------------------------------------
FP8_MAX = {"e4m3": 448.0, "e5m2": 57344.0}            # the largest finite value of each wire format
_FP8_DTYPE = {"e4m3": "f8e4m3", "e5m2": "f8e5m2"}
_BUCKET_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _pow2(k):
    """2^k as fp32 for an int32 tensor k, clamped to fp32's normal powers of two."""
    return torch.ldexp(torch.ones_like(k, dtype=torch.float32), k.clamp(-126, 127))


def next_fp8_scale(scale, amax, fmt="e4m3", margin=1, backoff=0.5):
    """The scale of the next step from this step's: a pure function of 1-element fp32 tensors on any device, no
    host synchronisation.  `scale` is a power of two and `amax` the abs-max of what was stored on the wire, in
    wire units (scaled values).
      * amax finite and > 0: the largest power of two p with p * (amax / scale) <= FP8_MAX[fmt] * 2^-margin;
      * amax inf or NAN (an overflow on the wire): scale * backoff, rounded down to a power of two;
      * amax 0: scale, unchanged.
    Clamped to fp32's normal powers of two, 2^-126 .. 2^127.  Exact: mantissas and exponents (torch.frexp), never
    a rounded quotient or logarithm."""
    if fmt not in FP8_MAX:
        raise ValueError(f"fmt must be 'e4m3' or 'e5m2', not {fmt!r}")
    target = torch.tensor(FP8_MAX[fmt] * 2.0 ** -int(margin), dtype=torch.float32, device=scale.device)
    finite = torch.isfinite(amax)
    safe = torch.where(finite & (amax > 0), amax, torch.ones_like(amax))
    ma, ea = torch.frexp(safe)                     # amax = ma * 2^ea, ma in [0.5, 1)
    _, es = torch.frexp(scale)                     # scale = 2^(es - 1)
    mt, et = torch.frexp(target)
    # p * ma * 2^(ea - es + 1) <= mt * 2^et, and mt / ma lies in (0.5, 2): its largest power of two is 1 or 1/2
    k = et - (ea - es + 1) - (ma > mt).to(torch.int32)
    grown = _pow2(k)
    _, eb = torch.frexp(scale * backoff)           # a value in [2^(eb - 1), 2^eb)
    backed = _pow2(eb - 1)
    return torch.where(finite, torch.where(amax > 0, grown, scale), backed)


def rank_seed(seed, rank):
    """The 64-bit device seed of one rank: the splitmix64 finaliser of seed + (rank + 1) golden gammas, i.e. the
    (rank + 1)-th output of splitmix64 started at `seed`; so ranks, and neighbouring seeds, get unrelated streams."""
    m = (1 << 64) - 1
    z = (int(seed) + (int(rank) + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


class Fp8CompressState:
    """What fp8_compress_hook needs: the communicator, the wire format ("e4m3" or "e5m2"), optionally a fixed
    topology, and the scale policy's two numbers (next_fp8_scale).  On the first bucket's device it keeps
    `scale` and `inv_scale` (1-element fp32, 1.0 at the start, always powers of two, so scale * inv_scale == 1
    exactly and quantize -> dequantize loses only the fp8 rounding), `amax` (the running maximum over the buckets
    since the last reset_amax(), in WIRE units: the scaled mean as stored in fp8) and a grow-only fp8 wire buffer.
    found_inf() and reset_amax() are HookState's; update_scale(), once per optimizer step, moves the scale on the
    device.  No host synchronisation anywhere.

    rounding="stochastic": the quantize rounds each element to one of its two fp8 neighbours with the expectation
    of the scaled value (ftar_cast_scaled_sr), so its error is zero-mean and averages down over ranks and steps
    where round-to-nearest pushes every rank the same way.  The state then keeps `seed`, a 1-element int64 device
    tensor derived once on the host from (seed, comm.rank) through the splitmix64 finaliser (rank_seed): ranks get
    unrelated streams.  It also keeps `offset`, a host-side count of the elements quantized so far, which grows by
    the bucket's numel per bucket and is never reset, so no two buckets of a run share a word.  Under graph
    capture the offset is baked into the captured kernel: a caller who replays a captured hook must change
    state.seed on the device between replays (e.g. state.seed.add_(1)), or every replay rounds the same way."""

    def __init__(self, comm, fmt="e4m3", topo=None, lonely=0, margin=1, backoff=0.5, rounding="nearest", seed=0):
        if fmt not in FP8_MAX:
            raise ValueError(f"fmt must be 'e4m3' or 'e5m2', not {fmt!r}")
        if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
            raise ValueError(f"margin must be an integer >= 0, not {margin!r}")
        if isinstance(backoff, bool) or not isinstance(backoff, (int, float)) or not 0 < backoff < 1:
            raise ValueError(f"backoff must lie in (0, 1), not {backoff!r}")
        if rounding not in ftar.ROUNDINGS:
            raise ValueError(f"rounding must be 'nearest' or 'stochastic', not {rounding!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an integer, not {seed!r}")
        self.comm, self.fmt, self.topo, self.lonely = comm, fmt, topo, lonely
        self.margin, self.backoff = margin, float(backoff)
        self.rounding, self.base_seed = rounding, seed
        self.seed = None      # stochastic: the rank's device seed, created with the scale
        self.offset = 0
        self.wire_dtype = _FP8_DTYPE[fmt]
        self.scale = self.inv_scale = self.amax = self._bucket_amax = self._wire = None
        self.calls = 0

    def _on(self, device, n):
        if self.scale is None:
            self.scale = torch.ones(1, dtype=torch.float32, device=device)
            self.inv_scale = torch.ones(1, dtype=torch.float32, device=device)
            self.amax = torch.zeros(1, dtype=torch.float32, device=device)
            self._bucket_amax = torch.zeros(1, dtype=torch.float32, device=device)
            if self.rounding == "stochastic":
                word = rank_seed(self.base_seed, getattr(self.comm, "rank", 0))
                self.seed = torch.tensor([word - (1 << 64) if word >> 63 else word], dtype=torch.int64, device=device)
        if self._wire is None or self._wire.numel() < n:
            self._wire = torch.empty(n, dtype=torch.uint8, device=device)
        return self._wire

    def _started(self, what):
        if self.scale is None:
            raise RuntimeError(f"{what} before the first bucket")

    def reset_amax(self):
        """Start a new running maximum (once per optimizer step, after found_inf() and update_scale())."""
        if self.amax is not None:
            self.amax.zero_()

    def found_inf(self):
        """A 1-element fp32 device tensor: 1.0 where `amax` is inf or NAN -- a bucket overflowed the wire at the
        quantize or in a fold, or held a NAN -- else 0.0; no host synchronisation."""
        self._started("found_inf()")
        return (~torch.isfinite(self.amax)).to(torch.float32)

    def update_scale(self):
        """scale = next_fp8_scale(scale, amax, ...), inv_scale = 1 / scale (exact), on the device."""
        self._started("update_scale()")
        self.scale.copy_(next_fp8_scale(self.scale, self.amax, self.fmt, self.margin, self.backoff))
        torch.reciprocal(self.scale, out=self.inv_scale)


def fp8_compress_hook(state, bucket):
    """DDP comm hook: an f32, bf16 or fp16 bucket reduced on an fp8 wire, all on the stream the backward pass runs
    on: (1) the bucket times state.scale, rounded to the wire format (ftar_cast_scaled; with
    state.rounding == "stochastic" ftar_cast_scaled_sr on state.seed at the running state.offset); (2) the wire's in-place
    AllReduce with op="avg" and amax -- the mean is taken inside the last fold, fp32 accumulate and one rounding
    in the one-round forms; (3) the wire times state.inv_scale back into the bucket; (4) state.amax =
    maximum(state.amax, this bucket's amax).  Returns a completed future, as allreduce_hook does.

      * state.amax is in WIRE units: the abs-max of the scaled mean as stored in fp8, not of the gradients.
      * The staged forms round partial sums to fp8 between hops (one rounding per hop or tree node); only the
        one-round forms sum in fp32 and round once.
      * Nothing saturates: an overflow at the quantize or in a fold becomes NAN (e4m3) or inf (e5m2) on the wire,
        reaches state.amax and so found_inf(); the step is then skipped and update_scale() backs the scale off.

    A bucket of any other dtype raises ValueError before any device work."""
    t = bucket.buffer()
    if t.dtype not in _BUCKET_DTYPES:
        raise ValueError(f"fp8_compress_hook takes float32, bfloat16 or float16 buckets, not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("fp8_compress_hook needs a contiguous bucket")
    n = t.numel()
    stream = torch.cuda.current_stream(t.device)
    wire = state._on(t.device, n)
    a = state._bucket_amax
    dt, f8 = ftar._dt(str(t.dtype)), ftar._dt(state.wire_dtype)
    if state.rounding == "stochastic":
        ftar.cast_scaled(t, wire, n, dt, f8, scale=state.scale, stream=stream, rounding="stochastic", seed=state.seed,
                         offset=state.offset)
        state.offset += n
    else:
        ftar.cast_scaled(t, wire, n, dt, f8, scale=state.scale, stream=stream)
    state.comm.allreduce(None, wire, n, f8, "avg", topo_=state.topo, lonely=state.lonely, stream=stream, amax=a)
    ftar.cast_scaled(wire, t, n, f8, dt, scale=state.inv_scale, stream=stream)
    torch.maximum(state.amax, a, out=state.amax)
    state.calls += 1
    fut = torch.futures.Future(devices=[t.device])
    fut.set_result(t)
    return fut


# ---- the MX (block-scaled) fp8 wire ---------------------------------------------------------------------
class MxCompressState:
    """What mx_compress_hook needs: the communicator, the wire format ("e4m3" or "e5m2"), optionally a fixed
    topology, and `headroom` (0..31): the binades left free above each block's peak (ftar_mx_scales).  On the first
    bucket's device it keeps a grow-only fp8 wire buffer, a grow-only uint8 scale buffer (one byte per 32 elements)
    and a 1-element fp32 flag.  found_inf() is 1.0 once any reduced scale byte since reset() was 255 -- a block that
    held an inf or a NaN on some rank -- and stays on the device.  There is no scale policy, no update_scale() and no
    amax: every block's scale is computed from this step's data.  No host synchronisation anywhere.

    rounding="stochastic": step (3) of the hook rounds each scaled element to one of its two fp8 neighbours with the
    expectation of the scaled value (ftar_mx_quantize_sr); the scale bytes, and so steps (1), (2), (4), (5) and
    found_inf(), do not change.  As in Fp8CompressState the state then keeps `seed`, a 1-element int64 device tensor
    derived once on the host from (seed, comm.rank) through rank_seed, and `offset`, a host-side count of the elements
    quantized so far, which grows by the bucket's numel per bucket and is never reset, so no two buckets of a run
    share a word.  Under graph capture the offset is baked into the captured kernel: a caller who replays a captured
    hook must change state.seed on the device between replays (e.g. state.seed.add_(1)), or every replay rounds the
    same way.  The default, "nearest", keeps no seed and stores the bits it always stored."""

    def __init__(self, comm, fmt="e4m3", topo=None, lonely=0, headroom=0, rounding="nearest", seed=0):
        if fmt not in FP8_MAX:
            raise ValueError(f"fmt must be 'e4m3' or 'e5m2', not {fmt!r}")
        if isinstance(headroom, bool) or not isinstance(headroom, int) or not 0 <= headroom <= 31:
            raise ValueError(f"headroom must be an integer in 0..31, not {headroom!r}")
        if rounding not in ftar.ROUNDINGS:
            raise ValueError(f"rounding must be 'nearest' or 'stochastic', not {rounding!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an integer, not {seed!r}")
        self.comm, self.fmt, self.topo, self.lonely, self.headroom = comm, fmt, topo, lonely, headroom
        self.rounding, self.base_seed = rounding, seed
        self.seed = None      # stochastic: the rank's device seed, created on the first bucket's device
        self.offset = 0
        self.wire_dtype = _FP8_DTYPE[fmt]
        self._wire = self._scales = self._inf = None
        self.calls = 0

    def _on(self, device, n):
        if self._inf is None:
            self._inf = torch.zeros(1, dtype=torch.float32, device=device)
            if self.rounding == "stochastic":
                word = rank_seed(self.base_seed, getattr(self.comm, "rank", 0))
                self.seed = torch.tensor([word - (1 << 64) if word >> 63 else word], dtype=torch.int64, device=device)
        if self._wire is None or self._wire.numel() < n:
            self._wire = torch.empty(n, dtype=torch.uint8, device=device)
            self._scales = torch.empty(ftar.mx_nblocks(n), dtype=torch.uint8, device=device)
        return self._wire, self._scales

    def reset(self):
        """Clear the flag (once per optimizer step, after the scaler has read found_inf())."""
        if self._inf is not None:
            self._inf.zero_()

    def found_inf(self):
        """A 1-element fp32 device tensor: 1.0 once a reduced scale byte since reset() was 255, else 0.0."""
        if self._inf is None:
            raise RuntimeError("found_inf() before the first bucket")
        return self._inf


def mx_compress_hook(state, bucket):
    """DDP comm hook: an f32, bf16 or fp16 bucket reduced on an MX wire -- fp8 elements plus one E8M0 scale byte per
    32 -- in five steps, all on the stream the backward pass runs on, no host synchronisation:
    (1) ftar_mx_scales: each block's scale byte from this rank's bucket, state.headroom binades above its peak;
    (2) the bytes' in-place AllReduce of u8 with op="max": every rank now holds each block's largest scale, and 255
        (NaN) wherever any rank's block held an inf or a NaN -- a NaN byte wins the unsigned MAX by itself;
    (3) ftar_mx_quantize with those given scales: two fp8 blocks that share a scale byte sum as plain fp8 values
        (with state.rounding == "stochastic" ftar_mx_quantize_sr on state.seed at the running state.offset);
    (4) the wire's in-place AllReduce with op="avg";
    (5) ftar_mx_dequantize back into the bucket; a block whose byte is 255 comes back all NaN on every rank, and
        state.found_inf() turns 1.0.
    Returns a completed future, as allreduce_hook does.

      * In the one-round forms (the default) the mean of P stored values, each at most the format's maximum, is
        summed in fp32, scaled and rounded once: it cannot overflow at headroom=0.  That holds for a one-stage
        topology ("P"); a multi-stage tree ("2,2") stores its inner nodes in fp8 in every form -- the one-round forms
        reproduce the staged bits -- and two equal peaks under one inner node overflow it at headroom=0.
      * The staged forms round partial sums to fp8 between hops, where a partial sum of up to P values must still fit:
        they need headroom >= ceil(log2 P) (a tree in any form: log2 of the ranks under its largest inner node).
      * The wire costs n + 2 * ceil(n / 32) bytes per rank (payload, and the scale bytes once in each AllReduce)
        against 2n for bf16, and the hook reads the bucket twice (steps 1 and 3).

    Prefer it to fp8_compress_hook when a bucket's layers differ by many binades (at one scale per bucket an e4m3
    element under 2^-10 of the largest is stored as zero) or when a skipped step after an overflow is not acceptable;
    fp8_compress_hook moves fewer bytes and reads the bucket once.
    A bucket that is not float32, bfloat16 or float16, or not contiguous, raises ValueError before any device work."""
    t = bucket.buffer()
    if t.dtype not in _BUCKET_DTYPES:
        raise ValueError(f"mx_compress_hook takes float32, bfloat16 or float16 buckets, not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("mx_compress_hook needs a contiguous bucket")
    n = t.numel()
    nb = ftar.mx_nblocks(n)
    stream = torch.cuda.current_stream(t.device)
    wire, scales = state._on(t.device, n)
    dt, f8 = ftar._dt(str(t.dtype)), ftar._dt(state.wire_dtype)
    ftar.mx_scales(t, scales, n, dt, f8, headroom=state.headroom, stream=stream)
    state.comm.allreduce(None, scales, nb, "u8", "max", topo_=state.topo, lonely=state.lonely, stream=stream)
    if state.rounding == "stochastic":
        ftar.mx_quantize(t, wire, scales, n, dt, f8, mode="given", stream=stream, rounding="stochastic",
                         seed=state.seed, offset=state.offset)
        state.offset += n
    else:
        ftar.mx_quantize(t, wire, scales, n, dt, f8, mode="given", stream=stream)
    state.comm.allreduce(None, wire, n, f8, "avg", topo_=state.topo, lonely=state.lonely, stream=stream)
    ftar.mx_dequantize(wire, scales, t, n, f8, dt, stream=stream)
    torch.maximum(state._inf, (scales[:nb].max() == 255).to(torch.float32).reshape(1), out=state._inf)
    state.calls += 1
    fut = torch.futures.Future(devices=[t.device])
    fut.set_result(t)
    return fut
