"""fp16 SUM and the MAX / MIN reductions on the GPU, from the kernel (ftar_reduce, ftar_reduce_nested) through
the engine's AllReduce (every topology and form, pieces, peer-direct, host buffers) to the Python surface
(allreduce_tensor, the DDP hook, the RCCL yardstick).  Neither extension has a reference or an oracle entry:
the expectations are the independent CPU implementations of tests/f16_minmax_ref.py (torch's fp32 adds and
float -> half conversion per schedule; integer-key MAX / MIN), compared bit for bit, NaN lanes as NaN or not.

Sizes are the smallest that still reach every path: n = 1 (head only), 255 (head/tail, no full tile),
4099 and 100 003 (full tiles of every (U, W) shape plus a partial tile, several workgroups); k crosses the
LDS-staged kernels (2..8, 2..16 for f32 and the 16-bit floats) and the runtime-k register kernel (9, 17, 33)."""
import ctypes

import numpy as np
import pytest

import f16_minmax_ref as ref
from gpu_util import filled_dev, from_dev, to_dev

pytestmark = pytest.mark.gpu

_groups = {}


def group(P):
    import ftar
    if P not in _groups:
        _groups[P] = ftar.Comm.init_local(P)
    return _groups[P]


def check(dt, got, want, what=""):
    assert ref.same_bits(dt, got, want), (what, ref.first_diff(dt, got, want))


def run_reduce(ins, dt, op, offsets=None, out_offset=0, inplace=False, shape=None):
    import ftar
    n = ins[0].size
    offsets = offsets or [0] * len(ins)
    devs = [to_dev(x, offset_elems=o) for x, o in zip(ins, offsets)]
    esz = ins[0].dtype.itemsize
    if inplace:
        dst_t, dst = devs[0]
        out_offset = offsets[0]
    else:
        dst_t, dst = filled_dev((n + out_offset) * esz)
        dst += out_offset * esz
    ftar.reduce([p for _, p in devs], dst, n, dt, op, shape=shape)
    return from_dev(dst_t, ins[0].dtype, n, out_offset)


# ---- ftar_reduce ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 4099, 100_003])
@pytest.mark.parametrize("k", [2, 3, 8, 9, 16, 17, 33])
def test_reduce_f16_sum_is_torch_fp32_fold_rounded_once(k, n):
    ins, want = ref.f16_fold_case(k, n)
    check("f16", run_reduce(ins, "f16", "sum"), want)


@pytest.mark.parametrize("n", [1, 255, 100_003])
@pytest.mark.parametrize("k", [2, 3, 8, 9, 17])
@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("dt", ref.MINMAX_DTYPES)
def test_reduce_max_min(dt, op, k, n):
    ins, want = ref.minmax_case(dt, op, k, n)
    check(dt, run_reduce(ins, dt, op), want)


def _expect(dt, op, ins):
    return ref.f16_fold(ins) if op == "sum" else ref.minmax(dt, op, ins)


@pytest.mark.parametrize("offs,out_off", [([1, 1], 1), ([0, 1], 0), ([2, 0, 1], 3)])
@pytest.mark.parametrize("dt,op", [("f16", "sum"), ("f16", "max"), ("i8", "min"), ("f64", "max")])
def test_reduce_unaligned(dt, op, offs, out_off):
    """Co-aligned offsets (vector path with an unaligned head and a short tail) and sources whose alignment
    differs from the destination's (the element-wise kernel)."""
    ins = ref.sources(dt, len(offs), 33_333)
    check(dt, run_reduce(ins, dt, op, offsets=offs, out_offset=out_off), _expect(dt, op, ins))


@pytest.mark.parametrize("dt,op", [("f16", "sum"), ("bf16", "max")])
def test_reduce_in_place(dt, op):
    """dst == srcs[0], the ring's in-place fold."""
    ins = ref.sources(dt, 3, 100_003)
    check(dt, run_reduce(ins, dt, op, inplace=True), _expect(dt, op, ins))


# ---- ftar_reduce_nested ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2), (2, 4), (4, 2), (2, 2, 2), (2, 3)])
def test_reduce_nested_f16_rounds_every_inner_node(shape):
    """The one-round tree reduce-scatter's fold: compile-time shapes on the LDS-staged kernel and a
    runtime-coded one (2,3) on the register kernel, against the per-node torch fold."""
    ins = ref.sources("f16", int(np.prod(shape)), 50_001)
    check("f16", run_reduce(ins, "f16", "sum", shape=list(shape)), ref.f16_nested(ins, shape))


def test_reduce_nested_max_is_the_flat_result():
    ins, want = ref.minmax_case("f32", "max", 8, 100_003)
    got = run_reduce(ins, "f32", "max", shape=[2, 2, 2])
    check("f32", got, want)
    assert got.tobytes() == run_reduce(ins, "f32", "max").tobytes()


def test_f16_conversions_match_integer_code_on_every_bit_pattern():
    """The production fp32 -> fp16 rounding over all 2^32 floats against an integer round-to-nearest-even,
    and the widening over all 2^16 halves against an integer expansion (ftar_debug_f16_cvt_check)."""
    import ftar
    lib = ftar.bench_lib()
    lib.ftar_debug_f16_cvt_check.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint)]
    bad, first = (ctypes.c_ulonglong * 2)(), (ctypes.c_uint * 2)()
    assert lib.ftar_debug_f16_cvt_check(bad, first) == 0
    assert bad[0] == 0, f"narrowing: {bad[0]} float patterns differ, first 0x{first[0]:08x}"
    assert bad[1] == 0, f"widening: {bad[1]} half patterns differ, first 0x{first[1]:04x}"


# ---- AllReduce on in-process groups ---------------------------------------------------------------------
N = 50_001
TOPOS = [(2, "1"), (4, "1"), (8, "1"), (8, "8"), (4, "2,2"), (8, "2,4"), (8, "2,2,2")]
LONELY = [(5, "2,2", 1), (8, "3,2", 2)]


def run_group(ins, topo, dt, op, lonely=0, form="direct", chunk_bytes=0):
    g = group(len(ins))
    g.set_chunk_bytes(chunk_bytes)
    g.set_allgather(form)
    g.set_reduce_scatter(form)
    n = ins[0].size
    bufs = [to_dev(x) for x in ins]
    g.allreduce(None, [p for _, p in bufs], n, dt, op, topo_=topo, lonely=lonely)
    return [from_dev(t, ins[0].dtype, n) for t, _ in bufs]


@pytest.mark.parametrize("chunk_bytes", [0, 512])
@pytest.mark.parametrize("form", ["stages", "direct"])
@pytest.mark.parametrize("P,topo", TOPOS)
def test_allreduce_f16_sum_is_the_schedules_torch_fold(P, topo, form, chunk_bytes):
    """Ring: one rounding per hop (staged hops, or the one-round fold with round_each); trees: one rounding
    per node (staged, or the nested fold).  Every rank, against the fold written out in torch."""
    ins, want = ref.f16_allreduce_case(P, topo, N)
    outs = run_group(ins, topo, "f16", "sum", form=form, chunk_bytes=chunk_bytes)
    for r in range(P):
        check("f16", outs[r], want, f"rank {r}")


@pytest.mark.parametrize("chunk_bytes", [0, 512])
@pytest.mark.parametrize("form", ["stages", "direct"])
@pytest.mark.parametrize("P,topo,lonely", LONELY)
def test_allreduce_f16_sum_lonely_layouts(P, topo, lonely, form, chunk_bytes):
    """Integer-valued inputs in [-8, 8]: every association is exact in fp16, so the plain sum is expected."""
    ins, want = ref.exact_sum_case("f16", P, N)
    outs = run_group(ins, topo, "f16", "sum", lonely=lonely, form=form, chunk_bytes=chunk_bytes)
    for r in range(P):
        check("f16", outs[r], want, f"rank {r}")


@pytest.mark.parametrize("P,topo,lonely", [(P, t, 0) for P, t in TOPOS] + LONELY)
@pytest.mark.parametrize("dt,op", [("f32", "max"), ("i8", "min"), ("bf16", "max")])
def test_allreduce_max_min_every_topology_and_form(dt, op, P, topo, lonely):
    """Exact and associative: every rank holds the flat CPU expectation, whatever the schedule, the form
    and the piece size."""
    ins, want = ref.minmax_case(dt, op, P, N)
    first = None
    for form in ("stages", "direct"):
        for chunk_bytes in (0, 512):
            outs = run_group(ins, topo, dt, op, lonely=lonely, form=form, chunk_bytes=chunk_bytes)
            for r in range(P):
                check(dt, outs[r], want, (form, chunk_bytes, r))
            first = outs[0] if first is None else first
            for r in range(P):   # and the same across forms and piece sizes (NaN lanes: NaN, payload open)
                check(dt, outs[r], first, (form, chunk_bytes, r, "vs stages / one piece"))


@pytest.mark.parametrize("mode", ["read", "write"])
@pytest.mark.parametrize("dt,op", [("f16", "sum"), ("f32", "max")])
def test_allreduce_peer_direct(dt, op, mode):
    P, topo = 4, "2,2"
    if op == "sum":
        ins, want = ref.f16_allreduce_case(P, topo, N)
    else:
        ins, want = ref.minmax_case(dt, op, P, N)
    g = group(P)
    g.set_peer_direct(mode)
    try:
        outs = run_group(ins, topo, dt, op)
    finally:
        g.set_peer_direct(False)
    for r in range(P):
        check(dt, outs[r], want, f"rank {r}")


def test_allreduce_host_buffers_f16_sum():
    """ftar_allreduce_host on pinned host buffers, P = 2 ring."""
    import torch
    P = 2
    ins, want = ref.f16_allreduce_case(P, "1", N)
    g = group(P)
    g.set_host_chunk_bytes(0)
    g.set_allgather("direct")
    g.set_reduce_scatter("direct")
    bufs = [torch.from_numpy(x.view(np.uint8).copy()).pin_memory() for x in ins]
    g.allreduce(None, bufs, N, "f16", "sum", topo_="1", host=True)
    for r in range(P):
        check("f16", bufs[r].numpy().view(np.uint16)[:N], want, f"rank {r}")


# ---- Python surface -------------------------------------------------------------------------------------
def test_allreduce_tensor_float16_and_max():
    """Comm.allreduce_tensor takes dtype and count from the tensor: a torch.float16 bucket, and op="max"."""
    import threading

    import torch
    P, topo = 4, "2,2"
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather("direct")
    g.set_reduce_scatter("direct")

    def run(tensors, op):
        errs = []

        def rank(r):
            try:
                assert g[r].allreduce_tensor(tensors[r], op=op, topo_=topo) is tensors[r]
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs

    ins, want = ref.f16_allreduce_case(P, topo, N)
    ts = [torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.float16) for x in ins]
    run(ts, "sum")
    for r in range(P):
        check("f16", ts[r].view(torch.int16).cpu().numpy(), want, f"rank {r}")
    ins, want = ref.minmax_case("f32", "max", P, N)
    ts = [torch.from_numpy(x.view(np.float32).copy()).cuda() for x in ins]
    run(ts, "max")
    for r in range(P):
        check("f32", ts[r].view(torch.int32).cpu().numpy(), want, f"rank {r}")


def test_ddp_hook_takes_an_fp16_bucket_and_rccl_yardstick_knows_the_extensions():
    """A one-rank RCCL communicator: the DDP hook on a stand-in bucket whose buffer is an fp16 CUDA tensor
    returns it unchanged (/ 1, then a one-rank AllReduce); ftar_rccl_allreduce with f16 / sum and f32 / max
    returns its input."""
    import torch

    import ftar
    import ftar.ddp

    class Bucket:
        def __init__(self, t):
            self.t = t

        def buffer(self):
            return self.t

    comm = ftar.Comm.init_rank(1, ftar.get_unique_id(), 0, 0)
    try:
        x = ref.sources("f16", 2, 4099, small_ints=True)[0]
        t = torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.float16)
        state = ftar.ddp.HookState(comm)
        fut = ftar.ddp.allreduce_hook(state, Bucket(t))
        out = fut.wait()
        torch.cuda.synchronize()
        assert out is t and state.calls == 1
        assert np.array_equal(t.view(torch.int16).cpu().numpy().view(np.uint16), x)

        for dt, op, src in (("f16", "sum", x), ("f32", "max", ref.sources("f32", 2, 4099, small_ints=True)[0])):
            s, sp = to_dev(src)
            d, dp = filled_dev(src.nbytes)
            comm.rccl_allreduce(sp, dp, src.size, dt, op)
            assert np.array_equal(from_dev(d, src.dtype, src.size), src), (dt, op)
    finally:
        comm.destroy()
