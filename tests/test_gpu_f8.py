"""The two OCP fp8 dtypes (f8e4m3, f8e5m2) on the GPU, from the kernel (ftar_reduce, ftar_reduce_nested,
ftar_reduce_scaled) through the engine's AllReduce (every topology and form, pieces, peer-direct, host buffers,
AVG) to the Python surface (allreduce_tensor, the RCCL yardstick).  There is no reference and no oracle entry:
the expectations are the independent CPU implementations of tests/f8_ref.py (torch's fp32 adds and float32 ->
float8 cast per schedule; integer-key MAX / MIN), compared bit for bit, NaN lanes as NaN or not.

Sizes are the smallest that still reach every path: n = 1 (head only), 15 (no full vector), 255 (vectors, no
full tile), 4099 and 100 003 (full tiles of every (U, W) shape plus a partial one, several workgroups); k
crosses the LDS-staged kernels (2..8) and the runtime-k register kernel (9, 16, 17, 33)."""
import ctypes

import numpy as np
import pytest

import f8_ref as ref
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


def run_reduce(ins, dt, op, offsets=None, out_offset=0, inplace=False, shape=None, scale=None):
    import ftar
    n = ins[0].size
    offsets = offsets or [0] * len(ins)
    devs = [to_dev(x, offset_elems=o) for x, o in zip(ins, offsets)]
    if inplace:
        dst_t, dst = devs[0]
        out_offset = offsets[0]
    else:
        dst_t, dst = filled_dev(n + out_offset)
        dst += out_offset
    ftar.reduce([p for _, p in devs], dst, n, dt, op, shape=shape, scale=scale)
    return from_dev(dst_t, np.uint8, n, out_offset)


# ---- ftar_reduce ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 255, 4099, 100_003])
@pytest.mark.parametrize("k", [2, 3, 8, 9, 16, 17, 33])
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_reduce_sum_is_torch_fp32_fold_rounded_once(dt, k, n):
    ins, want = ref.fold_case(dt, k, n)
    check(dt, run_reduce(ins, dt, "sum"), want)


@pytest.mark.parametrize("n", [1, 255, 100_003])
@pytest.mark.parametrize("k", [2, 3, 8, 9, 17])
@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_reduce_max_min(dt, op, k, n):
    ins, want = ref.minmax_case(dt, op, k, n)
    got = run_reduce(ins, dt, op)
    check(dt, got, want)
    ok = ~ref.nan_mask(dt, want)                 # a non-NaN result is one of the sources bit for bit
    assert np.logical_or.reduce([got == x for x in ins])[ok].all()


def _expect(dt, op, ins):
    return ref.fold(dt, ins) if op == "sum" else ref.minmax(dt, op, ins)


@pytest.mark.parametrize("offs,out_off", [([1, 1], 1), ([0, 1], 0), ([2, 0, 1], 3)])
@pytest.mark.parametrize("dt,op", [("f8e4m3", "sum"), ("f8e5m2", "sum"), ("f8e4m3", "max"), ("f8e5m2", "min")])
def test_reduce_unaligned(dt, op, offs, out_off):
    """Co-aligned offsets (vector path with an unaligned head and a short tail) and sources whose alignment
    differs from the destination's (the element-wise kernel)."""
    ins = ref.sources(dt, len(offs), 33_333)
    check(dt, run_reduce(ins, dt, op, offsets=offs, out_offset=out_off), _expect(dt, op, ins))


@pytest.mark.parametrize("dt,op", [("f8e4m3", "sum"), ("f8e5m2", "sum"), ("f8e5m2", "max")])
def test_reduce_in_place(dt, op):
    """dst == srcs[0], the ring's in-place fold."""
    ins = ref.sources(dt, 3, 100_003)
    check(dt, run_reduce(ins, dt, op, inplace=True), _expect(dt, op, ins))


# ---- ftar_reduce_nested, ftar_reduce_scaled -------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2), (2, 4), (4, 2), (2, 2, 2), (2, 3)])
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_reduce_nested_rounds_every_inner_node(dt, shape):
    """Compile-time shapes on the LDS-staged kernel and a runtime-coded one (2,3) on the register kernel,
    against the per-node torch fold."""
    ins = ref.sources(dt, int(np.prod(shape)), 50_001)
    check(dt, run_reduce(ins, dt, "sum", shape=list(shape)), ref.nested(dt, ins, shape))


@pytest.mark.parametrize("dt", ref.FORMATS)
def test_reduce_nested_max_is_the_flat_result(dt):
    ins, want = ref.minmax_case(dt, "max", 8, 100_003)
    got = run_reduce(ins, dt, "max", shape=[2, 2, 2])
    check(dt, got, want)
    assert got.tobytes() == run_reduce(ins, dt, "max").tobytes()


@pytest.mark.parametrize("shape", [None, (2, 2)])
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_reduce_scaled_scales_before_the_one_rounding(dt, shape):
    """ftar.reduce(..., scale=) flat and nested (2,2) with scale 1/4.  Lane 21 is max + max: the plain sum
    overflows (e4m3: NaN, e5m2: inf) and the scaled result is finite -- flat, where the fp32 accumulator
    holds 2 max; nested (2,2) rounds the pair's node first, so the overflow stands."""
    ins = ref.sources(dt, 4, 50_001)
    r = ref.scale_of(0.25)
    want = ref.nested(dt, ins, shape, r) if shape else ref.fold(dt, ins, r)
    got = run_reduce(ins, dt, "sum", shape=list(shape) if shape else None, scale=0.25)
    check(dt, got, want)
    over = 0x7F if dt == "f8e4m3" else 0x7C
    assert (ref.fold(dt, ins)[21] & 0x7F) == over
    if shape is None:
        assert got[21] == ref.encode(dt, [2 * (448.0 if dt == "f8e4m3" else 57344.0) / 4])[0]
    else:
        assert (got[21] & 0x7F) == over


@pytest.mark.parametrize("k", [2, 8])
def test_the_integer_key_max_variant_gives_the_same_bits(k):
    """The other formulation of MAX (F8KeyMinMax, kept as an A/B variant in libftar_bench.so: dtype code
    300 + e4m3, variant 62 = the production shape), vectors and the partial tile."""
    import ftar
    lib = ftar.bench_lib()
    lib.ftar_debug_reduce_variant.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    n = 16 * 6251
    ins, want = ref.minmax_case("f8e4m3", "max", k, n)
    devs = [to_dev(x) for x in ins]
    dst_t, dst = filled_dev(n)
    arr = (ctypes.c_void_p * k)(*[p for _, p in devs])
    assert lib.ftar_debug_reduce_variant(62, 300 + ftar.DTYPE["f8e4m3"], arr, k, dst, n, None) == 0
    check("f8e4m3", from_dev(dst_t, np.uint8, n), want)


def test_f8_conversions_match_integer_code_on_every_bit_pattern():
    """The production fp32 -> fp8 narrowing of both formats over all 2^32 floats against the integer RNE (the
    function tests/test_f8_api.py holds against torch's cast), and the widening over all 2^8 bytes against an
    integer expansion (ftar_debug_f8_cvt_check)."""
    import ftar
    lib = ftar.bench_lib()
    lib.ftar_debug_f8_cvt_check.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint)]
    bad, first = (ctypes.c_ulonglong * 4)(), (ctypes.c_uint * 4)()
    assert lib.ftar_debug_f8_cvt_check(bad, first) == 0
    for i, what in enumerate(("narrowing to e4m3", "narrowing to e5m2", "widening e4m3", "widening e5m2")):
        assert bad[i] == 0, f"{what}: {bad[i]} patterns differ, first 0x{first[i]:08x}"


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
    return [from_dev(t, np.uint8, n) for t, _ in bufs]


@pytest.mark.parametrize("chunk_bytes", [0, 512])
@pytest.mark.parametrize("form", ["stages", "direct"])
@pytest.mark.parametrize("P,topo", TOPOS)
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_allreduce_sum_is_the_schedules_torch_fold(dt, P, topo, form, chunk_bytes):
    """Ring: one rounding per hop (staged hops, or the one-round fold with round_each); trees: one rounding
    per node (staged, or the nested fold).  Every rank, against the fold written out in torch."""
    ins, want = ref.allreduce_case(dt, P, topo, N)
    outs = run_group(ins, topo, dt, "sum", form=form, chunk_bytes=chunk_bytes)
    for r in range(P):
        check(dt, outs[r], want, f"rank {r}")


@pytest.mark.parametrize("chunk_bytes", [0, 512])
@pytest.mark.parametrize("form", ["stages", "direct"])
@pytest.mark.parametrize("P,topo,lonely", LONELY)
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_allreduce_sum_lonely_layouts(dt, P, topo, lonely, form, chunk_bytes):
    """Integer-valued inputs in [-2, 2]: every association is exact, so the plain sum is expected."""
    ins, want = ref.exact_sum_case(dt, P, N)
    outs = run_group(ins, topo, dt, "sum", lonely=lonely, form=form, chunk_bytes=chunk_bytes)
    for r in range(P):
        check(dt, outs[r], want, f"rank {r}")


@pytest.mark.parametrize("P,topo,lonely", [(P, t, 0) for P, t in TOPOS] + LONELY)
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_allreduce_max_every_topology_and_form(dt, P, topo, lonely):
    """Exact and associative: every rank holds the flat CPU expectation, whatever the schedule, the form
    and the piece size."""
    ins, want = ref.minmax_case(dt, "max", P, N)
    first = None
    for form in ("stages", "direct"):
        for chunk_bytes in (0, 512):
            outs = run_group(ins, topo, dt, "max", lonely=lonely, form=form, chunk_bytes=chunk_bytes)
            for r in range(P):
                check(dt, outs[r], want, (form, chunk_bytes, r))
            first = outs[0] if first is None else first
            for r in range(P):   # and the same across forms and piece sizes (NaN lanes: NaN, payload open)
                check(dt, outs[r], first, (form, chunk_bytes, r, "vs stages / one piece"))


@pytest.mark.parametrize("form", ["direct", "stages"])
@pytest.mark.parametrize("P,topo", [(4, "2,2"), (8, "8"), (8, "1")])
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_allreduce_avg(dt, P, topo, form):
    """SUM's schedule with the root fold of each block scaled by 1.0f / P before its rounding.  Lane 21 holds
    max + max: in the one-round forms of a tree the e4m3 mean is finite where the e4m3 sum is NaN; where a
    staged hop or an inner node rounds the pair first, the overflow stands -- the expectation says which."""
    ins, want = ref.allreduce_case(dt, P, topo, N, avg=True)
    outs = run_group(ins, topo, dt, "avg", form=form)
    for r in range(P):
        check(dt, outs[r], want, f"rank {r}")
    if dt == "f8e4m3" and topo == "8":       # one node of 8: 2 x 448 / 8 = 112, under SUM a NaN
        assert ref.nan_mask(dt, ref.allreduce_case(dt, P, topo, N)[1])[21]
        assert outs[0][21] == ref.encode(dt, [112.0])[0]


@pytest.mark.parametrize("mode", ["read", "write"])
@pytest.mark.parametrize("dt,op", [("f8e4m3", "sum"), ("f8e5m2", "sum"), ("f8e4m3", "max")])
def test_allreduce_peer_direct(dt, op, mode):
    P, topo = 4, "2,2"
    ins, want = ref.allreduce_case(dt, P, topo, N) if op == "sum" else ref.minmax_case(dt, op, P, N)
    g = group(P)
    g.set_peer_direct(mode)
    try:
        outs = run_group(ins, topo, dt, op)
    finally:
        g.set_peer_direct(False)
    for r in range(P):
        check(dt, outs[r], want, f"rank {r}")


@pytest.mark.parametrize("dt", ref.FORMATS)
def test_allreduce_host_buffers_sum(dt):
    """ftar_allreduce_host on pinned host buffers, P = 2 ring."""
    import torch
    P = 2
    ins, want = ref.allreduce_case(dt, P, "1", N)
    g = group(P)
    g.set_host_chunk_bytes(0)
    g.set_allgather("direct")
    g.set_reduce_scatter("direct")
    bufs = [torch.from_numpy(x.copy()).pin_memory() for x in ins]
    g.allreduce(None, bufs, N, dt, "sum", topo_="1", host=True)
    for r in range(P):
        check(dt, bufs[r].numpy()[:N], want, f"rank {r}")


# ---- Python surface -------------------------------------------------------------------------------------
def test_allreduce_tensor_float8():
    """Comm.allreduce_tensor takes dtype and count from the tensor: torch.float8_e4m3fn CUDA tensors."""
    import threading

    import torch
    P, topo = 4, "2,2"
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather("direct")
    g.set_reduce_scatter("direct")
    ins, want = ref.allreduce_case("f8e4m3", P, topo, N)
    ts = [torch.from_numpy(x.copy()).cuda().view(torch.float8_e4m3fn) for x in ins]
    errs = []

    def rank(r):
        try:
            assert g[r].allreduce_tensor(ts[r], op="sum", topo_=topo) is ts[r]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for r in range(P):
        check("f8e4m3", ts[r].view(torch.uint8).cpu().numpy(), want, f"rank {r}")


def test_rccl_yardstick_knows_the_fp8_dtypes():
    """A one-rank RCCL communicator: ftar_rccl_allreduce returns its input for both dtypes."""
    import ftar
    comm = ftar.Comm.init_rank(1, ftar.get_unique_id(), 0, 0)
    try:
        for dt in ref.FORMATS:
            src = ref.sources(dt, 2, 4099, small_ints=True)[0]
            s, sp = to_dev(src)
            d, dp = filled_dev(src.nbytes)
            comm.rccl_allreduce(sp, dp, src.size, dt, "sum")
            assert np.array_equal(from_dev(d, np.uint8, src.size), src), dt
    finally:
        comm.destroy()
