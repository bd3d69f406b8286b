"""GPU tests of FTAR_AVG and ftar_reduce_scaled (include/ftar.h): every result bit for bit (NaN lanes: NaN or not)
against the per-schedule torch folds of tests/avg_ref.py, whose root fold -- and only it -- finishes as
(acc * r).to(dtype): the scaled kernels (LDS-staged, runtime-k, element-wise, nested), then op="avg" on
in-process groups in every form, piece size and buffer kind, the refusals, and the Python surfaces up to the
DDP hook's average="fused"."""
import threading

import numpy as np
import pytest

import avg_ref
import f16_minmax_ref as ref
from gpu_util import filled_dev, from_dev, to_dev

pytestmark = pytest.mark.gpu

UNSUPPORTED = 2
THIRD = float(np.float32(1) / np.float32(3))    # fl(1 / 3)
_groups = {}


def group(P):
    import ftar
    if P not in _groups:
        _groups[P] = ftar.Comm.init_local(P)
    return _groups[P]


def check(dt, got, want, what=""):
    assert ref.same_bits(dt, got, want), (what, ref.first_diff(dt, got, want))


def run_scaled(ins, dt, scale, offsets=None, out_offset=0, inplace=False, shape=None):
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
    ftar.reduce([p for _, p in devs], dst, n, dt, "sum", shape=shape, scale=scale)
    return from_dev(dst_t, ins[0].dtype, n, out_offset)


# ---- ftar_reduce_scaled ---------------------------------------------------------------------------------
KS = [1, 2, 3, 8, 9, 16, 17, 33]        # a scaled copy, the LDS kernels, f64's switch to registers at 9, runtime k
NS = [1, 255, 4099, 100_003]            # head only, no full tile, full tiles plus a partial one, several workgroups
SCALES = [THIRD, 0.125]


def _reduce_cases():
    """The cross product trimmed: each dtype sees every k and every n, with both scales, plus the largest n at the
    widest LDS kernel and at runtime k."""
    out = []
    for di, dt in enumerate(avg_ref.FLOAT_DTYPES):
        for i, k in enumerate(KS):
            out.append((dt, k, NS[(i + di) % 4], SCALES[(i + di) % 2]))
        out.append((dt, 16, 100_003, THIRD))
        out.append((dt, 33, 4099, THIRD))
        out.append((dt, 2, 100_003, 0.125))
    return sorted(set(out))


@pytest.mark.parametrize("dt,k,n,scale", _reduce_cases())
def test_reduce_scaled_is_the_torch_fold_scaled_then_rounded_once(dt, k, n, scale):
    ins, want = avg_ref.reduce_case(dt, k, n, scale)
    check(dt, run_scaled(ins, dt, scale), want)


@pytest.mark.parametrize("offs,out_off", [([1, 1], 1), ([0, 1], 0), ([2, 0, 1], 3)])
@pytest.mark.parametrize("dt", avg_ref.FLOAT_DTYPES)
def test_reduce_scaled_unaligned(dt, offs, out_off):
    """Co-aligned offsets (vector path with an unaligned head and a short tail) and sources whose alignment
    differs from the destination's (the element-wise kernel)."""
    ins, want = avg_ref.reduce_case(dt, len(offs), 33_333, THIRD)
    check(dt, run_scaled(ins, dt, THIRD, offsets=offs, out_offset=out_off), want)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_reduce_scaled_in_place(dt):
    """dst == srcs[0], the ring's in-place fold."""
    ins, want = avg_ref.reduce_case(dt, 3, 100_003, THIRD)
    check(dt, run_scaled(ins, dt, THIRD, inplace=True), want)


@pytest.mark.parametrize("shape", [(2, 2), (2, 4), (4, 2), (2, 2, 2), (2, 2, 2, 2), (2, 3)])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_reduce_scaled_nested_rounds_inner_nodes_and_scales_the_root(dt, shape):
    """Compile-time shapes on the LDS-staged kernel and a runtime-coded one (2,3): inner nodes rounded, the root
    scaled, then rounded."""
    k = int(np.prod(shape))
    scale = float(np.float32(1) / np.float32(k))
    ins, want = avg_ref.reduce_case(dt, k, 50_001, scale, shape=shape)
    check(dt, run_scaled(ins, dt, scale, shape=list(shape)), want)


def test_reduce_scaled_nested_unaligned_takes_the_element_kernel():
    ins, want = avg_ref.reduce_case("f16", 4, 33_333, 0.25, shape=(2, 2))
    check("f16", run_scaled(ins, "f16", 0.25, offsets=[2, 0, 1, 0], out_offset=3, shape=[2, 2]), want)
    check("f16", run_scaled(ins, "f16", 0.25, offsets=[1, 1, 1, 1], out_offset=1, shape=[2, 2]), want)


# Each fold family is one body under two __global__ names (csrc/reduce_impl.h); profiles and tools key on the
# names.  (call, the plain kernel's template id; the scaled one inserts "_scaled"): exact ids where the call
# fixes every template argument, else the prefix and the shape the id must hold.
FAMILIES = {
    "lds": (dict(dt="f32", k=2), "reduce_lds_kernel<F32Sum, 2, 1, 2, 2, true>"),
    "vec": (dict(dt="f32", k=17), "reduce_vec_kernel<F32Sum, 0, 2, true, true, 512>"),
    "elem": (dict(dt="f32", k=2, offsets=[0, 1]), "reduce_elem_kernel<F32Sum>"),
    "tree_lds": (dict(dt="f32", k=4, shape=(2, 2)), ("reduce_tree_lds_kernel<F32Sum, 4, ", "StaticShape<2, 2>")),
    "tree": (dict(dt="f64", k=4, shape=(2, 2)), ("reduce_tree_kernel<F64Sum, 4, 2, ", "StaticShape<2, 2>")),
    "tree_elem": (dict(dt="f32", k=4, shape=(2, 2), offsets=[0, 1, 0, 0]), "reduce_tree_elem_kernel<F32Sum>"),
}


@pytest.mark.parametrize("scale", [None, 0.25], ids=["plain", "scaled"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_fold_family_is_reached_under_its_name_in_both_finishes(family, scale):
    """n = 4099: a full tile, a partial one and a tail.  The plain expectation is the same torch fold with r = 1
    (an exact multiply)."""
    import ftar
    call, want_id = FAMILIES[family]
    dt, k, shape = call["dt"], call["k"], call.get("shape")
    ins, want = avg_ref.reduce_case(dt, k, 4099, 1.0 if scale is None else scale, shape=shape)
    got = run_scaled(ins, dt, scale, offsets=call.get("offsets"), shape=list(shape) if shape else None)
    name = ftar.names.kernel_symbol(ftar.last_kernel())
    if scale is not None:
        want_id = ([w.replace("_kernel<", "_scaled_kernel<") for w in want_id] if isinstance(want_id, tuple)
                   else want_id.replace("_kernel<", "_scaled_kernel<"))
    if isinstance(want_id, str):
        assert name == want_id
    else:
        assert name.startswith(want_id[0]) and want_id[1] in name, (name, want_id)
    check(dt, got, want, name)


# ---- AllReduce on in-process groups ---------------------------------------------------------------------
N = 50_001
TOPOS = [(2, "1"), (3, "1"), (3, "3"), (4, "2,2"), (6, "1"), (6, "2,3"), (8, "1"), (8, "8"), (8, "2,4"),
         (8, "2,2,2")]
LONELY = [(5, "2,2", 1), (8, "3,2", 2)]


def run_group(ins, topo, dt, op="avg", lonely=0, form="direct", chunk_bytes=0, allgather=None):
    g = group(len(ins))
    g.set_chunk_bytes(chunk_bytes)
    g.set_allgather(allgather or form)
    g.set_reduce_scatter(form)
    n = ins[0].size
    bufs = [to_dev(x) for x in ins]
    g.allreduce(None, [p for _, p in bufs], n, dt, op, topo_=topo, lonely=lonely)
    return [from_dev(t, ins[0].dtype, n) for t, _ in bufs]


def _every_form(ins, want, P, topo, dt, lonely=0):
    first = None
    for form in ("stages", "direct"):
        for chunk_bytes in (0, 512):
            outs = run_group(ins, topo, dt, lonely=lonely, form=form, chunk_bytes=chunk_bytes)
            for r in range(P):
                check(dt, outs[r], want, (form, chunk_bytes, r))
            first = outs[0] if first is None else first
            for r in range(P):   # and the same across forms and piece sizes
                check(dt, outs[r], first, (form, chunk_bytes, r, "vs stages / one piece"))


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("P,topo", TOPOS)
def test_allreduce_avg_is_the_schedules_fold_scaled_at_the_root(P, topo, dt):
    """Ring: one rounding per hop and the last hop scaled (staged hops, or the one-round fold that rounds before
    each add); trees: one rounding per node and the root scaled (staged, or the nested fold).  Every rank,
    every form and piece size, against the fold written out in torch, and against each other."""
    ins, want = avg_ref.allreduce_case(dt, P, topo, N)
    _every_form(ins, want, P, topo, dt)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("P,topo,lonely", LONELY)
def test_allreduce_avg_lonely_layouts(P, topo, lonely, dt):
    """Integer-valued inputs times P: the mean is exact for any association."""
    ins, want = avg_ref.exact_case(dt, P, N)
    _every_form(ins, want, P, topo, dt, lonely=lonely)


@pytest.mark.parametrize("mode", ["read", "write"])
def test_allreduce_avg_peer_direct(mode):
    P, topo = 4, "2,2"
    ins, want = avg_ref.allreduce_case("f16", P, topo, N)
    g = group(P)
    g.set_peer_direct(mode)
    try:
        outs = run_group(ins, topo, "f16")
    finally:
        g.set_peer_direct(False)
    for r in range(P):
        check("f16", outs[r], want, f"rank {r}")


def test_allreduce_avg_host_buffers():
    """ftar_allreduce_host on pinned host buffers, P = 2 ring, bf16."""
    import torch
    P = 2
    ins, want = avg_ref.allreduce_case("bf16", P, "1", N)
    g = group(P)
    g.set_host_chunk_bytes(0)
    g.set_allgather("direct")
    g.set_reduce_scatter("direct")
    bufs = [torch.from_numpy(x.view(np.uint8).copy()).pin_memory() for x in ins]
    g.allreduce(None, bufs, N, "bf16", "avg", topo_="1", host=True)
    for r in range(P):
        check("bf16", bufs[r].numpy().view(np.uint16)[:N], want, f"rank {r}")


def test_allreduce_avg_collective_allgather():
    P, topo, n = 4, "4", 50_000      # P | n: the all-gather is the one collective
    ins, want = avg_ref.allreduce_case("f32", P, topo, n)
    outs = run_group(ins, topo, "f32", form="direct", allgather="collective")
    assert group(P)[0].last_exec()["form"] == "collective"
    for r in range(P):
        check("f32", outs[r], want, f"rank {r}")


@pytest.mark.parametrize("dt", ["i32", "bool"])
def test_allreduce_avg_refuses_integers_and_leaves_the_buffers(dt):
    import ftar
    P = 2
    ins = ref.sources("i32", P, 4099) if dt == "i32" else tuple((x & 1).astype(np.uint8)
                                                                for x in ref.sources("u8", P, 4099))
    g = group(P)
    bufs = [to_dev(x) for x in ins]
    with pytest.raises(ftar.FtarError) as e:
        g.allreduce(None, [p for _, p in bufs], 4099, dt, "avg", topo_="1")
    assert e.value.status == UNSUPPORTED
    for (t, _), x in zip(bufs, ins):
        assert from_dev(t, x.dtype, x.size).tobytes() == x.tobytes()


# ---- Python surface -------------------------------------------------------------------------------------
def _on_threads(P, fn):
    import torch
    errs = []

    def rank(r):
        try:
            fn(r)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs


def _f16_tensors(ins):
    import torch
    return [torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.float16) for x in ins]


def _f16_bits(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _direct(P):
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather("direct")
    g.set_reduce_scatter("direct")
    return g


def test_allreduce_tensor_avg_float16():
    P, topo = 4, "2,2"
    g = _direct(P)
    ins, want = avg_ref.allreduce_case("f16", P, topo, N)
    ts = _f16_tensors(ins)
    _on_threads(P, lambda r: g[r].allreduce_tensor(ts[r], op="avg", topo_=topo))
    for r in range(P):
        check("f16", _f16_bits(ts[r]), want, f"rank {r}")
    ts = _f16_tensors(ins)
    assert g.allreduce_tensors(ts, op="avg", topo_=topo) is ts
    import torch
    torch.cuda.synchronize()
    for r in range(P):
        check("f16", _f16_bits(ts[r]), want, f"group, rank {r}")


class Bucket:
    """A stand-in for torch.distributed.GradBucket."""

    def __init__(self, t):
        self.t = t

    def buffer(self):
        return self.t


def test_ddp_hook_fused_average_over_threads():
    """P = 4 ranks on threads: average="fused" gives the avg_ref mean; the default state still divides and sums,
    bit for bit div_ followed by op="sum"."""
    import torch

    import ftar.ddp
    P, topo = 4, "2,2"
    g = _direct(P)
    ins, want = avg_ref.allreduce_case("f16", P, topo, N)

    ts = _f16_tensors(ins)
    states = [ftar.ddp.HookState(g[r], topo=topo, average="fused") for r in range(P)]
    outs = [None] * P

    def fused(r):
        outs[r] = ftar.ddp.allreduce_hook(states[r], Bucket(ts[r])).wait()
    _on_threads(P, fused)
    for r in range(P):
        assert outs[r] is ts[r] and states[r].calls == 1
        check("f16", _f16_bits(ts[r]), want, f"fused, rank {r}")

    ts = _f16_tensors(ins)
    states = [ftar.ddp.HookState(g[r], topo=topo) for r in range(P)]
    assert all(s.average == "divide" for s in states)
    _on_threads(P, lambda r: ftar.ddp.allreduce_hook(states[r], Bucket(ts[r])).wait())
    by_hand = _f16_tensors(ins)
    for t in by_hand:
        t.div_(P)
    g.allreduce_tensors(by_hand, op="sum", topo_=topo)
    torch.cuda.synchronize()
    for r in range(P):
        check("f16", _f16_bits(ts[r]), _f16_bits(by_hand[r]), f"divide, rank {r}")
    with pytest.raises(ValueError):
        ftar.ddp.HookState(g[0], average="mean")


def test_one_rank_rccl_hook_fused_and_rccl_avg_return_their_input():
    """A one-rank RCCL communicator: the fused hook returns the bucket unchanged (P = 1 is SUM's copy), and
    ftar_rccl_allreduce with op="avg" (ncclAvg) returns its input."""
    import torch

    import ftar
    import ftar.ddp
    comm = ftar.Comm.init_rank(1, ftar.get_unique_id(), 0, 0)
    try:
        x = ref.sources("f16", 2, 4099, small_ints=True)[0]
        t = torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.float16)
        state = ftar.ddp.HookState(comm, average="fused")
        out = ftar.ddp.allreduce_hook(state, Bucket(t)).wait()
        torch.cuda.synchronize()
        assert out is t and state.calls == 1
        assert np.array_equal(_f16_bits(t), x)
        for dt in ("f16", "f32"):
            src = ref.sources(dt, 2, 4099, small_ints=True)[0]
            s, sp = to_dev(src)
            d, dp = filled_dev(src.nbytes)
            comm.rccl_allreduce(sp, dp, src.size, dt, "avg")
            assert np.array_equal(from_dev(d, src.dtype, src.size), src), dt
        with pytest.raises(ftar.FtarError) as e:
            comm.rccl_allreduce(sp, dp, 16, "i32", "avg")
        assert e.value.status == UNSUPPORTED
    finally:
        comm.destroy()
