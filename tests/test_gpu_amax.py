"""GPU tests of the amax entry points (include/ftar.h): ftar_reduce_amax on one device, then ftar_allreduce_amax
on in-process groups in every form, the refusals, and the Python surfaces up to the DDP hook's track_amax.

Every case checks (a) the result bit for bit against the reference that already pins that fold, (b) the amax
word against tests/amax_ref.py's reading of that expectation, and (c) where the call also exists without amax,
that both give the same result bits.  Inputs are finite with one negative peak at a known position (amax_ref),
so a path that misses that position -- or forgets the abs -- leaves a different word."""
import threading

import numpy as np
import pytest

import amax_ref
import f16_minmax_ref as ref
import f8_ref
import kernel_edges
from gpu_util import filled_dev, from_dev, to_dev

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 2
INF32 = 0x7F800000
_groups = {}


def group(P):
    import ftar
    if P not in _groups:
        _groups[P] = ftar.Comm.init_local(P)
    return _groups[P]


def check(dt, got, want, what=""):
    m = f8_ref if amax_ref.is_f8(dt) else ref
    assert m.same_bits(dt, got, want), (what, m.first_diff(dt, got, want))


def check_word(got, want, what=""):
    assert amax_ref.matches(got, want), (what, hex(int(got)), want if want == amax_ref.NAN else hex(want))


def word_of(t):
    return int(from_dev(t, np.uint32, 1)[0])


def run_amax(ins, dt, scale, offsets=None, out_offset=0, inplace=False, shape=None, amax=None, plain=True):
    """ftar_reduce_amax on fresh device copies: (stored result, the amax word); with `plain` the same call
    without amax (ftar_reduce_scaled) must store the same bits."""
    import ftar
    n = ins[0].size
    offsets = offsets or [0] * len(ins)
    esz = ins[0].dtype.itemsize

    def launch(**kw):
        devs = [to_dev(x, offset_elems=o) for x, o in zip(ins, offsets)]
        if inplace:
            dst_t, dst, off = devs[0][0], devs[0][1], offsets[0]
        else:
            dst_t, dst = filled_dev((n + out_offset) * esz)
            dst, off = dst + out_offset * esz, out_offset
        ftar.reduce([p for _, p in devs], dst, n, dt, "sum", shape=shape, scale=scale, **kw)
        return from_dev(dst_t, ins[0].dtype, n, off)
    am_t, am = amax if amax is not None else filled_dev(4)      # 0xA5A5A5A5: a stale word to overwrite
    got = launch(amax=am)
    word = word_of(am_t)
    if plain:
        m = f8_ref if amax_ref.is_f8(dt) else ref
        assert m.same_bits(dt, launch(), got), "the amax call stores the scaled call's bits"
    return got, word


# ---- ftar_reduce_amax -----------------------------------------------------------------------------------
KS = [1, 2, 3, 8, 9, 17, 33]        # a scaled copy, the LDS kernels (fp8: up to 8), runtime k
NS = [1, 255, 4099, 100_003]        # head only, no full tile, full tiles plus a partial one, several workgroups


def _reduce_cases():
    """The cross product trimmed as tests/test_gpu_avg.py trims its own: each dtype sees every k and every n, with
    both scales, plus the largest n at the widest LDS kernel and at runtime k."""
    out = []
    for di, dt in enumerate(amax_ref.DTYPES):
        ks = [k for k in KS if k <= 17] if amax_ref.is_f8(dt) else KS
        for i, k in enumerate(ks):
            out.append((dt, k, NS[(i + di) % 4], (i + di) % 2 == 0))
        out.append((dt, 8 if amax_ref.is_f8(dt) else 16, 100_003, True))
        out.append((dt, ks[-1], 4099, True))
        out.append((dt, 2, 100_003, False))
    return sorted(set(out))


def _scale(k, mean):
    return float(np.float32(1) / np.float32(k)) if mean else 1.0


@pytest.mark.parametrize("dt,k,n,mean", _reduce_cases())
def test_reduce_amax_is_the_scaled_fold_and_its_abs_max(dt, k, n, mean):
    scale = _scale(k, mean)
    ins, want, word = amax_ref.reduce_case(dt, k, n, scale, n // 3)
    got, w = run_amax(ins, dt, scale)
    check(dt, got, want)
    check_word(w, word)


def tile_vectors(symbol):
    """The 16-byte vectors one workgroup of a launched *_amax_kernel covers per pass (kernel_edges.geometry
    reads the name)."""
    assert "_amax_kernel<" in symbol, symbol
    return kernel_edges.geometry(symbol).wg_tile


@pytest.mark.parametrize("k", [2, 17])
@pytest.mark.parametrize("n", [4099, 100_003])
@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_reduce_amax_finds_the_peak_at_every_edge(dt, n, k):
    """The head, the tail, the wave-tile edge and the full / partial workgroup-tile boundary: one launch each."""
    import ftar
    ve = amax_ref.elems_per_vector(dt)
    scale = _scale(k, True)
    ins, want, word = amax_ref.reduce_case(dt, k, n, scale, 0)
    run_amax(ins, dt, scale, plain=False)
    T = tile_vectors(ftar.names.kernel_symbol(ftar.last_kernel()))
    for p in sorted({0, 1, n - 2, n - 1, 64 * ve - 1, 64 * ve, T * ve - 1, T * ve}):
        if not 0 <= p < n:
            continue
        ins, want, word = amax_ref.reduce_case(dt, k, n, scale, p)
        got, w = run_amax(ins, dt, scale, plain=False)
        check(dt, got, want, p)
        check_word(w, word, p)


@pytest.mark.parametrize("offs,out_off", [([1, 1], 1), ([0, 1], 0), ([2, 0, 1], 3)])
@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_reduce_amax_unaligned(dt, offs, out_off):
    """Co-aligned offsets (an unaligned head and a short tail; the peak in the head, then in the tail) and
    mismatched alignment (the element-wise kernel)."""
    n = 33_333
    for p in (0, n - 1, n // 2):
        ins, want, word = amax_ref.reduce_case(dt, len(offs), n, 1.0, p)
        got, w = run_amax(ins, dt, 1.0, offsets=offs, out_offset=out_off)
        check(dt, got, want, p)
        check_word(w, word, p)


@pytest.mark.parametrize("dt", ["f16", "f32", "f8e5m2"])
def test_reduce_amax_in_place(dt):
    ins, want, word = amax_ref.reduce_case(dt, 3, 100_003, _scale(3, True), 77_777)
    got, w = run_amax(ins, dt, _scale(3, True), inplace=True)
    check(dt, got, want)
    check_word(w, word)


@pytest.mark.parametrize("shape", [(2, 2), (2, 4), (2, 2, 2), (2, 3)])
@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_reduce_amax_nested(dt, shape):
    k = int(np.prod(shape))
    for mean in (False, True):
        scale = _scale(k, mean)
        ins, want, word = amax_ref.reduce_case(dt, k, 50_001, scale, 50_000, shape=shape)
        got, w = run_amax(ins, dt, scale, shape=list(shape))
        check(dt, got, want, mean)
        check_word(w, word, mean)


# every fold family under its _amax_kernel name, as tests/test_gpu_avg.py FAMILIES does for _scaled (f64 has no
# amax: the register tree kernel is reached by a 2-byte runtime-coded shape)
FAMILIES = {
    "lds": (dict(dt="f32", k=2), "reduce_lds_amax_kernel<F32Sum, 2, 4, 4, 2, true>"),
    "vec": (dict(dt="f32", k=17), "reduce_vec_amax_kernel<F32Sum, 0, 2, true, true, 512>"),
    "copy": (dict(dt="f16", k=1), ("reduce_vec_amax_kernel<H16SumT<HalfFmt>, 0, 2, true, true, 512>", "")),
    "elem": (dict(dt="f32", k=2, offsets=[0, 1]), "reduce_elem_amax_kernel<F32Sum>"),
    "tree_lds": (dict(dt="f32", k=4, shape=(2, 2)), ("reduce_tree_lds_amax_kernel<F32Sum, 4, ", "StaticShape<2, 2>")),
    "tree": (dict(dt="bf16", k=6, shape=(2, 3)), ("reduce_tree_amax_kernel<", "RuntimeShape")),
    "tree_elem": (dict(dt="f32", k=4, shape=(2, 2), offsets=[0, 1, 0, 0]), "reduce_tree_elem_amax_kernel<F32Sum>"),
    "f8_lds": (dict(dt="f8e4m3", k=8), ("reduce_lds_amax_kernel<F8SumT<F8Fmt<false>", "")),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_fold_family_is_reached_under_its_amax_name(family):
    """n = 4099: a full tile, a partial one and a tail; the peak in the partial tile."""
    import ftar
    call, want_id = FAMILIES[family]
    dt, k, shape = call["dt"], call["k"], call.get("shape")
    scale = _scale(k, True)
    ins, want, word = amax_ref.reduce_case(dt, k, 4099, scale, 4090, shape=shape)
    got, w = run_amax(ins, dt, scale, offsets=call.get("offsets"), shape=list(shape) if shape else None, plain=False)
    name = ftar.names.kernel_symbol(ftar.last_kernel())
    if isinstance(want_id, str):
        assert name == want_id
    else:
        assert name.startswith(want_id[0]) and want_id[1] in name, (name, want_id)
    check(dt, got, want, name)
    check_word(w, word, name)


def _special(dt, n, lanes):
    """Two sources of zeros with `lanes` = {position: (encoding in source 0, encoding in source 1)}."""
    u = amax_ref.storage(dt)
    xs = [np.zeros(n, u), np.zeros(n, u)]
    for p, (a, b) in lanes.items():
        xs[0][p], xs[1][p] = a, b
    return xs


def _sign(dt):
    return 1 << (8 * np.dtype(amax_ref.storage(dt)).itemsize - 1)


@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_special_all_zeros_with_negative_zero_lanes_give_bits_0(dt):
    s = _sign(dt)
    ins = _special(dt, 4099, {0: (s, s), 5: (s, 0), 4098: (s, s), 2048: (0, s)})
    got, w = run_amax(ins, dt, 1.0)
    check(dt, got, amax_ref.fold(dt, ins, 1.0))
    assert w == 0


@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_special_a_subnormal_only_peak_is_kept(dt):
    ins = _special(dt, 4099, {4000: (_sign(dt) | 3, 0), 17: (1, 0)})
    want = amax_ref.fold(dt, ins, 1.0)
    got, w = run_amax(ins, dt, 1.0)
    check(dt, got, want)
    assert w == amax_ref.widen(dt, 3) and w != 0
    check_word(w, amax_ref.amax_bits(dt, want))


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32", "f8e5m2"])
def test_special_an_inf_source_gives_plus_inf(dt):
    ins = amax_ref.plant(dt, amax_ref.base_sources(dt, 3, 4099), 4097, 1, float("-inf"))
    want = amax_ref.fold(dt, ins, 1.0)
    got, w = run_amax(ins, dt, 1.0)
    check(dt, got, want)
    assert w == INF32 and amax_ref.amax_bits(dt, want) == INF32


@pytest.mark.parametrize("dt", amax_ref.DTYPES)
def test_special_a_nan_source_gives_nan(dt):
    ins = amax_ref.plant(dt, amax_ref.base_sources(dt, 3, 4099), 300, 2, float("nan"))
    want = amax_ref.fold(dt, ins, 1.0)
    got, w = run_amax(ins, dt, 1.0)
    check(dt, got, want)
    assert amax_ref.amax_bits(dt, want) == amax_ref.NAN
    check_word(w, amax_ref.NAN)


def test_special_f16_overflow_is_inf_at_scale_1_and_finite_at_half():
    ins = _special("f16", 4099, {1000: (amax_ref.encode("f16", 65504.0), amax_ref.encode("f16", 16.0))})
    got, w = run_amax(ins, "f16", 1.0)
    check("f16", got, amax_ref.fold("f16", ins, 1.0))
    assert w == INF32
    want = amax_ref.fold("f16", ins, 0.5)
    got, w = run_amax(ins, "f16", 0.5)
    check("f16", got, want)
    assert w == amax_ref.amax_bits("f16", want) and w < INF32 and w != 0


def test_special_e4m3_overflow_is_nan_at_scale_1_and_448_at_half():
    e448 = amax_ref.encode("f8e4m3", 448.0)
    ins = _special("f8e4m3", 4099, {1000: (e448, e448)})
    got, w = run_amax(ins, "f8e4m3", 1.0)
    check("f8e4m3", got, amax_ref.fold("f8e4m3", ins, 1.0))
    check_word(w, amax_ref.NAN)
    got, w = run_amax(ins, "f8e4m3", 0.5)
    check("f8e4m3", got, amax_ref.fold("f8e4m3", ins, 0.5))
    assert w == amax_ref.widen("f8e4m3", e448) == 0x43E00000     # 448.0f


@pytest.mark.parametrize("dt", ["f16", "f32", "f8e4m3"])
def test_a_stale_word_is_overwritten(dt):
    """Two calls on one amax pointer: with the peak, then without it -- the second reports the small value."""
    am = filled_dev(4)
    ins, want, word = amax_ref.reduce_case(dt, 2, 4099, 1.0, 2000)
    _, w = run_amax(ins, dt, 1.0, amax=am, plain=False)
    check_word(w, word)
    base = amax_ref.base_sources(dt, 2, 4099)
    small = amax_ref.amax_bits(dt, amax_ref.fold(dt, base, 1.0))
    assert small != amax_ref.NAN and small < word
    _, w = run_amax(base, dt, 1.0, amax=am, plain=False)
    check_word(w, small)


@pytest.mark.parametrize("dt,k,n", [("f32", 2, 4099), ("bf16", 17, 4099), ("f8e5m2", 3, 100_003), ("f16", 1, 255)])
def test_write_footprint_is_the_n_elements_and_the_one_word(dt, k, n):
    import ftar
    ins, want, word = amax_ref.reduce_case(dt, k, n, 1.0, n - 1)
    esz = ins[0].dtype.itemsize
    fold = kernel_edges.Fold(ins, want)
    am = kernel_edges.Arena(64)
    srcs, dst = fold.pointers(0)
    ftar.reduce(srcs, dst, n, dt, "sum", amax=am.ptr(16))
    import torch
    torch.cuda.synchronize()
    got = int(am.window(16, 20).cpu().numpy().view(np.uint32)[0])
    assert kernel_edges.check_untouched(am, 16, 20) is None
    check_word(got, word)
    assert fold.verify(0, n) is None
    assert esz * n == want.nbytes


def test_reduce_amax_captures_into_a_hip_graph():
    """A memset node and a kernel: replayed twice on different inputs, the word follows the inputs."""
    import ftar
    import torch
    dt, k, n = "f16", 8, 100_003
    ins, want, word = amax_ref.reduce_case(dt, k, n, 1.0, 5)
    srcs = [torch.from_numpy(x.view(np.int16).copy()).cuda() for x in ins]
    ptrs = [s.data_ptr() for s in srcs]
    out = torch.empty(n, dtype=torch.int16, device="cuda")
    am = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ftar.reduce(ptrs, out.data_ptr(), n, dt, "sum", stream=side, amax=am.data_ptr())
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    check(dt, out.cpu().numpy().view(np.uint16), want)
    check_word(int(am.cpu().numpy().view(np.uint32)[0]), word)
    ins2, want2, word2 = amax_ref.reduce_case(dt, k, n, 1.0, 99_999, src=0, seed=2)
    for s, x in zip(srcs, ins2):
        s.copy_(torch.from_numpy(x.view(np.int16).copy()))
    am.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    check(dt, out.cpu().numpy().view(np.uint16), want2)
    check_word(int(am.cpu().numpy().view(np.uint32)[0]), word2)


# ---- AllReduce on in-process groups ---------------------------------------------------------------------
N = 50_001
TOPOS = [(2, "1"), (3, "3"), (4, "2,2"), (6, "2,3"), (8, "1"), (8, "8"), (8, "2,2,2")]
LONELY = [(5, "2,2", 1), (8, "3,2", 2)]


def _settings(g, form="direct", chunk_bytes=0, allgather=None):
    g.set_chunk_bytes(chunk_bytes)
    g.set_allgather(allgather or form)
    g.set_reduce_scatter(form)


def run_group_amax(ins, topo, dt, op, lonely=0, form="direct", chunk_bytes=0, allgather=None, out_of_place=False,
                   amax=True):
    """Every rank's (result, amax word) of one call; amax=False: the same call without amax (words None)."""
    g = group(len(ins))
    _settings(g, form, chunk_bytes, allgather)
    n = ins[0].size
    bufs = [to_dev(x) for x in ins]
    outs = [filled_dev(ins[0].nbytes) for _ in ins] if out_of_place else bufs
    ams = [filled_dev(4) for _ in ins]
    g.allreduce([p for _, p in bufs] if out_of_place else None, [p for _, p in outs], n, dt, op, topo_=topo,
                lonely=lonely, amaxes=[p for _, p in ams] if amax else None)
    res = [from_dev(t, ins[0].dtype, n) for t, _ in outs]
    if out_of_place:
        for (t, _), x in zip(bufs, ins):
            assert from_dev(t, x.dtype, n).tobytes() == x.tobytes(), "sendbuf is read only"
    return res, [word_of(t) if amax else None for t, _ in ams]


def _check_ranks(dt, outs, words, want, word, what):
    for r, (o, w) in enumerate(zip(outs, words)):
        check(dt, o, want, (what, r))
        check_word(w, word, (what, r))
    if word != amax_ref.NAN:
        assert len(set(words)) == 1, (what, words)


def _every_form(case, P, topo, dt, op, lonely=0):
    """Every rank, stages / direct x whole blocks / 512-byte pieces: the expectation, its amax, one word across
    the forms, and the call without amax storing the same bits."""
    seen = set()
    for p in _placements(P):
        ins, want, word = case(p)
        for form in ("stages", "direct"):
            for chunk_bytes in (0, 512):
                outs, words = run_group_amax(ins, topo, dt, op, lonely=lonely, form=form, chunk_bytes=chunk_bytes)
                _check_ranks(dt, outs, words, want, word, (p, form, chunk_bytes))
                seen.update(words)
        plain, _ = run_group_amax(ins, topo, dt, op, lonely=lonely, amax=False)
        check(dt, plain[0], want, (p, "without amax"))
        assert len(seen) == 1, (p, seen)
        seen.clear()


def _placements(P, n=N):
    """The peak (in rank P // 2's input) at the first and the last element of blocks 0, P // 2 and P - 1."""
    out = []
    for b in sorted({0, P // 2, P - 1}):
        out += list(amax_ref.block_edges(n, P, b))
    return out


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("P,topo", TOPOS)
def test_allreduce_amax_every_topology_and_form(P, topo, dt, op):
    _every_form(lambda p: amax_ref.allreduce_case(dt, P, topo, N, op, p), P, topo, dt, op)


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("dt", ["f8e4m3", "f8e5m2"])
@pytest.mark.parametrize("P,topo", [(4, "2,2"), (8, "1")])
def test_allreduce_amax_fp8(P, topo, dt, op):
    _every_form(lambda p: amax_ref.allreduce_case(dt, P, topo, N, op, p), P, topo, dt, op)


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("P,topo,lonely", LONELY)
def test_allreduce_amax_lonely_layouts(P, topo, lonely, dt, op):
    """Exact integer inputs plus the peak: exact for any association."""
    _every_form(lambda p: amax_ref.exact_case(dt, P, N, op, p), P, topo, dt, op, lonely=lonely)


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("mode", ["read", "write"])
def test_allreduce_amax_peer_direct(mode, op):
    P, topo, dt = 4, "2,2", "f16"
    g = group(P)
    for p in _placements(P)[1:4]:
        ins, want, word = amax_ref.allreduce_case(dt, P, topo, N, op, p)
        g.set_peer_direct(mode)
        try:
            outs, words = run_group_amax(ins, topo, dt, op)
            assert g[0].last_exec()["form"] == "peer-" + mode
        finally:
            g.set_peer_direct(False)
        _check_ranks(dt, outs, words, want, word, (mode, p))


@pytest.mark.parametrize("op", ["sum", "avg"])
def test_allreduce_amax_collective_allgather(op):
    P, topo, n, dt = 4, "4", 50_000, "f32"       # P | n: the all-gather is the one collective
    for p in (n // P * 3, n - 1):
        ins, want, word = amax_ref.allreduce_case(dt, P, topo, n, op, p)
        outs, words = run_group_amax(ins, topo, dt, op, form="direct", allgather="collective")
        assert group(P)[0].last_exec()["form"] == "collective"
        _check_ranks(dt, outs, words, want, word, p)


@pytest.mark.parametrize("form", ["stages", "direct"])
@pytest.mark.parametrize("topo", ["1", "2,2,2"])
@pytest.mark.parametrize("n", [1, 3])
def test_allreduce_amax_with_empty_blocks(n, topo, form):
    P, dt = 8, "bf16"
    for op in ("sum", "avg"):
        ins, want, word = amax_ref.allreduce_case(dt, P, topo, n, op, n - 1)
        outs, words = run_group_amax(ins, topo, dt, op, form=form)
        _check_ranks(dt, outs, words, want, word, op)


@pytest.mark.parametrize("dt", ["f16", "f32", "f8e4m3"])
def test_allreduce_amax_on_one_rank_in_place_and_out_of_place(dt):
    """P = 1: the copy becomes a k = 1 amax fold; AVG's r is 1."""
    ins, _, _ = amax_ref.reduce_case(dt, 2, 4099, 1.0, 4098)
    x = ins[1]
    word = amax_ref.checked(dt, x, 4098)
    for op in ("sum", "avg"):
        for oop in (False, True):
            outs, words = run_group_amax([x], "1", dt, op, out_of_place=oop)
            _check_ranks(dt, outs, words, x, word, (op, oop))


@pytest.mark.parametrize("op", ["sum", "avg"])
def test_allreduce_amax_out_of_place(op):
    P, topo, dt = 4, "2,2", "bf16"
    ins, want, word = amax_ref.allreduce_case(dt, P, topo, N, op, N - 1)
    for form in ("stages", "direct"):
        outs, words = run_group_amax(ins, topo, dt, op, form=form, out_of_place=True)
        _check_ranks(dt, outs, words, want, word, form)


def test_amax_calls_on_two_streams_do_not_share_the_word_too_early():
    """The communicator's word and slots follow its scratch's rule: a call on another stream waits for the
    previous call's last use of them.  A large bucket with the peak on stream A, then at once a small one
    without it on stream B, and the other way round: each word is its own call's."""
    import torch
    P, topo, dt = 4, "2,2", "f16"
    g = group(P)
    _settings(g)
    big_n = 1 << 22
    big, want_big, word_big = amax_ref.allreduce_case(dt, P, topo, big_n, "sum", big_n - 1)
    small = amax_ref.base_sources(dt, P, 4099)
    want_small = amax_ref.schedule(dt, small, topo, "sum")
    word_small = amax_ref.amax_bits(dt, want_small)
    assert word_small != amax_ref.NAN and word_small < word_big
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for first_big in (True, False):
        bufs = {"big": [to_dev(x) for x in big], "small": [to_dev(x) for x in small]}
        ams = {k: [filled_dev(4) for _ in range(P)] for k in bufs}
        torch.cuda.synchronize()
        for which, s in ((("big", sa), ("small", sb)) if first_big else (("small", sb), ("big", sa))):
            n = big_n if which == "big" else 4099
            g.allreduce(None, [p for _, p in bufs[which]], n, dt, "sum", topo_=topo, streams=[s] * P,
                        amaxes=[p for _, p in ams[which]])
        torch.cuda.synchronize()
        for r in range(P):
            check(dt, from_dev(bufs["big"][r][0], big[0].dtype, big_n), want_big, (first_big, r))
            check(dt, from_dev(bufs["small"][r][0], small[0].dtype, 4099), want_small, (first_big, r))
            check_word(word_of(ams["big"][r][0]), word_big, (first_big, "big", r))
            check_word(word_of(ams["small"][r][0]), word_small, (first_big, "small", r))


def test_last_exec_after_an_amax_call_describes_the_buckets_allreduce():
    P, topo, dt = 4, "2,2", "f32"
    ins, want, word = amax_ref.allreduce_case(dt, P, topo, N, "sum", 5)
    _, _ = run_group_amax(ins, topo, dt, "sum", amax=False)
    plain = group(P)[0].last_exec()
    outs, words = run_group_amax(ins, topo, dt, "sum")
    assert group(P)[0].last_exec() == plain
    _check_ranks(dt, outs, words, want, word, "")


def test_allreduce_amax_of_zero_elements_is_plus_zero():
    P = 4
    g = group(P)
    _settings(g)
    bufs = [filled_dev(16) for _ in range(P)]
    ams = [filled_dev(4) for _ in range(P)]
    g.allreduce(None, [p for _, p in bufs], 0, "f16", "sum", topo_="2,2", amaxes=[p for _, p in ams])
    assert [word_of(t) for t, _ in ams] == [0] * P
    assert all(from_dev(t, np.uint8, 16).tolist() == [0xA5] * 16 for t, _ in bufs)


def test_overflow_made_visible():
    """fp16 sources whose per-lane sum exceeds 65504, direct form: SUM's amax is +inf, AVG's the mean's."""
    P, topo, dt, p = 4, "2,2", "f16", 12_345
    ins = amax_ref.base_sources(dt, P, N)
    for x in ins:
        x[p] = amax_ref.encode(dt, -30000.0)
    want = amax_ref.schedule(dt, ins, topo, "sum")
    outs, words = run_group_amax(ins, topo, dt, "sum")
    assert amax_ref.amax_bits(dt, want) == INF32
    _check_ranks(dt, outs, words, want, INF32, "sum")
    want = amax_ref.schedule(dt, ins, topo, "avg")
    word = amax_ref.checked(dt, want, p)
    assert word == amax_ref.widen(dt, amax_ref.encode(dt, 30000.0))
    outs, words = run_group_amax(ins, topo, dt, "avg")
    _check_ranks(dt, outs, words, want, word, "avg")


@pytest.mark.parametrize("dt,op", [("i32", "sum"), ("f64", "sum"), ("f32", "max")])
def test_allreduce_amax_refusals_leave_the_buffers_and_the_word(dt, op):
    import ftar
    P, n = 2, 4099
    ins = ref.sources(dt, P, n)
    g = group(P)
    _settings(g)
    bufs = [to_dev(x) for x in ins]
    ams = [filled_dev(4) for _ in range(P)]
    with pytest.raises(ftar.FtarError) as e:
        g.allreduce(None, [p for _, p in bufs], n, dt, op, topo_="1", amaxes=[p for _, p in ams])
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        g[0].allreduce(None, bufs[0][1], n, dt, op, topo_="1", amax=ams[0][1])
    assert e.value.status == UNSUPPORTED
    for (t, _), x in zip(bufs, ins):
        assert from_dev(t, x.dtype, x.size).tobytes() == x.tobytes()
    assert [word_of(t) for t, _ in ams] == [0xA5A5A5A5] * P


def test_allreduce_amax_under_capture_is_refused():
    """The capture stream itself for every rank: status 2 with "capture" in the message before anything is
    enqueued; an empty capture may be rejected at its end."""
    import torch

    import ftar
    P, n = 2, 1 << 12
    g = group(P)
    _settings(g)
    xs = [torch.ones(n, device="cuda") for _ in range(P)]
    ams = [torch.full((1,), 7.0, device="cuda") for _ in range(P)]
    g.allreduce(None, xs, n, "f32", "sum", topo_="2", amaxes=ams)      # warm: nothing would have to grow
    torch.cuda.synchronize()
    assert all(float(a) == float(P) for a in ams)
    for a in ams:
        a.fill_(7.0)
    s0 = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    errs = []
    with torch.cuda.stream(s0):
        try:
            with torch.cuda.graph(graph, stream=s0, capture_error_mode="relaxed"):
                try:
                    g.allreduce(None, xs, n, "f32", "sum", topo_="2", streams=[s0] * P, amaxes=ams)
                except ftar.FtarError as e:
                    errs.append(e)
                try:
                    g[0].allreduce(None, xs[0], n, "f32", "sum", topo_="2", stream=s0, amax=ams[0])
                except ftar.FtarError as e:
                    errs.append(e)
        except RuntimeError:
            pass   # an empty capture may be rejected at its end; the status is what matters
    torch.cuda.synchronize()
    assert len(errs) == 2 and all(e.status == UNSUPPORTED and "capture" in str(e) for e in errs), errs
    assert all(bool((x == P).all()) for x in xs) and all(float(a) == 7.0 for a in ams)


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


def _f32_word(t):
    import torch
    return int(t.view(torch.int32).cpu().numpy().view(np.uint32)[0])


def test_allreduce_tensor_amax_on_threads_and_allreduce_tensors_amaxes():
    import torch
    P, topo, dt = 4, "2,2", "f16"
    g = group(P)
    _settings(g)
    ins, want, word = amax_ref.allreduce_case(dt, P, topo, N, "avg", N // 2)
    ts = _f16_tensors(ins)
    ams = [torch.full((1,), -1.0, device="cuda") for _ in range(P)]
    _on_threads(P, lambda r: g[r].allreduce_tensor(ts[r], op="avg", topo_=topo, amax=ams[r]))
    for r in range(P):
        check(dt, _f16_bits(ts[r]), want, r)
        check_word(_f32_word(ams[r]), word, r)
    ts = _f16_tensors(ins)
    ams = [torch.full((1,), -1.0, device="cuda") for _ in range(P)]
    assert g.allreduce_tensors(ts, op="avg", topo_=topo, amaxes=ams) is ts
    torch.cuda.synchronize()
    for r in range(P):
        check(dt, _f16_bits(ts[r]), want, ("group", r))
        check_word(_f32_word(ams[r]), word, ("group", r))
    with pytest.raises(ValueError):
        g[0].allreduce_tensor(ts[0], amax=torch.zeros(2, device="cuda"))


class Bucket:
    """A stand-in for torch.distributed.GradBucket."""

    def __init__(self, t):
        self.t = t

    def buffer(self):
        return self.t


def test_ddp_hook_tracks_amax_and_found_inf_over_threads():
    """P = 4 ranks on threads, the staged ring (one rounding per hop), average="fused", two buckets per rank: a
    finite one, then one whose lane p overflows at the first hop (65504 + 65504) and stays inf through the mean."""
    import torch

    import ftar.ddp
    P, topo, dt, p = 4, "1", "f16", 4321
    g = group(P)
    _settings(g, form="stages")
    ins, want, word = amax_ref.allreduce_case(dt, P, topo, N, "avg", p)
    over = amax_ref.base_sources(dt, P, N, seed=2)
    for x in over:
        x[p] = amax_ref.encode(dt, 65504.0)
    want2 = amax_ref.schedule(dt, over, topo, "avg")
    assert amax_ref.amax_bits(dt, want2) == INF32
    states = [ftar.ddp.HookState(g[r], topo=topo, average="fused", track_amax=True) for r in range(P)]
    ts, ts2 = _f16_tensors(ins), _f16_tensors(over)
    _on_threads(P, lambda r: ftar.ddp.allreduce_hook(states[r], Bucket(ts[r])).wait())
    for r in range(P):
        check(dt, _f16_bits(ts[r]), want, r)
        check_word(_f32_word(states[r].amax), word, r)
        assert float(states[r].found_inf()) == 0.0 and states[r].found_inf().is_cuda
    _on_threads(P, lambda r: ftar.ddp.allreduce_hook(states[r], Bucket(ts2[r])).wait())
    for r in range(P):
        check(dt, _f16_bits(ts2[r]), want2, r)
        assert _f32_word(states[r].amax) == INF32 and float(states[r].found_inf()) == 1.0
        assert states[r].calls == 2
        states[r].reset_amax()
        assert _f32_word(states[r].amax) == 0 and float(states[r].found_inf()) == 0.0


def test_ddp_hook_without_track_amax_is_todays_hook():
    """The default state: div_ by the world size, then op="sum" -- bit for bit, and no amax state."""
    import torch

    import ftar.ddp
    P, topo, dt = 4, "2,2", "f16"
    g = group(P)
    _settings(g)
    ins, _, _ = amax_ref.allreduce_case(dt, P, topo, N, "sum", 7)
    ts = _f16_tensors(ins)
    states = [ftar.ddp.HookState(g[r], topo=topo) for r in range(P)]
    _on_threads(P, lambda r: ftar.ddp.allreduce_hook(states[r], Bucket(ts[r])).wait())
    by_hand = _f16_tensors(ins)
    for t in by_hand:
        t.div_(P)
    g.allreduce_tensors(by_hand, op="sum", topo_=topo)
    torch.cuda.synchronize()
    for r in range(P):
        check(dt, _f16_bits(ts[r]), _f16_bits(by_hand[r]), r)
        assert states[r].amax is None and states[r].track_amax is False
    # and with tracking, average="divide" keeps the div_ and runs SUM: the same bits, plus their amax
    ts = _f16_tensors(ins)
    states = [ftar.ddp.HookState(g[r], topo=topo, track_amax=True) for r in range(P)]
    _on_threads(P, lambda r: ftar.ddp.allreduce_hook(states[r], Bucket(ts[r])).wait())
    for r in range(P):
        check(dt, _f16_bits(ts[r]), _f16_bits(by_hand[r]), r)
        check_word(_f32_word(states[r].amax), amax_ref.amax_bits(dt, _f16_bits(by_hand[r])), r)
