"""GPU tests of the scaled casts (include/ftar.h: ftar_cast_scaled) and of the fp8-compressed DDP hook built on
them (ftar.ddp.fp8_compress_hook).

Every cast is compared bit for bit (NaN lanes as "NaN or not") with tests/cast_ref.py, whose pieces are held against
torch on the CPU by tests/test_cast_api.py; the amax word with tests/amax_ref.py's reading of the expected
destination.  The double-rounding witnesses of cast_ref are planted at every edge of the launched kernel's tile, in
the head and the tail of an unaligned call and in the element-wise kernel: a path that rounds the product once
fails there and nowhere else."""
import threading

import numpy as np
import pytest

import amax_ref
import cast_ref
import kernel_edges
from gpu_util import filled_dev, from_dev, to_dev

pytestmark = pytest.mark.gpu

INF32 = 0x7F800000
PAIRS = cast_ref.PAIRS
NS = [1, 15, 16, 17, 255, 4099, 100_003]
HALF = 0x3F000000


def esz(dt):
    return np.dtype(cast_ref.storage(dt)).itemsize


def scale_dev(r_bits):
    return None if r_bits is None else to_dev(np.array([r_bits], np.uint32))


def run_cast(src_dt, dst_dt, bits, r_bits=None, src_off=0, dst_off=0, amax=False, plain=True):
    """ftar.cast_scaled on a fresh device copy of `bits` at element offset src_off, into a destination at element
    offset dst_off: the stored bits (and the amax word; with `plain` the call without amax must store the same)."""
    import ftar
    bits = np.ascontiguousarray(bits).view(cast_ref.storage(src_dt))
    n = bits.size
    sc = scale_dev(r_bits)

    def launch(am):
        src_t, src = to_dev(bits, offset_elems=src_off)
        dst_t, dst = filled_dev((n + dst_off) * esz(dst_dt) + 64)
        dst += dst_off * esz(dst_dt)
        ftar.cast_scaled(src, dst, n, src_dt, dst_dt, scale=None if sc is None else sc[1], amax=am)
        got = from_dev(dst_t, cast_ref.storage(dst_dt), n, dst_off)
        assert from_dev(src_t, bits.dtype, n, src_off).tobytes() == bits.tobytes(), "the source is read only"
        return got
    if not amax:
        return launch(None)
    am_t, am = filled_dev(4)            # 0xA5A5A5A5: a stale word to overwrite
    got = launch(am)
    word = int(from_dev(am_t, np.uint32, 1)[0])
    if plain:
        assert cast_ref.same_bits(dst_dt, launch(None), got), "the amax call stores the plain call's bits"
    return got, word


def check(dt, got, want, what=""):
    assert cast_ref.same_bits(dt, got, want), (what, cast_ref.first_diff(dt, got, want))


def check_word(got, want, what=""):
    assert amax_ref.matches(got, want), (what, hex(int(got)), want if want == amax_ref.NAN else hex(want))


def inputs(dt, n, seed=1):
    """n finite elements of dt: |x| < 1 for the wide formats, |x| < 2 for fp8, with a few specials planted past
    lane 0 (an inf where the format has one, a NaN, -0, the largest finite value, the smallest subnormal)."""
    x = amax_ref.base_sources(dt, 2, max(n, 2), seed)[0][:n].copy()
    u, _, first_special = amax_ref.LAYOUT[dt]
    sign = 1 << (8 * np.dtype(u).itemsize - 1)
    for at, enc in ((7, first_special), (9, sign), (10, first_special - 1), (12, 1), (13, sign | first_special),
                    (14, first_special | 1 if dt != "f8e4m3" else first_special)):
        if at < n:
            x[at] = enc
    return x


def kernel():
    import ftar
    return ftar.names.kernel_symbol(ftar.last_kernel())


def tile_elems(symbol):
    """The elements one workgroup of a launched cast_vec*_kernel<Src, Dst, U, BS, LAYOUT> covers per pass."""
    name, a = kernel_edges.template_args(symbol)
    assert name in ("cast_vec_kernel", "cast_vec_amax_kernel"), symbol
    return int(a[-3]) * int(a[-2]) * 16


# ---- every pair, every size -----------------------------------------------------------------------------
def _size_cases():
    """The product trimmed as tests/test_gpu_avg.py trims its own: every pair sees every n, the scales alternating,
    plus the largest n at the other scale."""
    out = []
    for pi, (s, d) in enumerate(PAIRS):
        for i, n in enumerate(NS):
            out.append((s, d, n, (i + pi) % 2 == 0))
        out.append((s, d, NS[-1], pi % 2 == 0))
    return sorted(set(out))


@pytest.mark.parametrize("src,dst,n,scaled", _size_cases())
def test_every_pair_and_size_against_the_reference(src, dst, n, scaled):
    r = cast_ref.THIRD if scaled else None
    x = inputs(src, n)
    check(dst, run_cast(src, dst, x, r), cast_ref.cast(src, dst, x, r), kernel())


# ---- exhaustive sources ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", cast_ref.F8)
@pytest.mark.parametrize("src", ["bf16", "f16"])
def test_every_16_bit_encoding_quantizes_as_the_reference(src, dst):
    x = np.arange(65536, dtype=np.uint16)
    for r in cast_ref.SCALES:
        check(dst, run_cast(src, dst, x, r), cast_ref.cast(src, dst, x, r), hex(r))


@pytest.mark.parametrize("dst", cast_ref.WIDE)
@pytest.mark.parametrize("src", cast_ref.F8)
def test_every_fp8_encoding_dequantizes_as_the_reference(src, dst):
    x = np.resize(np.arange(256, dtype=np.uint8), 4099)
    for r in cast_ref.SCALES:
        check(dst, run_cast(src, dst, x, r), cast_ref.cast(src, dst, x, r), hex(r))


@pytest.mark.parametrize("low", [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], ids=hex)
@pytest.mark.parametrize("dst", cast_ref.F8)
def test_every_f32_high_half_quantizes_as_the_reference(dst, low):
    """The multiply-then-convert path on all 2^16 high halves over each low half around the fp32 -> fp8 ties (the
    conversion instruction alone is pinned on all 2^32 floats by tests/test_gpu_f8.py)."""
    x = (np.arange(65536, dtype=np.uint32) << np.uint32(16)) | np.uint32(low)
    for r in cast_ref.SCALES:
        check(dst, run_cast("f32", dst, x, r), cast_ref.cast("f32", dst, x, r), hex(r))


@pytest.mark.parametrize("name", sorted(cast_ref.ODD_SCALES))
@pytest.mark.parametrize("src,dst", PAIRS)
def test_a_scale_of_any_bit_pattern_is_ieee_multiplication(src, dst, name):
    r = cast_ref.ODD_SCALES[name]
    x = inputs(src, 4099, seed=2)
    check(dst, run_cast(src, dst, x, r), cast_ref.cast(src, dst, x, r), name)


# ---- the double-rounding witnesses ----------------------------------------------------------------------
def _witness_run(src, dst, n, positions, src_off=0, dst_off=0, family="cast_vec_kernel"):
    for x, r, twice, once in cast_ref.witnesses(dst, src):
        bits = inputs(src, n, seed=3)
        for p in positions:
            bits[p] = x
        want = cast_ref.cast(src, dst, bits, r)
        got = run_cast(src, dst, bits, r, src_off=src_off, dst_off=dst_off)
        assert kernel().startswith(family + "<"), kernel()
        for p in positions:
            assert int(want[p]) == twice != once
            assert int(got[p]) == twice, (p, hex(int(got[p])), "two roundings:", hex(twice), "one:", hex(once))
        check(dst, got, want, (hex(x), hex(r)))


@pytest.mark.parametrize("src,dst", cast_ref.witness_pairs())
def test_witnesses_at_every_tile_edge_round_twice(src, dst):
    import ftar
    run_cast(src, dst, inputs(src, 4099))
    T = tile_elems(kernel())
    n = 2 * T + 16 * 64 + 37
    pos = sorted({0, 1, n - 2, n - 1, 16 * 64 - 1, 16 * 64, T - 1, T})
    _witness_run(src, dst, n, pos)
    assert ftar.last_kernel() is not None


@pytest.mark.parametrize("src,dst", cast_ref.witness_pairs())
def test_witnesses_in_the_head_and_tail_of_an_unaligned_call_round_twice(src, dst):
    """Both pointers 4 elements behind a 16-byte boundary: a head of 12 elements, then vectors, then a tail."""
    n = 12 + 16 * 300 + 9
    _witness_run(src, dst, n, list(range(12)) + list(range(n - 9, n)), src_off=4, dst_off=4)


@pytest.mark.parametrize("src,dst", cast_ref.witness_pairs())
def test_witnesses_in_the_element_wise_kernel_round_twice(src, dst):
    n = 4099
    narrow_is_dst = cast_ref.is_f8(dst)
    _witness_run(src, dst, n, [0, 1, 255, 256, 2048, n - 2, n - 1], src_off=0 if narrow_is_dst else 1,
                 dst_off=1 if narrow_is_dst else 0, family="cast_elem_kernel")


# ---- alignment and the kernel reached -------------------------------------------------------------------
@pytest.mark.parametrize("narrow_off,wide_off,family", [(4, 4, "cast_vec"), (1, 0, "cast_elem"), (0, 1, "cast_elem"),
                                                        (0, 0, "cast_vec"), (16, 8, "cast_vec"), (3, 4, "cast_elem")])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_alignment_cases_and_the_kernel_reached(src, dst, narrow_off, wide_off, family):
    n = 4099
    quant = cast_ref.is_f8(dst)
    so, do = (wide_off, narrow_off) if quant else (narrow_off, wide_off)
    x = inputs(src, n, seed=4)
    want = cast_ref.cast(src, dst, x, cast_ref.THIRD)
    check(dst, run_cast(src, dst, x, cast_ref.THIRD, src_off=so, dst_off=do), want)
    assert kernel().startswith(family + "_kernel<"), kernel()
    got, word = run_cast(src, dst, x, cast_ref.THIRD, src_off=so, dst_off=do, amax=True, plain=False)
    assert kernel().startswith(family + "_amax_kernel<"), kernel()
    check(dst, got, want)
    check_word(word, amax_ref.amax_bits(dst, want))


# ---- write footprint ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off,doff", [(1, 0, 0), (17, 5, 5), (4099, 0, 0), (4099, 4, 4), (100_003, 1, 1), (4099, 1, 0),
                                        (4099, 0, 3)])
@pytest.mark.parametrize("src,dst", [("f32", "f8e4m3"), ("bf16", "f8e5m2"), ("f8e4m3", "f16"), ("f8e5m2", "f32")])
def test_write_footprint_is_the_n_elements_and_the_one_word(src, dst, n, off, doff):
    """Guarded arenas around the destination and the amax word: exactly n elements and, with amax, the 4 bytes of
    the word are written; the source arena is unchanged.  off / doff: the source / destination pointer that many
    elements past a 16-byte boundary (equal offsets are co-aligned, with a head of 16 - off elements; unequal ones
    take the element-wise kernel)."""
    import torch

    import ftar
    x = inputs(src, n, seed=5)
    want = cast_ref.cast(src, dst, x, HALF)
    sa = kernel_edges.Arena((n + off) * esz(src) + 16)
    sa.upload(off * esz(src), x)
    da = kernel_edges.Arena((n + doff) * esz(dst) + 16)
    am = kernel_edges.Arena(64)
    sc = scale_dev(HALF)
    lo, hi = doff * esz(dst), (doff + n) * esz(dst)
    for word_at in (None, 16):
        ftar.cast_scaled(sa.ptr(off * esz(src)), da.ptr(lo), n, src, dst, scale=sc[1],
                         amax=None if word_at is None else am.ptr(word_at))
        torch.cuda.synchronize()
        got = da.window(lo, hi).cpu().numpy().view(cast_ref.storage(dst))
        check(dst, got, want, word_at)
        assert kernel_edges.check_untouched(da, lo, hi) is None
        assert kernel_edges.check_untouched(sa) is None
        if word_at is None:
            assert kernel_edges.check_untouched(am) is None
        else:
            assert kernel_edges.check_untouched(am, 16, 20) is None
            check_word(int(am.window(16, 20).cpu().numpy().view(np.uint32)[0]), amax_ref.amax_bits(dst, want))
        da.restore(lo, hi)


# ---- amax -----------------------------------------------------------------------------------------------
def _peaked(src, n, p):
    """Finite inputs (|x| < 2) with -64 at p."""
    x = amax_ref.base_sources(src, 2, max(n, 2), 6)[0][:n].copy()
    x[p] = amax_ref.encode(src, -64.0)
    return x


@pytest.mark.parametrize("n", [4099, 100_003])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_amax_finds_the_peak_at_every_edge(src, dst, n):
    run_cast(src, dst, _peaked(src, n, 0), amax=True, plain=False)
    T = tile_elems(kernel())
    for p in sorted({0, 1, n - 2, n - 1, 16 * 64 - 1, 16 * 64, T - 1, T}):
        if not 0 <= p < n:
            continue
        x = _peaked(src, n, p)
        r = HALF if p % 2 else None
        want = cast_ref.cast(src, dst, x, r)
        got, word = run_cast(src, dst, x, r, amax=True, plain=p == 0)
        check(dst, got, want, p)
        check_word(word, amax_ref.checked(dst, want, p), p)
        assert word == amax_ref.widen(dst, amax_ref.encode(dst, 32.0 if p % 2 else 64.0))


@pytest.mark.parametrize("src,dst", PAIRS)
def test_amax_specials(src, dst):
    u = cast_ref.storage(src)
    sign = 1 << (8 * np.dtype(u).itemsize - 1)
    n = 4099
    # all zeros, some of them -0: bits 0
    x = np.zeros(n, u)
    x[[0, 5, 2048, n - 1]] = sign
    got, word = run_cast(src, dst, x, amax=True)
    check(dst, got, cast_ref.cast(src, dst, x))
    assert word == 0
    # a subnormal-only peak is kept (where the product stays representable: a wide source's smallest subnormal
    # underflows fp8 to zero, so the peak is the destination's own subnormal 3 ulp)
    x = np.zeros(n, u)
    x[4000] = sign | 3 if cast_ref.is_f8(src) else amax_ref.encode(src, -float(cast_ref.frac_of(dst, 3)))
    x[17] = 1 if cast_ref.is_f8(src) else amax_ref.encode(src, float(cast_ref.frac_of(dst, 1)))
    want = cast_ref.cast(src, dst, x)
    got, word = run_cast(src, dst, x, amax=True)
    check(dst, got, want)
    assert word == amax_ref.amax_bits(dst, want) != 0
    assert word == (amax_ref.widen(src, 3) if cast_ref.is_f8(src) else amax_ref.widen(dst, 3))
    # a NaN source gives NaN; an inf source +inf (e4m3 has no inf: as a source it cannot hold one, as a
    # destination it turns one into NaN)
    x = inputs(src, n, seed=7)
    x[7] = x[10] = x[13] = x[14] = 0
    x[300] = amax_ref.encode(src, float("nan"))
    got, word = run_cast(src, dst, x, amax=True)
    check(dst, got, cast_ref.cast(src, dst, x))
    check_word(word, amax_ref.NAN)
    if src != "f8e4m3":
        x[300] = amax_ref.encode(src, float("-inf"))
        want = cast_ref.cast(src, dst, x)
        got, word = run_cast(src, dst, x, amax=True)
        check(dst, got, want)
        check_word(word, amax_ref.NAN if dst == "f8e4m3" else INF32)
        assert amax_ref.amax_bits(dst, want) == (amax_ref.NAN if dst == "f8e4m3" else INF32)


@pytest.mark.parametrize("src", cast_ref.WIDE)
def test_e4m3_overflow_is_nan_at_scale_1_and_448_at_half(src):
    x = np.zeros(4099, cast_ref.storage(src))
    x[1000] = amax_ref.encode(src, 896.0)
    got, word = run_cast(src, "f8e4m3", x, cast_ref.ONE, amax=True)
    check("f8e4m3", got, cast_ref.cast(src, "f8e4m3", x, cast_ref.ONE))
    check_word(word, amax_ref.NAN)
    got, word = run_cast(src, "f8e4m3", x, HALF, amax=True)
    check("f8e4m3", got, cast_ref.cast(src, "f8e4m3", x, HALF))
    assert int(got[1000]) == 0x7E and word == 0x43E00000         # 448.0f
    got, word = run_cast(src, "f8e5m2", x, cast_ref.ONE, amax=True)      # e5m2 holds it
    assert word == amax_ref.widen("f8e5m2", amax_ref.encode("f8e5m2", 896.0))


def test_a_stale_word_is_overwritten_and_count_0_gives_plus_zero():
    import ftar
    src, dst, n = "bf16", "f8e4m3", 4099
    am_t, am = filled_dev(4)
    x = _peaked(src, n, 2000)
    s_t, s = to_dev(x)
    d_t, d = filled_dev(n)
    ftar.cast_scaled(s, d, n, src, dst, amax=am)
    check_word(int(from_dev(am_t, np.uint32, 1)[0]), amax_ref.widen(dst, amax_ref.encode(dst, 64.0)))
    x[2000] = 0
    s_t, s = to_dev(x)
    ftar.cast_scaled(s, d, n, src, dst, amax=am)
    small = amax_ref.amax_bits(dst, cast_ref.cast(src, dst, x))
    assert small != amax_ref.NAN and small < 0x42800000
    check_word(int(from_dev(am_t, np.uint32, 1)[0]), small)
    am_t, am = filled_dev(4)
    d_t, d = filled_dev(64)
    ftar.cast_scaled(s, d, 0, src, dst, amax=am)
    assert int(from_dev(am_t, np.uint32, 1)[0]) == 0
    ftar.cast_scaled(None, None, 0, src, dst, amax=am)
    assert int(from_dev(am_t, np.uint32, 1)[0]) == 0
    assert from_dev(d_t, np.uint8, 64).tolist() == [0xA5] * 64


def test_cast_scaled_tensor_and_refusals_leave_the_buffers():
    import torch

    import ftar
    n = 4099
    x = inputs("bf16", n, seed=8)
    src = torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.bfloat16)
    dst = torch.empty(n, dtype=torch.float8_e4m3fn, device="cuda")
    scale = torch.full((1,), 0.5, device="cuda")
    amax = torch.full((1,), -1.0, device="cuda")
    assert ftar.cast_scaled_tensor(src, dst, scale=scale, amax=amax) is dst
    torch.cuda.synchronize()
    want = cast_ref.cast("bf16", "f8e4m3", x, HALF)
    check("f8e4m3", dst.view(torch.uint8).cpu().numpy(), want)
    check_word(int(amax.view(torch.int32).cpu().numpy().view(np.uint32)[0]), amax_ref.amax_bits("f8e4m3", want))
    back = torch.empty(n, dtype=torch.float32, device="cuda")
    ftar.cast_scaled_tensor(dst, back, scale=torch.full((1,), 2.0, device="cuda"))
    torch.cuda.synchronize()
    check("f32", back.cpu().numpy().view(np.uint32), cast_ref.cast("f8e4m3", "f32", want, 0x40000000))
    # refused calls: the destination and the word keep their bytes
    d_t, d = filled_dev(n * 2)
    am_t, am = filled_dev(4)
    for sd, dd in (("bf16", "f16"), ("f32", "f32"), ("f64", "f8e4m3"), ("f8e4m3", "f8e5m2"), ("i32", "f8e4m3")):
        with pytest.raises(ftar.FtarError) as e:
            ftar.cast_scaled(src, d, n // 4, sd, dd, scale=scale, amax=am)
        assert e.value.status == 2
    with pytest.raises(ftar.FtarError) as e:
        ftar.cast_scaled(src, d, n, "bf16", "f8e4m3", scale=scale, amax=am + 2)
    assert e.value.status == 1
    assert from_dev(d_t, np.uint8, n * 2).tolist() == [0xA5] * (n * 2)
    assert int(from_dev(am_t, np.uint32, 1)[0]) == 0xA5A5A5A5


def test_cast_with_amax_captures_into_a_hip_graph_and_follows_the_device_scale():
    """A memset node and a kernel node; replayed twice with the scale tensor changed between the replays."""
    import torch

    import ftar
    src, dst, n = "f16", "f8e5m2", 100_003
    x = _peaked(src, n, 99_999)
    s = torch.from_numpy(x.view(np.int16).copy()).cuda()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    scale = torch.ones(1, device="cuda")
    am = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ftar.cast_scaled(s, out, n, src, dst, scale=scale, amax=am, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    for r_bits, r in ((cast_ref.ONE, 1.0), (0x3E800000, 0.25)):
        scale.fill_(r)
        am.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = cast_ref.cast(src, dst, x, r_bits)
        check(dst, out.cpu().numpy(), want, r)
        check_word(int(am.cpu().numpy().view(np.uint32)[0]), amax_ref.checked(dst, want, 99_999), r)


# ---- the fp8-compressed DDP hook ------------------------------------------------------------------------
N = 50_001
_groups = {}


def group(P):
    import ftar
    if P not in _groups:
        _groups[P] = ftar.Comm.init_local(P)
    return _groups[P]


class Bucket:
    """A stand-in for torch.distributed.GradBucket."""

    def __init__(self, t):
        self.t = t

    def buffer(self):
        return self.t


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


def _tensor(dt, bits):
    import torch
    if dt == "f32":
        return torch.from_numpy(bits.view(np.float32).copy()).cuda()
    tt = {"bf16": torch.bfloat16, "f16": torch.float16}[dt]
    return torch.from_numpy(bits.view(np.int16).copy()).cuda().view(tt)


def _bits_of(dt, t):
    import torch
    if dt == "f32":
        return t.cpu().numpy().view(np.uint32)
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _word(t):
    import torch
    return int(t.view(torch.int32).cpu().numpy().view(np.uint32)[0])


def _expect(dt, f8, ins, topo, scale_bits, inv_bits):
    """quantize -> the AVG schedule on the wire -> dequantize; (the bucket every rank ends with, the wire's amax)."""
    wire = [cast_ref.cast(dt, f8, x, scale_bits) for x in ins]
    red = amax_ref.schedule(f8, wire, topo, "avg")
    return cast_ref.cast(f8, dt, red, inv_bits), amax_ref.amax_bits(f8, red)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("topo,form", [("2,2", "direct"), ("1", "stages")])
def test_fp8_compress_hook_over_threads(topo, form, dt, fmt):
    """P = 4 ranks on threads, three buckets per rank: a finite one at scale 1; one whose lane p overflows the wire
    at the quantize (found_inf, then update_scale backs the scale off on the device); after reset_amax the first
    bucket again at the new scale, finite."""
    import torch

    import ftar.ddp
    P, p = 4, 4321
    f8 = "f8" + fmt
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather(form)
    g.set_reduce_scatter(form)
    ins = amax_ref.base_sources(dt, P, N, seed=9)
    want, word = _expect(dt, f8, ins, topo, cast_ref.ONE, cast_ref.ONE)
    assert word != amax_ref.NAN and 0 < word < INF32
    states = [ftar.ddp.Fp8CompressState(g[r], fmt=fmt, topo=topo) for r in range(P)]
    ts = [_tensor(dt, x) for x in ins]
    _on_threads(P, lambda r: ftar.ddp.fp8_compress_hook(states[r], Bucket(ts[r])).wait())
    for r in range(P):
        check(dt, _bits_of(dt, ts[r]), want, r)
        check_word(_word(states[r].amax), word, r)
        assert float(states[r].found_inf()) == 0.0 and states[r].found_inf().is_cuda
        assert float(states[r].scale) == 1.0 and float(states[r].inv_scale) == 1.0
    # a lane that overflows the wire on every rank: NaN (e4m3) / inf (e5m2) from the quantize on
    over = [x.copy() for x in amax_ref.base_sources(dt, P, N, seed=10)]
    for x in over:
        x[p] = amax_ref.encode(dt, 1024.0 if fmt == "e4m3" else 61440.0)
    want2, word2 = _expect(dt, f8, over, topo, cast_ref.ONE, cast_ref.ONE)
    assert word2 == (amax_ref.NAN if fmt == "e4m3" else INF32)
    ts2 = [_tensor(dt, x) for x in over]
    _on_threads(P, lambda r: ftar.ddp.fp8_compress_hook(states[r], Bucket(ts2[r])).wait())
    for r in range(P):
        check(dt, _bits_of(dt, ts2[r]), want2, r)
        check_word(_word(states[r].amax), word2, r)
        assert float(states[r].found_inf()) == 1.0
        states[r].update_scale()
        assert states[r].scale.is_cuda and float(states[r].scale) == 0.5 and float(states[r].inv_scale) == 2.0
        states[r].reset_amax()
        assert _word(states[r].amax) == 0 and float(states[r].found_inf()) == 0.0
    want3, word3 = _expect(dt, f8, ins, topo, HALF, 0x40000000)
    assert word3 != amax_ref.NAN and word3 < INF32
    ts3 = [_tensor(dt, x) for x in ins]
    _on_threads(P, lambda r: ftar.ddp.fp8_compress_hook(states[r], Bucket(ts3[r])).wait())
    for r in range(P):
        check(dt, _bits_of(dt, ts3[r]), want3, r)
        check_word(_word(states[r].amax), word3, r)
        assert float(states[r].found_inf()) == 0.0 and states[r].calls == 3
        assert bool(torch.isfinite(ts3[r].float()).all())


@pytest.mark.parametrize("topo,form", [("2,2", "direct"), ("1", "stages")])
@pytest.mark.parametrize("f8,nan", [("f8e4m3", 0x7F), ("f8e4m3", 0xFF), ("f8e5m2", 0x7E)])
def test_an_fp8_nan_on_the_wire_reaches_every_ranks_amax_word(f8, nan, topo, form):
    """What found_inf() stands on for e4m3, whose overflow is a NaN: one NaN byte in one rank's wire makes the
    AllReduce's amax a NaN on every rank.  (The fp8 conversions widen a NaN byte to a NaN with the sign set; the
    word must still be the largest of the ranks' words in the engine's integer maximum.)"""
    P, p = 4, 4321
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather(form)
    g.set_reduce_scatter(form)
    ins = [x.copy() for x in amax_ref.base_sources(f8, P, N, seed=11)]
    ins[1][p] = nan
    want = amax_ref.schedule(f8, ins, topo, "avg")
    assert amax_ref.amax_bits(f8, want) == amax_ref.NAN
    bufs = [to_dev(x) for x in ins]
    ams = [filled_dev(4) for _ in range(P)]
    g.allreduce(None, [q for _, q in bufs], N, f8, "avg", topo_=topo, amaxes=[q for _, q in ams])
    for r in range(P):
        check(f8, from_dev(bufs[r][0], np.uint8, N), want, r)
        check_word(int(from_dev(ams[r][0], np.uint32, 1)[0]), amax_ref.NAN, r)


def test_fp8_compress_hook_refuses_an_i32_bucket_before_any_device_work():
    import torch

    import ftar.ddp
    state = ftar.ddp.Fp8CompressState(group(4)[0], topo="2,2")
    t = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ftar.ddp.fp8_compress_hook(state, Bucket(t))
    torch.cuda.synchronize()
    assert bool((t == 7).all()) and state.scale is None and state.calls == 0
