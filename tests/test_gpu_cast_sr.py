"""GPU tests of the stochastic-rounding quantize (include/ftar.h: ftar_cast_scaled_sr) and of the fp8-compressed DDP
hook with rounding="stochastic".

Every comparison is bit for bit (NaN lanes as "NaN or not") with tests/sr_ref.py, which tests/test_sr_api.py holds
against its own definition on the CPU.  Calls through the generator compare with sr_ref.sr_cast; calls through the
bench library's words hook (ftar_bench_cast_sr_words: the production kernels and narrowing on an explicit array of
words) compare with sr_ref.sr_cast_words, which is how chosen words -- the thresholds 2^32 - F and 2^32 - F - 1
among them -- reach every source encoding."""
import ctypes
import threading

import numpy as np
import pytest

import amax_ref
import cast_ref
import kernel_edges
import sr_ref
from gpu_util import filled_dev, from_dev, to_dev

pytestmark = pytest.mark.gpu

INF32 = 0x7F800000
QUANT = [(w, f) for w in cast_ref.WIDE for f in cast_ref.F8]
LOWS = (0x0001, 0x7FFF, 0x8000, 0xFFFF)
TOP = (1 << 32) - 1
SEED = 0x0123456789ABCDEF
HALF = 0x3F000000


def esz(dt):
    return np.dtype(cast_ref.storage(dt)).itemsize


def scale_dev(r_bits):
    return None if r_bits is None else to_dev(np.array([r_bits], np.uint32))


def seed_dev(seed):
    return to_dev(np.array([seed & sr_ref.M64], np.uint64))


def run_sr(src_dt, dst_dt, bits, r_bits=None, seed=SEED, offset=0, src_off=0, dst_off=0, amax=False):
    """ftar.cast_scaled(..., rounding="stochastic") on a fresh device copy of `bits` at element offset src_off, into
    a destination at element offset dst_off: the stored bits, and with amax (the stored bits, the word)."""
    import ftar
    bits = np.ascontiguousarray(bits).view(cast_ref.storage(src_dt))
    n = bits.size
    sc = scale_dev(r_bits)
    sd = seed_dev(seed)
    src_t, src = to_dev(bits, offset_elems=src_off)
    dst_t, dst = filled_dev((n + dst_off) * esz(dst_dt) + 64)
    dst += dst_off * esz(dst_dt)
    am_t, am = filled_dev(4)
    ftar.cast_scaled(src, dst, n, src_dt, dst_dt, scale=None if sc is None else sc[1], amax=am if amax else None,
                     rounding="stochastic", seed=sd[1], offset=offset)
    got = from_dev(dst_t, np.uint8, n, dst_off)
    assert from_dev(src_t, bits.dtype, n, src_off).tobytes() == bits.tobytes(), "the source is read only"
    assert int(from_dev(sd[0], np.uint64, 1)[0]) == seed & sr_ref.M64, "the seed is read only"
    if not amax:
        assert int(from_dev(am_t, np.uint32, 1)[0]) == 0xA5A5A5A5
        return got
    return got, int(from_dev(am_t, np.uint32, 1)[0])


_words_hook = None


def run_words(src_dt, dst_dt, bits, w, r_bits=None):
    """The production stochastic cast on the explicit words w (ftar_bench_cast_sr_words)."""
    global _words_hook
    import torch

    import ftar
    if _words_hook is None:
        _words_hook = ftar.bench_lib().ftar_bench_cast_sr_words
        vp = ctypes.c_void_p
        _words_hook.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_size_t, vp, vp, vp]
    bits = np.ascontiguousarray(bits).view(cast_ref.storage(src_dt))
    n = bits.size
    w = np.broadcast_to(np.asarray(w, dtype=np.uint32), (n,)).copy()
    sc = scale_dev(r_bits)
    src_t, src = to_dev(bits)
    w_t, wp = to_dev(w)
    dst_t, dst = filled_dev(n + 64)
    st = _words_hook(src, cast_ref.ID[src_dt], dst, cast_ref.ID[dst_dt], n, None if sc is None else sc[1], wp, None)
    assert st == 0, (st, ftar.last_error())
    torch.cuda.synchronize()
    assert from_dev(dst_t, np.uint8, 64, n).tolist() == [0xA5] * 64
    return from_dev(dst_t, np.uint8, n)


def check(dt, got, want, what=""):
    assert cast_ref.same_bits(dt, got, want), (what, cast_ref.first_diff(dt, got, want))


def check_word(got, want, what=""):
    assert amax_ref.matches(got, want), (what, hex(int(got)), want if want == amax_ref.NAN else hex(want))


def inputs(dt, n, seed=1):
    """n elements of a wide dt, |x| < 1, with a few specials planted past lane 0: inf, -0, the largest finite value,
    the smallest subnormal, -inf, a NaN."""
    x = amax_ref.base_sources(dt, 2, max(n, 2), seed)[0][:n].copy()
    u, _, first_special = amax_ref.LAYOUT[dt]
    sign = 1 << (8 * np.dtype(u).itemsize - 1)
    for at, enc in ((7, first_special), (9, sign), (10, first_special - 1), (12, 1), (13, sign | first_special),
                    (14, first_special | 1)):
        if at < n:
            x[at] = enc
    return x


def kernel():
    import ftar
    return ftar.names.kernel_symbol(ftar.last_kernel())


def tile_elems(symbol):
    """The elements one workgroup of a launched cast_vec_sr*_kernel<Rd, Src, Dst, U, BS, LAYOUT> covers per pass."""
    name, a = kernel_edges.template_args(symbol)
    assert name in ("cast_vec_sr_kernel", "cast_vec_sr_amax_kernel"), symbol
    return int(a[-3]) * int(a[-2]) * 16


_tiles = {}


def tile(src, dst):
    if (src, dst) not in _tiles:
        run_sr(src, dst, inputs(src, 4099))
        _tiles[src, dst] = tile_elems(kernel())
    return _tiles[src, dst]


# ---- every pair, every size -----------------------------------------------------------------------------
SIZES = ["1", "15", "16", "17", "tile-1", "tile", "tile+1", "2*tile+5", "100003"]


def _n(label, T):
    return {"tile-1": T - 1, "tile": T, "tile+1": T + 1, "2*tile+5": 2 * T + 5}.get(label) or int(label)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("src,dst", QUANT)
def test_every_pair_and_size_against_the_reference(src, dst, size):
    """With and without a scale, with and without amax: the same bits either way of the latter."""
    n = _n(size, tile(src, dst))
    x = inputs(src, n)
    pi = QUANT.index((src, dst)) + SIZES.index(size)
    for r in (None, cast_ref.SCALES[1 + pi % (len(cast_ref.SCALES) - 1)]):
        want = sr_ref.sr_cast(src, dst, x, r, SEED, 3)
        check(dst, run_sr(src, dst, x, r, SEED, 3), want, (kernel(), r))
        got, word = run_sr(src, dst, x, r, SEED, 3, amax=True)
        check(dst, got, want, (kernel(), r, "amax"))
        check_word(word, amax_ref.amax_bits(dst, want), r)


def test_rne_calls_still_reach_the_rne_kernels():
    import ftar
    x = inputs("bf16", 4099)
    t, p = to_dev(x)
    d_t, d = filled_dev(4099)
    ftar.cast_scaled(p, d, 4099, "bf16", "f8e4m3")
    assert kernel().startswith("cast_vec_kernel<"), kernel()
    ftar.cast_scaled(p, d, 4099, "bf16", "f8e4m3", rounding="nearest", seed=None, offset=7)
    assert kernel().startswith("cast_vec_kernel<"), kernel()
    check("f8e4m3", from_dev(d_t, np.uint8, 4099), cast_ref.cast("bf16", "f8e4m3", x))
    ftar.cast_scaled(p, d + 1, 4098, "bf16", "f8e4m3")
    assert kernel().startswith("cast_elem_kernel<"), kernel()


# ---- every source encoding under chosen words -------------------------------------------------------------
def _word_sets(dst, p_bits):
    F = sr_ref.frac32(dst, p_bits).astype(np.uint64)
    thr = ((np.uint64(1) << np.uint64(32)) - F) & np.uint64(TOP)
    return [("0", 0), ("1", 1), ("2^31", 1 << 31), ("2^32-1", TOP), ("threshold", thr.astype(np.uint32)),
            ("threshold-1", ((thr - np.uint64(1)) & np.uint64(TOP)).astype(np.uint32))]


@pytest.mark.parametrize("dst", cast_ref.F8)
@pytest.mark.parametrize("src", ["bf16", "f16"])
def test_every_16_bit_encoding_under_the_edge_words(src, dst):
    x = np.arange(65536, dtype=np.uint16)
    for name, w in _word_sets(dst, sr_ref.product_bits(src, x)):
        check(dst, run_words(src, dst, x, w), sr_ref.sr_cast_words(src, dst, x, None, w), name)


@pytest.mark.parametrize("low", LOWS, ids=hex)
@pytest.mark.parametrize("dst", cast_ref.F8)
def test_every_f32_high_half_under_the_edge_words(dst, low):
    x = (np.arange(65536, dtype=np.uint32) << np.uint32(16)) | np.uint32(low)
    for name, w in _word_sets(dst, x):
        check(dst, run_words("f32", dst, x, w), sr_ref.sr_cast_words("f32", dst, x, None, w), name)


@pytest.mark.parametrize("dst", cast_ref.F8)
def test_the_words_hook_and_the_generator_agree(dst):
    x = inputs("f32", 4099, seed=2)
    w = sr_ref.words(SEED, sr_ref.indices(5, 4099))
    check(dst, run_words("f32", dst, x, w, cast_ref.THIRD), run_sr("f32", dst, x, cast_ref.THIRD, SEED, 5))


# ---- the word is a function of the seed and the global index alone ----------------------------------------
@pytest.mark.parametrize("narrow_off,wide_off,family", [(0, 0, "cast_vec_sr"), (4, 4, "cast_vec_sr"),
                                                        (1, 0, "cast_elem_sr"), (0, 1, "cast_elem_sr")])
@pytest.mark.parametrize("src,dst", QUANT)
def test_pointer_offsets_change_the_kernel_not_the_bits(src, dst, narrow_off, wide_off, family):
    n = 4099
    x = inputs(src, n, seed=4)
    want = sr_ref.sr_cast(src, dst, x, cast_ref.THIRD, SEED, 11)
    check(dst, run_sr(src, dst, x, cast_ref.THIRD, SEED, 11, src_off=wide_off, dst_off=narrow_off), want)
    assert kernel().startswith(family + "_kernel<"), kernel()
    got, word = run_sr(src, dst, x, cast_ref.THIRD, SEED, 11, src_off=wide_off, dst_off=narrow_off, amax=True)
    assert kernel().startswith(family + "_amax_kernel<"), kernel()
    check(dst, got, want)
    check_word(word, amax_ref.amax_bits(dst, want))


@pytest.mark.parametrize("src,dst", QUANT)
def test_one_call_equals_two_calls_split_anywhere(src, dst):
    T = tile(src, dst)
    n = 2 * T + 5
    x = inputs(src, n, seed=5)
    whole = run_sr(src, dst, x, HALF, SEED, 1000)
    check(dst, whole, sr_ref.sr_cast(src, dst, x, HALF, SEED, 1000))
    for a in (1, 16, T - 1, T + 1):
        parts = np.concatenate([run_sr(src, dst, x[:a], HALF, SEED, 1000), run_sr(src, dst, x[a:], HALF, SEED, 1000 + a)])
        assert parts.tobytes() == whole.tobytes(), a


@pytest.mark.parametrize("offset,n", [((1 << 32) - 8, 4099), (1 << 63, 4099), ((1 << 64) - 5, 17)], ids=hex)
@pytest.mark.parametrize("src,dst", [("bf16", "f8e4m3"), ("f32", "f8e5m2")])
def test_offsets_across_2_32_and_at_2_63(src, dst, offset, n):
    x = inputs(src, n, seed=6)
    for so, do in ((0, 0), (0, 1)):
        check(dst, run_sr(src, dst, x, None, SEED, offset, src_off=so, dst_off=do), sr_ref.sr_cast(src, dst, x, None, SEED, offset),
              (so, do))


def test_seeds_give_different_bits_and_the_reference_follows_each():
    x = inputs("bf16", 4099, seed=7)
    outs = []
    for seed in (0, 1, SEED, SEED + 1, sr_ref.M64):
        got = run_sr("bf16", "f8e4m3", x, cast_ref.THIRD, seed)
        check("f8e4m3", got, sr_ref.sr_cast("bf16", "f8e4m3", x, cast_ref.THIRD, seed), hex(seed))
        outs.append(got.tobytes())
    assert len(set(outs)) == len(outs)


# ---- write footprint ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off,doff", [(1, 0, 0), (17, 5, 5), (4099, 0, 0), (4099, 4, 4), (100_003, 1, 1), (4099, 1, 0),
                                        (4099, 0, 3)])
@pytest.mark.parametrize("src,dst", [("f32", "f8e4m3"), ("bf16", "f8e5m2"), ("f16", "f8e4m3")])
def test_write_footprint_is_the_n_bytes_and_the_one_word(src, dst, n, off, doff):
    import torch

    import ftar
    x = inputs(src, n, seed=5)
    want = sr_ref.sr_cast(src, dst, x, HALF, SEED, 77)
    sa = kernel_edges.Arena((n + off) * esz(src) + 16)
    sa.upload(off * esz(src), x)
    da = kernel_edges.Arena(n + doff + 16)
    am = kernel_edges.Arena(64)
    sd = kernel_edges.Arena(64)
    sd.upload(8, np.array([SEED], np.uint64))
    sc = scale_dev(HALF)
    lo, hi = doff, doff + n
    for word_at in (None, 16):
        ftar.cast_scaled(sa.ptr(off * esz(src)), da.ptr(lo), n, src, dst, scale=sc[1],
                         amax=None if word_at is None else am.ptr(word_at), rounding="stochastic", seed=sd.ptr(8), offset=77)
        torch.cuda.synchronize()
        check(dst, da.window(lo, hi).cpu().numpy(), want, word_at)
        assert kernel_edges.check_untouched(da, lo, hi) is None
        assert kernel_edges.check_untouched(sa) is None
        assert kernel_edges.check_untouched(sd) is None
        if word_at is None:
            assert kernel_edges.check_untouched(am) is None
        else:
            assert kernel_edges.check_untouched(am, 16, 20) is None
            check_word(int(am.window(16, 20).cpu().numpy().view(np.uint32)[0]), amax_ref.amax_bits(dst, want))
        da.restore(lo, hi)


# ---- specials ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", cast_ref.F8)
def test_specials_under_every_word(dst):
    nan, inf, ninf, nz, tiny, ntiny = 0x7FC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x80000001
    x = np.zeros(4099, np.uint32)
    at = [0, 5, 16, 17, 1023, 4098, 2000]
    x[at] = [nan, inf, ninf, nz, tiny, ntiny, nan | 0x80000000]
    for w in (0, 1, 1 << 31, TOP):
        got = run_words("f32", dst, x, w)
        check(dst, got, sr_ref.sr_cast_words("f32", dst, x, None, w), w)
        assert [int(got[i]) for i in (17, 1023, 4098)] == [0x80, 0x00, 0x80]
        assert (int(got[5]) & 0x7F, int(got[16]) & 0x7F) == ((0x7C, 0x7C) if dst == "f8e5m2" else (0x7F, 0x7F))
        assert int(got[16]) & 0x80 or dst == "f8e4m3"
        assert not np.delete(got, at).any()


@pytest.mark.parametrize("dst,lo,hi,top,last", [("f8e4m3", 448.0, 480.0, 0x7F, 0x7E), ("f8e5m2", 57344.0, 65536.0, 0x7C, 0x7B)])
def test_the_overflow_band_with_threshold_words_on_both_sides(dst, lo, hi, top, last):
    x = np.linspace(lo, hi, 4099, dtype=np.float32).view(np.uint32)
    x[1::2] |= np.uint32(0x80000000)
    F = sr_ref.frac32(dst, x).astype(np.uint64)
    thr = ((np.uint64(1) << np.uint64(32)) - F) & np.uint64(TOP)
    up = run_words("f32", dst, x, thr.astype(np.uint32))
    down = run_words("f32", dst, x, ((thr - np.uint64(1)) & np.uint64(TOP)).astype(np.uint32))
    check(dst, up, sr_ref.sr_cast_words("f32", dst, x, None, thr.astype(np.uint32)))
    check(dst, down, sr_ref.sr_cast_words("f32", dst, x, None, ((thr - np.uint64(1)) & np.uint64(TOP)).astype(np.uint32)))
    inside = slice(1, 4098)
    assert ((up[inside] & 0x7F) >= top).all() and ((down[inside] & 0x7F) == last).all()
    assert int(up[0]) == int(down[0]) == last and (int(up[4098]) & 0x7F) >= top and (int(down[4098]) & 0x7F) >= top
    for w in (0, TOP):      # from the band's end on: always
        got = run_words("f32", dst, np.array([hi, -hi, 2 * hi, 3e38], np.float32).view(np.uint32), w)
        assert ((got & 0x7F) >= top).all()


@pytest.mark.parametrize("src,dst", QUANT)
def test_amax_sees_a_nan_and_an_inf(src, dst):
    n = 4099
    x = inputs(src, n, seed=7)
    x[7] = x[10] = x[13] = x[14] = 0
    want = sr_ref.sr_cast(src, dst, x, None, SEED)
    got, word = run_sr(src, dst, x, None, SEED, amax=True)
    check(dst, got, want)
    check_word(word, amax_ref.amax_bits(dst, want))
    assert word != amax_ref.NAN and word < INF32
    x[300] = amax_ref.encode(src, float("nan"))
    got, word = run_sr(src, dst, x, None, SEED, amax=True)
    check(dst, got, sr_ref.sr_cast(src, dst, x, None, SEED))
    check_word(word, amax_ref.NAN)
    x[300] = amax_ref.encode(src, float("-inf"))
    got, word = run_sr(src, dst, x, None, SEED, amax=True)
    check(dst, got, sr_ref.sr_cast(src, dst, x, None, SEED))
    check_word(word, amax_ref.NAN if dst == "f8e4m3" else INF32)
    # an overflow at the quantize: 1024 into e4m3 is NaN, 2^17 into e5m2 inf
    x[300] = amax_ref.encode(src, 1024.0)
    got, word = run_sr(src, dst, x, 0x43000000 if dst == "f8e5m2" else None, SEED, amax=True)      # x 128
    check_word(word, amax_ref.NAN if dst == "f8e4m3" else INF32)
    # all zeros, some of them -0: bits 0
    z = np.zeros(n, cast_ref.storage(src))
    z[[0, 5, 2048, n - 1]] = 1 << (8 * esz(src) - 1)
    got, word = run_sr(src, dst, z, None, SEED, amax=True)
    assert word == 0 and [int(got[i]) for i in (0, 5, 2048, n - 1)] == [0x80] * 4 and not np.delete(got, [0, 5, 2048, n - 1]).any()


@pytest.mark.parametrize("name", sorted(cast_ref.ODD_SCALES))
@pytest.mark.parametrize("src,dst", QUANT)
def test_a_scale_of_any_bit_pattern_is_ieee_multiplication(src, dst, name):
    r = cast_ref.ODD_SCALES[name]
    x = inputs(src, 4099, seed=2)
    check(dst, run_sr(src, dst, x, r, SEED, 9), sr_ref.sr_cast(src, dst, x, r, SEED, 9), name)


def test_count_0_gives_plus_zero_and_touches_nothing_else():
    import ftar
    am_t, am = filled_dev(4)
    d_t, d = filled_dev(64)
    sd = seed_dev(SEED)
    ftar.cast_scaled(None, None, 0, "bf16", "f8e4m3", amax=am, rounding="stochastic", seed=sd[1])
    assert int(from_dev(am_t, np.uint32, 1)[0]) == 0
    assert from_dev(d_t, np.uint8, 64).tolist() == [0xA5] * 64


# ---- graph capture ----------------------------------------------------------------------------------------
def test_the_sr_cast_with_amax_captures_and_follows_the_device_seed_and_scale():
    """A memset node and a kernel node; replayed with the seed tensor, then the scale tensor, changed."""
    import torch

    import ftar
    src, dst, n = "f16", "f8e5m2", 100_003
    x = inputs(src, n, seed=8)
    x[7] = x[13] = x[14] = 0
    s = torch.from_numpy(x.view(np.int16).copy()).cuda()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    scale = torch.ones(1, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    am = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ftar.cast_scaled(s, out, n, src, dst, scale=scale, amax=am, stream=side, rounding="stochastic", seed=seed,
                             offset=123)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for sv, r_bits, r in ((5, cast_ref.ONE, 1.0), (6, cast_ref.ONE, 1.0), (6, 0x3E800000, 0.25), (-1, 0x3E800000, 0.25)):
        seed.fill_(sv)
        scale.fill_(r)
        am.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = sr_ref.sr_cast(src, dst, x, r_bits, sv & sr_ref.M64, 123)
        check(dst, out.cpu().numpy(), want, (sv, r))
        check_word(int(am.cpu().numpy().view(np.uint32)[0]), amax_ref.amax_bits(dst, want), (sv, r))
        seen.append(want.tobytes())
    assert len(set(seen)) == 4


def test_cast_scaled_tensor_with_stochastic_rounding():
    import torch

    import ftar
    n = 4099
    x = inputs("bf16", n, seed=8)
    src = torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.bfloat16)
    dst = torch.empty(n, dtype=torch.float8_e4m3fn, device="cuda")
    scale = torch.full((1,), 0.5, device="cuda")
    amax = torch.full((1,), -1.0, device="cuda")
    seed = torch.tensor([-3], dtype=torch.int64, device="cuda")
    assert ftar.cast_scaled_tensor(src, dst, scale=scale, amax=amax, rounding="stochastic", seed=seed, offset=50) is dst
    torch.cuda.synchronize()
    want = sr_ref.sr_cast("bf16", "f8e4m3", x, HALF, -3 & sr_ref.M64, 50)
    check("f8e4m3", dst.view(torch.uint8).cpu().numpy(), want)
    check_word(int(amax.view(torch.int32).cpu().numpy().view(np.uint32)[0]), amax_ref.amax_bits("f8e4m3", want))


# ---- refusals on the device -------------------------------------------------------------------------------
def test_refusals_leave_the_buffers():
    import torch

    import ftar
    n = 4099
    x = inputs("bf16", n, seed=8)
    s_t, s = to_dev(x)
    d_t, d = filled_dev(n * 2)
    am_t, am = filled_dev(4)
    sd = seed_dev(SEED)
    sc = scale_dev(HALF)
    with pytest.raises(ValueError):
        ftar.cast_scaled(s, d, n, "bf16", "f8e4m3", scale=sc[1], amax=am, rounding="bogus", seed=sd[1])
    with pytest.raises(ValueError):
        ftar.cast_scaled(s, d, n, "bf16", "f8e4m3", scale=sc[1], amax=am, rounding="stochastic")
    for sdt, ddt in (("f8e4m3", "bf16"), ("f8e5m2", "f32"), ("bf16", "f16"), ("f64", "f8e4m3")):
        with pytest.raises(ftar.FtarError) as e:
            ftar.cast_scaled(s, d, n // 4, sdt, ddt, scale=sc[1], amax=am, rounding="stochastic", seed=sd[1])
        assert e.value.status == 2
    for kw in (dict(seed=sd[1] + 4), dict(seed=sd[1], amax=am + 2), dict(seed=sd[1], scale=sc[1] + 1)):
        with pytest.raises(ftar.FtarError) as e:
            ftar.cast_scaled(s, d, n, "bf16", "f8e4m3", **{"scale": sc[1], "amax": am, "rounding": "stochastic", **kw})
        assert e.value.status == 1
    torch.cuda.synchronize()
    assert from_dev(d_t, np.uint8, n * 2).tolist() == [0xA5] * (n * 2)
    assert int(from_dev(am_t, np.uint32, 1)[0]) == 0xA5A5A5A5


# ---- the fp8-compressed DDP hook --------------------------------------------------------------------------
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


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("topo,form", [("2,2", "direct"), ("1", "stages")])
def test_fp8_compress_hook_with_stochastic_rounding_over_threads(topo, form, dt, fmt):
    """P = 4 ranks on threads, two buckets in a row: each rank quantizes with its own seed (rank_seed) at the running
    offset, the wire is averaged by the schedule, every rank dequantizes the same wire."""
    import ftar.ddp
    P, base = 4, 99
    f8 = "f8" + fmt
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather(form)
    g.set_reduce_scatter(form)
    states = [ftar.ddp.Fp8CompressState(g[r], fmt=fmt, topo=topo, rounding="stochastic", seed=base) for r in range(P)]
    offset, running = 0, 0
    for b, n in enumerate((N, 4099)):
        ins = [x[:n] for x in amax_ref.base_sources(dt, P, N, seed=9 + b)]
        wire = [sr_ref.sr_cast(dt, f8, ins[r], cast_ref.ONE, sr_ref.rank_seed(base, r), offset) for r in range(P)]
        assert len({w.tobytes() for w in wire}) == P
        red = amax_ref.schedule(f8, wire, topo, "avg")
        want = cast_ref.cast(f8, dt, red, cast_ref.ONE)
        word = amax_ref.amax_bits(f8, red)
        running = word if b == 0 else max(running, word)
        assert word != amax_ref.NAN and 0 < word < INF32
        ts = [_tensor(dt, x) for x in ins]
        _on_threads(P, lambda r: ftar.ddp.fp8_compress_hook(states[r], Bucket(ts[r])).wait())
        offset += n
        for r in range(P):
            check(dt, _bits_of(dt, ts[r]), want, (b, r))
            check_word(_word(states[r].amax), running, (b, r))
            assert states[r].offset == offset and states[r].calls == b + 1
            assert int(states[r].seed.cpu().numpy().view(np.uint64)[0]) == sr_ref.rank_seed(base, r)
            assert float(states[r].found_inf()) == 0.0


@pytest.mark.parametrize("topo,form", [("2,2", "direct"), ("1", "stages")])
def test_the_default_state_stores_the_rne_bits(topo, form):
    import ftar.ddp
    P, dt, f8 = 4, "bf16", "f8e4m3"
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather(form)
    g.set_reduce_scatter(form)
    ins = amax_ref.base_sources(dt, P, N, seed=9)
    wire = [cast_ref.cast(dt, f8, x, cast_ref.ONE) for x in ins]
    red = amax_ref.schedule(f8, wire, topo, "avg")
    want = cast_ref.cast(f8, dt, red, cast_ref.ONE)
    states = [ftar.ddp.Fp8CompressState(g[r], fmt="e4m3", topo=topo) for r in range(P)]
    ts = [_tensor(dt, x) for x in ins]
    _on_threads(P, lambda r: ftar.ddp.fp8_compress_hook(states[r], Bucket(ts[r])).wait())
    for r in range(P):
        check(dt, _bits_of(dt, ts[r]), want, r)
        check_word(_word(states[r].amax), amax_ref.amax_bits(f8, red), r)
        assert states[r].seed is None and states[r].offset == 0 and states[r].rounding == "nearest"
