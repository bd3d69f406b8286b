"""GPU tests of the stochastic MX quantize (include/ftar.h: ftar_mx_quantize_sr) and of the MX gradient hook with
rounding="stochastic" (ftar.ddp.mx_compress_hook).

Every stored byte is compared with tests/mx_sr_ref.py (NaN lanes as "NaN or not", cast_ref.same_bits), which
tests/test_mx_sr_api.py holds against its parts on the CPU; scale bytes are compared exactly.  Calls through the
generator compare with mx_sr_ref.quantize; calls through the bench library's words hook
(ftar_bench_mx_quantize_sr_words: the production kernels on an explicit array of words, words[i] for element i)
compare with mx_sr_ref.quantize_words, which is how a chosen word reaches a chosen element.  The tile of the vector
kernels is read from ftar.last_kernel()."""
import ctypes

import numpy as np
import pytest

import amax_ref
import cast_ref
import f8_ref
import kernel_edges
import mx_ref
import mx_sr_ref
import sr_ref
import test_gpu_mx as rne
from gpu_util import filled_dev, from_dev, to_dev
from test_gpu_mx import Bucket, _bits_of, _on_threads, _tensor, esz, family, group, kernel, sign_bit, spread

pytestmark = pytest.mark.gpu

COMBOS = rne.COMBOS
NS = [1, 31, 32, 33, 63, 64, 1023, 4099, 100_003]
B = mx_ref.BLOCK
TOP = (1 << 32) - 1
SEED = 0x0123456789ABCDEF
VEC, ELEM = "mx_quant_vec_sr_kernel", "mx_quant_elem_sr_kernel"
MODE = {"compute": 0, "given": 1}


def seed_dev(seed):
    return to_dev(np.array([seed & sr_ref.M64], np.uint64))


def check(dt, got, want, what=""):
    assert cast_ref.same_bits(dt, got, want), (what, kernel(), cast_ref.first_diff(dt, got, want))


def tile_elems(symbol, wide):
    """The elements one workgroup of mx_quant_vec_sr_kernel<Rd, Src, Dst, NI, BS, MODE> covers per pass."""
    name, a = kernel_edges.template_args(symbol)
    assert name == VEC, symbol
    return int(a[-3]) * int(a[-2]) * (16 // esz(wide))


def run_sr(wide, f8, bits, headroom=0, seed=SEED, offset=0, src_off=0, dst_off=0, sc_off=0, given=None, families=None):
    """(payload, scale bytes) of the stochastic quantize of a fresh device copy of `bits` at element offset src_off,
    the payload at byte offset dst_off, the scales at byte offset sc_off.  given=None: COMPUTE, and GIVEN on
    ftar_mx_scales' bytes, which must agree in every byte; given=bytes: GIVEN on those."""
    import ftar
    bits = np.ascontiguousarray(bits).view(cast_ref.storage(wide))
    n, nb = bits.size, mx_ref.nblocks(bits.size)
    src_t, src = to_dev(bits, offset_elems=src_off)
    sd_t, sd = seed_dev(seed)

    def payload(mode, sc_ptr, h):
        d_t, d = filled_dev(n + dst_off + 64)
        ftar.mx_quantize(src, d + dst_off, sc_ptr, n, wide, f8, mode=mode, headroom=h, rounding="stochastic", seed=sd,
                         offset=offset)
        if families is not None:
            families.append(family())
        assert from_dev(d_t, np.uint8, 64, n + dst_off).tolist() == [0xA5] * 64
        return from_dev(d_t, np.uint8, n, dst_off)
    if given is not None:
        g_t, g = to_dev(np.asarray(given, np.uint8), offset_elems=sc_off)
        got = payload("given", g, 0)
        assert from_dev(g_t, np.uint8, nb, sc_off).tobytes() == np.asarray(given, np.uint8)[:nb].tobytes()
        return got, np.asarray(given, np.uint8)[:nb]
    s1_t, s1 = filled_dev(nb + sc_off + 64)
    ftar.mx_scales(src, s1 + sc_off, n, wide, f8, headroom=headroom)
    sc1 = from_dev(s1_t, np.uint8, nb, sc_off)
    s2_t, s2 = filled_dev(nb + sc_off + 64)
    pay2 = payload("compute", s2 + sc_off, headroom)
    sc2 = from_dev(s2_t, np.uint8, nb, sc_off)
    pay3 = payload("given", s1 + sc_off, 0)
    assert sc1.tobytes() == sc2.tobytes(), ("COMPUTE's scales are ftar_mx_scales'", np.flatnonzero(sc1 != sc2)[:4])
    assert pay2.tobytes() == pay3.tobytes(), ("COMPUTE's payload is GIVEN's", np.flatnonzero(pay2 != pay3)[:4])
    assert from_dev(src_t, bits.dtype, n, src_off).tobytes() == bits.tobytes(), "the source is read only"
    assert int(from_dev(sd_t, np.uint64, 1)[0]) == seed & sr_ref.M64, "the seed is read only"
    return pay2, sc1


_hook = None


def run_words(wide, f8, bits, w, mode="compute", headroom=0, given=None, dst_off=0):
    """(payload, scale bytes, family) of the production kernels on the explicit words w."""
    global _hook
    import torch

    import ftar
    if _hook is None:
        _hook = ftar.bench_lib().ftar_bench_mx_quantize_sr_words
        vp, ci = ctypes.c_void_p, ctypes.c_int
        _hook.argtypes = [vp, ci, vp, ci, ctypes.c_size_t, ci, ci, vp, vp, vp]
    bits = np.ascontiguousarray(bits).view(cast_ref.storage(wide))
    n, nb = bits.size, mx_ref.nblocks(bits.size)
    w = np.broadcast_to(np.asarray(w, dtype=np.uint32), (n,)).copy()
    src_t, src = to_dev(bits)
    w_t, wp = to_dev(w)
    d_t, d = filled_dev(n + dst_off + 64)
    if mode == "given":
        s_t, s = to_dev(np.asarray(given, np.uint8))
    else:
        s_t, s = filled_dev(nb + 64)
    st = _hook(src, cast_ref.ID[wide], d + dst_off, cast_ref.ID[f8], n, MODE[mode], headroom, s, wp, None)
    assert st == 0, (st, ftar.last_error())
    torch.cuda.synchronize()
    fam = family()
    assert from_dev(d_t, np.uint8, 64, n + dst_off).tolist() == [0xA5] * 64
    return from_dev(d_t, np.uint8, n, dst_off), from_dev(s_t, np.uint8, nb), fam


_tiles = {}


def tile_of(wide, f8):
    if (wide, f8) not in _tiles:
        run_sr(wide, f8, spread(wide, 4099), given=np.full(mx_ref.nblocks(4099), 127, np.uint8))
        _tiles[wide, f8] = tile_elems(kernel(), wide)
    return _tiles[wide, f8]


def products(wide, bits, sc):
    """fp32 bit patterns of mul_rn_f32(widen(x), q(s)) per element (sr_ref.product_bits on each scale byte's elements)."""
    bits = np.asarray(bits).view(cast_ref.storage(wide))
    per = mx_ref._per_element(sc, bits.size)
    out = np.zeros(bits.size, np.uint32)
    for s in np.unique(per):
        out[per == s] = sr_ref.product_bits(wide, bits[per == s], mx_ref.q_bits(s))
    return out


def finite(f8, enc):
    return (enc & 0x7F) < (0x7C if f8 == "f8e5m2" else 0x7F)


# ---- every pair, every size -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_every_pair_and_size_against_the_reference(wide, f8, n):
    """COMPUTE, and GIVEN on ftar_mx_scales' bytes, agree with each other (run_sr) and with the reference; the scale
    bytes are the reference's and the round-to-nearest COMPUTE's."""
    import ftar
    h = n % 3
    x = spread(wide, n, seed=n)
    want_sc = mx_ref.scales(wide, f8, x, h)
    pay, sc = run_sr(wide, f8, x, h, offset=7)
    assert sc.tobytes() == want_sc.tobytes(), (np.flatnonzero(sc != want_sc)[:4], sc[:4], want_sc[:4])
    check(f8, pay, mx_sr_ref.quantize(wide, f8, x, want_sc, SEED, 7), n)
    s_t, s = to_dev(x)
    d_t, d = filled_dev(n)
    c_t, c = filled_dev(mx_ref.nblocks(n))
    ftar.mx_quantize(s, d, c, n, wide, f8, headroom=h)
    assert from_dev(c_t, np.uint8, sc.size).tobytes() == sc.tobytes(), "the round-to-nearest path's scale bytes"


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_tile_edges_in_the_vector_family(wide, f8):
    """A wrong index in the guarded tile or in a later tile shows only at these sizes."""
    T = tile_of(wide, f8)
    assert T % B == 0 and T >= 1024
    for n in (T - B, T, T + B, 2 * T + 33):
        fams = []
        x = spread(wide, n, seed=2)
        pay, sc = run_sr(wide, f8, x, 1, offset=3, families=fams)
        assert set(fams) == {VEC}, fams
        assert tile_elems(kernel(), wide) == T
        want_sc = mx_ref.scales(wide, f8, x, 1)
        assert sc.tobytes() == want_sc.tobytes()
        check(f8, pay, mx_sr_ref.quantize(wide, f8, x, want_sc, SEED, 3), n)


# ---- chosen words ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_the_words_hook_under_the_edge_words_in_both_families(wide, f8):
    """All 0, all 2^32 - 1, per element the threshold 2^32 - F (rounds up) and 2^32 - F - 1 (rounds down), F from
    sr_ref.frac32 of the element's product; and the generator's own words, which must give the generator's bits."""
    T = tile_of(wide, f8)
    for n in (T + 17, 4099):
        x = spread(wide, n, seed=4)
        sc = mx_ref.scales(wide, f8, x, 0)
        F = sr_ref.frac32(f8, products(wide, x, sc)).astype(np.uint64)
        assert (F > 0).sum() > n // 2
        thr = ((np.uint64(1) << np.uint64(32)) - F) & np.uint64(TOP)
        below = (thr - np.uint64(1)) & np.uint64(TOP)
        down = mx_sr_ref.quantize_words(wide, f8, x, sc, 0)
        sets = [("0", 0), ("2^32-1", TOP), ("threshold", thr.astype(np.uint32)), ("threshold-1", below.astype(np.uint32)),
                ("generator", sr_ref.words(SEED, sr_ref.indices(5, n)))]
        for name, w in sets:
            want = mx_sr_ref.quantize_words(wide, f8, x, sc, w)
            for dst_off, fam in ((0, VEC), (1, ELEM)):
                got, got_sc, ran = run_words(wide, f8, x, w, "compute", 0, dst_off=dst_off)
                assert ran == fam, (ran, fam)
                assert got_sc.tobytes() == sc.tobytes(), (name, fam)
                check(f8, got, want, (name, fam, n))
                got, _, ran = run_words(wide, f8, x, w, "given", 0, given=sc, dst_off=dst_off)
                assert ran == fam, (ran, fam)
                check(f8, got, want, (name, fam, n, "given"))
                if name == "2^32-1":
                    assert finite(f8, got).all(), "a finite block stores no NaN and no inf under any word"
                    assert finite(f8, want).all()
                if name == "threshold":
                    assert (((got & 0x7F).astype(int) - (down & 0x7F)) == (F > 0)).all(), "rounds up exactly where F > 0"
                if name == "threshold-1":
                    assert got[F > 0].tobytes() == down[F > 0].tobytes(), "rounds down where F > 0"
        check(f8, run_sr(wide, f8, x, 0, SEED, 5)[0], mx_sr_ref.quantize_words(wide, f8, x, sc, sets[-1][1]), "generator")


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_a_word_reaches_its_own_element(wide, f8):
    """A words array that is 2^32 - 1 at position p of three blocks -- the first, the last full block of the first
    tile, the partial last block (17 elements) -- and 0 elsewhere: exactly those elements move off the truncated
    payload.  Every input has its lowest mantissa bit set, so F > 0 everywhere."""
    T = tile_of(wide, f8)
    n = T + 3 * B + 17
    x = spread(wide, n, seed=3, lo=-8, hi=4) | 1
    sc = mx_ref.scales(wide, f8, x, 0)
    assert (sr_ref.frac32(f8, products(wide, x, sc)) > 0).all()
    blocks = [0, T // B - 1, mx_ref.nblocks(n) - 1]
    for dst_off, fam in ((0, VEC), (1, ELEM)):
        down, _, ran = run_words(wide, f8, x, 0, dst_off=dst_off)
        assert ran == fam
        check(f8, down, mx_sr_ref.quantize_words(wide, f8, x, sc, 0), fam)
        for p in range(B):
            at = [b * B + p for b in blocks if b * B + p < n]
            assert len(at) == (3 if p < 17 else 2)
            w = np.zeros(n, np.uint32)
            w[at] = TOP
            got, _, _ = run_words(wide, f8, x, w, dst_off=dst_off)
            moved = np.flatnonzero(got != down)
            assert moved.tolist() == at, (fam, p, moved[:8], at)
            assert ((got[at] & 0x7F).astype(int) == (down[at] & 0x7F).astype(int) + 1).all()


# ---- the word is a function of the seed and the global index alone ----------------------------------------
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (4, 4), (1, 0), (0, 1), (1, 1), (16, 16)])
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_pointer_offsets_change_the_kernel_not_the_bits(wide, f8, src_off, dst_off):
    """Element offsets of src and dst from a 16-byte boundary, the scales pointer odd: the same bits, from the vector
    kernel exactly when both pointers are 16-byte aligned."""
    n = 2 * tile_of(wide, f8) + 100
    x = spread(wide, n, seed=7)
    want_sc = mx_ref.scales(wide, f8, x, 1)
    fams = []
    pay, sc = run_sr(wide, f8, x, 1, offset=11, src_off=src_off, dst_off=dst_off, sc_off=1, families=fams)
    vec = (src_off * esz(wide)) % 16 == 0 and dst_off % 16 == 0
    assert set(fams) == {VEC if vec else ELEM}, fams
    assert sc.tobytes() == want_sc.tobytes()
    check(f8, pay, mx_sr_ref.quantize(wide, f8, x, want_sc, SEED, 11))


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_splitting_at_a_multiple_of_32_with_the_running_offset_stores_the_one_call_bits(wide, f8):
    import ftar
    n, cut, off = 100_003, 32 * 1001, 1000
    x = spread(wide, n, seed=9)
    want_sc = mx_ref.scales(wide, f8, x, 1)
    pay, sc = run_sr(wide, f8, x, 1, offset=off)
    assert sc.tobytes() == want_sc.tobytes()
    check(f8, pay, mx_sr_ref.quantize(wide, f8, x, want_sc, SEED, off))
    s_t, s = to_dev(x)
    d_t, d = filled_dev(n)
    c_t, c = filled_dev(mx_ref.nblocks(n))
    sd_t, sd = seed_dev(SEED)
    kw = dict(headroom=1, rounding="stochastic", seed=sd)
    ftar.mx_quantize(s, d, c, cut, wide, f8, offset=off, **kw)
    ftar.mx_quantize(s + cut * esz(wide), d + cut, c + cut // 32, n - cut, wide, f8, offset=off + cut, **kw)
    assert from_dev(c_t, np.uint8, sc.size).tobytes() == sc.tobytes()
    assert from_dev(d_t, np.uint8, n).tobytes() == pay.tobytes()


@pytest.mark.parametrize("offset,n", [((1 << 32) - 8, 4099), (1 << 63, 4099), ((1 << 64) - 5, 17)], ids=hex)
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_offsets_across_2_32_at_2_63_and_across_2_64(wide, f8, offset, n):
    x = spread(wide, n, seed=6)
    want_sc = mx_ref.scales(wide, f8, x, 0)
    want = mx_sr_ref.quantize(wide, f8, x, want_sc, SEED, offset)
    for dst_off, fam in ((0, VEC), (1, ELEM)):
        fams = []
        pay, sc = run_sr(wide, f8, x, 0, offset=offset, dst_off=dst_off, families=fams)
        assert set(fams) == {fam} and sc.tobytes() == want_sc.tobytes()
        check(f8, pay, want, fam)


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_seeds_give_different_bits_and_neither_is_round_to_nearest(wide, f8):
    """On these inputs the reference differs from the round-to-nearest payload in at least 15 % of the elements
    (measured: 22 to 25 %) and two seeds differ from each other in at least 20 % (29 to 34 %); the GPU stores the
    reference's bits, so a kernel that rounds to nearest or ignores the seed fails."""
    n = 100_003
    x = spread(wide, n, seed=9)
    sc = mx_ref.scales(wide, f8, x, 1)
    nearest = mx_ref.quantize(wide, f8, x, sc)
    wants = [mx_sr_ref.quantize(wide, f8, x, sc, seed) for seed in (SEED, SEED + 1)]
    for want in wants:
        assert (want != nearest).mean() >= 0.15, (want != nearest).mean()
    assert (wants[0] != wants[1]).mean() >= 0.20, (wants[0] != wants[1]).mean()
    gots = []
    for seed, want in zip((SEED, SEED + 1), wants):
        pay, got_sc = run_sr(wide, f8, x, 1, seed=seed)
        assert got_sc.tobytes() == sc.tobytes()
        check(f8, pay, want, hex(seed))
        gots.append(pay)
    assert (gots[0] != gots[1]).mean() >= 0.20


# ---- NaN blocks and foreign scales ----------------------------------------------------------------------
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_a_non_finite_block_holds_the_stochastic_plain_cast(wide, f8):
    n, off = 4099, 40
    x = spread(wide, n, seed=4)
    pay0, sc0 = run_sr(wide, f8, x, offset=off)
    inf = amax_ref.LAYOUT[wide][2]
    plants = {3: inf, 40: inf | 1, 127: inf | sign_bit(wide)}      # block -> +inf, a NaN, -inf
    y = x.copy()
    for b, enc in plants.items():
        y[b * B + (b % B)] = enc
    pay, sc = run_sr(wide, f8, y, offset=off)
    want_sc = mx_ref.scales(wide, f8, y, 0)
    assert sc.tobytes() == want_sc.tobytes() and sorted(np.flatnonzero(sc == 255)) == sorted(plants)
    check(f8, pay, mx_sr_ref.quantize(wide, f8, y, want_sc, SEED, off))
    per = np.repeat(np.arange(mx_ref.nblocks(n)), B)[:n]
    marked = np.isin(per, list(plants))
    assert pay[~marked].tobytes() == pay0[~marked].tobytes(), "the neighbouring blocks keep their bytes"
    others = ~np.isin(np.arange(sc.size), list(plants))
    assert sc[others].tobytes() == sc0[others].tobytes()
    for b in plants:
        blk = slice(b * B, b * B + B)
        check(f8, pay[blk], sr_ref.sr_cast(wide, f8, y[blk], cast_ref.ONE, SEED, off + b * B), ("r = 1.0 at the block's offset", b))


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_given_with_every_scale_byte_overflows_as_the_reference_says(wide, f8):
    from test_gpu_cast import inputs
    n = 256 * B * 2 - 9
    x = inputs(wide, n, seed=6)
    x[40::97] = spread(wide, n, seed=6)[40::97]       # and small magnitudes, which the large q of a small byte keeps
    sc = np.resize(np.arange(256, dtype=np.uint8), mx_ref.nblocks(n))
    want = mx_sr_ref.quantize(wide, f8, x, sc, SEED, 9)
    nan = cast_ref.nan_mask(f8, want)
    assert nan.any() and (~nan).any() and (f8 == "f8e4m3" or ((want & 0x7F) == 0x7C).any())
    got, _ = run_sr(wide, f8, x, offset=9, given=sc)
    assert family() == VEC
    check(f8, got, want)
    got, _ = run_sr(wide, f8, x, offset=9, given=sc, dst_off=1, sc_off=3)
    assert family() == ELEM
    check(f8, got, want, "element-wise")


# ---- write footprint ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc_off", [0, 1, 8])
@pytest.mark.parametrize("wide,f8", [("f32", "f8e4m3"), ("bf16", "f8e5m2"), ("f16", "f8e4m3")])
def test_write_footprint_is_the_n_bytes_and_the_nblocks_bytes(wide, f8, sc_off):
    """Guarded arenas: exactly n payload bytes and nblocks scale bytes (COMPUTE) or no scale byte (GIVEN) change; the
    source and the seed are unchanged."""
    import torch

    import ftar
    T = tile_of(wide, f8)
    for n in (1, 33, T, 2 * T + 33):
        nb = mx_ref.nblocks(n)
        x = spread(wide, n, seed=8)
        want_sc = mx_ref.scales(wide, f8, x, 0)
        want = mx_sr_ref.quantize(wide, f8, x, want_sc, SEED, 77)
        sa = kernel_edges.Arena(n * esz(wide) + 16)
        sa.upload(0, x)
        da = kernel_edges.Arena(n + 16)
        ca = kernel_edges.Arena(nb + sc_off + 32)
        sd = kernel_edges.Arena(64)
        sd.upload(8, np.array([SEED], np.uint64))
        for mode in ("compute", "given"):
            if mode == "given":
                ca.upload(sc_off, want_sc)
            ftar.mx_quantize(sa.ptr(), da.ptr(), ca.ptr(sc_off), n, wide, f8, mode=mode, rounding="stochastic",
                             seed=sd.ptr(8), offset=77)
            torch.cuda.synchronize()
            check(f8, da.window(0, n).cpu().numpy(), want, (mode, n))
            assert ca.window(sc_off, sc_off + nb).cpu().numpy().tobytes() == want_sc.tobytes(), (mode, n)
            if mode == "compute":
                assert kernel_edges.check_untouched(ca, sc_off, sc_off + nb) is None, (mode, n)
                ca.restore(sc_off, sc_off + nb)
            else:
                assert kernel_edges.check_untouched(ca) is None, "GIVEN writes no scale byte"
            assert kernel_edges.check_untouched(da, 0, n) is None, (mode, n)
            assert kernel_edges.check_untouched(sa) is None and kernel_edges.check_untouched(sd) is None
            da.restore(0, n)


# ---- graph capture --------------------------------------------------------------------------------------
def test_scales_the_stochastic_quantize_and_the_dequantize_capture_and_follow_the_device():
    """Kernels only: the three calls capture as they are; a replay reads what the source, the scales and the seed word
    hold on the device then."""
    import torch

    import ftar
    wide, f8, n, off = "f16", "f8e4m3", 100_003, 123
    xs = [spread(wide, n, seed=11), spread(wide, n, seed=12, lo=-8, hi=12)]
    src = _tensor(wide, xs[0])
    wire = torch.empty(n, dtype=torch.uint8, device="cuda")
    sc = torch.empty(mx_ref.nblocks(n), dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.float16, device="cuda")
    seed = torch.tensor([5], dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ftar.mx_scales(src, sc, n, wide, f8, headroom=1, stream=side)
            ftar.mx_quantize(src, wire, sc, n, wide, f8, mode="given", stream=side, rounding="stochastic", seed=seed,
                             offset=off)
            ftar.mx_dequantize(wire, sc, out, n, f8, wide, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for x, bump in ((xs[0], 0), (xs[1], 0), (xs[1], 1)):
        src.copy_(_tensor(wide, x))
        seed.add_(bump)
        g.replay()
        torch.cuda.synchronize()
        sv = int(seed.cpu()[0])
        want_sc = mx_ref.scales(wide, f8, x, 1)
        want = mx_sr_ref.quantize(wide, f8, x, want_sc, sv, off)
        assert sc.cpu().numpy().tobytes() == want_sc.tobytes()
        check(f8, wire.cpu().numpy(), want, (sv, bump))
        check(wide, _bits_of(wide, out), mx_ref.dequantize(f8, wide, want, want_sc))
        seen.append(want.tobytes())
    assert int(seed.cpu()[0]) == 6 and len(set(seen)) == 3


def test_the_tensor_form_with_stochastic_rounding():
    import torch

    import ftar
    n = 4099
    x = spread("bf16", n, seed=10)
    src = _tensor("bf16", x)
    wire = torch.empty(n, dtype=torch.float8_e5m2, device="cuda")
    sc = torch.empty(ftar.mx_nblocks(n), dtype=torch.uint8, device="cuda")
    seed = torch.tensor([-3], dtype=torch.int64, device="cuda")
    assert ftar.mx_quantize_tensor(src, wire, sc, headroom=2, rounding="stochastic", seed=seed, offset=50) is wire
    torch.cuda.synchronize()
    want_sc = mx_ref.scales("bf16", "f8e5m2", x, 2)
    assert sc.cpu().numpy().tobytes() == want_sc.tobytes()
    check("f8e5m2", wire.view(torch.uint8).cpu().numpy(), mx_sr_ref.quantize("bf16", "f8e5m2", x, want_sc, -3 & sr_ref.M64, 50))
    with pytest.raises(ValueError):
        ftar.mx_quantize_tensor(src, wire, sc, rounding="stochastic", seed=seed.cpu())


# ---- round to nearest is unaffected ---------------------------------------------------------------------
def test_rne_calls_still_reach_the_rne_kernels():
    import ftar
    n = 4099
    x = spread("bf16", n, seed=1)
    t, p = to_dev(x)
    d_t, d = filled_dev(n + 1)
    c_t, c = filled_dev(mx_ref.nblocks(n))
    sc = mx_ref.scales("bf16", "f8e4m3", x, 0)
    for kw in ({}, dict(rounding="nearest", seed=None, offset=7)):
        for mode in ("compute", "given"):
            ftar.mx_quantize(p, d, c, n, "bf16", "f8e4m3", mode=mode, **kw)
            assert kernel().startswith("mx_quant_vec_kernel<") and "Sr" not in kernel(), kernel()
            check("f8e4m3", from_dev(d_t, np.uint8, n), mx_ref.quantize("bf16", "f8e4m3", x, sc))
    ftar.mx_quantize(p, d + 1, c, n, "bf16", "f8e4m3")
    assert kernel().startswith("mx_quant_elem_kernel<") and "Sr" not in kernel(), kernel()
    sd_t, sd = seed_dev(SEED)
    ftar.mx_quantize(p, d, c, n, "bf16", "f8e4m3", rounding="stochastic", seed=sd)
    assert kernel().startswith(VEC + "<SrGen, "), kernel()


# ---- the MX gradient hook -------------------------------------------------------------------------------
N = rne.N


def _expect_sr(dt, f8, ins, topo, headroom, base, offset):
    """test_gpu_mx._expect with each rank's quantize stochastic at rank_seed(base, r) and `offset`."""
    sc = np.maximum.reduce([mx_ref.scales(dt, f8, x, headroom) for x in ins])
    wire = [mx_sr_ref.quantize(dt, f8, x, sc, sr_ref.rank_seed(base, r), offset) for r, x in enumerate(ins)]
    red = amax_ref.schedule(f8, wire, topo, "avg")
    return mx_ref.dequantize(f8, dt, red, sc), sc, red


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("topo,form,headroom", [("4", "direct", 0), ("1", "stages", 2)])
def test_mx_compress_hook_with_stochastic_rounding_over_threads(topo, form, headroom, dt, fmt):
    """P = 4 ranks on threads, two buckets in a row: each rank quantizes with its own seed (rank_seed) at the running
    offset against the agreed scale bytes, the wire is averaged by the schedule, every rank dequantizes the same
    wire.  Then the first bucket through a default state, which must store test_gpu_mx's round-to-nearest bits and
    another wire; then a NaN planted on one rank."""
    import ftar.ddp
    P, base = 4, 99
    f8 = "f8" + fmt
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather(form)
    g.set_reduce_scatter(form)
    assert N % B
    states = [ftar.ddp.MxCompressState(g[r], fmt=fmt, topo=topo, headroom=headroom, rounding="stochastic", seed=base)
              for r in range(P)]
    first = None
    for b in range(2):
        ins = [spread(dt, N, seed=20 + 10 * b + r, block_seed=19 + b) for r in range(P)]
        want, sc, red = _expect_sr(dt, f8, ins, topo, headroom, base, b * N)
        assert not f8_ref.nan_mask(f8, red).any() and not cast_ref.nan_mask(dt, want).any(), "finite in, no NaN expected"
        assert ((red & 0x7F) <= f8_ref.MAX_FINITE[f8]).all() and not (sc == 255).any()
        ts = [_tensor(dt, x) for x in ins]
        _on_threads(P, lambda r: ftar.ddp.mx_compress_hook(states[r], Bucket(ts[r])).wait())
        for r in range(P):
            assert f8_ref.same_bits(f8, from_dev(states[r]._wire, np.uint8, N), red), (b, r, "the reduced wire")
            assert from_dev(states[r]._scales, np.uint8, sc.size).tobytes() == sc.tobytes(), (b, r)
            check(dt, _bits_of(dt, ts[r]), want, (b, r))
            assert states[r].offset == (b + 1) * N and states[r].calls == b + 1
            assert int(states[r].seed.cpu().numpy().view(np.uint64)[0]) == sr_ref.rank_seed(base, r)
            assert float(states[r].found_inf()) == 0.0
        if b == 0:
            first = (ins, red)
    assert all(s.offset == 2 * N for s in states)
    # a default state on the first bucket: the round-to-nearest bits, and another wire than the stochastic state's
    ins, red_sr = first
    want, sc, red = rne._expect(dt, f8, ins, topo, headroom)
    assert not f8_ref.same_bits(f8, red, red_sr)
    plain = [ftar.ddp.MxCompressState(g[r], fmt=fmt, topo=topo, headroom=headroom) for r in range(P)]
    ts = [_tensor(dt, x) for x in ins]
    _on_threads(P, lambda r: ftar.ddp.mx_compress_hook(plain[r], Bucket(ts[r])).wait())
    for r in range(P):
        assert f8_ref.same_bits(f8, from_dev(plain[r]._wire, np.uint8, N), red), (r, "the round-to-nearest wire")
        check(dt, _bits_of(dt, ts[r]), want, r)
        assert (plain[r].rounding, plain[r].seed, plain[r].offset) == ("nearest", None, 0)
    # a NaN on one rank: that block NaN on every rank, found_inf() 1.0 on every rank
    p = 4321
    bad = [x.copy() for x in ins]
    bad[1][p] = amax_ref.encode(dt, float("nan"))
    want2, sc2, _ = _expect_sr(dt, f8, bad, topo, headroom, base, 2 * N)
    assert sc2[p // B] == 255 and (sc2 == 255).sum() == 1
    ts2 = [_tensor(dt, x) for x in bad]
    _on_threads(P, lambda r: ftar.ddp.mx_compress_hook(states[r], Bucket(ts2[r])).wait())
    for r in range(P):
        check(dt, _bits_of(dt, ts2[r]), want2, r)
        assert float(states[r].found_inf()) == 1.0 and states[r].offset == 3 * N
        states[r].reset()
        assert float(states[r].found_inf()) == 0.0
