"""GPU tests of the MX block-scaled casts (include/ftar.h: ftar_mx_scales, ftar_mx_quantize, ftar_mx_dequantize) and
of the MX gradient hook built on them (ftar.ddp.mx_compress_hook).

Scale bytes are compared exactly, payloads and dequantized values bit for bit (NaN lanes as "NaN or not",
cast_ref.same_bits) with tests/mx_ref.py, whose rule tests/test_mx_api.py holds against torch on the CPU.  Every
quantize case runs three ways -- ftar_mx_scales, the one-pass COMPUTE mode, and GIVEN on the bytes of the first --
and all must agree.  The tile of the vector kernels is read from ftar.last_kernel()."""
import threading

import numpy as np
import pytest

import amax_ref
import cast_ref
import f8_ref
import kernel_edges
import mx_ref
from gpu_util import filled_dev, from_dev, to_dev

pytestmark = pytest.mark.gpu

WIDE, F8 = cast_ref.WIDE, cast_ref.F8
COMBOS = [(w, f) for w in WIDE for f in F8]
NS = [1, 31, 32, 33, 63, 64, 1023, 4099, 100_003]
MANTISSAS = (0, 0x5FFFFF, 0x600000, 0x600001, 0x7FFFFF)


def esz(dt):
    return np.dtype(cast_ref.storage(dt)).itemsize


def sign_bit(dt):
    return 1 << (8 * esz(dt) - 1)


def spread(dt, n, seed=1, block_seed=None, lo=-30, hi=10, down=0):
    """n finite elements of a wide dtype whose magnitudes step block by block over 2^lo .. 2^hi (fp16: from 2^-22),
    each element up to 5 binades under its block's top; random signs and mantissas; what falls under the format's
    normal range is the subnormal (or zero) of that magnitude.  block_seed fixes the blocks' exponents apart from
    the elements' (the ranks of a hook case share them); down: every element that many binades lower."""
    rng = np.random.default_rng(seed)
    brng = np.random.default_rng(seed if block_seed is None else block_seed)
    mb, bias = cast_ref.FMT[dt]
    if dt == "f16":
        lo = max(lo, -22)
    be = brng.integers(lo, hi + 1, mx_ref.nblocks(n))
    field = np.repeat(be, mx_ref.BLOCK)[:n] - rng.integers(0, 6, n) - down + bias
    assert field.max() <= 2 * bias
    mant = rng.integers(0, 1 << mb, n)
    sub = ((1 << mb) | mant) >> np.clip(1 - field, 0, 40)
    bits = (rng.integers(0, 2, n) * sign_bit(dt)) | np.where(field > 0, (np.maximum(field, 0) << mb) | mant, sub)
    return bits.astype(cast_ref.storage(dt))


def enc_pow2(dt, k):
    """The encoding of 2^k (normal in dt)."""
    mb, bias = cast_ref.FMT[dt]
    assert 0 < k + bias < 2 * bias + 1
    return (k + bias) << mb


def kernel():
    import ftar
    return ftar.names.kernel_symbol(ftar.last_kernel())


def family():
    return kernel_edges.template_args(kernel())[0]


def tile_elems(symbol, wide):
    """The elements one workgroup of mx_quant_vec_kernel<Src, Dst, NI, BS, MODE> / mx_dequant_vec_kernel<Src, Dst,
    NI, BS> covers per pass: NI x BS wide vectors of 16 bytes."""
    name, a = kernel_edges.template_args(symbol)
    assert name in ("mx_quant_vec_kernel", "mx_dequant_vec_kernel"), symbol
    ni, bs = (int(a[-3]), int(a[-2])) if name == "mx_quant_vec_kernel" else (int(a[-2]), int(a[-1]))
    return ni * bs * (16 // esz(wide))


def run_quant(wide, f8, bits, headroom=0, src_off=0, dst_off=0, sc_off=0, given=None, families=None):
    """(payload, scale bytes) of a fresh device copy of `bits` at element offset src_off, the payload at byte offset
    dst_off and the scales at byte offset sc_off.  given=None: ftar_mx_scales, COMPUTE, and GIVEN on the first's
    bytes, which must all agree; given=bytes: GIVEN on those."""
    import ftar
    bits = np.ascontiguousarray(bits).view(cast_ref.storage(wide))
    n, nb = bits.size, mx_ref.nblocks(bits.size)
    src_t, src = to_dev(bits, offset_elems=src_off)

    def payload(mode, sc_ptr, h):
        d_t, d = filled_dev(n + dst_off + 64)
        ftar.mx_quantize(src, d + dst_off, sc_ptr, n, wide, f8, mode=mode, headroom=h)
        if families is not None:
            families.append(family())
        return from_dev(d_t, np.uint8, n, dst_off)
    if given is not None:
        g_t, g = to_dev(np.asarray(given, np.uint8), offset_elems=sc_off)
        got = payload("given", g, 0)
        assert from_dev(g_t, np.uint8, nb, sc_off).tobytes() == np.asarray(given, np.uint8)[:nb].tobytes()
        return got, np.asarray(given, np.uint8)[:nb]
    s1_t, s1 = filled_dev(nb + sc_off + 64)
    ftar.mx_scales(src, s1 + sc_off, n, wide, f8, headroom=headroom)
    if families is not None:
        families.append(family())
    sc1 = from_dev(s1_t, np.uint8, nb, sc_off)
    s2_t, s2 = filled_dev(nb + sc_off + 64)
    pay2 = payload("compute", s2 + sc_off, headroom)
    sc2 = from_dev(s2_t, np.uint8, nb, sc_off)
    pay3 = payload("given", s1 + sc_off, 0)
    assert sc1.tobytes() == sc2.tobytes(), ("COMPUTE's scales are ftar_mx_scales'", np.flatnonzero(sc1 != sc2)[:4])
    assert pay2.tobytes() == pay3.tobytes(), ("COMPUTE's payload is GIVEN's", np.flatnonzero(pay2 != pay3)[:4])
    assert from_dev(src_t, bits.dtype, n, src_off).tobytes() == bits.tobytes(), "the source is read only"
    return pay2, sc1


def run_dequant(f8, wide, pay, sc, src_off=0, dst_off=0, sc_off=0):
    import ftar
    pay = np.ascontiguousarray(pay).view(np.uint8)
    n = pay.size
    p_t, p = to_dev(pay, offset_elems=src_off)
    s_t, s = to_dev(np.asarray(sc, np.uint8), offset_elems=sc_off)
    d_t, d = filled_dev((n + dst_off) * esz(wide) + 64)
    ftar.mx_dequantize(p, s, d + dst_off * esz(wide), n, f8, wide)
    return from_dev(d_t, cast_ref.storage(wide), n, dst_off)


def check(dt, got, want, what=""):
    assert cast_ref.same_bits(dt, got, want), (what, cast_ref.first_diff(dt, got, want))


def check_all(wide, f8, bits, headroom=0, what="", **kw):
    """Scales, payload and the dequantize of one input against the reference; returns (payload, scales)."""
    want_sc = mx_ref.scales(wide, f8, bits, headroom)
    pay, sc = run_quant(wide, f8, bits, headroom, **kw)
    assert sc.tobytes() == want_sc.tobytes(), (what, kernel(), np.flatnonzero(sc != want_sc)[:4], sc[:4], want_sc[:4])
    check(f8, pay, mx_ref.quantize(wide, f8, bits, want_sc), (what, "payload"))
    back = run_dequant(f8, wide, pay, sc)
    check(wide, back, mx_ref.dequantize(f8, wide, pay, sc), (what, "dequantize", kernel()))
    return pay, sc


def tile_of(wide, f8):
    run_quant(wide, f8, spread(wide, 4099), given=np.full(mx_ref.nblocks(4099), 127, np.uint8))
    return tile_elems(kernel(), wide)


# ---- every pair, every size -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_every_pair_and_size_against_the_reference(wide, f8, n):
    check_all(wide, f8, spread(wide, n, seed=n), headroom=n % 3, what=n)


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_one_tile_exactly_and_a_block_either_side(wide, f8):
    T = tile_of(wide, f8)
    assert T % mx_ref.BLOCK == 0 and T >= 1024
    for n in (T - mx_ref.BLOCK, T, T + mx_ref.BLOCK):
        fams = []
        check_all(wide, f8, spread(wide, n, seed=2), what=n, families=fams)
        assert set(fams) == {"mx_quant_vec_kernel"}, fams
        assert family() == "mx_dequant_vec_kernel" and tile_elems(kernel(), wide) == T


# ---- the peak at every position of a block --------------------------------------------------------------
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_the_peak_is_found_at_every_position_of_a_block(wide, f8):
    """A cross-lane max that drops a lane shows here: the block's only large element at each of its 32 positions,
    in the first and the last block of a full tile, a block inside it, and the partial last block (17 elements)."""
    T = tile_of(wide, f8)
    n = T + 5 * mx_ref.BLOCK + 17
    blocks = [0, 7, T // mx_ref.BLOCK - 1, mx_ref.nblocks(n) - 1]
    base = spread(wide, n, seed=3, lo=-12, hi=-10)
    for p in range(mx_ref.BLOCK):
        x = base.copy()
        planted = []
        for b in blocks:
            at = b * mx_ref.BLOCK + p
            if at < n:
                x[at] = enc_pow2(wide, 5) | (sign_bit(wide) if p & 1 else 0) | 1      # just above 32
                planted.append(b)
        _, sc = check_all(wide, f8, x, what=p)
        assert len(planted) >= 3 and all(sc[b] == 127 + 5 - mx_ref.EMAX[f8] for b in planted), (p, sc[blocks])
        assert all(sc[b] < 127 - 9 - mx_ref.EMAX[f8] + 1 for b in range(sc.size) if b not in planted)


# ---- the 1.75 boundary at every exponent ----------------------------------------------------------------
def _peak_blocks(wide):
    """One block per listed peak: the peak at position b % 32, the rest at half its encoding (a smaller magnitude),
    signs alternating."""
    if wide == "f32":
        peaks = np.array([(e << 23) | m for e in range(256) for m in MANTISSAS], np.uint32)
    else:
        peaks = np.arange(0x8000, dtype=np.uint16)        # every non-negative encoding: inf and the NaNs included
    x = np.repeat(peaks >> 1, mx_ref.BLOCK).reshape(-1, mx_ref.BLOCK)
    x[np.arange(peaks.size), np.arange(peaks.size) % mx_ref.BLOCK] = peaks
    x[:, 1::2] |= sign_bit(wide)
    return peaks, x.reshape(-1)


@pytest.mark.parametrize("headroom", [0, 3])
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_the_boundary_at_every_exponent(wide, f8, headroom):
    """The clamps at 0, the subnormal peaks, the mantissas on either side of 1.75 and the non-finite peaks, each in
    a block of its own."""
    peaks, x = _peak_blocks(wide)
    _, sc = check_all(wide, f8, x, headroom=headroom)
    a = cast_ref.widen_bits(wide, peaks) & np.uint32(0x7FFFFFFF)
    assert sc.tobytes() == mx_ref.scale_of(a, f8, headroom).tobytes()
    assert (sc == headroom).any() and (sc == 255).any() and len(np.unique(sc)) > 20
    assert wide == "f16" or (sc == headroom).sum() > 4          # fp16's smallest subnormal widens to 2^-24: no clamp


# ---- NaN and zero blocks --------------------------------------------------------------------------------
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_a_non_finite_element_marks_its_block_alone(wide, f8):
    n = 4099
    x = spread(wide, n, seed=4)
    pay0, sc0 = check_all(wide, f8, x)
    inf = amax_ref.LAYOUT[wide][2]
    plants = {3: inf, 40: inf | 1, 127: inf | sign_bit(wide)}      # block -> +inf, a NaN, -inf
    y = x.copy()
    for b, enc in plants.items():
        y[b * mx_ref.BLOCK + (b % mx_ref.BLOCK)] = enc
    pay, sc = check_all(wide, f8, y, what="planted")
    per = np.repeat(np.arange(mx_ref.nblocks(n)), mx_ref.BLOCK)[:n]
    marked = np.isin(per, list(plants))
    assert sorted(np.flatnonzero(sc == 255)) == sorted(plants) and not (sc0 == 255).any()
    assert sc[~np.isin(np.arange(sc.size), list(plants))].tobytes() == sc0[~np.isin(np.arange(sc.size), list(plants))].tobytes()
    assert pay[~marked].tobytes() == pay0[~marked].tobytes(), "the neighbouring blocks keep their bytes"
    check(f8, pay[marked], cast_ref.cast(wide, f8, y[marked]), "a NaN block's payload is the plain cast")
    back = run_dequant(f8, wide, pay, sc)
    assert np.array_equal(cast_ref.nan_mask(wide, back), marked), "NaN across exactly those blocks"


@pytest.mark.parametrize("headroom", [0, 5])
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_zero_blocks_give_the_headroom_and_keep_their_signs(wide, f8, headroom):
    n = 4099
    x = spread(wide, n, seed=5)
    per = np.repeat(np.arange(mx_ref.nblocks(n)), mx_ref.BLOCK)[:n]
    x[per == 2] = 0
    x[per == 9] = sign_bit(wide)
    x[per == 128] = 0                                  # the partial last block: +0 and -0 mixed
    x[-1] = sign_bit(wide)
    pay, sc = check_all(wide, f8, x, headroom=headroom)
    assert sc[2] == sc[9] == sc[128] == headroom
    assert not pay[per == 2].any() and (pay[per == 9] == 0x80).all() and pay[-1] == 0x80 and not pay[per == 128][:-1].any()
    back = run_dequant(f8, wide, pay, sc)
    assert back[per == 2].tobytes() == x[per == 2].tobytes() and back[per == 9].tobytes() == x[per == 9].tobytes()
    assert back[per == 128].tobytes() == x[per == 128].tobytes()


# ---- GIVEN with any byte --------------------------------------------------------------------------------
@pytest.mark.parametrize("f8,wide", [(f, w) for f in F8 for w in WIDE])
def test_every_scale_byte_dequantizes_every_fp8_encoding(f8, wide):
    """256 scale bytes x 256 encodings: 8 blocks per byte."""
    pay = np.tile(np.arange(256, dtype=np.uint8), 256)
    sc = np.repeat(np.arange(256, dtype=np.uint8), 8)
    got = run_dequant(f8, wide, pay, sc)
    assert family() == "mx_dequant_vec_kernel"
    check(wide, got, mx_ref.dequantize(f8, wide, pay, sc))
    for off in (1, 3):      # and through the element-wise kernel
        got = run_dequant(f8, wide, pay, sc, src_off=off, sc_off=1)
        assert family() == "mx_dequant_elem_kernel"
        check(wide, got, mx_ref.dequantize(f8, wide, pay, sc), off)


@pytest.mark.parametrize("wide,f8", COMBOS)
def test_every_scale_byte_quantizes_with_the_overflow_to_nan_or_inf(wide, f8):
    from test_gpu_cast import inputs
    n = 256 * mx_ref.BLOCK * 2 - 9
    x = inputs(wide, n, seed=6)
    x[40::97] = spread(wide, n, seed=6)[40::97]       # and small magnitudes, which the large q of a small byte keeps
    sc = np.resize(np.arange(256, dtype=np.uint8), mx_ref.nblocks(n))
    want = mx_ref.quantize(wide, f8, x, sc)
    nan = cast_ref.nan_mask(f8, want)
    assert nan.any() and (~nan).any() and (f8 == "f8e4m3" or ((want & 0x7F) == 0x7C).any())
    got, _ = run_quant(wide, f8, x, given=sc)
    assert family() == "mx_quant_vec_kernel"
    check(f8, got, want)
    got, _ = run_quant(wide, f8, x, given=sc, dst_off=1, sc_off=3)
    assert family() == "mx_quant_elem_kernel"
    check(f8, got, want, "element-wise")


# ---- alignment and the kernel reached -------------------------------------------------------------------
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (4, 4), (1, 0), (0, 1), (1, 1), (16, 16)])
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_alignment_cases_and_the_kernel_reached(wide, f8, src_off, dst_off):
    """Element offsets of src and dst from a 16-byte boundary, the scales pointer odd: the same bits, from the
    vector kernels exactly when both pointers are 16-byte aligned."""
    n = 2 * tile_of(wide, f8) + 100
    x = spread(wide, n, seed=7)
    want_sc = mx_ref.scales(wide, f8, x, 1)
    want = mx_ref.quantize(wide, f8, x, want_sc)
    fams = []
    pay, sc = run_quant(wide, f8, x, 1, src_off=src_off, dst_off=dst_off, sc_off=1, families=fams)
    vec = (src_off * esz(wide)) % 16 == 0 and dst_off % 16 == 0
    # ftar_mx_scales has no dst: it runs the vector kernel whenever src is aligned
    assert fams[0] == ("mx_quant_vec_kernel" if (src_off * esz(wide)) % 16 == 0 else "mx_quant_elem_kernel")
    assert set(fams[1:]) == {"mx_quant_vec_kernel" if vec else "mx_quant_elem_kernel"}, fams
    assert sc.tobytes() == want_sc.tobytes()
    check(f8, pay, want)
    # the way back: src is the payload (dst_off), dst the wide side (src_off)
    back = run_dequant(f8, wide, pay, sc, src_off=dst_off, dst_off=src_off, sc_off=1)
    assert family() == ("mx_dequant_vec_kernel" if vec else "mx_dequant_elem_kernel")
    check(wide, back, mx_ref.dequantize(f8, wide, pay, sc))


# ---- write footprint ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc_off", [0, 1, 2, 4, 8, 16])
@pytest.mark.parametrize("wide,f8", [("f32", "f8e4m3"), ("bf16", "f8e5m2"), ("f16", "f8e4m3")])
def test_write_footprint_is_the_n_elements_and_the_nblocks_bytes(wide, f8, sc_off):
    """Guarded arenas around the payload, the scales and the dequantized copy: exactly n elements and nblocks bytes
    change and the source is unchanged, at every alignment of the scales pointer (each picks another store width)
    and at sizes under, on and over the tile."""
    import torch

    import ftar
    T = tile_of(wide, f8)
    for n in (1, 33, 4099, T, 2 * T + 33):
        nb = mx_ref.nblocks(n)
        x = spread(wide, n, seed=8)
        want_sc = mx_ref.scales(wide, f8, x, 0)
        want = mx_ref.quantize(wide, f8, x, want_sc)
        sa = kernel_edges.Arena(n * esz(wide) + 16)
        sa.upload(0, x)
        da = kernel_edges.Arena(n + 16)
        ca = kernel_edges.Arena(nb + sc_off + 32)
        wa = kernel_edges.Arena(n * esz(wide) + 16)
        for mode in ("scales", "compute", "given"):
            if mode == "scales":
                ftar.mx_scales(sa.ptr(), ca.ptr(sc_off), n, wide, f8)
            else:
                if mode == "given":
                    ca.upload(sc_off, want_sc)
                ftar.mx_quantize(sa.ptr(), da.ptr(), ca.ptr(sc_off), n, wide, f8, mode=mode)
            torch.cuda.synchronize()
            assert ca.window(sc_off, sc_off + nb).cpu().numpy().tobytes() == want_sc.tobytes(), (mode, n)
            assert kernel_edges.check_untouched(ca, sc_off, sc_off + nb) is None, (mode, n)
            assert kernel_edges.check_untouched(da, 0, 0 if mode == "scales" else n) is None, (mode, n)
            assert kernel_edges.check_untouched(sa) is None
            if mode != "scales":
                check(f8, da.window(0, n).cpu().numpy(), want, (mode, n))
                da.restore(0, n)
            if mode != "given":
                ca.restore(sc_off, sc_off + nb)
        da.upload(0, want)
        ftar.mx_dequantize(da.ptr(), ca.ptr(sc_off), wa.ptr(), n, f8, wide)
        torch.cuda.synchronize()
        got = wa.window(0, n * esz(wide)).cpu().numpy().view(cast_ref.storage(wide))
        check(wide, got, mx_ref.dequantize(f8, wide, want, want_sc), n)
        assert kernel_edges.check_untouched(wa, 0, n * esz(wide)) is None
        assert kernel_edges.check_untouched(da) is None and kernel_edges.check_untouched(ca) is None


# ---- split ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide,f8", COMBOS)
def test_splitting_at_a_multiple_of_32_stores_the_one_call_bits(wide, f8):
    import ftar
    n, cut = 100_003, 32 * 1001
    x = spread(wide, n, seed=9)
    pay, sc = check_all(wide, f8, x, headroom=1)
    s_t, s = to_dev(x)
    d_t, d = filled_dev(n)
    c_t, c = filled_dev(mx_ref.nblocks(n))
    w_t, w = filled_dev(n * esz(wide))
    ftar.mx_quantize(s, d, c, cut, wide, f8, headroom=1)
    ftar.mx_quantize(s + cut * esz(wide), d + cut, c + cut // 32, n - cut, wide, f8, headroom=1)
    assert from_dev(c_t, np.uint8, sc.size).tobytes() == sc.tobytes()
    assert from_dev(d_t, np.uint8, n).tobytes() == pay.tobytes()
    ftar.mx_dequantize(d, c, w, cut, f8, wide)
    ftar.mx_dequantize(d + cut, c + cut // 32, w + cut * esz(wide), n - cut, f8, wide)
    check(wide, from_dev(w_t, cast_ref.storage(wide), n), mx_ref.dequantize(f8, wide, pay, sc))


# ---- the tensor forms and graph capture -----------------------------------------------------------------
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


def test_the_tensor_forms():
    import torch

    import ftar
    n = 4099
    x = spread("bf16", n, seed=10)
    src = _tensor("bf16", x)
    wire = torch.empty(n, dtype=torch.float8_e5m2, device="cuda")
    sc = torch.empty(ftar.mx_nblocks(n), dtype=torch.uint8, device="cuda")
    assert ftar.mx_quantize_tensor(src, wire, sc, headroom=2) is wire
    back = torch.empty(n, dtype=torch.float32, device="cuda")
    assert ftar.mx_dequantize_tensor(wire, sc, back) is back
    torch.cuda.synchronize()
    want_sc = mx_ref.scales("bf16", "f8e5m2", x, 2)
    want = mx_ref.quantize("bf16", "f8e5m2", x, want_sc)
    assert sc.cpu().numpy().tobytes() == want_sc.tobytes()
    check("f8e5m2", wire.view(torch.uint8).cpu().numpy(), want)
    check("f32", back.cpu().numpy().view(np.uint32), mx_ref.dequantize("f8e5m2", "f32", want, want_sc))
    with pytest.raises(ValueError):
        ftar.mx_quantize_tensor(src, wire, sc[:-1])
    with pytest.raises(ValueError):
        ftar.mx_quantize_tensor(src, wire, sc.cpu())


def test_scales_quantize_and_dequantize_capture_into_one_graph_and_follow_the_data():
    """Kernels only: the three calls capture as they are, and a replay reads what the source and the scales hold on
    the device then."""
    import torch

    import ftar
    wide, f8, n = "f16", "f8e4m3", 100_003
    xs = [spread(wide, n, seed=11), spread(wide, n, seed=12, lo=-8, hi=12)]
    src = _tensor(wide, xs[0])
    wire = torch.empty(n, dtype=torch.uint8, device="cuda")
    sc = torch.empty(mx_ref.nblocks(n), dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.float16, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ftar.mx_scales(src, sc, n, wide, f8, headroom=1, stream=side)
            ftar.mx_quantize(src, wire, sc, n, wide, f8, mode="given", stream=side)
            ftar.mx_dequantize(wire, sc, out, n, f8, wide, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    for x in xs:
        src.copy_(_tensor(wide, x))
        g.replay()
        torch.cuda.synchronize()
        want_sc = mx_ref.scales(wide, f8, x, 1)
        want = mx_ref.quantize(wide, f8, x, want_sc)
        assert sc.cpu().numpy().tobytes() == want_sc.tobytes()
        check(f8, wire.cpu().numpy(), want)
        check(wide, _bits_of(wide, out), mx_ref.dequantize(f8, wide, want, want_sc))
    assert mx_ref.scales(wide, f8, xs[0], 1).tobytes() != mx_ref.scales(wide, f8, xs[1], 1).tobytes()


# ---- the MX gradient hook -------------------------------------------------------------------------------
N = 20_011
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


def _expect(dt, f8, ins, topo, headroom):
    """Every rank's scales, their MAX, the quantize at those, the AVG schedule on the wire, the dequantize:
    (the bucket every rank ends with, the agreed scale bytes, the reduced wire)."""
    sc = np.maximum.reduce([mx_ref.scales(dt, f8, x, headroom) for x in ins])
    wire = [mx_ref.quantize(dt, f8, x, sc) for x in ins]
    red = amax_ref.schedule(f8, wire, topo, "avg")
    return mx_ref.dequantize(f8, dt, red, sc), sc, red


def _nonzero_blocks(dt, bits):
    """Per block: does it hold an element that is not +-0?"""
    pad = np.zeros(mx_ref.nblocks(bits.size) * mx_ref.BLOCK, np.uint32)
    pad[:bits.size] = bits & amax_ref.LAYOUT[dt][1]
    return pad.reshape(-1, mx_ref.BLOCK).any(axis=1)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("topo,form,headroom,apart", [("2,2", "direct", 0, 6), ("1", "stages", 2, 0),
                                                      ("4", "direct", 0, 0), ("2,2", "direct", 1, 0)])
def test_mx_compress_hook_over_threads(topo, form, headroom, apart, dt, fmt):
    """P = 4 ranks on threads; the magnitudes step block by block over 2^-30 .. 2^10 (fp16: from 2^-22), the same
    steps on every rank.  Then the same bucket through fp8_compress_hook at scale 1, which loses the small blocks;
    then a NaN planted on one rank.

    The expectation of finite inputs must hold no NaN and no inf, which the headroom has to pay for wherever the
    schedule rounds a partial sum to fp8.  With apart == 0 every rank's block peaks at the same magnitude, the worst
    case: the flat one-round fold ("4") sums all four in fp32 and needs no headroom; the ring's hops store sums of
    up to three values and get headroom 2 (ceil(log2 P)); the "2,2" tree stores each pair's sum in fp8 in EVERY form
    (the one-round forms reproduce the staged bits) and gets headroom 1.  At headroom 0 the "2,2" tree is run on
    ranks whose values lie `apart` = 6 binades under the previous rank's: a pair's stored sum is then at most
    448 x (1 + 2^-6) = 455 <= 464 in e4m3, 57344 x (1 + 2^-6) < 61440 in e5m2, which round to the largest finite
    value, so nothing overflows; two equal peaks on one pair would (896 is NaN in e4m3)."""
    import torch

    import ftar.ddp
    P = 4
    f8 = "f8" + fmt
    g = group(P)
    g.set_chunk_bytes(0)
    g.set_allgather(form)
    g.set_reduce_scatter(form)
    assert N % mx_ref.BLOCK
    ins = [spread(dt, N, seed=20 + r, block_seed=19, down=apart * r) for r in range(P)]
    want, sc, red = _expect(dt, f8, ins, topo, headroom)
    assert not f8_ref.nan_mask(f8, red).any() and not cast_ref.nan_mask(dt, want).any(), "finite in, no NaN expected"
    assert ((red & 0x7F) <= f8_ref.MAX_FINITE[f8]).all(), "and no inf on the wire"
    assert not (sc == 255).any() and len(np.unique(sc)) > 20
    states = [ftar.ddp.MxCompressState(g[r], fmt=fmt, topo=topo, headroom=headroom) for r in range(P)]
    ts = [_tensor(dt, x) for x in ins]
    _on_threads(P, lambda r: ftar.ddp.mx_compress_hook(states[r], Bucket(ts[r])).wait())
    got = [_bits_of(dt, ts[r]) for r in range(P)]
    for r in range(P):
        assert f8_ref.same_bits(f8, from_dev(states[r]._wire, np.uint8, N), red), (r, "the reduced wire")
        assert from_dev(states[r]._scales, np.uint8, sc.size).tobytes() == sc.tobytes(), r
        check(dt, got[r], want, r)
        assert float(states[r].found_inf()) == 0.0 and states[r].found_inf().is_cuda and states[r].calls == 1
    # the one-scale wire on the same bucket: a block it returns as all zeros comes back non-zero here
    olds = [ftar.ddp.Fp8CompressState(g[r], fmt=fmt, topo=topo) for r in range(P)]
    ts1 = [_tensor(dt, x) for x in ins]
    _on_threads(P, lambda r: ftar.ddp.fp8_compress_hook(olds[r], Bucket(ts1[r])).wait())
    lost, kept = ~_nonzero_blocks(dt, _bits_of(dt, ts1[0])), _nonzero_blocks(dt, got[0])
    assert (lost & kept).any(), "a block the one-scale wire zeroes keeps values on the MX wire"
    # a NaN on one rank: that block NaN on every rank, found_inf() 1.0 on every rank
    p = 4321
    bad = [x.copy() for x in ins]
    bad[1][p] = amax_ref.encode(dt, float("nan"))
    want2, sc2, _ = _expect(dt, f8, bad, topo, headroom)
    blk = np.repeat(np.arange(sc2.size), mx_ref.BLOCK)[:N] == p // mx_ref.BLOCK
    assert sc2[p // mx_ref.BLOCK] == 255 and (sc2 == 255).sum() == 1
    assert np.array_equal(cast_ref.nan_mask(dt, want2), blk)
    ts2 = [_tensor(dt, x) for x in bad]
    _on_threads(P, lambda r: ftar.ddp.mx_compress_hook(states[r], Bucket(ts2[r])).wait())
    for r in range(P):
        check(dt, _bits_of(dt, ts2[r]), want2, r)
        assert float(states[r].found_inf()) == 1.0
        states[r].reset()
        assert float(states[r].found_inf()) == 0.0
    assert bool(torch.isfinite(ts[0].float()).all())


def test_mx_compress_hook_refuses_an_i32_bucket_before_any_device_work():
    import torch

    import ftar.ddp
    state = ftar.ddp.MxCompressState(group(4)[0], topo="2,2")
    t = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ftar.ddp.mx_compress_hook(state, Bucket(t))
    torch.cuda.synchronize()
    assert bool((t == 7).all()) and state._wire is None and state.calls == 0
