"""The stochastic-rounding quantize (include/ftar.h: ftar_cast_scaled_sr) without a GPU: the symbol, every refusal
in its order (with fake pointers: nothing here may reach HIP), the Python checks, the rounding function of
tests/sr_ref.py against its own definition, the generator's statistics, and the unbiasedness of the whole
reference."""
import math
import os

import numpy as np
import pytest

import cast_ref
import sr_ref

INVALID_ARG, UNSUPPORTED = 1, 2
FAKE_SRC, FAKE_DST, FAKE_WORD, FAKE_SEED = 0x10000, 0x20000, 0x30000, 0x40000
QUANT = [(w, f) for w in cast_ref.WIDE for f in cast_ref.F8]
LOWS = (0x0001, 0x7FFF, 0x8000, 0xFFFF)
TOP = (1 << 32) - 1


def call(src, sdt, dst, ddt, count, scale=None, seed=FAKE_SEED, offset=0, amax=None):
    import ftar
    return ftar.lib().ftar_cast_scaled_sr(src, sdt, dst, ddt, count, scale, seed, offset, amax, None)


# ---- the entry point --------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared():
    import ftar
    assert hasattr(ftar.lib(), "ftar_cast_scaled_sr")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "ftar_cast_scaled_sr(" in open(os.path.join(root, "include", "ftar.h")).read()


def test_every_pair_but_the_six_quantizes_is_refused_first():
    """All dtype ids 0..13 squared: an unsupported pair (the dequantize pairs among them) is status 2 whatever the
    other arguments; a quantize pair gets past that check and is refused for its NULL pointers, status 1."""
    passed = []
    for s in range(14):
        for d in range(14):
            st = call(None, s, None, d, 1)
            assert st in (INVALID_ARG, UNSUPPORTED), (s, d, st)
            if st == INVALID_ARG:
                passed.append((s, d))
            else:
                assert call(FAKE_SRC, s, FAKE_DST, d, 1, FAKE_WORD + 1, FAKE_SEED + 4, 0, FAKE_WORD + 2) == UNSUPPORTED
                assert call(FAKE_SRC, s, FAKE_DST, d, 1, None, None) == UNSUPPORTED
                assert call(FAKE_SRC, s, FAKE_DST, d, 0) == UNSUPPORTED
    assert sorted(passed) == sorted((cast_ref.ID[a], cast_ref.ID[b]) for a, b in QUANT) and len(passed) == 6
    for f, w in ((f, w) for f in cast_ref.F8 for w in cast_ref.WIDE):
        assert call(FAKE_SRC, cast_ref.ID[f], FAKE_DST, cast_ref.ID[w], 4) == UNSUPPORTED
    for s in (-1, 14, 11, 255):
        assert call(FAKE_SRC, s, FAKE_DST, 12, 1) == UNSUPPORTED and call(FAKE_SRC, 6, FAKE_DST, s, 1) == UNSUPPORTED


@pytest.mark.parametrize("sdt,ddt", [(cast_ref.ID[a], cast_ref.ID[b]) for a, b in QUANT])
def test_null_and_misaligned_arguments(sdt, ddt):
    assert call(None, sdt, FAKE_DST, ddt, 5) == INVALID_ARG
    assert call(FAKE_SRC, sdt, None, ddt, 5) == INVALID_ARG
    assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 5, seed=None) == INVALID_ARG
    assert call(None, sdt, None, ddt, 0, seed=None) == INVALID_ARG            # also with nothing to do
    for off in range(1, 8):
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 5, seed=FAKE_SEED + off) == INVALID_ARG
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 0, seed=FAKE_SEED + off) == INVALID_ARG
    for off in (1, 2, 3):
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 5, FAKE_WORD + off) == INVALID_ARG
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 5, amax=FAKE_WORD + off) == INVALID_ARG
        assert call(FAKE_SRC, sdt, FAKE_DST, ddt, 0, FAKE_WORD + off) == INVALID_ARG
    assert call(None, sdt, None, ddt, 0) == 0        # nothing to do, no amax: success without device work
    assert call(None, sdt, None, ddt, 0, offset=TOP << 32) == 0


def test_python_rounding_argument_checks():
    import torch

    import ftar
    for bad in ("bogus", "Stochastic", None, 1):
        with pytest.raises(ValueError):
            ftar.cast_scaled(FAKE_SRC, FAKE_DST, 4, "bf16", "f8e4m3", rounding=bad, seed=FAKE_SEED)
    with pytest.raises(ValueError):
        ftar.cast_scaled(FAKE_SRC, FAKE_DST, 4, "bf16", "f8e4m3", rounding="stochastic")
    with pytest.raises(ftar.FtarError) as e:
        ftar.cast_scaled(FAKE_SRC, FAKE_DST, 4, "f8e4m3", "bf16", rounding="stochastic", seed=FAKE_SEED)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.cast_scaled(FAKE_SRC, FAKE_DST, 4, "f32", "f8e5m2", rounding="stochastic", seed=FAKE_SEED + 4)
    assert e.value.status == INVALID_ARG
    a = torch.zeros(8, dtype=torch.bfloat16)
    b = torch.zeros(8, dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError):
        ftar.cast_scaled_tensor(a, b, rounding="bogus")
    with pytest.raises(ValueError):
        ftar.cast_scaled_tensor(a, b, rounding="stochastic")
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1), 7,
                torch.zeros(1, dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError):
            ftar.cast_scaled_tensor(a, b, rounding="stochastic", seed=bad)


def test_fp8_compress_state_rounding_arguments():
    import ftar.ddp as ddp
    for kw in (dict(rounding="bogus"), dict(rounding=None), dict(seed=1.5), dict(seed=True), dict(seed="7")):
        with pytest.raises(ValueError):
            ddp.Fp8CompressState(None, **kw)
    s = ddp.Fp8CompressState(None)
    assert (s.rounding, s.seed, s.offset) == ("nearest", None, 0)
    s = ddp.Fp8CompressState(None, rounding="stochastic", seed=5)
    assert (s.rounding, s.base_seed, s.seed, s.offset) == ("stochastic", 5, None, 0)
    seeds = {ddp.rank_seed(sd, r) for sd in (0, 1, 5) for r in range(8)}
    assert len(seeds) == 24 and all(0 <= x < 1 << 64 for x in seeds)
    assert all(ddp.rank_seed(sd, r) == sr_ref.rank_seed(sd, r) for sd in (0, 1, 1 << 63, -1) for r in range(4))


# ---- the rounding function against its own definition ---------------------------------------------------------
def f32_sweep(low):
    return (np.arange(65536, dtype=np.uint32) << np.uint32(16)) | np.uint32(low)


def _same(dt, got, want, what=""):
    assert cast_ref.same_bits(dt, got, want), (what, cast_ref.first_diff(dt, got, want))


@pytest.mark.parametrize("dt", cast_ref.F8)
def test_every_fp8_encoding_is_a_fixed_point(dt):
    enc = np.arange(256, dtype=np.uint8)
    u = cast_ref.widen_bits(dt, enc)
    assert not sr_ref.frac32(dt, u).any()
    for w in (0, 1, 1 << 31, TOP):
        _same(dt, sr_ref.sr_bits(dt, u, w), enc, w)
    assert sr_ref.sr_bits(dt, u, TOP)[0x80] == 0x80         # -0 stays -0


@pytest.mark.parametrize("low", (0,) + LOWS, ids=hex)
@pytest.mark.parametrize("dt", cast_ref.F8)
def test_word_zero_is_truncation_toward_zero(dt, low):
    u = f32_sweep(low)
    _same(dt, sr_ref.sr_bits(dt, u, 0), sr_ref.trunc_bits(dt, u), hex(low))


@pytest.mark.parametrize("dt", cast_ref.F8)
def test_the_result_is_monotone_in_the_word_and_one_of_two_neighbours(dt):
    ws = [0, 1, 0x1234, 1 << 16, 0x7FFFFFFF, 1 << 31, 0xC0000000, TOP - 1, TOP]
    for low in LOWS:
        u = f32_sweep(low)
        finite = (u & np.uint32(0x7FFFFFFF)) < np.uint32(0x7F800000)
        prev = sr_ref.sr_bits(dt, u, ws[0])
        lo = prev.copy()
        for w in ws[1:]:
            cur = sr_ref.sr_bits(dt, u, w)
            assert ((cur & 0x7F)[finite] >= (prev & 0x7F)[finite]).all()      # the magnitude's encoding never falls
            assert ((cur & 0x7F)[finite] - (lo & 0x7F)[finite] <= 1).all()    # and is lo or the next encoding
            assert ((cur & 0x80) == (lo & 0x80))[finite].all()
            prev = cur


@pytest.mark.parametrize("low", LOWS, ids=hex)
@pytest.mark.parametrize("dt", cast_ref.F8)
def test_the_threshold_word_rounds_up_and_the_one_below_it_down(dt, low):
    """Every high half: 2^32 - F rounds up, 2^32 - F - 1 down (F = 0: a representable value, both stay).  F is
    checked against exact rational arithmetic on a sample that covers the subnormal range and the overflow bands."""
    from fractions import Fraction
    u = f32_sweep(low)
    a = u & np.uint32(0x7FFFFFFF)
    finite = a < np.uint32(0x7F800000)
    F = sr_ref.frac32(dt, u).astype(np.uint64)
    down = sr_ref.sr_bits(dt, u, 0)
    nxt = 65536.0 if dt == "f8e5m2" else 480.0
    inband = finite & (a.view(np.float32) < np.float32(nxt))
    up_w = ((np.uint64(1) << np.uint64(32)) - F).astype(np.uint64)
    has = F > 0
    got_up = sr_ref.sr_bits(dt, u, (up_w & np.uint64(TOP)).astype(np.uint32))
    got_dn = sr_ref.sr_bits(dt, u, ((up_w - np.uint64(1)) & np.uint64(TOP)).astype(np.uint32))
    m = has & inband
    assert m.sum() > 1000
    assert ((got_up & 0x7F)[m] == (down & 0x7F)[m] + 1).all()
    assert (got_dn[m] == down[m]).all()
    assert (got_up[~has & finite] == down[~has & finite]).all()
    # the overflow bands: the up-rounded value is NaN (e4m3) / inf (e5m2)
    mb, bias = cast_ref.FMT[dt]
    maxfin = cast_ref.widen_bits(dt, np.array([0x7B if dt == "f8e5m2" else 0x7E], np.uint8))[0]
    band = m & (a > maxfin)
    assert band.sum() > 0
    assert ((got_up & 0x7F)[band] == (0x7C if dt == "f8e5m2" else 0x7F)).all()
    assert ((got_dn & 0x7F)[band] == (0x7B if dt == "f8e5m2" else 0x7E)).all()
    # F itself, exactly, on every 37th positive high half below the band's end
    emin = 1 - bias
    for i in range(1, 32768, 37):
        if not inband[i]:
            continue
        v = cast_ref.frac_of("f32", int(u[i]))
        if v == 0:
            continue
        e = v.numerator.bit_length() - v.denominator.bit_length()
        if Fraction(2) ** e > v:
            e -= 1
        ulp = Fraction(2) ** (max(e, emin) - mb)
        frac = v / ulp - (v / ulp).numerator // (v / ulp).denominator
        assert int(F[i]) == (frac * (1 << 32)).numerator // (frac * (1 << 32)).denominator, hex(int(u[i]))


def test_specials():
    nan, inf, ninf, nz, tiny = 0x7FC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x80000001
    u = np.array([nan, inf, ninf, 0, nz, tiny, nan | 0x80000000], np.uint32)
    for w in (0, 12345, TOP):
        e4 = sr_ref.sr_bits("f8e4m3", u, w)
        e5 = sr_ref.sr_bits("f8e5m2", u, w)
        assert [int(x) & 0x7F for x in e4[[0, 1, 2, 6]]] == [0x7F] * 4
        assert int(e5[0]) & 0x7F > 0x7C and int(e5[6]) & 0x7F > 0x7C
        assert (int(e5[1]), int(e5[2])) == (0x7C, 0xFC)
        assert [int(x) for x in e4[[3, 4, 5]]] == [0, 0x80, 0x80] and [int(x) for x in e5[[3, 4, 5]]] == [0, 0x80, 0x80]
    # from 480 / 65536 on: always NaN / inf
    big = np.array([0x43F00000, 0x43F00001, 0x7F7FFFFF], np.uint32)
    assert [int(x) for x in sr_ref.sr_bits("f8e4m3", big, 0)] == [0x7F] * 3
    big = np.array([0x47800000, 0x47800001, 0x7F7FFFFF], np.uint32)
    assert [int(x) for x in sr_ref.sr_bits("f8e5m2", big, 0)] == [0x7C] * 3


# ---- the generator --------------------------------------------------------------------------------------
N = 1 << 20
SEEDS = (0, 1, 0x123456789ABCDEF, 0x123456789ABCDF0, (1 << 64) - 1)
STARTS = (0, (1 << 32) - N // 2, 1 << 63)


def _corr(a, b):
    a = a.astype(np.float64) / 2.0 ** 32 - 0.5
    b = b.astype(np.float64) / 2.0 ** 32 - 0.5
    return float((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean()))


@pytest.mark.parametrize("start", STARTS, ids=hex)
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_generator_battery(seed, start):
    """N consecutive indices (from 0, across g = 2^32, from 2^63); every bound is 5 sigma of the statistic under
    uniform independent words, derived from N."""
    g = sr_ref.indices(start, N + 1)
    w = sr_ref.words(seed, g)
    u, nxt = w[:N], w[1:]
    x = u.astype(np.float64) / 2.0 ** 32
    assert abs(x.mean() - 0.5) < 5 * math.sqrt(1 / 12 / N), x.mean()
    for b in range(32):
        f = float(((u >> np.uint32(b)) & np.uint32(1)).mean())
        assert abs(f - 0.5) < 5 * 0.5 / math.sqrt(N), (b, f)
    counts = np.bincount((u >> np.uint32(24)).astype(np.int64), minlength=256)
    chi2 = float(((counts - N / 256) ** 2 / (N / 256)).sum())
    assert abs(chi2 - 255) < 5 * math.sqrt(2 * 255), chi2
    assert abs(_corr(u, nxt)) < 5 / math.sqrt(N)                              # U(g) with U(g + 1)
    assert abs(_corr(u, sr_ref.words((seed + 1) & sr_ref.M64, g[:N]))) < 5 / math.sqrt(N)   # U(s, g) with U(s + 1, g)
    assert len(np.unique(u)) > N - 5 * math.sqrt(N) - N * N / 2 ** 33        # birthday collisions only


def test_neighbouring_seeds_are_neither_shifts_nor_permutations():
    g = sr_ref.indices(0, N)
    a, b = sr_ref.words(7, g), sr_ref.words(8, g)
    assert (a == b).sum() < 5
    for lag in range(1, 65):
        assert abs(_corr(a[lag:], b[:-lag])) < 5 / math.sqrt(N - lag)
        assert abs(_corr(a[:-lag], b[lag:])) < 5 / math.sqrt(N - lag)
    # as multisets over 2^20 indices two independent streams share about N^2 / 2^32 = 256 values, not N
    assert len(np.intersect1d(a, b)) < 256 + 5 * 16
    # the high index word changes the stream as a seed does
    c = sr_ref.words(7, sr_ref.indices(1 << 32, N))
    assert (a == c).sum() < 5 and abs(_corr(a, c)) < 5 / math.sqrt(N)
    assert sr_ref.keys(7) != sr_ref.keys(8)


def test_words_depend_on_the_index_alone():
    g = sr_ref.indices((1 << 32) - 8, 4099)
    whole = sr_ref.words(3, g)
    parts = np.concatenate([sr_ref.words(3, sr_ref.indices((1 << 32) - 8 + a, b - a)) for a, b in ((0, 5), (5, 4000), (4000, 4099))])
    assert np.array_equal(whole, parts)
    assert int(sr_ref.words(3, np.uint64((1 << 64) - 1))) == int(sr_ref.words(3, sr_ref.indices((1 << 64) - 2, 2))[1])


# ---- unbiasedness of the whole reference ----------------------------------------------------------------
def _mean_sigma(dt, value, seed):
    src = np.full(N, np.float32(value)).view(np.uint32)
    enc = sr_ref.sr_cast("f32", dt, src, None, seed, 0)
    back = cast_ref.widen_bits(dt, enc).view(np.float32).astype(np.float64)
    vals = np.unique(back)
    return back.mean(), vals


def test_a_value_between_two_encodings_keeps_its_mean():
    """0.3 to e4m3: neighbours 0.28125 and 0.3125; RNE stores 0.3125 everywhere, about 250 sigma off."""
    v = float(np.float32(0.3))
    mean, vals = _mean_sigma("f8e4m3", v, 11)
    assert list(vals) == [0.28125, 0.3125]
    ulp = 0.03125
    f = (v - 0.28125) / ulp
    sigma = ulp * math.sqrt(f * (1 - f) / N)
    assert abs(mean - v) < 5 * sigma, (mean, v, sigma)
    rne = cast_ref.widen_bits("f8e4m3", cast_ref.cast("f32", "f8e4m3", np.array([v], np.float32).view(np.uint32)))
    assert float(rne.view(np.float32)[0]) == 0.3125 and abs(0.3125 - v) > 200 * sigma


@pytest.mark.parametrize("dt,ulp", [("f8e4m3", 2.0 ** -9), ("f8e5m2", 2.0 ** -16)])
def test_a_value_below_half_the_smallest_subnormal_is_not_lost(dt, ulp):
    v = float(np.float32(ulp * 0.2))
    mean, vals = _mean_sigma(dt, -v, 12)
    assert sorted(vals) == [-ulp, 0.0]
    sigma = ulp * math.sqrt(0.2 * 0.8 / N)
    assert mean != 0 and abs(mean + v) < 5 * sigma, (mean, v, sigma)
    rne = cast_ref.cast("f32", dt, np.array([-v], np.float32).view(np.uint32))
    assert int(rne[0]) == 0x80
