"""ftar_cast_half_sr (include/ftar.h) without a GPU: the symbol, every refusal in its order (fake pointers: nothing
here may reach HIP), the Python checks, and tests/half_sr_ref.py against the contract's own statements."""
import math
import os

import numpy as np
import pytest

import cast_ref
import half_sr_ref as hr

INVALID_ARG, UNSUPPORTED = 1, 2
SRC, DST, WORD, SEED = 0x10000, 0x20000, 0x30000, 0x40000      # fake pointers
DSTS = ("bf16", "f16")
TOP = (1 << 32) - 1


def call(src, sdt, dst, ddt, count, scale=None, seed=SEED, offset=0, amax=None):
    import ftar
    return ftar.lib().ftar_cast_half_sr(src, sdt, dst, ddt, count, scale, seed, offset, amax, None)


def test_the_symbol_and_its_refusals_in_their_order():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "ftar_cast_half_sr(" in open(os.path.join(root, "include", "ftar.h")).read()
    passed = []
    for s in range(14):
        for d in range(14):
            if call(None, s, None, d, 1) == INVALID_ARG:
                passed.append((s, d))
            else:      # the pair is refused first, whatever else is wrong
                assert call(SRC, s, DST, d, 1, WORD + 1, SEED + 4, 0, WORD + 2) == UNSUPPORTED
                assert call(SRC, s, DST, d, 0, None, None) == UNSUPPORTED
    assert passed == [(6, 9), (6, 10)]
    for ddt in (9, 10):
        assert call(None, 6, DST, ddt, 5) == call(SRC, 6, None, ddt, 5) == INVALID_ARG
        for count in (0, 5):
            assert call(SRC, 6, DST, ddt, count, seed=None) == INVALID_ARG
            assert all(call(SRC, 6, DST, ddt, count, seed=SEED + o) == INVALID_ARG for o in range(1, 8))
            assert all(call(SRC, 6, DST, ddt, count, WORD + o) == INVALID_ARG for o in (1, 2, 3))
            assert all(call(SRC, 6, DST, ddt, count, amax=WORD + o) == INVALID_ARG for o in (1, 2, 3))
        assert call(None, 6, None, ddt, 0, offset=TOP << 32) == 0      # nothing to do, no amax: no device work


def test_python_argument_checks():
    import torch

    import ftar
    import ftar.ddp as ddp
    with pytest.raises(ValueError):
        ftar.cast_half_sr(SRC, DST, 4, "f32", "bf16", None)
    with pytest.raises(ftar.FtarError) as e:
        ftar.cast_half_sr(SRC, DST, 4, "bf16", "f16", SEED)
    assert e.value.status == UNSUPPORTED
    a, b, sd = torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int64)
    for kw in (dict(seed=None), dict(seed=torch.zeros(2, dtype=torch.int64)), dict(seed=torch.zeros(1)), dict(seed=7),
               dict(seed=torch.zeros(1, dtype=torch.int64, device="meta")), dict(seed=sd, scale=torch.zeros(2)),
               dict(seed=sd, amax=torch.zeros(1, dtype=torch.float64)), dict(seed=sd, dst=b[:4]), dict(seed=sd, dst=b[::2])):
        with pytest.raises(ValueError):
            ftar.cast_half_sr_tensor(a, **{"dst": b, **kw})
    for kw in (dict(fmt="e4m3"), dict(fmt="f32"), dict(rounding="bogus"), dict(rounding=None), dict(seed=1.5), dict(seed=True)):
        with pytest.raises(ValueError):
            ddp.HalfCompressState(None, **kw)
    s = ddp.HalfCompressState(None, seed=5)
    assert (s.fmt, s.rounding, s.base_seed, s.seed, s.offset) == ("bf16", "stochastic", 5, None, 0)
    with pytest.raises(ValueError):      # a bucket that is not f32
        ddp.half_compress_hook(s, type("Bucket", (), {"buffer": lambda self: b})())


@pytest.mark.parametrize("low", (0x0001, 0x7FFF, 0x8000, 0xFFFF), ids=hex)
@pytest.mark.parametrize("dt", DSTS)
def test_the_reference_on_every_f32_high_half(dt, low):
    u = (np.arange(65536, dtype=np.uint32) << np.uint32(16)) | np.uint32(low)
    a = u & np.uint32(0x7FFFFFFF)
    finite, nan, inf = a < np.uint32(0x7F800000), a > np.uint32(0x7F800000), hr.INF[dt]
    F = hr.frac32(dt, u).astype(np.uint64)
    thr = (np.uint64(1) << np.uint64(32)) - F
    down, top = hr.sr16_bits(dt, u, 0), hr.sr16_bits(dt, u, TOP)
    up = hr.sr16_bits(dt, u, (thr & np.uint64(TOP)).astype(np.uint32))
    below = hr.sr16_bits(dt, u, ((thr - np.uint64(1)) & np.uint64(TOP)).astype(np.uint32))
    with np.errstate(invalid="ignore"):
        v = a.view(np.float32).astype(np.float64)
    # word 0 truncates toward zero: the stored magnitude is the largest one not above |p| (inf from 2 x 2^emax on)
    m = finite & (v < 2 * 2.0 ** (127 if dt == "bf16" else 15))
    lo_v, next_v = hr.widen(dt, down & 0x7FFF), hr.widen(dt, np.minimum((down & 0x7FFF) + 1, inf).astype(np.uint16))
    assert (lo_v[m] <= v[m]).all() and (v[m] < next_v[m]).all() and ((down ^ (u >> 16)) & 0x8000 == 0).all()
    assert ((down & 0x7FFF)[~m & ~nan] == inf).all()
    # the threshold word rounds up, the one below it down; F = 0 is a representable value and stays for every word
    has = m & (F > 0)
    assert has.sum() > 10000 and ((up & 0x7FFF)[has] == (down & 0x7FFF)[has] + 1).all() and (below[has] == down[has]).all()
    assert (top[m & (F == 0)] == down[m & (F == 0)]).all() and (top[has] == up[has]).all()
    for w in (down, top, up, below):      # the carry never reaches a NaN
        assert ((w & 0x7FFF)[nan] > inf).all() and ((w & 0x7FFF)[~nan] <= inf).all()


@pytest.mark.parametrize("dt", DSTS)
def test_fixed_points_and_the_overflow_band(dt):
    enc = np.arange(65536, dtype=np.uint16)
    u = cast_ref.widen_bits(dt, enc)
    assert not hr.frac32(dt, u).any()
    for w in (0, TOP):      # every encoding stays, -0 included
        assert cast_ref.same_bits(dt, hr.sr16_bits(dt, u, w), enc) and hr.sr16_bits(dt, u, w)[0x8000] == 0x8000
    # above the largest finite value: inf with probability frac; f16 from 65536 on always
    x = np.arange(1, 0x2000 if dt == "f16" else 0x10000, 7, dtype=np.uint32) + u[hr.INF[dt] - 1] | np.uint32(0x80000000)
    thr = (np.uint64(1) << np.uint64(32)) - hr.frac32(dt, x).astype(np.uint64)
    assert (hr.sr16_bits(dt, x, thr.astype(np.uint32)) == 0x8000 | hr.INF[dt]).all()
    assert (hr.sr16_bits(dt, x, (thr - np.uint64(1)).astype(np.uint32)) == 0x8000 | (hr.INF[dt] - 1)).all()
    big = np.array([65536.0, -65536.0, 65537.0, 3e38], np.float32).view(np.uint32)
    assert dt == "bf16" or [int(e) & 0x7FFF for e in hr.sr16_bits(dt, big, 0)] == [0x7C00] * 4


def test_a_value_between_two_bf16_encodings_keeps_its_mean():
    """0.3 to bf16 over 2^20 words: neighbours 0.298828125 and 0.30078125, within 5 sigma of the binomial."""
    N, v = 1 << 20, float(np.float32(0.3))
    back = hr.widen("bf16", hr.sr_cast("bf16", np.full(N, np.float32(0.3)).view(np.uint32), None, 11))
    assert list(np.unique(back)) == [0.298828125, 0.30078125]
    ulp = 2.0 ** -9
    f = (v - 0.298828125) / ulp
    assert abs(back.mean() - v) < 5 * ulp * math.sqrt(f * (1 - f) / N)
