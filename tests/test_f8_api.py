"""The two OCP fp8 dtypes at the API surface, without a GPU: the enum tables, what is refused before any device
work, the plan flag the fp8 ring fold depends on, and the self-checks of the CPU expectations (tests/f8_ref.py)
that the GPU tests in tests/test_gpu_f8.py and tests/test_gpu_f8_edges.py compare against."""
import numpy as np
import pytest

import f8_ref as ref

UNSUPPORTED = 2   # FTAR_ERR_UNSUPPORTED


def test_enum_tables_sizes_and_torch_names():
    import torch

    import ftar
    assert ftar.DTYPE["f8e4m3"] == 12 and ftar.DTYPE["f8e5m2"] == 13
    assert {n: ftar.DTYPE[n] for n in ref.ID} == ref.ID
    assert ftar.dtype_size("f8e4m3") == 1 and ftar.dtype_size("f8e5m2") == 1
    assert ftar._dt(torch.float8_e4m3fn) == 12 and ftar._dt(torch.float8_e5m2) == 13
    assert ftar._dt("torch.float8_e4m3fn") == 12 and ftar._dt("torch.float8_e5m2") == 13
    assert 11 not in ftar.DTYPE.values() and ftar.dtype_size(11) == 0          # 11 stays unassigned
    with pytest.raises(ftar.FtarError):
        ftar.reduce([1024, 2048], 4096, 10, 11, "sum")
    assert not any(v in (12, 13) for v in ftar.MPI_DTYPE.values())             # the MPI list stays the reference's
    for fnuz in ("torch.float8_e4m3fnuz", "torch.float8_e5m2fnuz"):            # MI300X's encodings are not these
        with pytest.raises(ValueError):
            ftar._dt(fnuz)


@pytest.mark.parametrize("dt", ref.FORMATS)
def test_band_is_refused_before_any_device_work(dt):
    """Fake pointers: the refusal must come before anything touches HIP."""
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048], 4096, 10, dt, "band")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048, 4096, 8192], 16384, 10, dt, "band", shape=[2, 2])
    assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("dt", ref.FORMATS)
def test_reduce_refuses_avg(dt):
    """A one-device reduce has no P: flat and nested refuse AVG, with fake pointers."""
    import ftar
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048], 4096, 10, dt, "avg")
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ftar.FtarError) as e:
        ftar.reduce([1024, 2048, 4096, 8192], 16384, 10, dt, "avg", shape=[2, 2])
    assert e.value.status == UNSUPPORTED


def test_f8_conversion_hook_lives_in_the_bench_library_only():
    import ftar
    assert hasattr(ftar.bench_lib(), "ftar_debug_f8_cvt_check")
    assert not hasattr(ftar.lib(), "ftar_debug_f8_cvt_check")


@pytest.mark.parametrize("P", [2, 4, 8])
def test_one_round_ring_plan_still_rounds_every_hop(P):
    """The plan carries round_each whatever the dtype: the fp8 ring fold reproduces the staged ring through it."""
    import ftar
    for r in range(P):
        items = [it for st in ftar.plan_json("1", P, r, 50_001)["stages"] for it in st["reduces"]]
        assert len(items) == 1 and items[0]["round_each"] == 1 and len(items[0]["srcs"]) == P


# ---- the helper's own checks ----------------------------------------------------------------------------
@pytest.mark.parametrize("low", [0x000, 0x001, 0xFFF])
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_integer_rne_is_torchs_cast_on_every_tie_and_its_neighbours(dt, low):
    """Every value of a float's high 20 bits with the low 12 bits 0x000, 0x001, 0xfff: a tie of either format
    has its low 20 (e4m3) or 21 (e5m2) bits equal to 0x80000 / 0x100000, so all of them are among the 0x000
    patterns and their two neighbours among the others; the subnormal ties (a shorter mantissa) likewise."""
    import torch
    u = (np.arange(1 << 20, dtype=np.uint32) << np.uint32(12)) | np.uint32(low)
    want = ref._bits(torch.from_numpy(u.view(np.float32).copy()).to(ref.torch_dtype(dt)))
    got = ref.rne_bits(dt, u)
    nw, ng = ref.nan_mask(dt, want), ref.nan_mask(dt, got)
    bad = np.flatnonzero((nw != ng) | (~nw & (got != want)))
    assert not bad.size, (hex(int(u[bad[0]])), hex(int(got[bad[0]])), hex(int(want[bad[0]])), bad.size)


@pytest.mark.parametrize("dt", ref.FORMATS)
def test_overflow_rules_and_the_round_trip(dt):
    f32 = lambda *v: np.array(v, np.float32).view(np.uint32)   # noqa: E731
    if dt == "f8e4m3":     # no inf: above 464 (a tie that goes to the even 448) everything is NaN
        assert ref.rne_bits(dt, f32(448, 464, -464)).tolist() == [0x7E, 0x7E, 0xFE]
        assert ref.nan_mask(dt, ref.rne_bits(dt, f32(np.nextafter(np.float32(464), np.float32(1e9)), 480, 1e9,
                                                     np.inf, -np.inf, np.nan))).all()
    else:                  # IEEE-like: 61440 is a tie that goes to the even encoding, inf's
        assert ref.rne_bits(dt, f32(57344, np.nextafter(np.float32(61440), np.float32(0)), 61440, -1e9,
                                    np.inf)).tolist() == [0x7B, 0x7B, 0x7C, 0xFC, 0x7C]
        assert ref.nan_mask(dt, ref.rne_bits(dt, f32(np.nan))).all()
    b = np.arange(256, dtype=np.uint8)                          # all 256 encodings widen and narrow back
    back = ref.rne_bits(dt, ref._t(dt, b).float().numpy().view(np.uint32))
    assert ref.same_bits(dt, back[~ref.nan_mask(dt, b)], b[~ref.nan_mask(dt, b)])
    assert np.array_equal(ref.nan_mask(dt, back), ref.nan_mask(dt, b))


def test_key_order_hand_written_cases():
    """Encodings in ascending order of value, -0 below +0, subnormals in place (e5m2 with its infs)."""
    asc = np.array([0xFC, 0xFB, 0xBC, 0x84, 0x83, 0x81, 0x80, 0x00, 0x01, 0x03, 0x04, 0x3C, 0x7B, 0x7C], np.uint8)
    assert np.all(np.diff(ref.keys(asc).astype(np.int64)) > 0)
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.keys_to_bits(ref.keys(every)), every)
    a, b = np.array([0x80, 0x00, 0x01, 0x81, 0x7F], np.uint8), np.array([0x00, 0x80, 0x02, 0x82, 0x38], np.uint8)
    for dt in ref.FORMATS:
        mx, mn = ref.minmax(dt, "max", [a, b]), ref.minmax(dt, "min", [a, b])
        assert mx[:4].tolist() == [0x00, 0x00, 0x02, 0x81] and mn[:4].tolist() == [0x80, 0x80, 0x01, 0x82]
        assert ref.nan_mask(dt, mx)[4] and ref.nan_mask(dt, mn)[4]
    # 0x7d is an ordinary e4m3 value (416) and an e5m2 NaN
    c, d = np.array([0x7D], np.uint8), np.array([0x38], np.uint8)
    assert ref.minmax("f8e4m3", "max", [c, d])[0] == 0x7D and ref.nan_mask("f8e5m2", ref.minmax("f8e5m2", "min", [c, d]))[0]


@pytest.mark.parametrize("k", [2, 8, 16])
@pytest.mark.parametrize("dt", ref.FORMATS)
def test_sources_carry_the_planted_lanes_and_few_nans(dt, k):
    n = 50_001
    ins, flat = ref.fold_case(dt, k, n)
    assert len(ins) == k and all(x.size == n and x.dtype == np.uint8 for x in ins)
    per_source = [float(ref.nan_mask(dt, x).mean()) for x in ins]
    assert per_source[0] > 0 and max(per_source[1:]) == 0                      # NaNs only where planted
    bulk = np.ones(n, bool)
    for off, stride in ((31, 97), (3, 89), (5, 83), (17, 103), (18, 103), (13, 79), (19, 107), (20, 107), (21, 107)):
        bulk[off::stride] = False
    assert all(((x[bulk] & 0x40) == 0).all() for x in ins)                     # |x| < 2 in the bulk
    assert not ref.nan_mask(dt, ins[0][:1]).any() and bulk[0]                  # lane 0 is ordinary
    (_, _, t0), (_, _, t1) = ref.TIES[dt]
    assert flat[19] == t0 and flat[20] == t1                                   # 16 + 1 -> 16, 18 + 1 -> 20 (e5m2: 8, 12)
    assert ref.encode(dt, [16.0, 20.0] if dt == "f8e4m3" else [8.0, 12.0]).tolist() == [t0, t1]
    assert (flat[21] & 0x7F) == (0x7F if dt == "f8e4m3" else 0x7C)             # max + max: NaN / +inf
    assert flat[11] == 0 and flat[12] == 0                                     # -0 + +0 = +0 under RNE
    assert ref.minmax(dt, "max", ins)[11] == 0 and ref.minmax(dt, "min", ins)[12] == 0x80   # -0 < +0
    assert ref.minmax(dt, "max", ins)[17] == k and ref.minmax(dt, "min", ins)[18] == (0x80 | k)
    if dt == "f8e5m2":
        assert (ins[k - 1] == 0x7C).any() and (ins[k // 2] == 0xFC).any()
    share = float(ref.nan_mask(dt, flat).mean())
    assert 0 < share < 0.025 and ref.same_bits(dt, flat, flat)
    if k >= 8:   # a wrong schedule cannot pass: the flat and the per-hop fold part in a third of the lanes
        assert float((ref.hop_fold(dt, ins) != flat).mean()) > 0.25


@pytest.mark.parametrize("dt", ref.FORMATS)
def test_schedules_differ_and_the_one_round_mean_survives_the_overflow(dt):
    P, n = 8, 50_001
    ins, flat = ref.fold_case(dt, P, n)
    rg, tr, ne = ref.ring(dt, ins), ref.tree(dt, ins, [2, 4]), ref.nested(dt, ins, [2, 4])
    for out in (rg, tr, ne):
        assert float(ref.nan_mask(dt, out).mean()) < 0.025 and ref.same_bits(dt, out, out)
    assert not ref.same_bits(dt, rg, flat) and not ref.same_bits(dt, tr, rg)
    mean = ref.fold(dt, ins, ref.recip(P))       # max + max = 2 max; / 8: finite in both formats
    assert not ref.nan_mask(dt, mean)[21] and mean[21] == ref.encode(dt, [448.0 / 4 if dt == "f8e4m3" else 57344.0 / 4])[0]
    ins4, want = ref.exact_sum_case(dt, 5, 1001)
    assert ref.same_bits(dt, ref.fold(dt, ins4), want) and ref.same_bits(dt, ref.ring(dt, ins4), want)


def test_same_bits_sees_a_single_wrong_lane_and_ignores_nan_payloads():
    ins, want = ref.fold_case("f8e5m2", 3, 4099)
    nan = np.flatnonzero(ref.nan_mask("f8e5m2", want))
    got = want.copy()
    got[nan[0]] = 0xFE                          # another NaN: the same
    assert ref.same_bits("f8e5m2", got, want)
    got[nan[0]] = 0x7C                          # inf where a NaN belongs
    assert not ref.same_bits("f8e5m2", got, want) and ref.first_diff("f8e5m2", got, want)[0] == nan[0]
    got = want.copy()
    got[7] ^= 1
    assert not ref.same_bits("f8e5m2", got, want) and ref.first_diff("f8e5m2", got, want)[0] == 7
    raw = [np.random.default_rng(j).integers(0, 256, 20_000, dtype=np.uint8) for j in range(16)]
    with pytest.raises(AssertionError, match="NaN lanes"):     # raw bytes are 2.3 % NaN per source: about 30 % NaN lanes at 16 sources
        ref.same_bits("f8e5m2", ref.minmax("f8e5m2", "max", raw), ref.minmax("f8e5m2", "max", raw))
