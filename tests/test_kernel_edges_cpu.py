"""The kernel-edge helper (tests/kernel_edges.py) tested on the CPU: the edge counts, the geometry parsed from
kernel ids, and the footprint checker on a host tensor -- a checker that misses a changed byte would let every
GPU footprint test pass."""
import numpy as np
import pytest

import kernel_edges as ke


@pytest.mark.parametrize("ve,wg", [(16, 1024), (8, 1280), (4, 128), (4, 1152), (2, 512), (16, 64)])
def test_edge_counts_hold_every_boundary(ve, wg):
    edges = ke.edge_counts(ve, wg)
    assert all(e.n >= 0 and e.nvec >= 0 and 0 <= e.head < ve and 0 <= e.tail < ve for e in edges)
    assert all(e.n == e.head + e.nvec * ve + e.tail for e in edges)
    nvecs = {e.nvec for e in edges}
    assert {0, 1, 63, 64, 65, wg - 1, wg, wg + 1, wg + 64, 3 * wg - 1} <= nvecs
    if wg > 64:
        assert wg - 64 in nvecs
    pairs = {(0, 0), (0, ve - 1), (ve - 1, 0), (1, 1), (ve - 1, ve - 1)}
    for v in nvecs:
        assert {(e.head, e.tail) for e in edges if e.nvec == v} == pairs
    assert len(set(edges)) == len(edges)
    assert ke.Edge(2 * (ve - 1), ve - 1, 0, ve - 1) in edges        # no vector at all, a head and a tail
    assert ke.Edge(wg * ve, 0, wg, 0) in edges                      # exactly one full workgroup
    for e in edges:                                                 # the offset that produces the head
        off = ke.head_offset(ve, e.head)
        assert 0 <= off < ve and (off + e.head) % ve == 0


# one literal id of each family, as tests/test_gpu_avg.py spells them
IDS = [
    ("reduce_lds_kernel<F32Sum, 2, 1, 2, 2, true>", 2 * 1 * 64, (1, 2)),
    ("reduce_lds_scaled_kernel<F32Sum, 2, 1, 2, 2, true>", 2 * 1 * 64, (1, 2)),
    ("reduce_lds_kernel<H16SumHopT<Bf16Fmt<true>>, 8, 4, 2, 2, true>", 2 * 4 * 64, (4, 2)),
    ("reduce_lds_kernel<MinMax<float, true>, 3, 3, 6, 2, true>", 6 * 3 * 64, (3, 6)),
    ("reduce_vec_kernel<F32Sum, 0, 2, true, true, 512>", 2 * 512, None),
    ("reduce_vec_scaled_kernel<F32Sum, 0, 2, true, true, 512>", 2 * 512, None),
    ("reduce_tree_lds_kernel<F32Sum, 4, 3, 6, StaticShape<2, 2>>", 6 * 3 * 64, (3, 6)),
    ("reduce_tree_lds_scaled_kernel<F32Sum, 8, 4, 2, StaticShape<2, 2, 2>>", 2 * 4 * 64, (4, 2)),
    ("reduce_tree_kernel<F64Sum, 4, 2, StaticShape<2, 2>>", 2 * 256, None),
    ("reduce_tree_scaled_kernel<F64Sum, 16, 1, RuntimeShape>", 256, None),
    ("reduce_elem_kernel<F32Sum>", 256, None),
    ("reduce_tree_elem_scaled_kernel<F32Sum>", 256, None),
    ("gather_kernel<true, false>", 2 * 256, None),
    ("reduce_lds_amax_kernel<F32Sum, 2, 4, 4, 2, true>", 4 * 4 * 64, (4, 4)),     # 4-byte k = 2 under amax: 4 x 4
    ("reduce_lds_amax_kernel<F8SumHopPreT<F8Fmt<true>>, 8, 4, 2, 2, true>", 2 * 4 * 64, (4, 2)),
    ("reduce_vec_amax_kernel<H16SumT<HalfFmt>, 0, 2, true, true, 512>", 2 * 512, None),
    ("reduce_tree_lds_amax_kernel<F8SumT<F8Fmt<false>>, 4, 4, 4, StaticShape<2, 2>>", 4 * 4 * 64, (4, 4)),
    ("reduce_tree_amax_kernel<H16SumT<Bf16Fmt<true>>, 6, 2, RuntimeShape>", 2 * 256, None),
    ("reduce_elem_amax_kernel<F32Sum>", 256, None),
    ("reduce_tree_elem_amax_kernel<F32Sum>", 256, None),
]


@pytest.mark.parametrize("symbol,wg_tile,shape", IDS)
def test_geometry_from_a_kernel_id(symbol, wg_tile, shape):
    assert ke.tiles(symbol) == (64, wg_tile)
    g = ke.geometry(symbol)
    assert g.lds_shape == shape
    assert g.family == symbol.split("<")[0].replace("_scaled", "").replace("_amax", "")


def test_geometry_reads_the_rocprof_spelling_through_kernel_symbol():
    from ftar.names import kernel_symbol
    raw = ("void ftar::(anonymous namespace)::reduce_tree_lds_kernel<ftar::(anonymous namespace)::F32Sum, 4, 3, 6, "
           "ftar::(anonymous namespace)::StaticShape<2, 2> >(ftar::(anonymous namespace)::Srcs<4>, "
           "ftar::(anonymous namespace)::TreeCode, void*, unsigned long, int, int)")
    assert ke.tiles(kernel_symbol(raw)) == (64, 6 * 3 * 64)
    assert ke.template_args("noop_kernel") == ("noop_kernel", [])
    with pytest.raises(ValueError):
        ke.geometry("noop_kernel")
    with pytest.raises(ValueError):
        ke.geometry("bf16_cvt_check_kernel<1>")


def test_an_fp16_kernel_name_the_runtime_leaves_mangled_is_still_read():
    """The fp16 MAX / MIN kernels carry _Float16 in their names, which an older C++ runtime's demangler refuses:
    ftar.last_kernel() demangles those itself, and the geometry comes out of the result."""
    import ftar
    raw = ("_ZN4ftar12_GLOBAL__N_117reduce_lds_kernelINS0_6MinMaxIDF16_Lb1EEELi2ELi4ELi4ELi2ELb1EEEvNS0_4SrcsIXT0_EEE"
           "Pvmii")
    symbol = ftar.kernel_symbol(ftar._demangle_f16(raw))
    assert symbol == "reduce_lds_kernel<MinMax<_Float16, true>, 2, 4, 4, 2, true>"
    assert ke.tiles(symbol) == (64, 4 * 4 * 64)
    assert ftar._demangle_f16("void f<int>()") == "void f<int>()"
    assert ftar._demangle_f16("_Zgarbage_DF16_") == "_Zgarbage_DF16_"


# ---- the footprint checker ---------------------------------------------------------------------------------
PAYLOAD = 5000


def test_pattern_depends_on_the_position():
    import torch
    p = ke.pattern(1 << 16, torch, "cpu").numpy()
    assert len(set(p[:256].tolist())) == 256                      # 131 is odd: every byte value in a run of 256
    assert not np.array_equal(p[:256], p[256:512])                # and the next run is not a copy of it
    assert not np.array_equal(p[:4096], p[4096:8192])


def test_arena_layout():
    a = ke.Arena(PAYLOAD, device="cpu")
    assert ke.GUARD == 64 << 10
    assert ke.GUARD <= a.origin < ke.GUARD + 16 and a.ptr() % 16 == 0
    assert a.total - a.origin - PAYLOAD >= ke.GUARD
    assert a.ptr(7) == a.buf.data_ptr() + a.origin + 7


def test_check_untouched_passes_on_an_intact_arena():
    a = ke.Arena(PAYLOAD, device="cpu")
    assert ke.check_untouched(a) is None
    assert ke.check_untouched(a, 100, 300) is None
    a.window(100, 300).fill_(0)                                    # a call may write its whole window
    assert ke.check_untouched(a, 100, 300) is None
    assert ke.check_untouched(a, windows=[(100, 200), (200, 300)]) is None
    a.restore(100, 300)
    assert ke.check_untouched(a) is None


def _flip(a, off):
    a.buf[a.origin + off] ^= 0x5A


@pytest.mark.parametrize("where", ["before lo", "after hi", "front guard's far end", "back guard's far end"])
def test_check_untouched_reports_one_changed_byte(where):
    a = ke.Arena(PAYLOAD, device="cpu")
    lo, hi = 1003, 3001
    a.window(lo, hi).fill_(0x11)
    off, said = {"before lo": (lo - 1, "lo - 1"), "after hi": (hi, "hi + 0"),
                 "front guard's far end": (-a.origin, f"lo - {lo + a.origin}"),
                 "back guard's far end": (a.total - a.origin - 1, f"hi + {a.total - a.origin - 1 - hi}")}[where]
    _flip(a, off)
    msg = ke.check_untouched(a, lo, hi)
    assert msg is not None and said in msg and f"payload offset {off})" in msg and "1 bytes differ" in msg
    _flip(a, off)
    assert ke.check_untouched(a, lo, hi) is None


def test_check_untouched_reports_a_byte_in_a_gap_between_segments():
    a = ke.Arena(PAYLOAD, device="cpu")
    wins = [(16, 116), (116 + 64, 1000), (1000 + 64, 1000 + 64)]      # 64-byte gaps; the last segment is empty
    for lo, hi in wins:
        a.window(lo, hi).fill_(0x22)
    assert ke.check_untouched(a, windows=wins) is None
    for off, said in ((116, "hi + 0 of window 0"), (116 + 40, "lo - 24 of window 1"), (1063, "lo - 1 of window 2")):
        _flip(a, off)
        msg = ke.check_untouched(a, windows=wins)
        assert msg is not None and said in msg, msg
        _flip(a, off)
    assert ke.check_untouched(a, windows=wins) is None


def test_check_untouched_holds_uploaded_sources():
    a = ke.Arena(PAYLOAD, device="cpu")
    x = np.arange(100, dtype=np.float32)
    a.upload(48, x)
    assert ke.check_untouched(a) is None
    assert np.array_equal(a.window(48, 448).numpy().view(np.float32), x)
    _flip(a, 48 + 399)
    assert "payload offset 447" in ke.check_untouched(a)


def test_fold_verify_on_the_cpu():
    """Fold's bookkeeping without a kernel: numpy plays the launch."""
    ins = ke.sources("i32", "sum", 3, 301)
    want = ins[0] + ins[1] + ins[2]
    f = ke.Fold(ins, want, shifts=[0, 1, 0], device="cpu")
    off, n = 3, 250
    for alias in (None, 0, 1):
        arena, lo = (f.dst, off * 4) if alias is None else (f.src, f.src_off(alias, off))
        srcs, dst = f.pointers(off, alias)
        assert dst == arena.ptr(lo) and srcs[1] % 16 == (srcs[0] + 4) % 16
        arena.window(lo, lo + n * 4).copy_(f.want[off * 4:(off + n) * 4])
        assert f.verify(off, n, alias) is None
        assert f.verify(0, 0) is None                                 # and verify put the arenas back
        arena.window(lo, lo + (n + 1) * 4).copy_(f.want[off * 4:(off + n + 1) * 4])   # one element too many
        assert "hi + 0" in f.verify(off, n, alias)
        arena.window(lo, lo + n * 4).copy_(f.want[(off + 1) * 4:(off + 1 + n) * 4])   # the wrong elements
        assert "payload" in f.verify(off, n, alias)
        assert f.verify(0, 0) is None


def test_inputs_are_finite_and_expectations_come_out_without_nan():
    for dt, op in (("f16", "sum"), ("bf16", "max"), ("f32", "min"), ("f64", "sum"), ("u8", "band")):
        ins = ke.sources(dt, op, 3, 1000)
        assert all(ke.no_nan(dt, x) for x in ins)
        assert ke.expected(dt, op, ins).size == 1000
    nan = np.array([0x7E00], np.uint16)
    assert not ke.no_nan("f16", nan) and not ke.no_nan("f32", np.array([np.inf], np.float32))
    ins = ke.sources("bf16", "sum", 3, 64)
    assert not np.array_equal(ke.hop_fold("bf16", ins), ke.hop_fold("bf16", ins, 0.25))


# ---- fp8 inputs and expectations ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ke.F8)
def test_fp8_inputs_and_expectations_come_from_f8_ref(dt):
    import f8_ref
    assert ke.STORAGE[dt] == np.uint8 and ke.esize(dt) == 1 and dt in ke.FLOATS
    ins = ke.sources(dt, "sum", 3, 1000)
    assert all(np.array_equal(a, b) for a, b in zip(ins, f8_ref.finite_sources(dt, 3, 1000)))
    assert len(ke.sources(dt, "sum", 1, 10)) == 1
    assert all(ke.no_nan(dt, x) for x in ins)
    assert np.array_equal(ke.expected(dt, "sum", ins), f8_ref.fold(dt, ins))
    assert np.array_equal(ke.expected(dt, "sum", ins, scale=0.25), f8_ref.fold(dt, ins, f8_ref.scale_of(0.25)))
    assert np.array_equal(ke.expected(dt, "sum", ins, hop=True), f8_ref.hop_fold(dt, ins))
    assert np.array_equal(ke.expected(dt, "sum", ins, hop=True, scale=0.25),
                          f8_ref.hop_fold(dt, ins, f8_ref.scale_of(0.25)))
    assert not np.array_equal(ke.expected(dt, "sum", ins, hop=True), ke.expected(dt, "sum", ins))
    four = ke.sources(dt, "sum", 4, 1000)
    assert np.array_equal(ke.expected(dt, "sum", four, shape=(2, 2)), f8_ref.nested(dt, four, (2, 2)))
    for op in ("max", "min"):
        assert np.array_equal(ke.expected(dt, op, ins), f8_ref.minmax(dt, op, ins))
    assert np.array_equal(ke.expected(dt, "sum", ins[:1]), ins[0])
    # what no_nan refuses: the format's NaN, and e5m2's inf
    assert not ke.no_nan(dt, np.array([0xFF], np.uint8))
    assert ke.no_nan("f8e4m3", np.array([0x7E], np.uint8)) and ke.no_nan("f8e5m2", np.array([0x7B], np.uint8))
    assert not ke.no_nan("f8e5m2", np.array([0x7C], np.uint8))


# ---- the staircase -----------------------------------------------------------------------------------------
def _ends(dt, wg_tile):
    ve = 16 // ke.esize(dt)
    return ve, sorted({ke.head_offset(ve, e.head) + e.n for e in ke.edge_counts(ve, wg_tile)})


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("wg_tile", [128, 512, 1024, 2048])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32", "f8e4m3", "f8e5m2"])
def test_staircase_steps_up_at_every_boundary(dt, wg_tile, scale):
    """The boundaries of edge_counts: the expectation's |value| never falls back under an earlier level, steps
    strictly up AT every boundary (staircase() asserts that itself), and -- the opposite property -- the word of [0, b) differs from
    the word of [0, b]: a checker fed one lane too many fails."""
    import amax_ref
    ve, bs = _ends(dt, wg_tile)
    assert 40 <= len(bs) <= 45
    ins, want = ke.staircase(dt, 3, bs, max(bs) + wg_tile * ve, scale=scale)
    assert len(ins) == 3 and want.size == max(bs) + wg_tile * ve and ke.no_nan(dt, want)
    keys = amax_ref.keys(dt, want).astype(np.int64)
    assert keys.min() > 0
    nz = np.stack([amax_ref.keys(dt, x) != 0 for x in ins])
    assert (nz.sum(axis=0) == 1).all() and (nz.argmax(axis=0) == np.arange(want.size) % 3).all()
    signs = np.ascontiguousarray(want).view(amax_ref.storage(dt)) != amax_ref.keys(dt, want)
    assert 0.3 < signs.mean() < 0.7, "the sign of the non-zero value is random"
    for b in bs:
        assert amax_ref.amax_bits(dt, want[:b]) != amax_ref.amax_bits(dt, want[:b + 1]), b
        assert b == 0 or keys[b:].min() > keys[:b].max()
    assert amax_ref.amax_bits(dt, want) > amax_ref.amax_bits(dt, want[:bs[-1]])      # larger values behind the last


def test_staircase_refuses_a_boundary_outside_the_sources_and_holds_for_a_hop_and_a_nested_fold():
    with pytest.raises(AssertionError):
        ke.staircase("bf16", 2, [10, 100], 100)
    for dt in ("f16", "f8e5m2"):
        _, bs = _ends(dt, 512)
        ke.staircase(dt, 8, bs, max(bs) + 64, scale=0.5, hop=True)
        ke.staircase(dt, 4, bs, max(bs) + 64, scale=1.0, shape=(2, 2))
        ke.staircase(dt, 1, bs, max(bs) + 64, scale=0.5)
    ke.staircase("f8e4m3", 64, [5, 70], 200)                 # finite at any k


def test_the_slot_sweeps_field_is_even_with_a_mantissa_and_one_step_widens_apart():
    import amax_ref
    for dt, e in ke.SWEEP_E.items():
        assert e % 2 == 0 and e + 1 < amax_ref.LAYOUT[dt][2]
        assert 0 < amax_ref.widen(dt, e) < amax_ref.widen(dt, e + 1) < 0x7F800000
        ins = ke.one_hot(dt, 3, np.full(100, e))
        want = ke.expected(dt, "sum", ins, scale=1.0)
        assert (amax_ref.keys(dt, want) == e).all()


# ---- Fold.verify with an amax word -------------------------------------------------------------------------
def test_fold_verify_with_a_word_on_the_cpu():
    """numpy plays the launch: a right word, a wrong word, and a fifth byte written beside it."""
    import amax_ref
    ins, want = ke.staircase("bf16", 2, [40, 253], 301, scale=1.0)
    f = ke.Fold(ins, want, device="cpu")
    off, n = 3, 250
    word = amax_ref.amax_bits("bf16", want[off:off + n])
    assert f.word_ptr() == f.am.ptr(ke.WORD_AT) and f.word_ptr() % 4 == 0 and f.am.payload_bytes == 64

    def play(w):
        f.dst.window(off * 2, (off + n) * 2).copy_(f.want[off * 2:(off + n) * 2])
        f.set_word(w)
    play(word)
    assert f.verify(off, n, word=word) is None
    assert ke.check_untouched(f.am) is None                       # and verify put the word's arena back
    play(word)
    assert f.verify(off, n) is None                               # without a word the word is not looked at
    play(amax_ref.amax_bits("bf16", want[off:off + n + 1]))       # one lane too many in the key
    assert "amax word" in f.verify(off, n, word=word)
    play(0)
    assert "amax word" in f.verify(off, n, word=word)
    play(word)
    f.am.buf[f.am.origin + ke.WORD_AT + 4] ^= 0x5A                # a fifth byte
    assert "amax word's arena" in f.verify(off, n, word=word)
    play(word)
    f.am.buf[f.am.origin + ke.WORD_AT - 1] ^= 0x5A
    assert "amax word's arena" in f.verify(off, n, word=word)
    play(0x7FC00000)
    assert f.verify(off, n, word=amax_ref.NAN) is None
    assert f.verify(0, 0) is None


def test_reduce_ex_knows_the_amax_hook():
    import ftar
    assert hasattr(ftar.bench_lib(), "ftar_debug_reduce_amax_ex")
