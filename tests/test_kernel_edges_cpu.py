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
]


@pytest.mark.parametrize("symbol,wg_tile,shape", IDS)
def test_geometry_from_a_kernel_id(symbol, wg_tile, shape):
    assert ke.tiles(symbol) == (64, wg_tile)
    g = ke.geometry(symbol)
    assert g.lds_shape == shape
    assert g.family == symbol.split("<")[0].replace("_scaled", "")


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
