"""The amax finish (AmaxFin, csrc/reduce_impl.h) at the edges of every fold family, on the helpers of
tests/kernel_edges.py and the cases of tests/test_gpu_kernel_edges.py.

  a. footprint and word at every edge count: each launch checks the payload bit for bit, the guards around the
     destination and the sources, the amax word against amax_ref's reading of exactly the expected payload, and the
     word's own 4-byte footprint -- once on ordinary finite inputs, once on staircase inputs whose values step up
     right behind every launch's range (a lane too many in the key gives a larger word);
  b. every slot of two workgroup tiles, a partial tile, the head and the tail wins by ONE encoding step over a
     field of equal |encoding| with a non-zero mantissa (a key that loses a low bit, a lane or a wave loses it);
  c. the word only grows: a launch maxes into whatever the word holds, as the engine's pieces do;
  d. the element-wise kernels carry the key over their grid-stride loop.

Expectations come from the references the suite pins (kernel_edges.expected, amax_ref.amax_bits / widen)."""
import numpy as np
import pytest

import amax_ref
import kernel_edges as ke
import test_gpu_kernel_edges as edges

pytestmark = pytest.mark.gpu

THIRD = edges.THIRD
INF32 = 0x7F800000


class AmaxLaunch:
    """(source pointers, destination pointer, count) -> one amax launch that maxes into the device word at .word.
    via "api": ftar.reduce(..., amax=), which zeroes the word first; via "hook": ftar_debug_reduce_amax_ex, which
    leaves the word to the caller (and reaches round_each and lds = false)."""

    def __init__(self, dt, via, scale, shape=None, **kw):
        self.dt, self.via, self.scale, self.shape, self.kw, self.word = dt, via, scale, shape, kw, None

    def __call__(self, srcs, dst, n):
        if self.via == "api":
            import ftar
            ftar.reduce(srcs, dst, n, self.dt, "sum", shape=list(self.shape) if self.shape else None,
                        scale=self.scale, amax=self.word)
        else:
            ke.reduce_ex(srcs, dst, n, self.dt, "sum", shape=self.shape, scale=self.scale, amax=self.word, **self.kw)


def probe(launch, dt, k, shifts=None):
    """edges.probe with a scratch word."""
    import torch
    scratch = torch.zeros(4, dtype=torch.int32, device="cuda")
    launch.word = scratch.data_ptr()
    symbol = edges.probe(launch, dt, k, shifts)
    launch.word = None
    return symbol


def amax_id(want_id, hop=False):
    """The plain kernel's id (tests/test_gpu_kernel_edges.py, tests/test_gpu_avg.py) as its amax kernel's; a hop
    fold under this finish is the Pre trait."""
    w = (want_id,) if isinstance(want_id, str) else tuple(want_id)
    if hop:
        w = (w[0] + "Pre",) + w[1:]
    w = tuple(x.replace("_kernel<", "_amax_kernel<") for x in w)
    exact = isinstance(want_id, str)

    def check(symbol):
        if exact:
            assert symbol == w[0]
        else:
            assert symbol.startswith(w[0]) and all(x in symbol for x in w[1:]), (symbol, w)
    return check


# ---- a. footprint and word at every edge count ------------------------------------------------------------
def _amax_cases():
    out = {name: dict(c) for name, c in edges.FAMILY_CASES.items() if c["dt"] in amax_ref.DTYPES}
    # 4-byte k = 2 under this finish runs 4 x 4 workgroups, a shape no other finish uses (launch_k: kWide)
    assert out["lds"]["want_id"] == "reduce_lds_kernel<F32Sum, 2, 1, 2, 2, true>"
    out["lds"]["want_id"] = "reduce_lds_kernel<F32Sum, 2, 4, 4, 2, true>"
    # f64 has no amax: the register tree kernel by a 2-byte runtime-coded shape, as tests/test_gpu_amax.py does
    out["tree_reg_bf16_2x3"] = dict(dt="bf16", k=6, shape=(2, 3), via="api",
                                    want_id=("reduce_tree_kernel<H16SumT<Bf16Fmt<", ", 6, 2, RuntimeShape>"))
    out["copy_f16_k1"] = dict(dt="f16", k=1, via="api",
                              want_id="reduce_vec_kernel<H16SumT<HalfFmt>, 0, 2, true, true, 512>")
    out["f8_lds_k8"] = dict(dt="f8e4m3", k=8, via="api", want_id=("reduce_lds_kernel<F8SumT<F8Fmt<false>", ", 8, "))
    out["f8_vec_k9"] = dict(dt="f8e5m2", k=9, via="api",
                            want_id=("reduce_vec_kernel<F8SumT<F8Fmt<true>", ", 0, 2, true, true, 512>"))
    out["f8_tree_lds_2x2"] = dict(dt="f8e4m3", k=4, shape=(2, 2), via="api",
                                  want_id=("reduce_tree_lds_kernel<F8SumT<F8Fmt<false>", "StaticShape<2, 2>"))
    return out


AMAX_CASES = _amax_cases()
STALE = 0xFFFFFFFF      # what the word holds before a call that zeroes it itself: above every result


@pytest.mark.parametrize("inputs", ["finite", "staircase"])
@pytest.mark.parametrize("family", sorted(AMAX_CASES))
def test_footprint_and_word_at_the_edges_of_every_family(family, inputs):
    """finite: the ordinary inputs at scale 1/3, through ftar.reduce(amax=) where that reaches the kernel.
    staircase: boundaries at every launch's own end, sources one workgroup tile longer than the last of them, at
    scale 1.0 or 0.5 (exact on these inputs), through the hook onto a word the test zeroes."""
    import ftar
    c = AMAX_CASES[family]
    dt, k, shape, shifts, hop = c["dt"], c["k"], c.get("shape"), c.get("shifts"), c.get("hop", False)
    stair = inputs == "staircase"
    scale = (1.0, 0.5)[sorted(AMAX_CASES).index(family) % 2] if stair else THIRD
    via = "api" if c["via"] == "api" and not stair else "hook"
    launch = AmaxLaunch(dt, via, scale, shape, **c.get("kw", {}))
    symbol = probe(launch, dt, k, shifts)
    amax_id(c["want_id"], hop)(symbol)
    ve = 16 // ke.esize(dt)
    g, edge_list = edges.edges_of(symbol, ve)
    ends = [ke.head_offset(ve, e.head) + e.n for e in edge_list]
    tile = g.wg_tile * (1 if g.family in edges.ELEMENTWISE else ve)
    fold = edges.fold_for(dt, "sum", k, max(ends) + tile + ve, shape, scale, hop, shifts, stair=ends if stair else None)
    launch.word = fold.word_ptr()
    ids = set()
    for e in edge_list:
        off = ke.head_offset(ve, e.head)
        srcs, dst = fold.pointers(off)
        fold.set_word(STALE if via == "api" else 0)
        launch(srcs, dst, e.n)
        word = amax_ref.amax_bits(dt, fold.want_host[off:off + e.n])
        assert word != amax_ref.NAN and (word > 0 or e.n == 0 or not stair)
        bad = fold.verify(off, e.n, word=word)
        assert bad is None, (e, ftar.last_kernel(), bad)
        if e.nvec >= 1:
            ids.add(ftar.last_kernel())
    assert ids == {symbol}, "one kernel for every count with vectors"


# ---- b. every slot, won by one encoding step --------------------------------------------------------------
SWEEPS = {
    "lds_f32_k2": dict(dt="f32", k=2, family="reduce_lds_kernel"),
    "lds_bf16_k2": dict(dt="bf16", k=2, family="reduce_lds_kernel"),
    "lds_f16_k8": dict(dt="f16", k=8, family="reduce_lds_kernel"),
    "lds_e4m3_k8": dict(dt="f8e4m3", k=8, family="reduce_lds_kernel"),
    "vec_f32_k17": dict(dt="f32", k=17, family="reduce_vec_kernel"),
    "vec_e5m2_k9": dict(dt="f8e5m2", k=9, family="reduce_vec_kernel"),
    "copy_bf16_k1": dict(dt="bf16", k=1, family="reduce_vec_kernel"),
    "tree_lds_f32_2x2": dict(dt="f32", k=4, shape=(2, 2), family="reduce_tree_lds_kernel"),
    "tree_reg_bf16_2x3": dict(dt="bf16", k=6, shape=(2, 3), family="reduce_tree_kernel"),
    "elem_f16_k3": dict(dt="f16", k=3, shifts=[0, 0, 1], family="reduce_elem_kernel"),
    "tree_elem_f32_2x2": dict(dt="f32", k=4, shape=(2, 2), shifts=[0, 1, 0, 0], family="reduce_tree_elem_kernel"),
    "hop_pre_f16_k3": dict(dt="f16", k=3, kw=dict(round_each=True), hop=True, family="reduce_lds_kernel",
                           named="H16SumHopPreT<HalfFmt>"),
    "hop_pre_e5m2_k8": dict(dt="f8e5m2", k=8, kw=dict(round_each=True), hop=True, family="reduce_lds_kernel",
                            named="F8SumHopPreT<F8Fmt<true>"),
}


MANTISSA = {"f8e4m3": 3, "f8e5m2": 2, "bf16": 7, "f16": 10, "f32": 23}


class Winner:
    """A field in which every lane's result has |encoding| E (kernel_edges.one_hot: one non-zero source per lane,
    random signs), and one-element device writes that raise one lane's to E + 1 and put it back."""

    def __init__(self, dt, k, length, shape=None, hop=False, shifts=None):
        import torch
        self.dt, self.k = dt, k
        self.E = ke.SWEEP_E[dt]
        u = amax_ref.storage(dt)
        self.ins = ke.one_hot(dt, k, np.full(length, self.E))
        want = ke.expected(dt, "sum", self.ins, shape=shape, scale=1.0, hop=hop)
        assert (amax_ref.keys(dt, want) == self.E).all(), "every lane of the expectation has |encoding| E"
        assert self.E % 2 == 0 and self.E & ((1 << MANTISSA[dt]) - 1), "E + 1 sets the lowest bit; E's mantissa is not 0"
        self.fold = ke.Fold(self.ins, want, shifts=shifts)
        esz = self.fold.esz
        sign = 1 << (8 * esz - 1)
        dev = self.fold.want.device
        self.bytes = {s: torch.from_numpy(np.array([s | (self.E + 1)], u).view(np.uint8).copy()).to(dev)
                      for s in (0, sign)}
        self.sign = sign
        self.word_e, self.word_e1 = amax_ref.widen(dt, self.E), amax_ref.widen(dt, self.E + 1)
        assert self.word_e1 > self.word_e > 0

    def _where(self, lane):
        j = lane % self.k
        f = self.fold
        return f.src.origin + f.src_off(j, lane), self.bytes[int(self.ins[j][lane]) & self.sign]

    def put(self, lane):
        a, b = self._where(lane)
        self.fold.src.buf[a:a + self.fold.esz] = b

    def take(self, lane):
        a, _ = self._where(lane)
        self.fold.src.buf[a:a + self.fold.esz] = self.fold.src.want[a:a + self.fold.esz]

    def verify(self, off, n, lane):
        """Fold.verify with the winner (lane, or None) in the expectation; the sources are as uploaded again."""
        f = self.fold
        if lane is None:
            return f.verify(off, n)
        lo, hi = lane * f.esz, (lane + 1) * f.esz
        keep = f.want[lo:hi].clone()
        f.want[lo:hi] = self._where(lane)[1]
        bad = f.verify(off, n)
        f.want[lo:hi] = keep
        return bad

    def sweep(self, launch, off, n, lanes):
        """One launch per lane of `lanes` (fold lanes, inside [off, off + n)) with the winner there, each into its
        own word, then one launch without a winner; the payload and the guards on the first, the last and every
        257th launch.  Returns the words."""
        import ftar
        import torch
        words = torch.zeros(len(lanes) + 1, dtype=torch.int32, device="cuda")
        srcs, dst = self.fold.pointers(off)
        for i, lane in enumerate(lanes + [None]):
            assert lane is None or off <= lane < off + n
            launch.word = words.data_ptr() + 4 * i
            if lane is not None:
                self.put(lane)
            launch(srcs, dst, n)
            if lane is not None:
                self.take(lane)
            if i % 257 == 0 or i >= len(lanes) - 1:
                bad = self.verify(off, n, lane)
                assert bad is None, (lane, ftar.last_kernel(), bad)
        torch.cuda.synchronize()
        return words.cpu().numpy().view(np.uint32)

    def check(self, words, lanes, off, what):
        wrong = np.flatnonzero(words[:-1] != np.uint32(self.word_e1))
        assert wrong.size == 0, (what, f"{wrong.size} of {len(lanes)} winners lost; the first at element "
                                 f"{lanes[wrong[0]] - off} of the launch: word 0x{int(words[wrong[0]]):08x}, want "
                                 f"0x{self.word_e1:08x}")
        assert int(words[-1]) == self.word_e, (what, "no winner", hex(int(words[-1])), hex(self.word_e))


@pytest.mark.parametrize("case", sorted(SWEEPS))
def test_every_slot_wins_by_one_encoding_step(case):
    """n = a head, two workgroup tiles, a partial tile of 65 vectors and a tail.  The winner visits every vector
    at in-vector element v % VE (every U slot, wave and byte lane), every element of the first and the last vector
    of tile 0, and every head and tail element; the element-wise kernels: every element of two 256-element tiles
    and a partial one."""
    import ftar
    c = SWEEPS[case]
    dt, k, shape, shifts = c["dt"], c["k"], c.get("shape"), c.get("shifts")
    launch = AmaxLaunch(dt, "hook", 1.0, shape, **c.get("kw", {}))
    symbol = probe(launch, dt, k, shifts)
    g = ke.geometry(symbol)
    assert g.family == c["family"] and "_amax_kernel<" in symbol and c.get("named", "") in symbol, symbol
    ve = 16 // ke.esize(dt)
    if g.family in edges.ELEMENTWISE:
        off, n = 0, 2 * g.wg_tile + 65
        at = list(range(n))
    else:
        T, h, t = g.wg_tile, ve - 1, ve - 1
        nvec = 2 * T + 65
        off, n = ke.head_offset(ve, h), h + nvec * ve + t
        at = [h + v * ve + v % ve for v in range(nvec)]
        at += [h + v * ve + e for v in (0, T - 1) for e in range(ve)]
        at += list(range(h)) + list(range(n - t, n))
        at = list(dict.fromkeys(at))
        assert {(a - h) // ve % T // 64 for a in at if h <= a < h + nvec * ve} == set(range(T // 64)), "every wave tile"
    w = Winner(dt, k, off + n + ve, shape, c.get("hop", False), shifts)
    lanes = [off + a for a in at]
    words = w.sweep(launch, off, n, lanes)
    assert ftar.last_kernel() == symbol
    w.check(words, lanes, off, symbol)


# ---- c. the word only grows -------------------------------------------------------------------------------
GROW = {
    "lds": dict(dt="bf16", k=2, family="reduce_lds_kernel"),
    "vec": dict(dt="f32", k=17, family="reduce_vec_kernel"),
    "elem": dict(dt="f8e4m3", k=2, shifts=[0, 1], family="reduce_elem_kernel"),
}
GROW_N = 4099           # a full tile, a partial one and a tail


@pytest.mark.parametrize("case", sorted(GROW))
def test_the_word_only_grows(case):
    """The engine zeroes the word once and lets one launch per piece max into it: a launch leaves the unsigned max
    of what the word held and its own amax -- at, one ulp under and over its own value, +inf, a NaN pattern."""
    import ftar
    c = GROW[case]
    dt, k, shifts = c["dt"], c["k"], c.get("shifts")
    launch = AmaxLaunch(dt, "hook", 1.0)
    fold = edges.fold_for(dt, "sum", k, GROW_N + 16, scale=1.0, shifts=shifts)
    launch.word = fold.word_ptr()
    srcs, dst = fold.pointers(0)
    m = amax_ref.amax_bits(dt, fold.want_host[:GROW_N])
    assert m != amax_ref.NAN and 1 < m < INF32
    for before in (0, m - 1, m, m + 1, INF32, 0x7FC00001):
        fold.set_word(before)
        launch(srcs, dst, GROW_N)
        bad = fold.verify(0, GROW_N, word=max(before, m))
        assert bad is None, (hex(before), hex(m), ftar.last_kernel(), bad)
    assert ke.geometry(ftar.last_kernel()).family == c["family"] and "_amax_kernel<" in ftar.last_kernel()
    # two launches on disjoint halves into one word, in both orders: staircase inputs that step up at the second
    # half, so one order grows the word and the other keeps it
    half = 2048
    fold = ke.Fold(*ke.staircase(dt, k, [half], GROW_N + 16, scale=1.0), shifts=shifts)
    launch.word = fold.word_ptr()
    parts = [(0, half), (half, GROW_N - half)]
    ms = [amax_ref.amax_bits(dt, fold.want_host[o:o + n]) for o, n in parts]
    m = amax_ref.amax_bits(dt, fold.want_host[:GROW_N])
    assert ms[0] < ms[1] == m
    for order in ((0, 1), (1, 0)):
        fold.set_word(0)
        o, n = parts[order[0]]
        launch(*fold.pointers(o), n)
        bad = fold.verify(o, n)            # the word is left as the first launch made it
        assert bad is None, (order, bad)
        o, n = parts[order[1]]
        launch(*fold.pointers(o), n)
        bad = fold.verify(o, n, word=m)
        assert bad is None, (order, [hex(x) for x in ms], bad)


# ---- d. the second grid-stride pass -----------------------------------------------------------------------
@pytest.mark.parametrize("dt,k,shape", [("f32", 3, None), ("bf16", 2, None), ("f32", 4, (2, 2))],
                         ids=["f32_k3", "bf16_k2", "tree_elem_f32_2x2"])
def test_elementwise_amax_carries_the_key_over_the_grid_stride_loop(dt, k, shape):
    """STRIDE_N elements on the 8192-workgroup grid: workgroup 0 runs a whole second pass, workgroup 1 a partial
    one.  The one-step winner sits in a lane of the first pass that has a second one (workgroups 0 and 1), in the
    whole second pass, in the partial one, and in the last element."""
    import ftar
    n, grid = edges.STRIDE_N, 8192 * 256
    shifts = [0] * (k - 1) + [1]
    launch = AmaxLaunch(dt, "hook", 1.0, shape)
    w = Winner(dt, k, n + 16, shape, False, shifts)
    lanes = [100, 256 + 1, grid + 100, grid + 256 + 1, n - 1]
    words = w.sweep(launch, 0, n, lanes)
    symbol = ftar.last_kernel()
    assert symbol.startswith("reduce_tree_elem_amax_kernel<" if shape else "reduce_elem_amax_kernel<"), symbol
    w.check(words, lanes, 0, symbol)
