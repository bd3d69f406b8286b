"""Helpers of the kernel-edge tests (tests/test_gpu_kernel_edges.py; self-tested on the CPU by
tests/test_kernel_edges_cpu.py): guarded arenas whose every byte outside a call's destination is checked after
the call, the tile geometry of a launched kernel read from its name, the element counts that sit on that
geometry's edges, inputs and expectations from the references the suite already pins (fp8: tests/f8_ref.py; the
amax word: tests/amax_ref.py), staircase inputs whose result steps up at chosen lanes, and ctypes wrappers of the
hooks in libftar_bench.so (ftar_debug_reduce_ex, ftar_debug_reduce_amax_ex, ftar_debug_gather).

No GPU import at module level: torch, ftar and the oracle are loaded by the functions that need them."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

GUARD = 64 << 10     # bytes on each side of an arena's payload: above the largest workgroup tile of any fold or
#                      copy kernel (18 KiB: LDS 4-byte k = 3..4; 16 KiB: the runtime-k register kernel)
WAVE_TILE = 64       # vectors one wave instruction moves (64 lanes x 16 B)
MAX_K = 64           # FTAR_MAX_K


# ---- arena ------------------------------------------------------------------------------------------------
def pattern(nbytes, torch, device):
    """The filler: byte i = f(i), so bytes copied from the wrong place show as well as bytes that changed."""
    i = torch.arange(nbytes, dtype=torch.int64, device=device)
    return ((i * 131 + (i >> 8) * 29 + 7) & 0xFF).to(torch.uint8)


class Arena:
    """One allocation [guard G][slack < 16 B][payload][guard G].  Offsets are bytes from the payload's start, which
    is 16-byte aligned.  `want` is what every byte must hold while no call is allowed to write it: the pattern,
    or what upload() put there (sources)."""

    def __init__(self, payload_bytes, device="cuda"):
        import torch
        self.torch = torch
        self.payload_bytes = int(payload_bytes)
        total = GUARD + 16 + self.payload_bytes + GUARD
        self.want = pattern(total, torch, device)
        self.buf = self.want.clone()
        self.origin = GUARD + (-(self.buf.data_ptr() + GUARD)) % 16
        self.total = total

    def ptr(self, off=0):
        return self.buf.data_ptr() + self.origin + off

    def upload(self, off, array):
        """Place a numpy array's bytes at payload offset `off`; they become what check_untouched expects."""
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert 0 <= off and off + raw.size <= self.payload_bytes
        t = self.torch.from_numpy(raw.copy()).to(self.buf.device)
        a = self.origin + off
        self.buf[a:a + raw.size] = t
        self.want[a:a + raw.size] = t

    def window(self, lo, hi):
        return self.buf[self.origin + lo:self.origin + hi]

    def restore(self, lo, hi):
        a, b = self.origin + lo, self.origin + hi
        self.buf[a:b] = self.want[a:b]


def check_untouched(arena, lo=0, hi=0, windows=None):
    """None when every byte of the arena outside [lo, hi) -- or outside every (lo, hi) of `windows`, ascending and
    disjoint -- still holds what it must; else a line naming the first differing byte relative to the nearest
    window edge ("lo - 3": three bytes in front of a window; "hi + 0": the first byte behind one)."""
    torch = arena.torch
    wins = [(lo, hi)] if windows is None else list(windows)
    edges = [-arena.origin]
    for a, b in wins:
        assert edges[-1] <= a <= b, "windows ascend and do not overlap"
        edges += [a, b]
    edges.append(arena.total - arena.origin)
    for g in range(0, len(edges), 2):       # the gaps: in front of the first window, between, behind the last
        a, b = edges[g] + arena.origin, edges[g + 1] + arena.origin
        if a == b or torch.equal(arena.buf[a:b], arena.want[a:b]):
            continue
        bad = int(torch.nonzero(arena.buf[a:b] != arena.want[a:b])[0]) + a
        off = bad - arena.origin
        behind = g // 2 - 1                 # the window this gap follows (-1: none)
        d_hi = off - wins[behind][1] if behind >= 0 else None
        d_lo = wins[behind + 1][0] - off if behind + 1 < len(wins) else None
        if d_lo is not None and (d_hi is None or d_lo <= d_hi):
            where = f"lo - {d_lo} of window {behind + 1} {wins[behind + 1]}"
        else:
            where = f"hi + {d_hi} of window {behind} {wins[behind]}"
        n_bad = int((arena.buf[a:b] != arena.want[a:b]).sum())
        return (f"stray write at {where} (payload offset {off}): holds 0x{int(arena.buf[bad]):02x}, must hold "
                f"0x{int(arena.want[bad]):02x}; {n_bad} bytes differ in that gap")
    return None


# ---- geometry from the kernel's name ----------------------------------------------------------------------
def template_args(symbol):
    """("reduce_lds_kernel", ["F32Sum", "2", "1", "2", "2", "true"]) of a kernel_symbol() id; nested <> kept whole."""
    symbol = symbol.strip()
    if "<" not in symbol:
        return symbol, []
    name, rest = symbol.split("<", 1)
    assert rest.endswith(">"), symbol
    args, depth, cur = [], 0, ""
    for ch in rest[:-1]:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    args.append(cur.strip())
    return name.strip(), args


Geometry = namedtuple("Geometry", "family wave_tile wg_tile lds_shape")


def geometry(symbol):
    """The tile geometry of a fold or copy kernel from its template id (csrc/reduce_impl.h; NAME_scaled_kernel and
    NAME_amax_kernel are read as NAME_kernel, their family): wg_tile = the 16-byte vectors one workgroup covers
    per pass -- W x U x 64 for the LDS-staged families, U x BS for reduce_vec*, U x 256 for reduce_tree*, 2 x 256
    for gather_kernel; the element-wise kernels cover 256 ELEMENTS per workgroup and pass.  lds_shape = (U, W) of
    an LDS-staged kernel, else None."""
    name, a = template_args(symbol)
    family = name.replace("_scaled_kernel", "_kernel").replace("_amax_kernel", "_kernel")
    if family == "reduce_lds_kernel":           # <Tr, K, U, W, AUX, PROG>
        u, w = int(a[2]), int(a[3])
        return Geometry(family, WAVE_TILE, w * u * WAVE_TILE, (u, w))
    if family == "reduce_tree_lds_kernel":      # <Tr, K, U, W, Sh>
        u, w = int(a[2]), int(a[3])
        return Geometry(family, WAVE_TILE, w * u * WAVE_TILE, (u, w))
    if family == "reduce_vec_kernel":           # <Tr, K, U, NTL, NTS, BS>
        return Geometry(family, WAVE_TILE, int(a[2]) * int(a[5]), None)
    if family == "reduce_tree_kernel":          # <Tr, K, U, Sh>
        return Geometry(family, WAVE_TILE, int(a[2]) * 256, None)
    if family == "gather_kernel":               # <NT, REL>
        return Geometry(family, WAVE_TILE, 2 * 256, None)
    if family in ("reduce_elem_kernel", "reduce_tree_elem_kernel"):
        return Geometry(family, WAVE_TILE, 256, None)
    raise ValueError(f"not a fold or copy kernel: {symbol!r}")


def tiles(symbol):
    """(wave_tile, wg_tile) of geometry()."""
    g = geometry(symbol)
    return g.wave_tile, g.wg_tile


# ---- counts on the edges ----------------------------------------------------------------------------------
Edge = namedtuple("Edge", "n head nvec tail")


def edge_nvecs(wg_tile):
    out = []
    for v in (0, 1, 63, 64, 65, wg_tile - 64, wg_tile - 1, wg_tile, wg_tile + 1, wg_tile + 64, 3 * wg_tile - 1):
        if v >= 0 and v not in out:
            out.append(v)
    return out


def edge_heads_tails(ve):
    out = []
    for h, t in ((0, 0), (0, ve - 1), (ve - 1, 0), (1, 1), (ve - 1, ve - 1)):
        if h < ve and t < ve and (h, t) not in out:
            out.append((h, t))
    return out


def edge_counts(ve, wg_tile):
    """Element counts n = head + nvec * ve + tail on every edge of a kernel whose workgroup covers wg_tile vectors
    of ve elements: Edge(n, head, nvec, tail).  head is produced by head_offset(ve, head)."""
    return [Edge(h + v * ve + t, h, v, t) for v in edge_nvecs(wg_tile) for h, t in edge_heads_tails(ve)]


def head_offset(ve, head):
    """The element offset from a 16-byte boundary at which dst and every source sit to give `head` head elements."""
    return (ve - head) % ve


# ---- inputs and expectations ------------------------------------------------------------------------------
STORAGE = {"u8": np.uint8, "i8": np.int8, "u16": np.uint16, "i16": np.int16, "i32": np.int32, "i64": np.int64,
           "f32": np.float32, "f64": np.float64, "bool": np.uint8, "bf16": np.uint16, "f16": np.uint16,
           "f8e4m3": np.uint8, "f8e5m2": np.uint8}
F8 = ("f8e4m3", "f8e5m2")
FLOATS = ("f16", "bf16", "f32", "f64") + F8


def esize(dt):
    return np.dtype(STORAGE[dt]).itemsize


def _f16_bits(f32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(f32)).to(torch.float16).view(torch.int16).numpy().view(np.uint16)


def sources(dt, op, k, n, seed=1):
    """k sources of n elements: finite, no NaN, |x| < 1 for the floats (a 64-way fp16 sum stays finite); BAND gets
    a shared mask ORed in; MAX / MIN of floats get lanes of +-0 facing each other and of subnormals.  fp8:
    f8_ref.finite_sources (|x| < 2, the zero, subnormal and tie lanes in every op), k <= 17."""
    if dt in F8:
        import f8_ref
        return [np.ascontiguousarray(x).copy() for x in f8_ref.finite_sources(dt, max(k, 2), n, seed)[:k]]
    import f16_minmax_ref as ref
    import ftar_inputs as fi
    base = {"f16": "f32"}.get(dt, dt)
    xs = [fi.fill(base, 9000 + 7 * seed + k, j, n) for j in range(k)]
    if dt == "f16":
        xs = [_f16_bits(x) for x in xs]
    if op == "band":
        mask = fi.fill(base, 9001 + 7 * seed + k, MAX_K, n)
        xs = [np.bitwise_or(x, mask) for x in xs]
    if op in ("max", "min") and dt in FLOATS:
        u = ref.FLOATS[dt][0]
        sign = u(1 << (ref.FLOATS[dt][1] - 1))
        xs = [np.ascontiguousarray(x).view(u).copy() for x in xs]
        for j in range(k):
            xs[j][3::41] = sign if j % 2 == 0 else 0      # -0 first, +0 and -0 facing each other
            xs[j][4::41] = 0 if j % 2 == 0 else sign      # +0 first
            xs[j][5::43] = u(1 + j)                       # positive subnormals 1 .. k ulp
            xs[j][6::43] = sign | u(1 + j)                # negative subnormals
        xs[k - 1][7::37] = u(1)                           # the smallest subnormal among ordinary values
    return [np.ascontiguousarray(x) for x in xs]


def as_bytes(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def no_nan(dt, x):
    """The CPU-side assertion that an input or expectation holds no NaN (and, being finite inputs, no inf)."""
    if dt not in FLOATS:
        return True
    if dt in F8:    # e4m3: 0x7f is its NaN; e5m2: 0x7c inf, above it NaN
        return not bool(((np.ascontiguousarray(x).view(np.uint8) & 0x7F) >= (0x7F if dt == "f8e4m3" else 0x7C)).any())
    import f16_minmax_ref as ref
    u, _, emask, _ = ref.FLOATS[dt]
    b = np.ascontiguousarray(x).view(u)
    return not bool(((b & u(emask)) == u(emask)).any())


def nested_oracle(dt, ins, shape):
    """tests/test_gpu_reduce.py nested_oracle: every node one oracle reduce."""
    import ftar_inputs as fi
    import oracle_lib
    vals = list(ins)
    for w in shape:
        vals = [oracle_lib.reduce(fi.BY_NAME[dt], 0, vals[i:i + w]) if w > 1 else vals[i]
                for i in range(0, len(vals), w)]
    return vals[0]


def hop_fold(dt, ins, scale=None):
    """The one-round ring folds (round_each, k > 2) written out in torch.  Plain: every add rounds to the format.
    Scaled: the accumulator is rounded before each add and the last sum times r (fp32) is rounded once."""
    import torch

    import avg_ref
    fmt = avg_ref._fmt(dt)[0]
    t = [avg_ref._t(dt, x) for x in ins]
    if scale is None:
        acc = t[0]
        for x in t[1:]:
            acc = (acc.float() + x.float()).to(fmt)
        return avg_ref._bits(dt, acc)
    acc = t[0].float()
    for x in t[1:]:
        acc = acc.to(fmt).float() + x.float()
    r = torch.tensor(np.float32(scale), dtype=torch.float32)
    return avg_ref._bits(dt, (acc * r).to(fmt))


def expected(dt, op, ins, shape=None, scale=None, hop=False):
    """The one bit pattern a fold of `ins` must give, from the reference that pins that fold."""
    import avg_ref
    import f16_minmax_ref as ref
    import ftar_inputs as fi
    import oracle_lib
    k = len(ins)
    if dt in F8:
        import f8_ref
        r = None if scale is None else f8_ref.scale_of(scale)
        if op in ("max", "min"):
            want = f8_ref.minmax(dt, op, ins)
        elif hop and k > 2:
            want = f8_ref.hop_fold(dt, ins, r)
        elif shape and k > 1:
            want = f8_ref.nested(dt, ins, shape, r)
        elif k == 1 and r is None:
            want = ins[0]
        else:
            want = f8_ref.fold(dt, ins, r)
    elif op in ("max", "min"):
        want = ref.minmax(dt, op, [np.ascontiguousarray(x).view(ref.storage(dt)) for x in ins])
    elif hop and k > 2:
        want = hop_fold(dt, ins, scale)
    elif scale is not None:
        r = avg_ref.scale_of(dt, scale)
        want = avg_ref.nested(dt, ins, shape, r) if shape and k > 1 else avg_ref.root_fold(dt, ins, r)
    elif k == 1:
        want = ins[0]
    elif dt in ("bf16", "f16") and op == "sum":
        one = avg_ref.scale_of(dt, 1.0)     # nested(): the root times 1.0f, an exact multiply
        want = avg_ref.nested(dt, ins, shape, one) if shape else avg_ref.sum_fold(dt, ins)
    elif shape and dt in FLOATS:
        want = nested_oracle(dt, ins, shape)
    else:
        want = oracle_lib.reduce(fi.BY_NAME[dt], {"sum": 0, "band": 1}[op], ins)
    assert all(no_nan(dt, x) for x in ins) and no_nan(dt, want), "inputs and expectation are finite"
    return np.ascontiguousarray(want)


# ---- inputs whose result's |value| is known lane by lane --------------------------------------------------
# (first |encoding|, step) of staircase(): a normal number small enough that every level of ~50 boundaries stays
# finite, halves exactly (scale 0.5) and keeps one encoding step between neighbouring levels
STAIR = {"f8e4m3": (0x10, 1), "f8e5m2": (0x08, 1), "bf16": (0x3000, 8), "f16": (0x3000, 8), "f32": (0x3F000000, 4096)}
# the slot sweeps' |encoding| E of every lane: even (so E + 1 differs from it in the lowest key bit alone) with a
# non-zero mantissa
SWEEP_E = {"f8e4m3": 0x34, "f8e5m2": 0x36, "bf16": 0x3F94, "f16": 0x3554, "f32": 0x3F955554}


def one_hot(dt, k, enc, seed=1):
    """k sources in which lane i has exactly one non-zero element, in source i % k: |encoding| enc[i] under a random
    sign; the other sources alternate +0 and -0 there.  Any SUM fold of them (flat, hop, nested; times 1.0 or, while
    the halves stay normal, 0.5) is exact: the result's |value| in lane i is that of enc[i] (times the scale)."""
    import amax_ref
    u, _, _ = amax_ref.LAYOUT[dt]
    enc = np.asarray(enc)
    n = enc.size
    sign = u(1) << u(8 * np.dtype(u).itemsize - 1)
    rng = np.random.default_rng([seed, 77, k, n])
    i = np.arange(n)
    val = enc.astype(u) | np.where(rng.integers(0, 2, n) == 1, sign, u(0)).astype(u)
    xs = []
    for j in range(k):
        zero = np.where((i + j) % 2 == 1, sign, u(0)).astype(u)
        xs.append(np.ascontiguousarray(np.where(i % k == j, val, zero).astype(u)))
    return xs


def staircase(dt, k, boundaries, length, scale=None, shape=None, hop=False, seed=1):
    """(sources, expectation) of one_hot() inputs whose lane i holds |encoding| first + step * level(i) +
    rand(step), level(i) = how many of `boundaries` are <= i: the result's |value| never falls back under an
    earlier level and steps strictly up AT every boundary, so a fold of [off, b) that also takes lane b (or any
    lane behind it) into its amax gives a larger word.
    Asserted here, on the expectation returned, for every boundary without exception:
    key(want[b]) > max(key(want[:b]))."""
    import amax_ref
    first, step = STAIR[dt]
    bs = np.array(sorted(set(int(b) for b in boundaries)), dtype=np.int64)
    assert bs.size and 0 <= bs[0] and bs[-1] < length, "every boundary is a lane of the sources"
    level = np.searchsorted(bs, np.arange(length), side="right")
    rng = np.random.default_rng([seed, 78, k, length])
    enc = first + step * level + rng.integers(0, step, length)
    ins = one_hot(dt, k, enc, seed)
    want = expected(dt, "sum", ins, shape=shape, scale=scale, hop=hop)
    keys = amax_ref.keys(dt, want).astype(np.int64)
    before = np.maximum.accumulate(keys)
    for b in bs:
        assert b == 0 or keys[b] > before[b - 1], ("no strict step at boundary", dt, k, int(b), scale)
    return ins, want


# ---- the hooks of libftar_bench.so ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hooks():
    import ftar
    lib = ftar.bench_lib()
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.ftar_debug_reduce_ex.argtypes = [ctypes.POINTER(vp), i, vp, sz, i, i, i, ctypes.POINTER(i), i, i,
                                         ctypes.POINTER(ctypes.c_double), vp]
    lib.ftar_debug_reduce_amax_ex.argtypes = [ctypes.POINTER(vp), i, vp, sz, i, i, i, ctypes.POINTER(i), i, i,
                                              ctypes.POINTER(ctypes.c_double), vp, vp]
    lib.ftar_debug_gather.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz), i, i, sz, i, vp]
    return lib


def reduce_ex(srcs, dst, count, dt, op="sum", round_each=False, shape=None, lds=True, scale=None, amax=None,
              check=True):
    """ftar::launch_reduce with every argument (ftar_debug_reduce_ex).  amax=ptr: the amax finish maxing into the
    device word at ptr AS IT IS (ftar_debug_reduce_amax_ex: no memset; the scale defaults to 1.0).  Returns the
    status, which check=False leaves to the caller (tests/fold_dispatch_cases.py records the refusals)."""
    import ftar
    arr = (ctypes.c_void_p * len(srcs))(*srcs)
    sh = (ctypes.c_int * max(1, len(shape or ())))(*(shape or ()))
    if amax is not None and scale is None:
        scale = 1.0
    sc = None if scale is None else ctypes.byref(ctypes.c_double(
        float(scale) if dt == "f64" else float(np.float32(scale))))
    if amax is None:
        st = _hooks().ftar_debug_reduce_ex(arr, len(srcs), dst, count, ftar.DTYPE[dt], ftar.OP[op], int(round_each),
                                           sh, len(shape or ()), int(lds), sc, None)
    else:
        st = _hooks().ftar_debug_reduce_amax_ex(arr, len(srcs), dst, count, ftar.DTYPE[dt], ftar.OP[op],
                                                int(round_each), sh, len(shape or ()), int(lds), sc, amax, None)
    assert st == 0 or not check, (st, ftar.last_error())
    return st


def gather(srcs, dsts, nbytes, nt=True, max_wg_per_seg=0, release_system=False):
    """ftar::launch_gather on the segments dsts[i][0 .. nbytes[i]) = srcs[i][...] (ftar_debug_gather)."""
    import ftar
    m = len(srcs)
    st = _hooks().ftar_debug_gather((ctypes.c_void_p * max(1, m))(*srcs), (ctypes.c_void_p * max(1, m))(*dsts),
                                    (ctypes.c_size_t * max(1, m))(*nbytes), m, int(nt), max_wg_per_seg,
                                    int(release_system), None)
    assert st == 0, (st, ftar.last_error())


# ---- one fold, many launches ------------------------------------------------------------------------------
WORD_AT = 16         # the amax word's offset in its 64-byte arena


class Fold:
    """k sources and their expectation on the device, uploaded once; launches at any element offset and count are
    pointer arithmetic into the source and destination arenas.  Source j's element i sits shifts[j] + i elements
    behind a 16-byte boundary (shifts: which sources are misaligned against the others)."""

    def __init__(self, ins, want, shifts=None, device="cuda"):
        import torch
        self.k, self.n = len(ins), ins[0].size
        self.esz = ins[0].dtype.itemsize
        self.ve = 16 // self.esz
        self.shifts = list(shifts or [0] * self.k)
        self.row = -(-(self.n * self.esz + 32) // 16) * 16 + 64
        self.src = Arena(self.k * self.row, device)
        for j, x in enumerate(ins):
            assert x.size == self.n and x.dtype.itemsize == self.esz
            self.src.upload(j * self.row + self.shifts[j] * self.esz, x)
        self.dst = Arena(self.n * self.esz + 16, device)
        self.want = torch.from_numpy(as_bytes(want).copy()).to(device)
        assert self.want.numel() == self.n * self.esz
        self.want_host = np.ascontiguousarray(want).reshape(-1)      # the expectation's elements, for amax_ref
        self.am = None

    def word_ptr(self):
        """The amax word of a launch: 4 bytes at offset WORD_AT of a guarded 64-byte arena of their own."""
        if self.am is None:
            self.am = Arena(64, self.want.device)
        return self.am.ptr(WORD_AT)

    def set_word(self, value):
        """What the word holds before a launch (the test's memset)."""
        self.word_ptr()
        raw = np.array([value], np.uint32).view(np.uint8)
        self.am.window(WORD_AT, WORD_AT + 4).copy_(self.src.torch.from_numpy(raw.copy()))

    def src_off(self, j, off):
        return j * self.row + (self.shifts[j] + off) * self.esz

    def pointers(self, off, alias=None):
        """(source pointers, destination pointer) of a launch on elements [off, off + n) of every source."""
        srcs = [self.src.ptr(self.src_off(j, off)) for j in range(self.k)]
        return srcs, (self.dst.ptr(off * self.esz) if alias is None else srcs[alias])

    def verify(self, off, n, alias=None, word=None):
        """After a launch on [off, off + n): None, or what is wrong -- the payload against the expectation, every
        byte around it, and every source that is not the destination.  word (amax_ref.amax_bits of the expected
        payload): also the amax word at word_ptr() against it (amax_ref.matches) and every byte of its arena but
        those 4.  Puts the arenas back."""
        torch = self.src.torch
        nb = n * self.esz
        if alias is None:
            arena, other, lo = self.dst, self.src, off * self.esz
        else:
            arena, other, lo = self.src, self.dst, self.src_off(alias, off)
        msgs = []
        got = arena.window(lo, lo + nb)
        exp = self.want[off * self.esz:off * self.esz + nb]
        if not torch.equal(got, exp):
            bad = torch.nonzero(got != exp).reshape(-1)
            e = int(bad[0]) // self.esz
            msgs.append(f"payload: {int(bad.numel())} bytes differ, first in element {e} of {n}: got "
                        f"{bytes(got[e * self.esz:(e + 1) * self.esz].cpu().tolist()).hex()}, want "
                        f"{bytes(exp[e * self.esz:(e + 1) * self.esz].cpu().tolist()).hex()}")
        stray = check_untouched(arena, lo, lo + nb)
        if stray:
            msgs.append(("destination arena: " if alias is None else "source arena around the aliased source: ") + stray)
        stray = check_untouched(other)
        if stray:
            msgs.append(("source arena: " if alias is None else "destination arena: ") + stray)
        if word is not None:
            import amax_ref
            self.word_ptr()
            got_w = int(self.am.window(WORD_AT, WORD_AT + 4).cpu().numpy().view(np.uint32)[0])
            if not amax_ref.matches(got_w, word):
                msgs.append(f"amax word: got 0x{got_w:08x}, want "
                            + (word if word == amax_ref.NAN else f"0x{word:08x}"))
            stray = check_untouched(self.am, WORD_AT, WORD_AT + 4)
            if stray:
                msgs.append("amax word's arena: " + stray)
            self.am.restore(-self.am.origin, self.am.total - self.am.origin)
        if msgs:
            for a in (self.src, self.dst):
                a.restore(-a.origin, a.total - a.origin)
            return "; ".join(msgs)
        arena.restore(lo, lo + nb)
        return None
