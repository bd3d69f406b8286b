"""The grid of ftar::launch_reduce calls whose kernel choice tests/golden/fold_dispatch.json pins
(tools/fold_dispatch_table.py writes it, tests/test_gpu_fold_dispatch.py compares): grid() yields every call,
run() makes them through kernel_edges.reduce_ex and records which kernel each reached or the status that refused
it, encode() / decode() pack that record.

No GPU import at module level: torch, ftar and kernel_edges' hooks are loaded by run()."""
from collections import namedtuple

DTYPES = ("u8", "i8", "u16", "i16", "i32", "i64", "f32", "f64", "bool", "bf16", "f16", "f8e4m3", "f8e5m2")
OPS = ("sum", "band", "max", "min")
FINISHES = ("plain", "scaled", "amax")            # no scale; a scale; a scale and the amax word
KS = (1, 2, 3, 8, 9, 16, 17, 64)                  # flat folds: a copy, both sides of k = 2 (all lds = 0 unrolls), of
#                                                   HOT = 8 and of HOT = 16, and FTAR_MAX_K
SHAPES = ((2, 2), (2, 4), (4, 2), (4, 4), (2, 2, 2), (2, 2, 2, 2),   # the compile-time shapes
          (3, 2), (3, 3), (3, 4),                                    # runtime leaf codes at an unrolled k (6, 9, 12)
          (5, 2))                                                    # a runtime-k tree
ALIGNS = ("aligned", "head", "split")             # all pointers on 16 bytes; all one element behind; source 0 alone
ESIZE = {"u8": 1, "i8": 1, "bool": 1, "f8e4m3": 1, "f8e5m2": 1, "u16": 2, "i16": 2, "bf16": 2, "f16": 2,
         "i32": 4, "f32": 4, "i64": 8, "f64": 8}
SCALE = 0.5
ROW = 128                                         # bytes between two sources: 3 vectors + 2 elements fit in 64

Case = namedtuple("Case", "dt op finish k shape lds align round_each")


def count(dt):
    """Three 16-byte vectors and one element: a vector body and a tail (and, shifted, a head)."""
    return 3 * (16 // ESIZE[dt]) + 1


def folds():
    """(k, shape) of every fold: the flat ones, and every shape at its own leaf count and at one leaf more (a
    shape that does not multiply out to k: refused where the shape is read, ignored where it is not)."""
    out = [(k, None) for k in KS]
    for sh in SHAPES:
        p = 1
        for w in sh:
            p *= w
        out += [(p, sh), (p + 1, sh)]
    return out


def grid():
    """Every call, in the file's order: the axes that change the kernel least run fastest."""
    for dt in DTYPES:
        for op in OPS:
            for fin in FINISHES:
                for k, sh in folds():
                    for lds in (1, 0):
                        for al in ALIGNS:
                            for re in (0, 1):
                                yield Case(dt, op, fin, k, sh, lds, al, re)


def axes():
    """What grid() is built from, as the golden file stores it: a file made from another grid does not compare."""
    return {"dtypes": list(DTYPES), "ops": list(OPS), "finishes": list(FINISHES), "ks": list(KS),
            "shapes": [list(s) for s in SHAPES], "aligns": list(ALIGNS), "lds": [1, 0], "round_each": [0, 1],
            "scale": SCALE, "count": "3 vectors + 1 element",
            "order": "dtype, op, finish, fold (flat k, then each shape at its k and at k + 1), lds, align, round_each"}


def encode(results):
    """results: per case a kernel name or a status code (int, nonzero).  -> (kernel table, runs): runs is a flat
    list of value, length pairs, value >= 0 an index into the table and value < 0 minus a status."""
    table, index, runs = [], {}, []
    for r in results:
        if isinstance(r, int):
            assert r > 0, r
            v = -r
        else:
            if r not in index:
                index[r] = len(table)
                table.append(r)
            v = index[r]
        if runs and runs[-2] == v:
            runs[-1] += 1
        else:
            runs += [v, 1]
    return table, runs


def decode(table, runs):
    out = []
    for v, n in zip(runs[0::2], runs[1::2]):
        out += [table[v] if v >= 0 else -v] * n
    return out


def run(cases):
    """Each case through kernel_edges.reduce_ex on zeroed buffers of its own size: ftar.last_kernel() of the call,
    or the status that refused it."""
    import torch

    import ftar
    import kernel_edges as ke

    src = torch.zeros(ke.MAX_K * ROW + 64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(ROW + 64, dtype=torch.uint8, device="cuda")
    word = torch.zeros(16, dtype=torch.uint8, device="cuda")
    s0, d0 = src.data_ptr() + (-src.data_ptr()) % 16, dst.data_ptr() + (-dst.data_ptr()) % 16
    out = []
    for c in cases:
        e = ESIZE[c.dt]
        assert (count(c.dt) + 1) * e <= 64 and c.k <= ke.MAX_K
        shift = 0 if c.align == "aligned" else e
        srcs = [s0 + j * ROW + (shift if c.align == "head" or j == 0 else 0) for j in range(c.k)]
        st = ke.reduce_ex(srcs, d0 + (shift if c.align == "head" else 0), count(c.dt), c.dt, c.op,
                          round_each=bool(c.round_each), shape=c.shape, lds=bool(c.lds),
                          scale=None if c.finish == "plain" else SCALE,
                          amax=word.data_ptr() if c.finish == "amax" else None, check=False)
        out.append(ftar.last_kernel() if st == 0 else int(st))
    torch.cuda.synchronize()
    return out
