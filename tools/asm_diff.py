#!/usr/bin/env python3
"""Compare two device assembly listings (hipcc --cuda-device-only -S) kernel by kernel.

    tools/asm_diff.py OLD.s NEW.s [--show SUBSTRING]

Per symbol the instruction stream is taken with comments and directives stripped and local labels
renumbered in order of appearance.  Prints the symbols only one side has, and for every kernel whose
stream differs: the instruction counts, whether the opcode multiset is equal (registers / operand
order / scheduling only), whether it is equal once _e32 / _e64 encodings are ignored, and the
resource lines the compiler prints after each kernel (VGPRs, scratch, occupancy).  Exit status 1 if
the symbol sets differ or a kernel gained scratch or lost occupancy, else 0.
"""
import argparse
import collections
import difflib
import re
import subprocess
import sys

RES = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def parse(path):
    """{symbol: (instructions, {resource: int})}"""
    out, sym, body = {}, None, []
    res_for = None
    for raw in open(path, errors="replace"):
        line = raw.strip()
        if sym is None:
            m = re.match(r"; (\w+): (\d+)$", line)
            if m and res_for and m.group(1) in RES:
                out[res_for][1][m.group(1)] = int(m.group(2))
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                sym, body, res_for = m.group(1), [], None
            continue
        if line.startswith(".Lfunc_end"):
            out[sym] = (renumber(body), {})
            res_for, sym = sym, None
            continue
        line = line.split(";", 1)[0].strip()
        if not line or line == sym + ":" or (line.startswith(".") and not line.endswith(":")):
            continue
        body.append(re.sub(r"\s+", " ", line))
    return out


def renumber(body):
    names = {}
    def sub(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    return [re.sub(r"\.L\w+", sub, l) for l in body]


def opcodes(body, strip_enc=False):
    ops = [l.split(" ", 1)[0] for l in body if not l.endswith(":")]
    if strip_enc:
        ops = [re.sub(r"_e(32|64)$", "", o) for o in ops]
    return collections.Counter(ops)


def demangle(syms):
    if not syms:
        return {}
    p = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True)
    names = p.stdout.splitlines() if p.returncode == 0 else syms
    short = [n.replace("ftar::(anonymous namespace)::", "") for n in names]
    return {s: re.sub(r"^void |\((Srcs|ftar::).*$", "", n) for s, n in zip(syms, short)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", help="print a unified diff of the kernels whose demangled name contains this")
    a = ap.parse_args()
    old, new = parse(a.old), parse(a.new)
    bad = False
    for s in sorted(set(old) ^ set(new)):
        print(("only in old: " if s in old else "only in new: ") + s)
        bad = True
    both = sorted(set(old) & set(new))
    diff = [s for s in both if old[s][0] != new[s][0]]
    names = demangle(diff)
    classes = collections.Counter()
    for s in diff:
        (ob, orr), (nb, nr) = old[s], new[s]
        if opcodes(ob) == opcodes(nb):
            cls = "same opcodes"
        elif opcodes(ob, True) == opcodes(nb, True):
            cls = "encoding only"
        else:
            cls = "different"
        classes[cls] += 1
        res = " ".join("%s %s->%s" % (k, orr.get(k), nr.get(k)) for k in RES if orr.get(k) != nr.get(k))
        print("%-14s %5d -> %5d  %s  %s" % (cls, len(ob), len(nb), names[s], res))
        if nr.get("ScratchSize", 0) > orr.get("ScratchSize", 0) or nr.get("Occupancy", 0) < orr.get("Occupancy", 0):
            print("  ^ gained scratch or lost occupancy")
            bad = True
        if a.show and a.show in names[s]:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(ob, nb, "old", "new", lineterm="", n=2))
    print("%d symbols, %d identical, %s" % (len(both), len(both) - len(diff), dict(classes) or "none differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
