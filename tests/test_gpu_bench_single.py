"""bench.py's N = 1 run as a process: the plain run is the headline alone, --steps sets the timed steps,
--dump-outputs writes what the last timed step computed, and --full adds the line items."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 100_003   # odd, several workgroups, far below the 64 MB dump limit: the bucket is written whole


def _bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--elements", str(N)] + extra
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=170)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    from ftar import inputs as fi
    d = _bench(["--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert not {"same_buffers", "k8", "engine_local", "host_local", "cpu_baseline"} & set(d), sorted(d)
    # step 2 (the last of 3) ran on buffer set 2: seeds 0x5EED + 2, sources 0 and 1, folded left to right
    got = np.load(tmp_path / "reduce_out.npy")
    exp = fi.fill("f32", 0x5EED + 2, 0, N) + fi.fill("f32", 0x5EED + 2, 1, N)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_full_run_keeps_the_line_items():
    d = _bench(["--full", "--no-engine-local", "--no-host-local", "--cpu-seconds", "0.2"])
    assert d["check"] == "bit-exact" and d["same_buffers"]["ms_per_step"] > 0
    assert d["k8"]["in_place"]["ms"] > 0 and d["cpu_baseline"]["value"] > 0
