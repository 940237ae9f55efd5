"""A plain `bench.py --gpus 1 --steps N --warmup W` on the GPU: the headline's line alone — none of the legs that take runs
of their own (they belong to --full) — with --steps the number of timed steps, and --dump-outputs writing what the last
timed step returned.  On a small binding (--workload) and small tables, so that it takes seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kmo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("orbit_counting", "traces_kept", "cold_start", "baseline_configs", "stretch_1gpu", "cpu_baseline", "device")


def test_plain_line_has_no_legs_and_dumps_the_last_steps_counts(tmp_path):
    dump = str(tmp_path / "outputs")
    env = dict(os.environ, KMC_BENCH_TABLE=str(1 << 20), KMC_BENCH_FRONTIER=str(1 << 16))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "Kip320,3,2,2,1", "--dump-outputs", dump], capture_output=True, text=True, env=env,
                       timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert [k for k in LEGS if k in r] == []
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    assert r["unit"] == "distinct states/s" and r["dtype"] == "u64"
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=2, R=2, E=1, invariants=("TypeOk", "WeakIsr", "StrongIsr")))
    assert abs(r["value"] - 1e3 * o.distinct / r["ms_per_step"]) <= 1e-6 * r["value"]   # 3 timed steps of o.distinct states each
    got = {f[:-4]: np.load(os.path.join(dump, f)) for f in sorted(os.listdir(dump))}
    assert sorted(got) == ["action_generated", "counts", "levels", "verdict", "violation_count"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert list(got["counts"][:3]) == [o.distinct, o.generated, o.depth] and got["verdict"][0] == 0
    assert list(got["levels"]) == list(o.levels)
