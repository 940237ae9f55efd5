"""Steps per second of k_simulate_from (walks from start states given as data) beside k_simulate, on the headline binding
(Kip320 3/6/6/2) and BASELINE config 5 (Kip320 7/8/8/3): depth 100, launches of 2^20 walks.  Three arms:
  (a) kmc_simulate — k_simulate, every walk from Init;
  (b) kmc_simulate_from with starts = {Init} at KMC_SIM_REFILL_MIN = 1, 16, 64 — the same walks as (a): every counter is
      asserted equal before a rate is reported;
  (c) kmc_simulate_from from the frontier of a level-limited search (headline level 23, config 5 level 10), sub-sampled evenly
      to at most 2^20 states, at the same three thresholds.
One handle per arm, all open together (a threshold is a compile-time constant: a handle's objects are built under the
KMC_JIT_DEFINES it was opened with, here into a cache directory per arm under kmc_cache_exp/sim_from/ — `--precompile` fills
them without a GPU, minutes for config 5, so that the measuring run compiles nothing); one warm-up batch per arm, then --repeats rounds in which the arms take turns, a
sample being as many back-to-back launches as fill --sample-ms of arm (a)'s kernel time; the sum of the launches' HIP-event
durations per sample, median and spread.  Writes profiles/simulate_from.json with a hash of every code object that ran and
the register / scratch / LDS figures of both kernels as the objects' metadata state them.

    python tools/sim_from_bench.py --precompile
    python tools/sim_from_bench.py [--walks N] [--depth D] [--repeats R] [--sample-ms MS] [--out FILE]
"""
import argparse
import glob
import hashlib
import json
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINDINGS = {   # name -> (constants, the level whose frontier arm (c) starts on)
    "headline_kip320_3_6_6_2": (dict(model="Kip320", n_replicas=3, log_size=6, max_records=6, max_leader_epoch=2), 23),
    "config5_kip320_7_8_8_3": (dict(model="Kip320", n_replicas=7, log_size=8, max_records=8, max_leader_epoch=3), 10),
}
THRESHOLDS = (1, 16, 64)
COUNTERS = ("walks", "states_generated", "action_taken", "ended_early", "longest_walk", "verdict", "launches")


def resources(path):
    """per kernel of a -simulate code object: the figures of its AMDGPU metadata note (llvm-readelf; the keys of a kernel's map)"""
    notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- (?=\.agpr_count)", notes):   # (a kernel's map begins with its first key)
        name = re.search(r"\.name:\s*(kmc_simulate(?:_from)?)_", blk)
        if name:
            out[name.group(1)] = {k: int(m.group(1)) for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                               "private_segment_fixed_size", "group_segment_fixed_size")
                                  for m in [re.search(r"\." + k + r":\s*(\d+)", blk)] if m}
    return out


def under(kmc, key, consts, precompile=False):
    """A handle opened under the defines of arm `key` ("a": none; n: -DKMC_SIM_REFILL_MIN=n), with a cache directory of its own,
    so that the one -simulate object in it is the one that ran; precompile: specialise its two objects instead (no GPU needed)."""
    old = os.environ.pop("KMC_JIT_DEFINES", None)
    if key != "a":
        os.environ["KMC_JIT_DEFINES"] = f"-DKMC_SIM_REFILL_MIN={key}"
    try:
        cache = os.path.join(ROOT, "kafka_specification_amd", "kmc_cache_exp", "sim_from", "default" if key == "a" else f"refill{key}")
        os.makedirs(cache, exist_ok=True)
        cfg = kmc.CheckerConfig(invariants=(), table_capacity=1 << 16, frontier_capacity=1 << 12, cache_dir=cache, **consts)
        if precompile:
            kmc.precompile(cfg, "gfx950", 0)
            kmc.precompile_simulate(cfg, "gfx950")
            return None
        stem = os.path.basename(kmc.code_object_path(cfg)).split("-gfx950-")[0]
        return kmc.ModelChecker(cfg), os.path.join(cache, "simulate", stem + "-gfx950-*-simulate.hsaco")
    finally:
        os.environ.pop("KMC_JIT_DEFINES", None)
        if old is not None:
            os.environ["KMC_JIT_DEFINES"] = old


def precompile_one(job):
    import kafka_specification_amd as kmc
    under(kmc, job[0], job[1], precompile=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sample-ms", type=float, default=200.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate_from.json"))
    ap.add_argument("--precompile", action="store_true", help="specialise the arms' code objects into their cache directories and stop (no GPU needed)")
    a = ap.parse_args()
    import numpy as np
    import kafka_specification_amd as kmc
    if a.precompile:
        from concurrent.futures import ProcessPoolExecutor
        with ProcessPoolExecutor(max_workers=8) as ex:
            list(ex.map(precompile_one, [(key, consts) for key in ("a",) + THRESHOLDS for (consts, _level) in BINDINGS.values()]))
        return
    report = dict(tool="tools/sim_from_bench.py", walks_per_launch=a.walks, depth=a.depth, repeats=a.repeats, sample_ms=a.sample_ms, seed=a.seed,
                  thresholds=list(THRESHOLDS), bindings={})
    for name, (consts, level) in BINDINGS.items():
        with kmc.ModelChecker(kmc.CheckerConfig(invariants=(), table_capacity=1 << 26, frontier_capacity=1 << 23, max_levels=level, **consts)) as mc:
            mc.run()
            front = mc.frontier_states()
        n_front = len(front)
        if n_front > (1 << 20):   # evenly
            front = front[(np.arange(1 << 20, dtype=np.uint64) * np.uint64(n_front)) >> np.uint64(20)]
        front = np.ascontiguousarray(front)
        handles = {key: under(kmc, key, consts) for key in ("a",) + THRESHOLDS}
        base = handles["a"][0]
        init = np.array([base.pack(base.walk(0, depth=1)[0][1])], dtype=np.uint64)
        arms = {"a_simulate": (base, None)}
        arms.update({f"b_from_init_refill{n}": (handles[n][0], init) for n in THRESHOLDS})
        arms.update({f"c_from_frontier_refill{n}": (handles[n][0], front) for n in THRESHOLDS})
        first = {k: mc.simulate(a.walks, depth=a.depth, seed=a.seed, starts=st) for k, (mc, st) in arms.items()}   # warm-up
        launches = max(1, math.ceil(a.sample_ms / (first["a_simulate"].seconds_kernel * 1e3)))
        runs = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, (mc, st) in arms.items():   # the arms take turns
                runs[k].append(mc.simulate(launches * a.walks, depth=a.depth, seed=a.seed, walks_per_launch=a.walks, starts=st))
        want = {c: getattr(runs["a_simulate"][0], c) for c in COUNTERS}
        for k in arms:
            assert all(all(getattr(r, c) == getattr(runs[k][0], c) for c in COUNTERS) for r in runs[k]), k
            if k.startswith("b_"):
                assert {c: getattr(runs[k][0], c) for c in COUNTERS} == want, f"{k}: other walks than k_simulate's"
        out = dict(constants=consts, launches_per_sample=launches, frontier=dict(level=level, states=n_front, starts=len(front)), arms={}, code_objects={})
        for k, rs in runs.items():
            ms = sorted(r.seconds_kernel * 1e3 for r in rs)
            steps = rs[0].states_generated - rs[0].walks
            med = statistics.median(ms)
            out["arms"][k] = dict(steps=steps, states_generated=rs[0].states_generated, ended_early=rs[0].ended_early, longest_walk=rs[0].longest_walk,
                                  mean_states_per_walk=rs[0].states_generated / rs[0].walks,
                                  kernel_ms=dict(median=med, min=ms[0], max=ms[-1], all=ms), steps_per_s=steps / (med * 1e-3))
            print(name, k, f"{steps / (med * 1e-3):.3e} steps/s", f"median {med:.2f} ms [{ms[0]:.2f}, {ms[-1]:.2f}]", flush=True)
        for key, (mc, pattern) in handles.items():
            (path,) = glob.glob(pattern)
            out["code_objects"]["default" if key == "a" else f"refill{key}"] = dict(
                file=os.path.basename(path), sha256=hashlib.sha256(open(path, "rb").read()).hexdigest(), kernels=resources(path))
            mc.close()
        report["bindings"][name] = out
    # the default threshold: the fastest of arm (c), its median kernel time summed over the bindings (the same walks at every threshold)
    total = {n: sum(b["arms"][f"c_from_frontier_refill{n}"]["kernel_ms"]["median"] for b in report["bindings"].values()) for n in THRESHOLDS}
    report["arm_c_kernel_ms_summed"] = {str(n): v for n, v in total.items()}
    report["fastest_threshold_arm_c"] = min(total, key=total.get)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"wrote": a.out, "fastest_threshold_arm_c": report["fastest_threshold_arm_c"]}))


if __name__ == "__main__":
    main()
