"""Steps per second of k_simulate (random simulation) on the headline binding (Kip320 3/6/6/2) and BASELINE config 5
(Kip320 7/8/8/3): depth 100, launches of 2^20 walks.  A launch of the headline takes 1.5 ms — too short a window to time alone —
so a timed sample is as many back-to-back launches (each of the next 2^20 walks) as fill --sample-ms of kernel time; one
warm-up batch, several samples, the sum of the launches' HIP-event durations per sample, median and spread.  Beside it the same walks run by the host emulation of the same lane-local code (tests/sim_emu.cpp) on 16 threads, in
the same run: a port of this engine's walk to the CPU, not TLC.  Writes profiles/sim_steps.json with the register / scratch
figures of the two code objects as their metadata states them.

    python tools/sim_bench.py [--walks N] [--depth D] [--repeats R] [--sample-ms MS] [--cpu-walks N] [--cpu-threads T] [--out FILE]
"""
import argparse
import glob
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BINDINGS = {
    "headline_kip320_3_6_6_2": (dict(model="Kip320", n_replicas=3, log_size=6, max_records=6, max_leader_epoch=2), (5, 3, 6, 6, 2, 0, 0)),
    "config5_kip320_7_8_8_3": (dict(model="Kip320", n_replicas=7, log_size=8, max_records=8, max_leader_epoch=3), (5, 7, 8, 8, 3, 0, 0)),
}


def msgpack_uint(blob, at):
    b = blob[at]
    if b <= 0x7f:
        return b
    if b == 0xcc:
        return blob[at + 1]
    if b == 0xcd:
        return int.from_bytes(blob[at + 1:at + 3], "big")
    if b == 0xce:
        return int.from_bytes(blob[at + 1:at + 5], "big")
    return None


def resources(path):
    """register and scratch figures of the (single) kernel of a -simulate code object, from its AMDGPU metadata note"""
    blob = open(path, "rb").read()
    out = {}
    for key in (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size"):
        at = blob.find(key.encode())
        out[key[1:]] = msgpack_uint(blob, at + len(key)) if at >= 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sample-ms", type=float, default=200.0, help="kernel time a timed sample should fill (launches per sample follow)")
    ap.add_argument("--cpu-walks", type=int, default=1 << 20, help="walks of the host emulation's leg (the first of the batch)")
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_steps.json"))
    a = ap.parse_args()
    import kafka_specification_amd as kmc
    import sim_emu
    report = dict(tool="tools/sim_bench.py", walks_per_launch=a.walks, sample_ms=a.sample_ms, depth=a.depth, repeats=a.repeats, seed=a.seed, bindings={})
    for name, (consts, c7) in BINDINGS.items():
        cfg = kmc.CheckerConfig(invariants=(), table_capacity=1 << 16, frontier_capacity=1 << 12, **consts)
        with kmc.ModelChecker(cfg) as mc:
            first = mc.simulate(a.walks, depth=a.depth, seed=a.seed)   # warm-up: the code object joins the handle, clocks rise
            launches = max(1, math.ceil(a.sample_ms / (first.seconds_kernel * 1e3)))
            runs = [mc.simulate(launches * a.walks, depth=a.depth, seed=a.seed, walks_per_launch=a.walks) for _ in range(a.repeats)]
        assert all(r.states_generated == runs[0].states_generated and r.launches == launches for r in runs)
        steps = runs[0].states_generated - runs[0].walks           # of one timed sample
        first_steps = first.states_generated - first.walks         # of the first 2^20 walks: what the emulation walks too
        kernel_ms = sorted(r.seconds_kernel * 1e3 for r in runs)
        # the fourth code object's file: in the cache's simulate/ sub-directory, same name and compiler as the search's own, tagged -simulate
        own = kmc.code_object_path(cfg)
        stem = os.path.basename(own).split("-gfx950-")[0]
        found = sorted(glob.glob(os.path.join(os.path.dirname(own), "simulate", stem + "-gfx950-*-c" + own.rsplit("-c", 1)[1].replace(".hsaco", "-simulate.hsaco"))))
        path = found[0] if found else ""
        t0 = time.perf_counter()
        emu = sim_emu.Batch(c7, a.seed, a.cpu_walks, a.depth, threads=a.cpu_threads, record=False)
        cpu_s = time.perf_counter() - t0
        cpu_steps = int(emu.result.states_generated - emu.result.walks)
        if a.cpu_walks == a.walks:
            assert cpu_steps == first_steps, "the emulation walked other walks"
        med = statistics.median(kernel_ms)
        report["bindings"][name] = dict(
            constants=consts, launches_per_sample=launches, walks_per_sample=launches * a.walks, steps=steps,
            states_generated=runs[0].states_generated, ended_early=runs[0].ended_early,
            first_launch=dict(walks=a.walks, steps=first_steps, kernel_ms=first.seconds_kernel * 1e3),
            kernel_ms=dict(median=med, min=kernel_ms[0], max=kernel_ms[-1], all=kernel_ms),
            gpu_steps_per_s=steps / (med * 1e-3), ns_per_step=med * 1e6 / steps, kernel_ms_per_launch=med / launches,
            wall_s_median=statistics.median(r.seconds_total for r in runs),
            host_emulation=dict(threads=a.cpu_threads, walks=a.cpu_walks, steps=cpu_steps, seconds=cpu_s, steps_per_s=cpu_steps / cpu_s,
                                note="tests/sim_emu.cpp: this engine's lane-local walk compiled for the host; a port, not TLC"),
            code_object=dict(file=os.path.basename(path), **(resources(path) if path else {})))
        print(name, json.dumps(report["bindings"][name]["kernel_ms"]), f"{steps / (med * 1e-3):.3e} steps/s GPU,",
              f"{cpu_steps / cpu_s:.3e} steps/s host emulation", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))


if __name__ == "__main__":
    main()
