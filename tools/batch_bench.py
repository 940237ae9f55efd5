"""States and records per second of kmc_successors_batch (batched successors and invariants of states given as data) on the
headline binding (Kip320 3/6/6/2) and BASELINE config 5 (Kip320 7/8/8/3): up to 2^20 states of one BFS level.  One call's kernels
take 0.2 - 1 ms — too short a window to time alone — so a timed sample is --calls back-to-back calls; one warm-up call, several
samples, per sample the sums of the calls' HIP-event kernel times (kmc_batch_result: all three and each kernel) and of their wall
times (copies included), median and spread over the samples.  Beside it, in the same run, the one-state loop (kmc_successors +
kmc_check_states per state, both called through ctypes into preallocated buffers, as the batch is) on the first 4,096 of those
states: the existing path and the only baseline there is.  Writes profiles/successors_batch.json with the register / scratch
figures of the two batch code objects as their metadata states them.  (Under libkmc_tuning.so, KMC_BLOCKS_PER_CU=B sizes the count
and emit grids at B blocks per CU instead of the kernels' residency: the A/B of the grid.)

    python tools/batch_bench.py [--states N] [--repeats R] [--calls C] [--loop-states N] [--out FILE]
"""
import argparse
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINDINGS = {
    "headline_kip320_3_6_6_2": dict(model="Kip320", n_replicas=3, log_size=6, max_records=6, max_leader_epoch=2),
    "config5_kip320_7_8_8_3": dict(model="Kip320", n_replicas=7, log_size=8, max_records=8, max_leader_epoch=3),
}
INV = ("TypeOk", "WeakIsr", "StrongIsr")


def resources(path):
    """per kernel of a -batch code object: the register and scratch figures of its AMDGPU metadata note (llvm-readelf; the keys
    that follow a kernel's .name in the note's sorted map)"""
    import subprocess
    notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split(".name:")[1:]:
        name = blk.split()[0]
        if name.startswith("kmc_batch_"):
            out["_".join(name.split("_")[:3])] = {
                k: int(m.group(1)) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
                for m in [re.search(r"\." + k + r":\s*(\d+)", blk)] if m}
    return out


def level_states(kmc, consts, want):
    """up to `want` states of the first BFS level that holds as many (else of the deepest level tried)"""
    best = None
    for lv in range(1, 40):
        cfg = kmc.CheckerConfig(invariants=(), table_capacity=1 << 26, frontier_capacity=1 << 23, max_levels=lv, **consts)
        with kmc.ModelChecker(cfg) as mc:
            r = mc.run()
            if best is None or r.levels[-1] > len(best[1]):
                best = (lv, mc.frontier_states()[:want])
            if r.levels[-1] >= want or r.levels[-1] == 0 or r.distinct > (1 << 24):
                break
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=32, help="back-to-back calls of one timed sample")
    ap.add_argument("--loop-states", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "successors_batch.json"))
    a = ap.parse_args()
    import numpy as np
    import kafka_specification_amd as kmc
    from kafka_specification_amd import _native as nat
    report = dict(tool="tools/batch_bench.py", repeats=a.repeats, calls_per_sample=a.calls, inv_mask=7, library=os.path.basename(nat.LIB_PATH),
                  blocks_per_cu=os.environ.get("KMC_BLOCKS_PER_CU", "residency"), bindings={})
    for name, consts in BINDINGS.items():
        level, states = level_states(kmc, consts, a.states)
        n = len(states)
        cfg = kmc.CheckerConfig(invariants=INV, table_capacity=1 << 16, frontier_capacity=1 << 12, **consts)
        with kmc.ModelChecker(cfg) as mc:
            offsets, records, _ = mc.successors_batch(states, inv_mask=7)   # warm-up: the code object joins the handle, staging is sized
            W = mc.state_words
            bc, res = nat.KmcBatchConfig(inv_mask=7, states_per_launch=0), nat.KmcBatchResult()
            bad = np.zeros(n, dtype=np.uint32)
            p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))
            samples = []   # per sample: kernel, count, scan, emit, wall — milliseconds PER CALL
            for _ in range(a.repeats):
                acc = [0.0] * 5
                for _ in range(a.calls):
                    nat.check(mc._lib.kmc_successors_batch(mc.handle, C.byref(bc), p64(states), n, p64(offsets), p64(records), len(records),
                                                           bad.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(res)))
                    for k, v in enumerate((res.seconds_kernel, res.seconds_count, res.seconds_scan, res.seconds_emit, res.seconds_total)):
                        acc[k] += v * 1e3
                samples.append([v / a.calls for v in acc])
            assert res.records == len(records)
            # the existing path: one launch and one wait per state and per question, into buffers allocated once
            m = min(a.loop_states, n)
            one, got = (C.c_uint32 * 1)(), C.c_uint64()
            out = np.zeros((4096, W + 2), dtype=np.uint64)
            first = np.ascontiguousarray(states[:m])
            stride = W * 8
            base = first.ctypes.data
            t0 = time.perf_counter()
            loop_records = 0
            for i in range(m):
                w = C.cast(base + i * stride, C.POINTER(C.c_uint64))
                nat.check(mc._lib.kmc_successors(mc.handle, w, p64(out), 4096, C.byref(got)))
                nat.check(mc._lib.kmc_check_states(mc.handle, w, 1, 7, one))
                loop_records += got.value
            loop_s = time.perf_counter() - t0 if m else float("nan")
            assert loop_records == int(offsets[m])
        col = lambda k: sorted(s[k] for s in samples)
        kernel_ms, wall_ms = col(0), col(4)
        kmed, wmed = statistics.median(kernel_ms), statistics.median(wall_ms)
        share = [statistics.median(col(k)) for k in (1, 2, 3)]
        own = kmc.code_object_path(cfg)
        stem = os.path.basename(own).split("-gfx950-")[0]
        found = sorted(glob.glob(os.path.join(os.path.dirname(own), "batch", stem + "-gfx950-*-batch.hsaco")))
        report["bindings"][name] = dict(
            constants=consts, level=level, states=n, records=len(records), state_words=W,
            kernel_ms=dict(median=kmed, min=kernel_ms[0], max=kernel_ms[-1], all=kernel_ms),
            wall_ms=dict(median=wmed, min=wall_ms[0], max=wall_ms[-1], all=wall_ms),
            kernel_ms_by_kernel=dict(count=share[0], scan=share[1], emit=share[2]),
            kernel_share=dict(count=share[0] / sum(share), scan=share[1] / sum(share), emit=share[2] / sum(share)),
            states_per_s=dict(kernel=n / (kmed * 1e-3), wall=n / (wmed * 1e-3)),
            records_per_s=dict(kernel=len(records) / (kmed * 1e-3), wall=len(records) / (wmed * 1e-3)),
            one_state_loop=dict(states=m, records=loop_records, seconds=loop_s, states_per_s=m / loop_s if m else None,
                                records_per_s=loop_records / loop_s if m else None,
                                note="kmc_successors + kmc_check_states per state through ctypes into preallocated buffers, same handle, same run"),
            emit_stores="LDS-staged",
            code_object=dict(file=os.path.basename(found[0]) if found else "", kernels=resources(found[0]) if found else {}))
        print(name, f"{n} states, {len(records)} records: kernels {kmed:.3f} ms, call {wmed:.3f} ms;",
              f"count {share[0]:.4f} scan {share[1]:.4f} emit {share[2]:.4f} ms;",
              f"one-state loop {m / loop_s if m else 0:.3e} states/s against {n / (wmed * 1e-3):.3e}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))


if __name__ == "__main__":
    main()
