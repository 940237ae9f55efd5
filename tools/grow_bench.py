"""What the growing seen-set costs, on the headline binding (Kip320 3/6/6/2, 279,753,922 states), one process, arms interleaved,
one warm-up and --repeats timed runs each, median and min - max.  Writes profiles/table_growth.json.

(a) kmc_run with the table and frontier bench.py passes (a fixed table: the code every search ran before growth existed) against
    kmc_run started at 2^24 slots with growth, under KMC_REHASH=window at each --window-kib and under KMC_REHASH=scatter.  A grown
    handle keeps its table, so every growing run has a handle of its own (opening and closing it is not timed).  Counts must equal
    the golden fixture in every arm.
(b) per growth record of the median run of each arm: entries per second and bytes read + written per second (old table in, new
    table out, predecessor words included), beside a device-to-device copy that moves the same number of bytes, timed in this
    process with device events; and the windowed-to-scatter ratio at each size.
(c) one more growing run (default kernel and window) under KMC_VERBOSE, whose per-growth line on stderr says where the HOST's time
    went: allocation of the new tables, the rehash with its wait, release of the old tables.

    python tools/grow_bench.py [--repeats R] [--window-kib 8,16,32,64,128] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def copy_gbps(nbytes, repeats=5):
    """GB/s (read + written) of a device-to-device copy that reads nbytes / 2 and writes nbytes / 2."""
    import torch
    n = max(nbytes // 2, 1 << 20)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst.copy_(src)
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return 2 * n / (statistics.median(ms) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-kib", default="8,16,32,64,128")
    ap.add_argument("--table", type=int, default=1 << 30)
    ap.add_argument("--frontier", type=int, default=1 << 26)
    ap.add_argument("--start", type=int, default=1 << 24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_growth.json"))
    a = ap.parse_args()
    import kafka_specification_amd as kmc
    from kafka_specification_amd.configs import HEADLINE
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_kip320_3_6_6_2.json")))
    arms = [("fixed", None, None)] + [(f"window_{k}k", "window", k) for k in a.window_kib.split(",")] + [("scatter", "scatter", None)]
    fixed = kmc.ModelChecker(kmc.CheckerConfig(**HEADLINE, table_capacity=a.table, frontier_capacity=a.frontier))
    runs = {name: [] for name, _, _ in arms}
    dropped = {}

    def once(name, kernel, kib):
        if kernel is None:
            r, growths = fixed.run(), []
        else:
            os.environ["KMC_REHASH"] = kernel
            os.environ["KMC_REHASH_WINDOW_KIB"] = str(kib or 32)
            with kmc.ModelChecker(kmc.CheckerConfig(**HEADLINE, table_capacity=a.start, frontier_capacity=a.frontier)) as mc:
                mc.enable_table_growth()
                r, growths = mc.run(), mc.growth_stats()
        assert (r.verdict, r.distinct, r.generated, r.depth) == ("ok", golden["distinct"], golden["generated"], golden["depth"]), (name, r)
        return dict(seconds_total=r.seconds_total, seconds_expand=r.seconds_expand, seconds_clear=r.seconds_clear,
                    expand_launches=r.expand_launches, table_slots_at_end=r.table_capacity, growths=growths)

    for rep in range(a.repeats + 1):   # (the first round is the warm-up)
        for name, kernel, kib in list(arms):
            try:
                rec = once(name, kernel, kib)
            except kmc.KmcError as e:   # (a window size the launch refuses: the arm is dropped and named)
                print(name, "dropped:", e, flush=True)
                arms.remove((name, kernel, kib))
                dropped[name] = str(e)
                continue
            if rep:
                runs[name].append(rec)
            print(rep, name, f"{rec['seconds_total'] * 1e3:.2f} ms, rehash {sum(g['rehash_ms'] for g in rec['growths']):.2f} ms in "
                  f"{len(rec['growths'])} growths", flush=True)
    fixed.close()

    # (c) the library's own account of one growing run: its stderr (the C library's, descriptor 2) read back
    import re
    import tempfile
    os.environ.pop("KMC_REHASH", None)
    os.environ.pop("KMC_REHASH_WINDOW_KIB", None)
    os.environ["KMC_VERBOSE"] = "1"
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            verbose_run = once("verbose", "window", None)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode("utf-8", "replace")
    os.environ.pop("KMC_VERBOSE")
    host = [dict(old_slots=int(m[0]), new_slots=int(m[1]), window_kib=int(m[2]), kernel_ms=float(m[3]), alloc_ms=float(m[4]),
                 rehash_and_wait_ms=float(m[5]), release_ms=float(m[6]))
            for m in re.findall(r"seen-set grown at depth \d+: (\d+) -> (\d+) slots.*?\(window (\d+) KiB\) ([\d.]+) ms; on the host: allocation "
                                r"([\d.]+) ms, rehash with its wait ([\d.]+) ms, release of the old tables ([\d.]+) ms", text)]
    assert len(host) == len(verbose_run["growths"]), text[-2000:]

    eb = 8   # the headline's entries: 64-bit, no predecessors
    report = dict(tool="tools/grow_bench.py", binding=HEADLINE, repeats=a.repeats, fixed_table=a.table, frontier=a.frontier,
                  start_slots=a.start, arms={}, copy={}, dropped_arms=dropped,
                  host_time_of_one_growing_run=dict(kmc_run_ms=verbose_run["seconds_total"] * 1e3, growths=host,
                                                    alloc_ms=sum(g["alloc_ms"] for g in host), release_ms=sum(g["release_ms"] for g in host),
                                                    rehash_and_wait_ms=sum(g["rehash_and_wait_ms"] for g in host)))
    for name, _, _ in arms:
        tot = sorted(x["seconds_total"] * 1e3 for x in runs[name])
        med = sorted(runs[name], key=lambda x: x["seconds_total"])[len(runs[name]) // 2]
        growths = []
        for k, g in enumerate(med["growths"]):
            ms = sorted(x["growths"][k]["rehash_ms"] for x in runs[name] if len(x["growths"]) == len(med["growths"]))
            nbytes = (g["old_slots"] + g["new_slots"]) * eb
            if nbytes not in report["copy"]:
                report["copy"][nbytes] = copy_gbps(nbytes)
            m = statistics.median(ms)
            growths.append(dict(g, rehash_ms=dict(median=m, min=ms[0], max=ms[-1]), entries_per_s=g["moved"] / (m * 1e-3),
                                bytes_moved=nbytes, gbytes_per_s=nbytes / (m * 1e-3) / 1e9, copy_gbytes_per_s=report["copy"][nbytes]))
        report["arms"][name] = dict(kmc_run_ms=dict(median=statistics.median(tot), min=tot[0], max=tot[-1], all=tot),
                                    expand_ms_median=statistics.median(x["seconds_expand"] * 1e3 for x in runs[name]),
                                    clear_ms_median=statistics.median(x["seconds_clear"] * 1e3 for x in runs[name]),
                                    rehash_ms_median=statistics.median(sum(g["rehash_ms"] for g in x["growths"]) for x in runs[name]),
                                    expand_launches=med["expand_launches"], table_slots_at_end=med["table_slots_at_end"], growths=growths)
    base = report["arms"]["fixed"]["kmc_run_ms"]["median"]
    for name in report["arms"]:
        report["arms"][name]["ratio_to_fixed"] = report["arms"][name]["kmc_run_ms"]["median"] / base
    sc = report["arms"]["scatter"]["growths"]
    for name, kernel, _ in arms:
        if kernel == "window":
            for g, s in zip(report["arms"][name]["growths"], sc):
                if (g["old_slots"], g["new_slots"]) == (s["old_slots"], s["new_slots"]):
                    g["speedup_over_scatter"] = s["rehash_ms"]["median"] / g["rehash_ms"]["median"]
    report["copy"] = {str(k): v for k, v in report["copy"].items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({name: dict(kmc_run_ms=v["kmc_run_ms"]["median"], ratio=v["ratio_to_fixed"], rehash_ms=v["rehash_ms_median"])
                      for name, v in report["arms"].items()}))
    print(json.dumps({"wrote": a.out}))


if __name__ == "__main__":
    main()
