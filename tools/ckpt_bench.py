"""What a checkpoint costs in both formats, on the headline binding (Kip320 3/6/6/2) stopped at --levels (near its widest level)
in a table of --table slots, and on one run that grew its table from --start slots: file bytes, wall time of save and of load,
one process, arms interleaved, one warm-up and --repeats timed rounds, median and min - max.  Writes
profiles/compact_checkpoint.json.

Arms of the load: the classic file into a table of the saved size (the only size it takes), the compact file into the saved
size, into the smallest that holds the entries at load 0.8 and into four times the saved size; the compact file through a window of 16 / 32 / 64 KiB and through the scatter
form (KMC_REHASH_WINDOW_KIB / KMC_REHASH are read by kmc_table_growth_enable, so these arms load into a handle with growth
enabled and capped at its own size), beside a device-to-device copy of the entries' bytes in and the table's bytes out.  Every
loaded handle must hold the saved frontier (kmc_contains on a sample) and report the saved counts.

Every save and load is also split by the library's own account (KMC_VERBOSE's "checkpoint save / load" line on stderr, read
back here): kernels by HIP events, device <-> host copies with their waits, file I/O.  Not here: a one-pass look-back pack to set
against the count / scan / write pack that ships (it was not written).

    python tools/ckpt_bench.py [--repeats R] [--levels L] [--table SLOTS] [--dir DIR] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.grow_bench import copy_gbps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--levels", type=int, default=26)   # (level 25 is the widest: 24.5 M of 146.9 M states stored by then)
    ap.add_argument("--table", type=int, default=1 << 28)
    ap.add_argument("--frontier", type=int, default=1 << 26)
    ap.add_argument("--start", type=int, default=1 << 24)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_checkpoint.json"))
    a = ap.parse_args()
    import kafka_specification_amd as kmc
    from kafka_specification_amd.configs import HEADLINE
    tmp = tempfile.TemporaryDirectory(dir=a.dir)
    path = {k: os.path.join(tmp.name, k + ".ckpt") for k in ("classic", "compact", "grown_classic", "grown_compact")}

    os.environ["KMC_VERBOSE"] = "1"   # (read when a handle is opened)

    def timed(f):
        """wall milliseconds of f() and the library's own split of them: its stderr (descriptor 2) read back"""
        with tempfile.TemporaryFile() as err:
            keep = os.dup(2)
            os.dup2(err.fileno(), 2)
            try:
                t0 = time.perf_counter()
                f()
                wall = (time.perf_counter() - t0) * 1e3
            finally:
                os.dup2(keep, 2)
                os.close(keep)
            err.seek(0)
            m = re.findall(r"checkpoint (?:save|load) \(\w+\): ([\d.]+) ms in all; kernels ([\d.]+) ms, device <-> host copies ([\d.]+) ms, "
                           r"file I/O ([\d.]+) ms", err.read().decode("utf-8", "replace"))
        assert len(m) == 1, m
        return dict(wall=wall, kernels=float(m[0][1]), copies=float(m[0][2]), file_io=float(m[0][3]))

    def stats(recs):
        out = {}
        for k in recs[0]:
            ms = sorted(r[k] for r in recs)
            out[k + "_ms"] = dict(median=statistics.median(ms), min=ms[0], max=ms[-1])
        return out

    # -- save: one handle per source, both formats in turn
    report = dict(tool="tools/ckpt_bench.py", binding=HEADLINE, levels=a.levels, repeats=a.repeats, pack="count / scan / write (three launches per stretch)",
                  pack_rejected="none: the one-pass decoupled look-back was not built, so no variant was measured against the one that ships",
                  sources={}, loads={})
    sample = {}
    for src, kw, grow in (("fixed", dict(table_capacity=a.table), False), ("grown", dict(table_capacity=a.start), True)):
        with kmc.ModelChecker(kmc.CheckerConfig(**HEADLINE, frontier_capacity=a.frontier, max_levels=a.levels, **kw)) as mc:
            if grow:
                mc.enable_table_growth()
            res = mc.run()
            assert res.verdict == "level_limit", res
            names = ("classic", "compact") if src == "fixed" else ("grown_classic", "grown_compact")
            ms = {n: [] for n in names}
            for rep in range(a.repeats + 1):
                for n in names:
                    t = timed(lambda: mc.save_checkpoint(path[n], compact=n.endswith("compact")))
                    if rep:
                        ms[n].append(t)
            sample[src] = mc.frontier_states()[::max(1, res.levels[-1] // 256)]
            report["sources"][src] = dict(table_slots=res.table_capacity, stored=res.orbit_representatives, load=res.orbit_representatives / res.table_capacity,
                                          growths=len(mc.growth_stats()), distinct=res.distinct, generated=res.generated,
                                          files={n: dict(bytes=os.path.getsize(path[n]), save=stats(ms[n])) for n in names})
            print(src, json.dumps(report["sources"][src]["files"]), flush=True)
    saved = report["sources"]["fixed"]

    # -- load: a fresh handle per arm and round (opening and closing it is not timed)
    arms = [("classic", "classic", a.table, {}), ("compact", "compact", a.table, {}), ("compact_smaller", "compact", -(-int(saved["stored"] / 0.8) // 64) * 64, {}),
            ("compact_times4", "compact", a.table * 4, {})]
    arms += [(f"compact_window_{k}k", "compact", a.table, {"KMC_REHASH": "window", "KMC_REHASH_WINDOW_KIB": str(k)}) for k in (16, 32, 64)]
    arms += [("compact_scatter", "compact", a.table, {"KMC_REHASH": "scatter"})]
    arms = [x for x in arms if saved["stored"] <= 0.9 * x[2]]
    ms = {x[0]: [] for x in arms}
    for rep in range(a.repeats + 1):
        for name, which, cap, env in arms:
            os.environ.update(env)
            with kmc.ModelChecker(kmc.CheckerConfig(**HEADLINE, table_capacity=cap, frontier_capacity=a.frontier)) as mc:
                if env:
                    mc.enable_table_growth(cap)
                t = timed(lambda: mc.load_checkpoint(path[which]))
                at = mc.result()
                assert (at.distinct, at.generated) == (saved["distinct"], saved["generated"]) and all(mc.contains(r) for r in sample["fixed"]), name
            for k in env:
                os.environ.pop(k)
            if rep:
                ms[name].append(t)
            print(rep, name, f"{t['wall']:.1f} ms", flush=True)
    for name, which, cap, env in arms:
        report["loads"][name] = dict(file=which, table_slots=cap, load=stats(ms[name]))
    nbytes = 8 * saved["stored"] + 8 * a.table   # entries in, table out (the headline's entries are one word)
    report["device_copy_of_the_same_bytes"] = dict(bytes=nbytes, gbytes_per_s=copy_gbps(nbytes))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))


if __name__ == "__main__":
    main()
