"""`tlc2.TLC`-shaped command line [TLC-recall]:

    python -m kafka_specification_amd.tlc [-config X.cfg] [-deadlock] [-continue] [-workers N]
                                          [-fp SEED] [-fp128] [-symmetry] [-fpcheck] [-verify] [-force] [-levels-csv FILE] [-gpus P] [-table SLOTS]
                                          [-frontier STATES] [-walks N [-walk-depth D] [-walk-seed S]] Spec.tla

Maps the root module's name to its lowered GPU model, reads constants / invariants from the
.cfg (default: Spec.cfg next to the module), runs the exhaustive search on the GPU and prints
TLC-style progress and summary lines.  -workers is accepted for command-line compatibility
and ignored (the GPU's waves are the workers).  No TLA+ is parsed: only the modules of
hachikuji/kafka-specification that have a Next are known — so the spec file given on the command line (and
every module it EXTENDS / INSTANCEs, when found beside it) is hashed against the revision the kernels were
lowered from (spec_revision.py); an edited spec is refused unless -force.

-walks N runs N random walks from Init instead of the search (random simulation, one GPU; -walk-depth D states per walk at
the most, default 100; -walk-seed S, default 0).  Stock TLC's -simulate / -depth / -seed spellings stay refused.

The seen-set holds 64-bit fingerprints, like TLC's FPSet: two distinct states with one fingerprint lose a state
silently.  Like TLC, the summary prints the estimated probability of that; -fpcheck runs the search a second
time with another fingerprint seed and compares the counts (a collision moves with the seed).
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

from . import _native as nat
from .cfg import CfgError, parse_cfg, to_checker_config
from .checker import ModelChecker
from .format import format_state


def _now():
    return time.strftime("%Y-%m-%d %H:%M:%S")


def _collision(distinct, generated, representatives, wide, finished_ok):
    """(lines, exit status or 0) of the library's kmc_collision_report (include/kmc.h): TLC's closing estimate, the advice to
    use -fp128 above FP128_ADVICE_ABOVE, and the warning with UNCERTIFIED_EXIT_CODE for a finished search above it."""
    out = C.create_string_buffer(2048)
    rc = nat.lib().kmc_collision_report(distinct, generated, representatives, int(wide), int(finished_ok), out, len(out))
    return out.value.decode().splitlines(), rc


def collision_report(distinct: int, generated: int, wide: bool = False):
    return _collision(distinct, generated, 0, wide, False)[0]


def uncertified(distinct: int, wide: bool) -> bool:
    """A finished 64-bit search whose birthday bound exceeds FP128_ADVICE_ABOVE: its distinct-state count is more likely to be
    off than not (BASELINE's target is the bit-identical count) — both front ends then exit with UNCERTIFIED_EXIT_CODE."""
    return _collision(distinct, distinct, 0, wide, True)[1] != 0


def __getattr__(name):
    """UNCERTIFIED_EXIT_CODE, FP128_ADVICE_ABOVE: the library's numbers (include/kmc.h), read when first asked for."""
    if name in ("UNCERTIFIED_EXIT_CODE", "FP128_ADVICE_ABOVE"):
        above = C.c_double()
        code = nat.lib().kmc_uncertified_policy(C.byref(above))
        return code if name == "UNCERTIFIED_EXIT_CODE" else above.value
    raise AttributeError(name)


def _run_walks(cc, sim, module) -> int:
    """-walks: a batch of random walks instead of the search; the report's lines are the library's (kmc_sim_report)."""
    native_cfg = cc.to_native()

    n_actions = nat.lib().kmc_action_count(native_cfg.model)
    names = (C.c_char_p * n_actions)(*[nat.lib().kmc_action_name(native_cfg.model, k) for k in range(n_actions)])

    def report(res, closing):
        out = C.create_string_buffer(4096)
        nat.lib().kmc_sim_report(C.byref(native_cfg), C.byref(sim), None if res is None else C.byref(res), closing, names,
                                 n_actions, out, len(out))
        return out.value.decode()
    print(report(None, 0))
    try:
        with ModelChecker(cc) as mc:
            r = nat.KmcSimResult()
            nat.check(nat.lib().kmc_simulate(mc.handle, C.byref(sim), C.byref(r)))
            rc = 0
            if r.verdict == 0:
                print("Random simulation completed. No error has been found.")
            else:
                if r.verdict == 1:
                    where = " by the initial state" if r.violation_step == 0 else ""
                    print(f"Error: Invariant {nat.invariant_names(cc.model)[r.violated_invariant]} is violated{where}.")
                else:
                    print("Error: Deadlock reached.")
                rc = 12 if r.verdict == 1 else 11
                behaviour = mc.walk(int(r.violation_walk), depth=int(sim.depth), seed=int(sim.seed))
                print(f"Error: The behavior up to this point is (walk {r.violation_walk}):")
                for k, (act, st, _choice, _n) in enumerate(behaviour, 1):
                    print(f"State {k}: " + ("<Initial predicate>" if act is None else f"<{act} of module {module}>"))
                    print(format_state(cc, st))
                    print()
            print(report(r, 1))
            steps = (r.states_generated - r.walks) / max(r.seconds_kernel, 1e-9)
            print(f"Finished in {r.seconds_total:.3f}s ({steps:.0f} steps/s in the simulate kernel, {r.seconds_kernel:.3f}s) at ({_now()})")
            return rc
    except nat.KmcError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 3


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="tlc", add_help=True, prefix_chars="-")
    ap.add_argument("spec")
    ap.add_argument("-config", default=None)
    ap.add_argument("-deadlock", action="store_true", help="do NOT check for deadlock (TLC semantics of -deadlock)")
    ap.add_argument("-continue", dest="cont", action="store_true")
    ap.add_argument("-workers", default="1")
    ap.add_argument("-fp", type=int, default=0)
    ap.add_argument("-gpus", type=int, default=1, help="P > 1: P logical shards on this process's GPU (loopback).  Real "
                    "multi-GPU runs: `python -m torch.distributed.run --nproc-per-node P -m kafka_specification_amd.tlc ...` "
                    "— one rank per GPU, the fingerprint space sharded over the ranks, rank 0 prints")
    ap.add_argument("-table", type=int, default=0)
    ap.add_argument("-frontier", type=int, default=0)
    ap.add_argument("-device", type=int, default=0)
    ap.add_argument("-notrace", action="store_true", help="do not keep predecessor links (no counterexample trace)")
    ap.add_argument("-levels-csv", dest="levels_csv", default=None, metavar="FILE",
                    help="write one line per BFS level (one GPU): frontier expanded, new states, probes, deadlocks, table load, "
                         "k_expand milliseconds, successors generated per disjunct of Next")
    ap.add_argument("-fp128", action="store_true",
                    help="128-bit seen-set entries: the fingerprint plus an independent 64-bit check word per state, in the same "
                         "cache line (no extra memory traffic per probe, twice the table bytes); a 64-bit fingerprint collision "
                         "is then recognised instead of losing a state")
    ap.add_argument("-symmetry", action="store_true",
                    help="orbit counting: the specs never tell two members of Replicas apart, so one state per orbit of the "
                         "permutations of Replicas is stored and expanded and every count is weighted by its orbit's size — the "
                         "numbers printed are those of the plain search (TLC without a SYMMETRY set; TLC's own SYMMETRY prints "
                         "the reduced counts) from ~1/|Replicas|! of the work.  Kafka family / FiniteReplicatedLog, up to 7 "
                         "replicas, one GPU")
    ap.add_argument("-fpcheck", action="store_true",
                    help="run the search again with a second fingerprint seed and compare the counts")
    ap.add_argument("-maxlevels", type=int, default=0, help="stop after this many BFS levels (verdict level_limit)")
    ap.add_argument("-checkpoint", default=None, metavar="DIR",
                    help="with -gpus P / torch.distributed.run and -maxlevels: every shard saves its table and frontier "
                         "there when the level limit is reached (TLC -checkpoint for a sharded search)")
    ap.add_argument("-recover", default=None, metavar="DIR", help="continue a sharded search from such a directory")
    ap.add_argument("-verify", action="store_true",
                    help="differential self-check: a second, differently compiled build of the kernels regenerates every "
                         "level and the per-action / deadlock / violation counts must agree (for constants no oracle reaches)")
    ap.add_argument("-force", action="store_true", help="check the built-in lowering although the spec text differs from it")
    # (text, not numbers: what the three mean and what is wrong with them is the library's kmc_walk_switches, as for the native CLI)
    ap.add_argument("-walks", default=None, metavar="N", help="random simulation: N random walks from Init instead of the search")
    ap.add_argument("-walk-depth", dest="walk_depth", default=None, metavar="D", help="states per walk at the most (100)")
    ap.add_argument("-walk-seed", dest="walk_seed", default=None, metavar="S", help="seed of the walks (0)")
    ap.add_argument("-v", action="store_true", dest="verbose",
                    help="one more closing line: where the wall time outside the search went (HIP start-up, code object, allocation, "
                         "first touch of the seen-set: kmc_timing)")
    # Stock TLC's other command-line switches [TLC-recall]: the ones that do not change what is checked are accepted and
    # ignored with a note (a wrapper script written for `java tlc2.TLC` keeps working); the ones that ask for another mode
    # of operation are refused — silently dropping them would answer a different question than the one asked.
    # Which is which, and why: the library's kmc_tlc_switch.
    argv = list(sys.argv[1:] if argv is None else argv)
    kept, i = [], 0
    while i < len(argv):
        t = argv[i]
        kind = C.c_int32()
        why = (nat.lib().kmc_tlc_switch(t.encode(), C.byref(kind)) or b"").decode()
        if kind.value == nat.KMC_SWITCH_IGNORED:
            print(f"Note: {t} is accepted for compatibility and ignored ({why})", file=sys.stderr)
        elif kind.value == nat.KMC_SWITCH_IGNORED_VALUE:
            print(f"Note: {t} {argv[i + 1] if i + 1 < len(argv) else ''} is accepted for compatibility and ignored "
                  f"({why})", file=sys.stderr)
            i += 1
        elif kind.value == nat.KMC_SWITCH_REFUSED:
            print(f"Error: {t} is not supported: {why}", file=sys.stderr)
            if t == "-simulate":
                print("Note: -walks N [-walk-depth D] [-walk-seed S] runs N random walks from Init", file=sys.stderr)
            return 2
        elif (t == "-checkpoint" and i + 1 < len(argv) and argv[i + 1].lstrip("-").isdigit()
              and not os.path.isdir(argv[i + 1])):
            # TLC's -checkpoint takes an interval in minutes; here a search takes milliseconds to seconds and -checkpoint DIR
            # names where a level-limited sharded search leaves its state (a directory that exists under a numeric name is
            # a directory; to CREATE one with a numeric name say ./2024)
            print(f"Note: -checkpoint {argv[i + 1]} (TLC's interval in minutes) is accepted and ignored; "
                  "-checkpoint DIR saves a level-limited sharded search", file=sys.stderr)
            i += 1
        else:
            kept.append(t)
        i += 1
    a = ap.parse_args(kept)
    sim, walk_mode = nat.KmcSimConfig(), C.c_int32()
    enc = lambda v: None if v is None else str(v).encode()   # noqa: E731
    if nat.lib().kmc_walk_switches(enc(a.walks), enc(a.walk_depth), enc(a.walk_seed), C.byref(sim), C.byref(walk_mode)) != 0:
        print(f"Error: {nat.lib().kmc_last_error().decode()}", file=sys.stderr)
        return 2

    module = os.path.splitext(os.path.basename(a.spec))[0]
    cfg_path = a.config or os.path.splitext(a.spec)[0] + ".cfg"
    if not os.path.exists(cfg_path):
        print(f"Error: configuration file {cfg_path} not found", file=sys.stderr)
        return 2
    try:
        mcfg = parse_cfg(open(cfg_path).read())
        over = dict(hash_seed=a.fp, device=a.device, continue_on_violation=a.cont, keep_trace=not a.notrace,
                    table_capacity=a.table, frontier_capacity=a.frontier, max_levels=a.maxlevels,
                    wide_fingerprint=a.fp128, symmetry=a.symmetry)
        if a.deadlock:
            over["check_deadlock"] = False
        cc = to_checker_config(module, mcfg, **over)
    except CfgError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 2

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        # launched by torch.distributed.run: one shard per rank (RCCL over xGMI, the exchange under the C ABI);
        # every rank computes the same global result, rank 0 reports it
        import torch
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if not dist.is_initialized():
            dist.init_process_group(backend=os.environ.get("KMC_BACKEND", "nccl"))
        if dist.get_backend() == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))
        if rank != 0:
            sys.stdout = open(os.devnull, "w")

    if a.verify:
        os.environ["KMC_VERIFY"] = "1"
    from .spec_revision import check_spec
    status, msgs = check_spec(a.spec)
    for m in msgs:
        print(("Warning: " if status != "mismatch" else "Error: ") + m, file=sys.stderr)
    if status == "mismatch":
        if not a.force:
            print("Error: the spec differs from the revision the GPU kernels were lowered from; nothing was checked "
                  "(-force checks the built-in lowering anyway)", file=sys.stderr)
            return 2
        print("Warning: -force: checking the BUILT-IN lowering, not the text of the spec given", file=sys.stderr)

    print(f"kafka_specification_amd model checker (MI355X) — module {module}, config {os.path.basename(cfg_path)}")
    if walk_mode.value:
        return _run_walks(cc, sim, module)
    print(f"Running breadth-first search Model-Checking with fp seed {a.fp} on GPU {a.device}.")
    print("Computing initial states...")

    def progress(i):
        if i["depth"] == 1:
            print(f"Finished computing initial states: {i['distinct']} distinct state generated at {_now()}.")
        else:
            print(f"Progress({i['depth']}) at {_now()}: {i['generated']} states generated, "
                  f"{i['distinct']} distinct states found, {i['new_states']} states left on queue.")

    from dataclasses import replace

    def search(conf, progress):
        if world > 1:
            from .sharded import check_distributed
            res = check_distributed(conf, progress, a.checkpoint, a.recover)
            return res, res.trace
        if a.gpus > 1:
            from .sharded import check_loopback
            res = check_loopback(conf, a.gpus, a.device, progress, a.checkpoint, a.recover)
            return res, res.trace   # walked owner by owner through the shards' predecessor tables
        with ModelChecker(conf) as mc:
            res = mc.run(progress)
            timing.update(mc.timing())
            nonlocal level_rows
            level_rows = mc.level_stats()
            trace = []
            if res.verdict in ("invariant",) and conf.keep_trace:
                trace = mc.trace()
            elif res.verdict == "deadlock":
                trace = [(None, mc.unpack(mc.witness()))]
            return res, trace

    second = None
    timing = {}
    level_rows = None   # -levels-csv: the per-expansion records of the search on one GPU (kmc_level_stats)
    try:
        res, trace = search(cc, progress)
        if a.fpcheck:
            seed2 = (a.fp * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D) & 0xFFFFFFFFFFFFFFFF
            second, _ = search(replace(cc, hash_seed=seed2, keep_trace=False), None)
            second = (seed2, second)
    except nat.KmcError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 3

    rc = 0
    if res.verdict == "ok":
        print("Model checking completed. No error has been found.")
    elif res.verdict == "invariant":
        where = " by the initial state" if res.violation_depth == 1 else ""
        print(f"Error: Invariant {res.violated_invariant} is violated{where}.")
        rc = 12
    elif res.verdict == "deadlock":
        print("Error: Deadlock reached.")
        rc = 11
    else:
        print(f"Error: search stopped: {res.verdict} (table {res.table_capacity} slots, "
              f"frontier {res.frontier_capacity} states)")
        rc = 1
    if trace:
        print("Error: The behavior up to this point is:")
        for k, (act, st) in enumerate(trace, 1):
            head = "<Initial predicate>" if act is None and k == 1 else f"<{act} of module {module}>"
            print(f"State {k}: {head}")
            print(format_state(cc, st))
            print()
    print(f"{res.generated} states generated, {res.distinct} distinct states found, "
          f"{res.queue_left} states left on queue.")
    print(f"The depth of the complete state graph search is {res.depth}.")
    if a.symmetry:
        print(f"Symmetry reduction (orbit counting over the permutations of Replicas): {res.orbit_representatives} states "
              f"were stored and expanded, one per orbit; every count above is the plain search's.")
    lines, uncertified_rc = _collision(res.distinct, res.generated, res.orbit_representatives if a.symmetry else 0, a.fp128, rc == 0)
    print("\n".join(lines))
    rc = uncertified_rc or rc
    if a.levels_csv and level_rows is not None:
        names = list(res.action_generated)
        with open(a.levels_csv, "w") as lf:
            lf.write("depth,frontier,new_states,stored_new,probes,deadlocks,table_load,expand_ms," + ",".join(names) + "\n")
            for st in level_rows:
                lf.write(f"{st['depth']},{st['frontier']},{st['new_states']},{st['stored_new']},{st['probes']},{st['deadlocks']},"
                         f"{st['table_load']:.6f},{st['expand_ms']:.4f}," + ",".join(str(st['generated'][n]) for n in names) + "\n")
    if second is not None:
        seed2, r2 = second
        same = (r2.verdict, r2.distinct, r2.generated, r2.depth) == (res.verdict, res.distinct, res.generated, res.depth)
        print(f"Fingerprint check: second run with fp seed {seed2}: {r2.generated} states generated, {r2.distinct} distinct "
              f"states found, depth {r2.depth} - " + ("identical to the first run." if same else
              "DIFFERENT from the first run: a fingerprint collision dropped states in at least one of them "
              "(a collision can only lose states: the larger count is the better lower bound)."))
        if not same and rc == 0:
            rc = 13
    print(f"Finished in {res.seconds_total:.3f}s ({res.distinct / max(res.seconds_total, 1e-9):,.0f} distinct states/s; "
          f"{res.seconds_expand:.3f}s in the expand kernel) at ({_now()})")
    if a.verbose and timing:
        print(f"Wall time outside the search: kmc_open {timing['open_s']:.3f}s (HIP initialisation {timing['hip_init_s']:.3f}s, code "
              f"object {timing['code_object_s']:.3f}s, allocation of {timing['device_bytes'] / 2 ** 30:.1f} GiB {timing['alloc_s']:.3f}s), "
              f"first clear of the seen-set {timing['first_clear_s']:.3f}s")
    return rc


if __name__ == "__main__":
    sys.exit(main())
