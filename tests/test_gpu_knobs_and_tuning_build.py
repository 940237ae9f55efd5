"""What the environment may change about a search, and in which library (README: "Environment the library honours" and "Tuning
build"):  libkmc.so reads none of the tuning aids' variables — a search under all of them is the plain chained search;
libkmc_tuning.so on a -DKMC_TUNING=1 code object still runs the dry and shadow passes, and they change no answer; and a handle's
knobs (csrc/kmc_engine_open.cpp: read_knobs) are read when the handle is opened, so two handles of one process follow two values.

Every run is a fresh child process.  All searches run at Kip320 3/2/2/1 with TypeOk, WeakIsr, StrongIsr — 22 levels, so kmc_run
chains more than one batch — against the C oracle.  That configuration holds its invariants and has no counterexample, so the
comparison of TRACES under the two forms of predecessor storage runs on Kip101 at the same constants, which violates one.
"""
import functools
import json
import os
import subprocess
import sys

import pytest

import kmo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING_LIB = os.path.join(ROOT, "kafka_specification_amd", "libkmc_tuning.so")
INV = ("TypeOk", "WeakIsr", "StrongIsr")
AIDS = ("KMC_DRYRUN", "KMC_SHADOW", "KMC_XFLAGS", "KMC_NO_CHAIN", "KMC_CHAIN_MAX", "KMC_BLOCKS_PER_CU")
KNOBS = ("KMC_SEEN_SET_CHUNK_LOG2", "KMC_SEEN_SET_SPREAD", "KMC_PAIRED_SLOTS", "KMC_VERBOSE", "KMC_JIT_DEFINES", "KMC_VERIFY",
         "KMC_LAYOUT", "KMC_LIB_PATH")

# the child: one handle per step, each opened (searched, closed) under the step's changes to the environment
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
from kafka_specification_amd import CheckerConfig, ModelChecker
out = []
for step in json.loads(sys.argv[2]):
    for k, v in step["env"].items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    sys.stderr.write("== handle %d\n" % len(out))
    sys.stderr.flush()
    cfg = CheckerConfig(model=step["model"], n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1,
                        invariants=("TypeOk", "WeakIsr", "StrongIsr"), table_capacity=1 << 20, frontier_capacity=1 << 18,
                        keep_trace=step["keep_trace"])
    with ModelChecker(cfg) as mc:
        r = mc.run()
        tr = mc.trace() if step["keep_trace"] and r.verdict == "invariant" else []
    out.append(dict(verdict=r.verdict, distinct=r.distinct, generated=r.generated, depth=r.depth, levels=r.levels,
                    expand_launches=r.expand_launches, violated_invariant=r.violated_invariant, violation_depth=r.violation_depth,
                    trace_len=len(tr), first=tr[0][1].hex() if tr else None, last=tr[-1][1].hex() if tr else None))
print("RESULT " + json.dumps(out))
"""


def step(env, model="Kip320", keep_trace=False):
    return dict(env=env, model=model, keep_trace=keep_trace)


def child(steps, **env):
    """-> ([result of each step], [what each step's handle wrote to stderr])"""
    base = {k: v for k, v in os.environ.items() if k not in AIDS + KNOBS}
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(steps)], capture_output=True, text=True, cwd=ROOT,
                       env=dict(base, **env), timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    results = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    said = r.stderr.split("== handle ")[1:]
    assert len(results) == len(said) == len(steps)
    return results, said


@functools.lru_cache(maxsize=None)
def oracle(model):
    return kmo.Run(kmo.make_config(model, N=3, L=2, R=2, E=1, invariants=INV))


def is_the_oracles(r):
    o = oracle("Kip320")
    assert o.verdict == "ok"
    return (r["verdict"], r["distinct"], r["generated"], r["depth"], r["levels"]) == (o.verdict, o.distinct, o.generated, o.depth, o.levels)


def test_the_shipped_library_ignores_the_tuning_aids():
    """libkmc.so under every aid at once: the oracle's search, as many launches as with none of them set (the chain was kept:
    KMC_NO_CHAIN / KMC_CHAIN_MAX=1 / KMC_DRYRUN would make it one launch and one wait per level), no dry pass reported.  (Before
    the aids left the library this run ended in "k_expand's dry mode is only compiled into a tuning build".)"""
    (plain,), _ = child([step({})])
    (aided,), (said,) = child([step({})], KMC_DRYRUN="1", KMC_SHADOW="1", KMC_NO_CHAIN="1", KMC_CHAIN_MAX="1", KMC_BLOCKS_PER_CU="1")
    print(plain["expand_launches"], aided["expand_launches"])
    assert is_the_oracles(plain) and is_the_oracles(aided), (plain, aided)
    assert aided["expand_launches"] == plain["expand_launches"]
    assert "dry/shadow" not in said, said[-1500:]


@pytest.mark.parametrize("aid, keep_trace", [
    ({"KMC_DRYRUN": "1"}, False),                        # no table access
    ({"KMC_DRYRUN": "2"}, False),                        # + read-only probes
    ({"KMC_SHADOW": "1", "KMC_XFLAGS": "0"}, True),      # paired slots: the shadow pass's predecessors lie in the copy
    ({"KMC_SHADOW": "1", "KMC_XFLAGS": "0"}, False),
])
def test_the_tuning_build_runs_its_passes_and_changes_no_answer(aid, keep_trace):
    """Both halves of a tuning build — libkmc_tuning.so through KMC_LIB_PATH, the dry kernel through KMC_JIT_DEFINES — with a
    dry or a shadow pass beside every level: the counts are the oracle's and the pass reports its time once, at the end of the
    search.  (No KMC_FLAG_X_* ablation is set: those change what the kernel does.)"""
    (r,), (said,) = child([step({}, keep_trace=keep_trace)], KMC_LIB_PATH=TUNING_LIB, KMC_JIT_DEFINES="-DKMC_TUNING=1", **aid)
    assert is_the_oracles(r), r
    assert said.count("[kmc] dry/shadow expand:") == 1, said[-1500:]
    assert r["expand_launches"] == r["depth"]            # level by level: one launch per level, the last one's finds nothing new


def test_the_seen_set_chunk_is_a_knob_of_the_handle_not_of_the_process():
    """Two handles of one process: the first opened under KMC_SEEN_SET_CHUNK_LOG2=0 gets one hipMalloc, the second — the variable
    unset by then — its chunks.  (While the value sat in a function-local static, the first one stuck.)"""
    results, said = child([step({"KMC_SEEN_SET_CHUNK_LOG2": "0"}), step({"KMC_SEEN_SET_CHUNK_LOG2": None})], KMC_VERBOSE="1")
    assert "(one hipMalloc)" in said[0] and "(mapped from chunks)" not in said[0], said[0][-1500:]
    assert "(mapped from chunks)" in said[1] and "(one hipMalloc)" not in said[1], said[1][-1500:]
    assert all(is_the_oracles(r) for r in results), results


def test_the_paired_slots_are_a_knob_of_the_handle_not_of_the_process():
    """Four trace-keeping handles of one process, KMC_PAIRED_SLOTS=0 / unset / 0 / unset: 8-byte slots with a predecessor table of
    their own, then 16-byte slots of fingerprint + predecessor, and back.  Kip320 gives the oracle's counts either way; Kip101's
    counterexample has the same length, first and last state either way (its middle is whichever parent claimed a state first)."""
    steps = [step({"KMC_PAIRED_SLOTS": v}, model=m, keep_trace=True) for m in ("Kip320", "Kip101") for v in ("0", None)]
    results, said = child(steps, KMC_VERBOSE="1")
    for k, text in enumerate(said):
        assert ("slots x 8 B" if k % 2 == 0 else "slots x 16 B") in text, text[-1500:]
    assert is_the_oracles(results[0]) and is_the_oracles(results[1]), results[:2]
    o = oracle("Kip101")
    assert o.verdict == "invariant"
    for r in results[2:]:
        assert (r["verdict"], r["violated_invariant"], r["violation_depth"]) == ("invariant", o.viol_inv, o.viol_depth), r
    a, b = results[2:]
    assert a["trace_len"] == b["trace_len"] >= 2 and (a["first"], a["last"]) == (b["first"], b["last"]), (a, b)
