"""1. k_expand sends a deadlocked state's fingerprint to the level's control block only for a host that reads it
(kmc_config.check_deadlock -> KMC_FLAG_DEADLOCK_WITNESS, csrc/kmc_common.h).  Without the flag such a state is counted and
nothing else, so:
  - a search with CHECK_DEADLOCK FALSE must still report every count of the oracle, deadlock_states among them, on the
    chained launch path (no progress callback) and on the level-by-level one (with a callback), plain and under orbit counting;
  - a search with CHECK_DEADLOCK TRUE must report the witness it always reported: the deadlocked state of the first deadlocked
    level with the smallest fingerprint — the same on both launch paths and on every run of a handle — and that state must
    have no successor.
2. kmc_run without a progress callback queues its launches in chains of CHAIN = 16 and looks at the counts once per chain
(csrc/kmc_engine_run.cpp).  Whatever ends a search — the last level, a level limit, a deadlock with its witness, the seen-set's
load limit — must end it with the same result wherever in a chain, and in which chain, it falls: the level-by-level path (a
progress callback) and the oracle are the references.

Workload of part 1: Kip320, Replicas = {b1, b2}, LogSize 2, MaxRecords 2, MaxLeaderEpoch 1 — 957 distinct states, 1,819 generated,
depth 15, 70 deadlocked states (the C oracle; Oracle-R agrees: tests/golden/oracle_r_ladder.json)."""
import pytest

import kmo
from kafka_specification_amd import CheckerConfig, ModelChecker

pytestmark = pytest.mark.gpu

BINDING = dict(model="Kip320", n_replicas=2, log_size=2, max_records=2, max_leader_epoch=1)
PATHS = ("chained", "level_by_level")


def oracle(check_deadlock):
    return kmo.Run(kmo.make_config("Kip320", N=2, L=2, R=2, E=1, invariants=("TypeOk",), check_deadlock=check_deadlock))


@pytest.fixture(scope="module")
def o_plain():
    o = oracle(False)
    assert (o.verdict, o.distinct, o.generated, o.depth, o.deadlock_states) == ("ok", 957, 1819, 15, 70)
    return o


@pytest.fixture(scope="module")
def o_deadlock():
    o = oracle(True)
    assert o.verdict == "deadlock"
    return o


def search(mc, path):
    return mc.run(progress=(lambda info: None) if path == "level_by_level" else None)


def checker(**kw):
    return ModelChecker(CheckerConfig(**BINDING, invariants=("TypeOk",), table_capacity=1 << 16, frontier_capacity=1 << 12, **kw))


@pytest.mark.parametrize("symmetry", (False, True), ids=("plain", "orbit_counting"))
@pytest.mark.parametrize("path", PATHS)
def test_counts_without_deadlock_checking(o_plain, path, symmetry):
    with checker(check_deadlock=False, symmetry=symmetry) as mc:
        res = search(mc, path)
    o = o_plain
    assert res.verdict == "ok" and res.queue_left == 0
    assert (res.distinct, res.generated, res.depth, res.levels) == (o.distinct, o.generated, o.depth, o.levels)
    assert res.deadlock_states == o.deadlock_states == 70
    assert list(res.action_generated.values()) == o.action_generated[:len(res.action_generated)]
    assert res.expand_launches >= res.depth


@pytest.fixture(scope="module")
def witnesses(o_deadlock):
    """(result, witness words, its successors) of two runs of one handle per launch path, CHECK_DEADLOCK TRUE."""
    out = {}
    for path in PATHS:
        with checker(check_deadlock=True) as mc:
            runs = []
            for _ in range(2):
                res = search(mc, path)
                w = mc.witness()
                runs.append((res, w, mc.successors(w)))
            out[path] = runs
    return out


@pytest.mark.parametrize("path", PATHS)
def test_deadlock_witness(o_deadlock, witnesses, path):
    o = o_deadlock
    for res, w, succ in witnesses[path]:
        assert res.verdict == "deadlock"
        assert res.violation_depth == len(o.levels)      # the oracle stops at its first level that holds a deadlocked state
        assert res.levels == o.levels and res.generated == o.generated and res.deadlock_states == o.deadlock_states
        assert succ == []                                # the device's own Next on the witness: nothing
        assert res.violation_fp != 0


def test_the_witness_is_the_same_on_both_paths_and_on_every_run(witnesses):
    fps = {(res.violation_fp, tuple(w)) for runs in witnesses.values() for res, w, _ in runs}
    assert len(fps) == 1, fps


def test_the_witness_is_the_smallest_fingerprint_among_the_deadlocked_states_of_its_level(o_deadlock, witnesses):
    """What `the same witness as before` means: of the deadlocked states of the first deadlocked level, the one whose
    fingerprint is smallest (the control block keeps the maximum of ~fp).  Every state of that level is asked for its
    successors and its fingerprint through the ABI."""
    res, w, _ = witnesses["chained"][0]
    depth = res.violation_depth
    with checker(check_deadlock=False, max_levels=depth) as mc:
        mc.run()
        rows = [tuple(int(x) for x in row) for row in mc.frontier_states()]
        dead = [row for row in rows if mc.successors(row) == []]
        assert len(rows) == o_deadlock.levels[-1] and dead
        best = min(dead, key=mc.fingerprint)
        assert mc.fingerprint(best) == res.violation_fp and list(best) == w


# ---- chains of launches -----------------------------------------------------------------------------------------------------
CHAIN = 16   # launches per chain (csrc/kmc_engine_internal.h: KMC_CHAIN_DEFAULT)
KIP320_3 = dict(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1)   # 39,619 states, depth 22


@pytest.fixture(scope="module")
def o_kip320_3():
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=2, R=2, E=1, invariants=("TypeOk",), threads=4))
    assert o.depth == 22 and o.depth % CHAIN and o.depth > CHAIN + 2
    return o


def run_paths(binding, **kw):
    out = {}
    for path in PATHS:
        with ModelChecker(CheckerConfig(**binding, invariants=("TypeOk",), **kw)) as mc:
            res = search(mc, path)
            out[path] = (res, mc.witness() if res.verdict in ("deadlock", "invariant") else None)
    return out


def test_a_depth_that_is_no_multiple_of_the_chain(o_kip320_3):
    """22 levels: the search ends inside the second chain, six launches in."""
    o = o_kip320_3
    for path, (res, _) in run_paths(KIP320_3, table_capacity=1 << 20, frontier_capacity=1 << 16).items():
        assert (res.verdict, res.distinct, res.generated, res.depth, res.levels) == ("ok", o.distinct, o.generated, o.depth, o.levels), path
        assert res.deadlock_states == o.deadlock_states and res.queue_left == 0
        assert list(res.action_generated.values()) == o.action_generated[:len(res.action_generated)]
        assert res.expand_launches >= res.depth


@pytest.mark.parametrize("check_deadlock", (False, True), ids=("to_the_end", "deadlock_stop"))
def test_one_state_per_level_ending_in_the_second_chain(check_deadlock):
    """IdSequence at MaxId = CHAIN + 3: 21 levels of one state; the last state has no successor.  With CHECK_DEADLOCK the verdict
    falls in the second chain, and its witness is fetched from a frontier the launches queued behind it must have left alone."""
    M = CHAIN + 3
    o = kmo.Run(kmo.make_config("IdSequence", MaxId=M, check_deadlock=check_deadlock))
    assert o.levels == [1] * (M + 2)
    got = run_paths(dict(model="IdSequence", max_id=M), check_deadlock=check_deadlock, table_capacity=1 << 12, frontier_capacity=1 << 10)
    for path, (res, w) in got.items():
        assert (res.verdict, res.distinct, res.generated, res.depth, res.levels) == (o.verdict, o.distinct, o.generated, o.depth, o.levels), path
        assert res.deadlock_states == o.deadlock_states == 1
        assert res.expand_launches >= res.depth - (1 if check_deadlock else 0)
        if check_deadlock:
            assert res.violation_depth == M + 2
    if check_deadlock:
        (ra, wa), (rb, wb) = got["chained"], got["level_by_level"]
        assert ra.violation_fp == rb.violation_fp != 0 and wa == wb
        with ModelChecker(CheckerConfig(model="IdSequence", max_id=M, table_capacity=1 << 12, frontier_capacity=1 << 10)) as mc:
            assert mc.successors(wa) == [] and mc.fingerprint(wa) == ra.violation_fp


@pytest.mark.parametrize("k", (CHAIN, CHAIN + 1, CHAIN + 2), ids=("before", "at", "after"))
def test_a_level_limit_around_a_chain_boundary(o_kip320_3, k):
    """The first chain expands levels 1 .. 16 and produces level 17: a limit of 17 levels ends exactly with it, 16 one launch
    earlier, 18 one launch into the next chain.  The last level is not expanded and stays on the queue."""
    o = o_kip320_3
    for path, (res, _) in run_paths(KIP320_3, max_levels=k, table_capacity=1 << 20, frontier_capacity=1 << 16).items():
        assert res.verdict == "level_limit" and res.levels == o.levels[:k] and res.depth == k, path
        assert res.distinct == sum(o.levels[:k]) and res.queue_left == o.levels[k - 1]
        assert res.expand_launches >= k - 1


def test_the_load_limit_reached_in_the_second_chain(o_kip320_3):
    """A seen-set of 660 x 64 slots holds 0.92 x 42,240 = 38,860 states before the search ends with table_full; the levels cross that
    with level 19 (39,277 states), behind the first chain; both paths book the same levels and stop there."""
    o = o_kip320_3
    slots = 660 * 64
    limit = int(0.92 * slots)
    crossing = next(d for d in range(1, len(o.levels) + 1) if sum(o.levels[:d]) > limit)
    assert crossing > CHAIN + 1, crossing
    got = run_paths(KIP320_3, table_capacity=slots, frontier_capacity=1 << 16)
    for path, (res, _) in got.items():
        assert res.verdict == "table_full" and res.levels == o.levels[:crossing], (path, res.levels)
        assert res.distinct == sum(o.levels[:crossing]) and res.queue_left == o.levels[crossing - 1]
    assert got["chained"][0].generated == got["level_by_level"][0].generated
