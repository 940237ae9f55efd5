"""k_simulate_from (ModelChecker.simulate / walk with starts=...) on the GPU: k_simulate's walks when started on Init, under every
refill threshold; walks from a frontier, verdicts and witnesses against a lock-step reference walker over successors_batch
and sim_draw; refusals; the seen-set left alone.  Shapes are test_gpu_simulate.py's: 4,096 + 37 walks of depth 48 in launches
of 1,024 — 17 chunks of 256 walkers, the last one partial, on few waves, so that every wave refills through several chunks."""
import dataclasses

import numpy as np
import pytest

from kafka_specification_amd import CheckerConfig, KmcError, ModelChecker
from kafka_specification_amd.checker import sim_draw
from test_gpu_simulate import BINDINGS, DEPTH, MODEL_NAMES, N_WALKS, SEED, SMALL, WPL, consts, layout, open_checker

pytestmark = pytest.mark.gpu
INV3 = ("TypeOk", "WeakIsr", "StrongIsr")
TRUNCATE = (2, 3, 2, 2, 2, 0, 0)   # KafkaTruncateToHighWatermark 3/2/2/2: walks of it reach a WeakIsr violation
_from_init = {}


def frontier(c):
    """the first BFS level of more than 256 states, invariants off; never a multiple of 64 states"""
    for lv in range(1, 40):
        with layout(c), ModelChecker(CheckerConfig(model=MODEL_NAMES[c[0]], **consts(c), table_capacity=1 << 20, frontier_capacity=1 << 16,
                                                   invariants=(), max_levels=lv)) as mc:
            assert mc.run().verdict == "level_limit"
            f = mc.frontier_states()
        if len(f) > 256:
            return f[:-1] if len(f) % 64 == 0 else f
    raise AssertionError("no level of more than 256 states")


def reference(mc, starts, first, n_walks, inv_mask=0, depth=DEPTH, seed=SEED):
    """The walks first .. first + n_walks - 1 in lock step, one successors_batch call per step.
    -> {w: [(kind, words, r, n)]}, {w: ("invariant", bits) | ("stuck", 0) | ("depth", 0)}"""
    W = mc.state_words
    walks = {w: [(-1, tuple(int(x) for x in starts[w % len(starts)]), 0, 0)] for w in range(first, first + n_walks)}
    live, end = sorted(walks), {}
    for t in range(depth):
        offsets, records, violated = mc.successors_batch(np.array([walks[w][-1][1] for w in live], dtype=np.uint64), inv_mask)
        still = []
        for i, w in enumerate(live):
            n = int(offsets[i + 1]) - int(offsets[i])
            if violated[i]:
                end[w] = ("invariant", int(violated[i]))
            elif t + 1 >= depth:
                end[w] = ("depth", 0)
            elif n == 0:
                end[w] = ("stuck", 0)
            else:
                r = sim_draw(seed, w, t, n)
                row = records[int(offsets[i]) + r]
                walks[w].append((int(row[W + 1]), tuple(int(x) for x in row[:W]), r, n))
                still.append(w)
        live = still
    return walks, end


def as_walk(mc, ref_walk, canon):
    """a reference walk in the form ModelChecker.walk returns"""
    names = mc.action_names()
    canon.update({s: mc.unpack(s) for (_k, s, _r, _n) in ref_walk if s not in canon})
    return [(None if k < 0 else names[k], canon[s], r, n) for (k, s, r, n) in ref_walk]


def verdict_of(end, walks, n_walks, stop="invariant"):
    """(launches, verdict, lowest violated bit, witness walk, witness step) of a batch from walk 0 that stops at its first verdict"""
    for launch, lo in enumerate(range(0, n_walks, WPL)):
        hits = [w for w in range(lo, min(lo + WPL, n_walks)) if end[w][0] == stop]
        if hits:
            bits = end[hits[0]][1]
            return launch + 1, stop, (bits & -bits).bit_length() - 1, hits[0], len(walks[hits[0]]) - 1
    return -(-n_walks // WPL), "ok", -1, 0, 0


def init_batches(bid):
    """k_simulate's recorded batch of a binding, computed once: its result, its walks, the packed Init"""
    if bid not in _from_init:
        with open_checker(BINDINGS[bid], invariants=()) as mc:
            res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, record=True)
            walks = [mc.walk(w, depth=DEPTH, seed=SEED) for w in range(N_WALKS)]
            _from_init[bid] = (res, walks, np.array([mc.pack(walks[0][0][1])], dtype=np.uint64))
    return _from_init[bid]


@pytest.mark.parametrize("bid,refill", [(b, None) for b in ("Kip320-3-2-2-1", "Kip279-3-2-2-2", "Kip320-7-1-1-0", "FiniteReplicatedLog-2-4-2")] +
                         [("Kip320-3-2-2-1", n) for n in (1, 16, 64)])
def test_started_on_init_the_walks_are_k_simulates(bid, refill, monkeypatch):
    want, want_walks, init = init_batches(bid)
    if refill is not None:   # (read when the handle is opened)
        monkeypatch.setenv("KMC_JIT_DEFINES", f"-DKMC_SIM_REFILL_MIN={refill}")
    with open_checker(BINDINGS[bid], invariants=()) as mc:
        monkeypatch.delenv("KMC_JIT_DEFINES", raising=False)
        got = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, record=True, starts=init)
        assert dataclasses.replace(got, seconds_total=0, seconds_kernel=0) == dataclasses.replace(want, seconds_total=0, seconds_kernel=0)
        assert got.launches == 5 and got.states_generated > N_WALKS
        for w in range(N_WALKS):
            assert mc.walk(w, depth=DEPTH, seed=SEED, starts=init) == want_walks[w], f"walk {w}"
        # a recorded from-batch is not k_simulate's batch, nor the other way round: both calls re-run, and agree
        assert mc.walk(7, depth=DEPTH, seed=SEED) == want_walks[7]
        mc.simulate(64, depth=DEPTH, seed=SEED, record=True)
        assert mc.walk(7, depth=DEPTH, seed=SEED, starts=init) == want_walks[7]


@pytest.mark.parametrize("bid", ["Kip320-3-2-2-1", "Kip279-3-2-2-2"])
def test_walks_from_a_frontier_against_the_reference(bid):
    c = BINDINGS[bid]
    starts = frontier(c)
    first = 1000   # (the mapping walk -> row is offset, and wraps)
    assert 256 < len(starts) < N_WALKS and len(starts) % 64
    with open_checker(c, invariants=()) as mc:
        walks, end = reference(mc, starts, first, N_WALKS + 1)
        res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, first_walk=first, walks_per_launch=WPL, record=True, starts=starts)
        canon = {}
        for w in range(first, first + N_WALKS):
            assert mc.walk(w, depth=DEPTH, seed=SEED, starts=starts) == as_walk(mc, walks[w], canon), f"walk {w}"
        outside = first + N_WALKS   # not in the recorded batch: re-run from its own row
        assert mc.walk(outside, depth=DEPTH, seed=SEED, starts=starts) == as_walk(mc, walks[outside], canon)
        del walks[outside]
        kinds = [k for wk in walks.values() for (k, _s, _r, _n) in wk[1:]]
        assert res.states_generated == sum(len(wk) for wk in walks.values())
        assert res.action_taken == {name: kinds.count(k) for k, name in enumerate(mc.action_names())}
        assert res.ended_early == sum(end[w][0] == "stuck" for w in walks) > 0
        assert res.longest_walk == max(len(wk) for wk in walks.values())
        assert (res.launches, res.walks, res.verdict) == (5, N_WALKS, "ok")
        assert min(len(wk) for wk in walks.values()) < DEPTH // 2   # (walks of uneven length: lanes were refilled mid-chunk)


def test_verdicts_against_the_reference():
    starts = frontier(TRUNCATE)
    with open_checker(TRUNCATE, invariants=()) as mc:
        walks, end = reference(mc, starts, 0, N_WALKS, inv_mask=7)
    want = verdict_of(end, walks, N_WALKS)
    assert want[1] == "invariant"
    with open_checker(TRUNCATE, invariants=INV3) as mc:
        res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, starts=starts)
        assert (res.launches, res.verdict, res.violated_invariant, res.violation_walk, res.violation_step) == \
            (want[0], "invariant", INV3[want[2]], want[3], want[4])
        bad = np.array([walks[want[3]][-1][1]], dtype=np.uint64)   # a violating state as a start state: the walk ends on s_0
        at0 = mc.simulate(8, depth=DEPTH, seed=SEED, starts=np.concatenate([bad, starts[:5]]))
        assert (at0.verdict, at0.violation_walk, at0.violation_step) == ("invariant", 0, 0)
    with open_checker(TRUNCATE, invariants=INV3, continue_on_violation=True) as mc:
        res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, starts=starts)
        counts = {name: sum(e[0] == "invariant" and e[1] >> k & 1 for e in end.values()) for k, name in enumerate(INV3)}
        assert {k: res.violation_count[k] for k in INV3} == counts and res.launches == 5
        assert (res.violation_walk, res.violation_step) == (want[3], want[4])
    starts = frontier(BINDINGS["Kip320-3-2-2-1"])
    with open_checker(BINDINGS["Kip320-3-2-2-1"], invariants=(), check_deadlock=True) as mc:
        walks, end = reference(mc, starts, 0, N_WALKS)
        want = verdict_of(end, walks, N_WALKS, stop="stuck")
        assert want[1] == "stuck"
        res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, starts=starts)
        assert (res.launches, res.verdict, res.violation_walk, res.violation_step) == (want[0], "deadlock", want[3], want[4])


def test_refusals_and_the_seen_set_left_alone():
    kip320 = dict(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1)
    one = np.zeros((1, 8), dtype=np.uint64)
    for kw, match, code in [(dict(model="AsyncIsr", n_replicas=3, log_size=2, max_leader_epoch=2, **SMALL), "AsyncIsr", 1),
                            (dict(kip320, symmetry=True, **SMALL), "symmetry", 1), (dict(kip320, device=-1), "host-only", 5)]:
        with ModelChecker(CheckerConfig(**kw)) as mc:
            with pytest.raises(KmcError, match=match) as e:
                mc.simulate(8, starts=one[:, :mc.state_words])
            assert e.value.code == code
    with ModelChecker(CheckerConfig(**kip320, invariants=INV3, table_capacity=1 << 20, frontier_capacity=1 << 16)) as mc:
        W = mc.state_words
        first = mc.run()
        init = np.array([mc.pack(mc.walk(0, depth=1)[0][1])], dtype=np.uint64)
        for kw, match in [(dict(depth=(1 << 20) + 1, starts=init), "depth"), (dict(walks_per_launch=(1 << 24) + 1, starts=init), "walks_per_launch"),
                          (dict(starts=np.zeros((0, W), dtype=np.uint64)), "start states"),
                          (dict(starts=np.zeros(((1 << 27) // W + 1, W), dtype=np.uint64)), "sub-sample"), (dict(n_walks=0, starts=init), "n_walks")]:
            with pytest.raises(KmcError, match=match) as e:
                mc.simulate(**{"n_walks": 8, **kw})
            assert e.value.code == 1
        with pytest.raises(KmcError, match="start states"):
            mc.walk(3, starts=np.zeros((0, W), dtype=np.uint64))
        probes = [init[0], np.array(mc.pack(mc.walk(5, depth=9)[-1][1]), dtype=np.uint64), np.full(W, 0x5555, dtype=np.uint64)]
        before = [mc.contains(p) for p in probes]
        mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, record=True, starts=init)
        ignore = dict(seconds_total=0, seconds_expand=0, seconds_inv=0, seconds_clear=0)
        assert dataclasses.replace(mc.result(), **ignore) == dataclasses.replace(first, **ignore)
        assert [mc.contains(p) for p in probes] == before and before[:2] == [True, True]
        again = mc.run()
        assert (again.verdict, again.distinct, again.generated, again.depth, again.levels) == \
            (first.verdict, first.distinct, first.generated, first.depth, first.levels)
