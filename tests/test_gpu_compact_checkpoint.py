"""Compact checkpoints through ModelChecker: a search stopped at a middle level is saved, loaded into a fresh handle of another
size (the saved one, a smaller one that is no power of two, eight times larger, a growing one opened at 1024 slots, a larger
frontier) and resumed; every count at the end is the uninterrupted run's and the C oracle's.  A violating binding's trace is held to
what a trace is (which predecessor a state keeps is decided by a race, in an uninterrupted run too).  The classic file is compared with a
second classic save of the same handle and with the size its layout gives; no file of an earlier revision is kept."""
import contextlib
import ctypes as C
import functools
import math
import os

import pytest

import kmo
from kafka_specification_amd import CheckerConfig, KmcError, ModelChecker
from kafka_specification_amd import _native as nat

pytestmark = pytest.mark.gpu

INV = ("TypeOk", "WeakIsr", "StrongIsr")
FRL = ("FiniteReplicatedLog", dict(n_replicas=2, log_size=4, n_log_records=4), dict(N=2, L=4, K=4), ("TypeOk",))       # 116,281 states
KIP320 = ("Kip320", dict(n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1), dict(N=3, L=2, R=2, E=1), ("TypeOk",))   # 39,619
KTHW = ("KafkaTruncateToHighWatermark", dict(n_replicas=3, log_size=2, max_records=2, max_leader_epoch=2), dict(N=3, L=2, R=2, E=2), INV)   # violates
# what is saved -> (binding, what opens it, environment, words per slot)
MODES = {
    "plain": (FRL, {}, {}, 1),
    "paired": (KTHW, dict(keep_trace=True), {}, 2),
    "predecessors apart": (KTHW, dict(keep_trace=True), {"KMC_PAIRED_SLOTS": "0"}, 1),
    "wide": (KIP320, dict(wide_fingerprint=True), {}, 2),
    "symmetry": (FRL, dict(symmetry=True), {}, 1),
}
SAVED_CAP, FCAP = 1 << 18, 1 << 17
HEADER, COMPACT_HEADER, SEGS, T = 8 + C.sizeof(nat.KmcConfig) + 10 * 8, 32, 8, 8


@functools.lru_cache(maxsize=None)
def oracle(mode):
    b = MODES[mode][0]
    return kmo.Run(kmo.make_config(b[0], **b[2], invariants=b[3], threads=8))


@contextlib.contextmanager
def checker(mode, table_capacity=SAVED_CAP, frontier_capacity=FCAP, grow=False, **kw):
    b, how, env, _ = MODES[mode]
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        with ModelChecker(CheckerConfig(model=b[0], invariants=b[3], table_capacity=table_capacity, frontier_capacity=frontier_capacity,
                                        **b[1], **how, **kw)) as mc:
            if grow:
                mc.enable_table_growth()
            yield mc


def middle(mode, stored_at_most=None):
    """levels searched before saving: past a third of the states (half way to the violation), or while stored_at_most states are stored"""
    o = oracle(mode)
    if stored_at_most:
        return max(k for k in range(1, len(o.levels)) if sum(o.levels[:k]) <= stored_at_most)
    if o.verdict == "invariant":
        return max(2, o.viol_depth // 2)
    return next(k for k in range(len(o.levels)) if sum(o.levels[:k]) > 0.35 * o.distinct) + 1


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """mode -> what a search stopped in the middle left: both files, the result, the frontier"""
    made = {}

    def get(mode, stored_at_most=None):
        if (mode, stored_at_most) not in made:
            d = tmp_path_factory.mktemp("ckpt")
            with checker(mode, max_levels=middle(mode, stored_at_most)) as mc:
                res = mc.run()
                assert res.verdict == "level_limit"
                for name, compact in (("compact", True), ("classic", False), ("classic2", False)):
                    mc.save_checkpoint(str(d / name), compact=compact)
                made[mode, stored_at_most] = dict(dir=d, res=res, frontier=mc.frontier_states(), words=mc.state_words)
        return made[mode, stored_at_most]
    return get


COUNTS = ("verdict", "distinct", "generated", "depth", "levels", "action_generated", "violated_invariant", "violation_depth", "violation_count",
          "deadlock_states", "queue_left", "orbit_representatives", "generated_repeats")


@functools.lru_cache(maxsize=None)
def uninterrupted(mode):
    with checker(mode) as mc:
        return mc.run()


def assert_ends_as_the_oracle(mode, mc, res):
    """every count of the resumed search is the uninterrupted engine run's and the C oracle's (a search is level-synchronous: its
    counts at a violation are as determined as at the end); a state found twice after a bad unpack would show in all of them"""
    o, full = oracle(mode), uninterrupted(mode)
    assert {k: getattr(res, k) for k in COUNTS} == {k: getattr(full, k) for k in COUNTS}
    assert (res.verdict, res.distinct, res.generated, res.depth, res.levels) == (o.verdict, o.distinct, o.generated, o.depth, o.levels)
    assert list(res.action_generated.values()) == o.action_generated[:len(res.action_generated)]
    if o.verdict == "invariant":
        assert (res.violated_invariant, res.violation_depth, res.violation_count) == (o.viol_inv, o.viol_depth, o.viol_count)
        trace = [st for _, st in mc.trace()]
        assert len(trace) == o.viol_depth and trace[0] == o.state(0) and trace[-1] == mc.unpack(mc.witness())
        for a, b in zip(trace, trace[1:]):
            assert b in {mc.unpack(w) for w, _, _ in mc.successors(mc.pack(a))}


def smaller_capacity(mode):
    return math.ceil(oracle(mode).distinct / 0.8 / 64) * 64 + 192   # (holds the whole search; no power of two)


@pytest.mark.parametrize("mode, into", [(m, i) for m in MODES for i in ("saved", "smaller", "eight times")] +
                         [("plain", "larger frontier"), ("wide", "growing")])
def test_resume_in_a_handle_of_another_size(saved, mode, into):
    s = saved(mode, 900 if into == "growing" else None)   # (900: what the growing handle's 1024 slots hold below the load limit)
    cap = {"smaller": smaller_capacity(mode), "eight times": 8 * SAVED_CAP, "growing": 1024}.get(into, SAVED_CAP)
    fcap = 2 * FCAP if into == "larger frontier" else FCAP
    assert cap % 64 == 0 and (into != "smaller" or (cap < SAVED_CAP and cap & (cap - 1)))
    with checker(mode, table_capacity=cap, frontier_capacity=fcap, grow=into == "growing") as mc:
        mc.load_checkpoint(str(s["dir"] / "compact"))
        at = mc.result()
        assert (at.table_capacity, at.frontier_capacity, at.levels, at.generated) == (cap, fcap, s["res"].levels, s["res"].generated)
        rows = mc.frontier_states()
        assert sorted(map(tuple, rows.tolist())) == sorted(map(tuple, s["frontier"].tolist())) and all(mc.contains(r) for r in rows)
        res = mc.resume()
        assert_ends_as_the_oracle(mode, mc, res)
        assert into != "growing" or (len(mc.growth_stats()) >= 1 and res.table_capacity > 1024)


@pytest.mark.parametrize("mode", list(MODES))
def test_file_sizes(saved, mode):
    s = saved(mode)
    _, how, env, sw = MODES[mode]
    res, W = s["res"], s["words"]
    apart = bool(env)
    planes = W + (1 if how.get("symmetry") else 0)
    common = C.sizeof(nat.KmcResult) + 8 * len(res.levels) + 8 * SEGS + 8 * W + 8 * planes * len(s["frontier"])
    tiles = -(-(SAVED_CAP // 64) // T)   # (one stretch: the table is smaller than the staging)
    size = {k: os.path.getsize(s["dir"] / k) for k in ("compact", "classic")}
    assert size["compact"] == HEADER + COMPACT_HEADER + common + 8 * (tiles + 1) + 8 * (sw + apart) * res.orbit_representatives
    assert size["classic"] == HEADER + common + 8 * (sw + apart) * SAVED_CAP and size["compact"] < size["classic"]
    assert open(s["dir"] / "classic", "rb").read() == open(s["dir"] / "classic2", "rb").read()


def test_refusals(saved, tmp_path):
    s = saved("plain")
    blob = open(s["dir"] / "compact", "rb").read()
    n = s["res"].orbit_representatives
    need = next(c for c in range(64, SAVED_CAP, 64) if n <= 0.92 * c)
    with checker("plain", table_capacity=need - 64) as mc:
        with pytest.raises(KmcError) as e:
            mc.load_checkpoint(str(s["dir"] / "compact"))
        assert e.value.code == 1 and f"table_capacity={need} " in str(e.value)   # KMC_E_ARG
    index_at = HEADER + COMPACT_HEADER + C.sizeof(nat.KmcResult) + 8 * len(s["res"].levels) + 8 * SEGS + 8 * s["words"]
    assert blob[index_at:index_at + 8] == bytes(8)   # (the index begins at 0)
    damaged = {"truncated in the entries": blob[:index_at + 8 * (SAVED_CAP // 512 + 1) + 8 * (n // 2)],
               "truncated in the frontier": blob[:-8],
               "an index word": blob[:index_at + 16] + (1 << 40).to_bytes(8, "little") + blob[index_at + 24:]}
    for data in damaged.values():
        (tmp_path / "damaged").write_bytes(data)
        with checker("plain") as mc:
            with pytest.raises(KmcError):
                mc.load_checkpoint(str(tmp_path / "damaged"))
    with checker("wide") as mc:   # other constants, another entry shape
        with pytest.raises(KmcError) as e:
            mc.load_checkpoint(str(s["dir"] / "compact"))
        assert e.value.code == 1
