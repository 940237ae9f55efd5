"""k_simulate on the GPU against the host emulation of the same lane-local code (tests/sim_emu.cpp), bit for bit: states,
kinds, choices, candidate counts, where each walk ends, every counter; against the GPU enumerator on sampled steps; the
independence of a walk from its batch; seeds; verdicts and witnesses; refusals; and the seen-set left alone.
Shapes: 4,096 + 37 walks (a partial last tile, more tiles than one wave takes) of depth 48 in launches of 1,024 (several
launches, the last one short) on one binding per path of the kernel."""
import ctypes as C
import os
import random

import pytest

import kmo
import sim_emu
from kafka_specification_amd import CheckerConfig, KmcError, ModelChecker
from kafka_specification_amd import _native as nat

pytestmark = pytest.mark.gpu

MODEL_NAMES = {v: k for k, v in kmo.MODELS.items()}
N_WALKS, DEPTH, WPL, SEED = 4096 + 37, 48, 1024, 0x5EED0001
SMALL = dict(table_capacity=1 << 16, frontier_capacity=1 << 12)
# id -> (model, N, L, R, E, K, layout mode of tests/sim_emu.cpp's entry)
BINDINGS = {
    "Kip320-3-2-2-1": (5, 3, 2, 2, 1, 0, 0),            # kind-major
    "Kip279-3-2-2-2": (4, 3, 2, 2, 2, 0, 0),            # HAS_EXTRA: records that repeat
    "Kip320-4-2-2-1": (5, 4, 2, 2, 1, 0, 0),            # instance bits over several words
    "Kip320-7-1-1-0": (5, 7, 1, 1, 0, 0, 0),            # seven replicas: 64-bit segments in the effect walk (the count is
                                                        # inst<I>'s guard block here as everywhere: no run-time guard<K> loop)
    "FiniteReplicatedLog-2-4-2": (1, 2, 4, 0, 0, 2, 0),  # instance-major
    "IdSequence-10": (0, 0, 0, 0, 0, 10, 0),
    "Kip320-3-2-2-1-tight": (5, 3, 2, 2, 1, 0, 1),
    "Kip320-3-2-2-1-rm": (5, 3, 2, 2, 1, 0, 2),
}


def consts(c):
    model, N, L, R, E, K, _lm = c
    if model == 0:
        return dict(max_id=K)
    if model == 1:
        return dict(n_replicas=N, log_size=L, n_log_records=K)
    return dict(n_replicas=N, log_size=L, max_records=R, max_leader_epoch=E)


class layout:
    """with layout(c): a handle opened inside reads the KMC_LAYOUT the emulation's entry was compiled with."""

    def __init__(self, c):
        self.value = sim_emu.LAYOUT_ENV[c[6]]

    def __enter__(self):
        self.old = os.environ.get("KMC_LAYOUT")
        os.environ["KMC_LAYOUT"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("KMC_LAYOUT", None)
        else:
            os.environ["KMC_LAYOUT"] = self.old


def open_checker(c, **kw):
    with layout(c):
        return ModelChecker(CheckerConfig(model=MODEL_NAMES[c[0]], **consts(c), **SMALL, **kw))


def emu_walks(mc, batch, indices):
    """the emulation's walks in the form ModelChecker.walk returns them"""
    names = mc.action_names()
    canon = {}

    def cb(words):
        if words not in canon:
            canon[words] = mc.unpack(words)
        return canon[words]
    return {w: [(None if k < 0 else names[k], cb(s), r, n) for (k, s, r, n) in batch.walk(w)] for w in indices}


def counters_of(res, mc):
    names = mc.action_names()
    inv = nat.invariant_names(mc.cfg.model)
    return dict(walks=res.walks, states_generated=res.states_generated,
                action_taken=[res.action_taken[n] for n in names] + [0] * (16 - len(names)), ended_early=res.ended_early,
                longest_walk=res.longest_walk, verdict=res.verdict,
                violated_invariant=-1 if res.violated_invariant is None else inv.index(res.violated_invariant),
                violation_walk=res.violation_walk, violation_step=res.violation_step,
                violation_count=[res.violation_count.get(n, 0) for n in inv], launches=res.launches)


_batches = {}


def recorded(bid):
    """One recorded batch per binding, computed once: the GPU's walks and counters, the emulation's, and a sample of steps
    checked against the GPU enumerator."""
    if bid not in _batches:
        c = BINDINGS[bid]
        emu = sim_emu.Batch(c, SEED, N_WALKS, DEPTH, walks_per_launch=WPL)
        with open_checker(c, invariants=()) as mc:
            res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, record=True)
            gpu = {w: mc.walk(w, depth=DEPTH, seed=SEED) for w in range(N_WALKS)}
            want = emu_walks(mc, emu, range(N_WALKS))
            rng = random.Random(len(bid))
            sampled = []
            while len(sampled) < 25:   # 25 steps per binding, 200 over the eight of them
                w = rng.randrange(N_WALKS)
                if len(gpu[w]) < 2:
                    continue
                t = rng.randrange(1, len(gpu[w]))
                succ = mc.successors(mc.pack(gpu[w][t - 1][1]))
                names = mc.action_names()
                sampled.append((w, t, gpu[w][t], [(names[k], mc.unpack(s)) for (s, _fp, k) in succ]))
            _batches[bid] = dict(gpu=gpu, emu=want, res=counters_of(res, mc), emu_res=emu.counters(), sampled=sampled)
    return _batches[bid]


@pytest.mark.parametrize("bid", sorted(BINDINGS))
def test_gpu_walks_equal_the_host_emulation_bit_for_bit(bid):
    b = recorded(bid)
    assert b["res"] == b["emu_res"]
    assert b["res"]["launches"] == 5 and b["res"]["walks"] == N_WALKS
    for w in range(N_WALKS):
        assert b["gpu"][w] == b["emu"][w], f"walk {w}"
    assert sum(len(x) for x in b["gpu"].values()) == b["res"]["states_generated"]
    assert max(len(x) for x in b["gpu"].values()) == b["res"]["longest_walk"]


def test_the_widest_shipped_object_walks_as_the_emulation_does():
    """BASELINE config 5 (Kip320 7/8/8/3: 357 instances, ten-word states, the object at the full register budget with spilled
    registers): a recorded batch with a partial last tile, every state of every walk against the emulation."""
    c = (5, 7, 8, 8, 3, 0, 0)
    walks, depth = 256 + 5, 100
    emu = sim_emu.Batch(c, SEED, walks, depth, walks_per_launch=128, threads=8)
    with open_checker(c, invariants=()) as mc:
        res = mc.simulate(walks, depth=depth, seed=SEED, walks_per_launch=128, record=True)
        assert counters_of(res, mc) == emu.counters() and res.launches == 3
        gpu = {w: mc.walk(w, depth=depth, seed=SEED) for w in range(walks)}
        want = emu_walks(mc, emu, range(walks))
    for w in range(walks):
        assert gpu[w] == want[w], f"walk {w}"
    assert res.longest_walk == depth


def test_a_repeated_record_is_walked_over():
    """Kip279: a successor two disjuncts of one binding yield stands twice in the enumeration (Kip279.tla:47-51)."""
    c = BINDINGS["Kip279-3-2-2-2"]
    b = recorded("Kip279-3-2-2-2")
    with open_checker(c, invariants=()) as mc:
        seen = 0
        done = set()
        for w in range(0, N_WALKS, 16):
            for t in range(1, len(b["gpu"][w])):
                prev = b["gpu"][w][t - 1][1]
                if prev in done:
                    continue
                done.add(prev)
                succ = [(s, k) for (s, _fp, k) in mc.successors(mc.pack(prev))]
                if len(set(succ)) < len(succ):
                    assert b["gpu"][w][t][3] == len(succ)
                    seen += 1
            if seen >= 3 or len(done) > 400:
                break
    assert seen >= 1, "no step of the sampled walks stood on a state with a repeated record"


@pytest.mark.parametrize("bid", sorted(BINDINGS))
def test_recorded_steps_against_the_enumerator(bid):
    b = recorded(bid)
    assert len(b["sampled"]) == 25
    for w, t, (name, state, choice, n_enabled), succ in b["sampled"]:
        assert (name, state) in succ, f"walk {w} step {t}"
        assert n_enabled == len(succ) and choice < n_enabled


@pytest.mark.parametrize("bid", ["Kip320-3-2-2-1", "Kip279-3-2-2-2"])
def test_a_walk_does_not_depend_on_its_batch(bid):
    c = BINDINGS[bid]
    b = recorded(bid)
    picks = (0, 63, 64, 1023, 1024, 4132)
    with open_checker(c, invariants=()) as mc:
        alone = {w: mc.walk(w, depth=DEPTH, seed=SEED) for w in picks}          # no recorded batch on this handle
        mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=257, record=True)
        other_launches = {w: mc.walk(w, depth=DEPTH, seed=SEED) for w in picks}
        started_there = {}
        for w in picks:
            mc.simulate(3, depth=DEPTH, seed=SEED, first_walk=w, record=True)
            started_there[w] = mc.walk(w, depth=DEPTH, seed=SEED)
    for w in picks:
        assert alone[w] == b["gpu"][w] == other_launches[w] == started_there[w], f"walk {w}"


def test_seed():
    c = BINDINGS["Kip320-3-2-2-1"]
    b = recorded("Kip320-3-2-2-1")
    with open_checker(c, invariants=()) as mc:
        again = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, record=True)
        assert counters_of(again, mc) == b["res"]
        assert all(mc.walk(w, depth=DEPTH, seed=SEED) == b["gpu"][w] for w in range(0, N_WALKS, 97))
        other = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED + 1, walks_per_launch=WPL, record=True)
        differ = sum(mc.walk(w, depth=DEPTH, seed=SEED + 1) != b["gpu"][w] for w in range(0, N_WALKS, 97))
        assert differ > 30 and counters_of(other, mc) != b["res"]


# (model, constants of tests/sim_emu.cpp, invariants, seed, walks, depth, walks per launch): chosen with the host emulation so
# that the first violation lies in the second (KafkaTruncateToHighWatermark) / third (Kip320FirstTry) launch
VERDICTS = {
    "KafkaTruncateToHighWatermark": ((2, 3, 2, 2, 2, 0, 0), ("TypeOk", "WeakIsr", "StrongIsr"), 1, 256, 40, 64),
    "Kip320FirstTry": ((6, 3, 2, 2, 2, 0, 0), ("TypeOk", "WeakIsr", "StrongIsr"), 1, 1 << 16, 40, 4096),
}


@pytest.mark.parametrize("name", sorted(VERDICTS))
def test_a_violation_is_found_where_the_emulation_finds_it(name):
    c, invariants, seed, walks, depth, wpl = VERDICTS[name]
    mask = sum(kmo.INV_BITS[i] for i in invariants)
    emu = sim_emu.Batch(c, seed, walks, depth, walks_per_launch=wpl, inv_mask=mask, record=False, threads=8).counters()
    assert emu["verdict"] == "invariant" and emu["launches"] >= 2 and emu["violated_invariant"] == 1
    with open_checker(c, invariants=invariants) as mc:
        res = mc.simulate(walks, depth=depth, seed=seed, walks_per_launch=wpl)
        assert counters_of(res, mc) == emu
        assert res.violated_invariant == "WeakIsr"
        behaviour = mc.walk(res.violation_walk, depth=depth, seed=seed)
        assert len(behaviour) == res.violation_step + 1
        # the behaviour replays through the enumerator from Init ...
        cur = None
        names = mc.action_names()
        for t, (action, state, _choice, _n) in enumerate(behaviour):
            words = mc.pack(state)
            if t == 0:
                ocfg = kmo.make_config(name, N=c[1], L=c[2], R=c[3], E=c[4], invariants=(), max_states=1, threads=1)
                assert action is None and state == kmo.Run(ocfg).state(0)
            else:
                assert (tuple(words), names.index(action)) in [(s, k) for (s, _fp, k) in mc.successors(cur)], f"step {t}"
            cur = words
        # ... and its last state is the witness: it fails the device's own predicate
        bad = (C.c_uint32 * 1)()
        nat.check(mc._lib.kmc_check_states(mc.handle, (C.c_uint64 * mc.state_words)(*cur), 1, mask, bad))
        assert bad[0] & 2
        for t in range(len(behaviour) - 1):   # ... the first such state of the walk
            nat.check(mc._lib.kmc_check_states(mc.handle, (C.c_uint64 * mc.state_words)(*mc.pack(behaviour[t][1])), 1, mask, bad))
            assert bad[0] == 0
    emu_all = sim_emu.Batch(c, seed, walks, depth, walks_per_launch=wpl, inv_mask=mask, record=False, threads=8,
                            continue_on_violation=True).counters()
    with open_checker(c, invariants=invariants, continue_on_violation=True) as mc:
        res = mc.simulate(walks, depth=depth, seed=seed, walks_per_launch=wpl)
        assert counters_of(res, mc) == emu_all
        assert res.launches == -(-walks // wpl) and res.violation_count["WeakIsr"] >= 1


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _front_end(front, *args):
    import subprocess
    import sys
    cmd = {"native": [os.path.join(ROOT, "kafka_specification_amd", "tlc")],
           "python": [sys.executable, "-m", "kafka_specification_amd.tlc"]}[front]
    # (KMC_NO_TORCH: the Python front end binds the system's HIP runtime without importing torch first — seconds per start)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), KMC_NO_TORCH="1")
    # (a small seen-set: the front ends size it from the free HBM by default, and mapping that takes seconds a walk never uses)
    r = subprocess.run(cmd + ["-table", str(1 << 16), "-frontier", str(1 << 12)] + list(args), capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    # the lines of the report: everything from the opening line on, the closing timing line excepted
    lines = r.stdout.splitlines()
    start = [i for i, l in enumerate(lines) if l.startswith("Running Random Simulation")]
    assert len(start) == 1, r.stdout + r.stderr
    body = [l for l in lines[start[0]:] if not l.startswith("Finished in ")]
    assert len(body) == len(lines) - start[0] - 1 and lines[-1].startswith("Finished in ")
    return r.returncode, body


def test_both_command_lines_print_the_same_violation():
    """-walks through both front ends (what these three tests are about: the two programs): the violating module with a fixed
    seed — status 12, the behaviour printed state by state, the same lines from both, the witness the emulation's."""
    spec = os.path.join("models", "KafkaTruncateToHighWatermark.tla")   # its .cfg: 3 / 2 / 2 / 2, TypeOk WeakIsr StrongIsr
    emu = sim_emu.Batch((2, 3, 2, 2, 2, 0, 0), 1, 4096, 40, inv_mask=7, record=False).counters()
    assert emu["verdict"] == "invariant"
    out = {f: _front_end(f, spec, "-deadlock", "-walks", "4096", "-walk-depth", "40", "-walk-seed", "1") for f in ("native", "python")}
    assert out["native"][0] == out["python"][0] == 12
    assert out["native"][1] == out["python"][1]
    body = out["native"][1]
    assert body[0] == "Running Random Simulation with seed 1: 4096 walks of at most 40 states on GPU 0."
    assert body[1] == "Error: Invariant WeakIsr is violated."
    assert body[2] == f"Error: The behavior up to this point is (walk {emu['violation_walk']}):"
    states = [l for l in body if l.startswith("State ")]
    assert len(states) == emu["violation_step"] + 1 and states[0] == "State 1: <Initial predicate>"
    assert all(" of module KafkaTruncateToHighWatermark>" in l for l in states[1:])
    assert sum(l.startswith("/\\ replicaLog = ") for l in body) == len(states)
    assert f"The number of states generated: {emu['states_generated']}" in body
    assert f"Progress: 4096 walks run in 1 launches, {emu['states_generated']} states checked." in body
    assert body[-1] == f"{emu['ended_early']} walks ended on a state without successors; the longest walk has {emu['longest_walk']} states."
    # the behaviour printed is the walk: its last state is ModelChecker.walk's, through the same formatter
    from kafka_specification_amd.format import format_state
    with open_checker((2, 3, 2, 2, 2, 0, 0), invariants=("TypeOk", "WeakIsr", "StrongIsr")) as mc:
        walk = mc.walk(emu["violation_walk"], depth=40, seed=1)
        last = format_state(mc.cfg, walk[-1][1]).splitlines()
    at = body.index(states[-1])
    assert body[at + 1:at + 1 + len(last)] == last


def test_both_command_lines_pass_a_batch_alike():
    kip320 = os.path.join("models", "Kip320.tla")
    ok = {f: _front_end(f, kip320, "-walks", "1000", "-walk-depth", "30") for f in ("native", "python")}
    assert ok["native"][0] == ok["python"][0] == 0 and ok["native"][1] == ok["python"][1]
    assert ok["native"][1][1] == "Random simulation completed. No error has been found."


def test_both_command_lines_print_the_same_checked_deadlock(tmp_path):
    """the models' own .cfg files all switch the check off: this one leaves TLC's default on"""
    kip320 = os.path.join("models", "Kip320.tla")
    cfg = tmp_path / "Kip320_deadlock.cfg"
    cfg.write_text("CONSTANTS\n  Replicas = {b1, b2, b3}\n  LogSize = 2\n  MaxRecords = 2\n  MaxLeaderEpoch = 1\n"
                   "INIT Init\nNEXT Next\nINVARIANTS TypeOk WeakIsr StrongIsr\n")
    emu = sim_emu.Batch(BINDINGS["Kip320-3-2-2-1"], 0, 512, 48, inv_mask=7, check_deadlock=True, record=False).counters()
    assert emu["verdict"] == "deadlock"
    dl = {f: _front_end(f, kip320, "-config", str(cfg), "-walks", "512", "-walk-depth", "48") for f in ("native", "python")}
    assert dl["native"][0] == dl["python"][0] == 11 and dl["native"][1] == dl["python"][1]
    assert dl["native"][1][1] == "Error: Deadlock reached."
    assert dl["native"][1][2] == f"Error: The behavior up to this point is (walk {emu['violation_walk']}):"
    assert sum(l.startswith("State ") for l in dl["native"][1]) == emu["violation_step"] + 1


def test_passing_invariants_and_the_checked_deadlock():
    c = BINDINGS["Kip320-3-2-2-1"]
    invariants = ("TypeOk", "WeakIsr", "StrongIsr")
    emu = sim_emu.Batch(c, SEED, N_WALKS, DEPTH, walks_per_launch=WPL, inv_mask=7, record=False).counters()
    assert emu["verdict"] == "ok" and emu["ended_early"] > 0
    with open_checker(c, invariants=invariants) as mc:
        res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL)
        assert res.verdict == "ok" and counters_of(res, mc) == emu
    emu = sim_emu.Batch(c, SEED, N_WALKS, DEPTH, walks_per_launch=WPL, inv_mask=7, check_deadlock=True, record=False).counters()
    assert emu["verdict"] == "deadlock"
    with open_checker(c, invariants=invariants, check_deadlock=True) as mc:
        res = mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL)
        assert res.verdict == "deadlock" and counters_of(res, mc) == emu
        last = mc.walk(res.violation_walk, depth=DEPTH, seed=SEED)
        assert len(last) == res.violation_step + 1 and mc.successors(mc.pack(last[-1][1])) == []


def test_refusals():
    with ModelChecker(CheckerConfig(model="AsyncIsr", n_replicas=3, log_size=2, max_leader_epoch=2, **SMALL)) as mc:
        with pytest.raises(KmcError, match="AsyncIsr") as e:
            mc.simulate(8)
        assert e.value.code == 1
    with ModelChecker(CheckerConfig(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1, symmetry=True,
                                    **SMALL)) as mc:
        with pytest.raises(KmcError, match="symmetry") as e:
            mc.simulate(8)
        assert e.value.code == 1
    with ModelChecker(CheckerConfig(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1, device=-1)) as mc:
        with pytest.raises(KmcError, match="host-only") as e:
            mc.simulate(8)
        assert e.value.code == 5
    with open_checker(BINDINGS["Kip320-3-2-2-1"]) as mc:
        with pytest.raises(KmcError, match="record") as e:
            mc.simulate(1 << 22, depth=100, record=True)   # 2^22 walks x 100 states x 3 words: beyond 1 GiB
        assert e.value.code == 1
        with pytest.raises(KmcError, match="n_walks") as e:
            mc.simulate(0)
        assert e.value.code == 1


def test_the_seen_set_is_untouched():
    inv = ("TypeOk", "WeakIsr", "StrongIsr")
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=2, R=2, E=1, invariants=inv))
    with ModelChecker(CheckerConfig(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1, invariants=inv,
                                    table_capacity=1 << 20, frontier_capacity=1 << 16)) as mc:
        first = mc.run()
        mc.simulate(N_WALKS, depth=DEPTH, seed=SEED, walks_per_launch=WPL, record=True)
        r = mc.run()
        assert (r.verdict, r.distinct, r.generated, r.depth, r.levels) == (o.verdict, o.distinct, o.generated, o.depth, o.levels)
        assert (first.distinct, first.generated) == (r.distinct, r.generated)
