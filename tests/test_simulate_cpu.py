"""Random simulation without a GPU: the lane-local layer of csrc/kmc_sim.h (compiled for the host by tests/sim_emu.cpp) against
the exact C oracle step by step, the bijection between draws and the enumeration of Next, the draw itself, both front ends'
new switches, and the same code under the sanitizers in a stand-alone program.  What this cannot cover is k_simulate's wave
layer: tests/test_gpu_simulate.py holds the GPU to this emulation bit for bit."""
import collections
import os
import subprocess
import sys

import pytest

import kmo
import sim_emu
from kafka_specification_amd import CheckerConfig, ModelChecker
from kafka_specification_amd.checker import sim_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_NAMES = {v: k for k, v in kmo.MODELS.items()}
# the small table every path of the lane-local layer goes through (tests/sim_emu.cpp also holds forced layouts and the bench's bindings: the GPU tests' and the tool's)
TABLE = [(5, 3, 2, 2, 1, 0, 0), (4, 3, 2, 2, 2, 0, 0), (2, 3, 2, 2, 2, 0, 0), (6, 3, 2, 2, 2, 0, 0), (3, 3, 2, 2, 2, 0, 0),
         (5, 4, 2, 2, 1, 0, 0), (5, 7, 1, 1, 0, 0, 0), (1, 2, 4, 0, 0, 2, 0), (0, 0, 0, 0, 0, 10, 0)]
SEED, WALKS, DEPTH = 20260101, 256, 40


def _ids(c):
    return f"{MODEL_NAMES[c[0]]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}-{c[5]}"


def _consts(c):
    model, N, L, R, E, K, _lm = c
    if model == 0:
        return dict(max_id=K), dict(MaxId=K)
    if model == 1:
        return dict(n_replicas=N, log_size=L, n_log_records=K), dict(N=N, L=L, K=K)
    return dict(n_replicas=N, log_size=L, max_records=R, max_leader_epoch=E), dict(N=N, L=L, R=R, E=E)


_cache = {}


def batch_of(c):
    """(walks as [(kind, canonical bytes, choice, n_enabled)], oracle config, state bytes): computed once per entry."""
    if c not in _cache:
        assert c in sim_emu.configs()
        name = MODEL_NAMES[c[0]]
        kc, oc = _consts(c)
        ocfg = kmo.make_config(name, invariants=(), max_states=1, threads=1, **oc)
        sb = kmo.Run(ocfg).sb
        b = sim_emu.Batch(c, SEED, WALKS, DEPTH)
        with ModelChecker(CheckerConfig(model=name, device=-1, **kc)) as mc:
            unpacked = {}

            def canon(words):
                if words not in unpacked:
                    unpacked[words] = mc.unpack(words)
                return unpacked[words]
            walks = [[(k, canon(w), r, n) for (k, w, r, n) in b.walk(i)] for i in range(WALKS)]
        _cache[c] = (walks, ocfg, sb)
    return _cache[c]


_succ = {}


def oracle_successors(c, ocfg, sb, state):
    key = (c, state)
    if key not in _succ:
        _succ[key] = kmo.successors(ocfg, state, sb)
    return _succ[key]


@pytest.mark.parametrize("c", TABLE, ids=_ids)
def test_every_step_is_a_step_of_the_oracle(c):
    walks, ocfg, sb = batch_of(c)
    steps = 0
    for w, walk in enumerate(walks):
        assert walk[0][0] == -1 and walk[0][2:] == (0, 0)
        assert walk[0][1] == kmo.Run(ocfg).state(0) if w == 0 else True   # Init
        for t in range(1, len(walk)):
            kind, state, choice, n_enabled = walk[t]
            want = oracle_successors(c, ocfg, sb, walk[t - 1][1])
            assert (kind, state) in want, f"walk {w} step {t}: not a successor of the state before it under that action"
            assert n_enabled == len(want), f"walk {w} step {t}: candidates"
            assert choice == sim_draw(SEED, w, t - 1, n_enabled) < n_enabled
            steps += 1
        # a walk ends by depth or on a state the oracle gives no successor (no invariant is checked here)
        assert len(walk) == DEPTH or not oracle_successors(c, ocfg, sb, walk[-1][1])
    assert steps > WALKS


@pytest.mark.parametrize("c", TABLE, ids=_ids)
def test_draws_map_onto_the_enumeration_one_to_one(c):
    walks, ocfg, sb = batch_of(c)
    chosen = collections.defaultdict(dict)   # state -> {choice: (kind, successor)}
    for walk in walks:
        for t in range(1, len(walk)):
            kind, state, choice, _n = walk[t]
            prev = chosen[walk[t - 1][1]].setdefault(choice, (kind, state))
            assert prev == (kind, state), "the same draw on the same state chose another record"
    complete = 0
    for state, by_choice in chosen.items():
        want = oracle_successors(c, ocfg, sb, state)
        if len(by_choice) == len(want):   # every one of 0..n-1 was drawn on this state
            assert sorted(by_choice) == list(range(len(want)))
            assert sorted(by_choice.values()) == sorted(want), "the chosen records are not the oracle's enumeration"
            complete += 1
    assert complete >= 1, "no state on which every candidate was drawn (Init with 256 walkers should be one)"
    assert len(chosen[walks[0][0][1]]) == len(oracle_successors(c, ocfg, sb, walks[0][0][1]))   # Init is one


def test_the_draw():
    assert all(sim_draw(s, w, t, 1) == 0 for s in (0, 1, 2 ** 64 - 1) for w in (0, 5, 2 ** 40) for t in (0, 1, 99))
    for n in (2, 3, 7, 64, 1000, 2 ** 16 + 1, 2 ** 20 - 1, 2 ** 20):
        assert all(sim_draw(s, w, t, n) < n for s in range(4) for w in range(16) for t in range(16))
    grid = {sim_draw(s, w, t, 2) for s in range(64) for w in range(64) for t in range(64)}
    assert grid == {0, 1}
    # the host emulation's and the library's are one definition (csrc/kmc_sim.h)
    assert all(sim_emu.draw(9, w, t, 1000) == sim_draw(9, w, t, 1000) for w in range(8) for t in range(8))


def _draw_by_definition(seed, walk, step, n):
    """The definition, written out: splitmix64's finaliser; key = mix(mix(seed + G) + walk * C); h = mix(key + (step + 1) * G);
    the draw is the high half of h * n."""
    M = 2 ** 64 - 1
    G, Cc = 0x9E3779B97F4A7C15, 0xD1342543DE82EF95

    def mix(x):
        x ^= x >> 30
        x = x * 0xbf58476d1ce4e5b9 & M
        x ^= x >> 27
        x = x * 0x94d049bb133111eb & M
        return x ^ (x >> 31)
    key = mix((mix((seed + G) & M) + walk * Cc) & M)
    return (mix((key + (step + 1) * G) & M) * n) >> 64


# sixteen (seed, walk, step, n) -> value pairs computed from the definition above when the function was introduced: they freeze it
FROZEN = [
    ((0, 0, 0, 2), 0), ((0, 0, 1, 2), 0), ((0, 1, 0, 7), 4), ((1, 0, 0, 7), 3),
    ((1, 2, 3, 10), 8), ((42, 1000, 99, 60), 22), ((42, 1001, 99, 60), 12), ((2 ** 64 - 1, 2 ** 64 - 1, 2 ** 20 - 1, 2 ** 20), 498128),
    ((20260101, 0, 0, 6), 2), ((20260101, 63, 5, 13), 11), ((20260101, 64, 5, 13), 9), ((7, 4132, 47, 357), 76),
    ((7, 1 << 33, 0, 3), 2), ((123456789, 5, 39, 2), 0), ((0xDEADBEEF, 77, 11, 1 << 19), 393775), ((3, 3, 3, 3), 1),
]


def test_the_draw_is_frozen():
    assert len(FROZEN) == 16
    for args, value in FROZEN:
        assert value is not None, "literal missing"
        assert sim_draw(*args) == value == _draw_by_definition(*args), args


def test_the_lane_local_layer_under_the_sanitizers():
    """tests/sim_san.cpp: its own main over the same table entries, -fsanitize=address,undefined; it is not loaded into Python."""
    exe = sim_emu.build_san()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sim_san ok" in r.stdout
    # ... and it ran the same walks: its checksum of a batch is the shared library's
    b = sim_emu.Batch((5, 3, 2, 2, 1, 0, 0), 5, 64, 24)
    line = [l for l in r.stdout.splitlines() if l.startswith("Kip320 3/2/2/1 ")][0]
    assert int(line.split()[-1]) == b.counters()["states_generated"]


# ---- the front ends -----------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "kafka_specification_amd", "tlc")
SPEC = os.path.join(ROOT, "models", "Kip320.tla")
FRONT_ENDS = {"native": [CLI], "python": [sys.executable, "-m", "kafka_specification_amd.tlc"]}


def _run(front, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="-1",
               ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run(FRONT_ENDS[front] + [SPEC] + list(args), capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)


@pytest.mark.parametrize("front", sorted(FRONT_ENDS))
def test_front_end_walk_switches(front):
    r = _run(front, "-walks", "0")
    assert r.returncode == 2 and "-walks" in r.stdout + r.stderr and "at least 1" in r.stdout + r.stderr
    r = _run(front, "-walk-depth", "10")
    assert r.returncode == 2 and "-walk-depth" in r.stdout + r.stderr and "-walks" in r.stdout + r.stderr
    r = _run(front, "-walk-seed", "10")
    assert r.returncode == 2 and "-walk-seed" in r.stdout + r.stderr
    r = _run(front, "-walks", "many")
    assert r.returncode == 2
    r = _run(front, "-deadlock", "-walks", "8")   # no GPU is visible: the run ends at the device
    assert r.returncode == 3, r.stdout + r.stderr
    r = _run(front, "-simulate")
    assert r.returncode == 2 and "random simulation is another mode of TLC" in r.stdout + r.stderr


def test_front_ends_say_the_same_about_the_walk_switches():
    for args in (("-walks", "0"), ("-walk-depth", "10"), ("-walk-seed", "1"), ("-walks", "x")):
        a, b = _run("native", *args), _run("python", *args)
        assert a.returncode == b.returncode == 2
        pick = lambda r: [l for l in (r.stdout + r.stderr).splitlines() if "-walk" in l]   # noqa: E731
        assert pick(a) == pick(b) and pick(a), args
