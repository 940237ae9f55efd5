"""Test-side binding of tests/sim_emu.cpp: random simulation's lane-local layer (csrc/kmc_sim.h) compiled for the host, and
the batch logic of the contract around it.  Test infrastructure only (and the CPU baseline of tools/sim_bench.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim_emu.cpp")
LIB = os.path.join(HERE, "_sim_emu.so")
SAN_SRC = os.path.join(HERE, "sim_san.cpp")
SAN_BIN = os.path.join(HERE, "_sim_san")
CSRC = os.path.join(HERE, "..", "kafka_specification_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.startswith("kmc_") and f.endswith(".h")]
_lib = None

LAYOUT_ENV = {0: "auto", 1: "tight", 2: "rm", 3: "rmg"}   # KMC_LAYOUT_* -> the KMC_LAYOUT value the host library reads
VERDICTS = ("ok", "invariant", "deadlock")


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(d) for d in deps)


def build():
    if _stale(LIB, DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", LIB, SRC])


def build_san():
    """tests/sim_san.cpp: the same code with its own main under -fsanitize=address,undefined (never loaded into Python)."""
    if _stale(SAN_BIN, DEPS + [SAN_SRC]):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                               "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: it runs whatever else is preloaded)
                               "-fno-sanitize-recover=all", "-DSIM_EMU_SMALL_TABLE=1", "-o", SAN_BIN, SAN_SRC])
    return SAN_BIN


class Result(C.Structure):
    _fields_ = [("walks", C.c_uint64), ("states_generated", C.c_uint64), ("action_taken", C.c_uint64 * 16),
                ("ended_early", C.c_uint64), ("longest_walk", C.c_uint64), ("verdict", C.c_int32),
                ("violated_invariant", C.c_int32), ("violation_walk", C.c_uint64), ("violation_step", C.c_uint64),
                ("violation_count", C.c_uint64 * 4), ("launches", C.c_uint64)]


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(LIB)
        l.sim_emu_configs.argtypes = [C.c_int, C.POINTER(C.c_int)]
        l.sim_emu_words.argtypes = [C.POINTER(C.c_int)]
        l.sim_emu_draw.restype = C.c_uint64
        l.sim_emu_draw.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
        l.sim_emu_run.argtypes = [C.POINTER(C.c_int), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32,
                                  C.c_int, C.c_int, C.c_int, C.POINTER(Result), C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def configs():
    """[(model, N, L, R, E, K, layout mode)] compiled into the emulation (IdSequence: K is MaxId)."""
    out = (C.c_int * 7)()
    n = lib().sim_emu_configs(-1, out)
    res = []
    for i in range(n):
        lib().sim_emu_configs(i, out)
        res.append(tuple(out))
    return res


def words(cfg7):
    return lib().sim_emu_words((C.c_int * 7)(*cfg7))


def draw(seed, walk, step, n):
    return int(lib().sim_emu_draw(seed, walk, step, n))


class Batch:
    """One batch run by the emulation.  result: the counters (Result); with record=True also lens[n_walks] and
    rec[n_walks, depth, W + 1] (uint64: state words, then kmc_sim_meta of how the state was reached)."""

    def __init__(self, cfg7, seed, n_walks, depth, first_walk=0, walks_per_launch=0, inv_mask=0, check_deadlock=False,
                 continue_on_violation=False, threads=4, record=True):
        self.W = words(cfg7)
        assert self.W > 0, f"{cfg7} is not compiled into tests/sim_emu.cpp"
        self.depth, self.n_walks, self.first_walk, self.seed = depth, n_walks, first_walk, seed
        self.result = Result()
        self.rec = np.zeros((n_walks, depth, self.W + 1), dtype=np.uint64) if record else None
        self.lens = np.zeros(n_walks, dtype=np.uint32)
        rc = lib().sim_emu_run((C.c_int * 7)(*cfg7), seed, first_walk, n_walks, depth, walks_per_launch, inv_mask,
                               int(check_deadlock), int(continue_on_violation), threads, C.byref(self.result),
                               self.rec.ctypes.data if record else None, self.lens.ctypes.data)
        assert rc == 0

    def walk(self, w):
        """[(kind or -1, state words tuple, choice, n_enabled)] of walk index w (absolute)."""
        i = w - self.first_walk
        out = []
        for t in range(int(self.lens[i])):
            meta = int(self.rec[i, t, self.W])
            out.append(((meta & 0xFFFF) - 1, tuple(int(x) for x in self.rec[i, t, :self.W]), (meta >> 16) & 0xFFFFFF, meta >> 40))
        return out

    def counters(self):
        r = self.result
        return dict(walks=int(r.walks), states_generated=int(r.states_generated), action_taken=[int(x) for x in r.action_taken],
                    ended_early=int(r.ended_early), longest_walk=int(r.longest_walk), verdict=VERDICTS[r.verdict],
                    violated_invariant=int(r.violated_invariant), violation_walk=int(r.violation_walk),
                    violation_step=int(r.violation_step), violation_count=[int(x) for x in r.violation_count],
                    launches=int(r.launches))
