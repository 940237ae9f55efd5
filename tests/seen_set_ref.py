"""Reference side of the seen-set's claim paths (csrc/kmc_sink.h: claim_steps, claim_steps<1>, claim_wide_steps, claim_any) and
of the host's walk along the same chains (table_lookup, csrc/kmc_engine_run.cpp), in plain Python and numpy: the fingerprint,
the check word of a wide slot and the reduced fingerprint of a -DKMC_TEST_FP_BITS build; synthetic states homed where a test
wants them; the one-level driver that hands records to k_insert through the level-step ABI and reads the table back from a
checkpoint; and the predicate every correct table image satisfies (placement under races is not deterministic: the predicate
says what all correct images have in common).  The slot functions, the sequential insert and the probe-path clause are
tests/rehash_ref.py's.  Importable without a GPU: tests/test_seen_set_ref_cpu.py holds the mirrors to the headers and the
predicate to one mutant per clause; tests/test_gpu_seen_set_direct.py uses it."""
import ctypes as C
import functools
import os

import numpy as np

import rehash_ref as rr

U64 = np.uint64
GOLD = 0x9E3779B97F4A7C15
CHECK_SEED = 0x6a09e667f3bcc908          # claim_any: the check word is the fingerprint under seed ^ this
ERR_TABLE_FULL = 2                       # KMC_ERR_TABLE_FULL
V_LEVEL_LIMIT = 5                        # KMC_V_LEVEL_LIMIT
SEGS = 8                                 # KMC_SEGS
MAX_PROBES = 1024                        # claim_steps: max_probes = min(cap - 1, 1024); a walk ends after 2 max_probes + 2 steps
LOAD_LIMIT = 0.92                        # KMC_TABLE_LOAD_LIMIT
M64 = (1 << 64) - 1

CONSTANTS = dict(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1, invariants=())
N_STATES = 39_619                        # reachable states of these constants
TEST_FP_BITS = 10
TEST_FP_DEFINES = "-DKMC_TUNING=1 -DKMC_TEST_FP_BITS=10"
DEFER_DEFINES = "-DKMC_DEFER_MIN_WORDS=1"

# shape -> (wide_fingerprint, keep_trace, words per slot in memory, predecessors in a table of their own,
#           rehash_ref's (slot words, predecessor word) of the image the predicate sees)
SHAPES = {"narrow": (False, False, 1, False, (1, False)),
          "paired": (False, True, 2, False, (1, True)),     # 16-byte slots of fingerprint + predecessor (KMC_FLAG_PAIRED)
          "wide": (True, True, 2, True, (2, True))}         # 16-byte slots of fingerprint + check word; a.pred[i] apart

# The smallest multiple of 64 slots with an odd number of groups in which the 39,619 reachable states, placed by their
# fingerprints, form no cyclic run of occupied slots longer than MAX_PROBES / 2 (tests/test_seen_set_ref_cpu.py re-derives it)
CROWDED_SEARCH_CAP = 64 * 679              # load 0.912, longest run 510


def max_probes(cap):
    return min(cap - 1, MAX_PROBES)


# -- kmc_common.h / kmc_sink.h ----------------------------------------------------------------------------------------------
def mix64(x):
    """kmc_mix64, on Python ints or uint64 arrays"""
    if isinstance(x, np.ndarray):
        x = x ^ (x >> U64(30))
        x = x * U64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> U64(27))
        x = x * U64(0x94d049bb133111eb)
        return x ^ (x >> U64(31))
    x ^= x >> 30
    x = x * 0xbf58476d1ce4e5b9 & M64
    x ^= x >> 27
    x = x * 0x94d049bb133111eb & M64
    return x ^ (x >> 31)


def fingerprint(states, seed=0):
    """kmc_fingerprint<W> of the rows of `states` (W < KMC_FOLD_MIN_WORDS = 8: the per-word chain), as a uint64 array"""
    states = np.asarray(states, dtype=U64)
    W = states.shape[1]
    assert W < 8
    h = np.full(len(states), mix64((seed + GOLD * (W + 1)) & M64), dtype=U64)
    with np.errstate(over="ignore"):
        for k in range(W):
            h = mix64(h ^ states[:, k]) + U64(GOLD)
    h[h == 0] = 1
    return h


def check_word(states, seed=0):
    return fingerprint(states, seed ^ CHECK_SEED)


def reduce_fp(fp, bits=TEST_FP_BITS):
    """KmcSink::fingerprint_of under -DKMC_TEST_FP_BITS=bits: what the table of such a build holds for the fingerprint fp"""
    if isinstance(fp, np.ndarray):
        with np.errstate(over="ignore"):
            return mix64((fp & U64((1 << bits) - 1)) + U64(GOLD)) | U64(1)
    return mix64(((fp & ((1 << bits) - 1)) + GOLD) & M64) | 1


# -- states -----------------------------------------------------------------------------------------------------------------
def synthetic(first, n, W, seed):
    """n synthetic "states", distinct by construction and never equal to a reachable one: bit 63 of word 0, the index
    first + k above bit 20, the other words random under `seed` — k_insert fingerprints and claims whatever words it is given"""
    states = np.random.default_rng([seed, first]).integers(0, 1 << 62, size=(n, W), dtype=U64)
    states[:, 0] = (np.arange(first, first + n, dtype=U64) << U64(20)) | U64(1 << 63)
    return states


def index_of(states):
    return ((np.asarray(states, dtype=U64)[:, 0] & U64((1 << 63) - 1)) >> U64(20)).astype(np.int64)


def select_homed(K, cap, groups, W, seed, first=0, fp_of=fingerprint, keep=None):
    """The first K synthetic states from index `first` on whose home slot, slot_of(fp_of(state), cap), lies in one of `groups`
    (None: anywhere) and for which keep(fingerprints) holds; (states, what fp_of gives for them)."""
    groups = None if groups is None else np.asarray(sorted(groups), dtype=U64)
    got, got_fp, at, have = [], [], first, 0
    while have < K:
        cand = synthetic(at, 1 << 15, W, seed)
        at += len(cand)
        fp = fp_of(cand)
        ok = np.ones(len(cand), dtype=bool) if groups is None else np.isin(rr.slot_of(fp, cap) >> U64(6), groups)
        if keep is not None:
            ok &= keep(fp)
        got.append(cand[ok])
        got_fp.append(fp[ok])
        have += int(ok.sum())
    return np.concatenate(got)[:K], np.concatenate(got_fp)[:K]


def meta_of(index, copy):
    """The predecessor word copy `copy` (0..15) of synthetic state `index` carries: distinct per copy, never 0"""
    return (0x5EED << 44) | (int(index) << 4) | int(copy)


def records(states, copies, trace, seed, copy0=0):
    """(records, allowed): every state copies[k] times, shuffled; with `trace` a record's last word is meta_of(index, copy0 + copy)
    and allowed[k] the metas of state k's copies."""
    states = np.asarray(states, dtype=U64)
    W = states.shape[1]
    which = np.repeat(np.arange(len(states)), copies)
    copy = np.concatenate([np.arange(copy0, copy0 + c) for c in copies]) if len(states) else np.zeros(0, dtype=np.int64)
    recs = np.zeros((len(which), W + (1 if trace else 0)), dtype=U64)
    recs[:, :W] = states[which]
    idx = index_of(states)
    if trace:
        recs[:, W] = [meta_of(idx[k], c) for k, c in zip(which, copy)]
    np.random.default_rng([seed, len(which)]).shuffle(recs)
    allowed = [frozenset(meta_of(idx[k], copy0 + c) for c in range(copies[k])) for k in range(len(states))]
    return recs, allowed


@functools.lru_cache(maxsize=None)
def host_handle(seed=0):
    """A host-only handle (device = -1) of the constants: pack / unpack / fingerprint under `seed`"""
    from kafka_specification_amd import CheckerConfig, ModelChecker
    return ModelChecker(CheckerConfig(**CONSTANTS, device=-1, hash_seed=seed))


@functools.lru_cache(maxsize=None)
def reachable():
    """(packed states, level sizes) of the exhaustive oracle, level after level"""
    import kmo
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=2, R=2, E=1, invariants=()))
    mc = host_handle()
    rows = np.array([mc.pack(s) for k in range(len(o.levels)) for s in sorted(o.level_states(k))], dtype=U64)
    assert len(rows) == N_STATES == o.distinct
    return rows, tuple(o.levels)


def real_states():
    """Init and the six states of the level the one-level driver really expands to"""
    rows, levels = reachable()
    assert levels[:2] == (1, 6)
    return rows[:7]


# -- runs of occupied slots ------------------------------------------------------------------------------------------------
def occupied(word0, cap):
    """Which slots a linear-probing table of `cap` slots holds after the fingerprints `word0` went in: the same for every
    order of insertion (a slot is taken as soon as anything reaches it).  A sweep with a carry, twice round for the wrap."""
    count = np.bincount(rr.slot_of(np.asarray(word0, dtype=U64), cap).astype(np.int64), minlength=cap).tolist()
    assert len(word0) <= cap
    taken = bytearray(cap)
    carry = 0
    for _round in range(2):
        for i in range(cap):
            if not taken[i]:
                carry += count[i]
                count[i] = 0
                if carry:
                    taken[i] = 1
                    carry -= 1
            else:
                carry += count[i]
                count[i] = 0
    assert carry == 0 and sum(taken) == len(word0)
    return np.frombuffer(bytes(taken), dtype=np.uint8).astype(bool)


def longest_cyclic_run(taken):
    """The longest run of occupied slots, the one over the end into slot 0 included"""
    taken = np.asarray(taken, dtype=bool)
    if taken.all():
        return len(taken)
    first_hole = int(np.flatnonzero(~taken)[0])
    t = np.roll(taken, -first_hole - 1)          # ends in a hole: no run wraps now
    edges = np.flatnonzero(np.diff(np.concatenate([[0], t.astype(np.int8), [0]])))
    return int((edges[1::2] - edges[0::2]).max()) if len(edges) else 0


def smallest_odd_cap(word0, run_limit):
    """The smallest multiple of 64 with an odd number of groups at which the longest cyclic run is at most run_limit"""
    G = (len(word0) + 63) // 64
    G += 1 - G % 2
    while longest_cyclic_run(occupied(word0, 64 * G)) > run_limit:
        G += 2
    return 64 * G


# -- the predicate ---------------------------------------------------------------------------------------------------------
def expected_rows(fps, chks=None, allowed=None):
    """Rows of the predicate's `expected`: (fingerprint, check word or None, the predecessor words allowed or None)"""
    n = len(fps)
    return [(int(fps[k]), None if chks is None else int(chks[k]), None if allowed is None else allowed[k]) for k in range(n)]


def seen_set_violations(image, pred_image, cap, shape, expected):
    """Every clause the table image violates, as text, in the order of the clauses.  image: cap x (1 or 2) words (a paired
    table's fingerprint words); pred_image: cap predecessor words or None; expected: expected_rows of what went in.
      1  word 0 of the occupied slots is, as a multiset, the expected fingerprints
      2  wide slots: word 1 is the check word that goes with word 0 (as a multiset of pairs), and none is 0
      3  no probe path from a home to its entry crosses an empty slot, cyclically
      4  empty slots are zero in every word and in their predecessor word
      5  the predecessor of an entry is one of the words allowed for it"""
    SW, SP = SHAPES[shape][4]
    out = []
    slots = np.asarray(image, dtype=U64).reshape(cap, SW)
    occ = np.flatnonzero(slots[:, 0])
    got0 = np.sort(slots[occ, 0])
    want0 = np.sort(np.array([e[0] for e in expected], dtype=U64))
    if len(got0) != len(want0):
        out.append(f"clause 1: the table holds {len(got0)} entries, {len(want0)} went in")
    elif not np.array_equal(got0, want0):
        k = int(np.flatnonzero(got0 != want0)[0])
        out.append(f"clause 1: the fingerprints differ as multisets; first in sorted order: table {int(got0[k]):#x}, expected {int(want0[k]):#x}")
    if SW == 2:
        got = sorted((int(a), int(b)) for a, b in slots[occ])
        want = sorted((e[0], e[1]) for e in expected)
        zeros = int((slots[occ, 1] == 0).sum())
        if zeros:
            out.append(f"clause 2: {zeros} occupied slot(s) without a check word, first slot {int(occ[slots[occ, 1] == 0][0])}")
        elif got != want and sorted(a for a, _ in got) == sorted(a for a, _ in want):
            bad = next(g for g, w in zip(got, want) if g != w)
            out.append(f"clause 2: the check words differ; first in sorted order: fingerprint {bad[0]:#x} holds {bad[1]:#x}")
    tabs = (slots.reshape(-1), None if not SP else np.asarray(pred_image, dtype=U64))
    for said in rr.rehash_violations(tabs, tabs, cap, cap, SW, SP):   # (its clauses 2 and 3 are the probe path and the empty slots)
        clause = int(said.split(":")[0].split()[1])
        assert clause in (2, 3), said
        out.append(f"clause {clause + 1}:" + said.split(":", 1)[1])
    if SP:
        key = (lambda i: (int(slots[i, 0]), int(slots[i, 1]))) if SW == 2 else (lambda i: int(slots[i, 0]))
        allowed = {}
        for fp, chk, al in expected:
            if al is not None:
                allowed.setdefault((fp, chk) if SW == 2 else fp, []).append(al)
        bad = []
        for i in occ:
            sets = allowed.get(key(int(i)))
            # (several expected entries under one key: the same state handed in by several launches — any of their words)
            if sets is not None and not any(int(tabs[1][i]) in s for s in sets):
                bad.append(int(i))
        if bad:
            out.append(f"clause 5: the predecessor word of slot {bad[0]}, {int(tabs[1][bad[0]]):#x}, is none its entry's copies carried "
                       f"({len(bad)} such slots)")
    return out


def check_seen_set(image, pred_image, cap, shape, expected):
    v = seen_set_violations(image, pred_image, cap, shape, expected)
    return v[0] if v else None


# -- what the cases put in (chosen here, on the CPU; tests/test_seen_set_ref_cpu.py checks their preconditions) -------------
def real_expected(reduced=False):
    """expected_rows of Init and the six states of the expanded level (their predecessor: 0, and Init's fingerprint)"""
    rows = real_states()
    fp = fingerprint(rows)
    if reduced:   # (the predecessor word of such a build is the parent's unreduced fingerprint: not judged)
        return expected_rows(reduce_fp(fp), check_word(rows))
    return expected_rows(fp, check_word(rows), [frozenset([0])] + [frozenset([int(fp[0])])] * 6)


def last_groups(cap, n=1):
    return set(range((cap >> 6) - n, cap >> 6))


@functools.lru_cache(maxsize=None)
def wrap_case(cap):
    """200 states homed in the last group (a group holds 64: the chain runs over the end of the table) and 50 more, absent"""
    states, fp = select_homed(250, cap, last_groups(cap), 2, seed=cap)
    copies = np.random.default_rng(cap).integers(1, 9, size=200)
    return states[:200], fp[:200], copies, states[200:]


@functools.lru_cache(maxsize=None)
def spread_case(cap, n_last, n_spread, seed):
    """n_last states homed in the last two groups and n_spread anywhere"""
    a, fa = select_homed(n_last, cap, last_groups(cap, 2), 2, seed=seed)
    b, fb = select_homed(n_spread, cap, None, 2, seed=seed, first=int(index_of(a)[-1]) + 1)
    return np.concatenate([a, b]), np.concatenate([fa, fb])


@functools.lru_cache(maxsize=None)
def fill_case(cap, n):
    """n states anywhere: for the fills of the smallest table"""
    return select_homed(n, cap, None, 2, seed=7 * cap)


@functools.lru_cache(maxsize=None)
def collision_case(cap=1024, n=300, values=3):
    """n distinct states that share `values` reduced fingerprints (-DKMC_TEST_FP_BITS), all homed in the last group by the
    mirror and none the reduced fingerprint of a real state; (states, reduced fingerprints)"""
    every = reduce_fp(np.arange(1 << TEST_FP_BITS, dtype=U64))
    taken = set(reduce_fp(fingerprint(real_states())).tolist())
    want = [int(r) for r in every if int(rr.slot_of(int(r), cap)) >> 6 == (cap >> 6) - 1 and int(r) not in taken][:values]
    assert len(want) == values
    want = np.array(want, dtype=U64)
    fp_of = lambda s: reduce_fp(fingerprint(s))
    return select_homed(n, cap, last_groups(cap), 2, seed=1010, fp_of=fp_of, keep=lambda fp: np.isin(fp, want))


# -- the checkpoint file (csrc/kmc_engine_step.cpp) ------------------------------------------------------------------------
CKPT_MAGIC = b"KMCCKPT7"
CKPT_TAIL_WORDS = ("table_cap", "fcap", "seg_cap", "level", "n_cur", "n_levels", "w", "has_pred", "layout_form", "canon_form")


def ckpt_header_bytes():
    from kafka_specification_amd import _native as nat
    return 8 + C.sizeof(nat.KmcConfig) + 8 * len(CKPT_TAIL_WORDS)


def ckpt_sizes(shape, cap, W, n_levels, n_cur):
    """Bytes of the parts of a checkpoint, in the file's order: header, result, level sizes, segment sizes, Init, the table,
    the predecessor table (0 when there is none of its own), the frontier's planes"""
    from kafka_specification_amd import _native as nat
    _wide, _trace, stride, pred_apart, _ = SHAPES[shape]
    return [ckpt_header_bytes(), C.sizeof(nat.KmcResult), 8 * n_levels, 8 * SEGS, 8 * W, 8 * cap * stride, 8 * cap if pred_apart else 0,
            8 * n_cur * W]


def split_image(shape, cap, table_words, pred_words):
    """(image, pred_image) as the predicate takes them, from the words of the file"""
    if shape == "paired":
        return table_words[0::2].copy(), table_words[1::2].copy()
    return table_words, pred_words


def read_checkpoint(path, shape, cap, W, n_levels, n_cur):
    """(image, pred_image) of the table in a checkpoint, located from the end of the file by the known sizes; the header's own
    words must agree with them."""
    blob = open(path, "rb").read()
    sizes = ckpt_sizes(shape, cap, W, n_levels, n_cur)
    assert len(blob) == sum(sizes), (len(blob), sizes)
    assert blob[:8] == CKPT_MAGIC
    tail = np.frombuffer(blob, dtype=U64, count=len(CKPT_TAIL_WORDS), offset=sizes[0] - 8 * len(CKPT_TAIL_WORDS))
    hd = dict(zip(CKPT_TAIL_WORDS, (int(x) for x in tail)))
    form = {"narrow": 0, "paired": 2, "wide": 1}[shape]
    assert (hd["table_cap"], hd["n_cur"], hd["n_levels"], hd["w"], hd["has_pred"]) == (cap, n_cur, n_levels, W, form), hd
    end = len(blob) - sizes[7]
    pred = np.frombuffer(blob, dtype=U64, count=sizes[6] // 8, offset=end - sizes[6]).copy() if sizes[6] else None
    table = np.frombuffer(blob, dtype=U64, count=sizes[5] // 8, offset=end - sizes[6] - sizes[5]).copy()
    return split_image(shape, cap, table, pred)


# -- one level through the level-step ABI (GPU tests only) ----------------------------------------------------------------
def open_checker(shape, cap, frontier_capacity=1 << 16, **kw):
    from kafka_specification_amd import CheckerConfig, ModelChecker
    wide, trace = SHAPES[shape][:2]
    return ModelChecker(CheckerConfig(**CONSTANTS, table_capacity=cap, frontier_capacity=frontier_capacity, wide_fingerprint=wide,
                                      keep_trace=trace, **kw))


class OneLevel:
    """kmc_step_begin, ONE kmc_step_expand (the real level of six states), then any number of insert() launches of records
    into k_insert, then finish().  A frontier that holds synthetic states is never expanded."""

    def __init__(self, mc):
        import torch
        from kafka_specification_amd import _native as nat
        self.mc, self.nat, self.lib, self.torch = mc, nat, nat.lib(), torch
        self.keep = []                                  # (the records stay on the device until the level is finished)
        nat.check(self.lib.kmc_step_begin(mc._h))
        nat.check(self.lib.kmc_step_expand(mc._h, None))
        torch.cuda.synchronize()

    def insert(self, recs):
        recs = np.ascontiguousarray(recs, dtype=U64)
        assert recs.ndim == 2 and recs.shape[1] == self.mc.state_words + (1 if self.mc.cfg.keep_trace else 0) and len(recs)
        dev = self.torch.from_numpy(recs.view(np.int64)).to("cuda:0")
        self.torch.cuda.synchronize()
        self.keep.append(dev)
        self.nat.check(self.lib.kmc_step_insert(self.mc._h, C.c_void_p(dev.data_ptr()), len(recs)))

    def finish(self):
        info = self.nat.KmcLevelInfo()
        self.nat.check(self.lib.kmc_step_finish(self.mc._h, C.byref(info)))
        self.keep.clear()
        return info

    def image(self, tmp_path, shape, cap):
        """(image, pred_image) of the table after finish(): the level limit as verdict, a checkpoint, the table out of its file"""
        self.nat.check(self.lib.kmc_step_set_verdict(self.mc._h, V_LEVEL_LIMIT))
        path = os.path.join(str(tmp_path), f"seen_set_{shape}_{cap}.ckpt")
        self.mc.save_checkpoint(path)
        n_cur = len(self.mc.frontier_states())
        got = read_checkpoint(path, shape, cap, self.mc.state_words, 2, n_cur)
        os.remove(path)
        return got


def pred_of(mc, fp):
    """(found, predecessor word) of the host's lookup of fp (kmc_pred_of)"""
    from kafka_specification_amd import _native as nat
    pred, found = C.c_uint64(), C.c_int32()
    nat.check(nat.lib().kmc_pred_of(mc._h, int(fp), C.byref(pred), C.byref(found)))
    return bool(found.value), int(pred.value)
