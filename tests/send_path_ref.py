"""Reference side of the sharded send path (csrc/kmc_sink.h, KmcSink::process<KMC_MODE_SHARDED>: owner bucketing, the sender-side
filter first_time, the overflow of a sub-buffer), in plain Python and numpy: the level-by-level search of seen_set_ref.CONSTANTS
with the device's own model templates as g++ compiles them (tests/host_emu.py) and seen_set_ref's fingerprint; kmc_owner; what
the send area of shard s of P must hold after ONE k_expand over a given frontier; the mirror of first_time and the runs of a
finished filter image; and the predicate a send area is judged by.  Which lane gets which position of a run, and which copy of
a state passes the filter, is not deterministic: the predicate says what all correct send areas have in common.  Importable
without a GPU: tests/test_send_path_ref_cpu.py holds it to the headers and to one mutant per clause and checks every
precondition of tests/test_gpu_send_path_direct.py, which uses it."""
import collections
import ctypes as C
import functools

import numpy as np

import host_emu
import seen_set_ref as sr

U64 = np.uint64
W = 2                                    # words of a state at seen_set_ref.CONSTANTS
SEGS = sr.SEGS                           # KMC_SEGS = KMC_SEND_SUBS: block b of k_expand fills sub-buffer b % SEGS
ERR_SEND_FULL = 4                        # KMC_ERR_SEND_FULL
POISON = 0xA5A5A5A5A5A5A5A5              # what a test fills a send area with before kmc_step_expand: no state word, no fingerprint
POISON_I64 = POISON - (1 << 64)
BLOCK_STATES = 256                       # expand_grid: one block of four waves per 256 frontier states (plain search)
BLOCK_STATES_SYMMETRY = 16               # ... per 16 under orbit counting (tiles of 4)
FILTER_PROBES = 64                       # first_time: a chain longer than this answers "fresh"
FILTER_SHIFT = 17                        # first_time: the index is (fp >> 17) & mask
MODES = ("exact", "filtered", "saturated", "overflowed")


def cfg6():
    from kafka_specification_amd import _native as nat
    c = sr.CONSTANTS
    return (nat.MODELS[c["model"]], c["n_replicas"], c["log_size"], c["max_records"], c["max_leader_epoch"], 0)


def owner(fp, P):
    """kmc_owner, on Python ints or uint64 arrays"""
    if isinstance(fp, np.ndarray):
        return ((((fp >> U64(40)) & U64(0xFFFFFF)) * U64(P)) >> U64(24)).astype(np.int64)
    return (((int(fp) >> 40) & 0xFFFFFF) * P) >> 24


def pow2_floor(x):
    return 1 << (int(x).bit_length() - 1)


def sent_cap(table_cap):
    """slots of the sender-side filter of a shard opened with that table capacity (kmc_engine_open.cpp)"""
    return pow2_floor(2 * ((table_cap + 63) // 64 * 64))


# -- the search --------------------------------------------------------------------------------------------------------------
def bindings(c6, state):
    """([(kind, successor)] with one entry per enabled binding of Next, the number TLC generates).  host_emu.successors lists a
    binding whose two disjuncts yield the same successor (Kip320.tla:82-83, the templates' `extra`, 0 or 1) twice in a row:
    k_expand counts it twice in `generated` and sends it into the sink ONCE."""
    lst = host_emu.successors(c6, state, cap=256)
    out, i = [], 0
    while i < len(lst):
        out.append(lst[i])
        i += 2 if i + 1 < len(lst) and lst[i + 1] == lst[i] else 1
    return out, len(lst)


Level = collections.namedtuple("Level", "states fp row parent kind words rfp generated")
# states (n, W): the level's states, representatives under orbit counting; fp (n,); row: state tuple -> its index;
# one record per binding of every state: parent (its state's index), kind, words (m, W: what travels), rfp (m,) its fingerprint;
# generated: what TLC counts for the level (the repeated disjuncts included)


@functools.lru_cache(maxsize=None)
def search(symmetry=False, max_levels=None):
    """The breadth-first search, level by level, as a tuple of Level; under `symmetry` the search over orbit representatives
    (host_emu.canon, the device's compile-time form), `max_levels` of it at the most."""
    c6 = cfg6()
    canon_of = {}

    def shipped(t):
        if not symmetry:
            return t
        if t not in canon_of:
            stab, rep = host_emu.canon(c6, t)
            assert stab > 0
            canon_of[t] = rep
        return canon_of[t]

    init = shipped(tuple(host_emu.init(c6)))
    cur, seen, out = [init], {init}, []
    while cur and (max_levels is None or len(out) < max_levels):
        parent, kind, words, generated = [], [], [], 0
        for i, s in enumerate(cur):
            recs, n = bindings(c6, s)
            generated += n
            for k, t in recs:
                parent.append(i)
                kind.append(k)
                words.append(shipped(t))
        states = np.array(cur, dtype=U64).reshape(len(cur), W)
        wa = np.array(words, dtype=U64).reshape(len(words), W)
        out.append(Level(states, sr.fingerprint(states), {s: i for i, s in enumerate(cur)}, np.array(parent, dtype=np.int64),
                         np.array(kind, dtype=np.int64), wa, sr.fingerprint(wa), generated))
        nxt = []
        for t in words:
            if t not in seen:
                seen.add(t)
                nxt.append(t)
        cur = nxt
    return tuple(out)


def owned(level, P, shard):
    """indices of the level's states shard `shard` of P owns"""
    return np.flatnonzero(owner(level.fp, P) == shard)


def frontier_rows(level, frontier):
    """indices of the states of a frontier read from the GPU; raises on a state the level does not hold, or holds twice"""
    rows = [level.row[tuple(int(x) for x in s)] for s in np.asarray(frontier, dtype=U64)]
    assert len(set(rows)) == len(rows), "a frontier holds a state twice"
    return np.array(rows, dtype=np.int64)


def expected_sends(level, P, shard, rows, trace):
    """(per destination the records shard `shard` of P must send when it expands the states `rows` of `level`, as (n, W[+1])
    arrays in no particular order — the last word the parent's fingerprint when traces are kept; the number of records that
    stay on the shard)."""
    pick = np.flatnonzero(np.isin(level.parent, rows))
    recs = np.zeros((len(pick), W + (1 if trace else 0)), dtype=U64)
    recs[:, :W] = level.words[pick]
    if trace:
        recs[:, W] = level.fp[level.parent[pick]]
    dst = owner(level.rfp[pick], P) if len(pick) else np.zeros(0, dtype=np.int64)
    return [recs[dst == d] if d != shard else recs[:0] for d in range(P)], int((dst == shard).sum())


def remote_counts(level, P, shard):
    """records per destination of the states the shard owns (0 for itself)"""
    sends, _ = expected_sends(level, P, shard, owned(level, P, shard), False)
    return [len(x) for x in sends]


# -- first_time's mirror ---------------------------------------------------------------------------------------------------
class Filter:
    """KmcSink::first_time, one caller at a time"""

    def __init__(self, cap):
        assert cap & (cap - 1) == 0
        self.mask, self.set = cap - 1, [0] * cap

    def first_time(self, fp):
        i = (fp >> FILTER_SHIFT) & self.mask
        for _ in range(FILTER_PROBES):
            if self.set[i] == 0:
                self.set[i] = fp
                return True
            if self.set[i] == fp:
                return False
            i = (i + 1) & self.mask
        return True


def filter_occupied(fps, cap):
    """Which slots a filter of `cap` slots would hold had every one of the distinct fingerprints `fps` found a place: as
    seen_set_ref.occupied, with first_time's index.  The occupied set of linear probing does not depend on the order of the
    inserts and only grows, so its longest run bounds every chain any interleaving of the lanes can meet."""
    fps = np.unique(np.asarray(fps, dtype=U64))
    assert len(fps) <= cap and cap & (cap - 1) == 0
    count = np.bincount(((fps >> U64(FILTER_SHIFT)) & U64(cap - 1)).astype(np.int64), minlength=cap).tolist()
    taken, carry = bytearray(cap), 0
    for _round in range(2):
        for i in range(cap):
            carry += count[i]
            count[i] = 0
            if not taken[i] and carry:
                taken[i] = 1
                carry -= 1
    assert carry == 0 and sum(taken) == len(fps)
    return np.frombuffer(bytes(taken), dtype=np.uint8).astype(bool)


def filter_longest_run(fps, cap):
    return sr.longest_cyclic_run(filter_occupied(fps, cap))


def remote_fingerprints(levels, P, shard):
    """every fingerprint shard `shard` of P generates for another shard over the levels, with repeats, in the search's order"""
    out = []
    for lv in levels:
        pick = np.flatnonzero(np.isin(lv.parent, owned(lv, P, shard)))
        fp = lv.rfp[pick]
        out.append(fp[owner(fp, P) != shard] if len(fp) else fp)
    return np.concatenate(out)


# -- the predicate ---------------------------------------------------------------------------------------------------------
def shipped_records(send, counts, d):
    """the first counts[d][sb] records of destination d's sub-buffers, one after the other"""
    cap = send.shape[2]
    return np.concatenate([send[d, sb, :min(int(counts[d, sb]), cap)] for sb in range(send.shape[1])])


def shipped_fingerprints(send, counts, shard):
    send = np.asarray(send).view(U64)
    counts = np.asarray(counts, dtype=np.int64)
    recs = np.concatenate([shipped_records(send, counts, d) for d in range(send.shape[0]) if d != shard])
    return set(sr.fingerprint(recs[:, :W]).tolist()) if len(recs) else set()


def _bag(rows):
    return collections.Counter(map(tuple, np.asarray(rows).tolist()))


def send_area_violations(send, counts, expected, shard, mode, shipped_before=frozenset()):
    """Every clause the send area of shard `shard` violates after one kmc_step_expand, as text, in the order of the clauses.
    send: the whole tensor [destination][sub-buffer][record][word], filled with POISON before the launch; counts: the published
    counts [destination][sub-buffer]; expected: expected_sends' list — every record the expansion GENERATES per destination;
    shipped_before (filtered, saturated): the fingerprints this shard shipped on earlier levels.
      1  the shard's own destination: counts 0, every word poison
      2  no count beyond the capacity; every word past a count is poison
      3  every record lies in the buffer of the shard that owns its fingerprint
      4  filtered: no two records of one fingerprint
      5  filtered: no fingerprint that was shipped on an earlier level
      6  records per destination: exact — the generated ones; filtered — one per fingerprint not shipped before; saturated —
         between those two; overflowed — the generated ones unless a sub-buffer of the destination is full, never more
      7  the states: exact — the generated multiset; overflowed, saturated — a sub-multiset of it; filtered, saturated — no
         fingerprint that was never shipped is missing, none is there that was not generated
      8  the parent words (traces): every record is a generated (state, parent) pair, as often at the most as it was generated"""
    assert mode in MODES
    send = np.asarray(send).view(U64)
    counts = np.asarray(counts, dtype=np.int64)
    P, subs, cap, RW = send.shape
    assert counts.shape == (P, subs) and len(expected) == P and 0 <= shard < P
    out = []
    if counts[shard].any():
        out.append(f"clause 1: shard {shard} publishes {int(counts[shard].sum())} records for itself")
    elif (send[shard] != U64(POISON)).any():
        sb, r, w = (int(x[0]) for x in np.nonzero(send[shard] != U64(POISON)))
        out.append(f"clause 1: the shard's own destination {shard} was written: sub-buffer {sb} record {r} word {w} holds {int(send[shard, sb, r, w]):#x}")
    for d in range(P):
        for sb in range(subs):
            if d == shard:
                continue
            c = int(counts[d, sb])
            if c > cap:
                out.append(f"clause 2: destination {d} sub-buffer {sb}: a count of {c} for {cap} records")
                break
            tail = send[d, sb, c:] != U64(POISON)
            if tail.any():
                r, w = (int(x[0]) for x in np.nonzero(tail))
                out.append(f"clause 2: destination {d} sub-buffer {sb}: word {w} of record {c + r}, past the count {c}, holds {int(send[d, sb, c + r, w]):#x}")
                break
        else:
            continue
        break
    got = [shipped_records(send, counts, d) if d != shard else send[d, 0, :0] for d in range(P)]
    got_fp = [sr.fingerprint(g[:, :W]) if len(g) else np.zeros(0, dtype=U64) for g in got]
    exp_fp = [sr.fingerprint(np.asarray(e)[:, :W]) if len(e) else np.zeros(0, dtype=U64) for e in expected]
    for d in range(P):
        bad = np.flatnonzero(owner(got_fp[d], P) != d) if len(got[d]) else []
        if len(bad):
            k = int(bad[0])
            out.append(f"clause 3: destination {d} holds the state {[hex(int(x)) for x in got[d][k, :W]]}, which shard {owner(int(got_fp[d][k]), P)} owns ({len(bad)} such records)")
            break
    if mode == "filtered":
        every = np.concatenate(got_fp)
        vals, n = np.unique(every, return_counts=True)
        if (n > 1).any():
            out.append(f"clause 4: {int((n > 1).sum())} fingerprint(s) shipped more than once in one level, first {int(vals[n > 1][0]):#x} ({int(n[n > 1][0])} records)")
        again = sorted(set(every.tolist()) & set(shipped_before))
        if again:
            out.append(f"clause 5: {len(again)} fingerprint(s) shipped on an earlier level shipped again, first {again[0]:#x}")
    for d in range(P):
        if d == shard:
            continue
        n_got, n_gen = len(got[d]), len(expected[d])
        n_new = len(set(exp_fp[d].tolist()) - set(shipped_before))
        if mode == "exact" and n_got != n_gen:
            out.append(f"clause 6: destination {d} received {n_got} records, {n_gen} were generated for it")
        elif mode == "filtered" and n_got != n_new:
            out.append(f"clause 6: destination {d} received {n_got} records for {n_new} fingerprints not shipped before")
        elif mode == "saturated" and not n_new <= n_got <= n_gen:
            out.append(f"clause 6: destination {d} received {n_got} records: {n_new} fingerprints not shipped before, {n_gen} generated")
        elif mode == "overflowed" and (n_got > n_gen or (n_got < n_gen and not (counts[d] == cap).any())):
            out.append(f"clause 6: destination {d} received {n_got} of {n_gen} records and none of its sub-buffers is full ({cap})")
        else:
            continue
        break
    for d in range(P):
        if d == shard:
            continue
        have, want = _bag(got[d][:, :W]), _bag(np.asarray(expected[d])[:, :W]) if len(expected[d]) else collections.Counter()
        said = None
        missing = sorted(set(exp_fp[d].tolist()) - set(shipped_before) - set(got_fp[d].tolist())) if mode in ("filtered", "saturated") else []
        if missing:
            said = f"{len(missing)} fingerprint(s) never shipped are missing, first {missing[0]:#x}"
        elif mode == "exact" and have != want:
            t = sorted((have - want) + (want - have))[0]
            said = f"the state {[hex(x) for x in t]} is there {have[t]} times, generated {want[t]} times"
        elif mode in ("overflowed", "saturated") and have - want:
            t = sorted(have - want)[0]
            said = f"the state {[hex(x) for x in t]} is there {have[t]} times, generated {want[t]} times"
        elif mode == "filtered" and set(have) - set(want):
            said = f"the state {[hex(x) for x in sorted(set(have) - set(want))[0]]} was not generated"
        if said:
            out.append(f"clause 7: destination {d}: {said}")
            break
    if RW > W:
        for d in range(P):
            if d == shard or not len(got[d]):
                continue
            have, want = _bag(got[d]), _bag(expected[d]) if len(expected[d]) else collections.Counter()
            over = (have - want) if mode != "exact" else (have - want) + (want - have)
            if over:
                t = sorted(over)[0]
                out.append(f"clause 8: destination {d}: the record {[hex(x) for x in t[:W]]} with parent {t[W]:#x} is there {have[t]} times, "
                           f"generated {want[t]} times")
                break
    return out


def check_send_area(send, counts, expected, shard, mode, shipped_before=frozenset()):
    """the first discrepancy as text, or None"""
    v = send_area_violations(send, counts, expected, shard, mode, shipped_before)
    return v[0] if v else None


# -- what the GPU cases rest on (chosen here, on the CPU; tests/test_send_path_ref_cpu.py checks every one) -------------------
SHARDS = (2, 3, 8)                       # case A
ROOMY = dict(table_capacity=1 << 16, frontier_capacity=1 << 15)   # per shard; the filter of such a shard has 2^17 slots
ROOMY_SEND = {1: 64, 2: 4096, 3: 2048, 8: 512}     # records per sub-buffer: ONE holds all a shard sends a destination in a level
# case C: 8 shards with the filter forced on; 127 groups of 64 slots -> a filter of pow2_floor(2 x 8128) = 8192 slots
SATURATED = dict(table_capacity=64 * 127, frontier_capacity=1 << 13)
# case D: the shard and level (0 = Init's) at P = 2 whose frontier fits one block and sends the most records
OVERFLOW_P = 2


@functools.lru_cache(maxsize=None)
def overflow_case():
    """(shard, level, destination, n): of the (shard, level) at OVERFLOW_P whose frontiers fit one block, the one with the most
    records for the other shard"""
    best = None
    for k, lv in enumerate(search()):
        for s in range(OVERFLOW_P):
            if 64 < len(owned(lv, OVERFLOW_P, s)) <= BLOCK_STATES:
                n = remote_counts(lv, OVERFLOW_P, s)
                d = int(np.argmax(n))
                if best is None or n[d] > best[3]:
                    best = (s, k, d, n[d])
    return best


# -- the driver (GPU tests only) -------------------------------------------------------------------------------------------
class Shards:
    """P HipShardEngine(native=False) on one device, stepped level by level: begin(); then per level expand() — every send area
    poisoned, one kmc_step_expand per shard, counts and whole tensors read back — route() of the filled slices to their owners'
    insert, and finish()."""

    def __init__(self, P, send_capacity=None, **cfg):
        import torch
        from kafka_specification_amd import CheckerConfig, _native as nat
        from kafka_specification_amd.sharded import HipShardEngine
        self.torch, self.nat, self.lib, self.P = torch, nat, nat.lib(), P
        base = CheckerConfig(**{**sr.CONSTANTS, **ROOMY, **cfg}, send_capacity=send_capacity or ROOMY_SEND[P])
        self.engines = []
        try:
            for s in range(P):
                self.engines.append(HipShardEngine(base, s, P, 0, native=False))
        except Exception:
            self.close()
            raise
        self.level = 0          # the level the shards hold, unexpanded (0: Init's)
        self.counts = self.sends = None

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def begin(self):
        for e in self.engines:
            e.begin()

    def frontiers(self):
        return [e.mc.frontier_states() for e in self.engines]

    def expand_one(self, s, send=None):
        """poison, kmc_step_expand, read back: (counts [P][SEGS], the area as uint64 [P][SEGS][cap][RW]) of shard s"""
        e = self.engines[s]
        send = e.send if send is None else send
        send.fill_(POISON_I64)
        self.torch.cuda.synchronize()
        c = (C.c_uint64 * (self.nat.KMC_MAX_SHARDS * SEGS))()
        self.nat.check(self.lib.kmc_step_expand(e.mc.handle, c))
        self.torch.cuda.synchronize()
        counts = np.array(c[:], dtype=np.int64).reshape(self.nat.KMC_MAX_SHARDS, SEGS)
        assert not counts[self.P:].any()
        return counts[:self.P].copy(), send.cpu().numpy().view(U64)

    def expand(self):
        got = [self.expand_one(s) for s in range(self.P)]
        self.counts, self.sends = [g[0] for g in got], [g[1] for g in got]
        return self.counts, self.sends

    def route(self, areas=None):
        """every filled slice to its owner's k_insert (`areas`: the device tensors to route from, the engines' own by default)"""
        for s, e in enumerate(self.engines):
            area = e.send if areas is None or areas[s] is None else areas[s]
            for d in range(self.P):
                for sb in range(SEGS):
                    n = min(int(self.counts[s][d, sb]), area.shape[2])
                    if n and d != s:
                        self.engines[d].insert(area[d, sb, :n])

    def finish(self):
        """-> the shards' kmc_level_info of the level just expanded"""
        infos = []
        for e in self.engines:
            info = self.nat.KmcLevelInfo()
            self.nat.check(self.lib.kmc_step_finish(e.mc.handle, C.byref(info)))
            infos.append(info)
        self.level += 1
        return infos

    def step(self):
        self.expand()
        self.route()
        return self.finish()
