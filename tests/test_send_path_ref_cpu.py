"""tests/send_path_ref.py is what tests/test_gpu_send_path_direct.py judges the sharded send path by, so it is held to account
here, without a GPU: its owner function against the library's kmc_owner_of and the header's line; its search against the
exhaustive oracle; its mirror of the sender-side filter against the text of first_time; its predicate against correct send
areas and one mutant per clause; and every precondition a GPU case rests on — frontiers of more than one block, sub-buffers no
placement of the blocks can overflow, filters that stay roomy, the filter that saturates, the level of the overflow case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_emu
import seen_set_ref as sr
import send_path_ref as sp
from kafka_specification_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_specification_amd", "csrc")
U64 = np.uint64
W = sp.W


def _source(name):
    return open(os.path.join(CSRC, name)).read()


# -- the mirrors -----------------------------------------------------------------------------------------------------------
def test_owner_is_the_librarys_on_random_fingerprints_and_on_the_edges_of_its_window():
    lib = nat.lib()
    assert "return (u32)((((fp >> 40) & 0xFFFFFFull) * (u64)nshards) >> 24);" in _source("kmc_common.h")
    rng = np.random.default_rng(24)
    for P in range(1, nat.KMC_MAX_SHARDS + 1):
        fps = rng.integers(0, 1 << 63, size=2000, dtype=U64) * U64(2) + rng.integers(0, 2, size=2000, dtype=U64)
        edges = []
        for d in range(P + 1):   # the first window value of every destination, the last of the one before, under any low 40 bits
            first = -(-(d << 24) // P)
            for x in (first - 1, first, first + 1):
                if 0 <= x < 1 << 24:
                    edges += [x << 40, (x << 40) | ((1 << 40) - 1), (x << 40) | 0x5A5A5A5A5A]
        fps = np.concatenate([fps, np.array(edges + [0, 1, (1 << 64) - 1, (1 << 40) - 1, 1 << 40], dtype=U64)])
        want = [int(lib.kmc_owner_of(C.c_uint64(int(f)), P)) for f in fps]
        assert sp.owner(fps, P).tolist() == want == [sp.owner(int(f), P) for f in fps]
        assert set(want) == set(range(P)) and want[-3] == P - 1 and want[-2] == 0


def test_the_filters_mirror_is_the_text_of_first_time():
    """first_time sits in the device-only part of csrc/kmc_sink.h (below #ifndef KMC_HOST_EMU: it uses atomicCAS), so g++ cannot
    compile it: the mirror is held to its text here and the function itself to GPU case B (roomy) and C (saturated).  The
    adversarial input: a run of 64 occupied slots that ends at the mask's wrap."""
    sink = _source("kmc_sink.h")
    body = re.search(r"static KMC_DEV bool first_time\(u64\* set, u64 mask, u64 fp\) \{(.*?)\n    \}\n", sink, re.S)
    assert body and sink.index("#ifndef KMC_HOST_EMU") < body.start()
    assert f"u64 i = (fp >> {sp.FILTER_SHIFT}) & mask;" in body.group(1) and f"probes < {sp.FILTER_PROBES}; ++probes" in body.group(1)
    assert "i = (i + 1) & mask;" in body.group(1) and body.group(1).rstrip().endswith("return true;")
    assert "h->sent_cap = pow2_floor(tcap * 2);" in _source("kmc_engine_open.cpp")
    assert sp.sent_cap(1 << 16) == 1 << 17 and sp.sent_cap(64 * 127) == 8192 and sp.sent_cap(1000) == 2048
    cap = 256
    at = lambda home, k: ((k + 1) << 40) | (home << sp.FILTER_SHIFT) | 1     # distinct fingerprints homed at `home`
    f = sp.Filter(cap)
    assert all(f.first_time(at(cap - 64, k)) for k in range(64))
    assert all(f.set[cap - 64:]) and not any(f.set[:cap - 64])                # the run of 64, up to the last slot
    assert not f.first_time(at(cap - 64, 63))                                 # the 64th probe still finds its entry
    late = at(cap - 64, 100)
    assert f.first_time(late) and f.first_time(late) and late not in f.set    # a chain of 64 answers "fresh", every time
    wraps = at(cap - 63, 7)
    assert f.first_time(wraps) and f.set[0] == wraps and not f.first_time(wraps)   # 63 probes, then slot 0 over the wrap
    assert sp.filter_longest_run([x for x in f.set if x], cap) == 65
    # random fingerprints in a roomy filter: first_time is "not seen before", whatever the order, and the occupied set is the sweep's
    rng = np.random.default_rng(3)
    fps = rng.integers(1, 1 << 62, size=300, dtype=U64).tolist()
    order = fps + [fps[i] for i in rng.integers(0, 300, size=500)]
    rng.shuffle(order)
    f, seen = sp.Filter(1024), set()
    for fp in order:
        assert f.first_time(fp) == (fp not in seen)
        seen.add(fp)
    assert np.array_equal(np.array(f.set) != 0, sp.filter_occupied(fps, 1024)) and sp.filter_longest_run(fps, 1024) < sp.FILTER_PROBES


# -- the search --------------------------------------------------------------------------------------------------------------
def test_the_search_is_the_oracles_level_by_level():
    import kmo
    rows, levels = sr.reachable()
    lv = sp.search()
    assert tuple(len(l.states) for l in lv) == levels and len(lv) <= 30
    at = np.concatenate([[0], np.cumsum(levels)])
    for k, l in enumerate(lv):
        assert set(map(tuple, l.states.tolist())) == set(map(tuple, rows[at[k]:at[k + 1]].tolist())), f"level {k}"
        assert np.array_equal(l.fp, sr.fingerprint(l.states)) and np.array_equal(l.rfp, sr.fingerprint(l.words))
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=2, R=2, E=1, invariants=()))
    assert 1 + sum(l.generated for l in lv) == o.generated
    # a binding whose two disjuncts coincide is generated twice and sent once: such pairs exist, and all are of one action
    c6 = sp.cfg6()
    pairs, kinds = 0, set()
    for l in lv[:12]:
        for s in l.states.tolist():
            lst = host_emu.successors(c6, s, cap=256)
            recs, n = sp.bindings(c6, s)
            assert n == len(lst) and len(recs) <= n <= 2 * len(recs)
            for a, b in zip(lst, lst[1:]):
                if a == b:
                    pairs += 1
                    kinds.add(a[0])
    assert pairs > 0 and len(kinds) == 1
    assert sum(l.generated - len(l.words) for l in lv[:12]) == pairs


def test_the_search_over_representatives_weighs_to_the_plain_one():
    c6 = sp.cfg6()
    plain, sym = sp.search(), sp.search(True)
    assert len(sym) == len(plain)
    for a, b in zip(plain, sym):
        orbit = 0
        for s in b.states.tolist():
            stab, rep = host_emu.canon(c6, s)
            assert rep == tuple(s) and 6 % stab == 0
            orbit += 6 // stab
        assert orbit == len(a.states)
        assert all(host_emu.canon(c6, t)[1] == tuple(t) for t in b.words[::7].tolist())   # what travels is a representative


# -- what the GPU cases rest on ----------------------------------------------------------------------------------------------
def test_expand_grid_is_one_block_per_256_states_and_per_16_under_orbit_counting():
    core = _source("kmc_engine_core.cpp")
    assert "const uint64_t per_tile = h->cfg.symmetry ? 4 : 64;" in core and "(tiles + KMC_WAVES - 1) / KMC_WAVES" in core
    assert "#define KMC_BLOCK 256" in _source("kmc_kernels.h") and "#define KMC_WAVES (KMC_BLOCK / 64)" in _source("kmc_kernels.h")
    assert (sp.BLOCK_STATES, sp.BLOCK_STATES_SYMMETRY) == (64 * 4, 4 * 4)
    assert "const u32 sub = blockIdx.x % KMC_SEGS;" in _source("kmc_sink.h") and sp.SEGS == nat.KMC_SEND_SUBS == 8
    assert re.search(r"#define KMC_ERR_SEND_FULL %du\b" % sp.ERR_SEND_FULL, _source("kmc_common.h"))


@pytest.mark.parametrize("symmetry", [False, True], ids=["plain", "orbits"])
@pytest.mark.parametrize("P", sp.SHARDS)
def test_case_a_some_frontier_takes_two_blocks_and_no_sub_buffer_can_overflow(P, symmetry):
    lv = sp.search(symmetry)
    per_block = sp.BLOCK_STATES_SYMMETRY if symmetry else sp.BLOCK_STATES
    widest = max(len(sp.owned(l, P, s)) for l in lv for s in range(P))
    assert widest > per_block                              # at least two blocks, i.e. two sub-buffers
    most = max(max(sp.remote_counts(l, P, s)) for l in lv for s in range(P))
    print(f"P {P}: widest frontier of a shard {widest}, most records for one destination in one level {most}")
    assert 0 < most <= sp.ROOMY_SEND[P]                    # wherever the blocks put them
    assert widest <= sp.ROOMY["frontier_capacity"] // sp.SEGS          # ... and a level fits ONE segment of the frontier
    total = max(sum(len(sp.owned(l, P, s)) for l in lv) for s in range(P))
    assert total < 0.5 * sp.ROOMY["table_capacity"]
    # every shard owns a part of every wide level, and the partition is one
    for l in lv:
        assert sum(len(sp.owned(l, P, s)) for s in range(P)) == len(l.states)


@pytest.mark.parametrize("P", [2, 3])
def test_case_b_the_filters_stay_roomy(P):
    cap = sp.sent_cap(sp.ROOMY["table_capacity"])
    for s in range(P):
        fps = sp.remote_fingerprints(sp.search(), P, s)
        run = sp.filter_longest_run(fps, cap)
        print(f"P {P} shard {s}: {len(fps)} remote successors, {len(set(fps.tolist()))} fingerprints in {cap} slots, longest run {run}")
        assert run < sp.FILTER_PROBES and len(set(fps.tolist())) < len(fps)   # no chain is cut; there is something to drop


def test_case_c_the_filter_saturates_and_the_seen_set_does_not():
    P, lv = 8, sp.search()
    tcap = sp.SATURATED["table_capacity"]
    cap = sp.sent_cap(tcap)
    assert tcap % 64 == 0 and cap == 8192
    saturated = 0
    for s in range(P):
        fps = sp.remote_fingerprints(lv, P, s)
        distinct = len(set(fps.tolist()))
        f = sp.Filter(cap)
        fresh = sum(f.first_time(int(x)) for x in fps)
        print(f"shard {s}: {distinct} fingerprints for {cap} slots; one caller at a time ships {fresh} of {len(fps)}")
        saturated += distinct > cap and fresh > distinct
        mine = np.concatenate([l.fp[sp.owned(l, P, s)] for l in lv])
        assert len(mine) < sr.LOAD_LIMIT * tcap and sr.longest_cyclic_run(sr.occupied(mine, tcap)) < sr.max_probes(tcap) // 2
        assert max(len(sp.owned(l, P, s)) for l in lv) <= sp.SATURATED["frontier_capacity"] // sp.SEGS
    assert saturated >= 1
    assert max(max(sp.remote_counts(l, P, s)) for l in lv for s in range(P)) <= sp.ROOMY_SEND[P]


def test_case_d_the_overflow_level_fits_one_block():
    s, k, d, n = sp.overflow_case()
    assert (s, k, d, n) == (1, 5, 0, 422)
    lv = sp.search()[k]
    rows = sp.owned(lv, sp.OVERFLOW_P, s)
    assert 64 < len(rows) <= sp.BLOCK_STATES and d != s      # one block, more than one of its waves: everything lands in sub-buffer 0
    sends, local = sp.expected_sends(lv, sp.OVERFLOW_P, s, rows, True)
    assert len(sends[d]) == n > 64 and sends[d].shape[1] == W + 1 and local > 0 and len(sends[s]) == 0
    assert set(sends[d][:, W].tolist()) <= set(lv.fp[rows].tolist())


# -- the predicate ---------------------------------------------------------------------------------------------------------
P_BASE, SHARD, LEVEL, CAP = 3, 1, 6, 48


def area_of(per_dest, seed=0, cap=CAP, trace=True):
    """(send, counts): the records spread over the sub-buffers of their destinations, the rest poison"""
    rng = np.random.default_rng(seed)
    RW = W + (1 if trace else 0)
    send = np.full((P_BASE, sp.SEGS, cap, RW), sp.POISON, dtype=U64)
    counts = np.zeros((P_BASE, sp.SEGS), dtype=np.int64)
    for d, recs in enumerate(per_dest):
        for r in rng.permutation(len(recs)):
            sb = int(rng.choice(np.flatnonzero(counts[d] < cap)))
            send[d, sb, counts[d, sb]] = recs[r]
            counts[d, sb] += 1
    return send, counts


def base(mode):
    """(send, counts, expected, shipped_before) of shard 1 of 3 at level 6, traces kept: a correct area of that mode"""
    lv = sp.search()
    expected, _ = sp.expected_sends(lv[LEVEL], P_BASE, SHARD, sp.owned(lv[LEVEL], P_BASE, SHARD), True)
    before = set(sp.remote_fingerprints(lv[:LEVEL], P_BASE, SHARD).tolist())
    if mode == "exact":
        return (*area_of(expected), expected, frozenset())
    once = []
    for recs in expected:       # one record, any of its copies, per fingerprint not shipped before
        fp = sr.fingerprint(recs[:, :W]) if len(recs) else np.zeros(0, dtype=U64)
        _, first = np.unique(fp, return_index=True)
        once.append(recs[[i for i in sorted(first) if int(fp[i]) not in before]])
    return (*area_of(once, seed=1), expected, frozenset(before))


def _records(send, counts, d):
    """(sub-buffer, record) of destination d's records"""
    return [(sb, r) for sb in range(sp.SEGS) for r in range(counts[d, sb])]


def m_moved_to_another_destinations_buffer(send, counts, expected):
    sb = int(np.flatnonzero(counts[0])[0])
    counts[0, sb] -= 1
    rec = send[0, sb, counts[0, sb]].copy()
    send[0, sb, counts[0, sb]] = sp.POISON
    sb2 = int(np.flatnonzero(counts[2] < CAP)[0])
    send[2, sb2, counts[2, sb2]] = rec
    counts[2, sb2] += 1


def m_overwritten_by_a_copy_of_its_neighbour(send, counts, expected):
    """two lanes with one `pos`: a record lost, another there twice, the counts those of a correct area"""
    sb = int(np.flatnonzero(counts[0] >= 2)[0])
    assert not np.array_equal(send[0, sb, 0, :W], send[0, sb, 1, :W])
    send[0, sb, 1] = send[0, sb, 0]


def m_parent_words_of_two_records_swapped(send, counts, expected):
    sb = int(np.flatnonzero(counts[2] >= 2)[0])
    r = next(r for r in range(1, counts[2, sb]) if send[2, sb, r, W] != send[2, sb, 0, W] and
             not np.array_equal(send[2, sb, r, :W], send[2, sb, 0, :W]))
    send[2, sb, 0, W], send[2, sb, r, W] = send[2, sb, r, W], send[2, sb, 0, W]


def m_record_removed_and_the_count_lowered(send, counts, expected):
    sb = int(np.flatnonzero(counts[2])[0])
    counts[2, sb] -= 1
    send[2, sb, counts[2, sb]] = sp.POISON


def m_word_written_just_past_a_count(send, counts, expected):
    """what a record written at `pos` = its count leaves behind (`pos <= a.send_cap` in a full sub-buffer: record 0 of the next)"""
    sb = int(np.flatnonzero(counts[0] < CAP)[0])
    send[0, sb, counts[0, sb], 1] = 0x1234


def m_word_written_into_the_own_destination(send, counts, expected):
    send[SHARD, 7, CAP - 1, W] = 0


def m_two_records_of_one_fingerprint(send, counts, expected):
    sb = int(np.flatnonzero((counts[0] > 0) & (counts[0] < CAP))[0])
    send[0, sb, counts[0, sb]] = send[0, sb, 0]
    counts[0, sb] += 1


def m_shipped_on_an_earlier_level_and_again(send, counts, expected, before):
    fp = sr.fingerprint(expected[2][:, :W])
    k = next(k for k in range(len(fp)) if int(fp[k]) in before)
    sb = int(np.flatnonzero(counts[2] < CAP)[0])
    send[2, sb, counts[2, sb]] = expected[2][k]
    counts[2, sb] += 1


# mutant -> (the mode it is judged in, the clause that speaks first)
MUTANTS = {
    m_word_written_into_the_own_destination: ("exact", 1),
    m_word_written_just_past_a_count: ("exact", 2),
    m_moved_to_another_destinations_buffer: ("exact", 3),
    m_two_records_of_one_fingerprint: ("filtered", 4),
    m_shipped_on_an_earlier_level_and_again: ("filtered", 5),
    m_record_removed_and_the_count_lowered: ("exact", 6),
    m_overwritten_by_a_copy_of_its_neighbour: ("exact", 7),
    m_parent_words_of_two_records_swapped: ("exact", 8),
}


def test_the_base_areas_are_what_the_mutants_need():
    send, counts, expected, _ = base("exact")
    assert [len(e) > 3 * sp.SEGS for e in expected] == [True, False, True] and len(expected[SHARD]) == 0
    assert counts.sum() == sum(len(e) for e in expected) and counts.max() <= CAP and (counts[[0, 2]] >= 2).all()
    fsend, fcounts, _, before = base("filtered")
    assert 0 < fcounts.sum() < counts.sum() and len(before) > 100
    for d in (0, 2):   # something to drop: a repeat inside the level, and a fingerprint of an earlier level
        fp = sr.fingerprint(expected[d][:, :W])
        assert len(set(fp.tolist())) < len(fp) and set(fp.tolist()) & before


@pytest.mark.parametrize("mode", sp.MODES)
def test_the_predicate_accepts_correct_areas(mode):
    send, counts, expected, before = base("exact" if mode in ("exact", "overflowed") else "filtered")
    assert sp.check_send_area(send, counts, expected, SHARD, mode, before) is None
    if mode == "exact":
        for seed in (5, 6):   # any placement
            assert sp.check_send_area(*area_of(expected, seed), expected, SHARD, mode) is None
        no_trace, _ = sp.expected_sends(sp.search()[LEVEL], P_BASE, SHARD, sp.owned(sp.search()[LEVEL], P_BASE, SHARD), False)
        assert sp.check_send_area(*area_of(no_trace, 7, trace=False), no_trace, SHARD, mode) is None
        assert sp.check_send_area(send, counts, expected, SHARD, "filtered", before).startswith("clause 4")
    if mode == "saturated":   # everything generated is as good as one per fingerprint
        send, counts, expected, _ = base("exact")
        assert sp.check_send_area(send, counts, expected, SHARD, mode, before) is None
    if mode == "overflowed":  # sub-buffers of 8 records: full ones, and any 8 of the generated records in each
        small = [e[:8 * sp.SEGS] if d == 0 else e[:5] if d == 2 else e for d, e in enumerate(expected)]
        send, counts = area_of(small, seed=2, cap=8)
        assert (counts[0] == 8).all() and counts[2].sum() == 5
        assert sp.check_send_area(send, counts, [expected[0], expected[1], expected[2][:5]], SHARD, mode) is None
        assert sp.check_send_area(send, counts, expected, SHARD, mode).startswith("clause 6: destination 2")   # lost, and nothing full
        assert sp.check_send_area(send, counts, [expected[0], expected[1], expected[2][:5]], SHARD, "exact").startswith("clause 6")
        send[0, 0, 0] = expected[2][0]
        assert sp.check_send_area(send, counts, [expected[0], expected[1], expected[2][:5]], SHARD, mode).startswith("clause 3")


@pytest.mark.parametrize("mutant", list(MUTANTS), ids=lambda m: m.__name__[2:])
def test_the_predicate_rejects(mutant):
    mode, clause = MUTANTS[mutant]
    send, counts, expected, before = base(mode)
    expected = list(expected)
    mutant(*((send, counts, expected, before) if mode == "filtered" and clause == 5 else (send, counts, expected)))
    said = sp.send_area_violations(send, counts, expected, SHARD, mode, before)
    print(said)
    assert said and said[0].startswith(f"clause {clause}:")          # the message names the clause the mutant breaks ...
    assert sp.check_send_area(send, counts, expected, SHARD, mode, before) == said[0]
    assert all(int(s.split(":")[0].split()[1]) >= clause for s in said)   # ... and no earlier clause speaks


def test_a_missing_fingerprint_is_missed_in_every_mode_that_filters():
    for mode in ("filtered", "saturated"):
        send, counts, expected, before = base("filtered")
        sb = int(np.flatnonzero(counts[0])[0])
        lost = int(sr.fingerprint(send[0, sb, counts[0, sb] - 1][None, :W])[0])
        there = sp.shipped_fingerprints(send, counts, SHARD) - {lost}
        stay = next(e for e in expected[0] if int(sr.fingerprint(e[None, :W])[0]) in there)
        send[0, sb, counts[0, sb] - 1] = stay                         # (the count stands: a copy of another record in its place)
        said = sp.send_area_violations(send, counts, expected, SHARD, mode, before)
        assert any(s.startswith("clause 7") and "missing" in s for s in said), said


def test_every_clause_has_a_mutant():
    assert sorted(c for _, c in MUTANTS.values()) == list(range(1, 9))
    assert sp.send_area_violations.__doc__.count("\n      ") >= 8
