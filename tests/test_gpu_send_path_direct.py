"""The send path of a sharded search (csrc/kmc_sink.h, KmcSink::process<KMC_MODE_SHARDED>: owner bucketing with one atomicAdd per
destination and batch, the sender-side filter first_time, the overflow of a sub-buffer and the counts clamped behind it), asked
directly: P shards on one device are stepped level by level through the level-step ABI, every send area is filled with a poison
word before its kmc_step_expand and read back WHOLE after it, and tests/send_path_ref.py's predicate says what it must hold — per
destination the multiset of (successor[, parent fingerprint]) the shard's frontier generates, found with the device's own model
templates on the host; nothing past a count, nothing in the shard's own destination.  A search that is only compared with the
oracle's counts at its end sees none of this: every state is generated about three times, on different shards and levels.

tests/test_send_path_ref_cpu.py holds the reference to the headers and the predicate to its mutants, and checks every
precondition a case rests on without a GPU.  Every comparison here is exact."""
import ctypes as C

import numpy as np
import pytest

import seen_set_ref as sr
import send_path_ref as sp

pytestmark = pytest.mark.gpu
U64 = np.uint64
W = sp.W


def judge(sends, counts, s, expected, mode, k, before=frozenset()):
    said = sp.check_send_area(sends[s], counts[s], expected, s, mode, before)
    assert said is None, f"shard {s}, level {k}: {said}"


def assert_frontiers(fronts, level, P, k):
    """every shard holds, as a set, the states of the level it owns: no other, none twice"""
    for s, f in enumerate(fronts):
        got = list(map(tuple, f.tolist()))
        want = set(map(tuple, level.states[sp.owned(level, P, s)].tolist())) if level is not None else set()
        assert len(got) == len(set(got)) and set(got) == want, f"shard {s}: the frontier of level {k}"


def generated_of(infos):
    return sum(int(x) for i in infos for x in i.generated_level)


# -- A: exact contents --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetry", [False, True], ids=["plain", "orbits"])
@pytest.mark.parametrize("trace", [False, True], ids=["notrace", "trace"])
@pytest.mark.parametrize("P", sp.SHARDS)
def test_every_send_area_of_the_search_holds_what_its_frontier_generates(P, trace, symmetry, monkeypatch):
    """Filter off: per shard and level the sub-buffers of a destination hold, together, exactly the records generated for it
    (under orbit counting: the representatives), each with the fingerprint of ITS parent; the rest of the tensor is poison;
    the counts add up; and after routing and kmc_step_finish every shard's frontier is the set of new states it owns — which
    also holds the local claim path of the sharded kernel to the reference."""
    monkeypatch.setenv("KMC_SEND_FILTER", "0")
    lv, plain = sp.search(symmetry), sp.search()
    two_sub_buffers = 0
    with sp.Shards(P, keep_trace=trace, symmetry=symmetry) as sh:
        sh.begin()
        fronts = sh.frontiers()
        assert_frontiers(fronts, lv[0], P, 0)
        for k, level in enumerate(lv):
            rows = [sp.frontier_rows(level, f) for f in fronts]
            counts, sends = sh.expand()
            for s in range(P):
                expected, _local = sp.expected_sends(level, P, s, rows[s], trace)
                judge(sends, counts, s, expected, "exact", k)
                assert int(counts[s].sum()) == sum(len(e) for e in expected)
                two_sub_buffers += int(((counts[s] > 0).sum(axis=1) >= 2).any())
            sh.route()
            infos = sh.finish()
            assert [int(i.error_flags) for i in infos] == [0] * P and sum(int(i.send_filtered) for i in infos) == 0
            assert generated_of(infos) == plain[k].generated          # (orbit counting weighs to the plain search's number)
            assert sum(int(i.new_states) for i in infos) == (len(plain[k + 1].states) if k + 1 < len(lv) else 0)
            fronts = sh.frontiers()
            assert_frontiers(fronts, lv[k + 1] if k + 1 < len(lv) else None, P, k + 1)
        assert two_sub_buffers > 0      # some level filled two sub-buffers of one destination: two blocks, two counters
        if not symmetry:
            # the reference's reading of a binding whose two disjuncts coincide (generated twice, sent once), against the
            # kernel's own count of them, which the sink never sees
            res = [e.mc.result() for e in sh.engines]
            assert sum(r.generated - r.generated_repeats for r in res) == 1 + sum(len(l.words) for l in lv)


# -- B: the filter, roomy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3])
def test_the_filter_ships_every_fingerprint_once_per_shard(P, monkeypatch):
    """Default policy (on for 2..4 shards) in filters no chain of which reaches 64 slots: over the whole search a shard ships
    exactly one record per fingerprint it has not shipped before, on any level; the record is one of the generated copies, with
    that copy's parent; and send_filtered is the rest, exactly."""
    monkeypatch.delenv("KMC_SEND_FILTER", raising=False)
    lv = sp.search()
    shipped = [set() for _ in range(P)]
    dropped = 0
    with sp.Shards(P, keep_trace=True) as sh:
        sh.begin()
        fronts = sh.frontiers()
        for k, level in enumerate(lv):
            rows = [sp.frontier_rows(level, f) for f in fronts]
            counts, sends = sh.expand()
            want_filtered = []
            for s in range(P):
                expected, _local = sp.expected_sends(level, P, s, rows[s], True)
                judge(sends, counts, s, expected, "filtered", k, frozenset(shipped[s]))
                want_filtered.append(sum(len(e) for e in expected) - int(counts[s].sum()))
                shipped[s] |= sp.shipped_fingerprints(sends[s], counts[s], s)
            sh.route()
            infos = sh.finish()
            assert [int(i.error_flags) for i in infos] == [0] * P
            assert [int(i.send_filtered) for i in infos] == want_filtered, f"level {k}"
            dropped += sum(want_filtered)
            fronts = sh.frontiers()
            assert_frontiers(fronts, lv[k + 1] if k + 1 < len(lv) else None, P, k + 1)
    remote = [sp.remote_fingerprints(lv, P, s) for s in range(P)]
    assert shipped == [set(x.tolist()) for x in remote]
    assert dropped == sum(len(x) for x in remote) - sum(len(x) for x in shipped) > 0


# -- C: the filter, saturated ---------------------------------------------------------------------------------------------------
def test_a_saturated_filter_ships_too_much_and_loses_nothing(monkeypatch):
    """8 shards, the filter forced on, 8192 slots for the ~9,800 fingerprints a shard generates for the others: chains pass 64
    slots and answer "fresh".  Every shipped multiset lies between one record per fingerprint never shipped and everything
    generated, no such fingerprint is missing, send_filtered is the rest, and the search is the oracle's."""
    import kmo
    monkeypatch.setenv("KMC_SEND_FILTER", "1")
    P, lv = 8, sp.search()
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=2, R=2, E=1, invariants=()))
    shipped = [set() for _ in range(P)]
    records = 0
    levels, per_action = [1], np.zeros(16, dtype=np.int64)
    with sp.Shards(P, **sp.SATURATED) as sh:
        n_actions = len(sh.engines[0].action_names())
        sh.begin()
        fronts = sh.frontiers()
        for k, level in enumerate(lv):
            rows = [sp.frontier_rows(level, f) for f in fronts]
            counts, sends = sh.expand()
            want_filtered = []
            for s in range(P):
                expected, _local = sp.expected_sends(level, P, s, rows[s], False)
                judge(sends, counts, s, expected, "saturated", k, frozenset(shipped[s]))
                want_filtered.append(sum(len(e) for e in expected) - int(counts[s].sum()))
                shipped[s] |= sp.shipped_fingerprints(sends[s], counts[s], s)
                records += int(counts[s].sum())
            sh.route()
            infos = sh.finish()
            assert [int(i.error_flags) for i in infos] == [0] * P
            assert [int(i.send_filtered) for i in infos] == want_filtered, f"level {k}"
            for i in infos:
                per_action += np.array(list(i.generated_level), dtype=np.int64)
            levels.append(sum(int(i.new_states) for i in infos))
            fronts = sh.frontiers()
            assert_frontiers(fronts, lv[k + 1] if k + 1 < len(lv) else None, P, k + 1)
    assert levels[-1] == 0 and levels[:-1] == list(o.levels)
    assert per_action.tolist()[:n_actions] == list(o.action_generated)[:n_actions] and 1 + int(per_action.sum()) == o.generated
    # a filter with fewer slots than fingerprints cannot remember all of them: some repeat was shipped again
    assert records > sum(len(x) for x in shipped)


# -- D: overflow ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [0, 1], ids=["n records fit", "n - 1 do not"])
def test_a_sub_buffer_of_exactly_n_records_and_of_one_less(short, monkeypatch):
    """The level whose frontier fits one block: all n records for the other shard land in sub-buffer 0.  The handle gets a send
    area of the test's own, n (n - 1) records per sub-buffer, between two poisoned guards.  n: no flag, count n, contents exact.
    n - 1: KMC_ERR_SEND_FULL after kmc_step_finish, the published count clamped to n - 1, the records there are n - 1 of the
    generated ones, and record 0 of the next sub-buffer, every other sub-buffer and both guards are untouched."""
    import torch
    from kafka_specification_amd import _native as nat
    monkeypatch.setenv("KMC_SEND_FILTER", "0")
    P = sp.OVERFLOW_P
    s, k, d, n = sp.overflow_case()
    lv = sp.search()
    cap, RW = n - short, W + 1
    with sp.Shards(P, keep_trace=True) as sh:
        sh.begin()
        for _ in range(k):
            assert [int(i.error_flags) for i in sh.step()] == [0] * P
        fronts = sh.frontiers()
        assert_frontiers(fronts, lv[k], P, k)
        words = P * sp.SEGS * cap * RW
        guard = 2 * words
        buf = torch.full((guard + words + guard,), sp.POISON_I64, dtype=torch.int64, device="cuda:0")
        area = buf[guard:guard + words].view(P, sp.SEGS, cap, RW)
        nat.check(nat.lib().kmc_step_set_send_buffer(sh.engines[s].mc.handle, C.c_void_p(area.data_ptr()), cap))
        got = {s: sh.expand_one(s, send=area), 1 - s: sh.expand_one(1 - s)}
        whole = buf.cpu().numpy().view(U64)
        assert (whole[:guard] == U64(sp.POISON)).all() and (whole[guard + words:] == U64(sp.POISON)).all()
        sh.counts, sh.sends = [got[x][0] for x in range(P)], [got[x][1] for x in range(P)]
        expected, _local = sp.expected_sends(lv[k], P, s, sp.frontier_rows(lv[k], fronts[s]), True)
        assert len(expected[d]) == n
        judge(sh.sends, sh.counts, s, expected, "overflowed" if short else "exact", k)
        assert sh.counts[s][d].tolist() == [cap] + [0] * (sp.SEGS - 1)
        other, _ = sp.expected_sends(lv[k], P, 1 - s, sp.frontier_rows(lv[k], fronts[1 - s]), True)
        judge(sh.sends, sh.counts, 1 - s, other, "exact", k)
        sh.route([area if x == s else None for x in range(P)])
        infos = sh.finish()
        assert int(infos[s].error_flags) == (sp.ERR_SEND_FULL if short else 0) and int(infos[1 - s].error_flags) == 0
        if not short:
            assert_frontiers(sh.frontiers(), lv[k + 1], P, k + 1)
        torch.cuda.synchronize()


@pytest.mark.parametrize("exchange", ["torch", "rccl"])
def test_a_search_whose_levels_exceed_its_sub_buffers_ends_frontier_full(exchange, monkeypatch):
    """Sub-buffers of 64 records where one level sends 422 into one of them: the whole loop-back search, through the torch
    slices and through the exchange under the C ABI, stops with the verdict `frontier_full` — no exception, no count."""
    from kafka_specification_amd import CheckerConfig
    from kafka_specification_amd.sharded import check_loopback
    monkeypatch.setenv("KMC_EXCHANGE", exchange)
    monkeypatch.setenv("KMC_SEND_FILTER", "0")
    assert sp.overflow_case()[3] > 64
    r = check_loopback(CheckerConfig(**sr.CONSTANTS, **sp.ROOMY, send_capacity=64), sp.OVERFLOW_P)
    assert r.verdict == "frontier_full"
    lv = sp.search()
    assert r.levels == [len(l.states) for l in lv[:len(r.levels)]] and 0 < len(r.levels) <= sp.overflow_case()[1] + 1


# -- E: one shard with a send buffer ----------------------------------------------------------------------------------------------
def test_one_shard_with_a_send_buffer_sends_nothing():
    """kmc_step_set_send_buffer allows n_shards = 1 (HipShardEngine(native=False) calls it): the sharded kernel with one
    destination, itself.  After every level the area is all poison, the counts are 0, and the levels are the oracle's."""
    lv = sp.search()
    with sp.Shards(1, frontier_capacity=1 << 16) as sh:
        sh.begin()
        for k, level in enumerate(lv):
            assert_frontiers(sh.frontiers(), level, 1, k)
            counts, sends = sh.expand()
            assert not counts[0].any() and sends[0].shape == (1, sp.SEGS, sp.ROOMY_SEND[1], W)
            judge(sends, counts, 0, [np.zeros((0, W), dtype=U64)], "exact", k)
            sh.route()
            (info,) = sh.finish()
            assert int(info.error_flags) == 0 and generated_of([info]) == level.generated
            assert int(info.new_states) == (len(lv[k + 1].states) if k + 1 < len(lv) else 0)
