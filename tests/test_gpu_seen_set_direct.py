"""The seen-set's claim paths (csrc/kmc_sink.h: claim_steps, claim_steps<1>, claim_wide_steps behind claim_any) and the host's
walk along the same chains (table_lookup: kmc_contains, kmc_pred_of), asked directly where open addressing goes wrong: tables
of an odd number of groups, chains that run over the last slot into slot 0, a table filled to its last slot and one state
beyond, long runs of entries under one fingerprint, and the search kernel's own claims in a table at load 0.91.

The direct cases hand synthetic records to k_insert through the level-step ABI — one real level, then launches of records
chosen on the CPU by their home slots (tests/seen_set_ref.py) — and read the table back from a checkpoint.  Which copy of a
state wins a slot and where it lands is not deterministic: the image is judged by seen_set_ref's predicate (the same
fingerprints, the matching check words, every entry reachable by its probe, nothing in an empty slot, every link one its
entry's copies carried), the counters and the frontier exactly.  tests/test_seen_set_ref_cpu.py holds the reference to the
headers and the predicate to its mutants, and checks every precondition a case rests on without a GPU."""
import numpy as np
import pytest

import seen_set_ref as sr

pytestmark = pytest.mark.gpu
U64 = np.uint64
SHAPES = list(sr.SHAPES)
CAPS = [1024, 1088, 64 * 1001]     # the smallest table kmc_open allows, 17 groups, an odd number of groups where the walk bound is 1024


def expected_of(states, allowed, reduced=False):
    fp = sr.fingerprint(states)
    return sr.real_expected(reduced) + sr.expected_rows(sr.reduce_fp(fp) if reduced else fp, sr.check_word(states), allowed)


def assert_frontier_is(mc, states):
    """the six real states and every synthetic state exactly once, no other"""
    got = mc.frontier_states()
    assert got.shape == (6 + len(states), mc.state_words)
    synthetic = got[(got[:, 0] >> U64(63)) == 1]
    assert len(synthetic) == len(states)
    assert np.array_equal(synthetic[np.argsort(synthetic[:, 0])], states[np.argsort(states[:, 0])])


def assert_host_finds(mc, shape, states, fps, allowed, absent=()):
    """table_lookup walks the chains the kernel built: contains, and pred_of with the stride of the shape"""
    assert mc.fingerprint(states[0]) == int(fps[0])
    for s in states:
        assert mc.contains(s)
    for s in absent:
        assert not mc.contains(s)
    if sr.SHAPES[shape][1]:
        for fp, al in zip(fps, allowed):
            found, pred = sr.pred_of(mc, fp)
            assert found and pred in al, (hex(int(fp)), hex(pred))
        for fp in sr.fingerprint(np.asarray(absent)) if len(absent) else ():
            assert sr.pred_of(mc, fp) == (False, 0)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_chain_over_the_end_of_the_table(shape, cap, tmp_path):
    """200 states homed in the last group, 1 to 8 copies of each, shuffled, in one launch: at least 136 of them are claimed
    past the wrap (a narrow claim, a paired claim with its link in the slot, a wide claim with a.pred[i]), and the host finds
    all of them, and not the 50 absent states homed in the same group, by walking over the end too."""
    states, fps, copies, absent = sr.wrap_case(cap)
    recs, allowed = sr.records(states, copies, sr.SHAPES[shape][1], seed=1)
    with sr.open_checker(shape, cap) as mc:
        level = sr.OneLevel(mc)
        level.insert(recs)
        info = level.finish()
        assert info.error_flags == 0
        assert int(info.new_states) == 6 + 200
        assert_frontier_is(mc, states)
        image, pred_image = level.image(tmp_path, shape, cap)
        assert sr.check_seen_set(image, pred_image, cap, shape, expected_of(states, allowed)) is None
        word0 = image.reshape(cap, -1)[:, 0]
        assert word0[cap - 64:].all() and word0[:100].all()
        assert_host_finds(mc, shape, states, fps, allowed, absent)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_second_launch_claims_only_what_the_first_did_not(shape, cap, tmp_path):
    """A prefill of 120, then a shuffle of 70 of those again with 80 new states: the states of the first launch keep the links
    of the first launch, only the new ones count, and the image of both is one correct table."""
    states, fps, copies, _ = sr.wrap_case(cap)
    trace = sr.SHAPES[shape][1]
    first, allowed1 = sr.records(states[:120], copies[:120], trace, seed=2)
    again = np.concatenate([np.arange(50, 120), np.arange(120, 200)])
    second, allowed2 = sr.records(states[again], copies[again], trace, seed=3, copy0=8)
    allowed = allowed1 + allowed2[70:]
    with sr.open_checker(shape, cap) as mc:
        level = sr.OneLevel(mc)
        level.insert(first)
        level.insert(second)
        info = level.finish()
        assert info.error_flags == 0
        assert int(info.new_states) == 6 + 200
        assert_frontier_is(mc, states)
        image, pred_image = level.image(tmp_path, shape, cap)
        assert sr.check_seen_set(image, pred_image, cap, shape, expected_of(states, allowed)) is None
        assert_host_finds(mc, shape, states[100:140], fps[100:140], allowed[100:140])


def _fill(level, states, trace, parts, seed):
    """`states` in len(parts) launches: launch k hands in states[parts[k]] (1 to 3 copies each); the links of a state are those of
    the first launch that held it"""
    allowed = [None] * len(states)
    for k, part in enumerate(parts):
        copies = np.random.default_rng([seed, k]).integers(1, 4, size=len(part))
        recs, al = sr.records(states[part], copies, trace, seed=seed + k, copy0=4 * k)
        for i, a in zip(part, al):
            if allowed[i] is None:
                allowed[i] = a
        level.insert(recs)
    return allowed


@pytest.mark.parametrize("shape", SHAPES)
def test_the_smallest_table_takes_1000_entries(shape, tmp_path):
    """1024 slots, walk bound 1023: a chain is never longer than the occupied slots, so every fill up to 1022 entries is inside
    the bound by construction.  993 states in two launches (the second repeats 300 of the first) beside the 7 real ones."""
    cap = 1024
    states, fps = sr.fill_case(cap, cap - 7 + 1)
    states, fps = states[:993], fps[:993]
    with sr.open_checker(shape, cap) as mc:
        level = sr.OneLevel(mc)
        allowed = _fill(level, states, sr.SHAPES[shape][1], [np.arange(0, 500), np.arange(200, 993)], seed=20)
        info = level.finish()
        assert info.error_flags == 0
        assert int(info.new_states) == 6 + 993
        assert_frontier_is(mc, states)
        image, pred_image = level.image(tmp_path, shape, cap)
        assert sr.check_seen_set(image, pred_image, cap, shape, expected_of(states, allowed)) is None
        assert int((image.reshape(cap, -1)[:, 0] != 0).sum()) == 1000
        assert_host_finds(mc, shape, states[::25], fps[::25], allowed[::25])


@pytest.mark.parametrize("one_more", [False, True], ids=["exactly full", "one state too many"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_smallest_table_filled_to_its_last_slot(shape, one_more, tmp_path):
    """Exactly cap entries: every state is placed (a walk of d slots is at most d loads and d + 1 compare-and-swaps, 2047 steps
    for d = 1023, inside the 2 max_probes + 2 = 2048 a walk may take), no error.  One state more: its walk meets no empty slot
    and no entry of its own, ends after 2049 loads with KMC_ERR_TABLE_FULL, and claims nothing — the table and the frontier are
    those of the full table."""
    cap = 1024
    states, fps = sr.fill_case(cap, cap - 7 + 1)
    extra, states = states[-1:], states[:-1]
    with sr.open_checker(shape, cap) as mc:
        level = sr.OneLevel(mc)
        allowed = _fill(level, states, sr.SHAPES[shape][1], [np.arange(0, 600), np.arange(400, cap - 7)], seed=30)
        if one_more:
            level.insert(sr.records(extra, [1], sr.SHAPES[shape][1], seed=33)[0])
        info = level.finish()
        assert info.error_flags == (sr.ERR_TABLE_FULL if one_more else 0)
        assert int(info.new_states) == 6 + (cap - 7)
        assert_frontier_is(mc, states)
        image, pred_image = level.image(tmp_path, shape, cap)
        assert image.reshape(cap, -1)[:, 0].all()
        assert sr.check_seen_set(image, pred_image, cap, shape, expected_of(states, allowed)) is None


@pytest.mark.parametrize("shape", SHAPES)
def test_a_crowded_corner_of_a_table_of_1001_groups(shape, tmp_path):
    """64 x 1001 slots: the walk bound is 1024 here.  400 states homed in the last two groups and 2000 anywhere; the longest
    cyclic run of the reference image is at most 512 (the occupied slots of a linear-probing table do not depend on the order
    of the inserts, so that bounds every chain the kernel can walk), and it runs over the end."""
    cap = 64 * 1001
    states, fps = sr.spread_case(cap, 400, 2000, seed=11)
    real = np.array([e[0] for e in sr.real_expected()], dtype=U64)
    taken = sr.occupied(np.concatenate([real, fps]), cap)
    assert sr.longest_cyclic_run(taken) <= sr.max_probes(cap) // 2 == 512 and taken[cap - 1] and taken[0]
    with sr.open_checker(shape, cap) as mc:
        level = sr.OneLevel(mc)
        allowed = _fill(level, states, sr.SHAPES[shape][1], [np.arange(0, 2400)], seed=40)
        info = level.finish()
        assert info.error_flags == 0
        assert int(info.new_states) == 6 + 2400
        assert_frontier_is(mc, states)
        image, pred_image = level.image(tmp_path, shape, cap)
        assert sr.check_seen_set(image, pred_image, cap, shape, expected_of(states, allowed)) is None
        assert np.array_equal(image.reshape(cap, -1)[:, 0] != 0, taken)
        pick = np.concatenate([np.arange(0, 400, 8), np.arange(400, 2400, 100)])
        absent, _ = sr.select_homed(10, cap, sr.last_groups(cap, 2), 2, seed=11, first=int(sr.index_of(states).max()) + 1)
        assert_host_finds(mc, shape, states[pick], fps[pick], [allowed[k] for k in pick], absent)


@pytest.mark.parametrize("shape", ["wide", "narrow"])
def test_300_states_under_3_fingerprints(shape, tmp_path, monkeypatch):
    """Collisions on demand (-DKMC_TUNING=1 -DKMC_TEST_FP_BITS=10): 300 distinct states that share 3 reduced fingerprints, homed
    in the last group of 1024 slots.  The wide table tells them apart by their check words — a lane walks on from a slot that
    holds ANOTHER state with its fingerprint (walk = true), a hundred times in a row and over the end of the table — and holds
    all 300; the narrow one merges them into 3.  (The host's lookup knows nothing of the define and is not asked.)"""
    monkeypatch.setenv("KMC_JIT_DEFINES", sr.TEST_FP_DEFINES)
    cap = 1024
    states, red = sr.collision_case()
    values, counts = np.unique(red, return_counts=True)
    recs, allowed = sr.records(states, np.random.default_rng(50).integers(1, 5, size=300), sr.SHAPES[shape][1], seed=51)
    real = sr.real_expected(reduced=True)
    with sr.open_checker(shape, cap) as mc:
        level = sr.OneLevel(mc)
        level.insert(recs)
        info = level.finish()
        assert info.error_flags == 0
        image, pred_image = level.image(tmp_path, shape, cap)
        word0 = image.reshape(cap, -1)[:, 0]
        if shape == "wide":
            assert int(info.new_states) == 6 + 300
            assert_frontier_is(mc, states)
            assert sr.check_seen_set(image, pred_image, cap, shape, expected_of(states, allowed, reduced=True)) is None
            assert [int((word0 == v).sum()) for v in values] == counts.tolist()
            assert set(image.reshape(cap, 2)[np.isin(word0, values), 1].tolist()) == set(sr.check_word(states).tolist())
            # (three home slots in a group of 64: at least 236 of the 300 lie past the wrap)
            assert word0[cap - 1] in values and word0[:200].all() and int(np.isin(word0[:512], values).sum()) >= 300 - 64
        else:
            merged = sorted({e[0] for e in real})             # (real states that share a reduced fingerprint merge as well)
            assert int(info.new_states) == len(merged) - 1 + 3
            got = mc.frontier_states()
            synthetic = got[(got[:, 0] >> U64(63)) == 1]
            assert len(synthetic) == 3 and sorted(sr.reduce_fp(sr.fingerprint(synthetic)).tolist()) == values.tolist()
            expected = sr.expected_rows(merged + values.tolist())
            assert sr.check_seen_set(image, pred_image, cap, shape, expected) is None


# -- the search kernel's own claims ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,defines", [("narrow", None), ("paired", None), ("wide", None), ("narrow", sr.DEFER_DEFINES)],
                         ids=["default", "paired", "wide", "deferred"])
def test_the_search_in_a_crowded_table_of_an_odd_number_of_groups(shape, defines, monkeypatch):
    """k_expand's own entry into the claim paths — immediately, or deferred by a flush (-DKMC_DEFER_MIN_WORDS=1) — in a table of
    679 groups that ends at load 0.912 with a longest run of 510 slots (seen_set_ref.CROWDED_SEARCH_CAP): every level is the
    oracle's set, the chained launches count the same, and with traces the host finds the last level's states and real
    predecessors of theirs."""
    if defines:
        monkeypatch.setenv("KMC_JIT_DEFINES", defines)
    rows, levels = sr.reachable()
    at = np.concatenate([[0], np.cumsum(levels)])
    want = [set(map(tuple, rows[at[k]:at[k + 1]].tolist())) for k in range(len(levels))]
    got = []
    with sr.open_checker(shape, sr.CROWDED_SEARCH_CAP, frontier_capacity=1 << 18) as mc:
        res = mc.run(progress=lambda info: got.append(set(map(tuple, mc.frontier_states().tolist()))))
        assert (res.verdict, res.distinct, res.levels, res.table_capacity) == ("ok", sr.N_STATES, list(levels), sr.CROWDED_SEARCH_CAP)
        for k in range(len(levels)):
            assert got[k] == want[k], f"level {k} state sets differ"
        again = mc.run()      # chained launches this time (no progress callback)
        assert (again.verdict, again.distinct, again.generated, again.levels) == ("ok", sr.N_STATES, res.generated, list(levels))
        for k in (len(levels) - 1, len(levels) - 6):
            sample = rows[at[k]:at[k + 1]][:: max(1, levels[k] // 12)]
            for s in sample:
                assert mc.contains(s)
            if sr.SHAPES[shape][1]:
                before = {int(f): r for f, r in zip(sr.fingerprint(rows[at[k - 1]:at[k]]), rows[at[k - 1]:at[k]])}
                for s, fp in zip(sample, sr.fingerprint(sample)):
                    found, pred = sr.pred_of(mc, fp)
                    assert found and pred in before, (hex(int(fp)), hex(pred))
                    assert tuple(s.tolist()) in {t for t, _fp, _kind in mc.successors(before[pred])}
        for s in sr.synthetic(0, 20, 2, seed=60):
            assert not mc.contains(s)
