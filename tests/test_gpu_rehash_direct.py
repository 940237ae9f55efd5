"""The rehash kernels of the growing seen-set (csrc/kmc_rehash.h) launched directly, from the shipped code object, on tables
made here — at the geometries the growth rule leaves to chance (ratios just above 1 and far above 2, partial last tiles, tiles
that are no multiple of the block, several tiles through one workgroup's window, more than 64 KiB of window) and on contents
that crowd, wrap and share word 0 — and judged by tests/rehash_ref.py's predicate: the same entries, every one reachable by its
probe, nothing else anywhere.  Every buffer lies between margins that must come back as they were; a windowed launch finds
the new tables poisoned, for the windowed kernel alone must write every slot.  All comparisons are exact."""
import functools

import numpy as np
import pytest

import rehash_ref as rr
from rehash_ref import ERR_LIST_FULL, ERR_TABLE_FULL, ERR_WINDOW, POISON_WORD, SHAPES, RehashRun

pytestmark = pytest.mark.gpu
U64 = np.uint64
ONES = 0xFFFFFFFFFFFFFFFF

# old groups, new groups, span, window groups, workgroups.  None: what window_span gives a window of 128 KiB for the shape
GEOMETRIES = [
    (1, 2, 1, 2, 1),        # one tile; the only window is the last: the wrap is phase two's
    (4, 8, 1, 2, 1),        # four tiles through one workgroup's window
    (3, 7, 2, 5, 1),        # a ratio that is no integer, a partial last tile
    (3, 7, 2, 5, 2),
    (5, 6, 3, 4, 1),        # ratio 1.2 (a crowded target under pattern B); tiles of 192 slots, no multiple of the 256 lanes
    (16, 33, 5, 11, 3),     # four tiles over three workgroups
    (7, 64, 1, 10, 2),      # one old group onto nine or ten new ones
    (64, 128, 31, 64, 2),   # the engine's choice for one-word entries at 32 KiB
    (128, 256, None, None, 2),   # 128 KiB of window: more than a launch gets without asking
]
PATTERNS = ["half", "crowded", "clustered", "shared word 0", "empty", "single"]


def _other_words(rng, n):
    """random words, 0 and all-ones among them (a predecessor of 0 is a value like any other)"""
    w = rng.integers(0, 1 << 63, size=n, dtype=U64) * U64(2) + rng.integers(0, 2, size=n, dtype=U64)
    kind = rng.integers(0, 10, size=n)
    w[kind == 0] = 0
    w[kind == 1] = U64(ONES)
    if n >= 2:
        w[0], w[-1] = 0, U64(ONES)
    return w


@functools.lru_cache(maxsize=None)
def content(pattern, G):
    """(rows of (word 0, word 1, predecessor), their slots in an old table of G groups), seeded by (pattern, G)"""
    cap = G * 64
    rng = np.random.default_rng([PATTERNS.index(pattern), G])
    if pattern in ("half", "crowded", "empty", "single"):
        n = {"half": cap // 2, "crowded": int(0.95 * cap), "empty": 0, "single": 1}[pattern]
        w0 = rng.integers(1, 1 << 63, size=n, dtype=U64) * U64(2) + U64(1)
        w1 = _other_words(rng, n)
    elif pattern == "clustered":   # every key in the first or the last old group, the low six bits 63
        n = min(cap // 2, 128)
        r = rng.integers(0, (1 << 32) // G - 1, size=n, dtype=U64)
        r[:2] = 0                  # key 0, and every key bit
        key = np.where(np.arange(n) % 2 == 0, r, U64(0xFFFFFFFF) - r)
        w0 = (rng.integers(0, 1 << 24, size=n, dtype=U64) << U64(40)) | (key << U64(8)) | (rng.integers(0, 4, size=n, dtype=U64) << U64(6)) | U64(63)
        w1 = _other_words(rng, n)
        groups = rr.slot_of(w0, cap) >> U64(6)
        assert set(groups.tolist()) <= {0, G - 1} and (w0 & U64(63) == 63).all()
    else:                          # runs of 2..8 entries under one word 0, told apart by word 1
        w0, w1 = [], []
        while len(w0) + 8 <= cap // 2:
            k = int(rng.integers(2, 9))
            w0 += [int(rng.integers(1, 1 << 63)) * 2 + 1] * k
            run = set()
            while len(run) < k:
                run.add(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)))
            run = sorted(run)
            if len(w1) == 0:
                run[0], run[-1] = 0, ONES
            w1 += run
        w0, w1 = np.array(w0, dtype=U64), np.array(w1, dtype=U64)
        order = rng.permutation(len(w0))   # (the runs arrive interleaved)
        w0, w1 = w0[order], w1[order]
    rows = np.stack([w0, w1, _other_words(rng, len(w0))], axis=1) if len(w0) else np.zeros((0, 3), dtype=U64)
    assert rows[:, 0].all()
    return rows, rr.place(rows[:, 0], cap)


def old_tables(pattern, G, tag):
    SW, SP = SHAPES[tag]
    rows, at = content(pattern, G)
    cols = [0] + ([1] if SW == 2 else []) + ([2] if SP else [])
    return rr.fill(rows[:, cols], at, G * 64, SW, SP), len(rows)


@functools.lru_cache(maxsize=None)
def listed_by_reference(pattern, G, G2, span):
    return rr.turned_away(old_tables(pattern, G, "1n")[0][0], G * 64, G2 * 64, span, 1)


def window_of(geometry, tag):
    G, G2, span, groups, grid = geometry
    if span is None:
        groups = 128 * 1024 // (64 * 8 * rr.entry_words(*SHAPES[tag]))
        span = rr.window_span(groups, G, G2)
    assert span >= 1 and rr.window_fits(G, G2, span, groups * 64)
    return span, groups * 64, grid


def cases(geometries):
    return [pytest.param(g, t, p, id=f"{g[0]}-{g[1]}" + (f"-grid{g[4]}" if len(g) > 2 else "") + f"-{t}-{p}")
            for g in geometries for t in SHAPES for p in PATTERNS if p != "shared word 0" or SHAPES[t][0] == 2]


@pytest.fixture(scope="module")
def mod():
    m = rr.RehashModule()
    yield m
    m.close()


@pytest.mark.parametrize("geometry,tag,pattern", cases(GEOMETRIES))
def test_window_and_overflow(mod, geometry, tag, pattern):
    G, G2 = geometry[:2]
    span, win_slots, grid = window_of(geometry, tag)
    old, n = old_tables(pattern, G, tag)
    run = RehashRun(mod, tag, "window", old, G * 64, G2 * 64, span=span, win_slots=win_slots, grid=grid)
    c = run.ctl
    print(f"entries {n}: err {c.err}, placed in windows {c.placed_window}, by phase two {c.placed_global}, listed {c.listed}")
    assert run.violation() is None
    assert c.err == 0
    assert c.placed_window + c.placed_global == n
    assert c.listed == c.placed_global
    assert c.listed == listed_by_reference(pattern, G, G2, span)   # (what a window turns away does not depend on the order of arrival)
    # the list holds the listed entries and nothing behind them
    EW = rr.entry_words(*SHAPES[tag])
    assert (run.list[c.listed * EW:] == U64(POISON_WORD)).all() and (run.list[:c.listed * EW:EW] != 0).all()


@pytest.mark.parametrize("geometry,tag,pattern", cases(sorted({g[:2] for g in GEOMETRIES})))
def test_scatter(mod, geometry, tag, pattern):
    G, G2 = geometry
    old, n = old_tables(pattern, G, tag)
    run = RehashRun(mod, tag, "scatter", old, G * 64, G2 * 64)
    c = run.ctl
    assert run.violation() is None
    assert (c.err, c.placed_window, c.placed_global, c.listed) == (0, 0, n, 0)
    assert (run.list == U64(POISON_WORD)).all()


def _no_margin_changed(run):
    return all(np.array_equal(got, want) for _, (got, want) in run.margins)


def _same(a, b):
    return all(x is None and y is None or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("tag", list(SHAPES))
def test_a_list_too_small_raises_its_flag_and_leaves_the_old_table_for_the_retry(mod, tag):
    """The state from which the host redoes a growth by scatter: the flag, nothing written behind the list, every window written
    all the same, the old tables as they were."""
    SW, SP = SHAPES[tag]
    EW = rr.entry_words(SW, SP)
    G, G2, span = 4, 8, 1
    old, n = old_tables("clustered", G, tag)
    turned = listed_by_reference("clustered", G, G2, span)
    list_cap = turned // 2
    assert list_cap >= 1
    run = RehashRun(mod, tag, "window", old, G * 64, G2 * 64, span=span, win_slots=2 * 64, grid=2, list_cap=list_cap)
    c = run.ctl
    assert c.err == ERR_LIST_FULL
    assert c.listed == turned > list_cap
    assert _no_margin_changed(run) and len(run.list) == list_cap * EW
    assert _same(run.old_now, old)
    assert not (run.new[0] == U64(POISON_WORD)).any() and not (SP and (run.new[1] == U64(POISON_WORD)).any())
    assert (c.placed_window, c.placed_global) == (n - turned, list_cap)
    # what the list did take are entries of the old table, each once
    want, _ = rr.entries_of(*old, G * 64, SW, SP)
    listed = run.list.reshape(list_cap, EW)
    assert len({tuple(r) for r in listed.tolist()}) == list_cap and {tuple(r) for r in listed.tolist()} <= {tuple(r) for r in want.tolist()}


@pytest.mark.parametrize("tag", list(SHAPES))
def test_a_window_too_small_raises_its_flag_and_writes_nothing_of_that_tile(mod, tag):
    SW, SP = SHAPES[tag]
    G, G2, span, win_slots = 3, 7, 2, 3 * 64
    w = rr.windows(G, G2, span)
    assert [hi - lo > win_slots for lo, hi in w] == [True, False]   # the first tile is a group short, the second fits
    old, n = old_tables("half", G, tag)
    run = RehashRun(mod, tag, "window", old, G * 64, G2 * 64, span=span, win_slots=win_slots, grid=1)
    assert run.ctl.err == ERR_WINDOW
    (lo0, hi0), (lo1, hi1) = w
    assert (run.new[0][lo0 * SW:hi0 * SW] == U64(POISON_WORD)).all() and not (run.new[0][lo1 * SW:hi1 * SW] == U64(POISON_WORD)).any()
    if SP:
        assert (run.new[1][lo0:hi0] == U64(POISON_WORD)).all() and not (run.new[1][lo1:hi1] == U64(POISON_WORD)).any()
    assert _no_margin_changed(run) and _same(run.old_now, old)
    # the tile that was left out lists nothing; the other one's entries are all in its window or were listed and placed there
    skip = lambda lo, hi: hi - lo > win_slots
    assert run.ctl.listed == run.ctl.placed_global == rr.turned_away(old[0], G * 64, G2 * 64, span, SW, skip)
    in_second = int(np.count_nonzero(old[0].reshape(G * 64, SW)[span * 64:, 0]))
    assert run.ctl.placed_window + run.ctl.placed_global == in_second
    assert int(np.count_nonzero(run.new[0].reshape(G2 * 64, SW)[lo1:hi1, 0])) == in_second


@pytest.mark.parametrize("tag", list(SHAPES))
def test_a_table_too_small_raises_its_flag_and_ends(mod, tag):
    """100 entries into 64 slots by scatter: the probe loop is bounded by the new table's size."""
    SW, SP = SHAPES[tag]
    rng = np.random.default_rng(7)
    rows = np.stack([rng.integers(1, 1 << 63, size=100, dtype=U64) * U64(2) + U64(1), _other_words(rng, 100), _other_words(rng, 100)], axis=1)
    old = rr.build_table(rows[:, [0] + ([1] if SW == 2 else []) + ([2] if SP else [])], 256, SW, SP)
    run = RehashRun(mod, tag, "scatter", old, 256, 64)
    c = run.ctl
    assert (c.err, c.placed_global, c.placed_window, c.listed) == (ERR_TABLE_FULL, 64, 0, 0)
    assert _no_margin_changed(run) and _same(run.old_now, old)
    got, occ = rr.entries_of(*run.new, 64, SW, SP)
    want, _ = rr.entries_of(*old, 256, SW, SP)
    assert len(occ) == 64 and {tuple(r) for r in got.tolist()} <= {tuple(r) for r in want.tolist()} and len({tuple(r) for r in got.tolist()}) == 64
