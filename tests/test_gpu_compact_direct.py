"""The pack and unpack kernels of the compact checkpoint (csrc/kmc_compact.h) launched directly, from the shipped table code
object, on tables made here.  Pack is held to numpy: the occupied slots in slot order, the prefix counts per tile of eight
groups, the table untouched.  Unpack gets entries and index computed HERE (not pack's output), finds its destination poisoned,
and is held to tests/rehash_ref.py's predicate.  The scatter form (a cleared table, kmc_rehash_overflow over the entry array) is
the second implementation.  Every buffer lies between margins that must come back as they were.  All comparisons are exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import rehash_ref as rr
from rehash_ref import ERR_LIST_FULL, ERR_TABLE_FULL, ERR_WINDOW, POISON_WORD, SHAPES, Guarded

U64 = np.uint64
T = 8              # KMC_COMPACT_TILE
LOAD_LIMIT = 0.92  # KMC_TABLE_LOAD_LIMIT
CTL_WORDS = C.sizeof(rr.KmcRehashCtl) // 8
ONES = 0xFFFFFFFFFFFFFFFF
PATTERNS = ["half", "crowded", "clustered", "shared word 0", "empty", "single"]
# old groups, new groups, span, window groups (None: no window holds a run — the scatter form only), workgroups, groups per stretch
GEOMETRIES = [
    (1, 1, 8, 1, 1, 8),
    (1, 2, 8, 2, 1, 8),
    (3, 7, 8, 7, 1, 8),       # a ratio that is no integer
    (5, 6, 8, 6, 2, 8),       # ratio 1.2: a crowded target
    (16, 5, 8, 3, 1, 16),     # a shrink; two runs through one workgroup's window
    (7, 64, None, None, 1, 8),
    (40, 56, 8, 12, 2, 16),   # five runs over two workgroups, three stretches
    (19, 33, 8, 14, 2, 24),   # G no multiple of the tile: the last run is three groups, the last tile too
]


class KmcCompactArgs(C.Structure):
    _fields_ = [("r", rr.KmcRehashArgs), ("g_first", C.c_uint64), ("g_end", C.c_uint64), ("index", C.c_uint64), ("entries", C.c_uint64),
                ("entries_cap", C.c_uint64)]


@functools.lru_cache(maxsize=None)
def content(pattern, G):
    """(rows of (word 0, word 1, predecessor), their slots after a sequential insert into G groups), seeded by (pattern, G)"""
    cap, rng = G * 64, np.random.default_rng([PATTERNS.index(pattern), G])
    n = {"half": cap // 2, "crowded": int(0.95 * cap), "clustered": min(cap // 2, 128), "shared word 0": cap // 2, "empty": 0, "single": 1}[pattern]
    w0 = rng.integers(1, 1 << 62, size=n, dtype=U64) * U64(2) + U64(1)
    if pattern == "clustered":   # keys of the first and of the last group, slot 63 of it: chains that leave every window, and wrap
        key = np.where(np.arange(n) % 2 == 0, U64(0), U64(0xFFFFFFFF))
        w0 = (rng.integers(1, 1 << 23, size=n, dtype=U64) << U64(40)) | (key << U64(8)) | U64(63)
    if pattern == "shared word 0":   # runs of four under one word 0, told apart by word 1, arriving interleaved
        w0 = rng.permutation(np.repeat(w0[:-(-n // 4)], 4)[:n])
    other = rng.integers(0, 1 << 63, size=(n, 2), dtype=U64) * U64(2) + rng.integers(0, 2, size=(n, 2), dtype=U64)
    if n >= 2:
        other[0], other[-1] = 0, U64(ONES)   # (0 and all-ones are values like any other, in word 1 and in a predecessor)
    rows = np.concatenate([w0[:, None], other], axis=1)
    return rows, rr.place(w0, cap)


def old_tables(pattern, G, tag):
    SW, SP = SHAPES[tag]
    rows, at = content(pattern, G)
    return rr.fill(rows[:, [0] + [1] * (SW == 2) + [2] * SP], at, G * 64, SW, SP), len(rows)


def cases(hows=(None,)):
    """every geometry, shape, content [and way to unpack; skipped: more entries than the loader itself takes into G' groups]"""
    return [pytest.param(g, t, p, *([h] if h else []), id=f"{g[0]}-{g[1]}-{t}-{p}" + (f"-{h}" if h else ""),
                         marks=[] if not h or len(content(p, g[0])[0]) <= LOAD_LIMIT * 64 * g[1] else pytest.mark.skip("over the load limit"))
            for g in GEOMETRIES for t in SHAPES for p in PATTERNS for h in hows
            if (p != "shared word 0" or SHAPES[t][0] == 2) and (h != "window" or g[3])]


def test_few_combinations_are_over_the_load_limit():
    unpacks = cases(("window", "scatter"))
    assert 0 < 4 * len([c for c in unpacks if c.marks]) < len(unpacks) and not any(c.marks for c in cases())


@pytest.fixture(scope="module")
def mod():
    m = rr.RehashModule()
    yield m
    m.close()


def launch(mod, name, args, blocks, lds=0):
    """a kernel of the shipped object, as kmc_ckpt_compact.cpp launches it"""
    f = C.c_void_p()
    mod._try(mod.hip.hipModuleGetFunction(C.byref(f), mod.mod, name.encode()), name)
    assert 1 <= blocks <= 4096 and lds <= 64 * 1024
    size = C.c_size_t(C.sizeof(args))
    config = (C.c_void_p * 5)(1, C.addressof(args), 2, C.addressof(size), 3)
    mod._try(mod.hip.hipModuleLaunchKernel(f, blocks, 1, 1, rr.REHASH_BLOCK, 1, 1, lds, None, None, config), name)


def packed(old, G, SW, SP, per):
    """(g0, g1, entries, index) of every stretch of `per` groups, by numpy"""
    for g0 in range(0, G, per):
        g1 = min(g0 + per, G)
        slots = old[0].reshape(G * 64, SW)[g0 * 64:g1 * 64]
        occ = np.flatnonzero(slots[:, 0])
        rows = slots[occ] if not SP else np.concatenate([slots[occ], old[1][g0 * 64:g1 * 64][occ, None]], axis=1)
        yield g0, g1, rows.reshape(-1), np.searchsorted(occ, np.arange(-(-(g1 - g0) // T) + 1) * T * 64).astype(U64)


def intact(bufs):
    return all((b.read()[1] == U64(rr.MARGIN_WORD)).all() for b in bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("geometry, tag, pattern", cases())
def test_pack(mod, geometry, tag, pattern):
    G, per = geometry[0], geometry[5]
    SW, SP = SHAPES[tag]
    EW = rr.entry_words(SW, SP)
    old, n = old_tables(pattern, G, tag)
    b_tab, b_pred = Guarded("the table", G * 64 * SW, 1024, old[0]), Guarded("the predecessor table", G * 64, 1024, old[1] if SP else 0)
    b_ctl = Guarded("the control block", CTL_WORDS, 1024, 0)
    for g0, g1, want_e, want_i in packed(old, G, SW, SP, per):
        cap = len(want_e) // EW
        b_e, b_i = Guarded("the entries", max(cap, 1) * EW, 1024, POISON_WORD), Guarded("the index", len(want_i), 1024, POISON_WORD)
        a = KmcCompactArgs(g_first=g0, g_end=g1, index=b_i.ptr, entries=b_e.ptr, entries_cap=cap)
        a.r.old_tab, a.r.old_pred, a.r.old_cap, a.r.ctl = b_tab.ptr, b_pred.ptr if SP else 0, G * 64, b_ctl.ptr
        assert g0 % T == 0 and g1 <= G
        launch(mod, f"kmc_pack_count_{tag}", a, len(want_i) - 1)
        launch(mod, "kmc_pack_scan", a, 1)
        launch(mod, f"kmc_pack_write_{tag}", a, 2)   # (fewer workgroups than tiles: a workgroup goes on to its next tile)
        mod.sync()
        assert np.array_equal(b_i.read()[0], want_i) and np.array_equal(b_e.read()[0][:cap * EW], want_e) and intact([b_e, b_i])
    ctl = rr.KmcRehashCtl.from_buffer_copy(b_ctl.read()[0].tobytes())
    assert (ctl.err, ctl.placed_global) == (0, n) and intact([b_tab, b_pred, b_ctl])
    assert np.array_equal(b_tab.read()[0], old[0]) and (not SP or np.array_equal(b_pred.read()[0], old[1]))


def unpack(mod, tag, old, G, G2, how, span=8, win_groups=0, grid=1, per=8, list_cap=None):
    """entries + index of an old table rebuilt in G2 groups -> (violations of the predicate, control block, new table).  window:
    the destination poisoned, kmc_unpack_window per stretch, then kmc_rehash_overflow over the list; scatter: the destination
    cleared, kmc_rehash_overflow over every stretch's entries."""
    SW, SP = SHAPES[tag]
    EW = rr.entry_words(SW, SP)
    first = POISON_WORD if how == "window" else 0
    list_cap = G * 64 if list_cap is None else list_cap
    b_new, b_npred = Guarded("the new table", G2 * 64 * SW, 1024, first), Guarded("the new predecessor table", G2 * 64, 1024, first)
    b_list, b_ctl = Guarded("the overflow list", max(list_cap, 1) * EW, 1024, POISON_WORD), Guarded("the control block", CTL_WORDS, 1024, 0)
    bufs = [b_new, b_npred, b_list, b_ctl]
    for g0, g1, e, ix in packed(old, G, SW, SP, per):
        n = len(e) // EW
        b_e, b_i = Guarded("the entries", max(n, 1) * EW, 1024, e if n else 0), Guarded("the index", len(ix), 1024, ix)
        bufs += [b_e, b_i]
        a = KmcCompactArgs(g_first=g0, g_end=g1, index=b_i.ptr, entries=b_e.ptr, entries_cap=n)
        r = a.r
        r.new_tab, r.new_pred, r.old_cap, r.new_cap = b_new.ptr, b_npred.ptr if SP else 0, G * 64, G2 * 64
        r.span, r.win_slots, r.list, r.list_cap, r.ctl = span, win_groups * 64, b_list.ptr, list_cap, b_ctl.ptr
        r.old_tab = r.old_pred = b_list.ptr   # (read by nothing: rehash_ref's launcher wants them set)
        assert g0 % T == 0 and g1 <= G and ix[-1] == n and (np.diff(ix.astype(np.int64)) >= 0).all()
        if how == "window":
            launch(mod, f"kmc_unpack_window_{tag}", a, grid, win_groups * 64 * EW * 8)
        else:   # the stretch's entries are the list: ctl.listed says how many (placed_global goes on adding up)
            mod.sync()
            b_ctl.dev[b_ctl.margin] = n
            b_ctl.dev.cpu()
            r.list, r.list_cap = b_e.ptr, n
            mod.launch("overflow", tag, r, max(1, -(-n // rr.REHASH_BLOCK)))
    if how == "window":
        mod.launch("overflow", tag, r, max(1, -(-min(list_cap, G * 64) // rr.REHASH_BLOCK)))
    mod.sync()
    new = (b_new.read()[0], b_npred.read()[0] if SP else None)
    margins = [(b.name, (b.read()[1], np.full(2 * b.margin, rr.MARGIN_WORD, dtype=U64))) for b in bufs]
    return (rr.rehash_violations(old, new, G * 64, G2 * 64, SW, SP, old, margins), rr.KmcRehashCtl.from_buffer_copy(b_ctl.read()[0].tobytes()), new[0])


@pytest.mark.gpu
@pytest.mark.parametrize("geometry, tag, pattern, how", cases(("window", "scatter")))
def test_unpack(mod, geometry, tag, pattern, how):
    G, G2, span, win, grid, per = geometry
    old, n = old_tables(pattern, G, tag)
    assert how == "scatter" or rr.window_fits(G, G2, span, win * 64)
    violations, c, _ = unpack(mod, tag, old, G, G2, how, span or 8, win or 0, grid, per)
    assert violations == []
    assert c.err == 0 and c.placed_window + c.placed_global == n and (c.listed == c.placed_global if how == "window" else c.placed_window == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(SHAPES))
def test_error_flags(mod, tag):
    # the list is full: the clustered chains leave both windows of 16 -> 16 groups, and the list holds one entry
    old, n = old_tables("clustered", 16, tag)
    violations, c, _ = unpack(mod, tag, old, 16, 16, "window", 8, 8, 1, 16, list_cap=1)
    assert c.err == ERR_LIST_FULL and c.listed > 1 and c.placed_window + c.listed == n and not any("clause 5" in v for v in violations)
    # the window is too small: nothing of the run is written
    _, c, new = unpack(mod, tag, old_tables("half", 3, tag)[0], 3, 7, "window", 8, 6, 1, 8)
    assert c.err == ERR_WINDOW and c.placed_window == 0 and (new == U64(POISON_WORD)).all()
    # the table is full: 121 entries for 64 slots
    old, n = old_tables("crowded", 2, tag)
    violations, c, _ = unpack(mod, tag, old, 2, 1, "scatter")
    assert c.err == ERR_TABLE_FULL and c.placed_global == 64 and n > 64 and not any("clause 5" in v for v in violations)
