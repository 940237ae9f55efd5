"""tests/rehash_ref.py is what tests/test_gpu_rehash_direct.py judges the rehash kernels by, so it is held to account here,
without a GPU: its ctypes mirrors and slot functions against csrc/kmc_rehash.h and csrc/kmc_common.h as g++ compiles them, its
predicate against a correct image and one mutant per way a rehash can go wrong, its windows against the bound window_span
(csrc/kmc_growth_engine.cpp) rests on."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import rehash_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64

PROBE = r'''
#define KMC_HOST_EMU 1
#include "kmc_rehash.h"
#include <cstddef>
#include <cstdio>
int main() {
    printf("ctl %zu %zu %zu %zu %zu %zu\n", sizeof(KmcRehashCtl), alignof(KmcRehashCtl), offsetof(KmcRehashCtl, listed),
           offsetof(KmcRehashCtl, placed_window), offsetof(KmcRehashCtl, placed_global), offsetof(KmcRehashCtl, err));
    printf("args %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(KmcRehashArgs), offsetof(KmcRehashArgs, old_tab),
           offsetof(KmcRehashArgs, old_pred), offsetof(KmcRehashArgs, new_tab), offsetof(KmcRehashArgs, new_pred),
           offsetof(KmcRehashArgs, old_cap), offsetof(KmcRehashArgs, new_cap), offsetof(KmcRehashArgs, span),
           offsetof(KmcRehashArgs, win_slots), offsetof(KmcRehashArgs, list), offsetof(KmcRehashArgs, list_cap), offsetof(KmcRehashArgs, ctl));
    printf("flags %u %u %u %d\n", KMC_REHASH_ERR_LIST_FULL, KMC_REHASH_ERR_WINDOW, KMC_REHASH_ERR_TABLE_FULL, KMC_REHASH_BLOCK);
    const unsigned long long caps[] = {64ull, 128ull, 192ull, 5 * 64ull, 7 * 64ull, 33 * 64ull, 1024ull, 1088ull, 1ull << 20,
                                       12500000000ull / 64 * 64, (1ull << 38) - 64};
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (unsigned long long cap : caps) {
        for (int k = 0; k < 40; ++k) {
            x = kmc_mix64(x + 0x9E3779B97F4A7C15ull);
            unsigned long long fp = x ? x : 1;
            if (k == 0) fp = ~0ull;                               // every bit
            if (k == 1) fp = 0xFFFFFFFFull << 8;                  // every key bit, nothing else
            if (k == 2) fp |= 0xFFFFFFFFull << 8;                 // every key bit among others
            if (k == 3) fp = 63;                                  // no key bit
            if (k == 4) fp &= ~(0xFFFFFFFFull << 8), fp |= 1;
            const unsigned long long i = kmc_slot_of(fp, cap);
            printf("slot %llu %llu %llu %llu\n", fp, cap, i, kmc_slot_next(i, cap));
        }
        printf("next %llu %llu %llu\n", cap, kmc_slot_next(cap - 1, cap), kmc_slot_next(cap - 2, cap));
    }
    return 0;
}
'''


def test_the_mirrors_and_the_slot_functions_are_the_headers(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "kafka_specification_amd", "csrc"), "-o", str(exe), str(src)])
    lines = [l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    by = lambda kind: [[int(x) for x in l[1:]] for l in lines if l[0] == kind]
    ctl, args = rr.KmcRehashCtl, rr.KmcRehashArgs
    assert by("ctl") == [[C.sizeof(ctl), 128, ctl.listed.offset, ctl.placed_window.offset, ctl.placed_global.offset, ctl.err.offset]]
    assert C.sizeof(ctl) % 128 == 0
    assert by("args") == [[C.sizeof(args)] + [getattr(args, f).offset for f, _ in args._fields_]]
    assert [f for f, _ in args._fields_] == ["old_tab", "old_pred", "new_tab", "new_pred", "old_cap", "new_cap", "span", "win_slots", "list",
                                             "list_cap", "ctl"]
    assert by("flags") == [[rr.ERR_LIST_FULL, rr.ERR_WINDOW, rr.ERR_TABLE_FULL, rr.REHASH_BLOCK]]
    slots = by("slot")
    assert len(slots) >= 400 and {cap for _, cap, _, _ in slots} >= {64, 192, 7 * 64, 1088}
    assert any((fp >> 8) & 0xFFFFFFFF == 0xFFFFFFFF for fp, _, _, _ in slots)
    for fp, cap, i, nxt in slots:
        assert rr.slot_of(fp, cap) == i and rr.slot_next(i, cap) == nxt and i < cap, (fp, cap)
    for cap, wrapped, last in by("next"):
        assert (rr.slot_next(cap - 1, cap), rr.slot_next(cap - 2, cap)) == (wrapped, last) == (0, cap - 1)
    # ... and the array form of slot_of is the scalar one
    for cap in sorted({cap for _, cap, _, _ in slots}):
        fps = np.array([fp for fp, c, _, _ in slots if c == cap], dtype=U64)
        assert rr.slot_of(fps, cap).tolist() == [i for _, c, i, _ in slots if c == cap]


# -- the predicate ---------------------------------------------------------------------------------------------------------
OLD_CAP, NEW_CAP = 128, 192
MARGIN = np.full(32, rr.MARGIN_WORD, dtype=U64)


def base(SW, SP):
    """(rows, old, new): 60-odd entries; two whose home is the last slot of the new table (one wraps to slot 0, nothing else
    lives near the wrap); for two-word slots two that share word 0; 0 and all-ones among the other words."""
    EW = rr.entry_words(SW, SP)
    rng = np.random.default_rng(1000 + 10 * SW + SP)
    rows = rng.integers(1, 1 << 63, size=(70, EW), dtype=U64) * U64(2) + U64(1)
    home = rr.slot_of(rows[:, 0], NEW_CAP)
    rows = rows[(home > 6) & (home < NEW_CAP - 8)]
    assert len(rows) > 50
    wrap = np.array([[(0xABCDEF << 40) | (0xFFFFFFFF << 8) | (k << 6) | 63] + [int(x) for x in rng.integers(1, 1 << 62, size=EW - 1)]
                     for k in range(2)], dtype=U64).reshape(2, EW)
    rows = np.concatenate([wrap, rows])
    if EW > 1:
        rows[5, 1:] = 0
        rows[6, 1:] = U64(0xFFFFFFFFFFFFFFFF)
    if SW == 2:
        rows[11, 0] = rows[10, 0]
    old = rr.build_table(rows, OLD_CAP, SW, SP, order=list(range(len(rows)))[::-1])
    new = rr.build_table(rows, NEW_CAP, SW, SP)
    return rows, old, new


class Image:
    """A new table a mutant may edit slot by slot."""

    def __init__(self, new, SW, SP):
        self.SW, self.SP = SW, SP
        self.tab, self.pred = new[0].copy(), None if new[1] is None else new[1].copy()

    def get(self, i):
        return [int(x) for x in self.tab[i * self.SW:(i + 1) * self.SW]] + ([int(self.pred[i])] if self.SP else [])

    def put(self, i, e):
        self.tab[i * self.SW:(i + 1) * self.SW] = e[:self.SW]
        if self.SP:
            self.pred[i] = e[self.SW]

    def clear(self, i):
        self.put(i, [0] * (self.SW + 1))

    def full(self, i):
        return self.tab[(i % NEW_CAP) * self.SW] != 0

    def home(self, i):
        return rr.slot_of(int(self.tab[i * self.SW]), NEW_CAP)


def _find(cond):
    return next(i for i in range(8, NEW_CAP - 8) if cond(i))


def m_dropped(im, old, margins, rows):
    im.clear(_find(lambda i: im.full(i) and not im.full(i + 1)))   # (the end of a chain: nothing behind it loses its path)


def m_duplicated(im, old, margins, rows):
    i = _find(lambda i: im.full(i) and not im.full(i + 1))
    im.put(i + 1, im.get(i))


def m_before_its_home(im, old, margins, rows):
    i = _find(lambda i: im.full(i) and im.home(i) == i and not im.full(i - 1) and not im.full(i + 1))
    im.put(i - 1, im.get(i))
    im.clear(i)


def m_hole_in_a_chain(im, old, margins, rows):
    i = _find(lambda i: im.full(i) and im.full(i + 1) and im.home(i + 1) <= i)   # the entry behind slot i was displaced across it
    e = next(j for j in range(i + 2, NEW_CAP) if not im.full(j))
    im.put(e, im.get(i))
    im.clear(i)


def m_wrapped_entry_past_the_end(im, old, margins, rows):
    assert im.full(NEW_CAP - 1) and im.full(0) and im.home(0) == NEW_CAP - 1 and not im.full(1)
    e = im.get(0)
    margins["the new table"][0][16:16 + im.SW] = e[:im.SW]   # (the upper margin begins at word 16 of the pair)
    if im.SP:
        margins["the new predecessor table"][0][16] = e[im.SW]
    im.clear(0)


def m_predecessors_swapped(im, old, margins, rows):
    i = _find(im.full)
    j = _find(lambda j: j > i and im.full(j) and im.pred[j] != im.pred[i])
    im.pred[i], im.pred[j] = im.pred[j], im.pred[i]


def m_word_1_swapped_under_one_word_0(im, old, margins, rows):
    i, j = [k for k in range(NEW_CAP) if im.tab[2 * k] == rows[10, 0]]
    assert im.tab[2 * i + 1] != im.tab[2 * j + 1]
    im.tab[2 * i + 1], im.tab[2 * j + 1] = im.tab[2 * j + 1], im.tab[2 * i + 1]


def m_word_1_doubled_under_one_word_0(im, old, margins, rows):
    i, j = [k for k in range(NEW_CAP) if im.tab[2 * k] == rows[10, 0]]
    im.tab[2 * j + 1] = im.tab[2 * i + 1]


def m_word_left_in_an_empty_slot(im, old, margins, rows):
    im.tab[_find(lambda i: not im.full(i)) * 2 + 1] = 5


def m_predecessor_left_in_an_empty_slot(im, old, margins, rows):
    im.pred[_find(lambda i: not im.full(i))] = 7


def m_old_table_modified(im, old, margins, rows):
    old[0][int(np.flatnonzero(old[0])[3])] ^= U64(1 << 40)


def m_old_predecessors_modified(im, old, margins, rows):
    old[1][17] ^= U64(1)


def m_margin_modified(im, old, margins, rows):
    margins["the overflow list"][0][31] ^= U64(1 << 63)


# mutant -> (the clauses it violates, the shapes it exists for)
MUTANTS = {
    m_dropped: ({1}, "1n 1p 2n 2p"),
    m_duplicated: ({1}, "1n 1p 2n 2p"),
    m_before_its_home: ({2}, "1n 1p 2n 2p"),
    m_hole_in_a_chain: ({2}, "1n 1p 2n 2p"),
    m_wrapped_entry_past_the_end: ({1, 5}, "1n 1p 2n 2p"),
    m_predecessors_swapped: ({1}, "1p 2p"),
    # (where nothing but word 1 tells the two entries apart — 2n — the swapped image holds the same entries in slots either may
    # claim: it is a correct image, so the mutant exists only where the predecessor word stays behind; 2n gets the next one)
    m_word_1_swapped_under_one_word_0: ({1}, "2p"),
    m_word_1_doubled_under_one_word_0: ({1}, "2n 2p"),
    m_word_left_in_an_empty_slot: ({3}, "2n 2p"),
    m_predecessor_left_in_an_empty_slot: ({3}, "1p 2p"),
    m_old_table_modified: ({4}, "1n 1p 2n 2p"),
    m_old_predecessors_modified: ({4}, "1p 2p"),
    m_margin_modified: ({5}, "1n 1p 2n 2p"),
}


def _margins():
    return {name: (MARGIN.copy(), MARGIN) for name in ("the old table", "the new table", "the new predecessor table", "the overflow list")}


@pytest.mark.parametrize("tag", list(rr.SHAPES))
def test_the_predicate_accepts_a_sequential_rehash(tag):
    SW, SP = rr.SHAPES[tag]
    rows, old, new = base(SW, SP)
    assert rr.check_rehash(old, new, OLD_CAP, NEW_CAP, SW, SP, old, list(_margins().items())) is None
    # ... whatever the order of the inserts, at a ratio just above 1 too, and for the empty table
    for cap, seed in ((OLD_CAP + 64, 1), (NEW_CAP, 2), (7 * 64, 3)):
        order = list(range(len(rows)))
        random.Random(seed).shuffle(order)
        assert rr.check_rehash(old, rr.build_table(rows, cap, SW, SP, order), OLD_CAP, cap, SW, SP, old) is None
    none = rr.build_table(np.zeros((0, rr.entry_words(SW, SP)), dtype=U64), 64, SW, SP)
    assert rr.check_rehash(none, rr.build_table([], 128, SW, SP), 64, 128, SW, SP, none) is None
    # the image holds what the mutants need: a chain that wraps, displaced entries, entries under one word 0
    assert new[0][(NEW_CAP - 1) * SW] and new[0][0] and rr.slot_of(int(new[0][0]), NEW_CAP) == NEW_CAP - 1


@pytest.mark.parametrize("tag,mutant", [(t, m) for m, (_, tags) in MUTANTS.items() for t in tags.split()],
                         ids=lambda v: v if isinstance(v, str) else v.__name__[2:])
def test_the_predicate_rejects(tag, mutant):
    SW, SP = rr.SHAPES[tag]
    rows, old, new = base(SW, SP)
    before = (old[0].copy(), None if old[1] is None else old[1].copy())
    im, margins = Image(new, SW, SP), _margins()
    mutant(im, old, margins, rows)
    said = rr.rehash_violations(old, (im.tab, im.pred), OLD_CAP, NEW_CAP, SW, SP, before, list(margins.items()))
    print(said)
    assert {int(s.split(":")[0].split()[1]) for s in said} == MUTANTS[mutant][0]
    assert all(s.startswith("clause ") for s in said)
    assert rr.check_rehash(old, (im.tab, im.pred), OLD_CAP, NEW_CAP, SW, SP, before, list(margins.items())) == said[0]


def test_the_windows_partition_the_new_table_and_fit_the_bound_the_host_relies_on():
    rng = random.Random(20)
    for k in range(4000):
        G = rng.randint(1, 300 if k % 2 else 12)
        G2 = G + rng.choice([0, 1, 2, rng.randint(0, G), rng.randint(0, 20 * G)])
        span = rng.randint(1, G + 2)
        w = rr.windows(G, G2, span)
        assert len(w) == (G + span - 1) // span and w[0][0] == 0 and w[-1][1] == G2 * 64
        assert all(a[1] == b[0] for a, b in zip(w, w[1:])) and all(lo < hi and lo % 64 == 0 == hi % 64 for lo, hi in w)
        bound = (span * G2 // G + 1) * 64
        assert max(hi - lo for lo, hi in w) <= bound and rr.window_fits(G, G2, span, bound)
        assert not rr.window_fits(G, G2, span, max(hi - lo for lo, hi in w) - 64)
        # the host's choice of span for a window of `groups` groups: every tile fits, or there is no span
        groups = rng.randint(1, 400)
        s = rr.window_span(groups, G, G2)
        assert s == 0 and (groups < 2 or (groups - 1) * G < G2) or rr.window_fits(G, G2, s, groups * 64)


def test_turned_away_counts_what_the_windows_turn_away():
    """Counted by hand: one window over the whole table turns away what a table without wrap-around cannot hold; five entries
    under one home, at either end of a table of two groups that doubles, tiles of one group and of two."""
    rows, old, new = base(1, False)
    assert rr.turned_away(old[0], OLD_CAP, NEW_CAP, 2, 1) == 1            # the one entry that wraps
    first = np.array([(k << 40) | 63 for k in range(1, 6)], dtype=U64)    # key 0: home 63 of 128, and of 256
    tab, _ = rr.build_table(first[:, None], 128, 1, False)
    assert np.flatnonzero(tab).tolist() == [63, 64, 65, 66, 67]
    assert rr.turned_away(tab, 128, 256, 1, 1) == 4     # four lie in the second tile, whose window [128, 256) is not their home's
    assert rr.turned_away(tab, 128, 256, 2, 1) == 0
    last = first | U64(0xFFFFFFFF << 8)                                   # every key bit: home 127 of 128, 255 of 256
    tab, _ = rr.build_table(last[:, None], 128, 1, False)
    assert np.flatnonzero(tab).tolist() == [0, 1, 2, 3, 127]
    assert rr.turned_away(tab, 128, 256, 1, 1) == 4     # the four that wrapped lie in the first tile
    assert rr.turned_away(tab, 128, 256, 2, 1) == 4     # one window: one fits its last slot, four run off its end
    assert rr.turned_away(tab, 128, 256, 2, 1, skip=lambda lo, hi: True) == 0


def test_the_path_of_the_table_code_object_names_the_object_the_engine_loads():
    """kmc_table_code_object_path: no GPU needed; a gfx950 ELF image under <cache>/table/ with the compiler's identity in its name,
    holding the three kernels of every entry shape — what the direct GPU test launches."""
    from kafka_specification_amd import compiler_identity, precompile_table, table_code_object_path
    precompile_table()
    path = table_code_object_path()
    assert os.path.basename(os.path.dirname(path)) == "table" and os.path.basename(path).startswith("kmc_table-gfx950-")
    assert any(path.endswith(f"-c{compiler_identity(which)}.hsaco") for which in (0, 1))   # this process's compiler, or the pinned one
    image = open(path, "rb").read()
    assert image[:4] == b"\x7fELF"
    for kind in ("window", "overflow", "scatter"):
        for tag in rr.SHAPES:
            assert f"kmc_rehash_{kind}_{tag}".encode() in image
    assert table_code_object_path("gfx950") == path
