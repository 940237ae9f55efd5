"""Reference side of the rehash kernels (csrc/kmc_rehash.h), in plain Python and numpy: the two slot functions of kmc_common.h,
ctypes mirrors of the kernels' argument and control blocks, a sequential open-addressing insert, the predicate a rehashed table
must satisfy (placement under races is not deterministic: the predicate says what every correct image has in common), the tiles'
windows by the header's formula, and — for tests/test_gpu_rehash_direct.py only — a launcher of the shipped code object.
Importable without a GPU: tests/test_rehash_ref_cpu.py holds the mirrors against the header and the predicate against mutants."""
import ctypes as C

import numpy as np

U64 = np.uint64
REHASH_BLOCK = 256
ERR_LIST_FULL, ERR_WINDOW, ERR_TABLE_FULL = 1, 2, 4
MARGIN_WORD = 0xA5C3A5C3_5A3C5A3C     # what the words around every buffer hold
POISON_WORD = 0xDEAD_F00D_DEAD_F00D   # what the new tables hold before a windowed launch (nonzero: an unwritten slot looks occupied)


# -- kmc_common.h ---------------------------------------------------------------------------------------------------------
def slot_of(fp, cap):
    """kmc_slot_of: bits 8..39 of the fingerprint scaled onto the 64-slot groups, its low six bits the slot of the group.
    Python ints or numpy uint64 arrays (the product of two 32-bit values fits 64 bits)."""
    if isinstance(fp, np.ndarray):
        key = (fp >> U64(8)) & U64(0xFFFFFFFF)
        return (((key * U64((cap >> 6) & 0xFFFFFFFF)) >> U64(32)) << U64(6)) | (fp & U64(63))
    return (((((fp >> 8) & 0xFFFFFFFF) * ((cap >> 6) & 0xFFFFFFFF)) >> 32) << 6) | (fp & 63)


def slot_next(i, cap):
    return 0 if i + 1 == cap else i + 1


# -- kmc_rehash.h ---------------------------------------------------------------------------------------------------------
class KmcRehashCtl(C.Structure):   # alignas(128): 256 bytes
    _fields_ = [("listed", C.c_uint64), ("listed_pad_", C.c_uint64 * 15), ("placed_window", C.c_uint64), ("placed_global", C.c_uint64),
                ("err", C.c_uint32), ("pad_", C.c_uint32), ("tail_", C.c_uint64 * 13)]


class KmcRehashArgs(C.Structure):
    _fields_ = [("old_tab", C.c_uint64), ("old_pred", C.c_uint64), ("new_tab", C.c_uint64), ("new_pred", C.c_uint64),
                ("old_cap", C.c_uint64), ("new_cap", C.c_uint64), ("span", C.c_uint64), ("win_slots", C.c_uint64),
                ("list", C.c_uint64), ("list_cap", C.c_uint64), ("ctl", C.c_uint64)]


SHAPES = {"1n": (1, False), "1p": (1, True), "2n": (2, False), "2p": (2, True)}   # tag -> (slot words, predecessors apart)


def entry_words(SW, SP):
    return SW + (1 if SP else 0)


# -- tables ---------------------------------------------------------------------------------------------------------------
def place(word0, cap, order=None):
    """Slot of every entry after a sequential insert in `order` (default: as given): linear probing from kmc_slot_of, wrapping."""
    taken = bytearray(cap)
    at = [0] * len(word0)
    if len(word0) > cap:
        raise ValueError("more entries than slots")
    for k in (range(len(word0)) if order is None else order):
        i = slot_of(int(word0[k]), cap)
        while taken[i]:
            i = slot_next(i, cap)
        taken[i] = 1
        at[k] = i
    return np.asarray(at, dtype=np.int64)


def fill(entries, at, cap, SW, SP):
    """(tab[cap * SW], pred[cap] or None) with entry k — a row of SW [+ 1] words — in slot at[k]."""
    entries = np.asarray(entries, dtype=U64).reshape(-1, entry_words(SW, SP))
    tab = np.zeros(cap * SW, dtype=U64)
    pred = np.zeros(cap, dtype=U64) if SP else None
    for w in range(SW):
        tab[at * SW + w] = entries[:, w]
    if SP:
        pred[at] = entries[:, SW]
    return tab, pred


def build_table(entries, cap, SW, SP, order=None):
    """A sequential open-addressing insert of `entries` (rows of SW words [+ the predecessor word]; word 0 never 0)."""
    entries = np.asarray(entries, dtype=U64).reshape(-1, entry_words(SW, SP))
    if len(entries) and not entries[:, 0].all():
        raise ValueError("word 0 of an entry is never 0")
    return fill(entries, place(entries[:, 0], cap, order), cap, SW, SP)


def entries_of(tab, pred, cap, SW, SP):
    """The occupied slots' entries as rows, in a canonical order, and the occupied slots' indices."""
    slots = tab.reshape(cap, SW)
    occ = np.flatnonzero(slots[:, 0])
    rows = slots[occ]
    if SP:
        rows = np.concatenate([rows, pred[occ, None]], axis=1)
    if len(rows):
        rows = rows[np.lexsort(rows.T[::-1])]
    return rows, occ


def rehash_violations(old, new, old_cap, new_cap, SW, SP, old_before=None, margins=()):
    """Every clause a rehash of `old` = (tab, pred) into `new` = (tab, pred) violates, as text, in the order of the clauses:
      1  the entries of the new table are, as a multiset, the entries of the old one (all words, and the predecessor word of the slot)
      2  every slot on the cyclic probe path from an entry's home to where it lies is occupied
      3  an unoccupied slot is zero in all of its words, and so is its predecessor word
      4  the old tables are what they were before the launch (`old_before`)
      5  `margins`, pairs (name, (got, want)) of the words around the buffers, are intact"""
    out = []
    otab, opred = old
    ntab, npred = new
    want, _ = entries_of(*(old_before if old_before is not None else old), old_cap, SW, SP)   # (what the launch was given)
    got, occ = entries_of(ntab, npred, new_cap, SW, SP)
    if want.shape != got.shape:
        out.append(f"clause 1: the new table holds {len(got)} entries, the old one {len(want)}")
    elif not np.array_equal(want, got):
        k = int(np.flatnonzero((want != got).any(axis=1))[0])
        out.append(f"clause 1: the entries differ as multisets; first in sorted order: new {[hex(int(x)) for x in got[k]]}, "
                   f"old {[hex(int(x)) for x in want[k]]}")
    slots = ntab.reshape(new_cap, SW)
    empty = slots[:, 0] == 0
    if len(occ):
        holes = np.concatenate([[0], np.cumsum(empty)])   # holes[i]: empty slots below i
        home = slot_of(slots[occ, 0], new_cap).astype(np.int64)
        on_path = np.where(home <= occ, holes[occ + 1] - holes[home], holes[new_cap] - holes[home] + holes[occ + 1])
        bad = np.flatnonzero(on_path)
        if len(bad):
            k = int(bad[0])
            out.append(f"clause 2: the entry in slot {int(occ[k])} (home {int(home[k])} of {new_cap}) lies behind {int(on_path[k])} empty "
                       f"slot(s) of its probe path: no probe finds it ({len(bad)} such entries)")
    dirty = empty & (slots != 0).any(axis=1)
    if SP:
        dirty |= empty & (npred != 0)
    if dirty.any():
        out.append(f"clause 3: the empty slot {int(np.flatnonzero(dirty)[0])} is not zero in all of its words ({int(dirty.sum())} such slots)")
    if old_before is not None:
        for name, now, then in (("table", otab, old_before[0]), ("predecessor table", opred, old_before[1])):
            if then is not None and not np.array_equal(now, then):
                out.append(f"clause 4: the old {name} changed, first at word {int(np.flatnonzero(now != then)[0])}")
    for name, (now, then) in margins:
        if not np.array_equal(now, then):
            out.append(f"clause 5: the margin of {name} changed, first at word {int(np.flatnonzero(now != then)[0])}")
    return out


def check_rehash(old, new, old_cap, new_cap, SW, SP, old_before=None, margins=()):
    """The first violation of rehash_violations as text, or None."""
    v = rehash_violations(old, new, old_cap, new_cap, SW, SP, old_before, margins)
    return v[0] if v else None


# -- the windows ----------------------------------------------------------------------------------------------------------
def windows(G, G2, span):
    """[lo, hi) in new slots of every tile of `span` old groups: tile t owns the new groups [floor(t span G'/G), floor(min((t+1) span, G) G'/G))."""
    out = []
    for g0 in range(0, G, span):
        g1 = min(g0 + span, G)
        out.append(((g0 * G2 // G) << 6, (g1 * G2 // G) << 6))
    return out


def window_fits(G, G2, span, win_slots):
    return all(hi - lo <= win_slots for lo, hi in windows(G, G2, span))


def window_span(win_groups, G, G2):
    """kmc_growth_engine.cpp's choice of span for a window of win_groups groups (0: no window holds a whole tile)."""
    return 0 if win_groups < 2 else (win_groups - 1) * G // G2


def turned_away(old_tab, old_cap, new_cap, span, SW, skip=lambda lo, hi: False):
    """How many entries the windows of a rehash turn away: home outside the tile's window, or a chain that runs off its end.  The
    number does not depend on the order in which a window's entries arrive (a slot keeps one of those that reach it and
    passes the others on).  Tiles for which skip(lo, hi) holds list nothing (the kernel leaves them out: KMC_REHASH_ERR_WINDOW)."""
    word0 = old_tab.reshape(old_cap, SW)[:, 0]
    n = 0
    for t, (lo, hi) in enumerate(windows(old_cap >> 6, new_cap >> 6, span)):
        if skip(lo, hi):
            continue
        taken = bytearray(hi - lo)
        for fp in word0[t * span * 64:(t + 1) * span * 64]:
            if not fp:
                continue
            p = slot_of(int(fp), new_cap)
            if lo <= p < hi:
                p -= lo
                while p < hi - lo and taken[p]:
                    p += 1
                if p < hi - lo:
                    taken[p] = 1
                    continue
            n += 1
    return n


# -- the launcher (GPU tests only) ----------------------------------------------------------------------------------------
class Guarded:
    """A device buffer of `words` 64-bit words inside a larger allocation whose margins, `margin` words on either side, hold
    MARGIN_WORD.  `init`: the interior's content (an array, or one word for all of it)."""

    def __init__(self, name, words, margin, init=0):
        import torch
        assert margin % 16 == 0 and margin > 0   # (the interior stays 128-byte aligned)
        self.name, self.words, self.margin = name, words, margin
        host = np.full(words + 2 * margin, MARGIN_WORD, dtype=U64)
        host[margin:margin + words] = init
        self.dev = torch.from_numpy(host.view(np.int64)).cuda()
        self.ptr = self.dev.data_ptr() + 8 * margin

    def read(self):
        """(interior, margins) as they are on the device now"""
        host = self.dev.cpu().numpy().view(U64)
        m = self.margin
        return host[m:m + self.words], np.concatenate([host[:m], host[m + self.words:]])


class RehashModule:
    """The shipped table code object, loaded once: kmc_rehash_{window,overflow,scatter}_<tag> launched as the engine launches them."""

    def __init__(self):
        import torch
        from kafka_specification_amd import table_code_object_path
        torch.cuda.init()
        torch.zeros(1, device="cuda")   # (the context is torch's)
        self.hip = C.CDLL("libamdhip64.so")
        for fn in ("hipModuleLoadData", "hipModuleGetFunction", "hipModuleLaunchKernel", "hipFuncSetAttribute", "hipDeviceSynchronize",
                   "hipModuleUnload"):
            getattr(self.hip, fn).restype = C.c_int
        self.hip.hipModuleLoadData.argtypes = [C.POINTER(C.c_void_p), C.c_char_p]
        self.hip.hipModuleGetFunction.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_char_p]
        self.hip.hipModuleLaunchKernel.argtypes = [C.c_void_p] + [C.c_uint] * 7 + [C.c_void_p, C.c_void_p, C.c_void_p]
        self.hip.hipFuncSetAttribute.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self.hip.hipModuleUnload.argtypes = [C.c_void_p]
        self.image = open(table_code_object_path(), "rb").read()
        self.mod = C.c_void_p()
        self._try(self.hip.hipModuleLoadData(C.byref(self.mod), self.image), "hipModuleLoadData")
        self.fn = {}
        self.lds_asked = {}

    def _try(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with HIP error {rc}")

    def close(self):
        if self.mod:
            self.hip.hipModuleUnload(self.mod)
            self.mod = C.c_void_p()

    def function(self, kind, tag):
        if (kind, tag) not in self.fn:
            f = C.c_void_p()
            self._try(self.hip.hipModuleGetFunction(C.byref(f), self.mod, f"kmc_rehash_{kind}_{tag}".encode()), f"kmc_rehash_{kind}_{tag}")
            self.fn[kind, tag] = f
        return self.fn[kind, tag]

    def launch(self, kind, tag, args, blocks, lds=0):
        SW, SP = SHAPES[tag]
        # what the kernels take for granted (the engine's launches satisfy it; a test must not send anything else to a device)
        assert args.old_cap % 64 == 0 and args.new_cap % 64 == 0 and args.old_cap and args.new_cap
        assert args.old_tab and args.new_tab and args.ctl and (not SP or (args.old_pred and args.new_pred))
        assert 1 <= blocks <= 4096
        if kind == "window":
            assert args.span >= 1 and args.list and lds == args.win_slots * entry_words(SW, SP) * 8 and 0 < lds <= 159 * 1024
        f = self.function(kind, tag)
        if lds > 64 * 1024 and self.lds_asked.get(tag, 0) < lds:   # (more than 64 KiB of dynamic LDS has to be asked for)
            self._try(self.hip.hipFuncSetAttribute(f, 8, lds), "hipFuncSetAttribute(MaxDynamicSharedMemorySize)")
            self.lds_asked[tag] = lds
        size = C.c_size_t(C.sizeof(args))
        config = (C.c_void_p * 5)(1, C.addressof(args), 2, C.addressof(size), 3)   # HIP_LAUNCH_PARAM_BUFFER_POINTER, _SIZE, _END
        self._try(self.hip.hipModuleLaunchKernel(f, blocks, 1, 1, REHASH_BLOCK, 1, 1, lds, None, None, config), f"launch of {kind}_{tag}")

    def sync(self):
        self._try(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")


class RehashRun:
    """One rehash of `old` = (tab, pred) on the device, every buffer guarded.  kernel "window": the new tables poisoned, both
    phases launched back to back as the host does; "scatter": the new tables cleared.  Afterwards: .new, .old_now, .ctl
    (a KmcRehashCtl), .list, and .margins for check_rehash."""

    def __init__(self, mod, tag, kernel, old, old_cap, new_cap, span=1, win_slots=0, grid=1, list_cap=None):
        SW, SP = SHAPES[tag]
        EW = entry_words(SW, SP)
        self.tag, self.old_cap, self.new_cap, self.old_before = tag, old_cap, new_cap, old
        margin = (max(win_slots * EW, 1024) + 15) // 16 * 16
        list_cap = old_cap if list_cap is None else list_cap
        first = POISON_WORD if kernel == "window" else 0
        b = self.buf = {"old table": Guarded("the old table", old_cap * SW, margin, old[0]),
                        "new table": Guarded("the new table", new_cap * SW, margin, first),
                        "list": Guarded("the overflow list", max(list_cap, 1) * EW, margin, POISON_WORD),
                        "ctl": Guarded("the control block", C.sizeof(KmcRehashCtl) // 8, margin, 0)}
        if SP:
            b["old pred"] = Guarded("the old predecessor table", old_cap, margin, old[1])
            b["new pred"] = Guarded("the new predecessor table", new_cap, margin, first)
        a = KmcRehashArgs(old_tab=b["old table"].ptr, old_pred=b["old pred"].ptr if SP else 0, new_tab=b["new table"].ptr,
                          new_pred=b["new pred"].ptr if SP else 0, old_cap=old_cap, new_cap=new_cap, span=span, win_slots=win_slots,
                          list=b["list"].ptr, list_cap=list_cap, ctl=b["ctl"].ptr)
        if kernel == "window":
            mod.launch("window", tag, a, grid, win_slots * EW * 8)
            mod.launch("overflow", tag, a, max(1, (min(list_cap, old_cap) + REHASH_BLOCK - 1) // REHASH_BLOCK))
        else:
            mod.launch("scatter", tag, a, (old_cap + REHASH_BLOCK - 1) // REHASH_BLOCK)
        mod.sync()
        got = {k: g.read() for k, g in b.items()}
        self.new = (got["new table"][0], got["new pred"][0] if SP else None)
        self.old_now = (got["old table"][0], got["old pred"][0] if SP else None)
        self.list = got["list"][0]
        self.ctl = KmcRehashCtl.from_buffer_copy(got["ctl"][0].tobytes())
        self.margins = [(g.name, (got[k][1], np.full(2 * g.margin, MARGIN_WORD, dtype=U64))) for k, g in b.items()]

    def violation(self):
        SW, SP = SHAPES[self.tag]
        return check_rehash(self.old_now, self.new, self.old_cap, self.new_cap, SW, SP, self.old_before, self.margins)
