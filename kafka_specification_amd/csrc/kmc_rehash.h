// kmc_rehash.h — the seen-set grows: the kernels that carry every entry of a table of `old_cap` slots over into one of `new_cap`
// slots (kmc_table_growth_enable, include/kmc.h; the host side is kmc_growth_engine.cpp).
// Model-independent: a code object of its own (kmc_layout.h + kmc_common.h + this file handed to hiprtc, cached under
// kmc_cache/table/), NOT one of the parts kmc_device.h lists — the model-specialised objects do not change with this file.
//
// An ENTRY is a slot's words (1: the fingerprint; 2: fingerprint + check word, or fingerprint + predecessor) plus, where the
// predecessors have a table of their own, the predecessor word of that slot.  All of it moves together; word 0 (never 0 in an
// occupied slot) is the only word a claim looks at.  Fingerprints are never COMPARED: every entry of a table is a distinct
// state by construction, and under wide entries two distinct states may share a fingerprint.
//
// k_rehash_window rests on kmc_slot_of being MONOTONE in the fingerprint's key bits: the home group is floor(key * G / 2^32), so
// a run of consecutive old groups maps onto a run of consecutive new groups, whatever the two sizes.  The old table is cut
// into tiles of `span` groups; tile t owns the new groups [floor(t span G'/G), floor(min((t+1) span, G) G'/G)) — windows that
// partition the new table exactly.  A workgroup builds its window in LDS (linear probing with a 64-bit LDS compare-and-swap)
// and writes it out whole, zeros included, in full lines: the new table is never cleared and never probed at random by
// this phase.  What does not land in the window — an entry the old table's probing had displaced across a tile boundary, a
// boundary group at a non-integer ratio, a chain that runs off the window's end (the last window included: the wrap is phase
// two's) — goes to an overflow list, and k_rehash_overflow places those by global compare-and-swap once every window is written.
// k_rehash_scatter is the plain form: the host clears the new table, one lane per old slot claims by global compare-and-swap.
#pragma once
#include "kmc_common.h"

#define KMC_REHASH_BLOCK 256
#define KMC_REHASH_ERR_LIST_FULL 1u     // the overflow list did not hold what the windows turned away: the host redoes the growth by scatter
#define KMC_REHASH_ERR_WINDOW 2u        // a tile's window exceeds the LDS the launch was given (a host bug: nothing of it was written)
#define KMC_REHASH_ERR_TABLE_FULL 4u    // a global probe chain went once round the new table

struct alignas(128) KmcRehashCtl {
    KmcCounterLine listed;   // entries appended to the overflow list (may exceed list_cap: the excess was not written)
    u64 placed_window;       // entries placed inside their window
    u64 placed_global;       // entries placed by global compare-and-swap (k_rehash_overflow, k_rehash_scatter)
    u32 err;
    u32 pad_;
};

struct KmcRehashArgs {
    const u64* old_tab;      // old_cap slots of SLOT_WORDS words
    const u64* old_pred;     // SEPARATE_PRED: old_cap words
    u64* new_tab;
    u64* new_pred;
    u64 old_cap, new_cap;    // slots: multiples of 64
    u64 span;                // old 64-slot groups per tile
    u64 win_slots;           // slots of LDS window the launch was given
    u64* list;               // overflow list: AoS entries of SLOT_WORDS + SEPARATE_PRED words
    u64 list_cap;            // entries
    KmcRehashCtl* ctl;
};

#ifndef KMC_HOST_EMU
typedef u64 KmcSlot2R __attribute__((ext_vector_type(2)));   // 16 bytes moved as one: a two-word slot, or two one-word slots

// One entry claims a slot of the new table by linear probing from its home, wrapping at the end, and stores its other words.
template <int SW, bool SP>
KMC_DEV bool kmc_rehash_claim_global(const KmcRehashArgs& a, const u64* e) {
    u64 i = kmc_slot_of(e[0], a.new_cap);
    for (u64 probes = 0; probes < a.new_cap; ++probes) {
        if (atomicCAS(&a.new_tab[i * SW], 0ull, e[0]) == 0ull) {
            if constexpr (SW == 2) a.new_tab[i * SW + 1] = e[1];
            if constexpr (SP) a.new_pred[i] = e[SW];
            return true;
        }
        i = kmc_slot_next(i, a.new_cap);
    }
    atomicOr(&a.ctl->err, KMC_REHASH_ERR_TABLE_FULL);
    return false;
}

// slot i of the old table as an entry; false: the slot is empty
template <int SW, bool SP>
KMC_DEV bool kmc_rehash_load(const KmcRehashArgs& a, u64 i, u64* e) {
    if constexpr (SW == 2) {
        const KmcSlot2R s = __builtin_nontemporal_load((const KmcSlot2R*)(a.old_tab + 2 * i));   // one 16-byte load
        e[0] = s[0];
        e[1] = s[1];
    } else {
        e[0] = __builtin_nontemporal_load(a.old_tab + i);
    }
    if constexpr (SP) e[SW] = __builtin_nontemporal_load(a.old_pred + i);
    return e[0] != 0ull;
}

// One entry goes into the LDS window of the new slots [lo, hi): a linear probe from its home, never past the window's end.
// false: the window turns it away (home outside, or the chain runs off the end).
template <int SW, bool SP>
KMC_DEV bool kmc_window_place(u64* win, u64* wpred, const u64* e, u64 home, u64 lo, u64 hi) {
    if (home < lo || home >= hi) return false;
    for (u64 p = home - lo; p < hi - lo; ++p) {
        if (atomicCAS(&win[p * SW], 0ull, e[0]) == 0ull) {   // ds_cmpst_rtn_b64
            if constexpr (SW == 2) win[p * SW + 1] = e[1];
            if constexpr (SP) wpred[p] = e[SW];
            return true;
        }
    }
    return false;
}

// The entries a window turned away (`over`, whole waves call this): one atomicAdd per wave, then every lane writes its own record
template <int EW>
KMC_DEV void kmc_window_list(const KmcRehashArgs& a, bool over, const u64* e) {
    const u64 m = __ballot(over);
    if (!m) return;
    u64 at = 0;
    if (kmc_lane() == 0) at = atomicAdd(&a.ctl->listed.v, (u64)__popcll(m));
    at = kmc_bcast64(at, 0) + kmc_rank_in(m);
    if (over) {
        if (at < a.list_cap) {
#pragma unroll
            for (int k = 0; k < EW; ++k) a.list[at * EW + k] = e[k];
        } else {
            atomicOr(&a.ctl->err, KMC_REHASH_ERR_LIST_FULL);
        }
    }
}

// The whole window goes out, zeros included, 16 bytes per lane and 1 KiB per wave and store: every new slot is written
// exactly once, by the tile that owns it.  A lane zeroes what it has read: the window is clean for the next tile.
template <int SW, bool SP>
KMC_DEV void kmc_window_flush(const KmcRehashArgs& a, u64* win, u64* wpred, u64 lo, u64 nsl) {
    const u32 tid = threadIdx.x;
    {
        KmcSlot2R* const out = (KmcSlot2R*)(a.new_tab + lo * SW);
        KmcSlot2R* const src = (KmcSlot2R*)win;
        for (u64 j = tid; j < nsl * SW / 2; j += KMC_REHASH_BLOCK) {
            out[j] = src[j];
            src[j] = KmcSlot2R(0ull);
        }
    }
    if constexpr (SP) {
        KmcSlot2R* const out = (KmcSlot2R*)(a.new_pred + lo);
        KmcSlot2R* const src = (KmcSlot2R*)wpred;
        for (u64 j = tid; j < nsl / 2; j += KMC_REHASH_BLOCK) {
            out[j] = src[j];
            src[j] = KmcSlot2R(0ull);
        }
    }
}

template <int SW, bool SP>
KMC_DEV void kmc_rehash_window_body(const KmcRehashArgs& a, u64* lds) {
    constexpr int EW = SW + (SP ? 1 : 0);
    u64* const win = lds;                              // [win_slots][SW]
    u64* const wpred = lds + a.win_slots * SW;         // SP: [win_slots]
    const u32 tid = threadIdx.x;
    const u64 G = a.old_cap >> 6, G2 = a.new_cap >> 6;          // (both below 2^32: the products below fit 64 bits)
    const u64 tiles = (G + a.span - 1) / a.span;
    for (u64 j = tid; j < a.win_slots * EW; j += KMC_REHASH_BLOCK) lds[j] = 0ull;   // (afterwards a window is zeroed as it is written out)
    u32 placed = 0;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 g0 = t * a.span, g1 = g0 + a.span < G ? g0 + a.span : G;
        const u64 lo = (g0 * G2 / G) << 6, hi = (g1 * G2 / G) << 6;         // the window: new slots [lo, hi)
        const u64 nsl = hi - lo;
        if (nsl > a.win_slots) {                                             // (uniform over the block)
            if (tid == 0) atomicOr(&a.ctl->err, KMC_REHASH_ERR_WINDOW);
            continue;
        }
        __syncthreads();   // the window is zero: the start-up loop, or the write-out of this block's last tile
        for (u64 base = g0 << 6; base < g1 << 6; base += KMC_REHASH_BLOCK) {   // (tiles are whole groups: a wave is all in or all out)
            const u64 i = base + tid;
            u64 e[EW];
            bool over = false;
            if (i < g1 << 6 && kmc_rehash_load<SW, SP>(a, i, e)) {
                over = !kmc_window_place<SW, SP>(win, wpred, e, kmc_slot_of(e[0], a.new_cap), lo, hi);
                placed += over ? 0u : 1u;
            }
            kmc_window_list<EW>(a, over, e);
        }
        __syncthreads();
        kmc_window_flush<SW, SP>(a, win, wpred, lo, nsl);
    }
    placed = kmc_wave_sum(placed);
    if (placed && kmc_lane() == 0) atomicAdd(&a.ctl->placed_window, (u64)placed);
}

// Phase two, launched behind the windows on the same stream: one lane per listed entry.  Nothing else touches the table meanwhile.
template <int SW, bool SP>
KMC_DEV void kmc_rehash_overflow_body(const KmcRehashArgs& a) {
    constexpr int EW = SW + (SP ? 1 : 0);
    const u64 listed = a.ctl->listed.v;
    const u64 n = listed < a.list_cap ? listed : a.list_cap;
    u32 placed = 0;
    for (u64 i = (u64)blockIdx.x * KMC_REHASH_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * KMC_REHASH_BLOCK) {
        u64 e[EW];
#pragma unroll
        for (int k = 0; k < EW; ++k) e[k] = a.list[i * EW + k];
        placed += kmc_rehash_claim_global<SW, SP>(a, e) ? 1u : 0u;
    }
    placed = kmc_wave_sum(placed);
    if (placed && kmc_lane() == 0) atomicAdd(&a.ctl->placed_global, (u64)placed);
}

// The plain form: the new table (and predecessor table) cleared by the host, one lane per old slot.
template <int SW, bool SP>
KMC_DEV void kmc_rehash_scatter_body(const KmcRehashArgs& a) {
    constexpr int EW = SW + (SP ? 1 : 0);
    u32 placed = 0;
    for (u64 i = (u64)blockIdx.x * KMC_REHASH_BLOCK + threadIdx.x; i < a.old_cap; i += (u64)gridDim.x * KMC_REHASH_BLOCK) {
        u64 e[EW];
        if (kmc_rehash_load<SW, SP>(a, i, e)) placed += kmc_rehash_claim_global<SW, SP>(a, e) ? 1u : 0u;
    }
    placed = kmc_wave_sum(placed);
    if (placed && kmc_lane() == 0) atomicAdd(&a.ctl->placed_global, (u64)placed);
}

// One instantiation per entry shape: <slot words><n|p> (p: a predecessor table of its own).  1n 64-bit; 1p 64-bit with separate
// predecessors; 2n paired (fingerprint, predecessor) and wide (fingerprint, check word) alike; 2p wide with separate predecessors.
#define KMC_REHASH_INSTANTIATE(TAG, SW, SP)                                                                              \
    extern "C" __global__ __launch_bounds__(KMC_REHASH_BLOCK) void kmc_rehash_window_##TAG(KmcRehashArgs a) {            \
        extern __shared__ __attribute__((aligned(16))) u64 kmc_rehash_lds[];                                             \
        kmc_rehash_window_body<SW, SP>(a, kmc_rehash_lds);                                                               \
    }                                                                                                                    \
    extern "C" __global__ __launch_bounds__(KMC_REHASH_BLOCK) void kmc_rehash_overflow_##TAG(KmcRehashArgs a) {          \
        kmc_rehash_overflow_body<SW, SP>(a);                                                                             \
    }                                                                                                                    \
    extern "C" __global__ __launch_bounds__(KMC_REHASH_BLOCK) void kmc_rehash_scatter_##TAG(KmcRehashArgs a) {           \
        kmc_rehash_scatter_body<SW, SP>(a);                                                                              \
    }
#define KMC_REHASH_INSTANTIATE_ALL         \
    KMC_REHASH_INSTANTIATE(1n, 1, false)   \
    KMC_REHASH_INSTANTIATE(1p, 1, true)    \
    KMC_REHASH_INSTANTIATE(2n, 2, false)   \
    KMC_REHASH_INSTANTIATE(2p, 2, true)
#endif  // !KMC_HOST_EMU
