// kmc_compact.h — a seen-set taken down to its entries and built again at any size: the kernels behind the compact checkpoint
// (kmc_checkpoint_save_compact, include/kmc.h; the host side is kmc_ckpt_compact.cpp).  Part of the table code
// object, behind kmc_rehash.h whose entries, control block, window helpers and second phase it shares; model-independent.
//
// PACK reads a STRETCH of the table — the old groups [g_first, g_end), as many as the host's staging holds — and leaves
//   entries: the occupied slots as AoS entries (kmc_rehash.h), dense and in slot order;
//   index:   for every TILE of KMC_COMPACT_TILE groups the number of entries before it in the stretch, and one closing total.
// Three launches on one stream: kmc_pack_count (a workgroup per tile counts its occupied slots), kmc_pack_scan (ONE workgroup
// turns the stretch's counts into exclusive prefix sums) and kmc_pack_write (a second streaming read: a tile's entries go
// to index[tile] + rank, the rank from __ballot / mbcnt within a wave — a wave reads exactly one group — and through LDS
// across the four waves).  Order across workgroups costs a second read of the table and no waiting: no workgroup ever
// depends on the progress of another.  The table is not modified.
//
// UNPACK is kmc_rehash_window with another source.  kmc_slot_of is monotone in the key, so the entries of a run of old groups
// (whatever the size of the table they were packed from) have their homes in a run of new groups.  A stretch is cut into
// TILE-RUNS of `span` old groups, span a multiple of the tile; run t covers [g0, g1) = [g_first + t span, min(g0 + span, g_end)),
// reads entries[index[(g0 - g_first) / TILE] .. index[ceil((g1 - g_first) / TILE)]) and owns the new groups
// [floor(g0 G'/G), floor(g1 G'/G)): consecutive runs of consecutive stretches partition the new table exactly, for G' below G
// too.  What a window turns away goes to the overflow list; kmc_rehash_overflow places the list once every window of every
// stretch is written.  The destination is never cleared, every new slot is written once, nothing is probed at random.
#pragma once
#include "kmc_rehash.h"

#define KMC_COMPACT_TILE 8   // groups per index entry — a constant of the file format: 8 bytes of index per 512 slots

struct KmcCompactArgs {
    KmcRehashArgs r;       // pack: old_tab, old_pred, old_cap (the table that is read), ctl.  unpack: new_tab, new_pred, new_cap,
                           // old_cap (of the table the entries were packed from), span, win_slots, list, list_cap, ctl
    u64 g_first, g_end;    // the stretch: old groups [g_first, g_end), g_first a multiple of KMC_COMPACT_TILE
    u64* index;            // ceil((g_end - g_first) / KMC_COMPACT_TILE) + 1 words
    u64* entries;          // AoS entries of SLOT_WORDS + SEPARATE_PRED words
    u64 entries_cap;       // entries
};

#ifndef KMC_HOST_EMU
KMC_DEV u64 kmc_compact_tiles(const KmcCompactArgs& c) { return (c.g_end - c.g_first + KMC_COMPACT_TILE - 1) / KMC_COMPACT_TILE; }

// a stretch the table does not hold is a host bug: nothing of it is read (uniform over the grid)
KMC_DEV bool kmc_compact_stretch_ok(const KmcCompactArgs& c) {
    if (c.g_first <= c.g_end && c.g_end <= c.r.old_cap >> 6 && c.g_first % KMC_COMPACT_TILE == 0) return true;
    if (threadIdx.x == 0) atomicOr(&c.r.ctl->err, KMC_REHASH_ERR_WINDOW);
    return false;
}

// the sum of one value per wave over the workgroup, and (*below) over the waves before this one.  Two barriers: `lds` is free again.
KMC_DEV u32 kmc_block_ranks(u32 mine, u32* lds, u32* below) {
    const u32 wave = threadIdx.x >> 6;
    if (kmc_lane() == 0) lds[wave] = mine;
    __syncthreads();
    u32 all = 0;
    *below = 0;
#pragma unroll
    for (u32 w = 0; w < KMC_REHASH_BLOCK / 64; ++w) {
        const u32 v = lds[w];
        all += v;
        *below += w < wave ? v : 0u;
    }
    __syncthreads();
    return all;
}

template <int SW, bool SP>
KMC_DEV void kmc_pack_count_body(const KmcCompactArgs& c, u32* lds) {
    if (!kmc_compact_stretch_ok(c)) return;
    const u64 tiles = kmc_compact_tiles(c);
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 s0 = (c.g_first + t * KMC_COMPACT_TILE) << 6;
        const u64 s1 = s0 + KMC_COMPACT_TILE * 64 < c.g_end << 6 ? s0 + KMC_COMPACT_TILE * 64 : c.g_end << 6;
        u32 n = 0, below;
        for (u64 i = s0 + threadIdx.x; i < s1; i += KMC_REHASH_BLOCK) {
            u64 w0;
            if constexpr (SW == 2) w0 = __builtin_nontemporal_load((const KmcSlot2R*)(c.r.old_tab + 2 * i))[0];
            else w0 = __builtin_nontemporal_load(c.r.old_tab + i);
            n += w0 != 0ull ? 1u : 0u;
        }
        n = kmc_block_ranks(kmc_wave_sum(n), lds, &below);
        if (threadIdx.x == 0) c.index[t] = n;
    }
}

// ONE workgroup: the tiles' counts become the number of entries before each tile, index[tiles] the stretch's total
KMC_DEV void kmc_pack_scan_body(const KmcCompactArgs& c, u64* lds) {
    if (!kmc_compact_stretch_ok(c)) return;
    const u64 tiles = kmc_compact_tiles(c);
    const u64 per = (tiles + KMC_REHASH_BLOCK - 1) / KMC_REHASH_BLOCK;
    const u64 lo = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, hi = lo + per < tiles ? lo + per : tiles;
    u64 sum = 0;
    for (u64 i = lo; i < hi; ++i) sum += c.index[i];
    lds[threadIdx.x] = sum;
    __syncthreads();
    u64 run = 0;
    for (u32 k = 0; k < threadIdx.x; ++k) run += lds[k];
    for (u64 i = lo; i < hi; ++i) {
        const u64 v = c.index[i];
        c.index[i] = run;
        run += v;
    }
    if (threadIdx.x == KMC_REHASH_BLOCK - 1) {   // (the last lane's chunk ends the stretch, or is empty behind it)
        c.index[tiles] = run;
        if (run > c.entries_cap) atomicOr(&c.r.ctl->err, KMC_REHASH_ERR_LIST_FULL);
    }
}

template <int SW, bool SP>
KMC_DEV void kmc_pack_write_body(const KmcCompactArgs& c, u32* lds) {
    constexpr int EW = SW + (SP ? 1 : 0);
    if (!kmc_compact_stretch_ok(c)) return;
    const u64 tiles = kmc_compact_tiles(c);
    u32 packed = 0;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 s0 = (c.g_first + t * KMC_COMPACT_TILE) << 6;
        const u64 s1 = s0 + KMC_COMPACT_TILE * 64 < c.g_end << 6 ? s0 + KMC_COMPACT_TILE * 64 : c.g_end << 6;
        u64 at = c.index[t];
        for (u64 base = s0; base < s1; base += KMC_REHASH_BLOCK) {   // (a wave reads one whole group, or none of it)
            const u64 i = base + threadIdx.x;
            u64 e[EW];
            const bool have = i < s1 && kmc_rehash_load<SW, SP>(c.r, i, e);
            const u64 m = __ballot(have);
            u32 below;
            const u32 all = kmc_block_ranks((u32)__popcll(m), lds, &below);
            const u64 mine = at + below + kmc_rank_in(m);
            if (have && mine < c.entries_cap) {   // (past the capacity: kmc_pack_scan has raised the flag)
                if constexpr (EW == 2) {
                    KmcSlot2R v;
                    v[0] = e[0];
                    v[1] = e[1];
                    *(KmcSlot2R*)(c.entries + 2 * mine) = v;
                } else {
#pragma unroll
                    for (int k = 0; k < EW; ++k) c.entries[mine * EW + k] = e[k];
                }
                ++packed;
            }
            at += all;
        }
    }
    packed = kmc_wave_sum(packed);
    if (packed && kmc_lane() == 0) atomicAdd(&c.r.ctl->placed_global, (u64)packed);   // (the host's check against the closing total)
}

template <int SW, bool SP>
KMC_DEV void kmc_unpack_window_body(const KmcCompactArgs& c, u64* lds) {
    constexpr int EW = SW + (SP ? 1 : 0);
    const KmcRehashArgs& a = c.r;
    if (!kmc_compact_stretch_ok(c)) return;
    if (a.span == 0 || a.span % KMC_COMPACT_TILE) {    // (a run must begin where an index entry does)
        if (threadIdx.x == 0) atomicOr(&a.ctl->err, KMC_REHASH_ERR_WINDOW);
        return;
    }
    u64* const win = lds;                              // [win_slots][SW]
    u64* const wpred = lds + a.win_slots * SW;         // SP: [win_slots]
    const u32 tid = threadIdx.x;
    const u64 G = a.old_cap >> 6, G2 = a.new_cap >> 6;
    const u64 runs = (c.g_end - c.g_first + a.span - 1) / a.span;
    for (u64 j = tid; j < a.win_slots * EW; j += KMC_REHASH_BLOCK) lds[j] = 0ull;
    u32 placed = 0;
    for (u64 t = blockIdx.x; t < runs; t += gridDim.x) {
        const u64 g0 = c.g_first + t * a.span, g1 = g0 + a.span < c.g_end ? g0 + a.span : c.g_end;
        const u64 lo = (g0 * G2 / G) << 6, hi = (g1 * G2 / G) << 6;
        const u64 nsl = hi - lo;
        if (nsl > a.win_slots) {   // (uniform over the block)
            if (tid == 0) atomicOr(&a.ctl->err, KMC_REHASH_ERR_WINDOW);
            continue;
        }
        __syncthreads();   // the window is zero
        const u64 i0 = c.index[(g0 - c.g_first) / KMC_COMPACT_TILE];
        u64 i1 = c.index[(g1 - c.g_first + KMC_COMPACT_TILE - 1) / KMC_COMPACT_TILE];
        if (i1 > c.entries_cap) i1 = c.entries_cap;   // (the host has checked the index; an entry that is not there is never read)
        for (u64 base = i0; base < i1; base += KMC_REHASH_BLOCK) {
            const u64 i = base + tid;
            u64 e[EW];
            bool over = false;
            if (i < i1) {
                if constexpr (EW == 2) {
                    const KmcSlot2R v = __builtin_nontemporal_load((const KmcSlot2R*)(c.entries + 2 * i));
                    e[0] = v[0];
                    e[1] = v[1];
                } else {
#pragma unroll
                    for (int k = 0; k < EW; ++k) e[k] = __builtin_nontemporal_load(c.entries + i * EW + k);
                }
                if (e[0] != 0ull) {   // (no entry at all: it is not counted, and the host's conservation check refuses the file)
                    over = !kmc_window_place<SW, SP>(win, wpred, e, kmc_slot_of(e[0], a.new_cap), lo, hi);
                    placed += over ? 0u : 1u;
                }
            }
            kmc_window_list<EW>(a, over, e);
        }
        __syncthreads();
        kmc_window_flush<SW, SP>(a, win, wpred, lo, nsl);
    }
    placed = kmc_wave_sum(placed);
    if (placed && kmc_lane() == 0) atomicAdd(&a.ctl->placed_window, (u64)placed);
}

#define KMC_COMPACT_INSTANTIATE(TAG, SW, SP)                                                                             \
    extern "C" __global__ __launch_bounds__(KMC_REHASH_BLOCK) void kmc_pack_count_##TAG(KmcCompactArgs c) {              \
        __shared__ u32 ranks[KMC_REHASH_BLOCK / 64];                                                                     \
        kmc_pack_count_body<SW, SP>(c, ranks);                                                                           \
    }                                                                                                                    \
    extern "C" __global__ __launch_bounds__(KMC_REHASH_BLOCK) void kmc_pack_write_##TAG(KmcCompactArgs c) {              \
        __shared__ u32 ranks[KMC_REHASH_BLOCK / 64];                                                                     \
        kmc_pack_write_body<SW, SP>(c, ranks);                                                                           \
    }                                                                                                                    \
    extern "C" __global__ __launch_bounds__(KMC_REHASH_BLOCK) void kmc_unpack_window_##TAG(KmcCompactArgs c) {           \
        extern __shared__ __attribute__((aligned(16))) u64 kmc_unpack_lds[];                                             \
        kmc_unpack_window_body<SW, SP>(c, kmc_unpack_lds);                                                               \
    }
#define KMC_COMPACT_INSTANTIATE_ALL                                                                                      \
    extern "C" __global__ __launch_bounds__(KMC_REHASH_BLOCK) void kmc_pack_scan(KmcCompactArgs c) {                     \
        __shared__ u64 sums[KMC_REHASH_BLOCK];                                                                           \
        kmc_pack_scan_body(c, sums);                                                                                     \
    }                                                                                                                    \
    KMC_COMPACT_INSTANTIATE(1n, 1, false)                                                                                \
    KMC_COMPACT_INSTANTIATE(1p, 1, true)                                                                                 \
    KMC_COMPACT_INSTANTIATE(2n, 2, false)                                                                                \
    KMC_COMPACT_INSTANTIATE(2p, 2, true)
#endif  // !KMC_HOST_EMU
