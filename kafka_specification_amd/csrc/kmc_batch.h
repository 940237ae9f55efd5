// kmc_batch.h — batched successor and invariant evaluation for states given as data: N packed states in, a CSR of their
// successor records out (kmc_successors_batch), over the same extract / inst<I> / apply<K> / violated_pre templates the search uses.
// Part of the device source (kmc_device.h lists the parts; the host engine hands their concatenation to hiprtc).
//
// Three kernels, a code object of their own (KMC_CODEOBJ_BATCH), no atomics, no control block — DESIGN.md 8d holds the contract:
//   k_batch_count  one lane per state: invariants, every guard of Next (KmcSim<M>::count), the number of records of the state
//                  and its "enabled instances" bitset into a scratch plane;
//   k_batch_scan   exclusive 64-bit prefix sum of the counts -> offsets[0..n] (a block-sums pass, then the scan);
//   k_batch_emit   one lane per state: every enabled instance's successor, fingerprint and kind, in INSTANCE order (action
//                  kinds in the module's order, bindings ascending, the two records of a doubly-enabled binding adjacent —
//                  k_simulate's numbering: record r is the candidate kmc_sim_draw(...) = r takes), written at
//                  offsets[i] + (records of the state before the instance) as W + 2 words: state, fingerprint, kind.
// What goes through LDS: the input is AoS ([n][W] words as the host hands it over), so a wave reads its 64 states as W whole
// 512-byte lines and turns them into one state per lane through its LDS rows; a leaf's records leave the other way round — every
// lane puts its record into the wave's LDS rows, then the lanes walk the WORDS of those rows together, consecutive lanes storing
// consecutive words of one record, so that a record (and its repeat, and a neighbour state's adjacent run) leaves in full lines.
#pragma once
#include "kmc_common.h"

#define KMC_CODEOBJ_BATCH 4u                 // the code object that holds the three kernels (KMC_ONLY_MODE)
#define KMC_BATCH_MAX_STATES (1u << 22)      // states of one launch, at the most
#define KMC_BATCH_SCAN_CHUNK 16384u          // counts one block of k_batch_scan covers: at most KMC_BATCH_MAX_STATES / this = 256 block sums
#define KMC_BATCH_TWO (1ull << 63)           // in a staged record's destination: the record is written twice

struct KmcBatchArgs {
    const u64* in;     // [n][W] packed states, AoS
    u32* count;        // [n] records per state
    u32* bits;         // nh planes of `stride` words: bit i of plane h, column c = instance 32 h + i of state c is enabled
    u64* offsets;      // [n + 1]
    u64* sums;         // k_batch_scan: one sum per block (at most 256)
    u64* rec;          // [cap][W + 2] records, AoS
    u32* violated;     // [n] KMC_INV_* bits
    u64 stride;
    u64 cap;           // k_batch_emit: records at or beyond it are not written (the host passes the end of a state's run)
    u64 seed;          // of the fingerprint
    u32 n;
    u32 inv_mask;
    u32 nh;            // planes the host allocated: (instances + 31) / 32
    u32 phase;         // k_batch_scan: 0 block sums, 1 the scan
};

#ifndef KMC_HOST_EMU
// The lanes of a wave hand data to each other through LDS rows of their own: what was stored is visible to every lane after this.
KMC_DEV void kmc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int W> struct KmcBatchTile {
    static constexpr int RW = W + 2;          // words of a record
    static constexpr int WP = W | 1;          // an input row in LDS: odd, so that 64 lanes reading a row each hit distinct banks
    static constexpr int RWP = RW | 1;        // ... and a staged record's
    static constexpr int ROWS = 64 * RWP;     // words of a wave's rows (an input tile, 64 * WP, fits)
    static constexpr int WORDS = ROWS + 64;   // ... and the 64 destinations of a leaf's records
    // 64 states of the AoS input -> one per lane.  `valid` (1..64) states exist; a lane beyond them holds the last one's words.
    static KMC_DEV void load(const u64* in, u64 tile, u32 valid, u64* rows, u32 lane, u64* s) {
        const u64* src = in + tile * 64ull * (u64)W;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const u32 idx = (u32)j * 64u + lane;   // word idx of the tile: state idx / W, word idx % W
            const u32 st = idx / (u32)W;
            if (st < valid) rows[st * WP + (idx - st * (u32)W)] = KMC_FRONTIER_LOAD(&src[idx]);
        }
        kmc_wave_sync();
        const u32 row = lane < valid ? lane : valid - 1u;
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = rows[row * WP + k];
        kmc_wave_sync();
    }
};

// k_batch_count.  Tiles of 64 states dealt to the grid's waves round-robin, as k_simulate deals its walkers.
template <class M> KMC_DEV void kmc_batch_count_body(const KmcBatchArgs& a) {
    constexpr int W = M::W;
    using S = KmcSim<M>;
    using T = KmcBatchTile<W>;
    __shared__ u64 lds[KMC_WAVES][64 * T::WP];
    const u32 lane = kmc_lane();
    const u32 wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 nwaves = gridDim.x * KMC_WAVES;
    const u32 ntiles = (a.n + 63u) >> 6;
#pragma clang loop unroll(disable)
    for (u32 tile = blockIdx.x * KMC_WAVES + wib; tile < ntiles; tile += nwaves) {
        const u32 valid = kmc_min(64u, a.n - tile * 64u);
        const bool alive = lane < valid;
        const u64 i = (u64)tile * 64ull + lane;
        u64 s[W];
        T::load(a.in, tile, valid, lds[wib], lane, s);
        const typename M::Pre pre = M::extract(s);
        const u32 bad = a.inv_mask ? M::violated_pre(pre, a.inv_mask) : 0u;
        typename S::Cand c;
        const u32 n = S::count(pre, s, alive ? 1u : 0u, c);
        if (alive) {
            a.violated[i] = bad;
            a.count[i] = n;
#pragma unroll
            for (int h = 0; h < S::NH; ++h)
                if ((u32)h < a.nh) a.bits[(u64)h * a.stride + i] = c.en[h];
        }
    }
}

// k_batch_scan.  Block b covers the counts [b CHUNK, (b + 1) CHUNK): phase 0 leaves their sum in sums[b]; phase 1 takes the sum of
// the blocks before it as its carry and scans its chunk in rounds of one block's width (a wave scan, the waves' totals through LDS).
KMC_DEV u32 kmc_wave_scan_incl(u32 x, u32 lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 y = (u32)__shfl_up((int)x, off);
        x += lane >= (u32)off ? y : 0u;
    }
    KMC_OPAQUE(x);
    return x;
}
KMC_DEV u64 kmc_wave_sum64(u64 x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)x, off), hi = (u32)__shfl_xor((int)(u32)(x >> 32), off);
        x += ((u64)hi << 32) | lo;
    }
    KMC_OPAQUE(x);
    return x;
}
KMC_DEV void kmc_batch_scan_body(const KmcBatchArgs& a) {
    __shared__ u64 wtot[KMC_WAVES];
    const u32 lane = kmc_lane();
    const u32 wib = threadIdx.x >> 6;
    const u64 lo = (u64)blockIdx.x * KMC_BATCH_SCAN_CHUNK;
    const u64 hi = lo + KMC_BATCH_SCAN_CHUNK < (u64)a.n ? lo + KMC_BATCH_SCAN_CHUNK : (u64)a.n;
    // the block's sum of x (phase 0), or of the block sums before this block (phase 1: at most 256 of them, one per thread)
    u64 mine = 0;
    if (a.phase == 0) {
        for (u64 j = lo + threadIdx.x; j < hi; j += KMC_BLOCK) mine += (u64)a.count[j];
    } else {
        mine = threadIdx.x < blockIdx.x ? a.sums[threadIdx.x] : 0ull;
    }
    const u64 wsum = kmc_wave_sum64(mine);
    if (lane == 0) wtot[wib] = wsum;
    __syncthreads();
    u64 carry = 0;
#pragma unroll
    for (int w = 0; w < KMC_WAVES; ++w) carry += wtot[w];
    __syncthreads();
    if (a.phase == 0) {
        if (threadIdx.x == 0) a.sums[blockIdx.x] = carry;
        return;
    }
    for (u64 base = lo; base < hi; base += KMC_BLOCK) {   // (block-uniform bounds: every thread takes every round)
        const u64 j = base + threadIdx.x;
        const u32 x = j < hi ? a.count[j] : 0u;
        const u32 incl = kmc_wave_scan_incl(x, lane);
        if (lane == 63) wtot[wib] = (u64)incl;
        __syncthreads();
        u64 before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < KMC_WAVES; ++w) {
            before += (u32)w < wib ? wtot[w] : 0ull;
            total += wtot[w];
        }
        if (j < hi) a.offsets[j] = carry + before + (u64)(incl - x);
        carry += total;
        __syncthreads();
    }
    if (hi == (u64)a.n && threadIdx.x == 0) a.offsets[a.n] = carry;
}

// k_batch_emit.  The state and its bitset in registers; the walk over the segments (replica-major layouts: apply<K>, binding
// per lane, every lane taking ITS next enabled binding of the segment until no lane has one left) or the instances (elsewhere:
// inst<I>); a leaf runs when some lane holds it.  `pos` runs along the state's records: instance order by construction.
template <class M> KMC_DEV void kmc_batch_emit_body(const KmcBatchArgs& a) {
    constexpr int W = M::W;
    using S = KmcSim<M>;
    using T = KmcBatchTile<W>;
    constexpr int RW = T::RW, RWP = T::RWP;
    __shared__ u64 lds[KMC_WAVES][T::WORDS];
    const u32 lane = kmc_lane();
    const u32 wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 nwaves = gridDim.x * KMC_WAVES;
    const u32 ntiles = (a.n + 63u) >> 6;
    u64* const rows = lds[wib];
    u64* const dst = rows + T::ROWS;
#pragma clang loop unroll(disable)
    for (u32 tile = blockIdx.x * KMC_WAVES + wib; tile < ntiles; tile += nwaves) {
        const u32 valid = kmc_min(64u, a.n - tile * 64u);
        const bool alive = lane < valid;
        const u64 i = (u64)tile * 64ull + (alive ? lane : valid - 1u);
        u64 s[W];
        T::load(a.in, tile, valid, rows, lane, s);
        const typename M::Pre pre = M::extract(s);
        u32 en[S::NH];
#pragma unroll
        for (int h = 0; h < S::NH; ++h) en[h] = (alive && (u32)h < a.nh) ? a.bits[(u64)h * a.stride + i] : 0u;
        u64 pos = a.offsets[i];
        // one leaf's records leave: lanes with `mine` (the set m) hold successor t of kind `kind`, `extra`: it counts twice
        auto put = [&](bool mine, u64 m, const u64* t, int kind, u32 extra) {
            const u32 q = kmc_rank_in(m);
            if (mine) {
#pragma unroll
                for (int k = 0; k < W; ++k) rows[q * RWP + k] = t[k];
                rows[q * RWP + W] = KmcSink<M>::fingerprint_of(t, a.seed);
                rows[q * RWP + W + 1] = (u64)(u32)kind;
                dst[q] = pos | (extra ? KMC_BATCH_TWO : 0ull);
                pos += extra ? 2ull : 1ull;
            }
            kmc_wave_sync();
            const u32 words = (u32)__popcll(m) * (u32)RW;
            for (u32 w = lane; w < words; w += 64u) {
                const u32 r = w / (u32)RW, k = w - r * (u32)RW;
                const u64 d = dst[r] & ~KMC_BATCH_TWO;
                const u64 v = rows[r * RWP + k];
                if (d < a.cap) a.rec[d * RW + k] = v;
                if ((dst[r] & KMC_BATCH_TWO) && d + 1 < a.cap) a.rec[(d + 1) * RW + k] = v;
            }
            kmc_wave_sync();
        };
        if constexpr (M::KIND_MAJOR) {
            kmc_static_for<0, M::NSEGS>([&](auto SS) {
                constexpr int sg = decltype(SS)::value;
                constexpr int K = M::seg_kind(sg);
                auto left = M::template seg_bits<sg>(en);   // this lane's enabled bindings of the segment, from its first one
#pragma clang loop unroll(disable)
                for (;;) {
                    const bool mine = left != 0;
                    const u64 m = __ballot(mine);
                    if (!m) break;
                    const u32 b = (u32)M::seg_first(sg) + (mine ? (u32)__builtin_ctzll((u64)left) : 0u);
                    left &= left - 1;
                    u32 extra = 0;
                    u64 t[W];
                    M::template apply<K>(pre, s, t, b, extra);
                    put(mine, m, t, K, extra);
                }
            });
        } else {
            kmc_static_for<0, M::NINST>([&](auto I) {
                constexpr int ii = decltype(I)::value;
                const bool mine = (en[ii >> 5] >> (ii & 31)) & 1u;
                const u64 m = __ballot(mine);
                if (m) {
                    int kind = 0;
                    u32 extra = 0;
                    u64 t[W];
                    (void)M::template inst<ii>(pre, s, t, kind, extra);
                    put(mine, m, t, kind, extra);
                }
            });
        }
    }
}

#if KMC_ONLY_MODE == 4
#define KMC_INSTANTIATE(NAME, ...)                                                                     \
    extern "C" __global__ __launch_bounds__(KMC_BLOCK) void kmc_batch_count_##NAME(KmcBatchArgs a) {   \
        kmc_batch_count_body<__VA_ARGS__>(a);                                                          \
    }                                                                                                  \
    extern "C" __global__ __launch_bounds__(KMC_BLOCK) void kmc_batch_scan_##NAME(KmcBatchArgs a) {    \
        kmc_batch_scan_body(a);                                                                        \
    }                                                                                                  \
    extern "C" __global__ __launch_bounds__(KMC_BLOCK) void kmc_batch_emit_##NAME(KmcBatchArgs a) {    \
        kmc_batch_emit_body<__VA_ARGS__>(a);                                                           \
    }
#endif
#endif  // !KMC_HOST_EMU
