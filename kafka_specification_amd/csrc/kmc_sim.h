// kmc_sim.h — random simulation: batched random walks over the same guard / apply / violated_pre templates the search uses.
// Part of the device source (kmc_device.h lists the parts; the host engine hands their concatenation to hiprtc).
//
// A walk is a pure function of (model constants, seed, walk index w) — DESIGN.md "Random simulation" holds the contract:
//   state 0 is Init; at step t the walk stands on s_t, whose candidates are TLC's enumeration of Next on s_t (one record per
//   satisfying binding and disjunct: what kmc_successors lists), n_t of them, here in INSTANCE order (action kinds in the
//   module's order, bindings ascending; an instance whose two disjuncts both hold — Kip279.tla:47-51, Kip320.tla:82-83 — holds
//   two consecutive records); r_t = kmc_sim_draw(seed, w, t, n_t) picks record r_t.  Every state is checked against the
//   invariants; the walk ends at its first violating state, at a state without candidates, or after `depth` states (the last
//   of those is checked, not expanded).
// Two layers: a LANE-LOCAL one (the draw, counting the candidates of a state, locating the r-th, its effect: plain integer
// code that g++ compiles too — tests/sim_emu.cpp) and the WAVE one (k_simulate: one lane per walker, state in registers; and
// k_simulate_from: walks from start states given as data, a lane refilled with the next walker when its own has ended).
#pragma once
#include "kmc_common.h"

#define KMC_CODEOBJ_SIM 3u         // the code object that holds k_simulate (KMC_ONLY_MODE; the search's modes are 0..2)
#define KMC_SIM_FLAG_RECORD 1u     // every walker stores every state it stands on
#define KMC_SIM_FLAG_DEADLOCK 2u   // CHECK_DEADLOCK: a state without candidates is a verdict, not just the walk's end
#define KMC_SIM_DEADLOCK_BIT 16u   // in a witness word: the walk ended in a checked deadlock (bits 0..3: the invariants violated)
#define KMC_SIM_NO_WITNESS (~0ull)
#define KMC_SIM_MAX_DEPTH (1u << 20)

// ---- the draw: a counter-based generator, no state, no library -------------------------------------------------------
// key = mix(mix(seed + G) + w * C); h_t = mix(key + (t + 1) * G) (the splitmix64 stream of the key: distinct t, distinct
// inputs of a bijection); r_t = the high 64 bits of h_t * n — multiply-high, no division, bias below n / 2^64.
KMC_HD inline u64 kmc_sim_key(u64 seed, u64 walk) {
    return kmc_mix64(kmc_mix64(seed + 0x9E3779B97F4A7C15ull) + walk * 0xD1342543DE82EF95ull);
}
KMC_HD inline u64 kmc_sim_draw_key(u64 key, u32 step, u32 n) {
    const u64 h = kmc_mix64(key + ((u64)step + 1ull) * 0x9E3779B97F4A7C15ull);
    return (u64)(((unsigned __int128)h * (unsigned __int128)n) >> 64);
}
KMC_HD inline u64 kmc_sim_draw_of(u64 seed, u64 walk, u32 step, u32 n) { return kmc_sim_draw_key(kmc_sim_key(seed, walk), step, n); }

// how a recorded state was reached: action kind + 1 (0: Init) | the record chosen << 16 | the candidates it was chosen among << 40
KMC_HD inline u64 kmc_sim_meta(int kind, u32 r, u32 n) { return (u64)(u32)(kind + 1) | ((u64)r << 16) | ((u64)n << 40); }

// ---- the lane-local layer --------------------------------------------------------------------------------------------
template <class M> struct KmcSim {
    static constexpr int W = M::W;
    static constexpr int NH = (M::NINST + 31) / 32;   // 32-bit words of a per-walker bitset over the action instances
    // The candidates of one state: the enabled instances, and those of them that hold a second record (both disjuncts of one
    // binding: `extra`, never more than one further record in these modules).
    struct Cand {
        u32 en[NH];
        u32 ex[M::HAS_EXTRA ? NH : 1];
    };
    // Every guard of Next in one straight-line block (inst<I> with its effect dead, as k_expand's pass 1; the bindings of
    // EXTRA_KIND keep what their multiplicity reads).  -> n, the number of records.
    static KMC_DEV u32 count(const typename M::Pre& pre, const u64* s, u32 alive01, Cand& c) {
#pragma unroll
        for (int h = 0; h < NH; ++h) c.en[h] = 0;
#pragma unroll
        for (int h = 0; h < (M::HAS_EXTRA ? NH : 1); ++h) c.ex[h] = 0;
        kmc_static_for<0, M::NINST>([&](auto I) {
            constexpr int i = decltype(I)::value;
            u64 tt[W];
            int kd;
            u32 ex;
            const u32 g01 = M::template inst<i>(pre, s, tt, kd, ex) & alive01;
            c.en[i >> 5] |= g01 << (i & 31);
            kmc_launder(c.en[i >> 5]);  // (keeps the OR chain sequential: kmc_expand_body)
            if constexpr (M::HAS_EXTRA) c.ex[i >> 5] |= (ex ? g01 : 0u) << (i & 31);
        });
        u32 n = 0;
#pragma unroll
        for (int h = 0; h < NH; ++h) n += (u32)__builtin_popcount(c.en[h]);
        if constexpr (M::HAS_EXTRA) {
#pragma unroll
            for (int h = 0; h < NH; ++h) n += (u32)__builtin_popcount(c.ex[h]);
        }
        return n;
    }
    // The instance that holds record r (r < n): the word by a running sum (a select chain, no indexed array), the bit by a
    // five-step bisection on "records below bit lo".
    static KMC_DEV u32 locate(const Cand& c, u32 r) {
        u32 e = 0, x = 0, rr = 0, hsel = 0, base = 0;
        bool done = false;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const u32 xh = M::HAS_EXTRA ? c.ex[M::HAS_EXTRA ? h : 0] : 0u;
            const u32 cnt = (u32)__builtin_popcount(c.en[h]) + (u32)__builtin_popcount(xh);
            const bool here = !done && r < base + cnt;
            e = here ? c.en[h] : e;
            x = here ? xh : x;
            rr = here ? r - base : rr;
            hsel = here ? (u32)h : hsel;
            done = done || here;
            base += cnt;
        }
        u32 lo = 0;   // the largest bit with at most rr records below it: that bit is set, and holds record rr
#pragma unroll
        for (u32 st = 16; st; st >>= 1) {
            const u32 m = (1u << (lo + st)) - 1u;
            const u32 below = (u32)__builtin_popcount(e & m) + (u32)__builtin_popcount(x & m);
            lo += below <= rr ? st : 0u;
        }
        return hsel * 32u + lo;
    }
    // The effect of instance ci on s -> t and its action kind, the way k_simulate's leaves apply it: apply<K> on the
    // replica-major layouts, inst<I> elsewhere.  (One walker at a time: the host emulation's step.)
    static KMC_DEV void effect(const typename M::Pre& pre, const u64* s, u32 ci, u64* t, int& kind) {
        if constexpr (M::KIND_MAJOR) {
            kmc_static_for<0, M::NSEGS>([&](auto SS) {
                constexpr int sg = decltype(SS)::value;
                constexpr int K = M::seg_kind(sg);
                constexpr u32 lo = (u32)(M::kind_base(K) + M::seg_first(sg)), cnt = (u32)M::seg_count(sg);
                if (ci - lo < cnt) {
                    u32 extra = 0;
                    M::template apply<K>(pre, s, t, ci - (u32)M::kind_base(K), extra);
                    kind = K;
                }
            });
        } else {
            kmc_dispatch<0, M::NINST>((int)ci, [&](auto I) {
                u32 extra = 0;
                (void)M::template inst<decltype(I)::value>(pre, s, t, kind, extra);
            });
        }
    }
};

// ---- the wave layer --------------------------------------------------------------------------------------------------
// One launch's control block: the host zeroes it (witness: all ones) before the launch and reads it back after.
struct alignas(128) KmcSimCtl {
    u64 taken[KMC_MAX_KINDS];   // steps taken per action kind
    u64 viol_count[4];          // walks that ended on a state violating invariant k
    u64 witness;                // min over the walks that ended in a verdict of (walker of the launch << 32 | step << 8 | bits)
    u64 states;                 // states stood on, Init included
    u64 ended_early;            // walks that ended on a state without candidates
    u64 longest;                // states of the longest walk
};
struct KmcSimArgs {
    KmcSimCtl* ctl;
    u64* rec;          // RECORD: planes [step][word][column] of rec_stride columns; word W is kmc_sim_meta of the state
    u64* rec_len;      // RECORD: states of the walk, per column
    u64 rec_stride;
    u64 rec_col0;      // the column of this launch's walker 0
    u64 seed;
    u64 first_walk;    // the walk index of this launch's walker 0
    u32 n;             // walkers of this launch
    u32 depth;         // states per walk, at the most
    u32 inv_mask;
    u32 flags;         // KMC_SIM_FLAG_*
};

// k_simulate_from's launch: k_simulate's, and the start states.  (A struct of its own: k_simulate's kernarg layout stays as it is.)
#define KMC_SIM_CHUNK 256u         // consecutive walkers of a launch that one wave walks, one after the other through its 64 lanes
#ifndef KMC_SIM_REFILL_MIN
#define KMC_SIM_REFILL_MIN 1       // free lanes at which a wave hands out new walkers (1..64; 64: idle until all 64 are done, as k_simulate).
                                   // 1: the fastest of 1 / 16 / 64 on walks from a frontier, DESIGN.md 8a (profiles/simulate_from.json)
#endif
struct KmcSimFromArgs {
    KmcSimCtl* ctl;
    u64* rec;
    u64* rec_len;
    u64 rec_stride;
    u64 rec_col0;
    u64 seed;
    u64 first_walk;
    const u64* starts;   // [n_starts][W] packed states, AoS: walker i of the launch starts on row (row0 + i) mod n_starts
    u32 n_starts;
    u32 row0;            // first_walk mod n_starts
    u32 n;
    u32 depth;
    u32 inv_mask;
    u32 flags;
};

#ifndef KMC_HOST_EMU
KMC_DEV u32 kmc_wave_max(u32 x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u32 y = (u32)__shfl_xor((int)x, off);
        x = y > x ? y : x;
    }
    KMC_OPAQUE(x);
    return x;
}

// k_simulate.  One lane per walker, its W state words in registers from Init to its end; tiles of 64 walkers dealt to the
// grid's waves round-robin (as k_expand deals frontier tiles); the step loop is wave-uniform and a finished lane idles until
// its tile is done.  Per step: extract, [record], invariants, count (KmcSim::count: the bitset design — DESIGN.md has the
// numbers it was chosen on), draw, locate, and the chosen instance's effect in a walk over the segments (replica-major
// layouts: KmcKafka::apply<K>, binding per lane) or the instances (elsewhere: inst<I>) in which a leaf runs only when some lane
// chose it.  No table, no frontier, no LDS; the control block receives a wave's counters once, at its end.
template <class M> KMC_DEV void kmc_simulate_body(const KmcSimArgs& a) {
    constexpr int W = M::W;
    using S = KmcSim<M>;
    const u32 lane = kmc_lane();
    const u32 wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 nwaves = gridDim.x * KMC_WAVES;
    const u32 wave0 = blockIdx.x * KMC_WAVES + wib;
    const u32 ntiles = (a.n + 63u) >> 6;
    const bool record = (a.flags & KMC_SIM_FLAG_RECORD) != 0;
    u64 taken_lane = 0;          // lane k: steps of action kind k
    u64 states = 0, early = 0;   // wave-uniform
    u32 longest = 0;             // per lane
#pragma clang loop unroll(disable)
    for (u32 tile = wave0; tile < ntiles; tile += nwaves) {
        const u32 rel = tile * 64u + lane;
        bool alive = rel < a.n;
        const u64 key = kmc_sim_key(a.seed, a.first_walk + rel);
        const u64 col = a.rec_col0 + rel;
        u64 s[W];
        M::init(s);
        u64 meta = 0;
        u32 len = 0;
#pragma clang loop unroll(disable)
        for (u32 t = 0;; ++t) {
            const typename M::Pre pre = M::extract(s);
            if (record && alive) {
#pragma unroll
                for (int k = 0; k < W; ++k) a.rec[((u64)t * (W + 1) + k) * a.rec_stride + col] = s[k];
                a.rec[((u64)t * (W + 1) + W) * a.rec_stride + col] = meta;
            }
            len = alive ? t + 1u : len;
            const u32 bad = (alive && a.inv_mask) ? M::violated_pre(pre, a.inv_mask) : 0u;
            if (__ballot(bad != 0)) {
                if (bad) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (bad >> k & 1u) atomicAdd(&a.ctl->viol_count[k], 1ull);
                    atomicMin(&a.ctl->witness, ((u64)rel << 32) | ((u64)t << 8) | (u64)(bad & 15u));
                }
                alive = alive && bad == 0;
            }
            if (t + 1u >= a.depth) break;
            if (__ballot(alive) == 0) break;
            typename S::Cand c;
            const u32 n = S::count(pre, s, alive ? 1u : 0u, c);
            const bool stuck = alive && n == 0;
            const u64 sm = __ballot(stuck);
            if (sm) {
                early += (u64)__popcll(sm);
                if (stuck && (a.flags & KMC_SIM_FLAG_DEADLOCK))
                    atomicMin(&a.ctl->witness, ((u64)rel << 32) | ((u64)t << 8) | (u64)KMC_SIM_DEADLOCK_BIT);
                alive = alive && !stuck;
            }
            const u32 r = alive ? (u32)kmc_sim_draw_key(key, t, n) : 0u;
            const u32 ci = alive ? S::locate(c, r) : (u32)M::NINST;   // (NINST: no leaf is this lane's)
            u64 nx[W];
#pragma unroll
            for (int k = 0; k < W; ++k) nx[k] = s[k];
            int kind = 0;
            if constexpr (M::KIND_MAJOR) {
                kmc_static_for<0, M::NSEGS>([&](auto SS) {
                    constexpr int sg = decltype(SS)::value;
                    constexpr int K = M::seg_kind(sg);
                    constexpr u32 lo = (u32)(M::kind_base(K) + M::seg_first(sg)), cnt = (u32)M::seg_count(sg);
                    const bool mine = ci - lo < cnt;
                    const u64 m = __ballot(mine);
                    if (m) {
                        const u32 b = mine ? ci - (u32)M::kind_base(K) : (u32)M::seg_first(sg);
                        u32 extra = 0;
                        u64 tt[W];
                        M::template apply<K>(pre, s, tt, b, extra);
#pragma unroll
                        for (int k = 0; k < W; ++k) nx[k] = mine ? tt[k] : nx[k];
                        kind = mine ? K : kind;
                        taken_lane += lane == (u32)K ? (u64)__popcll(m) : 0ull;
                    }
                });
            } else {
                kmc_static_for<0, M::NINST>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    const bool mine = ci == (u32)i;
                    const u64 m = __ballot(mine);
                    if (m) {
                        int kd = 0;
                        u32 extra = 0;
                        u64 tt[W];
                        (void)M::template inst<i>(pre, s, tt, kd, extra);
#pragma unroll
                        for (int k = 0; k < W; ++k) nx[k] = mine ? tt[k] : nx[k];
                        kind = mine ? kd : kind;
                        taken_lane += lane == (u32)kd ? (u64)__popcll(m) : 0ull;
                    }
                });
            }
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] = nx[k];
            meta = kmc_sim_meta(kind, r, n);
        }
        if (record && rel < a.n) a.rec_len[col] = (u64)len;
        states += (u64)kmc_wave_sum(len);   // (a tile's sum: at most 64 * KMC_SIM_MAX_DEPTH)
        longest = len > longest ? len : longest;
    }
    const u32 lmax = kmc_wave_max(longest);
    if (lane < (u32)M::NKINDS && taken_lane) atomicAdd(&a.ctl->taken[lane], taken_lane);
    if (lane == 0) {
        if (states) atomicAdd(&a.ctl->states, states);
        if (early) atomicAdd(&a.ctl->ended_early, early);
        if (lmax) atomicMax(&a.ctl->longest, (u64)lmax);
    }
}

template <int W> struct KmcBatchTile;   // kmc_batch.h: 64 rows of an AoS input -> one per lane, through the wave's LDS rows
KMC_DEV u64 kmc_wave_sum64(u64 x);      // kmc_batch.h

// k_simulate_from.  Walks from start states given as data: walker i of the launch starts on starts[(first_walk + i) mod n_starts]
// with t = 0 there; everything else is k_simulate's walk.  The work split is its own.  Walks that start deep in a bounded model
// end after few and unevenly many states, so a lane does not wait for its tile: the launch is cut into chunks of KMC_SIM_CHUNK
// consecutive walkers, wave v owns chunks v, v + nwaves, ... and sees them end to end as ONE sequence of `total` walkers behind
// the wave-uniform `cursor`; a lane holds one walker with ITS OWN step counter, key and index.  At the top of every step the
// wave ballots its free lanes; at KMC_SIM_REFILL_MIN of them (or when none is alive) free lane j takes walker cursor +
// rank(j) of the sequence, loads its start state and restarts at t = 0.  A fill of all 64 lanes whose walkers are 64
// consecutive rows of `starts` goes through LDS (KmcBatchTile::load: whole lines in, one state per lane out); a refill of a
// few lanes loads its rows directly.  The guard block, the draw and the effect walk are k_simulate's, with per-lane t.
// Counters: taken per kind by ballot popcount; states / longest per lane as a walk ends, ended_early by popcount, all sent to
// the control block once, at the wave's end.
template <class M> KMC_DEV void kmc_simulate_from_body(const KmcSimFromArgs& a) {
    static_assert(KMC_SIM_REFILL_MIN >= 1 && KMC_SIM_REFILL_MIN <= 64, "KMC_SIM_REFILL_MIN: 1..64 lanes");
    constexpr int W = M::W;
    using S = KmcSim<M>;
    using T = KmcBatchTile<W>;
    __shared__ u64 lds[KMC_WAVES][64 * T::WP];
    const u32 lane = kmc_lane();
    const u32 wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 nwaves = gridDim.x * KMC_WAVES;
    const u32 wave0 = blockIdx.x * KMC_WAVES + wib;
    const u32 nchunks = (a.n + KMC_SIM_CHUNK - 1u) / KMC_SIM_CHUNK;
    const bool record = (a.flags & KMC_SIM_FLAG_RECORD) != 0;
    // the wave's sequence: walker q of it is walker (wave0 + q / CHUNK * nwaves) * CHUNK + q % CHUNK of the launch
    u32 total = 0;
    if (wave0 < nchunks) {
        total = (nchunks - wave0 + nwaves - 1u) / nwaves * KMC_SIM_CHUNK;
        if ((nchunks - 1u - wave0) % nwaves == 0) total -= nchunks * KMC_SIM_CHUNK - a.n;   // (the launch's last chunk is this wave's)
    }
    u32 cursor = 0;              // wave-uniform: walkers of the sequence handed out
    u64 taken_lane = 0;          // lane k: steps of action kind k
    u64 early = 0;               // wave-uniform
    u64 states = 0;              // per lane, as `longest`
    u32 longest = 0;
    bool alive = false;
    u32 rel = 0, t = 0;          // this lane's walker: its index in the launch, the step it stands on
    u64 key = 0, meta = 0;
    u64 s[W];
    M::init(s);                  // (a lane that never gets a walker runs the leaves' code on a real state)
#pragma clang loop unroll(disable)
    for (;;) {
        const u64 fm = __ballot(!alive);
        const u32 nfree = (u32)__popcll(fm);
        if (cursor < total && (nfree >= (u32)KMC_SIM_REFILL_MIN || nfree == 64u)) {
            const u32 take = kmc_min(nfree, total - cursor);
            const u32 q = cursor + kmc_rank_in(fm);
            const bool mine = !alive && q < cursor + take;
            const u32 nrel = (wave0 + q / KMC_SIM_CHUNK * nwaves) * KMC_SIM_CHUNK + q % KMC_SIM_CHUNK;
            const u32 row = (a.row0 + nrel) % a.n_starts;   // (row0 < 2^27, nrel < 2^25: no wrap of the sum)
            const u32 r0 = __builtin_amdgcn_readfirstlane(row);
            if (fm == ~0ull && cursor % KMC_SIM_CHUNK + take <= KMC_SIM_CHUNK && r0 + take <= a.n_starts) {
                T::load(a.starts + (u64)r0 * (u64)W, 0, take, lds[wib], lane, s);   // lane j: row r0 + j, walker q
            } else if (mine) {
#pragma unroll
                for (int k = 0; k < W; ++k) s[k] = a.starts[(u64)row * (u64)W + k];
            }
            t = mine ? 0u : t;
            rel = mine ? nrel : rel;
            key = mine ? kmc_sim_key(a.seed, a.first_walk + nrel) : key;
            meta = mine ? 0ull : meta;
            alive = alive || mine;
            cursor += take;
        }
        if (__ballot(alive) == 0) break;   // (... and the cursor is exhausted: 64 free lanes would have been filled)
        const typename M::Pre pre = M::extract(s);
        const u64 col = a.rec_col0 + rel;
        if (record && alive) {
#pragma unroll
            for (int k = 0; k < W; ++k) a.rec[((u64)t * (W + 1) + k) * a.rec_stride + col] = s[k];
            a.rec[((u64)t * (W + 1) + W) * a.rec_stride + col] = meta;
        }
        const u32 bad = (alive && a.inv_mask) ? M::violated_pre(pre, a.inv_mask) : 0u;
        if (__ballot(bad != 0)) {
            if (bad) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (bad >> k & 1u) atomicAdd(&a.ctl->viol_count[k], 1ull);
                atomicMin(&a.ctl->witness, ((u64)rel << 32) | ((u64)t << 8) | (u64)(bad & 15u));
            }
        }
        bool live = alive && bad == 0 && t + 1u < a.depth;   // goes on to state t + 1
        if (__ballot(live)) {
            typename S::Cand c;
            const u32 n = S::count(pre, s, live ? 1u : 0u, c);
            const bool stuck = live && n == 0;
            const u64 sm = __ballot(stuck);
            if (sm) {
                early += (u64)__popcll(sm);
                if (stuck && (a.flags & KMC_SIM_FLAG_DEADLOCK))
                    atomicMin(&a.ctl->witness, ((u64)rel << 32) | ((u64)t << 8) | (u64)KMC_SIM_DEADLOCK_BIT);
                live = live && !stuck;
            }
            const u32 r = live ? (u32)kmc_sim_draw_key(key, t, n) : 0u;
            const u32 ci = live ? S::locate(c, r) : (u32)M::NINST;   // (NINST: no leaf is this lane's)
            u64 nx[W];
#pragma unroll
            for (int k = 0; k < W; ++k) nx[k] = s[k];
            int kind = 0;
            if constexpr (M::KIND_MAJOR) {
                kmc_static_for<0, M::NSEGS>([&](auto SS) {
                    constexpr int sg = decltype(SS)::value;
                    constexpr int K = M::seg_kind(sg);
                    constexpr u32 lo = (u32)(M::kind_base(K) + M::seg_first(sg)), cnt = (u32)M::seg_count(sg);
                    const bool mine = ci - lo < cnt;
                    const u64 m = __ballot(mine);
                    if (m) {
                        const u32 b = mine ? ci - (u32)M::kind_base(K) : (u32)M::seg_first(sg);
                        u32 extra = 0;
                        u64 tt[W];
                        M::template apply<K>(pre, s, tt, b, extra);
#pragma unroll
                        for (int k = 0; k < W; ++k) nx[k] = mine ? tt[k] : nx[k];
                        kind = mine ? K : kind;
                        taken_lane += lane == (u32)K ? (u64)__popcll(m) : 0ull;
                    }
                });
            } else {
                kmc_static_for<0, M::NINST>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    const bool mine = ci == (u32)i;
                    const u64 m = __ballot(mine);
                    if (m) {
                        int kd = 0;
                        u32 extra = 0;
                        u64 tt[W];
                        (void)M::template inst<i>(pre, s, tt, kd, extra);
#pragma unroll
                        for (int k = 0; k < W; ++k) nx[k] = mine ? tt[k] : nx[k];
                        kind = mine ? kd : kind;
                        taken_lane += lane == (u32)kd ? (u64)__popcll(m) : 0ull;
                    }
                });
            }
#pragma unroll
            for (int k = 0; k < W; ++k) s[k] = nx[k];
            meta = kmc_sim_meta(kind, r, n);
        }
        if (alive && !live) {   // the walk ends on state t: its lane is free from the next step on
            if (record) a.rec_len[col] = (u64)t + 1ull;
            states += (u64)t + 1ull;
            longest = t + 1u > longest ? t + 1u : longest;
        }
        alive = live;
        t += 1u;
    }
    const u32 lmax = kmc_wave_max(longest);
    const u64 nstates = kmc_wave_sum64(states);
    if (lane < (u32)M::NKINDS && taken_lane) atomicAdd(&a.ctl->taken[lane], taken_lane);
    if (lane == 0) {
        if (nstates) atomicAdd(&a.ctl->states, nstates);
        if (early) atomicAdd(&a.ctl->ended_early, early);
        if (lmax) atomicMax(&a.ctl->longest, (u64)lmax);
    }
}

#if KMC_ONLY_MODE == 3
#define KMC_INSTANTIATE(NAME, ...)                                                                \
    extern "C" __global__ __launch_bounds__(KMC_BLOCK) void kmc_simulate_##NAME(KmcSimArgs a) {   \
        kmc_simulate_body<__VA_ARGS__>(a);                                                        \
    }                                                                                             \
    extern "C" __global__ __launch_bounds__(KMC_BLOCK) void kmc_simulate_from_##NAME(KmcSimFromArgs a) { \
        kmc_simulate_from_body<__VA_ARGS__>(a);                                                   \
    }
#endif
#endif  // !KMC_HOST_EMU
