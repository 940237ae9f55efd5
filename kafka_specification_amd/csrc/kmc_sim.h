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
// code that g++ compiles too — tests/sim_emu.cpp) and the WAVE one (k_simulate: one lane per walker, state in registers).
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

#if KMC_ONLY_MODE == 3
#define KMC_INSTANTIATE(NAME, ...)                                                                \
    extern "C" __global__ __launch_bounds__(KMC_BLOCK) void kmc_simulate_##NAME(KmcSimArgs a) {   \
        kmc_simulate_body<__VA_ARGS__>(a);                                                        \
    }
#endif
#endif  // !KMC_HOST_EMU
