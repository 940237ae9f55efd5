// Host emulation of random simulation: the LANE-LOCAL layer of kafka_specification_amd/csrc/kmc_sim.h (the draw, counting a
// state's candidates, locating the r-th, its effect) compiled by g++ with KMC_HOST_EMU, one walker at a time, and the batch
// logic of include/kmc.h's contract around it (launches of walks_per_launch, the witness, the counters) written a second time.
// What k_simulate computes on the GPU must equal this bit for bit (tests/test_gpu_simulate.py); what this computes is held to
// the C oracle step by step (tests/test_simulate_cpu.py).  Also the CPU baseline of tools/sim_bench.py (a port, not TLC).
// TEST INFRASTRUCTURE ONLY — nothing in the product links this.
#define KMC_HOST_EMU 1
#include "../kafka_specification_amd/csrc/kmc_device.h"

#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

constexpr u32 END_STUCK = 32u;   // in a walk's end bits: it ended on a state without candidates (bits 0..3: invariants violated)

// One walk.  rec (optional): depth records of W + 1 words — the state, kmc_sim_meta of how it was reached.  -> its states.
template <class M> u32 walk(u64 seed, u64 w, u32 depth, u32 inv_mask, u64* rec, u32* end_bits, u64* taken) {
    using S = KmcSim<M>;
    constexpr int W = M::W;
    u64 s[W];
    M::init(s);
    u64 meta = 0;
    *end_bits = 0;
    for (u32 t = 0;; ++t) {
        const typename M::Pre pre = M::extract(s);
        if (rec) {
            for (int k = 0; k < W; ++k) rec[(size_t)t * (W + 1) + k] = s[k];
            rec[(size_t)t * (W + 1) + W] = meta;
        }
        const u32 bad = inv_mask ? M::violated_pre(pre, inv_mask) : 0u;
        if (bad) {
            *end_bits = bad & 15u;
            return t + 1;
        }
        if (t + 1 >= depth) return t + 1;
        typename S::Cand c;
        const u32 n = S::count(pre, s, 1u, c);
        if (n == 0) {
            *end_bits = END_STUCK;
            return t + 1;
        }
        const u32 r = (u32)kmc_sim_draw_of(seed, w, t, n);
        const u32 ci = S::locate(c, r);
        u64 nx[W];
        int kind = 0;
        S::effect(pre, s, ci, nx, kind);
        taken[kind] += 1;
        for (int k = 0; k < W; ++k) s[k] = nx[k];
        meta = kmc_sim_meta(kind, r, n);
    }
}

struct Entry {
    int model, N, L, R, E, K, lm;
    int words;
    u32 (*walk)(u64, u64, u32, u32, u64*, u32*, u64*);
};
#define KAFKA_LM(MODEL, N, L, R, E, LM) \
    {MODEL, N, L, R, E, 0, LM, KmcKafka<MODEL, N, L, R, E, LM>::W, walk<KmcKafka<MODEL, N, L, R, E, LM>>}
#define KAFKA(MODEL, N, L, R, E) KAFKA_LM(MODEL, N, L, R, E, KMC_LAYOUT_AUTO)
#define FRL(N, L, K) \
    {KMC_MODEL_FINITE_REPLICATED_LOG, N, L, 0, 0, K, 0, KmcFiniteReplicatedLog<N, L, K>::W, walk<KmcFiniteReplicatedLog<N, L, K>>}

const Entry TABLE[] = {
    KAFKA(KMC_MODEL_KIP320, 3, 2, 2, 1),
#ifndef SIM_EMU_SMALL_TABLE   // (tests/sim_san.cpp under -fsanitize=address,undefined keeps one entry of each shape)
    KAFKA(KMC_MODEL_TRUNCATE_TO_HW, 3, 2, 2, 2), KAFKA(KMC_MODEL_KIP320_FIRST_TRY, 3, 2, 2, 2), KAFKA(KMC_MODEL_KIP101, 3, 2, 2, 2),
    KAFKA(KMC_MODEL_KIP320, 4, 2, 2, 1), KAFKA(KMC_MODEL_KIP320, 7, 1, 1, 0),
    // the two arrangements of the state vector forced (KMC_LAYOUT=tight / rm on the host library's side)
    KAFKA_LM(KMC_MODEL_KIP320, 3, 2, 2, 1, KMC_LAYOUT_TIGHT),
    // the bindings tools/sim_bench.py measures: the headline and BASELINE config 5
    KAFKA(KMC_MODEL_KIP320, 3, 6, 6, 2), KAFKA(KMC_MODEL_KIP320, 7, 8, 8, 3),
#endif
    KAFKA_LM(KMC_MODEL_KIP320, 3, 2, 2, 1, KMC_LAYOUT_RM),
    KAFKA(KMC_MODEL_KIP279, 3, 2, 2, 2),
    FRL(2, 4, 2),
    {KMC_MODEL_IDSEQUENCE, 0, 0, 0, 0, 10, 0, 1, walk<KmcIdSequence<10>>},   // (K stands for MaxId here)
};

const Entry* find(const int* c7) {
    for (const Entry& e : TABLE)
        if (e.model == c7[0] && e.N == c7[1] && e.L == c7[2] && e.R == c7[3] && e.E == c7[4] && e.K == c7[5] && e.lm == c7[6]) return &e;
    return nullptr;
}

}  // namespace

extern "C" {

// mirrors kmc_sim_result (include/kmc.h) without the times
struct SimEmuResult {
    uint64_t walks, states_generated, action_taken[16], ended_early, longest_walk;
    int32_t verdict, violated_invariant;
    uint64_t violation_walk, violation_step, violation_count[4], launches;
};

// number of configurations compiled in; fills (model, N, L, R, E, K, layout mode) of entry i
int sim_emu_configs(int i, int* out7) {
    const int n = (int)(sizeof TABLE / sizeof TABLE[0]);
    if (i >= 0 && i < n) {
        const Entry& e = TABLE[i];
        out7[0] = e.model; out7[1] = e.N; out7[2] = e.L; out7[3] = e.R; out7[4] = e.E; out7[5] = e.K; out7[6] = e.lm;
    }
    return n;
}
int sim_emu_words(const int* c7) {
    const Entry* e = find(c7);
    return e ? e->words : -1;
}
uint64_t sim_emu_draw(uint64_t seed, uint64_t walk, uint32_t step, uint32_t n) { return kmc_sim_draw_of(seed, walk, step, n); }

// One batch by the contract.  rec (optional): [n_walks][depth][W + 1] words; lens (optional): [n_walks] states per walk (0 for a
// walk of a launch that never ran).  -> 0, -1 for an unknown configuration.
int sim_emu_run(const int* c7, uint64_t seed, uint64_t first_walk, uint64_t n_walks, uint32_t depth, uint64_t wpl, uint32_t inv_mask,
                int check_deadlock, int continue_on_violation, int threads, SimEmuResult* res, u64* rec, uint32_t* lens) {
    const Entry* e = find(c7);
    if (!e) return -1;
    if (depth == 0) depth = 100;
    if (wpl == 0) wpl = 1ull << 20;
    if (threads < 1) threads = 1;
    SimEmuResult r{};
    r.violated_invariant = -1;
    const size_t rw = (size_t)depth * (e->words + 1);
    if (lens) memset(lens, 0, n_walks * sizeof *lens);
    for (uint64_t done = 0; done < n_walks; done += wpl) {
        const uint64_t n = n_walks - done < wpl ? n_walks - done : wpl;
        std::vector<uint32_t> len(n), bits(n);
        std::vector<std::vector<u64>> taken(threads, std::vector<u64>(16, 0));
        auto work = [&](int th) {
            for (uint64_t i = th; i < n; i += threads)
                len[i] = e->walk(seed, first_walk + done + i, depth, inv_mask, rec ? rec + (done + i) * rw : nullptr, &bits[i], taken[th].data());
        };
        std::vector<std::thread> pool;
        for (int th = 1; th < threads; ++th) pool.emplace_back(work, th);
        work(0);
        for (auto& t : pool) t.join();
        r.launches += 1;
        r.walks += n;
        bool have = false;
        for (uint64_t i = 0; i < n; ++i) {
            r.states_generated += len[i];
            if (len[i] > r.longest_walk) r.longest_walk = len[i];
            if (lens) lens[done + i] = len[i];
            if (bits[i] & END_STUCK) r.ended_early += 1;
            for (int k = 0; k < 4; ++k) r.violation_count[k] += bits[i] >> k & 1u;
            const bool verdict_here = (bits[i] & 15u) || ((bits[i] & END_STUCK) && check_deadlock);
            if (verdict_here && !have && r.verdict == 0) {   // the smallest walk index of the first launch that holds one
                have = true;
                r.violation_walk = first_walk + done + i;
                r.violation_step = len[i] - 1;
                if (bits[i] & 15u) {
                    r.verdict = 1;
                    r.violated_invariant = __builtin_ctz(bits[i] & 15u);
                } else {
                    r.verdict = 2;
                }
            }
        }
        for (int th = 0; th < threads; ++th)
            for (int k = 0; k < 16; ++k) r.action_taken[k] += taken[th][k];
        if (r.verdict != 0 && !continue_on_violation) break;
    }
    *res = r;
    return 0;
}
}
