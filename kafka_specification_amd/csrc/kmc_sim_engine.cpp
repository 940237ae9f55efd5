// kmc_sim_engine.cpp — random simulation: kmc_simulate / kmc_simulate_walk / kmc_sim_draw over k_simulate, and kmc_simulate_from /
// kmc_simulate_from_walk (walks from start states given as data) over k_simulate_from (kmc_sim.h: both kernels), the
// fourth code object of a configuration.  Stands where TLC's -simulate mode stands [TLC-recall]; include/kmc.h holds the
// contract of a walk.  The seen-set, the frontiers and the search's control blocks are not touched.
#include "kmc_engine_internal.h"
using namespace kmc_engine;

namespace kmc_engine {

void sim_release(kmc_handle* h) {
    if (h->sim_rec) (void)hipFree(h->sim_rec);
    if (h->sim_one) (void)hipFree(h->sim_one);
    if (h->sim_starts) (void)hipFree(h->sim_starts);
    if (h->sim_ctl) (void)hipFree(h->sim_ctl);
    if (h->sim_ctl_host) (void)hipHostFree(h->sim_ctl_host);
    if (h->mod_sim) (void)hipModuleUnload(h->mod_sim);
    h->sim_rec = h->sim_one = h->sim_starts = nullptr;
    h->sim_starts_words = 0;
    h->sim_ctl = h->sim_ctl_host = nullptr;
    h->mod_sim = nullptr;
    h->f_sim = h->f_sim_from = nullptr;
}

}  // namespace kmc_engine

// what a handle cannot walk, and the defaults of a batch
static int sim_check(kmc_handle* h, const kmc_sim_config* sim, uint32_t* depth, uint64_t* wpl) {
    if (!h || !sim) return fail(KMC_E_ARG, "null argument");
    if (h->cfg.model == KMC_ASYNC_ISR)
        return fail(KMC_E_ARG, "random simulation of AsyncIsr is not implemented: which successors outside the state constraint "
                               "count as candidates of a walk is undecided");
    if (h->cfg.symmetry) return fail(KMC_E_ARG, "random simulation walks real states: open the handle without symmetry");
    if (!h->table) return fail(KMC_E_STATE, "host-only handle: random simulation runs on the device");
    *depth = sim->depth ? sim->depth : 100u;
    if (*depth > KMC_SIM_MAX_DEPTH) return fail(KMC_E_ARG, "depth %u: at most %u states per walk", *depth, KMC_SIM_MAX_DEPTH);
    *wpl = sim->walks_per_launch ? sim->walks_per_launch : (1ull << 20);
    if (*wpl > (1ull << 24)) return fail(KMC_E_ARG, "walks_per_launch %llu: at most 2^24", (unsigned long long)*wpl);
    return KMC_OK;
}

// ... and what kmc_simulate_from refuses of its start states
static int starts_check(const kmc_handle* h, const uint64_t* starts, uint64_t n_starts) {
    if (!starts || n_starts == 0) return fail(KMC_E_ARG, "no start states: kmc_simulate_from walks from at least one");
    if ((unsigned __int128)n_starts * h->W * 8 > KMC_SIM_STARTS_MAX_BYTES)
        return fail(KMC_E_ARG, "%llu start states take more than the staging's bound of %llu bytes: sub-sample them",
                    (unsigned long long)n_starts, (unsigned long long)KMC_SIM_STARTS_MAX_BYTES);
    return KMC_OK;
}

// k_simulate's code object joins the handle (from the cache; a cold cache compiles it: kmc_precompile_simulate), with its control block
static int sim_ensure(kmc_handle* h) {
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (!h->f_sim) {
        std::vector<char> code;
        std::string kname;
        int rc = get_code_object(h->cfg, h->arch, &code, &kname, nullptr, nullptr, KMC_CODEOBJ_SIM, &h->knobs.jit_defines, h->knobs.layout_mode);
        if (rc) return rc;
        HIP_TRY(hipModuleLoadData(&h->mod_sim, code.data()));
        HIP_TRY(hipModuleGetFunction(&h->f_sim, h->mod_sim, (std::string(MODE_KERNEL[KMC_CODEOBJ_SIM]) + "_" + h->kname).c_str()));
        HIP_TRY(hipModuleGetFunction(&h->f_sim_from, h->mod_sim, ("kmc_simulate_from_" + h->kname).c_str()));
    }
    if (!h->sim_ctl) HIP_TRY(hipMalloc(&h->sim_ctl, sizeof(KmcSimCtl)));
    if (!h->sim_ctl_host) HIP_TRY(hipHostMalloc(&h->sim_ctl_host, sizeof(KmcSimCtl)));
    return KMC_OK;
}

// words of a record area of `columns` walkers: depth planes of W + 1 words each, then the walks' lengths
static uint64_t rec_words(const kmc_handle* h, uint32_t depth, uint64_t columns) { return ((uint64_t)depth * (h->W + 1) + 1) * columns; }

// `n` rows of start states into the handle's staging, which grows on demand
static int starts_upload(kmc_handle* h, const uint64_t* rows, uint64_t n) {
    const uint64_t need = n * h->W;
    if (need > h->sim_starts_words) {
        if (h->sim_starts) (void)hipFree(h->sim_starts);
        h->sim_starts = nullptr;
        h->sim_starts_words = 0;
        if (hipMalloc(&h->sim_starts, need * 8) != hipSuccess) return fail(KMC_E_NOMEM, "start-state staging of %llu bytes", (unsigned long long)need * 8);
        h->sim_starts_words = need;
    }
    HIP_TRY(hipMemcpy(h->sim_starts, rows, need * 8, hipMemcpyHostToDevice));
    return KMC_OK;
}

// k_simulate's arguments: k_simulate_from's without the start states
static KmcSimArgs sim_args_of(const KmcSimFromArgs& f) {
    KmcSimArgs a{};
    a.rec = f.rec;
    a.rec_len = f.rec_len;
    a.rec_stride = f.rec_stride;
    a.rec_col0 = f.rec_col0;
    a.seed = f.seed;
    a.first_walk = f.first_walk;
    a.n = f.n;
    a.depth = f.depth;
    a.inv_mask = f.inv_mask;
    a.flags = f.flags;
    return a;
}

// one launch of k_simulate (KmcSimArgs) or k_simulate_from (KmcSimFromArgs): its control block zeroed before and, in sim_ctl_host,
// read back after; *ms = the kernel's duration
template <class Args> static int sim_launch(kmc_handle* h, Args a, float* ms) {
    constexpr bool from = std::is_same<Args, KmcSimFromArgs>::value;
    KmcSimCtl* c = h->sim_ctl_host;
    memset(c, 0, sizeof *c);
    c->witness = KMC_SIM_NO_WITNESS;
    HIP_TRY(hipMemcpyAsync(h->sim_ctl, c, sizeof *c, hipMemcpyHostToDevice, h->stream));
    a.ctl = h->sim_ctl;
    // (k_simulate: a tile of 64 walkers per wave and round; k_simulate_from: a chunk of KMC_SIM_CHUNK walkers per wave and round)
    const uint64_t per_block = from ? (uint64_t)KMC_SIM_CHUNK * KMC_WAVES : (uint64_t)KMC_BLOCK;
    uint64_t blocks = ((uint64_t)a.n + per_block - 1) / per_block;
    const uint64_t maxb = (uint64_t)h->n_cus * 8;
    if (blocks > maxb) blocks = maxb;
    size_t size = sizeof a;
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    HIP_TRY(hipModuleLaunchKernel(from ? h->f_sim_from : h->f_sim, (unsigned)blocks, 1, 1, KMC_BLOCK, 1, 1, 0, h->stream, nullptr, config));
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipMemcpyAsync(c, h->sim_ctl, sizeof *c, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return KMC_OK;
}

extern "C" {

uint64_t kmc_sim_draw(uint64_t seed, uint64_t walk, uint32_t step, uint32_t n) { return kmc_sim_draw_of(seed, walk, step, n); }

}  // extern "C"

// A batch.  starts = null: kmc_simulate (k_simulate, every walk from Init); else kmc_simulate_from (k_simulate_from).
static int sim_batch_run(kmc_handle* h, const kmc_sim_config* sim, const uint64_t* starts, uint64_t n_starts, bool from, kmc_sim_result* out) {
    uint32_t depth = 0;
    uint64_t wpl = 0;
    int rc = sim_check(h, sim, &depth, &wpl);
    if (rc) return rc;
    if (from && (rc = starts_check(h, starts, n_starts))) return rc;
    if (!out) return fail(KMC_E_ARG, "null argument");
    if (sim->n_walks == 0) return fail(KMC_E_ARG, "n_walks = 0: a batch holds at least one walk");
    const double t0 = now_s();
    if (sim->record) {
        const unsigned __int128 bytes = (unsigned __int128)rec_words(h, depth, 1) * sim->n_walks * 8;
        if (bytes > KMC_SIM_RECORD_MAX_BYTES)
            return fail(KMC_E_ARG, "recording %llu walks of depth %u takes more than the record buffer's bound of %llu bytes: record a "
                                   "smaller batch", (unsigned long long)sim->n_walks, depth, (unsigned long long)KMC_SIM_RECORD_MAX_BYTES);
    }
    if ((rc = sim_ensure(h))) return rc;
    h->sim_batch.valid = false;
    if (from && (rc = starts_upload(h, starts, n_starts))) return rc;
    if (sim->record) {
        const uint64_t need = rec_words(h, depth, sim->n_walks);
        if (need > h->sim_rec_words) {
            if (h->sim_rec) (void)hipFree(h->sim_rec);
            h->sim_rec = nullptr;
            h->sim_rec_words = 0;
            if (hipMalloc(&h->sim_rec, need * 8) != hipSuccess) return fail(KMC_E_NOMEM, "record buffer of %llu bytes", (unsigned long long)need * 8);
            h->sim_rec_words = need;
        }
    }
    kmc_sim_result r{};
    r.verdict = KMC_V_OK;
    r.violated_invariant = -1;
    KmcSimFromArgs a{};   // (k_simulate's arguments are these without the start states)
    a.rec = sim->record ? h->sim_rec : nullptr;
    a.rec_stride = sim->n_walks;
    a.rec_len = sim->record ? h->sim_rec + (uint64_t)depth * (h->W + 1) * sim->n_walks : nullptr;
    a.seed = sim->seed;
    a.starts = h->sim_starts;
    a.n_starts = (uint32_t)n_starts;
    a.depth = depth;
    a.inv_mask = h->cfg.invariant_mask;
    a.flags = (sim->record ? KMC_SIM_FLAG_RECORD : 0u) | (h->cfg.check_deadlock ? KMC_SIM_FLAG_DEADLOCK : 0u);
    for (uint64_t done = 0; done < sim->n_walks; done += wpl) {
        a.n = (uint32_t)(sim->n_walks - done < wpl ? sim->n_walks - done : wpl);
        a.rec_col0 = done;
        a.first_walk = sim->first_walk + done;
        float ms = 0;
        if (from) {
            a.row0 = (uint32_t)(a.first_walk % n_starts);
            rc = sim_launch(h, a, &ms);
        } else {
            rc = sim_launch(h, sim_args_of(a), &ms);
        }
        if (rc) return rc;
        const KmcSimCtl& c = *h->sim_ctl_host;
        r.launches += 1;
        r.seconds_kernel += ms * 1e-3;
        r.walks += a.n;
        r.states_generated += c.states;
        r.ended_early += c.ended_early;
        if (c.longest > r.longest_walk) r.longest_walk = c.longest;
        for (int k = 0; k < KMC_MAX_KINDS; ++k) r.action_taken[k] += c.taken[k];
        for (int k = 0; k < 4; ++k) r.violation_count[k] += c.viol_count[k];
        if (c.witness != KMC_SIM_NO_WITNESS && r.verdict == KMC_V_OK) {
            const uint32_t bits = (uint32_t)(c.witness & 0xFFu);
            r.violation_walk = a.first_walk + (c.witness >> 32);
            r.violation_step = (c.witness >> 8) & 0xFFFFFFu;
            if (bits & 15u) {
                r.verdict = KMC_V_INVARIANT;
                r.violated_invariant = __builtin_ctz(bits & 15u);
            } else {
                r.verdict = KMC_V_DEADLOCK;
            }
        }
        if (r.verdict != KMC_V_OK && !h->cfg.continue_on_violation) break;
    }
    if (sim->record) {
        h->sim_batch.seed = sim->seed;
        h->sim_batch.first_walk = sim->first_walk;
        h->sim_batch.walks_done = r.walks;
        h->sim_batch.stride = sim->n_walks;
        h->sim_batch.depth = depth;
        h->sim_batch.valid = true;
        h->sim_batch.from = from;
    }
    r.seconds_total = now_s() - t0;
    *out = r;
    return KMC_OK;
}

// One walk as data.  `from`: a walk of kmc_simulate_from, which starts on `start` (its row of the caller's start states).
static int sim_walk_read(kmc_handle* h, const kmc_sim_config* sim, bool from, const uint64_t* start, uint64_t walk, uint8_t* canon_states,
                         int32_t* kinds, uint32_t* choice, uint32_t* n_enabled, uint64_t cap, uint64_t* n_out) {
    uint32_t depth = 0;
    uint64_t wpl = 0;
    int rc = sim_check(h, sim, &depth, &wpl);
    if (rc) return rc;
    if (!n_out) return fail(KMC_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const auto& b = h->sim_batch;
    const u64* area = nullptr;
    uint64_t stride = 0, col = 0;
    // (a batch of the other call holds other walks under the same indices: it is not read)
    bool recorded = b.valid && b.from == from && b.seed == sim->seed && b.depth == depth && walk >= b.first_walk && walk - b.first_walk < b.walks_done;
    if (recorded && from) {   // ... nor is a from-batch that started this walk elsewhere: its recorded s_0 is compared
        std::vector<uint64_t> s0(h->W);
        HIP_TRY(hipMemcpy2D(s0.data(), 8, h->sim_rec + (walk - b.first_walk), b.stride * 8, 8, h->W, hipMemcpyDeviceToHost));
        recorded = memcmp(s0.data(), start, (size_t)h->W * 8) == 0;
    }
    if (recorded) {
        area = h->sim_rec;
        stride = b.stride;
        col = walk - b.first_walk;
    } else {   // not in the recorded batch: that one walker again, in record mode, into an area of its own
        if ((rc = sim_ensure(h))) return rc;
        const uint64_t need = rec_words(h, depth, 1);
        if (need > h->sim_one_words) {
            if (h->sim_one) (void)hipFree(h->sim_one);
            h->sim_one = nullptr;
            h->sim_one_words = 0;
            if (hipMalloc(&h->sim_one, need * 8) != hipSuccess) return fail(KMC_E_NOMEM, "record buffer of %llu bytes", (unsigned long long)need * 8);
            h->sim_one_words = need;
        }
        if (from && (rc = starts_upload(h, start, 1))) return rc;   // (only that row)
        KmcSimFromArgs a{};
        a.rec = h->sim_one;
        a.rec_stride = 1;
        a.rec_len = h->sim_one + (uint64_t)depth * (h->W + 1);
        a.rec_col0 = 0;
        a.seed = sim->seed;
        a.first_walk = walk;
        a.starts = h->sim_starts;
        a.n_starts = 1;
        a.row0 = 0;
        a.n = 1;
        a.depth = depth;
        a.inv_mask = h->cfg.invariant_mask;
        a.flags = KMC_SIM_FLAG_RECORD | (h->cfg.check_deadlock ? KMC_SIM_FLAG_DEADLOCK : 0u);
        float ms = 0;
        if ((rc = from ? sim_launch(h, a, &ms) : sim_launch(h, sim_args_of(a), &ms))) return rc;
        area = h->sim_one;
        stride = 1;
        col = 0;
    }
    const uint64_t rw = (uint64_t)h->W + 1;
    uint64_t len = 0;
    HIP_TRY(hipMemcpy(&len, area + (uint64_t)depth * rw * stride + col, 8, hipMemcpyDeviceToHost));
    if (len == 0 || len > depth) return fail(KMC_E_STATE, "recorded walk %llu has an impossible length %llu", (unsigned long long)walk, (unsigned long long)len);
    *n_out = len;
    const uint64_t take = len < cap ? len : cap;
    if (take == 0) return KMC_OK;
    std::vector<uint64_t> words(take * rw);   // the walk's column: one word per (step, plane)
    HIP_TRY(hipMemcpy2D(words.data(), 8, area + col, stride * 8, 8, take * rw, hipMemcpyDeviceToHost));
    const uint64_t cb = kmc_canon_bytes(h);
    for (uint64_t t = 0; t < take; ++t) {
        const uint64_t meta = words[t * rw + h->W];
        if (canon_states) kmc_unpack_state(h, &words[t * rw], canon_states + t * cb);
        if (kinds) kinds[t] = (int32_t)(meta & 0xFFFFu) - 1;
        if (choice) choice[t] = (uint32_t)(meta >> 16) & 0xFFFFFFu;
        if (n_enabled) n_enabled[t] = (uint32_t)(meta >> 40);
    }
    return KMC_OK;
}

extern "C" {

int kmc_simulate(kmc_handle* h, const kmc_sim_config* sim, kmc_sim_result* out) { return sim_batch_run(h, sim, nullptr, 0, false, out); }

int kmc_simulate_from(kmc_handle* h, const kmc_sim_config* sim, const uint64_t* starts, uint64_t n_starts, kmc_sim_result* out) {
    return sim_batch_run(h, sim, starts, n_starts, true, out);
}

int kmc_simulate_walk(kmc_handle* h, const kmc_sim_config* sim, uint64_t walk, uint8_t* canon_states, int32_t* kinds,
                      uint32_t* choice, uint32_t* n_enabled, uint64_t cap, uint64_t* n_out) {
    return sim_walk_read(h, sim, false, nullptr, walk, canon_states, kinds, choice, n_enabled, cap, n_out);
}

int kmc_simulate_from_walk(kmc_handle* h, const kmc_sim_config* sim, const uint64_t* starts, uint64_t n_starts, uint64_t walk,
                           uint8_t* canon_states, int32_t* kinds, uint32_t* choice, uint32_t* n_enabled, uint64_t cap, uint64_t* n_out) {
    uint32_t depth = 0;
    uint64_t wpl = 0;
    int rc = sim_check(h, sim, &depth, &wpl);
    if (rc || (rc = starts_check(h, starts, n_starts))) return rc;
    return sim_walk_read(h, sim, true, starts + (walk % n_starts) * h->W, walk, canon_states, kinds, choice, n_enabled, cap, n_out);
}

}  // extern "C"
