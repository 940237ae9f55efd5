// kmc_sim_engine.cpp — random simulation: kmc_simulate / kmc_simulate_walk / kmc_sim_draw over k_simulate (kmc_sim.h), the
// fourth code object of a configuration.  Stands where TLC's -simulate mode stands [TLC-recall]; include/kmc.h holds the
// contract of a walk.  The seen-set, the frontiers and the search's control blocks are not touched.
#include "kmc_engine_internal.h"
using namespace kmc_engine;

namespace kmc_engine {

void sim_release(kmc_handle* h) {
    if (h->sim_rec) (void)hipFree(h->sim_rec);
    if (h->sim_one) (void)hipFree(h->sim_one);
    if (h->sim_ctl) (void)hipFree(h->sim_ctl);
    if (h->sim_ctl_host) (void)hipHostFree(h->sim_ctl_host);
    if (h->mod_sim) (void)hipModuleUnload(h->mod_sim);
    h->sim_rec = h->sim_one = nullptr;
    h->sim_ctl = h->sim_ctl_host = nullptr;
    h->mod_sim = nullptr;
    h->f_sim = nullptr;
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
    }
    if (!h->sim_ctl) HIP_TRY(hipMalloc(&h->sim_ctl, sizeof(KmcSimCtl)));
    if (!h->sim_ctl_host) HIP_TRY(hipHostMalloc(&h->sim_ctl_host, sizeof(KmcSimCtl)));
    return KMC_OK;
}

// words of a record area of `columns` walkers: depth planes of W + 1 words each, then the walks' lengths
static uint64_t rec_words(const kmc_handle* h, uint32_t depth, uint64_t columns) { return ((uint64_t)depth * (h->W + 1) + 1) * columns; }

// one launch: its control block zeroed before and, in sim_ctl_host, read back after; *ms = the kernel's duration
static int sim_launch(kmc_handle* h, KmcSimArgs a, float* ms) {
    KmcSimCtl* c = h->sim_ctl_host;
    memset(c, 0, sizeof *c);
    c->witness = KMC_SIM_NO_WITNESS;
    HIP_TRY(hipMemcpyAsync(h->sim_ctl, c, sizeof *c, hipMemcpyHostToDevice, h->stream));
    a.ctl = h->sim_ctl;
    uint64_t blocks = ((uint64_t)a.n + KMC_BLOCK - 1) / KMC_BLOCK;
    const uint64_t maxb = (uint64_t)h->n_cus * 8;
    if (blocks > maxb) blocks = maxb;
    size_t size = sizeof a;
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    HIP_TRY(hipModuleLaunchKernel(h->f_sim, (unsigned)blocks, 1, 1, KMC_BLOCK, 1, 1, 0, h->stream, nullptr, config));
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipMemcpyAsync(c, h->sim_ctl, sizeof *c, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return KMC_OK;
}

extern "C" {

uint64_t kmc_sim_draw(uint64_t seed, uint64_t walk, uint32_t step, uint32_t n) { return kmc_sim_draw_of(seed, walk, step, n); }

int kmc_simulate(kmc_handle* h, const kmc_sim_config* sim, kmc_sim_result* out) {
    uint32_t depth = 0;
    uint64_t wpl = 0;
    int rc = sim_check(h, sim, &depth, &wpl);
    if (rc) return rc;
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
    KmcSimArgs a{};
    a.rec = sim->record ? h->sim_rec : nullptr;
    a.rec_stride = sim->n_walks;
    a.rec_len = sim->record ? h->sim_rec + (uint64_t)depth * (h->W + 1) * sim->n_walks : nullptr;
    a.seed = sim->seed;
    a.depth = depth;
    a.inv_mask = h->cfg.invariant_mask;
    a.flags = (sim->record ? KMC_SIM_FLAG_RECORD : 0u) | (h->cfg.check_deadlock ? KMC_SIM_FLAG_DEADLOCK : 0u);
    for (uint64_t done = 0; done < sim->n_walks; done += wpl) {
        a.n = (uint32_t)(sim->n_walks - done < wpl ? sim->n_walks - done : wpl);
        a.rec_col0 = done;
        a.first_walk = sim->first_walk + done;
        float ms = 0;
        if ((rc = sim_launch(h, a, &ms))) return rc;
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
    }
    r.seconds_total = now_s() - t0;
    *out = r;
    return KMC_OK;
}

int kmc_simulate_walk(kmc_handle* h, const kmc_sim_config* sim, uint64_t walk, uint8_t* canon_states, int32_t* kinds,
                      uint32_t* choice, uint32_t* n_enabled, uint64_t cap, uint64_t* n_out) {
    uint32_t depth = 0;
    uint64_t wpl = 0;
    int rc = sim_check(h, sim, &depth, &wpl);
    if (rc) return rc;
    if (!n_out) return fail(KMC_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const auto& b = h->sim_batch;
    const u64* area = nullptr;
    uint64_t stride = 0, col = 0;
    if (b.valid && b.seed == sim->seed && b.depth == depth && walk >= b.first_walk && walk - b.first_walk < b.walks_done) {
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
        KmcSimArgs a{};
        a.rec = h->sim_one;
        a.rec_stride = 1;
        a.rec_len = h->sim_one + (uint64_t)depth * (h->W + 1);
        a.rec_col0 = 0;
        a.seed = sim->seed;
        a.first_walk = walk;
        a.n = 1;
        a.depth = depth;
        a.inv_mask = h->cfg.invariant_mask;
        a.flags = KMC_SIM_FLAG_RECORD | (h->cfg.check_deadlock ? KMC_SIM_FLAG_DEADLOCK : 0u);
        float ms = 0;
        if ((rc = sim_launch(h, a, &ms))) return rc;
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

}  // extern "C"
