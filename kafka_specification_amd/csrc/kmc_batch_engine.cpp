// kmc_batch_engine.cpp — batched successors and invariants of states given as data: kmc_successors_batch / kmc_precompile_batch
// over k_batch_count / k_batch_scan / k_batch_emit (kmc_batch.h), a code object of its own per configuration.  include/kmc.h
// holds the contract.  The seen-set, the frontiers and the search's control blocks are not touched.
#include "kmc_engine_internal.h"
using namespace kmc_engine;

namespace kmc_engine {

static void batch_free_staging(kmc_handle* h) {
    auto& b = h->batch;
    if (b.in) (void)hipFree(b.in);
    if (b.count) (void)hipFree(b.count);
    if (b.offsets) (void)hipFree(b.offsets);
    b.in = b.offsets = nullptr;
    b.count = nullptr;
    b.states_cap = 0;
}

void batch_release(kmc_handle* h) {
    auto& b = h->batch;
    batch_free_staging(h);
    if (b.rec) (void)hipFree(b.rec);
    b.rec = nullptr;
    b.rec_cap = 0;
    for (hipEvent_t& e : b.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    if (b.mod) (void)hipModuleUnload(b.mod);
    b.mod = nullptr;
    b.f_count = b.f_scan = b.f_emit = nullptr;
}

}  // namespace kmc_engine

// words of a handle's "enabled instances" bitset: max_fanout is the models' NINST
static uint32_t batch_nh(const kmc_handle* h) { return (uint32_t)((max_fanout(h) + 31) / 32); }

// the kernels' code object joins the handle (from the cache; a cold cache compiles it: kmc_precompile_batch), with its events
static int batch_ensure(kmc_handle* h) {
    auto& b = h->batch;
    if (!b.f_emit) {
        std::vector<char> code;
        std::string kname;
        int rc = get_code_object(h->cfg, h->arch, &code, &kname, nullptr, nullptr, KMC_CODEOBJ_BATCH, &h->knobs.jit_defines, h->knobs.layout_mode);
        if (rc) return rc;
        HIP_TRY(hipModuleLoadData(&b.mod, code.data()));
        HIP_TRY(hipModuleGetFunction(&b.f_count, b.mod, ("kmc_batch_count_" + h->kname).c_str()));
        HIP_TRY(hipModuleGetFunction(&b.f_scan, b.mod, ("kmc_batch_scan_" + h->kname).c_str()));
        HIP_TRY(hipModuleGetFunction(&b.f_emit, b.mod, ("kmc_batch_emit_" + h->kname).c_str()));
        // the grids are one resident wave of blocks, as k_expand's: the tiles are dealt round-robin, queued blocks only unbalance the tail
        int occ = 0;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, b.f_count, KMC_BLOCK, 0) == hipSuccess && occ > 0) b.occ_count = occ > 8 ? 8 : occ;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, b.f_emit, KMC_BLOCK, 0) == hipSuccess && occ > 0) b.occ_emit = occ > 8 ? 8 : occ;
    }
    for (hipEvent_t& e : b.ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    return KMC_OK;
}

// the staging of a launch of m states (kept; grown when a larger launch comes)
static int batch_stage(kmc_handle* h, uint64_t m) {
    auto& b = h->batch;
    if (m <= b.states_cap) return KMC_OK;
    batch_free_staging(h);
    const uint64_t in_bytes = m * h->W * 8, cnt_bytes = m * (2 + (uint64_t)batch_nh(h)) * 4, off_bytes = (m + 1 + KMC_BLOCK) * 8;
    if (hipMalloc(&b.in, in_bytes) != hipSuccess || hipMalloc(&b.count, cnt_bytes) != hipSuccess ||
        hipMalloc(&b.offsets, off_bytes) != hipSuccess) {
        (void)hipGetLastError();
        batch_free_staging(h);
        return fail(KMC_E_NOMEM, "staging of %llu states: %llu bytes", (unsigned long long)m, (unsigned long long)(in_bytes + cnt_bytes + off_bytes));
    }
    b.states_cap = m;
    return KMC_OK;
}

static int batch_launch(kmc_handle* h, hipFunction_t f, KmcBatchArgs a, uint64_t blocks) {
    size_t size = sizeof a;
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(f, (unsigned)blocks, 1, 1, KMC_BLOCK, 1, 1, 0, h->stream, nullptr, config));
    return KMC_OK;
}

extern "C" {

int kmc_precompile_batch(const kmc_config* cfg, const char* arch) {
    if (!cfg) return fail(KMC_E_ARG, "null config");
    if (cfg->model == KMC_ASYNC_ISR || cfg->symmetry) return fail(KMC_E_ARG, "the batch kernels are not for AsyncIsr or symmetry handles");
    std::vector<char> code;
    std::string kname;
    return get_code_object(*cfg, arch ? arch : "gfx950", &code, &kname, nullptr, nullptr, KMC_CODEOBJ_BATCH);
}

int kmc_successors_batch(kmc_handle* h, const kmc_batch_config* bc, const uint64_t* words, uint64_t n, uint64_t* offsets,
                         uint64_t* records, uint64_t cap_records, uint32_t* violated, kmc_batch_result* out) {
    if (!h || !bc || !offsets || !out || (n && !words)) return fail(KMC_E_ARG, "null argument");
    if (!records && cap_records) return fail(KMC_E_ARG, "cap_records = %llu without a record buffer", (unsigned long long)cap_records);
    if (h->cfg.model == KMC_ASYNC_ISR)
        return fail(KMC_E_ARG, "batched successors of AsyncIsr are not implemented: which successors outside the state constraint "
                               "count as candidates of a walk is undecided, and a batch's record order is a walk's numbering");
    if (h->cfg.symmetry) return fail(KMC_E_ARG, "a batch enumerates real states: kmc_successors is the way to enumerate under orbit counting");
    if (bc->states_per_launch > KMC_BATCH_MAX_STATES)
        return fail(KMC_E_ARG, "states_per_launch %u: at most 2^22", bc->states_per_launch);
    if (!h->table) return fail(KMC_E_STATE, "host-only handle: a batch runs on the device");
    const double t0 = now_s();
    kmc_batch_result r{};
    r.states = n;
    offsets[0] = 0;
    if (n == 0) {
        *out = r;
        return KMC_OK;
    }
    HIP_TRY(hipSetDevice(h->cfg.device));
    int rc = batch_ensure(h);
    if (rc) return rc;
    auto& b = h->batch;
    const uint64_t spl = bc->states_per_launch ? bc->states_per_launch : (1ull << 20);
    const uint64_t rw = (uint64_t)h->W + 2;
    double ms_kernel[3] = {0, 0, 0};   // count, scan, emit
    uint64_t base = 0;                 // records of the states before this launch
    for (uint64_t done = 0; done < n; done += spl) {
        const uint64_t m = n - done < spl ? n - done : spl;
        if ((rc = batch_stage(h, m))) return rc;
        KmcBatchArgs a{};
        a.in = b.in;
        a.count = b.count;
        a.violated = b.count + b.states_cap;
        a.bits = b.count + 2 * b.states_cap;
        a.stride = b.states_cap;
        a.offsets = b.offsets;
        a.sums = b.offsets + b.states_cap + 1;
        a.seed = h->cfg.hash_seed;
        a.n = (uint32_t)m;
        a.inv_mask = bc->inv_mask & 15u;
        a.nh = batch_nh(h);
        HIP_TRY(hipMemcpyAsync(b.in, words + done * h->W, m * h->W * 8, hipMemcpyHostToDevice, h->stream));
        // (a tuning build's KMC_BLOCKS_PER_CU overrides the residency, as for k_expand: the A/B of the grid)
        const int forced = tuning_blocks_per_cu(h);
        auto grid = [&](int per_cu) {
            const uint64_t all = (m + KMC_BLOCK - 1) / KMC_BLOCK, maxb = (uint64_t)h->n_cus * (uint64_t)(forced > 0 ? forced : per_cu);
            return all < maxb ? all : maxb;
        };
        const uint64_t scan_blocks = (m + KMC_BATCH_SCAN_CHUNK - 1) / KMC_BATCH_SCAN_CHUNK;
        HIP_TRY(hipEventRecord(b.ev[0], h->stream));
        if ((rc = batch_launch(h, b.f_count, a, grid(b.occ_count)))) return rc;
        HIP_TRY(hipEventRecord(b.ev[1], h->stream));
        a.phase = 0;
        if ((rc = batch_launch(h, b.f_scan, a, scan_blocks))) return rc;
        a.phase = 1;
        if ((rc = batch_launch(h, b.f_scan, a, scan_blocks))) return rc;
        HIP_TRY(hipEventRecord(b.ev[2], h->stream));
        // the launch's offsets land in the caller's array (its last entry is the next launch's first) and get the launch's base
        HIP_TRY(hipMemcpyAsync(offsets + done, b.offsets, (m + 1) * 8, hipMemcpyDeviceToHost, h->stream));
        if (violated) HIP_TRY(hipMemcpyAsync(violated + done, a.violated, m * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
        ms_kernel[0] += ms;
        HIP_TRY(hipEventElapsedTime(&ms, b.ev[1], b.ev[2]));
        ms_kernel[1] += ms;
        uint64_t* off = offsets + done;
        const uint64_t total = off[m];
        // the records of this launch that are handed out: the runs that lie wholly below cap_records
        uint64_t take = 0;
        if (records && base < cap_records) {
            const uint64_t room = cap_records - base;
            if (total <= room) {
                take = total;
            } else {   // the last state whose run ends within the room
                uint64_t lo = 0, hi = m;   // off[lo] <= room < off[hi]
                while (hi - lo > 1) {
                    const uint64_t mid = (lo + hi) / 2;
                    if (off[mid] <= room) lo = mid;
                    else hi = mid;
                }
                take = off[lo];
            }
        }
        if (take) {
            if (take > b.rec_cap) {
                if (b.rec) (void)hipFree(b.rec);
                b.rec = nullptr;
                b.rec_cap = 0;
                if (hipMalloc(&b.rec, take * rw * 8) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(KMC_E_NOMEM, "record staging of %llu bytes", (unsigned long long)(take * rw * 8));
                }
                b.rec_cap = take;
            }
            a.rec = b.rec;
            a.cap = take;
            HIP_TRY(hipEventRecord(b.ev[3], h->stream));
            if ((rc = batch_launch(h, b.f_emit, a, grid(b.occ_emit)))) return rc;
            HIP_TRY(hipEventRecord(b.ev[4], h->stream));
            HIP_TRY(hipMemcpyAsync(records + base * rw, b.rec, take * rw * 8, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            HIP_TRY(hipEventElapsedTime(&ms, b.ev[3], b.ev[4]));
            ms_kernel[2] += ms;
        }
        if (base)
            for (uint64_t i = 0; i <= m; ++i) off[i] += base;
        base += total;
        r.launches += 1;
    }
    r.records = base;
    r.seconds_count = ms_kernel[0] * 1e-3;
    r.seconds_scan = ms_kernel[1] * 1e-3;
    r.seconds_emit = ms_kernel[2] * 1e-3;
    r.seconds_kernel = r.seconds_count + r.seconds_scan + r.seconds_emit;
    r.seconds_total = now_s() - t0;
    *out = r;
    return KMC_OK;
}

}  // extern "C"
