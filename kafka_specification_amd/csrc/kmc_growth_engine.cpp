// kmc_growth_engine.cpp — the growing seen-set: kmc_table_growth_enable / kmc_table_growth_stats / kmc_precompile_table, the two rules
// that say when and how far (grow_if_needed, called by run_levels between two levels), and the launches of kmc_rehash.h's
// kernels.  DESIGN.md §8b.  A handle that never asks for growth runs none of this.
#include "kmc_engine_internal.h"
using namespace kmc_engine;

namespace kmc_engine {

void growth_release(kmc_handle* h) {
    kmc_growth& g = h->growth;
    if (g.ctl) (void)hipFree(g.ctl);
    if (g.ctl_host) (void)hipHostFree(g.ctl_host);
    if (g.mod) (void)hipModuleUnload(g.mod);
    g.ctl = g.ctl_host = nullptr;
    g.mod = nullptr;
    g.f_window = g.f_overflow = g.f_scatter = nullptr;
    g.f_pack_count = g.f_pack_scan = g.f_pack_write = g.f_unpack = nullptr;
}

int table_kernels_ensure(kmc_handle* h) {
    kmc_growth& g = h->growth;
    if (!g.f_window) {
        std::vector<char> code;
        int rc = get_table_code_object(h->cfg.cache_dir, h->arch, &code);
        if (rc) return rc;
        HIP_TRY(hipModuleLoadData(&g.mod, code.data()));
        const std::string tag = std::string(h->stride_words() == 2 ? "2" : "1") + (separate_pred(h) ? "p" : "n");
        HIP_TRY(hipModuleGetFunction(&g.f_window, g.mod, ("kmc_rehash_window_" + tag).c_str()));
        HIP_TRY(hipModuleGetFunction(&g.f_overflow, g.mod, ("kmc_rehash_overflow_" + tag).c_str()));
        HIP_TRY(hipModuleGetFunction(&g.f_scatter, g.mod, ("kmc_rehash_scatter_" + tag).c_str()));
        HIP_TRY(hipModuleGetFunction(&g.f_pack_count, g.mod, ("kmc_pack_count_" + tag).c_str()));
        HIP_TRY(hipModuleGetFunction(&g.f_pack_scan, g.mod, "kmc_pack_scan"));
        HIP_TRY(hipModuleGetFunction(&g.f_pack_write, g.mod, ("kmc_pack_write_" + tag).c_str()));
        HIP_TRY(hipModuleGetFunction(&g.f_unpack, g.mod, ("kmc_unpack_window_" + tag).c_str()));
        // (more than 64 KiB of dynamic LDS has to be asked for; a window the device refuses is an error, never another size)
        if (g.window_bytes > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)g.f_window, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.window_bytes);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)g.f_unpack, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.window_bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                (void)hipModuleUnload(g.mod);
                g.mod = nullptr;
                g.f_window = nullptr;   // (asked again, and refused again, at the next growth)
                return fail(KMC_E_ARG, "KMC_REHASH_WINDOW_KIB=%llu: the device refuses a window of that size (%s)",
                            (unsigned long long)(g.window_bytes >> 10), hipGetErrorString(e));
            }
        }
    }
    if (!g.ctl) HIP_TRY(hipMalloc(&g.ctl, sizeof(KmcRehashCtl)));
    if (!g.ctl_host) HIP_TRY(hipHostMalloc(&g.ctl_host, sizeof(KmcRehashCtl)));
    return KMC_OK;
}

}  // namespace kmc_engine

static int rehash_launch(kmc_handle* h, hipFunction_t f, KmcRehashArgs a, uint64_t blocks, unsigned lds) {
    if (blocks < 1) blocks = 1;
    size_t size = sizeof a;
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(f, (unsigned)blocks, 1, 1, KMC_REHASH_BLOCK, 1, 1, lds, h->stream, nullptr, config));
    return KMC_OK;
}

// Old groups per tile of the windowed kernel, and the slots of LDS a window may take: a tile of `span` old groups owns at most
// floor(span G'/G) + 1 new groups, which must fit the window.  0: not even one group fits (the ratio of this growth is too large).
static uint64_t window_span(const kmc_handle* h, uint64_t old_cap, uint64_t new_cap, u64* win_slots) {
    const uint64_t win_groups = h->growth.window_bytes / (64 * 8 * entry_words(h));
    *win_slots = win_groups * 64;
    if (win_groups < 2) return 0;
    const unsigned __int128 span = (unsigned __int128)(win_groups - 1) * (old_cap >> 6) / (new_cap >> 6);
    return (uint64_t)span;
}

// Every entry of the current table (and predecessor table) is carried into nt / np of new_cap slots; st->kernel says which kernel
// ran (the windowed one falls back to scatter when its list overflows or the ratio of this growth leaves no window a whole group).
static int rehash(kmc_handle* h, u64* nt, u64* np, uint64_t new_cap, kmc_growth_stat* st) {
    kmc_growth& g = h->growth;
    KmcRehashArgs a{};
    a.old_tab = h->table;
    a.old_pred = separate_pred(h) ? h->pred : nullptr;
    a.new_tab = nt;
    a.new_pred = np;
    a.old_cap = h->table_cap;
    a.new_cap = new_cap;
    a.list = h->frontier[h->cur ^ 1];   // idle at a level boundary
    a.list_cap = h->fcap * (uint64_t)h->planes / entry_words(h);
    a.ctl = g.ctl;
    a.span = window_span(h, a.old_cap, a.new_cap, &a.win_slots);
    int kernel = g.kernel == 0 && a.span >= 1 ? 0 : 1;
    const uint64_t resident = (uint64_t)h->n_cus * 8;
    int rc = KMC_OK;
    if (!h->ev_aux[0]) {
        HIP_TRY(hipEventCreate(&h->ev_aux[0]));
        HIP_TRY(hipEventCreate(&h->ev_aux[1]));
    }
    for (;;) {
        HIP_TRY(hipMemsetAsync(g.ctl, 0, sizeof(KmcRehashCtl), h->stream));
        HIP_TRY(hipEventRecord(h->ev_aux[0], h->stream));
        if (kernel == 0) {
            const uint64_t tiles = ((a.old_cap >> 6) + a.span - 1) / a.span;
            const uint64_t per_cu = (160 * 1024 - 1024) / g.window_bytes;   // workgroups a CU's LDS holds
            const uint64_t grid = (uint64_t)h->n_cus * (per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu);
            if ((rc = rehash_launch(h, g.f_window, a, tiles < grid ? tiles : grid, (unsigned)(a.win_slots * entry_words(h) * 8)))) return rc;
            const uint64_t most = a.list_cap < a.old_cap ? a.list_cap : a.old_cap;
            const uint64_t blocks = (most + KMC_REHASH_BLOCK - 1) / KMC_REHASH_BLOCK;
            if ((rc = rehash_launch(h, g.f_overflow, a, blocks < resident ? blocks : resident, 0))) return rc;
        } else {
            HIP_TRY(hipMemsetAsync(nt, 0, new_cap * h->stride_words() * 8, h->stream));
            if (np) HIP_TRY(hipMemsetAsync(np, 0, new_cap * 8, h->stream));
            const uint64_t blocks = (a.old_cap + KMC_REHASH_BLOCK - 1) / KMC_REHASH_BLOCK;
            if ((rc = rehash_launch(h, g.f_scatter, a, blocks < resident ? blocks : resident, 0))) return rc;
        }
        HIP_TRY(hipEventRecord(h->ev_aux[1], h->stream));
        HIP_TRY(hipMemcpyAsync(g.ctl_host, g.ctl, sizeof(KmcRehashCtl), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev_aux[0], h->ev_aux[1]));
        st->rehash_ms += ms;
        if (kernel == 0 && (g.ctl_host->err & KMC_REHASH_ERR_LIST_FULL)) {   // the old table is untouched: once more, the plain way
            kernel = 1;
            continue;
        }
        break;
    }
    const KmcRehashCtl& c = *g.ctl_host;
    st->kernel = kernel;
    st->overflow = kernel == 0 ? c.placed_global : 0;
    st->moved = c.placed_window + c.placed_global;
    if (c.err)
        return fail(KMC_E_DEVICE, "growing the seen-set from %llu to %llu slots: the rehash reported error flags %u",
                    (unsigned long long)a.old_cap, (unsigned long long)new_cap, c.err);
    return KMC_OK;
}

namespace kmc_engine {

int grow_if_needed(kmc_handle* h) {
    kmc_growth& g = h->growth;
    kmc_result& r = h->res;
    const uint64_t stored = r.orbit_representatives;
    // the next level adds at most this many states (the bound of run_levels' chain planner)
    const uint64_t fan = max_fanout(h) ? max_fanout(h) : 1;
    const uint64_t bound = h->n_cur > h->fcap / fan ? h->fcap : h->n_cur * fan;
    const uint64_t safe = (uint64_t)((double)(stored + bound) / KMC_TABLE_LOAD_LIMIT) + 1;   // slots at which the level provably fits
    const bool by_load = (double)stored > 0.5 * (double)h->table_cap;
    const bool by_safety = safe > h->table_cap;
    if (!by_load && !by_safety) return KMC_OK;
    // how far: both rules at once (a table grown for the next level alone would be grown again by the load rule right after it)
    const uint64_t eb = entry_words(h) * 8;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    uint64_t most = (uint64_t)(0.85 * (double)free_b) / eb;   // ... while the old table still exists
    if (g.max_slots && most > g.max_slots) most = g.max_slots;
    if (most >> 6 > 0xFFFFFFFFull) most = 0xFFFFFFFFull << 6;
    most = most / 64 * 64;
    auto fit = [&](uint64_t want) { want = (want + 63) / 64 * 64; return want > most ? most : want; };
    // ... and never by less than a doubling: the safety rule's bound is loose (every state enabling every action instance), so
    // level after level it asks for a little more than the last time, and what a growth costs is mostly its allocation
    uint64_t want = 4 * stored > safe ? 4 * stored : safe;
    if (want < 2 * h->table_cap) want = 2 * h->table_cap;
    uint64_t tries[2] = {fit(want), fit(safe)};
    int rc = table_kernels_ensure(h);
    if (rc) return rc;
    for (int k = 0; k < 2; ++k) {
        const uint64_t new_cap = tries[k];
        if (new_cap <= h->table_cap || (k == 1 && new_cap == tries[0])) continue;
        const double t0 = now_s();
        u64* nt = seen_set_alloc(h, new_cap * h->stride_words() * 8);
        u64* np = nt && separate_pred(h) ? seen_set_alloc(h, new_cap * 8) : nullptr;
        if (!nt || (separate_pred(h) && !np)) {   // no room: once more at the least the next level needs, else go on as it is
            seen_set_free(h, nt);
            (void)hipGetLastError();
            continue;
        }
        kmc_growth_stat st{};
        st.depth = h->level;
        st.old_slots = h->table_cap;
        st.new_slots = new_cap;
        const double t1 = now_s();
        if ((rc = rehash(h, nt, np, new_cap, &st))) {
            const std::string keep = g_err;   // (the new tables go back; the old ones stay the handle's)
            (void)hipStreamSynchronize(h->stream);
            seen_set_free(h, nt);
            seen_set_free(h, np);
            g_err = keep;
            r.verdict = KMC_V_ERROR;
            return rc;
        }
        g.stats.push_back(st);
        // Conservation: what the new table holds must be what the search has stored
        if (st.moved != stored) {
            seen_set_free(h, nt);
            seen_set_free(h, np);
            r.verdict = KMC_V_ERROR;
            return fail(KMC_E_DEVICE, "growing the seen-set at depth %llu (%llu -> %llu slots): %llu entries were carried over but %llu "
                                      "states are stored: the rehash lost or invented entries", (unsigned long long)h->level,
                        (unsigned long long)st.old_slots, (unsigned long long)new_cap, (unsigned long long)st.moved, (unsigned long long)stored);
        }
        // the rehash has completed on the stream (rehash waits for its counters): the old tables go back
        u64* const old_t = h->table;
        u64* const old_p = separate_pred(h) ? h->pred : nullptr;
        h->table = nt;
        h->pred = h->paired ? nt + 1 : np ? np : h->pred;
        h->table_cap = new_cap;
        r.table_capacity = new_cap;
        const double t2 = now_s();
        seen_set_free(h, old_t);
        seen_set_free(h, old_p);
        if (h->knobs.verbose)
            fprintf(stderr, "[kmc] seen-set grown at depth %llu: %llu -> %llu slots, %llu entries (%llu by the second phase), %s kernel (window %llu KiB) %.3f ms; "
                            "on the host: allocation %.3f ms, rehash with its wait %.3f ms, release of the old tables %.3f ms\n",
                    (unsigned long long)st.depth, (unsigned long long)st.old_slots, (unsigned long long)new_cap, (unsigned long long)st.moved,
                    (unsigned long long)st.overflow, st.kernel ? "scatter" : "windowed", (unsigned long long)(g.window_bytes >> 10), st.rehash_ms,
                    1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (now_s() - t2));
        return KMC_OK;
    }
    return KMC_OK;   // nothing larger can be had: the search goes on in the table it has
}

}  // namespace kmc_engine

extern "C" {

int kmc_precompile_table(const char* arch) {
    std::vector<char> code;
    return get_table_code_object(nullptr, arch ? arch : "gfx950", &code);
}

int kmc_table_code_object_path(const char* arch, char* out, uint64_t cap) {
    if (!out || !cap) return fail(KMC_E_ARG, "null buffer");
    std::vector<char> code;
    std::string path;
    int rc = get_table_code_object(nullptr, arch ? arch : "gfx950", &code, &path);
    if (rc) return rc;
    if (path.size() + 1 > cap) return fail(KMC_E_ARG, "path of %zu bytes does not fit %llu", path.size(), (unsigned long long)cap);
    memcpy(out, path.c_str(), path.size() + 1);
    return KMC_OK;
}

int kmc_table_growth_enable(kmc_handle* h, uint64_t max_slots) {
    if (!h) return fail(KMC_E_ARG, "null handle");
    if (!h->table) return fail(KMC_E_ARG, "host-only handle (device = -1): there is no seen-set to grow");
    if (h->cfg.n_shards != 1) return fail(KMC_E_ARG, "table growth is for one GPU (n_shards = %d): a shard keeps the table it was opened with", h->cfg.n_shards);
    if (h->stepping) return fail(KMC_E_STATE, "table growth belongs to kmc_run / kmc_resume, not to the level-step interface");
    if (h->level || h->restored)
        return fail(KMC_E_STATE, "kmc_table_growth_enable comes right after kmc_open: this handle already holds a search or a loaded checkpoint");
    if (tuning_unchained(h)) return fail(KMC_E_STATE, "table growth and the tuning aids' level-by-level passes do not go together");
    if (max_slots && max_slots < h->table_cap)
        return fail(KMC_E_ARG, "max_slots %llu is below the %llu slots the handle was opened with", (unsigned long long)max_slots, (unsigned long long)h->table_cap);
    kmc_growth& g = h->growth;
    // the two knobs of growth, read once per handle, here: README "Growing the seen-set"
    const char* k = env_str("KMC_REHASH", "window");
    if (strcmp(k, "window") && strcmp(k, "scatter")) return fail(KMC_E_ARG, "KMC_REHASH=%s: expected window or scatter", k);
    g.kernel = !strcmp(k, "scatter");
    const long long kib = env_int("KMC_REHASH_WINDOW_KIB", 32);
    if (kib < 4 || kib > 159) return fail(KMC_E_ARG, "KMC_REHASH_WINDOW_KIB=%lld: a window takes between 4 and 159 KiB of LDS", kib);
    g.window_bytes = (uint64_t)kib * 1024;
    if (g.mod) growth_release(h);   // (joined by a checkpoint before this call: it joins again, its LDS limit raised for this window)
    g.max_slots = max_slots / 64 * 64;
    // Frontiers that kmc_open sized by itself were clipped to the table (a level cannot outgrow the seen-set): a growing handle's
    // are sized as beside an automatic table (auto_frontier_capacity, kmc_engine_open.cpp) or the level that no
    // longer fills the table would end the search with KMC_V_FRONTIER_FULL instead.
    if (h->cfg.frontier_capacity == 0) {
        HIP_TRY(hipSetDevice(h->cfg.device));
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const uint64_t fcap = auto_frontier_capacity(h, 0.85 * (double)free_b);
        if (fcap > h->fcap) {
            u64* f[2] = {nullptr, nullptr};
            for (int i = 0; i < 2; ++i)
                if (hipMalloc(&f[i], fcap * 8ull * h->planes) != hipSuccess) {
                    (void)hipFree(f[0]);
                    return fail(KMC_E_NOMEM, "cannot allocate frontier of %llu states", (unsigned long long)fcap);
                }
            HIP_TRY(hipStreamSynchronize(h->stream));
            for (int i = 0; i < 2; ++i) {
                (void)hipFree(h->frontier[i]);
                h->frontier[i] = f[i];
            }
            h->fcap = fcap;
            h->seg_cap = fcap / KMC_SEGS;
        }
    }
    g.enabled = true;
    return KMC_OK;
}

uint64_t kmc_table_growth_stats(kmc_handle* h, kmc_growth_stat* out, uint64_t cap) {
    if (!h) return 0;
    for (uint64_t i = 0; out && i < h->growth.stats.size() && i < cap; ++i) out[i] = h->growth.stats[i];
    return h->growth.stats.size();
}

}  // extern "C"
