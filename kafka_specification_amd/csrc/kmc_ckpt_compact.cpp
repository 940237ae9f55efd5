// kmc_ckpt_compact.cpp — the compact checkpoint's table part: the seen-set goes to the file as its entries and their index
// (kmc_pack_*), and comes back into a table of any sufficient size (kmc_unpack_window, kmc_rehash_overflow); kmc_compact.h has
// the kernels, kmc_engine_step.cpp the header, the frontier and everything both formats share.  DESIGN.md §8c.
//
// In the file, behind the init state, stretch by stretch: the stretch's index (one word per tile of KMC_COMPACT_TILE groups: the
// entries before it in the stretch; then the stretch's total), then its entries.  A stretch is what the staging holds, so save
// and load stream through one bounded pinned buffer and one device buffer of the same size.
#include "kmc_engine_internal.h"
using namespace kmc_engine;

namespace {

constexpr uint64_t STAGE_WORDS = 1ull << 24;   // 128 MiB of entries per stretch at the most (as the classic format's pieces)
constexpr uint64_t T = KMC_COMPACT_TILE;

uint64_t round_up(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }

// device and pinned staging of one stretch: the entries first (16-byte aligned), the index behind them
struct Staging {
    u64* dev = nullptr;
    uint64_t* host = nullptr;
    uint64_t entry_slots = 0;   // entries it holds
    uint64_t ew = 0;
    u64* dev_index() const { return dev + entry_slots * ew; }
    uint64_t* host_index() const { return host + entry_slots * ew; }
    int open(uint64_t groups, uint64_t entry_words) {
        entry_slots = groups * 64;
        ew = entry_words;
        const size_t bytes = (entry_slots * ew + groups / T + 2) * 8;
        if (hipMalloc(&dev, bytes) != hipSuccess || hipHostMalloc(&host, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(KMC_E_NOMEM, "checkpoint: cannot allocate %zu bytes of staging", bytes);
        }
        return KMC_OK;
    }
    ~Staging() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
    }
};

int launch_compact(kmc_handle* h, hipFunction_t f, KmcCompactArgs c, uint64_t blocks, unsigned lds) {
    const uint64_t most = (uint64_t)h->n_cus * 8;
    blocks = blocks < 1 ? 1 : blocks > most ? most : blocks;
    size_t size = sizeof c;
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &c, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(f, (unsigned)blocks, 1, 1, KMC_REHASH_BLOCK, 1, 1, lds, h->stream, nullptr, config));
    return KMC_OK;
}

int launch_overflow(kmc_handle* h, KmcRehashArgs a, uint64_t entries) {
    const uint64_t most = (uint64_t)h->n_cus * 8;
    uint64_t blocks = (entries + KMC_REHASH_BLOCK - 1) / KMC_REHASH_BLOCK;
    blocks = blocks < 1 ? 1 : blocks > most ? most : blocks;
    size_t size = sizeof a;
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(h->growth.f_overflow, (unsigned)blocks, 1, 1, KMC_REHASH_BLOCK, 1, 1, 0, h->stream, nullptr, config));
    return KMC_OK;
}

// the stream's work since ev_aux[0] was recorded, in milliseconds; called behind a wait for the stream
int kernel_ms_since(kmc_handle* h, CkptClock* clk) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_aux[0], h->ev_aux[1]));
    clk->kernel_ms += ms;
    return KMC_OK;
}

int read_ctl_block(kmc_handle* h) {
    HIP_TRY(hipMemcpyAsync(h->growth.ctl_host, h->growth.ctl, sizeof(KmcRehashCtl), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return KMC_OK;
}

// Old groups per tile-run, a multiple of the tile, such that the floor(span G'/G) + 1 new groups a run may own fit the window
// (and *win_slots, the window's slots); 0: the ratio leaves no such run, the table is built by scatter.
uint64_t unpack_span(const kmc_handle* h, uint64_t G, uint64_t G2, u64* win_slots) {
    const uint64_t win_groups = h->growth.window_bytes / (64 * 8 * entry_words(h));
    *win_slots = win_groups * 64;
    if (win_groups < 2) return 0;
    const uint64_t span = (uint64_t)((unsigned __int128)(win_groups - 1) * G / G2) / T * T;
    if (span < T && G <= T && G2 <= win_groups) return T;   // (one run is the whole table)
    return span;
}

}  // namespace

namespace kmc_engine {

CkptCompact compact_describe(const kmc_handle* h) {
    CkptCompact ch{};
    ch.n_entries = h->res.orbit_representatives;
    ch.entry_words = entry_words(h);
    ch.tile = T;
    const uint64_t fit = STAGE_WORDS / (64 * ch.entry_words) / T * T, all = round_up(h->table_cap >> 6, T);
    ch.stretch_groups = fit < all ? fit : all;
    return ch;
}

int compact_save_table(kmc_handle* h, FILE* f, const CkptCompact& ch, CkptClock* clk) {
    int rc = table_kernels_ensure(h);
    if (rc) return rc;
    kmc_growth& g = h->growth;
    Staging st;
    if ((rc = st.open(ch.stretch_groups, ch.entry_words))) return rc;
    KmcCompactArgs c{};
    c.r.old_tab = h->table;
    c.r.old_pred = separate_pred(h) ? h->pred : nullptr;
    c.r.old_cap = h->table_cap;
    c.r.ctl = g.ctl;
    c.index = st.dev_index();
    c.entries = st.dev;
    c.entries_cap = st.entry_slots;
    const uint64_t G = h->table_cap >> 6;
    uint64_t total = 0;
    if (!h->ev_aux[0]) {
        HIP_TRY(hipEventCreate(&h->ev_aux[0]));
        HIP_TRY(hipEventCreate(&h->ev_aux[1]));
    }
    HIP_TRY(hipMemsetAsync(g.ctl, 0, sizeof(KmcRehashCtl), h->stream));
    for (uint64_t g0 = 0; g0 < G; g0 += ch.stretch_groups) {
        c.g_first = g0;
        c.g_end = g0 + ch.stretch_groups < G ? g0 + ch.stretch_groups : G;
        const uint64_t tiles = (c.g_end - c.g_first + T - 1) / T;
        const double t0 = now_s();
        HIP_TRY(hipEventRecord(h->ev_aux[0], h->stream));
        if ((rc = launch_compact(h, g.f_pack_count, c, tiles, 0))) return rc;
        if ((rc = launch_compact(h, g.f_pack_scan, c, 1, 0))) return rc;
        if ((rc = launch_compact(h, g.f_pack_write, c, tiles, 0))) return rc;
        HIP_TRY(hipEventRecord(h->ev_aux[1], h->stream));
        HIP_TRY(hipMemcpyAsync(st.host_index(), st.dev_index(), (tiles + 1) * 8, hipMemcpyDeviceToHost, h->stream));
        if ((rc = read_ctl_block(h)) || (rc = kernel_ms_since(h, clk))) return rc;
        const uint64_t n = st.host_index()[tiles];
        if (g.ctl_host->err || n > st.entry_slots)
            return fail(KMC_E_DEVICE, "checkpoint: packing the seen-set reported error flags %u", g.ctl_host->err);
        if (n) HIP_TRY(hipMemcpyAsync(st.host, st.dev, n * ch.entry_words * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const double t1 = now_s();
        if (fwrite(st.host_index(), 8, tiles + 1, f) != tiles + 1 || fwrite(st.host, 8, n * ch.entry_words, f) != n * ch.entry_words)
            return fail(KMC_E_STATE, "checkpoint: short write");
        clk->copy_s += t1 - t0;   // (with the kernels' time, which the copies wait for: kernel_ms says how much of it)
        clk->io_s += now_s() - t1;
        total += n;
    }
    // Conservation: what went to the file must be what the search has stored
    if (total != ch.n_entries || g.ctl_host->placed_global != total)
        return fail(KMC_E_DEVICE, "checkpoint: %llu entries were counted and %llu packed but %llu states are stored",
                    (unsigned long long)total, (unsigned long long)g.ctl_host->placed_global, (unsigned long long)ch.n_entries);
    return KMC_OK;
}

int compact_check_header(const kmc_handle* h, const CkptCompact& ch, uint64_t saved_cap) {
    if (ch.tile != T || ch.entry_words != entry_words(h) || saved_cap == 0 || saved_cap % 64 || saved_cap >> 6 > 0xFFFFFFFFull ||
        ch.stretch_groups == 0 || ch.stretch_groups % T || ch.stretch_groups * 64 * ch.entry_words > STAGE_WORDS || ch.n_entries > saved_cap)
        return fail(KMC_E_ARG, "compact checkpoint header is inconsistent (tile %llu, %llu words per entry where this handle has %llu, "
                               "%llu entries of a table of %llu slots, stretches of %llu groups)",
                    (unsigned long long)ch.tile, (unsigned long long)ch.entry_words, (unsigned long long)entry_words(h),
                    (unsigned long long)ch.n_entries, (unsigned long long)saved_cap, (unsigned long long)ch.stretch_groups);
    if ((double)ch.n_entries > KMC_TABLE_LOAD_LIMIT * (double)h->table_cap) {
        uint64_t need = round_up((uint64_t)((double)ch.n_entries / KMC_TABLE_LOAD_LIMIT), 64);
        while ((double)ch.n_entries > KMC_TABLE_LOAD_LIMIT * (double)need) need += 64;
        return fail(KMC_E_ARG, "the checkpoint's %llu entries do not fit a table of %llu slots below load %.2f: open the handle with "
                               "table_capacity=%llu or more (or enable table growth before the search needs more)",
                    (unsigned long long)ch.n_entries, (unsigned long long)h->table_cap, KMC_TABLE_LOAD_LIMIT, (unsigned long long)need);
    }
    return KMC_OK;
}

int compact_load_table(kmc_handle* h, FILE* f, const CkptCompact& ch, uint64_t saved_cap, CkptClock* clk) {
    int rc = table_kernels_ensure(h);
    if (rc) return rc;
    kmc_growth& g = h->growth;
    const uint64_t G = saved_cap >> 6, G2 = h->table_cap >> 6, ew = ch.entry_words;
    const uint64_t sg = ch.stretch_groups < round_up(G, T) ? ch.stretch_groups : round_up(G, T);
    Staging st;
    if ((rc = st.open(sg, ew))) return rc;
    KmcCompactArgs c{};
    KmcRehashArgs& a = c.r;
    a.new_tab = h->table;
    a.new_pred = separate_pred(h) ? h->pred : nullptr;
    a.old_cap = saved_cap;
    a.new_cap = h->table_cap;
    a.list = h->frontier[1];   // both frontiers are idle until the saved one is read (into frontier[0], behind the table)
    a.list_cap = h->fcap * (uint64_t)h->planes / ew;
    a.ctl = g.ctl;
    a.span = unpack_span(h, G, G2, &a.win_slots);
    c.index = st.dev_index();
    c.entries = st.dev;
    bool windowed = g.kernel == 0 && a.span >= T;
    const long table_at = ftell(f);
    if (table_at < 0) return fail(KMC_E_STATE, "checkpoint: cannot tell the position in the file");
    uint64_t total = 0;
    for (;;) {
        HIP_TRY(hipMemsetAsync(g.ctl, 0, sizeof(KmcRehashCtl), h->stream));
        if (!windowed) {   // the scatter form: a cleared table, every entry claimed by global compare-and-swap
            HIP_TRY(hipMemsetAsync(h->table, 0, h->table_cap * h->stride_words() * 8, h->stream));
            if (a.new_pred) HIP_TRY(hipMemsetAsync(a.new_pred, 0, h->table_cap * 8, h->stream));
        }
        if (fseek(f, table_at, SEEK_SET) != 0) return fail(KMC_E_STATE, "checkpoint: cannot seek");
        total = 0;
        for (uint64_t g0 = 0; g0 < G; g0 += ch.stretch_groups) {
            c.g_first = g0;
            c.g_end = g0 + ch.stretch_groups < G ? g0 + ch.stretch_groups : G;
            const uint64_t tiles = (c.g_end - c.g_first + T - 1) / T;
            uint64_t* const ix = st.host_index();
            const double t0 = now_s();
            if (fread(ix, 8, tiles + 1, f) != tiles + 1) return fail(KMC_E_STATE, "checkpoint: short read");
            // the index is checked before it addresses anything: it begins at 0, a tile adds at most its slots, the total fits
            bool sane = ix[0] == 0;
            for (uint64_t t = 0; t < tiles && sane; ++t) sane = ix[t + 1] >= ix[t] && ix[t + 1] - ix[t] <= T * 64;
            const uint64_t n = ix[tiles];
            if (!sane || n > st.entry_slots || total + n > ch.n_entries)
                return fail(KMC_E_ARG, "checkpoint: the index of the stretch at group %llu is inconsistent", (unsigned long long)g0);
            if (fread(st.host, 8, n * ew, f) != n * ew) return fail(KMC_E_STATE, "checkpoint: short read");
            total += n;
            c.entries_cap = n;
            const double t1 = now_s();
            if (n) HIP_TRY(hipMemcpyAsync(st.dev, st.host, n * ew * 8, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(st.dev_index(), ix, (tiles + 1) * 8, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipEventRecord(h->ev_aux[0], h->stream));
            if (windowed) {
                const uint64_t runs = (c.g_end - c.g_first + a.span - 1) / a.span;
                const uint64_t per_cu = (160 * 1024 - 1024) / g.window_bytes;   // workgroups a CU's LDS holds
                const uint64_t grid = (uint64_t)h->n_cus * (per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu);
                if ((rc = launch_compact(h, g.f_unpack, c, runs < grid ? runs : grid, (unsigned)(a.win_slots * ew * 8)))) return rc;
            } else {       // the stretch's entries are the list (ix[tiles] still holds n: the staging is not touched before the wait below)
                KmcRehashArgs s = a;
                s.list = st.dev;
                s.list_cap = n;
                HIP_TRY(hipMemcpyAsync(&g.ctl->listed.v, &ix[tiles], 8, hipMemcpyHostToDevice, h->stream));
                if ((rc = launch_overflow(h, s, n))) return rc;
            }
            HIP_TRY(hipEventRecord(h->ev_aux[1], h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));   // the staging is free for the next stretch
            if ((rc = kernel_ms_since(h, clk))) return rc;
            clk->io_s += t1 - t0;
            clk->copy_s += now_s() - t1;   // (with the kernels' time: kernel_ms says how much of it)
        }
        HIP_TRY(hipEventRecord(h->ev_aux[0], h->stream));
        if (windowed && (rc = launch_overflow(h, a, a.list_cap < ch.n_entries ? a.list_cap : ch.n_entries))) return rc;
        HIP_TRY(hipEventRecord(h->ev_aux[1], h->stream));
        if ((rc = read_ctl_block(h)) || (rc = kernel_ms_since(h, clk))) return rc;
        if (windowed && (g.ctl_host->err & KMC_REHASH_ERR_LIST_FULL)) {   // every slot is rewritten: once more, the plain way
            windowed = false;
            continue;
        }
        break;
    }
    const KmcRehashCtl& k = *g.ctl_host;
    if (total != ch.n_entries)
        return fail(KMC_E_ARG, "checkpoint: the stretches hold %llu entries, the header says %llu", (unsigned long long)total, (unsigned long long)ch.n_entries);
    if (k.err)
        return fail(KMC_E_DEVICE, "checkpoint: rebuilding the seen-set in %llu slots reported error flags %u", (unsigned long long)h->table_cap, k.err);
    // Conservation: what the table holds now must be what the file's search had stored
    if (k.placed_window + k.placed_global != ch.n_entries || ch.n_entries != h->res.orbit_representatives)
        return fail(KMC_E_DEVICE, "checkpoint: %llu entries were placed (%llu by the windows) but the file holds %llu and its search had stored %llu",
                    (unsigned long long)(k.placed_window + k.placed_global), (unsigned long long)k.placed_window,
                    (unsigned long long)ch.n_entries, (unsigned long long)h->res.orbit_representatives);
    if (h->knobs.verbose)
        fprintf(stderr, "[kmc] compact checkpoint: %llu entries of a table of %llu slots rebuilt in %llu slots, %s (%llu by global claims)\n",
                (unsigned long long)ch.n_entries, (unsigned long long)saved_cap, (unsigned long long)h->table_cap,
                windowed ? "windowed" : "scatter", (unsigned long long)k.placed_global);
    return KMC_OK;
}

}  // namespace kmc_engine

extern "C" int kmc_checkpoint_save_compact(kmc_handle* h, const char* path) { return checkpoint_save(h, path, true); }
