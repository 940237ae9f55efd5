// kmc_engine_tuning.cpp — the tuning aids of the level loop (README: "Tuning build").  Compiled only with -DKMC_TUNING=1, the macro of
// the device's tuning build, into libkmc_tuning.so: libkmc.so has none of this and reads none of these variables (kmc_engine_internal.h
// holds the no-ops).  The dry and shadow passes also need the device's half, a code object built with KMC_JIT_DEFINES=-DKMC_TUNING=1.
#if !KMC_TUNING
#error "kmc_engine_tuning.cpp belongs to the tuning build only (-DKMC_TUNING=1)"
#endif
#include "kmc_engine_internal.h"

namespace kmc_engine {

void tuning_open(kmc_handle* h) {   // like the handle's knobs: read once, when the handle is opened
    kmc_tuning& t = h->tuning;
    t.shadow = (int)env_int("KMC_SHADOW", 0);          // every level first runs on a copy of the seen-set ...
    t.xflags = (uint32_t)env_int("KMC_XFLAGS", 0);     // ... with these KMC_FLAG_X_* ablations applied
    t.dry_mode = (int)env_int("KMC_DRYRUN", 0);        // 1..5: every level runs again without table writes / frontier traffic
    t.no_chain = (int)env_int("KMC_NO_CHAIN", 0);      // kmc_run launches level by level
    t.chain_max = (uint64_t)env_int("KMC_CHAIN_MAX", KMC_CHAIN_DEFAULT);   // levels per chained batch (at most KMC_CHAIN)
    t.blocks_per_cu = (int)env_int("KMC_BLOCKS_PER_CU", 0);                // k_expand's grid per CU instead of the occupancy query's
    if (hipModuleGetFunction(&t.f_expand_dry, h->mod, ("kmc_expand_dry_" + h->kname).c_str()) != hipSuccess) {
        t.f_expand_dry = nullptr;   // (the code object is not a tuning build)
        (void)hipGetLastError();
    }
}
void tuning_close(kmc_handle* h) {
    if (h->tuning.table2) (void)hipFree(h->tuning.table2);
}
hipFunction_t tuning_dry_kernel(const kmc_handle* h) { return h->tuning.f_expand_dry; }
bool tuning_unchained(const kmc_handle* h) { return h->tuning.shadow || h->tuning.dry_mode || h->tuning.no_chain; }
int tuning_blocks_per_cu(const kmc_handle* h) { return h->tuning.blocks_per_cu; }
uint64_t tuning_chain_max(const kmc_handle* h) { return h->tuning.chain_max; }

// one launch of k_expand between the handle's two events, waited for and booked as dry / shadow time
static int timed_pass(kmc_handle* h, unsigned mode, const KmcArgs& a) {
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    int rc = launch_expand(h, mode, a, expand_grid(h, h->n_cur));
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->tuning.dry_seconds += 1e-3 * ms;
    return KMC_OK;
}

// KMC_SHADOW: the identical level first runs on a copy of the table, with KMC_XFLAGS applied (`a`: the level's own arguments)
int tuning_shadow_level(kmc_handle* h, const KmcArgs& a) {
    kmc_tuning& t = h->tuning;
    if (!t.shadow) return KMC_OK;
    const size_t bytes = h->table_cap * h->stride_words() * 8;
    if (!t.table2) HIP_TRY(hipMalloc(&t.table2, bytes));
    HIP_TRY(hipMemcpyAsync(t.table2, h->table, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->ctl + 2, 0, sizeof(KmcLevelCtl), h->stream));
    KmcArgs x = a;
    x.table = t.table2;
    if (h->paired) x.pred = t.table2 + 1;
    x.ctl = h->ctl + 2;
    x.flags |= t.xflags;
    return timed_pass(h, KMC_MODE_LOCAL, x);
}

// KMC_DRYRUN: the level that has just run is timed again without table writes / frontier traffic
int tuning_dry_level(kmc_handle* h, const KmcArgs& a) {
    kmc_tuning& t = h->tuning;
    if (!t.dry_mode) return KMC_OK;
    KmcArgs d = a;  // 1: no table access at all, 2: + read-only probes, 3: + invariants on every successor
    if (t.dry_mode >= 2) d.flags |= KMC_FLAG_DRY_PROBE;
    if (t.dry_mode == 3) d.flags |= KMC_FLAG_DRY_INV;
    if (t.dry_mode == 4) d.flags |= KMC_FLAG_DRY_ATOM;
    if (t.dry_mode == 5) d.flags |= KMC_FLAG_DRY_RAND;
    d.ctl = h->ctl + 2;
    int rc = timed_pass(h, KMC_MODE_DRY, d);
    if (rc) return rc;
    KmcLevelCtl dc;
    HIP_TRY(hipMemcpy(&dc, h->ctl + 2, sizeof dc, hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) t.prof_dry[k] += dc.prof[k];
    HIP_TRY(hipMemsetAsync(h->ctl + 2, 0, sizeof(KmcLevelCtl), h->stream));
    return KMC_OK;
}

void tuning_report(kmc_handle* h) {
    kmc_tuning& t = h->tuning;
    if (const double tot = (double)t.prof_dry[7]) {
        fprintf(stderr, "[kmc] DRY per-wave ticks: load+extract+inv %.1f%%  guards %.1f%%  effects+push(incl flush) %.1f%%  "
                        "of which flush %.1f%%  tail %.1f%%  (total %.3g ticks)\n", 100 * t.prof_dry[0] / tot, 100 * t.prof_dry[1] / tot,
                100 * t.prof_dry[2] / tot, 100 * t.prof_dry[3] / tot, 100 * t.prof_dry[4] / tot, tot);
        for (int k = 0; k < 8; ++k) t.prof_dry[k] = 0;
    }
    if (t.dry_seconds > 0) fprintf(stderr, "[kmc] dry/shadow expand: %.3f ms vs real %.3f ms\n", 1e3 * t.dry_seconds, 1e3 * h->res.seconds_expand);
    t.dry_seconds = 0;
}

}  // namespace kmc_engine
