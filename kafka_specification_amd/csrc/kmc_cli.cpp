// kmc_cli.cpp — native `tlc`-shaped front end over the C ABI (include/kmc.h), for hosts without Python/torch: argument
// handling, the run and its TLC-shaped report.  What a .cfg, a spec file, a state and a stock-TLC switch mean is asked of the
// library (kmc_frontend.cpp), as kafka_specification_amd/tlc.py asks it.
//
//   tlc [-config X.cfg] [-deadlock] [-continue] [-workers N] [-fp SEED] [-fp128] [-symmetry] [-fpcheck] [-verify] [-force] [-levels-csv FILE] [-table SLOTS]
//       [-frontier STATES] [-device D] [-notrace] [-v] [-walks N [-walk-depth D] [-walk-seed S]] Spec.tla
//
// -walks N runs N random walks from Init instead of the search (random simulation: kmc_simulate; stock TLC's -simulate / -depth /
// -seed spellings stay refused), -walk-depth the states per walk at the most (100), -walk-seed the seed (0).
//
// [TLC-recall] flag names and output lines follow tlc2.TLC; TLC itself is not part of the
// reference repository.  The module name selects one of the lowered models; constants
// and invariants come from the .cfg (CONSTANT(S), INIT, NEXT, SPECIFICATION, INVARIANT(S),
// CHECK_DEADLOCK).  No TLA+ is parsed — therefore the spec file given (and every module it EXTENDS / INSTANCEs that
// is found beside it) is hashed against the revision the kernels were lowered from; an edited spec is refused unless
// -force (kmc_spec_check).  -fpcheck repeats the search with a second fingerprint seed and compares the counts; the summary
// prints TLC's collision-probability estimate (kmc_collision_report).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/kmc.h"

static double wall_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

namespace {

std::string now() {
    char buf[64];
    time_t t = time(nullptr);
    strftime(buf, sizeof buf, "%Y-%m-%d %H:%M:%S", localtime(&t));
    return buf;
}

// canonical bytes -> TLA+ text, the way TLC prints a trace state
void print_state(const kmc_config& c, const uint8_t* b, uint64_t n) {
    std::vector<char> text((size_t)kmc_format_state(&c, b, n, nullptr, 0) + 1);
    kmc_format_state(&c, b, n, text.data(), text.size());
    printf("%s\n", text.data());
}

// -walks: a batch of random walks instead of the search; the report's lines are the library's (kmc_sim_report)
int run_walks(const kmc_config& c, const kmc_sim_config& sim, const std::string& module) {
    char text[4096];
    std::vector<const char*> names;
    for (int k = 0; k < kmc_action_count(c.model); ++k) names.push_back(kmc_action_name(c.model, k));
    kmc_sim_report(&c, &sim, nullptr, 0, names.data(), (int32_t)names.size(), text, sizeof text);
    printf("%s\n", text);
    kmc_handle* h = nullptr;
    if (kmc_open(&c, &h) != KMC_OK) { fprintf(stderr, "Error: %s\n", kmc_last_error()); return 3; }
    kmc_sim_result r;
    if (kmc_simulate(h, &sim, &r) != KMC_OK) { fprintf(stderr, "Error: %s\n", kmc_last_error()); kmc_close(h); return 3; }
    int rc = 0;
    if (r.verdict == KMC_V_OK) {
        printf("Random simulation completed. No error has been found.\n");
    } else {
        if (r.verdict == KMC_V_INVARIANT) printf("Error: Invariant %s is violated%s.\n", kmc_model_invariant_name(c.model, r.violated_invariant),
                                                 r.violation_step == 0 ? " by the initial state" : "");
        else printf("Error: Deadlock reached.\n");
        rc = r.verdict == KMC_V_INVARIANT ? 12 : 11;
        const uint64_t cb = kmc_canon_bytes(h), cap = r.violation_step + 1;
        std::vector<uint8_t> states(cap * cb);
        std::vector<int32_t> kinds(cap);
        uint64_t nt = 0;
        if (kmc_simulate_walk(h, &sim, r.violation_walk, states.data(), kinds.data(), nullptr, nullptr, cap, &nt) == KMC_OK) {
            printf("Error: The behavior up to this point is (walk %llu):\n", (unsigned long long)r.violation_walk);
            for (uint64_t k = 0; k < nt && k < cap; ++k) {
                if (k == 0) printf("State 1: <Initial predicate>\n");
                else printf("State %llu: <%s of module %s>\n", (unsigned long long)(k + 1), kmc_action_name(c.model, kinds[k]), module.c_str());
                print_state(c, states.data() + k * cb, cb);
                printf("\n");
            }
        } else {
            fprintf(stderr, "Error: %s\n", kmc_last_error());
        }
    }
    kmc_sim_report(&c, &sim, &r, 1, names.data(), (int32_t)names.size(), text, sizeof text);
    printf("%s\n", text);
    printf("Finished in %.3fs (%.0f steps/s in the simulate kernel, %.3fs) at (%s)\n", r.seconds_total,
           (double)(r.states_generated - r.walks) / (r.seconds_kernel > 1e-9 ? r.seconds_kernel : 1e-9), r.seconds_kernel, now().c_str());
    kmc_close(h);
    return rc;
}

void on_level(const kmc_level_info* i, void*) {
    if (i->depth == 1)
        printf("Finished computing initial states: %llu distinct state generated at %s.\n",
               (unsigned long long)i->distinct_total, now().c_str());
    else
        printf("Progress(%llu) at %s: %llu states generated, %llu distinct states found, %llu states left on queue.\n",
               (unsigned long long)i->depth, now().c_str(), (unsigned long long)i->generated_total,
               (unsigned long long)i->distinct_total, (unsigned long long)i->new_states);
}

}  // namespace

int main(int argc, char** argv) {
    std::string spec, cfg_path;
    kmc_config c;
    memset(&c, 0, sizeof c);
    c.n_shards = 1;
    c.keep_trace = 1;
    bool no_deadlock = false, fpcheck = false, force = false, verbose = false;
    std::string levels_csv;
    const char *walks = nullptr, *walk_depth = nullptr, *walk_seed = nullptr;
    const double t_main0 = wall_s();
    int32_t stock = KMC_SWITCH_NONE;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* what) -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "Error: %s needs a value\n", what); exit(2); }
            return argv[++i];
        };
        if (a == "-abi-sizes") {   // tests/test_abi_cpu.py: the structs of include/kmc.h as this translation unit sees them
            printf("%zu %zu %zu %zu %zu\n", sizeof(kmc_config), sizeof(kmc_level_info), sizeof(kmc_result), sizeof(kmc_level_stat), sizeof(kmc_timing));
            return 0;
        }
        if (a == "-config") cfg_path = val("-config");
        else if (a == "-deadlock") no_deadlock = true;
        else if (a == "-continue") c.continue_on_violation = 1;
        else if (a == "-workers") val("-workers");  // accepted, ignored: the GPU's waves are the workers
        else if (a == "-fp") c.hash_seed = strtoull(val("-fp"), nullptr, 0);
        else if (a == "-table") c.table_capacity = strtoull(val("-table"), nullptr, 0);
        else if (a == "-frontier") c.frontier_capacity = strtoull(val("-frontier"), nullptr, 0);
        else if (a == "-device") c.device = atoi(val("-device"));
        else if (a == "-notrace") c.keep_trace = 0;
        else if (a == "-fpcheck") fpcheck = true;
        else if (a == "-fp128") c.wide_fingerprint = 1;  // 128-bit seen-set entries: fingerprint + independent check word
        else if (a == "-symmetry") c.symmetry = 1;  // orbit counting: one stored state per orbit of the permutations of Replicas
        else if (a == "-force") force = true;
        else if (a == "-levels-csv") levels_csv = val("-levels-csv");  // one line per BFS level: frontier, generated per disjunct, new, table load, kernel ms
        else if (a == "-walks") walks = val("-walks");   // random simulation: this many walks from Init instead of the search
        else if (a == "-walk-depth") walk_depth = val("-walk-depth");
        else if (a == "-walk-seed") walk_seed = val("-walk-seed");
        else if (a == "-v") verbose = true;   // where the wall time went: start-up (HIP, code object, allocation, first touch), search, teardown
        else if (a == "-verify") setenv("KMC_VERIFY", "1", 1);  // every level is regenerated by a second build of the kernels
        else if (const char* why = kmc_tlc_switch(a.c_str(), &stock)) {   // stock TLC's other switches [TLC-recall]
            if (stock == KMC_SWITCH_REFUSED) {
                fprintf(stderr, "Error: %s is not supported: %s\n", a.c_str(), why);
                if (a == "-simulate") fprintf(stderr, "Note: -walks N [-walk-depth D] [-walk-seed S] runs N random walks from Init\n");
                return 2;
            }
            if (stock == KMC_SWITCH_IGNORED) fprintf(stderr, "Note: %s is accepted for compatibility and ignored (%s)\n", a.c_str(), why);
            else fprintf(stderr, "Note: %s %s is accepted for compatibility and ignored (%s)\n", a.c_str(), val(a.c_str()), why);
        } else if (a == "-checkpoint") {
            const char* v = val("-checkpoint");   // TLC's interval in minutes; this front end has no sharded checkpoints
            fprintf(stderr, "Note: -checkpoint %s is accepted and ignored (a search takes milliseconds to seconds; the Python front "
                            "end's -checkpoint DIR saves a level-limited sharded search)\n", v);
        }
        else if (!a.empty() && a[0] == '-') { fprintf(stderr, "Error: unknown option %s\n", a.c_str()); return 2; }
        else spec = a;
    }
    kmc_sim_config sim;
    int32_t walk_mode = 0;
    if (kmc_walk_switches(walks, walk_depth, walk_seed, &sim, &walk_mode) != KMC_OK) { fprintf(stderr, "Error: %s\n", kmc_last_error()); return 2; }
    if (spec.empty()) { fprintf(stderr, "usage: tlc [-config X.cfg] [-deadlock] [-continue] [-fp N] Spec.tla\n"); return 2; }
    size_t slash = spec.find_last_of('/');
    std::string module = spec.substr(slash == std::string::npos ? 0 : slash + 1);
    if (module.size() > 4 && module.substr(module.size() - 4) == ".tla") module.resize(module.size() - 4);
    if (cfg_path.empty()) cfg_path = spec.substr(0, spec.size() - (spec.size() > 4 && spec.substr(spec.size() - 4) == ".tla" ? 4 : 0)) + ".cfg";
    FILE* f = fopen(cfg_path.c_str(), "rb");
    if (!f) { fprintf(stderr, "Error: configuration file %s not found\n", cfg_path.c_str()); return 2; }
    std::string text;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    if (kmc_cfg_bind(module.c_str(), text.c_str(), &c) != KMC_OK) { fprintf(stderr, "Error: %s\n", kmc_last_error()); return 2; }
    if (no_deadlock) c.check_deadlock = 0;

    char findings[16384];
    const int spec_status = kmc_spec_check(spec.c_str(), findings, sizeof findings);
    for (const char* line = findings; *line;) {
        const size_t len = strcspn(line, "\n");
        fprintf(stderr, "%s%.*s\n", spec_status == 2 ? "Error: " : "Warning: ", (int)len, line);
        line += len + (line[len] ? 1 : 0);
    }
    if (spec_status == 2) {
        if (!force) {
            fprintf(stderr, "Error: the spec differs from the revision the GPU kernels were lowered from; nothing was checked "
                            "(-force checks the built-in lowering anyway)\n");
            return 2;
        }
        fprintf(stderr, "Warning: -force: checking the BUILT-IN lowering, not the text of the spec given\n");
    }

    printf("kafka_specification_amd model checker (MI355X, native CLI) — module %s, config %s\n", module.c_str(), cfg_path.c_str());
    if (walk_mode) return run_walks(c, sim, module);
    printf("Running breadth-first search Model-Checking with fp seed %llu on GPU %d.\n", (unsigned long long)c.hash_seed, c.device);
    printf("Computing initial states...\n");
    kmc_handle* h = nullptr;
    const double t_open0 = wall_s();
    if (kmc_open(&c, &h) != KMC_OK) { fprintf(stderr, "Error: %s\n", kmc_last_error()); return 3; }
    const double t_run0 = wall_s();
    if (kmc_run(h, on_level, nullptr) != KMC_OK) { fprintf(stderr, "Error: %s\n", kmc_last_error()); kmc_close(h); return 3; }
    const double t_run1 = wall_s();
    kmc_result r;
    kmc_result_get(h, &r);
    kmc_timing tm;
    memset(&tm, 0, sizeof tm);
    kmc_timing_get(h, &tm);
    int rc = 0;
    if (r.verdict == KMC_V_OK) {
        printf("Model checking completed. No error has been found.\n");
    } else if (r.verdict == KMC_V_INVARIANT) {
        printf("Error: Invariant %s is violated%s.\n", kmc_model_invariant_name(c.model, r.violated_invariant),
               r.violation_depth == 1 ? " by the initial state" : "");
        rc = 12;
    } else if (r.verdict == KMC_V_DEADLOCK) {
        printf("Error: Deadlock reached.\n");
        rc = 11;
    } else {
        printf("Error: search stopped with verdict %d (table %llu slots, frontier %llu states)\n", r.verdict,
               (unsigned long long)r.table_capacity, (unsigned long long)r.frontier_capacity);
        rc = 1;
    }
    const uint64_t cb = kmc_canon_bytes(h);
    if (r.verdict == KMC_V_INVARIANT && c.keep_trace) {
        const uint64_t cap = r.violation_depth + 1;
        std::vector<uint8_t> states(cap * cb);
        std::vector<int32_t> kinds(cap);
        uint64_t nt = 0;
        if (kmc_trace(h, states.data(), kinds.data(), cap, &nt) == KMC_OK) {
            printf("Error: The behavior up to this point is:\n");
            for (uint64_t k = 0; k < nt && k < cap; ++k) {
                if (k == 0) printf("State 1: <Initial predicate>\n");
                else printf("State %llu: <%s of module %s>\n", (unsigned long long)(k + 1), kmc_action_name(c.model, kinds[k]), module.c_str());
                print_state(c, states.data() + k * cb, cb);
                printf("\n");
            }
        } else {
            fprintf(stderr, "Error: %s\n", kmc_last_error());
        }
    } else if (r.verdict == KMC_V_DEADLOCK) {
        std::vector<uint64_t> w(kmc_state_words(h));
        std::vector<uint8_t> st(cb);
        if (kmc_witness(h, w.data()) == KMC_OK) {
            kmc_unpack_state(h, w.data(), st.data());
            printf("Error: The deadlocked state is:\n");
            print_state(c, st.data(), cb);
        }
    }
    if (!levels_csv.empty()) {
        // the per-level view a user tunes constants and capacities by (kmc_level_stats: one record per expansion)
        std::vector<kmc_level_stat> st(kmc_level_stats(h, nullptr, 0));
        const uint64_t ns = kmc_level_stats(h, st.data(), st.size());
        if (FILE* lf = fopen(levels_csv.c_str(), "w")) {
            fprintf(lf, "depth,frontier,new_states,stored_new,probes,deadlocks,table_load,expand_ms");
            const int nk = kmc_action_count(c.model);
            for (int k = 0; k < nk; ++k) fprintf(lf, ",%s", kmc_action_name(c.model, k));
            fprintf(lf, "\n");
            for (uint64_t i = 0; i < ns && i < st.size(); ++i) {
                fprintf(lf, "%llu,%llu,%llu,%llu,%llu,%llu,%.6f,%.4f", (unsigned long long)st[i].depth, (unsigned long long)st[i].frontier,
                        (unsigned long long)st[i].new_states, (unsigned long long)st[i].stored_new, (unsigned long long)st[i].probes,
                        (unsigned long long)st[i].deadlocks, st[i].table_load, st[i].expand_ms);
                for (int k = 0; k < nk; ++k) fprintf(lf, ",%llu", (unsigned long long)st[i].generated[k]);
                fprintf(lf, "\n");
            }
            fclose(lf);
        } else {
            fprintf(stderr, "Error: cannot write %s\n", levels_csv.c_str());
        }
    }
    printf("%llu states generated, %llu distinct states found, %llu states left on queue.\n", (unsigned long long)r.generated,
           (unsigned long long)r.distinct, (unsigned long long)r.queue_left);
    printf("The depth of the complete state graph search is %llu.\n", (unsigned long long)r.depth);
    if (c.symmetry)
        printf("Symmetry reduction (orbit counting over the permutations of Replicas): %llu states were stored and expanded, one "
               "per orbit; every count above is the plain search's.\n", (unsigned long long)r.orbit_representatives);
    char estimate[2048];
    if (kmc_collision_report(r.distinct, r.generated, c.symmetry ? r.orbit_representatives : 0, c.wide_fingerprint, rc == 0, estimate,
                             sizeof estimate))
        rc = KMC_EXIT_UNCERTIFIED;
    printf("%s\n", estimate);
    if (fpcheck) {  // a collision moves with the seed: equal counts under two seeds make a silent loss very unlikely
        kmc_close(h);
        h = nullptr;
        kmc_config c2 = c;
        c2.hash_seed = c.hash_seed * 0x9E3779B97F4A7C15ull + 0x5851F42D4C957F2Dull;
        c2.keep_trace = 0;
        kmc_result r2;
        if (kmc_open(&c2, &h) != KMC_OK || kmc_run(h, nullptr, nullptr) != KMC_OK || kmc_result_get(h, &r2) != KMC_OK) {
            fprintf(stderr, "Error: %s\n", kmc_last_error());
            if (h) kmc_close(h);
            return 3;
        }
        const bool same = r2.verdict == r.verdict && r2.distinct == r.distinct && r2.generated == r.generated && r2.depth == r.depth;
        printf("Fingerprint check: second run with fp seed %llu: %llu states generated, %llu distinct states found, depth %llu - %s\n",
               (unsigned long long)c2.hash_seed, (unsigned long long)r2.generated, (unsigned long long)r2.distinct,
               (unsigned long long)r2.depth,
               same ? "identical to the first run." : "DIFFERENT from the first run: a fingerprint collision dropped states in at least one of them "
                      "(a collision can only lose states: the larger count is the better lower bound).");
        if (!same && rc == 0) rc = 13;
    }
    printf("Finished in %.3fs (%.0f distinct states/s; %.3fs in the expand kernel) at (%s)\n", r.seconds_total,
           r.distinct / (r.seconds_total > 1e-9 ? r.seconds_total : 1e-9), r.seconds_expand, now().c_str());
    const double t_close0 = wall_s();
    kmc_close(h);
    if (verbose) {
        // (printed after the teardown it accounts for; kmc_timing: include/kmc.h)
        const double t_end = wall_s();
        printf("Wall time: %.3fs in this process = %.3fs before kmc_open (arguments, .cfg, spec revision) + %.3fs kmc_open "
               "(HIP initialisation %.3fs, code object %.3fs, allocation of %.1f GiB %.3fs) + %.3fs kmc_run (first clear of the "
               "seen-set %.3fs, search %.3fs) + %.3fs verdict / trace + %.3fs teardown\n",
               t_end - t_main0, t_open0 - t_main0, t_run0 - t_open0, tm.hip_init_s, tm.code_object_s,
               (double)tm.device_bytes / (double)(1ull << 30), tm.alloc_s, t_run1 - t_run0, tm.first_clear_s, r.seconds_total,
               t_close0 - t_run1, t_end - t_close0);
    }
    return rc;
}
