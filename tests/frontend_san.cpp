// frontend_san.cpp — csrc/kmc_frontend.cpp alone under ASan + UBSan (tests/test_sanitizers_cpu.py): the .cfg reader on the files
// named on the command line (`module file accepted` triples) and on cut-off texts, the state printer at the largest constants
// and into buffers of every small size.  Prints what it did; a sanitizer report, or an answer other than the expected one, fails.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/kmc.h"

// what the front end asks of the engine, which is not linked here: the last error and the names of include/kmc.h
static std::string g_error;
namespace kmc_engine {
int fail(int code, const char* fmt, ...) {
    char buf[8192];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}
}  // namespace kmc_engine
extern "C" const char* kmc_last_error(void) { return g_error.c_str(); }
extern "C" const char* kmc_model_name(int32_t m) {
    static const char* const names[] = {"IdSequence", "FiniteReplicatedLog", "KafkaTruncateToHighWatermark", "Kip101", "Kip279", "Kip320",
                                        "Kip320FirstTry", "AsyncIsr"};
    return m >= 0 && m < 8 ? names[m] : "?";
}
extern "C" const char* kmc_model_invariant_name(int32_t model, int32_t i) {
    static const char* const kafka[] = {"TypeOk", "WeakIsr", "StrongIsr", "LeaderInIsr"};
    static const char* const async[] = {"TypeOk", "ValidHighWatermark", "LeaderOffsetInRange", "?"};
    return i < 0 || i > 3 ? "?" : model == KMC_ASYNC_ISR ? async[i] : kafka[i];
}

static int bad = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { printf("UNEXPECTED: %s\n", what); ++bad; }
}

int main(int argc, char** argv) {
    int bound = 0, refused = 0;
    for (int i = 1; i + 2 < argc; i += 3) {
        std::stringstream text;
        text << std::ifstream(argv[i + 1]).rdbuf();
        kmc_config c{};
        const int rc = kmc_cfg_bind(argv[i], text.str().c_str(), &c);
        expect((rc == KMC_OK) == (atoi(argv[i + 2]) != 0), argv[i + 1]);
        expect(rc == KMC_OK || rc == KMC_E_ARG, "status of kmc_cfg_bind");
        ++(rc == KMC_OK ? bound : refused);
        const std::string whole = text.str();          // ... and every cut of it: whatever the answer, no read past the end
        for (size_t n = 0; n < whole.size(); n += 1 + whole.size() / 64) kmc_cfg_bind(argv[i], whole.substr(0, n).c_str(), &c);
    }
    kmc_config c{};
    for (const char* cut : {"CONSTANTS Replicas = {b1, b2", "CONSTANT MaxId = 1 (* never closed", "CONSTANT MaxId = \"3", "CONSTANT", "{", "=",
                            "CONSTANT MaxId <-", "CONSTANTS Replicas = {,,}\nLogSize = 99999999999999999999999"})
        expect(kmc_cfg_bind("Kip320", cut, &c) == KMC_E_ARG, cut);

    // the largest constants of each family (include/kmc.h), every byte 0xff: all requests present, every set full
    struct { int model, N, L, E; uint64_t bytes; } biggest[] = {
        {KMC_KIP320, 8, 255, 7, 8 * 260 + 5 + 16}, {KMC_ASYNC_ISR, 6, 255, 7, 6 + 6 + 8 * 8 + 8}, {KMC_ASYNC_ISR, 8, 3, 63, 6 + 8 + 64 * 32 + 64},
        {KMC_FINITE_REPLICATED_LOG, 8, 255, 0, 8 * 256}, {KMC_IDSEQUENCE, 0, 0, 0, 8}};
    for (const auto& b : biggest) {
        c.model = b.model, c.n_replicas = b.N, c.log_size = b.L, c.max_leader_epoch = b.E;
        const uint64_t need = b.bytes;
        std::vector<uint8_t> canon(need, 0xff);        // (exactly the layout's bytes: a read past them is a heap overflow)
        const int64_t len = kmc_format_state(&c, canon.data(), need, nullptr, 0);
        expect(len > 0 && kmc_format_state(&c, canon.data(), need - 1, nullptr, 0) == -1, "length check of kmc_format_state");
        for (uint64_t cap : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)len, (uint64_t)len + 1}) {
            std::vector<char> out(cap);
            expect(kmc_format_state(&c, canon.data(), need, out.data(), cap) == len, "length of the text");
            expect(cap == 0 || strlen(out.data()) == (cap <= (uint64_t)len ? cap - 1 : (uint64_t)len), "text cut to the buffer");
        }
        printf("model %d: %llu canonical bytes, %lld characters\n", b.model, (unsigned long long)need, (long long)len);
    }
    c.n_replicas = 9;
    c.model = KMC_KIP320;
    uint8_t one = 0;
    expect(kmc_format_state(&c, &one, 1, nullptr, 0) == -1, "nine replicas");

    for (uint64_t cap : {0, 1, 2, 4096}) {
        std::vector<char> out(cap);
        expect(kmc_collision_report(6452700520ull, 20756484505ull, 0, 0, 1, out.data(), cap) == KMC_EXIT_UNCERTIFIED, "uncertified count");
        expect(kmc_collision_report(~0ull, ~0ull, ~0ull, 1, 1, out.data(), cap) == 0, "wide entries");
        expect(kmc_spec_check("/nonexistent/Kip320.tla", out.data(), cap) == 1, "absent spec");
    }
    int32_t kind = -1;
    expect(kmc_tlc_switch("-simulate", &kind) && kind == KMC_SWITCH_REFUSED && !kmc_tlc_switch("-config", &kind) && kind == KMC_SWITCH_NONE &&
               !kmc_tlc_switch(nullptr, nullptr), "switch classes");
    printf("%d bound, %d refused, %d unexpected\n", bound, refused, bad);
    return bad ? 1 : 0;
}
