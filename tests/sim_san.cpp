// Random simulation's lane-local layer under the sanitizers: tests/sim_emu.cpp (csrc/kmc_sim.h compiled for the host) with a
// main of its own, built with -fsanitize=address,undefined by tests/sim_emu.py: build_san.  Runs a recorded batch of every
// compiled entry, with the invariants on and off, on two threads, and prints one line per entry: name, constants, states.
// A stand-alone program on purpose: it is never loaded into Python.  TEST INFRASTRUCTURE ONLY.
#include "sim_emu.cpp"

#include <cstdio>

int main() {
    static const char* const NAMES[] = {"IdSequence", "FiniteReplicatedLog", "KafkaTruncateToHighWatermark", "Kip101", "Kip279",
                                        "Kip320", "Kip320FirstTry"};
    int c7[7];
    const int n = sim_emu_configs(-1, c7);
    for (int i = 0; i < n; ++i) {
        sim_emu_configs(i, c7);
        const int W = sim_emu_words(c7);
        if (W < 1) return 1;
        const uint32_t depth = 24;
        const uint64_t walks = 64;
        std::vector<u64> rec((size_t)walks * depth * (W + 1));
        std::vector<uint32_t> lens(walks);
        SimEmuResult plain, checked;
        if (sim_emu_run(c7, 5, 0, walks, depth, 24, 0, 0, 0, 2, &plain, rec.data(), lens.data())) return 1;
        if (sim_emu_run(c7, 5, 0, walks, depth, 24, 15, 1, 1, 2, &checked, nullptr, nullptr)) return 1;
        uint64_t sum = 0;
        for (uint32_t l : lens) sum += l;
        if (sum != plain.states_generated || plain.launches != 3 || checked.states_generated > plain.states_generated) return 2;
        printf("%s %d/%d/%d/%d %s%llu\n", NAMES[c7[0]], c7[1], c7[2], c7[3], c7[4], c7[6] ? "(forced layout) " : "",
               (unsigned long long)plain.states_generated);
    }
    puts("sim_san ok");
    return 0;
}
