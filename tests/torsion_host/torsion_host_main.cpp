// TEST-ONLY stand-alone program: the host twin of the torsion call (arpeggia_amd/csrc/torsion.cpp, arp_torsions_host) on the cases of a file, built with
// -fsanitize=address,undefined by tests/test_torsion_host.py.  No device code runs: the device half of torsion.cpp is given stubs.
//   file: u64 n_cases, then per case u64 F, u64 D, u32 B, u64 P, u32 G, F x D x 12 f64, P x 3 u32.
//   Prints one line of state digits per frame, then "hist2 <sum>".
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../arpeggia_amd/csrc/torsion.cpp"

namespace arp {
DebugKnobs g_debug{};
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
uint64_t rmsd_cap() { return 0; }
arp_status rmsd_frames_check(const arp_structure *, uint64_t, const double *, std::vector<double> *, const double **, uint64_t *, uint64_t *) { return ARP_ERR_BAD_INPUT; }
arp_status device_torsions(arp_context *, const TorsionJob &, TorsionOut *) { return ARP_ERR_BAD_INPUT; }
}  // namespace arp

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    uint64_t n_cases = 0;
    if (fread(&n_cases, 8, 1, fp) != 1) return 2;
    for (uint64_t c = 0; c < n_cases; c++) {
        uint64_t F = 0, D = 0, P = 0;
        uint32_t B = 0, G = 0;
        if (fread(&F, 8, 1, fp) != 1 || fread(&D, 8, 1, fp) != 1 || fread(&B, 4, 1, fp) != 1 || fread(&P, 8, 1, fp) != 1 || fread(&G, 4, 1, fp) != 1) return 2;
        // exactly-sized heap blocks: a read or write one element outside any of them is an error of the sanitizer
        std::vector<double> xyz(F * D * 12), cossin(F * D * 2), sums(D * 2);
        std::vector<uint32_t> pairs(P * 3), n_defined(D), state_counts(D * 4), n_transitions(D), hist(D * B), hist2((uint64_t)G * B * B);
        std::vector<float> angles(F * D);
        std::vector<uint8_t> states(F * D);
        if (fread(xyz.data(), 8, xyz.size(), fp) != xyz.size() || fread(pairs.data(), 4, pairs.size(), fp) != pairs.size()) return 2;
        if (arp_torsions_host(F, D, xyz.data(), B, P ? pairs.data() : nullptr, P, G, angles.data(), cossin.data(), states.data(), sums.data(), n_defined.data(),
                              state_counts.data(), n_transitions.data(), hist.data(), G ? hist2.data() : nullptr) != ARP_OK)
            return 1;
        for (uint64_t f = 0; f < F; f++) {
            for (uint64_t d = 0; d < D; d++) putchar('0' + states[f * D + d]);
            putchar('\n');
        }
        unsigned long long total = 0;
        for (uint32_t v : hist2) total += v;
        printf("hist2 %llu\n", total);
    }
    fclose(fp);
    return 0;
}
