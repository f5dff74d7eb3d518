// TEST-ONLY stand-alone program: the host twin of the secondary-structure call (arpeggia_amd/csrc/dssp.cpp, arp_dssp_host) on the cases of a file, built with
// -fsanitize=address,undefined by tests/test_dssp_host.py.  No device code runs: the device half of dssp.cpp is given stubs.
//   file: u64 n_cases, then per case u64 F, u64 R, F x R x 12 f64 (N, CA, C, O), R u8 flags.   Prints one line of "-HBEGITS" characters per frame.
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../arpeggia_amd/csrc/dssp.cpp"

namespace arp {
DebugKnobs g_debug{};
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
arp_status rmsd_frames_check(const arp_structure *, uint64_t, const double *, std::vector<double> *, const double **, uint64_t *, uint64_t *) { return ARP_ERR_BAD_INPUT; }
arp_status device_dssp(arp_context *, const DsspJob &, DsspOut *) { return ARP_ERR_BAD_INPUT; }
}  // namespace arp

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    uint64_t n_cases = 0;
    if (fread(&n_cases, 8, 1, fp) != 1) return 2;
    for (uint64_t c = 0; c < n_cases; c++) {
        uint64_t F = 0, R = 0;
        if (fread(&F, 8, 1, fp) != 1 || fread(&R, 8, 1, fp) != 1) return 2;
        // exactly-sized heap blocks: a read or write one element outside any of them is an error of the sanitizer
        std::vector<double> xyz(F * R * 12);
        std::vector<uint8_t> flags(R), codes(F * R);
        std::vector<uint32_t> counts(R * 8), frame_counts(F * 8), acc(F * R * 2);
        std::vector<float> en(F * R * 2);
        if (fread(xyz.data(), 8, xyz.size(), fp) != xyz.size() || fread(flags.data(), 1, R, fp) != R) return 2;
        if (arp_dssp_host(F, R, xyz.data(), flags.data(), codes.data(), counts.data(), frame_counts.data(), acc.data(), en.data()) != ARP_OK) return 1;
        for (uint64_t f = 0; f < F; f++) {
            for (uint64_t r = 0; r < R; r++) putchar("-HBEGITS"[codes[f * R + r]]);
            putchar('\n');
        }
    }
    fclose(fp);
    return 0;
}
