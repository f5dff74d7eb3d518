// The block layout rule of arpeggia_amd/csrc/host_common.h (seg_align, Bump, planned_bytes, carve_block), on the host alone: no device, no Python.
// A stand-alone program, built and run by tests/test_carve_host.py under -fsanitize=address,undefined -fno-sanitize-recover=all.  A clean exit (status 0,
// "ok", no sanitizer report) is the result.
//
// For 0, 1, 63, 64, 65 and 1000 elements, a layout of arrays of 8-, 1-, 2-, 4- and 16-byte elements with a take of no elements in its middle and a take that a
// flag switches on: the planning walk hands out null pointers only; the planned size is the sum of the arrays' sizes, each rounded up to 256; a heap block of
// exactly that size, 256-aligned, is carved and every array written from its first to its last byte; every pointer is 256-aligned; the arrays are disjoint,
// in the order of their takes, inside the block; and the layout ran twice.  Then a layout that asks for one element more on its second walk: wherever that
// element needs another segment (the final offsets differ), carve_block returns its error status with a message and nothing in the block was written; where
// the rounding of the first walk already holds it, the carve succeeds and the arrays still fit the block.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../arpeggia_amd/csrc/host_common.h"

namespace arp {
static char g_last_error[256];
static int g_errors = 0;
void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_last_error, sizeof g_last_error, fmt, ap); va_end(ap); g_errors++; }
}  // namespace arp

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) { fprintf(stderr, "%s:%d: n = %llu, with = %d: %s\n", __FILE__, __LINE__, (unsigned long long)n, (int)with, #cond); return 1; } \
    } while (0)

struct Wide { uint64_t w[2]; };
struct Arrays {
    double *a = nullptr; uint8_t *b = nullptr; uint16_t *none = nullptr, *c = nullptr; uint32_t *d = nullptr; Wide *e = nullptr;
    const void *ptr(int k) const { const void *p[6] = {a, b, none, c, d, e}; return p[k]; }
};

static int check(uint64_t n, bool with) {
    using namespace arp;
    Arrays v;
    int walks = 0;
    auto layout = [&](Bump &bp) {
        walks++;
        v.a = bp.take<double>(n); v.b = bp.take<uint8_t>(n);
        v.none = bp.take<uint16_t>(0);
        v.c = bp.take<uint16_t>(n);
        v.d = with ? bp.take<uint32_t>(n) : nullptr;
        v.e = bp.take<Wide>(n);
    };
    const uint64_t bytes[6] = {n * 8u, n, 0u, n * 2u, with ? n * 4u : 0u, n * 16u};
    uint64_t sum = 0;
    for (uint64_t b : bytes) sum += (b + 255u) / 256u * 256u;
    // the plan
    v.a = reinterpret_cast<double *>(&v);  // (anything but null: the planning walk must overwrite it)
    const uint64_t planned = planned_bytes(layout);
    CHECK(walks == 1);
    for (int k = 0; k < 6; k++) CHECK(v.ptr(k) == nullptr);
    CHECK(planned == sum);
    // the carve, on a heap block of exactly the planned size
    char *block = planned ? static_cast<char *>(aligned_alloc(256, planned)) : nullptr;
    CHECK(!planned || block);
    CHECK(carve_block(block, planned, layout) == ARP_OK && g_errors == 0);
    CHECK(walks == 2);
    const char *at = block;
    for (int k = 0; k < 6; k++) {
        const char *p = static_cast<const char *>(v.ptr(k));
        if (k == 4 && !with) { CHECK(p == nullptr); continue; }
        if (!planned) { CHECK(p == nullptr); continue; }
        CHECK(reinterpret_cast<uintptr_t>(p) % 256u == 0);
        CHECK(p >= at);               // behind the array before it
        at = p + bytes[k];
        CHECK(at <= block + planned);  // and inside the block
        memset(const_cast<char *>(p), 0xAB, bytes[k]);
    }
    // one element more on the second walk
    int second = 0;
    auto drifting = [&](Bump &bp) {
        v.b = bp.take<uint8_t>(n);
        v.a = bp.take<double>(n + second++);
    };
    const uint64_t first_plan = planned_bytes(drifting), honest = (n + 255u) / 256u * 256u + (n * 8u + 8u + 255u) / 256u * 256u;
    CHECK(first_plan <= planned);  // (the block above serves)
    if (block) memset(block, 0x5C, planned);
    const arp_status s = carve_block(block, first_plan, drifting);
    if (honest != first_plan) {
        CHECK(s == ARP_ERR_HIP && g_errors == 1 && strncmp(g_last_error, "internal error: ", 16) == 0);
        for (uint64_t k = 0; k < planned; k++) CHECK(block[k] == 0x5C);
        g_errors = 0;
    } else {
        CHECK(s == ARP_OK && g_errors == 0);
        CHECK(reinterpret_cast<char *>(v.a + n + 1u) <= block + first_plan);
        memset(v.a, 0xAB, (n + 1u) * 8u);
    }
    free(block);
    return 0;
}

int main() {
    const uint64_t counts[] = {0, 1, 63, 64, 65, 1000};
    for (uint64_t n : counts)
        for (int with = 0; with < 2; with++)
            if (check(n, with != 0)) return 1;
    puts("ok");
    return 0;
}
