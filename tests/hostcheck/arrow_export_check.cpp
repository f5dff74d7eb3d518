// Ownership and layout of the Arrow export of column-built tables (arpeggia_amd/csrc/table.cpp), on the host alone: no device, no Python.
// A stand-alone program; no test runs it.  Build and run from the repository root:
//
//   c++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tests/hostcheck/arrow_export_check.cpp
//       arpeggia_amd/csrc/table.cpp -o arrow_export_check   (one line), then ./arrow_export_check
//
// A clean exit (status 0, "ok", no sanitizer or leak report) is the result.  It fills an arp_table by hand for every kind the registry exporter
// serves -- the column-built contact table with null sc_* rows, atom frequencies, residue frequencies, a timeline table -- at 0, 1 and 9 rows (nine
// rows cross a validity byte), exports each, checks children, names, formats, flags, null counts, the offsets' last entry and values, and releases
// schema and array in both orders, with children moved out first as an Arrow consumer may, and with the table freed before the batch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../arpeggia_amd/csrc/table.h"

// what table.cpp takes from the rest of the library
namespace arp {
DebugKnobs g_debug{};
static char g_last_error[256];
void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_last_error, sizeof g_last_error, fmt, ap); va_end(ap); }
int host_threads() { return 2; }
}  // namespace arp
static const char *const kNames[] = {"StericClash", "CovalentBond", "VanDerWaalsContact"};
extern "C" const char *arp_interaction_name(int32_t code) { return code >= 0 && code < 3 ? kNames[code] : "?"; }

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

using namespace arp;

static EntityRec entity(size_t k, bool ring) {
    EntityRec e{};
    snprintf(e.chain, sizeof e.chain, "%s", k % 2 ? "A" : "BB");
    snprintf(e.resn, sizeof e.resn, "%s", k % 3 ? "PHE" : "GLY");
    snprintf(e.atomn, sizeof e.atomn, "%s", ring ? "Ring" : "CA");
    if (k % 4 == 0) e.insertion[0] = 'i';
    if (k % 5 == 0) e.altloc[0] = 'B';
    e.resi = (int32_t)k - 3; e.atomi = ring ? 0 : (int32_t)(10 * k); e.atom = ring ? -1 : (int32_t)k; e.model = 1;
    return e;
}

enum Kind { CONTACT, ATOM_FREQ, RESIDUE_FREQ, TIMELINE };
static arp_table *make_table(Kind kind, size_t n) {
    arp_table *t = new arp_table();
    t->n = n;
    if (kind == CONTACT) contact_columns(t);
    else frequency_columns(t, kind == RESIDUE_FREQ ? kResidueFreqSide : kAtomFreqSide);
    if (kind == TIMELINE) { t->tl.has_bitmap = true; t->tl.words_per_row = 1; t->tl.words.assign(n, 1u); t->tl_frames = 7; timeline_columns(t); }
    for (size_t k = 0; k < n; k++) {
        t->interaction[k] = (int32_t)(k % 3);
        t->from.put(k, entity(k, false)); t->to.put(k, entity(k + 1, kind != RESIDUE_FREQ && k == 2));
        if (kind == CONTACT) {
            t->model[k] = 1; t->distance[k] = 1.5f + (float)k;
            t->sc_valid[k] = k % 4 != 1;  // rows 1 and 5 are null: one in each validity byte's reach of 9 rows is checked below
            t->sc_dist[k] = 2.f * (float)k; t->sc_dihedral[k] = 3.f * (float)k; t->sc_angle[k] = 4.f * (float)k;
        } else {
            t->n_frames[k] = (uint32_t)k + 1; t->frequency[k] = 0.25f; t->min_distance[k] = 1.f; t->max_distance[k] = 2.f + (float)k;
            if (kind == RESIDUE_FREQ) { t->from.residue[k] = (int32_t)k; t->to.residue[k] = (int32_t)k + 1; }
            if (kind == TIMELINE) { t->tl.first[k] = 0; t->tl.last[k] = (uint32_t)k; t->tl.n_events[k] = 1; t->tl.longest[k] = (uint32_t)k + 1; t->mean_run[k] = 1.f + (float)k; }
        }
    }
    return t;
}

struct Expect { const char *name, *format; };
static std::vector<Expect> expected(Kind kind) {
    std::vector<Expect> side_atom = {{"chain", "u"}, {"resn", "u"}, {"resi", "i"}, {"insertion", "u"}, {"altloc", "u"}, {"atomn", "u"}, {"atomi", "i"}};
    std::vector<Expect> side_res = {{"chain", "u"}, {"resn", "u"}, {"resi", "i"}, {"insertion", "u"}};
    static std::vector<std::string> keep;  // the prefixed names
    keep.reserve(1024);
    std::vector<Expect> out;
    if (kind == CONTACT) out = {{"model", "I"}, {"interaction", "u"}, {"distance", "f"}};
    else out = {{"interaction", "u"}};
    for (const char *prefix : {"from_", "to_"})
        for (const Expect &e : kind == RESIDUE_FREQ ? side_res : side_atom) { keep.push_back(std::string(prefix) + e.name); out.push_back({keep.back().c_str(), e.format}); }
    if (kind == CONTACT) for (const char *n : {"sc_centroid_dist", "sc_dihedral", "sc_centroid_angle"}) out.push_back({n, "f"});
    else {
        out.push_back({"n_frames", "I"});
        for (const char *n : {"frequency", "min_distance", "max_distance"}) out.push_back({n, "f"});
    }
    if (kind == TIMELINE) {
        for (const char *n : {"first_frame", "last_frame", "n_events", "longest_run"}) out.push_back({n, "I"});
        out.push_back({"mean_run", "f"});
    }
    return out;
}

static std::string utf8_at(const ArrowArray *a, size_t i) {
    const int32_t *off = (const int32_t *)a->buffers[1];
    return std::string((const char *)a->buffers[2] + off[i], (size_t)(off[i + 1] - off[i]));
}

static void check_batch(Kind kind, size_t n, const arp_table *t, const ArrowArray &arr, const ArrowSchema &sch) {
    const std::vector<Expect> want = expected(kind);
    CHECK(arr.length == (int64_t)n && arr.null_count == 0 && arr.n_buffers == 1 && arr.buffers[0] == nullptr);
    CHECK(arr.n_children == (int64_t)want.size() && sch.n_children == arr.n_children);
    CHECK(strcmp(sch.format, "+s") == 0 && sch.flags == 0);
    const size_t expect_nulls = kind == CONTACT ? (n > 5 ? 2 : n > 1 ? 1 : 0) : 0;
    for (size_t c = 0; c < want.size(); c++) {
        const ArrowArray *a = arr.children[c];
        const ArrowSchema *s = sch.children[c];
        CHECK(strcmp(s->name, want[c].name) == 0 && strcmp(s->format, want[c].format) == 0);
        const bool sc = strncmp(want[c].name, "sc_", 3) == 0;
        CHECK(s->flags == (sc ? 2 : 0) && s->n_children == 0);
        CHECK(a->length == (int64_t)n && a->offset == 0 && a->n_children == 0);
        CHECK(a->n_buffers == (want[c].format[0] == 'u' ? 3 : 2));
        CHECK(a->null_count == (int64_t)(sc ? expect_nulls : 0));
        CHECK(a->buffers[1] != nullptr);
        if (sc) {
            CHECK(a->buffers[0] != nullptr);
            const uint8_t *bits = (const uint8_t *)a->buffers[0];
            for (size_t i = 0; i < n; i++) CHECK(((bits[i >> 3] >> (i & 7)) & 1u) == (i % 4 != 1 ? 1u : 0u));
            if (n) CHECK((bits[(n - 1) >> 3] >> ((n - 1) & 7 ) >> 1) == 0);  // no bit set past the last row
        } else CHECK(a->buffers[0] == nullptr);
        if (want[c].format[0] == 'u') {
            CHECK(a->buffers[2] != nullptr && ((const int32_t *)a->buffers[1])[0] == 0);
            int32_t total = 0;
            for (size_t i = 0; i < n; i++) total += (int32_t)utf8_at(a, i).size();
            CHECK(((const int32_t *)a->buffers[1])[n] == total);
        }
        // values: every batch column against the column accessor
        int32_t w = 0;
        const void *col = arp_table_column(t, want[c].name, &w);
        CHECK(n == 0 || col != nullptr);
        for (size_t i = 0; i < n; i++) {
            if (strcmp(want[c].name, "interaction") == 0) CHECK(utf8_at(a, i) == kNames[((const int32_t *)col)[i]]);
            else if (want[c].format[0] == 'u') { const char *p = (const char *)col + i * (size_t)w; CHECK(utf8_at(a, i) == std::string(p, strnlen(p, (size_t)w))); }
            else CHECK(w == 4 && memcmp((const char *)a->buffers[1] + 4 * i, (const char *)col + 4 * i, 4) == 0);
        }
    }
    if (n >= 3 && kind != RESIDUE_FREQ) {  // a few values by hand: row 2 names a ring on the `to` side
        const size_t to_atomn = kind == CONTACT ? 15 : 13;
        CHECK(strcmp(sch.children[to_atomn]->name, "to_atomn") == 0 && utf8_at(arr.children[to_atomn], 2) == "Ring" && utf8_at(arr.children[to_atomn], 1) == "CA");
        CHECK(utf8_at(arr.children[kind == CONTACT ? 1 : 0], 2) == "VanDerWaalsContact");
    }
}

// what the table serves and refuses by name (the widths of the vocabulary)
static void check_vocabulary(Kind kind, const arp_table *t) {
    struct Probe { const char *name; int contact, atom, residue; };  // width, 0 = refused; timeline names: width 4 on a timeline table only
    const Probe probes[] = {{"model", 4, 0, 0}, {"interaction", 4, 4, 4}, {"distance", 4, 0, 0}, {"from_chain", 8, 8, 8}, {"to_resn", 8, 8, 8}, {"from_atomn", 8, 8, 0},
                            {"to_insertion", 4, 4, 4}, {"from_altloc", 4, 4, 0}, {"to_resi", 4, 4, 4}, {"from_atomi", 4, 4, 0}, {"to_atom", 4, 4, 0}, {"from_ring", 0, 4, 0},
                            {"to_residue", 0, 0, 4}, {"sc_centroid_dist", 4, 0, 0}, {"sc_dihedral", 4, 0, 0}, {"sc_centroid_angle", 4, 0, 0}, {"sc_valid", 1, 0, 0},
                            {"n_frames", 0, 4, 4}, {"frequency", 0, 4, 4}, {"min_distance", 0, 4, 4}, {"max_distance", 0, 4, 4}, {"nonsense", 0, 0, 0}, {"from_", 0, 0, 0}};
    for (const Probe &p : probes) {
        const int want = kind == CONTACT ? p.contact : kind == RESIDUE_FREQ ? p.residue : p.atom;
        int32_t w = -1;
        const void *col = arp_table_column(t, p.name, &w);
        CHECK((col != nullptr) == (want != 0));
        if (col) CHECK(w == want);
    }
    for (const char *name : {"first_frame", "last_frame", "n_events", "longest_run", "mean_run"}) CHECK((arp_table_column(t, name, nullptr) != nullptr) == (kind == TIMELINE));
    CHECK((arp_table_timeline(t, nullptr, nullptr) != nullptr) == (kind == TIMELINE));
    CHECK(arp_table_similarity(t, nullptr, nullptr, nullptr) == nullptr);
}

int main() {
    int exports = 0;
    for (Kind kind : {CONTACT, ATOM_FREQ, RESIDUE_FREQ, TIMELINE})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)9})
            for (int order = 0; order < 4; order++) {
                arp_table *t = make_table(kind, n);
                if (n) check_vocabulary(kind, t);
                ArrowArray arr;
                ArrowSchema sch;
                CHECK(arp_table_export_arrow(t, &arr, &sch) == ARP_OK);
                check_batch(kind, n, t, arr, sch);
                exports++;
                switch (order) {
                    case 0: arr.release(&arr); sch.release(&sch); arp_table_free(t); break;   // array first
                    case 1: sch.release(&sch); arr.release(&arr); arp_table_free(t); break;   // schema first
                    case 2: {                                                                 // the table goes before the batch: the batch owns copies
                        arp_table_free(t);
                        const std::vector<Expect> want = expected(kind);
                        CHECK(strcmp(sch.children[0]->name, want[0].name) == 0);
                        if (n) CHECK(!utf8_at(arr.children[kind == CONTACT ? 1 : 0], n - 1).empty());
                        sch.release(&sch); arr.release(&arr);
                        break;
                    }
                    default: {                                                                // children moved out first, as a consumer may
                        std::vector<ArrowArray> kids((size_t)arr.n_children);
                        std::vector<ArrowSchema> fields((size_t)sch.n_children);
                        for (int64_t c = 0; c < arr.n_children; c += 2) { kids[(size_t)c] = *arr.children[c]; arr.children[c]->release = nullptr; }
                        for (int64_t c = 1; c < sch.n_children; c += 2) { fields[(size_t)c] = *sch.children[c]; sch.children[c]->release = nullptr; }
                        const int64_t nc = arr.n_children;
                        arr.release(&arr); sch.release(&sch);
                        CHECK(arr.release == nullptr && sch.release == nullptr);
                        arp_table_free(t);
                        for (int64_t c = 0; c < nc; c += 2) {
                            if (n && kids[(size_t)c].n_buffers == 3) (void)utf8_at(&kids[(size_t)c], n - 1);  // the moved child still owns its buffers
                            kids[(size_t)c].release(&kids[(size_t)c]);
                            CHECK(kids[(size_t)c].release == nullptr);
                        }
                        for (int64_t c = 1; c < nc; c += 2) { CHECK(fields[(size_t)c].name[0] != 0); fields[(size_t)c].release(&fields[(size_t)c]); }
                    }
                }
            }
    // arguments
    ArrowArray arr;
    ArrowSchema sch;
    CHECK(arp_table_export_arrow(nullptr, &arr, &sch) == ARP_ERR_BAD_INPUT && strcmp(g_last_error, "null argument") == 0);
    arp_table huge;
    huge.n = 0x7FFFFFF1ull;
    CHECK(arp_table_export_arrow(&huge, &arr, &sch) == ARP_ERR_BAD_INPUT && strcmp(g_last_error, "table too large for 32-bit utf8 offsets") == 0);
    printf("ok: %d exports\n", exports);
    return 0;
}
