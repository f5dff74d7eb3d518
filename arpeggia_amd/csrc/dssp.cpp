// Secondary structure by the rules of Kabsch & Sander 1983: the checks and the host half of arp_dssp (device pipeline: dssp.inl), and
// the definition in plain sequential C++, arp_dssp_host, its yardstick.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "debug_knobs.h"
#include "table.h"

using namespace arp;

namespace {
inline double dist(const double *a, const double *b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

// One frame of the definition (include/arpeggia_amd.h).  x: R x 4 (N, CA, C, O) x 3; code[R]; acc[R][2] and en[R][2] may be null.
struct HostFrame {
    int64_t R;
    const double *x;
    const uint8_t *flags;
    std::vector<uint8_t> brk, donor;
    std::vector<double> h;
    std::vector<uint32_t> best_i;
    std::vector<double> best_e;

    const double *at(int64_t r, int a) const { return x + (r * 4 + a) * 3; }
    bool cont(int64_t a, int64_t b) const {
        if (a < 0 || b >= R || a > b) return false;
        for (int64_t r = a + 1; r <= b; r++)
            if (brk[r]) return false;
        return true;
    }
    bool hb(int64_t i, int64_t j) const {
        if (i < 0 || j < 0 || i >= R || j >= R) return false;
        for (int k = 0; k < 2; k++)
            if (best_i[2 * j + k] == (uint32_t)i && best_e[2 * j + k] < kDsspHbond) return true;
        return false;
    }
    bool turn(int n, int64_t i) const { return cont(i, i + n) && hb(i, i + n); }
    bool pairable(int64_t i, int64_t j) const { return i >= 0 && j >= 0 && i < R && j < R && std::llabs(i - j) >= 3 && cont(i - 1, i + 1) && cont(j - 1, j + 1); }
    bool par(int64_t i, int64_t j) const { return pairable(i, j) && ((hb(i - 1, j) && hb(j, i + 1)) || (hb(j - 1, i) && hb(i, j + 1))); }
    bool anti(int64_t i, int64_t j) const { return pairable(i, j) && ((hb(i, j) && hb(j, i)) || (hb(i - 1, j + 1) && hb(j - 1, i + 1))); }

    void bonds() {
        brk.assign(R, 0); donor.assign(R, 0); h.assign(R * 3, 0.0);
        best_i.assign(R * 2, ARP_NONE);
        best_e.assign(R * 2, std::numeric_limits<double>::infinity());
        for (int64_t r = 0; r < R; r++) {
            brk[r] = r == 0 || (flags[r] & ARP_DSSP_CHAIN_START) || dist(at(r - 1, 2), at(r, 0)) > kDsspBreak;
            donor[r] = !brk[r] && !(flags[r] & ARP_DSSP_NO_H);
            if (!donor[r]) continue;
            const double *c = at(r - 1, 2), *o = at(r - 1, 3), *n = at(r, 0);
            const double len = dist(c, o);
            for (int k = 0; k < 3; k++) h[3 * r + k] = n[k] + (c[k] - o[k]) / len;
        }
        for (int64_t j = 0; j < R; j++) {
            if (!donor[j]) continue;
            const double *nj = at(j, 0), *hj = &h[3 * j];
            for (int64_t i = 0; i < R; i++) {
                if (i == j || i + 1 == j) continue;
                if (!(dist(at(i, 1), at(j, 1)) < kDsspCaCut)) continue;
                const double d_on = dist(at(i, 3), nj), d_ch = dist(at(i, 2), hj), d_oh = dist(at(i, 3), hj), d_cn = dist(at(i, 2), nj);
                double e = kDsspCoupling * (((1.0 / d_on + 1.0 / d_ch) - 1.0 / d_oh) - 1.0 / d_cn);
                if (d_on < kDsspMinDist || d_ch < kDsspMinDist || d_oh < kDsspMinDist || d_cn < kDsspMinDist) e = kDsspMinEnergy;
                uint32_t *bi = &best_i[2 * j];
                double *be = &best_e[2 * j];
                if (e < be[0]) { be[1] = be[0]; bi[1] = bi[0]; be[0] = e; bi[0] = (uint32_t)i; }
                else if (e < be[1]) { be[1] = e; bi[1] = (uint32_t)i; }
            }
        }
    }

    void states(uint8_t *code) const {
        enum { LOOP = 0, H = 1, B = 2, E = 3, G = 4, I = 5, T = 6, S = 7 };
        std::fill(code, code + R, (uint8_t)LOOP);
        for (int64_t i = 0; i < R; i++) {
            bool bridge = false, ladder = false;
            for (int64_t j = 0; j < R; j++) {
                const bool p = par(i, j), a = anti(i, j);
                bridge = bridge || p || a;
                ladder = ladder || (p && (par(i - 1, j - 1) || par(i + 1, j + 1))) || (a && (anti(i - 1, j + 1) || anti(i + 1, j - 1)));
            }
            if (bridge) code[i] = B;
            if (ladder) code[i] = E;
        }
        for (int64_t i = 0; i < R; i++)
            if (turn(4, i - 1) && turn(4, i))
                for (int64_t k = i; k < i + 4; k++) code[k] = H;
        const int helix[2][2] = {{3, G}, {5, I}};
        for (const auto &hx : helix) {
            const int n = hx[0];
            const uint8_t state = (uint8_t)hx[1];
            for (int64_t i = 0; i < R; i++) {
                if (!(turn(n, i - 1) && turn(n, i))) continue;
                bool open = true;
                for (int64_t k = i; k < i + n; k++) open = open && (code[k] == LOOP || code[k] == state);
                if (open)
                    for (int64_t k = i; k < i + n; k++) code[k] = state;
            }
        }
        for (int64_t k = 0; k < R; k++) {
            if (code[k] != LOOP) continue;
            for (int n = 3; n <= 5; n++)
                for (int64_t i = k - n + 1; i < k; i++)
                    if (turn(n, i)) code[k] = T;
        }
        for (int64_t k = 0; k < R; k++) {
            if (code[k] != LOOP || !cont(k - 2, k + 2)) continue;
            const double *a = at(k - 2, 1), *b = at(k, 1), *c = at(k + 2, 1);
            const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - b[0], vy = c[1] - b[1], vz = c[2] - b[2];
            const double dot = (ux * vx + uy * vy) + uz * vz;
            const double lu = std::sqrt((ux * ux + uy * uy) + uz * uz), lv = std::sqrt((vx * vx + vy * vy) + vz * vz);
            if (dot / (lu * lv) < kDsspCos70) code[k] = S;
        }
    }
};

arp_status flags_check(const uint8_t *flags, uint64_t n_res) {
    if (n_res == 0) { set_error("dssp: no residues (n_res == 0)"); return ARP_ERR_BAD_INPUT; }
    if (n_res >= kDsspMaxRes) { set_error("dssp: %llu residues, at most 2^28 - 1 are supported", (unsigned long long)n_res); return ARP_ERR_BAD_INPUT; }
    if (!flags) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t r = 0; r < n_res; r++)
        if (flags[r] & ~(ARP_DSSP_CHAIN_START | ARP_DSSP_NO_H)) {
            set_error("dssp: flags[%llu] = %u has a bit other than CHAIN_START (1) and NO_H (2)", (unsigned long long)r, (unsigned)flags[r]);
            return ARP_ERR_BAD_INPUT;
        }
    return ARP_OK;
}
}  // namespace

extern "C" arp_status arp_dssp_host(uint64_t n_frames, uint64_t n_res, const double *bb_xyz, const uint8_t *flags, uint8_t *codes, uint32_t *counts, uint32_t *frame_counts,
                                    uint32_t *hb_acceptor, float *hb_energy) try {
    const uint64_t F = n_frames, R = n_res;
    if (F == 0) { set_error("dssp: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    arp_status st = flags_check(flags, R);
    if (st != ARP_OK) return st;
    if (!bb_xyz || !counts) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t v = 0; v < F * R * 12; v++)
        if (!std::isfinite(bb_xyz[v])) {
            set_error("dssp: non-finite coordinate in frame %llu, residue %llu", (unsigned long long)(v / (12 * R)), (unsigned long long)(v / 12 % R));
            return ARP_ERR_BAD_INPUT;
        }
    std::fill(counts, counts + R * 8, 0u);
    std::vector<uint8_t> code(R);
    HostFrame hf;
    hf.R = (int64_t)R; hf.flags = flags;
    for (uint64_t f = 0; f < F; f++) {
        hf.x = bb_xyz + f * R * 12;
        hf.bonds();
        hf.states(code.data());
        uint32_t hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t r = 0; r < R; r++) { counts[r * 8 + code[r]]++; hist[code[r]]++; }
        if (codes) std::copy(code.begin(), code.end(), codes + f * R);
        if (frame_counts) std::copy(hist, hist + 8, frame_counts + f * 8);
        for (uint64_t e = 0; e < R * 2; e++) {
            const bool none = hf.best_i[e] == ARP_NONE;
            if (hb_acceptor) hb_acceptor[f * R * 2 + e] = hf.best_i[e];
            if (hb_energy) hb_energy[f * R * 2 + e] = none ? 0.0f : (float)hf.best_e[e];
        }
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_dssp(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *bb, const uint8_t *flags, uint64_t n_res, uint8_t *codes,
                               uint32_t *counts, uint32_t *frame_counts, uint32_t *hb_acceptor, float *hb_energy) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsd_frames_check(s, n_frames, xyz, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if (F >= (1ull << 32)) { set_error("dssp: 2^32 or more frames"); return ARP_ERR_BAD_INPUT; }
    if ((st = flags_check(flags, n_res)) != ARP_OK) return st;
    if (!bb) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t e = 0; e < n_res * 4; e++)
        if (bb[e] >= n0) {
            set_error("dssp: bb[%llu][%llu] = %u is not an atom of the topology (%llu atoms)", (unsigned long long)(e / 4), (unsigned long long)(e % 4), bb[e], (unsigned long long)n0);
            return ARP_ERR_BAD_INPUT;
        }
    if (!ctx) return ARP_OK;  // validation only
    if (!counts) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    DsspJob job;
    job.n_atoms = n0; job.n_frames = F; job.n_res = n_res; job.xyz = frames; job.bb = bb; job.flags = flags;
    job.chunk_atoms = g_debug.rmsd_chunk_atoms > 0 ? (uint64_t)g_debug.rmsd_chunk_atoms : 0u;
    DsspOut out;
    out.codes = codes; out.counts = counts; out.frame_counts = frame_counts; out.hb_acceptor = hb_acceptor; out.hb_energy = hb_energy;
    return device_dssp(ctx, job, &out);
} ARP_ABI_CATCH
