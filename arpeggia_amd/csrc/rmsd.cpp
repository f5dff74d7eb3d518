// RMSD between the frames of an ensemble after optimal superposition: the checks and the host half of arp_rmsd_matrix,
// arp_rmsd_reference and arp_rmsd_clusters (device pipeline: rmsd.inl), and the definition in plain sequential C++, arp_rmsd_host, their yardstick.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "debug_knobs.h"
#include "table.h"

using namespace arp;

namespace {
// The largest eigenvalue of a symmetric 4 x 4 matrix by cyclic Jacobi rotations (the upper triangle is used and destroyed).
double jacobi_top(double a[4][4]) {
    for (int sweep = 0; sweep < 32; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 4; p++) { diag += std::fabs(a[p][p]); for (int q = p + 1; q < 4; q++) off += std::fabs(a[p][q]); }
        if (off <= 1e-300 || off <= 1e-19 * diag) break;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = a[p][q];
                if (std::fabs(apq) <= 1e-300) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                a[p][p] -= t * apq; a[q][q] += t * apq; a[p][q] = 0.0;
                for (int k = 0; k < 4; k++) {
                    if (k == p || k == q) continue;
                    double &akp = k < p ? a[k][p] : a[p][k], &akq = k < q ? a[k][q] : a[q][k];
                    const double x = akp, y = akq;
                    akp = cs * x - sn * y;
                    akq = sn * x + cs * y;
                }
            }
    }
    return std::max(std::max(a[0][0], a[1][1]), std::max(a[2][2], a[3][3]));
}

}  // namespace

namespace arp {
uint64_t rmsd_cap() { return g_debug.rmsd_cap_bytes > 0 ? (uint64_t)g_debug.rmsd_cap_bytes : (1ull << 31); }

// The frame checks of the frequency call with its statuses and messages.  *frames: the coordinates (xyz, or the models' in `model_xyz`), *n0: the topology's
// atoms, *F: the frames.  (arp_dssp, which takes no selection, stops here.)
arp_status rmsd_frames_check(const arp_structure *s, uint64_t n_frames, const double *xyz, std::vector<double> *model_xyz, const double **frames, uint64_t *n0_out, uint64_t *F_out) {
    if (!s) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    uint64_t n0 = 0, r0 = 0, nm = 1;
    arp_status st = freq_topology(s, xyz == nullptr, &n0, &r0, &nm);
    if (st != ARP_OK) return st;
    const uint64_t F = xyz ? n_frames : nm;
    if (F == 0) { set_error("contact frequencies: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    if (n0 >= (1ull << 29)) { set_error("contact frequencies: the topology has %llu atoms, at most 2^29 - 1 are supported", (unsigned long long)n0); return ARP_ERR_BAD_INPUT; }
    if (F > (1ull << 40) / std::max<uint64_t>(n0, 1)) { set_error("contact frequencies: too many frames"); return ARP_ERR_BAD_INPUT; }
    if (!xyz) {  // the models' coordinates as F x n0 x 3
        model_xyz->resize(F * n0 * 3);
        for (uint64_t a = 0; a < F * n0; a++) { (*model_xyz)[3 * a] = s->x[a]; (*model_xyz)[3 * a + 1] = s->y[a]; (*model_xyz)[3 * a + 2] = s->z[a]; }
        xyz = model_xyz->data();
    }
    const uint64_t nv = F * n0 * 3;
    for (uint64_t v = 0; v < nv; v++)
        if (!std::isfinite(xyz[v])) {
            set_error("contact frequencies: non-finite coordinate in frame %llu, atom %llu", (unsigned long long)(v / (3 * n0)), (unsigned long long)(v / 3 % n0));
            return ARP_ERR_BAD_INPUT;
        }
    *frames = xyz; *n0_out = n0; *F_out = F;
    return ARP_OK;
}

// What the three device calls check before the device is touched: the frame checks, then the selection.
arp_status rmsd_check(const char *what, const arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, std::vector<double> *model_xyz,
                      const double **frames, uint64_t *n0_out, uint64_t *F_out) {
    const arp_status st = rmsd_frames_check(s, n_frames, xyz, model_xyz, frames, n0_out, F_out);
    if (st != ARP_OK) return st;
    const uint64_t n0 = *n0_out, F = *F_out;
    if (n_sel == 0) { set_error("%s: the selection is empty (n_sel == 0)", what); return ARP_ERR_BAD_INPUT; }
    if (!sel) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t i = 0; i < n_sel; i++) {
        if (sel[i] >= n0) { set_error("%s: sel[%llu] = %u is not an atom of the topology (%llu atoms)", what, (unsigned long long)i, sel[i], (unsigned long long)n0); return ARP_ERR_BAD_INPUT; }
        if (i && sel[i] <= sel[i - 1]) {
            set_error("%s: sel is not strictly increasing at index %llu (%u after %u)", what, (unsigned long long)i, sel[i], sel[i - 1]);
            return ARP_ERR_BAD_INPUT;
        }
    }
    if (F >= (1ull << 32)) { set_error("%s: 2^32 or more frames", what); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}

}  // namespace arp

namespace {
// the packed frames X[F][3][n_pad] and G[F] stay on the device for the call
arp_status rmsd_packed_cap(const char *what, uint64_t F, uint64_t n) {
    const uint64_t need = F * 3u * rmsd_n_pad(n) * 8u + F * 8u;
    if (need > rmsd_cap()) {
        set_error("%s: the packed coordinates of %llu frames (F) x %llu selected atoms (n) need %llu bytes, the limit is %llu (rmsd_cap_bytes)", what, (unsigned long long)F,
                  (unsigned long long)n, (unsigned long long)need, (unsigned long long)rmsd_cap());
        return ARP_ERR_CAPACITY;
    }
    return ARP_OK;
}

RmsdJob rmsd_job(RmsdJob::Kind kind, uint64_t n0, uint64_t F, const double *frames, const uint32_t *sel, uint64_t n_sel) {
    RmsdJob j;
    j.kind = kind; j.n_atoms = n0; j.n_frames = F; j.n_sel = n_sel; j.xyz = frames; j.sel = sel;
    j.chunk_atoms = g_debug.rmsd_chunk_atoms > 0 ? (uint64_t)g_debug.rmsd_chunk_atoms : 0u;
    return j;
}
}  // namespace

// The definition (include/arpeggia_amd.h) in plain sequential C++: f64 throughout, the sums in the order of the atoms, cyclic Jacobi on K(S).
extern "C" arp_status arp_rmsd_host(uint64_t n_frames, uint64_t n, const double *xyz_sel, float *out) try {
    if (n_frames && (!out || (n && !xyz_sel))) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (n_frames && n == 0) { set_error("rmsd: the selection is empty (n == 0)"); return ARP_ERR_BAD_INPUT; }
    const uint64_t F = n_frames;
    if (F > 46340u) { set_error("rmsd: the host definition fills an F x F matrix, %llu frames are too many for it", (unsigned long long)F); return ARP_ERR_CAPACITY; }
    for (uint64_t v = 0; v < F * n * 3; v++)
        if (!std::isfinite(xyz_sel[v])) { set_error("rmsd: non-finite coordinate in frame %llu, atom %llu", (unsigned long long)(v / (3 * n)), (unsigned long long)(v / 3 % n)); return ARP_ERR_BAD_INPUT; }
    std::vector<double> x(F * n * 3), g(F);
    for (uint64_t f = 0; f < F; f++) {
        const double *p = xyz_sel + f * n * 3;
        double c[3] = {0.0, 0.0, 0.0};
        for (uint64_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) c[k] += p[3 * i + k];
        for (int k = 0; k < 3; k++) c[k] /= (double)n;
        double sum = 0.0;
        for (uint64_t i = 0; i < n; i++) {
            double d[3];
            for (int k = 0; k < 3; k++) x[(f * n + i) * 3 + k] = d[k] = p[3 * i + k] - c[k];
            sum += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        }
        g[f] = sum;
    }
    for (uint64_t f = 0; f < F; f++) {
        out[f * F + f] = 0.0f;
        for (uint64_t h = f + 1; h < F; h++) {
            double s[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            const double *a = x.data() + f * n * 3, *b = x.data() + h * n * 3;
            for (uint64_t i = 0; i < n; i++)
                for (int u = 0; u < 3; u++) for (int v = 0; v < 3; v++) s[u][v] += a[3 * i + u] * b[3 * i + v];
            double k[4][4] = {};
            k[0][0] = (s[0][0] + s[1][1]) + s[2][2];
            k[1][1] = (s[0][0] - s[1][1]) - s[2][2];
            k[2][2] = (-s[0][0] + s[1][1]) - s[2][2];
            k[3][3] = (-s[0][0] - s[1][1]) + s[2][2];
            k[0][1] = s[1][2] - s[2][1]; k[0][2] = s[2][0] - s[0][2]; k[0][3] = s[0][1] - s[1][0];
            k[1][2] = s[0][1] + s[1][0]; k[1][3] = s[2][0] + s[0][2]; k[2][3] = s[1][2] + s[2][1];
            const double lambda = jacobi_top(k);
            const double msd = std::max(0.0, (g[f] + g[h] - 2.0 * lambda) / (double)n);
            out[f * F + h] = out[h * F + f] = (float)std::sqrt(msd);
        }
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_rmsd_matrix(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, float *out) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsd_check("rmsd matrix", s, n_frames, xyz, sel, n_sel, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if (!ctx) return ARP_OK;  // validation only
    if (!out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (F * F * 4u > rmsd_cap()) {
        set_error("rmsd matrix: the matrix of %llu frames (F) needs %llu bytes, the limit is %llu (rmsd_cap_bytes); arp_rmsd_clusters keeps one bit per pair",
                  (unsigned long long)F, (unsigned long long)(F * F * 4u), (unsigned long long)rmsd_cap());
        return ARP_ERR_CAPACITY;
    }
    if ((st = rmsd_packed_cap("rmsd matrix", F, n_sel)) != ARP_OK) return st;
    return device_rmsd(ctx, rmsd_job(RmsdJob::kMatrix, n0, F, frames, sel, n_sel), out, nullptr);
} ARP_ABI_CATCH

extern "C" arp_status arp_rmsd_reference(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const double *ref_xyz,
                                         uint64_t ref_frame, float *out) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsd_check("rmsd reference", s, n_frames, xyz, sel, n_sel, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if (!ref_xyz && ref_frame >= F) { set_error("rmsd reference: ref_frame %llu is not one of the %llu frames", (unsigned long long)ref_frame, (unsigned long long)F); return ARP_ERR_BAD_INPUT; }
    if (ref_xyz)
        for (uint64_t v = 0; v < n0 * 3; v++)
            if (!std::isfinite(ref_xyz[v])) { set_error("rmsd reference: non-finite coordinate in ref_xyz, atom %llu", (unsigned long long)(v / 3)); return ARP_ERR_BAD_INPUT; }
    if (!ctx) return ARP_OK;  // validation only
    if (!out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if ((st = rmsd_packed_cap("rmsd reference", F, n_sel)) != ARP_OK) return st;
    RmsdJob job = rmsd_job(RmsdJob::kReference, n0, F, frames, sel, n_sel);
    job.ref_xyz = ref_xyz; job.ref_frame = ref_xyz ? 0u : ref_frame;
    return device_rmsd(ctx, job, out, nullptr);
} ARP_ABI_CATCH

extern "C" arp_status arp_rmsd_clusters(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, float cutoff,
                                        uint32_t max_clusters, uint32_t *cluster, float *rmsd_to_centre, uint32_t *n_neighbours, uint32_t *centre, uint32_t *cluster_size,
                                        uint32_t *n_clusters) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsd_check("rmsd clusters", s, n_frames, xyz, sel, n_sel, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if (!std::isfinite(cutoff) || cutoff < 0.0f) { set_error("rmsd clusters: cutoff must be finite and not negative, got %g", (double)cutoff); return ARP_ERR_BAD_INPUT; }
    if (max_clusters == 0) { set_error("rmsd clusters: max_clusters must be at least 1 (ARP_NONE: no limit)"); return ARP_ERR_BAD_INPUT; }
    if (!ctx) return ARP_OK;  // validation only
    if (!cluster || !rmsd_to_centre || !n_neighbours || !centre || !cluster_size || !n_clusters) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const uint64_t bits = F >= (1ull << 20) ? ~0ull : F * ((F + 31u) / 32u) * 4u;  // (2^20 frames: the tile triangle of one launch)
    if (bits > rmsd_cap()) {
        set_error("rmsd clusters: the neighbour bits of %llu frames (F) need %llu bytes, the limit is %llu (rmsd_cap_bytes)", (unsigned long long)F, (unsigned long long)bits,
                  (unsigned long long)rmsd_cap());
        return ARP_ERR_CAPACITY;
    }
    if ((st = rmsd_packed_cap("rmsd clusters", F, n_sel)) != ARP_OK) return st;
    RmsdJob job = rmsd_job(RmsdJob::kClusters, n0, F, frames, sel, n_sel);
    job.cutoff = cutoff; job.max_clusters = max_clusters;
    ClustersHost c;
    if ((st = device_rmsd(ctx, job, nullptr, &c)) != ARP_OK) return st;
    std::copy(c.cluster.begin(), c.cluster.end(), cluster);
    if (F) memcpy(rmsd_to_centre, c.sim.data(), F * 4u);
    std::copy(c.n_neighbours.begin(), c.n_neighbours.end(), n_neighbours);
    std::copy(c.centre.begin(), c.centre.end(), centre);
    std::copy(c.cluster_size.begin(), c.cluster_size.end(), cluster_size);
    *n_clusters = (uint32_t)c.n_clusters;
    return ARP_OK;
} ARP_ABI_CATCH
