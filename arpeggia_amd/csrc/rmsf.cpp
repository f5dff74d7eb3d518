// RMSF and the mean structure: the checks and the host half of arp_rmsf (device pipeline: rmsf.inl), and the definition in plain
// sequential C++, arp_rmsf_host, its yardstick.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "debug_knobs.h"
#include "table.h"

using namespace arp;

namespace {
// A unit eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix by cyclic Jacobi rotations with the rotations accumulated (the upper triangle is
// used and destroyed): the column of the largest diagonal entry, the lowest index on ties.
void jacobi_vec(double a[4][4], double q[4]) {
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 32; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 4; p++) { diag += std::fabs(a[p][p]); for (int r = p + 1; r < 4; r++) off += std::fabs(a[p][r]); }
        if (off <= 1e-300 || off <= 1e-19 * diag) break;
        for (int p = 0; p < 3; p++)
            for (int r = p + 1; r < 4; r++) {
                const double apq = a[p][r];
                if (std::fabs(apq) <= 1e-300) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * apq);
                const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                a[p][p] -= t * apq; a[r][r] += t * apq; a[p][r] = 0.0;
                for (int k = 0; k < 4; k++) {
                    const double vx = v[k][p], vy = v[k][r];
                    v[k][p] = cs * vx - sn * vy;
                    v[k][r] = sn * vx + cs * vy;
                    if (k == p || k == r) continue;
                    double &akp = k < p ? a[k][p] : a[p][k], &akq = k < r ? a[k][r] : a[r][k];
                    const double x = akp, y = akq;
                    akp = cs * x - sn * y;
                    akq = sn * x + cs * y;
                }
            }
    }
    int top = 0;
    for (int p = 1; p < 4; p++)
        if (a[p][p] > a[top][top]) top = p;
    for (int k = 0; k < 4; k++) q[k] = v[k][top];
}

// R (row-major) of the top eigenvector of K(S), S = sum_i x_i T_i^T
void rotation_of(const double s[3][3], double r[9]) {
    double k[4][4] = {}, q[4];
    k[0][0] = (s[0][0] + s[1][1]) + s[2][2];
    k[1][1] = (s[0][0] - s[1][1]) - s[2][2];
    k[2][2] = (-s[0][0] + s[1][1]) - s[2][2];
    k[3][3] = (-s[0][0] - s[1][1]) + s[2][2];
    k[0][1] = s[1][2] - s[2][1]; k[0][2] = s[2][0] - s[0][2]; k[0][3] = s[0][1] - s[1][0];
    k[1][2] = s[0][1] + s[1][0]; k[1][3] = s[2][0] + s[0][2]; k[2][3] = s[1][2] + s[2][1];
    jacobi_vec(k, q);
    const double norm = std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double w = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
    r[0] = ((w * w + x * x) - y * y) - z * z; r[1] = 2.0 * (x * y - w * z);                r[2] = 2.0 * (x * z + w * y);
    r[3] = 2.0 * (y * x + w * z);               r[4] = ((w * w - x * x) + y * y) - z * z;  r[5] = 2.0 * (y * z - w * x);
    r[6] = 2.0 * (z * x - w * y);               r[7] = 2.0 * (z * y + w * x);              r[8] = ((w * w - x * x) - y * y) + z * z;
}

inline void rotate(const double *r, const double *x, double *y) {
    for (int k = 0; k < 3; k++) y[k] = (r[3 * k] * x[0] + r[3 * k + 1] * x[1]) + r[3 * k + 2] * x[2];
}

arp_status rounds_check(const char *what, uint32_t max_rounds, double tol) {
    if (max_rounds == 0) { set_error("%s: max_rounds must be at least 1 (1: the fit to a fixed reference)", what); return ARP_ERR_BAD_INPUT; }
    if (!std::isfinite(tol) || tol < 0.0) { set_error("%s: tol must be finite and not negative, got %g", what, tol); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
}  // namespace

// The definition (include/arpeggia_amd.h) in plain sequential C++ on already-selected coordinates: f64 throughout, every sum in the order of its index.
extern "C" arp_status arp_rmsf_host(uint64_t n_frames, uint64_t n, uint64_t m, const double *xyz_sel, const double *xyz_msel, const double *ref_sel, uint64_t ref_frame,
                                    uint32_t max_rounds, double tol, double *mean, float *rmsf, float *frame_rmsd, double *transforms, double *aligned, uint32_t *n_rounds,
                                    double *last_change) try {
    const uint64_t F = n_frames;
    if (F == 0) { set_error("rmsf: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    if (n == 0) { set_error("rmsf: the selection is empty (n == 0)"); return ARP_ERR_BAD_INPUT; }
    if (m == 0) { set_error("rmsf: the measured selection is empty (m == 0)"); return ARP_ERR_BAD_INPUT; }
    if (!xyz_sel || !mean || !rmsf || !frame_rmsd || !n_rounds || !last_change) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (!xyz_msel && m != n) { set_error("rmsf: xyz_msel == NULL measures the fit atoms, m must equal n (%llu), got %llu", (unsigned long long)n, (unsigned long long)m); return ARP_ERR_BAD_INPUT; }
    arp_status st = rounds_check("rmsf", max_rounds, tol);
    if (st != ARP_OK) return st;
    if (!ref_sel && ref_frame >= F) { set_error("rmsf: ref_frame %llu is not one of the %llu frames", (unsigned long long)ref_frame, (unsigned long long)F); return ARP_ERR_BAD_INPUT; }
    for (uint64_t v = 0; v < F * n * 3; v++)
        if (!std::isfinite(xyz_sel[v])) { set_error("rmsf: non-finite coordinate in frame %llu, atom %llu", (unsigned long long)(v / (3 * n)), (unsigned long long)(v / 3 % n)); return ARP_ERR_BAD_INPUT; }
    if (xyz_msel)
        for (uint64_t v = 0; v < F * m * 3; v++)
            if (!std::isfinite(xyz_msel[v])) { set_error("rmsf: non-finite measured coordinate in frame %llu, atom %llu", (unsigned long long)(v / (3 * m)), (unsigned long long)(v / 3 % m)); return ARP_ERR_BAD_INPUT; }
    if (ref_sel)
        for (uint64_t v = 0; v < n * 3; v++)
            if (!std::isfinite(ref_sel[v])) { set_error("rmsf: non-finite coordinate in ref_sel, atom %llu", (unsigned long long)(v / 3)); return ARP_ERR_BAD_INPUT; }
    // The centroid in two steps: c0 the mean, then r the mean of what is left after subtracting it.  c0 carries the rounding of a sum of absolute
    // coordinates, r finds that error to the rounding of the centred ones; coordinates are centred as (p - c0) - r, the centroid reported is c0 + r.
    auto centroid = [n](const double *p, double *c0, double *r) {
        for (int k = 0; k < 3; k++) c0[k] = r[k] = 0.0;
        for (uint64_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) c0[k] += p[3 * i + k];
        for (int k = 0; k < 3; k++) c0[k] /= (double)n;
        for (uint64_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) r[k] += p[3 * i + k] - c0[k];
        for (int k = 0; k < 3; k++) r[k] /= (double)n;
    };
    std::vector<double> x(F * n * 3), xm_own(xyz_msel ? F * m * 3 : 0), c(F * 3), target(n * 3), M(n * 3), R(F * 9);
    double c0[3], r[3];
    for (uint64_t f = 0; f < F; f++) {
        centroid(xyz_sel + f * n * 3, c0, r);
        for (int k = 0; k < 3; k++) c[f * 3 + k] = c0[k] + r[k];
        for (uint64_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) x[(f * n + i) * 3 + k] = (xyz_sel[(f * n + i) * 3 + k] - c0[k]) - r[k];
        if (xyz_msel)
            for (uint64_t i = 0; i < m; i++) for (int k = 0; k < 3; k++) xm_own[(f * m + i) * 3 + k] = (xyz_msel[(f * m + i) * 3 + k] - c0[k]) - r[k];
    }
    const double *xm = xyz_msel ? xm_own.data() : x.data();
    double c_t[3];
    if (ref_sel) {
        centroid(ref_sel, c0, r);
        for (int k = 0; k < 3; k++) c_t[k] = c0[k] + r[k];
        for (uint64_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) target[3 * i + k] = (ref_sel[3 * i + k] - c0[k]) - r[k];
    } else {
        for (int k = 0; k < 3; k++) c_t[k] = c[ref_frame * 3 + k];
        std::copy(x.begin() + ref_frame * n * 3, x.begin() + (ref_frame + 1) * n * 3, target.begin());
    }
    uint32_t round = 0;
    double change = 0.0;
    for (;;) {
        round++;
        std::fill(M.begin(), M.end(), 0.0);
        for (uint64_t f = 0; f < F; f++) {
            double s[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            const double *a = x.data() + f * n * 3;
            for (uint64_t i = 0; i < n; i++)
                for (int u = 0; u < 3; u++) for (int v = 0; v < 3; v++) s[u][v] += a[3 * i + u] * target[3 * i + v];
            rotation_of(s, &R[f * 9]);
            for (uint64_t i = 0; i < n; i++) {
                double y[3];
                rotate(&R[f * 9], a + 3 * i, y);
                for (int k = 0; k < 3; k++) M[3 * i + k] += y[k];
            }
        }
        double d2 = 0.0;
        for (uint64_t v = 0; v < n * 3; v++) { M[v] /= (double)F; const double d = M[v] - target[v]; d2 += d * d; }
        change = std::sqrt(d2 / (double)n);
        if (round == max_rounds || change <= tol) break;
        target = M;
    }
    // the measured atoms under the last rotations
    std::vector<double> mm(m * 3, 0.0), dev(m, 0.0);
    for (uint64_t f = 0; f < F; f++)
        for (uint64_t i = 0; i < m; i++) {
            double y[3];
            rotate(&R[f * 9], xm + (f * m + i) * 3, y);
            for (int k = 0; k < 3; k++) mm[3 * i + k] += y[k];
        }
    for (uint64_t v = 0; v < m * 3; v++) mm[v] /= (double)F;
    for (uint64_t f = 0; f < F; f++) {
        for (uint64_t i = 0; i < m; i++) {
            double y[3];
            rotate(&R[f * 9], xm + (f * m + i) * 3, y);
            const double d0 = y[0] - mm[3 * i], d1 = y[1] - mm[3 * i + 1], d2 = y[2] - mm[3 * i + 2];
            dev[i] += (d0 * d0 + d1 * d1) + d2 * d2;
            if (aligned) for (int k = 0; k < 3; k++) aligned[(f * m + i) * 3 + k] = y[k] + c_t[k];
        }
        double s = 0.0;
        for (uint64_t i = 0; i < n; i++) {
            double y[3];
            rotate(&R[f * 9], x.data() + (f * n + i) * 3, y);
            const double d0 = y[0] - M[3 * i], d1 = y[1] - M[3 * i + 1], d2 = y[2] - M[3 * i + 2];
            s += (d0 * d0 + d1 * d1) + d2 * d2;
        }
        frame_rmsd[f] = (float)std::sqrt(s / (double)n);
        if (transforms) {
            double *t = transforms + f * 12, rc[3];
            std::copy(&R[f * 9], &R[f * 9] + 9, t);
            rotate(&R[f * 9], &c[f * 3], rc);
            for (int k = 0; k < 3; k++) t[9 + k] = c_t[k] - rc[k];
        }
    }
    for (uint64_t i = 0; i < m; i++) {
        rmsf[i] = (float)std::sqrt(dev[i] / (double)F);
        for (int k = 0; k < 3; k++) mean[3 * i + k] = mm[3 * i + k] + c_t[k];
    }
    *n_rounds = round;
    *last_change = change;
    return ARP_OK;
} ARP_ABI_CATCH

uint64_t arp::rmsf_resident_bytes(uint64_t F, uint64_t n_sel, uint64_t m, bool own_msel) {
    return F * 3u * rmsd_n_pad(n_sel) * 8u + F * 8u + (own_msel ? F * 3u * rmsd_n_pad(m) * 8u : 0u);  // X, G and XM stay resident
}

arp_status arp::rmsf_check(const char *what, const arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const uint32_t *msel, uint64_t n_msel,
                           const double *ref_xyz, uint64_t ref_frame, uint32_t max_rounds, double tol, std::vector<double> *model_xyz, const double **frames, uint64_t *n0_out,
                           uint64_t *F_out) {
    arp_status st = rmsd_check(what, s, n_frames, xyz, sel, n_sel, model_xyz, frames, n0_out, F_out);
    if (st != ARP_OK) return st;
    const uint64_t n0 = *n0_out, F = *F_out;
    if (msel) {
        if (n_msel == 0) { set_error("%s: the measured selection is empty (n_msel == 0)", what); return ARP_ERR_BAD_INPUT; }
        for (uint64_t i = 0; i < n_msel; i++) {
            if (msel[i] >= n0) { set_error("%s: msel[%llu] = %u is not an atom of the topology (%llu atoms)", what, (unsigned long long)i, msel[i], (unsigned long long)n0); return ARP_ERR_BAD_INPUT; }
            if (i && msel[i] <= msel[i - 1]) {
                set_error("%s: msel is not strictly increasing at index %llu (%u after %u)", what, (unsigned long long)i, msel[i], msel[i - 1]);
                return ARP_ERR_BAD_INPUT;
            }
        }
    }
    if ((st = rounds_check(what, max_rounds, tol)) != ARP_OK) return st;
    if (!ref_xyz && ref_frame >= F) { set_error("%s: ref_frame %llu is not one of the %llu frames", what, (unsigned long long)ref_frame, (unsigned long long)F); return ARP_ERR_BAD_INPUT; }
    if (ref_xyz)
        for (uint64_t v = 0; v < n0 * 3; v++)
            if (!std::isfinite(ref_xyz[v])) { set_error("%s: non-finite coordinate in ref_xyz, atom %llu", what, (unsigned long long)(v / 3)); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}

extern "C" arp_status arp_rmsf(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const uint32_t *msel, uint64_t n_msel,
                               const double *ref_xyz, uint64_t ref_frame, uint32_t max_rounds, double tol, double *mean, float *rmsf, float *frame_rmsd, double *transforms,
                               double *aligned, uint32_t *n_rounds, double *last_change) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsf_check("rmsf", s, n_frames, xyz, sel, n_sel, msel, n_msel, ref_xyz, ref_frame, max_rounds, tol, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if (!ctx) return ARP_OK;  // validation only
    if (!mean || !rmsf || !frame_rmsd || !n_rounds || !last_change) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const uint64_t m = msel ? n_msel : n_sel;
    const uint64_t need = rmsf_resident_bytes(F, n_sel, m, msel != nullptr);
    if (need > rmsd_cap()) {
        set_error("rmsf: the packed coordinates of %llu frames (F) x %llu fit atoms (n) and %llu measured atoms (m) need %llu bytes, the limit is %llu (rmsd_cap_bytes)",
                  (unsigned long long)F, (unsigned long long)n_sel, (unsigned long long)m, (unsigned long long)need, (unsigned long long)rmsd_cap());
        return ARP_ERR_CAPACITY;
    }
    RmsfJob job;
    job.n_atoms = n0; job.n_frames = F; job.n_sel = n_sel; job.n_msel = m; job.xyz = frames; job.sel = sel; job.msel = msel;
    job.chunk_atoms = g_debug.rmsd_chunk_atoms > 0 ? (uint64_t)g_debug.rmsd_chunk_atoms : 0u;
    job.ref_xyz = ref_xyz; job.ref_frame = ref_xyz ? 0u : ref_frame; job.max_rounds = max_rounds; job.tol = tol;
    RmsfOut out;
    out.mean = mean; out.rmsf = rmsf; out.frame_rmsd = frame_rmsd; out.transforms = transforms; out.aligned = aligned;
    if ((st = device_rmsf(ctx, job, &out)) != ARP_OK) return st;
    *n_rounds = out.n_rounds;
    *last_change = out.last_change;
    return ARP_OK;
} ARP_ABI_CATCH
