// Covariance, DCCM and projection of an ensemble's motions: the checks and the host half of arp_covariance and arp_project (device
// pipeline: cov.inl behind rmsf.inl), and the definitions in plain sequential C++, arp_covariance_host and arp_project_host, their yardsticks.
#include <algorithm>
#include <cmath>

#include "debug_knobs.h"
#include "table.h"

using namespace arp;

namespace {
// the first non-finite value of v[count], or count
uint64_t first_non_finite(const double *v, uint64_t count) {
    for (uint64_t i = 0; i < count; i++)
        if (!std::isfinite(v[i])) return i;
    return count;
}

// what both projection calls check of their own arguments (m > 0 is the caller's)
arp_status project_check(uint64_t F, uint64_t m, const double *transforms, const double *mean, const double *modes, uint64_t k) {
    if (k == 0) { set_error("project: at least one mode is needed (k == 0)"); return ARP_ERR_BAD_INPUT; }
    if (k > 3 * m) { set_error("project: k = %llu modes are more than the %llu coordinates of %llu measured atoms", (unsigned long long)k, (unsigned long long)(3 * m), (unsigned long long)m); return ARP_ERR_BAD_INPUT; }
    if (!mean || !modes) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    uint64_t bad;
    if ((bad = first_non_finite(mean, m * 3)) < m * 3) { set_error("project: non-finite coordinate in mean, atom %llu", (unsigned long long)(bad / 3)); return ARP_ERR_BAD_INPUT; }
    if ((bad = first_non_finite(modes, k * 3 * m)) < k * 3 * m) { set_error("project: non-finite entry in mode %llu", (unsigned long long)(bad / (3 * m))); return ARP_ERR_BAD_INPUT; }
    if (transforms && (bad = first_non_finite(transforms, F * 12)) < F * 12) { set_error("project: non-finite entry in the transform of frame %llu", (unsigned long long)(bad / 12)); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
}  // namespace

// The definition (include/arpeggia_amd.h) in plain sequential C++ on already-superposed coordinates: f64 throughout, every sum in the order of its index.
extern "C" arp_status arp_covariance_host(uint64_t n_frames, uint64_t m, const double *aligned, const double *mean, double *cov, float *dccm) try {
    const uint64_t F = n_frames, L = 3 * m;
    if (F == 0) { set_error("covariance: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    if (m == 0) { set_error("covariance: the measured selection is empty (m == 0)"); return ARP_ERR_BAD_INPUT; }
    if (!aligned || !mean) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (!cov && !dccm) { set_error("covariance: neither cov nor dccm is asked for"); return ARP_ERR_BAD_INPUT; }
    uint64_t bad;
    if ((bad = first_non_finite(aligned, F * L)) < F * L) { set_error("covariance: non-finite coordinate in frame %llu, atom %llu", (unsigned long long)(bad / L), (unsigned long long)(bad / 3 % m)); return ARP_ERR_BAD_INPUT; }
    if ((bad = first_non_finite(mean, L)) < L) { set_error("covariance: non-finite coordinate in mean, atom %llu", (unsigned long long)(bad / 3)); return ARP_ERR_BAD_INPUT; }
    std::vector<double> d(F * L);
    for (uint64_t f = 0; f < F; f++)
        for (uint64_t a = 0; a < L; a++) d[f * L + a] = aligned[f * L + a] - mean[a];
    if (cov)
        for (uint64_t a = 0; a < L; a++)
            for (uint64_t b = a; b < L; b++) {
                double s = 0.0;
                for (uint64_t f = 0; f < F; f++) s += d[f * L + a] * d[f * L + b];
                cov[a * L + b] = cov[b * L + a] = s / (double)F;
            }
    if (dccm) {
        auto t_of = [&](uint64_t i, uint64_t j) {
            double s = 0.0;
            for (uint64_t f = 0; f < F; f++)
                for (int k = 0; k < 3; k++) s += d[f * L + 3 * i + k] * d[f * L + 3 * j + k];
            return s / (double)F;
        };
        std::vector<double> v(m);
        for (uint64_t i = 0; i < m; i++) v[i] = t_of(i, i);
        for (uint64_t i = 0; i < m; i++) {
            dccm[i * m + i] = 1.0f;
            for (uint64_t j = i + 1; j < m; j++) {
                float c = 0.0f;
                if (v[i] != 0.0 && v[j] != 0.0) c = (float)std::min(1.0, std::max(-1.0, t_of(i, j) / std::sqrt(v[i] * v[j])));
                dccm[i * m + j] = dccm[j * m + i] = c;
            }
        }
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_project_host(uint64_t n_frames, uint64_t m, const double *xyz_msel, const double *transforms, const double *mean, const double *modes, uint64_t k,
                                       double *proj) try {
    const uint64_t F = n_frames, L = 3 * m;
    if (F == 0) { set_error("project: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    if (m == 0) { set_error("project: the measured selection is empty (m == 0)"); return ARP_ERR_BAD_INPUT; }
    if (!xyz_msel || !proj) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status st = project_check(F, m, transforms, mean, modes, k);
    if (st != ARP_OK) return st;
    uint64_t bad;
    if ((bad = first_non_finite(xyz_msel, F * L)) < F * L) { set_error("project: non-finite coordinate in frame %llu, atom %llu", (unsigned long long)(bad / L), (unsigned long long)(bad / 3 % m)); return ARP_ERR_BAD_INPUT; }
    const double identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    std::vector<double> d(L);
    for (uint64_t f = 0; f < F; f++) {
        const double *t = transforms ? transforms + f * 12 : identity;
        for (uint64_t i = 0; i < m; i++) {
            const double *p = xyz_msel + (f * m + i) * 3;
            for (int c = 0; c < 3; c++) d[3 * i + c] = (((t[3 * c] * p[0] + t[3 * c + 1] * p[1]) + t[3 * c + 2] * p[2]) + t[9 + c]) - mean[3 * i + c];
        }
        for (uint64_t j = 0; j < k; j++) {
            double s = 0.0;
            for (uint64_t a = 0; a < L; a++) s += d[a] * modes[j * L + a];
            proj[f * k + j] = s;
        }
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_covariance(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const uint32_t *msel, uint64_t n_msel,
                                     const double *ref_xyz, uint64_t ref_frame, uint32_t max_rounds, double tol, double *cov, float *dccm, double *mean, float *rmsf, float *frame_rmsd,
                                     double *transforms, uint32_t *n_rounds, double *last_change) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsf_check("covariance", s, n_frames, xyz, sel, n_sel, msel, n_msel, ref_xyz, ref_frame, max_rounds, tol, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if (!ctx) return ARP_OK;  // validation only
    if (!cov && !dccm) { set_error("covariance: neither cov nor dccm is asked for"); return ARP_ERR_BAD_INPUT; }
    if (!mean || !rmsf || !frame_rmsd || !n_rounds || !last_change) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const uint64_t m = msel ? n_msel : n_sel;
    const uint64_t need = rmsf_resident_bytes(F, n_sel, m, msel != nullptr) + cov_extra_bytes(F, m, cov != nullptr, dccm != nullptr);
    if (need > rmsd_cap()) {
        set_error("covariance: the packed coordinates, the deviations, the outputs and the slab partials of %llu frames (F) x %llu measured atoms (m) need %llu bytes, the limit is %llu (rmsd_cap_bytes)",
                  (unsigned long long)F, (unsigned long long)m, (unsigned long long)need, (unsigned long long)rmsd_cap());
        return ARP_ERR_CAPACITY;
    }
    RmsfJob job;
    job.n_atoms = n0; job.n_frames = F; job.n_sel = n_sel; job.n_msel = m; job.xyz = frames; job.sel = sel; job.msel = msel;
    job.chunk_atoms = g_debug.rmsd_chunk_atoms > 0 ? (uint64_t)g_debug.rmsd_chunk_atoms : 0u;
    job.ref_xyz = ref_xyz; job.ref_frame = ref_xyz ? 0u : ref_frame; job.max_rounds = max_rounds; job.tol = tol;
    RmsfOut out;
    out.mean = mean; out.rmsf = rmsf; out.frame_rmsd = frame_rmsd; out.transforms = transforms; out.cov = cov; out.dccm = dccm;
    if ((st = device_rmsf(ctx, job, &out)) != ARP_OK) return st;
    *n_rounds = out.n_rounds;
    *last_change = out.last_change;
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_project(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *msel, uint64_t n_msel, const double *transforms,
                                  const double *mean, const double *modes, uint64_t k, double *proj) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsd_check("project", s, n_frames, xyz, msel, n_msel, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if ((st = project_check(F, n_msel, transforms, mean, modes, k)) != ARP_OK) return st;
    if (!ctx) return ARP_OK;  // validation only
    if (!proj) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const uint64_t need = F * 96u + n_msel * 28u + k * 3u * n_msel * 8u + F * k * 8u;  // the transforms, the selection, the mean, the modes and the projections (the staging buffer of a pass is sized by "rmsd_chunk_atoms" and not counted, as in the rmsd calls)
    if (need > rmsd_cap()) {
        set_error("project: %llu frames (F) x %llu measured atoms (m) x %llu modes (k) need %llu bytes, the limit is %llu (rmsd_cap_bytes)", (unsigned long long)F,
                  (unsigned long long)n_msel, (unsigned long long)k, (unsigned long long)need, (unsigned long long)rmsd_cap());
        return ARP_ERR_CAPACITY;
    }
    ProjectJob job;
    job.n_atoms = n0; job.n_frames = F; job.n_msel = n_msel; job.k = k; job.xyz = frames; job.msel = msel;
    job.chunk_atoms = g_debug.rmsd_chunk_atoms > 0 ? (uint64_t)g_debug.rmsd_chunk_atoms : 0u;
    job.transforms = transforms; job.mean = mean; job.modes = modes;
    return device_project(ctx, job, proj);
} ARP_ABI_CATCH
