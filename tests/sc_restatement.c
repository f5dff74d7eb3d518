/* Shape complementarity (Lawrence & Colman 1993) restated in plain sequential C, for the parity tests of arp_sc.
 *
 * It follows the reference's loops literally (src/sc/surface_generator.rs, src/sc/sc_calculator.rs): burial by a scan of every atom,
 * the low probes by a scan of every probe, the nearest dot by a scan of the whole other surface.  It shares no code with the product
 * and takes raw arrays (coordinates, radius, molecule, serial).  Everything is f64, compiled with -ffp-contract=off, and every
 * expression keeps the reference's operation order, so that the product's dots can be compared index for index.
 *
 * Tie breaks the reference leaves open: same-molecule neighbours of equal d^2 are ordered by atom index; of two
 * nearest dots at equal d^2 the lower index wins.  Sums (areas, means) run in index order.
 *
 * Build: cc -O2 -ffp-contract=off -shared -fPIC sc_restatement.c -o libscr.so -lm (tests/test_sc_host.py does this into tmp_path). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { double x, y, z; } V;
static V v3(double x, double y, double z) { V r = {x, y, z}; return r; }
static V add(V a, V b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
static V sub(V a, V b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
static V mul(V a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
static V dvd(V a, double s) { return v3(a.x / s, a.y / s, a.z / s); }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static double mag(V a) { double m = dot(a, a); return sqrt(m > 0.0 ? m : 0.0); }
static V normalized(V a) { double m = mag(a); return m > 0.0 ? v3(a.x / m, a.y / m, a.z / m) : a; }
static double dist2(V a, V b) { V d = sub(a, b); return dot(d, d); }
static double dist(V a, V b) { return sqrt(dist2(a, b)); }

enum { FAR = 0, BURIED = 1 };
enum { E_OK = 0, E_NO_ATOMS = 1, E_NO_GROUP1 = 2, E_NO_DOTS = 3, E_COINCIDENT = 4, E_TOO_MANY = 5 };

typedef struct { double p[3], n[3], area, nn_dist, score; int32_t flags, atom; } Dot;  /* flags: kind | 4 buried | 8 trimmed */
typedef struct { int a[3]; double height; V point, alt; } Probe;
typedef struct { Dot *d; size_t n, cap; } Dots;
typedef struct { Probe *d; size_t n, cap; } Probes;
typedef struct { V *d; size_t n, cap; } Pts;

#define PUSH(arr, val) do { if ((arr).n == (arr).cap) { (arr).cap = (arr).cap ? 2 * (arr).cap : 64; (arr).d = realloc((arr).d, (arr).cap * sizeof(*(arr).d)); } (arr).d[(arr).n++] = (val); } while (0)

typedef struct {
    double rp, density, band, sep, w;
    int n;
    const double *x, *y, *z, *r;
    const int32_t *mol;
    const int64_t *serial;
    V *c;
    int *att, *acc;
    int **nb; int *nnb;  /* same-molecule neighbours, sorted by (d^2, index) */
    Probes probes;
    Dots dots[2];
    int64_t n_convex, n_toroidal, n_concave;
    int err, err_i, err_j;
    int64_t branch[5];  /* times each quirk branch ran: see scr_branches */
    int64_t reach[6];   /* how far the run went into the paths the edge tests are about: see scr_reach */
} Run;

static int in_map(Run *R, int a, int b) { return dist2(R->c[a], R->c[b]) <= R->sep * R->sep; }

/* surface_generator.rs:976-1010 */
static int segment(V cen, double rad, V x, V y, double angle, double density, Pts *pts, double *ps) {
    pts->n = 0;
    if (rad <= 0.0) { *ps = 0.0; return 0; }
    double delta = 1.0 / (sqrt(density) * rad);
    double a = -delta / 2.0;
    for (int it = 0; it < 100000; it++) {
        a += delta;
        if (a > angle) break;
        double c = rad * cos(a), s = rad * sin(a);
        PUSH(*pts, add(add(cen, mul(x, c)), mul(y, s)));
    }
    if (a + delta < angle) return -1;
    *ps = pts->n == 0 ? 0.0 : rad * angle / (double)pts->n;
    return 0;
}
static int sample_arc(V cen, double rad, V axis, double density, V x, V v, Pts *pts, double *ps) {
    V y = cross(axis, x);
    double dt1 = dot(v, x), dt2 = dot(v, y);
    double angle = atan2(dt2, dt1);
    if (angle < 0.0) angle += 2.0 * M_PI;
    return segment(cen, rad, x, y, angle, density, pts, ps);
}
static int sample_circle(V cen, double rad, V axis, double density, Pts *pts, double *ps) {
    V v1 = normalized(v3(axis.y * axis.y + axis.z * axis.z, axis.x * axis.x + axis.z * axis.z, axis.x * axis.x + axis.y * axis.y));
    if (fabs(dot(v1, axis)) > 0.99) v1 = v3(1.0, 0.0, 0.0);
    V v2 = normalized(cross(axis, v1));
    V x = normalized(cross(axis, v2));
    V y = cross(axis, x);
    return segment(cen, rad, x, y, 2.0 * M_PI, density, pts, ps);
}
static double point_to_line(V cen, V axis, V p) {
    V v = sub(p, cen);
    double dt = dot(v, axis);
    double d2 = dot(v, v) - dt * dt;
    if (d2 < 0.0) d2 = 0.0;
    return sqrt(d2);
}
/* burial of a probe position: any atom of another molecule with d^2 <= (r + rp)^2 (add_dot, :897-905; :332-344; :842-854) */
static int buried_by_other(Run *R, int molecule, V pcen) {
    for (int b = 0; b < R->n; b++) {
        if (R->mol[b] == molecule) continue;
        double erl = R->r[b] + R->rp;
        if (dist2(pcen, R->c[b]) <= erl * erl) return 1;
    }
    return 0;
}
static void push_dot(Run *R, int molecule, int kind, V p, V nml, double area, int buried, int atom) {
    Dot d;
    memset(&d, 0, sizeof d);
    d.p[0] = p.x; d.p[1] = p.y; d.p[2] = p.z; d.n[0] = nml.x; d.n[1] = nml.y; d.n[2] = nml.z;
    d.area = area; d.flags = kind | (buried ? 4 : 0); d.atom = atom;
    PUSH(R->dots[molecule], d);
}
static void add_dot(Run *R, int molecule, V coor, double area, V pcen, int atom) {  /* :882-915, kind Reentrant */
    V nml = R->rp <= 0.0 ? sub(coor, R->c[atom]) : dvd(sub(pcen, coor), R->rp);
    push_dot(R, molecule, 1, coor, nml, area, buried_by_other(R, molecule, pcen), atom);
}

/* sc_calculator.rs:40-111 + surface_generator.rs:145-215 */
static int categorize(Run *R) {
    int n = R->n;
    double s2 = R->sep * R->sep;
    double *d2tmp = malloc(sizeof(double) * (n ? n : 1));
    int *idx = malloc(sizeof(int) * (n ? n : 1));
    for (int i = 0; i < n; i++) {
        double best = INFINITY;
        int m = 0;
        for (int j = 0; j < n; j++) {
            double d2 = dist2(R->c[i], R->c[j]);
            if (!(d2 <= s2)) {
                double br = R->r[i] + R->r[j] + 2.0 * R->rp;
                if (R->mol[j] == R->mol[i] && R->serial[j] != R->serial[i] && d2 < br * br) R->reach[4]++;
                continue;
            }
            if (R->mol[j] != R->mol[i] && d2 < best) best = d2;
            if (R->serial[j] == R->serial[i]) continue;
            if (R->mol[j] == R->mol[i]) {
                if (d2 <= 0.0001 && !R->err) { R->err = E_COINCIDENT; R->err_i = i; R->err_j = j; }
                double bridge = R->r[i] + R->r[j] + 2.0 * R->rp;
                if (d2 < bridge * bridge) {
                    int k = m++;  /* insertion by (d^2, index) */
                    while (k > 0 && (d2tmp[k - 1] > d2 || (d2tmp[k - 1] == d2 && idx[k - 1] > j))) { d2tmp[k] = d2tmp[k - 1]; idx[k] = idx[k - 1]; k--; }
                    d2tmp[k] = d2; idx[k] = j;
                }
            }
        }
        for (int q = 1; q < m; q++) if (d2tmp[q] == d2tmp[q - 1]) R->reach[2]++;
        R->att[i] = best < s2 ? BURIED : FAR;
        R->nnb[i] = m;
        R->nb[i] = malloc(sizeof(int) * (m ? m : 1));
        memcpy(R->nb[i], idx, sizeof(int) * m);
        if (m == 0) R->acc[i] = 1;
    }
    free(d2tmp); free(idx);
    return R->err;
}

static int collision2(Run *R, V pc, int a1, int a2, int i) {  /* :690-711 */
    for (int q = 0; q < R->nnb[i]; q++) {
        int ni = R->nb[i][q];
        if (R->serial[ni] == R->serial[a1] || R->serial[ni] == R->serial[a2]) continue;
        double e = R->r[ni] + R->rp;
        if (dist2(pc, R->c[ni]) <= e * e) return 1;
    }
    return 0;
}

static void triplets(Run *R, int i, int j, V ua, V mid, double ring_r) {  /* :442-545 */
    V ci = R->c[i];
    double ei = R->r[i] + R->rp, ej = R->r[j] + R->rp;
    int made = 0;
    for (int q = 0; q < R->nnb[i]; q++) {
        int k = R->nb[i][q];
        if (R->serial[k] <= R->serial[j]) continue;
        double ek = R->r[k] + R->rp;
        if (!in_map(R, j, k)) {
            if (sqrt(dist2(R->c[j], R->c[k])) < ej + ek) R->reach[3]++;
            continue;
        }
        if (sqrt(dist2(R->c[j], R->c[k])) >= ej + ek) continue;
        double dik = sqrt(dist2(ci, R->c[k]));
        if (dik >= ei + ek) continue;
        if (R->att[i] == FAR && R->att[j] == FAR && R->att[k] == FAR) continue;
        V uik = dvd(sub(R->c[k], ci), dik);
        double wedge = acos(dot(ua, uik));
        double sw = sin(wedge);
        if (sw <= 0.0) {
            double dtijk2 = dist(mid, R->c[k]);
            double rkp2 = ek * ek - ring_r * ring_r;
            if (dtijk2 < rkp2) { R->branch[0]++; return; }  /* (made_probe is not applied) */
            R->branch[1]++;
            continue;
        }
        V an = dvd(cross(ua, uik), sw);
        V perp = cross(an, ua);
        double asym_ik = (ei * ei - ek * ek) / dik;
        V mid_ik = add(mul(add(ci, R->c[k]), 0.5), mul(uik, asym_ik * 0.5));
        V cw = sub(mid_ik, mid);
        cw = v3(uik.x * cw.x, uik.y * cw.y, uik.z * cw.z);
        double csum = cw.x + cw.y + cw.z;
        V tc = add(mid, mul(perp, csum / sw));
        double h = ei * ei - dist2(tc, ci);
        if (h <= 0.0) continue;
        h = sqrt(h);
        for (int is0 = 1; is0 <= 2; is0++) {
            int sign = 3 - 2 * is0;
            V pc = add(tc, mul(an, h * (double)sign));
            if (collision2(R, pc, j, k, i)) continue;
            Probe p;
            p.height = h; p.point = pc; p.alt = mul(an, (double)sign);
            if (sign > 0) { p.a[0] = i; p.a[1] = j; } else { p.a[0] = j; p.a[1] = i; }
            p.a[2] = k;
            PUSH(R->probes, p);
            made = 1;
        }
    }
    if (made) R->acc[i] = 1;
}

static int reentrant(Run *R, int i, int j, V ua, V mid, double ring_r, int point_cusp, Pts *subs, Pts *pts) {  /* :547-688 */
    double rp = R->rp;
    double density = (R->density + R->density) / 2.0;  /* f64::midpoint of two finite values */
    double ei = R->r[i] + rp, ej = R->r[j] + rp;
    double rri = ring_r * R->r[i] / ei, rrj = ring_r * R->r[j] / ej;
    double belt = ring_r - rp;
    if (belt <= 0.0) belt = 0.0;
    double mean_r = (rri + 2.0 * belt + rrj) / 4.0;
    double ecc = mean_r / ring_r;
    double eff = ecc * ecc * density;
    double ts, ps;
    if (sample_circle(mid, ring_r, ua, eff, subs, &ts)) return E_TOO_MANY;
    for (size_t s = 0; s < subs->n; s++) {
        V rpnt = subs->d[s];
        int tooclose = 0;
        for (int q = 0; q < R->nnb[i]; q++) {
            int ni = R->nb[i][q];
            if (R->serial[ni] == R->serial[j]) continue;
            double e = R->r[ni] + rp;
            if (dist2(rpnt, R->c[ni]) < e * e) { tooclose = 1; break; }
        }
        if (tooclose) continue;
        R->acc[i] = 1; R->acc[j] = 1;
        V vpi = dvd(sub(R->c[i], rpnt), ei), vpj = dvd(sub(R->c[j], rpnt), ej);
        V tax = normalized(cross(vpi, vpj));
        double cusp = rp * rp - ring_r * ring_r;
        V arc_i, arc_j;
        if (cusp > 0.0 && point_cusp) {
            cusp = sqrt(cusp);
            V qij = sub(mid, mul(ua, cusp));
            arc_i = dvd(sub(qij, rpnt), rp);
            arc_j = v3(0.0, 0.0, 0.0);
        } else {
            arc_i = arc_j = normalized(add(vpi, vpj));
        }
        double dt = dot(arc_i, vpi);
        if (dt >= 1.0 || dt <= -1.0) { R->branch[2]++; return 0; }
        dt = dot(arc_j, vpj);
        if (dt >= 1.0 || dt <= -1.0) { R->branch[2]++; return 0; }
        if (R->att[i] != FAR) {
            if (sample_arc(rpnt, rp, tax, density, vpi, arc_i, pts, &ps)) return E_TOO_MANY;
            for (size_t t = 0; t < pts->n; t++) {
                double area = ps * ts * point_to_line(mid, ua, pts->d[t]) / ring_r;
                R->n_toroidal++;
                add_dot(R, R->mol[i], pts->d[t], area, rpnt, i);
            }
        }
        if (R->att[j] != FAR) continue;
        if (sample_arc(rpnt, rp, tax, density, arc_j, vpj, pts, &ps)) return E_TOO_MANY;
        if (pts->n) R->branch[4]++;
        R->n_toroidal += (int64_t)pts->n;
        for (size_t t = 0; t < pts->n; t++) {
            double area = ps * ts * point_to_line(mid, ua, pts->d[t]) / ring_r;
            add_dot(R, R->mol[j], pts->d[t], area, rpnt, j);
        }
    }
    return 0;
}

static int build_probes(Run *R, int i, Pts *subs, Pts *pts) {  /* :375-440 */
    V ci = R->c[i];
    double rp = R->rp, ei = R->r[i] + rp;
    int num = R->nnb[i];
    for (int q = 0; q < num; q++) {
        int j = R->nb[i][q];
        if (R->serial[j] <= R->serial[i]) continue;
        double ej = R->r[j] + rp;
        double d2 = dist2(ci, R->c[j]);
        double dij = sqrt(d2);
        V ua = dvd(sub(R->c[j], ci), dij);
        double asym = (ei * ei - ej * ej) / dij;
        V mid = add(mul(add(ci, R->c[j]), 0.5), mul(ua, asym * 0.5));
        double far = (ei + ej) * (ei + ej) - d2;
        if (far <= 0.0) continue;
        far = sqrt(far);
        double dr = R->r[i] - R->r[j];
        double contain = d2 - dr * dr;
        if (contain <= 0.0) continue;
        contain = sqrt(contain);
        double ring_r = 0.5 * far * contain / dij;
        if (num <= 1) { R->acc[i] = 1; R->acc[j] = 1; R->branch[3]++; break; }
        triplets(R, i, j, ua, mid, ring_r);
        int point_cusp = fabs(asym) < dij;
        if (R->att[i] != FAR || (R->att[j] != FAR && rp > 0.0)) {
            int e = reentrant(R, i, j, ua, mid, ring_r, point_cusp, subs, pts);
            if (e) return e;
        }
    }
    return 0;
}

static void contact_atom(Run *R, int i, Pts *lats, Pts *pts, Dots *tmp) {  /* :217-373 */
    double rp = R->rp;
    tmp->n = 0;
    if (R->att[i] == FAR || !R->acc[i]) return;
    V ci = R->c[i];
    V north = v3(0.0, 0.0, 1.0), south = v3(0.0, 0.0, -1.0), eq = v3(1.0, 0.0, 0.0);
    double ri = R->r[i], ei = ri + rp;
    if (R->nnb[i] > 0) {
        int m = R->nb[i][0];
        V cn = R->c[m];
        north = normalized(sub(ci, cn));
        V t = normalized(v3(north.y * north.y + north.z * north.z, north.x * north.x + north.z * north.z, north.x * north.x + north.y * north.y));
        if (fabs(dot(t, north)) > 0.99) t = v3(1.0, 0.0, 0.0);
        eq = normalized(cross(north, t));
        double rn = R->r[m], en = rn + rp;
        double dij = dist(ci, cn);
        V ua = dvd(sub(cn, ci), dij);
        double asym = (ei * ei - en * en) / dij;
        V mid = add(mul(add(ci, cn), 0.5), mul(ua, asym * 0.5));
        double far = (ei + en) * (ei + en) - dij * dij;
        if (far <= 0.0) return;
        far = sqrt(far);
        double dr = ri - rn;
        double contain = dij * dij - dr * dr;
        if (contain <= 0.0) return;
        contain = sqrt(contain);
        double ring_r = 0.5 * far * contain / dij;
        V rpnt = add(mid, mul(cross(eq, north), ring_r));
        south = dvd(sub(rpnt, ci), ei);
        if (dot(cross(north, south), eq) <= 0.0) return;
    }
    double cs, ps;
    if (sample_arc(v3(0.0, 0.0, 0.0), ri, eq, R->density, north, south, lats, &cs)) return;
    int64_t nlat = (int64_t)lats->n;
    int other = R->mol[i] == 0 ? 1 : 0;
    for (size_t l = 0; l < lats->n; l++) {
        double dt = dot(lats->d[l], north);
        V cen = add(ci, mul(north, dt));
        double rad = ri * ri - dt * dt;
        if (rad <= 0.0) continue;
        rad = sqrt(rad);
        if (sample_circle(cen, rad, north, R->density, pts, &ps)) { tmp->n = 0; return; }
        if (pts->n == 0) continue;
        double area = ps * cs;
        for (size_t t = 0; t < pts->n; t++) {
            V p = pts->d[t];
            V pcen = add(ci, mul(sub(p, ci), ei / ri));
            int coll = 0;
            for (int q = 1; q < R->nnb[i]; q++) {
                int a = R->nb[i][q];
                if (dist(pcen, R->c[a]) <= R->r[a] + rp) { coll = 1; break; }
            }
            if (coll) continue;
            int buried = 0;
            for (int b = 0; b < R->n; b++) {
                if (R->mol[b] != other) continue;
                double erl = R->r[b] + rp;
                if (dist2(pcen, R->c[b]) <= erl * erl) { buried = 1; break; }
            }
            V nml = rp <= 0.0 ? sub(p, ci) : dvd(sub(pcen, p), rp);
            Dot d;
            memset(&d, 0, sizeof d);
            d.p[0] = p.x; d.p[1] = p.y; d.p[2] = p.z; d.n[0] = nml.x; d.n[1] = nml.y; d.n[2] = nml.z;
            d.area = area; d.flags = 0 | (buried ? 4 : 0); d.atom = i;
            PUSH(*tmp, d);
        }
    }
    if (tmp->n && nlat > R->reach[0]) R->reach[0] = nlat;
}

static void concave_probe(Run *R, size_t pi, const int *low, size_t nlow, Pts *lats, Pts *pts, Dots *tmp0, Dots *tmp1) {  /* :713-880 */
    double rp = R->rp, rp2 = rp * rp;
    tmp0->n = tmp1->n = 0;
    Probe *pr = &R->probes.d[pi];
    V pijk = pr->point, uijk = pr->alt;
    double hijk = pr->height;
    double density = (R->density + R->density + R->density) / 3.0;
    size_t nnear = 0;
    int *nears = malloc(sizeof(int) * (nlow ? nlow : 1));
    for (size_t q = 0; q < nlow; q++) {
        if ((size_t)low[q] == pi) continue;
        if (dist2(pijk, R->probes.d[low[q]].point) <= 4.0 * rp2) nears[nnear++] = low[q];
    }
    V vp[3], vec[3];
    for (int k = 0; k < 3; k++) vp[k] = normalized(sub(R->c[pr->a[k]], pijk));
    vec[0] = normalized(cross(vp[0], vp[1]));
    vec[1] = normalized(cross(vp[1], vp[2]));
    vec[2] = normalized(cross(vp[2], vp[0]));
    double dm = -1.0;
    int mm = 0;
    for (int k = 0; k < 3; k++) { double dt = dot(uijk, vp[k]); if (dt > dm) { dm = dt; mm = k; } }
    V south = mul(uijk, -1.0);
    V axis = normalized(cross(vp[mm], south));
    double cs, ps;
    if (sample_arc(v3(0.0, 0.0, 0.0), rp, axis, density, vp[mm], south, lats, &cs)) { free(nears); return; }
    int64_t nlat = (int64_t)lats->n;
    for (size_t l = 0; l < lats->n; l++) {
        double dt = dot(lats->d[l], south);
        V cen = mul(south, dt);
        double rad = rp2 - dt * dt;
        if (rad <= 0.0) continue;
        rad = sqrt(rad);
        if (sample_circle(cen, rad, south, density, pts, &ps)) { tmp0->n = tmp1->n = 0; free(nears); return; }
        if (pts->n == 0) continue;
        double area = ps * cs;
        for (size_t t = 0; t < pts->n; t++) {
            V p = pts->d[t];
            if (dot(p, vec[0]) >= 0.0 || dot(p, vec[1]) >= 0.0 || dot(p, vec[2]) >= 0.0) continue;
            p = add(p, pijk);
            if (hijk < rp && nnear) {
                int coll = 0;
                for (size_t q = 0; q < nnear; q++) if (dist2(p, R->probes.d[nears[q]].point) < rp2) { coll = 1; break; }
                if (coll) continue;
            }
            int mc = 0;
            double dmin = 2.0 * rp;
            for (int kk = 0; kk < 3; kk++) {
                double d = dist(p, R->c[pr->a[kk]]) - R->r[pr->a[kk]];
                if (d < dmin) { dmin = d; mc = kk; }
            }
            int atom = pr->a[mc], molecule = R->mol[atom];
            V nml = rp <= 0.0 ? sub(p, R->c[atom]) : dvd(sub(pijk, p), rp);
            int buried = buried_by_other(R, molecule, pijk);
            Dot d;
            memset(&d, 0, sizeof d);
            d.p[0] = p.x; d.p[1] = p.y; d.p[2] = p.z; d.n[0] = nml.x; d.n[1] = nml.y; d.n[2] = nml.z;
            d.area = area; d.flags = 2 | (buried ? 4 : 0); d.atom = atom;
            if (molecule == 0) PUSH(*tmp0, d); else PUSH(*tmp1, d);
            if (l >= 64) R->reach[5]++;
        }
    }
    if (tmp0->n + tmp1->n && nlat > R->reach[1]) R->reach[1] = nlat;
    free(nears);
}

static void append(Dots *to, Dots *from) { for (size_t k = 0; k < from->n; k++) PUSH(*to, from->d[k]); }

typedef struct {
    int64_t n_atoms[2], n_buried_atoms[2], n_far_atoms[2], n_all_dots[2], n_trimmed_dots[2];
    double trimmed_area[2], d_mean[2], d_median[2], s_mean[2], s_median[2];
    int64_t n_convex, n_toroidal, n_concave, n_probes;
    double sc, distance, area;
    int32_t err, err_i, err_j;
} ScrResults;

static int cmp_d(const void *a, const void *b) { double x = *(const double *)a, y = *(const double *)b; return x < y ? -1 : x > y ? 1 : 0; }

/* sc_calculator.rs:143-347 */
static void trim_and_score(Run *R, ScrResults *o) {
    double b2 = R->band * R->band;
    for (int s = 0; s < 2; s++) {
        Dots *D = &R->dots[s];
        double area = 0.0;
        int64_t nt = 0;
        for (size_t a = 0; a < D->n; a++) {
            if (!(D->d[a].flags & 4)) continue;
            int hit = 0;
            V pa = v3(D->d[a].p[0], D->d[a].p[1], D->d[a].p[2]);
            for (size_t b = 0; b < D->n && !hit; b++) {
                if (D->d[b].flags & 4) continue;
                if (dist2(v3(D->d[b].p[0], D->d[b].p[1], D->d[b].p[2]), pa) <= b2) hit = 1;
            }
            if (hit) continue;
            D->d[a].flags |= 8;
            area += D->d[a].area;
            nt++;
        }
        o->trimmed_area[s] = area; o->n_trimmed_dots[s] = nt; o->n_all_dots[s] = (int64_t)D->n;
    }
    for (int my = 0; my < 2; my++) {
        Dots *M = &R->dots[my], *T = &R->dots[1 - my];
        if (o->n_trimmed_dots[my] == 0 || o->n_trimmed_dots[1 - my] == 0) continue;
        double *dv = malloc(sizeof(double) * o->n_trimmed_dots[my]), *sv = malloc(sizeof(double) * o->n_trimmed_dots[my]);
        double dsum = 0.0, ssum = 0.0;
        int64_t m = 0;
        for (size_t a = 0; a < M->n; a++) {
            if (!(M->d[a].flags & 8)) continue;
            double best = INFINITY;
            size_t bi = 0;
            for (size_t b = 0; b < T->n; b++) {
                if (!(T->d[b].flags & 8)) continue;
                double dx = T->d[b].p[0] - M->d[a].p[0], dy = T->d[b].p[1] - M->d[a].p[1], dz = T->d[b].p[2] - M->d[a].p[2];
                double d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < best) { best = d2; bi = b; }  /* strict: the lower index keeps a tie */
            }
            double d = sqrt(best);
            double r = M->d[a].n[0] * T->d[bi].n[0] + M->d[a].n[1] * T->d[bi].n[1] + M->d[a].n[2] * T->d[bi].n[2];
            r *= exp(-best * R->w);
            if (r < -0.999) r = -0.999;
            if (r > 0.999) r = 0.999;
            M->d[a].nn_dist = d; M->d[a].score = -r;
            dv[m] = d; sv[m] = -r; m++;
            dsum += d; ssum += r;
        }
        o->d_mean[my] = dsum / (double)m;
        o->s_mean[my] = -(ssum / (double)m);
        qsort(dv, m, sizeof(double), cmp_d); qsort(sv, m, sizeof(double), cmp_d);
        o->d_median[my] = dv[m / 2]; o->s_median[my] = sv[m / 2];
        free(dv); free(sv);
    }
    o->sc = (o->s_median[0] + o->s_median[1]) / 2.0;
    o->distance = (o->d_median[0] + o->d_median[1]) / 2.0;
    o->area = o->trimmed_area[0] + o->trimmed_area[1];
}

/* Runs the whole calculation.  Returns a handle (never NULL); scr_results / scr_dots read it, scr_free releases it. */
void *scr_run(int n, const double *x, const double *y, const double *z, const double *r, const int32_t *mol, const int64_t *serial,
              double rp, double density, double band, double sep, double w, ScrResults *o) {
    Run *R = calloc(1, sizeof(Run));
    memset(o, 0, sizeof *o);
    R->rp = rp; R->density = density; R->band = band; R->sep = sep; R->w = w;
    R->n = n; R->x = x; R->y = y; R->z = z; R->r = r; R->mol = mol; R->serial = serial;
    R->c = malloc(sizeof(V) * (n ? n : 1));
    R->att = calloc(n ? n : 1, sizeof(int)); R->acc = calloc(n ? n : 1, sizeof(int));
    R->nb = calloc(n ? n : 1, sizeof(int *)); R->nnb = calloc(n ? n : 1, sizeof(int));
    for (int i = 0; i < n; i++) {
        R->c[i] = v3(x[i], y[i], z[i]);
        o->n_atoms[mol[i]]++;
    }
    Pts a = {0}, b = {0};
    Dots t0 = {0}, t1 = {0};
    if (n == 0) { o->err = E_NO_ATOMS; goto done; }
    if (o->n_atoms[0] == 0) { o->err = E_NO_GROUP1; goto done; }
    if (categorize(R)) { o->err = R->err; o->err_i = R->err_i; o->err_j = R->err_j; goto done; }
    for (int i = 0; i < n; i++) {
        if (R->att[i] == BURIED) o->n_buried_atoms[mol[i]]++; else o->n_far_atoms[mol[i]]++;
    }
    for (int i = 0; i < n; i++) {
        if (R->att[i] == FAR) continue;
        int e = build_probes(R, i, &a, &b);
        if (e) { o->err = e; goto done; }
    }
    for (int i = 0; i < n; i++) {
        contact_atom(R, i, &a, &b, &t0);
        R->n_convex += (int64_t)t0.n;
        if (t0.n) append(&R->dots[mol[i]], &t0);
    }
    if (rp > 0.0) {
        int *low = malloc(sizeof(int) * (R->probes.n ? R->probes.n : 1));
        size_t nlow = 0;
        for (size_t p = 0; p < R->probes.n; p++) if (R->probes.d[p].height < rp) low[nlow++] = (int)p;
        for (size_t p = 0; p < R->probes.n; p++) {
            concave_probe(R, p, low, nlow, &a, &b, &t0, &t1);
            R->n_concave += (int64_t)(t0.n + t1.n);
            append(&R->dots[0], &t0); append(&R->dots[1], &t1);
        }
        free(low);
    }
    o->n_convex = R->n_convex; o->n_toroidal = R->n_toroidal; o->n_concave = R->n_concave; o->n_probes = (int64_t)R->probes.n;
    o->n_all_dots[0] = (int64_t)R->dots[0].n; o->n_all_dots[1] = (int64_t)R->dots[1].n;
    if (R->dots[0].n == 0 || R->dots[1].n == 0) { o->err = E_NO_DOTS; goto done; }
    trim_and_score(R, o);
done:
    free(a.d); free(b.d); free(t0.d); free(t1.d);
    return R;
}

int64_t scr_n_dots(void *h, int s) { return (int64_t)((Run *)h)->dots[s].n; }
/* dot k of surface s: xyz, normal, area, flags, nn_dist, score (0 where not trimmed) */
void scr_dots(void *h, int s, double *xyz, double *nml, double *area, int32_t *flags, double *nn, double *score) {
    Dots *D = &((Run *)h)->dots[s];
    for (size_t k = 0; k < D->n; k++) {
        for (int c = 0; c < 3; c++) { xyz[3 * k + c] = D->d[k].p[c]; nml[3 * k + c] = D->d[k].n[c]; }
        area[k] = D->d[k].area; flags[k] = D->d[k].flags; nn[k] = D->d[k].nn_dist; score[k] = D->d[k].score;
    }
}
int64_t scr_n_probes(void *h) { return (int64_t)((Run *)h)->probes.n; }
void scr_probes(void *h, int32_t *atoms, double *height, double *point) {
    Probes *P = &((Run *)h)->probes;
    for (size_t k = 0; k < P->n; k++) {
        for (int c = 0; c < 3; c++) atoms[3 * k + c] = P->d[k].a[c];
        height[k] = P->d[k].height;
        point[3 * k] = P->d[k].point.x; point[3 * k + 1] = P->d[k].point.y; point[3 * k + 2] = P->d[k].point.z;
    }
}
/* branch counts: [0] the sin_wedge <= 0 `return`, [1] its `continue`, [2] the ring-point |dot| >= 1 `return`, [3] the num_neighbors <= 1
 * `break`, [4] ring points whose Far atom j emitted an arc */
void scr_branches(void *h, int64_t *out) { memcpy(out, ((Run *)h)->branch, sizeof ((Run *)h)->branch); }
/* reach counters: [0] the largest latitude count of a contact atom that emitted a dot, [1] the same of a concave probe, [2] neighbour-list
 * entries whose d^2 equals that of the entry before them, [3] triplet candidates k outside j's map (d_jk^2 > sep^2) although
 * d_jk < e_j + e_k, [4] ordered same-molecule pairs with d^2 < bridge^2 that d^2 <= sep^2 rejected, [5] concave dots of latitudes 64 and up
 * (kept only if their probe is: a probe whose circle fails is dropped whole, which no case here reaches) */
void scr_reach(void *h, int64_t *out) { memcpy(out, ((Run *)h)->reach, sizeof ((Run *)h)->reach); }
void scr_free(void *h) {
    Run *R = h;
    for (int i = 0; i < R->n; i++) free(R->nb[i]);
    free(R->nb); free(R->nnb); free(R->c); free(R->att); free(R->acc);
    free(R->probes.d); free(R->dots[0].d); free(R->dots[1].d);
    free(R);
}
