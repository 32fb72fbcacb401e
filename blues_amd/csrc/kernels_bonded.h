// kernels_bonded.h -- harmonic bonds/angles, periodic torsions, env-env 1-4 exceptions, the
// positional restraint, harmonic centroid bonds, CMAP torsion correction maps and CHARMM's Urey-Bradley terms and harmonic
// impropers (K3/K4), fp64, gather form.
//
// OpenMM's HarmonicBondForce / HarmonicAngleForce / PeriodicTorsionForce / NonbondedForce
// exceptions / CustomExternalForce('k_restr*periodicdistance(x,y,z,x0,y0,z0)^2',
// reference blues/simulation.py:347) scatter each term's force to its atoms.  Here every
// MOBILE atom that takes part in a term owns a row of (term, role) entries and recomputes the
// terms it belongs to, keeping only its own component: 2-4x redundant flops on a few
// thousand cheap terms, but no atomics and a fixed summation order.
#pragma once
#include "device_common.h"

enum { T_BOND = 0, T_ANGLE = 1, T_TORSION = 2, T_EXC = 3, T_RESTR = 4, T_EWEX = 5, T_NTYPES = 6 };   // T_EWEX: Ewald correction of an excluded pair (BLUES_NB_PME)
// Harmonic centroid bonds (CustomCentroidBondForce '0.5*k*distance(g1,g2)^2' of a NoCutoff System): an ENTRY type only.  Its terms live in
// arrays of their own (BondedArgs::cent_*), its energy is booked with the restraint's, and only the CENT = true instantiations of the
// templates below know it -- the CENT = false ones, which every System without such bonds runs, are the code they were before it existed.
enum { T_CENT = T_NTYPES };   // (the first value past the per-type arrays; blues_engine.hip asserts it stays there)
#define CENT_GROUP 8   // places per group (BLUES_MAX_CENTROID_GROUP); a term is two groups, unused places hold atom -1 and weight 0
// CMAP torsions (OpenMM's CMAPTorsionForce: a tabulated energy over two dihedrals, bicubic patches): the second ENTRY-only type, on any
// System.  Terms in arrays of their own (BondedArgs::cmap_*), energy booked with the torsions', known to the CMAP = true instantiations only.
enum { T_CMAP = T_NTYPES + 1 };
#define CMAP_TWO_PI 6.283185307179586476925286766559
// CHARMM's Urey-Bradley 1-3 terms (T_BOND's form between the outer atoms of an angle; energy booked with the bonds') and harmonic
// impropers (E = k (psi - psi0)^2 over T_TORSION's dihedral; energy booked with the torsions'): two more ENTRY-only types, terms in
// arrays of their own (BondedArgs::ub_* / impr_*).  They have no template flag of their own: they ride with CMAP = true, which now reads
// "knows every entry-only type that can sit on any System".  A chamber topology carries maps and these terms together, a fourth flag
// would double the instantiations (lone, batched, entries, energy) for a branch the CMAP = true kernels skip in two compares, and the
// CMAP = false instantiations -- what every System without maps and without these terms launches -- stay the code they were.
enum { T_UREY = T_NTYPES + 2, T_IMPR = T_NTYPES + 3 };
#define IMPR_PI 3.141592653589793238462643383279

struct BondedArgs {
    int n_rows;
    const int* row_atom;    // caller index of the row's atom
    const int* row_start;   // [n_rows+1]
    const int* ent_type;    // per entry
    const int* ent_term;
    const int* ent_role;
    // all terms (caller indices)
    int n_terms[T_NTYPES];
    const int* atoms[T_NTYPES];      // 2,3,4,2,1,2 indices per term
    const double* params[T_NTYPES];  // 2,2,3,3,3,1 doubles per term (restraint: x0,y0,z0; Ewald correction: q_i q_j)
    double restr_k;
    double ewald_alpha;
    const double* x[3];
    Box3 box;
    int periodic;
    double* fent;    // [3][n_entries] per-entry forces
    int n_entries;
    int n;
    double* epart;   // [nblocks][T_NTYPES] (energy kernel)
    // Gaussian noise for the next O substeps, generated here (extra blocks of the same launch) so that the
    // log/sqrt/sincos of the Box-Muller transform are off the integrator's serial per-cluster path
    int n_mobile, n_noise; const int* mobile_atoms; double* noise;  // noise[(d*3+k)*n_mobile + m]
    unsigned long long seed; unsigned stream, draw_base;
    int n_entry_blocks;
    // centroid bonds: 2 * CENT_GROUP atoms and 2 * CENT_GROUP weights + k per term
    int n_cent; const int* cent_atoms; const double* cent_params;
    // CMAP torsions: 8 atoms per term; cmap_grid[2 t] = n of the term's map, [2 t + 1] = its first patch in cmap_coef, which holds 16
    // doubles per patch (i + n * j): c[a][b] of E = sum c[a][b] t^a u^b, t = phi / delta - i, u = psi / delta - j
    int n_cmap; const int* cmap_atoms; const int* cmap_grid; const double* cmap_coef;
    // Urey-Bradley terms: 2 atoms and (r0, k) per term; impropers: 4 atoms and (psi0, k) per term
    int n_ub; const int* ub_atoms; const double* ub_params;
    int n_impr; const int* impr_atoms; const double* impr_params;
};

__device__ inline void mi3(const BondedArgs& B, double d[3]) {
    if (B.periodic) for (int k = 0; k < 3; k++) d[k] = min_image_d(d[k], B.box.L[k], B.box.invL[k]);
}
__device__ inline void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// ---- CMAP: the dihedral of T_TORSION below (same vectors, sign rule and minimum image) shifted into [0, 2 pi], with what its
// position gradient needs
struct CmapDihedral { double m[3], nn[3], m2, n2, lkj, p, qq, phi, raw; };   // (raw: the angle in (-pi, pi], before the shift)
__device__ inline void cmap_dihedral(const BondedArgs& B, const int* q, CmapDihedral& D) {
    double rij[3], rkj[3], rkl[3];
    for (int c = 0; c < 3; c++) { rij[c] = B.x[c][q[0]] - B.x[c][q[1]]; rkj[c] = B.x[c][q[2]] - B.x[c][q[1]]; rkl[c] = B.x[c][q[2]] - B.x[c][q[3]]; }
    mi3(B, rij); mi3(B, rkj); mi3(B, rkl);
    cross3(rij, rkj, D.m); cross3(rkj, rkl, D.nn);
    D.m2 = dot3(D.m, D.m); D.n2 = dot3(D.nn, D.nn);
    const double lkj2 = dot3(rkj, rkj);
    D.lkj = sqrt(lkj2);
    // T_TORSION's angle -- cos = m.n / |m||n|, negative where rij.n < 0 -- taken as atan2(|rkj| rij.n, m.n): the same angle with the same
    // sign rule, but acos loses half its digits near 0 and pi (1e-8 rad), and here the angle picks the patch and the place within it
    const double phi = atan2(D.lkj * dot3(rij, D.nn), dot3(D.m, D.nn));
    D.phi = phi < 0.0 ? phi + CMAP_TWO_PI : phi; D.raw = phi;
    D.p = dot3(rij, rkj) / lkj2; D.qq = dot3(rkl, rkj) / lkj2;
}
// F += -ddphi * d(phi)/d(x of the atom in `role`): T_TORSION's fi, fl, sv expressions
__device__ inline void cmap_project(const CmapDihedral& D, const double ddphi, const int role, double F[3]) {
    for (int c = 0; c < 3; c++) {
        const double fi = -ddphi * D.lkj / D.m2 * D.m[c], fl = ddphi * D.lkj / D.n2 * D.nn[c];
        const double sv = D.p * fi - D.qq * fl;
        F[c] += role == 0 ? fi : (role == 1 ? -(fi - sv) : (role == 2 ? -(fl + sv) : fl));
    }
}
// patch index and local coordinate of an angle in [0, 2 pi] (-tiny + 2 pi rounds to 2 pi: patch n - 1 at t = 1, which continues patch 0 at t = 0)
__device__ inline int cmap_patch(const double ang, const int n, double* t) {
    const double s = ang * ((double)n / CMAP_TWO_PI);
    int i = (int)s; i = i > n - 1 ? n - 1 : (i < 0 ? 0 : i);
    *t = s - (double)i;
    return i;
}
__device__ inline double cmap_term(const BondedArgs& B, const int idx, const int role, double F[3]) {
    const int* q = B.cmap_atoms + 8 * idx;
    const int n = B.cmap_grid[2 * idx];
    CmapDihedral A, C;
    cmap_dihedral(B, q, A); cmap_dihedral(B, q + 4, C);
    double t, u;
    const int i = cmap_patch(A.phi, n, &t), j = cmap_patch(C.phi, n, &u);
    // the patch's 16 coefficients lie together, 128 B on a 128 B boundary: four 32 B loads
    const double4* cp = reinterpret_cast<const double4*>(B.cmap_coef + 16 * ((size_t)B.cmap_grid[2 * idx + 1] + (size_t)(i + n * j)));
    double e = 0.0, et = 0.0, eu = 0.0;
    for (int a = 3; a >= 0; a--) {   // Horner in t over rows r_a(u) = sum_b c[a][b] u^b, with d/dt and d/du carried along
        const double4 c = cp[a];
        const double r = ((c.w * u + c.z) * u + c.y) * u + c.x, ru = (3.0 * c.w * u + 2.0 * c.z) * u + c.y;
        et = et * t + e; e = e * t + r; eu = eu * t + ru;
    }
    if (role >= 0) {   // the entry's atom may sit in both dihedrals (Amber's five-atom form): every place that names it, in place order
        const double scale = (double)n / CMAP_TWO_PI;
        const int me = q[role];
        for (int pl = 0; pl < 8; pl++)
            if (q[pl] == me) cmap_project(pl < 4 ? A : C, (pl < 4 ? et : eu) * scale, pl & 3, F);
    }
    return e;
}

// ---- Urey-Bradley: T_BOND's expressions over the term's own arrays (minimum image, E = 0.5 k (r - r0)^2)
__device__ inline double urey_bradley_term(const BondedArgs& B, const int idx, const int role, double F[3]) {
    const int i = B.ub_atoms[2 * idx], j = B.ub_atoms[2 * idx + 1];
    const double r0 = B.ub_params[2 * idx], k = B.ub_params[2 * idx + 1];
    double d[3] = {B.x[0][i] - B.x[0][j], B.x[1][i] - B.x[1][j], B.x[2][i] - B.x[2][j]};
    mi3(B, d);
    const double r = sqrt(dot3(d, d)), dr = r - r0, fs = -k * dr / r;
    const double sgn = role == 0 ? 1.0 : -1.0;
    if (role >= 0) for (int c = 0; c < 3; c++) F[c] = sgn * fs * d[c];
    return 0.5 * k * dr * dr;
}
// ---- harmonic improper: E = k delta^2, delta = psi - psi0 wrapped into (-pi, pi], psi the dihedral 1-2-3-4 through atan2 (the terms sit
// at psi ~ psi0 = 0, where acos keeps half its digits and the energy is quadratic in the angle); dE/dpsi = 2 k delta, distributed as T_TORSION's
__device__ inline double improper_term(const BondedArgs& B, const int idx, const int role, double F[3]) {
    CmapDihedral D;
    cmap_dihedral(B, B.impr_atoms + 4 * idx, D);
    const double psi0 = B.impr_params[2 * idx], k = B.impr_params[2 * idx + 1];
    double delta = D.raw - psi0;
    delta = delta > IMPR_PI ? delta - CMAP_TWO_PI : (delta <= -IMPR_PI ? delta + CMAP_TWO_PI : delta);
    if (role >= 0) cmap_project(D, 2.0 * k * delta, role, F);
    return k * delta * delta;
}

// energy of term (type, idx); if role >= 0 also the force on the atom in that role
template <bool CENT = false, bool CMAP = false>
__device__ inline double bonded_term(const BondedArgs& B, int type, int idx, int role, double F[3]) {
    F[0] = F[1] = F[2] = 0.0;
    if constexpr (CMAP) {
        if (type == T_CMAP) return cmap_term(B, idx, role, F);
        if (type == T_UREY) return urey_bradley_term(B, idx, role, F);
        if (type == T_IMPR) return improper_term(B, idx, role, F);
    }
    if constexpr (CENT) {
        if (type == T_CENT) {  // E = 0.5 k |c1 - c2|^2, c = sum(w x) / sum(w): explicit weights, summed in the groups' order; never periodic
            const int* q = B.cent_atoms + 2 * CENT_GROUP * idx;
            const double* w = B.cent_params + (2 * CENT_GROUP + 1) * idx;
            const double kk = w[2 * CENT_GROUP];
            double c[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, W[2] = {0.0, 0.0};
            for (int g = 0; g < 2; g++)
                for (int s = 0; s < CENT_GROUP; s++) {
                    const int a = q[g * CENT_GROUP + s];
                    if (a < 0) break;
                    const double ws = w[g * CENT_GROUP + s];
                    W[g] += ws;
                    for (int m = 0; m < 3; m++) c[g][m] += ws * B.x[m][a];
                }
            double d[3];
            for (int m = 0; m < 3; m++) d[m] = c[0][m] / W[0] - c[1][m] / W[1];
            if (role >= 0) {   // role = the member's place: group 1 is pulled towards group 2 and the other way round
                const int g = role / CENT_GROUP;
                for (int m = 0; m < 3; m++) { const double f = kk * d[m] * w[role] / W[g]; F[m] = g == 0 ? -f : f; }
            }
            return 0.5 * kk * dot3(d, d);
        }
    }
    if (type == T_BOND) {
        const int i = B.atoms[T_BOND][2 * idx], j = B.atoms[T_BOND][2 * idx + 1];
        const double r0 = B.params[T_BOND][2 * idx], k = B.params[T_BOND][2 * idx + 1];
        double d[3] = {B.x[0][i] - B.x[0][j], B.x[1][i] - B.x[1][j], B.x[2][i] - B.x[2][j]};
        mi3(B, d);
        const double r = sqrt(dot3(d, d)), dr = r - r0, fs = -k * dr / r;
        const double sgn = role == 0 ? 1.0 : -1.0;
        if (role >= 0) for (int c = 0; c < 3; c++) F[c] = sgn * fs * d[c];
        return 0.5 * k * dr * dr;
    }
    if (type == T_ANGLE) {
        const int i = B.atoms[T_ANGLE][3 * idx], j = B.atoms[T_ANGLE][3 * idx + 1], k_ = B.atoms[T_ANGLE][3 * idx + 2];
        const double t0 = B.params[T_ANGLE][2 * idx], kk = B.params[T_ANGLE][2 * idx + 1];
        double u[3] = {B.x[0][i] - B.x[0][j], B.x[1][i] - B.x[1][j], B.x[2][i] - B.x[2][j]};
        double w[3] = {B.x[0][k_] - B.x[0][j], B.x[1][k_] - B.x[1][j], B.x[2][k_] - B.x[2][j]};
        mi3(B, u); mi3(B, w);
        const double lu = sqrt(dot3(u, u)), lw = sqrt(dot3(w, w));
        double c = dot3(u, w) / (lu * lw);
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
        const double th = acos(c), dth = th - t0;
        if (role >= 0) {
            double s = sqrt(1.0 - c * c); if (s < 1e-12) s = 1e-12;
            const double pre = kk * dth / s;
            for (int m = 0; m < 3; m++) {
                const double fi = pre * (w[m] / (lu * lw) - c * u[m] / (lu * lu));
                const double fk = pre * (u[m] / (lu * lw) - c * w[m] / (lw * lw));
                F[m] = role == 0 ? fi : (role == 2 ? fk : -(fi + fk));
            }
        }
        return 0.5 * kk * dth * dth;
    }
    if (type == T_TORSION) {
        const int* q = B.atoms[T_TORSION] + 4 * idx;
        const double per = B.params[T_TORSION][3 * idx], ph = B.params[T_TORSION][3 * idx + 1], kk = B.params[T_TORSION][3 * idx + 2];
        double rij[3], rkj[3], rkl[3], m[3], nn[3];
        for (int c = 0; c < 3; c++) { rij[c] = B.x[c][q[0]] - B.x[c][q[1]]; rkj[c] = B.x[c][q[2]] - B.x[c][q[1]]; rkl[c] = B.x[c][q[2]] - B.x[c][q[3]]; }
        mi3(B, rij); mi3(B, rkj); mi3(B, rkl);
        cross3(rij, rkj, m); cross3(rkj, rkl, nn);
        const double m2 = dot3(m, m), n2 = dot3(nn, nn), lkj2 = dot3(rkj, rkj), lkj = sqrt(lkj2);
        double cs = dot3(m, nn) / sqrt(m2 * n2);
        cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
        double phi = acos(cs); if (dot3(rij, nn) < 0.0) phi = -phi;
        if (role >= 0) {
            const double ddphi = -kk * per * sin(per * phi - ph);
            const double p = dot3(rij, rkj) / lkj2, qq = dot3(rkl, rkj) / lkj2;
            for (int c = 0; c < 3; c++) {
                const double fi = -ddphi * lkj / m2 * m[c], fl = ddphi * lkj / n2 * nn[c];
                const double sv = p * fi - qq * fl;
                F[c] = role == 0 ? fi : (role == 1 ? -(fi - sv) : (role == 2 ? -(fl + sv) : fl));
            }
        }
        return kk * (1.0 + cos(per * phi - ph));
    }
    if (type == T_EXC) {  // env-env 1-4: plain LJ + bare Coulomb, no cutoff
        const int i = B.atoms[T_EXC][2 * idx], j = B.atoms[T_EXC][2 * idx + 1];
        const double qq = B.params[T_EXC][3 * idx], sig = B.params[T_EXC][3 * idx + 1], eps = B.params[T_EXC][3 * idx + 2];
        double d[3] = {B.x[0][i] - B.x[0][j], B.x[1][i] - B.x[1][j], B.x[2][i] - B.x[2][j]};
        mi3(B, d);
        const double r2 = dot3(d, d);
        double fs, fc;
        const double e = plain_lj_d(r2, sig, eps, &fs) + coulomb_d(r2, qq, 0.0, false, &fc);
        const double sgn = role == 0 ? 1.0 : -1.0;
        if (role >= 0) for (int c = 0; c < 3; c++) F[c] = sgn * (fs + fc) * d[c];
        return e;
    }
    if (type == T_EWEX) {  // excluded pair under PME: its reciprocal-space interaction is taken out, -ONE_4PI_EPS0 q_i q_j erf(alpha r) / r
        const int i = B.atoms[T_EWEX][2 * idx], j = B.atoms[T_EWEX][2 * idx + 1];
        const double pre = ONE_4PI_EPS0 * B.params[T_EWEX][idx], al = B.ewald_alpha;
        double d[3] = {B.x[0][i] - B.x[0][j], B.x[1][i] - B.x[1][j], B.x[2][i] - B.x[2][j]};
        mi3(B, d);
        const double r2 = dot3(d, d), r = sqrt(r2), er = erf(al * r);
        if (role >= 0) {
            const double dEdr = -pre * (TWO_OVER_SQRT_PI * al * exp(-al * al * r2) / r - er / r2);
            const double fs = -dEdr / r, sgn = role == 0 ? 1.0 : -1.0;
            for (int c = 0; c < 3; c++) F[c] = sgn * fs * d[c];
        }
        return -pre * er / r;
    }
    // T_RESTR
    const int i = B.atoms[T_RESTR][idx];
    double d[3] = {B.x[0][i] - B.params[T_RESTR][3 * idx], B.x[1][i] - B.params[T_RESTR][3 * idx + 1], B.x[2][i] - B.params[T_RESTR][3 * idx + 2]};
    mi3(B, d);
    if (role >= 0) for (int c = 0; c < 3; c++) F[c] = -2.0 * B.restr_k * d[c];
    return B.restr_k * dot3(d, d);
}

// one thread per (row, entry): the force of one term on one of its mobile atoms -> fent[3][n_entries];
// blocks past n_entry_blocks draw the N(0,1) numbers of the coming O substeps (counter-based, so they can be
// produced before the velocities they will be applied to exist).
template <bool CENT = false, bool CMAP = false>
__device__ __forceinline__ void bonded_entries_body(const BondedArgs& B, const int block_id, const int nthreads) {
    if (block_id >= B.n_entry_blocks) {
        const int g = (block_id - B.n_entry_blocks) * nthreads + threadIdx.x;
        if (g >= B.n_mobile * B.n_noise) return;
        const int d = g / B.n_mobile, m = g - d * B.n_mobile;
        double z[3];
        gaussians3(B.seed, B.stream, B.draw_base + (unsigned)d, (unsigned)B.mobile_atoms[m], z);
        for (int k = 0; k < 3; k++) B.noise[(size_t)(d * 3 + k) * B.n_mobile + m] = z[k];
        return;
    }
    const int e = block_id * nthreads + threadIdx.x;
    if (e >= B.n_entries) return;
    double F[3];
    bonded_term<CENT, CMAP>(B, B.ent_type[e], B.ent_term[e], B.ent_role[e], F);
    B.fent[e] = F[0]; B.fent[B.n_entries + e] = F[1]; B.fent[2 * B.n_entries + e] = F[2];
}

template <bool CENT = false, bool CMAP = false>
__global__ void __launch_bounds__(128) k_bonded_entries(BondedArgs B) { bonded_entries_body<CENT, CMAP>(B, blockIdx.x, 128); }

// energy of every term (frozen ones included): per-block partial sums per type
// (CENT: the centroid bonds follow the six types; their energy goes into the restraint's partial -- both are energy term 7;
//  CMAP: the CMAP torsions follow those; their energy goes into the torsions' partial -- both are energy term 2; then the
//  Urey-Bradley terms, into the bonds' partial -- energy term 0 --, and the impropers, into the torsions')
template <bool CENT = false, bool CMAP = false>
__device__ __forceinline__ void bonded_energy_body(const BondedArgs& B) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    double e[T_NTYPES] = {0, 0, 0, 0, 0, 0};
    int base = 0;
    for (int ty = 0; ty < T_NTYPES; ty++) {
        const int idx = gid - base;
        if (idx >= 0 && idx < B.n_terms[ty]) { double F[3]; e[ty] = bonded_term(B, ty, idx, -1, F); }
        base += B.n_terms[ty];
    }
    if constexpr (CENT) {
        const int idx = gid - base;
        if (idx >= 0 && idx < B.n_cent) { double F[3]; e[T_RESTR] += bonded_term<true>(B, T_CENT, idx, -1, F); }
        base += B.n_cent;
    }
    if constexpr (CMAP) {
        const int idx = gid - base;
        if (idx >= 0 && idx < B.n_cmap) { double F[3]; e[T_TORSION] += cmap_term(B, idx, -1, F); }
        base += B.n_cmap;
        const int iu = gid - base;
        if (iu >= 0 && iu < B.n_ub) { double F[3]; e[T_BOND] += urey_bradley_term(B, iu, -1, F); }
        base += B.n_ub;
        const int ii = gid - base;
        if (ii >= 0 && ii < B.n_impr) { double F[3]; e[T_TORSION] += improper_term(B, ii, -1, F); }
    }
    __shared__ double s[4][T_NTYPES];
    for (int ty = 0; ty < T_NTYPES; ty++) { double v = wave_sum(e[ty]); if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6][ty] = v; }
    __syncthreads();
    if (threadIdx.x < T_NTYPES) B.epart[blockIdx.x * T_NTYPES + threadIdx.x] = s[0][threadIdx.x] + s[1][threadIdx.x] + s[2][threadIdx.x] + s[3][threadIdx.x];
}

template <bool CENT = false, bool CMAP = false>
__global__ void __launch_bounds__(256) k_bonded_energy(BondedArgs B) { bonded_energy_body<CENT, CMAP>(B); }
