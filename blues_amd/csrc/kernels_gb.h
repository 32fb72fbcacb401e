// kernels_gb.h -- implicit solvent of a NoCutoff System: GB-OBC (OpenMM's GBSAOBCForce) with the ACE surface term.
//
//   o_i = rho_i - 0.009, s_i = S_i o_i
//   I_i = o_i / 2 * sum_{j != i, o_i < r + s_j} term(r, o_i, s_j)                                   (descreening)
//   B_i = 1 / (1/o_i - tanh(alpha I - beta I^2 + gamma I^3) / rho_i)                                (Born radius)
//   E   = -pref [ 1/2 sum_i q~_i^2 / B_i + sum_{i<j} q~_i q~_j / f_ij ] + sum_i c_i sa (rho_i + 0.14)^2 (rho_i / B_i)^6
//   f_ij = sqrt(r^2 + B_i B_j exp(-r^2 / (4 B_i B_j))),  pref = ONE_4PI_EPS0 (1/eps_in - 1/eps_out), sa = 4 pi * surface_area_energy
// Exclusions play no part.  An alchemical atom carries q~ = lambda_electrostatics q and c = lambda_electrostatics, so at fixed positions
//   E(le) = E0 + le E1 + le^2 E2, and so do the forces and dE/dB_i: a pair belongs to class a_i + a_j (a = 1 for an alchemical
// atom), a self term to class 2 a_i, a surface term to class a_i.  Every kernel keeps the three coefficients; lambda enters as
// multiplications where the slots' forces are written (gb_chain_body) and where the sums are formed (k_finalize, the host).
//
// Three all-pairs passes in the manner of kernels_nocutoff.h: one thread per i-atom (every atom, frozen ones included), the j-atoms
// staged in LDS 256 at a time and walked in caller order, every pair evaluated from both ends, no atomics -- a thread's sums run over
// j in an order that depends on n only; lone chains and batches run the same kernels (below), so a chain gets the same bits either way.
//   1. gb_born_body:  I_i -> B_i and the chain factor dB_i/dI_i * o_i/2
//   2. gb_pair_body:  energy partials per block, the direct force on i, dE/dB_i (times the chain factor: G_i), three coefficients each
//   3. gb_chain_body: force on i from G_i d term_ij/dr and from every j's G_j d term_ji/dr; adds the direct force and writes the
//      slots' forces [9][n] that k_finalize adds (zero for frozen atoms)
// d term / dr = -2 t3 with t3 = (1 + s^2/r^2)(l^2 - u^2)/8 + ln(u/l) / (4 r^2): the parts through l and u cancel (or l is constant).
//
// Mixed precision (R = float): coordinates relative to the block's first atom as two fp32 numbers (kernels_nocutoff.h), pair
// arithmetic fp32; the per-atom sums, I_i, the tanh, B_i and every energy are fp64.  For a separated pair (r - s_j >= o_i) the term is
//   term = (x / (1 - x^2) - atanh x) / r = sum_k 2k/(2k+1) x^(2k+1) / r,  x = s_j / r
// -- the small difference of O(1/r) quantities that fp32 loses to cancellation -- so for x <= 0.4 the fp32 path sums the series (twelve
// terms: the first one left out is 0.16^12 of the leading one), and likewise for the derivative, sum_k 2k(2k+2)/(2k+1) x^(2k+1) / r^2.
// Every other pair -- close, overlapping, engulfed -- takes the closed form in fp64 in both precisions: for atoms that overlap (a
// decoupled ligand lets others in) its 1/r terms cancel.  Double precision: the closed forms throughout.
#pragma once
#include "device_common.h"

#define GB_THREADS 256
#define GB_NE 6   // energy partials of a block: polar E0, E1, E2, surface E0, E1, (unused)

struct GbArgs {
    int active;                 // (batched form) 0: the member sits this launch out
    int n;
    const double* x[3];         // positions, caller order
    const double4* par;         // [n] {charge, o = rho - 0.009, s = S o, rho}
    const int* alch;            // [n] 1 for an alchemical atom
    const double* mass;         // [n] 0: frozen (no force)
    double alpha, beta, gamma;  // OBC1 / OBC2
    double pref, sa;            // ONE_4PI_EPS0 (1/eps_in - 1/eps_out); 4 pi surface_area_energy
    double* born;               // [2][n] B_i, dB_i/dI_i * o_i / 2
    double* G;                  // [3][n] dE/dB_i * chain factor, per class
    double* fdir;               // [9][n] direct force per class
    double* fgb;                // [9][n] force per slot (k_finalize)
    double* epart;              // [blocks][GB_NE]
};
struct GbDyn { double le[3]; };   // lambda_electrostatics of the pass's three slots

template <typename R> __device__ __forceinline__ R gb_series(R x, const R* c) {
    const R x2 = x * x;
    R p = c[11];
#pragma unroll
    for (int k = 10; k >= 0; k--) p = p * x2 + c[k];
    return p * x2 * x;
}
// term(r, o_i, s_j)
template <typename R> __device__ __forceinline__ R gb_term(R r, R inv_r, R o, R s) {
    const R U = r + s;
    if (!(o < U)) return (R)0;
    const R dm = r - s;
    if constexpr (sizeof(R) == 4) {
        if (dm >= o && s <= (R)0.4 * r) {
            const R c[12] = {(R)(2.0 / 3), (R)(4.0 / 5), (R)(6.0 / 7), (R)(8.0 / 9), (R)(10.0 / 11), (R)(12.0 / 13), (R)(14.0 / 15), (R)(16.0 / 17), (R)(18.0 / 19), (R)(20.0 / 21), (R)(22.0 / 23), (R)(24.0 / 25)};
            return gb_series<R>(s * inv_r, c) * inv_r;
        }
    }
    // (the closed form in fp64 in either precision: for a pair closer than its radii -- an atom inside a decoupled ligand's -- the
    // terms in 1/r cancel each other and fp32 keeps no digit of what is left)
    const double rd = r, od = o, sd = s, ird = 1.0 / rd;
    const double L = max(od, fabs(rd - sd)), l = 1.0 / L, u = 1.0 / (rd + sd);
    const double dl = l * l - u * u;
    double t = l - u - 0.25 * rd * dl + 0.5 * log(u * L) * ird + 0.25 * sd * sd * ird * dl;
    if (od < sd - rd) t += 2.0 * (1.0 / od - l);
    return (R)t;
}
// -(d term / dr) / r = 2 t3 / r
template <typename R> __device__ __forceinline__ R gb_dterm(R r, R inv_r, R o, R s) {
    const R U = r + s;
    if (!(o < U)) return (R)0;
    const R dm = r - s, inv_r2 = inv_r * inv_r;
    if constexpr (sizeof(R) == 4) {
        if (dm >= o && s <= (R)0.4 * r) {
            const R c[12] = {(R)(8.0 / 3), (R)(24.0 / 5), (R)(48.0 / 7), (R)(80.0 / 9), (R)(120.0 / 11), (R)(168.0 / 13), (R)(224.0 / 15), (R)(288.0 / 17), (R)(360.0 / 19), (R)(440.0 / 21), (R)(528.0 / 23), (R)(624.0 / 25)};
            return gb_series<R>(s * inv_r, c) * inv_r2 * inv_r;
        }
    }
    const double rd = r, od = o, sd = s, ird = 1.0 / rd, ird2 = ird * ird;   // (fp64 in either precision: see gb_term)
    const double L = max(od, fabs(rd - sd)), l = 1.0 / L, u = 1.0 / (rd + sd);
    const double t3 = 0.125 * (1.0 + sd * sd * ird2) * (l * l - u * u) + 0.25 * log(u * L) * ird2;
    return (R)(2.0 * t3 * ird);
}

// the j-tile's coordinates relative to (xr0, xr1, xr2): rounded value and, in mixed precision, what the rounding left
template <typename R> struct GbTile {
    static constexpr bool SPLIT = sizeof(R) == 4;
    R x[GB_THREADS], y[GB_THREADS], z[GB_THREADS];
    R lx[SPLIT ? GB_THREADS : 1], ly[SPLIT ? GB_THREADS : 1], lz[SPLIT ? GB_THREADS : 1];
    __device__ __forceinline__ void put(int t, double dx, double dy, double dz) {
        x[t] = (R)dx; y[t] = (R)dy; z[t] = (R)dz;
        if constexpr (SPLIT) { lx[t] = (R)(dx - (double)(R)dx); ly[t] = (R)(dy - (double)(R)dy); lz[t] = (R)(dz - (double)(R)dz); }
    }
};
template <typename R> struct GbPoint {
    R x = (R)0, y = (R)0, z = (R)0, lx = (R)0, ly = (R)0, lz = (R)0;
    __device__ __forceinline__ void set(double dx, double dy, double dz) {
        x = (R)dx; y = (R)dy; z = (R)dz;
        if constexpr (sizeof(R) == 4) { lx = (R)(dx - (double)x); ly = (R)(dy - (double)y); lz = (R)(dz - (double)z); }
    }
    __device__ __forceinline__ void sep(const GbTile<R>& T, int u, R& dx, R& dy, R& dz) const {
        dx = x - T.x[u]; dy = y - T.y[u]; dz = z - T.z[u];
        if constexpr (sizeof(R) == 4) { dx += lx - T.lx[u]; dy += ly - T.ly[u]; dz += lz - T.lz[u]; }
    }
};

// ---- 1. Born radii
template <typename R>
__device__ __forceinline__ void gb_born_body(const GbArgs& A, const int blk) {
    __shared__ GbTile<R> T;
    __shared__ R ss[GB_THREADS];
    const int tid = threadIdx.x;
    const int i = blk * GB_THREADS + tid < A.n ? blk * GB_THREADS + tid : -1;
    const int i0 = blk * GB_THREADS;   // (the block's reference point: its first atom)
    const double xr0 = A.x[0][i0], xr1 = A.x[1][i0], xr2 = A.x[2][i0];
    GbPoint<R> P; R oi = (R)0;
    double4 Pi = make_double4(0.0, 0.0, 0.0, 0.0);
    if (i >= 0) { P.set(A.x[0][i] - xr0, A.x[1][i] - xr1, A.x[2][i] - xr2); Pi = A.par[i]; oi = (R)Pi.y; }
    double sum = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += GB_THREADS) {
        __syncthreads();   // (the previous tile has been read by every thread)
        const int j = j0 + tid;
        if (j < A.n) { T.put(tid, A.x[0][j] - xr0, A.x[1][j] - xr1, A.x[2][j] - xr2); ss[tid] = (R)A.par[j].z; }
        __syncthreads();
        if (i < 0) continue;
        const int jn = min(GB_THREADS, A.n - j0);
        for (int u = 0; u < jn; u++) {
            if (j0 + u == i) continue;
            R dx, dy, dz; P.sep(T, u, dx, dy, dz);
            const R r2 = dx * dx + dy * dy + dz * dz, inv_r = (R)1 / sqrt(r2), r = r2 * inv_r;
            sum += (double)gb_term<R>(r, inv_r, oi, ss[u]);
        }
    }
    if (i < 0) return;
    const double o = Pi.y, rho = Pi.w, psi = 0.5 * o * sum;
    const double t = tanh(psi * (A.alpha + psi * (-A.beta + psi * A.gamma)));
    const double B = 1.0 / (1.0 / o - t / rho);
    A.born[i] = B;
    A.born[(size_t)A.n + i] = B * B * (1.0 - t * t) * (A.alpha + psi * (-2.0 * A.beta + 3.0 * A.gamma * psi)) / rho * 0.5 * o;
}

// ---- 2. pairs: energies, direct force, dE/dB.  ENERGY: the energy partials only (nothing per atom is written)
template <typename R, bool ENERGY>
__device__ __forceinline__ void gb_pair_body(const GbArgs& A, const int blk) {
    __shared__ GbTile<R> T;
    __shared__ R sq[GB_THREADS], sb[GB_THREADS], sib[GB_THREADS];   // charge, B_j, 1 / B_j
    __shared__ int sa[GB_THREADS];
    __shared__ double s_e[GB_THREADS / 64][GB_NE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = blk * GB_THREADS + tid < A.n ? blk * GB_THREADS + tid : -1;
    const int i0 = blk * GB_THREADS;
    const double xr0 = A.x[0][i0], xr1 = A.x[1][i0], xr2 = A.x[2][i0];
    GbPoint<R> P; R qi = (R)0, bi = (R)1;
    if (i >= 0) { P.set(A.x[0][i] - xr0, A.x[1][i] - xr1, A.x[2][i] - xr2); qi = (R)A.par[i].x; bi = (R)A.born[i]; }
    const R q_inv4b = (R)0.25 / bi;
    // sums over j by the class of j (0: environment, 1: alchemical): energy q q / f, force scale, dE/dB_i
    double e[2] = {0.0, 0.0}, g[2] = {0.0, 0.0}, f[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int j0 = 0; j0 < A.n; j0 += GB_THREADS) {
        __syncthreads();
        const int j = j0 + tid;
        if (j < A.n) { T.put(tid, A.x[0][j] - xr0, A.x[1][j] - xr1, A.x[2][j] - xr2); const double bj = A.born[j]; sq[tid] = (R)A.par[j].x; sb[tid] = (R)bj; sib[tid] = (R)(1.0 / bj); sa[tid] = A.alch[j]; }
        __syncthreads();
        if (i < 0) continue;
        const int jn = min(GB_THREADS, A.n - j0);
        for (int u = 0; u < jn; u++) {
            if (j0 + u == i) continue;
            R dx, dy, dz; P.sep(T, u, dx, dy, dz);
            const R r2 = dx * dx + dy * dy + dz * dz;
            const R bj = sb[u], D = bi * bj;
            const R ex = exp(-(r2 * q_inv4b) * sib[u]);   // (-r^2 / (4 B_i B_j) without a division: 1 / (4 B_i) is the thread's, 1 / B_j staged)
            const R inv_f = (R)1 / sqrt(r2 + D * ex);
            const R qq = qi * sq[u], ee = qq * inv_f;
            const R qf3 = ee * inv_f * inv_f;
            const R fs = qf3 * ((R)1 - (R)0.25 * ex), gg = (R)0.5 * qf3 * ex * (bj + r2 * q_inv4b);
            if (sa[u]) {   // (the same for every thread of the wave: no divergence; constant indices keep the sums in registers)
                e[1] += (double)ee;
                if (!ENERGY) { g[1] += (double)gg; f[1][0] += (double)(fs * dx); f[1][1] += (double)(fs * dy); f[1][2] += (double)(fs * dz); }
            } else {
                e[0] += (double)ee;
                if (!ENERGY) { g[0] += (double)gg; f[0][0] += (double)(fs * dx); f[0][1] += (double)(fs * dy); f[0][2] += (double)(fs * dz); }
            }
        }
    }
    // this atom's share of the energy per class: half of each pair, the self term (class 2 a_i), the surface term (class a_i)
    double E[GB_NE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i >= 0) {
        const double4 Pi = A.par[i];
        const int a = A.alch[i];
        const double B = A.born[i], rb = Pi.w / B, rb3 = rb * rb * rb;
        const double self = 0.5 * Pi.x * Pi.x / B;
        const double esa = A.sa * (Pi.w + 0.14) * (Pi.w + 0.14) * rb3 * rb3;
        const double p0 = -A.pref * 0.5 * e[0], p1 = -A.pref * 0.5 * e[1], ps = -A.pref * self;
        // (constant indices: a == 0 -> classes 0, 1 and self in 0; a == 1 -> classes 1, 2 and self in 2)
        E[0] = a ? 0.0 : p0 + ps; E[1] = a ? p0 : p1; E[2] = a ? p1 + ps : 0.0;
        E[3] = a ? 0.0 : esa; E[4] = a ? esa : 0.0;
        if (!ENERGY) {
            const double ch = A.born[(size_t)A.n + i];
            const double g0 = A.pref * g[0], g1 = A.pref * g[1], gs = A.pref * self / B, ga = -6.0 * esa / B;
            const size_t n = A.n;
            A.G[i] = ch * (a ? 0.0 : g0 + gs + ga);
            A.G[n + i] = ch * (a ? g0 + ga : g1);
            A.G[2 * n + i] = ch * (a ? g1 + gs : 0.0);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double d0 = -A.pref * f[0][k], d1 = -A.pref * f[1][k];
                A.fdir[(size_t)k * n + i] = a ? 0.0 : d0;
                A.fdir[(size_t)(3 + k) * n + i] = a ? d0 : d1;
                A.fdir[(size_t)(6 + k) * n + i] = a ? d1 : 0.0;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < GB_NE; q++) { const double s = wave_sum(E[q]); if (lane == 0) s_e[wv][q] = s; }
    __syncthreads();
    if (tid < GB_NE) {
        double s = 0.0;
        for (int w = 0; w < GB_THREADS / 64; w++) s += s_e[w][tid];
        A.epart[(size_t)blk * GB_NE + tid] = s;
    }
}

// ---- 3. the chain term, and the slots' forces
template <typename R>
__device__ __forceinline__ void gb_chain_body(const GbArgs& A, const GbDyn& dyn, const int blk) {
    __shared__ GbTile<R> T;
    __shared__ R so[GB_THREADS], ss[GB_THREADS], sg[3][GB_THREADS];
    const int tid = threadIdx.x;
    const int ia = blk * GB_THREADS + tid < A.n ? blk * GB_THREADS + tid : -1;
    const int i = ia >= 0 && A.mass[ia] != 0.0 ? ia : -1;   // (a frozen atom receives no force: nothing to sum)
    const int i0 = blk * GB_THREADS;
    const double xr0 = A.x[0][i0], xr1 = A.x[1][i0], xr2 = A.x[2][i0];
    const size_t n = A.n;
    GbPoint<R> P; R oi = (R)0, si = (R)0;
    if (i >= 0) { P.set(A.x[0][i] - xr0, A.x[1][i] - xr1, A.x[2][i] - xr2); const double4 Pi = A.par[i]; oi = (R)Pi.y; si = (R)Pi.z; }
    double own[3] = {0.0, 0.0, 0.0};       // sum_j w_ij d (times G_i[c] at the end)
    double oth[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};   // sum_j G_j[c] w_ji d
    for (int j0 = 0; j0 < A.n; j0 += GB_THREADS) {
        __syncthreads();
        const int j = j0 + tid;
        if (j < A.n) {
            T.put(tid, A.x[0][j] - xr0, A.x[1][j] - xr1, A.x[2][j] - xr2);
            const double4 Pj = A.par[j];
            so[tid] = (R)Pj.y; ss[tid] = (R)Pj.z;
            sg[0][tid] = (R)A.G[j]; sg[1][tid] = (R)A.G[n + j]; sg[2][tid] = (R)A.G[2 * n + j];
        }
        __syncthreads();
        if (i < 0) continue;
        const int jn = min(GB_THREADS, A.n - j0);
        for (int u = 0; u < jn; u++) {
            if (j0 + u == i) continue;
            R dx, dy, dz; P.sep(T, u, dx, dy, dz);
            const R r2 = dx * dx + dy * dy + dz * dz, inv_r = (R)1 / sqrt(r2), r = r2 * inv_r;
            const R wij = gb_dterm<R>(r, inv_r, oi, ss[u]), wji = gb_dterm<R>(r, inv_r, so[u], si);
            own[0] += (double)(wij * dx); own[1] += (double)(wij * dy); own[2] += (double)(wij * dz);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const R gw = sg[c][u] * wji;
                oth[c][0] += (double)(gw * dx); oth[c][1] += (double)(gw * dy); oth[c][2] += (double)(gw * dz);
            }
        }
    }
    if (ia < 0) return;
    double F[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double Gi = i >= 0 ? A.G[(size_t)c * n + i] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) F[c][k] = i >= 0 ? A.fdir[(size_t)(c * 3 + k) * n + i] + (Gi * own[k] + oth[c][k]) : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
        for (int k = 0; k < 3; k++) A.fgb[(size_t)(s * 3 + k) * n + ia] = F[0][k] + dyn.le[s] * (F[1][k] + dyn.le[s] * F[2][k]);
}

// One set of kernels for a lone chain and a batch: blockIdx.y = member, its record in HBM (a lone engine launches them over its own
// one record).  The same machine code either way, so no choice the compiler makes between two instantiations of a body (which
// multiply-adds it fuses) can separate a batch member from the same chain alone.
template <typename R> __global__ void __launch_bounds__(GB_THREADS) k_gb_born_b(const GbArgs* __restrict__ recs) {
    const GbArgs& A = recs[blockIdx.y];
    if (!A.active) return;
    gb_born_body<R>(A, blockIdx.x);
}
template <typename R, bool ENERGY> __global__ void __launch_bounds__(GB_THREADS) k_gb_pairs_b(const GbArgs* __restrict__ recs) {
    const GbArgs& A = recs[blockIdx.y];
    if (!A.active) return;
    gb_pair_body<R, ENERGY>(A, blockIdx.x);
}
template <typename R> __global__ void __launch_bounds__(GB_THREADS) k_gb_chain_b(const GbArgs* __restrict__ recs, GbDyn d) {
    const GbArgs& A = recs[blockIdx.y];
    if (!A.active) return;
    gb_chain_body<R>(A, d, blockIdx.x);
}
