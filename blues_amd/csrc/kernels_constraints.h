// kernels_constraints.h -- general constraint clusters (AllBonds, HAngles): a connected component of the constraint graph that is
// neither a star nor a triangle of at most four atoms.  ONE WAVEFRONT owns one cluster.
//
// The cluster's positions, reference positions, velocities and inverse masses live in LDS as fp64 structure-of-arrays; lane l owns
// atoms l and l + 64 for everything that is per atom (kick, drift, noise, write-back).  SHAKE and RATTLE are Gauss-Seidel sweeps as in
// the oracle (oracle/blues_oracle.c: shake_gauss_seidel, constrain_velocities), made parallel by a colouring of the constraints
// that the host computes once: constraints of one colour share no atom, so the lanes of the wave update them side by side without
// atomics, and the colours follow one another in order.  The result is a function of the topology alone.
//
// The wave synchronises with itself only (a workgroup holds several clusters whose sweep counts differ: no block barrier in here).
// Included by kernels_integrate.h behind integrate_body, whose Program / IntArgs it interprets.
#pragma once

#define GEN_MAX_ATOMS 128     // per general cluster (two atoms per lane)
#define GEN_MAX_CONS 192
#define GEN_MAX_COLOURS 16
#define GEN_MAX_SWEEPS 500    // as the oracle
#define GEN_WAVES 4           // clusters per workgroup of 256 threads
#define GEN_LDS_DOUBLES (10 * GEN_MAX_ATOMS)

struct GenAtom { int atom, sorted, mobile, alch, islot, pad; double w; };   // caller index, image index, mobile index, alchemical index or -1, i-slot or -1, 1/mass
struct GenCons { int i, j; double d2; };                                    // local atom pair, distance^2; stored sorted by colour
struct GenCluster { int a0, na, c0, nc, ncol, pad; int col[GEN_MAX_COLOURS + 1]; };   // atoms [a0, a0 + na), constraints [c0, c0 + nc), colour q: [col[q], col[q + 1]) within them

// LDS of one wave: x[3], xref[3], v[3], w as [GEN_MAX_ATOMS] each; the constraints beside them
struct GenLds { double* s; int* ci; int* cj; double* d2; int* col; int ncol; };   // col: the colours' offsets (a copy of GenCluster::col)
#define GX(k, a) L.s[(k) * GEN_MAX_ATOMS + (a)]
#define GR(k, a) L.s[(3 + (k)) * GEN_MAX_ATOMS + (a)]
#define GV(k, a) L.s[(6 + (k)) * GEN_MAX_ATOMS + (a)]
#define GW(a) L.s[9 * GEN_MAX_ATOMS + (a)]

// the lanes of a wave run in lock step and its LDS operations complete in order: what is needed is that the compiler keeps the
// stores of one phase ahead of the loads of the next
__device__ __forceinline__ void gen_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }

#ifdef BLUES_GEN_SWEEPS
__device__ unsigned long long g_gen_sweeps[3];   // debug builds: SHAKE calls, sweeps in all, most sweeps of one call
#endif

// SHAKE: |d^2 - r^2| <= 2 tol d^2 skips a constraint; else delta = (d^2 - r^2) / (2 (r . r_ref)(w_i + w_j)) along r_ref.
// A sweep in which no lane updated ends the loop.
__device__ __forceinline__ bool shake_general(const GenLds& L, double tol, int lane) {
#pragma clang fp contract(off)   // (no fused multiply-add chosen by context: k_integrate_gen and k_integrate_gen_b must round alike)
    int it;
    for (it = 0; it < GEN_MAX_SWEEPS; it++) {
        bool upd = false;
        for (int q = 0; q < L.ncol; q++) {
            for (int c = L.col[q] + lane; c < L.col[q + 1]; c += 64) {
                const int i = L.ci[c], j = L.cj[c];
                const double d2 = L.d2[c];
                const double rp0 = GX(0, i) - GX(0, j), rp1 = GX(1, i) - GX(1, j), rp2 = GX(2, i) - GX(2, j);
                const double diff = d2 - (rp0 * rp0 + rp1 * rp1 + rp2 * rp2);
                if (fabs(diff) <= 2.0 * tol * d2) continue;
                upd = true;
                const double r0 = GR(0, i) - GR(0, j), r1 = GR(1, i) - GR(1, j), r2 = GR(2, i) - GR(2, j);
                const double wi = GW(i), wj = GW(j);
                const double delta = diff / (2.0 * (rp0 * r0 + rp1 * r1 + rp2 * r2) * (wi + wj));
                GX(0, i) += wi * delta * r0; GX(1, i) += wi * delta * r1; GX(2, i) += wi * delta * r2;
                GX(0, j) -= wj * delta * r0; GX(1, j) -= wj * delta * r1; GX(2, j) -= wj * delta * r2;
            }
            gen_sync();
        }
        if (__ballot(upd) == 0ull) break;
    }
#ifdef BLUES_GEN_SWEEPS
    if (lane == 0) { atomicAdd(&g_gen_sweeps[0], 1ull); atomicAdd(&g_gen_sweeps[1], (unsigned long long)(it + 1)); atomicMax(&g_gen_sweeps[2], (unsigned long long)(it + 1)); }
#endif
    return it < GEN_MAX_SWEEPS;
}

// RATTLE: delta = -(dv . r) / (r . r (w_i + w_j)), skipped when |delta| <= tol
__device__ __forceinline__ void rattle_general(const GenLds& L, double tol, int lane) {
#pragma clang fp contract(off)   // (no fused multiply-add chosen by context: k_integrate_gen and k_integrate_gen_b must round alike)
    for (int it = 0; it < GEN_MAX_SWEEPS; it++) {
        bool upd = false;
        for (int q = 0; q < L.ncol; q++) {
            for (int c = L.col[q] + lane; c < L.col[q + 1]; c += 64) {
                const int i = L.ci[c], j = L.cj[c];
                const double r0 = GX(0, i) - GX(0, j), r1 = GX(1, i) - GX(1, j), r2 = GX(2, i) - GX(2, j);
                const double u0 = GV(0, i) - GV(0, j), u1 = GV(1, i) - GV(1, j), u2 = GV(2, i) - GV(2, j);
                const double wi = GW(i), wj = GW(j);
                const double delta = -(u0 * r0 + u1 * r1 + u2 * r2) / ((r0 * r0 + r1 * r1 + r2 * r2) * (wi + wj));
                if (fabs(delta) <= tol) continue;
                upd = true;
                GV(0, i) += wi * delta * r0; GV(1, i) += wi * delta * r1; GV(2, i) += wi * delta * r2;
                GV(0, j) -= wj * delta * r0; GV(1, j) -= wj * delta * r1; GV(2, j) -= wj * delta * r2;
            }
            gen_sync();
        }
        if (__ballot(upd) == 0ull) break;
    }
}

__device__ __forceinline__ void gen_force(const IntArgs& A, const GenAtom& R, int slot, double F[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (R.alch >= 0) F[k] = A.ftot[(size_t)k * A.n + R.atom] + A.alch_self[(slot * 3 + k) * 64 + R.alch];
        else F[k] = A.ftot[(size_t)(slot * 3 + k) * A.n + R.atom];
    }
}
__device__ __forceinline__ void gen_noise(const IntArgs& A, const GenAtom& R, unsigned draw, double g[3]) {
    const unsigned nd = draw - A.noise_draw_base;
    if (nd < (unsigned)A.n_noise) { for (int k = 0; k < 3; k++) g[k] = A.noise[(size_t)(nd * 3 + k) * A.n_mobile + R.mobile]; }
    else gaussians3(A.seed, A.stream, draw, (unsigned)R.atom, g);
}

// The interpreter of integrate_body for the atoms of general cluster g: the same Program, the same per-atom arithmetic.  OP_H* and
// OP_END stay with block 0 of the small-cluster part of the launch.  cm_slot: this cluster's entry of cm_part (behind the small-cluster
// blocks'), summed in entry order by every OP_CM_APPLY.
__device__ __forceinline__ void integrate_general_body(IntArgs& A, const Program& prog, int g, GenLds& L) {
#pragma clang fp contract(off)   // (no fused multiply-add chosen by context: k_integrate_gen and k_integrate_gen_b must round alike)
    const int lane = threadIdx.x & 63;
    struct { int a0, na, c0, nc; } G;   // (wave-uniform: scalar registers)
    {
        const GenCluster* Gp = A.gen + g;
        G.a0 = __builtin_amdgcn_readfirstlane(Gp->a0); G.na = __builtin_amdgcn_readfirstlane(Gp->na);
        G.c0 = __builtin_amdgcn_readfirstlane(Gp->c0); G.nc = __builtin_amdgcn_readfirstlane(Gp->nc);
        L.ncol = __builtin_amdgcn_readfirstlane(Gp->ncol);
        if (lane <= GEN_MAX_COLOURS) L.col[lane] = Gp->col[lane];
    }
    GenAtom R[2]; bool on[2]; int la[2];
    double x1[2][3];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        la[u] = lane + 64 * u; on[u] = la[u] < G.na;
        if (on[u]) {
            R[u] = A.gen_atoms[G.a0 + la[u]];
            for (int k = 0; k < 3; k++) { GX(k, la[u]) = A.x[k][R[u].atom]; GR(k, la[u]) = GX(k, la[u]); GV(k, la[u]) = A.v[k][R[u].atom]; }
            GW(la[u]) = R[u].w;
        } else { R[u].atom = -1; R[u].sorted = 0; R[u].mobile = 0; R[u].alch = -1; R[u].islot = -1; R[u].w = 0.0; }
        for (int k = 0; k < 3; k++) x1[u][k] = 0.0;
    }
    for (int c = lane; c < G.nc; c += 64) { const GenCons K = A.gen_cons[G.c0 + c]; L.ci[c] = K.i; L.cj[c] = K.j; L.d2[c] = K.d2; }
    gen_sync();
    bool moved = false, ok = true;
    unsigned draw = A.draw_base;
    for (int op_i = 0; op_i < prog.n; op_i++) {
        const int op = prog.ops[op_i];
        switch (op) {
        case OP_V0: case OP_V1: case OP_V2: {
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) {
                double F[3]; gen_force(A, R[u], op - OP_V0, F);
                for (int k = 0; k < 3; k++) GV(k, la[u]) += A.hV * F[k] * R[u].w;
            }
            gen_sync();
            rattle_general(L, A.tol, lane);
        } break;
        case OP_R: case OP_A0: case OP_A1: case OP_A2: {
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) {
                if (op != OP_R) {
                    double F[3]; gen_force(A, R[u], op - OP_A0, F);
                    for (int k = 0; k < 3; k++) GV(k, la[u]) += A.hV * F[k] * R[u].w;
                }
                for (int k = 0; k < 3; k++) {
                    GR(k, la[u]) = GX(k, la[u]);
                    GX(k, la[u]) += A.hR * GV(k, la[u]);
                    x1[u][k] = GX(k, la[u]);
                }
            }
            gen_sync();
            ok &= shake_general(L, A.tol, lane);
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) for (int k = 0; k < 3; k++) GV(k, la[u]) += (GX(k, la[u]) - x1[u][k]) * A.inv_hR;
            gen_sync();
            if (op == OP_R) rattle_general(L, A.tol, lane);
            moved = true;
        } break;
        case OP_O: {
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) {
                double gs[3]; gen_noise(A, R[u], draw, gs);
                const double sd = sqrt(A.kT * R[u].w);
                for (int k = 0; k < 3; k++) GV(k, la[u]) = A.aO * GV(k, la[u]) + A.bO * sd * gs[k];
            }
            gen_sync();
            rattle_general(L, A.tol, lane);
            draw++;
        } break;
        case OP_L: {
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) {
                double F[3], gs[3];
                gen_force(A, R[u], 0, F);
                gen_noise(A, R[u], draw, gs);
                const double sd = sqrt(A.kT * R[u].w);
                for (int k = 0; k < 3; k++) {
                    GR(k, la[u]) = GX(k, la[u]);
                    GV(k, la[u]) = A.aL * GV(k, la[u]) + A.fsL * R[u].w * F[k] + A.nsL * sd * gs[k];
                    GX(k, la[u]) += A.dtL * GV(k, la[u]);
                }
            }
            gen_sync();
            ok &= shake_general(L, A.tol, lane);
            const double inv_dt = 1.0 / A.dtL;
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) for (int k = 0; k < 3; k++) GV(k, la[u]) = (GX(k, la[u]) - GR(k, la[u])) * inv_dt;
            gen_sync();
            moved = true;
            draw++;
        } break;
        case OP_RATTLE: rattle_general(L, A.tol, lane); break;
        case OP_PREP: {
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) for (int k = 0; k < 3; k++) GR(k, la[u]) = GX(k, la[u]);
            gen_sync();
            ok &= shake_general(L, A.tol, lane);
            rattle_general(L, A.tol, lane);
            moved = true;
        } break;
        case OP_CM_REDUCE: {   // (an engine with general clusters never takes the one-block form OP_CM_BLOCK: emit_cm)
            double p[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) for (int k = 0; k < 3; k++) p[k] += GV(k, la[u]) / R[u].w;
            for (int k = 0; k < 3; k++) { p[k] = wave_sum(p[k]); if (lane == k) A.cm_part[(size_t)(A.gen_block0 + g) * 3 + k] = p[k]; }
        } break;
        case OP_CM_APPLY: {
            double s = 0.0;
            if (lane < 3) { for (int b = 0; b < A.cm_nblocks; b++) s += A.cm_part[b * 3 + lane]; s = s / A.total_mass; }
            double cm[3];
            for (int k = 0; k < 3; k++) cm[k] = __shfl(s, k, 64);
#pragma unroll
            for (int u = 0; u < 2; u++) if (on[u]) for (int k = 0; k < 3; k++) GV(k, la[u]) -= cm[k];
            gen_sync();
        } break;
        default: break;   // OP_H01 / OP_H12 / OP_END: block 0 of the small-cluster part
        }
    }
    // ---- write back per atom, as at the end of integrate_body
    bool need_rebuild = false, bad = false;
#pragma unroll
    for (int u = 0; u < 2; u++) if (on[u]) {
        const int i = R[u].atom;
        double xa[3];
        for (int k = 0; k < 3; k++) { xa[k] = GX(k, la[u]); const double va = GV(k, la[u]); A.v[k][i] = va; bad |= !(xa[k] == xa[k]) || !(va == va); }
        if (moved) {
            double d2 = 0.0;
            for (int k = 0; k < 3; k++) { A.x[k][i] = xa[k]; const double d = xa[k] - A.xbuild[k][i]; d2 += d * d; }
            need_rebuild |= d2 > A.half_skin2;
            const int s = R[u].sorted;
            if (A.img_f) {
                unsigned uf[3]; to_fixed32(xa, A.box, uf); A.img_f[s].x = uf[0]; A.img_f[s].y = uf[1]; A.img_f[s].z = uf[2];
                if (A.pneed && R[u].islot >= 0) {
                    float p2 = 0.0f;
                    for (int k = 0; k < 3; k++) { const float e = (float)(int)(uf[k] - A.xprune[k][R[u].islot]) * A.fscale[k]; p2 += e * e; }
                    if (p2 > A.prune_trig2) A.pneed[R[u].islot] = 1;
                }
            }
            else { unsigned long long uf[3]; to_fixed(xa, A.box, uf); A.img_d[s].x = uf[0]; A.img_d[s].y = uf[1]; A.img_d[s].z = uf[2]; }
        }
    }
    if (need_rebuild) { A.flags->req_gen = A.flags->list_gen + 1; if (A.batch_req) *A.batch_req = 1; }
    if (bad) A.flags->nan_flag = 1;
    if (!ok && lane == 0) A.flags->constraint_fail = 1;
}

// One launch for a chain with general clusters: the small-cluster blocks of integrate_body first, the general clusters' workgroups at the
// tail of the grid (blockDim / 64 clusters each).  Engines without general clusters never launch this.
__device__ __forceinline__ void integrate_gen_dispatch(IntArgs& A, const Program& prog) {
    if ((int)blockIdx.x < A.gen_block0) { integrate_body(A, prog); return; }
    __shared__ double s_gen[GEN_WAVES][GEN_LDS_DOUBLES];
    __shared__ double s_d2[GEN_WAVES][GEN_MAX_CONS];
    __shared__ int s_ij[GEN_WAVES][2][GEN_MAX_CONS];
    __shared__ int s_col[GEN_WAVES][GEN_MAX_COLOURS + 1];
    const int wv = threadIdx.x >> 6;
    const int g = ((int)blockIdx.x - A.gen_block0) * (int)(blockDim.x >> 6) + wv;
    if (g >= A.n_gen) return;
    GenLds L; L.s = s_gen[wv]; L.ci = s_ij[wv][0]; L.cj = s_ij[wv][1]; L.d2 = s_d2[wv]; L.col = s_col[wv];
    integrate_general_body(A, prog, g, L);
}
__global__ void __launch_bounds__(256) k_integrate_gen(IntArgs A) { integrate_gen_dispatch(A, A.prog); }
#undef GX
#undef GR
#undef GV
#undef GW
