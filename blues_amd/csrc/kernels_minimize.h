// kernels_minimize.h -- the device-resident energy minimiser: FIRE (Bitzek et al., PRL 97, 170201) on the
// constraint manifold, fp64, one thread per constraint cluster as in the interpreter of kernels_integrate.h.
//
// One iteration = one ordinary force pass (slot 0 at the context's current lambdas) + the two kernels below:
//   k_fire_reduce_b   projects the force (the components along the constraints removed: RATTLE on w F at x_k) and writes this
//                     block's partials [fmax, G.G, v.v, G.v];
//   k_fire_step_b     every block adds the partials up in block order -- so every block derives the same decision --, tests
//                     convergence, adapts (dt, alpha), mixes and kicks the minimiser's own velocities, clips, drifts under SHAKE /
//                     RATTLE exactly as OP_R does, and writes back as integrate_body does (master positions, fixed-point image,
//                     list-validity test, prune flag, nan / constraint flags).  Block 0 publishes the next state into the OTHER half
//                     of the double-buffered state record: no block reads what another is writing.
// Sums: lanes by wave_sum, waves in wave order, blocks in index order -- a function of the topology only, so a member of a replica
// batch gets the bits of the same chain alone.  The kernels exist in the record form only (blockIdx.y selects the member's
// FireRec); a lone chain is a batch of one record.  A member that has converged, or has taken max_iter iterations and has had its
// force measured once more, is inert: neither kernel touches anything of it.
// The engine's own velocities are not used as scratch: vmin belongs to the minimiser.
#pragma once
#include "kernels_integrate.h"

struct FireState { double dt, alpha, fmax; int n_pos, iter, converged, done; };
struct FireRec {
    int active, max_iter, n_min, pad;
    double tol_f, dt_max, f_inc, f_dec, alpha0, f_alpha, max_step;
    double* vmin;        // [3][n] the minimiser's velocities, caller order
    double* part;        // [blocks][4] fmax, G.G, v.v, G.v
    FireState* state;    // [2]
    IntArgs in;
};

// max that keeps a NaN (fmax would drop it: a NaN force must not pass the convergence test)
__device__ __forceinline__ double fire_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ __forceinline__ double wave_max_nan(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fire_max(v, __shfl_xor(v, off, 64));
    return v;
}

// the thread's cluster at x_k with the minimiser's velocities (integrate_body's loads; an inactive thread gets an empty cluster)
__device__ __forceinline__ void fire_load(const IntArgs& A, const double* __restrict__ vmin, int cl, ClusterRec& R, Cluster& C) {
    if (cl < A.n_clusters) R = A.recs[cl];
    else { for (int a = 0; a < 4; a++) { R.atoms[a] = -1; R.alch[a] = -1; R.mobile[a] = 0; R.sorted[a] = 0; R.islot[a] = -1; R.w[a] = 0.0; } R.type = 0; R.nc = 0; R.na = 0; R.dist[0] = R.dist[1] = R.dist[2] = 0.0; }
    C.na = R.na; C.nc = R.nc; C.type = R.type;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = max(R.atoms[a], 0);
        C.id[a] = R.atoms[a]; C.al[a] = R.alch[a]; C.w[a] = R.w[a];
#pragma unroll
        for (int k = 0; k < 3; k++) { C.x[a][k] = A.x[k][i]; C.v[a][k] = vmin[(size_t)k * A.n + i]; }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) C.d2[c] = R.dist[c] * R.dist[c];
#pragma unroll
    for (int a = 0; a < 4; a++) if (a >= C.na) {
#pragma unroll
        for (int k = 0; k < 3; k++) { C.x[a][k] = 0.0; C.v[a][k] = 0.0; }
    }
}

// G = the slot-0 force with its components along the cluster's constraints removed: a = w F, RATTLE on a at x_k, G = a / w
__device__ __forceinline__ void fire_project(const IntArgs& A, Cluster& C, double G[4][3]) {
    double F[4][3], v0[4][3];
    load_force(A, C, 0, F);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int k = 0; k < 3; k++) { v0[a][k] = C.v[a][k]; C.v[a][k] = C.w[a] * F[a][k]; }
    rattle(C, A.tol, A);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int k = 0; k < 3; k++) { G[a][k] = (a < C.na && C.w[a] > 0.0) ? C.v[a][k] / C.w[a] : 0.0; C.v[a][k] = v0[a][k]; }
}

__global__ void __launch_bounds__(256) k_fire_reduce_b(const FireRec* __restrict__ recs, int parity) {
    const FireRec& rp = recs[blockIdx.y];
    if (!rp.active) return;
    if (rp.state[parity].done) return;
    IntArgs A = rp.in;
    const int tid = threadIdx.x, cl = blockIdx.x * blockDim.x + tid;
    __shared__ double s_red[4][4];
    ClusterRec R; Cluster C;
    fire_load(A, rp.vmin, cl, R, C);
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (cl < A.n_clusters) {
        double G[4][3];
        fire_project(A, C, G);
#pragma unroll
        for (int a = 0; a < 4; a++) if (a < C.na && C.w[a] > 0.0) {
#pragma unroll
            for (int k = 0; k < 3; k++) { q[0] = fire_max(q[0], fabs(G[a][k])); q[1] += G[a][k] * G[a][k]; q[2] += C.v[a][k] * C.v[a][k]; q[3] += G[a][k] * C.v[a][k]; }
        }
    }
    q[0] = wave_max_nan(q[0]);
#pragma unroll
    for (int j = 1; j < 4; j++) q[j] = wave_sum(q[j]);
    if ((tid & 63) == 0) { for (int j = 0; j < 4; j++) s_red[tid >> 6][j] = q[j]; }
    __syncthreads();
    if (tid < 4) {
        double t = s_red[0][tid];
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) t = tid == 0 ? fire_max(t, s_red[w][0]) : t + s_red[w][tid];
        rp.part[(size_t)blockIdx.x * 4 + tid] = t;
    }
}

__global__ void __launch_bounds__(256) k_fire_step_b(const FireRec* __restrict__ recs, int parity) {
    const FireRec& rp = recs[blockIdx.y];
    if (!rp.active) return;
    const int tid = threadIdx.x, cl = blockIdx.x * blockDim.x + tid;
    const FireState S = rp.state[parity];
    if (S.done) { if (blockIdx.x == 0 && tid == 0) rp.state[parity ^ 1] = S; return; }
    __shared__ double s_q[4];
    if (tid < 4) {   // the blocks' partials in block order: every block forms the same sums
        double t = rp.part[tid];
        for (int b = 1; b < (int)gridDim.x; b++) { const double p = rp.part[(size_t)b * 4 + tid]; t = tid == 0 ? fire_max(t, p) : t + p; }
        s_q[tid] = t;
    }
    __syncthreads();
    const double fmax = s_q[0], GG = s_q[1], VV = s_q[2], P = s_q[3];
    FireState N = S; N.fmax = fmax;
    bool stop = false, mix = false, zero = false;
    if (fmax <= rp.tol_f) { N.converged = 1; N.done = 1; stop = true; }   // the positions are those of the pass that met the test
    else if (S.iter >= rp.max_iter) { N.done = 1; stop = true; }          // out of iterations: this pass only measured fmax
    else {
        if (S.iter > 0) {   // adapt (nothing to adapt to before the first move: v = 0)
            if (P > 0.0) {
                N.n_pos = S.n_pos + 1;
                if (N.n_pos > rp.n_min) { N.dt = fmin(S.dt * rp.f_inc, rp.dt_max); N.alpha = S.alpha * rp.f_alpha; }
                mix = true;
            } else { N.n_pos = 0; N.dt = S.dt * rp.f_dec; N.alpha = rp.alpha0; zero = true; }
        }
        N.iter = S.iter + 1;
    }
    if (blockIdx.x == 0 && tid == 0) rp.state[parity ^ 1] = N;
    IntArgs A = rp.in;
    if (stop || cl >= A.n_clusters) return;

    ClusterRec R; Cluster C;
    fire_load(A, rp.vmin, cl, R, C);
    double G[4][3];
    fire_project(A, C, G);
    const double dt = N.dt, inv_dt = 1.0 / N.dt;
    const double ma = 1.0 - S.alpha, mb = mix ? S.alpha * sqrt(VV / GG) : 0.0;   // (the alpha from before this iteration's update)
#pragma unroll
    for (int a = 0; a < 4; a++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (mix) C.v[a][k] = ma * C.v[a][k] + mb * G[a][k];
            if (zero) C.v[a][k] = 0.0;
            C.v[a][k] += dt * G[a][k] * C.w[a];   // kick
        }
        // clip: no atom drifts further than max_step
        const double sp = sqrt(C.v[a][0] * C.v[a][0] + C.v[a][1] * C.v[a][1] + C.v[a][2] * C.v[a][2]) * dt;
        if (sp > rp.max_step) { const double sc = rp.max_step / sp; C.v[a][0] *= sc; C.v[a][1] *= sc; C.v[a][2] *= sc; }
    }
    bool ok = true;
    {   // drift: OP_R with hR = dt
        double xr[4][3], x1[4][3];
#pragma unroll
        for (int a = 0; a < 4; a++) for (int k = 0; k < 3; k++) {
            xr[a][k] = C.x[a][k];
            if (a < C.na) C.x[a][k] += dt * C.v[a][k];
            x1[a][k] = C.x[a][k];
        }
        ok &= shake(C, xr, A.tol, A);
#pragma unroll
        for (int a = 0; a < 4; a++) if (a < C.na) for (int k = 0; k < 3; k++) C.v[a][k] += (C.x[a][k] - x1[a][k]) * inv_dt;
        rattle(C, A.tol, A);
    }
    // ---- write back, refresh the fixed-point image, check list validity (integrate_body's, with the minimiser's velocities)
    bool need_rebuild = false, bad = false;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        if (a < C.na) {
            const int i = C.id[a];
            for (int k = 0; k < 3; k++) { rp.vmin[(size_t)k * A.n + i] = C.v[a][k]; bad |= !(C.x[a][k] == C.x[a][k]) || !(C.v[a][k] == C.v[a][k]); }
            double d2 = 0.0;
            for (int k = 0; k < 3; k++) { A.x[k][i] = C.x[a][k]; const double d = C.x[a][k] - A.xbuild[k][i]; d2 += d * d; }
            need_rebuild |= d2 > A.half_skin2;
            const int s = R.sorted[a];
            if (A.img_f) {
                unsigned u[3]; to_fixed32(C.x[a], A.box, u); A.img_f[s].x = u[0]; A.img_f[s].y = u[1]; A.img_f[s].z = u[2];
                if (A.pneed && R.islot[a] >= 0) {
                    float p2 = 0.0f;
                    for (int k = 0; k < 3; k++) { const float e = (float)(int)(u[k] - A.xprune[k][R.islot[a]]) * A.fscale[k]; p2 += e * e; }
                    if (p2 > A.prune_trig2) A.pneed[R.islot[a]] = 1;
                }
            }
            else { unsigned long long u[3]; to_fixed(C.x[a], A.box, u); A.img_d[s].x = u[0]; A.img_d[s].y = u[1]; A.img_d[s].z = u[2]; }
        }
    }
    if (need_rebuild) { A.flags->req_gen = A.flags->list_gen + 1; if (A.batch_req) *A.batch_req = 1; }
    if (bad) A.flags->nan_flag = 1;
    if (!ok) A.flags->constraint_fail = 1;
}

// the members' current state records in one buffer (one read-back per poll of a batch); a null pointer answers done = 1
__global__ void k_fire_gather_b(FireState* const* __restrict__ states, int R, int parity, FireState* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    FireState S; S.dt = 0.0; S.alpha = 0.0; S.fmax = 0.0; S.n_pos = 0; S.iter = 0; S.converged = 0; S.done = 1;
    if (states[r]) S = states[r][parity];
    out[r] = S;
}
