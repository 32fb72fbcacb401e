// kernels_pme.h -- smooth particle-mesh Ewald reciprocal space, the part of OpenMM's
// NonbondedForce under nonbondedMethod=PME (reference blues/simulation.py:219, examples/rotmove_cuda.yml:20) that the
// direct-space kernels leave out.  Same algorithm and conventions as the oracle (oracle/blues_oracle.c, reciprocal_space):
// order-`order` cardinal B-splines on the mesh points (floor(u) + k) mod K, E = 1/2 sum_m eterm(m) |Q^(m)|^2,
// forces from the spline derivatives [OpenMM 7.4.2 ReferencePME.cpp, recalled].
//
// MI355X shape.  The meshes of this path are small (18 x 27 x 36 for the 23k-atom box at ewaldErrorTolerance 0.005), and
// the sum is LINEAR in the charges: what the frozen atoms contribute -- their transformed charge mesh and their potential
// mesh -- is computed once per geometry (STATIC launch) and only the few hundred mobile charges are spread, transformed and
// gathered per step.  One workgroup per replica runs the whole pipeline (spread -> three axis transforms -> eterm ->
// three axis transforms back -> gather) with workgroup barriers between the phases: no launch boundaries, the mesh stays
// in the L2 of the replica's XCD.  Spreading accumulates in 64-bit fixed point (integer atomics commute: the result does
// not depend on the order in which the atoms arrive, so a batched replica stays bitwise identical to a lone one).
// The axis transforms are plain DFTs (K <= 256 per axis, any factorisation -- OpenMM's Reference platform takes the mesh
// sizes as ceil(...) gives them, 27 included).
#pragma once
#include "device_common.h"

#define PME_THREADS 1024
#define PME_MAX_ORDER 8
#define PME_FIX 1099511627776.0   // 2^40: fixed-point scale of the charge mesh
#define PME_FIX32 67108864.0f      // 2^26: the same in 32 bits (fast path: |mesh value| < 32 e, resolution 1.5e-8 e)

template <typename T> struct PmeArgs {
    int n, K[3], order, ng;
    int n_sel; const int* sel;         // atoms this launch spreads (and gathers): caller indices
    const double* x[3];                // master positions
    const double* qn;                  // [n] NonbondedForce charges (alchemical atoms: 0)
    const double* qn_full;             // [n] every atom's own charge: the NonbondedForce of the NON-alchemical System (want_energy bit 1: the mesh energy the MD / alch context would report)
    Box3 box;
    unsigned long long* acc;           // [ng] fixed-point charge mesh
    T* a_re; T* a_im; T* b_re; T* b_im;   // work meshes
    const T* eterm;                    // [ng], 0 at m = 0
    const T* tw_cos[3]; const T* tw_sin[3];   // cos / sin(2 pi t / K) per axis
    T* qf_re; T* qf_im; T* phi_f;      // static part: transform of the frozen charges' mesh, their potential mesh
    int have_static;                   // the static meshes hold something (there are frozen charges)
    double* frec;                      // [3][n] force on the selected atoms
    double* epart;                     // [1] mesh energy 1/2 sum eterm |Q^_f + Q^_m|^2 (dynamic launch, when want_energy)
    int want_energy;
    int* path;                         // [2] mobile launches served by the pruned in-LDS pipeline / by a general body (null: not counted -- the static launch)
};

template <typename T>
__device__ __forceinline__ void pme_splines(T dr, int order, T* w, T* dw) {
    w[order - 1] = (T)0; w[1] = dr; w[0] = (T)1 - dr;
    for (int l = 3; l < order; l++) {
        const T div = (T)1 / (T)(l - 1);
        w[l - 1] = div * dr * w[l - 2];
        for (int k = 1; k < l - 1; k++) w[l - k - 1] = div * ((dr + (T)k) * w[l - k - 2] + ((T)(l - k) - dr) * w[l - k - 1]);
        w[0] = div * ((T)1 - dr) * w[0];
    }
    dw[0] = -w[0];
    for (int k = 1; k < order; k++) dw[k] = w[k - 1] - w[k];
    const T div = (T)1 / (T)(order - 1);
    w[order - 1] = div * dr * w[order - 2];
    for (int k = 1; k < order - 1; k++) w[order - k - 1] = div * ((dr + (T)k) * w[order - k - 2] + ((T)(order - k) - dr) * w[order - k - 1]);
    w[0] = div * ((T)1 - dr) * w[0];
}

// the same with the order known at compile time: every loop unrolls, the arrays stay in registers (with a runtime order they are indexed
// dynamically and live in scratch memory -- measured: the per-step kernel spent most of its 280 us there)
template <typename T, int ORDER>
__device__ __forceinline__ void pme_splines_c(T dr, T* w, T* dw) {
    if (ORDER <= 0) { return; }
#pragma unroll
    for (int k = 0; k < (ORDER > 0 ? ORDER : 1); k++) w[k] = (T)0;
    w[1] = dr; w[0] = (T)1 - dr;
#pragma unroll
    for (int l = 3; l < ORDER; l++) {
        const T div = (T)1 / (T)(l - 1);
        w[l - 1] = div * dr * w[l - 2];
#pragma unroll
        for (int k = 1; k < l - 1; k++) w[l - k - 1] = div * ((dr + (T)k) * w[l - k - 2] + ((T)(l - k) - dr) * w[l - k - 1]);
        w[0] = div * ((T)1 - dr) * w[0];
    }
    dw[0] = -w[0];
#pragma unroll
    for (int k = 1; k < ORDER; k++) dw[k] = w[k - 1] - w[k];
    const T div = (T)1 / (T)(ORDER - 1);
    w[ORDER - 1] = div * dr * w[ORDER - 2];
#pragma unroll
    for (int k = 1; k < ORDER - 1; k++) w[ORDER - k - 1] = div * ((dr + (T)k) * w[ORDER - k - 2] + ((T)(ORDER - k) - dr) * w[ORDER - k - 1]);
    w[0] = div * ((T)1 - dr) * w[0];
}
// ORDER > 0: compile-time order; ORDER == 0: the runtime one
template <typename T, int ORDER>
__device__ __forceinline__ void pme_splines_any(T dr, int order, T* w, T* dw) {
    if constexpr (ORDER > 0) pme_splines_c<T, ORDER>(dr, w, dw); else pme_splines(dr, order, w, dw);
}

// mesh index and spline offset of atom i along axis d (fractional coordinate in fp64: the offset must not lose the position's digits)
template <typename T>
__device__ __forceinline__ void pme_locate(const PmeArgs<T>& P, int i, int d, int& ti, T& dr) {
    double fr = P.x[d][i] * P.box.invL[d]; fr -= floor(fr);
    const double u = fr * P.K[d];
    ti = (int)u; dr = (T)(u - ti);
    if (ti >= P.K[d]) ti -= P.K[d];
}

// one axis of the separable transform: out(m) = sum_k in(k) exp(sign 2 pi i m k / K) along axis ax, thread per output element
template <typename T>
__device__ __forceinline__ void pme_dft_axis(const PmeArgs<T>& P, const T* __restrict__ ire, const T* __restrict__ iim, T* __restrict__ ore, T* __restrict__ oim, int ax, T sign) {
    const int K = P.K[ax];
    const int st = ax == 0 ? P.K[1] * P.K[2] : (ax == 1 ? P.K[2] : 1);
    const T* tc = P.tw_cos[ax]; const T* ts = P.tw_sin[ax];
    for (int g = threadIdx.x; g < P.ng; g += PME_THREADS) {
        const int m = (g / st) % K, base = g - m * st;
        T sr = (T)0, si = (T)0;
        int t = 0;
        for (int k = 0; k < K; k++) {
            const T c = tc[t], s = sign * ts[t];
            const T a = ire[base + k * st], b = iim[base + k * st];
            sr = fma(a, c, fma(-b, s, sr)); si = fma(a, s, fma(b, c, si));
            t += m; if (t >= K) t -= K;
        }
        ore[g] = sr; oim[g] = si;
    }
}

template <typename T, bool STATIC, int ORDER = 0>
__device__ __forceinline__ void pme_body(const PmeArgs<T>& P) {
    const int tid = threadIdx.x, order = ORDER > 0 ? ORDER : P.order;
    const int K0 = P.K[0], K1 = P.K[1], K2 = P.K[2];
    if (!STATIC && tid == 0 && P.path) P.path[1]++;   // (a general body served this mobile launch: the host's choice, or one of k_pme_fast's two exits)
    // ---- charge mesh in fixed point
    for (int g = tid; g < P.ng; g += PME_THREADS) P.acc[g] = 0ull;
    __syncthreads();
    {   // work item = (atom, a, b): the order^2 (x, y) offsets of an atom, each spreading its column along z
        const int per = order * order;
        for (long w = tid; w < (long)P.n_sel * per; w += PME_THREADS) {
            const int s = (int)(w / per), ab = (int)(w - (long)s * per), a = ab / order, b = ab - a * order;
            const int i = P.sel[s];
            const double q = P.qn[i];
            if (q == 0.0) continue;
            int t0, t1, t2; T d0, d1, d2;
            pme_locate(P, i, 0, t0, d0); pme_locate(P, i, 1, t1, d1); pme_locate(P, i, 2, t2, d2);
            T w0[PME_MAX_ORDER], w1[PME_MAX_ORDER], w2[PME_MAX_ORDER], dw[PME_MAX_ORDER];
            pme_splines_any<T, ORDER>(d0, order, w0, dw); pme_splines_any<T, ORDER>(d1, order, w1, dw); pme_splines_any<T, ORDER>(d2, order, w2, dw);
            // (constant indices only into the spline arrays: a runtime index would put them in scratch memory)
            T wa = (T)0, wb = (T)0;
#pragma unroll
            for (int k = 0; k < PME_MAX_ORDER; k++) { if (k == a) wa = w0[k]; if (k == b) wb = w1[k]; }
            int ix = t0 + a; if (ix >= K0) ix -= K0;
            int iy = t1 + b; if (iy >= K1) iy -= K1;
            const double qab = q * (double)wa * (double)wb;
#pragma unroll
            for (int c = 0; c < PME_MAX_ORDER; c++) {
                if (c >= order) break;
                int iz = t2 + c; if (iz >= K2) iz -= K2;
                const long long v = llrint(qab * (double)w2[c] * PME_FIX);
                atomicAdd(&P.acc[((size_t)ix * K1 + iy) * K2 + iz], (unsigned long long)v);
            }
        }
    }
    __syncthreads();
    for (int g = tid; g < P.ng; g += PME_THREADS) { P.a_re[g] = (T)((double)(long long)P.acc[g] * (1.0 / PME_FIX)); P.a_im[g] = (T)0; }
    __syncthreads();
    // ---- forward transform z, y, x
    pme_dft_axis(P, P.a_re, P.a_im, P.b_re, P.b_im, 2, (T)-1); __syncthreads();
    pme_dft_axis(P, P.b_re, P.b_im, P.a_re, P.a_im, 1, (T)-1); __syncthreads();
    pme_dft_axis(P, P.a_re, P.a_im, P.b_re, P.b_im, 0, (T)-1); __syncthreads();
    // ---- energy (with the frozen charges' transform), static copy, multiplication by eterm
    if (!STATIC && P.want_energy) {
        double e = 0.0;
        for (int g = tid; g < P.ng; g += PME_THREADS) {
            const double re = (double)P.b_re[g] + (P.have_static ? (double)P.qf_re[g] : 0.0), im = (double)P.b_im[g] + (P.have_static ? (double)P.qf_im[g] : 0.0);
            e += (double)P.eterm[g] * (re * re + im * im);
        }
        __shared__ double s_e[PME_THREADS / 64];
        e = wave_sum(e);
        if ((tid & 63) == 0) s_e[tid >> 6] = e;
        __syncthreads();
        if (tid == 0) { double t = 0.0; for (int w = 0; w < PME_THREADS / 64; w++) t += s_e[w]; P.epart[0] = 0.5 * t; }
    }
    for (int g = tid; g < P.ng; g += PME_THREADS) {
        if (STATIC) { P.qf_re[g] = P.b_re[g]; P.qf_im[g] = P.b_im[g]; }
        const T et = P.eterm[g];
        P.b_re[g] *= et; P.b_im[g] *= et;
    }
    __syncthreads();
    // ---- backward transform x, y, z (the potential mesh is the real part)
    pme_dft_axis(P, P.b_re, P.b_im, P.a_re, P.a_im, 0, (T)1); __syncthreads();
    pme_dft_axis(P, P.a_re, P.a_im, P.b_re, P.b_im, 1, (T)1); __syncthreads();
    pme_dft_axis(P, P.b_re, P.b_im, P.a_re, P.a_im, 2, (T)1); __syncthreads();
    if (STATIC) {
        for (int g = tid; g < P.ng; g += PME_THREADS) P.phi_f[g] = P.a_re[g];
        return;
    }
    // ---- gather: the force on every selected atom from the potential of all charges (mobile: just computed; frozen: static)
    for (int s = tid; s < P.n_sel; s += PME_THREADS) {
        const int i = P.sel[s];
        const double q = P.qn[i];
        double fx = 0.0, fy = 0.0, fz = 0.0;
        if (q != 0.0) {
            int t0, t1, t2; T d0, d1, d2;
            pme_locate(P, i, 0, t0, d0); pme_locate(P, i, 1, t1, d1); pme_locate(P, i, 2, t2, d2);
            T w0[PME_MAX_ORDER], w1[PME_MAX_ORDER], w2[PME_MAX_ORDER], e0[PME_MAX_ORDER], e1[PME_MAX_ORDER], e2[PME_MAX_ORDER];
            pme_splines_any<T, ORDER>(d0, order, w0, e0); pme_splines_any<T, ORDER>(d1, order, w1, e1); pme_splines_any<T, ORDER>(d2, order, w2, e2);
#pragma unroll
            for (int a = 0; a < PME_MAX_ORDER; a++) {
                if (a >= order) break;
                int ix = t0 + a; if (ix >= K0) ix -= K0;
#pragma unroll
                for (int b = 0; b < PME_MAX_ORDER; b++) {
                    if (b >= order) break;
                    int iy = t1 + b; if (iy >= K1) iy -= K1;
                    T sx = (T)0, sz = (T)0;   // sum_c w2 phi and sum_c dw2 phi of this column
#pragma unroll
                    for (int c = 0; c < PME_MAX_ORDER; c++) {
                        if (c >= order) break;
                        int iz = t2 + c; if (iz >= K2) iz -= K2;
                        const size_t g = ((size_t)ix * K1 + iy) * K2 + iz;
                        const T phi = P.a_re[g] + (P.have_static ? P.phi_f[g] : (T)0);
                        sx = fma(w2[c], phi, sx); sz = fma(e2[c], phi, sz);
                    }
                    fx += (double)(e0[a] * w1[b] * sx); fy += (double)(w0[a] * e1[b] * sx); fz += (double)(w0[a] * w1[b] * sz);
                }
            }
            fx *= -q * K0 * P.box.invL[0]; fy *= -q * K1 * P.box.invL[1]; fz *= -q * K2 * P.box.invL[2];
        }
        P.frec[i] = fx; P.frec[(size_t)P.n + i] = fy; P.frec[2 * (size_t)P.n + i] = fz;
    }
}


// out-of-line copy of the general path for the fast kernel's fallbacks (kept out of its register allocation)
__device__ __noinline__ void pme_body_general_f(const PmeArgs<float>& P) { pme_body<float, false, 5>(P); }

// ---- fast path of the per-step (mobile) launch in mixed precision: everything between the spread and the gather lives in LDS, and
// the transforms are PRUNED.  The mobile charges occupy a small block of the mesh (their stencils span Lx x Ly x Lz points, ~13^3 of
// 18 x 27 x 36 for the benchmark), the potential is only needed on that block, and the charge mesh is real (half spectrum along z):
//   forward   z: (Lx, Ly) lines,  Lz inputs -> Hz = K2/2+1 outputs      y: (Lx, Hz) lines, Ly inputs -> K1      x: (K1, Hz) lines, Lx -> K0
//   backward  x: K0 inputs -> Lx outputs     y: K1 -> Ly     z: Hz (Hermitian weights 1,2,..,2[,1]) -> Lz real outputs
// = 0.5 M complex multiply-adds instead of 2.8 M for the full complex transforms.  One thread per (line, output); the inputs of a
// line are read from LDS at the same address by all the lanes that share the line (broadcast).
#define PME_LDS_Y 9280             // complex entries of buffer Y: the half spectrum K0 x K1 x (K2/2+1) (18 x 27 x 19 = 9,234 for the benchmark mesh)
#define PME_LDS_X 7424             // complex entries of buffer X: the block's lines along one full axis, Lx x K1 x (K2/2+1)
#define PME_LDS_ATOMS 768          // mobile atoms whose mesh position is cached in LDS (32 B each); more: the general path

struct PmeRegion { int s[3], L[3]; };   // block of the mesh: points (s + a) mod K, a < L, per axis

// (the buffers are addressed as offsets into ONE __shared__ array: through plain pointers the compiler cannot tell LDS from global memory
// and emits flat loads, each iteration then waiting out a full memory latency -- measured 296 us per launch instead of ~20)
extern __shared__ __align__(16) float2 pme_lds[];

template <int DIR>   // DIR = -1 forward, +1 backward
__device__ __forceinline__ void pme_pass(int in, int out, int nlines, int line_div,
                                         int in_s0, int in_s1, int in_st, int n_in, int k0, int out_s0, int out_s1, int out_st, int n_out, int m0,
                                         int K, int tw) {
    // line l = (l / line_div, l % line_div); element j of its input sits at in_s0*(l/line_div) + in_s1*(l%line_div) + in_st*j and stands for
    // mesh index (k0 + j) mod K; output o stands for index (m0 + o) mod K.  A thread keeps ONE output index o and walks the lines
    // (its phase exp(DIR 2 pi i m k0 / K) and the per-input rotation are loop invariants; no integer division per work item).  The phase
    // is advanced by a complex rotation per input (4 FMAs, no table look-up; <= 36 steps in fp32 on the benchmark mesh: ~2e-6 of a few % of
    // the force; up to K = 256 steps on the longest axis the engine accepts -- measured on 6 x 8 x 256 and 256 x 6 x 8, the force is
    // within 7.3e-7 of the oracle's, three times the general kernel's residual and 14 times inside the 1e-5 bound: profiles/pme_shapes/README.md).
    const int o = threadIdx.x % n_out, lg = threadIdx.x / n_out, nlg = PME_THREADS / n_out;
    if (lg >= nlg) return;   // (the threads past the last whole group of n_out sit this pass out)
    int m = m0 + o; if (m >= K) m -= K;
    int k = k0; if (k >= K) k -= K;
    const float2 p0 = pme_lds[tw + (m * k) % K], rot = pme_lds[tw + m];
    const float c0 = p0.x, s0 = DIR < 0 ? -p0.y : p0.y, rc = rot.x, rs = DIR < 0 ? -rot.y : rot.y;
    int l0 = lg / line_div, l1 = lg - l0 * line_div;
    const int d0 = nlg / line_div, d1 = nlg - d0 * line_div;
    for (int l = lg; l < nlines; l += nlg) {
        int src = in + in_s0 * l0 + in_s1 * l1;
        float c = c0, sn = s0, sr = 0.0f, si = 0.0f;
#pragma unroll 4
        for (int j = 0; j < n_in; j++) {
            const float2 v = pme_lds[src];
            src += in_st;
            sr = fmaf(v.x, c, fmaf(-v.y, sn, sr)); si = fmaf(v.x, sn, fmaf(v.y, c, si));
            const float c2 = fmaf(c, rc, -sn * rs); sn = fmaf(c, rs, sn * rc); c = c2;
        }
        pme_lds[out + out_s0 * l0 + out_s1 * l1 + out_st * o] = make_float2(sr, si);
        l0 += d0; l1 += d1; if (l1 >= line_div) { l1 -= line_div; l0++; }
    }
}

template <int ORDER>
__device__ __forceinline__ void pme_fast_body(const PmeArgs<float>& P) {
    const int X = 0, Y = PME_LDS_X, tw0 = PME_LDS_X + PME_LDS_Y, tw1 = tw0 + P.K[0], tw2 = tw1 + P.K[1];   // offsets into pme_lds
    const int AT = (tw2 + P.K[2] + 1) & ~1;   // per-atom cache: int4 {t0, t1, t2, selected index} + float4 {dr0, dr1, dr2, q}, 4 float2 slots per atom
    int4* at_i = reinterpret_cast<int4*>(pme_lds + AT); float4* at_f = reinterpret_cast<float4*>(pme_lds + AT + 2 * PME_LDS_ATOMS);
    int* acc = reinterpret_cast<int*>(pme_lds + Y);   // the block's charge mesh in 32-bit fixed point (before any transform): integer adds commute
    __shared__ int s_lo[3], s_hi[3], s_ref[3], s_first;
    __shared__ double s_e[PME_THREADS / 64];
    const int tid = threadIdx.x, order = ORDER > 0 ? ORDER : P.order;
    const int K0 = P.K[0], K1 = P.K[1], K2 = P.K[2], Hz = K2 / 2 + 1;
    NB_STAMP(blockIdx.x == 0 && tid == 0, 9);
    // ---- twiddles and the block that holds the mobile charges' stencils (relative to the first charged atom, through the periodic wrap)
    for (int k = tid; k < K0; k += PME_THREADS) pme_lds[tw0 + k] = make_float2(P.tw_cos[0][k], P.tw_sin[0][k]);
    for (int k = tid; k < K1; k += PME_THREADS) pme_lds[tw1 + k] = make_float2(P.tw_cos[1][k], P.tw_sin[1][k]);
    for (int k = tid; k < K2; k += PME_THREADS) pme_lds[tw2 + k] = make_float2(P.tw_cos[2][k], P.tw_sin[2][k]);
    if (tid < 3) { s_lo[tid] = 1 << 30; s_hi[tid] = -(1 << 30); }
    if (tid == 0) s_first = 1 << 30;
    if (P.n_sel > PME_LDS_ATOMS) { pme_body_general_f(P); return; }   // (block-uniform) too many mobile atoms to cache: the general path
    __syncthreads();
    // every selected atom's mesh position, once: three dependent global loads per atom (index -> charge, coordinates), all atoms in parallel
    // -- the spread and the gather below then run out of LDS (reading them again per work item cost ~250 us of pure memory latency)
    for (int s = tid; s < P.n_sel; s += PME_THREADS) {
        const int i = P.sel[s];
        int4 ti; float4 fr; ti.w = i;
        pme_locate(P, i, 0, ti.x, fr.x); pme_locate(P, i, 1, ti.y, fr.y); pme_locate(P, i, 2, ti.z, fr.z);
        fr.w = (float)P.qn[i];
        at_i[s] = ti; at_f[s] = fr;
        int mine = fr.w != 0.0f ? s : (1 << 30);
        for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
        if ((tid & 63) == 0 && mine < (1 << 30)) atomicMin(&s_first, mine);
    }
    __syncthreads();
    if (tid < 3) s_ref[tid] = s_first < P.n_sel ? (tid == 0 ? at_i[s_first].x : (tid == 1 ? at_i[s_first].y : at_i[s_first].z)) : 0;
    __syncthreads();
    {   // extent of the charged atoms' mesh indices around the reference: reduced in the wave first (64 lanes on one LDS address serialise)
        int lo[3] = {1 << 30, 1 << 30, 1 << 30}, hi[3] = {-(1 << 30), -(1 << 30), -(1 << 30)};
        for (int s = tid; s < P.n_sel; s += PME_THREADS) {
            if (at_f[s].w == 0.0f) continue;
            const int4 ti = at_i[s];
            const int tt[3] = {ti.x, ti.y, ti.z};
#pragma unroll
            for (int d = 0; d < 3; d++) {
                int del = tt[d] - s_ref[d]; const int K = P.K[d];
                if (2 * del >= K) del -= K; else if (2 * del < -K) del += K;
                lo[d] = min(lo[d], del); hi[d] = max(hi[d], del);
            }
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
            for (int o = 32; o > 0; o >>= 1) { lo[d] = min(lo[d], __shfl_xor(lo[d], o, 64)); hi[d] = max(hi[d], __shfl_xor(hi[d], o, 64)); }
            if ((tid & 63) == 0) { atomicMin(&s_lo[d], lo[d]); atomicMax(&s_hi[d], hi[d]); }
        }
    }
    __syncthreads();
    NB_STAMP(blockIdx.x == 0 && tid == 0, 10);
    PmeRegion R;
    bool fits = true;
    for (int d = 0; d < 3; d++) {
        const int K = P.K[d];
        if (s_hi[d] < s_lo[d]) { R.s[d] = 0; R.L[d] = 1; continue; }   // no charged atom: an empty block
        R.L[d] = s_hi[d] - s_lo[d] + order;
        int st = (s_ref[d] + s_lo[d]) % K; if (st < 0) st += K;
        R.s[d] = st;
        if (R.L[d] >= K) { R.L[d] = K; R.s[d] = 0; }
    }
    const int Lx = R.L[0], Ly = R.L[1], Lz = R.L[2];
    fits = Lx * Ly * Lz <= PME_LDS_X && Lx * K1 * Hz <= PME_LDS_X && Lx * Ly * Hz <= PME_LDS_Y && K0 * K1 * Hz <= PME_LDS_Y
           && P.n_sel * 16 <= PME_LDS_X && (Lx * Ly * Lz + 4 + P.n_sel * 48 + 1) / 2 <= PME_LDS_Y;   // (room for the atoms' spline weights beside the meshes)
    if (!fits) { pme_body_general_f(P); return; }   // (block-uniform) a spread-out mobile set: the general path
    if (tid == 0 && P.path) P.path[0]++;   // (read by blues_get_global "pme_fast_launches": the pruned pipeline served this launch)
    // ---- spread into the block (LDS, 64-bit integer adds: order-independent)
    for (int g = tid; g < Lx * Ly * Lz; g += PME_THREADS) acc[g] = 0;
    __syncthreads();
    // the atoms' spline weights once, into the (still unused) X buffer: 32 floats per atom = w_x[8] w_y[8] w_z[8] + padding; then a thread per
    // (atom, x offset, y offset) column.  (A thread per column that recomputed the splines, or a thread per atom with all order^3 points, both
    // cost several times more: redundant spline arithmetic / a 125-point unrolled body spilling registers.)
    float* wts = reinterpret_cast<float*>(pme_lds + X);
    for (int s = tid; s < P.n_sel; s += PME_THREADS) {
        const float4 fr = at_f[s];
        float w0[ORDER > 0 ? ORDER : PME_MAX_ORDER], w1[ORDER > 0 ? ORDER : PME_MAX_ORDER], w2[ORDER > 0 ? ORDER : PME_MAX_ORDER], dw[ORDER > 0 ? ORDER : PME_MAX_ORDER];
        pme_splines_any<float, ORDER>(fr.x, order, w0, dw); pme_splines_any<float, ORDER>(fr.y, order, w1, dw); pme_splines_any<float, ORDER>(fr.z, order, w2, dw);
#pragma unroll
        for (int k = 0; k < (ORDER > 0 ? ORDER : PME_MAX_ORDER); k++) { wts[s * 32 + k] = w0[k]; wts[s * 32 + 8 + k] = w1[k]; wts[s * 32 + 16 + k] = w2[k]; }
    }
    __syncthreads();
    {
        const int per = order * order;
        for (int w = tid; w < P.n_sel * per; w += PME_THREADS) {
            const int s = w / per, ab = w - s * per, a = ab / order, b = ab - a * order;
            const float4 fr = at_f[s]; const int4 ti = at_i[s];
            if (fr.w == 0.0f) continue;
            int ax = ti.x + a - R.s[0]; if (ax < 0) ax += K0; if (ax >= K0) ax -= K0;
            int ay = ti.y + b - R.s[1]; if (ay < 0) ay += K1; if (ay >= K1) ay -= K1;
            int az0 = ti.z - R.s[2]; if (az0 < 0) az0 += K2;
            const float qab = fr.w * PME_FIX32 * wts[s * 32 + a] * wts[s * 32 + 8 + b];
            const int row = (ax * Ly + ay) * Lz;
#pragma unroll
            for (int c = 0; c < (ORDER > 0 ? ORDER : PME_MAX_ORDER); c++) {
                if (c >= order) break;
                int az = az0 + c; if (az >= K2) az -= K2;
                atomicAdd(&acc[row + az], __float2int_rn(qab * wts[s * 32 + 16 + c]));
            }
        }
    }
    __syncthreads();
    NB_STAMP(blockIdx.x == 0 && tid == 0, 11);
    // block -> X as complex [Lx][Ly][Lz]   (Y is being read as acc: convert through registers, then write X)
    for (int g = tid; g < Lx * Ly * Lz; g += PME_THREADS) pme_lds[X + g] = make_float2((float)acc[g] * (1.0f / PME_FIX32), 0.0f);
    __syncthreads();
    NB_STAMP(blockIdx.x == 0 && tid == 0, 12);
    // ---- forward: z (X[Lx][Ly][Lz] -> Y[Lx][Ly][Hz]), y (-> X[Lx][K1][Hz]), x (-> Y[K0][K1][Hz])
    pme_pass<-1>(X, Y, Lx * Ly, Ly, Ly * Lz, Lz, 1, Lz, R.s[2], Ly * Hz, Hz, 1, Hz, 0, K2, tw2); __syncthreads();
    pme_pass<-1>(Y, X, Lx * Hz, Hz, Ly * Hz, 1, Hz, Ly, R.s[1], K1 * Hz, 1, Hz, K1, 0, K1, tw1); __syncthreads();
    pme_pass<-1>(X, Y, K1 * Hz, Hz, Hz, 1, K1 * Hz, Lx, R.s[0], Hz, 1, K1 * Hz, K0, 0, K0, tw0); __syncthreads();
    NB_STAMP(blockIdx.x == 0 && tid == 0, 13);
    // ---- energy with the frozen charges' transform (half spectrum: interior k_z count twice), then eterm
    if (P.want_energy) {
        double e = 0.0;
        for (int g = tid; g < K0 * K1 * Hz; g += PME_THREADS) {
            const int kz = g % Hz, xy = g / Hz; const size_t gf = (size_t)xy * K2 + kz;
            const double re = (double)pme_lds[Y + g].x + (P.have_static ? (double)P.qf_re[gf] : 0.0), im = (double)pme_lds[Y + g].y + (P.have_static ? (double)P.qf_im[gf] : 0.0);
            e += ((kz == 0 || 2 * kz == K2) ? 1.0 : 2.0) * (double)P.eterm[gf] * (re * re + im * im);
        }
        e = wave_sum(e);
        if ((tid & 63) == 0) s_e[tid >> 6] = e;
        __syncthreads();
        if (tid == 0) { double t = 0.0; for (int w = 0; w < PME_THREADS / 64; w++) t += s_e[w]; P.epart[0] = 0.5 * t; }
    }
    for (int g = tid; g < K0 * K1 * Hz; g += PME_THREADS) {
        const int kz = g % Hz, xy = g / Hz;
        // (eterm and the weight of the half spectrum's missing conjugates, 1 for k_z = 0 and K2/2, 2 otherwise: the last backward pass then is a plain sum)
        const float et = P.eterm[(size_t)xy * K2 + kz] * ((kz == 0 || 2 * kz == K2) ? 1.0f : 2.0f);
        pme_lds[Y + g].x *= et; pme_lds[Y + g].y *= et;
    }
    __syncthreads();
    NB_STAMP(blockIdx.x == 0 && tid == 0, 14);
    // ---- backward: x (Y[K0][K1][Hz] -> X[Lx][K1][Hz]), y (-> Y[Lx][Ly][Hz]), z (Hermitian, -> X[Lx][Ly][Lz], real part)
    pme_pass<1>(Y, X, K1 * Hz, Hz, Hz, 1, K1 * Hz, K0, 0, Hz, 1, K1 * Hz, Lx, R.s[0], K0, tw0); __syncthreads();
    pme_pass<1>(X, Y, Lx * Hz, Hz, K1 * Hz, 1, Hz, K1, 0, Ly * Hz, 1, Hz, Ly, R.s[1], K1, tw1); __syncthreads();
    pme_pass<1>(Y, X, Lx * Ly, Ly, Ly * Hz, Hz, 1, Hz, 0, Ly * Lz, Lz, 1, Lz, R.s[2], K2, tw2); __syncthreads();
    NB_STAMP(blockIdx.x == 0 && tid == 0, 15);
    // the frozen charges' potential on the block, once (Y is free now): the gather then reads LDS only
    float* phf = reinterpret_cast<float*>(pme_lds + Y);
    if (P.have_static) for (int g = tid; g < Lx * Ly * Lz; g += PME_THREADS) {
        const int az = g % Lz, ay = (g / Lz) % Ly, ax = g / (Lz * Ly);
        int ix = R.s[0] + ax; if (ix >= K0) ix -= K0;
        int iy = R.s[1] + ay; if (iy >= K1) iy -= K1;
        int iz = R.s[2] + az; if (iz >= K2) iz -= K2;
        phf[g] = P.phi_f[((size_t)ix * K1 + iy) * K2 + iz];
    }
    __syncthreads();
    // ---- gather: weights and their derivatives once per atom (into the free part of Y, behind the frozen potential's block), then 32 lanes per
    // atom, lane = (x offset, y offset) column, summed over the atom's lanes in a fixed order
    float* wg = phf + ((Lx * Ly * Lz + 3) & ~3);   // 48 floats per atom: w_x w_y w_z e_x e_y e_z (8 each)
    for (int s = tid; s < P.n_sel; s += PME_THREADS) {
        const float4 fr = at_f[s];
        float w0[ORDER > 0 ? ORDER : PME_MAX_ORDER], w1[ORDER > 0 ? ORDER : PME_MAX_ORDER], w2[ORDER > 0 ? ORDER : PME_MAX_ORDER];
        float e0[ORDER > 0 ? ORDER : PME_MAX_ORDER], e1[ORDER > 0 ? ORDER : PME_MAX_ORDER], e2[ORDER > 0 ? ORDER : PME_MAX_ORDER];
        pme_splines_any<float, ORDER>(fr.x, order, w0, e0); pme_splines_any<float, ORDER>(fr.y, order, w1, e1); pme_splines_any<float, ORDER>(fr.z, order, w2, e2);
#pragma unroll
        for (int k = 0; k < (ORDER > 0 ? ORDER : PME_MAX_ORDER); k++) {
            wg[s * 48 + k] = w0[k]; wg[s * 48 + 8 + k] = w1[k]; wg[s * 48 + 16 + k] = w2[k];
            wg[s * 48 + 24 + k] = e0[k]; wg[s * 48 + 32 + k] = e1[k]; wg[s * 48 + 40 + k] = e2[k];
        }
    }
    __syncthreads();
    for (int s0 = (tid >> 5); s0 < P.n_sel; s0 += PME_THREADS / 32) {
        const int ab = tid & 31;
        const float4 fr = at_f[s0]; const int4 ti = at_i[s0];
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        if (fr.w != 0.0f && ab < order * order) {
            const int a = ab / order, b = ab - a * order;
            const float* wv = wg + s0 * 48;
            int ax = ti.x + a - R.s[0]; if (ax < 0) ax += K0; if (ax >= K0) ax -= K0;
            int ay = ti.y + b - R.s[1]; if (ay < 0) ay += K1; if (ay >= K1) ay -= K1;
            int az0 = ti.z - R.s[2]; if (az0 < 0) az0 += K2;
            const int row = (ax * Ly + ay) * Lz;
            float sx = 0.0f, sz = 0.0f;
#pragma unroll
            for (int c = 0; c < (ORDER > 0 ? ORDER : PME_MAX_ORDER); c++) {
                if (c >= order) break;
                int az = az0 + c; if (az >= K2) az -= K2;
                const float phi = pme_lds[X + row + az].x + (P.have_static ? phf[row + az] : 0.0f);
                sx = fmaf(wv[16 + c], phi, sx); sz = fmaf(wv[40 + c], phi, sz);
            }
            fx = wv[24 + a] * wv[8 + b] * sx; fy = wv[a] * wv[32 + b] * sx; fz = wv[a] * wv[8 + b] * sz;
        }
        double gx = (double)fx, gy = (double)fy, gz = (double)fz;   // fixed-order sum over the 32 lanes of the atom
        for (int o = 16; o > 0; o >>= 1) { gx += __shfl_xor(gx, o, 64); gy += __shfl_xor(gy, o, 64); gz += __shfl_xor(gz, o, 64); }
        if ((tid & 31) == 0) {
            const int i = ti.w; const double q = (double)fr.w;
            P.frec[i] = -q * K0 * P.box.invL[0] * gx; P.frec[(size_t)P.n + i] = -q * K1 * P.box.invL[1] * gy; P.frec[2 * (size_t)P.n + i] = -q * K2 * P.box.invL[2] * gz;
        }
    }
    NB_STAMP(blockIdx.x == 0 && tid == 0, 16);
}

__global__ void __launch_bounds__(PME_THREADS) k_pme_fast(PmeArgs<float> P) { pme_fast_body<5>(P); }   // (the engine accepts order 5 only: OpenMM's)
#define PME_FAST_LDS(K0, K1, K2) ((size_t)(PME_LDS_X + PME_LDS_Y) * 8 + (size_t)((K0) + (K1) + (K2) + 2) * 8 + (size_t)PME_LDS_ATOMS * 32)

template <typename T, bool STATIC>
__global__ void __launch_bounds__(PME_THREADS) k_pme(PmeArgs<T> P) { pme_body<T, STATIC, 5>(P); }

// ---- exact PME treatment of the alchemical charges: q~_i = lambda_electrostatics^a_i q_i in reciprocal space, the self
// term, the neutralising background and the erf corrections of excluded pairs, so each of them is E0 + le E1 + le^2 E2 at fixed positions.
// The launches above keep what they do for the environment class (alchemical atoms carry qn = 0 there: frec, the env-env mesh energy, the
// static meshes of the frozen environment).  This kernel adds the second class.  The mobile environment charges are spread into the REAL
// part of the charge mesh and the alchemical charges (mobile or frozen) into the IMAGINARY part: the reciprocal-space kernel is real in
// real space (eterm(m) = eterm(-m)), the transforms are linear, so after the back transform the real part is the potential of the
// mobile environment and the imaginary part the potential of the alchemical atoms -- two classes for the transforms of one.
//   E1 = sum_a q_a phi_env(a) (+ background cross term + erf corrections of alchemical-environment exclusions)
//   E2 = 1/2 sum_a q_a phi_alch(a) (+ alchemical self term and background + erf corrections of alchemical-alchemical exclusions)
//   force per lambda slot: q_j le grad phi_alch on a mobile environment atom (q_j grad phi_env is frec), le q_a (grad phi_env + le grad phi_alch)
//   on an alchemical atom.
// The non-excluded alchemical x alchemical direct-space pairs, which the alchemical kernel scales with le, take le^2 here through a
// pair correction C_aa (le^2 - le) (kind 2 below).  Sums run in fixed orders (64-bit fixed-point spread, lanes by wave_sum, waves in
// wave order, an atom's pair entries in list order): a batch member equals the lone chain bit for bit.  One machine code serves both
// (record form, blockIdx.x = member), as for kernels_gb.h.
#define PMEX_NE 6   // energy partials, laid out like a GB block's for k_finalize: [1] E1, [2] E2 (+ C_aa), [4] -C_aa, [5] C_aa (read by the host only)
template <typename T> struct PmeExArgs {
    PmeArgs<T> P;                  // the engine's per-step arguments: meshes, tables, box, positions, sel = mobile atoms, qn
    int active;                    // (batched form) 0: the member sits this launch out
    int n_alch; const int* alch;   // alchemical atoms, caller indices
    const double* q;               // [n] every atom's own charge
    const int* alch_local;         // [n] >= 0: alchemical
    const int* mobile_index;       // [n] >= 0: mobile
    unsigned long long* acc2;      // [ng] fixed-point mesh of the alchemical class
    int n_pair; const int* pair_i; const int* pair_j; const double* pair_qq; const int* pair_kind;   // unique pairs (energies)
    int n_row; const int* row_atom; const int* row_start; const int* ent_j; const double* ent_qq; const int* ent_kind;   // per mobile atom (forces)
    double alpha, rc2;
    double c1, c2;                 // box constants: background cross term; alchemical self term + background
    double* fex;                   // [9][n] force per slot (k_finalize's fgb)
    double* epart;                 // [PMEX_NE]
    int* path;                     // [2] launches served by the pruned in-LDS pipeline / by the general one
};
struct PmeExDyn { double le[3]; };

// potential and gradient sums of the two classes at atom i: out[0..2] = sum of (dw w w, w dw w, w w dw) phi, out[3] = sum w w w phi
template <typename T>
__device__ __forceinline__ void pmex_gather(const PmeArgs<T>& P, int i, bool want_env, double env[4], double alc[4]) {
    constexpr int ORDER = 5;
    const int K0 = P.K[0], K1 = P.K[1], K2 = P.K[2];
    int t0, t1, t2; T d0, d1, d2;
    pme_locate(P, i, 0, t0, d0); pme_locate(P, i, 1, t1, d1); pme_locate(P, i, 2, t2, d2);
    T w0[ORDER], w1[ORDER], w2[ORDER], e0[ORDER], e1[ORDER], e2[ORDER];
    pme_splines_c<T, ORDER>(d0, w0, e0); pme_splines_c<T, ORDER>(d1, w1, e1); pme_splines_c<T, ORDER>(d2, w2, e2);
    for (int k = 0; k < 4; k++) { env[k] = 0.0; alc[k] = 0.0; }
#pragma unroll
    for (int a = 0; a < ORDER; a++) {
        int ix = t0 + a; if (ix >= K0) ix -= K0;
#pragma unroll
        for (int b = 0; b < ORDER; b++) {
            int iy = t1 + b; if (iy >= K1) iy -= K1;
            T sxe = (T)0, sze = (T)0, sxa = (T)0, sza = (T)0;
#pragma unroll
            for (int c = 0; c < ORDER; c++) {
                int iz = t2 + c; if (iz >= K2) iz -= K2;
                const size_t g = ((size_t)ix * K1 + iy) * K2 + iz;
                const T pa = P.a_im[g];
                sxa = fma(w2[c], pa, sxa); sza = fma(e2[c], pa, sza);
                if (want_env) {
                    const T pe = P.a_re[g] + (P.have_static ? P.phi_f[g] : (T)0);
                    sxe = fma(w2[c], pe, sxe); sze = fma(e2[c], pe, sze);
                }
            }
            alc[0] += (double)(e0[a] * w1[b] * sxa); alc[1] += (double)(w0[a] * e1[b] * sxa); alc[2] += (double)(w0[a] * w1[b] * sza); alc[3] += (double)(w0[a] * w1[b] * sxa);
            env[0] += (double)(e0[a] * w1[b] * sxe); env[1] += (double)(w0[a] * e1[b] * sxe); env[2] += (double)(w0[a] * w1[b] * sze); env[3] += (double)(w0[a] * w1[b] * sxe);
        }
    }
}

// one correction pair: kind 0 / 1 = erf correction of an excluded pair of class 1 / 2, kind 2 = direct-space alchemical x alchemical pair
// (class 2 minus the class 1 the alchemical kernel gives it).  d = x_i - x_j; returns the energy, *fs = force scale (force on i = fs d)
template <typename T>
__device__ __forceinline__ double pmex_pair(const PmeExArgs<T>& X, int i, int j, double qq, int kind, double d[3], double* fs) {
    const PmeArgs<T>& P = X.P;
    for (int k = 0; k < 3; k++) d[k] = min_image_d(P.x[k][i] - P.x[k][j], P.box.L[k], P.box.invL[k]);
    const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (kind == 2) {
        if (!(r2 < X.rc2)) { *fs = 0.0; return 0.0; }
        return coulomb_d(r2, qq, X.alpha, true, fs);
    }
    const double pre = ONE_4PI_EPS0 * qq, al = X.alpha, r = sqrt(r2), er = erf(al * r);
    const double dEdr = -pre * (TWO_OVER_SQRT_PI * al * exp(-al * al * r2) / r - er / r2);
    *fs = -dEdr / r;
    return -pre * er / r;
}


// ---- the alchemical class on the pruned in-LDS pipeline (mixed precision; the layout, the passes and the fixed-point spread of k_pme_fast).
// Two runs of the pipeline in one workgroup, each with its own small block in and its own block out:
//   1. the mobile environment charges, spread over the block U of all charged mobile and alchemical atoms, transformed back onto the block A
//      of the alchemical atoms only: phi_env there (plus the frozen environment's static potential mesh, read at the <= 64 atoms' stencils);
//   2. the alchemical charges, spread over A, transformed back onto U: phi_alch at every mobile atom and at the alchemical atoms.
// (k_pme_fast, whose body the direct-space treatment runs, keeps its mobile potential in LDS and is left as it is; run 1 repeats its
// spread and forward passes in LDS and prunes the backward passes to A.)  Entries of the atom cache: the mobile atoms (P.sel), then the
// alchemical atoms (mobile or frozen).  Per-atom sums over a stencil are taken by 32 lanes in a fixed shuffle order, the energies over
// the alchemical atoms by wave 0: a batch member equals the lone chain bit for bit.  Returns false (block-uniform, nothing written) when the
// blocks or the atoms do not fit the buffers: the caller then takes the general path.
#define PMEX_LDS_ATOMS (PME_LDS_ATOMS - 128)   // cache entries; the last 128 slots (4 KiB) hold the alchemical atoms' gathered sums
#define PMEX_MAX_ALCH 64

// one run: the block Ri of the charge mesh (32-bit fixed point at Y) -> the potential on the block Ro (real part of X[Lox][Loy][Loz])
__device__ __forceinline__ void pmex_fast_pipeline(const PmeArgs<float>& P, const PmeRegion& Ri, const PmeRegion& Ro) {
    const int X = 0, Y = PME_LDS_X, tw0 = PME_LDS_X + PME_LDS_Y, tw1 = tw0 + P.K[0], tw2 = tw1 + P.K[1];
    const int tid = threadIdx.x, K0 = P.K[0], K1 = P.K[1], K2 = P.K[2], Hz = K2 / 2 + 1;
    const int Lix = Ri.L[0], Liy = Ri.L[1], Liz = Ri.L[2], Lox = Ro.L[0], Loy = Ro.L[1], Loz = Ro.L[2];
    const int* acc = reinterpret_cast<const int*>(pme_lds + Y);
    for (int g = tid; g < Lix * Liy * Liz; g += PME_THREADS) pme_lds[X + g] = make_float2((float)acc[g] * (1.0f / PME_FIX32), 0.0f);
    __syncthreads();
    pme_pass<-1>(X, Y, Lix * Liy, Liy, Liy * Liz, Liz, 1, Liz, Ri.s[2], Liy * Hz, Hz, 1, Hz, 0, K2, tw2); __syncthreads();
    pme_pass<-1>(Y, X, Lix * Hz, Hz, Liy * Hz, 1, Hz, Liy, Ri.s[1], K1 * Hz, 1, Hz, K1, 0, K1, tw1); __syncthreads();
    pme_pass<-1>(X, Y, K1 * Hz, Hz, Hz, 1, K1 * Hz, Lix, Ri.s[0], Hz, 1, K1 * Hz, K0, 0, K0, tw0); __syncthreads();
    for (int g = tid; g < K0 * K1 * Hz; g += PME_THREADS) {   // eterm and the weight of the half spectrum's missing conjugates
        const int kz = g % Hz, xy = g / Hz;
        const float et = P.eterm[(size_t)xy * K2 + kz] * ((kz == 0 || 2 * kz == K2) ? 1.0f : 2.0f);
        pme_lds[Y + g].x *= et; pme_lds[Y + g].y *= et;
    }
    __syncthreads();
    pme_pass<1>(Y, X, K1 * Hz, Hz, Hz, 1, K1 * Hz, K0, 0, Hz, 1, K1 * Hz, Lox, Ro.s[0], K0, tw0); __syncthreads();
    pme_pass<1>(X, Y, Lox * Hz, Hz, K1 * Hz, 1, Hz, K1, 0, Loy * Hz, 1, Hz, Loy, Ro.s[1], K1, tw1); __syncthreads();
    pme_pass<1>(Y, X, Lox * Loy, Loy, Loy * Hz, Hz, 1, Hz, 0, Loy * Loz, Loz, 1, Loz, Ro.s[2], K2, tw2); __syncthreads();
}

__device__ __forceinline__ bool pmex_fast_mesh(const PmeExArgs<float>& Xa, const PmeExDyn& dyn, double& e1, double& e2) {
    constexpr int ORDER = 5;
    const PmeArgs<float>& P = Xa.P;
    const int X = 0, Y = PME_LDS_X, tw0 = PME_LDS_X + PME_LDS_Y, tw1 = tw0 + P.K[0], tw2 = tw1 + P.K[1];
    const int AT = (tw2 + P.K[2] + 1) & ~1;
    int4* at_i = reinterpret_cast<int4*>(pme_lds + AT); float4* at_f = reinterpret_cast<float4*>(pme_lds + AT + 2 * PMEX_LDS_ATOMS);
    double* s_pot = reinterpret_cast<double*>(pme_lds + AT + 4 * PMEX_LDS_ATOMS);   // [PMEX_MAX_ALCH][8]: sums of (dw w w, w dw w, w w dw, w w w) phi_env, then of phi_alch
    int* acc = reinterpret_cast<int*>(pme_lds + Y);
    __shared__ int s_lo[2][3], s_hi[2][3], s_ref[3], s_first;
    const int tid = threadIdx.x, n = P.n, n_sel = P.n_sel, ne = P.n_sel + Xa.n_alch;
    const int K0 = P.K[0], K1 = P.K[1], K2 = P.K[2], Hz = K2 / 2 + 1;
    const int ALCH = 1 << 30;   // flag in the cached atom index
    if (ne > PMEX_LDS_ATOMS || Xa.n_alch > PMEX_MAX_ALCH || K0 * K1 * Hz > PME_LDS_Y || ne * 16 > PME_LDS_X || (ne * 48 + 1) / 2 > PME_LDS_Y) return false;
    for (int k = tid; k < K0; k += PME_THREADS) pme_lds[tw0 + k] = make_float2(P.tw_cos[0][k], P.tw_sin[0][k]);
    for (int k = tid; k < K1; k += PME_THREADS) pme_lds[tw1 + k] = make_float2(P.tw_cos[1][k], P.tw_sin[1][k]);
    for (int k = tid; k < K2; k += PME_THREADS) pme_lds[tw2 + k] = make_float2(P.tw_cos[2][k], P.tw_sin[2][k]);
    if (tid < 6) { s_lo[tid / 3][tid % 3] = 1 << 30; s_hi[tid / 3][tid % 3] = -(1 << 30); }
    if (tid == 0) s_first = 1 << 30;
    for (int k = tid; k < PMEX_MAX_ALCH * 8; k += PME_THREADS) s_pot[k] = 0.0;
    __syncthreads();
    for (int s = tid; s < ne; s += PME_THREADS) {
        const int i = s < n_sel ? P.sel[s] : Xa.alch[s - n_sel];
        int4 ti; float4 fr;
        pme_locate(P, i, 0, ti.x, fr.x); pme_locate(P, i, 1, ti.y, fr.y); pme_locate(P, i, 2, ti.z, fr.z);
        fr.w = (float)Xa.q[i]; ti.w = i | (Xa.alch_local[i] >= 0 ? ALCH : 0);
        at_i[s] = ti; at_f[s] = fr;
        int mine = fr.w != 0.0f ? s : (1 << 30);
        for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
        if ((tid & 63) == 0 && mine < (1 << 30)) atomicMin(&s_first, mine);
    }
    __syncthreads();
    if (tid < 3) s_ref[tid] = s_first < ne ? (tid == 0 ? at_i[s_first].x : (tid == 1 ? at_i[s_first].y : at_i[s_first].z)) : 0;
    __syncthreads();
    {   // extents around the reference: [0] every charged entry (U), [1] the charged alchemical entries (A)
        int lo[2][3], hi[2][3];
        for (int r = 0; r < 2; r++) for (int d = 0; d < 3; d++) { lo[r][d] = 1 << 30; hi[r][d] = -(1 << 30); }
        for (int s = tid; s < ne; s += PME_THREADS) {
            if (at_f[s].w == 0.0f) continue;
            const int4 ti = at_i[s];
            const int tt[3] = {ti.x, ti.y, ti.z};
#pragma unroll
            for (int d = 0; d < 3; d++) {
                int del = tt[d] - s_ref[d]; const int K = P.K[d];
                if (2 * del >= K) del -= K; else if (2 * del < -K) del += K;
                lo[0][d] = min(lo[0][d], del); hi[0][d] = max(hi[0][d], del);
                if (s >= n_sel) { lo[1][d] = min(lo[1][d], del); hi[1][d] = max(hi[1][d], del); }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int d = 0; d < 3; d++) {
                for (int o = 32; o > 0; o >>= 1) { lo[r][d] = min(lo[r][d], __shfl_xor(lo[r][d], o, 64)); hi[r][d] = max(hi[r][d], __shfl_xor(hi[r][d], o, 64)); }
                if ((tid & 63) == 0) { atomicMin(&s_lo[r][d], lo[r][d]); atomicMax(&s_hi[r][d], hi[r][d]); }
            }
    }
    __syncthreads();
    PmeRegion R[2];   // [0] U, [1] A (inside U)
    for (int r = 0; r < 2; r++) for (int d = 0; d < 3; d++) {
        const int K = P.K[d];
        if (s_hi[r][d] < s_lo[r][d]) { R[r].s[d] = 0; R[r].L[d] = 1; continue; }   // no charged atom: an empty block
        R[r].L[d] = s_hi[r][d] - s_lo[r][d] + ORDER;
        int st = (s_ref[d] + s_lo[r][d]) % K; if (st < 0) st += K;
        R[r].s[d] = st;
        if (R[r].L[d] >= K) { R[r].L[d] = K; R[r].s[d] = 0; }
    }
    {
        const int Lx = R[0].L[0], Ly = R[0].L[1], Lz = R[0].L[2];   // (A's extents are at most U's)
        if (!(Lx * Ly * Lz <= PME_LDS_X && Lx * K1 * Hz <= PME_LDS_X && Lx * Ly * Hz <= PME_LDS_Y)) return false;   // (block-uniform) a spread-out mobile set
    }
    float* wts = reinterpret_cast<float*>(pme_lds + X);   // spread: 32 floats per entry, w_x[8] w_y[8] w_z[8]
    float* wg = reinterpret_cast<float*>(pme_lds + Y);    // gather: 48 floats per entry, w_x w_y w_z e_x e_y e_z (8 each)
    // spread of one class (cls 0: the mobile environment, cls 1: the alchemical atoms) into the block Ri
    auto spread = [&](int cls, const PmeRegion& Ri) {
        const int sb = cls ? n_sel : 0, se = cls ? ne : n_sel, Ly = Ri.L[1], Lz = Ri.L[2];
        for (int g = tid; g < Ri.L[0] * Ly * Lz; g += PME_THREADS) acc[g] = 0;
        for (int s = sb + tid; s < se; s += PME_THREADS) {
            const float4 fr = at_f[s];
            float w0[ORDER], w1[ORDER], w2[ORDER], dw[ORDER];
            pme_splines_c<float, ORDER>(fr.x, w0, dw); pme_splines_c<float, ORDER>(fr.y, w1, dw); pme_splines_c<float, ORDER>(fr.z, w2, dw);
#pragma unroll
            for (int k = 0; k < ORDER; k++) { wts[s * 32 + k] = w0[k]; wts[s * 32 + 8 + k] = w1[k]; wts[s * 32 + 16 + k] = w2[k]; }
        }
        __syncthreads();
        const int per = ORDER * ORDER;
        for (int w = tid; w < (se - sb) * per; w += PME_THREADS) {
            const int s = sb + w / per, ab = w % per, a = ab / ORDER, b = ab - a * ORDER;
            const float4 fr = at_f[s]; const int4 ti = at_i[s];
            if (fr.w == 0.0f || (!cls && (ti.w & ALCH))) continue;   // (a mobile alchemical atom is spread with its class)
            int ax = ti.x + a - Ri.s[0]; if (ax < 0) ax += K0; if (ax >= K0) ax -= K0;
            int ay = ti.y + b - Ri.s[1]; if (ay < 0) ay += K1; if (ay >= K1) ay -= K1;
            int az0 = ti.z - Ri.s[2]; if (az0 < 0) az0 += K2;
            const float qab = fr.w * PME_FIX32 * wts[s * 32 + a] * wts[s * 32 + 8 + b];
            const int row = (ax * Ly + ay) * Lz;
#pragma unroll
            for (int c = 0; c < ORDER; c++) {
                int az = az0 + c; if (az >= K2) az -= K2;
                atomicAdd(&acc[row + az], __float2int_rn(qab * wts[s * 32 + 16 + c]));
            }
        }
        __syncthreads();
    };
    // the sums of one potential over the stencils of the entries [sb, se), from the block Ro in X (with_static: plus the frozen environment's mesh)
    auto gather = [&](int sb, int se, const PmeRegion& Ro, bool with_static, auto&& sink) {
        const int Ly = Ro.L[1], Lz = Ro.L[2];
        for (int s = sb + tid; s < se; s += PME_THREADS) {
            const float4 fr = at_f[s];
            float w0[ORDER], w1[ORDER], w2[ORDER], e0[ORDER], e1_[ORDER], e2_[ORDER];
            pme_splines_c<float, ORDER>(fr.x, w0, e0); pme_splines_c<float, ORDER>(fr.y, w1, e1_); pme_splines_c<float, ORDER>(fr.z, w2, e2_);
            float* wv = wg + (s - sb) * 48;
#pragma unroll
            for (int k = 0; k < ORDER; k++) { wv[k] = w0[k]; wv[8 + k] = w1[k]; wv[16 + k] = w2[k]; wv[24 + k] = e0[k]; wv[32 + k] = e1_[k]; wv[40 + k] = e2_[k]; }
        }
        __syncthreads();
        for (int s0 = sb + (tid >> 5); s0 < se; s0 += PME_THREADS / 32) {
            const int ab = tid & 31;
            const float4 fr = at_f[s0]; const int4 ti = at_i[s0];
            float fx = 0.0f, fy = 0.0f, fz = 0.0f, fv = 0.0f;
            if (fr.w != 0.0f && ab < ORDER * ORDER) {
                const int a = ab / ORDER, b = ab - a * ORDER;
                const float* wv = wg + (s0 - sb) * 48;
                int ix = ti.x + a; if (ix >= K0) ix -= K0;
                int iy = ti.y + b; if (iy >= K1) iy -= K1;
                int ax = ix - Ro.s[0]; if (ax < 0) ax += K0;
                int ay = iy - Ro.s[1]; if (ay < 0) ay += K1;
                int az0 = ti.z - Ro.s[2]; if (az0 < 0) az0 += K2;
                const int row = (ax * Ly + ay) * Lz;
                float sx = 0.0f, sz = 0.0f;
#pragma unroll
                for (int c = 0; c < ORDER; c++) {
                    int az = az0 + c; if (az >= K2) az -= K2;
                    float phi = pme_lds[X + row + az].x;
                    if (with_static) { int iz = ti.z + c; if (iz >= K2) iz -= K2; phi += P.phi_f[((size_t)ix * K1 + iy) * K2 + iz]; }
                    sx = fmaf(wv[16 + c], phi, sx); sz = fmaf(wv[40 + c], phi, sz);
                }
                fx = wv[24 + a] * wv[8 + b] * sx; fy = wv[a] * wv[32 + b] * sx; fz = wv[a] * wv[8 + b] * sz; fv = wv[a] * wv[8 + b] * sx;
            }
            double g[4] = {(double)fx, (double)fy, (double)fz, (double)fv};   // fixed-order sum over the 32 lanes of the atom
            for (int o = 16; o > 0; o >>= 1) { g[0] += __shfl_xor(g[0], o, 64); g[1] += __shfl_xor(g[1], o, 64); g[2] += __shfl_xor(g[2], o, 64); g[3] += __shfl_xor(g[3], o, 64); }
            if ((tid & 31) == 0) sink(s0, ti.w & ~ALCH, (ti.w & ALCH) != 0, g);
        }
        __syncthreads();
    };
    // ---- 1. the mobile environment: U in, A out; phi_env (mobile + frozen) at the alchemical atoms
    spread(0, R[0]);
    pmex_fast_pipeline(P, R[0], R[1]);
    gather(n_sel, ne, R[1], P.have_static != 0, [&](int, int i, bool, const double* g) {
        double* sp = s_pot + 8 * Xa.alch_local[i];
        sp[0] = g[0]; sp[1] = g[1]; sp[2] = g[2]; sp[3] = g[3];
    });
    // ---- 2. the alchemical atoms: A in, U out; phi_alch at every entry, the per-slot forces of the mobile atoms
    spread(1, R[1]);
    pmex_fast_pipeline(P, R[1], R[0]);
    gather(0, ne, R[0], false, [&](int s, int i, bool alch, const double* g) {
        if (s >= n_sel) { double* sp = s_pot + 8 * Xa.alch_local[i] + 4; sp[0] = g[0]; sp[1] = g[1]; sp[2] = g[2]; sp[3] = g[3]; return; }
        const double q = Xa.q[i];
        const double sc[3] = {-q * K0 * P.box.invL[0], -q * K1 * P.box.invL[1], -q * K2 * P.box.invL[2]};
        const double* sp = s_pot + 8 * (alch ? Xa.alch_local[i] : 0);
        double fe[3], fa[3];
        for (int k = 0; k < 3; k++) { fe[k] = alch ? sc[k] * sp[k] : 0.0; fa[k] = sc[k] * g[k]; }
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            const double le = dyn.le[sl];
            for (int k = 0; k < 3; k++) Xa.fex[(size_t)(sl * 3 + k) * n + i] = alch ? le * (fe[k] + le * fa[k]) : le * fa[k];
        }
    });
    // ---- energies of the alchemical charges in the two potentials: lane a of wave 0 holds atom a's
    e1 = 0.0; e2 = 0.0;
    if (tid < Xa.n_alch) {
        const int i = Xa.alch[tid];
        const double q = Xa.q[i];
        const double* sp = s_pot + 8 * Xa.alch_local[i];
        e1 = q * sp[3]; e2 = 0.5 * q * sp[7];
    }
    return true;
}

// FAST: the mesh part was served by pmex_fast_mesh (its forces are in fex, e1 / e2 hold the alchemical atoms' mesh energies per lane)
template <typename T, bool FAST = false>
__device__ __forceinline__ void pmex_body(const PmeExArgs<T>& X, const PmeExDyn& dyn, double e1_in = 0.0, double e2_in = 0.0) {
    constexpr int ORDER = 5;
    const PmeArgs<T>& P = X.P;
    const int tid = threadIdx.x;
    const int K0 = P.K[0], K1 = P.K[1], K2 = P.K[2], n = P.n;
    __shared__ double s_e[PME_THREADS / 64][3];
    // ---- the two charge meshes in fixed point
    if constexpr (!FAST) {
    for (int g = tid; g < P.ng; g += PME_THREADS) { P.acc[g] = 0ull; X.acc2[g] = 0ull; }
    __syncthreads();
    {
        const int per = ORDER * ORDER;
        const long total = (long)(P.n_sel + X.n_alch) * per;
        for (long w = tid; w < total; w += PME_THREADS) {
            const int s = (int)(w / per), ab = (int)(w - (long)s * per), a = ab / ORDER, b = ab - a * ORDER;
            const bool alch = s >= P.n_sel;
            const int i = alch ? X.alch[s - P.n_sel] : P.sel[s];
            const double q = alch ? X.q[i] : P.qn[i];
            if (q == 0.0) continue;
            unsigned long long* acc = alch ? X.acc2 : P.acc;
            int t0, t1, t2; T d0, d1, d2;
            pme_locate(P, i, 0, t0, d0); pme_locate(P, i, 1, t1, d1); pme_locate(P, i, 2, t2, d2);
            T w0[ORDER], w1[ORDER], w2[ORDER], dw[ORDER];
            pme_splines_c<T, ORDER>(d0, w0, dw); pme_splines_c<T, ORDER>(d1, w1, dw); pme_splines_c<T, ORDER>(d2, w2, dw);
            T wa = (T)0, wb = (T)0;
#pragma unroll
            for (int k = 0; k < ORDER; k++) { if (k == a) wa = w0[k]; if (k == b) wb = w1[k]; }
            int ix = t0 + a; if (ix >= K0) ix -= K0;
            int iy = t1 + b; if (iy >= K1) iy -= K1;
            const double qab = q * (double)wa * (double)wb;
#pragma unroll
            for (int c = 0; c < ORDER; c++) {
                int iz = t2 + c; if (iz >= K2) iz -= K2;
                const long long v = llrint(qab * (double)w2[c] * PME_FIX);
                atomicAdd(&acc[((size_t)ix * K1 + iy) * K2 + iz], (unsigned long long)v);
            }
        }
    }
    __syncthreads();
    for (int g = tid; g < P.ng; g += PME_THREADS) {
        P.a_re[g] = (T)((double)(long long)P.acc[g] * (1.0 / PME_FIX));
        P.a_im[g] = (T)((double)(long long)X.acc2[g] * (1.0 / PME_FIX));
    }
    __syncthreads();
    // ---- forward z, y, x; eterm; backward x, y, z: real part = potential of the mobile environment, imaginary part = of the alchemical atoms
    pme_dft_axis(P, P.a_re, P.a_im, P.b_re, P.b_im, 2, (T)-1); __syncthreads();
    pme_dft_axis(P, P.b_re, P.b_im, P.a_re, P.a_im, 1, (T)-1); __syncthreads();
    pme_dft_axis(P, P.a_re, P.a_im, P.b_re, P.b_im, 0, (T)-1); __syncthreads();
    for (int g = tid; g < P.ng; g += PME_THREADS) { const T et = P.eterm[g]; P.b_re[g] *= et; P.b_im[g] *= et; }
    __syncthreads();
    pme_dft_axis(P, P.b_re, P.b_im, P.a_re, P.a_im, 0, (T)1); __syncthreads();
    pme_dft_axis(P, P.a_re, P.a_im, P.b_re, P.b_im, 1, (T)1); __syncthreads();
    pme_dft_axis(P, P.b_re, P.b_im, P.a_re, P.a_im, 2, (T)1); __syncthreads();
    }
    // ---- energies: the alchemical atoms' charges in the two potentials (wave 0; at most 64 alchemical atoms), then the correction pairs
    double e1 = e1_in, e2 = e2_in, caa = 0.0;
    if (tid < X.n_alch) {
        const int i = X.alch[tid];
        const double q = X.q[i];
        if (!FAST && q != 0.0) {
            double env[4], alc[4];
            pmex_gather(P, i, true, env, alc);
            e1 = q * env[3]; e2 = 0.5 * q * alc[3];
        }
        if (X.mobile_index[i] < 0) for (int k = 0; k < 9; k++) X.fex[(size_t)k * n + i] = 0.0;   // (a frozen alchemical atom: k_finalize reads its row)
    }
    for (int p = tid; p < X.n_pair; p += PME_THREADS) {
        double d[3], fs;
        const int kind = X.pair_kind[p];
        const double e = pmex_pair(X, X.pair_i[p], X.pair_j[p], X.pair_qq[p], kind, d, &fs);
        if (kind == 0) e1 += e; else if (kind == 1) e2 += e; else caa += e;
    }
    e1 = wave_sum(e1); e2 = wave_sum(e2); caa = wave_sum(caa);
    if ((tid & 63) == 0) { s_e[tid >> 6][0] = e1; s_e[tid >> 6][1] = e2; s_e[tid >> 6][2] = caa; }
    // ---- forces of the mesh on the mobile atoms, per slot
    if constexpr (!FAST) for (int s = tid; s < P.n_sel; s += PME_THREADS) {
        const int i = P.sel[s];
        const bool alch = X.alch_local[i] >= 0;
        const double q = X.q[i];
        double fe[3] = {0.0, 0.0, 0.0}, fa[3] = {0.0, 0.0, 0.0};
        if (q != 0.0) {
            double env[4], alc[4];
            pmex_gather(P, i, alch, env, alc);
            const double sc[3] = {-q * K0 * P.box.invL[0], -q * K1 * P.box.invL[1], -q * K2 * P.box.invL[2]};
            for (int k = 0; k < 3; k++) { fe[k] = sc[k] * env[k]; fa[k] = sc[k] * alc[k]; }
        }
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            const double le = dyn.le[sl];
            for (int k = 0; k < 3; k++) X.fex[(size_t)(sl * 3 + k) * n + i] = alch ? le * (fe[k] + le * fa[k]) : le * fa[k];
        }
    }
    __syncthreads();
    // ---- forces of the correction pairs: one thread per mobile atom that has any, its entries in list order
    for (int r = tid; r < X.n_row; r += PME_THREADS) {
        const int i = X.row_atom[r];
        double f1[3] = {0.0, 0.0, 0.0}, f2[3] = {0.0, 0.0, 0.0};
        for (int e = X.row_start[r]; e < X.row_start[r + 1]; e++) {
            double d[3], fs;
            const int kind = X.ent_kind[e];
            pmex_pair(X, i, X.ent_j[e], X.ent_qq[e], kind, d, &fs);
            for (int k = 0; k < 3; k++) {
                const double f = fs * d[k];
                if (kind == 0) f1[k] += f; else if (kind == 1) f2[k] += f; else { f2[k] += f; f1[k] -= f; }
            }
        }
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            const double le = dyn.le[sl];
            for (int k = 0; k < 3; k++) X.fex[(size_t)(sl * 3 + k) * n + i] += le * (f1[k] + le * f2[k]);
        }
    }
    if (tid == 0) {
        double t1 = 0.0, t2 = 0.0, tc = 0.0;
        for (int w = 0; w < PME_THREADS / 64; w++) { t1 += s_e[w][0]; t2 += s_e[w][1]; tc += s_e[w][2]; }
        if (X.path) X.path[FAST ? 0 : 1]++;   // (read by blues_get_exact_pme_path: which mesh path served the alchemical class)
        X.epart[0] = 0.0; X.epart[1] = t1 + X.c1; X.epart[2] = t2 + X.c2 + tc; X.epart[3] = 0.0; X.epart[4] = -tc; X.epart[5] = tc;
    }
}

template <typename T>
__global__ void __launch_bounds__(PME_THREADS) k_pme_exact_b(const PmeExArgs<T>* __restrict__ recs, PmeExDyn dyn) {
    const PmeExArgs<T>& X = recs[blockIdx.x];
    if (!X.active) return;
    pmex_body<T>(X, dyn);
}

// mixed precision on a mesh whose half spectrum fits LDS: the pruned pipeline, with the general body (kept out of line, out of this
// kernel's register allocation) for members whose atoms or blocks do not fit
__device__ __noinline__ void pmex_body_general_f(const PmeExArgs<float>& X, const PmeExDyn& dyn) { pmex_body<float, false>(X, dyn); }
__global__ void __launch_bounds__(PME_THREADS) k_pme_exact_fast_b(const PmeExArgs<float>* __restrict__ recs, PmeExDyn dyn) {
    const PmeExArgs<float>& X = recs[blockIdx.x];
    if (!X.active) return;
    double e1, e2;
    if (!pmex_fast_mesh(X, dyn, e1, e2)) { pmex_body_general_f(X, dyn); return; }
    pmex_body<float, true>(X, dyn, e1, e2);
}
