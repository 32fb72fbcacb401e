// kernels_nocutoff.h -- the environment x environment pairs of a System under nonbondedMethod=NoCutoff (vacuum).
//
// Every pair counts: no cutoff, no minimum image, no lists.  Plain 12-6 LJ and bare Coulomb 138.935456 q_i q_j / r between the
// non-alchemical atoms (the alchemical atoms' pairs are the alchemical kernel's, kernels_alch.h, fed a static j-list of every
// environment atom).  Excluded pairs (self included) are skipped; 1-4 exceptions are the bonded kernel's.
//
// One thread per i-atom, the j-atoms staged in LDS 256 at a time and walked in caller order: a thread sums the force on ITS atom
// over all j in a fixed order (each pair is evaluated from both ends; no atomics), so a chain gets the same bits alone and inside a
// batch.  The exclusions are the atom's sorted exclusion row (host-built, self included, duplicates removed) read with a cursor
// that advances as j passes its entries: one compare per pair.
//
// Forces: i = the mobile non-alchemical atoms by i-slot, into the one partial slab k_finalize reads ([3][n_islots]).
// Energies: i = every atom, each pair counted from both ends and halved; one (LJ, Coulomb) pair of partials per block.
//
// Mixed precision (R = float): coordinates relative to the block's first i-atom are formed in fp64 and kept as two fp32 numbers, the
// rounded value and what the rounding left (a vacuum molecule drifts, and one block's atoms may lie tens of nm apart: a single fp32
// offset from the reference would lose the digits of a short separation far from it).  A pair's separation is the difference of
// the rounded values -- exact for nearby atoms -- plus the difference of the remainders.  The pair arithmetic is fp32, every sum
// fp64.  Double precision: fp64 throughout.
#pragma once
#include "device_common.h"

#define NC_THREADS 256

struct NcArgs {
    int active;                 // (batched form) 0: the member sits this launch out
    int n, n_islots;            // atoms; i-slots (mobile non-alchemical atoms, padded to 64)
    const double* x[3];         // positions, caller order
    const double4* par;         // [n] {charge * sqrt(ONE_4PI_EPS0), sigma / 2, 2 sqrt(epsilon), 1 if alchemical}; 0 for alchemical atoms
    const int* tile_atoms;      // [n_islots] caller index of the i-slot's atom, or -1
    const int* ex_start;        // [n + 1] exclusion rows (caller order, ascending, self included)
    const int* ex_idx;
    double* fpart;              // [3][n_islots] force on the i-slots' atoms
    double* epart;              // [blocks][2] LJ, Coulomb (energy form)
};

template <typename R, bool ENERGY>
__device__ __forceinline__ void nocutoff_body(const NcArgs& A, const int blk) {
    constexpr bool SPLIT = sizeof(R) == 4;
    __shared__ R sx[NC_THREADS], sy[NC_THREADS], sz[NC_THREADS], sq[NC_THREADS], shs[NC_THREADS], sse[NC_THREADS];
    __shared__ R lx[SPLIT ? NC_THREADS : 1], ly[SPLIT ? NC_THREADS : 1], lz[SPLIT ? NC_THREADS : 1];   // remainders (mixed precision)
    __shared__ double s_e[NC_THREADS / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = blk * NC_THREADS + tid;
    int i = -1;
    if (ENERGY) { if (slot < A.n && A.par[slot].w == 0.0) i = slot; }
    else if (slot < A.n_islots) i = A.tile_atoms[slot];
    // the block's reference point: its first i-slot's atom (always a real atom: the i-slots are filled from the front)
    const int i0 = ENERGY ? blk * NC_THREADS : A.tile_atoms[blk * NC_THREADS];
    const double xr0 = i0 >= 0 ? A.x[0][i0] : 0.0, xr1 = i0 >= 0 ? A.x[1][i0] : 0.0, xr2 = i0 >= 0 ? A.x[2][i0] : 0.0;
    R xi = (R)0, yi = (R)0, zi = (R)0, xil = (R)0, yil = (R)0, zil = (R)0, qi = (R)0, hsi = (R)0, sei = (R)0;
    int p = 0, pe = 0;
    if (i >= 0) {
        const double dx = A.x[0][i] - xr0, dy = A.x[1][i] - xr1, dz = A.x[2][i] - xr2;
        xi = (R)dx; yi = (R)dy; zi = (R)dz;
        if constexpr (SPLIT) { xil = (R)(dx - (double)xi); yil = (R)(dy - (double)yi); zil = (R)(dz - (double)zi); }
        const double4 P = A.par[i];
        qi = (R)P.x; hsi = (R)P.y; sei = (R)P.z;
        p = A.ex_start[i]; pe = A.ex_start[i + 1];
    }
    int nx = p < pe ? A.ex_idx[p] : 0x7fffffff;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0, elj = 0.0, ecl = 0.0;
    for (int j0 = 0; j0 < A.n; j0 += NC_THREADS) {
        __syncthreads();   // (the previous tile has been read by every thread)
        const int j = j0 + tid;
        if (j < A.n) {
            const double dx = A.x[0][j] - xr0, dy = A.x[1][j] - xr1, dz = A.x[2][j] - xr2;
            sx[tid] = (R)dx; sy[tid] = (R)dy; sz[tid] = (R)dz;
            if constexpr (SPLIT) { lx[tid] = (R)(dx - (double)(R)dx); ly[tid] = (R)(dy - (double)(R)dy); lz[tid] = (R)(dz - (double)(R)dz); }
            const double4 P = A.par[j];
            sq[tid] = (R)P.x; shs[tid] = (R)P.y; sse[tid] = (R)P.z;
        }
        __syncthreads();
        if (i < 0) continue;
        const int jn = min(NC_THREADS, A.n - j0);
        for (int u = 0; u < jn; u++) {
            if (j0 + u == nx) { p++; nx = p < pe ? A.ex_idx[p] : 0x7fffffff; continue; }
            R dx = xi - sx[u], dy = yi - sy[u], dz = zi - sz[u];
            if constexpr (SPLIT) { dx += xil - lx[u]; dy += yil - ly[u]; dz += zil - lz[u]; }
            const R r2 = dx * dx + dy * dy + dz * dz;
            const R inv_r2 = (R)1 / r2, inv_r = (R)1 / sqrt(r2);
            const R sig = hsi + shs[u], eps4 = sei * sse[u], qq = qi * sq[u];
            const R s2 = sig * sig * inv_r2, s6 = s2 * s2 * s2;
            const R uc = qq * inv_r;
            const R fs = (eps4 * ((R)12 * s6 * s6 - (R)6 * s6) + uc) * inv_r2;
            f0 += (double)(fs * dx); f1 += (double)(fs * dy); f2 += (double)(fs * dz);
            if (ENERGY) { elj += (double)(eps4 * (s6 * s6 - s6)); ecl += (double)uc; }
        }
    }
    if (!ENERGY) {
        if (slot < A.n_islots) { A.fpart[slot] = f0; A.fpart[(size_t)A.n_islots + slot] = f1; A.fpart[2 * (size_t)A.n_islots + slot] = f2; }
        return;
    }
    elj = wave_sum(0.5 * elj); ecl = wave_sum(0.5 * ecl);   // (each pair was counted from both ends)
    if (lane == 0) { s_e[wv][0] = elj; s_e[wv][1] = ecl; }
    __syncthreads();
    if (tid < 2) {
        double s = 0.0;
        for (int w = 0; w < NC_THREADS / 64; w++) s += s_e[w][tid];
        A.epart[2 * (size_t)blk + tid] = s;
    }
}

template <typename R, bool ENERGY>
__global__ void __launch_bounds__(NC_THREADS) k_nocutoff(NcArgs A) { nocutoff_body<R, ENERGY>(A, blockIdx.x); }

// one launch for every member of a batch: blockIdx.y = member, its record in HBM
template <typename R, bool ENERGY>
__global__ void __launch_bounds__(NC_THREADS) k_nocutoff_b(const NcArgs* __restrict__ recs) {
    const NcArgs& A = recs[blockIdx.y];
    if (!A.active) return;
    nocutoff_body<R, ENERGY>(A, blockIdx.x);
}
