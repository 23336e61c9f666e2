// kernels_exact.h -- the exact Thole dipoles (polar_iterative off, reference src/energy/polar.c:91-95): A mu = E_static is
// solved directly on the polarizable view's expanded matrix, by a blocked right-looking Cholesky factorization A = L L^T
// and two blocked substitutions, fp64 throughout.  mpmc_hip_set_exact_polar() switches the engine to it.
//
// What is factored.  The resident A of the view (build_amatrix_kernel / update_amatrix_kernel, (3 nvpad)^2 doubles) is
// kept; chol_copy_kernel copies the lower-triangle tiles of its first n = 3 nv rows into a work copy W.  The factorization
// covers np = ceil(n / 64) panels, i.e. 64 np rows: rows n .. 64 np - 1 are given a unit diagonal and zeros elsewhere, so
// they factor to themselves, contribute exact zeros to every other row and leave every result a function of n alone, not
// of nvpad (64 np <= 3 nvpad always: nvpad is a multiple of 128).
//
// Panel width 64.  One wave has 64 lanes: the diagonal-block factor, the panel solve and both substitutions give a lane a
// row of the block, and the 64 x 64 tile of the trailing update is four waves of four 16 x 16 MFMA accumulators each.  A
// width of 32 would double the launch count (the small sizes are bound by it) and halve the flops per byte of the update.
//
// Launches.  Per panel k, three plain launches:
//   chol_diag_kernel   one workgroup: L11 = chol(W11) in LDS, unblocked, plain VALU; every pivot is tested with !(d > 0)
//                      (which also catches NaN): a failing pivot sets the call's flag word and is replaced by 1, so that
//                      the launches behind it run on, with their fixed trip counts, to numbers nobody uses.
//   chol_panel_kernel  np - 1 - k workgroups: L21 = W21 L11^-T, a lane per row, forward substitution in LDS, plain VALU.
//   chol_trail_kernel  the tiles (I, J), k < J <= I < np: W_IJ -= L_Ik L_Jk^T on v_mfma_f64_16x16x4_f64, operands staged
//                      through LDS.  All n^3 / 3 flops of the factorization are here.
// The last panel has only its diagonal block: 3 np - 2 launches, plus one copy.  A substitution is one launch per panel
// and direction (chol_fwd_kernel, chol_bwd_kernel): every workgroup of launch k solves the diagonal block k for itself
// (64 steps of a wave, cheaper than a launch) and applies the result to its own block of the right-hand side, the
// workgroup of block k stores it.  With chol_rhs_kernel in front and chol_energy_kernel behind, an energy() is
// (3 np - 2) + 1 + 2 np + 2 = 5 np + 1 launches.  The tensor (chol_tensor_kernel) is 2 np + 2 more on the same factor.
//
// Conditions carried over from kernels_vdw.h: no workgroup waits for another, nothing is persistent or cooperative,
// every loop's trip count is fixed before the launch, and every sum runs in an order that is a function of n alone -- the
// K order of the MFMA accumulation is m = 0, 4, .. 60 with the instruction's own fixed order inside a group of four, a
// row's substitution sums run left to right (right to left in the back substitution), the energy and tensor sums are
// strided per thread, then the 64-lane butterfly, then the waves left to right.  A result is a function of the input.
#pragma once
#include "kernels_polar.h"

namespace mpmc {

constexpr int kCholNB = 64;        // panel width = tile edge
constexpr int kCholLd = 65;        // row stride of a tile in LDS (doubles): a column walk touches every bank once
constexpr int kCholThreads = 256;  // every kernel of the file but the two one-block sums

typedef double chol_v4d __attribute__((ext_vector_type(4)));

// W <- the lower-triangle tiles of A's first n rows / columns; unit diagonal on the rows n .. 64 np - 1.  Clears the
// call's flag word.  grid = (np, np) [column tile, row tile]; block = kCholThreads.
__global__ __launch_bounds__(kCholThreads) void chol_copy_kernel(const double *__restrict__ A, int lda, int n,
                                                                  double *__restrict__ W, unsigned *__restrict__ flag) {
    const int J = blockIdx.x, I = blockIdx.y;
    if (I == 0 && J == 0 && threadIdx.x == 0) *flag = 0u;
    if (J > I) return;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const int j = J * kCholNB + c;
#pragma unroll 4
    for (int rr = 0; rr < kCholNB / 4; ++rr) {
        const int i = I * kCholNB + r0 + 4 * rr;
        const size_t o = (size_t)i * lda + j;
        W[o] = (i < n && j < n) ? A[o] : (i == j ? 1.0 : 0.0);
    }
}

// L11 = chol(W11), in place (lower triangle).  grid = 1; block = kCholThreads: thread (i = t & 63, q = t >> 6) owns the
// columns j + 1 + q, j + 5 + q, .. <= i of row i in the update behind column j.
__global__ __launch_bounds__(kCholThreads) void chol_diag_kernel(double *__restrict__ W, int lda, int k,
                                                                  unsigned *__restrict__ flag) {
    __shared__ double S[kCholNB * kCholLd];
    __shared__ double col[kCholNB], dg[kCholNB];
    const int i = threadIdx.x & 63, q = threadIdx.x >> 6;
    double *blk = W + ((size_t)k * kCholNB) * lda + (size_t)k * kCholNB;
#pragma unroll 4
    for (int rr = 0; rr < kCholNB / 4; ++rr) {
        const int r = q + 4 * rr;
        S[r * kCholLd + i] = blk[(size_t)r * lda + i];
    }
    __syncthreads();
    bool any_bad = false;
    for (int j = 0; j < kCholNB; ++j) {
        const double d = S[j * kCholLd + j];
        const bool bad = !(d > 0.0);
        any_bad |= bad;
        const double l = sqrt(bad ? 1.0 : d);
        if (q == 0) {
            if (i > j) {
                const double v = S[i * kCholLd + j] / l;
                col[i] = v;
                S[i * kCholLd + j] = v;
            } else if (i == j) {
                dg[j] = l;
            }
        }
        __syncthreads();
        if (i > j) {
            const double li = col[i];
            for (int c = j + 1 + q; c <= i; c += 4) S[i * kCholLd + c] = fma(-li, col[c], S[i * kCholLd + c]);
        }
        __syncthreads();
    }
    if (any_bad && threadIdx.x == 0) *flag = 1u;
#pragma unroll 4
    for (int rr = 0; rr < kCholNB / 4; ++rr) {
        const int r = q + 4 * rr;
        if (i <= r) blk[(size_t)r * lda + i] = (i == r) ? dg[r] : S[r * kCholLd + i];
    }
}

// L21 = W21 L11^-T for the 64 rows of block I = k + 1 + blockIdx.x.  All four waves bring the two tiles in (one round of
// loads in flight instead of a wave's sixteen), then wave 0 solves: lane r solves x L11^T = (row r), left to right.
// grid = np - 1 - k; block = kCholThreads.
__global__ __launch_bounds__(kCholThreads) void chol_panel_kernel(double *__restrict__ W, int lda, int k) {
    __shared__ double L[kCholNB * kCholNB];  // L11[j][m]: every lane reads the same word
    __shared__ double X[kCholNB * kCholLd];  // X[m][r]: column m of the block, lanes along the rows
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const size_t kb = (size_t)k * kCholNB, rb = (size_t)(k + 1 + blockIdx.x) * kCholNB;
#pragma unroll
    for (int rr = 0; rr < kCholNB / 4; ++rr) {
        const int r = q + 4 * rr;
        L[r * kCholNB + lane] = W[(kb + r) * lda + kb + lane];
        X[lane * kCholLd + r] = W[(rb + r) * lda + kb + lane];
    }
    __syncthreads();
    if (q == 0) {
        for (int j = 0; j < kCholNB; ++j) {
            double acc = X[j * kCholLd + lane];
            for (int m = 0; m < j; ++m) acc = fma(-X[m * kCholLd + lane], L[j * kCholNB + m], acc);
            X[j * kCholLd + lane] = acc / L[j * kCholNB + j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < kCholNB / 4; ++rr) {
        const int r = q + 4 * rr;
        W[(rb + r) * lda + kb + lane] = X[lane * kCholLd + r];
    }
}

// W_IJ -= L_Ik L_Jk^T for the tile I = k + 1 + blockIdx.y, J = k + 1 + blockIdx.x (J <= I).  Wave w owns the rows
// 16 w .. 16 w + 15 of the tile: four accumulators of v_mfma_f64_16x16x4_f64, which takes A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15] and holds D[row = (lane >> 4) + 4 reg][col = lane & 15].  The A operand is negated:
// fma(-a, b, c) is c - a b in the same bits.  grid = (np - 1 - k, np - 1 - k); block = kCholThreads.
__global__ __launch_bounds__(kCholThreads) void chol_trail_kernel(double *__restrict__ W, int lda, int k) {
    const int J = k + 1 + blockIdx.x, I = k + 1 + blockIdx.y;
    if (J > I) return;
    __shared__ double LA[kCholNB * kCholLd], LB[kCholNB * kCholLd];
    const size_t kb = (size_t)k * kCholNB;
    {
        const int c2 = (threadIdx.x & 31) * 2, r0 = threadIdx.x >> 5;
#pragma unroll
        for (int rr = 0; rr < kCholNB / 8; ++rr) {
            const int r = r0 + 8 * rr;
            const double2 va = *reinterpret_cast<const double2 *>(W + ((size_t)I * kCholNB + r) * lda + kb + c2);
            const double2 vb = *reinterpret_cast<const double2 *>(W + ((size_t)J * kCholNB + r) * lda + kb + c2);
            LA[r * kCholLd + c2] = va.x;
            LA[r * kCholLd + c2 + 1] = va.y;
            LB[r * kCholLd + c2] = vb.x;
            LB[r * kCholLd + c2 + 1] = vb.y;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    double *tile = W + ((size_t)I * kCholNB + 16 * w + lk) * lda + (size_t)J * kCholNB + lr;
    chol_v4d acc[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) acc[jt][reg] = tile[(size_t)(4 * reg) * lda + 16 * jt];
    __syncthreads();
#pragma unroll 4
    for (int m0 = 0; m0 < kCholNB; m0 += 4) {
        const double a = -LA[(16 * w + lr) * kCholLd + m0 + lk];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const double b = LB[(16 * jt + lr) * kCholLd + m0 + lk];
            acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[jt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) tile[(size_t)(4 * reg) * lda + 16 * jt] = acc[jt][reg];
}

// The right-hand sides, 64 np rows each (stride ldv).  NRHS = 1: E_static of the view; NRHS = 3: the unit field along q at
// every site (thole_polarizability.c:27-37 sums the blocks of A^-1: C[:, q] = sum_i mu_i^(q)).  Zero on the rows past n.
// grid = np; block = 64.
template <int NRHS>
__global__ __launch_bounds__(64) void chol_rhs_kernel(const double *__restrict__ es, int n, int ldv, double *__restrict__ b) {
    const int i = blockIdx.x * kCholNB + threadIdx.x;
#pragma unroll
    for (int r = 0; r < NRHS; ++r) {
        double v;
        if (NRHS == 1) v = (i < n) ? es[i] : 0.0;
        else v = (i < n && (i % 3) == r) ? 1.0 : 0.0;
        b[(size_t)r * ldv + i] = v;
    }
}

// Forward substitution, panel k: y_k = L11^-1 b_k (every workgroup, for itself); the workgroup of block I = k stores it, a
// workgroup I > k forms b_I -= L_Ik y_k.  b_k is complete when the launch starts and nobody writes it.  All four waves
// bring the two tiles in, then wave 0 works alone, lane i on row i; y_k travels between its lanes by lane reads.
// grid = np - k; block = kCholThreads.
template <int NRHS>
__global__ __launch_bounds__(kCholThreads) void chol_fwd_kernel(const double *__restrict__ W, int lda, int k,
                                                                 double *__restrict__ b, double *__restrict__ y, int ldv) {
    __shared__ double T[kCholNB * kCholLd], T2[kCholNB * kCholLd];
    const int i = threadIdx.x & 63, q = threadIdx.x >> 6, I = k + blockIdx.x;
    const size_t kb = (size_t)k * kCholNB, rb = (size_t)I * kCholNB;
#pragma unroll
    for (int rr = 0; rr < kCholNB / 4; ++rr) {
        const int r = q + 4 * rr;
        T[r * kCholLd + i] = W[(kb + r) * lda + kb + i];
        if (I != k) T2[r * kCholLd + i] = W[(rb + r) * lda + kb + i];
    }
    __syncthreads();
    if (q != 0) return;
    double acc[NRHS], mine[NRHS];
#pragma unroll
    for (int r = 0; r < NRHS; ++r) {
        acc[r] = b[(size_t)r * ldv + kb + i];
        mine[r] = 0.0;
    }
#pragma unroll 2
    for (int j = 0; j < kCholNB; ++j) {
        const double ljj = T[j * kCholLd + j], lij = T[i * kCholLd + j];
#pragma unroll
        for (int r = 0; r < NRHS; ++r) {
            const double yj = __shfl(acc[r], j) / ljj;
            if (i == j) mine[r] = yj;
            if (i > j) acc[r] = fma(-lij, yj, acc[r]);
        }
    }
    if (I == k) {
#pragma unroll
        for (int r = 0; r < NRHS; ++r) y[(size_t)r * ldv + kb + i] = mine[r];
        return;
    }
#pragma unroll
    for (int r = 0; r < NRHS; ++r) acc[r] = b[(size_t)r * ldv + rb + i];
#pragma unroll 2
    for (int j = 0; j < kCholNB; ++j) {
        const double lij = T2[i * kCholLd + j];
#pragma unroll
        for (int r = 0; r < NRHS; ++r) acc[r] = fma(-lij, __shfl(mine[r], j), acc[r]);
    }
#pragma unroll
    for (int r = 0; r < NRHS; ++r) b[(size_t)r * ldv + rb + i] = acc[r];
}

// Back substitution, panel k (launched for k = np - 1 .. 0): x_k = L11^-T y_k; the workgroup of block J = k stores it, a
// workgroup J < k forms y_J -= L_kJ^T x_k.  Loads and roles as in chol_fwd_kernel.  grid = k + 1; block = kCholThreads.
template <int NRHS>
__global__ __launch_bounds__(kCholThreads) void chol_bwd_kernel(const double *__restrict__ W, int lda, int k,
                                                                 double *__restrict__ y, double *__restrict__ x, int ldv) {
    __shared__ double T[kCholNB * kCholLd], T2[kCholNB * kCholLd];
    const int i = threadIdx.x & 63, q = threadIdx.x >> 6, J = blockIdx.x;
    const size_t kb = (size_t)k * kCholNB, cb = (size_t)J * kCholNB;
#pragma unroll
    for (int rr = 0; rr < kCholNB / 4; ++rr) {
        const int r = q + 4 * rr;
        T[r * kCholLd + i] = W[(kb + r) * lda + kb + i];
        if (J != k) T2[r * kCholLd + i] = W[(kb + r) * lda + cb + i];
    }
    __syncthreads();
    if (q != 0) return;
    double acc[NRHS], mine[NRHS];
#pragma unroll
    for (int r = 0; r < NRHS; ++r) {
        acc[r] = y[(size_t)r * ldv + kb + i];
        mine[r] = 0.0;
    }
#pragma unroll 2
    for (int j = kCholNB - 1; j >= 0; --j) {
        const double ljj = T[j * kCholLd + j], lji = T[j * kCholLd + i];
#pragma unroll
        for (int r = 0; r < NRHS; ++r) {
            const double xj = __shfl(acc[r], j) / ljj;
            if (i == j) mine[r] = xj;
            if (i < j) acc[r] = fma(-lji, xj, acc[r]);
        }
    }
    if (J == k) {
#pragma unroll
        for (int r = 0; r < NRHS; ++r) x[(size_t)r * ldv + kb + i] = mine[r];
        return;
    }
#pragma unroll
    for (int r = 0; r < NRHS; ++r) acc[r] = y[(size_t)r * ldv + cb + i];
#pragma unroll 2
    for (int j = 0; j < kCholNB; ++j) {
        const double lji = T2[j * kCholLd + i];
#pragma unroll
        for (int r = 0; r < NRHS; ++r) acc[r] = fma(-lji, __shfl(mine[r], j), acc[r]);
    }
#pragma unroll
    for (int r = 0; r < NRHS; ++r) y[(size_t)r * ldv + cb + i] = acc[r];
}

// The dipoles of the view and U_pol = -1/2 sum mu . E_static (polar.c:107-116) into the record slots the iterative path
// uses.  A set flag word (the matrix was not positive definite) selects the iterative path's divergence fallback
// mu = alpha E_static (fallback_dipoles_kernel, thole_iterative.c:199-210) and is reported in the slot behind U_pol, where
// the iterative path keeps <rrms> (0 in this mode).  grid = 1; block = 256.
__global__ __launch_bounds__(256) void chol_energy_kernel(int nv, int nvpad, const double *__restrict__ x,
                                                           const double *__restrict__ alpha, const double *__restrict__ es,
                                                           const unsigned *__restrict__ flag, double *__restrict__ mu,
                                                           double *__restrict__ out /* [2] */) {
    const bool failed = *flag != 0u;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nvpad; i += blockDim.x) {
        double m[3] = {0.0, 0.0, 0.0};
        if (i < nv) {
            const double al = alpha[i];
#pragma unroll
            for (int p = 0; p < 3; ++p) m[p] = failed ? al * es[3 * i + p] : x[3 * i + p];
            acc += m[0] * es[3 * i] + m[1] * es[3 * i + 1] + m[2] * es[3 * i + 2];
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) mu[3 * i + p] = m[p];
    }
    acc = wave_sum(acc);
    __shared__ double s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = -0.5 * ((s[0] + s[1]) + (s[2] + s[3]));
        out[1] = failed ? 1.0 : 0.0;
    }
}

// C[p][q] = sum_i x^(q)[3 i + p] (row-major out[9]) from the three unit-field solutions.  grid = 1; block = 256.
__global__ __launch_bounds__(256) void chol_tensor_kernel(int nv, const double *__restrict__ x, int ldv,
                                                           double *__restrict__ out /* [9] */) {
    double acc[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) acc[u] = 0.0;
    for (int i = threadIdx.x; i < nv; i += blockDim.x)
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[3 * p + q] += x[(size_t)q * ldv + 3 * i + p];
    __shared__ double s[4][9];
#pragma unroll
    for (int u = 0; u < 9; ++u) {
        const double v = wave_sum(acc[u]);
        if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6][u] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9) out[threadIdx.x] = (s[0][threadIdx.x] + s[1][threadIdx.x]) + (s[2][threadIdx.x] + s[3][threadIdx.x]);
}

}  // namespace mpmc
