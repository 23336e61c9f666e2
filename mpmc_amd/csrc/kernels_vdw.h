// kernels_vdw.h -- coupled-dipole many-body van der Waals (option polarvdw, reference src/energy/vdw.c) and what the
// reference switches with it: Lennard-Jones as repulsion only (lj.c:230-231, :77-78, :100-101) and the close-contact
// count behind cavity_autoreject_absolute (energy.c:48-64).
//
// What the reference sums, and this file therefore sums:
//   * k_i = sqrt(alpha_i) * omega_i; atoms with k_i == 0 are left out of the matrix (build_M).  Over the others
//     C = K A K, K = diag(k), A the full Thole matrix: diagonal blocks 1 / alpha_i, off-diagonal blocks the exponentially
//     damped dipole tensor at the minimum-image distance -- no cutoff, same-molecule and frozen-frozen pairs included.
//     e_total = 4.13412763705e16 * 3.81911146e-12 * sum_i sqrt(max(lambda_i(C), 0)).
//   * e_iso: the same expression for the diagonal sub-block of one molecule (the engine runs the same kernels on the site
//     list of the first molecule of each type and keeps the value).
//   * lr_corr (under rd_lrc): every unordered pair that is not frozen-frozen, same-molecule pairs included, whose two
//     alphas and two omegas are all non-zero: -4/3 pi cC / cutoff^3 / volume,
//     cC = 1.5 * 7.63822291e-12 * w_i w_j / (w_i + w_j) * 4.13412763705e16 * a_i a_j.
//   * repulsion: the Lennard-Jones pair rules (different molecules, not frozen-frozen, no zero parameter, both sigma > 0,
//     rimg - 1e-12 < cutoff) with 4 eps_ij (sigma_ij / r)^12 alone; pair correction (16/9) pi eps_ij sigma^3
//     (sigma / cutoff)^9 / volume over the pairs of the Lennard-Jones correction, self correction likewise per atom.
//   * contacts: the number of pairs on different molecules (frozen-frozen pairs count) with rimg < scale, rimg from
//     minimum_image() (the reference's fp64 operation order), compared as the reference compares it.
//
// The eigenvalue sum.  C is symmetric; its eigenvalues are found without eigenvectors:
//   1. vdw_build_kernel writes C (both triangles, bit-symmetric: the tensor is even in the displacement and the factors are
//      applied as (T * k_hi) * k_lo with hi the larger site index, the reference's lower triangle).
//   2. Unblocked Householder tridiagonalisation, column by column (LAPACK's dsytd2 recurrences): vdw_reflect_kernel forms
//      the reflector of column j (v, tau) and writes d_j, e_j; vdw_symv_kernel forms p = tau * C22 v on the trailing block;
//      vdw_rank2_kernel forms w = p - (tau / 2) (p.v) v and C22 -= v w^T + w v^T.  Three launches per column, no workgroup
//      waits for another.  DEVIATION from the textbook in-place form, owned here: both triangles of the trailing block are
//      kept up to date (in the same bits: the update of (r, c) and of (c, r) add the same two products), so that every
//      product is a coalesced row read; the reduction reads and writes twice the bytes of a lower-triangle one.
//   3. vdw_bisect_kernel: one thread per eigenvalue index, Sturm-count bisection from the Gershgorin interval with LAPACK's
//      pivot guard (a pivot above -pivmin that counts is pushed to -pivmin), kVdwBisectSteps halvings.
//   4. vdw_sum_kernel: sum of sqrt(lambda < 0 ? 0 : lambda), scaled.
// Every loop has a trip count fixed before the launch, and every reduction runs in an order that is a function of n
// alone: strided per-thread sums, the 64-lane butterfly, the waves left to right.
// A non-finite matrix (a frequency whose square overflows, a non-finite coordinate) must give a non-finite sum:
// comparisons would silently drop a NaN in the bisection, so vdw_sum_kernel adds 0 * (d_i + e_i) -- exactly +0 for finite
// input, NaN otherwise.
#pragma once
#include "kernels_polar.h"
#include "kernels_tile.h"

namespace mpmc {

constexpr double kVdwAu2InvSec = 4.13412763705e16;  // vdw.c:22
constexpr double kVdwHalfHbar = 3.81911146e-12;     // vdw.c:21 (K s)
constexpr double kVdwCHbar = 7.63822291e-12;        // vdw.c:20 (K s)
constexpr int kVdwBisectSteps = 64;                 // the Gershgorin interval halved to below one ulp of its width
constexpr double kVdwSafeMin = 2.2250738585072014e-308;

// the sites of one matrix: atom slot and k = sqrt(alpha) * omega of each (k != 0)
struct VdwSites {
    const int *idx;
    const double *k;
    int na;
};

// C for the sites of `s`: grid = (ceil(na / 64) [column sites], na [row site]), block = 64.  ld = 3 na.
__global__ __launch_bounds__(64) void vdw_build_kernel(DevAtoms a, DevBox bx, double damp, VdwSites s, double *__restrict__ C,
                                                        int ld, MoveList m) {
    const int ra = blockIdx.y;
    const int cb = blockIdx.x * 64 + threadIdx.x;
    if (cb >= s.na) return;
    const int ia = s.idx[ra], ja = s.idx[cb];
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // xx xy xz yy yz zz
    if (ra == cb) {
        const double k = s.k[ra];
        const double dg = (1.0 / a.alpha[ia]) * k * k;  // (A_ii * k_i) * k_i, vdw.c:125-126
        t[0] = t[3] = t[5] = dg;
    } else {
        double xi, yi, zi, xj, yj, zj;
        moved_position(a, m, ia, xi, yi, zi);
        moved_position(a, m, ja, xj, yj, zj);
        thole_tensor(bx, damp, xi - xj, yi - yj, zi - zj, t[0], t[1], t[2], t[3], t[4], t[5]);
        const double khi = s.k[max(ra, cb)], klo = s.k[min(ra, cb)];
#pragma unroll
        for (int u = 0; u < 6; ++u) t[u] = (t[u] * khi) * klo;
    }
    double *r0 = C + (size_t)(3 * ra) * ld + 3 * cb;
    r0[0] = t[0];
    r0[1] = t[1];
    r0[2] = t[2];
    r0[ld] = t[1];
    r0[ld + 1] = t[3];
    r0[ld + 2] = t[4];
    r0[2 * (size_t)ld] = t[2];
    r0[2 * (size_t)ld + 1] = t[4];
    r0[2 * (size_t)ld + 2] = t[5];
}

// sum of `acc` over the workgroup in a fixed order, delivered to every thread.  red: W + 1 doubles of LDS.
template <int W>
__device__ __forceinline__ double vdw_block_sum(double acc, double *red) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < W; ++k) t += red[k];
        red[W] = t;
    }
    __syncthreads();
    const double r = red[W];
    __syncthreads();
    return r;
}

// Reflector of column j (dlarfg on x = C[j+1 .. n-1][j], read as row j): v[0] = 1, v[i] = x_i / (x_0 - beta), scal[0] = tau,
// e[j] = beta, d[j] = C[j][j]; tau = 0 and e[j] = x_0 when the rest of the column is exactly zero.  The last column
// (j = n - 2) also writes d[n - 1].  One workgroup.
constexpr int kVdwReflectThreads = 1024;
__global__ __launch_bounds__(kVdwReflectThreads) void vdw_reflect_kernel(const double *__restrict__ C, int ld, int n, int j,
                                                                          double *__restrict__ v, double *__restrict__ scal,
                                                                          double *__restrict__ d, double *__restrict__ e) {
    __shared__ double red[kVdwReflectThreads / 64 + 1];
    const int mm = n - j - 1;
    const double *x = C + (size_t)j * ld + j + 1;
    double acc = 0.0;
    for (int i = 1 + (int)threadIdx.x; i < mm; i += kVdwReflectThreads) acc += x[i] * x[i];
    const double xn2 = vdw_block_sum<kVdwReflectThreads / 64>(acc, red);
    const double alpha = x[0];
    double beta = alpha, tau = 0.0, inv = 0.0;
    if (xn2 != 0.0) {  // (a NaN takes this branch and travels on)
        beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
        tau = (beta - alpha) / beta;
        inv = 1.0 / (alpha - beta);
    }
    for (int i = threadIdx.x; i < mm; i += kVdwReflectThreads) v[i] = (i == 0) ? 1.0 : x[i] * inv;
    if (threadIdx.x == 0) {
        scal[0] = tau;
        d[j] = C[(size_t)j * ld + j];
        e[j] = beta;
        if (j == n - 2) d[n - 1] = C[(size_t)(n - 1) * ld + n - 1];
    }
}

// p[i] = tau * sum_k C[j+1+i][j+1+k] v[k]: one wave per row, grid = ceil(mm / 4), block = 256.
constexpr int kVdwSymvWaves = 4;
__global__ __launch_bounds__(64 * kVdwSymvWaves) void vdw_symv_kernel(const double *__restrict__ C, int ld, int n, int j,
                                                                       const double *__restrict__ v,
                                                                       const double *__restrict__ scal, double *__restrict__ p) {
    const int lane = threadIdx.x & 63;
    const int mm = n - j - 1;
    const int i = blockIdx.x * kVdwSymvWaves + (threadIdx.x >> 6);
    if (i >= mm) return;
    const double *row = C + (size_t)(j + 1 + i) * ld + j + 1;
    double acc = 0.0;
    for (int k = lane; k < mm; k += 64) acc += row[k] * v[k];
    acc = wave_sum(acc);
    if (lane == 0) p[i] = scal[0] * acc;
}

// w = p - K v, K = (tau / 2) (p.v); one expression, never contracted: rows and columns use the same bits
__device__ __forceinline__ double vdw_w(double p, double K, double v) {
#pragma clang fp contract(off)
    const double t = K * v;
    return p - t;
}
__device__ __forceinline__ double vdw_rank2(double c, double vr, double wr, double vc, double wc) {
#pragma clang fp contract(off)
    const double t1 = vr * wc, t2 = wr * vc;
    const double s = t1 + t2;  // (c, r) forms t2 + t1: the same bits
    return c - s;
}

// C22 -= v w^T + w v^T: a workgroup takes kVdwUpdRows rows of the trailing block, a wave four of them; every workgroup forms
// p.v for itself, in the same order.  grid = ceil(mm / kVdwUpdRows), block = 256.
constexpr int kVdwUpdWaves = 4;
constexpr int kVdwUpdRowsPerWave = 4;
constexpr int kVdwUpdRows = kVdwUpdWaves * kVdwUpdRowsPerWave;
__global__ __launch_bounds__(64 * kVdwUpdWaves) void vdw_rank2_kernel(double *__restrict__ C, int ld, int n, int j,
                                                                       const double *__restrict__ v,
                                                                       const double *__restrict__ p,
                                                                       const double *__restrict__ scal) {
    __shared__ double red[kVdwUpdWaves + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int mm = n - j - 1;
    double acc = 0.0;
    for (int k = threadIdx.x; k < mm; k += 64 * kVdwUpdWaves) acc += p[k] * v[k];
    const double K = 0.5 * scal[0] * vdw_block_sum<kVdwUpdWaves>(acc, red);
    const int r0 = blockIdx.x * kVdwUpdRows + wv * kVdwUpdRowsPerWave;
    double vr[kVdwUpdRowsPerWave], wr[kVdwUpdRowsPerWave];
#pragma unroll
    for (int u = 0; u < kVdwUpdRowsPerWave; ++u) {
        const int r = min(r0 + u, mm - 1);
        vr[u] = v[r];
        wr[u] = vdw_w(p[r], K, vr[u]);
    }
    double *base = C + (size_t)(j + 1) * ld + j + 1;
    for (int c = lane; c < mm; c += 64) {
        const double vc = v[c];
        const double wc = vdw_w(p[c], K, vc);
#pragma unroll
        for (int u = 0; u < kVdwUpdRowsPerWave; ++u) {
            const int r = r0 + u;
            if (r < mm) {
                double *q = base + (size_t)r * ld + c;
                *q = vdw_rank2(*q, vr[u], wr[u], vc, wc);
            }
        }
    }
}

// Eigenvalue k (ascending) of the symmetric tridiagonal (d[0..n), e[0..n-1)): thread k.  grid = ceil(n / 64), block = 64.
__global__ __launch_bounds__(64) void vdw_bisect_kernel(const double *__restrict__ d, const double *__restrict__ e, int n,
                                                         double *__restrict__ lam) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    // Gershgorin interval and pivmin, the same for every thread (wave-uniform loads)
    double gl = d[0], gu = d[0], emax2 = 0.0, eprev = 0.0;
    for (int i = 0; i < n; ++i) {
        const double en = (i < n - 1) ? fabs(e[i]) : 0.0;
        const double lo = d[i] - eprev - en, hi = d[i] + eprev + en;
        gl = (lo < gl) ? lo : gl;
        gu = (hi > gu) ? hi : gu;
        emax2 = (en * en > emax2) ? en * en : emax2;
        eprev = en;
    }
    const double pivmin = kVdwSafeMin * ((emax2 > 1.0) ? emax2 : 1.0);
    const double bnorm = (fabs(gl) > fabs(gu)) ? fabs(gl) : fabs(gu);
    const double widen = 2.1 * bnorm * 0x1p-53 * (double)n + 2.1 * pivmin;  // dstebz
    double lo = gl - widen, hi = gu + widen;
    for (int it = 0; it < kVdwBisectSteps; ++it) {
        const double x = 0.5 * (lo + hi);
        // number of eigenvalues below x: negative pivots of the LDL^T of T - x (dlaebz)
        double q = d[0] - x;
        int cnt = 0;
        if (q <= pivmin) {
            ++cnt;
            q = (q < -pivmin) ? q : -pivmin;
        }
        for (int i = 1; i < n; ++i) {
            const double ei = e[i - 1];
            q = d[i] - (ei * ei) / q - x;
            if (q <= pivmin) {
                ++cnt;
                q = (q < -pivmin) ? q : -pivmin;
            }
        }
        if (cnt > k) hi = x;
        else lo = x;
    }
    if (k < n) lam[k] = 0.5 * (lo + hi);
}

// out[0] = au2invsec * halfHBAR * sum_k sqrt(lambda_k clipped at 0) (eigen2energy, vdw.c:209-221, :606).  One workgroup.
constexpr int kVdwSumThreads = 1024;
__global__ __launch_bounds__(kVdwSumThreads) void vdw_sum_kernel(const double *__restrict__ lam, const double *__restrict__ d,
                                                                  const double *__restrict__ e, int n,
                                                                  double *__restrict__ out) {
    __shared__ double red[kVdwSumThreads / 64 + 1];
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += kVdwSumThreads) {
        const double l = lam[k];
        acc += sqrt((l < 0.0) ? 0.0 : l);
        acc += 0.0 * d[k] + ((k < n - 1) ? 0.0 * e[k] : 0.0);  // +0, or NaN for a non-finite matrix
    }
    const double s = vdw_block_sum<kVdwSumThreads / 64>(acc, red);
    if (threadIdx.x == 0) out[0] = (s * kVdwAu2InvSec) * kVdwHalfHbar;
}

// lr_corr (lr_vdw_corr, vdw.c:346-385).  omega: per atom, zero for pad atoms.  Tile grid and partials as lj_lrc_kernel's.
constexpr int kVdwLrcWaves = 8;
__global__ __launch_bounds__(64 * kVdwLrcWaves) void vdw_lrc_kernel(DevAtoms a, const double *__restrict__ omega, DevBox bx,
                                                                     DirtyBlocks sel, double *__restrict__ partials) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    double *out = partials + (size_t)(I * gridDim.x + J);
    if (J < I) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    __shared__ double sal[kWave], sw[kWave];
    __shared__ int sfl[kWave];
    __shared__ double red[kVdwLrcWaves];
    if (wv == 0) {
        sal[lane] = a.alpha[J * kWave + lane];
        sw[lane] = omega[J * kWave + lane];
        sfl[lane] = a.flags[J * kWave + lane];
    }
    __syncthreads();
    const int i = I * kWave + lane;
    const double a1 = a.alpha[i], w1 = omega[i];
    const int fli = a.flags[i];
    const double rc = bx.cutoff;
    const double irc3 = 1.0 / (rc * rc * rc);
    double acc = 0.0;
    for (int jj = wv * (kWave / kVdwLrcWaves); jj < (wv + 1) * (kWave / kVdwLrcWaves); ++jj) {
        const int j = J * kWave + jj;
        if (!pair_in_sum(i, j, fli, sfl[jj])) continue;
        const double a2 = sal[jj], w2 = sw[jj];
        if (w1 == 0.0 || w2 == 0.0 || a1 == 0.0 || a2 == 0.0) continue;
        const double cC = 1.5 * kVdwCHbar * w1 * w2 / (w1 + w2) * kVdwAu2InvSec * a1 * a2;
        acc += -4.0 / 3.0 * kPI * cC * irc3 / bx.volume;
    }
    block_sum_store<kVdwLrcWaves>(acc, red, out);
}

struct RepTile {
    double x[kWave], y[kWave], z[kWave], eps[kWave], sig[kWave];
    int mol[kWave], flags[kWave];
};
__device__ __forceinline__ void load_rep_tile(RepTile &t, const DevAtoms &a, const MoveList &m, int j0, int lane) {
    const int j = j0 + lane;  // j < npad always (the grid covers npad / 64 tiles)
    moved_position(a, m, j, t.x[lane], t.y[lane], t.z[lane]);
    t.eps[lane] = a.eps[j];
    t.sig[lane] = a.sig[j];
    t.mol[lane] = a.mol[j];
    t.flags[lane] = a.flags[j];
}

// Repulsion-only Lennard-Jones pair sum.  Grids of the full and the incremental pass: owned_tile().  a: the REAL epsilon /
// sigma (the Lennard-Jones kernels of the same call are handed zeros); a moved atom's position comes from the list.
constexpr int kRepWaves = 8;
__global__ __launch_bounds__(64 * kRepWaves) void rep_tile_kernel(DevAtoms a, DevBox bx, DirtyBlocks sel,
                                                                   double *__restrict__ partials, MoveList m) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    double *out = partials + (size_t)I * gridDim.x + J;
    if (J < I) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    __shared__ RepTile tj, ti;
    __shared__ double red[kRepWaves];
    if (wv == 0) load_rep_tile(tj, a, m, J * kWave, lane);
    if (wv == 1) load_rep_tile(ti, a, m, I * kWave, lane);
    __syncthreads();
    const int i = I * kWave + lane;
    const double xi = ti.x[lane], yi = ti.y[lane], zi = ti.z[lane];
    const double epsi = ti.eps[lane], sigi = ti.sig[lane];
    const int moli = ti.mol[lane], fli = ti.flags[lane];
    const double rc = bx.cutoff, rc2_hi = cutoff_prefilter_sq(rc);
    double acc = 0.0;
    for (int jj = wv * (kWave / kRepWaves); jj < (wv + 1) * (kWave / kRepWaves); ++jj) {
        const int j = J * kWave + jj;
        if (!pair_in_sum(i, j, fli, tj.flags[jj])) continue;
        if (moli == tj.mol[jj]) continue;  // rd_excluded
        const double epsj = tj.eps[jj], sigj = tj.sig[jj];
        if (!(sigi > 0.0 && sigj > 0.0) || epsi == 0.0 || epsj == 0.0) continue;  // what the Lennard-Jones path leaves out
        double r2, ri2, dx, dy, dz;
        minimum_image_sq(bx, xi - tj.x[jj], yi - tj.y[jj], zi - tj.z[jj], r2, ri2, dx, dy, dz);
        if (!(ri2 <= rc2_hi)) continue;
        const double rimg = sqrt(ri2);
        if (!(rimg - kSMALL_dR < rc)) continue;
        const double sig = 0.5 * (sigi + sigj);
        const double eps = sqrt(epsi * epsj);
        const double sor = fabs(sig) / rimg;
        double s6 = sor * sor * sor;
        s6 *= s6;
        acc += 4.0 * eps * (s6 * s6);  // term6 = 0 (lj.c:230-231)
    }
    block_sum_store<kRepWaves>(acc, red, out);
}

// Its long-range correction: lj_lrc_kernel's pairs and atoms with the repulsion term alone (lj.c:77-78, :100-101).
__global__ __launch_bounds__(64 * kVdwLrcWaves) void rep_lrc_kernel(DevAtoms a, DevBox bx, DirtyBlocks sel,
                                                                  double *__restrict__ partials) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    double *out = partials + (size_t)(I * gridDim.x + J);
    if (J < I) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    __shared__ double seps[kWave], ssig[kWave];
    __shared__ int sfl[kWave];
    __shared__ double red[kVdwLrcWaves];
    if (wv == 0) {
        seps[lane] = a.eps[J * kWave + lane];
        ssig[lane] = a.sig[J * kWave + lane];
        sfl[lane] = a.flags[J * kWave + lane];
    }
    __syncthreads();
    const int i = I * kWave + lane;
    const double epsi = a.eps[i], sigi = a.sig[i];
    const int fli = a.flags[i];
    const double rc = bx.cutoff;
    double acc = 0.0;
    for (int jj = wv * (kWave / kVdwLrcWaves); jj < (wv + 1) * (kWave / kVdwLrcWaves); ++jj) {
        const int j = J * kWave + jj;
        if (!pair_in_sum(i, j, fli, sfl[jj])) continue;
        const double sigj = ssig[jj], epsj = seps[jj];
        double sig, eps;
        if (sigi < 0.0 || sigj < 0.0) {
            sig = 0.5 * (fabs(sigi) + fabs(sigj));
            eps = 0.0;  // never set for attractive-only pairs (pairs.c:201-203)
        } else if (sigi == 0.0 || sigj == 0.0) {
            sig = 0.0;
            eps = sqrt(epsi * epsj);
        } else {
            sig = 0.5 * (sigi + sigj);
            eps = sqrt(epsi * epsj);
        }
        if (eps != 0.0 && sig != 0.0) {
            const double sc = fabs(sig) / rc;
            double s3 = fabs(sig);
            s3 *= s3 * s3;
            const double sc3 = sc * sc * sc, sc9 = sc3 * sc3 * sc3;
            acc += (16.0 / 9.0) * kPI * eps * s3 * sc9 / bx.volume;
        }
    }
    if (I == J && wv == 0) {  // self term once per atom, on the diagonal tile
        if ((fli & kValid) && !(fli & kFrozen) && sigi != 0.0 && epsi != 0.0) {
            const double sc = fabs(sigi) / rc;
            double s3 = fabs(sigi);
            s3 *= s3 * s3;
            const double sc3 = sc * sc * sc, sc9 = sc3 * sc3 * sc3;
            acc += (16.0 / 9.0) * kPI * epsi * s3 * sc9 / bx.volume;
        }
    }
    block_sum_store<kVdwLrcWaves>(acc, red, out);
}

// Close contacts (cavity_absolute_check, energy.c:48-64): per tile, the number of pairs of two present atoms on different
// molecules with rimg < scale -- frozen-frozen pairs count.  The count goes to the spare fourth channel of the pair kernel's
// tile partials (which that kernel has just cleared), so it is added up, as a sum of exact small integers, by whoever adds
// up those partials.  Launched behind the pair kernel with the pair kernel's grid and dirty blocks.
constexpr int kContactWaves = 8;
__global__ __launch_bounds__(64 * kContactWaves) void contact_tile_kernel(DevAtoms a, DevBox bx, double scale, DirtyBlocks sel,
                                                                           double *__restrict__ pair_partials, int channels,
                                                                           int channel, MoveList m) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    if (J < I) return;  // (cleared by the pair kernel)
    double *out = pair_partials + (size_t)(I * gridDim.x + J) * channels + channel;
    __shared__ double sx[kWave], sy[kWave], sz[kWave];
    __shared__ int smol[kWave], sfl[kWave];
    __shared__ double red[kContactWaves];
    if (wv == 0) {
        const int j = J * kWave + lane;
        moved_position(a, m, j, sx[lane], sy[lane], sz[lane]);
        smol[lane] = a.mol[j];
        sfl[lane] = a.flags[j];
    }
    __syncthreads();
    const int i = I * kWave + lane;
    double xi, yi, zi;
    moved_position(a, m, i, xi, yi, zi);
    const int moli = a.mol[i], fli = a.flags[i];
    double acc = 0.0;
    for (int jj = wv * (kWave / kContactWaves); jj < (wv + 1) * (kWave / kContactWaves); ++jj) {
        const int j = J * kWave + jj;
        if (!(j > i) || !(fli & kValid) || !(sfl[jj] & kValid) || moli == smol[jj]) continue;
        double r, rimg, dx, dy, dz;
        minimum_image(bx, xi - sx[jj], yi - sy[jj], zi - sz[jj], r, rimg, dx, dy, dz);
        if (rimg < scale) acc += 1.0;
    }
    block_sum_store<kContactWaves>(acc, red, out);
}

}  // namespace mpmc
