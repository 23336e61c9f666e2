// kernels_dimer.h -- energies of a NON-PERIODIC dimer of two rigid molecules for many placements at once: the hot path
// of the reference's `ensemble surf` (src/mc/surface.c:16-76, :289-376) and of mpmc_hip_dimer_energies().
//
// Per placement three numbers, as surface_energy() splits them:
//   es     sum q_i q_j / r over the inter-molecular pairs with both charges non-zero (coulombic_nopbc, coulombic.c:198-217);
//          0 under rd_only;
//   rd     Lennard-Jones without cutoff, long-range correction or Feynman-Hibbs term (lj_nopbc, lj.c:279-317), or the
//          PHAHST term (disp_expansion_nopbc, disp_expansion.c:105-153), over the inter-molecular pairs pair_exclusions()
//          leaves in (pairs.c:56-78); per-pair functions: rdform_mix / rdform_lj (kernels_rdforms.h), disp_pair_energy
//          (kernels_disp.h);
//   polar  -1/2 sum mu . E_static (+ mu . ef_induced_change under polar_palmo, polar.c:107-116) of the Thole system of ALL
//          sites of both molecules: the A matrix over every pair, intra-molecular ones included, without cutoff
//          (thole_matrix.c:72-143, through thole_coef<MODEL>); the static field inter-molecular only and r != 0
//          (thole_field_nopbc, thole_field.c:39-68); the solver of thole_iterative.c.
// The cell is the zero-volume cell of a surf input: its reciprocal basis is NaN, minimum_image() takes its isnan branch and
// returns the plain displacement (pairs.c:279), and the cutoff is MAXVALUE (pbc.c:19), so no cutoff test can fail.
//
// Mapping.  ONE WAVE PER PLACEMENT; a workgroup is one wave and walks a chunk of kDimerChunk consecutive placements.
//   lanes 0 .. N-1 (N = n1 + n2 <= 32) own the sites, molecule 1's first: position, static field, dipole and the running
//   induced-field sum live in the lane's registers;
//   the n1 n2 inter-molecular pairs (es, rd) and the N (N - 1) / 2 pairs of the A matrix are dealt over the 64 lanes,
//   pair p to lane p % 64; the {c3, c5} of a pair sit in LDS (at most 496 x 16 B), the tensor is rebuilt from them and the
//   two positions wherever it is applied (as the engine's pair-coefficient sweeps do);
//   a Jacobi sweep is N steps in which every lane adds T_ik mu_k for the broadcast site k (ascending k: the reference's
//   order); a Gauss-Seidel sweep is such a pass followed by N steps in which the site whose turn it is takes its new dipole
//   and every other lane adds T_ik (mu_k_new - mu_k_old) to its sum.  No cross-lane reduction inside the solver.
// Determinism.  A placement's three numbers are a function of its two table entries and the molecules only: the lane
// that owns a pair or a site, and the order of every sum, depend on n1 and n2 alone.  Nothing is shared between placements,
// no workgroup waits for another, there are no atomics.  The grid form's means are summed in a fixed order (below).
//
// Geometry.  dimer_rotate_kernel fills one table per molecule, one entry per rotation, from the body frame (coordinates
// minus the mass-weighted centre, pairs.c:364-385) in the operation order of surface_dimer_geometry() (surface.c:402-430)
// without FMA contraction: molecule 2 to (r, 0, 0), each molecule back to its centre, R times the vector left to right,
// and out again.  The rotation matrices are the host's.  The list form has one entry per placement in either table; the
// grid form K1 and K2 entries and the placements (k1, k2), k2 fastest: the reference's loop order (surface.c:306-311).
//
// The means of the grid form (dimer_mean_kernel), each of the three channels alike:
//   chunk c = placements [c kDimerChunk, (c + 1) kDimerChunk) cut at the count: b_c = the sum of its values in ascending
//   order, starting from 0.0;
//   d_t (t < kDimerMeanThreads) = the sum of b_t, b_{t + 256}, b_{t + 512}, ... in ascending order, starting from 0.0;
//   for off = 128, 64, ..., 1: d_t += d_{t + off} for every t < off;  mean = d_0 / count.
#pragma once
#include "kernels_disp.h"
#include "kernels_polar.h"
#include "kernels_rdforms.h"

namespace mpmc {

constexpr int kDimerMolSites = 16;                                     // the ABI's molecule limit
constexpr int kDimerSites = 2 * kDimerMolSites;
constexpr int kDimerPairs = kDimerSites * (kDimerSites - 1) / 2;       // 496
constexpr int kDimerChunk = 256;                                       // placements per workgroup (MPMC_HIP_DIMER_CHUNK)
constexpr int kDimerMeanThreads = 256;
constexpr int kDimerNotConverged = 0x40000000;                         // status bit (MPMC_HIP_DIMER_NOT_CONVERGED)
constexpr int kDimerTabStride = 3 * kDimerMolSites;                    // doubles per table entry

struct DimerMol {  // body frame and per-site parameters; entries n .. 15 are zeros
    double bx[kDimerMolSites], by[kDimerMolSites], bz[kDimerMolSites];
    double q[kDimerMolSites], alpha[kDimerMolSites], eps[kDimerMolSites], sig[kDimerMolSites];
    double c6[kDimerMolSites], c8[kDimerMolSites], c10[kDimerMolSites];
    int n, pad;
};
struct DimerMols {
    DimerMol m[2];
};

struct DimerParams {
    int disp;          // disp_expansion instead of Lennard-Jones
    int mixing;        // RdMix (Lennard-Jones)
    DispParams dp;
    int rd_only;
    int polar;         // solve the Thole system (the host clears it under rd_only and when no site is polarizable)
    int max_iter;      // polar_max_iter (precision == 0)
    double precision;  // polar_precision (Debye); 0 = fixed count
    int gs;            // polar_gs or polar_gs_ranked
    int ranked;        // polar_gs_ranked
    int palmo;
    double gamma;      // polar_gamma
};

// where the launch reads its placements and leaves its results
struct DimerLaunch {
    const double *tab1, *tab2;  // rotated sites [K][16][3]
    int K2;                     // grid form: placement p = (p / K2, p % K2); 0 = list form: (p, p)
    long long count;
    double *es, *rd, *polar;    // list form [count]
    int *status;                // list form [count]
    double *mu;                 // list form, optional [count][32][3]
    double *partials;           // grid form [3][nchunk]
    int *failed;                // grid form [nchunk]: placements of the chunk whose solve did not converge
};

// One table: entry k, site s of molecule `which` (0 / 1).  rlist: the separation per entry (list form) or nullptr (r).
__global__ __launch_bounds__(64) void dimer_rotate_kernel(const DimerMols *__restrict__ dm, int which, int K,
                                                          const double *__restrict__ R, const double *__restrict__ rlist,
                                                          double r, double *__restrict__ tab) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long k = t / kDimerMolSites;
    const int s = (int)(t % kDimerMolSites);
    if (k >= K) return;
    const DimerMol &m = dm->m[which];
    double *o = tab + (size_t)k * kDimerTabStride + 3 * s;
    if (s >= m.n) {
        o[0] = o[1] = o[2] = 0.0;
        return;
    }
    const double cx = which ? (rlist ? rlist[k] : r) : 0.0;  // the molecule's centre: (cx, 0, 0)
    // surface.c:402-421: both molecules at the origin, then the second one out along x
    double x = m.bx[s] + cx, y = m.by[s] + 0.0, z = m.bz[s] + 0.0;
    // molecule_rotate_euler / _quaternion: to the centre, rotate, back (surface.c:110-145)
    x = x - cx;
    y = y - 0.0;
    z = z - 0.0;
    const double *Rk = R + 9 * (size_t)k;
    double nx = Rk[0] * x;
    nx = nx + Rk[1] * y;
    nx = nx + Rk[2] * z;
    double ny = Rk[3] * x;
    ny = ny + Rk[4] * y;
    ny = ny + Rk[5] * z;
    double nz = Rk[6] * x;
    nz = nz + Rk[7] * y;
    nz = nz + Rk[8] * z;
    o[0] = nx + cx;
    o[1] = ny + 0.0;
    o[2] = nz + 0.0;
}

// pair->r of the reference (pairs.c:269-273)
__device__ __forceinline__ double dimer_distance(double dx, double dy, double dz) {
#pragma clang fp contract(off)
    double r2 = dx * dx;
    r2 = r2 + dy * dy;
    r2 = r2 + dz * dz;
    return sqrt(r2);
}

// slot of the unordered pair {i, k}, i != k, in the triangular coefficient store
__device__ __forceinline__ int dimer_tri(int i, int k) {
    const int a = min(i, k), b = max(i, k);
    return b * (b - 1) / 2 + a;
}

struct DimerShared {
    double q[kDimerSites], alpha[kDimerSites], eps[kDimerSites], sig[kDimerSites];
    double c6[kDimerSites], c8[kDimerSites], c10[kDimerSites];
    double x[kDimerSites], y[kDimerSites], z[kDimerSites];
    double vx[kDimerSites], vy[kDimerSites], vz[kDimerSites];  // the dipoles (Jacobi pass) / the step's change (Gauss-Seidel)
    double metric[kDimerSites];
    double2 c[kDimerPairs];  // {c3, c5}
    int order[kDimerSites];
};

// G += T_ik v for the lane's site at (xi, yi, zi) and site k: T = c3 I - 3 c5 d d^T (thole_matrix.c:123-135)
__device__ __forceinline__ void dimer_apply(const DimerShared &s, int i, int k, double xi, double yi, double zi, double vx,
                                            double vy, double vz, double &gx, double &gy, double &gz) {
    const double2 c = s.c[dimer_tri(i, k)];
    const double dx = xi - s.x[k], dy = yi - s.y[k], dz = zi - s.z[k];
    const double t = -3.0 * c.y * (dx * vx + dy * vy + dz * vz);
    gx += c.x * vx + t * dx;
    gy += c.x * vy + t * dy;
    gz += c.x * vz + t * dz;
}

// The zero-volume cell of a surf input (pbc.c:19, :47-63): zero basis, 0 / 0 reciprocal basis, cutoff MAXVALUE.  Built in
// the kernel from constants, so that the compiler folds minimum_image() down to its isnan branch.
__device__ __forceinline__ DevBox dimer_box() {
    DevBox bx = {};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) bx.rb[i][j] = __builtin_nan("");
    bx.cutoff = kMAXVALUE;
    return bx;
}

// grid = (number of chunks), block = 64.  MODEL: kTholeExp, kTholeLinear or kTholeOff.
template <int MODEL>
__global__ __launch_bounds__(64) void dimer_energy_kernel(const DimerMols *__restrict__ dm, DimerParams P, TholeParams tp,
                                                          DimerLaunch L) {
    __shared__ DimerShared s;
    const DevBox bx = dimer_box();
    const int lane = threadIdx.x;
    const int n1 = dm->m[0].n, n2 = dm->m[1].n, N = n1 + n2;
    const bool site = lane < N;
    const int mol = lane < n1 ? 0 : 1, sidx = lane < n1 ? lane : lane - n1;
    if (lane < kDimerSites) {
        const DimerMol &m = dm->m[mol];
        s.q[lane] = site ? m.q[sidx] : 0.0;
        s.alpha[lane] = site ? m.alpha[sidx] : 0.0;
        s.eps[lane] = site ? m.eps[sidx] : 0.0;
        s.sig[lane] = site ? m.sig[sidx] : 0.0;
        s.c6[lane] = site ? m.c6[sidx] : 0.0;
        s.c8[lane] = site ? m.c8[sidx] : 0.0;
        s.c10[lane] = site ? m.c10[sidx] : 0.0;
    }
    const int npairs = N * (N - 1) / 2;
    __syncthreads();
    const double alpha_i = site ? s.alpha[lane] : 0.0;
    RdFormParams fp;
    fp.mixing = P.mixing;
    fp.fh = 0;  // lj_nopbc has no Feynman-Hibbs term
    fp.fh_order = 2;
    fp.temperature = 0.0;

    const long long p0 = (long long)blockIdx.x * kDimerChunk;
    const long long p1 = (p0 + kDimerChunk < L.count) ? p0 + kDimerChunk : L.count;
    double sum_es = 0.0, sum_rd = 0.0, sum_pol = 0.0;
    int sum_failed = 0;
    for (long long p = p0; p < p1; ++p) {
        const long long k1 = L.K2 ? p / L.K2 : p, k2 = L.K2 ? p % L.K2 : p;
        double xi = 0.0, yi = 0.0, zi = 0.0;
        __syncthreads();  // (the previous placement's readers of s.x / s.c are done)
        if (site) {
            const double *src = (mol ? L.tab2 + (size_t)k2 * kDimerTabStride : L.tab1 + (size_t)k1 * kDimerTabStride) + 3 * sidx;
            xi = src[0];
            yi = src[1];
            zi = src[2];
        }
        if (lane < kDimerSites) {
            s.x[lane] = xi;
            s.y[lane] = yi;
            s.z[lane] = zi;
        }
        __syncthreads();

        // ---- es and rd over the n1 n2 inter-molecular pairs, i on molecule 1 (the reference's pair: atom i, pair atom j) ----
        double es = 0.0, rd = 0.0;
        for (int pr = lane; pr < n1 * n2; pr += kWave) {
            const int i = pr / n2, j = n1 + pr % n2;
            const double r = dimer_distance(s.x[i] - s.x[j], s.y[i] - s.y[j], s.z[i] - s.z[j]);
            const double qi = s.q[i], qj = s.q[j];
            if (!P.rd_only && qi != 0.0 && qj != 0.0) es += qi * qj / r;  // !es_excluded (pairs.c:74)
            const double epsi = s.eps[i], sigi = s.sig[i], epsj = s.eps[j], sigj = s.sig[j];
            const bool null_rd = (epsi == 0.0 || sigi == 0.0 || epsj == 0.0 || sigj == 0.0);
            if (P.disp) {
                const double c6i = s.c6[i], c8i = s.c8[i], c10i = s.c10[i], c6j = s.c6[j], c8j = s.c8[j], c10j = s.c10[j];
                // rd_excluded: null repulsion AND null dispersion (pairs.c:68)
                if (null_rd && c6i == 0.0 && c8i == 0.0 && c10i == 0.0 && c6j == 0.0 && c8j == 0.0 && c10j == 0.0) continue;
                rd += disp_pair_energy(P.dp, epsi, sigi, c6i, c8i, c10i, epsj, sigj, c6j, c8j, c10j, r);
            } else {
                if (null_rd) continue;  // (c6 / c8 / c10 are not read in this mode: the ABI passes them under disp_expansion)
                double sig, eps;
                bool attractive;
                rdform_mix(P.mixing, epsi, sigi, epsj, sigj, sig, eps, attractive);
                rd += rdform_lj(r, sig, eps, attractive, fp, 1.0, 1.0);
            }
        }
        es = wave_sum(es);
        rd = wave_sum(rd);

        // ---- polarization ----
        double pol = 0.0;
        int status = 0;
        double mx = 0.0, my = 0.0, mz = 0.0;
        if (P.polar) {
            // A matrix coefficients of every pair, and the smallest distance between two polarizable sites (pairs.c:339-346)
            double rmin = kMAXVALUE;
#pragma unroll 1
            for (int pr = lane; pr < npairs; pr += kWave) {
                {
                    // the pair {a < b} with b (b - 1) / 2 + a = pr
                    int b = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)pr)) * 0.5f);
                    while (b * (b - 1) / 2 > pr) --b;
                    while ((b + 1) * b / 2 <= pr) ++b;
                    const int a = pr - b * (b - 1) / 2;
                    const double aa = (MODEL == kTholeLinear) ? s.alpha[a] * s.alpha[b] : 0.0;
                    const bool same = (a < n1) == (b < n1);
                    const bool excl = (MODEL == kTholeOff) ? (same || s.q[a] == 0.0 || s.q[b] == 0.0) : false;
                    double c3, c5, dx, dy, dz;
                    thole_coef<MODEL>(bx, tp, aa, excl, s.x[a] - s.x[b], s.y[a] - s.y[b], s.z[a] - s.z[b], c3, c5, dx, dy, dz);
                    s.c[pr] = make_double2(c3, c5);
                    if (P.ranked && s.alpha[a] != 0.0 && s.alpha[b] != 0.0)
                        rmin = fmin(rmin, dimer_distance(dx, dy, dz));
                }
            }
            // static field: the other molecule's sites in ascending order (thole_field.c:46-59)
            double ex = 0.0, ey = 0.0, ez = 0.0;
            if (site) {
#pragma clang fp contract(off)
                const int j0 = mol ? 0 : n1, j1 = mol ? n1 : N;
                for (int j = j0; j < j1; ++j) {
                    const double dx = xi - s.x[j], dy = yi - s.y[j], dz = zi - s.z[j];
                    const double r = dimer_distance(dx, dy, dz);
                    if (r != 0.0) {
                        const double r3 = r * r * r, qj = s.q[j];
                        ex = ex + qj * dx / r3;
                        ey = ey + qj * dy / r3;
                        ez = ez + qj * dz / r3;
                    }
                }
            }
            // the ranked order (pairs.c:347-359, update_ranking()): metric = pairs of polarizable sites within 1.5 rmin
            if (lane < kDimerSites) s.order[lane] = lane;
            bool use_ranked = false;
            if (P.ranked) {
                rmin = wave_min(rmin);
                double metric = 0.0;
                if (site && alpha_i != 0.0) {
                    for (int j = 0; j < N; ++j) {
                        if (j == lane || s.alpha[j] == 0.0) continue;
                        if (dimer_distance(xi - s.x[j], yi - s.y[j], zi - s.z[j]) <= rmin * 1.5) metric += 1.0;
                    }
                }
                if (lane < kDimerSites) s.metric[lane] = metric;
            }
            __syncthreads();

            // init_dipoles(): alpha E gamma
            mx = alpha_i * ex * P.gamma;
            my = alpha_i * ey * P.gamma;
            mz = alpha_i * ez * P.gamma;
            const double allowed = P.precision * P.precision * kDEBYE2SKA * kDEBYE2SKA;
            double chx = 0.0, chy = 0.0, chz = 0.0;  // ef_induced_change
            int iter = 0;
            bool keep = true, failed = false;
            while (keep) {
                ++iter;
                if (iter >= kMAX_ITERATION_COUNT && P.precision != 0.0) {  // thole_iterative.c:199-210
                    mx = alpha_i * ex;
                    my = alpha_i * ey;
                    mz = alpha_i * ez;
                    chx = chy = chz = 0.0;
                    failed = true;
                    break;
                }
                const double ox = mx, oy = my, oz = mz;
                // contract_dipoles(): G = sum_{k != i} T_ik mu_k over the dipoles as they stand
                if (lane < kDimerSites) {
                    s.vx[lane] = mx;
                    s.vy[lane] = my;
                    s.vz[lane] = mz;
                }
                __syncthreads();
                double gx = 0.0, gy = 0.0, gz = 0.0;
                for (int k = 0; k < N; ++k) {
                    if (s.alpha[k] == 0.0) continue;  // (its dipole is 0)
                    if (site && k != lane) dimer_apply(s, lane, k, xi, yi, zi, s.vx[k], s.vy[k], s.vz[k], gx, gy, gz);
                }
                double ux = gx, uy = gy, uz = gz;  // the sum the site's new dipole is formed from (-ef_induced)
                if (!P.gs) {
                    mx = alpha_i * (ex - gx);
                    my = alpha_i * (ey - gy);
                    mz = alpha_i * (ez - gz);
                } else {
                    for (int t = 0; t < N; ++t) {
                        const int k = s.order[t];
                        if (s.alpha[k] == 0.0) continue;  // thole_iterative.c:34-39
                        __syncthreads();
                        if (lane == k) {
                            ux = gx;
                            uy = gy;
                            uz = gz;
                            const double nx = alpha_i * (ex - gx), ny = alpha_i * (ey - gy), nz = alpha_i * (ez - gz);
                            s.vx[k] = nx - mx;
                            s.vy[k] = ny - my;
                            s.vz[k] = nz - mz;
                            mx = nx;
                            my = ny;
                            mz = nz;
                        }
                        __syncthreads();
                        if (site && lane != k) dimer_apply(s, lane, k, xi, yi, zi, s.vx[k], s.vy[k], s.vz[k], gx, gy, gz);
                    }
                }
                // are_we_done_yet()
                if (P.precision == 0.0) {
                    keep = (iter < P.max_iter);  // (the host passes polar_max_iter >= 1: the reference's `!=`)
                } else {
                    const double dx = mx - ox, dy = my - oy, dz = mz - oz;
                    keep = __any((dx * dx > allowed) || (dy * dy > allowed) || (dz * dz > allowed));
                }
                if (P.palmo && !keep) {  // palmo_contraction(): the field change a further contraction would see
                    chx = ux - gx;       // (Jacobi: the dipoles it runs on are still the old ones: 0)
                    chy = uy - gy;
                    chz = uz - gz;
                }
                if (P.ranked && keep && !use_ranked) {  // update_ranking(): stable, descending
                    use_ranked = true;
                    __syncthreads();
                    if (site) {
                        const double mi = s.metric[lane];
                        int pos = 0;
                        for (int j = 0; j < N; ++j) pos += (s.metric[j] > mi) || (s.metric[j] == mi && j < lane);
                        s.order[pos] = lane;
                    }
                    __syncthreads();
                }
            }
            double u = mx * ex + my * ey + mz * ez;
            if (P.palmo) u += mx * chx + my * chy + mz * chz;
            pol = -0.5 * wave_sum(u);
            status = iter | (failed ? kDimerNotConverged : 0);
            sum_failed += failed ? 1 : 0;
        }

        if (L.partials) {
            sum_es += es;
            sum_rd += rd;
            sum_pol += pol;
        } else {
            if (lane == 0) {
                L.es[p] = es;
                L.rd[p] = rd;
                L.polar[p] = pol;
                L.status[p] = status;
            }
            if (L.mu && lane < kDimerSites) {
                double *o = L.mu + ((size_t)p * kDimerSites + lane) * 3;
                o[0] = mx;
                o[1] = my;
                o[2] = mz;
            }
        }
    }
    if (L.partials && lane == 0) {
        const size_t nchunk = gridDim.x;
        L.partials[blockIdx.x] = sum_es;
        L.partials[nchunk + blockIdx.x] = sum_rd;
        L.partials[2 * nchunk + blockIdx.x] = sum_pol;
        L.failed[blockIdx.x] = sum_failed;
    }
}

// The three means and the count of non-converged placements from the chunk sums, in the order the head of this file states.
// grid = 1, block = kDimerMeanThreads.  out: [3] means; nfailed: [1].
__global__ __launch_bounds__(kDimerMeanThreads) void dimer_mean_kernel(const double *__restrict__ partials,
                                                                        const int *__restrict__ failed, int nchunk,
                                                                        long long count, double *__restrict__ out,
                                                                        long long *__restrict__ nfailed) {
    __shared__ double d[3][kDimerMeanThreads];
    __shared__ long long f[kDimerMeanThreads];
    const int t = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    long long nf = 0;
    for (int c = t; c < nchunk; c += kDimerMeanThreads) {
        a0 += partials[c];
        a1 += partials[(size_t)nchunk + c];
        a2 += partials[2 * (size_t)nchunk + c];
        nf += failed[c];
    }
    d[0][t] = a0;
    d[1][t] = a1;
    d[2][t] = a2;
    f[t] = nf;
    __syncthreads();
    for (int off = kDimerMeanThreads / 2; off > 0; off >>= 1) {
        if (t < off) {
            d[0][t] += d[0][t + off];
            d[1][t] += d[1][t + off];
            d[2][t] += d[2][t + off];
            f[t] += f[t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = d[0][0] / (double)count;
        out[1] = d[1][0] / (double)count;
        out[2] = d[2][0] / (double)count;
        nfailed[0] = f[0];
    }
}

}  // namespace mpmc
