// kernels_trial.h -- trial placements of ONE molecule against the resident configuration (mpmc_hip_trial_energies,
// DESIGN.md section 19): the part of the standard pair path's energy that a rigid re-placement of a molecule changes,
// for K placements in one batch.  What the reference's quantum_rotation scan (rotational_eigenspectrum.c:219-266) gets
// from 2 x 256 full energy() calls per molecule.
//
//   E_t = E_resident - (pair_m + recip)(current placement) + (pair_m + recip)(trial t)
//
// pair_m: Lennard-Jones (+ Feynman-Hibbs) and the real-space Ewald / Wolf term of the molecule's sites with every other
// valid atom -- the pair terms of pair_rd_es_body (kernels_pair.h) restated statement by statement, with its decisions,
// WITHOUT its fp32 screen (a screen only drops pairs the exact path would drop) -- and recip: w_k |S_rest(k) + s_t(k)|^2
// over the k list, S_rest = the resident block partial structure factors summed, minus the molecule's own share.  The
// long-range correction, the self term and the molecule's intra-molecular sums do not change under a rigid re-placement.
//
//   trial_pair_kernel          grid = ntrial + 1; workgroup b evaluates placement b - 1 (b = 0: the CURRENT placement, read
//                              from the resident coordinates, so that the subtraction pairs like with like); the sites
//                              sit in LDS, thread k takes the resident atoms k, k + 256, ...; wave butterflies, then the
//                              waves in order.
//   trial_recip_prepare_kernel grid = ceil(nk / 64); S_rest(k), once per call.
//   trial_recip_kernel         grid = (ceil(nk / 64), ntrial + 1); lane = k-vector; one chunk sum per workgroup.
//   trial_assemble_kernel      thread = trial: adds the chunk sums in order and forms E_t and the three terms.
// No atomics, no workgroup waits for another, every sum in an order the sizes fix: a placement's bits depend on the
// molecule, the placement and the resident configuration, not on ntrial or on the placement's position in the batch.
// None of these kernels writes anything the rest of the engine reads.
#pragma once
#include "kernels_pair.h"

namespace mpmc {

constexpr int kTrialSites = 16;  // sites of the molecule (kMaxEdit: what insert_molecule takes)
constexpr int kTrialWaves = 4;

struct TrialMol {
    int first, count;   // the molecule's slots
    const double *xyz;  // [ntrial][count][3]
};

// the sites of placement t (t < 0: the resident coordinates) and their parameters -> LDS; threads 0 .. count - 1
__device__ __forceinline__ void trial_load_site(const DevAtoms &a, const TrialMol &tm, int t, int s, double &x, double &y,
                                                double &z) {
    if (t < 0) {
        x = a.x[tm.first + s];
        y = a.y[tm.first + s];
        z = a.z[tm.first + s];
    } else {
        const double *p = tm.xyz + ((size_t)t * tm.count + s) * 3;
        x = p[0];
        y = p[1];
        z = p[2];
    }
}

template <int FH>
__global__ __launch_bounds__(64 * kTrialWaves) void trial_pair_kernel(DevAtoms a, DevBox bx, PairParams pp, TrialMol tm,
                                                                       double *__restrict__ out /* [ntrial + 1][2] */) {
    const int t = (int)blockIdx.x - 1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ double sx[kTrialSites], sy[kTrialSites], sz[kTrialSites], sq[kTrialSites], seps[kTrialSites],
        ssig[kTrialSites], smm[kTrialSites];
    __shared__ double red[kTrialWaves][2];
    if ((int)threadIdx.x < tm.count) {
        const int s = threadIdx.x;
        trial_load_site(a, tm, t, s, sx[s], sy[s], sz[s]);
        sq[s] = a.q[tm.first + s];
        seps[s] = a.eps[tm.first + s];
        ssig[s] = a.sig[tm.first + s];
        smm[s] = a.molmass[tm.first + s];
    }
    __syncthreads();

    const double rc = bx.cutoff;
    const double rc2_hi = cutoff_prefilter_sq(rc);
    const double alpha = pp.ewald_alpha;
    double e_rd = 0.0, e_es = 0.0;
    for (int j = threadIdx.x; j < a.n; j += 64 * kTrialWaves) {
        if (j >= tm.first && j < tm.first + tm.count) continue;  // the molecule's own slots
        if (!(a.flags[j] & kValid)) continue;                     // a hole; a frozen partner counts (the molecule is not)
        const double xj = a.x[j], yj = a.y[j], zj = a.z[j];
        const double epsj = a.eps[j], sigj = a.sig[j], qj = a.q[j], mj = a.molmass[j];
        for (int s = 0; s < tm.count; ++s) {
            const double xi = sx[s], yi = sy[s], zi = sz[s];
            const double qi = sq[s], epsi = seps[s], sigi = ssig[s], mmi = smm[s];
            double r2, ri2, dx, dy, dz;
            minimum_image_sq(bx, xi - xj, yi - yj, zi - zj, r2, ri2, dx, dy, dz);
            if (!(ri2 <= rc2_hi)) continue;  // superset of every cutoff test below
            const double rimg = sqrt(ri2);

            // ---- repulsion/dispersion: lj.c:189-250, mixing pairs.c:200-211 (Lorentz-Berthelot)
            const bool rd_excl = epsi == 0.0 || sigi == 0.0 || epsj == 0.0 || sigj == 0.0;
            if (!rd_excl && !(sigi < 0.0 || sigj < 0.0) && (rimg - kSMALL_dR < rc)) {
                const double sig = 0.5 * (sigi + sigj);
                const double eps = sqrt(epsi * epsj);
                double sor = fabs(sig) / rimg;
                double s6 = sor * sor * sor;
                s6 *= s6;
                const double s12 = s6 * s6;
                double e = 4.0 * eps * (s12 - s6);
                if (FH) {  // lj_fh_corr, lj.c:11-54
                    const double ir = 1.0 / rimg, ir2 = ir * ir, ir3 = ir2 * ir, ir4 = ir3 * ir;
                    const double rm = kAMU2KG * mmi * mj / (mmi + mj);
                    const double dE = -24.0 * eps * (2.0 * s12 - s6) * ir;
                    const double d2E = 24.0 * eps * (26.0 * s12 - 7.0 * s6) * ir2;
                    double corr = kM2A2 * (kHBAR2 / (24.0 * kKB * pp.temperature * rm)) * (d2E + 2.0 * dE / rimg);
                    if (FH >= 4) {
                        const double d3E = -1344.0 * eps * (6.0 * s12 - s6) * ir3;
                        const double d4E = 12096.0 * eps * (10.0 * s12 - s6) * ir4;
                        corr += kM2A4 * (kHBAR4 / (1152.0 * kKB2 * pp.temperature * pp.temperature * rm * rm)) *
                                (15.0 * dE * ir3 + 4.0 * d3E * ir + d4E);
                    }
                    e += corr;
                }
                e_rd += e;
            }

            // ---- electrostatics: Wolf (coulombic.c:269-308) or the real-space Ewald term (coulombic.c:149-194)
            if (!pp.rd_only && pp.wolf) {
                const bool es_excl = qi == 0.0 || qj == 0.0;
                if (!es_excl && (rimg < rc)) {
                    const double iR = 1.0 / rc;
                    e_es += qi * qj * (1.0 / rimg - pp.erfaRoverR - iR * iR * (rc - rimg));
                }
            } else if (!pp.rd_only) {
                const bool es_excl = qi == 0.0 || qj == 0.0;
                if (!es_excl && !(rimg > rc)) {
                    const double erfc_term = erfc(alpha * rimg);
                    double e = qi * qj * erfc_term / rimg;
                    if (FH) {  // coulombic_real_FH, coulombic.c:115-146 (added WITHOUT q_i q_j, as the reference does)
                        const double gaussian_term = exp(-alpha * alpha * rimg * rimg);
                        const double rr = rimg * rimg;
                        const double ir = 1.0 / rimg, ir2 = ir * ir, ir3 = ir * ir2, ir4 = ir2 * ir2;
                        const double a2 = alpha * alpha, a3 = a2 * alpha, a4 = a3 * alpha;
                        const double rm = kAMU2KG * mmi * mj / (mmi + mj);
                        const double sqrtpi = sqrt(kPI);
                        const double du = -2.0 * alpha * gaussian_term / (rimg * sqrtpi) - erfc_term * ir2;
                        const double d2u = (4.0 / sqrtpi) * gaussian_term * (a3 + 1.0 * ir2) + 2.0 * erfc_term * ir3;
                        double fh = kM2A2 * (kHBAR2 / (24.0 * kKB * pp.temperature * rm)) * (d2u + 2.0 * du / rimg);
                        if (FH >= 4) {
                            const double d3u =
                                (gaussian_term / sqrtpi) * (-8.0 * (a3 * a2) * rimg - 8.0 * a3 / rimg - 12.0 * alpha * ir3) -
                                6.0 * erfc_term * ir4;
                            const double d4u = (gaussian_term / sqrtpi) *
                                                   (8.0 * a3 * a2 + 16.0 * a3 * a4 * rr + 32.0 * a3 * ir2 + 48.0 * ir4) +
                                               24.0 * erfc_term * (ir4 * ir);
                            fh += kM2A4 *
                                  (kHBAR4 / (1152.0 * (kKB * kKB * pp.temperature * pp.temperature * rm * rm))) *
                                  (15.0 * du * ir3 + 4.0 * d3u / rimg + d4u);
                        }
                        e += fh;
                    }
                    e_es += e;
                }
            }
        }
    }

    e_rd = wave_sum(e_rd);
    e_es = wave_sum(e_es);
    if (lane == 0) {
        red[wv][0] = e_rd;
        red[wv][1] = e_es;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kTrialWaves; ++k) s += red[k][threadIdx.x];
        out[(size_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

// S_rest(k) = sum_b S_b(k) - s_m(k): the resident block partials (recip_partial_body) added up -- group g the blocks
// g, g + 4, ... in increasing order, then the groups in order -- minus the molecule's share at its resident coordinates.
constexpr int kTrialPrepGroups = 4;
__global__ __launch_bounds__(64 * kTrialPrepGroups) void trial_recip_prepare_kernel(DevAtoms a, const KVec *__restrict__ kv,
                                                                                    int nk, int nblocks,
                                                                                    const double2 *__restrict__ part,
                                                                                    TrialMol tm,
                                                                                    double2 *__restrict__ srest) {
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int k = blockIdx.x * kWave + lane;
    __shared__ double2 red[kTrialPrepGroups][kWave];
    double re = 0.0, im = 0.0;
    if (k < nk) {
        for (int b = g; b < nblocks; b += kTrialPrepGroups) {
            const double2 p = part[(size_t)b * nk + k];
            re += p.x;
            im += p.y;
        }
    }
    red[g][lane] = make_double2(re, im);
    __syncthreads();
    if (g != 0 || k >= nk) return;
    double r = 0.0, i = 0.0;
#pragma unroll
    for (int u = 0; u < kTrialPrepGroups; ++u) {
        r += red[u][lane].x;
        i += red[u][lane].y;
    }
    const KVec v = kv[k];
    double mr = 0.0, mi = 0.0;
    for (int s = 0; s < tm.count; ++s) {
        const double q = a.q[tm.first + s];
        if (q == 0.0) continue;  // wave-uniform
        double sn, cs;
        sincos(v.kx * a.x[tm.first + s] + v.ky * a.y[tm.first + s] + v.kz * a.z[tm.first + s], &sn, &cs);
        mr += q * cs;
        mi += q * sn;
    }
    srest[k] = make_double2(r - mr, i - mi);
}

// chunk[b][c] = sum over the 64 k-vectors of chunk c of w_k |S_rest(k) + s_t(k)|^2, placement t = b - 1
__global__ __launch_bounds__(64) void trial_recip_kernel(DevAtoms a, const KVec *__restrict__ kv, int nk,
                                                         const double2 *__restrict__ srest, TrialMol tm,
                                                         double *__restrict__ chunk /* [ntrial + 1][gridDim.x] */) {
    const int t = (int)blockIdx.y - 1;
    const int lane = threadIdx.x;
    __shared__ double sx[kTrialSites], sy[kTrialSites], sz[kTrialSites], sq[kTrialSites];
    if (lane < tm.count) {
        trial_load_site(a, tm, t, lane, sx[lane], sy[lane], sz[lane]);
        sq[lane] = a.q[tm.first + lane];
    }
    __syncthreads();
    const int k = blockIdx.x * kWave + lane;
    const KVec v = kv[min(k, nk - 1)];
    const double2 rest = srest[min(k, nk - 1)];
    double re = 0.0, im = 0.0;
    for (int s = 0; s < tm.count; ++s) {
        const double q = sq[s];
        if (q == 0.0) continue;  // wave-uniform
        double sn, cs;
        sincos(v.kx * sx[s] + v.ky * sy[s] + v.kz * sz[s], &sn, &cs);
        re += q * cs;
        im += q * sn;
    }
    const double r = rest.x + re, i = rest.y + im;
    double e = (k < nk) ? v.w * (r * r + i * i) : 0.0;
    e = wave_sum(e);
    if (lane == 0) chunk[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = e;
}

// energy[t] = (e_resident - ((rd_0 + es_0) + recip_0)) + ((rd_t + es_t) + recip_t), index 0 = the current placement;
// recip = (the chunk sums added in order) * recip_scale (4 pi / V, coulombic.c:92); terms[t] = rd_t, es_t, recip_t.
__global__ __launch_bounds__(256) void trial_assemble_kernel(const double *__restrict__ pair, const double *__restrict__ chunk,
                                                             int nchunk, int ntrial, double e_resident, double recip_scale,
                                                             double *__restrict__ energy, double *__restrict__ terms) {
#pragma clang fp contract(off)  // (the stated order, one rounding per operation: callers may restate it)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntrial) return;
    double c0 = 0.0, ct = 0.0;
    for (int c = 0; c < nchunk; ++c) {
        c0 += chunk[c];
        ct += chunk[(size_t)(t + 1) * nchunk + c];
    }
    const double recip0 = c0 * recip_scale, recipt = ct * recip_scale;
    const double rd0 = pair[0], es0 = pair[1];
    const double rdt = pair[2 * (size_t)(t + 1)], est = pair[2 * (size_t)(t + 1) + 1];
    const double base = e_resident - ((rd0 + es0) + recip0);
    energy[t] = base + ((rdt + est) + recipt);
    terms[3 * (size_t)t] = rdt;
    terms[3 * (size_t)t + 1] = est;
    terms[3 * (size_t)t + 2] = recipt;
}

}  // namespace mpmc
