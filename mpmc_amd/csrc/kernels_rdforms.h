// kernels_rdforms.h -- the pair potentials of energy() beside plain Lennard-Jones (mpmc_hip_set_rd_form): Silvera-Goldman
// (reference src/energy/sg.c:13-91), DREIDING exp-6 (dreiding.c:13-108), Halgren's buffered 14-7
// (lj_buffered_14_7.c:6-35), and Lennard-Jones itself (lj.c:165-276 without rd_crystal) so that the mixing rules of
// pairs.c:84-211 -- Lorentz-Berthelot, Waldman-Hagler, Halgren, C6 -- reach it.
//
// What the reference sums, and this file therefore sums (r = rimg of the minimum image; sigma_ij, eps_ij the mixed values):
//   * SG: every unordered pair with rimg < cutoff (strict).  No rd_excluded test and no parameter test: same-molecule
//     pairs take part, per-atom eps / sigma are not read.  In Bohr, x = rimg / 0.529177249:
//       U = exp(ALPHA - BETA x - GAMMA x^2) - (C6/x^6 + C8/x^8 + C10/x^10 - C9/x^9) f,  f = exp(-(RM/x - 1)^2) for x < RM, else 1.
//     Under feynman_hibbs the second-order term exactly as sg.c:56-72 writes it, whatever feynman_hibbs_order says: the
//     110 C10 / x^10 of the second derivative (not x^12), the mass of the molecule of the pair's FIRST atom (no reduced
//     mass), and the METER2ANGSTROM^2 prefactor on derivatives taken in Bohr.  The pair's sum times HARTREE2KELVIN.
//     OWNED DEVIATION: frozen-frozen pairs are left out.  The reference never computes their distance without
//     polarization (pairs.c:324) and sums what the memory held; the host layer refuses sg with two or more frozen atoms.
//   * DREIDING (gamma = 12): pairs with !(rimg > cutoff || rd_excluded || frozen-frozen) -- a pair exactly at the cutoff
//     counts -- eps_ij (t_exp - (gamma / (gamma - 6)) (r / sigma_ij)^-6), t_exp = 0 for an attractive-only pair, 1e40 for
//     rimg < 0.4 sigma_ij, else (6 / (gamma - 6)) exp(gamma (1 - r / sigma_ij)).  No Feynman-Hibbs term, no long-range
//     correction: the reference has neither.
//   * BUFFERED_14_7: the same pairs; eps_ij (1.07 / (rho + 0.07))^7 (1.12 / (rho^7 + 0.12) - 2), rho = r / sigma_ij.
//     attractive_only is ignored.  No Feynman-Hibbs term, no long-range correction.
//   * LJ: pairs with rimg - 1e-12 < cutoff, not rd_excluded, not frozen-frozen; 4 eps_ij (t12 - t6), t12 = 0 for an
//     attractive-only pair; lj_fh_corr at order 2 or 4 with the reduced molecular mass; under rd_lrc the pair correction
//     with the MIXED eps_ij / sigma_ij and the self correction with the atom's own values (rdform_lrc_kernel).
//   rd_excluded is pairs.c:61-71 as the Lennard-Jones path has it: same molecule, or one of the four eps / sigma is 0.  A
//   zero sigma_ij that survives it is followed literally: r / 0 = inf and the term is +-0.
// Mixing (rdform_mix): per pair from the per-atom eps, sigma of the upload.  An attractive-only pair (a sigma < 0 under
// Lorentz-Berthelot or Waldman-Hagler) has a pair epsilon the reference never assigns; it is 0 here, as on the
// Lennard-Jones path, and energy() refuses Waldman-Hagler with a negative sigma.
//
// Every comparison that decides something is formed in the reference's operation order without FMA contraction.
// DEVIATION from the literal expression, owned here: the integer powers are products (and one reciprocal) where the
// reference calls pow(); a term differs by ~1e-16 relative, four orders inside the tests' tolerance.
//
// One workgroup of 8 waves per 64 x 64 tile, J >= I, lane = row atom, each wave takes 8 of the 64 column atoms.  Dense:
// every pair's minimum image is formed, there is no candidate screen.  Tile ownership and the fixed-order sum are
// kernels_tile.h's.
#pragma once
#include "kernels_tile.h"

namespace mpmc {

enum RdForm : int { kRdFormOff = 0, kRdFormLJ = 1, kRdFormSG = 2, kRdFormDreiding = 3, kRdFormBuffered147 = 4 };
enum RdMix : int { kRdMixLB = 0, kRdMixWaldmanHagler = 1, kRdMixHalgren = 2, kRdMixC6 = 3 };

struct RdFormParams {
    int mixing;       // RdMix
    int fh;           // feynman_hibbs
    int fh_order;     // 2 or 4 (LJ form; SG is second order whatever this says)
    double temperature;
};

// reference src/include/defines.h:9, :25-44
constexpr double kSgAlpha = 1.713, kSgBeta = 1.5671, kSgGamma = 0.00993;
constexpr double kSgC6 = 12.14, kSgC8 = 215.2, kSgC10 = 4813.9, kSgC9 = 143.1, kSgRM = 8.321;
constexpr double kAU2ANGSTROM = 0.529177249;
constexpr double kHARTREE2KELVIN = 3.15774655e5;
constexpr double kHBAR = 1.054571e-34;
constexpr double kMETER2ANGSTROM = 1.0e10;
constexpr double kDreidingGamma = 12.0;

// pairs.c:84-211: sigma_ij, eps_ij and attractive_only of a pair
__device__ __forceinline__ void rdform_mix(int mixing, double epsi, double sigi, double epsj, double sigj, double &sig,
                                           double &eps, bool &attractive) {
#pragma clang fp contract(off)
    attractive = false;
    if (mixing == kRdMixWaldmanHagler) {  // :85-103
        double si3 = sigi;
        si3 *= si3 * si3;
        const double si6 = si3 * si3;
        double sj3 = sigj;
        sj3 *= sj3 * sj3;
        const double sj6 = sj3 * sj3;
        if (sigi < 0.0 || sigj < 0.0) {
            attractive = true;
            sig = pow(0.5 * (si6 + sj6), 1. / 6.);
            eps = 0.0;  // never assigned in the reference; energy() refuses the input
        } else if (sigi == 0.0 || sigj == 0.0) {
            sig = 0.0;
            eps = sqrt(epsi * epsj);
        } else {
            sig = pow(0.5 * (si6 + sj6), 1. / 6.);
            eps = sqrt(epsi * epsj) * 2.0 * si3 * sj3 / (si6 + sj6);
        }
    } else if (mixing == kRdMixHalgren) {  // :104-114
        if (sigi > 0.0 && sigj > 0.0)
            sig = (sigi * sigi * sigi + sigj * sigj * sigj) / (sigi * sigi + sigj * sigj);
        else
            sig = 0.0;
        if (epsi > 0.0 && epsj > 0.0) {
            const double s = sqrt(epsi) + sqrt(epsj);
            eps = 4 * epsi * epsj / (s * s);
        } else {
            eps = 0.0;
        }
    } else if (mixing == kRdMixC6) {  // :194-199
        sig = 0.5 * (sigi + sigj);
        if (sig != 0.0) {
            const double s = sigi + sigj, s2 = s * s;
            eps = 64.0 * sqrt(epsi * epsj) * (sigi * sigi * sigi) * (sigj * sigj * sigj) / (s2 * s2 * s2);
        } else {
            eps = 0.0;
        }
    } else {  // Lorentz-Berthelot, :200-211
        if (sigi < 0.0 || sigj < 0.0) {
            attractive = true;
            sig = 0.5 * (fabs(sigi) + fabs(sigj));
            eps = 0.0;  // never assigned for attractive-only pairs: 0, as on the Lennard-Jones path
        } else if (sigi == 0.0 || sigj == 0.0) {
            sig = 0.0;
            eps = sqrt(epsi * epsj);
        } else {
            sig = 0.5 * (sigi + sigj);
            eps = sqrt(epsi * epsj);
        }
    }
}

// sg.c:34-77 of one pair with rimg < cutoff; mass: of the molecule of the pair's first atom
__device__ __forceinline__ double rdform_sg(double rimg_angstrom, const RdFormParams &fp, double mass) {
#pragma clang fp contract(off)
    const double x = rimg_angstrom / kAU2ANGSTROM;
    const double repulsive = exp(kSgAlpha - kSgBeta * x - kSgGamma * x * x);
    const double ix = 1.0 / x, ix2 = ix * ix, ix4 = ix2 * ix2;
    const double ix6 = ix4 * ix2, ix8 = ix4 * ix4, ix9 = ix8 * ix, ix10 = ix8 * ix2;
    const double multipole = kSgC6 * ix6 + kSgC8 * ix8 + kSgC10 * ix10 - kSgC9 * ix9;
    const double r_rm = kSgRM / x;
    double damp = 1.0;
    if (x < kSgRM) damp = exp(-((r_rm - 1.0) * (r_rm - 1.0)));
    double e = repulsive - multipole * damp;
    if (fp.fh) {
        const double ix7 = ix6 * ix, ix11 = ix10 * ix;
        const double bg = kSgBeta + 2.0 * kSgGamma * x;
        double d1 = -bg * repulsive;
        d1 += (6.0 * kSgC6 * ix7 + 8.0 * kSgC8 * ix9 - 9.0 * kSgC9 * ix10 + 10.0 * kSgC10 * ix11) * damp;
        const double rd1 = (r_rm * r_rm - r_rm) / x;
        d1 += -2.0 * multipole * damp * rd1;
        double d2 = (bg * bg - 2.0 * kSgGamma) * repulsive;
        d2 += (-damp) * (42.0 * kSgC6 * ix8 + 72.0 * kSgC8 * ix10 - 90.0 * kSgC9 * ix11 + 110.0 * kSgC10 * ix10);  // (x^10: sg.c:65)
        d2 += damp * rd1 * (12.0 * kSgC6 * ix7 + 16.0 * kSgC8 * ix9 - 18.0 * kSgC9 * ix10 + 20.0 * kSgC10 * ix11);
        d2 += damp * (rd1 * rd1) * 4.0 * multipole;
        const double rd2 = (3.0 * r_rm * r_rm - 2.0 * r_rm) / (x * x);
        d2 += damp * rd2 * 2.0 * multipole;
        e += (kMETER2ANGSTROM * kMETER2ANGSTROM) * (kHBAR * kHBAR / (24.0 * kKB * fp.temperature * (kAMU2KG * mass))) *
             (d2 + 2.0 * d1 / x);
    }
    return e * kHARTREE2KELVIN;
}

// dreiding.c:36-52
__device__ __forceinline__ double rdform_dreiding(double rimg, double sig, double eps, bool attractive) {
#pragma clang fp contract(off)
    const double ros = rimg / sig;
    const double ros2 = ros * ros;
    const double term6 = (1.0 / (ros2 * ros2 * ros2)) * (kDreidingGamma / (kDreidingGamma - 6.0));
    double termexp = 0.0;
    if (!attractive) {
        if (rimg < 0.4 * sig)
            termexp = kMAXVALUE;
        else
            termexp = exp(kDreidingGamma * (1.0 - ros)) * (6.0 / (kDreidingGamma - 6.0));
    }
    return eps * (termexp - term6);
}

// lj_buffered_14_7.c:22-25
__device__ __forceinline__ double rdform_buffered(double rimg, double sig, double eps) {
#pragma clang fp contract(off)
    const double rho = rimg / sig;
    const double q = 1.07 / (rho + 0.07);
    const double q2 = q * q, q4 = q2 * q2;
    const double first = q4 * q2 * q;
    const double rho2 = rho * rho, rho4 = rho2 * rho2;
    const double second = 1.12 / (rho4 * rho2 * rho + 0.12) - 2;
    return eps * first * second;
}

// lj.c:218-249 and lj_fh_corr (lj.c:11-54); mi, mj: the two molecular masses
__device__ __forceinline__ double rdform_lj(double rimg, double sig, double eps, bool attractive, const RdFormParams &fp,
                                            double mi, double mj) {
#pragma clang fp contract(off)
    const double sor = fabs(sig) / rimg;
    double s6 = sor * sor * sor;
    s6 *= s6;
    const double t6 = s6;
    const double t12 = attractive ? 0.0 : s6 * s6;
    double e = 4.0 * eps * (t12 - t6);
    if (fp.fh) {
        const double ir = 1.0 / rimg, ir2 = ir * ir, ir3 = ir2 * ir, ir4 = ir3 * ir;
        const double rm = kAMU2KG * mi * mj / (mi + mj);
        const double dE = -24.0 * eps * (2.0 * t12 - t6) * ir;
        const double d2E = 24.0 * eps * (26.0 * t12 - 7.0 * t6) * ir2;
        double corr = kM2A2 * (kHBAR2 / (24.0 * kKB * fp.temperature * rm)) * (d2E + 2.0 * dE / rimg);
        if (fp.fh_order >= 4) {
            const double d3E = -1344.0 * eps * (6.0 * t12 - t6) * ir3;
            const double d4E = 12096.0 * eps * (10.0 * t12 - t6) * ir4;
            corr += kM2A4 * (kHBAR4 / (1152.0 * kKB2 * fp.temperature * fp.temperature * rm * rm)) *
                    (15.0 * dE * ir3 + 4.0 * d3E * ir + d4E);
        }
        e += corr;
    }
    return e;
}

struct RdFormTile {
    double x[kWave], y[kWave], z[kWave], eps[kWave], sig[kWave], mm[kWave];
    int mol[kWave], flags[kWave];
};

__device__ __forceinline__ void load_rdform_tile(RdFormTile &t, const DevAtoms &a, const MoveList &m, int j0, int lane) {
    const int j = j0 + lane;  // j < npad always (the grid covers npad / 64 tiles)
    moved_position(a, m, j, t.x[lane], t.y[lane], t.z[lane]);
    t.eps[lane] = a.eps[j];
    t.sig[lane] = a.sig[j];
    t.mm[lane] = a.molmass[j];
    t.mol[lane] = a.mol[j];
    t.flags[lane] = a.flags[j];
}

// Grids of the full and the incremental pass: owned_tile().  Like disp_tile_kernel this kernel takes a moved atom's
// position from the list, never from memory.  a: the REAL epsilon / sigma (the Lennard-Jones kernels of the same call
// are handed zeros).
constexpr int kRdFormWaves = 8;
constexpr int kRdFormJPerWave = kWave / kRdFormWaves;
template <int FORM>
__global__ __launch_bounds__(64 * kRdFormWaves) void rdform_tile_kernel(DevAtoms a, DevBox bx, RdFormParams fp,
                                                                         DirtyBlocks sel, double *__restrict__ partials,
                                                                         MoveList m) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    double *out = partials + (size_t)I * gridDim.x + J;
    if (J < I) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    __shared__ RdFormTile tj, ti;
    __shared__ double red[kRdFormWaves];
    if (wv == 0) load_rdform_tile(tj, a, m, J * kWave, lane);
    if (wv == 1) load_rdform_tile(ti, a, m, I * kWave, lane);
    __syncthreads();

    const int i = I * kWave + lane;
    const double xi = ti.x[lane], yi = ti.y[lane], zi = ti.z[lane];
    const double epsi = ti.eps[lane], sigi = ti.sig[lane], mmi = ti.mm[lane];
    const int moli = ti.mol[lane], fli = ti.flags[lane];
    const double rc = bx.cutoff;
    double acc = 0.0;
    for (int jj = wv * kRdFormJPerWave; jj < (wv + 1) * kRdFormJPerWave; ++jj) {
        const int j = J * kWave + jj;
        const int flj = tj.flags[jj];
        if (!pair_in_sum(i, j, fli, flj)) continue;
        const double epsj = tj.eps[jj], sigj = tj.sig[jj];
        if (FORM != kRdFormSG) {  // rd_excluded, pairs.c:61-71
            if (moli == tj.mol[jj] || epsi == 0.0 || sigi == 0.0 || epsj == 0.0 || sigj == 0.0) continue;
        }
        double r2u, ri2, dx, dy, dz;
        minimum_image_sq(bx, xi - tj.x[jj], yi - tj.y[jj], zi - tj.z[jj], r2u, ri2, dx, dy, dz);
        const double rimg = sqrt(ri2);
        if (FORM == kRdFormSG) {
            if (!(rimg < rc)) continue;  // sg.c:34
            acc += rdform_sg(rimg, fp, mmi);
        } else {
            if (FORM == kRdFormLJ) {
                if (!(rimg - kSMALL_dR < rc)) continue;  // lj.c:191
            } else {
                if (rimg > rc) continue;  // dreiding.c:35, lj_buffered_14_7.c:21
            }
            double sig, eps;
            bool attractive;
            rdform_mix(fp.mixing, epsi, sigi, epsj, sigj, sig, eps, attractive);
            if (FORM == kRdFormLJ)
                acc += rdform_lj(rimg, sig, eps, attractive, fp, mmi, tj.mm[jj]);
            else if (FORM == kRdFormDreiding)
                acc += rdform_dreiding(rimg, sig, eps, attractive);
            else
                acc += rdform_buffered(rimg, sig, eps);
        }
    }
    block_sum_store<kRdFormWaves>(acc, red, out);
}

// Long-range correction of the LJ form (lj_lrc_corr / lj_lrc_self, lj.c:56-107): every pair that is not frozen-frozen,
// same-molecule pairs included, whose MIXED eps_ij and sigma_ij are both non-zero, plus every non-frozen atom with its own
// non-zero values.  Parameters, the cutoff, the volume and which atoms exist: a full pass at upload, set_rd_form and box
// change; after mpmc_hip_edit_molecules only the tiles of the edited atoms' blocks are redone, like lj_lrc_kernel's.
// Grids: owned_tile(); tile partials [I][J].
constexpr int kRdFormLrcWaves = 8;
__device__ __forceinline__ double rdform_lrc_term(double eps, double sig, double rc, double volume) {
    const double sc = fabs(sig) / rc;
    double s3 = fabs(sig);
    s3 *= s3 * s3;
    const double sc3 = sc * sc * sc, sc9 = sc3 * sc3 * sc3;
    return ((16.0 / 3.0) * kPI * eps * s3) * ((1.0 / 3.0) * sc9 - sc3) / volume;
}
__global__ __launch_bounds__(64 * kRdFormLrcWaves) void rdform_lrc_kernel(DevAtoms a, DevBox bx, int mixing,
                                                                           DirtyBlocks sel, double *__restrict__ partials) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    double *out = partials + (size_t)I * gridDim.x + J;
    if (J < I) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    __shared__ double seps[kWave], ssig[kWave];
    __shared__ int sfl[kWave];
    __shared__ double red[kRdFormLrcWaves];
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
    for (int jj = wv * (kWave / kRdFormLrcWaves); jj < (wv + 1) * (kWave / kRdFormLrcWaves); ++jj) {
        const int j = J * kWave + jj;
        if (!pair_in_sum(i, j, fli, sfl[jj])) continue;
        double sig, eps;
        bool attractive;
        rdform_mix(mixing, epsi, sigi, seps[jj], ssig[jj], sig, eps, attractive);
        if (eps != 0.0 && sig != 0.0) acc += rdform_lrc_term(eps, sig, rc, bx.volume);
    }
    if (I == J && wv == 0) {  // self term once per atom, on the diagonal tile
        if ((fli & kValid) && !(fli & kFrozen) && sigi != 0.0 && epsi != 0.0) acc += rdform_lrc_term(epsi, sigi, rc, bx.volume);
    }
    block_sum_store<kRdFormLrcWaves>(acc, red, out);
}

}  // namespace mpmc
