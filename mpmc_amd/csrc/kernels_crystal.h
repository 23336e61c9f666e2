// kernels_crystal.h -- Lennard-Jones summed over lattice images beyond the minimum image (option rd_crystal, reference
// src/energy/lj.c:109-276).  With o = rd_crystal_order the images are n in {-(o-1) .. o-1}^3 and the cutoff is
// cutoff_c = 2.0 * pbc_cutoff * ((double)o - 0.5).
//
// What the reference sums, and this file therefore sums:
//   * pair part: EVERY unordered pair that is not frozen-frozen, same-molecule pairs included, whose minimum-image distance
//     passes `rimg - 1e-12 < cutoff_c`; for such a pair s6 = sum_n (|sigma_ij| / r_n)^6 and s12 likewise, over the images
//     with !(r_n > cutoff_c) -- an image at exactly the cutoff counts -- where r_n is measured from the RAW resident
//     coordinates (pos_i - pos_j, i < j in atom order), not from the minimum image: moving a molecule by a lattice vector
//     changes the sum, as it does in the reference (wrapall() only writes wrapped_pos).  n = 0 is skipped for a
//     same-molecule pair.  Energy 4 eps_ij (s12 - s6); the mixing is the Lennard-Jones path's (kernels_pair.h): a pair
//     with a sigma < 0 has eps_ij = 0 (never set in the reference) and a null-parameter pair has eps_ij = 0 or
//     sigma_ij = 0, so both give exactly 0 and are left out here.
//   * Feynman-Hibbs: lj_fh_corr once per pair with the SUMMED s12 and s6, evaluated at rimg, reduced mass from the two
//     molecular masses (m / 2 for a same-molecule pair) -- followed literally.
//   * self part: every atom, frozen ones included, unless sigma == 0 && eps == 0: all n != 0 with !(|n.basis| > cutoff_c),
//     0.5 (|sigma| / r)^6 and 0.5 (|sigma| / r)^12, energy 4 eps (t12 - s6) with t12 = 0 when sigma < 0.  Box and per-atom
//     parameters only: evaluated at upload and at box change (rdc_self_kernel).
//   * the long-range correction is lj_lrc_kernel's (kernels_pair.h), handed a box copy whose cutoff is cutoff_c.
//
// The cutoff decision is exact.  a[p] = ((b[0][p] n0 + b[1][p] n1) + b[2][p] n2) + (pos_i[p] - pos_j[p]) and
// r^2 = (a0 a0 + a1 a1) + a2 a2 are formed without FMA contraction in that order, and r^2 is compared with the host's
// r2max = max{x : sqrt(x) <= cutoff_c} (found with nextafter around cutoff_c^2): under a correctly rounded square root
// that is the decision `sqrt(r^2) > cutoff_c`.  In a lattice-like configuration thousands of images sit on the cutoff to
// the last bit (fixture 012), so `>=`, fp32 or a contracted r^2 changes the result well above the tests' tolerance.
//
// DEVIATION from the literal expression, owned here: the reference takes pow(|sigma| / r, 6) and pow(.., 12) of a
// square-rooted r; this file forms q = sigma^2 * (1 / r^2), q^3 and (q^3)^2 from one reciprocal of r^2.  The terms differ
// by ~1e-16 relative, four orders inside the tests' tolerance; no decision depends on them.
//
// One workgroup of 8 waves per 64 x 64 tile, J >= I, lane = row atom, each wave takes 8 of the 64 column atoms, the innermost
// loop runs over the images (translations staged once per workgroup in LDS); tile ownership and the fixed-order sum are
// kernels_tile.h's.
#pragma once
#include "kernels_tile.h"

namespace mpmc {

constexpr int kRdcMaxOrder = 4;
constexpr int kRdcMaxImages = (2 * kRdcMaxOrder - 1) * (2 * kRdcMaxOrder - 1) * (2 * kRdcMaxOrder - 1);  // 343

struct RdcParams {
    int order;         // rd_crystal_order, 1 .. kRdcMaxOrder
    int fh_order;      // 0 = off, 2, 4
    double cutoff_c;   // 2.0 * pbc_cutoff * ((double)order - 0.5)
    double r2max;      // max{x : sqrt(x) <= cutoff_c}
    double temperature;
};

// translation of image k (k = (n0 * w + n1) * w + n2 in the reference's loop order, w = 2 o - 1), lj.c:204-207
__device__ __forceinline__ void rdc_translation(const DevBox &bx, int order, int k, double &tx, double &ty, double &tz) {
#pragma clang fp contract(off)
    const int w = 2 * order - 1;
    const double n0 = (double)(k / (w * w) - (order - 1));
    const double n1 = (double)((k / w) % w - (order - 1));
    const double n2 = (double)(k % w - (order - 1));
    double t;
    t = bx.b[0][0] * n0;
    t = t + bx.b[1][0] * n1;
    tx = t + bx.b[2][0] * n2;
    t = bx.b[0][1] * n0;
    t = t + bx.b[1][1] * n1;
    ty = t + bx.b[2][1] * n2;
    t = bx.b[0][2] * n0;
    t = t + bx.b[1][2] * n1;
    tz = t + bx.b[2][2] * n2;
}

// r^2 of a displacement plus a translation, in the reference's operation order (lj.c:208-210)
__device__ __forceinline__ double rdc_image_r2(double tx, double ty, double tz, double dx, double dy, double dz) {
#pragma clang fp contract(off)
    const double a0 = tx + dx, a1 = ty + dy, a2 = tz + dz;
    double r2 = a0 * a0;
    r2 = r2 + a1 * a1;
    r2 = r2 + a2 * a2;
    return r2;
}

struct RdcTile {
    double x[kWave], y[kWave], z[kWave], eps[kWave], sig[kWave], mm[kWave];
    int mol[kWave], flags[kWave];
};

__device__ __forceinline__ void load_rdc_tile(RdcTile &t, const DevAtoms &a, const MoveList &m, int j0, int lane) {
    const int j = j0 + lane;  // j < npad always (the grid covers npad / 64 tiles)
    moved_position(a, m, j, t.x[lane], t.y[lane], t.z[lane]);
    t.eps[lane] = a.eps[j];
    t.sig[lane] = a.sig[j];
    t.mm[lane] = a.molmass[j];
    t.mol[lane] = a.mol[j];
    t.flags[lane] = a.flags[j];
}

// Grids of the full and the incremental pass: owned_tile().  Like disp_tile_kernel this kernel takes a moved atom's
// position from the list, never from memory.  a: the REAL epsilon / sigma (the
// Lennard-Jones kernels of the same call are handed zeros).
constexpr int kRdcWaves = 8;
constexpr int kRdcJPerWave = kWave / kRdcWaves;
__global__ __launch_bounds__(64 * kRdcWaves) void rdc_tile_kernel(DevAtoms a, DevBox bx, RdcParams rp, DirtyBlocks sel,
                                                                   double *__restrict__ partials, MoveList m) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    double *out = partials + (size_t)I * gridDim.x + J;
    if (J < I) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    __shared__ RdcTile tj, ti;
    __shared__ double simg[3][kRdcMaxImages];
    __shared__ double red[kRdcWaves];
    const int w = 2 * rp.order - 1;
    const int nimg = w * w * w, centre = nimg / 2;  // (order <= kRdcMaxOrder: checked by the host)
    if (wv == 0) load_rdc_tile(tj, a, m, J * kWave, lane);
    if (wv == 1) load_rdc_tile(ti, a, m, I * kWave, lane);
    if ((int)threadIdx.x < nimg) {
        double tx, ty, tz;
        rdc_translation(bx, rp.order, threadIdx.x, tx, ty, tz);
        simg[0][threadIdx.x] = tx;
        simg[1][threadIdx.x] = ty;
        simg[2][threadIdx.x] = tz;
    }
    __syncthreads();

    const int i = I * kWave + lane;
    const double xi = ti.x[lane], yi = ti.y[lane], zi = ti.z[lane];
    const double epsi = ti.eps[lane], sigi = ti.sig[lane], mmi = ti.mm[lane];
    const int moli = ti.mol[lane], fli = ti.flags[lane];
    double acc = 0.0;
    for (int jj = wv * kRdcJPerWave; jj < (wv + 1) * kRdcJPerWave; ++jj) {
        const int j = J * kWave + jj;
        const int flj = tj.flags[jj];
        if (!pair_in_sum(i, j, fli, flj)) continue;  // same-molecule pairs take part (lj.c:191-193)
        const double epsj = tj.eps[jj], sigj = tj.sig[jj];
        // Lorentz-Berthelot as the Lennard-Jones path mixes it (pairs.c:200-211): what is left out here is exactly 0
        if (!(sigi > 0.0 && sigj > 0.0) || epsi == 0.0 || epsj == 0.0) continue;
        const double sig = 0.5 * (sigi + sigj);
        const double eps = sqrt(epsi * epsj);
        const double dx = xi - tj.x[jj], dy = yi - tj.y[jj], dz = zi - tj.z[jj];
        double r2u, ri2, ex, ey, ez;
        minimum_image_sq(bx, dx, dy, dz, r2u, ri2, ex, ey, ez);
        const double rimg = sqrt(ri2);
        if (!(rimg - kSMALL_dR < rp.cutoff_c)) continue;
        const bool same = (moli == tj.mol[jj]);
        const double sig2 = sig * sig;
        double s6 = 0.0, s12 = 0.0;
        for (int k = 0; k < nimg; ++k) {
            if (same && k == centre) continue;  // no n = 0 for an intra-molecular pair (lj.c:202)
            const double r2 = rdc_image_r2(simg[0][k], simg[1][k], simg[2][k], dx, dy, dz);
            if (r2 > rp.r2max) continue;  // sqrt(r2) > cutoff_c, and nothing else
            const double q = sig2 * (1.0 / r2);
            const double q3 = q * q * q;
            s6 += q3;
            s12 += q3 * q3;
        }
        double e = 4.0 * eps * (s12 - s6);
        if (rp.fh_order) {  // lj_fh_corr (lj.c:11-54) with the summed terms, at rimg
            const double ir = 1.0 / rimg, ir2 = ir * ir, ir3 = ir2 * ir, ir4 = ir3 * ir;
            const double mj = tj.mm[jj];
            const double rm = kAMU2KG * mmi * mj / (mmi + mj);
            const double dE = -24.0 * eps * (2.0 * s12 - s6) * ir;
            const double d2E = 24.0 * eps * (26.0 * s12 - 7.0 * s6) * ir2;
            double corr = kM2A2 * (kHBAR2 / (24.0 * kKB * rp.temperature * rm)) * (d2E + 2.0 * dE / rimg);
            if (rp.fh_order >= 4) {
                const double d3E = -1344.0 * eps * (6.0 * s12 - s6) * ir3;
                const double d4E = 12096.0 * eps * (10.0 * s12 - s6) * ir4;
                corr += kM2A4 * (kHBAR4 / (1152.0 * kKB2 * rp.temperature * rp.temperature * rm * rm)) *
                        (15.0 * dE * ir3 + 4.0 * d3E * ir + d4E);
            }
            e += corr;
        }
        acc += e;
    }
    block_sum_store<kRdcWaves>(acc, red, out);
}

// Self part (rd_crystal_self, lj.c:109-162): the two lattice sums are the same for every atom, so they are formed once
// (in image order) and each atom takes 4 eps (sigma^12 L12 - sigma^6 L6).  One workgroup; fixed-order reduction.
constexpr int kRdcSelfThreads = 256;
__global__ __launch_bounds__(kRdcSelfThreads) void rdc_self_kernel(DevAtoms a, DevBox bx, RdcParams rp,
                                                                   double *__restrict__ out) {
    __shared__ double slat[2];
    __shared__ double s[kRdcSelfThreads / 64];
    if (threadIdx.x == 0) {
        const int w = 2 * rp.order - 1;
        const int nimg = w * w * w, centre = nimg / 2;
        double l6 = 0.0, l12 = 0.0;
        for (int k = 0; k < nimg; ++k) {
            if (k == centre) continue;
            double tx, ty, tz;
            rdc_translation(bx, rp.order, k, tx, ty, tz);
            const double r2 = rdc_image_r2(tx, ty, tz, 0.0, 0.0, 0.0);
            if (r2 > rp.r2max) continue;
            const double q = 1.0 / r2;
            const double q3 = q * q * q;
            l6 += 0.5 * q3;
            l12 += 0.5 * (q3 * q3);
        }
        slat[0] = l6;
        slat[1] = l12;
    }
    __syncthreads();
    const double l6 = slat[0], l12 = slat[1];
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.n; i += kRdcSelfThreads) {
        if (!(a.flags[i] & kValid)) continue;
        const double sig = a.sig[i], eps = a.eps[i];
        if (sig == 0.0 && eps == 0.0) continue;
        const double g2 = sig * sig, g6 = g2 * g2 * g2;
        const double t6 = g6 * l6;
        const double t12 = (sig < 0.0) ? 0.0 : (g6 * g6) * l12;  // attractive only
        acc += 4.0 * eps * (t12 - t6);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (s[0] + s[1]) + (s[2] + s[3]);
}

}  // namespace mpmc
