// kernels_disp.h -- the PHAHST repulsion/dispersion term (option disp_expansion): exponential repulsion and a
// Tang-Toennies-damped C6 / C8 / C10 series (reference src/energy/disp_expansion.c:40-103, mixing pairs.c:142-193).
//
// What the reference sums, and this file therefore sums:
//   * EVERY pair with !(rd_excluded || frozen) at its minimum-image distance, whatever that distance is -- there is no
//     cutoff test in disp_expansion() -- so this is a dense tile sum with no screen and no candidate list;
//   * rd_excluded = same molecule, or (one of the four eps / sig values is 0 AND all six c6 / c8 / c10 are 0);
//   * per-atom epsilon is the exponent b (1/A), per-atom sigma the range rho (A);
//   * the pair part of the long-range correction runs over every pair that is not frozen-frozen (same-molecule and
//     rd-excluded pairs included), the self part over every non-frozen atom with its coefficients as read, in atomic units.
// One workgroup of 8 waves per 64 x 64 tile, J >= I, lane = row atom, each wave takes 8 of the 64 column atoms; tile
// ownership and the fixed-order sum are kernels_tile.h's.
#pragma once
#include "kernels_tile.h"

namespace mpmc {

struct DispAtoms {  // per atom, npad entries (pad atoms: zeros)
    const double *b, *rho;  // what the upload brought as epsilon / sigma
    const double *c6, *c8, *c10;  // atomic units, as read
};

struct DispParams {
    int damp;         // damp_dispersion
    int extrapolate;  // extrapolate_disp_coeffs
    int schmidt;      // schmidt_mixing
};

// H Bohr^n -> K A^n.  DEVIATION from the literal expression, owned here: pairs.c:185-193 evaluates
// `sqrt(..) * 0.021958709 / (3.166811429 * 0.000001)`, a multiplication and then a division; this file multiplies by the
// quotient of the two constants, formed at compile time.  The mixed coefficient can therefore differ from the reference's
// in its last bit (relative 1.1e-16, four orders inside the tests' tolerance), and that value is also what the
// extrapolation's `!= 0` tests and the long-range correction see; a product that is non-zero one way is non-zero the other
// (a normal number times ~7e3 cannot underflow), so no decision changes.
constexpr double kDispHartreeK = 3.166811429 * 0.000001;
constexpr double kDispC6 = 0.021958709 / kDispHartreeK;
constexpr double kDispC8 = 0.0061490647 / kDispHartreeK;
constexpr double kDispC10 = 0.0017219135 / kDispHartreeK;
constexpr double kDispRepulsion = 315.7750382111558307123944638;  // K (10^-3 Hartree)

// mixed c6 / c8 / c10 of a pair (pairs.c:185-193)
__device__ __forceinline__ void disp_mix_coeffs(const DispParams &dp, double c6i, double c8i, double c10i, double c6j,
                                                double c8j, double c10j, double &c6, double &c8, double &c10) {
    c6 = sqrt(c6i * c6j) * kDispC6;
    c8 = sqrt(c8i * c8j) * kDispC8;
    if (dp.extrapolate)
        c10 = (c6 != 0.0 && c8 != 0.0) ? 49.0 / 40.0 * c8 * c8 / c6 : 0.0;
    else
        c10 = sqrt(c10i * c10j) * kDispC10;
}

struct DispTile {
    double x[kWave], y[kWave], z[kWave], b[kWave], rho[kWave], c6[kWave], c8[kWave], c10[kWave];
    int mol[kWave], flags[kWave];
};

__device__ __forceinline__ void load_disp_tile(DispTile &t, const DevAtoms &a, const DispAtoms &d, const MoveList &m, int j0,
                                               int lane) {
    const int j = j0 + lane;  // j < npad always (the grid covers npad / 64 tiles)
    moved_position(a, m, j, t.x[lane], t.y[lane], t.z[lane]);
    t.b[lane] = d.b[j];
    t.rho[lane] = d.rho[j];
    t.c6[lane] = d.c6[j];
    t.c8[lane] = d.c8[j];
    t.c10[lane] = d.c10[j];
    t.mol[lane] = a.mol[j];
    t.flags[lane] = a.flags[j];
}

// Grids of the full and the incremental pass: owned_tile().  m: the step's move, as the pair kernel in front of this launch
// carried it (that launch also wrote the coordinate arrays; a moved atom's position is taken from the list all the same, so
// this kernel never reads a coordinate the other stream's writer may be storing at the same time).
constexpr int kDispWaves = 8;
constexpr int kDispJPerWave = kWave / kDispWaves;
__global__ __launch_bounds__(64 * kDispWaves) void disp_tile_kernel(DevAtoms a, DispAtoms d, DevBox bx, DispParams dp,
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
    __shared__ DispTile tj, ti;
    __shared__ double red[kDispWaves];
    if (wv == 0) load_disp_tile(tj, a, d, m, J * kWave, lane);
    if (wv == 1) load_disp_tile(ti, a, d, m, I * kWave, lane);
    __syncthreads();

    const int i = I * kWave + lane;
    const double xi = ti.x[lane], yi = ti.y[lane], zi = ti.z[lane];
    const double bi = ti.b[lane], rhoi = ti.rho[lane];
    const double c6i = ti.c6[lane], c8i = ti.c8[lane], c10i = ti.c10[lane];
    const int moli = ti.mol[lane], fli = ti.flags[lane];
    const bool zero_i = (bi == 0.0 || rhoi == 0.0);
    const bool nodisp_i = (c6i == 0.0 && c8i == 0.0 && c10i == 0.0);
    double acc = 0.0;
    for (int jj = wv * kDispJPerWave; jj < (wv + 1) * kDispJPerWave; ++jj) {
        const int j = J * kWave + jj;
        const int flj = tj.flags[jj];
        if (!pair_in_sum(i, j, fli, flj)) continue;
        if (moli == tj.mol[jj]) continue;  // ... and not on one molecule (pairs.c:61-81)
        const double bj = tj.b[jj], rhoj = tj.rho[jj];
        const double c6j = tj.c6[jj], c8j = tj.c8[jj], c10j = tj.c10[jj];
        // null repulsion AND null dispersion (pairs.c:68)
        if ((zero_i || bj == 0.0 || rhoj == 0.0) && nodisp_i && (c6j == 0.0 && c8j == 0.0 && c10j == 0.0)) continue;

        double r2u, ri2, dx, dy, dz;
        minimum_image_sq(bx, xi - tj.x[jj], yi - tj.y[jj], zi - tj.z[jj], r2u, ri2, dx, dy, dz);
        const double r = sqrt(ri2);  // rimg; no cutoff (disp_expansion.c:56-80)

        // mixing (pairs.c:147-149, :180-181): followed literally, 0 / 0 = NaN included
        const double rho = 0.5 * (rhoi + rhoj);
        const double b = dp.schmidt ? (bi + bj) * bi * bj / (bi * bi + bj * bj) : 2.0 * bi * bj / (bi + bj);
        double c6, c8, c10;
        disp_mix_coeffs(dp, c6i, c8i, c10i, c6j, c8j, c10j, c6, c8, c10);

        double repulsion = 0.0;
        if (b != 0.0 && rho != 0.0) repulsion = kDispRepulsion * exp(-b * (r - rho));

        // one reciprocal for the three inverse powers
        const double r2 = r * r;
        const double ir2 = 1.0 / r2, ir4 = ir2 * ir2;
        const double ir6 = ir4 * ir2, ir8 = ir4 * ir4, ir10 = ir8 * ir2;
        double f6 = 1.0, f8 = 1.0, f10 = 1.0;
        if (dp.damp) {
            // tt_damping(n, x) = 1 - exp(-x) sum_{k <= n} x^k / k!, exactly 0 unless > 1e-9 (disp_expansion.c:164-177):
            // one exp, the three partial sums from one running term
            const double x = b * r;
            const double ex = exp(-x);
            double term = x, sum = 1.0 + x;
            term *= x * (1.0 / 2.0); sum += term;
            term *= x * (1.0 / 3.0); sum += term;
            term *= x * (1.0 / 4.0); sum += term;
            term *= x * (1.0 / 5.0); sum += term;
            term *= x * (1.0 / 6.0); sum += term;
            f6 = 1.0 - ex * sum;
            term *= x * (1.0 / 7.0); sum += term;
            term *= x * (1.0 / 8.0); sum += term;
            f8 = 1.0 - ex * sum;
            term *= x * (1.0 / 9.0); sum += term;
            term *= x * (1.0 / 10.0); sum += term;
            f10 = 1.0 - ex * sum;
            f6 = (f6 > 0.000000001) ? f6 : 0.0;  // (NaN compares false: 0, as in the reference)
            f8 = (f8 > 0.000000001) ? f8 : 0.0;
            f10 = (f10 > 0.000000001) ? f10 : 0.0;
        }
        acc += -f6 * c6 * ir6 - f8 * c8 * ir8 - f10 * c10 * ir10 + repulsion;
    }
    block_sum_store<kDispWaves>(acc, red, out);
}

// The term of one pair that is in the sum, at its distance r: mixing, repulsion, damped dispersion -- the pair term of
// disp_tile_kernel below, statement by statement, for the non-periodic sum of kernels_dimer.h (disp_expansion.c:118-140).
// disp_tile_kernel keeps its own text: calling this function from it changed which products the compiler fuses into an
// FMA, and with that the last bit of sums that are on record.
__device__ __forceinline__ double disp_pair_energy(const DispParams &dp, double bi, double rhoi, double c6i, double c8i,
                                                   double c10i, double bj, double rhoj, double c6j, double c8j, double c10j,
                                                   double r) {
    // mixing (pairs.c:147-149, :180-181): followed literally, 0 / 0 = NaN included
    const double rho = 0.5 * (rhoi + rhoj);
    const double b = dp.schmidt ? (bi + bj) * bi * bj / (bi * bi + bj * bj) : 2.0 * bi * bj / (bi + bj);
    double c6, c8, c10;
    disp_mix_coeffs(dp, c6i, c8i, c10i, c6j, c8j, c10j, c6, c8, c10);

    double repulsion = 0.0;
    if (b != 0.0 && rho != 0.0) repulsion = kDispRepulsion * exp(-b * (r - rho));

    // one reciprocal for the three inverse powers
    const double r2 = r * r;
    const double ir2 = 1.0 / r2, ir4 = ir2 * ir2;
    const double ir6 = ir4 * ir2, ir8 = ir4 * ir4, ir10 = ir8 * ir2;
    double f6 = 1.0, f8 = 1.0, f10 = 1.0;
    if (dp.damp) {
        // tt_damping(n, x) = 1 - exp(-x) sum_{k <= n} x^k / k!, exactly 0 unless > 1e-9 (disp_expansion.c:164-177):
        // one exp, the three partial sums from one running term
        const double x = b * r;
        const double ex = exp(-x);
        double term = x, sum = 1.0 + x;
        term *= x * (1.0 / 2.0); sum += term;
        term *= x * (1.0 / 3.0); sum += term;
        term *= x * (1.0 / 4.0); sum += term;
        term *= x * (1.0 / 5.0); sum += term;
        term *= x * (1.0 / 6.0); sum += term;
        f6 = 1.0 - ex * sum;
        term *= x * (1.0 / 7.0); sum += term;
        term *= x * (1.0 / 8.0); sum += term;
        f8 = 1.0 - ex * sum;
        term *= x * (1.0 / 9.0); sum += term;
        term *= x * (1.0 / 10.0); sum += term;
        f10 = 1.0 - ex * sum;
        f6 = (f6 > 0.000000001) ? f6 : 0.0;  // (NaN compares false: 0, as in the reference)
        f8 = (f8 > 0.000000001) ? f8 : 0.0;
        f10 = (f10 > 0.000000001) ? f10 : 0.0;
    }
    return -f6 * c6 * ir6 - f8 * c8 * ir8 - f10 * c10 * ir10 + repulsion;
}

// Long-range correction (disp_expansion.c:5-38, :50-53, :92-100): parameters, the cutoff, the volume and which atoms
// exist, no coordinate.  A full pass at upload / set_dispersion and at box change; after mpmc_hip_edit_molecules only the
// tiles of the edited atoms' blocks are redone, like lj_lrc_kernel's.  Grids: owned_tile(); tile partials [I][J], summed by
// reduce_rows_kernel.
constexpr int kDispLrcWaves = 8;
__device__ __forceinline__ double disp_lrc_term(double c6, double c8, double c10, double rc, double volume) {
    return -4.0 * kPI * (c6 / (3.0 * rc * rc * rc) + c8 / (5.0 * rc * rc * rc * rc * rc) +
                         c10 / (7.0 * rc * rc * rc * rc * rc * rc * rc)) / volume;
}
__global__ __launch_bounds__(64 * kDispLrcWaves) void disp_lrc_kernel(DevAtoms a, DispAtoms d, DevBox bx, DispParams dp,
                                                                      DirtyBlocks sel, double *__restrict__ partials) {
    int I, J;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!owned_tile(sel, I, J)) return;
    double *out = partials + (size_t)I * gridDim.x + J;
    if (J < I) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }
    __shared__ double s6[kWave], s8[kWave], s10[kWave];
    __shared__ int sfl[kWave];
    __shared__ double red[kDispLrcWaves];
    if (wv == 0) {
        s6[lane] = d.c6[J * kWave + lane];
        s8[lane] = d.c8[J * kWave + lane];
        s10[lane] = d.c10[J * kWave + lane];
        sfl[lane] = a.flags[J * kWave + lane];
    }
    __syncthreads();
    const int i = I * kWave + lane;
    const double c6i = d.c6[i], c8i = d.c8[i], c10i = d.c10[i];
    const int fli = a.flags[i];
    const double rc = bx.cutoff;
    double acc = 0.0;
    for (int jj = wv * (kWave / kDispLrcWaves); jj < (wv + 1) * (kWave / kDispLrcWaves); ++jj) {
        const int j = J * kWave + jj;
        const int flj = sfl[jj];
        // every pair that is not frozen-frozen: same-molecule and rd-excluded pairs included (disp_expansion.c:7, :50-53)
        if (!pair_in_sum(i, j, fli, flj)) continue;
        double c6, c8, c10;
        disp_mix_coeffs(dp, c6i, c8i, c10i, s6[jj], s8[jj], s10[jj], c6, c8, c10);
        acc += disp_lrc_term(c6, c8, c10, rc, bx.volume);
    }
    if (I == J && wv == 0) {  // self term once per atom, on the diagonal tile: coefficients as read (atomic units)
        if ((fli & kValid) && !(fli & kFrozen)) {
            double c10 = c10i;
            if (dp.extrapolate) c10 = (c6i != 0.0 && c8i != 0.0) ? 49.0 / 40.0 * c8i * c8i / c6i : 0.0;
            acc += disp_lrc_term(c6i, c8i, c10, rc, bx.volume);
        }
    }
    block_sum_store<kDispLrcWaves>(acc, red, out);
}

}  // namespace mpmc
