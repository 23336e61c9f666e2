// kernels_at.h -- the Axilrod-Teller triple-dipole term (option axilrod_teller; reference src/energy/axilrod_teller.cpp:85-179,
// called from energy.c:148-151 and reported as observables->three_body_energy).
//
// What the reference sums, and this file therefore sums:
//   * ALL ordered triples of pairwise distinct atoms that are not all three on one molecule, divided by 6 -- here every
//     unordered triple i < j < k once.  Two atoms of one molecule with a third elsewhere count; frozen atoms count (there is no
//     frozen test at all, unlike every pair term); there is no cutoff;
//   * three INDEPENDENT minimum images d_ij, d_ik, d_jk (d_ab = pos_a - pos_b).  In a periodic box they need not close a
//     triangle, and often do not; that is the reference's behaviour and is kept.  rint() is odd, so d_ba = -d_ab exactly and
//     the six orderings of a triple give the same term up to the rounding of its products;
//   * E_ijk = c9_ijk (1 + cos_part) / (r_ij r_ik r_jk)^3, cos_part = 3 [(-d_ij).(-d_ik) / (r_ij r_ik)] [d_ij.(-d_jk) /
//     (r_ij r_jk)] [d_ik.d_jk / (r_ik r_jk)], i.e. c9 t_ij t_ik t_jk (1 - 3 (e_ij.e_ik)(e_ij.e_jk)(e_ik.e_jk)) with
//     e = d / r and t = 1 / r^3: four doubles per pair;
//   * c9_ijk = pow(p_i p_j p_k, 1/3) * 3 / (1/(c_i/p_i) + 1/(c_j/p_j) + 1/(c_k/p_k)) * 0.0032539449 / 3.166811429e-6 with
//     p = pow(alpha * 6.7483345, 3), exactly 0 when one of the three polarizabilities is 0.
//
// DEVIATION from the literal coefficient, owned here (like kDispC6 in kernels_disp.h).  The engine keeps two values per
// atom, a_i = alpha_i * 6.7483345 and g_i = 1 / (c_i / p_i) (AtAtoms; formed on the host with the reference's own pow), and
// forms c9_ijk = a_i a_j a_k * 3 / (g_i + g_j + g_k) * K with the conversion quotient K formed at compile time:
// pow(p_i p_j p_k, 1/3) is a_i a_j a_k up to the rounding of two pow calls, and the multiplication by 0.0032539449
// followed by the division becomes one multiplication.  The value differs from the literal one by a few ulp (relative
// ~1e-15, three orders inside the tests' tolerance).  No zero / non-zero decision changes: a_i a_j a_k is 0 exactly when one
// polarizability is 0 (the values are of order 1 .. 100, no underflow), which is the reference's explicit test; a site
// with alpha != 0 and c = 0 has g = 1 / 0 = inf either way and 3 / inf = 0 exactly; K is a normal number of order 1e3.
//
// Layout.  The cached unit is one unordered triple I <= J <= K of the 64-atom blocks the pair kernels use, split into
// kAtSplit sub-partials by the k atom (a fixed layout: a function of the block count only, never tuned per call), so that
// a box of 8 blocks (120 units) still fills the device.  Unit (I, J, K) has index C(K+2, 3) + C(J+1, 2) + I, its
// sub-partials follow each other.  A sub-partial is a function of its three blocks' atoms only and is summed in a fixed
// order, so an incremental pass over the units that contain a moved block leaves the bits of a from-scratch pass.
// One workgroup of 8 waves per sub-partial: lane = atom i of block I, wave w owns the j atoms 8w .. 8w+7 of block J (their
// (i, j) pair data stay in registers), and the k atoms arrive in slices of 8: the (j, k) table of the slice (broadcast
// reads) and the (i, k) table (one column per lane) are formed once per workgroup in LDS.
#pragma once
#include "kernels_tile.h"

namespace mpmc {

struct AtAtoms {  // per atom, npad entries (pad atoms: a = 0, g = 1)
    const double *a;  // alpha * 6.7483345
    const double *g;  // 1 / (c9 / a^3); 1 where a == 0 (never used: the product has a factor 0)
};

constexpr double kAtHartreeK = 3.166811429 * 0.000001;
constexpr double kAtC9 = 0.0032539449 / kAtHartreeK;  // H Bohr^9 -> K A^9
constexpr double kAtAlpha = 6.7483345;                 // A^3 -> Bohr^3

constexpr int kAtWaves = 8;
constexpr int kAtJPerWave = kWave / kAtWaves;  // 8 j atoms per wave
constexpr int kAtSlice = 8;                    // k atoms per LDS slice
constexpr int kAtSplit = 4;                    // sub-partials per unit: 16 k atoms each
constexpr int kAtKPerSplit = kWave / kAtSplit;
constexpr int kAtNoMol = -0x7fffffff;          // "j and k are on different molecules" (pad molecule ids are -2 - index)

__host__ __device__ inline long at_unit_count(int nb) { return (long)nb * (nb + 1) * (nb + 2) / 6; }
__host__ __device__ inline long at_unit_index(int I, int J, int K) {  // I <= J <= K
    return (long)K * (K + 1) * (K + 2) / 6 + (long)J * (J + 1) / 2 + I;
}

struct AtBlock {
    double x[kWave], y[kWave], z[kWave], a[kWave], g[kWave];
    int mol[kWave];
};

// positions from the step's move where it carries one; an atom that is not there (padding, a hole) reads as a = 0
__device__ __forceinline__ void load_at_block(AtBlock &t, const DevAtoms &a, const AtAtoms &d, const MoveList &m, int j0,
                                              int lane) {
    const int j = j0 + lane;  // j < npad always (block indices are below npad / 64)
    moved_position(a, m, j, t.x[lane], t.y[lane], t.z[lane]);
    const bool valid = (a.flags[j] & kValid) != 0;
    t.a[lane] = valid ? d.a[j] : 0.0;
    t.g[lane] = valid ? d.g[j] : 1.0;
    t.mol[lane] = a.mol[j];
}

// e = d / r and t = 1 / r^3 of one pair at its own minimum image
__device__ __forceinline__ void at_pair(const DevBox &bx, double dx, double dy, double dz, double &ex, double &ey, double &ez,
                                        double &t) {
    double r2u, ri2, ox, oy, oz;
    minimum_image_sq(bx, dx, dy, dz, r2u, ri2, ox, oy, oz);
    const double ir = 1.0 / sqrt(ri2);
    ex = ox * ir;
    ey = oy * ir;
    ez = oz * ir;
    t = ir * ir * ir;
}

// Full pass (sel.n == 0): grid = (at_unit_count(nb) * kAtSplit), workgroup x = unit * kAtSplit + sub-partial.
// Incremental pass (sel.n > 0): grid = (nb (nb + 1) / 2 * kAtSplit, sel.n); workgroup (x, y) redoes sub-partial x % kAtSplit
// of the unit made of the dirty block sel.blk[y] and the block pair P <= Q numbered x / kAtSplit = Q (Q + 1) / 2 + P.
// A unit that holds several dirty blocks belongs to the one that comes first in sel: the workgroup of a later entry
// returns when P or Q is an earlier entry's block (every unit with a dirty block is redone exactly once: by its earliest
// dirty member, with the other two blocks as the pair, and a pair is enumerated once).
// m: the step's move as the pair kernel in front of this launch carried it (see disp_tile_kernel).
__global__ __launch_bounds__(64 * kAtWaves) void at_triple_kernel(DevAtoms a, AtAtoms d, DevBox bx, DirtyBlocks sel, int nb,
                                                                  double *__restrict__ partials, MoveList m) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = blockIdx.x % kAtSplit;
    int rest = blockIdx.x / kAtSplit;
    int I, J, K;
    if (sel.n > 0) {
        int Q = 0;
        while ((Q + 1) * (Q + 2) / 2 <= rest) ++Q;
        const int P = rest - Q * (Q + 1) / 2;
        const int D = sel.blk[blockIdx.y];
        for (int e = 0; e < (int)blockIdx.y; ++e)
            if (sel.blk[e] == P || sel.blk[e] == Q) return;
        I = min(D, P);
        K = max(D, Q);
        J = D + P + Q - I - K;
    } else {
        K = 0;
        while (at_unit_count(K + 1) <= rest) ++K;
        rest -= (int)at_unit_count(K);
        J = 0;
        while ((J + 1) * (J + 2) / 2 <= rest) ++J;
        I = rest - J * (J + 1) / 2;
    }
    if (I < 0 || I > J || J > K || K >= nb) return;  // (cannot happen with the grids above)
    double *out = partials + at_unit_index(I, J, K) * kAtSplit + sub;

    __shared__ AtBlock bi, bj, bk;
    __shared__ double jk[kWave][kAtSlice][5];   // e_jk (3), w = t_jk a_j a_k 3 K, g_j + g_k
    __shared__ int jkmol[kWave][kAtSlice];      // the molecule of j and k when it is the same one, else kAtNoMol
    __shared__ double ik[kAtSlice][4][kWave];   // e_ik (3), t_ik; one column per lane
    __shared__ double red[kAtWaves];
    __shared__ int active[3];
    if (wv == 0) load_at_block(bi, a, d, m, I * kWave, lane);
    if (wv == 1) load_at_block(bj, a, d, m, J * kWave, lane);
    if (wv == 2) load_at_block(bk, a, d, m, K * kWave, lane);
    __syncthreads();
    if (wv < 3) {  // a block without a three-body site: every triple of the unit is an exact 0
        const AtBlock &b = wv == 0 ? bi : (wv == 1 ? bj : bk);
        const unsigned long long any = __ballot(b.a[lane] != 0.0);
        if (lane == 0) active[wv] = any != 0ull;
    }
    __syncthreads();
    if (!(active[0] && active[1] && active[2])) {
        if (threadIdx.x == 0) out[0] = 0.0;
        return;
    }

    // (i, j) of this wave's 8 j atoms: registers for the whole k loop.  a_i is folded into t_ij.
    const int i = I * kWave + lane;
    const double xi = bi.x[lane], yi = bi.y[lane], zi = bi.z[lane];
    const double ai = bi.a[lane], gi = bi.g[lane];
    const int moli = bi.mol[lane];
    double eijx[kAtJPerWave], eijy[kAtJPerWave], eijz[kAtJPerWave], tij[kAtJPerWave];
#pragma unroll
    for (int q = 0; q < kAtJPerWave; ++q) {
        const int jj = wv * kAtJPerWave + q;
        const int j = J * kWave + jj;
        const double aj = bj.a[jj];
        double ex = 0.0, ey = 0.0, ez = 0.0, t = 0.0;
        if (i < j && ai != 0.0 && aj != 0.0) {
            at_pair(bx, xi - bj.x[jj], yi - bj.y[jj], zi - bj.z[jj], ex, ey, ez, t);
            t *= ai;
        }
        eijx[q] = ex;
        eijy[q] = ey;
        eijz[q] = ez;
        tij[q] = t;
    }

    double acc = 0.0;
    for (int k0 = sub * kAtKPerSplit; k0 < (sub + 1) * kAtKPerSplit; k0 += kAtSlice) {
        __syncthreads();  // the previous slice has been read
        {   // (j, k) table: 64 x 8 pairs, one per thread
            const int jj = threadIdx.x >> 3, kk = threadIdx.x & 7;
            const int j = J * kWave + jj, k = K * kWave + k0 + kk;
            const double aj = bj.a[jj], ak = bk.a[k0 + kk];
            double ex = 0.0, ey = 0.0, ez = 0.0, w = 0.0, gs = 1.0;
            if (j < k && aj != 0.0 && ak != 0.0) {
                double t;
                at_pair(bx, bj.x[jj] - bk.x[k0 + kk], bj.y[jj] - bk.y[k0 + kk], bj.z[jj] - bk.z[k0 + kk], ex, ey, ez, t);
                w = t * (aj * ak) * (3.0 * kAtC9);
                gs = bj.g[jj] + bk.g[k0 + kk];
            }
            jk[jj][kk][0] = ex;
            jk[jj][kk][1] = ey;
            jk[jj][kk][2] = ez;
            jk[jj][kk][3] = w;
            jk[jj][kk][4] = gs;
            jkmol[jj][kk] = (bj.mol[jj] == bk.mol[k0 + kk]) ? bj.mol[jj] : kAtNoMol;
        }
        {   // (i, k) table: 8 x 64 pairs, one per thread
            const int kk = threadIdx.x >> 6;
            const int k = K * kWave + k0 + kk;
            const double ak = bk.a[k0 + kk];
            double ex = 0.0, ey = 0.0, ez = 0.0, t = 0.0;
            if (i < k && ai != 0.0 && ak != 0.0)
                at_pair(bx, xi - bk.x[k0 + kk], yi - bk.y[k0 + kk], zi - bk.z[k0 + kk], ex, ey, ez, t);
            ik[kk][0][lane] = ex;
            ik[kk][1][lane] = ey;
            ik[kk][2][lane] = ez;
            ik[kk][3][lane] = t;
        }
        __syncthreads();
        for (int kk = 0; kk < kAtSlice; ++kk) {
            const double eikx = ik[kk][0][lane], eiky = ik[kk][1][lane], eikz = ik[kk][2][lane], tik = ik[kk][3][lane];
#pragma unroll
            for (int q = 0; q < kAtJPerWave; ++q) {
                const int jj = wv * kAtJPerWave + q;
                const double ejkx = jk[jj][kk][0], ejky = jk[jj][kk][1], ejkz = jk[jj][kk][2];
                const double w = jk[jj][kk][3], gs = jk[jj][kk][4];
                const double c1 = eijx[q] * eikx + eijy[q] * eiky + eijz[q] * eikz;
                const double c2 = eijx[q] * ejkx + eijy[q] * ejky + eijz[q] * ejkz;
                const double c3 = eikx * ejkx + eiky * ejky + eikz * ejkz;
                const double num = (tij[q] * tik) * w * (1.0 - 3.0 * (c1 * c2 * c3));
                double term = num / (gi + gs);
                if (jkmol[jj][kk] == moli) term = 0.0;  // all three on one molecule
                if (tij[q] == 0.0 || tik == 0.0 || w == 0.0) term = 0.0;  // not i < j < k, or a site without the term
                acc += term;
            }
        }
    }
    block_sum_store<kAtWaves>(acc, red, out);
}

}  // namespace mpmc
