// device_common.h -- shared device-side types and helpers (gfx950, wave64, fp64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "step_pods.h"  // DirtyBlocks, SweepParams, BlockList, GsBuild: kernel arguments the host's plans fill in

namespace mpmc {

// reference src/include/defines.h:7-61
constexpr double kHBAR2 = 1.11211999e-68;
constexpr double kHBAR4 = 1.23681087e-136;
constexpr double kKB = 1.3806503e-23;
constexpr double kKB2 = 1.90619525e-46;
constexpr double kM2A2 = 1.0e20;
constexpr double kM2A4 = 1.0e40;
constexpr double kAMU2KG = 1.66053873e-27;
constexpr double kDEBYE2SKA = 85.10597636;
constexpr double kMAXVALUE = 1.0e40;
constexpr double kSMALL_dR = 1.0e-12;
constexpr int kMAX_ITERATION_COUNT = 128;
constexpr double kPI = 3.14159265358979323846;
constexpr double kOneOverSqrtPi = 0.56418958354;  // reference src/polarization/thole_field.c:10

constexpr int kWave = 64;

enum AtomFlag : int { kFrozen = 1, kValid = 2 };

// Periodic cell, passed by value (lands in SGPRs / kernarg).
struct DevBox {
    double b[3][3];   // basis, rows = lattice vectors
    double rb[3][3];  // reciprocal_basis (matrix inverse), reference src/energy/pbc.c:47-63
    double cutoff;
    double volume;
    float fb[3][3];   // single-precision copies for the cutoff pre-filter
    float frb[3][3];
    float rc2_pre;    // (cutoff + 0.01 A)^2
    int screen64;     // some |coordinate| is too large for the fp32 screen: screen on fp64 displacements (see below)
    float half_tie32; // 0.5 - tie32: a fractional displacement this far from the integer it rounds to may round the other way
    double tie64;     // 2^-49 * max |rb|: the same guard for the fp64 screen, per A of |dx| + |dy| + |dz|
    int tie_guard;    // the cell is not orthorhombic: the screens apply the half-integer guard (see below)
};

// SoA view of the configuration resident in HBM.  All arrays have npad entries
// (npad = n rounded up to 64); pad atoms carry flags = 0, q = alpha = eps = sig = 0.
// Coordinates of the atoms moved since the last energy(), by value in the kernel arguments (kernels_polar.h:
// apply_moves_kernel; kernels_coef.h / kernels_pair.h: the kernels a move can ride in).
constexpr int kMaxMoves = 32;
struct MoveList {
    int n;
    int idx[kMaxMoves];
    double x[kMaxMoves], y[kMaxMoves], z[kMaxMoves];
};
struct MoveTargets {  // where a kernel that carries the move writes it (what apply_moves_kernel writes)
    double *x, *y, *z;
    const int *slot_of_atom;
    double *px, *py, *pz;
};

struct DevAtoms {
    const double *x, *y, *z;
    const double *q, *alpha, *eps, *sig, *molmass;
    const int *mol;
    const int *flags;
    int n, npad;
};

// position of atom i: from the step's move when it carries one for i, else from memory
__device__ __forceinline__ void moved_position(const DevAtoms &a, const MoveList &m, int i, double &x, double &y,
                                               double &z) {
    x = a.x[i];
    y = a.y[i];
    z = a.z[i];
    for (int e = 0; e < m.n; ++e) {
        if (m.idx[e] == i) {
            x = m.x[e];
            y = m.y[e];
            z = m.z[e];
        }
    }
}

// Minimum image exactly as the reference evaluates it (src/energy/pairs.c:230-290):
// same operation order, no FMA contraction, so the lattice translation picked by
// rint() -- and therefore r, rimg, dimg -- is bit-identical to the CPU path even for
// pairs sitting exactly on a half-box tie (common for framework atoms on special positions).
__device__ __forceinline__ void minimum_image(const DevBox &bx, double dx, double dy, double dz, double &r,
                                              double &rimg, double &ox, double &oy, double &oz) {
#pragma clang fp contract(off)
    double i0 = bx.rb[0][0] * dx;
    i0 = i0 + bx.rb[1][0] * dy;
    i0 = i0 + bx.rb[2][0] * dz;
    double i1 = bx.rb[0][1] * dx;
    i1 = i1 + bx.rb[1][1] * dy;
    i1 = i1 + bx.rb[2][1] * dz;
    double i2 = bx.rb[0][2] * dx;
    i2 = i2 + bx.rb[1][2] * dy;
    i2 = i2 + bx.rb[2][2] * dz;
    i0 = rint(i0);
    i1 = rint(i1);
    i2 = rint(i2);
    double t0 = bx.b[0][0] * i0;
    t0 = t0 + bx.b[1][0] * i1;
    t0 = t0 + bx.b[2][0] * i2;
    double t1 = bx.b[0][1] * i0;
    t1 = t1 + bx.b[1][1] * i1;
    t1 = t1 + bx.b[2][1] * i2;
    double t2 = bx.b[0][2] * i0;
    t2 = t2 + bx.b[1][2] * i1;
    t2 = t2 + bx.b[2][2] * i2;
    double ex = dx - t0, ey = dy - t1, ez = dz - t2;
    double r2 = dx * dx;
    r2 = r2 + dy * dy;
    r2 = r2 + dz * dz;
    double ri2 = ex * ex;
    ri2 = ri2 + ey * ey;
    ri2 = ri2 + ez * ez;
    r = sqrt(r2);
    double ri = sqrt(ri2);
    if (ri != ri) {  // isnan(ri) fallback, pairs.c:279
        rimg = r;
        ox = dx;
        oy = dy;
        oz = dz;
    } else {
        rimg = ri;
        ox = ex;
        oy = ey;
        oz = ez;
    }
}

// Same arithmetic, but returns the SQUARED distances so that callers can apply the cutoff before
// paying for an fp64 sqrt (most pairs of a big box lie outside it).  sqrt(r2)/sqrt(ri2) of the
// returned values are bit-identical to r/rimg of minimum_image().
__device__ __forceinline__ void minimum_image_sq(const DevBox &bx, double dx, double dy, double dz, double &r2o,
                                                 double &ri2o, double &ox, double &oy, double &oz) {
#pragma clang fp contract(off)
    double i0 = bx.rb[0][0] * dx;
    i0 = i0 + bx.rb[1][0] * dy;
    i0 = i0 + bx.rb[2][0] * dz;
    double i1 = bx.rb[0][1] * dx;
    i1 = i1 + bx.rb[1][1] * dy;
    i1 = i1 + bx.rb[2][1] * dz;
    double i2 = bx.rb[0][2] * dx;
    i2 = i2 + bx.rb[1][2] * dy;
    i2 = i2 + bx.rb[2][2] * dz;
    i0 = rint(i0);
    i1 = rint(i1);
    i2 = rint(i2);
    double t0 = bx.b[0][0] * i0;
    t0 = t0 + bx.b[1][0] * i1;
    t0 = t0 + bx.b[2][0] * i2;
    double t1 = bx.b[0][1] * i0;
    t1 = t1 + bx.b[1][1] * i1;
    t1 = t1 + bx.b[2][1] * i2;
    double t2 = bx.b[0][2] * i0;
    t2 = t2 + bx.b[1][2] * i1;
    t2 = t2 + bx.b[2][2] * i2;
    const double ex = dx - t0, ey = dy - t1, ez = dz - t2;
    double r2 = dx * dx;
    r2 = r2 + dy * dy;
    r2 = r2 + dz * dz;
    double ri2 = ex * ex;
    ri2 = ri2 + ey * ey;
    ri2 = ri2 + ez * ez;
    r2o = r2;
    if (ri2 != ri2) {  // isnan(ri) fallback, pairs.c:279 (sqrt(NaN) is NaN and ri2 is never negative)
        ri2o = r2;
        ox = dx;
        oy = dy;
        oz = dz;
    } else {
        ri2o = ri2;
        ox = ex;
        oy = ey;
        oz = ez;
    }
}

// Cheap single-precision screen for the cutoff-limited pair kernels: in a 40 A box with an 8 A cutoff
// 97 % of the pairs lie outside the cutoff, and the exact fp64 minimum image (no FMA contraction, ~46
// fp64 operations) is what those kernels spend their time on.  The screen evaluates the same minimum
// image in fp32 (~30 operations at twice the rate) and must keep EVERY pair the exact test accepts; pairs that
// pass are decided by the exact fp64 path as before, so the screen never changes a result, it can only lose one.
//
// Why it loses none, for every cell shape.  Let f_k be the fractional displacement the exact path hands to rint()
// and f'_k the screen's.  Two cases:
//  (a) rint(f'_k) == rint(f_k) for k = 0..2: both paths measure the SAME lattice image.  The reference never wraps
//      atom->pos (wrapall() only fills wrapped_pos, src/io/output.c:142-183) and a PQR may sit anywhere, so the host
//      tracks max |coordinate| over everything it sends (upload / update_atoms / insert_molecule / scale_box) and
//      keeps the fp32 screen to |x| <= kScreen32MaxCoord = 2048 A.  There an fp32 coordinate is off by <= 2^-13 A and
//      a coordinate difference by <= 3 * 2^-13 A (two roundings of the inputs, one of the difference, |d| < 4096);
//      the image translation sum_q fb[q][k] * i_q (|term| < 4096) adds <= ~3 * 2^-12 A: the screened distance is off
//      by < 2e-3 A, well inside the 0.01 A margin of rc2_pre.
//  (b) some rint(f'_k) != rint(f_k): the screen measured ANOTHER image.  Rounding can only flip rint() when f_k lies
//      within the error e_k = |f'_k - f_k| of a half-integer (bound below).
//      Orthorhombic cell (every off-diagonal basis entry exactly 0; S_k = 1 / L_k): the other image mirrors component k
//      of the displacement, (0.5 - u) L_k <-> (0.5 + u) L_k with u <= e_k, so the distance changes by at most
//      2 e_k L_k <= 22 * 2^-13 = 2.7e-3 A; with the 2e-3 A of (a) that is still under the 0.01 A margin, and the
//      screen needs nothing more.  DevBox::tie_guard = 0 there (wave-uniform: a kernel argument), so the cubic and
//      orthorhombic boxes, bench.py's among them, run the screen they always ran.
//      Sheared cell: the r^2 of the two images differ by 2 (s1 a.b + s2 a.c), which is of order L^2 -- the wrong image can
//      sit many A outside the cutoff while the right one is inside.  There (tie_guard = 1) the screen KEEPS, without
//      looking at the distance, every pair that has a component with 0.5 - |f'_k - rint(f'_k)| <= tie32, tie32 >= max_k e_k.
//      Bound on e_k (dev_box(), engine.hip): with S_k = sum_q |rb[q][k]|,
//        input error        3 * 2^-13 A per difference                       -> S_k * 3 * 2^-13
//        frb rounded to fp32, three products, two additions (fused or not): four relative errors of 2^-24 on terms
//        of magnitude <= S_k * 4096                                           -> S_k * 4 * 2^-12
//      e_k <= 11 * 2^-13 * S_k; tie32 = 1.25 * 11 * 2^-13 * max_k S_k (5e-5 .. 1e-4 in a 25 A cell, so well under
//      1e-3 of all pairs are kept on this ground -- the exact path drops them after its minimum image).  f'_k -
//      rint(f'_k) is exact in fp32 (Sterbenz), and the exact path's own error in f_k (~1e-13) vanishes in the 1.25.
// Above 2048 A the host sets DevBox::screen64 and the screen works on fp64 displacements, lattice reduction included.
// It is compiled with FMA contraction and minimum_image_sq() without, so the two can still round an f_k to different
// sides of a half-integer: the same guard applies with tie64 = 2^-48 + 2^-49 * max|rb| * (|dx| + |dy| + |dz|) (six
// roundings of 2^-53 relative to the largest partial sum, times 2.7).  In case (a) this screen's distance is exact to
// ~1e-10 A up to |x| ~ 1e5 A and never worse than the exact path's own resolution.
// tests/test_gpu_screen_edges.py holds both screens to this with near-tie pairs in sheared cells.
constexpr double kScreen32MaxCoord = 2048.0;
__device__ __forceinline__ bool prefilter_within_f(const DevBox &bx, float dx, float dy, float dz);
__device__ __forceinline__ bool prefilter_within_d(const DevBox &bx, double dx, double dy, double dz) {
    const double f0 = bx.rb[0][0] * dx + bx.rb[1][0] * dy + bx.rb[2][0] * dz;
    const double f1 = bx.rb[0][1] * dx + bx.rb[1][1] * dy + bx.rb[2][1] * dz;
    const double f2 = bx.rb[0][2] * dx + bx.rb[1][2] * dy + bx.rb[2][2] * dz;
    const double i0 = rint(f0), i1 = rint(f1), i2 = rint(f2);
    const double ex = dx - (bx.b[0][0] * i0 + bx.b[1][0] * i1 + bx.b[2][0] * i2);
    const double ey = dy - (bx.b[0][1] * i0 + bx.b[1][1] * i1 + bx.b[2][1] * i2);
    const double ez = dz - (bx.b[0][2] * i0 + bx.b[1][2] * i1 + bx.b[2][2] * i2);
    const double r2 = ex * ex + ey * ey + ez * ez;
    bool keep = !(r2 > (double)bx.rc2_pre);  // NaN passes: the exact path handles it
    if (bx.tie_guard) {                      // sheared cell: case (b) above
        const double edge = fmax(fmax(fabs(f0 - i0), fabs(f1 - i1)), fabs(f2 - i2));  // distance from the integer picked
        const double tie = 0x1p-48 + bx.tie64 * (fabs(dx) + fabs(dy) + fabs(dz));
        keep = keep || (edge >= 0.5 - tie);
    }
    return keep;
}
// same screen on single-precision displacements (coordinates rounded to fp32 when a tile is staged)
__device__ __forceinline__ bool prefilter_within_f(const DevBox &bx, float dx, float dy, float dz) {
    const float f0 = bx.frb[0][0] * dx + bx.frb[1][0] * dy + bx.frb[2][0] * dz;
    const float f1 = bx.frb[0][1] * dx + bx.frb[1][1] * dy + bx.frb[2][1] * dz;
    const float f2 = bx.frb[0][2] * dx + bx.frb[1][2] * dy + bx.frb[2][2] * dz;
    const float i0 = rintf(f0), i1 = rintf(f1), i2 = rintf(f2);
    const float ex = dx - (bx.fb[0][0] * i0 + bx.fb[1][0] * i1 + bx.fb[2][0] * i2);
    const float ey = dy - (bx.fb[0][1] * i0 + bx.fb[1][1] * i1 + bx.fb[2][1] * i2);
    const float ez = dz - (bx.fb[0][2] * i0 + bx.fb[1][2] * i1 + bx.fb[2][2] * i2);
    const float r2 = ex * ex + ey * ey + ez * ez;
    bool keep = !(r2 > bx.rc2_pre);  // NaN passes: the exact path handles it
    if (bx.tie_guard) {              // sheared cell: case (b) above
        const float edge = fmaxf(fmaxf(fabsf(f0 - i0), fabsf(f1 - i1)), fabsf(f2 - i2));  // one v_max3_f32 with |.| modifiers
        keep = keep || (edge >= bx.half_tie32);
    }
    return keep;
}

// Squared-distance pre-filter for the cutoff tests `rimg - 1e-12 < rc` / `!(rimg > rc)`: any pair that
// passes those tests has rimg^2 below this bound, so pairs above it can be dropped before the sqrt.
__device__ __forceinline__ double cutoff_prefilter_sq(double rc) {
    const double h = rc + 1.0e-9;
    return h * h;
}

// Broadcast lane `src` (wave-uniform index) of a double through SGPRs: two v_readlane_b32 instead of
// the two ds_bpermute_b32 (LDS crossbar round trips) that a generic __shfl costs.
__device__ __forceinline__ double readlane_f64(double v, int src) {
    const int s = __builtin_amdgcn_readfirstlane(src);
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), s);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), s);
    return __hiloint2double(hi, lo);
}

// 64-lane butterfly sum; every lane ends with the total (fixed order => deterministic).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}

}  // namespace mpmc
