// kernels_cavity.h -- the cavity grid of cavity_bias (reference src/mc/cavity.c:17-179).
//
// G^3 grid points inside the cell; occ[g] = number of atoms closer than cavity_radius to point g (no minimum image:
// the caller passes wrapped positions); a point is open when occ[g] == 0; open_list[] = the open points in ascending
// flat index g = (i G + j) G + k; a dart hits when it is closer than cavity_radius to some open point.  Everything
// counted here is an integer, so no result depends on the order of a sum.
//
// The comparison.  The reference decides `sqrt(s) < R` with a correctly rounded sqrt.  sqrt is monotone, so with T = the
// smallest double whose (host, correctly rounded) sqrt is >= R, sqrt(s) < R holds exactly when s < T: the device compares
// squares and never takes a root.  s is formed in the reference's operation order without FMA contraction
// (cavity_dist2), as minimum_image() in device_common.h forms its sums.  A NaN s fails both tests.
#pragma once

#include "device_common.h"

namespace mpmc {

constexpr int kCavThreads = 256;   // grid points (or darts) per workgroup = positions staged through LDS per chunk
constexpr int kCavMaxGrid = 64;    // cavity_grid_size: 64^3 points = 1024 workgroups = the scan kernel's reach
constexpr int kCavMaxEdit = 16;    // points that leave / enter in one edit
constexpr int kCavMaxBlocks = kCavMaxGrid * kCavMaxGrid * kCavMaxGrid / kCavThreads;

enum CavCounter { CAV_OPEN = 0, CAV_NCOUNTER };
// the record in mapped host memory (doubles, so that the host waits for it like for the result record)
enum CavRecord { CR_OPEN = 0, CR_HITS, CR_PICK_G, CR_PICK_X, CR_PICK_Y, CR_PICK_Z, CR_SEQ, CR_COUNT };

// by value in the kernel arguments
struct CavityFrac {  // (i + 1) / (G + 1), i = 0 .. G - 1, divided on the host
    double c[kCavMaxGrid];
};
struct CavityBasis {
    double b[3][3];  // rows = lattice vectors
};
struct CavityEdit {
    int n_out, n_in;
    double out[kCavMaxEdit][3], in[kCavMaxEdit][3];
};

// ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2, every operation rounded (cavity.c:154-156, :59-61)
__device__ __forceinline__ double cavity_dist2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    double s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    return s;
}

// grid = ceil(P / 256); one grid point per thread.  pos[p] = ((b[0][p] c0 + b[1][p] c1) + b[2][p] c2) - 0.5 b[0][p]
// - 0.5 b[1][p] - 0.5 b[2][p], left to right (cavity.c:140-148).
__global__ __launch_bounds__(kCavThreads) void cavity_points_kernel(int G, CavityFrac f, CavityBasis bs,
                                                                    double *__restrict__ gx, double *__restrict__ gy,
                                                                    double *__restrict__ gz) {
#pragma clang fp contract(off)
    const int g = blockIdx.x * kCavThreads + threadIdx.x;
    if (g >= G * G * G) return;
    const double c0 = f.c[g / (G * G)], c1 = f.c[(g / G) % G], c2 = f.c[g % G];
    double v[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        double t = bs.b[0][p] * c0;
        t = t + bs.b[1][p] * c1;
        t = t + bs.b[2][p] * c2;
        t = t - 0.5 * bs.b[0][p];
        t = t - 0.5 * bs.b[1][p];
        t = t - 0.5 * bs.b[2][p];
        v[p] = t;
    }
    gx[g] = v[0];
    gy[g] = v[1];
    gz[g] = v[2];
}

// The from-scratch occupancy.  grid = ceil(P / 256); a workgroup takes 256 grid points, one per lane, and walks the n
// atoms in chunks of 256 staged through LDS (every lane reads the same staged atom: a broadcast).
__global__ __launch_bounds__(kCavThreads) void cavity_bin_kernel(int P, const double *__restrict__ gx,
                                                                 const double *__restrict__ gy,
                                                                 const double *__restrict__ gz, int n,
                                                                 const double *__restrict__ ax,
                                                                 const double *__restrict__ ay,
                                                                 const double *__restrict__ az, double T,
                                                                 int *__restrict__ occ) {
    __shared__ double sx[kCavThreads], sy[kCavThreads], sz[kCavThreads];
    const int g = blockIdx.x * kCavThreads + threadIdx.x;
    const bool valid = g < P;
    const double px = valid ? gx[g] : 0.0, py = valid ? gy[g] : 0.0, pz = valid ? gz[g] : 0.0;
    int cnt = 0;
    for (int base = 0; base < n; base += kCavThreads) {
        const int m = min(kCavThreads, n - base);
        if ((int)threadIdx.x < m) {
            sx[threadIdx.x] = ax[base + threadIdx.x];
            sy[threadIdx.x] = ay[base + threadIdx.x];
            sz[threadIdx.x] = az[base + threadIdx.x];
        }
        __syncthreads();
        for (int a = 0; a < m; ++a) cnt += (cavity_dist2(px, py, pz, sx[a], sy[a], sz[a]) < T) ? 1 : 0;
        __syncthreads();
    }
    if (valid) occ[g] = cnt;
}

// number of set flags in the workgroup (every thread gets it); `scratch` holds one int per wave
__device__ __forceinline__ int cavity_block_count(bool flag, int *scratch) {
    const unsigned long long ballot = __ballot(flag);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kCavThreads / 64; ++w) total += scratch[w];
    return total;
}

// The edit, and the first phase of the compaction.  grid = ceil(P / 256); one grid point per thread:
// occ += (entering points within R) - (leaving points within R), then block_open[b] = open points of this workgroup.
// With an empty edit nothing is written to occ.
__global__ __launch_bounds__(kCavThreads) void cavity_edit_kernel(int P, const double *__restrict__ gx,
                                                                  const double *__restrict__ gy,
                                                                  const double *__restrict__ gz, CavityEdit ed, double T,
                                                                  int *__restrict__ occ, int *__restrict__ block_open) {
    __shared__ int scratch[kCavThreads / 64];
    const int g = blockIdx.x * kCavThreads + threadIdx.x;
    bool open = false;
    if (g < P) {
        int o = occ[g];
        if (ed.n_in + ed.n_out > 0) {
            const double px = gx[g], py = gy[g], pz = gz[g];
            for (int e = 0; e < ed.n_in; ++e)
                o += (cavity_dist2(px, py, pz, ed.in[e][0], ed.in[e][1], ed.in[e][2]) < T) ? 1 : 0;
            for (int e = 0; e < ed.n_out; ++e)
                o -= (cavity_dist2(px, py, pz, ed.out[e][0], ed.out[e][1], ed.out[e][2]) < T) ? 1 : 0;
            occ[g] = o;
        }
        open = o == 0;
    }
    const int total = cavity_block_count(open, scratch);
    if (threadIdx.x == 0) block_open[blockIdx.x] = total;
}

// Second phase: one workgroup, block_off[b] = open points in front of workgroup b (exclusive scan of up to
// kCavMaxBlocks counts: thread t sums blocks [t per, (t + 1) per), the 256 sums are scanned in LDS).  It also
// publishes the total and clears the darts' hit flags.
__global__ __launch_bounds__(kCavThreads) void cavity_scan_kernel(int nb, const int *__restrict__ block_open,
                                                                  int *__restrict__ block_off,
                                                                  int *__restrict__ counters, int n_darts,
                                                                  int *__restrict__ dart_hit) {
    __shared__ int part[kCavThreads];
    for (int i = threadIdx.x; i < n_darts; i += kCavThreads) dart_hit[i] = 0;
    const int per = (nb + kCavThreads - 1) / kCavThreads;
    const int lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    int mine = 0;
    for (int b = lo; b < hi; ++b) mine += block_open[b];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kCavThreads; d <<= 1) {  // inclusive scan
        const int add = ((int)threadIdx.x >= d) ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int run = part[threadIdx.x] - mine;
    for (int b = lo; b < hi; ++b) {
        block_off[b] = run;
        run += block_open[b];
    }
    if (threadIdx.x == kCavThreads - 1) counters[CAV_OPEN] = part[kCavThreads - 1];
}

// Third phase: grid = ceil(P / 256); the open points of workgroup b go to open_list[block_off[b] ...] in ascending g.
__global__ __launch_bounds__(kCavThreads) void cavity_scatter_kernel(int P, const int *__restrict__ occ,
                                                                     const int *__restrict__ block_off,
                                                                     int *__restrict__ open_list) {
    __shared__ int wave_open[kCavThreads / 64];
    const int g = blockIdx.x * kCavThreads + threadIdx.x;
    const bool open = g < P && occ[g] == 0;
    const unsigned long long ballot = __ballot(open);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_open[wave] = __popcll(ballot);
    __syncthreads();
    if (!open) return;
    int at = block_off[blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += wave_open[w];
    open_list[at] = g;  // at < number of open points <= P
}

// The darts.  grid = (ceil(n_darts / 256), slices); one dart per lane; workgroup (bx, by) tests its 256 darts against the
// 256-point chunks by, by + slices, ... of the open list, staged through LDS -- the darts alone are ~120 waves, far fewer
// than the device holds, so the open list is shared out as well.  A lane that has its hit skips the chunks that follow;
// inside a chunk the tests are branch-free.  dart = [n_darts][3]; dart_hit[i] (cleared by the scan kernel) becomes 1 when
// some workgroup found dart i inside an open sphere: every writer stores the same 1.
__global__ __launch_bounds__(kCavThreads) void cavity_darts_kernel(int n_darts, const double *__restrict__ dart,
                                                                   const int *__restrict__ open_list,
                                                                   const double *__restrict__ gx,
                                                                   const double *__restrict__ gy,
                                                                   const double *__restrict__ gz, double T,
                                                                   const int *__restrict__ counters,
                                                                   int *__restrict__ dart_hit) {
    __shared__ double sx[kCavThreads], sy[kCavThreads], sz[kCavThreads];
    const int n_open = counters[CAV_OPEN];
    const int i = blockIdx.x * kCavThreads + threadIdx.x;
    const bool valid = i < n_darts;
    const double x = valid ? dart[3 * (size_t)i] : 0.0, y = valid ? dart[3 * (size_t)i + 1] : 0.0,
                 z = valid ? dart[3 * (size_t)i + 2] : 0.0;
    bool hit = false;
    for (int base = blockIdx.y * kCavThreads; base < n_open; base += gridDim.y * kCavThreads) {  // (block-uniform bounds)
        const int m = min(kCavThreads, n_open - base);
        if ((int)threadIdx.x < m) {
            const int g = open_list[base + threadIdx.x];
            sx[threadIdx.x] = gx[g];
            sy[threadIdx.x] = gy[g];
            sz[threadIdx.x] = gz[g];
        }
        __syncthreads();
        if (valid && !hit) {
            int found = 0;
#pragma unroll 8
            for (int a = 0; a < m; ++a) found |= (cavity_dist2(x, y, z, sx[a], sy[a], sz[a]) < T) ? 1 : 0;
            hit = found != 0;
        }
        __syncthreads();
    }
    if (hit) dart_hit[i] = 1;
}

// One workgroup: the darts' flags are counted, the counts go to the mapped record, the sequence number last.
__global__ __launch_bounds__(kCavThreads) void cavity_publish_kernel(int n_darts, const int *__restrict__ dart_hit,
                                                                     const int *__restrict__ counters,
                                                                     volatile double *rec, double seq) {
    __shared__ int part[kCavThreads];
    int mine = 0;
    for (int i = threadIdx.x; i < n_darts; i += kCavThreads) mine += dart_hit[i];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int s = kCavThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    rec[CR_OPEN] = (double)counters[CAV_OPEN];
    rec[CR_HITS] = (double)part[0];
    __threadfence_system();
    rec[CR_SEQ] = seq;
}

// One thread: the index-th open point (the host has checked index < open) to the mapped record.
__global__ __launch_bounds__(64) void cavity_pick_kernel(int index, const int *__restrict__ open_list,
                                                         const double *__restrict__ gx, const double *__restrict__ gy,
                                                         const double *__restrict__ gz, volatile double *rec,
                                                         double seq) {
    if (threadIdx.x != 0) return;
    const int g = open_list[index];
    rec[CR_PICK_G] = (double)g;
    rec[CR_PICK_X] = gx[g];
    rec[CR_PICK_Y] = gy[g];
    rec[CR_PICK_Z] = gz[g];
    __threadfence_system();
    rec[CR_SEQ] = seq;
}

}  // namespace mpmc
