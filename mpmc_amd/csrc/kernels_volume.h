// kernels_volume.h -- the NPT volume move on the resident configuration (mpmc_hip_scale_box).
//
// The reference's volume_change() / revert_volume_change() (mc_moves.c:168-248) scale the basis and shift every
// molecule rigidly by (scaled COM - COM): one fp64 addition per coordinate of every atom, frozen molecules
// included.  The host computes the per-molecule displacement with its own COMs (the engine holds molecular
// masses only, and a device reduction would not round like update_com()); the device performs the very same
// addition, so that device coordinates stay bit-identical to the host's lists.
#pragma once

#include "device_common.h"

namespace mpmc {

constexpr int kShiftThreads = 256;

// grid = ceil(n / 256); one atom slot per thread.  mol[i] is the molecule's position in upload order (holes and
// pad slots carry negative ids and are not valid).  The compacted copy sweep view 0 reads follows along, as in
// apply_moves_kernel.
__global__ __launch_bounds__(kShiftThreads) void shift_molecules_kernel(
    int n, int n_molecules, const double *__restrict__ delta, const int *__restrict__ mol,
    const int *__restrict__ flags, double *__restrict__ x, double *__restrict__ y, double *__restrict__ z,
    const int *__restrict__ slot_of_atom, double *__restrict__ px, double *__restrict__ py,
    double *__restrict__ pz) {
    const int i = blockIdx.x * kShiftThreads + threadIdx.x;
    if (i >= n) return;
    if (!(flags[i] & kValid)) return;
    const int m = mol[i];
    if (m < 0 || m >= n_molecules) return;  // (never for a valid slot of an unedited upload: checked on the host)
    const double nx = x[i] + delta[3 * m + 0];
    const double ny = y[i] + delta[3 * m + 1];
    const double nz = z[i] + delta[3 * m + 2];
    x[i] = nx;
    y[i] = ny;
    z[i] = nz;
    const int s = slot_of_atom[i];
    if (s >= 0) {
        px[s] = nx;
        py[s] = ny;
        pz[s] = nz;
    }
}

// max |coordinate| over the valid slots (one workgroup): run only when the host's running bound on coord_max would
// cross kScreen32MaxCoord, to replace the bound -- which only grows -- by the true value.
__global__ __launch_bounds__(kShiftThreads) void coord_absmax_kernel(int n, const int *__restrict__ flags,
                                                                     const double *__restrict__ x,
                                                                     const double *__restrict__ y,
                                                                     const double *__restrict__ z,
                                                                     double *__restrict__ out) {
    __shared__ double part[kShiftThreads];
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += kShiftThreads) {
        if (!(flags[i] & kValid)) continue;
        const double v = fmax(fabs(x[i]), fmax(fabs(y[i]), fabs(z[i])));
        if (!(v <= m)) m = (v == v) ? v : INFINITY;  // (a NaN coordinate counts as "beyond the fp32 screen")
    }
    part[threadIdx.x] = m;
    __syncthreads();
    for (int s = kShiftThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

}  // namespace mpmc
