// step_pods.h -- the kernel-argument structs that the host's step plans (step_plan.h) fill in, and their constants.
// Plain C++: no HIP header, nothing device-specific.  The kernels that read them say what every member means to them
// (device_common.h, kernels_polar.h, kernels_gs_chain.h).
#pragma once

namespace mpmc {

// 64-atom blocks (atom order) that hold an atom moved since the last energy(); carried in the kernel
// arguments.  n == 0 means "everything": the tiled pair/field kernels then cover their whole grid,
// otherwise only the tiles that touch one of these blocks (their partial sums persist in HBM, and a
// tile's partial is a function of its two blocks' atoms only, so the result is bit-identical).
constexpr int kMaxDirtyBlocks = 16;
struct DirtyBlocks {
    int n;
    int blk[kMaxDirtyBlocks];
};

struct SweepParams {
    double w_new;    // weight of new_mu in mu_out (1 for plain Jacobi)
    double w_old;    // weight of old mu
    int want_rrms;   // polar_rrms || polar_precision > 0
    int want_err;    // polar_precision > 0: the host reads max (new-old)^2 after every sweep
    int err_slot;    // index into errmax[] for this iteration
    int skip_sums;   // 1: the block's energy / RRMS sums are not wanted (an iteration that is known not to be the last)
    // Fixed-count plain Jacobi with the last sweep deferred (pair_finish_kernel): which of the
    // extra jobs this sweep's finish does.  0 everywhere else.
    int energy_mode = 0;      // kEnergyStoreSums | kEnergyMid [| kEnergyPrevSums]
};
// n sweeps, m = ceil(n / 2); s_k = T mu_{k-1} are the sums of sweep k
constexpr int kEnergyStoreSums = 1;  // sweep n - m of an odd n: keep the sums s_{n-m} per site (SweepView::tmu0)
constexpr int kEnergyMid = 2;        // sweep m: the block's energy share is sum_i (mu_m.E - (mu_m - mu_{m-1}).s_{n-m})
constexpr int kEnergyPrevSums = 4;   // with kEnergyMid, odd n: s_{n-m} are the stored sums, not this sweep's own

constexpr int kGsMaxLag = 4;              // cached lags: P (1), Q (2), and up to two more

// ---- the chain kernel's workgroups (kernels_gs_chain.h): block u has max(1, min(u, nlag)) of them -- main(u) and one
// auxiliary workgroup aux(u, k) per lag k = 2 .. min(u, nlag).  Number of workgroups in front of block t's (= tickets before
// aux(t, nlag)), and of the whole chain with t = nb.  (constexpr: the device compiler takes a constexpr function for the
// host and the device alike, so the kernel, the host's grid size and the CPU check of tests/step_plan_check.cpp run the
// same text and this header still names nothing of HIP.)
constexpr int gs_chain_ticket_base(int t, int nlag) {
    // block u has 1 + min(u, nlag) - 1 ... = max(1, min(u, nlag)) workgroups
    int n = 0;
    for (int u = 0; u < t && u < nlag; ++u) n += (u < 1 ? 1 : u);
    if (t > nlag) n += (t - nlag) * nlag;
    return n;
}

constexpr int kMaxBlockList = 48;
struct BlockList {
    int n;
    int blk[kMaxBlockList];
};

// What one launch of gs_block_inverse_kernel rebuilds (kernels_gs_chain.h says which z-slice reads which list).
struct GsBuild {
    BlockList inv;             // z-slice 0: M_t of these blocks
    BlockList own;             // z-slice 1: every L(k)_t, k = 1 .. min(t, nlag), of these blocks (their M_t changed), ONE pass
    BlockList nb[kGsMaxLag];   // z-slice 1 + k: L(k)_t alone (the tile (t-k, t) changed: t = a changed block + k)
    double *Minv;
    double *Lnb[kGsMaxLag];
    int nlag;
    int nb_all;                // > 0: every block of the view (slices 0 and 1 take blockIdx.y as the block, the others nothing)
};

}  // namespace mpmc
