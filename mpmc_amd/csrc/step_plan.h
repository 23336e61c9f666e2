// step_plan.h -- the decisions of one evaluation that are plain functions of a few integers: which chain data a move
// invalidates, the ranked walk, what each Jacobi sweep's finish does, how the j-range of a tiled kernel is chunked, where
// an inserted molecule goes.  Host C++17 only, no HIP header: engine.hip / engine_polar.inc launch what these functions
// decide, and tests/test_step_plan.py holds them to their descriptions on a CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "step_pods.h"

namespace mpmc {

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- chunking: the j-range of npad atoms in chunks of whole 64-atom tiles, about `target` workgroups in all
struct ChunkPlan {
    int nchunk, chunk;  // chunks, atoms per chunk
};
static inline ChunkPlan chunk_plan(int npad, int target) {
    const int ntile = npad / 64;
    int nchunk = std::max(1, std::min(ntile, target / ntile));
    const int chunk = round_up((npad + nchunk - 1) / nchunk, 64);
    nchunk = (npad + chunk - 1) / chunk;
    return {nchunk, chunk};
}

// ---- atoms -> the 64-atom blocks they are in, each once (unused entries zero); false: more blocks than the list holds
static inline bool blocks_of(const std::vector<int> &atoms, DirtyBlocks &out) {
    memset(&out, 0, sizeof(out));
    for (int atom : atoms) {
        const int b = atom / 64;
        bool seen = false;
        for (int k = 0; k < out.n; ++k) seen |= (out.blk[k] == b);
        if (seen) continue;
        if (out.n == kMaxDirtyBlocks) {
            memset(&out, 0, sizeof(out));
            return false;
        }
        out.blk[out.n++] = b;
    }
    return true;
}

// ---- grand-canonical edits
// Where a molecule of `count` atoms goes: the most recent hole of exactly that size, else new slots at the end.  hole: its
// index in `holes`, or -1.  false: the context is full.
static inline bool place_molecule(const std::vector<std::pair<int, int>> &holes, int n, int max_atoms, int count, int &first,
                                  int &hole) {
    first = hole = -1;
    for (int h = (int)holes.size() - 1; h >= 0; --h)
        if (holes[h].second == count) {
            hole = h;
            first = holes[h].first;
            return true;
        }
    if (n + count > max_atoms) return false;
    first = n;
    return true;
}
// View slots an insertion at `first` appends: a polarizable site takes the atom slot's old view slot if it has one
// (never in the Gauss-Seidel modes, whose caller sends the whole sweep order anew).
static inline int count_new_view_slots(const std::vector<int> &slot_of_atom, bool gs_mode, int first, int count,
                                       const double *polarizability) {
    int new_view = 0;
    for (int i = 0; i < count; ++i) {
        const bool had = !gs_mode && first + i < (int)slot_of_atom.size() && slot_of_atom[first + i] >= 0;
        if (polarizability[i] != 0.0 && !had) ++new_view;
    }
    return new_view;
}

// ---- Jacobi-type sweeps
// the mixing weights of iteration k (thole_iterative.c:238-252)
static inline void mixing_weights(bool sor, bool esor, double gamma, int k, double &w_new, double &w_old) {
    w_new = 1.0;
    w_old = 0.0;
    if (sor) {
        w_new = gamma;
        w_old = 1.0 - gamma;
    } else if (esor) {
        w_old = std::exp(-gamma * k);
        w_new = 1.0 - w_old;
    }
}
// What the finish of Jacobi sweep `iteration` (1-based) of `max_iter` does.  defer: the solve leaves its last sweep to
// whoever asks for the dipoles (defer_last_sweep()), and U_pol comes from the finish of sweep m = ceil(n / 2)
// (pair_finish_kernel); no other finish of the call writes the block sums.
static inline SweepParams jacobi_sweep_params(int iteration, int max_iter, double precision, bool want_rrms, bool defer,
                                              double w_new, double w_old) {
    SweepParams sp;
    sp.w_new = w_new;
    sp.w_old = w_old;
    sp.want_rrms = want_rrms;
    sp.want_err = precision > 0.0;
    sp.err_slot = iteration;
    sp.skip_sums = (precision == 0.0 && iteration < max_iter) ? 1 : 0;
    const int mid = (max_iter + 1) / 2;
    if (defer) {
        const bool odd = max_iter & 1;
        sp.skip_sums = 1;
        if (odd && iteration == max_iter - mid) sp.energy_mode |= kEnergyStoreSums;
        if (iteration == mid) sp.energy_mode |= kEnergyMid | (odd ? kEnergyPrevSums : 0);
    }
    return sp;
}
// Is sweep `iteration` of a deferring solve recorded (PendingSweep) instead of launched?  Sweep n, and sweeps m + 1 .. n - 1
// once the record HAS gone out behind the finish of sweep m (published).
static inline bool sweep_is_pending(int iteration, int max_iter, bool defer, bool published) {
    const int mid = (max_iter + 1) / 2;
    return defer && (iteration == max_iter || (iteration > mid && published));
}

// ---- polar_gs_ranked: the ranked walk (update_ranking, thole_iterative.c:143-164).  The polarizable sites keep their
// relative order: a stable sort of view 0's order `v0idx` (atom indices) by descending metric rk[atom] -> perm[0 .. nv).
// The metric is a neighbour COUNT: a stable counting sort, O(n), instead of a comparison sort -- this runs on the host in
// the middle of a call, every grand-canonical step; anything that is not a count below 1024 takes std::stable_sort.
static inline void ranked_walk(const double *rk, const std::vector<int> &v0idx, int *perm) {
    const int nv = (int)v0idx.size();
    constexpr int kMaxRank = 1024;
    bool small = true;
    int cnt[kMaxRank + 1] = {0};
    for (int k = 0; k < nv && small; ++k) {
        const double r = rk[v0idx[k]];
        if (!(r >= 0.0 && r < kMaxRank && r == (double)(int)r)) small = false;
        else ++cnt[(int)r];
    }
    if (small) {
        int start[kMaxRank + 1];
        int acc = 0;
        for (int r = kMaxRank - 1; r >= 0; --r) {  // descending metric
            start[r] = acc;
            acc += cnt[r];
        }
        for (int k = 0; k < nv; ++k) perm[start[(int)rk[v0idx[k]]]++] = v0idx[k];
    } else {
        std::vector<int> walk(v0idx);
        std::stable_sort(walk.begin(), walk.end(), [rk](int x, int y) { return rk[x] > rk[y]; });
        std::copy(walk.begin(), walk.end(), perm);
    }
}

// ---- Gauss-Seidel chain data (kernels_gs_chain.h): what gs_block_inverse_kernel has to redo
static inline bool listed(const BlockList &l, int b) {
    for (int q = 0; q < l.n; ++q)
        if (l.blk[q] == b) return true;
    return false;
}
// The three block lists of `gb` (everything else in it zero) for a view of nt blocks with nlag cached lags.  fresh: the
// chain data were up to date before this call's changes -- which are the view slots `dirty` and, with tail >= 0, a new order
// from block `tail` on.  A block whose own atoms changed: M_b and every L(k)_b (`inv`, `own`: one pass); the blocks k
// places behind it: L(k)_{b+k} (`nb[k-1]`).  Returns full, with the lists empty and nb_all = nt: everything is rebuilt (not
// fresh, or more changed blocks than a list holds).
static inline bool plan_chain_build(bool fresh, int tail, int nt, int nlag, const int *dirty, int nd, GsBuild &gb) {
    memset(&gb, 0, sizeof(gb));
    bool full = !fresh;
    auto add_block = [&](int b) {
        if (listed(gb.inv, b)) return;
        if (gb.inv.n == kMaxBlockList) {
            full = true;
            return;
        }
        gb.inv.blk[gb.inv.n++] = b;
        if (b >= 1) gb.own.blk[gb.own.n++] = b;
        for (int k = 1; k <= nlag; ++k) {
            const int tt = b + k;
            if (tt >= nt || listed(gb.nb[k - 1], tt)) continue;
            if (gb.nb[k - 1].n == kMaxBlockList) {
                full = true;
                return;
            }
            gb.nb[k - 1].blk[gb.nb[k - 1].n++] = tt;
        }
    };
    if (fresh && tail >= 0)  // every block of the re-ordered tail (the tiles that join it to the prefix are theirs)
        for (int b = tail; b < nt && !full; ++b) add_block(b);
    if (fresh)
        for (int k = 0; k < nd && !full; ++k) add_block(dirty[k] / 64);
    // (a block listed in `own` has all its lags rebuilt there: drop it from the single-lag lists)
    for (int k = 0; k < nlag && !full; ++k) {
        BlockList &l = gb.nb[k];
        int m = 0;
        for (int q = 0; q < l.n; ++q)
            if (!listed(gb.own, l.blk[q])) l.blk[m++] = l.blk[q];
        l.n = m;
    }
    if (full) {
        memset(&gb, 0, sizeof(gb));
        gb.nb_all = nt;
    }
    return full;
}

// Waves per workgroup of gs_block_inverse_kernel for `nsolve` passes: 192 / WAVES workgroups of WAVES waves per pass (each
// holds ~97 KB of LDS: one per CU).  4 waves x 48 workgroups finish a pass soonest (the moved atoms' blocks of view 0 are
// on the step's critical path), but only while all of them find a CU at once: a move rebuilds M_b, {L(k)_b},
// L(1)_b+1 .. L(nlag)_b+nlag = 2 + nlag passes; when two blocks moved (or the view's tail is re-ordered) 8 waves x 24 keep
// the launch to one dispatch round, and a rebuild of many blocks is a matter of throughput: 16 waves x 12 repeat the tile
// expansion least often.
// The other view's rebuild, in the side stream, runs BESIDE the main stream's chain kernel, whose `chain_wgs` workgroups
// need a CU each as well (both kinds own a CU's LDS): it takes the fastest geometry that leaves the chain its CUs -- with
// 8 x 24 and round 2's seven passes the two launches together oversubscribed the 256 CUs and the chain took 85 us instead
// of 73; always 16 x 12 (a few dozen CUs, but 48 us per launch) left the main stream of a 1 024-atom step, whose sweeps
// are 23 us long, waiting 60 us for the ranked view at its view switch.  (side_waves = 16, option gs_side_waves: always 16.)
static inline int inverse_waves(int nsolve, bool main_stream, int side_waves, int chain_wgs) {
    int waves;
    if (main_stream)
        waves = (48 * nsolve <= 256) ? 4 : ((24 * nsolve <= 256) ? 8 : 16);
    else if (side_waves == 16)
        waves = 16;
    else
        waves = (48 * nsolve + chain_wgs <= 256) ? 4 : ((24 * nsolve + chain_wgs <= 256) ? 8 : 16);
    return waves;
}

}  // namespace mpmc
