// (half-tile workgroups in pair_sweep_kernel when a CU gets only a few tiles: see the measurement in DESIGN.md section 3)
static constexpr bool kSweepSplitAuto = false;
// engine_polar.inc -- orchestration of polar() (reference src/energy/polar.c:31-135 and
// src/polarization/thole_iterative.c:168-259) on the device.  Included by engine.hip.
//
// The SCF runs in a "sweep view": the polarizable atoms, compacted, in sweep order (see
// SweepView in engine.hip).  Per energy(): gather the view's coordinates, build its A block,
// compute E_static for ALL atoms (field files need it), gather it into the view, iterate,
// scatter mu / E_ind / dE_ind back to atom order.

// the coefficient update setup_view() prepared, as a launch of its own (when it cannot ride in the field kernel's)
static int launch_coef_job(mpmc_hip_ctx *c, const DevBox &bx) {
    if (!c->call.coef_job_valid) return 0;
    c->call.coef_job_valid = false;
    const CoefJob &cj = c->call.coef_job;
    MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((update_coef_moves_kernel<kM>), dim3(cj.nt, cj.dm.n), dim3(64), 0, c->stream, cj.pa,
                                              bx, cj.tp, cj.dm, cj.ntld, cj.C, cj.m, cj.gx, cj.gy, cj.gz, cj.slot_of_atom, cj.px,
                                              cj.py, cj.pz));
    if (c->call.coef_job_fork) hipEventRecord(c->ev_fork, c->stream);
    return 0;
}

static int launch_field(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx) {
    const mpmc_hip_params &P = c->par;
    ScopedTimer t(c, T_FIELD);
    FieldParams fp;
    fp.wolf_alpha = P.polar_wolf_alpha;
    fp.cutoffterm = 0.0;
    // enough j-chunks to fill the chip: ~2048 waves in flight
    const int ntile = c->npad / 64;
    const ChunkPlan cp = chunk_plan(c->npad, 4096);
    const int nchunk = cp.nchunk, chunk = cp.chunk;
    fp.chunk = chunk;
    // The real-space partials persist between calls: with nothing moved since the last call the kernel is
    // skipped, after a single-molecule move only the tiles of the moved atoms' blocks are recomputed.
    const bool wolf = P.polar_wolf || c->thole_wolf_full;  // thole_field.c:32
    const int mode = P.polar_ewald ? kFieldEwald : (!wolf ? kFieldBare : (P.polar_wolf_alpha == 0.0 ? kFieldWolf0 : kFieldWolfA));
    const int key = mode * 1000003 + chunk;
    DirtyBlocks sel = c->call.dirty_blocks;
    const bool resident = c->field_part_valid && c->field_key == key;
    if (!resident) sel.n = 0;
    const bool skip = resident && sel.n == 0 && c->dirty_atoms.empty();
    dim3 grid = (sel.n > 0) ? dim3(std::max(nchunk, ntile), sel.n, 2) : dim3(nchunk, ntile), block(64 * kFieldWaves);
    c->field_part_valid = true;
    c->field_key = key;
    // The step's coefficient update (and with it the move) rides in a third z-slice of the incremental grid when there
    // is one and it has room (8 units of 64 partners per workgroup); otherwise it is a launch of its own, here.
    bool fused = false;
    if (c->call.coef_job_valid) {
        const CoefJob &cj = c->call.coef_job;
        fused = c->opt.fuse_field && !skip && sel.n > 0 && !P.polar_ewald && c->graph_mode == GM_DIRECT &&
                (long)grid.x * sel.n * kFieldWaves >= (long)cj.nt * cj.dm.n;
        if (fused) grid.z = 3;
        else if (launch_coef_job(c, bx)) return -1;
    }
    if (P.polar_ewald) {
        // ewald_estatic(): reciprocal part into extra partial slots, real part in the pair slots
        if (build_field_kvectors(c)) return -1;
        const int nkc = 8, kchunk = (c->nkf + nkc - 1) / nkc;
        if (c->nkf > 0 && c->graph_mode != GM_UPDATE) {  // (static nodes of a step graph)
            hipLaunchKernelGGL(ewald_field_sf_kernel, dim3(c->nkf), dim3(256), 0, c->stream, a, c->d_kvecf, c->d_sf);
            hipLaunchKernelGGL(ewald_field_recip_kernel, dim3(nkc, ntile), dim3(64), 0, c->stream, a, c->d_kvecf, c->d_sf,
                               c->nkf, kchunk, 8.0 * kPI / c->volume, nchunk, c->d_fieldpart);
        }
        fp.wolf_alpha = c->polar_ewald_alpha;
        if (!skip)
            HIPCHK(launch_slot(c, GS_FIELD, static_field_kernel<kFieldEwald>, grid, block, c->stream, a, bx, fp, sel,
                               c->d_fieldpart));
        c->es_slots = nchunk + (c->nkf > 0 ? nkc : 0);
        c->es_stale = true;
        return 0;
    }
    if (mode == kFieldWolfA) {
        const double al = P.polar_wolf_alpha, R = c->cutoff, rR = 1.0 / R;
        fp.cutoffterm = std::erfc(al * R) * rR * rR + 2.0 * al * kOneOverSqrtPi * std::exp(-al * al * R * R) * rR;
    }
    // KERNEL<kF> for the call's field mode (the Ewald form has returned above)
#define MPMC_FIELD_DISPATCH(...)                                                       \
    do switch (mode) {                                                                 \
        case kFieldBare: { constexpr int kF = kFieldBare; __VA_ARGS__; break; }        \
        case kFieldWolf0: { constexpr int kF = kFieldWolf0; __VA_ARGS__; break; }      \
        default: { constexpr int kF = kFieldWolfA; __VA_ARGS__; break; }               \
    } while (0)
    if (fused) {
        const CoefJob &cj = c->call.coef_job;
        c->call.coef_job_valid = false;
        MPMC_FIELD_DISPATCH(MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((field_coef_kernel<kF, kM>), grid, block, 0, c->stream, a, bx,
                                                                      fp, sel, c->d_fieldpart, cj)));
        HIPCHK(hipGetLastError());
        if (c->call.coef_job_fork) hipEventRecord(c->ev_fork, c->stream);
    } else if (!skip) {
        MPMC_FIELD_DISPATCH(HIPCHK(launch_slot(c, GS_FIELD, static_field_kernel<kF>, grid, block, c->stream, a, bx, fp, sel,
                                               c->d_fieldpart)));
    }
#undef MPMC_FIELD_DISPATCH
    c->es_slots = nchunk;
    c->es_stale = true;
    return 0;
}

// the pending move, the plain way (apply_moves_kernel), when it could not ride inside the coefficient update
static int apply_deferred_moves(mpmc_hip_ctx *c) {
    if (!c->call.moves_deferred) return 0;
    c->call.moves_deferred = false;
    c->call.side_carry = false;  // (the side stream waits for the event below)
    if (flush_moves(c)) return -1;
    if (c->opt.overlap) hipEventRecord(c->ev_fork, c->stream);
    return 0;
}

// collect the view slots of the atoms moved since the last energy(); false if there are too many
static bool collect_dirty_slots(mpmc_hip_ctx *c, const SweepView &v, DirtyList &dl, int &nd) {
    nd = 0;
    for (int atom : c->dirty_atoms) {
        const int slot = v.slot_of_atom[atom];
        if (slot < 0) continue;
        bool seen = false;
        for (int k = 0; k < nd; ++k) seen |= (c->h_dirty[k] == slot);
        if (seen) continue;
        if (nd == kMaxDirty) return false;
        c->h_dirty[nd++] = slot;
    }
    for (int k = 0; k < kMaxDirty; ++k) dl.slot[k] = (k < nd) ? c->h_dirty[k] : 0;
    return true;
}

// diagnostic only (option "inv_stamps"): block, then print where a gs_block_inverse_kernel launch's time went
static int print_inv_stamps(hipStream_t st, const unsigned long long *istamps, size_t nwg, int waves, const GsBuild &gb,
                            int nsingle, bool full) {
    std::vector<unsigned long long> h(nwg * 4);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(h.data(), istamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull, t3 = 0;
    double ph[3] = {0, 0, 0}, phmax[3] = {0, 0, 0}, start_max = 0;
    int live = 0;
    for (size_t g = 0; g < nwg; ++g) {
        if (!h[4 * g + 3]) continue;
        t0 = std::min(t0, h[4 * g]);
    }
    for (size_t g = 0; g < nwg; ++g) {
        if (!h[4 * g + 3]) continue;
        ++live;
        t3 = std::max(t3, h[4 * g + 3]);
        start_max = std::max(start_max, (double)(h[4 * g] - t0) * 0.01);
        for (int k = 0; k < 3; ++k) {
            const double d = (double)(h[4 * g + k + 1] - h[4 * g + k]) * 0.01;
            ph[k] += d;
            phmax[k] = std::max(phmax[k], d);
        }
    }
    fprintf(stderr, "INV_STAMPS waves %d, %d live workgroups of %zu (lists %d %d %d, full %d): span %.2f us, last start +%.2f us; "
                    "mean (max) us: loads %.2f (%.2f), expansion %.2f (%.2f), substitution %.2f (%.2f)\n",
            waves, live, nwg, gb.inv.n, gb.own.n, nsingle, full ? 1 : 0, (double)(t3 - t0) * 0.01, start_max, ph[0] / std::max(live, 1),
            phmax[0], ph[1] / std::max(live, 1), phmax[1], ph[2] / std::max(live, 1), phmax[2]);
    return 0;
}

// Gauss-Seidel chain data (kernels_gs_chain.h) of a view of nt blocks whose coefficients setup_view() has just brought up
// to date on stream `st`: the inverse of a diagonal block is a function of that block's atoms, the expanded tile (t, t-k) of
// blocks t and t-k: after a move only those of the moved atoms' blocks (the view slots `dl`) and of a re-ordered tail are
// redone.  Maintained only while every call keeps them up to date (M_call), else rebuilt.  coef_updated: the coefficients
// were updated in place, not rebuilt.
static int maintain_chain_data(mpmc_hip_ctx *c, SweepView &v, const DevBox &bx, hipStream_t st, int nt, bool coef_updated,
                               int tail, const DirtyList &dl, int nd) {
    if (ensure_view_chain(c, v, st)) return -1;
    const bool fresh = coef_updated && v.M_epoch == v.C_epoch && v.M_call + 1 == c->energy_calls;
    // How many lags a view caches is decided when it is rebuilt as a whole: the option's value -- unless the view was rebuilt
    // as a whole in the previous call too (a grand-canonical chain rebuilds its ranked view every step: the rebuild, not
    // the sweeps, bounds such a step, and a third lag costs it more than the shorter sweeps return: 1 380 vs 1 425 steps/s).
    if (!fresh || v.nlag < 2 || v.nlag > c->opt.gs_lags) {
        // (three calls in a row: a ranked walk that changes and changes back in consecutive NVT steps keeps the full count)
        const bool again = v.last_full_call >= 0 && (unsigned long long)v.last_full_call + 1 >= c->energy_calls;
        v.full_streak = again ? v.full_streak + 1 : 0;
        v.nlag = (v.full_streak >= 2) ? std::min(2, c->opt.gs_lags) : c->opt.gs_lags;
    }
    const int nlag = v.nlag;
    GsBuild gb;
    const bool full = plan_chain_build(fresh && v.nlag_built == v.nlag, tail, nt, nlag, dl.slot, nd, gb);
    if (full) v.last_full_call = (long long)c->energy_calls;
    v.nlag_built = nlag;
    gb.Minv = v.Minv;
    for (int k = 0; k < kGsMaxLag; ++k) gb.Lnb[k] = v.Lnb[k];
    gb.nlag = nlag;
    int nsingle = 0, nsingle_max = 0;
    for (int k = 0; k < nlag; ++k) {
        nsingle += gb.nb[k].n;
        nsingle_max = std::max(nsingle_max, gb.nb[k].n);
    }
    // One launch: z-slice 0 the block inverses M_t (list `inv`), z-slice 1 all neighbour matrices L(k)_t = M_t D T(t,t-k)
    // of the blocks that changed themselves (list `own`, one pass for the nlag right-hand sides), z-slice 1 + k the one
    // matrix L(k)_t of the block k places behind a changed one -- the same forward substitution with other right-hand sides.
    if (full || gb.inv.n > 0 || gb.own.n > 0 || nsingle > 0) {
        const int nblk = full ? nt : std::max(std::max(gb.inv.n, gb.own.n), nsingle_max);
        const int nsolve = full ? 2 * nt : gb.inv.n + gb.own.n + nsingle;
        const int waves = inverse_waves(nsolve, st == c->stream, c->opt.gs_side_waves, gs_chain_ticket_base(nt, nlag));
        // The main stream's builder is forked to a stream of its own: nothing but the chain kernel reads its output, and the
        // launches between here and the chain (static field, view set-up, upper-triangle sums: ~28 us) do not depend on it.
        hipStream_t bst = st;
        // (Only for views of 24 blocks or more: below that the launches in between are short, the front of the step is bound
        //  by the host's launch rate, and the four event calls of the fork cost more than it hides -- 4 400 vs 4 650 steps/s
        //  at 1 024 atoms, +3 % at 4 096; option gs_build_fork = 2 forces it.)
        if (st == c->stream && c->opt.inv_stamps <= 0 && (c->opt.gs_build_fork == 2 || (c->opt.gs_build_fork == 1 && nt >= 24))) {
            HIPCHK(hipEventRecord(c->ev_bfork, c->stream));
            HIPCHK(hipStreamWaitEvent(c->stream3, c->ev_bfork, 0));
            bst = c->stream3;
        }
        const dim3 gi(192 / waves, nblk, full ? 2 : 2 + nlag), bi(64 * waves);
        unsigned long long *istamps = nullptr;
        const size_t nwg = (size_t)gi.x * gi.y * gi.z;
        if (c->opt.inv_stamps > 0 && st == c->stream) {
            if (!c->d_istamps) HIPCHK(c->d_istamps.alloc((size_t)16 * 256 * 3 * 4));
            if (nwg <= (size_t)16 * 256 * 3) {
                HIPCHK(hipMemsetAsync(c->d_istamps, 0, nwg * 4 * sizeof(unsigned long long), st));
                istamps = c->d_istamps;
            }
        }
#define MPMC_LAUNCH_INVERSE(O, W)                                                                                          \
    hipLaunchKernelGGL((gs_block_inverse_kernel<O, W>), gi, bi, kInverseLds, bst, v.C, v.ntld, v.px, v.py, v.pz, v.palpha, bx, \
                       gb, istamps)
        if (c->box_ortho) {
            if (waves == 4) MPMC_LAUNCH_INVERSE(1, 4);
            else if (waves == 8) MPMC_LAUNCH_INVERSE(1, 8);
            else MPMC_LAUNCH_INVERSE(1, 16);
        } else {
            if (waves == 4) MPMC_LAUNCH_INVERSE(0, 4);
            else if (waves == 8) MPMC_LAUNCH_INVERSE(0, 8);
            else MPMC_LAUNCH_INVERSE(0, 16);
        }
#undef MPMC_LAUNCH_INVERSE
        if (bst != st) {
            HIPCHK(hipEventRecord(c->ev_bjoin, bst));
            c->call.build_join_pending = true;
        }
        if (istamps) {
            --c->opt.inv_stamps;
            if (print_inv_stamps(st, istamps, nwg, waves, gb, nsingle, full)) return -1;
        }
    }
    v.M_epoch = v.C_epoch;
    v.M_call = c->energy_calls;
    return 0;
}

// setup_view(): view 0's coefficient update that also applies the pending move becomes the call's CoefJob, and the move
// is no longer pending on the main stream.
static void hand_over_coef_job(mpmc_hip_ctx *c, const SweepView &v, const DevAtoms &pa, const TholeParams &tp,
                               const DirtyMoves &dm, int nt) {
    CoefJob &cj = c->call.coef_job;
    cj.pa = pa;
    cj.tp = tp;
    cj.dm = dm;
    cj.nt = nt;
    cj.ntld = v.ntld;
    cj.C = v.C;
    cj.m = c->pending;
    cj.gx = c->d_x;
    cj.gy = c->d_y;
    cj.gz = c->d_z;
    cj.slot_of_atom = (const int *)v.d_slot;
    cj.px = v.px;
    cj.py = v.py;
    cj.pz = v.pz;
    c->call.coef_job_valid = true;
    if (c->call.side_carry) c->call.side_moves = c->pending;  // the side stream's pair kernel applies it too
    c->pending.n = 0;
    c->call.moves_deferred = false;
    // the new coordinates are in place (no event when the side stream does not wait for them: it carries the
    // move in its pair kernel, or -- Gauss-Seidel modes -- applies it for itself first)
    c->call.coef_job_fork = c->opt.overlap && !c->call.side_carry && c->call.side_apply.n == 0;
}

// gather the view's per-atom data from the current configuration and build its A block -- as pair
// coefficients (kernels_coef.h) for the Jacobi/Palmo sweeps, expanded (3 nv x 3 nv doubles) for the
// Gauss-Seidel kernels, which walk rows of the matrix
static int setup_view(mpmc_hip_ctx *c, SweepView &v, const DevAtoms &a, const DevBox &bx, bool incremental,
                      bool want_coef, bool want_matrix, bool want_chain = false, hipStream_t side = nullptr) {
    // `side`: maintain the view on that stream instead of the engine's main one (the ranked view of a speculative
    // polar_gs_ranked call is brought up to date beside the first sweep)
    const hipStream_t st = side ? side : c->stream;
    // The step's move may still be pending (enqueue_direct defers it when this call can apply it inside the coefficient
    // update of view 0, below); anything else that is about to read coordinates needs it applied first.
    bool fuse_moves = false;
    if (c->call.moves_deferred && &v == &c->view[0]) {
        fuse_moves = !side && incremental && v.pos_valid && want_coef && v.C_valid && v.rebuild_from < 0 && !c->all_dirty &&
                     c->opt.incremental;
        if (!fuse_moves && apply_deferred_moves(c)) return -1;
    }
    if (!(incremental && v.pos_valid)) {
        // every allocated slot is defined (zeros / invalid past nv): inserts may grow the view into them
        const dim3 g((v.cap + 255) / 256), b(256);
        hipLaunchKernelGGL(gather_atoms_kernel, g, b, 0, st, v.nv, v.cap, v.d_idx, a, v.px, v.py, v.pz,
                           v.palpha, v.pflags);
        v.pos_valid = incremental && (&v == &c->view[0]);  // view 0 tracks later moves through apply_moves_kernel
    }
    DevAtoms pa = a;
    pa.x = v.px;
    pa.y = v.py;
    pa.z = v.pz;
    pa.alpha = v.palpha;
    pa.flags = v.pflags;
    pa.n = v.nv;
    pa.npad = v.nvpad;
    const TholeParams tp = thole_params(c, v.d_idx);  // (q and mol stay in atom order: the undamped model reads them through d_idx)
    ScopedTimer t(c, T_AMAT, st);
    // The tensor data stays resident between calls: after a single-molecule move only the entries of pairs
    // that involve a moved atom are rewritten (bit-identical to a full rebuild).
    DirtyList dl;
    int nd = 0;
    const bool can_update = incremental && !c->all_dirty && c->opt.incremental && collect_dirty_slots(c, v, dl, nd);
    const int nt = std::max(1, (v.nv + kCoefTile - 1) / kCoefTile);
    bool coef_updated = false;  // C was brought up to date by rewriting the dirty slots' entries only
    // a view whose ORDER changed from block `tail` on (set_sweep_order after a grand-canonical edit): the data of the
    // blocks in front of it are still those of their atoms; the tail is rebuilt, then moved atoms are updated as usual
    int tail = -1;
    if (v.rebuild_from >= 0) {
        if (want_coef && want_chain && can_update && v.C_valid && v.rebuild_from < nt && nt - v.rebuild_from <= kMaxBlockList - 16)
            tail = v.rebuild_from;
        else
            v.C_valid = false;  // cannot keep the prefix: everything is rebuilt
        v.rebuild_from = -1;
    }
    if (want_coef) {
        if (ensure_view_coef(c, v, nt, st)) return -1;
        if (can_update && v.C_valid) {
            if (tail >= 0)
                MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((build_coef_kernel<kM>), dim3(nt, nt), dim3(64 * kCoefWaves), 0, st, pa,
                                                          bx, tp, v.ntld, v.C, tail));
            if (nd > 0 && side)
                MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((update_coef_kernel<kM>), dim3(nt, nd), dim3(64), 0, st, pa, bx, tp, dl,
                                                          v.ntld, v.C));
            else if (nd > 0 && fuse_moves && nd <= kMaxDirtyMoves) {
                // the move and the coefficient update in one launch (kernels_coef.h)
                DirtyMoves dm;
                dm.n = nd;
                for (int k = 0; k < kMaxDirtyMoves; ++k) {
                    dm.slot[k] = (k < nd) ? dl.slot[k] : 0;
                    dm.x[k] = dm.y[k] = dm.z[k] = 0.0;
                }
                bool all_found = true;
                for (int k = 0; k < nd; ++k) {
                    const int atom = v.h_idx[dl.slot[k]];
                    bool found = false;
                    for (int e = 0; e < c->pending.n; ++e) {
                        if (c->pending.idx[e] == atom) {
                            dm.x[k] = c->pending.x[e];
                            dm.y[k] = c->pending.y[e];
                            dm.z[k] = c->pending.z[e];
                            found = true;
                        }
                    }
                    all_found &= found;
                }
                if (all_found) {
                    // handed to launch_field(), the next launch of the chain, which lets it ride in the field kernel's
                    // grid (field_coef_kernel) or, when it cannot, launches update_coef_moves_kernel in front of it
                    hand_over_coef_job(c, v, pa, tp, dm, nt);
                    // with chain data to maintain, the job cannot wait for launch_field(): the block matrices below are
                    // functions of the updated coefficients
                    if (want_chain && launch_coef_job(c, bx)) return -1;
                } else {  // a dirty slot whose coordinates are already on the device (staged copy): the plain way
                    if (apply_deferred_moves(c)) return -1;
                    MPMC_THOLE_DISPATCH(c, HIPCHK(launch_slot(c, GS_COEF, update_coef_kernel<kM>, dim3(nt, nd), dim3(64), c->stream,
                                                              pa, bx, tp, dl, v.ntld, v.C)));
                }
            } else if (nd > 0) {
                if (c->call.moves_deferred && &v == &c->view[0] && apply_deferred_moves(c)) return -1;
                MPMC_THOLE_DISPATCH(c, HIPCHK(launch_slot(c, GS_COEF, update_coef_kernel<kM>, dim3(nt, nd), dim3(64), c->stream, pa,
                                                          bx, tp, dl, v.ntld, v.C)));
            }
            if (c->call.moves_deferred && &v == &c->view[0] && apply_deferred_moves(c)) return -1;  // (nd == 0: nothing fused)
            coef_updated = true;
        } else {
            if (c->call.moves_deferred && &v == &c->view[0] && apply_deferred_moves(c)) return -1;
            MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((build_coef_kernel<kM>), dim3(nt, nt), dim3(64 * kCoefWaves), 0, st, pa, bx,
                                                      tp, v.ntld, v.C, 0));
            v.C_valid = true;
            ++v.C_epoch;
        }
    } else {
        v.C_valid = false;
    }
    if (want_chain && want_coef && maintain_chain_data(c, v, bx, st, nt, coef_updated, tail, dl, nd)) return -1;
    if (want_matrix) {
        if (ensure_view_matrix(v)) return -1;
        if (can_update && v.A_valid) {
            if (nd > 0)
                MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((update_amatrix_kernel<kM>), dim3(v.nvpad / 128, nd), dim3(64), 0, st, pa,
                                                          bx, tp, dl, v.A, 3 * v.nvpad));
        } else {
            MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((build_amatrix_kernel<kM>), dim3(v.nvpad / 128, v.nvpad / kARows), dim3(64), 0,
                                                      st, pa, bx, tp, v.A, 3 * v.nvpad));
            v.A_valid = true;
        }
    } else {
        v.A_valid = false;
    }
    return 0;
}

// Jacobi / Palmo pass over the view's matrix: symmetric (upper triangle, half the bytes) or plain.
template <int MODE>
static int launch_sweep(mpmc_hip_ctx *c, SweepView &v, const DevBox &bx, const double *mu_in, double *out,
                        const SweepParams &sp, int timer_class, const double *mu_final = nullptr) {
    const int nvpad = v.nvpad, lda = 3 * nvpad;
    if (v.C_valid) {
        const int nt = std::max(1, (v.nv + kCoefTile - 1) / kCoefTile);
        if (ensure_coef_scratch(v, nt)) return -1;
        CoefFinish fin;
        fin.alpha = v.palpha;
        fin.flags = v.pflags;
        fin.mu_in = mu_in;
        fin.es = v.es;
        fin.ef_induced = v.efind;
        fin.out = out;
        fin.rrms = v.rrms;
        fin.errmax = c->d_errmax;
        fin.mu_final = mu_final;
        fin.energy_part = v.energy_part;
        fin.tmu0 = v.tmu0;
        fin.sp = sp;
        size_t half_plane = 0;
        {
            // the pass over the pair coefficients alone; on timed calls the kernel's own begin / end timestamps
            const int ntiles = nt * (nt + 1) / 2;
            // half-tile workgroups where a CU gets only a few tiles (beyond the resident solver's range, below ~8 per CU)
            const bool split = c->opt.sweep_split > 0 || (c->opt.sweep_split < 0 && kSweepSplitAuto && nt > 21 && ntiles < 8 * c->num_cus);
            half_plane = split ? 2 * (3 * (size_t)kCoefTile * nt) * (size_t)nt : 0;
            const dim3 g(split ? 16 * ((ntiles + 7) / 8) : ntiles), b(64 * kCoefWaves);
            // a tile set that fits the Infinity Cache is re-read from it sweep after sweep (default-policy loads: 32 vs
            // 38 us per sweep at 8192 atoms, 191 MB); one that does not is streamed (non-temporal: 145 vs 150 us at 16384)
            const size_t tile_bytes = (size_t)nt * (nt + 1) / 2 * kCoefTile * kCoefTile * sizeof(double2);
            const bool sweep_nt = c->opt.sweep_nt > 0 || (c->opt.sweep_nt < 0 && tile_bytes > ((size_t)224 << 20));
            void (*kern)(const double2 *, int, int, const double *, const double *, const double *, const double *, DevBox,
                         double *, double *, int, size_t) =
                c->box_ortho ? (sweep_nt ? pair_sweep_kernel<1, 1> : pair_sweep_kernel<1, 0>)
                             : (sweep_nt ? pair_sweep_kernel<0, 1> : pair_sweep_kernel<0, 0>);
            if (split)
                kern = c->box_ortho ? (sweep_nt ? pair_sweep_kernel<1, 1, 0, 1> : pair_sweep_kernel<1, 0, 0, 1>)
                                    : (sweep_nt ? pair_sweep_kernel<0, 1, 0, 1> : pair_sweep_kernel<0, 0, 0, 1>);
            if (c->opt.sweep_ablate == 1) kern = pair_sweep_kernel<1, 0, 1>;  // timing-only experiments (ortho boxes)
            if (c->opt.sweep_ablate == 2) kern = pair_sweep_kernel<1, 0, 2>;
            if (c->opt.sweep_ablate) half_plane = 0;
            HIPCHK(launch_timed(c, timer_class, kern, g, b, 0, c->stream, (const double2 *)v.C, nt, v.ntld,
                                (const double *)v.px, (const double *)v.py, (const double *)v.pz, mu_in, bx, v.Srow, v.Zcol,
                                c->opt.sweep_alternate ? (c->sweep_parity++ & 1) : 0, half_plane));
        }
        {
            ScopedTimer t2(c, T_OTHER);
            hipLaunchKernelGGL(pair_finish_kernel<MODE>, dim3(nt), dim3(64 * kCoefFinishGroups), 0, c->stream, nt, v.Srow,
                               v.Zcol, fin, half_plane);
        }
        c->energy_part = v.energy_part;
        c->energy_nt = nt;
        return 0;
    }
    c->energy_nt = 0;
    // below ~2k polarizable atoms the triangle has too few 32x128-atom units to fill 256 CUs
    if (c->opt.symmetric && (nvpad >= 2048 || c->opt.symmetric > 1)) {
        if (ensure_sym_scratch(v)) return -1;
        {
            ScopedTimer t(c, timer_class);  // the HBM-bound pass alone, so it can be held against rocprof
            const dim3 g(nvpad / kSymChunkAtoms, nvpad / kSymRowAtoms);
            const int rev = (c->opt.sym_mode & 1) ? (c->sweep_parity++ & 1) : 0;
            if (c->opt.sym_mode & 2)
                hipLaunchKernelGGL(symv_kernel<1>, g, dim3(64), 0, c->stream, v.A, lda, nvpad, mu_in, v.Srow, v.Zcol, rev,
                                   v.nv);
            else
                hipLaunchKernelGGL(symv_kernel<0>, g, dim3(64), 0, c->stream, v.A, lda, nvpad, mu_in, v.Srow, v.Zcol, rev,
                                   v.nv);
        }
        ScopedTimer t2(c, T_OTHER);
        hipLaunchKernelGGL(symv_finish_kernel<MODE>, dim3(nvpad / 64), dim3(1024), 0, c->stream, nvpad, v.Srow, v.Zcol,
                           v.palpha, v.pflags, mu_in, v.es, v.efind, out, v.rrms, c->d_errmax, sp);
    } else {
        ScopedTimer t(c, timer_class);
        hipLaunchKernelGGL(sweep_kernel<MODE>, dim3(nvpad), dim3(64), 0, c->stream, v.A, lda, nvpad, v.palpha,
                           v.pflags, mu_in, v.es, v.efind, out, v.rrms, c->d_errmax, sp);
    }
    return 0;
}

// Does this call leave its LAST Jacobi sweep to whoever asks for the dipoles?  U_pol = -1/2 sum mu_n.E needs the dipoles and
// sums of sweeps up to ceil(n / 2) only (kernels_coef.h, pair_finish_kernel; DESIGN.md section 3), and sweep n produces
// nothing else a Monte Carlo step reads.  A function of the flags, the view's size and the device alone -- not of options other than the
// storage the sweeps run on, of the resident solver's fallback state or of earlier calls -- so that U_pol's last bits
// are a function of the configuration: plain fixed-count Jacobi (gamma = 1, at least two sweeps, no RRMS) on pair
// coefficients, on a view too large for the one-launch solvers (resident_plan()'s size test), whose results the
// launch-per-sweep path is held to bit for bit.
static bool defer_last_sweep(const mpmc_hip_ctx *c, const SweepView &v) {
    const mpmc_hip_params &P = c->par;
    if (!c->opt.pair_coef || !v.C_valid) return false;
    if (P.polar_zodid || P.polar_gs || P.polar_gs_ranked || P.polar_palmo || P.polar_sor || P.polar_esor || P.polar_rrms)
        return false;
    if (P.polar_precision != 0.0 || P.polar_gamma != 1.0 || P.polar_max_iter < 2) return false;
    const int nt = std::max(1, (v.nv + kCoefTile - 1) / kCoefTile);
    return nt * (nt + 1) / 2 + nt > c->num_cus;
}

// The sweeps the last call left out, now and in order: mu_n into the buffer result_mu already names, E_ind(mu_{n-1}) into
// the view.  Same launches with the same arguments as when the call itself ran them, hence the same bits.
static int complete_pending_sweep(mpmc_hip_ctx *c) {
    if (c->psweep.sweeps.empty()) return 0;
    PendingSweep p;
    std::swap(p, c->psweep);  // (nothing is pending any more, whatever a launch below returns)
    HIPCHK(hipSetDevice(c->device));
    for (const PendingSweep::One &s : p.sweeps)
        if (launch_sweep<kSweepJacobi>(c, *p.view, p.bx, s.mu_in, s.mu_out, s.sp, T_SWEEP)) return -1;
    return 0;
}

static void (*chain_kernel_of(int ortho))(GsChain) { return ortho ? gs_chain_kernel<1> : gs_chain_kernel<0>; }

// Gauss-Seidel runs on the chain kernel (pair coefficients + cached block inverses) unless the A/B options say
// otherwise; the older path walks the expanded matrix with two launches per block.
static bool gs_uses_chain(const mpmc_hip_ctx *c) { return c->opt.pair_coef != 0 && c->opt.persistent_gs != 0; }

// One exact Gauss-Seidel sweep in the view's order -- see kernels_gs_chain.h (default) / kernels_gs.h.
struct GsFinishArgs {  // the end-of-sweep bookkeeping, for the chain kernel's tail (or gs_finish_kernel)
    double w_new, w_old;
    int want_rrms, err_slot;
    double *mu_out;
};
static int launch_gs_sweep(mpmc_hip_ctx *c, SweepView &v, const DevAtoms &a, const DevBox &bx, const double *mu_old,
                           const GsFinishArgs *fin = nullptr, bool *finished = nullptr) {
    if (finished) *finished = false;
    const int nvpad = v.nvpad, lda = 3 * nvpad;
    (void)a;
    ++c->call.gs_sweeps;
    if (gs_uses_chain(c) && v.C_valid) {
        // upper-triangle product with the old dipoles from the pair coefficients (fully parallel) ...
        const int nt = std::max(1, (v.nv + kCoefTile - 1) / kCoefTile);
        if (ensure_coef_scratch(v, nt)) return -1;
        // (fold_upper: the chain's workgroups add up the row sums of their blocks themselves while they wait for their turn --
        //  no pair_upper_finish_kernel launch; the upper kernel then arms the hand-off buffer.  Only with the end-of-sweep
        //  bookkeeping folded into the chain as well: gs_finish_kernel reads y for the padding blocks too.)
        const bool fold_upper = c->opt.gs_fold_upper && fin && c->opt.gs_fold_finish && !c->opt.gs_ablate;
        {
            ScopedTimer tu(c, T_OTHER);
            const dim3 g(nt * (nt + 1) / 2), b(64 * kCoefWaves);
            const int rev = c->opt.sweep_alternate ? (c->sweep_parity++ & 1) : 0;
            if (c->box_ortho)
                hipLaunchKernelGGL(pair_upper_kernel<1>, g, b, 0, c->stream, v.C, nt, v.ntld, v.px, v.py, v.pz, mu_old, bx, v.Srow, rev,
                                   fold_upper ? nt : 0, v.mupub, v.gsflags, c->gs_qoff);
            else
                hipLaunchKernelGGL(pair_upper_kernel<0>, g, b, 0, c->stream, v.C, nt, v.ntld, v.px, v.py, v.pz, mu_old, bx, v.Srow, rev,
                                   fold_upper ? nt : 0, v.mupub, v.gsflags, c->gs_qoff);
            // (also arms the hand-off buffer: mu_new at the sentinel pattern, ticket counter zero)
            if (!fold_upper)
                hipLaunchKernelGGL(pair_upper_finish_kernel, dim3(nvpad / 64), dim3(64 * kCoefFinishGroups), 0, c->stream, nt,
                                   v.Srow, v.y, 1, v.mupub, v.gsflags, c->gs_qoff);
        }
        // ... then ONE persistent launch for the lower triangle: a workgroup per 64-atom block
        GsChain gp;
        gp.C = v.C;
        gp.ntld = v.ntld;
        gp.nb = nt;
        gp.px = v.px;
        gp.py = v.py;
        gp.pz = v.pz;
        gp.alpha = v.palpha;
        gp.es = v.es;
        gp.Minv = v.Minv;
        for (int k = 0; k < kGsMaxLag; ++k) {
            gp.Lnb[k] = v.Lnb[k];
            gp.pub[k] = v.mupub + k * (size_t)c->gs_qoff;
        }
        gp.nlag = v.nlag >= 2 ? v.nlag : c->opt.gs_lags;
        gp.y = v.y;
        gp.mu_new = v.mupub;
        gp.flags = v.gsflags;
        gp.bx = bx;
        gp.fault_block = (c->opt.gs_fault_sweep > 0 && c->call.gs_sweeps == c->opt.gs_fault_sweep) ? std::min(1, nt - 1) : -1;
        gp.stamps = nullptr;
        gp.Srow = fold_upper ? v.Srow : nullptr;
        gp.nt_upper = nt;
        gp.ablate = c->opt.gs_ablate;
        memset(&gp.fin, 0, sizeof(gp.fin));
        if (fin && c->opt.gs_fold_finish && !c->opt.gs_ablate) {
            gp.fin.on = 1;
            gp.fin.flags = v.pflags;
            gp.fin.mu_old = mu_old;
            gp.fin.w_new = fin->w_new;
            gp.fin.w_old = fin->w_old;
            gp.fin.want_rrms = fin->want_rrms;
            gp.fin.err_slot = fin->err_slot;
            gp.fin.mu_out = fin->mu_out;
            gp.fin.mu_new_lin = v.munew;
            gp.fin.ef_induced = v.efind;
            gp.fin.rrms = v.rrms;
            gp.fin.errmax = c->d_errmax;
            if (finished) *finished = true;
        }
        if (c->opt.gs_stamps > 0) {
            const size_t need = (size_t)(c->max_npad / 64 + 1) * 16;
            if (c->d_stamps.size() < need) HIPCHK(c->d_stamps.alloc(need));
            HIPCHK(hipMemsetAsync(c->d_stamps, 0, (size_t)nt * 16 * sizeof(unsigned long long), c->stream));
            gp.stamps = c->d_stamps;
        }
        {
            void (*kern)(GsChain) = chain_kernel_of(c->box_ortho ? 1 : 0);
            if (c->call.build_join_pending) {  // the chain data of this call's move (built beside the launches in front of this one)
                HIPCHK(hipStreamWaitEvent(c->stream, c->ev_bjoin, 0));
                c->call.build_join_pending = false;
            }
            // (main workgroups of all blocks + an auxiliary one per lag 2 .. nlag of the blocks t >= lag; roles by ticket)
            const int grid = gs_chain_ticket_base(nt, gp.nlag);
            HIPCHK(launch_timed(c, T_SWEEP, kern, dim3(grid), dim3(kChainThreads), kChainLds, c->stream, gp));
        }
        if (gp.stamps) {
            // diagnostic only: block until the sweep is done and print, per block, the stamps relative to the launch
            --c->opt.gs_stamps;
            std::vector<unsigned long long> h((size_t)nt * 16);
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipMemcpy(h.data(), c->d_stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            unsigned long long t0 = ~0ull;
            for (int b = 0; b < nt; ++b) t0 = std::min(t0, h[(size_t)b * 16]);
            fprintf(stderr, "GS_STAMPS sweep %d (us since the first workgroup started; 0 start, 1 staged, 2/3 and 4/5 the last two far tiles, "
                            "6 far sums in LDS, 7 w_t done, 8 mu(t-1) in LDS, 9 P product summed, 10 published, 11 end)\n",
                    c->call.gs_sweeps);
            for (int b = 0; b < nt; ++b) {
                fprintf(stderr, "GS_STAMPS b%02d", b);
                for (int k = 0; k < 12; ++k)
                    fprintf(stderr, " %7.2f", h[(size_t)b * 16 + k] ? (double)(h[(size_t)b * 16 + k] - t0) * 0.01 : -1.0);
                // effective shader clock of this workgroup's CU over its lifetime: s_memtime ticks per 100 MHz tick
                const double dt = (double)(h[(size_t)b * 16 + 11] - h[(size_t)b * 16 + 0]);
                // when the publishing wave's write-through stores had been acknowledged, after "published"
                fprintf(stderr, "  ack +%.2f", (double)(h[(size_t)b * 16 + 14] - h[(size_t)b * 16 + 10]) * 0.01);
                fprintf(stderr, "  clk %6.0f MHz\n", dt > 0 ? 100.0 * (double)(h[(size_t)b * 16 + 13] - h[(size_t)b * 16 + 12]) / dt : 0.0);
            }
        }
        c->call.gs_used[&v == &c->view[1] ? 1 : 0] = true;  // its error word is checked at the end of energy()
        return 0;
    }
    ScopedTimer t(c, T_SWEEP);
    const int nb = nvpad / kGsBlock;
    hipLaunchKernelGGL(gs_upper_kernel, dim3(nvpad / 4), dim3(256), 0, c->stream, v.A, lda, nvpad, mu_old, v.y);
    for (int b = 0; b < nb; ++b) {
        hipLaunchKernelGGL(gs_solve_block_kernel, dim3(1), dim3(64), 0, c->stream, v.A, lda, b, v.palpha, v.es, v.y,
                           v.munew);
        if (b + 1 < nb)
            hipLaunchKernelGGL(gs_update_kernel, dim3(nb - (b + 1)), dim3(256), 0, c->stream, v.A, lda, b, v.munew,
                               v.y);
    }
    return 0;
}

// The whole Jacobi-type solve in one launch (kernels_resident.h).  Results: dipoles in v.mu1, E_induced / RRMS /
// dE_induced (Palmo) in the view's vectors, per-block energy sums in v.energy_part -- as the multi-launch loop leaves
// them, bit for bit.
static int launch_resident(mpmc_hip_ctx *c, SweepView &v, const DevBox &bx, const ResidentPlan &rp, bool want_rrms) {
    const mpmc_hip_params &P = c->par;
    if (!c->res_attr_set) {
        for (const void *k : resident_kernels())
            HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kResidentLdsMax));
        c->res_attr_set = true;
    }
    ResidentSolve rs;
    rs.C = v.C;
    rs.nt = rp.nt;
    rs.ntld = v.ntld;
    rs.pld = v.res_pld;
    rs.ntiles = rp.ntiles;
    rs.ngroups = rp.ngroups;
    rs.px = v.px;
    rs.py = v.py;
    rs.pz = v.pz;
    rs.alpha = v.palpha;
    rs.es = v.es;
    rs.pflags = v.pflags;
    rs.pub = v.respub;
    rs.slab = (size_t)3 * v.nvpad;
    rs.P = v.resP;
    rs.pstride = (size_t)v.res_pld * v.res_pld * 384;
    rs.mu_out = v.mu1;
    rs.ef_induced = v.efind;
    rs.rrms = v.rrms;
    rs.efchg = v.efchg;
    rs.energy_part = v.energy_part;
    rs.flags = v.gsflags;
    rs.niter = P.polar_max_iter;
    rs.palmo = P.polar_palmo ? 1 : 0;
    rs.want_rrms = want_rrms ? 1 : 0;
    for (int k = 1; k <= kResMaxSweeps; ++k)
        mixing_weights(P.polar_sor, P.polar_esor, P.polar_gamma, k, rs.w_new[k - 1], rs.w_old[k - 1]);
    rs.bx = bx;
    rs.fault = c->opt.res_fault;
    c->opt.res_fault = 0;
    rs.stamps = nullptr;
    const int nrole = rp.fold ? rp.ngroups : rp.nt + rp.ngroups;
    const size_t nstamp = (size_t)nrole * (kResMaxSweeps + 1) * 4;
    if (c->opt.res_stamps > 0) {
        const size_t need = (size_t)768 * (kResMaxSweeps + 1) * 4;
        if (c->d_stamps.size() < need) HIPCHK(c->d_stamps.alloc(need));
        HIPCHK(hipMemsetAsync(c->d_stamps, 0, nstamp * sizeof(unsigned long long), c->stream));
        rs.stamps = c->d_stamps;
    }
    if (c->opt.res_side) feed_side_stream(c);
    ResidentKernel kern = resident_kernel_of(c->box_ortho ? 1 : 0, rp.K, rp.fold);
    HIPCHK(launch_timed(c, T_SWEEP, kern, dim3(nrole), dim3(kResThreads), (size_t)rp.lds, c->stream, rs));
    if (rs.stamps) {
        // diagnostic only: per sweep, when the tile groups had their dipoles / finished multiplying / had published, and
        // when the finishers had their partial sums / had published (us since the first workgroup started; mean and max)
        --c->opt.res_stamps;
        std::vector<unsigned long long> h(nstamp);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(h.data(), c->d_stamps, nstamp * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t1 = 0;
        for (int r = 0; r < nrole; ++r) {
            const unsigned long long v = h[(size_t)r * (kResMaxSweeps + 1) * 4];
            if (v) t0 = std::min(t0, v), t1 = std::max(t1, v);
        }
        fprintf(stderr, "RES_STAMPS nt %d tiles %d groups %d K %d lds %d: workgroups started over %.2f us\n", rp.nt, rp.ntiles,
                rp.ngroups, rp.K, rp.lds, (double)(t1 - t0) * 0.01);
        for (int k = 1; k <= rs.niter; ++k) {
            double mean[5] = {0, 0, 0, 0, 0}, mx[5] = {0, 0, 0, 0, 0};
            int cnt[5] = {0, 0, 0, 0, 0};
            for (int r = 0; r < nrole; ++r) {
                const bool fin = !rp.fold && r < rp.nt;
                for (int q = 0; q < (fin ? 2 : 3); ++q) {
                    const unsigned long long v = h[((size_t)r * (kResMaxSweeps + 1) + k) * 4 + q];
                    if (!v) continue;
                    const int col = fin ? 3 + q : q;
                    const double us = (double)(v - t0) * 0.01;
                    mean[col] += us;
                    mx[col] = std::max(mx[col], us);
                    ++cnt[col];
                }
            }
            for (int q = 0; q < 5; ++q) mean[q] /= std::max(1, cnt[q]);
            double fin_start = 0, fin_it = 0, tile_it = 0;
            for (int r = 0; r < nrole; ++r) {
                const unsigned long long *hh = &h[((size_t)r * (kResMaxSweeps + 1) + k) * 4];
                if (rp.fold) continue;  // (no finisher roles, no iteration counts)
                if (r < rp.nt) {
                    fin_start += (double)(hh[3] - t0) * 0.01 / rp.nt;
                    fin_it += (double)hh[2] / rp.nt;
                } else {
                    tile_it += (double)hh[3] / rp.ngroups;
                }
            }
            fprintf(stderr, "RES_STAMPS sweep %2d  finisher poll began %6.2f, iterations %.1f; tile poll iterations %.1f\n", k, fin_start,
                    fin_it, tile_it);
            fprintf(stderr, "RES_STAMPS sweep %2d  tiles: mu in %6.2f/%6.2f  product %6.2f/%6.2f  published %6.2f/%6.2f   finishers: sums in "
                            "%6.2f/%6.2f  mu out %6.2f/%6.2f\n", k, mean[0], mx[0], mean[1], mx[1], mean[2], mx[2], mean[3], mx[3],
                    mean[4], mx[4]);
        }
    }
    feed_side_stream(c);
    ++c->resident_calls;
    c->call.gs_used[0] = true;  // the sticky error word travels with the result record (publish_result_kernel)
    c->energy_part = v.energy_part;
    c->energy_nt = rp.nt;
    return 0;
}

// ---- exact dipoles (mpmc_hip_set_exact_polar, kernels_exact.h): the work copy the factorization runs in, the vectors of
// the substitutions (b, y, x: three right-hand sides each, stride 3 nvpad), the call's flag word and the tensor's nine
// sums.  Allocated on first use; a copy that does not fit is an error, by byte count.
static int ensure_exact_work(mpmc_hip_ctx *c, const SweepView &v) {
    const size_t lda = 3 * (size_t)v.nvpad, need = lda * lda;
    if (c->d_chol_W.size() < need) {
        c->chol_nv = 0;  // (whatever factor was there goes with its buffer)
        if (c->d_chol_W.alloc(need) != hipSuccess) {
            (void)hipGetLastError();
            return fail("MPMC_HIP: energy: exact polarization: the work copy of the %zu x %zu matrix, %zu bytes, does not fit "
                        "the device", lda, lda, need * sizeof(double));
        }
    }
    if (c->d_chol_vec.size() < 9 * lda) HIPCHK(c->d_chol_vec.alloc(9 * lda));
    if (!c->d_chol_flag) HIPCHK(c->d_chol_flag.alloc(2));
    if (!c->d_chol_tensor) HIPCHK(c->d_chol_tensor.alloc(9));
    return 0;
}

// A = L L^T of the view's matrix in the work copy: one copy, then diagonal block / panel / trailing update per panel of 64
// rows (the last panel has only its diagonal block): 3 np - 1 launches.  On timed calls the trailing updates carry their
// own begin / end timestamps (class T_SWEEP).
static int exact_factor(mpmc_hip_ctx *c, const SweepView &v) {
    const int n = 3 * v.nv, lda = 3 * v.nvpad, np = (n + kCholNB - 1) / kCholNB;
    hipLaunchKernelGGL(chol_copy_kernel, dim3(np, np), dim3(kCholThreads), 0, c->stream, (const double *)v.A, lda, n,
                       c->d_chol_W.get(), c->d_chol_flag.get());
    for (int k = 0; k < np; ++k) {
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(kCholThreads), 0, c->stream, c->d_chol_W.get(), lda, k,
                           c->d_chol_flag.get());
        const int m = np - 1 - k;
        if (m == 0) break;
        hipLaunchKernelGGL(chol_panel_kernel, dim3(m), dim3(kCholThreads), 0, c->stream, c->d_chol_W.get(), lda, k);
        HIPCHK(launch_timed(c, T_SWEEP, chol_trail_kernel, dim3(m, m), dim3(kCholThreads), 0, c->stream, c->d_chol_W.get(),
                            lda, k));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// L L^T x = b for NRHS right-hand sides on the factor in the work copy: x in the third of the three vectors.
// 2 np + 1 launches.
template <int NRHS>
static int exact_substitute(mpmc_hip_ctx *c, int nv, int nvpad, const double *es) {
    const int n = 3 * nv, lda = 3 * nvpad, np = (n + kCholNB - 1) / kCholNB;
    double *b = c->d_chol_vec, *y = b + 3 * (size_t)lda, *x = y + 3 * (size_t)lda;
    hipLaunchKernelGGL(chol_rhs_kernel<NRHS>, dim3(np), dim3(64), 0, c->stream, es, n, lda, b);
    for (int k = 0; k < np; ++k)
        hipLaunchKernelGGL(chol_fwd_kernel<NRHS>, dim3(np - k), dim3(kCholThreads), 0, c->stream, (const double *)c->d_chol_W.get(), lda,
                           k, b, y, lda);
    for (int k = np - 1; k >= 0; --k)
        hipLaunchKernelGGL(chol_bwd_kernel<NRHS>, dim3(k + 1), dim3(kCholThreads), 0, c->stream, (const double *)c->d_chol_W.get(), lda,
                           k, y, x, lda);
    HIPCHK(hipGetLastError());
    return 0;
}

// polar() with polar_iterative off (polar.c:91-95): the view's matrix is kept resident and updated as for the
// Gauss-Seidel kernels, the static field is gathered as ever, then A mu = E_static is solved directly.  No sweep, no
// ranking, no resident solver, no deferral: polar_iterations = 0, E_ind and dE_ind stay zero (the reference leaves them
// untouched on this path).  The flag word of the factorization travels in the record slot behind U_pol.
static int run_exact_polarization(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx) {
    SweepView *V = &c->view[0];
    if (setup_view(c, *V, a, bx, true, false, true)) return -1;
    if (launch_field(c, a, bx)) return -1;
    c->call.resident = false;
    c->psweep.drop();
    hipLaunchKernelGGL(init_view_kernel, dim3(V->nvpad / 64), dim3(64 * kFieldGroups), 0, c->stream, V->nv, V->nvpad,
                       V->d_idx, V->palpha, c->d_fieldpart, c->es_slots, c->npad, 1.0, V->es, V->mu0, V->efind, V->efchg,
                       V->rrms, c->d_errmax, (unsigned *)nullptr, (unsigned *)nullptr, (double *)nullptr, 0,
                       (size_t)3 * V->nvpad);
    if (ensure_exact_work(c, *V)) return -1;
    {
        ScopedTimer t(c, T_PALMO);  // (the whole solve; the trailing updates alone are the call's T_SWEEP records)
        if (exact_factor(c, *V)) return -1;
        // the device is busy now: feed the LJ / Ewald stream
        feed_side_stream(c);
        if (exact_substitute<1>(c, V->nv, V->nvpad, V->es)) return -1;
        hipLaunchKernelGGL(chol_energy_kernel, dim3(1), dim3(256), 0, c->stream, V->nv, V->nvpad,
                           (const double *)(c->d_chol_vec + 6 * (size_t)(3 * V->nvpad)), (const double *)V->palpha,
                           (const double *)V->es, (const unsigned *)c->d_chol_flag.get(), V->mu1.get(), c->d_res + R_UPOL);
    }
    c->chol_nv = V->nv;
    c->chol_nvpad = V->nvpad;
    {
        ScopedTimer t(c, T_EVPAIR);
    }
    c->result_view = V;
    c->result_mu = V->mu1;
    c->results_scattered = false;
    c->energy_nt = 0;
    c->have_polar_result = true;
    return 0;
}

// polar_gs_ranked: the ranking work of one call (a local of run_polarization()).  Two parts: (A) the metric's four kernels,
// (B) the ranked view's maintenance (speculative form) or the copy for the host's sort, and the event the main stream waits
// for at the view switch.
struct RankJob {
    bool ranked = false;     // the call ranks at all
    bool spec_rank = false;  // speculative form: the previous call's walk is assumed, the device checks it
    bool rank_side = false;  // the work runs on the side stream
    hipStream_t rs = nullptr;
    bool enqueued = false, metric_enqueued = false;  // part B (which includes A) / part A went out
};

// (A) the ranking metric (pairs.c:337-360), once per call
static void enqueue_rank_metric(mpmc_hip_ctx *c, RankJob &rj, const DevAtoms &a, const DevBox &bx) {
    if (rj.metric_enqueued || !rj.ranked) return;
    rj.metric_enqueued = true;
    const int npad = c->npad, n = c->n;
    const hipStream_t rs = rj.rs;
    if (rj.rank_side) side_wait_for_moves(c, rs);  // the new coordinates are in place on this stream too
    ScopedTimer t(c, T_OTHER, rs);
    const int ntile = npad / 64;
    // scratch of its own: the static-field and pair partials persist between calls
    hipLaunchKernelGGL(rank_rmin_kernel, dim3(ntile, ntile), dim3(64), 0, rs, a, bx, c->d_rankpart);
    // (the counters and the "ranking changed" word are cleared by the same launch)
    hipLaunchKernelGGL(reduce_min_kernel, dim3(1), dim3(256), 0, rs, c->d_rankpart, ntile * ntile,
                       c->d_res + R_RMIN, c->d_rankcnt, npad, c->d_res + R_RANKCHG);
    const ChunkPlan cp = chunk_plan(npad, 2048);
    hipLaunchKernelGGL(rank_count_kernel, dim3(cp.nchunk, ntile), dim3(64), 0, rs, a, c->d_res + R_RMIN, cp.chunk,
                       c->d_rankcnt);
    hipLaunchKernelGGL(count_to_rank_kernel, dim3((npad + 255) / 256), dim3(256), 0, rs, npad, c->d_rankcnt,
                       c->d_rank, n, rj.spec_rank ? (const double *)c->d_rank_used : (const double *)nullptr,
                       c->d_res + R_RANKCHG);
}

// (B) and (A), once per call
static int enqueue_rank(mpmc_hip_ctx *c, RankJob &rj, const DevAtoms &a, const DevBox &bx) {
    if (rj.enqueued || !rj.ranked) return 0;
    rj.enqueued = true;
    const hipStream_t rs = rj.rs;
    if (rj.spec_rank) {
        // The ranked view, for the same walk as in the previous call: only what the moved atoms touch is redone.  This
        // does not depend on the metric, and it is what the main stream waits for at the view switch: it goes FIRST
        // (unless the metric's kernels are out already: rank_late = 2), the metric's kernels -- whose verdict only the
        // host reads, at the end of the call -- behind it.  (At 1024 atoms the side stream's eight small launches in
        // the old order took longer than the main stream's set-up + first sweep, which then waited ~25 us.)
        SweepView &W = c->view[1];
        if (rj.rank_side) side_wait_for_moves(c, rs);
        W.ranked_call = c->energy_calls;
        if (setup_view(c, W, a, bx, true, true, false, true, rs)) return -1;
        hipEventRecord(c->ev_rank, rs);
        enqueue_rank_metric(c, rj, a, bx);
    } else if (rj.rank_side) {
        // the metric is only needed after the first sweep: it is computed on the side stream, beside that sweep
        enqueue_rank_metric(c, rj, a, bx);
        // the host will sort the metric: bring it over behind the rank kernels, so that at the view switch the host
        // waits for this copy only (not for the first sweep) and sorts while the device still works on that sweep
        HIPCHK(hipMemcpyAsync(c->h_rank, c->d_rank, c->n * sizeof(double), hipMemcpyDeviceToHost, rs));
        hipEventRecord(c->ev_rank, rs);
    } else {
        enqueue_rank_metric(c, rj, a, bx);  // (one stream: the metric's kernels in line, the host copies it at the view switch)
    }
    c->call.rank_on_side = rj.rank_side && !rj.spec_rank;
    return 0;
}

// update_ranking (thole_iterative.c:143-164), host form: the metric comes to the host, is sorted (ranked_walk), and view 1
// becomes the ranked view -- maintained if the walk is the previous call's, else rebuilt.  On the side stream where the
// metric was made there, beside the first sweep that the main stream is still working on.
static int rebuild_ranked_view(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, bool chain_mode) {
    const int npad = c->npad, n = c->n;
    SweepView &W = c->view[1];
    const SweepView &V0 = c->view[0];
    if (c->call.rank_on_side) {
        HIPCHK(hipEventSynchronize(c->ev_rank));           // the metric is on the host
        hipStreamWaitEvent(c->stream, c->ev_rank, 0);      // and d_rank is complete for the main stream
    } else {
        HIPCHK(hipMemcpyAsync(c->h_rank, c->d_rank, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    // The ranked view is (re)built on the SIDE stream, where the metric was made, beside the first sweep that
    // the main stream is still working on -- after a grand-canonical edit that is a whole view (coefficient
    // tiles, block inverses, tensor tiles: ~100 us at 4096 atoms), which used to wait in the main stream's
    // queue behind that sweep and then run alone.  (The side stream has nothing else queued yet: the LJ /
    // Ewald kernels are fed at the end of the call.)
    const bool view_on_side = c->call.rank_on_side && chain_mode && c->opt.rank_view_side;
    const hipStream_t ws = view_on_side ? c->stream2 : c->stream;
    const double *rk = c->h_rank;
    c->rank_saved.assign(rk, rk + n);  // for mpmc_hip_download_ranking (the full ranked_array is made there)
    c->perm_ranked = true;
    // a stable sort of view 0's order (= the caller's atom order, also after grand-canonical edits) by the metric
    const int nv = (int)V0.h_idx.size();
    ranked_walk(rk, V0.h_idx, c->h_perm.get());
    // A single-molecule move rarely changes the ranked order: if the walk is the one of the previous
    // call, the ranked view's data are still resident and only what the moved atoms touch is redone
    // (the reference rebuilds everything; so did this engine: 118 us at 4096 atoms).
    const bool same_walk = (chain_mode ? W.C_valid : (W.A_valid && (W.C_valid || !c->opt.pair_coef))) &&
                           W.ranked_call + 1 == c->energy_calls && W.nv == nv &&
                           W.nvpad == V0.nvpad && std::equal(c->h_perm.get(), c->h_perm + nv, W.h_idx.begin());
    W.ranked_call = c->energy_calls;
    if (!same_walk) {
        W.nv = nv;
        W.nvpad = V0.nvpad;
        W.h_idx.assign(c->h_perm.get(), c->h_perm + nv);
        W.slot_of_atom.assign(n, -1);
        for (int k = 0; k < npad; ++k) c->h_slotmap[k] = -1;
        for (int k = 0; k < nv; ++k) {
            W.slot_of_atom[c->h_perm[k]] = k;
            c->h_slotmap[c->h_perm[k]] = k;
        }
        // (pinned sources: asynchronous copies in stream order; the host does not touch them again
        // before energy_end() has returned)
        HIPCHK(hipMemcpyAsync(W.d_idx, c->h_perm, nv * sizeof(int), hipMemcpyHostToDevice, ws));
        HIPCHK(hipMemcpyAsync(W.d_slot, c->h_slotmap, npad * sizeof(int), hipMemcpyHostToDevice, ws));
        W.A_valid = false;
        W.C_valid = false;
    }
    if (setup_view(c, W, a, bx, same_walk, c->opt.pair_coef != 0, !chain_mode, chain_mode,
                   view_on_side ? ws : (hipStream_t) nullptr))
        return -1;
    // what later speculative calls are checked against: the metric this walk was sorted from
    HIPCHK(hipMemcpyAsync(c->d_rank_used, c->d_rank, n * sizeof(double), hipMemcpyDeviceToDevice, ws));
    c->rank_used_valid = true;
    if (view_on_side) {  // the main stream picks the ranked view up at the view switch
        hipEventRecord(c->ev_rank, ws);
        hipStreamWaitEvent(c->stream, c->ev_rank, 0);
    }
    return 0;
}

// The switch to the ranked view behind the first sweep: the view is ready (speculative form: maintained on the side
// stream; else rebuild_ranked_view()), then the static field and current dipoles of the same atoms go from view 0 to
// view 1 and the per-call scratch is cleared.  The solve goes on in view 1: V, mu_in, mu_out are its.
static int switch_to_ranked_view(mpmc_hip_ctx *c, const RankJob &rj, const DevAtoms &a, const DevBox &bx, bool chain_mode,
                                 SweepView *&V, double *&mu_in, double *&mu_out) {
    SweepView &W = c->view[1];
    ScopedTimer t(c, T_OTHER);
    if (rj.spec_rank) {
        // the walk of the previous call, already maintained on the side stream
        hipStreamWaitEvent(c->stream, c->ev_rank, 0);
    } else if (rebuild_ranked_view(c, a, bx, chain_mode)) {
        return -1;
    }
    const dim3 gvec((V->nvpad + 255) / 256), bvec(256);
    hipLaunchKernelGGL(switch_view_kernel, gvec, bvec, 0, c->stream, W.nv, W.nvpad, W.d_idx, c->view[0].d_slot,
                       c->view[0].es, mu_in, W.es, W.mu0, W.efchg, W.rrms);
    V = &W;
    mu_in = W.mu0;
    mu_out = W.mu1;
    return 0;
}

static int run_polarization(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, int *n_iter, int *iter_success) {
    const mpmc_hip_params &P = c->par;
    const int n = c->n;
    const bool gs = c->call.gs_mode;
    const bool want_rrms = P.polar_rrms || P.polar_precision > 0.0;
    *n_iter = 0;
    *iter_success = 0;
    c->energy_nt = 0;
    c->call.gs_sweeps = 0;
    if (c->call.exact) return run_exact_polarization(c, a, bx);
    // ---- ranking metric (pairs.c:337-360), needed from the 2nd sweep on.
    // Speculative form: the ranked view (1) of the previous call is assumed to be still the right walk (a single-
    // molecule move changes the metric only when molecules come within 1.5 r_min of each other); its data are brought
    // up to date and the metric is computed on the SIDE stream beside the first sweep, the device checks the
    // assumption (count_to_rank_kernel), and energy_end() repeats the call with the host in the loop if it failed.
    const bool ranked = P.polar_gs_ranked && !P.polar_zodid;
    SweepView &W = c->view[1];
    const bool chain_mode = gs && gs_uses_chain(c);
    const bool spec_rank = ranked && chain_mode && c->opt.spec_rank && c->opt.overlap && !c->force_host_rank &&
                           P.polar_precision == 0.0 && P.polar_max_iter >= 2 && c->rank_used_valid && W.C_valid &&
                           W.ranked_call + 1 == c->energy_calls && W.nvpad == c->view[0].nvpad &&
                           W.nv == c->view[0].nv && (int)c->rank_saved.size() == n && !c->all_dirty;
    c->call.spec_rank = spec_rank;
    c->perm_ranked = spec_rank;  // mpmc_hip_download_ranking sorts the saved metric when asked (else: identity)
    // (Enqueued AFTER the first sweep's launches -- enqueue_rank() below: the host needs ~4 us per launch, and with these
    //  8-9 side-stream launches in front the main stream sat idle for ~35 us at the head of every step, waiting for its
    //  own first kernels to be enqueued; the side stream still has the whole first sweep to do its work in.)
    // Two parts: (A) the metric's four kernels, (B) the ranked view's maintenance (speculative form) or the copy for the
    // host's sort, and the event the main stream waits for at the view switch.
    RankJob rj;
    rj.ranked = ranked;
    rj.spec_rank = spec_rank;
    rj.rank_side = ranked && (spec_rank || (c->opt.overlap && chain_mode));
    rj.rs = rj.rank_side ? c->stream2 : c->stream;
    // (only the speculative form waits: when the host has to sort the metric in the middle of the call, the sooner the
    //  rank kernels start the sooner it can)
    if (!(c->opt.rank_late && spec_rank) && enqueue_rank(c, rj, a, bx)) return -1;

    // ---- A matrix of the polarizable block (thole_matrix.c:38-146)
    SweepView *V = &c->view[0];
    if (!P.polar_zodid) {
        // Jacobi-type solves run on pair coefficients alone; the Gauss-Seidel kernels walk rows of the expanded
        // matrix, and take their upper-triangle product from the coefficients as well
        const bool chain = gs && gs_uses_chain(c);
        if (setup_view(c, *V, a, bx, true, c->opt.pair_coef != 0, (gs && !chain) || !c->opt.pair_coef, chain)) return -1;
    } else {
        const dim3 g((V->nvpad + 255) / 256), b(256);
        hipLaunchKernelGGL(gather_atoms_kernel, g, b, 0, c->stream, V->nv, V->nvpad, V->d_idx, a, V->px, V->py, V->pz,
                           V->palpha, V->pflags);
    }

    // (rank_late = 2: the metric's four kernels go out here, behind the main stream's first launches -- the moved blocks'
    //  coefficient update and block inverse keep the device busy for ~25 us while the host enqueues them -- so that the
    //  heavy ranking kernels run beside the view set-up rather than beside the latency-bound chain of the first sweep)
    if (ranked && spec_rank && c->opt.rank_late >= 2) enqueue_rank_metric(c, rj, a, bx);

    // ---- static field for every atom (thole_field.c:14-36)
    if (launch_field(c, a, bx)) return -1;

    // ---- init_dipoles (thole_iterative.c:13-25), fused with the gather of E_static into the view
    double *mu_in = V->mu0, *mu_out = V->mu1;
    // a fixed-count Jacobi-type solve that fits the chip runs as ONE launch with its tiles in registers
    const ResidentPlan rp = resident_plan(c, *V);
    if (rp.ok && ensure_view_resident(c, *V)) return -1;
    c->call.resident = rp.ok;
    {
        const double scale = (!P.polar_sor && !P.polar_esor) ? P.polar_gamma : 1.0;
        hipLaunchKernelGGL(init_view_kernel, dim3(V->nvpad / 64), dim3(64 * kFieldGroups), 0, c->stream, V->nv,
                           V->nvpad, V->d_idx, V->palpha, c->d_fieldpart, c->es_slots, c->npad, scale, V->es, mu_in,
                           V->efind, V->efchg, V->rrms, c->d_errmax,
                           (chain_mode || rp.ok) ? c->view[0].gsflags : (unsigned *)nullptr,
                           chain_mode ? c->view[1].gsflags : (unsigned *)nullptr,
                           rp.ok ? V->respub : (double *)nullptr, P.polar_max_iter, (size_t)3 * V->nvpad);
    }

    int iteration_counter = 0;
    bool ranked_active = false;  // becomes true after the first update_ranking()
    const bool defer = !rp.ok && defer_last_sweep(c, *V);
    c->psweep.drop();  // (begin_call() has; an abandoned graph capture runs this function twice in one call)
    if (rp.ok) {
        if (launch_resident(c, *V, bx, rp, want_rrms)) return -1;
        iteration_counter = P.polar_max_iter;
        mu_in = V->mu1;  // where the finishers leave the final dipoles
    } else if (!P.polar_zodid) {
        bool keep_iterating = true;
        while (keep_iterating) {
            iteration_counter++;
            const int nvpad = V->nvpad;
            const dim3 gvec((nvpad + 255) / 256), bvec(256);
            // divergence detection (thole_iterative.c:199-210)
            if (iteration_counter >= kMAX_ITERATION_COUNT && P.polar_precision != 0.0) {
                hipLaunchKernelGGL(fallback_dipoles_kernel, gvec, bvec, 0, c->stream, nvpad, V->palpha, V->es, mu_in,
                                   V->efchg);
                *iter_success = 1;
                break;
            }
            double w_new, w_old;
            mixing_weights(P.polar_sor, P.polar_esor, P.polar_gamma, iteration_counter, w_new, w_old);
            const double *palmo_mu = mu_in;  // Jacobi: mu still holds the pre-sweep values
            if (!gs) {
                const SweepParams sp = jacobi_sweep_params(iteration_counter, P.polar_max_iter, P.polar_precision, want_rrms,
                                                           defer, w_new, w_old);
                const int mid = (P.polar_max_iter + 1) / 2;
                // sweep n, and sweeps m + 1 .. n - 1 once the record HAS gone out behind the finish of sweep m (published: not
                // on a timed or captured call, nor while a builder join is pending): recorded in order, not launched
                // (complete_pending_sweep()).  The ping-pong below goes on as if they had been.
                if (sweep_is_pending(iteration_counter, P.polar_max_iter, defer, c->call.published)) {
                    PendingSweep &ps = c->psweep;
                    ps.view = V;
                    ps.bx = bx;
                    PendingSweep::One one;
                    one.mu_in = mu_in;
                    one.mu_out = mu_out;
                    one.sp = sp;
                    ps.sweeps.push_back(one);
                } else if (launch_sweep<kSweepJacobi>(c, *V, bx, mu_in, mu_out, sp, T_SWEEP)) {
                    return -1;
                }
                // the device is busy now: feed the LJ/Ewald stream (its ~55 us of kernels only have to be done by the
                // time the last sweep is)
                if (iteration_counter == c->opt.side_after || P.polar_max_iter < c->opt.side_after) feed_side_stream(c);
                // U_pol is complete behind this finish: the record goes out here, and sweeps m + 1 .. n - 1, which only a
                // later reader of the dipoles needs, are then left to that reader (above) (enqueue_direct; the side stream
                // is fed first, so that the host is not left waiting for a record whose other half has not been enqueued)
                if (defer && iteration_counter == mid && c->call.may_publish_early) {
                    feed_side_stream(c);
                    publish_early(c);
                }
            } else {
                GsFinishArgs gfa;
                gfa.w_new = w_new;
                gfa.w_old = w_old;
                gfa.want_rrms = (int)want_rrms;
                gfa.err_slot = (P.polar_precision > 0.0) ? iteration_counter : -1;
                gfa.mu_out = mu_out;
                bool finished = false;  // the chain kernel's workgroups did the block's end-of-sweep bookkeeping themselves
                if (launch_gs_sweep(c, *V, a, bx, mu_in, &gfa, &finished)) return -1;
                const bool planar = gs_uses_chain(c) && V->C_valid;  // what launch_gs_sweep just ran
                if (!finished)
                hipLaunchKernelGGL(gs_finish_kernel, gvec, bvec, 0, c->stream, nvpad, V->palpha, V->pflags, mu_in,
                                   (const double *)(planar ? V->mupub : V->munew), planar ? 1 : 0, V->y, w_new, w_old,
                                   (int)want_rrms, iteration_counter, mu_out, planar ? V->munew : (double *)nullptr,
                                   V->efind, V->rrms, c->d_errmax);
                palmo_mu = V->munew;  // GS updated mu in place: the contraction sees the new dipoles
            }

            // are_we_done_yet (thole_iterative.c:94-117)
            if (P.polar_precision == 0.0) {
                keep_iterating = (iteration_counter != P.polar_max_iter);
            } else {
                HIPCHK(hipMemcpyAsync(c->h_err, c->d_errmax + iteration_counter, sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
                double emax;
                memcpy(&emax, c->h_err, sizeof(double));
                const double allowed = P.polar_precision * P.polar_precision * kDEBYE2SKA * kDEBYE2SKA;
                keep_iterating = (emax > allowed);
            }

            // Palmo-Krimm: one more contraction for the change in induced field (thole_iterative.c:233-235)
            if (P.polar_palmo && !keep_iterating) {
                SweepParams sp;
                sp.w_new = 1.0;
                sp.w_old = 0.0;
                sp.want_rrms = 0;
                sp.want_err = 0;
                sp.err_slot = 0;
                sp.skip_sums = 0;
                if (launch_sweep<kSweepPalmo>(c, *V, bx, palmo_mu, V->efchg, sp, T_PALMO, gs ? V->munew : mu_out)) return -1;
            }

            std::swap(mu_in, mu_out);  // "save the dipoles for the next pass" (thole_iterative.c:238-252)

            // update_ranking (thole_iterative.c:143-164): stable descending sort of rank_metric.  After the
            // first call the order is final, so the ranked view is set up exactly once per energy().
            // the first sweep is enqueued: now the ranking work, on its stream
            if (enqueue_rank(c, rj, a, bx)) return -1;
            if (ranked && keep_iterating && !ranked_active) {
                if (switch_to_ranked_view(c, rj, a, bx, chain_mode, V, mu_in, mu_out)) return -1;
                ranked_active = true;
            }
        }
    }
    *n_iter = iteration_counter;
    if (enqueue_rank(c, rj, a, bx)) return -1;  // (no sweep ran: the metric is still part of the call's results)

    {
        // calibration for the event-pair timings above: two event records with nothing in between
        ScopedTimer t(c, T_EVPAIR);
    }
    // ---- mu, E_ind, dE_ind stay in view order until download_dipoles() asks for atom order
    c->result_view = V;
    c->result_mu = mu_in;
    c->results_scattered = false;
    // ---- U_pol and <rrms> (polar.c:13-28, :107-116): folded from the finish step's per-block sums by the
    // publish kernel, or by a pass of its own on the other solver paths
    if (P.polar_zodid || iteration_counter == 0 || *iter_success) c->energy_nt = 0;
    if (c->energy_nt == 0) {
        ScopedTimer t(c, T_OTHER);
        hipLaunchKernelGGL(polar_energy_kernel, dim3(1), dim3(256), 0, c->stream, V->nv, n, mu_in, V->es, V->efchg,
                           P.polar_palmo, V->rrms, c->d_res + R_UPOL);
    }
    c->have_polar_result = true;
    return 0;
}
