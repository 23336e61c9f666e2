// engine_dense.inc -- host side of the dense energy modes (DESIGN.md section 1b and sections 9-12, 15): the setters of
// disp_expansion, axilrod_teller, rd_crystal, set_rd_form, polarvdw and the close-contact count with their getters, the tile
// pass scaffold (TileSum: tile_pass / static_pass / lrc_pass) and the launches of each mode's sums.  Included by engine.hip.

// the zero epsilon / sigma the Lennard-Jones kernels read under disp_expansion and rd_crystal
static int alloc_zero_params(mpmc_hip_ctx *c) {
    if (c->d_zero) return 0;
    HIPCHK(c->d_zero.alloc(c->max_npad));
    HIPCHK(hipMemsetAsync(c->d_zero, 0, (size_t)c->max_npad * sizeof(double), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
// The [ntile * ntile] tile partials of a mode's sums, allocated the first time the mode is switched on.
static int alloc_tile_parts(mpmc_hip_ctx *c, std::initializer_list<TileSum *> sums) {
    const size_t ntile = c->max_npad / 64;
    for (TileSum *ts : sums)
        if (!ts->part) HIPCHK(ts->part.alloc(ntile * ntile));
    return 0;
}
// What the setters of per-atom data refuse before anything else (`name`: the setter's, as its messages spell it).
static int per_atom_setter_refused(const mpmc_hip_ctx *c, const char *name) {
    if (c->in_flight) return fail("MPMC_HIP: %s between energy_begin() and energy_end()", name);
    if (!c->have_atoms) return fail("MPMC_HIP: %s: no configuration uploaded", name);
    if (c->edited) return fail("MPMC_HIP: %s: molecules were inserted or removed since the upload", name);
    return 0;
}
// The Lennard-Jones kernels change between real and zero parameters: how every setter of a mode that owns rd_energy ends.
// Two differences are on purpose: a call that changes nothing returns before it drops anything, and set_vdw() with new
// frequencies in a mode that is already on leaves the Lennard-Jones partials alone (their parameters stay zero).
static void lj_kernels_switched(mpmc_hip_ctx *c) {
    c->pair_part_valid = c->lrc.valid = false;
    c->all_dirty = true;
    ++c->config_rev;
}
// disp_expansion (PHAHST): the resident epsilon / sigma become the exponent b and the range rho of the exponential
// repulsion, and c6 / c8 / c10 (atomic units, upload order) arrive here.  Until the next upload the LJ kernels see zero
// parameters and the dense kernels of kernels_disp.h form rd_energy.
extern "C" int mpmc_hip_set_dispersion(mpmc_hip_ctx *c, const mpmc_hip_disp_params *p, int n, const double *c6,
                                       const double *c8, const double *c10) {
    if (!c || !p) return fail("MPMC_HIP: set_dispersion: null argument");
    if (per_atom_setter_refused(c, "set_dispersion")) return -1;
    if (n != c->n) return fail("MPMC_HIP: set_dispersion: %d coefficients for the %d atoms of the upload", n, c->n);
    HIPCHK(hipSetDevice(c->device));
    if (flush_moves(c)) return -1;  // keep the order of the caller's operations
    c->disp.valid = c->disp_lrc.valid = false;
    lj_kernels_switched(c);
    if (!p->disp_expansion) {
        c->disp_on = false;
        return 0;
    }
    if (!c6 || !c8 || !c10) return fail("MPMC_HIP: set_dispersion: null array");
    const size_t nall = c->max_npad;
    if (!c->d_c6) {
        HIPCHK(c->d_c6.alloc(nall));
        HIPCHK(c->d_c8.alloc(nall));
        HIPCHK(c->d_c10.alloc(nall));
    }
    if (alloc_tile_parts(c, {&c->disp, &c->disp_lrc}) || alloc_zero_params(c)) return -1;
    std::vector<double> h6(nall, 0.0), h8(nall, 0.0), h10(nall, 0.0);  // pad atoms: zeros
    std::copy(c6, c6 + n, h6.begin());
    std::copy(c8, c8 + n, h8.begin());
    std::copy(c10, c10 + n, h10.begin());
    const size_t bd = nall * sizeof(double);
    HIPCHK(hipMemcpyAsync(c->d_c6, h6.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_c8, h8.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_c10, h10.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->disp_par.damp = p->damp_dispersion != 0;
    c->disp_par.extrapolate = p->extrapolate_disp_coeffs != 0;
    c->disp_par.schmidt = p->schmidt_mixing != 0;
    c->disp_on = true;
    return 0;
}

// axilrod_teller: the triple-dipole term.  c9 (atomic units, upload order) is the EFFECTIVE per-atom coefficient: under
// midzuno_kihara_approx the caller has already replaced it by 3/4 alpha 6.7483345 c6.  The polarizabilities are the upload's.
extern "C" int mpmc_hip_set_axilrod_teller(mpmc_hip_ctx *c, int enable, int n, const double *c9) {
    if (!c) return fail("MPMC_HIP: set_axilrod_teller: null context");
    if (per_atom_setter_refused(c, "set_axilrod_teller")) return -1;
    HIPCHK(hipSetDevice(c->device));
    if (!enable) {
        if (flush_moves(c)) return -1;
        c->at_on = false;
        c->at.valid = false;
        ++c->config_rev;
        return 0;
    }
    if (n != c->n) return fail("MPMC_HIP: set_axilrod_teller: %d coefficients for the %d atoms of the upload", n, c->n);
    if (!c9) return fail("MPMC_HIP: set_axilrod_teller: null array");
    if (flush_moves(c)) return -1;  // keep the order of the caller's operations
    const size_t nall = c->max_npad;
    std::vector<double> ha(nall, 0.0), hg(nall, 1.0);  // pad atoms: no three-body site
    HIPCHK(hipMemcpyAsync(ha.data(), c->d_alpha, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
        const double alpha = ha[i];
        if (alpha < 0.0) return fail("MPMC_HIP: set_axilrod_teller: negative polarizability %g of atom %d", alpha, i);
        at_site_values(alpha, c9[i], ha[i], hg[i]);
    }
    if (!c->d_at_a) {
        HIPCHK(c->d_at_a.alloc(nall));
        HIPCHK(c->d_at_g.alloc(nall));
        HIPCHK(c->at.part.alloc((size_t)at_unit_count((int)(nall / 64)) * kAtSplit));
    }
    const size_t bd = nall * sizeof(double);
    HIPCHK(hipMemcpyAsync(c->d_at_a, ha.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_at_g, hg.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->at.valid = false;
    c->at_on = true;
    ++c->config_rev;
    return 0;
}

// rd_crystal: Lennard-Jones summed over the lattice images n in {-(order-1) .. order-1}^3 out to
// 2 * pbc_cutoff * (order - 0.5) (kernels_crystal.h).  0 switches it off.  A setting of the context, like set_params().
extern "C" int mpmc_hip_set_rd_crystal(mpmc_hip_ctx *c, int order) {
    if (!c) return fail("MPMC_HIP: set_rd_crystal: null context");
    if (c->in_flight) return fail("MPMC_HIP: set_rd_crystal between energy_begin() and energy_end()");
    if (order < 0 || order > kRdcMaxOrder)
        return fail("MPMC_HIP: set_rd_crystal: rd_crystal_order %d outside 1 .. %d (0 = off)", order, kRdcMaxOrder);
    if (order == c->rdc_order) return 0;  // nothing to change: no partial sum is thrown away
    HIPCHK(hipSetDevice(c->device));
    if (c->have_atoms && flush_moves(c)) return -1;  // keep the order of the caller's operations
    if (order > 0 && (alloc_zero_params(c) || alloc_tile_parts(c, {&c->rdc, &c->rdc_static}))) return -1;
    c->rdc_order = order;
    c->rdc.valid = c->rdc_static.valid = false;
    lj_kernels_switched(c);  // (between two orders too, as it always has)
    return 0;
}

// The pair potentials beside plain Lennard-Jones (kernels_rdforms.h): form 0 returns to the standard path.  A setting of
// the context, like set_rd_crystal().  Under the SG form the context evaluates what it evaluates under rd_only.
extern "C" int mpmc_hip_set_rd_form(mpmc_hip_ctx *c, const mpmc_hip_rd_form_params *p) {
    if (!c || !p) return fail("MPMC_HIP: set_rd_form: null argument");
    if (c->in_flight) return fail("MPMC_HIP: set_rd_form between energy_begin() and energy_end()");
    if (p->form < 0 || p->form > MPMC_HIP_RD_BUFFERED_14_7)
        return fail("MPMC_HIP: set_rd_form: form %d outside 0 .. %d", p->form, MPMC_HIP_RD_BUFFERED_14_7);
    if (p->mixing < 0 || p->mixing > MPMC_HIP_RD_MIX_C6)
        return fail("MPMC_HIP: set_rd_form: mixing %d outside 0 .. %d", p->mixing, MPMC_HIP_RD_MIX_C6);
    const int mix = p->form ? p->mixing : 0;
    if (p->form == c->rd_form && mix == c->rd_mix) return 0;  // nothing to change: no partial sum is thrown away
    HIPCHK(hipSetDevice(c->device));
    if (complete_pending_sweep(c)) return -1;
    if (c->have_atoms && flush_moves(c)) return -1;  // keep the order of the caller's operations
    if (p->form && (alloc_zero_params(c) || alloc_tile_parts(c, {&c->rdf, &c->rdf_lrc}))) return -1;
    const bool rd_only_changes = (p->form == kRdFormSG) != (c->rd_form == kRdFormSG);
    c->rd_form = p->form;
    c->rd_mix = mix;
    c->rdf.valid = c->rdf_lrc.valid = false;
    if (rd_only_changes && c->have_params) {  // as a set_params() that changes rd_only
        c->par = c->par_user;
        if (c->rd_form == kRdFormSG) c->par.rd_only = 1;
        params_or_grid_changed(c);
        c->kvecf_valid = false;
        c->kvec_valid = false;
    }
    lj_kernels_switched(c);  // (between two forms or mixing rules too, as it always has)
    return 0;
}

extern "C" int mpmc_hip_get_three_body_energy(mpmc_hip_ctx *c, double *out) {
    if (!c || !out) return fail("MPMC_HIP: get_three_body_energy: null argument");
    if (c->in_flight) return fail("MPMC_HIP: get_three_body_energy between energy_begin() and energy_end()");
    *out = c->at_on ? c->three_body : 0.0;
    return 0;
}

// polarvdw: the coupled-dipole many-body van der Waals term and repulsion-only Lennard-Jones (kernels_vdw.h).  omega
// (atomic units, upload order) and the type id of every atom's molecule arrive here; the polarizabilities and the
// molecules are the upload's.  Until the next upload the LJ kernels see zero parameters.
extern "C" int mpmc_hip_set_vdw(mpmc_hip_ctx *c, int enable, int n, const double *omega, const int *mol_type) {
    if (!c) return fail("MPMC_HIP: set_vdw: null context");
    if (per_atom_setter_refused(c, "set_vdw")) return -1;
    HIPCHK(hipSetDevice(c->device));
    if (!enable) {
        c->vdw_iso.clear();
        if (!c->vdw_on) return 0;
        if (flush_moves(c)) return -1;
        c->vdw_on = false;
        c->rep.valid = c->rep_lrc.valid = c->vdw.valid = c->vdw_lrc.valid = false;
        lj_kernels_switched(c);
        return 0;
    }
    if (n != c->n) return fail("MPMC_HIP: set_vdw: %d frequencies for the %d atoms of the upload", n, c->n);
    if (!omega || !mol_type) return fail("MPMC_HIP: set_vdw: null array");
    if (flush_moves(c)) return -1;  // keep the order of the caller's operations
    const size_t nall = c->max_npad;
    std::vector<double> ha(nall, 0.0), hw(nall, 0.0), hk;
    std::vector<int> hmol(nall, 0), hidx;
    HIPCHK(hipMemcpyAsync(ha.data(), c->d_alpha, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hmol.data(), c->d_mol, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<mpmc_hip_ctx::VdwMolecule> mols;
    for (int i = 0; i < n; ++i) {
        if (ha[i] < 0.0) return fail("MPMC_HIP: set_vdw: negative polarizability %g of atom %d", ha[i], i);
        if (i == 0 || hmol[i] != hmol[i - 1]) {
            mols.push_back({mol_type[i], (int)hidx.size(), 0});
        } else if (mol_type[i] != mols.back().type) {
            return fail("MPMC_HIP: set_vdw: atom %d has type id %d, its molecule %d", i, mol_type[i], mols.back().type);
        }
        hw[i] = omega[i];
        const double k = std::sqrt(ha[i]) * omega[i];  // getsqrtKinv, vdw.c:337
        if (k != 0.0) {  // build_M leaves the others out (vdw.c:119)
            hidx.push_back(i);
            hk.push_back(k);
            ++mols.back().sites;
        }
    }
    const int na = (int)hidx.size();
    if (!c->d_vdw_w) {
        HIPCHK(c->d_vdw_w.alloc(nall));
        HIPCHK(c->d_vdw_idx.alloc(nall));
        HIPCHK(c->d_vdw_k.alloc(nall));
    }
    if (alloc_tile_parts(c, {&c->vdw_lrc, &c->rep, &c->rep_lrc}) || alloc_zero_params(c)) return -1;
    const size_t nc = 3 * (size_t)std::max(na, 1);
    if (c->d_vdw_C.size() < nc * nc) {
        HIPCHK(c->d_vdw_C.alloc(nc * nc));
        HIPCHK(c->d_vdw_vec.alloc(5 * nc + 2));
    }
    HIPCHK(hipMemcpyAsync(c->d_vdw_w, hw.data(), nall * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (na > 0) {
        HIPCHK(hipMemcpyAsync(c->d_vdw_idx, hidx.data(), (size_t)na * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_vdw_k, hk.data(), (size_t)na * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->vdw_na = na;
    c->vdw_mols = std::move(mols);
    c->vdw_iso_summed = false;
    c->rep.valid = c->rep_lrc.valid = c->vdw.valid = c->vdw_lrc.valid = false;
    if (c->vdw_on)
        ++c->config_rev;  // (new frequencies in a mode that was on: the Lennard-Jones kernels keep their zero parameters)
    else
        lj_kernels_switched(c);
    c->vdw_on = true;
    return 0;
}

extern "C" int mpmc_hip_get_vdw_energy(mpmc_hip_ctx *c, double *out) {
    if (!c || !out) return fail("MPMC_HIP: get_vdw_energy: null argument");
    if (c->in_flight) return fail("MPMC_HIP: get_vdw_energy between energy_begin() and energy_end()");
    *out = c->vdw_on ? c->vdw_energy : 0.0;
    return 0;
}

extern "C" int mpmc_hip_get_vdw_terms(mpmc_hip_ctx *c, double terms[5]) {
    if (!c || !terms) return fail("MPMC_HIP: get_vdw_terms: null argument");
    if (c->in_flight) return fail("MPMC_HIP: get_vdw_terms between energy_begin() and energy_end()");
    for (int k = 0; k < 5; ++k) terms[k] = c->vdw_on ? c->vdw_terms[k] : 0.0;
    return 0;
}

// cavity_autoreject_absolute: count the pairs on different molecules closer than `scale` (kernels_vdw.h).  0 switches it
// off.  A setting of the context, like set_rd_crystal().
extern "C" int mpmc_hip_set_autoreject(mpmc_hip_ctx *c, double scale) {
    if (!c) return fail("MPMC_HIP: set_autoreject: null context");
    if (c->in_flight) return fail("MPMC_HIP: set_autoreject between energy_begin() and energy_end()");
    if (!(scale >= 0.0) || !std::isfinite(scale)) return fail("MPMC_HIP: set_autoreject: scale %g (0 = off)", scale);
    if (scale == c->autoreject_scale) return 0;
    HIPCHK(hipSetDevice(c->device));
    if (c->have_atoms && flush_moves(c)) return -1;  // keep the order of the caller's operations
    c->autoreject_scale = scale;
    c->pair_part_valid = false;  // the count travels in the pair kernel's tile partials
    c->all_dirty = true;
    ++c->config_rev;
    return 0;
}

extern "C" int mpmc_hip_get_close_contacts(mpmc_hip_ctx *c, long long *count) {
    if (!c || !count) return fail("MPMC_HIP: get_close_contacts: null argument");
    if (c->in_flight) return fail("MPMC_HIP: get_close_contacts between energy_begin() and energy_end()");
    *count = c->autoreject_scale != 0.0 ? c->close_contacts : 0;
    return 0;
}

// ---- Dense tile sums (kernels_tile.h).  The fixed-order sum of a TileSum's partials into its slot of d_res:
static void sum_tiles(mpmc_hip_ctx *c, const TileSum &ts, int nparts, ResSlot slot, hipStream_t sb) {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(kReduceThreads), 0, sb, ts.part, nparts, 1, c->d_res + slot);
}

// The pass of a sum over positions, behind the pair kernel: same stream, same dirty blocks, same move.  enqueue(sel)
// launches the term's kernel over the tiles of the blocks in sel (sel.n == 0: all of them).
template <typename Enqueue>
static int tile_pass(mpmc_hip_ctx *c, TileSum &ts, int nparts, ResSlot slot, hipStream_t sb, Enqueue &&enqueue) {
    DirtyBlocks sel = c->call.dirty_blocks;
    if (!ts.valid) sel.n = 0;
    if (ts.valid && c->dirty_atoms.empty()) return 0;  // nothing moved: d_res[slot] is still that sum
    ScopedTimer t(c, T_PAIR, sb);
    enqueue(sel);
    sum_tiles(c, ts, nparts, slot, sb);
    HIPCHK(hipGetLastError());
    ts.valid = true;
    return 0;
}

// A static sum (parameters, cutoff, volume and which atoms exist: no coordinate), made again when it is stale.  enqueue()
// launches its kernels; nparts == 0: they left no tile partials to add up.
template <typename Enqueue>
static int static_pass(mpmc_hip_ctx *c, TileSum &ts, bool stale, int nparts, ResSlot slot, hipStream_t sb, Enqueue &&enqueue) {
    if (!stale) return 0;
    ScopedTimer t(c, T_OTHER, sb);
    enqueue();
    if (nparts > 0) sum_tiles(c, ts, nparts, slot, sb);
    HIPCHK(hipGetLastError());
    ts.valid = true;
    return 0;
}

// A mode's long-range correction, a static sum that exists only while `wanted` (rd_lrc): otherwise the publish kernel writes
// its slot as zero, and the sum is dropped so that switching rd_lrc back on makes it again.
template <typename Enqueue>
static int lrc_pass(mpmc_hip_ctx *c, TileSum &ts, bool wanted, bool stale, int nparts, ResSlot slot, hipStream_t sb,
                    Enqueue &&enqueue) {
    if (wanted) return static_pass(c, ts, stale, nparts, slot, sb, enqueue);
    c->call.res_zero_mask |= 1u << slot;
    ts.valid = false;
    return 0;
}

// Which tiles the pass of a static sum redoes after insertions / removals: sel = the blocks of lrc_dirty_atoms, or all of
// them (sel.n == 0) when the sum has to be made from scratch (`scratch`: it is not valid, or the list held more blocks than
// a selection does).  Returns "stale": the sum is not that of the atoms that exist now.
static bool lrc_selection(const mpmc_hip_ctx *c, bool scratch, DirtyBlocks &sel) {
    sel = c->call.lrc_blocks;  // (n = 0 after an overflow)
    if (scratch) sel.n = 0;
    return scratch || c->call.lrc_edited;
}

// disp_expansion: the dense pair sum, and its long-range correction when the parameters, the cutoff or the volume changed.
static int launch_disp(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, hipStream_t sb) {
    const int ntile = c->npad / 64;
    const DispAtoms da = {c->d_eps, c->d_sig, c->d_c6, c->d_c8, c->d_c10};
    DirtyBlocks lsel;
    const bool stale = lrc_selection(c, !c->disp_lrc.valid, lsel);
    if (lrc_pass(c, c->disp_lrc, c->par.rd_lrc, stale, ntile * ntile, R_DISP_LRC, sb, [&] {
            hipLaunchKernelGGL(disp_lrc_kernel, dim3(ntile, lsel.n > 0 ? lsel.n : ntile), dim3(64 * kDispLrcWaves), 0, sb, a, da,
                               bx, c->disp_par, lsel, c->disp_lrc.part);
        }))
        return -1;
    return tile_pass(c, c->disp, ntile * ntile, R_DISP, sb, [&](const DirtyBlocks &sel) {
        hipLaunchKernelGGL(disp_tile_kernel, dim3(ntile, sel.n > 0 ? sel.n : ntile), dim3(64 * kDispWaves), 0, sb, a, da, bx,
                           c->disp_par, sel, c->disp.part, c->call.pair_moves);
    });
}

// rd_crystal: cutoff_c and the squared-distance threshold that decides exactly as `sqrt(r2) > cutoff_c` does
static RdcParams rdc_params(const mpmc_hip_ctx *c) {
    RdcParams rp;
    rp.order = c->rdc_order;
    rp.fh_order = c->par.feynman_hibbs ? c->par.feynman_hibbs_order : 0;
    rp.temperature = c->par.temperature;
    rp.cutoff_c = 2.0 * c->cutoff * ((double)c->rdc_order - 0.5);  // lj.c:176
    double x = rp.cutoff_c * rp.cutoff_c;
    while (std::sqrt(x) > rp.cutoff_c) x = std::nextafter(x, 0.0);
    while (std::sqrt(std::nextafter(x, INFINITY)) <= rp.cutoff_c) x = std::nextafter(x, INFINITY);
    rp.r2max = x;
    return rp;
}

// rd_crystal: the image sum; the self part and the long-range correction at cutoff_c when the parameters, the box or rd_lrc
// changed.  `a` carries zero epsilon / sigma in this mode: these kernels get the real ones.
static int launch_rdc(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, hipStream_t sb) {
    const int ntile = c->npad / 64;
    const DevAtoms lj = lj_atoms(c, a);
    const RdcParams rp = rdc_params(c);
    const int want_lrc = c->par.rd_lrc ? 1 : 0;
    // (after an edit the self part, a sum over the atoms that exist, is made again whole; the correction by edited blocks)
    DirtyBlocks lsel;
    const bool stale = lrc_selection(c, !c->rdc_static.valid || c->rdc_static_lrc != want_lrc, lsel);
    if (static_pass(c, c->rdc_static, stale, want_lrc ? ntile * ntile : 0, R_DISP_LRC, sb, [&] {
            hipLaunchKernelGGL(rdc_self_kernel, dim3(1), dim3(kRdcSelfThreads), 0, sb, lj, bx, rp, c->d_res + R_RDC_SELF);
            if (!want_lrc) return;
            DevBox bc = bx;
            bc.cutoff = rp.cutoff_c;  // lj_lrc_corr / lj_lrc_self at the crystal cutoff (lj.c:188, :273)
            hipLaunchKernelGGL(lj_lrc_kernel, dim3(ntile, lsel.n > 0 ? lsel.n : ntile), dim3(64 * kLrcWaves), 0, sb, lj, bc, lsel,
                               c->rdc_static.part);
        }))
        return -1;
    c->rdc_static_lrc = want_lrc;
    if (!want_lrc) c->call.res_zero_mask |= 1u << R_DISP_LRC;
    return tile_pass(c, c->rdc, ntile * ntile, R_DISP, sb, [&](const DirtyBlocks &sel) {
        hipLaunchKernelGGL(rdc_tile_kernel, dim3(ntile, sel.n > 0 ? sel.n : ntile), dim3(64 * kRdcWaves), 0, sb, lj, bx, rp, sel,
                           c->rdc.part, c->call.pair_moves);
    });
}

// set_rd_form: the dense pair sum of the form, and under rd_lrc the LJ form's long-range correction when the parameters,
// the mixing, the cutoff or the volume changed.  `a` carries zero epsilon / sigma in this mode: these kernels get the real
// ones.
static int launch_rdform(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, hipStream_t sb) {
    const int ntile = c->npad / 64;
    const DevAtoms lj = lj_atoms(c, a);
    RdFormParams fp;
    fp.mixing = c->rd_mix;
    fp.fh = c->par.feynman_hibbs ? 1 : 0;
    fp.fh_order = c->par.feynman_hibbs_order;
    fp.temperature = c->par.temperature;
    DirtyBlocks lsel;
    const bool stale = lrc_selection(c, !c->rdf_lrc.valid, lsel);
    if (lrc_pass(c, c->rdf_lrc, c->rd_form == kRdFormLJ && c->par.rd_lrc, stale, ntile * ntile, R_DISP_LRC, sb, [&] {
            hipLaunchKernelGGL(rdform_lrc_kernel, dim3(ntile, lsel.n > 0 ? lsel.n : ntile), dim3(64 * kRdFormLrcWaves), 0, sb, lj,
                               bx, c->rd_mix, lsel, c->rdf_lrc.part);
        }))
        return -1;
    return tile_pass(c, c->rdf, ntile * ntile, R_DISP, sb, [&](const DirtyBlocks &sel) {
        const dim3 grid(ntile, sel.n > 0 ? sel.n : ntile), block(64 * kRdFormWaves);
        double *part = c->rdf.part;
        const MoveList &mv = c->call.pair_moves;
        switch (c->rd_form) {
        case kRdFormLJ: hipLaunchKernelGGL(rdform_tile_kernel<kRdFormLJ>, grid, block, 0, sb, lj, bx, fp, sel, part, mv); break;
        case kRdFormSG: hipLaunchKernelGGL(rdform_tile_kernel<kRdFormSG>, grid, block, 0, sb, lj, bx, fp, sel, part, mv); break;
        case kRdFormDreiding:
            hipLaunchKernelGGL(rdform_tile_kernel<kRdFormDreiding>, grid, block, 0, sb, lj, bx, fp, sel, part, mv);
            break;
        default:
            hipLaunchKernelGGL(rdform_tile_kernel<kRdFormBuffered147>, grid, block, 0, sb, lj, bx, fp, sel, part, mv);
            break;
        }
    });
}

// axilrod_teller: the block-triple sum (behind the pair and the dispersion launch); the order of the sum over all its
// partials is a function of the block count only.
static int launch_at(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, hipStream_t sb) {
    const int ntile = c->npad / 64;
    const AtAtoms ta = {c->d_at_a, c->d_at_g};
    const long units = at_unit_count(ntile);
    return tile_pass(c, c->at, (int)(units * kAtSplit), R_AT, sb, [&](const DirtyBlocks &sel) {
        const dim3 grid = sel.n > 0 ? dim3((unsigned)(ntile * (ntile + 1) / 2 * kAtSplit), (unsigned)sel.n)
                                    : dim3((unsigned)(units * kAtSplit));
        hipLaunchKernelGGL(at_triple_kernel, grid, dim3(64 * kAtWaves), 0, sb, a, ta, bx, sel, ntile, c->at.part,
                           c->call.pair_moves);
    });
}

// polarvdw: au2invsec * halfHBAR * sum sqrt(max(lambda, 0)) of the matrix C of `na` sites (the run [first, first + na) of
// the site list) -> out[0].  Build, 3 (n - 2) + 1 launches of the Householder reduction, bisection, sum: plain launches on
// one stream, every trip count known here (kernels_vdw.h).
static int vdw_eigen_sum(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, int first, int na, const MoveList &mv,
                         double *out, hipStream_t sb) {
    if (na <= 0) {  // a matrix of dimension 0: no eigenvalue (lapack_diag returns NULL, vdw.c:169)
        HIPCHK(hipMemsetAsync(out, 0, sizeof(double), sb));
        return 0;
    }
    const int n = 3 * na, ld = n;
    const size_t nc = 3 * (size_t)std::max(c->vdw_na, 1);
    double *C = c->d_vdw_C, *v = c->d_vdw_vec, *p = v + nc, *d = p + nc, *e = d + nc, *lam = e + nc, *scal = lam + nc;
    const VdwSites s = {c->d_vdw_idx + first, c->d_vdw_k + first, na};
    hipLaunchKernelGGL(vdw_build_kernel, dim3((na + 63) / 64, na), dim3(64), 0, sb, a, bx, c->par.polar_damp, s, C, ld, mv);
    for (int j = 0; j < n - 2; ++j) {
        const int mm = n - j - 1;
        hipLaunchKernelGGL(vdw_reflect_kernel, dim3(1), dim3(kVdwReflectThreads), 0, sb, C, ld, n, j, v, scal, d, e);
        hipLaunchKernelGGL(vdw_symv_kernel, dim3((mm + kVdwSymvWaves - 1) / kVdwSymvWaves), dim3(64 * kVdwSymvWaves), 0, sb, C, ld,
                           n, j, v, scal, p);
        hipLaunchKernelGGL(vdw_rank2_kernel, dim3((mm + kVdwUpdRows - 1) / kVdwUpdRows), dim3(64 * kVdwUpdWaves), 0, sb, C, ld, n,
                           j, v, p, scal);
    }
    hipLaunchKernelGGL(vdw_reflect_kernel, dim3(1), dim3(kVdwReflectThreads), 0, sb, C, ld, n, n - 2, v, scal, d, e);
    hipLaunchKernelGGL(vdw_bisect_kernel, dim3((n + 63) / 64), dim3(64), 0, sb, d, e, n, lam);
    hipLaunchKernelGGL(vdw_sum_kernel, dim3(1), dim3(kVdwSumThreads), 0, sb, lam, d, e, n, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// polarvdw: e_iso of every molecule type that has none yet, from the first molecule of the type in this upload
// (calc_e_iso, vdw.c:225-259), then the sum over the molecules in upload order (sum_eiso_vdw).  Runs on the main stream in
// front of the evaluation and waits for it: once per type for as long as the mode stays on.
static int vdw_ensure_iso(mpmc_hip_ctx *c) {
    if (c->vdw_iso_summed) return 0;
    const DevAtoms a = dev_atoms(c);
    const DevBox bx = dev_box(c);
    const size_t nc = 3 * (size_t)std::max(c->vdw_na, 1);
    double *slot = c->d_vdw_vec + 5 * nc + 1;
    for (const auto &m : c->vdw_mols) {
        if (c->vdw_iso.count(m.type)) continue;
        double v = 0.0;
        if (vdw_eigen_sum(c, a, bx, m.first_site, m.sites, c->pending, slot, c->stream)) return -1;
        HIPCHK(hipMemcpyAsync(&v, slot, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->vdw_iso[m.type] = v;
    }
    double s = 0.0;
    for (const auto &m : c->vdw_mols) s += c->vdw_iso[m.type];
    c->vdw_e_iso = s;
    c->vdw_iso_summed = true;
    return 0;
}

// polarvdw: the repulsion-only pair sum and its long-range correction (R_DISP, R_DISP_LRC), then lr_corr and the
// eigenvalue sum of the whole configuration behind them on the same stream.  `a` carries zero epsilon / sigma in this
// mode: the repulsion kernels get the real ones.
static int launch_vdw(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, hipStream_t sb) {
    const int ntile = c->npad / 64;
    const DevAtoms lj = lj_atoms(c, a);
    const DirtyBlocks all = {};
    if (lrc_pass(c, c->rep_lrc, c->par.rd_lrc, !c->rep_lrc.valid, ntile * ntile, R_DISP_LRC, sb, [&] {
            hipLaunchKernelGGL(rep_lrc_kernel, dim3(ntile, ntile), dim3(64 * kVdwLrcWaves), 0, sb, lj, bx, all, c->rep_lrc.part);
        }))
        return -1;
    if (tile_pass(c, c->rep, ntile * ntile, R_DISP, sb, [&](const DirtyBlocks &sel) {
            hipLaunchKernelGGL(rep_tile_kernel, dim3(ntile, sel.n > 0 ? sel.n : ntile), dim3(64 * kRepWaves), 0, sb, lj, bx, sel,
                               c->rep.part, c->call.pair_moves);
        }))
        return -1;
    if (c->par.rd_only) {  // vdw() is not called under rd_only (energy.c:149-177)
        c->call.res_zero_mask |= (1u << R_VDW) | (1u << R_VDW_LRC);
        c->vdw.valid = c->vdw_lrc.valid = false;
        return 0;
    }
    if (lrc_pass(c, c->vdw_lrc, c->par.rd_lrc, !c->vdw_lrc.valid, ntile * ntile, R_VDW_LRC, sb, [&] {
            hipLaunchKernelGGL(vdw_lrc_kernel, dim3(ntile, ntile), dim3(64 * kVdwLrcWaves), 0, sb, a, (const double *)c->d_vdw_w,
                               bx, all, c->vdw_lrc.part);
        }))
        return -1;
    if (c->vdw.valid && c->dirty_atoms.empty()) return 0;  // nothing moved: d_res[R_VDW] is still that sum
    ScopedTimer t(c, T_OTHER, sb);
    if (vdw_eigen_sum(c, a, bx, 0, c->vdw_na, c->call.pair_moves, c->d_res + R_VDW, sb)) return -1;
    c->vdw.valid = true;
    return 0;
}
