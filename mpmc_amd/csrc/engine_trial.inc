// engine_trial.inc -- host side of mpmc_hip_trial_energies() (kernels_trial.h, DESIGN.md section 19): the total energy of
// the resident configuration with ONE molecule at each of K trial placements.  Included by engine.hip.
// Two paths.  The batched one (the standard pair path without polarization) reads the resident coordinates, parameters and
// block partial structure factors, writes only the d_trial_* buffers, and leaves every cached sum, the last record and
// any pending sweep as they were.  The serial one (everything else, or option "trial_batched" 0) is the public
// update_atoms() + energy() sequence, trial after trial, then the original coordinates and one more energy().

// what the last completed energy() evaluated is still what is resident: no upload, move, edit, box, parameter or option
// change since (every one of them bumps config_rev or leaves a dirty atom)
static bool trial_result_current(const mpmc_hip_ctx *c) {
    return c->result_valid && c->result_rev == c->config_rev && !c->all_dirty && c->dirty_atoms.empty() &&
           c->pending.n == 0 && c->lrc_dirty_atoms.empty();
}

static bool trial_batched_mode(const mpmc_hip_ctx *c) {
    const bool do_polar = !c->par.rd_only && c->par.polarization;
    return c->trial_batched && !do_polar && !c->disp_on && !c->rdc_order && !c->vdw_on && !c->rd_form && !c->at_on;
}

template <typename T>
static hipError_t trial_grow(DevBuf<T> &b, size_t count) {
    if (b.size() >= count) return hipSuccess;
    return b.alloc(count + count / 4);
}

// [first, first + count) is one whole valid, non-frozen molecule: read from the device's own molecule ids and flags
static int trial_check_molecule(mpmc_hip_ctx *c, int first, int count) {
    const char *bad = "MPMC_HIP: trial_energies: slots [%d, %d) are not one whole valid, non-frozen molecule of 1 .. %d sites (%s)";
    if (count < 1 || count > kTrialSites) return fail(bad, first, first + count, kTrialSites, "site count");
    if (first < 0 || first > c->n - count) return fail(bad, first, first + count, kTrialSites, "outside the slots in use");
    const int lo = std::max(first - 1, 0), hi = std::min(first + count + 1, c->n);
    int mol[kTrialSites + 2], fl[kTrialSites + 2];
    HIPCHK(hipMemcpyAsync(mol, c->d_mol + lo, (size_t)(hi - lo) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(fl, c->d_flags + lo, (size_t)(hi - lo) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int id = mol[first - lo];
    for (int i = first; i < first + count; ++i) {
        if (!(fl[i - lo] & kValid)) return fail(bad, first, first + count, kTrialSites, "a slot holds no atom");
        if (mol[i - lo] != id) return fail(bad, first, first + count, kTrialSites, "more than one molecule");
        if (fl[i - lo] & kFrozen) return fail(bad, first, first + count, kTrialSites, "frozen");
    }
    if (lo < first && (fl[0] & kValid) && mol[0] == id)
        return fail(bad, first, first + count, kTrialSites, "the molecule starts earlier");
    if (hi > first + count && (fl[hi - 1 - lo] & kValid) && mol[hi - 1 - lo] == id)
        return fail(bad, first, first + count, kTrialSites, "the molecule goes on");
    return 0;
}

static int trial_serial(mpmc_hip_ctx *c, int first, int count, int ntrial, const double *xyz, double *energy) {
    double ox[kTrialSites], oy[kTrialSites], oz[kTrialSites];
    const size_t b = (size_t)count * sizeof(double);
    HIPCHK(hipMemcpyAsync(ox, c->d_x + first, b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(oy, c->d_y + first, b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(oz, c->d_z + first, b, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = 0;
    std::string err;
    mpmc_hip_result r;
    for (int t = 0; t < ntrial && !rc; ++t) {
        double x[kTrialSites], y[kTrialSites], z[kTrialSites];
        for (int s = 0; s < count; ++s) {
            const double *p = xyz + ((size_t)t * count + s) * 3;
            x[s] = p[0];
            y[s] = p[1];
            z[s] = p[2];
        }
        rc = mpmc_hip_update_atoms(c, first, count, x, y, z);
        if (!rc) rc = mpmc_hip_energy(c, &r);
        if (!rc) energy[t] = r.energy;
    }
    if (rc) err = g_err;
    // back to the configuration the caller has, whatever happened
    int rc2 = mpmc_hip_update_atoms(c, first, count, ox, oy, oz);
    if (!rc2) rc2 = mpmc_hip_energy(c, &r);
    if (rc) g_err = err;
    return (rc || rc2) ? -1 : 0;
}

static int trial_batched(mpmc_hip_ctx *c, int first, int count, int ntrial, const double *xyz, double *energy,
                         double *terms) {
    const mpmc_hip_params &P = c->par;
    const bool ewald = !P.rd_only && !P.wolf && c->nk > 0;
    if (ewald && (!c->recip_part_valid || !c->d_sfpart || !c->kvec_valid))
        return fail("MPMC_HIP: trial_energies: internal: no resident structure factors");
    const size_t nt = (size_t)ntrial, nb = nt + 1;
    const int nchunk = ewald ? (c->nk + 63) / 64 : 0;
    HIPCHK(hipStreamSynchronize(c->stream));  // (an earlier call's kernels may still read the buffers grown below)
    HIPCHK(trial_grow(c->d_trial_xyz, nt * count * 3));
    HIPCHK(trial_grow(c->d_trial_pair, nb * 2));
    HIPCHK(trial_grow(c->d_trial_out, nt * 4));
    if (ewald) {
        HIPCHK(trial_grow(c->d_trial_chunk, nb * nchunk));
        HIPCHK(trial_grow(c->d_trial_srest, (size_t)c->nk));
    }
    HIPCHK(hipMemcpyAsync(c->d_trial_xyz, xyz, nt * count * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const DevAtoms a = dev_atoms(c);
    const DevBox bx = dev_box(c);
    PairParams pp;  // as launch_pair_kernel() fills it
    pp.ewald_alpha = c->ewald_alpha;
    pp.temperature = P.temperature;
    pp.rd_only = P.rd_only;
    pp.fh_order = P.feynman_hibbs ? P.feynman_hibbs_order : 0;
    pp.wolf = P.wolf;
    pp.erfaRoverR = std::erf(c->ewald_alpha * c->cutoff) / c->cutoff;
    TrialMol tm = {first, count, c->d_trial_xyz.get()};
    const dim3 grid((unsigned)nb), block(64 * kTrialWaves);
    if (pp.fh_order == 0)
        hipLaunchKernelGGL(trial_pair_kernel<0>, grid, block, 0, c->stream, a, bx, pp, tm, c->d_trial_pair.get());
    else if (pp.fh_order == 2)
        hipLaunchKernelGGL(trial_pair_kernel<2>, grid, block, 0, c->stream, a, bx, pp, tm, c->d_trial_pair.get());
    else
        hipLaunchKernelGGL(trial_pair_kernel<4>, grid, block, 0, c->stream, a, bx, pp, tm, c->d_trial_pair.get());
    if (ewald) {
        hipLaunchKernelGGL(trial_recip_prepare_kernel, dim3(nchunk), dim3(64 * kTrialPrepGroups), 0, c->stream, a,
                           (const KVec *)c->d_kvec, c->nk, c->npad / 64, (const double2 *)c->d_sfpart, tm,
                           c->d_trial_srest.get());
        hipLaunchKernelGGL(trial_recip_kernel, dim3(nchunk, (unsigned)nb), dim3(64), 0, c->stream, a, (const KVec *)c->d_kvec,
                           c->nk, (const double2 *)c->d_trial_srest, tm, c->d_trial_chunk.get());
    }
    double *d_e = c->d_trial_out.get(), *d_t = d_e + nt;
    hipLaunchKernelGGL(trial_assemble_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream,
                       (const double *)c->d_trial_pair, (const double *)c->d_trial_chunk, nchunk, ntrial,
                       c->last_result.energy, 4.0 * kPI / c->volume, d_e, d_t);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(energy, d_e, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (terms) HIPCHK(hipMemcpyAsync(terms, d_t, 3 * nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mpmc_hip_trial_energies(mpmc_hip_ctx *c, int first_slot, int count, int ntrial, const double *xyz,
                                       double *energy, double *terms) {
    if (!c) return fail("MPMC_HIP: trial_energies: null context");
    if (c->in_flight) return fail("MPMC_HIP: trial_energies between energy_begin() and energy_end()");
    if (ntrial < 1) return fail("MPMC_HIP: trial_energies: ntrial = %d (at least 1)", ntrial);
    if (!xyz || !energy) return fail("MPMC_HIP: trial_energies: null argument");
    if (!c->have_atoms || !trial_result_current(c))
        return fail("MPMC_HIP: trial_energies needs a completed energy() on the current configuration (an upload, move, "
                    "edit, box or parameter change came after the last one)");
    HIPCHK(hipSetDevice(c->device));
    if (trial_check_molecule(c, first_slot, count)) return -1;
    const bool batched = trial_batched_mode(c);
    if (terms && !batched)
        return fail("MPMC_HIP: trial_energies: terms are the batched path's (no polarization, no dense mode, option "
                    "trial_batched 1)");
    ++c->trial_calls;
    if (batched) return trial_batched(c, first_slot, count, ntrial, xyz, energy, terms);
    return trial_serial(c, first_slot, count, ntrial, xyz, energy);
}

extern "C" long long mpmc_hip_trial_call_count(mpmc_hip_ctx *c) { return c ? (long long)c->trial_calls : 0; }
