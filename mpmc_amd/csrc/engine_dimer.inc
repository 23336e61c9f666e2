// engine_dimer.inc -- host side of the dimer scans (kernels_dimer.h): mpmc_hip_dimer_energies() and
// mpmc_hip_dimer_grid_means().  Included by engine.hip.  Nothing here reads or writes the resident configuration, its
// caches or the last result; the context gives its device, its main stream and the d_dimer_* buffers.

// molecule_rotate_euler() (surface.c:116-125), or under surf_global_axis the matrix of molecule_rotate_quaternion()'s
// `total` (surface.c:177-193, quaternion.c:45-83): R p = total p total*, expanded for a quaternion of any norm.
static void dimer_rotation(int global_axis, double alpha, double beta, double gamma, double R[9]) {
    if (!global_axis) {
        R[0] = cos(gamma) * cos(beta) * cos(alpha) - sin(gamma) * sin(alpha);
        R[1] = sin(gamma) * cos(beta) * cos(alpha) + cos(gamma) * sin(alpha);
        R[2] = -sin(beta) * cos(alpha);
        R[3] = -cos(gamma) * cos(beta) * sin(alpha) - sin(gamma) * cos(alpha);
        R[4] = -sin(gamma) * cos(beta) * sin(alpha) + cos(gamma) * cos(alpha);
        R[5] = sin(beta) * sin(alpha);
        R[6] = cos(gamma) * sin(beta);
        R[7] = sin(gamma) * sin(beta);
        R[8] = cos(beta);
        return;
    }
    struct Q {
        double x, y, z, w;
    };
    auto axis = [](double x, double y, double z, double angle) {  // quaternion_construct_axis_angle_degree()
        angle /= 57.2957795;
        const double s = sin(angle / 2);
        return Q{x * s, y * s, z * s, cos(angle / 2)};
    };
    auto mul = [](const Q &a, const Q &b) {  // quaternion_multiplication()
        return Q{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
                 a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
    };
    Q t{0., 0., 0., 1.};
    t = mul(axis(0., 0., 1., alpha), t);
    t = mul(axis(0., 1., 0., beta), t);
    t = mul(axis(1., 0., 0., gamma), t);  // (about x: kept as the reference has it)
    const double xx = t.x * t.x, yy = t.y * t.y, zz = t.z * t.z, ww = t.w * t.w;
    R[0] = ww + xx - yy - zz;
    R[1] = 2.0 * (t.x * t.y - t.w * t.z);
    R[2] = 2.0 * (t.x * t.z + t.w * t.y);
    R[3] = 2.0 * (t.x * t.y + t.w * t.z);
    R[4] = ww - xx + yy - zz;
    R[5] = 2.0 * (t.y * t.z - t.w * t.x);
    R[6] = 2.0 * (t.x * t.z - t.w * t.y);
    R[7] = 2.0 * (t.y * t.z + t.w * t.x);
    R[8] = ww - xx - yy + zz;
}

extern "C" void mpmc_hip_default_dimer_params(mpmc_hip_dimer_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->damp_type = 2;
    p->polar_max_iter = 10;
    p->polar_gamma = 1.0;
}

// body frame and parameters of one molecule (update_com(), pairs.c:364-385: the mass-weighted centre, summed in site order)
static int dimer_fill_molecule(const char *what, const char *which, const mpmc_hip_molecule *m, bool disp, DimerMol &out,
                               bool &polarizable) {
    memset(&out, 0, sizeof(out));
    if (!m) return fail("MPMC_HIP: %s: null molecule %s", what, which);
    if (m->count < 1 || m->count > kDimerMolSites)
        return fail("MPMC_HIP: %s: molecule %s has %d sites (1 .. %d)", what, which, m->count, kDimerMolSites);
    if (!m->x || !m->y || !m->z || !m->charge || !m->polarizability || !m->epsilon || !m->sigma || !m->mass)
        return fail("MPMC_HIP: %s: molecule %s: null array", what, which);
    if (disp && (!m->c6 || !m->c8 || !m->c10))
        return fail("MPMC_HIP: %s: molecule %s: disp_expansion reads c6 / c8 / c10", what, which);
    double mass = 0.0, com[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < m->count; ++s) {
        mass += m->mass[s];
        com[0] += m->mass[s] * m->x[s];
        com[1] += m->mass[s] * m->y[s];
        com[2] += m->mass[s] * m->z[s];
    }
    for (int p = 0; p < 3; ++p) com[p] /= mass;
    if (!std::isfinite(com[0]) || !std::isfinite(com[1]) || !std::isfinite(com[2]))
        return fail("MPMC_HIP: %s: molecule %s has no centre of mass (total mass %g)", what, which, mass);
    out.n = m->count;
    for (int s = 0; s < m->count; ++s) {
        out.bx[s] = m->x[s] - com[0];
        out.by[s] = m->y[s] - com[1];
        out.bz[s] = m->z[s] - com[2];
        out.q[s] = m->charge[s];
        out.alpha[s] = m->polarizability[s];
        out.eps[s] = m->epsilon[s];
        out.sig[s] = m->sigma[s];
        if (disp) {
            out.c6[s] = m->c6[s];
            out.c8[s] = m->c8[s];
            out.c10[s] = m->c10[s];
        }
        if (m->polarizability[s] < 0.0) return fail("MPMC_HIP: %s: molecule %s: negative polarizability", what, which);
        if (m->polarizability[s] != 0.0) polarizable = true;
    }
    return 0;
}

struct DimerSetup {
    DimerParams P;
    TholeParams tp;
    int model;
};

// checks shared by both entries; uploads the molecules
static int dimer_prepare(mpmc_hip_ctx *c, const char *what, const mpmc_hip_dimer_params *p, const mpmc_hip_molecule *a,
                         const mpmc_hip_molecule *b, DimerSetup &su) {
    if (!c) return fail("MPMC_HIP: %s: null context", what);
    if (c->in_flight) return fail("MPMC_HIP: %s between energy_begin() and energy_end()", what);
    if (!p) return fail("MPMC_HIP: %s: null parameters", what);
    if (p->rd_form != 0 && p->rd_form != MPMC_HIP_RD_LJ)
        return fail("MPMC_HIP: %s: rd_form %d is not supported (Lennard-Jones or disp_expansion)", what, p->rd_form);
    if (p->mixing < MPMC_HIP_RD_MIX_LB || p->mixing > MPMC_HIP_RD_MIX_C6)
        return fail("MPMC_HIP: %s: unknown mixing rule %d", what, p->mixing);
    if (p->disp_expansion && p->mixing != MPMC_HIP_RD_MIX_LB)
        return fail("MPMC_HIP: %s: a Lennard-Jones mixing rule together with disp_expansion", what);
    if (p->damp_type < 0 || p->damp_type > 2) return fail("MPMC_HIP: %s: damp_type %d (0, 1 or 2)", what, p->damp_type);
    DimerMols hm;
    bool polarizable = false;
    if (dimer_fill_molecule(what, "a", a, p->disp_expansion != 0, hm.m[0], polarizable)) return -1;
    if (dimer_fill_molecule(what, "b", b, p->disp_expansion != 0, hm.m[1], polarizable)) return -1;
    if (p->mixing == MPMC_HIP_RD_MIX_WALDMAN_HAGLER) {
        for (int w = 0; w < 2; ++w)
            for (int s = 0; s < hm.m[w].n; ++s)
                if (hm.m[w].sig[s] < 0.0)
                    return fail("MPMC_HIP: %s: waldmanhagler with a negative sigma (the reference never assigns such a pair's epsilon)", what);
    }
    memset(&su, 0, sizeof(su));
    DimerParams &P = su.P;
    P.disp = p->disp_expansion != 0;
    P.mixing = p->mixing;
    P.dp.damp = p->damp_dispersion != 0;
    P.dp.extrapolate = p->extrapolate_disp_coeffs != 0;
    P.dp.schmidt = p->schmidt_mixing != 0;
    P.rd_only = p->rd_only != 0;
    P.polar = polarizable && !P.rd_only;
    P.max_iter = p->polar_max_iter;
    P.precision = p->polar_precision;
    P.gs = (p->polar_gs || p->polar_gs_ranked) ? 1 : 0;
    P.ranked = p->polar_gs_ranked != 0;
    P.palmo = p->polar_palmo != 0;
    P.gamma = p->polar_gamma;
    if (P.polar) {
        if (!(p->polar_precision >= 0.0) || !std::isfinite(p->polar_precision))
            return fail("MPMC_HIP: %s: polar_precision %g", what, p->polar_precision);
        if (p->polar_precision > 0.0 ? p->polar_max_iter != 0 : p->polar_max_iter < 1)
            return fail("MPMC_HIP: %s: polar_max_iter %d (at least 1, or 0 together with polar_precision > 0)", what,
                        p->polar_max_iter);
        if (p->damp_type != 0 && !(p->polar_damp > 0.0))
            return fail("MPMC_HIP: %s: polar_damp %g must be positive with this damp_type", what, p->polar_damp);
        if (!std::isfinite(p->polar_gamma)) return fail("MPMC_HIP: %s: polar_gamma %g", what, p->polar_gamma);
    }
    su.model = p->damp_type == 2 ? kTholeExp : (p->damp_type == 1 ? kTholeLinear : kTholeOff);
    su.tp.damp = p->polar_damp;
    su.tp.rc = kMAXVALUE;
    su.tp.idx = nullptr;

    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));  // (an earlier dimer call's kernels may still read the buffers reused below)
    if (!c->d_dimer_mols) HIPCHK(c->d_dimer_mols.alloc(sizeof(DimerMols)));
    if (!c->d_dimer_means) HIPCHK(c->d_dimer_means.alloc(4));
    HIPCHK(hipMemcpyAsync(c->d_dimer_mols, &hm, sizeof(hm), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (hm is on this stack frame)
    return 0;
}

template <typename T>
static hipError_t dimer_grow(DevBuf<T> &b, size_t count) {
    if (b.size() >= count) return hipSuccess;
    return b.alloc(count + count / 4);
}

// the two tables: K[w] rotations per molecule from R[w]; rlist: separations per entry (list form) or nullptr
static int dimer_tables(mpmc_hip_ctx *c, const int K[2], const std::vector<double> R[2], const double *rlist, double r) {
    for (int w = 0; w < 2; ++w) {
        HIPCHK(dimer_grow(c->d_dimer_rot[w], 9 * (size_t)K[w]));
        HIPCHK(dimer_grow(c->d_dimer_tab[w], kDimerTabStride * (size_t)K[w]));
        HIPCHK(hipMemcpyAsync(c->d_dimer_rot[w], R[w].data(), 9 * (size_t)K[w] * sizeof(double), hipMemcpyHostToDevice,
                              c->stream));
    }
    const double *d_r = nullptr;
    if (rlist) {
        HIPCHK(dimer_grow(c->d_dimer_r, (size_t)K[1]));
        HIPCHK(hipMemcpyAsync(c->d_dimer_r, rlist, (size_t)K[1] * sizeof(double), hipMemcpyHostToDevice, c->stream));
        d_r = c->d_dimer_r;
    }
    for (int w = 0; w < 2; ++w) {
        const long long threads = (long long)K[w] * kDimerMolSites;
        hipLaunchKernelGGL(dimer_rotate_kernel, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, c->stream,
                           (const DimerMols *)c->d_dimer_mols.get(), w, K[w], (const double *)c->d_dimer_rot[w], d_r, r,
                           c->d_dimer_tab[w].get());
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int dimer_launch(mpmc_hip_ctx *c, const DimerSetup &su, const DimerLaunch &L, long long nchunk) {
    const DimerMols *dm = (const DimerMols *)c->d_dimer_mols.get();
    const dim3 grid((unsigned)nchunk), block(64);
    if (su.model == kTholeExp)
        hipLaunchKernelGGL(dimer_energy_kernel<kTholeExp>, grid, block, 0, c->stream, dm, su.P, su.tp, L);
    else if (su.model == kTholeLinear)
        hipLaunchKernelGGL(dimer_energy_kernel<kTholeLinear>, grid, block, 0, c->stream, dm, su.P, su.tp, L);
    else
        hipLaunchKernelGGL(dimer_energy_kernel<kTholeOff>, grid, block, 0, c->stream, dm, su.P, su.tp, L);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mpmc_hip_dimer_energies(mpmc_hip_ctx *c, const mpmc_hip_dimer_params *p, const mpmc_hip_molecule *a,
                                       const mpmc_hip_molecule *b, int nconf, const double *conf, double *es, double *rd,
                                       double *polar, int *status, double *mu) {
    const char *what = "dimer_energies";
    if (c && c->in_flight) return fail("MPMC_HIP: %s between energy_begin() and energy_end()", what);
    if (nconf < 0 || nconf > MPMC_HIP_DIMER_MAX_CONF)
        return fail("MPMC_HIP: %s: nconf = %d (0 .. %d)", what, nconf, MPMC_HIP_DIMER_MAX_CONF);
    if (nconf > 0 && (!conf || !es || !rd || !polar || !status)) return fail("MPMC_HIP: %s: null argument", what);
    DimerSetup su;
    if (dimer_prepare(c, what, p, a, b, su)) return -1;
    if (nconf == 0) return 0;
    const size_t n = (size_t)nconf;
    std::vector<double> R[2], rl(n);
    R[0].resize(9 * n);
    R[1].resize(9 * n);
    for (size_t k = 0; k < n; ++k) {
        const double *q = conf + 7 * k;
        rl[k] = q[0];
        dimer_rotation(p->global_axis, q[1], q[2], q[3], &R[0][9 * k]);
        dimer_rotation(p->global_axis, q[4], q[5], q[6], &R[1][9 * k]);
    }
    const int K[2] = {nconf, nconf};
    if (dimer_tables(c, K, R, rl.data(), 0.0)) return -1;
    HIPCHK(dimer_grow(c->d_dimer_out, 3 * n));
    HIPCHK(dimer_grow(c->d_dimer_status, n));
    if (mu) HIPCHK(dimer_grow(c->d_dimer_mu, 3 * kDimerSites * n));
    DimerLaunch L;
    memset(&L, 0, sizeof(L));
    L.tab1 = c->d_dimer_tab[0];
    L.tab2 = c->d_dimer_tab[1];
    L.K2 = 0;
    L.count = nconf;
    L.es = c->d_dimer_out.get();
    L.rd = L.es + n;
    L.polar = L.es + 2 * n;
    L.status = c->d_dimer_status.get();
    L.mu = mu ? c->d_dimer_mu.get() : nullptr;
    if (dimer_launch(c, su, L, ((long long)nconf + kDimerChunk - 1) / kDimerChunk)) return -1;
    HIPCHK(hipMemcpyAsync(es, L.es, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rd, L.rd, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(polar, L.polar, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, L.status, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (mu) HIPCHK(hipMemcpyAsync(mu, L.mu, 3 * kDimerSites * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mpmc_hip_dimer_grid_means(mpmc_hip_ctx *c, const mpmc_hip_dimer_params *p, const mpmc_hip_molecule *a,
                                         const mpmc_hip_molecule *b, double r, const int n[6],
                                         const double *const angles[6], double means[3], long long counts[2]) {
    const char *what = "dimer_grid_means";
    if (c && c->in_flight) return fail("MPMC_HIP: %s between energy_begin() and energy_end()", what);
    if (!n || !angles || !means || !counts) return fail("MPMC_HIP: %s: null argument", what);
    long long K[2] = {1, 1};
    for (int k = 0; k < 6; ++k) {
        if (n[k] < 1 || !angles[k]) return fail("MPMC_HIP: %s: angle list %d is empty", what, k);
        K[k / 3] *= n[k];
        if (K[k / 3] > MPMC_HIP_DIMER_MAX_CONF)
            return fail("MPMC_HIP: %s: more than %d rotations of one molecule", what, MPMC_HIP_DIMER_MAX_CONF);
    }
    const long long count = K[0] * K[1];
    const long long nchunk = (count + kDimerChunk - 1) / kDimerChunk;
    if (nchunk > (1ll << 30)) return fail("MPMC_HIP: %s: %lld placements are too many for one call", what, count);
    DimerSetup su;
    if (dimer_prepare(c, what, p, a, b, su)) return -1;
    std::vector<double> R[2];
    for (int w = 0; w < 2; ++w) {
        R[w].resize(9 * (size_t)K[w]);
        size_t k = 0;
        for (int ia = 0; ia < n[3 * w]; ++ia)
            for (int ib = 0; ib < n[3 * w + 1]; ++ib)
                for (int ig = 0; ig < n[3 * w + 2]; ++ig, ++k)
                    dimer_rotation(p->global_axis, angles[3 * w][ia], angles[3 * w + 1][ib], angles[3 * w + 2][ig],
                                   &R[w][9 * k]);
    }
    const int Ki[2] = {(int)K[0], (int)K[1]};
    if (dimer_tables(c, Ki, R, nullptr, r)) return -1;
    HIPCHK(dimer_grow(c->d_dimer_out, 3 * (size_t)nchunk));
    HIPCHK(dimer_grow(c->d_dimer_status, (size_t)nchunk));
    DimerLaunch L;
    memset(&L, 0, sizeof(L));
    L.tab1 = c->d_dimer_tab[0];
    L.tab2 = c->d_dimer_tab[1];
    L.K2 = Ki[1];
    L.count = count;
    L.partials = c->d_dimer_out.get();
    L.failed = c->d_dimer_status.get();
    if (dimer_launch(c, su, L, nchunk)) return -1;
    double *d_means = c->d_dimer_means.get();
    hipLaunchKernelGGL(dimer_mean_kernel, dim3(1), dim3(kDimerMeanThreads), 0, c->stream, (const double *)L.partials,
                       (const int *)L.failed, (int)nchunk, count, d_means, reinterpret_cast<long long *>(d_means + 3));
    HIPCHK(hipGetLastError());
    double h[4];
    HIPCHK(hipMemcpyAsync(h, d_means, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) means[k] = h[k];
    counts[0] = count;
    memcpy(&counts[1], &h[3], sizeof(long long));
    return 0;
}
