/*
 * qrot.c -- `quantum_rotation on`: the rotational levels of every movable molecule in the field of all others
 * (reference src/quantum_rotation/: rotational_eigenspectrum.c, rotational_potential.c, rotational_integrate.c,
 * rotational_basis.c; called from mc.c:253-256 and :304-308, single_point.c:15, replay.c:69).
 *
 * Per movable molecule: the potential V(theta, phi) on a 16 x 16 Gauss-Legendre grid, H_ij = <l_i m_i| V |l_j m_j> +
 * B l (l + 1) delta_ij in the Y_lm basis up to l_max <= 8, its eigenvalues (the levels) and eigenvectors, the g / u
 * symmetry of each level from random points of the run's generator, and the partition functions over the lowest
 * quantum_rotation_sum levels.
 *
 * What differs from the reference's evaluation, not from its definition:
 *   - the 256 energies of a molecule's grid are ONE mpmc_hip_trial_energies() call (the reference: 512 full energies),
 *     and the observables stay those of the configuration (the reference leaves the last grid orientation's behind);
 *   - Y_lm is tabulated on the grid once per l_max, from the standard recurrence of the associated Legendre functions
 *     (Condon-Shortley phase, sin(theta) taken with its sign: the functions of the reference's hard-coded table, which it
 *     evaluates 4 x 256 times per matrix element); every matrix element is still the reference's sum over the grid in
 *     its (p, t) order;
 *   - the eigen-solve is a cyclic Jacobi for the complex Hermitian matrix (the reference: LAPACK's zhpevx): eigenvectors
 *     of degenerate levels, and every eigenvector's phase, are the solver's;
 *   - determine_rotational_eigensymmetry() names a `system` that is not in its scope; its evident meaning,
 *     get_rand(system), is taken.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mpmc_host.h"

#define G QUANTUM_ROTATION_GRID
#define KB_SI 1.3806503e-23 /* defines.h:12 */
#define H_SI 6.626068e-34   /* defines.h:8 */
#define C_SI 2.99792458e8   /* defines.h:15 */

/* Gauss-Legendre abscissas and weights, N = 16 (Abramowitz & Stegun, p. 916) */
static const double roots[G] = {-0.989400934991649932596, -0.944575023073232576078, -0.865631202387831743880,
                                -0.755404408355003033895, -0.617876244402643748447, -0.458016777657227386342,
                                -0.281603550779258913230, -0.095012509837637440185, 0.095012509837637440185,
                                0.281603550779258913230,  0.458016777657227386342,  0.617876244402643748447,
                                0.755404408355003033895,  0.865631202387831743880,  0.944575023073232576078,
                                0.989400934991649932596};
static const double gl_weights[G] = {0.027152459411754094852, 0.062253523938647892863, 0.095158511682492784810,
                                     0.124628971255533872052, 0.149595988816576732081, 0.169156519395002538189,
                                     0.182603415044923588867, 0.189450610455068496285, 0.189450610455068496285,
                                     0.182603415044923588867, 0.169156519395002538189, 0.149595988816576732081,
                                     0.124628971255533872052, 0.095158511682492784810, 0.062253523938647892863,
                                     0.027152459411754094852};

static double g_times[3];
void qrot_last_times(double out[3]) { memcpy(out, g_times, sizeof(g_times)); }
static double now_s(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + 1e-9 * t.tv_nsec;
}

void qrot_grid(double theta[G], double phi[G], double weights[G]) {
    for (int k = 0; k < G; k++) {
        phi[k] = M_PI * roots[k] + M_PI;                /* rotational_eigenspectrum.c:258 */
        theta[k] = 0.5 * M_PI * roots[k] + 0.5 * M_PI;  /* :260 */
        weights[k] = gl_weights[k];
    }
}

/* Y_lm(theta, phi): sqrt((2l + 1) / 4 pi (l - |m|)! / (l + |m|)!) P_l^|m|(cos theta) e^{i m phi}, Condon-Shortley phase
 * in P, and for m < 0 the reference's Y_l(-m) = (-1)^m cc(Y_lm) (rotational_basis.c:130-137).  sin(theta) enters with its
 * sign, as in the reference's table: the symmetry test evaluates it at theta + pi. */
double qrot_basis(int type, int l, int m, double theta, double phi) {
    const int ma = abs(m);
    const double x = cos(theta), s = sin(theta);
    double pmm = 1.0; /* P_ma^ma = (-1)^ma (2 ma - 1)!! s^ma */
    for (int k = 1; k <= ma; k++) pmm *= -(2.0 * k - 1.0) * s;
    double p = pmm;
    if (l > ma) {
        double pm1 = pmm, pl = x * (2.0 * ma + 1.0) * pmm; /* P_{ma+1}^ma */
        for (int ll = ma + 2; ll <= l; ll++) {
            const double next = (x * (2.0 * ll - 1.0) * pl - (ll + ma - 1.0) * pm1) / (double)(ll - ma);
            pm1 = pl;
            pl = next;
        }
        p = pl;
    }
    double ratio = 1.0; /* (l - ma)! / (l + ma)! */
    for (int k = l - ma + 1; k <= l + ma; k++) ratio /= (double)k;
    const double legendre = sqrt((2.0 * l + 1.0) / (4.0 * M_PI) * ratio) * p;
    double Ylm;
    if (m < 0) {
        Ylm = (type == 0) ? legendre * cos((double)ma * phi) : -1.0 * legendre * sin((double)ma * phi);
        if (ma & 1) Ylm *= -1.0;
    } else {
        Ylm = (type == 0) ? legendre * cos((double)m * phi) : legendre * sin((double)m * phi);
    }
    return Ylm;
}

/* Y_lm on the grid, [index][p * G + t], index = l (l + 1) + m: made once per l_max */
static double *g_yre, *g_yim;
static int g_ylmax = -1;
static int basis_table(int l_max) {
    if (g_ylmax == l_max) return 0;
    const int dim = (l_max + 1) * (l_max + 1);
    free(g_yre);
    free(g_yim);
    g_yre = malloc((size_t)dim * G * G * sizeof(double));
    g_yim = malloc((size_t)dim * G * G * sizeof(double));
    g_ylmax = -1;
    if (!g_yre || !g_yim) return -1;
    double theta[G], phi[G], w[G];
    qrot_grid(theta, phi, w);
    for (int l = 0, index = 0; l <= l_max; l++)
        for (int m = -l; m <= l; m++, index++)
            for (int p = 0; p < G; p++)
                for (int t = 0; t < G; t++) {
                    g_yre[((size_t)index * G + p) * G + t] = qrot_basis(0, l, m, theta[t], phi[p]);
                    g_yim[((size_t)index * G + p) * G + t] = qrot_basis(1, l, m, theta[t], phi[p]);
                }
    g_ylmax = l_max;
    return 0;
}

/* rotational_hamiltonian() + rotational_integrate(): h [dim][dim][2], row-major */
int qrot_hamiltonian(int l_max, double B, const double V[G][G], double *h) {
    const int dim = (l_max + 1) * (l_max + 1);
    if (l_max < 0 || l_max > QROT_L_LIMIT || basis_table(l_max)) return -1; /* (no table: nothing is written) */
    for (int i = 0, li = 0; i < dim; i++) {
        const int mi = i - li * (li + 1);
        const double *yir = g_yre + (size_t)i * G * G, *yii = g_yim + (size_t)i * G * G;
        for (int j = i; j < dim; j++) {
            const double *yjr = g_yre + (size_t)j * G * G, *yji = g_yim + (size_t)j * G * G;
            double re = 0, im = 0;
            for (int p = 0; p < G; p++) {
                const double phi_weight = gl_weights[p];
                for (int t = 0; t < G; t++) {
                    const double theta_weight = gl_weights[t];
                    const double potential = V[t][p];
                    const int k = p * G + t;
                    double integrand = (yir[k] * yjr[k] + yii[k] * yji[k]);
                    integrand *= potential;
                    re += phi_weight * theta_weight * integrand;
                    integrand = (yir[k] * yji[k] - yii[k] * yjr[k]);
                    integrand *= potential;
                    im += phi_weight * theta_weight * integrand;
                }
            }
            re *= 0.5 * M_PI * M_PI;
            im *= 0.5 * M_PI * M_PI;
            h[2 * ((size_t)i * dim + j)] = re;
            h[2 * ((size_t)i * dim + j) + 1] = im;
            if (i != j) {
                h[2 * ((size_t)j * dim + i)] = re;
                h[2 * ((size_t)j * dim + i) + 1] = -1.0 * im;
            } else {
                h[2 * ((size_t)i * dim + j)] += B * ((double)(li * (li + 1)));
            }
        }
        if (mi == li) li++;
    }
    return 0;
}

/* Cyclic Jacobi for a complex Hermitian matrix.  A rotation in the (p, q) plane with a_pq = |a_pq| e^{i f}: J = D R, D =
 * diag(.., 1 at p, .., e^{-i f} at q, ..) makes the element real, R is the real Jacobi rotation that annihilates it
 * (t = sgn(tau) / (|tau| + sqrt(1 + tau^2)), tau = (a_qq - a_pp) / 2 |a_pq|); A <- J^H A J, V <- V J.  Sweeps run until the
 * off-diagonal norm is below 2^-53 of the matrix norm (or exactly zero). */
int qrot_jacobi(int dim, const double *h, double *eval, double *evec, long *rotations) {
    const size_t n = (size_t)dim;
    double *a = malloc(n * n * 2 * sizeof(double)), *v = calloc(n * n * 2, sizeof(double));
    long rot = 0;
    int sweeps = -1;
    if (!a || !v) {
        free(a);
        free(v);
        return -1;
    }
    memcpy(a, h, n * n * 2 * sizeof(double));
    for (size_t i = 0; i < n; i++) v[2 * (i * n + i)] = 1.0;
    double norm2 = 0;
    for (size_t k = 0; k < n * n * 2; k++) norm2 += a[k] * a[k];
#define RE(M, r, c) M[2 * ((size_t)(r) * n + (c))]
#define IM(M, r, c) M[2 * ((size_t)(r) * n + (c)) + 1]
    for (int sweep = 0; sweep <= 64; sweep++) {
        double off2 = 0;
        for (size_t p = 0; p < n; p++)
            for (size_t q = p + 1; q < n; q++) off2 += 2.0 * (RE(a, p, q) * RE(a, p, q) + IM(a, p, q) * IM(a, p, q));
        if (off2 == 0.0 || off2 <= 0x1p-106 * norm2) {
            sweeps = sweep;
            break;
        }
        if (sweep == 64) break;
        for (size_t p = 0; p < n; p++)
            for (size_t q = p + 1; q < n; q++) {
                const double xr = RE(a, p, q), xi = IM(a, p, q);
                const double mag = hypot(xr, xi);
                if (mag == 0.0) continue;
                const double er = xr / mag, ei = xi / mag; /* e^{i f} */
                const double tau = (RE(a, q, q) - RE(a, p, p)) / (2.0 * mag);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                /* J: J_pp = c, J_pq = s, J_qp = -s e^{-i f}, J_qq = c e^{-i f} */
                const double jqp_r = -s * er, jqp_i = s * ei, jqq_r = c * er, jqq_i = -c * ei;
                for (int pass = 0; pass < 2; pass++) { /* M <- M J for M = A, then V */
                    double *M = pass ? v : a;
                    for (size_t k = 0; k < n; k++) {
                        const double pr = RE(M, k, p), pi = IM(M, k, p), qr = RE(M, k, q), qi = IM(M, k, q);
                        RE(M, k, p) = pr * c + (qr * jqp_r - qi * jqp_i);
                        IM(M, k, p) = pi * c + (qr * jqp_i + qi * jqp_r);
                        RE(M, k, q) = pr * s + (qr * jqq_r - qi * jqq_i);
                        IM(M, k, q) = pi * s + (qr * jqq_i + qi * jqq_r);
                    }
                }
                for (size_t k = 0; k < n; k++) { /* A <- J^H A: rows p and q */
                    const double pr = RE(a, p, k), pi = IM(a, p, k), qr = RE(a, q, k), qi = IM(a, q, k);
                    /* conj(J_qp) = -s e^{i f}, conj(J_qq) = c e^{i f} */
                    RE(a, p, k) = c * pr + (jqp_r * qr + jqp_i * qi);
                    IM(a, p, k) = c * pi + (jqp_r * qi - jqp_i * qr);
                    RE(a, q, k) = s * pr + (jqq_r * qr + jqq_i * qi);
                    IM(a, q, k) = s * pi + (jqq_r * qi - jqq_i * qr);
                }
                RE(a, p, q) = IM(a, p, q) = RE(a, q, p) = IM(a, q, p) = 0.0;
                IM(a, p, p) = IM(a, q, q) = 0.0;
                ++rot;
            }
    }
    if (rotations) *rotations = rot;
    if (sweeps >= 0) { /* ascending order (insertion sort of an index: dim <= 81) */
        int *order = malloc(n * sizeof(int));
        if (!order) sweeps = -1;
        for (int i = 0; i < dim && sweeps >= 0; i++) {
            int k = i;
            while (k > 0 && RE(a, order[k - 1], order[k - 1]) > RE(a, i, i)) {
                order[k] = order[k - 1];
                k--;
            }
            order[k] = i;
        }
        for (int i = 0; i < dim && sweeps >= 0; i++) {
            eval[i] = RE(a, order[i], order[i]);
            for (size_t k = 0; k < n; k++) { /* eigenvector i = column order[i] of V */
                evec[2 * ((size_t)i * n + k)] = RE(v, k, order[i]);
                evec[2 * ((size_t)i * n + k) + 1] = IM(v, k, order[i]);
            }
        }
        free(order);
    }
#undef RE
#undef IM
    free(a);
    free(v);
    return sweeps;
}

/* determine_rotational_eigensymmetry(), rotational_eigenspectrum.c:78-130: the real parts only, the largest of 64 random
 * points, and the (theta + pi, phi + pi) "inversion", as written.  evec: [dim][2] of one level. */
int qrot_symmetry(system_t *system, int l_max, const double *evec) {
    double max_sqmod = 0, max_theta = 0, max_phi = 0;
    for (int i = 0; i < QUANTUM_ROTATION_SYMMETRY_POINTS; i++) {
        const double theta = get_rand(system) * M_PI;
        const double phi = get_rand(system) * 2.0 * M_PI;
        double wf = 0;
        for (int l = 0, index = 0; l <= l_max; l++)
            for (int m = -l; m <= l; m++, index++) wf += evec[2 * index] * qrot_basis(0, l, m, theta, phi);
        const double sqmod = wf * wf;
        if (sqmod > max_sqmod) {
            max_sqmod = sqmod;
            max_theta = theta;
            max_phi = phi;
        }
    }
    double max_wf = 0, inv_wf = 0;
    for (int l = 0, index = 0; l <= l_max; l++)
        for (int m = -l; m <= l; m++, index++) {
            max_wf += evec[2 * index] * qrot_basis(0, l, m, max_theta, max_phi);
            inv_wf += evec[2 * index] * qrot_basis(0, l, m, (max_theta + M_PI), (max_phi + M_PI));
        }
    return (max_wf * inv_wf < 0.0) ? QUANTUM_ROTATION_ANTISYMMETRIC : QUANTUM_ROTATION_SYMMETRIC;
}

static void mat_vec(const double r[3][3], const double in[3], double out[3]) {
    for (int k = 0; k < 3; k++) out[k] = r[k][0] * in[0] + r[k][1] * in[1] + r[k][2] * in[2];
}

/* align_molecule() then rotate_spherical() (rotational_potential.c:50-200) for every grid point, each from the unmodified
 * coordinates, about the stored centre of mass.  xyz [256][n][3], index p * G + t. */
int qrot_placements(const molecule_t *molecule, double *xyz) {
    int n = 0;
    for (const atom_t *a = molecule->atoms; a; a = a->next) n++;
    double *al = malloc((size_t)(n > 0 ? n : 1) * 3 * sizeof(double));
    if (!al || n < 2) {
        free(al);
        return -1;
    }
    const double *com = molecule->com;
    /* ---- align_molecule(): translate to the origin, the axis from the SECOND atom on, the first one off the origin */
    int k = 0, axis = -1;
    for (const atom_t *a = molecule->atoms; a; a = a->next, k++) {
        for (int q = 0; q < 3; q++) al[3 * k + q] = a->pos[q] - com[q];
        if (k >= 1 && axis < 0 && !((al[3 * k] == 0.0) && (al[3 * k + 1] == 0.0) && (al[3 * k + 2] == 0.0))) axis = k;
    }
    if (axis < 0) {
        free(al);
        return -1;
    }
    const double *v = al + 3 * axis;
    double theta, phi;
    if (v[2] == 0.0)
        theta = M_PI / 2.0;
    else
        theta = acos(v[2] / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
    if (v[0] == 0) {
        if (v[1] > 0.0 + 1.0e-12)
            phi = M_PI / 2.0;
        else if (v[1] < 0.0 - 1.0e-12)
            phi = 3.0 / 2.0 * M_PI;
        else
            phi = 0.0;
    } else if (v[1] == 0) {
        if (v[1] > 0.0) /* (never: kept as the reference has it) */
            phi = 0;
        else
            phi = M_PI;
    } else {
        phi = atan(fabs(v[1] / v[0]));
        if ((v[1] / v[0]) < 0.0) phi *= -1.0;
    }
    double r[3][3];
    r[0][0] = cos(theta) * cos(phi);
    r[0][1] = cos(theta) * sin(phi);
    r[0][2] = -sin(theta);
    r[1][0] = -sin(phi);
    r[1][1] = cos(phi);
    r[1][2] = 0;
    r[2][0] = sin(theta) * cos(phi);
    r[2][1] = sin(theta) * sin(phi);
    r[2][2] = cos(theta);
    for (k = 0; k < n; k++) {
        double out[3];
        mat_vec(r, al + 3 * k, out);
        for (int q = 0; q < 3; q++) al[3 * k + q] = out[q] + com[q]; /* ... and back from the origin */
    }
    /* ---- rotate_spherical() to every (theta, phi) of the grid */
    double gt[G], gp[G], w[G];
    qrot_grid(gt, gp, w);
    for (int p = 0; p < G; p++)
        for (int t = 0; t < G; t++) {
            r[0][0] = cos(gp[p]) * cos(gt[t]);
            r[0][1] = -sin(gp[p]);
            r[0][2] = cos(gp[p]) * (-sin(gt[t]));
            r[1][0] = sin(gp[p]) * cos(gt[t]);
            r[1][1] = cos(gp[p]);
            r[1][2] = sin(gp[p]) * (-sin(gt[t]));
            r[2][0] = sin(gt[t]);
            r[2][1] = 0;
            r[2][2] = cos(gt[t]);
            double *dst = xyz + (size_t)(p * G + t) * n * 3;
            for (k = 0; k < n; k++) {
                double in[3], out[3];
                for (int q = 0; q < 3; q++) in[q] = al[3 * k + q] - com[q];
                mat_vec(r, in, out);
                for (int q = 0; q < 3; q++) dst[3 * k + q] = out[q] + com[q];
            }
        }
    free(al);
    return n;
}

/* rotational_potential() under quantum_rotation_hindered: B * barrier * sin^2(theta), times the grid's sin(theta) */
void qrot_hindered_grid(double B, double barrier, double V[G][G]) {
    double gt[G], gp[G], w[G];
    qrot_grid(gt, gp, w);
    for (int p = 0; p < G; p++)
        for (int t = 0; t < G; t++) {
            const double rval = sin(gt[t]);
            V[t][p] = sin(gt[t]) * (B * barrier * (rval * rval));
        }
}

/* qrot_options() (check_input.c:236-280) and what this layer refuses */
int qrot_check(system_t *system) {
    char linebuf[MAXLINE];
    if (!system->quantum_rotation) return 0;
    output("INPUT: Quantum rotational eigenspectrum calculation enabled\n");
    if (system->quantum_rotation_B <= 0.0) {
        error("INPUT: invalid quantum rotational constant B specified\n");
        return -1;
    }
    snprintf(linebuf, MAXLINE, "INPUT: Quantum rotational constant B = %.3f K (%.3f cm^-1)\n", system->quantum_rotation_B,
             system->quantum_rotation_B * KB_SI / (100.0 * H_SI * C_SI));
    output(linebuf);
    if (system->quantum_rotation_level_max <= 0) {
        error("INPUT: invalid quantum rotation level max\n");
        return -1;
    }
    snprintf(linebuf, MAXLINE, "INPUT: Quantum rotation level max = %d\n", system->quantum_rotation_level_max);
    output(linebuf);
    if (system->quantum_rotation_l_max <= 0) {
        error("INPUT: invalid quantum rotation l_max\n");
        return -1;
    }
    if (system->quantum_rotation_l_max > QROT_L_LIMIT) {
        error("INPUT: quantum_rotation_l_max above 8 is refused: the basis is defined up to l = 8\n");
        return -1;
    }
    snprintf(linebuf, MAXLINE, "INPUT: Quantum rotation l_max = %d\n", system->quantum_rotation_l_max);
    output(linebuf);
    if (system->quantum_rotation_level_max > (system->quantum_rotation_l_max + 1) * (system->quantum_rotation_l_max + 1)) {
        error("INPUT: quantum rotational levels cannot exceed l_max + 1 X l_max +1\n");
        return -1;
    }
    if (system->quantum_rotation_sum <= 0 || system->quantum_rotation_sum > system->quantum_rotation_level_max) {
        error("INPUT: quantum rotational sum for partition function invalid\n");
        return -1;
    }
    snprintf(linebuf, MAXLINE, "INPUT: Quantum rotation sum = %d\n", system->quantum_rotation_sum);
    output(linebuf);
    if (system->ensemble == ENSEMBLE_NPT || system->ensemble == ENSEMBLE_SURF) {
        error("INPUT: quantum_rotation with ensemble npt or surf is not implemented by this host layer\n");
        return -1;
    }
    for (const molecule_t *m = system->molecules; m; m = m->next)
        if (!m->frozen && !(m->atoms && m->atoms->next)) {
            error("INPUT: quantum_rotation needs at least two sites on every movable molecule (not enough atomic sites to "
                  "calculate angular orientation)\n");
            return -1;
        }
    return 0;
}

/* quantum_system_rotational_energies(), rotational_eigenspectrum.c:269-339 */
int quantum_system_rotational_energies(system_t *system) {
    const int l_max = system->quantum_rotation_l_max, level_max = system->quantum_rotation_level_max;
    const int dim = (l_max + 1) * (l_max + 1);
    if (l_max < 1 || l_max > QROT_L_LIMIT || level_max < 1 || level_max > dim) return -1;
    double V[G][G], gt[G], gp[G], w[G];
    qrot_grid(gt, gp, w);
    double *h = malloc((size_t)dim * dim * 2 * sizeof(double)), *evec = malloc((size_t)dim * dim * 2 * sizeof(double));
    double eval[QROT_DIM_LIMIT], *xyz = NULL, trial[G * G];
    int rc = h && evec ? 0 : -1, xyz_sites = 0;
    memset(g_times, 0, sizeof(g_times));
    for (molecule_t *m = system->molecules; m && !rc; m = m->next) {
        if (m->frozen) continue;
        /* generate the necessary grids */
        double t0 = now_s();
        if (system->quantum_rotation_hindered) {
            qrot_hindered_grid(system->quantum_rotation_B, system->quantum_rotation_hindered_barrier, V);
        } else {
            int n = 0;
            for (const atom_t *a = m->atoms; a; a = a->next) n++;
            if (n > xyz_sites) {
                free(xyz);
                xyz = malloc((size_t)G * G * n * 3 * sizeof(double));
                xyz_sites = xyz ? n : 0;
            }
            if (!xyz || qrot_placements(m, xyz) != n) {
                error("QROT: a movable molecule has no site off its centre of mass\n");
                rc = -1;
                break;
            }
            if (energy_hip_trial_energies(system, m, G * G, xyz, trial)) {
                rc = -1;
                break;
            }
            for (int p = 0; p < G; p++)
                for (int t = 0; t < G; t++) V[t][p] = sin(gt[t]) * trial[p * G + t];
        }
        double t1 = now_s();
        /* get the eigenspectrum */
        if (qrot_hamiltonian(l_max, system->quantum_rotation_B, (const double(*)[G])V, h)) {
            error("QROT: no memory for the table of spherical harmonics\n");
            rc = -1;
            break;
        }
        double t2 = now_s();
        if (qrot_jacobi(dim, h, eval, evec, NULL) < 0) {
            error("QROT: the eigen-solve did not converge (non-finite potential on the grid?)\n");
            rc = -1;
            break;
        }
        for (int i = 0; i < level_max; i++) m->quantum_rotational_energies[i] = eval[i];
        for (int i = 0; i < level_max; i++)
            m->quantum_rotational_eigensymmetry[i] = qrot_symmetry(system, l_max, evec + (size_t)i * dim * 2);
        /* sum over states into molecular rotational partition functions; 3: degeneracy of the nuclear wavefunction */
        m->rot_partfunc_g = 0;
        m->rot_partfunc_u = 0;
        for (int i = 0; i < system->quantum_rotation_sum; i++) {
            if (m->quantum_rotational_eigensymmetry[i] == QUANTUM_ROTATION_SYMMETRIC)
                m->rot_partfunc_g += exp(-m->quantum_rotational_energies[i] / system->temperature);
            else
                m->rot_partfunc_u += 3. * exp(-m->quantum_rotational_energies[i] / system->temperature);
        }
        if (m->nuclear_spin == NUCLEAR_SPIN_PARA)
            m->rot_partfunc = m->rot_partfunc_g / (m->rot_partfunc_g + m->rot_partfunc_u);
        else
            m->rot_partfunc = m->rot_partfunc_u / (m->rot_partfunc_g + m->rot_partfunc_u);
        double t3 = now_s();
        g_times[0] += t1 - t0;
        g_times[1] += t2 - t1;
        g_times[2] += t3 - t2;
        /* the reference's DEBUG_QROT lines (rotational_eigenspectrum.c:307-322), one per level */
        for (int i = 0; i < level_max; i++) {
            const double e = m->quantum_rotational_energies[i];
            printf("DEBUG_QROT: molecule #%d (%s) rotational level %d = %.6f K (%.6f cm^-1 or %.6f meV or %.6f / B) ", m->id,
                   m->moleculetype, i, e, e * KB_SI / (100.0 * H_SI * C_SI),
                   8.61733238e-2 * (e - m->quantum_rotational_energies[0]), e / system->quantum_rotation_B);
            if (m->quantum_rotational_eigensymmetry[i] == QUANTUM_ROTATION_SYMMETRIC)
                printf("*** symmetric ***");
            else
                printf("*** antisymmetric ***");
            printf("\n");
        }
        if (system->quantum_rotation_eigenvectors)
            for (int i = 0; i < level_max; i++) {
                printf("DEBUG_QROT: molecule #%d (%s) eigenvec rot level %d\n", m->id, m->moleculetype, i);
                for (int j = 0; j < dim; j++)
                    printf("\tj=%d %.6f %.6f\n", j, evec[2 * ((size_t)i * dim + j)], evec[2 * ((size_t)i * dim + j) + 1]);
                printf("\n");
            }
        fflush(stdout);
    }
    free(h);
    free(evec);
    free(xyz);
    return rc;
}
