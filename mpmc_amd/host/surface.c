/* surface.c -- `ensemble surf`: the potential energy curve of a dimer (reference src/mc/surface.c:227-380), restated on
 * the device's dimer scans (mpmc_hip_dimer_grid_means, include/mpmc_hip.h).
 *
 * What is kept as the reference has it: the loop bounds -- `for (r = surf_min; r <= surf_max; r += surf_inc)` and, per
 * angle, `for (x = 0; x <= 2 pi (or pi); x += surf_ang)`, in double -- which decide the grid sizes; the preserve mode
 * (identity rotations on the input orientation, after the optional one-off surf_preserve_rotation); the printed lines.
 * OWNED DEVIATIONS: every placement is built from the pristine body frame, where the reference
 * rotates and un-rotates the live coordinates cumulatively; the mean is the engine's fixed-order sum, where the reference
 * keeps a running average; and under surf_decomp with disp_expansion the rd column is the true value, where the
 * reference's is stale (its ENERGY_ES call consumes the pair list's "changed" flag and disp_expansion_nopbc skips
 * every pair). */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "mpmc_host.h"

#define SURF_MAX_SITES 16 /* the ABI's molecule limit */

int surface_loop_count(double top, double step) {
    int n = 0;
    for (double x = 0; x <= top; x += step) ++n;
    return n;
}

static int natoms_of(const molecule_t *m) {
    int n = 0;
    for (const atom_t *a = m->atoms; a; a = a->next) ++n;
    return n;
}

const char *surface_refused(const system_t *s) {
    if (s->surf_virial) return "surf_virial is parsed by the reference and computed nowhere; it is not implemented";
    if (s->surf_output_on || s->surf_print_level) return "surf_output / surf_print_level (the surface trajectory file) is not implemented";
    if (s->sg) return "sg is not implemented in the non-periodic sums";
    if (s->dreiding) return "dreiding is not implemented in the non-periodic sums";
    if (s->lj_buffered_14_7) return "lj_buffered_14_7 is not implemented in the non-periodic sums";
    if (s->axilrod_teller) return "axilrod_teller is not implemented in the non-periodic sums";
    if (s->polarvdw) return "polarvdw (cdvdw) is not implemented in the non-periodic sums";
    if (s->cdvdw_exp_repulsion || s->cdvdw_sig_repulsion || s->cdvdw_9th_repulsion)
        return "the cdvdw_*_repulsion family is not implemented in the non-periodic sums";
    if (s->disp_expansion_mbvdw) return "disp_expansion_mbvdw is not implemented";
    if (s->gilbert_smith_mixing || s->bohm_ahlrichs_mixing || s->wilson_popelier_mixing)
        return "gilbert_smith_mixing / bohm_ahlrichs_mixing / wilson_popelier_mixing are not implemented";
    if (s->polarization && !s->rd_only) {
        if (s->polar_wolf) return "polar_wolf needs a cell; a dimer scan has none";
        if (s->polar_wolf_full) return "polar_wolf_full needs a cell; a dimer scan has none";
        if (s->polar_ewald) return "polar_ewald needs a cell; a dimer scan has none";
        if (s->polar_ewald_full) return "polar_ewald_full needs a cell; a dimer scan has none";
        if (!s->polar_iterative) return "polar_iterative off (matrix inversion) is not implemented for dimer scans";
        if (s->polar_sor) return "polar_sor is not implemented for dimer scans";
        if (s->polar_esor) return "polar_esor is not implemented for dimer scans";
        if (s->polar_zodid) return "polar_zodid is not implemented for dimer scans";
        if (s->polar_rrms) return "polar_rrms is not implemented for dimer scans";
    }
    const molecule_t *a = s->molecules, *b = a ? a->next : NULL;
    if (!b) return "the input PQR has only a single molecule";
    if (b->next) return "the input PQR must contain exactly two molecules";
    if (a->frozen && b->frozen) return "both molecules are frozen (the reference never measures such pairs without polarization)";
    if (natoms_of(a) > SURF_MAX_SITES || natoms_of(b) > SURF_MAX_SITES) return "more than 16 sites on a molecule";
    return NULL;
}

typedef struct {
    int n;
    double x[SURF_MAX_SITES], y[SURF_MAX_SITES], z[SURF_MAX_SITES], charge[SURF_MAX_SITES], alpha[SURF_MAX_SITES],
        eps[SURF_MAX_SITES], sig[SURF_MAX_SITES], mass[SURF_MAX_SITES], c6[SURF_MAX_SITES], c8[SURF_MAX_SITES],
        c10[SURF_MAX_SITES];
    mpmc_hip_molecule m;
} surf_molecule;

static void surf_fill(surf_molecule *o, const molecule_t *mol, int with_alpha) {
    memset(o, 0, sizeof(*o));
    for (const atom_t *a = mol->atoms; a; a = a->next, o->n++) {
        const int k = o->n;
        o->x[k] = a->pos[0];
        o->y[k] = a->pos[1];
        o->z[k] = a->pos[2];
        o->charge[k] = a->charge;
        o->alpha[k] = with_alpha ? a->polarizability : 0.0;
        o->eps[k] = a->epsilon;
        o->sig[k] = a->sigma;
        o->mass[k] = a->mass;
        o->c6[k] = a->c6;
        o->c8[k] = a->c8;
        o->c10[k] = a->c10;
    }
    o->m.count = o->n;
    o->m.x = o->x;
    o->m.y = o->y;
    o->m.z = o->z;
    o->m.charge = o->charge;
    o->m.polarizability = o->alpha;
    o->m.epsilon = o->eps;
    o->m.sigma = o->sig;
    o->m.mass = o->mass;
    o->m.c6 = o->c6;
    o->m.c8 = o->c8;
    o->m.c10 = o->c10;
}

/* The one-off surf_preserve_rotation (surface.c:247-254): surface_dimer_geometry(r = 0) with the six angles, i.e. each
 * molecule rotated about its mass-weighted centre; the later placements then use identity rotations on the result. */
static void surf_rotate_about_com(surf_molecule *o, int global_axis, const double ang[3]) {
    double mass = 0.0, com[3] = {0.0, 0.0, 0.0}, R[9];
    for (int k = 0; k < o->n; k++) {
        mass += o->mass[k];
        com[0] += o->mass[k] * o->x[k];
        com[1] += o->mass[k] * o->y[k];
        com[2] += o->mass[k] * o->z[k];
    }
    for (int p = 0; p < 3; p++) com[p] /= mass;
    const double alpha = ang[0], beta = ang[1], gamma = ang[2];
    if (!global_axis) { /* molecule_rotate_euler(), surface.c:116-125 */
        R[0] = cos(gamma) * cos(beta) * cos(alpha) - sin(gamma) * sin(alpha);
        R[1] = sin(gamma) * cos(beta) * cos(alpha) + cos(gamma) * sin(alpha);
        R[2] = -sin(beta) * cos(alpha);
        R[3] = -cos(gamma) * cos(beta) * sin(alpha) - sin(gamma) * cos(alpha);
        R[4] = -sin(gamma) * cos(beta) * sin(alpha) + cos(gamma) * cos(alpha);
        R[5] = sin(beta) * sin(alpha);
        R[6] = cos(gamma) * sin(beta);
        R[7] = sin(gamma) * sin(beta);
        R[8] = cos(beta);
    } else { /* molecule_rotate_quaternion(), surface.c:177-193: degrees, z then y then x */
        double q[4] = {0., 0., 0., 1.}; /* x y z w */
        const double axes[3][3] = {{0., 0., 1.}, {0., 1., 0.}, {1., 0., 0.}};
        for (int k = 0; k < 3; k++) {
            const double half = ang[k] / 57.2957795 / 2, s = sin(half);
            const double a[4] = {axes[k][0] * s, axes[k][1] * s, axes[k][2] * s, cos(half)}, b[4] = {q[0], q[1], q[2], q[3]};
            q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
            q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
            q[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
            q[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
        }
        const double xx = q[0] * q[0], yy = q[1] * q[1], zz = q[2] * q[2], ww = q[3] * q[3];
        R[0] = ww + xx - yy - zz;
        R[1] = 2.0 * (q[0] * q[1] - q[3] * q[2]);
        R[2] = 2.0 * (q[0] * q[2] + q[3] * q[1]);
        R[3] = 2.0 * (q[0] * q[1] + q[3] * q[2]);
        R[4] = ww - xx + yy - zz;
        R[5] = 2.0 * (q[1] * q[2] - q[3] * q[0]);
        R[6] = 2.0 * (q[0] * q[2] - q[3] * q[1]);
        R[7] = 2.0 * (q[1] * q[2] + q[3] * q[0]);
        R[8] = ww - xx - yy + zz;
    }
    for (int k = 0; k < o->n; k++) {
        const double x = o->x[k] - com[0], y = o->y[k] - com[1], z = o->z[k] - com[2];
        o->x[k] = R[0] * x + R[1] * y + R[2] * z + com[0];
        o->y[k] = R[3] * x + R[4] * y + R[5] * z + com[1];
        o->z[k] = R[6] * x + R[7] * y + R[8] * z + com[2];
    }
}

static double *surf_angles(double top, double step, int *n) {
    *n = surface_loop_count(top, step);
    double *v = malloc((size_t)(*n > 0 ? *n : 1) * sizeof(double));
    int k = 0;
    for (double x = 0; x <= top; x += step) v[k++] = x;
    return v;
}

int surface(system_t *system, int device) {
    char linebuf[MAXLINE];
    const char *why = surface_refused(system);
    if (why) {
        snprintf(linebuf, MAXLINE, "SURFACE: %s\n", why);
        error(linebuf);
        return -1;
    }
    const int polar = system->polarization && !system->rd_only;
    surf_molecule a, b;
    surf_fill(&a, system->molecules, polar);
    surf_fill(&b, system->molecules->next, polar);

    mpmc_hip_dimer_params p;
    mpmc_hip_default_dimer_params(&p);
    p.rd_form = MPMC_HIP_RD_LJ;
    p.mixing = system->waldmanhagler ? MPMC_HIP_RD_MIX_WALDMAN_HAGLER
               : system->halgren_mixing ? MPMC_HIP_RD_MIX_HALGREN
               : system->c6_mixing ? MPMC_HIP_RD_MIX_C6 : MPMC_HIP_RD_MIX_LB;
    p.disp_expansion = system->disp_expansion;
    p.damp_dispersion = system->damp_dispersion;
    p.extrapolate_disp_coeffs = system->extrapolate_disp_coeffs;
    p.schmidt_mixing = system->schmidt_mixing;
    if (p.disp_expansion) p.mixing = MPMC_HIP_RD_MIX_LB; /* (pairs.c:84-211: the first rule that matches decides) */
    p.rd_only = system->rd_only;
    p.damp_type = system->damp_type;
    p.polar_damp = system->polar_damp;
    p.polar_max_iter = system->polar_max_iter;
    p.polar_precision = system->polar_precision;
    p.polar_gs = system->polar_gs;
    p.polar_gs_ranked = system->polar_gs_ranked;
    p.polar_palmo = system->polar_palmo;
    p.polar_gamma = system->polar_gamma;
    p.global_axis = system->surf_global_axis_on;

    double zero = 0.0, *lists[6];
    int n[6];
    if (system->surf_preserve) {
        if (system->surf_preserve_rotation_on) {
            const double *g = system->surf_preserve_rotation;
            surf_rotate_about_com(&a, p.global_axis, g);
            surf_rotate_about_com(&b, p.global_axis, g + 3);
            printf("SURFACE: Setting preserve angles (radians) for molecule 1: %lf %lf %lf\n", g[0], g[1], g[2]);
            printf("SURFACE: Setting preserve angles (radians) for molecule 2: %lf %lf %lf\n", g[3], g[4], g[5]);
        }
        for (int k = 0; k < 6; k++) lists[k] = &zero, n[k] = 1;
    } else {
        for (int k = 0; k < 6; k++) lists[k] = surf_angles((k % 3 == 1) ? M_PI : 2.0 * M_PI, system->surf_ang, &n[k]);
    }

    mpmc_hip_ctx *ctx = NULL;
    int rc = 0;
    if (mpmc_hip_create(&ctx, device, 64)) {
        snprintf(linebuf, MAXLINE, "SURFACE: %s\n", mpmc_hip_last_error());
        error(linebuf);
        rc = -1;
    }
    for (double r = system->surf_min; !rc && r <= system->surf_max; r += system->surf_inc) {
        double means[3];
        long long counts[2];
        const double *const angles[6] = {lists[0], lists[1], lists[2], lists[3], lists[4], lists[5]};
        if (mpmc_hip_dimer_grid_means(ctx, &p, &a.m, &b.m, r, n, angles, means, counts)) {
            snprintf(linebuf, MAXLINE, "SURFACE: %s\n", mpmc_hip_last_error());
            error(linebuf);
            rc = -1;
            break;
        }
        if (counts[1]) { /* polar.c:81-88, once per separation instead of once per placement */
            snprintf(linebuf, MAXLINE, "POLAR: polarization iterative solver failed to reach convergence (%lld of %lld placements).\n",
                     counts[1], counts[0]);
            error(linebuf);
        }
        if (system->surf_decomp && system->surf_preserve)
            printf("%.5f %.5f %.5f %.5f %.5f\n", r, means[0], means[1], means[2], 0.0); /* (pe_vdw: polarvdw is refused) */
        else if (system->surf_decomp)
            printf("%.5f %.5f %.5f %.5f\n", r, means[0], means[1], means[2]);
        else
            printf("%.5f %.5f\n", r, means[0] + means[1] + means[2]);
        fflush(stdout);
    }
    if (ctx) mpmc_hip_destroy(ctx);
    if (!system->surf_preserve)
        for (int k = 0; k < 6; k++) free(lists[k]);
    return rc;
}
