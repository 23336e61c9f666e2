/*
 * energy_hip.c -- `double energy(system_t*)` on the MI355X engine: the reference-side binding.
 *
 * Same call surface as the reference's dispatcher (src/energy/energy.c:67-226): the caller hands over the
 * system with its molecule / atom lists and gets the potential energy back, with system->observables,
 * system->iter_success, nodestats->polarization_iterations, natoms and last_volume filled in.  What differs is
 * inside: the lists are flattened to SoA once, the configuration stays resident on the device, and on later
 * calls only what changed is sent (one molecule after make_move(), the same one again after restore(), an
 * inserted / removed molecule under `ensemble uvt`).
 *
 * This one file serves two trees (see energy_hip.h):
 *   reference tree:  src/energy/energy_hip.c, compiled against <structs.h> + <function_prototypes.h>; needs
 *                    one new member, `int hip;`, in system_t (the `hip on` keyword, like `cuda on`);
 *   this repository: mpmc_amd/host/, -DMPMC_SHIM_HOST_MIRROR, against mpmc_host.h.
 * It reads only members both trees have, and keeps every piece of engine state in a side table keyed by
 * `system_t *` -- no engine fields in system_t or molecule_t.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#ifdef MPMC_SHIM_HOST_MIRROR
#include "mpmc_host.h"
#else
#include <structs.h>
#include <function_prototypes.h>
extern int rank, size; /* src/main/main.c:8 (declared in mc.h, which needs the generated cmake_config.h) */
#endif
#include "energy_hip.h"

/* ---- side table ------------------------------------------------------------------------------------------- */

/* a molecule the device holds: where it sits in the list (array index = list position), which device slots it
 * owns, and the list node that represented it when the lists were last walked (a hint for the notes only) */
typedef struct {
    molecule_t *mol;
    atom_t *atoms; /* its first atom then: a frozen molecule whose list node still points there was not touched */
    int slot, natoms, frozen;
} resident_t;

/* a molecule the cavity grid's occupancy holds: its list node then, and its run in the flat coordinate arrays */
typedef struct {
    molecule_t *mol;
    atom_t *atoms;
    int first, natoms, frozen;
} cavity_entry_t;

/* Everything a full upload sends beside the atoms and the box: fill_settings() derives it from the keywords, full_upload()
 * applies it, and energy_hip_begin() compares the whole record -- a mode that has a member here cannot go stale. */
typedef struct {
    mpmc_hip_params params;
    mpmc_hip_disp_params disp;
    mpmc_hip_rd_form_params rd_form; /* the pair potential and mixing rule */
    mpmc_hip_thole_model thole;      /* the dipole tensor (polar_damp_type, polar_wolf_full) */
    int rdc_order;                   /* rd_crystal_order (0: rd_crystal off) */
    int vdw_on;                      /* polarvdw */
    int exact;                       /* the exact dipoles (polarization with polar_iterative off) */
    int axilrod_teller, midzuno_kihara_approx; /* the second decides the per-atom c9 that is sent (0 while the first is off) */
    double ar_scale;                 /* cavity_autoreject_scale (0: cavity_autoreject_absolute off) */
} sent_settings_t;

/* the per-atom columns of the host image; atom_columns() says which member of atom_t each one is */
enum { COL_X, COL_Y, COL_Z, COL_Q, COL_ALPHA, COL_EPS, COL_SIG, COL_MASS, COL_C6, COL_C8, COL_C10, COL_C9, COL_OMEGA, NCOL };

typedef struct shim_state {
    system_t *system;
    mpmc_hip_ctx *ctx;
    mpmc_hip_comm *comm;
    int device;   /* -1: choose (rank % device count) */
    int capacity; /* atoms the context was created for */
    int uploaded; /* a configuration is resident */
    sent_settings_t sent; /* as sent with that upload */
    int failed;   /* device / ABI failure of the last call */
    double last_energy; /* what the last energy_hip_end() returned (restore() takes a rejected trial's out of the observables) */
    /* host image of the device, by DEVICE SLOT (the engine keeps its own atom order once molecules are inserted
     * or removed): coordinates as last sent, and the parameters that tell species apart.  c6 / c8 / c10 (disp_expansion) and
     * omega (polarvdw) go with every full upload; c9 (axilrod_teller) is kept as read, its effective value is what is sent */
    int cap;
    double *col[NCOL];
    /* the resident molecules in LIST order */
    resident_t *res, *res2;
    int nres, res_cap;
    molecule_t **mols; /* scratch: the list as an array */
    int mols_cap;
    /* notes from mc_moves.c since the device was last in line with the lists */
    int in_sync, nnotes;
    struct { molecule_t *now, *was; } notes[8];
    int last_found;
    /* noted volume moves (energy_hip_note_volume_change): one displacement per resident molecule, in list order */
    int nvol, vol_notes_off;
    double *vol_delta[4];
    /* cavity_bias (energy_hip_cavity_update): the grid as sent, and what the device's occupancy was last given -- the
     * molecules in LIST order with their coordinates as read then (raw) and as binned (wrapped), flat, molecule after
     * molecule.  Independent of the residents above: the grid knows no device slot, and at the top of make_move() the
     * resident configuration still is the previous trial's. */
    mpmc_hip_ctx *cav_ctx; /* the context the grid was set on */
    int cav_grid;
    double cav_radius;
    int cav_valid; /* the table below is what the device holds */
    cavity_entry_t *cav, *cav2;
    int ncav, cav_cap;
    double *cav_raw, *cav_raw2, *cav_wrapped, *cav_wrapped2; /* [3 * cav_atoms_cap] each */
    int cav_atoms, cav_atoms_cap;
    double *cav_darts; /* [cav_ndarts][3]: the last call's dart positions */
    int cav_ndarts, cav_darts_cap, cav_hits;
    int cav_failed; /* a device / ABI failure in a cavity call: the next energy_hip() reports it (sticky) */
    long trial_calls;    /* energy_hip_trial_energies() calls that reached the engine */
    long sync_counts[3]; /* full uploads, mpmc_hip_edit_molecules calls that answered 0, molecules they removed + inserted */
    int timing;
    mpmc_hip_timings tsum;
    int walker_rank, walker_nranks;
    double pool_buf[64];
    struct shim_state *next;
} shim_state;

static shim_state *g_states;

static shim_state *state_of(system_t *system, int create) {
    for (shim_state *s = g_states; s; s = s->next)
        if (s->system == system) return s;
    if (!create) return NULL;
    shim_state *s = calloc(1, sizeof(shim_state));
    if (!s) return NULL;
    s->system = system;
    s->device = -1;
    s->walker_nranks = 1;
    s->next = g_states;
    g_states = s;
    return s;
}

static void free_image(shim_state *st) {
    for (int c = 0; c < NCOL; c++) {
        free(st->col[c]);
        st->col[c] = NULL;
    }
    st->cap = 0;
}

void energy_hip_cleanup(system_t *system) {
    shim_state **pp = &g_states;
    for (; *pp && (*pp)->system != system; pp = &(*pp)->next) {}
    shim_state *st = *pp;
    if (!st) return;
    *pp = st->next;
    if (st->comm) mpmc_hip_comm_destroy(st->comm);
    if (st->ctx) mpmc_hip_destroy(st->ctx);
    free_image(st);
    for (int v = 0; v < st->nvol; v++) free(st->vol_delta[v]);
    free(st->res); free(st->res2); free(st->mols);
    free(st->cav); free(st->cav2); free(st->cav_raw); free(st->cav_raw2); free(st->cav_wrapped); free(st->cav_wrapped2);
    free(st->cav_darts);
    free(st);
}

void energy_hip_set_device(system_t *system, int device) {
    shim_state *st = state_of(system, 1);
    if (st) st->device = device;
}
mpmc_hip_ctx *energy_hip_context(system_t *system) {
    shim_state *st = state_of(system, 0);
    return st ? st->ctx : NULL;
}
int energy_hip_failed(system_t *system) {
    shim_state *st = state_of(system, 0);
    return st ? st->failed : 0;
}
double energy_hip_last_energy(system_t *system) {
    shim_state *st = state_of(system, 0);
    return st ? st->last_energy : 0.0;
}
void energy_hip_enable_timing(system_t *system, int on) {
    shim_state *st = state_of(system, 1);
    if (!st) return;
    st->timing = on;
    memset(&st->tsum, 0, sizeof(st->tsum));
}
void energy_hip_get_timings(system_t *system, mpmc_hip_timings *out) {
    shim_state *st = state_of(system, 0);
    if (st) *out = st->tsum;
    else memset(out, 0, sizeof(*out));
}

/* ---- host-side profile (MPMC_HIP_HOST_PROFILE) -------------------------------------------------------------- */
static double g_prof[4]; /* seconds in list work + updates, begin, bookkeeping, end */
static long g_prof_calls, g_prof_base;
static double g_prof_t0, g_prof_tlast;
static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
void energy_hip_profile_report(void) {
    if (getenv("MPMC_HIP_HOST_PROFILE") && g_prof_calls)
    {
        const long nc = g_prof_calls - g_prof_base > 0 ? g_prof_calls - g_prof_base : 1;
        fprintf(stderr, "host energy(): %ld steady-state calls; list work + updates %.1f us, begin %.1f us, bookkeeping %.1f us, "
                        "end %.1f us per call; %.1f us per call between energy() calls (MC logic)\n", nc,
                1e6 * g_prof[0] / nc, 1e6 * g_prof[1] / nc, 1e6 * g_prof[2] / nc, 1e6 * g_prof[3] / nc,
                1e6 * ((g_prof_tlast - g_prof_t0) - (g_prof[0] + g_prof[1] + g_prof[2] + g_prof[3])) / nc);
    }
}

#ifdef MPMC_SHIM_HOST_MIRROR
/* the reference has these in src/energy/energy.c:16-46 and src/energy/pairs.c:364-385 */
int countNatoms(system_t *system) {
    int N = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next) N++;
    return N;
}
static void countN(system_t *system) {
    system->observables->N = 0;
    system->observables->spin_ratio = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        if (!m->frozen) {
            system->observables->N += 1.0;
            /* energy.c:26-27, under quantum_rotation only: runs without it keep printing the 0 they always printed */
            if (system->quantum_rotation && m->nuclear_spin == NUCLEAR_SPIN_PARA) system->observables->spin_ratio += 1.0;
        }
}
void update_com(molecule_t *molecules) {
    for (molecule_t *m = molecules; m; m = m->next) {
        for (int i = 0; i < 3; i++) m->com[i] = 0;
        m->mass = 0;
        for (atom_t *a = m->atoms; a; a = a->next) {
            m->mass += a->mass;
            for (int i = 0; i < 3; i++) m->com[i] += a->mass * a->pos[i];
        }
        for (int i = 0; i < 3; i++) m->com[i] /= m->mass;
    }
}
#endif

/* ---- keyword -> engine parameter, 1:1 ------------------------------------------------------------------------ */
static void fill_params(const system_t *s, mpmc_hip_params *p) {
    memset(p, 0, sizeof(*p)); /* padding too: the record is compared with memcmp() */
    mpmc_hip_default_params(p);
    p->temperature = s->temperature;
    p->rd_only = s->rd_only || s->sg; /* energy.c:108, :154: no electrostatics and no polarization under sg */
    p->rd_lrc = s->rd_lrc;
    p->feynman_hibbs = s->feynman_hibbs;
    p->feynman_hibbs_order = s->feynman_hibbs_order;
    p->ewald_alpha_set = 1; /* pbc() already resolved it (pbc.c:73-76) */
    p->ewald_alpha = s->ewald_alpha;
    p->ewald_kmax = s->ewald_kmax;
    p->polarization = s->polarization;
    p->polar_damp = s->polar_damp;
    p->polar_max_iter = s->polar_max_iter;
    p->polar_precision = s->polar_precision;
    p->polar_gamma = s->polar_gamma;
    p->polar_gs = s->polar_gs;
    p->polar_gs_ranked = s->polar_gs_ranked;
    p->polar_sor = s->polar_sor;
    p->polar_esor = s->polar_esor;
    p->polar_palmo = s->polar_palmo;
    p->polar_rrms = s->polar_rrms;
    p->polar_zodid = s->polar_zodid;
    p->polar_wolf = s->polar_wolf;
    p->polar_wolf_alpha = s->polar_wolf_alpha;
    p->polar_ewald = s->polar_ewald;
    p->polar_ewald_alpha_set = 1;
    p->polar_ewald_alpha = s->polar_ewald_alpha;
    p->wolf = s->wolf;
}

/* energy.c:132-145: sg, dreiding and lj_buffered_14_7 in the order of its branches; a mixing rule alone puts Lennard-Jones on
 * the dense path that knows the rule (pairs.c:84-211, in the order of its branches) */
static void fill_rd_form(const system_t *s, mpmc_hip_rd_form_params *f) {
    memset(f, 0, sizeof(*f));
    f->mixing = s->waldmanhagler ? MPMC_HIP_RD_MIX_WALDMAN_HAGLER
                : s->halgren_mixing ? MPMC_HIP_RD_MIX_HALGREN
                : s->c6_mixing      ? MPMC_HIP_RD_MIX_C6
                                    : MPMC_HIP_RD_MIX_LB;
    if (s->sg)
        f->form = MPMC_HIP_RD_SG;
    else if (s->dreiding)
        f->form = MPMC_HIP_RD_DREIDING;
    else if (s->lj_buffered_14_7)
        f->form = MPMC_HIP_RD_BUFFERED_14_7;
    else if (f->mixing != MPMC_HIP_RD_MIX_LB)
        f->form = MPMC_HIP_RD_LJ;
    if (!f->form) f->mixing = 0;
}

/* thole_matrix.c:90-135: the tensor of the A matrix.  Without polarization the engine keeps its default (the matrix of
 * polarvdw is the exponential one: unsupported() refuses the others there). */
static void fill_thole_model(const system_t *s, mpmc_hip_thole_model *m) {
    memset(m, 0, sizeof(*m));
    m->damp_type = s->polarization ? s->damp_type : DAMPING_EXPONENTIAL;
    m->wolf_full = (s->polarization && s->polar_wolf_full) ? 1 : 0;
}

static void fill_disp_params(const system_t *s, mpmc_hip_disp_params *d) {
    memset(d, 0, sizeof(*d));
    d->disp_expansion = s->disp_expansion;
    d->damp_dispersion = s->damp_dispersion;
    d->extrapolate_disp_coeffs = s->extrapolate_disp_coeffs;
    d->schmidt_mixing = s->schmidt_mixing;
}

static void fill_settings(const system_t *s, sent_settings_t *t) {
    memset(t, 0, sizeof(*t)); /* padding too: the record is compared with memcmp() */
    fill_params(s, &t->params);
    fill_disp_params(s, &t->disp);
    fill_rd_form(s, &t->rd_form);
    fill_thole_model(s, &t->thole);
    t->rdc_order = s->rd_crystal ? s->rd_crystal_order : 0;
    t->vdw_on = (s->polarvdw != 0);
    t->exact = (s->polarization && !s->polar_iterative);
    t->axilrod_teller = (s->axilrod_teller != 0);
    t->midzuno_kihara_approx = (t->axilrod_teller && s->midzuno_kihara_approx);
    t->ar_scale = s->cavity_autoreject_absolute ? s->cavity_autoreject_scale : 0.0;
}

/* The dense energy modes, where every change of N used to be an upload: only there does the walk look two places ahead.  On
 * the standard path it stays as it was: where it gives up and uploads decides the slot order, the slot order the rounding
 * of the sums, and the bits of such chains are on record (tests/golden). */
static int dense_mode(const sent_settings_t *t) {
    return t->disp.disp_expansion || t->axilrod_teller || t->rdc_order || t->rd_form.form;
}

/* What the engine does not compute must not be asked of it silently (the twin of the `cuda on` guard,
 * src/io/check_input.c:325-341, extended to the whole of energy()). */
static const char *unsupported(const system_t *s) {
#ifndef MPMC_SHIM_HOST_MIRROR
    if (s->rd_anharmonic) return "rd_anharmonic (the anharmonic bond) is not on the device";
    if (s->gwp) return "gwp (Gaussian wave packets) is not on the device";
    if (s->spectre) return "spectre is not on the device";
    /* pairs.c:85-141: these mixing branches come before the disp_expansion one (sg is refused above, the cdvdw_*
     * repulsions below) */
    if (s->disp_expansion && (s->waldmanhagler || s->halgren_mixing))
        return "disp_expansion with waldmanhagler / halgren_mixing is not on the device";
    if (s->polarvdw && (s->waldmanhagler || s->halgren_mixing))
        return "polarvdw with waldmanhagler / halgren_mixing is not on the device";
    if (s->polarvdw && s->vdw_fh_2be) return "vdw_fh_2be is not on the device";
    if (s->ensemble == ENSEMBLE_SURF && (s->sg || s->dreiding || s->lj_buffered_14_7 || s->waldmanhagler || s->halgren_mixing ||
                                         s->c6_mixing))
        return "ensemble surf with sg / dreiding / lj_buffered_14_7 or a mixing rule is not on the device";
    if (s->ensemble == ENSEMBLE_NVE) return "ensemble nve is not supported";
#endif
    /* the linear and the undamped tensor and polar_wolf_full are on the device (mpmc_hip_set_thole_model); the reference's
     * polar_ewald_full applies one k-component to all three field components (polar_ewald.c:267-268): nothing to match */
    if (s->polarization && s->polar_ewald_full) return "polar_ewald_full is not on the device";
    if (s->polarization && s->polar_wolf_full && s->damp_type != DAMPING_EXPONENTIAL)
        return "polar_wolf_full needs polar_damp_type exponential";
    if (s->polarvdw && (s->damp_type != DAMPING_EXPONENTIAL || s->polar_wolf_full))
        return "polarvdw with polar_damp_type linear / off or polar_wolf_full is not on the device";
    /* sg, dreiding, lj_buffered_14_7 and the Lennard-Jones mixing rules are on the device (mpmc_hip_set_rd_form); the
     * combinations it does not have are refused by name */
    {
        mpmc_hip_rd_form_params f;
        fill_rd_form(s, &f);
        if (f.form && s->disp_expansion)
            return "disp_expansion with sg / dreiding / lj_buffered_14_7 / c6_mixing is not on the device";
        if (f.form && s->rd_crystal)
            return "rd_crystal with sg / dreiding / lj_buffered_14_7 or a mixing rule is not on the device";
        if (f.form && s->polarvdw)
            return "polarvdw with sg / dreiding / lj_buffered_14_7 / c6_mixing is not on the device";
        if (f.form == MPMC_HIP_RD_SG && f.mixing != MPMC_HIP_RD_MIX_LB)
            return "sg with waldmanhagler / halgren_mixing / c6_mixing is refused (the reference ignores the mixing rule there)";
        if (f.form == MPMC_HIP_RD_SG || (f.form && f.mixing == MPMC_HIP_RD_MIX_WALDMAN_HAGLER)) {
            int nfrozen = 0, negative = 0;
            for (const molecule_t *m = s->molecules; m; m = m->next)
                for (const atom_t *a = m->atoms; a; a = a->next) {
                    nfrozen += (a->frozen != 0);
                    negative |= (a->sigma < 0.0);
                }
            if (f.form == MPMC_HIP_RD_SG && nfrozen >= 2)
                return "sg with two or more frozen atoms is refused (the reference sums uninitialised distances for "
                       "frozen-frozen pairs there)";
            if (f.form != MPMC_HIP_RD_SG && negative)
                return "waldmanhagler with a negative sigma is refused (the reference never assigns the epsilon of such a pair)";
        }
    }
    /* polar_iterative off: the exact dipoles are on the device (mpmc_hip_set_exact_polar); the rest is refused by name */
    if (s->polarization && !s->polar_iterative && s->polar_zodid)
        return "ZODID and matrix inversion cannot both be set! (polar_zodid with polar_iterative off)"; /* check_input.c:349-353 */
    if (s->polarization && !s->polar_iterative && s->polar_palmo)
        return "polar_palmo with polar_iterative off is not on the device (the reference would add a stale ef_induced_change)";
    if (s->polarization && !s->polar_iterative && s->polarvdw)
        return "polarvdw with polar_iterative off is not on the device (the reference forces the iterative solver there)";
    if (s->polarizability_tensor && s->polar_iterative)
        return "iterative polarizability tensor method not implemented"; /* check_input.c:343-347 */
    /* polarvdw: the coupled-dipole term with repulsion-only Lennard-Jones is on the device; the rest is refused by name */
    if (s->cdvdw_exp_repulsion) return "cdvdw_exp_repulsion is not on the device";
    if (s->cdvdw_sig_repulsion) return "cdvdw_sig_repulsion is not on the device";
    if (s->cdvdw_9th_repulsion) return "cdvdw_9th_repulsion is not on the device";
    if (s->polarvdw == 2) return "polarvdw evects (eigenvectors) is not on the device";
    if (s->polarvdw == 3) return "polarvdw comp (two-body comparison) is not on the device";
    if (s->polarvdw && s->feynman_hibbs)
        return "feynman_hibbs with polarvdw is not on the device (the reference's finite-difference correction divides "
               "eigensolver noise by 1e-8 and cannot be matched)";
    if (s->polarvdw && !s->polarization) return "polarvdw without polarization (the reference would read an unbuilt A matrix)";
    if (s->polarvdw && !s->cavity_autoreject_absolute && s->ensemble != ENSEMBLE_REPLAY)
        return "cavity_autoreject_absolute must be used with polarvdw + Feynman Hibbs."; /* check_input.c:216-219 */
    if (s->polarvdw && s->disp_expansion) return "disp_expansion with polarvdw is not on the device";
    if (s->polarvdw && s->rd_crystal) return "rd_crystal with polarvdw is not on the device";
    if (s->polarvdw && s->axilrod_teller) return "axilrod_teller with polarvdw is not on the device";
    /* rd_crystal (Lennard-Jones over lattice images) is on the device up to order 4; disp_expansion() ignores it */
    if (s->rd_crystal && s->disp_expansion) return "rd_crystal with disp_expansion is not on the device";
    if (s->rd_crystal && s->rd_crystal_order > 4) return "rd_crystal_order above 4 is not on the device";
    /* disp_expansion: the default and the Schmidt mixing of the exponent are on the device; the rest is refused by name */
    if (s->disp_expansion_mbvdw) return "disp_expansion_mbvdw (many-body van der Waals) is not on the device";
    if (s->disp_expansion && s->gilbert_smith_mixing) return "gilbert_smith_mixing is not on the device";
    if (s->disp_expansion && s->bohm_ahlrichs_mixing) return "bohm_ahlrichs_mixing is not on the device";
    if (s->disp_expansion && s->wilson_popelier_mixing) return "wilson_popelier_mixing is not on the device";
    return NULL;
}
const char *energy_hip_unsupported(const system_t *system) { return unsupported(system); }

static int hip_fail(const char *what) {
    char buf[2 * MAXLINE];
    snprintf(buf, sizeof(buf), "ENERGY: HIP engine: %s: %s\n", what, mpmc_hip_last_error());
    error(buf);
    return -1;
}

/* every error return of energy_hip_begin() / _end() goes through here: the failure is recorded in its own channel
 * and the notes are dropped -- restore() may free a molecule that is still noted -- so the next energy(), if the
 * caller tries one, walks the lists */
static void drop_volume_notes(shim_state *st) {
    for (int v = 0; v < st->nvol; v++) free(st->vol_delta[v]);
    st->nvol = 0;
}

static int device_failed(shim_state *st) {
    st->failed = 1;
    drop_volume_notes(st);
    st->nnotes = 0;
    st->in_sync = 0;
    return -1;
}

static int image_reserve(shim_state *st, int cap) {
    if (st->cap >= cap) return 0;
    free_image(st);
    for (int c = 0; c < NCOL; c++)
        if (!(st->col[c] = malloc((size_t)cap * sizeof(double)))) return -1;
    st->cap = cap;
    return 0;
}

/* one atom's value in every column of the image */
static void atom_columns(const atom_t *a, double v[NCOL]) {
    v[COL_X] = a->pos[0]; v[COL_Y] = a->pos[1]; v[COL_Z] = a->pos[2];
    v[COL_Q] = a->charge; v[COL_ALPHA] = a->polarizability; v[COL_EPS] = a->epsilon; v[COL_SIG] = a->sigma;
    v[COL_MASS] = a->mass;
    v[COL_C6] = a->c6; v[COL_C8] = a->c8; v[COL_C10] = a->c10; v[COL_C9] = a->c9; v[COL_OMEGA] = a->omega;
}

/* system->pbc->basis, row-major, as the engine takes it */
static void basis_of(const system_t *system, double basis[9]) {
    for (int p = 0; p < 3; p++)
        for (int r = 0; r < 3; r++) basis[3 * p + r] = system->pbc->basis[p][r];
}

static int residents_reserve(shim_state *st, int n) {
    if (st->res_cap >= n) return 0;
    const int cap = 2 * n + 64;
    resident_t *a = realloc(st->res, cap * sizeof(resident_t)), *b = realloc(st->res2, cap * sizeof(resident_t));
    if (a) st->res = a;
    if (b) st->res2 = b;
    if (!a || !b) return -1;
    st->res_cap = cap;
    return 0;
}

/* the molecule list as an array (list position -> node) */
static int list_to_array(shim_state *st, system_t *system) {
    int n = 0;
    for (molecule_t *m = system->molecules; m; m = m->next) n++;
    if (n > st->mols_cap) {
        molecule_t **a = realloc(st->mols, (2 * n + 64) * sizeof(molecule_t *));
        if (!a) return -1;
        st->mols = a;
        st->mols_cap = 2 * n + 64;
    }
    n = 0;
    for (molecule_t *m = system->molecules; m; m = m->next) st->mols[n++] = m;
    return n;
}

static int natoms_of(const molecule_t *m) {
    int k = 0;
    for (const atom_t *a = m->atoms; a; a = a->next) k++;
    return k;
}

/* two moleculetype strings compare equal (what strncmp(a, b, MAXLINE) == 0 says, vdw.c:273) */
static int same_type(const char *a, const char *b) {
    for (int k = 0; k < MAXLINE; k++) {
        if (a[k] != b[k]) return 0;
        if (!a[k]) break;
    }
    return 1;
}

/* The per-atom coefficient mpmc_hip_set_axilrod_teller() and mpmc_hip_edit_molecules() take: c9 as read, or the
 * Midzuno-Kihara replacement (axilrod_teller.cpp:114-118, the same expression left to right). */
double energy_hip_effective_c9(int midzuno_kihara_approx, double alpha, double c6, double c9) {
    return midzuno_kihara_approx ? 3.0 / 4.0 * alpha * 6.7483345 * c6 : c9;
}

/* whole configuration, slots = list order */
static int full_upload(shim_state *st, system_t *system) {
    const int n = system->natoms;
    const int nm = list_to_array(st, system);
    if (nm < 0 || image_reserve(st, st->capacity > n ? st->capacity : n) || residents_reserve(st, nm)) {
        error("ENERGY: HIP engine: out of host memory\n");
        return -1;
    }
    sent_settings_t *sent = &st->sent;
    double *const *col = st->col;
    fill_settings(system, sent);
    /* (in front of the parameters: the exact mode takes a set with neither polar_max_iter nor polar_precision) */
    if (mpmc_hip_set_exact_polar(st->ctx, sent->exact)) return hip_fail("set_exact_polar");
    /* (likewise: under polar_damp_type off the engine takes a set without polar_damp) */
    if (mpmc_hip_set_thole_model(st->ctx, &sent->thole)) return hip_fail("set_thole_model");
    int *mol = malloc((n > 0 ? n : 1) * sizeof(int));
    uint8_t *fz = malloc(n > 0 ? n : 1);
    if (!mol || !fz) {
        free(mol); free(fz);
        error("ENERGY: HIP engine: out of host memory\n");
        return -1;
    }
    int i = 0;
    st->nres = 0;
    st->uploaded = 0; /* until every call below has been taken: a failure half-way leaves nothing to update or edit */
    for (int mi = 0; mi < nm; mi++) {
        molecule_t *m = st->mols[mi];
        const int first = i;
        for (atom_t *a = m->atoms; a; a = a->next, i++) {
            double v[NCOL];
            atom_columns(a, v);
            for (int c = 0; c < NCOL; c++) st->col[c][i] = v[c];
            mol[i] = mi; /* list position: distinct per molecule even if PQR ids repeat */
            fz[i] = (uint8_t)(a->frozen != 0);
        }
        resident_t *r = &st->res[st->nres++];
        r->mol = m; r->atoms = m->atoms; r->slot = first; r->natoms = i - first; r->frozen = (m->frozen != 0);
    }
    double basis[9];
    basis_of(system, basis);
    int rc = mpmc_hip_set_params(st->ctx, &sent->params);
    if (!rc) rc = mpmc_hip_set_box(st->ctx, basis, system->pbc->cutoff);
    if (!rc)
        rc = mpmc_hip_upload(st->ctx, n, col[COL_X], col[COL_Y], col[COL_Z], col[COL_Q], col[COL_ALPHA], col[COL_EPS], col[COL_SIG],
                             col[COL_MASS], mol, fz);
    free(mol); free(fz);
    if (rc) return hip_fail("upload");
    if (mpmc_hip_set_rd_crystal(st->ctx, sent->rdc_order)) return hip_fail("set_rd_crystal");
    if (mpmc_hip_set_rd_form(st->ctx, &sent->rd_form)) return hip_fail("set_rd_form");
    /* (an upload leaves the context on Lennard-Jones: nothing to say unless the PHAHST potential is asked for) */
    if (sent->disp.disp_expansion && mpmc_hip_set_dispersion(st->ctx, &sent->disp, n, col[COL_C6], col[COL_C8], col[COL_C10]))
        return hip_fail("set_dispersion");
    if (sent->axilrod_teller) {
        /* the engine takes the EFFECTIVE per-atom coefficient */
        double *eff = malloc((n > 0 ? n : 1) * sizeof(double));
        if (!eff) {
            error("ENERGY: HIP engine: out of host memory\n");
            return -1;
        }
        for (int k = 0; k < n; k++)
            eff[k] = energy_hip_effective_c9(sent->midzuno_kihara_approx, col[COL_ALPHA][k], col[COL_C6][k], col[COL_C9][k]);
        rc = mpmc_hip_set_axilrod_teller(st->ctx, 1, n, eff);
        free(eff);
        if (rc) return hip_fail("set_axilrod_teller");
    }
    if (sent->vdw_on) {
        /* type ids: the first-seen order of moleculetype, which is what the reference's e_iso list is keyed by
         * (vdw.c:262-320) */
        int *type = malloc((n > 0 ? n : 1) * sizeof(int));
        molecule_t **seen = malloc((nm > 0 ? nm : 1) * sizeof(molecule_t *));
        if (!type || !seen) {
            free(type); free(seen);
            error("ENERGY: HIP engine: out of host memory\n");
            return -1;
        }
        int nseen = 0, k = 0;
        for (int mi = 0; mi < nm; mi++) {
            molecule_t *m = st->mols[mi];
            int t = 0;
            while (t < nseen && !same_type(seen[t]->moleculetype, m->moleculetype)) t++;
            if (t == nseen) seen[nseen++] = m;
            for (atom_t *a = m->atoms; a; a = a->next) type[k++] = t;
        }
        rc = mpmc_hip_set_vdw(st->ctx, 1, n, col[COL_OMEGA], type);
        free(type); free(seen);
        if (rc) return hip_fail("set_vdw");
    }
    if (mpmc_hip_set_autoreject(st->ctx, sent->ar_scale)) return hip_fail("set_autoreject");
    st->uploaded = 1;
    st->in_sync = 1;
    st->nnotes = 0;
    st->sync_counts[0]++;
    drop_volume_notes(st);
    return 0;
}

void energy_hip_note_moved(system_t *system, molecule_t *now, molecule_t *was) {
    shim_state *st = state_of(system, 0);
    if (!st || !st->in_sync) return;
    if (st->nnotes == 8) {
        st->in_sync = 0; /* too many: the next energy() walks the lists */
        return;
    }
    st->notes[st->nnotes].now = now;
    st->notes[st->nnotes].was = was;
    st->nnotes++;
}
void energy_hip_note_list_changed(system_t *system) {
    shim_state *st = state_of(system, 0);
    if (st) st->in_sync = 0;
}
/* volume_change() / revert_volume_change() shifted every molecule rigidly: delta_per_molecule[3 * k + i] is what was
 * added to coordinate i of every atom of the k-th molecule of the list.  The next energy_hip() then scales the box
 * of the resident configuration (mpmc_hip_scale_box) instead of uploading everything again. */
void energy_hip_note_volume_change(system_t *system, const double *delta_per_molecule) {
    shim_state *st = state_of(system, 0);
    if (!st || !st->in_sync) return;
    double *copy = NULL;
    if (!st->vol_notes_off && delta_per_molecule && st->nvol < 4 && st->nres > 0)
        copy = malloc((size_t)st->nres * 3 * sizeof(double));
    if (!copy) {
        st->in_sync = 0; /* the next energy() uploads the whole configuration */
        return;
    }
    memcpy(copy, delta_per_molecule, (size_t)st->nres * 3 * sizeof(double));
    st->vol_delta[st->nvol++] = copy;
}
/* how energy_hip() has kept the device in line so far: full uploads, edit calls that were carried out, molecules they
 * removed + inserted (zeros before the first call) */
void energy_hip_sync_counts(system_t *system, long out[3]) {
    shim_state *st = state_of(system, 0);
    for (int k = 0; k < 3; k++) out[k] = st ? st->sync_counts[k] : 0;
}
int energy_hip_trial_energies(system_t *system, molecule_t *molecule, int ntrial, const double *xyz, double *energy) {
    shim_state *st = state_of(system, 0);
    if (!st || !st->ctx || !st->uploaded) return hip_fail("trial_energies before the first energy()");
    const resident_t *r = NULL;
    for (int k = 0; k < st->nres && !r; k++)
        if (st->res[k].mol == molecule) r = &st->res[k];
    if (!r) return hip_fail("trial_energies: the molecule is not one the device holds");
    ++st->trial_calls;
    if (mpmc_hip_trial_energies(st->ctx, r->slot, r->natoms, ntrial, xyz, energy, NULL)) {
        st->failed = 1;
        return hip_fail("trial_energies");
    }
    return 0;
}
long energy_hip_trial_calls(system_t *system) {
    shim_state *st = state_of(system, 0);
    return st ? st->trial_calls : 0;
}
void energy_hip_set_volume_notes(system_t *system, int on) {
    shim_state *st = state_of(system, 1);
    if (st) st->vol_notes_off = !on;
}

/* Carry out the noted volume moves on the resident configuration: the host image takes the additions the lists
 * took (same operands, same order: the image stays bit-identical to the lists), the device the same through
 * mpmc_hip_scale_box().  Molecules noted as displaced are compared with the image afterwards, so the order in which
 * displacements and volume moves were noted does not matter.  Every call is given the box as it is now: with more
 * than one note pending (mc() never leaves more than a revert and the next change) the earlier calls set up a box
 * that only the last one's matters for -- a lattice sum on the host each, nothing on the device.  Returns 1 when the engine wants the whole
 * configuration again, < 0 on error. */
static int apply_volume_notes(shim_state *st, system_t *system) {
    double basis[9];
    basis_of(system, basis);
    double *x = st->col[COL_X], *y = st->col[COL_Y], *z = st->col[COL_Z];
    for (int v = 0; v < st->nvol; v++) {
        const double *d = st->vol_delta[v];
        const int rc = mpmc_hip_scale_box(st->ctx, basis, system->pbc->cutoff, st->nres, d);
        if (rc < 0) return hip_fail("scale_box");
        if (rc > 0) return 1;
        for (int k = 0; k < st->nres; k++) {
            const int s = st->res[k].slot;
            for (int a = 0; a < st->res[k].natoms; a++) {
                x[s + a] += d[3 * k + 0]; y[s + a] += d[3 * k + 1]; z[s + a] += d[3 * k + 2];
            }
        }
    }
    drop_volume_notes(st);
    return 0;
}

/* does list node m still hold exactly what resident r's slots were last sent? */
static int same_place(const shim_state *st, const molecule_t *m, const resident_t *r) {
    if ((m->frozen != 0) != r->frozen) return 0;
    if (r->frozen) /* never moved (mc_moves.c picks among the others): no comparison of coordinates */
        return m->atoms == r->atoms || natoms_of(m) == r->natoms;
    int k = 0, moved = 0;
    const double *x = st->col[COL_X] + r->slot, *y = st->col[COL_Y] + r->slot, *z = st->col[COL_Z] + r->slot;
    for (const atom_t *a = m->atoms; a; a = a->next, k++) {
        if (k == r->natoms) return 0;
        moved |= (a->pos[0] != x[k]) | (a->pos[1] != y[k]) | (a->pos[2] != z[k]);
    }
    return k == r->natoms && !moved;
}

/* could m be resident r after a displacement (same atoms, site by site)? */
static int same_species(const shim_state *st, const molecule_t *m, const resident_t *r) {
    if ((m->frozen != 0) != r->frozen) return 0;
    int k = 0;
    const int s = r->slot;
    for (const atom_t *a = m->atoms; a; a = a->next, k++) {
        if (k == r->natoms) return 0;
        double v[NCOL];
        atom_columns(a, v);
        for (int c = COL_Q; c < NCOL; c++)
            if (v[c] != st->col[c][s + k]) return 0;
    }
    return k == r->natoms;
}

/* re-send the coordinates of resident r from list node m if they differ */
static int sync_coordinates(shim_state *st, molecule_t *m, resident_t *r) {
    double *x = st->col[COL_X] + r->slot, *y = st->col[COL_Y] + r->slot, *z = st->col[COL_Z] + r->slot;
    int k = 0, moved = 0;
    for (atom_t *a = m->atoms; a; a = a->next, k++) moved |= (a->pos[0] != x[k]) | (a->pos[1] != y[k]) | (a->pos[2] != z[k]);
    r->mol = m;
    r->atoms = m->atoms;
    if (!moved) return 0;
    k = 0;
    for (atom_t *a = m->atoms; a; a = a->next, k++) {
        x[k] = a->pos[0]; y[k] = a->pos[1]; z[k] = a->pos[2];
    }
    if (mpmc_hip_update_atoms(st->ctx, r->slot, k, x, y, z)) return hip_fail("update_atoms");
    return 0;
}

/* The short way: only the molecules mc_moves.c noted.  Returns 1 when a note cannot be placed (the caller then
 * walks the lists), < 0 on error. */
static int sync_noted(shim_state *st) {
    for (int t = 0; t < st->nnotes; t++) {
        molecule_t *was = st->notes[t].was;
        int i = -1;
        if (st->last_found < st->nres && st->res[st->last_found].mol == was)
            i = st->last_found;
        else
            for (int k = 0; k < st->nres; k++)
                if (st->res[k].mol == was) {
                    i = k;
                    break;
                }
        if (i < 0) return 1;
        st->last_found = i;
        molecule_t *now = st->notes[t].now;
        if (natoms_of(now) != st->res[i].natoms) return 1;
        const int rc = sync_coordinates(st, now, &st->res[i]);
        if (rc) {
            st->nnotes = 0; /* never keep a note across an error: the molecule may be freed by restore() */
            st->in_sync = 0;
            return rc;
        }
    }
    st->nnotes = 0;
    return 0;
}

/* What the walk decided: the new resident table (in `out`, n entries in list order) and what has to happen for the device
 * to hold it.  The limits are the engine's: beyond them mpmc_hip_edit_molecules() would answer 1. */
enum { kMol = 8, kAt = 16, kMoved = 16 };
typedef struct {
    int n;
    int ngone, gone[kMol];     /* residents (indices of the old table) whose slots are given up */
    int nfresh, fresh[kMol];   /* entries of the new table that have no slots yet (slot -1) */
    int nmoved, moved[kMoved]; /* entries of the new table whose coordinates differ from the image */
} walk_plan_t;

/* The deciding half of sync_walk(): how the molecule list lines up with the residents, whatever the caller did to the lists
 * since the last call.  No engine call; nothing changes but `out` and `plan`.  The residents (in the list order of the last
 * call) are aligned with the list as it is now, front to back: a node that holds exactly what a resident's slots hold is
 * that resident; otherwise the node is NEW if the node behind it is the resident (a grand-canonical insertion goes in front
 * of the molecule it was copied from, mc_moves.c:626-637), the resident is GONE if the node is the next resident (a removal,
 * or restore() taking an insertion back), in the dense modes the same two one place further on (restore() undoing one trial
 * and make_move() making the next can leave two new nodes or two gone residents side by side, and read as displacements they
 * would shift every molecule behind them by one until the walk gives up), and else the node is the resident DISPLACED if it
 * is the same species site by site.  Only what the device holds matters -- which atoms at which coordinates, and for the
 * Gauss-Seidel solvers in which order -- so "the rejected insertion was taken out and its neighbour displaced" may
 * legitimately be carried out as "the rejected insertion's slots get the neighbour's new coordinates and the neighbour's
 * slots are freed".  Returns 1 when there is no such alignment within the limits. */
static int plan_walk(const shim_state *st, molecule_t *const *mols, int nm, int two_ahead, resident_t *out, walk_plan_t *plan) {
    const resident_t *res = st->res;
    const int nres = st->nres;
    int i = 0, j = 0, n = 0;
    memset(plan, 0, sizeof(*plan));
    while (i < nm || j < nres) {
        enum { KEPT, GONE, FRESH, MOVED } what;
        if (i < nm && j < nres && same_place(st, mols[i], &res[j])) what = KEPT;
        else if (i < nm && j + 1 < nres && same_place(st, mols[i], &res[j + 1])) what = GONE;
        else if (i + 1 < nm && j < nres && same_place(st, mols[i + 1], &res[j])) what = FRESH;
        /* two residents in a row are gone: a rejected insertion taken back and the molecule beside it removed */
        else if (two_ahead && i < nm && j + 2 < nres && same_place(st, mols[i], &res[j + 2])) what = GONE;
        /* two new nodes in a row: a rejected removal put back and an insertion beside it */
        else if (two_ahead && i + 2 < nm && j < nres && same_place(st, mols[i + 2], &res[j])) what = FRESH;
        else if (i < nm && j < nres && same_species(st, mols[i], &res[j])) what = MOVED;
        else if (i == nm) what = GONE;
        else if (j == nres) what = FRESH;
        else return 1;
        if (what == GONE) {
            if (plan->ngone == kMol) return 1;
            plan->gone[plan->ngone++] = j++;
        } else if (what == FRESH) {
            molecule_t *m = mols[i++];
            const resident_t r = {m, m->atoms, -1, natoms_of(m), m->frozen != 0};
            if (plan->nfresh == kMol || r.natoms > kAt) return 1;
            plan->fresh[plan->nfresh++] = n;
            out[n++] = r;
        } else { /* the resident, in this node now */
            if (what == MOVED) {
                if (plan->nmoved == kMoved) return 1;
                plan->moved[plan->nmoved++] = n;
            }
            out[n] = res[j++];
            out[n].atoms = mols[i]->atoms;
            out[n++].mol = mols[i++];
        }
    }
    plan->n = n;
    return 0;
}

/* The removals and insertions of a plan in one call: the engine removes first, so that an insertion of the same size can
 * take the slots, and answers 1 before it has changed anything.  Afterwards the image holds the new molecules in the slots
 * the engine gave them, and `out` knows those slots.  Returns the engine's 1, < 0 on error. */
static int edit_residents(shim_state *st, resident_t *out, const walk_plan_t *plan) {
    double buf[NCOL][kMol][kAt]; /* the new molecules, column by column as read ... */
    double eff_c9[kMol][kAt];    /* ... and the c9 the engine is given in place of buf[COL_C9] */
    mpmc_hip_molecule ins[kMol];
    int rfirst[kMol], rcount[kMol], slot[kMol];
    for (int f = 0; f < plan->ngone; f++) {
        rfirst[f] = st->res[plan->gone[f]].slot;
        rcount[f] = st->res[plan->gone[f]].natoms;
    }
    for (int f = 0; f < plan->nfresh; f++) {
        const resident_t *r = &out[plan->fresh[f]];
        int k = 0;
        for (const atom_t *a = r->mol->atoms; a; a = a->next, k++) {
            double v[NCOL];
            atom_columns(a, v);
            for (int c = 0; c < NCOL; c++) buf[c][f][k] = v[c];
            eff_c9[f][k] = energy_hip_effective_c9(st->sent.midzuno_kihara_approx, v[COL_ALPHA], v[COL_C6], v[COL_C9]);
        }
        mpmc_hip_molecule *m = &ins[f];
        m->count = k; m->frozen = r->frozen;
        m->x = buf[COL_X][f]; m->y = buf[COL_Y][f]; m->z = buf[COL_Z][f]; m->charge = buf[COL_Q][f];
        m->polarizability = buf[COL_ALPHA][f]; m->epsilon = buf[COL_EPS][f]; m->sigma = buf[COL_SIG][f]; m->mass = buf[COL_MASS][f];
        m->c6 = buf[COL_C6][f]; m->c8 = buf[COL_C8][f]; m->c10 = buf[COL_C10][f]; m->c9 = eff_c9[f];
        slot[f] = -1;
    }
    const int rc = mpmc_hip_edit_molecules(st->ctx, plan->ngone, rfirst, rcount, plan->nfresh, ins, slot);
    if (rc < 0) return hip_fail("edit_molecules");
    if (rc > 0) return 1;
    st->sync_counts[1]++;
    st->sync_counts[2] += plan->ngone + plan->nfresh;
    for (int f = 0; f < plan->nfresh; f++) {
        const int s = slot[f], k = ins[f].count;
        if (s < 0 || s + k > st->cap) {
            st->uploaded = 0; /* (cannot happen: the image was reserved for the context's capacity) */
            return 1;
        }
        for (int c = 0; c < NCOL; c++) memcpy(st->col[c] + s, buf[c][f], (size_t)k * sizeof(double));
        out[plan->fresh[f]].slot = s;
    }
    return 0;
}

/* Bring the device in line with the molecule lists without a re-upload: plan_walk() decides, and this carries the plan out --
 * the edit call, the displaced molecules' coordinates, the new resident table, and for the Gauss-Seidel solvers the order.
 * Returns 1 when the engine wants the whole configuration again (no alignment, too many edits, context full,
 * solver mode without incremental edits), < 0 on error. */
static int sync_walk(shim_state *st, system_t *system) {
    const int nm = list_to_array(st, system);
    if (nm < 0 || residents_reserve(st, nm > st->nres ? nm : st->nres)) return 1;
    resident_t *res = st->res, *out = st->res2;
    walk_plan_t plan;
    if (plan_walk(st, st->mols, nm, dense_mode(&st->sent), out, &plan)) return 1;
    const int edited = plan.ngone || plan.nfresh;
    if (edited) {
        const int rc = edit_residents(st, out, &plan);
        if (rc) return rc;
    }
    for (int f = 0; f < plan.nmoved; f++) {
        const int rc = sync_coordinates(st, out[plan.moved[f]].mol, &out[plan.moved[f]]);
        if (rc) return rc;
    }
    st->res = out;
    st->res2 = res;
    st->nres = plan.n;
    int natoms = 0;
    for (int k = 0; k < plan.n; k++) natoms += out[k].natoms;
    if (edited && system->polarization && (system->polar_gs || system->polar_gs_ranked)) {
        /* Gauss-Seidel sweeps walk the atoms in list order (the reference's atom_array, thole_iterative.c:27-59), and the
         * device slots no longer follow the lists: state the order of the polarizable sites */
        int *order = malloc((natoms > 0 ? natoms : 1) * sizeof(int));
        if (!order) return 1;
        int k = 0;
        for (int r = 0; r < plan.n; r++)
            for (int a = 0; a < out[r].natoms; a++)
                if (st->col[COL_ALPHA][out[r].slot + a] != 0.0) order[k++] = out[r].slot + a;
        const int rc = mpmc_hip_set_sweep_order(st->ctx, k, order);
        free(order);
        if (rc) return hip_fail("set_sweep_order");
    }
    system->natoms = natoms; /* energy.c:88 */
    st->in_sync = 1;
    st->nnotes = 0;
    return 0;
}

/* ---- cavity_bias: the grid of the reference's src/mc/cavity.c on the device ---------------------------------------- */

/* a failure of a cavity call: its message, energy()'s failure channel (the next energy_hip() stops the chain), and the
 * table dropped */
static int cavity_failed(shim_state *st, const char *what) {
    if (what) hip_fail(what);
    if (!st) return -1;
    st->failed = 1;
    st->cav_failed = 1;
    st->cav_valid = 0;
    return -1;
}

static int cavity_reserve(shim_state *st, int nmol, int natoms) {
    if (st->cav_cap < nmol) {
        const int cap = 2 * nmol + 64;
        cavity_entry_t *a = realloc(st->cav, cap * sizeof(cavity_entry_t)), *b = realloc(st->cav2, cap * sizeof(cavity_entry_t));
        if (a) st->cav = a;
        if (b) st->cav2 = b;
        if (!a || !b) return -1;
        st->cav_cap = cap;
    }
    if (st->cav_atoms_cap < natoms) {
        const int cap = 2 * natoms + 64;
        double **arr[4] = {&st->cav_raw, &st->cav_raw2, &st->cav_wrapped, &st->cav_wrapped2};
        int bad = 0;
        for (int k = 0; k < 4; k++) { /* (realloc keeps what the live pair holds) */
            double *p = realloc(*arr[k], 3 * (size_t)cap * sizeof(double));
            if (p) *arr[k] = p;
            else bad = 1;
        }
        if (bad) return -1;
        st->cav_atoms_cap = cap;
    }
    return 0;
}

/* wrapped_pos of one molecule as wrapall() leaves it (output.c:142-183): the tree's own function on a list of one */
static void cavity_wrap_one(molecule_t *m, pbc_t *pbc) {
    molecule_t *next = m->next;
    m->next = NULL;
    wrapall(m, pbc);
    m->next = next;
}

/* list node m as entry e with its coordinates at atom offset `first` of raw / wrapped (wrapped_pos must be current) */
static void cavity_record(cavity_entry_t *e, molecule_t *m, int first, double *raw, double *wrapped) {
    int k = first;
    for (atom_t *a = m->atoms; a; a = a->next, k++)
        for (int p = 0; p < 3; p++) {
            raw[3 * k + p] = a->pos[p];
            wrapped[3 * k + p] = a->wrapped_pos[p];
        }
    e->mol = m; e->atoms = m->atoms; e->first = first; e->natoms = k - first; e->frozen = (m->frozen != 0);
}

/* does list node m still hold exactly what entry e was binned from?  (same_place() for this table) */
static int cavity_same(const shim_state *st, const molecule_t *m, const cavity_entry_t *e) {
    if ((m->frozen != 0) != e->frozen) return 0;
    if (e->frozen) return m->atoms == e->atoms || natoms_of(m) == e->natoms;
    int k = 0, moved = 0;
    const double *raw = st->cav_raw + 3 * (size_t)e->first;
    for (const atom_t *a = m->atoms; a; a = a->next, k++) {
        if (k == e->natoms) return 0;
        moved |= (a->pos[0] != raw[3 * k]) | (a->pos[1] != raw[3 * k + 1]) | (a->pos[2] != raw[3 * k + 2]);
    }
    return k == e->natoms && !moved;
}

/* The difference between what was last binned and the list as it is now -- the accepted configuration at the top of
 * make_move() -- as the points that leave (out_xyz) and enter (in_xyz) the occupancy, at most 16 each.  Front to back as
 * sync_walk(): a node that holds what an entry holds is that entry; else the node is new if the node behind it is the
 * entry (an insertion goes in front of the molecule it was copied from), the entry is gone if the node is the next entry,
 * and else the node is the entry displaced.  Only new and displaced molecules are wrapped.  Returns 1 when no such
 * difference can be stated (the caller bins from scratch). */
static int cavity_diff(shim_state *st, system_t *system, double *out_xyz, int *n_out, double *in_xyz, int *n_in) {
    const int nm = list_to_array(st, system);
    if (nm < 0) return 1;
    if (cavity_reserve(st, nm, st->cav_atoms + 16)) return 1; /* (at most 16 atoms enter, or the answer is 1) */
    molecule_t **mols = st->mols;
    cavity_entry_t *old = st->cav, *out = st->cav2;
    int i = 0, j = 0, n2 = 0, at = 0;
    *n_out = *n_in = 0;
    while (i < nm || j < st->ncav) {
        int keep = 0, fresh = 0, gone = 0;
        if (i < nm && j < st->ncav && cavity_same(st, mols[i], &old[j]))
            keep = 1;
        else if (i + 1 < nm && j < st->ncav && cavity_same(st, mols[i + 1], &old[j]))
            fresh = 1;
        else if (i < nm && j + 1 < st->ncav && cavity_same(st, mols[i], &old[j + 1]))
            gone = 1;
        else if (i < nm && j < st->ncav && !old[j].frozen && !mols[i]->frozen && natoms_of(mols[i]) == old[j].natoms)
            fresh = gone = 1; /* displaced: leaves where it was, enters where it is */
        else if (i == nm)
            gone = 1;
        else if (j == st->ncav)
            fresh = 1;
        else
            return 1;
        if (keep) {
            const int n = old[j].natoms;
            memcpy(st->cav_raw2 + 3 * (size_t)at, st->cav_raw + 3 * (size_t)old[j].first, 3 * (size_t)n * sizeof(double));
            memcpy(st->cav_wrapped2 + 3 * (size_t)at, st->cav_wrapped + 3 * (size_t)old[j].first, 3 * (size_t)n * sizeof(double));
            out[n2] = old[j++];
            out[n2].mol = mols[i];
            out[n2].atoms = mols[i++]->atoms;
            out[n2++].first = at;
            at += n;
            continue;
        }
        if (gone) {
            const int n = old[j].natoms;
            if (*n_out + n > 16) return 1;
            memcpy(out_xyz + 3 * *n_out, st->cav_wrapped + 3 * (size_t)old[j].first, 3 * (size_t)n * sizeof(double));
            *n_out += n;
            j++;
        }
        if (fresh) {
            const int n = natoms_of(mols[i]);
            if (*n_in + n > 16 || at + n > st->cav_atoms_cap) return 1;
            cavity_wrap_one(mols[i], system->pbc);
            cavity_record(&out[n2++], mols[i++], at, st->cav_raw2, st->cav_wrapped2);
            memcpy(in_xyz + 3 * *n_in, st->cav_wrapped2 + 3 * (size_t)at, 3 * (size_t)n * sizeof(double));
            *n_in += n;
            at += n;
        }
    }
    st->cav = out; st->cav2 = old;
    double *t = st->cav_raw; st->cav_raw = st->cav_raw2; st->cav_raw2 = t;
    t = st->cav_wrapped; st->cav_wrapped = st->cav_wrapped2; st->cav_wrapped2 = t;
    st->ncav = n2;
    st->cav_atoms = at;
    return 0;
}

/* the from-scratch occupancy: every molecule wrapped (wrapall(), as pairs.c:334 does on every step), recorded, binned */
static int cavity_full_bin(shim_state *st, system_t *system) {
    const int nm = list_to_array(st, system);
    int natoms = 0;
    for (int k = 0; k < nm; k++) natoms += natoms_of(st->mols[k]);
    if (nm < 0 || cavity_reserve(st, nm, natoms)) {
        error("ENERGY: HIP engine: out of host memory\n");
        return cavity_failed(st, NULL);
    }
    wrapall(system->molecules, system->pbc);
    int at = 0;
    for (int k = 0; k < nm; k++) {
        cavity_record(&st->cav[k], st->mols[k], at, st->cav_raw, st->cav_wrapped);
        at += st->cav[k].natoms;
    }
    st->ncav = nm;
    st->cav_atoms = at;
    double *x = malloc(3 * (size_t)(at > 0 ? at : 1) * sizeof(double));
    if (!x) {
        error("ENERGY: HIP engine: out of host memory\n");
        return cavity_failed(st, NULL);
    }
    double *y = x + at, *z = x + 2 * (size_t)at;
    for (int k = 0; k < at; k++) {
        x[k] = st->cav_wrapped[3 * k]; y[k] = st->cav_wrapped[3 * k + 1]; z[k] = st->cav_wrapped[3 * k + 2];
    }
    const int rc = mpmc_hip_cavity_bin(st->ctx, at, x, y, z);
    free(x);
    if (rc) return cavity_failed(st, "cavity_bin");
    st->cav_valid = 1;
    return 0;
}

/* cavity_update_grid() (cavity.c:112-179) for the accepted configuration the lists hold: system->cavities_open,
 * system->cavity_volume and nodestats->cavity_bias_probability.  The darts of cavity_volume() are drawn here with the
 * tree's get_rand(), three per dart, whether or not anything is open, and their positions formed as cavity.c:52-61 does.
 * Before the first energy_hip() there is no device context: the call then takes its draws and nothing else -- mc() makes
 * it once in front of the first energy() (mc.c:245), and nothing reads that call's results.  Returns 0, or -1 after a
 * device / ABI failure, which the next energy_hip() reports in its own channel. */
int energy_hip_cavity_update(system_t *system) {
    shim_state *st = state_of(system, 1);
    const int num_darts = (int)(system->pbc->volume * 0.1); /* DARTSCALE, defines.h:67 */
    const int P = system->cavity_grid_size * system->cavity_grid_size * system->cavity_grid_size;
    if (!st) {
        error("ENERGY: HIP engine: out of host memory\n");
        return -1;
    }
    if (num_darts > st->cav_darts_cap) {
        double *d = realloc(st->cav_darts, 3 * (size_t)num_darts * sizeof(double));
        if (!d) {
            error("ENERGY: HIP engine: out of host memory\n");
            return cavity_failed(st, NULL);
        }
        st->cav_darts = d;
        st->cav_darts_cap = num_darts;
    }
    for (int throw = 0; throw < num_darts; throw++) {
        double grid_vec[3];
        for (int p = 0; p < 3; p++) grid_vec[p] = -0.5 + get_rand(system);
        for (int p = 0; p < 3; p++) {
            double v = system->pbc->basis[0][p] * grid_vec[0];
            v = v + system->pbc->basis[1][p] * grid_vec[1];
            v = v + system->pbc->basis[2][p] * grid_vec[2];
            st->cav_darts[3 * throw + p] = v;
        }
    }
    st->cav_ndarts = num_darts > 0 ? num_darts : 0;
    st->cav_hits = 0;
    system->cavities_open = 0;
    system->cavity_volume = 0;
    system->nodestats->cavity_bias_probability = 0;
    if (!st->ctx) return 0; /* the call in front of the first energy(): the draws only */
    if (st->cav_ctx != st->ctx || st->cav_grid != system->cavity_grid_size || st->cav_radius != system->cavity_radius) {
        if (mpmc_hip_set_cavity_grid(st->ctx, system->cavity_grid_size, system->cavity_radius))
            return cavity_failed(st, "set_cavity_grid");
        st->cav_ctx = st->ctx;
        st->cav_grid = system->cavity_grid_size;
        st->cav_radius = system->cavity_radius;
        st->cav_valid = 0;
    }
    double out_xyz[3 * 16], in_xyz[3 * 16];
    int n_out = 0, n_in = 0, open = 0, hits = 0, rc = 1;
    if (st->cav_valid) rc = cavity_diff(st, system, out_xyz, &n_out, in_xyz, &n_in);
    if (rc == 0) {
        rc = mpmc_hip_cavity_update(st->ctx, n_out, out_xyz, n_in, in_xyz, st->cav_ndarts, st->cav_darts, &open, &hits);
        if (rc < 0) return cavity_failed(st, "cavity_update");
    }
    if (rc > 0) { /* no difference to state, or the engine wants the whole occupancy again (a new box, A/B option) */
        if (cavity_full_bin(st, system)) return -1;
        if (mpmc_hip_cavity_update(st->ctx, 0, NULL, 0, NULL, st->cav_ndarts, st->cav_darts, &open, &hits))
            return cavity_failed(st, "cavity_update");
    }
    st->cav_hits = hits;
    system->cavities_open = open;
    system->nodestats->cavity_bias_probability = ((double)open) / ((double)P); /* cavity.c:103 */
    const double fraction_hits = ((double)hits) / ((double)num_darts);          /* cavity.c:68-69 */
    system->cavity_volume = fraction_hits * system->pbc->volume;
    return 0;
}

/* make_move()'s scan of cavity_grid (mc_moves.c:590-606): the position of the index-th open point of the last
 * energy_hip_cavity_update(), in (i, j, k) order */
int energy_hip_cavity_point(system_t *system, int index, double com[3]) {
    shim_state *st = state_of(system, 0);
    int grid_index = -1;
    com[0] = com[1] = com[2] = 0;
    if (!st || !st->ctx) return cavity_failed(st, NULL);
    if (mpmc_hip_cavity_point(st->ctx, index, &grid_index, com)) return cavity_failed(st, "cavity_point");
    return 0;
}

/* the last energy_hip_cavity_update()'s darts ([n][3], owned by the binding) and how many of them hit; returns n */
int energy_hip_cavity_darts(system_t *system, const double **darts, int *hits) {
    shim_state *st = state_of(system, 0);
    if (darts) *darts = st ? st->cav_darts : NULL;
    if (hits) *hits = st ? st->cav_hits : 0;
    return st ? st->cav_ndarts : 0;
}

/* First half of energy(): bring the device in line with the lists and enqueue the evaluation. */
int energy_hip_begin(system_t *system) {
    const double t0 = now_s();
    shim_state *st = state_of(system, 1);
    if (!st) {
        error("ENERGY: HIP engine: out of host memory\n");
        return -1;
    }
    st->failed = 0;
    if (st->cav_failed) { /* the failure of a cavity grid call is reported here, in energy()'s own channel */
        error("ENERGY: HIP engine: the cavity grid failed on the device\n");
        return device_failed(st);
    }
    const char *why = unsupported(system);
    if (why) {
        char buf[2 * MAXLINE];
        snprintf(buf, sizeof(buf), "ENERGY: HIP engine: %s\n", why);
        error(buf);
        return device_failed(st);
    }
    int need_upload = !st->ctx || !st->uploaded || system->last_volume != system->pbc->volume;
    /* ... unless the box changed by volume moves that were noted: those are carried out on the resident configuration */
    const int scale_box = st->ctx && st->uploaded && st->in_sync && st->nvol > 0;
    if (scale_box) need_upload = 0;
    if (!need_upload) {
        sent_settings_t now;
        fill_settings(system, &now); /* simulated annealing moves the temperature, surface fits the charges ... */
        /* (byte for byte, the doubles too: a cavity_autoreject_scale that goes from 0 to -0 uploads again where != saw no
         * change, and one that is NaN no longer uploads on every call) */
        if (memcmp(&now, &st->sent, sizeof(now))) need_upload = 1;
    }
    if (!need_upload && scale_box) {
        const int rc = apply_volume_notes(st, system);
        if (rc < 0) return device_failed(st);
        need_upload = rc;
    }
    if (!need_upload) {
        static int verify = -1;
        if (verify < 0) verify = getenv("MPMC_HIP_VERIFY_NOTES") != NULL;
        int rc = 1;
        if (st->in_sync) rc = sync_noted(st); /* the noted molecules only */
        if (rc == 0 && verify) {
            /* every difference the walk could find must have been a noted molecule */
            const int nm = list_to_array(st, system);
            int bad = (nm != st->nres);
            for (int k = 0; k < nm && !bad; k++) bad = !same_place(st, st->mols[k], &st->res[k]);
            if (bad) {
                error("ENERGY: HIP engine: a molecule changed without a note (energy_hip_note_moved)\n");
                return device_failed(st);
            }
        }
        if (rc == 1) rc = sync_walk(st, system);
        if (rc < 0) return device_failed(st);
        need_upload = rc;
    }
    if (need_upload) {
        system->natoms = countNatoms(system);
        if (st->ctx && system->natoms > st->capacity) { /* uvt grew past the context */
            mpmc_hip_destroy(st->ctx);
            st->ctx = NULL;
            st->cav_ctx = NULL; /* the cavity grid went with it */
        }
        if (!st->ctx) {
            /* head-room for insertions: a context is sized once, like the reference's pair-list growth steps */
            st->capacity = system->natoms + (system->ensemble == ENSEMBLE_UVT ? system->natoms / 2 + 1024 : 0);
            int device = st->device;
            if (device < 0) {
#ifdef MPMC_SHIM_HOST_MIRROR
                device = 0;
#else
                const int ndev = mpmc_hip_device_count();
                device = ndev > 0 ? rank % ndev : 0; /* one walker per GPU (mc.c's one chain per MPI rank) */
#endif
            }
            if (mpmc_hip_create(&st->ctx, device, st->capacity)) {
                hip_fail("create");
                return device_failed(st);
            }
            st->device = device;
            st->uploaded = 0;
        }
        if (full_upload(st, system)) return device_failed(st);
    }
    const double t1 = now_s();
    if (mpmc_hip_energy_begin(st->ctx)) {
        hip_fail("energy");
        return device_failed(st);
    }
    g_prof[0] += t1 - t0;
    g_prof[1] += now_s() - t1;
    return 0;
}

/* an error return of energy_hip_end() */
static double end_failed(shim_state *st, const char *what) {
    hip_fail(what);
    device_failed(st);
    return NAN;
}

/* Second half: the bookkeeping that does not need the energies runs while the device works, then the result
 * is collected into system->observables. */
double energy_hip_end(system_t *system) {
    shim_state *st = state_of(system, 0);
    if (!st || !st->ctx) return NAN;
    const double t2 = now_s();
    update_com(system->molecules); /* pairs.c:331 */
    countN(system);                /* energy.c:213 */
    const double t3 = now_s();
    mpmc_hip_result r;
    if (mpmc_hip_energy_end(st->ctx, &r)) return end_failed(st, "energy");
    const double t4 = now_s();
    g_prof[2] += t3 - t2; g_prof[3] += t4 - t3;
    if (++g_prof_calls == 64) { /* steady state only: forget the upload and the first steps */
        g_prof[0] = g_prof[1] = g_prof[2] = g_prof[3] = 0.0;
        g_prof_t0 = t4;
        g_prof_base = 64;
    }
    g_prof_tlast = t4;
    if (st->timing) {
        mpmc_hip_timings t;
        if (!mpmc_hip_get_timings(st->ctx, &t)) {
            mpmc_hip_timings *s = &st->tsum;
            s->pair_ms += t.pair_ms; s->recip_ms += t.recip_ms; s->field_ms += t.field_ms;
            s->amatrix_ms += t.amatrix_ms; s->sweep_ms += t.sweep_ms; s->palmo_ms += t.palmo_ms;
            s->other_ms += t.other_ms; s->total_ms += t.total_ms;
            s->sweep_count += t.sweep_count; s->amatrix_count += t.amatrix_count;
            s->event_pair_ms += t.event_pair_ms; s->event_pair_count += t.event_pair_count;
            s->spec_rank_redos = t.spec_rank_redos; /* cumulative in the engine */
            s->resident_calls = t.resident_calls;
            s->resident_fallbacks = t.resident_fallbacks;
            s->pending_sweeps = t.pending_sweeps; /* state of the last evaluation */
        }
    }
    observables_t *o = system->observables;
    if (system->cavity_autoreject_absolute) {
        long long contacts = 0;
        if (mpmc_hip_get_close_contacts(st->ctx, &contacts)) return end_failed(st, "get_close_contacts");
        if (contacts > 0) {
            /* energy.c:99-102, :187-194: a bad contact.  The potential energy is MAXVALUE, the rejection is counted, and
             * the terms of the observables stay what the previous call left (the reference skips their evaluation; here
             * the device evaluated them beside the count and they are dropped) */
            system->count_autorejects++;
            o->energy = MAXVALUE;
            if (o->N > 0.0) o->spin_ratio /= o->N;     /* energy.c:211 */
            o->NU = o->N * o->energy;                  /* energy.c:220 */
            system->last_volume = system->pbc->volume; /* energy.c:223 */
            st->last_energy = o->energy;
            return o->energy;
        }
    }
    o->rd_energy = r.rd_energy;
    o->coulombic_energy = r.coulombic_energy;
    o->polarization_energy = r.polarization_energy;
    o->energy = r.energy;
    o->three_body_energy = 0.0; /* energy.c:148-151, :194: part of o->energy when axilrod_teller is on */
    if (system->axilrod_teller && mpmc_hip_get_three_body_energy(st->ctx, &o->three_body_energy))
        return end_failed(st, "get_three_body_energy");
    /* energy.c:165-177: assigned only while polarvdw is on and rd_only is off; part of o->energy then */
    if (system->polarvdw && !system->rd_only && mpmc_hip_get_vdw_energy(st->ctx, &o->vdw_energy))
        return end_failed(st, "get_vdw_energy");
    o->dipole_rrms = r.dipole_rrms;
    system->nodestats->polarization_iterations = (double)r.polar_iterations;
    if (r.iter_success) system->iter_success = 1; /* thole_iterative.c:207; mc.c:347 resets it */
    if (o->N > 0.0) o->spin_ratio /= o->N;           /* energy.c:214 */
    o->NU = o->N * o->energy;                        /* energy.c:219 */
    system->last_volume = system->pbc->volume;       /* energy.c:222 */
    st->last_energy = o->energy;
    return o->energy;
}

/* `polarizability_tensor on` (polar.c:98-104, thole_polarizability.c): the 3 x 3 molecular tensor of the last energy(),
 * tensor[3 p + q] in A^3, from the device's factor (mpmc_hip_get_polarizability_tensor).  print != 0: the reference's block through
 * output() as well -- header, rules, three %.4f rows, the isotropic term, XX/ZZ.  OWNED DEVIATION: the reference dumps the
 * A and B matrices in front of the block; this layer never forms B and prints neither. */
int energy_hip_polarizability_tensor(system_t *system, double tensor[9], int print) {
    shim_state *st = state_of(system, 0);
    if (!st || !st->ctx) return -1;
    if (mpmc_hip_get_polarizability_tensor(st->ctx, tensor)) return hip_fail("get_polarizability_tensor");
    if (!print) return 0;
    /* (through output(), the tree's writer to stdout, as one block) */
    char buf[2 * MAXLINE];
    snprintf(buf, sizeof(buf),
             "POLARIZATION: polarizability tensor (A^3):\n##########################\n%.4f %.4f %.4f \n%.4f %.4f %.4f \n"
             "%.4f %.4f %.4f \n##########################\nisotropic = %.4f\nXX/ZZ = %.4f\n",
             tensor[0], tensor[1], tensor[2], tensor[3], tensor[4], tensor[5], tensor[6], tensor[7], tensor[8],
             (tensor[0] + tensor[4] + tensor[8]) / 3.0, tensor[0] / tensor[8]);
    output(buf);
    return 0;
}

/* A non-finite return with energy_hip_failed() == 0 is a bad contact, which mc.c treats as a reject
 * (mc.c:315-318); with it set it is a device / ABI failure and the chain must stop. */
double energy_hip(system_t *system) {
    if (energy_hip_begin(system)) return NAN;
    return energy_hip_end(system);
}

int energy_hip_download_dipoles(system_t *system) {
    shim_state *st = state_of(system, 0);
    if (!st || !st->ctx) return -1;
    const int n = mpmc_hip_slot_count(st->ctx); /* device slots, holes included */
    double *buf = malloc(4 * 3 * (size_t)(n > 0 ? n : 1) * sizeof(double));
    if (!buf) return -1;
    double *mu = buf, *es = buf + 3 * n, *ei = buf + 6 * n, *ec = buf + 9 * n;
    if (mpmc_hip_download_dipoles(st->ctx, mu, es, ei, ec)) {
        free(buf);
        return hip_fail("download_dipoles");
    }
    /* residents are in list order and the device is in line with the lists after an energy() */
    int r = 0;
    for (molecule_t *m = system->molecules; m && r < st->nres; m = m->next, r++) {
        int i = st->res[r].slot;
        for (atom_t *a = m->atoms; a; a = a->next, i++)
            for (int p = 0; p < 3; p++) {
                a->mu[p] = mu[3 * i + p];
                a->ef_static[p] = es[3 * i + p];
                a->ef_induced[p] = ei[3 * i + p];
                a->ef_induced_change[p] = ec[3 * i + p];
            }
    }
    free(buf);
    return 0;
}

int energy_hip_corrtime(system_t *system) {
#ifndef MPMC_SHIM_HOST_MIRROR
    wrapall(system->molecules, system->pbc); /* pairs.c:334 does this on every step; only the writers read it */
#endif
    if (system->polarization && !system->rd_only && !system->sg) return energy_hip_download_dipoles(system);
    return 0;
}

/* ---- walker pooling: the MPI_Gather of the reference (mc.c:417-432), over RCCL through the C ABI ------------ */
int walkers_unique_id(unsigned char id[128]) {
    if (mpmc_hip_comm_unique_id(id)) {
        error("MC: could not make a communicator id\n");
        return -1;
    }
    return 0;
}

int walkers_init(system_t *system, int nranks, int rank_, const unsigned char id[128]) {
    shim_state *st = state_of(system, 1);
    if (!st || nranks < 1 || rank_ < 0 || rank_ >= nranks) return -1;
    st->walker_rank = rank_;
    st->walker_nranks = nranks;
    if (nranks == 1 && !id) return 0; /* nothing to pool with (with an id a 1-rank communicator is made: same code path) */
    if (!st->ctx) {
        error("MC: walkers_init needs the device context (call energy() first)\n");
        return -1;
    }
    if (mpmc_hip_comm_create(&st->comm, st->ctx, nranks, rank_, id)) {
        char buf[2 * MAXLINE];
        snprintf(buf, sizeof(buf), "MC: walkers_init: %s\n", mpmc_hip_last_error());
        error(buf);
        return -1;
    }
    return 0;
}

int walkers_init_from_env(system_t *system) {
    const char *sn = getenv("MPMC_HIP_NRANKS"), *sr = getenv("MPMC_HIP_RANK"), *path = getenv("MPMC_HIP_ID_FILE");
    const int nranks = sn ? atoi(sn) : 1, rank_ = sr ? atoi(sr) : 0;
    if (nranks <= 1) return walkers_init(system, 1, 0, NULL);
    if (!path || rank_ < 0 || rank_ >= nranks) {
        error("MC: MPMC_HIP_NRANKS > 1 needs MPMC_HIP_RANK in [0, NRANKS) and MPMC_HIP_ID_FILE\n");
        return -1;
    }
    unsigned char id[128];
    if (rank_ == 0) {
        char tmp[2 * MAXLINE];
        if (walkers_unique_id(id)) return -1;
        snprintf(tmp, sizeof(tmp), "%s.tmp", path);
        FILE *f = fopen(tmp, "wb");
        if (!f || fwrite(id, 1, 128, f) != 128 || fclose(f) || rename(tmp, path)) {
            error("MC: could not publish the communicator id (MPMC_HIP_ID_FILE)\n");
            return -1;
        }
    } else {
        const char *st = getenv("MPMC_HIP_ID_TIMEOUT");
        const double deadline = now_s() + (st ? atof(st) : 120.0);
        size_t got = 0;
        while (got != 128) {
            FILE *f = fopen(path, "rb");
            if (f) {
                got = fread(id, 1, 128, f);
                fclose(f);
            }
            if (got == 128) break;
            if (now_s() > deadline) {
                error("MC: timed out waiting for the communicator id (MPMC_HIP_ID_FILE)\n");
                return -1;
            }
            struct timespec nap = {0, 20 * 1000 * 1000};
            nanosleep(&nap, NULL);
        }
    }
    return walkers_init(system, nranks, rank_, id);
}

int walkers_gather(system_t *system, const void *snd_strct, int msgsize, void *rcv_strct) {
    shim_state *st = state_of(system, 0);
    if (msgsize <= 0) return -1;
    if (!st || !st->comm) { /* a single walker: mc.c:435 */
        memcpy(rcv_strct, snd_strct, msgsize);
        return 0;
    }
    if (mpmc_hip_gather_observables(st->comm, snd_strct, msgsize, rcv_strct)) {
        char buf[2 * MAXLINE];
        snprintf(buf, sizeof(buf), "MC: walkers_gather: %s\n", mpmc_hip_last_error());
        error(buf);
        return -1;
    }
    return 0;
}

int walkers_pool_begin(system_t *system, const double *values, int count) {
    shim_state *st = state_of(system, 1);
    if (!st || count <= 0 || count > 64) return -1;
    if (!st->comm) { /* a single walker: the pooled sums are its own */
        memcpy(st->pool_buf, values, count * sizeof(double));
        return 0;
    }
    return mpmc_hip_allreduce_observables_begin(st->comm, values, count) ? -1 : 0;
}

int walkers_pool_end(system_t *system, double *values, int count) {
    shim_state *st = state_of(system, 0);
    if (!st || count <= 0 || count > 64) return -1;
    if (!st->comm) {
        memcpy(values, st->pool_buf, count * sizeof(double));
        return 0;
    }
    return mpmc_hip_allreduce_observables_end(st->comm, values) ? -1 : 0;
}

void walkers_finalize(system_t *system) {
    shim_state *st = state_of(system, 0);
    if (st && st->comm) mpmc_hip_comm_destroy(st->comm);
    if (st) st->comm = NULL;
}
