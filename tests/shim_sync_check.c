/* How mpmc_amd/host/energy_hip.c keeps the device in line with the molecule lists, on a CPU: this program is compiled together
 * with the binding (-DMPMC_SHIM_HOST_MIRROR) and defines every mpmc_hip_* entry it calls as a stub that appends the call to a
 * textual trace.  The stub engine hands out slots as the engine does (the most recent hole of exactly that size, else the
 * end; place_molecule() in mpmc_amd/csrc/step_plan.h).  Each case drives energy_hip_begin() / energy_hip_end() and the
 * energy_hip_note_*() calls on small lists and holds the trace and energy_hip_sync_counts() to what is written here.  Every
 * case's trace is printed, so two builds of the binding can be compared as text.  Built and run by tests/test_shim_sync.py with
 * -fsanitize=address,undefined; exit status 0 = every check held. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mpmc_host.h"

static int failures = 0;
#define CHECK(cond, ...)                           \
    do {                                           \
        if (!(cond)) {                             \
            ++failures;                            \
            fprintf(stderr, "FAILED %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);          \
            fprintf(stderr, "\n");                 \
            if (failures > 20) exit(1);            \
        }                                          \
    } while (0)

/* ---- the trace ------------------------------------------------------------------------------------------------------ */
static char g_trace[1 << 16];
static size_t g_len;

static void T(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(g_trace + g_len, sizeof(g_trace) - g_len, fmt, ap);
    va_end(ap);
    if (n < 0 || (size_t)n >= sizeof(g_trace) - g_len) {
        fprintf(stderr, "the trace buffer is full\n");
        exit(1);
    }
    g_len += (size_t)n;
}
static void Tv(const char *name, const double *v, int n) {
    T(" %s=", name);
    for (int k = 0; k < n; k++) T(k ? ",%g" : "%g", v[k]);
}
static void Ti(const char *name, const int *v, int n) {
    T(" %s=", name);
    for (int k = 0; k < n; k++) T(k ? ",%d" : "%d", v[k]);
}

/* ---- the recording engine ------------------------------------------------------------------------------------------- */
struct mpmc_hip_ctx {
    int cap, n;                        /* atoms it was created for; slots in use, holes included */
    int nholes, hole[64][2];           /* first slot, count: oldest first */
    int dispersion, axilrod_teller;    /* which per-atom arrays an edit reads */
};
static int g_live_contexts;
static int g_edit_answer, g_scale_answer; /* what the next edit_molecules / scale_box call answers instead of doing its work */
static int g_upload_arrays;               /* the trace of an upload carries the per-atom arrays too */

const char *mpmc_hip_last_error(void) { return "stub"; }
int mpmc_hip_device_count(void) { return 1; }
int mpmc_hip_create(mpmc_hip_ctx **ctx, int device, int max_atoms) {
    T("create device=%d capacity=%d\n", device, max_atoms);
    *ctx = calloc(1, sizeof(**ctx));
    (*ctx)->cap = max_atoms;
    g_live_contexts++;
    return 0;
}
void mpmc_hip_destroy(mpmc_hip_ctx *ctx) {
    T("destroy\n");
    g_live_contexts--;
    free(ctx);
}
void mpmc_hip_default_params(mpmc_hip_params *p) {
    memset(p, 0, sizeof(*p));
    p->rd_lrc = 1;
    p->ewald_kmax = 7;
    p->polar_max_iter = 10;
    p->polar_gamma = 1.0;
}
/* (the members that differ from the defaults above) */
int mpmc_hip_set_params(mpmc_hip_ctx *ctx, const mpmc_hip_params *p) {
    mpmc_hip_params d;
    (void)ctx;
    mpmc_hip_default_params(&d);
    T("set_params");
#define F(name, fmt) \
    if (p->name != d.name) T(" " #name "=" fmt, p->name)
    F(temperature, "%g"); F(rd_only, "%d"); F(rd_lrc, "%d"); F(feynman_hibbs, "%d"); F(feynman_hibbs_order, "%d");
    F(ewald_alpha_set, "%d"); F(ewald_alpha, "%g"); F(ewald_kmax, "%d"); F(polarization, "%d"); F(polar_damp, "%g");
    F(polar_max_iter, "%d"); F(polar_precision, "%g"); F(polar_gamma, "%g"); F(polar_gs, "%d"); F(polar_gs_ranked, "%d");
    F(polar_sor, "%d"); F(polar_esor, "%d"); F(polar_palmo, "%d"); F(polar_rrms, "%d"); F(polar_zodid, "%d");
    F(polar_wolf, "%d"); F(polar_wolf_alpha, "%g"); F(polar_ewald, "%d"); F(polar_ewald_alpha_set, "%d");
    F(polar_ewald_alpha, "%g"); F(wolf, "%d");
#undef F
    T("\n");
    return 0;
}
int mpmc_hip_set_box(mpmc_hip_ctx *ctx, const double basis[9], double pbc_cutoff) {
    (void)ctx;
    T("set_box");
    Tv("basis", basis, 9);
    T(" cutoff=%g\n", pbc_cutoff);
    return 0;
}
int mpmc_hip_scale_box(mpmc_hip_ctx *ctx, const double basis[9], double pbc_cutoff, int n_molecules, const double *delta) {
    (void)ctx;
    T("scale_box");
    if (g_scale_answer) {
        const int a = g_scale_answer;
        g_scale_answer = 0;
        T(" -> %d\n", a);
        return a;
    }
    Tv("basis", basis, 9);
    T(" cutoff=%g n=%d", pbc_cutoff, n_molecules);
    Tv("delta", delta, 3 * n_molecules);
    T("\n");
    return 0;
}
int mpmc_hip_upload(mpmc_hip_ctx *ctx, int n, const double *x, const double *y, const double *z, const double *charge,
                    const double *polarizability, const double *epsilon, const double *sigma, const double *mass,
                    const int *molecule, const uint8_t *frozen) {
    T("upload n=%d", n);
    if (n > ctx->cap) {
        T(" -> -1\n");
        return -1;
    }
    if (g_upload_arrays) {
        int fz[64];
        for (int k = 0; k < n && k < 64; k++) fz[k] = frozen[k];
        Tv("x", x, n); Tv("y", y, n); Tv("z", z, n); Tv("q", charge, n); Tv("alpha", polarizability, n); Tv("eps", epsilon, n);
        Tv("sig", sigma, n); Tv("mass", mass, n); Ti("molecule", molecule, n); Ti("frozen", fz, n < 64 ? n : 64);
    }
    T("\n");
    ctx->n = n;
    ctx->nholes = 0;
    ctx->dispersion = ctx->axilrod_teller = 0;
    return 0;
}
int mpmc_hip_set_dispersion(mpmc_hip_ctx *ctx, const mpmc_hip_disp_params *p, int n, const double *c6, const double *c8,
                            const double *c10) {
    T("set_dispersion %d %d %d %d n=%d", p->disp_expansion, p->damp_dispersion, p->extrapolate_disp_coeffs, p->schmidt_mixing, n);
    if (g_upload_arrays) {
        Tv("c6", c6, n); Tv("c8", c8, n); Tv("c10", c10, n);
    }
    T("\n");
    ctx->dispersion = p->disp_expansion;
    return 0;
}
int mpmc_hip_set_axilrod_teller(mpmc_hip_ctx *ctx, int enable, int n, const double *c9) {
    T("set_axilrod_teller %d n=%d", enable, n);
    Tv("c9", c9, n);
    T("\n");
    ctx->axilrod_teller = enable;
    return 0;
}
int mpmc_hip_set_rd_crystal(mpmc_hip_ctx *ctx, int order) {
    (void)ctx;
    T("set_rd_crystal %d\n", order);
    return 0;
}
int mpmc_hip_set_rd_form(mpmc_hip_ctx *ctx, const mpmc_hip_rd_form_params *p) {
    (void)ctx;
    T("set_rd_form %d %d\n", p->form, p->mixing);
    return 0;
}
int mpmc_hip_set_vdw(mpmc_hip_ctx *ctx, int enable, int n, const double *omega, const int *mol_type) {
    (void)ctx;
    T("set_vdw %d n=%d", enable, n);
    Tv("omega", omega, n);
    Ti("type", mol_type, n);
    T("\n");
    return 0;
}
int mpmc_hip_set_exact_polar(mpmc_hip_ctx *ctx, int enable) {
    (void)ctx;
    T("set_exact_polar %d\n", enable);
    return 0;
}
int mpmc_hip_set_thole_model(mpmc_hip_ctx *ctx, const mpmc_hip_thole_model *m) {
    (void)ctx;
    T("set_thole_model %d %d\n", m->damp_type, m->wolf_full);
    return 0;
}
int mpmc_hip_set_autoreject(mpmc_hip_ctx *ctx, double scale) {
    (void)ctx;
    T("set_autoreject %g\n", scale);
    return 0;
}
int mpmc_hip_update_atoms(mpmc_hip_ctx *ctx, int first, int count, const double *x, const double *y, const double *z) {
    T("update_atoms %d+%d", first, count);
    CHECK(first >= 0 && count > 0 && first + count <= ctx->n, "update_atoms outside the slots in use: %d+%d of %d", first, count, ctx->n);
    Tv("x", x, count); Tv("y", y, count); Tv("z", z, count);
    T("\n");
    return 0;
}
/* all or nothing, as the engine: the answer is decided on a copy */
int mpmc_hip_edit_molecules(mpmc_hip_ctx *ctx, int nremove, const int *remove_first_slot, const int *remove_count, int ninsert,
                            const mpmc_hip_molecule *insert, int *insert_first_slot) {
    T("edit_molecules");
    if (g_edit_answer) {
        const int a = g_edit_answer;
        g_edit_answer = 0;
        T(" -> %d\n", a);
        return a;
    }
    struct mpmc_hip_ctx t = *ctx;
    int slot[8], full = (nremove > 8 || ninsert > 8);
    for (int k = 0; k < nremove && !full; k++) {
        CHECK(remove_first_slot[k] >= 0 && remove_first_slot[k] + remove_count[k] <= t.n, "a removal outside the slots in use");
        if (t.nholes == 64) {
            full = 1;
            break;
        }
        t.hole[t.nholes][0] = remove_first_slot[k];
        t.hole[t.nholes++][1] = remove_count[k];
    }
    for (int k = 0; k < ninsert && !full; k++) {
        const int count = insert[k].count;
        int h = t.nholes - 1;
        while (h >= 0 && t.hole[h][1] != count) h--;
        if (count < 1 || count > 16)
            full = 1;
        else if (h >= 0) {
            slot[k] = t.hole[h][0];
            for (t.nholes--; h < t.nholes; h++) memcpy(t.hole[h], t.hole[h + 1], sizeof(t.hole[h]));
        } else if (t.n + count <= t.cap) {
            slot[k] = t.n;
            t.n += count;
        } else
            full = 1;
    }
    if (full) {
        T(" -> 1\n");
        return 1;
    }
    *ctx = t;
    T(" remove=");
    for (int k = 0; k < nremove; k++) T(k ? ",%d+%d" : "%d+%d", remove_first_slot[k], remove_count[k]);
    T(" insert=%d\n", ninsert);
    for (int k = 0; k < ninsert; k++) {
        const mpmc_hip_molecule *m = &insert[k];
        insert_first_slot[k] = slot[k];
        T("  at %d count=%d frozen=%d", slot[k], m->count, m->frozen);
        Tv("x", m->x, m->count); Tv("y", m->y, m->count); Tv("z", m->z, m->count); Tv("q", m->charge, m->count);
        Tv("alpha", m->polarizability, m->count); Tv("eps", m->epsilon, m->count); Tv("sig", m->sigma, m->count);
        Tv("mass", m->mass, m->count);
        if (ctx->dispersion) {
            Tv("c6", m->c6, m->count); Tv("c8", m->c8, m->count); Tv("c10", m->c10, m->count);
        }
        if (ctx->axilrod_teller) Tv("c9", m->c9, m->count);
        T("\n");
    }
    return 0;
}
int mpmc_hip_set_sweep_order(mpmc_hip_ctx *ctx, int count, const int *slots) {
    (void)ctx;
    T("set_sweep_order");
    Ti("slots", slots, count);
    T("\n");
    return 0;
}
int mpmc_hip_slot_count(mpmc_hip_ctx *ctx) { return ctx->n; }
int mpmc_hip_energy_begin(mpmc_hip_ctx *ctx) {
    (void)ctx;
    T("energy_begin\n");
    return 0;
}
int mpmc_hip_energy_end(mpmc_hip_ctx *ctx, mpmc_hip_result *out) {
    (void)ctx;
    T("energy_end\n");
    memset(out, 0, sizeof(*out));
    out->energy = -1.5;
    return 0;
}
/* the entries the cases here do not reach */
int mpmc_hip_get_timings(mpmc_hip_ctx *ctx, mpmc_hip_timings *t) { (void)ctx; memset(t, 0, sizeof(*t)); return 0; }
int mpmc_hip_get_close_contacts(mpmc_hip_ctx *ctx, long long *count) { (void)ctx; *count = 0; return 0; }
int mpmc_hip_get_three_body_energy(mpmc_hip_ctx *ctx, double *out) { (void)ctx; *out = 0.0; return 0; }
int mpmc_hip_get_vdw_energy(mpmc_hip_ctx *ctx, double *out) { (void)ctx; *out = 0.0; return 0; }
int mpmc_hip_get_polarizability_tensor(mpmc_hip_ctx *ctx, double out[9]) { (void)ctx; memset(out, 0, 9 * sizeof(double)); return 0; }
int mpmc_hip_download_dipoles(mpmc_hip_ctx *ctx, double *mu, double *ef_static, double *ef_induced, double *ef_induced_change) {
    (void)ctx; (void)mu; (void)ef_static; (void)ef_induced; (void)ef_induced_change;
    return -1;
}
int mpmc_hip_trial_energies(mpmc_hip_ctx *ctx, int first_slot, int count, int ntrial, const double *xyz, double *energy,
                            double *terms) {
    (void)ctx; (void)first_slot; (void)count; (void)ntrial; (void)xyz; (void)energy; (void)terms;
    return -1;
}
int mpmc_hip_set_cavity_grid(mpmc_hip_ctx *ctx, int grid_size, double radius) { (void)ctx; (void)grid_size; (void)radius; return -1; }
int mpmc_hip_cavity_bin(mpmc_hip_ctx *ctx, int n, const double *x, const double *y, const double *z) {
    (void)ctx; (void)n; (void)x; (void)y; (void)z;
    return -1;
}
int mpmc_hip_cavity_update(mpmc_hip_ctx *ctx, int n_out, const double *out_xyz, int n_in, const double *in_xyz, int n_darts,
                           const double *dart_xyz, int *cavities_open, int *hits) {
    (void)ctx; (void)n_out; (void)out_xyz; (void)n_in; (void)in_xyz; (void)n_darts; (void)dart_xyz; (void)cavities_open; (void)hits;
    return -1;
}
int mpmc_hip_cavity_point(mpmc_hip_ctx *ctx, int index, int *grid_index, double pos[3]) {
    (void)ctx; (void)index; (void)grid_index; (void)pos;
    return -1;
}
int mpmc_hip_comm_unique_id(unsigned char id[128]) { (void)id; return -1; }
int mpmc_hip_comm_create(mpmc_hip_comm **comm, mpmc_hip_ctx *ctx, int nranks, int rank, const unsigned char id[128]) {
    (void)comm; (void)ctx; (void)nranks; (void)rank; (void)id;
    return -1;
}
void mpmc_hip_comm_destroy(mpmc_hip_comm *comm) { (void)comm; }
int mpmc_hip_gather_observables(mpmc_hip_comm *comm, const void *record, int bytes, void *records) {
    (void)comm; (void)record; (void)bytes; (void)records;
    return -1;
}
int mpmc_hip_allreduce_observables_begin(mpmc_hip_comm *comm, const double *values, int count) {
    (void)comm; (void)values; (void)count;
    return -1;
}
int mpmc_hip_allreduce_observables_end(mpmc_hip_comm *comm, double *values) { (void)comm; (void)values; return -1; }

/* what the binding takes from the tree it is compiled into */
void error(const char *msg) { T("error: %s", msg); }
void output(const char *msg) { (void)msg; }
double get_rand(system_t *system) { (void)system; return 0.5; }
int wrapall(molecule_t *molecules, pbc_t *pbc) { (void)molecules; (void)pbc; return 0; }

/* ---- small lists ---------------------------------------------------------------------------------------------------- */
typedef struct { double q, alpha, eps, sig, mass, c6, c8, c10, c9, omega; } species_t;
static const species_t A = {0.5, 1.5, 10, 3, 2, 6, 8, 10, 9, 0.25};
static const species_t B = {-0.25, 0, 20, 2.5, 4, 16, 18, 110, 19, 0.75}; /* not polarizable */

/* a molecule of n atoms: site k has (k + 1) times the species' values and sits at (x0 + k, x0 / 2, -x0) */
static molecule_t *mol_new(const species_t *sp, int n, double x0) {
    molecule_t *m = calloc(1, sizeof(*m));
    atom_t **tail = &m->atoms;
    snprintf(m->moleculetype, MAXLINE, "%s", sp == &A ? "A" : "B");
    for (int k = 0; k < n; k++) {
        atom_t *a = calloc(1, sizeof(*a));
        const double f = k + 1;
        a->charge = f * sp->q; a->polarizability = f * sp->alpha; a->epsilon = f * sp->eps; a->sigma = f * sp->sig;
        a->mass = f * sp->mass; a->c6 = f * sp->c6; a->c8 = f * sp->c8; a->c10 = f * sp->c10; a->c9 = f * sp->c9;
        a->omega = f * sp->omega;
        a->pos[0] = x0 + k; a->pos[1] = x0 / 2; a->pos[2] = -x0;
        *tail = a;
        tail = &a->next;
    }
    return m;
}
/* copy_molecule(): a deep copy, as checkpoint() keeps and restore() links back in */
static molecule_t *mol_copy(const molecule_t *src) {
    molecule_t *m = malloc(sizeof(*m));
    *m = *src;
    m->next = NULL;
    atom_t **tail = &m->atoms;
    for (const atom_t *a = src->atoms; a; a = a->next) {
        atom_t *c = malloc(sizeof(*c));
        *c = *a;
        c->next = NULL;
        *tail = c;
        tail = &c->next;
    }
    return m;
}
static void mol_free(molecule_t *m) {
    for (atom_t *a = m->atoms, *next; a; a = next) {
        next = a->next;
        free(a);
    }
    free(m);
}
static void mol_shift(molecule_t *m, double dx, double dy, double dz) {
    for (atom_t *a = m->atoms; a; a = a->next) {
        a->pos[0] += dx; a->pos[1] += dy; a->pos[2] += dz;
    }
}
static void mol_freeze(molecule_t *m, int frozen) {
    m->frozen = frozen;
    for (atom_t *a = m->atoms; a; a = a->next) a->frozen = frozen;
}
static molecule_t **list_link(system_t *s, int index) {
    molecule_t **pp = &s->molecules;
    while (index-- > 0 && *pp) pp = &(*pp)->next;
    return pp;
}
static molecule_t *list_at(system_t *s, int index) { return *list_link(s, index); }
static void list_insert(system_t *s, int index, molecule_t *m) {
    molecule_t **pp = list_link(s, index);
    m->next = *pp;
    *pp = m;
}
static molecule_t *list_take(system_t *s, int index) {
    molecule_t **pp = list_link(s, index), *m = *pp;
    *pp = m->next;
    m->next = NULL;
    return m;
}

/* nmol molecules of species A with `natoms` atoms each, molecule i at x0 = 10 i, in a cubic box of 40 A; ensemble uvt, so
 * that the context has head-room */
static system_t *sys_new(int nmol, int natoms) {
    system_t *s = calloc(1, sizeof(*s));
    s->pbc = calloc(1, sizeof(*s->pbc));
    s->observables = calloc(1, sizeof(*s->observables));
    s->nodestats = calloc(1, sizeof(*s->nodestats));
    s->ensemble = ENSEMBLE_UVT;
    s->hip = 1;
    s->temperature = 300.0;
    s->rd_lrc = 1; s->ewald_kmax = 7; s->polar_max_iter = 10; s->polar_gamma = 1.0; s->polar_iterative = 1;
    s->damp_type = DAMPING_EXPONENTIAL;
    for (int p = 0; p < 3; p++) s->pbc->basis[p][p] = 40.0;
    s->pbc->cutoff = 20.0;
    s->pbc->volume = 64000.0;
    for (int i = 0; i < nmol; i++) list_insert(s, i, mol_new(&A, natoms, 10.0 * i));
    return s;
}
static void sys_free(system_t *s) {
    energy_hip_cleanup(s);
    CHECK(!strcmp(g_trace, "destroy\n"), "cleanup:\n%s", g_trace);
    g_len = 0;
    g_trace[0] = 0;
    while (s->molecules) mol_free(list_take(s, 0));
    free(s->pbc); free(s->observables); free(s->nodestats);
    free(s);
}

/* one energy(): 0, or -1 when energy_hip_begin() failed */
static int run(system_t *s) {
    if (energy_hip_begin(s)) return -1;
    const double e = energy_hip_end(s);
    CHECK(e == -1.5 && !energy_hip_failed(s), "energy_hip_end() gave %g", e);
    return 0;
}

/* prints the trace since the last call, holds it to `want` (NULL: printed only) and the sync counts to uploads / edit calls /
 * molecules edited since the system's first call, and starts a new trace */
static void expect(system_t *s, const char *what, const char *want, long uploads, long edits, long edited) {
    long c[3];
    energy_hip_sync_counts(s, c);
    printf("== %s\n%scounts %ld %ld %ld\n", what, g_trace, c[0], c[1], c[2]);
    if (want) CHECK(!strcmp(g_trace, want), "%s: the trace is\n%s-- and not\n%s", what, g_trace, want);
    CHECK(c[0] == uploads && c[1] == edits && c[2] == edited, "%s: sync counts %ld %ld %ld, not %ld %ld %ld", what, c[0], c[1],
          c[2], uploads, edits, edited);
    g_len = 0;
    g_trace[0] = 0;
}
static int traced(const char *what) { return strstr(g_trace, what) != NULL; }
static int count_traced(const char *what) {
    int n = 0;
    for (const char *p = g_trace; (p = strstr(p, what)); p += strlen(what)) n++;
    return n;
}

#define NOTHING "energy_begin\nenergy_end\n"
#define PARAMS "set_params temperature=300 ewald_alpha_set=1 polar_ewald_alpha_set=1\n"
#define BOX "set_box basis=40,0,0,0,40,0,0,0,40 cutoff=20\n"

/* ---- the cases ------------------------------------------------------------------------------------------------------ */

/* the first call: create, then the setters in the one order the engine takes them in */
static void first_call(void) {
    system_t *s = sys_new(3, 2);
    run(s);
    expect(s, "first call, standard path",
           "create device=0 capacity=1033\nset_exact_polar 0\nset_thole_model 2 0\n" PARAMS BOX
           "upload n=6\nset_rd_crystal 0\nset_rd_form 0 0\nset_autoreject 0\n" NOTHING, 1, 0, 0);
    run(s);
    expect(s, "unchanged lists", NOTHING, 1, 0, 0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "unchanged lists, walked", NOTHING, 1, 0, 0);
    sys_free(s);

    /* every optional setter that can stand beside the others, and the arrays an upload carries */
    s = sys_new(0, 0);
    list_insert(s, 0, mol_new(&A, 2, 1.0));
    list_insert(s, 1, mol_new(&B, 1, 5.0));
    mol_freeze(list_at(s, 1), 1);
    s->disp_expansion = s->damp_dispersion = 1;
    s->axilrod_teller = 1;
    s->cavity_autoreject_absolute = 1;
    s->cavity_autoreject_scale = 1.75;
    g_upload_arrays = 1;
    run(s);
    expect(s, "first call, disp_expansion + axilrod_teller + autoreject",
           "create device=0 capacity=1028\nset_exact_polar 0\nset_thole_model 2 0\n" PARAMS BOX
           "upload n=3 x=1,2,5 y=0.5,0.5,2.5 z=-1,-1,-5 q=0.5,1,-0.25 alpha=1.5,3,0 eps=10,20,20 sig=3,6,2.5 mass=2,4,4"
           " molecule=0,0,1 frozen=0,0,1\n"
           "set_rd_crystal 0\nset_rd_form 0 0\nset_dispersion 1 1 0 0 n=3 c6=6,12,16 c8=8,16,18 c10=10,20,110\n"
           "set_axilrod_teller 1 n=3 c9=9,18,19\nset_autoreject 1.75\n" NOTHING, 1, 0, 0);
    sys_free(s);

    s = sys_new(0, 0);
    list_insert(s, 0, mol_new(&A, 1, 1.0));
    list_insert(s, 1, mol_new(&B, 2, 5.0));
    list_insert(s, 2, mol_new(&A, 1, 9.0));
    s->polarization = 1;
    s->polar_damp = 2.5;
    s->polarvdw = 1;
    s->cavity_autoreject_absolute = 1;
    s->cavity_autoreject_scale = 2.0;
    run(s);
    expect(s, "first call, polarvdw",
           "create device=0 capacity=1030\nset_exact_polar 0\nset_thole_model 2 0\n"
           "set_params temperature=300 ewald_alpha_set=1 polarization=1 polar_damp=2.5 polar_ewald_alpha_set=1\n" BOX
           "upload n=4 x=1,5,6,9 y=0.5,2.5,2.5,4.5 z=-1,-5,-5,-9 q=0.5,-0.25,-0.5,0.5 alpha=1.5,0,0,1.5 eps=10,20,40,10"
           " sig=3,2.5,5,3 mass=2,4,8,2 molecule=0,1,1,2 frozen=0,0,0,0\n"
           "set_rd_crystal 0\nset_rd_form 0 0\nset_vdw 1 n=4 omega=0.25,0.75,1.5,0.25 type=0,1,1,0\nset_autoreject 2\n" NOTHING,
           1, 0, 0);
    sys_free(s);
    g_upload_arrays = 0;

    s = sys_new(2, 1);
    s->polarization = 1;
    s->polar_iterative = 0;
    s->damp_type = DAMPING_LINEAR;
    s->rd_crystal = 1;
    s->rd_crystal_order = 3;
    run(s);
    expect(s, "first call, exact dipoles + linear damping + rd_crystal",
           "create device=0 capacity=1027\nset_exact_polar 1\nset_thole_model 1 0\n"
           "set_params temperature=300 ewald_alpha_set=1 polarization=1 polar_ewald_alpha_set=1\n" BOX
           "upload n=2\nset_rd_crystal 3\nset_rd_form 0 0\nset_autoreject 0\n" NOTHING, 1, 0, 0);
    sys_free(s);
}

/* one member of what an upload sends changed: the whole configuration goes again */
static void settings_changes(void) {
    system_t *s = sys_new(2, 2);
    s->polarization = 1;
    long uploads = 0;
    run(s);
    expect(s, "settings: first call", NULL, ++uploads, 0, 0);
#define CHANGED(what, statement)                                                        \
    do {                                                                                \
        statement;                                                                      \
        run(s);                                                                         \
        CHECK(traced("upload n=4") && !traced("create"), "%s: no upload\n%s", what, g_trace); \
        expect(s, "settings: " what, NULL, ++uploads, 0, 0);                            \
        run(s);                                                                         \
        expect(s, "settings: " what ", again", NOTHING, uploads, 0, 0);                 \
    } while (0)
    CHANGED("temperature", s->temperature = 350.0);
    CHANGED("polar_gs", s->polar_gs = 1);
    CHANGED("damp_dispersion", s->damp_dispersion = 1);
    CHANGED("rd_crystal", (s->rd_crystal = 1, s->rd_crystal_order = 2));
    CHANGED("rd_crystal_order", s->rd_crystal_order = 3);
    CHANGED("rd_crystal off", s->rd_crystal = 0);
    CHANGED("c6_mixing", s->c6_mixing = 1);
    CHANGED("dreiding", s->dreiding = 1);
    CHANGED("pair potential off", (s->c6_mixing = 0, s->dreiding = 0));
    CHANGED("polar_damp_type", s->damp_type = DAMPING_LINEAR);
    CHANGED("polar_damp_type back", s->damp_type = DAMPING_EXPONENTIAL);
    CHANGED("polar_wolf_full", s->polar_wolf_full = 1);
    CHANGED("polar_wolf_full off", s->polar_wolf_full = 0);
    CHANGED("cavity_autoreject_absolute", (s->cavity_autoreject_absolute = 1, s->cavity_autoreject_scale = 2.0));
    CHANGED("cavity_autoreject_scale", s->cavity_autoreject_scale = 2.5);
    CHANGED("polarvdw", s->polarvdw = 1);
    CHANGED("polarvdw off", s->polarvdw = 0);
    CHANGED("polar_iterative off", s->polar_iterative = 0);
    CHANGED("polar_iterative", s->polar_iterative = 1);
    CHANGED("axilrod_teller", s->axilrod_teller = 1);
    CHANGED("midzuno_kihara_approx", s->midzuno_kihara_approx = 1);
    CHANGED("axilrod_teller off", s->axilrod_teller = 0);
#undef CHANGED
    sys_free(s);
}

static void displacements(void) {
    system_t *s = sys_new(4, 2);
    run(s);
    expect(s, "displacement: first call", NULL, 1, 0, 0);
    molecule_t *m = list_at(s, 2);
    mol_shift(m, 0.5, 0.25, -1.0);
    energy_hip_note_moved(s, m, m);
    run(s);
    expect(s, "displacement, noted", "update_atoms 4+2 x=20.5,21.5 y=10.25,10.25 z=-21,-21\n" NOTHING, 1, 0, 0);
    /* restore(): the backup is linked in where the altered molecule was, with the coordinates the device was sent */
    molecule_t *backup = mol_copy(m);
    list_insert(s, 2, backup);
    energy_hip_note_moved(s, backup, m);
    mol_free(list_take(s, 3));
    run(s);
    expect(s, "restore()'s relinked backup, unchanged coordinates", NOTHING, 1, 0, 0);
    /* ... and it is the resident now: a note that names it is placed */
    mol_shift(backup, 1.0, 0.0, 0.0);
    energy_hip_note_moved(s, backup, backup);
    run(s);
    expect(s, "displacement of the relinked backup, noted", "update_atoms 4+2 x=21.5,22.5 y=10.25,10.25 z=-21,-21\n" NOTHING, 1, 0, 0);
    /* a trial displaced and taken back with a backup that holds the OLD coordinates: those are sent */
    backup = mol_copy(list_at(s, 1));
    mol_shift(list_at(s, 1), 0.0, 2.0, 0.0);
    energy_hip_note_moved(s, list_at(s, 1), list_at(s, 1));
    run(s);
    expect(s, "trial displacement", "update_atoms 2+2 x=10,11 y=7,7 z=-10,-10\n" NOTHING, 1, 0, 0);
    m = list_take(s, 1);
    list_insert(s, 1, backup);
    energy_hip_note_moved(s, backup, m);
    mol_free(m);
    run(s);
    expect(s, "trial displacement taken back", "update_atoms 2+2 x=10,11 y=5,5 z=-10,-10\n" NOTHING, 1, 0, 0);
    /* not noted: the walk finds it */
    mol_shift(list_at(s, 3), 0.0, 0.0, 3.0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "displacement, found by the walk", "update_atoms 6+2 x=30,31 y=15,15 z=-27,-27\n" NOTHING, 1, 0, 0);
    /* a note that cannot be placed (the molecule is not a resident) hands over to the walk */
    m = list_at(s, 0);
    mol_shift(m, 0.125, 0.0, 0.0);
    static molecule_t stranger;
    energy_hip_note_moved(s, m, &stranger);
    run(s);
    expect(s, "a note that names no resident", "update_atoms 0+2 x=0.125,1.125 y=0,0 z=0,0\n" NOTHING, 1, 0, 0);
    sys_free(s);

    /* more notes than the binding keeps: the walk takes over and sends the same */
    for (int noted = 0; noted < 2; noted++) {
        s = sys_new(10, 1);
        run(s);
        expect(s, "nine displacements: first call", NULL, 1, 0, 0);
        for (int i = 0; i < 9; i++) {
            m = list_at(s, i);
            mol_shift(m, 0.5, 0.0, 0.0);
            if (noted) energy_hip_note_moved(s, m, m);
        }
        if (!noted) energy_hip_note_list_changed(s);
        run(s);
        expect(s, noted ? "nine displacements, noted" : "nine displacements, walked",
               "update_atoms 0+1 x=0.5 y=0 z=0\nupdate_atoms 1+1 x=10.5 y=5 z=-10\nupdate_atoms 2+1 x=20.5 y=10 z=-20\n"
               "update_atoms 3+1 x=30.5 y=15 z=-30\nupdate_atoms 4+1 x=40.5 y=20 z=-40\nupdate_atoms 5+1 x=50.5 y=25 z=-50\n"
               "update_atoms 6+1 x=60.5 y=30 z=-60\nupdate_atoms 7+1 x=70.5 y=35 z=-70\nupdate_atoms 8+1 x=80.5 y=40 z=-80\n" NOTHING,
               1, 0, 0);
        sys_free(s);
    }
}

#define INS_A2(slot, x, y, z) "  at " #slot " count=2 frozen=0 x=" x " y=" y " z=" z " q=0.5,1 alpha=1.5,3 eps=10,20 sig=3,6 mass=2,4"

static void insertions_and_removals(void) {
    system_t *s = sys_new(3, 2);
    run(s);
    expect(s, "edits: first call", NULL, 1, 0, 0);
    /* an insertion goes in front of the molecule it was copied from */
    molecule_t *m = mol_copy(list_at(s, 1));
    mol_shift(m, 3.0, 0.0, 0.0);
    list_insert(s, 1, m);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "insertion", "edit_molecules remove= insert=1\n" INS_A2(6, "13,14", "5,5", "-10,-10") "\n" NOTHING, 1, 1, 1);
    CHECK(s->natoms == 8, "natoms %d", s->natoms);
    /* rejected: restore() takes it out again */
    mol_free(list_take(s, 1));
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "rejected insertion taken back", "edit_molecules remove=6+2 insert=0\n" NOTHING, 1, 2, 2);
    CHECK(s->natoms == 6, "natoms %d", s->natoms);
    /* a removal */
    molecule_t *removed = list_take(s, 0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "removal", "edit_molecules remove=0+2 insert=0\n" NOTHING, 1, 3, 3);
    /* rejected: restore() links the backup in again, and it takes the most recent hole of its size */
    list_insert(s, 0, removed);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "rejected removal put back", "edit_molecules remove= insert=1\n" INS_A2(0, "0,1", "0,0", "-0,-0") "\n" NOTHING, 1, 4, 4);
    /* the image knows where the engine put a molecule: a displacement of an inserted one goes to its slots */
    m = mol_copy(list_at(s, 2));
    mol_shift(m, 0.0, 1.0, 0.0);
    list_insert(s, 2, m);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "insertion into the older hole", "edit_molecules remove= insert=1\n" INS_A2(6, "20,21", "11,11", "-20,-20") "\n" NOTHING, 1,
           5, 5);
    mol_shift(m, 0.0, 0.0, 0.5);
    energy_hip_note_moved(s, m, m);
    run(s);
    expect(s, "displacement of the inserted molecule", "update_atoms 6+2 x=20,21 y=11,11 z=-19.5,-19.5\n" NOTHING, 1, 5, 5);
    /* a removal and an insertion of another size in one walk: one call, and the hole is not taken */
    mol_free(list_take(s, 1));
    list_insert(s, 3, mol_new(&B, 1, 7.0));
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "removal and insertion in one call",
           "edit_molecules remove=2+2 insert=1\n  at 8 count=1 frozen=0 x=7 y=3.5 z=-7 q=-0.25 alpha=0 eps=20 sig=2.5 mass=4\n" NOTHING, 1, 6, 7);
    sys_free(s);
}

/* two new nodes side by side, then two gone residents side by side.  mode 0: the standard path, which does not look two
 * places ahead -- its trace is what the walk has always done there, displacements that shift the molecules behind by one */
static void two_side_by_side(int mode) {
    static const char *const name[5] = {"standard path", "disp_expansion", "axilrod_teller", "rd_crystal", "dreiding"};
    char what[128];
    system_t *s = sys_new(5, 1);
    if (mode == 1) s->disp_expansion = 1;
    if (mode == 2) s->axilrod_teller = 1;
    if (mode == 3) s->rd_crystal = 1, s->rd_crystal_order = 2;
    if (mode == 4) s->dreiding = 1;
    run(s);
    snprintf(what, sizeof(what), "two side by side, %s: first call", name[mode]);
    expect(s, what, NULL, 1, 0, 0);
    list_insert(s, 1, mol_new(&A, 1, 3.0));
    list_insert(s, 2, mol_new(&A, 1, 6.0));
    energy_hip_note_list_changed(s);
    run(s);
    snprintf(what, sizeof(what), "two new nodes side by side, %s", name[mode]);
#define ONE_A(slot, x, y, z) "  at " #slot " count=1 frozen=0 x=" #x " y=" #y " z=" #z " q=0.5 alpha=1.5 eps=10 sig=3 mass=2"
    if (mode == 0)
        expect(s, what,
               "edit_molecules remove= insert=2\n" ONE_A(5, 30, 15, -30) "\n" ONE_A(6, 40, 20, -40) "\n"
               "update_atoms 1+1 x=3 y=1.5 z=-3\nupdate_atoms 2+1 x=6 y=3 z=-6\nupdate_atoms 3+1 x=10 y=5 z=-10\n"
               "update_atoms 4+1 x=20 y=10 z=-20\n" NOTHING, 1, 1, 2);
    else {
        const char *tail = mode == 1 ? " c6=6 c8=8 c10=10\n" : mode == 2 ? " c9=9\n" : "\n";
        char want[1024];
        snprintf(want, sizeof(want), "edit_molecules remove= insert=2\n%s%s%s%s" NOTHING, ONE_A(5, 3, 1.5, -3), tail, ONE_A(6, 6, 3, -6),
                 tail);
        expect(s, what, want, 1, 1, 2);
    }
    mol_free(list_take(s, 3));
    mol_free(list_take(s, 3));
    energy_hip_note_list_changed(s);
    run(s);
    snprintf(what, sizeof(what), "two gone residents side by side, %s", name[mode]);
    if (mode == 0)
        /* the residents in list order sit in slots 0 1 2 3 4 5 6 with x = 0 3 6 10 20 30 40; x = 10 and 20 leave */
        expect(s, what,
               "edit_molecules remove=5+1,6+1 insert=0\nupdate_atoms 3+1 x=30 y=15 z=-30\nupdate_atoms 4+1 x=40 y=20 z=-40\n" NOTHING, 1,
               2, 4);
    else
        expect(s, what, "edit_molecules remove=1+1,2+1 insert=0\n" NOTHING, 1, 2, 4);
    sys_free(s);
}

/* what an insertion carries under disp_expansion + axilrod_teller, and what the image keeps of it */
static void insertion_data(int midzuno_kihara) {
    system_t *s = sys_new(2, 2);
    s->disp_expansion = 1;
    s->axilrod_teller = 1;
    s->midzuno_kihara_approx = midzuno_kihara;
    run(s);
    CHECK(traced(midzuno_kihara ? "set_axilrod_teller 1 n=4 c9=45.5513,182.205,45.5513,182.205\n"
                                : "set_axilrod_teller 1 n=4 c9=9,18,9,18\n"), "the upload's c9:\n%s", g_trace);
    expect(s, midzuno_kihara ? "insertion data, midzuno_kihara_approx: first call" : "insertion data: first call", NULL, 1, 0, 0);
    list_insert(s, 0, mol_new(&A, 2, 4.0));
    energy_hip_note_list_changed(s);
    run(s);
    /* effective c9 under the approximation: 3/4 alpha 6.7483345 c6 = 45.55... and 4 times that for the second site */
    expect(s, midzuno_kihara ? "insertion data, midzuno_kihara_approx" : "insertion data",
           midzuno_kihara ? "edit_molecules remove= insert=1\n" INS_A2(4, "4,5", "2,2", "-4,-4")
                                " c6=6,12 c8=8,16 c10=10,20 c9=45.5513,182.205\n" NOTHING
                          : "edit_molecules remove= insert=1\n" INS_A2(4, "4,5", "2,2", "-4,-4") " c6=6,12 c8=8,16 c10=10,20 c9=9,18\n" NOTHING,
           1, 1, 1);
    /* the image holds c9 as read, not the effective one: the new molecule is found in place */
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "insertion data: unchanged lists afterwards", NOTHING, 1, 1, 1);
    mol_shift(list_at(s, 0), 0.0, 0.0, 1.0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "insertion data: the walk knows the inserted molecule by every column", "update_atoms 4+2 x=4,5 y=2,2 z=-3,-3\n" NOTHING, 1, 1, 1);
    /* ... and every column of it is the molecule's: a node that differs in one of them is no displaced resident.  With the
     * inserted molecule in front, the walk then has nothing to hold on to and the configuration is sent again. */
    for (int column = 0; column < 10; column++) {
        atom_t *a = list_at(s, 0)->atoms->next;
        double *v[10] = {&a->charge, &a->polarizability, &a->epsilon, &a->sigma, &a->mass, &a->c6, &a->c8, &a->c10, &a->c9, &a->omega};
        const double keep = *v[column];
        *v[column] += 1.0;
        a->pos[0] += 0.5;
        energy_hip_note_list_changed(s);
        run(s);
        CHECK(traced("upload n=6") && !traced("update_atoms"), "column %d of the inserted molecule is not compared\n%s", column, g_trace);
        expect(s, "insertion data: another species in its place", NULL, 2 + column, 1 + 2 * column, 1 + 2 * column);
        /* back to the species, from an upload: the edit is made again for the next column */
        *v[column] = keep;
        molecule_t *m = list_take(s, 0);
        energy_hip_note_list_changed(s);
        run(s);
        list_insert(s, 0, m);
        energy_hip_note_list_changed(s);
        run(s);
        expect(s, "insertion data: taken out and put in again", NULL, 2 + column, 3 + 2 * column, 3 + 2 * column);
    }
    sys_free(s);
}

static void gauss_seidel(int ranked) {
    system_t *s = sys_new(0, 0);
    list_insert(s, 0, mol_new(&A, 2, 0.0));
    list_insert(s, 1, mol_new(&B, 1, 10.0));
    list_insert(s, 2, mol_new(&A, 1, 20.0));
    s->polarization = 1;
    if (ranked) s->polar_gs_ranked = 1;
    else s->polar_gs = 1;
    run(s);
    expect(s, "Gauss-Seidel: first call", NULL, 1, 0, 0);
    mol_shift(list_at(s, 2), 1.0, 0.0, 0.0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "Gauss-Seidel: a displacement states no order", "update_atoms 3+1 x=21 y=10 z=-20\n" NOTHING, 1, 0, 0);
    /* slots: A 0 1, B 2, A 3; the new A goes to 4 5 but stands second in the list */
    list_insert(s, 1, mol_new(&A, 2, 5.0));
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "Gauss-Seidel: an insertion states the list order of the polarizable sites",
           "edit_molecules remove= insert=1\n" INS_A2(4, "5,6", "2.5,2.5", "-5,-5") "\nset_sweep_order slots=0,1,4,5,3\n" NOTHING, 1, 1, 1);
    mol_free(list_take(s, 0));
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "Gauss-Seidel: a removal does too", "edit_molecules remove=0+2 insert=0\nset_sweep_order slots=4,5,3\n" NOTHING, 1, 2, 2);
    s->polar_gs = s->polar_gs_ranked = 0;
    run(s);
    expect(s, "Gauss-Seidel off", NULL, 2, 2, 2);
    mol_free(list_take(s, 0));
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "Jacobi: an edit states no order", "edit_molecules remove=0+2 insert=0\n" NOTHING, 2, 3, 3);
    sys_free(s);
}

static void limits(void) {
    system_t *s = sys_new(20, 1);
    run(s);
    expect(s, "limits: first call", NULL, 1, 0, 0);
    for (int k = 0; k < 8; k++) mol_free(list_take(s, 12));
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "8 gone", "edit_molecules remove=12+1,13+1,14+1,15+1,16+1,17+1,18+1,19+1 insert=0\n" NOTHING, 1, 1, 8);
    for (int k = 0; k < 9; k++) mol_free(list_take(s, 3));
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("upload n=3") && !traced("edit_molecules"), "9 gone\n%s", g_trace);
    expect(s, "9 gone", NULL, 2, 1, 8);
    for (int k = 0; k < 8; k++) list_insert(s, 3 + k, mol_new(&A, 1, 100.0 + k));
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("edit_molecules remove= insert=8\n") && !traced("upload"), "8 new\n%s", g_trace);
    expect(s, "8 new", NULL, 2, 2, 16);
    for (int k = 0; k < 9; k++) list_insert(s, 11 + k, mol_new(&A, 1, 200.0 + k));
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("upload n=20") && !traced("edit_molecules"), "9 new\n%s", g_trace);
    expect(s, "9 new", NULL, 3, 2, 16);
    for (int k = 0; k < 16; k++) mol_shift(list_at(s, k), 0.0, 0.5, 0.0);
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(count_traced("update_atoms") == 16 && !traced("upload"), "16 displaced\n%s", g_trace);
    expect(s, "16 displaced", NULL, 3, 2, 16);
    for (int k = 0; k < 17; k++) mol_shift(list_at(s, k), 0.0, 0.5, 0.0);
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("upload n=20") && !traced("update_atoms"), "17 displaced\n%s", g_trace);
    expect(s, "17 displaced", NULL, 4, 2, 16);
    list_insert(s, 20, mol_new(&A, 16, 300.0));
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("edit_molecules remove= insert=1\n  at 20 count=16") && !traced("upload"), "a new molecule of 16 atoms\n%s", g_trace);
    expect(s, "a new molecule of 16 atoms", NULL, 4, 3, 17);
    list_insert(s, 0, mol_new(&A, 17, 400.0));
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("upload n=53") && !traced("edit_molecules"), "a new molecule of 17 atoms\n%s", g_trace);
    expect(s, "a new molecule of 17 atoms", NULL, 5, 3, 17);
    /* the engine wants the whole configuration again */
    mol_free(list_take(s, 5));
    energy_hip_note_list_changed(s);
    g_edit_answer = 1;
    run(s);
    expect(s, "the engine answers 1",
           "edit_molecules -> 1\nset_exact_polar 0\nset_thole_model 2 0\n" PARAMS BOX
           "upload n=52\nset_rd_crystal 0\nset_rd_form 0 0\nset_autoreject 0\n" NOTHING, 6, 3, 17);
    sys_free(s);
}

static void engine_failure(void) {
    system_t *s = sys_new(3, 1);
    run(s);
    expect(s, "failure: first call", NULL, 1, 0, 0);
    mol_free(list_take(s, 1));
    energy_hip_note_list_changed(s);
    g_edit_answer = -1;
    CHECK(energy_hip_begin(s) == -1 && energy_hip_failed(s), "a failed edit must fail the call");
    expect(s, "the engine answers -1", "edit_molecules -> -1\nerror: ENERGY: HIP engine: edit_molecules: stub\n", 1, 0, 0);
    /* the notes are gone with it: a note made now is not taken, and the next call walks and finds the removal itself */
    molecule_t *m = list_at(s, 0);
    energy_hip_note_moved(s, m, m);
    run(s);
    expect(s, "the call after a failure walks", "edit_molecules remove=1+1 insert=0\n" NOTHING, 1, 1, 1);
    /* a failure with notes pending: none of them survives it */
    mol_shift(m, 1.0, 0.0, 0.0);
    energy_hip_note_moved(s, m, m);
    s->polarization = 1;
    s->polar_ewald_full = 1; /* refused by name */
    CHECK(energy_hip_begin(s) == -1 && energy_hip_failed(s), "an unsupported keyword must fail the call");
    expect(s, "a refused keyword", "error: ENERGY: HIP engine: polar_ewald_full is not on the device\n", 1, 1, 1);
    s->polarization = s->polar_ewald_full = 0;
    run(s);
    CHECK(!energy_hip_failed(s), "the failure flag is cleared by the next call");
    expect(s, "the call after a refusal walks", "update_atoms 0+1 x=1 y=0 z=0\n" NOTHING, 1, 1, 1);
    sys_free(s);
}

static void frozen_molecules(void) {
    system_t *s = sys_new(3, 2);
    mol_freeze(list_at(s, 0), 1);
    run(s);
    expect(s, "frozen: first call", NULL, 1, 0, 0);
    /* never compared by coordinates: whatever the list node holds, it is the resident */
    mol_shift(list_at(s, 0), 5.0, 5.0, 5.0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "a frozen molecule is not compared by coordinates", NOTHING, 1, 0, 0);
    molecule_t *m = mol_copy(list_at(s, 0));
    mol_free(list_take(s, 0));
    list_insert(s, 0, m);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "a frozen molecule in another node is the resident by its atom count", NOTHING, 1, 0, 0);
    /* frozen against non-frozen is no match, neither in place nor as a displacement */
    mol_freeze(list_at(s, 0), 0);
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("upload n=6") && !traced("update_atoms"), "frozen against non-frozen\n%s", g_trace);
    expect(s, "a frozen resident against a movable node", NULL, 2, 0, 0);
    mol_freeze(list_at(s, 1), 1);
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("upload n=6") && !traced("update_atoms"), "non-frozen against frozen\n%s", g_trace);
    expect(s, "a movable resident against a frozen node", NULL, 3, 0, 0);
    sys_free(s);
}

static void volume_move(system_t *s, double *delta, double scale) {
    int k = 0;
    for (molecule_t *m = s->molecules; m; m = m->next, k++) {
        delta[3 * k] = scale * (k + 1); delta[3 * k + 1] = -scale; delta[3 * k + 2] = 0.5 * scale;
        mol_shift(m, delta[3 * k], delta[3 * k + 1], delta[3 * k + 2]);
    }
    for (int p = 0; p < 3; p++) s->pbc->basis[p][p] += scale;
    s->pbc->cutoff = s->pbc->basis[0][0] / 2;
    s->pbc->volume = s->pbc->basis[0][0] * s->pbc->basis[1][1] * s->pbc->basis[2][2];
}

static void volume_notes(void) {
    system_t *s = sys_new(3, 2);
    double delta[9];
    s->ensemble = ENSEMBLE_NPT;
    run(s);
    expect(s, "volume: first call", NULL, 1, 0, 0);
    volume_move(s, delta, 2.0);
    energy_hip_note_volume_change(s, delta);
    run(s);
    expect(s, "one noted volume move",
           "scale_box basis=42,0,0,0,42,0,0,0,42 cutoff=21 n=3 delta=2,-2,1,4,-2,1,6,-2,1\n" NOTHING, 1, 0, 0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "the image took the same additions", NOTHING, 1, 0, 0);
    /* a revert and the next change: both carried out, each call given the box as it is now */
    volume_move(s, delta, -2.0);
    energy_hip_note_volume_change(s, delta);
    volume_move(s, delta, 1.0);
    energy_hip_note_volume_change(s, delta);
    molecule_t *m = list_at(s, 1);
    mol_shift(m, 0.0, 0.0, 0.25);
    energy_hip_note_moved(s, m, m);
    run(s);
    expect(s, "two noted volume moves and a displacement",
           "scale_box basis=41,0,0,0,41,0,0,0,41 cutoff=20.5 n=3 delta=-2,2,-1,-4,2,-1,-6,2,-1\n"
           "scale_box basis=41,0,0,0,41,0,0,0,41 cutoff=20.5 n=3 delta=1,-1,0.5,2,-1,0.5,3,-1,0.5\n"
           "update_atoms 2+2 x=12,13 y=4,4 z=-9.25,-9.25\n" NOTHING, 1, 0, 0);
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "the image took both", NOTHING, 1, 0, 0);
    volume_move(s, delta, 1.0);
    energy_hip_note_volume_change(s, delta);
    g_scale_answer = 1;
    run(s);
    CHECK(traced("scale_box -> 1\nset_exact_polar 0\n") && traced("set_box basis=42,0,0,0,42,0,0,0,42 cutoff=21\nupload n=6\n"),
          "scale_box answering 1\n%s", g_trace);
    expect(s, "scale_box answers 1", NULL, 2, 0, 0);
    volume_move(s, delta, 1.0); /* not noted at all */
    run(s);
    CHECK(traced("upload n=6") && !traced("scale_box"), "a volume move without a note\n%s", g_trace);
    expect(s, "a volume move without a note", NULL, 3, 0, 0);
    energy_hip_set_volume_notes(s, 0);
    volume_move(s, delta, 1.0);
    energy_hip_note_volume_change(s, delta);
    run(s);
    CHECK(traced("upload n=6") && !traced("scale_box"), "volume notes switched off\n%s", g_trace);
    expect(s, "volume notes switched off", NULL, 4, 0, 0);
    energy_hip_set_volume_notes(s, 1);
    volume_move(s, delta, 1.0);
    energy_hip_note_volume_change(s, delta);
    run(s);
    CHECK(traced("scale_box basis=45,") && !traced("upload"), "volume notes switched on again\n%s", g_trace);
    expect(s, "volume notes switched on again", NULL, 4, 0, 0);
    sys_free(s);
}

/* a context is made for the atoms of the first call (and head-room under uvt only): one molecule more does not fit */
static void growth(void) {
    system_t *s = sys_new(2, 2);
    s->ensemble = ENSEMBLE_NVT;
    run(s);
    CHECK(traced("create device=0 capacity=4\n"), "the first context\n%s", g_trace);
    expect(s, "growth: first call", NULL, 1, 0, 0);
    list_insert(s, 2, mol_new(&A, 2, 50.0));
    energy_hip_note_list_changed(s);
    run(s);
    expect(s, "growth past the context's capacity",
           "edit_molecules -> 1\ndestroy\ncreate device=0 capacity=6\nset_exact_polar 0\nset_thole_model 2 0\n" PARAMS BOX
           "upload n=6\nset_rd_crystal 0\nset_rd_form 0 0\nset_autoreject 0\n" NOTHING, 2, 0, 0);
    s->ensemble = ENSEMBLE_UVT;
    for (int k = 0; k < 3; k++) list_insert(s, 3 + k, mol_new(&A, 1, 60.0 + k));
    energy_hip_note_list_changed(s);
    run(s);
    CHECK(traced("edit_molecules -> 1\ndestroy\ncreate device=0 capacity=1037\n") && traced("upload n=9"), "uvt growth\n%s", g_trace);
    expect(s, "uvt growth", NULL, 3, 0, 0);
    sys_free(s);
    CHECK(g_live_contexts == 0, "%d contexts left", g_live_contexts);
}

int main(void) {
    first_call();
    displacements();
    insertions_and_removals();
    for (int mode = 0; mode < 5; mode++) two_side_by_side(mode);
    insertion_data(0);
    insertion_data(1);
    gauss_seidel(0);
    gauss_seidel(1);
    limits();
    engine_failure();
    frozen_molecules();
    volume_notes();
    growth();
    settings_changes();
    CHECK(g_live_contexts == 0, "%d contexts left", g_live_contexts);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("every check held\n");
    return 0;
}
