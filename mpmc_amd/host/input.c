/*
 * input.c -- config keywords, PQR geometry and box set-up for the host layer.
 *
 * Follows the reference's formats so its sample inputs run unchanged: flat `keyword value` lines
 * with `!`/`#` comments (reference src/io/input.c:73-1597 -- only the keywords of the hot path are
 * accepted, anything else is an error exactly like an unknown keyword there), whitespace PQR
 * (src/io/read_pqr.c:155-389), box set-up (src/io/simulation_box.c:28-81, src/energy/pbc.c:13-83).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "mpmc_host.h"

void output(const char *msg) {
    fputs(msg, stdout);
    fflush(stdout);
}
void error(const char *msg) {
    fputs(msg, stderr);
    fflush(stderr);
}

static int safe_atof(const char *s, double *out) {
    char *end;
    if (!s || !*s) return 1;
    *out = strtod(s, &end);
    return (*end != 0);
}
static int safe_atoi(const char *s, int *out) {
    char *end;
    if (!s || !*s) return 1;
    *out = (int)strtol(s, &end, 10);
    return (*end != 0);
}
static int on_off(const char *s, int *out) {
    if (!strcasecmp(s, "on")) {
        *out = 1;
        return 0;
    }
    if (!strcasecmp(s, "off")) {
        *out = 0;
        return 0;
    }
    return 1;
}

/* reference setdefaults(), src/io/input.c:1598-1667 */
static void setdefaults(system_t *system) {
    system->scale_charge = 1.0;
    system->rot_factor = 1.0;
    system->move_factor = 1.0;
    system->ewald_alpha = 0.5;
    system->ewald_kmax = 7;
    system->polar_ewald_alpha = 0.5;
    system->polar_gamma = 1.0;
    system->polar_max_iter = 10;
    system->rd_lrc = 1;
    system->wrapall = 1;
    system->hip = 1;
    system->corrtime = 1;
    system->feynman_hibbs_order = 2;
    system->volume_change_factor = 0.25; /* input.c:1608-1611 */
    system->quantum_rotation_level_max = QUANTUM_ROTATION_LEVEL_MAX; /* input.c:1648-1654 */
    system->quantum_rotation_l_max = QUANTUM_ROTATION_L_MAX;
    system->quantum_rotation_sum = QUANTUM_ROTATION_SUM;
    system->spinflip_probability = 0;
    strcpy(system->job_name, "untitled");
}

static system_t *alloc_system(void) {
    system_t *system = calloc(1, sizeof(system_t));
    system->pbc = calloc(1, sizeof(pbc_t));
    system->observables = calloc(1, sizeof(observables_t));
    system->nodestats = calloc(1, sizeof(nodestats_t));
    system->avg_nodestats = calloc(1, sizeof(avg_nodestats_t));
    system->avg_observables = calloc(1, sizeof(avg_observables_t));
    system->checkpoint = calloc(1, sizeof(checkpoint_t));
    system->checkpoint->observables = calloc(1, sizeof(observables_t));
    setdefaults(system);
    return system;
}

/* one keyword line; returns non-zero on an invalid command (reference do_command, input.c:73) */
int do_command(system_t *system, char **token) {
    const char *k = token[0], *v = token[1];
    if (!k[0] || k[0] == '!' || k[0] == '#') return 0; /* comment / blank, input.c:76-85 */
#define FLAG(name, field) \
    if (!strcasecmp(k, name)) return on_off(v, &system->field)
#define REAL(name, field) \
    if (!strcasecmp(k, name)) return safe_atof(v, &system->field)
#define INT(name, field) \
    if (!strcasecmp(k, name)) return safe_atoi(v, &system->field)
#define TEXT(name, field)                         \
    if (!strcasecmp(k, name)) {                   \
        if (!v[0]) return 1;                      \
        strncpy(system->field, v, MAXLINE - 1);   \
        return 0;                                 \
    }
    if (!strcasecmp(k, "ensemble")) {
        if (!strcasecmp(v, "nvt"))
            system->ensemble = ENSEMBLE_NVT;
        else if (!strcasecmp(v, "uvt"))
            system->ensemble = ENSEMBLE_UVT;
        else if (!strcasecmp(v, "npt"))
            system->ensemble = ENSEMBLE_NPT;
        else if (!strcasecmp(v, "total_energy"))
            system->ensemble = ENSEMBLE_TE;
        else if (!strcasecmp(v, "replay"))
            system->ensemble = ENSEMBLE_REPLAY;
        else if (!strcasecmp(v, "surf"))
            system->ensemble = ENSEMBLE_SURF;
        else if (!strcasecmp(v, "surf_fit")) {
            error("INPUT: ensemble surf_fit is not implemented by this host layer\n");
            return 1;
        } else if (!strcasecmp(v, "nve")) {
            error("INPUT: ensemble nve is not implemented by this host layer\n");
            return 1;
        } else {
            error("INPUT: only `ensemble nvt`, `uvt`, `npt`, `total_energy`, `replay` and `surf` are implemented by this "
                  "host layer\n");
            return 1;
        }
        return 0;
    }
    /* ensemble surf, input.c:170-335 */
    REAL("surf_min", surf_min);
    REAL("surf_max", surf_max);
    REAL("surf_inc", surf_inc);
    REAL("surf_ang", surf_ang);
    FLAG("surf_preserve", surf_preserve);
    FLAG("surf_decomp", surf_decomp);
    FLAG("surf_global_axis", surf_global_axis_on);
    FLAG("surf_virial", surf_virial);          /* refused by name (check_system) */
    INT("surf_print_level", surf_print_level); /* likewise */
    if (!strcasecmp(k, "surf_output")) {       /* likewise */
        system->surf_output_on = 1;
        return 0;
    }
    if (!strcasecmp(k, "surf_preserve_rotation")) {
        if (system->surf_preserve_rotation_on) {
            error("INPUT: surf_preserve_rotationalready set.\n");
            return 1;
        }
        system->surf_preserve_rotation_on = 1;
        for (int i = 0; i < 6; i++)
            if (safe_atof(token[1 + i], &system->surf_preserve_rotation[i])) return 1;
        return 0;
    }
    if (!strcasecmp(k, "preset_seeds")) {
        int s;
        if (safe_atoi(v, &s)) {
            char *end;
            unsigned long u = strtoul(v, &end, 10);
            if (*end) return 1;
            s = (int)u;
        }
        system->preset_seeds = (unsigned int)s;
        system->preset_seeds_on = 1;
        return 0;
    }
    INT("numsteps", numsteps);
    INT("corrtime", corrtime);
    REAL("move_factor", move_factor);
    REAL("rot_factor", rot_factor);
    if (!strcasecmp(k, "move_probability")) { /* input.c:606-615: the deprecated names, still in the sample inputs */
        output("WARNING: move_probability is deprecated, use move_factor instead\n");
        return safe_atof(v, &system->move_factor);
    }
    if (!strcasecmp(k, "rot_probability")) {
        output("WARNING: rot_probability is deprecated, use rot_factor instead\n");
        return safe_atof(v, &system->rot_factor);
    }
    REAL("temperature", temperature);
    REAL("scale_charge", scale_charge);
    REAL("insert_probability", insert_probability);
    REAL("pressure", pressure);
    REAL("volume_probability", volume_probability);
    REAL("volume_change_factor", volume_change_factor);
    if (!strcasecmp(k, "user_fugacities")) {
        system->user_fugacities = 1;
        return safe_atof(v, &system->fugacity);
    }
    if (!strcasecmp(k, "h2_fugacity") || !strcasecmp(k, "co2_fugacity") || !strcasecmp(k, "ch4_fugacity") ||
        !strcasecmp(k, "n2_fugacity")) {
        int on = 0;
        if (on_off(v, &on)) return 1;
        if (on && system->ensemble == ENSEMBLE_UVT)
            error("INPUT: equation-of-state fugacities are not part of this host layer; the pressure (or "
                  "user_fugacities) is used as the fugacity\n");
        return 0;
    }
    FLAG("rd_only", rd_only);
    FLAG("wolf", wolf);
    FLAG("rd_lrc", rd_lrc);
    FLAG("feynman_hibbs", feynman_hibbs);
    FLAG("disp_expansion", disp_expansion); /* input.c:944-1058 */
    FLAG("extrapolate_disp_coeffs", extrapolate_disp_coeffs);
    FLAG("damp_dispersion", damp_dispersion);
    FLAG("schmidt_mixing", schmidt_mixing);
    FLAG("axilrod_teller", axilrod_teller); /* input.c:992-1013 */
    FLAG("midzuno_kihara_approx", midzuno_kihara_approx);
    FLAG("rd_crystal", rd_crystal); /* input.c:814-826 */
    FLAG("sg", sg);                 /* input.c:884-941, :1064-1073 */
    FLAG("dreiding", dreiding);
    FLAG("lj_buffered_14_7", lj_buffered_14_7);
    FLAG("waldmanhagler", waldmanhagler);
    FLAG("halgren_mixing", halgren_mixing);
    FLAG("c6_mixing", c6_mixing);
    if (!strcasecmp(k, "polarvdw") || !strcasecmp(k, "cdvdw")) { /* input.c:446-475 */
        if (!strcasecmp(v, "off")) {
            system->polarvdw = 0;
            return 0;
        }
        if (!strcasecmp(v, "on"))
            system->polarvdw = 1;
        else if (!strcasecmp(v, "evects"))
            system->polarvdw = 2; /* refused by energy_hip.c, by name */
        else if (!strcasecmp(v, "comp"))
            system->polarvdw = 3; /* likewise */
        else
            return 1;
        system->polarization = 1;
        system->polar_iterative = 1;
        output("INPUT: Forcing polar_iterative ON for CP-VdW.\n");
        return 0;
    }
    FLAG("cdvdw_9th_repulsion", cdvdw_9th_repulsion); /* these three are refused by energy_hip.c, each by name */
    FLAG("cdvdw_exp_repulsion", cdvdw_exp_repulsion);
    FLAG("cdvdw_sig_repulsion", cdvdw_sig_repulsion);
    FLAG("cavity_autoreject_absolute", cavity_autoreject_absolute); /* input.c:413-427 */
    REAL("cavity_autoreject_scale", cavity_autoreject_scale);
    FLAG("cavity_bias", cavity_bias); /* input.c:397-412 */
    INT("cavity_grid", cavity_grid_size);
    REAL("cavity_radius", cavity_radius);
    INT("rd_crystal_order", rd_crystal_order);
    FLAG("read_pqr_box", read_pqr_box_on); /* input.c:1448-1455 */
    FLAG("calc_pressure", calc_pressure);  /* input.c:575-582; refused by name in replay (check_system) */
    FLAG("disp_expansion_mbvdw", disp_expansion_mbvdw); /* these four are refused by energy_hip.c, each by name */
    FLAG("gilbert_smith_mixing", gilbert_smith_mixing);
    FLAG("bohm_ahlrichs_mixing", bohm_ahlrichs_mixing);
    FLAG("wilson_popelier_mixing", wilson_popelier_mixing);
    INT("feynman_hibbs_order", feynman_hibbs_order);
    FLAG("wrapall", wrapall);
    if (!strcasecmp(k, "ewald_alpha")) {
        system->ewald_alpha_set = 1;
        return safe_atof(v, &system->ewald_alpha);
    }
    INT("ewald_kmax", ewald_kmax);
    if (!strcasecmp(k, "pbc_cutoff")) return safe_atof(v, &system->pbc->cutoff);
    FLAG("polarization", polarization);
    FLAG("polar_iterative", polar_iterative);             /* input.c:1146-1153; off: the exact dipoles */
    FLAG("polarizability_tensor", polarizability_tensor); /* input.c:1126-1133 */
    FLAG("polar_ewald", polar_ewald);
    if (!strcasecmp(k, "polar_ewald_alpha")) {
        system->polar_ewald_alpha_set = 1;
        return safe_atof(v, &system->polar_ewald_alpha);
    }
    FLAG("polar_zodid", polar_zodid);
    FLAG("polar_palmo", polar_palmo);
    FLAG("polar_gs", polar_gs);
    FLAG("polar_gs_ranked", polar_gs_ranked);
    FLAG("polar_sor", polar_sor);
    FLAG("polar_esor", polar_esor);
    FLAG("polar_rrms", polar_rrms);
    FLAG("polar_wolf", polar_wolf);
    REAL("polar_wolf_alpha", polar_wolf_alpha);
    REAL("polar_wolf_damp", polar_wolf_alpha);
    REAL("polar_gamma", polar_gamma);
    REAL("polar_damp", polar_damp);
    REAL("polar_precision", polar_precision);
    INT("polar_max_iter", polar_max_iter);
    if (!strcasecmp(k, "polar_damp_type")) {
        /* input.c:1217-1232; an absent keyword leaves DAMPING_OFF, as there */
        if (!strcasecmp(v, "none") || !strcasecmp(v, "off"))
            system->damp_type = DAMPING_OFF;
        else if (!strcasecmp(v, "linear"))
            system->damp_type = DAMPING_LINEAR;
        else if (!strcasecmp(v, "exponential"))
            system->damp_type = DAMPING_EXPONENTIAL;
        else
            return 1;
        return 0;
    }
    FLAG("polar_wolf_full", polar_wolf_full);   /* input.c:530-538 */
    FLAG("polar_ewald_full", polar_ewald_full); /* input.c:508-516; refused by energy_hip.c, by name */
    /* quantum_rotation, input.c:1271-1304 and :632 */
    FLAG("quantum_rotation", quantum_rotation);
    FLAG("quantum_rotation_hindered", quantum_rotation_hindered);
    FLAG("quantum_rotation_eigenvectors", quantum_rotation_eigenvectors); /* (this layer's: print the eigenvectors too) */
    REAL("quantum_rotation_hindered_barrier", quantum_rotation_hindered_barrier);
    REAL("quantum_rotation_B", quantum_rotation_B);
    INT("quantum_rotation_level_max", quantum_rotation_level_max);
    INT("quantum_rotation_l_max", quantum_rotation_l_max);
    INT("quantum_rotation_sum", quantum_rotation_sum);
    REAL("spinflip_probability", spinflip_probability);
    FLAG("cuda", cuda);
    FLAG("hip", hip);
    TEXT("job_name", job_name);
    TEXT("pqr_input", pqr_input);
    TEXT("traj_input", traj_input);
    TEXT("pqr_output", pqr_output);
    TEXT("pqr_restart", pqr_restart);
    TEXT("energy_output", energy_output);
    if (!strcasecmp(k, "basis1") || !strcasecmp(k, "basis2") || !strcasecmp(k, "basis3")) {
        const int r = k[5] - '1';
        return safe_atof(token[1], &system->pbc->basis[r][0]) || safe_atof(token[2], &system->pbc->basis[r][1]) ||
               safe_atof(token[3], &system->pbc->basis[r][2]);
    }
    /* keywords of the reference that do not touch the NVT energy path are accepted and ignored */
    {
        static const char *ignored[] = {"free_volume",
                                        "traj_output",   "dipole_output",  "field_output",
                                        "pop_histogram",      "pop_histogram_output", "histogram_output", NULL};
        for (int i = 0; ignored[i]; i++)
            if (!strcasecmp(k, ignored[i])) return 0;
    }
    return 1;
#undef FLAG
#undef REAL
#undef INT
#undef TEXT
}

/* reference read_config(), src/io/input.c:1669-1737 */
system_t *read_config(char *input_file) {
    char linebuffer[MAXLINE], errormsg[2 * MAXLINE];
    char tok[10][MAXLINE], *token[10];
    int linenum = 0;
    FILE *fp = fopen(input_file, "r");
    if (!fp) {
        snprintf(errormsg, sizeof(errormsg), "INPUT: could not open %s\n", input_file);
        error(errormsg);
        return NULL;
    }
    system_t *system = alloc_system();
    for (int i = 0; i < 10; i++) token[i] = tok[i];
    while (fgets(linebuffer, MAXLINE, fp)) {
        linenum++;
        for (int i = 0; i < 10; i++) tok[i][0] = 0;
        sscanf(linebuffer, "%s %s %s %s %s %s %s %s %s %s", tok[0], tok[1], tok[2], tok[3], tok[4], tok[5], tok[6],
               tok[7], tok[8], tok[9]);
        if (do_command(system, token) != 0) {
            snprintf(errormsg, sizeof(errormsg), "INPUT: invalid command on line %d.\n> %s\n", linenum, linebuffer);
            error(errormsg);
            fclose(fp);
            free_system(system);
            return NULL;
        }
    }
    fclose(fp);
    return system;
}

/* reference read_molecules(), src/io/read_pqr.c:155-389 */
molecule_t *read_molecules(FILE *fp, system_t *system) {
    char linebuf[MAXLINE];
    char t[20][MAXLINE];
    molecule_t *molecules = NULL, *molecule_ptr = NULL;
    atom_t *atom_tail = NULL;
    int atom_counter = 0, moveable = 0;
    while (fgets(linebuf, MAXLINE, fp)) {
        for (int i = 0; i < 20; i++) t[i][0] = 0;
        sscanf(linebuf, "%s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s", t[0], t[1], t[2], t[3], t[4],
               t[5], t[6], t[7], t[8], t[9], t[10], t[11], t[12], t[13], t[14], t[15], t[16], t[17], t[18], t[19]);
        if (!strncasecmp(t[0], "END", 3)) break;
        if (strcasecmp(t[0], "ATOM") || !strcasecmp(t[3], "BOX")) continue;
        const int frozen = !strcasecmp(t[4], "F");
        const int molid = atoi(t[5]);
        if (!molecule_ptr || molecule_ptr->id != molid) {
            molecule_t *m = calloc(1, sizeof(molecule_t));
            if (molecule_ptr)
                molecule_ptr->next = m;
            else
                molecules = m;
            molecule_ptr = m;
            atom_tail = NULL;
        }
        strncpy(molecule_ptr->moleculetype, t[3], MAXLINE - 1);
        molecule_ptr->id = molid;
        molecule_ptr->frozen = frozen;
        atom_t *a = calloc(1, sizeof(atom_t));
        a->id = ++atom_counter;
        a->bond_id = atoi(t[1]);
        strncpy(a->atomtype, t[2], MAXLINE - 1);
        a->frozen = frozen;
        a->pos[0] = atof(t[6]);
        a->pos[1] = atof(t[7]);
        a->pos[2] = atof(t[8]);
        a->mass = atof(t[9]);
        a->charge = atof(t[10]) * E2REDUCED; /* read_pqr.c:249 */
        if (frozen) a->charge *= system->scale_charge;
        a->polarizability = atof(t[11]);
        a->epsilon = atof(t[12]);
        a->sigma = atof(t[13]);
        if (system->polarvdw && !system->cdvdw_exp_repulsion && a->sigma != 1.0) { /* read_pqr.c:266-271 */
            error("warning: setting sigma to 1.0 (due to polarvdw)\n");
            a->sigma = 1.0;
        }
        /* t[14]: omega in atomic units (polarvdw); t[15]: gwp_alpha (not used here); then c6, c8, c10 and c9 in atomic
         * units (read_pqr.c:216, :253-258); absent columns read as 0 */
        a->omega = atof(t[14]);
        a->c6 = atof(t[16]);
        a->c8 = atof(t[17]);
        a->c10 = atof(t[18]);
        a->c9 = atof(t[19]);
        molecule_ptr->mass += a->mass;
        if (atom_tail)
            atom_tail->next = a;
        else
            molecule_ptr->atoms = a;
        atom_tail = a;
    }
    for (molecule_ptr = molecules; molecule_ptr; molecule_ptr = molecule_ptr->next)
        if (!molecule_ptr->frozen) ++moveable;
    if (!atom_counter) return NULL;
    if (!moveable) {
        error("INPUT: no moveable molecules found, there must be at least one in your PQR file\n");
        return NULL;
    }
    return molecules;
}

/* reference pbc(), src/energy/pbc.c:66-83 (volume, cutoff, ewald alphas, reciprocal basis) */
void pbc(system_t *system) {
    pbc_t *p = system->pbc;
    double (*b)[3] = p->basis, (*rb)[3] = p->reciprocal_basis;
    double vol = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1]);
    vol += b[0][1] * (b[1][2] * b[2][0] - b[1][0] * b[2][2]);
    vol += b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0]);
    p->volume = vol;
    if (p->cutoff == 0.) {
        double short_mag = MAXVALUE;
        if (vol > 0)
            for (int i = -5; i <= 5; i++)
                for (int j = -5; j <= 5; j++)
                    for (int k = -5; k <= 5; k++) {
                        double v[3];
                        if (!i && !j && !k) continue;
                        for (int q = 0; q < 3; q++) v[q] = i * b[0][q] + j * b[1][q] + k * b[2][q];
                        double mag = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                        if (mag < short_mag) short_mag = mag;
                    }
        p->cutoff = (vol > 0) ? 0.5 * short_mag : MAXVALUE;
    }
    if (system->ewald_alpha_set != 1) system->ewald_alpha = 3.5 / p->cutoff;
    if (system->polar_ewald_alpha_set != 1) system->polar_ewald_alpha = 3.5 / p->cutoff;
    const double iv = 1.0 / vol;
    rb[0][0] = iv * (b[1][1] * b[2][2] - b[1][2] * b[2][1]);
    rb[0][1] = iv * (b[0][2] * b[2][1] - b[0][1] * b[2][2]);
    rb[0][2] = iv * (b[0][1] * b[1][2] - b[0][2] * b[1][1]);
    rb[1][0] = iv * (b[1][2] * b[2][0] - b[1][0] * b[2][2]);
    rb[1][1] = iv * (b[0][0] * b[2][2] - b[0][2] * b[2][0]);
    rb[1][2] = iv * (b[0][2] * b[1][0] - b[0][0] * b[1][2]);
    rb[2][0] = iv * (b[1][0] * b[2][1] - b[1][1] * b[2][0]);
    rb[2][1] = iv * (b[0][1] * b[2][0] - b[0][0] * b[2][1]);
    rb[2][2] = iv * (b[0][0] * b[1][1] - b[0][1] * b[1][0]);
}

/* cavity_bias (check_input.c:880-892), shared with host_apply_config().  Outside `ensemble uvt` the reference would only
 * burn random numbers on the grid, and the device grid holds at most 64^3 points: both are refused by name. */
int check_cavity_bias(system_t *system) {
    char linebuf[MAXLINE];
    if (!system->cavity_bias) return 0;
    if ((system->cavity_grid_size <= 0) || (system->cavity_radius <= 0.0)) {
        error("INPUT: invalid cavity grid or radius specified\n");
        return -1;
    }
    if (system->ensemble != ENSEMBLE_UVT) {
        error("INPUT: cavity_bias needs ensemble uvt (it biases insertions and removals only)\n");
        return -1;
    }
    if (system->cavity_grid_size > 64) {
        error("INPUT: cavity_grid above 64 is not on the device\n");
        return -1;
    }
    output("INPUT: cavity-biased umbrella sampling activated\n");
    snprintf(linebuf, MAXLINE, "INPUT: cavity grid size is %dx%dx%d points with a sphere radius of %.3f A\n",
             system->cavity_grid_size, system->cavity_grid_size, system->cavity_grid_size, system->cavity_radius);
    output(linebuf);
    return 0;
}

/* ensemble_surf_options(), check_input.c:88-132, and what this layer's surface() does not run */
static int check_surf(system_t *system) {
    char linebuf[MAXLINE];
    if (!system->surf_min) system->surf_min = 0.5; /* SURF_MIN, SURF_MAX, SURF_INC: defines.h:144-146 */
    if (!system->surf_max) system->surf_max = 25.0;
    if (!system->surf_inc) system->surf_inc = 0.25;
    if (system->surf_max < system->surf_min) {
        error("INPUT: surf_max is greater than surf_min\n");
        return -1;
    }
    snprintf(linebuf, MAXLINE, "INPUT: minimum surface coordinate is %.3f\n", system->surf_min);
    output(linebuf);
    snprintf(linebuf, MAXLINE, "INPUT: maximum surface coordinate is %.3f\n", system->surf_max);
    output(linebuf);
    if (system->surf_inc <= 0.0) {
        error("INPUT: surf_inc is less than or equal to 0\n");
        return -1;
    }
    snprintf(linebuf, MAXLINE, "INPUT: incremental surface displacement coordinate is %.3f\n", system->surf_inc);
    output(linebuf);
    if (!system->surf_preserve && !system->surf_virial) {
        if (system->surf_ang <= 0.0) {
            error("INPUT: surf_ang is less than or equal to 0\n");
            return -1;
        }
        snprintf(linebuf, MAXLINE, "INPUT: incremental surface angle coordinate is %.3f\n", system->surf_ang);
        output(linebuf);
    }
    if (system->read_pqr_box_on) {
        error("INPUT: read_pqr_box is not compatible with surf.\n");
        return -1;
    }
    const char *why = surface_refused(system);
    if (why) {
        snprintf(linebuf, MAXLINE, "INPUT: ensemble surf: %s\n", why);
        error(linebuf);
        return -1;
    }
    return 0;
}

/* the checks of reference src/io/check_input.c that concern this path */
static int check_system(system_t *system) {
    char linebuf[MAXLINE];
    if (!system->hip) {
        error("INPUT: `hip off` requested but this host layer has no CPU energy path\n");
        return -1;
    }
    if (system->ensemble != ENSEMBLE_NVT && system->ensemble != ENSEMBLE_TE && system->ensemble != ENSEMBLE_UVT &&
        system->ensemble != ENSEMBLE_NPT && system->ensemble != ENSEMBLE_REPLAY && system->ensemble != ENSEMBLE_SURF) {
        error("INPUT: ensemble must be nvt, uvt, npt, total_energy, replay or surf\n");
        return -1;
    }
    if (system->ensemble == ENSEMBLE_SURF && check_surf(system)) return -1;
    if (system->ensemble == ENSEMBLE_REPLAY && !system->traj_input[0]) {
        error("INPUT: ensemble replay needs traj_input\n");
        return -1;
    }
    if (system->ensemble == ENSEMBLE_REPLAY && system->calc_pressure) {
        error("INPUT: calc_pressure in ensemble replay is not implemented by this host layer\n");
        return -1;
    }
    if (system->rd_crystal) { /* check_input.c:1258-1267 */
        if (system->rd_crystal_order <= 0) {
            error("INPUT: rd_crystal_order must be a positive integer\n");
            return -1;
        }
        snprintf(linebuf, MAXLINE, "INPUT: rd crystal order set to %d.\n", system->rd_crystal_order);
        output(linebuf);
    }
    /* check_input.c:1269-1287 */
    if (system->sg) output("INPUT: Molecular potential is Silvera-Goldman\n");
    if (system->waldmanhagler) output("INPUT: Using Waldman-Hagler mixing rules for LJ-interactions.\n");
    if (system->halgren_mixing) output("INPUT: Using Halgren mixing rules for LJ-interactions.\n");
    if (system->c6_mixing) output("INPUT: Using C6 mixing rules for LJ-interactions.\n");
    if ((system->waldmanhagler && system->halgren_mixing) || (system->waldmanhagler && system->c6_mixing) ||
        (system->halgren_mixing && system->c6_mixing)) {
        error("INPUT: more than one mixing rule specified\n");
        return -1;
    }
    if (system->dreiding) output("INPUT: Molecular potential is DREIDING\n");
    if (system->lj_buffered_14_7) output("INPUT: Molecular potential is lj_buffered_14_7\n");
    if (system->polarvdw && !system->cavity_autoreject_absolute && system->ensemble != ENSEMBLE_REPLAY) {
        error("INPUT: cavity_autoreject_absolute must be used with polarvdw + Feynman Hibbs.\n"); /* check_input.c:216-221 */
        return -1;
    }
    if (system->polarvdw) output("INPUT: polarvdw (coupled-dipole van der Waals) activated\n"); /* check_input.c:495-497 */
    if (system->cavity_autoreject_absolute) { /* check_input.c:872-878 */
        output("INPUT: cavity autoreject absolute activated\n");
        if ((system->cavity_autoreject_scale <= 0.0) || (system->cavity_autoreject_scale > 1.78)) {
            error("INPUT: cavity_autoreject_scale either not set or out of range\n");
            return -1;
        }
    }
    if (check_cavity_bias(system)) return -1;
    if (qrot_check(system)) return -1;
    if (system->ensemble == ENSEMBLE_NPT && !(system->pressure > 0.0)) { /* check_input.c:673-678 */
        error("INPUT: invalid pressure set for NPT\n");
        return -1;
    }
    if (system->ensemble == ENSEMBLE_UVT && !system->user_fugacities) system->fugacity = system->pressure;
    if (system->ensemble == ENSEMBLE_UVT && !(system->fugacity > 0.0)) {
        error("INPUT: uvt needs a pressure (or user_fugacities) > 0\n");
        return -1;
    }
    if (system->polarization) {
        if (system->polar_iterative && system->polarizability_tensor) { /* check_input.c:343-347 */
            error("INPUT: iterative polarizability tensor method not implemented\n");
            return -1;
        }
        if (!system->polar_iterative && system->polar_zodid) { /* check_input.c:349-353 */
            error("INPUT: ZODID and matrix inversion cannot both be set!\n");
            return -1;
        }
        if (!system->polar_iterative) { /* check_input.c:486-492 */
            output("INPUT: Matrix polarization activated\n");
            if (system->polarizability_tensor) output("INPUT: Polarizability tensor calculation activated\n");
        }
        if (system->polar_wolf_full) output("INPUT: Full polar wolf treatment activated.\n"); /* check_input.c:359-361 */
        /* check_input.c:391-409 */
        if (system->damp_type == DAMPING_LINEAR)
            output("INPUT: Thole linear damping activated\n");
        else if (system->damp_type == DAMPING_OFF)
            output("INPUT: Thole linear damping is OFF\n");
        else if (system->damp_type != DAMPING_EXPONENTIAL) {
            error("INPUT: Thole damping method not specified\n");
            return -1;
        }
        if (system->polar_damp <= 0.0 && system->damp_type != DAMPING_OFF) {
            error("INPUT: damping factor must be specified\n");
            return -1;
        }
        if ((system->polar_precision > 0.0) && (system->polar_max_iter > 0)) { /* check_input.c:424-428 */
            error("INPUT: cannot specify both polar_precision and polar_max_iter, must pick one\n");
            return -1;
        }
    }
    if (system->ensemble == ENSEMBLE_SURF) return 0; /* no basis is required: a zero volume gives cutoff = MAXVALUE (pbc.c:19) */
    if ((system->pbc->volume <= 0.0) || (system->pbc->cutoff <= 0.0)) {
        error("INPUT: invalid simulation box dimensions.\n");
        return -1;
    }
    snprintf(linebuf, MAXLINE, "INPUT: unit cell volume = %.3f A^3 (cutoff = %.3f A)\n", system->pbc->volume,
             system->pbc->cutoff);
    output(linebuf);
    return 0;
}

/* reference setup_system(), src/io/input.c:1739-1837 */
system_t *setup_system(char *input_file) {
    system_t *system = read_config(input_file);
    if (!system) return NULL;
    if (!system->pqr_input[0]) snprintf(system->pqr_input, MAXLINE, "%s.initial.pqr", system->job_name);
    /* pqr_input / traj_input are relative to the directory of the input file, like running the reference in that directory;
     * ensemble replay takes its first configuration from the trajectory (input.c:1762-1768) */
    const int replay = (system->ensemble == ENSEMBLE_REPLAY);
    char *name = replay ? system->traj_input : system->pqr_input;
    char path[2 * MAXLINE];
    const char *slash = strrchr(input_file, '/');
    if (slash && name[0] != '/')
        snprintf(path, sizeof(path), "%.*s/%s", (int)(slash - input_file), input_file, name);
    else
        snprintf(path, sizeof(path), "%s", name);
    FILE *fp = fopen(path, "r");
    if (!fp) {
        char msg[3 * MAXLINE];
        snprintf(msg, sizeof(msg), "INPUT: could not open %s %s\n", replay ? "traj_input" : "pqr_input", path);
        error(msg);
        free_system(system);
        return NULL;
    }
    if (replay) {
        if (strlen(path) >= MAXLINE) {
            error("INPUT: traj_input path too long\n");
            fclose(fp);
            free_system(system);
            return NULL;
        }
        memmove(system->traj_input, path, strlen(path) + 1); /* replay_trajectory() opens it again */
        if (read_frame(fp, system) != 0) system->molecules = NULL;
    } else
        system->molecules = read_molecules(fp, system);
    fclose(fp);
    if (!system->molecules) {
        error("INPUT: error reading in input molecules\n");
        free_system(system);
        return NULL;
    }
    pbc(system);
    if (check_system(system)) {
        free_system(system);
        return NULL;
    }
    system->natoms = countNatoms(system);
    return system;
}

system_t *system_from_arrays(int n, const double *pos, const double *charge, const double *polarizability,
                             const double *epsilon, const double *sigma, const double *mass, const int *molecule,
                             const int *frozen, const double basis[9]) {
    system_t *system = alloc_system();
    molecule_t *molecule_ptr = NULL;
    atom_t *atom_tail = NULL;
    system->ensemble = ENSEMBLE_NVT;
    for (int i = 0; i < n; i++) {
        if (!molecule_ptr || molecule[i] != molecule_ptr->id) {
            molecule_t *m = calloc(1, sizeof(molecule_t));
            if (molecule_ptr)
                molecule_ptr->next = m;
            else
                system->molecules = m;
            molecule_ptr = m;
            m->id = molecule[i];
            m->frozen = frozen[i];
            atom_tail = NULL;
        }
        atom_t *a = calloc(1, sizeof(atom_t));
        a->id = i + 1;
        a->frozen = frozen[i];
        for (int p = 0; p < 3; p++) a->pos[p] = pos[3 * i + p];
        a->mass = mass[i];
        a->charge = charge[i];
        a->polarizability = polarizability[i];
        a->epsilon = epsilon[i];
        a->sigma = sigma[i];
        molecule_ptr->mass += a->mass;
        if (atom_tail)
            atom_tail->next = a;
        else
            molecule_ptr->atoms = a;
        atom_tail = a;
    }
    for (int p = 0; p < 3; p++)
        for (int q = 0; q < 3; q++) system->pbc->basis[p][q] = basis[3 * p + q];
    system->natoms = n;
    return system;
}

void free_system(system_t *system) {
    if (!system) return;
    energy_hip_profile_report();
    energy_hip_cleanup(system); /* communicator, device context, host image */
    free(system->movable);
    free(system->movable_prev);
    molecule_t *m = system->molecules;
    while (m) {
        atom_t *a = m->atoms;
        while (a) {
            atom_t *an = a->next;
            free(a);
            a = an;
        }
        molecule_t *mn = m->next;
        free(m);
        m = mn;
    }
    if (system->fp_energy) fclose(system->fp_energy);
    free(system->pbc);
    free(system->observables);
    free(system->nodestats);
    free(system->avg_nodestats);
    free(system->avg_observables);
    if (system->checkpoint) {
        if (system->checkpoint->molecule_backup) free_molecule(system, system->checkpoint->molecule_backup);
        free(system->checkpoint->observables);
        free(system->checkpoint);
    }
    free(system);
}

/* PQR writer in the reference's column layout (src/io/output.c:write_molecules) */
int write_molecules(system_t *system, const char *filename) {
    FILE *fp = fopen(filename, "w");
    if (!fp) return -1;
    int i = 1, j = 1;
    /* molecules are numbered in list order (output.c:356-391), not by the id they were read with: an inserted molecule is a
     * copy of its neighbour in the list, id included, and a reader starts a new molecule only where the id changes */
    for (molecule_t *m = system->molecules; m; m = m->next, j++)
        for (atom_t *a = m->atoms; a; a = a->next, i++)
            /* omega (written only while polarvdw is on: every other run's file stays what it was) and gwp_alpha (not held
             * here: 0), then c6 c8 c10 c9, as output.c:436-447 writes them: a restart from this file keeps the dispersion
             * coefficients of a disp_expansion / axilrod_teller run and the frequencies of a polarvdw run */
            fprintf(fp, "ATOM  %5d %-4.45s %-3.3s %-1.1s %4d   %8.3f%8.3f%8.3f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f "
                        "%8.5f %8.5f %8.5f\n", i,
                    a->atomtype[0] ? a->atomtype : "X", m->moleculetype[0] ? m->moleculetype : "M",
                    m->frozen ? "F" : "M", j, a->pos[0], a->pos[1], a->pos[2], a->mass, a->charge / E2REDUCED,
                    a->polarizability, a->epsilon, a->sigma, system->polarvdw ? a->omega : 0.0, 0.0, a->c6, a->c8, a->c10,
                    a->c9);
    fprintf(fp, "END\n");
    fclose(fp);
    return 0;
}

/* The restart file of the reference (output.c:315-564; mc.c:392 rewrites it at every corrtime, the driver writes the one
 * that stays: the state after the last step).  Unlike write_molecules() above it numbers the molecules in list order -- an
 * inserted molecule is a copy of the one behind it, id included, and read_molecules() starts a molecule where the id
 * changes -- and writes what wrapall() makes of the coordinates (pairs.c:331-334 leaves them so after every energy()).
 * The box follows as the reference's REMARK lines; its CRYST1 line and the eight BOX marker atoms, which a reader skips,
 * are not written. */
int write_restart(system_t *system, const char *filename) {
    FILE *fp = fopen(filename, "w");
    if (!fp) return -1;
    const pbc_t *p = system->pbc;
    int ext_output = 0; /* output.c:326-335: %8.3f unless a basis component needs more room */
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            if (p->basis[i][j] >= 100.0) ext_output = 1;
    update_com(system->molecules);
    wrapall(system->molecules, system->pbc);
    int i = 1, j = 1;
    for (molecule_t *m = system->molecules; m; m = m->next, j++)
        for (atom_t *a = m->atoms; a; a = a->next, i++) {
            const double *x = system->wrapall ? a->wrapped_pos : a->pos;
            fprintf(fp, "ATOM  %5d %-4.45s %-3.3s %-1.1s %4d   ", i, a->atomtype[0] ? a->atomtype : "X",
                    m->moleculetype[0] ? m->moleculetype : "M", a->frozen ? "F" : "M", j);
            if (ext_output)
                fprintf(fp, "%11.6f %11.6f %11.6f ", x[0], x[1], x[2]);
            else
                fprintf(fp, "%8.3f%8.3f%8.3f", x[0], x[1], x[2]);
            fprintf(fp, " %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f %8.5f\n", a->mass,
                    a->charge / E2REDUCED, a->polarizability, a->epsilon, a->sigma, a->omega, 0.0, a->c6, a->c8, a->c10,
                    a->c9);
        }
    for (int k = 0; k < 3; k++)
        fprintf(fp, "REMARK BOX BASIS[%d] = %20.14f %20.14f %20.14f\n", k, p->basis[k][0], p->basis[k][1], p->basis[k][2]);
    fprintf(fp, "END\n");
    fclose(fp);
    return 0;
}
