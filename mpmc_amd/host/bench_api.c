/* bench_api.c -- flat entry points over the host layer for ctypes callers (bench.py, tests). */
#include <stdlib.h>
#include <string.h>

#include <math.h>
#include "mpmc_host.h"


/* apply keyword lines ("polar_max_iter 4\npolar_gs on\n...") to a system built from arrays */
int host_apply_config(system_t *system, const char *text) {
    char line[MAXLINE], tok[10][MAXLINE], *token[10];
    for (int i = 0; i < 10; i++) token[i] = tok[i];
    system->polar_iterative = 1; /* a system built from arrays iterates unless the text says `polar_iterative off` */
    system->damp_type = DAMPING_EXPONENTIAL; /* ... and has the exponential tensor unless the text names another */
    const char *p = text;
    while (*p) {
        size_t len = strcspn(p, "\n");
        if (len >= MAXLINE) return 1;
        memcpy(line, p, len);
        line[len] = 0;
        p += len + (p[len] == '\n');
        for (int i = 0; i < 10; i++) tok[i][0] = 0;
        sscanf(line, "%s %s %s %s %s %s %s %s %s %s", tok[0], tok[1], tok[2], tok[3], tok[4], tok[5], tok[6], tok[7],
               tok[8], tok[9]);
        if (do_command(system, token)) return 1;
    }
    pbc(system);
    if (system->ensemble == ENSEMBLE_UVT && !system->user_fugacities) system->fugacity = system->pressure;
    if (system->ensemble == ENSEMBLE_UVT && !(system->fugacity > 0.0)) return 1;
    if (system->ensemble == ENSEMBLE_NPT && !(system->pressure > 0.0)) return 1; /* check_input.c:673-678 */
    if (system->rd_crystal && system->rd_crystal_order <= 0) return 1;            /* check_input.c:1258-1263 */
    if (system->waldmanhagler + system->halgren_mixing + system->c6_mixing > 1) return 1; /* check_input.c:1277-1281 */
    if (system->cavity_autoreject_absolute &&                                     /* check_input.c:872-878 */
        ((system->cavity_autoreject_scale <= 0.0) || (system->cavity_autoreject_scale > 1.78)))
        return 1;
    if (check_cavity_bias(system)) return 1; /* check_input.c:880-892 */
    if (qrot_check(system)) return 1;        /* check_input.c:236-280 */
    return 0;
}

/* quantum_rotation: one evaluation for every movable molecule (0, or -1); the levels, symmetries and the three partition
 * functions (g, u, the molecule's own) of the index-th movable molecule as the last evaluation left them, and the nuclear
 * spin of that molecule: returns the number of levels (quantum_rotation_level_max), -1 when there is no such molecule; counters: [0] trial-energy calls of the binding, [1] accepted and [2] rejected spin-flip moves */
int host_qrot_evaluate(system_t *system) { return quantum_system_rotational_energies(system); }
int host_qrot_levels(system_t *system, int index, double *levels, int *symmetry, double partfunc[3], int *nuclear_spin) {
    int k = 0;
    for (molecule_t *m = system->molecules; m; m = m->next) {
        if (m->frozen) continue;
        if (k++ != index) continue;
        for (int i = 0; i < system->quantum_rotation_level_max; i++) {
            levels[i] = m->quantum_rotational_energies[i];
            symmetry[i] = m->quantum_rotational_eigensymmetry[i];
        }
        partfunc[0] = m->rot_partfunc_g;
        partfunc[1] = m->rot_partfunc_u;
        partfunc[2] = m->rot_partfunc;
        *nuclear_spin = m->nuclear_spin;
        return system->quantum_rotation_level_max;
    }
    return -1;
}
double host_get_spin_ratio(system_t *system) { return system->observables->spin_ratio; }
double host_last_energy(system_t *system) { return energy_hip_last_energy(system); }
/* the 256 grid placements of the index-th movable molecule, xyz [256][n][3]; returns n (-1: no such molecule) */
int host_qrot_placements(system_t *system, int index, double *xyz) {
    int k = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        if (!m->frozen && k++ == index) return qrot_placements(m, xyz);
    return -1;
}
void host_qrot_times(double out[3]) { qrot_last_times(out); }
void host_qrot_counts(system_t *system, long out[3]) {
    out[0] = energy_hip_trial_calls(system);
    out[1] = system->nodestats->accept_spinflip;
    out[2] = system->nodestats->reject_spinflip;
}
int host_last_movetype(system_t *system) { return system->checkpoint->movetype; }

/* what mc() does behind every step's accept / reject for one walker: the running means of the node statistics
 * (mc.c:362) and, at every corrtime, their average over the walkers -- here the one (mc.c:438, :470) */
static void step_statistics(system_t *system) {
    update_nodestats(system->nodestats, system->avg_nodestats);
    if (system->corrtime > 0 && !(system->step % system->corrtime)) {
        clear_avg_nodestats(system);
        update_root_nodestats(system, system->avg_nodestats, system->avg_observables);
    }
}

/* run `nsteps` more MC steps on an initialised chain; returns accepted count */
int host_mc_steps(system_t *system, int nsteps) {
    int acc0 = system->nodestats->accept;
    if (system->step == 0 && system->avg_observables->counter == 0.0) {
        /* first call: initial energy + first checkpoint, as mc() does */
        system->observables->volume = system->pbc->volume;
        if (system->cavity_bias) energy_hip_cavity_update(system); /* mc.c:245: the draws of its darts only */
        double e = energy(system);
        if (energy_hip_failed(system) || e != e) return -1;
        if (system->quantum_rotation && quantum_system_rotational_energies(system)) return -1; /* mc.c:253-256 */
        checkpoint(system);
        system->avg_observables->counter = 1.0;
    }
    for (int k = 0; k < nsteps; k++) {
        ++system->step;
        const double initial_energy = system->observables->energy;
        make_move(system);
        const double final_energy = energy(system);
        if (energy_hip_failed(system)) return -1; /* device failure: stop, never count it as a reject */
        const int spinflip_move = system->checkpoint->movetype == MOVETYPE_SPINFLIP;
        if (system->quantum_rotation && spinflip_move && quantum_system_rotational_energies(system)) return -1; /* mc.c:304-308 */
        if (final_energy != final_energy || final_energy - final_energy != 0.0) {
            system->observables->energy = MAXVALUE;
            system->nodestats->boltzmann_factor = 0;
        } else
            boltzmann_factor(system, initial_energy, final_energy);
        const int volume_move = system->checkpoint->movetype == MOVETYPE_VOLUME;
        if ((get_rand(system) < system->nodestats->boltzmann_factor) && (system->iter_success == 0)) {
            checkpoint(system);
            ++system->nodestats->accept;
            if (volume_move) ++system->nodestats->accept_volume;
            if (spinflip_move) ++system->nodestats->accept_spinflip;
        } else {
            system->iter_success = 0;
            restore(system);
            ++system->nodestats->reject;
            if (volume_move) ++system->nodestats->reject_volume;
            if (spinflip_move) ++system->nodestats->reject_spinflip;
        }
        step_statistics(system);
    }
    return system->nodestats->accept - acc0;
}

/* The same chain for W walkers at once (independent systems, each with its own engine context, possibly on one
 * device): the trial moves of all walkers are enqueued before the first result is collected, so one walker's
 * launch gaps and host work are filled with another's kernels.  Every walker takes exactly the steps it would
 * take alone -- its random numbers, decisions and energies do not depend on its neighbours. */
int host_mc_steps_multi(system_t **systems, int nwalkers, int nsteps) {
    int accepted = 0;
    for (int w = 0; w < nwalkers; w++) {
        system_t *system = systems[w];
        if (system->step == 0 && system->avg_observables->counter == 0.0) {
            system->observables->volume = system->pbc->volume;
            if (system->cavity_bias) energy_hip_cavity_update(system); /* mc.c:245 */
            double e = energy(system);
            if (energy_hip_failed(system) || e != e) return -1;
            checkpoint(system);
            system->avg_observables->counter = 1.0;
        }
    }
    double initial[64];
    int ok[64];
    if (nwalkers > 64) return -1;
    for (int k = 0; k < nsteps; k++) {
        for (int w = 0; w < nwalkers; w++) {
            system_t *system = systems[w];
            ++system->step;
            initial[w] = system->observables->energy;
            make_move(system);
            ok[w] = (energy_hip_begin(system) == 0);
        }
        int failed = 0;
        for (int w = 0; w < nwalkers; w++) failed |= !ok[w];
        for (int w = 0; w < nwalkers; w++) {
            system_t *system = systems[w];
            /* every evaluation in flight is collected, also after a failure, so that no context is left mid-call */
            const double final_energy = ok[w] ? energy_hip_end(system) : NAN;
            failed |= energy_hip_failed(system);
            if (failed) continue;
            if (final_energy != final_energy || final_energy - final_energy != 0.0) {
                system->observables->energy = MAXVALUE;
                system->nodestats->boltzmann_factor = 0;
            } else
                boltzmann_factor(system, initial[w], final_energy);
            if ((get_rand(system) < system->nodestats->boltzmann_factor) && (system->iter_success == 0)) {
                checkpoint(system);
                ++system->nodestats->accept;
                ++accepted;
            } else {
                system->iter_success = 0;
                restore(system);
                ++system->nodestats->reject;
            }
            step_statistics(system);
        }
        if (failed) return -1;
    }
    return accepted;
}

void host_set_device(system_t *system, int device) { energy_hip_set_device(system, device); }
void host_enable_timing(system_t *system, int on) {
    energy_hip_enable_timing(system, on);
}
void host_get_timings(system_t *system, mpmc_hip_timings *out) { energy_hip_get_timings(system, out); }
void host_get_observables(system_t *system, double out[8]) {
    const observables_t *o = system->observables;
    out[0] = o->energy;
    out[1] = o->coulombic_energy;
    out[2] = o->rd_energy;
    out[3] = o->polarization_energy;
    out[4] = o->N;
    out[5] = system->nodestats->polarization_iterations;
    out[6] = (double)system->nodestats->accept;
    out[7] = (double)system->nodestats->reject;
}
void host_get_positions(system_t *system, double *pos) {
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next, i++)
            for (int p = 0; p < 3; p++) pos[3 * i + p] = a->pos[p];
}
int host_get_dipoles(system_t *system, double *mu, double *ef_static, double *ef_induced) {
    if (energy_hip_download_dipoles(system)) return -1;
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next, i++)
            for (int p = 0; p < 3; p++) {
                mu[3 * i + p] = a->mu[p];
                ef_static[3 * i + p] = a->ef_static[p];
                ef_induced[3 * i + p] = a->ef_induced[p];
            }
    return 0;
}
void host_seed(system_t *system, unsigned int seed) {
    system->preset_seeds = seed;
    system->preset_seeds_on = 1;
    system->rng_initialized = 0;
}
double host_get_rand(system_t *system) { return get_rand(system); }

/* for CPU tests of the move machinery: what energy() leaves behind for checkpoint()/make_move()
 * (molecule COMs and observables->N), without evaluating an energy */
void host_init_chain_no_energy(system_t *system) {
    update_com(system->molecules);
    system->observables->N = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        if (!m->frozen) system->observables->N += 1.0;
    checkpoint(system);
}

int host_set_option(system_t *system, const char *name, int value) {
    if (!energy_hip_context(system)) return -1;
    return mpmc_hip_set_option(energy_hip_context(system), name, value);
}

int host_natoms(system_t *system) { return countNatoms(system); }
int host_device_error(system_t *system) { return energy_hip_failed(system); }
void host_profile_report(void) { energy_hip_profile_report(); }
/* full flat copy of the current configuration (N may have changed under uvt) */
void host_get_system(system_t *system, double *pos, double *charge, double *alpha, double *eps, double *sig,
                     double *mass, int *molecule, int *frozen) {
    int i = 0, mi = 0;
    for (molecule_t *m = system->molecules; m; m = m->next, mi++)
        for (atom_t *a = m->atoms; a; a = a->next, i++) {
            for (int p = 0; p < 3; p++) pos[3 * i + p] = a->pos[p];
            charge[i] = a->charge;
            alpha[i] = a->polarizability;
            eps[i] = a->epsilon;
            sig[i] = a->sigma;
            mass[i] = a->mass;
            molecule[i] = mi;
            frozen[i] = a->frozen;
        }
}
void host_set_ensemble(system_t *system, int ensemble) { system->ensemble = ensemble; }

/* ---- disp_expansion (PHAHST) ---------------------------------------------------------------------------------- */
/* what the readers left: the four keywords the engine takes and the four it refuses, and the per-atom coefficients */
void host_get_disp_flags(system_t *system, int out[8]) {
    out[0] = system->disp_expansion;
    out[1] = system->damp_dispersion;
    out[2] = system->extrapolate_disp_coeffs;
    out[3] = system->schmidt_mixing;
    out[4] = system->disp_expansion_mbvdw;
    out[5] = system->gilbert_smith_mixing;
    out[6] = system->bohm_ahlrichs_mixing;
    out[7] = system->wilson_popelier_mixing;
}
void host_get_dispersion(system_t *system, double *c6, double *c8, double *c10) {
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next, i++) {
            c6[i] = a->c6;
            c8[i] = a->c8;
            c10[i] = a->c10;
        }
}
void host_set_dispersion(system_t *system, const double *c6, const double *c8, const double *c10) {
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next, i++) {
            a->c6 = c6[i];
            a->c8 = c8[i];
            a->c10 = c10[i];
        }
}
/* ---- axilrod_teller ------------------------------------------------------------------------------------------- */
void host_get_at_flags(system_t *system, int out[2]) {
    out[0] = system->axilrod_teller;
    out[1] = system->midzuno_kihara_approx;
}
void host_get_c9(system_t *system, double *c9) {
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next, i++) c9[i] = a->c9;
}
void host_set_c9(system_t *system, const double *c9) {
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next, i++) a->c9 = c9[i];
}
double host_get_three_body_energy(system_t *system) { return system->observables->three_body_energy; }
/* ---- polarvdw and cavity_autoreject_absolute ------------------------------------------------------------------ */
/* polarvdw, cavity_autoreject_absolute, cavity_autoreject_scale, count_autorejects, observables->vdw_energy */
void host_get_vdw(system_t *system, double out[5]) {
    out[0] = (double)system->polarvdw;
    out[1] = (double)system->cavity_autoreject_absolute;
    out[2] = system->cavity_autoreject_scale;
    out[3] = (double)system->count_autorejects;
    out[4] = system->observables->vdw_energy;
}
void host_get_omega(system_t *system, double *omega) {
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next)
        for (atom_t *a = m->atoms; a; a = a->next, i++) omega[i] = a->omega;
}
/* per-atom omega (atomic units) and type id of a system built from arrays: the molecule type becomes "T<id>" */
void host_set_omega(system_t *system, const double *omega, const int *mol_type) {
    int i = 0;
    for (molecule_t *m = system->molecules; m; m = m->next) {
        if (m->atoms) snprintf(m->moleculetype, MAXLINE, "T%d", mol_type[i]);
        for (atom_t *a = m->atoms; a; a = a->next, i++) a->omega = omega[i];
    }
}
/* test entry: the index-th molecule of the list steps by d, outside Metropolis; the next energy() finds it by walking
 * the lists.  Returns non-zero when there is no such molecule. */
int host_displace_molecule(system_t *system, int index, const double d[3]) {
    molecule_t *m = system->molecules;
    for (int k = 0; m && k < index; k++) m = m->next;
    if (!m || index < 0) return 1;
    for (atom_t *a = m->atoms; a; a = a->next)
        for (int p = 0; p < 3; p++) a->pos[p] += d[p];
    energy_hip_note_list_changed(system);
    return 0;
}
/* ---- rd_crystal and ensemble replay ---------------------------------------------------------------------------- */
void host_get_rdc_flags(system_t *system, int out[2]) {
    out[0] = system->rd_crystal;
    out[1] = system->rd_crystal_order;
}
/* sg, dreiding, lj_buffered_14_7, waldmanhagler, halgren_mixing, c6_mixing */
void host_get_rdform_flags(system_t *system, int out[6]) {
    out[0] = system->sg;
    out[1] = system->dreiding;
    out[2] = system->lj_buffered_14_7;
    out[3] = system->waldmanhagler;
    out[4] = system->halgren_mixing;
    out[5] = system->c6_mixing;
}
/* the dipole tensor's keywords as read: damp_type (DAMPING_OFF / _LINEAR / _EXPONENTIAL), polar_wolf_full, polar_ewald_full */
void host_get_thole_flags(system_t *system, int out[3]) {
    out[0] = system->damp_type;
    out[1] = system->polar_wolf_full;
    out[2] = system->polar_ewald_full;
}
/* frame `index` (from 0) of the PQR trajectory `path` becomes the system's configuration, read the way
 * replay_trajectory() reads it: every frame in front of it is read (and freed) first, so the box and the cutoff are
 * what a replay would hold at that frame.  Returns read_frame()'s answer for that frame (1: the trajectory is shorter). */
int host_read_frame(system_t *system, const char *path, int index) {
    FILE *fp = fopen(path, "r");
    if (!fp) return -1;
    int rc = 0;
    for (int k = 0; k <= index && rc == 0; k++) rc = read_frame(fp, system);
    fclose(fp);
    return rc;
}
/* the reason energy() would refuse this system, or NULL */
const char *host_unsupported(system_t *system) { return energy_hip_unsupported(system); }
/* polarizability_tensor: the tensor of the last energy() (no printing); non-zero when the engine refuses */
int host_get_polarizability_tensor(system_t *system, double out[9]) {
    return energy_hip_polarizability_tensor(system, out, 0);
}

/* ---- npt ---------------------------------------------------------------------------------------------------- */
void host_get_basis(system_t *system, double basis[9]) {
    for (int p = 0; p < 3; p++)
        for (int q = 0; q < 3; q++) basis[3 * p + q] = system->pbc->basis[p][q];
}
/* volume, cutoff, the volume moves accepted / rejected so far, the move checkpoint() decided on */
void host_get_npt(system_t *system, double out[5]) {
    out[0] = system->pbc->volume;
    out[1] = system->pbc->cutoff;
    out[2] = (double)system->nodestats->accept_volume;
    out[3] = (double)system->nodestats->reject_volume;
    out[4] = (double)system->checkpoint->movetype;
}
/* 0 = energy_hip() ignores volume-move notes: every volume step uploads the whole configuration (A/B, tests) */
void host_set_volume_notes(system_t *system, int on) { energy_hip_set_volume_notes(system, on); }
/* full uploads, edit calls carried out, molecules they removed + inserted (energy_hip_sync_counts) */
void host_get_sync_counts(system_t *system, long out[3]) { energy_hip_sync_counts(system, out); }
/* the per-atom c9 the binding sends (energy_hip_effective_c9) */
double host_effective_c9(int midzuno_kihara_approx, double alpha, double c6, double c9) {
    return energy_hip_effective_c9(midzuno_kihara_approx, alpha, c6, c9);
}
/* One volume move to a stated new volume, outside Metropolis, so that tests reach both branches: exactly what
 * make_move() does for MOVETYPE_VOLUME except that the new volume is given instead of drawn (as the reference's
 * ENSEMBLE_REPLAY branch, mc_moves.c:176-178), and on request exactly what restore() does to take it back.  The
 * observables are checkpointed first, as checkpoint() does.  No energy is evaluated here (only the centres of mass
 * an energy() between the two would leave are refreshed). */
void host_force_volume_move(system_t *system, double new_volume, int revert) {
    memcpy(system->checkpoint->observables, system->observables, sizeof(observables_t));
    system->checkpoint->observables->volume = system->pbc->volume;
    volume_change_to(system, new_volume);
    if (revert) {
        update_com(system->molecules); /* what the energy() between a change and its revert leaves (pairs.c:331) */
        memcpy(system->observables, system->checkpoint->observables, sizeof(observables_t));
        revert_volume_change(system);
    }
}

/* ---- cavity_bias ----------------------------------------------------------------------------------------------- */
/* the keywords as read: cavity_bias, cavity_grid, cavity_radius */
void host_get_cavity_flags(system_t *system, double out[3]) {
    out[0] = (double)system->cavity_bias;
    out[1] = (double)system->cavity_grid_size;
    out[2] = system->cavity_radius;
}
/* the state after the last make_move(): cavities_open, hits and number of the darts, cavity_volume,
 * nodestats->cavity_bias_probability, its running mean over this walker's steps (avg_nodestats), the corrtime mean over
 * the walkers (avg_observables), checkpoint->biased_move, nodestats->boltzmann_factor, the last trial's energy (kept by the binding: restore() takes a
 * rejected one out of the observables).  Returns the number of darts. */
int host_get_cavity(system_t *system, double out[10]) {
    int hits = 0;
    const int n_darts = energy_hip_cavity_darts(system, NULL, &hits);
    out[0] = (double)system->cavities_open;
    out[1] = (double)hits;
    out[2] = (double)n_darts;
    out[3] = system->cavity_volume;
    out[4] = system->nodestats->cavity_bias_probability;
    out[5] = system->avg_nodestats->cavity_bias_probability;
    out[6] = system->avg_observables->cavity_bias_probability;
    out[7] = (double)system->checkpoint->biased_move;
    out[8] = system->nodestats->boltzmann_factor;
    out[9] = energy_hip_last_energy(system);
    return n_darts;
}
/* the last make_move()'s dart positions, [n][3] with n = host_get_cavity()'s answer */
void host_get_cavity_darts(system_t *system, double *darts) {
    const double *d = NULL;
    const int n = energy_hip_cavity_darts(system, &d, NULL);
    if (d && n > 0) memcpy(darts, d, 3 * (size_t)n * sizeof(double));
}
