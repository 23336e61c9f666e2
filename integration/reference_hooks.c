/*
 * reference_hooks.c -- every line a maintainer adds to the reference tree (smann95/mpmc) OUTSIDE
 * src/energy/energy_hip.c, collected in one translation unit so that it can be compiled against the reference's
 * real headers.  tests/test_reference_binding.py does that in the build container (gcc -fsyntax-only with
 * -I/root/reference/src/include, <structs.h> taken from a scratch copy that has the one new member `int hip;`),
 * and checks that the C snippets of INTEGRATION.md are excerpts of this file and of mpmc_amd/host/energy_hip.c.
 * Nothing here is compiled into this repository's own libraries; each function is the patch to the reference
 * function named in its comment, reduced to the added lines plus the statements they sit between.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <structs.h>
#include <function_prototypes.h>
extern int rank, size; /* src/main/main.c:8 */
#include "energy_hip.h"

/* src/io/input.c, do_command(): next to the `cuda` keyword (:1245-1255) */
int hook_do_command(system_t *system, char **token) {
    if (!strcasecmp(token[0], "hip")) {
        if (!strcasecmp(token[1], "on"))
            system->hip = 1;
        else if (!strcasecmp(token[1], "off"))
            system->hip = 0;
        else
            return 1;
    }
    return 0;
}

/* src/io/check_input.c: the twin of the `cuda` guard (:325-341); energy_hip() repeats these checks on every
 * call and fails (never computes something else) when an option it does not implement is on.  `disp_expansion` is no
 * longer among them (default and Schmidt mixing, with or without damp_dispersion / extrapolate_disp_coeffs); the other
 * mixing rules and disp_expansion_mbvdw are refused there, each by name.  Nor is `polar_iterative off`: the engine solves
 * the linear system directly then (mpmc_hip_set_exact_polar).  Nor are polar_damp_type linear / off and polar_wolf_full:
 * the engine has all of thole_amatrix()'s tensors (mpmc_hip_set_thole_model); what stays is the one combination it
 * refuses */
int hook_check_system(system_t *system) {
    if (system->hip && system->polarization) {
        if (system->polar_wolf_full && system->damp_type != DAMPING_EXPONENTIAL) {
            error("INPUT: HIP engine: polar_wolf_full needs polar_damp_type exponential\n");
            return -1;
        }
    }
    return 0;
}

/* src/energy/energy.c:67, first statement of energy() */
double hook_energy(system_t *system) {
    if (system->hip) return energy_hip(system);
    return 0.0; /* ... unchanged CPU path ... */
}

/* src/energy/energy.c:229, first statement of energy_no_observables() */
double hook_energy_no_observables(system_t *system) {
    if (system->hip) {
        observables_t keep = *system->observables; /* this entry point must leave the observables alone */
        const double potential_energy = energy_hip(system);
        *system->observables = keep;
        return potential_energy;
    }
    return 0.0; /* ... unchanged CPU path ... */
}

/* src/energy/pairs.c: first statement of setup_pairs() (:550), pairs() (:293), flag_all_pairs() (:44),
 * update_pairs_insert() (:388), update_pairs_remove() (:431), unupdate_pairs_insert() (:469) and
 * unupdate_pairs_remove() (:507): with `hip on` there is no pair list (200 B per pair: 1.7 GB at 4096 atoms,
 * 45 GB for the 21 183 atoms of sample_configs_gpu/3_PCN61); copy_molecule() and cleanup() already cope with
 * atom->pairs == NULL (mc_moves.c:364, cleanup.c:19) */
void hook_pairs(system_t *system) {
    if (system->hip) return;
}

/* src/main/main.c:176 and src/main/cleanup.c:219: the A matrix lives in HBM */
void hook_main(system_t *system) {
    if (system->polarization && !system->cuda && !system->hip && !system->polar_zodid)
        thole_resize_matrices(system);
}
void hook_cleanup(system_t *system) {
    if (system->hip) energy_hip_cleanup(system);
    if (system->polarization && !system->cuda && !system->hip) free_matrices(system);
}

/* src/main/main.c, after the MPI block (:45-52): without MPI, the launcher's environment names the walker
 * (one process per GPU: MPMC_HIP_RANK / MPMC_HIP_NRANKS / MPMC_HIP_ID_FILE, see walkers_init_from_env()) */
void hook_main_rank(void) {
#ifndef MPI
    if (getenv("MPMC_HIP_NRANKS") && getenv("MPMC_HIP_RANK")) {
        size = atoi(getenv("MPMC_HIP_NRANKS"));
        rank = atoi(getenv("MPMC_HIP_RANK"));
    }
#endif
}

/* src/mc/mc.c, mc(): the lines added around the existing statements (:246-251, :302, :398-414, :431-436) */
int hook_mc(system_t *system, char *snd_strct, char *rcv_strct, int msgsize, double *temperature_mpi) {
    double initial_energy, final_energy;

    /* :243-246 -- rcv_strct / temperature_mpi are allocated on every rank, not only on the root: the gather
     * below is an all-gather (the root still is the only one that averages and writes) */
    if (system->hip || !rank) {
        rcv_strct = calloc(size, msgsize);
        temperature_mpi = calloc(size, sizeof(double));
    }

    /* :251 */
    initial_energy = energy(system);
    if (system->hip && energy_hip_failed(system)) return (-1); /* a dead device is not a bad contact */
    if (system->hip && walkers_init_from_env(system) < 0) return (-1); /* needs the context energy() made */

    /* :302 */
    final_energy = energy(system);
    if (system->hip && energy_hip_failed(system)) {
        error("MC: the HIP engine failed, stopping the chain\n");
        return (-1);
    }

    /* :398-414, in front of write_dipole() / write_field() (and of write_states(), which prints wrapped_pos) */
    if (system->hip) energy_hip_corrtime(system);
    if (system->polarization) {
        write_dipole(system);
        write_field(system);
    }

    /* :431-436, the branch without MPI */
#ifndef MPI
    if (system->hip && size > 1) {
        if (walkers_gather(system, snd_strct, msgsize, rcv_strct) < 0) return (-1);
        if (walkers_gather(system, &(system->temperature), sizeof(double), temperature_mpi) < 0) return (-1);
    } else {
        memcpy(rcv_strct, snd_strct, msgsize);
        temperature_mpi[0] = system->temperature;
    }
#endif
    (void)initial_energy;
    (void)final_energy;
    return 0;
}

/* src/mc/mc_moves.c (optional: saves energy_hip() one list walk per step).  make_move(), MOVETYPE_DISPLACE /
 * MOVETYPE_ADIABATIC (:697-718), after the displacement: */
void hook_make_move_displace(system_t *system) {
    energy_hip_note_moved(system, system->checkpoint->molecule_altered, system->checkpoint->molecule_altered);
}
/* make_move() MOVETYPE_INSERT / MOVETYPE_REMOVE and restore()'s counterparts: */
void hook_list_changed(system_t *system) {
    energy_hip_note_list_changed(system);
}
/* volume_change() (:168-210) and revert_volume_change() (:213-248), the same added lines in both (nothing else of
 * either function changes): the displacement of every molecule is kept while the molecule loop runs and handed over
 * behind it, so that energy_hip() moves the resident configuration into the new box instead of uploading it again
 * (without them: a full upload, as before).  `delta_pos` is the loop's own variable. */
void hook_volume_change(system_t *system, const double delta_pos[3]) {
    molecule_t *m;

    /* in front of the molecule loop (:195 / :232) */
    int hip_k = 0, hip_n = 0;
    for (m = system->molecules; m; m = m->next) hip_n++;
    double *hip_delta = system->hip ? malloc(3 * hip_n * sizeof(double)) : NULL;

    /* inside it, once per molecule, behind the loop that fills delta_pos (:200 / :238) */
    if (hip_delta) memcpy(hip_delta + 3 * hip_k++, delta_pos, 3 * sizeof(double));

    /* behind it (:207 / :245) */
    if (system->hip && !hip_delta) energy_hip_note_list_changed(system);
    if (hip_delta) energy_hip_note_volume_change(system, hip_delta);
    free(hip_delta);
}
/* src/mc/cavity.c, cavity_update_grid() (:112), first statement: with `hip on` the grid lives on the device.  The binding
 * draws the darts of cavity_volume() itself (same get_rand() calls, same order) and fills cavities_open, cavity_volume
 * and nodestats->cavity_bias_probability; system->cavity_grid stays unused (setup_cavity_grid() may still allocate it) */
void hook_cavity_update_grid(system_t *system) {
    if (system->hip) {
        energy_hip_cavity_update(system);
        return;
    }
    /* ... unchanged CPU path ... */
}
/* src/mc/mc_moves.c, make_move(), MOVETYPE_INSERT under cavity_bias (:587-606): the scan of cavity_grid that lists the
 * open points is skipped, the position of the random_index-th open point comes from the device.  `random_index` and
 * `com` are the function's own variables; the draw of random_index (:603) stays where it is, in front of this line */
void hook_make_move_cavity_point(system_t *system, int random_index, double com[3]) {
    if (system->hip) energy_hip_cavity_point(system, random_index, com);
}
/* src/quantum_rotation/rotational_eigenspectrum.c, quantum_rotational_grid() (:219-266) under `hip on`: the 256 grid
 * energies of a molecule in ONE call instead of an energy_no_observables() + energy() pair per grid point inside
 * rotational_potential().  xyz: the placements align_molecule() + rotate_spherical() give, [p * 16 + t][sites][3], formed
 * from copies of the molecule's coordinates; energies: [p * 16 + t].  The molecule and the observables stay untouched;
 * the caller multiplies with sin(theta) into quantum_rotational_potential_grid[t][p] as before. */
int hook_quantum_rotational_grid(system_t *system, molecule_t *molecule, const double *xyz, double *energies) {
    if (system->hip)
        return energy_hip_trial_energies(system, molecule, QUANTUM_ROTATION_GRID * QUANTUM_ROTATION_GRID, xyz, energies);
    return 1; /* ... unchanged CPU path ... */
}
/* restore(), default branch (:778-797), where the backup is linked into the list in place of the altered node: */
void hook_restore_displace(system_t *system) {
    energy_hip_note_moved(system, system->checkpoint->molecule_backup, system->checkpoint->molecule_altered);
}
