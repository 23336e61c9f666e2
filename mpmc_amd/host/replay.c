/*
 * replay.c -- `ensemble replay`: energy() of every frame of a PQR trajectory (reference src/mc/replay.c:34-98,
 * src/io/simulation_box.c:28-60, src/io/read_pqr.c:3-106).
 *
 * A frame is the ATOM lines up to an END line; under `read_pqr_box on` its `REMARK BOX BASIS[k] = x y z` lines, which
 * stand in front of that END, set the box.  Every frame frees the molecules of the one before, reads its own, runs pbc()
 * and energy() -- a full upload, and a new device context when the frame has more atoms than the context holds -- and
 * writes one observables line.  As in the reference, pbc() keeps a cutoff that is already set: without `pbc_cutoff` the
 * cutoff of the FIRST frame's box holds for the whole trajectory.  calc_pressure is refused at input time.
 */
#include <stdlib.h>
#include <string.h>

#include "mpmc_host.h"

static void free_molecules(molecule_t *m) {
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
}

static int to_double(const char *s, double *out) {
    char *end;
    if (!s[0]) return 1;
    *out = strtod(s, &end);
    return *end != 0;
}

/* read_pqr_box(), read_pqr.c:3-72: the REMARK BOX lines between the current position and the next END */
static void read_frame_box(FILE *fp, system_t *system) {
    char buffer[MAXLINE], token[7][MAXLINE];
    while (fgets(buffer, MAXLINE, fp)) {
        for (int i = 0; i < 7; i++) token[i][0] = 0;
        sscanf(buffer, "%s %s %s %s %s %s %s", token[0], token[1], token[2], token[3], token[4], token[5], token[6]);
        if (!strncmp(token[0], "END", 3)) break;
        if (strcmp(token[0], "REMARK") || strcmp(token[1], "BOX") || strcmp(token[3], "=")) continue;
        if (strncmp(token[2], "BASIS[", 6) || token[2][6] < '0' || token[2][6] > '2' || strcmp(token[2] + 7, "]")) continue;
        double v[3];
        if (to_double(token[4], &v[0]) || to_double(token[5], &v[1]) || to_double(token[6], &v[2])) continue;
        memcpy(system->pbc->basis[token[2][6] - '0'], v, sizeof(v));
    }
}

int read_frame(FILE *fp, system_t *system) {
    free_molecules(system->molecules);
    system->molecules = NULL;
    system->movable_valid = 0;
    system->natoms = 0;
    energy_hip_note_list_changed(system); /* the molecules the device layer knew are gone */
    const long start = ftell(fp);
    system->molecules = read_molecules(fp, system); /* up to and including the END line */
    if (!system->molecules) {
        output("INPUT: end of trajectory file\n");
        return 1;
    }
    if (system->read_pqr_box_on) {
        if (start < 0 || fseek(fp, start, SEEK_SET)) {
            error("INPUT: could not rewind the trajectory for its box\n");
            return -1;
        }
        read_frame_box(fp, system);
    }
    pbc(system);
    if ((system->pbc->volume <= 0.0) || (system->pbc->cutoff <= 0.0)) {
        error("INPUT: invalid simulation box dimensions.\n");
        return -1;
    }
    system->natoms = countNatoms(system);
    return 0;
}

int replay_trajectory(system_t *system) {
    char linebuf[MAXLINE];
    FILE *finput = fopen(system->traj_input, "r");
    if (!finput) {
        snprintf(linebuf, MAXLINE, "REPLAY: could not open traj_input %.400s\n", system->traj_input);
        error(linebuf);
        return -1;
    }
    system->step = 0;
    if (system->energy_output[0] && !system->fp_energy) {
        system->fp_energy = fopen(system->energy_output, "w");
        if (!system->fp_energy) {
            error("REPLAY: could not open files\n");
            fclose(finput);
            return -1;
        }
        fprintf(system->fp_energy,
                "#step #energy #coulombic #rd #polar #vdw #kinetic #kin_temp #N #spin_ratio #volume #core_temp\n");
    }
    int rc = 0;
    for (;;) {
        const int got = read_frame(finput, system); /* frees the frame before (or what setup_system() read) */
        if (got == 1) break;
        if (got) {
            output("REPLAY: simulation box not properly set up\n");
            rc = -1;
            break;
        }
        system->step++;
        system->observables->volume = system->pbc->volume;
        system->last_volume = -1.0; /* a new configuration: energy() uploads it as a whole */
        energy(system);
        if (energy_hip_failed(system)) {
            error("REPLAY: the device engine failed, stopping\n");
            rc = -1;
            break;
        }
        /* replay.c:69: solve for the rotational energy levels */
        if (system->quantum_rotation && quantum_system_rotational_energies(system)) {
            rc = -1;
            break;
        }
        if (system->fp_energy) write_observables(system->fp_energy, system, system->observables, system->temperature);
    }
    fclose(finput);
    snprintf(linebuf, MAXLINE, "REPLAY: %d frames\n", system->step);
    output(linebuf);
    return rc;
}
