/*
 * mc.c -- canonical (NVT), grand-canonical (UVT) and isobaric (NPT) Markov chain, host side; mirrors the control flow of the reference's
 * mc() (src/mc/mc.c:196-525), checkpoint()/restore() (src/mc/checkpoint.c:4-186,
 * src/mc/mc_moves.c:744-807), make_move()/displace() (src/mc/mc_moves.c:378-488, :567-741) and
 * get_rand() (src/mersenne/mersenne.cpp:9-22) for the displacement move.  Random numbers are
 * consumed in the reference's order: pick molecule, 6 for translate, 4 for rotate, 1 for Metropolis.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "mpmc_host.h"

/* ---- std::mt19937 + std::uniform_real_distribution<double>(0,1) as libstdc++ evaluates it:
 * generate_canonical<double,53> draws two 32-bit words, sum = w0 + w1 * 2^32, result sum / 2^64.
 * The generator state lives in the system_t (the reference has one per process = per walker; here one
 * process may drive several walkers, each with its own stream of numbers). */
void seed_rng(system_t *system, unsigned int seed) {
    unsigned int *mt = system->rng_mt;
    int mti;
    mt[0] = seed;
    for (mti = 1; mti < 624; mti++) mt[mti] = 1812433253u * (mt[mti - 1] ^ (mt[mti - 1] >> 30)) + (unsigned int)mti;
    system->rng_mti = mti;
}

static unsigned int mt_next(system_t *system) {
    unsigned int *mt = system->rng_mt;
    if (system->rng_mti >= 624) {
        for (int k = 0; k < 624; k++) {
            unsigned int y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
            mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        system->rng_mti = 0;
    }
    unsigned int y = mt[system->rng_mti++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

double get_rand(system_t *system) {
    if (!system->rng_initialized) {
        system->rng_initialized = 1;
        if (system->preset_seeds_on)
            seed_rng(system, system->preset_seeds);
        else {
            unsigned int s = 5489u;
            FILE *f = fopen("/dev/urandom", "rb");
            if (f) {
                if (fread(&s, sizeof(s), 1, f) != 1) s = 5489u;
                fclose(f);
            }
            seed_rng(system, s);
        }
    }
    double sum = 0.0, tmp = 1.0;
    for (int k = 0; k < 2; k++) {
        sum += (double)mt_next(system) * tmp;
        tmp *= 4294967296.0;
    }
    double ret = sum / tmp;
    if (ret >= 1.0) ret = nextafter(1.0, 0.0);
    return ret;
}

/* ---- moves ---------------------------------------------------------------------------------- */
void translate(system_t *system, molecule_t *molecule, pbc_t *pbc, double scale) {
    double trans_x = scale * get_rand(system) * pbc->cutoff;
    double trans_y = scale * get_rand(system) * pbc->cutoff;
    double trans_z = scale * get_rand(system) * pbc->cutoff;
    if (get_rand(system) < 0.5) trans_x *= -1.0;
    if (get_rand(system) < 0.5) trans_y *= -1.0;
    if (get_rand(system) < 0.5) trans_z *= -1.0;
    molecule->com[0] += trans_x;
    molecule->com[1] += trans_y;
    molecule->com[2] += trans_z;
    for (atom_t *a = molecule->atoms; a; a = a->next) {
        a->pos[0] += trans_x;
        a->pos[1] += trans_y;
        a->pos[2] += trans_z;
    }
}

typedef struct { double x, y, z, w; } quat_t;
static quat_t qmul(quat_t a, quat_t b) { /* reference src/main/quaternion.c:65-75 */
    quat_t r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    return r;
}

void rotate(system_t *system, molecule_t *molecule, pbc_t *pbc, double scale) {
    (void)pbc;
    double x = get_rand(system) - 0.5;
    double y = get_rand(system) - 0.5;
    double z = get_rand(system) - 0.5;
    double angle = get_rand(system) * 360 * scale;
    quat_t q = {0., 0., 0., 1.}, qc;
    angle /= 57.2957795; /* quaternion_construct_axis_angle_degree, quaternion.c:44-59 */
    double magnitude = sqrt(x * x + y * y + z * z);
    if (magnitude != 0.0) {
        x /= magnitude;
        y /= magnitude;
        z /= magnitude;
        double sinAngle = sin(angle / 2);
        q.x = x * sinAngle;
        q.y = y * sinAngle;
        q.z = z * sinAngle;
        q.w = cos(angle / 2);
    }
    qc.x = -q.x; qc.y = -q.y; qc.z = -q.z; qc.w = q.w;
    const double com[3] = {molecule->com[0], molecule->com[1], molecule->com[2]};
    for (atom_t *a = molecule->atoms; a; a = a->next) {
        quat_t p = {a->pos[0] - com[0], a->pos[1] - com[1], a->pos[2] - com[2], 0.};
        quat_t ans = qmul(q, qmul(p, qc));
        a->pos[0] = ans.x + com[0];
        a->pos[1] = ans.y + com[1];
        a->pos[2] = ans.z + com[2];
    }
}

/* ---- npt: scale the volume (reference volume_change() / revert_volume_change(), src/mc/mc_moves.c:168-248) ---- */
int wrapall(molecule_t *molecules, pbc_t *pbc) { /* reference src/io/output.c:142-183 */
    double d[3], dimg[3];
    for (molecule_t *m = molecules; m; m = m->next) {
        if (!m->frozen) {
            for (int i = 0; i < 3; i++) {
                d[i] = 0;
                for (int j = 0; j < 3; j++) d[i] += pbc->reciprocal_basis[j][i] * m->com[j];
                d[i] = rint(d[i]);
            }
            for (int i = 0; i < 3; i++) {
                dimg[i] = 0;
                for (int j = 0; j < 3; j++) dimg[i] += pbc->basis[j][i] * d[j];
                m->wrapped_com[i] = dimg[i];
            }
            for (atom_t *a = m->atoms; a; a = a->next)
                for (int i = 0; i < 3; i++) a->wrapped_pos[i] = a->pos[i] - dimg[i];
        } else
            for (atom_t *a = m->atoms; a; a = a->next)
                for (int i = 0; i < 3; i++) a->wrapped_pos[i] = a->pos[i];
    }
    return 0;
}

/* what both functions share: the basis is scaled, pbc() redone (the cutoff, once set, stays: pbc.c:71), and every
 * molecule -- frozen ones too -- is shifted rigidly by (scaled COM - COM).  The displacements are handed to the
 * binding, whose device copy takes the very same additions (energy_hip_note_volume_change). */
static void scale_volume(system_t *system, double new_volume, int revert) {
    double new_com[3], old_com[3], delta_pos[3];
    int nmol = 0, k = 0;
    for (molecule_t *m = system->molecules; m; m = m->next) nmol++;
    double *hip_delta = malloc((nmol > 0 ? nmol : 1) * 3 * sizeof(double));

    const double basis_scale_factor = pow(new_volume / system->pbc->volume, 1.0 / 3.0);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) system->pbc->basis[i][j] *= basis_scale_factor;

    pbc(system);
    system->observables->volume = system->pbc->volume;

    for (molecule_t *m = system->molecules; m; m = m->next, k++) {
        for (int i = 0; i < 3; i++) {
            old_com[i] = m->com[i]; /* a change leaves com to the next energy(); a revert has none following */
            new_com[i] = m->com[i] * basis_scale_factor;
            if (revert) m->com[i] = new_com[i];
            delta_pos[i] = new_com[i] - old_com[i];
            if (hip_delta) hip_delta[3 * k + i] = delta_pos[i];
        }
        for (atom_t *a = m->atoms; a; a = a->next)
            for (int i = 0; i < 3; i++) {
                a->pos[i] += delta_pos[i];
                a->wrapped_pos[i] += delta_pos[i];
            }
    }
    if (revert) wrapall(system->molecules, system->pbc);
    if (hip_delta)
        energy_hip_note_volume_change(system, hip_delta);
    else
        energy_hip_note_list_changed(system);
    free(hip_delta);
}

void volume_change_to(system_t *system, double new_volume) { scale_volume(system, new_volume, 0); }

void volume_change(system_t *system) {
    const double log_new_volume = log(system->pbc->volume) + (get_rand(system) - 0.5) * system->volume_change_factor;
    const double new_volume = exp(log_new_volume);
    scale_volume(system, new_volume, 0);
}

void revert_volume_change(system_t *system) {
    /* system->pbc->volume still has the rejected value until pbc() is called */
    scale_volume(system, system->checkpoint->observables->volume, 1);
}

/* deep copy of a molecule and its atoms (reference copy_molecule(), src/mc/mc_moves.c:251-330) */
molecule_t *copy_molecule(system_t *system, molecule_t *src) {
    (void)system;
    molecule_t *dst = calloc(1, sizeof(molecule_t));
    memcpy(dst, src, sizeof(molecule_t));
    dst->next = NULL;
    dst->atoms = NULL;
    atom_t *tail = NULL;
    for (atom_t *a = src->atoms; a; a = a->next) {
        atom_t *c = calloc(1, sizeof(atom_t));
        memcpy(c, a, sizeof(atom_t));
        c->next = NULL;
        if (tail)
            tail->next = c;
        else
            dst->atoms = c;
        tail = c;
    }
    return dst;
}

void free_molecule(system_t *system, molecule_t *molecule) {
    (void)system;
    atom_t *a = molecule->atoms;
    while (a) {
        atom_t *n = a->next;
        free(a);
        a = n;
    }
    free(molecule);
}

/* (a) decides the next move, (b) backs up the state it will alter (reference checkpoint(),
 * src/mc/checkpoint.c:4-186; the NVT and plain UVT branches) */
void checkpoint(system_t *system) {
    checkpoint_t *cp = system->checkpoint;
    memcpy(cp->observables, system->observables, sizeof(observables_t));

    /* table of the movable molecules (the reference walks the list for this, twice per step) */
    if (!system->movable_valid) {
        int n = 0;
        for (molecule_t *m = system->molecules; m; m = m->next)
            if (!m->frozen) ++n;
        if (n > system->movable_cap) {
            free(system->movable);
            free(system->movable_prev);
            system->movable_cap = 2 * n + 64;
            system->movable = malloc(system->movable_cap * sizeof(molecule_t *));
            system->movable_prev = malloc(system->movable_cap * sizeof(molecule_t *));
        }
        n = 0;
        molecule_t *before = NULL;
        for (molecule_t *m = system->molecules; m; before = m, m = m->next)
            if (!m->frozen) {
                system->movable[n] = m;
                system->movable_prev[n++] = before;
            }
        system->nmovable = n;
        system->movable_valid = 1;
    }
    int num_molecules_exchange = system->nmovable;

    if (system->ensemble == ENSEMBLE_UVT) {
        if (get_rand(system) < system->insert_probability) {
            if (get_rand(system) < 0.5)
                cp->movetype = MOVETYPE_INSERT;
            else
                cp->movetype = MOVETYPE_REMOVE;
        } else if (system->quantum_rotation) { /* checkpoint.c:57-65 */
            if (get_rand(system) < system->spinflip_probability)
                cp->movetype = MOVETYPE_SPINFLIP;
            else
                cp->movetype = MOVETYPE_DISPLACE;
        } else
            cp->movetype = MOVETYPE_DISPLACE;
    } else if (system->ensemble == ENSEMBLE_NPT) { /* checkpoint.c:84-98 */
        if (system->volume_probability == 0.0) { /* not set: volume moves with probability 1 / nmolecules */
            if (get_rand(system) < 1.0 / system->observables->N)
                cp->movetype = MOVETYPE_VOLUME;
            else
                cp->movetype = MOVETYPE_DISPLACE;
        } else {
            if (get_rand(system) < system->volume_probability)
                cp->movetype = MOVETYPE_VOLUME;
            else
                cp->movetype = MOVETYPE_DISPLACE;
        }
    } else if (system->quantum_rotation && (get_rand(system) < system->spinflip_probability)) /* nvt, checkpoint.c:78-81 */
        cp->movetype = MOVETYPE_SPINFLIP;
    else
        cp->movetype = MOVETYPE_DISPLACE;

    /* randomly pick a (moveable) molecule: floor(rand * N) over the exchangeable ones in list order */
    --num_molecules_exchange;
    int altered = (int)floor(get_rand(system) * system->observables->N);
    molecule_t *pick = NULL, *head = NULL;
    if (altered >= 0 && altered < system->nmovable) {
        pick = system->movable[altered];
        head = system->movable_prev[altered];
    }
    cp->altered_index = altered;
    cp->molecule_altered = pick;
    /* never completely empty the list */
    if (!num_molecules_exchange && cp->movetype == MOVETYPE_REMOVE) cp->movetype = MOVETYPE_DISPLACE;
    cp->head = head;
    cp->tail = pick ? pick->next : NULL;
    if (cp->molecule_backup) {
        free_molecule(system, cp->molecule_backup);
        cp->molecule_backup = NULL;
    }
    if (pick) cp->molecule_backup = copy_molecule(system, pick);
}

/* apply what checkpoint() decided (reference make_move(), src/mc/mc_moves.c:567-741) */
void make_move(system_t *system) {
    checkpoint_t *cp = system->checkpoint;
    /* update the cavity grid prior to making a move (mc_moves.c:577-580): on the device, for the accepted configuration */
    if (system->cavity_bias) {
        energy_hip_cavity_update(system); /* (a device failure stops the chain at the next energy()) */
        cp->biased_move = 0;
    }
    if (cp->movetype == MOVETYPE_VOLUME) { /* (needs no picked molecule) */
        volume_change(system);
        return;
    }
    if (!cp->molecule_altered) return;
    switch (cp->movetype) {
        case MOVETYPE_INSERT: {
            /* insert a copy of the picked molecule at a random position and orientation */
            double rand[3], com[3];
            if (system->cavity_bias && system->cavities_open) { /* umbrella sampling, mc_moves.c:585-608 */
                /* doing a biased move - this flag lets boltzmann_factor() know about it */
                cp->biased_move = 1;
                /* insert randomly at one of the free cavity points: the reference lists them in (i, j, k) order, the
                 * device keeps that list */
                const int random_index =
                    (system->cavities_open - 1) - (int)rint(((double)(system->cavities_open - 1)) * get_rand(system));
                energy_hip_cavity_point(system, random_index, com);
            } else {
                for (int p = 0; p < 3; p++) rand[p] = 0.5 - get_rand(system);
                for (int p = 0; p < 3; p++) {
                    com[p] = 0;
                    for (int q = 0; q < 3; q++) com[p] += system->pbc->basis[q][p] * rand[q];
                }
            }
            energy_hip_note_list_changed(system);
            system->movable_valid = 0;
            molecule_t *ins = cp->molecule_backup;
            for (atom_t *a = ins->atoms; a; a = a->next)
                for (int p = 0; p < 3; p++) a->pos[p] += com[p] - ins->com[p];
            for (int p = 0; p < 3; p++) ins->com[p] = com[p];
            rotate(system, ins, system->pbc, 1.0);
            /* insert into the list, in front of the molecule it was copied from */
            if (!cp->head)
                system->molecules = ins;
            else
                cp->head->next = ins;
            ins->next = cp->molecule_altered;
            cp->molecule_altered = ins;
            cp->tail = ins->next;
            cp->molecule_backup = NULL;
            break;
        }
        case MOVETYPE_REMOVE:
            if (system->cavity_bias) { /* mc_moves.c:675-681 */
                if (get_rand(system) < pow((1.0 - system->avg_observables->cavity_bias_probability),
                                           ((double)system->cavity_grid_size * system->cavity_grid_size * system->cavity_grid_size)))
                    cp->biased_move = 0;
                else
                    cp->biased_move = 1;
            }
            energy_hip_note_list_changed(system);
            system->movable_valid = 0;
            /* remove 'altered' from the list */
            if (!cp->head)
                system->molecules = system->molecules->next;
            else
                cp->head->next = cp->tail;
            free_molecule(system, cp->molecule_altered);
            cp->molecule_altered = NULL;
            break;
        case MOVETYPE_SPINFLIP: /* mc_moves.c:721-726: no coordinate changes */
            if (get_rand(system) < 0.5)
                cp->molecule_altered->nuclear_spin = NUCLEAR_SPIN_PARA;
            else
                cp->molecule_altered->nuclear_spin = NUCLEAR_SPIN_ORTHO;
            break;
        default:
            translate(system, cp->molecule_altered, system->pbc, system->move_factor);
            rotate(system, cp->molecule_altered, system->pbc, system->rot_factor);
            energy_hip_note_moved(system, cp->molecule_altered, cp->molecule_altered);
    }
}

/* undo make_move() and pick the next move (reference restore(), mc_moves.c:744-807) */
void restore(system_t *system) {
    checkpoint_t *cp = system->checkpoint;
    memcpy(system->observables, cp->observables, sizeof(observables_t));
    switch (cp->movetype) {
        case MOVETYPE_INSERT:
            energy_hip_note_list_changed(system);
            system->movable_valid = 0;
            /* take altered out of the list */
            if (!cp->head)
                system->molecules = system->molecules->next;
            else
                cp->head->next = cp->tail;
            free_molecule(system, cp->molecule_altered);
            cp->molecule_altered = NULL;
            break;
        case MOVETYPE_REMOVE:
            energy_hip_note_list_changed(system);
            system->movable_valid = 0;
            /* put backup back into the list */
            if (!cp->head)
                system->molecules = cp->molecule_backup;
            else
                cp->head->next = cp->molecule_backup;
            cp->molecule_backup->next = cp->tail;
            cp->molecule_backup = NULL;
            break;
        case MOVETYPE_VOLUME:
            revert_volume_change(system);
            break;
        default:
            if (cp->molecule_altered) {
                /* link the backup into the working list again */
                if (!cp->head)
                    system->molecules = cp->molecule_backup;
                else
                    cp->head->next = cp->molecule_backup;
                cp->molecule_backup->next = cp->tail;
                /* the device still holds the rejected coordinates; the backup takes the altered node's place */
                energy_hip_note_moved(system, cp->molecule_backup, cp->molecule_altered);
                if (system->movable_valid) { /* the backup takes the altered molecule's place in the table too */
                    const int k = cp->altered_index;
                    system->movable[k] = cp->molecule_backup;
                    if (k + 1 < system->nmovable && system->movable_prev[k + 1] == cp->molecule_altered)
                        system->movable_prev[k + 1] = cp->molecule_backup;
                }
                free_molecule(system, cp->molecule_altered);
                cp->molecule_altered = NULL;
                cp->molecule_backup = NULL;
            }
    }
    checkpoint(system);
}

/* reference boltzmann_factor(), src/mc/mc.c:37-135: NVT, NPT, and UVT with and without cavity bias (one sorbate type) */
void boltzmann_factor(system_t *system, double initial_energy, double final_energy) {
    const double delta_energy = final_energy - initial_energy;
    double bf = exp(-delta_energy / system->temperature);
    if (system->ensemble == ENSEMBLE_UVT) {
        const double fugacity = system->fugacity;
        /* if biased_move is not set no cavity was available: the normal evaluation below (mc.c:53-77) */
        if (system->cavity_bias && system->checkpoint->biased_move) {
            if (system->checkpoint->movetype == MOVETYPE_INSERT)
                bf = (system->cavity_volume * system->avg_nodestats->cavity_bias_probability * fugacity * ATM2REDUCED /
                      (system->temperature * system->observables->N)) *
                     exp(-delta_energy / system->temperature);
            else if (system->checkpoint->movetype == MOVETYPE_REMOVE)
                bf = (system->temperature * (system->observables->N + 1.0)) /
                     (system->cavity_volume * system->avg_nodestats->cavity_bias_probability * fugacity * ATM2REDUCED) *
                     exp(-delta_energy / system->temperature);
        } else if (system->checkpoint->movetype == MOVETYPE_INSERT)
            bf = system->pbc->volume * fugacity * ATM2REDUCED / (system->temperature * (double)(system->observables->N)) *
                 exp(-delta_energy / system->temperature);
        else if (system->checkpoint->movetype == MOVETYPE_REMOVE)
            bf = system->temperature * ((double)(system->observables->N) + 1.0) /
                 (system->pbc->volume * fugacity * ATM2REDUCED) * exp(-delta_energy / system->temperature);
    } else if (system->ensemble == ENSEMBLE_NPT && system->checkpoint->movetype == MOVETYPE_VOLUME) { /* mc.c:116-129 */
        const double v_old = system->checkpoint->observables->volume;
        const double v_new = system->observables->volume;
        bf = exp(-(delta_energy + system->pressure * ATM2REDUCED * (v_new - v_old) -
                   (system->observables->N + 1) * system->temperature * log(v_new / v_old)) /
                 system->temperature);
    }
    /* mc.c:95-96, :108-109: the rotational partition function ratio of the flipped molecule */
    if (system->checkpoint->movetype == MOVETYPE_SPINFLIP && system->checkpoint->molecule_altered)
        bf = system->checkpoint->molecule_altered->rot_partfunc * exp(-delta_energy / system->temperature);
    system->nodestats->boltzmann_factor = bf;
}

/* reference write_observables(), src/io/output.c:988-1006 */
void write_observables(FILE *fp, system_t *system, observables_t *o, double core_temp) {
    fprintf(fp, "%d %f %f %f %f %f %f %f %f %f %f %f\n", system->step, o->energy, o->coulombic_energy, o->rd_energy,
            o->polarization_energy, o->vdw_energy, o->kinetic_energy, o->temperature, o->N, o->spin_ratio, o->volume,
            core_temp);
    fflush(fp);
}

/* one walker's record in the gather at corrtime (the reference packs observables_t + avg_nodestats_t, mc.c:417-428) */
typedef struct {
    observables_t observables;
    double polarization_iterations;
    avg_nodestats_t avg_nodestats;
} walker_record_t;

/* each walker's running means over its steps (reference update_nodestats(), src/io/average.c:55-80; the reference's
 * function-static counter is avg_nodestats->steps here, one per walker) */
void update_nodestats(nodestats_t *nodestats, avg_nodestats_t *avg_nodestats) {
    const int counter = ++avg_nodestats->steps;
    const double factor = ((double)(counter - 1)) / ((double)(counter));
    avg_nodestats->cavity_bias_probability =
        factor * avg_nodestats->cavity_bias_probability + nodestats->cavity_bias_probability / ((double)counter);
    avg_nodestats->cavity_bias_probability_sq =
        factor * avg_nodestats->cavity_bias_probability_sq +
        nodestats->cavity_bias_probability * nodestats->cavity_bias_probability / ((double)counter);
}

/* at every corrtime, in front of the loop over the walkers (average.c:351-376) */
void clear_avg_nodestats(system_t *system) {
    system->avg_nodestats->counter = 0;
    system->avg_observables->cavity_bias_probability = 0;
    system->avg_observables->cavity_bias_probability_sq = 0;
}

/* ... and once per walker inside it (average.c:378-400): the mean over the walkers of their running means */
void update_root_nodestats(system_t *system, avg_nodestats_t *avg_nodestats, avg_observables_t *avg_observables) {
    const double m = (double)(++system->avg_nodestats->counter);
    const double factor = (m - 1.0) / m;
    avg_observables->cavity_bias_probability =
        factor * avg_observables->cavity_bias_probability + avg_nodestats->cavity_bias_probability / m;
    avg_observables->cavity_bias_probability_sq =
        factor * avg_observables->cavity_bias_probability_sq + avg_nodestats->cavity_bias_probability_sq / m;
}

static void update_averages(system_t *system, const observables_t *o, double polarization_iterations) {
    avg_observables_t *a = system->avg_observables;
    const double m = a->counter / (a->counter + 1.0), f = 1.0 / (a->counter + 1.0); /* running mean, average.c:213-229 */
    a->energy = m * a->energy + f * o->energy;
    a->energy_sq = m * a->energy_sq + f * o->energy * o->energy;
    a->coulombic_energy = m * a->coulombic_energy + f * o->coulombic_energy;
    a->rd_energy = m * a->rd_energy + f * o->rd_energy;
    a->polarization_energy = m * a->polarization_energy + f * o->polarization_energy;
    a->polarization_iterations = m * a->polarization_iterations + f * polarization_iterations;
    a->counter += 1.0;
}

/* implements the Markov chain */
int mc(system_t *system) {
    double initial_energy, final_energy;
    char linebuf[MAXLINE];
    system->observables->volume = system->pbc->volume;
    system->observables->temperature = 0;

    /* update the grid for the first time (mc.c:245): there is no device context yet and nothing reads this call's
     * results -- make_move() updates again before any use -- so it only takes the draws of its darts */
    if (system->cavity_bias) energy_hip_cavity_update(system);

    /* get the initial energy of the system */
    system->step = 0;
    initial_energy = energy(system);
    if (energy_hip_failed(system)) return -1; /* device failure: not a property of the configuration */
    /* solve for the rotational energy levels (mc.c:253-256) */
    if (system->quantum_rotation && quantum_system_rotational_energies(system)) return -1;
    /* one process per GPU started by a plain launcher: MPMC_HIP_RANK / MPMC_HIP_NRANKS / MPMC_HIP_ID_FILE name the
     * walker (the reference's `rank`, `size`: main.c:45-52); the communicator lives on the device energy() chose */
    const int size = getenv("MPMC_HIP_NRANKS") ? atoi(getenv("MPMC_HIP_NRANKS")) : 1;
    const int rank = getenv("MPMC_HIP_RANK") ? atoi(getenv("MPMC_HIP_RANK")) : 0;
    if (walkers_init_from_env(system) < 0) return -1;
    walker_record_t snd, *rcv = calloc(size > 0 ? size : 1, sizeof(walker_record_t));
    if (!rcv) return -1;
    /* be a bit forgiving of the initial state */
    if (!isfinite(initial_energy)) initial_energy = system->observables->energy = MAXVALUE;

    if (!rank && system->energy_output[0] && !system->fp_energy) {
        system->fp_energy = fopen(system->energy_output, "w");
        if (!system->fp_energy) {
            error("MC: could not open files\n");
            return -1;
        }
        fprintf(system->fp_energy,
                "#step #energy #coulombic #rd #polar #vdw #kinetic #kin_temp #N #spin_ratio #volume #core_temp\n");
    }
    /* average in the initial values once (root only, as mc.c:276-279) */
    if (!rank) update_averages(system, system->observables, system->nodestats->polarization_iterations);
    if (system->fp_energy) write_observables(system->fp_energy, system, system->observables, system->temperature);

    /* save the initial state */
    checkpoint(system);

    /* main MC loop */
    for (system->step = 1; system->step <= system->numsteps; (system->step)++) {
        /* restore the last accepted energy */
        initial_energy = system->observables->energy;
        /* perturb the system */
        make_move(system);
        /* calculate the energy change */
        final_energy = energy(system);
        if (energy_hip_failed(system)) { /* a device / ABI failure is never turned into a rejected move */
            error("MC: the device engine failed, stopping the chain\n");
            free(rcv);
            return -1;
        }
        /* solve for the rotational energy levels (mc.c:304-308) */
        if (system->quantum_rotation && system->checkpoint->movetype == MOVETYPE_SPINFLIP &&
            quantum_system_rotational_energies(system)) {
            error("MC: the device engine failed, stopping the chain\n");
            free(rcv);
            return -1;
        }
        /* treat a bad contact as a reject */
        if (!isfinite(final_energy)) {
            system->observables->energy = MAXVALUE;
            system->nodestats->boltzmann_factor = 0;
        } else
            boltzmann_factor(system, initial_energy, final_energy);

        /* Metropolis function */
        const int volume_move = system->checkpoint->movetype == MOVETYPE_VOLUME; /* mc.c:160-190 */
        const int spinflip_move = system->checkpoint->movetype == MOVETYPE_SPINFLIP;
        if ((get_rand(system) < system->nodestats->boltzmann_factor) && (system->iter_success == 0)) {
            checkpoint(system);
            ++system->nodestats->accept;
            if (volume_move)
                ++system->nodestats->accept_volume;
            else if (spinflip_move)
                ++system->nodestats->accept_spinflip;
            else
                ++system->nodestats->accept_displace;
        } else {
            system->iter_success = 0; /* reset the polar iterative failure flag */
            restore(system);
            ++system->nodestats->reject;
            if (volume_move)
                ++system->nodestats->reject_volume;
            else if (spinflip_move)
                ++system->nodestats->reject_spinflip;
            else
                ++system->nodestats->reject_displace;
        }
        system->nodestats->acceptance_rate =
            (double)system->nodestats->accept / (double)(system->nodestats->accept + system->nodestats->reject);
        /* each node calculates its stats (mc.c:362) */
        update_nodestats(system->nodestats, system->avg_nodestats);

        /* do this every correlation time */
        if (!(system->step % system->corrtime)) {
            /* every walker's record to every rank (mc.c:431 MPI_Gather; here an all-gather over xGMI), then the
             * head node averages walker by walker and writes one line per walker (mc.c:443-476) */
            memset(&snd, 0, sizeof(snd));
            snd.observables = *system->observables;
            snd.polarization_iterations = system->nodestats->polarization_iterations;
            snd.avg_nodestats = *system->avg_nodestats;
            if (walkers_gather(system, &snd, (int)sizeof(snd), rcv) < 0) {
                free(rcv);
                return -1;
            }
            if (!rank) {
                clear_avg_nodestats(system); /* mc.c:438: avoid double-counting */
                for (int j = 0; j < size; j++) {
                    if (system->fp_energy)
                        write_observables(system->fp_energy, system, &rcv[j].observables, system->temperature);
                    update_root_nodestats(system, &rcv[j].avg_nodestats, system->avg_observables);
                    update_averages(system, &rcv[j].observables, rcv[j].polarization_iterations);
                }
            }
        }
    }
    free(rcv);
    snprintf(linebuf, MAXLINE, "MC: %d steps, acceptance rate %.4f, <E> = %.6f K\n", system->numsteps,
             system->nodestats->acceptance_rate, system->avg_observables->energy);
    output(linebuf);
    return 0;
}
