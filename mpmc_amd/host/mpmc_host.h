/*
 * mpmc_host.h -- C host layer above the C ABI (include/mpmc_hip.h).
 *
 * Mirrors, for the hot path only, the reference's own host interface: the same type and field
 * names (reference src/include/structs.h: atom_t :39-83, molecule_t :85-98, pbc_t :100-105,
 * observables_t :152-162, system_t :347-513) and the same entry points
 * (`double energy(system_t*)` src/energy/energy.c:67, `int mc(system_t*)` src/mc/mc.c:196,
 * `system_t *setup_system(char*)` src/io/input.c:1739, `double get_rand(system_t*)`
 * src/mersenne/mersenne.cpp:9), so that code written against the reference reads the same here.
 * Only the fields the energy path and the NVT driver touch are present; molecules and atoms are
 * the reference's singly linked lists.  The pair list does not exist: pair geometry lives on the
 * device.
 */
#ifndef MPMC_HOST_H
#define MPMC_HOST_H

#include <stdio.h>

#include <mpmc_hip.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAXLINE 512
#define MAXVALUE 1.0e40
#define E2REDUCED 408.7816 /* reference src/include/defines.h:45 */
#define ATM2REDUCED 0.0073389366 /* convert from atm to K/A^3, defines.h:46 */

enum { ENSEMBLE_UVT, ENSEMBLE_NVT, ENSEMBLE_SURF, ENSEMBLE_SURF_FIT, ENSEMBLE_NVE, ENSEMBLE_TE, ENSEMBLE_NPT,
       ENSEMBLE_REPLAY };
enum { MOVETYPE_INSERT, MOVETYPE_REMOVE, MOVETYPE_DISPLACE, MOVETYPE_VOLUME, MOVETYPE_SPINFLIP };
enum { DAMPING_OFF, DAMPING_LINEAR, DAMPING_EXPONENTIAL }; /* defines.h:91-93 */
enum { NUCLEAR_SPIN_PARA, NUCLEAR_SPIN_ORTHO };             /* defines.h:94-95 */
/* quantum_rotation (defines.h:69-78; qrot.c) */
#define QUANTUM_ROTATION_SYMMETRIC 0
#define QUANTUM_ROTATION_ANTISYMMETRIC 1
#define QUANTUM_ROTATION_SYMMETRY_POINTS 64
#define QUANTUM_ROTATION_LEVEL_MAX 36
#define QUANTUM_ROTATION_L_MAX 5
#define QUANTUM_ROTATION_GRID 16
#define QUANTUM_ROTATION_SUM 10
#define QROT_L_LIMIT 8                                         /* the basis the reference hard-codes (rotational_basis.c) */
#define QROT_DIM_LIMIT ((QROT_L_LIMIT + 1) * (QROT_L_LIMIT + 1)) /* 81 */

typedef struct _atom {
    int id, bond_id;
    char atomtype[MAXLINE];
    int frozen;
    double mass, charge, polarizability, epsilon, sigma;
    double c6, c8, c10; /* disp_expansion: dispersion coefficients in atomic units (structs.h:54, read_pqr.c:255-257) */
    double c9;          /* axilrod_teller: three-body coefficient in atomic units (read_pqr.c:258) */
    double omega;       /* polarvdw: characteristic frequency in atomic units (structs.h, read_pqr.c:253) */
    double pos[3], wrapped_pos[3];
    double ef_static[3], ef_static_self[3], ef_induced[3], ef_induced_change[3];
    double mu[3], old_mu[3], new_mu[3];
    double dipole_rrms, rank_metric;
    struct _atom *next;
} atom_t;

typedef struct _molecule {
    int id;
    char moleculetype[MAXLINE];
    double mass;
    int frozen;
    double com[3], wrapped_com[3];
    /* quantum_rotation (structs.h:62-73): the spin isomer, the molecule's rotational partition functions and its levels.
     * Inline arrays: copy_molecule() copies them with the molecule, restore() brings them back with it.  The eigenvectors
     * are not kept (quantum_rotation_eigenvectors prints them where they are made). */
    int nuclear_spin;
    double rot_partfunc_g, rot_partfunc_u, rot_partfunc;
    double quantum_rotational_energies[QROT_DIM_LIMIT];
    int quantum_rotational_eigensymmetry[QROT_DIM_LIMIT];
    atom_t *atoms;
    struct _molecule *next;
} molecule_t;

typedef struct _pbc {
    double basis[3][3];            /* unit cell lattice (A) */
    double reciprocal_basis[3][3]; /* reciprocal space lattice (1/A) */
    double cutoff;                 /* radial cutoff (A) */
    double volume;                 /* unit cell volume (A^3) */
} pbc_t;

typedef struct _observables {
    double energy, coulombic_energy, rd_energy, polarization_energy, vdw_energy, three_body_energy;
    double dipole_rrms, kinetic_energy, temperature, volume, N, NU, spin_ratio;
} observables_t;

typedef struct _nodestats {
    int accept, reject;
    int accept_displace, reject_displace;
    int accept_volume, reject_volume; /* npt (mc.c:164-165, :189-190) */
    int accept_spinflip, reject_spinflip; /* quantum_rotation (mc.c:161-162, :186-187) */
    double boltzmann_factor, acceptance_rate, acceptance_rate_displace;
    double polarization_iterations;
    double cavity_bias_probability; /* cavity_bias: open grid points / all grid points of this step (cavity.c:85-107) */
} nodestats_t;

/* per-walker running means over the steps (structs.h:142-150, average.c:55-80) */
typedef struct _avg_nodestats {
    int counter; /* walkers averaged in at this corrtime (average.c:355, :381) */
    int steps;   /* steps averaged in: the function-static counter of the reference's update_nodestats(), here per walker */
    double cavity_bias_probability, cavity_bias_probability_sq;
} avg_nodestats_t;

typedef struct _avg_observables {
    double energy, energy_sq, coulombic_energy, rd_energy, polarization_energy, polarization_iterations;
    double counter;
    /* cavity_bias: mean over the walkers of their running means, redone at every corrtime (average.c:369-370, :398-399) */
    double cavity_bias_probability, cavity_bias_probability_sq;
} avg_observables_t;

typedef struct _checkpoint {
    int movetype, biased_move; /* biased_move: the move takes the cavity-biased acceptance (mc_moves.c:587, :675-681) */
    molecule_t *molecule_altered, *molecule_backup; /* as in the reference: the backup is a deep copy */
    molecule_t *head, *tail;                        /* neighbours of molecule_altered in the list */
    int altered_index;                              /* its rank among the movable molecules */
    observables_t *observables;
} checkpoint_t;

typedef struct _system {
    int ensemble;
    int cuda; /* kept: reference keyword `cuda on` (input.c:1245) */
    int hip;  /* keyword `hip on|off`; this layer has no CPU path, so it must stay on */
    int numsteps, corrtime, step;
    double move_factor, rot_factor, temperature, scale_charge;
    double insert_probability, pressure, fugacity; /* uvt: fugacity = user_fugacities value, else pressure */
    int user_fugacities;
    double volume_probability, volume_change_factor; /* npt (input.c:635-640; defaults 0.0 and 0.25) */
    int preset_seeds_on;
    unsigned int preset_seeds;
    int rng_initialized;
    unsigned int rng_mt[624]; /* std::mt19937 state of this walker */
    int rng_mti;
    /* energy options (reference keywords) */
    int rd_only, rd_lrc, feynman_hibbs, feynman_hibbs_order, wrapall, wolf;
    int ewald_alpha_set, ewald_kmax, polar_ewald_alpha_set;
    double ewald_alpha, polar_ewald_alpha;
    int polarizability_tensor; /* structs.h:429: print the molecular tensor after the first energy() and leave (exact dipoles only) */
    int polarization, polar_iterative, polar_ewald, polar_zodid, polar_palmo, polar_gs, polar_gs_ranked, polar_sor,
        polar_esor, polar_max_iter, polar_wolf, polar_rrms, damp_type;
    /* the dipole tensor beside damp_type (structs.h:432-433): polar_wolf_full is sent with mpmc_hip_set_thole_model(),
     * polar_ewald_full is read so that energy_hip.c can refuse it by name */
    int polar_wolf_full, polar_ewald_full;
    double polar_gamma, polar_damp, polar_precision, polar_wolf_alpha;
    /* the PHAHST family (structs.h:420-421): exp repulsion + C6 / C8 / C10 dispersion instead of Lennard-Jones; the last
     * four are read so that energy_hip.c can refuse them by name */
    int disp_expansion, extrapolate_disp_coeffs, damp_dispersion, schmidt_mixing;
    int disp_expansion_mbvdw, gilbert_smith_mixing, bohm_ahlrichs_mixing, wilson_popelier_mixing;
    /* the triple-dipole three-body term (structs.h:422); midzuno_kihara_approx: c9 = 3/4 alpha c6 per atom */
    int axilrod_teller, midzuno_kihara_approx;
    /* Lennard-Jones over lattice images (structs.h, lj.c:109-276): sent with mpmc_hip_set_rd_crystal() */
    int rd_crystal, rd_crystal_order;
    /* the other pair potentials of energy() (structs.h; sg.c, dreiding.c, lj_buffered_14_7.c) and the Lennard-Jones mixing
     * rules of pairs.c:84-211: sent with mpmc_hip_set_rd_form() */
    int sg, dreiding, lj_buffered_14_7, waldmanhagler, halgren_mixing, c6_mixing;
    /* coupled-dipole many-body van der Waals (structs.h; vdw.c): 1 = on; 2 (evects) and 3 (comp) are read so that
     * energy_hip.c can refuse them by name, like the three repulsion variants */
    int polarvdw, cdvdw_exp_repulsion, cdvdw_sig_repulsion, cdvdw_9th_repulsion;
    /* cavity_autoreject_absolute (energy.c:48-64, :99-102, :187-191): a pair of atoms on different molecules closer than
     * the scale makes energy() return MAXVALUE; count_autorejects counts those calls */
    int cavity_autoreject_absolute, count_autorejects;
    double cavity_autoreject_scale;
    /* cavity_bias (structs.h:402-406, cavity.c, mc_moves.c:577-608, :675-681, mc.c:54-77): insertions go to open points of
     * a cavity_grid_size^3 grid; the grid itself lives on the device (energy_hip_cavity_update) */
    int cavity_bias, cavity_grid_size, cavities_open;
    double cavity_radius, cavity_volume;
    /* ensemble replay (replay.c): the trajectory, whether its REMARK BOX lines set the box, and calc_pressure, which is
     * read so that replay can refuse it by name */
    int read_pqr_box_on, calc_pressure;
    char traj_input[MAXLINE];
    /* ensemble surf (structs.h; check_input.c:88-132, surface.c): the scan and its switches.  surf_virial, surf_output and
     * surf_print_level are read so that check_system() can refuse them by name, like ensemble surf_fit and nve */
    double surf_min, surf_max, surf_inc, surf_ang;
    int surf_preserve, surf_decomp, surf_global_axis_on, surf_virial, surf_print_level, surf_output_on;
    int surf_preserve_rotation_on;     /* the keyword was given: its six angles (radians) follow */
    double surf_preserve_rotation[6];  /* alpha1 beta1 gamma1 alpha2 beta2 gamma2 */
    /* quantum_rotation (structs.h:465-468, input.c:1271-1304, check_input.c:236-280): rotational levels of every movable
     * molecule in the field of the others (qrot.c), and the spin-flip move (spinflip_probability) */
    int quantum_rotation, quantum_rotation_hindered, quantum_rotation_level_max, quantum_rotation_l_max, quantum_rotation_sum;
    int quantum_rotation_eigenvectors; /* not a reference keyword: print the eigenvectors too (the reference does under DEBUG) */
    double quantum_rotation_B, quantum_rotation_hindered_barrier, spinflip_probability;
    int iter_success; /* the reference's convergence-FAILURE flag */
    int natoms;
    char job_name[MAXLINE], pqr_input[MAXLINE], energy_output[MAXLINE], pqr_output[MAXLINE];
    char pqr_restart[MAXLINE]; /* the state after the last step, as the reference's restart file has it (write_restart()) */
    pbc_t *pbc;
    molecule_t *molecules;
    observables_t *observables;
    nodestats_t *nodestats;
    avg_nodestats_t *avg_nodestats;
    avg_observables_t *avg_observables;
    checkpoint_t *checkpoint;
    double last_volume;
    /* the movable (non-frozen) molecules in list order and each one's predecessor in the list, so that
     * checkpoint() need not walk the list twice per step; rebuilt after insertions / removals */
    struct _molecule **movable, **movable_prev;
    int nmovable, movable_cap, movable_valid;
    /* (no engine fields: energy_hip.c keeps device context, residency, failure flag, communicator and timings in a
     * side table keyed by the system_t pointer -- exactly as it does inside the reference tree) */
    FILE *fp_energy;
} system_t;

/* input (reference src/io/input.c, read_pqr.c, simulation_box.c) */
system_t *setup_system(char *input_file);
system_t *read_config(char *input_file);
int do_command(system_t *system, char **token);
molecule_t *read_molecules(FILE *fp, system_t *system);
void pbc(system_t *system);
int check_cavity_bias(system_t *system); /* the cavity_bias block of check_system(): 0 = fine (or off), -1 = refused */
/* build a system from flat arrays (what tests and bench.py use instead of a PQR file) */
system_t *system_from_arrays(int n, const double *pos, const double *charge, const double *polarizability,
                             const double *epsilon, const double *sigma, const double *mass, const int *molecule,
                             const int *frozen, const double basis[9]);
void free_system(system_t *system);

/* energy (reference src/energy/energy.c; energy.c here is the dispatcher with the `hip` hook, energy_hip.c the
 * binding itself -- see energy_hip.h, included at the end of this header) */
double energy(system_t *system);
int countNatoms(system_t *system);
void update_com(molecule_t *molecules);

/* Monte Carlo (reference src/mc/mc.c, mc_moves.c, checkpoint.c, src/mersenne/mersenne.cpp) */
int mc(system_t *system);
/* ensemble replay (reference src/mc/replay.c): energy() of every frame of system->traj_input, one observables line each.
 * read_frame(): the next frame's molecules (and box, under read_pqr_box) into `system`, whose old molecules it frees;
 * 0 = a frame was read, 1 = end of the trajectory, -1 = error. */
int replay_trajectory(system_t *system);
/* ensemble surf (reference src/mc/surface.c:227-380): the dimer curve on device `device`, the reference's lines on stdout.
 * surface_refused(): NULL, or why this layer does not run the input (each reason names its keyword).
 * surface_loop_count(): how many values `for (x = 0; x <= top; x += step)` visits, in double, as the reference loops. */
int surface(system_t *system, int device);
const char *surface_refused(const system_t *system);
int surface_loop_count(double top, double step);
int read_frame(FILE *fp, system_t *system);
/* quantum_rotation (reference src/quantum_rotation/; qrot.c).  quantum_system_rotational_energies(): for every movable
 * molecule the potential on the 16 x 16 Gauss-Legendre grid -- ONE energy_hip_trial_energies() call of 256 placements, or
 * the hindered-rotor potential -- the Hamiltonian in the Y_lm basis, its levels, their g / u symmetry (random points from
 * the run's generator) and the partition functions; prints the reference's DEBUG_QROT lines.  0, or -1 when the device
 * failed.  The pieces, for tests and tools:
 *   qrot_check()         the keyword block's checks (qrot_options(), check_input.c:236-280) and this layer's refusals;
 *   qrot_placements()    xyz [256][n][3], index p * 16 + t: align_molecule() then rotate_spherical() from the unmodified
 *                        coordinates; returns the site count, -1 when no site is off the centre of mass;
 *   qrot_hamiltonian()   h [dim][dim][2] from V[t][p] (sin(theta) included), dim = (l_max + 1)^2; 0, or -1 (l_max outside
 *                        0 .. 8, or no memory for the table of Y_lm on the grid: h is not written);
 *   qrot_jacobi()        cyclic Jacobi for a complex Hermitian matrix: ascending eigenvalues, evec [dim][dim][2] with row i
 *                        the i-th eigenvector; returns the sweeps taken, -1 when 64 sweeps did not converge;
 *   qrot_symmetry()      determine_rotational_eigensymmetry() of one eigenvector (draws 128 numbers);
 *   qrot_basis()         Y_lm(theta, phi), type 0 = real part, 1 = imaginary part. */
int quantum_system_rotational_energies(system_t *system);
int qrot_check(system_t *system);
int qrot_placements(const molecule_t *molecule, double *xyz);
void qrot_grid(double theta[QUANTUM_ROTATION_GRID], double phi[QUANTUM_ROTATION_GRID], double weights[QUANTUM_ROTATION_GRID]);
void qrot_hindered_grid(double B, double barrier, double V[QUANTUM_ROTATION_GRID][QUANTUM_ROTATION_GRID]);
int qrot_hamiltonian(int l_max, double B, const double V[QUANTUM_ROTATION_GRID][QUANTUM_ROTATION_GRID], double *h);
int qrot_jacobi(int dim, const double *h, double *eval, double *evec, long *rotations);
int qrot_symmetry(system_t *system, int l_max, const double *evec);
double qrot_basis(int type, int l, int m, double theta, double phi);
/* wall time of the last evaluation's parts, summed over the molecules: scan, Hamiltonian, eigen-solve + symmetry (seconds) */
void qrot_last_times(double out[3]);
void write_observables(FILE *fp, system_t *system, observables_t *o, double core_temp);
void checkpoint(system_t *system);
void restore(system_t *system);
void make_move(system_t *system);
void boltzmann_factor(system_t *system, double initial_energy, double final_energy);
/* node statistics (reference src/io/average.c:55-80, :351-400; the cavity_bias members only) */
void update_nodestats(nodestats_t *nodestats, avg_nodestats_t *avg_nodestats);
void clear_avg_nodestats(system_t *system);
void update_root_nodestats(system_t *system, avg_nodestats_t *avg_nodestats, avg_observables_t *avg_observables);
double get_rand(system_t *system);
void seed_rng(system_t *system, unsigned int seed);
molecule_t *copy_molecule(system_t *system, molecule_t *src);
void free_molecule(system_t *system, molecule_t *molecule);
void translate(system_t *system, molecule_t *molecule, pbc_t *pbc, double scale);
void rotate(system_t *system, molecule_t *molecule, pbc_t *pbc, double scale);
void volume_change(system_t *system);        /* npt: mc_moves.c:168-210 */
void volume_change_to(system_t *system, double new_volume); /* not a reference function: volume_change() from its basis scaling on, for
                                                              * a given volume (the forced-move test entry of bench_api.c) */
void revert_volume_change(system_t *system); /* mc_moves.c:213-248 */
int wrapall(molecule_t *molecules, pbc_t *pbc);

/* output */
void output(const char *msg);
void error(const char *msg);
int write_molecules(system_t *system, const char *filename);
/* `pqr_restart`: the configuration in the layout of the reference's restart file (output.c:315-564) -- molecules numbered
 * in list order, coordinates wrapped molecule by molecule under `wrapall`, the box as REMARK BOX BASIS lines */
int write_restart(system_t *system, const char *filename);

#ifdef __cplusplus
}
#endif

#include "energy_hip.h" /* energy_hip(), the notes, the dipole download, walkers_*() */
#endif
