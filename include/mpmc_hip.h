/*
 * mpmc_hip.h -- C ABI of the MI355X (gfx950) per-step energy engine for MPMC.
 *
 * This is the drop-in boundary for the reference's `double energy(system_t*)`
 * hot path (reference src/energy/energy.c:67-226).  Plain C types only: the
 * reference's C host code (src/energy/energy.c, where `#ifdef CUDA` spawns
 * `polar_cuda()` today, energy.c:108-129 and :181-186) binds these entry points
 * directly; INTEGRATION.md shows the patch.  The same library is what the
 * repo's own host layer (mpmc_amd/host/ directory, mirroring system_t/energy()) and the Python
 * tests (ctypes) call.
 *
 * Conventions
 *   - every call returns 0 on success, <0 on error (message: mpmc_hip_last_error());
 *     mirrors the reference plugin's "print and carry on" only in that nothing aborts
 *     (reference src/polarization_gpu/polar_cuda_pcg.cu:205-219).
 *   - SCF non-convergence is NOT an error: result.iter_success = 1, the reference's
 *     (misnamed) failure flag (reference src/polarization/thole_iterative.c:199-210),
 *     which the caller copies to system->iter_success so mc.c:322 rejects the move.
 *   - all arithmetic fp64; units as in the reference: K, Angstrom, charges in
 *     sqrt(K*A) (e * 408.7816, reference src/io/read_pqr.c:249), alpha in A^3.
 *   - host buffers are caller-owned; the context keeps device-resident SoA copies.
 *   - one context per device and per MC walker; a context is not thread-safe.
 *   - there is NO CPU fallback: every entry point fails if no gfx950 device is usable.
 */
#ifndef MPMC_HIP_H
#define MPMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPMC_HIP_ABI_VERSION 1

typedef struct mpmc_hip_ctx mpmc_hip_ctx;
typedef struct mpmc_hip_comm mpmc_hip_comm;

/* Run-time switches.  Field names are the reference's config keywords
 * (reference src/io/input.c:437-1255, defaults :1598-1667). */
typedef struct mpmc_hip_params {
    double temperature;        /* temperature (K); Feynman-Hibbs needs it                        */
    int rd_only;               /* rd_only: skip electrostatics and polarization (energy.c:108,149) */
    int rd_lrc;                /* rd_lrc (default 1): LJ long-range correction (lj.c:56-107)     */
    int feynman_hibbs;         /* feynman_hibbs (lj.c:11-54, coulombic.c:115-146)                */
    int feynman_hibbs_order;   /* feynman_hibbs_order: 2 or 4                                    */
    int ewald_alpha_set;       /* ewald_alpha given explicitly (input.c:1093-1096)               */
    double ewald_alpha;        /* else 3.5 / cutoff (pbc.c:73-74)                                */
    int ewald_kmax;            /* ewald_kmax (default 7, defines.h:61)                           */
    int polarization;          /* polarization on (Thole, iterative solver, exponential damping) */
    double polar_damp;         /* polar_damp (lambda, e.g. 2.1304)                               */
    int polar_max_iter;        /* polar_max_iter (default 10); must be 0 if polar_precision > 0  */
    double polar_precision;    /* polar_precision in Debye (thole_iterative.c:104)               */
    double polar_gamma;        /* polar_gamma (default 1): pre-conditioning / SOR / ESOR weight  */
    int polar_gs;              /* polar_gs: Gauss-Seidel in atom order                           */
    int polar_gs_ranked;       /* polar_gs_ranked: Gauss-Seidel in ranked order (pairs.c:337-360)*/
    int polar_sor;             /* polar_sor                                                      */
    int polar_esor;            /* polar_esor                                                     */
    int polar_palmo;           /* polar_palmo: Palmo-Krimm extra contraction                     */
    int polar_rrms;            /* polar_rrms: report dipole RRMS                                 */
    int polar_zodid;           /* polar_zodid: dipoles = alpha*E, no iteration                   */
    int polar_wolf;            /* polar_wolf: Wolf static field (thole_field.c:71-124)           */
    double polar_wolf_alpha;   /* polar_wolf_alpha (a.k.a. polar_wolf_damp)                      */
    int polar_ewald;           /* polar_ewald: Ewald static field (polar_ewald.c:38-174)         */
    int polar_ewald_alpha_set; /* polar_ewald_alpha given explicitly                             */
    double polar_ewald_alpha;  /* else 3.5 / cutoff (pbc.c:75-76)                                */
    int wolf;                  /* wolf: Wolf-summation electrostatics instead of Ewald (coulombic.c:269-308) */
} mpmc_hip_params;

/* What energy() leaves in system->observables / nodestats (structs.h:152-162),
 * plus the split of the Ewald sum and a status word. */
typedef struct mpmc_hip_result {
    double energy;              /* observables->energy              */
    double rd_energy;           /* observables->rd_energy           */
    double coulombic_energy;    /* observables->coulombic_energy    */
    double polarization_energy; /* observables->polarization_energy */
    double es_real, es_recip, es_self;
    double dipole_rrms;         /* observables->dipole_rrms         */
    double volume, cutoff, ewald_alpha, polar_ewald_alpha;
    int polar_iterations;       /* nodestats->polarization_iterations */
    int iter_success;           /* system->iter_success (1 = SCF FAILED to converge) */
    int n_atoms;
    int status;                 /* 0 ok; bit 0: non-finite energy */
} mpmc_hip_result;

/* Device time of the last mpmc_hip_energy() by kernel class, from HIP events
 * recorded on the engine's own streams (milliseconds; count = launches). */
typedef struct mpmc_hip_timings {
    float pair_ms;        /* LJ + real-space Ewald pair kernel           */
    float recip_ms;       /* reciprocal-space structure factors          */
    float field_ms;       /* Thole static field                          */
    float amatrix_ms;     /* A-matrix build (HBM-write bound)            */
    float sweep_ms;       /* all dipole sweeps (HBM-read bound)          */
    float palmo_ms;       /* Palmo-Krimm contraction                     */
    float other_ms;       /* rank metric, reductions, finalisation       */
    float total_ms;       /* first launch to last kernel end             */
    int sweep_count;      /* number of sweep launches inside sweep_ms    */
    int amatrix_count;
    int graph_steps;      /* energy() calls replayed as a HIP graph so far (option "step_graph") */
    float event_pair_ms;  /* calibration: summed elapsed time of EMPTY event pairs (two records, nothing  */
    int event_pair_count; /* between): what an event pair adds to the kernel it brackets               */
    int spec_rank_redos;  /* polar_gs_ranked: calls repeated because the ranked walk assumed at enqueue time was
                           * not the one the new ranking metric gives (cumulative)              */
    int resident_calls;   /* energy() calls whose dipole solve ran as one resident launch (option "resident_jacobi";
                           * cumulative)                                                                       */
    int resident_fallbacks; /* such calls that were repeated on the multi-launch path because a hand-off of the
                           * resident kernel timed out (the device was shared); the context then stays there    */
    int pending_sweeps;   /* sweeps of the last evaluation's fixed-count Jacobi solve that are not launched yet: U_pol
                           * does not need them, mpmc_hip_download_dipoles() launches them (state, not a measurement) */
} mpmc_hip_timings;

const char *mpmc_hip_last_error(void);
int mpmc_hip_abi_version(void);
int mpmc_hip_device_count(void);

/* Persistent context (replaces the per-call cudaMalloc/cublasCreate/free of the
 * reference plugin, polar_cuda_pcg.cu:221-401).  max_atoms bounds every later upload. */
int mpmc_hip_create(mpmc_hip_ctx **ctx, int device, int max_atoms);
void mpmc_hip_destroy(mpmc_hip_ctx *ctx);

/* Engine knobs, for A/B measurement.  None changes what is computed; "pair_coefficients" and
 * "symmetric_sweep" change the rounding of the sweep sums (1e-15 relative), the others are bit-neutral
 * (tests/test_gpu_parity.py compares them bit for bit).
 *   "pair_coefficients"   (default 1): Jacobi/SOR/ESOR/Palmo sweeps run on {c3, c5} per pair (16 B) with the
 *                          geometry rebuilt in registers; 0 = on the expanded (3N)^2 A matrix (72 B per pair);
 *   "incremental_amatrix" (default 1): after mpmc_hip_update_atoms() rewrite only the entries (coefficients,
 *                          or block-rows/-columns of A) of pairs that involve a moved atom instead of rebuilding;
 *   "incremental_pairs"   (default 1): the 64x64-atom tile partial sums of the LJ/Ewald pair kernel and of the
 *                          static field (and, under disp_expansion, of the dense repulsion / dispersion tile kernel) persist between
 *                          calls; only tiles of moved atoms' blocks are recomputed;
 *   "overlap_streams"     (default 1): run the LJ/Ewald kernels on a second HIP stream beside the
 *                          polarization chain;
 *   "side_after"          (default 1; at least 1): the LJ/Ewald stream is fed after this many sweeps have been enqueued;
 *   "symmetric_sweep"     (default 1; with pair_coefficients = 0): sweeps read only the upper triangle of A and
 *                          use every element for both products; 0 = full-matrix sweep; 2 = also below 2048 atoms;
 *   "sym_mode"            (default 0): symmetric sweep on A: bit 0 = alternate the sweep direction, bit 1 = default-policy loads;
 *   "timing"              (default 1): 0 = record no HIP events; 1 = the sweep kernels (pair_sweep_kernel /
 *                          gs_chain_kernel) of every 32nd call ("timing_interval" changes the 32) are launched with a
 *                          start / stop event pair that carries the dispatch's own begin / end timestamps; 2 = time
 *                          every kernel class of every call (an event pair recorded AROUND a launch costs ~5
 *                          microseconds of stream time);
 *   "timing_interval"     (default 32; at least 1): timing 1 / -1 sample every this many calls;
 *   "persistent_gs"       (default 1): Gauss-Seidel lower-triangle phase as one persistent launch (gs_chain_kernel:
 *                          a workgroup per 64-atom block in ticket order, cached block inverses, pair coefficients);
 *                          0 = the literal forward substitution on the expanded matrix, two launches per block;
 *   "speculative_ranking" (default 1): polar_gs_ranked calls are enqueued for the ranked walk of the previous call
 *                          and checked on the device (repeated with the host sorting when the metric changed);
 *                          0 = the host sorts the ranking metric in every call;
 *   "fuse_tensor"         accepted and ignored (round 2's A/B switch for the expanded sub-diagonal tiles, which the chain
 *                          kernel no longer uses: it holds P_t = M_t D T(t,t-1), built in the block-inverse launch);
 *   "gs_lags"             (default 3; 2 .. 4): how many of a block's most recent sources the chain kernel takes from cached
 *                          matrices L(k)_t = M_t D T(t,t-k) (k = 1: main workgroup's registers, k >= 2: one auxiliary workgroup
 *                          each) instead of from the pair coefficients; rounding of the sweep differs at 1e-13 between values; the
 *                          count belongs to a VIEW: one that is rebuilt as a whole in three consecutive calls (the evaluation of
 *                          an upload counts) uses min(2, gs_lags) from the third on, and the option's value again from the first whole
 *                          rebuild that does not directly follow another -- the ranked view of a grand-canonical chain, whose atom-order view keeps its prefix and the option's
 *                          value, and both views of a context with incremental_amatrix = 0;
 *   "gs_build_fork"       (default 1): the chain-data rebuild of the main stream's view runs on a stream of its own beside the
 *                          step's next launches (views of 24+ blocks; 2 = always, 0 = in the main stream; bit-neutral);
 *   "gs_side_waves"       (default 0): the OTHER view's incremental rebuild in the side stream takes the fastest workgroup geometry
 *                          that leaves the concurrently running chain kernel its compute units; 16 = always 16-wave workgroups (bit-neutral);
 *   "rank_view_side"      (default 1): polar_gs_ranked calls in which the host sorts the metric (after a grand-canonical
 *                          edit, or when the speculated walk was wrong): the ranked view is (re)built on the side
 *                          stream beside the first sweep instead of on the main stream behind it (0 = main; A/B);
 *   "gs_fold_upper"       (default 1): the chain kernel's workgroups add up pair_upper_kernel's row sums of their own
 *                          blocks (0 = pair_upper_finish_kernel as a launch of its own in front of every chain launch);
 *   "gs_fold_finish"      (default 1): the chain kernel's workgroups do the end-of-sweep bookkeeping of their own block
 *                          (0 = gs_finish_kernel as a launch of its own behind every chain launch; A/B; same bits);
 *   "rank_late"           (default 1): in a speculative polar_gs_ranked call the side stream's ranking kernels and
 *                          ranked-view maintenance are enqueued behind the first sweep's launches, so the main stream's
 *                          own first kernels are not kept waiting for the host (0 = in front; 2 = the metric's four kernels behind the
 *                          main stream's first launches, the view maintenance behind the sweep: measured the same; A/B);
 *   "resident_jacobi"     (default 1): fixed-count Jacobi / SOR / ESOR / Palmo solves of views of up to 21 blocks
 *                          (1 344 polarizable sites) run as ONE launch with the coefficient tiles held in registers
 *                          (jacobi_resident_kernel); a launch that gives up on a hand-off (device shared with another
 *                          process) makes energy_end() repeat the call launch by launch and keeps the context there
 *                          (mpmc_hip_timings.resident_fallbacks); 0 = one sweep + one finish launch per iteration;
 *   "resident_fold"       (default 16): views of up to this many blocks run that launch WITHOUT finisher workgroups
 *                          (jacobi_folded_kernel: every tile workgroup finishes its own two blocks, one hand-off per
 *                          sweep instead of two); 0 = a finisher workgroup per block at every size (A/B; same bits);
 *   "resident_side"       (default 0): 1 = the LJ/Ewald stream is fed before the resident launch instead of behind it (A/B);
 *   "sweep_alternate"     (default 1): pair_sweep_kernel walks each XCD's tiles forwards / backwards in alternate sweeps;
 *   "sweep_nt"            (default -1): coefficient loads of the sweep non-temporal (1), default policy (0), or
 *                          non-temporal only when the tile set exceeds the Infinity Cache (-1);
 *   "sweep_split"         (default -1): half-tile workgroups in pair_sweep_kernel: 1 always, 0 never, -1 by size (A/B);
 *   "fuse_moves"          (default 1): a single-molecule move is applied inside the coefficient update of the step
 *                          (update_coef_moves_kernel) instead of by a launch of its own;
 *   "gs_fuse_moves"       (default 1): Gauss-Seidel modes on the chain kernel: the move rides in the coefficient update of
 *                          view 0 as well (0 = apply_moves_kernel + update_coef_kernel; A/B; same bits);
 *   "fuse_field"          (default 1): ... and both ride in a third z-slice of the incremental static-field launch
 *                          (field_coef_kernel): the step's first launch does the move, the coefficient update and the
 *                          field; 0 = update_coef_moves_kernel as a launch of its own (A/B; same bits);
 *   "fuse_recip"          (default 1): the reciprocal-space partial structure factors ride in a second z-slice of the
 *                          pair kernel's launch (pair_recip_kernel) when both passes cover the same blocks; 0 =
 *                          recip_partial_kernel as a launch of its own (A/B; same bits);
 *   "split_record"        (default 1): in the Jacobi-type polarizable modes the LJ / Ewald stream publishes its own
 *                          slots of the result record (sequence number of its own), so the main stream does not wait
 *                          for it in front of its publish launch; 0 = join event + one record (A/B; same bits);
 *   "side_moves"          (default 1): in such a step the LJ / Ewald stream's pair kernel applies the same move for itself
 *                          (both streams write the same coordinates, neither reads a moved atom from memory), so no event
 *                          is recorded between the main stream's first two launches; where the move is applied by
 *                          apply_moves_kernel (Gauss-Seidel modes, precision mode) the side stream runs that kernel too, in
 *                          front of its first launch; 0 = fork event (A/B; same bits);
 *   "resident_stamps" / "sweep_ablate": diagnostics (in-kernel time line of the resident launch; timing-only ablations
 *                          of the sweep: results are wrong); "resident_fault": test hook (a lost hand-off);
 *   "gs_stamps"           diagnostic: the next `value` Gauss-Seidel sweeps print in-kernel time stamps per block;
 *   "inv_stamps"          diagnostic: the next `value` block-inverse launches of the main stream print in-kernel time stamps;
 *   "gs_ablate"           timing-only ablations of the chain kernel (results are wrong; tools/gs_ablate.py);
 *   "gs_fault_sweep"      test hook: in sweep number `value` of a call one block is never published (the call must
 *                          fail with a hand-off error, tests/test_gpu_parity.py);
 *   "step_graph"          (default 0): replay a steady-state MC step as a HIP graph (bit-identical; measured
 *                          slower than direct launches on ROCm 7.2);
 *   "cavity_incremental"  (default 1): 0 = mpmc_hip_cavity_update() answers 1 to every non-empty edit (A/B; same bits).
 *                          A knob of the cavity grid, kept with the grid's state: it touches nothing of an evaluation;
 *   "trial_batched"       (default 1): 0 = mpmc_hip_trial_energies() takes its serial path in every mode (A/B, and the
 *                          batched path's check).  A knob of that entry, like the one above: it touches nothing of an
 *                          evaluation, and setting it does not count as a change since the last energy(). */
int mpmc_hip_set_option(mpmc_hip_ctx *ctx, const char *name, int value);

void mpmc_hip_default_params(mpmc_hip_params *p);
int mpmc_hip_set_params(mpmc_hip_ctx *ctx, const mpmc_hip_params *p);

/* basis: rows = lattice vectors, row-major [3][3] (system->pbc->basis, input.c:1527-1561).
 * pbc_cutoff = 0 => half the shortest lattice vector (pbc.c:13-34). */
int mpmc_hip_set_box(mpmc_hip_ctx *ctx, const double basis[9], double pbc_cutoff);

/* NPT volume move (mc_moves.c:168-210) and its revert (:213-248) on the resident configuration:
 * new basis (+ pbc_cutoff as in set_box) and one displacement per molecule, in upload order;
 * every atom of molecule m becomes pos + delta[m] -- the very addition volume_change() does.
 * Nothing is uploaded again and the call does not wait for the device.  Return 0 = done; 1 = the resident
 * molecules are no longer those of the upload (insert_molecule / remove_molecule since): upload the whole
 * configuration again; < 0 = error (evaluation in flight, nothing uploaded, wrong n_molecules, bad box). */
int mpmc_hip_scale_box(mpmc_hip_ctx *ctx, const double basis[9], double pbc_cutoff,
                       int n_molecules, const double *delta /* [n_molecules][3] */);

/* Full configuration, atoms in the reference's list order (molecule after molecule).
 * molecule[i]: id of the molecule; a molecule is a contiguous run of equal ids.
 * mass[i]: atomic mass (amu); molecular masses are summed here (pairs.c:364-385). */
int mpmc_hip_upload(mpmc_hip_ctx *ctx, int n, const double *x, const double *y, const double *z,
                    const double *charge, const double *polarizability, const double *epsilon,
                    const double *sigma, const double *mass, const int *molecule, const uint8_t *frozen);

/* disp_expansion, the PHAHST force-field family (reference src/energy/disp_expansion.c:40-103, mixing pairs.c:142-193):
 * rd_energy = sum over ALL pairs that are neither on one molecule, nor frozen-frozen, nor null (one of the four epsilon /
 * sigma values 0 AND all six c6 / c8 / c10 0) -- there is no cutoff in this sum -- of
 *     315.7750382111558 exp(-b_ij (r - rho_ij)) - f6 c6_ij / r^6 - f8 c8_ij / r^8 - f10 c10_ij / r^10
 * at the minimum-image distance r, plus the long-range correction under rd_lrc.  The per-atom epsilon of the upload is
 * the exponent b (1/A), the per-atom sigma the range rho (A).  Field names are the reference's keywords:
 *   disp_expansion           1 = this potential instead of Lennard-Jones; 0 = back to Lennard-Jones (arrays ignored);
 *   damp_dispersion          f_n = Tang-Toennies damping 1 - exp(-x) sum_{k<=n} x^k / k!, x = b_ij r, exactly 0 unless
 *                            > 1e-9; 0 = f_n = 1;
 *   extrapolate_disp_coeffs  c10_ij = (49/40) c8_ij^2 / c6_ij (0 when c6_ij or c8_ij is 0) instead of the mixed c10;
 *   schmidt_mixing           b_ij = (b_i + b_j) b_i b_j / (b_i^2 + b_j^2) instead of 2 b_i b_j / (b_i + b_j).
 * rho_ij = (rho_i + rho_j) / 2; c6_ij = sqrt(c6_i c6_j) * 0.021958709 / 3.166811429e-6 (c8: 0.0061490647, c10:
 * 0.0017219135).  There is no Feynman-Hibbs term in this potential (feynman_hibbs still acts on the Ewald real term). */
typedef struct mpmc_hip_disp_params {
    int disp_expansion;
    int damp_dispersion;
    int extrapolate_disp_coeffs;
    int schmidt_mixing;
} mpmc_hip_disp_params;

/* c6 / c8 / c10: per atom, in upload order, in atomic units (as a PQR file carries them); n = the upload's atom count.
 * Called after mpmc_hip_upload(); a later upload without it returns the context to Lennard-Jones.  update_atoms,
 * scale_box, energy_begin / _end and several contexts work as before; in this mode insert_molecule / remove_molecule
 * answer 1 (upload the whole configuration again). */
int mpmc_hip_set_dispersion(mpmc_hip_ctx *ctx, const mpmc_hip_disp_params *p, int n, const double *c6, const double *c8,
                            const double *c10);

/* axilrod_teller, the triple-dipole three-body dispersion term (reference src/energy/axilrod_teller.cpp:85-179; added to
 * potential_energy at energy.c:194 and reported as observables->three_body_energy).  The sum runs over every unordered
 * triple of distinct atoms that are not all three on one molecule -- frozen atoms included, no cutoff -- with three
 * independent minimum images d_ij, d_ik, d_jk (which need not close a triangle in a periodic box; kept as the reference has it):
 *     E_ijk = c9_ijk (1 - 3 (e_ij.e_ik)(e_ij.e_jk)(e_ik.e_jk)) / (r_ij r_ik r_jk)^3,        e = d / r,
 *     c9_ijk = a_i a_j a_k * 3 / (a_i^3 / c9_i + a_j^3 / c9_j + a_k^3 / c9_k) * 0.0032539449 / 3.166811429e-6,
 * a = polarizability * 6.7483345; exactly 0 when one of the three polarizabilities or coefficients is 0.
 * c9: per atom, in upload order, in atomic units, n = the upload's atom count.  It is the EFFECTIVE coefficient: under the
 * reference's midzuno_kihara_approx the caller passes 3/4 * polarizability * 6.7483345 * c6 in its place.  The
 * polarizabilities are the upload's; a negative one is an error.  Called after mpmc_hip_upload(), independent of
 * mpmc_hip_set_dispersion(); enable = 0 (c9 ignored), or a later upload without this call, switches the term off.
 * While it is on, mpmc_hip_result.energy includes the term (a non-finite term sets status bit 0), insert_molecule /
 * remove_molecule answer 1 (upload the whole configuration again), and update_atoms, scale_box, energy_begin / _end
 * and several contexts work as before: after a move only the block triples that hold a moved block are summed again,
 * with the bits of a from-scratch evaluation. */
int mpmc_hip_set_axilrod_teller(mpmc_hip_ctx *ctx, int enable, int n, const double *c9);
/* observables->three_body_energy of the last completed energy() / energy_end(); 0 while the term is off. */
int mpmc_hip_get_three_body_energy(mpmc_hip_ctx *ctx, double *out);

/* rd_crystal, Lennard-Jones summed over lattice images beyond the minimum image (reference src/energy/lj.c:109-276).
 * order = rd_crystal_order: 0 switches the mode off, 1 .. 4 switch it on; anything else is an error.  With
 * cutoff_c = 2.0 * cutoff * ((double)order - 0.5) (cutoff: mpmc_hip_result.cutoff) and n in {-(order-1) .. order-1}^3,
 * rd_energy becomes the sum of
 *   - the pair part: every unordered pair that is not frozen-frozen, same-molecule pairs included, with
 *     rimg - 1e-12 < cutoff_c: 4 eps_ij (s12 - s6), s6 = sum_n (|sigma_ij| / r_n)^6 over the images with
 *     !(r_n > cutoff_c), r_n from the RAW resident coordinates pos_i - pos_j + n.basis (not the minimum image: moving
 *     a molecule by a lattice vector changes the sum, as in the reference), n = 0 skipped for a same-molecule pair;
 *     under feynman_hibbs lj_fh_corr once per pair, with the summed terms, at rimg;
 *   - the self part: every atom (frozen ones included) with its own images n != 0, |n.basis| <= cutoff_c, half weight;
 *   - with rd_lrc the long-range correction evaluated at cutoff_c.
 * The decision `r_n > cutoff_c` is taken in fp64 in the reference's operation order, so an image exactly at the cutoff
 * counts here when it counts there.  The mixing is the Lennard-Jones path's.
 * A setting of the context like mpmc_hip_set_params(): it carries no per-atom data and persists across uploads.  Not
 * allowed between energy_begin() and energy_end().  energy() refuses the combination with disp_expansion
 * (mpmc_hip_set_dispersion), whose sum in the reference ignores rd_crystal.  While it is on, insert_molecule /
 * remove_molecule answer 1 (upload the whole configuration again); update_atoms, scale_box, energy_begin / _end,
 * several contexts, rd_only, polarization, Ewald / Wolf and axilrod_teller work as before, and after a move only the
 * tiles of the moved atoms' blocks are summed again, with the bits of a from-scratch evaluation. */
int mpmc_hip_set_rd_crystal(mpmc_hip_ctx *ctx, int order);

/* The pair potentials of the reference's energy() beside plain Lennard-Jones (src/energy/energy.c:132-145), and the
 * Lennard-Jones mixing rules of pairs.c:84-211.  With r the minimum-image distance and sigma_ij, eps_ij the mixed values,
 * rd_energy becomes a dense sum over the unordered pairs that are not frozen-frozen of
 *   MPMC_HIP_RD_SG             Silvera-Goldman (sg.c:13-91): every pair with r < cutoff, same-molecule pairs included; the
 *                              per-atom eps / sigma are not read.  x = r / 0.529177249,
 *                              U = exp(1.713 - 1.5671 x - 0.00993 x^2) - (12.14/x^6 + 215.2/x^8 + 4813.9/x^10 - 143.1/x^9) f,
 *                              f = exp(-(8.321/x - 1)^2) for x < 8.321, else 1; under feynman_hibbs the second-order term
 *                              of sg.c:56-72 as written there (whatever feynman_hibbs_order says; mass of the molecule of
 *                              the pair's first atom); times 3.15774655e5.  In this form energy() computes what it computes
 *                              under rd_only: coulombic_energy = polarization_energy = 0 (energy.c:108, :154).
 *                              OWNED DEVIATION: the reference sums uninitialised distances for frozen-frozen pairs here.
 *   MPMC_HIP_RD_DREIDING       exp-6, gamma = 12 (dreiding.c:13-108): pairs with !(r > cutoff) that are not rd-excluded;
 *                              eps_ij (t - 2 (r / sigma_ij)^-6), t = 0 for an attractive-only pair, 1e40 for
 *                              r < 0.4 sigma_ij, else exp(12 (1 - r / sigma_ij)).  1e40 is finite: it is passed through.
 *   MPMC_HIP_RD_BUFFERED_14_7  Halgren's buffered 14-7 (lj_buffered_14_7.c:6-35): the same pairs;
 *                              eps_ij (1.07 / (rho + 0.07))^7 (1.12 / (rho^7 + 0.12) - 2), rho = r / sigma_ij.
 *   MPMC_HIP_RD_LJ             Lennard-Jones as lj.c:165-276 has it without rd_crystal -- r - 1e-12 < cutoff, attractive-only
 *                              pairs, lj_fh_corr at order 2 or 4, under rd_lrc the pair correction with the MIXED values
 *                              and the self correction with the atom's own -- so that the mixing rules reach it.  With
 *                              MPMC_HIP_RD_MIX_LB it restates the standard path (dense, without its screen).
 * rd-excluded is the standard path's rule: same molecule, or one of the four per-atom eps / sigma is 0.  DREIDING and the
 * buffered 14-7 have no Feynman-Hibbs term and no long-range correction, as in the reference.
 * mixing, evaluated per pair on the device from the upload's per-atom eps / sigma:
 *   MPMC_HIP_RD_MIX_LB              Lorentz-Berthelot, |sigma| and attractive-only for a negative sigma (pairs.c:200-211)
 *   MPMC_HIP_RD_MIX_WALDMAN_HAGLER  sigma_ij = ((s_i^6 + s_j^6) / 2)^(1/6), eps_ij = sqrt(e_i e_j) 2 s_i^3 s_j^3 / (s_i^6 + s_j^6)
 *   MPMC_HIP_RD_MIX_HALGREN         sigma_ij = (s_i^3 + s_j^3) / (s_i^2 + s_j^2), eps_ij = 4 e_i e_j / (sqrt e_i + sqrt e_j)^2,
 *                                   each 0 unless both values are > 0
 *   MPMC_HIP_RD_MIX_C6              sigma_ij = (s_i + s_j) / 2, eps_ij = 64 sqrt(e_i e_j) s_i^3 s_j^3 / (s_i + s_j)^6
 * form = 0 returns to the standard path, whose results keep their bits.  A setting of the context like
 * mpmc_hip_set_rd_crystal(): it carries no per-atom data and persists across uploads; not allowed between energy_begin()
 * and energy_end().  While a form is on, insert_molecule / remove_molecule answer 1 (upload the whole configuration
 * again); update_atoms, scale_box, energy_begin / _end, several contexts and axilrod_teller work as before, and after a
 * move only the tiles of the moved atoms' blocks are summed again, with the bits of a from-scratch evaluation.  energy()
 * refuses, by name: a form together with disp_expansion, rd_crystal or polarvdw; MPMC_HIP_RD_MIX_WALDMAN_HAGLER with a
 * negative sigma in the upload (the reference never assigns such a pair's epsilon); MPMC_HIP_RD_SG with a mixing other than
 * MPMC_HIP_RD_MIX_LB (the reference ignores the mixing there). */
enum {
    MPMC_HIP_RD_LJ = 1,
    MPMC_HIP_RD_SG = 2,
    MPMC_HIP_RD_DREIDING = 3,
    MPMC_HIP_RD_BUFFERED_14_7 = 4
};
enum {
    MPMC_HIP_RD_MIX_LB = 0,
    MPMC_HIP_RD_MIX_WALDMAN_HAGLER = 1,
    MPMC_HIP_RD_MIX_HALGREN = 2,
    MPMC_HIP_RD_MIX_C6 = 3
};
typedef struct mpmc_hip_rd_form_params {
    int form;   /* 0 = the standard path, or MPMC_HIP_RD_* */
    int mixing; /* MPMC_HIP_RD_MIX_* */
} mpmc_hip_rd_form_params;
int mpmc_hip_set_rd_form(mpmc_hip_ctx *ctx, const mpmc_hip_rd_form_params *p);

/* polarvdw (alias cdvdw), the coupled-dipole many-body van der Waals term (reference src/energy/vdw.c:579-632; added to
 * potential_energy at energy.c:194 and reported as observables->vdw_energy; not computed under rd_only):
 *     vdw_energy = e_total - e_iso + lr_corr.
 * With k_i = sqrt(polarizability_i) * omega_i, the atoms with k_i != 0 and K = diag(k), C = K A K is formed from the FULL
 * Thole matrix A -- diagonal blocks 1 / alpha_i, off-diagonal blocks the exponentially damped (polar_damp) dipole tensor at
 * the minimum-image distance; no cutoff; same-molecule and frozen-frozen pairs included -- and
 *     e_total = 4.13412763705e16 * 3.81911146e-12 * sum_i sqrt(max(lambda_i(C), 0))       (negative eigenvalues clipped);
 *     e_iso   = sum over the molecules, in upload order, of the same expression for the molecule's own diagonal sub-block
 *               of C, evaluated ONCE per type id, on the first molecule of the type the context sees, and kept while the
 *               mode stays on (kept as the reference has it: a later molecule of the type with another geometry still
 *               takes the first one's value);
 *     lr_corr = under rd_lrc, over every unordered pair that is not frozen-frozen, same-molecule pairs included, whose
 *               alpha_i, alpha_j, omega_i, omega_j are all non-zero: -4/3 pi cC / cutoff^3 / volume with
 *               cC = 1.5 * 7.63822291e-12 * w_i w_j / (w_i + w_j) * 4.13412763705e16 * a_i a_j.
 * In this mode Lennard-Jones is repulsion only (lj.c:230-231): rd_energy = sum over the Lennard-Jones pairs of
 * 4 eps_ij (sigma_ij / r)^12, plus under rd_lrc (16/9) pi eps sigma^3 (sigma / cutoff)^9 / volume per pair and per atom
 * (lj.c:77-78, :100-101).  The eigenvalues come from a Householder tridiagonalisation and Sturm-count bisection on the
 * device; the matrix is rebuilt from the resident positions in every call.
 * omega: per atom, in upload order, in atomic units (PQR column 15).  mol_type[i]: an id that is equal for all atoms of all
 * molecules of one type.  The polarizabilities (a negative one is an error) and the molecules are the upload's.  Called
 * after mpmc_hip_upload(); enable = 0 (arrays ignored), or a later upload without this call, switches the mode off and
 * returns the context to Lennard-Jones; the e_iso values survive a new upload as long as set_vdw(enable = 1) follows it
 * before the next energy().  While the mode is on, mpmc_hip_result.energy includes the term (a non-finite term sets status
 * bit 0), insert_molecule / remove_molecule answer 1 (upload the whole configuration again), and update_atoms, scale_box,
 * energy_begin / _end, several contexts, Ewald / Wolf and every solver mode work as before.  energy() refuses the
 * combinations with mpmc_hip_set_dispersion, mpmc_hip_set_rd_crystal, mpmc_hip_set_axilrod_teller and feynman_hibbs. */
int mpmc_hip_set_vdw(mpmc_hip_ctx *ctx, int enable, int n, const double *omega, const int *mol_type);
/* observables->vdw_energy of the last completed energy() / energy_end(); 0 while the mode is off. */
int mpmc_hip_get_vdw_energy(mpmc_hip_ctx *ctx, double *out);
/* Its parts, and the mode's rd_energy parts: e_total, e_iso, lr_corr, the repulsion pair sum, the repulsion long-range
 * correction (pair + self); zeros while the mode is off. */
int mpmc_hip_get_vdw_terms(mpmc_hip_ctx *ctx, double terms[5]);

/* The exact Thole dipoles (polar_iterative off, reference src/energy/polar.c:91-95): A mu = E_static is solved directly, by
 * a blocked fp64 Cholesky factorization of the polarizable sites' matrix on the device and two substitutions
 * (kernels_exact.h), instead of iteratively.  enable = 0 returns to the iterative solvers.  A setting
 * of the context like mpmc_hip_set_rd_crystal(): it persists across uploads; not allowed between energy_begin() and
 * energy_end().  While it is on:
 *   - polarization_energy = -1/2 sum mu . E_static of the solution, polar_iterations = 0, dipole_rrms = 0, and
 *     download_dipoles() gives ef_induced and ef_induced_change as zeros (the reference leaves them untouched);
 *   - polar_gs, polar_gs_ranked, polar_sor, polar_esor, polar_gamma, polar_max_iter and polar_precision are ignored, and
 *     set_params() accepts a set with neither polar_max_iter nor polar_precision;
 *   - energy() refuses polar_zodid, polar_palmo and polarvdw (mpmc_hip_set_vdw) by name;
 *   - insert_molecule / remove_molecule answer 1 (upload the whole configuration again); update_atoms, scale_box,
 *     energy_begin / _end and several contexts work as before, with the bits of a from-scratch evaluation;
 *   - the work copy of the matrix, (3 nvpad)^2 doubles beside the resident matrix of the same size, is allocated at the
 *     first energy(); if it does not fit, energy() fails and names the byte count.
 * OWNED DEVIATION: a matrix that is not positive definite (a polarization catastrophe) has no Cholesky factor.  The
 * reference's pivoted LU would return numbers; this engine reports iter_success = 1 (the reference's "solver failed", on
 * which the Monte Carlo driver rejects the move) and gives the iterative solvers' divergence fallback mu = alpha E_static
 * with U_pol from those.  The flag is that call's alone.  mpmc_hip_timings in this mode: sweep_ms / sweep_count are the
 * trailing-update kernels, palmo_ms (option "timing" 2) the whole solve. */
int mpmc_hip_set_exact_polar(mpmc_hip_ctx *ctx, int enable);
/* The molecular polarizability tensor of the reference's `polarizability_tensor on` (thole_polarizability.c:27-37),
 * out[3 p + q] = sum_ij (A^-1)[3i+p][3j+q] in A^3, from three unit-field right-hand sides on the factor of the last
 * completed energy() (the inverse is never formed).  An error, by name, while the exact mode is off, before an energy()
 * with polarization has completed in it, or when that call's matrix was not positive definite. */
int mpmc_hip_get_polarizability_tensor(mpmc_hip_ctx *ctx, double out[9]);

/* The dipole tensor of the A matrix (reference thole_amatrix(), thole_matrix.c:90-135): T = c3 I - 3 c5 d d^T with
 *   damp_type 2 (exponential, the default): c3 = damp1/r^3, c5 = damp2/r^5, damp1 = 1 - e^{-lr}(l^2r^2/2 + lr + 1),
 *                 damp2 = damp1 - e^{-lr} l^3r^3/6, l = polar_damp;
 *   damp_type 1 (linear, Thole's original): s = polar_damp (alpha_i alpha_j)^(1/6), v = r/s; for r < s damp1 = (4 - 3v) v^3
 *                 and damp2 = v^4, otherwise both 1 (a site with alpha = 0 gives s = 0: undamped);
 *   damp_type 0 (off / none, Applequist): damp1 = damp2 = 1, but 0 for a pair the reference calls es_excluded: two atoms
 *                 of one molecule, or a pair in which either charge is exactly 0.0 (pairs.c:61-77; the quirk is kept);
 *                 set_params() then accepts polar_damp <= 0 (check_input.c:406-409);
 *   wolf_full (polar_wolf_full; damp_type 2 only): c3 = damp1/r^3 - wdamp1/rc^3, c5 = damp2/r^5 - wdamp2/(r^2 rc^3) with
 *                 wdamp = damp at r = rc = the box cutoff, for EVERY pair (the reference has no r < rc test there), and
 *                 the static field is the Wolf field whether or not polar_wolf is set (thole_field.c:32).
 * The values of damp_type are the reference's (DAMPING_OFF / _LINEAR / _EXPONENTIAL).  A setting of the context like
 * mpmc_hip_set_rd_crystal(): it persists across uploads, the default is {2, 0}, and it is not allowed between
 * energy_begin() and energy_end().  Changing it drops the coefficient store, the expanded matrix and the chain data.
 * Refused by name: wolf_full with a damp_type other than 2; at energy(), a non-default model while polarvdw
 * (mpmc_hip_set_vdw) is on -- the reference's e2body() / calc_e_iso() are written for the exponential form. */
typedef struct mpmc_hip_thole_model {
    int damp_type; /* 0 off, 1 linear, 2 exponential */
    int wolf_full; /* polar_wolf_full */
} mpmc_hip_thole_model;
int mpmc_hip_set_thole_model(mpmc_hip_ctx *ctx, const mpmc_hip_thole_model *m);

/* cavity_autoreject_absolute (reference energy.c:48-64): with scale = cavity_autoreject_scale > 0 every energy() also
 * counts the pairs of atoms on DIFFERENT molecules -- frozen-frozen pairs included -- whose minimum-image distance is
 * < scale, the distance and the comparison in the reference's fp64 operation order.  0 = off.  A setting of the context
 * like mpmc_hip_set_rd_crystal(): it persists across uploads and is usable in every mode.  The engine only counts: what
 * the reference does on a non-zero count (return MAXVALUE, leave the observables, count the rejection) is the caller's.
 * The count of the last completed energy() / energy_end() is valid whatever the other terms came out as -- a close contact
 * routinely makes the repulsion, and can make the coupled-dipole term, non-finite (status bit 0): energy_end() still
 * returns 0 and the count is that of the configuration. */
int mpmc_hip_set_autoreject(mpmc_hip_ctx *ctx, double scale);
int mpmc_hip_get_close_contacts(mpmc_hip_ctx *ctx, long long *count);

/* cavity_bias (reference src/mc/cavity.c:17-179): the cavity grid.  With G = cavity_grid_size and P = G^3, grid point
 * g = (i G + j) G + k sits at the fractional coordinates ((i+1)/(G+1), (j+1)/(G+1), (k+1)/(G+1)) - 1/2 of the cell,
 *     pos[p] = ((b[0][p] c0 + b[1][p] c1) + b[2][p] c2) - 0.5 b[0][p] - 0.5 b[1][p] - 0.5 b[2][p]
 * evaluated left to right in fp64 without contraction.  occupancy[g] = the number of binned positions w with
 * sqrt(((gx-wx)^2 + (gy-wy)^2) + (gz-wz)^2) < cavity_radius -- no minimum image: the caller passes the reference's
 * wrapped_pos -- decided exactly as a correctly rounded sqrt decides (the device compares the square with the smallest
 * double T whose square root is >= cavity_radius).  A point is open when its occupancy is 0; a dart hits when it is closer
 * than cavity_radius, in the same sense, to some open point.
 * The grid is state of the context, independent of the atom slots: upload, update_atoms, insert / remove and energy()
 * leave it alone; the caller names the positions that are binned, that leave and that enter.  set_box / scale_box move
 * the points and invalidate the occupancy.  None of these calls is allowed between energy_begin() and energy_end().
 *   set_cavity_grid   grid_size 1 .. 64 and cavity_radius > 0 switch the grid on (a larger grid_size is refused by name);
 *                     grid_size 0 switches it off.  A setting like mpmc_hip_set_rd_crystal(): it persists across uploads.
 *                     The occupancy is invalid until the next cavity_bin.
 *   cavity_bin        the from-scratch occupancy of these n positions (n = 0 is valid); replaces what was there.
 *   cavity_update     first the edit: occupancy += (in points within the radius) - (out points within it), n_out = n_in =
 *                     0 allowed; then the list of the open points in ascending g and its length *cavities_open; then
 *                     the darts (dart_xyz [n_darts][3], n_darts = 0 allowed): *hits = how many of them hit.
 *                     Return 0 = done; 1 = cannot be done incrementally (more than 16 points either way, option
 *                     "cavity_incremental" 0 with a non-empty edit, or no valid occupancy): cavity_bin the current
 *                     positions and call again with an empty edit; < 0 = error.
 *   cavity_point      the index-th open point of the last cavity_update, by flat index and position; an index outside
 *                     [0, cavities_open) is an error.
 *   download_cavity_grid  occupancy [P] and pos [P][3], for tests and tools; either pointer may be NULL, not both.
 * Option "cavity_incremental" (default 1; mpmc_hip_set_option): 0 = cavity_update answers 1 to every non-empty edit (A/B). */
int mpmc_hip_set_cavity_grid(mpmc_hip_ctx *ctx, int grid_size, double radius);
int mpmc_hip_cavity_bin(mpmc_hip_ctx *ctx, int n, const double *x, const double *y, const double *z);
int mpmc_hip_cavity_update(mpmc_hip_ctx *ctx, int n_out, const double *out_xyz, int n_in, const double *in_xyz,
                           int n_darts, const double *dart_xyz, int *cavities_open, int *hits);
int mpmc_hip_cavity_point(mpmc_hip_ctx *ctx, int index, int *grid_index, double pos[3]);
int mpmc_hip_download_cavity_grid(mpmc_hip_ctx *ctx, int *occupancy, double *pos);

/* New coordinates for atoms [first, first+count): the delta after one MC move
 * (make_move perturbs one molecule, mc_moves.c:567). */
int mpmc_hip_update_atoms(mpmc_hip_ctx *ctx, int first, int count, const double *x, const double *y,
                          const double *z);

/* Grand-canonical moves (mc_moves.c:583-697) without a re-upload: one molecule of `count` atoms enters or
 * leaves the resident configuration.  The engine keeps its own atom order: an inserted molecule gets the
 * slots [*first_slot, *first_slot + count) -- a hole left by a removed molecule of the same size, or new
 * slots at the end -- and that slot range is what later update_atoms / remove_molecule calls and the
 * per-atom downloads (which span mpmc_hip_slot_count() slots, holes reading as zeros) refer to.
 * `mass` = atomic masses (the molecular mass is their sum), `frozen` applies to the whole molecule.
 * Return 0 = done; 1 = cannot be done incrementally (context full, more than 16 atoms, Gauss-Seidel on the
 * expanded matrix (persistent_gs = 0), incremental options off): upload the whole configuration again; < 0 = error.
 * In Gauss-Seidel modes follow up with mpmc_hip_set_sweep_order().
 * These two entries cannot carry the per-atom data of the dense energy modes, so they answer 1 while
 * mpmc_hip_set_dispersion(), mpmc_hip_set_axilrod_teller(), mpmc_hip_set_rd_crystal() or mpmc_hip_set_rd_form() is on,
 * and keep doing so: mpmc_hip_edit_molecules() below is the entry that edits in those modes. */
int mpmc_hip_insert_molecule(mpmc_hip_ctx *ctx, int count, const double *x, const double *y, const double *z,
                             const double *charge, const double *polarizability, const double *epsilon,
                             const double *sigma, const double *mass, int frozen, int *first_slot);
int mpmc_hip_remove_molecule(mpmc_hip_ctx *ctx, int first_slot, int count);

/* Several molecules leave and enter in one call, in every mode that has device-side edits.
 *   Removals are carried out first, in the order given (remove_first_slot[k], remove_count[k]); insertions follow, in the
 *   order given, insert_first_slot[k] receiving the first slot of insert[k].  The slot rules, the sweep-view slots and the
 *   Gauss-Seidel protocol (mpmc_hip_set_sweep_order) are those of the two entries above: called with the same molecules
 *   this entry leaves what the sequence of those calls leaves, bit for bit.
 *   A molecule brings what insert_molecule takes, and the per-atom data of the modes that are on: c6 / c8 / c10 while
 *   mpmc_hip_set_dispersion() is on (epsilon / sigma are then the exponent b and the range rho, as at the upload), and c9
 *   while mpmc_hip_set_axilrod_teller() is on -- the EFFECTIVE coefficient, as that call takes it.  Arrays of a mode that
 *   is off are not read and may be NULL.
 *   It works on the standard path, and while set_dispersion, set_axilrod_teller (beside Lennard-Jones or beside
 *   disp_expansion), set_rd_crystal or set_rd_form is on.
 * Return 0 = done; 1 = upload the whole configuration again: more than 8 removals or 8 insertions, a molecule above 16
 * atoms, no room in the context or in the sweep view, mpmc_hip_set_vdw() or mpmc_hip_set_exact_polar() on, "pair_coefficients",
 * "incremental_amatrix" or "incremental_pairs" at 0, Gauss-Seidel without the chain kernel; < 0 = error (a bad slot
 * range, a NULL array the active mode reads, a negative polarizability under axilrod_teller, a call between
 * energy_begin() and energy_end()).
 * All or nothing: whatever makes the call answer 1 or fail is decided before anything changes, and the next energy()
 * then returns what it would have returned without the call. */
typedef struct {
    int count;                 /* atoms of the molecule, 1 .. 16 */
    int frozen;
    const double *x, *y, *z, *charge, *polarizability, *epsilon, *sigma, *mass;
    const double *c6, *c8, *c10;   /* read while mpmc_hip_set_dispersion() is on, else may be NULL */
    const double *c9;              /* read while mpmc_hip_set_axilrod_teller() is on: the EFFECTIVE c9, as that call takes it */
} mpmc_hip_molecule;

int mpmc_hip_edit_molecules(mpmc_hip_ctx *ctx,
                            int nremove, const int *remove_first_slot, const int *remove_count,
                            int ninsert, const mpmc_hip_molecule *insert, int *insert_first_slot);
/* Gauss-Seidel modes (polar_gs / polar_gs_ranked) only: their result depends on the ORDER in which the atoms are
 * swept -- the order of the reference's atom_array (the molecule lists), which thole_iterative.c walks and
 * update_ranking() re-sorts stably -- and after insert / remove the engine's slot order is no longer that order.
 * The caller states it: slots[k] = device slot of the k-th POLARIZABLE atom (polarizability != 0) in its own atom
 * order.  Required after every insert_molecule / remove_molecule before the next energy() (which fails otherwise);
 * accepted and ignored in the other solver modes.  Replaces the reference's rebuild of atom_array
 * (pairs.c:388-547) for this purpose. */
int mpmc_hip_set_sweep_order(mpmc_hip_ctx *ctx, int count, const int *slots);
int mpmc_hip_slot_count(mpmc_hip_ctx *ctx);

/* Dimer scans: the energies of a NON-PERIODIC dimer of two rigid molecules for many placements at once -- the hot path of
 * the reference's `ensemble surf` (src/mc/surface.c:16-76, :289-376) and what a force-field fitting loop asks for.  Per
 * placement three numbers, as surface_energy() splits them:
 *   es     sum q_i q_j / r over the inter-molecular pairs with both charges non-zero (coulombic_nopbc, coulombic.c:198-217);
 *          0 under rd_only;
 *   rd     Lennard-Jones as lj_nopbc has it (lj.c:279-317: no cutoff, no long-range correction, no Feynman-Hibbs term,
 *          fabs(sigma)) under the mixing rule `mixing`, or under disp_expansion the PHAHST term (disp_expansion.c:105-153),
 *          over the inter-molecular pairs pair_exclusions() leaves in (pairs.c:56-78);
 *   polar  -1/2 sum mu . E_static (+ mu . ef_induced_change under polar_palmo) of the Thole system of ALL sites of both
 *          molecules: A over every pair, intra-molecular ones included, without cutoff (tensor: damp_type, as
 *          mpmc_hip_set_thole_model has it, without wolf_full); static field from the OTHER molecule's charges only
 *          (thole_field_nopbc, thole_field.c:39-68); solver of thole_iterative.c: dipoles start at alpha E polar_gamma, then
 *          Jacobi, polar_gs (order: molecule a's sites, then b's) or polar_gs_ranked (metric of pairs.c:337-359; the first
 *          sweep in list order, the later ones in stable descending order of the metric), polar_max_iter sweeps, or with
 *          polar_precision > 0 (polar_max_iter = 0) until no dipole component changed by more than polar_precision Debye;
 *          the 128th sweep is not run: the dipoles fall back to alpha E and the placement is flagged.  Sites with
 *          alpha = 0 are skipped.  0 when rd_only is set or no site is polarizable.
 * Geometry of a placement (r, alpha1, beta1, gamma1, alpha2, beta2, gamma2), surface_dimer_geometry() (surface.c:383-433)
 * applied to the PRISTINE body frames (coordinates minus the mass-weighted centre, pairs.c:364-385), without FMA
 * contraction: molecule b's centre to (r, 0, 0), then each molecule is rotated about its own centre.  The rotation matrices
 * are formed on the host with the host's cos / sin: molecule_rotate_euler() (surface.c:116-125), or with global_axis
 * molecule_rotate_quaternion() (:177-193), kept as it is: the angles are divided by 57.2957795 although the scan hands it
 * radians, and the third rotation is about x.
 * OWNED DEVIATION: the reference rotates and un-rotates the live coordinates cumulatively; every placement here starts
 * from the pristine frame.
 * A placement's numbers depend on that placement alone -- not on its place in the batch, the batch size or the form of
 * the call -- and the means of the grid form are summed in an order the grid sizes fix.
 * Both entries use the context for its device, its stream and buffers of their own: they work on a context that has had
 * no upload, and leave the resident configuration, its cached sums and the last result alone.  Not allowed between
 * energy_begin() and energy_end().  Inputs are not screened for overlapping sites: r = 0 between two sites gives the
 * reference's inf / NaN. */
typedef struct mpmc_hip_dimer_params {
    int rd_form;   /* 0 or MPMC_HIP_RD_LJ (the other forms are refused) */
    int mixing;    /* MPMC_HIP_RD_MIX_* (Lennard-Jones) */
    int disp_expansion, damp_dispersion, extrapolate_disp_coeffs, schmidt_mixing; /* as mpmc_hip_disp_params */
    int rd_only;
    int damp_type;          /* 0 off, 1 linear, 2 exponential */
    double polar_damp;
    int polar_max_iter;
    double polar_precision;
    int polar_gs, polar_gs_ranked, polar_palmo;
    double polar_gamma;
    int global_axis;        /* surf_global_axis */
} mpmc_hip_dimer_params;
void mpmc_hip_default_dimer_params(mpmc_hip_dimer_params *p);

#define MPMC_HIP_DIMER_CHUNK 256                /* placements per workgroup: the unit of the grid form's fixed-order sum */
#define MPMC_HIP_DIMER_NOT_CONVERGED 0x40000000 /* status bit: the 128-sweep give-up (dipoles = alpha E) */
#define MPMC_HIP_DIMER_MAX_CONF (1 << 20)       /* placements per list call, and rotations per molecule of a grid call */

/* List form.  a, b: 1 .. 16 sites each; x / y / z, charge, polarizability, epsilon, sigma, mass are read, c6 / c8 / c10
 * under disp_expansion (atomic units; epsilon / sigma are then the exponent b and the range rho); frozen and c9 are not.
 * conf: [nconf][7] = r, alpha1, beta1, gamma1, alpha2, beta2, gamma2.  es, rd, polar: [nconf].  status: [nconf], the
 * sweeps taken, | MPMC_HIP_DIMER_NOT_CONVERGED.  mu: NULL, or [nconf][32][3], the dipoles, a's sites first then b's, the
 * rest zeros. */
int mpmc_hip_dimer_energies(mpmc_hip_ctx *ctx, const mpmc_hip_dimer_params *p, const mpmc_hip_molecule *a,
                            const mpmc_hip_molecule *b, int nconf, const double *conf, double *es, double *rd,
                            double *polar, int *status, double *mu);
/* Grid form: one separation and six lists of angle values, angles[k][0 .. n[k]) for k = alpha1, beta1, gamma1, alpha2,
 * beta2, gamma2; the placements are their Cartesian product, the last index fastest (surface.c:306-311).  Nothing per
 * placement leaves the device.  means: es, rd, polar.  counts: [0] the placements, [1] those flagged not converged. */
int mpmc_hip_dimer_grid_means(mpmc_hip_ctx *ctx, const mpmc_hip_dimer_params *p, const mpmc_hip_molecule *a,
                              const mpmc_hip_molecule *b, double r, const int n[6], const double *const angles[6],
                              double means[3], long long counts[2]);

/* Trial placements: the total energy of the resident configuration with ONE molecule at each of ntrial placements, the
 * configuration itself left untouched -- what the reference's quantum_rotation scan takes 2 x 256 full energy() calls per
 * molecule for (rotational_eigenspectrum.c:219-266, rotational_potential.c:211-253), and what Widom insertion, multiple-try
 * and configurational-bias moves would ask for.
 *   first_slot, count   the molecule: one whole valid, non-frozen molecule of 1 .. 16 sites, by its slot range;
 *   xyz                 [ntrial][count][3], the sites of each placement in slot order.  The placements are RIGID re-placements
 *                       of the molecule (rotations, translations): its intra-molecular terms are taken from the resident result;
 *   energy              [ntrial]: what energy() would return as mpmc_hip_result.energy after update_atoms(first_slot, count,
 *                       placement t);
 *   terms               NULL, or [ntrial][3]: rd, es_real and es_recip of placement t as the batched path forms them -- the
 *                       molecule's Lennard-Jones (+ Feynman-Hibbs) and real-space Ewald / Wolf sums with every other atom, and
 *                       (4 pi / V) sum_k w_k |S_rest(k) + s_t(k)|^2.  With (rd_0, es_0, recip_0) the terms of the molecule's
 *                       CURRENT placement (pass its coordinates as a placement to read them) and E the energy of the last
 *                       energy(),   energy[t] == (E - ((rd_0 + es_0) + recip_0)) + ((rd_t + es_t) + recip_t)   in fp64, one
 *                       rounding per operation.
 * The call needs a completed energy() on the current configuration and leaves the resident configuration, every cached sum,
 * the last result record and any pending deferred sweeps as they were.  Refused by name, before anything changes: a call
 * between energy_begin() and energy_end(); ntrial < 1; an upload, move (update_atoms), edit (insert / remove / edit_molecules),
 * box change (set_box / scale_box), set_params, mode setter or evaluation option since the last completed energy(); a slot
 * range that is not one whole valid, non-frozen molecule of 1 .. 16 sites.
 * Two paths, the same numbers to 1e-12 of the sum of the magnitudes of the energy's terms:
 *   batched  the standard pair path without polarization (Lennard-Jones with Lorentz-Berthelot mixing, feynman_hibbs, Ewald /
 *            Wolf / rd_only, rd_lrc): at most 4 launches per call whatever ntrial (kernels_trial.h).
 *            A placement's bits depend on the molecule, the placement and the resident configuration -- not on ntrial or on
 *            the placement's position in the batch;
 *   serial   with polarization, disp_expansion, set_rd_form, rd_crystal, axilrod_teller, polarvdw or the exact dipoles, and
 *            whenever option "trial_batched" (default 1; mpmc_hip_set_option; setting it is no change of the evaluation) is 0:
 *            update_atoms() + energy() per placement, then the original coordinates and one more energy().  energy[t] is,
 *            bit for bit, what that public sequence returns, and the context afterwards gives the bits of one that never made
 *            the call.  terms must be NULL on this path (refused by name).
 * mpmc_hip_trial_call_count(): calls so far that passed their checks. */
int mpmc_hip_trial_energies(mpmc_hip_ctx *ctx, int first_slot, int count, int ntrial, const double *xyz, double *energy,
                            double *terms);
long long mpmc_hip_trial_call_count(mpmc_hip_ctx *ctx);

/* One full energy() evaluation on the device.
 * What has been computed when it returns: every energy term of the result, and the dipoles of all sweeps the energy
 * needs.  A fixed-count plain Jacobi solve -- polar_max_iter = n >= 2, polar_precision = 0, polar_gamma = 1, none of
 * polar_sor / polar_esor / polar_palmo / polar_rrms / polar_zodid / polar_gs / polar_gs_ranked -- on pair coefficients
 * and on a view too large for the one-launch solvers (nt (nt + 1) / 2 + nt > compute units for nt 64-site blocks: 22
 * blocks or more on MI355X) launches at most n - 1 sweeps: with T symmetric, U_pol = -1/2 sum mu_n.E is known behind
 * the finish of sweep m = ceil(n / 2).  polar_iterations is n all the same.  The n-th sweep (mu_n,
 * E_ind of mu_{n-1}) stays pending, and so do sweeps m + 1 .. n - 1 when the call published its result behind sweep m
 * (every untimed launch-by-launch call with the side stream's own record; mpmc_hip_timings.pending_sweeps says how
 * many): they are launched, in order, by the first call that reads their output or that changes what they read (below),
 * and dropped by the next energy() if nobody did.  Every other solve runs all its sweeps inside the call, as before. */
int mpmc_hip_energy(mpmc_hip_ctx *ctx, mpmc_hip_result *out);

/* The same in two halves: _begin enqueues the evaluation and returns, _end waits for it and fills the
 * result.  The reference's energy() does host-side bookkeeping that does not depend on the energies
 * (update_com(), countN(): pairs.c:331, energy.c:217); between the two calls that work overlaps the
 * device.  No upload/update_atoms/set_box/scale_box is accepted while an evaluation is in flight. */
int mpmc_hip_energy_begin(mpmc_hip_ctx *ctx);
int mpmc_hip_energy_end(mpmc_hip_ctx *ctx, mpmc_hip_result *out);

/* Per-atom vectors of the last energy(): atom->mu, ef_static, ef_induced,
 * ef_induced_change, each [n][3] (needed by write_dipole/write_field at corrtime,
 * output.c:1029-1088).  Any pointer may be NULL.
 * May launch device work beyond the copies: the last call's pending Jacobi sweeps (see mpmc_hip_energy; one sweep +
 * one finish launch each, up to n - ceil(n / 2) of them, the first time only), then the scatter to atom order.  The
 * vectors are, bit for bit, those the call would have left had it run the sweeps itself.  The pending sweeps are also
 * completed by whatever changes the device state they read while the result stays readable -- moves that are applied
 * at once (more than 32 atoms, or a full move list), mpmc_hip_set_box, mpmc_hip_scale_box, mpmc_hip_set_params, mpmc_hip_set_option,
 * mpmc_hip_download_amatrix with moves queued -- and dropped where the result itself is discarded (upload,
 * insert_molecule, remove_molecule, set_sweep_order).  Moves that are only queued (mpmc_hip_update_atoms of a
 * molecule) touch nothing: a Monte Carlo step pays nothing for it. */
int mpmc_hip_download_dipoles(mpmc_hip_ctx *ctx, double *mu, double *ef_static, double *ef_induced,
                              double *ef_induced_change);

/* system->A_matrix of the last energy(): [3n][3n] row-major (thole_matrix.c:38-146). */
int mpmc_hip_download_amatrix(mpmc_hip_ctx *ctx, double *A);

/* atom->rank_metric [n] and the final sweep order [n] (polar_gs_ranked), both over mpmc_hip_slot_count() slots.  After
 * insert / remove the order is the stable sort of the order stated by mpmc_hip_set_sweep_order(): the polarizable
 * sites appear in it in the order they were swept in (sites without polarizability and holes keep their slot's place). */
int mpmc_hip_download_ranking(mpmc_hip_ctx *ctx, double *rank_metric, int *ranked_array);

int mpmc_hip_get_timings(mpmc_hip_ctx *ctx, mpmc_hip_timings *t);

/* Walker averaging over xGMI: replaces the MPI_Gather of observables every corrtime
 * (mc.c:417-432).  id is a 128-byte RCCL unique id made on rank 0 and handed to the
 * other ranks by the caller's own launcher (MPI, torchrun env, a file). */
int mpmc_hip_comm_unique_id(unsigned char id[128]);
int mpmc_hip_comm_create(mpmc_hip_comm **comm, mpmc_hip_ctx *ctx, int nranks, int rank,
                         const unsigned char id[128]);
int mpmc_hip_comm_size(const mpmc_hip_comm *comm);
int mpmc_hip_comm_rank(const mpmc_hip_comm *comm);
/* Sum of `values[0..count)` (count <= 64) over all walkers, in place; blocking, like the MPI_Gather it replaces. */
int mpmc_hip_allreduce_observables(mpmc_hip_comm *comm, double *values, int count);
/* The same in two halves on the communicator's own stream: _begin copies `values` and starts the collective,
 * _end waits and writes the sums.  The averages are reported only, never fed back into the chain, so the
 * energy() calls of the next corrtime interval can run in between.  One collective in flight per communicator. */
int mpmc_hip_allreduce_observables_begin(mpmc_hip_comm *comm, const double *values, int count);
int mpmc_hip_allreduce_observables_end(mpmc_hip_comm *comm, double *values);
/* The MPI_Gather itself (mc.c:431: MPI_Gather(snd_strct, 1, msgtype, rcv_strct, ...)): every walker contributes a
 * record of `bytes` bytes (observables_t + avg_nodestats_t [+ histogram, sorbate info], mc.c:225-227) and receives
 * the records of all walkers in rank order -- nranks * bytes bytes -- so that whichever rank acts as root can run
 * update_root_averages() per walker (mc.c:443-476) unchanged.  An all-gather over xGMI; blocking, like the call
 * it replaces; `bytes` must be the same on every rank. */
int mpmc_hip_gather_observables(mpmc_hip_comm *comm, const void *record, int bytes, void *records);
void mpmc_hip_comm_destroy(mpmc_hip_comm *comm);

#ifdef __cplusplus
}
#endif
#endif
