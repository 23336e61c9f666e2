/*
 * energy_hip.h -- what energy_hip.c exports to the rest of the host code.
 *
 * energy_hip.c is ONE source file for two trees:
 *   - the reference tree (smann95/mpmc): copied to src/energy/energy_hip.c and compiled against the
 *     reference's own <structs.h> / <function_prototypes.h>; the only change it needs in those headers is the
 *     keyword flag `int hip;` in system_t (next to `int cuda;`, structs.h:350).  tests/test_reference_binding.py
 *     compiles it exactly that way in the build container;
 *   - this repository's C host layer (mpmc_amd/host/, -DMPMC_SHIM_HOST_MIRROR), whose mpmc_host.h mirrors the
 *     reference's types for the hot path -- that build is what the GPU tests and bench.py run.
 * All engine state (device context, the host image of what the device holds, residency of molecules, the RCCL
 * communicator, failure flag, timings) lives in a side table inside energy_hip.c keyed by `system_t *`; neither
 * system_t nor molecule_t carries engine fields.
 *
 * Include AFTER the tree's struct header (this file needs system_t and molecule_t).
 */
#ifndef ENERGY_HIP_H
#define ENERGY_HIP_H

#include <mpmc_hip.h>

#ifdef __cplusplus
extern "C" {
#endif

/* energy() on the device: same contract as the reference's dispatcher (src/energy/energy.c:67-226) -- returns
 * the potential energy and fills system->observables, nodestats->polarization_iterations, iter_success, natoms,
 * last_volume.  Returns NAN with energy_hip_failed() set when the device or the ABI failed. */
double energy_hip(system_t *system);
/* the same in two halves (the second does update_com() / countN() while the device works) */
int energy_hip_begin(system_t *system);
double energy_hip_end(system_t *system);
/* Device / ABI failure of the last energy_hip(): its own channel, NOT a Monte Carlo reject.  mc() looks here
 * right after energy() and stops; only a call that succeeded and produced a non-finite energy is a bad contact
 * (src/mc/mc.c:315-318). */
int energy_hip_failed(system_t *system);
/* NULL when the device computes everything this system asks of energy(), else the reason it is refused */
const char *energy_hip_unsupported(const system_t *system);

/* Optional notes from mc_moves.c (worth one list walk per step): molecule `now` sits in the list where `was`
 * sat when the device last saw it -- make_move()'s displacement: (altered, altered); restore()'s relinked
 * backup: (molecule_backup, molecule_altered).  Insertions / removals / anything else: _list_changed().
 * Without these calls energy_hip() walks the lists on every call and finds the differences itself. */
void energy_hip_note_moved(system_t *system, molecule_t *now, molecule_t *was);
void energy_hip_note_list_changed(system_t *system);
/* volume_change() / revert_volume_change() (npt): every molecule was shifted rigidly; delta_per_molecule[3 * k + i] is
 * what was added to coordinate i of the atoms of the k-th molecule of the list (copied; the caller keeps its array).
 * The next energy_hip() then moves the resident configuration into the new box (mpmc_hip_scale_box) instead of
 * uploading everything again.  Without this note a changed volume means a full upload, as before. */
void energy_hip_note_volume_change(system_t *system, const double *delta_per_molecule);
/* on = 0: volume notes are ignored (the full upload of an un-hooked caller; for A/B measurement and tests) */
void energy_hip_set_volume_notes(system_t *system, int on);

/* How energy_hip() has kept the device in line with the lists since the first call: out[0] full uploads, out[1] calls of
 * mpmc_hip_edit_molecules() that were carried out (grand-canonical insertions / removals without a re-upload), out[2]
 * molecules those calls removed + inserted. */
void energy_hip_sync_counts(system_t *system, long out[3]);
/* quantum_rotation: the total energies of the configuration the device holds with `molecule` (a movable molecule of the
 * lists, as of the last energy_hip()) at ntrial placements xyz [ntrial][natoms][3] -- mpmc_hip_trial_energies() on its
 * slots.  Needs a completed energy_hip() on the lists as they are.  0, or -1 with energy_hip_failed() set.
 * energy_hip_trial_calls(): such calls so far. */
int energy_hip_trial_energies(system_t *system, molecule_t *molecule, int ntrial, const double *xyz, double *energy);
long energy_hip_trial_calls(system_t *system);
/* the per-atom c9 the engine is given: as read, or 3/4 alpha 6.7483345 c6 under midzuno_kihara_approx */
double energy_hip_effective_c9(int midzuno_kihara_approx, double alpha, double c6, double c9);

/* atom->mu / ef_static / ef_induced / ef_induced_change as polar() leaves them; called where the reference
 * reads them (write_dipole() / write_field() at corrtime, src/mc/mc.c:398-414) instead of on every step */
int energy_hip_download_dipoles(system_t *system);
/* everything the reference's per-step pairs() / polar() leave behind for the writers of a corrtime block
 * (mc.c:366-414): wrapped coordinates (pairs.c:334) and, with polarization, the per-atom vectors above.
 * A fixed-count Jacobi solve of n sweeps leaves up to n - ceil(n / 2) of them to this call (the engine launches them
 * when the dipoles are asked for: mpmc_hip_timings.pending_sweeps), so a driver pays them once per corrtime block */
int energy_hip_corrtime(system_t *system);

/* `polarizability_tensor on` with polar_iterative off: the molecular polarizability tensor of the last energy_hip(),
 * tensor[3 p + q] in A^3; print != 0 also writes the reference's block (thole_polarizability.c:50-70) to stdout.  The reference
 * prints it inside the first polar() and leaves with die(0); here the driver calls this after its first energy() and
 * returns 0.  Non-zero: no context, or the engine refused (its message goes to error()). */
int energy_hip_polarizability_tensor(system_t *system, double tensor[9], int print);

/* cavity_bias: cavity_update_grid() (src/mc/cavity.c:112-179) on the device, for the accepted configuration the lists hold
 * at the top of make_move().  Draws the 3 * (int)(0.1 V) numbers of cavity_volume()'s darts with get_rand() in the
 * reference's order, wraps only the molecules that changed since its last call (their wrapped_pos is wrapall()'s), sends
 * the difference to the engine's grid (mpmc_hip_cavity_update) or bins everything again when the engine asks for it, and
 * fills system->cavities_open, system->cavity_volume and nodestats->cavity_bias_probability.  Before the first
 * energy_hip() (mc.c:245) it takes the draws only.  A device / ABI failure is reported by the next energy_hip() through
 * energy_hip_failed(): it never becomes a rejected move. */
int energy_hip_cavity_update(system_t *system);
/* the position of the index-th open grid point of that call in (i, j, k) order: what make_move()'s scan of cavity_grid
 * (mc_moves.c:590-606) gives the biased insertion as centre of mass */
int energy_hip_cavity_point(system_t *system, int index, double com[3]);
/* that call's dart positions ([n][3], owned by the binding) and hit count; returns n (tests, tools) */
int energy_hip_cavity_darts(system_t *system, const double **darts, int *hits);

/* cleanup() (src/main/cleanup.c): destroys the device context and the side table entry */
void energy_hip_cleanup(system_t *system);

/* plumbing */
void energy_hip_set_device(system_t *system, int device); /* default: rank % device count (mirror: 0) */
mpmc_hip_ctx *energy_hip_context(system_t *system);       /* NULL before the first energy_hip() */
double energy_hip_last_energy(system_t *system);          /* the last energy_hip()'s return value (a rejected trial's too) */
void energy_hip_enable_timing(system_t *system, int on);
void energy_hip_get_timings(system_t *system, mpmc_hip_timings *out);
void energy_hip_profile_report(void);

/* Walker averaging over xGMI (replaces MPI_Gather / MPI_Type_contiguous of src/mc/mc.c:230-231, :431-432).
 * walkers_unique_id() on rank 0, the launcher hands the 128 bytes round, walkers_init() on every rank after its
 * first energy() (the communicator lives on the engine's device).
 * walkers_gather(): every rank contributes `msgsize` bytes (the snd_strct of mc.c:417-428) and receives all
 * ranks' records in rank order (the rcv_strct of mc.c:431) -- an all-gather, so any rank may act as root.
 * walkers_pool_begin/_end(): sum of a short vector of doubles over all walkers, asynchronous. */
int walkers_unique_id(unsigned char id[128]);
int walkers_init(system_t *system, int nranks, int rank, const unsigned char id[128]);
/* the same for a process started once per GPU by a plain launcher (no MPI): MPMC_HIP_NRANKS, MPMC_HIP_RANK and
 * MPMC_HIP_ID_FILE in the environment; rank 0 makes the id and publishes it through that file (written under a
 * temporary name, then renamed), the others wait for it (MPMC_HIP_ID_TIMEOUT seconds, default 120).  Returns 0
 * and does nothing when MPMC_HIP_NRANKS is unset or 1. */
int walkers_init_from_env(system_t *system);
int walkers_gather(system_t *system, const void *snd_strct, int msgsize, void *rcv_strct);
int walkers_pool_begin(system_t *system, const double *values, int count);
int walkers_pool_end(system_t *system, double *values, int count);
void walkers_finalize(system_t *system);

#ifdef __cplusplus
}
#endif
#endif
