"""ctypes binding of the C host layer (mpmc_amd/host/libmpmc_host.so): system_t, energy(), mc() -- the mirror
of the reference's host interface that sits above the C ABI.  Plumbing for tests and bench.py."""
import ctypes as C
import os

import numpy as np

from . import engine

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPMC_HOST_LIB: the sanitizer build (make -C mpmc_amd/host asan) for tests/run_asan.sh
LIB_PATH = os.environ.get("MPMC_HOST_LIB") or os.path.join(_HERE, "host", "libmpmc_host.so")
EXE_PATH = os.path.join(_HERE, "host", "mpmc_hip")

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("mpmc_amd/host/libmpmc_host.so is not built (run __graft_entry__.build())")
    engine.load()  # libmpmc_hip.so first (also found through the rpath)
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.system_from_arrays.restype = vp
    lib.system_from_arrays.argtypes = [C.c_int] + [vp] * 9
    lib.setup_system.restype = vp
    lib.setup_system.argtypes = [C.c_char_p]
    lib.free_system.argtypes = [vp]
    lib.free_system.restype = None
    lib.host_apply_config.argtypes = [vp, C.c_char_p]
    lib.host_mc_steps.argtypes = [vp, C.c_int]
    lib.host_set_device.argtypes = [vp, C.c_int]
    lib.host_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    lib.host_enable_timing.argtypes = [vp, C.c_int]
    lib.host_get_timings.argtypes = [vp, C.POINTER(engine.Timings)]
    lib.host_get_observables.argtypes = [vp, vp]
    lib.host_get_positions.argtypes = [vp, vp]
    lib.host_get_dipoles.argtypes = [vp, vp, vp, vp]
    lib.host_natoms.argtypes = [vp]
    lib.host_get_system.argtypes = [vp] * 9
    lib.host_seed.argtypes = [vp, C.c_uint]
    lib.host_mc_steps_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    lib.host_mc_steps_multi.restype = C.c_int
    lib.host_get_rand.argtypes = [vp]
    lib.host_get_rand.restype = C.c_double
    lib.energy.argtypes = [vp]
    lib.energy.restype = C.c_double
    lib.mc.argtypes = [vp]
    lib.countNatoms.argtypes = [vp]
    lib.translate.argtypes = [vp, vp, vp, C.c_double]
    lib.checkpoint.argtypes = [vp]
    lib.make_move.argtypes = [vp]
    lib.restore.argtypes = [vp]
    lib.walkers_unique_id.argtypes = [vp]
    lib.walkers_init.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.walkers_pool_begin.argtypes = [vp, vp, C.c_int]
    lib.walkers_pool_end.argtypes = [vp, vp, C.c_int]
    lib.walkers_finalize.argtypes = [vp]
    lib.walkers_finalize.restype = None
    lib.host_device_error.argtypes = [vp]
    lib.host_get_basis.argtypes = [vp, vp]
    lib.host_get_basis.restype = None
    lib.host_get_npt.argtypes = [vp, vp]
    lib.host_get_npt.restype = None
    lib.host_set_volume_notes.argtypes = [vp, C.c_int]
    lib.host_set_volume_notes.restype = None
    lib.host_force_volume_move.argtypes = [vp, C.c_double, C.c_int]
    lib.host_force_volume_move.restype = None
    lib.host_init_chain_no_energy.argtypes = [vp]
    lib.host_init_chain_no_energy.restype = None
    lib.host_get_disp_flags.argtypes = [vp, vp]
    lib.host_get_disp_flags.restype = None
    lib.host_get_dispersion.argtypes = [vp, vp, vp, vp]
    lib.host_get_dispersion.restype = None
    lib.host_set_dispersion.argtypes = [vp, vp, vp, vp]
    lib.host_set_dispersion.restype = None
    lib.host_get_at_flags.argtypes = [vp, vp]
    lib.host_get_at_flags.restype = None
    lib.host_get_c9.argtypes = [vp, vp]
    lib.host_get_c9.restype = None
    lib.host_set_c9.argtypes = [vp, vp]
    lib.host_set_c9.restype = None
    lib.host_get_three_body_energy.argtypes = [vp]
    lib.host_get_three_body_energy.restype = C.c_double
    lib.host_get_vdw.argtypes = [vp, vp]
    lib.host_get_vdw.restype = None
    lib.host_get_omega.argtypes = [vp, vp]
    lib.host_get_omega.restype = None
    lib.host_set_omega.argtypes = [vp, vp, vp]
    lib.host_set_omega.restype = None
    lib.host_displace_molecule.argtypes = [vp, C.c_int, vp]
    lib.host_get_rdc_flags.argtypes = [vp, vp]
    lib.host_get_rdc_flags.restype = None
    lib.host_get_rdform_flags.argtypes = [vp, vp]
    lib.host_get_rdform_flags.restype = None
    lib.host_get_thole_flags.argtypes = [vp, vp]
    lib.host_get_thole_flags.restype = None
    lib.host_read_frame.argtypes = [vp, C.c_char_p, C.c_int]
    lib.host_unsupported.argtypes = [vp]
    lib.host_unsupported.restype = C.c_char_p
    lib.host_get_polarizability_tensor.argtypes = [vp, vp]
    lib.host_get_cavity_flags.argtypes = [vp, vp]
    lib.host_get_cavity_flags.restype = None
    lib.host_get_cavity.argtypes = [vp, vp]
    lib.host_get_cavity.restype = C.c_int
    lib.host_get_cavity_darts.argtypes = [vp, vp]
    lib.host_get_cavity_darts.restype = None
    lib.host_get_sync_counts.argtypes = [vp, C.POINTER(C.c_long)]
    lib.host_get_sync_counts.restype = None
    lib.host_effective_c9.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double]
    lib.host_effective_c9.restype = C.c_double
    lib.host_qrot_evaluate.argtypes = [vp]
    lib.host_qrot_levels.argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    lib.host_qrot_counts.argtypes = [vp, C.POINTER(C.c_long)]
    lib.host_qrot_counts.restype = None
    lib.host_last_movetype.argtypes = [vp]
    lib.host_qrot_placements.argtypes = [vp, C.c_int, vp]
    lib.host_qrot_times.argtypes = [vp]
    lib.host_qrot_times.restype = None
    lib.qrot_jacobi.argtypes = [C.c_int, vp, vp, vp, C.POINTER(C.c_long)]
    lib.qrot_hamiltonian.argtypes = [C.c_int, C.c_double, vp, vp]
    lib.host_get_spin_ratio.argtypes = [vp]
    lib.host_get_spin_ratio.restype = C.c_double
    lib.host_last_energy.argtypes = [vp]
    lib.host_last_energy.restype = C.c_double
    lib.qrot_hindered_grid.argtypes = [C.c_double, C.c_double, vp]
    lib.qrot_hindered_grid.restype = None
    lib.qrot_symmetry.argtypes = [vp, C.c_int, vp]
    lib.qrot_basis.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.qrot_basis.restype = C.c_double
    lib.qrot_last_times.argtypes = [vp]
    lib.qrot_last_times.restype = None
    lib.volume_change.argtypes = [vp]
    lib.volume_change.restype = None
    lib.revert_volume_change.argtypes = [vp]
    lib.revert_volume_change.restype = None
    _lib = lib
    return lib


def config_text(flags, extra=None):
    """flags in C-ABI / oracle naming -> the reference's keyword lines."""
    onoff = {"rd_only", "rd_lrc", "feynman_hibbs", "polarization", "polar_gs", "polar_gs_ranked", "polar_sor",
             "polar_esor", "polar_palmo", "polar_rrms", "polar_zodid", "polar_wolf", "polar_ewald", "wolf",
             "disp_expansion", "damp_dispersion", "extrapolate_disp_coeffs", "schmidt_mixing", "axilrod_teller",
             "midzuno_kihara_approx", "rd_crystal", "read_pqr_box", "calc_pressure", "polarvdw", "cdvdw",
             "cavity_autoreject_absolute", "cavity_bias", "cdvdw_exp_repulsion", "cdvdw_sig_repulsion",
             "cdvdw_9th_repulsion", "sg", "dreiding", "lj_buffered_14_7", "waldmanhagler", "halgren_mixing", "c6_mixing",
             "polar_iterative", "polarizability_tensor", "polar_wolf_full", "quantum_rotation",
             "quantum_rotation_hindered", "quantum_rotation_eigenvectors"}
    lines = []
    for k, v in flags.items():
        if k in ("polarvdw", "cdvdw") and isinstance(v, str):
            lines.append("%s %s" % (k, v))  # evects / comp
        elif k == "polar_damp_type":
            lines.append("%s %s" % (k, v))  # a bare word: exponential | linear | off | none
        elif k in onoff:
            lines.append("%s %s" % (k, "on" if v else "off"))
        elif k in ("ewald_alpha_set", "polar_ewald_alpha_set"):
            continue
        else:
            lines.append("%s %r" % (k, v))
    if flags.get("polarization"):
        if "polar_damp_type" not in flags:
            lines.append("polar_damp_type exponential")
        if "polar_iterative" not in flags:  # (polar_iterative=0: the exact dipoles)
            lines.append("polar_iterative on")
    for k, v in (extra or {}).items():
        lines.append("%s %s" % (k, v))
    return "\n".join(lines) + "\n"


def walkers_unique_id():
    """128-byte RCCL id (made on rank 0, handed to the other ranks by the launcher)."""
    buf = (C.c_ubyte * 128)()
    if load().walkers_unique_id(buf) != 0:
        raise engine.EngineError("walkers_unique_id: " + engine.load().mpmc_hip_last_error().decode())
    return bytes(buf)


def mc_steps_multi(walkers, nsteps):
    """Advance several HostSystem walkers together (one process, interleaved on the device): every walker takes
    `nsteps` steps exactly as it would alone.  Returns the number of accepted moves over all walkers."""
    lib = walkers[0].lib
    arr = (C.c_void_p * len(walkers))(*[w.ptr for w in walkers])
    acc = lib.host_mc_steps_multi(arr, len(walkers), int(nsteps))
    if acc < 0:
        raise engine.EngineError(engine.load().mpmc_hip_last_error().decode())
    return acc


class HostSystem:
    """A system_t built from arrays, driven through the C host layer."""

    def __init__(self, system, flags, device=0, seed=None, move_factor=0.01, rot_factor=0.01, extra=None):
        self.lib = load()
        n = len(system["charge"])
        self.n = n
        arrs = [np.ascontiguousarray(system["pos"], dtype=np.float64).reshape(n, 3)]
        arrs += [np.ascontiguousarray(system[k], dtype=np.float64)
                 for k in ("charge", "alpha", "epsilon", "sigma", "mass")]
        arrs += [np.ascontiguousarray(system[k], dtype=np.int32) for k in ("molecule", "frozen")]
        arrs += [np.ascontiguousarray(system["basis"], dtype=np.float64).reshape(9)]
        self.ptr = C.c_void_p(self.lib.system_from_arrays(n, *[a.ctypes.data for a in arrs]))
        if "c6" in system:  # PHAHST: per-atom dispersion coefficients (atomic units)
            c = [np.ascontiguousarray(system.get(k, np.zeros(n)), dtype=np.float64) for k in ("c6", "c8", "c10")]
            self.lib.host_set_dispersion(self.ptr, *[a.ctypes.data for a in c])
        if "c9" in system:  # axilrod_teller: per-atom three-body coefficient (atomic units)
            c9 = np.ascontiguousarray(system["c9"], dtype=np.float64)
            self.lib.host_set_c9(self.ptr, c9.ctypes.data)
        if "omega" in system:  # polarvdw: per-atom frequency (atomic units) and the molecules' type ids
            w = np.ascontiguousarray(system["omega"], dtype=np.float64)
            t = np.ascontiguousarray(system.get("mol_type", np.zeros(n)), dtype=np.int32)
            self.lib.host_set_omega(self.ptr, w.ctypes.data, t.ctypes.data)
        extra = dict({"move_factor": move_factor, "rot_factor": rot_factor}, **(extra or {}))
        if self.lib.host_apply_config(self.ptr, config_text(flags, extra).encode()) != 0:
            raise ValueError("host layer rejected the configuration")
        self.lib.host_set_device(self.ptr, device)
        if seed is not None:
            self.lib.host_seed(self.ptr, int(seed))

    def close(self):
        if self.ptr:
            self.lib.free_system(self.ptr)
            self.ptr = C.c_void_p()

    def energy(self):
        return self.lib.energy(self.ptr)

    def set_option(self, name, value):
        """Engine A/B knob (mpmc_hip_set_option); the device context exists after the first energy()."""
        if self.lib.host_set_option(self.ptr, name.encode(), int(value)) != 0:
            raise engine.EngineError(engine.load().mpmc_hip_last_error().decode())

    def three_body_energy(self):
        """observables->three_body_energy of the last energy() (0 unless axilrod_teller is on)."""
        return self.lib.host_get_three_body_energy(self.ptr)

    def displace_molecule(self, index, d):
        """The index-th molecule of the list steps by d, outside Metropolis (a test entry)."""
        v = np.ascontiguousarray(d, dtype=np.float64)
        if self.lib.host_displace_molecule(self.ptr, int(index), v.ctypes.data) != 0:
            raise IndexError(index)

    def polarizability_tensor(self):
        """The 3 x 3 molecular polarizability tensor (A^3) of the last energy(): polar_iterative=0 only."""
        out = np.zeros(9)
        if self.lib.host_get_polarizability_tensor(self.ptr, out.ctypes.data) != 0:
            raise engine.EngineError(engine.load().mpmc_hip_last_error().decode())
        return out.reshape(3, 3)

    def vdw(self):
        """polarvdw / cavity_autoreject_absolute state: the keywords as read, count_autorejects, observables->vdw_energy."""
        out = np.zeros(5)
        self.lib.host_get_vdw(self.ptr, out.ctypes.data)
        return dict(polarvdw=int(out[0]), cavity_autoreject_absolute=int(out[1]), cavity_autoreject_scale=out[2],
                    count_autorejects=int(out[3]), vdw_energy=out[4])

    def cavity_flags(self):
        """cavity_bias, cavity_grid and cavity_radius as read."""
        out = np.zeros(3)
        self.lib.host_get_cavity_flags(self.ptr, out.ctypes.data)
        return dict(cavity_bias=int(out[0]), cavity_grid=int(out[1]), cavity_radius=out[2])

    def cavity(self):
        """The cavity-bias state after the last make_move(): the grid's counts for the configuration the move started from,
        the running means, and whether the move takes the biased acceptance."""
        out = np.zeros(10)
        self.lib.host_get_cavity(self.ptr, out.ctypes.data)
        return dict(cavities_open=int(out[0]), hits=int(out[1]), n_darts=int(out[2]), cavity_volume=out[3],
                    cavity_bias_probability=out[4], avg_nodestats=out[5], avg_observables=out[6],
                    biased_move=int(out[7]), boltzmann_factor=out[8], trial_energy=out[9])

    def cavity_darts(self):
        """The dart positions [n, 3] of the last make_move()'s grid update."""
        out = np.zeros(10)
        n = self.lib.host_get_cavity(self.ptr, out.ctypes.data)
        darts = np.zeros((max(n, 0), 3))
        self.lib.host_get_cavity_darts(self.ptr, darts.ctypes.data)
        return darts

    def observables(self):
        out = np.zeros(8)
        self.lib.host_get_observables(self.ptr, out.ctypes.data)
        npt = np.zeros(5)
        self.lib.host_get_npt(self.ptr, npt.ctypes.data)
        return dict(energy=out[0], coulombic_energy=out[1], rd_energy=out[2], polarization_energy=out[3], N=out[4],
                    polar_iterations=out[5], accept=int(out[6]), reject=int(out[7]), volume=npt[0], cutoff=npt[1],
                    accept_volume=int(npt[2]), reject_volume=int(npt[3]))

    # ---- npt
    def basis(self):
        """Current lattice vectors (rows), which volume moves scale."""
        b = np.zeros(9)
        self.lib.host_get_basis(self.ptr, b.ctypes.data)
        return b.reshape(3, 3)

    def next_movetype(self):
        """What checkpoint() decided the next make_move() does: 'insert', 'remove', 'displace', 'volume' or 'spinflip'."""
        npt = np.zeros(5)
        self.lib.host_get_npt(self.ptr, npt.ctypes.data)
        return ("insert", "remove", "displace", "volume", "spinflip")[int(npt[4])]

    # ---- quantum_rotation
    def qrot_evaluate(self):
        """One quantum_system_rotational_energies() over the movable molecules (needs a completed energy() unless the
        potential is the hindered rotor's); prints the DEBUG_QROT lines."""
        if self.lib.host_qrot_evaluate(self.ptr) != 0:
            raise engine.EngineError("quantum_rotation: the evaluation failed")

    def rotational_levels(self):
        """Per movable molecule, as the last evaluation left them: dict(levels [level_max] in K, symmetry [level_max]
        (0 symmetric, 1 antisymmetric), rot_partfunc_g, rot_partfunc_u, rot_partfunc, nuclear_spin (0 para, 1 ortho))."""
        out = []
        while True:
            lev, sym, pf, spin = np.zeros(81), np.zeros(81, dtype=np.int32), np.zeros(3), C.c_int(0)
            n = self.lib.host_qrot_levels(self.ptr, len(out), lev.ctypes.data, sym.ctypes.data, pf.ctypes.data, C.byref(spin))
            if n < 0:
                return out
            out.append(dict(levels=lev[:n].copy(), symmetry=sym[:n].copy(), rot_partfunc_g=pf[0], rot_partfunc_u=pf[1],
                            rot_partfunc=pf[2], nuclear_spin=spin.value))

    def spin_ratio(self):
        """observables->spin_ratio of the last energy(): the para fraction of the movable molecules (0 without
        quantum_rotation)."""
        return float(self.lib.host_get_spin_ratio(self.ptr))

    def last_energy(self):
        """What the last energy() returned -- a rejected trial's too."""
        return float(self.lib.host_last_energy(self.ptr))

    def qrot_counts(self):
        """Trial-energy calls the binding has made (one per movable molecule per evaluation), accepted and rejected
        spin-flip moves."""
        out = (C.c_long * 3)()
        self.lib.host_qrot_counts(self.ptr, out)
        return dict(trial_calls=int(out[0]), accept_spinflip=int(out[1]), reject_spinflip=int(out[2]))

    def set_volume_notes(self, on):
        """False: the binding ignores volume-move notes, so every volume step uploads the whole configuration."""
        self.lib.host_set_volume_notes(self.ptr, int(bool(on)))

    def force_volume_move(self, new_volume, revert=False):
        """One volume move to `new_volume` outside Metropolis and, on request, its revert (no energy evaluated)."""
        self.lib.host_force_volume_move(self.ptr, float(new_volume), int(bool(revert)))

    def sync_counts(self):
        """How the binding has kept the device in line so far (host_get_sync_counts): full uploads, edit calls that were
        carried out (mpmc_hip_edit_molecules), molecules those calls removed + inserted."""
        out = (C.c_long * 3)()
        self.lib.host_get_sync_counts(self.ptr, out)
        return dict(full_uploads=int(out[0]), edit_calls=int(out[1]), molecules_edited=int(out[2]))

    def mc_steps(self, nsteps):
        r = self.lib.host_mc_steps(self.ptr, int(nsteps))
        if r < 0:
            raise engine.EngineError(engine.load().mpmc_hip_last_error().decode())
        return r

    # ---- walker pooling through the C ABI's RCCL entry (the reference's MPI_Gather, mc.c:417-432)
    def walkers_init(self, nranks, rank, unique_id):
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id)) if unique_id is not None else None
        if self.lib.walkers_init(self.ptr, int(nranks), int(rank), buf) != 0:
            raise engine.EngineError("walkers_init: " + engine.load().mpmc_hip_last_error().decode())

    def pool_begin(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if self.lib.walkers_pool_begin(self.ptr, v.ctypes.data, len(v)) != 0:
            raise engine.EngineError("walkers_pool_begin: " + engine.load().mpmc_hip_last_error().decode())

    def pool_end(self, count):
        out = np.zeros(count)
        if self.lib.walkers_pool_end(self.ptr, out.ctypes.data, count) != 0:
            raise engine.EngineError("walkers_pool_end: " + engine.load().mpmc_hip_last_error().decode())
        return out

    def positions(self):
        pos = np.zeros((self.natoms(), 3))
        self.lib.host_get_positions(self.ptr, pos.ctypes.data)
        return pos

    def natoms(self):
        return int(self.lib.host_natoms(self.ptr))

    def system(self, basis):
        """Current configuration as a dict of arrays (N may differ from the initial one under uvt)."""
        n = self.natoms()
        f = {k: np.zeros(n) for k in ("charge", "alpha", "epsilon", "sigma", "mass")}
        pos = np.zeros((n, 3))
        mol = np.zeros(n, dtype=np.int32)
        frz = np.zeros(n, dtype=np.int32)
        self.lib.host_get_system(self.ptr, pos.ctypes.data, f["charge"].ctypes.data, f["alpha"].ctypes.data,
                                 f["epsilon"].ctypes.data, f["sigma"].ctypes.data, f["mass"].ctypes.data,
                                 mol.ctypes.data, frz.ctypes.data)
        return dict(pos=pos, molecule=mol, frozen=frz, basis=np.asarray(basis, dtype=np.float64), **f)

    def dipoles(self):
        n = self.natoms()  # differs from the initial count under uvt
        mu, es, ei = (np.zeros((n, 3)) for _ in range(3))
        if self.lib.host_get_dipoles(self.ptr, mu.ctypes.data, es.ctypes.data, ei.ctypes.data):
            raise engine.EngineError(engine.load().mpmc_hip_last_error().decode())
        return dict(mu=mu, ef_static=es, ef_induced=ei)

    def enable_timing(self, on=True):
        self.lib.host_enable_timing(self.ptr, int(on))

    def timings(self):
        t = engine.Timings()
        self.lib.host_get_timings(self.ptr, C.byref(t))
        return {f: getattr(t, f) for f, _ in engine.Timings._fields_}
