"""ctypes binding of the C ABI in include/mpmc_hip.h (libmpmc_hip.so).

This is plumbing for tests and bench.py; the product is the shared library.  There is no
fallback: if the library or a gfx950 device is missing every call raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmpmc_hip.so")

# every symbol include/mpmc_hip.h declares
EXPORTS = [
    "mpmc_hip_last_error", "mpmc_hip_abi_version", "mpmc_hip_device_count", "mpmc_hip_create",
    "mpmc_hip_destroy", "mpmc_hip_set_option", "mpmc_hip_default_params", "mpmc_hip_set_params", "mpmc_hip_set_box",
    "mpmc_hip_scale_box",
    "mpmc_hip_upload", "mpmc_hip_set_dispersion", "mpmc_hip_set_axilrod_teller", "mpmc_hip_get_three_body_energy",
    "mpmc_hip_set_rd_crystal", "mpmc_hip_set_rd_form", "mpmc_hip_set_vdw", "mpmc_hip_get_vdw_energy", "mpmc_hip_get_vdw_terms",
    "mpmc_hip_set_autoreject", "mpmc_hip_get_close_contacts",
    "mpmc_hip_set_cavity_grid", "mpmc_hip_cavity_bin", "mpmc_hip_cavity_update", "mpmc_hip_cavity_point",
    "mpmc_hip_download_cavity_grid",
    "mpmc_hip_set_exact_polar", "mpmc_hip_get_polarizability_tensor", "mpmc_hip_set_thole_model",
    "mpmc_hip_update_atoms", "mpmc_hip_insert_molecule", "mpmc_hip_remove_molecule", "mpmc_hip_edit_molecules",
    "mpmc_hip_slot_count", "mpmc_hip_set_sweep_order",
    "mpmc_hip_default_dimer_params", "mpmc_hip_dimer_energies", "mpmc_hip_dimer_grid_means",
    "mpmc_hip_trial_energies", "mpmc_hip_trial_call_count", "mpmc_hip_energy", "mpmc_hip_energy_begin", "mpmc_hip_energy_end",
    "mpmc_hip_download_dipoles",
    "mpmc_hip_download_amatrix", "mpmc_hip_download_ranking", "mpmc_hip_get_timings",
    "mpmc_hip_comm_unique_id", "mpmc_hip_comm_create", "mpmc_hip_comm_size", "mpmc_hip_comm_rank",
    "mpmc_hip_allreduce_observables", "mpmc_hip_allreduce_observables_begin", "mpmc_hip_allreduce_observables_end",
    "mpmc_hip_gather_observables", "mpmc_hip_comm_destroy",
]


class Params(C.Structure):
    _fields_ = [
        ("temperature", C.c_double),
        ("rd_only", C.c_int),
        ("rd_lrc", C.c_int),
        ("feynman_hibbs", C.c_int),
        ("feynman_hibbs_order", C.c_int),
        ("ewald_alpha_set", C.c_int),
        ("ewald_alpha", C.c_double),
        ("ewald_kmax", C.c_int),
        ("polarization", C.c_int),
        ("polar_damp", C.c_double),
        ("polar_max_iter", C.c_int),
        ("polar_precision", C.c_double),
        ("polar_gamma", C.c_double),
        ("polar_gs", C.c_int),
        ("polar_gs_ranked", C.c_int),
        ("polar_sor", C.c_int),
        ("polar_esor", C.c_int),
        ("polar_palmo", C.c_int),
        ("polar_rrms", C.c_int),
        ("polar_zodid", C.c_int),
        ("polar_wolf", C.c_int),
        ("polar_wolf_alpha", C.c_double),
        ("polar_ewald", C.c_int),
        ("polar_ewald_alpha_set", C.c_int),
        ("polar_ewald_alpha", C.c_double),
        ("wolf", C.c_int),
    ]


class Result(C.Structure):
    _fields_ = [
        ("energy", C.c_double),
        ("rd_energy", C.c_double),
        ("coulombic_energy", C.c_double),
        ("polarization_energy", C.c_double),
        ("es_real", C.c_double),
        ("es_recip", C.c_double),
        ("es_self", C.c_double),
        ("dipole_rrms", C.c_double),
        ("volume", C.c_double),
        ("cutoff", C.c_double),
        ("ewald_alpha", C.c_double),
        ("polar_ewald_alpha", C.c_double),
        ("polar_iterations", C.c_int),
        ("iter_success", C.c_int),
        ("n_atoms", C.c_int),
        ("status", C.c_int),
    ]


class Timings(C.Structure):
    _fields_ = [
        ("pair_ms", C.c_float),
        ("recip_ms", C.c_float),
        ("field_ms", C.c_float),
        ("amatrix_ms", C.c_float),
        ("sweep_ms", C.c_float),
        ("palmo_ms", C.c_float),
        ("other_ms", C.c_float),
        ("total_ms", C.c_float),
        ("sweep_count", C.c_int),
        ("amatrix_count", C.c_int),
        ("graph_steps", C.c_int),
        ("event_pair_ms", C.c_float),
        ("event_pair_count", C.c_int),
        ("spec_rank_redos", C.c_int),
        ("resident_calls", C.c_int),
        ("resident_fallbacks", C.c_int),
        ("pending_sweeps", C.c_int),
    ]


class DispParams(C.Structure):
    """mpmc_hip_disp_params: the PHAHST switches (reference keywords)."""
    _fields_ = [
        ("disp_expansion", C.c_int),
        ("damp_dispersion", C.c_int),
        ("extrapolate_disp_coeffs", C.c_int),
        ("schmidt_mixing", C.c_int),
    ]


class RdFormParams(C.Structure):
    """mpmc_hip_rd_form_params: the pair potential and the Lennard-Jones mixing rule (mpmc_hip_set_rd_form)."""
    _fields_ = [
        ("form", C.c_int),
        ("mixing", C.c_int),
    ]


class TholeModel(C.Structure):
    """mpmc_hip_thole_model: the dipole tensor of the A matrix (mpmc_hip_set_thole_model)."""
    _fields_ = [
        ("damp_type", C.c_int),
        ("wolf_full", C.c_int),
    ]


class Molecule(C.Structure):
    """mpmc_hip_molecule: one molecule of mpmc_hip_edit_molecules()."""
    _fields_ = [("count", C.c_int), ("frozen", C.c_int)] + [
        (k, C.c_void_p) for k in ("x", "y", "z", "charge", "polarizability", "epsilon", "sigma", "mass",
                                  "c6", "c8", "c10", "c9")]


class DimerParams(C.Structure):
    """mpmc_hip_dimer_params: what a dimer scan computes (mpmc_hip_dimer_energies / _grid_means)."""
    _fields_ = [
        ("rd_form", C.c_int),
        ("mixing", C.c_int),
        ("disp_expansion", C.c_int),
        ("damp_dispersion", C.c_int),
        ("extrapolate_disp_coeffs", C.c_int),
        ("schmidt_mixing", C.c_int),
        ("rd_only", C.c_int),
        ("damp_type", C.c_int),
        ("polar_damp", C.c_double),
        ("polar_max_iter", C.c_int),
        ("polar_precision", C.c_double),
        ("polar_gs", C.c_int),
        ("polar_gs_ranked", C.c_int),
        ("polar_palmo", C.c_int),
        ("polar_gamma", C.c_double),
        ("global_axis", C.c_int),
    ]


DIMER_CHUNK = 256  # MPMC_HIP_DIMER_CHUNK: placements per workgroup, the unit of the grid form's fixed-order sum
DIMER_NOT_CONVERGED = 0x40000000  # MPMC_HIP_DIMER_NOT_CONVERGED
DIMER_SITES = 32  # rows per placement of the dipoles dimer_energies(mu=True) returns
THOLE_DAMPINGS = {"off": 0, "none": 0, "linear": 1, "exponential": 2}  # the reference's DAMPING_* values
RD_FORMS = {"off": 0, "lj": 1, "sg": 2, "dreiding": 3, "lj_buffered_14_7": 4}  # MPMC_HIP_RD_*
RD_MIXINGS = {"lb": 0, "waldmanhagler": 1, "halgren_mixing": 2, "c6_mixing": 3}  # MPMC_HIP_RD_MIX_*
PARAM_NAMES = [f[0] for f in Params._fields_]
DISP_NAMES = [f[0] for f in DispParams._fields_]
AT_NAMES = ["axilrod_teller", "midzuno_kihara_approx"]  # mpmc_hip_set_axilrod_teller (reference keywords)
RDC_NAMES = ["rd_crystal", "rd_crystal_order"]  # mpmc_hip_set_rd_crystal (reference keywords)
RDFORM_NAMES = ["sg", "dreiding", "lj_buffered_14_7", "waldmanhagler", "halgren_mixing", "c6_mixing"]  # mpmc_hip_set_rd_form
VDW_NAMES = ["polarvdw", "cdvdw"]  # mpmc_hip_set_vdw (reference keywords)
AUTOREJECT_NAMES = ["cavity_autoreject_absolute", "cavity_autoreject_scale"]  # mpmc_hip_set_autoreject (reference keywords)
EXACT_NAMES = ["polar_iterative"]  # mpmc_hip_set_exact_polar (reference keyword; 0 = the exact dipoles)
THOLE_NAMES = ["polar_damp_type", "polar_wolf_full"]  # mpmc_hip_set_thole_model (reference keywords)
VDW_TERMS = ["e_total", "e_iso", "lr_corr", "repulsion", "repulsion_lrc"]  # mpmc_hip_get_vdw_terms, in its order
# flags that make_params() leaves to others: pbc_cutoff is a box property at this boundary (set_box), the rest are the
# arguments of the calls above (Engine.load_system)
NOT_PARAMS = frozenset(["pbc_cutoff"] + DISP_NAMES + AT_NAMES + RDC_NAMES + RDFORM_NAMES + VDW_NAMES + AUTOREJECT_NAMES + EXACT_NAMES
                       + THOLE_NAMES)
AT_ALPHA_AU = 6.7483345  # A^3 -> Bohr^3, as the reference writes it (axilrod_teller.cpp:115)

_lib = None


def load():
    """Load libmpmc_hip.so and declare prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmpmc_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
            "there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    lib.mpmc_hip_last_error.restype = C.c_char_p
    lib.mpmc_hip_abi_version.restype = C.c_int
    lib.mpmc_hip_device_count.restype = C.c_int
    lib.mpmc_hip_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    lib.mpmc_hip_destroy.argtypes = [vp]
    lib.mpmc_hip_destroy.restype = None
    lib.mpmc_hip_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    lib.mpmc_hip_default_params.argtypes = [C.POINTER(Params)]
    lib.mpmc_hip_default_params.restype = None
    lib.mpmc_hip_set_params.argtypes = [vp, C.POINTER(Params)]
    lib.mpmc_hip_set_box.argtypes = [vp, dp, C.c_double]
    lib.mpmc_hip_scale_box.argtypes = [vp, dp, C.c_double, C.c_int, vp]
    lib.mpmc_hip_upload.argtypes = [vp, C.c_int] + [vp] * 10
    lib.mpmc_hip_set_dispersion.argtypes = [vp, C.POINTER(DispParams), C.c_int, vp, vp, vp]
    lib.mpmc_hip_set_axilrod_teller.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.mpmc_hip_get_three_body_energy.argtypes = [vp, dp]
    lib.mpmc_hip_set_rd_crystal.argtypes = [vp, C.c_int]
    lib.mpmc_hip_set_rd_form.argtypes = [vp, C.POINTER(RdFormParams)]
    lib.mpmc_hip_set_vdw.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    lib.mpmc_hip_get_vdw_energy.argtypes = [vp, dp]
    lib.mpmc_hip_get_vdw_terms.argtypes = [vp, dp]
    lib.mpmc_hip_set_exact_polar.argtypes = [vp, C.c_int]
    lib.mpmc_hip_get_polarizability_tensor.argtypes = [vp, dp]
    lib.mpmc_hip_set_thole_model.argtypes = [vp, C.POINTER(TholeModel)]
    lib.mpmc_hip_set_autoreject.argtypes = [vp, C.c_double]
    lib.mpmc_hip_get_close_contacts.argtypes = [vp, C.POINTER(C.c_longlong)]
    ip = C.POINTER(C.c_int)
    lib.mpmc_hip_set_cavity_grid.argtypes = [vp, C.c_int, C.c_double]
    lib.mpmc_hip_cavity_bin.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.mpmc_hip_cavity_update.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, ip, ip]
    lib.mpmc_hip_cavity_point.argtypes = [vp, C.c_int, ip, dp]
    lib.mpmc_hip_download_cavity_grid.argtypes = [vp, vp, vp]
    lib.mpmc_hip_update_atoms.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    lib.mpmc_hip_insert_molecule.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    lib.mpmc_hip_remove_molecule.argtypes = [vp, C.c_int, C.c_int]
    lib.mpmc_hip_edit_molecules.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(Molecule), vp]
    lib.mpmc_hip_slot_count.argtypes = [vp]
    lib.mpmc_hip_set_sweep_order.argtypes = [vp, C.c_int, vp]
    lib.mpmc_hip_default_dimer_params.argtypes = [C.POINTER(DimerParams)]
    lib.mpmc_hip_default_dimer_params.restype = None
    lib.mpmc_hip_dimer_energies.argtypes = [vp, C.POINTER(DimerParams), C.POINTER(Molecule), C.POINTER(Molecule), C.c_int,
                                            vp, vp, vp, vp, vp, vp]
    lib.mpmc_hip_dimer_grid_means.argtypes = [vp, C.POINTER(DimerParams), C.POINTER(Molecule), C.POINTER(Molecule),
                                              C.c_double, ip, C.POINTER(vp), dp, C.POINTER(C.c_longlong)]
    lib.mpmc_hip_trial_energies.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.mpmc_hip_trial_call_count.argtypes = [vp]
    lib.mpmc_hip_trial_call_count.restype = C.c_longlong
    lib.mpmc_hip_energy.argtypes = [vp, C.POINTER(Result)]
    lib.mpmc_hip_energy_begin.argtypes = [vp]
    lib.mpmc_hip_energy_end.argtypes = [vp, C.POINTER(Result)]
    lib.mpmc_hip_download_dipoles.argtypes = [vp, vp, vp, vp, vp]
    lib.mpmc_hip_download_amatrix.argtypes = [vp, vp]
    lib.mpmc_hip_download_ranking.argtypes = [vp, vp, vp]
    lib.mpmc_hip_get_timings.argtypes = [vp, C.POINTER(Timings)]
    lib.mpmc_hip_comm_unique_id.argtypes = [vp]
    lib.mpmc_hip_comm_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, vp]
    lib.mpmc_hip_allreduce_observables.argtypes = [vp, vp, C.c_int]
    lib.mpmc_hip_allreduce_observables_begin.argtypes = [vp, vp, C.c_int]
    lib.mpmc_hip_allreduce_observables_end.argtypes = [vp, vp]
    lib.mpmc_hip_gather_observables.argtypes = [vp, vp, C.c_int, vp]
    lib.mpmc_hip_comm_size.argtypes = [vp]
    lib.mpmc_hip_comm_rank.argtypes = [vp]
    lib.mpmc_hip_comm_destroy.argtypes = [vp]
    lib.mpmc_hip_comm_destroy.restype = None
    _lib = lib
    return lib


class EngineError(RuntimeError):
    pass


def _chk(rc):
    if rc != 0:
        raise EngineError(load().mpmc_hip_last_error().decode())


def make_params(**kw):
    p = Params()
    load().mpmc_hip_default_params(C.byref(p))
    for k, v in kw.items():
        if k in NOT_PARAMS:
            continue
        if k not in PARAM_NAMES:
            raise KeyError(k)
        setattr(p, k, v)
    return p


def effective_c9(system, midzuno_kihara_approx=False):
    """Per-atom c9 as mpmc_hip_set_axilrod_teller() takes it: the array as read, or the Midzuno-Kihara replacement
    3/4 * alpha * 6.7483345 * c6 evaluated left to right as the reference does (axilrod_teller.cpp:115)."""
    n = len(system["alpha"])
    if midzuno_kihara_approx:
        alpha = np.asarray(system["alpha"], dtype=np.float64)
        c6 = np.asarray(system.get("c6", np.zeros(n)), dtype=np.float64)
        return np.ascontiguousarray(3.0 / 4.0 * alpha * AT_ALPHA_AU * c6)
    return np.ascontiguousarray(system.get("c9", np.zeros(n)), dtype=np.float64)


def rd_form_of(params):
    """(form, mixing) names of set_rd_form() for a flag set: the first of sg / dreiding / lj_buffered_14_7 that is on,
    else "lj" when a mixing rule is named, else "off"; two mixing rules are the reference's input error
    (check_input.c:1277-1281)."""
    mix = [m for m in ("waldmanhagler", "halgren_mixing", "c6_mixing") if params.get(m)]
    if len(mix) > 1:
        raise ValueError("INPUT: more than one mixing rule specified")
    form = next((f for f in ("sg", "dreiding", "lj_buffered_14_7") if params.get(f)), "lj" if mix else "off")
    return form, (mix[0] if mix else "lb")


def make_dimer_params(**flags):
    """mpmc_hip_dimer_params from reference keywords: waldmanhagler / halgren_mixing / c6_mixing, the PHAHST switches,
    rd_only, polar_damp_type ("exponential" | "linear" | "off" | "none"), polar_damp, polar_max_iter, polar_precision,
    polar_gs, polar_gs_ranked, polar_palmo, polar_gamma, and surf_global_axis (or global_axis)."""
    p = DimerParams()
    load().mpmc_hip_default_dimer_params(C.byref(p))
    flags = dict(flags)
    form, mix = rd_form_of(flags)
    if form not in ("off", "lj"):
        raise ValueError("a dimer scan has Lennard-Jones or disp_expansion, not %s" % form)
    p.rd_form, p.mixing = RD_FORMS["lj"], RD_MIXINGS[mix]
    for k in ("waldmanhagler", "halgren_mixing", "c6_mixing"):
        flags.pop(k, None)
    damping = flags.pop("polar_damp_type", "exponential")
    p.damp_type = THOLE_DAMPINGS[damping.lower()] if isinstance(damping, str) else int(damping)
    p.global_axis = int(bool(flags.pop("surf_global_axis", flags.pop("global_axis", 0))))
    flags.pop("polarization", None)  # (a site's polarizability says whether the Thole system is solved)
    for k, v in flags.items():
        if k not in dict(DimerParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _dimer_molecule(d, keep):
    """mpmc_hip_molecule of a dict with pos [k, 3], charge, alpha, epsilon, sigma, mass and optionally c6 / c8 / c10."""
    m = Molecule()
    pos = np.ascontiguousarray(d["pos"], dtype=np.float64).reshape(-1, 3)
    m.count, m.frozen = pos.shape[0], 0
    for k, name in enumerate("xyz"):
        keep.append(np.ascontiguousarray(pos[:, k]))
        setattr(m, name, keep[-1].ctypes.data)
    for field, key in (("charge", "charge"), ("polarizability", "alpha"), ("epsilon", "epsilon"), ("sigma", "sigma"),
                       ("mass", "mass"), ("c6", "c6"), ("c8", "c8"), ("c10", "c10")):
        if d.get(key) is None:
            continue
        a = np.ascontiguousarray(d[key], dtype=np.float64)
        if a.shape != (pos.shape[0],):
            raise ValueError("dimer: %s must have one entry per site of the molecule" % key)
        keep.append(a)
        setattr(m, field, a.ctypes.data)
    return m


class Engine:
    """One device context = one MC walker's energy engine."""

    def __init__(self, max_atoms, device=0):
        self.lib = load()
        self.ctx = C.c_void_p()
        _chk(self.lib.mpmc_hip_create(C.byref(self.ctx), device, int(max_atoms)))
        self.n = 0

    def close(self):
        if self.ctx:
            self.lib.mpmc_hip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, **kw):
        p = kw.pop("_struct", None) or make_params(**kw)
        _chk(self.lib.mpmc_hip_set_params(self.ctx, C.byref(p)))

    def set_option(self, name, value):
        _chk(self.lib.mpmc_hip_set_option(self.ctx, name.encode(), int(value)))

    def set_box(self, basis, pbc_cutoff=0.0):
        b = np.ascontiguousarray(basis, dtype=np.float64).reshape(9)
        _chk(self.lib.mpmc_hip_set_box(self.ctx, b.ctypes.data_as(C.POINTER(C.c_double)), float(pbc_cutoff)))

    def scale_box(self, basis, delta, pbc_cutoff=0.0):
        """NPT volume move on the resident configuration (mpmc_hip_scale_box): the new basis and one displacement
        per molecule, in upload order.  False = the engine asks for a full upload instead."""
        b = np.ascontiguousarray(basis, dtype=np.float64).reshape(9)
        d = np.ascontiguousarray(delta, dtype=np.float64).reshape(-1, 3)
        rc = self.lib.mpmc_hip_scale_box(self.ctx, b.ctypes.data_as(C.POINTER(C.c_double)), float(pbc_cutoff),
                                         d.shape[0], d.ctypes.data)
        if rc < 0:
            _chk(rc)
        return rc == 0

    def upload(self, system):
        """system: dict with pos[n,3], charge, alpha, epsilon, sigma, mass, molecule, frozen (and, for set_dispersion(),
        optional c6, c8, c10)."""
        pos = np.ascontiguousarray(system["pos"], dtype=np.float64)
        n = pos.shape[0]
        cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
        arrs = cols + [np.ascontiguousarray(system[k], dtype=np.float64)
                       for k in ("charge", "alpha", "epsilon", "sigma", "mass")]
        mol = np.ascontiguousarray(system["molecule"], dtype=np.int32)
        frz = np.ascontiguousarray(system["frozen"], dtype=np.uint8)
        _chk(self.lib.mpmc_hip_upload(self.ctx, n, *[a.ctypes.data for a in arrs], mol.ctypes.data, frz.ctypes.data))
        self.n = n

    def set_dispersion(self, system, **flags):
        """PHAHST (mpmc_hip_set_dispersion), after upload(): the four switches and the per-atom c6 / c8 / c10 of
        `system` (atomic units; a missing array reads as zeros)."""
        p = DispParams(**{k: int(flags.get(k, 0)) for k in DISP_NAMES})
        n = self.n
        arrs = [np.ascontiguousarray(system.get(k, np.zeros(n)), dtype=np.float64) for k in ("c6", "c8", "c10")]
        for a in arrs:
            if a.shape != (n,):
                raise ValueError("c6 / c8 / c10 must have one entry per uploaded atom")
        _chk(self.lib.mpmc_hip_set_dispersion(self.ctx, C.byref(p), n, *[a.ctypes.data for a in arrs]))

    def set_axilrod_teller(self, system, enable=True, midzuno_kihara_approx=False):
        """The three-body term (mpmc_hip_set_axilrod_teller), after upload(): the per-atom c9 of `system` (atomic units; a
        missing array reads as zeros), or under midzuno_kihara_approx 3/4 alpha 6.7483345 c6 in its place
        (axilrod_teller.cpp:114-118).  enable=False switches the term off."""
        if not enable:
            _chk(self.lib.mpmc_hip_set_axilrod_teller(self.ctx, 0, 0, None))
            return
        c9 = effective_c9(system, midzuno_kihara_approx)
        if c9.shape != (self.n,):
            raise ValueError("c9 (c6, alpha) must have one entry per uploaded atom")
        _chk(self.lib.mpmc_hip_set_axilrod_teller(self.ctx, 1, self.n, c9.ctypes.data))

    def set_rd_crystal(self, order):
        """Lennard-Jones over lattice images (mpmc_hip_set_rd_crystal): order = rd_crystal_order, 1 .. 4; 0 switches the
        mode off.  A context setting: it persists across uploads."""
        _chk(self.lib.mpmc_hip_set_rd_crystal(self.ctx, int(order)))

    def set_rd_form(self, form, mixing="lb"):
        """The pair potential of rd_energy (mpmc_hip_set_rd_form): form "sg", "dreiding", "lj_buffered_14_7" or "lj"
        (Lennard-Jones on the dense path, for the mixing rules), "off" / None / 0 for the standard path; mixing "lb",
        "waldmanhagler", "halgren_mixing" or "c6_mixing".  A context setting: it persists across uploads."""
        form = "off" if not form else form
        if form not in RD_FORMS:
            raise ValueError("unknown rd form %r (one of %s)" % (form, ", ".join(RD_FORMS)))
        if mixing not in RD_MIXINGS:
            raise ValueError("unknown mixing rule %r (one of %s)" % (mixing, ", ".join(RD_MIXINGS)))
        p = RdFormParams(RD_FORMS[form], RD_MIXINGS[mixing])
        _chk(self.lib.mpmc_hip_set_rd_form(self.ctx, C.byref(p)))

    def set_vdw(self, system, enable=True):
        """Coupled-dipole van der Waals + repulsion-only Lennard-Jones (mpmc_hip_set_vdw), after upload(): the per-atom
        omega of `system` (atomic units) and its per-atom mol_type ids.  enable=False switches the mode off."""
        if not enable:
            _chk(self.lib.mpmc_hip_set_vdw(self.ctx, 0, 0, None, None))
            return
        omega = np.ascontiguousarray(system["omega"], dtype=np.float64)
        mtype = np.ascontiguousarray(system["mol_type"], dtype=np.int32)
        if omega.shape != (self.n,) or mtype.shape != (self.n,):
            raise ValueError("omega and mol_type must have one entry per uploaded atom")
        _chk(self.lib.mpmc_hip_set_vdw(self.ctx, 1, self.n, omega.ctypes.data, mtype.ctypes.data))

    def vdw_energy(self):
        """observables->vdw_energy of the last completed energy(); 0 while the mode is off."""
        v = C.c_double(0.0)
        _chk(self.lib.mpmc_hip_get_vdw_energy(self.ctx, C.byref(v)))
        return v.value

    def vdw_terms(self):
        """e_total, e_iso, lr_corr, repulsion, repulsion_lrc of the last completed energy() (mpmc_hip_get_vdw_terms)."""
        t = (C.c_double * 5)()
        _chk(self.lib.mpmc_hip_get_vdw_terms(self.ctx, t))
        return dict(zip(VDW_TERMS, [float(x) for x in t]))

    def set_exact_polar(self, enable):
        """The exact Thole dipoles (mpmc_hip_set_exact_polar; the reference's polar_iterative off): A mu = E_static by a
        Cholesky factorization on the device instead of an iterative solve.  A context setting: it persists across
        uploads."""
        _chk(self.lib.mpmc_hip_set_exact_polar(self.ctx, int(bool(enable))))

    def set_thole_model(self, damping="exponential", wolf_full=False):
        """The dipole tensor of the A matrix (mpmc_hip_set_thole_model): damping "exponential" (the default), "linear"
        (Thole's original model) or "off" / "none" (undamped; es_excluded pairs do not couple), as the reference's
        polar_damp_type; wolf_full = its polar_wolf_full (exponential only).  A context setting: it persists across
        uploads."""
        if isinstance(damping, str):
            if damping.lower() not in THOLE_DAMPINGS:
                raise ValueError("set_thole_model: damping %r is none of %s" % (damping, sorted(THOLE_DAMPINGS)))
            damping = THOLE_DAMPINGS[damping.lower()]
        m = TholeModel(int(damping), int(bool(wolf_full)))
        _chk(self.lib.mpmc_hip_set_thole_model(self.ctx, C.byref(m)))

    def polarizability_tensor(self):
        """The 3 x 3 molecular polarizability tensor (A^3) of the last completed energy() in the exact mode
        (mpmc_hip_get_polarizability_tensor; the reference's polarizability_tensor on)."""
        t = (C.c_double * 9)()
        _chk(self.lib.mpmc_hip_get_polarizability_tensor(self.ctx, t))
        return np.array([float(x) for x in t]).reshape(3, 3)

    def set_autoreject(self, scale):
        """cavity_autoreject_absolute (mpmc_hip_set_autoreject): scale = cavity_autoreject_scale; 0 switches it off.  A
        context setting: it persists across uploads."""
        _chk(self.lib.mpmc_hip_set_autoreject(self.ctx, float(scale)))

    def close_contacts(self):
        """Different-molecule pairs closer than the scale in the last completed energy(); 0 while the setting is off."""
        v = C.c_longlong(0)
        _chk(self.lib.mpmc_hip_get_close_contacts(self.ctx, C.byref(v)))
        return v.value

    def set_cavity_grid(self, grid_size, radius=0.0):
        """The cavity grid of cavity_bias (mpmc_hip_set_cavity_grid): grid_size = cavity_grid (1 .. 64; 0 switches it off),
        radius = cavity_radius.  A context setting: it persists across uploads; the occupancy is invalid until cavity_bin()."""
        _chk(self.lib.mpmc_hip_set_cavity_grid(self.ctx, int(grid_size), float(radius)))
        self.cavity_points = int(grid_size) ** 3

    def cavity_bin(self, pos):
        """The from-scratch occupancy of these positions [n, 3] (mpmc_hip_cavity_bin); n = 0 is valid."""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
        _chk(self.lib.mpmc_hip_cavity_bin(self.ctx, pos.shape[0], *[a.ctypes.data for a in cols]))

    def cavity_update(self, out_pos=(), in_pos=(), darts=()):
        """The edit (positions that leave / enter, [n, 3] each), the ordered list of the open points and the darts
        ([n, 3]) in one call (mpmc_hip_cavity_update).  Returns (cavities_open, hits), or None when the engine asks for
        cavity_bin() and a call with an empty edit instead."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in (out_pos, in_pos, darts)]
        n_open, hits = C.c_int(-1), C.c_int(-1)
        args = []
        for a in arrs:
            args += [a.shape[0], a.ctypes.data if a.shape[0] else None]
        rc = self.lib.mpmc_hip_cavity_update(self.ctx, *args, C.byref(n_open), C.byref(hits))
        if rc < 0:
            _chk(rc)
        if rc > 0:
            return None
        return n_open.value, hits.value

    def cavity_point(self, index):
        """(flat grid index, position [3]) of the index-th open point of the last cavity_update()."""
        g = C.c_int(-1)
        pos = (C.c_double * 3)()
        _chk(self.lib.mpmc_hip_cavity_point(self.ctx, int(index), C.byref(g), pos))
        return g.value, np.array([pos[0], pos[1], pos[2]])

    def cavity_grid(self, occupancy=True):
        """(occupancy [P] int32, positions [P, 3]) of the cavity grid (mpmc_hip_download_cavity_grid); occupancy=False gives
        None in its place (there is none before the first cavity_bin() of a grid or box)."""
        P = self.cavity_points
        occ = np.zeros(P, dtype=np.int32) if occupancy else None
        pos = np.zeros((P, 3))
        _chk(self.lib.mpmc_hip_download_cavity_grid(self.ctx, occ.ctypes.data if occupancy else None, pos.ctypes.data))
        return occ, pos

    def three_body_energy(self):
        """observables->three_body_energy of the last completed energy(); 0 while the term is off."""
        v = C.c_double(0.0)
        _chk(self.lib.mpmc_hip_get_three_body_energy(self.ctx, C.byref(v)))
        return v.value

    def load_system(self, system, params):
        """Convenience: params (incl. optional pbc_cutoff) + box + atoms (+ the dispersion record when the flags carry
        disp_expansion, + the three-body coefficients when they carry axilrod_teller, + omega and the type ids when they
        carry polarvdw).  cavity_autoreject_absolute + cavity_autoreject_scale switch the close-contact count on; without
        them it is switched off.  rd_crystal / rd_crystal_order among
        the flags switch the image sum on (order 1 when only rd_crystal is given); without them it is switched off.
        polar_iterative = 0 together with polarization switches the exact dipoles on; anything else switches them off.
        sg / dreiding / lj_buffered_14_7 switch that pair potential on (set_rd_form), waldmanhagler / halgren_mixing /
        c6_mixing name its mixing rule and, without another form, switch the dense Lennard-Jones form on; without any of
        the six the standard path is restored.  polar_damp_type ("exponential" | "linear" | "off" | "none") and
        polar_wolf_full name the dipole tensor (set_thole_model); without them the default, exponential, is restored."""
        self.set_thole_model(params.get("polar_damp_type", "exponential"), bool(params.get("polar_wolf_full")))
        self.set_exact_polar("polar_iterative" in params and not params["polar_iterative"]
                             and bool(params.get("polarization")))
        self.set_params(**params)
        self.set_rd_crystal(int(params.get("rd_crystal_order", 1)) if params.get("rd_crystal") else 0)
        self.set_rd_form(*rd_form_of(params))
        self.set_autoreject(float(params.get("cavity_autoreject_scale", 0.0))
                            if params.get("cavity_autoreject_absolute") else 0.0)
        self.set_box(system["basis"], params.get("pbc_cutoff", 0.0))
        self.upload(system)
        if params.get("disp_expansion"):
            self.set_dispersion(system, **{k: params[k] for k in DISP_NAMES if k in params})
        if params.get("axilrod_teller"):
            self.set_axilrod_teller(system, midzuno_kihara_approx=bool(params.get("midzuno_kihara_approx")))
        if params.get("polarvdw") or params.get("cdvdw"):
            self.set_vdw(system)

    def update_atoms(self, first, pos):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
        _chk(self.lib.mpmc_hip_update_atoms(self.ctx, int(first), pos.shape[0], *[a.ctypes.data for a in cols]))

    def insert_molecule(self, pos, charge, alpha, epsilon, sigma, mass, frozen=False):
        """One molecule enters the resident configuration (mpmc_hip_insert_molecule).  Returns its first slot, or
        None when the engine asks for a full upload instead."""
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (charge, alpha, epsilon, sigma, mass)]
        first = C.c_int(-1)
        rc = self.lib.mpmc_hip_insert_molecule(self.ctx, pos.shape[0], *[a.ctypes.data for a in cols + arrs],
                                               int(bool(frozen)), C.byref(first))
        if rc < 0:
            _chk(rc)
        if rc > 0:
            return None
        self.n = int(self.lib.mpmc_hip_slot_count(self.ctx))
        return first.value

    def remove_molecule(self, first, count):
        """The molecule in slots [first, first + count) leaves (mpmc_hip_remove_molecule); False = upload instead."""
        rc = self.lib.mpmc_hip_remove_molecule(self.ctx, int(first), int(count))
        if rc < 0:
            _chk(rc)
        return rc == 0

    def edit_molecules(self, remove=(), insert=()):
        """Several molecules leave and enter in one call (mpmc_hip_edit_molecules), in every mode with device-side edits.
        remove: (first, count) pairs, carried out first; insert: dicts with pos [k, 3], charge, alpha, epsilon, sigma,
        mass and optionally frozen, c6, c8, c10 (read under disp_expansion) and c9 (the EFFECTIVE coefficient, read under
        axilrod_teller).  Returns the list of the inserted molecules' first slots, or None when the engine asks for a
        full upload instead (nothing has changed then)."""
        remove = [(int(f), int(k)) for f, k in remove]
        rf = np.ascontiguousarray([f for f, _ in remove], dtype=np.int32)
        rk = np.ascontiguousarray([k for _, k in remove], dtype=np.int32)
        mols = (Molecule * max(1, len(insert)))()
        keep = []  # the arrays the structs point into
        for m, d in zip(mols, insert):
            pos = np.ascontiguousarray(d["pos"], dtype=np.float64).reshape(-1, 3)
            m.count, m.frozen = pos.shape[0], int(bool(d.get("frozen", False)))
            for k, name in enumerate("xyz"):
                keep.append(np.ascontiguousarray(pos[:, k]))
                setattr(m, name, keep[-1].ctypes.data)
            for field, key in (("charge", "charge"), ("polarizability", "alpha"), ("epsilon", "epsilon"),
                               ("sigma", "sigma"), ("mass", "mass"), ("c6", "c6"), ("c8", "c8"), ("c10", "c10"), ("c9", "c9")):
                if d.get(key) is None:
                    continue  # (a NULL pointer: the engine names a missing array its mode reads)
                a = np.ascontiguousarray(d[key], dtype=np.float64)
                if a.shape != (pos.shape[0],):
                    raise ValueError("edit_molecules: %s must have one entry per atom of the molecule" % key)
                keep.append(a)
                setattr(m, field, a.ctypes.data)
        first = np.full(max(1, len(insert)), -1, dtype=np.int32)
        rc = self.lib.mpmc_hip_edit_molecules(self.ctx, len(remove), rf.ctypes.data if remove else None,
                                              rk.ctypes.data if remove else None, len(insert),
                                              mols if len(insert) else None, first.ctypes.data if len(insert) else None)
        if rc < 0:
            _chk(rc)
        if rc > 0:
            return None
        self.n = int(self.lib.mpmc_hip_slot_count(self.ctx))
        return [int(f) for f in first[:len(insert)]]

    def set_sweep_order(self, slots):
        """Gauss-Seidel modes after insert / remove: device slots of the polarizable atoms in the caller's atom order."""
        a = np.ascontiguousarray(slots, dtype=np.int32)
        _chk(self.lib.mpmc_hip_set_sweep_order(self.ctx, len(a), a.ctypes.data))

    def dimer_energies(self, a, b, conf, mu=False, **flags):
        """Energies of the non-periodic dimer a + b at the placements conf [n, 7] = (r, alpha1, beta1, gamma1, alpha2, beta2,
        gamma2) (mpmc_hip_dimer_energies).  a, b: dicts with pos [k, 3], charge, alpha, epsilon, sigma, mass and, under
        disp_expansion, c6 / c8 / c10; flags: make_dimer_params().  Returns dict(es, rd, polar [n], iterations [n],
        not_converged [n]) and with mu=True the dipoles mu [n, 32, 3] (a's sites first, then b's)."""
        p = flags.pop("_struct", None) or make_dimer_params(**flags)
        conf = np.ascontiguousarray(conf, dtype=np.float64).reshape(-1, 7)
        n = conf.shape[0]
        keep = []
        ma, mb = _dimer_molecule(a, keep), _dimer_molecule(b, keep)
        out = {k: np.zeros(n) for k in ("es", "rd", "polar")}
        status = np.zeros(n, dtype=np.int32)
        dip = np.zeros((n, DIMER_SITES, 3)) if mu else None
        _chk(self.lib.mpmc_hip_dimer_energies(self.ctx, C.byref(p), C.byref(ma), C.byref(mb), n, conf.ctypes.data,
                                              out["es"].ctypes.data, out["rd"].ctypes.data, out["polar"].ctypes.data,
                                              status.ctypes.data, dip.ctypes.data if mu else None))
        out["iterations"] = status & ~DIMER_NOT_CONVERGED
        out["not_converged"] = (status & DIMER_NOT_CONVERGED) != 0
        if mu:
            out["mu"] = dip
        return out

    def dimer_grid_means(self, a, b, r, angles, **flags):
        """Means of es, rd and polar over the Cartesian product of six angle lists (alpha1, beta1, gamma1, alpha2, beta2,
        gamma2; the last fastest) at separation r (mpmc_hip_dimer_grid_means).  Returns dict(es, rd, polar, count,
        not_converged)."""
        p = flags.pop("_struct", None) or make_dimer_params(**flags)
        lists = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in angles]
        if len(lists) != 6:
            raise ValueError("dimer_grid_means: six angle lists")
        keep = []
        ma, mb = _dimer_molecule(a, keep), _dimer_molecule(b, keep)
        n = (C.c_int * 6)(*[len(x) for x in lists])
        ptrs = (C.c_void_p * 6)(*[x.ctypes.data for x in lists])
        means = (C.c_double * 3)()
        counts = (C.c_longlong * 2)()
        _chk(self.lib.mpmc_hip_dimer_grid_means(self.ctx, C.byref(p), C.byref(ma), C.byref(mb), float(r), n, ptrs, means,
                                                counts))
        return dict(es=means[0], rd=means[1], polar=means[2], count=int(counts[0]), not_converged=int(counts[1]))

    def trial_energies(self, first, xyz, terms=False):
        """Total energies of the resident configuration with the molecule in slots [first, first + k) at each of the
        placements xyz [ntrial, k, 3] (mpmc_hip_trial_energies); the configuration is left as it is.  Needs a completed
        energy() on the current configuration.  Returns energy [ntrial]; with terms=True (batched path only) the pair
        (energy, terms [ntrial, 3]) with the molecule's rd, es_real and es_recip per placement."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if xyz.ndim != 3 or xyz.shape[2] != 3:
            raise ValueError("trial_energies: xyz must be [ntrial, sites, 3]")
        nt, k = xyz.shape[0], xyz.shape[1]
        e = np.zeros(nt)
        tr = np.zeros((nt, 3)) if terms else None
        _chk(self.lib.mpmc_hip_trial_energies(self.ctx, int(first), k, nt, xyz.ctypes.data, e.ctypes.data,
                                              tr.ctypes.data if terms else None))
        return (e, tr) if terms else e

    def trial_call_count(self):
        """mpmc_hip_trial_energies() calls of this context that passed their checks."""
        return int(self.lib.mpmc_hip_trial_call_count(self.ctx))

    def energy(self):
        r = Result()
        _chk(self.lib.mpmc_hip_energy(self.ctx, C.byref(r)))
        return {f: getattr(r, f) for f, _ in Result._fields_}

    def energy_begin(self):
        _chk(self.lib.mpmc_hip_energy_begin(self.ctx))

    def energy_end(self):
        r = Result()
        _chk(self.lib.mpmc_hip_energy_end(self.ctx, C.byref(r)))
        return {f: getattr(r, f) for f, _ in Result._fields_}

    def dipoles(self):
        out = {k: np.zeros((self.n, 3)) for k in ("mu", "ef_static", "ef_induced", "ef_induced_change")}
        _chk(self.lib.mpmc_hip_download_dipoles(self.ctx, out["mu"].ctypes.data, out["ef_static"].ctypes.data,
                                                out["ef_induced"].ctypes.data,
                                                out["ef_induced_change"].ctypes.data))
        return out

    def amatrix(self):
        A = np.zeros((3 * self.n, 3 * self.n))
        _chk(self.lib.mpmc_hip_download_amatrix(self.ctx, A.ctypes.data))
        return A

    def ranking(self):
        rank = np.zeros(self.n)
        order = np.zeros(self.n, dtype=np.int32)
        _chk(self.lib.mpmc_hip_download_ranking(self.ctx, rank.ctypes.data, order.ctypes.data))
        return rank, order

    def timings(self):
        t = Timings()
        _chk(self.lib.mpmc_hip_get_timings(self.ctx, C.byref(t)))
        return {f: getattr(t, f) for f, _ in Timings._fields_}
