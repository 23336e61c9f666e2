"""quantum_rotation on the CPU: the independent model (tests/qrot_reference.py) against closed forms, and the host
layer's pieces (mpmc_amd/host/qrot.c, through ctypes) against the model -- Y_lm, the quadrature, the C Jacobi solver,
the symmetry test, the parser and its refusals, and the move-type draw order.

The Jacobi bound.  One rotation replaces two rows and two columns by combinations with |c|, |s| <= 1: a handful of
roundings per element, <= 4 u of the element's size.  In a sweep every element is touched by the 2 dim - 3 rotations that
share an index with it, so a sweep perturbs the matrix by <= 8 dim u ||H||_F in the Frobenius norm, and by Weyl every
eigenvalue by as much.  With the sweeps the solver reports (qrot_jacobi returns them) and one more for the stopping
threshold (off-diagonal norm <= u ||H||_F) and numpy's own eigh:  |lambda - lambda_eigh| <= 8 (sweeps + 1) dim u ||H||_F,
u = 2^-53.  The residual ||H v - lambda v|| is held to the same bound.  The largest ratio seen is printed
(profiles/quantum_rotation/README.md records it)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import qrot_reference as qr
from mpmc_amd import host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    return host.load()


def c_jacobi(lib, H):
    dim = H.shape[0]
    h = np.ascontiguousarray(np.stack([H.real, H.imag], axis=-1), dtype=np.float64)
    ev, vec = np.zeros(dim), np.zeros((dim, dim, 2))
    rot = C.c_long(0)
    sweeps = lib.qrot_jacobi(dim, h.ctypes.data, ev.ctypes.data, vec.ctypes.data, C.byref(rot))
    assert sweeps >= 0, "the solver did not converge"
    return ev, vec[..., 0] + 1j * vec[..., 1], sweeps, rot.value


def c_hindered_hamiltonian(lib, l_max, B, barrier):
    V = np.zeros((16, 16))
    lib.qrot_hindered_grid(B, barrier, V.ctypes.data)
    dim = (l_max + 1) ** 2
    h = np.zeros((dim, dim, 2))
    lib.qrot_hamiltonian(l_max, B, V.ctypes.data, h.ctypes.data)
    return V, h[..., 0] + 1j * h[..., 1]


def test_the_model_s_ylm_are_the_closed_forms():
    rng = np.random.default_rng(0)
    theta, phi = rng.uniform(0, 2 * math.pi, 50), rng.uniform(0, 4 * math.pi, 50)  # (theta beyond pi: sin enters signed)
    for l in range(3):
        for m in range(-l, l + 1):
            re, im = qr.ylm(l, m, theta, phi)
            want = qr.closed_form(l, m, theta, phi)
            assert np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - want).max() < 4e-16, (l, m)


def test_the_c_basis_is_the_model_s(lib):
    rng = np.random.default_rng(1)
    theta = np.concatenate([qr.THETA, rng.uniform(0, 2 * math.pi, 8)])
    phi = np.concatenate([qr.PHI, rng.uniform(0, 3 * math.pi, 8)])
    worst = 0.0
    for l in range(9):
        for m in range(-l, l + 1):
            re, im = qr.ylm(l, m, theta, phi)
            got_re = np.array([lib.qrot_basis(0, l, m, t, p) for t, p in zip(theta, phi)])
            got_im = np.array([lib.qrot_basis(1, l, m, t, p) for t, p in zip(theta, phi)])
            worst = max(worst, np.abs(got_re - re.astype(np.float64)).max(), np.abs(got_im - im.astype(np.float64)).max())
    assert worst < 2e-14, worst  # |Y| <= 1.6; the recurrence of l = 8 is ~30 operations


def test_the_grid_is_gauss_legendre_16():
    x, w = np.polynomial.legendre.leggauss(16)
    assert np.abs(qr._ROOTS - x).max() < 2e-16 and abs(w.sum() - 2.0) < 1e-15


@pytest.mark.parametrize("l_max", [1, 4, 7, 8])
def test_orthonormality_under_the_quadrature(lib, l_max):
    """<lm|l'm'> with the grid's sin(theta): the identity to the quadrature's own error, which the MODEL states and this
    test prints -- it is far above rounding and grows with l.  The C Hamiltonian of the potential 1 with B = 0 is that
    overlap matrix, and must agree with the model's to rounding."""
    S, err = qr.overlap(l_max)
    print("l_max %d: largest |<lm|l'm'> - delta| under the 16 x 16 quadrature = %.3e" % (l_max, err))
    V = np.repeat(np.sin(qr.THETA_C)[:, None], 16, axis=1).copy()
    dim = (l_max + 1) ** 2
    h = np.zeros((dim, dim, 2))
    lib.qrot_hamiltonian(l_max, 0.0, V.ctypes.data, h.ctypes.data)
    got = h[..., 0] + 1j * h[..., 1]
    assert np.abs(got - S).max() < 1e-13
    assert np.abs(got - np.eye(dim)).max() <= err + 1e-13
    # (err is a statement about the reference's grid, not about the code: 5e-16 at l_max 1, 6e-3 at 4, 0.6 at 7 -- the phi
    #  integral of e^{i (m' - m) phi} by a 16-point Gauss-Legendre rule on [0, 2 pi] is poor beyond |m' - m| ~ 8 -- and the
    #  levels are DEFINED with it)


CASES = [(l_max, barrier) for l_max in (1, 4, 7, 8) for barrier in (0.0, 1.0, 10.0, 100.0)]


@pytest.mark.parametrize("l_max,barrier", CASES)
def test_jacobi_on_the_hindered_rotor(lib, l_max, barrier):
    B = 85.35060622
    V, H = c_hindered_hamiltonian(lib, l_max, B, barrier)
    assert np.abs(V - qr.hindered_grid(B, barrier)).max() < 1e-12 * max(1.0, B * barrier)
    Hm = qr.hamiltonian(V, l_max, B)
    dim = H.shape[0]
    norm = np.linalg.norm(Hm)
    assert np.abs(H - Hm).max() <= 64 * 256 * U * max(norm, 1.0)  # a 256-term sum of products, fp64 against longdouble
    assert np.array_equal(H, H.conj().T)
    ev, vec, sweeps, rot = c_jacobi(lib, H)
    want = np.linalg.eigh(H)[0]
    bound = 8 * (sweeps + 1) * dim * U * np.linalg.norm(H)
    resid = max(np.linalg.norm(H @ vec[i] - ev[i] * vec[i]) for i in range(dim))
    print("hindered l_max %d barrier %g: %d sweeps, %d rotations, |dlambda| / bound = %.3f, residual / bound = %.3f"
          % (l_max, barrier, sweeps, rot, np.abs(ev - want).max() / bound, resid / bound))
    assert (np.diff(ev) >= 0).all()
    assert np.abs(ev - want).max() <= bound and resid <= bound
    assert np.abs(vec.conj() @ vec.T - np.eye(dim)).max() <= 8 * (sweeps + 1) * dim * U
    if barrier == 0.0:  # the free rotor: the potential is exactly 0 on the grid, the levels are B l (l + 1), 2l + 1 times
        free = np.sort([B * l * (l + 1) for l, _ in qr.index_lm(l_max)])
        assert np.abs(ev - free).max() <= bound


@pytest.mark.parametrize("dim", [4, 49, 81])
def test_jacobi_on_random_hermitian_matrices_with_degenerate_pairs(lib, dim):
    rng = np.random.default_rng(dim)
    lam = np.sort(rng.normal(size=dim) * 100.0)
    lam[1] = lam[0]
    lam[dim - 1] = lam[dim - 2]
    lam[dim // 2] = lam[dim // 2 - 1]
    Q = np.linalg.qr(rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)))[0]
    H = (Q * lam) @ Q.conj().T
    H = 0.5 * (H + H.conj().T)
    ev, vec, sweeps, rot = c_jacobi(lib, H)
    bound = 8 * (sweeps + 1) * dim * U * np.linalg.norm(H)
    resid = max(np.linalg.norm(H @ vec[i] - ev[i] * vec[i]) for i in range(dim))
    want = np.linalg.eigh(H)[0]
    print("random dim %d: %d sweeps, %d rotations, |dlambda| / bound = %.3f, residual / bound = %.3f"
          % (dim, sweeps, rot, np.abs(ev - want).max() / bound, resid / bound))
    assert np.abs(ev - want).max() <= bound and np.abs(ev - np.sort(lam)).max() <= bound and resid <= bound


def _cpu_system(flags, seed=11, extra=None, n=10, system=None):
    return host.HostSystem(system or synth.s_pol(n), flags, seed=seed, extra=extra)


QROT = dict(temperature=50.0, rd_only=1, quantum_rotation=1, quantum_rotation_B=85.35060622, quantum_rotation_l_max=4,
            quantum_rotation_level_max=25, quantum_rotation_sum=10)


def test_symmetries_and_partition_functions_do_not_depend_on_the_solver_s_vectors(lib):
    """Every eigenvector times a random phase, degenerate pairs mixed by a random unitary: the same symmetries from the
    same random numbers, and so the same partition functions.  (In the hindered rotor |m| and the parity of l are good
    quantum numbers, and the reference's map (theta + pi, phi + pi) multiplies Y_lm by (-1)^(l + m): the sign it reads
    off is a property of the level, not of the vector picked in its eigenspace.)"""
    l_max, B = 4, 85.35060622
    _, H = c_hindered_hamiltonian(lib, l_max, B, 10.0)
    ev, vec, _, _ = c_jacobi(lib, H)
    dim = len(ev)
    rng = np.random.default_rng(5)
    mixed = vec * np.exp(1j * rng.uniform(0, 2 * math.pi, dim))[:, None]
    i = 0
    while i + 1 < dim:
        if abs(ev[i + 1] - ev[i]) < 1e-9 * B:
            Q = np.linalg.qr(rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2)))[0]
            mixed[i:i + 2] = Q @ mixed[i:i + 2]
            i += 2
        else:
            i += 1
    assert max(np.linalg.norm(H @ mixed[i] - ev[i] * mixed[i]) for i in range(dim)) < 1e-10 * np.linalg.norm(H)

    def symmetries(vectors, who):
        hs = _cpu_system(QROT, seed=77)
        try:
            out = []
            for v in vectors:
                flat = np.ascontiguousarray(np.stack([v.real, v.imag], axis=-1))
                out.append(lib.qrot_symmetry(hs.ptr, l_max, flat.ctypes.data))
            return out
        finally:
            hs.close()

    a, b = symmetries(vec, "solver"), symmetries(mixed, "mixed")
    model_rng = qr.new_rng(77)
    model = [qr.symmetry(v, l_max, model_rng) for v in vec]
    assert a == b == model
    assert 0 < sum(a) < dim
    assert qr.partition_functions(ev, a, 10, 50.0, qr.PARA) == qr.partition_functions(ev, b, 10, 50.0, qr.PARA)


def test_placements_are_the_model_s(lib):
    lib.qrot_placements.argtypes = [C.c_void_p, C.c_void_p]
    system = synth.s_pol(10)
    hs = _cpu_system(QROT, system=system)
    try:
        lib.host_init_chain_no_energy(hs.ptr)  # (update_com)
        pos = system["pos"][:5]  # the first movable molecule
        mass = system["mass"][:5]
        com = np.zeros(3)
        tot = 0.0
        for k in range(5):  # update_com(): summed in site order
            tot += mass[k]
            com += mass[k] * pos[k]
        com /= tot
        want = qr.placements(pos, com)
        got = np.zeros((256, 5, 3))
        assert lib.host_qrot_placements(hs.ptr, 0, got.ctypes.data) == 5
        assert np.abs(got - want).max() < 1e-14
        d0 = np.linalg.norm(pos[:, None] - pos[None], axis=2)
        for p in got[::17]:
            assert np.abs(np.linalg.norm(p[:, None] - p[None], axis=2) - d0).max() < 1e-13  # rigid
    finally:
        hs.close()


@pytest.mark.parametrize("change,extra,why", [
    (dict(quantum_rotation_B=0.0), None, "invalid quantum rotational constant B"),
    (dict(quantum_rotation_l_max=9, quantum_rotation_level_max=25), None, "quantum_rotation_l_max above 8 is refused"),
    (dict(quantum_rotation_l_max=0), None, "invalid quantum rotation l_max"),
    (dict(quantum_rotation_level_max=0), None, "invalid quantum rotation level max"),
    (dict(quantum_rotation_level_max=26), None, "quantum rotational levels cannot exceed"),
    (dict(quantum_rotation_sum=26), None, "quantum rotational sum for partition function invalid"),
    (dict(quantum_rotation_sum=0), None, "quantum rotational sum for partition function invalid"),
    (dict(), dict(ensemble="npt", pressure=1.0), "quantum_rotation with ensemble npt or surf is not implemented"),
    (dict(), dict(ensemble="surf"), "quantum_rotation with ensemble npt or surf is not implemented"),
])
def test_the_keyword_block_s_refusals(change, extra, why, capfd):
    with pytest.raises(ValueError):
        _cpu_system(dict(QROT, **change), extra=extra)
    assert why in capfd.readouterr().err  # refused by name
    _cpu_system(QROT).close()  # (the unchanged block is accepted)


def test_a_movable_molecule_of_one_site_is_refused(capfd):
    with pytest.raises(ValueError):
        _cpu_system(QROT, system=synth.s_lj(8))
    assert "needs at least two sites on every movable molecule" in capfd.readouterr().err


def test_the_sample_s_keyword_file_is_read(lib, capfd, tmp_path):
    import shutil
    gold = os.path.join(ROOT, "tests", "golden", "qrot")
    shutil.copy(os.path.join(gold, "MOF5+QR.inp"), tmp_path / "MOF5+QR.inp")
    shutil.copy(os.path.join(gold, "MOF5+alpha.pdb"), tmp_path / "input.pqr")  # (the keyword file names input.pqr)
    lib.setup_system.restype = C.c_void_p
    ptr = lib.setup_system(str(tmp_path / "MOF5+QR.inp").encode())
    assert ptr
    out = capfd.readouterr().out
    assert "Quantum rotational eigenspectrum calculation enabled" in out and "Quantum rotation l_max = 7" in out
    lib.free_system(C.c_void_p(ptr))


@pytest.mark.parametrize("ensemble", ["nvt", "uvt"])
def test_move_type_draws(lib, ensemble):
    """checkpoint()'s draws under quantum_rotation against the numpy restatement: 300 checkpoints, one seed."""
    extra = dict(spinflip_probability=0.5)
    if ensemble == "uvt":
        extra.update(ensemble="uvt", insert_probability=0.3, pressure=1.0)
    hs = _cpu_system(QROT, seed=4242, extra=extra)
    try:
        rng = qr.new_rng(4242)
        lib.host_init_chain_no_energy(hs.ptr)
        lib.checkpoint.argtypes = [C.c_void_p]
        lib.checkpoint.restype = None
        kinds = []
        for _ in range(300):
            want, _ = qr.movetype_draw(rng, ensemble, 0.5, 0.3)
            kinds.append(want)
            assert hs.next_movetype() == want
            lib.checkpoint(hs.ptr)
        assert {"displace", "spinflip"} <= set(kinds) and (ensemble == "nvt" or {"insert", "remove"} <= set(kinds))
    finally:
        hs.close()
