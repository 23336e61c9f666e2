"""CPU-only tests of the NPT ensemble: keywords, the volume move of the C host layer against a restatement of the
reference's arithmetic (mc_moves.c:168-248, checkpoint.c:84-98), and the presence of the device entry point and its
kernel in the built library.  Energies need the GPU: tests/test_gpu_npt.py."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from mpmc_amd import engine, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQR = os.path.join(ROOT, "tests", "data", "bssp_small", "small.initial.pqr")
LIB = os.path.join(ROOT, "mpmc_amd", "csrc", "libmpmc_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    if not os.path.exists(host.LIB_PATH) or not os.path.exists(engine.LIB_PATH):
        g.build()


NPT_INPUT = ("ensemble npt\ntemperature 77\n%sbasis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\n"
             "numsteps 10\npqr_input " + PQR + "\n")


# ---- 1. keywords -----------------------------------------------------------------------------------------------
def test_npt_keywords_are_accepted(tmp_path):
    (tmp_path / "in").write_text(NPT_INPUT % "pressure 1.5\nvolume_probability 0.25\nvolume_change_factor 0.1\n")
    lib = host.load()
    p = lib.setup_system(str(tmp_path / "in").encode())
    assert p
    lib.free_system(p)
    # the defaults (reference input.c:1608-1611): volume_probability 0, volume_change_factor 0.25
    (tmp_path / "in2").write_text(NPT_INPUT % "pressure 1.5\n")
    p = lib.setup_system(str(tmp_path / "in2").encode())
    assert p
    lib.free_system(p)


def test_npt_without_pressure_is_rejected(tmp_path):
    """reference check_input.c:673-678"""
    (tmp_path / "in").write_text(NPT_INPUT % "volume_probability 0.25\n")
    assert not host.load().setup_system(str(tmp_path / "in").encode())
    with pytest.raises(ValueError):
        host.HostSystem(synth.s_pol(20), synth.FLAGS_POL_JACOBI, extra={"ensemble": "npt"})


# ---- restatement of the reference in Python floats (IEEE doubles; math.* is the C library's) --------------------
def volume_of(b):
    """pbc_volume(), pbc.c:36-44"""
    v = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1])
    v += b[0][1] * (b[1][2] * b[2][0] - b[1][0] * b[2][2])
    v += b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0])
    return v


def centres_of_mass(s, pos):
    """update_com(), pairs.c:364-385: sums in atom order, then one division"""
    mol = np.asarray(s["molecule"])
    out = []
    for m in sorted(set(mol.tolist()), key=lambda k: int(np.flatnonzero(mol == k)[0])):
        mass, com = 0.0, [0.0, 0.0, 0.0]
        for i in np.flatnonzero(mol == m):
            mass += float(s["mass"][i])
            for p in range(3):
                com[p] += float(s["mass"][i]) * float(pos[i, p])
        out.append([c / mass for c in com])
    return out


def scaled(s, pos, com, basis, new_volume):
    """mc_moves.c:184-207 (and :221-245): basis, volume, per-molecule displacement, positions"""
    old_volume = volume_of(basis)
    f = math.pow(new_volume / old_volume, 1.0 / 3.0)
    nb = [[basis[i][j] * f for j in range(3)] for i in range(3)]
    mol = np.asarray(s["molecule"])
    first = {}
    for i, m in enumerate(mol.tolist()):
        first.setdefault(m, len(first))
    npos = np.array(pos, dtype=np.float64)
    delta = []
    for k in range(len(com)):
        delta.append([com[k][p] * f - com[k][p] for p in range(3)])
    for i in range(len(npos)):
        for p in range(3):
            npos[i, p] = float(pos[i, p]) + delta[first[int(mol[i])]][p]
    return nb, volume_of(nb), np.array(delta), npos, f


def npt_host(s, flags, seed, volume_probability, factor=0.25):
    h = host.HostSystem(s, flags, seed=seed, extra={"ensemble": "npt", "pressure": 1.0,
                                                     "volume_probability": repr(volume_probability),
                                                     "volume_change_factor": repr(factor)})
    return h


def draws(s, flags, seed, n):
    """the first n numbers of the get_rand() stream of that seed"""
    h = host.HostSystem(s, flags, seed=seed)
    out = [h.lib.host_get_rand(h.ptr) for _ in range(n)]
    h.close()
    return out


# ---- 2. the move itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume_probability", [0.0, 1.0])
def test_volume_change_is_rigid_bit_exact_and_draws_like_the_reference(volume_probability):
    s = synth.s_pol(52)  # 10 five-site molecules + 2 single sites; every one of them is shifted
    seed, factor = 4711, 0.25
    u = draws(s, synth.FLAGS_POL_JACOBI, seed, 4)
    h = npt_host(s, synth.FLAGS_POL_JACOBI, seed, volume_probability, factor)
    lib = h.lib
    basis0 = h.basis().tolist()
    cutoff0 = h.observables()["cutoff"]
    assert cutoff0 == 0.5 * min(np.linalg.norm(np.array(basis0), axis=1))
    lib.host_init_chain_no_energy(h.ptr)  # update_com + N + checkpoint(): the move decision, then the molecule pick
    nmol = len(set(s["molecule"].tolist()))
    # checkpoint.c:84-98: one draw for the decision -- against 1/N when volume_probability is not set --, and the draw
    # of the molecule pick (:126) still happens
    threshold = volume_probability if volume_probability != 0.0 else 1.0 / nmol
    assert h.next_movetype() == ("volume" if u[0] < threshold else "displace")
    if volume_probability == 1.0:
        lib.make_move(h.ptr)  # through make_move()'s new case
    else:
        lib.volume_change(h.ptr)
    # mc_moves.c:180: one draw
    new_volume = math.exp(math.log(volume_of(basis0)) + (u[2] - 0.5) * factor)
    com = centres_of_mass(s, s["pos"])
    nb, nvol, delta, npos, _ = scaled(s, s["pos"], com, basis0, new_volume)
    got = h.positions()
    assert np.array_equal(h.basis(), np.array(nb))
    obs = h.observables()
    assert obs["volume"] == nvol and nvol != volume_of(basis0)
    assert obs["cutoff"] == cutoff0  # pbc() keeps a cutoff once it is set (pbc.c:71)
    assert np.array_equal(got, npos)
    # rigid: every atom is exactly pos + delta of its molecule
    first = {}
    for m in s["molecule"].tolist():
        first.setdefault(m, len(first))
    for i in range(len(got)):
        assert np.array_equal(got[i], s["pos"][i] + delta[first[int(s["molecule"][i])]])
    # exactly three numbers were consumed
    assert lib.host_get_rand(h.ptr) == u[3]
    h.close()


def test_npt_checkpoint_mixes_volume_and_displacement_moves():
    """volume_probability 0.3: the decision follows the first draw of every checkpoint()"""
    s = synth.s_pol(50)
    h = npt_host(s, synth.FLAGS_POL_JACOBI, 99, 0.3)
    ref = host.HostSystem(s, synth.FLAGS_POL_JACOBI, seed=99)
    h.lib.host_init_chain_no_energy(h.ptr)
    kinds = set()
    for _ in range(40):
        u0 = ref.lib.host_get_rand(ref.ptr)
        ref.lib.host_get_rand(ref.ptr)
        kind = h.next_movetype()
        assert kind == ("volume" if u0 < 0.3 else "displace")
        kinds.add(kind)
        h.lib.checkpoint(h.ptr)
    assert kinds == {"volume", "displace"}
    h.close()
    ref.close()


# ---- 3. change + revert ------------------------------------------------------------------------------------------
def test_revert_restores_volume_and_positions_to_rounding():
    """revert_volume_change() is arithmetic (mc_moves.c:213-248), not a restore from a copy.

    Bound, in units of ulp(M), M = the largest |coordinate| (atoms and centres of mass) met on the way: a coordinate
    goes through pos + (c f1 - c) and then + (c' f2 - c'): two products, two differences and two additions, each
    rounded once at a magnitude of at most M: 6 x 1/2 = 3 ulp.  c' is the centre of mass update_com() recomputes from
    the shifted atoms (a weighted mean of at most 5 atoms: 5 products, 4 + 4 additions and a division behind it, about
    (5 + 2) / 2 = 3.5 ulp), and f1 f2 differs from 1 by the errors of two pow() (1 ulp each), of the two volume
    quotients (1/2 each) and of the scaled basis' determinant (three roundings per term and per factor, some 4 ulp,
    a third of which survives the cube root): about 4.5 ulp relative, times |c| <= M.  Together 11 ulp; the test
    allows 16.  The volume itself is the determinant of the basis scaled by f1 f2: three times that relative error
    plus the determinant's own, below 32 ulp of the volume."""
    s = synth.s_pol(52)
    for factor in (0.97, 1.03):
        h = npt_host(s, synth.FLAGS_POL_JACOBI, 5, 0.3)
        h.lib.host_init_chain_no_energy(h.ptr)
        pos0, basis0 = h.positions(), h.basis().tolist()
        obs0 = h.observables()
        v0 = volume_of(basis0)
        h.force_volume_move(factor * v0)
        assert np.max(np.abs(h.positions() - pos0)) > 1e-3
        h.close()
        h = npt_host(s, synth.FLAGS_POL_JACOBI, 5, 0.3)
        h.lib.host_init_chain_no_energy(h.ptr)
        h.force_volume_move(factor * v0, revert=True)
        # the restatement, bit for bit: change, the centres of mass the energy() in between recomputes, revert
        com0 = centres_of_mass(s, pos0)
        nb, nvol, _, p1, _ = scaled(s, pos0, com0, basis0, factor * v0)
        com1 = centres_of_mass(s, p1)
        rb, rvol, _, p2, _ = scaled(s, p1, com1, nb, v0)
        assert np.array_equal(h.positions(), p2) and np.array_equal(h.basis(), np.array(rb))
        obs = h.observables()
        assert obs["volume"] == rvol
        M = max(factor, 1.0) * max(np.max(np.abs(pos0)), np.max(np.abs(np.array(com0))))
        err = np.max(np.abs(p2 - pos0))
        print("revert (x%.2f): max |pos - pos0| = %.3e = %.2f ulp(M); V/V0 - 1 = %.3e" %
              (factor, err, err / np.spacing(M), rvol / v0 - 1.0))
        assert err <= 16 * np.spacing(M)
        assert abs(rvol / v0 - 1.0) < 32 * 2.0 ** -52
        # the observables are the ones copied back from the checkpoint
        for k in ("energy", "coulombic_energy", "rd_energy", "polarization_energy", "N"):
            assert obs[k] == obs0[k]
        h.close()


# ---- 4. the device entry point and its kernel ----------------------------------------------------------------------
def test_scale_box_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mpmc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+mpmc_hip_scale_box\s*\(\s*mpmc_hip_ctx\s*\*\s*ctx,\s*const double basis\[9\],\s*double pbc_cutoff,"
                     r"\s*int n_molecules,\s*const double \*delta\s*\)", hdr)
    assert "mpmc_hip_scale_box" in engine.EXPORTS
    lib = engine.load()
    assert hasattr(lib, "mpmc_hip_scale_box") and lib.mpmc_hip_scale_box.argtypes is not None
    assert callable(getattr(engine.Engine, "scale_box"))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert re.search(r"\bT mpmc_hip_scale_box\b", exported)
    assert lib.mpmc_hip_abi_version() == 1
    hostlib = subprocess.check_output(["nm", "-D", "--defined-only", host.LIB_PATH], text=True)
    for name in ("energy_hip_note_volume_change", "volume_change", "revert_volume_change", "host_get_basis",
                 "host_force_volume_move"):
        assert re.search(r"\bT %s\b" % name, hostlib), name


def test_code_object_has_the_volume_kernel_without_scratch(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "mpmc.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", LIB, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    hits = []
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name and "shift_molecules_kernel" in name.group(1):
            field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1))
            hits.append((field("private_segment_fixed_size"), field("vgpr_spill_count"), field("sgpr_spill_count")))
    assert hits == [(0, 0, 0)]
