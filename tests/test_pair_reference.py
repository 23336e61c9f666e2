"""The per-pair reference (tests/pair_reference.py) against the CPU oracle on generic inputs: pins the helper that the
adversarial-geometry tests rely on to the oracle, and the oracle to an independent restatement of the pair sums."""
import numpy as np
import pytest

import pair_reference as pr
from mpmc_amd import synth
from oracle import oracle

RTOL = 1e-10  # the suite's energy bar (tests/test_gpu_parity.py)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def sheared_es_432():
    s = synth.s_es(432)
    L = s["basis"][0, 0]
    s["basis"] = np.array([[L, 0, 0], [0.2 * L, 0.95 * L, 0], [0.1 * L, -0.15 * L, 0.9 * L]])  # test_triclinic_box
    return s


POL = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_max_iter=2)
CASES = {
    "lj256": (lambda: synth.s_lj(256), synth.FLAGS_LJ),
    "lj256_fh4": (lambda: synth.s_lj(256), dict(temperature=100.0, rd_only=1, feynman_hibbs=1, feynman_hibbs_order=4)),
    "es432_sheared_fh4": (sheared_es_432, dict(temperature=100.0, feynman_hibbs=1, feynman_hibbs_order=4)),
    "es432_sheared": (sheared_es_432, dict(temperature=100.0)),
    "es432_sheared_wolf": (sheared_es_432, dict(temperature=100.0, wolf=1)),
    "pol320_bare": (lambda: synth.s_pol(320), POL),
    "pol320_wolf0": (lambda: synth.s_pol(320), dict(POL, polar_wolf=1)),
    "pol320_wolf": (lambda: synth.s_pol(320), dict(POL, polar_wolf=1, polar_wolf_alpha=0.13)),
    "pol320_ewald": (lambda: synth.s_pol(320), dict(POL, polar_ewald=1)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_pair_table_sums_match_the_oracle(case):
    make, p = CASES[case]
    s = make()
    t = pr.pair_table(s, p)
    got = pr.sums(t, s, p)
    pol = bool(p.get("polarization"))
    want = oracle.energy(s, p, want_vectors=pol)
    assert t["rc"] == want["cutoff"] and t["volume"] == want["volume"]
    assert rel(got["rd_energy"], want["rd_energy"]) < RTOL, (got["rd_energy"], want["rd_energy"])
    assert rel(got["es_real"], want["es_real"]) < RTOL, (got["es_real"], want["es_real"])
    if not p.get("rd_only"):
        assert want["es_real"] != 0.0
    if pol:
        scale = np.abs(want["ef_static"]).max()
        assert np.abs(got["ef_static"] - want["ef_static"]).max() <= 1e-11 * scale


def test_minimum_image_is_the_oracles_bit_for_bit():
    """rint() image, r and rimg of every pair of a sheared box equal the oracle's own minimum_image()."""
    import ctypes as C
    s = sheared_es_432()
    lib = oracle.lib()
    vol, rb, rc = pr.pbc(s["basis"])
    b = np.ascontiguousarray(s["basis"], dtype=np.float64)
    rbc = np.ascontiguousarray(rb)
    rng = np.random.default_rng(0)
    I, J = rng.integers(0, 432, size=(2, 500))
    _, r, rimg, dimg = pr.minimum_image(s["basis"], rb, s["pos"][I] - s["pos"][J])
    for k in range(len(I)):
        ro, rio, di = C.c_double(), C.c_double(), (C.c_double * 3)()
        pi, pj = np.ascontiguousarray(s["pos"][I[k]]), np.ascontiguousarray(s["pos"][J[k]])
        lib.orc_minimum_image(b.ctypes.data_as(C.c_void_p), rbc.ctypes.data_as(C.c_void_p), pi.ctypes.data_as(C.c_void_p),
                              pj.ctypes.data_as(C.c_void_p), C.byref(ro), C.byref(rio), di)
        assert (ro.value, rio.value, tuple(di)) == (r[k], rimg[k], tuple(dimg[k]))
