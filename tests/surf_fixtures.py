"""Readers of tests/golden/surf/<name>/ (input, dimer.pqr, reference.out) and the longdouble model of the lines `ensemble
surf` prints for them, from tests/dimer_reference.py: every placement from the pristine frame, plain means.  Helper module
for tests/test_dimer_reference.py, tests/test_gpu_surf_host.py and tests/golden/make_surf_fixtures.py; it reads the files
with a parser of its own and shares nothing with the host layer."""
import functools
import os

import numpy as np

import dimer_reference as dr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surf")
E2REDUCED = 408.7816
ON_OFF = ("polarization", "polar_iterative", "polar_gs", "polar_gs_ranked", "polar_palmo", "surf_preserve", "surf_decomp",
          "surf_global_axis", "waldmanhagler", "halgren_mixing", "c6_mixing", "disp_expansion", "damp_dispersion",
          "extrapolate_disp_coeffs", "schmidt_mixing", "rd_only")
REAL = ("surf_min", "surf_max", "surf_inc", "surf_ang", "polar_damp", "polar_precision", "polar_gamma")


def names():
    return sorted(d for d in os.listdir(GOLD) if os.path.isdir(os.path.join(GOLD, d)))


def read_input(name):
    cfg = {}
    for line in open(os.path.join(GOLD, name, "input")):
        t = line.split()
        if not t or t[0][0] in "!#":
            continue
        if t[0] in ON_OFF:
            cfg[t[0]] = int(t[1] == "on")
        elif t[0] in REAL:
            cfg[t[0]] = float(t[1])
        elif t[0] == "polar_max_iter":
            cfg[t[0]] = int(t[1])
        elif t[0] == "surf_preserve_rotation":
            cfg[t[0]] = [float(x) for x in t[1:7]]
        else:
            cfg[t[0]] = t[1]
    return cfg


def read_pqr(name):
    mols = {}
    for line in open(os.path.join(GOLD, name, "dimer.pqr")):
        t = line.split()
        if not t or t[0] != "ATOM":
            continue
        v = [float(x) for x in t[6:]] + [0.0] * 13
        m = mols.setdefault(int(t[5]), {k: [] for k in ("pos", "mass", "charge", "alpha", "epsilon", "sigma", "c6", "c8", "c10")})
        m["pos"].append(v[0:3])
        for key, x in zip(("mass", "charge", "alpha", "epsilon", "sigma"), v[3:8]):
            m[key].append(x * E2REDUCED if key == "charge" else x)
        for key, x in zip(("c6", "c8", "c10"), v[10:13]):  # (v[8], v[9]: omega, gwp_alpha)
            m[key].append(x)
    out = [{k: np.array(v) for k, v in mols[i].items()} for i in sorted(mols)]
    assert len(out) == 2
    return out


def flags_of(cfg):
    f = {k: cfg[k] for k in ("polar_gs", "polar_gs_ranked", "polar_palmo", "waldmanhagler", "halgren_mixing", "c6_mixing",
                             "disp_expansion", "damp_dispersion", "extrapolate_disp_coeffs", "schmidt_mixing", "rd_only",
                             "polar_damp", "polar_precision", "polar_gamma", "polar_max_iter", "surf_global_axis") if k in cfg}
    if "polar_damp_type" in cfg:
        f["polar_damp_type"] = cfg["polar_damp_type"]
    f.setdefault("polar_max_iter", 10)
    return f


def molecules(name):
    """the two molecules as the scan sees them: polarizabilities only under `polarization on`, and in preserve mode after
    the one-off surf_preserve_rotation about each molecule's centre"""
    cfg = read_input(name)
    a, b = read_pqr(name)
    if not cfg.get("polarization"):
        a, b = dict(a, alpha=np.zeros(len(a["alpha"]))), dict(b, alpha=np.zeros(len(b["alpha"])))
    if cfg.get("surf_preserve") and "surf_preserve_rotation" in cfg:
        g = cfg["surf_preserve_rotation"]
        ga = bool(cfg.get("surf_global_axis"))
        a = dict(a, pos=dr.place(dr.body_frame(a), dr.rotation(*g[:3], global_axis=ga), 0.0))
        b = dict(b, pos=dr.place(dr.body_frame(b), dr.rotation(*g[3:], global_axis=ga), 0.0))
    return a, b


def grid_sizes(name):
    cfg = read_input(name)
    if cfg.get("surf_preserve"):
        return [1] * 6
    return [len(x) for x in dr.angle_lists(cfg["surf_ang"])]


def reference_lines(name):
    return [l.strip() for l in open(os.path.join(GOLD, name, "reference.out")) if l.strip()]


@functools.lru_cache(maxsize=None)
def model_values(name, first_only=False):
    """per separation (or for the first one only): (r, es, rd, polar) means in longdouble"""
    cfg = read_input(name)
    a, b = molecules(name)
    flags = flags_of(cfg)
    lists = [[0.0]] * 6 if cfg.get("surf_preserve") else dr.angle_lists(cfg["surf_ang"])
    rows = []
    for r in dr.scan_values(cfg["surf_min"], cfg["surf_max"], cfg["surf_inc"]):
        es, rd, pol = dr.grid_energies(a, b, r, lists, flags)
        rows.append((r,) + tuple(np.sum(x) / len(x) for x in (es, rd, pol)))
        if first_only:
            break
    return rows


def format_rows(name, rows):
    """the reference's lines (surface.c:276-283, :366-375) for (r, es, rd, polar) rows"""
    cfg = read_input(name)
    out = []
    for r, es, rd, pol in rows:
        if cfg.get("surf_decomp") and cfg.get("surf_preserve"):
            out.append("%.5f %.5f %.5f %.5f %.5f" % (r, es, rd, pol, 0.0))
        elif cfg.get("surf_decomp"):
            out.append("%.5f %.5f %.5f %.5f" % (r, es, rd, pol))
        else:
            out.append("%.5f %.5f" % (r, es + rd + pol))
    return out


def model_lines(name, first_only=False):
    return format_rows(name, model_values(name, first_only))


def compare_lines(want, got):
    """(values that differ by one unit of the last printed digit, values compared); anything further apart fails"""
    assert len(want) == len(got), (len(want), len(got))
    exits = total = 0
    for lw, lg in zip(want, got):
        tw, tg = lw.split(), lg.split()
        assert len(tw) == len(tg), (lw, lg)
        for w, g in zip(tw, tg):
            total += 1
            if w == g:
                continue
            assert abs(round(float(w) * 1e5) - round(float(g) * 1e5)) <= 1, (lw, lg)
            exits += 1
    return exits, total
