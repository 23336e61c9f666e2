"""The inputs of the Axilrod-Teller GPU tests (tests/test_gpu_at.py) and their reference values, shared with the CPU
test that checks the condition these inputs have to meet (tests/test_at_reference.py).

The condition: the smallest non-zero |term| of a case is at least 100 tolerances (tolerance = 1e-12 * sum |terms|), so
that one dropped or doubled triple fails the comparison.  A box in which every atom carries the term cannot meet it:
the terms fall off as r^-9 over the whole cell and the angular factor 1 - 3 cos cos cos passes through zero, so among
the 2.4e5 non-zero triples of synth.s_at(130) the smallest is 2.8e-12 of sum |terms| (4.4e-18 for s_at(320)).  The
cases therefore keep s_at's atoms, molecules and geometry but leave the term on a FEW sites -- about five per 64-atom
block -- and switch it off on all others in the two ways the term knows (even atom index: polarizability 0; odd:
polarizability kept, c9 = c6 = 0), which both give exact zeros.  The sites that keep it always include the first and the
last atom, the atoms on both sides of every block boundary (a two-site sorbate or the frozen framework molecule sits
across each), three atoms of the framework molecule (an all-on-one-molecule triple) and the last two atoms (the
partial block).  The remaining sites are drawn with the first seed, counting from 0, for which the condition holds with
a tenfold margin for c9 as read and under midzuno_kihara_approx; the rule looks at the reference values only.
"""
import functools

import numpy as np

import at_reference as ref
from mpmc_amd import synth

PER_BLOCK = 5
TOLERANCE = 1e-12   # of sum |terms|: the project's tolerance for a dense fp64 sum
MARGIN = 100.0      # smallest non-zero |term| >= MARGIN * TOLERANCE * sum |terms|
NAMES = ("n130", "n200", "n320", "n130_triclinic")
_SIZES = {"n130": 130, "n200": 200, "n320": 320, "n130_triclinic": 130}


def _restrict(base, active):
    out = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    n = len(out["alpha"])
    on = np.zeros(n, dtype=bool)
    on[list(active)] = True
    ms, qq, al, ep, sg, c6, c9 = synth.AT_ATOM
    for i in range(n):
        if on[i]:
            if out["alpha"][i] == 0.0 or out["c9"][i] == 0.0:  # one of s_at's own switched-off single atoms
                out["alpha"][i], out["c6"][i], out["c9"][i] = al, c6, c9
        elif i % 2 == 0:
            out["alpha"][i] = 0.0
        else:
            out["c6"][i] = 0.0
            out["c9"][i] = 0.0
    out["active"] = sorted(active)
    return out


def _subsystem(s, idx):
    idx = np.asarray(idx)
    return dict(pos=s["pos"][idx], alpha=s["alpha"][idx], molecule=s["molecule"][idx], c6=s["c6"][idx], c9=s["c9"][idx],
                basis=s["basis"])


def _forced(n):
    nfr = n // 3
    f = {0, nfr // 2, nfr - 1, n - 2, n - 1}
    for b in range(64, n, 64):
        f.update((b - 1, b))
    return f


@functools.lru_cache(maxsize=None)
def case(name):
    n = _SIZES[name]
    base = synth.s_at(n)
    if name.endswith("triclinic"):
        base = ref.triclinic(base)
    forced = _forced(n)
    nb = (n + 63) // 64
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        active = set(forced)
        for b in range(nb):
            lo, hi = 64 * b, min(64 * b + 64, n)
            have = sum(1 for a in active if lo <= a < hi)
            pool = [a for a in range(lo, hi) if a not in active]
            if have < PER_BLOCK and pool:
                active.update(rng.choice(pool, size=min(PER_BLOCK - have, len(pool)), replace=False).tolist())
        s = _restrict(base, active)
        sub = _subsystem(s, s["active"])  # every other site gives exact zeros
        ok = True
        for mk in (False, True):
            u = ref.unordered(sub, mk)
            ok = ok and u.min_nonzero >= 10.0 * MARGIN * TOLERANCE * u.sum_abs
        if ok:
            return s
    raise AssertionError("no site selection meets the condition for " + name)


@functools.lru_cache(maxsize=None)
def reference(name, mk=False):
    """(b) of at_reference on the whole case: computed once, shared by every test that needs it."""
    return ref.unordered(case(name), mk)


def without_term(s):
    return {k: v for k, v in s.items() if k != "active"}
