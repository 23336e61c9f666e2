"""The random draws behind a reference chain, replayed from its input and its energy file alone (a plain helper module).

The reference program draws from std::mt19937 seeded with `preset_seeds`, two 32-bit words per number
(libstdc++'s generate_canonical<double, 53>: (w0 + w1 2^32) / 2^64).  How many numbers a step takes depends only on the
kind of its move, and the kind only on the draws and on N, which the energy file has for every step under `corrtime 1`:

  checkpoint   uvt: one draw against insert_probability and, below it, one for insert (< 0.5) or remove; npt: one draw
               against volume_probability (not set: 1 / N); then, in every ensemble, one draw for the molecule.  A removal
               drawn while one movable molecule is left becomes a displacement.
  the move     displace: 6 (translate) + 4 (rotate); insert: 3 (position) + 4 (rotate); remove: 0; volume: 1
  Metropolis   1

So the file tells, per step, the kind of move, the Metropolis draw u, and -- for every ACCEPTED move, where the energies
before and after are both in the file -- the acceptance factor the reference must have compared u with.  That is what
tests/test_reference_chains.py asserts the fixtures' seeds were chosen for: steps at which a term of the factor decides.
No cavity_bias here (its grid takes draws of its own).
"""
import math
from decimal import Decimal

ATM2REDUCED = 0.0073389366


class MT19937:
    def __init__(self, seed):
        self.mt = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            self.mt.append((1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xFFFFFFFF)
        self.index = 624

    def word(self):
        mt = self.mt
        if self.index >= 624:
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.index = 0
        y = mt[self.index]
        self.index += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y

    def rand(self):
        w0, w1 = self.word(), self.word()
        return (float(w0) + float(w1) * 4294967296.0) / 18446744073709551616.0


DRAWS = dict(displace=10, insert=7, remove=0, volume=1)


def replay(kw, rows):
    """kw: the input's keywords (name -> list of values); rows: the data lines of the energy file as lists of strings.
    Returns one dict per step: kind, drawn (the kind checkpoint() drew: `remove` where it became a displacement), u, accepted,
    N_before, N_after, dE, V_before, V_after.  Raises AssertionError where the file cannot be the chain of these draws."""
    assert int(kw["corrtime"][0]) == 1 and kw.get("cavity_bias", ["off"])[0] == "off"
    ensemble = kw["ensemble"][0]
    rng = MT19937(int(kw["preset_seeds"][0]))
    p_insert = float(kw.get("insert_probability", ["0"])[0])
    p_volume = float(kw.get("volume_probability", ["0"])[0])

    def checkpoint(n):
        kind = "displace"
        if ensemble == "uvt":
            if rng.rand() < p_insert:
                kind = "insert" if rng.rand() < 0.5 else "remove"
        elif ensemble == "npt":
            if rng.rand() < (p_volume if p_volume != 0.0 else 1.0 / n):
                kind = "volume"
        rng.rand()  # the molecule
        return kind

    steps = []
    drawn = checkpoint(float(rows[0][8]))
    for before, after in zip(rows, rows[1:]):
        nb, na = int(Decimal(before[8])), int(Decimal(after[8]))
        kind = "displace" if (drawn == "remove" and nb == 1) else drawn
        for _ in range(DRAWS[kind]):
            rng.rand()
        u = rng.rand()
        changed = (before[1] != after[1]) or (before[8] != after[8]) or (before[10] != after[10])
        assert na - nb == ({"insert": 1, "remove": -1}.get(kind, 0) if changed else 0), (after[0], kind, nb, na)
        if kind != "volume":
            assert before[10] == after[10], (after[0], kind)
        steps.append(dict(step=int(after[0]), kind=kind, drawn=drawn, u=u, accepted=changed, N_before=nb, N_after=na,
                          dE=float(Decimal(after[1]) - Decimal(before[1])), V_before=float(before[10]),
                          V_after=float(after[10])))
        drawn = checkpoint(float(na))
    return steps


def factor(kw, s, n_shift=0, pv=1.0):
    """The acceptance factor of an accepted step as boltzmann_factor() of the reference forms it (mc.c:37-135), with the
    molecule count of its prefactor shifted by n_shift: 0 is the reference's rule; -1 is insertion over N, removal with
    N, the volume move's log term with N in place of N + 1.  pv scales the volume move's P dV term."""
    T = float(kw["temperature"][0])
    bf = math.exp(-s["dE"] / T)
    if s["kind"] == "insert":
        f = float(kw["user_fugacities"][0])
        return s["V_after"] * f * ATM2REDUCED / (T * (s["N_after"] + n_shift)) * bf
    if s["kind"] == "remove":
        f = float(kw["user_fugacities"][0])
        return T * (s["N_after"] + 1.0 + n_shift) / (s["V_after"] * f * ATM2REDUCED) * bf
    if s["kind"] == "volume":
        P = float(kw["pressure"][0])
        return math.exp(-(s["dE"] + pv * P * ATM2REDUCED * (s["V_after"] - s["V_before"]) -
                          (s["N_after"] + 1 + n_shift) * T * math.log(s["V_after"] / s["V_before"])) / T)
    return bf
