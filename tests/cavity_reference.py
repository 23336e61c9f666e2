"""Independent numpy restatement of the cavity grid of cavity_bias (reference src/mc/cavity.c:17-179, the biased insertion
of src/mc/mc_moves.c:585-608), in float64 with the reference's operation order.  numpy neither contracts a * b + c into an
FMA nor reorders a sum written out operation by operation, and its sqrt is correctly rounded, so every function here
decides as the reference's C does."""
import numpy as np


def grid_points(basis, G):
    """[G^3, 3] positions, flat index g = (i G + j) G + k (k fastest):
    pos[p] = ((b[0][p] c0 + b[1][p] c1) + b[2][p] c2) - 0.5 b[0][p] - 0.5 b[1][p] - 0.5 b[2][p], left to right."""
    b = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    frac = (np.arange(G, dtype=np.float64) + 1.0) / np.float64(G + 1)
    c0, c1, c2 = [a.reshape(-1) for a in np.meshgrid(frac, frac, frac, indexing="ij")]
    pos = np.empty((G ** 3, 3))
    for p in range(3):
        t = b[0, p] * c0
        t = t + b[1, p] * c1
        t = t + b[2, p] * c2
        t = t - 0.5 * b[0, p]
        t = t - 0.5 * b[1, p]
        t = t - 0.5 * b[2, p]
        pos[:, p] = t
    return pos


def dist2(a, b):
    """((ax - bx)^2 + (ay - by)^2) + (az - bz)^2 with broadcasting over the leading axes."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    s = d[..., 0] * d[..., 0]
    s = s + d[..., 1] * d[..., 1]
    s = s + d[..., 2] * d[..., 2]
    return s


def within(a, b, radius):
    """The reference's test itself: sqrt(s) < radius."""
    return np.sqrt(dist2(a, b)) < np.float64(radius)


def threshold(radius):
    """The smallest double T with sqrt(T) >= radius: sqrt(s) < radius  <=>  s < T."""
    r = np.float64(radius)
    t = r * r
    while np.sqrt(t) < r:
        t = np.nextafter(t, np.inf)
    while True:
        below = np.nextafter(t, 0.0)
        if below == t or np.sqrt(below) < r:
            return t
        t = below


def occupancy(points, atoms, radius):
    """occ[g] = number of atoms within the radius of point g (no minimum image)."""
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    occ = np.zeros(len(points), dtype=np.int32)
    for lo in range(0, len(atoms), 128):
        occ += within(points[:, None, :], atoms[None, lo:lo + 128, :], radius).sum(axis=1).astype(np.int32)
    return occ


def open_list(occ):
    """Flat indices of the open points (occupancy 0), ascending = the reference's (i, j, k) scan order."""
    return np.flatnonzero(np.asarray(occ) == 0).astype(np.int32)


def dart_positions(basis, u):
    """u [n, 3] uniform draws -> positions: f = -0.5 + u, x[p] = (b[0][p] f0 + b[1][p] f1) + b[2][p] f2."""
    b = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    f = -0.5 + np.asarray(u, dtype=np.float64).reshape(-1, 3)
    x = np.empty_like(f)
    for p in range(3):
        t = b[0, p] * f[:, 0]
        t = t + b[1, p] * f[:, 1]
        t = t + b[2, p] * f[:, 2]
        x[:, p] = t
    return x


def dart_hits(points, opened, darts, radius):
    """How many darts lie within the radius of some open point."""
    darts = np.asarray(darts, dtype=np.float64).reshape(-1, 3)
    if len(opened) == 0 or len(darts) == 0:
        return 0
    hit = np.zeros(len(darts), dtype=bool)
    op = points[opened]
    for lo in range(0, len(op), 256):
        hit |= within(darts[:, None, :], op[None, lo:lo + 256, :], radius).any(axis=1)
    return int(hit.sum())


def reciprocal_basis(basis):
    """The matrix inverse as pbc() forms it (reference src/energy/pbc.c:47-63), and the volume."""
    b = np.asarray(basis, dtype=np.float64).reshape(3, 3)
    vol = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1])
    vol += b[0][1] * (b[1][2] * b[2][0] - b[1][0] * b[2][2])
    vol += b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0])
    iv = 1.0 / vol
    rb = np.empty((3, 3))
    rb[0][0] = iv * (b[1][1] * b[2][2] - b[1][2] * b[2][1])
    rb[0][1] = iv * (b[0][2] * b[2][1] - b[0][1] * b[2][2])
    rb[0][2] = iv * (b[0][1] * b[1][2] - b[0][2] * b[1][1])
    rb[1][0] = iv * (b[1][2] * b[2][0] - b[1][0] * b[2][2])
    rb[1][1] = iv * (b[0][0] * b[2][2] - b[0][2] * b[2][0])
    rb[1][2] = iv * (b[0][2] * b[1][0] - b[0][0] * b[1][2])
    rb[2][0] = iv * (b[1][0] * b[2][1] - b[1][1] * b[2][0])
    rb[2][1] = iv * (b[0][1] * b[2][0] - b[0][0] * b[2][1])
    rb[2][2] = iv * (b[0][0] * b[1][1] - b[0][1] * b[1][0])
    return rb, vol


def wrapped_positions(system):
    """wrapped_pos of every atom as update_com() + wrapall() leave it (pairs.c:364-385, output.c:142-183): a frozen
    molecule is not wrapped, every other one is shifted by the lattice vector of rint(reciprocal . com).  `system` is a
    dict of arrays (pos, mass, molecule, frozen, basis); a molecule is a contiguous run of equal ids."""
    pos = np.asarray(system["pos"], dtype=np.float64)
    mass = np.asarray(system["mass"], dtype=np.float64)
    mol = np.asarray(system["molecule"])
    frozen = np.asarray(system["frozen"])
    b = np.asarray(system["basis"], dtype=np.float64).reshape(3, 3)
    rb, _ = reciprocal_basis(b)
    out = pos.copy()
    lo = 0
    while lo < len(pos):
        hi = lo
        while hi < len(pos) and mol[hi] == mol[lo]:
            hi += 1
        if not frozen[lo]:
            com = np.zeros(3)
            total = 0.0
            for a in range(lo, hi):
                total += mass[a]
                for i in range(3):
                    com[i] += mass[a] * pos[a, i]
            for i in range(3):
                com[i] /= total
            d = np.zeros(3)
            for i in range(3):
                for j in range(3):
                    d[i] += rb[j][i] * com[j]
                d[i] = np.rint(d[i])
            for i in range(3):
                dimg = 0.0
                for j in range(3):
                    dimg += b[j][i] * d[j]
                out[lo:hi, i] = pos[lo:hi, i] - dimg
        lo = hi
    return out


def cavity_volume(hits, n_darts, volume):
    """(hits / n) * volume in doubles (cavity.c:83)."""
    return (np.float64(hits) / np.float64(n_darts)) * np.float64(volume)


def random_index(n_open, u):
    """(open - 1) - (int) rint((open - 1) u) (mc_moves.c:589); rint rounds ties to even, as numpy's does."""
    return int((n_open - 1) - int(np.rint(np.float64(n_open - 1) * np.float64(u))))
