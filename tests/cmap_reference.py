"""Independent numpy / scipy reference of the CMAP torsion term (include/blues_engine.h: BluesSystemExt).

A map is n x n energies, E[i, j] at phi = 2 pi i / n, psi = 2 pi j / n.  With delta = 2 pi / n:
  d1[i, j]   derivative at knot i of the periodic C2 cubic spline through E[:, j]   (scipy's CubicSpline, bc_type='periodic'),
  d2[i, j]   the same along j,
  d12[i, j]  derivative at knot j of the periodic spline through d1[i, :],
and within patch (floor(phi / delta), floor(psi / delta)), both clamped to n - 1, the energy is the bicubic Hermite patch through
E, d1, d2, d12 at the four corners -- evaluated here in the Hermite BASIS (the engine stores 16 polynomial coefficients per patch).
Nothing in this file is shared with the engine."""
import numpy as np
from scipy.interpolate import CubicSpline

TWO_PI = 2.0 * np.pi


def _knot_derivatives(y, delta):
    """derivative at every knot of the periodic cubic spline through y[0..n) (axis 0), spacing delta"""
    n = y.shape[0]
    x = np.arange(n + 1) * delta
    cs = CubicSpline(x, np.concatenate([y, y[:1]], axis=0), axis=0, bc_type="periodic")
    return cs(x[:n], 1)


def tables(E):
    """(d1, d2, d12) of a map, per radian"""
    E = np.asarray(E, dtype=np.float64)
    delta = TWO_PI / E.shape[0]
    d1 = _knot_derivatives(E, delta)
    d2 = _knot_derivatives(E.T, delta).T
    d12 = _knot_derivatives(d1.T, delta).T
    return d1, d2, d12


def _basis(t):
    """Hermite basis and its derivative at t: columns value(0), value(1), slope(0), slope(1)"""
    t2, t3 = t * t, t * t * t
    h = np.stack([2 * t3 - 3 * t2 + 1, -2 * t3 + 3 * t2, t3 - 2 * t2 + t, t3 - t2], axis=-1)
    dh = np.stack([6 * t2 - 6 * t, -6 * t2 + 6 * t, 3 * t2 - 4 * t + 1, 3 * t2 - 2 * t], axis=-1)
    return h, dh


def evaluate(E, phi, psi, tab=None):
    """(energy, dE/dphi, dE/dpsi) at angles in [0, 2 pi] (arrays or scalars)"""
    E = np.asarray(E, dtype=np.float64)
    n = E.shape[0]
    delta = TWO_PI / n
    d1, d2, d12 = tables(E) if tab is None else tab
    phi, psi = np.atleast_1d(np.asarray(phi, dtype=np.float64)), np.atleast_1d(np.asarray(psi, dtype=np.float64))
    i = np.minimum(np.floor(phi / delta).astype(np.int64), n - 1)
    j = np.minimum(np.floor(psi / delta).astype(np.int64), n - 1)
    t, u = phi / delta - i, psi / delta - j
    ht, dht = _basis(t)
    hu, dhu = _basis(u)
    scale = np.array([1.0, 1.0, delta, delta])
    ht, dht, hu, dhu = ht * scale, dht * scale, hu * scale, dhu * scale
    i1, j1 = (i + 1) % n, (j + 1) % n
    # G[..., a, b]: a over (f(i), f(i+1), d/dphi(i), d/dphi(i+1)), b the same along psi
    G = np.empty(phi.shape + (4, 4))
    for a, (ii, fa) in enumerate(((i, 0), (i1, 0), (i, 1), (i1, 1))):
        for b, (jj, fb) in enumerate(((j, 0), (j1, 0), (j, 1), (j1, 1))):
            G[..., a, b] = ((E, d2), (d1, d12))[fa][fb][ii, jj]
    e = np.einsum("...a,...ab,...b->...", ht, G, hu)
    ep = np.einsum("...a,...ab,...b->...", dht, G, hu) / delta
    es = np.einsum("...a,...ab,...b->...", ht, G, dhu) / delta
    return e, ep, es


def _min_image(d, box):
    return d if box is None else d - box * np.round(d / box)


def dihedral(x4, box=None):
    """(angle, d angle / d x (4, 3)) of four positions: the dihedral of a periodic torsion -- rij = x0 - x1, rkj = x2 - x1,
    rkl = x2 - x3, m = rij x rkj, n = rkj x rkl, cos = m.n / |m||n|, negative where rij.n < 0 -- taken through atan2 and shifted into
    [0, 2 pi) (a negative angle below half an ulp of 2 pi rounds to 2 pi itself)"""
    x4 = np.asarray(x4, dtype=np.float64)
    box = None if box is None else np.asarray(box, dtype=np.float64)
    rij, rkj, rkl = _min_image(x4[0] - x4[1], box), _min_image(x4[2] - x4[1], box), _min_image(x4[2] - x4[3], box)
    m, nn = np.cross(rij, rkj), np.cross(rkj, rkl)
    lkj = np.sqrt(rkj @ rkj)
    ang = np.arctan2(lkj * (rij @ nn), m @ nn)     # (that angle, conditioned well at 0 and pi too)
    if ang < 0.0:
        ang += TWO_PI
    g = np.zeros((4, 3))
    g[0] = lkj / (m @ m) * m
    g[3] = -lkj / (nn @ nn) * nn
    p, q = (rij @ rkj) / (lkj * lkj), (rkl @ rkj) / (lkj * lkj)
    sv = p * g[0] - q * g[3]
    g[1] = -g[0] + sv
    g[2] = -g[3] - sv
    return ang, g


def angles(torsions, x, box=None):
    """(m, 2) phi, psi of every torsion row (map, a1..a4, b1..b4)"""
    t = np.asarray(torsions).reshape(-1, 9)
    x = np.asarray(x, dtype=np.float64)
    return np.array([[dihedral(x[r[1:5]], box)[0], dihedral(x[r[5:9]], box)[0]] for r in t]).reshape(-1, 2)


def energy_forces(maps, torsions, x, box=None, tabs=None):
    """total CMAP energy and the (n, 3) forces of a configuration"""
    x = np.asarray(x, dtype=np.float64)
    F = np.zeros_like(x)
    e_tot = 0.0
    for r in np.asarray(torsions).reshape(-1, 9):
        mp = int(r[0])
        phi, gphi = dihedral(x[r[1:5]], box)
        psi, gpsi = dihedral(x[r[5:9]], box)
        e, ep, es = evaluate(maps[mp], phi, psi, None if tabs is None else tabs[mp])
        e_tot += float(e[0])
        np.add.at(F, r[1:5], -ep[0] * gphi)
        np.add.at(F, r[5:9], -es[0] * gpsi)
    return e_tot, F
