"""Plain numpy fp64 reference of CHARMM's Urey-Bradley terms, harmonic impropers and of the 1-4 exception sum: energies and analytic
forces with the minimum image, for tests/test_charmm_cpu.py (which pins it by itself: forces against central differences, second
order) and tests/test_gpu_charmm.py.  No test of its own.

  Urey-Bradley  E = 0.5 k (r - r0)^2, r the minimum-image distance of the two atoms;
  improper      E = k d^2, d = psi - psi0 wrapped into (-pi, pi], psi the dihedral of atoms 1-2-3-4 with the vectors and sign rule of a
                periodic torsion, taken as atan2(|rkj| rij.n, m.n) with m = rij x rkj, n = rkj x rkl;
  1-4 sum       sum 4 eps ((sigma / r)^12 - (sigma / r)^6) + 138.935456 qq / r over the exception pairs."""
import numpy as np

ONE_4PI_EPS0 = 138.935456


def _mi(d, box):
    if box is None:
        return d
    box = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    return d - box * np.round(d / box)


def dihedral(x4, box=None):
    """psi in (-pi, pi] of four positions, and its gradient (4, 3)"""
    rij, rkj, rkl = _mi(x4[0] - x4[1], box), _mi(x4[2] - x4[1], box), _mi(x4[2] - x4[3], box)
    m, n = np.cross(rij, rkj), np.cross(rkj, rkl)
    lkj2 = rkj @ rkj
    lkj = np.sqrt(lkj2)
    psi = np.arctan2(lkj * (rij @ n), m @ n)
    gi, gl = lkj / (m @ m) * m, -lkj / (n @ n) * n          # d psi / d x_i, d psi / d x_l
    p, q = (rij @ rkj) / lkj2, (rkl @ rkj) / lkj2
    sv = p * gi - q * gl
    return psi, np.array([gi, -(gi - sv), -(gl + sv), gl])


def wrap(d):
    """into (-pi, pi]"""
    return d - 2.0 * np.pi if d > np.pi else (d + 2.0 * np.pi if d <= -np.pi else d)


def improper_angles(atoms, x, box=None):
    return np.array([dihedral(x[np.asarray(q)], box)[0] for q in np.asarray(atoms).reshape(-1, 4)])


def urey_bradley(atoms, params, x, box=None):
    """(energy, forces (n, 3))"""
    x = np.asarray(x, dtype=np.float64)
    e, f = 0.0, np.zeros_like(x)
    for (i, j), (r0, k) in zip(np.asarray(atoms).reshape(-1, 2), np.asarray(params, dtype=np.float64).reshape(-1, 2)):
        d = _mi(x[i] - x[j], box)
        r = np.sqrt(d @ d)
        e += 0.5 * k * (r - r0) ** 2
        g = k * (r - r0) / r * d
        f[i] -= g; f[j] += g
    return e, f


def impropers(atoms, params, x, box=None):
    """(energy, forces (n, 3))"""
    x = np.asarray(x, dtype=np.float64)
    e, f = 0.0, np.zeros_like(x)
    for q, (psi0, k) in zip(np.asarray(atoms).reshape(-1, 4), np.asarray(params, dtype=np.float64).reshape(-1, 2)):
        psi, grad = dihedral(x[q], box)
        d = wrap(psi - psi0)
        e += k * d * d
        for a in range(4):
            f[q[a]] -= 2.0 * k * d * grad[a]
    return e, f


def energy_forces(s, x, box=None):
    """both terms of a SystemData at x: (E Urey-Bradley, E improper, forces of both)"""
    eu, fu = urey_bradley(s.urey_bradley_atoms, s.urey_bradley_params, x, box)
    ei, fi = impropers(s.improper_atoms, s.improper_params, x, box)
    return eu, ei, fu + fi


def exceptions(atoms, params, x, box=None):
    """(energy, forces) of the 1-4 exception sum: params rows (qq, sigma, epsilon)"""
    x = np.asarray(x, dtype=np.float64)
    e, f = 0.0, np.zeros_like(x)
    for (i, j), (qq, sig, eps) in zip(np.asarray(atoms).reshape(-1, 2), np.asarray(params, dtype=np.float64).reshape(-1, 3)):
        d = _mi(x[i] - x[j], box)
        r2 = d @ d
        r = np.sqrt(r2)
        s6 = (sig * sig / r2) ** 3
        e += 4.0 * eps * (s6 * s6 - s6) + ONE_4PI_EPS0 * qq / r
        g = (4.0 * eps * (12.0 * s6 * s6 - 6.0 * s6) / r2 + ONE_4PI_EPS0 * qq / (r2 * r)) * d      # -dE/dx_i
        f[i] += g; f[j] -= g
    return e, f


def four_atoms(psi, b=0.15, theta=1.9):
    """four positions whose dihedral 0-1-2-3 is psi (up to rounding), built from bond length, bond angle and dihedral"""
    x = [b * np.array([np.cos(theta), np.sin(theta), 0.0]), np.zeros(3), np.array([b, 0.0, 0.0])]
    bc = np.array([1.0, 0.0, 0.0])
    nrm = np.cross(x[1] - x[0], bc); nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    x.append(x[2] - b * np.cos(theta) * bc + b * np.sin(theta) * np.cos(psi) * m + b * np.sin(theta) * np.sin(psi) * nrm)
    return np.array(x) + np.array([0.31, -0.12, 0.07])
