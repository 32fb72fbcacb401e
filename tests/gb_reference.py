"""numpy fp64 restatement of the GB-OBC implicit solvent (OpenMM's GBSAOBCForce with the ACE surface term), the reference of
tests/test_implicit_solvent_cpu.py and tests/test_gpu_implicit_solvent.py.  Units: nm, kJ/mol.

    o_i = rho_i - 0.009, s_i = S_i o_i
    I_i = o_i / 2 * sum_{j != i, o_i < r + s_j} term(r, o_i, s_j)
    B_i = 1 / (1/o_i - tanh(alpha I - beta I^2 + gamma I^3) / rho_i)
    E   = -K (1/eps_in - 1/eps_out) [ 1/2 sum_i q~_i^2 / B_i + sum_{i<j} q~_i q~_j / f_ij ] + sum_i c_i 4 pi sa (rho_i + 0.14)^2 (rho_i / B_i)^6

An alchemical atom carries q~ = lambda_electrostatics q and c = lambda_electrostatics, so E(le) = E0 + le E1 + le^2 E2; a pair belongs to
class a_i + a_j, a self term to class 2 a_i, a surface term to class a_i.  `coefficients` returns the three classes of the polar energy,
the surface energy and the force; `evaluate` combines them at one lambda.  It is pinned by itself (Born ion, a quadrature of the
descreening integral, far ions, central differences, vanishing net force and torque) in test_implicit_solvent_cpu.py."""
import numpy as np

ONE_4PI_EPS0 = 138.935456
OFFSET = 0.009
PROBE = 0.14
SURFACE_AREA_ENERGY = 2.25936
OBC = {1: (0.8, 0.0, 2.909125), 2: (1.0, 0.8, 4.85), "OBC1": (0.8, 0.0, 2.909125), "OBC2": (1.0, 0.8, 4.85)}


def descreening_term(r, o, s):
    """term(r, o_i, s_j), elementwise (0 where o_i >= r + s_j)."""
    r, o, s = np.broadcast_arrays(np.asarray(r, dtype=np.float64), np.asarray(o, dtype=np.float64), np.asarray(s, dtype=np.float64))
    U = r + s
    L = np.maximum(o, np.abs(r - s))
    with np.errstate(divide="ignore", invalid="ignore"):
        l, u = 1.0 / L, 1.0 / U
        t = l - u + 0.25 * r * (u * u - l * l) + 0.5 * np.log(u / l) / r + 0.25 * (s * s / r) * (l * l - u * u)
        t = np.where(o < s - r, t + 2.0 * (1.0 / o - l), t)
    return np.where(o < U, t, 0.0)


def descreening_slope(r, o, s):
    """d term / dr, elementwise: -2 t3, t3 = (1 + s^2/r^2)(l^2 - u^2)/8 + ln(u/l)/(4 r^2) (the parts through l and u cancel)."""
    r, o, s = np.broadcast_arrays(np.asarray(r, dtype=np.float64), np.asarray(o, dtype=np.float64), np.asarray(s, dtype=np.float64))
    U = r + s
    L = np.maximum(o, np.abs(r - s))
    with np.errstate(divide="ignore", invalid="ignore"):
        l, u = 1.0 / L, 1.0 / U
        t3 = 0.125 * (1.0 + s * s / (r * r)) * (l * l - u * u) + 0.25 * np.log(u / l) / (r * r)
    return np.where(o < U, -2.0 * t3, 0.0)


def _pairs(x):
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]                      # d[i, j] = x_i - x_j
    r = np.sqrt((d * d).sum(-1))
    np.fill_diagonal(r, 1.0)                               # (never used: the diagonal is masked out below)
    return d, r


def born_radii(x, radius, scale, model=2):
    """(I, B, dB/dI) per atom."""
    alpha, beta, gamma = OBC[model]
    rho = np.asarray(radius, dtype=np.float64); o = rho - OFFSET; s = np.asarray(scale, dtype=np.float64) * o
    _, r = _pairs(x)
    off = ~np.eye(len(rho), dtype=bool)
    T = np.where(off, descreening_term(r, o[:, None], s[None, :]), 0.0)
    I = 0.5 * o * T.sum(1)
    t = np.tanh(alpha * I - beta * I * I + gamma * I ** 3)
    B = 1.0 / (1.0 / o - t / rho)
    dB = B * B * (1.0 - t * t) * (alpha - 2.0 * beta * I + 3.0 * gamma * I * I) / rho
    return I, B, dB


def coefficients(x, charge, radius, scale, alchemical=(), model=2, solute_dielectric=1.0, solvent_dielectric=78.5,
                 surface_area_energy=SURFACE_AREA_ENERGY):
    """{'polar': (3,), 'surface': (3,), 'force': (3, n, 3), 'born': (n,)}: the coefficients of 1, le, le^2."""
    x = np.asarray(x, dtype=np.float64); n = len(x)
    q = np.asarray(charge, dtype=np.float64); rho = np.asarray(radius, dtype=np.float64)
    o = rho - OFFSET; s = np.asarray(scale, dtype=np.float64) * o
    a = np.zeros(n, dtype=np.int64); a[np.asarray(alchemical, dtype=np.int64)] = 1
    pref = ONE_4PI_EPS0 * (1.0 / solute_dielectric - 1.0 / solvent_dielectric)
    I, B, dB = born_radii(x, radius, scale, model)
    chain = dB * 0.5 * o                                    # dB_i / d(sum_j term_ij)
    d, r = _pairs(x)
    off = ~np.eye(n, dtype=bool)
    D = B[:, None] * B[None, :]
    ex = np.exp(-r * r / (4.0 * D))
    inv_f = 1.0 / np.sqrt(r * r + D * ex)
    qq = q[:, None] * q[None, :]
    cls = a[:, None] + a[None, :]
    esa = 4.0 * np.pi * surface_area_energy * (rho + PROBE) ** 2 * (rho / B) ** 6
    slope = np.where(off, descreening_slope(r, o[:, None], s[None, :]), 0.0)    # slope[i, j] = d term_ij / dr
    polar, surface, force = np.zeros(3), np.zeros(3), np.zeros((3, n, 3))
    for c in range(3):
        M = off & (cls == c)
        self_c = (2 * a == c)
        polar[c] = -pref * (0.5 * (qq * inv_f)[M].sum() + 0.5 * (q * q / B)[self_c].sum())
        surface[c] = esa[a == c].sum()
        dEdB = pref * np.where(M, 0.5 * qq * inv_f ** 3 * ex * (B[None, :] + r * r / (4.0 * B[:, None])), 0.0).sum(1)
        dEdB += np.where(self_c, 0.5 * pref * q * q / (B * B), 0.0) + np.where(a == c, -6.0 * esa / B, 0.0)
        direct = -pref * (np.where(M, qq * inv_f ** 3 * (1.0 - 0.25 * ex), 0.0)[:, :, None] * d).sum(1)
        G = dEdB * chain
        # dE/dx_i = sum_j (G_i slope_ij + G_j slope_ji) d_ij / r
        w = (G[:, None] * slope + G[None, :] * slope.T) / r
        force[c] = direct - (w[:, :, None] * d).sum(1)
    return {"polar": polar, "surface": surface, "force": force, "born": B, "integral": I}


def evaluate(coef, lambda_electrostatics=1.0):
    """(polar energy, surface energy, forces) at one lambda_electrostatics."""
    p = np.array([1.0, lambda_electrostatics, lambda_electrostatics ** 2])
    return float(coef["polar"] @ p), float(coef["surface"] @ p), np.tensordot(p, coef["force"], axes=1)


def system_coefficients(system, x=None):
    """`coefficients` for a SystemData that carries implicit_solvent."""
    gb = system.implicit_solvent
    return coefficients(system.positions if x is None else x, system.charge, gb.radius, gb.scale, np.asarray(system.alchemical_atoms).reshape(-1),
                        int(gb.model), gb.solute_dielectric, gb.solvent_dielectric, gb.surface_area_energy)
