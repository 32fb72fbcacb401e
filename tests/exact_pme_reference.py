"""fp64 reference of the 'exact' alchemical PME treatment, composed from three evaluations of the unchanged CPU oracle:

    U_exact(x; ls, le) = U[A0](x; ls, .) + U[M(le)](x) - U[M(0)](x)          (the same for the forces and for the ten terms)

A0   = the alchemical System under 'direct-space' with the alchemical atoms' charges set to 0 and the chargeProd of every exception
       that holds an alchemical atom set to 0: sterics (softcore by lambda_sterics), bonded terms and the environment's electrostatics.
M(c) = the same System with `alchemical_atoms` empty, the alchemical atoms' charges multiplied by c and those exceptions' chargeProd
       multiplied by c: a plain System whose every electrostatic term -- direct space, reciprocal space, self term, background,
       excluded-pair corrections -- uses q~ = c q.  M(le) - M(0) is what the alchemical charges add; its Lennard-Jones, bonded and
       dispersion parts cancel.  Exceptions are linear in c (as the exact treatment scales them), everything else in q~ is quadratic.

The composition files the ligand's electrostatics under the plain terms ([3], [4], [8]), so terms are compared in groups:
[0] [1] [2] [7] [9] each, [5], the sum [3] + [4] + [6], [8], and the total (`GROUPS`).
"""
import copy

import numpy as np

from blues_amd import integrators
from oracle import oracle

GROUPS = ((0,), (1,), (2,), (7,), (9,), (5,), (3, 4, 6), (8,))


def group_terms(terms):
    """The ten energy terms summed into the comparable groups (+ the total as the last entry)."""
    t = np.asarray(terms, dtype=np.float64)
    return np.array([t[list(g)].sum() for g in GROUPS] + [t.sum()])


def _with_scaled_alchemical_charges(system, c, keep_alchemical):
    s = copy.copy(system)
    s.alchemical_pme_treatment = "direct-space"     # (the oracle knows one treatment; the field does not reach it)
    lig = np.asarray(system.alchemical_atoms, dtype=np.int64).reshape(-1)
    is_lig = np.zeros(system.n_atoms, bool); is_lig[lig] = True
    s.charge = np.array(system.charge, dtype=np.float64, copy=True); s.charge[lig] *= c
    ea = np.asarray(system.exception_atoms, dtype=np.int64).reshape(-1, 2)
    s.exception_params = np.array(system.exception_params, dtype=np.float64, copy=True).reshape(-1, 3)
    if len(ea):
        s.exception_params[is_lig[ea[:, 0]] | is_lig[ea[:, 1]], 0] *= c
    if not keep_alchemical:
        s.alchemical_atoms = np.zeros((0,), np.int32)
    return s


class ExactPmeReference:
    """U_exact, its forces and terms for one System; the three oracle contexts are made once and re-positioned per evaluation.
    M(c) is re-made per distinct c (its charges are part of the oracle's System), cached."""

    def __init__(self, system, openmp=False):
        oracle.build()
        self.system, self._openmp = system, openmp
        self._data = integrators.generateNCMCIntegrator(nstepsNC=2, dt=0.002, temperature=300.0, seed=1).to_data(precision=1)
        self._a0 = oracle.Oracle(_with_scaled_alchemical_charges(system, 0.0, True), self._data, openmp=openmp)
        self._m = {}

    def _plain(self, c):
        c = float(c)
        if c not in self._m:
            self._m[c] = oracle.Oracle(_with_scaled_alchemical_charges(self.system, c, False), self._data, openmp=self._openmp)
        return self._m[c]

    def evaluate(self, x, ls, le, box=None):
        """(energy, forces [n][3], terms [10]) of the exact treatment at positions x."""
        parts = []
        for o, args, sign in ((self._a0, (ls, 1.0), 1.0), (self._plain(le), (1.0, 1.0), 1.0), (self._plain(0.0), (1.0, 1.0), -1.0)):
            if box is not None:
                o.set_box(box)
            o.set_positions(x)
            e, f, t = o.energy_forces(*args)
            parts.append((sign * e, sign * f, sign * t))
        return sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts)

    def energy(self, x, ls, le):
        return self.evaluate(x, ls, le)[0]

    def charge_coefficients(self, x):
        """(E1, E2) of U[M(le)](x) - U[M(0)](x) = le E1 + le^2 E2: what the alchemical charges add, from le = 0, 1/2, 1 (the composition is
        exactly quadratic: test_exact_pme_cpu.py).  With `sterics_part` the work of a switch needs six oracle evaluations per
        configuration instead of three per (configuration, lambda) pair."""
        u = []
        for c in (0.0, 0.5, 1.0):
            o = self._plain(c); o.set_positions(x)
            u.append(o.energy_forces(1.0, 1.0, forces=False)[0])
        e2 = 2.0 * (u[2] - 2.0 * u[1] + u[0])
        return (u[2] - u[0]) - e2, e2

    def sterics_part(self, x, ls):
        """U[A0](x; ls): everything that does not depend on lambda_electrostatics."""
        self._a0.set_positions(x)
        return self._a0.energy_forces(ls, 1.0, forces=False)[0]

    def coefficients(self, x, ls):
        """(E0, E1, E2) of U_exact(x; ls, le) = E0 + le E1 + le^2 E2, from le = 0, 1/2, 1."""
        u0, uh, u1 = (self.energy(x, ls, le) for le in (0.0, 0.5, 1.0))
        e2 = 2.0 * (u1 - 2.0 * uh + u0)
        return u0, (u1 - u0) - e2, e2
