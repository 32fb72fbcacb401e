"""The device-resident minimiser's algorithm in numpy: FIRE (Bitzek et al., PRL 97, 170201) on the constraint
manifold.  TEST INFRASTRUCTURE ONLY: forces come from a callable (the CPU oracle in the tests), SHAKE and RATTLE are solved per
cluster of coupled constraints by Newton iteration on the multipliers to 1e-13, every number is fp64.

One pass k, at x_k: F = forces(x_k); G = F with its components along the constraints removed (a = w F, RATTLE on a, G = a / w);
fmax = max |G|, GG, VV, P = G.v over the mobile atoms; stop if fmax <= tolerance (converged) or k = max_iterations; adapt (k > 0);
kick v += dt w G; clip |v_i| dt <= max_step per atom; drift x += dt v, SHAKE against x_k, v += (x - x1) / dt, RATTLE.
"""
import numpy as np

DEFAULTS = dict(dt0=0.001, dt_max=0.01, n_min=5, f_inc=1.1, f_dec=0.5, alpha0=0.1, f_alpha=0.99, max_step=0.01)
SOLVE_TOL = 1e-13


class Constraints(object):
    """Distance constraints grouped into clusters of coupled ones.  w: inverse masses (0: frozen); constraints between two
    frozen atoms are dropped, as the engine drops them.  box: edge lengths of a periodic box (None: none): differences are
    taken to the nearest image."""

    def __init__(self, atoms, dist, w, box=None):
        atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, 2); dist = np.asarray(dist, dtype=np.float64).reshape(-1)
        self.w = np.asarray(w, dtype=np.float64)
        live = (self.w[atoms[:, 0]] > 0) | (self.w[atoms[:, 1]] > 0) if len(atoms) else np.zeros(0, bool)
        self.atoms, self.dist = atoms[live], dist[live]
        self.box = None if box is None or not np.all(np.asarray(box) > 0) else np.asarray(box, dtype=np.float64).reshape(3)
        parent = {}

        def find(a):
            while parent.setdefault(a, a) != a:
                parent[a] = parent[parent[a]]; a = parent[a]
            return a
        for i, j in self.atoms:
            parent[find(int(i))] = find(int(j))
        groups = {}
        for c, (i, j) in enumerate(self.atoms):
            groups.setdefault(find(int(i)), []).append(c)
        self.clusters = []
        for cons in groups.values():
            cons = np.array(cons); ci, cj = self.atoms[cons, 0], self.atoms[cons, 1]
            # coef[c, c2] = w_i(c) s(c2, i(c)) - w_j(c) s(c2, j(c)), s(c2, a) = +1 / -1 if a is the first / second atom of c2
            s_i = (ci[:, None] == ci[None, :]).astype(float) - (ci[:, None] == cj[None, :]).astype(float)
            s_j = (cj[:, None] == ci[None, :]).astype(float) - (cj[:, None] == cj[None, :]).astype(float)
            coef = self.w[ci][:, None] * s_i - self.w[cj][:, None] * s_j
            self.clusters.append((ci, cj, self.dist[cons] ** 2, coef))

    def diff(self, x, ci, cj):
        d = x[ci] - x[cj]
        if self.box is not None:
            d -= self.box * np.round(d / self.box)
        return d

    def shake(self, x, xref):
        """x moved onto the constraints along the bond directions of xref (in place; returns x)."""
        for ci, cj, d2, coef in self.clusters:
            r = self.diff(xref, ci, cj)
            for _ in range(100):
                D = self.diff(x, ci, cj)
                g = -((D * D).sum(1) - d2)
                if np.all(np.abs(g) <= SOLVE_TOL * d2):
                    break
                dl = np.linalg.solve(2.0 * (D @ r.T) * coef, g)
                np.add.at(x, ci, (dl * self.w[ci])[:, None] * r)
                np.add.at(x, cj, -(dl * self.w[cj])[:, None] * r)
            else:
                raise RuntimeError("SHAKE did not converge")
        return x

    def rattle(self, x, v):
        """v with its components along the constraints at x removed (in place; returns v).  Linear: one solve per cluster."""
        for ci, cj, d2, coef in self.clusters:
            r = self.diff(x, ci, cj)
            b = -((v[ci] - v[cj]) * r).sum(1)
            mu = np.linalg.solve((r @ r.T) * coef, b)
            np.add.at(v, ci, (mu * self.w[ci])[:, None] * r)
            np.add.at(v, cj, -(mu * self.w[cj])[:, None] * r)
        return v

    def project_force(self, x, F):
        """G: the force with its components along the constraints removed (0 on frozen atoms)."""
        a = self.rattle(x, self.w[:, None] * F)
        mobile = self.w > 0
        G = np.zeros_like(a)
        G[mobile] = a[mobile] / self.w[mobile][:, None]
        return G


def minimize(x, cons, forces, tolerance, max_iterations=0, **fire):
    """Returns (x, result, record): result as the engine's result record (without the energies); record[k] = dict(P, GG, VV, fmax,
    dt, alpha, n_pos, clip) of pass k -- dt, alpha, n_pos after the pass's adaptation, clip = min over the atoms of
    | |v_i| dt / max_step - 1 | (how close a clip decision was; inf when the pass did not move)."""
    p = dict(DEFAULTS); p.update(fire)
    max_iterations = int(max_iterations) if max_iterations else 10000
    w = cons.w; mobile = w > 0
    x = cons.shake(np.array(x, dtype=np.float64), np.array(x, dtype=np.float64))
    v = np.zeros_like(x)
    dt, alpha, n_pos, it, converged = p["dt0"], p["alpha0"], 0, 0, 0
    record = []
    while True:
        G = cons.project_force(x, forces(x))
        fmax = np.abs(G[mobile]).max() if mobile.any() else 0.0
        GG, VV, P = (G[mobile] ** 2).sum(), (v[mobile] ** 2).sum(), (G[mobile] * v[mobile]).sum()
        rec = dict(P=P, GG=GG, VV=VV, fmax=fmax, clip=np.inf)
        if fmax <= tolerance:
            converged = 1
        if converged or it >= max_iterations:
            rec.update(dt=dt, alpha=alpha, n_pos=n_pos); record.append(rec)
            break
        if it > 0:
            if P > 0.0:
                n_pos += 1
                a_old = alpha
                if n_pos > p["n_min"]:
                    dt = min(dt * p["f_inc"], p["dt_max"]); alpha *= p["f_alpha"]
                v = (1.0 - a_old) * v + a_old * np.sqrt(VV / GG) * G
            else:
                n_pos = 0; dt *= p["f_dec"]; alpha = p["alpha0"]; v = np.zeros_like(v)
        v = v + dt * G * w[:, None]
        ratio = np.sqrt((v * v).sum(1)) * dt / p["max_step"]
        rec["clip"] = np.abs(ratio[mobile] - 1.0).min()
        over = ratio > 1.0
        v[over] /= ratio[over][:, None]
        x1 = x + dt * v
        xn = cons.shake(x1.copy(), x)
        v = cons.rattle(xn, v + (xn - x1) / dt)
        x = xn
        it += 1
        rec.update(dt=dt, alpha=alpha, n_pos=n_pos); record.append(rec)
    result = dict(converged=converged, iterations=it, n_pos=n_pos, fmax=fmax, dt=dt, alpha=alpha)
    return x, result, record


def lj13(sigma=0.2, epsilon=0.3, jitter=0.01, seed=5):
    """The 13-atom Lennard-Jones cluster in vacuum: a centre atom and an icosahedron at the pair-minimum distance, perturbed; atom 0
    alchemical (at lambda = 1 it is an ordinary atom), no constraints."""
    from blues_amd._abi import NB_NOCUTOFF, SystemData
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    vert = np.array([(0, s1, s2 * phi) for s1 in (1, -1) for s2 in (1, -1)], dtype=np.float64)
    vert = np.concatenate([vert, vert[:, [1, 2, 0]], vert[:, [2, 0, 1]]])
    vert *= 2.0 ** (1.0 / 6.0) * sigma / np.sqrt(1.0 + phi * phi)
    x = np.concatenate([np.zeros((1, 3)), vert]) + 1.0
    x += jitter * np.random.RandomState(seed).uniform(-1.0, 1.0, x.shape)
    n = 13
    return SystemData(box=np.zeros(3), mass=np.full(n, 12.0), charge=np.zeros(n), sigma=np.full(n, sigma), epsilon=np.full(n, epsilon),
                      alchemical_atoms=np.arange(1, dtype=np.int32), nonbonded_method=NB_NOCUTOFF, cutoff=1.0, ewald_alpha=0.0,
                      dispersion_correction=False, remove_cm_motion=False, positions=x)


def kabsch_rmsd_max(a, b):
    """Largest atom displacement between a and b after the best rigid superposition of b onto a."""
    ca, cb = a.mean(0), b.mean(0)
    H = (b - cb).T @ (a - ca)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    Rm = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return np.sqrt((((b - cb) @ Rm.T - (a - ca)) ** 2).sum(1)).max()


def oracle_forces(oracle_obj, lambda_sterics=1.0, lambda_electrostatics=1.0):
    """forces(x) and energy(x) callables on a CPU oracle."""
    def forces(x):
        oracle_obj.set_positions(x)
        return oracle_obj.energy_forces(lambda_sterics, lambda_electrostatics)[1]

    def energy(x):
        oracle_obj.set_positions(x)
        return oracle_obj.energy_forces(lambda_sterics, lambda_electrostatics, forces=False)[0]
    return forces, energy
