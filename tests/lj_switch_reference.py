"""numpy fp64 reference of what a Lennard-Jones switching function CHANGES (tests/test_lj_switch_cpu.py, tests/test_gpu_lj_switch.py).

Independent of the engine and of the oracle: it knows the pair classes the engine documents (include/blues_engine.h:
BluesSystemExtV4) and nothing of its code.  With rs the switch distance, rc the cutoff, x = (r - rs) / (rc - rs) clamped to [0, 1] and
    S = 1 - 10 x^3 + 15 x^4 - 6 x^5,
a switched System differs from the unswitched one by  dE = sum U(r) (S(r) - 1)  over the non-excluded minimum-image pairs with
rs < r < rc, where U is
  * 4 eps ((sigma / r)^12 - (sigma / r)^6) between two non-alchemical atoms (sigma arithmetic, eps geometric mean),
  * the softcore form  ls 4 eps x (x - 1), x = 1 / (alpha (1 - ls) + (r / sigma)^6)  between an alchemical and a non-alchemical atom,
  * between two alchemical atoms the softcore form with annihilate_sterics, the plain 12-6 form without,
and by the shell integral of the dispersion correction.  Coulomb, exceptions (excluded pairs), the mesh and bonded terms do not change.

Pairs are found by binning the atoms into cells of at least the cutoff (boxes of three or more cells per edge: the S23k box) or by
chunked rows (smaller boxes): 23,400 atoms take about two seconds."""
import numpy as np


def switch(r, rs, rc):
    """S(r) and dS/dr."""
    r = np.asarray(r, dtype=np.float64)
    x = np.clip((r - rs) / (rc - rs), 0.0, 1.0)
    return 1.0 - 10.0 * x ** 3 + 15.0 * x ** 4 - 6.0 * x ** 5, -30.0 * x ** 2 * (1.0 - x) ** 2 / (rc - rs)


def plain_lj(r, sigma, eps):
    """U and dU/dr of 4 eps ((sigma / r)^12 - (sigma / r)^6)."""
    s6 = (sigma / r) ** 6
    return 4.0 * eps * (s6 * s6 - s6), 4.0 * eps * (-12.0 * s6 * s6 + 6.0 * s6) / r


def softcore_lj(r, sigma, eps, ls, alpha):
    """U and dU/dr of ls 4 eps x (x - 1), x = 1 / (alpha (1 - ls) + (r / sigma)^6); 0 where eps or sigma is 0."""
    ok = (eps != 0.0) & (sigma != 0.0)
    sg = np.where(ok, sigma, 1.0)
    q6 = (r / sg) ** 6
    x = 1.0 / (alpha * (1.0 - ls) + q6)
    u = ls * 4.0 * eps * x * (x - 1.0)
    du = ls * 4.0 * eps * (2.0 * x - 1.0) * (-x * x * 6.0 * q6 / r)
    return np.where(ok, u, 0.0), np.where(ok, du, 0.0)


def _pairs_rows(x, box, rc, chunk=512):
    n = len(x)
    out_i, out_j = [], []
    for a in range(0, n, chunk):
        d = x[a:a + chunk, None, :] - x[None, :, :]
        d -= box * np.rint(d / box)
        r2 = (d * d).sum(-1)
        i, j = np.nonzero(r2 < rc * rc)
        i += a
        keep = i < j
        out_i.append(i[keep]); out_j.append(j[keep])
    return np.concatenate(out_i), np.concatenate(out_j)


def _pairs_cells(x, box, rc):
    nc = np.floor(box / rc).astype(np.int64)
    f = x / box
    f -= np.floor(f)
    c = np.minimum((f * nc).astype(np.int64), nc - 1)
    cid = (c[:, 0] * nc[1] + c[:, 1]) * nc[2] + c[:, 2]
    order = np.argsort(cid, kind="stable")
    start = np.searchsorted(cid[order], np.arange(nc.prod() + 1))
    half = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) > (0, 0, 0)]
    out_i, out_j = [], []
    for cx in range(nc[0]):
        for cy in range(nc[1]):
            for cz in range(nc[2]):
                a = order[start[(cx * nc[1] + cy) * nc[2] + cz]:start[(cx * nc[1] + cy) * nc[2] + cz + 1]]
                if len(a) == 0:
                    continue
                for off in [(0, 0, 0)] + half:
                    k = (((cx + off[0]) % nc[0]) * nc[1] + (cy + off[1]) % nc[1]) * nc[2] + (cz + off[2]) % nc[2]
                    b = order[start[k]:start[k + 1]]
                    if len(b) == 0:
                        continue
                    d = x[a][:, None, :] - x[b][None, :, :]
                    d -= box * np.rint(d / box)
                    i, j = np.nonzero((d * d).sum(-1) < rc * rc)
                    i, j = a[i], b[j]
                    if off == (0, 0, 0):
                        keep = i < j
                        i, j = i[keep], j[keep]
                    out_i.append(np.minimum(i, j)); out_j.append(np.maximum(i, j))
    return np.concatenate(out_i), np.concatenate(out_j)


def pairs_within(positions, box, rc):
    """(i, j), i < j: every pair whose minimum-image distance is below rc, once."""
    x = np.asarray(positions, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(-1)[:3]
    assert rc <= 0.5 * box.min()
    if np.all(np.floor(box / rc) >= 3):
        return _pairs_cells(x, box, rc)
    return _pairs_rows(x, box, rc)


def delta(system, positions, lambda_sterics, switch_distance=None):
    """What the switch changes at `positions`: {"dE_env": ..., "dE_alch": ..., "dE": their sum, "dF": (n, 3), "pairs": pairs in the
    shell}.  dE_env belongs to energy term [3] (pairs of two non-alchemical atoms), dE_alch to term [5] (pairs with an alchemical atom)."""
    rs = float(system.switch_distance if switch_distance is None else switch_distance)
    rc = float(system.cutoff)
    assert 0.0 < rs < rc
    x = np.asarray(positions, dtype=np.float64)
    box = np.asarray(system.box, dtype=np.float64).reshape(-1)[:3]
    n = system.n_atoms
    i, j = pairs_within(x, box, rc)
    d = x[i] - x[j]
    d -= box * np.rint(d / box)
    r = np.sqrt((d * d).sum(-1))
    shell = r > rs
    ex = np.concatenate([np.asarray(system.exclusions, dtype=np.int64).reshape(-1, 2), np.asarray(system.exception_atoms, dtype=np.int64).reshape(-1, 2)])
    shell &= ~np.isin(i * n + j, np.minimum(ex[:, 0], ex[:, 1]) * n + np.maximum(ex[:, 0], ex[:, 1]))
    i, j, d, r = i[shell], j[shell], d[shell], r[shell]
    sig = 0.5 * (np.asarray(system.sigma, dtype=np.float64)[i] + np.asarray(system.sigma, dtype=np.float64)[j])
    eps = np.sqrt(np.asarray(system.epsilon, dtype=np.float64)[i] * np.asarray(system.epsilon, dtype=np.float64)[j])
    alch = np.zeros(n, bool); alch[np.asarray(system.alchemical_atoms, dtype=np.int64).reshape(-1)] = True
    n_alch = alch[i].astype(int) + alch[j].astype(int)
    soft = (n_alch == 1) | ((n_alch == 2) & bool(system.annihilate_sterics))
    up, dup = plain_lj(r, sig, eps)
    us, dus = softcore_lj(r, sig, eps, float(lambda_sterics), float(system.softcore_alpha))
    u, du = np.where(soft, us, up), np.where(soft, dus, dup)
    S, dS = switch(r, rs, rc)
    e = u * (S - 1.0)
    dvdr = du * (S - 1.0) + u * dS
    fvec = (-dvdr / r)[:, None] * d          # force on i; minus that on j
    dF = np.zeros((n, 3))
    for k in range(3):
        dF[:, k] = np.bincount(i, fvec[:, k], n) - np.bincount(j, fvec[:, k], n)
    return {"dE_env": float(e[n_alch == 0].sum()), "dE_alch": float(e[n_alch > 0].sum()), "dE": float(e.sum()), "dF": dF, "pairs": int(len(r)),
            "atoms_in_shell": np.unique(np.concatenate([i, j]))}


def _adaptive_simpson(f, a, b, rel=1e-13):
    """Adaptive Simpson with Richardson's correction; the subdivision stops where a panel's estimate moves by less than rel of the whole."""
    fa, fm, fb = f(a), f(0.5 * (a + b)), f(b)
    whole = (b - a) / 6.0 * (fa + 4.0 * fm + fb)
    scale = [abs(whole)]

    def rec(a, fa, m, fm, b, fb, s, depth):
        lm, rm = 0.5 * (a + m), 0.5 * (m + b)
        flm, frm = f(lm), f(rm)
        left, right = (m - a) / 6.0 * (fa + 4.0 * flm + fm), (b - m) / 6.0 * (fm + 4.0 * frm + fb)
        if depth > 40 or abs(left + right - s) <= 15.0 * rel * scale[0] * (b - a):
            return left + right + (left + right - s) / 15.0
        return rec(a, fa, lm, flm, m, fm, left, depth + 1) + rec(m, fm, rm, frm, b, fb, right, depth + 1)
    first = rec(a, fa, 0.5 * (a + b), fm, b, fb, whole, 0)
    scale[0] = abs(first) / (b - a)          # (second pass with the integral's own size as the scale)
    return rec(a, fa, 0.5 * (a + b), fm, b, fb, whole, 0)


def dispersion_correction(system, zero_epsilon=()):
    """The long-range dispersion correction with the switching function: (2 pi N^2 / V) <int_rs^inf r^2 U(r) (1 - S(r)) dr>, the average
    over all pairs i <= j (OpenMM's count) by (sigma, epsilon) class, S = 0 beyond the cutoff; the shell part by adaptive quadrature of
    r^2 U (1 - S) class by class is the same as sigma^12 I12 - sigma^6 I6 with two quadratures, which is what is done."""
    rs, rc = float(system.switch_distance), float(system.cutoff)
    n = system.n_atoms
    eps = np.array(system.epsilon, dtype=np.float64); eps[np.asarray(zero_epsilon, dtype=np.int64)] = 0.0
    sig = np.asarray(system.sigma, dtype=np.float64)
    count = {}
    for s_, e_ in zip(sig.tolist(), eps.tolist()):
        count[(s_, e_)] = count.get((s_, e_), 0) + 1
    keys = sorted(count)
    i12 = i6 = 0.0
    if 0.0 < rs < rc:
        one_minus_s = lambda r: 1.0 - float(switch(r, rs, rc)[0])
        i12 = _adaptive_simpson(lambda r: one_minus_s(r) / r ** 10, rs, rc)
        i6 = _adaptive_simpson(lambda r: one_minus_s(r) / r ** 4, rs, rc)
    total = 0.0
    for a, (sa, ea) in enumerate(keys):
        for sb, eb in keys[a:]:
            pairs = 0.5 * count[(sa, ea)] * (count[(sa, ea)] + 1.0) if (sa, ea) == (sb, eb) else float(count[(sa, ea)]) * count[(sb, eb)]
            sg6 = (0.5 * (sa + sb)) ** 6
            # int_rs^inf r^2 4 eps (sg^12 / r^12 - sg^6 / r^6) (1 - S) dr, S = 0 beyond rc
            total += pairs * 4.0 * np.sqrt(ea * eb) * (sg6 * sg6 * (i12 + 1.0 / (9.0 * rc ** 9)) - sg6 * (i6 + 1.0 / (3.0 * rc ** 3)))
    V = float(np.prod(np.asarray(system.box, dtype=np.float64).reshape(-1)[:3]))
    return 2.0 * np.pi * n * float(n) / V * total / (0.5 * n * (n + 1.0))
