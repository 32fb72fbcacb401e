"""Implicit solvent without a GPU: the numpy reference of the GB-OBC forms (tests/gb_reference.py) pinned by itself -- Born ion, the
descreening integral by quadrature, far ions, forces against central differences, vanishing net force and torque -- and the host side:
system_from_amber(implicit_solvent=...), the refusals, the ctypes mirror of BluesImplicitSolventDesc."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import gb_reference as gbr
from blues_amd import _abi, amber, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 138.935456


def amber_system(name, alchemical=(), **kw):
    prm = amber.read_prmtop(os.path.join(GOLDEN, name + ".prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, name + ".inpcrd"))
    return prm, amber.system_from_amber(prm, pos, box, constraints="HBonds", alchemical_atoms=alchemical, nonbonded_method="NoCutoff", **kw)


def random_cluster(n=12, seed=5):
    """n atoms on a jittered lattice of 0.17 nm (bonded-like contacts, overlapping and engulfing descreening spheres)."""
    rng = np.random.RandomState(seed)
    grid = np.array([(i, j, k) for i in range(3) for j in range(2) for k in range(2)], dtype=np.float64)[:n]
    x = 0.17 * grid + rng.uniform(-0.03, 0.03, (n, 3))
    q = rng.uniform(-0.8, 0.8, n)
    rho = rng.uniform(0.10, 0.20, n); rho[3] = 0.06; rho[4] = 0.3      # (a small atom beside a large one: the engulfed branch)
    S = rng.uniform(0.7, 0.95, n)
    return x, q, rho, S


@pytest.mark.parametrize("model", [1, 2])
def test_born_energy_of_one_ion(model):
    """One atom: I = 0, B = rho - 0.009, E = -K/2 (1/eps_in - 1/eps_out) q^2 / B + 4 pi sa (rho + 0.14)^2 (rho / B)^6, to rounding."""
    q, rho = -1.0, 0.17
    c = gbr.coefficients(np.zeros((1, 3)), [q], [rho], [0.8], model=model, solute_dielectric=2.0, solvent_dielectric=78.5)
    B = rho - 0.009
    assert c["born"][0] == pytest.approx(B, rel=1e-15)
    pol, sa, f = gbr.evaluate(c, 1.0)
    assert pol == pytest.approx(-0.5 * K * (1.0 / 2.0 - 1.0 / 78.5) * q * q / B, rel=1e-14)
    assert sa == pytest.approx(4.0 * np.pi * 2.25936 * (rho + 0.14) ** 2 * (rho / B) ** 6, rel=1e-14)
    assert np.all(f == 0.0)
    # alchemical: charge and surface term scaled by lambda
    c = gbr.coefficients(np.zeros((1, 3)), [q], [rho], [0.8], alchemical=[0], model=model)
    pol_h, sa_h, _ = gbr.evaluate(c, 0.5)
    pol_1, sa_1, _ = gbr.evaluate(c, 1.0)
    assert pol_h == pytest.approx(0.25 * pol_1, rel=1e-14) and sa_h == pytest.approx(0.5 * sa_1, rel=1e-14)


def _quadrature(r, o, s, n):
    """(1/4 pi) int dV / |x|^4 over the part of the sphere (radius s, centre at distance r) outside the sphere of radius o about the
    origin: shells of radius p about the origin, of which the fraction (1 - cos theta) / 2, cos theta = (p^2 + r^2 - s^2) / (2 p r),
    lies inside the far sphere (all of it for p < s - r); composite Simpson with n intervals per smooth piece."""
    def simpson(f, a, b):
        if b <= a:
            return 0.0
        p = np.linspace(a, b, n + 1)
        w = np.ones(n + 1); w[1:-1:2] = 4.0; w[2:-1:2] = 2.0
        return float((w * f(p)).sum() * (b - a) / (3.0 * n))
    total = simpson(lambda p: 1.0 / (p * p), o, s - r)                                   # engulfed shells (empty unless o < s - r)
    total += simpson(lambda p: 0.5 * (1.0 - (p * p + r * r - s * s) / (2.0 * p * r)) / (p * p), max(o, abs(r - s)), r + s)
    return total


@pytest.mark.parametrize("r,o,s,case", [(0.5, 0.15, 0.12, "separated"), (0.2, 0.15, 0.12, "overlapping"), (0.1, 0.051, 0.2619, "engulfed")])
def test_descreening_term_is_the_integral(r, o, s, case):
    """term / 2 = (1/4 pi) int dV / |x|^4 over j's scaled sphere outside i's.  The bar is the quadrature's own convergence: ten times the
    change from halving its step (Simpson: the finer value is about 16 times closer than that change), plus rounding."""
    assert {"separated": r - s >= o, "overlapping": abs(r - s) < o < r + s, "engulfed": o < s - r}[case]
    coarse, fine = _quadrature(r, o, s, 2000), _quadrature(r, o, s, 4000)
    bar = 10.0 * abs(fine - coarse) + 1e-13 * abs(fine)
    assert bar < 1e-9 * abs(fine)
    assert abs(0.5 * float(gbr.descreening_term(r, o, s)) - fine) <= bar, (case, 0.5 * float(gbr.descreening_term(r, o, s)), fine, bar)


def test_no_descreening_is_exactly_zero():
    assert float(gbr.descreening_term(0.05, 0.2, 0.1)) == 0.0 and float(gbr.descreening_term(0.1, 0.2, 0.1)) == 0.0     # o >= r + s
    assert float(gbr.descreening_slope(0.05, 0.2, 0.1)) == 0.0
    # leading term of the far series: term -> (2/3) s^3 / r^4
    assert float(gbr.descreening_term(50.0, 0.15, 0.1)) == pytest.approx(2.0 / 3.0 * 0.1 ** 3 / 50.0 ** 4, rel=1e-4)


def test_two_far_ions():
    """r >> B: f -> r, Born radii -> the lone ions'; E -> the two Born energies - K (1/eps_in - 1/eps_out) q1 q2 / r."""
    r = 200.0
    q, rho = np.array([1.0, -1.0]), np.array([0.15, 0.2])
    c = gbr.coefficients(np.array([[0.0, 0, 0], [r, 0, 0]]), q, rho, [0.8, 0.8], surface_area_energy=0.0)
    pref = K * (1.0 - 1.0 / 78.5)
    lone = -0.5 * pref * (q * q / (rho - 0.009)).sum()
    pol = gbr.evaluate(c, 1.0)[0]
    # (descreening at 200 nm changes B by ~ s^3 / r^4 ~ 1e-12 relative; exp(-r^2 / 4 B B) underflows: f = r exactly)
    assert pol - lone == pytest.approx(-pref * q[0] * q[1] / r, rel=1e-9)


def _central_differences(x, energy, atoms, h):
    f = np.zeros((len(atoms), 3))
    for n, a in enumerate(atoms):
        for k in range(3):
            xp = x.copy(); xp[a, k] += h
            xm = x.copy(); xm[a, k] -= h
            f[n, k] = -(energy(xp) - energy(xm)) / (2.0 * h)
    return f


def fd_bar(fmax, e_abs, h):
    """Central differences of E with step h: truncation h^2 |E'''| / 6 with |E'''| <= Fmax / l^2, l = 0.009 nm (the dielectric offset: the
    shortest length of the model, far below any interatomic distance here), plus rounding 4 eps |E| / (2 h) of the two energies."""
    return fmax * (h / 0.009) ** 2 / 6.0 + 4.0 * np.finfo(float).eps * e_abs / (2.0 * h)


@pytest.mark.parametrize("case", ["vacDivaline", "cluster"])
@pytest.mark.parametrize("model", [1, 2])
def test_forces_are_the_gradient(case, model):
    if case == "vacDivaline":
        _, s = amber_system("vacDivaline", list(range(22, 32)), implicit_solvent="OBC%d" % model)
        x, q, rho, S, alch = s.positions, s.charge, s.implicit_solvent.radius, s.implicit_solvent.scale, list(range(22, 32))
        atoms = [0, 5, 11, 22, 23, 30, 34]
    else:
        x, q, rho, S = random_cluster()
        alch, atoms = [2, 3, 7], list(range(12))
    h = 1e-5
    for le in (1.0, 0.3):
        def energy(xx):
            pol, sa, _ = gbr.evaluate(gbr.coefficients(xx, q, rho, S, alch, model), le)
            return pol + sa
        pol, sa, f = gbr.evaluate(gbr.coefficients(x, q, rho, S, alch, model), le)
        fd = _central_differences(np.array(x, dtype=np.float64), energy, atoms, h)
        bar = fd_bar(np.abs(f).max(), abs(pol + sa), h)
        assert bar < 1e-5 * np.abs(f).max()
        assert np.abs(fd - f[atoms]).max() <= bar, (case, model, le, np.abs(fd - f[atoms]).max(), bar)


@pytest.mark.parametrize("case", ["vacDivaline", "cluster"])
def test_net_force_and_torque_vanish(case):
    """E depends on distances only: the forces of every lambda class sum to zero and exert no torque (to rounding of n^2 terms)."""
    if case == "vacDivaline":
        _, s = amber_system("vacDivaline", list(range(22, 32)), implicit_solvent="OBC2")
        c = gbr.system_coefficients(s); x = s.positions
    else:
        x, q, rho, S = random_cluster()
        c = gbr.coefficients(x, q, rho, S, [2, 3, 7])
    for k in range(3):
        f = c["force"][k]
        scale = max(np.abs(f).max(), 1e-300)
        assert np.abs(f.sum(0)).max() <= 1e-12 * scale * len(x)
        assert np.abs(np.cross(x - x.mean(0), f).sum(0)).max() <= 1e-12 * scale * len(x) * np.abs(x - x.mean(0)).max()


@pytest.mark.parametrize("name", ["vacDivaline", "TOL-parm"])
def test_system_from_amber_fills_the_field(name):
    prm, s = amber_system(name, implicit_solvent="OBC2", solute_dielectric=1.5)
    gb = s.implicit_solvent
    assert gb.model == _abi.GB_OBC2 and gb.solute_dielectric == 1.5 and gb.solvent_dielectric == 78.5 and gb.surface_area_energy == 2.25936
    typed = np.asarray(prm["RADII"]) > 0.0       # (TOL-parm's water is written without types or GB parameters: it gets mbondi's, as it gets TIP3P's LJ)
    assert np.array_equal(gb.radius[typed], np.asarray(prm["RADII"])[typed] * 0.1) and np.array_equal(gb.scale[typed], np.asarray(prm["SCREEN"])[typed])
    assert typed.sum() == {"vacDivaline": 35, "TOL-parm": 15}[name]
    assert set(np.unique(gb.radius[~typed])) <= {0.08, 0.15} and np.all(gb.scale[~typed] == 0.85)
    assert len(gb.radius) == s.n_atoms and gb.radius.min() > 0.05 and 0.0 < gb.scale.min() <= gb.scale.max() < 1.0
    assert amber_system(name, implicit_solvent="OBC1")[1].implicit_solvent.model == _abi.GB_OBC1
    assert amber_system(name)[1].implicit_solvent is None
    # the helpers that copy a System carry the field
    assert systems.freeze_atoms(s, [0, 1]).implicit_solvent is gb
    assert systems.restrain_positions(s, [0], 10.0).implicit_solvent is gb
    s.check_implicit_solvent()
    d, keep = gb.to_desc()
    assert d.model == 2 and d.radius[s.n_atoms - 1] == gb.radius[-1] and d.scale[0] == gb.scale[0]


def test_save_and_load_carry_the_field(tmp_path):
    _, s = amber_system("vacDivaline", implicit_solvent="OBC1", solvent_dielectric=60.0)
    p = str(tmp_path / "s.npz")
    systems.save_system(p, s)
    t, extra = systems.load_system(p)
    assert systems.same_implicit_solvent(s.implicit_solvent, t.implicit_solvent) and not extra
    assert not systems.same_implicit_solvent(s.implicit_solvent, None) and systems.same_implicit_solvent(None, None)


def test_refusals():
    prm = amber.read_prmtop(os.path.join(GOLDEN, "TOL-parm.prmtop"))
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "TOL-parm.inpcrd"))
    with pytest.raises(ValueError, match="NoCutoff"):
        amber.system_from_amber(prm, pos, box, nonbonded_method="PME", implicit_solvent="OBC2")
    for name in ("HCT", "GBn", "GBn2"):
        with pytest.raises(ValueError, match="OBC1.*OBC2"):
            amber.system_from_amber(prm, pos, box, nonbonded_method="NoCutoff", implicit_solvent=name)
    with pytest.raises(ValueError, match="OBC1.*OBC2"):
        amber.system_from_amber(prm, pos, box, nonbonded_method="NoCutoff", implicit_solvent="OBC2", implicit_solvent_kappa=1.0)
    with pytest.raises(ValueError, match="OBC1.*OBC2"):
        amber.system_from_amber(prm, pos, box, nonbonded_method="NoCutoff", implicit_solvent="OBC2", implicit_solvent_salt_conc=0.15)
    s = amber.system_from_amber(prm, pos, box, nonbonded_method="NoCutoff", implicit_solvent="OBC2")
    s.implicit_solvent.radius[7] = 0.009
    with pytest.raises(ValueError, match="radius.*atom 7"):
        s.check_implicit_solvent()
    s.implicit_solvent.radius[7] = 0.15
    s.implicit_solvent.solvent_dielectric = 0.0
    with pytest.raises(ValueError, match="dielectric"):
        s.check_implicit_solvent()
    s.implicit_solvent.solvent_dielectric = 78.5
    s.custom_pair_mode = _abi.PAIR_ETHYLENE
    with pytest.raises(ValueError, match="custom forces"):
        s.check_implicit_solvent()
    s.custom_pair_mode = _abi.PAIR_STANDARD
    s.annihilate_electrostatics = False
    with pytest.raises(ValueError, match="annihilate_electrostatics"):
        s.check_implicit_solvent()
    s.annihilate_electrostatics = True
    s.check_implicit_solvent()
    # the engine's wrapper raises them before any library is loaded
    from blues_amd import integrators
    from blues_amd.engine import EngineError, NativeEngine
    data = integrators.generateNCMCIntegrator(nstepsNC=4, dt=0.002, temperature=300.0, seed=1).to_data(precision=1)
    data.measure_heat = 1
    with pytest.raises(EngineError, match="measure_shadow_work / measure_heat"):
        NativeEngine(s, data)


def test_ctypes_mirror_of_the_descriptor(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    probe = tmp_path / "gb_sizes.c"
    probe.write_text('#include "blues_engine.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(BluesImplicitSolventDesc), '
                     'offsetof(BluesImplicitSolventDesc, solute_dielectric), offsetof(BluesImplicitSolventDesc, radius), offsetof(BluesImplicitSolventDesc, scale), '
                     'BLUES_ABI_VERSION); return (int)(sizeof(&blues_engine_create_gb) == 0); }\n')
    exe = tmp_path / "gb_sizes"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o", str(tmp_path / "gb_sizes.o")])
    probe2 = tmp_path / "gb_sizes2.c"
    probe2.write_text(probe.read_text().replace("return (int)(sizeof(&blues_engine_create_gb) == 0);", "return 0;"))
    subprocess.check_call([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe2), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _abi.BluesImplicitSolventDesc
    assert out == [ctypes.sizeof(D), D.solute_dielectric.offset, D.radius.offset, D.scale.offset, _abi.ABI_VERSION]
    assert (_abi.GB_NONE, _abi.GB_OBC1, _abi.GB_OBC2) == (0, 1, 2)
