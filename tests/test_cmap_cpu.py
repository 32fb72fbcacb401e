"""CPU suite of the CMAP torsion term: the numpy / scipy reference (tests/cmap_reference.py) pinned by itself, the prmtop mapping,
the refusals of SystemData.check_cmap, the descriptor layout and the helpers that carry the fields."""
import copy
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cmap_cases as cc
import cmap_reference as ref
from blues_amd import _abi, amber, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TWO_PI = 2.0 * np.pi


# ---- 1. the reference
def _surface_error(n, count=200000, seed=11):
    a = np.random.default_rng(seed).uniform(0.0, TWO_PI, size=(count, 2))
    e, _, _ = ref.evaluate(cc.surface_map(n), a[:, 0], a[:, 1])
    return np.abs(e - cc.surface(a[:, 0], a[:, 1])).max()


def test_reference_is_fourth_order_on_an_analytic_surface():
    """E = 4 cos phi + 2 sin 2 psi + 3 cos(phi - psi + 0.4): measured 5.3e-4 kJ/mol at n = 24 and 3.2e-5 at n = 48 (ratio 16.3) over
    200,000 random angles.  Bars: 2 x 5.3e-4, ratio within 12..20 -- a wrong derivative or a transposed index breaks fourth order."""
    e24, e48 = _surface_error(24), _surface_error(48)
    print("CMAP reference against the surface: n=24 %.3e, n=48 %.3e, ratio %.2f" % (e24, e48, e24 / e48))
    assert e24 <= 2.0 * 5.3e-4
    assert 12.0 <= e24 / e48 <= 20.0


def test_reference_derivatives_are_the_gradient_of_its_energy():
    E = cc.random_map(8)
    tab = ref.tables(E)
    a = np.random.default_rng(2).uniform(0.05, TWO_PI - 0.05, size=(200, 2))
    h = 1e-6
    _, ep, es = ref.evaluate(E, a[:, 0], a[:, 1], tab)
    dp = (ref.evaluate(E, a[:, 0] + h, a[:, 1], tab)[0] - ref.evaluate(E, a[:, 0] - h, a[:, 1], tab)[0]) / (2 * h)
    ds = (ref.evaluate(E, a[:, 0], a[:, 1] + h, tab)[0] - ref.evaluate(E, a[:, 0], a[:, 1] - h, tab)[0]) / (2 * h)
    scale = np.abs(ep).max()
    assert np.abs(dp - ep).max() <= 1e-7 * scale and np.abs(ds - es).max() <= 1e-7 * scale


@pytest.mark.parametrize("n", [4, 5, 24])
def test_reference_is_exact_at_grid_points_and_continuous_across_patches(n):
    E = cc.random_map(n, seed=n)
    tab = ref.tables(E)
    g = np.arange(n) * TWO_PI / n
    P, S = np.meshgrid(g, g, indexing="ij")
    e, ep, es = ref.evaluate(E, P.reshape(-1), S.reshape(-1), tab)
    assert np.abs(e.reshape(n, n) - E).max() <= 1e-12
    assert np.abs(ep.reshape(n, n) - tab[0]).max() <= 1e-12 * max(1.0, np.abs(tab[0]).max())
    assert np.abs(es.reshape(n, n) - tab[1]).max() <= 1e-12 * max(1.0, np.abs(tab[1]).max())
    # across every patch border and across the seam (0 / 2 pi), 1e-9 rad to either side, the other angle anywhere
    other = np.random.default_rng(3).uniform(0.0, TWO_PI, size=n + 1)
    border = np.arange(n + 1) * TWO_PI / n
    below, above = (border - 1e-9) % TWO_PI, (border + 1e-9) % TWO_PI
    size = [np.abs(q).max() for q in ref.evaluate(E, np.random.default_rng(4).uniform(0, TWO_PI, 4000), np.random.default_rng(5).uniform(0, TWO_PI, 4000), tab)]
    curv = 40.0 * max(size) * (n / TWO_PI) ** 2       # (a generous bound of the second derivatives: what 2e-9 rad may change)
    for first in (True, False):
        lo = ref.evaluate(E, below, other, tab) if first else ref.evaluate(E, other, below, tab)
        hi = ref.evaluate(E, above, other, tab) if first else ref.evaluate(E, other, above, tab)
        for q in range(3):
            assert np.abs(lo[q] - hi[q]).max() <= 2e-9 * curv + 1e-12 * size[q], (first, q, np.abs(lo[q] - hi[q]).max())
    # the end of the range: 2 pi itself and the double just below it lie in patch n - 1 (floor(phi / delta) = n there) and continue 0
    top = np.array([TWO_PI, np.nextafter(TWO_PI, 0.0)])
    for q, (x, y) in enumerate(zip(ref.evaluate(E, top, other[:2], tab), ref.evaluate(E, np.zeros(2), other[:2], tab))):
        assert np.abs(x - y).max() <= 1e-12 * size[q]


def test_reference_dihedral_gradient_and_range():
    rng = np.random.default_rng(8)
    for _ in range(20):
        x = rng.normal(size=(4, 3)) * 0.2
        a, g = ref.dihedral(x)
        assert 0.0 <= a <= TWO_PI
        num = np.zeros((4, 3))
        for i in range(4):
            for k in range(3):
                xp, xm = x.copy(), x.copy(); xp[i, k] += 1e-6; xm[i, k] -= 1e-6
                d = ref.dihedral(xp)[0] - ref.dihedral(xm)[0]
                num[i, k] = (d - TWO_PI * np.round(d / TWO_PI)) / 2e-6
        assert np.abs(num - g).max() <= 1e-6 * np.abs(g).max()
        assert np.abs(g.sum(0)).max() <= 1e-12 * np.abs(g).max()
    x = cc.five_atoms(0.3, 5.0)
    assert abs(ref.dihedral(x[:4])[0] - 0.3) < 1e-12 and abs(ref.dihedral(x[1:])[0] - 5.0) < 1e-12
    box = np.array([2.0, 2.5, 3.0])
    moved = x[:4] + np.array([[2.0, 0, 0], [0, -2.5, 0], [0, 0, 3.0], [-2.0, 2.5, 0]])
    assert abs(ref.dihedral(moved, box)[0] - ref.dihedral(x[:4])[0]) < 1e-12


# ---- 2. the prmtop mapping
def _sections(prefix, maps_kcal, index, count=None, comment=True):
    out = []
    def flag(name, fmt, values, per_line, form):
        out.append("%%FLAG %s%s" % (prefix, name))
        if comment:
            out.append("%COMMENT  hand-made for the test")
        out.append("%%FORMAT(%s)" % fmt)
        values = list(values)
        for k in range(0, len(values), per_line):
            out.append("".join(form % v for v in values[k:k + per_line]))
        if not values:
            out.append("")
    flag("CMAP_COUNT", "2I8", count if count is not None else (len(index), len(maps_kcal)), 2, "%8d")
    flag("CMAP_RESOLUTION", "20I4", [g.shape[0] for g in maps_kcal], 20, "%4d")
    for k, g in enumerate(maps_kcal):
        flag("CMAP_PARAMETER_%02d" % (k + 1), "8F9.5", g.reshape(-1), 8, "%9.5f")
    flag("CMAP_INDEX", "6I8", [v for row in index for v in row], 6, "%8d")
    return "\n".join(out) + "\n"


def _file_maps():
    rng = np.random.default_rng(21)
    return [np.round(rng.normal(size=(4, 4)) * 3.0, 5), np.round(rng.normal(size=(24, 24)) * 3.0, 5)]


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(open(os.path.join(GOLDEN, "vacDivaline.prmtop")).read() + text)
    return amber.read_prmtop(str(p))


@pytest.mark.parametrize("prefix", ["", "CHARMM_"])
def test_prmtop_sections_become_the_fields(tmp_path, prefix):
    plain = amber.read_prmtop(os.path.join(GOLDEN, "vacDivaline.prmtop"))
    five = cc.backbone_atoms(plain["ATOM_NAME"])
    assert [plain["ATOM_NAME"][a] for a in five] == ["C", "N", "CA", "C", "OXT"] and five == [16, 18, 20, 32, 34]   # (a dipeptide: no third residue's N)
    G = _file_maps()
    prm = _write(tmp_path, "a.prmtop", _sections(prefix, G, [[a + 1 for a in five] + [2]]))
    maps, tors = amber.cmap_from_prmtop(prm, 35)
    assert len(maps) == 2 and maps[0].shape == (4, 4) and maps[1].shape == (24, 24)
    assert tors.tolist() == [[1, 16, 18, 20, 32, 18, 20, 32, 34]]
    for g, m in zip(G, maps):
        n = g.shape[0]
        for k in range(n):
            for l in range(n):       # file index [k][l] (phi slow, both from -180 degrees) arrives at E[(k - n/2) mod n, (l - n/2) mod n] in kJ/mol
                assert m[(k - n // 2) % n, (l - n // 2) % n] == pytest.approx(4.184 * g[k, l], rel=1e-15, abs=0.0)
    pos, _, box = amber.read_inpcrd(os.path.join(GOLDEN, "vacDivaline.inpcrd"))
    s = amber.system_from_amber(prm, pos, box, nonbonded_method="NoCutoff")
    assert np.array_equal(s.cmap_torsions, tors) and all(np.array_equal(a, b) for a, b in zip(s.cmap_maps, maps)) and s.has_cmap
    none = amber.system_from_amber(plain, pos, box, nonbonded_method="NoCutoff")
    assert none.cmap_maps == () and none.cmap_torsions.shape == (0, 9) and not none.has_cmap and none.ext_desc() is None
    assert amber.cmap_from_prmtop(plain)[0] == ()


def test_prmtop_refusals(tmp_path):
    G = _file_maps()
    ok = [[17, 19, 21, 33, 35, 1]]
    odd = [np.zeros((5, 5))]
    cases = [
        (_sections("", odd, ok), "odd resolution 5"),
        (_sections("", G, ok, count=(2, 2)), "CMAP_INDEX holds 6 integers"),
        (_sections("", G, ok, count=(1, 3)), "CMAP_RESOLUTION holds 2"),
        (_sections("", G, ok).replace("%FLAG CMAP_PARAMETER_02", "%FLAG CMAP_PARAMETER_09"), "CMAP_PARAMETER_02 holds 0 values"),
        (_sections("", G, [[17, 19, 21, 33, 35, 3]]), "type 3 of 2"),
        (_sections("", G, [[17, 19, 21, 33, 35, 0]]), "type 0 of 2"),
        (_sections("", G, [[17, 19, 21, 33, 36, 1]]), "atom out of range"),
        (_sections("", G, [[0, 19, 21, 33, 35, 1]]), "atom out of range"),
    ]
    for k, (text, why) in enumerate(cases):
        prm = _write(tmp_path, "bad%d.prmtop" % k, text)
        with pytest.raises(ValueError, match=why):
            amber.cmap_from_prmtop(prm, 35)


# ---- 3. what check_cmap (and, with the same words, the library) refuses
def test_check_cmap_refusals():
    from blues_amd import engine
    good = cc.divaline([cc.surface_map(8)])
    good.check_cmap()
    def bad(**kw):
        s = copy.copy(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    t = good.cmap_torsions
    def tor(col, val):
        q = t.copy(); q[0, col] = val
        return q
    nan = cc.surface_map(8); nan[3, 2] = np.inf
    cases = [
        (bad(cmap_maps=(np.zeros((3, 3)),)), "size 3x3; a map is n x n with n from 4 to 64"),
        (bad(cmap_maps=(np.zeros((65, 65)),)), "size 65x65"),
        (bad(cmap_maps=(np.zeros((8, 6)),)), "size 8x6"),
        (bad(cmap_maps=(nan,)), "map 0: an energy is not finite"),
        (bad(cmap_torsions=tor(0, 1)), "torsion 0: map 1 of 1"),
        (bad(cmap_torsions=tor(0, -1)), "torsion 0: map -1 of 1"),
        (bad(cmap_maps=()), "torsion 0: map 0 of 0"),
        (bad(cmap_torsions=tor(8, 35)), "torsion 0: atom index out of range"),
        (bad(cmap_torsions=tor(1, -1)), "torsion 0: atom index out of range"),
        (bad(cmap_torsions=tor(4, int(t[0, 1]))), "two equal atoms within one dihedral"),
        (bad(cmap_torsions=tor(8, int(t[0, 6]))), "two equal atoms within one dihedral"),
        (bad(cmap_torsions=np.zeros((1, 8), np.int32)), r"an \(m, 9\) array"),
    ]
    data = _abi.IntegratorData(timestep=0.002, temperature=300.0, nsteps_neq=2, lambda_sterics=np.ones(5), lambda_electrostatics=np.ones(5))
    for s, why in cases:
        with pytest.raises(ValueError, match=why):
            s.check_cmap()
        with pytest.raises(engine.EngineError, match=why):     # the wrapper, before any library is loaded
            engine.NativeEngine(s, data)


def test_a_library_without_the_entry_point_is_named(monkeypatch):
    from blues_amd import engine
    lib = type("Old", (), {"blues_engine_create_ext": 1})()      # a library from before the maps
    monkeypatch.setattr(engine, "load", lambda: lib)
    data = _abi.IntegratorData(timestep=0.002, temperature=300.0, nsteps_neq=2, lambda_sterics=np.ones(5), lambda_electrostatics=np.ones(5))
    with pytest.raises(engine.EngineError, match="blues_get_cmap_angles"):
        engine.NativeEngine(cc.divaline([cc.surface_map(8)]), data)
    assert "blues_get_cmap_angles" in _abi.OPTIONAL_SYMBOLS and "blues_get_cmap_angles" in _abi.ENGINE_SYMBOLS


# ---- 4. the descriptor
def test_ctypes_mirror_of_the_descriptor(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    fields = ["struct_size", "alchemical_pme_treatment", "n_cmap_maps", "cmap_size", "cmap_energy", "n_cmap_torsions", "cmap_torsion_map", "cmap_torsion_atoms"]
    probe = tmp_path / "ext_sizes.c"
    probe.write_text('#include "blues_engine.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu ' + "%zu " * len(fields) + '%d %d %d %d\\n", sizeof(BluesSystemExt), '
                     + ", ".join("offsetof(BluesSystemExt, %s)" % f for f in fields)
                     + ', BLUES_ABI_VERSION, BLUES_SYSTEM_EXT_SIZE_V1, BLUES_CMAP_MIN_SIZE, BLUES_CMAP_MAX_SIZE); return 0; }\n')
    exe = tmp_path / "ext_sizes"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _abi.BluesSystemExt
    assert [n for n, _ in D._fields_] == fields
    assert out == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields] + [_abi.ABI_VERSION, _abi.SYSTEM_EXT_SIZE_V1, _abi.CMAP_MIN_SIZE, _abi.CMAP_MAX_SIZE]
    assert _abi.ABI_VERSION == 9 and _abi.N_ENERGY_TERMS == 10
    assert D.n_cmap_maps.offset == _abi.SYSTEM_EXT_SIZE_V1        # the new fields begin where the old struct ended


def test_ext_desc_carries_maps_in_the_abi_order():
    E = np.arange(16.0).reshape(4, 4); E[1, 2] = 77.0
    s = cc.divaline([E, cc.surface_map(6)])
    s.cmap_torsions = np.concatenate([s.cmap_torsions, s.cmap_torsions + np.array([1] + [0] * 8, np.int32)])
    d = s.ext_desc()
    assert d.struct_size == ctypes.sizeof(_abi.BluesSystemExt) and d.alchemical_pme_treatment == 0 and d.n_cmap_maps == 2 and d.n_cmap_torsions == 2
    assert [d.cmap_size[k] for k in range(2)] == [4, 6]
    assert d.cmap_energy[1 + 4 * 2] == 77.0 and d.cmap_energy[16] == cc.surface_map(6)[0, 0]        # energy[i + n * j]
    assert [d.cmap_torsion_map[k] for k in range(2)] == [0, 1]
    assert [d.cmap_torsion_atoms[k] for k in range(16)] == list(s.cmap_torsions[0, 1:]) * 2


# ---- 5. the helpers that carry the fields
def test_save_load_tile_and_freeze_carry_the_fields(tmp_path):
    s = cc.divaline([cc.surface_map(8), cc.random_map(5)])
    s.cmap_torsions = np.concatenate([s.cmap_torsions, np.array([[1, 0, 4, 16, 18, 6, 4, 16, 17]], np.int32)])
    s.check_cmap()
    systems.save_system(str(tmp_path / "s.npz"), s)
    back, extra = systems.load_system(str(tmp_path / "s.npz"))
    assert extra == {} and np.array_equal(back.cmap_torsions, s.cmap_torsions) and len(back.cmap_maps) == 2
    assert all(np.array_equal(a, b) for a, b in zip(back.cmap_maps, s.cmap_maps))
    systems.save_system(str(tmp_path / "p.npz"), cc.divaline())
    back, _ = systems.load_system(str(tmp_path / "p.npz"))
    assert not back.has_cmap and not any(k.startswith("cmap") for k in np.load(str(tmp_path / "p.npz")).files)
    s.box = np.array([3.0, 3.0, 3.0])
    t = systems.tile_system(s, (2, 1, 1))
    assert t.cmap_torsions.shape == (4, 9) and np.array_equal(t.cmap_torsions[:2], s.cmap_torsions)
    assert np.array_equal(t.cmap_torsions[2:, 0], s.cmap_torsions[:, 0]) and np.array_equal(t.cmap_torsions[2:, 1:], s.cmap_torsions[:, 1:] + 35)
    assert len(t.cmap_maps) == 2
    t.check_cmap()
    e0, _ = ref.energy_forces(s.cmap_maps, s.cmap_torsions, s.positions)
    e1, _ = ref.energy_forces(t.cmap_maps, t.cmap_torsions, t.positions)
    assert e1 == pytest.approx(2.0 * e0, rel=1e-13)
    for f in (systems.freeze_atoms(s, [16, 18]), systems.freeze_except(s, [20])):
        assert np.array_equal(f.cmap_torsions, s.cmap_torsions) and len(f.cmap_maps) == 2
