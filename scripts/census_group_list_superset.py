"""Census behind the group lists' kept supersets (kernels_nb.h: build_lists_body): on the flagship (S23k, 275 mobile atoms, frozen) the
size of a list's superset -- every non-alchemical atom within the list's sphere + slack D of its centre, and every mobile one -- for
D = 0.2, 0.3 and 0.4 nm, for the group list (all i-slots: one list at 5 tiles per list) and for the alchemical tile's list, beside
the number of atoms the sphere test itself passes.  Sizes only: how long a chain stays inside needs a trajectory (the GPU counts
blues_get_global("group_list_superset_served" / "_fallback") say it for the runs in profiles/group_list_superset/README.md).
   python scripts/census_group_list_superset.py"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from blues_amd import systems

CUTOFF, SKIN = 1.0, 0.20   # list radius of a frozen candidate in a mostly frozen chain of a large batch (blues_engine.hip: derive_margins)

s, _v = systems.s23k(mobile_atoms=275, frozen=True)
x = np.asarray(s.positions).reshape(-1, 3); box = np.asarray(s.box).reshape(-1)[:3]
mi = lambda d: d - box * np.round(d / box)
alch = np.zeros(len(x), bool); alch[np.asarray(s.alchemical_atoms)] = True
mobile = (np.asarray(s.mass) > 0) & ~alch
print("atoms %d, mobile non-alchemical %d, alchemical %d, box %s" % (len(x), mobile.sum(), alch.sum(), box))
for name, sel in (("group list (all i-slots)", mobile), ("alchemical tile", alch)):
    xi = x[sel]
    rel = mi(xi - xi[0])
    mid = 0.5 * (rel.min(0) + rel.max(0))
    rad = np.sqrt(((rel - mid) ** 2).sum(1).max())
    d = np.sqrt((mi(x - (xi[0] + mid)) ** 2).sum(1))
    base = (~alch & (d < rad + CUTOFF + SKIN)).sum()
    print("%s: radius %.3f nm, sphere test passes %d atoms" % (name, rad, base))
    for D in (0.2, 0.3, 0.4):
        n = (~alch & (mobile | (d < rad + CUTOFF + SKIN + D))).sum()
        print("    D = %.1f nm: superset %5d atoms = %.3f of all, %d chunks of 64 per wave of 16 (all atoms: %d)" % (D, n, n / len(x), -(-n // 1024), -(-len(x) // 1024)))
