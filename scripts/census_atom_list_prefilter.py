"""Census behind the prefilter of the atoms'-list builder (kernels_nb.h: build_atom_lists_body): for units of consecutive i-slots of the
flagship's mobile set in its sort order (S23k, 275 mobile atoms, one group list), the unit's reach (largest distance of one of its
atoms from the centre) and the share of the group list that lies within list radius + reach of the centre -- what the unit's walk
still has to test after the prefilter.  Units: the block's 8 slots, a wave's 2 slots (if they were adjacent), 3 slots.
   python scripts/census_atom_list_prefilter.py"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from blues_amd import systems

CUTOFF, SKIN, SKIN_M = 1.0, 0.20, 0.40   # the margins of a mostly frozen chain in a large batch (blues_engine.hip: derive_margins)


def hilbert3(X, bits=10):   # Skilling's transpose, as blues_engine.hip
    X = X.copy().astype(np.uint32)
    M = np.uint32(1 << (bits - 1))
    Q = M
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            m = (X[:, i] & Q) != 0
            X[m, 0] ^= P
            t = (X[:, 0] ^ X[:, i]) & P
            t[m] = 0
            X[:, 0] ^= t; X[:, i] ^= t
        Q >>= 1
    for i in range(1, 3): X[:, i] ^= X[:, i - 1]
    t = np.zeros(len(X), np.uint32)
    Q = M
    while Q > 1:
        m = (X[:, 2] & Q) != 0
        t[m] ^= np.uint32(Q - 1)
        Q >>= 1
    for i in range(3): X[:, i] ^= t
    key = np.zeros(len(X), np.uint64)
    for b in range(bits - 1, -1, -1):
        for i in range(3):
            key = (key << np.uint64(1)) | ((X[:, i] >> np.uint32(b)) & 1).astype(np.uint64)
    return key


s, _v = systems.s23k(mobile_atoms=275, frozen=True)
x = np.asarray(s.positions).reshape(-1, 3); box = np.asarray(s.box).reshape(-1)[:3]
fr = (x / box) % 1.0
order = np.argsort(hilbert3(np.minimum(1023, (fr * 1024).astype(np.int64))), kind="stable")
mi = lambda d: d - box * np.round(d / box)
alch = np.zeros(len(x), bool); alch[np.asarray(s.alchemical_atoms)] = True
mobile = np.asarray(s.mass) > 0
islots = np.array([o for o in order if mobile[o] and not alch[o]])        # the i-slots: mobile, non-alchemical atoms in sorted order
xi = x[islots]
print("i-slots", len(islots), "box", box)
# the group list (one group holds every tile here): what lies within the list radius of the group's bounding sphere
ref = xi[0]; rel = mi(xi - ref); mid = ref + 0.5 * (rel.min(0) + rel.max(0)); rad = np.sqrt((mi(xi - mid) ** 2).sum(1)).max()
rl = np.where(mobile, CUTOFF + SKIN_M, CUTOFF + SKIN)
lo, hi = rel.min(0), rel.max(0)
dbox = np.maximum(0.0, np.maximum(lo - mi(x - ref), mi(x - ref) - hi))
cand = np.nonzero((np.sqrt((mi(x - mid) ** 2).sum(1)) < rl + rad) & (np.sqrt((dbox ** 2).sum(1)) < rl))[0]
print("group radius %.3f nm, group list %d candidates (%d mobile)" % (rad, len(cand), mobile[cand].sum()))
xc, rlc = x[cand], rl[cand]
d = np.sqrt((mi(xi[:, None, :] - xc[None, :, :]) ** 2).sum(-1))
print("entries of an atom's full list: mean %.0f" % (d < rlc[None, :]).sum(1).mean())
for name, U in (("block of 8 slots", 8), ("3 slots", 3), ("wave's 2 slots, adjacent", 2)):
    for centre in ("mean", "first atom"):
        reach, kept = [], []
        for b in range(0, len(xi), U):
            p = xi[b:b + U]
            c = p[0] + (mi(p - p[0]).mean(0) if centre == "mean" else 0.0)
            r = np.sqrt((mi(p - c) ** 2).sum(1)).max()
            reach.append(r); kept.append((np.sqrt((mi(xc - c) ** 2).sum(1)) < rlc + r).sum() / len(cand))
        reach, kept = np.array(reach), np.array(kept)
        print("%-26s centre = %-10s reach mean %.3f  p90 %.3f  max %.3f nm | kept share mean %.3f  max %.3f" % (name, centre, reach.mean(), np.percentile(reach, 90), reach.max(), kept.mean(), kept.max()))
        if U == 8 and centre == "mean":
            for thr in (0.3, 0.4, 0.5, 0.6, 0.8):
                print("    blocks with reach > %.1f nm: %d of %d, their kept share %.3f" % (thr, (reach > thr).sum(), len(reach), kept[reach > thr].mean() if (reach > thr).any() else 0.0))
