"""One chain to the letter (configs[1]): step time of a lone S23k engine under a few tuning specs.
   python scripts/dev_single.py "" "fuse_finalize=0" "fast_step=0,fuse_finalize=0" ..."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blues_amd import build, integrators, systems, tuning
build.build_engine()
from blues_amd.engine import NativeEngine
system, vel = systems.s23k(mobile_atoms=275, frozen=True)
for spec in (sys.argv[1:] or [""]):
    tuning.reset()
    if spec:
        tuning.set(**tuning.parse(spec))
    g = NativeEngine(system, integrators.generateNCMCIntegrator(nstepsNC=1200, dt=0.004, temperature=300.0, seed=3).to_data(precision=0)); g.set_velocities(vel)
    g.step(100)
    g.get_global("protocol_work")
    t0 = time.perf_counter(); g.step(1000); w = g.get_global("protocol_work"); dt = time.perf_counter() - t0
    print("[%s] %.2f us/step  %.0f ns/day  work %.6f  launches %d" % (spec, 1e6 * dt / 1000, 1000 * 0.004e-3 / (dt / 86400.0), w, g.stats()["kernel_launches"]), flush=True)
    g.close()
