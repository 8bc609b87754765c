"""Cost of tracer particles on a refined hierarchy: Sedov n^3 + one refined level (ErrorEst-driven grids, regrid_int 2), one tracer per level-0
cell.  Two hierarchies are stepped alternately from the same start: one with AmrSimulation.do_tracers = 1, one without tracers on the same path
(reference-shaped operators on every level, no overlap) — by passivity they hold the same states, so every pair of steps does the same hydro work.
Wall time per coarse step between device synchronisations (the AMR driver is host-bound at small sizes: that is part of what a step costs);
medians over `pairs` pairs after `warmup` pairs, with the range.  Prints one JSON line; profiles/tracers/README.md keeps the results.
    python profiles/tools/tracer_amr_time.py [n max_grid_size blocking_factor pairs warmup]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from quokka_amd.amr_simulation import sedov_amr_problem  # noqa: E402
from quokka_amd.multifab import Context  # noqa: E402

argv = sys.argv[1:]
n = int(argv[0]) if len(argv) > 0 else 32
mgs = int(argv[1]) if len(argv) > 1 else 16
bf = int(argv[2]) if len(argv) > 2 else 8
pairs = int(argv[3]) if len(argv) > 3 else 15
warmup = int(argv[4]) if len(argv) > 4 else 4
ctx = Context(0)


def make(tracers: bool):
    amr = sedov_amr_problem(ctx, n, max_level=1, max_grid_size=mgs, blocking_factor=bf)
    if tracers:
        amr.do_tracers = 1
        amr.InitTracerParticles()
    else:
        for L in amr.levels:
            L.use_fused = False
    return amr


def timed(amr):
    if not amr.do_tracers:  # (levels a regrid made take the default path otherwise)
        for L in amr.levels:
            L.use_fused = False
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    amr.step()
    torch.cuda.synchronize()
    return 1.0e3 * (time.perf_counter() - t0)


def med(v):
    return sorted(v)[len(v) // 2]


with_t, without = make(True), make(False)
w, wo = [], []
for it in range(warmup + pairs):
    a, b = timed(with_t), timed(without)
    assert with_t.dt_ == without.dt_, "the tracers are not passive"
    if it >= warmup:
        w.append(a)
        wo.append(b)
counts = [L.tracers.num_particles for L in with_t.levels]
print(json.dumps({"n": n, "max_grid_size": mgs, "blocking_factor": bf, "pairs": pairs, "warmup": warmup, "coarse_steps": with_t.istep[0],
                  "cells_per_level": [with_t.CountCells(l) for l in range(with_t.finest_level + 1)], "particles_per_level": counts,
                  "step_with_tracers_ms": round(med(w), 3), "step_without_ms": round(med(wo), 3), "ratio": round(med(w) / med(wo), 4),
                  "with_range_ms": [round(min(w), 3), round(max(w), 3)], "without_range_ms": [round(min(wo), 3), round(max(wo), 3)]}))
