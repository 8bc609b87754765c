"""Cost of self-gravity (csrc/qk_gravity.hip) on one level: a Gaussian blob of gas in a unit box of n^3 cells (default 64; boxes of at most 128^3),
G = 1, the reference's default tolerances (1e-5, 1e-5).  HIP-event time of one open-boundary solve from a zero first guess and of the kick, the
profiled time of every gravity kernel group in that solve (the two multigrid solves — host reads of the residual norm included —, the S^2 surface
potential, its reduction), and the V-cycle counts; next to the time of a hydro step of the same state.  Each figure is the median of `reps` (5)
repetitions.  Prints one JSON line; profiles/gravity/README.md keeps the results.     python profiles/tools/gravity_time.py [n ...]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import read_profile  # noqa: E402
from quokka_amd import capi  # noqa: E402
from quokka_amd.multifab import Context  # noqa: E402
from quokka_amd.simulation import Geometry, HydroSimulation  # noqa: E402

sizes = [int(a) for a in sys.argv[1:]] or [64]
reps = 5
ctx = Context(0)
L = ctx.L


def med(v):
    return sorted(v)[len(v) // 2]


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def one(n):
    geom = Geometry(3, [n, n, n], [0.0] * 3, [1.0] * 3, [0, 0, 0])
    bcs = [([capi.BC_FOEXTRAP] * 3, [capi.BC_FOEXTRAP] * 3) for _ in range(6)]
    sim = HydroSimulation(ctx, geom, capi.traits(5.0 / 3.0, False, 3), bcs, [min(n, 128)] * 3)
    sim.stopTime_ = 1.0e30
    dx = geom.dx

    def ic(i, j, k):
        r2 = ((i + 0.5) * dx[0] - 0.45) ** 2 + ((j + 0.5) * dx[1] - 0.55) ** 2 + ((k + 0.5) * dx[2] - 0.5) ** 2
        U = np.zeros((6,) + i.shape)
        U[0] = 1.0 + 10.0 * np.exp(-0.5 * r2 / 0.12 ** 2)
        U[5] = 0.1 / (5.0 / 3.0 - 1.0)
        U[4] = U[5]
        return U

    sim.doPoissonSolve_, sim.Gconst_ = 1, 1.0
    sim.set_initial_conditions(ic)  # (the first solve: allocations)
    solve, kick, prof, cycles = [], [], [], None
    for _ in range(reps):
        L.qk_profile_reset(ctx.h)
        L.qk_profile_enable(ctx.h, 1)
        solve.append(events(sim.calculateGpotAllLevels))
        L.qk_profile_enable(ctx.h, 0)
        prof.append({k: v[1] for k, v in read_profile(ctx).items() if k.startswith("gravity_")})
        cycles = sim.poisson.cycles
        kick.append(events(lambda: sim.gravAccelAllLevels(0.0)))  # (dt = 0: the state stays what it is)
    sim.doPoissonSolve_ = 0
    hydro = [events(lambda: sim.step()) for _ in range(reps + 1)][1:]
    return {"n": n, "boxes": sim.lev.nboxes, "ghosts": sim.poisson.S, "pairs": sim.poisson.S ** 2, "v_cycles": list(cycles),
            "residual": list(sim.poisson.resnorm), "open_solve_ms": med(solve), "open_solve_ms_all": solve, "kick_ms": med(kick),
            "kernel_groups_ms": {k: med([p.get(k, float("nan")) for p in prof]) for k in sorted(prof[0])},
            "surface_potential_ns_per_pair": med([p.get("gravity_surface_potential", float("nan")) for p in prof]) * 1e6 / sim.poisson.S ** 2,
            "hydro_step_ms": med(hydro)}


print(json.dumps({"reltol": 1.0e-5, "abstol": 1.0e-5, "runs": [one(n) for n in sizes]}))
