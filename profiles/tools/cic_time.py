"""Cost of the CIC particles (csrc/qk_cic.hip) on one level: HIP-event medians (of `reps` = 5) of the deposit as the driver runs it (key kernel + stable
sort + range lookup + deposit kernel), of the kick and of the drift, for 2, 1e4 and 1e6 particles on n^3 cells (default 64 and 128) of a unit box —
uniformly random, and a Gaussian cluster of sigma = 0.05 box lengths at the centre — with the profiled time of the two deposit kernels alone.  Then
the reference's BinaryOrbit deck (tests/golden/BinaryOrbit.in, BinaryOrbit_particles.txt) to its stop_time: worst separation error sampled every
step and every tenth step (the reference's sampling), and the wall time.  Prints one JSON line; profiles/cic/README.md keeps the results.
     python profiles/tools/cic_time.py [--no-orbit] [n ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import read_profile  # noqa: E402
from quokka_amd import capi  # noqa: E402
from quokka_amd.cic import CICParticles  # noqa: E402
from quokka_amd.gravity import PoissonSolver  # noqa: E402
from quokka_amd.multifab import Context  # noqa: E402
from quokka_amd.simulation import Geometry, HydroSimulation  # noqa: E402

args = sys.argv[1:]
orbit = "--no-orbit" not in args
sizes = [int(a) for a in args if not a.startswith("--")] or [64, 128]
reps = 5
ctx = Context(0)
L = ctx.L
GOLDEN = os.path.join(ROOT, "tests", "golden")


def med(v):
    return sorted(v)[len(v) // 2]


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def particles(kind, count, rng):
    if kind == "uniform":
        return rng.random((count, 3))
    return np.clip(0.5 + 0.05 * rng.standard_normal((count, 3)), 0.0, np.nextafter(1.0, 0.0))


def one(n):
    geom = Geometry(3, [n, n, n], [0.0] * 3, [1.0] * 3, [0, 0, 0])
    bcs = [([capi.BC_FOEXTRAP] * 3, [capi.BC_FOEXTRAP] * 3) for _ in range(6)]
    sim = HydroSimulation(ctx, geom, capi.traits(5.0 / 3.0, False, 3), bcs, [min(n, 128)] * 3)
    ps = PoissonSolver(ctx, [n, n, n], geom.dx[0])
    phi = torch.randn(ps.phi.shape, dtype=torch.float64, device=ctx.device)
    rng = np.random.default_rng(n)
    runs = []
    for kind in ("uniform", "cluster"):
        for count in (2, 10 ** 4, 10 ** 6):
            cic = CICParticles(sim)
            pos = particles(kind, count, rng)
            cic.init_from_arrays(pos, np.full(count, 1.0 / count), np.zeros((count, 3)))
            fullest = int(torch.bincount(cic.cell_keys()).max().item())
            cic.deposit(ps, 1.0)  # (allocations)
            dep, kick, drift, prof = [], [], [], []
            for _ in range(reps):
                ps.zero_rhs()
                L.qk_profile_reset(ctx.h)
                L.qk_profile_enable(ctx.h, 1)
                dep.append(events(lambda: cic.deposit(ps, 1.0)))
                L.qk_profile_enable(ctx.h, 0)
                prof.append({k: v[1] for k, v in read_profile(ctx).items() if k.startswith("cic_")})
                kick.append(events(lambda: cic.kick(phi, 0.0)))   # (dt = 0: the velocities stay what they are)
                drift.append(events(lambda: cic.drift(0.0)))
            runs.append({"n": n, "particles": kind, "np": count, "fullest_base_cell": fullest, "deposit_ms": med(dep), "kick_ms": med(kick),
                         "drift_ms": med(drift), "kernels_ms": {k: med([p.get(k, float("nan")) for p in prof]) for k in sorted(prof[0])}})
    return runs


def binary_orbit():
    deck = {}
    for line in open(os.path.join(GOLDEN, "BinaryOrbit.in")):
        line = line.split("#")[0].strip()
        if "=" in line:
            k, v = line.split("=", 1)
            deck[k.strip()] = v.split()
    n = [int(v) for v in deck["amr.n_cell"]]
    geom = Geometry(3, n, [float(v) for v in deck["geometry.prob_lo"]], [float(v) for v in deck["geometry.prob_hi"]], [0, 0, 0])
    bcs = []
    for comp in range(6):
        kinds = [capi.BC_REFLECT_ODD if comp == 1 + d else capi.BC_REFLECT_EVEN for d in range(3)]
        bcs.append((list(kinds), list(kinds)))
    sim = HydroSimulation(ctx, geom, capi.traits(1.0, False, 3, cs_isothermal=1.3e7), bcs, [int(deck["amr.max_grid_size"][0])] * 3)
    sim.cflNumber_, sim.stopTime_, sim.maxTimesteps_ = float(deck["cfl"][0]), float(deck["stop_time"][0]), int(deck["max_timesteps"][0])
    sim.doPoissonSolve_, sim.initDt_, sim.do_cic_particles = 1, 1.0e3, 1
    sim.createInitialParticles = lambda s: s.CICParticles.init_from_ascii_file(os.path.join(GOLDEN, "BinaryOrbit_particles.txt"))

    def ic(i, j, k):
        U = np.zeros((6,) + i.shape)
        U[0] = 1.0e-22
        return U
    sim.set_initial_conditions(ic)
    worst, worst10, worst_step = 0.0, 0.0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while sim.istep < sim.maxTimesteps_ and sim.tNew_ < sim.stopTime_ * (1.0 - 1.0e-12):
        if not sim.step():
            break
        p = sim.CICParticles.positions()
        if p.shape[0] != 2:
            break
        err = abs(np.sqrt(((p[0] - p[1]) ** 2).sum()) - 6.25e12) / geom.dx[0]
        if err > worst:
            worst, worst_step = err, sim.istep
        if sim.istep % 10 == 0:
            worst10 = max(worst10, err)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    mom = (sim.CICParticles.masses()[:, None] * sim.CICParticles.velocities()).sum(axis=0)
    return {"steps": sim.istep, "t_end": sim.tNew_, "particles_left": sim.CICParticles.num_particles, "worst_separation_error_cells": worst,
            "worst_at_step": worst_step, "worst_every_tenth_step": worst10, "criterion": 0.18, "wall_s": wall, "ms_per_step": 1.0e3 * wall / max(sim.istep, 1),
            "total_particle_momentum": mom.tolist(), "one_particle_momentum": 2.0e34 * 10332860.0}


out = {"runs": [r for n in sizes for r in one(n)]}
if orbit:
    out["binary_orbit"] = binary_orbit()
print(json.dumps(out))
