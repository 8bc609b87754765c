"""Cost of the tracer particles on the benchmark geometry: Sedov n^3 (default 256) in 128^3 boxes, one tracer per cell (16.8 M), operator-path
steps.  HIP-event time of the AdvectWithUmac kernel from step 1 on — the particles in cell order — and after `steps` (default 200) steps, next to the
time of operator-path steps of the same run taken with do_tracers = 0 (the particles sit those steps out: a timing run).  Each sample is the median of
five steps with tracers and five without, alternating.  The step
with tracers also pays the snapshot the retry loop takes (a clone of every particle array) and one device -> host read in Redistribute: the tool
reports the step times so that the difference shows them.
--fused-stages: the same on the fused kernels with HydroSimulation.tracers_on_fused_stages = 1 (stage 2 stores avgFaceVel itself); the step
without tracers is then the exact-form fused step, and the keys that say "operator" hold the fused figures ("path" tells which).
Prints one JSON line; profiles/tracers/README.md keeps the results.     python profiles/tools/tracer_time.py [n steps] [--fused-stages]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import read_profile  # noqa: E402
from quokka_amd.multifab import Context  # noqa: E402
from quokka_amd.simulation import sedov_problem  # noqa: E402

fused_stages = "--fused-stages" in sys.argv[1:]
argv = [a for a in sys.argv[1:] if a != "--fused-stages"]
n = int(argv[0]) if len(argv) > 0 else 256
steps = int(argv[1]) if len(argv) > 1 else 200
ctx = Context(0)
L = ctx.L
sim = sedov_problem(ctx, n, max_grid_size=min(n, 128), use_fused=fused_stages)
sim.tracers_on_fused_stages = int(fused_stages)
sim.do_tracers = 1
sim.InitTracerParticles()
np0 = sim.tracers.num_particles


def timed_step(with_tracers: bool):
    """one step between two events; with tracers also the profiled time of the tracer kernels in it"""
    sim.do_tracers = 1 if with_tracers else 0
    L.qk_profile_reset(ctx.h)
    L.qk_profile_enable(ctx.h, 1)  # (in both, so that both step times carry the same event pairs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert sim.step()
    e1.record()
    torch.cuda.synchronize()
    L.qk_profile_enable(ctx.h, 0)
    sim.do_tracers = 1
    k = {name: v[1] / max(v[0], 1) for name, v in read_profile(ctx).items() if name.startswith("tracer_")} if with_tracers else {}
    return e0.elapsed_time(e1), k


def med(v):
    return sorted(v)[len(v) // 2]


def sample(label, pairs=5):
    """medians over `pairs` steps with tracers and `pairs` without, alternating (other work shares the host; the first step also allocates)"""
    first = sim.istep + 1
    w, wo, ks = [], [], []
    for _ in range(pairs):
        ms, k = timed_step(True)
        w.append(ms)
        ks.append(k)
        wo.append(timed_step(False)[0])
    adv = med([k.get("tracer_AdvectWithUmac", float("nan")) for k in ks])
    red = med([k.get("tracer_Redistribute", float("nan")) for k in ks])
    ms_with, ms_without = med(w), med(wo)
    row = {"at": label, "steps": [first, sim.istep], "particles": sim.tracers.num_particles, "advect_ms": adv, "redistribute_ms": red,
           "advect_ns_per_particle": adv * 1e6 / max(sim.tracers.num_particles, 1), "step_with_tracers_ms": ms_with, "step_with_tracers_ms_all": w,
           "operator_step_without_tracers_ms": ms_without, "operator_step_without_tracers_ms_all": wo, "advect_over_operator_step": adv / ms_without}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


L.qk_profile_only(ctx.h, None)
rows = [sample("from step 1, cell order")]  # (the first step also pays the first allocations of the operator path: hence medians)
while sim.istep < steps:
    assert sim.step()
rows.append(sample(f"after {steps} steps"))
print(json.dumps({"path": "fused stages, exact form" if fused_stages else "operators", "n": n, "boxes": sim.lev.nboxes, "particles_at_start": np0, "samples": rows}))
