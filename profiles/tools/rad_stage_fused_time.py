#!/usr/bin/env python3
"""ms per call of qk_rad_stage_fused on one N^3 box (default 128) with NG photon groups (default 4), stages 1 and 2 (in place), order 3, on a valid
random state with a floor: prints one JSON line.  Same-box A/B of two builds: run it once per library with QK_LIB_PATH, interleaved.
    python profiles/tools/rad_stage_fused_time.py [N NG reps]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from quokka_amd import capi  # noqa: E402
from quokka_amd.multifab import Context, Level, MultiFab  # noqa: E402
from quokka_amd.radhydro import _d3  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 128
NG = int(sys.argv[2]) if len(sys.argv) > 2 else 4
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
c, chat = 2.99792458e10, 2.99792458e9
ctx = Context(0)
lev = Level(ctx, 3, [([0, 0, 0], [N - 1] * 3)])
rt = capi.RadTraits(c, chat, 7.5657e-15, 1.0e-3, 1, 0, 1.0, 1.0, 1.0, 1, 0)
rt.ngroups = NG
rng = np.random.default_rng(1)
shp = (N + 8,) * 3
U = np.zeros((6 + 4 * NG,) + shp)
U[0], U[4], U[5] = 1.0, 1.0, 1.0
for g in range(NG):
    E = rng.uniform(1.0, 2.0, shp)
    U[6 + 4 * g] = E
    for a in range(3):
        U[7 + 4 * g + a] = rng.uniform(-0.3, 0.3, shp) * c * E
U0, U1 = MultiFab(lev, 6 + 4 * NG, 4), MultiFab(lev, 6 + 4 * NG, 4)
U0.set_fab(0, U)
acc = MultiFab(lev, 4 * NG, 0)
dt, dx = 0.3 / chat, _d3([1.0, 1.0, 1.0])
out = {"N": N, "ngroups": NG, "lib": os.path.basename(os.path.dirname(os.path.dirname(capi.LIB_PATH))) + "/" + os.path.basename(capi.LIB_PATH)}


def stage(n):
    if n == 1:
        ctx.check(ctx.L.qk_rad_stage_fused(lev.h, ctx.stream(), C.byref(rt), 3, 1, U0.ptr, U0.ptr, U1.ptr, acc.ptr, None, dt, dx, None), "stage 1")
    else:
        ctx.check(ctx.L.qk_rad_stage_fused(lev.h, ctx.stream(), C.byref(rt), 3, 2, U1.ptr, U0.ptr, U1.ptr, acc.ptr, None, dt, dx, None), "stage 2")


for n in (1, 2):
    U1.copy_from(U0)
    for _ in range(3):
        stage(n)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        stage(n)
    t1.record()
    torch.cuda.synchronize()
    out[f"stage{n}_ms"] = round(t0.elapsed_time(t1) / reps, 4)
print(json.dumps(out))
