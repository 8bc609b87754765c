"""Cost of one DiagPDF output (csrc/qk_diag.hip, quokka_amd/diagnostics.py) on one level, of the shape of the reference's `hist1`
(tests/golden/ShockCloud_diag.in): two log-spaced derived variables of 50 bins each, mass-weighted.  The state is the Sedov blast of bench.py after ten
steps (nearly every cell in one bin), then density and energy spread log-uniformly over the deck's ranges (every bin filled); n^3 cells in boxes of 128^3 (default n = 128 and 256, i.e. one box and eight boxes); `temperature` and `nH` are stand-ins derived from the
energy per mass and the density, scaled into the deck's ranges.  HIP-event medians of `reps` = 5:
  whole     DiagPDF.process with the derived variables already computed (what an output costs once the fields exist)
  keys      the key kernel (qk_diag_keys)
  sort      torch.sort(stable=True) of the keys + torch.searchsorted of the 2501 bin edges
  segsum    the passes of the segment sum: block tables (torch) + qk_diag_segsum
  rest      the level's sum into the histogram and the copy to the host
(each part timed alone, ended by a synchronise: where the host enqueues ahead of the GPU in the whole run, the parts add up to more than `whole`)
  derived   filling the two derived MultiFabs with torch operations (the problem's hook, not part of the library)
  step      one fused hydro step (RK2) of the same state
Writes README.md and diag_pdf_time.json into --out (default profiles/diag_pdf) and prints the JSON line.
     python profiles/tools/diag_pdf_time.py [--out DIR] [n ...]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from quokka_amd import diagnostics  # noqa: E402
from quokka_amd.multifab import Context  # noqa: E402
from quokka_amd.simulation import sedov_problem  # noqa: E402

args = sys.argv[1:]
out_dir = os.path.join(ROOT, "profiles", "diag_pdf")
if "--out" in args:
    k = args.index("--out")
    out_dir = args[k + 1]
    del args[k:k + 2]
sizes = [int(a) for a in args] or [128, 256]
reps = 5
ctx = Context(0)


def med(v):
    return sorted(v)[len(v) // 2]


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def derived(L, name, out):
    for b in range(L.lev.nboxes):
        U = L.state_new_cc_.valid(b)
        if name == "nH":
            out.valid(b)[0].copy_(U[0])
        else:
            out.valid(b)[0].copy_(U[4] / U[0] * 1.0e8)  # (the ambient gas lands near 1e3 .. 1e4, the hot bubble above)


PARAMS = {"quokka.diagnostics": "hist1", "quokka.hist1.type": "DiagPDF", "quokka.hist1.int": 20, "quokka.hist1.weight_by": "mass",
          "quokka.hist1.var_names": "temperature nH", "quokka.hist1.temperature.nBins": 50, "quokka.hist1.temperature.log_spaced_bins": 1,
          "quokka.hist1.temperature.range": "1e2 1e8", "quokka.hist1.nH.nBins": 50, "quokka.hist1.nH.log_spaced_bins": 1, "quokka.hist1.nH.range": "1e-3 1e3"}


def measure(sim, d, state, step):
    n = sim.geom.n_cell[0]
    fields = diagnostics.compute_fields(sim, [sim], sim.m_diagVars)  # (also the warm-up of the derived fill)
    der = [events(lambda: diagnostics.compute_fields(sim, [sim], sim.m_diagVars)) for _ in range(reps)]
    field_list = [fields[nm][0] for nm in d._field_order()]
    pdf = d.process(sim, fields)  # (warm-up: allocations, the sort's work space)
    whole = [events(lambda: d.process(sim, fields)) for _ in range(reps)]
    keys_t, sort_t, seg_t, rest_t = [], [], [], []
    bins = torch.arange(d.total_bins + 1, dtype=torch.int64, device=ctx.device)
    zeros = torch.zeros(d.total_bins, dtype=torch.float64, device=ctx.device)
    for _ in range(reps + 1):
        box = {}
        keys_t.append(events(lambda: box.update(kw=d.level_keys_weights(sim, field_list, None))))
        keys, weights = box["kw"]

        def sort():
            sk, perm = torch.sort(keys, stable=True)
            box["perm"], box["off"] = perm, torch.searchsorted(sk, bins)
        sort_t.append(events(sort))
        seg_t.append(events(lambda: box.update(seg=diagnostics.segment_sums(ctx, weights, box["perm"], box["off"], d.total_bins))))
        rest_t.append(events(lambda: (zeros + diagnostics.bin_sums(*box["seg"])).cpu()))
    keys_t, sort_t, seg_t, rest_t = keys_t[1:], sort_t[1:], seg_t[1:], rest_t[1:]
    return {"n": n, "state": state, "boxes": sim.lev.nboxes, "cells": n ** 3, "bins": d.total_bins, "bins_filled": int((pdf != 0.0).sum()),
            "cells_taking_part": int((box["kw"][0] < d.total_bins).sum().item()), "fullest_bin_cells": int(torch.bincount(box["kw"][0])[:d.total_bins].max().item()),
            "passes": diagnostics.num_passes(n ** 3), "whole_ms": med(whole), "keys_ms": med(keys_t), "sort_ms": med(sort_t), "segsum_ms": med(seg_t),
            "rest_ms": med(rest_t), "derived_ms": med(der), "step_ms": med(step) if step else None, "spread_whole_ms": [min(whole), max(whole)],
            "spread_step_ms": [min(step), max(step)] if step else None}


def one(n):
    sim = sedov_problem(ctx, n, max_grid_size=128)
    for _ in range(10):
        assert sim.step()
    step = [events(lambda: sim.step()) for _ in range(reps)]
    sim.derivedNames_, sim.ComputeDerivedVar = ["temperature", "nH"], derived
    sim.createDiagnostics(PARAMS)
    d = sim.m_diagnostics[0]
    out = [measure(sim, d, "blast", step)]
    # the same lattice with density and energy spread over the deck's ranges, so that every bin is filled (not a state the hydro could advance)
    gen = torch.Generator(device=ctx.device).manual_seed(n)
    for b in range(sim.lev.nboxes):
        U = sim.state_new_cc_.valid(b)
        U[0].copy_(10.0 ** (6.0 * torch.rand(U[0].shape, dtype=torch.float64, device=ctx.device, generator=gen) - 3.0))
        U[4].copy_(U[0] * 10.0 ** (6.0 * torch.rand(U[0].shape, dtype=torch.float64, device=ctx.device, generator=gen) - 6.0))
    out.append(measure(sim, d, "spread", None))
    return out


runs = [r for n in sizes for r in one(n)]
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "diag_pdf_time.json"), "w") as f:
    f.write(json.dumps({"runs": runs}) + "\n")
lines = ["# DiagPDF histograms: measured cost (`csrc/qk_diag.hip`, DESIGN.md §15)", "",
         "One MI355X, `python profiles/tools/diag_pdf_time.py " + " ".join(str(n) for n in sizes) + "` (`diag_pdf_time.json` is its output; this file is written by",
         "the tool).  One output of the shape of the reference's `hist1`: two log-spaced derived variables of 50 bins, mass-weighted, on one level of n³ cells",
         "in boxes of 128³.  State `blast`: the Sedov blast of `bench.py` after ten steps, where nearly every cell falls into ONE bin (the ambient gas); state",
         "`spread`: density and energy per mass drawn log-uniformly over the deck's ranges, every bin filled.  HIP-event times, medians of five (smallest and",
         "largest of the whole output and of the step in brackets).  `whole` is `DiagPDF.process` with the derived variables computed.  Its parts, each",
         "measured ALONE between two events and ended by a synchronise: `keys` the key kernel; `sort` the stable `torch.sort` of the keys and the",
         "`torch.searchsorted` of the bin edges; `segsum` the passes of the segment sum with the torch operations that build their block tables; `rest` the",
         "level's sum into the histogram and its copy to the host.  The parts add up to more than `whole` where the host enqueues ahead of the GPU in the whole",
         "run and cannot when a part is timed alone — `segsum` is some forty small launches, bound by the host.  `derived` is the problem's hook that fills the",
         "two derived arrays with torch operations; `step` one fused RK2 hydro step of the blast.  No threshold was set for this change: the figures are",
         "here so that the next change has something to compare against.", "",
         "| cells | boxes | state | cells taking part | bins filled | fullest bin | passes | whole | keys | sort | segsum | rest | derived | step |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
for r in runs:
    step = f"{r['step_ms']:.3f} ms ({r['spread_step_ms'][0]:.3f} … {r['spread_step_ms'][1]:.3f})" if r["step_ms"] is not None else "–"
    lines.append(f"| {r['n']}³ | {r['boxes']} | {r['state']} | {r['cells_taking_part']} | {r['bins_filled']} of {r['bins']} | {r['fullest_bin_cells']} | {r['passes']} | "
                 f"{r['whole_ms']:.3f} ms ({r['spread_whole_ms'][0]:.3f} … {r['spread_whole_ms'][1]:.3f}) | {r['keys_ms']:.3f} ms | {r['sort_ms']:.3f} ms | "
                 f"{r['segsum_ms']:.3f} ms | {r['rest_ms']:.3f} ms | {r['derived_ms']:.3f} ms | {step} |")
lines += ["", "With `int = 20`, as in the deck, one output is paid once per twenty steps.", "",
          "`resources_result.txt`: `profiles/tools/resource_usage.py qk_diag.hip` — the six new kernels; none uses scratch memory and all reach 8 waves per SIMD.",
          "No other `.hip` file is changed, so the tables of `profiles/cic/resources_result.txt` and `profiles/gravity/resources_result.txt` stand for the rest.", ""]
with open(os.path.join(out_dir, "README.md"), "w") as f:
    f.write("\n".join(lines))
print(json.dumps({"runs": runs}))
