"""The path bench.py times — the carried form of the RK2 average (rk2_carry_rhs = 1), the X sweep folded into the Y march (QK_FUSEX, k_sweep_xy), the
primitive hand-off between the stages — against the CPU oracle's carried form (oracle/hydro_sim.hpp HydroSim::rk2_carry_rhs, the kernel's formula
restated), in EVERY bit and every dt — the state after the steps and the half step the last stage 1 stored (S = U_old + (dt/2) r_1 and
P(U_old): a one-ulp error in the stored pressure moves the P dV term of the auxiliary internal energy far below that energy's last bit, and
SyncDualEnergy overwrites it in most cells, so the state alone cannot show it).  The other carried tests compare HIP with HIP, or hold the carried form to the exact one within 1e-12 relative
L1, which lets a wrong pressure in one P dV term or a wrong wave-edge face in a few rows through; these do not.

Each oracle run is computed once for the module and compared with every GPU variant of it: the carried oracle does not depend on the box layout
(tests/test_oracle_carried_cpu.py::test_carried_form_does_not_depend_on_the_box_layout)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import SCALARS, SEDOV
from quokka_amd.simulation import developed_state, sedov_problem

pytestmark = pytest.mark.gpu
NO_FOFC = {"fofc1_cells": 0, "fofc2_cells": 0, "retries": 0, "carry2_fallbacks": 0}


def gather(boxes, vals, n_cell, nc):
    U = np.zeros((nc, n_cell[2], n_cell[1], n_cell[0]))
    for (lo, hi), v in zip(boxes, vals):
        U[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = v
    return U


def gather_oracle(so, n_cell):
    return gather([so.box(b) for b in range(so.nboxes)], [so.valid(b) for b in range(so.nboxes)], n_cell, so.ncomp)


def gather_gpu(sg, n_cell):
    return gather(sg.my_boxes, sg.gather_valid_local(), n_cell, sg.state_new_cc_.ncomp)


def half_oracle(so, n_cell):
    """S = U_old + (dt/2) r_1 and P(U_old) as the last carried stage 1 stored them"""
    return gather([so.box(b) for b in range(so.nboxes)], [so.carry_half(b) for b in range(so.nboxes)], n_cell, so.ncomp + 1)


def half_gpu(sg, n_cell):
    return gather(sg.my_boxes, [sg.rhs1().valid(b).cpu().numpy() for b in range(sg.lev.nboxes)], n_cell, sg.hydro.nvar_ + 1)


def assert_same(Ug, Uo, what):
    if not np.array_equal(Ug, Uo):
        bad = np.argwhere(Ug != Uo)
        n, k, j, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} values differ; first at component {n}, cell (i, j, k) = ({i}, {j}, {k}): "
                             f"{Ug[n, k, j, i]!r} (GPU) vs {Uo[n, k, j, i]!r} (oracle); max abs diff {np.abs(Ug - Uo).max():.3e}")


class fusex:
    """QK_FUSEX for the launches inside the block (the kernel reads it per launch), restored afterwards"""

    def __init__(self, on):
        self.value = "1" if on else "0"

    def __enter__(self):
        self.old = os.environ.get("QK_FUSEX")
        os.environ["QK_FUSEX"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("QK_FUSEX", None)
        else:
            os.environ["QK_FUSEX"] = self.old


class kernel_counts:
    """launches per kernel inside the block, from the library's own kernel profile (qk_profile_*, as bench.py read_profile)"""

    def __init__(self, ctx):
        self.ctx, self.counts = ctx, {}

    def __enter__(self):
        L, h = self.ctx.L, self.ctx.h
        L.qk_profile_reset(h)
        L.qk_profile_only(h, None)
        L.qk_profile_enable(h, 1)
        return self

    def __exit__(self, *exc):
        L, h = self.ctx.L, self.ctx.h
        try:
            for k in range(L.qk_profile_num_kernels(h)):
                name, cnt, ms = C.c_char_p(), C.c_long(), C.c_double()
                L.qk_profile_get(h, k, C.byref(name), C.byref(cnt), C.byref(ms))
                self.counts[name.value.decode()] = self.counts.get(name.value.decode(), 0) + cnt.value
        finally:
            L.qk_profile_enable(h, 0)
            L.qk_profile_reset(h)

    def __getitem__(self, name):
        return self.counts.get(name, 0)


@pytest.fixture(scope="module")
def carried():
    """the module's oracle runs, each computed once: carried(key, make) -> make()'s result"""
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    return get


def oracle_carried(oracle, n, n_cell, nsteps, mgs, developed=False, order=-1):
    """the carried oracle on the geometry of sedov_problem(ctx, n, n_cell=n_cell): (state, dt of every step, the last stored half step)"""
    so = oracle.sim(SEDOV, 3, list(n_cell), [0, 0, 0], [1.2 * c / n for c in n_cell], [0, 0, 0], max_grid_size=list(mgs), reconstruction_order=order)
    so.set_rk2_carry_rhs(True)
    if developed:
        for b in range(so.nboxes):
            lo, hi = so.box(b)
            so.set_state(developed_state(n, lo, hi), b, 0)
    dts = []
    for it in range(nsteps):
        assert so.step(), f"oracle advance failed at step {it}"
        dts.append(so.dt)
    assert so.counters() == NO_FOFC, so.counters()
    return gather_oracle(so, n_cell), dts, half_oracle(so, n_cell)


def two_width_level(ctx):
    """192 x 64 x 64 cells in a 128-wide and a 64-wide box (tests/test_hydro_step_gpu.py::test_x_sweep_inside_the_y_march_with_boxes_of_two_widths)"""
    from quokka_amd import capi
    from quokka_amd.simulation import Geometry, HydroSimulation
    geom = Geometry(3, [192, 64, 64], [0.0, 0.0, 0.0], [3.6, 1.2, 1.2], [0, 0, 0])
    bcs = []
    for c in range(6):
        lo = [capi.BC_REFLECT_ODD if c == 1 + d else capi.BC_REFLECT_EVEN for d in range(3)]
        bcs.append((lo, list(lo)))
    boxes = [([0, 0, 0], [127, 63, 63]), ([128, 0, 0], [191, 63, 63])]
    s = HydroSimulation(ctx, geom, capi.traits(1.4, False, 3), bcs, [128, 64, 64], boxes=boxes, owner=[0, 0])
    s.reconstructionOrder_, s.stopTime_, s.cflNumber_ = 3, 1.0, 0.3
    assert sorted({hi[0] - lo[0] + 1 for lo, hi in s.my_boxes}) == [64, 128]
    return s


def gpu_carried(ctx, n, n_cell, nsteps, mgs, developed=False, fusex_on=True, order=3, level=None):
    """the GPU path in the carried form with the hand-off on: (sim, dt of every step, launches per kernel)"""
    with fusex(fusex_on):
        sg = level if level is not None else sedov_problem(ctx, n, max_grid_size=mgs, n_cell=list(n_cell))
        sg.rk2_carry_rhs = True
        sg.prim_handoff = True
        sg.reconstructionOrder_ = order
        if developed:
            for b, (lo, hi) in enumerate(sg.my_boxes):
                sg.state_new_cc_.set_fab(b, developed_state(n, lo, hi))
            sg._signal_of_state_new = None
        assert sg._prim_handoff_applies()
        dts = []
        with kernel_counts(ctx) as prof:
            for it in range(nsteps):
                assert sg.step(), f"GPU advance failed at step {it}"
                dts.append(sg.dt_)
    assert sg.counters.get("prim_handoff_dropped", 0) == 0
    assert sg.counters["fofc1_stages"] == sg.counters["fofc2_stages"] == sg.counters["retries"] == 0, sg.counters
    return sg, dts, prof


def assert_sweeps(prof, nsteps, fusex_on):
    """the X sweep ran inside the Y march (k_sweep_xy, once per stage) or as launches of its own — and nothing else"""
    if fusex_on:
        assert (prof["k_sweep_xy"], prof["k_sweep_x"], prof["k_sweep_y"]) == (2 * nsteps, 0, 0), prof.counts
    else:
        assert (prof["k_sweep_xy"], prof["k_sweep_x"], prof["k_sweep_y"]) == (0, 2 * nsteps, 2 * nsteps), prof.counts
    assert prof["k_sweep_z"] == 2 * nsteps, prof.counts


@pytest.mark.parametrize("fusex_on", [True, False])
@pytest.mark.parametrize("N,nsteps", [(128, 4), (256, 3)])
def test_headline_geometry_equals_the_carried_oracle(ctx, oracle, carried, N, nsteps, fusex_on):
    """128^3 boxes (one at 128^3, eight at 256^3) from the developed blast — a Mach-3 shell crossing wave edges, 32-row batches, march segments and
    box faces, every limiter and HLLC fan active —, carried form, hand-off on, with the X sweep inside the Y march and without it"""
    Uo, dto, Ho = carried(("developed", N), lambda: oracle_carried(oracle, N, [N] * 3, nsteps, [128] * 3, developed=True))
    sg, dts, prof = gpu_carried(ctx, N, [N] * 3, nsteps, 128, developed=True, fusex_on=fusex_on)
    assert sg.lev.nboxes == (N // 128) ** 3
    assert_sweeps(prof, nsteps, fusex_on)
    assert dts == dto, (dts, dto)
    assert Uo[0].max() > 2.0 and Uo[0].min() < 1.1  # (the state is developed)
    assert_same(gather_gpu(sg, [N] * 3), Uo, f"{N}^3, QK_FUSEX={int(fusex_on)}")
    assert_same(half_gpu(sg, [N] * 3), Ho, "the stored half step")


@pytest.mark.parametrize("mgs", [128, 64])
def test_what_bench_times_equals_the_carried_oracle(ctx, oracle, carried, mgs):
    """bench.py's headline workload as it runs it: Sedov initial conditions, carried form, hand-off on, QK_FUSEX on, its 3 warm-up + 20 timed steps —
    at 128^3 in boxes of 128 and of 64 cells (both whole 64-cell waves wide)"""
    Uo, dto, Ho = carried("bench128", lambda: oracle_carried(oracle, 128, [128] * 3, 23, [64] * 3))
    sg, dts, prof = gpu_carried(ctx, 128, [128] * 3, 23, mgs)
    assert sg.lev.nboxes == (128 // mgs) ** 3
    assert_sweeps(prof, 23, True)
    assert dts == dto, (dts, dto)
    assert_same(gather_gpu(sg, [128] * 3), Uo, f"128^3 in {mgs}^3 boxes, 23 steps")
    assert_same(half_gpu(sg, [128] * 3), Ho, "the stored half step")


def test_fusex_with_boxes_of_two_widths_equals_the_carried_oracle(ctx, oracle):
    """192 x 64 x 64 cells chopped at 128: the fused launch is sized for the 128-wide box, the chunk beyond the 64-wide one leaves at once; 5 steps from
    the developed blast"""
    n_cell = (192, 64, 64)
    Uo, dto, Ho = oracle_carried(oracle, 64, n_cell, 5, n_cell, developed=True)
    sg, dts, prof = gpu_carried(ctx, 64, n_cell, 5, None, developed=True, level=two_width_level(ctx))
    assert_sweeps(prof, 5, True)
    assert dts == dto, (dts, dto)
    assert_same(gather_gpu(sg, n_cell), Uo, "192 x 64 x 64 in boxes 128 and 64 wide")
    assert_same(half_gpu(sg, n_cell), Ho, "the stored half step")


@pytest.mark.parametrize("shape", [(64, 8, 8), (64, 24, 40), (128, 40, 24), (64, 72, 8), (192, 8, 56), (64, 16, 136)])
def test_fusex_on_boxes_of_odd_heights_equals_the_carried_oracle(ctx, oracle, shape):
    """one box of 8, 24, 40, 72 ... rows: fewer rows than one batch of wave-edge faces, a last batch that is not full, marches shorter than one
    segment; 4 steps from the developed blast"""
    Uo, dto, Ho = oracle_carried(oracle, 64, shape, 4, shape, developed=True)
    sg, dts, prof = gpu_carried(ctx, 64, shape, 4, list(shape), developed=True)
    assert sg.lev.nboxes == 1
    assert_sweeps(prof, 4, True)
    assert dts == dto, (dts, dto)
    assert_same(gather_gpu(sg, shape), Uo, f"box {shape}")
    assert_same(half_gpu(sg, shape), Ho, "the stored half step")


def test_flagged_steps_on_the_fusex_path_equal_the_carried_oracle(ctx, oracle):
    """64^3 in one box, carried form, hand-off on, QK_FUSEX on: 3 steps, one step at 6x the CFL step, 3 steps.  The over-CFL step drops the hand-off,
    corrects stage 1 (S keeps the uncorrected r_1), redoes a flagged carried stage 2 in the exact form (its own first pass, then its correction) and
    is retried with 2, 4 and 8 substeps — every bit of the carried oracle after that step and at the end"""
    N = 64
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[N] * 3)
    so.set_rk2_carry_rhs(True)
    with fusex(True):
        sg = sedov_problem(ctx, N, max_grid_size=N)
        sg.rk2_carry_rhs = True
        sg.prim_handoff = True
        assert sg._prim_handoff_applies()
        for it in range(3):
            assert so.step() and sg.step()
            assert so.dt == sg.dt_, it
        dt = so.compute_dt() * 6.0
        with kernel_counts(ctx) as prof:
            assert so.advance_fixed_dt(dt) and sg.step(dt)
        co = so.counters()
        assert co["fofc1_cells"] > 0 and co["carry2_fallbacks"] > 0 and co["retries"] > 0, co
        assert sg.counters["fofc1_stages"] > 0 and sg.counters["fofc2_stages"] > 0, sg.counters
        assert sg.counters["retries"] == co["retries"] and sg.counters["prim_handoff_dropped"] > 0, (sg.counters, co)
        assert prof["k_sweep_xy"] > 0, prof.counts  # (the clean substeps ran on the fused X + Y march)
        assert_same(gather_gpu(sg, [N] * 3), gather_oracle(so, [N] * 3), "after the over-CFL step")
        assert_same(half_gpu(sg, [N] * 3), half_oracle(so, [N] * 3), "the half step the over-CFL step stored last")
        for it in range(3):
            assert so.step() and sg.step()
            assert so.dt == sg.dt_, it
    assert_same(gather_gpu(sg, [N] * 3), gather_oracle(so, [N] * 3), "3 steps later")
    assert_same(half_gpu(sg, [N] * 3), half_oracle(so, [N] * 3), "the stored half step, 3 steps later")


@pytest.mark.parametrize("order", [2, 1])
def test_lower_orders_equal_the_carried_oracle(ctx, oracle, order):
    """PLM and donor cell in the carried form (k_sweep_x + the marching sweeps: 16-cell boxes are no whole wave wide), Sedov 32^3 in 16^3 boxes, 10 steps"""
    Uo, dto, Ho = oracle_carried(oracle, 32, [32] * 3, 10, [16] * 3, order=order)
    sg, dts, prof = gpu_carried(ctx, 32, [32] * 3, 10, 16, order=order)
    assert_sweeps(prof, 10, False)
    assert dts == dto, (dts, dto)
    assert_same(gather_gpu(sg, [32] * 3), Uo, f"reconstruction order {order}")
    assert_same(half_gpu(sg, [32] * 3), Ho, "the stored half step")


@pytest.mark.parametrize("nscalars", [1, 2])
def test_passive_scalars_equal_the_carried_oracle(ctx, oracle, nscalars):
    """the carried form with passive scalars (NS > 0: the X sweep is never folded into the march there), on the PassiveScalar problem's 3-D geometry
    (32 x 16 x 16 cells in 16^3 boxes, as tests/test_hydro_step_gpu.py::test_passive_scalars_match_oracle), 10 steps, every component"""
    from quokka_amd.simulation import scalar_contact_problem
    n_cell, mgs = [32, 16, 16], [16, 16, 16]
    so = oracle.sim(SCALARS, 3, n_cell, [0, 0, 0], [1.0, 1.0, 1.0], [1, 1, 1], max_grid_size=mgs, nscalars=nscalars)
    so.set_rk2_carry_rhs(True)
    with fusex(True):
        sg = scalar_contact_problem(ctx, n_cell[0], nscalars=nscalars, ndim=3, max_grid_size=mgs)
        sg.rk2_carry_rhs = True
        assert sg._carry_active() and sg.state_new_cc_.ncomp == 6 + nscalars
        for b in range(so.nboxes):
            sg.state_new_cc_.set_fab(b, so.state(b, 0))
            sg.state_old_cc_.set_fab(b, so.state(b, 1))
        with kernel_counts(ctx) as prof:
            for it in range(10):
                assert so.step() and sg.step()
                assert so.dt == sg.dt_, it
    assert prof["k_sweep_x"] == 20 and prof["k_sweep_xy"] == 0, prof.counts
    assert so.counters() == NO_FOFC and sg.counters["fofc1_stages"] == sg.counters["fofc2_stages"] == 0
    assert_same(gather_gpu(sg, n_cell), gather_oracle(so, n_cell), f"{nscalars} passive scalars")
    assert_same(half_gpu(sg, n_cell), half_oracle(so, n_cell), "the stored half step")
    assert float(sg.state_new_cc_.valid(0)[6].max()) > 0.9  # (the scalar's step is still there)


def test_cxx_host_in_the_carried_form_equals_the_carried_oracle(oracle, carried, tmp_path):
    """the C++17 host running the reference's unchanged HydroBlast3D problem file (oracle/_ref) in the carried form: 128^3 in 64^3 boxes, 23 steps,
    hand-off on — the per-box dump, reassembled in chop_domain order, equals the oracle run of test_what_bench_times_equals_the_carried_oracle"""
    from quokka_amd.simulation import chop_domain
    from test_reference_problems_gpu import exe
    Uo, dto, Ho = carried("bench128", lambda: oracle_carried(oracle, 128, [128] * 3, 23, [64] * 3))
    dump = str(tmp_path / "state.bin")
    cmd = [exe("ref_HydroBlast3D"), "geometry.prob_lo=0 0 0", "geometry.prob_hi=1.2 1.2 1.2", "geometry.is_periodic=0 0 0", "amr.n_cell=128 128 128",
           "amr.max_grid_size=64", "max_timesteps=23", "hydro.rk2_carry_rhs=1", f"qk.dump_state={dump}"]
    env = dict(os.environ, QK_FUSEX="1")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    out = p.stdout + p.stderr
    assert os.path.exists(dump), out[-2000:]
    meta = [float(x) for x in open(dump + ".meta").read().split()]
    assert int(meta[0]) == 23 and meta[2] == dto[-1], (meta, dto[-1])
    assert "prim_handoff=1 prim_handoff_dropped=0" in out, out[-2000:]
    data = np.fromfile(dump, dtype=np.float64)
    boxes = chop_domain([128] * 3, [64] * 3)
    assert data.size == 6 * 128 ** 3
    Ug = gather(boxes, data.reshape(len(boxes), 6, 64, 64, 64), [128] * 3, 6)
    assert_same(Ug, Uo, "C++ host, 128^3 in 64^3 boxes, 23 steps")
