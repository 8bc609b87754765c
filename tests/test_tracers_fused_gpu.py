"""Tracer particles on the fused hydro stages: stage 2 of the exact form stores avgFaceVel itself (qk_hydro_stage_args::store_vel_rk2 / velRk2,
HydroSimulation.tracers_on_fused_stages).  The kernels against the reference-shaped operators through the C-ABI, then the driver against a run
with tracers on the default (operator) path.  Every comparison is bit for bit: the fused sweeps and the operators share their device functions."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import tracer_reference as tr
from quokka_amd import capi
from quokka_amd.hydro_system import replaceFluxes
from quokka_amd.multifab import MultiFab
from quokka_amd.simulation import Geometry, HydroSimulation, sedov_problem
from test_tracers_gpu import download_faces, record_advects, ref_geom, replay

pytestmark = pytest.mark.gpu
GAMMA = 1.4
DT = 1.0e-3


# ---------------------------------------------------------------------- helpers
def fused_source_constants():
    """(cells an x-sweep tile updates, lanes of a marching wave) as csrc/qk_hydro_fused.hip defines them"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "csrc", "qk_hydro_fused.hip")).read()
    xb = int(re.search(r"#define QK_XB (\d+)", src).group(1))
    halo = int(re.search(r"constexpr int XOUT = XB - (\d+);", src).group(1))
    wave = int(re.search(r"dim3\((\d+), MARCH_BY\)", src).group(1))
    return xb - halo, wave


def smooth_state(n_cell, ndim, nscalars, seed):
    """a random smooth positive state on the whole (periodic) domain, conserved variables [comp, k, j, i]: one Fourier mode per variable and
    direction with random phases, amplitudes well inside positivity, plus 1 % noise so that no two faces carry the same numbers"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = n_cell[2], n_cell[1], n_cell[0]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    x = [(i + 0.5) / nx, (j + 0.5) / ny, (k + 0.5) / nz]

    def wave(amp):
        f = np.zeros(i.shape)
        for d in range(ndim):
            f = f + np.sin(2.0 * np.pi * (x[d] + rng.uniform()))
        return amp * f / ndim + 0.01 * rng.uniform(-1.0, 1.0, size=i.shape)

    rho = 1.0 + wave(0.3)
    v = [wave(0.4) for _ in range(3)]
    P = 1.0 + wave(0.3)
    U = np.zeros((6 + nscalars, nz, ny, nx))
    U[0] = rho
    for d in range(3):
        U[1 + d] = rho * v[d]
    U[5] = P / (GAMMA - 1.0)
    U[4] = U[5] + 0.5 * rho * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    for n in range(nscalars):
        U[6 + n] = rho * (0.5 + wave(0.4))
    return U


def make_sim(ctx, ndim, n_cell, mgs, nscalars=0, seed=5):
    n_cell = (list(n_cell) + [1, 1])[:3]
    geom = Geometry(ndim, n_cell, [0.0] * 3, [1.0] * 3, [1 if d < ndim else 0 for d in range(3)])
    nc = 6 + nscalars
    bcs = [([capi.BC_INT_DIR] * 3, [capi.BC_INT_DIR] * 3) for _ in range(nc)]
    sim = HydroSimulation(ctx, geom, capi.traits(GAMMA, False, ndim, nscalars=nscalars), bcs, (list(mgs) + [1, 1])[:3], ncomp_cc=nc)
    assert sim.use_fused
    U0 = smooth_state(n_cell, ndim, nscalars, seed)
    sim.set_initial_conditions(lambda i, j, k: U0[:, k, j, i])
    return sim


def face_arrays(sim, fill=float("nan")):
    return [MultiFab(sim.lev, 1, 0, facedir=d, fill=fill) for d in range(sim.geom.ndim)]


def stage_args(sim, stage, U_in, U_old, U_out, dt, store_vel=0, vel=None, fofc=0, carry=0):
    """qk_hydro_stage_args of an exact-form (carry = 0) stage over all boxes, built here field by field: reports in slot 0 of the simulation's words"""
    a = capi.StageArgs()
    a.U_in, a.U_old, a.U_out = U_in.ptr, U_old.ptr, U_out.ptr
    nd = sim.geom.ndim
    for d in range(3):
        a.halfFlux[d] = sim.halfFlux[d].ptr if d < nd else None
        a.halfVel[d] = sim.halfVel[d].ptr if d < nd else None
        a.dx[d] = sim.geom.dx[d] if d < nd else 1.0
        a.velRk2[d] = vel[d].ptr if (vel is not None and d < nd and vel[d] is not None) else None
    a.redoFlag = sim.redoFlag.ptr
    w = sim._dev_words.data_ptr()
    a.d_redo_count, a.d_error_flag = C.c_void_p(w + 16), C.c_void_p(w + 24)
    if stage == 2:
        a.d_max_signal = C.c_void_p(w)
    a.scratch, a.scratch_bytes = C.c_void_p(sim.scratch.data_ptr()), sim.scratch.numel() * 8
    a.dt, a.stage, a.reconstruction_order = dt, stage, 3
    a.densityFloor, a.tempFloor, a.use_dual_energy, a.K_visc = 0.0, 0.0, 1, 0.0
    a.store_vel_rk2, a.fofc_pass, a.rk2_carry_rhs = store_vel, fofc, carry
    if carry:
        a.rhs1 = sim.rhs1().ptr
    return a


def launch(sim, a) -> int:
    """the stage; returns the count of flagged (correction pass: still invalid) cells; raises capi.QkError where the library refuses"""
    c = sim.ctx
    sim._fused_begin(a.stage)
    c.check(c.L.qk_hydro_stage_fused(sim.lev.h, c.stream(), C.byref(sim.traits), C.byref(a)), "qk_hydro_stage_fused")
    return sim._fused_end(a.stage)


def fabs(mfs, sim):
    return [[mf.fab_numpy(b).copy() for b in range(sim.lev.nboxes)] for mf in mfs]


class FirstPass:
    """stage 1 and stage 2 (first pass, store_vel_rk2) of one state on the fused kernels, and what the operators give for the same stage 2"""

    def __init__(self, ctx, ndim, n_cell, mgs, nscalars=0):
        sim = self.sim = make_sim(ctx, ndim, n_cell, mgs, nscalars)
        old, inter, new = sim.state_old_cc_, sim.state_inter_cc_, sim.state_new_cc_
        sim.fillBoundaryConditions(old)
        assert launch(sim, stage_args(sim, 1, old, old, inter, DT)) == 0, "the state must not flag cells"
        self.v1 = fabs(sim.halfVel, sim)
        sim.fillBoundaryConditions(inter)
        self.vel = face_arrays(sim)  # NaN: a face the stage leaves out shows
        assert launch(sim, stage_args(sim, 2, inter, old, new, DT, store_vel=1, vel=self.vel)) == 0
        self.got = fabs(self.vel, sim)
        self.v1_after = fabs(sim.halfVel, sim)
        self.new = [new.valid(b).cpu().numpy() for b in range(sim.lev.nboxes)]
        # the operators on the same intermediate state, as _stage_unfused forms the average: (0 + 0.5 v1) + 0.5 v2, Saxpy by Saxpy
        t = sim._tmp()
        sim.computeHydroFluxes(inter, t["flux"], t["vel"])
        self.v2 = fabs(t["vel"], sim)
        self.want = [[0.5 * a + 0.5 * b for a, b in zip(self.v1[d], self.v2[d])] for d in range(ndim)]


def check_first_pass(fp: FirstPass):
    sim = fp.sim
    for d in range(sim.geom.ndim):
        differs_v1 = differs_v2 = False
        for b in range(sim.lev.nboxes):
            got, want = fp.got[d][b], fp.want[d][b]
            assert np.isfinite(want).all()
            assert np.array_equal(got, want), (d, b, np.argwhere(got != want)[:5].tolist())
            assert np.array_equal(fp.v1_after[d][b], fp.v1[d][b]), f"stage 2 changed halfVel, direction {d}, box {b}"
            differs_v1 = differs_v1 or not np.array_equal(got, fp.v1[d][b])
            differs_v2 = differs_v2 or not np.array_equal(got, fp.v2[d][b])
        assert differs_v1 and differs_v2, f"direction {d}: the average is one stage's own velocity"
        assert any(np.abs(w).max() > 0.0 for w in fp.want[d])
    # the store changes nothing else: the same stage 2 without it leaves the same state
    old, inter, new = sim.state_old_cc_, sim.state_inter_cc_, sim.state_new_cc_
    assert launch(sim, stage_args(sim, 2, inter, old, new, DT)) == 0
    for b in range(sim.lev.nboxes):
        assert np.array_equal(new.valid(b).cpu().numpy(), fp.new[b])


@pytest.fixture(scope="module")
def case16(ctx):
    """3-D 16^3 in 8^3 boxes: box high faces, faces shared by two boxes; shared by the kernel tests (they leave its arrays as they are)"""
    return FirstPass(ctx, 3, [16, 16, 16], [8, 8, 8])


# ---------------------------------------------------------------------- 1. kernel, first pass
def test_first_pass_stores_the_rk2_average_on_every_face_3d(case16):
    assert case16.sim.lev.nboxes == 8
    check_first_pass(case16)


def test_first_pass_on_a_row_longer_than_an_x_sweep_tile(ctx):
    """one box, 264 x 8 x 8: the x extent is more than one x-sweep tile and no whole number of marching waves, so faces are evaluated by two
    tiles (each must find v1 intact and leave one value) and the last wave of the marches is partly idle"""
    xout, wave = fused_source_constants()
    nx = 264
    assert nx > xout and nx % wave != 0 and nx % 64 != 0, (xout, wave)
    fp = FirstPass(ctx, 3, [nx, 8, 8], [nx, 8, 8])
    assert fp.sim.lev.nboxes == 1
    check_first_pass(fp)


def test_first_pass_2d(ctx):
    fp = FirstPass(ctx, 2, [16, 16], [8, 8])
    assert fp.sim.lev.nboxes == 4
    check_first_pass(fp)


def test_first_pass_1d(ctx):
    check_first_pass(FirstPass(ctx, 1, [32], [32]))


def test_first_pass_with_a_passive_scalar(ctx):
    fp = FirstPass(ctx, 3, [16, 16, 16], [8, 8, 8], nscalars=1)
    assert fp.sim.state_new_cc_.ncomp == 7
    check_first_pass(fp)


# ---------------------------------------------------------------------- 2. kernel, correction pass
def test_correction_pass_stores_first_order_velocities_on_the_faces_of_flagged_cells(case16):
    """redoFlag set by hand at three cells of the 16^3 state — one inside a box, one on a box face next to another box, one on a box face at the
    domain edge —: the pass writes EVERY face, the first-pass average with the faces of those cells replaced by the first-order (donor cell + LLF)
    face velocity of the old state, as computeFOHydroFluxes + replaceFluxes(face_ncomp = 1) of _stage_unfused give it"""
    fp, sim = case16, case16.sim
    lev, n = sim.lev, 16
    old, inter, new = sim.state_old_cc_, sim.state_inter_cc_, sim.state_new_cc_
    cells = [(3, 3, 3), (7, 4, 4), (15, 12, 2)]  # (i, j, k)
    sim.redoFlag.storage.zero_()
    for (i, j, k) in cells:
        hit = 0
        for b, (lo, hi) in enumerate(sim.my_boxes):
            if all(lo[d] <= c <= hi[d] for d, c in enumerate((i, j, k))):
                sim.redoFlag.valid(b)[0, k - lo[2], j - lo[1], i - lo[0]] = 1
                hit += 1
        assert hit == 1
    sim._fill_flag_ghosts()  # qk_FillBoundary_local_int on one rank
    vel = face_arrays(sim)
    launch(sim, stage_args(sim, 2, inter, old, new, DT, store_vel=1, vel=vel, fofc=1))
    got = fabs(vel, sim)
    # expected, on the operators
    t = sim._tmp()
    sim.computeFOHydroFluxes(old, t["FOflux"], t["FOvel"])
    want_mf = face_arrays(sim)
    g = ref_geom(sim.geom)
    ndiff = 0
    for d in range(3):
        for b in range(lev.nboxes):
            want_mf[d].set_fab(b, fp.want[d][b])
        replaceFluxes(lev, d, want_mf[d], t["FOvel"][d], sim.redoFlag, 1)
        for b in range(lev.nboxes):
            want = want_mf[d].fab_numpy(b)
            assert np.array_equal(got[d][b], want), (d, b, np.argwhere(got[d][b] != want)[:5].tolist())
            assert np.array_equal(sim.halfVel[d].fab_numpy(b), fp.v1[d][b])
        # faces that differ from the first-pass average, each counted once: the global array without its top plane (face n is face 0)
        now = tr.assemble_faces(g, d, sim.my_boxes, got[d])
        first = tr.assemble_faces(g, d, sim.my_boxes, fp.want[d])
        ndiff += int((np.take(now, range(n), axis=2 - d) != np.take(first, range(n), axis=2 - d)).sum())
    print(f"faces replaced: {ndiff}")
    assert 0 < ndiff <= 3 * 6


# ---------------------------------------------------------------------- driver
def record_sources(sim):
    """wrap sim.tracers.advect: which arrays every call was handed"""
    src = []
    inner = sim.tracers.advect

    def advect(umac, dt):
        tmp = sim._unfused_tmp
        src.append("velRk2" if umac is getattr(sim, "_velRk2", None) else "rk2vel" if (tmp is not None and umac is tmp["rk2vel"]) else "other")
        inner(umac, dt)

    sim.tracers.advect = advect
    return src


def tracer_sedov(ctx, on_fused, **attrs):
    sim = sedov_problem(ctx, 16, max_grid_size=8)
    assert sim.use_fused and sim.tracers_on_fused_stages == 0
    for k, v in attrs.items():
        setattr(sim, k, v)
    sim.do_tracers = 1
    sim.tracers_on_fused_stages = int(on_fused)
    sim.InitTracerParticles()
    return sim


def same_state(a, b):
    return all(torch.equal(a.state_new_cc_.valid(n), b.state_new_cc_.valid(n)) for n in range(a.lev.nboxes))


def same_calls(ca, cb):
    assert len(ca) == len(cb), (len(ca), len(cb))
    for n, ((ua, dta), (ub, dtb)) in enumerate(zip(ca, cb)):
        assert dta == dtb, (n, dta, dtb)
        for d in range(len(ua)):
            assert np.array_equal(ua[d], ub[d]), (n, d)


def test_driver_sedov_on_the_fused_stages_equals_the_operator_path(ctx):
    """Sedov 16^3 in 8^3 boxes, 5 steps with tracers_on_fused_stages = 1 against a run with tracers on the default path: dt, state, the face
    arrays handed to AdvectWithUmac and the positions at every step; no stage of the fused run went to the reference-shaped operators; the
    positions are the numpy replay of the recorded calls"""
    fus, ops = tracer_sedov(ctx, True), tracer_sedov(ctx, False)
    g = ref_geom(fus.geom)
    src = record_sources(fus)
    cf, co = record_advects(fus, g), record_advects(ops, g)
    pos = fus.tracers.positions()
    start = pos
    for step in range(5):
        assert fus.step() and ops.step()
        assert fus.dt_ == ops.dt_, step
        assert same_state(fus, ops), step
        assert len(cf) == 1
        same_calls(cf, co)
        assert np.array_equal(fus.tracers.positions(), ops.tracers.positions()), step
        new, keep = replay(g, pos, cf)
        assert keep.all() and np.array_equal(fus.tracers.positions(), new), step
        pos = new
        cf.clear()
        co.clear()
    assert src == ["velRk2"] * 5
    assert fus.counters.get("operator_stages", 0) == 0, fus.counters
    assert ops.counters["operator_stages"] == 10, ops.counters
    assert np.abs(pos - start).max() > 0.0


def over_cfl_pair(ctx, factor, **attrs):
    """the over-CFL step of test_retries_roll_the_tracers_back on both paths: three steps, then step(factor * dt)"""
    out = []
    for on_fused in (True, False):
        sim = tracer_sedov(ctx, on_fused, **attrs)
        g = ref_geom(sim.geom)
        for _ in range(3):
            assert sim.step()
        dt = sim.computeTimestepAtLevel() * factor
        src = record_sources(sim)
        calls = record_advects(sim, g)
        assert sim.step(dt)
        out.append((sim, calls, src, dt))
    return out


def test_driver_retries(ctx):
    (fus, cf, src, dtf), (ops, co, _, dto) = over_cfl_pair(ctx, 6.0)
    assert dtf == dto
    assert fus.counters["retries"] > 0 and fus.counters["retries"] == ops.counters["retries"]
    same_calls(cf, co)  # number, dt and face arrays of every call, those of dropped attempts included
    assert same_state(fus, ops)
    assert np.array_equal(fus.tracers.positions(), ops.tracers.positions())
    assert fus.counters["fofc1_stages"] == ops.counters["fofc1_stages"] and fus.counters["fofc2_stages"] == ops.counters["fofc2_stages"]
    assert fus.counters["fofc2_stages"] > 0, "no stage-2 correction pass stored avgFaceVel"
    assert set(src) == {"velRk2"} and fus.counters.get("operator_stages", 0) == 0
    print(f"retries {fus.counters['retries']}, advect calls {len(cf)}, counters {fus.counters}")


def test_driver_takes_the_exact_form_whatever_rk2_carry_rhs_says(ctx):
    fus = tracer_sedov(ctx, True, rk2_carry_rhs=True)
    ref = sedov_problem(ctx, 16, max_grid_size=8)  # fused, exact form, no tracers
    assert ref.use_fused and not ref._carry_active() and not fus._carry_active()
    start = fus.tracers.positions()
    for step in range(5):
        assert fus.step() and ref.step()
        assert fus.dt_ == ref.dt_ and same_state(fus, ref), step
    assert fus.counters.get("operator_stages", 0) == 0
    assert np.abs(fus.tracers.positions() - start).max() > 0.0
    # without tracers the same switches do select the carried form
    plain = sedov_problem(ctx, 16, max_grid_size=8)
    plain.rk2_carry_rhs, plain.tracers_on_fused_stages = True, 1
    assert plain._carry_active()


def test_driver_with_artificial_viscosity_takes_the_operators_average_of_a_redone_stage_2(ctx):
    """artificialViscosityK_ = 0.1 in the over-CFL step (6 x dt, the multiplier of the test without viscosity): the fused correction pass does not
    apply, a flagged stage is redone by _redo_stage_unfused, and after a redone stage 2 the tracers move on the operators' rk2vel"""
    (fus, cf, src, _), (ops, co, _, _) = over_cfl_pair(ctx, 6.0, artificialViscosityK_=0.1)
    print(f"fused-path counters {fus.counters}, operator-path counters {ops.counters}, sources {src}")
    assert fus.counters["fofc1_stages"] + fus.counters["fofc2_stages"] > 0
    assert fus.counters["fofc2_stages"] > 0 and "rk2vel" in src, "no stage 2 was redone on the operators"
    assert fus.counters.get("operator_stages", 0) > 0
    assert fus.counters["retries"] == ops.counters["retries"]
    same_calls(cf, co)
    assert same_state(fus, ops)
    assert np.array_equal(fus.tracers.positions(), ops.tracers.positions())


# ---------------------------------------------------------------------- 7. refusals through the C-ABI
def test_library_refuses_what_store_vel_rk2_cannot_do(case16):
    sim = case16.sim
    old, inter, new = sim.state_old_cc_, sim.state_inter_cc_, sim.state_new_cc_
    vel = face_arrays(sim)
    with pytest.raises(capi.QkError, match="store_vel_rk2"):  # the carried form has no halfVel
        launch(sim, stage_args(sim, 2, inter, old, new, DT, store_vel=1, vel=vel, carry=1))
    with pytest.raises(capi.QkError, match="store_vel_rk2"):  # stage 1
        launch(sim, stage_args(sim, 1, old, old, new, DT, store_vel=1, vel=vel))
    with pytest.raises(capi.QkError, match="store_vel_rk2"):  # a NULL array
        launch(sim, stage_args(sim, 2, inter, old, new, DT, store_vel=1, vel=[vel[0], None, vel[2]]))
    with pytest.raises(capi.QkError, match="store_vel_rk2"):  # over v1
        launch(sim, stage_args(sim, 2, inter, old, new, DT, store_vel=1, vel=[sim.halfVel[0], vel[1], vel[2]]))
    for d in range(3):
        assert torch.isnan(vel[d].storage).all(), "a refused call wrote"
    # field 0, arrays NULL: an ordinary exact-form stage 2
    assert launch(sim, stage_args(sim, 2, inter, old, new, DT)) == 0
    for b in range(sim.lev.nboxes):
        assert np.array_equal(new.valid(b).cpu().numpy(), case16.new[b])


# ---------------------------------------------------------------------- 8. default unchanged
def test_default_tracer_run_stays_on_the_operators(ctx):
    sim = tracer_sedov(ctx, False)
    src = record_sources(sim)
    for _ in range(2):
        assert sim.step()
    assert sim.counters["operator_stages"] == 4 and src == ["rk2vel"] * 2
    assert getattr(sim, "_velRk2", None) is None  # nothing allocated
