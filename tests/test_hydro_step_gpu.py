"""GPU parity of whole hydro steps (ghost fill + RK2 + FOFC + retries + dt control) against the CPU oracle.
Everything here is bit-exact: integer/index work AND the FP64 state (the tolerance north_star allows, 1e-12
relative L1, is never needed because kernels and oracle share association order and FMA contraction is off)."""
import os

import numpy as np
import pytest
import torch

from oracle.pyoracle import SEDOV, SOD
from quokka_amd.simulation import sedov_problem, sod_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def gather_oracle(s, N):
    U = np.zeros((s.ncomp, N, N, N))
    for b in range(s.nboxes):
        lo, hi = s.box(b)
        U[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = s.valid(b)
    return U


def gather_gpu(sim, N):
    U = np.zeros((6, N, N, N))
    for (lo, hi), v in zip(sim.my_boxes, sim.gather_valid_local()):
        U[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = v
    return U


def rel_l1(a, b):
    return max(np.abs(a[n] - b[n]).sum() / max(np.abs(b[n]).sum(), 1e-300) for n in range(a.shape[0]))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("mgs", [32, 16])
def test_sedov_steps_bit_exact(ctx, oracle, fused, mgs):
    N, nsteps = 32, 12
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sg = sedov_problem(ctx, N, max_grid_size=mgs, use_fused=fused)
    assert np.array_equal(gather_oracle(so, N), gather_gpu(sg, N))
    for it in range(nsteps):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, f"dt differs at step {it}: {so.dt} vs {sg.dt_}"
    Uo, Ug = gather_oracle(so, N), gather_gpu(sg, N)
    assert rel_l1(Ug, Uo) <= 1e-12
    assert np.array_equal(Uo, Ug), f"max abs diff {np.abs(Uo - Ug).max()}"
    assert so.time == sg.tNew_


def test_sedov_anisotropic_boxes_bit_exact(ctx, oracle):
    """non-cubic boxes (64 x 32 x 32): full 64-lane waves along x, several boxes along y and z"""
    N, nsteps = 64, 6
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[64, 32, 32])
    sg = sedov_problem(ctx, N, max_grid_size=[64, 32, 32])
    for it in range(nsteps):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, f"dt differs at step {it}: {so.dt} vs {sg.dt_}"
    Uo, Ug = gather_oracle(so, N), gather_gpu(sg, N)
    assert np.array_equal(Uo, Ug), f"max abs diff {np.abs(Uo - Ug).max()}"


def test_overlapped_fill_split_stage_bit_exact(ctx, oracle):
    """the multi-GPU schedule on one GPU: boxes 1, 4, 6 are declared 'remote dependent' by hand, so every stage runs as
    early group -> (exchange) -> late group with the physical boundaries split the same way; the result must not change"""
    N, mgs, nsteps = 32, 16, 8
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sg = sedov_problem(ctx, N, max_grid_size=mgs)
    sg.min_overlap_cells = 1  # (production: only groups that fill the GPU on their own are split)
    assert sg.overlap_groups() is None
    for b in (1, 4, 6):
        sg.ghost.set_box_remote(b, True)
    groups = sg.overlap_groups()
    assert groups is not None and groups[1][1] == [1, 4, 6] and len(groups[0][1]) == 5
    for it in range(nsteps):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_
    assert np.array_equal(gather_oracle(so, N), gather_gpu(sg, N))
    # ghost cells too (stage inputs of the next step)
    so.fill_ghosts(0, so.time)
    sg.fillBoundaryConditions(sg.state_new_cc_)
    for b in range(sg.lev.nboxes):
        assert np.array_equal(so.state(b), sg.state_new_cc_.fab_numpy(b))


def test_ghost_fill_matches_oracle(ctx, oracle):
    """FillBoundary between 8 boxes + reflecting walls: every ghost cell, every component."""
    N, mgs = 16, 8
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sg = sedov_problem(ctx, N, max_grid_size=mgs)
    for _ in range(3):
        assert so.step() and sg.step()
    so.fill_ghosts(0, so.time)
    sg.fillBoundaryConditions(sg.state_new_cc_)
    torch.cuda.synchronize()
    for b in range(so.nboxes):
        assert np.array_equal(so.state(b), sg.state_new_cc_.fab_numpy(b)), f"box {b}"


@pytest.mark.parametrize("fused_fofc", [True, False])
def test_fofc_and_retries_match_oracle(ctx, oracle, fused_fofc):
    """A 6x over-CFL step: first-order flux correction fires in both stages and the advance is retried with dt/2^n
    (reference src/QuokkaSimulation.hpp:911-964, 1144-1184, 1232-1270).  fused_fofc: the correction as one more fused pass
    (qk_hydro_stage_args::fofc_pass — first-order fluxes of the flagged faces evaluated on demand inside the sweeps) or the whole stage
    redone on the reference-shaped operators; either way every bit of the oracle's state."""
    N, mgs = 16, 8
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sg = sedov_problem(ctx, N, max_grid_size=mgs)
    sg.fused_fofc = fused_fofc
    for _ in range(3):
        assert so.step() and sg.step()
    dt = so.compute_dt() * 6.0
    assert so.advance_fixed_dt(dt)
    assert sg.step(dt)
    co = so.counters()
    assert co["fofc1_cells"] > 0 and co["fofc2_cells"] > 0 and co["retries"] > 0, co
    assert sg.counters["retries"] == co["retries"]
    assert sg.counters["fofc1_stages"] > 0 and sg.counters["fofc2_stages"] > 0
    assert np.array_equal(gather_oracle(so, N), gather_gpu(sg, N))


def test_fused_fofc_pass_floors_cells_it_could_not_repair(ctx):
    """abort_on_fofc_failure = 0 with a density floor: cells still at rho <= 0 after the first-order flux correction are handed to EnforceLimits
    and SyncDualEnergy like every other cell (reference src/QuokkaSimulation.hpp:1180-1192, :1267-1279) — the floor is what repairs them.  The
    fused correction pass must leave the same state as the stage redone on the reference-shaped operators: no non-positive density, same bits."""
    N, mgs = 16, 8
    sims = []
    for fused_fofc in (True, False):
        sg = sedov_problem(ctx, N, max_grid_size=mgs)
        sg.fused_fofc = fused_fofc
        for _ in range(3):
            assert sg.step()
        sg.abortOnFofcFailure_ = 0
        sg.densityFloor_ = 1.0e-3
        dt = sg.computeTimestepAtLevel() * 40.0  # far over the CFL limit: first-order fluxes cannot keep every cell positive either
        sg.state_old_cc_, sg.state_new_cc_ = sg.state_new_cc_, sg.state_old_cc_
        sg.advanceHydroAtLevel(sg.state_old_cc_, dt)  # (returns False: the CFL check fails afterwards, as it would in the reference)
        assert sg.counters["fofc1_stages"] > 0
        sims.append(sg)
    Uf, Uo = gather_gpu(sims[0], N), gather_gpu(sims[1], N)
    assert np.isfinite(Uo).all() and Uo[0].min() >= 1.0e-3
    assert (Uo[0] == 1.0e-3).any(), "no cell was floored: the test state does not exercise the branch"
    assert np.array_equal(Uf, Uo), f"rel L1 {np.abs(Uf - Uo).sum() / np.abs(Uo).sum()}"


@pytest.mark.parametrize("fused", [False, True])
def test_sod_shocktube_full_run_matches_golden(ctx, fused):
    """BASELINE config 1 (1-D Sod, 1024 cells, single box, Dirichlet x-boundaries) run to t = 0.4 with the reference-shaped operators
    (fused = False) and with the fused stage of a 1-D build (k_pre3 + the x sweep carrying the epilogue: 2 launches per stage instead of
    ~30); compared with the committed oracle state and the exact solution."""
    sim = sod_problem(ctx, 1024, use_fused=fused)
    assert sim.use_fused == fused
    assert sim.evolve()
    assert abs(sim.tNew_ - 0.4) < 1e-12
    sol = sim.gather_valid_local()[0][:, 0, 0, :]
    gold = np.load(os.path.join(HERE, "golden", "sod_1024_final.npy"))
    assert rel_l1(sol, gold) <= 1e-12
    assert np.array_equal(sol, gold)
    # (the reference's 0.002 criterion belongs to the deck's one-refined-level geometry and is asserted there:
    # tests/test_reference_problems_gpu.py::test_unmodified_shocktube_problem_meets_the_reference_criterion)


def test_sedov_conservation_gpu(ctx):
    """reference src/problems/HydroBlast3D/test_hydro3d_blast.cpp:181-199: |dE/E| <= 2e-15 on the GPU path."""
    N = 64
    sim = sedov_problem(ctx, N, max_grid_size=32)
    E0 = sum(float(sim.state_new_cc_.valid(b)[4].sum().item()) for b in range(sim.lev.nboxes))
    for _ in range(20):
        assert sim.step()
    U = gather_gpu(sim, N)
    E1 = U[4].sum()
    assert abs(E1 - E0) / E0 <= 2e-15 * 4  # box-wise device sums reorder the initial total; compare loosely
    assert abs(np.abs(U[0] - U[0].transpose(0, 2, 1)).max()) <= 1e-14


@pytest.mark.parametrize("isothermal", [False, True])
@pytest.mark.parametrize("reconstruct_eint", [False, True])
@pytest.mark.parametrize("order", [3, 2, 1])
def test_fused_stage_equals_reference_shaped_operators(ctx, order, reconstruct_eint, isothermal):
    _fused_vs_operators(ctx, order, reconstruct_eint, isothermal, 0.0)


@pytest.mark.parametrize("order", [3, 1])
def test_fused_stage_with_artificial_viscosity_equals_operators(ctx, order):
    """hydro.artificial_viscosity_coefficient > 0 (Colella & Woodward eq. 4.2, hydro_system.hpp:1054-1076) in the fused sweeps"""
    _fused_vs_operators(ctx, order, False, False, 0.1)


@pytest.mark.parametrize("order,reconstruct_eint,isothermal",
                         [(o, r, i) for i in (False, True) for r in (False, True) for o in (3, 2, 1) if not (i and r)])
def test_fused_stage_equals_operators_on_a_state_that_takes_every_fan(ctx, order, reconstruct_eint, isothermal):
    """the same comparison on fan_state (tests/hydro_cells_reference.py): random_state plus a rotating bulk velocity of a few c_s, so that both
    supersonic fans and both star fans occur in every direction (asserted on the CPU: tests/test_hydro_cells_reference.py)"""
    _fused_vs_operators(ctx, order, reconstruct_eint, isothermal, 0.0, state="fans")


@pytest.mark.parametrize("order", [3, 1])
def test_fused_stage_with_artificial_viscosity_equals_operators_on_a_state_that_takes_every_fan(ctx, order):
    _fused_vs_operators(ctx, order, False, False, 0.1, state="fans")


def test_fused_stage_on_a_state_that_takes_every_fan_matches_the_oracle(ctx, oracle):
    """The fused stage against the oracle itself, not against the operators: fan_state loaded into both, the geometry of _fused_vs_operators
    (32 x 24 x 16, two boxes, periodic), two advances of a fixed dt, every bit of the state.  Gamma law (the simulation oracle has no 3-D
    isothermal set-up).  No flux correction and no retry on either side."""
    import hydro_cells_reference as H
    from quokka_amd import capi
    from quokka_amd.simulation import Geometry, HydroSimulation
    from test_hydro_ops_gpu import random_state
    N = (32, 24, 16)
    U0 = H.fan_state(random_state(np.random.default_rng(7), (N[2], N[1], N[0])))
    so = oracle.sim(SEDOV, 3, list(N), [0.0] * 3, [1.0, 0.75, 0.5], [1, 1, 1], max_grid_size=[16, 24, 16])
    geom = Geometry(3, list(N), [0.0] * 3, [1.0, 0.75, 0.5], [1, 1, 1])
    bcs = [([capi.BC_INT_DIR] * 3, [capi.BC_INT_DIR] * 3)] * 6
    sg = HydroSimulation(ctx, geom, capi.traits(1.4, False, 3), bcs, [16, 24, 16], use_fused=True)
    sg.reconstructionOrder_ = 3
    assert sg.use_fused and so.nboxes == sg.lev.nboxes == 2
    ng = so.nghost
    pad = H.periodic_pad(U0, ng)
    for b in range(so.nboxes):
        lo, hi = so.box(b)
        assert (list(lo), list(hi)) == (list(sg.my_boxes[b][0]), list(sg.my_boxes[b][1]))
        fab = np.ascontiguousarray(pad[:, lo[2]:hi[2] + 1 + 2 * ng, lo[1]:hi[1] + 1 + 2 * ng, lo[0]:hi[0] + 1 + 2 * ng])
        so.set_state(fab, b, 0)
        sg.state_new_cc_.set_fab(b, fab)
    sg._signal_of_state_new = None
    dt = 2.0e-4
    for it in range(2):
        assert so.advance_fixed_dt(dt) and sg.step(dt), it
    co = so.counters()
    assert co["fofc1_cells"] == co["fofc2_cells"] == co["retries"] == 0, co
    assert sg.counters["fofc1_stages"] == sg.counters["fofc2_stages"] == sg.counters["retries"] == 0
    for b in range(so.nboxes):
        got, want = sg.state_new_cc_.valid(b).cpu().numpy(), so.valid(b)
        assert np.isfinite(want).all() and not np.array_equal(want, U0[:, so.box(b)[0][2]:so.box(b)[1][2] + 1, so.box(b)[0][1]:so.box(b)[1][1] + 1,
                                                                        so.box(b)[0][0]:so.box(b)[1][0] + 1])
        assert np.array_equal(got, want), f"box {b}: {int((got != want).sum())} values differ, max abs diff {np.abs(got - want).max()}"


def _fused_vs_operators(ctx, order, reconstruct_eint, isothermal, K_visc, state="random"):
    """Every template combination of the fused stage kernels (reconstruction order x reconstruct_eint x gamma-law /
    isothermal) against the reference-shaped operator chain — which tests/test_hydro_ops_gpu.py pins to the oracle — on a
    random shocked state, two boxes, periodic: both RK stages, new state, stage-1 face fluxes and redo flags bit for bit."""
    from quokka_amd import capi
    from quokka_amd.simulation import Geometry, HydroSimulation
    from test_hydro_ops_gpu import random_state

    if isothermal and reconstruct_eint:
        pytest.skip("gamma = 1 has no internal-energy reconstruction")
    N = (32, 24, 16)
    geom = Geometry(3, list(N), [0.0] * 3, [1.0, 0.75, 0.5], [1, 1, 1])
    tr = capi.traits(1.0, False, 3, cs_isothermal=1.3) if isothermal else capi.traits(1.4, reconstruct_eint, 3)
    bcs = [([capi.BC_INT_DIR] * 3, [capi.BC_INT_DIR] * 3)] * 6
    rng = np.random.default_rng(7)
    U0 = random_state(rng, (N[2], N[1], N[0]))
    if state == "fans":
        import hydro_cells_reference as H
        U0 = H.fan_state(U0)

    def run(fused):
        sim = HydroSimulation(ctx, geom, tr, bcs, [16, 24, 16], use_fused=fused)
        sim.reconstructionOrder_ = order
        sim.artificialViscosityK_ = K_visc
        sim.set_initial_conditions(lambda i, j, k: U0[:, k, j, i])
        dt = 2.0e-4
        old, inter, new = sim.state_old_cc_, sim.state_inter_cc_, sim.state_new_cc_
        sim.fillBoundaryConditions(old)
        assert sim._stage(1, old, old, inter, dt)
        f1 = [sim.halfFlux[d].fab_numpy(b) for d in range(3) for b in range(sim.lev.nboxes)]
        flag1 = [sim.redoFlag.fab_numpy(b) for b in range(sim.lev.nboxes)]
        sim.fillBoundaryConditions(inter)
        assert sim._stage(2, inter, old, new, dt)
        return ([inter.valid(b).cpu().numpy() for b in range(sim.lev.nboxes)], [new.valid(b).cpu().numpy() for b in range(sim.lev.nboxes)], f1, flag1,
                sim.counters)

    a, b = run(True), run(False)
    assert a[4]["fofc1_stages"] == 0 and b[4]["fofc1_stages"] == 0, "the test state must not trigger the flux correction"
    for name, x, y in zip(("stage 1 state", "stage 2 state", "stage 1 face fluxes", "redo flags"), a[:4], b[:4]):
        for n, (p, q) in enumerate(zip(x, y)):
            assert np.array_equal(p, q), f"{name}, array {n}: max abs diff {np.abs(p - q).max()}"


def test_sedov_ragged_boxes_bit_exact(ctx, oracle):
    """40^3 in boxes of at most 16: BoxArray::maxSize cuts 40 into 14 + 13 + 13, so one launch covers boxes of different
    extents (masked lanes / rows in every fused kernel, ghost plan between unequal neighbours)"""
    N, nsteps = 40, 6
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[16] * 3)
    sg = sedov_problem(ctx, N, max_grid_size=16)
    sizes = {tuple(hi[d] - lo[d] + 1 for d in range(3)) for lo, hi in sg.my_boxes}
    assert len(sizes) > 1, sizes
    for b, (lo, hi) in enumerate(sg.my_boxes):
        olo, ohi = so.box(b)
        assert list(olo) == list(lo) and list(ohi) == list(hi)
    for it in range(nsteps):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, f"dt differs at step {it}"
    assert np.array_equal(gather_oracle(so, N), gather_gpu(sg, N))


@pytest.mark.parametrize("periodic", [[0, 0, 0], [1, 1, 1]])
def test_sum_boundary_is_the_transpose_of_fill_boundary(ctx, periodic):
    """SumBoundary adds every ghost value to the valid cell it mirrors: checked item by item against the FillBoundary plan (integer-valued
    data, so the order of the additions cannot matter)"""
    from quokka_amd import capi
    from quokka_amd.multifab import Level, MultiFab
    from quokka_amd.simulation import GhostExchange, Geometry, chop_domain
    N, mgs, ng, nc = 16, 8, 1, 2
    geom = Geometry(3, [N] * 3, [0.0] * 3, [1.0] * 3, periodic)
    boxes = chop_domain([N] * 3, [mgs] * 3)
    lev = Level(ctx, 3, boxes)
    bcs = [([capi.BC_INT_DIR] * 3, [capi.BC_INT_DIR] * 3)] * nc
    ex = GhostExchange(lev, geom, nc, ng, boxes, [0] * len(boxes), 0, bcs)
    mf = MultiFab(lev, nc, ng)
    rng = np.random.default_rng(4)
    host = [rng.integers(-50, 50, size=s).astype(np.float64) for s in mf.shapes]
    for b, a in enumerate(host):
        mf.set_fab(b, a)
    ex.sum_boundary(mf)
    torch.cuda.synchronize()
    want = [a.copy() for a in host]
    for db, sb, lo, hi, sh, off in ex.items(0):
        d0, s0 = mf.begins[db], mf.begins[sb]
        g = host[db][:, lo[2] - d0[2]:hi[2] - d0[2] + 1, lo[1] - d0[1]:hi[1] - d0[1] + 1, lo[0] - d0[0]:hi[0] - d0[0] + 1]
        want[sb][:, lo[2] - sh[2] - s0[2]:hi[2] - sh[2] - s0[2] + 1, lo[1] - sh[1] - s0[1]:hi[1] - sh[1] - s0[1] + 1, lo[0] - sh[0] - s0[0]:hi[0] - sh[0] - s0[0] + 1] += g
    for b in range(len(boxes)):
        assert np.array_equal(mf.fab_numpy(b), want[b]), f"box {b}"
    assert any(not np.array_equal(want[b], host[b]) for b in range(len(boxes)))


@pytest.mark.parametrize("ndim,nscalars,nsteps", [(1, 1, 300), (3, 2, 12), (3, 1, 6), (3, 3, 6)])
def test_passive_scalars_match_oracle(ctx, oracle, ndim, nscalars, nsteps):
    """Passive scalars through the fused stage (hydro_system.hpp:340-343 cons->prim, HLLC.hpp:126-136 flux,
    hydro_system.hpp:1062-1076 viscosity term, :713-722 density floor): the advected contact of the PassiveScalar problem,
    several boxes, every component bit for bit; the scalar's integral is conserved to round-off."""
    from oracle.pyoracle import SCALARS
    from quokka_amd.simulation import scalar_contact_problem
    n_cell = [128, 1, 1] if ndim == 1 else [32, 16, 16]
    mgs = [64, 1, 1] if ndim == 1 else [16, 16, 16]
    so = oracle.sim(SCALARS, ndim, n_cell, [0, 0, 0], [1.0, 1.0, 1.0], [1, 1, 1], max_grid_size=mgs, nscalars=nscalars)
    sg = scalar_contact_problem(ctx, n_cell[0], nscalars=nscalars, ndim=ndim, max_grid_size=mgs)
    # the fused stage (instantiated for up to 3 passive scalars): 3-D and, since round 3, the 1-D build (x sweep + epilogue)
    assert sg.use_fused and sg.state_new_cc_.ncomp == 6 + nscalars
    sg_ops = None
    if sg.use_fused:  # the same run through the operator path: must agree with the fused stage in every bit
        sg_ops = scalar_contact_problem(ctx, n_cell[0], nscalars=nscalars, ndim=ndim, max_grid_size=mgs)
        sg_ops.use_fused = False
    for b in range(so.nboxes):
        assert sg.my_boxes[b] == tuple(so.box(b)) or list(sg.my_boxes[b][0]) == list(so.box(b)[0])
        sg.state_new_cc_.set_fab(b, so.state(b, 0))
        sg.state_old_cc_.set_fab(b, so.state(b, 1))
        if sg_ops is not None:
            sg_ops.state_new_cc_.set_fab(b, so.state(b, 0))
            sg_ops.state_old_cc_.set_fab(b, so.state(b, 1))
    s0 = sum(float(sg.state_new_cc_.valid(b)[6].sum()) for b in range(sg.lev.nboxes))
    for it in range(nsteps):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
        if sg_ops is not None:
            assert sg_ops.step() and sg_ops.dt_ == sg.dt_
    if sg.use_fused:
        assert sg.counters["fofc1_stages"] == sg.counters["fofc2_stages"] == 0  # every stage was carried by the fused kernels
    for b in range(so.nboxes):
        a, g = so.valid(b), sg.state_new_cc_.valid(b).cpu().numpy()
        assert np.array_equal(a, g), (b, [float(np.abs(a[n] - g[n]).max()) for n in range(6 + nscalars)])
        if sg_ops is not None:
            assert np.array_equal(g, sg_ops.state_new_cc_.valid(b).cpu().numpy()), b
    s1 = sum(float(sg.state_new_cc_.valid(b)[6].sum()) for b in range(sg.lev.nboxes))
    assert abs(s1 - s0) <= 1e-13 * abs(s0)
    assert float(sg.state_new_cc_.valid(0)[6].max()) > 0.9  # the step is still there


@pytest.mark.parametrize("name", ["vacuum", "shuosher", "highmach", "sms", "leblanc"])
def test_tabulated_1d_known_answers_on_the_gpu_path(ctx, oracle, name):
    """The reference's four 1-D hydro tests with tabulated solutions (tests/hydro1d_cases.py), run to their stop times through the
    C-ABI: the final state equals the oracle's in every bit (same initial state: sin() of the generators differs by an ulp between
    libms), so the reference's tolerance is met by the GPU path exactly as by the oracle.  Exercises Dirichlet faces, dt control
    (maxDt, initDt), strong rarefactions / shocks, the dual-energy switch and (HighMach) the retry path."""
    import hydro1d_cases as H
    from quokka_amd.simulation import hydro1d_problem
    c = H.CASES[name]
    so = H.oracle_sim(oracle, name)
    sg = hydro1d_problem(ctx, c["spec"], c["nx"], c["hi"], c["max_timesteps"], c.get("mgs"), use_fused=True)  # the fused stage of a 1-D build
    assert sg.use_fused
    for b in range(so.nboxes):
        assert np.allclose(sg.state_new_cc_.fab_numpy(b), so.state(b, 0), rtol=1e-14, atol=1e-300)  # the generators agree to libm accuracy
        sg.state_new_cc_.set_fab(b, so.state(b, 0))
        sg.state_old_cc_.set_fab(b, so.state(b, 1))
    assert so.evolve() and sg.evolve()
    assert (so.istep, so.time) == (sg.istep, sg.tNew_)
    Uo = H.gather_x(so)
    Ug = np.concatenate([sg.state_new_cc_.valid(b).cpu().numpy()[:, 0, 0, :] for b in range(sg.lev.nboxes)], axis=-1)
    assert np.array_equal(Uo, Ug), [float(np.abs(Uo[n] - Ug[n]).max()) for n in range(6)]
    assert sg.counters["retries"] == so.counters()["retries"]
    assert H.error_norm(H.reference_state(name), Ug) < c["tol"]


def test_linear_sound_wave_on_the_gpu_path(ctx, oracle):
    """HydroWave through the C-ABI: bit for bit with the oracle after one period (2998 steps at CFL 0.1), hence the same error
    (rms of mean |U(1) - U(0)| < 1e-8, the reference's criterion for 100 cells)"""
    import hydro1d_cases as H
    from quokka_amd.simulation import hydro1d_problem
    c = H.CASES["wave"]
    so = H.oracle_sim(oracle, "wave")
    sg = hydro1d_problem(ctx, c["spec"], c["nx"], c["hi"], c["max_timesteps"])
    assert np.allclose(sg.state_new_cc_.fab_numpy(0), so.state(0, 0), rtol=1e-13, atol=1e-300)
    sg.state_new_cc_.set_fab(0, so.state(0, 0))
    sg.state_old_cc_.set_fab(0, so.state(0, 1))
    U0 = H.gather_x(so)
    assert so.evolve() and sg.evolve()
    Ug = sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, :]
    assert np.array_equal(H.gather_x(so), Ug) and so.istep == sg.istep
    assert H.wave_error(U0, Ug) < c["tol"]


def test_flux_rk2_of_the_fused_stage_is_race_free_and_equals_the_operator_path(ctx):
    """`store_flux_rk2` (what the flux registers of an AMR hierarchy accumulate): the stage-2 x sweep evaluates the face between two of
    its 250-cell tiles in both tiles; the first version averaged F1 in place there, so the second evaluation could read the averaged
    value.  flux_rk2 now goes to separate arrays: on rows long enough to span several tiles, repeated runs give the operator path's
    0.5 F1 + 0.5 F2 bit for bit in every face, the new state is unaffected, F1 is left intact, and aliasing the two is refused."""
    from quokka_amd import capi
    from quokka_amd.simulation import Geometry, HydroSimulation
    from test_hydro_ops_gpu import random_state
    N = (96, 20, 8)  # flat slab rows of (96 + 8) x 20 cells: eight tile boundaries per plane
    geom = Geometry(3, list(N), [0.0] * 3, [1.0, 0.25, 0.125], [1, 1, 1])
    tr = capi.traits(1.4, False, 3)
    bcs = [([capi.BC_INT_DIR] * 3, [capi.BC_INT_DIR] * 3)] * 6
    U0 = random_state(np.random.default_rng(11), (N[2], N[1], N[0]))

    def run(fused):
        sim = HydroSimulation(ctx, geom, tr, bcs, list(N), use_fused=fused)
        sim.store_flux_rk2 = True
        sim.set_initial_conditions(lambda i, j, k: U0[:, k, j, i])
        dt = 1.0e-4
        old, inter, new = sim.state_old_cc_, sim.state_inter_cc_, sim.state_new_cc_
        sim.fillBoundaryConditions(old)
        assert sim._stage(1, old, old, inter, dt)
        f1 = [sim.halfFlux[d].fab_numpy(0).copy() for d in range(3)]
        sim.fillBoundaryConditions(inter)
        assert sim._stage(2, inter, old, new, dt)
        if fused:
            for d in range(3):
                assert np.array_equal(sim.halfFlux[d].fab_numpy(0), f1[d]), "stage 2 must leave the stage-1 flux alone"
        return [sim.fluxRk2()[d].fab_numpy(0) for d in range(3)], new.valid(0).cpu().numpy(), sim

    want, new_want, _ = run(False)
    for rep in range(12):
        got, new_got, sim = run(True)
        for d in range(3):
            assert np.array_equal(got[d], want[d]), (rep, d, float(np.abs(got[d] - want[d]).max()))
        assert np.array_equal(new_got, new_want)
    # aliasing flux_rk2 with the stage-1 flux is refused by the library
    sim._fluxRk2 = sim.halfFlux
    sim.fillBoundaryConditions(sim.state_inter_cc_)
    with pytest.raises(capi.QkError, match="fluxRk2"):
        sim._stage(2, sim.state_inter_cc_, sim.state_old_cc_, sim.state_new_cc_, 1.0e-4)


@pytest.mark.parametrize("ndim", [1, 2])
def test_flux_rk2_of_the_fused_stage_in_one_and_two_dimensions(ctx, ndim):
    """the same in 1-D / 2-D builds (the x sweep carries the epilogue in 1-D, the marching y sweep through the index-swap view in 2-D): what the
    flux registers of a 1-D / 2-D hierarchy accumulate — flux_rk2 of every direction and the new state equal the operator path's bit for bit"""
    from quokka_amd import capi
    from quokka_amd.simulation import Geometry, HydroSimulation
    from test_hydro_ops_gpu import random_state
    N = (96, 20, 1) if ndim == 2 else (300, 1, 1)
    geom = Geometry(ndim, list(N), [0.0] * 3, [1.0, 0.25, 1.0], [1, 1, 0] if ndim == 2 else [1, 0, 0])
    tr = capi.traits(1.4, False, ndim)
    bcs = [([capi.BC_INT_DIR] * 3, [capi.BC_INT_DIR] * 3)] * 6
    U0 = random_state(np.random.default_rng(12), (N[2], N[1], N[0]))

    def run(fused):
        sim = HydroSimulation(ctx, geom, tr, bcs, [48, 10, 1] if ndim == 2 else [100, 1, 1], use_fused=fused)
        sim.store_flux_rk2 = True
        sim.set_initial_conditions(lambda i, j, k: U0[:, k, j, i])
        dt = 1.0e-4
        old, inter, new = sim.state_old_cc_, sim.state_inter_cc_, sim.state_new_cc_
        sim.fillBoundaryConditions(old)
        assert sim._stage(1, old, old, inter, dt)
        sim.fillBoundaryConditions(inter)
        assert sim._stage(2, inter, old, new, dt)
        return [[sim.fluxRk2()[d].fab_numpy(b) for b in range(sim.lev.nboxes)] for d in range(ndim)], sim.gather_valid_local()

    want, new_want = run(False)
    got, new_got = run(True)
    for d in range(ndim):
        for b in range(len(want[d])):
            assert np.array_equal(got[d][b], want[d][b]), (d, b, float(np.abs(got[d][b] - want[d][b]).max()))
    for a, b in zip(new_got, new_want):
        assert np.array_equal(a, b)


def test_mass_scalars_cma_match_oracle(ctx, oracle):
    """HydroShocktubeCMA through the C-ABI (`nmscalars = 3`): consistent multi-fluid advection of the partial-density fluxes, the
    non-negativity check of isStateValid and the renormalisation in EnforceLimits, with artificial viscosity — 1500 steps from the
    oracle's initial state bit for bit, the reference's 1e-13 criterion after every step on the GPU state."""
    from oracle.pyoracle import SHOCKTUBE_CMA
    from quokka_amd.simulation import shocktube_cma_problem
    so = oracle.sim(SHOCKTUBE_CMA, 1, [1024, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[1024, 1, 1])
    U0 = so.valid(0).copy()
    sg = shocktube_cma_problem(ctx, 1024, initial_state=U0)
    assert np.array_equal(U0, sg.state_new_cc_.valid(0).cpu().numpy())
    worst = 0.0
    for it in range(1500):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
        if it % 50 == 0 or it == 1499:
            U = sg.state_new_cc_.valid(0).cpu().numpy()
            assert np.array_equal(so.valid(0), U), it
            worst = max(worst, float(np.abs(1.0 - U[6:9, 0, 0].sum(axis=0) / U[0, 0, 0]).max()))
    assert worst < 1.0e-13
    sp = shocktube_cma_problem(ctx, 1024)  # the Python evaluation of the initial profile: equal to rounding
    assert np.allclose(sp.state_new_cc_.valid(0).cpu().numpy(), U0, rtol=1e-13, atol=1e-16)


# ------------------------------------------------------------------ the carried-right-hand-side form of the RK2 average (rk2_carry_rhs)
@pytest.mark.parametrize("mgs", [32, 16])
def test_carried_rhs_mode_stays_within_the_parity_tolerance(ctx, oracle, mgs):
    """qk_hydro_stage_args::rk2_carry_rhs = 1: stage 1 stores div F1 / div v1 per cell, stage 2 averages the right-hand sides instead of the face
    fluxes.  Not bit-exact by construction (different rounding of the same quantity): the contract is north_star's 1e-12 relative L1 per
    conserved component against the oracle — checked after 40 steps of the blast crossing box boundaries — and it must really be the other
    mode (some bits differ), with the face arrays never touched.  Against the oracle's own carried form (set_rk2_carry_rhs): every bit and every dt."""
    N, nsteps = 32, 40
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sc = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sc.set_rk2_carry_rhs(True)
    sg = sedov_problem(ctx, N, max_grid_size=mgs)
    sg.rk2_carry_rhs = True
    for d in range(3):
        sg.halfFlux[d].storage.fill_(float("nan"))  # a read of F1 would poison the state
    for it in range(nsteps):
        assert so.step() and sg.step() and sc.step()
        assert abs(so.dt - sg.dt_) <= 1e-13 * so.dt, f"dt at step {it}: {so.dt} vs {sg.dt_}"
        assert sc.dt == sg.dt_, f"dt at step {it}: {sc.dt} (carried oracle) vs {sg.dt_}"
    Uo, Ug = gather_oracle(so, N), gather_gpu(sg, N)
    assert np.isfinite(Ug).all()
    err = rel_l1(Ug, Uo)
    print(f"carried-rhs mode vs oracle after {nsteps} steps ({mgs}^3 boxes): relative L1 = {err:.3e}")
    assert err <= 1e-12
    assert not np.array_equal(Uo, Ug)
    Uc = gather_oracle(sc, N)
    assert np.array_equal(Uc, Ug), f"carried oracle: {int((Uc != Ug).sum())} values differ, max abs diff {np.abs(Uc - Ug).max()}"
    assert all(bool(torch.isnan(sg.halfFlux[d].storage).all()) for d in range(3))
    assert sg.counters["fofc1_stages"] + sg.counters["fofc2_stages"] == 0


def test_carried_rhs_mode_with_first_order_flux_correction(ctx, oracle):
    """the carried mode when the fused stages flag cells: stage 1 takes the fused correction pass; stage 2 — whose correction replaces
    flux_rk2 = 0.5 F1 + 0.5 F2 of a face as a whole, with F1 never stored in this mode — is redone in the exact form on the FUSED kernels (F1
    from one more run of the stage-1 sweeps over the old state).  No reference-shaped operator runs.  Same over-CFL step as
    test_fofc_and_retries_match_oracle.  Every bit of the oracle's own carried form (set_rk2_carry_rhs), which takes the same stage-1 correction,
    exact-form stage 2 and retries."""
    N, mgs = 16, 8
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sc = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sc.set_rk2_carry_rhs(True)
    sg = sedov_problem(ctx, N, max_grid_size=mgs)
    sg.rk2_carry_rhs = True
    for _ in range(3):
        assert so.step() and sg.step() and sc.step()
        assert sc.dt == sg.dt_
    dt = so.compute_dt() * 6.0
    assert so.advance_fixed_dt(dt) and sc.advance_fixed_dt(dt)
    def no_operators(*a, **k):
        raise AssertionError("a stage fell back to the reference-shaped operators")
    sg._redo_stage_unfused = no_operators
    assert sg.step(dt)
    co = so.counters()
    assert sg.counters["retries"] == co["retries"] and sg.counters["fofc1_stages"] > 0 and sg.counters["fofc2_stages"] > 0
    assert sg._unfused_tmp is None  # (the operator path's temporaries were never even allocated)
    assert rel_l1(gather_gpu(sg, N), gather_oracle(so, N)) <= 1e-12
    cc = sc.counters()
    assert cc["retries"] == co["retries"] and cc["fofc1_cells"] > 0 and cc["carry2_fallbacks"] > 0, cc
    assert np.array_equal(gather_oracle(sc, N), gather_gpu(sg, N))


def test_drift_of_the_carried_form_is_that_of_a_one_ulp_perturbation(ctx):
    """How far the carried half step drifts from the exact form over a long run, with a yardstick: a third run in the EXACT form whose blast energy is
    one unit in the last place higher (relative 2e-16: the size of one rounding difference).  128^3, lockstep.  Through the 1000 steps the deck of
    BASELINE config 2 runs, the carried form stays within 1e-12 (measured 3e-15) — and wherever it later does not, the perturbed exact run has left
    the exact run just as far: the blast amplifies rounding-level differences by ~10^14 in 5000 steps (profiles/round4/carry_drift_128.txt), so a
    cell-by-cell tolerance over the reference ctest's 12 000 steps pins nothing but that instability."""
    N = 128
    a, b, c = (sedov_problem(ctx, N, max_grid_size=128) for _ in range(3))
    b.rk2_carry_rhs = True
    v = c.state_new_cc_.valid(0)
    e = v[4, 0, 0, 0].item()
    v[4, 0, 0, 0] = float(np.nextafter(e, 2 * e))
    c.fillBoundaryConditions(c.state_new_cc_)

    def dist(x, y):
        worst = 0.0
        for n in range(6):
            p, q = x.state_new_cc_.valid(0)[n], y.state_new_cc_.valid(0)[n]
            worst = max(worst, float((p - q).abs().sum(dtype=torch.float64)) / max(float(p.abs().sum(dtype=torch.float64)), 1e-300))
        return worst

    for it in range(1, 3001):
        assert a.step() and b.step() and c.step()
        if it in (100, 1000, 2000, 3000):
            carry, ulp = dist(a, b), dist(a, c)
            print(f"step {it}: carried vs exact {carry:.2e}; exact with the blast energy one ulp up vs exact {ulp:.2e}")
            assert carry <= max(1e-12, 10.0 * ulp), (it, carry, ulp)
            if it <= 1000:
                assert carry <= 1e-12, (it, carry)
    assert b.counters["fofc1_stages"] + b.counters["fofc2_stages"] + b.counters["retries"] == 0


def test_carried_rhs_mode_with_passive_scalars_and_lower_orders(ctx):
    """every instantiation of the carried mode (PPM / PLM / donor cell, 0 and 2 passive scalars) against the exact mode of the same build"""
    from quokka_amd.simulation import sedov_problem as mk
    for order in (3, 2, 1):
        a, b = mk(ctx, 32, max_grid_size=16), mk(ctx, 32, max_grid_size=16)
        a.reconstructionOrder_ = b.reconstructionOrder_ = order
        b.rk2_carry_rhs = True
        for _ in range(10):
            assert a.step() and b.step()
        assert rel_l1(gather_gpu(b, 32), gather_gpu(a, 32)) <= 1e-12, order


# ------------------------------------------------------------------ the primitive hand-off between the stages of a step (prim_out / prim_in)
@pytest.mark.gpu
def test_primitive_handoff_between_the_stages_changes_no_bit(ctx, oracle):
    """qk_hydro_stage_args::prim_out / prim_in: the final sweep of stage 1 stores the primitives of the intermediate state (one pressure more: its
    limits already formed the velocities), the pre-pass and the three sweeps of stage 2 read them instead of converting the conserved state 4.9
    times per cell.  Same bytes, same bits: the exact form against the oracle, the carried form against itself without the hand-off; and a step
    whose stages flag cells (6x over-CFL: first-order flux correction + retries) drops the attempt and proceeds as without it."""
    N, mgs = 32, 16
    so = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    sg = sedov_problem(ctx, N, max_grid_size=mgs)
    sg.prim_handoff = True
    assert sg._prim_handoff_applies()
    for it in range(12):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, it
    assert np.array_equal(gather_oracle(so, N), gather_gpu(sg, N))
    assert sg.counters.get("prim_handoff_dropped", 0) == 0
    # flagged cells: the attempt is dropped, the correction runs as it does without the hand-off
    dt = so.compute_dt() * 6.0
    assert so.advance_fixed_dt(dt) and sg.step(dt)
    co = so.counters()
    assert co["fofc1_cells"] > 0 and co["retries"] > 0 and sg.counters["prim_handoff_dropped"] > 0
    assert sg.counters["retries"] == co["retries"]
    for it in range(3):
        assert so.step() and sg.step()
    assert np.array_equal(gather_oracle(so, N), gather_gpu(sg, N))
    # the carried form
    a, b = sedov_problem(ctx, N, max_grid_size=mgs), sedov_problem(ctx, N, max_grid_size=mgs)
    a.rk2_carry_rhs = b.rk2_carry_rhs = True
    b.prim_handoff = True
    for it in range(12):
        assert a.step() and b.step()
        assert a.dt_ == b.dt_
    assert np.array_equal(gather_gpu(a, N), gather_gpu(b, N))
    assert b.counters.get("prim_handoff_dropped", 0) == 0


# ------------------------------------------------------------------ the X sweep folded into the Y march (FUSEX)
@pytest.mark.parametrize("N,mgs,handoff", [(128, 64, True), (128, 128, True), (128, 128, False), (64, 64, True)])
def test_x_sweep_inside_the_y_march_changes_no_bit(ctx, N, mgs, handoff):
    """k_sweep_march<Y, ..., FUSEX>: the X sweep of a row is formed inside the Y march from the neighbouring lanes (wave-private LDS), the two
    faces a wave cannot form from its own 64 lanes come from a batch pass every 32 rows — the X launch, its 128 B per cell and the 56 B per
    cell Y used to read back are gone.  Same device functions on the same operands: the carried form with QK_FUSEX=1 equals QK_FUSEX=0 in
    every bit — from the developed blast (every limiter and HLLC fan active), boxes one and two waves wide, a single box marched in several
    segments, with and without the primitive hand-off; six steps."""
    import os
    from quokka_amd.simulation import developed_state, sedov_problem
    finals = []
    try:
        for fusex in ("0", "1"):
            os.environ["QK_FUSEX"] = fusex
            s = sedov_problem(ctx, N, max_grid_size=mgs)
            s.rk2_carry_rhs = True
            s.prim_handoff = handoff
            for b, (lo, hi) in enumerate(s.my_boxes):
                s.state_new_cc_.set_fab(b, developed_state(N, lo, hi))
            s._signal_of_state_new = None
            dts = []
            for _ in range(6):
                assert s.step()
                dts.append(s.dt_)
            assert s.counters["fofc1_stages"] + s.counters["fofc2_stages"] == 0
            finals.append((gather_gpu(s, N), dts))
    finally:
        os.environ.pop("QK_FUSEX", None)
    assert finals[0][1] == finals[1][1]
    assert np.array_equal(finals[0][0], finals[1][0])


def test_x_sweep_inside_the_y_march_with_boxes_of_two_widths(ctx):
    """FUSEX on a level whose boxes are 128 and 64 cells wide (192 x 64 x 64 cells chopped at 128): the launch is sized for the widest box, the
    64-cell chunk beyond a narrow box leaves at once (its edge faces would lie outside the fab).  Equal to QK_FUSEX=0 in every bit."""
    import os
    from quokka_amd import capi
    from quokka_amd.simulation import Geometry, HydroSimulation, developed_state
    finals = []
    try:
        for fusex in ("0", "1"):
            os.environ["QK_FUSEX"] = fusex
            geom = Geometry(3, [192, 64, 64], [0.0, 0.0, 0.0], [3.6, 1.2, 1.2], [0, 0, 0])
            bcs = []
            for c in range(6):
                lo = [capi.BC_REFLECT_ODD if c == 1 + d else capi.BC_REFLECT_EVEN for d in range(3)]
                bcs.append((lo, list(lo)))
            boxes = [([0, 0, 0], [127, 63, 63]), ([128, 0, 0], [191, 63, 63])]
            s = HydroSimulation(ctx, geom, capi.traits(1.4, False, 3), bcs, [128, 64, 64], boxes=boxes, owner=[0, 0])
            s.reconstructionOrder_, s.stopTime_, s.cflNumber_ = 3, 1.0, 0.3
            assert sorted({hi[0] - lo[0] + 1 for lo, hi in s.my_boxes}) == [64, 128]
            s.rk2_carry_rhs = True
            for b, (lo, hi) in enumerate(s.my_boxes):
                s.state_new_cc_.set_fab(b, developed_state(64, lo, hi))
            s._signal_of_state_new = None
            for _ in range(5):
                assert s.step()
            finals.append([v.copy() for v in s.gather_valid_local()])
    finally:
        os.environ.pop("QK_FUSEX", None)
    for a, b in zip(*finals):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", [(64, 8, 8), (64, 24, 40), (128, 40, 24), (64, 72, 8), (192, 8, 56), (64, 16, 136)])
def test_x_sweep_inside_the_y_march_on_boxes_of_odd_heights(ctx, shape):
    """FUSEX on the boxes a hierarchy with amr.blocking_factor = 8 produces: 64-cell multiples wide, but 8, 24, 40, 72 ... rows high and deep — fewer rows than one
    batch of wave-edge faces (16), a last batch that is not full, marches shorter than one segment.  One box, reflecting walls, the developed blast; equal to
    QK_FUSEX=0 in every bit after four steps."""
    import os
    from quokka_amd import capi
    from quokka_amd.simulation import Geometry, HydroSimulation, developed_state
    finals = []
    try:
        for fusex in ("0", "1"):
            os.environ["QK_FUSEX"] = fusex
            geom = Geometry(3, list(shape), [0.0, 0.0, 0.0], [1.2 * shape[0] / 64, 1.2 * shape[1] / 64, 1.2 * shape[2] / 64], [0, 0, 0])
            bcs = []
            for c in range(6):
                lo = [capi.BC_REFLECT_ODD if c == 1 + d else capi.BC_REFLECT_EVEN for d in range(3)]
                bcs.append((lo, list(lo)))
            boxes = [([0, 0, 0], [shape[0] - 1, shape[1] - 1, shape[2] - 1])]
            s = HydroSimulation(ctx, geom, capi.traits(1.4, False, 3), bcs, list(shape), boxes=boxes, owner=[0])
            s.reconstructionOrder_, s.stopTime_, s.cflNumber_ = 3, 1.0, 0.3
            s.rk2_carry_rhs = True
            for b, (lo, hi) in enumerate(s.my_boxes):
                s.state_new_cc_.set_fab(b, developed_state(64, lo, hi))
            s._signal_of_state_new = None
            for _ in range(4):
                assert s.step()
            finals.append(([v.copy() for v in s.gather_valid_local()], dict(s.counters)))
    finally:
        os.environ.pop("QK_FUSEX", None)
    assert finals[0][1] == finals[1][1]
    for a, b in zip(finals[0][0], finals[1][0]):
        assert np.isfinite(a).all() and np.array_equal(a, b)
