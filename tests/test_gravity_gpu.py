"""Self-gravity on the GPU (csrc/qk_gravity.hip, quokka_amd/gravity.py) against the numpy restatement of tests/gravity_reference.py:
the multigrid Dirichlet solve to the maximum-principle bound, the surface potential to the rounding of its sum, right-hand side and kick bit for bit,
and the driver — switch off, G = 0, a collapsing cold blob replayed step by step, the time step after the kick, every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import gravity_reference as gr
from quokka_amd import capi
from quokka_amd.gravity import NotConverged, PoissonSolver
from quokka_amd.multifab import Level, MultiFab
from quokka_amd.simulation import Geometry, HydroSimulation, chop_domain

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------- helpers
def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def random_problem(n, seed):
    """random right-hand side on the interior, random Dirichlet data on the ghost list, zero first guess"""
    rng = np.random.default_rng(seed)
    f = np.zeros(gr.dense_shape(n))
    gr.interior(f)[...] = rng.standard_normal(gr.interior(f).shape)
    phi = np.zeros_like(f)
    g, _ = gr.ghost_list(n)
    gr.put(phi, g, rng.standard_normal(g.shape[0]))
    return f, phi


def check_dirichlet(n, h, f, ghosts, phi_gpu, tol):
    """the two assertions of every Dirichlet case: the residual recomputed in numpy, and the distance to the direct solve within the maximum-principle bound
    (plus the same bound for the direct solve's own residual: the triangle inequality)"""
    g, _ = gr.ghost_list(n)
    assert np.array_equal(gr.at(phi_gpu, g), gr.at(ghosts, g)), "the solve changed the Dirichlet data"
    res = np.abs(gr.residual(phi_gpu, f, h)).max()
    direct = gr.dirichlet_solve_direct(f, ghosts, h)
    res_direct = np.abs(gr.residual(direct, f, h)).max()
    err = np.abs(gr.interior(phi_gpu) - gr.interior(direct)).max()
    bound = gr.max_principle_bound(n, h, res) + gr.max_principle_bound(n, h, res_direct)
    print(f"n = {n}: residual {res:.3e} (tolerance {tol:.3e}), |phi - direct| {err:.3e}, bound {bound:.3e}")
    assert res <= tol
    assert err <= bound
    return res


def hydro_sim(ctx, n_cell, mgs, prob_hi=None, periodic=(0, 0, 0)):
    ndim = len(n_cell)
    hi = list(prob_hi) if prob_hi is not None else [1.0] * 3
    geom = Geometry(ndim, list(n_cell), [0.0, 0.0, 0.0], hi, list(periodic))
    bcs = [([capi.BC_FOEXTRAP] * 3, [capi.BC_FOEXTRAP] * 3) for _ in range(6)]
    sim = HydroSimulation(ctx, geom, capi.traits(5.0 / 3.0, False, ndim), bcs, list(mgs))
    sim.cflNumber_, sim.stopTime_ = 0.3, 1.0e30
    return sim


def blob_ic(sim, amp=10.0, sigma=0.12, centre=(0.45, 0.55, 0.5), P=0.1):
    dx = sim.geom.dx

    def ic(i, j, k):
        x, y, z = (i + 0.5) * dx[0], (j + 0.5) * dx[1], (k + 0.5) * dx[2]
        r2 = (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2
        U = np.zeros((6,) + i.shape)
        U[0] = 1.0 + amp * np.exp(-0.5 * r2 / sigma ** 2)
        U[5] = P / (5.0 / 3.0 - 1.0)
        U[4] = U[5]
        return U
    return ic


def global_state(sim):
    n = sim.geom.n_cell
    out = np.zeros((sim.ncomp_cc, n[2], n[1], n[0]))
    for b, (lo, hi) in enumerate(sim.my_boxes):
        out[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = sim.state_new_cc_.valid(b).cpu().numpy()
    return out


# ---------------------------------------------------------------------- the Dirichlet solve
@pytest.mark.parametrize("n", [(8, 8, 8), (16, 8, 12), (34, 34, 34)])
def test_dirichlet_solve_random(ctx, n):
    """(34^3 halves once, to 17^3 = 4913 cells: a coarsest level too large for the single-workgroup launch of the small levels — its sweeps are
    launches, and being smoothed rather than solved it costs cycles: 27 in the numpy prototype of the same algorithm against 9-11 elsewhere)"""
    h = 1.0 / n[0]
    f, ghosts = random_problem(n, seed=sum(n))
    ps = PoissonSolver(ctx, n, h)
    ps.rhs.copy_(dev(ctx, f))
    ps.phi.copy_(dev(ctx, ghosts))
    cycles, res_gpu = ps.solve_dirichlet(1.0e-10, 0.0)
    tol = 1.0e-10 * np.abs(f).max()
    res = check_dirichlet(n, h, f, ghosts, ps.phi.cpu().numpy(), tol)
    print(f"{cycles} V-cycles, residual on the device {res_gpu:.3e}")
    assert 0 < cycles <= (30 if n != (34, 34, 34) else 100) and res_gpu <= tol


def test_dirichlet_solve_32_from_eight_boxes(ctx):
    """32^3 with the right-hand side filled from a level of eight 16^3 boxes (qk_gravity_fill_rhs adds to what is there)"""
    n, h, G = (32, 32, 32), 1.0 / 32, 0.37
    boxes = chop_domain(list(n), [16, 16, 16])
    assert len(boxes) == 8
    lev = Level(ctx, 3, boxes)
    rng = np.random.default_rng(32)
    state = MultiFab(lev, 6, 4, fill=0.0)
    rho = rng.standard_normal((n[2], n[1], n[0]))
    for b, (lo, hi) in enumerate(boxes):
        state.valid(b)[0].copy_(dev(ctx, rho[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]))
    f, ghosts = random_problem(n, seed=5)  # (f: what is there before the add)
    ps = PoissonSolver(ctx, n, h)
    ps.rhs.copy_(dev(ctx, f))
    ps.fill_rhs(lev, state, G)
    gr.fill_rhs(f, rho, G)
    assert np.array_equal(ps.rhs.cpu().numpy(), f)
    ps.phi.copy_(dev(ctx, ghosts))
    cycles, _ = ps.solve_dirichlet(1.0e-10, 0.0)
    check_dirichlet(n, h, f, ghosts, ps.phi.cpu().numpy(), 1.0e-10 * np.abs(f).max())
    assert 0 < cycles <= 30


def test_dirichlet_solve_reports_no_convergence(ctx):
    n, h = (8, 8, 8), 0.125
    f, ghosts = random_problem(n, seed=1)
    ps = PoissonSolver(ctx, n, h)
    ps.rhs.copy_(dev(ctx, f))
    ps.phi.copy_(dev(ctx, ghosts))
    it, res = C.c_int(-1), C.c_double(-1.0)
    rc = ctx.L.qk_gravity_dirichlet_solve(ctx.h, ctx.stream(), ps._n, h, ps._p(ps.rhs), ps._p(ps.phi), 1.0e-30, 0.0, 1, ps._p(ps.scratch),
                                          ps.scratch.numel() * 8, C.byref(it), C.byref(res))
    assert rc == capi.QK_ERR_NOT_CONVERGED and it.value == 1 and res.value > 0.0
    with pytest.raises(NotConverged, match="V-cycles"):
        ps.solve_dirichlet(1.0e-30, 0.0, max_iter=1)
    # a right-hand side that is not finite is an error, never a silent result
    f[3, 3, 3] = np.nan
    ps.rhs.copy_(dev(ctx, f))
    with pytest.raises(capi.QkError, match="NaN"):
        ps.solve_dirichlet(1.0e-10, 0.0)


# ---------------------------------------------------------------------- the surface potential
@pytest.mark.parametrize("n", [(8, 8, 8), (8, 6, 4)])
def test_surface_potential_random(ctx, n):
    g, _ = gr.ghost_list(n)
    S = g.shape[0]
    # the case holds the tabulated offsets, an offset across an edge and pairs on opposite faces
    d = g[:, None, :] - g[None, :, :]
    r2 = (d * d).sum(axis=2)
    assert {0, 1, 2} <= set(np.unique(r2).tolist())
    normal = np.argmax((g == -1) | (g == np.array(n)), axis=1)  # the direction of the face a ghost lies on
    assert ((r2 == 2) & (normal[:, None] != normal[None, :])).any(), "no pair across an edge"
    for dd in range(3):
        assert (np.abs(d[..., dd]) == n[dd] + 1).any(), f"no pair on the opposite faces of direction {dd}"
    rng = np.random.default_rng(7)
    s = rng.standard_normal(S)
    ps = PoissonSolver(ctx, n, 1.0)
    assert ps.S == S
    ps.s.copy_(dev(ctx, s))
    ps.surface_potential()
    bc = ps.bc.cpu().numpy()
    ref, mag = gr.surface_potential(n, s, return_abs=True)
    worst = (np.abs(bc - ref) / mag).max()
    print(f"n = {n}: S = {S}, max |bc - numpy| / sum|K s| = {worst:.3e}")
    assert np.all(np.abs(bc - ref) <= 1.0e-12 * mag)


# ---------------------------------------------------------------------- the open solve
def test_open_solve_gaussian_and_corner_blob(ctx):
    """16^3: the offset Gaussian plus a blob two cells from a corner.  Step by step against the restatement: the bound of each Dirichlet solve, the
    boundary data through the sum of |K| (an error of s moves bc by at most sum_g' |K(g - g')| times it) and its rounding, then the maximum principle
    for the boundary data of step 4."""
    N = 16
    n = (N, N, N)
    f, h, coords, _ = gr.gaussian_case(N, (0.12, -0.07, 0.05))
    z, y, x = coords
    c = (2 + 0.5) * h - 0.5
    blob = 0.3 * np.exp(-0.5 * ((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) / 0.04 ** 2) / ((2.0 * np.pi) ** 1.5 * 0.04 ** 3)
    gr.fill_rhs(f, gr.interior(blob), 1.0)
    g, nb = gr.ghost_list(n)
    reltol = 1.0e-10
    ps = PoissonSolver(ctx, n, h)
    ps.rhs.copy_(dev(ctx, f))
    # steps by hand
    ps.zero_phi()
    ps.solve_dirichlet(reltol, 0.0)
    phi0 = ps.phi.cpu().numpy()
    r0 = check_dirichlet(n, h, f, np.zeros_like(f), phi0, reltol * np.abs(f).max())
    ps.surface_gather()
    s = ps.s.cpu().numpy()
    assert np.array_equal(s, gr.at(phi0, nb))
    ps.surface_potential()
    bc = ps.bc.cpu().numpy()
    ps.surface_scatter()
    ghosts = np.zeros_like(f)
    gr.put(ghosts, g, bc)
    after_scatter = ps.phi.cpu().numpy()
    assert np.array_equal(gr.at(after_scatter, g), bc) and np.array_equal(gr.interior(after_scatter), gr.interior(phi0))
    ps.solve_dirichlet(reltol, 0.0)
    phi = ps.phi.cpu().numpy()
    r1 = check_dirichlet(n, h, f, ghosts, phi, reltol * np.abs(f).max())
    # against the restatement's open solve
    ref, bc_ref, phi0_ref = gr.open_solve(f, h)
    d = g[:, None, :] - g[None, :, :]
    absK = np.abs(gr.lattice_K(d[..., 0], d[..., 1], d[..., 2]))
    kappa = absK.sum(axis=1).max()
    _, mag = gr.surface_potential(n, gr.at(phi0_ref, nb), return_abs=True)
    res_ref0 = np.abs(gr.residual(phi0_ref, f, h)).max()
    res_ref1 = np.abs(gr.residual(ref, f, h)).max()
    b0 = gr.max_principle_bound(n, h, r0) + gr.max_principle_bound(n, h, res_ref0)
    bound_bc = kappa * b0 + 1.0e-12 * mag.max()
    bound = bound_bc + gr.max_principle_bound(n, h, r1) + gr.max_principle_bound(n, h, res_ref1)
    err_bc, err = np.abs(bc - bc_ref).max(), np.abs(phi - ref).max()
    print(f"open solve: |bc - ref| {err_bc:.3e} (bound {bound_bc:.3e}), |phi - ref| {err:.3e} (bound {bound:.3e}), max |phi| {np.abs(ref).max():.3e}")
    assert err_bc <= bound_bc and err <= bound
    # the driver's entry does the same steps: the same bits
    ps.solve_open(reltol, 0.0)
    assert np.array_equal(ps.phi.cpu().numpy(), phi) and np.array_equal(ps.bc.cpu().numpy(), bc)
    assert ps.cycles[0] > 0 and ps.cycles[1] > 0


# ---------------------------------------------------------------------- right-hand side and kick
def test_rhs_and_kick_bit_for_bit(ctx):
    """two boxes: every cell, so the cells on the box seam and on every domain face (phi(+-1) from the ghost layer), non-zero momenta"""
    n, dx, dt, G = (16, 8, 8), (0.25, 0.25, 0.25), 0.0371, 1.3
    boxes = chop_domain(list(n), [8, 8, 8])
    assert len(boxes) == 2
    lev = Level(ctx, 3, boxes)
    rng = np.random.default_rng(11)
    U = rng.standard_normal((6, n[2], n[1], n[0]))
    U[0] = rng.uniform(0.5, 2.0, size=U[0].shape)
    state = MultiFab(lev, 6, 4, fill=0.0)
    for b, (lo, hi) in enumerate(boxes):
        state.valid(b).copy_(dev(ctx, U[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]))
    ghost_cells_before = [state.fabs[b].cpu().numpy().copy() for b in range(2)]
    ps = PoissonSolver(ctx, n, dx[0])
    f0 = rng.standard_normal(gr.dense_shape(n))
    ps.rhs.copy_(dev(ctx, f0))
    ps.fill_rhs(lev, state, G)
    f = f0.copy()
    gr.fill_rhs(f, U[0], G)
    assert np.array_equal(ps.rhs.cpu().numpy(), f)  # (the ghost layer of rhs included: untouched)
    phi = rng.standard_normal(gr.dense_shape(n))
    ps.phi.copy_(dev(ctx, phi))
    ps.kick(lev, state, dx, dt)
    V = gr.kick(U, phi, dx, dt)
    assert not np.array_equal(V[1:5], U[1:5])
    for b, (lo, hi) in enumerate(boxes):
        got = state.valid(b).cpu().numpy()
        assert np.array_equal(got, V[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]), f"box {b}"
        # ghost cells of the state are not touched
        after = state.fabs[b].cpu().numpy()
        mask = np.ones(after.shape, dtype=bool)
        mask[:, 4:-4, 4:-4, 4:-4] = False
        assert np.array_equal(after[mask], ghost_cells_before[b][mask])
    # the library's refusals: unequal spacing, a 2-D level, a cell count it is not built for
    with pytest.raises(capi.QkError, match="cubic"):
        ps.kick(lev, state, (0.25, 0.25, 0.5), dt)
    lev2 = Level(ctx, 2, [([0, 0, 0], [15, 7, 0])])
    rc = ctx.L.qk_gravity_kick(lev2.h, ctx.stream(), ps._n, ps._p(ps.phi), (C.c_double * 3)(*dx), dt, state.ptr)
    assert rc == capi.QK_ERR_UNSUPPORTED
    rc = ctx.L.qk_gravity_fill_rhs(lev2.h, ctx.stream(), G, state.ptr, 0, ps._n, ps._p(ps.rhs))
    assert rc == capi.QK_ERR_UNSUPPORTED
    with pytest.raises(capi.QkError, match="even cell count"):
        PoissonSolver(ctx, (8, 7, 8), 1.0)


# ---------------------------------------------------------------------- the driver
def gravity_kernel_names(ctx):
    names = []
    for k in range(ctx.L.qk_profile_num_kernels(ctx.h)):
        name, cnt, ms = C.c_char_p(), C.c_long(), C.c_double()
        ctx.check(ctx.L.qk_profile_get(ctx.h, k, C.byref(name), C.byref(cnt), C.byref(ms)), "qk_profile_get")
        if cnt.value > 0 and name.value.decode().startswith("gravity"):
            names.append(name.value.decode())
    return names


def run_steps(ctx, nsteps, setup=None, mgs=(16, 16, 16)):
    sim = hydro_sim(ctx, (16, 16, 16), mgs)
    if setup is not None:
        setup(sim)
    sim.set_initial_conditions(blob_ic(sim))
    dts = []
    for _ in range(nsteps):
        assert sim.step()
        dts.append(sim.dt_)
    return sim, dts, global_state(sim)


def test_driver_switch_off_and_zero_G(ctx):
    ctx.L.qk_profile_reset(ctx.h)
    ctx.L.qk_profile_enable(ctx.h, 1)
    try:
        sim0, dts0, U0 = run_steps(ctx, 3)
        assert gravity_kernel_names(ctx) == [], "the default run launched gravity kernels"
    finally:
        ctx.L.qk_profile_enable(ctx.h, 0)
        ctx.L.qk_profile_reset(ctx.h)
    assert sim0.doPoissonSolve_ == 0 and sim0.phi is None and sim0.poisson is None
    assert sim0.reltolPoisson_ == 1.0e-5 and sim0.abstolPoisson_ == 1.0e-5 and sim0.Gconst_ == 6.67430e-8

    def on_zero_G(sim):
        sim.doPoissonSolve_, sim.Gconst_ = 1, 0.0
    sim1, dts1, U1 = run_steps(ctx, 3, on_zero_G)
    assert sim1.phi is not None and not sim1.phi.any()
    assert dts1 == dts0 and np.array_equal(U1, U0)


def test_driver_blob_replayed(ctx):
    """three steps of a cold blob, two boxes: every solve and kick replayed in numpy from the state seen between them"""
    seen, G = [], 0.05

    def setup(sim):
        sim.doPoissonSolve_, sim.Gconst_ = 1, G
        sim.on_gravity = lambda s, dt: seen.append((dt, global_state(s), s.phi.cpu().numpy().copy(), s.poisson.resnorm, s.poisson.cycles,
                                                    s._signal_of_state_new))
    sim = hydro_sim(ctx, (16, 16, 16), (8, 16, 16))
    assert len(sim.my_boxes) == 2
    setup(sim)
    sim.set_initial_conditions(blob_ic(sim))
    assert sim.phi is not None and not seen  # (the solve after the initial conditions: no kick, no hook)
    n, h = (16, 16, 16), sim.geom.dx[0]
    g, nb = gr.ghost_list(n)
    d = g[:, None, :] - g[None, :, :]
    kappa = np.abs(gr.lattice_K(d[..., 0], d[..., 1], d[..., 2])).sum(axis=1).max()
    for step in range(3):
        assert sim.step()
        assert len(seen) == step + 1
        dt, U, phi, resnorm, cycles, stale = seen[-1]
        assert dt == sim.dt_
        f = np.zeros(gr.dense_shape(n))
        gr.fill_rhs(f, U[0], G)
        assert np.array_equal(sim.poisson.rhs.cpu().numpy(), f)
        tol = max(1.0e-5 * np.abs(f).max(), 1.0e-5 * gr.interior(f).min())
        ref, bc_ref, phi0_ref = gr.open_solve(f, h)
        r1 = np.abs(gr.residual(phi, f, h)).max()
        assert r1 <= tol and resnorm[0] <= tol and resnorm[1] <= tol
        _, mag = gr.surface_potential(n, gr.at(phi0_ref, nb), return_abs=True)
        b0 = gr.max_principle_bound(n, h, resnorm[0]) + gr.max_principle_bound(n, h, np.abs(gr.residual(phi0_ref, f, h)).max())
        bound = kappa * b0 + 1.0e-12 * mag.max() + gr.max_principle_bound(n, h, r1) + gr.max_principle_bound(n, h, np.abs(gr.residual(ref, f, h)).max())
        err = np.abs(phi - ref).max()
        print(f"step {step}: V-cycles {cycles}, |phi - ref| {err:.3e} (bound {bound:.3e}, max |phi| {np.abs(ref).max():.3e})")
        assert err <= bound
        # the kick, given that phi, bit for bit
        V = gr.kick(U, phi, sim.geom.dx, dt)
        got = global_state(sim)
        assert np.array_equal(got, V)
        assert not np.array_equal(got[1:4], U[1:4])
        # the next time step: the maxima the last stage left describe the state before the kick and are dropped
        assert sim._signal_of_state_new is None
        dt_next = sim.computeTimestepAtLevel()
        m = float(sim.hydro.maxSignalSpeedLocal(sim.lev, sim.state_new_cc_, which=1, out=sim.dev_max).item())
        assert dt_next == sim.cflNumber_ * (sim.min_dx() / m)
        if stale is not None:
            assert stale[1] != m, "the kick did not change the signal speed: the check above shows nothing"
            print(f"         dt from the maxima before the kick {sim.cflNumber_ * (sim.min_dx() / stale[1]):.6e}, after {dt_next:.6e}")


def test_driver_refusals(ctx):
    def expect(sim, pattern):
        sim.doPoissonSolve_ = 1
        with pytest.raises(capi.QkError, match=pattern):
            sim.calculateGpotAllLevels()
        assert sim.phi is None

    sim = hydro_sim(ctx, (8, 8, 8), (8, 8, 8))
    sim.set_initial_conditions(blob_ic(sim))
    sim.nranks = 2
    expect(sim, "one rank")
    sim.nranks = 1
    sim.do_cic_particles = 1
    expect(sim, "CIC particles")
    with pytest.raises(capi.QkError, match="CIC particles"):
        sim.step()
    sim.do_cic_particles = 0
    sim.calculateGpotAllLevels()  # (and with nothing in the way it solves)
    assert sim.phi is not None

    expect(hydro_sim(ctx, (8, 8), (8, 8, 1)), "ndim = 3")
    expect(hydro_sim(ctx, (8, 8, 8), (8, 8, 8), prob_hi=(1.0, 1.0, 1.0 + 1.0e-9)), "cubic cells")
    ok = hydro_sim(ctx, (8, 8, 8), (8, 8, 8), prob_hi=(1.0, 1.0, 1.0 + 1.0e-14))  # (equal to 1e-12 relative: accepted)
    ok.set_initial_conditions(blob_ic(ok))
    ok.doPoissonSolve_ = 1
    ok.calculateGpotAllLevels()
    assert ok.phi is not None

    class Derived(HydroSimulation):
        pass
    geom = Geometry(3, [8, 8, 8], [0.0] * 3, [1.0] * 3, [0, 0, 0])
    bcs = [([capi.BC_FOEXTRAP] * 3, [capi.BC_FOEXTRAP] * 3) for _ in range(6)]
    expect(Derived(ctx, geom, capi.traits(5.0 / 3.0, False, 3), bcs, [8, 8, 8]), "not for Derived")

    from quokka_amd.radhydro import matter_coupling_problem
    rad = matter_coupling_problem(ctx)
    expect(rad, "not for RadhydroSimulation")
    with pytest.raises(capi.QkError, match="not for RadhydroSimulation"):
        rad.step()

    from quokka_amd.amr_simulation import sedov_amr_problem
    amr = sedov_amr_problem(ctx, 32, 1, max_grid_size=16, blocking_factor=8)
    expect(amr.levels[0], "not for AmrLevelSim")
    with pytest.raises(capi.QkError, match="not for AmrSimulation"):
        amr.step()
    amr.levels[0].doPoissonSolve_ = 0
    amr.doPoissonSolve_ = 1
    with pytest.raises(capi.QkError, match="not for AmrSimulation"):
        amr.step()
    with pytest.raises(capi.QkError, match="not for AmrSimulation"):
        amr.setInitialConditions()
