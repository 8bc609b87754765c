"""Tracer particles on the GPU (csrc/qk_tracer.hip, quokka_amd/tracers.py) against the numpy restatement of tests/tracer_reference.py, bit
for bit: the kernels on random face fields, then through the driver (uniform flow, passivity, retries, outflow, refusals)."""
import types

import numpy as np
import pytest
import torch

import tracer_reference as tr
from quokka_amd import capi
from quokka_amd.multifab import Level, MultiFab
from quokka_amd.simulation import Geometry, HydroSimulation, chop_domain, sedov_problem
from quokka_amd.tracers import TracerParticles

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------- helpers
def make_container(ctx, geom: Geometry, mgs):
    """a TracerParticles on a bare level (no hydro state): (container, boxes, restatement geometry)"""
    boxes = chop_domain(geom.n_cell, (list(mgs) + [1, 1])[:3])
    lev = Level(ctx, geom.ndim, boxes)
    host = types.SimpleNamespace(ctx=ctx, lev=lev, geom=geom, rank=0)
    return TracerParticles(host), boxes, ref_geom(geom)


def ref_geom(geom: Geometry) -> tr.TracerGeom:
    nd = geom.ndim
    g = tr.TracerGeom(nd, geom.n_cell[:nd], geom.prob_lo[:nd], geom.prob_hi[:nd], geom.periodic[:nd])
    assert g.dx == geom.dx[:nd]
    return g


def upload_faces(lev, g, boxes, umac_global):
    out = []
    for d in range(g.ndim):
        mf = MultiFab(lev, 1, 0, facedir=d)
        for b, (lo, hi) in enumerate(boxes):
            mf.set_fab(b, tr.box_faces(g, umac_global[d], d, lo, hi))
        out.append(mf)
    return out


def download_faces(g, boxes, umac):
    return [tr.assemble_faces(g, d, boxes, [umac[d].fab_numpy(b) for b in range(len(boxes))]) for d in range(g.ndim)]


def sample_particles(g: tr.TracerGeom, boxes, rng, n_random=200):
    """cell centres, points exactly on faces, edges and the domain corners, points within one ulp of box boundaries, random ones"""
    nd = g.ndim
    lo, hi = np.array(g.prob_lo), np.array(g.prob_hi)
    dx = np.array(g.dx)
    n = np.array(g.n_cell)
    rand = lambda m: lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(m, nd))
    centres = lo + (rng.integers(0, n, size=(150, nd)) + 0.5) * dx
    on_face = rand(100)
    for p in on_face:  # one coordinate on a face (0 .. N: the domain faces included)
        e = rng.integers(0, nd)
        p[e] = lo[e] + rng.integers(0, n[e] + 1) * dx[e]
    on_edge = rand(60)
    for p in on_edge:  # two coordinates on faces
        for e in rng.choice(nd, size=min(2, nd), replace=False):
            p[e] = lo[e] + rng.integers(0, n[e] + 1) * dx[e]
    corners = np.array([[(lo[e], hi[e])[(c >> e) & 1] for e in range(nd)] for c in range(2 ** nd)])
    near = rand(100)
    edges = [sorted({b[0][e] for b in boxes} | {b[1][e] + 1 for b in boxes}) for e in range(nd)]
    for m, p in enumerate(near):  # one ulp to either side of a box boundary
        e = rng.integers(0, nd)
        xb = lo[e] + edges[e][rng.integers(0, len(edges[e]))] * dx[e]
        p[e] = np.nextafter(xb, np.inf if m % 2 else -np.inf)
    return np.ascontiguousarray(np.concatenate([centres, on_face, on_edge, corners, near, rand(n_random)], axis=0))


CASES_3D = [((8, 8, 8), (4, 4, 4)), ((12, 8, 8), (8, 8, 8))]  # eight 4^3 boxes; a remainder box (6 + 6 of max_grid_size 8)
BCS = {"periodic": (1, 1, 1), "outflow": (0, 0, 0), "mixed": (1, 0, 0)}


def kernel_case_inputs(g: tr.TracerGeom, boxes, seed):
    """random global face arrays, the particles, and dt such that the fastest half-step displacement is 1.5 cells: stencil indices then land up
    to two beyond the domain on both sides (asserted, from the inputs alone)"""
    rng = np.random.default_rng(seed)
    umac_global = tr.random_faces(g, rng)
    pos = sample_particles(g, boxes, rng)
    v0 = tr.interp_all(g, umac_global, pos)
    dt = 3.0 * min(g.dx) / np.abs(v0).max()
    xm = pos + (0.5 * dt) * v0
    for e in range(g.ndim):
        i0 = np.floor((xm[:, e] - g.prob_lo[e]) * g.dxi[e] - 0.5)  # the transverse stencil's low index
        assert i0.min() <= -2 and i0.max() + 1 >= g.n_cell[e] + 1, (e, i0.min(), i0.max())
    return umac_global, pos, dt


def run_kernel_case(ctx, geom, mgs, seed):
    tp, boxes, g = make_container(ctx, geom, mgs)
    umac_global, pos, dt = kernel_case_inputs(g, boxes, seed)
    umac = upload_faces(tp.lev, g, boxes, umac_global)
    tp.load(pos, np.zeros_like(pos), np.arange(1, pos.shape[0] + 1))
    tp.advect(umac, dt)
    xr, vr = tr.advect(g, umac_global, dt, pos)
    xg, vg = tp.positions(), tp.velocities()
    assert np.array_equal(vg, vr), f"vel: {np.abs(vg - vr).max()} at {np.argwhere(vg != vr)[:5].tolist()}"
    assert np.array_equal(xg, xr), f"pos: {np.abs(xg - xr).max()}"
    tp.redistribute()
    pr, keep = tr.redistribute(g, xr)
    assert np.array_equal(tp.last_keep.cpu().numpy(), keep)
    assert np.array_equal(tp.positions(), pr[keep]) and np.array_equal(tp.ids(), np.arange(1, pos.shape[0] + 1)[keep])
    assert np.array_equal(tp.velocities(), vr[keep]) and tp.num_particles == int(keep.sum())
    return tp


@pytest.mark.parametrize("bc", list(BCS))
@pytest.mark.parametrize("n_cell,mgs", CASES_3D)
def test_kernel_3d_matches_restatement(ctx, n_cell, mgs, bc):
    geom = Geometry(3, list(n_cell), [-0.3, 0.1, 0.25], [0.9, 1.0, 1.05], list(BCS[bc]))
    tp = run_kernel_case(ctx, geom, mgs, seed=11)
    assert tp.lattice() == ([4, 4, 4], 8) if n_cell == (8, 8, 8) else tp.lattice() == ([6, 8, 8], 2)


@pytest.mark.parametrize("bc", list(BCS))
def test_kernel_2d_matches_restatement(ctx, bc):
    geom = Geometry(2, [8, 8], [-0.3, 0.1, 0.0], [0.9, 1.0, 1.0], list(BCS[bc]))
    run_kernel_case(ctx, geom, (4, 4), seed=12)


def test_kernel_with_a_lattice_too_large_for_lds(ctx):
    """130 x 66 cells in boxes of at most 8: edges 8 and 7 long, granularity 1, 8580 lattice entries (> 4096): the kernel that reads the
    lattice from global memory; same checks"""
    geom = Geometry(2, [130, 66], [0.0, 0.0, 0.0], [1.3, 0.66, 1.0], [1, 0, 0])
    tp = run_kernel_case(ctx, geom, (8, 8), seed=13)
    assert tp.lattice() == ([1, 1, 1], 130 * 66)


def test_init_one_per_cell(ctx):
    sim = sedov_problem(ctx, 12, max_grid_size=[8, 4, 12], n_cell=[12, 8, 12])
    sim.do_tracers = 1
    sim.InitTracerParticles()
    t = sim.tracers
    g = ref_geom(sim.geom)
    pos, ids = tr.init_one_per_cell(g, sim.my_boxes)
    assert t.num_particles == sim.CountCells() == 12 * 8 * 12
    assert np.array_equal(t.positions(), pos) and np.array_equal(t.ids(), ids) and ids[0] == 1 and ids[-1] == sim.CountCells()
    assert not t.velocities().any() and not t.cpu.cpu().numpy().any()
    snap = t.snapshot()
    t.load(pos[:5] + 0.01, pos[:5], ids[:5])
    assert t.num_particles == 5
    t.restore(snap)
    assert np.array_equal(t.positions(), pos) and np.array_equal(t.ids(), ids)


# ---------------------------------------------------------------------- through the driver
def uniform_sim(ctx, ndim, n, mgs, vel, periodic, P=1.0):
    geom = Geometry(ndim, [n] * ndim, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [periodic] * 3)
    bc = capi.BC_INT_DIR if periodic else capi.BC_FOEXTRAP
    bcs = [([bc if d < ndim else capi.BC_INT_DIR for d in range(3)],) * 2 for _ in range(6)]
    sim = HydroSimulation(ctx, geom, capi.traits(1.4, False, ndim), bcs, [mgs] * ndim, use_fused=False)
    sim.do_tracers = 1
    v = list(vel) + [0.0] * (3 - len(vel))

    def ic(i, j, k):
        U = np.zeros((6,) + i.shape)
        U[0] = 1.0
        U[1], U[2], U[3] = v[0], v[1], v[2]
        U[5] = P / 0.4
        U[4] = U[5] + 0.5 * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return U

    sim.set_initial_conditions(ic)
    return sim


def record_advects(sim, g):
    """wrap sim.tracers.advect: every call leaves (global face arrays, dt) in the returned list"""
    calls = []
    inner = sim.tracers.advect

    def advect(umac, dt):
        calls.append((download_faces(g, sim.my_boxes, umac), dt))
        inner(umac, dt)

    sim.tracers.advect = advect
    return calls


def replay(g, pos, calls):
    for umac, dt in calls:
        pos, _ = tr.advect(g, umac, dt, pos)
    return tr.redistribute(g, pos)


def test_uniform_flow_carries_every_tracer_by_v_t(ctx):
    """16^3 periodic in 8^3 boxes, uniform state (rho = 1, P = 1) moving with v: after 10 steps every tracer sits at its start + v t, wrapped.

    What the driver must hand to AdvectWithUmac is v itself to within k eps |v_d|, asserted on every recorded call before anything else.  k from
    HLLC on a uniform subsonic state (csrc/qk_device.hpp hllc / faceFlux; every division there is correctly rounded), in units of eps |u|, with
    A = S_L - u < 0 < B = S_R - u, |A|, |B| >= c and r = |u| / c:
      S_star = (rho u A - rho u B) / (rho A - rho B), the SAME floating A and B above and below, so only the roundings count: the two products
        of each numerator term (1, weighted by (|A| + |B|) / |A - B| = 1), its subtraction (0.5), the denominator's products (0.5) and
        subtraction (0.5), the division (0.5)                                                                            -> 3
      F_rho = S_star (S_K rho - u rho) / (S_K - S_star): the two products (0.5 (|S_K| + |u|) / c <= r + 0.5) and their difference (0.5), the
        product with S_star (0.5) and S_star's own error (3), the denominator's rounding (0.5) and its distance from S_K - u
        (|u| 3 eps / c = 3 r), the division (0.5)                                                                        -> 5.5 + 4 r
      v_norm = F_rho / rho with rho = 1, and 0.5 v1 + 0.5 v2 of two equal numbers: exact.  The fluxes of a uniform state are the same at every
      face, so the state stays uniform bit for bit and (rho, m) never change.
    Then per step and direction:
      |v1 - v_d| <= (k + 17.5) eps |v_d|        (17.5: weights that add up to 1, tests/test_tracer_reference.py)
      x + dt v1: the product and the sum round once each: 0.5 eps dt |v1| + 0.5 eps L, the periodic shift once more: 0.5 eps L   (L = 1 >= |x|)
    and the expected value start + v * t, wrapped, is itself computed with three roundings of numbers <= 2 L."""
    v = (0.3, -0.2, 0.1)
    sim = uniform_sim(ctx, 3, 16, 8, v, periodic=1)
    g = ref_geom(sim.geom)
    calls = record_advects(sim, g)
    start = sim.tracers.positions()
    n0 = sim.tracers.num_particles
    assert n0 == 16 ** 3
    for _ in range(10):
        assert sim.step()
    assert sim.tracers.num_particles == n0 and len(calls) == 10 and np.array_equal(sim.tracers.ids(), np.arange(1, n0 + 1))
    pos = sim.tracers.positions()
    c_sound = np.sqrt(1.4 * 1.0 / 1.0)
    for d in range(3):
        k = 5.5 + 4.0 * abs(v[d]) / c_sound
        bound = 3.0 * EPS * 2.0 + 5.0 * EPS * abs(v[d]) * sim.tNew_  # (the expected value; tNew_ is a sum of 10 rounded terms)
        for umac, dt in calls:
            delta = np.abs(umac[d] - v[d]).max()
            print(f"direction {d}: face velocities within {delta / (EPS * abs(v[d])):.2f} eps |v| of v (k = {k:.2f})")
            assert delta <= k * EPS * abs(v[d])
            bound += dt * (k + 17.5) * EPS * abs(v[d]) + 0.5 * EPS * dt * abs(v[d]) * (1.0 + k * EPS) + EPS * 1.0
        expect = np.mod(start[:, d] + v[d] * sim.tNew_, 1.0)
        diff = np.abs(pos[:, d] - expect)
        diff = np.minimum(diff, 1.0 - diff)  # (a tracer within rounding of the periodic face may sit on either side of it)
        print(f"direction {d}: max error {diff.max():.3e}, bound {bound:.3e}")
        assert diff.max() <= bound
        assert (pos[:, d] >= 0.0).all() and (pos[:, d] < 1.0).all()


def test_tracers_are_passive_and_follow_the_recorded_face_velocities(ctx):
    """Sedov 16^3 in 8^3 boxes, 5 steps: the state and every dt are those of the operator-path run without tracers, bit for bit; the field of each
    AdvectWithUmac call is 0.5 v1 + 0.5 v2 of the two stages' face velocities; the positions after every step are the restatement's, replayed on
    the face velocities and dt of each call"""
    ref = sedov_problem(ctx, 16, max_grid_size=8, use_fused=False)
    sim = sedov_problem(ctx, 16, max_grid_size=8)  # (use_fused as by default: with tracers both stages take the operator path)
    sim.do_tracers = 1
    sim.InitTracerParticles()
    g = ref_geom(sim.geom)
    calls = record_advects(sim, g)
    pos = sim.tracers.positions()
    moved = 0.0
    for step in range(5):
        assert ref.step() and sim.step()
        assert sim.dt_ == ref.dt_, step
        for b in range(sim.lev.nboxes):
            assert torch.equal(sim.state_new_cc_.valid(b), ref.state_new_cc_.valid(b)), (step, b)
        assert len(calls) == 1
        # what the driver handed over is the RK2 average of the two stages' face velocities, face by face: neither stage's own
        v1 = download_faces(g, sim.my_boxes, sim.halfVel)
        v2 = download_faces(g, sim.my_boxes, sim._tmp()["vel"])
        for d in range(3):
            assert np.array_equal(calls[0][0][d], 0.5 * v1[d] + 0.5 * v2[d]), (step, d)
            assert not np.array_equal(calls[0][0][d], v2[d]) and not np.array_equal(calls[0][0][d], v1[d])
        assert sim.counters["fofc1_stages"] == sim.counters["fofc2_stages"] == 0  # (a correction would replace faces of the average)
        new, keep = replay(g, pos, calls)
        calls.clear()
        assert keep.all()
        assert np.array_equal(sim.tracers.positions(), new), step
        moved = max(moved, np.abs(new - pos).max())
        pos = new
    assert moved > 0.0


def test_retries_roll_the_tracers_back(ctx):
    """the over-CFL step of tests/test_hydro_step_gpu.py::test_fofc_and_retries_match_oracle: the positions are the replay of ONLY the sub-steps
    of the attempt that succeeded, started from the particles as they were before the step"""
    sim = sedov_problem(ctx, 16, max_grid_size=8)
    sim.do_tracers = 1
    sim.InitTracerParticles()
    g = ref_geom(sim.geom)
    for _ in range(3):
        assert sim.step()
    dt = sim.computeTimestepAtLevel() * 6.0
    calls = record_advects(sim, g)
    restores = []
    inner_restore = sim.tracers.restore

    def restore(snap):  # every retry starts here: what was recorded so far belongs to a dropped attempt
        restores.append(len(calls))
        calls.clear()
        inner_restore(snap)

    sim.tracers.restore = restore
    before = sim.tracers.positions()
    assert sim.step(dt)
    assert sim.counters["retries"] > 0 and len(restores) == sim.counters["retries"]
    assert len(calls) == 2 ** sim.counters["retries"]  # the substeps of the successful attempt
    assert abs(sum(c[1] for c in calls) - dt) <= 4 * EPS * dt
    new, keep = replay(g, before, calls)
    assert keep.all() and np.array_equal(sim.tracers.positions(), new)
    print(f"retries {sim.counters['retries']}, advect calls dropped per retry {restores}")


def test_outflow_drops_exactly_the_tracers_that_left(ctx):
    """2-D 16^2, outflow boundaries, uniform supersonic state moving in +x: run until the first column of tracers has left through the top x face"""
    sim = uniform_sim(ctx, 2, 16, 8, (1.0, 0.0), periodic=0, P=0.01)
    g = ref_geom(sim.geom)
    calls = record_advects(sim, g)
    n0 = sim.tracers.num_particles
    assert n0 == 256
    pos, ids = sim.tracers.positions(), sim.tracers.ids()
    for step in range(40):
        assert sim.step()
        new, keep = replay(g, pos, calls)
        calls.clear()
        left = new[:, 0] >= g.prob_hi[0]
        assert np.array_equal(~keep, left)  # nothing leaves any other way
        pos, ids = new[keep], ids[keep]
        assert sim.tracers.num_particles == len(ids)
        assert np.array_equal(sim.tracers.ids(), ids)  # the survivors, in their order
        assert np.array_equal(sim.tracers.positions(), pos)
        if len(ids) < n0:
            break
    assert len(ids) == n0 - 16, "one column of 16 tracers leaves first"
    assert np.all(np.diff(ids) > 0)


def test_refusals(ctx):
    sim = sedov_problem(ctx, 16, max_grid_size=8)
    sim.do_tracers = 1
    sim.integratorOrder_ = 1
    with pytest.raises(capi.QkError, match="integratorOrder_"):
        sim.InitTracerParticles()
    sim.integratorOrder_ = 2
    sim.InitTracerParticles()
    sim.integratorOrder_ = 1
    with pytest.raises(capi.QkError, match="integratorOrder_"):
        sim.step()
    late = sedov_problem(ctx, 16, max_grid_size=8)
    late.do_tracers = 1
    with pytest.raises(capi.QkError, match="do_tracers"):
        late.step()
    from quokka_amd.amr_simulation import AmrSimulation
    amr = AmrSimulation(ctx, sim.geom, sim.traits, [], max_level=0)
    amr.do_tracers = 1
    with pytest.raises(capi.QkError, match="AMR driver"):
        amr.step()
