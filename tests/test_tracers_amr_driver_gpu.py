"""Tracer particles through the AMR driver (quokka_amd/amr_simulation.py, DESIGN.md §11 "refined levels"): every AdvectWithUmac and every
Redistribute of a run is replayed in numpy (tests/tracer_amr_reference.py) on the fields the driver handed over, bit for bit; the particles are
passive; the schedule keeps every particle on the finest level that covers it; retries roll a level's particles back; refusals."""
import numpy as np
import pytest
import torch

import tracer_amr_reference as ta
import tracer_reference as tr
from quokka_amd import capi
from quokka_amd.amr_simulation import AmrSimulation, sedov_amr_problem
from quokka_amd.simulation import Geometry
from quokka_amd.tracers import CUR, PREV

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


# fine cells [0, 16) x [0, 8)^2 round the blast corner in two boxes: the shock crosses the coarse-fine boundary, four coarse cells out, within ten steps
STATIC_FINE = [([0, 0, 0], [7, 7, 7]), ([8, 0, 0], [15, 7, 7])]


def sedov_hierarchy(ctx, tracers: bool, static=True):
    amr = sedov_amr_problem(ctx, 32, max_level=1, max_grid_size=16, blocking_factor=8, static_fine_boxes=[STATIC_FINE] if static else None)
    if tracers:
        amr.do_tracers = 1
        amr.InitTracerParticles()
    else:  # the path a tracer run takes: the reference-shaped operators on every level, no overlap
        for L in amr.levels:
            L.use_fused = False
    return amr


def ref_geoms(amr):
    g0 = amr.geom0
    base = tr.TracerGeom(3, g0.n_cell[:3], g0.prob_lo[:3], g0.prob_hi[:3], g0.periodic[:3])
    assert base.dx == g0.dx[:3]
    return [ta.level_geom(base, m) for m in range(amr.max_level + 1)]


class Recorder:
    """every advect (with the fields of both kinds of every level involved, copied to the host) and every redistribute of a run, in order.
    A level's retry starts again at the time its dropped attempt started at: an advect of a level that does not lie after the trailing advects
    of the same level replaces them."""

    def __init__(self, amr):
        self.amr, self.geoms, self.events, self.dropped = amr, ref_geoms(amr), [], 0
        self.fallback_moving = 0  # (particle, advect) pairs replayed with a stencil face off the particle's level and a velocity that is not zero
        amr.on_tracer_advect = self.on_advect
        inner = amr.RedistributeTracers

        def redistribute(lev_min=0, ngrow=0):
            self.events.append(("redistribute", lev_min, ngrow, [[(list(lo), list(hi)) for lo, hi in L.my_boxes] for L in amr.levels]))
            inner(lev_min, ngrow)

        amr.RedistributeTracers = redistribute

    def faces(self, m, kind):
        boxes, arrays = self.amr.tracer_fields(m, kind)
        return ta.LevelFaces(self.geoms[m], boxes, [[arrays[d].fab_numpy(b) for b in range(len(boxes))] for d in range(3)])

    def on_advect(self, lev, time, dt, alpha, beta):
        while self.events and self.events[-1][0] == "advect" and self.events[-1][1] == lev and self.events[-1][2] >= time:
            self.events.pop()
            self.dropped += 1
        cur = [self.faces(m, CUR) for m in range(lev + 1)]
        prev = [self.faces(m, PREV) for m in range(lev)] + [None]
        self.events.append(("advect", lev, time, dt, alpha, beta, cur, prev))

    def replay(self, ids, pos, level):
        """the events so far on (ids, pos, level); forgets them"""
        for ev in self.events:
            if ev[0] == "advect":
                _, lev, _time, dt, alpha, beta, cur, prev = ev
                sel = level == lev
                if sel.any():
                    F = ta.compose_field(cur, prev, lev, alpha, beta)
                    if lev > 0:
                        n_off = ta.stencil_classes(cur[lev], F, dt, pos[sel])[1]
                    pos[sel], vel = tr.advect(cur[lev].g, F, dt, pos[sel])
                    if lev > 0:
                        self.fallback_moving += int(((n_off > 0) & (vel != 0.0).any(axis=1)).sum())
            else:
                _, lev_min, ngrow, boxes = ev
                sel = np.flatnonzero(level >= lev_min)
                nlev = len(boxes)
                p, new, keep = ta.where(self.geoms[:nlev], boxes, lev_min, ngrow, pos[sel], np.minimum(level[sel], nlev - 1).astype(np.int32))
                pos[sel], level[sel] = p, new
                gone = sel[~keep]
                ids, pos, level = np.delete(ids, gone), np.delete(pos, gone, axis=0), np.delete(level, gone)
        self.events = []
        return ids, pos, level


def by_id(amr):
    ids, pos, lev = amr.tracer_ids(), amr.tracer_positions(), amr.tracer_levels()
    o = np.argsort(ids, kind="stable")
    return ids[o], pos[o], lev[o]


def assert_finest_covering_level(amr, rec):
    ids, pos, lev = by_id(amr)
    boxes = [L.my_boxes for L in amr.levels]
    _, new, keep = ta.where(rec.geoms[:len(boxes)], boxes, 0, 0, pos, lev)
    assert keep.all() and np.array_equal(new, lev)


def run_and_replay(amr, rec, nsteps, step=None):
    ids, pos, lev = by_id(amr)
    ids0 = ids.copy()
    moved, changed = 0.0, 0
    for it in range(nsteps):
        (step or amr.step)()
        rid, rpos, rlev = rec.replay(ids.copy(), pos.copy(), lev.copy())
        gid, gpos, glev = by_id(amr)
        assert np.array_equal(gid, rid) and np.array_equal(glev, rlev), it
        assert np.array_equal(gpos, rpos), (it, np.abs(gpos - rpos).max())
        assert_finest_covering_level(amr, rec)
        keep = np.isin(ids, gid)
        moved = max(moved, np.abs(gpos - pos[keep]).max())
        changed += int((glev != lev[keep]).sum())
        ids, pos, lev = gid, gpos, glev
    assert np.array_equal(ids, ids0), "ids unchanged as a set (reflecting walls: nothing leaves)"
    return moved, changed


def test_setup_one_particle_per_coarse_cell_on_the_finest_covering_level(ctx):
    amr = sedov_hierarchy(ctx, True)
    g = ref_geoms(amr)
    pos, ids = tr.init_one_per_cell(g[0], amr.levels[0].my_boxes)
    gid, gpos, glev = by_id(amr)
    assert amr.num_tracers == 32 ** 3 and np.array_equal(gid, ids) and np.array_equal(gpos, pos)
    inside = (pos[:, 0] < 8 * g[0].dx[0]) & (pos[:, 1] < 4 * g[0].dx[1]) & (pos[:, 2] < 4 * g[0].dx[2])
    assert np.array_equal(glev, inside.astype(np.int32)) and inside.sum() == 128
    assert amr.levels[1].tracers.num_particles == 128 and amr.levels[0].tracers.num_particles == 32 ** 3 - 128


def test_replay_and_passivity_on_static_grids(ctx):
    """Sedov 32^3 + one static level: positions, levels and ids are the numpy replay's after every coarse step; the states of both levels and
    every dt are those of the same hierarchy on the same path (operators, no overlap) without tracers"""
    ref = sedov_hierarchy(ctx, False)
    amr = sedov_hierarchy(ctx, True)
    rec = Recorder(amr)
    plain = []

    def step():
        ref.step()
        amr.step()
        assert amr.dt_ == ref.dt_
        for l in range(2):
            for b in range(amr.levels[l].lev.nboxes):
                assert torch.equal(amr.levels[l].state_new_cc_.valid(b), ref.levels[l].state_new_cc_.valid(b)), (l, b)
        # level 0, fine, Redistribute(1, 1, 1), fine, Redistribute(0, 1, 0); a level step retried in substeps advects once per substep
        order = []
        for e in rec.events:
            key = (e[0], e[1]) if e[0] == "advect" else (e[0], e[1], e[2])
            if not (order and order[-1] == key and e[0] == "advect"):
                order.append(key)
        assert order == [("advect", 0), ("advect", 1), ("redistribute", 1, 1), ("advect", 1), ("redistribute", 0, 0)], order
        adv = [e for e in rec.events if e[0] == "advect"]
        if len(adv) == 3:  # no substeps: the fine level reads its parent at a quarter and at three quarters of the coarse step
            plain.append(1)
            for e, (al, be) in zip(adv, [(0.0, 1.0), (0.75, 0.25), (0.25, 0.75)]):
                assert abs(e[4] - al) <= 1e-12 and abs(e[5] - be) <= 1e-12, (e[4], e[5])

    moved, changed = run_and_replay(amr, rec, 24, step)
    print(f"largest displacement in one coarse step {moved:.3e} (dx0 = {amr.geom0.dx[0]:.3e}), level changes {changed}, "
          f"moving particles with fallback faces {rec.fallback_moving}")
    assert moved > 0.0 and amr.levels[0].counters["operator_stages"] > 0 and len(plain) > 0
    assert rec.fallback_moving > 0, "the fallback faces never carried a velocity"


def test_regrid_moves_particles_between_levels(ctx):
    """ErrorEst-driven grids, regrid_int = 2, 32^3: the same replay and invariants while the refined region follows the blast; particles
    change level"""
    amr = sedov_hierarchy(ctx, True, static=False)
    assert amr.regrid_int == 2 and amr.finest_level == 1
    rec = Recorder(amr)
    grids0 = sorted(map(str, amr.levels[1].my_boxes))
    moved, changed = run_and_replay(amr, rec, 12)
    print(f"largest displacement in one coarse step {moved:.3e}, level changes {changed}")
    assert sorted(map(str, amr.levels[1].my_boxes)) != grids0, "the grids never changed"
    assert changed > 0 and moved > 0.0


def uniform_hierarchy(ctx, v):
    """16^3 periodic, uniform state moving with v, one static fine box [8, 24)^3 in the middle"""
    geom = Geometry(3, [16] * 3, [0.0] * 3, [1.0] * 3, [1, 1, 1])
    bcs = [([capi.BC_INT_DIR] * 3,) * 2 for _ in range(6)]
    amr = AmrSimulation(ctx, geom, capi.traits(1.4, False, 3), bcs, 1, max_grid_size=16, blocking_factor=8)
    amr.static_fine_boxes = [[([8, 8, 8], [23, 23, 23])]]

    def ic_for(_geom):
        def ic(i, j, k):
            U = np.zeros((6,) + i.shape)
            U[0] = 1.0
            U[1], U[2], U[3] = v
            U[5] = 1.0 / 0.4
            U[4] = U[5] + 0.5 * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            return U
        return ic

    amr.initial_conditions = ic_for
    amr.do_tracers = 1
    amr.setInitialConditions()
    return amr


def test_uniform_flow_crosses_the_coarse_fine_boundary_both_ways(ctx):
    """Every tracer sits at its start + v t, wrapped, while tracers enter and leave the fine box.

    The bound is built as in tests/test_tracers_gpu.py::test_uniform_flow_carries_every_tracer_by_v_t, with the deviation of the face
    velocities MEASURED per advect call instead of derived (reflux and average-down leave a uniform state uniform only to rounding):
      delta = the largest |u - v_d| over every face array handed over (the level's own, and the parent's prev and cur);
      a fallback face: alpha u_p + beta u_c with alpha + beta = 1 rounds two products and a sum (1.5 eps |v|), rule 3 with w in {0, 1/2} has
        exact products and one rounded sum (0.5 eps |v|)                                          -> delta + 2 eps |v|
      the interpolation, weights that add up to 1 (tests/test_tracer_reference.py)              -> + 17.5 eps |v|
      x + dt v1: product and sum round once each, 0.5 eps dt |v1| + 0.5 eps L, and the periodic shift of the Redistribute that follows
        once more, 0.5 eps L   (L = 1 >= |x|)
    summed over ALL advect calls (a particle takes the coarse one or the two fine ones of a coarse step, never all three: an upper bound).
    The start is taken after the first coarse step: before it `prev` of level 0 is zero, which the fine level's first two advects blend in.
    Expected value: three roundings of numbers <= 2 L, and T = tNew - t0 with tNew a sum of 13 rounded terms."""
    v = (0.3, -0.2, 0.1)
    amr = uniform_hierarchy(ctx, v)
    rec = Recorder(amr)
    amr.step()  # (prev of level 0 is zero before its first step: the fine level's first two advects blend it in; the test starts after them)
    rec.events = []
    ids, start, lev0 = by_id(amr)
    t0 = amr.tNew_
    bound = np.full(3, 3.0 * EPS * 2.0)
    worst = np.zeros(3)
    changed = 0
    lev = lev0
    for it in range(12):
        amr.step()
        for ev in rec.events:
            if ev[0] != "advect":
                continue
            _, l, _time, dt, alpha, beta, cur, prev = ev
            for d in range(3):
                delta = max(np.abs(np.asarray(f) - v[d]).max() for LF in cur + [p for p in prev if p is not None] for f in LF.fabs[d])
                worst[d] = max(worst[d], delta)
                dev = delta + (2.0 + 17.5) * EPS * abs(v[d])
                bound[d] += dt * dev + 0.5 * EPS * dt * (abs(v[d]) + dev) + EPS * 1.0
        rec.events = []
        gid, gpos, glev = by_id(amr)
        assert np.array_equal(gid, ids)
        changed_now = glev != lev
        changed += int(changed_now.sum())
        lev = glev
        assert_finest_covering_level(amr, rec)
    up, down = int(((lev0 == 0) & (lev == 1)).sum()), int(((lev0 == 1) & (lev == 0)).sum())
    T = amr.tNew_ - t0
    print(f"{changed} level changes, {up} coarse -> fine and {down} fine -> coarse over the run")
    assert up > 0 and down > 0
    for d in range(3):
        expect = np.mod(start[:, d] + v[d] * T, 1.0)
        diff = np.abs(gpos[:, d] - expect)
        diff = np.minimum(diff, 1.0 - diff)
        b = bound[d] + 7.0 * EPS * abs(v[d]) * amr.tNew_
        print(f"direction {d}: face velocities within {worst[d] / (EPS * abs(v[d])):.1f} eps |v| of v; max error {diff.max():.3e}, bound {b:.3e}")
        assert diff.max() <= b


def test_a_retry_on_the_fine_level_starts_from_the_snapshot(ctx):
    """an over-CFL coarse step (6 dt, as tests/test_tracers_gpu.py forces one): the levels retry with substeps; the positions are the replay of
    only the attempts that stood"""
    amr = sedov_hierarchy(ctx, True)
    for _ in range(3):
        amr.step()
    rec = Recorder(amr)
    restores = []
    fine = amr.levels[1].tracers
    inner = fine.restore

    def restore(snap):
        snap_pos = torch.stack(snap["pos"], dim=1).cpu().numpy()
        restores.append(not np.array_equal(fine.positions(), snap_pos))  # the dropped attempt had moved the particles?
        inner(snap)
        assert np.array_equal(fine.positions(), snap_pos)

    fine.restore = restore
    retries_before = amr.levels[1].counters["retries"]

    def step():
        amr.computeTimestep()
        amr.dt_ = [6.0 * dt for dt in amr.dt_]
        amr.timeStepWithSubcycling(0, amr.tNew_)
        amr.tNew_ += amr.dt_[0]

    run_and_replay(amr, rec, 1, step)
    retries = amr.levels[1].counters["retries"] - retries_before
    print(f"retries on level 1: {retries}, on level 0: {amr.levels[0].counters['retries']}, advect events dropped {rec.dropped}")
    assert retries > 0 and len(restores) == retries and rec.dropped > 0
    assert any(restores), "no dropped attempt had moved the particles"


def test_refusals(ctx):
    amr = sedov_hierarchy(ctx, False)
    amr.do_tracers = 1
    with pytest.raises(capi.QkError, match="AMR driver.*setInitialConditions"):
        amr.step()
    amr.integratorOrder_ = 1
    with pytest.raises(capi.QkError, match="integratorOrder_"):
        amr.InitTracerParticles()
    amr.integratorOrder_ = 2
    amr.nranks = 2
    with pytest.raises(capi.QkError, match="nranks"):
        amr.InitTracerParticles()
    amr.nranks = 1
    amr.rad_traits = object()
    with pytest.raises(capi.QkError, match="RadAmrLevelSim"):
        amr.InitTracerParticles()
    amr.rad_traits = None
    amr.InitTracerParticles()
    amr.levels[1].tracers_on_fused_stages = 1
    with pytest.raises(capi.QkError, match="tracers_on_fused_stages"):
        amr.step()
    amr.levels[1].tracers_on_fused_stages = 0
    amr.levels[1].integratorOrder_ = 1
    with pytest.raises(capi.QkError, match="integratorOrder_"):
        amr.step()
    amr.levels[1].integratorOrder_ = 2
    amr.overlap_children = True
    assert amr._overlap_split(0) is None  # no children beside the far boxes with tracers
    amr.step()
    assert amr.num_tracers == 32 ** 3


def test_a_rad_level_is_refused_by_name(ctx):
    from quokka_amd.amr_simulation import RadAmrLevelSim
    L = RadAmrLevelSim.__new__(RadAmrLevelSim)
    L.nranks, L.integratorOrder_, L.tracers_on_fused_stages = 1, 2, 0
    with pytest.raises(capi.QkError, match="RadAmrLevelSim"):
        L._check_tracers()
