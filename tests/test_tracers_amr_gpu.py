"""Tracer kernels on a refined hierarchy (csrc/qk_tracer.hip: qk_tracer_plan_create_refined, the parent links, qk_tracer_Where) through the C-ABI
against the numpy restatement of tests/tracer_amr_reference.py, bit for bit: hand-made boxes, random face fields."""
import functools
import types

import numpy as np
import pytest
import torch

import tracer_amr_reference as ta
import tracer_reference as tr
from quokka_amd import capi
from quokka_amd.multifab import Level, MultiFab
from quokka_amd.simulation import Geometry, chop_domain
from quokka_amd.tracers import CUR, PREV, TracerParticles, TracerPlan, where

pytestmark = pytest.mark.gpu


def cube(lo, hi):
    return (list(lo), list(hi))


def halves_x(lo, hi):
    """the box [lo, hi] in two boxes, cut in x"""
    mid = (lo[0] + hi[0] + 1) // 2
    return [cube(lo, [mid - 1, hi[1], hi[2]]), cube([mid, lo[1], lo[2]], hi)]


# name -> (ndim, level-0 cells, periodicity, boxes per level of `cur`, boxes per level of `prev` (levels below the finest), particle level)
L0_3D = chop_domain([16, 16, 16], [8, 8, 8])
L0_3D_PREV = chop_domain([16, 16, 16], [16, 8, 16])  # the previous step's level 0 had other boxes
CASES = {
    "interior": (3, 16, (0, 0, 0), [L0_3D, halves_x([8, 8, 8], [23, 23, 23])], [L0_3D_PREV]),
    "low_x_periodic": (3, 16, (1, 0, 0), [L0_3D, halves_x([0, 8, 8], [15, 23, 23])], [L0_3D_PREV]),
    "low_x_outflow": (3, 16, (0, 0, 0), [L0_3D, halves_x([0, 8, 8], [15, 23, 23])], [L0_3D_PREV]),
    "2d": (2, 32, (0, 1, 0), [chop_domain([32, 32, 1], [16, 16, 1]), halves_x([16, 16, 0], [47, 39, 0])], [chop_domain([32, 32, 1], [32, 16, 1])]),
    # level 2 flush against level 1's high-x edge (fine cell 23 = level-2 cell 47): not properly nested; prev of level 1 had one box, shifted
    "three_levels": (3, 16, (0, 0, 0), [L0_3D, halves_x([8, 8, 8], [23, 23, 23]), [cube([32, 24, 24], [47, 39, 39])]],
                     [L0_3D_PREV, [cube([10, 8, 8], [25, 23, 19])]]),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name, seed=21):
    """geometries, random fields of both kinds on every level, 4096 particles uniform in the finest level's boxes grown by three of its cells,
    dt such that the fastest half-step is 1.5 cells; computed once per case and shared (nothing changes them)"""
    ndim, n0, per, cur_boxes, prev_boxes = CASES[name]
    rng = np.random.default_rng(seed)
    n_cell = [n0] * ndim + [1] * (3 - ndim)
    g0 = tr.TracerGeom(ndim, n_cell[:ndim], [-0.3, 0.1, 0.25][:ndim], [0.9, 1.3, 1.45][:ndim], list(per[:ndim]))
    lev = len(cur_boxes) - 1
    geoms = [ta.level_geom(g0, m) for m in range(lev + 1)]
    fields = {}
    for kind, boxes in ((CUR, cur_boxes), (PREV, prev_boxes)):
        for m, bx in enumerate(boxes):
            fields[kind, m] = tr.random_faces(geoms[m], rng)
    g = geoms[lev]
    lo = np.array([min(b[0][e] for b in cur_boxes[lev]) for e in range(ndim)]) - 3
    hi = np.array([max(b[1][e] for b in cur_boxes[lev]) for e in range(ndim)]) + 1 + 3
    pos = np.array(g.prob_lo) + (lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(4096, ndim))) * np.array(g.dx)
    return g0, geoms, fields, np.ascontiguousarray(pos)


def level_faces(geoms, boxes, fields, kind):
    return [ta.LevelFaces(geoms[m], boxes[m], [[tr.box_faces(geoms[m], fields[kind, m][d], d, lo, hi) for lo, hi in boxes[m]]
                                               for d in range(geoms[m].ndim)]) for m in range(len(boxes))]


@functools.lru_cache(maxsize=None)
def case_reference(name, alpha, beta):
    """the restatement's answer, and the classes of stencils the particles fall into (asserted: a condition on the inputs, not a tolerance)"""
    ndim, n0, per, cur_boxes, prev_boxes = CASES[name]
    g0, geoms, fields, pos = case_inputs(name)
    lev = len(cur_boxes) - 1
    cur = level_faces(geoms, cur_boxes, fields, CUR)
    prev = level_faces(geoms, prev_boxes, fields, PREV) + [None]
    F = ta.compose_field(cur, prev, lev, alpha, beta)
    v0 = tr.interp_all(geoms[lev], F, pos)
    dt = 3.0 * min(geoms[lev].dx) / np.abs(v0).max()
    x, v = tr.advect(geoms[lev], F, dt, pos)
    n_held, n_off, odd, even = ta.stencil_classes(cur[lev], F, dt, pos)
    classes = {"on": int(((n_off == 0)).sum()), "straddling": int(((n_off > 0) & (n_held > 0)).sum()), "off": int((n_held == 0).sum()),
               "odd": int(odd.sum()), "even": int(even.sum())}
    return dt, x, v, classes


class GpuHierarchy:
    """levels, plans and face arrays of both kinds on the device, linked as the driver links them"""

    def __init__(self, ctx, name):
        ndim, n0, per, cur_boxes, prev_boxes = CASES[name]
        g0, geoms, fields, _ = case_inputs(name)
        self.keep = []
        self.geoms = [Geometry(ndim, list(geoms[m].n_cell) + [1] * (3 - ndim), list(g0.prob_lo) + [0.0] * (3 - ndim), list(g0.prob_hi) + [1.0] * (3 - ndim),
                               list(per)) for m in range(len(geoms))]
        for m, g in enumerate(geoms):
            assert g.dx == self.geoms[m].dx[:ndim]
        self.plans, self.arrays = {}, {}
        for kind, boxes in ((CUR, cur_boxes), (PREV, prev_boxes)):
            for m, bx in enumerate(boxes):
                lev = Level(ctx, ndim, bx)
                self.plans[kind, m] = TracerPlan(ctx, lev, self.geoms[m], refined=m > 0, boxes=bx)
                arrs = []
                for d in range(ndim):
                    mf = MultiFab(lev, 1, 0, facedir=d)
                    for b, (lo, hi) in enumerate(bx):
                        mf.set_fab(b, tr.box_faces(geoms[m], fields[kind, m][d], d, lo, hi))
                    arrs.append(mf)
                self.arrays[kind, m] = arrs
        self.lev = len(cur_boxes) - 1
        for m in range(1, self.lev + 1):
            for kind in (CUR, PREV):
                if (kind, m) in self.plans:
                    for k in (CUR, PREV):
                        self.plans[kind, m].set_parent(k, self.plans[k, m - 1], self.arrays[k, m - 1])
        host = types.SimpleNamespace(ctx=ctx, lev=self.plans[CUR, self.lev].lev, geom=self.geoms[self.lev], rank=0, my_boxes=cur_boxes[self.lev])
        self.tp = TracerParticles(host, refined=True)
        self.tp.plan = self.plans[CUR, self.lev]

    def advect(self, pos, alpha, beta, dt):
        self.plans[CUR, self.lev].set_time_weights(alpha, beta)
        self.tp.load(pos, np.zeros_like(pos), np.arange(1, pos.shape[0] + 1))
        self.tp.advect(self.arrays[CUR, self.lev], dt)
        return self.tp.positions(), self.tp.velocities()


def check_case(ctx, name, alpha, beta):
    dt, xr, vr, classes = case_reference(name, alpha, beta)
    print(name, (alpha, beta), classes)
    assert min(classes.values()) > 0, classes
    H = GpuHierarchy(ctx, name)
    xg, vg = H.advect(case_inputs(name)[3], alpha, beta, dt)
    bad = np.argwhere(vg != vr)
    assert np.array_equal(vg, vr), f"vel: {len(bad)} differ, first {bad[:5].tolist()}, max {np.nanmax(np.abs(vg - vr))}"
    assert np.array_equal(xg, xr)


@pytest.mark.parametrize("name", list(CASES))
def test_advect_on_a_refined_level_matches_restatement(ctx, name):
    check_case(ctx, name, 0.75, 0.25)


@pytest.mark.parametrize("alpha,beta", [(0.25, 0.75), (0.0, 1.0), (1.0, 0.0)])
def test_time_weights_and_short_cuts(ctx, alpha, beta):
    check_case(ctx, "interior", alpha, beta)
    if alpha in (0.0, 1.0):  # the short cut reads one kind alone: the answer differs from the other kind's
        assert not np.array_equal(case_reference("interior", alpha, beta)[2], case_reference("interior", beta, alpha)[2])


def test_a_refined_level_that_tiles_the_domain_takes_todays_kernel_and_bits(ctx):
    """boxes that cover the domain: no holes, no link needed, the single-level kernel's answer"""
    g = tr.TracerGeom(3, [8, 8, 8], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1, 0, 0])
    geom = Geometry(3, [8, 8, 8], [0.0] * 3, [1.0] * 3, [1, 0, 0])
    boxes = [cube([0, 0, 0], [3, 7, 7]), cube([4, 0, 0], [7, 7, 3]), cube([4, 0, 4], [7, 7, 7])]
    rng = np.random.default_rng(4)
    u = tr.random_faces(g, rng)
    pos = rng.uniform(-0.1, 1.1, size=(1000, 3))
    lev = Level(ctx, 3, boxes)
    tp = TracerParticles(types.SimpleNamespace(ctx=ctx, lev=lev, geom=geom, rank=0), refined=True)
    arrs = []
    for d in range(3):
        mf = MultiFab(lev, 1, 0, facedir=d)
        for b, (lo, hi) in enumerate(boxes):
            mf.set_fab(b, tr.box_faces(g, u[d], d, lo, hi))
        arrs.append(mf)
    tp.load(pos, np.zeros_like(pos), np.arange(1000))
    tp.advect(arrs, 0.05)
    xr, vr = tr.advect(g, u, 0.05, pos)
    assert np.array_equal(tp.positions(), xr) and np.array_equal(tp.velocities(), vr)


def test_a_plan_with_holes_needs_its_parent(ctx):
    boxes = halves_x([8, 8, 8], [23, 23, 23])
    geom = Geometry(3, [32, 32, 32], [0.0] * 3, [1.0] * 3, [0, 0, 0])
    lev = Level(ctx, 3, boxes)
    host = types.SimpleNamespace(ctx=ctx, lev=lev, geom=geom, rank=0)
    with pytest.raises(capi.QkError, match="do not tile the domain"):  # the single-level plan keeps refusing
        TracerParticles(host)
    tp = TracerParticles(host, refined=True)
    arrs = [MultiFab(lev, 1, 0, facedir=d, fill=0.0) for d in range(3)]
    pos = np.full((4, 3), 0.5)
    tp.load(pos, np.zeros_like(pos), np.arange(4))
    with pytest.raises(capi.QkError, match="no parent link"):
        tp.advect(arrs, 0.1)
    assert np.array_equal(tp.positions(), pos)
    # a parent of the wrong size is refused when it is linked
    lev0 = Level(ctx, 3, chop_domain([8, 8, 8], [8, 8, 8]))
    p0 = TracerPlan(ctx, lev0, Geometry(3, [8, 8, 8], [0.0] * 3, [1.0] * 3, [0, 0, 0]))
    with pytest.raises(capi.QkError, match="coarsened by 2"):
        tp.plan.set_parent(CUR, p0, [MultiFab(lev0, 1, 0, facedir=d, fill=0.0) for d in range(3)])


# ---------------------------------------------------------------------- qk_tracer_Where
WHERE_BOXES = [L0_3D, halves_x([8, 8, 8], [23, 23, 23]) + [cube([0, 0, 24], [7, 7, 31])], [cube([24, 24, 24], [39, 39, 39]), cube([0, 0, 56], [7, 7, 63])]]


@functools.lru_cache(maxsize=None)
def where_inputs():
    rng = np.random.default_rng(33)
    g0 = tr.TracerGeom(3, [16, 16, 16], [-0.3, 0.1, 0.25], [0.9, 1.3, 1.45], [1, 0, 1])
    geoms = [ta.level_geom(g0, m) for m in range(3)]
    lo, hi = np.array(g0.prob_lo), np.array(g0.prob_hi)
    rand = lo + (hi - lo) * rng.uniform(-0.2, 1.2, size=(3000, 3))  # some outside: shifted (x, z) or dropped (y)
    edge = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(1500, 3))
    edges = sorted({0, 64} | {4 * b[0][e] for b in WHERE_BOXES[0] for e in range(3)} | {2 * v for b in WHERE_BOXES[1] for e in range(3) for v in (b[0][e], b[1][e] + 1)}
                   | {v for b in WHERE_BOXES[2] for e in range(3) for v in (b[0][e], b[1][e] + 1)})  # box and domain edges in level-2 cells
    for m, p in enumerate(edge):  # one to three coordinates exactly on an edge, or one ulp to either side
        for e in rng.choice(3, size=rng.integers(1, 4), replace=False):
            xb = lo[e] + edges[rng.integers(0, len(edges))] * geoms[2].dx[e]
            p[e] = (xb, np.nextafter(xb, np.inf), np.nextafter(xb, -np.inf))[m % 3]
    pos = np.ascontiguousarray(np.concatenate([rand, edge]))
    level = rng.integers(0, 3, size=pos.shape[0]).astype(np.int32)
    return g0, geoms, pos, level


@pytest.mark.parametrize("ngrow", [0, 1, 2])
@pytest.mark.parametrize("lev_min", [0, 1])
def test_where_matches_restatement(ctx, lev_min, ngrow):
    g0, geoms, pos, level = where_inputs()
    pr, new_r, keep_r = ta.where(geoms, WHERE_BOXES, lev_min, ngrow, pos, level)
    assert 0 < keep_r.sum() < len(keep_r) and all((new_r == m).any() for m in range(3))
    stays = keep_r & (new_r == level)
    finest = ta.where(geoms, WHERE_BOXES, lev_min, 0, pos, level)[1]
    if ngrow > 0:
        assert (stays & (finest != level)).any(), "the grown boxes keep particles that ngrow = 0 would move"
    plans = []
    for m in range(3):
        G = Geometry(3, list(geoms[m].n_cell), list(g0.prob_lo), list(g0.prob_hi), list(g0.periodic))
        lev = Level(ctx, 3, WHERE_BOXES[m])
        plans.append(TracerPlan(ctx, lev, G, refined=m > 0))
    dpos = [torch.from_numpy(np.ascontiguousarray(pos[:, d])).to(ctx.device) for d in range(3)]
    new, keep = where(ctx, plans, lev_min, ngrow, dpos, torch.from_numpy(level).to(ctx.device))
    assert np.array_equal(keep.cpu().numpy(), keep_r)
    assert np.array_equal(new.cpu().numpy(), new_r), np.argwhere(new.cpu().numpy() != new_r)[:10].tolist()
    pg = torch.stack(dpos, dim=1).cpu().numpy()
    assert np.array_equal(pg[keep_r], pr[keep_r])
