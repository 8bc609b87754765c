"""CPU test of the host-side plan behind qk_hydro_stage_args::ghost_from_source (qk_ghost_source_plan / qk_ghost_source_lookup, no GPU): on the
geometries tests/test_ghost_from_source_gpu.py runs, the map of every cell a fused stage can read outside a box — the four ghost layers, edges and
corners included — names the cell and the sign the ghost fill copies from.

Two fills are asked.  tests/ghost_reference.py (the fill written from its definition, cell by cell) on all four geometries; oracle/boundary.hpp
through an oracle simulation wherever the oracle's problems can build the geometry — its Sedov problem reflects at every wall that is not periodic,
so the fully periodic lattice, the single periodic box and the lattice that reflects in x are compared with it as well, and the octant with
extrapolating high faces with the definition alone.  Valid cells carry ghost_reference.encode(): the value names the source cell and component,
its sign the flip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import ghost_reference as ref  # noqa: E402

NG = ref.NGHOST
NC = 6


def lattice(nb, blen):
    """boxes of a regular lattice, in an order that is NOT lexicographic (the plan must not depend on it)"""
    boxes = [([i * blen[0], j * blen[1], k * blen[2]], [(i + 1) * blen[0] - 1, (j + 1) * blen[1] - 1, (k + 1) * blen[2] - 1])
             for k in range(nb[2]) for j in range(nb[1]) for i in range(nb[0])]
    return boxes[1::2] + boxes[0::2]


def hydro_bcs(lo_type, hi_type):
    """per component (lo[3], hi[3]); 'reflect': the normal momentum odd, everything else even"""
    def one(kind, n, d):
        if kind == "reflect":
            return ref.REFLECT_ODD if n == 1 + d else ref.REFLECT_EVEN
        return {"extrap": ref.FOEXTRAP, "periodic": ref.INT_DIR}[kind]
    return [([one(lo_type[d], n, d) for d in range(3)], [one(hi_type[d], n, d) for d in range(3)]) for n in range(NC)]


# id, boxes per dimension, box shape, rule beyond the low faces, beyond the high faces
GEOMETRIES = [
    ("octant-2x2x2", (2, 2, 2), (64, 16, 16), ("reflect",) * 3, ("extrap",) * 3),
    ("periodic-2x2x2", (2, 2, 2), (64, 16, 16), ("periodic",) * 3, ("periodic",) * 3),
    ("periodic-one-box", (1, 1, 1), (64, 16, 16), ("periodic",) * 3, ("periodic",) * 3),
    ("reflect-x-2x1x1", (2, 1, 1), (128, 8, 8), ("reflect", "periodic", "periodic"), ("reflect", "periodic", "periodic")),
]


def make_plan(nb, blen, lo_t, hi_t, boxes=None):
    from quokka_amd import capi
    from quokka_amd.multifab import Level, PlanningContext
    ctx = PlanningContext()
    n_cell = [nb[d] * blen[d] for d in range(3)]
    periodic = [int(lo_t[d] == "periodic") for d in range(3)]
    boxes = lattice(nb, blen) if boxes is None else boxes
    lev = Level(ctx, 3, boxes)
    geom = capi.Geometry(capi.Box((C.c_int * 3)(0, 0, 0), (C.c_int * 3)(*[n - 1 for n in n_cell])), (C.c_int * 3)(*periodic), 3)
    bcs = hydro_bcs(lo_t, hi_t)
    arr = (capi.BCRec * NC)(*[capi.BCRec((C.c_int * 3)(*lo), (C.c_int * 3)(*hi)) for lo, hi in bcs])
    q = C.c_int(-1)
    ctx.check(ctx.L.qk_ghost_source_plan(lev.h, C.byref(geom), NG, NC, arr, len(boxes), C.byref(q)), "qk_ghost_source_plan")
    return ctx, lev, boxes, ref.geom(3, n_cell, periodic), bcs, q.value


def mapped_fab(ctx, lev, boxes, g, b):
    """the grown fab of box b as the map says it: every cell outside the box takes sign * encode(source cell), asked cell by cell"""
    L = ctx.L
    box = boxes[b]
    fab = ref.new_fab(box, g, NG, NC)
    o = ref.origin_of(box, g, NG)
    nz, ny, nx = fab.shape[1:]
    sb, si, fl = C.c_int(), (C.c_int * 3)(), (C.c_int * 3)()
    for kk in range(nz):
        for jj in range(ny):
            inner = NG <= kk < nz - NG and NG <= jj < ny - NG
            for ii in (list(range(NG)) + list(range(nx - NG, nx)) if inner else range(nx)):
                idx = (C.c_int * 3)(o[0] + ii, o[1] + jj, o[2] + kk)
                ctx.check(L.qk_ghost_source_lookup(lev.h, b, idx, C.byref(sb), si, fl), "qk_ghost_source_lookup")
                lo, hi = boxes[sb.value]
                assert all(lo[d] <= si[d] <= hi[d] for d in range(3)), "the source is not a valid cell of the box the map names"
                for n in range(NC):
                    sign = -1.0 if (1 <= n <= 3 and fl[n - 1]) else 1.0
                    fab[n, kk, jj, ii] = sign * ref.encode(si[0], si[1], si[2], n, g.n_cell)
    return fab


@pytest.mark.parametrize("cid,nb,blen,lo_t,hi_t", GEOMETRIES, ids=[c[0] for c in GEOMETRIES])
def test_source_map_names_the_cells_the_fill_copies_from(cid, nb, blen, lo_t, hi_t):
    ctx, lev, boxes, g, bcs, q = make_plan(nb, blen, lo_t, hi_t)
    assert q == 1, "the geometry was expected to qualify"
    want = [ref.new_fab(b, g, NG, NC) for b in boxes]
    ref.fill_boundary(boxes, want, g, NG)
    for box, fab in zip(boxes, want):
        ref.fill_physical(fab, ref.origin_of(box, g, NG), g, bcs)
    for b in range(len(boxes)):
        assert not np.isnan(want[b]).any(), "the fill leaves a ghost cell unset: nothing to compare the map with"
        got = mapped_fab(ctx, lev, boxes, g, b)
        assert np.array_equal(got, want[b]), f"box {b}: {int((got != want[b]).sum())} values differ"


@pytest.mark.parametrize("cid,nb,blen,lo_t,hi_t", [c for c in GEOMETRIES if "extrap" not in c[4]], ids=[c[0] for c in GEOMETRIES if "extrap" not in c[4]])
def test_source_map_against_the_fill_of_the_oracle(oracle, cid, nb, blen, lo_t, hi_t):
    """oracle/boundary.hpp through the oracle's Sedov simulation (reflecting walls wherever the domain is not periodic)"""
    from oracle.pyoracle import SEDOV
    ctx, lev, boxes, g, bcs, q = make_plan(nb, blen, lo_t, hi_t)
    assert q == 1
    so = oracle.sim(SEDOV, 3, g.n_cell, [0.0] * 3, [1.0] * 3, g.periodic, max_grid_size=list(blen))
    assert so.nboxes == len(boxes) and so.ncomp == NC and so.nghost == NG
    mine = {tuple(lo): b for b, (lo, hi) in enumerate(boxes)}
    for ob in range(so.nboxes):
        lo, hi = so.box(ob)
        so.set_state(ref.new_fab((lo, hi), g, NG, NC, ghosts=-7.0), ob)
    so.fill_ghosts()
    for ob in range(so.nboxes):
        lo, hi = so.box(ob)
        b = mine[tuple(lo)]
        assert boxes[b][1] == list(hi)
        got = mapped_fab(ctx, lev, boxes, g, b)
        assert np.array_equal(got, so.state(ob)), f"box {b}: {int((got != so.state(ob)).sum())} values differ"


def test_levels_that_do_not_qualify_are_refused():
    per, refl, ext = ("periodic",) * 3, ("reflect",) * 3, ("extrap",) * 3
    # two boxes of different sizes
    assert make_plan((1, 1, 1), (192, 16, 16), refl, ext, boxes=[([0, 0, 0], [127, 15, 15]), ([128, 0, 0], [191, 15, 15])])[5] == 0
    # boxes that are not whole waves wide, boxes shorter than the ghost width
    assert make_plan((2, 2, 2), (32, 16, 16), refl, ext)[5] == 0
    assert make_plan((1, 2, 2), (64, 2, 16), per, per)[5] == 0
    # a lattice that does not cover the domain
    assert make_plan((2, 1, 1), (64, 16, 16), per, per, boxes=[([0, 0, 0], [63, 15, 15])])[5] == 0
    # a face that is neither periodic, reflecting nor extrapolating (an interior type on a wall that is not periodic)
    from quokka_amd import capi
    from quokka_amd.multifab import Level, PlanningContext
    ctx = PlanningContext()
    lev = Level(ctx, 3, [([0, 0, 0], [63, 15, 15])])
    geom = capi.Geometry(capi.Box((C.c_int * 3)(0, 0, 0), (C.c_int * 3)(63, 15, 15)), (C.c_int * 3)(0, 0, 0), 3)
    for bad in (ref.EXT_DIR, ref.INT_DIR):
        bcs = hydro_bcs(refl, refl)
        bcs[0][1][2] = bad
        arr = (capi.BCRec * NC)(*[capi.BCRec((C.c_int * 3)(*lo), (C.c_int * 3)(*hi)) for lo, hi in bcs])
        q = C.c_int(-1)
        ctx.check(ctx.L.qk_ghost_source_plan(lev.h, C.byref(geom), NG, NC, arr, 1, C.byref(q)), "qk_ghost_source_plan")
        assert q.value == 0
    # ... and a parity other than the normal momentum's: the energy odd at the x walls
    bcs = hydro_bcs(refl, refl)
    bcs[4][0][0] = ref.REFLECT_ODD
    arr = (capi.BCRec * NC)(*[capi.BCRec((C.c_int * 3)(*lo), (C.c_int * 3)(*hi)) for lo, hi in bcs])
    q = C.c_int(-1)
    ctx.check(ctx.L.qk_ghost_source_plan(lev.h, C.byref(geom), NG, NC, arr, 1, C.byref(q)), "qk_ghost_source_plan")
    assert q.value == 0
    # the single box with proper reflecting walls does qualify
    assert make_plan((1, 1, 1), (64, 16, 16), refl, refl)[5] == 1
