"""CPU proof of tests/ghost_reference.py and of the plans the ghost-motion kernels execute: the items of GhostExchange.items() and
ParallelCopy.items() from a PlanningContext are replayed with numpy (as test_multirank_gloo.py does) on every geometry
test_ghost_motion_gpu.py runs, with one rank and with two ranks in one process, and must reproduce the brute-force reference cell for cell —
ghost cells nobody fills included (NaN stays NaN).  All comparisons are equalities of whole fabs."""
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


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def lib_geom(g):
    from quokka_amd.simulation import Geometry
    return Geometry(g.ndim, list(g.n_cell), [0.0] * 3, [1.0] * 3, list(g.periodic))


def region(fab, begin, lo, hi, shift=(0, 0, 0)):
    """numpy view of fab[(ncomp), z, y, x] over the index region [lo, hi] shifted by -shift"""
    sl = [slice(None)]
    for d in (2, 1, 0):
        a = lo[d] - shift[d] - begin[d]
        assert a >= 0, "a plan item reaches outside its fab"
        sl.append(slice(a, hi[d] - shift[d] - begin[d] + 1))
    v = fab[tuple(sl)]
    assert v.shape[1:] == tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0)), "a plan item reaches outside its fab"
    return v


class Ranks:
    """the ghost plans of all ranks of one level in one process (PlanningContext: host logic only)"""

    def __init__(self, g, boxes, owner, ncomp, nghost=NG):
        from quokka_amd.multifab import Level, PlanningContext
        from quokka_amd.simulation import GhostExchange
        self.g, self.boxes, self.owner, self.ng = g, boxes, owner, nghost
        self.ctx = PlanningContext()
        self.nranks = max(owner) + 1
        self.mine = [[b for b, o in enumerate(owner) if o == r] for r in range(self.nranks)]
        self.levels = [Level(self.ctx, g.ndim, [boxes[b] for b in m]) for m in self.mine]
        bcs = ref.BCS_A * ncomp
        self.ex = [GhostExchange(lev, lib_geom(g), ncomp, nghost, boxes, owner, r, bcs[:ncomp]) for r, lev in enumerate(self.levels)]
        self.begins = [ref.origin_of(b, g, nghost) for b in boxes]

    def fill(self, fabs):
        """FillBoundary: pack -> wire -> same-rank copies -> unpack, numpy moving the plan's items"""
        wire = {}
        for r, ex in enumerate(self.ex):
            for k, peer, sbuf, rbuf in ex.peers:
                buf = np.full(sbuf.numel(), np.nan)
                for db, sb, lo, hi, sh, off in ex.items(1, k):
                    v = region(fabs[self.mine[r][sb]], self.begins[self.mine[r][sb]], lo, hi, sh)
                    buf[off:off + v.size] = v.reshape(-1)
                wire[(r, peer)] = buf
        for r, ex in enumerate(self.ex):
            for db, sb, lo, hi, sh, off in ex.items(0):
                gd, gs = self.mine[r][db], self.mine[r][sb]
                region(fabs[gd], self.begins[gd], lo, hi)[...] = region(fabs[gs], self.begins[gs], lo, hi, sh)
        for r, ex in enumerate(self.ex):
            for k, peer, sbuf, rbuf in ex.peers:
                buf = wire[(peer, r)]
                assert buf.size == rbuf.numel()
                for db, sb, lo, hi, sh, off in ex.items(2, k):
                    gd = self.mine[r][db]
                    v = region(fabs[gd], self.begins[gd], lo, hi)
                    v[...] = buf[off:off + v.size].reshape(v.shape)

    def sum(self, fabs):
        """SumBoundary: the receive strips travel back and are added to the valid cells they mirror"""
        wire = {}
        for r, ex in enumerate(self.ex):
            for k, peer, sbuf, rbuf in ex.peers:
                buf = np.full(rbuf.numel(), np.nan)
                for db, sb, lo, hi, sh, off in ex.items(2, k):
                    gd = self.mine[r][db]
                    v = region(fabs[gd], self.begins[gd], lo, hi)
                    buf[off:off + v.size] = v.reshape(-1)
                wire[(r, peer)] = buf
        for r, ex in enumerate(self.ex):
            for db, sb, lo, hi, sh, off in ex.items(0):
                gd, gs = self.mine[r][db], self.mine[r][sb]
                region(fabs[gs], self.begins[gs], lo, hi, sh)[...] += region(fabs[gd], self.begins[gd], lo, hi)
        for r, ex in enumerate(self.ex):
            for k, peer, sbuf, rbuf in ex.peers:
                buf = wire[(peer, r)]
                assert buf.size == sbuf.numel()
                for db, sb, lo, hi, sh, off in ex.items(1, k):
                    gs = self.mine[r][sb]
                    v = region(fabs[gs], self.begins[gs], lo, hi, sh)
                    v[...] += buf[off:off + v.size].reshape(v.shape)


CASES = ref.fill_cases()


def with_ranks(cases):
    out = []
    for cid, g, boxes, owner in cases:
        out.append(pytest.param(g, boxes, [0] * len(boxes), id=cid + "-1rank"))
        if max(owner) > 0:
            out.append(pytest.param(g, boxes, owner, id=cid + "-2ranks"))
    return out


@pytest.mark.parametrize("g,boxes,owner", with_ranks(CASES))
def test_fill_boundary_plan_matches_definition(g, boxes, owner):
    nc = 3
    fabs = [ref.new_fab(b, g, NG, nc) for b in boxes]
    want = [f.copy() for f in fabs]
    ref.fill_boundary(boxes, want, g, NG)
    Ranks(g, boxes, owner, nc).fill(fabs)
    for b in range(len(boxes)):
        assert same(fabs[b], want[b]), f"box {b}: {int((~np.isclose(fabs[b], want[b], equal_nan=True)).sum())} cells differ"


@pytest.mark.parametrize("g,boxes,owner", with_ranks(CASES))
def test_sum_boundary_plan_matches_definition(g, boxes, owner):
    nc = 2
    fabs = [ref.filled_fab(b, g, NG, nc, tag=t) for t, b in enumerate(boxes)]
    want = [f.copy() for f in fabs]
    ref.sum_boundary(boxes, want, g, NG)
    Ranks(g, boxes, owner, nc).sum(fabs)
    for b in range(len(boxes)):
        assert same(fabs[b], want[b]), f"box {b} differs"


@pytest.mark.parametrize("g,boxes,owner", with_ranks(CASES))
def test_physical_boundary_slabs_cover_exactly_the_cells_beyond_the_walls(g, boxes, owner):
    """k_physbc runs over the items of kind 3: together they must be the cells of the grown boxes beyond a non-periodic face, no others"""
    R = Ranks(g, boxes, owner, 3)
    for r, ex in enumerate(R.ex):
        hit = [np.zeros(ref.shape_of(boxes[b], g, NG), dtype=bool) for b in R.mine[r]]
        for db, sb, lo, hi, sh, off in ex.items(3):
            region(hit[db][None], R.begins[R.mine[r][db]], lo, hi)[...] = True
        for n, b in enumerate(R.mine[r]):
            i, j, k = ref.axes_of(boxes[b], g, NG)
            out = np.zeros_like(hit[n])
            for d, x in ((0, i[None, None, :]), (1, j[None, :, None]), (2, k[:, None, None])):
                if d < g.ndim and not g.periodic[d]:
                    out |= (x < 0) | (x > g.n_cell[d] - 1)
            assert np.array_equal(hit[n], out)


def test_many_boxes_plan_matches_definition():
    """2548 boxes of 4^3: 66 248 same-rank items (the GPU test launches them in chunks)"""
    cid, g, boxes, _ = ref.many_boxes_case()
    fabs = [ref.new_fab(b, g, NG, 1) for b in boxes]
    want = [f.copy() for f in fabs]
    ref.fill_boundary(boxes, want, g, NG)
    R = Ranks(g, boxes, [0] * len(boxes), 1)
    assert len(R.ex[0].items(0)) == 2548 * 26 == 66248
    R.fill(fabs)
    assert all(same(a, b) for a, b in zip(fabs, want))
    assert not any(np.isnan(a).any() for a in fabs)


# ------------------------------------------------------------------------------------------------ the sweep against a one-shot composition
def oneshot_physbc(fab, origin, g, bcs):
    """per cell beyond a wall: every direction's source index and sign composed at once (the algorithm of the kernel, restated independently of
    it), reading the array as it was before the call"""
    before = fab.copy()
    nc, nz, ny, nx = fab.shape
    for n in range(nc):
        lo_t, hi_t = bcs[n]
        for kk in range(nz):
            for jj in range(ny):
                for ii in range(nx):
                    idx = [origin[0] + ii, origin[1] + jj, origin[2] + kk]
                    src, sign, any_ = list(idx), 1.0, False
                    for d in range(g.ndim):
                        if g.periodic[d]:
                            continue
                        hi_edge = g.n_cell[d] - 1
                        if idx[d] < 0:
                            t, edge, mirror = lo_t[d], 0, -idx[d] - 1
                        elif idx[d] > hi_edge:
                            t, edge, mirror = hi_t[d], hi_edge, 2 * hi_edge - idx[d] + 1
                        else:
                            continue
                        if t == ref.FOEXTRAP:
                            src[d], any_ = edge, True
                        elif t in (ref.REFLECT_EVEN, ref.REFLECT_ODD):
                            src[d], any_ = mirror, True
                            sign *= -1.0 if t == ref.REFLECT_ODD else 1.0
                    if any_:
                        fab[n, kk, jj, ii] = sign * before[n, src[2] - origin[2], src[1] - origin[1], src[0] - origin[0]]


@pytest.mark.parametrize("cid,g,boxes,owner", [c for c in ref.ragged_cases() if c[0] in ("ragged3d-p000", "ragged3d-p010", "ragged2d-p00", "ragged1d-p0")]
                         + [ref.partial_case()], ids=lambda v: v if isinstance(v, str) else "")
def test_sweep_equals_one_shot_composition(cid, g, boxes, owner):
    fabs = [ref.new_fab(b, g, NG, 3) for b in boxes]
    ref.fill_boundary(boxes, fabs, g, NG)
    for bcs in (ref.BCS_A, ref.BCS_B):
        for box, fab in zip(boxes, fabs):
            a, b = fab.copy(), fab.copy()
            ref.fill_physical(a, ref.origin_of(box, g, NG), g, bcs)
            oneshot_physbc(b, ref.origin_of(box, g, NG), g, bcs)
            assert same(a, b)
            assert not same(a, fab), "the case has no wall"


def test_thin_wall_direction_types_are_order_independent():
    """the boundary types of the 124 x 124 x 2 GPU case on a small box of the same thickness: no cell read is a cell written"""
    g, box = ref.geom(3, [12, 10, 2], [0, 0, 0]), ([0, 0, 0], [11, 9, 1])
    fab = ref.new_fab(box, g, NG, 2)
    a, b = fab.copy(), fab.copy()
    ref.fill_physical(a, ref.origin_of(box, g, NG), g, ref.BCS_THIN_Z)
    oneshot_physbc(b, ref.origin_of(box, g, NG), g, ref.BCS_THIN_Z)
    assert same(a, b) and not same(a, fab)
    c, d = fab.copy(), fab.copy()
    ref.fill_physical(c, ref.origin_of(box, g, NG), g, ref.BCS_A[1:])
    oneshot_physbc(d, ref.origin_of(box, g, NG), g, ref.BCS_A[1:])
    assert not same(c, d), "reflections across a 2-cell direction were expected to depend on the order"


def test_component_range_of_the_reference():
    cid, g, boxes, owner = ref.ragged_cases()[0]
    fab = ref.new_fab(boxes[0], g, NG, 3)
    full = fab.copy()
    ref.fill_physical(full, ref.origin_of(boxes[0], g, NG), g, ref.BCS_A)
    part = fab.copy()
    ref.fill_physical(part, ref.origin_of(boxes[0], g, NG), g, ref.BCS_A, scomp=1, ncomp=1)
    assert same(part[1], full[1]) and same(part[0], fab[0]) and same(part[2], fab[2])


def hydro_bcs(nc):
    """reflecting walls of a hydro state: the momentum normal to a wall is odd"""
    return [([ref.REFLECT_ODD if n == 1 + d else ref.REFLECT_EVEN for d in range(3)],) * 2 for n in range(nc)]


def test_dirichlet_faces_by_hand():
    """constants on x-lo and y-hi: x faces first, a disabled face falls through to the BCRec; the interior / kinetic / Marshak terms against
    hand-written arithmetic at single cells"""
    g = ref.geom(3, [12, 10, 8], [0, 0, 0])
    box = ([0, 0, 0], [11, 9, 7])
    o = ref.origin_of(box, g, NG)
    nc = 6
    fab = ref.new_fab(box, g, NG, nc)

    def at(a, n, i, j, k):
        return a[n, k - o[2], j - o[1], i - o[0]]

    xlo, yhi = [10 + n for n in range(nc)], [20 + n for n in range(nc)]
    a = fab.copy()
    ref.fill_physical(a, o, g, hydro_bcs(nc), {(0, 0): xlo, (1, 1): yhi})
    for n in range(nc):
        assert at(a, n, -2, 3, 3) == xlo[n] and at(a, n, 5, 11, 3) == yhi[n]
        assert at(a, n, -1, 12, -3) == xlo[n]  # x first, also beyond the (reflecting) z-lo face
        assert at(a, n, 13, 10, 2) == yhi[n]  # beyond x-hi (disabled) and y-hi
        s = -1.0 if n in (1, 2) else 1.0  # beyond x-hi and y-lo, both reflecting: mirrored twice
        assert at(a, n, 12, -1, 2) == s * at(fab, n, 11, 0, 2)
    gp = ref.geom(3, [12, 10, 8], [0, 1, 1])
    vals = [2.0, 3.0, 5.0, 7.0, 11.0, 13.0]
    b = ref.new_fab(box, gp, NG, nc)
    ref.fill_boundary([box], [b], gp, NG)
    b0 = b.copy()
    ref.fill_physical(b, o, gp, hydro_bcs(nc), {(0, 1): {"values": vals, "interior": [1], "kinetic_from_interior": True},
                                               (0, 0): {"values": vals, "marshak": (2, 3, 4.0)}})
    m = at(b0, 1, 11, -2, 9)  # the first cell inside x-hi, transverse indices in the periodic ghost region
    assert at(b, 1, 14, -2, 9) == m and at(b, 4, 14, -2, 9) == 13.0 + 0.5 * m * m / 2.0 and at(b, 0, 14, -2, 9) == 2.0
    E0, F0 = at(b0, 2, 0, 4, 4), at(b0, 3, 0, 4, 4)
    assert at(b, 3, -3, 4, 4) == 0.5 * 4.0 * 5.0 - 0.5 * (4.0 * E0 + 2.0 * F0) and at(b, 2, -3, 4, 4) == 5.0


# ------------------------------------------------------------------------------------------------ ParallelCopy / ParallelAdd
class PcRanks:
    def __init__(self, g, src_boxes, src_owner, dst_boxes, dst_owner, ncomp, **kw):
        from quokka_amd.amr import ParallelCopy
        from quokka_amd.multifab import PlanningContext
        self.ctx = PlanningContext()
        self.nranks = max(max(src_owner), max(dst_owner)) + 1
        self.smine = [[b for b, o in enumerate(src_owner) if o == r] for r in range(self.nranks)]
        self.dmine = [[b for b, o in enumerate(dst_owner) if o == r] for r in range(self.nranks)]
        self.plans = [ParallelCopy(self.ctx, lib_geom(g), src_boxes, src_owner, dst_boxes, dst_owner, ncomp, r, **kw) for r in range(self.nranks)]

    def run(self, src, sbeg, dst, dbeg, scomp_src, scomp_dst, ncomp, add):
        cs, cd = slice(scomp_src, scomp_src + ncomp), slice(scomp_dst, scomp_dst + ncomp)
        wire = {}
        for r, plan in enumerate(self.plans):
            for k, peer, sbuf, rbuf in plan.peers:
                buf = np.full(sbuf.numel(), np.nan)
                for db, sb, lo, hi, sh, off in plan.items(1, k):
                    gs = self.smine[r][sb]
                    v = region(src[gs][cs], sbeg[gs], lo, hi, sh)
                    buf[off:off + v.size] = v.reshape(-1)
                wire[(r, peer)] = buf

        def put(out, v):
            out[...] = out + v if add else v

        for r, plan in enumerate(self.plans):
            for db, sb, lo, hi, sh, off in plan.items(0):
                gd, gs = self.dmine[r][db], self.smine[r][sb]
                put(region(dst[gd][cd], dbeg[gd], lo, hi), region(src[gs][cs], sbeg[gs], lo, hi, sh))
        for r, plan in enumerate(self.plans):
            for k, peer, sbuf, rbuf in plan.peers:
                kk = [q for q, pr, _, _ in self.plans[peer].peers if pr == r]
                assert len(kk) == 1
                buf = wire[(peer, r)]
                assert buf.size == rbuf.numel()
                for db, sb, lo, hi, sh, off in plan.items(2, k):
                    gd = self.dmine[r][db]
                    out = region(dst[gd][cd], dbeg[gd], lo, hi)
                    put(out, buf[off:off + out.size].reshape(out.shape))


def pc_owners(two_ranks):
    if two_ranks:
        return ref.PC_TILING_OWNER, ref.PC_ODD_OWNER
    return [0] * len(ref.PC_TILING), [0] * len(ref.PC_ODD)


@pytest.mark.parametrize("two_ranks", [False, True], ids=["1rank", "2ranks"])
def test_parallel_copy_plan_matches_definition(two_ranks):
    """tiling (4 components) -> odd boxes grown by 3 (5 components): components 1-2 land in components 2-3"""
    g, town, oown = ref.PC_GEOM, *pc_owners(two_ranks)
    src = [ref.new_fab(b, g, 0, 4) for b in ref.PC_TILING]
    dst = [np.full((5,) + ref.shape_of(b, g, 3), np.nan) for b in ref.PC_ODD]
    want = [d.copy() for d in dst]
    ref.parallel_copy(ref.PC_TILING, src, ref.PC_ODD, want, g, dst_nghost=3, scomp_src=1, scomp_dst=2, ncomp=2)
    PcRanks(g, ref.PC_TILING, town, ref.PC_ODD, oown, 2, dst_nghost=3).run(
        src, [ref.origin_of(b, g, 0) for b in ref.PC_TILING], dst, [ref.origin_of(b, g, 3) for b in ref.PC_ODD], 1, 2, 2, False)
    for a, b in zip(dst, want):
        assert same(a, b)
        assert np.isnan(a[[0, 1, 4]]).all() and not np.isnan(a[2]).all()
    assert np.isnan(dst[0][2]).any(), "no destination cell beyond the y wall"


@pytest.mark.parametrize("holes", [None, ref.PC_HOLES], ids=["", "holes"])
@pytest.mark.parametrize("two_ranks", [False, True], ids=["1rank", "2ranks"])
def test_parallel_add_plan_matches_definition(two_ranks, holes):
    """the one-cell rings of the odd boxes (4 components) added to the tiling (5 components)"""
    g, town, oown = ref.PC_GEOM, *pc_owners(two_ranks)
    src = [ref.filled_fab(b, g, 1, 4, tag=t) for t, b in enumerate(ref.PC_ODD)]
    for b, f in zip(ref.PC_ODD, src):
        f[ref.valid_slices(b, g, 1)] = 1.0e300  # valid cells of a ring-only source never travel
    dst = [ref.new_fab(b, g, 0, 5) for b in ref.PC_TILING]
    want = [d.copy() for d in dst]
    ref.parallel_copy(ref.PC_ODD, src, ref.PC_TILING, want, g, src_nghost=1, src_ring_only=True, holes=holes, scomp_src=1, scomp_dst=2, ncomp=2, add=True)
    PcRanks(g, ref.PC_ODD, oown, ref.PC_TILING, town, 2, src_nghost=1, src_ring_only=True, dst_holes=holes).run(
        src, [ref.origin_of(b, g, 1) for b in ref.PC_ODD], dst, [ref.origin_of(b, g, 0) for b in ref.PC_TILING], 1, 2, 2, True)
    for a, b, box in zip(dst, want, ref.PC_TILING):
        assert same(a, b)
        assert same(a[[0, 1, 4]], ref.new_fab(box, g, 0, 5)[[0, 1, 4]])
    assert max(float(np.abs(b).max()) for b in want) < 1.0e299


def test_two_rings_land_on_one_cell():
    """the case is only a test of the add groups if some cell of the tiling receives from two rings"""
    g = ref.PC_GEOM
    ones = [np.ones((1,) + ref.shape_of(b, g, 1)) for b in ref.PC_ODD]
    dst = [np.zeros((1,) + ref.shape_of(b, g, 0)) for b in ref.PC_TILING]
    ref.parallel_copy(ref.PC_ODD, ones, ref.PC_TILING, dst, g, src_nghost=1, src_ring_only=True, ncomp=1, add=True)
    assert max(d.max() for d in dst) >= 2.0
    assert sum(d.sum() for d in dst) == sum(np.prod(ref.shape_of(b, g, 1)) - np.prod(ref.shape_of(b, g, 0)) for b in ref.PC_ODD)
