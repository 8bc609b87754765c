"""The kernels that move ghost data — k_copy in its six modes and its int instantiation, k_physbc<true/false>, k_pcopy in its three modes
with and without ADD, k_copy_box — against the brute-force reference of tests/ghost_reference.py, cell by cell, through Level, MultiFab,
GhostExchange, ParallelCopy and capi.  Every comparison is np.array_equal(..., equal_nan=True) on whole fabs, ghost cells included: the data
are small integers (ghost_reference.encode), cells nobody may write start as NaN.  There is no tolerance in this file, only sizes.

Two ranks run in ONE process: two Levels and two plans over one owner list; what a rank packs for a peer is copied into the peer's receive
buffer with torch.Tensor.copy_ (no RCCL, no second process)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import ghost_reference as ref  # noqa: E402
from quokka_amd import capi  # noqa: E402
from quokka_amd.amr import ParallelCopy  # noqa: E402
from quokka_amd.multifab import Level, MultiFab  # noqa: E402
from quokka_amd.simulation import Geometry, GhostExchange  # noqa: E402

pytestmark = pytest.mark.gpu
NG = ref.NGHOST


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def lib_geom(g):
    return Geometry(g.ndim, list(g.n_cell), [0.0] * 3, [1.0] * 3, list(g.periodic))


def _host_views(mf, host):
    out = []
    for off, shp, p in zip(mf.offsets, mf.shapes, mf.pitches):
        it = host.itemsize
        out.append(np.lib.stride_tricks.as_strided(host[off:], shape=shp, strides=(p * shp[2] * shp[1] * it, p * shp[2] * it, p * it, it)))
    return out


def put(mf, fabs):
    """whole storage in one copy; the pad columns of pitched rows hold NaN (-7 in an int MultiFab)"""
    npdt = np.int32 if mf.dtype == torch.int32 else np.float64
    host = np.full(mf.storage.numel(), -7 if npdt == np.int32 else np.nan, dtype=npdt)
    for v, a in zip(_host_views(mf, host), fabs):
        assert v.shape == a.shape
        v[...] = a
    mf.storage.copy_(torch.from_numpy(host))


def get(mf):
    host = mf.storage.cpu().numpy()
    return [v.copy() for v in _host_views(mf, host)]


def vp(t):
    return C.c_void_p(t.data_ptr())


class Ranks:
    """the Levels, ghost plans and MultiFabs of all ranks of one level on one GPU"""

    def __init__(self, ctx, g, boxes, owner, ncomp, bcs=None, dirichlet=None, dtype=torch.float64):
        self.ctx, self.g, self.boxes, self.ncomp = ctx, g, boxes, ncomp
        self.nranks = max(owner) + 1
        self.mine = [[b for b, o in enumerate(owner) if o == r] for r in range(self.nranks)]
        self.levels = [Level(ctx, g.ndim, [boxes[b] for b in m]) for m in self.mine]
        bcs = (ref.BCS_A * ncomp)[:ncomp] if bcs is None else bcs
        self.ex = [GhostExchange(lev, lib_geom(g), ncomp, NG, boxes, owner, r, bcs, dirichlet=dirichlet, dtype=dtype) for r, lev in enumerate(self.levels)]
        self.mf = [MultiFab(lev, ncomp, NG, dtype=dtype) for lev in self.levels]

    def put(self, fabs):
        for r, m in enumerate(self.mine):
            put(self.mf[r], [fabs[b] for b in m])

    def get(self):
        out = [None] * len(self.boxes)
        for r, m in enumerate(self.mine):
            for b, a in zip(m, get(self.mf[r])):
                out[b] = a
        return out

    def _wire(self, src_is_send):
        """the strips every rank packed, moved into its peers' buffers"""
        for r, ex in enumerate(self.ex):
            for k, peer, sbuf, rbuf in ex.peers:
                kk = [q for q, pr, _, _ in self.ex[peer].peers if pr == r]
                assert len(kk) == 1
                _, _, psbuf, prbuf = self.ex[peer].peers[kk[0]]
                if src_is_send:
                    assert prbuf.numel() == sbuf.numel()
                    prbuf.copy_(sbuf)
                else:
                    assert psbuf.numel() == rbuf.numel()
                    psbuf.copy_(rbuf)

    def fill(self, physbc=True):
        """one rank: GhostExchange.fill, the product path; several: pack -> copy_ -> local -> unpack -> physbc through capi"""
        ctx, L, s = self.ctx, self.ctx.L, self.ctx.stream()
        if self.nranks == 1 and self.mf[0].dtype == torch.float64 and physbc:
            self.ex[0].fill(self.mf[0])
            return
        i = "_int" if self.mf[0].dtype == torch.int32 else ""
        for ex, mf in zip(self.ex, self.mf):
            for k, peer, sbuf, rbuf in ex.peers:
                sbuf.fill_(-5)
                ctx.check(getattr(L, "qk_FillBoundary_pack" + i)(ex.h, s, k, mf.ptr, vp(sbuf)), "pack")
        self._wire(True)
        for ex, mf in zip(self.ex, self.mf):
            ctx.check(getattr(L, "qk_FillBoundary_local" + i)(ex.h, s, mf.ptr), "local")
            for k, peer, sbuf, rbuf in ex.peers:
                ctx.check(getattr(L, "qk_FillBoundary_unpack" + i)(ex.h, s, k, mf.ptr, vp(rbuf)), "unpack")
            if physbc and not i:
                ctx.check(L.qk_FillPhysicalBoundary(ex.h, s, mf.ptr, ex.bcs, ex.dirichlet), "physbc")

    def sum(self):
        ctx, L, s = self.ctx, self.ctx.L, self.ctx.stream()
        if self.nranks == 1:
            self.ex[0].sum_boundary(self.mf[0])
            return
        for ex, mf in zip(self.ex, self.mf):
            for k, peer, sbuf, rbuf in ex.peers:
                ctx.check(L.qk_SumBoundary_pack(ex.h, s, k, mf.ptr, vp(rbuf)), "sum pack")
        self._wire(False)
        for ex, mf in zip(self.ex, self.mf):
            ctx.check(L.qk_SumBoundary_local(ex.h, s, mf.ptr), "sum local")
            for k, peer, sbuf, rbuf in ex.peers:
                ctx.check(L.qk_SumBoundary_unpack(ex.h, s, k, mf.ptr, vp(sbuf)), "sum unpack")


def reference_fill(g, boxes, fabs, bcs, dirichlet=None, physbc=True):
    want = [f.copy() for f in fabs]
    ref.fill_boundary(boxes, want, g, NG)
    if physbc:
        for box, w in zip(boxes, want):
            ref.fill_physical(w, ref.origin_of(box, g, NG), g, bcs, dirichlet)
    return want


def assert_fabs(got, want):
    for b, (a, w) in enumerate(zip(got, want)):
        assert a.shape == w.shape
        assert same(a, w), f"box {b}: {int((~((a == w) | (np.isnan(a) & np.isnan(w)))).sum())} of {a.size} values differ"


def with_ranks(cases):
    out = []
    for cid, g, boxes, owner in cases:
        out.append(pytest.param(g, boxes, [0] * len(boxes), id=cid + "-1rank"))
        if max(owner) > 0:
            out.append(pytest.param(g, boxes, owner, id=cid + "-2ranks"))
    return out


# ------------------------------------------------------------------------------------------------ ghost fill + physical boundaries
@pytest.mark.parametrize("g,boxes,owner", with_ranks(ref.fill_cases()))
def test_fill_and_physical_boundaries(ctx, g, boxes, owner):
    """ragged layouts in 1, 2 and 3 dimensions with every combination of periodic flags and mixed boundary types, one box as wide as and
    narrower than the ghost width, a partially covered domain, a narrow periodic direction shared by two ranks"""
    R = Ranks(ctx, g, boxes, owner, 3)
    fabs = [ref.new_fab(b, g, NG, 3) for b in boxes]
    R.put(fabs)
    R.fill()
    assert_fabs(R.get(), reference_fill(g, boxes, fabs, ref.BCS_A))


@pytest.mark.parametrize("g,boxes,owner", with_ranks(ref.fill_cases()))
def test_fill_int(ctx, g, boxes, owner):
    """the int instantiation of the copy kernel (local, pack, unpack) on an int32 MultiFab; -1 marks a cell nobody wrote"""
    R = Ranks(ctx, g, boxes, owner, 2, dtype=torch.int32)
    fabs = [ref.new_fab(b, g, NG, 2, dtype=np.int32, ghosts=-1) for b in boxes]
    R.put(fabs)
    R.fill()
    got = R.get()
    assert got[0].dtype == np.int32
    assert_fabs(got, reference_fill(g, boxes, fabs, None, physbc=False))


def ragged(cid):
    return [c for c in ref.ragged_cases() if c[0] == cid][0]


def test_component_range(ctx):
    """set_components(1, 1): the same-rank copies and the physical boundaries touch component 1 alone, in ghost and valid cells; back to
    all components the full fill is right again"""
    cid, g, boxes, owner = ragged("ragged3d-p010")
    R = Ranks(ctx, g, boxes, [0] * len(boxes), 3)
    fabs = [ref.new_fab(b, g, NG, 3) for b in boxes]
    full = [f.copy() for f in fabs]
    ref.fill_boundary(boxes, full, g, NG)
    want = [f.copy() for f in fabs]
    for box, w, f in zip(boxes, want, full):
        w[1] = f[1]
        ref.fill_physical(w, ref.origin_of(box, g, NG), g, ref.BCS_A, scomp=1, ncomp=1)
    R.put(fabs)
    ctx.check(ctx.L.qk_ghost_plan_set_components(R.ex[0].h, 1, 1), "set_components")
    R.fill()
    assert_fabs(R.get(), want)
    ctx.check(ctx.L.qk_ghost_plan_set_components(R.ex[0].h, 0, -1), "set_components")
    R.put(fabs)
    R.fill()
    assert_fabs(R.get(), reference_fill(g, boxes, fabs, ref.BCS_A))


DIR3 = {(0, 0): [10.0, 11.0, 12.0], (1, 1): [20.0, 21.0, 22.0]}


def test_boundary_description_cache(ctx):
    """one plan, called with BCRecs A, B, A, then with a Dirichlet model, then without: the device copy of the description follows"""
    cid, g, boxes, owner = ragged("ragged3d-p000")
    R = Ranks(ctx, g, boxes, [0] * len(boxes), 3)
    ex = R.ex[0]
    other = Ranks(ctx, g, boxes, [0] * len(boxes), 3, bcs=ref.BCS_B, dirichlet=DIR3).ex[0]
    A, B, D = ex.bcs, other.bcs, other.dirichlet
    fabs = [ref.new_fab(b, g, NG, 3) for b in boxes]
    for step, (bcs_c, bcs, dir_c, dirichlet) in enumerate([(A, ref.BCS_A, None, None), (B, ref.BCS_B, None, None), (A, ref.BCS_A, None, None),
                                                           (A, ref.BCS_A, D, DIR3), (A, ref.BCS_A, None, None)]):
        ex.bcs, ex.dirichlet = bcs_c, dir_c
        R.put(fabs)
        R.fill()
        want = reference_fill(g, boxes, fabs, bcs, dirichlet)
        assert_fabs(R.get(), want)
        if step in (1, 3):
            assert not all(same(a, b) for a, b in zip(want, reference_fill(g, boxes, fabs, ref.BCS_A))), "the descriptions do not differ"


def test_box_subsets(ctx):
    """LOCAL_ONLY leaves the wall cells of a box marked remote untouched; REMOTE_DEPENDENT after it completes the fill: together they are ALL"""
    cid, g, boxes, owner = ragged("ragged3d-p000")
    R = Ranks(ctx, g, boxes, [0] * len(boxes), 3)
    ex, mf = R.ex[0], R.mf[0]
    L, s = ctx.L, ctx.stream()
    late = 2
    ex.set_box_remote(late, True)
    assert ex.remote_boxes() == [late]
    fabs = [ref.new_fab(b, g, NG, 3) for b in boxes]
    R.put(fabs)
    ctx.check(L.qk_FillBoundary_local(ex.h, s, mf.ptr), "local")
    ctx.check(L.qk_FillPhysicalBoundary_subset(ex.h, s, mf.ptr, ex.bcs, None, capi.BOXES_LOCAL_ONLY), "physbc local")
    want = reference_fill(g, boxes, fabs, ref.BCS_A)
    early = reference_fill(g, boxes, fabs, ref.BCS_A, physbc=False)
    got = R.get()
    for b in range(len(boxes)):
        assert same(got[b], early[b] if b == late else want[b]), f"box {b}"
    assert not same(early[late], want[late])
    i, j, k = ref.axes_of(boxes[late], g, NG)
    beyond = (i[None, None, :] < 0) | (k[:, None, None] < 0) | (k[:, None, None] > g.n_cell[2] - 1) | (j[None, :, None] > g.n_cell[1] - 1)
    assert beyond.any() and np.isnan(got[late][:, beyond]).all()
    ctx.check(L.qk_FillPhysicalBoundary_subset(ex.h, s, mf.ptr, ex.bcs, None, capi.BOXES_REMOTE_DEPENDENT), "physbc remote")
    assert_fabs(R.get(), want)
    ex.set_box_remote(late, False)
    R.put(fabs)
    R.fill()
    assert_fabs(R.get(), want)


def hydro_bcs(nc):
    """reflecting walls of a hydro state: the momentum normal to a wall is odd"""
    return [([ref.REFLECT_ODD if n == 1 + d else ref.REFLECT_EVEN for d in range(3)],) * 2 for n in range(nc)]


@pytest.mark.parametrize("two_ranks", [False, True], ids=["1rank", "2ranks"])
def test_dirichlet_constant_faces_edges_and_corners(ctx, two_ranks):
    """constant states beyond x-lo and y-hi, reflecting walls elsewhere: at edges and corners the first enabled face in x, y, z order wins
    and a disabled face falls through to the BCRec"""
    cid, g, boxes, owner = ragged("ragged3d-p000")
    nc = 6
    dirichlet = {(0, 0): [10.0 + n for n in range(nc)], (1, 1): [20.0 + n for n in range(nc)]}
    R = Ranks(ctx, g, boxes, owner if two_ranks else [0] * len(boxes), nc, bcs=hydro_bcs(nc), dirichlet=dirichlet)
    fabs = [ref.new_fab(b, g, NG, nc) for b in boxes]
    R.put(fabs)
    R.fill()
    assert_fabs(R.get(), reference_fill(g, boxes, fabs, hydro_bcs(nc), dirichlet))


def test_dirichlet_interior_kinetic_and_marshak(ctx):
    """x-hi: the normal momentum follows the cell inside the face and the total energy gets its kinetic energy; x-lo: the Marshak flux.
    Both read a cell INSIDE the domain in x at the ghost cell's own (j, k).  y and z are periodic here, so that cell is either valid or a
    ghost cell FillBoundary filled — never one the boundary launch itself writes; where it would be (a wall in y or z) neither the kernel nor
    the functor it restates defines an order, and there is nothing to test against.  rho = 2 and c = 4 are powers of two and every other
    value is a small integer: 0.5 m^2 / rho and 0.5 c E_inc - 0.5 (c E_0 + 2 F_0) are exact, contracted to FMAs or not."""
    n_cell, boxes = ref.RAGGED[3]
    g = ref.geom(3, n_cell, [0, 1, 1])
    nc = 6
    vals = [2.0, 3.0, 5.0, 7.0, 11.0, 13.0]
    dirichlet = {(0, 1): {"values": vals, "interior": [1], "kinetic_from_interior": True}, (0, 0): {"values": [4.0 + v for v in vals], "marshak": (2, 3, 4.0)}}
    R = Ranks(ctx, g, boxes, [0] * len(boxes), nc, bcs=hydro_bcs(nc), dirichlet=dirichlet)
    fabs = [ref.new_fab(b, g, NG, nc) for b in boxes]
    R.put(fabs)
    R.fill()
    want = reference_fill(g, boxes, fabs, hydro_bcs(nc), dirichlet)
    assert_fabs(R.get(), want)
    assert not any(np.isnan(w).any() for w in want)


@pytest.mark.parametrize("cid,g,boxes,ncomp,bcs", ref.big_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_regions_larger_than_one_grid(ctx, cid, g, boxes, ncomp, bcs):
    """a face strip of 40 x 40 x 4 cells x 11 components = 70 400 values and a wall slab of 132 x 132 x 4 = 69 696 cells: more than the
    65 536 threads of one launch's x grid, so the grid-stride loops of k_copy and k_physbc take a second trip"""
    R = Ranks(ctx, g, boxes, [0], ncomp, bcs=bcs)
    fabs = [ref.new_fab(b, g, NG, ncomp) for b in boxes]
    R.put(fabs)
    R.fill()
    assert_fabs(R.get(), reference_fill(g, boxes, fabs, bcs))


SUM_CASES = [c for c in ref.fill_cases() if c[0].startswith("ragged3d") or c[0] in ("onebox-2x6x4", "narrow-3x6x4")]


@pytest.mark.parametrize("g,boxes,owner", with_ranks(SUM_CASES))
def test_sum_boundary(ctx, g, boxes, owner):
    """every ghost value is added to the valid cell it is a copy of, periodic images any number of periods away included (integer data:
    the order of the atomic adds cannot show)"""
    R = Ranks(ctx, g, boxes, owner, 2)
    fabs = [ref.filled_fab(b, g, NG, 2, tag=t) for t, b in enumerate(boxes)]
    want = [f.copy() for f in fabs]
    ref.sum_boundary(boxes, want, g, NG)
    R.put(fabs)
    R.sum()
    assert_fabs(R.get(), want)


def test_many_items_in_chunks(ctx):
    """2548 boxes of 4^3, all periodic: 66 248 same-rank items, more than the 65 535 one launch can carry in gridDim.y — the ghost plan launches
    them in chunks.  Measured on an MI355X: see the printed line (plan set-up is O(boxes^2 x shifts) on the host)."""
    cid, g, boxes, _ = ref.many_boxes_case()
    t0 = time.perf_counter()
    R = Ranks(ctx, g, boxes, [0] * len(boxes), 1)
    t1 = time.perf_counter()
    assert ctx.L.qk_ghost_plan_num_items(R.ex[0].h, 0, 0) == 66248
    fabs = [ref.new_fab(b, g, NG, 1) for b in boxes]
    want = reference_fill(g, boxes, fabs, None, physbc=False)
    R.put(fabs)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    R.fill()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(f"many items: level + plan set-up {t1 - t0:.2f} s, fill of 66248 items {1e3 * (t3 - t2):.2f} ms")
    assert_fabs(R.get(), want)


# ------------------------------------------------------------------------------------------------ ParallelCopy / ParallelAdd / copy_box
class PcRanks:
    def __init__(self, ctx, g, src_boxes, src_owner, src_ncomp, src_ng, dst_boxes, dst_owner, dst_ncomp, dst_ng, ncomp, **kw):
        self.ctx = ctx
        self.nranks = max(max(src_owner), max(dst_owner)) + 1
        self.smine = [[b for b, o in enumerate(src_owner) if o == r] for r in range(self.nranks)]
        self.dmine = [[b for b, o in enumerate(dst_owner) if o == r] for r in range(self.nranks)]
        self.slev = [Level(ctx, 3, [src_boxes[b] for b in m]) for m in self.smine]
        self.dlev = [Level(ctx, 3, [dst_boxes[b] for b in m]) for m in self.dmine]
        self.src = [MultiFab(lev, src_ncomp, src_ng) for lev in self.slev]
        self.dst = [MultiFab(lev, dst_ncomp, dst_ng) for lev in self.dlev]
        self.plans = [ParallelCopy(ctx, lib_geom(g), src_boxes, src_owner, dst_boxes, dst_owner, ncomp, r, **kw) for r in range(self.nranks)]
        self.ndst = len(dst_boxes)

    def put(self, src, dst):
        for r in range(self.nranks):
            put(self.src[r], [src[b] for b in self.smine[r]])
            put(self.dst[r], [dst[b] for b in self.dmine[r]])

    def get(self):
        out = [None] * self.ndst
        for r, m in enumerate(self.dmine):
            for b, a in zip(m, get(self.dst[r])):
                out[b] = a
        return out

    def run(self, scomp_src, scomp_dst, add):
        ctx, L, s = self.ctx, self.ctx.L, self.ctx.stream()
        if self.nranks == 1:
            self.plans[0](self.src[0], self.dst[0], scomp_src, scomp_dst, add)
            return
        for r, plan in enumerate(self.plans):
            for k, peer, sbuf, rbuf in plan.peers:
                if sbuf.numel():
                    ctx.check(L.qk_ParallelCopy_pack(plan.h, s, k, self.src[r].ptr, scomp_src, vp(sbuf)), "pcopy pack")
        for r, plan in enumerate(self.plans):
            for k, peer, sbuf, rbuf in plan.peers:
                kk = [q for q, pr, _, _ in self.plans[peer].peers if pr == r]
                assert len(kk) == 1
                prbuf = self.plans[peer].peers[kk[0]][3]
                assert prbuf.numel() == sbuf.numel()
                prbuf.copy_(sbuf)
        for r, plan in enumerate(self.plans):
            ctx.check(L.qk_ParallelCopy_local(plan.h, s, self.src[r].ptr, self.dst[r].ptr, scomp_src, scomp_dst, int(add)), "pcopy local")
            for k, peer, sbuf, rbuf in plan.peers:
                if rbuf.numel():
                    ctx.check(L.qk_ParallelCopy_unpack(plan.h, s, k, self.dst[r].ptr, scomp_dst, vp(rbuf), int(add)), "pcopy unpack")


def pc_owners(two_ranks):
    if two_ranks:
        return ref.PC_TILING_OWNER, ref.PC_ODD_OWNER
    return [0] * len(ref.PC_TILING), [0] * len(ref.PC_ODD)


@pytest.mark.parametrize("two_ranks", [False, True], ids=["1rank", "2ranks"])
def test_parallel_copy(ctx, two_ranks):
    """tiling of 8^3 boxes (4 components) -> three odd boxes grown by 3 (5 components), one straddling the periodic x face: components 1-2
    land in components 2-3; the other components and the cells beyond the y walls keep their NaN"""
    g, (town, oown) = ref.PC_GEOM, pc_owners(two_ranks)
    src = [ref.new_fab(b, g, 0, 4) for b in ref.PC_TILING]
    dst = [np.full((5,) + ref.shape_of(b, g, 3), np.nan) for b in ref.PC_ODD]
    want = [d.copy() for d in dst]
    ref.parallel_copy(ref.PC_TILING, src, ref.PC_ODD, want, g, dst_nghost=3, scomp_src=1, scomp_dst=2, ncomp=2)
    P = PcRanks(ctx, g, ref.PC_TILING, town, 4, 0, ref.PC_ODD, oown, 5, 3, 2, dst_nghost=3)
    P.put(src, dst)
    P.run(1, 2, False)
    got = P.get()
    assert_fabs(got, want)
    assert all(np.isnan(a[[0, 1, 4]]).all() and not np.isnan(a[2]).all() for a in got) and np.isnan(got[0][2]).any()


@pytest.mark.parametrize("holes", [None, ref.PC_HOLES], ids=["", "holes"])
@pytest.mark.parametrize("two_ranks", [False, True], ids=["1rank", "2ranks"])
def test_parallel_add_is_deterministic(ctx, two_ranks, holes):
    """the one-cell rings of the odd boxes (4 components) added to the tiling (5 components); two of the boxes abut, so two rings land on one
    cell (tests/test_ghost_reference.py::test_two_rings_land_on_one_cell) and the add groups decide the order; run twice: identical bits"""
    g, (town, oown) = ref.PC_GEOM, pc_owners(two_ranks)
    src = [ref.filled_fab(b, g, 1, 4, tag=t) for t, b in enumerate(ref.PC_ODD)]
    for b, f in zip(ref.PC_ODD, src):
        f[ref.valid_slices(b, g, 1)] = 1.0e300  # the valid cells of a ring-only source never travel
    dst = [ref.new_fab(b, g, 0, 5) for b in ref.PC_TILING]
    want = [d.copy() for d in dst]
    ref.parallel_copy(ref.PC_ODD, src, ref.PC_TILING, want, g, src_nghost=1, src_ring_only=True, holes=holes, scomp_src=1, scomp_dst=2, ncomp=2, add=True)
    P = PcRanks(ctx, g, ref.PC_ODD, oown, 4, 1, ref.PC_TILING, town, 5, 0, 2, src_nghost=1, src_ring_only=True, dst_holes=holes)
    runs = []
    for _ in range(2):
        P.put(src, dst)
        P.run(1, 2, True)
        runs.append(P.get())
    assert_fabs(runs[0], want)
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_copy_box(ctx):
    """a sub-box between two fabs of different origin, ghost width and component count, scomp != dcomp: nothing else changes"""
    g = ref.geom(3, [16, 16, 16], [0, 0, 0])
    sbox, dbox = ([0, 0, 0], [9, 7, 5]), ([2, 1, 0], [12, 9, 6])
    S, D = MultiFab(Level(ctx, 3, [sbox]), 4, 2), MultiFab(Level(ctx, 3, [dbox]), 5, 1)
    src, dst = ref.filled_fab(sbox, g, 2, 4, tag=1), np.full((5,) + ref.shape_of(dbox, g, 1), np.nan)
    put(S, [src])
    put(D, [dst])
    lo, hi = [3, 2, 1], [9, 7, 5]
    ctx.check(ctx.L.qk_copy_box(ctx.h, ctx.stream(), S.host_table[0:1].ctypes.data_as(C.c_void_p), D.host_table[0:1].ctypes.data_as(C.c_void_p),
                                (C.c_int * 3)(*lo), (C.c_int * 3)(*hi), 1, 3, 2), "qk_copy_box")
    so, do = ref.origin_of(sbox, g, 2), ref.origin_of(dbox, g, 1)
    want = dst.copy()
    want[(slice(3, 5),) + tuple(slice(lo[d] - do[d], hi[d] - do[d] + 1) for d in (2, 1, 0))] = \
        src[(slice(1, 3),) + tuple(slice(lo[d] - so[d], hi[d] - so[d] + 1) for d in (2, 1, 0))]
    assert_fabs(get(D), [want])
    assert_fabs(get(S), [src])
