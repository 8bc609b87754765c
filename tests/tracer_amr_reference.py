"""numpy restatement of the tracer kernels on a refined hierarchy (include/quokka_amd.h "tracer particles on a refined hierarchy", DESIGN.md §11
"refined levels"), written from that text on top of tests/tracer_reference.py: per level ONE global face array at that level's resolution — the
level's own faces where it holds them, the parent's (time first, then space) elsewhere, recursively — handed to the single-level `advect`; and
`where`, the level a particle belongs to.  Every operation rounds once, in the order the header states: the GPU tests compare bit for bit."""
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

import tracer_reference as tr

Box = Tuple[Sequence[int], Sequence[int]]


@dataclass
class LevelFaces:
    """one level's face data of one kind (prev / cur): its geometry, the boxes of the plan that belongs to the data, and per direction the
    boxes' arrays (each shaped as tr.box_faces gives them: the box's top face included)"""
    g: tr.TracerGeom
    boxes: List[Box]
    fabs: List[List[np.ndarray]] = field(default_factory=list)  # [d][box]


def level_geom(g0: tr.TracerGeom, lev: int) -> tr.TracerGeom:
    return tr.TracerGeom(g0.ndim, [n * 2 ** lev for n in g0.n_cell], g0.prob_lo, g0.prob_hi, g0.periodic)


def cell_mask(g: tr.TracerGeom, boxes: Sequence[Box]) -> np.ndarray:
    """cells a box covers, indexed [k, j, i]"""
    m = np.zeros(tuple(reversed(g.n_cell[:g.ndim])), dtype=bool)
    for lo, hi in boxes:
        m[tuple(slice(lo[e], hi[e] + 1) for e in reversed(range(g.ndim)))] = True
    return m


def held_and_own(L: LevelFaces, d: int):
    """(held, own): which faces of direction d the level holds — a face belongs to the box whose low face it is, the domain's top face to the
    last box — and their stored values (NaN elsewhere)"""
    g = L.g
    held = np.zeros(tr.face_shape(g, d), dtype=bool)
    own = np.full(tr.face_shape(g, d), np.nan)
    for (lo, hi), fab in zip(L.boxes, L.fabs[d]):
        a = np.asarray(fab).reshape(tuple(hi[e] - lo[e] + 1 + (1 if e == d else 0) for e in reversed(range(g.ndim))))
        top = hi[d] + 1 == g.n_cell[d]
        dst = tuple(slice(lo[e], hi[e] + 1 + (1 if (e == d and top) else 0)) for e in reversed(range(g.ndim)))
        src = tuple(slice(0, hi[e] - lo[e] + 1 + (1 if (e == d and top) else 0)) for e in reversed(range(g.ndim)))
        held[dst] = True
        own[dst] = a[src]
    return held, own


def from_parent(g: tr.TracerGeom, gp: tr.TracerGeom, d: int, P: np.ndarray) -> np.ndarray:
    """rule 3 for EVERY face of direction d of the level with geometry g, P the parent's global face array:
    (1 - w) P(c) + w P(c + e_d), c = floor(i / 2), w = 0.5 (i_d - 2 c_d); c and c + e_d resolved against the parent's domain"""
    nd = g.ndim
    shape = tr.face_shape(g, d)
    grids = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")  # [k, j, i] order
    i = {e: grids[nd - 1 - e] for e in range(nd)}
    c = {e: i[e] // 2 for e in range(nd)}
    w = 0.5 * (i[d] - 2 * c[d]).astype(np.float64)

    def at(shift):
        idx = [tr.resolve(c[e] + (shift if e == d else 0), gp.n_cell[e], bool(gp.periodic[e]), e == d) for e in range(nd)]
        return P[tuple(idx[e] for e in reversed(range(nd)))]

    return (1.0 - w) * at(0) + w * at(1)


def compose_pure(levels: Sequence[LevelFaces], lev: int, d: int) -> np.ndarray:
    """U^K of level `lev` on every face of its domain, for the kind the LevelFaces hold: stored where held, rule 3 on the parent's U^K elsewhere"""
    held, own = held_and_own(levels[lev], d)
    if lev == 0:
        assert held.all(), "level 0 holds every face"
        return own
    return np.where(held, own, from_parent(levels[lev].g, levels[lev - 1].g, d, compose_pure(levels, lev - 1, d)))


def blend(alpha: float, beta: float, prev: np.ndarray, cur: np.ndarray) -> np.ndarray:
    """G = alpha U^prev + beta U^cur; alpha == 0: cur alone, beta == 0: prev alone (the almostEqual short cuts)"""
    if alpha == 0.0:
        return cur
    if beta == 0.0:
        return prev
    return alpha * prev + beta * cur


def compose_field(cur: Sequence[LevelFaces], prev: Sequence[LevelFaces], lev: int, alpha: float, beta: float) -> List[np.ndarray]:
    """rule 4: the global face arrays a particle of level `lev` is advected with.  cur[lev] holds the level's own avgFaceVel; cur[m], prev[m],
    m < lev, the ancestors' of their current and previous steps (prev with the boxes that step had)"""
    out = []
    for d in range(cur[lev].g.ndim):
        held, own = held_and_own(cur[lev], d)
        if lev == 0:
            assert held.all()
            out.append(own)
            continue
        G = blend(alpha, beta, compose_pure(prev, lev - 1, d), compose_pure(cur, lev - 1, d))
        out.append(np.where(held, own, from_parent(cur[lev].g, cur[lev - 1].g, d, G)))
    return out


def advect(cur: Sequence[LevelFaces], prev: Sequence[LevelFaces], lev: int, alpha: float, beta: float, dt: float, pos: np.ndarray):
    return tr.advect(cur[lev].g, compose_field(cur, prev, lev, alpha, beta), dt, pos)


def stencil_classes(L: LevelFaces, field_: List[np.ndarray], dt: float, pos: np.ndarray):
    """per particle, over both passes and all components: (number of stencil faces held, number not held, fallback faces with odd normal index,
    with even normal index)"""
    g = L.g
    nd = g.ndim
    v0 = tr.interp_all(g, field_, pos)
    xm = pos + (0.5 * dt) * v0
    n_held = np.zeros(pos.shape[0], dtype=int)
    n_off = np.zeros(pos.shape[0], dtype=int)
    odd = np.zeros(pos.shape[0], dtype=int)
    even = np.zeros(pos.shape[0], dtype=int)
    for x in (pos, xm):
        for d in range(nd):
            held, _ = held_and_own(L, d)
            i0 = []
            for e in range(nd):
                l = (x[:, e] - g.prob_lo[e]) * g.dxi[e]
                if e != d:
                    l = l - 0.5
                i0.append(np.floor(l).astype(np.int64))
            for s in range(2 ** nd):
                idx = [tr.resolve(i0[e] + ((s >> e) & 1), g.n_cell[e], bool(g.periodic[e]), e == d) for e in range(nd)]
                h = held[tuple(idx[e] for e in reversed(range(nd)))]
                n_held += h
                n_off += ~h
                odd += (~h) & (idx[d] % 2 == 1)
                even += (~h) & (idx[d] % 2 == 0)
    return n_held, n_off, odd, even


def where(geoms: Sequence[tr.TracerGeom], boxes: Sequence[Sequence[Box]], lev_min: int, ngrow: int, pos: np.ndarray, level: np.ndarray):
    """qk_tracer_Where: (positions after the periodic shift, new level per particle (-1: dropped), keep)"""
    g0 = geoms[0]
    nd = g0.ndim
    pos, keep = tr.redistribute(g0, pos)
    nlev = len(geoms)
    masks = [cell_mask(geoms[m], boxes[m]) for m in range(nlev)]
    assert masks[0].all()

    def cells(m):
        out = []
        for e in range(nd):
            with np.errstate(invalid="ignore"):
                i = np.floor((pos[:, e] - g0.prob_lo[e]) * geoms[m].dxi[e])
            i = np.where(np.isfinite(i), i, 0.0).astype(np.int64)
            out.append(np.clip(i, 0, geoms[m].n_cell[e] - 1))
        return out

    stays = np.zeros(pos.shape[0], dtype=bool)
    if ngrow > 0:  # (c): within ngrow cells (no periodic wrap) of a cell of a box of its own level
        for m in range(nlev):
            grown = masks[m].copy()
            for _ in range(ngrow):  # one cell per pass, one direction after the other: diagonals included
                for ax in range(nd):
                    a = grown.copy()
                    sl_lo = [slice(None)] * nd
                    sl_hi = [slice(None)] * nd
                    sl_lo[ax], sl_hi[ax] = slice(0, -1), slice(1, None)
                    a[tuple(sl_lo)] |= grown[tuple(sl_hi)]
                    a[tuple(sl_hi)] |= grown[tuple(sl_lo)]
                    grown = a
            c = cells(m)
            stays |= grown[tuple(c[e] for e in reversed(range(nd)))] & (level == m)
    finest = np.zeros(pos.shape[0], dtype=np.int32)
    for m in range(nlev):  # (d): the finest level that holds the cell — over [lev_min, finest] first and the levels below next is the same order
        c = cells(m)
        finest = np.where(masks[m][tuple(c[e] for e in reversed(range(nd)))], m, finest).astype(np.int32)
    new = np.where(stays, level, finest).astype(np.int32)
    new[~keep] = -1
    return pos, new, keep
