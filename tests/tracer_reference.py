"""numpy restatement of the tracer-particle kernels (include/quokka_amd.h "tracer particles"), written from that text: a global
face array per direction, indices outside the domain wrapped (periodic) or clamped (everything else), the same association order.  HIP with
contraction off and numpy both round every operation once: the GPU tests compare bit for bit."""
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np


@dataclass
class TracerGeom:
    ndim: int
    n_cell: Sequence[int]
    prob_lo: Sequence[float]
    prob_hi: Sequence[float]
    periodic: Sequence[int]

    def __post_init__(self):
        self.dx = [(self.prob_hi[d] - self.prob_lo[d]) / self.n_cell[d] for d in range(self.ndim)]  # as quokka_amd.simulation.Geometry
        self.dxi = [1.0 / h for h in self.dx]


def face_shape(g: TracerGeom, d: int):
    """shape of the global face array of direction d, indexed [k, j, i] (2-D: [j, i], 1-D: [i])"""
    return tuple(g.n_cell[e] + (1 if e == d else 0) for e in reversed(range(g.ndim)))


def resolve(i: np.ndarray, n: int, periodic: bool, face: bool) -> np.ndarray:
    """a stencil index -> the array index it reads: modulo n in a periodic direction (face n == face 0), else clamped to [0, n - 1] (cells) or
    [0, n] (faces of the normal direction)"""
    if periodic:
        return np.mod(i, n)
    return np.clip(i, 0, n if face else n - 1)


def interp_mac(g: TracerGeom, u: np.ndarray, d: int, x: np.ndarray) -> np.ndarray:
    """I_d(x): u the global face array of direction d, x (np, ndim)"""
    nd = g.ndim
    idx, s = [], []
    for e in range(nd):
        l = (x[:, e] - g.prob_lo[e]) * g.dxi[e]
        if e != d:
            l = l - 0.5
        i0 = np.floor(l).astype(np.int64)
        w = l - i0.astype(np.float64)
        s.append((1.0 - w, w))
        idx.append(tuple(resolve(i0 + ii, g.n_cell[e], bool(g.periodic[e]), e == d) for ii in (0, 1)))
    acc = np.zeros(x.shape[0])
    for kk in ((0, 1) if nd > 2 else (0,)):
        for jj in ((0, 1) if nd > 1 else (0,)):
            for ii in (0, 1):
                w = s[0][ii]
                if nd > 1:
                    w = w * s[1][jj]
                if nd > 2:
                    w = w * s[2][kk]
                if nd == 3:
                    val = u[idx[2][kk], idx[1][jj], idx[0][ii]]
                elif nd == 2:
                    val = u[idx[1][jj], idx[0][ii]]
                else:
                    val = u[idx[0][ii]]
                acc = acc + w * val
    return acc


def interp_all(g: TracerGeom, umac: List[np.ndarray], x: np.ndarray) -> np.ndarray:
    return np.stack([interp_mac(g, umac[d], d, x) for d in range(g.ndim)], axis=1)


def advect(g: TracerGeom, umac: List[np.ndarray], dt: float, pos: np.ndarray):
    """both passes of the predictor-corrector: returns (new positions, velocities)"""
    hdt = 0.5 * dt
    v0 = interp_all(g, umac, pos)
    xm = pos + hdt * v0
    v1 = interp_all(g, umac, xm)
    return pos + dt * v1, v1


def redistribute(g: TracerGeom, pos: np.ndarray):
    """returns (positions after the periodic shift, keep)"""
    pos = pos.copy()
    keep = np.ones(pos.shape[0], dtype=bool)
    for e in range(g.ndim):
        plo, phi = g.prob_lo[e], g.prob_hi[e]
        x = pos[:, e]
        if g.periodic[e]:
            length = phi - plo
            outside = ~((x >= plo) & (x < phi))
            with np.errstate(invalid="ignore"):
                xs = x - np.floor((x - plo) / length) * length  # any number of periods; one period: exactly x -+ length
            xs = np.where((xs < plo) | (xs >= phi), plo, xs)    # below plo, or on phi, through rounding (a NaN stays a NaN and is dropped)
            x = np.where(outside, xs, x)
            pos[:, e] = x
        keep &= (x >= plo) & (x < phi)
    return pos, keep


def init_one_per_cell(g: TracerGeom, boxes, off=0.5, first_id=1):
    """positions (np, ndim) and ids: boxes in order, cells in Fortran order (i fastest)"""
    out = []
    for lo, hi in boxes:
        rng = [np.arange(lo[e], hi[e] + 1) if e < g.ndim else np.arange(1) for e in range(3)]
        k, j, i = np.meshgrid(rng[2], rng[1], rng[0], indexing="ij")
        cell = (i.reshape(-1), j.reshape(-1), k.reshape(-1))
        out.append(np.stack([g.prob_lo[e] + (cell[e].astype(np.float64) + off) * g.dx[e] for e in range(g.ndim)], axis=1))
    pos = np.concatenate(out, axis=0)
    return pos, first_id + np.arange(pos.shape[0], dtype=np.int64)


def random_faces(g: TracerGeom, rng, scale=1.0) -> List[np.ndarray]:
    return [scale * rng.uniform(-1.0, 1.0, size=face_shape(g, d)) for d in range(g.ndim)]


def box_faces(g: TracerGeom, u: np.ndarray, d: int, lo, hi) -> np.ndarray:
    """the part of the global face array of direction d that box [lo, hi] holds (its top face included), shaped (1, nz, ny, nx) like a fab"""
    sl = tuple(slice(lo[e], hi[e] + 1 + (1 if e == d else 0)) for e in reversed(range(g.ndim)))
    return u[sl].reshape((1,) + (1,) * (3 - g.ndim) + u[sl].shape)


def assemble_faces(g: TracerGeom, d: int, boxes, fabs: List[np.ndarray]) -> np.ndarray:
    """global face array of direction d from the boxes' arrays (each (1, nz, ny, nx)): a face shared by two boxes is taken from the box whose
    low face it is, the domain's top face from the last box"""
    u = np.full(face_shape(g, d), np.nan)
    for (lo, hi), fab in zip(boxes, fabs):
        a = np.asarray(fab).reshape(tuple(hi[e] - lo[e] + 1 + (1 if e == d else 0) for e in reversed(range(g.ndim))))
        top = hi[d] + 1 == g.n_cell[d]
        dst = tuple(slice(lo[e], hi[e] + 1 + (1 if (e == d and top) else 0)) for e in reversed(range(g.ndim)))
        src = tuple(slice(0, hi[e] - lo[e] + 1 + (1 if (e == d and top) else 0)) for e in reversed(range(g.ndim)))
        u[dst] = a[src]
    assert not np.isnan(u).any()
    return u
