"""numpy restatement of the CIC particles (csrc/qk_cic.hip): stencil, keys, deposit, kick, drift and the order of one step, every
operation in the order §14 writes it, so that the kernels can be compared bit for bit.  No GPU, numpy only; beside gravity_reference.py, whose dense
arrays (shape (N2+2, N1+2, N0+2), cell (i, j, k) at [k+1, j+1, i+1]) it shares.  n = (N0, N1, N2); pos, vel: (np, 3); mass: (np,)."""
from __future__ import annotations

import numpy as np

import gravity_reference as gr


def stencil(n, plo, dx, pos):
    """(l, bf, w): lattice coordinate (np, 3), its floor as a double (np, 3), the weights (np, 3, 2)"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    dxi = 1.0 / np.asarray(dx, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        l = (pos - np.asarray(plo, dtype=np.float64)[None, :]) * dxi[None, :] - 0.5
        bf = np.floor(l)
        t = l - bf
        w = np.stack([1.0 - t, t], axis=2)
    return l, bf, w


def takes_part(n, l):
    N = np.asarray(n, dtype=np.float64)[None, :]
    return ((l >= -1.0) & (l < N)).all(axis=1)


def num_keys(n):
    return (n[0] + 1) * (n[1] + 1) * (n[2] + 1)


def cell_keys(n, plo, dx, pos):
    """the key of the base cell per particle, the sentinel num_keys(n) where it does not take part"""
    l, bf, _ = stencil(n, plo, dx, pos)
    part = takes_part(n, l)
    b = np.where(part[:, None], bf, -1.0).astype(np.int64)
    keys = (b[:, 0] + 1) + (n[0] + 1) * ((b[:, 1] + 1) + (n[1] + 1) * (b[:, 2] + 1))
    return np.where(part, keys, num_keys(n))


def contributions(n, plo, dx, pos, mass, G):
    """every (cell, value) the deposit adds, in the fixed order of one cell's sum: returns a dict cell (i, j, k) -> list of W * (((4 pi) G) m),
    sorted by (kk, jj, ii) of the source offset (kk outermost, ii fastest) and, within one base cell, by storage index"""
    l, bf, w = stencil(n, plo, dx, pos)
    part = takes_part(n, l)
    mass = np.asarray(mass, dtype=np.float64)
    out = {}
    for p in np.nonzero(part)[0]:
        b = bf[p].astype(np.int64)
        q = ((4.0 * np.pi) * G) * mass[p]
        for kk in range(2):
            for jj in range(2):
                for ii in range(2):
                    c = (int(b[0]) + ii, int(b[1]) + jj, int(b[2]) + kk)
                    if not all(0 <= c[d] < n[d] for d in range(3)):
                        continue  # a weight outside the domain is dropped
                    W = (w[p, 0, ii] * w[p, 1, jj]) * w[p, 2, kk]
                    out.setdefault(c, []).append(((kk, jj, ii), int(p), W * q))
    return {c: [v for _, _, v in sorted(lst, key=lambda e: (e[0], e[1]))] for c, lst in out.items()}


def deposit(f, n, plo, dx, pos, mass, G, order=None):
    """write (sum W 4 pi G m) * (1 / vol) into the cells of the dense array f that a particle reaches (the others are not written).  order: a function
    that permutes one cell's list of contributions (the test that shows the sum is order-sensitive)"""
    inv_vol = 1.0 / (dx[0] * dx[1] * dx[2])
    for (i, j, k), vals in contributions(n, plo, dx, pos, mass, G).items():
        if order is not None:
            vals = order(vals)
        s = 0.0
        for v in vals:
            s = s + v
        f[k + 1, j + 1, i + 1] = s * inv_vol
    return f


def kick(n, plo, dx, pos, vel, phi, dt):
    """vel_d += (0.5 dt) * (W * a_d) over the eight stencil cells (kk outermost, ii fastest), d outermost; indices clamped to [0, N - 1] on the
    double; a_d = -0.5 * dxi_d * (phi(c + e_d) - phi(c - e_d)).  Returns the new velocities."""
    _, bf, w = stencil(n, plo, dx, pos)
    dxi = 1.0 / np.asarray(dx, dtype=np.float64)
    v = np.array(vel, dtype=np.float64).reshape(-1, 3).copy()
    half_dt = 0.5 * dt

    def clamp(d, o):
        with np.errstate(invalid="ignore"):
            x = bf[:, d] + float(o)
            return np.where(x >= 0.0, np.where(x <= float(n[d] - 1), x, float(n[d] - 1)), 0.0).astype(np.int64)

    for d in range(3):
        e = [1 if d == 0 else 0, 1 if d == 1 else 0, 1 if d == 2 else 0]
        for kk in range(2):
            for jj in range(2):
                for ii in range(2):
                    ci, cj, ck = clamp(0, ii), clamp(1, jj), clamp(2, kk)
                    W = (w[:, 0, ii] * w[:, 1, jj]) * w[:, 2, kk]
                    up = phi[ck + 1 + e[2], cj + 1 + e[1], ci + 1 + e[0]]
                    dn = phi[ck + 1 - e[2], cj + 1 - e[1], ci + 1 - e[0]]
                    acc = -0.5 * dxi[d] * (up - dn)
                    v[:, d] = v[:, d] + half_dt * (W * acc)
    return v


def drift(pos, vel, dt):
    return np.asarray(pos, dtype=np.float64) + dt * np.asarray(vel, dtype=np.float64)


def inside(plo, phi_, pos):
    """Redistribute on a non-periodic domain: the particles in [plo, phi) in every direction stay"""
    pos = np.asarray(pos)
    return ((pos >= np.asarray(plo)[None, :]) & (pos < np.asarray(phi_)[None, :])).all(axis=1)


def particle_rhs(n, plo, dx, pos, mass, G):
    return deposit(np.zeros(gr.dense_shape(n)), n, plo, dx, pos, mass, G)


def step(n, plo, phi_, dx, pos, vel, mass, G, phi_old, dt, solve):
    """one step for particles alone (the gas is left out): kick(phi at t), Redistribute, drift, solve, kick(phi at t + dt).
    solve(rhs) -> the dense potential.  Returns (pos, vel, mass, phi_new)."""
    vel = kick(n, plo, dx, pos, vel, phi_old, dt)
    keep = inside(plo, phi_, pos)
    pos, vel, mass = pos[keep], vel[keep], mass[keep]
    pos = drift(pos, vel, dt)
    phi_new = solve(particle_rhs(n, plo, dx, pos, mass, G))
    vel = kick(n, plo, dx, pos, vel, phi_new, dt)
    return pos, vel, mass, phi_new


def read_ascii(path):
    """count, then x y z mass vx vy vz per line -> (pos, mass, vel)"""
    tok = open(path).read().split()
    n = int(tok[0])
    a = np.array([float(t) for t in tok[1:1 + 7 * n]]).reshape(n, 7)
    return a[:, 0:3].copy(), a[:, 3].copy(), a[:, 4:7].copy()
