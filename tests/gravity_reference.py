"""numpy restatement of the self-gravity solver (csrc/qk_gravity.hip): the lattice kernel K, James' method on the lattice, the
right-hand side, the kick, and a DIRECT Dirichlet solve by sine transforms (odd-extension FFT).  No GPU, numpy only.

Arrays are dense, shape (N2+2, N1+2, N0+2) (x fastest), cell (i, j, k) of the lattice at [k+1, j+1, i+1]; the ghost layer holds the Dirichlet data at
the centres of the face-adjacent ghost cells.  n = (N0, N1, N2)."""
from __future__ import annotations

import numpy as np

K0 = -0.2527310098586630  # the cubic lattice Green's function at the origin
K1 = K0 + 1.0 / 6.0       # r^2 = 1


def lattice_K(n0, n1, n2):
    """K(n) for integer offsets (arrays broadcast): tabulated at r^2 = 0 and 1, else -1/(4 pi r) * [1 + (-3 + 5 (n0^4+n1^4+n2^4)/r^4) / (8 r^2)]"""
    n0, n1, n2 = (np.asarray(a, dtype=np.int64) for a in (n0, n1, n2))
    r2i = n0 * n0 + n1 * n1 + n2 * n2
    r2 = np.where(r2i < 2, 2, r2i).astype(np.float64)  # (placeholder where tabulated)
    r = np.sqrt(r2)
    n4 = (n0 ** 4 + n1 ** 4 + n2 ** 4).astype(np.float64)
    far = -1.0 / (4.0 * np.pi * r) * (1.0 + (-3.0 + 5.0 * n4 / (r2 * r2)) / (8.0 * r2))
    return np.where(r2i == 0, K0, np.where(r2i == 1, K1, far))


def dense_shape(n):
    return (n[2] + 2, n[1] + 2, n[0] + 2)


def interior(a):
    return a[1:-1, 1:-1, 1:-1]


def ghost_list(n):
    """(S, 3) ghost cells (x, y, z) in list order — x-lo, x-hi, y-lo, y-hi, z-lo, z-hi; within a face the lower tangential direction fastest — and
    (S, 3) their interior neighbours"""
    g, nb = [], []
    for d in range(3):
        ta, tb = (1 if d == 0 else 0), (1 if d == 2 else 2)
        b, a = np.meshgrid(np.arange(n[tb]), np.arange(n[ta]), indexing="ij")
        a, b = a.reshape(-1), b.reshape(-1)
        for side in (0, 1):
            c = np.zeros((a.size, 3), dtype=np.int64)
            c[:, ta], c[:, tb] = a, b
            c[:, d] = -1 if side == 0 else n[d]
            m = c.copy()
            m[:, d] = 0 if side == 0 else n[d] - 1
            g.append(c)
            nb.append(m)
    return np.concatenate(g), np.concatenate(nb)


def at(a, cells):
    """values of the dense array at (S, 3) cells"""
    return a[cells[:, 2] + 1, cells[:, 1] + 1, cells[:, 0] + 1]


def put(a, cells, v):
    a[cells[:, 2] + 1, cells[:, 1] + 1, cells[:, 0] + 1] = v


def surface_potential(n, s, chunk=512, return_abs=False):
    """bc(g) = - sum_g' K(g - g') s(g'); return_abs: also sum_g' |K s| per target (the scale of its rounding error)"""
    g, _ = ghost_list(n)
    S = g.shape[0]
    bc, mag = np.zeros(S), np.zeros(S)
    for t0 in range(0, S, chunk):
        d = g[t0:t0 + chunk, None, :] - g[None, :, :]
        Ks = lattice_K(d[..., 0], d[..., 1], d[..., 2]) * s[None, :]
        bc[t0:t0 + chunk] = -Ks.sum(axis=1)
        mag[t0:t0 + chunk] = np.abs(Ks).sum(axis=1)
    return (bc, mag) if return_abs else bc


def laplacian(phi, h):
    """L phi on the interior cells from the dense array (ghost layer = Dirichlet data)"""
    c = interior(phi)
    return ((phi[1:-1, 1:-1, 2:] - 2.0 * c + phi[1:-1, 1:-1, :-2]) + (phi[1:-1, 2:, 1:-1] - 2.0 * c + phi[1:-1, :-2, 1:-1])
            + (phi[2:, 1:-1, 1:-1] - 2.0 * c + phi[:-2, 1:-1, 1:-1])) / (h * h)


def residual(phi, f, h):
    return interior(f) - laplacian(phi, h)


def _dst1(x, axis):
    """S_k = sum_j x_j sin(pi (j+1)(k+1) / (N+1)) along `axis`, through the FFT of the odd extension of length 2 (N+1)"""
    x = np.moveaxis(x, axis, -1)
    N = x.shape[-1]
    y = np.zeros(x.shape[:-1] + (2 * (N + 1),))
    y[..., 1:N + 1] = x
    y[..., N + 2:] = -x[..., ::-1]
    Y = np.fft.fft(y, axis=-1)
    return np.moveaxis(-0.5 * Y[..., 1:N + 1].imag, -1, axis)


def dirichlet_solve_direct(f, phi_ghost, h):
    """L phi = f with the ghost layer of `phi_ghost` as Dirichlet data: the data moves to the right-hand side, then three sine transforms, a division
    by the eigenvalues (2 cos(pi k / (N+1)) - 2) / h^2 and three inverse transforms.  Returns the dense array, ghost layer kept."""
    rhs = interior(f).copy()
    ih2 = 1.0 / (h * h)
    rhs[:, :, 0] -= phi_ghost[1:-1, 1:-1, 0] * ih2
    rhs[:, :, -1] -= phi_ghost[1:-1, 1:-1, -1] * ih2
    rhs[:, 0, :] -= phi_ghost[1:-1, 0, 1:-1] * ih2
    rhs[:, -1, :] -= phi_ghost[1:-1, -1, 1:-1] * ih2
    rhs[0, :, :] -= phi_ghost[0, 1:-1, 1:-1] * ih2
    rhs[-1, :, :] -= phi_ghost[-1, 1:-1, 1:-1] * ih2
    t = rhs
    lam = 0.0
    for ax in range(3):
        N = t.shape[ax]
        t = _dst1(t, ax)
        shp = [1, 1, 1]
        shp[ax] = N
        lam = lam + ((2.0 * np.cos(np.pi * np.arange(1, N + 1) / (N + 1)) - 2.0) * ih2).reshape(shp)
    t = t / lam
    for ax in range(3):
        t = _dst1(t, ax) * (2.0 / (t.shape[ax] + 1))
    out = phi_ghost.copy()
    interior(out)[...] = t
    return out


def open_solve(f, h):
    """James' method on the lattice, steps 1-4 of DESIGN.md §13, with direct Dirichlet solves.  Returns (phi, bc, phi0)."""
    n = (f.shape[2] - 2, f.shape[1] - 2, f.shape[0] - 2)
    g, nb = ghost_list(n)
    phi0 = dirichlet_solve_direct(f, np.zeros_like(f), h)
    s = at(phi0, nb)
    bc = surface_potential(n, s)
    ghosts = np.zeros_like(f)
    put(ghosts, g, bc)
    return dirichlet_solve_direct(f, ghosts, h), bc, phi0


def fill_rhs(f, rho, G):
    """f += 4.0 * M_PI * G * rho on the interior (rho: (N2, N1, N0))"""
    interior(f)[...] = interior(f) + 4.0 * np.pi * G * rho


def kick(U, phi, dx, dt):
    """the reference's kick (src/QuokkaSimulation.hpp:734-754) on a global (ncomp, N2, N1, N0) state, operations in its order; returns the new state"""
    U = U.copy()
    rho, px, py, pz = U[0], U[1].copy(), U[2].copy(), U[3].copy()
    KE_old = 0.5 * (px * px + py * py + pz * pz) / rho
    gx = -0.5 * (phi[1:-1, 1:-1, 2:] - phi[1:-1, 1:-1, :-2]) / dx[0]
    gy = -0.5 * (phi[1:-1, 2:, 1:-1] - phi[1:-1, :-2, 1:-1]) / dx[1]
    gz = -0.5 * (phi[2:, 1:-1, 1:-1] - phi[:-2, 1:-1, 1:-1]) / dx[2]
    px += dt * rho * gx
    py += dt * rho * gy
    pz += dt * rho * gz
    KE_new = 0.5 * (px * px + py * py + pz * pz) / rho
    U[1], U[2], U[3] = px, py, pz
    U[4] = U[4] + (KE_new - KE_old)
    return U


def max_principle_bound(n, h, res_norm):
    """|phi - phi_exact|_inf <= (W^2 / 8) |residual|_inf, W = (min N_d + 1) h: the discrete maximum principle with the comparison function
    x (W - x) / 2 along the shortest direction (the Dirichlet planes are the ghost centres, W apart)"""
    W = (min(n) + 1) * h
    return W * W / 8.0 * res_norm


def gaussian_case(N, offset=(0.0, 0.0, 0.0), sigma=0.06):
    """unit-mass Gaussian in the unit box [-1/2, 1/2]^3, G = 1: (f dense, h, cell-centre coordinates incl. ghost layer (z, y, x), centre)"""
    h = 1.0 / N
    c = (np.arange(-1, N + 1) + 0.5) * h - 0.5
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    r2 = (x - offset[0]) ** 2 + (y - offset[1]) ** 2 + (z - offset[2]) ** 2
    rho = np.exp(-0.5 * r2 / sigma ** 2) / ((2.0 * np.pi) ** 1.5 * sigma ** 3)
    f = np.zeros((N + 2,) * 3)
    fill_rhs(f, interior(rho), 1.0)
    return f, h, (z, y, x), offset


def gaussian_potential(coords, offset, sigma=0.06):
    from math import erf
    z, y, x = coords
    r = np.sqrt((x - offset[0]) ** 2 + (y - offset[1]) ** 2 + (z - offset[2]) ** 2)
    return -np.vectorize(erf)(r / (np.sqrt(2.0) * sigma)) / r, r
