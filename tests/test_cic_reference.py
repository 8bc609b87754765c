"""The numpy restatement of the CIC particles (tests/cic_reference.py) against what it must do physically: no GPU.  The last test is the
reference's BinaryOrbit pass criterion on the two-body fixture, through the direct open-boundary solve of gravity_reference.py."""
import os

import numpy as np

import cic_reference as cr
import gravity_reference as gr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, PLO, DX = (8, 6, 4), (0.25, -1.75, 11.0), (0.25, 0.25, 0.25)  # (dyadic: cell centres and faces are exact)
PHI = tuple(PLO[d] + N[d] * DX[d] for d in range(3))
VOL = DX[0] * DX[1] * DX[2]


def centre(c):
    return np.array([PLO[d] + (c[d] + 0.5) * DX[d] for d in range(3)])


def test_particle_at_a_cell_centre_deposits_into_exactly_one_cell():
    G, m = 0.7, 3.0
    for c in [(0, 0, 0), (3, 2, 1), (7, 5, 3)]:
        f = cr.particle_rhs(N, PLO, DX, centre(c)[None, :], np.array([m]), G)
        nz = np.argwhere(f != 0.0)
        assert nz.tolist() == [[c[2] + 1, c[1] + 1, c[0] + 1]]
        assert abs(f[c[2] + 1, c[1] + 1, c[0] + 1] - ((4.0 * np.pi) * G) * m * (1.0 / VOL)) <= 1.0e-12 * m / VOL


def test_deposit_conserves_mass_half_a_cell_inside():
    rng = np.random.default_rng(3)
    lo, hi = np.array(PLO) + 0.5 * DX[0], np.array(PHI) - 0.5 * DX[0]
    pos = lo + rng.random((400, 3)) * (hi - lo)
    mass = 10.0 ** rng.uniform(-3, 3, 400)
    G = 0.37
    f = cr.particle_rhs(N, PLO, DX, pos, mass, G)
    total, want = gr.interior(f).sum() * VOL, 4.0 * np.pi * G * mass.sum()
    assert abs(total - want) <= 1.0e-12 * want
    assert not f[0].any() and not f[-1].any() and not f[:, 0].any() and not f[:, -1].any() and not f[:, :, 0].any() and not f[:, :, -1].any()


def test_linear_potential_gives_every_particle_minus_the_slope():
    slope = np.array([1.5, -0.25, 3.0])
    c = [PLO[d] + (np.arange(-1, N[d] + 1) + 0.5) * DX[d] for d in range(3)]
    z, y, x = np.meshgrid(c[2], c[1], c[0], indexing="ij")
    phi = slope[0] * x + slope[1] * y + slope[2] * z
    rng = np.random.default_rng(5)
    pos = np.array(PLO) + rng.uniform(-1.5, 1.5, (200, 3)) * np.array(DX) + rng.random((200, 3)) * (np.array(PHI) - np.array(PLO))
    pos[:8] = [[PLO[0] - 7.0, PHI[1] + 5.0, PLO[2] + 0.1], PLO, PHI, [PHI[0], PLO[1], PHI[2]], centre((0, 0, 0)), centre((7, 5, 3)),
               [1.0e300, -1.0e300, 1.0e300], [PLO[0], PHI[1] + 100.0, PLO[2] - 100.0]]
    dt = 0.125
    v = cr.kick(N, PLO, DX, pos, np.zeros_like(pos), phi, dt)
    acc = v / (0.5 * dt)
    assert np.abs(acc + slope[None, :]).max() <= 1.0e-10 * np.abs(slope).max()


def test_weights_dropped_at_each_of_the_six_faces():
    G, m = 1.0, 2.0
    full = ((4.0 * np.pi) * G) * m * (1.0 / VOL)
    for d in range(3):
        for side in (0, 1):
            c = [3, 2, 1]
            c[d] = 0 if side == 0 else N[d] - 1
            x = centre(c)
            x[d] += (-0.25 if side == 0 else 0.25) * DX[d]  # a quarter of a cell towards the face: a quarter of the mass falls outside
            f = cr.particle_rhs(N, PLO, DX, x[None, :], np.array([m]), G)
            nz = np.argwhere(f != 0.0)
            assert nz.tolist() == [[c[2] + 1, c[1] + 1, c[0] + 1]], "the dropped weight was written somewhere"
            assert abs(f[c[2] + 1, c[1] + 1, c[0] + 1] - 0.75 * full) <= 1.0e-12 * full
            # up to one cell outside it still reaches the boundary cell; beyond that nothing
            x[d] = (PLO[d] - 0.25 * DX[d]) if side == 0 else (PHI[d] + 0.25 * DX[d])
            f = cr.particle_rhs(N, PLO, DX, x[None, :], np.array([m]), G)
            assert abs(f[c[2] + 1, c[1] + 1, c[0] + 1] - 0.25 * full) <= 1.0e-12 * full and np.count_nonzero(f) == 1
            x[d] = (PLO[d] - 0.75 * DX[d]) if side == 0 else (PHI[d] + 0.75 * DX[d])
            assert not cr.particle_rhs(N, PLO, DX, x[None, :], np.array([m]), G).any()
            assert cr.cell_keys(N, PLO, DX, x[None, :])[0] == cr.num_keys(N)


def test_two_body_orbit_meets_the_reference_criterion():
    """BinaryOrbit_particles.txt on 32^3 over [-2.5e13, 2.5e13]^3, particles alone, 120 steps at dt = 0.3 dx / 1.3e7: the worst
    |separation - 6.25e12| / dx over every step within 0.18 cell widths (the reference's max_err_tol)."""
    n, plo, phi_ = (32, 32, 32), (-2.5e13,) * 3, (2.5e13,) * 3
    dx = (5.0e13 / 32,) * 3
    G = 6.67430e-8
    pos, mass, vel = cr.read_ascii(os.path.join(GOLDEN, "BinaryOrbit_particles.txt"))
    assert pos.shape == (2, 3)
    dt = 0.3 * dx[0] / 1.3e7

    # gr.open_solve with the S x S matrix of the lattice kernel formed once (from a table over the offsets) instead of once per solve
    g, nb = gr.ghost_list(n)
    r = np.arange(-(n[0] + 1), n[0] + 2)
    table = gr.lattice_K(r[:, None, None], r[None, :, None], r[None, None, :])
    K = np.empty((g.shape[0], g.shape[0]))
    for t0 in range(0, g.shape[0], 512):
        d = g[t0:t0 + 512, None, :] - g[None, :, :] + (n[0] + 1)
        K[t0:t0 + 512] = table[d[..., 0], d[..., 1], d[..., 2]]

    def solve(rhs):
        phi0 = gr.dirichlet_solve_direct(rhs, np.zeros_like(rhs), dx[0])
        ghosts = np.zeros_like(rhs)
        gr.put(ghosts, g, -(K @ gr.at(phi0, nb)))
        return gr.dirichlet_solve_direct(rhs, ghosts, dx[0])

    phi = solve(cr.particle_rhs(n, plo, dx, pos, mass, G))
    worst = 0.0
    for _ in range(120):
        pos, vel, mass, phi = cr.step(n, plo, phi_, dx, pos, vel, mass, G, phi, dt, solve)
        assert pos.shape == (2, 3)
        worst = max(worst, abs(np.sqrt(((pos[0] - pos[1]) ** 2).sum()) - 6.25e12) / dx[0])
    print(f"worst separation error over 120 steps: {worst:.4f} cell widths; momentum {(mass[:, None] * vel).sum(axis=0)}")
    assert worst <= 0.18
