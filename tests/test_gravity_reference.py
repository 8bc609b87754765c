"""The numpy restatement of the self-gravity solver (tests/gravity_reference.py) against what is known in closed form: the potential
of a Gaussian, the exact lattice Green's function at three offsets, and the discrete equation itself.  No GPU."""
import numpy as np
import pytest

import gravity_reference as gr

OFFSET = (0.12, -0.07, 0.05)


@pytest.fixture(scope="module")
def gaussian_runs():
    out = {}
    for name, off in (("centred", (0.0, 0.0, 0.0)), ("offset", OFFSET)):
        for N in (16, 32):
            f, h, coords, _ = gr.gaussian_case(N, off)
            phi, bc, _ = gr.open_solve(f, h)
            exact, r = gr.gaussian_potential(coords, off)
            g, _ = gr.ghost_list((N, N, N))
            err = np.abs(gr.interior(phi) - gr.interior(exact)).max() / np.abs(gr.interior(exact)).max()
            out[name, N] = dict(f=f, h=h, phi=phi, bc=bc, err=err, bc_dev=np.abs(bc * gr.at(r, g) + 1.0).max())
    return out


@pytest.mark.parametrize("name", ["centred", "offset"])
def test_gaussian_potential_converges_at_second_order(gaussian_runs, name):
    e16, e32 = gaussian_runs[name, 16]["err"], gaussian_runs[name, 32]["err"]
    print(f"{name}: max|phi - exact| / max|exact| = {e16:.3e} (16), {e32:.3e} (32), ratio {e32 / e16:.3f}")
    assert e32 <= 0.35 * e16


@pytest.mark.parametrize("name", ["centred", "offset"])
def test_boundary_data_is_the_point_mass_potential(gaussian_runs, name):
    dev = gaussian_runs[name, 32]["bc_dev"]
    print(f"{name}: max|bc r + 1| at 32 = {dev:.3e}")
    assert dev <= 1.5e-3


@pytest.mark.parametrize("name", ["centred", "offset"])
@pytest.mark.parametrize("N", [16, 32])
def test_discrete_equation_holds(gaussian_runs, name, N):
    run = gaussian_runs[name, N]
    res = np.abs(gr.residual(run["phi"], run["f"], run["h"])).max()
    assert res <= 1.0e-10 * np.abs(run["f"]).max()
    # the ghost layer of phi is bc, in list order
    g, _ = gr.ghost_list((N, N, N))
    assert np.array_equal(gr.at(run["phi"], g), run["bc"])


@pytest.mark.parametrize("n,exact,rel", [((1, 1, 0), -0.0551914338, 1.5e-2), ((2, 1, 0), -0.0359316026, 1.0e-3), ((4, 4, 4), -0.0114456699, 1.0e-4)])
def test_lattice_kernel_against_exact_values(n, exact, rel):
    for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        for sign in (1, -1):
            k = float(gr.lattice_K(*[sign * n[p] for p in perm]))
            assert abs(k - exact) <= rel * abs(exact), (n, k, exact)


def test_lattice_kernel_tabulated_offsets():
    assert float(gr.lattice_K(0, 0, 0)) == gr.K0 == -0.2527310098586630
    for n in ((1, 0, 0), (0, -1, 0), (0, 0, 1)):
        assert float(gr.lattice_K(*n)) == gr.K0 + 1.0 / 6.0


def test_direct_solve_with_random_ghost_data():
    rng = np.random.default_rng(3)
    n, h = (6, 4, 8), 0.37
    f = np.zeros(gr.dense_shape(n))
    gr.interior(f)[...] = rng.standard_normal(gr.interior(f).shape)
    ghosts = np.zeros_like(f)
    g, nb = gr.ghost_list(n)
    assert g.shape[0] == 2 * (n[0] * n[1] + n[1] * n[2] + n[0] * n[2]) and len({tuple(c) for c in g}) == g.shape[0]
    assert np.array_equal(np.abs(g - nb).sum(axis=1), np.ones(g.shape[0], dtype=np.int64))
    gr.put(ghosts, g, rng.standard_normal(g.shape[0]))
    phi = gr.dirichlet_solve_direct(f, ghosts, h)
    assert np.abs(gr.residual(phi, f, h)).max() <= 1.0e-10 * np.abs(f).max() / 1.0


def test_kick_and_rhs_by_hand():
    n = (4, 4, 4)
    phi = np.zeros(gr.dense_shape(n))
    phi[:, :, :] = np.arange(6)[None, None, :] * 2.0  # phi = 2 (i + 1): g_x = -2 / dx
    U = np.zeros((6, 4, 4, 4))
    U[0], U[1], U[4] = 2.0, 1.0, 5.0
    V = gr.kick(U, phi, (0.5, 0.5, 0.5), 0.25)
    assert np.all(V[1] == 1.0 + 0.25 * 2.0 * (-4.0)) and np.all(V[2] == 0.0) and np.all(V[0] == 2.0) and np.all(V[5] == 0.0)
    assert np.all(V[4] == 5.0 + (0.5 * 1.0 / 2.0 - 0.5 * 1.0 / 2.0))
    f = np.ones(gr.dense_shape(n))
    gr.fill_rhs(f, U[0], 3.0)
    assert np.all(gr.interior(f) == 1.0 + 4.0 * np.pi * 3.0 * 2.0) and f[0, 0, 0] == 1.0
