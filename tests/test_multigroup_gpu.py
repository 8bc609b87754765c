"""GPU parity of the MULTIGROUP radiation path (qk_rad_* with ngroups > 1, qk_rad_AddSourceTermsMultiGroup) against the CPU oracle, and the pass
criteria of the reference's multigroup ctests on the GPU.

The multigroup exchange calls pow / exp / log / log10 (group-mean opacities, Planck function at the group edges, the table look-up of the
Planck integral): glibc and the device libm agree to <= 1-2 ulp, not bit for bit, so the comparison uses the tolerance north_star states
(1e-12 relative L1 on every conserved component); the transport part (no libm) is compared bit for bit on its own."""
import os

import numpy as np
import pytest
import torch

from oracle.pyoracle import (LINE_COOLING, LINE_COOLING_MG, MARSHAK_DUST, MARSHAK_DUST_PE, MARSHAK_VAYTET, PIECEWISE_CONSTANT, PPL_FIXED_SLOPE, PPL_FULL_SPECTRUM, PULSE_MG, PULSE_MG_GREY, RADDUST, RADDUST_MG,
                             RADSHOCK_MG, RADTUBE)
from test_multigroup_oracle import (A_RAD, H_PLANCK, K_B, line_cooling_error, marshak_dust_error, marshak_dust_pe_error, pulse_mg_error, raddust_error, radshock_mg_error, tube_table)

pytestmark = pytest.mark.gpu


def seed(so, sg):
    for b in range(so.nboxes):
        sg.state_new_cc_.set_fab(b, so.state(b, 0))
        sg.state_old_cc_.set_fab(b, so.state(b, 1))
    sg._signal_of_state_new = None


def compare(so, sg, tol=1e-12, mom_scale=None, energy_scale=None):
    """energy_scale: a group that only holds its floor (|E_g| << the radiation energy of the problem) is compared on that scale"""
    Uo = so.valid(0)
    Ug = sg.state_new_cc_.valid(0).cpu().numpy()
    assert not np.isnan(Ug).any()
    nc = Uo.shape[0]
    for n in range(nc):
        num = np.abs(Ug[n] - Uo[n]).sum()
        den = np.abs(Uo[n]).sum()
        if den == 0.0:
            assert num == 0.0, n
        elif mom_scale is not None and (n in (1, 2, 3) or (n >= 6 and (n - 6) % 4 != 0)):
            # momenta / radiation fluxes that cancel over the domain: absolute measure on the scale of the matching energy-like quantity
            assert num <= tol * max(den, mom_scale[n]), (n, num, den)
        elif energy_scale is not None and n >= 6 and (n - 6) % 4 == 0:
            assert num <= tol * max(den, energy_scale), (n, num, den)
        else:
            assert num <= tol * den, (n, num / den)
    return Uo, Ug


def flux_scales(Uo, c, cs=1e5, fscale=1e-6):
    """|F| is compared on the scale c E of its group where it (nearly) vanishes; gas momenta on rho * cs (cs: a sound speed of the problem)"""
    s = {1: np.abs(Uo[0]).sum() * cs, 2: np.abs(Uo[0]).sum() * cs, 3: np.abs(Uo[0]).sum() * cs}
    ng = (Uo.shape[0] - 6) // 4
    for g in range(ng):
        for d in (1, 2, 3):
            s[6 + 4 * g + d] = fscale * c * np.abs(Uo[6 + 4 * g]).sum()
    return s


@pytest.mark.parametrize("bnd,unit", [([1e15, 1e16, 1e17, 1e18, 1e19, 1e20], H_PLANCK), ([0.01 * 2.75e7, 3.3 * 2.75e7, 1000 * 2.75e7], K_B),
                                      ([6e10, 6e11, 6e12, 6e13, 6e14], H_PLANCK)])
def test_planck_fractions_on_device_match_oracle(ctx, oracle, bnd, unit):
    from quokka_amd import capi
    from quokka_amd.radhydro_multigroup import planck_fractions
    ng = len(bnd) - 1
    floor = 1e-30
    rt = capi.RadTraits(2.99792458e10, 2.99792458e10, A_RAD, floor, 1, 0, 0.0, 0.0, 0.0, 0, 0)
    rt.set_groups(bnd, unit, 1, [0.0] * (ng + 1), [1.0] * (ng + 1))
    T = np.logspace(1.5, 9.5, 331)
    f, E = planck_fractions(ctx, rt, K_B, T)
    for i, t in enumerate(T):
        fo, Eo = oracle.planck_fractions(bnd, unit, K_B, A_RAD, floor, float(t))
        # log10 of the device and of glibc differ in the last place: the interpolated integral moves by ~1e-16 of ITS value; a group
        # fraction is a difference of two such values
        assert np.allclose(f[i], fo, rtol=1e-12, atol=2e-16), (t, f[i], fo)
        assert np.allclose(E[i], Eo, rtol=1e-12, atol=2e-16 * A_RAD * t ** 4), (t, E[i], Eo)
    assert np.allclose(f.sum(axis=1), 1.0, rtol=0, atol=4e-16)


@pytest.mark.parametrize("model", [PPL_FIXED_SLOPE, PIECEWISE_CONSTANT, PPL_FULL_SPECTRUM])
def test_multigroup_shock_steps_match_oracle(ctx, oracle, model):
    """RadhydroShockMultigroup: 5 groups, hydro + radiation subcycles with beta_order 1 (work and pressure terms), Dirichlet states; 40 coupled
    steps from the discontinuity"""
    from quokka_amd.radhydro_multigroup import RadShockMGConstants as S, radshock_mg_problem
    nx, nsteps = 64, 40
    so = oracle.sim(RADSHOCK_MG, 1, [nx, 1, 1], [0, 0, 0], [S.Lx, 1, 1], [0, 1, 1], max_grid_size=[nx, 1, 1], opacity_model=model)
    sg = radshock_mg_problem(ctx, nx, opacity_model=model)
    assert sg.ncomp_override == so.ncomp == 26
    # the product's own generator: Planck fractions from the device function
    assert np.allclose(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy(), rtol=1e-12, atol=0.0)
    seed(so, sg)
    for it in range(nsteps):
        assert so.step() and sg.step(), it
        assert abs(so.dt - sg.dt_) <= 1e-13 * so.dt, (it, so.dt, sg.dt_)
    Uo = so.valid(0)
    compare(so, sg, mom_scale=flux_scales(Uo, S.c))
    co = so.rad_counters()
    assert co["fail_coupling"] == co["fail_outer"] == 0
    assert sg.rad_counters["solves"] == co["solves"]
    assert abs(sg.rad_counters["newton_iterations"] - co["newton_iterations"]) <= 1e-3 * co["newton_iterations"]


def test_multigroup_shock_meets_the_reference_criterion_on_gpu(ctx):
    from quokka_amd.radhydro_multigroup import radshock_mg_problem
    sg = radshock_mg_problem(ctx, 64)
    assert sg.evolve() and abs(sg.tNew_ - 1.0e-9) < 1e-24
    err = radshock_mg_error(sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, :])
    assert 1e-4 < err < 0.008, err


def test_radiation_tube_steps_match_oracle_and_criterion(ctx, oracle):
    """RadTube: 2 groups, piecewise-constant opacity, ghost cells that follow the interior momentum / flux (qk_dirichlet_face::interior_mask)"""
    from quokka_amd.radhydro_multigroup import RadTubeConstants as S, radtube_problem
    tab = tube_table()
    cols = [tab[:, n] for n in range(4)]
    so = oracle.sim(RADTUBE, 1, [128, 1, 1], [0, 0, 0], [128.0, 1, 1], [0, 1, 1], max_grid_size=[128, 1, 1], table=cols)
    sg = radtube_problem(ctx, cols)
    U0 = sg.state_new_cc_.valid(0).cpu().numpy().copy()
    assert np.allclose(so.valid(0), U0, rtol=1e-12, atol=0.0)
    seed(so, sg)
    for it in range(30):
        assert so.step() and sg.step(), it
    # a static equilibrium: the momenta are the small residual (~3e-4 rho a0) of forces that cancel, the fluxes the diffusion flux
    # ~ c / (3 tau) dE of cells of optical depth 100-200 (7e-6 c E: differences of neighbouring energies, compared on the scale 1e-4 c E)
    compare(so, sg, mom_scale=flux_scales(so.valid(0), 2.99792458e10, cs=S.a0, fscale=1e-4))
    # ghost cells: the functor's values, component by component
    sg.fillBoundaryConditions(sg.state_new_cc_)
    so.fill_ghosts(0, so.time)
    Go, Gg = so.state(0, 0)[:, 0, 0, :], sg.state_new_cc_.fabs[0].cpu().numpy()[:, 0, 0, :]
    scl = flux_scales(so.valid(0), 2.99792458e10, cs=S.a0, fscale=1e-4)
    for n in range(14):
        tol = 1e-11 * max(np.abs(Go[n]).max(), scl.get(n, 0.0) / 128)  # (single cells: the L1 norms above are within 1e-12)
        for sl in (slice(0, 4), slice(-4, None)):
            assert np.all(np.abs(Go[n, sl] - Gg[n, sl]) <= tol), (n, Go[n, sl], Gg[n, sl])
    # the ghost momentum / normal fluxes are the first valid cell's, the total energy carries that cell's kinetic energy
    assert np.all(Gg[1, :4] == Gg[1, 4]) and np.all(Gg[7, :4] == Gg[7, 4]) and np.all(Gg[11, -4:] == Gg[11, -5])
    assert np.all(Gg[4, :4] == Gg[5, :4] + 0.5 * (Gg[1, 4] * Gg[1, 4]) / S.rho0)
    assert sg.evolve()
    U = sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, :]
    T0 = np.power((U0[6, 0, 0] + U0[10, 0, 0]) / A_RAD, 0.25)
    T = np.power((U[6] + U[10]) / A_RAD, 0.25)
    err = float(np.abs(T - T0).sum() / np.abs(T0).sum())
    assert err < 0.003, err  # test_radiation_tube.cpp:366-384


def test_advected_multigroup_pulse_steps_match_oracle_and_criterion(ctx, oracle):
    """RadhydroPulseMGconst: the grey run and the advected 4-group run, 100 steps each (the file's max_timesteps); periodic"""
    from quokka_amd.radhydro_multigroup import PulseMGConstants as S, pulse_mg_problem
    out = []
    for problem, mgflag in ((PULSE_MG_GREY, False), (PULSE_MG, True)):
        so = oracle.sim(problem, 1, [64, 1, 1], [-512.0, 0, 0], [512.0, 1, 1], [1, 1, 1], max_grid_size=[64, 1, 1])
        sg = pulse_mg_problem(ctx, mgflag)
        assert np.allclose(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy(), rtol=1e-12, atol=0.0)
        seed(so, sg)
        assert so.evolve() and sg.evolve() and so.istep == sg.istep == 100
        compare(so, sg, tol=1e-11 if mgflag else 1e-12, mom_scale=flux_scales(so.valid(0), S.c))
        out.append((sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, :], sg.tNew_))
    err = pulse_mg_error(out[0][0], out[1][0], out[1][1])
    assert err < 0.006, err


@pytest.mark.parametrize("model", [PPL_FULL_SPECTRUM, PPL_FIXED_SLOPE, PIECEWISE_CONSTANT])
def test_marshak_vaytet_steps_match_oracle(ctx, oracle, model):
    """RadMarshakVaytet: radiation only, kappa ~ nu^-2 (exponent -2: the PPL group means, the delta-B terms and the diffusion flux-mean opacity all
    differ from the grey case), the full-spectrum model re-fits the spectral slopes every Newton iteration"""
    from quokka_amd.radhydro_multigroup import marshak_vaytet_problem
    so = oracle.sim(MARSHAK_VAYTET, 1, [64, 1, 1], [0.0, 0, 0], [20.0, 1, 1], [0, 1, 1], max_grid_size=[64, 1, 1], opacity_model=model)
    sg = marshak_vaytet_problem(ctx, 64, opacity_model=model)
    assert np.allclose(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy(), rtol=1e-12, atol=0.0)
    seed(so, sg)
    for it in range(400):
        assert so.step() and sg.step(), it
    compare(so, sg, tol=1e-11, mom_scale=flux_scales(so.valid(0), 2.99792458e10))
    co = so.rad_counters()
    assert sg.rad_counters["solves"] == co["solves"] and co["fail_coupling"] == co["fail_outer"] == 0


def test_marshak_vaytet_runs_to_the_end_on_gpu(ctx):
    """the reference's ctest criterion: t_end reached without a Newton-Raphson failure (the driver raises on one)"""
    from quokka_amd.radhydro_multigroup import marshak_vaytet_problem
    sg = marshak_vaytet_problem(ctx, 64)
    assert sg.evolve() and abs(sg.tNew_ - 1.36e-7) < 1e-20 and sg.istep > 30000
    U = sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, :]
    Trad = np.power(sum(U[6 + 4 * g] for g in range(4)) / A_RAD, 0.25)
    assert 900.0 < Trad[0] < 1000.0 and 300.0 < Trad[-1] < 302.0 and np.all(np.diff(Trad) < 0)
    assert sg.rad_counters["max_newton_iterations"] < 30


def test_multigroup_transport_in_3d_is_bit_exact(ctx, oracle):
    """The 3-D flux kernels (LDS slab kernel along x, marching kernels along y / z) with the group index folded into the grid, through the driver:
    RadhydroShockMultigroup on the deck's 64 x 4 x 4 cells in two boxes, a rippled state with structure along y and z, radiation transport only
    (PredictStep + AddFluxesRK2, no source term: no libm) — bit for bit.  This geometry has no seams: the slab of 40 x 4 positions is one X workgroup's,
    every Y and Z pencil one strip's — the seams of the kernels and the whole-cell state repair are pinned in tests/test_rad_transport_cells_gpu.py."""
    from quokka_amd.radhydro_multigroup import RadShockMGConstants as S, radshock_mg_problem
    n = [64, 4, 4]
    so = oracle.sim(RADSHOCK_MG, 3, n, [0, 0, 0], [S.Lx, 0.001575, 1.0], [0, 1, 1], max_grid_size=[32, 4, 4])
    ng = 5
    sg = radshock_mg_problem(ctx, 64, three_d=True, max_grid_size=[32, 4, 4])
    geom = sg.geom
    assert so.nboxes == sg.lev.nboxes == 2
    rng = np.random.default_rng(11)
    for order in (3, 2, 1):
        for b in range(so.nboxes):
            U = so.state(b, 0).copy()
            shp = U.shape[1:]
            for g in range(ng):
                E = U[6 + 4 * g] * (1.0 + 0.3 * rng.random(shp))
                U[6 + 4 * g] = E
                # reduced fluxes up to ~0.9 in random directions; a few cells beyond the causal limit and a few negative energies so that
                # the first-order fallback of the Riemann solver and the state repair both run
                f = 0.9 * rng.random(shp)
                d = rng.normal(size=(3,) + shp)
                d /= np.sqrt((d * d).sum(axis=0))
                bad = rng.random(shp) < 0.01
                f = np.where(bad, 1.3, f)
                for a in range(3):
                    U[6 + 4 * g + 1 + a] = f * d[a] * S.c * E
                U[6 + 4 * g] = np.where(rng.random(shp) < 0.005, -E, U[6 + 4 * g])
            so.set_state(U, b, 0)
            so.set_state(U, b, 1)
            sg.state_new_cc_.set_fab(b, U)
            sg.state_old_cc_.set_fab(b, U)
        so.set_rad_reconstruction_order(order)
        sg.radiationReconstructionOrder_ = order
        dt = 0.3 * min(geom.dx) / S.chat
        so.rad_transport_only(dt)
        sg.advanceRadiationForwardEuler(dt)
        sg.advanceRadiationMidpointRK2(dt)
        for b in range(so.nboxes):
            a, g_ = so.valid(b), sg.state_new_cc_.valid(b).cpu().numpy()
            assert np.array_equal(a[6:], g_[6:]), (order, b, np.abs(a[6:] - g_[6:]).max())


def test_dust_model_steps_match_oracle_and_criterion(ctx, oracle):
    """RadDust: the DUST instantiation of the single-group exchange kernel (no libm beyond sqrt: bit for bit), and the reference's criterion"""
    from quokka_amd.radhydro_multigroup import raddust_problem
    so = oracle.sim(RADDUST, 1, [8, 1, 1], [0, 0, 0], [1.0, 1, 1], [1, 1, 1], max_grid_size=[8, 1, 1])
    sg = raddust_problem(ctx)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    ts, us = [], []
    for it in range(1000):
        assert so.step() and sg.step(), it
        assert so.dt == sg.dt_
        ts.append(sg.tNew_)
        us.append(sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, 0])
        if it in (0, 9, 99, 999):
            assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy()), it
    co = so.rad_counters()
    assert sg.rad_counters["solves"] == co["solves"] and sg.rad_counters["newton_iterations"] == co["newton_iterations"]
    assert co["fail_coupling"] == co["fail_dust"] == co["fail_outer"] == 0
    err = raddust_error(np.array(ts), np.array(us))
    assert err < 0.0008, err


def test_multigroup_dust_model_coupled_branch_matches_oracle_and_criterion(ctx, oracle):
    """RadDustMG: the DUST instantiation of the multigroup exchange kernel on the coupled branch of radiation_dust_system.hpp (gas, dust and the
    four groups in one Newton-Raphson system; the Planck fractions call exp / the table: tolerance, not bits)"""
    from quokka_amd.radhydro_multigroup import raddust_problem
    so = oracle.sim(RADDUST_MG, 1, [8, 1, 1], [0, 0, 0], [1.0, 1, 1], [1, 1, 1], max_grid_size=[8, 1, 1])
    sg = raddust_problem(ctx, multigroup=True)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    ts, us = [], []
    for it in range(1000):
        assert so.step() and sg.step(), it
        assert so.dt == sg.dt_
        ts.append(sg.tNew_)
        us.append(sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, 0])
        if it in (0, 9, 99, 999):
            compare(so, sg, tol=1e-11, mom_scale=flux_scales(so.valid(0), 1.0e8, cs=1.0, fscale=1e-6))
    co = so.rad_counters()
    assert sg.rad_counters["solves"] == co["solves"] and abs(sg.rad_counters["newton_iterations"] - co["newton_iterations"]) <= 0.01 * co["newton_iterations"]  # (8 identical cells: a cell one iteration apart near the residual tolerance counts 8 times)
    assert sg.rad_counters["decoupled"] == co["decoupled"] == 0
    err = raddust_error(np.array(ts), np.array(us), ngroups=4)
    assert err < 0.0008, err


def test_multigroup_dust_model_decoupled_branch_matches_oracle_and_criterion(ctx, oracle):
    """RadMarshakDust: two groups, every solve on the decoupled branch (dust temperature and the groups iterated with the gas-dust exchange rate
    frozen, the gas energy updated afterwards); the partial boundary functor (gas state everywhere, radiation state beyond the lower face only)
    through qk_dirichlet_face::interior_mask"""
    from quokka_amd.radhydro_multigroup import marshak_dust_problem
    so = oracle.sim(MARSHAK_DUST, 1, [256, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[256, 1, 1])
    sg = marshak_dust_problem(ctx, 256)
    assert np.allclose(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy(), rtol=1e-13, atol=0.0)
    seed(so, sg)
    for it in range(60):
        assert so.step() and sg.step(), it
        assert so.dt == sg.dt_
    compare(so, sg, tol=1e-11, mom_scale=flux_scales(so.valid(0), 1.0, cs=1.0, fscale=1e-6))
    # ghost cells: gas state and (lower face) the streaming radiation state from the functor, the radiation state of the upper face from inside
    sg.fillBoundaryConditions(sg.state_new_cc_)
    so.fill_ghosts(0, so.time)
    Go, Gg = so.state(0, 0)[:, 0, 0, :], sg.state_new_cc_.fabs[0].cpu().numpy()[:, 0, 0, :]
    assert np.array_equal(Go[:6, :4], Gg[:6, :4]) and np.array_equal(Go[:6, -4:], Gg[:6, -4:]) and np.array_equal(Go[6:, :4], Gg[6:, :4])
    assert np.all(Gg[6:, -4:] == Gg[6:, -5:-4]) and np.allclose(Go[6:, -4:], Gg[6:, -4:], rtol=1e-9, atol=1e-30)
    assert so.evolve() and sg.evolve() and so.istep == sg.istep
    compare(so, sg, tol=1e-10, mom_scale=flux_scales(so.valid(0), 1.0, cs=1.0, fscale=1e-6))
    co = so.rad_counters()
    assert sg.rad_counters["solves"] == co["solves"] == co["decoupled"]
    assert sg.rad_counters["decoupled"] == co["decoupled"]
    err = marshak_dust_error(sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, :], sg.tNew_)
    assert err < 0.01, err


@pytest.mark.parametrize("multigroup,dust_coeff", [(False, 1e-20), (True, 1e-20), (True, 1e20)])
def test_line_cooling_problems_match_oracle_and_criterion(ctx, oracle, multigroup, dust_coeff):
    """RadLineCooling (one group: the cooling / cosmic-ray terms of the DUST instantiation of the single-group kernel) and RadLineCoolingMG with
    both decks (the decoupled and the coupled branch of the multigroup solve with photoelectric heating); kappa = 0: no libm beyond sqrt and the
    Planck fractions of a state that does not emit"""
    from quokka_amd.radhydro_multigroup import line_cooling_problem
    so = oracle.sim(LINE_COOLING_MG if multigroup else LINE_COOLING, 1, [8, 1, 1], [0, 0, 0], [64.0, 1, 1], [1, 1, 1], max_grid_size=[8, 1, 1], dust_coeff=dust_coeff)
    sg = line_cooling_problem(ctx, multigroup, dust_coeff)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    ts, us = [], []
    for it in range(1000):
        assert so.step() and sg.step(), it
        assert so.dt == sg.dt_
        ts.append(sg.tNew_)
        us.append(sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, 0])
        if it in (0, 9, 99, 999):
            compare(so, sg, tol=1e-12, mom_scale=flux_scales(so.valid(0), 1.0, cs=1.0, fscale=1e-6))
    co = so.rad_counters()
    assert sg.rad_counters["solves"] == co["solves"] and sg.rad_counters["decoupled"] == co["decoupled"]
    assert sg.rad_counters["newton_iterations"] == co["newton_iterations"]
    err = line_cooling_error(np.array(ts), np.array(us), 0.05 if multigroup else 0.03)
    assert err < 0.0005, err


@pytest.mark.parametrize("dust_coeff", [1e20, 1e-20])
def test_photoelectric_heating_front_matches_oracle_and_criterion(ctx, oracle, dust_coeff):
    """RadMarshakDustPE with its two decks: the Jacobian with the FUV column and SolveLinearEqsWithLastColumn (coupled), the scalar gas-energy solve
    with the photoelectric term (decoupled)"""
    from quokka_amd.radhydro_multigroup import marshak_dust_pe_problem
    so = oracle.sim(MARSHAK_DUST_PE, 1, [256, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[256, 1, 1], dust_coeff=dust_coeff)
    sg = marshak_dust_pe_problem(ctx, dust_coeff)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    assert so.evolve() and sg.evolve() and so.istep == sg.istep
    # (the IR group holds its floor, 1e-6 of the FUV energy density: compared on the scale of the FUV group)
    ms = flux_scales(so.valid(0), 1.0, cs=1.0, fscale=1e-6)
    ms[7] = ms[8] = ms[9] = 1.0 * np.abs(so.valid(0)[10]).sum()  # c * sum E_FUV: the IR group is rounding noise around its floor
    compare(so, sg, tol=1e-11, mom_scale=ms, energy_scale=np.abs(so.valid(0)[10]).sum())
    co = so.rad_counters()
    assert sg.rad_counters["solves"] == co["solves"] and sg.rad_counters["decoupled"] == co["decoupled"]
    err = marshak_dust_pe_error(sg.state_new_cc_.valid(0).cpu().numpy()[:, 0, 0, :], sg.tNew_)
    assert err < 0.01, err


def test_multigroup_transport_with_the_wavespeed_correction_matches_oracle(ctx, oracle):
    """use_wavespeed_correction_ with several photon groups (reference src/radiation/radiation_system.hpp:863-868: DefineOpacityExponentsAndLowerValues +
    ComputeBinCenterOpacity either side of the face, one optical depth per group): RadhydroShockMultigroup's five groups on 64 x 4 x 4 cells in two
    boxes, a rippled radiation state over a gas density roughened across six decades (optical depths per cell on both sides of 1), transport only.
    The bin-centre opacity is a std::pow: 1e-12 relative L1 per radiation component (bit for bit where the exponents vanish), and the correction
    does change the fluxes."""
    from quokka_amd.radhydro_multigroup import RadShockMGConstants as S, radshock_mg_problem
    n = [64, 4, 4]
    ng = 5
    results = []
    for corr in (True, False):
        so = oracle.sim(RADSHOCK_MG, 3, n, [0, 0, 0], [S.Lx, 0.001575, 1.0], [0, 1, 1], max_grid_size=[32, 4, 4])
        sg = radshock_mg_problem(ctx, 64, three_d=True, max_grid_size=[32, 4, 4])
        rng = np.random.default_rng(21)
        for b in range(so.nboxes):
            U = so.state(b, 0).copy()
            shp = U.shape[1:]
            U[0:6] *= 10.0 ** rng.uniform(-3.0, 3.0, shp)
            for g in range(ng):
                E = U[6 + 4 * g] * (1.0 + 0.3 * rng.random(shp))
                U[6 + 4 * g] = E
                f = 0.8 * rng.random(shp)
                d = rng.normal(size=(3,) + shp)
                d /= np.sqrt((d * d).sum(axis=0))
                for a in range(3):
                    U[6 + 4 * g + 1 + a] = f * d[a] * S.c * E
            so.set_state(U, b, 0)
            so.set_state(U, b, 1)
            sg.state_new_cc_.set_fab(b, U)
            sg.state_old_cc_.set_fab(b, U)
        so.set_wavespeed_correction(corr)
        sg.use_wavespeed_correction_ = corr
        dt = 0.3 * min(sg.geom.dx) / S.chat
        so.rad_transport_only(dt)
        sg.advanceRadiationForwardEuler(dt)
        sg.advanceRadiationMidpointRK2(dt)
        out = []
        for b in range(so.nboxes):
            a, g_ = so.valid(b), sg.state_new_cc_.valid(b).cpu().numpy()
            for c in range(6, 6 + 4 * ng):
                den = np.abs(a[c]).sum()
                assert np.abs(a[c] - g_[c]).sum() <= 1e-12 * max(den, 1e-300), (corr, b, c)
            out.append(g_)
        results.append(out)
    assert any(not np.array_equal(x[6], y[6]) for x, y in zip(*results))
