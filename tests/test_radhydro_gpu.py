"""GPU parity of the coupled radiation-hydrodynamics step (BASELINE config 4, RadhydroShell) against the CPU oracle.

The radiation update contains pow(T, 4) / pow(T, 3) (std::pow in the reference): glibc and the device libm agree to
<= 1 ulp, not bit-for-bit, so the default build is compared with the tolerance north_star states (1e-12 relative L1 on
every conserved component).  With pow_mode = 1 (repeated multiplication on both sides) everything else is bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle.pyoracle import SHELL
from quokka_amd.radhydro import ShellConstants, shell_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def table():
    tab = np.loadtxt(os.path.join(HERE, "golden", "dust_shell_initial_conditions.txt"), skiprows=1)
    return tab[:, 0], tab[:, 2], tab[:, 3]


def make_pair(ctx, oracle, N, mgs, pow_mode):
    L = ShellConstants.L_box
    so = oracle.sim(SHELL, 3, [N] * 3, [0, 0, 0], [L] * 3, [1, 1, 1], max_grid_size=[mgs] * 3, table=table(), rad_pow_mode=pow_mode)
    sg = shell_problem(ctx, N, table(), max_grid_size=mgs, pow_mode=pow_mode)
    return so, sg


def seed_from_oracle(so, sg):
    """identical inputs: the oracle's initial state and source array (the product's own generators are checked separately)"""
    for b in range(so.nboxes):
        sg.state_new_cc_.set_fab(b, so.state(b, 0))
        sg.state_old_cc_.set_fab(b, so.state(b, 1))
        sg.radEnergySource.fabs[b][0].copy_(torch.from_numpy(so.rad_source(b, 0.0)))
    sg._source_set = True


def gather(sim_boxes, valid_list, N, nc=10):
    U = np.zeros((nc, N, N, N))
    for (lo, hi), v in zip(sim_boxes, valid_list):
        U[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = v
    return U


def rel_l1(a, b):
    return [np.abs(a[n] - b[n]).sum() / max(np.abs(b[n]).sum(), 1e-300) for n in range(a.shape[0])]


def test_shell_generators_match_oracle(ctx, oracle):
    """ICs (table interpolation, Gaussian shell) and the point source: same formulas, libm exp/pow differ by <= a few ulp."""
    so, sg = make_pair(ctx, oracle, 16, 8, 0)
    for b in range(so.nboxes):
        a, g = so.valid(b), sg.state_new_cc_.valid(b).cpu().numpy()
        assert np.allclose(a, g, rtol=1e-13, atol=0.0)
        sg._fill_source(0.0)
        assert np.allclose(so.rad_source(b, 0.0), sg.radEnergySource.fabs[b][0].cpu().numpy(), rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("N,mgs,rad_order", [pytest.param(16, 16, 2, id="16-2"), pytest.param(16, 8, 2, id="8-2"), pytest.param(16, 8, 3, id="8-3"),
                                             pytest.param(16, 16, 1, id="16-1"), (20, 20, 3), (20, 20, 2)])  # (the 16^3 cases keep their ids)
def test_radhydro_steps_bit_exact_with_shared_pow(ctx, oracle, N, mgs, rad_order):
    """(rad_order: the problem uses PLM = 2; 3 and 1 exercise the PPM and donor-cell variants of the three flux kernels in 3-D.
    The single 20^3 box: a Y strip of 16 cells and a tail of 4, marches of 8 + 8 + 5 faces, an X slab of 560 positions in three workgroups)"""
    nsteps = 3
    so, sg = make_pair(ctx, oracle, N, mgs, 1)
    so.set_rad_reconstruction_order(rad_order)
    sg.radiationReconstructionOrder_ = rad_order
    seed_from_oracle(so, sg)
    for it in range(nsteps):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    Uo = gather([so.box(b) for b in range(so.nboxes)], [so.valid(b) for b in range(so.nboxes)], N)
    Ug = gather(sg.my_boxes, sg.gather_valid_local(), N)
    assert not np.isnan(Ug).any()
    assert np.array_equal(Uo, Ug), f"rel L1 per component {rel_l1(Ug, Uo)}"
    co = so.rad_counters()
    assert co["fail_coupling"] == co["fail_outer"] == 0
    assert sg.rad_counters["solves"] == co["solves"]
    assert sg.rad_counters["newton_iterations"] == co["newton_iterations"]
    assert sg.rad_counters["max_newton_iterations"] == co["max_newton_iterations"]
    assert sg.radiationCellUpdates_ == co["rad_cell_updates"] and co["rad_cell_updates"] == 10 * nsteps * N ** 3


def test_radhydro_steps_within_1e12_with_libm_pow(ctx, oracle):
    """the shipped configuration (std::pow as the reference): <= 1e-12 relative L1 on every conserved component"""
    N, nsteps = 16, 3
    so, sg = make_pair(ctx, oracle, N, 8, 0)
    seed_from_oracle(so, sg)
    for _ in range(nsteps):
        assert so.step() and sg.step()
    Uo = gather([so.box(b) for b in range(so.nboxes)], [so.valid(b) for b in range(so.nboxes)], N)
    Ug = gather(sg.my_boxes, sg.gather_valid_local(), N)
    err = rel_l1(Ug, Uo)
    # momenta are ~1e-15 of their scale after 3 steps (sum of |p| over a symmetric shell): compare them in absolute terms
    scale = np.abs(Uo[0]).sum() * ShellConstants.a0
    for n in (0, 4, 5, 6, 7, 8, 9):
        assert err[n] <= 1e-12, (n, err)
    for n in (1, 2, 3):
        assert np.abs(Ug[n] - Uo[n]).sum() <= 1e-12 * scale, (n, err)


def test_radiative_shock_steps_match_oracle(ctx, oracle):
    """RadhydroShockCGS (1-D, Dirichlet states beyond both faces, kappa = k0 / rho, Eddington approximation — the second members of
    the closed opacity / closure sets): 150 coupled steps, bit for bit with the shared T^4 evaluation"""
    from oracle.pyoracle import RADSHOCK
    from quokka_amd.radhydro import radshock_problem
    nx, nsteps = 512, 150
    so = oracle.sim(RADSHOCK, 1, [nx, 1, 1], [0, 0, 0], [0.01575, 1, 1], [0, 1, 1], max_grid_size=[nx, 1, 1], rad_pow_mode=1)
    sg = radshock_problem(ctx, nx, pow_mode=1)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())  # the generators agree exactly (no libm calls)
    for it in range(nsteps):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    Uo, Ug = so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(Uo, Ug), f"rel L1 per component {rel_l1(Ug, Uo)}"
    co = so.rad_counters()
    assert sg.rad_counters["solves"] == co["solves"] and sg.rad_counters["newton_iterations"] == co["newton_iterations"]
    assert co["fail_coupling"] == co["fail_outer"] == 0


def test_streaming_front_matches_oracle_and_the_reference_criterion(ctx, oracle):
    """RadStreaming, the full run (667 steps; radiation only: the hydro variables are copied, dt from c_hat alone): every bit of the
    final state equals the oracle's, and the reference's criterion (relative L1 error < 0.01 against the step function) holds"""
    from oracle.pyoracle import STREAMING
    from quokka_amd.radhydro import streaming_problem
    so = oracle.sim(STREAMING, 1, [1000, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[1000, 1, 1], rad_pow_mode=1)
    sg = streaming_problem(ctx, 1000, pow_mode=1)
    assert so.evolve() and sg.evolve()
    assert (so.istep, so.time) == (sg.istep, sg.tNew_) == (667, 1.0)
    Uo, Ug = so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(Uo, Ug), f"rel L1 per component {rel_l1(Ug, Uo)}"
    x = (np.arange(1000) + 0.5) / 1000
    exact = np.where(x <= 0.2, 1.0, 0.0)
    assert np.abs(Ug[6, 0, 0] - exact).sum() / exact.sum() < 0.01


def test_streaming_front_along_y_in_a_2d_build_matches_oracle_and_criterion(ctx, oracle):
    """RadStreamingY: the radiation operators on an AMREX_SPACEDIM == 2 level (LDS slab kernel along x, marching kernel along y on the single
    plane; PredictStep / AddFluxesRK2 with the x and y terms; Dirichlet faces in y) — two boxes, bit for bit, and the reference's criterion"""
    from oracle.pyoracle import STREAMING_Y
    from quokka_amd.radhydro import streaming_y_problem
    so = oracle.sim(STREAMING_Y, 2, [8, 100, 1], [0, 0, 0], [1.0, 1.0, 1.0], [1, 0, 1], max_grid_size=[8, 50, 1], rad_pow_mode=1)
    sg = streaming_y_problem(ctx, (8, 100), pow_mode=1, max_grid_size=[8, 50, 1])
    assert so.nboxes == sg.lev.nboxes == 2
    assert so.evolve() and sg.evolve()
    assert (so.istep, so.time) == (sg.istep, sg.tNew_)
    for b in range(so.nboxes):
        Uo, Ug = so.valid(b), sg.state_new_cc_.valid(b).cpu().numpy()
        assert np.array_equal(Uo, Ug), (b, rel_l1(Ug, Uo))
    U = np.concatenate([sg.state_new_cc_.valid(b).cpu().numpy() for b in range(sg.lev.nboxes)], axis=2) if sg.lev.nboxes > 1 else sg.state_new_cc_.valid(0).cpu().numpy()
    y = (np.arange(100) + 0.5) / 100
    exact = np.where(y <= 0.2, 1.0, 0.0)
    assert np.abs(U[6, 0, :, 0] - exact).sum() / exact.sum() < 0.05
    assert np.all(U[7] == 0.0) and U[8].max() > 0.5


def test_shell_accelerates_as_the_thin_shell_solution_predicts(ctx):
    """The physics check the reference has for RadhydroShell (extern/dust_shell/analyze.py:50-57 plots it; no tolerance there): the
    density-weighted mean speed of the shell against the thin-shell solution M(R) = sqrt(2) M0 sqrt(1 - 1/R).  At 128^3 the shell
    follows it from below (finite thickness, tau ~ 7): 0.85 +- 0.02 of the analytic speed up to T = 0.125 (profiles/tools/
    shell_velocity.py); checked here at T = 0.025 (230 steps x 10 radiation substeps)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "profiles", "tools"))
    import shell_velocity
    (T, mach, analytic), = shell_velocity.run(128, 1, t_end=0.025)
    assert abs(T - 0.025) < 1e-12
    assert 0.82 < mach / analytic < 0.92, (mach, analytic)


def test_su_olson_and_matter_coupling_match_oracle(ctx, oracle):
    """The T^4 member of the EOS hook set (`eos_temperature_model = 1`), a time-dependent radiation source, reflecting walls and a
    constant time step through the C-ABI: RadSuOlson for 400 steps and RadMatterCoupling for 3000 steps, bit for bit (shared T^4
    evaluation); the reference's criteria are evaluated on the oracle's full runs in tests/test_oracle_known_answers.py."""
    from oracle.pyoracle import COUPLING, SUOLSON
    from quokka_amd.radhydro import matter_coupling_problem, suolson_problem
    so = oracle.sim(SUOLSON, 1, [1500, 1, 1], [0, 0, 0], [30.0, 1, 1], [0, 0, 0], max_grid_size=[1500, 1, 1], rad_pow_mode=1)
    sg = suolson_problem(ctx, 1500, pow_mode=1)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    for it in range(400):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    assert so.time > 1.5  # well into the regime where the wave has left the source region

    so = oracle.sim(COUPLING, 1, [4, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 0, 0], max_grid_size=[4, 1, 1], rad_pow_mode=1)
    sg = matter_coupling_problem(ctx, 4, pow_mode=1)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    for it in range(3000):
        assert so.step() and sg.step()
    assert sg.dt_ == 1.0e-8 and np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    assert sg.state_new_cc_.valid(0)[4, 0, 0, 1].item() > 1.0e4  # the gas has heated by orders of magnitude

    # RadMatterCouplingRSLA: the same with c_hat = 0.1 c
    so = oracle.sim(COUPLING, 1, [4, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 0, 0], max_grid_size=[4, 1, 1], rad_pow_mode=1, c_hat_factor=0.1)
    sr = matter_coupling_problem(ctx, 4, pow_mode=1, c_hat_factor=0.1)
    for it in range(3000):
        assert so.step() and sr.step()
    U = sr.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(so.valid(0), U) and not np.array_equal(U, sg.state_new_cc_.valid(0).cpu().numpy())


def test_uniform_advecting_beta_order_2_matches_oracle(ctx, oracle):
    """RadhydroUniformAdvecting through the C-ABI: the whole run (125 steps) of the reference problem bit for bit and within its
    1e-10 criterion.  The uniform state sits at the fixed point of the O(beta^2) terms, so the same terms are also compared on a
    state with gradients: the radiative shock with RadSystem_Traits::beta_order overridden to 2 and to 3, 120 steps each."""
    from oracle.pyoracle import ADVECTING, RADSHOCK
    from quokka_amd.radhydro import radshock_problem, uniform_advecting_problem
    so = oracle.sim(ADVECTING, 1, [64, 1, 1], [0, 0, 0], [64.0, 1, 1], [1, 1, 1], max_grid_size=[64, 1, 1], rad_pow_mode=1)
    sg = uniform_advecting_problem(ctx, 64, pow_mode=1)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    assert so.evolve() and sg.evolve()
    assert so.istep == sg.istep == 125 and so.time == sg.tNew_
    U = sg.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(so.valid(0), U)
    T = (5.0 / 3.0 - 1.0) * U[5, 0, 0] / U[0, 0, 0]
    assert float(np.abs(T - 1.0).sum() / T.size) < 1.0e-10

    ref = None
    for beta_order in (1, 2, 3):
        so = oracle.sim(RADSHOCK, 1, [256, 1, 1], [0, 0, 0], [0.01575, 1, 1], [0, 1, 1], max_grid_size=[256, 1, 1], rad_pow_mode=1,
                        beta_order=beta_order)
        sg = radshock_problem(ctx, 256, pow_mode=1, beta_order=beta_order)
        for it in range(120):
            assert so.step() and sg.step()
            assert so.dt == sg.dt_, (beta_order, it, so.dt, sg.dt_)
        U = sg.state_new_cc_.valid(0).cpu().numpy()
        assert np.array_equal(so.valid(0), U), beta_order
        if ref is None:
            ref = U
        else:
            assert not np.array_equal(ref, U)  # the higher-order terms did act


def test_marshak_boundary_condition_matches_oracle(ctx, oracle):
    """RadMarshak through the C-ABI: the Marshak member of the closed boundary set (`qk_dirichlet_face::marshak`: the ghost flux follows
    the first valid cell), radiation only, T^4 material — 1500 steps (the dt ramp and ~1.3 time units of the wave) bit for bit."""
    from oracle.pyoracle import MARSHAK
    from quokka_amd.radhydro import marshak_problem
    so = oracle.sim(MARSHAK, 1, [80, 1, 1], [0, 0, 0], [20.0, 1, 1], [0, 1, 1], max_grid_size=[80, 1, 1], rad_pow_mode=1)
    sg = marshak_problem(ctx, 80, pow_mode=1)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    for it in range(1500):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    U = sg.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(so.valid(0), U)
    assert so.time > 1.0 and U[6, 0, 0, 0] > 0.3 and U[6, 0, 0, -1] < 2e-8  # the wave has entered; the far side is still cold


def test_marshak_face_is_validated(ctx):
    """the library refuses a Marshak description on an upper face or with bad component indices"""
    from quokka_amd.radhydro import RAD0, RadhydroSimulation
    from quokka_amd.simulation import Geometry
    from quokka_amd import capi
    geom = Geometry(1, [16], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 1, 1])
    bcs = [([capi.BC_EXT_DIR, 0, 0], [capi.BC_EXT_DIR, 0, 0]) for _ in range(10)]
    tr = capi.traits(5.0 / 3.0, True, 1, mean_molecular_weight=1.0, boltzmann_constant=1.0)
    rt = capi.RadTraits(1.0, 1.0, 1.0, 0.0, 0, 0, 1.0, 1.0, 1.0, 0, 0)
    for face, spec in (((0, 1), (RAD0, RAD0 + 1, 1.0)), ((0, 0), (RAD0, RAD0, 1.0)), ((0, 0), (RAD0, 12, 1.0)), ((0, 0), (RAD0, RAD0 + 1, 0.0))):
        sim = RadhydroSimulation(ctx, geom, tr, rt, bcs, [16, 1, 1], use_fused=False, dirichlet={face: {"values": [1.0] * 10, "marshak": spec}})
        with pytest.raises(capi.QkError):
            sim.set_initial_conditions(lambda i, j, k: np.ones((10,) + i.shape))
            sim.fillBoundaryConditions(sim.state_new_cc_)


def test_radiation_driven_isothermal_wind_matches_oracle(ctx, oracle):
    """RadForce through the C-ABI: isothermal EOS (`gamma = 1`, `cs_isothermal`) in the reference-shaped hydro operators and in the
    radiation source update (no energy exchange, radiation force only), inflow face + extrapolation — 1200 steps bit for bit, then
    the reference's criterion on the GPU's own full run."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_oracle_known_answers import radforce_error
    from oracle.pyoracle import RADFORCE
    from quokka_amd.radhydro import radforce_problem
    so = oracle.sim(RADFORCE, 1, [128, 1, 1], [0, 0, 0], [1.0263747986171498e16, 1, 1], [0, 1, 1], max_grid_size=[128, 1, 1], rad_pow_mode=1)
    sg = radforce_problem(ctx, 128, pow_mode=1)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    for it in range(1200):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    assert sg.evolve() and sg.istep == 9520
    err = radforce_error(sg.state_new_cc_.valid(0).cpu().numpy())
    assert 1e-5 < err < 0.002, err


def test_temperature_dependent_opacity_matches_oracle(ctx, oracle):
    """RadMarshakAsymptotic through the C-ABI: `opacity_model = 2` (kappa = k0 (T / T_ref)^p / rho, here p = -3; its own instantiation
    of the source kernel), Eddington approximation and the Marshak face together — 2500 steps bit for bit (pow_mode 1: the power
    is a product on both sides), with Newton iterations beyond the first (the opacity changes inside the solve)."""
    from oracle.pyoracle import MARSHAK_ASYMPTOTIC
    from quokka_amd.radhydro import marshak_asymptotic_problem
    so = oracle.sim(MARSHAK_ASYMPTOTIC, 1, [60, 1, 1], [0, 0, 0], [0.66, 1, 1], [0, 1, 1], max_grid_size=[60, 1, 1], rad_pow_mode=1)
    sg = marshak_asymptotic_problem(ctx, 60, pow_mode=1)
    assert np.array_equal(so.valid(0), sg.state_new_cc_.valid(0).cpu().numpy())
    for it in range(2500):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    U = sg.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(so.valid(0), U)
    assert so.rad_counters()["max_newton_iterations"] >= 3
    assert U[4, 0, 0, 0] > 100 * U[4, 0, 0, -1]  # the first cell has been heated

    # pow_mode 0 (the library's pow, as the reference's std::pow): same physics to rounding
    sp = marshak_asymptotic_problem(ctx, 60, pow_mode=0)
    for it in range(2500):
        assert sp.step()
    V = sp.state_new_cc_.valid(0).cpu().numpy()
    assert np.allclose(V, U, rtol=1e-9, atol=0)


def test_floored_power_law_opacity_matches_oracle(ctx, oracle):
    """RadPulse through the C-ABI: `opacity_model = 2` with exponent +3 and floor 1 (cells on both sides of the floor), c_hat = c / 10,
    starting from the oracle's initial state — 3000 steps bit for bit; and from the Python evaluation of the Gaussian to 1e-10."""
    from oracle.pyoracle import RADPULSE
    from quokka_amd.radhydro import radpulse_problem
    so = oracle.sim(RADPULSE, 1, [32, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[32, 1, 1], rad_pow_mode=1)
    U0 = so.valid(0).copy()
    T0 = U0[5, 0, 0] / U0[0, 0, 0]  # k_B = 2/3, mu = 1, gamma = 5/3: T = E_int / rho
    assert T0.max() > 1.0 > T0.min()  # the floor max((T / T0)^3, 1) is active in the wings only
    sg = radpulse_problem(ctx, 32, pow_mode=1, initial_state=U0)
    assert np.array_equal(U0, sg.state_new_cc_.valid(0).cpu().numpy())
    for it in range(3000):
        assert so.step() and sg.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    U = sg.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(so.valid(0), U)
    assert U[6, 0, 0].max() > 1e3 * 4.0e-20  # radiation has come into equilibrium with the hot gas
    sp = radpulse_problem(ctx, 32, pow_mode=1)
    assert np.allclose(sp.state_new_cc_.valid(0).cpu().numpy(), U0, rtol=1e-14, atol=0)
    for it in range(3000):
        assert sp.step()
    assert np.allclose(sp.state_new_cc_.valid(0).cpu().numpy(), U, rtol=1e-10, atol=0)


@pytest.mark.parametrize("rad_order", [1, 2, 3])
def test_fused_radiation_stage_equals_the_separate_operators(ctx, rad_order):
    """qk_rad_stage_fused (three sweeps that take the flux divergence where the fluxes are produced; the Z sweep finishes PredictStep /
    AddFluxesRK2 and writes the stage-2 state in place) against computeRadiationFluxes + PredictStep / AddFluxesRK2: every component of the
    state and, when they are asked for (flux registers), the face fluxes of both stages, bit for bit.  The shell at 16^3 in 8^3 boxes and in a
    single 16^3 box (the Y sweep marches strips of 16 cells; tests/test_full_size_configs_gpu.py runs 128^3 boxes: eight strips per pencil), and
    in a single 40^3 box, the smallest with strip seams and tail strips everywhere: Y strips of 16 + 16 + 8 cells, Z strips of 32 + 8 (stage 1; stage 2
    marches whole pencils), 41 flux faces = 5 strips of 8 + one that holds only the last face, 48 x 40 = 1920 slab positions per plane in eight X
    workgroups whose seams fall in mid-row, a partial wave of 40 lanes along x."""
    for N, mgs in ((16, 8), (16, 16), (40, 40)):
        sims = []
        for fused in (True, False):
            s = shell_problem(ctx, N, table(), max_grid_size=mgs, pow_mode=1)
            s.radiationReconstructionOrder_ = rad_order
            assert s.use_fused_rad
            s.use_fused_rad = fused
            s.store_rad_flux = True
            for _ in range(2):
                assert s.step()
            sims.append(s)
        a, b = sims
        for x, y in zip(a.gather_valid_local(), b.gather_valid_local()):
            assert np.array_equal(x, y)
        for d in range(3):
            for fa, fb in ((a.radFluxOld[d], b.radFluxOld[d]), (a.radFlux[d], b.radFlux[d])):
                for n in range(a.lev.nboxes):
                    assert torch.equal(fa.fabs[n], fb.fabs[n]), (N, mgs, d, n)
        assert a.rad_counters == b.rad_counters


def test_fused_radiation_stage_in_place_through_two_tables_over_one_storage(ctx):
    """qk_rad_stage_fused, stage 1 (the Z sweep marches strips of 32 cells when U_new is not U_in), called with U_new = a SECOND descriptor table
    over the storage of U_in (MultiFab.subset_ptr: the same fab pointers at another table address — what the host cannot tell from the table
    pointers): the kernel sees the equal fab pointers and gives a pencil to one thread; the result is the out-of-place stage's, bit for bit.
    One 64^3 box (two strips per pencil), all three reconstruction orders."""
    import ctypes as C
    from quokka_amd.multifab import MultiFab
    from quokka_amd.radhydro import _d3
    for order in (1, 2, 3):
        s = shell_problem(ctx, 64, table(), max_grid_size=64, pow_mode=1)
        s.radiationReconstructionOrder_ = order
        assert s.step()
        U = s.state_new_cc_
        s._fill_rad_ghosts(U)
        out = MultiFab(s.lev, U.ncomp, U.nghost, fill=0.0)
        out.copy_from(U)
        acc = MultiFab(s.lev, s.nrad, 0)
        dt = 0.3 * s.geom.dx[0] / s.rad_traits.c_hat
        c = ctx

        def stage(U_new_ptr):
            c.check(c.L.qk_rad_stage_fused(s.lev.h, c.stream(), C.byref(s.rad_traits), order, 1, U.ptr, U.ptr, U_new_ptr, acc.ptr, None, float(dt),
                                           _d3(s.geom.dx), None), "qk_rad_stage_fused")
        stage(out.ptr)  # out of place: strips
        want = [out.valid(b).clone() for b in range(s.lev.nboxes)]
        alias = U.subset_ptr(list(range(s.lev.nboxes)))
        assert alias.value != U.ptr.value
        stage(alias)  # in place through another table
        for b in range(s.lev.nboxes):
            assert torch.equal(U.valid(b), want[b]), (order, b)
        assert not torch.equal(want[0][6], s.state_old_cc_.valid(0)[6])  # (the stage changed the radiation energy)


@pytest.mark.gpu
def test_mirrored_radiation_swap_equals_the_copy(ctx):
    """qk_rad_AddSourceTermsSingleGroupMirror: the stage-2 source-term kernel of substep i stores the new radiation components of the valid
    cells into state_old as well, which is what swapRadiationState() (reference src/QuokkaSimulation.hpp:1783-1788) copies when substep i + 1
    opens; the ghost cells it does not write are all filled by advanceRadiationForwardEuler before anything reads them.  Both ways: every
    component of the new state, the radiation components of the valid cells of the old state and the Newton counters, bit for bit; and the
    run takes several substeps per step (otherwise nothing is tested)."""
    sims = []
    for mirror in (True, False):
        s = shell_problem(ctx, 16, table(), max_grid_size=8, pow_mode=1)
        assert s.use_rad_mirror
        s.use_rad_mirror = mirror
        for _ in range(3):
            assert s.step()
        sims.append(s)
    a, b = sims
    assert a.rad_counters == b.rad_counters and a.rad_counters["solves"] > 2 * 3 * 16 ** 3  # more than one substep per step
    for x, y in zip(a.gather_valid_local(), b.gather_valid_local()):
        assert np.array_equal(x, y)
    ng = a.state_old_cc_.nghost
    for n in range(a.lev.nboxes):
        va = a.state_old_cc_.fabs[n][6:10, ng:-ng, ng:-ng, ng:-ng]
        vb = b.state_old_cc_.fabs[n][6:10, ng:-ng, ng:-ng, ng:-ng]
        assert torch.equal(va, vb), n


@pytest.mark.gpu
def test_shell_with_the_carried_rk2_average_stays_within_tolerance(ctx):
    """bench.py runs the hydro stage pair of the shell in the headline's form of the RK2 average (rk2_carry_rhs: 0.5 rhs1 + 0.5 rhs2 on the cell
    instead of 0.5 F1 + 0.5 F2 on the faces; PLM here, the Sedov tests cover PPM): <= 1e-12 relative L1 per component against the
    reference's form after 5 coupled radiation-hydro steps, and the carried form is really the one that ran."""
    sims = []
    for carry in (False, True):
        s = shell_problem(ctx, 16, table(), max_grid_size=8, pow_mode=1)
        s.rk2_carry_rhs = carry
        for _ in range(5):
            assert s.step()
        assert s._carry_active() == carry
        sims.append(s)
    a, b = sims
    for x, y in zip(a.gather_valid_local(), b.gather_valid_local()):
        for n in range(x.shape[0]):
            den = np.abs(x[n]).sum()
            if den > 0:
                assert np.abs(x[n] - y[n]).sum() <= 1e-12 * den, n


@pytest.mark.parametrize("rad_order", [2, 3])
def test_fused_radiation_stage_with_four_photon_groups(ctx, rad_order):
    """qk_rad_stage_fused with ngroups > 1 (one set of sweeps per photon group: the groups are transported independently, reference
    src/radiation/radiation_system.hpp:667-771) against computeRadiationFluxes + PredictStep / AddFluxesRK2 on a 3-D level of eight boxes with
    rough, valid radiation states in every group: both stages, every component and every stored face flux, bit for bit."""
    from quokka_amd import capi
    from quokka_amd.radhydro import RAD0, RadhydroSimulation
    from quokka_amd.radhydro_multigroup import H_PLANCK, PPL_FIXED_SLOPE, PulseMGConstants as S
    from quokka_amd.simulation import Geometry
    ng, n = 4, 16
    ncomp = RAD0 + 4 * ng
    geom = Geometry(3, [n] * 3, [0.0] * 3, [1024.0] * 3, [1, 1, 1])
    bcs = [([capi.BC_INT_DIR] * 3, [capi.BC_INT_DIR] * 3) for _ in range(ncomp)]
    traits = capi.traits(5.0 / 3.0, True, 3, mean_molecular_weight=S.mu, boltzmann_constant=capi.K_B)
    sims = []
    for fused in (True, False):
        rt = capi.RadTraits(S.c, S.chat, S.a_rad, S.erad_floor, 1, 0, S.kappa0, S.kappa0, S.kappa0, 1, 0)
        rt.set_groups(S.boundaries, H_PLANCK, PPL_FIXED_SLOPE, [0.0] * (ng + 1), [S.kappa0] * (ng + 1))
        s = RadhydroSimulation(ctx, geom, traits, rt, bcs, [8] * 3)
        assert s.nGroups == ng and s.use_fused_rad
        s.use_fused_rad = fused
        s.store_rad_flux = True
        s.radiationReconstructionOrder_ = rad_order
        rng = np.random.default_rng(3)

        def ic(i, j, k):
            U = np.zeros((ncomp,) + i.shape)
            U[0], U[4], U[5] = 1.0, 1.0, 1.0
            for g in range(ng):
                E = S.Erad0 * rng.uniform(0.1, 10.0, i.shape)
                f = rng.uniform(-0.55, 0.55, (3,) + i.shape)  # |F| <= 0.95 c E
                U[RAD0 + 4 * g] = E
                for d in range(3):
                    U[RAD0 + 4 * g + 1 + d] = f[d] * S.c * E
            return U

        s.set_initial_conditions(ic)
        s.state_old_cc_.copy_from(s.state_new_cc_)
        dt = 0.3 * geom.dx[0] / S.chat
        s.advanceRadiationForwardEuler(dt)
        s.advanceRadiationMidpointRK2(dt)
        sims.append(s)
    a, b = sims
    for x, y in zip(a.gather_valid_local(), b.gather_valid_local()):
        assert np.array_equal(x, y)
    for d in range(3):
        for fa, fb in ((a.radFluxOld[d], b.radFluxOld[d]), (a.radFlux[d], b.radFlux[d])):
            for k in range(a.lev.nboxes):
                assert torch.equal(fa.fabs[k], fb.fabs[k]), (d, k)
    # the transport did change every group
    new, old = a.state_new_cc_.valid(0).cpu().numpy(), a.state_old_cc_.valid(0).cpu().numpy()
    for g in range(ng):
        assert not np.array_equal(new[RAD0 + 4 * g], old[RAD0 + 4 * g])


# ------------------------------------------------------------------ use_wavespeed_correction (ComputeCellOpticalDepth + S_corr on the even faces)
def test_wavespeed_correction_factors_match_the_defining_formula(ctx):
    """qk_rad_ComputeWavespeedCorrection (reference src/radiation/radiation_system.hpp:803-871, :1098-1109) on a rough gas state, constant flux-mean
    opacity (tau = dl rho kappa: no libm): epsilon = min(1, 1 / harmonic mean of the two cells' optical depths) on the faces with i + j + k even, 1
    on the others — every face of every direction equal in every bit to the same IEEE operations in numpy; both sides of tau = 1 occur."""
    from quokka_amd.multifab import MultiFab
    from quokka_amd.radhydro import _d3, _p3
    s = shell_problem(ctx, 16, table(), max_grid_size=8, pow_mode=1)
    rng = np.random.default_rng(5)
    N, ng = 16, 4
    # optical depths per cell between 0.01 and 100 (periodic box: the ghost-inclusive field is built by wrapping)
    rho = 10.0 ** rng.uniform(-2.0, 2.0, (N + 2 * ng,) * 3) / (float(s.geom.dx[0]) * float(s.rad_traits.kappaF))
    idx = (np.arange(-ng, N + ng)) % N
    rho = rho[ng:-ng, ng:-ng, ng:-ng][np.ix_(idx, idx, idx)]
    for b, (lo, hi) in enumerate(s.my_boxes):
        U = s.state_new_cc_.fabs[b].cpu().numpy().copy()
        sl = tuple(slice(lo[d], hi[d] + 1 + 2 * ng) for d in (2, 1, 0))
        U[0] = rho[sl]
        s.state_new_cc_.set_fab(b, U)
    eps = [MultiFab(s.lev, 1, 0, facedir=d) for d in range(3)]
    c = ctx
    c.check(c.L.qk_rad_ComputeWavespeedCorrection(s.lev.h, c.stream(), C.byref(s.rad_traits), C.byref(s.traits), 3, s.state_new_cc_.ptr, _d3(s.geom.dx), _p3(eps)),
            "qk_rad_ComputeWavespeedCorrection")
    kappaF = float(s.rad_traits.kappaF)
    assert int(s.rad_traits.opacity_model) == 0
    below = above = 0
    for d in range(3):
        dl = float(s.geom.dx[d])
        for b, (lo, hi) in enumerate(s.my_boxes):
            got = eps[d].fabs[b][0].cpu().numpy()  # [k, j, i], nodal in d
            n = [hi[a] - lo[a] + 1 + (1 if a == d else 0) for a in range(3)]
            k, j, i = np.meshgrid(*(np.arange(lo[a], lo[a] + n[a]) for a in (2, 1, 0)), indexing="ij")
            sh = [0, 0, 0]
            sh[d] = 1
            rR = rho[k + ng, j + ng, i + ng]
            rL = rho[k + ng - sh[2], j + ng - sh[1], i + ng - sh[0]]
            tL, tR = dl * rL * kappaF, dl * rR * kappaF
            tau = (tL * tR * 2.0) / (tL + tR)
            inv = 1.0 / tau
            want = np.where((i + j + k) % 2 == 0, np.where(inv < 1.0, inv, 1.0), 1.0)
            assert got.shape == want.shape and np.array_equal(got, want), (d, b)
            below += int(((want < 1.0)).sum())
            above += int(((want == 1.0) & ((i + j + k) % 2 == 0)).sum())
    assert below > 100 and above > 100, (below, above)


@pytest.mark.parametrize("fused", [True, False])
def test_wavespeed_corrected_transport_matches_oracle_in_3d(ctx, oracle, fused):
    """use_wavespeed_correction_ = true (reference src/QuokkaSimulation.hpp:133, :1958-1960) through the three flux kernels of a 3-D level — the fused
    sweeps and the separate operators —: the shell at 16^3 in 8^3 boxes with the gas density roughened over four decades (cell optical depths on both
    sides of 1), three coupled steps, every component bit for bit against the oracle's restatement; and the correction does change the answer."""
    N = 16
    finals = []
    for corr in (True, False):
        so, sg = make_pair(ctx, oracle, N, 8, 1)
        rng = np.random.default_rng(9)
        fac = 10.0 ** rng.uniform(-2.0, 2.0, (N, N, N))
        for b in range(so.nboxes):
            lo, hi = so.box(b)
            U = so.state(b, 0).copy()
            f = np.ones(U.shape[1:])
            f[4:-4, 4:-4, 4:-4] = fac[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
            U[0:6] *= f  # (rho, momenta and energies together: velocities and temperature as before)
            so.set_state(U, b, 0)
            so.set_state(U, b, 1)
        so.set_wavespeed_correction(corr)
        sg.use_wavespeed_correction_ = corr
        sg.use_fused_rad = fused
        seed_from_oracle(so, sg)
        for it in range(3):
            assert so.step() and sg.step()
            assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
        Uo = gather([so.box(b) for b in range(so.nboxes)], [so.valid(b) for b in range(so.nboxes)], N)
        Ug = gather(sg.my_boxes, sg.gather_valid_local(), N)
        assert not np.isnan(Ug).any()
        assert np.array_equal(Uo, Ug), f"corr={corr}: rel L1 per component {rel_l1(Ug, Uo)}"
        finals.append(Ug)
    assert not np.array_equal(finals[0][6], finals[1][6]), "the correction changed nothing: the test state never reaches tau > 1 on an even face"


def test_wavespeed_corrected_marshak_wave_matches_oracle(ctx, oracle):
    """tests/MarshakAsymptoticCorr.in (marshak.use_wavespeed_correction = true): the temperature power-law opacity inside ComputeCellOpticalDepth
    (`opacity_model = 2`, ~1e5 optical depths per cell: epsilon << 1 on every even face), 2500 steps bit for bit (pow_mode 1)."""
    from oracle.pyoracle import MARSHAK_ASYMPTOTIC
    from quokka_amd.radhydro import marshak_asymptotic_problem
    so = oracle.sim(MARSHAK_ASYMPTOTIC, 1, [60, 1, 1], [0, 0, 0], [0.66, 1, 1], [0, 1, 1], max_grid_size=[60, 1, 1], rad_pow_mode=1)
    sg = marshak_asymptotic_problem(ctx, 60, pow_mode=1)
    so.set_wavespeed_correction(True)
    sg.use_wavespeed_correction_ = True
    ref = marshak_asymptotic_problem(ctx, 60, pow_mode=1)
    for it in range(2500):
        assert so.step() and sg.step() and ref.step()
        assert so.dt == sg.dt_, (it, so.dt, sg.dt_)
    U = sg.state_new_cc_.valid(0).cpu().numpy()
    assert np.array_equal(so.valid(0), U)
    assert not np.array_equal(U[6], ref.state_new_cc_.valid(0).cpu().numpy()[6])
