"""The reference's OWN problem files — read in place from /root/reference/src/problems, compiled UNCHANGED against quokka_amd/host
(oracle/Makefile refproblem, into oracle/_ref/: -x hip; their ParallelFor / MFIter lambdas, setCustomBoundaryConditions and
ErrorEst run as HIP kernels, every hot-path operator goes through the C-ABI) — run on the GPU with the reference's decks and meet the
reference's own pass criteria.  The binaries are built where the reference tree exists and travel to the GPU machine with
oracle/_ref/MANIFEST; the sources do not.  A binary the MANIFEST lists but that is missing is a FAILURE; the module
skips only where nothing was ever built (no MANIFEST)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "quokka_amd", "host")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")


def exe(name):
    path = os.path.join(REF_BIN, name)
    if not os.path.exists(path):
        manifest = os.path.join(REF_BIN, "MANIFEST")
        built = open(manifest).read().split() if os.path.exists(manifest) else []
        assert name not in built, f"{name} is listed in oracle/_ref/MANIFEST but missing: the reference-problem coverage would silently be zero"
        pytest.skip(f"{name} not built (needs the reference tree at build time: __graft_entry__.build_refproblems)")
    return path


def run(cmd, cwd, timeout=900):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    return p.returncode, p.stdout + p.stderr


def test_unmodified_sedov_problem_matches_the_oracle_state_and_its_own_criteria(tmp_path):
    dump = str(tmp_path / "state.bin")
    rc, out = run([exe("ref_HydroBlast3D"), "geometry.prob_lo=0 0 0", "geometry.prob_hi=1.2 1.2 1.2", "geometry.is_periodic=0 0 0", "amr.n_cell=32 32 32",
                   "amr.max_grid_size=32", "max_timesteps=10", f"qk.dump_state={dump}"], str(tmp_path))
    gold = np.load(os.path.join(ROOT, "tests", "golden", "sedov_32_step10.npz"))["state"]
    data = np.fromfile(dump, dtype=np.float64)
    assert np.array_equal(data.reshape(6, 32, 32, 32), gold), out[-1500:]  # the device-lambda initial conditions + fused path == oracle, bit for bit
    assert "Energy conservation is OK." in out
    # the reference's ctest: 128^3 to t = 1 (energy to 2e-15, kinetic-energy fraction within 1 % of 0.218729): exit status 0
    rc, out = run([exe("ref_HydroBlast3D"), os.path.join(HOST, "decks", "blast_unigrid_256.in"), "amr.n_cell=128 128 128", "amr.max_grid_size=128", "max_timesteps=20000"], str(tmp_path))
    assert rc == 0, out[-2000:]
    assert "Energy conservation is OK." in out and "Kinetic energy production is OK." in out


def test_carried_form_over_the_whole_run_of_the_reference_ctest(tmp_path):
    """The headline's form of the RK2 average (hydro.rk2_carry_rhs = 1: the carried half step) over a WHOLE run, not 25 or 40 steps: the
    reference's HydroBlast3D ctest — 128^3 to t = 1, ~12 000 steps — through the unchanged problem file in both forms.  Both meet both criteria of
    the reference (energy to 2e-15, kinetic-energy fraction within 1 % of 0.218729: exit status 0).  The final STATES are not comparable cell by
    cell: the blast amplifies a one-ulp difference by 10^14 within 5000 steps, in either form (tests/test_hydro_step_gpu.py::
    test_drift_of_the_carried_form_is_that_of_a_one_ulp_perturbation measures it, profiles/round4/carry_drift_128.txt) — their difference is printed."""
    import re
    states, steps = {}, {}
    for mode in (0, 1):
        dump = str(tmp_path / f"state{mode}.bin")
        rc, out = run([exe("ref_HydroBlast3D"), os.path.join(HOST, "decks", "blast_unigrid_256.in"), "amr.n_cell=128 128 128", "amr.max_grid_size=128",
                       "max_timesteps=20000", f"hydro.rk2_carry_rhs={mode}", f"qk.dump_state={dump}"], str(tmp_path))
        assert rc == 0, out[-2000:]
        assert "Energy conservation is OK." in out and "Kinetic energy production is OK." in out
        m = re.search(r"qk counters: steps=(\d+) fofc_stages=(\d+) retries=(\d+)", out)
        assert m, out[-1500:]
        steps[mode] = tuple(int(x) for x in m.groups())
        states[mode] = np.fromfile(dump, dtype=np.float64).reshape(6, 128, 128, 128)
    assert min(steps[0][0], steps[1][0]) > 5000 and abs(steps[0][0] - steps[1][0]) < 0.1 * steps[0][0], steps
    worst = max(np.abs(states[1][n] - states[0][n]).sum() / np.abs(states[0][n]).sum() for n in (0, 4))
    print(f"carried half step vs exact form, HydroBlast3D 128^3 to t = 1: steps / fofc stages / retries {steps[0]} vs {steps[1]}; "
          f"relative L1 of density and energy at t = 1: {worst:.2e} (chaotic amplification of rounding, see the docstring)")


def test_unmodified_sedov_problem_with_its_own_error_estimator_on_three_levels(tmp_path):
    """blast_amr_maxlev2.in (BASELINE config 5): the problem's ErrorEst — a device lambda over MFIter boxes calling HydroSystem::ComputePressure —
    drives the regridding; energy is conserved across levels"""
    import re
    updates = []
    # (hydro.rk2_carry_rhs = 1: the base level in the carried form of the RK2 average, flux_rk2 formed only on the faces its flux register marks —
    # qk_hydro_stage_args::flux_mask; the same grids, the same conservation)
    for extra in ([], ["hydro.rk2_carry_rhs=1"]):
        rc, out = run([exe("ref_HydroBlast3D"), os.path.join(HOST, "decks", "blast_amr_maxlev2.in"), "amr.n_cell=64 64 64", "max_timesteps=40"] + extra, str(tmp_path))
        assert "Energy conservation is OK." in out, out[-2000:]
        m = re.findall(r"Zone-updates on level (\d): (\d+)", out)
        assert len(m) == 3 and int(m[2][1]) > 0, out[-2000:]  # a level 2 exists and was advanced
        updates.append(m)
    assert updates[0] == updates[1], updates


def test_unmodified_shocktube_problem_meets_the_reference_criterion(tmp_path):
    """tests/shocktube.in with the reference's own computeReferenceSolution (reads ../extern/ppm1d/output: the committed byte-identical copy is
    put where the problem looks for it) and its device setCustomBoundaryConditions (Dirichlet states): relative L1 error <= 0.002, exit 0"""
    os.makedirs(tmp_path / "extern" / "ppm1d")
    os.makedirs(tmp_path / "build")
    shutil.copy(os.path.join(ROOT, "tests", "golden", "ppm1d_sod_exact.txt"), tmp_path / "extern" / "ppm1d" / "output")
    rc, out = run([exe("ref_HydroShocktube"), os.path.join(HOST, "decks", "shocktube_amr.in")], str(tmp_path / "build"))
    assert rc == 0, out[-2500:]


def test_unmodified_shell_problem_matches_the_python_driver(tmp_path, ctx):
    """RadhydroShell (BASELINE config 4) at 32^3: initial conditions interpolated from ./initial_conditions.txt inside a device lambda
    (Gpu::DeviceVector tables), the problem's opacity specialisations, the point source set by the problem's own kernel.  The reference has
    no pass criterion for it beyond finishing; the state after its 50 coupled steps must agree to 1e-11 with the Python driver's
    (quokka_amd/radhydro.py, which tests/test_radhydro_gpu.py holds to the oracle bit for bit; numpy and device libm differ by an ulp in
    exp / pow of the initial conditions)."""
    from quokka_amd.radhydro import shell_problem
    shutil.copy(os.path.join(ROOT, "tests", "golden", "dust_shell_initial_conditions.txt"), tmp_path / "initial_conditions.txt")
    args = [os.path.join(HOST, "decks", "radhydro_shell_256.in"), "amr.n_cell=32 32 32", "amr.max_grid_size=16", "max_timesteps=50"]  # (the reference problem sets maxTimesteps_ = 50 itself)
    dump = str(tmp_path / "ref_RadhydroShell.bin")
    rc, out = run([exe("ref_RadhydroShell")] + args + [f"qk.dump_state={dump}"], str(tmp_path))
    assert rc == 0, out[-2500:]
    assert "Performance figure-of-merit" in out
    a = np.fromfile(dump, dtype=np.float64)
    tab = np.loadtxt(os.path.join(ROOT, "tests", "golden", "dust_shell_initial_conditions.txt"), skiprows=1)
    sim = shell_problem(ctx, 32, (tab[:, 0], tab[:, 2], tab[:, 3]), max_grid_size=16)
    assert sim.evolve() and sim.istep == 50
    b = np.stack([sim.state_new_cc_.valid(k).cpu().numpy().reshape(10, -1) for k in range(sim.lev.nboxes)])
    assert a.size == 8 * 10 * 16 ** 3
    a = a.reshape(8, 10, -1)
    for n in (0, 4, 5, 6):  # density, gas energies, radiation energy (momenta / fluxes sum to ~0 over the symmetric shell)
        assert np.abs(a[:, n] - b[:, n]).sum() <= 1e-11 * np.abs(b[:, n]).sum(), n


def test_unmodified_shell_problem_on_a_refined_hierarchy(tmp_path, ctx):
    """RadhydroShell with the reference's AMR deck (tests/radhydro_shell_amr.in, scaled to 32^3 + one level): radiation on refined levels in the
    C++ host — the radiation subcycle of every level with coarse-fine ghost cells interpolated at the substep's time, the radiation fluxes of both
    stages in the flux register of the radiation block, the problem's own ErrorEst (density jump) as a device lambda.  No pass criterion in the
    file; here: the same number of refined cell-updates and the same level-0 state (to 1e-12: host / device libm in the initial conditions) as
    the Python AMR driver, whose radiation levels tests/test_amr_radiation_gpu.py pins by bit-equality with uniform runs and by conservation."""
    import re
    from quokka_amd.amr_simulation import shell_amr_problem
    shutil.copy(os.path.join(ROOT, "tests", "golden", "dust_shell_initial_conditions.txt"), tmp_path / "initial_conditions.txt")
    dump = str(tmp_path / "shell_amr.bin")
    rc, out = run([exe("ref_RadhydroShell"), os.path.join(HOST, "decks", "radhydro_shell_amr.in"), "amr.n_cell=32 32 32", "amr.max_level=1",
                   "amr.blocking_factor=8", "amr.max_grid_size=32", f"qk.dump_state={dump}"], str(tmp_path))
    assert rc == 0 and "Finished." in out, out[-2500:]
    m = re.search(r"Zone-updates on level 1: (\d+) \((\d+) grids\)", out)
    assert m and int(m.group(1)) > 10 ** 7
    tab = np.loadtxt(os.path.join(ROOT, "tests", "golden", "dust_shell_initial_conditions.txt"), skiprows=1)
    amr = shell_amr_problem(ctx, 32, 1, (tab[:, 0], tab[:, 2], tab[:, 3]), max_grid_size=32, blocking_factor=8)
    amr.evolve()
    a = np.fromfile(dump, dtype=np.float64).reshape(10, 32, 32, 32)
    b = amr.levels[0].state_new_cc_.valid(0).cpu().numpy()
    assert amr.istep[0] == 50 and amr.cellUpdatesEachLevel_[1] == int(m.group(1))
    for n in (0, 4, 5, 6):
        assert np.abs(a[n] - b[n]).sum() <= 1e-12 * np.abs(b[n]).sum(), (n, np.abs(a[n] - b[n]).sum() / np.abs(b[n]).sum())


def extern_tree(tmp_path, files):
    """the reference's problem files open `../extern/...` relative to their working directory (its tests/ directory): put the committed copies of
    those data tables where the unmodified problem looks for them"""
    build = tmp_path / "build"
    os.makedirs(build)
    for rel, golden in files.items():
        dst = tmp_path / "extern" / rel
        os.makedirs(dst.parent, exist_ok=True)
        shutil.copy(os.path.join(ROOT, "tests", "golden", golden), dst)
    return str(build)


def test_unmodified_multigroup_shock_meets_the_reference_criterion(tmp_path):
    """RadhydroShockMultigroup, unchanged: 5 photon groups, PPL_opacity_fixed_slope_spectrum; its setCustomBoundaryConditions and initial
    conditions call RadSystem::ComputeThermalRadiationMultiGroup inside device lambdas (the host mirror's own Planck-integral interpolation);
    DefineOpacityExponentsAndLowerValues is sampled into the closed set (577 / rho, exponent 0).  Exit status 0 = T_rad within 0.008 of the
    Lowrie-Edwards solution."""
    cwd = extern_tree(tmp_path, {"LowrieEdwards/shock.txt": "LowrieEdwards_shock.txt"})
    rc, out = run([exe("ref_RadhydroShockMultigroup"), os.path.join(HOST, "decks", "radshockMG.in")], cwd)
    assert rc == 0, out[-2500:]


@pytest.mark.parametrize("name,deck,extern,steps", [
    ("RadhydroShockMultigroup", "radshockMG.in", {"LowrieEdwards/shock.txt": "LowrieEdwards_shock.txt"}, 400),  # 5 groups, fixed-slope spectrum, beta_order 1
    ("RadMarshakVaytet", "MarshakVaytet.in", {}, 400),  # 6 groups, full spectrum (slopes re-fitted in every Newton iteration), kappa ~ nu^-2
])
def test_compiled_multigroup_opacity_hook_equals_the_closed_set(tmp_path, name, deck, extern, steps):
    """The multigroup kernel with the problem's DefineOpacityExponentsAndLowerValues COMPILED in (qkhost::ProblemRadMG: at(rho, T) refreshes the
    exponents and lower values at the five places the reference evaluates the hook) against the library's closed-set instantiation, on problems
    both can express (`qk.mg_compiled_hook = 1` forces the former): the final state of the unchanged reference problem, bit for bit.  What
    only the compiled hook can express is RadhydroPulseMGint (MORE_CTESTS)."""
    dumps = []
    for forced in (0, 1):
        cwd = extern_tree(tmp_path / f"w{forced}", extern)
        dump = os.path.join(cwd, "state.bin")
        rc, out = run([exe(f"ref_{name}"), os.path.join(HOST, "decks", deck), f"max_timesteps={steps}", f"qk.mg_compiled_hook={forced}",
                       f"qk.dump_state={dump}", "plotfile_interval=-1", "checkpoint_interval=-1"], cwd)
        assert os.path.exists(dump), out[-2500:]  # (the truncated run may miss the problem's own criterion: only the state is compared)
        dumps.append(np.fromfile(dump, dtype=np.float64))
    assert dumps[0].size > 0 and np.isfinite(dumps[0]).all()
    assert np.array_equal(dumps[0], dumps[1])


def test_unmodified_radiation_tube_meets_the_reference_criterion(tmp_path):
    """RadTube, unchanged: 2 groups, piecewise-constant opacity, table-interpolated initial conditions (preCalculateInitialConditions ->
    Gpu::DeviceVector), a boundary functor that reads the first valid cell.  Exit status 0 = T_rad within 0.003 of the static solution."""
    cwd = extern_tree(tmp_path, {"pressure_tube/initial_conditions.txt": "pressure_tube_initial_conditions.txt"})
    rc, out = run([exe("ref_RadTube"), os.path.join(HOST, "decks", "RadTube.in")], cwd)
    assert rc == 0, out[-2500:]


def test_unmodified_dust_problem_meets_the_reference_criterion(tmp_path):
    """RadDust, unchanged: ISM_Traits::enable_dust_gas_thermal_coupling_model, the problem's own ComputeThermalRadiationSingleGroup hooks
    (detected as the linearised emission), dust_gas_interaction_coeff from the deck, computeAfterTimestep collecting T_gas / T_rad every step.
    Exit status 0 = within 0.0008 of extern/data/dust/rad_dust_exact.csv."""
    cwd = extern_tree(tmp_path, {"data/dust/rad_dust_exact.csv": "rad_dust_exact.csv"})
    rc, out = run([exe("ref_RadDust"), os.path.join(HOST, "decks", "RadDust.in")], cwd)
    assert rc == 0, out[-2500:]


def test_unmodified_multigroup_dust_problem_meets_the_reference_criterion(tmp_path):
    """RadDustMG, unchanged (it includes radiation/radiation_dust_system.hpp): four groups, the problem's own ComputeThermalRadiationMultiGroup hooks
    (detected as the linearised emission), ISM_Traits::gas_dust_coupling_threshold; the coupled branch of the multigroup dust solve.
    Exit status 0 = within 0.0008 of extern/data/dust/rad_dust_exact.csv."""
    cwd = extern_tree(tmp_path, {"data/dust/rad_dust_exact.csv": "rad_dust_exact.csv"})
    rc, out = run([exe("ref_RadDustMG"), os.path.join(HOST, "decks", "RadDust.in")], cwd)
    assert rc == 0, out[-2500:]


def test_unmodified_two_group_marshak_wave_with_dust_meets_the_reference_criterion(tmp_path):
    """RadMarshakDust, unchanged: two groups with kappa1 / kappa2 read from the deck by the problem itself (amrex::ParmParse in problem_main, stored in
    managed globals the opacity hook reads), a boundary functor that writes the gas state on every outside cell and the streaming radiation
    state beyond the lower face only; every solve on the decoupled branch.  Exit status 0 = within 0.01 of the analytic solution."""
    rc, out = run([exe("ref_RadMarshakDust"), os.path.join(HOST, "decks", "RadMarshakDust.in")], str(tmp_path))
    assert rc == 0, out[-2500:]


def test_unmodified_line_cooling_problem_meets_the_reference_criterion(tmp_path):
    """RadLineCooling, unchanged: the problem's DefineNetCoolingRate / ...TempDerivative / DefineCosmicRayHeatingRate specialisations are
    compiled into the single-group Newton-Raphson kernel of the problem's translation unit (qk_problem_kernels.hpp).  Exit status 0 = within 0.0005 of the analytic cooling curve."""
    rc, out = run([exe("ref_RadLineCooling"), os.path.join(HOST, "decks", "RadLineCooling.in")], str(tmp_path))
    assert rc == 0, out[-2500:]


@pytest.mark.parametrize("coeff", ["1e-20", "1e20"])
def test_unmodified_multigroup_line_cooling_problem_meets_the_reference_criterion(tmp_path, coeff):
    """RadLineCoolingMG, unchanged, with both of the reference's decks (RadLineCooling.in: decoupled gas and dust; RadLineCoolingCoupled.in):
    ISM_Traits::enable_photoelectric_heating, DefinePhotoelectricHeatingE1Derivative.  Exit status 0 = within 0.0005."""
    rc, out = run([exe("ref_RadLineCoolingMG"), os.path.join(HOST, "decks", "RadLineCooling.in"), f"radiation.dust_gas_interaction_coeff={coeff}"], str(tmp_path))
    assert rc == 0, out[-2500:]


@pytest.mark.parametrize("coeff", ["1e20", "1e-20"])
def test_unmodified_photoelectric_heating_front_meets_the_reference_criterion(tmp_path, coeff):
    """RadMarshakDustPE, unchanged, with both decks (coupled / decoupled).  Exit status 0 = within 0.01 of T = 1 + (t - x), E_FUV = 1 behind the front."""
    rc, out = run([exe("ref_RadMarshakDustPE"), os.path.join(HOST, "decks", "RadMarshakDustPE.in"), f"radiation.dust_gas_interaction_coeff={coeff}"], str(tmp_path))
    assert rc == 0, out[-2500:]


def test_unmodified_multigroup_pulse_meets_the_reference_criterion(tmp_path):
    """RadhydroPulseMGconst, unchanged: two simulations in one executable (grey at rest, 4 groups advected), compared with each other; 0.006"""
    rc, out = run([exe("ref_RadhydroPulseMGconst"), os.path.join(HOST, "decks", "RadhydroPulse.in")], str(tmp_path))
    assert rc == 0, out[-2500:]


def test_unmodified_vaytet_marshak_wave_runs_to_the_end(tmp_path):
    """RadMarshakVaytet, unchanged (PPL_opacity_full_spectrum, kappa ~ nu^-2, radiation only): the ctest passes when t_end is reached"""
    rc, out = run([exe("ref_RadMarshakVaytet"), os.path.join(HOST, "decks", "MarshakVaytet.in")], str(tmp_path), timeout=1500)
    assert rc == 0, out[-2500:]
    assert os.path.exists(tmp_path / "marshak_wave_Vaytet.csv")


def test_unmodified_nscbc_channel_meets_the_reference_criterion(tmp_path):
    """NSCBC/channel.cpp, unchanged (ctest ChannelFlow): a subsonic channel flow driven from 2e3 to 4e3 cm/s through a characteristic inflow
    (relaxation to the target temperature / velocity / scalar) and a characteristic outflow (far-field pressure), one passive scalar.  The
    boundary functor calls NSCBC::setInflowX1Lower / setOutflowBoundary — the host mirror's own characteristic formulation
    (quokka_amd/host/compat/nscbc.hpp) — inside the boundary kernel.  Exit status 0 = the rms of the component-wise relative L1 errors against
    the steady state (density, velocity, pressure, scalar) is below 3e-5 after t = 0.1 s."""
    rc, out = run([exe("ref_NSCBC_channel"), os.path.join(HOST, "decks", "NSCBC_Channel.in")], str(tmp_path), timeout=1500)
    assert rc == 0, out[-2500:]
    assert "rms of component-wise relative L1 error norms" in out


def test_unmodified_nscbc_vortex_runs_in_2d(tmp_path):
    """NSCBC/vortex.cpp, unchanged, as the 2-D build (AMREX_SPACEDIM = 2) of the host mirror: a vortex convected at 1e4 cm/s through characteristic
    outflow faces in x (transverse terms active: the flow has gradients along the boundary), periodic in y.  The reference's problem has no error
    norm (returns 0); here: it reaches t_end, the state is finite, the pressure stays within 1 % of the far field and the vortex is still there."""
    dump = str(tmp_path / "v.bin")
    rc, out = run([exe("ref_NSCBC_vortex"), os.path.join(HOST, "decks", "NSCBC_Vortex.in"), f"qk.dump_state={dump}"], str(tmp_path))
    assert rc == 0, out[-2500:]
    U = np.fromfile(dump, dtype=np.float64).reshape(7, 128, 128)
    assert np.isfinite(U).all()
    rho, px, py = U[0], U[1], U[2]
    P = (1.4 - 1.0) * (U[4] - 0.5 * (px * px + py * py) / rho)
    assert np.abs(P / 1.01325e6 - 1.0).max() < 0.01
    assert np.abs(py / rho).max() > 50.0 and np.abs(px / rho - 1.0e4).max() < 1.0e3


def test_unmodified_streaming_front_along_y_meets_the_reference_criterion(tmp_path):
    """RadStreamingY, unchanged, as the 2-D build its CMakeLists.txt asks for: the radiation operators on an AMREX_SPACEDIM == 2 level, Dirichlet
    faces in y written by the problem's own boundary functor.  Exit status 0 = within 0.05 of the step function at y = c t."""
    rc, out = run([exe("ref_RadStreamingY"), os.path.join(HOST, "decks", "RadStreamingY.in")], str(tmp_path))
    assert rc == 0, out[-2500:]


def test_unmodified_quirk_problem_meets_the_reference_criterion_and_matches_the_python_driver(tmp_path, ctx):
    """HydroQuirk, unchanged, as the 2-D build the reference's CMake enables it for: its computeAfterTimestep locates the shock's box with
    MFIter / Box::contains(IntVect) and evaluates the entropy jump with amrex::launch on a single-cell box into an amrex::AsyncArray; exit
    status 0 = max |delta s| <= 0.06 (no carbuncle).  The final state equals the Python driver's (which tests/test_hydro_2d.py ties to the
    oracle bit for bit), 772 steps later."""
    from quokka_amd.simulation import quirk_problem
    dump = str(tmp_path / "q.bin")
    rc, out = run([exe("ref_HydroQuirk"), os.path.join(HOST, "decks", "quirk.in"), f"qk.dump_state={dump}"], str(tmp_path))
    assert rc == 0 and "looks stable against the Carbuncle" in out, out[-2500:]
    U = np.fromfile(dump, dtype=np.float64).reshape(6, 16, 128)
    sg = quirk_problem(ctx, 2)
    assert sg.evolve() and sg.istep == 772
    assert np.array_equal(U, sg.state_new_cc_.valid(0).cpu().numpy()[:, 0])


def test_unmodified_implosion_problem_keeps_its_exact_diagonal_symmetry(tmp_path):
    """HydroRichtmeyerMeshkov, unchanged (2-D): after EVERY step the problem gathers the state with FabArray::ParallelCopy and aborts unless
    U(i, j) == U(j, i) exactly (momenta swapped) — which holds only if the y sweep of the 2-D build performs the x sweep's arithmetic on
    swapped indices (ArrayView_2d's index swap).  Four boxes, reflecting walls, run to the problem's own t = 2.5."""
    rc, out = run([exe("ref_HydroRichtmeyerMeshkov"), os.path.join(HOST, "decks", "implosion2d.in"), "amr.n_cell=32 32 8", "amr.max_grid_size=16", "amr.blocking_factor=16"],
                  str(tmp_path))
    assert rc == 0 and "Finished." in out and "not symmetric" not in out, out[-2500:]


def test_unmodified_rayleigh_taylor_problem_runs_with_its_strang_split_gravity(tmp_path):
    """RayleighTaylor3D, unchanged: gravity through addStrangSplitSources written as amrex::ParallelFor(MultiFab, f(box, i, j, k)) over
    MultiFab::arrays(), random initial velocities (ParallelForRNG), a passive scalar, reflecting walls in z, the mixing profile through
    QuokkaSimulation::computeAxisAlignedProfile.  No pass criterion in the file (returns 0); here: mass and scalar are conserved, the
    hydrostatic state holds (|v_z| stays at the size of the seeded perturbation) and the profile is the step 0 -> 1 of the scalar."""
    dump = str(tmp_path / "rt.bin")
    rc, out = run([exe("ref_RayleighTaylor3D"), os.path.join(HOST, "decks", "RT3D.in"), "amr.n_cell=64 64 64", "amr.max_grid_size=32", "max_timesteps=60",
                   f"qk.dump_state={dump}"], str(tmp_path))
    assert rc == 0 and "Performance figure-of-merit" in out, out[-2500:]
    U = np.fromfile(dump, dtype=np.float64).reshape(8, 7, 32, 32, 32)
    assert np.isfinite(U).all()
    n = 64 ** 3
    assert abs(U[:, 0].sum() / n - 1.5) < 1e-12 and abs(U[:, 6].sum() / n - 0.5) < 1e-12
    assert np.abs(U[:, 3] / U[:, 0]).max() < 0.02 and np.abs(U[:, 1]).max() < 0.02
    prof = np.loadtxt(os.path.join(str(tmp_path), "profile.txt"))
    # (the scalar is a conserved density: it is compressed with the heavy gas settling in the field, a few 1e-3)
    assert prof.shape == (64,) and np.all(prof[:28] < 1e-6) and np.all(np.abs(prof[36:] - 1.0) < 0.01)


@pytest.mark.parametrize("name,problem,ncell", [("ref_Advection", "ADVECTION_SAWTOOTH", 400), ("ref_AdvectionSemiellipse", "ADVECTION_SEMIELLIPSE", 400)])
def test_unmodified_advection_problems_meet_the_reference_criterion_and_match_the_oracle(tmp_path, oracle, name, problem, ncell):
    """Advection / AdvectionSemiellipse, unchanged (ctests ScalarAdvection, ScalarAdvectionSemiEllipse): AdvectionSimulation<problem_t> and
    LinearAdvectionSystem<problem_t> of the host mirror (quokka_advection.hpp) on qk_ReconstructStatesPPM + qk_advect_*; 10 000 RK2 steps, one period.
    Exit status 0 = relative L1 error <= 0.015 (test_advection.cpp:160-166); the final state equals the oracle's (oracle/hydro_sim.hpp
    advanceAdvectionAtLevel) in every bit (sawtooth) / to 1e-12 (semi-ellipse: libm in its initial condition)."""
    import oracle.pyoracle as po
    dump = str(tmp_path / "adv.bin")
    rc, out = run([exe(name), os.path.join(HOST, "decks", "advection_sawtooth.in"), f"qk.dump_state={dump}"], str(tmp_path))
    assert rc == 0 and "Relative rms L1 error norm" in out, out[-2000:]
    meta = [float(x) for x in open(dump + ".meta").read().split()]
    so = oracle.sim(getattr(po, problem), 1, [ncell, 1, 1], [0, 0, 0], [1.0, 1, 1], [1, 1, 1], max_grid_size=[ncell, 1, 1])
    assert so.evolve()
    assert int(meta[0]) == so.istep == 10000 and meta[1] == so.time and 1e-3 < meta[5] <= 0.015
    got, want = np.fromfile(dump, dtype=np.float64), so.valid(0).ravel()
    if problem == "ADVECTION_SAWTOOTH":
        assert np.array_equal(got, want)
    else:  # the semi-ellipse is initialised with std::sqrt(1 - std::pow(z, 2)) inside a device lambda: device libm vs glibc, an ulp in the initial state
        assert np.abs(got - want).sum() <= 1e-12 * np.abs(want).sum()


def test_unmodified_advection2d_problem_on_the_unrefined_grid_matches_the_oracle(tmp_path, oracle):
    """Advection2D, unchanged, as the 2-D build: four boxes, both sweeps of the advection solver (the y sweep through the 2-D index-swap view of
    qk_ReconstructStatesPPM), on the unrefined grid, where the error is 0.34 on oracle and GPU alike (exit status 1): the comparison with the
    oracle is the test — every bit after 227 steps.  (The problem's ctest refines three levels: next test.)"""
    from oracle.pyoracle import ADVECTION_SQUARE_2D
    dump = str(tmp_path / "adv2d.bin")
    rc, out = run([exe("ref_Advection2D"), os.path.join(HOST, "decks", "advection2d.in"), f"qk.dump_state={dump}"], str(tmp_path))
    assert rc in (0, 1) and "Relative rms L1 error norm" in out, out[-2000:]
    meta = [float(x) for x in open(dump + ".meta").read().split()]
    so = oracle.sim(ADVECTION_SQUARE_2D, 2, [64, 64, 1], [0, 0, 0], [1.0, 1.0, 1], [1, 1, 1], max_grid_size=[32, 32, 1])
    assert so.evolve()
    assert int(meta[0]) == so.istep and meta[1] == so.time
    got = np.fromfile(dump, dtype=np.float64).reshape(4, 32, 32)
    for b in range(4):
        assert np.array_equal(got[b], so.valid(b).reshape(32, 32)), b


@pytest.mark.parametrize("max_level", [1, 2])
def test_unmodified_blast2d_problem_on_a_two_dimensional_hierarchy(tmp_path, max_level):
    """HydroBlast2D, unchanged, with amr.max_level > 0: the level machinery of a 2-D build (tags -> Berger-Rigoutsos boxes, FillPatch from the
    parent, subcycling, flux registers with two fine faces per coarse face, average-down of four children).  With the grids frozen after the
    initial regrid (amr.regrid_int beyond the run) mass and total energy are conserved to rounding; with regridding every second step mass
    still is, while the energy moves by the amount the reference's own PreInterpState / PostInterpState hooks cost where new fine cells are
    created inside moving gas (they interpolate the internal energy, not the total: reference src/QuokkaSimulation.hpp:804-840).  (The problem
    file writes the four radiation components of a state that has none: amrex_mini.hpp keeps slack behind the last fab for that.)"""
    import re
    args = [exe("ref_HydroBlast2D"), "geometry.prob_lo=0 0 0", "geometry.prob_hi=1 1 1", "geometry.is_periodic=0 0 0", "amr.n_cell=128 128 8",
            "amr.max_grid_size=64", "amr.blocking_factor=16", "amr.n_error_buf=3", "do_reflux=1", "plotfile_interval=-1", "checkpoint_interval=-1",
            "do_tracers=0", f"amr.max_level={max_level}"]

    def errors(out):
        rel = dict(re.findall(r"Initial (gasDensity|gasEnergy) = \S+\n\s+absolute conservation error = \S+\n\s+relative conservation error = (\S+)", out))
        return float(rel["gasDensity"]), float(rel["gasEnergy"])
    rc, out = run(args + ["amr.regrid_int=100000"], str(tmp_path))
    assert rc == 0 and f"Zone-updates on level {max_level}" in out, out[-2500:]
    dm, de = errors(out)
    assert abs(dm) <= 1e-14 and abs(de) <= 1e-14, (dm, de)
    rc, out = run(args, str(tmp_path))
    assert rc == 0 and f"Zone-updates on level {max_level}" in out, out[-2500:]
    dm, de = errors(out)
    assert abs(dm) <= 1e-14 and abs(de) <= 2e-2, (dm, de)


def test_unmodified_face_centred_quantities_problem_round_trips_its_checkpoint(tmp_path):
    """FCQuantities, unchanged (the reference's ctest of the same name, deck tests/fc_hydro_wave.in): a face-centred state (one face velocity and
    one field component per direction: Physics_Indices::nvarPerDim_fc = 2) initialised by setInitialConditionsOnGridFaceVars, written to
    chk00000 as Level_0/Face_x|y|z next to Level_0/Cell (nodal boxes: one more index in the face direction, index type 1 there), read back by
    a second simulation object; the problem aborts unless the two agree exactly.  Also: the Face_* files as amrex::VisMF lays them out, and the
    plotfile carries the cell-centre averages 0.5 (f_i + f_i+1) after the cell-centred components."""
    from quokka_amd import plotfile
    rc, out = run([exe("ref_FCQuantities"), os.path.join(HOST, "decks", "fc_hydro_wave.in")], str(tmp_path))
    assert rc == 0 and "Accumulated error in MFs read from chk-file: 0" in out, out[-2500:]
    lvl = tmp_path / "chk00000" / "Level_0"
    for d, name in enumerate("xyz"):
        hdr = open(lvl / f"Face_{name}_H").read().split("\n")
        hi = [99, 39, 3]
        hi[d] += 1
        typ = ["0", "0", "0"]
        typ[d] = "1"
        assert hdr[:4] == ["1", "1", "2", "4"] and hdr[5] == f"((0,0,0) ({hi[0]},{hi[1]},{hi[2]}) ({','.join(typ)}))", hdr[:7]
        mf = plotfile.read_vismf(str(lvl / f"Face_{name}"))
        (lo, fhi), a = mf.fabboxes[0], mf.fabs[0]
        assert lo == [-4, -4, -4] and a.shape == (2,) + tuple(fhi[e] - lo[e] + 1 for e in (2, 1, 0))
        valid = a[:, 4:-4, 4:-4, 4:-4]
        idx = np.arange(hi[d] + 1) % 2
        want = (d + 1.0) + idx.reshape([-1 if e == d else 1 for e in (2, 1, 0)])  # 1 + i % 2, 2 + j % 2, 3 + k % 2 on the field component
        assert np.array_equal(valid[1], np.broadcast_to(want, valid[1].shape)) and not valid[0].any()
    plt = plotfile.read_plotfile(str(tmp_path / "plt00000"))
    assert plt.varnames[6:] == ["x-velocity", "y-velocity", "z-velocity", "x-BField", "y-BField", "z-BField"]
    fab = plt.levels[0].fabs[0]
    assert fab.shape == (12, 4, 40, 100)
    for d in range(3):  # per direction: [face velocity, field] averaged to the cell centre
        assert not fab[6 + 2 * d].any() and np.all(fab[7 + 2 * d] == d + 1.5)


def test_unmodified_advection2d_problem_with_its_three_level_ctest_deck(tmp_path):
    """Advection2D, unchanged, with the reference's ctest deck (tests/advection2d_amr.in: 64^2 base grid, amr.max_level = 3, subcycling, reflux,
    periodic): the advection solver on a 2-D hierarchy — AdvectionSimulation objects as the levels of AmrDriver (quokka_advection.hpp).  The
    square pulse crosses the periodic faces once; the hierarchy shrinks and regrows on the way (tags buffered through the periodic faces,
    proper nesting across them, the margins of levels rebuilt together, the start-up iteration that gives the narrow ring of level 2 its
    child).  EXIT STATUS 0: the reference's criterion — relative L1 error against its point-sampled solution <= 0.15, of which 0.138 is the
    difference between point samples and exact cell averages on level 0 — is met with 0.1447 (0.34 on level 0 alone).  Also: all four levels
    advance; the scalar is conserved to rounding through every regrid and through the periodic faces; two runs agree in every bit (they did not
    while geom[lev] of a level object read past a one-element vector: quokka_host.hpp ThisLevel)."""
    import re
    args = [exe("ref_Advection2D"), os.path.join(HOST, "decks", "advection2d_amr.in")]
    dumps = []
    for name, env in (("t0", {"QK_MAX_COARSE_STEPS": "0"}), ("a", {}), ("b", {})):
        dump = str(tmp_path / f"{name}.bin")
        p = subprocess.run(args + [f"qk.dump_state={dump}"], capture_output=True, text=True, timeout=900, cwd=str(tmp_path), env=dict(os.environ, **env))
        out = p.stdout + p.stderr
        assert p.returncode == 0, out[-2500:]  # (t0, no step taken, passes as well: the initial hierarchy is 0.129 from the point samples)
        dumps.append((np.fromfile(dump, dtype=np.float64), out))
    (u0, _), (ua, out), (ub, _) = dumps
    assert np.array_equal(ua, ub)
    updates = [int(x) for x in re.findall(r"Zone-updates on level \d: (\d+) ", out)]
    assert len(updates) == 4 and all(u > 0 for u in updates) and updates[0] == 227 * 64 * 64, updates
    assert abs(ua.sum() - u0.sum()) <= 1e-13 * u0.sum(), (ua.sum(), u0.sum())
    err = float(re.search(r"Relative rms L1 error norm = (\S+)", out).group(1))
    assert 0.138 < err <= 0.15, err


def test_unmodified_shocktube_cma_problem_with_its_refined_ctest_deck(tmp_path):
    """HydroShocktubeCMA, unchanged, with the reference's ctest deck (tests/shocktube_cma.in: three mass scalars with the consistent multi-fluid
    advection of the partial densities, artificial viscosity, one refined level with subcycling and reflux — nine components through
    interpolation, flux registers and average-down; mass scalars keep a level off the fused stage: the reference-shaped operators run).  Exit
    status 0: after every step the partial densities sum to the density to 1e-13 on level 0, which holds the average of the refined level
    (test_hydro_shocktube_cma.cpp:205-235)."""
    rc, out = run([exe("ref_HydroShocktubeCMA"), os.path.join(HOST, "decks", "shocktube_cma.in")], str(tmp_path))
    assert rc == 0, out[-2500:]
    import re
    updates = [int(x) for x in re.findall(r"Zone-updates on level \d: (\d+) ", out)]
    assert len(updates) == 2 and updates[1] > updates[0] > 0, updates


@pytest.mark.parametrize("name,deck", [("RadBeam", "beam.in"), ("RadShadow", "shadow.in")])
def test_unmodified_radiation_problems_on_two_dimensional_hierarchies(tmp_path, name, deck):
    """RadBeam and RadShadow, unchanged, with the reference's decks (tests/beam.in, tests/shadow.in: 2-D, amr.max_level = 2, subcycling, reflux;
    radiation only — is_hydro_enabled = false —, custom boundary functions on the device): the radiation block through FillPatch, the second
    flux register of a level and average-down on 2-D hierarchies.  The reference gives these problems no pass criterion (they return 0): 40
    coarse steps here, every level advances and the state stays finite."""
    import re
    dump = str(tmp_path / "state.bin")
    p = subprocess.run([exe(f"ref_{name}"), os.path.join(HOST, "decks", deck), "plotfile_interval=-1", "checkpoint_interval=-1", f"qk.dump_state={dump}"],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path), env=dict(os.environ, QK_MAX_COARSE_STEPS="40"))
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-2500:]
    updates = [int(x) for x in re.findall(r"Zone-updates on level \d: (\d+) ", out)]
    assert len(updates) == 3 and all(u > 0 for u in updates), updates
    u = np.fromfile(dump, dtype=np.float64)
    assert np.isfinite(u).all()


MORE_CTESTS = [  # (problem directory, deck of its add_test line, {extern path the problem opens: committed copy under tests/golden}, slow)
    ("HydroHighMach", "HighMach.in", {"highmach_reference.txt": "highmach_reference.txt"}, False),
    ("HydroLeblanc", "leblanc.in", {"ppm1d/leblanc.dat": "ppm1d_leblanc.dat"}, False),
    ("HydroSMS", "SlowMovingShock.in", {}, False),
    ("HydroShuOsher", "ShuOsher.in", {"ShuOsher_athena_3c_hllc_vl.txt": "ShuOsher_athena_3c_hllc_vl.txt"}, False),
    ("HydroVacuum", "vacuum.in", {"Toro/e1rpex.out": "Toro_e1rpex.out"}, False),
    ("HydroWave", "hydro_wave.in", {}, False),
    ("RadSuOlson", "SuOlson.in", {}, False),
    ("RadhydroShock", "radshock_dimensionless.in", {"LowrieEdwards/shock.txt": "LowrieEdwards_shock.txt"}, False),
    ("RadMarshakCGS", "MarshakCGS.in", {"SuOlson/100pt_tau10p0.dat": "SuOlson_100pt_tau10p0.dat"}, False),
    ("RadPulse", "RadPulse.in", {}, False),
    ("RadhydroBB", "RadhydroBB.in", {"Doppler-spectrum/exact_flux_density.csv": "Doppler_exact_flux_density.csv"}, False),
    ("RadhydroPulse", "RadhydroPulse.in", {}, False),
    ("RadhydroPulseDyn", "RadhydroPulseDyn.in", {}, False),
    ("RadhydroPulseGrey", "RadhydroPulseGrey.in", {}, False),
    ("RadhydroPulseMGint", "RadhydroPulse.in", {}, False),  # opacity exponents that follow T: the problem's hook compiled into the multigroup kernel
    # one-cell problems of ~1e5 steps: bound by launch latency, about four minutes each — run with QK_SLOW_TESTS=1 (both exit 0: 2.4e-7 / 3.3e-5
    # against their 1e-5 / ... criteria on the builder's box)
    ("RadMatterCoupling", "energyexchange.in", {}, True),
    ("RadMatterCouplingRSLA", "MatterEnergyExchangeRSLA.in", {}, True),
]


@pytest.mark.parametrize("name,deck,extern,slow", MORE_CTESTS, ids=[c[0] for c in MORE_CTESTS])
def test_unmodified_reference_ctest_exits_zero(tmp_path, name, deck, extern, slow):
    """The reference's ctest of that name: its problem file compiled unchanged against the host mirror, run from the reference's own deck in a
    working directory laid out like the reference's tests/ (data tables under ../extern), and held to the pass criterion coded in the problem
    file — exit status 0.  (The CPU oracle meets the same criteria in tests/test_oracle_known_answers.py; this is the GPU path through the C++17
    host, hooks compiled as device code.)"""
    if slow and os.environ.get("QK_SLOW_TESTS") != "1":
        pytest.skip("about four minutes of launch latency; QK_SLOW_TESTS=1 runs it")
    cwd = extern_tree(tmp_path, extern)
    rc, out = run([exe(f"ref_{name}"), os.path.join(HOST, "decks", deck), "plotfile_interval=-1", "checkpoint_interval=-1"], cwd)
    assert rc == 0, out[-2500:]


def conservation_error(out, component):
    """relative conservation error the executable prints for that component after evolve (None: the line is not there)"""
    m = re.search(r"Initial " + re.escape(component) + r" = \S+\s+absolute conservation error = \S+\s+relative conservation error = (\S+)", out)
    return float(m.group(1)) if m else None


CLOUDY_TABLE = os.path.join(ROOT, "tests", "golden", "isrf_1000Go_grains.h5")


def test_cooling_problem_unchanged_with_the_tabulated_cooling_source(tmp_path):
    """src/problems/Cooling, unchanged: amrex::TableData (the random phases of its initial perturbation, filled on the host, copied to the device,
    read by the initial-condition kernel), its custom boundary pair (extrapolation below, Dirichlet above) and the Strang-split cooling source.
    The reference's deck names a Grackle table (an empty submodule of the reference tree) and no cooling.cooling_table_type — which the reference's
    own constructor answers with "Invalid cooling table type!" (src/QuokkaSimulation.hpp:362-374); so does this host.  Grackle tables are refused
    by name; with the Cloudy table of the cloudy_cooling_tools (the reference's extern/cooling/isrf_1000Go_grains.h5) the problem runs WITH its
    cooling source: substeps are reported from every source call and the gas loses thermal energy that the run without cooling keeps."""
    deck = os.path.join(HOST, "decks", "Cooling.in")
    common = ["max_timesteps=20", "plotfile_interval=-1", "checkpoint_interval=-1"]
    rc, out = run([exe("ref_Cooling"), deck] + common, str(tmp_path))
    assert rc != 0 and "Invalid cooling table type!" in out, out[-1500:]
    rc, out = run([exe("ref_Cooling"), deck, "cooling.cooling_table_type=grackle"] + common, str(tmp_path))
    assert rc != 0 and "Grackle-like cooling" in out and "not built" in out, out[-1500:]
    cloudy = ["cooling.cooling_table_type=cloudy_cooling_tools", f"cooling.hdf5_data_file={CLOUDY_TABLE}"]
    rc, cooled = run([exe("ref_Cooling"), deck] + cloudy + common, str(tmp_path))
    assert rc == 0 and "Performance figure-of-merit" in cooled, cooled[-2000:]
    assert cooled.count("cooling substeps (per cell)") >= 40  # two source calls per step
    rc, adiabatic = run([exe("ref_Cooling"), deck, "cooling.enabled=0"] + common, str(tmp_path))
    assert rc == 0 and "cooling substeps" not in adiabatic, adiabatic[-2000:]
    e_cool, e_adia = conservation_error(cooled, "gasInternalEnergy"), conservation_error(adiabatic, "gasInternalEnergy")
    assert e_cool is not None and e_adia is not None and e_cool < e_adia - 1.0e-6, (e_cool, e_adia)  # (signed: final minus initial)


def test_shockcloud_unchanged_with_its_cloudy_table(tmp_path):
    """src/problems/ShockCloud, unchanged, on the geometry and parameters of the reference's tests/ShockCloud_32.in: a shocked wind overruns a cold
    cloud; both cool through the Cloudy table (read by the library's own HDF5 reader).  The problem calls the table functions from host code
    (problem_main: cloud temperature, cooling length), from its own kernels (ErrorEst, derived variables) and through the Strang source; NSCBC
    inflow / outflow in x, mass scalars for cloud and wind material, the cloud-tracking frame shift after every step (volume integrals,
    simulationMetadata_).  No pass criterion in the reference (a regression test there): exit 0, a cooling report from every source call, the cloud's
    partial density conserved to rounding while wind material enters through the inflow boundary."""
    cwd = str(tmp_path)
    os.symlink(CLOUDY_TABLE, os.path.join(cwd, "isrf_1000Go_grains.h5"))  # the deck names ./isrf_1000Go_grains.h5, as the reference's
    rc, out = run([exe("ref_ShockCloud"), os.path.join(HOST, "decks", "shockcloud_32.in"), "max_timesteps=60"], cwd)
    assert rc == 0 and "Performance figure-of-merit" in out, out[-2500:]
    assert "Reading cloudy-cooling-tools tables" in out and out.count("cooling substeps (per cell)") >= 120
    cloud = conservation_error(out, "component7")  # scalar 1: the cloud's partial density (cloud.cpp:106-108)
    assert cloud is not None and abs(cloud) < 1.0e-12, cloud
    assert conservation_error(out, "gasDensity") > 1.0e-3  # the wind blows in
    m = re.search(r"retries=(\d+)", out)
    assert m and int(m.group(1)) <= 4


def test_randomblast_unchanged_without_its_grackle_cooling(tmp_path):
    """src/problems/RandomBlast, unchanged.  Its deck cools with Grackle's tables, which are not in the reference tree: that deck is refused by name.
    With cooling off the problem is supernova injection into a periodic box — Poisson-distributed explosions drawn on the host
    (amrex::RandomPoisson / Random after InitRandom(42)), their positions handed to the injection kernel through pinned-memory
    amrex::TableData<Real, 1>, deposited through a Wendland kernel in computeAfterLevelAdvance.  Mass is conserved exactly (ejecta mass 0) and the
    energy in the box grows by exactly what the problem reports as injected."""
    deck = os.path.join(HOST, "decks", "randomblast_hydro.in")
    rc, out = run([exe("ref_RandomBlast"), deck, "cooling.enabled=1", "cooling.cooling_table_type=grackle", "cooling.hdf5_data_file=none.h5", "max_timesteps=3"], str(tmp_path))
    assert rc != 0 and "Grackle-like cooling" in out, out[-1500:]
    rc, out = run([exe("ref_RandomBlast"), deck, "max_timesteps=40"], str(tmp_path))
    assert rc == 0, out[-2500:]
    injected = float(re.search(r"Cumulative injected energy = (\S+)", out).group(1))
    assert injected > 0 and injected % 1.0e51 == 0  # whole supernovae of 1e51 erg
    m = re.search(r"Initial gasEnergy = (\S+)\s+absolute conservation error = (\S+)", out)
    assert abs(float(m.group(2)) / injected - 1.0) < 1.0e-9, (m.group(2), injected)
    assert conservation_error(out, "gasDensity") == 0.0


def test_cxx_host_children_beside_the_far_boxes_and_the_rollback_are_bit_identical(tmp_path):
    """The speculative coarse step of the C++ host (host/quokka_amr.hpp: AmrDriver::speculativeSplit / snapshotAbove / deferredVerdicts,
    QuokkaSimulation::advanceLevelBegin / advanceLevelDeferred — the schedule quokka_amd/amr_simulation.py introduced in round 5): stage 2 of the
    level-0 boxes no child reads on a second stream while the children advance, every verdict read once at the end of the coarse step, a bad one
    rolled back (states, times, step counters, the grids of a regrid in between) and redone in the ordinary order.  The reference's unchanged
    HydroBlast3D on blast_amr_maxlev2.in scaled down (64^3 in 32^3 boxes, blocking factor 8), 14 coarse steps: the ordinary order, the
    overlapped one, the overlapped one with the verdict of coarse step 5 forced bad — the same zone-update counts per level and the level-0
    state equal in every bit; exact and carried form of the RK2 average."""
    import re
    deck = os.path.join(HOST, "decks", "blast_amr_maxlev2.in")
    common = [deck, "amr.n_cell=64 64 64", "amr.max_grid_size=32", "amr.blocking_factor=8", "max_timesteps=14"]
    for form in ([], ["hydro.rk2_carry_rhs=1"]):
        results = []
        for tag, extra in (("plain", ["qk.overlap_children=0"]), ("overlap", ["qk.overlap_children=1"]),
                           ("rollback", ["qk.overlap_children=1", "qk.force_speculation_failure_at=5"])):
            dump = str(tmp_path / f"{tag}{len(form)}.bin")
            rc, out = run([exe("ref_HydroBlast3D")] + common + form + extra + [f"qk.dump_state={dump}"], str(tmp_path))
            assert "Energy conservation is OK." in out, out[-2500:]
            zones = re.findall(r"Zone-updates on level (\d): (\d+)", out)
            m = re.search(r"speculative coarse steps: overlapped=(\d+) rolled_back=(\d+)", out)
            results.append((np.fromfile(dump, dtype=np.float64), zones, (int(m.group(1)), int(m.group(2))) if m else (0, 0), open(dump + ".meta").read().split()[:3]))
        plain, over, roll = results
        assert len(plain[1]) == 3 and int(plain[1][2][1]) > 0  # a level 2 exists and was advanced
        assert plain[2] == (0, 0) and over[2][0] >= 10 and over[2][1] <= 2, (plain[2], over[2])
        assert roll[2][1] == over[2][1] + 1, (over[2], roll[2])
        for other in (over, roll):
            assert other[1] == plain[1] and other[3] == plain[3], (plain[1], other[1], plain[3], other[3])
            assert np.array_equal(plain[0], other[0])
