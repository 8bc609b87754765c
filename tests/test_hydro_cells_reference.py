"""The array-level hydro entries of the oracle (oracle_capi.cpp: orc_hydro_*) held to the defining statements without a GPU, and the population
condition of every case tests/test_hydro_cells_gpu.py runs: a targeted branch holds at least 1 % of the samples and at least 256 of them.

Riemann fans: on a supersonic face the flux is the physical flux of the upwind state in every bit; with equal sides it is the physical flux
within a bound counted from the star formula; a mirrored face gives the mirrored flux in every bit wherever the reference's statements are
themselves symmetric (the two that are not are named in test_mirror_symmetry).  Cell operators: against an np.longdouble restatement of
hydro_system.hpp, per-cell bound (roundings + 1) x eps x the largest intermediate magnitude; flags and counts exactly."""
from dataclasses import replace

import numpy as np
import pytest

import hydro_cells_reference as H

EPS = H.EPS


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def run_flux_case(oracle, c, L=None, R=None, prim=None):
    L0, R0, prim0, vlo, vhi = c.build()
    L, R, prim = (L0 if L is None else L), (R0 if R is None else R), (prim0 if prim is None else prim)
    F, V = oracle.hydro_face_fluxes(c.eos.oracle_traits(c.ndim, c.reconstruct_eint, c.nscalars), c.riemann, c.d, L, R, prim, vlo, vhi, 1, c.K_visc)
    return L, R, prim, F, V


# ------------------------------------------------------------------------------------------------ populations
@pytest.mark.parametrize("case", H.flux_cases(), ids=lambda c: c.id)
def test_flux_case_populations(oracle, case):
    L, R, prim, F, V = run_flux_case(oracle, case)
    cl = case.classify(L, R, prim)
    print(f"{case.id}: {L[0].size} faces; " + ", ".join(f"{k} {H.population(m)[0]}" for k, m in cl.items() if k != "S"))
    for k in case.targets:
        assert H.holds(cl[k]), (case.id, k, H.population(cl[k]))
    # the classifier's own mass-flux sign against the oracle's (it only counts: a handful of last-ulp ties would do no harm)
    assert ((F[0] >= 0) == cl["mass_flux_ge_0"]).mean() > 0.999
    assert np.isfinite(F).all() and np.isfinite(V).all(), "the flux comparison holds valid states only"


CELL_CASES = H.CELL_EOS
NCELL = int(np.prod(H.box_shape(*H.CELL_BOX)))


def cell_populations(units, gamma):
    """name -> (classes, targeted) of every cell-operator case of one EOS"""
    eos = H.Eos(H.UNITS[units], gamma)
    out = {}
    for floor_zero in (False, True):
        U, rf, Tf = H.limits_cells(eos, NCELL, 31, H.NSCAL, H.NMSCAL, floor_zero)
        out[f"limits-floor{'0' if floor_zero else '+'}"] = (H.classify_limits(eos, U, rf, Tf, H.NSCAL, H.NMSCAL), H.limits_targets(eos, floor_zero))
    out["dual-energy"] = (H.classify_dual_energy(H.dual_energy_cells(eos, NCELL, 32)), H.DUAL_TARGETS)
    out["signal"] = (H.classify_signal(eos, H.signal_cells(eos, NCELL, 33)), H.signal_targets(eos))
    U, rhs, dt = H.predict_cells(eos, NCELL, 34, H.NSCAL, H.NMSCAL)
    out["predict"] = (H.classify_predict(U, rhs, dt, H.NMSCAL), H.PREDICT_TARGETS)
    return out


@pytest.mark.parametrize("units,gamma", CELL_CASES)
def test_cell_case_populations(units, gamma):
    for name, (c, want) in cell_populations(units, gamma).items():
        print(f"{units}-g{gamma:.3g}-{name}: {NCELL} cells; " + ", ".join(f"{k} {H.population(m)[0]}" for k, m in c.items()))
        H.assert_populations(f"{units}-g{gamma:.3g}-{name}", c, want)


# ------------------------------------------------------------------------------------------------ the three structural checks of HLLC
FAN_CASES = [c for c in H.flux_cases() if c.riemann == H.HLLC and c.family == "b"]


@pytest.mark.parametrize("case", FAN_CASES, ids=lambda c: c.id)
def test_supersonic_fan_is_the_upwind_physical_flux_in_every_bit(oracle, case):
    """S_L > 0: F = F(left state); S_R < 0: F = F(right state) (HLLC.hpp:142-150), formed with the expression of HLLC.hpp:132-133 in float64.
    K_visc = 0 (the viscosity term is not part of the statement).  Faces are chosen by the classifier's wave speeds, at least 1e-9 (|u| + c_s)
    away from zero so that a last-ulp difference cannot move a face into the star fan."""
    case = replace(case, K_visc=0.0)
    L, R, prim, F, V = run_flux_case(oracle, case)
    cl = case.classify(L, R, prim)
    S_L, _, S_R = cl["S"]
    AN = H.axes(case.ndim, case.d)[0]
    tol = 1e-9 * (np.abs(L[1 + AN]) + np.abs(S_L - L[1 + AN]))
    for name, mask, q, other, left in (("S_L > 0", S_L > tol, L, R, True), ("S_R < 0", S_R < -tol, R, L, False)):
        assert H.holds(mask), name
        Fp, Vp = H.physical_flux(case.eos, q, other, case.reconstruct_eint, case.ndim, case.d, left)
        assert np.array_equal(bits(F[:, mask]), bits(Fp[:, mask])), name
        assert np.array_equal(bits(V[mask]), bits(Vp[mask])), name


EQUAL_CASES = [c for c in H.flux_cases() if c.riemann == H.HLLC and c.family == "a"]


@pytest.mark.parametrize("case", EQUAL_CASES, ids=lambda c: c.id)
def test_equal_sides_give_the_physical_flux_within_the_rounding_of_the_star_formula(oracle, case):
    """L == R and du = dw = 0: exactly, S* = u, P_LR = P and F*_K = F_K for any S_K.  In float64 (HLLC.hpp:97-136):
      S*: rho u, S_K - u, their product, on both sides (6), the difference (1), rho (S_K - u) on both sides (2), the difference (1; the two
          terms have the same sign: no cancellation), the quotient (1); theta (P_R - P_L) = 0 is exact: 11 roundings, so S* = u (1 + 11 eps);
      S* enters F*_K twice, as the factor of (S_K U - F_K) and in the denominator S_K - S*: 22;
      F*_K itself: rho u (1), S_K U (1), u U and P D and their sum (3), S_K U - F_K (1), the product with S* (1), S_K P_LR (1), times D* (1),
          the sum (1), S_K - S* (1), the quotient (1): 12.
    34 roundings, + 1, times the largest intermediate magnitude of the component,
      M_n = (|S*| (|S_K U_n| + |F_n|) + |S_K D*_n| (P + rho (|S_L - u| + |S_R - u|) |u|)) / |S_K - S*|
    (the second P_LR term, 0.5 phi rho (S_K - u) (S* - u) summed over both sides, vanishes exactly and is carried at its intermediate size)."""
    case = replace(case, K_visc=0.0)
    L, _, _, vlo, vhi = case.build()
    R = L.copy()
    prim = H.prim_velocities(case.ndim, case.d, L.shape[0], 0.0, 0, flat=True)
    _, _, _, F, V = run_flux_case(oracle, case, L, R, prim)
    cl = case.classify(L, R, prim)
    assert H.holds(cl["star_L"]) and H.holds(cl["star_R"])
    S_L, S_s, S_R = cl["S"]
    eos = case.eos
    AN, AV, AW = H.axes(case.ndim, case.d)
    Fp, _ = H.physical_flux(eos, L, R, case.reconstruct_eint, case.ndim, case.d, True)
    rho, u = L[0], L[1 + AN]
    P = H.face_pressure(eos, L, case.reconstruct_eint)
    left = S_s > 0
    S_K = np.where(left, S_L, S_R)
    Pmag = P + rho * (np.abs(S_L - u) + np.abs(S_R - u)) * np.abs(u)
    comps = [(0, rho, 0.0), (1 + AN, rho * u, 1.0), (1 + AV, rho * L[1 + AV], 0.0), (1 + AW, rho * L[1 + AW], 0.0)]
    if not eos.isothermal:
        ke = 0.5 * rho * (L[1] ** 2 + L[2] ** 2 + L[3] ** 2)
        comps += [(4, (P / ((eos.gamma - 1.0) * rho)) * rho + ke, np.abs(S_s)), (5, rho * L[5] if case.reconstruct_eint else L[5], 0.0)]
    comps += [(6 + s, L[6 + s], 0.0) for s in range(case.nscalars)]
    worst = 0.0
    for n, U_n, Dstar in comps:
        M = (np.abs(S_s) * (np.abs(S_K * U_n) + np.abs(Fp[n])) + np.abs(S_K) * Dstar * Pmag) / np.abs(S_K - S_s)
        err = np.abs(F[n].astype(np.longdouble) - Fp[n].astype(np.longdouble)).astype(np.float64)
        bound = 35 * EPS * M
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (case.id, n, float((err / bound).max()))
    print(f"{case.id}: largest |F - F_phys| / bound = {worst:.3f}")


MIRROR_CASES = [c for c in H.flux_cases() if c.riemann == H.HLLC]


def mirrored(case, L, R):
    AN = H.axes(case.ndim, case.d)[0]
    Lm, Rm = R.copy(), L.copy()
    Lm[1 + AN] = -Lm[1 + AN]
    Rm[1 + AN] = -Rm[1 + AN]
    return Lm, Rm


@pytest.mark.parametrize("case", MIRROR_CASES, ids=lambda c: c.id)
def test_mirror_symmetry(oracle, case):
    """Swap the sides and negate the normal velocity (du, dw and div v are unchanged): the mass, energy, transverse-momentum and scalar fluxes and
    the face velocity change sign, the normal-momentum flux does not — in every bit, because additions commute and negation is exact.

    Two statements of the reference are NOT symmetric, and the faces they act on are set apart here, each by its own predicate (no tolerance):
      (1) HLLC.hpp:55, C_tilde_P = 0.5 * (e_L drdp_L + e_R drdp_R + rho_L dedp_L + rho_R dedp_R): a sum of four terms evaluated left to right.
          The mirror image evaluates ((b + a) + d) + c where the original evaluates ((a + b) + c) + d; c = rho_L dedp_L and d = rho_R dedp_R are
          both 1 / (gamma - 1) up to one rounding each, and where they differ the two sums can differ in the last bit.  It reaches the flux
          through cs_tilde only where cs_exp > 0 AND the Roe-average estimate u_tilde -+ cs_tilde is the one min / max selects for S_L or S_R.
          Faces where c == d, or cs_exp <= 0, or the isothermal EOS, are exactly symmetric and asserted so.
      (2) HLLC.hpp:142-150, the fan selection, tests S_L > 0 first and S_R >= 0 last.  Where S* lies outside [S_L, S_R] (possible for
          independent sides: the carbuncle factor theta scales the pressure jump in S* alone) the original and the mirror image select
          different fans.  Faces with S_L < S* < S_R are asserted; the others are counted and printed.
    The ties S* == 0, S_L == 0, S_R == 0 and a zero mass flux are excluded.
    Measured (32 768 faces, family a): statement (1) breaks the symmetry of 173 - 191 of the ~7 650 ordered CGS faces it can act on and of none in
    code units (there boltzmann_constant = 1 makes the first two terms 1e16 times the last two, which the sum then absorbs); statement (2) that
    of 25 - 140 of the 3 400 - 8 700 faces whose waves are not ordered.  Family b and the isothermal cases are symmetric on every face."""
    L, R, prim, F, V = run_flux_case(oracle, case)
    Lm, Rm = mirrored(case, L, R)
    _, _, _, Fm, Vm = run_flux_case(oracle, case, Lm, Rm, prim)
    cl = case.classify(L, R, prim)
    clm = case.classify(Lm, Rm, prim)
    S_L, S_s, S_R = cl["S"]
    AN = H.axes(case.ndim, case.d)[0]
    sign = -np.ones(F.shape[0])
    sign[1 + AN] = 1.0
    want = sign[:, None, None, None] * F
    ordered = (S_L < S_s) & (S_s < S_R) & (S_L != 0) & (S_s != 0) & (S_R != 0) & (F[0] != 0)
    # the classifier's fans of the two images must be mirror images of each other too (a last-ulp disagreement with the oracle on a tie)
    ordered &= (cl["fan_L"] == clm["fan_R"]) & (cl["star_L"] == clm["star_R"]) & (cl["star_R"] == clm["star_L"])
    eos = case.eos
    exact = ordered
    if not eos.isothermal:
        g = eos.gamma
        c_, d_ = L[0] * (1.0 / ((g - 1.0) * L[0])), R[0] * (1.0 / ((g - 1.0) * R[0]))  # rho dedp of either side, as EOS.hpp:246-302 forms them
        exact = ordered & ((c_ == d_) | cl["cs_exp_le_0"])
    same = ((bits(Fm) == bits(want)) | ((Fm == 0.0) & (want == 0.0))).all(axis=0) & (bits(Vm) == bits(-V))
    print(f"{case.id}: {ordered.sum()} of {ordered.size} faces with ordered waves, {(~ordered & ~same).sum()} of the others are not symmetric; "
          f"{exact.sum()} ordered faces free of statement (1), {(ordered & ~exact & ~same).sum()} of the other {(ordered & ~exact).sum()} are not symmetric")
    assert H.holds(exact)
    assert same[exact].all(), (case.id, int((exact & ~same).sum()))


# ------------------------------------------------------------------------------------------------ cell operators against extended precision
def fabs_of(U, ng=2):
    lo, hi = H.CELL_BOX
    return H.embed(U, lo, hi, ng), lo, hi


@pytest.mark.parametrize("units,gamma", CELL_CASES)
@pytest.mark.parametrize("floor_zero", [False, True])
def test_enforce_limits_against_extended_precision(oracle, units, gamma, floor_zero):
    eos = H.Eos(H.UNITS[units], gamma)
    U, rf, Tf = H.limits_cells(eos, NCELL, 31, 3, 2, floor_zero)
    fab, lo, hi = fabs_of(U)
    t = eos.oracle_traits(3, True, 3)
    out = oracle.hydro_enforce_limits(t, fab, lo, hi, 2, rf, Tf, nmscalars=2)
    assert np.isnan(out[:, H.ghost_mask(lo, hi, 2)]).all()
    got = out[H.interior(2)].reshape(U.shape)
    want, bound = H.ld_enforce_limits(eos, U, rf, Tf, 3, 2)
    c = H.classify_limits(eos, U, rf, Tf, 3, 2)
    # momenta are never written; rho is the floor or itself, exactly
    assert np.array_equal(bits(got[1:4]), bits(U[1:4]))
    assert np.array_equal(bits(got[0]), bits(np.where(c["rho_lt_floor"], rf, U[0])))
    # cells whose temperature predicates sit within their own rounding of the floor are ties: left to the bit-for-bit comparison on the GPU
    clear = np.ones(NCELL, dtype=bool)
    if not eos.isothermal:
        rho_new = np.where(U[0] < rf, rf, U[0])
        ok = rho_new > H.DBL_MIN
        safe = np.where(ok, rho_new, 1.0).astype(np.longdouble)
        V = U.astype(np.longdouble)
        Ekin = 0.5 * safe * ((V[1] / safe) ** 2 + (V[2] / safe) ** 2 + (V[3] / safe) ** 2)
        Ef = eos.eint_from_T(safe, np.longdouble(Tf))
        clear = ~ok | ((np.abs((V[4] - Ekin) - Ef) > 32 * EPS * np.maximum(np.abs(V[4]), Ekin)) & (np.abs(V[5] - Ef) > 32 * EPS * np.abs(Ef)))
        assert clear.mean() > 0.99
    for n in (4, 5, 6, 7, 8):
        err = np.abs(got[n].astype(np.longdouble) - want[n])
        fin = np.isfinite(want[n].astype(np.float64)) & clear
        assert (err[fin] <= bound[n][fin]).all(), (n, float((err[fin] / np.maximum(bound[n][fin], 1e-300)).max()))
    # branch choices, exactly: an energy is rewritten exactly where its temperature lies under the floor
    if not eos.isothermal:
        assert np.array_equal((bits(got[4]) != bits(U[4]))[clear], (c["prim_below_aux_below"] | c["prim_below_aux_above"])[clear])
        assert np.array_equal((bits(got[5]) != bits(U[5]))[clear], (c["prim_below_aux_below"] | c["prim_above_aux_below"])[clear])
    if floor_zero:
        assert (got[6:9][:, c["scalars_zeroed"]] == 0.0).all()


@pytest.mark.parametrize("units,gamma", CELL_CASES)
def test_sync_dual_energy_against_extended_precision(oracle, units, gamma):
    eos = H.Eos(H.UNITS[units], gamma)
    U = H.dual_energy_cells(eos, NCELL, 32)
    fab, lo, hi = fabs_of(U)
    out, fatal = oracle.hydro_sync_dual_energy(eos.oracle_traits(3, True, 0), fab, lo, hi, 2)
    assert np.isnan(out[:, H.ghost_mask(lo, hi, 2)]).all()
    got = out[H.interior(2)].reshape(U.shape)
    c = H.classify_dual_energy(U)
    assert np.array_equal(fatal.reshape(-1), c["fatal_rho_le_0"])
    assert np.array_equal(bits(got[:4]), bits(U[:4]))
    assert np.array_equal(bits(got[:, fatal.reshape(-1)]), bits(U[:, fatal.reshape(-1)])), "a fatal cell is left untouched"
    E, Ei, bE, bEi, clear = H.ld_sync_dual_energy(U)
    clear = clear | c["tie"] | c["fatal_rho_le_0"]
    assert clear.mean() > 0.99
    assert (np.abs(got[4] - E)[clear] <= bE[clear]).all() and (np.abs(got[5] - Ei)[clear] <= bEi[clear]).all()
    # the switch, exactly: E is rewritten only on the auxiliary side, and there E_int keeps its bits (the tie E_int,cons == eta E included)
    aux = c["use_auxiliary"] & clear
    assert np.array_equal(bits(got[5][aux]), bits(U[5][aux])) and np.array_equal(bits(got[4][c["use_conserved"] & clear]), bits(U[4][c["use_conserved"] & clear]))


@pytest.mark.parametrize("units,gamma", CELL_CASES)
def test_signal_speed_against_extended_precision(oracle, units, gamma):
    eos = H.Eos(H.UNITS[units], gamma)
    U = H.signal_cells(eos, NCELL, 33)
    fab, lo, hi = fabs_of(U)
    t = eos.oracle_traits(3, True, 0)
    sig = oracle.hydro_max_signal_speed(t, fab, lo, hi, 2).reshape(-1)
    want, bound = H.ld_signal_speed(eos, U, 1)
    c = H.classify_signal(eos, U)
    assert np.array_equal(np.isnan(sig), c["thermal_lt_0"]), "NaN exactly where E - E_kin < 0"
    fin = ~c["thermal_lt_0"]
    assert (np.abs(sig.astype(np.longdouble) - want)[fin] <= bound[fin]).all()
    if not eos.isothermal:
        assert np.isnan(sig[0]) and np.isnan(sig[-1]) and np.isnan(sig[NCELL // 2]) and fin.any()
    # the reductions: a NaN never wins; which = 1 is the maximum of the array above in every bit, which = 0 (another expression for |v|) within the bound
    m1 = oracle.hydro_max_signal_local(t, 1, fab, lo, hi, 2)
    m0 = oracle.hydro_max_signal_local(t, 0, fab, lo, hi, 2)
    assert m1 == sig[fin].max()
    i = int(np.argmax(np.where(fin, sig, -np.inf)))
    assert abs(m0 - m1) <= 2 * bound[fin].max() and m0 >= float(want[i]) - bound[i]


@pytest.mark.parametrize("units,gamma", CELL_CASES)
@pytest.mark.parametrize("nvars", [9, 7])
def test_predict_step_against_extended_precision(oracle, units, gamma, nvars):
    """nvars = 9: all six hydro variables and three scalars, two of them partial densities; nvars = 7: too few for the mass-scalar check to apply"""
    eos = H.Eos(H.UNITS[units], gamma)
    U, rhs, dt = H.predict_cells(eos, NCELL, 34, 3, 2)
    fab, lo, hi = fabs_of(U)
    new0 = np.full_like(fab, -3.25)
    out, flags, count = oracle.hydro_predict_step(eos.oracle_traits(3, True, 3), fab, new0, np.ascontiguousarray(rhs[:nvars]).reshape((nvars,) + H.box_shape(lo, hi)),
                                                  dt, nvars, lo, hi, 2, nmscalars=2)
    assert (out[:, H.ghost_mask(lo, hi, 2)] == -3.25).all() and (out[nvars:] == -3.25).all()
    got = out[H.interior(2)].reshape(U.shape)[:nvars]
    want, bound = H.ld_predict_step(U[:nvars], rhs[:nvars], dt)
    fin = np.isfinite(want.astype(np.float64))
    assert (np.abs(got - want)[fin] <= bound[fin]).all() and np.isnan(got[~fin]).all()
    c = H.classify_predict(U, rhs, dt, 2 if nvars >= 8 else 0)
    assert np.array_equal(flags.reshape(-1) == 0, c["valid"]) and count == int((~c["valid"]).sum())
    assert got[0][c["rho_eq_0"]].size and (got[0][c["rho_eq_0"]] == 0.0).all()


@pytest.mark.parametrize("units,gamma", CELL_CASES)
@pytest.mark.parametrize("ndim,nvars", [(3, 8), (2, 6), (1, 6)])
def test_rhs_and_pdv_against_extended_precision(oracle, units, gamma, ndim, nvars):
    eos = H.Eos(H.UNITS[units], gamma)
    lo = [0, 0, 0]
    hi = [[40, 0, 0], [20, 12, 0], [12, 10, 6]][ndim - 1]
    ncell = int(np.prod(H.box_shape(lo, hi)))
    rng = np.random.default_rng(35)
    dx = [0.37, 1.3, 2.9]
    ns = nvars - 6
    t = eos.oracle_traits(ndim, True, ns)
    U = H._base_cells(eos, np.random.default_rng(36), int(np.prod(H.box_shape(lo, hi, 1, ndim))), ns).reshape((nvars,) + H.box_shape(lo, hi, 1, ndim))
    scale = float(np.median(np.abs(U[4])))
    fluxes = [scale * rng.standard_normal((nvars,) + H.box_shape(lo, hi, 0, ndim, d)) for d in range(ndim)]
    rhs = oracle.hydro_rhs_from_fluxes(t, fluxes, dx, nvars, lo, hi)
    want, bound = H.ld_rhs_from_fluxes(fluxes, dx, ndim)
    assert (np.abs(rhs - want) <= bound).all()
    vscale = float(np.median(np.abs(U[1] / U[0])))
    vels = [vscale * rng.standard_normal(H.box_shape(lo, hi, 0, ndim, d)) for d in range(ndim)]
    redo = (rng.random(H.box_shape(lo, hi)) < 0.4).astype(np.int32)
    assert H.holds(redo.reshape(-1) == 1) or ncell < 25600
    out = oracle.hydro_add_pdv(t, rhs, U, dx, vels, redo, lo, hi, 1)
    assert np.array_equal(bits(np.delete(out, 5, axis=0)), bits(np.delete(rhs, 5, axis=0))), "only the internal-energy component is written"
    want, bound = H.ld_add_pdv(eos, rhs[5], U, vels, redo, dx, ndim, 1)
    assert (np.abs(out[5] - want) <= bound).all(), float((np.abs(out[5] - want) / bound).max())
    # the two formulas differ: flagged cells are not within the bound of the unflagged formula (and the reverse)
    other, _ = H.ld_add_pdv(eos, rhs[5], U, vels, 1 - redo, dx, ndim, 1)
    assert (np.abs(out[5] - other) > bound).mean() > 0.9


# ------------------------------------------------------------------------------------------------ the whole-stage state that takes the fans
def test_fan_state_takes_every_fan_in_every_direction_without_flux_correction(oracle):
    """fan_state as tests/test_hydro_step_gpu.py loads it (32 x 24 x 16, two boxes, periodic): with the piecewise-constant face states of the
    oracle's primitives (those of the order-1 runs; PPM moves a face state by a fraction of the cell-to-cell difference) every fan holds at
    least 1 % of the faces of every direction, gamma law and isothermal (c_s = 1.3); and two advances of dt = 2e-4 on the oracle flag no cell
    (the GPU tests assert 'the test state must not trigger the flux correction')."""
    from oracle.pyoracle import SEDOV
    from test_hydro_ops_gpu import random_state
    N = (32, 24, 16)
    U0 = H.fan_state(random_state(np.random.default_rng(7), (N[2], N[1], N[0])))
    for gamma in (1.4, 1.0):
        eos = H.Eos(H.Units("step", (0, 0), (0, 0), H.M_U, H.K_B, 1.3), gamma)
        t = eos.oracle_traits(3, False, 0)
        prim = oracle.cons_to_prim(t, H.periodic_pad(U0, 2), [-2] * 3, [N[0] + 1, N[1] + 1, N[2] + 1])
        for d in range(3):
            L, R = H.donor_cell_faces(prim, d, 2)
            du, dw, div = H.velocity_differences(prim, 3, d, 2, list(N))
            cl = H.classify_faces(eos, L, R, False, 3, d, du, dw, div, 0.0)
            print(f"fan_state gamma {gamma} direction {d}: " + ", ".join(f"{k} {H.population(cl[k])[0]}" for k in ("fan_L", "star_L", "star_R", "fan_R")) +
                  f" of {L[0].size} faces")
            H.assert_populations(f"fan_state gamma {gamma} direction {d}", cl, ("fan_L", "star_L", "star_R", "fan_R"))
    so = oracle.sim(SEDOV, 3, list(N), [0.0] * 3, [1.0, 0.75, 0.5], [1, 1, 1], max_grid_size=[16, 24, 16])
    ng = so.nghost
    pad = H.periodic_pad(U0, ng)
    fabs = []
    for b in range(so.nboxes):
        lo, hi = so.box(b)
        fabs.append(np.ascontiguousarray(pad[:, lo[2]:hi[2] + 1 + 2 * ng, lo[1]:hi[1] + 1 + 2 * ng, lo[0]:hi[0] + 1 + 2 * ng]))
        so.set_state(np.where(H.ghost_mask(lo, hi, ng), -1.0, fabs[b]), b, 0)
    so.fill_ghosts(0, 0.0)
    for b in range(so.nboxes):
        assert np.array_equal(so.state(b), fabs[b]), "the ghost fill of the periodic domain is the periodic image"
    for _ in range(2):
        assert so.advance_fixed_dt(2.0e-4)
    co = so.counters()
    assert co["fofc1_cells"] == co["fofc2_cells"] == co["retries"] == 0, co
