"""The oracle's matter-radiation exchange (oracle/radiation.hpp AddSourceTermsSingleGroup, through the per-cell entry orc_rad_source_cells) against
things that are not a restatement of it: the defining implicit system solved at 50 digits, the loop bounds of the reference's scheme, and the caps of
the cell generator the GPU tests (test_rad_source_cells_gpu.py) rely on.  No GPU."""
import numpy as np
import pytest

import rad_source_reference as R


def run_oracle(oracle, ts, U, src, dt_radiation, stage):
    return oracle.rad_source_cells(R.oracle_traits(ts), U, src, dt_radiation, stage)


def ulps(a: float, b: float) -> float:
    return abs(a - b) / np.spacing(abs(b)) if b != 0 else (0.0 if a == 0 else np.inf)


@pytest.mark.parametrize("unit", ["cgs", "dimensionless"])
@pytest.mark.parametrize("source", [False, True], ids=["nosrc", "src"])
def test_oracle_solves_the_defining_equations(oracle, unit, source):
    """(3a) beta_order 0, equal constant opacities, stage 2 (dt = (1 - IMEX_a32) dt_radiation): on exit of a converged Newton solve both residuals are
    below r E_tot0 (r = 1e-11); with J00 = 1, J01 = c / c_hat, J10 >= 0, J11 <= -1 (|det| >= 1) that puts E_int within 2 r E_tot0 and
    (c / c_hat) E_r within 3 r E_tot0 of the root to first order — asserted with a factor 2 for the second-order term and rounding.  The flux is
    one division: 4 ulp.
    Measured (2000 cells per unit system and source flag, about 1980 converged with the source on): |E_int - exact| <= 0.94 r E_tot0,
    (c / c_hat) |E_r - exact| <= 1.21 r E_tot0, flux within 2 ulp."""
    import mpmath as mp
    n = 2000
    ts = R.units(unit, beta_order=0)
    ts = R.with_traits(ts, kappaP=ts.kappa_nominal, kappaE=ts.kappa_nominal, kappaF=ts.kappa_nominal)
    dt_rad = R.DT[unit]
    U, src = R.generate_cells(ts, dt_rad, 2, n, seed=7 + int(source), source=source)
    Uo, rec, tot = run_oracle(oracle, ts, U, src, dt_rad, 2)
    ok = ~R.failed_cells(Uo, rec)
    assert ok.sum() >= 0.9 * n and (source or ok.all())
    assert np.array_equal(rec["solves"], np.ones(n, dtype=np.int32))
    dt = R.stage_dt(dt_rad, 2)
    Eint, Er, F = R.exact_exchange(ts, U[:, ok], src[ok], dt)
    cs = ts.c / ts.chat
    E0 = R.eint_from_egas(U)[ok]
    Etot0 = E0 + cs * (U[6, ok] + src[ok] * dt * ts.chat)
    worst = [0.0, 0.0, 0.0]
    bad = []
    for m, i in enumerate(np.flatnonzero(ok)):
        dE = float(abs(mp.mpf(float(Uo[5, i])) - Eint[m])) / (R.RESID_TOL * Etot0[m])
        dR = float(cs * abs(mp.mpf(float(Uo[6, i])) - Er[m])) / (R.RESID_TOL * Etot0[m])
        dF = max(ulps(float(Uo[7 + d, i]), float(F[d][m])) for d in range(3))
        worst = [max(worst[0], dE), max(worst[1], dR), max(worst[2], dF)]
        if dE > 4.0 or dR > 6.0 or dF > 4.0:
            bad.append((int(i), dE, dR, dF, U[:, i].tolist(), float(src[i])))
    print(f"{unit} source {source}: {ok.sum()} converged cells; max |E_int - exact| = {worst[0]:.3g} r E_tot0, "
          f"max (c/c_hat)|E_r - exact| = {worst[1]:.3g} r E_tot0, max flux distance {worst[2]:.3g} ulp")
    assert not bad, bad[:3]
    # the gas energy: E_gas = E_int + E_kin with the momentum the flux update gives, and the total energy of the cell balances the source
    assert np.array_equal(Uo[0], U[0])


@pytest.mark.parametrize("case", R.branch_cases(), ids=lambda c: c.id)
def test_generator_stays_inside_the_caps(oracle, case):
    """(3b) the share of cells in which the oracle reports a failure or returns a non-finite value: 0 with the source off, at most 2 % with it on.
    Measured (4096 cells per case): 0 in all 36 cases with the source off; 0.1 - 0.93 % with it on (the source strengths of the sweep end where
    rad_source_reference.LOG10_SRC says, and why)."""
    n = 4096
    ts = case.traits()
    U, src = R.generate_cells(ts, case.dt, case.stage, n, case.seed, case.source)
    assert np.isfinite(U).all() and np.isfinite(src).all() and (U[0] > 0).all() and (U[6] > 0).all()
    Uo, rec, tot = run_oracle(oracle, ts, U, src, case.dt, case.stage)
    share = R.failed_cells(Uo, rec).mean()
    print(f"{case.id}: failed share {share:.4%}, max Newton {rec['newton_max'].max()}, cells with > 1 solve {np.mean(rec['solves'] > 1):.2%}")
    assert share <= (0.02 if case.source else 0.0)
    assert tot[0] == rec["solves"].sum() and tot[1] == rec["newton"].sum() and tot[2] == rec["newton_max"].max()
    assert tot[4] == rec["fail_newton"].sum() and tot[6] == rec["fail_outer"].sum() and tot[3] == 0 and tot[5] == 0


@pytest.mark.parametrize("beta_order", [0, 1, 2, 3])
def test_failure_semantics_of_a_nan_cell(oracle, beta_order):
    """(3c) a cell whose gas energy is NaN never meets the residual test (a comparison with NaN is false), so every Newton solve runs its
    `for (n = 0; n < 100; ++n)` to the end and is a failure; it is COUNTED as n + 1 = 101 iterations, the counter's convention for every solve
    (source_terms_single_group.hpp:345-346: Add(n + 1), Max(n + 1)).  With a work term (beta_order >= 1) the lagged work is NaN after the first
    pass, none of the four `break` tests of the outer loop holds, and the outer loop runs its 5 passes: 5 solves, 5 Newton failures, 1 outer
    failure.  beta_order 0 leaves the outer loop after one pass."""
    ts = R.units("cgs", beta_order=beta_order)
    U, src = R.generate_cells(ts, 1.0e3, 1, 8, seed=3, source=False)
    U[4, 3] = np.nan
    Uo, rec, tot = run_oracle(oracle, ts, U, src, 1.0e3, 1)
    passes = R.MAX_OUTER if beta_order >= 1 else 1
    assert rec["solves"][3] == passes
    assert rec["newton"][3] == passes * (R.MAX_NEWTON + 1) and rec["newton_max"][3] == R.MAX_NEWTON + 1
    assert rec["fail_newton"][3] == passes
    assert rec["fail_outer"][3] == (1 if beta_order >= 1 else 0)
    others = np.arange(8) != 3
    assert not rec["fail_newton"][others].any() and not rec["fail_outer"][others].any() and np.isfinite(Uo[:, others]).all()
    assert tot[4] == passes and tot[6] == (1 if beta_order >= 1 else 0) and tot[2] == R.MAX_NEWTON + 1
    assert np.isnan(Uo[5, 3]) and Uo[0, 3] == U[0, 3]
