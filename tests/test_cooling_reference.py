"""The CPU side of the cell-by-cell pin of the tabulated cooling (tests/test_cooling_cells_gpu.py is the GPU side; tests/cooling_reference.py holds
what they share).  The cooling kernels have a second instantiation over a log10 and an x^(-1/2) made of correctly rounded operations
(csrc/qk_portable_libm.hpp), which the oracle reproduces through its libm hook (oracle/portable_libm.hpp, written independently).  Here:
  * the two copies of the portable functions are equal in every bit, and an honest log10 / x^(-1/2).  Measured against mpmath over the arguments the
    algorithm uses (30000 each of n_H 1e-8 ... 1e8, T 1 ... 1e10, epsilon 1e-12 ... 1e6): log10 at most 2.57 ulps from the exact value (n_H 2.57,
    T 2.31, epsilon 2.12; glibc's: 0.59), the inverse square root at most 0.50 ulps from x^(-1/2) and never more than one ulp from glibc's
    pow(x, -0.5);
  * the host side of csrc/qk_cooling_device.hpp under the portable policy equals the oracle under the portable hook bit for bit;
  * the portable oracle is a member of the family the glibc oracle spans under a one-ulp perturbation of its input.  Measured on the sweep set
    (4096 wide cells, dt = 2e3 yr): cooled energies more than 1e-12 apart in 33.8 % of the cells, max 1.8e-4, relative L1 8.8e-8; the yardstick
    (glibc oracle, E one ulp up): 43.3 %, max 2.0e-4, L1 9.1e-8.  ComputeTgasFromEgas on 60000 wide cells: 0.37 % (max 6.6e-6, L1 1.2e-11) against
    3.3 % (max 8.7e-6, L1 7.2e-11);
  * the sets the GPU tests run have the failure shares and the branch coverage the tests rely on."""
import mpmath
import numpy as np
import pytest

import cooling_reference as R
from cooling_reference import GAMMA, MAX_SUBSTEPS, T_FLOOR

mpmath.mp.prec = 200


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return R.HostCheck(tmp_path_factory.mktemp("hostcheck"))


def libm_arguments(n, seed=5):
    """what the algorithm passes to log10 (n_H, T) and to x^(-1/2) (epsilon)"""
    r = np.random.default_rng(seed)
    return 10 ** r.uniform(-8.0, 8.0, n), 10 ** r.uniform(0.0, 10.0, n), 10 ** r.uniform(-12.0, 6.0, n)


def ulps_from(got, exact):
    """|got - exact| in units of the spacing of doubles at the exact value (exact: mpmath numbers)"""
    return np.array([float(abs(mpmath.mpf(float(g)) - e) / mpmath.mpf(float(np.spacing(abs(float(e)))))) for g, e in zip(got, exact)])


def test_the_two_copies_of_the_portable_libm_are_equal_in_every_bit(host):
    r = np.random.default_rng(1)
    n = 1 << 20
    bits = r.integers(0, 1 << 63, n, dtype=np.int64)  # every positive double, subnormals, infinities and NaNs with it
    orc = R.oracle()
    axis_ends = np.concatenate([10.0 ** orc.prepared(0)[[0, -1]], [10.0, 1.0e9], orc.prepared(1)[[0, -1]]])
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 5e-324, 2.0 ** -1074, 2.0 ** -1022, np.nextafter(2.0 ** -1022, 0.0), np.finfo(float).max, 1.0,
                        np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), np.sqrt(0.5), np.nextafter(np.sqrt(0.5), 0.0), np.nextafter(np.sqrt(0.5), 1.0), np.sqrt(2.0)])
    x = np.concatenate([bits.view(np.float64), -bits[:4096].view(np.float64), 10.0 ** np.arange(-307, 309), r.uniform(0.0, 5e-308, 4096), axis_ends, special,
                        *libm_arguments(1 << 17)])
    assert x.size >= 1000000 and np.isnan(x).any() and (x == 0).any() and np.isinf(x).any() and ((x > 0) & (x < 2.0 ** -1022)).any()
    for which, code in ((0, host.LOG10), (1, host.INV_SQRT)):
        lib, own = host.evaluate(code, x, x, portable=True), orc.portable_libm(which, x)
        assert np.array_equal(np.isnan(lib), np.isnan(own))
        ok = ~np.isnan(own)
        assert np.array_equal(lib[ok].view(np.int64), own[ok].view(np.int64)), which
    # what they return at the ends: log10(0) = -inf, log10(inf) = inf, NaN for a negative or NaN argument; exact powers of two are exact multiples
    lg = orc.portable_libm(0, np.array([0.0, -0.0, np.inf, -1.0, np.nan, 1.0]))
    assert lg[0] == -np.inf and lg[1] == -np.inf and lg[2] == np.inf and np.isnan(lg[3:5]).all() and lg[5] == 0.0
    rs = orc.portable_libm(1, np.array([0.0, np.inf, 4.0, -1.0]))
    assert rs[0] == np.inf and rs[1] == 0.0 and rs[2] == 0.5 and np.isnan(rs[3])


def test_the_portable_libm_is_an_honest_log10_and_inverse_square_root():
    orc = R.oracle()
    n = 30000
    n_H, T, eps = libm_arguments(n)
    worst = {}
    for name, x in (("n_H", n_H), ("T", T), ("epsilon", eps)):
        exact = [mpmath.log10(mpmath.mpf(float(v))) for v in x]
        worst["log10 " + name] = ulps_from(orc.portable_libm(0, x), exact).max()
        worst["glibc log10 " + name] = ulps_from(np.log10(x), exact).max()
        exact = [1 / mpmath.sqrt(mpmath.mpf(float(v))) for v in x]
        worst["rsqrt " + name] = ulps_from(orc.portable_libm(1, x), exact).max()
    print({k: round(float(v), 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= (1.0 if k.startswith("rsqrt") else 4.0), (k, v)
    # against pow(x, -0.5) as glibc rounds it: at most one ulp
    got, want = orc.portable_libm(1, eps), np.power(eps, -0.5)
    assert np.max(np.abs(got - want) / np.spacing(want)) <= 1.0


def test_host_side_under_the_portable_policy_equals_the_portable_oracle_bit_for_bit(host):
    orc = R.oracle()
    n = 60000
    r = np.random.default_rng(7)
    rho, T = 10 ** r.uniform(-27.5, -19.5, n), 10 ** r.uniform(0.8, 9.2, n)  # the wide sample: beyond the table's rows at both ends
    E = orc.evaluate(orc.EGAS_FROM_TGAS, rho, T, GAMMA)
    assert np.array_equal(host.evaluate(1, rho, T), E)
    assert np.array_equal(host.evaluate(4, rho, T), orc.evaluate(orc.NET_HEATING, rho, T, GAMMA))
    for what in (orc.TGAS_FROM_EGAS, orc.MMW, orc.COOLING_LENGTH):
        assert np.array_equal(host.evaluate(what, rho, E), orc.evaluate(what, rho, E, GAMMA), equal_nan=True), what
    # the portable policy is a different function: the comparison above is not one of glibc with itself
    assert not np.array_equal(E, R.oracle("glibc").evaluate(orc.EGAS_FROM_TGAS, rho, T, GAMMA))
    m = 6000
    U = np.zeros((6, m))
    U[0], U[4], U[5] = rho[:m], E[:m], E[:m]
    dt = 1.0e4 * R.YEAR
    U1, ns = orc.compute_cooling(U, GAMMA, dt, T_FLOOR)
    Eh, nh = host.cool(rho[:m], E[:m], dt)
    assert np.array_equal(nh, ns) and ns.max() > 100
    assert np.array_equal(E[:m] + (Eh - E[:m]), U1[5])
    # and the targeted cells (E_int as the kernel forms it: E_gas - E_kin)
    for name, (res, _bits) in R.targeted().items():
        Eint = res.U[4] - (res.U[1] ** 2 + res.U[2] ** 2 + res.U[3] ** 2) / (2.0 * res.U[0])
        Eh, nh = host.cool(res.U[0], Eint, res.dt)
        assert np.array_equal(nh, res.ns), name
        assert np.array_equal(res.U[4] + (Eh - Eint), res.U1[4], equal_nan=True), name


def disagreement(a, b):
    """(share of cells more than 1e-12 apart, largest relative difference, relative L1)"""
    err = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return float(np.mean(err > 1.0e-12)), float(err.max()), float(np.abs(a - b).sum() / np.abs(b).sum())


def test_portable_and_glibc_oracles_are_members_of_one_family():
    """the statement under test is the reference's algorithm with a log10 correct to the last bits — the portable oracle must differ from the glibc
    oracle no more than the glibc oracle differs from itself with the energy one ulp up (x 3, + 1e-4: the margin tests/test_cooling_gpu.py allows)"""
    og, op = R.oracle("glibc"), R.oracle()
    s = R.sweep_set()
    U_g, ns_g = og.compute_cooling(s.U, GAMMA, s.dt, T_FLOOR)
    U_up = np.array(s.U)
    U_up[4] = np.nextafter(U_up[4], np.inf)
    U_y, ns_y = og.compute_cooling(U_up, GAMMA, s.dt, T_FLOOR)
    got, yard = disagreement(s.U1[5], U_g[5]), disagreement(U_y[5], U_g[5])
    print("cooled energy, portable vs glibc (share > 1e-12, max, L1):", got, "; glibc vs glibc(+1 ulp):", yard)
    for g, y in zip(got, yard):
        assert g <= 3.0 * y + 1.0e-4, (got, yard)
    assert abs(int(s.ns.sum()) - int(ns_g.sum())) <= max(3 * abs(int(ns_y.sum()) - int(ns_g.sum())), 1.0e-4 * int(ns_g.sum()))
    n = 60000
    r = np.random.default_rng(7)
    rho, T = 10 ** r.uniform(-27.5, -19.5, n), 10 ** r.uniform(0.8, 9.2, n)
    E = og.evaluate(og.EGAS_FROM_TGAS, rho, T, GAMMA)
    T_g = og.evaluate(og.TGAS_FROM_EGAS, rho, E, GAMMA)
    got = disagreement(op.evaluate(op.TGAS_FROM_EGAS, rho, E, GAMMA), T_g)
    yard = disagreement(og.evaluate(og.TGAS_FROM_EGAS, rho, np.nextafter(E, np.inf), GAMMA), T_g)
    print("T(E), portable vs glibc:", got, "; glibc vs glibc(+1 ulp):", yard)
    for g, y in zip(got, yard):
        assert g <= 3.0 * y + 1.0e-4, (got, yard)


def test_failure_shares_of_the_sets_the_gpu_tests_run():
    s, f = R.sweep_set(), R.failure_set()
    assert int((s.ns >= MAX_SUBSTEPS).sum()) == 0 and s.ns.max() > 1000 and 100 < s.ns.mean() < 200
    share = float(np.mean(f.ns >= MAX_SUBSTEPS))
    assert 0.01 <= share <= 0.05, share
    assert np.array_equal(f.ns >= MAX_SUBSTEPS, f.has("max_substeps"))  # (every failure of this set is the step limit, none the seven refusals)
    L = R.large_set()
    assert L.ns.size == 84 ** 3 > 2048 * 256 and L.ns.max() < MAX_SUBSTEPS and 3.0 < L.ns.mean() < 5.0
    heavy, light = R.heavy_and_light()
    assert heavy.shape == (6, 64) and light.shape == (6, 4032)


def test_branch_coverage_of_the_sets_the_gpu_tests_run():
    orc = R.oracle()
    sets = R.gpu_sets()
    count = {name: sum(int(res.has(name).sum()) for _, res in sets) for name in orc.BRANCHES if name != "eta_floor"}
    depth = np.concatenate([res.rec["deepest_retry"] for _, res in sets])
    count.update({"retry 1": int((depth == 1).sum()), "retry 2": int((depth == 2).sum()), "retry >= 3": int((depth >= 3).sum())})
    print(count)
    for name, c in count.items():
        assert c >= 8, (name, c)
    # each targeted case goes where it was aimed, in every cell
    for name, (res, bits) in R.targeted().items():
        for b in bits:
            assert res.has(b).all(), (name, b)
    t = R.targeted()
    assert (t["nan_energy"][0].ns == MAX_SUBSTEPS).all() and (t["nan_energy"][0].rec["failed_rhs"] == 7).all() and (t["nan_energy"][0].rec["refused"] == 7).all()
    assert not t["thin"][0].has("nh_high").any() and not t["dense"][0].has("nh_low").any()
    # the random sets alone reach Algorithm 748's fall-backs, both ends of the energy range and retries one and two deep
    s = R.sweep_set()
    for name in ("emin", "emax", "parabola", "secant", "bisect", "coincide"):
        assert s.has(name).sum() >= 8, name
    # not reached by any cell with a finite energy (2 x 4096 wide cells, 592704 narrow cells, the targeted cells): a failed right-hand side, an
    # empty bracket, seven refusals.  A change that makes one reachable should be noticed — and given a test.
    # Nor by any cell at all: a step-size factor below 0.1 on the third or a later attempt of a step (the lower end of the clamp [0.1, 0.3]) — also
    # absent from 5 x 65536 wide cells at dt = 2e3 ... 2e7 yr.  Mutants of that clamp (0.1 -> 0.2, `k == 1` -> `k >= 1`) therefore pass every test.
    for name, res in sets + [("large", R.large_set())]:
        assert not res.has("eta_floor").any(), name
        finite = np.isfinite(res.U[4])
        assert not (res.rec["failed_rhs"][finite] > 0).any(), name
        for b in ("empty_bracket", "seven_refusals"):
            assert not res.has(b)[finite].any(), (name, b)
