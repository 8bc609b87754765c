"""The tabulated-cooling kernels held to the oracle cell by cell, bit for bit (tests/test_cooling_reference.py is the CPU side, with the argument
for the method; tests/cooling_reference.py holds the sets).  The kernels' portable instantiation (qk_cooling_set_libm) calls a log10 and an
x^(-1/2) the CPU reproduces in every bit, so EVERYTHING else — interpolation, Algorithm 748, the Heun ladder, the persistent-lane queue, the
counters, the hand-rolled quotients — must equal the oracle exactly: every comparison through that instantiation is equality of bits (NaN = NaN).
The production instantiation differs from it in the two libm calls only; they are measured here against mpmath (device log10 and pow(x, -1/2):
see test_device_libm_is_within_one_ulp), and tests/test_cooling_gpu.py keeps covering its integration statistically.  cool::quo, the quotient
primitive, is compared with IEEE division through the constructions of tests/test_arith_primitives_gpu.py."""
import mpmath
import numpy as np
import pytest

import cooling_reference as R
from cooling_reference import GAMMA, MAX_SUBSTEPS, T_FLOOR
from quokka_amd.cooling import COOLING_LENGTH, EGAS_FROM_TGAS, INV_SQRT, LOG10, MMW, NET_HEATING, QUO, TGAS_FROM_EGAS
from test_arith_primitives_gpu import HI, LO, NPAIR, bits, mant

pytestmark = pytest.mark.gpu
mpmath.mp.prec = 200


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, int((np.isnan(got) != nan).sum()))
    bad = bits(got[~nan]) != bits(want[~nan])
    assert not bad.any(), (what, int(bad.sum()), np.where(bad)[0][:5].tolist(), got[~nan][bad][:3].tolist(), want[~nan][bad][:3].tolist())


@pytest.fixture(scope="module")
def small(ctx):
    """a level of one cell: the handle for qk_cooling_evaluate"""
    return R.GpuLevel(ctx, 1, [([0, 0, 0], [0, 0, 0])])


def check_source(ctx, ndim, boxes, U, dt, U_want, ns_want, calls=1):
    """the source on a level of `boxes` holding the cell list U: bit-equal state, exact counters, NaN ghost cells, density and momentum untouched"""
    lev = R.GpuLevel(ctx, ndim, boxes)
    lev.put(U)
    before, ghosts = lev.get()
    assert ghosts and np.array_equal(before, U, equal_nan=True)
    for _ in range(calls):
        ok, mx, sm = lev.source(dt)
    got, ghosts = lev.get()
    assert ghosts
    assert np.array_equal(got[:4], U[:4])
    assert_same_bits(got[4], U_want[4], "E_gas")
    assert_same_bits(got[5], U_want[5], "E_int")
    assert (mx, sm) == (int(ns_want.max()), int(ns_want.sum()))
    assert ok == bool(ns_want.max() < MAX_SUBSTEPS)
    return got


def test_device_and_host_portable_libm_are_equal_in_every_bit(small):
    r = np.random.default_rng(2)
    x = np.concatenate([r.integers(0, 1 << 63, 1 << 20, dtype=np.int64).view(np.float64), 10.0 ** np.arange(-307, 309), r.uniform(0.0, 5e-308, 4096),
                        10 ** r.uniform(-12.0, 10.0, 1 << 17), [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 5e-324, 2.0 ** -1022, np.finfo(float).max, 1.0, np.sqrt(0.5)]])
    orc = R.oracle()
    assert_same_bits(small.evaluate(LOG10, x, x), orc.portable_libm(0, x), "log10")
    assert_same_bits(small.evaluate(INV_SQRT, x, x), orc.portable_libm(1, x), "x^(-1/2)")


def test_per_cell_functions_equal_the_oracle_in_every_bit(small):
    orc = R.oracle()
    rho, _, T = R.wide_ism(200000, 3)
    E = orc.evaluate(orc.EGAS_FROM_TGAS, rho, T, GAMMA)
    assert_same_bits(small.evaluate(EGAS_FROM_TGAS, rho, T), E, "E(T)")
    assert_same_bits(small.evaluate(NET_HEATING, rho, T), orc.evaluate(orc.NET_HEATING, rho, T, GAMMA), "net heating")
    for what_g, what_o in ((TGAS_FROM_EGAS, orc.TGAS_FROM_EGAS), (MMW, orc.MMW), (COOLING_LENGTH, orc.COOLING_LENGTH)):
        assert_same_bits(small.evaluate(what_g, rho, E), orc.evaluate(what_o, rho, E, GAMMA), what_g)
    # a NaN energy is a NaN temperature on both sides (the empty bracket), a negative one the table's lower end
    E[:64], E[64:128] = np.nan, -E[64:128]
    assert_same_bits(small.evaluate(TGAS_FROM_EGAS, rho, E), orc.evaluate(orc.TGAS_FROM_EGAS, rho, E, GAMMA), "T(E), NaN and negative E")


def test_source_on_the_sweep_set(ctx):
    s = R.sweep_set()
    check_source(ctx, 3, R.uniform_boxes([16] * 3, 8), s.U, s.dt, s.U1, s.ns)


def test_source_on_the_failure_set_returns_false_and_keeps_the_partial_energy(ctx):
    f = R.failure_set()
    failed = f.ns >= MAX_SUBSTEPS
    assert failed.sum() > 0
    lev = R.GpuLevel(ctx, 3, R.uniform_boxes([16] * 3, 8))
    lev.put(f.U)
    ok, mx, sm = lev.source(f.dt)
    assert ok is False and mx == MAX_SUBSTEPS and sm == int(f.ns.sum())
    got, ghosts = lev.get()
    assert ghosts and np.array_equal(got[:4], f.U[:4])
    assert_same_bits(got[4], f.U1[4])
    assert_same_bits(got[5], f.U1[5])
    # the failed cells hold the energy after 2000 substeps, not the one they started with, and as many cells changed as the oracle changed
    assert (got[5][failed] != f.U[5][failed]).all()
    assert int((got[5] != f.U[5]).sum()) == int((f.U1[5] != f.U[5]).sum())


@pytest.mark.parametrize("name", ["on_emin", "on_emax", "below_emin", "negative_eint", "thin", "dense", "dense_cold", "nan_energy"])
def test_targeted_cells(ctx, name):
    res, must = R.targeted()[name]
    for b in must:
        assert res.has(b).all(), (name, b)  # (the oracle went where the case aims)
    got = check_source(ctx, 1, [([0, 0, 0], [R.NT - 1, 0, 0])], res.U, res.dt, res.U1, res.ns)
    if name == "nan_energy":
        assert np.isnan(got[4]).all() and np.isnan(got[5]).all() and (res.ns == MAX_SUBSTEPS).all()


GEOMETRIES = {
    "one cell": (1, [([0, 0, 0], [0, 0, 0])]),
    "63 cells": (1, [([0, 0, 0], [62, 0, 0])]),
    "65 cells": (1, [([0, 0, 0], [64, 0, 0])]),
    "24 x 7": (2, [([0, 0, 0], [23, 6, 0])]),
    "24 x 7 in two boxes": (2, R.split_boxes([24, 7, 1], [[16], [], []])),
    "12 + 4 along each axis": (3, R.split_boxes([16] * 3, [[12]] * 3)),  # 8 boxes of 12^3 ... 4^3: the indices outside a smaller box are skipped
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_queue_geometry(ctx, name):
    ndim, boxes = GEOMETRIES[name]
    s = R.sweep_set()
    n = sum(int(np.prod([hi[d] - lo[d] + 1 for d in range(3)])) for lo, hi in boxes)
    first = int(np.argmax(s.ns)) if n == 1 else 0  # (the single cell: the one that takes the most substeps)
    sl = slice(first, first + n)
    check_source(ctx, ndim, boxes, s.U[:, sl], s.dt, s.U1[:, sl], s.ns[sl])


def test_more_cells_than_lanes(ctx):
    L = R.large_set()
    assert L.ns.size > 2048 * 256
    check_source(ctx, 3, [([0, 0, 0], [83, 83, 83])], L.U, L.dt, L.U1, L.ns)


@pytest.mark.parametrize("layout", ["one wave", "scattered"])
def test_expensive_cells_in_one_wave_and_scattered(ctx, layout):
    heavy, light = R.heavy_and_light()
    U = np.empty((6, 4096))
    where = np.arange(64) if layout == "one wave" else np.arange(64) * 64 + 37
    mask = np.zeros(4096, dtype=bool)
    mask[where] = True
    U[:, mask], U[:, ~mask] = heavy, light
    res = R.run_oracle(U, R.DT_SWEEP)
    assert (res.ns[mask] >= 800).all() and (res.ns[~mask] == 1).all()
    check_source(ctx, 3, [([0, 0, 0], [15, 15, 15])], U, res.dt, res.U1, res.ns)


def test_two_calls_in_a_row_on_the_same_level(ctx):
    """the queue word of the level is reset before every launch: the second call takes every cell again"""
    s = R.sweep_set()
    second = R.run_oracle(np.array(s.U1), s.dt)
    assert second.ns.sum() != s.ns.sum()
    check_source(ctx, 3, R.uniform_boxes([16] * 3, 8), s.U, s.dt, second.U1, second.ns, calls=2)


def test_device_libm_is_within_one_ulp(small):
    """the production instantiation's two libm calls against mpmath over the arguments the algorithm uses (8000 each of n_H 1e-8 ... 1e8,
    T 1 ... 1e10, epsilon 1e-12 ... 1e6): at most one ulp from the correctly rounded value — what the docstring of tests/test_cooling_gpu.py relies
    on.  Measured on an MI355X: log10 at most 1 ulp from the correctly rounded value (0.62 ulps from the exact one), 0.15 ... 0.29 % of the
    results differ from glibc's; pow(x, -0.5) at most 1 ulp from the correctly rounded value but up to 1.24 ulps from the exact one, and 25 % of
    the results differ from glibc's (profiles/cooling_pins/device_libm.txt)"""
    r = np.random.default_rng(5)
    n = 8000
    worst = []
    for name, x in (("n_H", 10 ** r.uniform(-8.0, 8.0, n)), ("T", 10 ** r.uniform(0.0, 10.0, n)), ("epsilon", 10 ** r.uniform(-12.0, 6.0, n))):
        for code, fn, host in ((LOG10, mpmath.log10, np.log10), (INV_SQRT, lambda v: 1 / mpmath.sqrt(v), lambda v: np.power(v, -0.5))):
            got = small.evaluate(code, x, x, portable=False)
            exact = [fn(mpmath.mpf(float(v))) for v in x]
            rounded = np.array([float(e) for e in exact])  # (mpmath rounds to nearest)
            from_rounded = np.abs(got - rounded) / np.spacing(rounded)
            from_exact = np.array([float(abs(mpmath.mpf(float(g)) - e) / mpmath.mpf(float(np.spacing(abs(float(e)))))) for g, e in zip(got, exact)])
            print(f"device {'log10' if code == LOG10 else 'pow(x, -0.5)'} over {name}: max {from_rounded.max():.0f} ulps from the correctly rounded value, "
                  f"{from_exact.max():.3f} ulps from the exact one; {np.mean(got != host(x)):.3%} of the results differ from glibc's")
            worst.append((name, code, float(from_rounded.max())))
    for name, code, w in worst:
        assert w <= 1.0, (name, code, w)


# ---------------------------------------------------------------- cool::quo = over(n, denOf(d)) against IEEE division
def quo(small, a, b):
    return small.evaluate(QUO, a, b)


def test_quo_random_operands_and_neighbours_of_rounding_midpoints(small):
    r = np.random.default_rng(1)
    eb, eq = r.integers(-500, 501, NPAIR), r.integers(-500, 501, NPAIR)
    ea = np.clip(eb + eq, -500, 500)
    sign = lambda: np.where(r.random(NPAIR) < 0.5, -1.0, 1.0)
    a, b = sign() * np.ldexp(mant(r, NPAIR), ea), sign() * np.ldexp(mant(r, NPAIR), eb)
    assert_same_bits(quo(small, a, b), a / b, "random")
    # numerators on either side of q_mid * b, q_mid the midpoint of two adjacent doubles (tests/test_arith_primitives_gpu.py)
    L = np.longdouble
    assert np.finfo(L).nmant >= 63
    n = NPAIR // 4
    q = np.ldexp(mant(r, n), r.integers(-60, 61, n))
    b = np.ldexp(mant(r, n), r.integers(-200, 201, n))
    p = ((q.astype(L) + np.spacing(q).astype(L) / 2) * b.astype(L)).astype(np.float64)
    a = np.concatenate([np.nextafter(p, -np.inf), p, np.nextafter(p, np.inf), np.nextafter(np.nextafter(p, np.inf), np.inf)])
    bb = np.concatenate([b] * 4) * np.where(r.random(4 * n) < 0.5, -1.0, 1.0)
    assert_same_bits(quo(small, a, bb), a / bb, "midpoints")
    # what Algorithm 748 divides: function values up to 1e9 K over their differences, temperatures over temperature differences down to 1e-5 T
    f = 10 ** r.uniform(-8.0, 9.0, NPAIR) * sign()
    d = f * 10 ** r.uniform(-12.0, 1.0, NPAIR) * sign()
    assert_same_bits(quo(small, f, d), f / d, "function values")


def test_quo_over_the_exponent_ladder_and_what_holds_outside_it(small):
    """bits of IEEE for 2^-996 <= |d|, |n|, |n / d| <= 2^1004 (the range csrc/qk_device.hpp documents for recipOf / divBy, the same recipe); outside
    it what the header comment of csrc/qk_cooling_device.hpp states, asserted as observed on an MI355X"""
    r = np.random.default_rng(7)
    eb = r.integers(LO, HI + 1, NPAIR)
    eq = r.integers(LO + 1, HI, NPAIR)
    keep = (eb + eq >= LO) & (eb + eq <= HI)
    eb, eq = eb[keep], eq[keep]
    a, b = np.ldexp(mant(r, eb.size), eb + eq), np.ldexp(mant(r, eb.size), eb)
    assert_same_bits(quo(small, a, b), a / b, "ladder")
    big = np.finfo(float).max
    with np.errstate(all="ignore"):
        # DBL_MAX, the sentinel of guardedQuotient, as a numerator: the guard lets it through to quo only over |d| >= 1 — the quotient of IEEE
        d = np.concatenate([np.ldexp(mant(r, 4096), r.integers(0, 900, 4096)), [1.0, 2.0, 3.0, 1.0e9]]) * np.where(r.random(4100) < 0.5, -1.0, 1.0)
        n = np.full(d.size, big)
        assert_same_bits(quo(small, n, d), n / d, "DBL_MAX numerators")
        # a quotient that overflows, an infinite numerator: NaN where IEEE gives +-inf
        got = quo(small, np.array([big, -big, np.inf, -np.inf, 1.0e300]), np.array([0.5, 0.25, 3.0, 3.0, 1.0e-300]))
        print("overflowing quotients and infinite numerators:", got.tolist())
        assert np.isnan(got).all()
        # a zero, infinite or NaN denominator, a NaN numerator: NaN (IEEE: +-inf, 0, NaN, NaN)
        got = quo(small, np.array([1.0, -3.0, 2.5, 7.0, 1.0, np.nan, 0.0]), np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0, 0.0]))
        print("zero / infinite / NaN denominators:", got.tolist())
        assert np.isnan(got).all()
    # a zero numerator over a normal denominator: a zero (of either sign)
    assert (quo(small, np.array([0.0, -0.0, 0.0]), np.array([3.0, 3.0, -1.0e-5])) == 0.0).all()
