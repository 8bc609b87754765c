"""The slope limiters MC and minmod of csrc/qk_device.hpp as the hydro kernels instantiate them, through qk_arith_evaluate, against the expression as the
reference writes it — 0.5 * (sgn(a) + sgn(b)) * min(...) with the integer sgn — evaluated in numpy float64, bit for bit.  The device forms the factor
0.5 * (sgn(a) + sgn(b)) without integers (halfSgnSum: the operands' sign bits under the bits of 0.5, zeroed where the operand is zero, one exact add);
it must be the same double for every pair of operands, the zeros, subnormals and infinities included, or the sign of a zero slope changes.

The minimum is the one-instruction form (smin: v_min_f64), which drops a NaN operand — inf + (-inf) inside MC — where std::min would hand it on: np.fmin
here.  Where the expression itself is not a number (0 * inf: slopes +inf and -inf) both sides must say so; the payload of a NaN is not compared."""
import itertools

import numpy as np
import pytest

from quokka_amd import capi
from test_arith_primitives_gpu import bits, ev, mant

pytestmark = pytest.mark.gpu
NPAIR = 1 << 16


def sgn(v):
    return (0.0 < v).astype(np.int64) - (v < 0.0).astype(np.int64)


def mc_as_written(a, b):
    with np.errstate(all="ignore"):
        return 0.5 * (sgn(a) + sgn(b)).astype(np.float64) * np.fmin(0.5 * np.abs(a + b), np.fmin(2.0 * np.abs(a), 2.0 * np.abs(b)))


def minmod_as_written(a, b):
    with np.errstate(all="ignore"):
        return 0.5 * (sgn(a) + sgn(b)).astype(np.float64) * np.fmin(np.abs(a), np.abs(b))


LIMITERS = [(capi.ARITH_MC, mc_as_written, "MC"), (capi.ARITH_MINMOD, minmod_as_written, "minmod")]


def assert_same_bits(got, want, a, b, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where the expression has none, or the reverse", a[np.isnan(got) != nan][:4].tolist(), b[np.isnan(got) != nan][:4].tolist())
    bad = (bits(got) != bits(want)) & ~nan
    assert not bad.any(), (what, int(bad.sum()), a[bad][:4].tolist(), b[bad][:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
    # the signed zeros, explicitly: a slope of -0 where the reference has +0 is a different bit pattern of the state
    zero = (want == 0.0)
    assert np.array_equal(np.signbit(got[zero]), np.signbit(want[zero])), (what, "sign of a zero slope")


@pytest.fixture(scope="module")
def random_pairs():
    """2^16 pairs with random signs over +-500 binades, all 52 significand bits random; a quarter of them within four binades of each other (the
    three arguments of MC's minimum then compete) and a sixteenth with an operand replaced by a zero of either sign"""
    r = np.random.default_rng(11)
    sign = lambda: np.where(r.random(NPAIR) < 0.5, -1.0, 1.0)
    ea = r.integers(-500, 501, NPAIR)
    eb = np.where(r.random(NPAIR) < 0.25, np.clip(ea + r.integers(-4, 5, NPAIR), -500, 500), r.integers(-500, 501, NPAIR))
    a, b = sign() * np.ldexp(mant(r, NPAIR), ea), sign() * np.ldexp(mant(r, NPAIR), eb)
    z = r.random(NPAIR)
    a = np.where(z < 1 / 32, np.where(r.random(NPAIR) < 0.5, -0.0, 0.0), a)
    b = np.where((z >= 1 / 32) & (z < 1 / 16), np.where(r.random(NPAIR) < 0.5, -0.0, 0.0), b)
    return a, b


@pytest.mark.parametrize("what,as_written,name", LIMITERS, ids=[l[2] for l in LIMITERS])
def test_random_pairs_over_a_thousand_binades(ctx, random_pairs, what, as_written, name):
    a, b = random_pairs
    want = as_written(a, b)
    assert (want > 0).mean() > 0.15 and (want < 0).mean() > 0.15 and (want == 0).mean() > 0.3  # (every value of the factor occurs)
    assert_same_bits(ev(ctx, what, a, b), want, a, b, name)
    assert_same_bits(ev(ctx, what, b, a), as_written(b, a), b, a, name + " (operands swapped)")


@pytest.mark.parametrize("what,as_written,name", LIMITERS, ids=[l[2] for l in LIMITERS])
def test_zeros_subnormals_units_and_infinities_crossed(ctx, what, as_written, name):
    tiny = 5e-324
    special = [0.0, -0.0, tiny, -tiny, 1.0, -1.0, np.inf, -np.inf]
    at = lambda x: next(k for k, s in enumerate(special) if s == x and np.signbit(s) == np.signbit(x))  # (0.0 == -0.0: list.index cannot tell them apart)
    pairs = np.array(list(itertools.product(special, special)))
    a, b = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    want = as_written(a, b)
    got = ev(ctx, what, a, b)
    assert_same_bits(got, want, a, b, name)
    # what the expression gives there, spelled out: a zero operand makes the slope a zero with the sign of the OTHER operand's sign factor ...
    for x, y, neg in [(0.0, -1.0, True), (-0.0, -1.0, True), (-1.0, 0.0, True), (0.0, 1.0, False), (-0.0, 1.0, False), (-0.0, -0.0, False), (0.0, -0.0, False),
                      (-0.0, -tiny, True), (-tiny, tiny, False), (-1.0, 1.0, False)]:
        i = at(x) * len(special) + at(y)
        assert (a[i], b[i]) == (x, y) and np.signbit(a[i]) == np.signbit(x) and np.signbit(b[i]) == np.signbit(y)
        assert got[i] == 0.0 and bool(np.signbit(got[i])) == neg, (name, x, y, got[i])
    # ... equal signs keep the sign, subnormal operands count as nonzero, and slopes of +inf and -inf give 0 * inf
    i = at(-tiny) * len(special) + at(-1.0)
    assert got[i] < 0.0
    i = at(np.inf) * len(special) + at(-np.inf)
    assert np.isnan(got[i]) and np.isnan(want[i])
