"""The hand-rolled FP64 division and square root of csrc/qk_device.hpp (recipOf / divBy / divN / recipExact / sqrtN) through qk_arith_evaluate,
against numpy's `/` and sqrt — IEEE correctly rounded on the CPU — bit for bit: every "same bits as the oracle" of the hydro and radiation kernels
rests on them.  Inside the range the header comment of qk_device.hpp states they must give the bits of IEEE; outside it only what the comment
documents (NaN for a zero, infinite or subnormal denominator; a zero quotient of either sign)."""
import ctypes as C

import numpy as np
import pytest
import torch

from quokka_amd import capi

pytestmark = pytest.mark.gpu
NPAIR = 1 << 20
NWALK = 1 << 16

# the range of qk_device.hpp's comment: measured on an MI355X by the walks below (no difference from IEEE down to 2^-1004 and up to the end of the
# walk at 2^1020; the first one at 2^-1012, for the divisions and for sqrtN alike), then shrunk by 16 binades.  Bits of IEEE for
#   2^LO <= |d|, |n|, |n / d| <= 2^HI;   sqrtN: x >= 2^LO
LO, HI = -996, 1004
WALK_TOP = 1020


def ev(ctx, what, a=None, b=None):
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(ctx.device)
    da, db = dev(a), dev(b)
    n = (a if a is not None else b).size
    out = torch.empty(n, dtype=torch.float64, device=ctx.device)
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    ctx.check(ctx.L.qk_arith_evaluate(ctx.h, ctx.stream(), int(what), n, ptr(da), ptr(db), ptr(out)), "qk_arith_evaluate")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def mant(r, n):
    """random significands in [1, 2) with all 52 bits random"""
    return 1.0 + r.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52


def assert_divisions_equal_ieee(ctx, a, b, what=""):
    with np.errstate(all="ignore"):
        want = a / b
        want_r = 1.0 / b
    assert np.isfinite(want).all() and np.isfinite(want_r).all(), what
    for fn in (capi.ARITH_DIVBY_RECIPOF, capi.ARITH_DIVN):
        got = ev(ctx, fn, a, b)
        bad = bits(got) != bits(want)
        assert not bad.any(), (what, fn, int(bad.sum()), a[bad][:3].tolist(), b[bad][:3].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())
    got = ev(ctx, capi.ARITH_RECIPEXACT, None, b)
    bad = bits(got) != bits(want_r)
    assert not bad.any(), (what, "recipExact", int(bad.sum()), b[bad][:3].tolist(), got[bad][:3].tolist(), want_r[bad][:3].tolist())


def test_random_operands_over_a_thousand_binades(ctx):
    r = np.random.default_rng(1)
    eb = r.integers(-500, 501, NPAIR)
    eq = r.integers(-500, 501, NPAIR)
    ea = np.clip(eb + eq, -500, 500)
    sign = lambda: np.where(r.random(NPAIR) < 0.5, -1.0, 1.0)
    a, b = sign() * np.ldexp(mant(r, NPAIR), ea), sign() * np.ldexp(mant(r, NPAIR), eb)
    assert_divisions_equal_ieee(ctx, a, b, "random")
    assert_divisions_equal_ieee(ctx, b.copy(), b, "a == b")


def test_denominators_next_to_powers_of_two(ctx):
    """1 +- k ulp and 2^m (1 +- k ulp): the reciprocal is as far from a representable number as it gets"""
    r = np.random.default_rng(2)
    k = r.integers(0, 2048, NPAIR)
    up = r.random(NPAIR) < 0.5
    one = np.where(up, 1.0 + k * 2.0 ** -52, 1.0 - k * 2.0 ** -53)
    m = np.where(r.random(NPAIR) < 0.5, 0, r.integers(-500, 501, NPAIR))
    b = np.ldexp(one, m)
    a = np.ldexp(mant(r, NPAIR), np.clip(m + r.integers(-40, 41, NPAIR), -500, 500)) * np.where(r.random(NPAIR) < 0.5, -1.0, 1.0)
    assert_divisions_equal_ieee(ctx, a, b, "1 +- k ulp")


def test_quotients_next_to_a_rounding_midpoint(ctx):
    """numerators q_mid * b rounded to the doubles on either side, q_mid the midpoint of two adjacent doubles: the quotient lies within an ulp of
    the point where round-to-nearest changes its answer"""
    r = np.random.default_rng(3)
    L = np.longdouble
    assert np.finfo(L).nmant >= 63, "needs the 64-bit significand of x87 extended precision"
    n = NPAIR // 4
    q = np.ldexp(mant(r, n), r.integers(-60, 61, n))
    b = np.ldexp(mant(r, n), r.integers(-200, 201, n))
    q_mid = q.astype(L) + np.spacing(q).astype(L) / 2
    p = (q_mid * b.astype(L)).astype(np.float64)
    cands = [np.nextafter(p, -np.inf), p, np.nextafter(p, np.inf), np.nextafter(np.nextafter(p, np.inf), np.inf)]
    a = np.concatenate(cands)
    bb = np.concatenate([b] * 4)
    with np.errstate(all="ignore"):
        want = a / bb
    # the construction does what it says: both neighbours of the midpoint are hit
    assert (want[:n] <= q).mean() > 0.3 and (want[2 * n:3 * n] > q).mean() > 0.3
    assert_divisions_equal_ieee(ctx, a, bb * np.where(r.random(4 * n) < 0.5, -1.0, 1.0), "midpoints")


def test_zero_numerators_give_a_zero_of_either_sign(ctx):
    """documented: a zero quotient may come out as +0 where IEEE gives -0"""
    r = np.random.default_rng(4)
    b = np.ldexp(mant(r, 4096), r.integers(-500, 501, 4096)) * np.where(r.random(4096) < 0.5, -1.0, 1.0)
    for zero in (0.0, -0.0):
        a = np.full(4096, zero)
        for fn in (capi.ARITH_DIVBY_RECIPOF, capi.ARITH_DIVN):
            got = ev(ctx, fn, a, b)
            assert (got == 0.0).all()
        if zero == 0.0:
            pos = b > 0
            assert not np.signbit(ev(ctx, capi.ARITH_DIVN, a, b)[pos]).any()  # (+0 / positive: +0 as IEEE)


def test_magnitudes_of_the_matter_radiation_exchange_in_cgs(ctx):
    """what the exchange kernel divides by in CGS: c c_hat, c^2, c E_r down to E_r = 1e-30, tau from 1e-12, c_v = rho k_B / (mu (gamma - 1)) at
    rho = 1e-27 — far from the O(1) states of test_hydro_ops_gpu.py"""
    r = np.random.default_rng(5)
    c = 2.99792458e10
    n = NPAIR // 4
    dens = [np.where(r.random(n) < 0.5, c * (0.1 * c), c * c),
            c * 10.0 ** r.uniform(-30.0, 20.0, n),
            10.0 ** r.uniform(-12.0, 12.0, n),
            10.0 ** r.uniform(-27.0, -3.0, n) * 1.380649e-16 / (1.6605390666e-24 * (5.0 / 3.0 - 1.0))]
    b = np.concatenate(dens)
    a = b * mant(r, 4 * n) * 10.0 ** r.uniform(-60.0, 60.0, 4 * n) * np.where(r.random(4 * n) < 0.5, -1.0, 1.0)
    assert_divisions_equal_ieee(ctx, a, b, "CGS")


def test_square_roots(ctx):
    r = np.random.default_rng(6)
    x = np.ldexp(mant(r, NPAIR), r.integers(-700, 1000, NPAIR))
    got = ev(ctx, capi.ARITH_SQRTN, x)
    assert np.array_equal(bits(got), bits(np.sqrt(x)))
    # perfect squares and their two neighbours, over the even binades
    n = NPAIR // 4
    root = r.integers(1, 1 << 26, n).astype(np.float64)
    sq = np.ldexp(root * root, 2 * r.integers(-300, 301, n))
    x = np.concatenate([np.nextafter(sq, 0.0), sq, np.nextafter(sq, np.inf)])
    got = ev(ctx, capi.ARITH_SQRTN, x)
    assert np.array_equal(bits(got), bits(np.sqrt(x)))
    assert np.array_equal(got[n:2 * n] ** 2, sq)
    special = np.array([0.0, -0.0, np.inf])
    assert np.array_equal(bits(ev(ctx, capi.ARITH_SQRTN, special)), bits(special))
    neg = -np.ldexp(mant(r, 4096), r.integers(-700, 1000, 4096))
    assert np.isnan(ev(ctx, capi.ARITH_SQRTN, np.concatenate([neg, [-np.inf]]))).all()


def first_difference(exps, differs):
    """the first exponent of an outward walk at which any sample differs (None: none does)"""
    for e, d in zip(exps, differs):
        if d:
            return int(e)
    return None


def walk_division(ctx, r, exps, which):
    """2^16 random pairs per exponent of the walk: `which` = 'den' (d at 2^e, quotient in [1/2, 2)), 'quo' (d in [1, 2), quotient at 2^e) or
    'num' (numerator at 2^e, quotient in [1/2, 2)): per exponent, whether any of divBy(recipOf), divN, recipExact differs from IEEE"""
    out = []
    for e in exps:
        if which == "quo":
            b = mant(r, NWALK)
            a = np.ldexp(mant(r, NWALK), int(e))
        else:
            b = np.ldexp(mant(r, NWALK), int(e))
            a = np.ldexp(mant(r, NWALK), int(e))
        with np.errstate(all="ignore"):
            want, want_r = a / b, 1.0 / b
        d = (bits(ev(ctx, capi.ARITH_DIVBY_RECIPOF, a, b)) != bits(want)).any() or (bits(ev(ctx, capi.ARITH_DIVN, a, b)) != bits(want)).any()
        if which == "den":
            d = d or (bits(ev(ctx, capi.ARITH_RECIPEXACT, None, b)) != bits(want_r)).any()
        out.append(bool(d))
    return out


def test_measured_range_of_the_divisions_and_what_holds_outside(ctx):
    """walks the exponent of the denominator (with it the numerator's) and of the quotient outward in steps of 8 and records the first one at which any
    of 2^16 samples differs from IEEE; the header comment of qk_device.hpp carries the measured range, shrunk by 16 binades — asserted here as
    bit equality inside and as a measured edge that lies outside"""
    r = np.random.default_rng(7)
    down = lambda start: list(range(start, -1075, -8))
    up = lambda start: list(range(start, WALK_TOP + 1, 8))
    # denominator and numerator together at 2^e, quotient O(1): below, the residual fma(-d, q, n) ~ 2^-104 n goes subnormal first
    e_dn = first_difference(down(-900), walk_division(ctx, r, down(-900), "den"))
    e_up = first_difference(up(900), walk_division(ctx, r, up(900), "den"))
    q_dn = first_difference(down(-900), walk_division(ctx, r, down(-900), "quo"))
    q_up = first_difference(up(900), walk_division(ctx, r, up(900), "quo"))
    print(f"first exponent (steps of 8) at which a division differs from IEEE: denominator = numerator scale 2^{e_dn} / 2^{e_up}, "
          f"quotient (denominator in [1, 2)) 2^{q_dn} / 2^{q_up}")
    assert e_dn is None or e_dn < LO - 8
    assert e_up is None and q_up is None  # (nothing up to 2^WALK_TOP)
    assert q_dn is None or q_dn < LO - 8
    # inside the stated range: denominators, numerators and quotients over all of it
    eb = r.integers(LO, HI + 1, NPAIR)
    eq = r.integers(LO + 1, HI, NPAIR)  # (the significands move the quotient by up to a binade)
    keep = (eb + eq >= LO) & (eb + eq <= HI)
    assert keep.mean() > 0.5
    eb, eq = eb[keep], eq[keep]
    a, b = np.ldexp(mant(r, eb.size), eb + eq), np.ldexp(mant(r, eb.size), eb)
    with np.errstate(all="ignore"):
        want = a / b
    assert (np.abs(want) >= 2.0 ** LO).all() and (np.abs(want) <= 2.0 ** HI).all()
    for fn in (capi.ARITH_DIVBY_RECIPOF, capi.ARITH_DIVN):
        assert np.array_equal(bits(ev(ctx, fn, a, b)), bits(want)), fn
    # outside, what the comment documents: a zero or infinite denominator gives NaN (a subnormal one NaN or an inexact quotient: not asserted),
    # an infinite numerator gives NaN
    bad_den = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -2.0 ** -1040, 2.0 ** -1023])
    num = np.array([1.0, -3.0, 2.5, 1e300, 1e-300, 7.0, 1.0])
    print("n / d for d =", bad_den.tolist(), ":", ev(ctx, capi.ARITH_DIVN, num, bad_den).tolist())
    for fn in (capi.ARITH_DIVBY_RECIPOF, capi.ARITH_DIVN):
        assert np.isnan(ev(ctx, fn, num, bad_den)[:4]).all(), fn
        assert np.isnan(ev(ctx, fn, np.array([np.inf, -np.inf]), np.array([3.0, 8.987551787368176e20]))).all(), fn


def test_measured_range_of_the_square_root(ctx):
    """sqrtN leaves out the range scaling hipcc's sqrt applies below 2^-767: the walk records where its bits first leave IEEE"""
    r = np.random.default_rng(8)
    exps = list(range(-700, -1075, -8))
    differs = []
    for e in exps:
        x = np.ldexp(mant(r, NWALK), int(e))
        differs.append(bool((bits(ev(ctx, capi.ARITH_SQRTN, x)) != bits(np.sqrt(x))).any()))
    first = first_difference(exps, differs)
    print(f"first exponent (steps of 8) at which sqrtN differs from IEEE: 2^{first}")
    assert first is None or first < LO - 8
    x = np.ldexp(mant(r, NPAIR), r.integers(LO, 1024, NPAIR))
    assert np.array_equal(bits(ev(ctx, capi.ARITH_SQRTN, x)), bits(np.sqrt(x)))
