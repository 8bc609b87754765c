// ORACLE — TEST INFRASTRUCTURE ONLY (see grid.hpp header).
//
// portable_libm.hpp: the oracle's own log10 and x^(-1/2) from correctly rounded operations only, so that a GPU kernel built over the same recipe
// can be held to the oracle in every bit (cooling.hpp routes its per-cell libm calls through a hook that selects glibc, the default, or these).
// Written from the recipe, not from the library's header (quokka_amd/csrc/qk_portable_libm.hpp); tests/test_cooling_reference.py holds the two
// equal in every bit.  The recipe:
//   log10 x:  frexp gives x = f 2^e with f in [1/2, 1); f below sqrt(1/2) is doubled (e one less), so f in [sqrt(1/2), sqrt(2)).
//             t = (f - 1) / (f + 1), w = t t, ln f = 2 t + 2 t (w S), S = sum_{n=1..12} w^(n-1) / (2 n + 1) by Horner from the last term.
//             result = e H + (e L + ln f / ln 10) with H + L = log10(2), H = 0x1.34413509fp-2.
//   x^(-1/2): y = 1 / sqrt(x), then one Newton step y + (y / 2) (1 - x y y) with the residual from two fma: p = x y, p' = fma(x, y, -p),
//             residual = fma(-p, y, 1) - p' y; y returned as it is when it is 0, inf or NaN.
#ifndef ORACLE_PORTABLE_LIBM_HPP_
#define ORACLE_PORTABLE_LIBM_HPP_

#include <cmath>
#include <limits>

namespace oracle::portable_libm
{

inline auto log10_portable(const double x) -> double
{
	if (std::isnan(x) || x < 0.0) {
		return std::numeric_limits<double>::quiet_NaN();
	}
	if (x == 0.0) {
		return -std::numeric_limits<double>::infinity();
	}
	if (std::isinf(x)) {
		return std::numeric_limits<double>::infinity();
	}
	int e = 0;
	double f = std::frexp(x, &e);
	if (f < 0.70710678118654752440) {
		f = f * 2.0;
		e = e - 1;
	}
	const double t = (f - 1.0) / (f + 1.0);
	const double w = t * t;
	double S = 1.0 / 25.0;
	for (int odd = 23; odd >= 3; odd -= 2) {
		S = S * w + 1.0 / static_cast<double>(odd);
	}
	const double t2 = 2.0 * t;
	const double ln_f = t2 + t2 * (w * S);
	const double H = 0x1.34413509fp-2;
	const double L = 0x1.e7fbcc47c4acdp-40;
	const double inv_ln10 = 0.43429448190325182765;
	const double de = static_cast<double>(e);
	return de * H + (de * L + ln_f * inv_ln10);
}

inline auto rsqrt_portable(const double x) -> double
{
	const double y = 1.0 / std::sqrt(x);
	if (std::isnan(y) || std::isinf(y) || y <= 0.0) {
		return y;
	}
	const double p = x * y;			  // ~ sqrt(x)
	const double p_err = std::fma(x, y, -p);  // x y = p + p_err exactly
	const double res = std::fma(-p, y, 1.0) - p_err * y; // 1 - x y y
	return std::fma(0.5 * y, res, y);
}

} // namespace oracle::portable_libm

#endif // ORACLE_PORTABLE_LIBM_HPP_
