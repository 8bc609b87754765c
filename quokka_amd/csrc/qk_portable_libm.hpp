// qk_portable_libm.hpp — a log10 and an x^(-1/2) made of operations IEEE 754 rounds correctly (frexp, int -> double, + - * /, sqrt, fma), so that the host
// and the device return the SAME BITS for every argument (with -ffp-contract=off on both sides: the Makefile sets it).  They exist for the tests: the
// cooling kernels (qk_cooling.hip) have a second instantiation over these two functions, which the CPU oracle reproduces in every bit — the device
// libm's log10 / pow differ from glibc's in the last bit, and the cooling algorithm is discontinuous at that level.  Production never selects them.
//   log10: x = 2^k m, m in [sqrt(1/2), sqrt(2)); s = (m - 1) / (m + 1); ln m = 2 s + 2 s z Q(z), z = s^2, Q the series 1/3 + z/5 + ... + z^11/25
//          (z <= 0.0295: the first term left out is < 2e-21 of 2 s); log10 x = k log10(2) [hi + lo, k hi exact] + ln m / ln 10
//          measured over the arguments the cooling algorithm passes: <= 2.6 ulps from the exact value (tests/test_cooling_reference.py)
//   rsqrt: 1.0 / sqrt(x) corrected by one Newton step whose residual two fma form (fma is correctly rounded on both sides, and an explicit call is
//          not a contraction): <= 0.51 ulps from x^(-1/2)
#ifndef QK_PORTABLE_LIBM_HPP_
#define QK_PORTABLE_LIBM_HPP_

#include <cmath>

#ifndef QK_HD
#if defined(__HIPCC__)
#define QK_HD __host__ __device__ inline
#else
#define QK_HD inline
#endif
#endif

namespace qk
{
namespace portable
{

QK_HD auto log10(double x) -> double
{
	if (!(x > 0.0)) {
		return (x == 0.0) ? -HUGE_VAL : NAN; // (a NaN or a negative argument: NaN)
	}
	if (x == HUGE_VAL) {
		return x;
	}
	constexpr double SQRT_HALF = 0.70710678118654752440;
	constexpr double LOG10_2_HI = 0x1.34413509f0000p-2; // log10(2) with 16 trailing zero bits: k * HI is exact for |k| <= 1100
	constexpr double LOG10_2_LO = 0x1.e7fbcc47c4acdp-40;
	constexpr double INV_LN10 = 0.43429448190325182765;
	int k = 0;
	double m = frexp(x, &k); // [1/2, 1)
	if (m < SQRT_HALF) {
		m *= 2.0;
		k -= 1;
	}
	const double s = (m - 1.0) / (m + 1.0);
	const double z = s * s;
	double q = 1.0 / 25.0;
	q = q * z + 1.0 / 23.0;
	q = q * z + 1.0 / 21.0;
	q = q * z + 1.0 / 19.0;
	q = q * z + 1.0 / 17.0;
	q = q * z + 1.0 / 15.0;
	q = q * z + 1.0 / 13.0;
	q = q * z + 1.0 / 11.0;
	q = q * z + 1.0 / 9.0;
	q = q * z + 1.0 / 7.0;
	q = q * z + 1.0 / 5.0;
	q = q * z + 1.0 / 3.0;
	const double two_s = 2.0 * s;
	const double ln_m = two_s + two_s * (z * q);
	const double kd = static_cast<double>(k);
	return kd * LOG10_2_HI + (kd * LOG10_2_LO + ln_m * INV_LN10);
}

QK_HD auto rsqrt(double x) -> double
{
	const double r = 1.0 / sqrt(x); // two roundings: up to 1.5 ulps from x^(-1/2)
	if (!(r > 0.0) || r == HUGE_VAL) {
		return r; // (x = inf, 0, negative or NaN: 0, inf, NaN)
	}
	// one Newton step on the residual 1 - x r^2, which two fma form exactly enough: the result is the correctly rounded x^(-1/2) in all but rare ties
	const double t = x * r;
	const double t_lo = fma(x, r, -t);
	const double e = fma(-t, r, 1.0) - t_lo * r;
	return fma(0.5 * r, e, r);
}

} // namespace portable
} // namespace qk

#endif // QK_PORTABLE_LIBM_HPP_
