// qk_cic_index.hpp — stencil arithmetic of the CIC particles (qk_cic.hip), host and device: the lattice coordinate of a position, the
// take-part decision, the base cell, the linear weights, the key on the (N0+1)(N1+1)(N2+1) lattice of possible base cells, and the clamp of the kick.
// Plain C++ (no HIP types) so that a stand-alone host program can exercise it under a sanitizer.  Every decision is taken on doubles BEFORE a
// conversion to an integer: a far-away (or non-finite) position cannot overflow an int.
#ifndef QK_CIC_INDEX_HPP_
#define QK_CIC_INDEX_HPP_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define QK_CIC_HD __host__ __device__ inline
#else
#define QK_CIC_HD inline
#endif

namespace qk
{
namespace cic
{

// one direction of a particle's stencil: l = (x - plo) * dxi - 0.5, bf = floor(l) (kept as a double), t = l - bf, weights {1 - t, t}
struct Axis {
	double l;
	double bf;
	double w0;
	double w1;
};

QK_CIC_HD auto axis(double x, double plo, double dxi) -> Axis
{
	Axis a;
	a.l = (x - plo) * dxi - 0.5;
	a.bf = std::floor(a.l);
	const double t = a.l - a.bf;
	a.w0 = 1.0 - t;
	a.w1 = t;
	return a;
}

// the particle reaches at least one cell column of direction d: -1.0 <= l < N (false for a NaN)
QK_CIC_HD auto takesPart(const Axis &a, int n) -> bool { return a.l >= -1.0 && a.l < static_cast<double>(n); }

// base cell of a direction that takes part: in [-1, N - 1]
QK_CIC_HD auto baseCell(const Axis &a) -> int { return static_cast<int>(a.bf); }

// number of possible base cells (b + 1 in [0, N_d] per direction) — also the sentinel key of a particle that does not take part
QK_CIC_HD auto numKeys(const int (&n)[3]) -> int64_t { return static_cast<int64_t>(n[0] + 1) * (n[1] + 1) * (n[2] + 1); }

// key of base cell (b0, b1, b2), each in [-1, N_d - 1]: the linear index of b + 1, x fastest
QK_CIC_HD auto keyOf(const int (&n)[3], int b0, int b1, int b2) -> int64_t
{
	return (b0 + 1) + static_cast<int64_t>(n[0] + 1) * ((b1 + 1) + static_cast<int64_t>(n[1] + 1) * (b2 + 1));
}

QK_CIC_HD auto particleKey(const int (&n)[3], const Axis &a0, const Axis &a1, const Axis &a2) -> int64_t
{
	if (!(takesPart(a0, n[0]) && takesPart(a1, n[1]) && takesPart(a2, n[2]))) {
		return numKeys(n);
	}
	return keyOf(n, baseCell(a0), baseCell(a1), baseCell(a2));
}

// stencil cell bf + o (o = 0 or 1) of the kick, clamped to [0, N - 1] on the double (a NaN goes to 0)
QK_CIC_HD auto clampCell(double bf, int o, int n) -> int
{
	const double v = bf + static_cast<double>(o);
	return v >= 0.0 ? (v <= static_cast<double>(n - 1) ? static_cast<int>(v) : n - 1) : 0;
}

} // namespace cic
} // namespace qk

#endif // QK_CIC_INDEX_HPP_
