// Stand-alone check of the stencil arithmetic of the CIC particles (quokka_amd/csrc/qk_cic_index.hpp), meant to be built with
// -fsanitize=address,undefined: positions on cell centres, cell faces, domain faces, one and many cells outside and at +-1e300 (and non-finite ones)
// are walked per direction and combined; a key indexes a heap array of exactly numKeys() + 1 entries and a clamped stencil cell a heap array of
// exactly the dense size, so an index out of bounds — or a double converted to an int it does not fit — is reported by the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "qk_cic_index.hpp"
#include "qk_gravity_index.hpp"

using namespace qk;

static int fail(const char *what, const int (&n)[3], double x)
{
	std::fprintf(stderr, "FAIL %s at n = (%d, %d, %d), x = %.17g\n", what, n[0], n[1], n[2], x);
	return 1;
}

// positions of one direction with N cells from plo, spacing dx
static std::vector<double> positions(int N, double plo, double dx)
{
	std::vector<double> v;
	for (int c = -3; c <= N + 2; ++c) {
		v.push_back(plo + (c + 0.5) * dx);  // cell centres, up to three cells outside
		v.push_back(plo + c * dx);	      // cell faces, the domain faces among them
		v.push_back(plo + (c + 0.25) * dx); // between
		v.push_back(plo + (c + 0.999999) * dx);
	}
	v.push_back(std::nextafter(plo, -1.0e300));
	v.push_back(std::nextafter(plo + N * dx, 1.0e300));
	v.push_back(plo - 0.5 * dx); // l = -1 exactly: the last position that takes part
	v.push_back(std::nextafter(plo - 0.5 * dx, -1.0e300));
	v.push_back(plo + (N + 0.5) * dx); // l = N: the first that does not
	v.push_back(std::nextafter(plo + (N + 0.5) * dx, -1.0e300));
	for (double far : {1.0e3, 1.0e10, 3.0e9 * dx, 1.0e19 * dx, 1.0e300}) {
		v.push_back(plo + far);
		v.push_back(plo - far);
	}
	v.push_back(std::numeric_limits<double>::infinity());
	v.push_back(-std::numeric_limits<double>::infinity());
	v.push_back(std::numeric_limits<double>::quiet_NaN());
	return v;
}

static int check(const int (&n)[3], const double (&plo)[3], double dx)
{
	const double dxi = 1.0 / dx;
	const int64_t nk = cic::numKeys(n);
	std::vector<int64_t> count(static_cast<size_t>(nk) + 1, 0);
	const gravity::Dims D{{n[0], n[1], n[2]}};
	std::vector<double> dense(static_cast<size_t>(gravity::denseSize(D)), 0.0);
	std::vector<double> px[3];
	for (int d = 0; d < 3; ++d) {
		px[d] = positions(n[d], plo[d], dx);
	}
	// per direction: weights, take-part decision, clamp
	for (int d = 0; d < 3; ++d) {
		for (double x : px[d]) {
			const cic::Axis a = cic::axis(x, plo[d], dxi);
			const bool part = cic::takesPart(a, n[d]);
			if (std::isfinite(x) && std::fabs(x) < 1.0e200) {
				if (!(a.w0 >= 0.0 && a.w0 <= 1.0 && a.w1 >= 0.0 && a.w1 < 1.0) || a.w0 + a.w1 != 1.0) {
					return fail("weights", n, x);
				}
			}
			if (part != (a.l >= -1.0 && a.l < n[d])) {
				return fail("take-part decision", n, x);
			}
			if (part) {
				const int b = cic::baseCell(a);
				if (b < -1 || b > n[d] - 1 || static_cast<double>(b) != a.bf) {
					return fail("base cell", n, x);
				}
			}
			for (int o = 0; o < 2; ++o) {
				const int c = cic::clampCell(a.bf, o, n[d]);
				if (c < 0 || c > n[d] - 1) {
					return fail("clamp", n, x);
				}
				if (part && a.bf + o >= 0.0 && a.bf + o <= n[d] - 1 && c != cic::baseCell(a) + o) {
					return fail("clamp moved an interior cell", n, x);
				}
			}
		}
	}
	// combined: keys and the dense cells the kick reads
	for (double x2 : px[2]) {
		for (double x1 : px[1]) {
			for (double x0 : px[0]) {
				const cic::Axis a0 = cic::axis(x0, plo[0], dxi), a1 = cic::axis(x1, plo[1], dxi), a2 = cic::axis(x2, plo[2], dxi);
				const int64_t key = cic::particleKey(n, a0, a1, a2);
				const bool part = cic::takesPart(a0, n[0]) && cic::takesPart(a1, n[1]) && cic::takesPart(a2, n[2]);
				if (key < 0 || key > nk || (key == nk) == part) {
					return fail("key range / sentinel", n, x0);
				}
				count[static_cast<size_t>(key)] += 1; // (raw access: the sanitizer's to catch)
				if (part) {
					const int b0 = cic::baseCell(a0), b1 = cic::baseCell(a1), b2 = cic::baseCell(a2);
					if (key != (b0 + 1) + static_cast<int64_t>(n[0] + 1) * ((b1 + 1) + static_cast<int64_t>(n[1] + 1) * (b2 + 1))) {
						return fail("key", n, x0);
					}
				}
				for (int o = 0; o < 8; ++o) {
					const int ci = cic::clampCell(a0.bf, o & 1, n[0]), cj = cic::clampCell(a1.bf, (o >> 1) & 1, n[1]),
						  ck = cic::clampCell(a2.bf, o >> 2, n[2]);
					const int64_t idx = gravity::denseIndex(D, ci, cj, ck);
					const int64_t sx = n[0] + 2, sy = sx * (n[1] + 2);
					for (int64_t st : {static_cast<int64_t>(1), sx, sy}) {
						dense[static_cast<size_t>(idx + st)] += 1.0;
						dense[static_cast<size_t>(idx - st)] += 1.0;
					}
				}
			}
		}
	}
	// every key of the deposit kernel's gather: cell c and its eight source base cells
	for (int k = 0; k < n[2]; ++k) {
		for (int j = 0; j < n[1]; ++j) {
			for (int i = 0; i < n[0]; ++i) {
				for (int o = 0; o < 8; ++o) {
					const int64_t key = cic::keyOf(n, i - (o & 1), j - ((o >> 1) & 1), k - (o >> 2));
					if (key < 0 || key >= nk) {
						return fail("gather key", n, static_cast<double>(i));
					}
					count[static_cast<size_t>(key) + 1] += 0;
				}
			}
		}
	}
	// edges and corners of the dense array are never touched by the kick's reads
	for (int k = -1; k <= n[2]; ++k) {
		for (int j = -1; j <= n[1]; ++j) {
			for (int i = -1; i <= n[0]; ++i) {
				const int out = (i < 0 || i >= n[0]) + (j < 0 || j >= n[1]) + (k < 0 || k >= n[2]);
				if (out >= 2 && dense[static_cast<size_t>(gravity::denseIndex(D, i, j, k))] != 0.0) {
					return fail("an edge or corner of the dense array is read", n, static_cast<double>(i));
				}
			}
		}
	}
	return 0;
}

int main()
{
	const int sizes[][3] = {{4, 4, 4}, {8, 6, 4}, {16, 8, 12}, {4, 32, 6}};
	const double plos[][3] = {{0.0, 0.0, 0.0}, {-2.5e13, -2.5e13, -2.5e13}, {0.3, -1.7, 11.0}};
	const double dxs[] = {0.25, 1.5625e12, 0.0625};
	for (const auto &n : sizes) {
		for (int g = 0; g < 3; ++g) {
			if (check(n, plos[g], dxs[g]) != 0) {
				return 1;
			}
		}
	}
	std::puts("cic index bookkeeping OK");
	return 0;
}
