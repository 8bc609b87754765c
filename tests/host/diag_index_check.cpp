// Stand-alone check of the index arithmetic of the DiagPDF histograms (quokka_amd/csrc/qk_diag_index.hpp), meant to be built with
// -fsanitize=address,undefined: values on the edges of linear and log-spaced axes, NaN, infinities and huge values are walked, and a bin that is in
// range indexes a heap array of exactly total_bins entries; the block table of a list is walked for the lengths at which the number of blocks or of
// passes changes, every block indexing a heap array of exactly the list's length — so an index out of bounds, or a double converted to an int it does
// not fit, is reported by the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "qk_diag_index.hpp"

using namespace qk;

static int fail(const char *what, double x)
{
	std::fprintf(stderr, "FAIL %s at %.17g\n", what, x);
	return 1;
}

static diag::Axis makeAxis(int nbins, int log_spaced, double low, double high)
{
	diag::Axis a;
	a.nbins = nbins;
	a.log_spaced = log_spaced;
	if (log_spaced != 0) {
		const double range = std::log10(high) - std::log10(low);
		a.lowT = std::log10(low);
		a.widthT = range / static_cast<double>(nbins);
	} else {
		a.lowT = low;
		a.widthT = (high - low) / static_cast<double>(nbins);
	}
	return a;
}

static int checkBins()
{
	const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
	const double big = std::numeric_limits<double>::max();
	// linear axis on exact doubles: [1, 3) in 4 bins of 0.5
	const diag::Axis lin = makeAxis(4, 0, 1.0, 3.0);
	std::vector<int> hits(4, 0);
	struct Case {
		double x;
		int bin; // -1: takes no part
	};
	const Case cases[] = {{1.0, 0},
			      {std::nextafter(1.0, 0.0), -1},
			      {1.5, 1},
			      {std::nextafter(1.5, 0.0), 0},
			      {2.0, 2},
			      {2.5, 3},
			      {std::nextafter(3.0, 0.0), 3},
			      {3.0, -1},
			      {nan, -1},
			      {inf, -1},
			      {-inf, -1},
			      {1.0e300, -1},
			      {-1.0e300, -1},
			      {big, -1},
			      {-big, -1},
			      {3.0e9, -1},
			      {-3.0e9, -1},
			      {1.0e19, -1}};
	for (const Case &c : cases) {
		const double q = diag::binCoordinate(lin, c.x);
		const bool in = diag::inRange(lin, q);
		if (in != (c.bin >= 0)) {
			return fail("linear: in range", c.x);
		}
		if (in) {
			const int b = diag::binOf(q);
			if (b != c.bin) {
				return fail("linear: bin", c.x);
			}
			hits[static_cast<size_t>(b)] += 1; // (heap array of exactly nbins entries)
		}
	}
	// log-spaced axis: [1e2, 1e8) in 6 bins; the decades 1e3 .. 1e7 sit on edges whose side the libm decides: walked half a bin away
	const diag::Axis lg = makeAxis(6, 1, 1.0e2, 1.0e8);
	const Case lcases[] = {{3.0e2, 0}, {3.0e3, 1}, {3.0e4, 2}, {3.0e5, 3}, {3.0e6, 4}, {3.0e7, 5}, {3.0e8, -1}, {3.0e1, -1}, {0.0, -1}, {-0.0, -1},
			       {-1.0, -1}, {nan, -1}, {inf, -1}, {-inf, -1}, {1.0e300, -1}, {big, -1}, {5.0e-324, -1}};
	std::vector<int> lhits(6, 0);
	for (const Case &c : lcases) {
		const double q = diag::binCoordinate(lg, c.x);
		const bool in = diag::inRange(lg, q);
		if (in != (c.bin >= 0)) {
			return fail("log: in range", c.x);
		}
		if (in) {
			const int b = diag::binOf(q);
			if (b != c.bin) {
				return fail("log: bin", c.x);
			}
			lhits[static_cast<size_t>(b)] += 1;
		}
	}
	// a degenerate axis (low == high): the width is 0, q is NaN or infinite, nothing is in range and nothing is converted
	const diag::Axis flat = makeAxis(3, 0, 2.0, 2.0);
	for (double x : {1.0, 2.0, 3.0, nan}) {
		if (diag::inRange(flat, diag::binCoordinate(flat, x))) {
			return fail("degenerate axis: in range", x);
		}
	}
	// the linear bin: the last variable runs fastest; total bins and its refusals
	const diag::Axis axes[3] = {makeAxis(3, 0, 0.0, 3.0), makeAxis(4, 0, 0.0, 4.0), makeAxis(5, 0, 0.0, 5.0)};
	const int64_t tb = diag::totalBins(axes, 3);
	if (tb != 60) {
		return fail("totalBins", static_cast<double>(tb));
	}
	std::vector<int> pdf(static_cast<size_t>(tb), 0);
	const double xs[3] = {2.5, 1.5, 0.5};
	int64_t cbin = 0;
	for (int n = 0; n < 3; ++n) {
		cbin = diag::linearBin(cbin, axes[n], diag::binOf(diag::binCoordinate(axes[n], xs[n])));
	}
	if (cbin != (2 * 4 + 1) * 5 + 0) {
		return fail("linearBin", static_cast<double>(cbin));
	}
	pdf[static_cast<size_t>(cbin)] += 1;
	const diag::Axis many[2] = {makeAxis(4096, 0, 0.0, 1.0), makeAxis(4097, 0, 0.0, 1.0)};
	const diag::Axis exact[2] = {makeAxis(4096, 0, 0.0, 1.0), makeAxis(4096, 0, 0.0, 1.0)};
	const diag::Axis none[1] = {makeAxis(0, 0, 0.0, 1.0)};
	if (diag::totalBins(many, 2) != -1 || diag::totalBins(exact, 2) != diag::kMaxTotalBins || diag::totalBins(none, 1) != -1) {
		return fail("totalBins: limits", 0.0);
	}
	return 0;
}

// S of a list by the block table, every access through the table; compared with the sum in long double
static int checkBlocks()
{
	const int64_t lengths[] = {1, 2, 255, 256, 257, 65536, 65537};
	const int passes[] = {1, 1, 1, 1, 2, 2, 3};
	if (diag::numBlocks(0) != 0) {
		return fail("numBlocks(0)", 0.0);
	}
	int which = 0;
	for (int64_t n : lengths) {
		if (diag::numPasses(n) != passes[which++]) {
			return fail("numPasses", static_cast<double>(n));
		}
		std::vector<double> list(static_cast<size_t>(n));
		long double exact = 0.0L, mag = 0.0L;
		uint64_t state = 0x9E3779B97F4A7C15ULL + static_cast<uint64_t>(n);
		for (int64_t e = 0; e < n; ++e) {
			state = state * 6364136223846793005ULL + 1442695040888963407ULL;
			const double u = static_cast<double>(state >> 11) * (1.0 / 9007199254740992.0);
			list[static_cast<size_t>(e)] = std::pow(10.0, 6.0 * u - 3.0); // six decades
			exact += list[static_cast<size_t>(e)];
			mag += std::fabs(list[static_cast<size_t>(e)]);
		}
		int taken = 0;
		while (true) {
			const int64_t len = static_cast<int64_t>(list.size()), nb = diag::numBlocks(len);
			std::vector<double> next(static_cast<size_t>(nb));
			int64_t covered = 0;
			for (int64_t j = 0; j < nb; ++j) {
				const diag::Block b = diag::blockOf(0, len, j);
				if (!diag::blockIsValid(b.start, b.len, len) || b.start != covered) {
					return fail("blockOf", static_cast<double>(n));
				}
				covered += b.len;
				double v[diag::kBlock];
				for (int t = 0; t < diag::kBlock; ++t) {
					v[t] = t < b.len ? list[static_cast<size_t>(b.start + t)] : 0.0;
				}
				next[static_cast<size_t>(j)] = diag::treeReduce(v);
			}
			if (covered != len) {
				return fail("blocks do not cover the list", static_cast<double>(n));
			}
			list.swap(next);
			++taken;
			if (list.size() == 1) {
				break;
			}
		}
		if (taken != diag::numPasses(n)) {
			return fail("passes taken", static_cast<double>(n));
		}
		const long double err = std::fabs(static_cast<long double>(list[0]) - exact);
		if (err > 64.0L * 1.1102230246251565404e-16L * mag) {
			return fail("S is far from the exact sum", static_cast<double>(n));
		}
	}
	// blocks that a workgroup must refuse
	if (diag::blockIsValid(0, 0, 10) || diag::blockIsValid(-1, 1, 10) || diag::blockIsValid(10, 1, 10) || diag::blockIsValid(0, 257, 1000) ||
	    diag::blockIsValid(5, 6, 10) || !diag::blockIsValid(4, 6, 10) || diag::blockIsValid(0, 1, 0)) {
		return fail("blockIsValid", 0.0);
	}
	// a single -0.0 takes one pass and comes out as +0.0; a full block of -0.0 keeps its sign
	double v[diag::kBlock];
	for (int t = 0; t < diag::kBlock; ++t) {
		v[t] = t == 0 ? -0.0 : 0.0;
	}
	if (std::signbit(diag::treeReduce(v))) {
		return fail("tree of one -0.0", 0.0);
	}
	for (int t = 0; t < diag::kBlock; ++t) {
		v[t] = -0.0;
	}
	if (!std::signbit(diag::treeReduce(v))) {
		return fail("tree of 256 -0.0", 0.0);
	}
	return 0;
}

int main()
{
	if (checkBins() != 0 || checkBlocks() != 0) {
		return 1;
	}
	std::printf("OK\n");
	return 0;
}
