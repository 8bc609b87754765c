// qk_diag_index.hpp — index arithmetic of the DiagPDF histograms (qk_diag.hip), host and device: the bin of a value, the linear bin of
// a cell, the cut of a bin's weight list into blocks of 256 and the fixed tree that reduces one block.  Plain C++ (no HIP types) so that a stand-alone
// host program can exercise it under a sanitizer.  Every decision is taken on doubles BEFORE a conversion to an integer: a NaN, an infinity or 1e300
// takes no part and cannot overflow an int.
#ifndef QK_DIAG_INDEX_HPP_
#define QK_DIAG_INDEX_HPP_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define QK_DIAG_HD __host__ __device__ inline
#else
#define QK_DIAG_HD inline
#endif

namespace qk
{
namespace diag
{

constexpr int kBlock = 256;				    // weights per block == threads per workgroup of the segment sum
constexpr int64_t kMaxTotalBins = static_cast<int64_t>(1) << 24; // more bins than this: QK_ERR_UNSUPPORTED

// one histogram axis: lowT = log10(low) or low; widthT = (log10(high) - log10(low)) / nbins or (high - low) / nbins (formed by the caller)
struct Axis {
	double lowT;
	double widthT;
	int nbins;
	int log_spaced;
};

// q = (val - lowT) / widthT with val = log10(x) or x (reference DiagPDF::getBinIndex1D, before its floor and cast)
QK_DIAG_HD auto binCoordinate(const Axis &a, double x) -> double
{
	const double val = a.log_spaced != 0 ? std::log10(x) : x;
	return (val - a.lowT) / a.widthT;
}

// in range iff 0.0 <= q < nbins (false for a NaN): the reference's 0 <= floor(q) < nbins wherever its cast is defined
QK_DIAG_HD auto inRange(const Axis &a, double q) -> bool { return q >= 0.0 && q < static_cast<double>(a.nbins); }

// bin of a coordinate that is in range
QK_DIAG_HD auto binOf(double q) -> int { return static_cast<int>(std::floor(q)); }

// cbin = cbin * nbins + bin: the last variable runs fastest
QK_DIAG_HD auto linearBin(int64_t cbin, const Axis &a, int bin) -> int64_t { return cbin * a.nbins + static_cast<int64_t>(bin); }

// product of the bin counts; -1 if a count is not positive or the product exceeds kMaxTotalBins
QK_DIAG_HD auto totalBins(const Axis *axes, int nvars) -> int64_t
{
	int64_t t = 1;
	for (int n = 0; n < nvars; ++n) {
		if (axes[n].nbins <= 0) {
			return -1;
		}
		t *= axes[n].nbins;
		if (t > kMaxTotalBins) {
			return -1;
		}
	}
	return t;
}

// ---- the sum S(list) of one bin: blocks of 256 from the start of the list, the last one padded with +0.0, each reduced by the tree below; the block
// results, in order, are the next list; repeated until one value is left.  An empty list gives +0.0 and takes no pass.

// blocks that a list of `count` weights is cut into
QK_DIAG_HD auto numBlocks(int64_t count) -> int64_t { return (count + (kBlock - 1)) / kBlock; }

// passes until a list of `count` weights (count >= 1) has become one value: 1 for 1 .. 256, 2 for 257 .. 65536, ...
QK_DIAG_HD auto numPasses(int64_t count) -> int
{
	int p = 1;
	for (int64_t c = numBlocks(count); c > 1; c = numBlocks(c)) {
		++p;
	}
	return p;
}

// block j (0 <= j < numBlocks(hi - lo)) of the list that occupies [lo, hi) of an array: first element and length (1 .. 256)
struct Block {
	int64_t start;
	int64_t len;
};
QK_DIAG_HD auto blockOf(int64_t lo, int64_t hi, int64_t j) -> Block
{
	Block b;
	b.start = lo + j * kBlock;
	const int64_t rest = hi - b.start;
	b.len = rest < kBlock ? rest : static_cast<int64_t>(kBlock);
	return b;
}

// what a workgroup may be handed: a block that lies inside an array of n elements
QK_DIAG_HD auto blockIsValid(int64_t start, int64_t len, int64_t n) -> bool { return start >= 0 && len >= 1 && len <= kBlock && start <= n - len; }

// the fixed tree on one block of 256 values (padded by the caller): v[t] = v[t] + v[t + s] for t < s, s = 128, 64, ..., 1; the result is v[0].
// Serial form of what the workgroup does with one thread per t (the steps of one s are independent).
inline auto treeReduce(double *v) -> double
{
	for (int s = kBlock / 2; s >= 1; s /= 2) {
		for (int t = 0; t < s; ++t) {
			v[t] = v[t] + v[t + s];
		}
	}
	return v[0];
}

} // namespace diag
} // namespace qk

#endif // QK_DIAG_INDEX_HPP_
