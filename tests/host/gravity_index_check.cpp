// Stand-alone check of the ghost-list bookkeeping of the self-gravity solver (quokka_amd/csrc/qk_gravity_index.hpp), meant to be built with
// -fsanitize=address,undefined: every ghost of the list is written into and read from a heap array of exactly denseSize() doubles, so an index
// out of bounds is reported by the sanitizer, and the list is checked to hold every face-adjacent ghost cell exactly once, in the documented order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qk_gravity_index.hpp"

using namespace qk::gravity;

static int fail(const char *what, const Dims &D, long long g)
{
	std::fprintf(stderr, "FAIL %s at n = (%d, %d, %d), g = %lld\n", what, D.n[0], D.n[1], D.n[2], g);
	return 1;
}

static int check(const Dims D)
{
	const int64_t S = numGhosts(D);
	if (S != 2 * (static_cast<int64_t>(D.n[0]) * D.n[1] + static_cast<int64_t>(D.n[1]) * D.n[2] + static_cast<int64_t>(D.n[0]) * D.n[2])) {
		return fail("numGhosts", D, -1);
	}
	std::vector<double> dense(static_cast<size_t>(denseSize(D)), 0.0);
	std::vector<int> hits(dense.size(), 0);
	int64_t prev_key = -1;
	for (int64_t g = 0; g < S; ++g) {
		int xyz[3], nb[3], side;
		const int d = ghostCoord(D, g, xyz, side);
		ghostNeighbour(D, d, side, xyz, nb);
		if (d < 0 || d > 2 || (side != 0 && side != 1) || xyz[d] != (side == 0 ? -1 : D.n[d])) {
			return fail("normal coordinate", D, g);
		}
		for (int e = 0; e < 3; ++e) {
			if (e != d && (xyz[e] < 0 || xyz[e] >= D.n[e])) {
				return fail("tangential coordinate", D, g);
			}
			if (nb[e] < 0 || nb[e] >= D.n[e] || (e != d && nb[e] != xyz[e])) {
				return fail("neighbour", D, g);
			}
		}
		if ((nb[d] > xyz[d] ? nb[d] - xyz[d] : xyz[d] - nb[d]) != 1) {
			return fail("neighbour distance", D, g);
		}
		// list order: face, then the slow tangential index, then the fast one
		const int ta = d == 0 ? 1 : 0, tb = d == 2 ? 1 : 2;
		const int64_t key = ((static_cast<int64_t>(2 * d + side) * 8192 + xyz[tb]) * 8192) + xyz[ta];
		if (key <= prev_key) {
			return fail("list order", D, g);
		}
		prev_key = key;
		const int64_t ig = denseIndex(D, xyz[0], xyz[1], xyz[2]), in = denseIndex(D, nb[0], nb[1], nb[2]);
		dense.at(static_cast<size_t>(ig)) += 1.0;
		dense[static_cast<size_t>(ig)] += dense[static_cast<size_t>(in)]; // (raw accesses: the sanitizer's to catch)
		hits[static_cast<size_t>(ig)] += 1;
	}
	int64_t once = 0;
	for (int h : hits) {
		if (h > 1) {
			return fail("a ghost cell listed twice", D, -1);
		}
		once += h;
	}
	return once == S ? 0 : fail("coverage", D, -1);
}

int main()
{
	const int sizes[][3] = {{4, 4, 4}, {8, 8, 8}, {8, 6, 4}, {16, 8, 12}, {4, 32, 6}, {64, 4, 4}};
	for (const auto &n : sizes) {
		if (check(Dims{{n[0], n[1], n[2]}}) != 0) {
			return 1;
		}
	}
	std::puts("gravity index bookkeeping OK");
	return 0;
}
