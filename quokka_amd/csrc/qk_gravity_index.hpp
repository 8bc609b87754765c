// qk_gravity_index.hpp — index bookkeeping of the self-gravity solver (qk_gravity.hip), host and device:
// the dense (N0+2)(N1+2)(N2+2) array with one ghost layer, and the list of the S = 2 (N1 N2 + N0 N2 + N0 N1) face-adjacent ghost cells.
// Plain C++ (no HIP types) so that a stand-alone host program can exercise it under a sanitizer.
#ifndef QK_GRAVITY_INDEX_HPP_
#define QK_GRAVITY_INDEX_HPP_

#include <cstdint>

#if defined(__HIPCC__)
#define QK_GRAV_HD __host__ __device__ inline
#else
#define QK_GRAV_HD inline
#endif

namespace qk
{
namespace gravity
{

struct Dims {
	int n[3];
};

// cell (i, j, k), each in [-1, N_d], of the dense array, x fastest
QK_GRAV_HD auto denseIndex(const Dims &D, int i, int j, int k) -> int64_t
{
	return (i + 1) + static_cast<int64_t>(D.n[0] + 2) * ((j + 1) + static_cast<int64_t>(D.n[1] + 2) * (k + 1));
}

QK_GRAV_HD auto denseSize(const Dims &D) -> int64_t { return static_cast<int64_t>(D.n[0] + 2) * (D.n[1] + 2) * (D.n[2] + 2); }

// ghosts of the two faces normal to direction d (one face)
QK_GRAV_HD auto faceSize(const Dims &D, int d) -> int64_t
{
	return d == 0 ? static_cast<int64_t>(D.n[1]) * D.n[2] : (d == 1 ? static_cast<int64_t>(D.n[0]) * D.n[2] : static_cast<int64_t>(D.n[0]) * D.n[1]);
}

QK_GRAV_HD auto numGhosts(const Dims &D) -> int64_t { return 2 * (faceSize(D, 0) + faceSize(D, 1) + faceSize(D, 2)); }

// Ghost g of the list: faces in the order x-lo, x-hi, y-lo, y-hi, z-lo, z-hi; within a face the two tangential indices, the lower direction fastest.
// xyz: the ghost cell (normal coordinate -1 or N_d).  Returns the normal direction; side: 0 low, 1 high.
QK_GRAV_HD auto ghostCoord(const Dims &D, int64_t g, int (&xyz)[3], int &side) -> int
{
	// (written without run-time subscripts: the arrays stay in registers on the device)
	const int64_t f0 = faceSize(D, 0), f1 = faceSize(D, 1);
	int d = 0;
	if (g >= 2 * f0) {
		g -= 2 * f0;
		d = 1;
		if (g >= 2 * f1) {
			g -= 2 * f1;
			d = 2;
		}
	}
	const int64_t fs = d == 0 ? f0 : (d == 1 ? f1 : faceSize(D, 2));
	side = g >= fs ? 1 : 0;
	const int64_t t = g - side * fs;
	const int na = d == 0 ? D.n[1] : D.n[0]; // extent of the fast tangential direction (y for the x faces, else x)
	const int a = static_cast<int>(t % na), b = static_cast<int>(t / na);
	const int nd = d == 0 ? D.n[0] : (d == 1 ? D.n[1] : D.n[2]);
	const int nrm = side == 0 ? -1 : nd;
	xyz[0] = d == 0 ? nrm : a;
	xyz[1] = d == 0 ? a : (d == 1 ? nrm : b);
	xyz[2] = d == 2 ? nrm : b;
	return d;
}

// the interior neighbour nb(g) of ghost cell xyz with normal direction d
QK_GRAV_HD void ghostNeighbour(const Dims &D, int d, int side, const int (&xyz)[3], int (&nb)[3])
{
	nb[0] = d == 0 ? (side == 0 ? 0 : D.n[0] - 1) : xyz[0];
	nb[1] = d == 1 ? (side == 0 ? 0 : D.n[1] - 1) : xyz[1];
	nb[2] = d == 2 ? (side == 0 ? 0 : D.n[2] - 1) : xyz[2];
}

} // namespace gravity
} // namespace qk

#endif // QK_GRAVITY_INDEX_HPP_
