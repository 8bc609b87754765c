// qk_ghost_source.hpp — where the value of a cell OUTSIDE a box comes from, on a level whose ghost fill is a pure re-addressing:
// equal boxes on a regular lattice that covers a rectangular domain, all on this rank, every domain face periodic, reflecting or first-order
// extrapolating.  There, what FillBoundary (k_copy) followed by PhysBCFunct (k_physbc) leaves in a ghost cell is the value of exactly one valid
// cell, possibly with the sign of the normal momentum (velocity) flipped.  The map below names that cell; a consumer that applies it reads what
// the fill would have put into the ghost cell, bit for bit, and nobody has to write the ghost cell (qk_hydro_stage_args::ghost_from_source).
//
// The map is one entry per box, dimension and side (GhostFace): index i beyond that face of the box is index a + b i of box `box` —
//   a face inside the domain   the neighbouring box, same index                       a = 0, b = 1
//   periodic wall              the box at the other end of the lattice, i -+ width    a = -+ width, b = 1
//   reflecting wall            the box itself, 2 lo - 1 - i  |  2 hi + 1 - i          b = -1, flip: the normal component changes sign (REFLECT_ODD)
//   extrapolating wall         the box itself, lo  |  hi                              b = 0
// (k_physbc, qk_boundary.hip, composes the same per-dimension rules; k_copy supplies the periodic images and the neighbours' cells and runs
// first.)  A cell that is outside in several dimensions — the edges the pre-pass rim reads — follows the entries dimension by dimension: each acts on
// its own index, and on a regular lattice the box reached through x has the same y and z faces rules as the one it was reached from.
// Shared by the kernels and by the host-side plan (and its CPU test): host + device.
#ifndef QK_GHOST_SOURCE_HPP_
#define QK_GHOST_SOURCE_HPP_

#include <hip/hip_runtime.h>

#include "quokka_amd.h"

namespace qk
{

struct GhostFace {
	int box;  // local index of the source box
	int a, b; // source index = a + b * index
	int flip; // 1: mirrored (the component normal to the face changes sign)
};
// the entry of box `box`, dimension d, side (0 low, 1 high) in the table [nboxes][3][2]
__host__ __device__ __forceinline__ auto ghostFaceSlot(int box, int d, int side) -> int { return 6 * box + 2 * d + side; }

} // namespace qk

#endif // QK_GHOST_SOURCE_HPP_
