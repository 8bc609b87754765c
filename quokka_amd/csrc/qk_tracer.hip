// qk_tracer.hip — tracer particles on one level and one rank (include/quokka_amd.h "tracer particles"):
//   qk_tracer_plan_create      the cell -> box lattice of a BoxArray that tiles the domain
//   qk_tracer_InitOnePerCell   one particle per valid cell                              (reference src/simulation.hpp:1993-2005)
//   qk_tracer_AdvectWithUmac   AMReX's predictor-corrector MAC advection, both passes    (reference src/QuokkaSimulation.hpp:1290-1314)
//   qk_tracer_Redistribute     periodic shift / drop beyond non-periodic faces           (reference src/simulation.hpp:1317-1329)
//   qk_tracer_plan_create_refined / _set_parent / _set_time_weights / qk_tracer_Where: refined levels (DESIGN.md §11 "refined levels";
//                              reference src/simulation.hpp:1413, :1849-1852, :1896-1936, :1254-1258, :1317-1329)
// The face velocities carry no ghost faces here: an index outside the domain is wrapped (periodic) or clamped (everything else), which is what the
// reference's two ghost faces hold (int_dir / foextrap, src/simulation.hpp:182-205).
#include <algorithm>
#include <numeric>
#include <vector>

#include "qk_device.hpp"
#include "qk_internal.hpp"

using namespace qk;

namespace
{

constexpr int kMaxLdsLattice = 4096; // entries (16 KiB of LDS: ten 256-thread workgroups per CU); larger lattices are read from global memory
constexpr int kMaxCellsPerDir = 32768; // cell / granularity by a 32-bit multiply-high is exact below this (see latticeCoord)

// what the kernels need of the geometry; passed by value (kernel arguments are read through the scalar path)
struct TracerGeom {
	double plo[3], phi[3], dx[3], dxi[3];
	int n[3];	 // n_cell
	int periodic[3];
	int gran[3];	 // lattice granularity: the common divisor of all box edges in that direction
	unsigned magic[3]; // ceil(2^32 / gran) (gran >= 2): cell / gran == umulhi(cell, magic) for cell * gran < 2^32
	int nl[3];	 // lattice extent = n / gran
	int nlat;	 // nl[0] * nl[1] * nl[2]
};

constexpr int kMaxDepth = QK_TRACER_MAX_DEPTH;

// one ancestor level of one kind (prev / cur): what a face lookup on it needs
struct TracerLink {
	int n[3], periodic[3], gran[3];
	unsigned magic[3];
	int nl[3];
	const int *lattice;
	const qk_array4 *u[3];
};

// the ancestors of a refined level: e[kind][0] the parent, e[kind][1] its parent ...; the last entry filled of a kind has no holes
struct TracerChain {
	double alpha, beta;
	TracerLink e[2][kMaxDepth];
};

// the levels of a hierarchy as qk_tracer_Where reads them
struct WhereLevel {
	double dxi[3];
	int n[3], gran[3];
	unsigned magic[3];
	int nl[3];
	const int *lattice;
};
struct WhereArgs {
	int nlev, ngrow;
	WhereLevel L[kMaxDepth + 1];
};

} // namespace

struct qk_tracer_plan {
	qk_level *lev = nullptr;
	TracerGeom g{};
	std::vector<int> lattice;	  // host copy: lattice cell -> box index, x fastest
	std::vector<int64_t> cell_offset; // number of valid cells in the boxes before box b (nboxes + 1 entries)
	int *d_lattice = nullptr;
	int64_t *d_cell_offset = nullptr;
	// refined levels: the lattice may hold -1 (`holes`); link[kind]: the parent plan of that kind and its face arrays
	bool holes = false;
	struct Link {
		qk_tracer_plan *parent = nullptr;
		const qk_array4 *u[3] = {nullptr, nullptr, nullptr};
	} link[2];
	double alpha = 0.0, beta = 1.0;
	unsigned char *d_defer = nullptr; // one byte per particle: its stencil left the level in the first launch of AdvectWithUmac
	int64_t defer_cap = 0;
};

namespace
{

// index resolution in direction e for a stencil index `i` (cell index, or face index of the normal direction when `face`):
// periodic: modulo n (face n == face 0); else clamped to [0, n - 1] (cells) or [0, n] (faces)
QK_DEV auto resolveIndex(int i, int n, bool periodic, bool face) -> int
{
	if (periodic) {
		if (static_cast<unsigned>(i) >= static_cast<unsigned>(n)) { // (rare: only next to the domain faces)
			i %= n;
			if (i < 0) {
				i += n;
			}
		}
		return i;
	}
	const int top = face ? n : n - 1;
	return i < 0 ? 0 : (i > top ? top : i);
}

QK_DEV auto latticeCoord(int cell, int gran, unsigned magic) -> int
{
	return gran == 1 ? cell : static_cast<int>(__umulhi(static_cast<unsigned>(cell), magic));
}

// MAC interpolation of component D at position x (qk_tracer_AdvectWithUmac in include/quokka_amd.h)
// HOLES: a lattice entry may be -1 (a refined level); such a stencil point is left out and `off` set — the caller then discards the result
template <int NDIM, int D, bool HOLES, class LAT>
QK_DEV auto interpMac(const TracerGeom &g, LAT lat, const qk_array4 *__restrict__ u_t, const double (&x)[3], bool &off) -> double
{
	int idx[3][2] = {{0, 0}, {0, 0}, {0, 0}}; // resolved array index per direction and stencil point
	int lc[3][2] = {{0, 0}, {0, 0}, {0, 0}};  // lattice coordinate of the cell that owns it
	double sw[3][2] = {{1.0, 0.0}, {1.0, 0.0}, {1.0, 0.0}};
#pragma unroll
	for (int e = 0; e < NDIM; ++e) {
		double l = (x[e] - g.plo[e]) * g.dxi[e];
		if (e != D) {
			l -= 0.5;
		}
		const double fl = floor(l);
		const int i0 = static_cast<int>(fl);
		const double w = l - static_cast<double>(i0);
		sw[e][0] = 1.0 - w;
		sw[e][1] = w;
#pragma unroll
		for (int ii = 0; ii < 2; ++ii) {
			const int r = resolveIndex(i0 + ii, g.n[e], g.periodic[e] != 0, e == D);
			idx[e][ii] = r;
			// a shared face belongs to the box whose low face it is; the domain's top face to the last box
			const int cell = (e == D && r == g.n[e]) ? r - 1 : r;
			lc[e][ii] = latticeCoord(cell, g.gran[e], g.magic[e]);
		}
	}
	double acc = 0.0;
#pragma unroll
	for (int kk = 0; kk < (NDIM > 2 ? 2 : 1); ++kk) {
#pragma unroll
		for (int jj = 0; jj < (NDIM > 1 ? 2 : 1); ++jj) {
#pragma unroll
			for (int ii = 0; ii < 2; ++ii) {
				const int b = lat[lc[0][ii] + g.nl[0] * (lc[1][jj] + g.nl[1] * lc[2][kk])];
				if constexpr (HOLES) {
					if (b < 0) {
						off = true;
						continue;
					}
				}
				const RA4 U(u_t[b]);
				double w = sw[0][ii];
				if (NDIM > 1) {
					w = w * sw[1][jj];
				}
				if (NDIM > 2) {
					w = w * sw[2][kk];
				}
				acc = acc + w * U.p[U.idx(idx[0][ii], idx[1][jj], idx[2][kk])];
			}
		}
	}
	return acc;
}

template <int NDIM, bool HOLES, class LAT>
QK_DEV void interpAll(const TracerGeom &g, LAT lat, const qk_array4 *u0, const qk_array4 *u1, const qk_array4 *u2, const double (&x)[3], double (&v)[3],
		      bool &off)
{
	v[0] = interpMac<NDIM, 0, HOLES>(g, lat, u0, x, off);
	if constexpr (NDIM > 1) {
		v[1] = interpMac<NDIM, 1, HOLES>(g, lat, u1, x, off);
	}
	if constexpr (NDIM > 2) {
		v[2] = interpMac<NDIM, 2, HOLES>(g, lat, u2, x, off);
	}
}

// one thread per particle, grid-stride.  LDS_LAT: the lattice is staged in LDS (nlat <= kMaxLdsLattice), else read from global memory.
// HOLES (a refined level): a particle whose stencil leaves the level's boxes in either pass is not moved; defer[p] says so (k_tracer_advect_deferred).
template <int NDIM, bool LDS_LAT, bool HOLES = false>
__global__ void __launch_bounds__(256) k_tracer_advect(const TracerGeom g, const int *__restrict__ d_lattice, const qk_array4 *__restrict__ u0,
						       const qk_array4 *__restrict__ u1, const qk_array4 *__restrict__ u2, const double dt, const int64_t np,
						       double *__restrict__ x0, double *__restrict__ x1, double *__restrict__ x2, double *__restrict__ v0,
						       double *__restrict__ v1, double *__restrict__ v2, unsigned char *__restrict__ defer)
{
	__shared__ int s_lat[LDS_LAT ? kMaxLdsLattice : 1];
	if constexpr (LDS_LAT) {
		for (int t = threadIdx.x; t < g.nlat; t += blockDim.x) {
			s_lat[t] = d_lattice[t];
		}
		__syncthreads();
	}
	double *const xp[3] = {x0, x1, x2};
	double *const vp[3] = {v0, v1, v2};
	const double hdt = 0.5 * dt;
	for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < np; p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
		double x[3] = {0.0, 0.0, 0.0}, xm[3] = {0.0, 0.0, 0.0}, va[3] = {0.0, 0.0, 0.0}, vb[3] = {0.0, 0.0, 0.0};
#pragma unroll
		for (int e = 0; e < NDIM; ++e) {
			x[e] = xp[e][p];
		}
		bool off = false;
		if constexpr (LDS_LAT) {
			interpAll<NDIM, HOLES>(g, s_lat, u0, u1, u2, x, va, off);
		} else {
			interpAll<NDIM, HOLES>(g, d_lattice, u0, u1, u2, x, va, off);
		}
#pragma unroll
		for (int e = 0; e < NDIM; ++e) {
			xm[e] = x[e] + hdt * va[e];
		}
		if constexpr (HOLES) {
			if (off) {
				defer[p] = 1;
				continue;
			}
		}
		if constexpr (LDS_LAT) {
			interpAll<NDIM, HOLES>(g, s_lat, u0, u1, u2, xm, vb, off);
		} else {
			interpAll<NDIM, HOLES>(g, d_lattice, u0, u1, u2, xm, vb, off);
		}
		if constexpr (HOLES) {
			defer[p] = off ? 1 : 0;
			if (off) {
				continue;
			}
		}
#pragma unroll
		for (int e = 0; e < NDIM; ++e) {
			xp[e][p] = x[e] + dt * vb[e];
			vp[e][p] = vb[e];
		}
	}
}

// ---- refined levels: the particles k_tracer_advect<.., HOLES> left (include/quokka_amd.h "tracer particles on a refined hierarchy")
// U^K of ancestor KIDX at face (i0, i1, i2) of direction D: the stored value where that plan holds the face, else rule 3 on ITS parent
// (1 - w) U(c) + w U(c + e_D), c = floor(i / 2), w = 0.5 (i_D - 2 c_D): face_linear_interp at ratio 2 (reference src/simulation.hpp:1413, :1849-1852)
template <int NDIM, int D, int KIDX> QK_DEV auto chainValue(const TracerChain &c, const int kind, int i0, int i1, int i2) -> double
{
	const TracerLink &L = c.e[kind][KIDX];
	i0 = resolveIndex(i0, L.n[0], L.periodic[0] != 0, D == 0);
	if (NDIM > 1) {
		i1 = resolveIndex(i1, L.n[1], L.periodic[1] != 0, D == 1);
	}
	if (NDIM > 2) {
		i2 = resolveIndex(i2, L.n[2], L.periodic[2] != 0, D == 2);
	}
	const int c0 = (D == 0 && i0 == L.n[0]) ? i0 - 1 : i0, c1 = (D == 1 && i1 == L.n[1]) ? i1 - 1 : i1, c2 = (D == 2 && i2 == L.n[2]) ? i2 - 1 : i2;
	const int b = L.lattice[latticeCoord(c0, L.gran[0], L.magic[0]) +
				L.nl[0] * (latticeCoord(c1, L.gran[1], L.magic[1]) + L.nl[1] * latticeCoord(c2, L.gran[2], L.magic[2]))];
	if (b >= 0) {
		const RA4 U(L.u[D][b]);
		return U.p[U.idx(i0, i1, i2)];
	}
	if constexpr (KIDX + 1 < kMaxDepth) {
		const int p0 = i0 >> 1, p1 = i1 >> 1, p2 = i2 >> 1; // (resolved: not negative)
		const int iD = D == 0 ? i0 : (D == 1 ? i1 : i2), pD = D == 0 ? p0 : (D == 1 ? p1 : p2);
		const double w = 0.5 * static_cast<double>(iD - 2 * pD);
		double ab[2] = {0.0, 0.0};
#pragma unroll 1
		for (int s = 0; s < 2; ++s) {
			const double val = chainValue<NDIM, D, KIDX + 1>(c, kind, p0 + (D == 0 ? s : 0), p1 + (D == 1 ? s : 0), p2 + (D == 2 ? s : 0));
			ab[0] = s == 0 ? val : ab[0];
			ab[1] = s == 1 ? val : ab[1];
		}
		return (1.0 - w) * ab[0] + w * ab[1];
	}
	return __builtin_nan(""); // (not reached: the host ends every chain at a plan without holes)
}

// G = alpha U^prev + beta U^cur of the parent, time first (FillPatchTwoLevels' GetData, reference src/simulation.hpp:1896-1936)
template <int NDIM, int D> QK_DEV auto parentField(const TracerChain &c, const int i0, const int i1, const int i2) -> double
{
	double up = 0.0, uc = 0.0;
	if (c.alpha != 0.0) {
		up = chainValue<NDIM, D, 0>(c, QK_TRACER_PREV, i0, i1, i2);
	}
	if (c.beta != 0.0 || c.alpha == 0.0) {
		uc = chainValue<NDIM, D, 0>(c, QK_TRACER_CUR, i0, i1, i2);
	}
	return c.alpha == 0.0 ? uc : (c.beta == 0.0 ? up : c.alpha * up + c.beta * uc);
}

// interpMac with the fallback: the loops are kept rolled (the path is rare and must stay small), the arithmetic and its order are interpMac's
template <int NDIM, int D>
QK_DEV auto interpMacLinked(const TracerGeom &g, const int *__restrict__ lat, const qk_array4 *__restrict__ u_t, const TracerChain &c, const double x0,
			    const double x1, const double x2) -> double
{
	int ia[3] = {0, 0, 0};
	double wa[3] = {0.0, 0.0, 0.0};
	const double xs[3] = {x0, x1, x2};
#pragma unroll
	for (int e = 0; e < NDIM; ++e) {
		double l = (xs[e] - g.plo[e]) * g.dxi[e];
		if (e != D) {
			l -= 0.5;
		}
		const double fl = floor(l);
		ia[e] = static_cast<int>(fl);
		wa[e] = l - static_cast<double>(ia[e]);
	}
	double acc = 0.0;
#pragma unroll 1
	for (int s = 0; s < (1 << NDIM); ++s) { // kk outermost, ii innermost
		const int ii = s & 1, jj = (s >> 1) & 1, kk = (s >> 2) & 1;
		const int r0 = resolveIndex(ia[0] + ii, g.n[0], g.periodic[0] != 0, D == 0);
		const int r1 = NDIM > 1 ? resolveIndex(ia[1] + jj, g.n[1], g.periodic[1] != 0, D == 1) : 0;
		const int r2 = NDIM > 2 ? resolveIndex(ia[2] + kk, g.n[2], g.periodic[2] != 0, D == 2) : 0;
		double w = ii != 0 ? wa[0] : 1.0 - wa[0];
		if (NDIM > 1) {
			w = w * (jj != 0 ? wa[1] : 1.0 - wa[1]);
		}
		if (NDIM > 2) {
			w = w * (kk != 0 ? wa[2] : 1.0 - wa[2]);
		}
		const int c0 = (D == 0 && r0 == g.n[0]) ? r0 - 1 : r0, c1 = (D == 1 && r1 == g.n[1]) ? r1 - 1 : r1, c2 = (D == 2 && r2 == g.n[2]) ? r2 - 1 : r2;
		const int b = lat[latticeCoord(c0, g.gran[0], g.magic[0]) +
				  g.nl[0] * (latticeCoord(c1, g.gran[1], g.magic[1]) + g.nl[1] * latticeCoord(c2, g.gran[2], g.magic[2]))];
		double val;
		if (b >= 0) {
			const RA4 U(u_t[b]);
			val = U.p[U.idx(r0, r1, r2)];
		} else {
			const int p0 = r0 >> 1, p1 = r1 >> 1, p2 = r2 >> 1;
			const int rD = D == 0 ? r0 : (D == 1 ? r1 : r2), pD = D == 0 ? p0 : (D == 1 ? p1 : p2);
			const double wn = 0.5 * static_cast<double>(rD - 2 * pD);
			double ab[2] = {0.0, 0.0};
#pragma unroll 1
			for (int t = 0; t < 2; ++t) {
				const double gv = parentField<NDIM, D>(c, p0 + (D == 0 ? t : 0), p1 + (D == 1 ? t : 0), p2 + (D == 2 ? t : 0));
				ab[0] = t == 0 ? gv : ab[0];
				ab[1] = t == 1 ? gv : ab[1];
			}
			val = (1.0 - wn) * ab[0] + wn * ab[1];
		}
		acc = acc + w * val;
	}
	return acc;
}

// the second launch of AdvectWithUmac on a refined level: one thread per particle, only the marked ones work
template <int NDIM>
__global__ void __launch_bounds__(256) k_tracer_advect_deferred(const TracerGeom g, const int *__restrict__ d_lattice, const qk_array4 *__restrict__ u0,
								const qk_array4 *__restrict__ u1, const qk_array4 *__restrict__ u2, const TracerChain c,
								const double dt, const int64_t np, double *__restrict__ x0, double *__restrict__ x1,
								double *__restrict__ x2, double *__restrict__ v0, double *__restrict__ v1, double *__restrict__ v2,
								const unsigned char *__restrict__ defer)
{
	const double hdt = 0.5 * dt;
	for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < np; p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
		if (defer[p] == 0) {
			continue;
		}
		const double xa = x0[p], xb = NDIM > 1 ? x1[p] : 0.0, xc = NDIM > 2 ? x2[p] : 0.0;
		double pa = xa, pb = xb, pc = xc, va = 0.0, vb = 0.0, vc = 0.0;
#pragma unroll 1
		for (int pass = 0; pass < 2; ++pass) {
			va = interpMacLinked<NDIM, 0>(g, d_lattice, u0, c, pa, pb, pc);
			if constexpr (NDIM > 1) {
				vb = interpMacLinked<NDIM, 1>(g, d_lattice, u1, c, pa, pb, pc);
			}
			if constexpr (NDIM > 2) {
				vc = interpMacLinked<NDIM, 2>(g, d_lattice, u2, c, pa, pb, pc);
			}
			const double h = pass == 0 ? hdt : dt;
			pa = xa + h * va;
			if constexpr (NDIM > 1) {
				pb = xb + h * vb;
			}
			if constexpr (NDIM > 2) {
				pc = xc + h * vc;
			}
		}
		x0[p] = pa;
		v0[p] = va;
		if constexpr (NDIM > 1) {
			x1[p] = pb;
			v1[p] = vb;
		}
		if constexpr (NDIM > 2) {
			x2[p] = pc;
			v2[p] = vc;
		}
	}
}

__global__ void __launch_bounds__(256) k_tracer_init(const TracerGeom g, const int ndim, const qk_box *__restrict__ boxes, const int64_t *__restrict__ cell_offset,
						     const double o0, const double o1, const double o2, double *__restrict__ x0, double *__restrict__ x1,
						     double *__restrict__ x2, double *__restrict__ v0, double *__restrict__ v1, double *__restrict__ v2,
						     int64_t *__restrict__ id, int *__restrict__ cpu, const int64_t first_id, const int rank)
{
	const qk_box bx = boxes[blockIdx.y];
	const int l0 = bx.hi[0] - bx.lo[0] + 1, l1 = bx.hi[1] - bx.lo[1] + 1, l2 = bx.hi[2] - bx.lo[2] + 1;
	const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (t >= static_cast<int64_t>(l0) * l1 * l2) {
		return;
	}
	const int k = static_cast<int>(t / (static_cast<int64_t>(l0) * l1));
	const int r = static_cast<int>(t - static_cast<int64_t>(k) * l0 * l1);
	const int j = r / l0;
	const int i = r - j * l0;
	const int64_t p = cell_offset[blockIdx.y] + t; // Fortran order inside the box, boxes in order
	x0[p] = g.plo[0] + (static_cast<double>(bx.lo[0] + i) + o0) * g.dx[0];
	v0[p] = 0.0;
	if (ndim > 1) {
		x1[p] = g.plo[1] + (static_cast<double>(bx.lo[1] + j) + o1) * g.dx[1];
		v1[p] = 0.0;
	}
	if (ndim > 2) {
		x2[p] = g.plo[2] + (static_cast<double>(bx.lo[2] + k) + o2) * g.dx[2];
		v2[p] = 0.0;
	}
	id[p] = first_id + p;
	cpu[p] = rank;
}

// the periodic shift of particle p and whether it then lies inside the domain (qk_tracer_Redistribute in include/quokka_amd.h)
template <class G> QK_DEV auto shiftIntoDomain(const G &g, const int ndim, double *const (&xp)[3], const int64_t p) -> bool
{
	bool inside = true;
	for (int e = 0; e < ndim; ++e) {
		const double plo = g.plo[e], phi = g.phi[e];
		double x = xp[e][p];
		if (g.periodic[e] != 0 && !(x >= plo && x < phi)) {
			// any number of periods outside: x -= floor((x - plo) / len) * len (one period: exactly x -+ len), then the two roundings
			// that can leave the result outside by an ulp.  A NaN or an infinite position stays outside and is dropped below.
			const double len = phi - plo;
			x = x - floor((x - plo) / len) * len;
			if (x < plo || x >= phi) { // below plo, or on phi, through rounding
				x = plo;
			}
			xp[e][p] = x;
		}
		inside = inside && (x >= plo && x < phi);
	}
	return inside;
}

__global__ void __launch_bounds__(256) k_tracer_redistribute(const TracerGeom g, const int ndim, const int64_t np, double *__restrict__ x0,
							     double *__restrict__ x1, double *__restrict__ x2, unsigned char *__restrict__ keep)
{
	double *const xp[3] = {x0, x1, x2};
	for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < np; p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
		keep[p] = shiftIntoDomain(g, ndim, xp, p) ? 1 : 0;
	}
}

// does a box of level L hold a cell of [lo, hi] (cell indices inside the domain)?  A lattice entry is one box or none.
QK_DEV auto anyBoxIn(const WhereLevel &L, const int (&lo)[3], const int (&hi)[3]) -> bool
{
	int a[3], b[3];
	for (int e = 0; e < 3; ++e) {
		a[e] = latticeCoord(lo[e], L.gran[e], L.magic[e]);
		b[e] = latticeCoord(hi[e], L.gran[e], L.magic[e]);
	}
	for (int k = a[2]; k <= b[2]; ++k) {
		for (int j = a[1]; j <= b[1]; ++j) {
			for (int i = a[0]; i <= b[0]; ++i) {
				if (L.lattice[i + L.nl[0] * (j + L.nl[1] * k)] >= 0) {
					return true;
				}
			}
		}
	}
	return false;
}

// qk_tracer_Where: g is level 0's geometry (prob_lo / prob_hi / periodicity of the hierarchy)
__global__ void __launch_bounds__(256) k_tracer_where(const TracerGeom g, const WhereArgs A, const int ndim, const int64_t np, double *__restrict__ x0,
						      double *__restrict__ x1, double *__restrict__ x2, const int *__restrict__ level,
						      int *__restrict__ new_level, unsigned char *__restrict__ keep)
{
	double *const xp[3] = {x0, x1, x2};
	for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < np; p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
		const bool inside = shiftIntoDomain(g, ndim, xp, p);
		keep[p] = inside ? 1 : 0;
		if (!inside) {
			new_level[p] = -1;
			continue;
		}
		const double xs[3] = {x0[p], ndim > 1 ? x1[p] : 0.0, ndim > 2 ? x2[p] : 0.0};
		const int cur = level[p];
		int out = -1;
		int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
		if (A.ngrow > 0 && cur >= 0 && cur < A.nlev) { // (c): inside a box of its own level grown by ngrow cells
			const WhereLevel &L = A.L[cur];
			for (int e = 0; e < ndim; ++e) {
				int i = static_cast<int>(floor((xs[e] - g.plo[e]) * L.dxi[e]));
				i = i < 0 ? 0 : (i > L.n[e] - 1 ? L.n[e] - 1 : i);
				lo[e] = i - A.ngrow < 0 ? 0 : i - A.ngrow;
				hi[e] = i + A.ngrow > L.n[e] - 1 ? L.n[e] - 1 : i + A.ngrow;
			}
			if (anyBoxIn(L, lo, hi)) {
				out = cur;
			}
		}
		// (d): the finest level of [lev_min, finest] that holds the cell, else the finest one below lev_min — finest first over all levels
		for (int m = A.nlev - 1; m >= 0 && out < 0; --m) {
			const WhereLevel &L = A.L[m];
			for (int e = 0; e < ndim; ++e) {
				int i = static_cast<int>(floor((xs[e] - g.plo[e]) * L.dxi[e]));
				i = i < 0 ? 0 : (i > L.n[e] - 1 ? L.n[e] - 1 : i);
				lo[e] = hi[e] = i;
			}
			if (anyBoxIn(L, lo, hi)) {
				out = m;
			}
		}
		new_level[p] = out;
	}
}

auto particleGrid(int64_t np) -> unsigned
{
	// grid-stride: at most 8 workgroups of 256 threads per CU on 256 CUs
	return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((np + 255) / 256, 256 * 8)));
}

// allow_holes: qk_tracer_plan_create_refined (the boxes need not cover the domain)
auto planCreate(qk_level *lev, qk_tracer_plan **plan, const qk_geometry *geom, const double prob_lo[3], const double prob_hi[3], const double dx[3],
		const bool allow_holes) -> int
{
	if (lev == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = lev->ctx;
	QK_REQUIRE(ctx, plan && geom && prob_lo && prob_hi && dx, "qk_tracer_plan_create: NULL argument");
	QK_REQUIRE(ctx, geom->ndim == lev->ndim, "qk_tracer_plan_create: the geometry and the level differ in ndim");
	const int nd = lev->ndim;
	TracerGeom g{};
	int64_t domain_cells = 1;
	for (int d = 0; d < 3; ++d) {
		const bool on = d < nd;
		QK_REQUIRE(ctx, geom->domain.lo[d] == 0, "qk_tracer_plan_create: the domain must start at cell 0");
		g.n[d] = on ? geom->domain.hi[d] + 1 : 1;
		QK_REQUIRE(ctx, g.n[d] >= 1, "qk_tracer_plan_create: empty domain");
		QK_REQUIRE(ctx, !on || dx[d] > 0.0, "qk_tracer_plan_create: dx must be positive");
		if (g.n[d] >= kMaxCellsPerDir) {
			return setError(ctx, QK_ERR_UNSUPPORTED, "qk_tracer_plan_create: 32768 cells or more in one direction");
		}
		g.plo[d] = on ? prob_lo[d] : 0.0;
		g.phi[d] = on ? prob_hi[d] : 1.0;
		g.dx[d] = on ? dx[d] : 1.0;
		g.dxi[d] = 1.0 / g.dx[d];
		g.periodic[d] = (on && geom->periodic[d] != 0) ? 1 : 0;
		domain_cells *= g.n[d];
	}
	// granularity: the common divisor of every box edge (and of the domain length)
	int64_t box_cells = 0;
	for (int d = 0; d < 3; ++d) {
		int gd = g.n[d];
		for (const qk_box &b : lev->boxes) {
			if (b.lo[d] < 0 || b.hi[d] >= g.n[d] || b.hi[d] < b.lo[d]) {
				return setError(ctx, QK_ERR_UNSUPPORTED, "qk_tracer_plan_create: a box reaches outside the domain");
			}
			gd = std::gcd(gd, std::gcd(b.lo[d], b.hi[d] + 1));
		}
		g.gran[d] = gd;
		g.nl[d] = g.n[d] / gd;
		g.magic[d] = gd >= 2 ? static_cast<unsigned>(((1ULL << 32) + static_cast<unsigned>(gd) - 1) / static_cast<unsigned>(gd)) : 0U;
	}
	for (const qk_box &b : lev->boxes) {
		box_cells += static_cast<int64_t>(b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1) * (b.hi[2] - b.lo[2] + 1);
	}
	if (box_cells != domain_cells && !allow_holes) {
		return setError(ctx, QK_ERR_UNSUPPORTED, "qk_tracer_plan_create: the level's boxes do not tile the domain (a refined level, or boxes of other ranks)");
	}
	const int64_t nlat = static_cast<int64_t>(g.nl[0]) * g.nl[1] * g.nl[2];
	if (nlat > (int64_t(1) << 28)) {
		return setError(ctx, QK_ERR_UNSUPPORTED, "qk_tracer_plan_create: the box lattice has more than 2^28 entries");
	}
	g.nlat = static_cast<int>(nlat);
	auto *P = new qk_tracer_plan;
	P->lev = lev;
	P->g = g;
	P->lattice.assign(static_cast<size_t>(nlat), -1);
	P->cell_offset.assign(lev->boxes.size() + 1, 0);
	for (size_t b = 0; b < lev->boxes.size(); ++b) {
		const qk_box &bx = lev->boxes[b];
		P->cell_offset[b + 1] = P->cell_offset[b] + static_cast<int64_t>(bx.hi[0] - bx.lo[0] + 1) * (bx.hi[1] - bx.lo[1] + 1) * (bx.hi[2] - bx.lo[2] + 1);
		for (int lk = bx.lo[2] / g.gran[2]; lk <= bx.hi[2] / g.gran[2]; ++lk) {
			for (int lj = bx.lo[1] / g.gran[1]; lj <= bx.hi[1] / g.gran[1]; ++lj) {
				for (int li = bx.lo[0] / g.gran[0]; li <= bx.hi[0] / g.gran[0]; ++li) {
					int &slot = P->lattice[li + static_cast<size_t>(g.nl[0]) * (lj + static_cast<size_t>(g.nl[1]) * lk)];
					if (slot != -1) { // two boxes overlap (the cell counts matched by accident)
						delete P;
						return setError(ctx, QK_ERR_UNSUPPORTED, "qk_tracer_plan_create: the level's boxes overlap");
					}
					slot = static_cast<int>(b);
				}
			}
		}
	}
	// (equal cell counts and no overlap: every lattice entry is set; a refined level's plan keeps -1 where it has no box)
	P->holes = std::find(P->lattice.begin(), P->lattice.end(), -1) != P->lattice.end();
	if (ctx->device >= 0) {
		hipError_t e = hipMalloc(reinterpret_cast<void **>(&P->d_lattice), sizeof(int) * static_cast<size_t>(nlat));
		if (e == hipSuccess) {
			e = hipMemcpy(P->d_lattice, P->lattice.data(), sizeof(int) * static_cast<size_t>(nlat), hipMemcpyHostToDevice);
		}
		if (e == hipSuccess) {
			e = hipMalloc(reinterpret_cast<void **>(&P->d_cell_offset), sizeof(int64_t) * P->cell_offset.size());
		}
		if (e == hipSuccess) {
			e = hipMemcpy(P->d_cell_offset, P->cell_offset.data(), sizeof(int64_t) * P->cell_offset.size(), hipMemcpyHostToDevice);
		}
		if (e != hipSuccess) {
			(void)hipFree(P->d_lattice);
			(void)hipFree(P->d_cell_offset);
			delete P;
			return setError(ctx, QK_ERR_HIP, "qk_tracer_plan_create", hipGetErrorString(e));
		}
	}
	*plan = P;
	return QK_OK;
}

// the ancestors of `plan` as the deferred kernel reads them; false: a link is missing or the chain is deeper than kMaxDepth
auto buildChain(const qk_tracer_plan *plan, TracerChain &c) -> bool
{
	c = TracerChain{};
	c.alpha = plan->alpha;
	c.beta = plan->beta;
	for (int kind = 0; kind < 2; ++kind) {
		const qk_tracer_plan *q = plan;
		for (int k = 0;; ++k) {
			const qk_tracer_plan::Link &lk = q->link[kind];
			if (k == kMaxDepth || lk.parent == nullptr) {
				return false;
			}
			TracerLink &e = c.e[kind][k];
			for (int d = 0; d < 3; ++d) {
				e.n[d] = lk.parent->g.n[d];
				e.periodic[d] = lk.parent->g.periodic[d];
				e.gran[d] = lk.parent->g.gran[d];
				e.magic[d] = lk.parent->g.magic[d];
				e.nl[d] = lk.parent->g.nl[d];
				e.u[d] = lk.u[d];
			}
			e.lattice = lk.parent->d_lattice;
			if (!lk.parent->holes) {
				break;
			}
			q = lk.parent;
		}
	}
	return true;
}

} // namespace

extern "C" {

int qk_tracer_plan_create(qk_level *lev, qk_tracer_plan **plan, const qk_geometry *geom, const double prob_lo[3], const double prob_hi[3], const double dx[3])
{
	return planCreate(lev, plan, geom, prob_lo, prob_hi, dx, false);
}

int qk_tracer_plan_create_refined(qk_level *lev, qk_tracer_plan **plan, const qk_geometry *geom, const double prob_lo[3], const double prob_hi[3],
				  const double dx[3])
{
	return planCreate(lev, plan, geom, prob_lo, prob_hi, dx, true);
}

int qk_tracer_plan_set_parent(qk_tracer_plan *plan, int kind, qk_tracer_plan *parent, const qk_array4 *const parent_umac[3])
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = plan->lev->ctx;
	const int nd = plan->lev->ndim;
	QK_REQUIRE(ctx, (kind == QK_TRACER_PREV || kind == QK_TRACER_CUR) && parent && parent_umac && parent != plan, "tracer_plan_set_parent: bad argument");
	QK_REQUIRE(ctx, parent->lev->ndim == nd && parent->lev->ctx == ctx, "tracer_plan_set_parent: the parent plan is of another context or ndim");
	for (int d = 0; d < nd; ++d) {
		QK_REQUIRE(ctx, parent_umac[d], "tracer_plan_set_parent: NULL face table");
		QK_REQUIRE(ctx, 2 * parent->g.n[d] == plan->g.n[d] && parent->g.periodic[d] == plan->g.periodic[d],
			   "tracer_plan_set_parent: the parent's domain is not this level's coarsened by 2");
	}
	plan->link[kind].parent = parent;
	for (int d = 0; d < 3; ++d) {
		plan->link[kind].u[d] = d < nd ? parent_umac[d] : nullptr;
	}
	return QK_OK;
}

int qk_tracer_plan_set_time_weights(qk_tracer_plan *plan, double alpha, double beta)
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(plan->lev->ctx, alpha != 0.0 || beta != 0.0, "tracer_plan_set_time_weights: both weights are zero");
	plan->alpha = alpha;
	plan->beta = beta;
	return QK_OK;
}

int qk_tracer_plan_clear_parent(qk_tracer_plan *plan)
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
	plan->link[0] = plan->link[1] = qk_tracer_plan::Link{};
	plan->alpha = 0.0;
	plan->beta = 1.0;
	return QK_OK;
}

int qk_tracer_plan_destroy(qk_tracer_plan *plan)
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
	(void)hipFree(plan->d_defer);
	(void)hipFree(plan->d_lattice);
	(void)hipFree(plan->d_cell_offset);
	delete plan;
	return QK_OK;
}

int qk_tracer_plan_lattice(qk_tracer_plan *plan, int granularity[3], int64_t *nentries)
{
	if (plan == nullptr || granularity == nullptr || nentries == nullptr) {
		return QK_ERR_INVALID;
	}
	for (int d = 0; d < 3; ++d) {
		granularity[d] = plan->g.gran[d];
	}
	*nentries = plan->g.nlat;
	return QK_OK;
}

int qk_tracer_InitOnePerCell(qk_tracer_plan *plan, qk_stream s, const double off[3], double *const pos[3], double *const vel[3], int64_t *id, int *cpu,
			     int64_t first_id, int rank)
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_level *lev = plan->lev;
	qk_ctx *ctx = lev->ctx;
	const int nd = lev->ndim;
	QK_REQUIRE(ctx, off && pos && vel && id && cpu, "tracer_InitOnePerCell: NULL argument");
	for (int d = 0; d < nd; ++d) {
		QK_REQUIRE(ctx, pos[d] && vel[d], "tracer_InitOnePerCell: NULL particle array");
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "tracer_InitOnePerCell: planning-only context");
	if (lev->nboxes == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	const CellLaunch L = cellLaunch(lev, 0, -1);
	ProfScope prof(ctx, st, "tracer_InitOnePerCell");
	hipLaunchKernelGGL(k_tracer_init, L.grid, L.block, 0, st, plan->g, nd, lev->d_boxes, plan->d_cell_offset, off[0], off[1], off[2], pos[0],
			   nd > 1 ? pos[1] : nullptr, nd > 2 ? pos[2] : nullptr, vel[0], nd > 1 ? vel[1] : nullptr, nd > 2 ? vel[2] : nullptr, id, cpu, first_id,
			   rank);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_tracer_AdvectWithUmac(qk_tracer_plan *plan, qk_stream s, const qk_array4 *const umac[3], double dt, int64_t np, double *const pos[3],
			     double *const vel[3])
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_level *lev = plan->lev;
	qk_ctx *ctx = lev->ctx;
	const int nd = lev->ndim;
	QK_REQUIRE(ctx, umac && pos && vel && np >= 0, "tracer_AdvectWithUmac: NULL argument");
	for (int d = 0; d < nd; ++d) {
		QK_REQUIRE(ctx, umac[d] && pos[d] && vel[d], "tracer_AdvectWithUmac: NULL array");
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "tracer_AdvectWithUmac: planning-only context");
	if (np == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	const dim3 grid(particleGrid(np)), block(256);
	const bool lds = plan->g.nlat <= kMaxLdsLattice;
	TracerChain chain{};
	if (plan->holes) { // a refined level: faces outside its boxes come from the parent chain
		if (!buildChain(plan, chain)) {
			return setError(ctx, QK_ERR_UNSUPPORTED,
					"tracer_AdvectWithUmac: the level's boxes do not tile the domain and the plan has no parent link down to a level that does "
					"(qk_tracer_plan_set_parent, at most QK_TRACER_MAX_DEPTH deep)");
		}
		if (np > plan->defer_cap) {
			(void)hipFree(plan->d_defer);
			plan->d_defer = nullptr;
			plan->defer_cap = 0;
			QK_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void **>(&plan->d_defer), static_cast<size_t>(np)));
			plan->defer_cap = np;
		}
	}
	unsigned char *defer = plan->d_defer;
	const qk_array4 *u1 = nd > 1 ? umac[1] : nullptr, *u2 = nd > 2 ? umac[2] : nullptr;
	double *x1 = nd > 1 ? pos[1] : nullptr, *x2 = nd > 2 ? pos[2] : nullptr, *v1 = nd > 1 ? vel[1] : nullptr, *v2 = nd > 2 ? vel[2] : nullptr;
	ProfScope prof(ctx, st, "tracer_AdvectWithUmac");
#define QK_TRACER_LAUNCH(ND, LDS)                                                                                                                    \
	do {                                                                                                                                             \
		if (plan->holes) {                                                                                                                       \
			hipLaunchKernelGGL((k_tracer_advect<ND, LDS, true>), grid, block, 0, st, plan->g, plan->d_lattice, umac[0], u1, u2, dt, np, pos[0], x1, \
					   x2, vel[0], v1, v2, defer);                                                                                   \
			hipLaunchKernelGGL((k_tracer_advect_deferred<ND>), grid, block, 0, st, plan->g, plan->d_lattice, umac[0], u1, u2, chain, dt, np,   \
					   pos[0], x1, x2, vel[0], v1, v2, defer);                                                                       \
		} else {                                                                                                                                 \
			hipLaunchKernelGGL((k_tracer_advect<ND, LDS, false>), grid, block, 0, st, plan->g, plan->d_lattice, umac[0], u1, u2, dt, np, pos[0], x1, \
					   x2, vel[0], v1, v2, defer);                                                                                   \
		}                                                                                                                                        \
	} while (0)
	if (nd == 3) {
		if (lds) {
			QK_TRACER_LAUNCH(3, true);
		} else {
			QK_TRACER_LAUNCH(3, false);
		}
	} else if (nd == 2) {
		if (lds) {
			QK_TRACER_LAUNCH(2, true);
		} else {
			QK_TRACER_LAUNCH(2, false);
		}
	} else {
		if (lds) {
			QK_TRACER_LAUNCH(1, true);
		} else {
			QK_TRACER_LAUNCH(1, false);
		}
	}
#undef QK_TRACER_LAUNCH
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_tracer_Redistribute(qk_tracer_plan *plan, qk_stream s, int64_t np, double *const pos[3], unsigned char *keep)
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_level *lev = plan->lev;
	qk_ctx *ctx = lev->ctx;
	const int nd = lev->ndim;
	QK_REQUIRE(ctx, pos && keep && np >= 0, "tracer_Redistribute: NULL argument");
	for (int d = 0; d < nd; ++d) {
		QK_REQUIRE(ctx, pos[d], "tracer_Redistribute: NULL position array");
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "tracer_Redistribute: planning-only context");
	if (np == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "tracer_Redistribute");
	hipLaunchKernelGGL(k_tracer_redistribute, dim3(particleGrid(np)), dim3(256), 0, st, plan->g, nd, np, pos[0], nd > 1 ? pos[1] : nullptr,
			   nd > 2 ? pos[2] : nullptr, keep);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_tracer_Where(qk_tracer_plan *const plans[], int nlevels, qk_stream s, int lev_min, int ngrow, int64_t np, double *const pos[3], const int *level,
		    int *new_level, unsigned char *keep)
{
	if (plans == nullptr || nlevels < 1 || plans[0] == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = plans[0]->lev->ctx;
	const int nd = plans[0]->lev->ndim;
	QK_REQUIRE(ctx, pos && level && new_level && keep && np >= 0, "tracer_Where: NULL argument");
	QK_REQUIRE(ctx, lev_min >= 0 && lev_min < nlevels && ngrow >= 0, "tracer_Where: lev_min or ngrow out of range");
	if (nlevels > kMaxDepth + 1) {
		return setError(ctx, QK_ERR_UNSUPPORTED, "tracer_Where: more than QK_TRACER_MAX_DEPTH + 1 levels");
	}
	QK_REQUIRE(ctx, !plans[0]->holes, "tracer_Where: level 0 must tile the domain");
	for (int d = 0; d < nd; ++d) {
		QK_REQUIRE(ctx, pos[d], "tracer_Where: NULL position array");
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "tracer_Where: planning-only context");
	WhereArgs A{};
	A.nlev = nlevels;
	A.ngrow = ngrow;
	for (int m = 0; m < nlevels; ++m) {
		QK_REQUIRE(ctx, plans[m] && plans[m]->lev->ndim == nd && plans[m]->lev->ctx == ctx, "tracer_Where: bad plan");
		const TracerGeom &g = plans[m]->g;
		for (int d = 0; d < 3; ++d) {
			A.L[m].dxi[d] = g.dxi[d];
			A.L[m].n[d] = g.n[d];
			A.L[m].gran[d] = g.gran[d];
			A.L[m].magic[d] = g.magic[d];
			A.L[m].nl[d] = g.nl[d];
		}
		A.L[m].lattice = plans[m]->d_lattice;
	}
	if (np == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "tracer_Where");
	hipLaunchKernelGGL(k_tracer_where, dim3(particleGrid(np)), dim3(256), 0, st, plans[0]->g, A, nd, np, pos[0], nd > 1 ? pos[1] : nullptr,
			   nd > 2 ? pos[2] : nullptr, level, new_level, keep);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

} // extern "C"
