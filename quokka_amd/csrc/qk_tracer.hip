// qk_tracer.hip — tracer particles on one level and one rank (include/quokka_amd.h "tracer particles"):
//   qk_tracer_plan_create      the cell -> box lattice of a BoxArray that tiles the domain
//   qk_tracer_InitOnePerCell   one particle per valid cell                              (reference src/simulation.hpp:1993-2005)
//   qk_tracer_AdvectWithUmac   AMReX's predictor-corrector MAC advection, both passes    (reference src/QuokkaSimulation.hpp:1290-1314)
//   qk_tracer_Redistribute     periodic shift / drop beyond non-periodic faces           (reference src/simulation.hpp:1317-1329)
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

} // namespace

struct qk_tracer_plan {
	qk_level *lev = nullptr;
	TracerGeom g{};
	std::vector<int> lattice;	  // host copy: lattice cell -> box index, x fastest
	std::vector<int64_t> cell_offset; // number of valid cells in the boxes before box b (nboxes + 1 entries)
	int *d_lattice = nullptr;
	int64_t *d_cell_offset = nullptr;
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
template <int NDIM, int D, class LAT> QK_DEV auto interpMac(const TracerGeom &g, LAT lat, const qk_array4 *__restrict__ u_t, const double (&x)[3]) -> double
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

template <int NDIM, class LAT>
QK_DEV void interpAll(const TracerGeom &g, LAT lat, const qk_array4 *u0, const qk_array4 *u1, const qk_array4 *u2, const double (&x)[3], double (&v)[3])
{
	v[0] = interpMac<NDIM, 0>(g, lat, u0, x);
	if constexpr (NDIM > 1) {
		v[1] = interpMac<NDIM, 1>(g, lat, u1, x);
	}
	if constexpr (NDIM > 2) {
		v[2] = interpMac<NDIM, 2>(g, lat, u2, x);
	}
}

// one thread per particle, grid-stride.  LDS_LAT: the lattice is staged in LDS (nlat <= kMaxLdsLattice), else read from global memory.
template <int NDIM, bool LDS_LAT>
__global__ void __launch_bounds__(256) k_tracer_advect(const TracerGeom g, const int *__restrict__ d_lattice, const qk_array4 *__restrict__ u0,
						       const qk_array4 *__restrict__ u1, const qk_array4 *__restrict__ u2, const double dt, const int64_t np,
						       double *__restrict__ x0, double *__restrict__ x1, double *__restrict__ x2, double *__restrict__ v0,
						       double *__restrict__ v1, double *__restrict__ v2)
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
		if constexpr (LDS_LAT) {
			interpAll<NDIM>(g, s_lat, u0, u1, u2, x, va);
		} else {
			interpAll<NDIM>(g, d_lattice, u0, u1, u2, x, va);
		}
#pragma unroll
		for (int e = 0; e < NDIM; ++e) {
			xm[e] = x[e] + hdt * va[e];
		}
		if constexpr (LDS_LAT) {
			interpAll<NDIM>(g, s_lat, u0, u1, u2, xm, vb);
		} else {
			interpAll<NDIM>(g, d_lattice, u0, u1, u2, xm, vb);
		}
#pragma unroll
		for (int e = 0; e < NDIM; ++e) {
			xp[e][p] = x[e] + dt * vb[e];
			vp[e][p] = vb[e];
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

__global__ void __launch_bounds__(256) k_tracer_redistribute(const TracerGeom g, const int ndim, const int64_t np, double *__restrict__ x0,
							     double *__restrict__ x1, double *__restrict__ x2, unsigned char *__restrict__ keep)
{
	double *const xp[3] = {x0, x1, x2};
	for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < np; p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
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
		keep[p] = inside ? 1 : 0;
	}
}

auto particleGrid(int64_t np) -> unsigned
{
	// grid-stride: at most 8 workgroups of 256 threads per CU on 256 CUs
	return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((np + 255) / 256, 256 * 8)));
}

} // namespace

extern "C" {

int qk_tracer_plan_create(qk_level *lev, qk_tracer_plan **plan, const qk_geometry *geom, const double prob_lo[3], const double prob_hi[3], const double dx[3])
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
	if (box_cells != domain_cells) {
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
	// (equal cell counts and no overlap: every lattice entry is set)
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

int qk_tracer_plan_destroy(qk_tracer_plan *plan)
{
	if (plan == nullptr) {
		return QK_ERR_INVALID;
	}
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
	const qk_array4 *u1 = nd > 1 ? umac[1] : nullptr, *u2 = nd > 2 ? umac[2] : nullptr;
	double *x1 = nd > 1 ? pos[1] : nullptr, *x2 = nd > 2 ? pos[2] : nullptr, *v1 = nd > 1 ? vel[1] : nullptr, *v2 = nd > 2 ? vel[2] : nullptr;
	ProfScope prof(ctx, st, "tracer_AdvectWithUmac");
#define QK_TRACER_LAUNCH(ND, LDS)                                                                                                                    \
	hipLaunchKernelGGL((k_tracer_advect<ND, LDS>), grid, block, 0, st, plan->g, plan->d_lattice, umac[0], u1, u2, dt, np, pos[0], x1, x2, vel[0], v1, v2)
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

} // extern "C"
