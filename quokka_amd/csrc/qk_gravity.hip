// qk_gravity.hip — self-gravity on one level and one rank, 3-D, cubic cells (include/quokka_amd.h "self-gravity"):
//   qk_gravity_fill_rhs            f += 4 pi G rho into the dense array             (reference src/QuokkaSimulation.hpp:709-722)
//   qk_gravity_dirichlet_solve     L phi = f, Dirichlet data in the ghost layer: geometric multigrid, cell-centred
//   qk_gravity_surface_gather      s(g) = phi0(nb(g))                               (James' method, step 2)
//   qk_gravity_surface_potential   bc(g) = - sum_g' K(g - g') s(g')                 (step 3: the S^2 kernel)
//   qk_gravity_surface_scatter     ghost layer of phi <- bc
//   qk_gravity_kick                the operator-split kick                          (reference src/QuokkaSimulation.hpp:724-757)
// The reference hands the open-boundary solve to amrex::OpenBCSolver (src/simulation.hpp:1011-1069), whose sources are not part of it; the
// discrete problem solved here is this project's definition and is restated in numpy by tests/gravity_reference.py.
// Every kernel step is one ordinary launch; nothing waits on another workgroup.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "qk_device.hpp"
#include "qk_gravity_index.hpp"
#include "qk_internal.hpp"

using namespace qk;
using qk::gravity::Dims;

namespace
{

constexpr int kMaxMgLevels = 24;
constexpr int kPreSmooth = 2, kPostSmooth = 2; // red-black pairs
constexpr int kBottomSweeps = 24;	       // red-black pairs on the coarsest level
constexpr int kTailCells = 4096;	       // levels of at most this many cells (16^3) are taken together in one single-workgroup launch
constexpr int kTailThreads = 1024;
constexpr int kMaxTailLevels = 8;	       // (more levels than this below the first small one — a very elongated domain —: the tail starts further down)
constexpr int kSurfTile = 256;		       // sources per LDS tile == targets per workgroup
constexpr int kSurfMaxParts = 64;	       // the source list is cut into at most this many parts (one partial sum each)

// one multigrid level as the kernels see it (by value: scalar registers)
struct MgGeom {
	int n[3];
	double a[3];	 // 1 / h_d^2
	double c[3];	 // value of a cell beyond the domain face in direction d as a multiple of the cell inside: (theta - 1) / theta, where theta h_d is
			 // the distance from the first cell centre to the plane on which the level-0 ghost centres lie
	int ghost_data;	 // level 0: the ghost layer of u holds the Dirichlet data and is read instead
	int64_t sx, sy;	 // strides of the dense array (ghost layer included on every level)
};

struct MgLevel {
	MgGeom g{};
	int coarsen[3] = {0, 0, 0}; // the step from this level to the next halves direction d
	int64_t ncell = 0, size = 0;
	double *u = nullptr, *f = nullptr, *r = nullptr;
};

auto buildLevels(const int n[3], double h, std::vector<MgLevel> &lv) -> void
{
	lv.clear();
	MgLevel L;
	double hd[3], dist[3]; // spacing; distance of the first cell centre from the Dirichlet plane
	for (int d = 0; d < 3; ++d) {
		L.g.n[d] = n[d];
		hd[d] = h;
		dist[d] = h;
	}
	for (int l = 0; l < kMaxMgLevels; ++l) {
		for (int d = 0; d < 3; ++d) {
			L.g.a[d] = 1.0 / (hd[d] * hd[d]);
			const double theta = dist[d] / hd[d];
			L.g.c[d] = (theta - 1.0) / theta;
		}
		L.g.ghost_data = l == 0 ? 1 : 0;
		L.g.sx = L.g.n[0] + 2;
		L.g.sy = static_cast<int64_t>(L.g.n[0] + 2) * (L.g.n[1] + 2);
		L.ncell = static_cast<int64_t>(L.g.n[0]) * L.g.n[1] * L.g.n[2];
		L.size = static_cast<int64_t>(L.g.n[0] + 2) * (L.g.n[1] + 2) * (L.g.n[2] + 2);
		bool any = false;
		for (int d = 0; d < 3; ++d) {
			L.coarsen[d] = (L.g.n[d] % 2 == 0 && L.g.n[d] >= 4) ? 1 : 0;
			any = any || L.coarsen[d] != 0;
		}
		if (!any || l == kMaxMgLevels - 1) {
			L.coarsen[0] = L.coarsen[1] = L.coarsen[2] = 0;
			lv.push_back(L);
			break;
		}
		lv.push_back(L);
		for (int d = 0; d < 3; ++d) {
			if (L.coarsen[d] != 0) {
				L.g.n[d] /= 2;
				dist[d] += 0.5 * hd[d];
				hd[d] *= 2.0;
			}
		}
	}
}

constexpr int64_t kWordsBytes = 64; // device words at the head of the scratch: [0] max |f|, [1] key of min f, [2] max |residual|

auto mgScratchBytes(const std::vector<MgLevel> &lv) -> int64_t
{
	int64_t nd = lv[0].size; // r of level 0
	for (size_t l = 1; l < lv.size(); ++l) {
		nd += 3 * lv[l].size;
	}
	return kWordsBytes + 8 * nd;
}

struct SurfSplit {
	int64_t S;
	int ntile, tiles_per_part, nparts;
};

auto surfSplit(const int n[3]) -> SurfSplit
{
	const Dims D{{n[0], n[1], n[2]}};
	SurfSplit sp{};
	sp.S = gravity::numGhosts(D);
	sp.ntile = static_cast<int>((sp.S + kSurfTile - 1) / kSurfTile);
	// enough workgroups to fill the device at the sizes of the reference's gravity decks: about 2048, each part at least one tile
	const int want = std::max(1, std::min(kSurfMaxParts, 2048 / std::max(sp.ntile, 1)));
	sp.tiles_per_part = (sp.ntile + want - 1) / want;
	sp.nparts = (sp.ntile + sp.tiles_per_part - 1) / sp.tiles_per_part;
	return sp;
}

auto checkDims(qk_ctx *ctx, const int n[3], const char *who) -> int
{
	if (n == nullptr) {
		return setError(ctx, QK_ERR_INVALID, who, "n is NULL");
	}
	for (int d = 0; d < 3; ++d) {
		if (n[d] < 4 || n[d] % 2 != 0 || n[d] > 4096) {
			return setError(ctx, QK_ERR_UNSUPPORTED, who, "self-gravity needs an even cell count of 4 .. 4096 in every direction");
		}
	}
	return QK_OK;
}

// ---------------------------------------------------------------------------------------------------------------- reductions
// order-preserving key of a double (any sign) for atomicMin / atomicMax on 64-bit words
QK_DEV auto orderedKey(double v) -> unsigned long long
{
	const auto b = static_cast<unsigned long long>(__double_as_longlong(v));
	return (b >> 63) != 0 ? ~b : (b | 0x8000000000000000ULL);
}
auto keyToDouble(unsigned long long k) -> double
{
	const unsigned long long b = (k >> 63) != 0 ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
	double v;
	std::memcpy(&v, &b, sizeof v);
	return v;
}

// max over the workgroup of a non-negative value (a NaN counts as +inf: an unconverged or invalid field must never look small)
QK_DEV auto blockMaxNonNeg(double v, double *s_red) -> double
{
	if (!(v == v)) {
		v = __builtin_inf();
	}
	s_red[threadIdx.x] = v;
	__syncthreads();
	for (int w = blockDim.x / 2; w > 0; w >>= 1) {
		if (static_cast<int>(threadIdx.x) < w) {
			s_red[threadIdx.x] = fmax(s_red[threadIdx.x], s_red[threadIdx.x + w]);
		}
		__syncthreads();
	}
	return s_red[0];
}

// words[0] = max |f|, words[1] = key of min f over the interior cells
__global__ void __launch_bounds__(256) k_grav_norms(const MgGeom g, const int64_t ncell, const double *__restrict__ f, unsigned long long *__restrict__ words)
{
	__shared__ double s_red[256];
	__shared__ unsigned long long s_min[256];
	double mx = 0.0;
	unsigned long long mn = ~0ULL;
	for (int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; c < ncell; c += static_cast<int64_t>(gridDim.x) * blockDim.x) {
		const int i = static_cast<int>(c % g.n[0]);
		const int64_t t = c / g.n[0];
		const int j = static_cast<int>(t % g.n[1]), k = static_cast<int>(t / g.n[1]);
		const double v = f[(i + 1) + g.sx * (j + 1) + g.sy * (k + 1)];
		const double av = fabs(v);
		mx = (av == av) ? fmax(mx, av) : __builtin_inf();
		const unsigned long long key = orderedKey(v);
		mn = key < mn ? key : mn;
	}
	const double bm = blockMaxNonNeg(mx, s_red);
	s_min[threadIdx.x] = mn;
	__syncthreads();
	for (int w = blockDim.x / 2; w > 0; w >>= 1) {
		if (static_cast<int>(threadIdx.x) < w) {
			const unsigned long long o = s_min[threadIdx.x + w];
			if (o < s_min[threadIdx.x]) {
				s_min[threadIdx.x] = o;
			}
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		atomicMax(&words[0], static_cast<unsigned long long>(__double_as_longlong(bm)));
		atomicMin(&words[1], s_min[0]);
	}
}

// ---------------------------------------------------------------------------------------------------------------- multigrid kernels
// sum of a_d * neighbour over the neighbours that exist (inside the domain, or the ghost layer of level 0) and the diagonal of -L
QK_DEV void stencil(const MgGeom &g, const double *__restrict__ u, int i, int j, int k, int64_t idx, double &sum, double &diag)
{
	const int ijk[3] = {i, j, k};
	const int64_t st[3] = {1, g.sx, g.sy};
	sum = 0.0;
	diag = 0.0;
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		const bool lo_in = ijk[d] > 0 || g.ghost_data != 0;
		const bool hi_in = ijk[d] < g.n[d] - 1 || g.ghost_data != 0;
		// a cell beyond the face counts as c_d * u(centre): it moves to the diagonal
		const double um = lo_in ? u[idx - st[d]] : 0.0;
		const double up = hi_in ? u[idx + st[d]] : 0.0;
		sum = sum + g.a[d] * (um + up);
		diag = diag + g.a[d] * ((lo_in ? 1.0 : 1.0 - g.c[d]) + (hi_in ? 1.0 : 1.0 - g.c[d]));
	}
}

QK_DEV auto cellOf(const MgGeom &g, int64_t c, int &i, int &j, int &k) -> int64_t
{
	i = static_cast<int>(c % g.n[0]);
	const int64_t t = c / g.n[0];
	j = static_cast<int>(t % g.n[1]);
	k = static_cast<int>(t / g.n[1]);
	return (i + 1) + g.sx * (j + 1) + g.sy * (k + 1);
}

// The per-cell steps (c: the linear index of an interior cell of the level they run on), shared by the one-thread-per-cell kernels of the large levels
// and the single-workgroup kernel of the small ones.

// one colour of a red-black Gauss-Seidel sweep
QK_DEV void smoothCell(const MgGeom &g, int64_t c, double *__restrict__ u, const double *__restrict__ f, int colour)
{
	int i, j, k;
	const int64_t idx = cellOf(g, c, i, j, k);
	if (((i + j + k) & 1) != colour) {
		return;
	}
	double sum, diag;
	stencil(g, u, i, j, k, idx, sum, diag);
	u[idx] = (sum - f[idx]) / diag;
}

// r = f - L u; returns it
QK_DEV auto residualCell(const MgGeom &g, int64_t c, const double *__restrict__ u, const double *__restrict__ f, double *__restrict__ r) -> double
{
	int i, j, k;
	const int64_t idx = cellOf(g, c, i, j, k);
	double sum, diag;
	stencil(g, u, i, j, k, idx, sum, diag);
	const double res = f[idx] - (sum - diag * u[idx]);
	r[idx] = res;
	return res;
}

// f_coarse = mean of r_fine over the children, u_coarse = 0 (c: a coarse cell)
QK_DEV void restrictCell(const MgGeom &gf, const MgGeom &gc, int c0, int c1, int c2, int64_t c, const double *__restrict__ r_f, double *__restrict__ f_c,
			 double *__restrict__ u_c)
{
	int I, J, K;
	const int64_t idx = cellOf(gc, c, I, J, K);
	const int i0 = c0 != 0 ? 2 * I : I, j0 = c1 != 0 ? 2 * J : J, k0 = c2 != 0 ? 2 * K : K;
	double acc = 0.0;
	for (int kk = 0; kk <= c2; ++kk) {
		for (int jj = 0; jj <= c1; ++jj) {
			for (int ii = 0; ii <= c0; ++ii) {
				acc = acc + r_f[(i0 + ii + 1) + gf.sx * (j0 + jj + 1) + gf.sy * (k0 + kk + 1)];
			}
		}
	}
	const int nchild = (1 + c0) * (1 + c1) * (1 + c2);
	f_c[idx] = acc / static_cast<double>(nchild);
	u_c[idx] = 0.0;
}

// u_fine += P u_coarse: linear in every halved direction (weights 3/4, 1/4), a coarse cell beyond the face counting as c_d * (the cell inside)
// (c: a fine cell)
QK_DEV void prolongCell(const MgGeom &gf, const MgGeom &gc, int c0, int c1, int c2, int64_t c, const double *__restrict__ u_c, double *__restrict__ u_f)
{
	int ijk[3];
	const int64_t idx = cellOf(gf, c, ijk[0], ijk[1], ijk[2]);
	const int co[3] = {c0, c1, c2};
	int ci[3][2];
	double w[3][2];
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		if (co[d] == 0) {
			ci[d][0] = ci[d][1] = ijk[d];
			w[d][0] = 1.0;
			w[d][1] = 0.0;
		} else {
			const int I = ijk[d] >> 1;
			int nb = (ijk[d] & 1) != 0 ? I + 1 : I - 1;
			double wn = 0.25;
			if (nb < 0 || nb >= gc.n[d]) { // beyond the face: c_d times the cell inside
				nb = I;
				wn = 0.25 * gc.c[d];
			}
			ci[d][0] = I;
			ci[d][1] = nb;
			w[d][0] = 0.75;
			w[d][1] = wn;
		}
	}
	double acc = 0.0;
#pragma unroll
	for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
		for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
			for (int ii = 0; ii < 2; ++ii) {
				const double ww = (w[0][ii] * w[1][jj]) * w[2][kk];
				acc = acc + ww * u_c[(ci[0][ii] + 1) + gc.sx * (ci[1][jj] + 1) + gc.sy * (ci[2][kk] + 1)];
			}
		}
	}
	u_f[idx] = u_f[idx] + acc;
}

__global__ void __launch_bounds__(256) k_mg_smooth(const MgGeom g, const int64_t ncell, double *__restrict__ u, const double *__restrict__ f, const int colour)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (c < ncell) {
		smoothCell(g, c, u, f, colour);
	}
}

// norm (optional): max |r| through an atomic max on the bit pattern
__global__ void __launch_bounds__(256) k_mg_residual(const MgGeom g, const int64_t ncell, const double *__restrict__ u, const double *__restrict__ f,
						     double *__restrict__ r, unsigned long long *__restrict__ norm)
{
	__shared__ double s_red[256];
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	const double res = c < ncell ? residualCell(g, c, u, f, r) : 0.0;
	if (norm != nullptr) { // (uniform over the launch)
		const double bm = blockMaxNonNeg(fabs(res), s_red);
		if (threadIdx.x == 0) {
			atomicMax(norm, static_cast<unsigned long long>(__double_as_longlong(bm)));
		}
	}
}

__global__ void __launch_bounds__(256) k_mg_restrict(const MgGeom gf, const MgGeom gc, const int c0, const int c1, const int c2, const int64_t ncell_c,
						     const double *__restrict__ r_f, double *__restrict__ f_c, double *__restrict__ u_c)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (c < ncell_c) {
		restrictCell(gf, gc, c0, c1, c2, c, r_f, f_c, u_c);
	}
}

__global__ void __launch_bounds__(256) k_mg_prolong(const MgGeom gf, const MgGeom gc, const int c0, const int c1, const int c2, const int64_t ncell_f,
						    const double *__restrict__ u_c, double *__restrict__ u_f)
{
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (c < ncell_f) {
		prolongCell(gf, gc, c0, c1, c2, c, u_c, u_f);
	}
}

// The small levels — from the first one of at most kTailCells cells down to the coarsest — in ONE single-workgroup launch: the same V-cycle steps in the
// same order as the per-level launches (so the same values), separated by workgroup barriers only.  The first level of the tail holds f and u = 0.
struct MgTail {
	int nlev;
	MgGeom g[kMaxTailLevels];
	int coarsen[kMaxTailLevels][3];
	int ncell[kMaxTailLevels];
	double *u[kMaxTailLevels], *f[kMaxTailLevels], *r[kMaxTailLevels];
};

QK_DEV void tailSmooth(const MgGeom &g, int ncell, double *u, const double *f, int npairs)
{
	for (int s = 0; s < 2 * npairs; ++s) {
		for (int c = threadIdx.x; c < ncell; c += blockDim.x) {
			smoothCell(g, c, u, f, s & 1);
		}
		__syncthreads();
	}
}

__global__ void __launch_bounds__(kTailThreads) k_mg_tail(const MgTail T)
{
	const int last = T.nlev - 1;
	for (int l = 0; l < last; ++l) {
		tailSmooth(T.g[l], T.ncell[l], T.u[l], T.f[l], kPreSmooth);
		for (int c = threadIdx.x; c < T.ncell[l]; c += blockDim.x) {
			(void)residualCell(T.g[l], c, T.u[l], T.f[l], T.r[l]);
		}
		__syncthreads();
		for (int c = threadIdx.x; c < T.ncell[l + 1]; c += blockDim.x) {
			restrictCell(T.g[l], T.g[l + 1], T.coarsen[l][0], T.coarsen[l][1], T.coarsen[l][2], c, T.r[l], T.f[l + 1], T.u[l + 1]);
		}
		__syncthreads();
	}
	tailSmooth(T.g[last], T.ncell[last], T.u[last], T.f[last], kBottomSweeps);
	for (int l = last - 1; l >= 0; --l) {
		for (int c = threadIdx.x; c < T.ncell[l]; c += blockDim.x) {
			prolongCell(T.g[l], T.g[l + 1], T.coarsen[l][0], T.coarsen[l][1], T.coarsen[l][2], c, T.u[l + 1], T.u[l]);
		}
		__syncthreads();
		tailSmooth(T.g[l], T.ncell[l], T.u[l], T.f[l], kPostSmooth);
	}
}

// ---------------------------------------------------------------------------------------------------------------- surface kernels
__global__ void __launch_bounds__(256) k_grav_surface_gather(const Dims D, const int64_t S, const double *__restrict__ phi, double *__restrict__ s_out)
{
	const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (g >= S) {
		return;
	}
	int xyz[3], nb[3], side;
	const int d = gravity::ghostCoord(D, g, xyz, side);
	gravity::ghostNeighbour(D, d, side, xyz, nb);
	s_out[g] = phi[gravity::denseIndex(D, nb[0], nb[1], nb[2])];
}

__global__ void __launch_bounds__(256) k_grav_surface_scatter(const Dims D, const int64_t S, const double *__restrict__ bc, double *__restrict__ phi)
{
	const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (g >= S) {
		return;
	}
	int xyz[3], side;
	(void)gravity::ghostCoord(D, g, xyz, side);
	phi[gravity::denseIndex(D, xyz[0], xyz[1], xyz[2])] = bc[g];
}

// the lattice kernel K(n) of DESIGN.md §13 for an integer offset with r^2 >= 2 (the two tabulated offsets are selected on integers by the caller)
QK_DEV auto latticeKernelFar(int dx, int dy, int dz, int r2i) -> double
{
	const double r2 = static_cast<double>(r2i);
	// 1 / r from v_rsq_f64 and two Newton steps (r^2 is an exact small integer: no range concerns)
	double y = __builtin_amdgcn_rsq(r2);
	y = y * (1.5 - (0.5 * r2) * (y * y));
	y = y * (1.5 - (0.5 * r2) * (y * y));
	const double ir2 = y * y;
	const double x2 = static_cast<double>(dx * dx), y2 = static_cast<double>(dy * dy), z2 = static_cast<double>(dz * dz);
	const double n4 = x2 * x2 + y2 * y2 + z2 * z2;
	const double corr = (-3.0 + 5.0 * n4 * (ir2 * ir2)) * (0.125 * ir2);
	return (-0.07957747154594767 * y) * (1.0 + corr); // -1 / (4 pi r) * [1 + (-3 + 5 sum n_d^4 / r^4) / (8 r^2)]
}

constexpr double kLatticeK0 = -0.2527310098586630;	   // the cubic lattice Green's function at the origin
constexpr double kLatticeK1 = -0.2527310098586630 + 1.0 / 6.0; // r^2 = 1

// partial[p * S + t] = sum over the sources of part p of K(t - g') s(g'): one target per thread, sources through LDS in tiles, sources in list order
__global__ void __launch_bounds__(kSurfTile) k_grav_surface_potential(const Dims D, const int64_t S, const int tiles_per_part, const double *__restrict__ s_in,
									       double *__restrict__ partial)
{
	__shared__ int s_x[kSurfTile], s_y[kSurfTile], s_z[kSurfTile];
	__shared__ double s_s[kSurfTile];
	const int64_t t = static_cast<int64_t>(blockIdx.x) * kSurfTile + threadIdx.x;
	int tx[3] = {0, 0, 0}, side;
	if (t < S) {
		(void)gravity::ghostCoord(D, t, tx, side);
	}
	const int64_t src0 = static_cast<int64_t>(blockIdx.y) * tiles_per_part * kSurfTile;
	const int64_t src1 = src0 + static_cast<int64_t>(tiles_per_part) * kSurfTile < S ? src0 + static_cast<int64_t>(tiles_per_part) * kSurfTile : S;
	double acc = 0.0;
	for (int64_t base = src0; base < src1; base += kSurfTile) {
		const int64_t left = src1 - base;
		const int cnt = left < kSurfTile ? static_cast<int>(left) : kSurfTile;
		__syncthreads(); // the previous tile has been read by everyone
		if (static_cast<int>(threadIdx.x) < cnt) {
			int sx[3], sd;
			(void)gravity::ghostCoord(D, base + threadIdx.x, sx, sd);
			s_x[threadIdx.x] = sx[0];
			s_y[threadIdx.x] = sx[1];
			s_z[threadIdx.x] = sx[2];
			s_s[threadIdx.x] = s_in[base + threadIdx.x];
		}
		__syncthreads();
		for (int q = 0; q < cnt; ++q) {
			const int dx = tx[0] - s_x[q], dy = tx[1] - s_y[q], dz = tx[2] - s_z[q];
			const int r2 = dx * dx + dy * dy + dz * dz;
			const double far = latticeKernelFar(dx, dy, dz, r2);
			const double K = r2 == 0 ? kLatticeK0 : (r2 == 1 ? kLatticeK1 : far);
			acc = acc + K * s_s[q];
		}
	}
	if (t < S) {
		partial[static_cast<int64_t>(blockIdx.y) * S + t] = acc;
	}
}

// bc = -(partial[0] + partial[1] + ...), parts in order
__global__ void __launch_bounds__(256) k_grav_surface_reduce(const int64_t S, const int nparts, const double *__restrict__ partial, double *__restrict__ bc)
{
	const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (t >= S) {
		return;
	}
	double acc = 0.0;
	for (int p = 0; p < nparts; ++p) {
		acc = acc + partial[static_cast<int64_t>(p) * S + t];
	}
	bc[t] = -acc;
}

// ---------------------------------------------------------------------------------------------------------------- per valid cell of the level's boxes
__global__ void __launch_bounds__(256) k_grav_fill_rhs(const qk_box *__restrict__ boxes, const Dims D, const double G, const qk_array4 *__restrict__ state_t,
						       const int comp, double *__restrict__ f)
{
	const qk_box bx = boxes[blockIdx.y];
	const int nx = bx.hi[0] - bx.lo[0] + 1, ny = bx.hi[1] - bx.lo[1] + 1, nz = bx.hi[2] - bx.lo[2] + 1;
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (c >= static_cast<int64_t>(nx) * ny * nz) {
		return;
	}
	const int i = bx.lo[0] + static_cast<int>(c % nx), j = bx.lo[1] + static_cast<int>((c / nx) % ny), k = bx.lo[2] + static_cast<int>(c / (static_cast<int64_t>(nx) * ny));
	const RA4 U(state_t[blockIdx.y]);
	const int64_t idx = gravity::denseIndex(D, i, j, k);
	// *add*, as the reference (a particle deposit may precede it)
	f[idx] = f[idx] + 4.0 * M_PI * G * U(i, j, k, comp);
}

__global__ void __launch_bounds__(256) k_grav_kick(const qk_box *__restrict__ boxes, const Dims D, const double *__restrict__ phi, const double dx0,
						   const double dx1, const double dx2, const double dt, const qk_array4 *__restrict__ state_t)
{
	const qk_box bx = boxes[blockIdx.y];
	const int nx = bx.hi[0] - bx.lo[0] + 1, ny = bx.hi[1] - bx.lo[1] + 1, nz = bx.hi[2] - bx.lo[2] + 1;
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (c >= static_cast<int64_t>(nx) * ny * nz) {
		return;
	}
	const int i = bx.lo[0] + static_cast<int>(c % nx), j = bx.lo[1] + static_cast<int>((c / nx) % ny), k = bx.lo[2] + static_cast<int>(c / (static_cast<int64_t>(nx) * ny));
	const WA4 U(state_t[blockIdx.y]);
	const int64_t idx = gravity::denseIndex(D, i, j, k);
	const int64_t sx = D.n[0] + 2, sy = sx * (D.n[1] + 2);
	// reference src/QuokkaSimulation.hpp:734-754, its operations in its order
	const double rho = U(i, j, k, RHO);
	double px = U(i, j, k, MX);
	double py = U(i, j, k, MY);
	double pz = U(i, j, k, MZ);
	const double KE_old = 0.5 * (px * px + py * py + pz * pz) / rho;
	const double gx = -0.5 * (phi[idx + 1] - phi[idx - 1]) / dx0;
	const double gy = -0.5 * (phi[idx + sx] - phi[idx - sx]) / dx1;
	const double gz = -0.5 * (phi[idx + sy] - phi[idx - sy]) / dx2;
	px += dt * rho * gx;
	py += dt * rho * gy;
	pz += dt * rho * gz;
	const double KE_new = 0.5 * (px * px + py * py + pz * pz) / rho;
	const double dKE = KE_new - KE_old;
	U(i, j, k, MX) = px;
	U(i, j, k, MY) = py;
	U(i, j, k, MZ) = pz;
	U(i, j, k, ENE) += dKE;
}

auto grid1(int64_t n) -> dim3 { return dim3(static_cast<unsigned>((n + 255) / 256), 1, 1); }

// the level's boxes lie inside the lattice [0, n) (so that every dense index the per-cell kernels form is in bounds)
auto checkLevel(qk_level *lev, const int n[3], const char *who) -> int
{
	qk_ctx *ctx = lev->ctx;
	if (lev->ndim != 3) {
		return setError(ctx, QK_ERR_UNSUPPORTED, who, "self-gravity is built for ndim = 3 (as the reference: AMREX_SPACEDIM == 3)");
	}
	for (const qk_box &b : lev->boxes) {
		for (int d = 0; d < 3; ++d) {
			if (b.lo[d] < 0 || b.hi[d] >= n[d] || b.hi[d] < b.lo[d]) {
				return setError(ctx, QK_ERR_INVALID, who, "a box of the level lies outside the lattice n");
			}
		}
	}
	return QK_OK;
}

} // namespace

extern "C" {

int64_t qk_gravity_scratch_bytes(const int n[3])
{
	if (checkDims(nullptr, n, "") != QK_OK) {
		return -1;
	}
	std::vector<MgLevel> lv;
	buildLevels(n, 1.0, lv);
	const SurfSplit sp = surfSplit(n);
	return std::max(mgScratchBytes(lv), static_cast<int64_t>(8) * sp.nparts * sp.S);
}

int64_t qk_gravity_num_ghosts(const int n[3])
{
	if (checkDims(nullptr, n, "") != QK_OK) {
		return -1;
	}
	return gravity::numGhosts(Dims{{n[0], n[1], n[2]}});
}

int qk_gravity_fill_rhs(qk_level *lev, qk_stream s, double G, const qk_array4 *state, int density_comp, const int n[3], double *f)
{
	if (lev == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = lev->ctx;
	QK_REQUIRE(ctx, state && f && density_comp >= 0, "gravity_fill_rhs: NULL argument");
	QK_REQUIRE(ctx, ctx->device >= 0, "gravity_fill_rhs: planning-only context");
	if (int rc = checkDims(ctx, n, "gravity_fill_rhs"); rc != QK_OK) {
		return rc;
	}
	if (int rc = checkLevel(lev, n, "gravity_fill_rhs"); rc != QK_OK) {
		return rc;
	}
	if (lev->nboxes == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	const CellLaunch L = cellLaunch(lev, 0, -1);
	ProfScope prof(ctx, st, "gravity_fill_rhs");
	hipLaunchKernelGGL(k_grav_fill_rhs, L.grid, L.block, 0, st, lev->d_boxes, Dims{{n[0], n[1], n[2]}}, G, state, density_comp, f);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_gravity_kick(qk_level *lev, qk_stream s, const int n[3], const double *phi, const double dx[3], double dt, const qk_array4 *state)
{
	if (lev == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = lev->ctx;
	QK_REQUIRE(ctx, state && phi && dx, "gravity_kick: NULL argument");
	QK_REQUIRE(ctx, ctx->device >= 0, "gravity_kick: planning-only context");
	if (int rc = checkDims(ctx, n, "gravity_kick"); rc != QK_OK) {
		return rc;
	}
	if (int rc = checkLevel(lev, n, "gravity_kick"); rc != QK_OK) {
		return rc;
	}
	for (int d = 1; d < 3; ++d) {
		if (!(std::fabs(dx[d] - dx[0]) <= 1.0e-12 * std::fabs(dx[0])) || !(dx[0] > 0.0)) {
			return setError(ctx, QK_ERR_UNSUPPORTED, "gravity_kick", "self-gravity is built for cubic cells (dx equal in all directions to 1e-12 relative)");
		}
	}
	if (lev->nboxes == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	const CellLaunch L = cellLaunch(lev, 0, -1);
	ProfScope prof(ctx, st, "gravity_kick");
	hipLaunchKernelGGL(k_grav_kick, L.grid, L.block, 0, st, lev->d_boxes, Dims{{n[0], n[1], n[2]}}, phi, dx[0], dx[1], dx[2], dt, state);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_gravity_surface_gather(qk_ctx *ctx, qk_stream s, const int n[3], const double *phi, double *s_out)
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, phi && s_out, "gravity_surface_gather: NULL argument");
	QK_REQUIRE(ctx, ctx->device >= 0, "gravity_surface_gather: planning-only context");
	if (int rc = checkDims(ctx, n, "gravity_surface_gather"); rc != QK_OK) {
		return rc;
	}
	const Dims D{{n[0], n[1], n[2]}};
	const int64_t S = gravity::numGhosts(D);
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "gravity_surface_gather");
	hipLaunchKernelGGL(k_grav_surface_gather, grid1(S), dim3(256), 0, st, D, S, phi, s_out);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_gravity_surface_scatter(qk_ctx *ctx, qk_stream s, const int n[3], const double *bc, double *phi)
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, phi && bc, "gravity_surface_scatter: NULL argument");
	QK_REQUIRE(ctx, ctx->device >= 0, "gravity_surface_scatter: planning-only context");
	if (int rc = checkDims(ctx, n, "gravity_surface_scatter"); rc != QK_OK) {
		return rc;
	}
	const Dims D{{n[0], n[1], n[2]}};
	const int64_t S = gravity::numGhosts(D);
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "gravity_surface_scatter");
	hipLaunchKernelGGL(k_grav_surface_scatter, grid1(S), dim3(256), 0, st, D, S, bc, phi);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_gravity_surface_potential(qk_ctx *ctx, qk_stream s, const int n[3], const double *s_in, double *bc, void *scratch, int64_t scratch_bytes)
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, s_in && bc && scratch, "gravity_surface_potential: NULL argument");
	QK_REQUIRE(ctx, ctx->device >= 0, "gravity_surface_potential: planning-only context");
	if (int rc = checkDims(ctx, n, "gravity_surface_potential"); rc != QK_OK) {
		return rc;
	}
	const SurfSplit sp = surfSplit(n);
	QK_REQUIRE(ctx, scratch_bytes >= static_cast<int64_t>(8) * sp.nparts * sp.S, "gravity_surface_potential: scratch smaller than qk_gravity_scratch_bytes");
	const Dims D{{n[0], n[1], n[2]}};
	auto st = static_cast<hipStream_t>(s);
	auto *partial = static_cast<double *>(scratch);
	{
		ProfScope prof(ctx, st, "gravity_surface_potential");
		hipLaunchKernelGGL(k_grav_surface_potential, dim3(static_cast<unsigned>(sp.ntile), static_cast<unsigned>(sp.nparts), 1), dim3(kSurfTile), 0, st, D, sp.S,
				   sp.tiles_per_part, s_in, partial);
		QK_HIP_CHECK(ctx, hipGetLastError());
	}
	ProfScope prof(ctx, st, "gravity_surface_reduce");
	hipLaunchKernelGGL(k_grav_surface_reduce, grid1(sp.S), dim3(256), 0, st, sp.S, sp.nparts, partial, bc);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_gravity_dirichlet_solve(qk_ctx *ctx, qk_stream s, const int n[3], double h, const double *f, double *phi, double reltol, double abstol, int max_iter,
			       void *scratch, int64_t scratch_bytes, int *iters, double *resnorm)
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, f && phi && scratch && max_iter >= 0 && h > 0.0, "gravity_dirichlet_solve: bad argument");
	QK_REQUIRE(ctx, ctx->device >= 0, "gravity_dirichlet_solve: planning-only context");
	if (int rc = checkDims(ctx, n, "gravity_dirichlet_solve"); rc != QK_OK) {
		return rc;
	}
	std::vector<MgLevel> lv;
	buildLevels(n, h, lv);
	QK_REQUIRE(ctx, scratch_bytes >= mgScratchBytes(lv), "gravity_dirichlet_solve: scratch smaller than qk_gravity_scratch_bytes");
	auto st = static_cast<hipStream_t>(s);
	auto *words = static_cast<unsigned long long *>(scratch);
	auto *base = reinterpret_cast<double *>(static_cast<char *>(scratch) + kWordsBytes);
	lv[0].u = phi;
	lv[0].f = const_cast<double *>(f);
	lv[0].r = base;
	base += lv[0].size;
	for (size_t l = 1; l < lv.size(); ++l) {
		lv[l].u = base;
		lv[l].f = base + lv[l].size;
		lv[l].r = base + 2 * lv[l].size;
		base += 3 * lv[l].size;
	}
	const int nl = static_cast<int>(lv.size());
	unsigned long long hw[3] = {0, 0, 0};

	auto smooth = [&](const MgLevel &L, int npairs) {
		for (int p = 0; p < 2 * npairs; ++p) {
			hipLaunchKernelGGL(k_mg_smooth, grid1(L.ncell), dim3(256), 0, st, L.g, L.ncell, L.u, L.f, p & 1);
		}
	};
	// the tail: the first level of at most kTailCells cells and everything below it (none: the coarsest level is large — its sweeps are launches)
	int tail0 = nl;
	for (int l = 1; l < nl; ++l) {
		if (lv[l].ncell <= kTailCells && nl - l <= kMaxTailLevels) {
			tail0 = l;
			break;
		}
	}
	MgTail tail{};
	if (tail0 < nl) {
		tail.nlev = nl - tail0;
		for (int l = tail0; l < nl; ++l) {
			const int t = l - tail0;
			tail.g[t] = lv[l].g;
			tail.ncell[t] = static_cast<int>(lv[l].ncell);
			tail.u[t] = lv[l].u;
			tail.f[t] = lv[l].f;
			tail.r[t] = lv[l].r;
			for (int d = 0; d < 3; ++d) {
				tail.coarsen[t][d] = lv[l].coarsen[d];
			}
		}
	}
	const int ntop = tail0 < nl ? tail0 : nl - 1; // levels 0 .. ntop - 1 are taken launch by launch on the way down and up
	// max |f - L phi| on level 0, read by the host: once per cycle
	auto residualNorm = [&](double &out) -> int {
		QK_HIP_CHECK(ctx, hipMemsetAsync(&words[2], 0, 8, st));
		hipLaunchKernelGGL(k_mg_residual, grid1(lv[0].ncell), dim3(256), 0, st, lv[0].g, lv[0].ncell, lv[0].u, lv[0].f, lv[0].r, &words[2]);
		QK_HIP_CHECK(ctx, hipGetLastError());
		QK_HIP_CHECK(ctx, hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, st));
		QK_HIP_CHECK(ctx, hipStreamSynchronize(st));
		std::memcpy(&out, &hw[2], 8);
		return QK_OK;
	};

	ProfScope prof(ctx, st, "gravity_dirichlet_solve");
	// the norms of f: max |f| and min f (the reference's abstol is abstolPoisson_ * rhs.min(), src/simulation.hpp:1054-1057)
	{
		const unsigned long long init[2] = {0ULL, ~0ULL};
		QK_HIP_CHECK(ctx, hipMemcpyAsync(words, init, sizeof init, hipMemcpyHostToDevice, st));
		QK_HIP_CHECK(ctx, hipStreamSynchronize(st)); // (`init` is on the stack)
		const unsigned nb = static_cast<unsigned>(std::min<int64_t>((lv[0].ncell + 255) / 256, 1024));
		hipLaunchKernelGGL(k_grav_norms, dim3(nb), dim3(256), 0, st, lv[0].g, lv[0].ncell, lv[0].f, words);
		QK_HIP_CHECK(ctx, hipGetLastError());
	}
	double res = 0.0, tol = 0.0;
	int it = 0;
	int rc = QK_OK;
	for (;; ++it) {
		if (int e = residualNorm(res); e != QK_OK) {
			return e;
		}
		if (it == 0) {
			double fmax;
			std::memcpy(&fmax, &hw[0], 8);
			const double fmin = keyToDouble(hw[1]);
			if (!std::isfinite(fmax)) {
				return setError(ctx, QK_ERR_STATE, "gravity_dirichlet_solve", "the right-hand side holds a NaN or an infinity");
			}
			tol = std::max(reltol * fmax, abstol * fmin);
		}
		if (res <= tol) {
			break;
		}
		if (it >= max_iter) {
			rc = QK_ERR_NOT_CONVERGED;
			break;
		}
		// one V-cycle
		for (int l = 0; l < ntop; ++l) {
			const MgLevel &F = lv[l], &Cc = lv[l + 1];
			smooth(F, kPreSmooth);
			hipLaunchKernelGGL(k_mg_residual, grid1(F.ncell), dim3(256), 0, st, F.g, F.ncell, F.u, F.f, F.r, static_cast<unsigned long long *>(nullptr));
			hipLaunchKernelGGL(k_mg_restrict, grid1(Cc.ncell), dim3(256), 0, st, F.g, Cc.g, F.coarsen[0], F.coarsen[1], F.coarsen[2], Cc.ncell, F.r, Cc.f, Cc.u);
		}
		if (tail0 < nl) {
			hipLaunchKernelGGL(k_mg_tail, dim3(1), dim3(kTailThreads), 0, st, tail);
		} else {
			smooth(lv[nl - 1], kBottomSweeps);
		}
		for (int l = ntop - 1; l >= 0; --l) {
			const MgLevel &F = lv[l], &Cc = lv[l + 1];
			hipLaunchKernelGGL(k_mg_prolong, grid1(F.ncell), dim3(256), 0, st, F.g, Cc.g, F.coarsen[0], F.coarsen[1], F.coarsen[2], F.ncell, Cc.u, F.u);
			smooth(F, kPostSmooth);
		}
		QK_HIP_CHECK(ctx, hipGetLastError());
	}
	if (iters != nullptr) {
		*iters = it;
	}
	if (resnorm != nullptr) {
		*resnorm = res;
	}
	if (rc != QK_OK) {
		return setError(ctx, rc, "gravity_dirichlet_solve", "the residual did not reach the tolerance within max_iter cycles");
	}
	return QK_OK;
}

} // extern "C"
