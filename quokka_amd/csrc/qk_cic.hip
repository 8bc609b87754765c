// qk_cic.hip — massive cloud-in-cell particles on one level: the deposit into the Poisson right-hand side, the leapfrog kick from the
// dense potential and the drift.
//
// Reference: src/simulation.hpp:1043-1047 with src/particles/CICParticles.hpp (deposit, weight 4 pi G m), :1107-1193 (kick), :1195-1216 (drift).
// AMReX's ParticleToMesh / ParticleInterpolator::Linear are not restated: the discrete operations are this project's definition (§14), written so that
// the result is deterministic — the deposit is a GATHER over cells in a fixed order (no floating-point atomics), fed by a stable sort of per-particle
// base-cell keys that the caller does between qk_cic_cell_keys and qk_cic_deposit.
// Every kernel is one ordinary launch; nothing waits on another workgroup.
#include <cmath>

#include "qk_cic_index.hpp"
#include "qk_device.hpp"
#include "qk_gravity_index.hpp"
#include "qk_internal.hpp"

using namespace qk;

namespace
{

using gravity::Dims;

struct CicGeom {
	int n[3];
	double plo[3];
	double dxi[3];
};

__global__ void __launch_bounds__(256) k_cic_keys(const CicGeom g, const int64_t np, const double *__restrict__ x0, const double *__restrict__ x1,
						  const double *__restrict__ x2, int64_t *__restrict__ keys)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (p >= np) {
		return;
	}
	const cic::Axis a0 = cic::axis(x0[p], g.plo[0], g.dxi[0]);
	const cic::Axis a1 = cic::axis(x1[p], g.plo[1], g.dxi[1]);
	const cic::Axis a2 = cic::axis(x2[p], g.plo[2], g.dxi[2]);
	keys[p] = cic::particleKey(g.n, a0, a1, a2);
}

// One thread per interior cell c, x fastest.  Its eight source base cells b = c - (ii, jj, kk), kk outermost and ii fastest; within one base cell the
// particles in ascending storage index (perm is the stable sort of the keys; offsets[key] .. offsets[key + 1] its range).  The weights are recomputed
// from the position.  A cell that no particle reaches is not written.
__global__ void __launch_bounds__(256) k_cic_deposit(const CicGeom g, const double fourPiG, const double inv_vol, const double *__restrict__ x0,
						     const double *__restrict__ x1, const double *__restrict__ x2, const double *__restrict__ mass,
						     const int64_t *__restrict__ perm, const int64_t *__restrict__ offsets, double *__restrict__ rhs)
{
	const int64_t ncell = static_cast<int64_t>(g.n[0]) * g.n[1] * g.n[2];
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (c >= ncell) {
		return;
	}
	const int i = static_cast<int>(c % g.n[0]), j = static_cast<int>((c / g.n[0]) % g.n[1]), k = static_cast<int>(c / (static_cast<int64_t>(g.n[0]) * g.n[1]));
	double sum = 0.0;
	int64_t reached = 0;
#pragma unroll
	for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
		for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
			for (int ii = 0; ii < 2; ++ii) {
				const int64_t key = cic::keyOf(g.n, i - ii, j - jj, k - kk); // (c_d - 1 >= -1: always a possible base cell)
				const int64_t s0 = offsets[key], s1 = offsets[key + 1];
				reached += s1 - s0;
				for (int64_t s = s0; s < s1; ++s) {
					const int64_t p = perm[s];
					const cic::Axis a0 = cic::axis(x0[p], g.plo[0], g.dxi[0]);
					const cic::Axis a1 = cic::axis(x1[p], g.plo[1], g.dxi[1]);
					const cic::Axis a2 = cic::axis(x2[p], g.plo[2], g.dxi[2]);
					const double W = ((ii == 0 ? a0.w0 : a0.w1) * (jj == 0 ? a1.w0 : a1.w1)) * (kk == 0 ? a2.w0 : a2.w1);
					sum = sum + W * (fourPiG * mass[p]);
				}
			}
		}
	}
	if (reached > 0) {
		rhs[gravity::denseIndex(Dims{{g.n[0], g.n[1], g.n[2]}}, i, j, k)] = sum * inv_vol;
	}
}

// One thread per particle, taking part or not.  The eight stencil cells, each index clamped to [0, N_d - 1] (the first-order extrapolated ghost layer
// of the reference's acceleration array, extended beyond); the acceleration is formed on the fly from the dense potential, whose face-adjacent ghost
// layer holds the boundary data (edges and corners are never read: a clamped cell is interior, and c +- e_d moves in one direction only).
template <int d>
__device__ __forceinline__ auto kickComponent(const CicGeom &g, const double *__restrict__ phi, const cic::Axis &a0, const cic::Axis &a1, const cic::Axis &a2,
					      const double half_dt, double v) -> double
{
	const Dims D{{g.n[0], g.n[1], g.n[2]}};
	const int64_t sx = g.n[0] + 2, sy = sx * (g.n[1] + 2);
	const int64_t st = d == 0 ? 1 : (d == 1 ? sx : sy);
	const double dxi = d == 0 ? g.dxi[0] : (d == 1 ? g.dxi[1] : g.dxi[2]);
#pragma unroll
	for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
		for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
			for (int ii = 0; ii < 2; ++ii) {
				const int ci = cic::clampCell(a0.bf, ii, g.n[0]), cj = cic::clampCell(a1.bf, jj, g.n[1]), ck = cic::clampCell(a2.bf, kk, g.n[2]);
				const int64_t idx = gravity::denseIndex(D, ci, cj, ck);
				const double W = ((ii == 0 ? a0.w0 : a0.w1) * (jj == 0 ? a1.w0 : a1.w1)) * (kk == 0 ? a2.w0 : a2.w1);
				const double acc = -0.5 * dxi * (phi[idx + st] - phi[idx - st]);
				v += half_dt * (W * acc);
			}
		}
	}
	return v;
}

__global__ void __launch_bounds__(256) k_cic_kick(const CicGeom g, const double *__restrict__ phi, const double half_dt, const int64_t np,
						  const double *__restrict__ x0, const double *__restrict__ x1, const double *__restrict__ x2,
						  double *__restrict__ v0, double *__restrict__ v1, double *__restrict__ v2)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (p >= np) {
		return;
	}
	const cic::Axis a0 = cic::axis(x0[p], g.plo[0], g.dxi[0]);
	const cic::Axis a1 = cic::axis(x1[p], g.plo[1], g.dxi[1]);
	const cic::Axis a2 = cic::axis(x2[p], g.plo[2], g.dxi[2]);
	v0[p] = kickComponent<0>(g, phi, a0, a1, a2, half_dt, v0[p]);
	v1[p] = kickComponent<1>(g, phi, a0, a1, a2, half_dt, v1[p]);
	v2[p] = kickComponent<2>(g, phi, a0, a1, a2, half_dt, v2[p]);
}

__global__ void __launch_bounds__(256) k_cic_drift(const double dt, const int64_t np, double *__restrict__ x0, double *__restrict__ x1,
						   double *__restrict__ x2, const double *__restrict__ v0, const double *__restrict__ v1,
						   const double *__restrict__ v2)
{
	const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (p >= np) {
		return;
	}
	x0[p] += dt * v0[p];
	x1[p] += dt * v1[p];
	x2[p] += dt * v2[p];
}

auto grid1(int64_t n) -> dim3 { return dim3(static_cast<unsigned>((n + 255) / 256), 1, 1); }

// n as the Poisson solver takes it, cubic cells; fills the kernels' geometry
auto cicGeom(qk_ctx *ctx, const int n[3], const double plo[3], const double dx[3], const char *who, CicGeom &g) -> int
{
	if (n == nullptr || plo == nullptr || dx == nullptr) {
		return setError(ctx, QK_ERR_INVALID, who, "NULL argument");
	}
	if (qk_gravity_num_ghosts(n) < 0) {
		return setError(ctx, QK_ERR_UNSUPPORTED, who, "CIC particles need the lattice of the Poisson solve: an even cell count of 4 .. 4096 in every direction");
	}
	for (int d = 0; d < 3; ++d) {
		if (!(dx[0] > 0.0) || !(std::fabs(dx[d] - dx[0]) <= 1.0e-12 * std::fabs(dx[0]))) {
			return setError(ctx, QK_ERR_UNSUPPORTED, who, "CIC particles are built for cubic cells (dx equal in all directions to 1e-12 relative)");
		}
		if (!std::isfinite(plo[d])) {
			return setError(ctx, QK_ERR_INVALID, who, "prob_lo is not finite");
		}
		g.n[d] = n[d];
		g.plo[d] = plo[d];
		g.dxi[d] = 1.0 / dx[d];
	}
	return QK_OK;
}

} // namespace

extern "C" {

int qk_cic_cell_keys(qk_ctx *ctx, qk_stream s, const int n[3], const double prob_lo[3], const double dx[3], int64_t np, const double *const pos[3],
		     int64_t *keys)
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "cic_cell_keys: planning-only context");
	QK_REQUIRE(ctx, np >= 0, "cic_cell_keys: np < 0");
	CicGeom g;
	if (int rc = cicGeom(ctx, n, prob_lo, dx, "cic_cell_keys", g); rc != QK_OK) {
		return rc;
	}
	if (np == 0) {
		return QK_OK;
	}
	QK_REQUIRE(ctx, pos && pos[0] && pos[1] && pos[2] && keys, "cic_cell_keys: NULL argument");
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "cic_keys");
	hipLaunchKernelGGL(k_cic_keys, grid1(np), dim3(256), 0, st, g, np, pos[0], pos[1], pos[2], keys);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_cic_deposit(qk_ctx *ctx, qk_stream s, const int n[3], const double prob_lo[3], const double dx[3], double G, int64_t np,
		   const double *const pos[3], const double *mass, const int64_t *perm, const int64_t *offsets, double *rhs)
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "cic_deposit: planning-only context");
	QK_REQUIRE(ctx, np >= 0, "cic_deposit: np < 0");
	CicGeom g;
	if (int rc = cicGeom(ctx, n, prob_lo, dx, "cic_deposit", g); rc != QK_OK) {
		return rc;
	}
	if (np == 0) {
		return QK_OK;
	}
	QK_REQUIRE(ctx, pos && pos[0] && pos[1] && pos[2] && mass && perm && offsets && rhs, "cic_deposit: NULL argument");
	auto st = static_cast<hipStream_t>(s);
	const int64_t ncell = static_cast<int64_t>(n[0]) * n[1] * n[2];
	ProfScope prof(ctx, st, "cic_deposit");
	hipLaunchKernelGGL(k_cic_deposit, grid1(ncell), dim3(256), 0, st, g, ((4.0 * M_PI) * G), 1.0 / (dx[0] * dx[1] * dx[2]), pos[0], pos[1], pos[2], mass, perm,
			   offsets, rhs);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_cic_kick(qk_ctx *ctx, qk_stream s, const int n[3], const double prob_lo[3], const double dx[3], double dt, const double *phi, int64_t np,
		const double *const pos[3], double *const vel[3])
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "cic_kick: planning-only context");
	QK_REQUIRE(ctx, np >= 0, "cic_kick: np < 0");
	CicGeom g;
	if (int rc = cicGeom(ctx, n, prob_lo, dx, "cic_kick", g); rc != QK_OK) {
		return rc;
	}
	if (np == 0) {
		return QK_OK;
	}
	QK_REQUIRE(ctx, phi && pos && pos[0] && pos[1] && pos[2] && vel && vel[0] && vel[1] && vel[2], "cic_kick: NULL argument");
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "cic_kick");
	hipLaunchKernelGGL(k_cic_kick, grid1(np), dim3(256), 0, st, g, phi, 0.5 * dt, np, pos[0], pos[1], pos[2], vel[0], vel[1], vel[2]);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_cic_drift(qk_ctx *ctx, qk_stream s, double dt, int64_t np, double *const pos[3], const double *const vel[3])
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "cic_drift: planning-only context");
	QK_REQUIRE(ctx, np >= 0, "cic_drift: np < 0");
	if (np == 0) {
		return QK_OK;
	}
	QK_REQUIRE(ctx, pos && pos[0] && pos[1] && pos[2] && vel && vel[0] && vel[1] && vel[2], "cic_drift: NULL argument");
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "cic_drift");
	hipLaunchKernelGGL(k_cic_drift, grid1(np), dim3(256), 0, st, dt, np, pos[0], pos[1], pos[2], vel[0], vel[1], vel[2]);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

} // extern "C"
