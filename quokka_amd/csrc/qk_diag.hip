// qk_diag.hip — DiagPDF histograms: the fine-covered mask of a level, the minimum and maximum of a field, the linear bin and weight
// of every cell, and the segment sum that reduces the weights of every bin in a fixed order.
//
// Reference: src/io/DiagPDF.cpp (processDiag, getBinIndex1D, MFVecMin / MFVecMax), src/io/DiagFilter.cpp, amrex::makeFineMask.  The reference
// accumulates with amrex::HostDevice::Atomic::Add, which fixes no order; the order of the sum is this project's definition (§15): between
// qk_diag_keys and qk_diag_segsum the caller sorts the keys (stable) and looks up the range of every bin, as for the CIC deposit (§14).
// Every kernel is one ordinary launch; nothing waits on another workgroup; there are no floating-point atomics.
#include <cmath>
#include <limits>

#include "qk_device.hpp"
#include "qk_diag_index.hpp"
#include "qk_internal.hpp"

using namespace qk;

namespace
{

constexpr int kMinmaxPerThread = 16; // cells per thread of the min / max kernel: one partial per 4096 cells

struct CellOfBox {
	bool inside;
	int i, j, k;
	int64_t c; // index within the valid box, k outermost and i fastest
};

// cell `c` (this thread's) of box blockIdx.y
QK_DEV auto cellOfBox(const qk_box &bx, int64_t c) -> CellOfBox
{
	const int nx = bx.hi[0] - bx.lo[0] + 1, ny = bx.hi[1] - bx.lo[1] + 1, nz = bx.hi[2] - bx.lo[2] + 1;
	CellOfBox r;
	r.c = c;
	r.inside = c < static_cast<int64_t>(nx) * ny * nz;
	r.i = bx.lo[0] + static_cast<int>(c % nx);
	r.j = bx.lo[1] + static_cast<int>((c / nx) % ny);
	r.k = bx.lo[2] + static_cast<int>(c / (static_cast<int64_t>(nx) * ny));
	return r;
}

__global__ void __launch_bounds__(256) k_diag_mask_set(const qk_box *__restrict__ boxes, const qk_iarray4 *__restrict__ mask_t)
{
	const CellOfBox q = cellOfBox(boxes[blockIdx.y], static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x);
	if (!q.inside) {
		return;
	}
	const IA4 m(mask_t[blockIdx.y]);
	m(q.i, q.j, q.k) = 1;
}

// item blockIdx.y: {box, lo[3], hi[3]} — the cells of a coarsened box of the next level that lie in box `box` of this level.  The region is clipped
// against the box again here: a cell outside the box is never written.
__global__ void __launch_bounds__(256) k_diag_mask_clear(const qk_box *__restrict__ boxes, const int nboxes, const int *__restrict__ items,
							 const qk_iarray4 *__restrict__ mask_t)
{
	const int *it = items + 7 * static_cast<int64_t>(blockIdx.y);
	const int b = it[0];
	if (b < 0 || b >= nboxes) {
		return;
	}
	const qk_box bx = boxes[b];
	int lo[3], hi[3];
	for (int d = 0; d < 3; ++d) {
		lo[d] = it[1 + d] > bx.lo[d] ? it[1 + d] : bx.lo[d];
		hi[d] = it[4 + d] < bx.hi[d] ? it[4 + d] : bx.hi[d];
		if (hi[d] < lo[d]) {
			return;
		}
	}
	const int nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
	const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (c >= static_cast<int64_t>(nx) * ny * nz) {
		return;
	}
	const IA4 m(mask_t[b]);
	m(lo[0] + static_cast<int>(c % nx), lo[1] + static_cast<int>((c / nx) % ny), lo[2] + static_cast<int>(c / (static_cast<int64_t>(nx) * ny))) = 0;
}

// One partial {min, max, flag} per workgroup: 256 threads x kMinmaxPerThread cells of box blockIdx.y.  A value that is not finite raises the flag and
// takes no part in the minimum or the maximum.
__global__ void __launch_bounds__(256) k_diag_minmax_partial(const qk_box *__restrict__ boxes, const qk_array4 *__restrict__ field_t, const int comp,
							     double *__restrict__ partials)
{
	__shared__ double s_min[256], s_max[256], s_flag[256];
	const qk_box bx = boxes[blockIdx.y];
	const RA4 F(field_t[blockIdx.y]);
	double vmin = std::numeric_limits<double>::infinity(), vmax = -std::numeric_limits<double>::infinity(), flag = 0.0;
	const int64_t base = static_cast<int64_t>(blockIdx.x) * (256 * kMinmaxPerThread);
	for (int r = 0; r < kMinmaxPerThread; ++r) {
		const CellOfBox q = cellOfBox(bx, base + r * 256 + threadIdx.x);
		if (q.inside) {
			const double v = F(q.i, q.j, q.k, comp);
			if (std::isfinite(v)) {
				vmin = v < vmin ? v : vmin;
				vmax = v > vmax ? v : vmax;
			} else {
				flag = 1.0;
			}
		}
	}
	const int t = threadIdx.x;
	s_min[t] = vmin;
	s_max[t] = vmax;
	s_flag[t] = flag;
	__syncthreads();
	for (int s = 128; s >= 1; s >>= 1) {
		if (t < s) {
			s_min[t] = s_min[t + s] < s_min[t] ? s_min[t + s] : s_min[t];
			s_max[t] = s_max[t + s] > s_max[t] ? s_max[t + s] : s_max[t];
			s_flag[t] = s_flag[t + s] > s_flag[t] ? s_flag[t + s] : s_flag[t];
		}
		__syncthreads();
	}
	if (t == 0) {
		double *p = partials + 3 * (static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x);
		p[0] = s_min[0];
		p[1] = s_max[0];
		p[2] = s_flag[0];
	}
}

// one workgroup: the partials to {min, max, flag} in partials[3 * nparts ..]
__global__ void __launch_bounds__(256) k_diag_minmax_final(const int64_t nparts, double *__restrict__ partials)
{
	__shared__ double s_min[256], s_max[256], s_flag[256];
	double vmin = std::numeric_limits<double>::infinity(), vmax = -std::numeric_limits<double>::infinity(), flag = 0.0;
	for (int64_t p = threadIdx.x; p < nparts; p += 256) {
		const double a = partials[3 * p], b = partials[3 * p + 1], f = partials[3 * p + 2];
		vmin = a < vmin ? a : vmin;
		vmax = b > vmax ? b : vmax;
		flag = f > flag ? f : flag;
	}
	const int t = threadIdx.x;
	s_min[t] = vmin;
	s_max[t] = vmax;
	s_flag[t] = flag;
	__syncthreads();
	for (int s = 128; s >= 1; s >>= 1) {
		if (t < s) {
			s_min[t] = s_min[t + s] < s_min[t] ? s_min[t + s] : s_min[t];
			s_max[t] = s_max[t + s] > s_max[t] ? s_max[t + s] : s_max[t];
			s_flag[t] = s_flag[t + s] > s_flag[t] ? s_flag[t + s] : s_flag[t];
		}
		__syncthreads();
	}
	if (t == 0) {
		partials[3 * nparts] = s_min[0];
		partials[3 * nparts + 1] = s_max[0];
		partials[3 * nparts + 2] = s_flag[0];
	}
}

struct KeyVar {
	const qk_array4 *table;
	int comp;
	diag::Axis axis;
};
struct KeyFilter {
	const qk_array4 *table;
	int comp;
	double low, high;
};
struct KeyArgs {
	int nvars, nfilters;
	KeyVar vars[QK_DIAG_MAX_VARS];
	KeyFilter filters[QK_DIAG_MAX_FILTERS];
	double weight_fac;
	const qk_array4 *density; // NULL: the weight is weight_fac
	int density_comp;
	int64_t total_bins;
};

// One thread per valid cell of box blockIdx.y; e = box_offset[box] + (index within the box, k outermost and i fastest).  A cell that the mask or a
// filter removes, or that is out of range in a variable, gets the sentinel key total_bins.  The weight is written for every cell.
__global__ void __launch_bounds__(256) k_diag_keys(const qk_box *__restrict__ boxes, const KeyArgs a, const qk_iarray4 *__restrict__ mask_t,
						   const int64_t *__restrict__ box_offset, const int64_t ncells, int64_t *__restrict__ keys,
						   double *__restrict__ weights)
{
	const int b = blockIdx.y;
	const CellOfBox q = cellOfBox(boxes[b], static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x);
	if (!q.inside) {
		return;
	}
	const int64_t e = box_offset[b] + q.c;
	if (e < 0 || e >= ncells) {
		return;
	}
	bool part = true;
	if (mask_t != nullptr) {
		const CIA4 m(mask_t[b]);
		part = m(q.i, q.j, q.k) != 0;
	}
	for (int f = 0; f < a.nfilters; ++f) {
		const RA4 F(a.filters[f].table[b]);
		const double fval = F(q.i, q.j, q.k, a.filters[f].comp);
		if (fval < a.filters[f].low || fval > a.filters[f].high) { // (a NaN keeps the cell, as the reference's comparison does)
			part = false;
		}
	}
	int64_t cbin = 0;
	for (int n = 0; n < a.nvars; ++n) {
		const RA4 V(a.vars[n].table[b]);
		const double x = V(q.i, q.j, q.k, a.vars[n].comp);
		const double coord = diag::binCoordinate(a.vars[n].axis, x);
		if (diag::inRange(a.vars[n].axis, coord)) {
			cbin = diag::linearBin(cbin, a.vars[n].axis, diag::binOf(coord));
		} else {
			part = false;
		}
	}
	double weight = a.weight_fac;
	if (a.density != nullptr) {
		const RA4 R(a.density[b]);
		weight = weight * R(q.i, q.j, q.k, a.density_comp);
	}
	keys[e] = part ? cbin : a.total_bins;
	weights[e] = weight;
}

// One workgroup per block of the table: dst[blockIdx.x] = the tree sum of src[perm[start .. start + len)] (perm NULL: src[start .. start + len)),
// padded with +0.0 to 256 values; v[t] = v[t] + v[t + s] for t < s, s = 128 .. 1.  A block of length 0 (the launch is an upper bound) writes nothing;
// with copy_single a block of one value hands it on unchanged (a later pass of a bin that is already reduced).
__global__ void __launch_bounds__(256) k_diag_segsum(const int64_t *__restrict__ blk_start, const int64_t *__restrict__ blk_len, const double *__restrict__ src,
						     const int64_t *__restrict__ perm, const int64_t nsrc, const int64_t nperm, const int copy_single,
						     double *__restrict__ dst)
{
	__shared__ double v[diag::kBlock];
	const int64_t start = blk_start[blockIdx.x], len = blk_len[blockIdx.x];
	if (!diag::blockIsValid(start, len, perm != nullptr ? nperm : nsrc)) { // (uniform over the workgroup)
		return;
	}
	const int t = threadIdx.x;
	double x = 0.0;
	if (t < len) {
		int64_t p = start + t;
		if (perm != nullptr) {
			p = perm[p];
		}
		x = (p >= 0 && p < nsrc) ? src[p] : std::numeric_limits<double>::quiet_NaN();
	}
	if (copy_single != 0 && len == 1) {
		if (t == 0) {
			dst[blockIdx.x] = x;
		}
		return;
	}
	v[t] = x;
	__syncthreads();
	for (int s = diag::kBlock / 2; s >= 1; s >>= 1) {
		if (t < s) {
			v[t] = v[t] + v[t + s];
		}
		__syncthreads();
	}
	if (t == 0) {
		dst[blockIdx.x] = v[0];
	}
}

auto minmaxGridX(const qk_level *lev) -> int64_t
{
	const int64_t n = static_cast<int64_t>(lev->maxlen[0]) * lev->maxlen[1] * lev->maxlen[2];
	const int64_t per = 256 * kMinmaxPerThread;
	return (n + per - 1) / per;
}

} // namespace

extern "C" {

int qk_diag_mask(qk_level *lev, qk_stream s, qk_iarray4 *mask, int nitems, const int *items, int64_t max_item_cells)
{
	if (lev == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = lev->ctx;
	QK_REQUIRE(ctx, ctx->device >= 0, "diag_mask: planning-only context");
	QK_REQUIRE(ctx, mask != nullptr, "diag_mask: NULL argument");
	QK_REQUIRE(ctx, nitems >= 0 && max_item_cells >= 0, "diag_mask: negative size");
	QK_REQUIRE(ctx, nitems == 0 || (items != nullptr && max_item_cells > 0), "diag_mask: items announced and none given");
	QK_REQUIRE(ctx, nitems <= 65535, "diag_mask: more than 65535 items");
	if (lev->nboxes == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	const CellLaunch L = cellLaunch(lev, 0, -1);
	// an item lies inside one box of the level: the kernel clips it, so a larger max_item_cells only launches threads that return
	const int64_t box_cells = static_cast<int64_t>(lev->maxlen[0]) * lev->maxlen[1] * lev->maxlen[2];
	const int64_t per_item = max_item_cells < box_cells ? max_item_cells : box_cells;
	ProfScope prof(ctx, st, "diag_mask");
	hipLaunchKernelGGL(k_diag_mask_set, L.grid, L.block, 0, st, lev->d_boxes, mask);
	QK_HIP_CHECK(ctx, hipGetLastError());
	if (nitems > 0) {
		hipLaunchKernelGGL(k_diag_mask_clear, dim3(static_cast<unsigned>((per_item + 255) / 256), static_cast<unsigned>(nitems), 1), dim3(256), 0, st,
				   lev->d_boxes, lev->nboxes, items, mask);
		QK_HIP_CHECK(ctx, hipGetLastError());
	}
	return QK_OK;
}

int64_t qk_diag_minmax_scratch_bytes(qk_level *lev)
{
	if (lev == nullptr) {
		return -1;
	}
	return 3 * static_cast<int64_t>(sizeof(double)) * (minmaxGridX(lev) * lev->nboxes + 1);
}

int qk_diag_minmax(qk_level *lev, qk_stream s, const qk_array4 *field, int comp, void *scratch, int64_t scratch_bytes, double minmax[2])
{
	if (lev == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = lev->ctx;
	QK_REQUIRE(ctx, ctx->device >= 0, "diag_minmax: planning-only context");
	QK_REQUIRE(ctx, field != nullptr && scratch != nullptr && minmax != nullptr, "diag_minmax: NULL argument");
	QK_REQUIRE(ctx, comp >= 0, "diag_minmax: comp < 0");
	QK_REQUIRE(ctx, scratch_bytes >= qk_diag_minmax_scratch_bytes(lev), "diag_minmax: scratch smaller than qk_diag_minmax_scratch_bytes");
	minmax[0] = std::numeric_limits<double>::max();
	minmax[1] = std::numeric_limits<double>::lowest();
	if (lev->nboxes == 0) {
		return QK_OK;
	}
	auto st = static_cast<hipStream_t>(s);
	const int64_t gx = minmaxGridX(lev), nparts = gx * lev->nboxes;
	auto *partials = static_cast<double *>(scratch);
	double h[3] = {0.0, 0.0, 0.0};
	{
		ProfScope prof(ctx, st, "diag_minmax");
		hipLaunchKernelGGL(k_diag_minmax_partial, dim3(static_cast<unsigned>(gx), static_cast<unsigned>(lev->nboxes), 1), dim3(256), 0, st, lev->d_boxes, field,
				   comp, partials);
		QK_HIP_CHECK(ctx, hipGetLastError());
		hipLaunchKernelGGL(k_diag_minmax_final, dim3(1), dim3(256), 0, st, nparts, partials);
		QK_HIP_CHECK(ctx, hipGetLastError());
	}
	QK_HIP_CHECK(ctx, hipMemcpyAsync(h, partials + 3 * nparts, sizeof(h), hipMemcpyDeviceToHost, st));
	QK_HIP_CHECK(ctx, hipStreamSynchronize(st));
	if (h[2] != 0.0) {
		return setError(ctx, QK_ERR_STATE, "diag_minmax", "the field holds a value that is not finite");
	}
	minmax[0] = h[0];
	minmax[1] = h[1];
	return QK_OK;
}

int qk_diag_keys(qk_level *lev, qk_stream s, const qk_diag_pdf *pdf, const qk_iarray4 *mask, const int64_t *box_offset, int64_t ncells, int64_t *keys,
		 double *weights)
{
	if (lev == nullptr) {
		return QK_ERR_INVALID;
	}
	qk_ctx *ctx = lev->ctx;
	QK_REQUIRE(ctx, ctx->device >= 0, "diag_keys: planning-only context");
	QK_REQUIRE(ctx, pdf != nullptr, "diag_keys: NULL argument");
	QK_REQUIRE(ctx, pdf->nvars >= 1 && pdf->nvars <= QK_DIAG_MAX_VARS, "diag_keys: 1 .. QK_DIAG_MAX_VARS variables");
	QK_REQUIRE(ctx, pdf->nfilters >= 0 && pdf->nfilters <= QK_DIAG_MAX_FILTERS, "diag_keys: 0 .. QK_DIAG_MAX_FILTERS filters");
	QK_REQUIRE(ctx, ncells >= 0, "diag_keys: ncells < 0");
	KeyArgs a{};
	a.nvars = pdf->nvars;
	a.nfilters = pdf->nfilters;
	diag::Axis axes[QK_DIAG_MAX_VARS];
	for (int n = 0; n < pdf->nvars; ++n) {
		const qk_diag_var &v = pdf->vars[n];
		QK_REQUIRE(ctx, v.table != nullptr && v.comp >= 0, "diag_keys: a variable without a table or with comp < 0");
		QK_REQUIRE(ctx, v.nbins > 0, "diag_keys: nbins <= 0");
		axes[n] = diag::Axis{v.low_t, v.width_t, v.nbins, v.log_spaced != 0 ? 1 : 0};
		a.vars[n] = KeyVar{v.table, v.comp, axes[n]};
	}
	for (int f = 0; f < pdf->nfilters; ++f) {
		const qk_diag_filter &fl = pdf->filters[f];
		QK_REQUIRE(ctx, fl.table != nullptr && fl.comp >= 0, "diag_keys: a filter without a table or with comp < 0");
		a.filters[f] = KeyFilter{fl.table, fl.comp, fl.low, fl.high};
	}
	a.total_bins = diag::totalBins(axes, pdf->nvars);
	if (a.total_bins < 0) {
		return setError(ctx, QK_ERR_UNSUPPORTED, "diag_keys", "more than 2^24 bins in all");
	}
	QK_REQUIRE(ctx, pdf->density == nullptr || pdf->density_comp >= 0, "diag_keys: density_comp < 0");
	a.weight_fac = pdf->weight_fac;
	a.density = pdf->density;
	a.density_comp = pdf->density_comp;
	if (lev->nboxes == 0 || ncells == 0) {
		return QK_OK;
	}
	QK_REQUIRE(ctx, box_offset != nullptr && keys != nullptr && weights != nullptr, "diag_keys: NULL argument");
	auto st = static_cast<hipStream_t>(s);
	const CellLaunch L = cellLaunch(lev, 0, -1);
	ProfScope prof(ctx, st, "diag_keys");
	hipLaunchKernelGGL(k_diag_keys, L.grid, L.block, 0, st, lev->d_boxes, a, mask, box_offset, ncells, keys, weights);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

int qk_diag_segsum(qk_ctx *ctx, qk_stream s, int64_t nblocks, const int64_t *blk_start, const int64_t *blk_len, const double *src, int64_t nsrc,
		   const int64_t *perm, int64_t nperm, int copy_single, double *dst)
{
	if (ctx == nullptr) {
		return QK_ERR_INVALID;
	}
	QK_REQUIRE(ctx, ctx->device >= 0, "diag_segsum: planning-only context");
	QK_REQUIRE(ctx, nblocks >= 0 && nsrc >= 0 && nperm >= 0, "diag_segsum: negative size");
	QK_REQUIRE(ctx, nblocks <= 0x7fffffff, "diag_segsum: more than 2^31 - 1 blocks");
	if (nblocks == 0) {
		return QK_OK;
	}
	QK_REQUIRE(ctx, blk_start && blk_len && src && dst, "diag_segsum: NULL argument");
	auto st = static_cast<hipStream_t>(s);
	ProfScope prof(ctx, st, "diag_segsum");
	hipLaunchKernelGGL(k_diag_segsum, dim3(static_cast<unsigned>(nblocks)), dim3(256), 0, st, blk_start, blk_len, src, perm, nsrc, nperm, copy_single, dst);
	QK_HIP_CHECK(ctx, hipGetLastError());
	return QK_OK;
}

} // extern "C"
