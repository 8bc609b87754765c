"""DiagPDF histograms on the GPU (csrc/qk_diag.hip, quokka_amd/diagnostics.py) against the numpy restatement of tests/diag_pdf_reference.py:
the segment sum alone, keys and weights and the histogram on one level and on a two-level hierarchy, every comparison bit for bit; then the driver —
nothing configured, files at the reference's steps and under its names, every refusal.

Input condition for log-spaced variables: the device's log10 is not the host's, so the inputs are built such that the bin coordinate q, as the
restatement computes it, stays at least 1e-6 away from every integer (asserted here on the CPU): no cell can change its bin and none needs leaving out.
Linear variables are tested on the edges themselves."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import diag_pdf_reference as dr
from quokka_amd import capi, diagnostics
from quokka_amd.amr_simulation import AmrSimulation
from quokka_amd.plotfile import component_names
from quokka_amd.simulation import Geometry, HydroSimulation

pytestmark = pytest.mark.gpu

NAMES = component_names(6)
# dyadic dx: every weight and every partial sum of a volume-weighted histogram is exact.  192 and 1536 cells: less and more than one workgroup of 256
LATTICES = {"8x6x4": ((8, 6, 4), 0.25, (4, 6, 4)), "16x8x12": ((16, 8, 12), 0.125, (8, 4, 6))}


# ---------------------------------------------------------------------- helpers
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_sim(ctx, n, h, mgs, ndim=3):
    n = list(n) + [1] * (3 - len(n))
    geom = Geometry(ndim, n[:ndim], [0.0, 0.0, 0.0], [n[d] * h if d < ndim else 1.0 for d in range(3)], [0, 0, 0])
    bcs = [([capi.BC_FOEXTRAP] * 3, [capi.BC_FOEXTRAP] * 3) for _ in range(6)]
    sim = HydroSimulation(ctx, geom, capi.traits(5.0 / 3.0, False, ndim), bcs, list(mgs)[:ndim], use_fused=(ndim == 3))
    sim.cflNumber_, sim.stopTime_ = 0.3, 1.0e30
    return sim


def random_state(rng, shape, specials=True):
    """(6, nz, ny, nx): density and internal energy over decades (log axes), gasEnergy in [0.25, 0.75] with cells ON the edges of a dyadic axis and
    cells that are not finite or huge (a linear axis), momenta in (-1, 1) with a NaN in x (a filter field)"""
    U = np.zeros((6,) + shape)
    U[0] = 10.0 ** rng.uniform(-3.0, 3.0, shape)
    U[1:4] = rng.uniform(-1.0, 1.0, (3,) + shape)
    U[4] = rng.uniform(0.25, 0.75, shape)
    U[5] = 10.0 ** rng.uniform(-2.0, 2.0, shape)
    if specials:
        flat = U[4].reshape(-1)
        vals = [0.25, 0.375, 0.5, 0.625, 0.75, np.nextafter(0.75, 0.0), np.nextafter(0.25, 0.0), np.nextafter(0.5, 0.0), np.nan, np.inf, -np.inf,
                1.0e300, -1.0e300]
        where = rng.choice(flat.size, len(vals), replace=False)
        flat[where] = vals
        U[1].reshape(-1)[rng.choice(flat.size, 3, replace=False)] = [np.nan, 0.0, 0.5]
    return U


def fill(sim, seed, specials=True):
    rng = np.random.default_rng(seed)
    for b, (lo, hi) in enumerate(sim.lev.boxes):
        sim.state_new_cc_.valid(b).copy_(torch.from_numpy(random_state(rng, dr.box_shape(lo, hi), specials)))
    return sim


def half_energy(L, name, out):
    """a derived variable: ComputeDerivedVar(level_sim, name, out), torch operations on out.valid(b)"""
    assert name == "half_energy"
    for b in range(L.lev.nboxes):
        out.valid(b)[0].copy_(L.state_new_cc_.valid(b)[4] * 0.5)


def level_dict(L):
    """the level as the restatement takes it: valid cells of every state component and of the derived variable"""
    st = [L.state_new_cc_.valid(b).cpu().numpy() for b in range(L.lev.nboxes)]
    fields = {nm: [s[c].copy() for s in st] for c, nm in enumerate(NAMES)}
    fields["half_energy"] = [s[4] * 0.5 for s in st]
    return {"boxes": L.lev.boxes, "dx": tuple(L.geom.dx), "fields": fields}


def hist_of(d, ndim):
    return {"vars": [(v.name, v.nbins, v.log_spaced, None if v.use_field_minmax else v.low, None if v.use_field_minmax else v.high) for v in d.vars],
            "filters": [(f.field_name, f.low, f.high) for f in d.filters], "weight_by": d.weight_type, "ndim": ndim}


def assert_log_margin(hist, levels):
    """the input condition: q of every log-spaced variable at least 1e-6 away from every integer"""
    for name, nbins, log_spaced, low, high in dr.resolve_ranges(hist, levels)["vars"]:
        if log_spaced:
            for L in levels:
                for a in L["fields"][name]:
                    q = dr.bin_coordinate(a, nbins, 1, low, high)
                    q = q[np.isfinite(q)]
                    assert np.abs(q - np.round(q)).min() >= 1.0e-6, name


def pdf_params(**kw):
    """deck keys of one DiagPDF `h`: vars = [(name, nbins, log, range or None)], filters = [(name, field, key, value)]"""
    p = {"quokka.diagnostics": "h", "quokka.h.type": "DiagPDF", "quokka.h.int": kw.get("int", 1), "quokka.h.var_names": [v[0] for v in kw["vars"]]}
    if "weight_by" in kw:
        p["quokka.h.weight_by"] = kw["weight_by"]
    if "file" in kw:
        p["quokka.h.file"] = kw["file"]
    for name, nbins, log, rng in kw["vars"]:
        p[f"quokka.h.{name}.nBins"], p[f"quokka.h.{name}.log_spaced_bins"] = nbins, log
        if rng is not None:
            p[f"quokka.h.{name}.range"] = list(rng)
    if kw.get("filters"):
        p["quokka.h.filters"] = [f[0] for f in kw["filters"]]
        for fname, field, key, value in kw["filters"]:
            p[f"quokka.h.{fname}.field_name"], p[f"quokka.h.{fname}.{key}"] = field, value
    return p


E_AXIS = ("gasEnergy", 4, 0, (0.25, 0.75))                # linear, dyadic edges: cells sit ON them
RHO_AXIS = ("gasDensity", 7, 1, (1.0e-3, 1.0e3))          # log-spaced
EINT_AXIS = ("gasInternalEnergy", 5, 1, (3.0e-2, 2.0e1))  # log-spaced, cells outside on both sides
CONFIGS = {
    "1var_linear_volume": dict(vars=[E_AXIS]),
    "2var_lin_log_mass": dict(vars=[E_AXIS, RHO_AXIS], weight_by="mass"),
    "3var_counts_greater": dict(vars=[RHO_AXIS, E_AXIS, EINT_AXIS], weight_by="cell_counts", filters=[("f1", "y-GasMomentum", "value_greater", -0.5)]),
    "filters_less_inrange_nan": dict(vars=[EINT_AXIS], weight_by="volume",
                                     filters=[("f1", "x-GasMomentum", "value_less", 0.5), ("f2", "z-GasMomentum", "value_inrange", [0.75, -0.75])]),
    "derived_and_field_range_mass": dict(vars=[("half_energy", 4, 0, (0.125, 0.375)), ("y-GasMomentum", 6, 0, None)], weight_by="mass"),
    "log_mass_field_range_linear": dict(vars=[("z-GasMomentum", 3, 0, None), RHO_AXIS], weight_by="mass"),
}

_SIMS = {}


def lattice_sim(ctx, name):
    if name not in _SIMS:
        n, h, mgs = LATTICES[name]
        sim = fill(make_sim(ctx, n, h, mgs), seed=sum(n))
        sim.derivedNames_, sim.ComputeDerivedVar = ["half_energy"], half_energy
        _SIMS[name] = (sim, [level_dict(sim)])
    return _SIMS[name]


def check_against_restatement(sim, levels_gpu, levels, d, ndim=3):
    """keys and weights of every level, then the histogram, bit for bit; returns the histogram"""
    hist = hist_of(d, ndim)
    assert_log_margin(hist, levels)
    pdf = d.process(sim)  # (takes the absent ranges from the field, as every output does)
    resolved = dr.resolve_ranges(hist, levels)
    assert [(v.low, v.high) for v in d.vars] == [(lo, hi) for _, _, _, lo, hi in resolved["vars"]]
    fields = diagnostics.compute_fields(sim, levels_gpu, d.var_list())
    for l, L in enumerate(levels_gpu):
        finer_gpu = levels_gpu[l + 1].all_boxes if l + 1 < len(levels_gpu) else None
        finer = levels[l + 1]["boxes"] if l + 1 < len(levels) else None
        keys, weights = d.level_keys_weights(L, [fields[n][l] for n in d._field_order()], finer_gpu)
        rk, rw = dr.level_keys_weights(resolved, levels[l], finer)
        assert np.array_equal(keys.cpu().numpy(), rk), f"keys of level {l}"
        assert same_bits(weights.cpu().numpy(), rw), f"weights of level {l}"
    ref = dr.pdf(hist, levels)
    assert same_bits(pdf, ref)
    return pdf


# ---------------------------------------------------------------------- the segment sum alone
def test_segsum_alone_bit_for_bit(ctx):
    """every list length at which the number of blocks or passes changes, each in a bin of its own, among empty bins; weights over six decades with
    both signs; a lone -0.0 (one pass: +0.0); a full block of -0.0 (stays -0.0 through the later passes); a NaN (propagates); a permutation that is
    not the identity"""
    rng = np.random.default_rng(5)
    counts = [0, 1, 2, 255, 0, 256, 257, 65536, 0, 65537, 256, 0]
    nbins = len(counts)
    keys = np.repeat(np.arange(nbins), counts)
    w = 10.0 ** rng.uniform(-3.0, 3.0, keys.size) * rng.choice([-1.0, 1.0], keys.size)
    w[keys == 1] = -0.0
    w[keys == 10] = -0.0
    w[np.nonzero(keys == 6)[0][100]] = np.nan
    shuffle = rng.permutation(keys.size)
    keys, w = keys[shuffle], w[shuffle]
    dev = ctx.device
    sk, perm = torch.sort(torch.from_numpy(keys).to(dev), stable=True)
    assert not torch.equal(perm, torch.arange(keys.size, device=dev))
    off = torch.searchsorted(sk, torch.arange(nbins + 1, device=dev))
    part, o = diagnostics.segment_sums(ctx, torch.from_numpy(w).to(dev), perm, off, nbins)
    part, o = part.cpu().numpy(), o.cpu().numpy()
    order = np.argsort(keys, kind="stable")
    start = np.concatenate([[0], np.cumsum(counts)])
    for b in range(nbins):
        assert (o[b + 1] > o[b]) == (counts[b] > 0), b
        if counts[b] > 0:
            assert o[b + 1] - o[b] == 1
            ref = dr.tree_sum(w[order[start[b]:start[b + 1]]])
            assert same_bits(part[o[b]], ref), (b, counts[b], part[o[b]], ref)
    assert not np.signbit(part[o[1]]) and part[o[1]] == 0.0 and np.signbit(part[o[10]]) and np.isnan(part[o[6]])
    # without a permutation: the identity order of the sorted weights
    ws = torch.from_numpy(w[order]).to(dev)
    part2, o2 = diagnostics.segment_sums(ctx, ws, None, off, nbins)
    assert same_bits(part2.cpu().numpy()[o2.cpu().numpy()[:-1][np.array(counts) > 0]], part[o[:-1][np.array(counts) > 0]])


def test_entry_points_refuse_bad_arguments(ctx):
    L, sim = ctx.L, lattice_sim(ctx, "8x6x4")[0]
    buf = torch.zeros(64, dtype=torch.int64, device=ctx.device)
    p = C.c_void_p(buf.data_ptr())
    assert L.qk_diag_segsum(ctx.h, ctx.stream(), 1, None, p, p, 1, None, 0, 0, p) == capi.QK_ERR_INVALID
    assert L.qk_diag_segsum(ctx.h, ctx.stream(), -1, p, p, p, 1, None, 0, 0, p) == capi.QK_ERR_INVALID
    assert L.qk_diag_mask(sim.lev.h, ctx.stream(), None, 0, None, 0) == capi.QK_ERR_INVALID
    assert L.qk_diag_mask(sim.lev.h, ctx.stream(), p, 1, None, 8) == capi.QK_ERR_INVALID
    out = (C.c_double * 2)()
    assert L.qk_diag_minmax(sim.lev.h, ctx.stream(), sim.state_new_cc_.ptr, 0, None, 0, out) == capi.QK_ERR_INVALID
    assert L.qk_diag_minmax(sim.lev.h, ctx.stream(), sim.state_new_cc_.ptr, 0, p, 8, out) == capi.QK_ERR_INVALID  # scratch too small
    a = capi.DiagPdf()
    assert L.qk_diag_keys(sim.lev.h, ctx.stream(), C.byref(a), None, p, 192, p, p) == capi.QK_ERR_INVALID  # no variables
    a.nvars = 2
    for n in range(2):
        a.vars[n].table, a.vars[n].comp, a.vars[n].nbins, a.vars[n].width_t = sim.state_new_cc_.ptr, 0, 4097, 1.0
    assert L.qk_diag_keys(sim.lev.h, ctx.stream(), C.byref(a), None, p, 192, p, p) == capi.QK_ERR_UNSUPPORTED  # 4097^2 > 2^24 bins
    a.vars[1].nbins = 0
    assert L.qk_diag_keys(sim.lev.h, ctx.stream(), C.byref(a), None, p, 192, p, p) == capi.QK_ERR_INVALID
    a.vars[1].nbins = 4
    assert L.qk_diag_keys(sim.lev.h, ctx.stream(), C.byref(a), None, None, 192, p, p) == capi.QK_ERR_INVALID


# ---------------------------------------------------------------------- one level
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("lattice", sorted(LATTICES))
def test_keys_weights_and_pdf_bit_for_bit(ctx, lattice, config):
    sim, levels = lattice_sim(ctx, lattice)
    d = diagnostics.build_diagnostics(pdf_params(**CONFIGS[config]), diagnostics.available_names(sim))[0][0]
    pdf = check_against_restatement(sim, [sim], levels, d)
    assert pdf.shape == (d.total_bins,) and np.count_nonzero(pdf[np.isfinite(pdf)]) > 1
    assert same_bits(d.process(sim), pdf)  # the same diagnostic twice: identical bits


def test_volume_sum_is_exact_and_cell_counts_are_integers(ctx):
    sim, levels = lattice_sim(ctx, "16x8x12")
    names = diagnostics.available_names(sim)
    d = diagnostics.build_diagnostics(pdf_params(vars=[("y-GasMomentum", 9, 0, (-1.0, 1.0)), ("z-GasMomentum", 5, 0, (-1.0, 1.0))]), names)[0][0]
    pdf = check_against_restatement(sim, [sim], levels, d)
    assert float(np.sum(pdf)) == 16 * 8 * 12 * 0.125 ** 3  # the range covers every value; dyadic dx: no rounding anywhere
    d = diagnostics.build_diagnostics(pdf_params(vars=[("y-GasMomentum", 9, 0, (-1.0, 1.0))], weight_by="cell_counts"), names)[0][0]
    pdf = check_against_restatement(sim, [sim], levels, d)
    assert np.array_equal(pdf, np.floor(pdf)) and pdf.sum() == 16 * 8 * 12


@pytest.mark.parametrize("ndim,n,mgs", [(1, (40,), (24,)), (2, (12, 10), (8, 5))])
def test_lower_dimensions(ctx, ndim, n, mgs):
    """weightFac is dx0 in 1-D and dx0 * dx1 in 2-D"""
    sim = fill(make_sim(ctx, n, 0.25, mgs, ndim=ndim), seed=40 + ndim)
    assert sim.lev.nboxes == (2 if ndim == 1 else 4)
    d = diagnostics.build_diagnostics(pdf_params(vars=[E_AXIS, RHO_AXIS], weight_by="mass"), NAMES)[0][0]
    check_against_restatement(sim, [sim], [level_dict(sim)], d, ndim=ndim)
    d = diagnostics.build_diagnostics(pdf_params(vars=[("y-GasMomentum", 4, 0, (-1.0, 1.0))]), NAMES)[0][0]
    pdf = check_against_restatement(sim, [sim], [level_dict(sim)], d, ndim=ndim)
    assert float(np.sum(pdf)) == int(np.prod(n)) * 0.25 ** ndim


def test_one_bin_of_73728_weights_takes_three_passes(ctx):
    sim = fill(make_sim(ctx, (48, 48, 32), 0.125, (48, 48, 32)), seed=9, specials=False)
    n = 48 * 48 * 32
    assert n > 65536 and diagnostics.num_passes(n) == 3 == dr.num_passes(n)
    d = diagnostics.build_diagnostics(pdf_params(vars=[("gasEnergy", 1, 0, (0.0, 1.0))], weight_by="mass"), NAMES)[0][0]
    levels = [level_dict(sim)]
    pdf = check_against_restatement(sim, [sim], levels, d)
    w = (0.125 * 0.125) * 0.125 * np.concatenate([a.reshape(-1) for a in levels[0]["fields"]["gasDensity"]])
    left = 0.0
    for x in w.tolist():
        left = left + x
    print(f"S = {pdf[0]!r}, left to right {left!r}")
    assert pdf[0] != left and abs(pdf[0] - left) < 1.0e-10 * left  # the fixed tree, not the storage order


def test_range_from_the_field_uses_min_and_max_of_all_cells(ctx):
    sim, levels = lattice_sim(ctx, "16x8x12")
    lo, hi = dr.field_range(levels, "gasInternalEnergy")
    assert diagnostics._minmax(sim, sim.state_new_cc_, 5) == (lo, hi)
    with pytest.raises(capi.QkError, match="not finite"):
        diagnostics._minmax(sim, sim.state_new_cc_, 4)  # gasEnergy holds a NaN and infinities


# ---------------------------------------------------------------------- a two-level hierarchy
def two_level_amr(ctx, seed=21):
    """16^3 cells on [0, 1]^3 (dx = 1/16) with one fixed 16^3 fine box over the 8^3 coarse cells [4, 11]^3"""
    geom = Geometry(3, [16, 16, 16], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 0, 0])
    bcs = [([capi.BC_FOEXTRAP] * 3, [capi.BC_FOEXTRAP] * 3) for _ in range(6)]
    amr = AmrSimulation(ctx, geom, capi.traits(5.0 / 3.0, False, 3), bcs, 1, 16, 8)
    amr.static_fine_boxes = [[([8, 8, 8], [23, 23, 23])]]

    def ic_for(geom_l):
        def ic(i, j, k):
            U = np.zeros((6,) + i.shape)
            U[0], U[4], U[5] = 1.0, 1.5, 1.5
            return U
        return ic
    amr.initial_conditions = ic_for
    amr.setInitialConditions()
    assert amr.finest_level == 1 and amr.levels[1].all_boxes == [([8, 8, 8], [23, 23, 23])]
    rng = np.random.default_rng(seed)
    for L in amr.levels:
        for b, (lo, hi) in enumerate(L.lev.boxes):
            L.state_new_cc_.valid(b).copy_(torch.from_numpy(random_state(rng, dr.box_shape(lo, hi))))
    amr.derivedNames_, amr.ComputeDerivedVar = ["half_energy"], half_energy
    return amr


def test_two_level_hierarchy(ctx):
    amr = two_level_amr(ctx)
    levels = [level_dict(L) for L in amr.levels]
    names = diagnostics.available_names(amr)
    d = diagnostics.build_diagnostics(pdf_params(vars=[E_AXIS, RHO_AXIS], weight_by="mass"), names)[0][0]
    mask = d.level_mask(amr.levels[0], amr.levels[1].all_boxes)
    ref_mask = dr.fine_mask(levels[0]["boxes"], levels[1]["boxes"])
    for b in range(amr.levels[0].lev.nboxes):
        assert np.array_equal(mask.valid(b)[0].cpu().numpy(), ref_mask[b])
    assert sum(int(m.sum()) for m in ref_mask) == 16 ** 3 - 8 ** 3
    assert d.level_mask(amr.levels[1], None) is None
    check_against_restatement(amr, amr.levels, levels, d)
    d = diagnostics.build_diagnostics(pdf_params(vars=[("half_energy", 8, 0, None)], filters=[("f", "gasDensity", "value_greater", 1.0)]), names)[0][0]
    with pytest.raises(capi.QkError, match="half_energy is not finite"):
        d.process(amr)  # the range is taken from the field on every level: gasEnergy holds values that are not finite
    d = diagnostics.build_diagnostics(pdf_params(vars=[("y-GasMomentum", 8, 0, None), ("z-GasMomentum", 3, 0, (-1.0, 1.0))]), names)[0][0]
    check_against_restatement(amr, amr.levels, levels, d)
    d = diagnostics.build_diagnostics(pdf_params(vars=[("y-GasMomentum", 8, 0, (-1.0, 1.0))]), names)[0][0]
    pdf = check_against_restatement(amr, amr.levels, levels, d)
    assert float(np.sum(pdf)) == 1.0  # (16^3 - 8^3) / 16^3 + 16^3 / 32^3: a covered coarse cell is not counted twice


# ---------------------------------------------------------------------- the driver
def kernel_names(ctx, prefix):
    names = []
    for k in range(ctx.L.qk_profile_num_kernels(ctx.h)):
        name, cnt, ms = C.c_char_p(), C.c_long(), C.c_double()
        ctx.check(ctx.L.qk_profile_get(ctx.h, k, C.byref(name), C.byref(cnt), C.byref(ms)), "qk_profile_get")
        if cnt.value > 0 and name.value.decode().startswith(prefix):
            names.append(name.value.decode())
    return sorted(names)


def blob(sim):
    dx = sim.geom.dx

    def ic(i, j, k):
        x, y, z = (i + 0.5) * dx[0], (j + 0.5) * dx[1], (k + 0.5) * dx[2]
        U = np.zeros((6,) + i.shape)
        U[0] = 1.0 + 4.0 * np.exp(-0.5 * ((x - 0.9) ** 2 + (y - 1.1) ** 2 + (z - 1.0) ** 2) / 0.3 ** 2)
        U[5] = 0.1 * U[0] ** (5.0 / 3.0) / (5.0 / 3.0 - 1.0)
        U[4] = U[5]
        return U
    return ic


def driver_sim(ctx):
    sim = make_sim(ctx, (16, 16, 16), 0.125, (8, 16, 16))
    return sim, blob(sim)


def state_of(sim):
    return np.stack([sim.state_new_cc_.valid(b).cpu().numpy() for b in range(sim.lev.nboxes)])


def test_nothing_configured_launches_nothing_and_keeps_the_bits(ctx):
    plain, ic = driver_sim(ctx)
    plain.set_initial_conditions(ic)
    for _ in range(3):
        assert plain.step()  # (step() has no diagnostics hook at all: the parent's path)
    sim, ic = driver_sim(ctx)
    ctx.L.qk_profile_reset(ctx.h)
    ctx.L.qk_profile_enable(ctx.h, 1)
    try:
        sim.set_initial_conditions(ic)
        sim.maxTimesteps_ = 3
        assert sim.evolve() and sim.istep == 3
        assert sim.doDiagnostics() == []
        names = kernel_names(ctx, "")
    finally:
        ctx.L.qk_profile_enable(ctx.h, 0)
        ctx.L.qk_profile_reset(ctx.h)
    assert names and not [n for n in names if n.startswith("diag")]
    assert same_bits(state_of(sim), state_of(plain)) and sim.tNew_ == plain.tNew_


def test_evolve_writes_the_files_of_steps_0_2_4(ctx, tmp_path):
    sim, ic = driver_sim(ctx)
    stem = str(tmp_path / "PDFDensEnergy")
    sim.createDiagnostics(pdf_params(int=2, file=stem, weight_by="mass", vars=[("gasDensity", 6, 1, (0.5, 8.0)), ("gasInternalEnergy", 5, 0, None)]))
    assert sim.m_diagVars == ["gasDensity", "gasInternalEnergy"] and len(sim.m_diagnostics) == 1
    got, orig = [], sim.doDiagnostics
    sim.doDiagnostics = lambda: got.extend((sim.istep, p, pdf.copy()) for p, pdf in orig())
    ctx.L.qk_profile_reset(ctx.h)
    ctx.L.qk_profile_enable(ctx.h, 1)
    try:
        sim.set_initial_conditions(ic)
        sim.maxTimesteps_ = 4
        assert sim.evolve() and sim.istep == 4
        names = kernel_names(ctx, "diag")
    finally:
        ctx.L.qk_profile_enable(ctx.h, 0)
        ctx.L.qk_profile_reset(ctx.h)
    assert names == ["diag_keys", "diag_minmax", "diag_segsum"]  # (one level: no mask)
    assert [(s, os.path.basename(p)) for s, p, _ in got] == [(0, "PDFDensEnergy000000.dat"), (2, "PDFDensEnergy000002.dat"), (4, "PDFDensEnergy000004.dat")]
    assert sorted(os.listdir(tmp_path)) == [os.path.basename(p) for _, p, _ in got]
    d = sim.m_diagnostics[0]
    assert d.last_path == got[-1][1] and same_bits(d.last_pdf, got[-1][2])
    for step, path, pdf in got:
        header, rows = diagnostics.read_pdf_file(path)
        assert int(header["cycle"][0]) == step and header["variables"] == ["gasDensity", "gasInternalEnergy"] and header["is_log_spaced"] == ["1", "0"]
        assert rows.shape == (30, 7) and same_bits(rows[:, 6], pdf)  # %.17e round-trips every double
        assert np.array_equal(rows[:, 0] * 5 + rows[:, 3], np.arange(30))
    assert float(header["time"][0]) == sim.tNew_
    # mass-weighted, the density axis covers every cell, the energy axis is taken from the field (its maximum sits on the upper edge and is dropped)
    total = sum(float(((0.125 * 0.125) * 0.125 * sim.state_new_cc_.valid(b)[0]).sum()) for b in range(sim.lev.nboxes))
    assert 0.9 * total < got[-1][2].sum() <= total * (1.0 + 1.0e-12)
    assert not same_bits(got[0][2], got[2][2])
    assert same_bits(d.process(sim), got[-1][2])  # process() computes without writing
    assert sorted(os.listdir(tmp_path)) == [os.path.basename(p) for _, p, _ in got]


REFUSALS = {
    "DiagFramePlane": ({"quokka.h.type": "DiagFramePlane"}, "DiagFramePlane is not built"),
    "unknown_type": ({"quokka.h.type": "DiagSomething"}, "DiagSomething is not built"),
    "no_interval": ({"quokka.h.int": -1}, r"quokka\.h\.int and quokka\.h\.per must be > 0"),
    "missing_nBins": ({"quokka.h.gasDensity.nBins": None}, r"quokka\.h\.gasDensity\.nBins is missing"),
    "filter_without_field": ({"quokka.h.filters": "f", "quokka.h.f.value_less": 1.0}, r"filter: quokka\.h\.f is missing a field_name"),
    "filter_without_range": ({"quokka.h.filters": "f", "quokka.h.f.field_name": "gasEnergy"}, r"filter: quokka\.h\.f is missing a range definition"),
    "weight_by": ({"quokka.h.weight_by": "energy"}, "Invalid histogram weight type! Must be either 'volume', 'mass' or 'cell_counts'."),
    "unknown_field": ({"quokka.h.var_names": "nH", "quokka.h.nH.nBins": 4}, r"\[Diagnostics\] Field nH is not available!"),
    "unknown_filter_field": ({"quokka.h.filters": "f", "quokka.h.f.field_name": "entropy", "quokka.h.f.value_less": 1.0},
                             r"\[Diagnostics\] Field entropy is not available!"),
    "log_nonpositive_given": ({"quokka.h.gasDensity.range": [0.0, 10.0]}, "For log-spaced bins, histogram bounds must be positive!"),
    "nonfinite_given": ({"quokka.h.gasDensity.range": ["1.0", "inf"]}, "is not finite"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_at_creation(ctx, case):
    sim, _ = driver_sim(ctx)
    params = pdf_params(vars=[("gasDensity", 4, 1, (0.5, 8.0))])
    change, message = REFUSALS[case]
    for k, v in change.items():
        if v is None:
            del params[k]
        else:
            params[k] = v
    with pytest.raises(capi.QkError, match=message):
        sim.createDiagnostics(params)
    assert sim.m_diagnostics == []


def test_refusals_at_output_and_for_several_ranks(ctx):
    sim, ic = driver_sim(ctx)
    sim.set_initial_conditions(ic)
    sim.state_new_cc_.valid(0)[1, 2, 3, 1] = -0.25
    sim.createDiagnostics(pdf_params(vars=[("x-GasMomentum", 4, 1, None)]))
    with pytest.raises(capi.QkError, match="For log-spaced bins, histogram bounds must be positive!"):
        sim.doDiagnostics()  # the range taken from the field has a non-positive bound
    sim.state_new_cc_.valid(1)[1, 2, 3, 1] = float("inf")
    with pytest.raises(capi.QkError, match="the range of field x-GasMomentum is not finite"):
        sim.doDiagnostics()
    sim.nranks = 2
    with pytest.raises(capi.QkError, match="nranks > 1"):
        sim.createDiagnostics(pdf_params(vars=[("gasDensity", 4, 1, (0.5, 8.0))]))
    with pytest.raises(capi.QkError, match="nranks > 1"):
        sim.doDiagnostics()
    sim.nranks = 1
    amr = AmrSimulation(ctx, sim.geom, sim.traits, [([capi.BC_FOEXTRAP] * 3, [capi.BC_FOEXTRAP] * 3) for _ in range(6)], 1, 16, 8, nranks=2)
    with pytest.raises(capi.QkError, match="nranks > 1"):
        amr.createDiagnostics(pdf_params(vars=[("gasDensity", 4, 1, (0.5, 8.0))]))
