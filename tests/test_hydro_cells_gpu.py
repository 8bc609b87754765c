"""The hydro Riemann fans and cell-update operators (csrc/qk_device.hpp hllc / hlldHydro / llf / faceFlux / scalarFlux / enforceLimits /
syncDualEnergy / signalSpeed through the qk_hydro_* entries of csrc/qk_hydro_ops.hip) against the array-level entries of the oracle, bit for bit,
on inputs built to take every branch.  The faces and cells come from tests/hydro_cells_reference.py; tests/test_hydro_cells_reference.py holds the
oracle entries themselves to the defining statements on the CPU and asserts the same population conditions there.

Every comparison: where the oracle is finite the bits are equal, where it is not the GPU is not finite either.  Ghost cells hold NaN (or a
sentinel) and are asserted untouched.  Every case asserts from the classifier that the branches it targets hold at least 1 % of its samples and at
least 256 of them before it compares a value.  One box of at most 32^3 per launch, plus a two-box level of unequal boxes (17 x 5 x 3 next to
7 x 5 x 3) for the per-box indexing and the maxlen masking of launchCells, k_maxSignal and k_fixupState (its few hundred cells carry the same
cell mix; the population condition is asserted on the large box).

HLLD: its branch `rhoStarL <= 0` (qk_device.hpp hlldHydro, the NaN of the reference's left Alfven speed) cannot be reached from finite states with
positive densities — in the left star fan S_L < 0 <= S_M, so rhoStarL = rho_L (S_L - u_L) / (S_L - S_M) is a positive density times the quotient
of two negative numbers — and states that are not (NaN, zero density) are outside the flux comparison: no case targets it.

Measured on an MI355X: the 104 cases of this file take 2.9 s together."""
import ctypes as C

import numpy as np
import pytest
import torch

import hydro_cells_reference as H
from quokka_amd.hydro_system import HydroSystem
from quokka_amd.multifab import Level, MultiFab

pytestmark = pytest.mark.gpu
NAN = float("nan")
NG = 2


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def assert_same_bits(got, want, what=""):
    """every value the oracle has finite: equal in every bit; where the oracle is not finite, neither is the GPU (the rule of
    tests/test_rad_source_cells_gpu.py: divBy documents a different non-number for a zero or subnormal denominator)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    diff = fin & (bits(got) != bits(want))
    if diff.any():
        i = tuple(np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {diff.sum()} of {fin.sum()} finite values differ; first at {i}: GPU {got[i]!r} oracle {want[i]!r}")
    assert not np.isfinite(got[~fin]).any(), f"{what}: the GPU is finite where the oracle is not"


# ------------------------------------------------------------------------------------------------ qk_hydro_ComputeFluxes
FLUX_CASES = H.flux_cases()


def gpu_face_fluxes(ctx, case, L, R, prim, vlo, vhi):
    lev = Level(ctx, case.ndim, [(vlo, vhi)])
    nv = 6 + case.nscalars
    hs = HydroSystem(case.eos.device_traits(case.ndim, case.reconstruct_eint, case.nscalars))
    Lm, Rm = MultiFab(lev, nv, 0, facedir=case.d), MultiFab(lev, nv, 0, facedir=case.d)
    Pm = MultiFab(lev, nv, 1)
    Fm, Vm = MultiFab(lev, nv, 1, facedir=case.d, fill=NAN), MultiFab(lev, 1, 1, facedir=case.d, fill=NAN)
    Lm.set_fab(0, L)
    Rm.set_fab(0, R)
    Pm.set_fab(0, prim)
    hs.ComputeFluxes(lev, case.riemann, case.d, Fm, Vm, Lm, Rm, Pm, case.K_visc)
    torch.cuda.synchronize()
    F, V = Fm.fab_numpy(0), Vm.fab_numpy(0)
    inn = H.interior(1, case.ndim)
    ghost = np.ones(F.shape[1:], dtype=bool)
    ghost[inn[1:]] = False
    assert np.isnan(F[:, ghost]).all() and np.isnan(V[:, ghost]).all(), "faces outside the face box written"
    return np.ascontiguousarray(F[inn]), np.ascontiguousarray(V[inn][0])


@pytest.mark.parametrize("case", FLUX_CASES, ids=lambda c: c.id)
def test_compute_fluxes_on_generated_states_bit_for_bit(ctx, oracle, case):
    """every face an independent sample: L and R drawn freely, the primitives only supply du, dvl, dvr, dwl, dwr (their other components are NaN
    and must not be read).  Flux of every component — the passive scalars in all four fans — and the face velocity."""
    L, R, prim, vlo, vhi = case.build()
    cl = case.classify(L, R, prim)
    H.assert_populations(case.id, cl, case.targets)
    Fo, Vo = oracle.hydro_face_fluxes(case.eos.oracle_traits(case.ndim, case.reconstruct_eint, case.nscalars), case.riemann, case.d, L, R, prim, vlo, vhi, 1,
                                      case.K_visc)
    assert np.isfinite(Fo).all() and np.isfinite(Vo).all()
    Fg, Vg = gpu_face_fluxes(ctx, case, L, R, prim, vlo, vhi)
    assert_same_bits(Fg, Fo, case.id + " flux")
    assert_same_bits(Vg, Vo, case.id + " face velocity")
    if case.nscalars > 0 and case.riemann == H.HLLC:
        for fan in ("fan_L", "star_L", "star_R", "fan_R"):  # (compared above; here: the scalar fluxes are populated in every fan)
            assert (Fo[6:][:, cl[fan]] != 0.0).any(), fan


# ------------------------------------------------------------------------------------------------ cell-local operators
class Cells:
    """one level (one box or two unequal ones) holding n generated cells, box after box, x fastest"""

    def __init__(self, ctx, boxes, ndim=3):
        self.ctx, self.boxes, self.ndim = ctx, boxes, ndim
        self.lev = Level(ctx, ndim, boxes)
        self.counts = [int(np.prod(H.box_shape(lo, hi))) for lo, hi in boxes]
        self.n = sum(self.counts)

    def split(self, U):
        out, o = [], 0
        for c in self.counts:
            out.append(np.ascontiguousarray(U[..., o:o + c]))
            o += c
        return out

    def mf(self, U, ng=NG, dtype=torch.float64, fill=NAN):
        """MultiFab of the cells U [ncomp, n] with `fill` in the ghost cells"""
        m = MultiFab(self.lev, U.shape[0], ng, dtype=dtype, fill=None if dtype != torch.float64 else fill)
        for b, ((lo, hi), part) in enumerate(zip(self.boxes, self.split(U))):
            fab = np.full((U.shape[0],) + H.box_shape(lo, hi, ng, self.ndim), fill if dtype == torch.float64 else 0, dtype=np.float64 if dtype == torch.float64 else np.int32)
            fab[H.interior(ng, self.ndim)] = part.reshape((U.shape[0],) + H.box_shape(lo, hi))
            m.set_fab(b, fab)
        return m

    def fabs(self, U, ng=NG, fill=NAN):
        return [H.embed(part, lo, hi, ng, self.ndim) if np.isnan(fill) else self._embed(part, lo, hi, ng, fill) for (lo, hi), part in zip(self.boxes, self.split(U))]

    def _embed(self, part, lo, hi, ng, fill):
        fab = np.full((part.shape[0],) + H.box_shape(lo, hi, ng, self.ndim), fill)
        fab[H.interior(ng, self.ndim)] = part.reshape((part.shape[0],) + H.box_shape(lo, hi))
        return fab

    def valid(self, m, ng=NG, fill=NAN):
        """the valid cells of MultiFab m as [ncomp, n]; asserts the ghost cells still hold `fill`"""
        parts = []
        for b, (lo, hi) in enumerate(self.boxes):
            a = m.fab_numpy(b)
            g = H.ghost_mask(lo, hi, ng, self.ndim)
            assert (np.isnan(a[:, g]).all() if np.isnan(fill) else (a[:, g] == fill).all()), "ghost cells written"
            parts.append(a[H.interior(ng, self.ndim)].reshape(a.shape[0], -1))
        return np.concatenate(parts, axis=1)

    def gather(self, per_box):
        """per-box oracle fabs (ghosted) -> [ncomp, n]"""
        return np.concatenate([a[H.interior(NG, self.ndim)].reshape(a.shape[0], -1) for a in per_box], axis=1)


LAYOUTS = {"box": [H.CELL_BOX], "two-boxes": H.TWO_BOXES}


@pytest.fixture(scope="module", params=list(LAYOUTS), ids=list(LAYOUTS))
def cells(request, ctx):
    return Cells(ctx, LAYOUTS[request.param])


def check_populations(cells, what, classes, targets):
    """the population condition, on the box large enough to hold it (the two-box level carries the same mix in a few hundred cells: there, present)"""
    if cells.n >= 12 * H.MIN_COUNT:  # (the generators deal the cells into up to twelve groups)
        H.assert_populations(what, classes, targets)
    else:
        for k in targets:
            assert classes[k].any(), (what, k)


EOS_IDS = [f"{u}-g{g:.3g}" for u, g in H.CELL_EOS]


@pytest.mark.parametrize("units,gamma", H.CELL_EOS, ids=EOS_IDS)
@pytest.mark.parametrize("reconstruct_eint", [False, True])
def test_conserved_to_primitive_on_the_extreme_cells(cells, oracle, units, gamma, reconstruct_eint):
    """the cells of the dual-energy case (kinetic-dominated, E_tot < 0, rho == 0, rho < 0) and of the signal-speed case (at rest, E - E_kin < 0)"""
    eos = H.Eos(H.UNITS[units], gamma)
    U = np.concatenate([H.dual_energy_cells(eos, cells.n, 41, H.NSCAL)[:, :cells.n // 2], np.concatenate(
        [H.signal_cells(eos, cells.n, 42), np.ones((H.NSCAL, cells.n))], axis=0)[:, cells.n // 2:]], axis=1)
    hs = HydroSystem(eos.device_traits(3, reconstruct_eint, H.NSCAL))
    cons, prim = cells.mf(U), cells.mf(np.full_like(U, NAN))
    hs.ConservedToPrimitive(cells.lev, cons, prim, 0)
    torch.cuda.synchronize()
    got = cells.valid(prim)
    t = eos.oracle_traits(3, reconstruct_eint, H.NSCAL)
    want = cells.gather([oracle.cons_to_prim(t, fab, *oracle._grown(t, lo, hi, NG)) for (lo, hi), fab in zip(cells.boxes, cells.fabs(U))])
    assert_same_bits(got, want, "ConservedToPrimitive")


@pytest.mark.parametrize("units,gamma", H.CELL_EOS, ids=EOS_IDS)
@pytest.mark.parametrize("floor_zero", [False, True], ids=["floor+", "floor0"])
def test_enforce_limits_against_the_oracle(cells, oracle, units, gamma, floor_zero):
    eos = H.Eos(H.UNITS[units], gamma)
    U, rf, Tf = H.limits_cells(eos, cells.n, 31, H.NSCAL, H.NMSCAL, floor_zero)
    check_populations(cells, "EnforceLimits", H.classify_limits(eos, U, rf, Tf, H.NSCAL, H.NMSCAL), H.limits_targets(eos, floor_zero))
    t = eos.oracle_traits(3, True, H.NSCAL)
    want = cells.gather([oracle.hydro_enforce_limits(t, fab, lo, hi, NG, rf, Tf, nmscalars=H.NMSCAL) for (lo, hi), fab in zip(cells.boxes, cells.fabs(U))])
    S = cells.mf(U)
    HydroSystem(eos.device_traits(3, True, H.NSCAL, H.NMSCAL)).EnforceLimits(cells.lev, rf, Tf, S)
    torch.cuda.synchronize()
    assert_same_bits(cells.valid(S), want, "EnforceLimits")


@pytest.mark.parametrize("units,gamma", H.CELL_EOS, ids=EOS_IDS)
@pytest.mark.parametrize("with_fatal", [True, False], ids=["fatal", "no-fatal"])
def test_sync_dual_energy_against_the_oracle(cells, oracle, units, gamma, with_fatal):
    """the flag is raised exactly when the oracle reports a cell the reference aborts on (rho <= 0); such cells are left untouched"""
    eos = H.Eos(H.UNITS[units], gamma)
    U = H.dual_energy_cells(eos, cells.n, 32)
    c = H.classify_dual_energy(U)
    if not with_fatal:
        U[0] = np.where(c["fatal_rho_le_0"], 1.0, np.abs(U[0]))
        U[0] = np.where(U[0] == 0.0, 1.0, U[0])
        c = H.classify_dual_energy(U)
        assert not c["fatal_rho_le_0"].any()
    check_populations(cells, "SyncDualEnergy", c, H.DUAL_TARGETS if with_fatal else H.DUAL_TARGETS[1:3])
    t = eos.oracle_traits(3, True, 0)
    res = [oracle.hydro_sync_dual_energy(t, fab, lo, hi, NG) for (lo, hi), fab in zip(cells.boxes, cells.fabs(U))]
    want = cells.gather([r[0] for r in res])
    fatal = np.concatenate([r[1].reshape(-1) for r in res])
    assert fatal.any() == with_fatal
    S = cells.mf(U)
    err = torch.zeros(1, dtype=torch.int32, device=cells.ctx.device)
    HydroSystem(eos.device_traits(3, True, 0)).SyncDualEnergy(cells.lev, S, err)
    torch.cuda.synchronize()
    got = cells.valid(S)
    assert int(err.item()) == int(with_fatal)
    assert np.array_equal(bits(got[:, fatal]), bits(U[:, fatal])), "a fatal cell was modified"
    assert_same_bits(got, want, "SyncDualEnergy")


@pytest.mark.parametrize("units,gamma", H.CELL_EOS, ids=EOS_IDS)
def test_signal_speeds_against_the_oracle(cells, oracle, units, gamma):
    """ComputeMaxSignalSpeed as an array, and both reductions; cells whose thermal energy is negative give NaN (first, last and middle cell of the
    level among them) and must not win the maximum"""
    eos = H.Eos(H.UNITS[units], gamma)
    U = H.signal_cells(eos, cells.n, 33)
    check_populations(cells, "signal speed", H.classify_signal(eos, U), H.signal_targets(eos))
    t = eos.oracle_traits(3, True, 0)
    fabs = cells.fabs(U)
    want = np.concatenate([oracle.hydro_max_signal_speed(t, fab, lo, hi, NG).reshape(1, -1) for (lo, hi), fab in zip(cells.boxes, fabs)], axis=1)
    hs = HydroSystem(eos.device_traits(3, True, 0))
    cons, sig = cells.mf(U), cells.mf(np.full((1, cells.n), -2.5), fill=-2.5)
    hs.ComputeMaxSignalSpeed(cells.lev, cons, sig)
    torch.cuda.synchronize()
    assert_same_bits(cells.valid(sig, fill=-2.5), want, "ComputeMaxSignalSpeed")
    if not eos.isothermal:
        assert np.isnan(want[0, 0]) and np.isnan(want[0, -1]) and np.isfinite(want).any()
    for which in (0, 1):
        m = max(oracle.hydro_max_signal_local(t, which, fab, lo, hi, NG) for (lo, hi), fab in zip(cells.boxes, fabs))
        got = float(hs.maxSignalSpeedLocal(cells.lev, cons, which=which).item())
        assert np.isfinite(m) and bits(np.float64(got)) == bits(np.float64(m)), (which, got, m)


@pytest.mark.parametrize("units,gamma", H.CELL_EOS[:2], ids=EOS_IDS[:2])
@pytest.mark.parametrize("nvars", [9, 7])
def test_predict_step_against_the_oracle(cells, oracle, units, gamma, nvars):
    """state, flags and the counter; nvars = 7 is too small for the mass-scalar check to apply (the scalars beyond it are not written)"""
    eos = H.Eos(H.UNITS[units], gamma)
    U, rhs, dt = H.predict_cells(eos, cells.n, 34, H.NSCAL, H.NMSCAL)
    check_populations(cells, "PredictStep", H.classify_predict(U, rhs, dt, H.NMSCAL), H.PREDICT_TARGETS)
    t = eos.oracle_traits(3, True, H.NSCAL)
    new0 = np.full_like(U, -3.25)
    rparts = cells.split(np.ascontiguousarray(rhs[:nvars]))
    res = [oracle.hydro_predict_step(t, fab, n0, r.reshape((nvars,) + H.box_shape(lo, hi)), dt, nvars, lo, hi, NG, nmscalars=H.NMSCAL)
           for (lo, hi), fab, n0, r in zip(cells.boxes, cells.fabs(U), cells.fabs(new0, fill=-3.25), rparts)]
    want = cells.gather([r[0] for r in res])
    wflags = np.concatenate([r[1].reshape(-1) for r in res])
    wcount = sum(r[2] for r in res)
    assert 0 < wcount < cells.n
    old, new = cells.mf(U), cells.mf(new0, fill=-3.25)
    R = cells.mf(np.ascontiguousarray(rhs[:nvars]), ng=0)
    flags = MultiFab(cells.lev, 1, 0, dtype=torch.int32)
    flags.storage.fill_(-1)
    cnt = torch.zeros(1, dtype=torch.int64, device=cells.ctx.device)
    HydroSystem(eos.device_traits(3, True, H.NSCAL, H.NMSCAL)).PredictStep(cells.lev, old, new, R, dt, nvars, flags, cnt)
    torch.cuda.synchronize()
    assert_same_bits(cells.valid(new, fill=-3.25), want, "PredictStep")
    gflags = np.concatenate([flags.fab_numpy(b).reshape(-1) for b in range(len(cells.boxes))])
    assert np.array_equal(gflags, wflags) and int(cnt.item()) == wcount


@pytest.mark.parametrize("units,gamma", H.CELL_EOS, ids=EOS_IDS)
@pytest.mark.parametrize("floor_zero,dual", [(False, 1), (True, 1), (False, 0)], ids=["floor+-dual", "floor0-dual", "floor+-nodual"])
def test_fixup_state_against_the_oracle_chain(cells, oracle, units, gamma, floor_zero, dual):
    """qk_hydro_FixupState against the oracle's EnforceLimits, SyncDualEnergy and the two maxima: the fused pass one hop from the oracle"""
    eos = H.Eos(H.UNITS[units], gamma)
    U, rf, Tf = H.limits_cells(eos, cells.n, 37, H.NSCAL, H.NMSCAL, floor_zero)
    check_populations(cells, "FixupState", H.classify_limits(eos, U, rf, Tf, H.NSCAL, H.NMSCAL), H.limits_targets(eos, floor_zero))
    t = eos.oracle_traits(3, True, H.NSCAL)
    outs, fatal_any, maxima = [], False, [-np.inf, -np.inf]
    for (lo, hi), fab in zip(cells.boxes, cells.fabs(U)):
        a = oracle.hydro_enforce_limits(t, fab, lo, hi, NG, rf, Tf, nmscalars=H.NMSCAL)
        if dual:
            a, fatal = oracle.hydro_sync_dual_energy(t, a, lo, hi, NG)
            fatal_any = fatal_any or bool(fatal.any())
        for w in (0, 1):
            maxima[w] = max(maxima[w], oracle.hydro_max_signal_local(t, w, a, lo, hi, NG))
        outs.append(a)
    assert fatal_any == bool(floor_zero and dual)  # (floor 0: the cells with rho <= 0 stay at rho = 0)
    S = cells.mf(U)
    ctx = cells.ctx
    tr = eos.device_traits(3, True, H.NSCAL, H.NMSCAL)
    err = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    sig = torch.full((2,), -1.0, dtype=torch.float64, device=ctx.device)
    ctx.check(ctx.L.qk_hydro_FixupState(cells.lev.h, ctx.stream(), C.byref(tr), rf, Tf, dual, S.ptr, C.c_void_p(err.data_ptr()), C.c_void_p(sig.data_ptr())),
              "qk_hydro_FixupState")
    torch.cuda.synchronize()
    assert_same_bits(cells.valid(S), cells.gather(outs), "FixupState")
    assert int(err.item()) == int(fatal_any)
    # (floor 0, isothermal: a cell left at rho = 0 with momentum has |v| = inf and c_s = cs_iso: the maximum is +inf on both sides)
    assert not np.isnan(maxima).any() and np.array_equal(bits(np.array(sig.tolist())), bits(np.array(maxima))), (sig.tolist(), maxima)


# ------------------------------------------------------------------------------------------------ stencil operators
STENCIL = [(3, 8, [([0, 0, 0], [20, 14, 10])]), (3, 6, H.TWO_BOXES), (2, 6, [([0, 0, 0], [40, 26, 0])]), (1, 8, [([0, 0, 0], [300, 0, 0])])]


@pytest.mark.parametrize("units,gamma", H.CELL_EOS, ids=EOS_IDS)
@pytest.mark.parametrize("ndim,nvars,boxes", STENCIL, ids=["3d-8", "3d-two-boxes-6", "2d-6", "1d-8"])
def test_rhs_from_fluxes_and_pdv_against_the_oracle(ctx, oracle, units, gamma, ndim, nvars, boxes):
    """ComputeRhsFromFluxes with unequal dx, then AddInternalEnergyPdV with a random redo-flag array: both divergence formulas in one launch"""
    eos = H.Eos(H.UNITS[units], gamma)
    ns = nvars - 6
    dx = [0.37, 1.3, 2.9]
    lev = Level(ctx, ndim, boxes)
    hs = HydroSystem(eos.device_traits(ndim, True, ns))
    t = eos.oracle_traits(ndim, True, ns)
    rng = np.random.default_rng(35)
    Fm = [MultiFab(lev, nvars, 0, facedir=d) for d in range(ndim)]
    Vm = [MultiFab(lev, 1, 0, facedir=d) for d in range(ndim)]
    Um = MultiFab(lev, nvars, 1)
    Rm = MultiFab(lev, nvars, 1, fill=NAN)
    flag = MultiFab(lev, 1, 0, dtype=torch.int32)
    want_rhs, want_pdv, nflag = [], [], 0
    for b, (lo, hi) in enumerate(boxes):
        U = H._base_cells(eos, rng, int(np.prod(H.box_shape(lo, hi, 1, ndim))), ns).reshape((nvars,) + H.box_shape(lo, hi, 1, ndim))
        scale, vscale = float(np.median(np.abs(U[4]))), float(np.median(np.abs(U[1] / U[0])))
        fluxes = [scale * rng.standard_normal((nvars,) + H.box_shape(lo, hi, 0, ndim, d)) for d in range(ndim)]
        vels = [vscale * rng.standard_normal(H.box_shape(lo, hi, 0, ndim, d)) for d in range(ndim)]
        redo = (rng.random(H.box_shape(lo, hi)) < 0.4).astype(np.int32)
        nflag += int(redo.sum())
        for d in range(ndim):
            Fm[d].set_fab(b, fluxes[d])
            Vm[d].set_fab(b, vels[d][None])
        Um.set_fab(b, U)
        flag.set_fab(b, redo[None])
        rhs = oracle.hydro_rhs_from_fluxes(t, fluxes, dx, nvars, lo, hi)
        want_rhs.append(rhs)
        want_pdv.append(oracle.hydro_add_pdv(t, rhs, U, dx, vels, redo, lo, hi, 1))
    ncell = lev.num_cells()
    assert 0.3 * ncell < nflag < 0.5 * ncell  # both formulas, each on far more than 1 % of the cells
    hs.ComputeRhsFromFluxes(lev, Rm, Fm, dx, nvars)
    torch.cuda.synchronize()
    inn = H.interior(1, ndim)
    for b, (lo, hi) in enumerate(boxes):
        a = Rm.fab_numpy(b)
        assert np.isnan(a[:, H.ghost_mask(lo, hi, 1, ndim)]).all()
        assert_same_bits(a[inn], want_rhs[b], f"ComputeRhsFromFluxes box {b}")
    hs.AddInternalEnergyPdV(lev, Rm, Um, dx, Vm, flag)
    torch.cuda.synchronize()
    for b, (lo, hi) in enumerate(boxes):
        a = Rm.fab_numpy(b)
        assert np.isnan(a[:, H.ghost_mask(lo, hi, 1, ndim)]).all()
        assert_same_bits(a[inn], want_pdv[b], f"AddInternalEnergyPdV box {b}")
        assert not np.array_equal(a[inn][5], want_rhs[b][5])
