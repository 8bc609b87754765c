"""The multigroup matter-radiation exchange kernels (csrc/qk_rad_mg_launch.hpp k_rad_source_mg<NG, DUST, MC>, arithmetic in qk_rad_mg_device.hpp)
cell by cell against the per-cell multigroup entry of the oracle: every NG instantiation, the three opacity models, lower values that depend on
rho and T, both stages, the isothermal EOS, the rarely taken arithmetic branches (each case asserts from the oracle's branch mask that its cells
took the branch), the failure counters with non-zero values and the launch geometry.  The cells come from tests/rad_mg_source_reference.py;
tests/test_rad_mg_source_reference.py holds the oracle itself and the generator's caps on the CPU.

The device libm and glibc differ in the last place, so where pow / exp / log / log10 enter, the yardstick is the oracle against itself with those
four functions moved by up to JITTER_ULPS ulps (3 seeds); where none enters, every bit.

One 3-D level of two boxes of different size, 20 x 8 x 8 and 11 x 8 x 8 (1280 + 704 = 1984 cells per launch: the grid sized for the larger box
over-covers the smaller one, whose cells end partway through a block at a wave boundary), two ghost cells holding NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import rad_mg_source_reference as M
from quokka_amd.multifab import Level, MultiFab

pytestmark = pytest.mark.gpu
NGROW = 2
EPS = np.finfo(np.float64).eps
BOXES = [([0, 0, 0], [19, 7, 7]), ([20, 0, 0], [30, 7, 7])]
BOXES_ODD = [([0, 0, 0], [6, 4, 2]), ([7, 0, 0], [70, 0, 0])]  # 105 cells end partway through a wave; 64 x 1 x 1 is exactly one wave


def ncells(boxes):
    return [int(np.prod([h - l + 1 for l, h in zip(lo, hi)])) for lo, hi in boxes]


class Launch:
    def __init__(self, ctx, boxes):
        self.ctx, self.boxes = ctx, boxes
        self.lev = Level(ctx, 3, boxes)
        self.n = ncells(boxes)
        self.N = sum(self.n)
        self.fabs = {}
        self.cnt = torch.zeros(8, dtype=torch.int32, device=ctx.device)

    def fabs_of(self, ng):
        if ng not in self.fabs:
            self.fabs[ng] = (MultiFab(self.lev, 6 + 4 * ng, NGROW), MultiFab(self.lev, ng, 0))
        return self.fabs[ng]

    def call(self, ts, dt_radiation, stage, ng):
        Uf, Qf = self.fabs_of(ng)
        rt, t = M.device_traits(ts)
        it, fail = C.c_void_p(self.cnt.data_ptr()), C.c_void_p(self.cnt[4:].data_ptr())
        return self.ctx.L.qk_rad_AddSourceTermsMultiGroup(self.lev.h, self.ctx.stream(), C.byref(rt), C.byref(t), Uf.ptr, Qf.ptr, C.c_double(dt_radiation),
                                                          int(stage), it, fail)

    def run(self, ts, U, src, dt_radiation, stage):
        """(state of the valid cells [6 + 4 ng, N], counters [7] in the oracle's layout); asserts that every ghost cell still holds NaN"""
        ng, nc = ts.ng, 6 + 4 * ts.ng
        assert U.shape == (nc, self.N) and src.shape == (ng, self.N)
        Uf, Qf = self.fabs_of(ng)
        at = 0
        for b, (lo, hi) in enumerate(self.boxes):
            nx, ny, nz = (hi[d] - lo[d] + 1 for d in range(3))
            fab = np.full(Uf.shapes[b], np.nan)
            fab[:, NGROW:-NGROW, NGROW:-NGROW, NGROW:-NGROW] = U[:, at:at + self.n[b]].reshape(nc, nz, ny, nx)
            Uf.set_fab(b, fab)
            Qf.set_fab(b, src[:, at:at + self.n[b]].reshape(ng, nz, ny, nx))
            at += self.n[b]
        self.cnt.zero_()
        self.ctx.check(self.call(ts, dt_radiation, stage, ng), "qk_rad_AddSourceTermsMultiGroup")
        torch.cuda.synchronize()
        got = np.empty((nc, self.N))
        at = 0
        for b in range(len(self.boxes)):
            out = Uf.fab_numpy(b)
            ghost = np.ones(out.shape[1:], dtype=bool)
            ghost[NGROW:-NGROW, NGROW:-NGROW, NGROW:-NGROW] = False
            assert np.isnan(out[:, ghost]).all(), f"ghost cells of box {b} written"
            got[:, at:at + self.n[b]] = out[:, NGROW:-NGROW, NGROW:-NGROW, NGROW:-NGROW].reshape(nc, self.n[b])
            at += self.n[b]
        return got, [int(v) for v in self.cnt[:7].cpu()]


@pytest.fixture(scope="module")
def launch(ctx):
    return Launch(ctx, BOXES)


@pytest.fixture(scope="module")
def launch_odd(ctx):
    return Launch(ctx, BOXES_ODD)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def assert_same_bits(got, want, what=""):
    """every value the oracle has finite: equal in every bit; where the oracle is not finite, neither is the GPU"""
    fin = np.isfinite(want)
    diff = fin & (bits(got) != bits(want))
    if diff.any():
        c, i = np.argwhere(diff)[0]
        raise AssertionError(f"{what}: {diff.sum()} finite values differ in {diff.any(axis=0).sum()} cells; first: component {c} cell {i} "
                             f"GPU {got[c, i]!r} oracle {want[c, i]!r}")
    assert not np.isfinite(got[~fin]).any(), f"{what}: the GPU is finite where the oracle is not"


class Run:
    """one launch and the oracle's plain and jittered runs on the same cells"""

    def __init__(self, launch, oracle, ts, U, src, dt_radiation, stage, name):
        self.ts, self.U, self.src, self.dt_radiation, self.stage, self.name = ts, U, src, dt_radiation, stage, name
        self.dt = M.stage_dt(dt_radiation, stage)
        ot = M.oracle_traits(ts)
        self.Uo, self.rec, self.tot = oracle.rad_mg_source_cells(ot, U, src, dt_radiation, stage)
        self.jit = [oracle.rad_mg_source_cells(ot, U, src, dt_radiation, stage, seed, M.JITTER_ULPS) for seed in M.JITTER_SEEDS]
        self.got, self.cnt = launch.run(ts, U, src, dt_radiation, stage)
        self.failed = M.failed_cells(self.Uo, self.rec)
        self.ok = ~self.failed
        self.err = M.cell_errors(ts, U, src, self.dt, self.got, self.Uo)
        self.yard = np.max([M.cell_errors(ts, U, src, self.dt, Uj, self.Uo) for Uj, _, _ in self.jit], axis=0)

    def took(self, name):
        return M.took(self.rec, name)

    # ---- the assertions of the issue, by number
    def check_untouched(self):
        """(1) density in every bit; where the oracle returns the input bits of a component (finite), so does the GPU"""
        assert np.array_equal(bits(self.got[0]), bits(self.U[0])), "density modified"
        same = (bits(self.Uo) == bits(self.U)) & np.isfinite(self.Uo) & self.ok[None, :]
        untouched = same.all(axis=1)  # components the scheme leaves alone in every cell
        for c in np.flatnonzero(untouched):
            assert np.array_equal(bits(self.got[c, self.ok]), bits(self.U[c, self.ok])), f"component {c} modified"

    def check_failed_cells_agree(self):
        """cells the plain oracle fails in are left out of the comparison of values; whether a cell ends finite is compared as the values are: the
        number of cells that are finite on one side only, GPU against the plain oracle, is at most twice the largest such number between a
        jittered run and the plain oracle, plus one — and none where no jittered run differs from the plain oracle in this: the patterns are then the
        same; a cell that is non-finite on the GPU fails in the plain or in a jittered run"""
        fin_o, fin_g = np.isfinite(self.Uo).all(axis=0), np.isfinite(self.got).all(axis=0)
        bad_any = self.failed.copy()
        yard = 0
        for Uj, rj, _ in self.jit:
            bad_any |= M.failed_cells(Uj, rj)
            yard = max(yard, int((np.isfinite(Uj).all(axis=0) != fin_o).sum()))
        mism = int((fin_g != fin_o).sum())
        print(f"{self.name}: cells finite on one side only: GPU vs oracle {mism}, jitter vs oracle at most {yard}")
        assert mism <= (2 * yard + 1 if yard else 0)
        assert not (~fin_g & ~bad_any).any(), f"{self.name}: {(~fin_g & ~bad_any).sum()} cells non-finite on the GPU alone"

    def check_hard_cap(self):
        """(2) beta_order 0, no dust: two converged solutions each within K_ROOT r E_tot0 of the root"""
        assert self.ts.beta_order == 0 and not self.ts.dust
        cs = self.ts.c / self.ts.chat
        E0 = M.eint_from_egas(self.U)
        Etot0 = E0 + cs * (self.U[6::4].sum(axis=0) + (self.src * self.dt * self.ts.chat).sum(axis=0))
        e_gas = np.abs(self.got[5] - self.Uo[5]) / Etot0
        e_rad = cs * np.abs(self.got[6::4] - self.Uo[6::4]).sum(axis=0) / Etot0
        cap = 2.0 * M.K_ROOT * M.RESID_TOL
        print(f"{self.name}: hard cap {cap:.3g}: e_gas max {e_gas[self.ok].max():.3g}, e_rad max {e_rad[self.ok].max():.3g}")
        assert (e_gas[self.ok] <= cap).all() and (e_rad[self.ok] <= cap).all()

    def check_distribution(self):
        """(3) the error ladder against the jitter yardstick"""
        err, yard = self.err[self.ok], self.yard[self.ok]
        le, ly = M.ladder(err), M.ladder(yard)
        print(f"{self.name}: {self.ok.sum()} cells; GPU vs oracle   > 1e-15 .. 1e-10: {le} max {err.max():.3g}")
        print(f"{self.name}: {' ' * len(str(self.ok.sum()))}        jitter vs oracle > 1e-15 .. 1e-10: {ly} max {yard.max():.3g}")
        if yard.max() == 0.0:
            assert_same_bits(self.got[:, self.ok], self.Uo[:, self.ok], self.name)
            return
        for t, a, b in zip(M.LADDER, le, ly):
            assert a <= 2 * b + 1, f"{self.name}: {a} cells beyond {t:g} on the GPU, {b} under the jitter"
        assert err.max() <= 3.0 * yard.max(), f"{self.name}: largest error {err.max():.3g}, largest under the jitter {yard.max():.3g}"

    def check_counters(self, exact=False):
        """(4) [solves, Newton iterations, largest Newton count, decoupled, Newton failures, negative dust temperatures, outer failures]"""
        print(f"{self.name}: counters GPU {self.cnt}, oracle {self.tot}, jittered {[t for _, _, t in self.jit]}")
        if exact:
            assert self.cnt == self.tot, (self.cnt, self.tot)
            return
        if self.ts.beta_order == 0:
            assert self.cnt[0] == self.tot[0] == (0 if self.ts.gamma == 1.0 else self.U.shape[1])
        for k in range(7):
            # "within the spread of the jittered runs around the plain oracle, widened by that spread once more"
            spread = max(abs(t[k] - self.tot[k]) for _, _, t in self.jit)
            assert abs(self.cnt[k] - self.tot[k]) <= 2 * spread, f"{self.name}: counter {k}: GPU {self.cnt[k]}, oracle {self.tot[k]}, jitter spread {spread}"

    def check_conservation(self):
        """(5) from the GPU output alone, in extended precision, on the cells that converged"""
        ok = self.ok & np.isfinite(self.got).all(axis=0)
        for Uj, rj, _ in self.jit:  # (converged: in the plain and in every jittered run — the GPU keeps no record per cell)
            ok &= ~M.failed_cells(Uj, rj)
        e, p, exact = M.conservation_defects(self.ts, self.U[:, ok], self.src[:, ok], self.dt_radiation, self.stage, self.got[:, ok])
        print(f"{self.name}: energy defect at most {e:.3g} of the bound, momentum defect at most {p:.3g} of the bound")
        assert e <= 1.0 and p <= 1.0 and exact

    def check_all(self):
        self.check_untouched()
        self.check_failed_cells_agree()
        if self.ts.beta_order == 0 and not self.ts.dust and self.ts.gamma != 1.0:
            self.check_hard_cap()
        self.check_distribution()
        self.check_counters()
        if not self.ts.dust and self.ts.gamma != 1.0:  # (the dust model's heating and cooling terms are no part of this balance; gamma == 1: no exchange)
            self.check_conservation()


def case_run(launch, oracle, case):
    ts = case.traits()
    U, src = M.generate_cells(ts, case.unit, case.dt, case.stage, launch.N, case.seed, case.source)
    return Run(launch, oracle, ts, U, src, case.dt, case.stage, case.id)


# ------------------------------------------------------------------------------------------------ branch sweep, NG = 4
@pytest.fixture(scope="module", params=M.branch_cases(), ids=lambda c: c.id)
def branch(request, launch, oracle):
    return request.param, case_run(launch, oracle, request.param)


def test_branch_sweep_stays_within_the_jitter_yardstick(branch):
    """NG = 4: the three opacity models x beta_order 0 / 1 x both stages x five lower-value sets (constant, / rho, rho^0.5, T^-2, T^+1.5), the group
    exponents 0 / -2 / mixed cycling: assertions (1) to (5)"""
    case, R = branch
    R.check_all()
    assert R.failed.mean() <= (0.02 if case.source else 0.0)
    assert R.rec["newton_max"].max() >= 3 and R.took("x_ge_100").any() and R.took("below_table").any()


def test_branch_sweep_fluxes_and_momenta_are_exact_where_no_libm_enters(branch):
    """(1) piecewise_constant, beta_order 0, lower values independent of T: kappaF = lower, the flux update is a product and a quotient"""
    case, R = branch
    if not (case.model == M.PIECEWISE_CONSTANT and case.beta_order == 0 and R.ts.T_exp == 0.0 and R.ts.rho_exp in (0.0, -1.0)):
        return
    comps = [1, 2, 3] + [c for g in range(R.ts.ng) for c in (7 + 4 * g, 8 + 4 * g, 9 + 4 * g)]
    assert_same_bits(R.got[comps][:, R.ok], R.Uo[comps][:, R.ok], case.id)


# ------------------------------------------------------------------------------------------------ NG sweep: every instantiation
@pytest.fixture(scope="module", params=M.ng_cases(), ids=lambda c: c.id)
def ng_case(request, launch, oracle):
    return request.param, case_run(launch, oracle, request.param)


def test_every_group_count_stays_within_the_jitter_yardstick(ng_case):
    """NG = 2, 3, 5, 6, 8 with every opacity model at beta_order 1, stage 2; NG = 8 (9 edges over six decades) also at beta_order 0, stage 1"""
    case, R = ng_case
    R.check_all()
    assert R.failed.mean() <= (0.02 if case.source else 0.0)


@pytest.mark.parametrize("model", [1, 2, 3])
def test_odd_boxes_end_partway_through_a_wave(launch_odd, oracle, model):
    """7 x 5 x 3 (105 cells: the last wave of the box is partly valid) and 64 x 1 x 1 (exactly one wave)"""
    case = M.Case(4, model, 1, 2, source=False, unit="cgs", eddington=0, kexp="kmix", lower="const", seed=7000 + model)
    R = case_run(launch_odd, oracle, case)
    R.check_all()
    assert R.tot[0] >= launch_odd.N


def test_counter_slots_shared_by_two_waves_keep_the_largest_newton_count(ctx, oracle):
    """the counters go through wave % NSLOT slots (NSLOT = 1024): a level of 52 boxes — 20 x 8 x 8, fifty single cells, 11 x 8 x 8 — launches 52 x 20
    waves, so that waves 4 .. 10 of the last box share their slots with waves 0 .. 6 of the first.  Sums add, the largest Newton count is a maximum."""
    boxes = [BOXES[0]] + [([100 + 2 * i, 0, 0], [100 + 2 * i, 0, 0]) for i in range(50)] + [BOXES[1]]
    L = Launch(ctx, boxes)
    assert (len(boxes) - 1) * 5 * 4 + 4 == 1024  # wave 4 of the last box is wave 1024 of the launch: slot 0
    case = M.Case(4, 1, 0, 1, source=False, unit="cgs", eddington=0, kexp="k-2", lower="const", seed=7100)
    R = case_run(L, oracle, case)
    R.check_distribution()
    R.check_counters()
    first, last = R.rec["newton_max"][:1280].reshape(20, 64).max(axis=1), R.rec["newton_max"][-704:].reshape(11, 64).max(axis=1)
    assert (first[:7] + last[4:] > R.tot[2]).all(), "the counts of two waves that share a slot add up to more than the largest count"
    assert R.cnt[0] == R.tot[0] == L.N and R.tot[4] == 0


# ------------------------------------------------------------------------------------------------ targeted branches
def targeted(launch, oracle, name):
    """the case `name` of rad_mg_source_reference.TARGETED; that its cells take the branch, per the oracle's mask, is asserted here and, with the
    failing shares, in tests/test_rad_mg_source_reference.py"""
    t = M.TARGETED[name]
    U, src = t.cells(launch.N)
    R = Run(launch, oracle, t.ts, U, src, t.dt, t.stage, name)
    M.check_targeted(t, R.Uo, R.rec, R.tot)
    return R


@pytest.mark.parametrize("model", [1, 2, 3])
def test_a_group_without_opacity_keeps_its_energy(launch, oracle, model):
    """mg_kappa_lower = 0 at the lower edge of one interior group: tau_g = 0, Jgg = -inf, the guess is kept"""
    R = targeted(launch, oracle, f"zero-tau-{M.MODEL_NAME[model]}")
    R.check_all()
    if model == 1:
        assert np.array_equal(bits(R.got[6 + 4, R.ok]), bits(R.U[6 + 4, R.ok])), "the energy of the group without opacity changed"
        assert np.array_equal(bits(R.got[7 + 4:10 + 4, R.ok]), bits(R.U[7 + 4:10 + 4, R.ok])), "the flux of the group without opacity changed"


@pytest.mark.parametrize("model", [1, 3])
def test_energy_step_constraint(launch, oracle, model):
    """enable_dE_constrain: radiation 30 to 100 times hotter than the gas at large optical depth — the Newton step in temperature exceeds
    max(T_gas, T_rad) and the gas is put at the radiation temperature instead"""
    targeted(launch, oracle, f"dE-constraint-{M.MODEL_NAME[model]}").check_all()


@pytest.mark.parametrize("model", [2, 3])
def test_flux_mean_with_a_vanishing_denominator(launch, oracle, model):
    """ComputeDiffusionFluxMeanOpacity, denom <= 0: cold gas, the last group wholly beyond x = 100 (no thermal energy, no Planck function at either
    edge): kappaF = 0 there"""
    targeted(launch, oracle, f"denom-{M.MODEL_NAME[model]}").check_all()


@pytest.mark.parametrize("slope", [150, -150])
def test_group_mean_opacity_of_a_steep_spectrum(launch, oracle, slope):
    """ComputeGroupMeanOpacity in the full-spectrum model, alpha > 100 and alpha < -100: the group energies a power law of index +-150 across four
    narrow groups (edges 0.5 .. 2 k_B T1)"""
    targeted(launch, oracle, f"steep-{slope:+d}").check_all()


@pytest.mark.parametrize("model", [2, 3])
def test_group_mean_opacity_takes_both_logarithms(launch, oracle, model):
    """|alpha| < 1e-8 in both parts: alpha_quant = -1 (the fixed-slope model, and the edge groups of the full-spectrum model) with group exponents 0"""
    targeted(launch, oracle, f"log-log-{M.MODEL_NAME[model]}").check_all()


@pytest.mark.parametrize("name", [n for n in M.TARGETED if n.startswith("slope_")])
def test_spectral_slopes_of_empty_and_negative_groups(launch, oracle, name):
    """ComputeRadQuantityExponents: exactly zero energy in two neighbouring groups (slope 0) and one negative group (slope +-max).
    In the cold cells of the zero-energy cases (117 of 1984) an emptied group has no thermal energy either (x >= 100), still holds exactly 0 after
    the solve, and UpdateFlux forms the reduced flux F / (c * 0).  The reference's clamp(f, 0., 1.) keeps the NaN of 0 / 0 and the cell ends NaN in
    momentum, gas energy and that group's flux; with chi = 1/3 there is no clamp and the cell stays finite unless the group has a flux in all
    three components (f = inf, inf / inf in the unit vector; a component without flux is 0 / 0, f is NaN, fails `f > 0` and n = 0).  The kernel's
    v_max / v_min clamp dropped the NaN and returned finite values in those 117 cells until radSourceCellMG restored it (qk_rad_mg_device.hpp):
    whether a cell ends finite is part of what is compared here, and no jittered run moves it, so the GPU's non-finite cells are the oracle's."""
    targeted(launch, oracle, name).check_all()


def test_slopes_freeze_after_five_newton_iterations(launch, oracle):
    """full-spectrum model: from the sixth Newton iteration on the slopes of the fifth are kept"""
    targeted(launch, oracle, "slopes-frozen").check_all()


def test_thermal_emission_on_the_energy_floor(launch, oracle):
    """ComputeThermalRadiationMultiGroup: cold gas, the last group far in the Wien tail: its thermal energy is raised to Erad_floor / nGroups"""
    targeted(launch, oracle, "floor").check_all()


@pytest.mark.parametrize("branch_name", ["x_ge_100", "below_table"])
@pytest.mark.parametrize("model", [1, 2])
def test_every_edge_outside_the_planck_table(launch, oracle, model, branch_name):
    """all group edges at x >= 100 (all thermal energy in the last group) and all below the table's first entry (the series)"""
    targeted(launch, oracle, f"{branch_name}-{M.MODEL_NAME[model]}").check_all()


# ------------------------------------------------------------------------------------------------ isothermal
@pytest.mark.parametrize("model", [1, 2, 3])
def test_isothermal_gas_exchanges_momentum_only(launch, oracle, model):
    """gamma == 1: no solve; only the fluxes and the gas momentum move.  piecewise_constant: every bit; the power-law models take one pow per group"""
    R = targeted(launch, oracle, f"isothermal-{M.MODEL_NAME[model]}")
    assert np.isfinite(R.Uo).all() and R.tot[0] == 0
    R.check_counters(exact=True)
    for c in [0, 4, 5] + [6 + 4 * g for g in range(4)]:
        assert np.array_equal(bits(R.got[c]), bits(R.U[c])), c
    if model == 1:
        assert_same_bits(R.got, R.Uo, R.name)
    R.check_distribution()
    flux = [c for g in range(4) for c in (7 + 4 * g, 8 + 4 * g, 9 + 4 * g)]
    moved = np.abs(R.U[flux]).sum(axis=0) > 0
    assert moved.any() and (R.got[flux][:, moved] != R.U[flux][:, moved]).any(axis=0).all() and np.array_equal(R.got[flux][:, ~moved], R.U[flux][:, ~moved])
    assert (R.got[1:4] != R.U[1:4]).any(axis=0).mean() > 0.5


# ------------------------------------------------------------------------------------------------ failure paths
def test_failure_counters_carry_what_the_oracle_counts(launch, oracle):
    """60 cells with NaN gas energy, and then also 60 radiation-dominated cells (X = 1e12) the reference gives up on, spliced into an ordinary list,
    spread over the waves and both boxes (rad_mg_source_reference.failure_cells).  With several groups a NaN cell counts 1 solve of 101
    iterations, 1 Newton failure and no outer failure (tests/test_rad_mg_source_reference.py: the lagged-work test
    `sum(abs(work - work_prev)) > ref_work` is false for NaN, so the first pass is accepted); the outer failures come from the X = 1e12 cells.
    Both kinds fail by construction — the same record in the plain oracle and under every jitter seed, and no jitter seed moves a counter of
    either list (asserted) — so every counter equals the oracle's.  The ordinary cells do not see their neighbours."""
    ts, U_plain, U_nan, U_both, src = M.failure_cells(oracle)
    case = M.FAILURE_CASE
    ordinary = np.ones(launch.N, dtype=bool)
    ordinary[M.NAN_AT] = ordinary[M.GIVEN_UP_AT] = False
    assert np.unique(np.concatenate([M.NAN_AT, M.GIVEN_UP_AT])).size == 120 and (M.NAN_AT >= 1280).sum() >= 10 and (M.GIVEN_UP_AT >= 1280).sum() >= 10
    plain, cnt_plain = launch.run(ts, U_plain, src, case.dt, case.stage)
    assert cnt_plain[4] == 0 and cnt_plain[6] == 0

    R = Run(launch, oracle, ts, U_nan, src, case.dt, case.stage, "failure-list-nan")
    assert (R.failed == ~np.isfinite(U_nan[4])).all() and all(t == R.tot for _, _, t in R.jit)
    assert R.cnt[4] == 60 and R.cnt[6] == 0 and R.cnt[2] == M.MAX_NEWTON + 1
    R.check_counters(exact=True)
    R.check_failed_cells_agree()
    assert not np.isfinite(R.got[4:6, M.NAN_AT]).any()
    assert np.array_equal(bits(R.got[:, ~R.failed]), bits(plain[:, ~R.failed]))

    R = Run(launch, oracle, ts, U_both, src, case.dt, case.stage, "failure-list")
    assert (R.failed == ~ordinary).all() and all(t == R.tot for _, _, t in R.jit)
    assert R.rec["fail_outer"][M.GIVEN_UP_AT].sum() >= 10 and R.tot[6] == R.rec["fail_outer"][M.GIVEN_UP_AT].sum()
    R.check_counters(exact=True)
    R.check_failed_cells_agree()
    assert not np.isfinite(R.got[4:6, M.NAN_AT]).any()
    assert np.array_equal(bits(R.got[:, ordinary]), bits(plain[:, ordinary]))


# ------------------------------------------------------------------------------------------------ the dust instantiation
@pytest.mark.parametrize("ng,variant", M.DUST_CASES)
def test_dust_launch_straddles_the_coupling_threshold(launch, oracle, ng, variant):
    """k_rad_source_mg<NG, true>: one launch whose cells lie on both sides of gas_dust_coupling_threshold — coupled and decoupled solves in the same
    wave — and in part of whose coupled cells the dust temperature goes negative (fail_dust != 0; those cells count as failed and are left out of the
    comparison of values).  With photoelectric heating: the last column of the Jacobian in the coupled solve, the scalar gas-energy solve in the
    decoupled one.  Line cooling, cosmic-ray heating and the linearised emission each once.  Inputs: see rad_mg_source_reference.DUST_COEFF."""
    targeted(launch, oracle, f"dust-ng{ng}-{variant}").check_all()


# ------------------------------------------------------------------------------------------------ refusals (no launch)
def test_refusals(launch, ctx):
    ts = M.make_traits("cgs", 4, 1, beta_order=1)
    QK_ERR_INVALID, QK_ERR_UNSUPPORTED = -1, -3

    def refused(ts_bad, rc_want, words, ng=4):
        rc = launch.call(ts_bad, 1.0, 1, ng)
        msg = ctx.L.qk_last_error(ctx.h).decode()
        assert rc == rc_want and words in msg, (rc, msg)

    seven = M.replace(ts, bnd=tuple(10.0 ** (g - 3) for g in range(8)), kexp=(0.0,) * 8, klow=(1.0,) * 8)
    refused(seven, QK_ERR_UNSUPPORTED, "ngroups must be one of 2, 3, 4, 5, 6, 8")
    refused(M.replace(ts, beta_order=2), QK_ERR_UNSUPPORTED, "beta_order must be 0 or 1")
    refused(M.replace(ts, cr_heating=1.0), QK_ERR_UNSUPPORTED, "together with the dust model only")
    refused(M.replace(ts, cooling=(0.0, 1.0, 0.0, 0.0)), QK_ERR_UNSUPPORTED, "together with the dust model only")
    refused(M.replace(ts, pe=1), QK_ERR_UNSUPPORTED, "together with the dust model only")
    refused(M.replace(ts, T_exp=1.5, T_ref=0.0), QK_ERR_INVALID, "mg_kappa_T_ref must be positive")
