"""Helpers of the cell-by-cell tests of the MULTIGROUP matter-radiation exchange (AddSourceTermsMultiGroup): trait sets, a seeded cell generator,
the per-cell error measure and an independent 50-digit solution of the implicit system.  Nothing here needs a GPU; mpmath is imported by
exact_exchange_mg alone (the GPU tests do not call it); the two *_traits functions import the ctypes bindings when called.

Constants of the reference's scheme, quoted from its headers (src/radiation/radiation_system.hpp:52, src/radiation/source_terms_multi_group.hpp:230-231,
:677, :762-763) and NOT read from the kernel under test."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from rad_source_reference import A_CGS, C_CGS, GAMMA, IMEX_A32, K_B, M_U, _directions, stage_dt  # noqa: F401  (the same unit systems and stage rule)

RESID_TOL = 1.0e-11    # source_terms_multi_group.hpp:230
MAX_NEWTON = 100       # :231, `for (; n < maxIter; ++n)`: a solve that never converges is counted as n + 1 = 101
MAX_OUTER = 5          # :677
REL_LAG_TOL = 1.0e-8   # :762
LAG_TOL = 1.0e-13      # :763
MAX_ITER_ALPHA = 5     # radiation_system.hpp:41 max_iter_to_update_alpha_E

PIECEWISE_CONSTANT, PPL_FIXED_SLOPE, PPL_FULL_SPECTRUM = 1, 2, 3
MODEL_NAME = {1: "pc", 2: "fixed", 3: "full"}

# The amplitude of the libm jitter of the oracle (orc_set_libm_jitter): the sum of the two libraries' error bounds for pow, exp, log and log10 in
# double precision, 1 ulp each as far as memory of ROCm's math-API accuracy table and of the glibc manual's "Errors in Math Functions" goes —
# the figure is NOT read from them.
JITTER_ULPS = 2
JITTER_SEEDS = (11, 12, 13)

# largest measured distance of the CPU oracle from the exact root, in units of RESID_TOL E_tot0 (tests/test_rad_mg_source_reference.py), times 1.5
K_ROOT_MEASURED = {"piecewise_constant": (0.326, 0.999), "PPL_fixed_slope": (0.991, 0.994)}  # (gas energy, radiation energy), 2e4 cells per model
K_ROOT = 1.5 * max(max(v) for v in K_ROOT_MEASURED.values())


@dataclass(frozen=True)
class MGTraits:
    """the fields of qk_rad_traits / qk_hydro_traits the multigroup exchange reads"""
    c: float
    chat: float
    arad: float
    kB: float
    mmw: float
    bnd: tuple
    energy_unit: float
    model: int
    kexp: tuple
    klow: tuple
    rho_exp: float = 0.0
    T_ref: float = 0.0
    T_exp: float = 0.0
    gamma: float = GAMMA
    beta_order: int = 1
    eddington_model: int = 0
    pow_mode: int = 1
    Erad_floor: float = 0.0
    dust: int = 0
    dust_coeff: float = 2.5e-34
    dust_threshold: float = 1.0e-6
    thermal_model: int = 0
    cooling: tuple = ()
    cr_heating: float = 0.0
    pe: int = 0
    pe_derivative: float = 0.0

    @property
    def ng(self) -> int:
        return len(self.bnd) - 1

    @property
    def cvp(self) -> float:
        return self.kB / (self.mmw * (GAMMA - 1.0))


def oracle_traits(ts: MGTraits):
    from oracle.pyoracle import RadMGCellTraits
    t = RadMGCellTraits()
    t.c_light, t.c_hat, t.radiation_constant, t.Erad_floor, t.energy_unit = ts.c, ts.chat, ts.arad, ts.Erad_floor, ts.energy_unit
    for g in range(ts.ng + 1):
        t.rad_boundaries[g], t.mg_kappa_exponent[g], t.mg_kappa_lower[g] = ts.bnd[g], ts.kexp[g], ts.klow[g]
    t.mg_kappa_rho_exponent, t.mg_kappa_T_ref, t.mg_kappa_T_exponent = ts.rho_exp, ts.T_ref, ts.T_exp
    t.dust_gas_interaction_coeff, t.gas_dust_coupling_threshold = ts.dust_coeff, ts.dust_threshold
    for g, v in enumerate(ts.cooling):
        t.cooling_linear_coeff[g] = v
    t.cr_heating_rate, t.pe_heating_E1_derivative = ts.cr_heating, ts.pe_derivative
    t.gamma, t.mean_molecular_weight, t.boltzmann_constant = ts.gamma, ts.mmw, ts.kB
    t.beta_order, t.eddington_model, t.pow_mode, t.ngroups, t.mg_opacity_model = ts.beta_order, ts.eddington_model, ts.pow_mode, ts.ng, ts.model
    t.enable_dust_gas_thermal_coupling_model, t.thermal_model, t.enable_photoelectric_heating = ts.dust, ts.thermal_model, ts.pe
    return t


def device_traits(ts: MGTraits):
    from quokka_amd import capi
    rt = capi.RadTraits(ts.c, ts.chat, ts.arad, ts.Erad_floor, ts.beta_order, 0, 0.0, 0.0, 0.0, ts.pow_mode, ts.eddington_model)
    rt.set_groups(list(ts.bnd), ts.energy_unit, ts.model, list(ts.kexp), list(ts.klow), rho_exponent=ts.rho_exp, T_ref=ts.T_ref, T_exponent=ts.T_exp)
    rt.enable_dust_gas_thermal_coupling_model, rt.dust_gas_interaction_coeff = ts.dust, ts.dust_coeff
    rt.thermal_model, rt.gas_dust_coupling_threshold = ts.thermal_model, ts.dust_threshold
    for g, v in enumerate(ts.cooling):
        rt.cooling_linear_coeff[g] = v
    rt.cr_heating_rate, rt.enable_photoelectric_heating, rt.pe_heating_E1_derivative = ts.cr_heating, ts.pe, ts.pe_derivative
    return rt, capi.traits(ts.gamma, False, 3, mean_molecular_weight=ts.mmw, boltzmann_constant=ts.kB)


# ------------------------------------------------------------------------------------------------ unit systems and group structures
# (c, c_hat, a, k_B, mu, dt_radiation, nominal opacity): the two systems of rad_source_reference.units() with its time steps and its nominal opacities
UNITS = {"cgs": (C_CGS, 0.1 * C_CGS, A_CGS, K_B, M_U, 1.0e3, 1.0), "dimensionless": (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0e30)}
# group edges in units of k_B T1 (T1: the gas temperature at tau = X = 1): with k_B T over 10^-2.7 .. 10^2.7 around it the edges' x = h nu / k_B T run
# from 2e-6 (below the table's first entry, 1e-3) to 5e5 (above 100) in every case
EDGES = {2: (1e-3, 1.0, 1e3), 3: (1e-3, 0.3, 3.0, 1e3), 4: (1e-3, 0.1, 1.0, 10.0, 1e3), 5: (1e-3, 0.1, 0.5, 2.0, 10.0, 1e3),
         6: (1e-3, 0.03, 0.3, 1.0, 3.0, 30.0, 1e3), 8: tuple(10.0 ** (-3.0 + 0.75 * g) for g in range(9))}  # NG = 8: 9 edges over six decades


def reference_point(unit: str):
    """(rho1, T1): the density and gas temperature at which tau = dt rho k_nom c_hat = 1 (stage 1) and X = (c / c_hat) a T^4 / E_int = 1"""
    c, chat, arad, kB, mmw, dt, k_nom = UNITS[unit]
    rho1 = 1.0 / (dt * k_nom * chat)
    T1 = float(np.cbrt(rho1 * (kB / (mmw * (GAMMA - 1.0))) / ((c / chat) * arad)))
    return rho1, T1


def group_exponents(name: str, ng: int) -> tuple:
    """mg_kappa_exponent per edge: all 0, all -2, or mixed"""
    if name == "k0":
        return (0.0,) * (ng + 1)
    if name == "k-2":
        return (-2.0,) * (ng + 1)
    assert name == "kmix"
    return tuple((0.0, -2.0, 1.0, -1.0, 0.5, -0.5, -2.0, 0.0, 1.0)[g] for g in range(ng + 1))


def lower_values(bnd, kexp) -> np.ndarray:
    """lower values continuous across the edges, klow[g + 1] = klow[g] (nu[g + 1] / nu[g])^kexp[g], scaled so that the largest is 1"""
    k = [1.0]
    for g in range(len(bnd) - 1):
        k.append(k[-1] * (bnd[g + 1] / bnd[g]) ** kexp[g])
    k = np.array(k)
    return k / k[:-1].max()


# name -> (mg_kappa_rho_exponent, mg_kappa_T_exponent); the lower values are scaled so that every set has the nominal opacity at (rho1, T1)
LOWER_SETS = {"const": (0.0, 0.0), "per_rho": (-1.0, 0.0), "rho0.5": (0.5, 0.0), "T-2": (0.0, -2.0), "T+1.5": (0.0, 1.5)}


def make_traits(unit: str, ng: int, model: int, kexp_name: str = "k0", lower: str = "const", zero_group=None, **kw) -> MGTraits:
    c, chat, arad, kB, mmw, dt, k_nom = UNITS[unit]
    rho1, T1 = reference_point(unit)
    bnd = EDGES[ng]
    kexp = group_exponents(kexp_name, ng)
    a, b = LOWER_SETS[lower]
    klow = lower_values(bnd, kexp) * k_nom / rho1 ** a
    if zero_group is not None:
        klow[zero_group] = 0.0
    return MGTraits(c, chat, arad, kB, mmw, tuple(float(v) for v in bnd), kB * T1, model, kexp, tuple(float(v) for v in klow), rho_exp=a,
                    T_ref=(T1 if b != 0.0 else 0.0), T_exp=b, **kw)


@dataclass(frozen=True)
class Case:
    ng: int
    model: int
    beta_order: int
    stage: int
    source: bool
    unit: str
    eddington: int
    kexp: str
    lower: str
    seed: int

    @property
    def id(self) -> str:
        return (f"ng{self.ng}-{MODEL_NAME[self.model]}-b{self.beta_order}-s{self.stage}-{self.kexp}-{self.lower}-{'src' if self.source else 'nosrc'}-"
                f"{self.unit[:3]}-edd{self.eddington}")

    @property
    def dt(self) -> float:
        return UNITS[self.unit][5]

    def traits(self) -> MGTraits:
        return make_traits(self.unit, self.ng, self.model, self.kexp, self.lower, beta_order=self.beta_order, eddington_model=self.eddington)


def branch_cases() -> list:
    """NG = 4: every (opacity model, beta_order, stage, lower-value set); the group exponents cycle; source, unit system and closure alternate so that
    each value of each meets every model, every beta_order and both stages"""
    out = []
    for im, model in enumerate((1, 2, 3)):
        for beta in (0, 1):
            for stage in (1, 2):
                for il, lower in enumerate(LOWER_SETS):
                    k = im + beta + stage + il
                    kexp = ("k0", "k-2", "kmix")[(il + im + stage) % 3]
                    out.append(Case(4, model, beta, stage, source=bool((k + il // 2) % 2), unit=("cgs", "dimensionless")[(k // 2 + beta) % 2],
                                    eddington=(il + stage + im) % 2, kexp=kexp, lower=lower, seed=5000 + len(out)))
    return out


def ng_cases() -> list:
    """each of NG = 2, 3, 5, 6, 8 with every opacity model at beta_order 1, stage 2; NG = 8 also at beta_order 0, stage 1"""
    out = []
    for ing, ng in enumerate((2, 3, 5, 6, 8)):
        for model in (1, 2, 3):
            k = ing + model
            out.append(Case(ng, model, 1, 2, source=bool(k % 2), unit=("cgs", "dimensionless")[(k // 2) % 2], eddington=k % 2,
                            kexp=("k0", "k-2", "kmix")[k % 3], lower=("const", "per_rho")[ing % 2], seed=6000 + len(out)))
    for model in (1, 2, 3):
        out.append(Case(8, model, 0, 1, source=bool(model % 2), unit=("dimensionless", "cgs")[model % 2], eddington=0, kexp=("k-2", "kmix", "k0")[model - 1],
                        lower="const", seed=6100 + model))
    return out


# ------------------------------------------------------------------------------------------------ cell generator
def planck_share(x_edges: np.ndarray) -> np.ndarray:
    """(generator only) the share of a T^4 between consecutive x = h nu / k_B T: the series 1 - 15 / pi^4 sum_n e^(-n x) (x^3 / n + 3 x^2 / n^2 +
    6 x / n^3 + 6 / n^4), x^3 / 3 below 1e-2; first and last group take what lies outside the edges"""
    x = np.asarray(x_edges, dtype=np.float64)
    n = np.arange(1.0, 400.0)[:, None, None]
    xx = np.minimum(x, 700.0)[None]
    s = (np.exp(-n * xx) * (xx ** 3 / n + 3 * xx ** 2 / n ** 2 + 6 * xx / n ** 3 + 6 / n ** 4)).sum(axis=0)
    P = np.where(x < 1e-2, (15.0 / np.pi ** 4) * x ** 3 / 3.0, 1.0 - (15.0 / np.pi ** 4) * s)
    P[0], P[-1] = 0.0, 1.0
    return np.clip(np.diff(P, axis=0), 0.0, 1.0)


# src_g dt c_hat / E_g of the cells with an energy source, and the floor under a group's share of a T_r^4.  NARROWED on the CPU oracle until the caps of
# tests/test_rad_mg_source_reference.py hold (the measured failing shares stand in that file's docstrings).
LOG10_SRC = (-3.0, 1.0)
SHARE_FLOOR = 1.0e-8
LOG10_TAU = (-6.0, 6.0)
LOG10_X = (-3.0, 3.0)
LOG10_X_T_DEPENDENT = (-2.0, 2.0)
LOG10_X_PER_RHO = (-3.0, 1.5)
LOG10_TR = (float(np.log10(0.3)), float(np.log10(3.0)))
LOG10_TR_OPACITY_FALLING_WITH_T = (float(np.log10(0.3)), 0.0)


def sample_ranges(ts: "MGTraits"):
    """(log10 X range, log10 T_r / T range) of the branch sweep for a trait set.  What was narrowed, on the CPU oracle with the source off (2e4 cells
    per case, the full ranges [1e-3, 1e3] and [0.3, 3]):
      * lower values k / rho (tau the same in every cell): the Newton iteration ends at 100 or in NaN in 0.005 - 0.025 % of the cells, all of them
        with X > 10^1.8 and T_r within 20 % of T — radiation-dominated cells at equilibrium, where the 1e-11 residual test is at the rounding of the
        sum.  X stops at 10^1.5.
      * lower values falling with T (T^-2): 0.4 - 0.85 % fail, all of them with T_r > 3 T (the gas heats, the opacity drops under the iteration:
        the single-group power law of rad_source_reference.py shows the same).  T_r stays at or below T, and X inside [1e-2, 1e2] for both
        temperature exponents."""
    if ts.T_exp != 0.0:
        return LOG10_X_T_DEPENDENT, (LOG10_TR_OPACITY_FALLING_WITH_T if ts.T_exp < 0.0 else LOG10_TR)
    if ts.rho_exp == -1.0:
        return LOG10_X_PER_RHO, LOG10_TR
    return LOG10_X, LOG10_TR


def generate_cells(ts: MGTraits, unit: str, dt_radiation: float, stage: int, n: int, seed: int, source: bool, log10_X=None, log10_src=None,
                   log10_Tr=None, share_floor=SHARE_FLOOR, log10_tau=LOG10_TAU):
    """(U[6 + 4 ng, n], src[ng, n]).  Sampled per cell: log10 tau uniform in [-6, 6] for the group of largest opacity (tau = dt rho kappa c_hat at the
    nominal opacity; sets whose lower values depend on rho or T have that optical depth at (rho1, T1) and spread further); X = (c / c_hat) a T^4 /
    E_int log-uniform in [1e-3, 1e3] (narrower for some sets: sample_ranges); tau fixes rho, X then T, so that k_B T runs over five decades
    around the energy unit; E_g = the Planck share of group g at a radiation temperature of 0.3 .. 3 T (sample_ranges; the share not below SHARE_FLOOR) times a T_r^4 times a
    log-uniform factor in [0.1, 10] per group; reduced flux 0 / 0.999999 / uniform below, per group, in random directions; gas at rest in one cell of
    ten, beta log-uniform in [1e-6, 1e-2] otherwise; the energy source off, or src_g dt c_hat / E_g log-uniform (LOG10_SRC) in half of the cells."""
    r = np.random.default_rng(seed)
    ng = ts.ng
    dt = stage_dt(dt_radiation, stage)
    cs = ts.c / ts.chat
    k_nom = UNITS[unit][6]
    tau = 10.0 ** r.uniform(log10_tau[0], log10_tau[1], n)
    lo_X, hi_X = log10_X if log10_X is not None else sample_ranges(ts)[0]
    log10_Tr = log10_Tr if log10_Tr is not None else sample_ranges(ts)[1]
    X = 10.0 ** r.uniform(lo_X, hi_X, n)
    rho = tau / (dt * k_nom * ts.chat)
    T = np.cbrt(X * rho * ts.cvp / (cs * ts.arad))
    Eint = rho * ts.cvp * T
    Tr = T * 10.0 ** r.uniform(log10_Tr[0], log10_Tr[1], n)
    x_edges = (ts.energy_unit * np.array(ts.bnd))[:, None] / (ts.kB * Tr)[None, :]
    share = np.maximum(planck_share(x_edges), share_floor)
    Eg = share * (ts.arad * Tr ** 4)[None, :] * 10.0 ** r.uniform(-1.0, 1.0, (ng, n))
    beta = np.where(r.random(n) < 0.1, 0.0, 10.0 ** r.uniform(-6.0, -2.0, n))
    mom = _directions(r, n) * (beta * ts.c * rho)
    U = np.zeros((6 + 4 * ng, n))
    U[0], U[1:4], U[5] = rho, mom + 0.0, Eint
    U[4] = Eint + (mom * mom).sum(axis=0) / (2.0 * rho)
    src = np.zeros((ng, n))
    on = (r.random(n) < 0.5) & bool(source)
    lo_s, hi_s = log10_src if log10_src is not None else LOG10_SRC
    for g in range(ng):
        u = r.random(n)
        f = np.where(u < 0.1, 0.0, np.where(u < 0.2, 0.999999, r.uniform(0.0, 0.999999, n)))
        U[6 + 4 * g] = Eg[g]
        U[7 + 4 * g:10 + 4 * g] = _directions(r, n) * (f * ts.c * Eg[g]) + 0.0
        src[g] = np.where(on, 10.0 ** r.uniform(lo_s, hi_s, n) * Eg[g] / (dt * ts.chat), 0.0)
    return U, src


def eint_from_egas(U: np.ndarray) -> np.ndarray:
    """ComputeEintFromEgas in the same double-precision operations: what the scheme takes as the initial gas energy"""
    return U[4] - (U[1] * U[1] + U[2] * U[2] + U[3] * U[3]) / (2.0 * U[0])


def failed_cells(Uo: np.ndarray, rec: dict) -> np.ndarray:
    """cells in which the oracle reports a failure or returns a non-finite value"""
    return (rec["fail_newton"] > 0) | (rec["fail_outer"] > 0) | (rec["fail_dust"] > 0) | ~np.isfinite(Uo).all(axis=0)


def took(rec: dict, name: str) -> np.ndarray:
    from oracle.pyoracle import MG_BRANCH_BIT
    return (rec["mask"] & MG_BRANCH_BIT[name]) != 0


# ------------------------------------------------------------------------------------------------ the error measure
def cell_errors(ts: MGTraits, U0: np.ndarray, src: np.ndarray, dt: float, A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """the distance of two results A and B of the same cells on the scheme's own scale, per cell: the largest of
        e_gas = |dE_int| / E_tot0,   e_rad = (c / c_hat) sum_g |dE_g| / E_tot0,   e_F = |dF_g| / (c E_g + |F_g0|) per group and component,
        e_p = |dp| / (|p0| + sum_g (c E_g + |F_g0|) / (c c_hat)) per component
    with E_tot0 = E_int0 + (c / c_hat) sum_g (E_g0 + Src_g), the scheme's own normaliser, and E_g of B (the reference side).  A cell in which one
    side is finite and the other is not counts as inf; both non-finite in the same component: that component is left out.  (gamma == 1: E_tot0 is
    taken with the stored internal energy.)"""
    ng = ts.ng
    cs, cc = ts.c / ts.chat, ts.c * ts.chat
    E0 = eint_from_egas(U0)
    Src = src * dt * ts.chat
    Etot0 = np.abs(E0) + cs * (np.abs(U0[6::4]).sum(axis=0) + Src.sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        def d(a, b, scale):
            both_bad = ~np.isfinite(a) & ~np.isfinite(b)
            e = np.abs(a - b) / scale
            e = np.where(np.isfinite(a) != np.isfinite(b), np.inf, e)
            return np.where(both_bad | ((a == b) & np.isfinite(a)), 0.0, e)
        err = np.maximum(d(A[5], B[5], Etot0), cs * sum(d(A[6 + 4 * g], B[6 + 4 * g], 1.0) for g in range(ng)) / Etot0)
        fscale = [ts.c * np.abs(B[6 + 4 * g]) + np.sqrt((U0[7 + 4 * g:10 + 4 * g] ** 2).sum(axis=0)) for g in range(ng)]
        pscale = sum(fscale) / cc
        for k in range(3):
            for g in range(ng):
                err = np.maximum(err, d(A[7 + 4 * g + k], B[7 + 4 * g + k], np.where(fscale[g] > 0, fscale[g], 1.0)))
            s = np.abs(U0[1 + k]) + pscale
            err = np.maximum(err, d(A[1 + k], B[1 + k], np.where(s > 0, s, 1.0)))
    return np.where(np.isnan(err), np.inf, err)


def conservation_defects(ts: MGTraits, U: np.ndarray, src: np.ndarray, dt_radiation: float, stage: int, out: np.ndarray):
    """from one result alone, in extended precision so that only the scheme's own roundings count: (largest energy defect, largest momentum defect,
    both in units of their bounds; whether the stored E is the stored E_int plus the kinetic energy of the stored momentum in every bit).
    Energy: both residuals of a converged solve are below r E_tot0, so E_int + (c / c_hat) sum_g E_g changes by the sources within 2 r E_tot0
    (beta_order 1: with the kinetic energy, which enters through p^2 / (2 rho) in double precision — 4 eps of each stored total is added, as in
    test_rad_source_cells_gpu.py::test_branch_sweep_conserves_energy_and_momentum).  Momentum: p + sum_g F_g / (c c_hat) per component within
    4 eps of the summed magnitudes.  At stage 1 the gas side took IMEX_a32 of the change: undone here."""
    L = np.longdouble
    eps = L(np.finfo(np.float64).eps)
    w = L(1.0) / L(IMEX_A32) if stage == 1 else L(1.0)
    U0, U1 = U.astype(L), out.astype(L)
    cs, cc = L(ts.c) / L(ts.chat), L(ts.c) * L(ts.chat)
    dt = L(stage_dt(dt_radiation, stage))
    Src = (src.astype(L) * dt * L(ts.chat)).sum(axis=0)
    Eint0 = eint_from_egas(U).astype(L)
    p_full = U0[1:4] + w * (U1[1:4] - U0[1:4])
    Eint_full = Eint0 + w * (U1[5] - Eint0)
    Etot0 = Eint0 + cs * (U0[6::4].sum(axis=0) + Src)
    before, after = Etot0, Eint_full + cs * U1[6::4].sum(axis=0)
    tol = 2 * L(RESID_TOL) * Etot0
    if ts.beta_order >= 1:
        before = before + (U0[1:4] * U0[1:4]).sum(axis=0) / (2 * U0[0])
        after = after + (p_full * p_full).sum(axis=0) / (2 * U0[0])
        tol = tol + w * 4 * eps * (np.abs(U0[4]) + np.abs(U1[4]))
    e = float(np.max(np.abs(after - before) / tol)) if U.shape[1] else 0.0
    pw = 0.0
    for k in range(3):
        F0, F1 = U0[7 + k::4], U1[7 + k::4]
        dp = p_full[k] + F1.sum(axis=0) / cc - U0[1 + k] - F0.sum(axis=0) / cc
        ptol = 4 * eps * (np.abs(U0[1 + k]) + np.abs(U1[1 + k]) + (np.abs(F0) + np.abs(F1)).sum(axis=0) / cc)
        if U.shape[1]:
            pw = max(pw, float(np.max(np.abs(dp) / np.where(ptol > 0, ptol, 1))))
    exact = bool(np.array_equal(out[4], out[5] + (out[1:4] ** 2).sum(axis=0) / (2.0 * out[0])))
    return e, pw, exact


LADDER = (1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10)


def ladder(e: np.ndarray) -> list:
    return [int((e > t).sum()) for t in LADDER]


# ------------------------------------------------------------------------------------------------ the defining equations at 50 digits
def _double_fractions(ts: MGTraits, table: np.ndarray, T: np.ndarray) -> np.ndarray:
    """(bracketing only) the Planck fractions of exact_exchange_mg in double precision, vectorised over the cells"""
    ng = ts.ng
    x = (ts.energy_unit * np.array(ts.bnd[1:ng]))[:, None] / (ts.kB * T)[None, :]
    lx = np.log10(x)
    gap = 5.0 / 999.0
    j = np.clip(((lx + 3.0) / 5.0 * 999).astype(np.int64), 0, 998)
    y = (table[j + 1] - table[j]) / gap * (lx - (-3.0 + j * gap)) + table[j]
    y = np.where(lx < -3.0, np.clip((-4 + x) * x + 8 * np.log((2 + x) / 2), 0.0, table[0]), y)
    y = np.where((lx >= 2.0) | (x >= 100.0), 1.0, y)
    y = np.concatenate([np.zeros((1, T.size)), y, np.ones((1, T.size))])
    return np.diff(y, axis=0)


def exact_exchange_mg(ts: MGTraits, U: np.ndarray, src: np.ndarray, dt: float, table: np.ndarray):
    """beta_order 0, gamma law, no dust, Erad_floor 0, lower values independent of T, piecewise_constant or PPL_fixed_slope: the backward-Euler
    exchange over `dt` (the stage's dt) from its equations

        E_g = (E_g0 + Src_g + tau_g B_g(T)) / (1 + tau_g),   tau_g = dt rho kappaP_g c_hat,   B_g = a T^4 f_g(T),   Src_g = src_g dt c_hat
        E_int(T) + (c / c_hat) sum_g E_g = E_int0 + (c / c_hat) sum_g (E_g0 + Src_g)
        F_g = F_g0 / (1 + rho kappaF_g(T) c_hat dt)

    f_g: the Planck fractions from the oracle's table VALUES (`table`, data) by the rule of csrc/qk_planck.hpp:39-40 — below the table the series
    (-4 + x) x + 8 log((2 + x) / 2) held between 0 and the first entry, inside it linear interpolation in log10 x between the bracketing points,
    1 from x = 100 on — evaluated in mpmath, so that the exact solution solves the same equations.  kappaP_g: the lower value (piecewise constant),
    or lower_g ((r^k - 1) / k) / ln r with r = nu_R / nu_L, k the group's exponent (the group mean of a power law under a nu^-1 weight, the closed form of
    ComputeGroupMeanOpacity with alpha_quant = -1, reference radiation_system.hpp:1252-1287; k = 0: lower_g).  kappaF_g: kappaP_g (piecewise
    constant); else ComputeDiffusionFluxMeanOpacity as the reference header states it (radiation_system.hpp:1328-1352, with PlanckFunction :1311-1326):
        [(kappaP + kappaE / 3) B_g + (k kappaE B_g - d(nu kappa B)) / 3] / [4 B_g / 3 - d(nu B) / 3],   0 where the denominator is not positive,
        d(nu q B) = nu_R q_R B(nu_R) - nu_L q_L B(nu_L),   B(nu) = (e / k_B T) (15 / pi^4) a T^4 x^3 / (e^x - 1),  x = e nu / k_B T  (0 beyond x = 100).
    One equation in T whose left side increases with T (every B_g does); the interpolated table is only piecewise smooth, so the root is bracketed,
    not iterated: bisection in double precision over all cells at once down to a relative width of 1e-13, then the bracket is verified (and where the double-precision sum cancels, widened) at 50 digits
    and closed to 1e-40 by the Illinois method, which never leaves it.  Returns (E_int[n], E_g[ng][n], F[ng][3][n]) as mpmath numbers."""
    import mpmath as mp
    assert ts.beta_order == 0 and ts.gamma != 1.0 and not ts.dust and ts.Erad_floor == 0.0 and ts.T_exp == 0.0 and ts.model in (1, 2)
    mp.mp.dps = 50
    m = mp.mpf
    ng, n = ts.ng, U.shape[1]
    E0 = eint_from_egas(U)
    rho_f = {0.0: np.ones(n), -1.0: 1.0 / U[0]}.get(ts.rho_exp, U[0] ** ts.rho_exp)
    # group means in double for the bracketing
    mean = np.ones(ng)
    if ts.model == PPL_FIXED_SLOPE:
        for g in range(ng):
            r, k = ts.bnd[g + 1] / ts.bnd[g], ts.kexp[g]
            mean[g] = 1.0 if k == 0.0 else ((r ** k - 1.0) / k) / np.log(r)
    kP = np.array(ts.klow[:ng])[:, None] * mean[:, None] * rho_f[None, :]
    tau = dt * U[0][None, :] * kP * ts.chat
    wgt = tau / (1.0 + tau)
    cs = ts.c / ts.chat
    Src = src * dt * ts.chat
    a1 = U[0] * ts.cvp

    def G(T):
        B = ts.arad * T ** 4 * _double_fractions(ts, table, T)
        return a1 * T + cs * (wgt * (B - U[6::4] - Src)).sum(axis=0) - E0

    hi = (E0 + cs * (U[6::4] + Src).sum(axis=0)) / a1 * (1.0 + 1e-12)
    lo = hi * 1e-30
    for _ in range(160):
        mid = np.sqrt(lo) * np.sqrt(hi)
        up = G(mid) > 0
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    lo, hi = lo * (1.0 - 1e-13), hi * (1.0 + 1e-13)

    tab = [m(float(v)) for v in table]
    gap = m(5) / 999
    cs_m, a_m, kB_m, eu_m, dt_m, chat_m = m(ts.c) / m(ts.chat), m(ts.arad), m(ts.kB), m(ts.energy_unit), m(dt), m(ts.chat)
    cvp_m = kB_m / (m(ts.mmw) * (m(ts.gamma) - 1))
    bnd = [m(b) for b in ts.bnd]
    mean_m = [m(1)] * ng
    if ts.model == PPL_FIXED_SLOPE:
        mean_m = [m(1) if ts.kexp[g] == 0.0 else (((bnd[g + 1] / bnd[g]) ** m(ts.kexp[g]) - 1) / m(ts.kexp[g])) / mp.log(bnd[g + 1] / bnd[g]) for g in range(ng)]

    def Y(x):
        if x >= 100:
            return m(1)
        lx = mp.log10(x)
        if lx < -3:
            return min(max((-4 + x) * x + 8 * mp.log((2 + x) / 2), m(0)), tab[0])
        if lx >= 2:
            return m(1)
        j = int(mp.floor((lx + 3) / 5 * 999))
        if j >= 999:
            return m(1)
        return (tab[j + 1] - tab[j]) / gap * (lx - (-3 + j * gap)) + tab[j]

    def planck(nu, T):
        coeff = eu_m / (kB_m * T)
        x = coeff * nu
        if x > 100:
            return m(0)
        return coeff / (mp.pi ** 4 / 15) * (a_m * T ** 4) * (x ** 3 / mp.expm1(x))

    Eint, Eg, F = [None] * n, [[None] * n for _ in range(ng)], [[[None] * n for _ in range(3)] for _ in range(ng)]
    for i in range(n):
        rho = m(float(U[0, i]))
        rf = m(1) if ts.rho_exp == 0.0 else (1 / rho if ts.rho_exp == -1.0 else rho ** m(ts.rho_exp))
        low = [m(ts.klow[g]) * rf for g in range(ng)]
        kPm = [low[g] * mean_m[g] for g in range(ng)]
        tau_m = [dt_m * rho * kPm[g] * chat_m for g in range(ng)]
        E0g = [m(float(U[6 + 4 * g, i])) + m(float(src[g, i])) * dt_m * chat_m for g in range(ng)]
        a1m = rho * cvp_m
        Ei0 = m(float(E0[i]))

        def frac(T):
            ys = [m(0)] + [Y(eu_m * bnd[g + 1] / (kB_m * T)) for g in range(ng - 1)] + [m(1)]
            return [ys[g + 1] - ys[g] for g in range(ng)]

        def Gm(T):
            f = frac(T)
            return a1m * T + cs_m * sum(tau_m[g] / (1 + tau_m[g]) * (a_m * T ** 4 * f[g] - E0g[g]) for g in range(ng)) - Ei0

        a, b = m(float(lo[i])), m(float(hi[i]))
        fa, fb = Gm(a), Gm(b)
        wide = m(10) ** -12
        while (fa > 0 or fb < 0) and wide < 1:  # (the double-precision G cancels to a few digits in radiation-dominated cells: widen at 50 digits)
            if fa > 0:
                a = a * (1 - wide)
                fa = Gm(a)
            if fb < 0:
                b = b * (1 + wide)
                fb = Gm(b)
            wide *= 10
        assert fa <= 0 <= fb, f"exact_exchange_mg: cell {i}: no bracket"
        side = 0
        for _ in range(200):
            if b - a <= m(10) ** -40 * b or fa == 0 or fb == 0:
                break
            c = (a * fb - b * fa) / (fb - fa)
            if not (a < c < b):
                c = (a + b) / 2
            fc = Gm(c)
            if fc > 0:
                b, fb = c, fc
                if side == 1:
                    fa /= 2
                side = 1
            else:
                a, fa = c, fc
                if side == -1:
                    fb /= 2
                side = -1
        else:
            raise AssertionError("exact_exchange_mg: no convergence")
        T = a if fa == 0 else b
        f = frac(T)
        B = [a_m * T ** 4 * f[g] for g in range(ng)]
        Eint[i] = a1m * T
        for g in range(ng):
            Eg[g][i] = (E0g[g] + tau_m[g] * B[g]) / (1 + tau_m[g])
            if ts.model == PIECEWISE_CONSTANT:
                kF = kPm[g]
            else:
                k = m(ts.kexp[g])
                BL, BR = planck(bnd[g], T), planck(bnd[g + 1], T)
                kR = low[g] * (bnd[g + 1] / bnd[g]) ** k
                d_kB = bnd[g + 1] * kR * BR - bnd[g] * low[g] * BL
                d_B = bnd[g + 1] * BR - bnd[g] * BL
                den = m(4) / 3 * B[g] - d_B / 3
                kF = m(0) if den <= 0 else ((kPm[g] + kPm[g] / 3) * B[g] + (k * kPm[g] * B[g] - d_kB) / 3) / den
            for d3 in range(3):
                F[g][d3][i] = m(float(U[7 + 4 * g + d3, i])) / (1 + rho * kF * chat_m * dt_m)
    return Eint, Eg, F


# ------------------------------------------------------------------------------------------------ targeted cases
# One case per rarely taken branch, for the launch geometry of the GPU tests (N_LAUNCH cells).  They are defined here, beside the generator, so that
# the CPU suite checks what each relies on — the share of cells that take the branch per the oracle's mask, the share that fails — and the GPU
# suite runs the same cells.
N_LAUNCH = 20 * 8 * 8 + 11 * 8 * 8
NARROW_EDGES = (0.5, 0.8, 1.0, 1.25, 2.0)


def power_law_energies(slope):
    """E_g / (nu_R - nu_L) proportional to (bin centre)^slope across the groups, the total unchanged"""
    b = np.array(NARROW_EDGES)
    w = np.sqrt(b[:-1] * b[1:]) ** slope * np.diff(b)

    def edit(U, src):
        tot = U[6::4].sum(axis=0)
        for g in range(4):
            f = w[g] / w.sum()
            U[7 + 4 * g:10 + 4 * g] *= (f * tot / U[6 + 4 * g])[None, :]
            U[6 + 4 * g] = f * tot
    return edit


def zero_two_groups(U, src):
    U[6 + 4:14 + 4] = 0.0  # groups 1 and 2: energy and flux exactly zero
    src[1:3] = 0.0


def negative_group(U, src):
    U[6 + 4 * 2] = -1.0e-3 * U[6]
    U[7 + 4 * 2:10 + 4 * 2] = 0.0
    src[2] = 0.0


def empty_group_with_flux(U, src):
    U[6 + 4:14 + 4:4] = 0.0  # groups 1 and 2: energy exactly zero, the flux kept
    src[1:3] = 0.0


@dataclass(frozen=True)
class Targeted:
    name: str
    ts: MGTraits
    unit: str = "cgs"
    stage: int = 1
    seed: int = 8000
    edit: object = None
    gen: tuple = ()           # keyword arguments of generate_cells, as items
    branches: tuple = ()      # bits of the oracle's mask that at least `share` of the cells must carry
    share: float = 0.5
    never: tuple = ()         # bits that no cell may carry
    decoupled: tuple = None   # (lowest, highest) share of decoupled cells, each wave of the first box holding both kinds

    @property
    def dt(self) -> float:
        return UNITS[self.unit][5]

    def cells(self, n: int = N_LAUNCH):
        U, src = generate_cells(self.ts, self.unit, self.dt, self.stage, n, self.seed, False, **dict(self.gen))
        if self.edit is not None:
            self.edit(U, src)
        return U, src


# Found on the CPU.  At the default threshold (1e-6) a launch straddles it only with dust_gas_interaction_coeff near 3e-38, where a sixth of the
# cells — coupled ones just above the threshold — never converge: their iteration wanders with a negative dust temperature for 100 passes, and
# their counts vary by more than three jitter seeds span.  With coeff = 1e-32 and threshold = 1 the launch straddles the threshold as well (57 %
# decoupled), 1.5 % of the cells fail, every counter is the same under seven jitter seeds without photoelectric heating and within 1 with it,
# and with photoelectric heating 1.5 % of the cells still see a negative dust temperature (fail_dust != 0).
DUST_COEFF, DUST_THRESHOLD = 1.0e-32, 1.0
DUST_VARIANTS = {"plain": dict(), "pe": dict(pe=1, pe_derivative=1.0e-3), "cooling": dict(cooling=(4.0e-11, 0.0, 2.0e-11, 0.0)),
                 "cosmic-rays": dict(cr_heating=3.0e-10), "linear-emission": dict(thermal_model=1, dust_coeff=1.0e-30, dust_threshold=1.0e-6)}  # (a T: every cell coupled)
DUST_CASES = ((2, "plain"), (4, "plain"), (2, "pe"), (4, "pe"), (4, "cooling"), (4, "cosmic-rays"), (4, "linear-emission"))


def _targeted_cases() -> dict:
    out = []

    def add(name, ts, **kw):
        kw["gen"] = tuple(sorted(kw.get("gen", {}).items()))
        out.append(Targeted(name, ts, **kw))

    for model in (1, 2, 3):
        add(f"zero-tau-{MODEL_NAME[model]}", make_traits("cgs", 4, model, "k0", "const", zero_group=1, beta_order=0), seed=8001 + model,
            branches=("zero_tau",), share=1.0)
    for model in (1, 3):
        add(f"dE-constraint-{MODEL_NAME[model]}", make_traits("cgs", 4, model, "k0", "const", beta_order=1), stage=2, seed=8010 + model,
            gen=dict(log10_Tr=(float(np.log10(30.0)), 2.0), log10_tau=(1.0, 6.0), log10_X=(-2.0, 1.0)), branches=("dE_constrain",))
    for model in (2, 3):
        add(f"denom-{MODEL_NAME[model]}", make_traits("cgs", 4, model, "k-2", "const", beta_order=1), seed=8020 + model,
            gen=dict(log10_tau=(-6.0, -2.0), log10_X=(-3.0, -1.0)), branches=("denom_le_0", "x_ge_100"))
    ts = make_traits("cgs", 4, 3, "kmix", "const", beta_order=0)
    ts = replace(ts, bnd=NARROW_EDGES, klow=tuple(float(v) for v in lower_values(NARROW_EDGES, ts.kexp) * UNITS["cgs"][6]))
    for slope, branch in ((150.0, "alpha_gt_100"), (-150.0, "alpha_lt_m100")):
        add(f"steep-{slope:+.0f}", ts, seed=8030, edit=power_law_energies(slope), gen=dict(log10_tau=(-3.0, 0.0), log10_X=(-1.0, 1.0)), branches=(branch,))
    for model in (2, 3):
        add(f"log-log-{MODEL_NAME[model]}", make_traits("dimensionless", 4, model, "k0", "const", beta_order=1), unit="dimensionless", stage=2,
            seed=8040 + model, branches=("alpha_near_0",), share=1.0)
    for edit, branch, eddington in ((zero_two_groups, "slope_zero_mean", 0), (zero_two_groups, "slope_zero_mean", 1),
                                    (empty_group_with_flux, "slope_zero_mean", 1), (negative_group, "slope_sign_change", 0)):
        add(f"{branch}-{edit.__name__}-edd{eddington}", make_traits("cgs", 4, 3, "k-2", "const", beta_order=1, eddington_model=eddington), stage=2,
            seed=8050, edit=edit, gen=dict(log10_tau=(-4.0, 0.0)), branches=(branch,))
    add("slopes-frozen", make_traits("cgs", 4, 3, "kmix", "per_rho", beta_order=1), stage=2, seed=8060, branches=("slopes_frozen",))
    ts = make_traits("cgs", 4, 1, "k0", "const", beta_order=0)
    add("floor", replace(ts, Erad_floor=4 * 1.0e-7 * ts.arad * reference_point("cgs")[1] ** 4), seed=8070,
        gen=dict(log10_tau=(0.0, 1.0), log10_X=(-3.0, -2.0)), branches=("floor_clamp",))
    for model in (1, 2):
        for scale, branch, other in ((1.0e8, "x_ge_100", "below_table"), (1.0e-8, "below_table", "x_ge_100")):
            ts = make_traits("cgs", 4, model, "k-2", "const", beta_order=1)
            add(f"{branch}-{MODEL_NAME[model]}", replace(ts, bnd=tuple(b * scale for b in ts.bnd)), stage=2, seed=8080 + model,
                gen=dict(share_floor=1e-3), branches=(branch,), share=1.0, never=(other,))
    for model in (1, 2, 3):
        add(f"isothermal-{MODEL_NAME[model]}", make_traits("cgs", 4, model, "kmix", "const", beta_order=1, gamma=1.0), seed=8090 + model)
    for ng, variant in DUST_CASES:
        kw = dict(DUST_VARIANTS[variant])
        if "cooling" in kw:
            kw["cooling"] = kw["cooling"][:ng]
        ts = make_traits("cgs", ng, 1, "k0", "const", beta_order=1, dust=1, **{"dust_coeff": DUST_COEFF, "dust_threshold": DUST_THRESHOLD, **kw})
        add(f"dust-ng{ng}-{variant}", ts, seed=9000 + ng, gen=dict(log10_tau=(-2.0, 2.0), log10_X=(-1.0, 1.0)),
            decoupled=(None if variant == "linear-emission" else (0.3, 0.7)))
    return {t.name: t for t in out}


TARGETED = _targeted_cases()


def check_targeted(t: Targeted, Uo: np.ndarray, rec: dict, tot: list):
    """what a targeted case relies on, from the plain oracle alone (asserted by the CPU suite, and again where the GPU suite runs the case)"""
    failed = failed_cells(Uo, rec)
    print(f"{t.name}: failed share {failed.mean():.2%}" + "".join(f", {b} {took(rec, b).mean():.1%}" for b in t.branches + t.never))
    for b in t.branches:
        assert took(rec, b).mean() >= t.share, f"{t.name}: branch {b} taken by {took(rec, b).mean():.1%} of the cells only"
    for b in t.never:
        assert not took(rec, b).any(), f"{t.name}: branch {b} taken"
    if t.decoupled is not None:
        dec = took(rec, "decoupled")
        print(f"{t.name}: decoupled {dec.mean():.1%}, negative dust temperature {took(rec, 'negative_dust_T').mean():.1%}")
        assert t.decoupled[0] <= dec.mean() <= t.decoupled[1]
        waves = dec[:1280].reshape(20, 64)
        assert (waves.any(axis=1) & ~waves.all(axis=1)).all(), "every wave of the first box holds both kinds"
        assert tot[3] > 0 and (tot[5] > 0 or not t.ts.pe)
    compared = ~failed if not t.branches else ~failed & np.all([took(rec, b) for b in t.branches], axis=0)
    assert compared.mean() >= 0.5, f"{t.name}: only {compared.mean():.1%} of the cells take the branch and are compared (the failing ones are not)"
    if t.ts.gamma == 1.0:
        assert np.isfinite(Uo).all() and tot[0] == 0
    if t.name == "slopes-frozen":
        assert np.median(rec["newton_max"]) > MAX_ITER_ALPHA
    if t.edit in (zero_two_groups, empty_group_with_flux):
        empty = (Uo[6 + 4] == 0.0) | (Uo[6 + 8] == 0.0)
        bad = ~np.isfinite(Uo).all(axis=0)
        print(f"{t.name}: a group still empty after the solve in {empty.sum()} cells, {bad.sum()} cells non-finite in the oracle")
        if t.edit is empty_group_with_flux:  # (the work term of a group with a flux refills it in most cells; a fifth of the fluxes vanish or lie along an axis)
            assert empty.sum() >= 20 and 10 <= bad.sum() < empty.sum()
        else:
            assert empty.sum() >= 50 and (bad.sum() >= 50 if t.ts.eddington_model == 0 else not bad[empty].any())


# ------------------------------------------------------------------------------------------------ the failure list
FAILURE_CASE = Case(4, 1, 1, 2, source=False, unit="cgs", eddington=0, kexp="k0", lower="const", seed=8100)
NAN_AT, GIVEN_UP_AT = 5 + 33 * np.arange(60), 6 + 33 * np.arange(60)  # spread over the waves and over both boxes (cells 1280 .. 1983: the second)


def failure_cells(oracle):
    """(traits, U_plain, U_nan, U_both, src): an ordinary list of N_LAUNCH cells; the same with NaN gas energy in the cells NAN_AT; and that with 60
    radiation-dominated cells (X = 1e12) the reference gives up on in the cells GIVEN_UP_AT.  Found on the CPU: of 400 cells at X = 1e10 the oracle
    fails in 243, at X = 1e12 in 325, at X = 1e14 in 378, and with sources of 1e6 .. 1e12 E_g in 183 .. 197 of 197, those without an outer failure
    (totals of the X = 1e12 list: 1491 solves, 896 Newton failures, 126 outer failures).  The 60 cells are the first of the X = 1e12 candidates
    whose record — failing — is the same in the plain oracle and under every jitter seed: failing by construction, not marginal."""
    case = FAILURE_CASE
    ts = case.traits()
    U_plain, src = generate_cells(ts, case.unit, case.dt, case.stage, N_LAUNCH, case.seed, False)
    Ux, sx = generate_cells(ts, case.unit, case.dt, case.stage, 400, case.seed + 1, False, log10_X=(12.0, 12.0))
    runs = [oracle.rad_mg_source_cells(oracle_traits(ts), Ux, sx, case.dt, case.stage, seed, JITTER_ULPS if seed else 0) for seed in (0,) + JITTER_SEEDS]
    steady = failed_cells(runs[0][0], runs[0][1])
    for Uj, rj, _ in runs[1:]:
        steady &= failed_cells(Uj, rj) & np.all([rj[k] == runs[0][1][k] for k in rj], axis=0)
    pick = np.flatnonzero(steady)[:60]
    assert pick.size == 60
    U_nan = U_plain.copy()
    U_nan[4, NAN_AT] = np.nan
    U_both = U_nan.copy()
    U_both[:, GIVEN_UP_AT] = Ux[:, pick]
    return ts, U_plain, U_nan, U_both, src
