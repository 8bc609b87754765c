"""Helpers of the cell-by-cell tests of the matter-radiation exchange (AddSourceTermsSingleGroup): trait sets, a seeded cell generator and an
independent 50-digit solution of the implicit system.  Nothing here needs a GPU; mpmath is imported by exact_exchange alone (the GPU tests do not
call it); the two *_traits functions import the ctypes bindings when called.

Constants of the reference's scheme, quoted from its headers (src/radiation/radiation_system.hpp:52, src/radiation/source_terms_single_group.hpp:100,
:158-159) and NOT read from the kernel under test."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

IMEX_A32 = 0.5       # radiation_system.hpp:52
RESID_TOL = 1.0e-11  # source_terms_single_group.hpp:158
MAX_NEWTON = 100     # :159, `for (n = 0; n < maxIter; ++n)`: a solve that never converges leaves the loop with n == 100 and is counted as n + 1 (:345)
MAX_OUTER = 5        # :100, `for (ite = 0; ite < max_ite; ++ite)`

C_CGS = 2.99792458e10
A_CGS = 4.0 * 5.670374419e-5 / C_CGS
K_B = 1.380649e-16
M_U = 1.6605390666e-24
GAMMA = 5.0 / 3.0


@dataclass(frozen=True)
class ExchangeTraits:
    """the fields of qk_rad_traits / qk_hydro_traits the exchange reads"""
    c: float
    chat: float
    arad: float
    kB: float        # EOS_Traits::boltzmann_constant
    mmw: float       # EOS_Traits::mean_molecular_weight
    gamma: float = GAMMA
    beta_order: int = 1
    opacity_model: int = 0
    kappaP: float = 1.0
    kappaE: float = 1.0
    kappaF: float = 1.0
    T_ref: float = 1.0
    T_exp: float = 0.0
    pow_floor: float = 0.0
    pow_mode: int = 1
    eddington_model: int = 0
    Erad_floor: float = 0.0
    kappa_nominal: float = 1.0  # (generator only) the opacity that turns tau into a density where kappaP itself cannot: k0 / rho, kappaP = 0

    @property
    def cvp(self) -> float:
        """E_int = rho cvp T for the gamma law"""
        return self.kB / (self.mmw * (GAMMA - 1.0))


def units(name: str, **kw) -> ExchangeTraits:
    if name == "cgs":
        return ExchangeTraits(C_CGS, 0.1 * C_CGS, A_CGS, K_B, M_U, **kw)
    assert name == "dimensionless"
    return ExchangeTraits(1.0, 1.0, 1.0, 1.0, 1.0, kappa_nominal=KAPPA_DIMENSIONLESS, **kw)


def oracle_traits(ts: ExchangeTraits):
    from oracle.pyoracle import RadCellTraits
    return RadCellTraits(ts.c, ts.chat, ts.arad, ts.Erad_floor, ts.kappaP, ts.kappaE, ts.kappaF, ts.T_ref, ts.T_exp, ts.pow_floor, ts.gamma, ts.mmw, ts.kB,
                         ts.beta_order, ts.opacity_model, ts.pow_mode, ts.eddington_model)


def device_traits(ts: ExchangeTraits):
    from quokka_amd import capi
    rt = capi.RadTraits(ts.c, ts.chat, ts.arad, ts.Erad_floor, ts.beta_order, ts.opacity_model, ts.kappaP, ts.kappaE, ts.kappaF, ts.pow_mode,
                        ts.eddington_model, ts.T_ref, ts.T_exp, ts.pow_floor)
    return rt, capi.traits(ts.gamma, False, 3, mean_molecular_weight=ts.mmw, boltzmann_constant=ts.kB)


def stage_dt(dt_radiation: float, stage: int) -> float:
    return (1.0 - IMEX_A32) * dt_radiation if stage == 2 else dt_radiation


# ------------------------------------------------------------------------------------------------ opacity sets
# name -> (fields of ExchangeTraits, dt_radiation per unit system is chosen so that tau = dt rho kappaP c_hat is O(1) at the middle of the ranges)
OPACITY_SETS = {
    "equal": dict(),
    "P2E": dict(kappaP=2.0, kappaE=1.0, kappaF=1.0),
    "F3E": dict(kappaP=1.0, kappaE=1.0, kappaF=3.0),
    "per_rho": dict(opacity_model=1),                                                   # kappa = k0 / rho
    "T-3": dict(opacity_model=2, T_exp=-3.0),                                           # RadMarshakAsymptotic
    "T-3.5": dict(opacity_model=2, T_exp=-3.5, kappaF=1.5),                             # RadhydroPulseGrey: the flux mean differs
    "T+3floor": dict(opacity_model=2, T_exp=3.0, pow_floor=1.0),                        # RadPulse
}
DT = {"cgs": 1.0e3, "dimensionless": 1.0}
# c = a = k_B / mu = 1 is a unit system in which the radiation constant is enormous against the gas constants (CGS: a c^2 / (k_B / m_u)^4 ~ 1e-26
# per g cm^-3 K^-3...): at densities of order one the ranges of X put E_r far above rho c^2, the momentum exchange drives the gas past c and the
# reference's iteration fails in a quarter of the moving cells (measured on the CPU oracle: 24 % at kappa = 1, 0.4 % at 1e20, none from 1e28).
# The dimensionless cases therefore use kappa = 1e30 (rho = tau / (dt kappa c_hat) in [1e-36, 1e-24]) and, for the power law, T_ref = 1e-12.
KAPPA_DIMENSIONLESS = 1.0e30
T_REF = {"cgs": 1.0e3, "dimensionless": 1.0e-12}


# src dt c_hat / E_r of the cells with an energy source.  The reference's iteration gives up on strong sources — no cell below 3, 4 % of the cells at
# 10, 40 % at 300 - 1000, measured on the CPU oracle — and with the full range [1e-3, 1e3] 2.8 - 5.5 % of all cells fail (1.3 - 1.5 % only for
# kappaP = 2 kappaE), above the 2 % the branch sweep may lose.  The sweep therefore stops at 1e2 (at 10^1.5 for the power-law opacities, which
# fail about twice as often): at most 0.94 % of the cells of any case then fail.  The sources from there to 1e3 are in the failure-path test of
# test_rad_source_cells_gpu.py, where failing is what is tested.
LOG10_SRC = (-3.0, 2.0)
LOG10_SRC_POWER_LAW = (-3.0, 1.5)


def tau_ref(ts: ExchangeTraits) -> float:
    """power-law opacity: the optical depth of a cell at T_ref (with a floor: the least optical depth there is)"""
    return 1.0e-6 if ts.pow_floor > 0 else 1.0


@dataclass(frozen=True)
class Case:
    beta_order: int
    opacity: str
    stage: int
    source: bool
    unit: str
    eddington: int
    seed: int

    @property
    def id(self) -> str:
        return f"b{self.beta_order}-{self.opacity}-s{self.stage}-{'src' if self.source else 'nosrc'}-{self.unit[:3]}-edd{self.eddington}"

    def traits(self, pow_mode: int = 1) -> ExchangeTraits:
        ts = units(self.unit, beta_order=self.beta_order, eddington_model=self.eddington, pow_mode=pow_mode, T_ref=T_REF[self.unit],
                   **OPACITY_SETS[self.opacity])
        # constant opacities as given; k0 / rho: tau = dt k0 c_hat = 1 in every cell; power law: tau = TAU_REF at T_ref (see generate_cells)
        scale = {0: ts.kappa_nominal, 1: 1.0 / (self.dt * ts.chat), 2: tau_ref(ts) / (self.dt * ts.chat)}[ts.opacity_model]
        return replace(ts, kappaP=ts.kappaP * scale, kappaE=ts.kappaE * scale, kappaF=ts.kappaF * scale)

    @property
    def dt(self) -> float:
        return DT[self.unit]


def branch_cases() -> list:
    """a covering subset of beta_order x opacity set x stage x source x unit system x eddington_model: every (beta_order, opacity set) pair at both
    stages; source, unit system and closure alternate so that every value of each meets every beta_order, every opacity set and both stages"""
    out = []
    for ib, beta in enumerate((0, 1, 2, 3)):
        for io, name in enumerate(OPACITY_SETS):
            for stage in (1, 2):
                k = ib + io + stage
                out.append(Case(beta, name, stage, source=bool((k + io // 2) % 2), unit=("cgs", "dimensionless")[(k // 2 + ib) % 2],
                                eddington=(io + stage + ib // 2) % 2, seed=1000 + len(out)))
    # the closure only matters with a work term and a flux: both closures for each beta_order >= 1 in CGS with different means as well
    for beta in (1, 2, 3):
        for edd in (0, 1):
            out.append(Case(beta, "F3E", 2, source=False, unit="cgs", eddington=edd, seed=2000 + len(out)))
    return out


# ------------------------------------------------------------------------------------------------ cell generator
def _directions(r: np.random.Generator, n: int) -> np.ndarray:
    """unit vectors, random on the sphere; one in ten along an axis (the other two components exactly zero)"""
    v = r.normal(size=(3, n))
    v /= np.sqrt((v * v).sum(axis=0))
    axis = r.random(n) < 0.1
    ax = r.integers(0, 3, n)
    sign = np.where(r.random(n) < 0.5, -1.0, 1.0)
    for d in range(3):
        v[d] = np.where(axis, np.where(ax == d, sign, 0.0), v[d])
    return v


def generate_cells(ts: ExchangeTraits, dt_radiation: float, stage: int, n: int, seed: int, source: bool, log10_X=(-4.0, 4.0), log10_src=None):
    """(U[10, n], src[n]).  Sampled: log10 tau uniform in [-6, 6] (tau = dt rho kappaP c_hat, dt the stage's), X = (c / c_hat) a T^4 / E_int
    log-uniform in [1e-4, 1e4] (log10_X: another range, for the cells meant to fail), E_r / (a T^4) log-uniform in [1e-3, 1e3] ([1e-2, 1] for the power law), the reduced flux 0 / 0.999999 / uniform below, gas at rest in one cell of
    ten and beta log-uniform in [1e-6, 1e-2] otherwise, the energy source off or src dt c_hat / E_r log-uniform in [1e-3, 1e2] in half of the cells
    (LOG10_SRC above; log10_src: another range).
    Constant opacity: tau fixes rho, X then T.  kappa = k0 / rho: tau is the same in every cell (dt k0 c_hat), rho is drawn as for kappa_nominal (so is it where kappaP = 0).
    Power law: tau fixes T (10 % of the cells sit below T_ref, on the floor where there is one), X then rho."""
    r = np.random.default_rng(seed)
    dt = stage_dt(dt_radiation, stage)
    cs = ts.c / ts.chat
    tau = 10.0 ** r.uniform(-6.0, 6.0, n)
    X = 10.0 ** r.uniform(log10_X[0], log10_X[1], n)
    k_nom = ts.kappaP if (ts.opacity_model == 0 and ts.kappaP > 0) else ts.kappa_nominal
    if ts.opacity_model == 2:
        # tau = dt k0 c_hat max((T / T_ref)^p, floor) with dt k0 c_hat = tau_ref (Case.traits; a factor 1 - IMEX_a32 off at stage 2)
        x = (tau / tau_ref(ts)) ** (1.0 / ts.T_exp)
        low = r.random(n) < 0.1
        if ts.pow_floor > 0:
            x = np.where(low, r.uniform(0.1, 1.0, n), x)
        T = ts.T_ref * x
        # X = cs a T^4 / (rho cvp T)
        rho = cs * ts.arad * T ** 3 / (X * ts.cvp)
    else:
        rho = tau / (dt * k_nom * ts.chat)
        # X = cs a T^4 / (rho cvp T)  ->  T^3 = X rho cvp / (cs a)
        T = np.cbrt(X * rho * ts.cvp / (cs * ts.arad))
    Eint = rho * ts.cvp * T
    # (power law: the opacity moves by T^p within the solve.  With p < 0 and radiation hotter than the gas the reference's Newton iteration fails in
    # 3 - 17 % of the cells with E_r > a T^4; with p = +3, X > 1e3 and E_r < 4e-3 a T^4 — gas that cools fivefold — in 4e-5 of the cells, source off,
    # both measured on the CPU oracle; none of 8e5 cells fails inside [1e-2, 1], which is the range the power-law sets use)
    lo_hi = (-2.0, 0.0) if ts.opacity_model == 2 else (-3.0, 3.0)
    Er = 10.0 ** r.uniform(lo_hi[0], lo_hi[1], n) * ts.arad * T ** 4
    u = r.random(n)
    f = np.where(u < 0.1, 0.0, np.where(u < 0.2, 0.999999, r.uniform(0.0, 0.999999, n)))
    F = _directions(r, n) * (f * ts.c * Er)
    beta = np.where(r.random(n) < 0.1, 0.0, 10.0 ** r.uniform(-6.0, -2.0, n))
    mom = _directions(r, n) * (beta * ts.c * rho)
    U = np.zeros((10, n))
    U[0], U[1:4], U[5], U[6], U[7:10] = rho, mom + 0.0, Eint, Er, F + 0.0  # (+ 0.0: no -0, which the scheme's `0. + dMomentum` turns into +0)
    U[4] = Eint + (mom * mom).sum(axis=0) / (2.0 * rho)
    on = (r.random(n) < 0.5) & bool(source)
    lo_s, hi_s = log10_src if log10_src is not None else (LOG10_SRC_POWER_LAW if ts.opacity_model == 2 else LOG10_SRC)
    ratio = 10.0 ** r.uniform(lo_s, hi_s, n)
    src = np.where(on, ratio * Er / (dt * ts.chat), 0.0)
    return U, src


def eint_from_egas(U: np.ndarray) -> np.ndarray:
    """ComputeEintFromEgas (radiation_system.hpp) in the same double-precision operations: what the scheme takes as the initial gas energy"""
    return U[4] - (U[1] * U[1] + U[2] * U[2] + U[3] * U[3]) / (2.0 * U[0])


def failed_cells(Uo: np.ndarray, rec: dict) -> np.ndarray:
    """cells in which the oracle reports a failure or returns a non-finite value"""
    return (rec["fail_newton"] > 0) | (rec["fail_outer"] > 0) | ~np.isfinite(Uo).all(axis=0)


# ------------------------------------------------------------------------------------------------ the defining equations at 50 digits
def exact_exchange(ts: ExchangeTraits, U: np.ndarray, src: np.ndarray, dt: float):
    """beta_order 0, kappaP == kappaE, constant opacity, gamma law: the backward-Euler exchange over `dt` (the stage's dt) from its equations

        E_r = (E_r0 + Src + tau a T^4) / (1 + tau),   tau = dt rho kappaP c_hat,   Src = src dt c_hat
        E_int(T) + (c / c_hat) E_r = E_int0 + (c / c_hat) (E_r0 + Src)
        F = F0 / (1 + rho kappaF c_hat dt)

    One increasing convex equation in T, solved by Newton's method from above (monotone convergence) to 1e-45.  Returns (E_int, E_r, F[3]) as arrays
    of mpmath numbers; E_int0 is the initial gas energy as the scheme forms it (eint_from_egas)."""
    import mpmath as mp
    assert ts.beta_order == 0 and ts.kappaP == ts.kappaE and ts.opacity_model == 0 and ts.gamma != 1.0
    mp.mp.dps = 50
    m = mp.mpf
    cs = m(ts.c) / m(ts.chat)
    cvp = m(ts.kB) / (m(ts.mmw) * (m(ts.gamma) - 1))
    E0 = eint_from_egas(U)
    n = U.shape[1]
    Eint, Er, F = [None] * n, [None] * n, [[None] * n for _ in range(3)]
    for i in range(n):
        rho = m(float(U[0, i]))
        tau = m(dt) * rho * m(ts.kappaP) * m(ts.chat)
        Src = m(float(src[i])) * m(dt) * m(ts.chat)
        Er0 = m(float(U[6, i]))
        # a1 T + b T^4 = C  with  a1 = rho cvp,  b = cs tau a / (1 + tau),  C = E_int0 + cs (E_r0 + Src) tau / (1 + tau)
        a1 = rho * cvp
        b = cs * tau * m(ts.arad) / (1 + tau)
        Cc = m(float(E0[i])) + cs * (Er0 + Src) * tau / (1 + tau)
        T = Cc / a1
        if b > 0:
            T = min(T, mp.root(Cc / b, 4))
            for _ in range(200):
                d = (a1 * T + b * T ** 4 - Cc) / (a1 + 4 * b * T ** 3)
                T -= d
                if abs(d) <= m(10) ** -45 * T:
                    break
            else:
                raise AssertionError("exact_exchange: no convergence")
        Eint[i] = a1 * T
        Er[i] = (Er0 + Src + tau * m(ts.arad) * T ** 4) / (1 + tau)
        den = 1 + rho * m(ts.kappaF) * m(ts.chat) * m(dt)
        for d3 in range(3):
            F[d3][i] = m(float(U[7 + d3, i])) / den
    return Eint, Er, F


def with_traits(ts: ExchangeTraits, **kw) -> ExchangeTraits:
    return replace(ts, **kw)
