"""Helpers of the face-by-face and cell-by-cell tests of the hydro operators (tests/test_hydro_cells_reference.py, tests/test_hydro_cells_gpu.py):
trait sets, seeded generators of face states and cell states built to take every branch of the Riemann solvers and of the cell-update operators, a
numpy classifier that names the branch of each sample, and an np.longdouble restatement of the cell operators.  Nothing here needs a GPU.

The classifier only COUNTS populations (a case must hold enough samples of the branch it targets); it never decides whether a value passes.  A tie
it resolves differently from the oracle in the last ulp moves one sample from one count to another and does no harm.

Constants of the reference's scheme are quoted from its headers (src/hydro/HLLC.hpp, src/hydro/HLLD.hpp, src/hydro/hydro_system.hpp) and not read
from the kernels under test."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

EPS = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
K_B = 1.380649e-16
M_U = 1.6605390666e-24
ETA_DUAL = 1.0e-3     # hydro_system.hpp:822
SMALL_X = 1.0e-30     # network_rp::small_x (hydro_system.hpp:731)
HLLC, LLF, HLLD = 0, 1, 2
MIN_SHARE, MIN_COUNT = 0.01, 256  # the population condition: a targeted branch holds at least 1 % of the samples and at least 256 of them


# ------------------------------------------------------------------------------------------------ trait sets
@dataclass(frozen=True)
class Units:
    """magnitudes of one unit system and the EOS constants that go with it"""
    name: str
    rho: tuple        # log10 range of the density
    cs: tuple         # log10 range of the sound speed (gamma law: P = rho c_s^2 / gamma)
    mmw: float        # EOS_Traits::mean_molecular_weight
    kB: float         # EOS_Traits::boltzmann_constant
    cs_iso: float     # EOS_Traits::cs_isothermal of the isothermal runs


# code units: rho over four decades, P = rho c_s^2 / gamma over six (c_s over three, independent of rho)
CODE = Units("code", (-2.0, 2.0), (-1.5, 1.5), 1.0, 1.0, 1.0)
# CGS: rho of 1e-27 .. 1e-20 g cm^-3, c_s of 1e5 .. 1e8 cm s^-1 (velocities up to Mach 10: 1e9), hydrogen and the CGS Boltzmann constant
CGS = Units("cgs", (-27.0, -20.0), (5.0, 8.0), M_U, K_B, 2.0e4)
UNITS = {"code": CODE, "cgs": CGS}


@dataclass(frozen=True)
class Eos:
    units: Units
    gamma: float = 1.4

    @property
    def isothermal(self) -> bool:
        return self.gamma == 1.0

    def oracle_traits(self, ndim=3, reconstruct_eint=True, nscalars=0):
        from oracle import pyoracle
        return pyoracle.traits(self.gamma, reconstruct_eint, ndim, nscalars, self.units.mmw, self.units.kB, self.units.cs_iso if self.isothermal else float("nan"))

    def device_traits(self, ndim=3, reconstruct_eint=True, nscalars=0, nmscalars=0):
        from quokka_amd import capi
        return capi.traits(self.gamma, reconstruct_eint, ndim, self.units.mmw, self.units.kB, self.units.cs_iso if self.isothermal else float("nan"), nscalars,
                           nmscalars)

    # the gamma-law EOS in the direct association (oracle/eos.hpp variant 0), float64 or longdouble according to the arguments
    def T_from_eint(self, rho, Eint):
        e = Eint / rho
        T = e * (self.units.mmw / M_U) * M_U * (self.gamma - 1.0) / K_B
        return T * K_B / self.units.kB

    def eint_from_T(self, rho, T):
        p = rho * T * K_B / ((self.units.mmw / M_U) * M_U)
        e = p / ((self.gamma - 1.0) * rho)
        return e * rho * self.units.kB / K_B


# ------------------------------------------------------------------------------------------------ face states
def _logu(rng, lo, hi, n):
    return 10.0 ** rng.uniform(lo, hi, n)


def face_box(ndim: int, d: int):
    """(vlo, vhi) of a valid box whose face box in direction d holds 32^3 (3-D), 128^2 (2-D) or 4096 (1-D) faces"""
    n = {3: [32, 32, 32], 2: [128, 128, 1], 1: [4096, 1, 1]}[ndim]
    n[d] -= 1
    return [0, 0, 0], [n[0] - 1, n[1] - 1, n[2] - 1]


def face_shape(ndim: int, d: int):
    lo, hi = face_box(ndim, d)
    return tuple(hi[a] - lo[a] + 1 + (1 if a == d else 0) for a in (2, 1, 0))


def face_states(eos: Eos, family: str, d: int, n: int, seed: int, nscalars: int = 0):
    """n independent faces: dict of rho [2, n], vel [2, 3, n] (array order x, y, z), P [2, n], Eaux [2, n], scal [2, nscalars, n]; side 0 is the left one.
    family 'a': independent sides; rho and c_s log-uniform over the ranges of the unit system, Mach number log-uniform over 1e-3 .. 10 in a random
    direction — the star fans, the cs_exp <= 0 fallback, the low-Mach factor.
    family 'b': nearly equal sides (1 % scatter) carried by a common bulk velocity of Mach -10 .. 10 along the face normal — the supersonic fans."""
    rng = np.random.default_rng(seed)
    u = eos.units
    g = eos.gamma
    rho, P, vel = np.empty((2, n)), np.empty((2, n)), np.empty((2, 3, n))

    def cs_of(r, p):
        return np.full(n, u.cs_iso) if eos.isothermal else np.sqrt(g * p / r)

    if family == "a":
        for s in range(2):
            rho[s] = _logu(rng, *u.rho, n)
            P[s] = rho[s] * _logu(rng, *u.cs, n) ** 2 / (g if not eos.isothermal else 1.0)
            mach = _logu(rng, -3.0, 1.0, n)
            e = rng.standard_normal((3, n))
            e /= np.sqrt((e * e).sum(axis=0))
            vel[s] = mach * cs_of(rho[s], P[s]) * e
    else:
        assert family == "b"
        rho[0] = _logu(rng, *u.rho, n)
        P[0] = rho[0] * _logu(rng, *u.cs, n) ** 2 / (g if not eos.isothermal else 1.0)
        cs = cs_of(rho[0], P[0])
        vel[0] = 0.1 * cs * rng.uniform(-1.0, 1.0, (3, n))
        vel[0, d] = rng.uniform(-10.0, 10.0, n) * cs
        rho[1] = rho[0] * (1.0 + 0.01 * rng.standard_normal(n))
        P[1] = P[0] * (1.0 + 0.01 * rng.standard_normal(n))
        vel[1] = vel[0] + 0.01 * cs * rng.standard_normal((3, n))
    if eos.isothermal:
        P = rho * (u.cs_iso * u.cs_iso)
    Eaux = P / ((g - 1.0) if not eos.isothermal else 1.0) * (1.0 + 0.01 * rng.standard_normal((2, n)))
    scal = rho[:, None, :] * rng.uniform(0.0, 1.0, (2, nscalars, n))
    return dict(rho=rho, vel=vel, P=P, Eaux=Eaux, scal=scal)


def pack_face_states(eos: Eos, fs, reconstruct_eint: bool, shape):
    """the left and right reconstructed primitive states as ComputeFluxes reads them (hydro_system.hpp:881-938), [nvar, nz, ny, nx] each"""
    out = []
    for s in range(2):
        rho = fs["rho"][s]
        if reconstruct_eint and not eos.isothermal:
            c4, c5 = fs["P"][s] / ((eos.gamma - 1.0) * rho), fs["Eaux"][s] / rho  # specific internal energies
        else:
            c4, c5 = fs["P"][s], fs["Eaux"][s]
        q = np.concatenate([rho[None], fs["vel"][s], c4[None], c5[None], fs["scal"][s]], axis=0)
        out.append(np.ascontiguousarray(q.reshape((q.shape[0],) + tuple(shape))))
    return out


def face_pressure(eos: Eos, q, reconstruct_eint: bool):
    """P as ComputeFluxes forms it from a packed state (float64, the reference's association)"""
    rho = q[0]
    if eos.isothermal:
        return rho * (eos.units.cs_iso * eos.units.cs_iso)
    if reconstruct_eint:
        return (eos.gamma - 1.0) * rho * ((q[4] * rho) / rho)
    return q[4]


def prim_velocities(ndim: int, d: int, nvar: int, vscale: float, seed: int, ng: int = 1, flat: bool = False):
    """the primitive array ComputeFluxes takes its velocity differences from: the valid box of face_box grown by ng, velocities uniform in
    +-1.5 vscale per cell (differences up to 3 vscale, either sign), every other component NaN (it must not be read).  flat: zero velocities."""
    lo, hi = face_box(ndim, d)
    shape = tuple(hi[a] - lo[a] + 1 + (2 * ng if a < ndim else 0) for a in (2, 1, 0))
    rng = np.random.default_rng(seed)
    q = np.full((nvar,) + shape, np.nan)
    q[1:4] = 0.0 if flat else vscale * rng.uniform(-1.5, 1.5, (3,) + shape)
    return q


def axes(ndim: int, d: int):
    """array axes (0 = x, 1 = y, 2 = z) of the normal, view-j and view-k directions (hydro_system.hpp:954-976)"""
    if ndim == 2 and d == 1:
        return 1, 0, 2
    return d, (d + 1) % 3, (d + 2) % 3


def velocity_differences(prim, ndim: int, d: int, ng: int = 1, nvalid=None):
    """du, dw and div_v of every face of the face box (hydro_system.hpp:1019-1055), by numpy slicing; nvalid: the extents (x, y, z) of the valid
    box prim is grown from (default: the box of face_box)"""
    if nvalid is None:
        lo, hi = face_box(ndim, d)
        nvalid = [hi[a] - lo[a] + 1 for a in range(3)]
    AN, AV, AW = axes(ndim, d)

    def cells(comp, shift):
        """velocity component `comp` at the cell to the RIGHT of each face (shift[a] added to its index)"""
        sl = []
        for a in (2, 1, 0):
            g = ng if a < ndim else 0
            n = nvalid[a] + (1 if a == d else 0)
            sl.append(slice(g + shift[a], g + shift[a] + n))
        return prim[1 + comp][tuple(sl)]

    def sh(a, s, base=(0, 0, 0)):
        r = list(base)
        r[a] += s
        return r

    left = sh(AN, -1)
    du = cells(AN, (0, 0, 0)) - cells(AN, left)
    dw = np.zeros_like(du)
    div = du.copy()
    if ndim >= 2:
        dvl = np.minimum(cells(AV, sh(AV, 1, left)) - cells(AV, left), cells(AV, left) - cells(AV, sh(AV, -1, left)))
        dvr = np.minimum(cells(AV, sh(AV, 1)) - cells(AV, (0, 0, 0)), cells(AV, (0, 0, 0)) - cells(AV, sh(AV, -1)))
        dw = np.minimum(dvl, dvr)
        div = div + 0.5 * (dvl + dvr)
    if ndim == 3:
        dwl = np.minimum(cells(AW, sh(AW, 1, left)) - cells(AW, left), cells(AW, left) - cells(AW, sh(AW, -1, left)))
        dwr = np.minimum(cells(AW, sh(AW, 1)) - cells(AW, (0, 0, 0)), cells(AW, (0, 0, 0)) - cells(AW, sh(AW, -1)))
        dw = np.minimum(np.minimum(dwl, dwr), dw)
        div = div + 0.5 * (dwl + dwr)
    return du, dw, div


def classify_faces(eos: Eos, L, R, reconstruct_eint: bool, ndim: int, d: int, du, dw, div_v, K_visc: float, riemann: int = HLLC):
    """the branch of every face as boolean arrays: the fan ('fan_L', 'star_L', 'star_R', 'fan_R'), 'cs_exp_le_0', 'theta_lt_1', 'chi_lt_1',
    'mass_flux_ge_0' / 'mass_flux_lt_0', 'viscosity'; for HLLD its own fans and 'rhoStarL_le_0'.  Also returns the wave speeds."""
    AN, AV, AW = axes(ndim, d)
    g = eos.gamma
    iso = eos.isothermal
    with np.errstate(all="ignore"):
        rl, rr = L[0], R[0]
        PL, PR = face_pressure(eos, L, reconstruct_eint), face_pressure(eos, R, reconstruct_eint)
        ul, ur = L[1 + AN], R[1 + AN]
        if iso:
            csl = np.full_like(rl, eos.units.cs_iso)
            csr = csl
        else:
            csl, csr = np.sqrt(g * PL / rl), np.sqrt(g * PR / rr)
        viscosity = K_visc * np.maximum(-div_v, 0.0)
        out = {"viscosity": viscosity > 0.0}
        if riemann == LLF:
            Sp = np.maximum(np.abs(ul) + csl, np.abs(ur) + csr)
            F0 = 0.5 * (ul * rl + ur * rr) - (0.5 * Sp) * (rr - rl)
        elif riemann == HLLD:
            cfl, cfr = np.sqrt(0.5 * (g * PL + np.sqrt((g * PL) ** 2)) / rl), np.sqrt(0.5 * (g * PR + np.sqrt((g * PR) ** 2)) / rr)
            S_L, S_R = np.minimum(ul - cfl, ur - cfr), np.maximum(ul + cfl, ur + cfr)
            aL, aR = S_L - ul, S_R - ur
            S_M = (aR * (ur * rr) - aL * (ul * rl) + (PL - PR)) / (aR * rr - aL * rl)
            rsl, rsr = rl * aL / (S_L - S_M), rr * aR / (S_R - S_M)
            fanL = S_L >= 0.0
            fanR = ~fanL & (S_R <= 0.0)
            starL = ~fanL & ~fanR & (S_M >= 0.0)
            starR = ~fanL & ~fanR & ~starL
            out.update(fan_L=fanL, fan_R=fanR, star_L=starL, star_R=starR, rhoStarL_le_0=starL & ~(rsl > 0.0))
            F0 = np.where(fanL, ul * rl, np.where(fanR, ur * rr, np.where(starL, ul * rl + S_L * (rsl - rl), ur * rr + S_R * (rsr - rr))))
            out["S"] = (S_L, S_M, S_R)
        else:
            wl, wr = np.sqrt(rl), np.sqrt(rr)
            norm = 1.0 / (wl + wr)
            ut = (wl * ul + wr * ur) * norm
            dU = ul - ur
            if iso:
                cst = 0.5 * (csl + csr)
                G = 1.0
                cs_exp = np.ones_like(rl)
            else:
                vt = (wl * L[1 + AV] + wr * R[1 + AV]) * norm
                wt = (wl * L[1 + AW] + wr * R[1 + AW]) * norm
                EL = (PL / ((g - 1.0) * rl)) * rl + 0.5 * rl * (L[1] ** 2 + L[2] ** 2 + L[3] ** 2)
                ER = (PR / ((g - 1.0) * rr)) * rr + 0.5 * rr * (R[1] ** 2 + R[2] ** 2 + R[3] ** 2)
                Ht = (wl * ((EL + PL) / rl) + wr * ((ER + PR) / rr)) * norm
                EiL = rl * L[5] if reconstruct_eint else L[5]
                EiR = rr * R[5] if reconstruct_eint else R[5]
                kr = K_B / eos.units.kB
                Crho = 0.5 * (EiL / rl + EiR / rr)
                CP = 0.5 * ((EiL / rl) / ((PL / rl) * kr) + (EiR / rr) / ((PR / rr) * kr) + rl / ((g - 1.0) * rl) + rr / ((g - 1.0) * rr))
                cs_exp = Ht - 0.5 * (ut * ut + vt * vt + wt * wt) - Crho
                cst = np.where(cs_exp <= 0, 0.5 * (csl + csr), np.sqrt(np.abs(cs_exp) / CP))
                G = 0.5 * (1.0 + g)
            sN = 0.5 * G * np.maximum(dU, 0.0)
            S_L = np.minimum(ul - (csl + sN), ut - (cst + sN))
            S_R = np.maximum(ur + (csr + sN), ut + (cst + sN))
            cmax = np.maximum(csl, csr)
            tp = np.minimum(1.0, (cmax - np.minimum(du, 0.0)) / (cmax - np.minimum(dw, 0.0)))
            theta = tp ** 4
            S_s = (theta * (PR - PL) + (rl * ul * (S_L - ul) - rr * ur * (S_R - ur))) / (rl * (S_L - ul) - rr * (S_R - ur))
            vm = np.maximum(np.sqrt(L[1] ** 2 + L[2] ** 2 + L[3] ** 2), np.sqrt(R[1] ** 2 + R[2] ** 2 + R[3] ** 2))
            chi = np.minimum(1.0, vm / cmax)
            fanL = S_L > 0.0
            starL = ~fanL & (S_s > 0.0) & (S_L <= 0.0)
            starR = ~fanL & ~starL & (S_s <= 0.0) & (S_R >= 0.0)
            fanR = ~fanL & ~starL & ~starR
            out.update(fan_L=fanL, star_L=starL, star_R=starR, fan_R=fanR, cs_exp_le_0=(cs_exp <= 0) & (not iso), theta_lt_1=theta < 1.0, chi_lt_1=chi < 1.0)
            F0 = np.where(fanL, ul * rl, np.where(starL, S_s * (S_L * rl - ul * rl) / (S_L - S_s),
                                                   np.where(starR, S_s * (S_R * rr - ur * rr) / (S_R - S_s), ur * rr)))
            out["S"] = (S_L, S_s, S_R)
        F0 = F0 + viscosity * (rl - rr)
        out["mass_flux_ge_0"] = F0 >= 0.0
        out["mass_flux_lt_0"] = F0 < 0.0
    return out


def population(mask) -> tuple:
    return int(np.count_nonzero(mask)), float(np.count_nonzero(mask)) / mask.size


def holds(mask) -> bool:
    """the population condition"""
    n, share = population(mask)
    return n >= MIN_COUNT and share >= MIN_SHARE


@dataclass(frozen=True)
class FluxCase:
    """one launch of ComputeFluxes: what it fixes and the branches it targets (each must hold the population condition)"""
    id: str
    family: str
    units: str
    riemann: int = HLLC
    d: int = 0
    ndim: int = 3
    gamma: float = 1.4
    reconstruct_eint: bool = False
    K_visc: float = 0.0
    nscalars: int = 0
    seed: int = 1
    targets: tuple = ()

    @property
    def eos(self) -> Eos:
        return Eos(UNITS[self.units], self.gamma)

    def build(self):
        """(L, R, prim, vlo, vhi) of the case, deterministic"""
        eos = self.eos
        shape = face_shape(self.ndim, self.d)
        n = int(np.prod(shape))
        fs = face_states(eos, self.family, self.d, n, self.seed, self.nscalars)
        L, R = pack_face_states(eos, fs, self.reconstruct_eint, shape)
        cs = np.full(n, eos.units.cs_iso) if eos.isothermal else np.sqrt(self.gamma * fs["P"][0] / fs["rho"][0])
        prim = prim_velocities(self.ndim, self.d, 6 + self.nscalars, float(np.median(cs)), self.seed + 1000)
        vlo, vhi = face_box(self.ndim, self.d)
        return L, R, prim, vlo, vhi

    def classify(self, L, R, prim):
        du, dw, div = velocity_differences(prim, self.ndim, self.d)
        return classify_faces(self.eos, L, R, self.reconstruct_eint, self.ndim, self.d, du, dw, div, self.K_visc, self.riemann)


STAR = ("star_L", "star_R", "cs_exp_le_0", "theta_lt_1", "chi_lt_1", "mass_flux_ge_0", "mass_flux_lt_0")
FANS = ("fan_L", "fan_R", "star_L", "star_R", "mass_flux_ge_0", "mass_flux_lt_0")
ISO_STAR = ("star_L", "star_R", "theta_lt_1", "chi_lt_1")
HLLD_ALL = ("fan_L", "fan_R", "star_L", "star_R")


def flux_cases():
    """a case list, not the full product: the three solvers, directions 0 / 1 / 2, ndim 1 / 2 / 3, gamma-law and isothermal, reconstruct_eint on and
    off, K_visc 0 and 0.1, nscalars 0 and 2, code units and CGS; both families for each EOS and unit system"""
    c = []
    for units in ("code", "cgs"):
        c += [
            FluxCase(f"hllc-a-{units}-x", "a", units, d=0, seed=11, targets=STAR),
            FluxCase(f"hllc-b-{units}-x", "b", units, d=0, seed=12, targets=FANS),
            FluxCase(f"hllc-a-{units}-y-eint-visc-scal", "a", units, d=1, reconstruct_eint=True, K_visc=0.1, nscalars=2, seed=13, targets=STAR + ("viscosity",)),
            FluxCase(f"hllc-b-{units}-z-eint-visc-scal", "b", units, d=2, reconstruct_eint=True, K_visc=0.1, nscalars=2, seed=14, targets=FANS + ("viscosity",)),
            FluxCase(f"hllc-a-{units}-iso-y", "a", units, d=1, gamma=1.0, seed=15, targets=ISO_STAR),
            FluxCase(f"hllc-b-{units}-iso-z-visc-scal", "b", units, d=2, gamma=1.0, K_visc=0.1, nscalars=2, seed=16, targets=FANS + ("viscosity",)),
            FluxCase(f"llf-a-{units}-z-scal", "a", units, riemann=LLF, d=2, nscalars=2, K_visc=0.1, seed=17, targets=("mass_flux_ge_0", "mass_flux_lt_0", "viscosity")),
            FluxCase(f"hlld-a-{units}-y", "a", units, riemann=HLLD, d=1, seed=18, targets=("star_L", "star_R")),
            FluxCase(f"hlld-b-{units}-x-eint", "b", units, riemann=HLLD, d=0, reconstruct_eint=True, seed=19, targets=HLLD_ALL),
        ]
    c += [
        FluxCase("hllc-b-code-2d-x", "b", "code", d=0, ndim=2, seed=21, targets=FANS),
        FluxCase("hllc-a-cgs-2d-y-eint-visc-scal", "a", "cgs", d=1, ndim=2, reconstruct_eint=True, K_visc=0.1, nscalars=2, seed=22, targets=STAR + ("viscosity",)),
        FluxCase("hllc-b-cgs-1d-visc", "b", "cgs", d=0, ndim=1, K_visc=0.1, seed=23, targets=("fan_L", "fan_R", "mass_flux_ge_0", "mass_flux_lt_0", "viscosity")),
        FluxCase("hllc-a-code-1d-eint-scal", "a", "code", d=0, ndim=1, reconstruct_eint=True, nscalars=2, seed=24, targets=("star_L", "star_R", "cs_exp_le_0", "chi_lt_1")),
        FluxCase("hllc-a-code-g53-x", "a", "code", d=0, gamma=5.0 / 3.0, seed=25, targets=STAR),
        FluxCase("llf-b-code-iso-2d-y", "b", "code", riemann=LLF, d=1, ndim=2, gamma=1.0, seed=26, targets=("mass_flux_ge_0", "mass_flux_lt_0")),
    ]
    return c


# ------------------------------------------------------------------------------------------------ cell states of the update operators
CELL_BOX = ([0, 0, 0], [31, 30, 16])  # 32 x 31 x 17: odd extents, more than one workgroup
TWO_BOXES = [([0, 0, 0], [16, 4, 2]), ([17, 0, 0], [23, 4, 2])]  # 17 x 5 x 3 next to 7 x 5 x 3


def box_shape(lo, hi, ng=0, ndim=3, facedir=-1):
    return tuple(hi[a] - lo[a] + 1 + (2 * ng if a < ndim else 0) + (1 if a == facedir else 0) for a in (2, 1, 0))


def embed(valid, lo, hi, ng, ndim=3):
    """[ncomp, cells of the box in x-fastest order] -> the ghosted fab [ncomp, nz, ny, nx] with NaN in the ghost cells"""
    nc = valid.shape[0]
    fab = np.full((nc,) + box_shape(lo, hi, ng, ndim), np.nan)
    fab[interior(ng, ndim)] = valid.reshape((nc,) + box_shape(lo, hi))
    return fab


def interior(ng, ndim=3):
    return tuple([slice(None)] + [slice(ng, -ng) if (a < ndim and ng > 0) else slice(None) for a in (2, 1, 0)])


def ghost_mask(lo, hi, ng, ndim=3):
    m = np.ones(box_shape(lo, hi, ng, ndim), dtype=bool)
    m[interior(ng, ndim)[1:]] = False
    return m


def _base_cells(eos: Eos, rng, n, nscalars):
    """valid gas: rho and c_s over the unit system's ranges, Mach number log-uniform over 1e-3 .. 10, the auxiliary energy within 1 % of E - E_kin"""
    u = eos.units
    g = eos.gamma if not eos.isothermal else 5.0 / 3.0
    rho = _logu(rng, *u.rho, n)
    cs = _logu(rng, *u.cs, n)
    P = rho * cs * cs / g
    e = rng.standard_normal((3, n))
    e /= np.sqrt((e * e).sum(axis=0))
    v = _logu(rng, -3.0, 1.0, n) * cs * e
    U = np.zeros((6 + nscalars, n))
    U[0] = rho
    U[1:4] = rho * v
    Eint = P / (g - 1.0)
    U[4] = Eint + 0.5 * rho * (v * v).sum(axis=0)
    U[5] = Eint * (1.0 + 0.01 * rng.standard_normal(n))
    for s in range(nscalars):
        U[6 + s] = rho * rng.uniform(0.05, 1.0, n)
    return U


def _groups(rng, n, k):
    """a seeded assignment of n cells to k groups of (nearly) equal size"""
    return rng.permutation(np.arange(n) % k)


def limits_cells(eos: Eos, n: int, seed: int, nscalars: int, nmscalars: int, floor_zero: bool):
    """cells for EnforceLimits: (U [6 + nscalars, n], densityFloor, tempFloor).
    floor > 0: rho below / on / above the floor; the four combinations of the primitive and auxiliary temperature below / above the floor;
    E_tot - E_kin < 0; negative mass scalars; a mass-scalar sum of zero.
    floor == 0: negative rho (the scalar-zeroing branch), rho == 0 and 0 < rho <= DBL_MIN (which skip the temperature part), valid rho."""
    rng = np.random.default_rng(seed)
    u = eos.units
    U = _base_cells(eos, rng, n, nscalars)
    rho_floor = 0.0 if floor_zero else 10.0 ** (u.rho[0] + 0.3 * (u.rho[1] - u.rho[0]))  # 30 % of the cells lie below
    grp = _groups(rng, n, 12)
    if floor_zero:
        U[0] = np.where(grp == 0, -U[0], U[0])
        U[0] = np.where(grp == 1, 0.0, U[0])
        U[0] = np.where(grp == 2, DBL_MIN * rng.uniform(0.0, 1.0, n), U[0])  # subnormal or DBL_MIN itself below
        U[0] = np.where(grp == 3, DBL_MIN, U[0])
    else:
        U[0] = np.where(grp == 0, rho_floor, U[0])
    rho_new = np.maximum(U[0], rho_floor)
    ok = rho_new > DBL_MIN
    safe = np.where(ok, rho_new, 1.0)
    Ekin = 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / safe
    T_floor = 0.0
    if not eos.isothermal:
        # the floor temperature: the median of the cells' own temperatures, so that about half lie below
        T = eos.T_from_eint(safe, U[4] - Ekin)
        T_floor = float(np.median(T[ok]))
        E_floor = eos.eint_from_T(safe, T_floor)
        # groups 4..7: (prim below, aux below), (below, above), (above, below), (above, above), each a factor 2 .. 10 away from the floor
        for k, (pb, ab) in enumerate([(True, True), (True, False), (False, True), (False, False)]):
            m = (grp == 4 + k) & ok
            fp = rng.uniform(2.0, 10.0, n)
            fa = rng.uniform(2.0, 10.0, n)
            U[4] = np.where(m, Ekin + E_floor * (1.0 / fp if pb else fp), U[4])
            U[5] = np.where(m, E_floor * (1.0 / fa if ab else fa), U[5])
        m = (grp == 8) & ok
        U[4] = np.where(m, Ekin * rng.uniform(0.0, 0.99, n), U[4])  # E_tot - E_kin < 0: a negative primitive temperature
    if nmscalars > 0:
        m = grp == 9
        for s in range(nmscalars):
            U[6 + s] = np.where(m & (rng.random(n) < 0.6), -np.abs(U[6 + s]), U[6 + s])
        m = grp == 10
        for s in range(nmscalars):
            U[6 + s] = np.where(m, 0.0, U[6 + s])  # sum == 0 <= DBL_MIN: no renormalisation
        m = grp == 11
        for s in range(nmscalars):
            U[6 + s] = np.where(m, DBL_MIN / nmscalars if s == 0 else 0.0, U[6 + s])  # sum == DBL_MIN / nmscalars: on or under the threshold
    return U, rho_floor, T_floor


def classify_limits(eos: Eos, U, rho_floor, T_floor, nscalars, nmscalars):
    with np.errstate(all="ignore"):
        rho = U[0]
        rho_new = np.where(rho < rho_floor, rho_floor, rho)
        ok = (rho_new > DBL_MIN) & (not eos.isothermal)
        safe = np.where(rho_new > DBL_MIN, rho_new, 1.0)
        Ekin = 0.5 * safe * ((U[1] / safe) ** 2 + (U[2] / safe) ** 2 + (U[3] / safe) ** 2)
        out = {"rho_lt_floor": rho < rho_floor, "rho_eq_floor": rho == rho_floor, "rho_gt_floor": rho > rho_floor,
               "scalars_zeroed": (rho < rho_floor) & (rho_floor == 0.0) & (nscalars > 0), "rho_new_le_DBL_MIN": ~(rho_new > DBL_MIN)}
        if not eos.isothermal:
            Tp, Ta = eos.T_from_eint(safe, U[4] - Ekin), eos.T_from_eint(safe, U[5])
            pb, ab = Tp < T_floor, Ta < T_floor
            out.update(prim_below_aux_below=ok & pb & ab, prim_below_aux_above=ok & pb & ~ab, prim_above_aux_below=ok & ~pb & ab,
                       prim_above_aux_above=ok & ~pb & ~ab, thermal_lt_0=ok & (U[4] - Ekin < 0.0))
        if nmscalars > 0:
            ms = U[6:6 + nmscalars]
            fixed = np.where(ms < 0.0, SMALL_X * rho_new, ms)
            out.update(mass_scalar_negative=(ms < 0.0).any(axis=0), mass_sum_le_DBL_MIN=~(fixed.sum(axis=0) > DBL_MIN),
                       mass_renormalised=(fixed.sum(axis=0) > DBL_MIN) & (rho_new > DBL_MIN))
    return out


def dual_energy_cells(eos: Eos, n: int, seed: int, nscalars: int = 0):
    """cells for SyncDualEnergy: the switch E_int,cons > eta E_tot on both sides (kinetic-dominated cells whose thermal part is 1e-5 .. 1e-2 of the
    total), the exact tie of gas at rest with E_tot = 0, negative E_tot, rho == 0 and rho < 0 (fatal in the reference)"""
    rng = np.random.default_rng(seed)
    U = _base_cells(eos, rng, n, nscalars)
    grp = _groups(rng, n, 8)
    Ekin = 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / U[0]
    m = (grp == 0) | (grp == 1)
    U[4] = np.where(m, Ekin * (1.0 + _logu(rng, -5.0, -2.0, n)), U[4])  # E_int,cons / E_tot between 1e-5 and 1e-2: both sides of eta = 1e-3
    m = grp == 2
    U[1:4] = np.where(m, 0.0, U[1:4])
    U[4] = np.where(m, 0.0, U[4])  # E_int,cons = 0 = eta E_tot: the tie takes the auxiliary branch
    m = grp == 3
    U[4] = np.where(m, -np.abs(U[4]), U[4])
    U[0] = np.where(grp == 4, 0.0, U[0])
    U[0] = np.where(grp == 5, -U[0], U[0])
    return U


def classify_dual_energy(U):
    with np.errstate(all="ignore"):
        fatal = U[0] <= 0.0
        Ekin = (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / (2.0 * np.where(fatal, 1.0, U[0]))
        Ec = U[4] - Ekin
        return {"fatal_rho_le_0": fatal, "use_conserved": ~fatal & (Ec > ETA_DUAL * U[4]), "use_auxiliary": ~fatal & ~(Ec > ETA_DUAL * U[4]),
                "tie": ~fatal & (Ec == ETA_DUAL * U[4]), "Etot_lt_0": ~fatal & (U[4] < 0.0)}


def signal_cells(eos: Eos, n: int, seed: int, nan_cells: bool = True):
    """cells for the signal speed: gas at rest (sqrt(0)), and — gamma law — cells with E - E_kin < 0 whose signal speed is NaN and must not win the
    maximum, placed first, last and in the middle of the box; every other cell valid"""
    rng = np.random.default_rng(seed)
    U = _base_cells(eos, rng, n, 0)
    grp = _groups(rng, n, 8)
    U[1:4] = np.where(grp == 0, 0.0, U[1:4])
    U[4] = np.where(grp == 0, U[5], U[4])
    if nan_cells and not eos.isothermal:
        Ekin = 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / U[0]
        m = grp == 1
        m[[0, n // 2, n - 1]] = True
        m[1] = False  # (at least one valid cell right next to the first)
        U[4] = np.where(m, 0.5 * Ekin - 1e-3 * U[5], U[4])
    return U


def classify_signal(eos: Eos, U):
    with np.errstate(all="ignore"):
        Ekin = 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / U[0]
        return {"at_rest": (U[1] == 0) & (U[2] == 0) & (U[3] == 0), "thermal_lt_0": (U[4] - Ekin < 0.0) & (not eos.isothermal)}


def predict_cells(eos: Eos, n: int, seed: int, nscalars: int, nmscalars: int):
    """(U_old [6 + nscalars, n], rhs, dt) for PredictStep: the new density exactly 0 (dt = 1 / 2 and rhs = -2 rho, both products exact), negative,
    NaN, a negative new mass scalar, and valid cells"""
    rng = np.random.default_rng(seed)
    U = _base_cells(eos, rng, n, nscalars)
    dt = 0.5
    rhs = U * rng.uniform(-0.5, 0.5, U.shape)
    grp = _groups(rng, n, 8)
    rhs[0] = np.where(grp == 0, -2.0 * U[0], rhs[0])
    rhs[0] = np.where(grp == 1, -2.0 * U[0] * rng.uniform(1.01, 3.0, n), rhs[0])
    rhs[0] = np.where(grp == 2, np.nan, rhs[0])
    for s in range(nmscalars):
        rhs[6 + s] = np.where((grp == 3) & (rng.random(n) < 0.7), -2.0 * U[6 + s] * rng.uniform(1.01, 3.0, n), rhs[6 + s])
    return U, rhs, dt


def classify_predict(U, rhs, dt, nmscalars):
    with np.errstate(all="ignore"):
        new = U + dt * rhs
        out = {"rho_eq_0": new[0] == 0.0, "rho_lt_0": new[0] < 0.0, "rho_nan": np.isnan(new[0]), "valid": new[0] > 0.0}
        if nmscalars > 0:
            neg = (new[6:6 + nmscalars] < 0.0).any(axis=0)
            out["mass_scalar_negative"] = neg & (new[0] > 0.0)
            out["valid"] = out["valid"] & ~neg
        return out


# ------------------------------------------------------------------------------------------------ np.longdouble restatement of the cell operators
# Each returns (value, bound): the statement of hydro_system.hpp evaluated in extended precision, and the per-cell bound
# (roundings in the float64 formula + 1) x eps x the largest intermediate magnitude.
LD = np.longdouble


def ld_enforce_limits(eos: Eos, U, rho_floor, T_floor, nscalars, nmscalars):
    """hydro_system.hpp:696-773.  Branches are taken on the float64 predicates of classify_limits (cells whose predicate could flip within the bound
    are the caller's to exclude); returns (state, bound) for rho, E, E_int and the scalars."""
    with np.errstate(all="ignore"):
        c = classify_limits(eos, U, rho_floor, T_floor, nscalars, nmscalars)
        out = U.astype(LD)
        mag = np.abs(U).astype(LD)
        lo = c["rho_lt_floor"]
        rho_new = np.where(lo, LD(rho_floor), out[0])
        out[0] = rho_new
        for s in range(nscalars):  # :713-722: 2 roundings (rho / rho_new, the product)
            q = out[6 + s]
            out[6 + s] = np.where(lo, LD(0.0) if rho_floor == 0.0 else q * (U[0].astype(LD) / rho_new), q)
        if nmscalars > 0:  # :725-744: up to nmscalars - 1 sums, the quotient by rho, the quotient of each scalar: nmscalars + 2 roundings
            ms = out[6:6 + nmscalars]
            ms = np.where(ms < 0, LD(SMALL_X) * rho_new, ms)
            sp = ms.sum(axis=0)
            out[6:6 + nmscalars] = np.where(c["mass_renormalised"], ms / (sp / np.where(rho_new == 0, LD(1), rho_new)), ms)
        # (a rounding that lands in the subnormal range — the scalars of the DBL_MIN group — errs by up to half the subnormal spacing instead)
        bound = (3 + nmscalars + 1) * (EPS * np.abs(out) + float(np.finfo(np.float64).smallest_subnormal))
        if not eos.isothermal:
            ok = rho_new > DBL_MIN
            safe = np.where(ok, rho_new, LD(1))
            Ekin = LD(0.5) * safe * ((out[1] / safe) ** 2 + (out[2] / safe) ** 2 + (out[3] / safe) ** 2)
            Ef = eos.eint_from_T(safe, LD(T_floor))
            pb = c["prim_below_aux_below"] | c["prim_below_aux_above"]
            ab = c["prim_below_aux_below"] | c["prim_above_aux_below"]
            # E = Ekin + E_floor: Ekin 9 roundings (3 quotients, 3 squares, 2 sums, 2 products - the product by 0.5 is exact), E_floor 8
            # (ComputeEintFromTgas: 3 in p, 2 in e, 3 after), the sum 1: 18, + 1
            out[4] = np.where(ok & pb, Ekin + Ef, out[4])
            out[5] = np.where(ok & ab, Ef, out[5])
            bound[4] = np.where(ok & pb, 19 * EPS * (np.abs(Ekin) + np.abs(Ef)), 0.0)
            bound[5] = np.where(ok & ab, 9 * EPS * np.abs(Ef), 0.0)
        bound[0:4] = 0.0
        return out, bound


def ld_sync_dual_energy(U):
    """hydro_system.hpp:816-850 on the non-fatal cells: (E, E_int) and their bounds.  E_kin: 3 squares, 2 sums, the product 2 rho (exact), the
    quotient: 6 roundings; E_int,cons = E - E_kin one more: 8 eps max(|E|, E_kin); E = E_int,aux + E_kin: 8 eps (|E_int,aux| + E_kin)."""
    with np.errstate(all="ignore"):
        c = classify_dual_energy(U)
        V = U.astype(LD)
        Ekin = (V[1] ** 2 + V[2] ** 2 + V[3] ** 2) / (LD(2) * np.where(c["fatal_rho_le_0"], LD(1), V[0]))
        E = np.where(c["use_conserved"], V[4], V[5] + Ekin)
        Ei = np.where(c["use_conserved"], V[4] - Ekin, V[5])
        bE = np.where(c["use_conserved"], 0.0, 8 * EPS * (np.abs(V[5]) + Ekin))
        bEi = np.where(c["use_conserved"], 8 * EPS * np.maximum(np.abs(V[4]), Ekin), 0.0)
        E = np.where(c["fatal_rho_le_0"], V[4], E)
        Ei = np.where(c["fatal_rho_le_0"], V[5], Ei)
        # how far the switch is from flipping: |E_int,cons - eta E| against the rounding of its two sides
        margin = np.abs((V[4] - Ekin) - LD(ETA_DUAL) * V[4]) - 9 * EPS * np.maximum(np.abs(V[4]), Ekin)
        return E, Ei, bE, bEi, margin > 0


def ld_signal_speed(eos: Eos, U, which: int):
    """hydro_system.hpp:198-252: c_s + |v|.  gamma law: E_kin 9 roundings, E - E_kin 1, P = (gamma - 1) rho (E_th / rho) 3, gamma P / rho 2, the
    root 1: 16 on c_s^2 = gamma (gamma - 1) E_th / rho, whose cancellation is relative to max(|E|, E_kin); |v| 7 roundings; the sum 1."""
    with np.errstate(all="ignore"):
        V = U.astype(LD)
        rho = V[0]
        v2 = (V[1] / rho) ** 2 + (V[2] / rho) ** 2 + (V[3] / rho) ** 2
        vmag = np.sqrt(v2)
        if eos.isothermal:
            cs = np.full_like(vmag, LD(eos.units.cs_iso))
            bcs = np.zeros(cs.shape)
        else:
            g = LD(eos.gamma)
            Ekin = LD(0.5) * rho * v2
            Eth = V[4] - Ekin
            cs2 = g * (g - 1) * Eth / rho
            cs = np.sqrt(cs2)
            # d(c_s) = d(c_s^2) / (2 c_s): the absolute error of c_s^2 is 17 eps gamma (gamma - 1) max(|E|, E_kin) / rho
            bcs = 17 * EPS * (g * (g - 1) * np.maximum(np.abs(V[4]), Ekin) / rho) / (2 * cs) + EPS * cs
        return cs + vmag, (bcs + 9 * EPS * vmag + EPS * (cs + vmag)).astype(np.float64)


def ld_predict_step(U, rhs, dt):
    """hydro_system.hpp:475-497: U + dt rhs, 2 roundings: 3 eps (|U| + |dt rhs|)"""
    with np.errstate(all="ignore"):
        return U.astype(LD) + LD(dt) * rhs.astype(LD), 3 * EPS * (np.abs(U) + np.abs(dt * rhs))


def ld_rhs_from_fluxes(fluxes, dx, ndim):
    """hydro_system.hpp:448-473: sum over d of (1 / dx_d) (F_d(i) - F_d(i + 1)): per direction the reciprocal, the difference, the product, and
    ndim - 1 sums: 4 ndim roundings, + 1, times the sum of the terms' magnitudes"""
    val, mag = 0, 0
    for d in range(ndim):
        F = fluxes[d].astype(LD)
        ax = 3 - d
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        val = val + (LD(1) / LD(dx[d])) * (F[tuple(lo)] - F[tuple(hi)])
        mag = mag + (np.abs(F[tuple(lo)]) + np.abs(F[tuple(hi)])) / LD(dx[d])
    return val, ((4 * ndim + 1) * EPS * mag).astype(np.float64)


def ld_add_pdv(eos: Eos, rhs5, Ug, vels, redo, dx, ndim, ng):
    """hydro_system.hpp:775-814 on the valid cells: rhs5 - P div(v); P as ComputePressure (13 roundings, relative to max(|E|, E_kin) (gamma - 1)),
    div(v) 3 ndim roundings (face velocities) or 5 ndim + 1 (cell velocities), the product and the sum: 13 + 5 ndim + 4, times
    (|rhs5| + Pmag sum |v terms| / dx)"""
    with np.errstate(all="ignore"):
        V = Ug.astype(LD)
        inn = interior(ng, ndim)
        C = V[inn]
        rho = C[0]
        if eos.isothermal:
            P = rho * LD(eos.units.cs_iso) * LD(eos.units.cs_iso)
            Pmag = np.abs(P)
        else:
            Ekin = LD(0.5) * rho * ((C[1] / rho) ** 2 + (C[2] / rho) ** 2 + (C[3] / rho) ** 2)
            P = LD(eos.gamma - 1.0) * (C[4] - Ekin)
            Pmag = LD(eos.gamma - 1.0) * np.maximum(np.abs(C[4]), Ekin)
        div_f, div_c, mag_f, mag_c = 0, 0, 0, 0
        for d in range(ndim):
            ax = 2 - d
            v = vels[d].astype(LD)
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            div_f = div_f + (v[tuple(hi)] - v[tuple(lo)]) / LD(dx[d])
            mag_f = mag_f + (np.abs(v[tuple(hi)]) + np.abs(v[tuple(lo)])) / LD(dx[d])
            vel = V[1 + d] / V[0]
            sp = [slice(None)] + [slice(ng, -ng) if a < ndim else slice(None) for a in (2, 1, 0)]
            p, m = list(sp[1:]), list(sp[1:])
            p[ax], m[ax] = slice(ng + 1, vel.shape[ax] - ng + 1), slice(ng - 1, -ng - 1)
            div_c = div_c + (vel[tuple(p)] - vel[tuple(m)]) / LD(dx[d])
            mag_c = mag_c + (np.abs(vel[tuple(p)]) + np.abs(vel[tuple(m)])) / LD(dx[d])
        div = np.where(redo == 0, div_f, LD(0.5) * div_c)
        mag = np.where(redo == 0, mag_f, LD(0.5) * mag_c)
        val = rhs5.astype(LD) - P * div
        return val, ((13 + 5 * ndim + 4 + 1) * EPS * (np.abs(rhs5) + Pmag * mag)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the physical flux of one side
def physical_flux(eos: Eos, q, other, reconstruct_eint: bool, ndim: int, d: int, left: bool):
    """F = u U + P D of the packed state q (hydro_system.hpp:881-1003, HLLC.hpp:116-133) in float64 with the reference's association, in ARRAY
    component order, after the steps ComputeFluxes applies to every flux with K_visc = 0 (:1076-1091); `other` is the state of the other side
    (the face velocity divides by its density when the mass flux has the matching sign).  Returns (flux [nvar, ...], face velocity)."""
    AN, AV, AW = axes(ndim, d)
    g = eos.gamma
    rho, vx, vy, vz = q[0], q[1], q[2], q[3]
    P = face_pressure(eos, q, reconstruct_eint)
    u, v, w = q[1 + AN], q[1 + AV], q[1 + AW]
    if eos.isothermal:
        E = Eint = np.full_like(rho, np.nan)
    else:
        ke = 0.5 * rho * (vx * vx + vy * vy + vz * vz)
        E = (P / ((g - 1.0) * rho)) * rho + ke
        Eint = rho * q[5] if reconstruct_eint else q[5]
    U = [rho, rho * u, rho * v, rho * w, E, Eint] + [q[6 + s] for s in range(q.shape[0] - 6)]
    D = [0.0, 1.0, 0.0, 0.0, u, 0.0] + [0.0] * (q.shape[0] - 6)
    Fc = [u * U[n] + P * D[n] for n in range(len(U))]
    F = np.empty_like(q)
    for n in (0, 4, 5):
        F[n] = Fc[n] + 0.0  # (the viscosity term of K_visc = 0: + 0 (U_L - U_R))
    for s in range(q.shape[0] - 6):
        F[6 + s] = Fc[6 + s] + 0.0
    F[1 + AN], F[1 + AV], F[1 + AW] = Fc[1], Fc[2], Fc[3]
    if eos.isothermal:
        F[4] = 0.0
        F[5] = 0.0
    rho_L, rho_R = (q[0], other[0]) if left else (other[0], q[0])
    return F, np.where(F[0] >= 0.0, F[0] / rho_R, F[0] / rho_L)


# ------------------------------------------------------------------------------------------------ the cell-operator cases and what each targets
CELL_EOS = [("code", 1.4), ("cgs", 5.0 / 3.0), ("cgs", 1.0)]  # (unit system, gamma); gamma == 1: isothermal
NSCAL, NMSCAL = 3, 2  # three passive scalars, the first two of them partial densities


def limits_targets(eos: Eos, floor_zero: bool):
    if floor_zero:
        return ["scalars_zeroed", "rho_new_le_DBL_MIN", "rho_gt_floor"]
    want = ["rho_lt_floor", "rho_eq_floor", "rho_gt_floor", "mass_scalar_negative", "mass_sum_le_DBL_MIN", "mass_renormalised"]
    if not eos.isothermal:
        want += ["prim_below_aux_below", "prim_below_aux_above", "prim_above_aux_below", "prim_above_aux_above", "thermal_lt_0"]
    return want


DUAL_TARGETS = ["fatal_rho_le_0", "use_conserved", "use_auxiliary", "tie", "Etot_lt_0"]
PREDICT_TARGETS = ["rho_eq_0", "rho_lt_0", "rho_nan", "mass_scalar_negative", "valid"]


def signal_targets(eos: Eos):
    return ["at_rest"] + ([] if eos.isothermal else ["thermal_lt_0"])


def assert_populations(what: str, classes, targets):
    for k in targets:
        assert holds(classes[k]), (what, k, population(classes[k]))


# ------------------------------------------------------------------------------------------------ a whole state that takes the fans
def fan_state(base, gamma: float = 1.4, amplitude: float = 6.0):
    """`base` (a conserved gamma-law state [6, nz, ny, nx] with sound speeds of 1 .. 3, such as random_state of tests/test_hydro_ops_gpu.py) plus a
    smooth periodic bulk velocity of `amplitude` whose direction rotates across the domain, (cos a, sin a cos b, sin a sin b) with
    a = 2 pi (i / nx + k / nz) and b = 2 pi j / ny: along every axis the normal velocity passes through both supersonic ranges and through zero,
    so all four fans of the Riemann solver occur in every direction.  Thermal and auxiliary internal energy are kept."""
    nz, ny, nx = base.shape[1:]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    a, b = 2.0 * np.pi * (i / nx + k / nz), 2.0 * np.pi * j / ny
    bulk = amplitude * np.stack([np.cos(a), np.sin(a) * np.cos(b), np.sin(a) * np.sin(b)])
    rho = base[0]
    v = base[1:4] / rho
    thermal = base[4] - 0.5 * rho * (v * v).sum(axis=0)
    v = v + bulk
    U = base.copy()
    U[1:4] = rho * v
    U[4] = thermal + 0.5 * rho * (v * v).sum(axis=0)
    return U


def periodic_pad(U, ng: int):
    """[ncomp, nz, ny, nx] -> the same grown by ng periodic images in every direction"""
    idx = [np.arange(-ng, n + ng) % n for n in U.shape[1:]]
    return np.ascontiguousarray(U[:, idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]])


def donor_cell_faces(prim, d: int, ng: int):
    """the piecewise-constant face states of direction d on the face box of the valid box (hyperbolic_system.hpp ReconstructStatesConstant):
    L = q(i - 1), R = q(i); prim is ghosted by ng >= 1 in all three directions"""
    def cut(shift):
        sl = [slice(None)]
        for a in (2, 1, 0):
            n = prim.shape[3 - a] - 2 * ng + (1 if a == d else 0)
            s0 = ng + (shift if a == d else 0)
            sl.append(slice(s0, s0 + n))
        return np.ascontiguousarray(prim[tuple(sl)])
    return cut(-1), cut(0)
