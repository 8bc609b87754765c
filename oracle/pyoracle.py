"""ORACLE — TEST INFRASTRUCTURE ONLY.

ctypes/numpy binding of oracle/liboracle.so (the CPU restatement of the reference algorithm).
Only tests/, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import this.
Arrays are Fortran-order with the component index outermost (amrex::Array4 layout), i.e. a numpy
array of shape (ncomp, nz, ny, nx) in C order.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

K_B = 1.380649e-16
M_U = 1.6605390666e-24

SOD, CONTACT, SEDOV, SHELL, RADSHOCK, STREAMING, SCALARS, HYDRO1D, COUPLING, SUOLSON, ADVECTING, MARSHAK, RADFORCE, MARSHAK_ASYMPTOTIC, RADPULSE, SHOCKTUBE_CMA = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15
# multigroup radiation (oracle/problems_multigroup.hpp); PULSE_MG = the advecting 4-group run, PULSE_MG_GREY = the static grey run of the same file
RADSHOCK_MG, RADTUBE, MARSHAK_VAYTET, PULSE_MG, PULSE_MG_GREY, RADDUST = 16, 17, 18, 19, 20, 21
QUIRK = 22  # HydroQuirk: the 2-D (or 3-D) odd-even decoupling test
RADDUST_MG = 24  # RadDustMG: the same relaxation with 4 photon groups (multigroup dust exchange)
LINE_COOLING = 26  # RadLineCooling: one group, line cooling linear in T + cosmic-ray heating (dust_coeff = the deck's coefficient)
LINE_COOLING_MG = 27  # RadLineCoolingMG: four groups + photoelectric heating by the last group
MARSHAK_DUST_PE = 28  # RadMarshakDustPE: FUV front heating the gas photoelectrically
STREAMING_Y = 29  # RadStreamingY: the streaming front along y in a 2-D build
ADVECTION_SAWTOOTH, ADVECTION_SEMIELLIPSE, ADVECTION_SQUARE_2D = 31, 32, 33  # linear advection of a scalar (AdvectionSimulation)
GENERAL_OPACITY = 30  # kappa = kappa0 rho^0.3 T^-1.7 (no reference problem: the pin of the compiled opacity hooks of the C++ host)
MARSHAK_DUST = 25  # RadMarshakDust: two groups (IR / FUV), dust model with the decoupled branch
BLAST2D = 23  # HydroBlast2D: circular blast in a reflecting box, as a 2-D build or as a 3-D build uniform in z
# OpacityModel (radiation_system.hpp:64-71)
PIECEWISE_CONSTANT, PPL_FIXED_SLOPE, PPL_FULL_SPECTRUM = 1, 2, 3


def build(force: bool = False) -> None:
    """Compile the oracle with gcc (seconds)."""
    lib = os.path.join(_HERE, "liboracle.so")
    if force or not os.path.exists(lib):
        subprocess.check_call(["make", "-C", _HERE, "-s"] + (["-B"] if force else []))


class HydroTraits(C.Structure):
    _fields_ = [
        ("gamma", C.c_double),
        ("cs_isothermal", C.c_double),
        ("mean_molecular_weight", C.c_double),
        ("boltzmann_constant", C.c_double),
        ("reconstruct_eint", C.c_int),
        ("nscalars", C.c_int),
        ("ndim", C.c_int),
    ]


def traits(gamma=1.4, reconstruct_eint=True, ndim=3, nscalars=0, mean_molecular_weight=M_U, boltzmann_constant=K_B,
           cs_isothermal=float("nan")) -> HydroTraits:
    return HydroTraits(gamma, cs_isothermal, mean_molecular_weight, boltzmann_constant, int(reconstruct_eint), nscalars, ndim)


class RadCellTraits(C.Structure):
    """orc_rad_cell_traits: what the matter-radiation exchange reads of qk_rad_traits / qk_hydro_traits (gamma == 1: isothermal)"""
    _fields_ = [("c_light", C.c_double), ("c_hat", C.c_double), ("radiation_constant", C.c_double), ("Erad_floor", C.c_double),
                ("kappaP", C.c_double), ("kappaE", C.c_double), ("kappaF", C.c_double),
                ("opacity_T_ref", C.c_double), ("opacity_T_exponent", C.c_double), ("opacity_pow_floor", C.c_double),
                ("gamma", C.c_double), ("mean_molecular_weight", C.c_double), ("boltzmann_constant", C.c_double),
                ("beta_order", C.c_int), ("opacity_model", C.c_int), ("pow_mode", C.c_int), ("eddington_model", C.c_int)]


class RadMGCellTraits(C.Structure):
    """orc_rad_mg_cell_traits: what the multigroup matter-radiation exchange reads of qk_rad_traits / qk_hydro_traits (gamma == 1: isothermal)"""
    _fields_ = [("c_light", C.c_double), ("c_hat", C.c_double), ("radiation_constant", C.c_double), ("Erad_floor", C.c_double),
                ("energy_unit", C.c_double),
                ("rad_boundaries", C.c_double * 9), ("mg_kappa_exponent", C.c_double * 9), ("mg_kappa_lower", C.c_double * 9),
                ("mg_kappa_rho_exponent", C.c_double), ("mg_kappa_T_ref", C.c_double), ("mg_kappa_T_exponent", C.c_double),
                ("dust_gas_interaction_coeff", C.c_double), ("gas_dust_coupling_threshold", C.c_double),
                ("cooling_linear_coeff", C.c_double * 8), ("cr_heating_rate", C.c_double), ("pe_heating_E1_derivative", C.c_double),
                ("gamma", C.c_double), ("mean_molecular_weight", C.c_double), ("boltzmann_constant", C.c_double),
                ("beta_order", C.c_int), ("eddington_model", C.c_int), ("pow_mode", C.c_int), ("ngroups", C.c_int), ("mg_opacity_model", C.c_int),
                ("enable_dust_gas_thermal_coupling_model", C.c_int), ("thermal_model", C.c_int), ("enable_photoelectric_heating", C.c_int)]


# the bits of the branch mask orc_rad_mg_source_cells records per cell (oracle/radiation_multigroup.hpp, diag::Branch)
MG_BRANCHES = ("zero_tau", "dE_constrain", "denom_le_0", "alpha_gt_100", "alpha_lt_m100", "alpha_near_0", "slope_zero_mean", "slope_sign_change",
               "slopes_frozen", "floor_clamp", "x_ge_100", "below_table", "decoupled", "negative_dust_T")
MG_BRANCH_BIT = {name: 1 << i for i, name in enumerate(MG_BRANCHES)}

# the bits orc_rad_face_fluxes / orc_rad_transport_stage record per face and per cell (oracle/radiation.hpp, tdiag::Face / tdiag::Cell)
RAD_FACE_BRANCHES = ("fallback", "erad_L_le_0", "erad_R_le_0", "f_L_ge_1", "f_R_ge_1", "clamp_L", "clamp_R", "no_dir_L", "no_dir_R", "S_floor_L", "S_floor_R",
                     "nonfinite")
RAD_FACE_BIT = {name: 1 << i for i, name in enumerate(RAD_FACE_BRANCHES)}
RAD_CELL_BRANCHES = ("invalid_E", "invalid_f", "f_nan", "lifted", "rescaled", "by_other")
RAD_CELL_BIT = {name: 1 << i for i, name in enumerate(RAD_CELL_BRANCHES)}


class SimConfig(C.Structure):
    _fields_ = [
        ("problem", C.c_int),
        ("ndim", C.c_int),
        ("n_cell", C.c_int * 3),
        ("max_grid_size", C.c_int * 3),
        ("prob_lo", C.c_double * 3),
        ("prob_hi", C.c_double * 3),
        ("periodic", C.c_int * 3),
        ("cfl", C.c_double),
        ("stop_time", C.c_double),
        ("max_timesteps", C.c_long),
        ("reconstruction_order", C.c_int),
        ("nscalars", C.c_int),
        ("table_len", C.c_int),
        ("table_r", C.POINTER(C.c_double)),
        ("table_Erad", C.POINTER(C.c_double)),
        ("table_Frad", C.POINTER(C.c_double)),
        ("rad_pow_mode", C.c_int),
        ("h1d", C.c_double * 12),
        ("h1d_i", C.c_int * 2),
        ("table_extra", C.POINTER(C.c_double)),
        ("opacity_model", C.c_int),
    ]


_I3 = C.c_int * 3


def _i3(v):
    return _I3(*[int(x) for x in v])


def _dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


def usable_cores() -> int:
    """threads worth using: the affinity mask, capped by twice the cgroup CPU quota (the GPU boxes show 256 CPUs and grant 16)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(round(2 * float(quota) / float(period)))))
    except (OSError, ValueError):
        pass
    if "OMP_NUM_THREADS" in os.environ:
        n = int(os.environ["OMP_NUM_THREADS"])
    return n


class Oracle:
    def __init__(self, variant: str = "direct"):
        build()
        name = "liboracle.so" if variant == "direct" else "liboracle_eosT.so"
        self.lib = C.CDLL(os.path.join(_HERE, name))
        L = self.lib
        L.orc_sim_create.restype = C.c_void_p
        L.orc_sim_create.argtypes = [C.POINTER(SimConfig)]
        for f in ("orc_sim_destroy",):
            getattr(L, f).argtypes = [C.c_void_p]
        for f in ("orc_sim_nboxes", "orc_sim_ncomp", "orc_sim_nghost", "orc_sim_step", "orc_sim_evolve"):
            getattr(L, f).argtypes = [C.c_void_p]
            getattr(L, f).restype = C.c_int
        for f in ("orc_sim_time", "orc_sim_dt", "orc_sim_compute_dt"):
            getattr(L, f).argtypes = [C.c_void_p]
            getattr(L, f).restype = C.c_double
        for f in ("orc_sim_istep", "orc_sim_cell_updates"):
            getattr(L, f).argtypes = [C.c_void_p]
            getattr(L, f).restype = C.c_long
        L.orc_sim_box.argtypes = [C.c_void_p, C.c_int, _I3, _I3]
        L.orc_sim_get_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.orc_sim_set_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.orc_sim_fill_ghosts.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.orc_sim_counters.argtypes = [C.c_void_p, C.c_long * 3]
        L.orc_sim_advance_fixed_dt.argtypes = [C.c_void_p, C.c_double]
        L.orc_sim_advance_fixed_dt.restype = C.c_int
        L.orc_eos_variant.restype = C.c_int
        L.orc_sim_rad_counters.argtypes = [C.c_void_p, C.c_long * 8]
        L.orc_sim_tag_relative_gradient.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
        L.orc_sim_tag_centered_gradient.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
        L.orc_sim_rad_source.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double)]
        L.orc_sim_rad_transport_only.argtypes = [C.c_void_p, C.c_double]
        D, DP = C.c_double, C.POINTER(C.c_double)
        L.orc_planck_integral.argtypes, L.orc_planck_integral.restype = [D], D
        L.orc_planck_table_entry.argtypes, L.orc_planck_table_entry.restype = [C.c_int], D
        L.orc_planck_fractions.argtypes = [C.c_int, DP, D, D, D, D, D, DP, DP]
        L.orc_planck_function.argtypes, L.orc_planck_function.restype = [D, D, D, D, D], D
        L.orc_group_mean_opacity.argtypes = [C.c_int, DP, DP, DP, DP, DP]
        L.orc_rad_quantity_exponents.argtypes = [C.c_int, DP, DP, DP]

    # ---------------------------------------------------------------- the matter-radiation exchange, cell by cell
    def rad_source_cells(self, t: RadCellTraits, U: np.ndarray, src: np.ndarray, dt_radiation: float, stage: int):
        """AddSourceTermsSingleGroup on every cell of U[10, n] as a box of its own.  Returns (U after, record, totals): record is a dict of int32
        arrays over the cells — solves, newton (iterations summed over the solves, n + 1 each), newton_max, fail_newton, fail_outer —, totals
        the counters in the layout of the C-ABI: iteration counter [0..3], failure counter [0..2]"""
        U = np.ascontiguousarray(U, dtype=np.float64).copy()
        src = np.ascontiguousarray(src, dtype=np.float64)
        n = U.shape[1]
        assert U.shape == (10, n) and src.shape == (n,)
        rec = np.zeros((5, n), dtype=np.int32)
        tot = (C.c_long * 7)()
        f = self.lib.orc_rad_source_cells
        f.argtypes = [C.POINTER(RadCellTraits), C.c_long, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(C.c_int),
                      C.POINTER(C.c_long)]
        f.restype = None
        self.lib.orc_set_num_threads(int(max(1, min(usable_cores(), n // 512))))
        f(C.byref(t), n, _dp(U), _dp(src), float(dt_radiation), int(stage), rec.ctypes.data_as(C.POINTER(C.c_int)), tot)
        keys = ("solves", "newton", "newton_max", "fail_newton", "fail_outer")
        return U, dict(zip(keys, rec)), [int(v) for v in tot]

    def set_libm_jitter(self, seed: int, ulps: int = 0):
        """seed 0: libm as it is.  Otherwise pow / exp / log / log10 of the multigroup path move by up to `ulps` ulps, chosen by a hash of
        (seed, function, argument bits).  Process-wide: reset to 0 after use."""
        self.lib.orc_set_libm_jitter.argtypes = [C.c_ulonglong, C.c_int]
        self.lib.orc_set_libm_jitter.restype = None
        self.lib.orc_set_libm_jitter(int(seed), int(ulps))

    def rad_mg_source_cells(self, t: RadMGCellTraits, U: np.ndarray, src: np.ndarray, dt_radiation: float, stage: int, jitter_seed: int = 0,
                            jitter_ulps: int = 0):
        """AddSourceTermsMultiGroup on every cell of U[6 + 4 ng, n] as a box of its own; src[ng, n].  Returns (U after, record, totals): record is
        a dict of int32 arrays over the cells — solves, newton (n + 1 summed over the solves), newton_max, fail_newton, fail_outer, fail_dust,
        decoupled, mask (MG_BRANCH_BIT) —, totals the counters in the layout of the C-ABI: iteration counter [0..3], failure counter [0..2]"""
        ng = int(t.ngroups)
        U = np.ascontiguousarray(U, dtype=np.float64).copy()
        src = np.ascontiguousarray(src, dtype=np.float64)
        n = U.shape[1]
        assert 2 <= ng <= 8 and U.shape == (6 + 4 * ng, n) and src.shape == (ng, n)
        rec = np.zeros((8, n), dtype=np.int32)
        tot = (C.c_long * 7)()
        f = self.lib.orc_rad_mg_source_cells
        f.argtypes = [C.POINTER(RadMGCellTraits), C.c_long, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(C.c_int),
                      C.POINTER(C.c_long)]
        f.restype = None
        self.lib.orc_set_num_threads(int(max(1, min(usable_cores(), n // 128))))
        self.set_libm_jitter(jitter_seed, jitter_ulps)
        try:
            f(C.byref(t), n, _dp(U), _dp(src), float(dt_radiation), int(stage), rec.ctypes.data_as(C.POINTER(C.c_int)), tot)
        finally:
            self.set_libm_jitter(0, 0)
        keys = ("solves", "newton", "newton_max", "fail_newton", "fail_outer", "fail_dust", "decoupled", "mask")
        return U, dict(zip(keys, rec)), [int(v) for v in tot]

    # ---------------------------------------------------------------- the radiation transport operators, face by face and stage by stage
    def rad_cons_to_prim(self, t: RadCellTraits, cons: np.ndarray) -> np.ndarray:
        """ConservedToPrimitive of one photon group on cons[4, n] = (E, Fx, Fy, Fz): prim[4, n] = (E, fx, fy, fz)"""
        cons = np.ascontiguousarray(cons, dtype=np.float64)
        assert cons.ndim == 2 and cons.shape[0] == 4
        prim = np.empty_like(cons)
        f = self.lib.orc_rad_cons_to_prim
        f.argtypes, f.restype = [C.POINTER(RadCellTraits), C.c_long, C.POINTER(C.c_double), C.POINTER(C.c_double)], None
        f(C.byref(t), cons.shape[1], _dp(cons), _dp(prim))
        return prim

    def rad_face_fluxes(self, t: RadCellTraits, direction, pL, pR, consL, consR, eps=None):
        """ComputeFluxes on n faces, each a box of its own: direction[n] (0..2), pL / pR / consL / consR [4, n], eps[n] (None: 1, no wavespeed
        correction).  Returns (F[4, n], mask[n]) with the bits of RAD_FACE_BIT"""
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (pL, pR, consL, consR)]
        n = a[0].shape[1]
        assert all(v.shape == (4, n) for v in a)
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(direction, dtype=np.int32), (n,)))
        e = np.ones(n) if eps is None else np.ascontiguousarray(eps, dtype=np.float64)
        assert e.shape == (n,) and d.min() >= 0 and d.max() <= 2
        F, mask = np.empty((4, n)), np.zeros(n, dtype=np.int32)
        f = self.lib.orc_rad_face_fluxes
        DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
        f.argtypes, f.restype = [C.POINTER(RadCellTraits), C.c_long, IP, DP, DP, DP, DP, DP, DP, IP], None
        self.lib.orc_set_num_threads(int(max(1, min(usable_cores(), n // 4096))))
        f(C.byref(t), n, d.ctypes.data_as(IP), _dp(a[0]), _dp(a[1]), _dp(a[2]), _dp(a[3]), _dp(e), _dp(F), mask.ctypes.data_as(IP))
        return F, mask

    def rad_transport_stage(self, t: RadCellTraits, ngroups: int, ndim: int, order: int, stage: int, U_in: np.ndarray, U0: np.ndarray, vlo, vhi, dt: float, dx,
                            eps=None, nghost: int = 4):
        """One transport stage of one box on ghost-filled arrays (6 + 4 ngroups, nz, ny, nx) that the caller owns: computeRadiationFluxes(U_in) and
        PredictStep(U0) (stage 1) or AddFluxesRK2(U0, U1 = U_in) (stage 2).  eps: None or one array (ngroups, faces...) per direction.  Returns
        (U_new — a copy of U_in with the radiation components of the valid cells replaced —, [flux_d (4 ngroups, faces...)], [face mask_d (ngroups,
        faces...), RAD_FACE_BIT], cell mask (ngroups, valid cells...), RAD_CELL_BIT)"""
        U_in = np.ascontiguousarray(U_in, dtype=np.float64)
        U0 = np.ascontiguousarray(U0, dtype=np.float64)
        nv = [int(vhi[d] - vlo[d] + 1) for d in range(3)]
        shape = (6 + 4 * ngroups,) + tuple(nv[d] + (2 * nghost if d < ndim else 0) for d in (2, 1, 0))
        assert U_in.shape == shape and U0.shape == shape, (U_in.shape, U0.shape, shape)
        U_new = U_in.copy()
        DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
        flux, fmask, epsp = [], [], (DP * 3)()
        fp, mp = (DP * 3)(), (IP * 3)()
        keep = []
        for d in range(ndim):
            n = list(nv)
            n[d] += 1
            fs = (n[2], n[1], n[0])
            flux.append(np.empty((4 * ngroups,) + fs))
            fmask.append(np.zeros((ngroups,) + fs, dtype=np.int32))
            fp[d], mp[d] = _dp(flux[d]), fmask[d].ctypes.data_as(IP)
            if eps is not None and eps[d] is not None:
                e = np.ascontiguousarray(eps[d], dtype=np.float64)
                assert e.shape == (ngroups,) + fs
                keep.append(e)
                epsp[d] = _dp(e)
        cmask = np.zeros((ngroups, nv[2], nv[1], nv[0]), dtype=np.int32)
        f = self.lib.orc_rad_transport_stage
        f.argtypes = [C.POINTER(RadCellTraits), C.c_int, C.c_int, C.c_int, C.c_int, DP, DP, DP, _I3, _I3, C.c_int, C.c_double, C.c_double * 3, DP * 3, DP * 3,
                      IP * 3, IP]
        f.restype = None
        f(C.byref(t), int(ngroups), int(ndim), int(order), int(stage), _dp(U_in), _dp(U0), _dp(U_new), _i3(vlo), _i3(vhi), int(nghost), float(dt),
          (C.c_double * 3)(*[float(x) for x in dx]), epsp, fp, mp, cmask.ctypes.data_as(IP))
        return U_new, flux, fmask, cmask

    # ---------------------------------------------------------------- multigroup helper functions
    def planck_integral(self, x: float) -> float:
        return self.lib.orc_planck_integral(float(x))

    def planck_table(self) -> np.ndarray:
        return np.array([self.lib.orc_planck_table_entry(j) for j in range(1000)])

    def planck_fractions(self, boundaries, energy_unit, k_B, a_rad, Erad_floor, T):
        b = np.ascontiguousarray(boundaries, dtype=np.float64)
        n = len(b) - 1
        f, E = np.empty(n), np.empty(n)
        self.lib.orc_planck_fractions(n, _dp(b), energy_unit, k_B, a_rad, Erad_floor, T, _dp(f), _dp(E))
        return f, E

    def planck_function(self, energy_unit, k_B, a_rad, nu, T) -> float:
        return self.lib.orc_planck_function(energy_unit, k_B, a_rad, nu, T)

    def group_mean_opacity(self, boundaries, expo, lower, alpha_quant) -> np.ndarray:
        b, e, l, a = (np.ascontiguousarray(v, dtype=np.float64) for v in (boundaries, expo, lower, alpha_quant))
        k = np.empty(len(b) - 1)
        self.lib.orc_group_mean_opacity(len(b) - 1, _dp(b), _dp(e), _dp(l), _dp(a), _dp(k))
        return k

    def rad_quantity_exponents(self, boundaries, quant) -> np.ndarray:
        b, q = (np.ascontiguousarray(v, dtype=np.float64) for v in (boundaries, quant))
        e = np.empty(len(q))
        self.lib.orc_rad_quantity_exponents(len(q), _dp(b), _dp(q), _dp(e))
        return e

    # ---------------------------------------------------------------- per-operator
    def cons_to_prim(self, t: HydroTraits, cons: np.ndarray, glo, ghi) -> np.ndarray:
        prim = np.empty_like(cons)
        self.lib.orc_cons_to_prim(C.byref(t), _dp(cons), _dp(prim), _i3(glo), _i3(ghi))
        return prim

    def flattening_coefficients(self, t: HydroTraits, d: int, prim: np.ndarray, glo, ghi, clo, chi) -> np.ndarray:
        shape = tuple(int(chi[a] - clo[a] + 1) for a in (2, 1, 0))
        out = np.empty(shape, dtype=np.float64)
        self.lib.orc_flattening_coefficients(C.byref(t), int(d), _dp(prim), _i3(glo), _i3(ghi), _dp(out), _i3(clo), _i3(chi))
        return out

    def compute_hydro_fluxes(self, t: HydroTraits, order: int, cons: np.ndarray, vlo, vhi, nghost=4, K_visc=0.0, mhd_stub=False):
        """cons: (nvar, ...) on the valid box grown by nghost. Returns ([flux_d], [facevel_d]).  mhd_stub: Physics_Traits::is_mhd_enabled — the
        interface fluxes come from HLLD with the reference's B = 0 stub (hydro_system.hpp:987-1003) instead of HLLC"""
        if mhd_stub:
            assert order in (1, 2, 3)
            order = order + 10
        nv = 6 + t.nscalars
        fl, fv = [], []
        for d in range(3):
            if d < t.ndim:
                n = [int(vhi[a] - vlo[a] + 1) for a in range(3)]
                n[d] += 1
                fl.append(np.empty((nv, n[2], n[1], n[0]), dtype=np.float64))
                fv.append(np.empty((n[2], n[1], n[0]), dtype=np.float64))
            else:
                fl.append(np.empty((0,), dtype=np.float64))
                fv.append(np.empty((0,), dtype=np.float64))
        self.lib.orc_compute_hydro_fluxes(C.byref(t), int(order), C.c_double(K_visc), _dp(cons), _i3(vlo), _i3(vhi), int(nghost),
                                          _dp(fl[0]), _dp(fl[1]), _dp(fl[2]), _dp(fv[0]), _dp(fv[1]), _dp(fv[2]))
        return fl[: t.ndim], fv[: t.ndim]

    # ---------------------------------------------------------------- hydro operators on arrays the caller owns
    # v = (vlo, vhi) is the valid box; cell-centred state arrays live on v grown by `nghost` in the first t.ndim directions
    @staticmethod
    def _grown(t: HydroTraits, vlo, vhi, ng):
        return [int(vlo[d]) - (ng if d < t.ndim else 0) for d in range(3)], [int(vhi[d]) + (ng if d < t.ndim else 0) for d in range(3)]

    @staticmethod
    def _shape(lo, hi, facedir=-1):
        return tuple(int(hi[d] - lo[d] + 1 + (1 if d == facedir else 0)) for d in (2, 1, 0))

    def hydro_face_fluxes(self, t: HydroTraits, riemann: int, d: int, L: np.ndarray, R: np.ndarray, prim: np.ndarray, vlo, vhi, nghost_prim=1, K_visc=0.0):
        """ComputeFluxes<riemann, d> on caller-supplied left / right states (face box of v, nvar components) and primitives (v grown by
        nghost_prim, the velocity differences only): returns (flux, face velocity) on the face box"""
        nv = 6 + t.nscalars
        fs = self._shape(vlo, vhi, d)
        assert L.shape == R.shape == (nv,) + fs and prim.shape == (nv,) + self._shape(*self._grown(t, vlo, vhi, nghost_prim)) and nghost_prim >= 1
        flux, fvel = np.empty((nv,) + fs), np.empty(fs)
        f = self.lib.orc_hydro_face_fluxes
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, _I3, _I3, C.c_int, C.c_void_p,
                                 C.c_void_p], None
        f(C.byref(t), int(riemann), int(d), float(K_visc), _dp(L), _dp(R), _dp(prim), _i3(vlo), _i3(vhi), int(nghost_prim), _dp(flux), _dp(fvel))
        return flux, fvel

    def hydro_enforce_limits(self, t: HydroTraits, state: np.ndarray, vlo, vhi, nghost, density_floor: float, temp_floor: float, nmscalars=0) -> np.ndarray:
        glo, ghi = self._grown(t, vlo, vhi, nghost)
        out = np.array(state, dtype=np.float64, order="C")
        assert out.shape == (6 + t.nscalars,) + self._shape(glo, ghi)
        f = self.lib.orc_hydro_enforce_limits
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_int, C.c_double, C.c_double, C.c_void_p, _I3, _I3, _I3, _I3], None
        f(C.byref(t), int(nmscalars), float(density_floor), float(temp_floor), _dp(out), _i3(glo), _i3(ghi), _i3(vlo), _i3(vhi))
        return out

    def hydro_sync_dual_energy(self, t: HydroTraits, state: np.ndarray, vlo, vhi, nghost):
        """returns (state, fatal): fatal (bool, on v) marks the cells the reference aborts on (rho <= 0); they are left untouched"""
        glo, ghi = self._grown(t, vlo, vhi, nghost)
        out = np.array(state, dtype=np.float64, order="C")
        assert out.shape == (6 + t.nscalars,) + self._shape(glo, ghi)
        fatal = np.zeros(self._shape(vlo, vhi), dtype=np.int32)
        f = self.lib.orc_hydro_sync_dual_energy
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_void_p, _I3, _I3, _I3, _I3, C.c_void_p], C.c_long
        n = f(C.byref(t), _dp(out), _i3(glo), _i3(ghi), _i3(vlo), _i3(vhi), fatal.ctypes.data_as(C.c_void_p))
        assert n == int(fatal.sum())
        return out, fatal.astype(bool)

    def hydro_max_signal_speed(self, t: HydroTraits, cons: np.ndarray, vlo, vhi, nghost) -> np.ndarray:
        glo, ghi = self._grown(t, vlo, vhi, nghost)
        assert cons.shape == (6 + t.nscalars,) + self._shape(glo, ghi)
        out = np.empty(self._shape(vlo, vhi))
        f = self.lib.orc_hydro_max_signal_speed
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_void_p, _I3, _I3, _I3, _I3, C.c_void_p], None
        f(C.byref(t), _dp(cons), _i3(glo), _i3(ghi), _i3(vlo), _i3(vhi), _dp(out))
        return out

    def hydro_max_signal_local(self, t: HydroTraits, which: int, cons: np.ndarray, vlo, vhi, nghost) -> float:
        """the serial reduction over v: which = 0 maxSignalSpeedLocal, which = 1 the maximum of ComputeMaxSignalSpeed (a NaN never wins)"""
        glo, ghi = self._grown(t, vlo, vhi, nghost)
        assert cons.shape == (6 + t.nscalars,) + self._shape(glo, ghi)
        f = self.lib.orc_hydro_max_signal_local
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_int, C.c_void_p, _I3, _I3, _I3, _I3], C.c_double
        return float(f(C.byref(t), int(which), _dp(cons), _i3(glo), _i3(ghi), _i3(vlo), _i3(vhi)))

    def hydro_predict_step(self, t: HydroTraits, cons_old: np.ndarray, cons_new: np.ndarray, rhs: np.ndarray, dt: float, nvars: int, vlo, vhi, nghost,
                           nmscalars=0):
        """PredictStep + isStateValid: returns (new state, redo flags on v, number of flagged cells); cons_new supplies what the call leaves alone"""
        glo, ghi = self._grown(t, vlo, vhi, nghost)
        out = np.array(cons_new, dtype=np.float64, order="C")
        assert cons_old.shape == out.shape == (out.shape[0],) + self._shape(glo, ghi) and rhs.shape == (nvars,) + self._shape(vlo, vhi)
        flags = np.full(self._shape(vlo, vhi), -1, dtype=np.int32)
        f = self.lib.orc_hydro_predict_step
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, _I3, _I3, _I3, _I3,
                                 C.c_void_p], C.c_long
        n = f(C.byref(t), int(nmscalars), _dp(cons_old), _dp(out), out.shape[0], _dp(rhs), float(dt), int(nvars), _i3(glo), _i3(ghi), _i3(vlo), _i3(vhi),
              flags.ctypes.data_as(C.c_void_p))
        return out, flags, int(n)

    def hydro_rhs_from_fluxes(self, t: HydroTraits, fluxes, dx, nvars: int, vlo, vhi) -> np.ndarray:
        for d in range(t.ndim):
            assert fluxes[d].shape == (nvars,) + self._shape(vlo, vhi, d)
        rhs = np.empty((nvars,) + self._shape(vlo, vhi))
        ptrs = (C.c_void_p * 3)(*[fluxes[d].ctypes.data if d < t.ndim else None for d in range(3)])
        for d in range(t.ndim):
            _dp(fluxes[d])
        f = self.lib.orc_hydro_rhs_from_fluxes
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_void_p, C.c_void_p * 3, C.c_double * 3, C.c_int, _I3, _I3], None
        f(C.byref(t), _dp(rhs), ptrs, (C.c_double * 3)(*[float(x) for x in dx]), int(nvars), _i3(vlo), _i3(vhi))
        return rhs

    def hydro_add_pdv(self, t: HydroTraits, rhs: np.ndarray, cons: np.ndarray, dx, vels, redo: np.ndarray, vlo, vhi, nghost) -> np.ndarray:
        """AddInternalEnergyPdV: rhs (on v) + the -P div(v) term, div(v) from the face velocities (redo == 0) or from the cell velocities"""
        glo, ghi = self._grown(t, vlo, vhi, nghost)
        out = np.array(rhs, dtype=np.float64, order="C")
        assert nghost >= 1 and cons.shape == (6 + t.nscalars,) + self._shape(glo, ghi) and out.shape[1:] == self._shape(vlo, vhi) == redo.shape
        assert redo.dtype == np.int32 and redo.flags["C_CONTIGUOUS"]
        for d in range(t.ndim):
            assert vels[d].shape == self._shape(vlo, vhi, d)
            _dp(vels[d])
        ptrs = (C.c_void_p * 3)(*[vels[d].ctypes.data if d < t.ndim else None for d in range(3)])
        f = self.lib.orc_hydro_add_pdv
        f.argtypes, f.restype = [C.POINTER(HydroTraits), C.c_void_p, C.c_int, C.c_void_p, _I3, _I3, C.c_double * 3, C.c_void_p * 3, C.c_void_p, _I3, _I3], None
        f(C.byref(t), _dp(out), out.shape[0], _dp(cons), _i3(glo), _i3(ghi), (C.c_double * 3)(*[float(x) for x in dx]), ptrs,
          redo.ctypes.data_as(C.c_void_p), _i3(vlo), _i3(vhi))
        return out

    # ---------------------------------------------------------------- whole simulation
    def average_down(self, fine: np.ndarray, flo, crse: np.ndarray, clo, region, scomp: int, ncomp: int, ratio=(2, 2, 2)):
        """amrex::average_down restated: fine / crse are (ncomp_total, nz, ny, nx) float64 arrays whose lower corners are flo / clo;
        region = (lo, hi) in coarse indices; crse is modified in place"""
        assert fine.dtype == np.float64 and crse.dtype == np.float64 and fine.flags["C_CONTIGUOUS"] and crse.flags["C_CONTIGUOUS"]
        fhi = [flo[d] + fine.shape[3 - d] - 1 for d in range(3)]
        chi = [clo[d] + crse.shape[3 - d] - 1 for d in range(3)]
        L = self.lib
        L.orc_average_down.argtypes = [C.c_void_p, _I3, _I3, C.c_void_p, _I3, _I3, C.c_int, _I3, _I3, C.c_int, C.c_int, _I3]
        L.orc_average_down(fine.ctypes.data_as(C.c_void_p), _i3(flo), _i3(fhi), crse.ctypes.data_as(C.c_void_p), _i3(clo), _i3(chi), fine.shape[0],
                           _i3(region[0]), _i3(region[1]), scomp, ncomp, _i3(ratio))

    def interp_from_coarse(self, fine: np.ndarray, flo, crse_old: np.ndarray, crse_new: np.ndarray, clo, region, w_old: float, w_new: float, ncomp: int,
                           method: int = 1, hooks: bool = True, ndim: int = 3, ratio=(2, 2, 2)):
        """coarse -> fine interpolation restated (oracle/amr.hpp): fills `region` = (lo, hi) (fine indices) of `fine` in place"""
        for a in (fine, crse_old, crse_new):
            assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
        fhi = [flo[d] + fine.shape[3 - d] - 1 for d in range(3)]
        chi = [clo[d] + crse_old.shape[3 - d] - 1 for d in range(3)]
        L = self.lib
        L.orc_interp_from_coarse.argtypes = [C.c_void_p, _I3, _I3, C.c_void_p, C.c_void_p, _I3, _I3, C.c_int, _I3, _I3, C.c_double, C.c_double, C.c_int, C.c_int,
                                             C.c_int, C.c_int, _I3]
        L.orc_interp_from_coarse(fine.ctypes.data_as(C.c_void_p), _i3(flo), _i3(fhi), crse_old.ctypes.data_as(C.c_void_p), crse_new.ctypes.data_as(C.c_void_p),
                                 _i3(clo), _i3(chi), fine.shape[0], _i3(region[0]), _i3(region[1]), w_old, w_new, ncomp, method, int(hooks), ndim, _i3(ratio))

    def sim(self, problem, ndim, n_cell, prob_lo, prob_hi, periodic, max_grid_size=None, cfl=-1.0, stop_time=-1.0,
            max_timesteps=-1, reconstruction_order=-1, nscalars=0, table=None, rad_pow_mode=0, hydro1d=None, beta_order=0, c_hat_factor=0.0,
            opacity_model=0, dust_coeff=0.0) -> "OracleSim":
        n_cell = list(n_cell) + [1] * (3 - len(n_cell))
        mgs = list(max_grid_size) if max_grid_size is not None else list(n_cell)
        mgs = mgs + [1] * (3 - len(mgs))
        cfg = SimConfig(problem, ndim, _i3(n_cell), _i3(mgs), (C.c_double * 3)(*prob_lo), (C.c_double * 3)(*prob_hi), _i3(periodic),
                        cfl, stop_time, max_timesteps, reconstruction_order, nscalars)
        if table is not None:  # (r_over_r0, Erad, Frad) columns
            cols = [np.ascontiguousarray(c, dtype=np.float64) for c in table]
            cfg.table_len = len(cols[0])
            cfg.table_r, cfg.table_Erad, cfg.table_Frad = (_dp(c) for c in cols[:3])
            if len(cols) > 3:  # RADTUBE: (x, rho, Pgas, Erad)
                cfg.table_extra = _dp(cols[3])
            self._keepalive = cols
        cfg.rad_pow_mode = rad_pow_mode
        cfg.opacity_model = int(opacity_model)
        if hydro1d is not None:  # dict: gamma, profile, x_split, left, right, dirichlet, cfl, max_dt, init_dt, stop_time (see oracle/problems.hpp Hydro1DSpec)
            h = hydro1d
            vals = [h["gamma"], h.get("x_split", 0.0)] + list(h.get("left", [0, 0, 0])) + list(h.get("right", [0, 0, 0])) + \
                   [h["cfl"], h.get("max_dt", -1.0), h.get("init_dt", -1.0), h["stop_time"]]
            cfg.h1d = (C.c_double * 12)(*[float(v) for v in vals])
            cfg.h1d_i = (C.c_int * 2)(int(h.get("profile", 0)), int(h.get("dirichlet", 1)))
        if c_hat_factor > 0:  # COUPLING: the reduced-speed-of-light variant (RadMatterCouplingRSLA)
            cfg.h1d[0] = float(c_hat_factor)
        if dust_coeff > 0:  # LINE_COOLING*, MARSHAK_DUST_PE: radiation.dust_gas_interaction_coeff of the deck
            cfg.h1d[1] = float(dust_coeff)
        if beta_order > 0:  # RADSHOCK / ADVECTING parity variants: override RadSystem_Traits::beta_order
            cfg.h1d_i[0] = int(beta_order)
        # team size by problem size: ~16k cells per thread at least (a 1-D 512-cell run makes ~10^5 tiny parallel regions per second)
        ncells = int(np.prod(n_cell[:ndim]))
        self.lib.orc_set_num_threads(int(max(1, min(usable_cores(), ncells // 16384))))
        h = self.lib.orc_sim_create(C.byref(cfg))
        assert h, "oracle: unknown problem"
        return OracleSim(self, h, ndim)


@dataclass
class OracleSim:
    o: Oracle
    h: int
    ndim: int

    def __del__(self):
        try:
            self.o.lib.orc_sim_destroy(self.h)
        except Exception:
            pass

    @property
    def nboxes(self):
        return self.o.lib.orc_sim_nboxes(self.h)

    @property
    def ncomp(self):
        return self.o.lib.orc_sim_ncomp(self.h)

    @property
    def nghost(self):
        return self.o.lib.orc_sim_nghost(self.h)

    @property
    def time(self):
        return self.o.lib.orc_sim_time(self.h)

    @property
    def dt(self):
        return self.o.lib.orc_sim_dt(self.h)

    @property
    def istep(self):
        return self.o.lib.orc_sim_istep(self.h)

    def box(self, b):
        lo, hi = _I3(), _I3()
        self.o.lib.orc_sim_box(self.h, b, lo, hi)
        return list(lo), list(hi)

    def fab_shape(self, b):
        lo, hi = self.box(b)
        ng = self.nghost
        n = [hi[d] - lo[d] + 1 + (2 * ng if d < self.ndim else 0) for d in range(3)]
        return (self.ncomp, n[2], n[1], n[0])

    def state(self, b=0, which=0) -> np.ndarray:
        """Whole fab (valid + ghosts) as (ncomp, nz, ny, nx)."""
        a = np.empty(self.fab_shape(b), dtype=np.float64)
        self.o.lib.orc_sim_get_state(self.h, which, b, _dp(a))
        return a

    def valid(self, b=0, which=0) -> np.ndarray:
        a = self.state(b, which)
        ng = self.nghost
        sl = [slice(None)] + [slice(ng, -ng) if d < self.ndim else slice(None) for d in (2, 1, 0)]
        return np.ascontiguousarray(a[tuple(sl)])

    def set_state(self, a: np.ndarray, b=0, which=0):
        assert a.shape == self.fab_shape(b)
        self.o.lib.orc_sim_set_state(self.h, which, b, _dp(np.ascontiguousarray(a)))

    def fill_ghosts(self, which=0, time=0.0):
        self.o.lib.orc_sim_fill_ghosts(self.h, which, time)

    def compute_dt(self) -> float:
        return self.o.lib.orc_sim_compute_dt(self.h)

    def step(self) -> bool:
        return bool(self.o.lib.orc_sim_step(self.h))

    def advance_fixed_dt(self, dt: float) -> bool:
        return bool(self.o.lib.orc_sim_advance_fixed_dt(self.h, dt))

    def evolve(self) -> bool:
        return bool(self.o.lib.orc_sim_evolve(self.h))

    def set_limits(self, density_floor: float = 0.0, temp_floor: float = 0.0):
        """the floors EnforceLimits applies after every stage (0: none, the default)"""
        self.o.lib.orc_sim_set_limits.argtypes = [C.c_void_p, C.c_double, C.c_double]
        self.o.lib.orc_sim_set_limits(self.h, float(density_floor), float(temp_floor))

    def set_fused_fluxes(self, on: bool, stages: bool = True):
        """the fused, vectorised flux evaluation (oracle/hydro_fused.hpp) instead of the operator sequence: the same bits, one pass per box;
        stages: the update, the limits and the dual-energy sync of a stage in the same pass over the box as well (HydroSim::fusedStage)"""
        self.o.lib.orc_sim_set_fused_fluxes.argtypes = [C.c_void_p, C.c_int]
        self.o.lib.orc_sim_set_fused_fluxes(self.h, (1 if on else 0) | (2 if (on and stages) else 0))

    def set_rk2_carry_rhs(self, on: bool):
        """the carried form of the RK2 average (HydroSim::rk2_carry_rhs; the GPU path's `rk2_carry_rhs`): stage 1 keeps U_old + (dt/2) r_1 and P(U_old)
        per cell, stage 2 finishes with (dt/2) r_2 of its own fluxes.  Off by default (the reference's flux_rk2 = 0.5 F1 + 0.5 F2)."""
        self.o.lib.orc_sim_set_rk2_carry_rhs.argtypes = [C.c_void_p, C.c_int]
        self.o.lib.orc_sim_set_rk2_carry_rhs(self.h, int(bool(on)))

    def carry_half(self, b: int = 0) -> np.ndarray:
        """what the last stage 1 of the carried form stored for box b: (ncomp + 1, nz, ny, nx), S = U_old + (dt/2) r_1 then P(U_old)"""
        lo, hi = self.box(b)
        a = np.empty((self.ncomp + 1,) + tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0)))
        f = self.o.lib.orc_sim_carry_half
        f.argtypes, f.restype = [C.c_void_p, C.c_int, C.POINTER(C.c_double)], C.c_long
        assert f(self.h, int(b), _dp(a)) == a.size, "no carried stage 1 has run"
        return a

    def hydro_fluxes(self, b: int, direction: int, fused: bool):
        """(flux[6, faces...], face velocity) of box b from the current state_new (ghost cells filled here), by either form"""
        lo, hi = self.box(b)
        n = [hi[d] - lo[d] + 1 + (1 if d == direction else 0) for d in range(3)]
        F = np.empty((6, n[2], n[1], n[0]))
        V = np.empty((n[2], n[1], n[0]))
        f = self.o.lib.orc_sim_hydro_fluxes
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        assert f(self.h, int(bool(fused)), int(b), int(direction), _dp(F), _dp(V)) == V.size
        return F, V

    def rad_transport_only(self, dt_radiation: float):
        self.o.lib.orc_sim_rad_transport_only(self.h, float(dt_radiation))

    def set_rad_reconstruction_order(self, order: int):
        self.o.lib.orc_sim_set_rad_reconstruction_order.argtypes = [C.c_void_p, C.c_int]
        self.o.lib.orc_sim_set_rad_reconstruction_order(self.h, int(order))

    def set_wavespeed_correction(self, on: bool):
        """QuokkaSimulation::use_wavespeed_correction_ (reference src/QuokkaSimulation.hpp:133): ComputeCellOpticalDepth + S_corr on even faces"""
        self.o.lib.orc_sim_set_wavespeed_correction.argtypes = [C.c_void_p, C.c_int]
        self.o.lib.orc_sim_set_wavespeed_correction(self.h, int(bool(on)))

    def run_record(self, nsteps: int, b=0, cell=(0, 0, 0)):
        """nsteps steps; returns (times, states[nsteps, ncomp]) of one valid cell after every step"""
        t = np.zeros(nsteps)
        u = np.zeros((nsteps, self.ncomp))
        f = self.o.lib.orc_sim_run_record
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        n = f(self.h, nsteps, int(b), int(cell[0]), int(cell[1]), int(cell[2]), _dp(t), _dp(u))
        return t[:n], u[:n]

    def rad_counters(self):
        out = (C.c_long * 8)()
        self.o.lib.orc_sim_rad_counters(self.h, out)
        keys = ["solves", "newton_iterations", "max_newton_iterations", "decoupled", "fail_coupling", "fail_dust", "fail_outer", "rad_cell_updates"]
        return dict(zip(keys, list(out)))

    def tag_relative_gradient(self, b: int, field: int, eta_threshold: float, q_min: float, min_inclusive: bool) -> np.ndarray:
        """ErrorEst (gradient-threshold family) on the ghost-filled new state of box b: int8 array over the valid box (2 = TagBox::SET)"""
        lo, hi = self.box(b)
        t = np.zeros((hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1), dtype=np.int8)
        self.o.lib.orc_sim_tag_relative_gradient(self.h, b, int(field), C.c_double(eta_threshold), C.c_double(q_min), int(bool(min_inclusive)),
                                                 t.ctypes.data_as(C.c_void_p))
        return t

    def tag_centered_gradient(self, b: int, comp: int, direction: int, dx: float, eta_threshold: float, q_min: float, min_inclusive: bool) -> np.ndarray:
        """ErrorEst of HydroShocktube (centred difference / (2 dx)) on the ghost-filled new state of box b"""
        lo, hi = self.box(b)
        t = np.zeros((hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1), dtype=np.int8)
        self.o.lib.orc_sim_tag_centered_gradient(self.h, b, int(comp), int(direction), C.c_double(dx), C.c_double(eta_threshold), C.c_double(q_min),
                                                 int(bool(min_inclusive)), t.ctypes.data_as(C.c_void_p))
        return t

    def rad_source(self, b=0, time=0.0) -> np.ndarray:
        lo, hi = self.box(b)
        a = np.empty((hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1), dtype=np.float64)
        self.o.lib.orc_sim_rad_source(self.h, b, C.c_double(time), _dp(a))
        return a

    def counters(self):
        out = (C.c_long * 3)()
        self.o.lib.orc_sim_counters(self.h, out)
        f = self.o.lib.orc_sim_carry2_fallbacks
        f.argtypes, f.restype = [C.c_void_p], C.c_long
        # carry2_fallbacks: stages 2 of the carried form (set_rk2_carry_rhs) whose carried pass flagged cells and that were redone in the exact form
        return {"fofc1_cells": out[0], "fofc2_cells": out[1], "retries": out[2], "carry2_fallbacks": f(self.h)}


class OracleCloudy:
    """oracle/cooling.hpp: the reference's tabulated cooling on the arrays of a cloudy_cooling_tools file (Parameter1, Temperature, Cooling,
    Heating, MMW as H5Dread delivers them)"""
    TGAS_FROM_EGAS, EGAS_FROM_TGAS, MMW, COOLING_LENGTH, NET_HEATING = range(5)

    # the branch mask of cooling_cells (oracle/cooling.hpp: BR_*)
    BRANCHES = ("emin", "emax", "nh_low", "nh_high", "yi_quirk", "ix_top", "parabola", "secant", "bisect", "empty_bracket", "seven_refusals",
                "max_substeps", "nan_dt_guess", "coincide", "eta_floor")

    def __init__(self, arrays: dict, variant: str = "direct", libm: str = "glibc"):
        """libm: "glibc" — std::log10 / std::pow, as the reference — or "portable": oracle/portable_libm.hpp, the functions a GPU reproduces bit for
        bit (the kernels' portable instantiation is compared with this one)"""
        self.o = Oracle(variant)
        self.libm = {"glibc": 0, "portable": 1}[libm]
        L = self.lib = self.o.lib
        L.orc_cloudy_create.restype = C.c_void_p
        DP = C.POINTER(C.c_double)
        L.orc_cloudy_create.argtypes = [C.c_int, C.c_int, DP, DP, DP, DP, DP]
        L.orc_cloudy_destroy.argtypes = [C.c_void_p]
        L.orc_cloudy_ranges.argtypes = [C.c_void_p, DP]
        L.orc_cloudy_get.argtypes = [C.c_void_p, C.c_int, DP]
        L.orc_cloudy_evaluate.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_long, DP, DP, DP]
        L.orc_cloudy_compute_cooling.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_long, DP, C.POINTER(C.c_int)]
        L.orc_cloudy_cooling_cells.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_long, DP, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.orc_cloudy_set_libm.argtypes = [C.c_int]
        L.orc_portable_libm.argtypes = [C.c_int, C.c_long, DP, DP]
        a = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
        self.n0, self.n1 = a["Cooling"].shape
        self.h = C.c_void_p(L.orc_cloudy_create(self.n0, self.n1, _dp(a["Parameter1"]), _dp(a["Temperature"]), _dp(a["Cooling"]), _dp(a["Heating"]), _dp(a["MMW"])))

    def __del__(self):
        try:
            self.lib.orc_cloudy_destroy(self.h)
        except Exception:
            pass

    def ranges(self):
        """(T_min, T_max, mmw_min, mmw_max)"""
        r = np.zeros(4)
        self.lib.orc_cloudy_ranges(self.h, _dp(r))
        return tuple(float(v) for v in r)

    def prepared(self, which: int) -> np.ndarray:
        """0 log_nH, 1 log_Tgas, 2 cooling, 3 heating, 4 mean molecular weight (n_H fastest)"""
        out = np.zeros([self.n0, self.n1, self.n0 * self.n1, self.n0 * self.n1, self.n0 * self.n1][which])
        self.lib.orc_cloudy_get(self.h, which, _dp(out))
        return out

    def evaluate(self, what: int, rho, val, gamma: float) -> np.ndarray:
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        val = np.ascontiguousarray(val, dtype=np.float64)
        out = np.zeros_like(rho)
        self.lib.orc_cloudy_set_libm(self.libm)
        self.lib.orc_cloudy_evaluate(self.h, gamma, what, rho.size, _dp(rho), _dp(val), _dp(out))
        return out

    def compute_cooling(self, U: np.ndarray, gamma: float, dt: float, T_floor: float):
        """U[6, n] = (rho, x1Mom, x2Mom, x3Mom, Egas, Eint_aux): returns (U after computeCooling, substeps per cell)"""
        U = np.ascontiguousarray(U, dtype=np.float64).copy()
        n = U.shape[1]
        ns = np.zeros(n, dtype=np.int32)
        self.lib.orc_cloudy_set_libm(self.libm)
        self.lib.orc_cloudy_compute_cooling(self.h, gamma, dt, T_floor, n, _dp(U), ns.ctypes.data_as(C.POINTER(C.c_int)))
        return U, ns

    def cooling_cells(self, U: np.ndarray, gamma: float, dt: float, T_floor: float):
        """compute_cooling with a record per cell: returns (U after, substeps, rec) — rec a dict of int arrays: attempts, refused, deepest_retry,
        failed_rhs, f_evals (Algorithm 748), mask (bit i = BRANCHES[i])"""
        U = np.ascontiguousarray(U, dtype=np.float64).copy()
        n = U.shape[1]
        ns = np.zeros(n, dtype=np.int32)
        rec = np.zeros((6, n), dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self.lib.orc_cloudy_set_libm(self.libm)
        self.lib.orc_cloudy_cooling_cells(self.h, gamma, dt, T_floor, n, _dp(U), ip(ns), ip(rec))
        return U, ns, dict(zip(("attempts", "refused", "deepest_retry", "failed_rhs", "f_evals", "mask"), rec))

    def bit(self, name: str) -> int:
        return 1 << self.BRANCHES.index(name)

    def portable_libm(self, which: int, x) -> np.ndarray:
        """oracle/portable_libm.hpp: which = 0 log10, 1 x^(-1/2)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        self.lib.orc_portable_libm(which, x.size, _dp(x), _dp(out))
        return out
