"""GPU parity of every reference-shaped hydro operator (C-ABI) against the CPU oracle: bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import pyoracle
from quokka_amd import capi
from quokka_amd.hydro_system import HydroSystem, HyperbolicSystem
from quokka_amd.multifab import Level, MultiFab

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def random_state(rng, shape, shock=True):
    """Smooth background + a strong jump: positive rho and pressure, all six comps populated."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
    rho = 1.0 + 0.3 * np.sin(5 * x + 2 * y) * np.cos(3 * z) + 0.05 * rng.standard_normal(shape)
    P = 1.0 + 0.4 * np.cos(4 * y - z) + 0.05 * rng.standard_normal(shape)
    if shock:
        m = (x + 0.3 * y + 0.2 * z) < 0.7
        rho = np.where(m, rho * 8.0, rho)
        P = np.where(m, P * 50.0, P)
    v = [0.5 * np.sin(6 * x * (d + 1) + y) + 0.2 * rng.standard_normal(shape) for d in range(3)]
    g = 1.4
    U = np.zeros((6,) + shape)
    U[0] = rho
    for d in range(3):
        U[1 + d] = rho * v[d]
    U[4] = P / (g - 1) + 0.5 * rho * (v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    U[5] = P / (g - 1) * (1.0 + 0.01 * rng.standard_normal(shape))
    return U


def gpu_fluxes(ctx, tr, cons_np, vlo, vhi, order, ndim=3, K_visc=0.0, fo=False, riemann=None):
    """computeHydroFluxes / computeFOHydroFluxes (reference src/QuokkaSimulation.hpp:1403-1568) with the C-ABI operators."""
    lev = Level(ctx, ndim, [(vlo, vhi)])
    hs = HydroSystem(tr)
    nv, ng = 6, 4
    cons = MultiFab(lev, nv, ng)
    cons.set_fab(0, cons_np)
    prim = MultiFab(lev, nv, ng)
    hs.ConservedToPrimitive(lev, cons, prim, ng)
    chis = [MultiFab(lev, 1, 2, fill=float("nan")) for _ in range(3)]
    if not fo:
        for d in range(ndim):
            hs.ComputeFlatteningCoefficients(lev, d, prim, chis[d], 2)
    F, V, LS, RS = [], [], [], []
    for d in range(ndim):
        L = MultiFab(lev, nv, 1, facedir=d, fill=float("nan"))
        R = MultiFab(lev, nv, 1, facedir=d, fill=float("nan"))
        if fo or order == 1:
            HyperbolicSystem.ReconstructStatesConstant(lev, d, prim, L, R, 1, nv)
        elif order == 2:
            HyperbolicSystem.ReconstructStatesPLM(lev, d, capi.LIMITER_MINMOD, prim, L, R, 1, nv)
        else:
            HyperbolicSystem.ReconstructStatesPPM(lev, d, prim, L, R, 1, nv)
        if not fo:
            hs.FlattenShocks(lev, d, prim, chis[0], chis[1] if ndim > 1 else None, chis[2] if ndim > 2 else None, L, R, 1, nv)
        f = MultiFab(lev, nv, 0, facedir=d)
        v = MultiFab(lev, 1, 0, facedir=d)
        hs.ComputeFluxes(lev, riemann if riemann is not None else (capi.RIEMANN_LLF if fo else capi.RIEMANN_HLLC), d, f, v, L, R, prim, K_visc)
        F.append(f.fab_numpy(0))
        V.append(v.fab_numpy(0)[0])
    torch.cuda.synchronize()
    return F, V, prim.fab_numpy(0), [c.fab_numpy(0)[0] for c in chis]


@pytest.mark.parametrize("reconstruct_eint", [False, True])
@pytest.mark.parametrize("order", [3, 2, 1, 0])
def test_flux_pipeline_bit_exact_random_3d(ctx, oracle, reconstruct_eint, order):
    rng = np.random.default_rng(1234 + order)
    n, ng = 20, 4
    shape = (n + 2 * ng,) * 3
    U = random_state(rng, shape)
    vlo, vhi = [0, 0, 0], [n - 1] * 3
    to = pyoracle.traits(1.4, reconstruct_eint, 3)
    tg = capi.traits(1.4, reconstruct_eint, 3)
    fo = order == 0
    Fo, Vo = oracle.compute_hydro_fluxes(to, order, U, vlo, vhi)
    Fg, Vg, prim, chis = gpu_fluxes(ctx, tg, U, vlo, vhi, order, fo=fo)
    glo, ghi = [-ng] * 3, [n - 1 + ng] * 3
    assert np.array_equal(prim, oracle.cons_to_prim(to, U, glo, ghi))
    if not fo:
        for d in range(3):
            co = oracle.flattening_coefficients(to, d, prim, glo, ghi, [-2] * 3, [n + 1] * 3)
            assert np.array_equal(co, chis[d]), f"chi dir {d}"
            assert (co < 1.0).any(), "test state has no shock: flattening untested"
    for d in range(3):
        assert np.array_equal(Fo[d], Fg[d]), f"flux dir {d}: max diff {np.abs(Fo[d] - Fg[d]).max()}"
        assert np.array_equal(Vo[d], Vg[d]), f"face velocity dir {d}"


def test_flux_pipeline_bit_exact_on_sedov_state(ctx, oracle):
    """Golden ghost-filled Sedov state after 10 steps (E_int floor path, strong blast)."""
    U = np.load(os.path.join(HERE, "golden", "sedov_32_step10_ghosted.npz"))["state"]
    vlo, vhi = [0, 0, 0], [31, 31, 31]
    to, tg = pyoracle.traits(1.4, False, 3), capi.traits(1.4, False, 3)
    for order in (3, 0):
        Fo, Vo = oracle.compute_hydro_fluxes(to, order, U, vlo, vhi)
        Fg, Vg, _, _ = gpu_fluxes(ctx, tg, U, vlo, vhi, order, fo=(order == 0))
        for d in range(3):
            assert np.array_equal(Fo[d], Fg[d]) and np.array_equal(Vo[d], Vg[d])


def test_flux_pipeline_bit_exact_1d(ctx, oracle):
    rng = np.random.default_rng(7)
    n, ng = 200, 4
    U3 = random_state(rng, (1, 1, n + 2 * ng))
    vlo, vhi = [0, 0, 0], [n - 1, 0, 0]
    to, tg = pyoracle.traits(1.4, True, 1), capi.traits(1.4, True, 1)
    for order in (3, 2, 0):
        Fo, Vo = oracle.compute_hydro_fluxes(to, order, U3, vlo, vhi)
        Fg, Vg, _, _ = gpu_fluxes(ctx, tg, U3, vlo, vhi, order, ndim=1, fo=(order == 0))
        assert np.array_equal(Fo[0], Fg[0]) and np.array_equal(Vo[0], Vg[0])


def test_artificial_viscosity_path(ctx, oracle):
    rng = np.random.default_rng(99)
    n, ng = 12, 4
    U = random_state(rng, (n + 2 * ng,) * 3)
    vlo, vhi = [0, 0, 0], [n - 1] * 3
    to, tg = pyoracle.traits(1.4, True, 3), capi.traits(1.4, True, 3)
    Fo, Vo = oracle.compute_hydro_fluxes(to, 3, U, vlo, vhi, K_visc=0.1)
    Fg, Vg, _, _ = gpu_fluxes(ctx, tg, U, vlo, vhi, 3, K_visc=0.1)
    for d in range(3):
        assert np.array_equal(Fo[d], Fg[d]) and np.array_equal(Vo[d], Vg[d])


def test_unsupported_and_invalid_arguments_fail_loudly(ctx):
    lev = Level(ctx, 3, [([0, 0, 0], [7, 7, 7])])
    mf = MultiFab(lev, 6, 4, fill=1.0)
    for bad in (capi.traits(1.4, True, 3, nscalars=9), capi.traits(1.4, True, 3, nscalars=1, nmscalars=2), capi.traits(1.4, True, 4),
                capi.traits(1.4, True, 3, eos_temperature_model=1, eos_alpha=0.0)):  # > QK_MAX_SCALARS, more mass than passive scalars, ndim 4, T^4 material without alpha
        with pytest.raises(capi.QkError):
            HydroSystem(bad).ConservedToPrimitive(lev, mf, mf, 4)
    with pytest.raises(capi.QkError):
        HyperbolicSystem.ReconstructStatesPPM(lev, 7, mf, mf, mf, 1, 6)


# ------------------------------------------------------------------ HLLD with the reference's B = 0 stub (hydro_system.hpp:987-1003, HLLD.hpp)
@pytest.mark.parametrize("reconstruct_eint", [False, True])
def test_hlld_stub_fluxes_bit_exact_random_3d(ctx, oracle, reconstruct_eint):
    """ComputeFluxes<RiemannSolver::HLLD, DIR> as the reference instantiates it for Physics_Traits::is_mhd_enabled problems — bx = 0, zero
    transverse fields — against the oracle's statement-by-statement restatement of HLLD.hpp: fluxes and face velocities of all three
    directions, every bit; and it is NOT the HLLC flux (different wave-speed estimates), except that no internal-energy flux exists."""
    rng = np.random.default_rng(77)
    n, ng = 16, 4
    U = random_state(rng, (n + 2 * ng,) * 3)
    tr_o, tr_g = pyoracle.traits(1.4, reconstruct_eint, 3), capi.traits(1.4, reconstruct_eint, 3)
    Fo, Vo = oracle.compute_hydro_fluxes(tr_o, 3, U, [0] * 3, [n - 1] * 3, mhd_stub=True)
    Fg, Vg, _, _ = gpu_fluxes(ctx, tr_g, U, [0] * 3, [n - 1] * 3, 3, riemann=capi.RIEMANN_HLLD)
    Fc, _, _, _ = gpu_fluxes(ctx, tr_g, U, [0] * 3, [n - 1] * 3, 3)
    for d in range(3):
        assert np.array_equal(Fo[d], Fg[d]) and np.array_equal(Vo[d], Vg[d]), d
        assert not Fg[d][5].any()  # HLLD.hpp:331: {rho, mx, my, mz, E, 0.0}
        assert not np.array_equal(Fg[d][:5], Fc[d][:5])
        # same physics: the two approximate solvers agree to a few per cent of the flux scale on these smooth random states
        assert np.abs(Fg[d][:5] - Fc[d][:5]).sum() < 0.2 * np.abs(Fc[d][:5]).sum()


@pytest.mark.parametrize("nscalars,dual", [(0, 1), (2, 1), (0, 0)])
def test_fixup_state_equals_its_three_operators(ctx, nscalars, dual):
    """qk_hydro_FixupState (EnforceLimits + SyncDualEnergy in one pass, CFL maxima reduced on the way out: what every level of an AMR hierarchy
    runs after reflux + average-down, reference src/QuokkaSimulation.hpp:761-770) against qk_hydro_EnforceLimits, qk_hydro_SyncDualEnergy and
    qk_hydro_maxSignalSpeedLocal(0 / 1) on a state with cells under the density floor, under the temperature floor and on both branches of the
    dual-energy switch: state and both maxima bit for bit, two boxes, ghost cells untouched."""
    rng = np.random.default_rng(11)
    tr = capi.traits(1.4, True, 3)
    tr.nscalars = nscalars
    nc = 6 + nscalars
    boxes = [([0, 0, 0], [15, 11, 9]), ([16, 0, 0], [31, 11, 9])]
    lev = Level(ctx, 3, boxes)
    hs = HydroSystem(tr)
    A, B = MultiFab(lev, nc, 4), MultiFab(lev, nc, 4)
    for b, (lo, hi) in enumerate(boxes):
        shape = tuple(hi[d] - lo[d] + 1 + 8 for d in (2, 1, 0))
        U = np.zeros((nc,) + shape)
        U[:6] = random_state(rng, shape)
        U[0] = np.where(rng.random(shape) < 0.1, 1e-4, U[0])            # below the density floor
        U[4] = np.where(rng.random(shape) < 0.1, 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / U[0] * (1 + 1e-6), U[4])  # Eint_cons <= eta Etot; cold
        for n in range(nscalars):
            U[6 + n] = rng.random(shape)
        A.set_fab(b, U)
        B.set_fab(b, U)
    rho_floor, T_floor = 1e-2, 1.2e-8  # (code units: T = P / rho x 1.2e-8 K here, so part of the cells is colder)
    err = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    hs.EnforceLimits(lev, rho_floor, T_floor, A)
    if dual:
        hs.SyncDualEnergy(lev, A, err)
    want = [float(hs.maxSignalSpeedLocal(lev, A, which=w).item()) for w in (0, 1)]
    sig = torch.full((2,), -1.0, dtype=torch.float64, device=ctx.device)
    err2 = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    ctx.check(ctx.L.qk_hydro_FixupState(lev.h, ctx.stream(), C.byref(tr), rho_floor, T_floor, dual, B.ptr, C.c_void_p(err2.data_ptr()), C.c_void_p(sig.data_ptr())),
              "qk_hydro_FixupState")
    torch.cuda.synchronize()
    for b in range(2):
        assert np.array_equal(A.fab_numpy(b), B.fab_numpy(b)), b
    assert sig.tolist() == want and int(err.item()) == int(err2.item()) == 0
    assert float((B.valid(0)[0] == rho_floor).sum()) > 0  # the floor acted
