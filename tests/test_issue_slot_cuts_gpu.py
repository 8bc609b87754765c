"""The marching sweeps after three cuts of FP64 issue slots (csrc/qk_hydro_fused.hip, csrc/qk_device.hpp): the limiters' sign factor without integers
(halfSgnSum), the two quotients by a grid spacing on a reciprocal refined once per launch (divBySpacing), and D_y of the x faces taken from the
march's register window instead of the pre-pass's array (FUSEX).  None of them may move a bit:

  * carried form, X sweep inside the Y march (QK_FUSEX=1: D_y from the window, both quotients on reciprocals) against the four-launch path
    (QK_FUSEX=0: D_y as the pre-pass stored it, k_sweep_x's quotient by `/`): every bit after two steps;
  * exact form (flux_rk2 = 0.5 F1 + 0.5 F2) against the CPU oracle, whose limiters use the integer sign and whose quotients are IEEE: every bit.

On the smallest shapes on which FUSEX and its batch pass run — one 64 x 16 x 16 box, and two of them side by side in x —, reflecting walls, from
the developed blast with what the cuts are sensitive to planted in it: a slab exactly at rest (every slope and every velocity difference a zero:
the sign factor's k = 0, the quotients' zero numerators), a uniform slab in motion (flat: the extremum branch of ppmEdges in every variable) and
momenta of -0.0 in the slab at rest (a velocity divergence of -0, which `/` keeps and a bare reciprocal multiply-and-correct loses)."""
import numpy as np
import pytest

from oracle.pyoracle import SEDOV
from quokka_amd import capi
from quokka_amd.simulation import developed_state, sedov_problem
from test_arith_primitives_gpu import bits, ev, mant
from test_carried_form_oracle_gpu import assert_same, fusex, gather_gpu, gather_oracle

pytestmark = pytest.mark.gpu
N = 64
GEOMETRIES = {"A: one 64x16x16 box": [64, 16, 16], "B: two 64x16x16 boxes side by side in x": [128, 16, 16]}
MGS = [64, 16, 16]
SHELL_RADIUS = {64: 0.62, 128: 0.85}  # in units of the x edge (planted_state)


def planted_state(lo, hi, nx, ng=4):
    """developed_state with the nx cells of the domain's x edge as the unit of length and the shell at SHELL_RADIUS of it: the shell crosses box A
    and the second box of B, and the far field ends 8.5 shell widths outside it, where the velocities are still above 1e-50.  (Further out
    exp(-((r - R) / w)^2) runs through 1e-150 ... 1e-300 on its way to an exact zero; products of such velocities are subnormal, outside the range
    in which qk_device.hpp's divisions are the bits of `/` (2^-996, tests/test_arith_primitives_gpu.py) — a documented limit of the Riemann path,
    not this module's subject, which the slab at rest would show: a momentum of 2.5e-308 in it came out one subnormal ulp from the oracle's.)
    On the ghosted fab [lo - ng, hi + ng], planted by GLOBAL cell index (every box sees the same field; the ghost cells are refilled):
    y in 3..6: gas exactly at rest with the blast's density and pressure, x momentum -0.0 in every other cell of rows 4 and 5 and y, z momenta -0.0
    in row 5; y in 10..12: a uniform slab (rho 1.3, v = (0.4, -0.2, 0.1), P 0.7)"""
    U = developed_state(nx, lo, hi, ng=ng, R=SHELL_RADIUS[nx])
    idx = [np.arange(lo[d] - ng, hi[d] + ng + 1) for d in range(3)]
    k, j, i = np.meshgrid(idx[2], idx[1], idx[0], indexing="ij")
    rest = (j >= 3) & (j <= 6)
    U[4] = np.where(rest, U[5], U[4])
    for n in (1, 2, 3):
        U[n] = np.where(rest, 0.0, U[n])
    U[1] = np.where(rest & ((j == 4) | (j == 5)) & (i % 2 == 0), -0.0, U[1])
    U[2] = np.where(rest & (j == 5), -0.0, U[2])
    U[3] = np.where(rest & (j == 5), -0.0, U[3])
    flat = (j >= 10) & (j <= 12)
    rho, v, P = 1.3, (0.4, -0.2, 0.1), 0.7
    for n, val in enumerate([rho, rho * v[0], rho * v[1], rho * v[2], P / 0.4 + 0.5 * rho * (v[0] ** 2 + v[1] ** 2 + v[2] ** 2), P / 0.4]):
        U[n] = np.where(flat, val, U[n])
    return U


def gpu_run(ctx, n_cell, carry, fusex_on, nsteps):
    with fusex(fusex_on):
        s = sedov_problem(ctx, N, max_grid_size=MGS, n_cell=n_cell)
        s.rk2_carry_rhs = carry
        for b, (lo, hi) in enumerate(s.my_boxes):
            s.state_new_cc_.set_fab(b, planted_state(lo, hi, n_cell[0]))
        s._signal_of_state_new = None
        dts = []
        for _ in range(nsteps):
            assert s.step()
            dts.append(s.dt_)
    return s, dts


@pytest.mark.parametrize("nx", [64, 128])
def test_the_planted_state_holds_what_it_says(nx):
    U = planted_state([0, 0, 0], [nx - 1, 15, 15], nx)[:, 4:-4, 4:-4, 4:-4]
    assert (U[1:4, :, 3:7, :] == 0.0).all() and np.signbit(U[1, :, 4, 0::2]).all() and not np.signbit(U[1, :, 4, 1::2]).any()
    assert np.signbit(U[2, :, 5, :]).all() and np.signbit(U[3, :, 5, :]).all() and not np.signbit(U[2, :, 4, :]).any()
    assert all(np.ptp(U[n, :, 10:13, :]) == 0.0 for n in range(6))
    assert U[0].max() > 2.0 and np.abs(U[1]).max() > 1.0 and U[0, :, :, nx - 64:].max() > 2.0  # (the shell crosses the last box)
    v = np.abs(U[1:4] / U[0])
    assert v[v > 0].min() > 1e-50


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_carried_form_with_the_x_sweep_inside_the_y_march_equals_the_four_launch_path(ctx, geometry):
    n_cell = GEOMETRIES[geometry]
    finals = []
    for on in (False, True):
        s, dts = gpu_run(ctx, n_cell, True, on, 2)
        assert s.lev.nboxes == n_cell[0] // 64
        finals.append((gather_gpu(s, n_cell), dts))
    assert finals[0][1] == finals[1][1]
    assert np.isfinite(finals[0][0]).all()
    assert_same(finals[1][0], finals[0][0], f"{geometry}: QK_FUSEX=1 against QK_FUSEX=0")
    assert np.array_equal(np.signbit(finals[1][0]), np.signbit(finals[0][0]))  # (array_equal takes -0 for +0)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_exact_form_equals_the_oracle(ctx, oracle, geometry):
    n_cell = GEOMETRIES[geometry]
    so = oracle.sim(SEDOV, 3, n_cell, [0, 0, 0], [1.2 * c / N for c in n_cell], [0, 0, 0], max_grid_size=MGS)
    for b in range(so.nboxes):
        lo, hi = so.box(b)
        so.set_state(planted_state(lo, hi, n_cell[0]), b, 0)
    dto = []
    for _ in range(2):
        assert so.step()
        dto.append(so.dt)
    s, dts = gpu_run(ctx, n_cell, False, True, 2)
    assert dts == dto, (dts, dto)
    Uo, Ug = gather_oracle(so, n_cell), gather_gpu(s, n_cell)
    assert_same(Ug, Uo, geometry)
    assert np.array_equal(np.signbit(Ug), np.signbit(Uo))


def test_quotient_by_a_spacing_keeps_the_bits_and_the_sign_of_a_zero(ctx):
    """divBySpacing over what the sweeps hand it: spacings 1.2 / n and powers of two, numerators over +-40 binades around the spacing and zeros of
    either sign — the bits of IEEE `/`, the sign of a zero quotient included (divBy alone gives +0 for -0 / dx)"""
    r = np.random.default_rng(21)
    n = 1 << 16
    dx = np.where(r.random(n) < 0.5, 1.2 / r.integers(8, 4097, n), np.ldexp(1.0, r.integers(-12, 3, n)))
    a = np.ldexp(mant(r, n), r.integers(-40, 41, n)) * dx * np.where(r.random(n) < 0.5, -1.0, 1.0)
    a[: n // 8] = np.where(r.random(n // 8) < 0.5, -0.0, 0.0)
    with np.errstate(all="ignore"):
        want = a / dx
    got = ev(ctx, capi.ARITH_DIVBY_SPACING, a, dx)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(np.signbit(got[: n // 8]), np.signbit(a[: n // 8])) and np.signbit(a[: n // 8]).any()
