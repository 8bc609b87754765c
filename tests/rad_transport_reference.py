"""What the tests of the radiation TRANSPORT kernels share (tests/test_rad_transport_reference.py on the CPU, tests/test_rad_transport_cells_gpu.py on
the GPU): an independent 50-digit restatement of one HLL face flux, seeded generators of faces and of ghost-filled levels with a share of invalid
cells, the named faces that sit on a branch each, and the seams of the kernels' decompositions.

The flux formulas (reference src/radiation/radiation_system.hpp:773-790, :873-983, :1054-1131), written from the equations and not from the oracle:

  chi(f)  = (3 + 4 f^2) / (5 + 2 sqrt(4 - 3 f^2))                    Levermore's closure (or 1/3: the Eddington approximation)
  T_ij    = (1 - chi)/2 delta_ij + (3 chi - 1)/2 n_i n_j,  n = f / |f|
  F(U)    = (c_hat / c F_n,  c_hat c T_nj E),   U = (E, F) = (E, c E f)
  S_R     = c_hat max(0.1, sqrt(T_nn,R)),  S_L = -c_hat max(0.1, sqrt(T_nn,L))
  F_HLL   = (S_R F(U_L) - S_L F(U_R) + epsilon S_R S_L (U_R - U_L)) / (S_R - S_L),   epsilon = (eps, 1, 1, 1)
"""
from __future__ import annotations

import numpy as np

from dataclasses import dataclass
from functools import lru_cache

from oracle.pyoracle import RAD_FACE_BIT, RadCellTraits

C_CGS, CHAT_CGS = 2.99792458e10, 2.99792458e9  # the random sets: c_hat = 0.1 c
C_EXACT, CHAT_EXACT = 1024.0, 64.0             # the named faces: F = f c E and F / (c E) are exact for E a power of two

# Oracle against the 50-digit flux, 2e4 admissible faces per direction and closure (seeds 1 .. 6), largest error over all sets and components.
# In ulps of the largest of the three terms of the HLL sum: 13061.5 (transverse momentum flux, chi = 1/3, direction 0) — not "a few".  The third term
# holds U_R - U_L, the difference of two products f (c E) rounded twice each, and two cells that carry nearly the same flux cancel it: the error is a
# few ulps of those PRODUCTS, any number of ulps of their difference.
# In ulps of the largest rounded operand (mp_face_flux: the terms, the two products, the isotropic pressure): 28.11 (energy flux, Levermore, direction
# 2).  That is rounding as well: across a beam (f -> 1 along the face) T_nn = (1 - chi) / 2 cancels down to the floor 0.01 of the wave speed, which
# magnifies the half ulp of chi a hundredfold, the square root halves it, and S enters every term.  Nothing beyond rounding was found in the oracle.
# Each cap is twice the measured maximum, rounded up.
ORACLE_ULP_MEASURED_TERMS = 13061.5
ORACLE_ULP_CAP_TERMS = 26123.0
ORACLE_ULP_MEASURED_OPERANDS = 28.11
ORACLE_ULP_CAP_OPERANDS = 57.0

# Where the transport entries equal the reference in every bit (include/quokka_amd.h), from the ladders of tests/test_rad_transport_cells_gpu.py
PARITY_CE = (2.0 ** -996, 2.0 ** 1004)  # c E of both cells of a face
PARITY_F = 1.0e-200                     # |f| from here to 1: the whole ladder, f^2 subnormal or zero at its lower end


def cell_traits(c=C_CGS, chat=CHAT_CGS, floor=0.0, eddington=0) -> RadCellTraits:
    t = RadCellTraits()
    t.c_light, t.c_hat, t.radiation_constant, t.Erad_floor = c, chat, 7.5657e-15, floor
    t.gamma, t.mean_molecular_weight, t.boltzmann_constant = 5.0 / 3.0, 1.0, 1.0
    t.beta_order, t.opacity_model, t.pow_mode, t.eddington_model = 1, 0, 1, eddington
    return t


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """element-wise: the same bit pattern, or a NaN in both"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------ the independent flux
def mp_face_flux(direction: int, pL, pR, c: float, chat: float, eps: float, eddington: int):
    """(F[4], scale, operands) of one face between admissible states p = (E, fx, fy, fz), 50 digits.  scale: the largest of the three terms of the HLL
    sum per component.  operands: the largest magnitude that is ROUNDED on the way to the component — the three terms, the two products whose
    difference U_R - U_L the third term holds, and (momentum components) the isotropic pressure c_hat c E / 2 (1 - chi) under which 1 - chi cancels."""
    import mpmath as mp
    mp.mp.dps = 50
    c, chat, eps = mp.mpf(c), mp.mpf(chat), mp.mpf(eps)

    def side(p):
        E = mp.mpf(float(p[0]))
        f = [mp.mpf(float(v)) for v in p[1:]]
        fn = mp.sqrt(sum(v * v for v in f))
        chi = mp.mpf(1) / 3 if eddington == 1 else (3 + 4 * fn * fn) / (5 + 2 * mp.sqrt(4 - 3 * fn * fn))
        n = [v / fn for v in f] if fn > 0 else [mp.mpf(0)] * 3
        T = [(1 - chi) / 2 * (1 if j == direction else 0) + (3 * chi - 1) / 2 * n[direction] * n[j] for j in range(3)]
        U = [E] + [c * E * v for v in f]
        F = [chat / c * U[1 + direction]] + [chat * c * T[j] * E for j in range(3)]
        S = chat * max(mp.mpf("0.1"), mp.sqrt(T[direction]))
        return U, F, S

    UL, FL, SL = side(pL)
    UR, FR, SR = side(pR)
    SL = -SL
    out, scale, operands = [], [], []
    for n in range(4):
        e = eps if n == 0 else 1
        w = e * SR * SL / (SR - SL)
        terms = (SR * FL[n] / (SR - SL), SL * FR[n] / (SR - SL), w * (UR[n] - UL[n]))
        out.append(terms[0] - terms[1] + terms[2])
        scale.append(max(abs(t) for t in terms))
        inside = [abs(w * UR[n]), abs(w * UL[n])]
        if n > 0:
            inside += [abs(SR / (SR - SL) * chat * c * UL[0]), abs(SL / (SR - SL) * chat * c * UR[0])]
        operands.append(max([scale[-1]] + inside))
    return out, scale, operands


def ulps_off(got: float, want, scale) -> float:
    """|got - want| in ulps of `scale` (mpmath numbers in, float out)"""
    import mpmath as mp
    s = float(scale)
    if s == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return float(abs(mp.mpf(got) - want) / mp.mpf(float(np.spacing(s))))


# ------------------------------------------------------------------ random faces
def _directions(rng, n, aligned_share=0.3):
    d = rng.normal(size=(3, n))
    d /= np.sqrt((d * d).sum(axis=0))
    al = rng.random(n) < aligned_share
    ax = rng.integers(0, 3, n)
    sg = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    for a in range(3):
        d[a] = np.where(al, np.where(ax == a, sg, 0.0), d[a])
    return d


def random_cells(rng, n, c, fmax=1.2, decades=30.0):
    """cons[4, n]: E log-uniform over `decades` around 1, |f| uniform in [0, fmax], directions random with an axis-aligned share"""
    E = 10.0 ** rng.uniform(-0.5 * decades, 0.5 * decades, n)
    f = rng.uniform(0.0, fmax, n)
    d = _directions(rng, n)
    return np.stack([E] + [f * d[a] * (c * E) for a in range(3)])


def random_faces(oracle, seed: int, n: int, c=C_CGS, chat=CHAT_CGS, admissible=False):
    """n faces: (direction[n], pL, pR, consL, consR [4, n], eps[n]).  The face states are the cells' primitives on half of the faces and moved a
    quarter of the way to the other cell on the rest (what a reconstruction does); the two cells of a face lie within three decades of each other.
    admissible: |f| < 1 on both sides, so that no face takes the fallback (the faces the 50-digit flux covers)."""
    rng = np.random.default_rng(seed)
    fmax = 0.999 if admissible else 1.2
    cL = random_cells(rng, n, c, fmax)
    cR = random_cells(rng, n, c, fmax)
    ratio = 10.0 ** rng.uniform(-3.0, 3.0, n) * cL[0] / cR[0]
    cR = cR * ratio
    t = cell_traits(c, chat)
    qL, qR = oracle.rad_cons_to_prim(t, cL), oracle.rad_cons_to_prim(t, cR)
    moved = rng.random(n) < 0.5
    pL = np.where(moved, qL + 0.25 * (qR - qL), qL)
    pR = np.where(moved, qR - 0.25 * (qR - qL), qR)
    if admissible:  # (a convex combination of two reduced fluxes inside the unit ball stays inside)
        assert np.all((pL[1:] ** 2).sum(axis=0) < 1.0) and np.all((pR[1:] ** 2).sum(axis=0) < 1.0)
    direction = rng.integers(0, 3, n).astype(np.int32)
    eps = np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.01, 1.0, n))
    return direction, pL, pR, np.ascontiguousarray(cL), np.ascontiguousarray(cR), eps


# ------------------------------------------------------------------ the named faces
def _cons(E, f, c):
    return np.array([E, f[0] * (c * E), f[1] * (c * E), f[2] * (c * E)])


def targeted_faces(c=C_EXACT):
    """The faces that sit on one branch each.  Returns (names, direction[n], pL, pR, consL, consR [4, n], want) — want[name] = (bits that must be
    set, bits that must be clear) of RAD_FACE_BIT.  The face states are the cells' own (E, f), given exactly; c = 1024 and E = 1 make F = f c E exact."""
    B = RAD_FACE_BIT
    four = B["erad_L_le_0"] | B["erad_R_le_0"] | B["f_L_ge_1"] | B["f_R_ge_1"]
    ok_L, ok_R = (1.0, (0.3, 0.1, -0.2)), (2.0, (-0.2, 0.25, 0.1))
    one = float(np.nextafter(1.0, 0.0))
    cases = []

    def add(name, L, R, must, mustnot, d=0, pL=None, pR=None):
        cL, cR = _cons(L[0], L[1], c), _cons(R[0], R[1], c)
        pl = np.array([L[0], *L[1]]) if pL is None else np.array([pL[0], *pL[1]])
        pr = np.array([R[0], *R[1]]) if pR is None else np.array([pR[0], *pR[1]])
        cases.append((name, d, pl, pr, cL, cR, must, mustnot))

    fb = B["fallback"]
    add("trigger_erad_L", (-1.0, ok_L[1]), ok_R, fb | B["erad_L_le_0"], four & ~B["erad_L_le_0"] | B["nonfinite"])
    add("trigger_erad_R", ok_L, (-2.0, ok_R[1]), fb | B["erad_R_le_0"], four & ~B["erad_R_le_0"] | B["nonfinite"])
    add("trigger_f_L", (1.0, (1.2, 0.0, 0.0)), ok_R, fb | B["f_L_ge_1"] | B["clamp_L"], four & ~B["f_L_ge_1"] | B["nonfinite"])
    add("trigger_f_R", ok_L, (2.0, (0.0, -1.1, 0.0)), fb | B["f_R_ge_1"] | B["clamp_R"], four & ~B["f_R_ge_1"] | B["nonfinite"], d=1)
    for k, f in enumerate(((0.6, 0.8, 0.0), (0.36, 0.48, 0.8), (1.0, 0.0, 0.0))):
        for d in range(3):
            add(f"f_exactly_1_{k}_dir{d}", (1.0, f), ok_R, fb | B["f_L_ge_1"], four & ~B["f_L_ge_1"] | B["clamp_L"] | B["nonfinite"], d=d)
    add("f_just_below_1", (1.0, (one, 0.0, 0.0)), ok_R, 0, fb | four | B["nonfinite"])
    add("f_just_below_1_R", ok_L, (1.0, (0.0, 0.0, -one)), 0, fb | four | B["nonfinite"], d=2)
    add("f_1_perpendicular", (1.0, (0.0, 1.0, 0.0)), ok_R, fb | B["f_L_ge_1"] | B["S_floor_L"], B["clamp_L"] | B["S_floor_R"] | B["nonfinite"], d=0)
    add("f_1_perpendicular_R", ok_L, (1.0, (0.0, 0.0, -1.0)), fb | B["f_R_ge_1"] | B["S_floor_R"], B["clamp_R"] | B["S_floor_L"] | B["nonfinite"], d=1)
    add("f_0_left", (1.0, (0.0, 0.0, 0.0)), ok_R, B["no_dir_L"], fb | B["no_dir_R"] | B["nonfinite"])
    add("f_0_right", ok_L, (1.0, (0.0, 0.0, 0.0)), B["no_dir_R"], fb | B["no_dir_L"] | B["nonfinite"], d=2)
    add("f_0_both", (1.0, (0.0, 0.0, 0.0)), (4.0, (0.0, 0.0, 0.0)), B["no_dir_L"] | B["no_dir_R"], fb | B["nonfinite"], d=1)
    # the face states are fine on the left, the right one has no energy: the fallback reads the left CELL, whose reduced flux is 1.3
    add("fallback_onto_f_gt_1", (1.0, (1.3, 0.0, 0.0)), (-1.0, ok_R[1]), fb | B["erad_R_le_0"] | B["clamp_L"], B["f_L_ge_1"] | B["nonfinite"], pL=(1.0, (0.5, 0.0, 0.0)))
    add("fallback_onto_f_gt_1_R", (-1.0, ok_L[1]), (1.0, (0.0, 0.78, 1.04)), fb | B["erad_L_le_0"] | B["clamp_R"], B["f_R_ge_1"] | B["nonfinite"], d=2,
        pR=(1.0, (0.0, 0.3, 0.4)))
    add("E_0_F_0", (0.0, (0.0, 0.0, 0.0)), ok_R, fb | B["erad_L_le_0"] | B["no_dir_L"] | B["nonfinite"], 0)
    add("E_0_F_0_R", ok_L, (0.0, (0.0, 0.0, 0.0)), fb | B["erad_R_le_0"] | B["no_dir_R"] | B["nonfinite"], 0, d=1)
    add("E_lt_0_both", (-1.0, ok_L[1]), (-3.0, ok_R[1]), fb | B["erad_L_le_0"] | B["erad_R_le_0"], B["nonfinite"])
    names = [k[0] for k in cases]
    arr = [np.ascontiguousarray(np.stack([k[i] for k in cases], axis=1)) for i in (2, 3, 4, 5)]
    direction = np.array([k[1] for k in cases], dtype=np.int32)
    # E = 0 with flux: the conserved flux cannot come from f c E
    extra = []
    for k, F in enumerate(((3.0, 0.0, 0.0), (0.0, -2.0, 5.0), (1.0, 2.0, -3.0))):
        for d in range(3):
            extra.append((f"E_0_F_{k + 1}_components_dir{d}", d, np.array([0.0, *F])))
    pl = np.array([ok_L[0], *ok_L[1]])
    for name, d, U in extra:
        names.append(name)
        direction = np.append(direction, np.int32(d))
        # the face state of the empty cell: its own primitives, F / (c 0) = +-inf or NaN
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.array([0.0, *(U[1:] / (c * 0.0))])
        arr[0] = np.concatenate([arr[0], pl[:, None]], axis=1)
        arr[1] = np.concatenate([arr[1], q[:, None]], axis=1)
        arr[2] = np.concatenate([arr[2], _cons(*ok_L, c)[:, None]], axis=1)
        arr[3] = np.concatenate([arr[3], U[:, None]], axis=1)
    want = {k[0]: (k[6], k[7]) for k in cases}
    for name, d, U in extra:
        want[name] = (fb | B["erad_R_le_0"] | B["nonfinite"], 0)
    return names, direction, arr[0], arr[1], arr[2], arr[3], want


def ladder_E(c=C_EXACT):
    """(E[n], direction, pL, pR, consL, consR): a face between (E, f_L) and (2 E, f_R) for E = 1e-300 ... 1e300, two steps per decade"""
    E = 10.0 ** np.arange(-300.0, 300.5, 0.5)
    fL, fR = np.array([0.3, 0.1, -0.2]), np.array([-0.2, 0.25, 0.1])
    with np.errstate(over="ignore"):
        cL = np.stack([E] + [fL[a] * (c * E) for a in range(3)])
        cR = np.stack([2.0 * E] + [fR[a] * (c * (2.0 * E)) for a in range(3)])
    pL = np.stack([E] + [np.full_like(E, fL[a]) for a in range(3)])
    pR = np.stack([2.0 * E] + [np.full_like(E, fR[a]) for a in range(3)])
    return E, np.zeros(E.size, dtype=np.int32), pL, pR, cL, cR


def ladder_f(c=C_EXACT):
    """(|f|[n], direction, pL, pR, consL, consR): a face between (1, |f| n_L) and (2, 0.5 |f| n_R) for |f| = 1e-200 ... 1, two steps per decade"""
    f = np.minimum(10.0 ** np.arange(-200.0, 0.25, 0.5), float(np.nextafter(1.0, 0.0)))
    nL, nR = np.array([0.6, 0.0, 0.8]), np.array([0.0, -1.0, 0.0])
    pL = np.stack([np.ones_like(f)] + [f * nL[a] for a in range(3)])
    pR = np.stack([np.full_like(f, 2.0)] + [0.5 * f * nR[a] for a in range(3)])
    cL = np.stack([pL[0]] + [pL[1 + a] * (c * pL[0]) for a in range(3)])
    cR = np.stack([pR[0]] + [pR[1 + a] * (c * pR[0]) for a in range(3)])
    return f, np.full(f.size, 2, dtype=np.int32), pL, pR, cL, cR


# ------------------------------------------------------------------ levels with a share of invalid cells
# X seams of one 40-cell box with 4 ghost cells (rows of 48 slab positions): the first position of every workgroup but the first, as (row, i).
# The flux kernel's workgroups advance by 250 positions, the sweep's by 249.
def x_seams(step: int, n: int = 40, nghost: int = 4):
    rowlen = n + 2 * nghost
    return [(f // rowlen, f % rowlen - nghost) for f in range(step, rowlen * n, step)]


SEAMS_40 = {
    "x_flux": x_seams(250), "x_sweep": x_seams(249),  # (row j, i)
    "y_strips": [16, 32],                                # first cell of a Y strip of the sweep (16 + 16 + 8)
    "z_strips": [32],                                    # first cell of the second Z strip (32 + 8, stage 1 out of place)
    "march_faces": [8, 16, 24, 32, 40],                  # first face of a strip of the flux marches (5 x 8 + the lone last face)
}
assert SEAMS_40["x_flux"] == [(5, 6), (10, 16), (15, 26), (20, 36), (26, -2), (31, 8), (36, 18)]
assert SEAMS_40["x_sweep"] == [(5, 5), (10, 14), (15, 23), (20, 32), (25, 41), (31, 2), (36, 11)]
SEAM_PLANES = (3, 33)  # the planes k (X seams) / pencils (Y, Z seams) in which invalid cells are planted at the seams


def seam_cells_40(nghost: int = 4):
    """(i, j, k) of the cells planted invalid in a 40^3 box: the cell left of every X seam (valid range), the cell before and at every strip start"""
    out = []
    for k in SEAM_PLANES:
        for row, i in SEAMS_40["x_flux"] + SEAMS_40["x_sweep"]:
            out.append((min(max(i - 1, 0), 39), row, k))
        for j in SEAMS_40["y_strips"] + SEAMS_40["march_faces"][:-1]:
            out += [(k, j - 1, 7), (k + 1, j, 7)]
        for kk in SEAMS_40["z_strips"] + SEAMS_40["march_faces"][:-1]:
            out += [(k, 9, kk - 1), (k + 1, 9, kk)]
        out += [(k, 39, 11), (k, 11, 39), (39, k, 11)]  # the cells before the lone last faces
    return sorted(set(out))


def random_level(seed: int, shape, ngroups: int, bad_share: float, floor: float, c=C_CGS, planted=(), nghost: int = 4, ndim: int = 3, quiet_group=None,
                 bad_group=None, negative_zeros=False):
    """U[6 + 4 ngroups, nz, ny, nx] (ghost cells included, filled like any others: the stage fills no boundary).  Energies log-uniform over three
    decades above 10 floor-per-group (or around 1), |f| <= 0.95 in random directions with an axis-aligned share; per group 1 % of the cells
    without flux and 1 % grazing (axis-aligned, 0.99 <= |f| < 1: T_nn < 0.01 across it); a share `bad_share` of the cells invalid in one group, a third each:
    |F| = 1.3 c E, E < 0 and (floor > 0) 0 < E < floor-per-group with f <= 1.  planted: (i, j, k) valid-cell indices made invalid as well, kinds in
    turn.  quiet_group: that group holds half its floor and no flux in every cell — a uniform state, whose flux divergence is exactly zero, so it is
    still valid and below its floor after the stage: the group amendRadState lifts only where ANOTHER group is invalid.  bad_group: the group the
    invalid cells are invalid in (default: a random one per cell).  Returns (U, kind[ngroups, nz, ny, nx]: 0 fine, 1 f = 1.3, 2 E < 0, 3 below the floor)."""
    rng = np.random.default_rng(seed)
    shp = tuple(shape)
    U = np.zeros((6 + 4 * ngroups,) + shp)
    U[0], U[4], U[5] = 1.0, 1.0, 1.0
    fl = floor / ngroups
    E0 = 10.0 * fl if fl > 0 else 1.0
    kind = np.zeros((ngroups,) + shp, dtype=np.int8)
    ncell = int(np.prod(shp))
    which = rng.integers(0, ngroups, shp)  # the group that is invalid in a bad cell
    if quiet_group is not None:
        which = np.where(which == quiet_group, (quiet_group + 1) % ngroups, which)
    if bad_group is not None:
        which = np.full(shp, bad_group)
    bad = rng.random(shp) < bad_share
    nk = 3 if fl > 0 else 2
    k_of = rng.integers(1, nk + 1, shp)
    off = [nghost if d < ndim else 0 for d in (2, 1, 0)]
    for n, (i, j, k) in enumerate(planted):
        idx = (k + off[0], j + off[1], i + off[2])
        bad[idx] = True
        k_of[idx] = 1 + n % nk
    for g in range(ngroups):
        E = E0 * 10.0 ** rng.uniform(0.0, 3.0, shp)
        f = rng.uniform(0.0, 0.95, shp)
        d = _directions(rng, ncell).reshape((3,) + shp)
        r = rng.random(shp)
        f = np.where(r < 0.01, 0.0, f)
        graze = (r >= 0.01) & (r < 0.02)
        ax = rng.integers(0, 3, shp)
        for a in range(3):
            d[a] = np.where(graze, (ax == a) * 1.0, d[a])
        f = np.where(graze, rng.uniform(0.99, 0.9999, shp), f)
        mine = bad & (which == g)
        kind[g] = np.where(mine, k_of, 0)
        f = np.where(kind[g] == 1, 1.3, f)
        E = np.where(kind[g] == 3, fl * rng.uniform(0.1, 0.9, shp), E)
        for a in range(3):
            # (+ 0.0: a component without flux is +0.  Where two of the three cell values PPM's std::minmax compares are zeros of opposite sign, the
            # reference returns one by position and v_min_f64 / v_max_f64 the other by sign: an exactly-zero flux then differs in its sign alone —
            # the tie csrc/qk_device.hpp documents for smin / smax, met in 1-3 of 65600 faces with -0 components in the cells without flux.)
            U[6 + 4 * g + 1 + a] = f * d[a] * (c * E) + (0.0 if not negative_zeros else -0.0)
        U[6 + 4 * g] = np.where(kind[g] == 2, -E, E)
    if quiet_group is not None:
        assert fl > 0
        U[6 + 4 * quiet_group] = 0.5 * fl
        U[6 + 4 * quiet_group + 1: 6 + 4 * quiet_group + 4] = 0.0
        kind[quiet_group] = 0
    return U, kind


def count_bits(mask: np.ndarray, names: dict) -> dict:
    return {k: int(((mask & b) != 0).sum()) for k, b in names.items()}


FACE_BITS_RANDOM = tuple(k for k in RAD_FACE_BIT if k != "nonfinite")            # what a random level with a floor must reach >= 50 times
CELL_BITS_RANDOM = ("invalid_E", "invalid_f", "lifted", "rescaled")             # and, with several groups, "by_other"


# ------------------------------------------------------------------ the stage cases both suites run
FLOOR = 1.0e-3  # RadSystem_Traits::Erad_floor of the levels with a floor (per group: FLOOR / ngroups)
DX = (1.0, 0.5, 2.0)  # three different cell widths: a direction taken for another shows
DT = 0.3 * 0.5 / CHAT_CGS


@dataclass(frozen=True)
class StageCase:
    name: str
    ndim: int
    n: int            # cells per box edge (active dimensions)
    nboxes: int       # 1, or 8 boxes of n^3
    ngroups: int
    bad_share: float
    order: int
    stage: int
    eps: bool
    seed: int
    floor: float = FLOOR
    eddington: int = 0
    bad_group: int = -1    # the group the invalid cells are invalid in (-1: a random one per cell)
    quiet_group: int = -1  # the group that is valid and below its floor everywhere (-1: seed % ngroups where there are several groups and a floor)
    follows: str = ""      # stage 2 only: U_in is the oracle's result of that stage-1 case, U0 its input
    negative_zeros: bool = False  # the components without flux keep the sign of f d c E (random_level)

    @property
    def quiet(self):
        if self.quiet_group >= 0:
            return self.quiet_group
        return (self.seed % self.ngroups) if (self.ngroups > 1 and self.floor > 0) else None

    def boxes(self):
        n = self.n
        if self.nboxes == 1:
            return [([0, 0, 0], [n - 1 if d < self.ndim else 0 for d in range(3)])]
        assert self.nboxes == 8 and self.ndim == 3
        return [([i * n, j * n, k * n], [i * n + n - 1, j * n + n - 1, k * n + n - 1]) for k in (0, 1) for j in (0, 1) for i in (0, 1)]

    def fab_shape(self):
        return tuple(self.n + 8 if d < self.ndim else 1 for d in (2, 1, 0))


# One 40^3 box: every seam of the fused sweeps and of the flux kernels (SEAMS_40), every (order, stage, group count) with the invalid share and the
# wavespeed-correction arrays alternating so that each pair of the two occurs with every order; eight 20^3 boxes: Y strips of 16 + 4 cells, the box
# index in the grid; a 1-D level (the per-face flux kernel) and a 2-D level (the 3-D kernels on one plane).
STAGE_CASES = []
for _n, (_o, _s, _g) in enumerate((o, s, g) for o in (3, 2, 1) for s in (1, 2) for g in (1, 4)):
    _share, _eps = (0.01, 0.30)[(_n + _n // 4) % 2], bool((_n // 2 + _n // 4) % 2)
    STAGE_CASES.append(StageCase(f"box40-o{_o}-s{_s}-g{_g}-{int(100 * _share)}pct" + ("-eps" if _eps else ""), 3, 40, 1, _g, _share, _o, _s, _eps, 101 + _n))
STAGE_CASES += [
    StageCase("box40-o2-s2-g1-1pct-chi13", 3, 40, 1, 1, 0.01, 2, 2, False, 120, eddington=1),
    StageCase("box40-o3-s1-g4-30pct-chi13-eps", 3, 40, 1, 4, 0.30, 3, 1, True, 121, eddington=1),
    StageCase("boxes20-o3-s2-g1-30pct", 3, 20, 8, 1, 0.30, 3, 2, False, 130),
    StageCase("boxes20-o2-s1-g4-1pct-eps", 3, 20, 8, 4, 0.01, 2, 1, True, 131),
    StageCase("line64-o3-s1-g1-30pct", 1, 64, 1, 1, 0.30, 3, 1, False, 140),
    StageCase("line64-o2-s2-g4-30pct-eps", 1, 64, 1, 4, 0.30, 2, 2, True, 141),
    StageCase("line64-o1-s1-g4-30pct", 1, 64, 1, 4, 0.30, 1, 1, False, 142),
    StageCase("plane40-o3-s2-g1-30pct-eps", 2, 40, 1, 1, 0.30, 3, 2, True, 150),
    StageCase("plane40-o2-s1-g4-1pct", 2, 40, 1, 4, 0.01, 2, 1, False, 151),
    StageCase("plane40-o1-s1-g4-30pct", 2, 40, 1, 4, 0.30, 1, 1, False, 152),
]
# The whole-cell verdict: four groups, one (`bad_group`) invalid in 5 % of the cells of a 24^3 box — |F| = 1.3 c E or E < 0 —, another (`quiet_group`)
# valid and below its floor everywhere.  Every ordered pair of positions, the stages and orders in turn.
VERDICT_CASES = [StageCase(f"verdict-bad{a}-quiet{q}", 3, 24, 1, 4, 0.05, 1 + (a + q) % 3, 1 + (a + 2 * q) % 2, False, 200 + 4 * a + q, bad_group=a, quiet_group=q)
                 for a in range(4) for q in range(4) if a != q]
# Erad_floor = 0: the repair of the first stage leaves cells with E = 0, F = +-0, which the second stage reads
FLOOR0_CASES = [StageCase(f"floor0-o{o}-s1", 3, 24, 1, 1, 0.05, o, 1, False, 300 + o, floor=0.0) for o in (1, 2, 3)]
# zeros of both signs in the cells without flux: the one documented difference, the sign of an exactly-zero flux (see random_level)
NEGZERO_CASES = [StageCase(f"negzero-o{o}-s1", 3, 40, 1, 1, 0.01, o, 1, False, 101, negative_zeros=True) for o in (2, 3)]
STAGE_CASE = {c.name: c for c in STAGE_CASES + VERDICT_CASES + FLOOR0_CASES + NEGZERO_CASES}
STAGE_CASE.update({c.name.replace("-s1", "-s2"): StageCase(c.name.replace("-s1", "-s2"), 3, 24, 1, 1, 0.05, c.order, 2, False, c.seed, floor=0.0, follows=c.name)
                   for c in FLOOR0_CASES})


def stage_inputs(case: StageCase):
    """per box: (U_in, U0, eps[3] or None); U0 is U_in itself in stage 1"""
    if case.follows:
        first = stage_inputs(STAGE_CASE[case.follows])
        return [(r[0], U, None) for r, (U, _, _) in zip(stage_reference(case.follows), first)]
    out = []
    for b, (lo, hi) in enumerate(case.boxes()):
        planted = seam_cells_40() if (case.n == 40 and case.ndim == 3) else ()
        share = case.bad_share if case.ndim == 3 else max(case.bad_share, 0.05)
        U, _ = random_level(1000 * case.seed + b, case.fab_shape(), case.ngroups, share, case.floor, planted=planted, ndim=case.ndim, quiet_group=case.quiet,
                            bad_group=case.bad_group if case.bad_group >= 0 else None, negative_zeros=case.negative_zeros)
        U0 = U
        if case.stage == 2:
            U0, _ = random_level(1000 * case.seed + 500 + b, case.fab_shape(), case.ngroups, share, case.floor, ndim=case.ndim, quiet_group=case.quiet)
        eps = None
        if case.eps:
            rng = np.random.default_rng(77 * case.seed + b)
            eps = []
            for d in range(case.ndim):
                n = [hi[a] - lo[a] + 1 + (1 if a == d else 0) for a in range(3)]
                shp = (case.ngroups, n[2], n[1], n[0])
                eps.append(np.where(rng.random(shp) < 0.5, 1.0, rng.uniform(0.01, 1.0, shp)))
        out.append((U, U0, eps))
    return out


_ORACLE = None


def the_oracle():
    global _ORACLE
    if _ORACLE is None:
        from oracle.pyoracle import Oracle
        _ORACLE = Oracle("direct")
    return _ORACLE


@lru_cache(maxsize=None)
def stage_reference(name: str):
    """the oracle's stage of every box of the case: list of (U_new, [flux_d], [face mask_d], cell mask); computed once, read-only"""
    case = STAGE_CASE[name]
    t = cell_traits(floor=case.floor, eddington=case.eddington)
    out = []
    for (lo, hi), (U, U0, eps) in zip(case.boxes(), stage_inputs(case)):
        r = the_oracle().rad_transport_stage(t, case.ngroups, case.ndim, case.order, case.stage, U, U0, lo, hi, DT, DX, eps)
        for a in (r[0], *r[1], *r[2], r[3]):
            a.setflags(write=False)
        out.append(r)
    return out
