"""CPU half of the transport pins (no GPU): the oracle's face flux against an independent 50-digit flux, exact properties of the oracle's flux, and
the conditions on the generated inputs that tests/test_rad_transport_cells_gpu.py relies on — every branch bit it claims is present in the
ORACLE's record, non-numbers only where they are named, an invalid cell at every seam."""
import numpy as np
import pytest

import rad_transport_reference as R
from oracle.pyoracle import RAD_CELL_BIT, RAD_FACE_BIT

B = RAD_FACE_BIT


@pytest.mark.parametrize("eddington", [0, 1])
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_oracle_flux_is_within_rounding_of_the_50_digit_flux(oracle, direction, eddington):
    """2e4 seeded admissible faces (E over 30 decades, |f| < 1, a quarter of the way reconstructed on half of them, eps < 1 on half): the largest
    error of each flux component in ulps of the largest of the three terms of the HLL sum, and in ulps of the largest rounded operand, stays below
    twice the measured maximum (tests/rad_transport_reference.py: the figures and why the first is not "a few")."""
    n = 20000
    _, pL, pR, cL, cR, eps = R.random_faces(oracle, 1 + direction + 3 * eddington, n, admissible=True)
    t = R.cell_traits(eddington=eddington)
    F, mask = oracle.rad_face_fluxes(t, direction, pL, pR, cL, cR, eps)
    assert not np.any(mask & (B["fallback"] | B["nonfinite"]))
    worst, worst_op = np.zeros(4), np.zeros(4)
    for i in range(n):
        want, scale, operands = R.mp_face_flux(direction, pL[:, i], pR[:, i], R.C_CGS, R.CHAT_CGS, eps[i], eddington)
        for c in range(4):
            worst[c] = max(worst[c], R.ulps_off(F[c, i], want[c], scale[c]))
            worst_op[c] = max(worst_op[c], R.ulps_off(F[c, i], want[c], operands[c]))
    print("oracle vs 50 digits, ulps of the largest term / of the largest operand:", direction, eddington, worst, worst_op)
    assert np.all(worst <= R.ORACLE_ULP_CAP_TERMS), worst
    assert np.all(worst_op <= R.ORACLE_ULP_CAP_OPERANDS), worst_op
    assert R.ORACLE_ULP_CAP_TERMS == np.ceil(2.0 * R.ORACLE_ULP_MEASURED_TERMS) and R.ORACLE_ULP_CAP_OPERANDS == np.ceil(2.0 * R.ORACLE_ULP_MEASURED_OPERANDS)


def test_equal_admissible_states_give_the_physical_flux(oracle):
    """L == R: the dissipative term is exactly zero (asserted through eps, which then changes no bit) and S_R / (S_R - S_L) - S_L / (S_R - S_L) = 1 —
    the 50-digit HLL flux of equal states IS the physical flux ((c_hat / c) F_n, c_hat c T_nj E), and the oracle's is within the rounding cap of it"""
    rng = np.random.default_rng(5)
    n = 4000
    t = R.cell_traits()
    U = R.random_cells(rng, n, R.C_CGS, fmax=0.999)
    p = oracle.rad_cons_to_prim(t, U)
    for d in range(3):
        F, mask = oracle.rad_face_fluxes(t, d, p, p, U, U)
        assert not np.any(mask & B["fallback"])
        for i in range(0, n, 40):
            want, _, operands = R.mp_face_flux(d, p[:, i], p[:, i], R.C_CGS, R.CHAT_CGS, 1.0, 0)
            for c in range(4):
                assert R.ulps_off(F[c, i], want[c], operands[c]) <= R.ORACLE_ULP_CAP_OPERANDS
        assert np.array_equal(F[0] != 0, U[1 + d] != 0)
        Fe, _ = oracle.rad_face_fluxes(t, d, p, p, U, U, np.full(n, 0.25))
        assert np.all(R.same_bits(F, Fe))


def test_mirroring_the_normal_component_negates_three_components_bit_for_bit(oracle):
    """x_n -> -x_n: the left state becomes the right one with f_n negated; the energy flux and the two transverse momentum fluxes change sign, the
    normal one does not — in every bit: S_R - S_L is the same difference, and the sum (a - b) + c becomes (b - a) + (-c)"""
    n = 20000
    for d in range(3):
        _, pL, pR, cL, cR, eps = R.random_faces(oracle, 40 + d, n)
        t = R.cell_traits()
        F, mask = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR, eps)

        def mirror(a):
            m = a.copy()
            m[1 + d] = -m[1 + d]
            return m
        Fm, maskm = oracle.rad_face_fluxes(t, d, mirror(pR), mirror(pL), mirror(cR), mirror(cL), eps)
        sign = -np.ones(4)
        sign[1 + d] = 1.0
        # (every non-zero value by its bits; a component that is exactly zero — an axis-aligned flux — is +0 on both sides: (+0 - +0) + +0)
        assert np.array_equal(Fm, sign[:, None] * F) and np.isfinite(F).all(), d
        assert ((mask & B["fallback"]) != 0).sum() == ((maskm & B["fallback"]) != 0).sum() > 1000


def test_eps_changes_the_energy_flux_only(oracle):
    n = 20000
    d, pL, pR, cL, cR, eps = R.random_faces(oracle, 50, n)
    t = R.cell_traits()
    F1, _ = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR, None)
    Fe, _ = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR, eps)
    assert np.all(R.same_bits(F1[1:], Fe[1:]))
    changed = ~R.same_bits(F1[0], Fe[0])
    assert changed[eps < 1.0].mean() > 0.9 and not changed[eps == 1.0].any()


def test_the_fallback_flux_is_the_donor_cell_flux_of_the_two_cells(oracle):
    """a face that takes the fallback forgets its reconstructed states: the same bits as the donor-cell face of the same two cells, whose states are
    the cells' own primitives (and which takes the fallback as well)"""
    n = 20000
    d, pL, pR, cL, cR, eps = R.random_faces(oracle, 60, n)
    t = R.cell_traits()
    F, mask = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR, eps)
    fb = (mask & B["fallback"]) != 0
    assert 2000 < fb.sum() < n - 2000
    qL, qR = oracle.rad_cons_to_prim(t, cL), oracle.rad_cons_to_prim(t, cR)
    Fd, maskd = oracle.rad_face_fluxes(t, d, qL, qR, cL, cR, eps)
    both = fb & ((maskd & B["fallback"]) != 0)
    assert both.sum() > 1000 and np.all(R.same_bits(F[:, both], Fd[:, both]))
    # (reduced fluxes moved towards each other stay inside the unit ball when both cells are: a face state beyond it means a cell beyond it)
    assert not np.any(fb & ~both)
    moved = ~R.same_bits(pL, qL).all(axis=0)
    assert (both & moved).sum() >= 100  # (moving the face states towards each other takes most of them back inside)


def test_named_faces_take_the_branch_they_are_named_for(oracle):
    names, d, pL, pR, cL, cR, want = R.targeted_faces()
    for eddington in (0, 1):
        t = R.cell_traits(R.C_EXACT, R.CHAT_EXACT, eddington=eddington)
        F, mask = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR)
        for i, name in enumerate(names):
            must, mustnot = want[name]
            if eddington == 1:  # chi = 1/3: T_nn = 1/3, the floor on S never acts; f = NaN leaves the finite tensor of f = 0
                must &= ~(B["S_floor_L"] | B["S_floor_R"])
                if name.startswith("E_0") and "3_components" not in name:
                    must &= ~B["nonfinite"]
            assert (mask[i] & must) == must and (mask[i] & mustnot) == 0, (name, eddington, bin(mask[i]), bin(must), bin(mustnot))
    # the three exact unit vectors ARE exact: the first test of the fallback sees f == 1
    for f in ((0.6, 0.8, 0.0), (0.36, 0.48, 0.8), (1.0, 0.0, 0.0)):
        assert np.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]) == 1.0


def test_ladders_stay_finite_in_the_oracle(oracle):
    t = R.cell_traits(R.C_EXACT, R.CHAT_EXACT)
    E, d, pL, pR, cL, cR = R.ladder_E()
    F, mask = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR)
    ok = (E >= 1e-290) & (E <= 1e290)
    assert np.isfinite(F[:, ok]).all() and not np.any(mask[ok] & B["fallback"])
    f, d, pL, pR, cL, cR = R.ladder_f()
    F, mask = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR)
    assert np.isfinite(F).all() and not np.any(mask & B["fallback"])
    assert np.any(mask & B["no_dir_L"]) and not np.all(mask & B["no_dir_L"])  # f^2 underflows at the bottom of the ladder: n = 0 there


@pytest.mark.parametrize("floor", [R.FLOOR, 0.0])
def test_random_faces_reach_every_branch_and_no_non_number(oracle, floor):
    """(a face knows no floor: the two values only show that the traits do not matter here)"""
    n = 20000
    d, pL, pR, cL, cR, eps = R.random_faces(oracle, 70, n)
    F, mask = oracle.rad_face_fluxes(R.cell_traits(floor=floor), d, pL, pR, cL, cR, eps)
    count = R.count_bits(mask, B)
    assert count["nonfinite"] == 0 and np.isfinite(F).all()
    for k in ("fallback", "f_L_ge_1", "f_R_ge_1", "clamp_L", "clamp_R", "S_floor_L", "S_floor_R"):
        assert count[k] >= 50, count
    assert set(np.unique(d)) == {0, 1, 2}


@pytest.mark.parametrize("name", [c.name for c in R.STAGE_CASES + R.VERDICT_CASES])
def test_random_levels_reach_every_branch_at_least_50_times_and_no_non_number(name):
    """from the oracle's masks.  3-D levels and the 40 x 40 plane: every face bit but `nonfinite` and every cell bit but `f_nan` at least 50 times
    (S_floor needs Levermore's closure, by_other several groups; the plane's exceptions are named below); the 64-cell line is too small for 50 and
    must show the fallback and a repair.  A floor above 0: no non-number anywhere in the fluxes or the new state."""
    case = R.STAGE_CASE[name]
    ref = R.stage_reference(name)
    fm = np.concatenate([m.ravel() for r in ref for m in r[2]])
    cm = np.concatenate([r[3].ravel() for r in ref])
    fc, cc = R.count_bits(fm, RAD_FACE_BIT), R.count_bits(cm, RAD_CELL_BIT)
    assert fc["nonfinite"] == 0 and cc["f_nan"] == 0
    for r in ref:
        assert np.isfinite(r[0]).all() and all(np.isfinite(f).all() for f in r[1])
    faces = [k for k in R.FACE_BITS_RANDOM if not (case.eddington == 1 and k.startswith("S_floor"))]
    cells = R.CELL_BITS_RANDOM + (("by_other",) if case.ngroups > 1 else ())

    def need(k):
        if case.ndim == 3:
            return 50
        if case.ndim == 1:  # 65 faces, 64 cells: the fallback with each trigger and a repair must show, the rarer bits cannot be asked for
            return 1 if k in ("fallback", "erad_L_le_0", "erad_R_le_0", "f_L_ge_1", "f_R_ge_1", "clamp_L", "clamp_R") + cells else 0
        # the 40 x 40 plane: 50 as well, but for what 1600 cells cannot hold — 16 cells without flux per group (no_dir with one group), 16 invalid
        # cells at the 1 % share (the cell bits there)
        if (k.startswith("no_dir") and case.ngroups == 1) or (k in cells and case.bad_share < 0.05):
            return 1
        return 50
    for k in faces:
        assert fc[k] >= need(k), (k, fc)
    for k in cells:
        assert cc[k] >= need(k), (k, cc)


def test_verdict_cases_hold_a_valid_group_below_its_floor_in_cells_another_group_spoils():
    """what the whole-cell verdict tests claim, from the oracle's record: in every case the quiet group is lifted (by_other) in at least 100 cells and
    in no cell by its own fault; the spoiling group is invalid by E <= 0 in some of them and by f > 1 in others"""
    C = RAD_CELL_BIT
    for case in R.VERDICT_CASES:
        (U_new, _, _, cm), = R.stage_reference(case.name)
        q, a = cm[case.quiet_group], cm[case.bad_group]
        lifted = (q & C["by_other"]) != 0
        assert lifted.sum() >= 100 and not np.any(q & (C["invalid_E"] | C["invalid_f"])), case.name
        assert np.all((q[lifted] & C["lifted"]) != 0)
        assert ((a[lifted] & C["invalid_E"]) != 0).sum() >= 20 and ((a[lifted] & C["invalid_f"]) != 0).sum() >= 20, case.name
        fl = case.floor / 4
        Eq = U_new[6 + 4 * case.quiet_group][4:-4, 4:-4, 4:-4]
        assert np.all(Eq[lifted] == fl) and np.all(Eq[~lifted & (Eq != fl)] == 0.5 * fl)


def test_floor_0_cases_feed_empty_cells_to_the_second_stage():
    """Erad_floor = 0: stage 1 has no non-number and leaves cells with E = 0, F = +-0; stage 2 reads them: NaN momentum fluxes at their faces, NaN in
    the new state of the cells and their neighbours — the only place of the random sets where non-numbers appear"""
    for c in R.FLOOR0_CASES:
        (U1, flux, fm, cm), = R.stage_reference(c.name)
        assert np.isfinite(U1).all() and all(np.isfinite(f).all() for f in flux)
        v = U1[6:10, 4:-4, 4:-4, 4:-4]
        empty = (v[0] == 0.0)
        assert empty.sum() >= 100 and np.all(v[1:, empty] == 0.0) and not np.any(v[0] < 0)
        (U2, flux2, fm2, cm2), = R.stage_reference(c.name.replace("-s1", "-s2"))
        nf = sum(int(((m & B["nonfinite"]) != 0).sum()) for m in fm2)
        assert nf >= 3 * empty.sum() and ((cm2 & RAD_CELL_BIT["f_nan"]) != 0).sum() >= empty.sum()
        assert np.isnan(U2[6:10, 4:-4, 4:-4, 4:-4]).any(axis=0).sum() > empty.sum()


def test_an_invalid_cell_lies_within_two_cells_of_every_seam():
    """the 40^3 cases: every X seam of the flux kernel and of the sweep (row, i), every strip start of the Y and Z sweeps and of the flux marches has
    an invalid INPUT cell within two cells along the sweep direction — and the oracle took the fallback at a face there"""
    for case in R.STAGE_CASES:
        if not (case.n == 40 and case.ndim == 3):
            continue
        (U, _, _), = R.stage_inputs(case)
        (_, _, fm, _), = R.stage_reference(case.name)
        E = np.stack([U[6 + 4 * g] for g in range(case.ngroups)])[:, 4:-4, 4:-4, 4:-4]
        F2 = np.stack([(U[7 + 4 * g: 10 + 4 * g] ** 2).sum(axis=0) for g in range(case.ngroups)])[:, 4:-4, 4:-4, 4:-4]
        bad = ((E <= 0) | (F2 > (R.C_CGS * E) ** 2)).any(axis=0)  # [k, j, i]
        fb = [((m & B["fallback"]) != 0).any(axis=0) for m in fm]
        for row, i in R.SEAMS_40["x_flux"] + R.SEAMS_40["x_sweep"]:
            lo, hi = max(i - 2, 0), min(i + 2, 39)
            assert bad[:, row, lo:hi + 1].any(), (case.name, row, i)
            assert fb[0][:, row, max(i - 2, 0):min(i + 2, 40) + 1].any(), (case.name, row, i)
        for j in R.SEAMS_40["y_strips"] + R.SEAMS_40["march_faces"]:
            assert bad[:, max(j - 2, 0):min(j + 2, 40), :].any() and fb[1][:, j, :].any(), (case.name, "y", j)
        for k in R.SEAMS_40["z_strips"] + R.SEAMS_40["march_faces"]:
            assert bad[max(k - 2, 0):min(k + 2, 40), :, :].any() and fb[2][k, :, :].any(), (case.name, "z", k)


def test_an_invalid_cell_lies_at_the_strip_seam_of_every_20_cubed_box():
    """the eight 20^3 boxes: Y strips of 16 + 4 cells; in every box an invalid INPUT cell within two cells of j = 16 (box-relative) and a y face there
    at which the oracle took the fallback; likewise at the march strips' first faces 8 and 16 and the last strip's 20 along y and z"""
    for case in R.STAGE_CASES:
        if case.nboxes != 8:
            continue
        for (U, _, _), (_, _, fm, _) in zip(R.stage_inputs(case), R.stage_reference(case.name)):
            E = np.stack([U[6 + 4 * g] for g in range(case.ngroups)])[:, 4:-4, 4:-4, 4:-4]
            F2 = np.stack([(U[7 + 4 * g: 10 + 4 * g] ** 2).sum(axis=0) for g in range(case.ngroups)])[:, 4:-4, 4:-4, 4:-4]
            bad = ((E <= 0) | (F2 > (R.C_CGS * E) ** 2)).any(axis=0)
            fb = [((m & B["fallback"]) != 0).any(axis=0) for m in fm]
            for s in (8, 16, 20):
                assert bad[:, max(s - 2, 0):min(s + 2, 20), :].any() and fb[1][:, s, :].any(), (case.name, "y", s)
                assert bad[max(s - 2, 0):min(s + 2, 20), :, :].any() and fb[2][s, :, :].any(), (case.name, "z", s)
