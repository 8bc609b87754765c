"""The radiation TRANSPORT kernels against the oracle, face by face and cell by cell, at their branches and at the seams of their decompositions:
qk_rad_ConservedToPrimitive, qk_rad_ComputeFluxes, qk_rad_computeRadiationFluxes + qk_rad_PredictStep / qk_rad_AddFluxesRK2 and qk_rad_stage_fused,
called straight through the C-ABI on arrays this file fills (ghost cells included: nothing fills a boundary here).

Every comparison is bit for bit — no libm is on this path —: any NaN equals any NaN in the same position, everything else compares by bit pattern.
The inputs, the oracle's results and the branch masks come from tests/rad_transport_reference.py; tests/test_rad_transport_reference.py asserts on
the CPU, from the ORACLE's masks, that the cases reach the branches and seams claimed here."""
import ctypes as C

import numpy as np
import pytest

import rad_transport_reference as R
from oracle.pyoracle import RAD_CELL_BIT, RAD_FACE_BIT

pytestmark = pytest.mark.gpu

POISON = -1.2345e300  # what the arrays a stage writes hold beforehand: it must survive wherever the stage has no business


def rad_traits(c=R.C_CGS, chat=R.CHAT_CGS, floor=0.0, eddington=0, ngroups=1):
    from quokka_amd import capi
    rt = capi.RadTraits(c, chat, 7.5657e-15, floor, 1, 0, 1.0, 1.0, 1.0, 1, eddington)
    rt.ngroups = ngroups
    return rt


def assert_same(got, want, what):
    """bit for bit (NaN == NaN); the message names how many entries differ and the first of them"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~R.same_bits(got, want)
    if bad.any():
        where = np.argwhere(bad)
        first = [(tuple(int(v) for v in w), float(got[tuple(w)]), float(want[tuple(w)])) for w in where[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ; index, GPU, oracle: {first}")


# ------------------------------------------------------------------ faces
def gpu_faces(ctx, rt, d, pL, pR, cL, cR, eps=None):
    """qk_rad_ComputeFluxes in direction d and qk_rad_ConservedToPrimitive on n independent faces laid out on one box that is two cells thick along d:
    returns (F[4, n], prim of the left cells [4, n], prim of the right cells)"""
    from quokka_amd.multifab import Level, MultiFab
    n = pL.shape[1]
    hi = [n - 1, 0, 0]
    if d == 0:
        hi = [1, n - 1, 0]
    else:
        hi[d] = 1
    lev = Level(ctx, 3, [([0, 0, 0], hi)])
    cons = MultiFab(lev, 10, 1, fill=0.0)  # one ghost cell: the kernel also evaluates the two outer faces of the box, which read a cell beyond it
    left, right, flux = (MultiFab(lev, 4, 0, facedir=d, fill=0.0) for _ in range(3))
    epsm = MultiFab(lev, 1, 0, facedir=d, fill=1.0)
    prim = MultiFab(lev, 4, 0, fill=0.0)

    def cell(side):  # index of the cells / the face in a (nz, ny, nx) array: the run of n along x (along y for d == 0)
        return {0: (0, slice(None), side), 1: (0, side, slice(None)), 2: (side, 0, slice(None))}[d]
    U = np.zeros(cons.shapes[0])
    Uv = U[:, 1:-1, 1:-1, 1:-1]
    Uv[0], Uv[4], Uv[5] = 1.0, 1.0, 1.0
    Uv[(slice(6, 10),) + cell(0)] = cL
    Uv[(slice(6, 10),) + cell(1)] = cR
    cons.set_fab(0, U)
    for mf, a in ((left, pL), (right, pR), (epsm, None if eps is None else eps[None, :])):
        if a is not None:
            A = np.zeros(mf.shapes[0]) + (1.0 if mf is epsm else 0.0)
            A[(slice(None),) + cell(1)] = a
            mf.set_fab(0, A)
    c = ctx
    c.check(c.L.qk_rad_ComputeFluxes(lev.h, c.stream(), C.byref(rt), d, flux.ptr, left.ptr, right.ptr, cons.ptr, epsm.ptr if eps is not None else None),
            "qk_rad_ComputeFluxes")
    c.check(c.L.qk_rad_ConservedToPrimitive(lev.h, c.stream(), C.byref(rt), cons.ptr, prim.ptr, 0), "qk_rad_ConservedToPrimitive")
    F = flux.fab_numpy(0)[(slice(None),) + cell(1)]
    P = prim.fab_numpy(0)
    return F, P[(slice(None),) + cell(0)], P[(slice(None),) + cell(1)]


def faces_by_direction(ctx, rt, direction, pL, pR, cL, cR, eps=None):
    F, qL, qR = (np.empty_like(pL) for _ in range(3))
    for d in range(3):
        m = direction == d
        if m.any():
            F[:, m], qL[:, m], qR[:, m] = gpu_faces(ctx, rt, d, pL[:, m], pR[:, m], cL[:, m], cR[:, m], None if eps is None else eps[m])
    return F, qL, qR


@pytest.mark.parametrize("eddington", [0, 1])
def test_named_faces_match_the_oracle(ctx, oracle, eddington):
    """every named face (tests/rad_transport_reference.py: each fallback trigger alone, f exactly 1 and one ulp below, f = 1 across the face, f = 0, the
    fallback onto a cell with f > 1, E = 0 with and without flux, E < 0 on both sides), c_hat != c: the flux and the primitives of both cells.  E = 0:
    the reference's momentum fluxes are NaN and its reduced fluxes +-inf or NaN, and so are the kernel's."""
    names, d, pL, pR, cL, cR, want = R.targeted_faces()
    t = R.cell_traits(R.C_EXACT, R.CHAT_EXACT, eddington=eddington)
    Fo, mask = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR)
    F, qL, qR = faces_by_direction(ctx, rad_traits(R.C_EXACT, R.CHAT_EXACT, eddington=eddington), d, pL, pR, cL, cR)
    for i, name in enumerate(names):
        assert_same(F[:, i], Fo[:, i], f"flux of {name} (mask {mask[i]:#x})")
    assert_same(qL, oracle.rad_cons_to_prim(t, cL), "primitives, left cells")
    assert_same(qR, oracle.rad_cons_to_prim(t, cR), "primitives, right cells")
    assert ((mask & RAD_FACE_BIT["nonfinite"]) != 0).sum() >= (3 if eddington else 11) and np.isinf(qR).any() and np.isnan(qR).any()


@pytest.mark.parametrize("with_eps", [False, True])
@pytest.mark.parametrize("eddington", [0, 1])
def test_random_faces_match_the_oracle(ctx, oracle, eddington, with_eps):
    """2e4 seeded faces in the three directions, E over 30 decades, |f| up to 1.2, c_hat = 0.1 c, with and without the wavespeed-correction factor:
    the flux of every face and the primitives of every cell; a third of the faces take the fallback (asserted from the oracle's mask)"""
    d, pL, pR, cL, cR, eps = R.random_faces(oracle, 80 + eddington, 20000)
    eps = eps if with_eps else None
    t = R.cell_traits(eddington=eddington)
    Fo, mask = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR, eps)
    count = R.count_bits(mask, RAD_FACE_BIT)
    assert count["nonfinite"] == 0 and all(count[k] >= 50 for k in ("fallback", "f_L_ge_1", "f_R_ge_1", "clamp_L", "clamp_R"))
    F, qL, qR = faces_by_direction(ctx, rad_traits(eddington=eddington), d, pL, pR, cL, cR, eps)
    assert_same(F, Fo, "flux")
    assert_same(qL, oracle.rad_cons_to_prim(t, cL), "primitives, left cells")
    assert_same(qR, oracle.rad_cons_to_prim(t, cR), "primitives, right cells")


def test_ladders_in_E_and_f_report_where_bit_parity_ends(ctx, oracle):
    """the E ladder (1e-300 ... 1e300) and the |f| ladder (1e-200 ... 1) of tests/rad_transport_reference.py with c = 1024: prints the first E on either
    side and the first |f| at which a bit of the flux or of the primitives differs, and asserts equality inside the range include/quokka_amd.h states
    for the transport entries: c E of both cells in R.PARITY_CE, and every |f| of the ladder from R.PARITY_F up — flux and primitives of both cells"""
    t = R.cell_traits(R.C_EXACT, R.CHAT_EXACT)
    rt = rad_traits(R.C_EXACT, R.CHAT_EXACT)
    E, d, pL, pR, cL, cR = R.ladder_E()
    Fo, _ = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR)
    F, qL, qR = faces_by_direction(ctx, rt, d, pL, pR, cL, cR)
    same = R.same_bits(F, Fo).all(axis=0) & R.same_bits(qL, oracle.rad_cons_to_prim(t, cL)).all(axis=0) & R.same_bits(qR, oracle.rad_cons_to_prim(t, cR)).all(axis=0)
    low, high = E[~same & (E < 1.0)], E[~same & (E > 1.0)]
    print("E ladder: bits differ from", low.max() if low.size else None, "down and from", high.min() if high.size else None, "up; c E = 1024 E")
    cE = R.C_EXACT * E
    inside = (cE >= R.PARITY_CE[0]) & (2.0 * cE <= R.PARITY_CE[1])
    assert inside.sum() > 1000 and same[inside].all(), (E[inside & ~same][:4], E[inside & ~same][-4:])
    f, d, pL, pR, cL, cR = R.ladder_f()
    Fo, _ = oracle.rad_face_fluxes(t, d, pL, pR, cL, cR)
    F, qL, qR = faces_by_direction(ctx, rt, d, pL, pR, cL, cR)
    same = R.same_bits(F, Fo).all(axis=0) & R.same_bits(qL, oracle.rad_cons_to_prim(t, cL)).all(axis=0) & R.same_bits(qR, oracle.rad_cons_to_prim(t, cR)).all(axis=0)
    print("|f| ladder: bits differ at", f[~same])
    sub = (f * f > 0.0) & (f * f < 2.0 ** -1022)
    assert f.min() <= R.PARITY_F and sub.sum() >= 10  # (the whole ladder, the rungs whose f^2 is subnormal included)
    assert same.all(), f[~same]


# ------------------------------------------------------------------ stages
def gpu_stage(ctx, case, route, inputs, in_place=False, second_table=False):
    """one transport stage of the case's level by `route` ("separate": computeRadiationFluxes + PredictStep / AddFluxesRK2; "fused": qk_rad_stage_fused).
    Returns per box (U_new fab, [flux_d]) and checks that the ghost cells of the accumulator kept their poison."""
    from quokka_amd.multifab import Level, MultiFab
    from quokka_amd.radhydro import _d3, _p3
    ng, nd = case.ngroups, case.ndim
    ncomp, nrad = 6 + 4 * ng, 4 * ng
    lev = Level(ctx, nd, case.boxes())
    Uin, U0 = MultiFab(lev, ncomp, 4, fill=0.0), None
    for b, (U, U0a, _) in enumerate(inputs):
        Uin.set_fab(b, U)
    if case.stage == 2:
        U0 = MultiFab(lev, ncomp, 4, fill=0.0)
        for b, (_, U0a, _) in enumerate(inputs):
            U0.set_fab(b, U0a)
    else:
        U0 = Uin
    Unew = Uin if (in_place or second_table) else MultiFab(lev, ncomp, 4, fill=POISON)
    new_ptr = Uin.subset_ptr(list(range(lev.nboxes))) if second_table else Unew.ptr
    assert not second_table or new_ptr.value != Uin.ptr.value
    flux = [MultiFab(lev, nrad, 0, facedir=d, fill=POISON) for d in range(nd)]
    eps = None
    if case.eps:
        eps = [MultiFab(lev, ng, 0, facedir=d, fill=1.0) for d in range(nd)]
        for b, (_, _, e) in enumerate(inputs):
            for d in range(nd):
                eps[d].set_fab(b, e[d])
    c, rt = ctx, rad_traits(floor=case.floor, eddington=case.eddington, ngroups=ng)
    if route == "fused":
        acc = MultiFab(lev, nrad, 2, fill=POISON)  # (two ghost cells the stage has no use for)
        c.check(c.L.qk_rad_stage_fused(lev.h, c.stream(), C.byref(rt), case.order, case.stage, Uin.ptr, U0.ptr, new_ptr, acc.ptr, _p3(flux), float(R.DT), _d3(R.DX),
                                       _p3(eps) if eps else None), "qk_rad_stage_fused")
        for b in range(lev.nboxes):
            A = acc.fab_numpy(b)
            A[:, 2:-2, 2:-2, 2:-2] = POISON
            assert np.all(A == POISON), "qk_rad_stage_fused wrote a ghost cell of the accumulator"
    else:
        c.check(c.L.qk_rad_computeRadiationFluxes(lev.h, c.stream(), C.byref(rt), nd, case.order, Uin.ptr, _p3(flux), _p3(eps) if eps else None),
                "qk_rad_computeRadiationFluxes")
        if case.stage == 1:
            c.check(c.L.qk_rad_PredictStep(lev.h, c.stream(), C.byref(rt), nd, U0.ptr, new_ptr, _p3(flux), float(R.DT), _d3(R.DX)), "qk_rad_PredictStep")
        else:  # (the old-state fluxes have weight 0.5 - IMEX_a32 = 0 and are not read: any arrays)
            c.check(c.L.qk_rad_AddFluxesRK2(lev.h, c.stream(), C.byref(rt), nd, new_ptr, U0.ptr, Uin.ptr, _p3(flux), _p3(flux), float(R.DT), _d3(R.DX)),
                    "qk_rad_AddFluxesRK2")
    return [(Unew.fab_numpy(b), [f.fab_numpy(b) for f in flux]) for b in range(lev.nboxes)]


def check_stage(case, got, ref, in_place=False):
    """fluxes of every direction and the whole U_new fab of every box: the valid cells' radiation components are the oracle's, every other entry is
    what it was (the poison; in place: the input)"""
    nd = case.ndim
    for b, ((Ug, Fg), (Uo, Fo, fmask, cmask)) in enumerate(zip(got, ref)):
        for d in range(nd):
            assert_same(Fg[d], Fo[d], f"{case.name}: box {b}, flux along {d}")
        want = np.array(Uo)
        if not in_place:
            v = tuple([slice(6, None)] + [slice(4, -4) if a < nd else slice(None) for a in (2, 1, 0)])
            want = np.full_like(Uo, POISON)
            want[v] = Uo[v]
        assert_same(Ug, want, f"{case.name}: box {b}, new state")


def routes(case):
    return ("separate", "fused") if case.ndim == 3 else ("separate",)


@pytest.mark.parametrize("route", ["separate", "fused"])
@pytest.mark.parametrize("name", [c.name for c in R.STAGE_CASES])
def test_stage_matches_the_oracle(ctx, name, route):
    """Both device routes against orc_rad_transport_stage on identical ghost-filled arrays: the fluxes in every direction and every component of the new
    state; ghost cells and gas components of U_new and the ghost cells of the accumulator keep their poison.  One 40^3 box (every seam: Y strips of
    16 + 16 + 8, Z strips of 32 + 8, flux marches of 5 x 8 faces + the lone last one, eight X workgroups with seams in mid-row), eight 20^3 boxes, a
    64-cell line and a 40 x 40 plane (separate operators only: the fused stage is 3-D); orders 1-3, stages 1 and 2, 1 and 4 groups, 1 % and 30 % of the
    cells invalid, with and without wavespeed-correction arrays, both closures."""
    case = R.STAGE_CASE[name]
    if route not in routes(case):
        from quokka_amd import capi
        with pytest.raises(capi.QkError):  # 1-D / 2-D levels: QK_ERR_UNSUPPORTED, as include/quokka_amd.h says
            gpu_stage(ctx, case, route, R.stage_inputs(case))
        return
    check_stage(case, gpu_stage(ctx, case, route, R.stage_inputs(case)), R.stage_reference(name))


@pytest.mark.parametrize("route", ["separate", "fused"])
@pytest.mark.parametrize("name", ["box40-o3-s2-g4-30pct-eps", "box40-o2-s2-g1-30pct", "box40-o1-s2-g4-30pct-eps", "boxes20-o3-s2-g1-30pct"])
def test_stage_2_in_place_matches_the_oracle(ctx, name, route):
    """stage 2 with U_new = U_in, as the drivers run it, on the 30 % states: the whole array afterwards — ghost cells and gas components untouched"""
    case = R.STAGE_CASE[name]
    check_stage(case, gpu_stage(ctx, case, route, R.stage_inputs(case), in_place=True), R.stage_reference(name), in_place=True)


@pytest.mark.parametrize("name", ["box40-o3-s1-g4-30pct", "box40-o2-s1-g1-30pct-eps", "box40-o1-s1-g4-30pct"])
def test_stage_1_through_a_second_descriptor_table_matches_the_oracle(ctx, name):
    """stage 1 of the fused route with U_new = a second descriptor table over the storage of U_in (= U0): the Z sweep sees the equal fab pointers and
    marches whole pencils; the result is the oracle's, written in place"""
    case = R.STAGE_CASE[name]
    check_stage(case, gpu_stage(ctx, case, "fused", R.stage_inputs(case), second_table=True), R.stage_reference(name), in_place=True)


@pytest.mark.parametrize("route", ["separate", "fused"])
@pytest.mark.parametrize("name", [c.name for c in R.VERDICT_CASES])
def test_whole_cell_verdict(ctx, name, route):
    """isStateValid is a property of the cell, amendRadState repairs every group (reference src/radiation/radiation_system.hpp:626-665): four groups, one
    invalid in 5 % of the cells, another valid and below its floor everywhere — where the first spoils the cell the second is lifted to the floor (the
    oracle's by_other bit, >= 100 cells per case: tests/test_rad_transport_reference.py), on both routes, at every pair of group positions."""
    case = R.STAGE_CASE[name]
    ref = R.stage_reference(name)
    assert ((ref[0][3][case.quiet_group] & RAD_CELL_BIT["by_other"]) != 0).sum() >= 100
    check_stage(case, gpu_stage(ctx, case, route, R.stage_inputs(case)), ref)


@pytest.mark.parametrize("route", ["separate", "fused"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_two_stages_with_a_zero_floor_keep_the_reference_non_numbers(ctx, order, route):
    """Erad_floor = 0 (the shell problem's setting): stage 1 repairs negative energies to E = 0, F = +-0; stage 2 reads those cells: F / (c 0) is NaN,
    the momentum fluxes at their faces and the new state of the cells around them are NaN in the reference, and here — every component, every
    non-number, the neighbours included"""
    first, second = R.STAGE_CASE[f"floor0-o{order}-s1"], R.STAGE_CASE[f"floor0-o{order}-s2"]
    got1 = gpu_stage(ctx, first, route, R.stage_inputs(first))
    check_stage(first, got1, R.stage_reference(first.name))
    ref2 = R.stage_reference(second.name)
    assert sum(int(((m & RAD_FACE_BIT["nonfinite"]) != 0).sum()) for m in ref2[0][2]) >= 300 and ((ref2[0][3] & RAD_CELL_BIT["f_nan"]) != 0).sum() >= 100
    # the second stage starts from the GPU's own first stage (ghost cells: the input's, as in the oracle's chain)
    (U, U0, _), = R.stage_inputs(second)
    mine = np.array(U0)
    v = (slice(6, None), slice(4, -4), slice(4, -4), slice(4, -4))
    mine[v] = got1[0][0][v]
    assert_same(mine, U, "the state between the stages")
    check_stage(second, gpu_stage(ctx, second, route, [(mine, U0, None)]), ref2)


@pytest.mark.parametrize("route", ["separate", "fused"])
@pytest.mark.parametrize("name", [c.name for c in R.NEGZERO_CASES])
def test_zeros_of_both_signs_change_at_most_the_sign_of_a_zero(ctx, name, route):
    """The one difference this file found and left: the inputs of the other tests hold +0 where a cell has no flux; with -0 among them (f d c E of a
    direction with negative components) PPM's std::minmax meets zeros of opposite sign, returns one by position where v_min_f64 / v_max_f64 return one
    by sign (csrc/qk_device.hpp, smin / smax), and an exactly-zero flux comes out with the other sign: 6 of the 459200 flux and state entries of
    the PPM case on an MI355X, none with PLM (printed).  Asserted: every entry has the oracle's VALUE (-0 == +0), and an entry whose bits differ is a zero."""
    case = R.STAGE_CASE[name]
    got, ref = gpu_stage(ctx, case, route, R.stage_inputs(case)), R.stage_reference(name)
    n = 0
    for (Ug, Fg), (Uo, Fo, _, _) in zip(got, ref):
        v = (slice(6, None), slice(4, -4), slice(4, -4), slice(4, -4))
        for a, b in [(Ug[v], Uo[v])] + list(zip(Fg, Fo)):
            assert np.isfinite(b).all() and np.array_equal(a, b)
            n += int((~R.same_bits(a, b)).sum())
    print(f"{name} {route}: {n} zeros of the other sign")
    assert n == {2: 0, 3: 6}[case.order]  # (measured, both routes alike; seeded inputs: another count means the kernels or the inputs changed)
