"""CPU checks of the numpy restatement of the tracer kernels (tests/tracer_reference.py) that the GPU tests compare against bit for bit, and
of the host side of the plan (the cell -> box lattice; no kernel runs)."""
import ctypes as C

import numpy as np
import pytest

import tracer_reference as tr

EPS = np.finfo(np.float64).eps


def geom3(periodic=(0, 0, 0), n=(8, 6, 5)):
    return tr.TracerGeom(3, list(n), [-0.3, 0.1, 0.25], [0.9, 1.0, 1.0], list(periodic))


def test_linear_field_is_interpolated_exactly_to_rounding():
    """A field linear in x, y, z, away from the clamped edge (stencil inside the domain), is reproduced by the trilinear weights in exact
    arithmetic.  Rounding, in units of eps * max|u| (weights <= 1, sum of weights 1, |b_e| L_e <= 2 max|u| for a linear field):
      l_e = (x - plo) * dxi, - 0.5: three roundings of relative size eps / 2 on a number below N; it moves the evaluation point by
            1.5 eps |l_e| cells, the value by 1.5 eps |b_e| L_e <= 3 per direction                                       ->  9
      s_e = {1 - w, w}: absolute error eps / 2 each, carried into each of the 8 weight products by factors <= 1: 3 * 0.5 * 8  -> 12
      (s_0 * s_1) * s_2 and the product with u: three roundings, relative, summed over weights that add up to 1: 1.5       ->  1.5
      the eight additions, each eps / 2 of a partial sum <= max|u|                                                       ->  4
      the face values themselves (a + b . x evaluated in floating point, about four roundings), averaged with weights     ->  2
      the expected value, evaluated the same way                                                                          ->  2"""
    bound_units = 9 + 12 + 1.5 + 4 + 2 + 2
    g = geom3()
    a, b = 0.7, np.array([1.3, -0.8, 0.45])
    rng = np.random.default_rng(1)

    def field(d):
        coords = []
        for e in range(3):
            i = np.arange(g.n_cell[e] + (1 if e == d else 0), dtype=np.float64)
            coords.append(g.prob_lo[e] + (i + (0.0 if e == d else 0.5)) * g.dx[e])
        z, y, x = np.meshgrid(coords[2], coords[1], coords[0], indexing="ij")
        return a + b[0] * x + b[1] * y + b[2] * z

    umac = [field(d) for d in range(3)]
    umax = max(np.abs(u).max() for u in umac)
    lo = np.array([g.prob_lo[e] + 0.5 * g.dx[e] for e in range(3)])
    hi = np.array([g.prob_hi[e] - 0.5 * g.dx[e] for e in range(3)])
    x = lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(2000, 3))
    x = np.minimum(np.maximum(x, lo), np.nextafter(hi, lo))  # i_e + 1 <= N - 1 for the transverse stencils
    v = tr.interp_all(g, umac, x)
    expect = a + b[0] * x[:, 0] + b[1] * x[:, 1] + b[2] * x[:, 2]
    err = np.abs(v - expect[:, None]).max()
    print(f"linear field: max error {err / (EPS * umax):.2f} eps max|u| (bound {bound_units})")
    assert err <= bound_units * EPS * umax
    # at the clamped edge the field is extended as a constant (foextrap): a particle half a cell outside reads the boundary values
    xe = np.array([[g.prob_lo[0] - 0.4 * g.dx[0], 0.5, 0.6]])
    at_face = tr.interp_mac(g, umac[0], 0, np.array([[g.prob_lo[0], 0.5, 0.6]]))[0]
    assert abs(tr.interp_mac(g, umac[0], 0, xe)[0] - at_face) <= 17.5 * EPS * umax  # (weights that add up to 1: the bound of the uniform-field test)


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_uniform_field_moves_every_particle_by_dt_v(ndim):
    """weights that add up to 1 within 17.5 eps (the s_e, product and addition terms of the bound above): |v1 - v| <= 17.5 eps |v|, and the
    position takes dt * v1 with one rounding of the product and one of the sum"""
    g = tr.TracerGeom(ndim, [8, 6, 5][:ndim], [-0.3, 0.1, 0.25][:ndim], [0.9, 1.0, 1.0][:ndim], [1, 0, 1][:ndim])
    vel = [0.3, -0.2, 0.1][:ndim]
    umac = [np.full(tr.face_shape(g, d), vel[d]) for d in range(ndim)]
    rng = np.random.default_rng(2)
    x = np.array(g.prob_lo) + (np.array(g.prob_hi) - np.array(g.prob_lo)) * rng.uniform(-0.1, 1.1, size=(500, ndim))
    dt = 0.37
    xn, v1 = tr.advect(g, umac, dt, x)
    for d in range(ndim):
        assert np.abs(v1[:, d] - vel[d]).max() <= 17.5 * EPS * abs(vel[d])
        tol = dt * 18.0 * EPS * abs(vel[d]) + 0.5 * EPS * np.abs(xn[:, d]).max() + 0.5 * EPS * abs(x[:, d]).max()
        assert np.abs(xn[:, d] - (x[:, d] + dt * vel[d])).max() <= tol


def test_periodic_faces_reenter_and_outflow_faces_drop():
    g = geom3(periodic=(1, 0, 0))
    length = g.prob_hi[0] - g.prob_lo[0]
    x = np.array([[g.prob_hi[0] + 0.01, 0.5, 0.5],       # leaves through the periodic top face: re-enters
                  [g.prob_lo[0] - 0.01, 0.5, 0.5],       # ... bottom face
                  [0.0, g.prob_hi[1] + 0.01, 0.5],       # leaves through an outflow face: dropped
                  [0.0, 0.5, g.prob_lo[2] - 1e-12],      # dropped
                  [g.prob_hi[0], 0.5, 0.5],              # exactly on phi: belongs to the next period
                  [np.nextafter(g.prob_lo[0], -np.inf), 0.5, 0.5],  # one ulp below plo: + length lands on phi through rounding -> plo
                  [0.0, 0.5, 0.5]])
    p, keep = tr.redistribute(g, x)
    assert keep.tolist() == [True, True, False, False, True, True, True]
    assert p[0, 0] == x[0, 0] - length and p[1, 0] == x[1, 0] + length
    assert p[4, 0] == x[4, 0] - length and p[5, 0] in (x[5, 0] + length, g.prob_lo[0])
    # a shift that lands exactly on phi through rounding is moved to plo: -1e-17 + 1.0 == 1.0
    g01 = tr.TracerGeom(3, [8, 6, 5], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1, 1, 1])
    p01, k01 = tr.redistribute(g01, np.array([[-1.0e-17, 0.5, 0.5], [1.0, 0.5, 0.5], [2.5, 0.5, 0.5]]))
    assert p01[:, 0].tolist() == [0.0, 0.0, 0.5] and k01.tolist() == [True, True, True]  # (2.5: two periods outside, still shifted in)
    p_bad, k_bad = tr.redistribute(g01, np.array([[np.inf, 0.5, 0.5], [np.nan, 0.5, 0.5], [-7.25, 0.5, 0.5]]))
    assert k_bad.tolist() == [False, False, True] and p_bad[2, 0] == 0.75
    assert np.all((p[keep, 0] >= g.prob_lo[0]) & (p[keep, 0] < g.prob_hi[0]))
    assert np.array_equal(p[:, 1:], x[:, 1:])  # non-periodic directions are not shifted
    # a tracer carried over the periodic face by a uniform flow comes back in at the other side
    umac = [np.full(tr.face_shape(g, d), v) for d, v in enumerate((1.0, 0.0, 0.0))]
    xn, _ = tr.advect(g, umac, 0.02, np.array([[g.prob_hi[0] - 0.01, 0.5, 0.5]]))
    pn, kn = tr.redistribute(g, xn)
    assert kn[0] and abs(pn[0, 0] - (g.prob_lo[0] + 0.01)) < 1e-14


def test_init_one_per_cell_order():
    g = tr.TracerGeom(2, [4, 2], [0.0, 0.0], [1.0, 1.0], [0, 0])
    pos, ids = tr.init_one_per_cell(g, [([0, 0, 0], [1, 1, 0]), ([2, 0, 0], [3, 1, 0])])
    assert ids.tolist() == list(range(1, 9))
    assert pos[:4].tolist() == [[0.125, 0.25], [0.375, 0.25], [0.125, 0.75], [0.375, 0.75]] and pos[4].tolist() == [0.625, 0.25]


def test_assemble_faces_inverts_box_faces():
    g = geom3(n=(8, 8, 8))
    rng = np.random.default_rng(3)
    umac = tr.random_faces(g, rng)
    boxes = [([i, j, k], [i + 3, j + 3, k + 3]) for k in (0, 4) for j in (0, 4) for i in (0, 4)]
    for d in range(3):
        fabs = [tr.box_faces(g, umac[d], d, lo, hi) for lo, hi in boxes]
        assert np.array_equal(tr.assemble_faces(g, d, boxes, fabs), umac[d])


def test_plan_lattice_and_refusal_of_a_level_that_does_not_tile_the_domain():
    """host side of qk_tracer_plan_create on a planning-only context: the lattice granularity is the common divisor of the box edges (remainder
    boxes included); boxes that do not tile the domain are refused with QK_ERR_UNSUPPORTED"""
    from quokka_amd import capi
    from quokka_amd.multifab import Level, PlanningContext
    from quokka_amd.simulation import Geometry, chop_domain
    ctx = PlanningContext()

    def plan(geom, boxes):
        lev = Level(ctx, geom.ndim, boxes)
        gc = geom.c_struct()
        d3 = lambda v: (C.c_double * 3)(*v)
        h = C.c_void_p()
        rc = ctx.L.qk_tracer_plan_create(lev.h, C.byref(h), C.byref(gc), d3(geom.prob_lo), d3(geom.prob_hi), d3(geom.dx))
        if rc != capi.QK_OK:
            return rc, None
        gran, n = (C.c_int * 3)(), C.c_int64()
        assert ctx.L.qk_tracer_plan_lattice(h, gran, C.byref(n)) == capi.QK_OK
        ctx.L.qk_tracer_plan_destroy(h)
        return rc, (list(gran), n.value)

    geom = Geometry(3, [12, 8, 8], [0.0] * 3, [1.5, 1.0, 1.0], [1, 0, 0])
    assert plan(geom, chop_domain([12, 8, 8], [8, 8, 8])) == (capi.QK_OK, ([6, 8, 8], 2))          # 6 + 6
    assert plan(geom, chop_domain([12, 8, 8], [5, 4, 8])) == (capi.QK_OK, ([4, 4, 8], 6))          # 4 + 4 + 4
    geom13 = Geometry(2, [13, 8], [0.0] * 3, [1.0] * 3, [0, 0])
    assert plan(geom13, chop_domain([13, 8, 1], [8, 8, 1])) == (capi.QK_OK, ([1, 8, 1], 13))       # 7 + 6
    boxes = chop_domain([12, 8, 8], [8, 8, 8])
    assert plan(geom, boxes[:1])[0] == capi.QK_ERR_UNSUPPORTED                                     # a hole
    assert plan(geom, [boxes[0], boxes[0]])[0] == capi.QK_ERR_UNSUPPORTED                          # the right number of cells, overlapping
    assert plan(geom, [([0, 0, 0], [12, 7, 7])])[0] == capi.QK_ERR_UNSUPPORTED                     # beyond the domain
