"""The numpy restatement of the tracer kernels on a refined hierarchy (tests/tracer_amr_reference.py) against the single-level one and against
what the rules say by hand.  No GPU."""
import numpy as np

import tracer_amr_reference as ta
import tracer_reference as tr

G0 = tr.TracerGeom(3, [4, 4, 4], [-0.3, 0.1, 0.25], [0.9, 1.0, 1.05], [1, 0, 0])
BOX0 = [([0, 0, 0], [3, 3, 3])]


def faces_of(g, boxes, umac_global):
    return ta.LevelFaces(g, boxes, [[tr.box_faces(g, umac_global[d], d, lo, hi) for lo, hi in boxes] for d in range(g.ndim)])


def two_levels(fine_boxes, seed=3, const=None):
    rng = np.random.default_rng(seed)
    g1 = ta.level_geom(G0, 1)
    mk = (lambda g: tr.random_faces(g, rng)) if const is None else (lambda g: [np.full(tr.face_shape(g, d), const) for d in range(3)])
    u0c, u0p, u1 = mk(G0), mk(G0), mk(g1)
    cur = [faces_of(G0, BOX0, u0c), faces_of(g1, fine_boxes, u1)]
    prev = [faces_of(G0, BOX0, u0p), faces_of(g1, fine_boxes, [np.zeros_like(a) for a in u1])]
    return g1, u0c, u0p, u1, cur, prev


def test_a_refined_level_that_tiles_the_domain_is_the_single_level_advect():
    tiles = [([0, 0, 0], [3, 7, 7]), ([4, 0, 0], [7, 7, 3]), ([4, 0, 4], [7, 7, 7])]
    g1, _, _, u1, cur, prev = two_levels(tiles)
    rng = np.random.default_rng(5)
    pos = np.array(G0.prob_lo) + (np.array(G0.prob_hi) - np.array(G0.prob_lo)) * rng.uniform(-0.1, 1.1, size=(500, 3))
    dt = 2.0 * min(g1.dx)
    x, v = ta.advect(cur, prev, 1, 0.75, 0.25, dt, pos)
    xr, vr = tr.advect(g1, u1, dt, pos)
    assert np.array_equal(x, xr) and np.array_equal(v, vr)
    for d in range(3):
        assert np.array_equal(ta.compose_field(cur, prev, 1, 0.75, 0.25)[d], u1[d])


def test_a_constant_field_gives_that_constant_on_every_fallback_face():
    """(1 - w) c + w c with w in {0, 0.5} and alpha c + beta c with alpha + beta = 1 in binary fractions are exact"""
    fine = [([2, 2, 2], [5, 5, 5])]
    c = 0.3
    for alpha, beta in ((0.75, 0.25), (0.25, 0.75), (0.0, 1.0), (1.0, 0.0)):
        _, _, _, _, cur, prev = two_levels(fine, const=c)
        for d in range(3):
            held, _ = ta.held_and_own(cur[1], d)
            assert not held.all() and held.any()
            f = ta.compose_field(cur, prev, 1, alpha, beta)[d]
            assert np.array_equal(f, np.full(f.shape, c))


def test_even_faces_return_the_coarse_value_and_odd_ones_the_mean():
    fine = [([2, 2, 2], [5, 5, 5])]
    g1, u0c, u0p, _, cur, prev = two_levels(fine)
    for alpha, beta, G in ((0.0, 1.0, u0c), (1.0, 0.0, u0p), (0.25, 0.75, [0.25 * p + 0.75 * c for p, c in zip(u0p, u0c)])):
        for d in range(3):
            f = ta.compose_field(cur, prev, 1, alpha, beta)[d]
            held, own = ta.held_and_own(cur[1], d)
            assert np.array_equal(f[held], own[held])
            n_even = n_odd = 0
            for idx in np.argwhere(~held):
                i = idx[::-1]  # (i0, i1, i2)
                c = [int(x) // 2 for x in i]
                if G0.periodic[d]:
                    c[d] %= G0.n_cell[d]  # (face N of a periodic direction is face 0; no stencil reads it)
                lo = G[d][c[2], c[1], c[0]]
                if i[d] % 2 == 0:
                    assert f[tuple(idx)] == lo
                    n_even += 1
                else:
                    c[d] = (c[d] + 1) % G0.n_cell[d] if G0.periodic[d] else min(c[d] + 1, G0.n_cell[d])
                    assert f[tuple(idx)] == 0.5 * lo + 0.5 * G[d][c[2], c[1], c[0]]
                    n_odd += 1
            assert n_even > 0 and n_odd > 0


def test_three_levels_fall_through_two():
    """a level-2 box flush against level 1's edge: its outer faces come from level 0 through level 1's rule"""
    rng = np.random.default_rng(9)
    g1, g2 = ta.level_geom(G0, 1), ta.level_geom(G0, 2)
    b1, b2 = [([2, 2, 2], [5, 5, 5])], [([4, 4, 4], [7, 7, 11])]  # level 2 reaches fine cell 11 = level-1 cell 5, level 1's edge
    u = [tr.random_faces(g, rng) for g in (G0, g1, g2)]
    cur = [faces_of(G0, BOX0, u[0]), faces_of(g1, b1, u[1]), faces_of(g2, b2, u[2])]
    f = ta.compose_field(cur, cur, 2, 0.0, 1.0)
    # face (i, j, k) = (4, 4, 13) of direction x on level 2: not held; parent face (2, 2, 6) on level 1: cell k = 6 is outside [2, 5]: level 0's (1, 1, 3)
    assert f[0][13, 4, 4] == u[0][0][3, 1, 1]
    # odd in x on level 2, the parent's faces again from level 0 (even and odd there)
    assert f[0][13, 4, 5] == 0.5 * u[0][0][3, 1, 1] + 0.5 * (0.5 * u[0][0][3, 1, 1] + 0.5 * u[0][0][3, 1, 2])


def test_where():
    g = [G0, ta.level_geom(G0, 1), ta.level_geom(G0, 2)]
    boxes = [BOX0, [([2, 2, 2], [5, 5, 5])], [([6, 6, 6], [9, 9, 9])]]
    dx0 = np.array(G0.dx)
    lo = np.array(G0.prob_lo)
    cell0 = lambda i, j, k: lo + (np.array([i, j, k]) + 0.5) * dx0
    pos = np.array([cell0(0, 0, 0), cell0(1, 1, 1) - 0.2 * dx0, cell0(2, 2, 2) - 0.3 * dx0, cell0(0, 3, 3), lo + np.array([-0.5, 2.0, 2.0]) * dx0,
                    lo + np.array([1.0, -0.1, 1.0]) * dx0])
    level = np.zeros(6, dtype=np.int32)
    p, new, keep = ta.where(g, boxes, 0, 0, pos, level)
    assert keep.tolist() == [True, True, True, True, True, False]
    assert new.tolist() == [0, 1, 2, 0, 0, -1]
    assert p[4, 0] == pos[4, 0] + (G0.prob_hi[0] - G0.prob_lo[0])  # periodic in x
    # ngrow: a particle of level 1 half a coarse cell outside its box stays with ngrow = 1 (one fine cell) and 2, leaves with 0
    q = np.array([lo + np.array([0.75, 1.6, 1.6]) * dx0, lo + np.array([0.25, 1.6, 1.6]) * dx0, cell0(1, 1, 1) + 0.6 * dx0])
    lv = np.array([1, 1, 1], dtype=np.int32)
    assert ta.where(g, boxes, 1, 0, q, lv)[1].tolist() == [0, 0, 2]
    assert ta.where(g, boxes, 1, 1, q, lv)[1].tolist() == [1, 0, 1]  # (inside its own level: it stays although level 2 holds the cell)
    assert ta.where(g, boxes, 1, 2, q, lv)[1].tolist() == [1, 1, 1]
