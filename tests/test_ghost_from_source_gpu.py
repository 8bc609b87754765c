"""qk_hydro_stage_args::ghost_from_source on the GPU: the fused stages of the carried form read every cell outside a box from the valid cell the ghost
fill would have copied, and the two fills of a step are not run.  Each case compares against today's path (ghost_from_source off: fills on) in every
bit of every valid cell and of dt after 3 RK2 steps from the developed blast, carried form with the primitive hand-off, asserts that no fill ran
during those steps, then fills explicitly and compares the ghost cells too.  The first-order correction takes the fallback (fills first) and a
level that is not a lattice is refused by the qualification test; both stay bit-equal.  The host-side plan alone: tests/test_ghost_source_plan.py."""
import numpy as np
import pytest

from quokka_amd import capi
from quokka_amd.simulation import Geometry, HydroSimulation, developed_state, sedov_problem

pytestmark = pytest.mark.gpu


def hydro_bcs(lo_t, hi_t):
    def one(kind, n, d):
        if kind == "reflect":
            return capi.BC_REFLECT_ODD if n == 1 + d else capi.BC_REFLECT_EVEN
        return {"extrap": capi.BC_FOEXTRAP, "periodic": capi.BC_INT_DIR}[kind]
    return [([one(lo_t[d], n, d) for d in range(3)], [one(hi_t[d], n, d) for d in range(3)]) for n in range(6)]


def count_fills(sim):
    """every route of a HydroSimulation to qk_FillBoundary_* / qk_FillPhysicalBoundary* goes through GhostExchange.fill_with"""
    calls = []
    inner = sim.ghost.fill_with

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    sim.ghost.fill_with = counted
    return calls


def lattice_sim(ctx, nb, blen, lo_t, hi_t, N, gfs, boxes=None):
    n_cell = [nb[d] * blen[d] for d in range(3)]
    geom = Geometry(3, n_cell, [0.0] * 3, [1.2 * n_cell[d] / N for d in range(3)], [int(lo_t[d] == "periodic") for d in range(3)])
    if boxes is None:
        boxes = [([i * blen[0], j * blen[1], k * blen[2]], [(i + 1) * blen[0] - 1, (j + 1) * blen[1] - 1, (k + 1) * blen[2] - 1])
                 for k in range(nb[2]) for j in range(nb[1]) for i in range(nb[0])]
    s = HydroSimulation(ctx, geom, capi.traits(1.4, False, 3), hydro_bcs(lo_t, hi_t), list(blen), boxes=boxes, owner=[0] * len(boxes))
    s.reconstructionOrder_, s.stopTime_, s.cflNumber_ = 3, 1.0, 0.3
    s.rk2_carry_rhs = True
    s.prim_handoff = True
    s.ghost_from_source = gfs
    for b, (lo, hi) in enumerate(s.my_boxes):
        s.state_new_cc_.set_fab(b, developed_state(N, lo, hi))
    s._signal_of_state_new = None
    return s


def run_pair(make, nsteps=3):
    """(flag off, flag on): dts, valid cells and — after one explicit fill — whole fabs, fills counted during the steps"""
    out = []
    for gfs in (False, True):
        s = make(gfs)
        calls = count_fills(s)
        dts = []
        for _ in range(nsteps):
            assert s.step()
            dts.append(s.dt_)
        during = len(calls)
        valid = [v.copy() for v in s.gather_valid_local()]
        s.fillBoundaryConditions(s.state_new_cc_)
        fabs = [s.state_new_cc_.fab_numpy(b).copy() for b in range(s.lev.nboxes)]
        out.append((s, dts, valid, fabs, during))
    return out


def assert_same_bits(off, on):
    assert off[1] == on[1], "dt differs"
    for b, (x, y) in enumerate(zip(off[2], on[2])):
        assert np.isfinite(x).all()
        assert np.array_equal(x, y), f"box {b}: {int((x != y).sum())} valid values differ"
    for b, (x, y) in enumerate(zip(off[3], on[3])):
        assert np.array_equal(x, y), f"box {b}: ghost cells differ after the explicit fill"


REFL, EXT, PER = ("reflect",) * 3, ("extrap",) * 3, ("periodic",) * 3
CASES = [
    # the benchmark's octant: 2 x 2 x 2 boxes of 64 x 16 x 16, reflecting low faces, extrapolating high faces
    pytest.param((2, 2, 2), (64, 16, 16), REFL, EXT, 128, id="octant-2x2x2"),
    pytest.param((2, 2, 2), (64, 16, 16), PER, PER, 128, id="periodic-2x2x2"),
    # one box, its own neighbour on all six faces
    pytest.param((1, 1, 1), (64, 16, 16), PER, PER, 128, id="periodic-one-box"),
    # two chunks per row, a march shorter than one batch of wave-edge faces, a mirrored source inside the edge batch
    pytest.param((2, 1, 1), (128, 8, 8), ("reflect", "periodic", "periodic"), ("reflect", "periodic", "periodic"), 256, id="reflect-x-2x1x1"),
]


@pytest.mark.parametrize("nb,blen,lo_t,hi_t,N", CASES)
def test_stage_reads_across_box_faces_bit_for_bit(ctx, nb, blen, lo_t, hi_t, N):
    off, on = run_pair(lambda gfs: lattice_sim(ctx, nb, blen, lo_t, hi_t, N, gfs))
    for s in (off[0], on[0]):
        assert s.counters["fofc1_stages"] + s.counters["fofc2_stages"] + s.counters["retries"] == 0, "the case must not leave the fused path"
        assert s.counters.get("prim_handoff_dropped", 0) == 0
    assert not off[0]._ghost_from_source_applies() and on[0]._ghost_from_source_applies()
    assert off[4] == 2 * 3, "today's path fills once per stage"
    assert on[4] == 0, "a fill ran during the steps"
    assert_same_bits(off, on)


def test_first_order_correction_takes_the_fallback(ctx):
    """the forcing of tests/test_hydro_step_gpu.py (three steps of the point blast, then one step at six times the CFL step): cells are flagged,
    the attempt with the hand-off is dropped, the correction passes and the retries read filled ghost cells — the fills run first"""
    out = []
    for gfs in (False, True):
        s = sedov_problem(ctx, 64, max_grid_size=[64, 16, 16])
        s.rk2_carry_rhs = True
        s.prim_handoff = True
        s.ghost_from_source = gfs
        assert s._ghost_from_source_applies() == gfs
        calls = count_fills(s)
        dts = []
        for _ in range(3):
            assert s.step()
            dts.append(s.dt_)
        before = len(calls)
        assert before == (0 if gfs else 6)
        s.computeTimestep()
        assert s.step(s.dt_ * 6.0)
        dts.append(s.dt_)
        assert s.counters["fofc1_stages"] + s.counters["fofc2_stages"] > 0, s.counters
        assert len(calls) > before, "the correction ran on ghost cells nobody filled"
        assert s.step()
        dts.append(s.dt_)
        valid = [v.copy() for v in s.gather_valid_local()]
        out.append((s, dts, valid, [], len(calls), dict(s.counters)))
    assert out[0][5] == out[1][5]
    assert_same_bits(out[0], out[1])


def test_level_that_is_not_a_lattice_is_refused(ctx):
    """two boxes of different sizes: the qualification test says no and the stage runs today's path"""
    boxes = [([0, 0, 0], [127, 15, 15]), ([128, 0, 0], [191, 15, 15])]
    off, on = run_pair(lambda gfs: lattice_sim(ctx, (1, 1, 1), (192, 16, 16), REFL, EXT, 192, gfs, boxes=boxes))
    assert not on[0]._ghost_from_source_applies() and on[0]._gfs_qualifies is False
    assert off[4] == on[4] == 6
    assert_same_bits(off, on)
