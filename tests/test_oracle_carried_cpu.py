"""The carried form of the RK2 average in the CPU oracle (HydroSim::rk2_carry_rhs, oracle/hydro_sim.hpp): the restatement of the GPU kernel's
formula — stage 1 stores S = U_old + (dt/2) r_1 and P(U_old) per cell, stage 2 finishes S + (dt/2) r_2 — that
tests/test_carried_form_oracle_gpu.py holds the carried kernels to in every bit.  Here, on the CPU: within the parity tolerance of the exact form
(the link to the reference) and not equal to it, through flux corrections and retries, and independent of the box layout (the GPU gates reuse
one oracle run for several layouts) and of the form of the flux evaluation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import SEDOV, Oracle  # noqa: E402


@pytest.fixture(scope="module")
def oracle():
    return Oracle("direct")


def mk(o, n, mgs, carry):
    s = o.sim(SEDOV, 3, [n] * 3, [0, 0, 0], [1.2] * 3, [0, 0, 0], max_grid_size=[mgs] * 3)
    s.set_rk2_carry_rhs(carry)
    return s


def gather(s, n):
    U = np.zeros((s.ncomp, n, n, n))
    for b in range(s.nboxes):
        lo, hi = s.box(b)
        U[:, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = s.valid(b)
    return U


def rel_l1(a, b):
    return [float(np.abs(a[n] - b[n]).sum() / max(np.abs(b[n]).sum(), 1e-300)) for n in range(a.shape[0])]


def test_carried_form_stays_within_the_parity_tolerance_of_the_exact_form(oracle):
    """Sedov 32^3 in 16^3 boxes, 40 steps: <= 1e-12 relative L1 per conserved component, dt within 1e-13, and really the other form"""
    N, nsteps = 32, 40
    a, b = mk(oracle, N, 16, False), mk(oracle, N, 16, True)
    for it in range(nsteps):
        assert a.step() and b.step()
        assert abs(a.dt - b.dt) <= 1e-13 * a.dt, (it, a.dt, b.dt)
    Ua, Ub = gather(a, N), gather(b, N)
    err = rel_l1(Ub, Ua)
    assert max(err) <= 1e-12, err
    assert not np.array_equal(Ua, Ub)
    assert b.counters() == {"fofc1_cells": 0, "fofc2_cells": 0, "retries": 0, "carry2_fallbacks": 0}


def test_carried_form_through_flux_corrections_and_retries(oracle):
    """the over-CFL step of tests/test_hydro_step_gpu.py::test_fofc_and_retries_match_oracle (16^3 in 8^3 boxes, 3 steps, then 6x the CFL step) in
    the carried form: stage 1 is corrected (S keeps its uncorrected r_1), a carried stage 2 flags cells and is redone in the exact form, the advance
    is retried with substeps — and the result stays within the parity tolerance of the exact form"""
    N, mgs = 16, 8
    a, b = mk(oracle, N, mgs, False), mk(oracle, N, mgs, True)
    for _ in range(3):
        assert a.step() and b.step()
    dt = a.compute_dt() * 6.0
    assert a.advance_fixed_dt(dt) and b.advance_fixed_dt(dt)
    cb = b.counters()
    assert cb["fofc1_cells"] > 0 and cb["carry2_fallbacks"] > 0 and cb["retries"] > 0, cb
    assert a.counters()["carry2_fallbacks"] == 0
    err = rel_l1(gather(b, N), gather(a, N))
    assert max(err) <= 1e-12, err
    assert not np.array_equal(gather(a, N), gather(b, N))


def test_carried_form_with_the_fused_flux_evaluation_changes_no_bit(oracle):
    """set_fused_fluxes(True) (oracle/hydro_fused.hpp) in the carried form: the fluxes come from the fused evaluation, the stages from the operator
    path (the whole-stage leg, HydroSim::fusedStage, forms the exact average only and stands aside) — every bit of the operator form, through 8
    steps and an over-CFL step with corrections and retries"""
    N, mgs = 32, 16
    a, b = mk(oracle, N, mgs, True), mk(oracle, N, mgs, True)
    b.set_fused_fluxes(True)
    for it in range(8):
        assert a.step() and b.step()
        assert a.dt == b.dt, it
    assert np.array_equal(gather(a, N), gather(b, N))
    dt = a.compute_dt() * 6.0
    assert a.advance_fixed_dt(dt) and b.advance_fixed_dt(dt)
    assert a.counters() == b.counters() and a.counters()["fofc1_cells"] > 0, (a.counters(), b.counters())
    assert np.array_equal(gather(a, N), gather(b, N))


def test_carried_form_does_not_depend_on_the_box_layout(oracle):
    """32^3 in eight 16^3 boxes == 32^3 in one box, in every bit and every dt: the young blast (12 steps) and the developed shell (3 steps).  The GPU
    gates compare several box layouts with one oracle run of this form."""
    from quokka_amd.simulation import developed_state
    N = 32
    for developed, nsteps in ((False, 12), (True, 3)):
        a, b = mk(oracle, N, 16, True), mk(oracle, N, 32, True)
        if developed:
            for s in (a, b):
                for k in range(s.nboxes):
                    lo, hi = s.box(k)
                    s.set_state(developed_state(N, lo, hi), k, 0)
        for it in range(nsteps):
            assert a.step() and b.step()
            assert a.dt == b.dt, (developed, it)
        assert np.array_equal(gather(a, N), gather(b, N)), developed
