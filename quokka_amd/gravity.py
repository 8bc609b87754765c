"""Self-gravity on one level and one rank (reference src/simulation.hpp:665, :883, :1011-1095; src/QuokkaSimulation.hpp:709-757): lap(phi) = 4 pi G rho
with open boundaries by James' method on the lattice, then the operator-split kick.  DESIGN.md §13 defines the discrete problem.

Host plumbing only: the dense arrays are torch tensors, every cell is touched by the HIP kernels of csrc/qk_gravity.hip.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import capi
from .multifab import MultiFab


def _i3(n: Sequence[int]):
    return (C.c_int * 3)(*[int(x) for x in n])


class NotConverged(capi.QkError):
    """a Dirichlet solve did not reach its tolerance within max_iter cycles"""


class PoissonSolver:
    """The open-boundary solve on the lattice n = (N0, N1, N2) with spacing h.  `phi`, `rhs`: dense (N2+2, N1+2, N0+2) device arrays (x fastest);
    the ghost layer of `phi` holds the boundary data the kick reads.  After solve_open: `cycles` = (V-cycles of step 1, of step 4), `resnorm`
    likewise, `s` and `bc` the screening values and boundary data in ghost-list order."""

    def __init__(self, ctx, n: Sequence[int], h: float):
        self.ctx, self.n, self.h = ctx, [int(x) for x in n], float(h)
        self._n = _i3(self.n)
        L = ctx.L
        nbytes = int(L.qk_gravity_scratch_bytes(self._n))
        self.S = int(L.qk_gravity_num_ghosts(self._n))
        if nbytes < 0 or self.S < 0:
            raise capi.QkError(f"doPoissonSolve_: self-gravity needs an even cell count of 4 .. 4096 in every direction, not {self.n}")
        dev = ctx.device
        shape = (self.n[2] + 2, self.n[1] + 2, self.n[0] + 2)
        self.phi = torch.zeros(shape, dtype=torch.float64, device=dev)
        self.rhs = torch.zeros(shape, dtype=torch.float64, device=dev)
        self.s = torch.zeros(self.S, dtype=torch.float64, device=dev)
        self.bc = torch.zeros(self.S, dtype=torch.float64, device=dev)
        self.scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        self.max_iter = 100
        self.cycles, self.resnorm = (0, 0), (0.0, 0.0)

    @staticmethod
    def _p(t: torch.Tensor) -> C.c_void_p:
        return C.c_void_p(t.data_ptr())

    def zero_rhs(self):
        c = self.ctx
        c.check(c.L.qk_clear_bytes(c.h, c.stream(), self._p(self.rhs), self.rhs.numel() * 8), "qk_clear_bytes")

    def zero_phi(self):
        c = self.ctx
        c.check(c.L.qk_clear_bytes(c.h, c.stream(), self._p(self.phi), self.phi.numel() * 8), "qk_clear_bytes")

    def fill_rhs(self, lev, state: MultiFab, G: float, density_comp: int = 0):
        """rhs += 4 pi G rho (fillPoissonRhsAtLevel)"""
        c = self.ctx
        c.check(c.L.qk_gravity_fill_rhs(lev.h, c.stream(), float(G), state.ptr, int(density_comp), self._n, self._p(self.rhs)), "qk_gravity_fill_rhs")

    def solve_dirichlet(self, reltol: float, abstol: float, max_iter=None):
        """L phi = rhs with the ghost layer of phi as data and its interior as the first guess.  Returns (cycles, max |rhs - L phi|); raises
        NotConverged where the tolerance is not reached."""
        c = self.ctx
        it, res = C.c_int(0), C.c_double(0.0)
        rc = c.L.qk_gravity_dirichlet_solve(c.h, c.stream(), self._n, self.h, self._p(self.rhs), self._p(self.phi), float(reltol), float(abstol),
                                            int(self.max_iter if max_iter is None else max_iter), self._p(self.scratch), self.scratch.numel() * 8,
                                            C.byref(it), C.byref(res))
        if rc == capi.QK_ERR_NOT_CONVERGED:
            raise NotConverged(f"qk_gravity_dirichlet_solve: max |rhs - L phi| = {res.value:.6e} after {it.value} V-cycles (status {rc}): "
                               f"{c.L.qk_last_error(c.h).decode()}")
        c.check(rc, "qk_gravity_dirichlet_solve")
        return it.value, res.value

    def surface_gather(self):
        c = self.ctx
        c.check(c.L.qk_gravity_surface_gather(c.h, c.stream(), self._n, self._p(self.phi), self._p(self.s)), "qk_gravity_surface_gather")

    def surface_potential(self):
        c = self.ctx
        c.check(c.L.qk_gravity_surface_potential(c.h, c.stream(), self._n, self._p(self.s), self._p(self.bc), self._p(self.scratch),
                                                 self.scratch.numel() * 8), "qk_gravity_surface_potential")

    def surface_scatter(self):
        c = self.ctx
        c.check(c.L.qk_gravity_surface_scatter(c.h, c.stream(), self._n, self._p(self.bc), self._p(self.phi)), "qk_gravity_surface_scatter")

    def solve_open(self, reltol: float, abstol: float):
        """steps 1-4 of James' method on the lattice from the rhs as it stands; phi of step 1 is the first guess of step 4"""
        self.zero_phi()
        it0, r0 = self.solve_dirichlet(reltol, abstol)
        self.surface_gather()
        self.surface_potential()
        self.surface_scatter()
        it1, r1 = self.solve_dirichlet(reltol, abstol)
        self.cycles, self.resnorm = (it0, it1), (r0, r1)

    def kick(self, lev, state: MultiFab, dx: Sequence[float], dt: float):
        """applyPoissonGravityAtLevel on the valid cells of `state`"""
        c = self.ctx
        c.check(c.L.qk_gravity_kick(lev.h, c.stream(), self._n, self._p(self.phi), (C.c_double * 3)(*[float(x) for x in dx]), float(dt), state.ptr),
                "qk_gravity_kick")


def check_supported(sim, need_cic_container: bool = True):
    """what the self-gravity solver is built for: a plain HydroSimulation, one rank, 3-D, cubic cells; CIC particles (do_cic_particles) with their
    container in place (need_cic_container = False: the call that creates it) — refused by name otherwise"""
    from .simulation import HydroSimulation
    if type(sim) is not HydroSimulation:
        raise capi.QkError(f"doPoissonSolve_: self-gravity is built for HydroSimulation (one level, hydro only), not for {type(sim).__name__}")
    if sim.nranks > 1:
        raise capi.QkError("doPoissonSolve_: self-gravity is built for one rank (nranks > 1: the dense potential is not distributed)")
    if sim.geom.ndim < 3:
        raise capi.QkError(f"doPoissonSolve_: self-gravity is built for ndim = 3 (as the reference: AMREX_SPACEDIM == 3), not ndim = {sim.geom.ndim}")
    dx = sim.geom.dx
    if any(not (abs(dx[d] - dx[0]) <= 1.0e-12 * abs(dx[0])) for d in (1, 2)):
        raise capi.QkError(f"doPoissonSolve_: self-gravity is built for cubic cells (dx equal in all directions to 1e-12 relative), not dx = {dx}")
    if getattr(sim, "do_cic_particles", 0) and need_cic_container and getattr(sim, "CICParticles", None) is None:
        raise capi.QkError("doPoissonSolve_: CIC particles (do_cic_particles) have no container: the switch was set after set_initial_conditions, "
                           "which creates it — call InitCICParticles()")
