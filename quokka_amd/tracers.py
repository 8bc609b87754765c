"""Tracer particles on one rank, per level (reference src/simulation.hpp:398, :593, :1993-2005, :1317-1329; src/QuokkaSimulation.hpp:1290-1314):
one particle per cell, advected with the time-averaged face velocity of the RK2 step.

Host plumbing only: the particle arrays are torch tensors (structure of arrays, as the C-ABI takes them), every particle is moved by the HIP kernels
of csrc/qk_tracer.hip.  Compaction after a Redistribute that dropped particles is a boolean mask over the arrays, order-preserving.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import capi
from .multifab import MultiFab


def _d3(v: Sequence[float]):
    return (C.c_double * 3)(*[float(x) for x in (list(v) + [0.0, 0.0, 0.0])[:3]])


PREV, CUR = 0, 1  # QK_TRACER_PREV / QK_TRACER_CUR


class TracerPlan:
    """qk_tracer_plan of one level: the cell -> box lattice and the geometry.  refined = True: the boxes need not tile the domain
    (qk_tracer_plan_create_refined); AdvectWithUmac then needs the links to the parent level's plans and face arrays (set_parent)."""

    def __init__(self, ctx, lev, geom, refined: bool = False, boxes=None):
        self.ctx, self.lev, self.geom, self.refined = ctx, lev, geom, refined
        self.boxes = [(list(lo), list(hi)) for lo, hi in boxes] if boxes is not None else None  # (host copy, for read-out)
        self._geom_c = geom.c_struct()
        h = C.c_void_p()
        fn = ctx.L.qk_tracer_plan_create_refined if refined else ctx.L.qk_tracer_plan_create
        ctx.check(fn(lev.h, C.byref(h), C.byref(self._geom_c), _d3(geom.prob_lo), _d3(geom.prob_hi), _d3(geom.dx)),
                  "qk_tracer_plan_create_refined" if refined else "qk_tracer_plan_create")
        self.h = h
        self._linked = {}  # kind -> (parent plan, its face arrays): the library keeps their pointers, this keeps them alive

    def set_parent(self, kind: int, parent: "TracerPlan", umac: Sequence[MultiFab]):
        """the parent level's plan and face arrays of one kind (PREV: its previous step, with the boxes that step had; CUR: its current step)"""
        nd = self.geom.ndim
        for d in range(nd):
            assert umac[d].facedir == d and umac[d].ncomp == 1 and umac[d].nghost == 0 and umac[d].level is parent.lev
        tabs = (C.c_void_p * 3)(*[umac[d].ptr if d < nd else None for d in range(3)])
        self.ctx.check(self.ctx.L.qk_tracer_plan_set_parent(self.h, int(kind), parent.h, tabs), "qk_tracer_plan_set_parent")
        self._linked[kind] = (parent, list(umac[:nd]))

    def set_time_weights(self, alpha: float, beta: float):
        self.ctx.check(self.ctx.L.qk_tracer_plan_set_time_weights(self.h, float(alpha), float(beta)), "qk_tracer_plan_set_time_weights")

    def clear_parent(self):
        self.ctx.check(self.ctx.L.qk_tracer_plan_clear_parent(self.h), "qk_tracer_plan_clear_parent")
        self._linked = {}

    def __del__(self):
        try:
            self.ctx.L.qk_tracer_plan_destroy(self.h)
        except Exception:
            pass


def where(ctx, plans: Sequence[TracerPlan], lev_min: int, ngrow: int, pos: Sequence[torch.Tensor], level: torch.Tensor):
    """qk_tracer_Where: (new level per particle (int32, -1 = dropped), keep (bool)); `pos` is shifted in place in the periodic directions"""
    n = int(level.numel())
    new = torch.empty(n, dtype=torch.int32, device=ctx.device)
    keep = torch.empty(n, dtype=torch.bool, device=ctx.device)
    if n == 0:
        return new, keep
    assert level.dtype == torch.int32 and level.is_contiguous()
    hs = (C.c_void_p * len(plans))(*[p.h for p in plans])
    ctx.check(ctx.L.qk_tracer_Where(hs, len(plans), ctx.stream(), int(lev_min), int(ngrow), n, TracerParticles._ptrs(pos), C.c_void_p(level.data_ptr()),
                                    C.c_void_p(new.data_ptr()), C.c_void_p(keep.data_ptr())), "qk_tracer_Where")
    return new, keep


class TracerParticles:
    """amrex::TracerParticleContainer for a HydroSimulation, or for one level of an AmrSimulation (refined = True: a TracerPlan whose boxes need
    not tile the domain): pos / vel (double, per direction), id (int64), cpu (int32) in device memory."""

    def __init__(self, sim, refined: bool = False):
        self.sim, self.ctx, self.lev, self.geom = sim, sim.ctx, sim.lev, sim.geom
        self.ndim = sim.geom.ndim
        self.plan = TracerPlan(self.ctx, self.lev, self.geom, refined, getattr(sim, "my_boxes", None))
        self.last_keep = None
        self._alloc(0)

    @property
    def h(self):
        return self.plan.h

    def _alloc(self, n: int):
        dev = self.ctx.device
        self.pos: List[torch.Tensor] = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(self.ndim)]
        self.vel: List[torch.Tensor] = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(self.ndim)]
        self.id = torch.zeros(n, dtype=torch.int64, device=dev)
        self.cpu = torch.zeros(n, dtype=torch.int32, device=dev)

    @staticmethod
    def _ptrs(arrs: Sequence[torch.Tensor]):
        return (C.c_void_p * 3)(*[C.c_void_p(a.data_ptr()) if a.numel() > 0 else None for a in arrs] + [None] * (3 - len(arrs)))

    @property
    def num_particles(self) -> int:
        return int(self.id.numel())

    def lattice(self):
        """(granularity per direction, number of entries) of the plan's cell -> box lattice"""
        gran, n = (C.c_int * 3)(), C.c_int64()
        self.ctx.check(self.ctx.L.qk_tracer_plan_lattice(self.h, gran, C.byref(n)), "qk_tracer_plan_lattice")
        return list(gran), int(n.value)

    # ------------------------------------------------------------------ the three operations
    def init_one_per_cell(self, off: Sequence[float] = (0.5, 0.5, 0.5), first_id: int = 1):
        """InitOnePerCell(0.5, 0.5, 0.5, pdata) (reference src/simulation.hpp:1993-2005).  Ids run from `first_id` over the boxes in order, cells
        in Fortran order: this project's numbering."""
        self._alloc(self.lev.num_cells())
        if self.num_particles == 0:
            return
        c = self.ctx
        c.check(c.L.qk_tracer_InitOnePerCell(self.h, c.stream(), _d3(off), self._ptrs(self.pos), self._ptrs(self.vel), C.c_void_p(self.id.data_ptr()),
                                            C.c_void_p(self.cpu.data_ptr()), int(first_id), int(self.sim.rank)), "qk_tracer_InitOnePerCell")

    def advect(self, umac: Sequence[MultiFab], dt: float):
        """AdvectWithUmac(umac, lev, dt): umac[d] face-centred in d, one component, no ghost faces.  The driver hands over avgFaceVel of the
        stage-2 attempt that stood (HydroSimulation._avg_face_vel): the operators' rk2vel, or velRk2 of the fused stage 2 (tracers_on_fused_stages)"""
        assert len(umac) >= self.ndim
        for d in range(self.ndim):
            assert umac[d].facedir == d and umac[d].ncomp == 1 and umac[d].nghost == 0 and umac[d].level is self.lev
        if self.num_particles == 0:
            return
        c = self.ctx
        tabs = (C.c_void_p * 3)(*[umac[d].ptr if d < self.ndim else None for d in range(3)])
        c.check(c.L.qk_tracer_AdvectWithUmac(self.h, c.stream(), tabs, float(dt), self.num_particles, self._ptrs(self.pos), self._ptrs(self.vel)),
                "qk_tracer_AdvectWithUmac")

    def redistribute(self) -> int:
        """Redistribute(lev, lev, ngrow = 0): periodic shift, particles beyond a non-periodic face dropped.  Returns the number dropped."""
        n = self.num_particles
        c = self.ctx
        keep = self.last_keep = torch.empty(n, dtype=torch.bool, device=c.device)  # (kept: which particles of the last call stayed)
        if n == 0:
            return 0
        c.check(c.L.qk_tracer_Redistribute(self.h, c.stream(), n, self._ptrs(self.pos), C.c_void_p(keep.data_ptr())), "qk_tracer_Redistribute")
        if bool(keep.all()):  # (one device -> host read per step)
            return 0
        self.pos = [a[keep] for a in self.pos]
        self.vel = [a[keep] for a in self.vel]
        self.id, self.cpu = self.id[keep], self.cpu[keep]
        return n - self.num_particles

    # ------------------------------------------------------------------ retries, save and restore
    def snapshot(self) -> Dict[str, object]:
        return {"pos": [a.clone() for a in self.pos], "vel": [a.clone() for a in self.vel], "id": self.id.clone(), "cpu": self.cpu.clone()}

    def restore(self, snap: Dict[str, object]):
        """back to a snapshot(); the snapshot stays usable for further retries"""
        self.pos = [a.clone() for a in snap["pos"]]
        self.vel = [a.clone() for a in snap["vel"]]
        self.id, self.cpu = snap["id"].clone(), snap["cpu"].clone()

    def positions(self) -> np.ndarray:
        return torch.stack(self.pos, dim=1).cpu().numpy() if self.num_particles else np.zeros((0, self.ndim))

    def velocities(self) -> np.ndarray:
        return torch.stack(self.vel, dim=1).cpu().numpy() if self.num_particles else np.zeros((0, self.ndim))

    def ids(self) -> np.ndarray:
        return self.id.cpu().numpy()

    def load(self, positions, velocities, ids):
        """take over the particles of a saved run: positions / velocities (np, ndim), ids (np,); cpu = this rank"""
        p, v, i = np.asarray(positions, dtype=np.float64), np.asarray(velocities, dtype=np.float64), np.asarray(ids, dtype=np.int64)
        if p.ndim != 2 or p.shape[1] != self.ndim or v.shape != p.shape or i.shape != (p.shape[0],):
            raise capi.QkError(f"TracerParticles.load: expected positions and velocities of shape (np, {self.ndim}) and ids of shape (np,)")
        dev = self.ctx.device
        self.pos = [torch.from_numpy(np.ascontiguousarray(p[:, d])).to(dev) for d in range(self.ndim)]
        self.vel = [torch.from_numpy(np.ascontiguousarray(v[:, d])).to(dev) for d in range(self.ndim)]
        self.id = torch.from_numpy(np.ascontiguousarray(i)).to(dev)
        self.cpu = torch.full((p.shape[0],), int(self.sim.rank), dtype=torch.int32, device=dev)

    def take(self, pos, vel, ids, cpu):
        """take over device arrays as they are (the AMR driver's Redistribute)"""
        self.pos, self.vel, self.id, self.cpu = list(pos), list(vel), ids, cpu
