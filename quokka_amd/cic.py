"""Massive cloud-in-cell particles on one level and one rank (reference src/simulation.hpp:652-653, :2007-2016, :1043-1047, :1107-1216, :1330-1341;
src/particles/CICParticles.hpp): they are deposited into the Poisson right-hand side before the gas, kicked by the potential and drifted.
DESIGN.md §14 defines the discrete operations — this project's definition, not AMReX's ParticleToMesh / ParticleInterpolator.

Host plumbing only: the particle arrays are torch tensors (structure of arrays, as the C-ABI takes them), every particle and every cell is touched by
the HIP kernels of csrc/qk_cic.hip.  Between the key kernel and the deposit kernel the keys are sorted (torch.sort, stable) and the range of every
base cell is looked up (torch.searchsorted); compaction after a Redistribute that dropped particles is a boolean mask, order-preserving.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np
import torch

from . import capi
from .tracers import TracerPlan, where


def _d3(v: Sequence[float]):
    return (C.c_double * 3)(*[float(x) for x in v])


def _i3(n: Sequence[int]):
    return (C.c_int * 3)(*[int(x) for x in n])


class CICParticles:
    """quokka::CICParticleContainer for a HydroSimulation: pos / vel (double, per direction), mass (double), id (int64, from 1 in creation order),
    cpu (int32) in device memory.  `num_dropped`: how many particles Redistribute has removed so far."""

    def __init__(self, sim):
        if sim.geom.ndim != 3:
            raise capi.QkError(f"CIC particles are built for ndim = 3, not ndim = {sim.geom.ndim}")
        self.sim, self.ctx, self.lev, self.geom = sim, sim.ctx, sim.lev, sim.geom
        self.plan = TracerPlan(self.ctx, self.lev, self.geom, False, getattr(sim, "my_boxes", None))
        self._n, self._plo, self._dx = _i3(self.geom.n_cell), _d3(self.geom.prob_lo), _d3(self.geom.dx)
        n = self.geom.n_cell
        self.num_keys = (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
        self._cells = None  # 0 .. num_keys on the device, made by the first deposit
        self.num_dropped = 0
        self.last_keep = None
        self._next_id = 1
        self._alloc(0)

    def _alloc(self, n: int):
        dev = self.ctx.device
        self.pos: List[torch.Tensor] = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3)]
        self.vel: List[torch.Tensor] = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3)]
        self.mass = torch.zeros(n, dtype=torch.float64, device=dev)
        self.id = torch.zeros(n, dtype=torch.int64, device=dev)
        self.cpu = torch.zeros(n, dtype=torch.int32, device=dev)

    @staticmethod
    def _ptrs(arrs: Sequence[torch.Tensor]):
        return (C.c_void_p * 3)(*[C.c_void_p(a.data_ptr()) if a.numel() > 0 else None for a in arrs])

    @staticmethod
    def _p(t: torch.Tensor):
        return C.c_void_p(t.data_ptr()) if t.numel() > 0 else None

    @property
    def num_particles(self) -> int:
        return int(self.id.numel())

    # ------------------------------------------------------------------ creation
    def init_from_arrays(self, pos, mass, vel):
        """the particles of this container: pos (np, 3), mass (np,), vel (np, 3); ids from 1 in the order given.  Non-finite values are refused."""
        p, m, v = np.asarray(pos, dtype=np.float64), np.asarray(mass, dtype=np.float64), np.asarray(vel, dtype=np.float64)
        p, v = p.reshape(-1, 3) if p.size == 0 else p, v.reshape(-1, 3) if v.size == 0 else v
        if p.ndim != 2 or p.shape[1] != 3 or v.shape != p.shape or m.shape != (p.shape[0],):
            raise capi.QkError("CIC particles: expected pos and vel of shape (np, 3) and mass of shape (np,)")
        for name, a in (("positions", p), ("masses", m), ("velocities", v)):
            if not np.isfinite(a).all():
                raise capi.QkError(f"CIC particles: {name} that are not finite are refused")
        self._next_id = 1
        self.load(p, v, m, np.arange(self._next_id, self._next_id + p.shape[0], dtype=np.int64))
        self._next_id += p.shape[0]

    def init_from_ascii_file(self, path: str):
        """InitFromAsciiFile(path, nreal_extra = 4): the first line is the count, then `x y z mass vx vy vz` per line (the reference's
        BinaryOrbit_particles.txt)"""
        with open(path) as f:
            tok = f.read().split()
        if not tok:
            raise capi.QkError(f"CIC particles: {path} is empty")
        try:
            n = int(tok[0])
            vals = np.array([float(t) for t in tok[1:]], dtype=np.float64)
        except ValueError as e:
            raise capi.QkError(f"CIC particles: {path}: {e}")
        if n < 0 or vals.size != 7 * n:
            raise capi.QkError(f"CIC particles: {path} announces {tok[0]} particles of 7 numbers (x y z mass vx vy vz) and holds {vals.size} numbers")
        vals = vals.reshape(n, 7)
        self.init_from_arrays(vals[:, 0:3], vals[:, 3], vals[:, 4:7])

    def init_random(self, n: int, seed: int, mass: float, vel=(0.0, 0.0, 0.0)):
        """n particles of one mass and velocity, uniform in the domain from numpy.random.default_rng(seed): x_d = lo_d + u * (hi_d - lo_d), the
        three coordinates of a particle drawn together.  This project's own stream — NOT the positions AMReX's InitRandom would give."""
        rng = np.random.default_rng(int(seed))
        lo, hi = np.array(self.geom.prob_lo[:3], dtype=np.float64), np.array(self.geom.prob_hi[:3], dtype=np.float64)
        p = lo[None, :] + rng.random((int(n), 3)) * (hi - lo)[None, :]
        self.init_from_arrays(p, np.full(int(n), float(mass)), np.tile(np.asarray(vel, dtype=np.float64), (int(n), 1)))

    # ------------------------------------------------------------------ the operations
    def cell_keys(self) -> torch.Tensor:
        """qk_cic_cell_keys: the base-cell key per particle (int64), the sentinel num_keys for a particle that does not take part"""
        c, n = self.ctx, self.num_particles
        keys = torch.empty(n, dtype=torch.int64, device=c.device)
        c.check(c.L.qk_cic_cell_keys(c.h, c.stream(), self._n, self._plo, self._dx, n, self._ptrs(self.pos), self._p(keys)), "qk_cic_cell_keys")
        return keys

    def deposit(self, poisson, G: float):
        """rhs(c) = (sum W 4 pi G m) / vol for every cell a particle reaches (ParticleToMesh with weight 4 pi G mass, reference
        src/simulation.hpp:1043-1047) into the zeroed right-hand side of `poisson`, before fill_rhs adds the gas"""
        n = self.num_particles
        if n == 0:
            return
        if list(poisson.n) != [int(x) for x in self.geom.n_cell]:
            raise capi.QkError(f"CIC particles: the Poisson solver's lattice {poisson.n} is not the level's {self.geom.n_cell}")
        c = self.ctx
        keys = self.cell_keys()
        sorted_keys, perm = torch.sort(keys, stable=True)
        if self._cells is None:
            self._cells = torch.arange(self.num_keys + 1, dtype=torch.int64, device=c.device)
        offsets = torch.searchsorted(sorted_keys, self._cells).contiguous()
        c.check(c.L.qk_cic_deposit(c.h, c.stream(), self._n, self._plo, self._dx, float(G), n, self._ptrs(self.pos), self._p(self.mass),
                                   self._p(perm), self._p(offsets), C.c_void_p(poisson.rhs.data_ptr())), "qk_cic_deposit")

    def kick(self, phi: torch.Tensor, dt: float):
        """vel += 0.5 dt * (acceleration interpolated from the dense potential) (kickParticlesAllLevels, reference src/simulation.hpp:1107-1193)"""
        n = self.num_particles
        if n == 0:
            return
        g = self.geom.n_cell
        if tuple(phi.shape) != (g[2] + 2, g[1] + 2, g[0] + 2) or phi.dtype != torch.float64 or not phi.is_contiguous():
            raise capi.QkError(f"CIC particles: phi must be the dense ({g[2] + 2}, {g[1] + 2}, {g[0] + 2}) double array of the Poisson solve")
        c = self.ctx
        c.check(c.L.qk_cic_kick(c.h, c.stream(), self._n, self._plo, self._dx, float(dt), C.c_void_p(phi.data_ptr()), n, self._ptrs(self.pos),
                                self._ptrs(self.vel)), "qk_cic_kick")

    def drift(self, dt: float):
        """pos += dt * vel (driftParticlesAllLevels, reference src/simulation.hpp:1195-1216)"""
        n = self.num_particles
        if n == 0:
            return
        c = self.ctx
        c.check(c.L.qk_cic_drift(c.h, c.stream(), float(dt), n, self._ptrs(self.pos), self._ptrs(self.vel)), "qk_cic_drift")

    def redistribute(self) -> int:
        """Redistribute on level 0 (reference src/simulation.hpp:1330-1341): periodic shift, particles beyond a non-periodic face dropped
        (qk_tracer_Where on this level's plan).  Returns the number dropped and adds it to num_dropped."""
        n = self.num_particles
        if n == 0:
            self.last_keep = torch.empty(0, dtype=torch.bool, device=self.ctx.device)
            return 0
        level = torch.zeros(n, dtype=torch.int32, device=self.ctx.device)
        _, keep = where(self.ctx, [self.plan], 0, 0, self.pos, level)
        self.last_keep = keep
        if bool(keep.all()):  # (one device -> host read per step)
            return 0
        self.pos = [a[keep] for a in self.pos]
        self.vel = [a[keep] for a in self.vel]
        self.mass, self.id, self.cpu = self.mass[keep], self.id[keep], self.cpu[keep]
        dropped = n - self.num_particles
        self.num_dropped += dropped
        return dropped

    # ------------------------------------------------------------------ read-out and restore
    def positions(self) -> np.ndarray:
        return torch.stack(self.pos, dim=1).cpu().numpy() if self.num_particles else np.zeros((0, 3))

    def velocities(self) -> np.ndarray:
        return torch.stack(self.vel, dim=1).cpu().numpy() if self.num_particles else np.zeros((0, 3))

    def masses(self) -> np.ndarray:
        return self.mass.cpu().numpy()

    def ids(self) -> np.ndarray:
        return self.id.cpu().numpy()

    def load(self, positions, velocities, masses, ids):
        """take over the particles of a saved run: positions / velocities (np, 3), masses and ids (np,); cpu = this rank"""
        p, v = np.asarray(positions, dtype=np.float64), np.asarray(velocities, dtype=np.float64)
        m, i = np.asarray(masses, dtype=np.float64), np.asarray(ids, dtype=np.int64)
        if p.ndim != 2 or p.shape[1] != 3 or v.shape != p.shape or m.shape != (p.shape[0],) or i.shape != (p.shape[0],):
            raise capi.QkError("CICParticles.load: expected positions and velocities of shape (np, 3) and masses and ids of shape (np,)")
        dev = self.ctx.device
        self.pos = [torch.from_numpy(np.ascontiguousarray(p[:, d])).to(dev) for d in range(3)]
        self.vel = [torch.from_numpy(np.ascontiguousarray(v[:, d])).to(dev) for d in range(3)]
        self.mass = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        self.id = torch.from_numpy(np.ascontiguousarray(i)).to(dev)
        self.cpu = torch.full((p.shape[0],), int(self.sim.rank), dtype=torch.int32, device=dev)
        self._next_id = int(i.max()) + 1 if i.size else 1
