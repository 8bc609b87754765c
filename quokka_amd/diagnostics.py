"""In-situ diagnostics: the DiagPDF histograms of the reference (src/io/DiagPDF.cpp with DiagBase.cpp and DiagFilter.cpp; created and driven as in
src/simulation.hpp:2120-2205).  DESIGN.md §15 defines the one thing the reference leaves open, the order of the sum.

Host plumbing only: deck keys, the intersection list of the fine-covered mask, and between the key kernel and the segment sum a stable sort of the keys
(torch.sort), the range of every bin (torch.searchsorted) and the block table of every pass (integer torch operations).  Every cell and every weight is
touched by the HIP kernels of csrc/qk_diag.hip; the levels' sums are added in order.  DiagFramePlane, projections and statistics are not built.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi
from .multifab import MultiFab
from .plotfile import component_names

BLOCK = 256
MAX_TOTAL_BINS = 1 << 24
DBL_MAX = float(np.finfo(np.float64).max)
WEIGHT_TYPES = ("volume", "mass", "cell_counts")
INVALID_WEIGHT = "Invalid histogram weight type! Must be either 'volume', 'mass' or 'cell_counts'."


# ---------------------------------------------------------------------- deck keys
def parse_deck(path: str) -> Dict[str, List[str]]:
    """the `quokka.*` keys of an inputs file: key -> list of words.  `#` starts a comment, a trailing `\\` continues the line, quotes around a
    word are dropped; a key given twice keeps its last value (as amrex::ParmParse's query does)"""
    with open(path) as f:
        raw = f.read().split("\n")
    lines, cur = [], ""
    for ln in raw:
        ln = ln.split("#", 1)[0].rstrip()
        if ln.endswith("\\"):
            cur += ln[:-1] + " "
            continue
        lines.append(cur + ln)
        cur = ""
    if cur:
        lines.append(cur)
    out: Dict[str, List[str]] = {}
    for ln in lines:
        if "=" not in ln:
            continue
        key, val = ln.split("=", 1)
        key = key.strip()
        if key.startswith("quokka."):
            out[key] = [w.strip("\"'") for w in val.split()]
    return out


def _words(params, key: str) -> Optional[List[str]]:
    """the value of a key as a list of words (a str is split, a number or a list of them is converted); None if the key is absent"""
    if key not in params:
        return None
    v = params[key]
    if isinstance(v, str):
        return v.split()
    if isinstance(v, (list, tuple)):
        return [w if isinstance(w, str) else repr(float(w)) if isinstance(w, float) else str(w) for w in v]
    return [repr(float(v)) if isinstance(v, float) else str(v)]


def _one(params, key: str, conv, default=None):
    w = _words(params, key)
    if not w:
        return default
    try:
        return conv(w[0])
    except ValueError:
        raise capi.QkError(f"[Diagnostics] {key} = {w[0]}: not a value of the expected kind")


def _int(s: str) -> int:
    return int(float(s)) if any(c in s for c in ".eE") else int(s)


def _pair(params, key: str) -> Optional[Tuple[float, float]]:
    w = _words(params, key)
    if not w:
        return None
    if len(w) < 2:
        raise capi.QkError(f"[Diagnostics] {key} needs two numbers")
    try:
        a, b = float(w[0]), float(w[1])
    except ValueError:
        raise capi.QkError(f"[Diagnostics] {key} = {w[0]} {w[1]}: not two numbers")
    return min(a, b), max(a, b)


# ---------------------------------------------------------------------- DiagFilter / DiagBase / DiagPDF
class DiagFilter:
    """reference src/io/DiagFilter.cpp: a cell is removed iff value < low || value > high"""

    def __init__(self, prefix: str, params):
        self.prefix = prefix
        self.field_name = _one(params, prefix + ".field_name", str, "")
        if not self.field_name:
            raise capi.QkError(f"filter: {prefix} is missing a field_name !")
        if _words(params, prefix + ".value_greater"):
            self.low, self.high = _one(params, prefix + ".value_greater", float), DBL_MAX
        elif _words(params, prefix + ".value_less"):
            self.low, self.high = -DBL_MAX, _one(params, prefix + ".value_less", float)
        elif _words(params, prefix + ".value_inrange"):
            self.low, self.high = _pair(params, prefix + ".value_inrange")
        else:
            raise capi.QkError(f"filter: {prefix} is missing a range definition !")


class DiagVar:
    def __init__(self, name: str, nbins: int, log_spaced: int, rng: Optional[Tuple[float, float]]):
        self.name, self.nbins, self.log_spaced = name, nbins, log_spaced
        self.use_field_minmax = rng is None
        self.low, self.high = rng if rng is not None else (0.0, 0.0)

    def transform(self) -> Tuple[float, float]:
        """(lowT, widthT): the range difference first, then one division by (double)nBins (reference src/io/DiagPDF.cpp:136-138)"""
        if self.log_spaced:
            rng = math.log10(self.high) - math.log10(self.low)
            return math.log10(self.low), rng / float(self.nbins)
        return self.low, (self.high - self.low) / float(self.nbins)


class DiagPDF:
    """reference src/io/DiagPDF.cpp (init, addVars, processDiag, writePDFToFile) on src/io/DiagBase.cpp (init, doDiag)"""

    def __init__(self, prefix: str, name: str, params):
        self.prefix, self.name = prefix, name
        # DiagBase::init
        self.interval = _one(params, prefix + ".int", _int, -1)
        self.per = _one(params, prefix + ".per", float, -1.0)
        self.diagfile = _one(params, prefix + ".file", str, name)
        if not (self.interval > 0 or self.per > 0.0):
            raise capi.QkError(f"[Diagnostics] {prefix}: one of {prefix}.int and {prefix}.per must be > 0")
        self.filters = [DiagFilter(prefix + "." + f, params) for f in (_words(params, prefix + ".filters") or [])]
        if len(self.filters) > capi.DIAG_MAX_FILTERS:
            raise capi.QkError(f"[Diagnostics] {prefix}: more than {capi.DIAG_MAX_FILTERS} filters are not built")
        # DiagPDF::init
        self.weight_type = _one(params, prefix + ".weight_by", str, "volume")
        if self.weight_type not in WEIGHT_TYPES:
            raise capi.QkError(f"[Diagnostics] {prefix}.weight_by = {self.weight_type}: {INVALID_WEIGHT}")
        names = _words(params, prefix + ".var_names") or []
        if not 1 <= len(names) <= capi.DIAG_MAX_VARS:
            raise capi.QkError(f"[Diagnostics] {prefix}.var_names must name 1 .. {capi.DIAG_MAX_VARS} variables, not {len(names)}")
        self.vars: List[DiagVar] = []
        for v in names:
            vp = prefix + "." + v
            nbins = _one(params, vp + ".nBins", _int)
            if nbins is None:
                raise capi.QkError(f"[Diagnostics] {vp}.nBins is missing")
            if nbins <= 0:
                raise capi.QkError(f"[Diagnostics] {vp}.nBins = {nbins} must be > 0")
            log_spaced = 1 if _one(params, vp + ".log_spaced_bins", _int, 0) != 0 else 0
            rng = _pair(params, vp + ".range")
            if rng is not None:
                if not (math.isfinite(rng[0]) and math.isfinite(rng[1])):
                    raise capi.QkError(f"[Diagnostics] {vp}.range = {rng[0]} {rng[1]} is not finite")
                if log_spaced and not (rng[0] > 0 and rng[1] > 0):
                    raise capi.QkError(f"[Diagnostics] {vp}: For log-spaced bins, histogram bounds must be positive!")
            self.vars.append(DiagVar(v, nbins, log_spaced, rng))
        self.total_bins = 1
        for v in self.vars:
            self.total_bins *= v.nbins
        if self.total_bins > MAX_TOTAL_BINS:
            raise capi.QkError(f"[Diagnostics] {prefix}: {self.total_bins} bins in all; more than 2^24 are not built")
        self.last_pdf: Optional[np.ndarray] = None
        self.last_path: Optional[str] = None

    def addVars(self, var_list: List[str]):
        for f in self.filters:
            var_list.append(f.field_name)
        if self.weight_type == "mass":
            var_list.append("gasDensity")
        for v in self.vars:
            var_list.append(v.name)

    def var_list(self) -> List[str]:
        out: List[str] = []
        self.addVars(out)
        return sorted(set(out))

    def doDiag(self, time: float, nstep: int) -> bool:
        """reference src/io/DiagBase.cpp:47-58: `per` is parsed and never triggers"""
        return self.interval > 0 and nstep % self.interval == 0

    # ------------------------------------------------------------------ the histogram
    def process(self, sim, fields=None) -> np.ndarray:
        """the histogram of the simulation's state as it stands (processDiag without the file): numpy, length total_bins"""
        levels = _levels_of(sim)
        if fields is None:
            fields = compute_fields(sim, levels, self.var_list())
        ctx = levels[0].ctx
        for v in self.vars:
            if v.use_field_minmax:
                lo, hi = DBL_MAX, -DBL_MAX
                for l, L in enumerate(levels):
                    mf, comp = fields[v.name][l]
                    try:
                        a, b = _minmax(L, mf, comp)
                    except capi.QkError as e:
                        raise capi.QkError(f"[Diagnostics] {self.prefix}: the range of field {v.name} is not finite ({e})")
                    lo, hi = min(lo, a), max(hi, b)
                v.low, v.high = lo, hi
            if v.log_spaced and not (v.low > 0 and v.high > 0):
                raise capi.QkError(f"[Diagnostics] {self.prefix}.{v.name}: For log-spaced bins, histogram bounds must be positive! "
                                   f"(range {v.low} .. {v.high})")
        tb = self.total_bins
        dev = ctx.device
        bins = torch.arange(tb + 1, dtype=torch.int64, device=dev)
        pdf = torch.zeros(tb, dtype=torch.float64, device=dev)
        for l, L in enumerate(levels):
            finer = levels[l + 1].all_boxes if l + 1 < len(levels) else None
            keys, weights = self.level_keys_weights(L, [fields[n][l] for n in self._field_order()], finer)
            sorted_keys, perm = torch.sort(keys, stable=True)
            offsets = torch.searchsorted(sorted_keys, bins)
            pdf = pdf + bin_sums(*segment_sums(ctx, weights, perm, offsets, tb))  # (((0.0 + S_0) + S_1) + ...
        return pdf.cpu().numpy()

    def _field_order(self) -> List[str]:
        return [f.field_name for f in self.filters] + [v.name for v in self.vars] + (["gasDensity"] if self.weight_type == "mass" else [])

    def weight_factor(self, L) -> float:
        if self.weight_type == "cell_counts":
            return 1.0
        dx, nd = L.geom.dx, L.geom.ndim
        return dx[0] if nd == 1 else ((dx[0] * dx[1]) if nd == 2 else ((dx[0] * dx[1]) * dx[2]))

    def level_mask(self, L, finer_boxes) -> Optional[MultiFab]:
        """makeFineMask at ratio 2 (None on the finest level): 1, and 0 where a box of the next level covers the cell"""
        if finer_boxes is None:
            return None
        ctx = L.ctx
        mask = MultiFab(L.lev, 1, 0, dtype=torch.int32)
        items, biggest = [], 0
        for flo, fhi in finer_boxes:
            clo, chi = [x // 2 for x in flo], [x // 2 for x in fhi]
            for b, (lo, hi) in enumerate(L.lev.boxes):
                a = [max(clo[d], lo[d]) for d in range(3)]
                z = [min(chi[d], hi[d]) for d in range(3)]
                if all(a[d] <= z[d] for d in range(3)):
                    items.append([b] + a + z)
                    biggest = max(biggest, (z[0] - a[0] + 1) * (z[1] - a[1] + 1) * (z[2] - a[2] + 1))
        it = torch.tensor(items, dtype=torch.int32, device=ctx.device).reshape(-1) if items else None
        ctx.check(ctx.L.qk_diag_mask(L.lev.h, ctx.stream(), mask.ptr, len(items), C.c_void_p(it.data_ptr()) if items else None, biggest), "qk_diag_mask")
        return mask

    def level_keys_weights(self, L, field_list, finer_boxes) -> Tuple[torch.Tensor, torch.Tensor]:
        """(keys, weights) of level L in enumeration order (qk_diag_keys); field_list: (MultiFab, comp) per name of _field_order()"""
        ctx = L.ctx
        sizes = [(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1) for lo, hi in L.lev.boxes]
        ncells = sum(sizes)
        box_offset = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), dtype=torch.int64, device=ctx.device)
        mask = self.level_mask(L, finer_boxes)
        a = capi.DiagPdf()
        a.nvars, a.nfilters = len(self.vars), len(self.filters)
        it = iter(field_list)
        for n, f in enumerate(self.filters):
            mf, comp = next(it)
            a.filters[n].table, a.filters[n].comp, a.filters[n].low, a.filters[n].high = mf.ptr, comp, f.low, f.high
        for n, v in enumerate(self.vars):
            mf, comp = next(it)
            low_t, width_t = v.transform()
            a.vars[n].table, a.vars[n].comp, a.vars[n].nbins, a.vars[n].log_spaced = mf.ptr, comp, v.nbins, v.log_spaced
            a.vars[n].low_t, a.vars[n].width_t = low_t, width_t
        a.weight_fac = self.weight_factor(L)
        if self.weight_type == "mass":
            mf, comp = next(it)
            a.density, a.density_comp = mf.ptr, comp
        keys = torch.empty(ncells, dtype=torch.int64, device=ctx.device)
        weights = torch.empty(ncells, dtype=torch.float64, device=ctx.device)
        ctx.check(ctx.L.qk_diag_keys(L.lev.h, ctx.stream(), C.byref(a), mask.ptr if mask is not None else None, C.c_void_p(box_offset.data_ptr()), ncells,
                                     C.c_void_p(keys.data_ptr()), C.c_void_p(weights.data_ptr())), "qk_diag_keys")
        return keys, weights

    # ------------------------------------------------------------------ the file
    def file_name(self, nstep: int, time: float) -> str:
        name = ""
        if self.interval > 0:
            name = self.diagfile + "%06d" % nstep  # amrex::Concatenate(m_diagfile, a_nstep, 6)
        if self.per > 0.0:
            name = self.diagfile + "%f" % time     # std::to_string(a_time)
        return name + ".dat"

    def write(self, nstep: int, time: float, pdf: np.ndarray) -> str:
        path = self.file_name(nstep, time)
        with open(path, "w") as f:
            f.write(self.format(nstep, time, pdf))
        return path

    def format(self, nstep: int, time: float, pdf: Sequence[float]) -> str:
        """writePDFToFile (reference src/io/DiagPDF.cpp:275-379), character for character"""
        width = 25
        widths = [max(width, len(v.name) + 5) for v in self.vars]
        out = ["# " + "%*s" % (width, "time:") + " " + "%*.17e" % (width, time) + "\n",
               "# " + "%*s" % (width, "cycle:") + " " + "%*d" % (width, nstep) + "\n",
               "# " + "%*s" % (width, "variables:") + "".join(" " + "%*s" % (width, v.name) for v in self.vars) + "\n",
               "# " + "%*s" % (width, "is_log_spaced:") + "".join(" " + "%*d" % (width, v.log_spaced) for v in self.vars) + "\n",
               "".join("%*s" % (w, v.name + "_idx") + " " + "%*s" % (w, v.name + "_min") + " " + "%*s" % (w, v.name + "_max")
                       for v, w in zip(self.vars, widths)) + " " + "%*s" % (width, self.weight_type + "_sum") + "\n"]
        tr = [v.transform() for v in self.vars]
        for linidx in range(len(pdf)):
            idx, cbin = [0] * len(self.vars), linidx
            for n in range(len(self.vars) - 1, -1, -1):
                idx[n] = cbin % self.vars[n].nbins
                cbin = (cbin - idx[n]) // self.vars[n].nbins
            row = []
            for n, (v, w) in enumerate(zip(self.vars, widths)):
                left = tr[n][0] + float(idx[n]) * tr[n][1]
                right = left + tr[n][1]
                if v.log_spaced:
                    left, right = _pow10(left), _pow10(right)
                row.append("%*d" % (width, idx[n]) + " " + "%*.17e" % (w, left) + " " + "%*.17e" % (w, right) + " ")
            out.append("".join(row) + "%*.17e" % (width, float(pdf[linidx])) + "\n")
        return "".join(out)


def _pow10(x: float) -> float:
    try:
        return math.pow(10.0, x)
    except OverflowError:
        return math.inf


def read_pdf_file(path: str):
    """(header dict, rows): the four `# key: values` lines and the numeric rows of a file written by DiagPDF.write (the last column is the histogram)"""
    with open(path) as f:
        lines = f.read().split("\n")
    header = {}
    for ln in lines[:4]:
        key, _, val = ln[1:].partition(":")
        header[key.strip()] = val.split()
    header["columns"] = lines[4].split()
    rows = [[float(w) for w in ln.split()] for ln in lines[5:] if ln.strip()]
    return header, np.array(rows, dtype=np.float64)


# ---------------------------------------------------------------------- the segment sum
def num_passes(count: int) -> int:
    p, c = 1, (count + BLOCK - 1) // BLOCK
    while c > 1:
        p, c = p + 1, (c + BLOCK - 1) // BLOCK
    return p


def segment_sums(ctx, weights: torch.Tensor, perm: Optional[torch.Tensor], offsets: torch.Tensor, nbins: int):
    """S of every bin: bin b's weights are weights[perm[offsets[b] .. offsets[b + 1])] (perm None: weights[...]).  Returns (part, off):
    bin b's sum is part[off[b]] where off[b + 1] > off[b], and +0.0 where the bin is empty.  The block table of every pass is built on the device;
    the upper bound ceil(n / 256) + nbins of blocks is launched and the empty ones exit, so the host reads nothing."""
    dev = ctx.device
    n = int(perm.numel()) if perm is not None else int(weights.numel())
    src, off = weights, offsets
    for p in range(num_passes(max(n, 1))):
        count = off[1:] - off[:-1]
        nblk = (count + (BLOCK - 1)) // BLOCK
        cum = torch.cumsum(nblk, 0)
        nlaunch = (n + BLOCK - 1) // BLOCK + nbins
        m = torch.arange(nlaunch, dtype=torch.int64, device=dev)
        b = torch.searchsorted(cum, m, right=True)
        bc = torch.clamp(b, max=nbins - 1)
        start = off[bc] + (m - (cum[bc] - nblk[bc])) * BLOCK
        length = torch.where(b < nbins, torch.clamp(off[bc + 1] - start, min=0, max=BLOCK), torch.zeros_like(m))
        dst = torch.empty(nlaunch, dtype=torch.float64, device=dev)
        ctx.check(ctx.L.qk_diag_segsum(ctx.h, ctx.stream(), nlaunch, C.c_void_p(start.data_ptr()), C.c_void_p(length.data_ptr()),
                                       C.c_void_p(src.data_ptr()), int(src.numel()), C.c_void_p(perm.data_ptr()) if perm is not None else None,
                                       int(perm.numel()) if perm is not None else 0, 1 if p > 0 else 0, C.c_void_p(dst.data_ptr())), "qk_diag_segsum")
        src, perm, n = dst, None, nlaunch
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), cum])
    return src, off


def bin_sums(part: torch.Tensor, off: torch.Tensor) -> torch.Tensor:
    """S of every bin from what segment_sums returns: part[off[b]], and +0.0 for an empty bin"""
    zero = torch.zeros((), dtype=torch.float64, device=part.device)
    return torch.where(off[1:] > off[:-1], part[torch.clamp(off[:-1], max=part.numel() - 1)], zero)


def _minmax(L, mf: MultiFab, comp: int) -> Tuple[float, float]:
    ctx = L.ctx
    nbytes = int(ctx.L.qk_diag_minmax_scratch_bytes(L.lev.h))
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=ctx.device)
    out = (C.c_double * 2)()
    ctx.check(ctx.L.qk_diag_minmax(L.lev.h, ctx.stream(), mf.ptr, int(comp), C.c_void_p(scratch.data_ptr()), nbytes, out), "qk_diag_minmax")
    return float(out[0]), float(out[1])


# ---------------------------------------------------------------------- the simulation's side (reference src/simulation.hpp:2120-2205)
def _levels_of(sim):
    return list(sim.levels) if hasattr(sim, "levels") else [sim]


def _ncomp_cc(sim) -> int:
    if hasattr(sim, "levels"):
        if getattr(sim, "rad_traits", None) is not None:
            raise capi.QkError("[Diagnostics] diagnostics on an AmrSimulation are built for hydro levels, not for levels with radiation")
        return 6
    return int(sim.ncomp_cc)


def available_names(sim) -> List[str]:
    return component_names(_ncomp_cc(sim)) + [str(n) for n in getattr(sim, "derivedNames_", [])]


def build_diagnostics(params, names: Sequence[str]) -> Tuple[List[DiagPDF], List[str]]:
    """createDiagnostics without a simulation: (m_diagnostics, m_diagVars) from the deck keys; names: the fields that exist"""
    diags: List[DiagPDF] = []
    diag_vars: List[str] = []
    for name in (_words(params, "quokka.diagnostics") or []):
        prefix = "quokka." + name
        kind = _one(params, prefix + ".type", str)
        if kind is None:
            raise capi.QkError(f"[Diagnostics] {prefix}.type is missing")
        if kind != "DiagPDF":
            raise capi.QkError(f"[Diagnostics] {prefix}.type = {kind} is not built (only DiagPDF is; DiagFramePlane, projections and statistics "
                               "are out of scope)")
        d = DiagPDF(prefix, name, params)
        d.addVars(diag_vars)
        diags.append(d)
    diag_vars = sorted(set(diag_vars))
    for v in diag_vars:
        if v not in names:
            raise capi.QkError(f"[Diagnostics] Field {v} is not available!")
    return diags, diag_vars


def create_diagnostics(sim, params):
    if int(getattr(sim, "nranks", 1)) > 1:
        raise capi.QkError("[Diagnostics] diagnostics are built for one rank (nranks > 1: the ranks' histograms would need a fixed order of their own)")
    sim.m_diagnostics, sim.m_diagVars = build_diagnostics(params, available_names(sim))


def compute_fields(sim, levels, names: Sequence[str]) -> Dict[str, List[Tuple[MultiFab, int]]]:
    """name -> per level (MultiFab, component): a state component is read in place from state_new_cc_; a derived variable is computed into a
    one-component MultiFab without ghost cells by sim.ComputeDerivedVar(level_sim, name, out)"""
    state_names = component_names(_ncomp_cc(sim))
    out: Dict[str, List[Tuple[MultiFab, int]]] = {}
    for name in names:
        if name in state_names:
            out[name] = [(L.state_new_cc_, state_names.index(name)) for L in levels]
        elif name in getattr(sim, "derivedNames_", []):
            fn = getattr(sim, "ComputeDerivedVar", None)
            if fn is None:
                raise capi.QkError(f"[Diagnostics] Field {name} is a derived variable and the simulation has no ComputeDerivedVar")
            per_level = []
            for L in levels:
                mf = MultiFab(L.lev, 1, 0, fill=0.0)
                fn(L, name, mf)
                per_level.append((mf, 0))
            out[name] = per_level
        else:
            raise capi.QkError(f"[Diagnostics] Field {name} is not available!")
    return out


def do_diagnostics(sim) -> List[Tuple[str, np.ndarray]]:
    """every diagnostic whose doDiag(tNew, istep) holds is processed and written: the list of (path, pdf)"""
    diags = getattr(sim, "m_diagnostics", None)
    if not diags:
        return []
    istep = sim.istep[0] if isinstance(sim.istep, (list, tuple)) else sim.istep
    time = float(sim.tNew_)
    due = [d for d in diags if d.doDiag(time, istep)]
    if not due:
        return []
    if int(getattr(sim, "nranks", 1)) > 1:
        raise capi.QkError("[Diagnostics] diagnostics are built for one rank (nranks > 1)")
    fields = compute_fields(sim, _levels_of(sim), sim.m_diagVars)
    out = []
    for d in due:
        pdf = d.process(sim, fields)
        d.last_pdf, d.last_path = pdf, d.write(istep, time, pdf)
        out.append((d.last_path, pdf))
    return out
