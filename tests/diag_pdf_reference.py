"""numpy restatement of the DiagPDF histograms (csrc/qk_diag.hip, quokka_amd/diagnostics.py): the fine-covered mask, the filters, the bin
of a cell, its weight, and the sum of every bin in the fixed order §15 writes, so that the kernels can be compared bit for bit.  No GPU, numpy only.

A level is a dict  {"boxes": [(lo, hi), ...], "dx": (dx0, dx1, dx2), "fields": {name: [array per box, shape (nz, ny, nx)]}}  — valid cells only.
A histogram is a dict  {"vars": [(name, nbins, log_spaced, low, high), ...], "filters": [(name, low, high), ...], "weight_by": str, "ndim": int}."""
from __future__ import annotations

import math

import numpy as np

BLOCK = 256
DBL_MAX = float(np.finfo(np.float64).max)


# ---------------------------------------------------------------------- the sum
def tree_sum(weights) -> float:
    """S(list): empty -> +0.0; else blocks of 256 from the start, the last padded with +0.0, each reduced by v[t] = v[t] + v[t + s] (t < s,
    s = 128 .. 1); the block results, in order, are the new list; repeated until one value is left"""
    v = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if v.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            nb = (v.size + BLOCK - 1) // BLOCK
            pad = np.zeros(nb * BLOCK, dtype=np.float64)
            pad[:v.size] = v
            blk = pad.reshape(nb, BLOCK)
            s = BLOCK // 2
            while s >= 1:
                blk[:, :s] = blk[:, :s] + blk[:, s:2 * s]
                s //= 2
            v = blk[:, 0].copy()
            if v.size == 1:
                return float(v[0])


def num_passes(count: int) -> int:
    p, c = 1, (count + BLOCK - 1) // BLOCK
    while c > 1:
        p, c = p + 1, (c + BLOCK - 1) // BLOCK
    return p


# ---------------------------------------------------------------------- bins
def axis_transform(nbins: int, log_spaced: int, low: float, high: float):
    """(lowT, widthT): the range difference first, then one division by (double)nbins (reference src/io/DiagPDF.cpp:136-138)"""
    if log_spaced:
        rng = math.log10(high) - math.log10(low)
        return math.log10(low), rng / float(nbins)
    return low, (high - low) / float(nbins)


def bin_coordinate(x, nbins: int, log_spaced: int, low: float, high: float):
    lowT, widthT = axis_transform(nbins, log_spaced, low, high)
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        val = np.log10(x) if log_spaced else x
        return (val - lowT) / widthT


def bin_of(q, nbins: int):
    """(in range, bin): in range iff q >= 0.0 and q < nbins, decided on the double; bin = floor(q) where in range, else 0"""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (q >= 0.0) & (q < float(nbins))
        b = np.where(ok, np.floor(np.where(ok, q, 0.0)), 0.0).astype(np.int64)
    return ok, b


def total_bins(hist) -> int:
    t = 1
    for _, nbins, _, _, _ in hist["vars"]:
        t *= int(nbins)
    return t


# ---------------------------------------------------------------------- which cells
def box_shape(lo, hi):
    return (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)


def fine_mask(boxes, finer_boxes):
    """makeFineMask at ratio 2: per box an int array of 1, 0 where a box of the next level (coarsened by 2) covers the cell; finer_boxes None: all 1"""
    out = []
    for lo, hi in boxes:
        m = np.ones(box_shape(lo, hi), dtype=np.int32)
        for flo, fhi in (finer_boxes or []):
            clo, chi = [x // 2 for x in flo], [x // 2 for x in fhi]
            a = [max(clo[d], lo[d]) for d in range(3)]
            b = [min(chi[d], hi[d]) for d in range(3)]
            if all(a[d] <= b[d] for d in range(3)):
                m[a[2] - lo[2]:b[2] - lo[2] + 1, a[1] - lo[1]:b[1] - lo[1] + 1, a[0] - lo[0]:b[0] - lo[0] + 1] = 0
        out.append(m)
    return out


def weight_factor(hist, dx) -> float:
    if hist["weight_by"] in ("volume", "mass"):
        nd = hist["ndim"]
        return dx[0] if nd == 1 else ((dx[0] * dx[1]) if nd == 2 else ((dx[0] * dx[1]) * dx[2]))
    if hist["weight_by"] == "cell_counts":
        return 1.0
    raise ValueError("Invalid histogram weight type! Must be either 'volume', 'mass' or 'cell_counts'.")


def field_range(levels, name):
    """min and max over all valid cells of all levels, fine-covered cells included"""
    lo = min(float(a.min()) for L in levels for a in L["fields"][name])
    hi = max(float(a.max()) for L in levels for a in L["fields"][name])
    return lo, hi


def resolve_ranges(hist, levels):
    """the histogram with every absent range (low None) taken from the field"""
    out = dict(hist)
    out["vars"] = []
    for name, nbins, log_spaced, low, high in hist["vars"]:
        if low is None:
            low, high = field_range(levels, name)
        out["vars"].append((name, nbins, log_spaced, low, high))
    return out


def level_keys_weights(hist, level, finer_boxes):
    """(keys, weights) of the level in enumeration order: box ascending, within a box k outermost and i fastest; the sentinel total_bins for a cell that
    takes no part"""
    tb = total_bins(hist)
    masks = fine_mask(level["boxes"], finer_boxes)
    wf = weight_factor(hist, level["dx"])
    keys, weights = [], []
    for b in range(len(level["boxes"])):
        part = masks[b] != 0
        for name, low, high in hist.get("filters", []):
            f = level["fields"][name][b]
            with np.errstate(invalid="ignore"):
                part = part & ~((f < low) | (f > high))
        cbin = np.zeros(part.shape, dtype=np.int64)
        for name, nbins, log_spaced, low, high in hist["vars"]:
            ok, bn = bin_of(bin_coordinate(level["fields"][name][b], nbins, log_spaced, low, high), nbins)
            part = part & ok
            cbin = cbin * int(nbins) + bn
        w = np.full(part.shape, wf, dtype=np.float64)
        if hist["weight_by"] == "mass":
            w = w * level["fields"]["gasDensity"][b]
        keys.append(np.where(part, cbin, tb).reshape(-1))
        weights.append(w.reshape(-1))
    return np.concatenate(keys), np.concatenate(weights)


def level_sums(keys, weights, tb: int):
    """S of every bin: the bin's weights in enumeration order"""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    off = np.searchsorted(sk, np.arange(tb + 1))
    out = np.zeros(tb, dtype=np.float64)
    for b in np.nonzero(off[1:] > off[:-1])[0]:
        out[b] = tree_sum(weights[order[off[b]:off[b + 1]]])
    return out


def pdf(hist, levels):
    """pdf[b] = (((0.0 + S_0[b]) + S_1[b]) + ...) over the levels ascending; ranges that are absent are taken from the fields first"""
    hist = resolve_ranges(hist, levels)
    tb = total_bins(hist)
    out = np.zeros(tb, dtype=np.float64)
    for l, L in enumerate(levels):
        finer = levels[l + 1]["boxes"] if l + 1 < len(levels) else None
        k, w = level_keys_weights(hist, L, finer)
        with np.errstate(invalid="ignore", over="ignore"):
            out = out + level_sums(k, w, tb)
    return out
