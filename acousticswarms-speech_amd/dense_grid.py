"""Dense TDoA-lattice candidate enumeration (BASELINE.json config 5: "16-mic array, dense
TDoA grid, SRP-PHAT bypassed").

With the pruning stage bypassed every hypercube of the integer TDoA lattice that some point
of the region of interest falls into is a candidate.  The cubes follow the conventions of the
search stages: offsets are relative to microphone 0 in samples (``pair_offsets``,
sep/helpers/local_utils_3d.py:221-225), a cube of width w is centred on a multiple of w in
every pair dimension and owns the grid points whose TDoA rounds to it (the membership test
of ``Patch.hyperbola_sample``, sep/Traditional_SP/Patch_3D.py:40-47, without its 1e-3 slack,
so every point belongs to exactly one cube).  The reference has no function for this
configuration; it only defines the stress workload, so there is no fixture to pin and the
enumeration is checked by its own invariants (tests/test_search_host.py).
"""
import collections

import numpy as np

from .patch import Patch, pair_offsets


def roi_grid(roi, step):
    """[3,n] float64 grid points of the ROI [x0,x1,y0,y1,z0,z1] at ``step`` metres."""
    ax = [np.arange(roi[2 * k], roi[2 * k + 1] + 1e-9, step) for k in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()])


def dense_tdoa_candidates(mic_positions, roi, width=2, step=0.02, chunk=1 << 20, with_points=True):
    """All non-empty width-``width`` TDoA cubes of the ROI.

    Returns (offsets int64 [N, M-1] sorted lexicographically, counts [N], patches) where
    ``patches`` is a list of ``Patch`` (sample_offset, width_list = width, area_points = the
    grid points inside) or None when ``with_points`` is False (tens of thousands of candidates:
    the scorer only needs the offsets)."""
    mic = np.asarray(mic_positions, dtype=np.float64)
    P = mic.shape[0] - 1
    pts = roi_grid(roi, step)
    n = pts.shape[1]
    cells = np.empty((n, P), dtype=np.int64)
    for lo in range(0, n, chunk):                            # bounded temporaries: chunk x P float64
        hi = min(n, lo + chunk)
        cells[lo:hi] = np.rint(pair_offsets(pts[:, lo:hi], mic) / width).astype(np.int64).T
    key = np.ascontiguousarray(cells).view([("", np.int64)] * P).ravel()
    order = np.argsort(key, kind="stable")
    sk = key[order]
    first = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    counts = np.diff(np.concatenate([first, [n]]))
    offsets = cells[order[first]] * width
    patches = None
    if with_points:
        patches = []
        for k, (a, c) in enumerate(zip(first, counts)):
            patches.append(Patch(offsets[k].astype(np.float64), np.full(P, float(width)), pts[:, order[a:a + c]]))
    return offsets, counts, patches


# ---- the coarse lattice of an array: stage 1 without a pruner (Prone_method="DENSE") ---------------------------
class Lattice(collections.namedtuple("Lattice", "cells bounds members centres")):
    """``cells`` int32 [N,P], ``bounds`` int32 [N+1], ``members`` int32 [n_kept], ``centres`` float64 [N,3] of
    ``coarse_lattice``; ``width`` is the cube width the cells were taken at."""

    def __new__(cls, cells, bounds, members, centres, width):
        self = super().__new__(cls, cells, bounds, members, centres)
        self.width = width
        return self

    @property
    def n_cubes(self):
        return int(self.cells.shape[0])


def lookup_axes(node):
    """(xs, ys, zs) of the 1 cm lookup grid of an ``SRPPhat`` node, host- or device-built."""
    pos = node.Pos_1
    if hasattr(pos, "xx"):
        return pos.xx, pos.yy, pos.zz
    return pos[0, :, 0, 0], pos[:, 0, 0, 1], pos[0, 0, :, 2]


def lattice_keep_mask(node):
    """bool [ny*nx*nz]: lookup points outside the keep-out rectangle around the array -- the comparisons of
    ``SRPPhat._valid_mask`` on the lookup grid's own axes."""
    xs, ys, zs = lookup_axes(node)
    b = node.array_border
    inside = ((xs[None, :] > b[0]) & (xs[None, :] < b[2]) & (ys[:, None] > b[1]) & (ys[:, None] < b[3]))
    return np.broadcast_to(~inside[:, :, None], (len(ys), len(xs), len(zs))).reshape(-1)


def coarse_lattice(node, width=8):
    """Every non-empty width-``width`` TDoA cube of the 1 cm lookup grid of ``node`` (an ``SRPPhat``): the stage-1
    candidate list of a search with the pruner taken out.

    Points: ``Pos_1`` / ``_planes_1`` [P,ny,nx,nz], point index i = (iy*nx + ix)*nz + iz, without the points whose x
    lies strictly inside (array_border[0], array_border[2]) and whose y strictly inside (array_border[1],
    array_border[3]).  The cell of point i on pair p is rint(planes[p][i] / width) (IEEE divide, round half to
    even); a cube is a distinct cell vector.  Cubes are ordered lexicographically (pair 0 most significant, signed),
    the members of a cube in ascending i, and a centre is the sequential float64 sum of the member positions in
    that order divided by their number.  csrc/geometry_kernels.hip (``asw_geom_lattice``) builds the same tables on
    the GPU, bit for bit; this is their statement."""
    planes = node._planes_1
    P = planes.shape[0]
    flat = planes.reshape(P, -1)
    kept = np.flatnonzero(lattice_keep_mask(node))
    cells = np.empty((kept.shape[0], P), dtype=np.int32)
    for p in range(P):                                       # bounded temporaries: one plane at a time
        cells[:, p] = np.rint(flat[p, kept] / width)
    if kept.shape[0] == 0:
        return Lattice(np.zeros((0, P), np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 3)), width)
    order = np.lexsort(cells.T[::-1])                        # stable; the last key given is the most significant
    sc = cells[order]
    first = np.flatnonzero(np.concatenate([[True], np.any(sc[1:] != sc[:-1], axis=1)]))
    bounds = np.concatenate([first, [kept.shape[0]]]).astype(np.int32)
    members = kept[order].astype(np.int32)
    pos = node.Pos_1.reshape(-1, 3)[members]
    centres = np.empty((first.shape[0], 3))
    for g in range(first.shape[0]):
        a, b = bounds[g], bounds[g + 1]
        centres[g] = np.cumsum(pos[a:b], axis=0)[-1] / float(b - a)      # one member after the other
    return Lattice(np.ascontiguousarray(sc[first]), bounds, members, centres, width)


def lattice_patches(node, lattice):
    """The lattice as the patch list of stage 1: one fresh ``Patch`` per cube (``check_out`` mutates its offsets and
    widths) holding the cube's 1 cm points, with the cube's centre as ``peak_pos`` -- the fine stage builds its
    centre candidate from it."""
    cells, bounds, members, centres = lattice
    width = lattice.width
    P = cells.shape[1]
    pos = node.Pos_1.reshape(-1, 3)[members]
    offsets = cells.astype(np.float64) * width
    return [Patch(offsets[g].copy(), np.full(P, width), pos[bounds[g]:bounds[g + 1]].T, centres[g].copy())
            for g in range(cells.shape[0])]


def lattice_offsets_i32(lattice):
    """int32 [N,P] = cells * width: the offsets ``spot.offsets_from_patches(lattice_patches(...))`` gives (whole
    numbers, exact in float32), without a patch."""
    return np.ascontiguousarray((lattice.cells.astype(np.int64) * int(lattice.width)).astype(np.int32))


def lattice_dis1(lattice, mic_positions):
    """float64 [N]: 1 + the distance of every cube's centre to microphone 0, formed per cube by the very expression of
    ``search.binary_search_baseline`` (``np.linalg.norm(c - mic_positions[0])``, then ``d + 1``)."""
    out = np.empty(lattice.n_cubes, dtype=np.float64)
    for g in range(lattice.n_cubes):
        out[g] = np.linalg.norm(lattice.centres[g] - mic_positions[0]) + 1
    return out


class LatticePatches(object):
    """``lattice_patches(node, lattice)`` as a lazy sequence: ``len``, iteration, integer and slice indexing.  ``[g]``
    builds a fresh ``Patch`` equal to item g of the list (``check_out`` mutates a patch, so every access returns a new
    object); ``built`` counts them.  ``offsets_i32`` and ``dis1`` are the tables of ``lattice_offsets_i32`` and
    ``lattice_dis1`` (``dis1`` may be None when no microphone position was given): a search that decides its coarse
    stage on the GPU scores the first, weights by the second and builds only the patches it keeps."""

    def __init__(self, node, lattice, offsets_i32=None, dis1=None):
        self.node, self.lattice = node, lattice
        self.offsets_i32 = lattice_offsets_i32(lattice) if offsets_i32 is None else offsets_i32
        self.dis1 = dis1
        self.built = 0

    def __len__(self):
        return self.lattice.n_cubes

    def _patch(self, g):
        cells, bounds, members, centres = self.lattice
        width = self.lattice.width
        pos = self.node.Pos_1.reshape(-1, 3)[members[bounds[g]:bounds[g + 1]]]
        self.built += 1
        return Patch(cells[g].astype(np.float64) * width, np.full(cells.shape[1], width), pos.T, centres[g].copy())

    def __getitem__(self, g):
        if isinstance(g, slice):
            return [self._patch(k) for k in range(*g.indices(len(self)))]
        k = int(g)
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError(f"cube {g} of a lattice of {len(self)}")
        return self._patch(k)

    def __iter__(self):
        return (self._patch(g) for g in range(len(self)))


# ---- non-maximum suppression over the lattice (Prone_method="DENSE_NMS") ---------------------------------------
def lattice_local_maxima(cells, scores, radius=1, chunk=1 << 22):
    """(best int32 [N], degree int32 [N]) of the cubes ``cells`` int32 [N,P] (as ``coarse_lattice`` /
    ``dense_tdoa_candidates`` return them) under ``scores`` float64 [N], all finite.

    Cube j is near cube i when max_p |cells[i,p] - cells[j,p]| <= ``radius`` (Chebyshev distance in cell space; i is
    near itself).  ``degree[i]`` counts the near cubes other than i; ``best[i]`` is the near cube with the largest
    score, the lowest index among equals (-0.0 equals 0.0).  Cube i is a local maximum when ``best[i] == i``.
    csrc/geometry_kernels.hip (``asw_lattice_nms``) computes the same two arrays on the GPU, exactly; this is their
    statement.  Rows are taken ``chunk // N`` at a time, so the [rows, N] temporaries stay bounded."""
    cells = np.asarray(cells)
    scores = np.asarray(scores, dtype=np.float64)
    if cells.ndim != 2 or scores.shape != (cells.shape[0],):
        raise ValueError(f"cells must be [N, P] and scores [N], got {cells.shape} and {scores.shape}")
    if int(radius) != radius or radius < 1:
        raise ValueError(f"radius must be a whole number >= 1, got {radius!r}")
    if not np.all(np.isfinite(scores)):
        raise ValueError("every score must be finite")
    N, P = cells.shape
    best, degree = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
    wide = cells.astype(np.int64)                            # differences of int32 cells cannot overflow
    rows = max(1, int(chunk) // max(N, 1))
    for lo in range(0, N, rows):
        hi = min(N, lo + rows)
        near = np.ones((hi - lo, N), dtype=bool)
        for p in range(P):                                   # one pair at a time
            near &= np.abs(wide[lo:hi, p, None] - wide[None, :, p]) <= radius
        degree[lo:hi] = near.sum(axis=1) - 1
        best[lo:hi] = np.argmax(np.where(near, scores[None, :], -np.inf), axis=1)     # first of the largest
    return best, degree


def lattice_local_maxima_device(cells_dev, scores, radius=1, sorted_checked=False):
    """``lattice_local_maxima`` by ``torch.ops.asw.lattice_nms`` on a cells tensor that lives on the GPU: only the N
    scores go up, ``best`` and ``degree`` come back.  Refuses what the statement refuses, and a table whose column 0
    decreases somewhere -- the kernel finds the cubes near a block of rows by bisection in that column.
    ``scores`` may also be a float64 tensor on the cells' device: nothing goes up then, nothing waits for the device and
    ``best`` and ``degree`` are returned as device tensors; whether every score is finite cannot be asked without a
    read-back and is left to the caller (a score that is not finite only loses comparisons, it faults nothing), and the
    caller vouches for the sort order with ``sorted_checked`` once it has asked."""
    import torch
    from . import native
    resident = isinstance(scores, torch.Tensor)
    if resident:
        if scores.device != cells_dev.device or scores.dtype != torch.float64:
            raise ValueError("device scores must be float64 on the device of cells")
        scores = scores.contiguous()
    else:
        scores = np.ascontiguousarray(scores, dtype=np.float64)
    if cells_dev.dim() != 2 or tuple(scores.shape) != (int(cells_dev.shape[0]),):
        raise ValueError(f"cells must be [N, P] and scores [N], got {tuple(cells_dev.shape)} and {tuple(scores.shape)}")
    if int(radius) != radius or radius < 1:
        raise ValueError(f"radius must be a whole number >= 1, got {radius!r}")
    if not resident and not np.all(np.isfinite(scores)):
        raise ValueError("every score must be finite")
    if not sorted_checked and cells_dev.shape[0] > 1 and not bool((cells_dev[1:, 0] >= cells_dev[:-1, 0]).all()):
        raise ValueError("column 0 of cells must be non-decreasing (the lattice is sorted with pair 0 most significant)")
    if resident:
        best, degree = native.torch_ops().lattice_nms(cells_dev, scores, int(radius))
        return best, degree
    best, degree = native.torch_ops().lattice_nms(cells_dev, torch.from_numpy(scores).to(cells_dev.device), int(radius))
    return best.cpu().numpy(), degree.cpu().numpy()
