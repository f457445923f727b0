"""SRP-PHAT pruning stage: geometry tables on the host (or, with ``geometry="device"``, built on the
GPU by csrc/geometry_kernels.hip), steered-response map on the GPU.

Mirrors ``SRP_PHAT`` (sep/Traditional_SP/SRP_Prunning.py:101-643; SURVEY.md §8 a-O, a-P,
a-Q) with the same method names used by the search (``reset``,
``SRP_Map_WINDOW_new``, ``local_source_adaptive``).  Differences by design:

* the one-off 3-D -> TDoA map (``Map_3D_TDoA`` + BFS ``search_cluster``, :277-344; 44 s
  of pure-Python loops in the reference) is computed with vectorised numpy and a sparse
  connected-components pass -- same clusters, same order;
* the [G,198,21] complex128 steering table (:368-381,230-246; 1.16 GB) is never built:
  the HIP map kernel regenerates exp(j w dtau) from the [G,M] propagation delays;
* the map itself (``SRP_Map_WINDOW_torch``, :387-434) runs in libasw_hip.so
  (csrc/srp_kernels.hip) -- there is no host fallback;
* the alternative MUSIC and TOPS maps (``MUSIC_Map_WINDOW`` / ``TOPS_Map_WINDOW``, :436-497)
  run in csrc/pruner_kernels.hip.  Where the reference would divide 0/0 (no complete
  window), they raise ``RuntimeError`` instead of leaving a NaN map;
* ``SRPPhat(..., geometry="device")`` builds the same tables with the ``torch.ops.asw.geom_*`` kernels -- for
  arrays that change from mixture to mixture, where the host build costs more than a batched search.  The
  integer tables are equal and the float tables bit-identical to the host build (same float64 expression
  order, no fma); ``clusters`` is then a lazy sequence over the CSR member arrays and ``Pos_5`` / ``Pos_1``
  are generated from the point index.  ``"device"`` without a GPU raises ``RuntimeError``;
* ``lattice_width=`` also builds the coarse TDoA lattice of the 1 cm lookup grid (``dense_grid.coarse_lattice``, the
  stage-1 list of ``Prone_method="DENSE"``) in the node's geometry mode: numpy on the host, ``geom_lattice`` on
  the planes tensor the device build made.  ``lattice_local_maxima`` (``Prone_method="DENSE_NMS"``) then runs on it: the
  numpy statement on the host, ``lattice_nms`` on the cells tensor a device build keeps on the GPU.
"""
import threading

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from .patch import Patch

ERR_TOLERANCE = 0.2        # SRP_Prunning.py:17
TOPS_WINDOW = 72000        # TOPS_Map_WINDOW ignores its window argument (SRP_Prunning.py:475)


class GridCluster(object):
    """A set of voxels sharing one quantised TDoA vector (SRP_Prunning.py:68-96)."""
    __slots__ = ("sample_offset", "grids", "index")

    def __init__(self, sample_offset, grids, index):
        self.sample_offset = sample_offset      # int [M-1]
        self.grids = grids                      # float [n,3]
        self.index = index                      # int [n,3] voxel indices

    def cluster_size(self):
        return len(self.index)

    def center_pos(self):
        return np.mean(self.grids, axis=0)


class ClusterSeq(object):
    """The cluster list of a device-built node: a read-only sequence whose items are ``GridCluster`` objects made
    on demand from the CSR arrays (``offsets`` [G,P], ``bounds`` [G+1], ``members`` [V]: flat voxel indices,
    ascending within a cluster) and the lattice axes.  Item i equals item i of the host-built list."""

    def __init__(self, offsets, bounds, members, x_grids, y_grids, z_grids):
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.bounds = np.asarray(bounds, dtype=np.int64)
        self.members = np.asarray(members, dtype=np.int64)
        self.axes = (np.asarray(x_grids), np.asarray(y_grids), np.asarray(z_grids))
        self.shape = tuple(len(a) for a in self.axes)

    def __len__(self):
        return self.offsets.shape[0]

    def sizes(self):
        return np.diff(self.bounds)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        i = int(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError("cluster index out of range")
        mem = self.members[self.bounds[i]:self.bounds[i + 1]]
        ix, iy, iz = np.unravel_index(mem, self.shape)
        pts = np.stack([self.axes[0][ix], self.axes[1][iy], self.axes[2][iz]], axis=1)
        return GridCluster(self.offsets[i], pts, np.stack([ix, iy, iz], axis=1))

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class LookupPositions(object):
    """``Pos_5`` / ``Pos_1`` of a device-built node: the [ny,nx,nz,3] point table of a lookup grid, generated from
    the flat point index ((y*nx + x)*nz + z) instead of stored.  Supports what the cube scans use:
    ``pos.reshape(-1, 3)[idx]``; ``np.asarray(pos)`` materialises the table."""

    def __init__(self, xx, yy, zz):
        self.xx, self.yy, self.zz = xx, yy, zz
        self.shape = (len(yy), len(xx), len(zz), 3)

    def reshape(self, *shape):
        if shape not in ((-1, 3), ((-1, 3),)):
            return np.asarray(self).reshape(*shape)
        return self

    def __getitem__(self, idx):
        y, x, z = np.unravel_index(np.asarray(idx, dtype=np.int64), self.shape[:3])
        return np.stack([self.xx[x], self.yy[y], self.zz[z]], axis=-1)

    def __array__(self, dtype=None, copy=None):
        X, Y, Z = np.meshgrid(self.xx, self.yy, self.zz)
        a = np.stack((X, Y, Z), axis=3)
        return a if dtype is None else a.astype(dtype)


_TABLES_LOCK = threading.RLock()        # guards the lazily built lattice tables of every node (SRPPhat.lattice_tables)
_TWIDDLES = {}
_TWIDDLES_LOCK = threading.Lock()


def _twiddles(freq_bins, n_fft, dev):
    """(nb_pad, DFT twiddle table on ``dev``) of a bin range.  The table does not depend on the array, so it is
    uploaded once per device and bin range and shared by every node (with one array per mixture it would
    otherwise cross PCIe once per mixture: 3.1 MB)."""
    import torch
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    nb = len(freq_bins)
    key = (index, int(n_fft), int(freq_bins[0]), nb, bool(np.array_equal(freq_bins, np.arange(freq_bins[0], freq_bins[0] + nb))))
    with _TWIDDLES_LOCK:
        hit = _TWIDDLES.get(key) if key[-1] else None
        if hit is None:
            nb_pad = ((nb + 63) // 64) * 64
            k = freq_bins.astype(np.float64)[:, None]
            nn = np.arange(n_fft, dtype=np.float64)[None, :]
            ang = 2 * np.pi * k * nn / n_fft
            tw = np.zeros((2 * nb_pad, n_fft), dtype=np.float32)
            tw[:nb] = np.cos(ang)
            tw[nb_pad:nb_pad + nb] = -np.sin(ang)
            hit = (nb_pad, torch.from_numpy(tw).to(dev))
            if key[-1]:
                _TWIDDLES[key] = hit
    return hit


def _offsets_within(offsets, center, width):
    """All pairs within +-width/2 of ``center`` (hyperbola_offset / hyperbola_area_sample,
    SRP_Prunning.py:19-39); offsets [..., P].  The same comparisons as the all-pairs mask,
    evaluated pair by pair on the survivors only (the cube is a tiny part of the table)."""
    c = np.asarray(center, dtype=np.float64)
    lo, hi = c - width / 2, c + width / 2
    P = offsets.shape[-1]
    flat = offsets.reshape(-1, P)
    v = flat[:, 0]
    idx = np.flatnonzero((v >= lo[0]) & (v <= hi[0]))
    for p in range(1, P):
        if idx.shape[0] == 0:
            break
        v = flat[idx, p]
        idx = idx[(v >= lo[p]) & (v <= hi[p])]
    mask = np.zeros(flat.shape[0], dtype=bool)
    mask[idx] = True
    return mask.reshape(offsets.shape[:-1])


class SRPPhat(object):
    def __init__(self, mic_pos, freq_bins, Range_spk, C=343, FS=16000, n_fft=1024, grid_size=0.06,
                 grid_size_z=0.1, sample_resolution=4, threshold=0.03, WIDTH=8, device=None, geometry="host",
                 lattice_width=None):
        if geometry not in ("host", "device"):
            raise ValueError(f'geometry must be "host" or "device", got {geometry!r}')
        self.geometry = geometry
        self.lattice_width = lattice_width
        self.lattice = None
        self.device = device
        self.C, self.FS, self.n_fft = C, FS, n_fft
        self.freq_bins = np.asarray(freq_bins)
        self.mic_pos = np.asarray(mic_pos, dtype=np.float64)
        self.num_mic = self.mic_pos.shape[0]
        self.mic_center = self.mic_pos.mean(0)
        self.sample_resolution = sample_resolution
        self.WIDTH = WIDTH
        self.threshold = threshold
        self.Range_spk = Range_spk
        r = Range_spk
        self.x_grids = np.arange(r[0], r[1], grid_size)
        self.y_grids = np.arange(r[2], r[3], grid_size)
        self.z_grids = np.arange(r[4], r[5], grid_size_z)
        self.Lx, self.Ly, self.Lz = len(self.x_grids), len(self.y_grids), len(self.z_grids)
        self.Axis_range = [[r[0], r[1]], [r[2], r[3]], [r[4], r[5]]]
        keepout = 0.2                                       # :174-180
        self.array_border = [self.mic_pos[:, 0].min() - keepout, self.mic_pos[:, 1].min() - keepout,
                             self.mic_pos[:, 0].max() + keepout, self.mic_pos[:, 1].max() + keepout]
        self.omega = 2 * np.pi * FS * self.freq_bins / n_fft
        self._geom_dev = None
        if geometry == "device":
            self._build_on_device()
        else:
            self._build_on_host()
            if lattice_width is not None:
                self.lattice = self.coarse_lattice(lattice_width)
        self.tops_coef = 2 * np.pi * FS / (n_fft * C)
        self.tops_max_bin = None
        ii, jj = np.triu_indices(self.num_mic, k=1)          # row-major upper triangle == mask_triu order
        self.pair_i, self.pair_j = ii.astype(np.int32), jj.astype(np.int32)
        self.SRP_map = np.zeros(self.grids.shape[0], dtype=np.float32)
        self.MAX_POWER, self.Min_POWER = -100, 0.0
        self._dev = None

    # ---- one-off geometry ---------------------------------------------------------
    def _build_on_host(self):
        gx, gy = np.meshgrid(self.x_grids, self.y_grids, indexing="ij")
        self.dis_matrix = np.sqrt((gx - self.mic_center[0]) ** 2 + (gy - self.mic_center[1]) ** 2) + 1e-8

        # 5 cm and 1 cm lookup grids with their TDoA vectors (:149-170)
        self.Pos_5, self.Offset_5 = self._lookup_grid(0.05)
        self.Pos_1, self.Offset_1 = self._lookup_grid(0.01)
        # pair-major copies for the cube scans (asw_cube_select_planes streams one pair's plane)
        self._planes_5 = np.ascontiguousarray(np.moveaxis(self.Offset_5, 3, 0))
        self._planes_1 = np.ascontiguousarray(np.moveaxis(self.Offset_1, 3, 0))

        self._map_3d_tdoa()

        # propagation delays used by the steering term; mic z is ignored and the point's z is
        # taken absolute, exactly as generate_mod_vector does (:368-381)
        dx = self.grids[:, None, 0] - self.mic_pos[None, :, 0]
        dy = self.grids[:, None, 1] - self.mic_pos[None, :, 1]
        self.tau = np.sqrt(dx ** 2 + dy ** 2 + self.grids[:, None, 2] ** 2) / self.C      # [G,M] seconds
        # TOPS path differences (TOPS_block.py:45-48,105-112): mics and points centred on the mic mean, in
        # full 3-D; delta[g, m] = |p_g| - |p_g - m_m|.  The steering phase is tops_coef * (k - f0) * delta.
        pc = self.grids - self.mic_center
        mc = self.mic_pos - self.mic_center
        self.tops_delta = np.linalg.norm(pc, axis=1)[:, None] - np.linalg.norm(pc[:, None, :] - mc[None], axis=2)

    def _build_on_device(self):
        """The same tables from csrc/geometry_kernels.hip (``torch.ops.asw.geom_*``): the kernels get the axis arrays
        computed here, so every position is the host's; tau and tops_delta also stay on the device for the map
        kernels.  ``build_times`` keeps the split of the build: kernels (to the last synchronise), device-to-host
        copies, host remainder, in seconds."""
        import time
        import torch
        from . import native
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError('geometry="device" builds the tables on the MI355X (no host fallback)')
        t0 = time.perf_counter()
        ops = native.torch_ops()
        r = self.Range_spk
        C, FS = float(self.C), float(self.FS)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        mics = up(self.mic_pos)
        zz = np.arange(r[4], r[5], 0.1)
        zz_d = up(zz)
        lookup = {}
        axes_1 = None
        for step in (0.05, 0.01):
            xx, yy = np.arange(r[0], r[1], step), np.arange(r[2], r[3], step)
            axes_1 = (up(xx), up(yy), zz_d)
            lookup[step] = (xx, yy, ops.geom_lookup_planes(axes_1[1], axes_1[0], zz_d, mics, C, FS))
        xs, ys, zs = up(self.x_grids), up(self.y_grids), up(self.z_grids)
        centre = [float(v) for v in self.mic_center]
        q, valid, dis = ops.geom_voxel_map(xs, ys, zs, mics, [float(v) for v in self.array_border], centre, C, FS,
                                           float(self.sample_resolution))
        labels, self.label_sweeps = ops.geom_label(q, valid, self.Lx, self.Ly, self.Lz)
        power_index, valid_flat, valid_cid, members, bounds, offsets, centres, tau, delta = \
            ops.geom_compact(labels, q, xs, ys, zs, mics, centre, C)
        G = int(offsets.shape[0])
        if G == 0:
            raise RuntimeError("the keep-out region covers the whole speaker range: no valid voxel")
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()

        (xx5, yy5, p5), (xx1, yy1, p1) = lookup[0.05], lookup[0.01]
        self._planes_5, self._planes_1 = native.to_host(p5), native.to_host(p1)     # one copy per table
        small = [t.cpu().numpy() for t in (power_index, valid_flat, valid_cid, members, bounds, offsets, centres, tau, delta,
                                            dis)]
        t2 = time.perf_counter()

        self.Offset_5, self.Offset_1 = np.moveaxis(self._planes_5, 0, 3), np.moveaxis(self._planes_1, 0, 3)   # views
        self.Pos_5, self.Pos_1 = LookupPositions(xx5, yy5, zz), LookupPositions(xx1, yy1, zz)
        self.POWER_MAP = np.zeros((self.Lx, self.Ly, self.Lz))
        self.POWER_INDEX = small[0].astype(int).reshape(self.Lx, self.Ly, self.Lz)
        self._valid_flat, self._valid_cid = small[1].astype(np.int64), small[2].astype(np.int64)
        self.clusters = ClusterSeq(small[5], small[4], small[3], self.x_grids, self.y_grids, self.z_grids)
        self.grids, self.tau, self.tops_delta, self.dis_matrix = small[6], small[7], small[8], small[9]
        self.SRP_times = G
        self._geom_dev = {"dev": dev, "tau": tau, "delta": delta}
        self.build_times = {"kernels_s": t1 - t0, "d2h_s": t2 - t1, "host_s": time.perf_counter() - t2}
        if self.lattice_width is not None:
            # the lattice is made of the 1 cm planes: they stay on the device (P x points x 8 bytes) for as long as the
            # node lives, so another width costs no upload either
            t3 = time.perf_counter()
            self._geom_dev.update(planes_1=p1, axes_1=axes_1)
            self.lattice = self.coarse_lattice(self.lattice_width)
            self.build_times["lattice_s"] = time.perf_counter() - t3

    def coarse_lattice(self, width):
        """``dense_grid.coarse_lattice`` of this node in its geometry mode.  A host-built node evaluates the numpy
        statement; a device-built one runs ``torch.ops.asw.geom_lattice`` on the planes tensor its build left on the
        GPU (a node made with ``lattice_width=``) and copies only cells, bounds, members and centres to the host."""
        from .dense_grid import Lattice, coarse_lattice
        if self.geometry != "device":
            return coarse_lattice(self, width)
        from . import native
        g = self._geom_dev
        if g is None or g.get("planes_1") is None:
            raise RuntimeError("a device-built node keeps its 1 cm planes on the GPU only when made with lattice_width=")
        xs, ys, zs = g["axes_1"]
        out = native.torch_ops().geom_lattice(g["planes_1"], xs, ys, zs, [float(v) for v in self.array_border], float(width))
        cells, bounds, members, centres = (t.cpu().numpy() for t in out)
        if width == self.lattice_width:
            # the node's own lattice: its cells stay on the device for lattice_local_maxima (N x P x 4 bytes of their
            # own -- the op's result is a slice of a table sized for every lookup point)
            g["cells"] = out[0].clone()
        return Lattice(cells, bounds, members, centres, width)

    def lattice_local_maxima(self, scores, radius=1):
        """``dense_grid.lattice_local_maxima`` of this node's lattice (a node made with ``lattice_width=``) under
        ``scores`` [n_cubes], in the node's geometry mode: the numpy statement on a host-built node,
        ``torch.ops.asw.lattice_nms`` on the cells tensor the lattice build left on the GPU on a device-built one --
        the scores go up, (best, degree) come back, same values."""
        from .dense_grid import lattice_local_maxima, lattice_local_maxima_device
        if self.lattice is None:
            raise RuntimeError("this node has no lattice: make it with lattice_width=")
        if np.shape(scores) != (self.lattice.n_cubes,):
            raise ValueError(f"scores must hold one value per cube ({self.lattice.n_cubes}), got shape {np.shape(scores)}")
        if self.geometry != "device":
            return lattice_local_maxima(self.lattice.cells, scores, radius)
        return lattice_local_maxima_device(self._geom_dev["cells"], scores, radius)

    def lattice_tables(self, mic_positions=None):
        """(offsets_i32 [N,P], dis1 [N]) of this node's lattice (``dense_grid.lattice_offsets_i32`` / ``lattice_dis1``
        against ``mic_positions[0]``, default the node's own microphone 0), built at the first call and kept: the
        tables of a search that decides its coarse stage on the GPU."""
        from .dense_grid import lattice_dis1, lattice_offsets_i32
        if self.lattice is None:
            raise RuntimeError("this node has no lattice: make it with lattice_width=")
        with _TABLES_LOCK:
            if getattr(self, "_lattice_tables", None) is None:
                mic = self.mic_pos if mic_positions is None else mic_positions
                self._lattice_tables = (lattice_offsets_i32(self.lattice), lattice_dis1(self.lattice, mic))
                self._lattice_dev = {}
            return self._lattice_tables

    def lattice_tables_device(self, device):
        """{"offsets": int32 [N,P], "dis1": float64 [N], "cells": int32 [N,P]} of ``lattice_tables`` as tensors on
        ``device``, made once per device and kept.  On a device-built node whose cells live on that device the
        offsets derive from that tensor and the cells are it; everything else goes up once.  The sort order the
        ``lattice_nms`` kernel needs is asked here, once."""
        import torch
        offsets, dis1 = self.lattice_tables()
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        with _TABLES_LOCK:
            hit = self._lattice_dev.get(device)
            if hit is None:
                g = self._geom_dev
                cells = g.get("cells") if g is not None else None
                if cells is not None and cells.device == device:
                    off_d = (cells * int(self.lattice.width)).contiguous()
                else:
                    cells = torch.from_numpy(np.ascontiguousarray(self.lattice.cells, dtype=np.int32)).to(device)
                    off_d = torch.from_numpy(offsets).to(device)
                if cells.shape[0] > 1 and not bool((cells[1:, 0] >= cells[:-1, 0]).all()):
                    raise ValueError("column 0 of cells must be non-decreasing (the lattice is sorted with pair 0 most significant)")
                hit = self._lattice_dev[device] = {"offsets": off_d, "dis1": torch.from_numpy(dis1).to(device), "cells": cells}
            return hit

    def lattice_local_maxima_resident(self, scores_dev, radius=1):
        """``lattice_local_maxima`` under scores that are a float64 tensor [n_cubes]: -> (best, degree) as int32 tensors
        on the scores' device.  On the GPU ``torch.ops.asw.lattice_nms`` runs on the cells of ``lattice_tables_device``
        with no upload, no read-back and no check that the scores are finite (the caller learns that from
        ``coarse_select``'s count); CPU tensors (a stand-in scorer) go through the numpy statement."""
        import torch
        from .dense_grid import lattice_local_maxima, lattice_local_maxima_device
        if tuple(scores_dev.shape) != (self.lattice.n_cubes,):
            raise ValueError(f"scores must hold one value per cube ({self.lattice.n_cubes}), got shape {tuple(scores_dev.shape)}")
        if not scores_dev.is_cuda:
            best, degree = lattice_local_maxima(self.lattice.cells, scores_dev.numpy(), radius)
            return torch.from_numpy(best), torch.from_numpy(degree)
        cells = self.lattice_tables_device(scores_dev.device)["cells"]
        return lattice_local_maxima_device(cells, scores_dev, radius, sorted_checked=True)

    def _lookup_grid(self, step):
        r = self.Range_spk
        xx, yy, zz = np.arange(r[0], r[1], step), np.arange(r[2], r[3], step), np.arange(r[4], r[5], 0.1)
        X, Y, Z = np.meshgrid(xx, yy, zz)
        pos = np.stack((X, Y, Z), axis=3)
        d0 = np.linalg.norm(pos - self.mic_pos[0, :], axis=3) / self.C * self.FS
        offs = [np.linalg.norm(pos - self.mic_pos[i, :], axis=3) / self.C * self.FS - d0
                for i in range(1, self.num_mic)]
        return pos, np.stack(offs, axis=3)

    def _valid_mask(self):
        b = self.array_border
        inside = ((self.x_grids[:, None] > b[0]) & (self.x_grids[:, None] < b[2])
                  & (self.y_grids[None, :] > b[1]) & (self.y_grids[None, :] < b[3]))
        return np.broadcast_to(~inside[:, :, None], (self.Lx, self.Ly, self.Lz))

    def _map_3d_tdoa(self):
        """Quantised TDoA per voxel, then merge 26-connected voxels with identical TDoA
        (Map_3D_TDoA + search_cluster, :277-344).  Cluster order = order in which the
        reference's (ix,iy,iz) scan first meets each cluster."""
        Lx, Ly, Lz = self.Lx, self.Ly, self.Lz
        X, Y, Z = np.meshgrid(self.x_grids, self.y_grids, self.z_grids, indexing="ij")
        pos = np.stack([X, Y, Z], axis=-1)
        d = np.linalg.norm(pos[..., None, :] - self.mic_pos[None, None, None], axis=-1)
        off = (d[..., 1:] - d[..., :1]) / self.C * self.FS
        q = np.round(off / self.sample_resolution).astype(int) * self.sample_resolution
        valid = self._valid_mask()
        n = Lx * Ly * Lz
        flat_valid = valid.reshape(n)
        qf = q.reshape(n, -1)
        idx3 = np.arange(n).reshape(Lx, Ly, Lz)
        rows, cols = [], []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    if (dx, dy, dz) <= (0, 0, 0):
                        continue                        # each undirected neighbour pair once
                    sa = (slice(max(0, -dx), Lx - max(0, dx)), slice(max(0, -dy), Ly - max(0, dy)),
                          slice(max(0, -dz), Lz - max(0, dz)))
                    sb = (slice(max(0, dx), Lx - max(0, -dx)), slice(max(0, dy), Ly - max(0, -dy)),
                          slice(max(0, dz), Lz - max(0, -dz)))
                    a, b = idx3[sa].ravel(), idx3[sb].ravel()
                    same = flat_valid[a] & flat_valid[b] & np.all(qf[a] == qf[b], axis=1)
                    rows.append(a[same])
                    cols.append(b[same])
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        graph = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n, n))
        _, lab = connected_components(graph, directed=False)
        vid = np.flatnonzero(flat_valid)
        if vid.shape[0] == 0:                                # the device build's message for G == 0
            raise RuntimeError("the keep-out region covers the whole speaker range: no valid voxel")
        vlab = lab[vid]
        _, first = np.unique(vlab, return_index=True)        # first voxel (scan order) of each label
        order = np.argsort(first)
        rank_of = np.empty(vlab.max() + 1, dtype=np.int64)
        rank_of[np.unique(vlab)[order]] = np.arange(len(order))
        cid = rank_of[vlab]
        G = len(order)
        self.POWER_MAP = np.zeros((Lx, Ly, Lz))
        self.POWER_INDEX = np.zeros((Lx, Ly, Lz), dtype=int)
        self.POWER_INDEX.reshape(n)[vid] = cid
        self._valid_flat = vid
        self._valid_cid = cid
        posf = pos.reshape(n, 3)
        srt = np.argsort(cid, kind="stable")
        bounds = np.searchsorted(cid[srt], np.arange(G + 1))
        ix3 = np.stack(np.unravel_index(vid, (Lx, Ly, Lz)), axis=1)
        self.clusters = []
        centers = np.zeros((G, 3))
        for g in range(G):
            mem = srt[bounds[g]:bounds[g + 1]]
            pts = posf[vid[mem]]
            self.clusters.append(GridCluster(qf[vid[mem[0]]], pts, ix3[mem]))
            centers[g] = pts.mean(axis=0)
        self.grids = centers
        self.SRP_times = G

    # ---- per-mixture -----------------------------------------------------------------
    def reset(self):
        self.SRP_map = np.zeros(self.grids.shape[0], dtype=np.float32)

    def _device_tables(self, dev):
        import torch
        if self._dev is None or self._dev["dev"] != dev:
            nb_pad, tw = _twiddles(self.freq_bins, self.n_fft, dev)
            built = self._geom_dev if self._geom_dev is not None and self._geom_dev["dev"] == dev else None
            self._dev = {"dev": dev, "nb_pad": nb_pad, "tw": tw,
                         # a device-built node left its delays on the device: nothing to upload again
                         "tau": built["tau"] if built else torch.from_numpy(np.ascontiguousarray(self.tau)).to(dev),
                         "omega": torch.from_numpy(np.ascontiguousarray(self.omega, dtype=np.float64)).to(dev),
                         "pi": torch.from_numpy(self.pair_i).to(dev), "pj": torch.from_numpy(self.pair_j).to(dev),
                         "delta": built["delta"] if built else torch.from_numpy(np.ascontiguousarray(self.tops_delta)).to(dev)}
        return self._dev

    def _device_signal(self, signal):
        """(device, mixture as a float32 device tensor zero-padded to a multiple of 4 samples)."""
        import torch
        nb = len(self.freq_bins)
        assert np.array_equal(self.freq_bins, np.arange(self.freq_bins[0], self.freq_bins[0] + nb)), \
            "the pruning kernels take a contiguous bin range"
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("the pruning maps run only on the MI355X (no host fallback)")
        M, T = signal.shape
        assert self.mic_pos.shape[0] == M
        sig = torch.as_tensor(signal, dtype=torch.float32).to(dev)
        Tp = (T + 3) // 4 * 4
        if Tp != T:
            sig = torch.nn.functional.pad(sig, (0, Tp - T))
        return dev, sig.contiguous()

    def SRP_Map_WINDOW_new(self, signal, window=36000, tol=1e-8):
        """Steered-response map, maximum over half-overlapped windows (:383-434)."""
        import torch
        from . import native
        dev = torch.device(self.device if self.device is not None else "cuda")
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("SRP map runs only on the MI355X (no host fallback)")
        M, T = signal.shape
        assert self.mic_pos.shape[0] == M
        step = window // 2
        n_win = 0
        for j in range(0, T // step - 1):                  # :398-402
            if j * step + window > T:
                break
            n_win += 1
        t = self._device_tables(dev)
        sig = torch.as_tensor(signal, dtype=torch.float32).to(dev)
        Tp = (T + 3) // 4 * 4
        if Tp != T:
            sig = torch.nn.functional.pad(sig, (0, Tp - T))
        sig = sig.contiguous()
        hop = self.n_fft // 4
        # torch.ops.asw.srp_phat_map: DFT-GEMM + PHAT + cross-spectra, then the steered map
        out = native.torch_ops().srp_phat_map(sig, t["tw"], t["pi"], t["pj"], t["tau"], t["omega"], int(window), int(step),
                                              int(n_win), int(self.n_fft), int(hop), float(tol))
        self.SRP_map = out.cpu().numpy()
        self._finish_map()

    @staticmethod
    def _whole_windows(T, window):
        """Windows of the MUSIC / TOPS loops (:442-450,476-484): step = window, no overlap."""
        n = 0
        for j in range(T // window):
            if j * window + window > T:
                break
            n += 1
        return n

    def MUSIC_Map_WINDOW(self, signal, window=36000, tol=1e-8):
        """MUSIC pseudo-spectrum map (:436-467, MUSIC_block.py): per window and bin the noise
        subspace of the frame-averaged covariance, P = 1/|a^H En En^H a|, normalised per bin by its
        maximum over the grid, averaged over bins and then over the non-overlapping windows."""
        from . import native
        T = signal.shape[1]
        n_win = self._whole_windows(T, window)
        if n_win == 0:
            raise RuntimeError(f"MUSIC map: a {T}-sample mixture holds no whole {window}-sample window "
                               "(the reference would return a NaN map)")
        dev, sig = self._device_signal(signal)
        t = self._device_tables(dev)
        out = native.torch_ops().music_map(sig, t["tau"], t["omega"], int(self.freq_bins[0]), int(window), int(window),
                                           int(n_win), int(self.n_fft), int(self.n_fft // 4))
        self.SRP_map = out.cpu().numpy()
        self._finish_map()

    def TOPS_Map_WINDOW(self, signal, window=36000, tol=1e-8):
        """TOPS map (:470-497, TOPS_block.py:62-136): per 72 000-sample window (the argument is ignored, as
        in the reference) 1/s_min of D = [F0^H diag(conj phi_k) W_k]_k, averaged over windows.
        ``tops_max_bin`` keeps the reference bin index chosen in each window."""
        from . import native
        T = signal.shape[1]
        n_win = self._whole_windows(T, TOPS_WINDOW)
        if n_win == 0:
            raise RuntimeError(f"TOPS map needs at least {TOPS_WINDOW} samples, got {T} "
                               "(the reference would return a NaN map)")
        dev, sig = self._device_signal(signal)
        t = self._device_tables(dev)
        out, max_bin = native.torch_ops().tops_map(sig, t["delta"], int(self.freq_bins[0]),
                                                   int(len(self.freq_bins)), float(self.tops_coef), TOPS_WINDOW,
                                                   TOPS_WINDOW, int(n_win), int(self.n_fft), int(self.n_fft // 4))
        self.SRP_map = out.cpu().numpy()
        self.tops_max_bin = max_bin.cpu().numpy()
        self._finish_map()

    def set_map(self, srp_map):
        """Install a map computed elsewhere (tests / oracle) and refresh the derived state."""
        self.SRP_map = np.asarray(srp_map, dtype=np.float32)
        self._finish_map()

    def _finish_map(self):
        self.MAX_POWER = float(np.amax(self.SRP_map))
        self.Min_POWER = float(np.amin(self.SRP_map))
        # fill_powermap_torch (:347-357): every voxel takes its cluster's value
        self.POWER_MAP.reshape(-1)[self._valid_flat] = self.SRP_map[self._valid_cid]

    # ---- peak picking -------------------------------------------------------------------
    def find_valid_peak_new(self, rato=4):
        """Cluster ids of local maxima (5x5 in x,y; dz in {-1,0}) above the distance-weighted
        adaptive threshold, or of any voxel above `rato` times it (:500-544)."""
        thr = self.threshold[0] * self.MAX_POWER
        thr = min(max(thr, self.threshold[1]), self.threshold[2])
        thr2 = thr * rato
        print("Adaptive threshold: ", self.MAX_POWER, thr, thr2)
        pm = self.POWER_MAP
        NX, NY, NZ = pm.shape
        core = pm[2:-2, 2:-2, 1:-1]
        t1 = (thr * (0.9 + 1 / self.dis_matrix))[2:-2, 2:-2, None]
        t2 = (thr2 * (1 + 1 / self.dis_matrix))[2:-2, 2:-2, None]
        is_max = np.ones(core.shape, dtype=bool)
        for dx in range(-2, 3):
            for dy in range(-2, 3):
                for dz in range(-1, 1):
                    if dx == 0 and dy == 0 and dz == 0:
                        continue
                    is_max &= core >= pm[2 + dx:NX - 2 + dx, 2 + dy:NY - 2 + dy, 1 + dz:NZ - 1 + dz]
        sel = (is_max & (core > t1) & (core <= t2)) | (core > t2)
        peaks, seen = [], set()
        for ix, iy, iz in np.transpose(np.nonzero(sel)):
            g = int(self.POWER_INDEX[ix + 2, iy + 2, iz + 1])
            if g not in seen:
                seen.add(g)
                peaks.append(g)
        return peaks

    def hyperbola_area_init(self, sample_offsets, width):
        """3-D points (1 cm grid) whose TDoA lies inside the cube, found through the 5 cm
        grid's bounding box (:41-61).  Returns [3,n] or None."""
        pts = self._cube_points(self.Pos_5, self._planes_5, sample_offsets, width)
        if pts.shape[0] == 0:
            return None
        ax = self.Axis_range
        x0, x1 = max(ax[0][0], pts[:, 0].min() - 0.05), min(ax[0][1], pts[:, 0].max() + 0.05)
        y0, y1 = max(ax[1][0], pts[:, 1].min() - 0.05), min(ax[1][1], pts[:, 1].max() + 0.05)
        xi0, xi1 = int(np.floor((x0 - ax[0][0]) / 0.01)), int(np.ceil((x1 - ax[0][0]) / 0.01))
        yi0, yi1 = int(np.floor((y0 - ax[1][0]) / 0.01)), int(np.ceil((y1 - ax[1][0]) / 0.01))
        return self._cube_points(self.Pos_1, self._planes_1, sample_offsets, width, yi0, yi1, xi0, xi1).T

    @staticmethod
    def _cube_points(pos, planes, center, width, y0=0, y1=None, x0=0, x1=None):
        """Points [n,3] of the lookup grid (sub-box [y0,y1) x [x0,x1)) whose TDoA lies within
        +-width/2 of ``center`` on every pair: the native box scan (csrc/search_host.cpp,
        same comparisons and order as the boolean mask of ``_offsets_within``) over the
        pair-major table ``planes`` [P, ny, nx, nz]."""
        from ctypes import byref, c_int64, c_void_p
        from . import native
        P, ny, nx, nz = planes.shape
        y1 = ny if y1 is None else min(y1, ny)
        x1 = nx if x1 is None else min(x1, nx)
        y0, x0 = max(y0, 0), max(x0, 0)
        if y1 <= y0 or x1 <= x0:
            return np.zeros((0, 3))
        c = np.asarray(center, dtype=np.float64)
        lo, hi = np.ascontiguousarray(c - width / 2), np.ascontiguousarray(c + width / 2)
        cap = (y1 - y0) * (x1 - x0) * nz
        idx = np.empty(cap, dtype=np.int32)
        n = c_int64()
        native.check(native.lib().asw_cube_select_planes(c_void_p(planes.ctypes.data), ny, nx, nz, P, y0, y1, x0, x1,
                                                  c_void_p(lo.ctypes.data), c_void_p(hi.ctypes.data),
                                                  c_void_p(idx.ctypes.data), cap, byref(n)))
        return pos.reshape(-1, 3)[idx[:n.value]]

    def local_source_adaptive(self):
        """Greedy peak -> width-8 hypercube list (:547-643): strongest peak first, each new
        cube trimmed on its high side against the cubes already accepted, peaks covered by
        a cube are not revisited."""
        peak_index = self.find_valid_peak_new()
        print("peak_index: ", len(peak_index))
        peaks = self.SRP_map[peak_index]
        peaks_pos = self.grids[peak_index]
        self.peaks, self.peaks_pos = peaks, peaks_pos
        peaks_sample = np.array([self.clusters[i].sample_offset for i in peak_index])
        visited = np.zeros_like(peaks)
        P = self.num_mic - 1
        W = self.WIDTH
        accepted, peak_candidate = [], []
        for k in np.argsort(-1 * peaks):
            if visited[k] >= 1:
                continue
            center = peaks_sample[k]
            peak_candidate.append(peaks_pos[k, :])
            occupy = np.ones((P, W))
            for p in accepted:
                delta = p.sample_offset - center
                lo1 = delta - p.width_list / 2
                hi1 = delta + p.width_list / 2
                d1 = int(round((lo1 - W / 2).max()))
                d2 = int(round((hi1 + W / 2).min()))
                if d1 >= 0 or d2 <= 0:
                    continue                                   # disjoint in some pair
                # d1 < 0 always holds here, so only the high side is ever trimmed (a-Q)
                if W + d1 < 0:
                    occupy[:, :] = 0
                else:
                    occupy[:, W + d1:] = 0
            widths, offs, dead = [], [], False
            for i in range(P):
                on = np.where(occupy[i])[0]
                if on.shape[0] == 0:
                    dead = True
                    break
                widths.append(on.shape[0])
                offs.append(int(round(center[i] + (on[0] + on[-1] - W + 1) / 2)))
            if dead:
                continue
            visited += _offsets_within(peaks_sample, center, W + ERR_TOLERANCE).astype(int)
            widths, offs = np.array(widths), np.array(offs)
            # the reference uses the FIRST pair's trimmed width for every pair here (:629)
            area = self.hyperbola_area_init(offs, widths[0] + ERR_TOLERANCE)
            if area is None or area.shape[-1] == 0:
                continue
            accepted.append(Patch(offs, widths, area, peaks_pos[k, :]))
        print("SRP-PHAT candidate number: ", len(accepted))
        self.peak_candidate = np.array(peak_candidate)
        return accepted
