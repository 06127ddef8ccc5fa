"""The DTU benchmark's numbers for a fused point cloud, on the device: accuracy and completeness.

The reference scores a scan with MATLAB (evaluations/dtu/BaseEvalMain_web.m -> PointCompareMain.m -> reducePts_haa.m, MaxDistCP.m):
thin the cloud to one point per 0.2 mm neighbourhood, measure the nearest-neighbour distances cloud -> scanned surface (accuracy) and
back (completeness), capped at 60 mm, mask both sets, and report mean and median below 20 mm.  This module restates those four files
on the kernels of csrc/dtu_eval.hip and takes ``dtu_fusion.fuse_scan``'s ``xyz`` as it lies on the device -- no PLY, no KD-tree, no
MATLAB.  MATLAB computes in double; every geometric decision here is made in fp64 on the fp32 coordinates converted to fp64, with the
squared distance always (dx*dx + dy*dy) + dz*dz.

Two stated departures from the .m files:
  * the visiting order of the thinning is an ARGUMENT (a permutation, or a seed for ``torch.randperm`` on a CPU generator):
    MATLAB's ``randperm`` stream (reducePts_haa.m:9) cannot be reproduced and is not part of the contract;
  * distances >= ``max_dist`` are reported as ``max_dist``.  In MaxDistCP.m they are whatever the KD-tree of the point's 60 mm block
    returned (the nearest target inside the block's +-60 mm surroundings, :22-33); no statistic reads them (BaseEvalMain_web.m:72,75
    keep values below 20).  Below ``max_dist`` the values are MATLAB's exactly.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops

CELL_MARGIN = 1.0 + 2.0 ** -20          # smallest grid cell of the thinning, in units of dst
UNDECIDED, KEPT, REMOVED = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------------
# grid plumbing: extents, cell keys, sort
# ---------------------------------------------------------------------------------------------------------------------------
def _extent(xyz, name):
    """[2,3] fp64 on the host: per-axis minimum and maximum (the grid's one host synchronisation)."""
    ext = torch.stack([xyz.amin(0), xyz.amax(0)]).double().cpu()
    if not bool(torch.isfinite(ext).all()):
        raise ValueError(f"{name}: non-finite coordinate")
    return ext


def _grid(ext, cell):
    """(i0, dims) of the zero-anchored grid of edge ``cell`` over the extent: floor is monotonic, so the cell indices of the extreme
    coordinates bound every point's (same IEEE fp64 division as the kernel's)."""
    idx = torch.floor(ext / cell)
    if float(idx.abs().max()) >= 2.0 ** 30:
        raise ValueError(f"cell {cell} is too small for coordinates up to {float(ext.abs().max())}")
    i0 = [int(v) for v in idx[0]]
    dims = [int(b) - a + 1 for a, b in zip(i0, idx[1])]
    if dims[0] > 2 ** 21 or dims[1] > 2 ** 21 or dims[2] > 2 ** 20:
        raise ValueError(f"cell {cell} gives a grid of {dims} cells (limit 2^21 x 2^21 x 2^20)")
    return i0, dims


def _sorted_by_cell(xyz, cell, i0, dims, w=None):
    """-> (pts4 [n,4] fp32 in key order with column 3 = the int32 ``w`` as bits (or zero), sorted keys [n] int64, perm [n])."""
    keys, perm = torch.sort(ops.dtu_cell_keys(xyz, cell, i0, dims))
    rows = torch.zeros(xyz.shape[0], 4, device=xyz.device, dtype=torch.int32)        # integer copies: bits move unchanged
    rows[:, :3] = xyz[perm].view(torch.int32)
    if w is not None:
        rows[:, 3] = w[perm]
    return rows.view(torch.float32), keys, perm


def _points(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError(f"{name}: fp32 tensor [n,3] expected")
    return x.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. reducePts_haa.m
# ---------------------------------------------------------------------------------------------------------------------------
@ops.on_tensor_device
def reduce_points(xyz, dst, order=None, seed=None, cell=None):
    """reducePts_haa.m:6-33 on the device: visit the points in ``order``; a point still alive removes every point within ``dst`` of it
    (Euclidean, inclusive: d <= dst, the ``rangesearch`` of :22).  xyz [M,3] fp32 -> (keep [M] bool = ``indexSet``, rounds).

    The neighbour relation is symmetric, so the loop's result is the lexicographically first maximal independent set under the
    order -- the overlapping chunks of :16-20 visit one point twice and change nothing.  It is computed as rounds over
    {undecided, kept, removed}, each reading the previous round's buffer (``ops.dtu_reduce_round``), until no point is undecided:
    the same set whatever the scheduling.  ``rounds`` is the number of rounds that took; the undecided count is read once per round.

    order: permutation of M (order[k] = the point visited k-th, MATLAB's ``RandOrd``), or ``seed`` for ``torch.randperm`` on a CPU
    generator; neither = index order.  MATLAB's own random order (:9) is not reproducible and not part of the contract.
    cell: edge of the candidate grid, at least dst * (1 + 2^-20) (the default); the result does not depend on it."""
    xyz = _points(xyz, "xyz")
    n, dev = xyz.shape[0], xyz.device
    dst = float(dst)
    if not (0.0 <= dst < 1e150):
        raise ValueError("reduce_points: dst must be a finite non-negative number")
    if order is not None and seed is not None:
        raise ValueError("reduce_points: give order or seed, not both")
    if n == 0:
        return torch.zeros(0, device=dev, dtype=torch.bool), 0
    if seed is not None:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))
    if order is None:
        rank = torch.arange(n, device=dev, dtype=torch.int32)
    else:
        if not isinstance(order, torch.Tensor) or order.dim() != 1 or order.numel() != n or order.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"reduce_points: order must be an integer permutation of {n}")
        order = order.to(dev).long()
        if int(order.min()) < 0 or int(order.max()) >= n:
            raise ValueError("reduce_points: order holds an index outside the points")
        rank = torch.full((n,), -1, device=dev, dtype=torch.int32)
        rank[order] = torch.arange(n, device=dev, dtype=torch.int32)
        if int(rank.min()) < 0:
            raise ValueError("reduce_points: order is not a permutation (an index is missing)")
    low = dst * CELL_MARGIN
    if cell is None:
        cell = low if dst > 0.0 else 1.0
    cell = float(cell)
    if not cell >= low or not cell > 0.0:
        raise ValueError(f"reduce_points: the grid cell must be at least dst * (1 + 2^-20) = {low}")
    i0, dims = _grid(_extent(xyz, "xyz"), cell)
    pts4, keys, perm = _sorted_by_cell(xyz, cell, i0, dims, rank)
    state = [torch.zeros(n, device=dev, dtype=torch.uint8), torch.empty(n, device=dev, dtype=torch.uint8)]
    left = torch.empty(ops.dtu_reduce_blocks(n), device=dev, dtype=torch.int32)
    rounds = 0
    while True:
        ops.dtu_reduce_round(pts4, keys, dims, dst, state[0], state[1], left)
        state.reverse()
        rounds += 1
        if int(left.sum()) == 0:
            break
        if rounds > n:                 # every round decides at least the undecided point of smallest rank
            raise RuntimeError("reduce_points: no progress")
    keep = torch.empty(n, device=dev, dtype=torch.bool)
    keep[perm] = state[0] == KEPT
    return keep, rounds


# ---------------------------------------------------------------------------------------------------------------------------
# 2. MaxDistCP.m
# ---------------------------------------------------------------------------------------------------------------------------
@ops.on_tensor_device
def nn_dist2_capped(src, dst_pts, cap, cell=None):
    """The ``knnsearch`` of MaxDistCP.m:31-33 without the block loop around it: src [n,3], dst_pts [m,3] fp32 ->
    fp64 [n] = min(cap^2, min_j d^2(src_i, dst_pts_j)).  A minimum does not depend on the visiting order, and the shell search
    visits a superset of the cells that can hold it, so the values are reproducible bit for bit and independent of ``cell`` (the
    edge of the grid over ``dst_pts``; default: half the largest extent over the cube root of m).  m = 0 gives cap^2."""
    src, dst_pts = _points(src, "src"), _points(dst_pts, "dst_pts")
    cap = float(cap)
    if not (0.0 <= cap < 1e150):
        raise ValueError("nn_dist2_capped: cap must be a finite non-negative number")
    m, dev = dst_pts.shape[0], dst_pts.device
    if src.device != dev:
        raise ValueError("nn_dist2_capped: both point sets must be on one device")
    if m == 0:
        return ops.dtu_nn_capped(src, torch.zeros(0, 4, device=dev), torch.zeros(0, device=dev, dtype=torch.int64), 1.0, (0, 0, 0),
                                 (1, 1, 1), cap)
    if src.shape[0] and not bool(torch.isfinite(src).all()):
        raise ValueError("src: non-finite coordinate")
    ext = _extent(dst_pts, "dst_pts")
    if cell is None:
        cell = 0.5 * float((ext[1] - ext[0]).max()) / m ** (1.0 / 3.0)
        cell = max(cell, float(ext.abs().max()) * 2.0 ** -28)
        if cell <= 0.0:
            cell = 1.0
    cell = float(cell)
    if not cell > 0.0:
        raise ValueError("nn_dist2_capped: cell must be positive")
    i0, dims = _grid(ext, cell)
    to4, keys, _ = _sorted_by_cell(dst_pts, cell, i0, dims)
    return ops.dtu_nn_capped(src, to4, keys, cell, i0, dims, cap)


def block_range(bb, max_dist):
    """The half-open box the block loop of MaxDistCP.m:5-18 covers: blocks 0..floor((BB(2,:) - BB(1,:)) / MaxDist) of edge MaxDist
    per axis from BB(1,:).  A ``from`` point outside it is in no block and keeps MaxDist (:3).  bb [2,3] fp64 -> (lo [3], hi [3])."""
    nb = torch.floor((bb[1] - bb[0]) / max_dist)
    return bb[0], bb[0] + (nb + 1.0) * max_dist


def max_dist_cp(q_to, q_from, bb, max_dist, cell=None):
    """``Dist = MaxDistCP(Qto, Qfrom, BB, MaxDist)``: -> (Dist [n] fp64, Dist^2 [n] fp64).  Inside the block range a value below
    MaxDist is MATLAB's exactly (a block's tree holds everything within MaxDist of the block, :22-26); values MATLAB would report at or
    above MaxDist, and points outside the range, are MaxDist here (module docstring)."""
    d2 = nn_dist2_capped(q_from, q_to, max_dist, cell)
    lo, hi = block_range(bb, max_dist)
    q = q_from.double()
    inside = ((q >= lo) & (q < hi)).all(1)
    d2 = torch.where(inside, d2, torch.full_like(d2, float(max_dist) * float(max_dist)))
    d = torch.where(inside, torch.sqrt(d2), torch.full_like(d2, float(max_dist)))
    return d, d2


# ---------------------------------------------------------------------------------------------------------------------------
# 3 + 4. PointCompareMain.m, BaseEvalMain_web.m:69-78
# ---------------------------------------------------------------------------------------------------------------------------
def _mean_median(v):
    """mean and median as MATLAB's (the median of an even count is the mean of the two middle values); NaN for an empty set.  Sort and
    index: torch.quantile limits its input size."""
    n = v.numel()
    if n == 0:
        nan = torch.full((), float("nan"), device=v.device, dtype=torch.float64)
        return nan, nan.clone()
    s = torch.sort(v).values
    med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0
    return v.mean(), med


@ops.on_tensor_device
def point_compare(xyz, stl, obs_mask, bb, res, plane, dst=0.2, max_dist=60.0, outlier=20.0, order=None, seed=0, nn_cell=None):
    """``BaseEval = PointCompareMain(cSet, Qdata, dst, dataPath)`` (PointCompareMain.m:1-53) and the statistics of
    BaseEvalMain_web.m:69-78, everything on the device.

    xyz [M,3] fp32: the fused vertices (``fuse_scan(...)["xyz"]`` as it is); stl [S,3] fp32: the scanned surface, already reduced
    (:12); obs_mask [X,Y,Z] bool, bb [2,3], res: ``ObsMask``, ``BB``, ``Res`` of ObsMask<scan>_10.mat (:16-18); plane [4]: ``P`` of
    Plane<scan>.mat (:50); order / seed: the thinning's visiting order (``reduce_points``; seed is ignored when order is given).

    -> dict of device tensors: Qdata [N,3] (the reduced cloud, :7,45), Ddata [N] / Dstl [S] fp64 (:22,26; their squares Ddata2 /
    Dstl2), DataInMask [N] bool (:32-40), StlAbovePlane [S] bool (:52), keep [M] bool, and fp64 scalars acc_mean, acc_median (mean /
    median of Ddata[DataInMask & Ddata < outlier], BaseEvalMain_web.m:74-77), comp_mean, comp_median (Dstl[StlAbovePlane & Dstl <
    outlier], :71-72,78), overall = (acc_mean + comp_mean) / 2, downsample_factor (reducePts_haa.m:35); int64 scalars n_input,
    n_reduced, n_acc, n_comp, rounds."""
    xyz, stl = _points(xyz, "xyz"), _points(stl, "stl")
    dev = xyz.device
    if stl.device != dev:
        raise ValueError("point_compare: xyz and stl must be on one device")
    bb = torch.as_tensor(bb, dtype=torch.float64).reshape(2, 3)
    plane_h = [float(v) for v in torch.as_tensor(plane, dtype=torch.float64).reshape(4).cpu()]
    bb_h = bb.cpu()
    obs = torch.as_tensor(obs_mask)
    if obs.dim() != 3:
        raise ValueError("point_compare: obs_mask [X,Y,Z] expected")
    obs = (obs != 0).to(dev).contiguous()
    keep, rounds = reduce_points(xyz, dst, order=order, seed=None if order is not None else seed)
    q = xyz[keep]
    bb_d = bb_h.to(dev)
    d_data, d2_data = max_dist_cp(stl, q, bb_d, float(max_dist), nn_cell)
    d_stl, d2_stl = max_dist_cp(q, stl, bb_d, float(max_dist), nn_cell)
    in_mask = ops.dtu_obs_mask(q, obs, [float(v) for v in bb_h[0]], float(res))
    above = ops.dtu_above_plane(stl, plane_h)
    acc = d_data[in_mask & (d_data < outlier)]
    comp = d_stl[above & (d_stl < outlier)]
    acc_mean, acc_median = _mean_median(acc)
    comp_mean, comp_median = _mean_median(comp)

    def count(v):
        return torch.tensor(int(v), device=dev, dtype=torch.int64)

    n_red = q.shape[0]
    return {"Qdata": q, "Ddata": d_data, "Dstl": d_stl, "Ddata2": d2_data, "Dstl2": d2_stl, "DataInMask": in_mask,
            "StlAbovePlane": above, "keep": keep,
            "acc_mean": acc_mean, "acc_median": acc_median, "comp_mean": comp_mean, "comp_median": comp_median,
            "overall": (acc_mean + comp_mean) / 2.0,
            "downsample_factor": torch.tensor(xyz.shape[0] / n_red if n_red else float("nan"), device=dev, dtype=torch.float64),
            "n_input": count(xyz.shape[0]), "n_reduced": count(n_red), "n_acc": count(acc.numel()), "n_comp": count(comp.numel()),
            "rounds": count(rounds)}


# ---------------------------------------------------------------------------------------------------------------------------
# files: PLY, ObsMask / Plane .mat
# ---------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_xyz(path):
    """The x, y, z of a PLY file's ``vertex`` element as float32 [n,3] (what BaseEvalMain_web.m:51-52 and PointCompareMain.m:12-13 take
    from ``plyread``).  Header-driven: ASCII and binary files of either byte order, any further vertex properties (colours, normals)
    in any position; elements in front of ``vertex`` are skipped when their size is fixed."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: PLY header without end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if not elements:
                    raise ValueError(f"{path}: property before any element")
                elements[-1][2].append((tok[-1], None) if tok[1] == "list" else (tok[2], _PLY_TYPES.get(tok[1])))
                if tok[1] != "list" and tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown property type {tok[1]}")
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unknown PLY format {fmt}")
        for name, count, props in elements:
            fixed = all(t_ is not None for _, t_ in props)
            if name != "vertex":
                if fmt == "ascii":
                    for _ in range(count):
                        f.readline()
                elif fixed:
                    f.seek(count * sum(np.dtype(t_).itemsize for _, t_ in props), os.SEEK_CUR)
                else:
                    raise ValueError(f"{path}: a list element ({name}) lies in front of the vertices")
                continue
            names = [p for p, _ in props]
            if not fixed or any(a not in names for a in "xyz"):
                raise ValueError(f"{path}: the vertex element needs scalar properties x, y, z")
            if fmt == "ascii":
                rows = np.loadtxt(f, dtype=np.float64, max_rows=count, ndmin=2) if count else np.zeros((0, len(names)))
                if rows.shape != (count, len(names)):
                    raise ValueError(f"{path}: {count} vertices of {len(names)} properties expected")
                return np.stack([rows[:, names.index(a)] for a in "xyz"], -1).astype(np.float32)
            end = "<" if fmt == "binary_little_endian" else ">"
            dt = np.dtype([(p, end + t_) for p, t_ in props])
            data = np.fromfile(f, dtype=dt, count=count)
            if data.shape[0] != count:
                raise ValueError(f"{path}: file ends inside the vertices")
            return np.stack([data[a] for a in "xyz"], -1).astype(np.float32)
    raise ValueError(f"{path}: no vertex element")


def load_gt(data_path, scan):
    """The ground truth of one scan as PointCompareMain.m:10-18,50 loads it from the DTU "SampleSet" directory:
    Points/stl/stl<scan:03d>_total.ply, ObsMask/ObsMask<scan>_10.mat (ObsMask, BB, Res) and ObsMask/Plane<scan>.mat (P) ->
    dict(stl [S,3] float32, obs_mask [X,Y,Z] bool, bb [2,3] float64, res float, plane [4] float64), numpy arrays.  The .mat files
    are read with scipy.io.loadmat, i.e. MATLAB formats up to v7.2 (what the dataset ships); a v7.3 (HDF5) file is a ValueError."""
    from scipy.io import loadmat                   # lazy: only the file readers need scipy
    scan = int(scan)

    def mat(name):
        path = os.path.join(data_path, "ObsMask", name)
        try:
            return loadmat(path)
        except NotImplementedError as e:           # scipy reads MATLAB files up to v7.2; v7.3 files are HDF5
            raise ValueError(f"{path}: a MATLAB v7.3 (HDF5) file, which scipy.io.loadmat cannot read; save it again with "
                             "save(..., '-v7') (the DTU SampleSet ships v5 files)") from e

    m, p = mat(f"ObsMask{scan}_10.mat"), mat(f"Plane{scan}.mat")
    return {"stl": read_ply_xyz(os.path.join(data_path, "Points", "stl", f"stl{scan:03d}_total.ply")),
            "obs_mask": np.ascontiguousarray(np.asarray(m["ObsMask"]) != 0),
            "bb": np.asarray(m["BB"], dtype=np.float64).reshape(2, 3),
            "res": float(np.asarray(m["Res"]).reshape(-1)[0]),
            "plane": np.asarray(p["P"], dtype=np.float64).reshape(4)}


def evaluate_scan(xyz_or_ply, data_path, scan, device="cuda", **kwargs):
    """BaseEvalMain_web.m:51-78 for one scan: ``xyz_or_ply`` is the fused cloud, either a tensor [M,3] (``fuse_scan``'s ``xyz``, used
    where it lies) or the path of a PLY file; the ground truth comes from ``load_gt(data_path, scan)``; keyword arguments go to
    ``point_compare`` -> its dict."""
    if isinstance(xyz_or_ply, (str, os.PathLike)):
        xyz = torch.from_numpy(read_ply_xyz(xyz_or_ply)).to(device)
    else:
        xyz = xyz_or_ply
    gt = load_gt(data_path, scan)
    return point_compare(xyz, torch.from_numpy(gt["stl"]).to(xyz.device), torch.from_numpy(gt["obs_mask"]), gt["bb"], gt["res"],
                         gt["plane"], **kwargs)
