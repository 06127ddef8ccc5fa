"""CPU restatement of the reference's DTU evaluation (evaluations/dtu/reducePts_haa.m, MaxDistCP.m, PointCompareMain.m,
BaseEvalMain_web.m:69-78) in numpy fp64 + scipy.spatial.cKDTree: what effi_mvs_plus_amd/dtu_eval.py is checked against.

MATLAB works in double, so fp32 coordinates are converted to fp64 first.  The KD-trees only propose candidates: every decision
uses the squared distance (dx*dx + dy*dy) + dz*dz evaluated here in that order (``dist2``), never the tree's own value.
"""
import numpy as np
from scipy.spatial import cKDTree

CLEARANCE = 1e-12           # generators keep every pair distance this far (relative) from dst: ~8 fp64 roundings


def dist2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def neighbour_pairs(xyz, dst):
    """All i < j with d(i, j) <= dst (inclusive, reducePts_haa.m:22 ``rangesearch``) -> ([P,2] int64, their d^2)."""
    p = np.asarray(xyz, dtype=np.float64)
    if len(p) < 2:
        return np.zeros((0, 2), np.int64), np.zeros(0)
    cand = cKDTree(p).query_pairs(dst * (1.0 + 1e-6) + 1e-300, output_type="ndarray").astype(np.int64).reshape(-1, 2)
    d2 = dist2(p[cand[:, 0]], p[cand[:, 1]])
    return cand, d2


def min_clearance(xyz, dst):
    """Smallest |d / dst - 1| over the candidate pairs around the threshold (inf when there is none)."""
    _, d2 = neighbour_pairs(xyz, dst)
    return float(np.min(np.abs(np.sqrt(d2) / dst - 1.0))) if len(d2) else float("inf")


def assert_clear(xyz, dst):
    c = min_clearance(xyz, dst)
    assert c > CLEARANCE, f"a pair distance lies within {c:.1e} (relative) of dst"
    return c


def adjacency(xyz, dst):
    """CSR neighbour lists (the point itself excluded): (start [n+1], idx)."""
    n = len(xyz)
    cand, d2 = neighbour_pairs(xyz, dst)
    pairs = cand[d2 <= dst * dst]
    both = np.concatenate([pairs, pairs[:, ::-1]])
    both = both[np.argsort(both[:, 0], kind="stable")]
    start = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(both[:, 0], minlength=n), out=start[1:])
    return start, both[:, 1]


def reduce_sequential(xyz, dst, order, chunk=4000000, adj=None):
    """reducePts_haa.m:8-31 line by line, chunk ranges included (``Chunks = 1:min(4e6, n-1):n; Chunks(end) = n``; consecutive ranges
    share their end point, which is visited twice).  order: 0-based permutation (``RandOrd - 1``) -> indexSet.  n <= 1: the .m file's
    ``Chunks`` is empty there; every point is kept.  adj: ``adjacency(xyz, dst)`` when the caller already has it."""
    n = len(xyz)
    index_set = np.ones(n, bool)
    if n <= 1:
        return index_set
    start, idx = adj if adj is not None else adjacency(xyz, dst)
    chunks = list(range(1, n + 1, min(int(chunk), n - 1)))
    chunks[-1] = n
    for c in range(len(chunks) - 1):
        for pos in range(chunks[c], chunks[c + 1] + 1):             # Range = Chunks(c):Chunks(c+1), 1-based, inclusive
            i = order[pos - 1]
            if index_set[i]:
                index_set[idx[start[i]:start[i + 1]]] = False
                index_set[i] = True
    return index_set


def reduce_rounds(xyz, dst, order):
    """The same set as rounds over {undecided, kept, removed}, each round reading the previous round's states: an undecided point is
    removed if an earlier-ranked neighbour is kept, kept if all of them are removed -> (indexSet, rounds)."""
    n = len(xyz)
    if n == 0:
        return np.zeros(0, bool), 0
    rank = np.empty(n, np.int64)
    rank[np.asarray(order)] = np.arange(n)
    cand, d2 = neighbour_pairs(xyz, dst)
    pairs = cand[d2 <= dst * dst]
    both = np.concatenate([pairs, pairs[:, ::-1]])
    i, j = both[rank[both[:, 1]] < rank[both[:, 0]]].T             # j is an earlier-ranked neighbour of i
    state = np.zeros(n, np.int8)                                     # 0 undecided, 1 kept, 2 removed
    rounds = 0
    while True:
        kept_before = np.bincount(i, weights=state[j] == 1, minlength=n) > 0
        open_before = np.bincount(i, weights=state[j] == 0, minlength=n) > 0
        new = np.where(kept_before, 2, np.where(open_before, 0, 1)).astype(np.int8)
        state = np.where(state == 0, new, state)
        rounds += 1
        if not (state == 0).any():
            return state == 1, rounds


def nn_dist2_capped(src, to, cap):
    """min(cap^2, min_j d^2(src_i, to_j)) in fp64; the tree proposes its 8 nearest, ``dist2`` decides."""
    src, to = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(to, dtype=np.float64).reshape(-1, 3)
    out = np.full(len(src), float(cap) * float(cap))
    if len(to) == 0 or len(src) == 0:
        return out
    k = min(8, len(to))
    _, idx = cKDTree(to).query(src, k=k)
    idx = idx.reshape(len(src), k)
    return np.minimum(out, dist2(src[:, None, :], to[idx]).min(1))


def block_range(bb, max_dist):
    bb = np.asarray(bb, dtype=np.float64)
    nb = np.floor((bb[1] - bb[0]) / max_dist)
    return bb[0], bb[0] + (nb + 1.0) * max_dist


def max_dist_cp(q_to, q_from, bb, max_dist):
    """Capped nearest neighbour + the range rule of the block loop -> (Dist, Dist^2)."""
    q = np.asarray(q_from, dtype=np.float64).reshape(-1, 3)
    d2 = nn_dist2_capped(q_from, q_to, max_dist)
    lo, hi = block_range(bb, max_dist)
    inside = ((q >= lo) & (q < hi)).all(1)
    d2 = np.where(inside, d2, float(max_dist) * float(max_dist))
    return np.where(inside, np.sqrt(d2), float(max_dist)), d2


def max_dist_cp_literal(q_to, q_from, bb, max_dist):
    """MaxDistCP.m:3-39 line by line (a KD-tree per block over the targets within MaxDist of the block) -> Dist."""
    q_to, q_from = np.asarray(q_to, dtype=np.float64).reshape(-1, 3), np.asarray(q_from, dtype=np.float64).reshape(-1, 3)
    bb = np.asarray(bb, dtype=np.float64)
    dist = np.ones(len(q_from)) * max_dist
    rng = np.floor((bb[1] - bb[0]) / max_dist).astype(int)
    for x in range(rng[0] + 1):
        for y in range(rng[1] + 1):
            for z in range(rng[2] + 1):
                low = bb[0] + np.array([x, y, z]) * max_dist
                high = low + max_dist
                idx_f = np.nonzero(((q_from >= low) & (q_from < high)).all(1))[0]
                low, high = low - max_dist, high + max_dist
                idx_t = np.nonzero(((q_to >= low) & (q_to < high)).all(1))[0]
                if len(idx_t) == 0:
                    dist[idx_f] = max_dist
                elif len(idx_f):
                    dist[idx_f] = np.sqrt(nn_dist2_capped(q_from[idx_f], q_to[idx_t], 1e100))
    return dist


def matlab_round(v):
    """MATLAB's round: halves away from zero (np.round / torch.round go to even)."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    f = np.floor(a)
    return np.copysign(f + (a - f >= 0.5), v)


def data_in_mask(q, obs_mask, bb, res):
    """PointCompareMain.m:32-40."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    bb = np.asarray(bb, dtype=np.float64)
    qv = matlab_round((q - bb[0]) / res + 1.0)
    size = np.array(obs_mask.shape, dtype=np.float64)
    ok = ((qv > 0) & (qv <= size)).all(1)
    out = np.zeros(len(q), bool)
    iv = qv[ok].astype(np.int64) - 1
    out[ok] = np.asarray(obs_mask)[iv[:, 0], iv[:, 1], iv[:, 2]] != 0
    return out


def stl_above_plane(stl, plane):
    """PointCompareMain.m:52, summed left to right."""
    s, p = np.asarray(stl, dtype=np.float64).reshape(-1, 3), np.asarray(plane, dtype=np.float64).reshape(4)
    return ((p[0] * s[:, 0] + p[1] * s[:, 1]) + p[2] * s[:, 2]) + p[3] > 0


def mean_median(v):
    if len(v) == 0:
        return float("nan"), float("nan")
    s, n = np.sort(v), len(v)
    return float(np.mean(v)), float(s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0)


def point_compare(xyz, stl, obs_mask, bb, res, plane, order, dst=0.2, max_dist=60.0, outlier=20.0):
    """PointCompareMain.m + BaseEvalMain_web.m:69-78 with the rounds-free sequential thinning."""
    xyz, stl = np.asarray(xyz, dtype=np.float32), np.asarray(stl, dtype=np.float32)
    keep = reduce_sequential(xyz, dst, order)
    q = xyz[keep]
    d_data, d2_data = max_dist_cp(stl, q, bb, max_dist)
    d_stl, d2_stl = max_dist_cp(q, stl, bb, max_dist)
    in_mask, above = data_in_mask(q, obs_mask, bb, res), stl_above_plane(stl, plane)
    acc, comp = d_data[in_mask & (d_data < outlier)], d_stl[above & (d_stl < outlier)]
    (am, ad), (cm, cd) = mean_median(acc), mean_median(comp)
    return {"keep": keep, "Qdata": q, "Ddata": d_data, "Dstl": d_stl, "Ddata2": d2_data, "Dstl2": d2_stl, "DataInMask": in_mask,
            "StlAbovePlane": above, "acc_mean": am, "acc_median": ad, "comp_mean": cm, "comp_median": cd, "overall": (am + cm) / 2.0,
            "downsample_factor": len(xyz) / max(len(q), 1), "n_input": len(xyz), "n_reduced": len(q), "n_acc": len(acc),
            "n_comp": len(comp)}


# ---- generators shared by the host and the GPU tests -------------------------------------------------------------------------------
def noisy_patch(n, seed, half=2.5, sigma=0.05, dst=0.2):
    """x, y uniform in +-half (cell indices cross zero), z normal: ~85 neighbours within 0.2 for n = 20000 on 5 x 5."""
    g = np.random.default_rng(seed)
    xyz = np.stack([g.uniform(-half, half, n), g.uniform(-half, half, n), g.normal(0.0, sigma, n)], -1).astype(np.float32)
    assert_clear(xyz, dst)
    return xyz


def collinear(n=300, step=0.15, dst=0.2):
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = np.arange(n, dtype=np.float64) * step
    assert_clear(xyz, dst)
    return xyz


def two_surfaces(n_q, n_t, seed, far=200, outside=200, reach=100.0):
    """Queries on z ~ 0.3 + noise, targets on z ~ 0 + noise over 40 x 40, plus ``far`` queries ``reach`` above and ``outside`` queries
    beside the targets' bounding box."""
    g = np.random.default_rng(seed)
    t = np.stack([g.uniform(-20, 20, n_t), g.uniform(-20, 20, n_t), g.normal(0.0, 0.05, n_t)], -1)
    q = np.stack([g.uniform(-20, 20, n_q), g.uniform(-20, 20, n_q), 0.3 + g.normal(0.0, 0.05, n_q)], -1)
    f = np.stack([g.uniform(-20, 20, far), g.uniform(-20, 20, far), reach + g.uniform(0, 5, far)], -1)
    o = np.stack([g.uniform(21, 30, outside) * g.choice([-1.0, 1.0], outside), g.uniform(-30, 30, outside), g.normal(0, 1.0, outside)], -1)
    return np.concatenate([q, f, o]).astype(np.float32), t.astype(np.float32)


def synthetic_scan(seed=0, n_data=30000, n_stl=10000, dst=0.2):
    """A scan for point_compare: the surface z = 2 sin(x / 7) over x in [2, 98], y in [2, 38]; data = surface + noise, 3 % outliers up
    to 30 above it, 2 % beyond the block range in x; BB = [0,0,-20] .. [100,40,20] gives floor(100/60) + 1 = 2 blocks along x and one
    along y and z; ObsMask 40^3 at Res 2.5 (the data beside the range in x falls outside the mask volume, a fifth of the rest into unset voxels);
    the plane z = 0 puts about half of the ground truth below it."""
    g = np.random.default_rng(seed)

    def surf(n):
        x, y = g.uniform(2, 98, n), g.uniform(2, 38, n)
        return np.stack([x, y, 2.0 * np.sin(x / 7.0)], -1)

    data = surf(n_data) + g.normal(0, 0.08, (n_data, 3))
    k = int(0.03 * n_data)
    data[:k, 2] += g.uniform(1, 30, k)
    j = int(0.02 * n_data)
    data[k:k + j, 0] = g.choice([-1.0, 1.0], j) * g.uniform(0.5, 8, j) + np.where(g.random(j) < 0.5, 0.0, 120.0)
    stl = surf(n_stl)
    bb = np.array([[0.0, 0.0, -20.0], [100.0, 40.0, 20.0]])
    obs = g.random((40, 40, 40)) < 0.8
    plane = np.array([0.0, 0.0, 1.0, 0.0])
    data, stl = data.astype(np.float32), stl.astype(np.float32)
    assert_clear(data, dst)
    return {"xyz": data, "stl": stl, "obs_mask": obs, "bb": bb, "res": 2.5, "plane": plane}
