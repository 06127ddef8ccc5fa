#!/usr/bin/env python3
"""Times the DTU evaluation (effi_mvs_plus_amd/dtu_eval.py) on a synthetic scan of the workload's size: about 20 M fused points on a
noisy surface (a reduction factor of 5-10 at dst = 0.2) against 2.5 M ground-truth points, phase by phase: cell keys + sort, the
thinning with its rounds, the two capped nearest-neighbour passes (for several grid cells), masks and statistics; then
``point_compare`` as a whole.

There is no earlier implementation to time against.  The comparison (--cpu) is the CPU restatement of the MATLAB files on the same
box: scipy.spatial.cKDTree with ``workers`` threads -- for the thinning on a crop of --cpu-reduce-points points at the full density
(range search by the tree, then the sequential loop of reducePts_haa.m:24-30 in Python, which is its cost), for the two
nearest-neighbour passes at full size.  Where both sides ran, their results are compared (kept set on the crop, distances).

Results go to --out (default out/dtu_eval.txt) and to stdout.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DST, MAX_DIST = 0.2, 60.0


def surface(x, y):
    return 5.0 * np.sin(x / 40.0) * np.cos(y / 55.0)


def make_scan(n_data, n_stl, side, noise, seed):
    g = np.random.default_rng(seed)
    x, y = g.uniform(0, side, n_data).astype(np.float32), g.uniform(0, side, n_data).astype(np.float32)
    z = (surface(x, y) + g.normal(0, noise, n_data)).astype(np.float32)
    k = n_data // 100                                             # 1 % outliers up to 30 off the surface
    z[:k] += g.uniform(-30, 30, k).astype(np.float32)
    data = np.stack([x, y, z], -1)
    m = int(np.ceil(np.sqrt(n_stl)))                              # ground truth: a jittered grid of about n_stl points
    gx, gy = np.meshgrid((np.arange(m) + 0.5) * side / m, (np.arange(m) + 0.5) * side / m, indexing="ij")
    sx = (gx.ravel() + g.uniform(-0.2, 0.2, m * m) * side / m).astype(np.float32)
    sy = (gy.ravel() + g.uniform(-0.2, 0.2, m * m) * side / m).astype(np.float32)
    stl = np.stack([sx, sy, surface(sx, sy).astype(np.float32)], -1)
    bb = np.array([[-10.0, -10.0, -40.0], [side + 10.0, side + 10.0, 40.0]])
    obs = np.ones((200, 200, 200), bool)
    obs[:, :, :20] = False
    return data, stl, obs, bb, float((side + 20.0) / 199.0), np.array([0.0, 0.0, 1.0, 2.0])


class Timer:
    def __init__(self, lines):
        self.lines = lines

    def gpu(self, name, fn, note=""):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        self.say(f"{name:<58s} {dt * 1e3:10.1f} ms  {note(out) if callable(note) else note}")
        return out, dt

    def cpu(self, name, fn, note=""):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        self.say(f"{name:<58s} {dt:10.2f} s   {note(out) if callable(note) else note}")
        return out, dt

    def say(self, line):
        print(line, flush=True)
        self.lines.append(line)


def gpu_reduce_phases(T, xyz, order, label):
    """reduce_points taken apart for its phases (same calls, same result)."""
    from effi_mvs_plus_amd import dtu_eval as E, ops
    n, dev = xyz.shape[0], xyz.device
    cell = DST * E.CELL_MARGIN
    rank = torch.empty(n, device=dev, dtype=torch.int32)
    rank[order] = torch.arange(n, device=dev, dtype=torch.int32)
    (i0, dims), _ = T.gpu(f"{label}: extent + grid", lambda: E._grid(E._extent(xyz, "xyz"), cell), lambda r: f"grid {r[1]}")
    (pts4, keys, perm), t_sort = T.gpu(f"{label}: cell keys + sort + gather", lambda: E._sorted_by_cell(xyz, cell, i0, dims, rank))
    state = [torch.zeros(n, device=dev, dtype=torch.uint8), torch.empty(n, device=dev, dtype=torch.uint8)]
    left = torch.empty(ops.dtu_reduce_blocks(n), device=dev, dtype=torch.int32)
    rounds, t_rounds = 0, 0.0
    while True:
        def one():
            ops.dtu_reduce_round(pts4, keys, dims, DST, state[0], state[1], left)
            return int(left.sum())
        und, dt = T.gpu(f"{label}: round {rounds + 1}", one, lambda u: f"{u} undecided left")
        state.reverse()
        rounds += 1
        t_rounds += dt
        if und == 0:
            break
    keep = torch.empty(n, device=dev, dtype=torch.bool)
    keep[perm] = state[0] == E.KEPT
    kept = int(keep.sum())
    T.say(f"{label}: {rounds} rounds {t_rounds * 1e3:.1f} ms, sort {t_sort * 1e3:.1f} ms; keeps {kept} of {n} (factor {n / kept:.2f})")
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000000)
    ap.add_argument("--stl", type=int, default=2500000)
    ap.add_argument("--side", type=float, default=400.0, help="edge of the square surface patch (mm)")
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cells", default="0.5,1,2,4", help="grid cells tried for the nearest-neighbour passes (besides the default)")
    ap.add_argument("--cpu", action="store_true", help="also time the cKDTree restatement")
    ap.add_argument("--cpu-reduce-points", type=int, default=1000000)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "dtu_eval.txt"))
    a = ap.parse_args()
    from effi_mvs_plus_amd import dtu_eval as E, ops

    lines = []
    T = Timer(lines)
    dev = "cuda:0"
    T.say(f"# dtu_eval bench: {a.points} fused points, {a.stl} ground-truth points, {a.side:g} mm patch, noise {a.noise}, dst {DST}, "
          f"MaxDist {MAX_DIST}; {torch.cuda.get_device_name(0)}")
    (data, stl, obs, bb, res, plane), _ = T.cpu("make the scan (host)", lambda: make_scan(a.points, a.stl, a.side, a.noise, a.seed))
    order_h = torch.randperm(len(data), generator=torch.Generator().manual_seed(0))
    xyz, stl_d, order = torch.from_numpy(data).to(dev), torch.from_numpy(stl).to(dev), order_h.to(dev)
    E.reduce_points(xyz[:100000].contiguous(), DST, seed=0)       # warm-up: library load, workspace, allocator
    torch.cuda.synchronize()

    T.say("## GPU, phase by phase")
    keep = gpu_reduce_phases(T, xyz, order, "reduce")
    q = xyz[keep]
    T.say(f"nearest neighbour: {q.shape[0]} reduced points <-> {stl_d.shape[0]} ground-truth points")
    d2 = {}
    for cell in [None] + [float(c) for c in a.cells.split(",") if c]:
        for name, (src, to) in (("data->stl", (q, stl_d)), ("stl->data", (stl_d, q))):
            out, _ = T.gpu(f"nn {name}, cell {'default' if cell is None else cell}", lambda: E.nn_dist2_capped(src, to, MAX_DIST, cell=cell),
                           lambda o: f"median d {float(o.sqrt().median()):.4f}, {int((o >= MAX_DIST ** 2).sum())} at the cap")
            if name in d2:
                assert torch.equal(out, d2[name]), "the distances depend on the cell size"
            d2[name] = out
    T.gpu("masks (ObsMask + plane)", lambda: (ops.dtu_obs_mask(q, torch.from_numpy(obs).to(dev), list(bb[0]), res),
                                              ops.dtu_above_plane(stl_d, list(plane))))
    T.gpu("statistics (2 x sort + mean)", lambda: (E._mean_median(d2["data->stl"].sqrt()), E._mean_median(d2["stl->data"].sqrt())))
    T.say("## GPU, point_compare as a whole (obs_mask upload included)")
    r, _ = T.gpu("point_compare", lambda: E.point_compare(xyz, stl_d, torch.from_numpy(obs), bb, res, plane, order=order_h),
                 lambda r: "acc %.4f / %.4f  comp %.4f / %.4f  overall %.4f  factor %.2f  rounds %d" % tuple(
                     float(r[k]) for k in ("acc_mean", "acc_median", "comp_mean", "comp_median", "overall", "downsample_factor", "rounds")))
    assert torch.equal(r["keep"], keep)

    if a.cpu:
        from scipy.spatial import cKDTree
        T.say(f"## CPU restatement (cKDTree, workers={a.workers})")
        # crop at full density: the points left of the x that holds cpu_reduce_points of them
        n_c = min(a.cpu_reduce_points, len(data))
        xcut = np.partition(data[:, 0], n_c - 1)[n_c - 1]
        crop = data[data[:, 0] <= xcut]
        order_c = torch.randperm(len(crop), generator=torch.Generator().manual_seed(1))
        p64 = crop.astype(np.float64)
        tree, t_b = T.cpu(f"reduce crop of {len(crop)}: build tree", lambda: cKDTree(p64))
        idx, t_q = T.cpu("reduce crop: range search in visiting order", lambda: tree.query_ball_point(p64[order_c.numpy()], DST, workers=a.workers))

        def loop():
            alive = np.ones(len(crop), bool)
            for k, i in enumerate(order_c.numpy()):
                if alive[i]:
                    alive[idx[k]] = False
                    alive[i] = True
            return alive
        alive, t_l = T.cpu("reduce crop: sequential loop", loop, lambda al: f"keeps {int(al.sum())}")
        crop_d = torch.from_numpy(crop).to(dev)
        (kc, rc), t_g = T.gpu("reduce crop on the GPU (reduce_points)", lambda: E.reduce_points(crop_d, DST, order=order_c))
        diff = int((kc.cpu().numpy() != alive).sum())
        T.say(f"reduce crop: CPU {t_b + t_q + t_l:.2f} s vs GPU {t_g * 1e3:.1f} ms ({rc} rounds) = {(t_b + t_q + t_l) / t_g:.0f}x; "
              f"kept sets differ in {diff} points (the tree decides d <= dst with its own rounding)")
        del idx, tree
        qh, t_cpu_nn = q.cpu().numpy().astype(np.float64), 0.0
        s64 = stl.astype(np.float64)
        for name, (src, to) in (("data->stl", (qh, s64)), ("stl->data", (s64, qh))):
            tr, tb = T.cpu(f"nn {name}: build tree over {len(to)}", lambda: cKDTree(to))
            (dd, _), tq = T.cpu(f"nn {name}: query {len(src)}", lambda: tr.query(src, k=1, distance_upper_bound=MAX_DIST, workers=a.workers))
            t_cpu_nn += tb + tq
            got = d2[name].sqrt().cpu().numpy()
            ok = np.isfinite(dd)
            T.say(f"nn {name}: max |d_gpu - d_tree| = {np.abs(got[ok] - dd[ok]).max():.3e} over {int(ok.sum())} finite, "
                  f"{int((~ok).sum())} beyond the cap on the CPU, {int((got >= MAX_DIST).sum())} on the GPU")
        T.say(f"nn passes: CPU {t_cpu_nn:.2f} s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
