"""The cases of the Gipuma fusion tests, as numpy arrays: the smallest shapes at which the kernel can go
wrong -- 37x53 (not a multiple of the 256-pixel workgroup, several workgroups) and 7x9 (less than one wave).  ``case(name)`` ->
dict(depths [n,h,w], cams [n,2,4,4], images [n,h,w,3], conf [n,h,w] or None, pair_data or None, prob_thr, thr, num, exact) with
``exact`` one of None (decisions by float64 intervals), "all" (every operation of the chain is exact in fp32: the float64 value IS
the fp32 result, nothing is undecided, everything is compared bitwise) or "decisions" (the decisions are exact, the averages are not).
"""
import functools

import numpy as np
import torch

from effi_mvs_plus_amd import synth

f32 = np.float32
PAIRS = [(0, [1, 2]), (1, [0, 2, 3]), (2, [0, 1, 3, 4, 5]), (3, [5, 4, 2, 1]), (5, [4, 3])]      # tests/test_gpu_fusion_scan.py's
DEPTH_MIN, DEPTH_MAX = f32(0.001), f32(100000.0)


def _cams(centres, f, cx, cy):
    cams = np.zeros((len(centres), 2, 4, 4), f32)
    for v, c in enumerate(centres):
        cams[v, 0] = np.eye(4, dtype=f32)
        cams[v, 0, :3, 3] = -np.asarray(c, f32)
        cams[v, 1, :3, :3] = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    return cams


def _blocks(rng, h, w, values, weights, size=4):
    b = rng.choice(np.asarray(values, f32), size=((h + size - 1) // size, (w + size - 1) // size), p=weights)
    return np.kron(b, np.ones((size, size), f32))[:h, :w].astype(f32)


def exact_rig(h, w, values, weights, n=6, seed=0):
    """R = I, C_v = (4 v, 0, 0), f = 64, integer principal point, depths from ``values`` per 4x4 block and view: every projection is
    an integer (64 * 4 k / d for d a power of two up to 256) and every disparity f b / d a dyadic number."""
    rng = np.random.default_rng(seed)
    depths = np.stack([_blocks(rng, h, w, values, weights) for _ in range(n)])
    images = rng.random((n, h, w, 3), dtype=f32)
    return dict(depths=depths, cams=_cams([(4.0 * v, 0, 0) for v in range(n)], 64.0, w // 2, h // 2), images=images)


def near_rig(h, w, n, seed=0):
    """R = I, C_v = (v 2^-16, 0, 0), f = 64: the views all but coincide, so that depths at the ends of [depth_min, depth_max] still
    project inside a small image (64 * 2^-16 / 0.001 = 0.98 pixels per camera step at depth_min)."""
    rng = np.random.default_rng(seed)
    depths = np.ones((n, h, w), f32)
    return dict(depths=depths, cams=_cams([(v * 2.0 ** -16, 0, 0) for v in range(n)], 64.0, w // 2, h // 2),
                images=rng.random((n, h, w, 3), dtype=f32))


def general(h, w, noise_mm, n=6, seed=3):
    d, cams = synth.synth_depth_maps(h, w, n, seed=seed, noise_mm=noise_mm, outlier_frac=0.08, pixel_center=0.0)
    g = torch.Generator().manual_seed(seed + 7)
    conf = torch.rand(n, h, w, generator=g).numpy()
    images = torch.rand(n, h, w, 3, generator=g).numpy()
    d = d.numpy().copy()
    d[1::2, h // 4:h // 4 + 3, w // 3:w // 3 + 5] = 0.0               # a block of zero depths in every second view
    return dict(depths=d.astype(f32), cams=cams.numpy().astype(f32), images=images.astype(f32), conf=conf.astype(f32))


def _reversed_rows(n):
    return [(r, [s for s in range(n) if s != r]) for r in reversed(range(n))]


def _depth_edges():
    c = near_rig(9, 12, 3, seed=5)
    d = c["depths"]
    d[:, :, 0:4] = DEPTH_MIN
    d[:, :, 8:12] = DEPTH_MAX
    d[:, 2, 0:4] = np.nextafter(DEPTH_MIN, f32(0))                    # just outside: never live, never a consistent source
    d[:, 6, 8:12] = np.nextafter(DEPTH_MAX, f32(np.inf))
    d[1, 4, :] = np.nan
    return dict(c, thr=0.25, num=2)


def _full64():
    c = near_rig(5, 8, 65, seed=6)
    c["depths"][64, 1, 2:5] = 0.0                                     # the LAST source (bit 63 of the mask) fails on three pixels
    c["depths"][0, 3, 1] = 0.0
    return dict(c, pair_data=[(0, list(range(1, 65)))], thr=0.25, num=64)


_BUILD = {
    "exact_37x53": lambda: dict(exact_rig(37, 53, (0, 32, 64, 128), (0.1, 0.3, 0.3, 0.3)), thr=0.25, num=2, exact="all"),
    "exact_7x9": lambda: dict(exact_rig(7, 9, (0, 128, 256), (0.1, 0.45, 0.45), seed=1), thr=0.25, num=2, exact="all"),
    "exact_reversed": lambda: dict(exact_rig(37, 53, (0, 32, 64, 128), (0.1, 0.3, 0.3, 0.3)), thr=0.25, num=2, exact="all",
                                   pair_data=_reversed_rows(6)),
    # |f b / z - f b / d_s| = 2 exactly for neighbouring views at depths 128 and 64: `<` against `<=` at the threshold
    "exact_edge": lambda: dict(exact_rig(37, 53, (0, 32, 64, 128), (0.1, 0.3, 0.3, 0.3)), thr=2.0, num=2, exact="decisions"),
    "general_37x53": lambda: dict(general(37, 53, 0.4), thr=0.02, num=3, conf=None),
    "general_lownoise": lambda: dict(general(37, 53, 0.03), thr=0.25, num=3, conf=None),
    "general_7x9": lambda: dict(general(7, 9, 0.4), thr=0.02, num=3, conf=None),
    "pairs": lambda: dict(general(37, 53, 0.4), thr=0.02, num=2, conf=None, pair_data=PAIRS),
    "prob": lambda: dict(general(37, 53, 0.4), thr=0.02, num=3, prob_thr=0.3),
    "too_many_needed": lambda: dict(exact_rig(7, 9, (0, 128, 256), (0.1, 0.45, 0.45), seed=1), thr=0.25, num=6, exact="all"),
    "depth_edges": _depth_edges,
    "full64": _full64,
}
CASES = tuple(_BUILD)
# cases whose cloud may (must) be empty or whose masks are full by construction
EMPTY = ("too_many_needed",)


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(conf=None, pair_data=None, prob_thr=0.5, exact=None)
    c.update(_BUILD[name]())
    c["name"] = name
    for k in ("depths", "cams", "images", "conf"):
        if c[k] is not None:
            c[k] = np.ascontiguousarray(c[k], f32)
            c[k].setflags(write=False)
    return c


def rows_of(c):
    n = c["depths"].shape[0]
    pd = c["pair_data"]
    return [(r, [s for s in range(n) if s != r]) for r in range(n)] if pd is None else [(int(r), [int(s) for s in ss]) for r, ss in pd]
