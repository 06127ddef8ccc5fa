"""The inputs of the fusion bound tests, shared by tests/test_fusion_bound_host.py (CPU) and
tests/test_gpu_fusion_bounds.py, with the interval references computed once per case and kept.

Shapes: the smallest at which the forms change -- 9x13 (fewer pixels than one 256-thread workgroup), 16x32 (exactly two), 37x50 (odd,
eight workgroups with a ragged last one) and the fixture sizes 96x128 / 70x90; confidence maps at the depth size, at twice it, and at
75x101 / 47x61 (non-dyadic nearest-index ratios)."""
import functools
import math

import numpy as np
import torch

import common  # noqa: F401  (puts the repository root on sys.path)
from effi_mvs_plus_amd import synth

import fusion_bound as FB

f32 = np.float32


def _conf(shape, seed):
    return None if shape is None else torch.rand(*shape, generator=torch.Generator().manual_seed(seed + 100)).numpy()


def _roll(cams, deg):
    """Source views rotated about their optical axis and pitched a little: general rotation matrices, so that a single-precision inverse
    is not the double one rounded."""
    cams = cams.copy()
    for v in range(1, cams.shape[0]):
        a, b = math.radians(deg * v), math.radians(1.7 * v)
        Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
        Rx = np.array([[1.0, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        E = cams[v, 0].astype(np.float64)
        E[:3, :3], E[:3, 3] = Rz @ Rx @ E[:3, :3], Rz @ Rx @ E[:3, 3]
        cams[v, 0] = E.astype(f32)
    return cams


# name -> (H, W, N views, synth kwargs, rig, conf shape, prob_thr, dh (None = V), dist_base, rel_base, relative)
_TT = {
    "fixture_a":         (96, 128, 6, dict(seed=3), None, (192, 256), 0.3, 2, 4.0, 1.3, False),
    "fixture_b":         (70, 90, 11, dict(seed=5), None, (140, 180), 0.55, 3, 6.0, 400.0, True),
    "tiny_v1":           (9, 13, 2, dict(seed=11), None, None, 0.0, 1, 4.0, 0.25, False),     # 13 px across: 4 mm per pixel step
    "two_wg_v2_dh_v":    (16, 32, 3, dict(seed=12), None, (16, 32), 0.4, None, 4.0, 1300.0, True),
    "odd_v5_conf75x101": (37, 50, 6, dict(seed=13), None, (75, 101), 0.5, 1, 4.0, 1.3, False),
    "odd_n4":            (37, 50, 4, dict(seed=1), None, None, 0.0, 2, 4.0, 1.3, False),
    "v10_conf47x61":     (70, 90, 11, dict(seed=14), None, (47, 61), 0.45, 2, 4.0, 1300.0, True),
    "consistent_v16":    (40, 56, 17, dict(seed=9, noise_mm=0.0, outlier_frac=0.0), "outside", None, 0.0, 2, 4.0, 1.3, False),
    "consistent_dh_v":   (16, 32, 6, dict(seed=15, noise_mm=0.0, outlier_frac=0.0), None, None, 0.0, None, 4.0, 1.3, False),
    "border_v5":         (37, 50, 6, dict(seed=16), "border", (74, 100), 0.3, 2, 4.0, 1.3, False),
    "inside_v5":         (37, 50, 6, dict(seed=17), "inside", None, 0.0, 2, 4.0, 1300.0, True),
    "rolled_v5":         (37, 50, 6, dict(seed=18), "rolled", None, 0.0, 2, 4.0, 1300.0, True),
}
TT_CASES = list(_TT)


@functools.lru_cache(maxsize=None)
def tt_case(name):
    H, W, N, kw, rig, cshape, prob, dh, dist, rel, relative = _TT[name]
    d, cams = synth.synth_depth_maps(H, W, N, **kw)
    d, cams = d.numpy(), cams.numpy().copy()
    if rig == "outside":
        cams[3, 0, 0, 3] += 4000.0                       # source view 3 shifted far sideways: every sample falls outside
    elif rig == "border":
        cams[2, 0, 0, 3] += 376.0                        # ~25 px: half of the samples of source view 2 fall off the image
        cams[4, 0, 1, 3] -= 300.0                        # ~20 px upwards for source view 4
    elif rig == "inside":
        cams[2, 0, 2, 3] -= 680.0                        # source camera moved into the scene: Z <= 0 for about half of the pixels
        d[0, 0, 3:6] = 0.0                               # and three reference depths of 0: the relative difference divides by them
    elif rig == "rolled":
        cams = _roll(cams, 7.0)
    if name.startswith("fixture"):
        conf = torch.rand(1, *cshape, generator=torch.Generator().manual_seed(kw["seed"] + 100))[0].numpy()     # as tests/test_fusion.py
    else:
        conf = _conf(cshape, kw["seed"])
    return dict(name=name, ref_depth=d[0], src_depths=d[1:], ref_cam=cams[0], src_cams=cams[1:], conf=conf, prob_thr=prob,
                dh=(N - 1 if dh is None else dh), dist_base=dist, rel_base=rel, relative=relative)


def tt_args(c):
    return (c["ref_depth"], c["src_depths"], c["ref_cam"], c["src_cams"], c["conf"], c["prob_thr"], c["dh"], c["dist_base"], c["rel_base"],
            c["relative"])


@functools.lru_cache(maxsize=None)
def tt_ref(name):
    return FB.tt_reference(*tt_args(tt_case(name)))


@functools.lru_cache(maxsize=None)
def tt_restated(name):
    return FB.tt_restate(*tt_args(tt_case(name)))


# a scan whose table rows have different source counts (the table row is blockIdx.y of the scan launch)
TT_SCAN = dict(H=16, W=32, N=6, seed=21, rows=[(0, [1, 2, 3]), (1, [0, 2]), (4, [0, 1, 2, 3, 5]), (2, [3, 1])], dh=2, dist_base=4.0,
               rel_base=1.3, relative=False, prob_thr=0.35)


@functools.lru_cache(maxsize=None)
def tt_scan():
    c = dict(TT_SCAN)
    d, cams = synth.synth_depth_maps(c["H"], c["W"], c["N"], seed=c["seed"])
    c["depths"], c["cams"] = d.numpy(), cams.numpy()
    c["conf"] = torch.rand(len(c["rows"]), 2 * c["H"], 2 * c["W"], generator=torch.Generator().manual_seed(5)).numpy()
    return c


def tt_scan_row(c, r, shift=0):
    """The arguments of tt_reference / tt_restate for row r of the scan; shift: the mutant that reads the source ids one slot early
    (row[s] for row[1 + s]: the reference view itself comes first, the last source is never read)."""
    ref, srcs = c["rows"][r]
    srcs = ([ref] + srcs)[:len(srcs)] if shift else srcs
    return (c["depths"][ref], c["depths"][srcs], c["cams"][ref], c["cams"][srcs], c["conf"][r], c["prob_thr"], c["dh"], c["dist_base"],
            c["rel_base"], c["relative"])


@functools.lru_cache(maxsize=None)
def tt_scan_ref(r):
    return FB.tt_reference(*tt_scan_row(tt_scan(), r))


# planted ties of fusion_vis_filter_kernel: dist_base = 4 and rel_base a power of two make the thresholds and the planted values exact
def vis_ties(relative):
    """ref_depth [h,w], xyd [V,3,h,w] with, per pixel, dx = step / 4 exactly (dy = 0: sqrtf exact) or one ulp below, and
    ddiff = step / rel_base exactly or one ulp below, cycling over the thresholds.  relative: ref_depth is a power of two, so the
    quotient is exact."""
    h, w, V, thres, dist_base, rel_base = 9, 13, 5, 2, 4.0, (16.0 if relative else 8.0)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, v = xs.astype(f32) + f32(0.5), ys.astype(f32) + f32(0.5)
    ref_depth = np.full((h, w), 512.0, f32)
    xyd = np.zeros((V, 3, h, w), f32)
    p = ys * w + xs
    for s in range(V):
        step = (thres + (p + s) % (V + 1 - thres)).astype(f32)
        kind = (p // 4 + s) % 4                             # 0: both at the tie, 1: dx one ulp below, 2: ddiff one ulp below, 3: both below
        dx = step / f32(dist_base)
        dd = step / f32(rel_base) * (f32(512.0) if relative else f32(1.0))
        x, d = u + dx, ref_depth - dd
        assert np.array_equal(x.astype(np.float64), u.astype(np.float64) + dx) and np.array_equal(d.astype(np.float64), 512.0 - dd.astype(np.float64))
        x = np.where((kind == 1) | (kind == 3), np.nextafter(x, f32(0)), x)             # one ulp of the stored coordinate below the tie
        d = np.where((kind == 2) | (kind == 3), np.nextafter(d, f32(1024)), d)
        xyd[s, 0], xyd[s, 1], xyd[s, 2] = x, v, d
        # the kernel's two subtractions are exact on these values (neighbouring fp32 numbers): the tie is met or missed by one ulp
        assert np.array_equal((x - u).astype(np.float64), x.astype(np.float64) - u) and np.array_equal((ref_depth - d).astype(np.float64), 512.0 - d.astype(np.float64))
    return dict(ref_depth=ref_depth, xyd=xyd, dist_base=dist_base, rel_base=rel_base, thres=thres, relative=relative)


# ---- DTU ----
# name -> (H, W, N, seed, noise_mm, rig, with confidence, s, e)
_DTU = {
    "tiny_n2":        (9, 13, 2, 1, 0.03, None, True, 1, 11),
    "odd_n3_loose":   (37, 50, 3, 2, 0.4, None, True, 1, 11),
    "odd_n3_short":   (37, 50, 3, 4, 0.03, None, False, 2, 6),
    "n5_tight":       (75, 101, 5, 5, 0.03, None, True, 1, 11),
    "n11_loose":      (96, 128, 11, 3, 0.4, None, True, 1, 11),
    "rolled_n3":      (37, 50, 3, 6, 0.03, "rolled", True, 1, 11),
}
DTU_CASES = list(_DTU)


@functools.lru_cache(maxsize=None)
def dtu_case(name):
    H, W, N, seed, noise, rig, with_conf, s, e = _DTU[name]
    d, cams = synth.synth_depth_maps(H, W, N, seed=seed, noise_mm=noise, outlier_frac=0.08, pixel_center=0.0)
    d, cams = d.numpy(), cams.numpy().copy()
    if rig == "rolled":
        cams = _roll(cams, 5.0)
    conf = torch.rand(H, W, generator=torch.Generator().manual_seed(seed + 7)).numpy() if with_conf else None
    return dict(name=name, ref_depth=d[0], src_depths=d[1:], ref_cam=cams[0], src_cams=cams[1:], conf=conf, conf_thr=0.5, conf_keep=0.75,
                s=s, e=e, dist_base=0.5, diff_base=0.25)


def dtu_args(c):
    return (c["ref_depth"], c["src_depths"], c["ref_cam"], c["src_cams"], c["conf"], c["conf_thr"], c["conf_keep"], c["s"], c["e"],
            c["dist_base"], c["diff_base"])


@functools.lru_cache(maxsize=None)
def dtu_ref(name):
    return FB.dtu_reference(*dtu_args(dtu_case(name)))


@functools.lru_cache(maxsize=None)
def dtu_restated(name):
    return FB.dtu_restate(*dtu_args(dtu_case(name)))


DTU_SCAN = dict(H=9, W=13, N=5, seed=31, rows=[(0, [1, 2]), (3, [0, 1, 2, 4]), (1, [4])], s=1, e=11)


@functools.lru_cache(maxsize=None)
def dtu_scan():
    c = dict(DTU_SCAN)
    d, cams = synth.synth_depth_maps(c["H"], c["W"], c["N"], seed=c["seed"], noise_mm=0.03, outlier_frac=0.08, pixel_center=0.0)
    c["depths"], c["cams"] = d.numpy(), cams.numpy()
    c["conf"] = torch.rand(len(c["rows"]), c["H"], c["W"], generator=torch.Generator().manual_seed(6)).numpy()
    return c


def dtu_scan_row(c, r):
    ref, srcs = c["rows"][r]
    return (c["depths"][ref], c["depths"][srcs], c["cams"][ref], c["cams"][srcs], c["conf"][r], 0.5, 0.75, c["s"], c["e"], 0.5, 0.25)


@functools.lru_cache(maxsize=None)
def dtu_scan_ref(r):
    return FB.dtu_reference(*dtu_scan_row(dtu_scan(), r))


def vis_ties_expected(t):
    """The exact masks of the planted ties: every difference and quotient is exact on these values, so float64 gives the true answer."""
    rd, xyd = t["ref_depth"].astype(np.float64), t["xyd"].astype(np.float64)
    V, _, h, w = xyd.shape
    u = np.arange(w, dtype=np.float64)[None, :] + 0.5
    nthr = V + 1 - t["thres"]
    out = np.zeros((V, nthr, h, w), bool)
    for s in range(V):
        cdiff, ddiff = np.abs(xyd[s, 0] - u), np.abs(rd - xyd[s, 2])
        if t["relative"]:
            ddiff = ddiff / rd
        for k in range(nthr):
            out[s, k] = (cdiff < (t["thres"] + k) / t["dist_base"]) & (ddiff < (t["thres"] + k) / t["rel_base"])
    return out


def points_inputs(name):
    """(mode, pts [n, 3 or 4] fp32, cam [2,4,4], depth [n] or None) for ops.fusion_points' four modes, chained: each mode's input is the
    fp32 restatement of the one before, on the case's reference camera and first source camera."""
    c = tt_case(name)
    h, w = c["ref_depth"].shape
    ys, xs = FB.pixel_grid(h, w)
    grid = np.stack([xs + 0.5, ys + 0.5, np.ones(h * w)], 1).astype(f32)
    n = h * w
    full = lambda comps: np.stack([np.broadcast_to(np.asarray(x, f32), (n,)) for x in comps], 1).copy()      # noqa: E731
    with np.errstate(all="ignore"):
        cam_pt = full(FB.points_chain(FB.F32, 0, grid, c["ref_cam"], c["ref_depth"].reshape(-1)))
        world = full(FB.points_chain(FB.F32, 1, cam_pt, c["ref_cam"]))
        src_pt = full(FB.points_chain(FB.F32, 2, world, c["src_cams"][0]))
    return [(0, grid, c["ref_cam"], c["ref_depth"].reshape(-1)), (1, cam_pt, c["ref_cam"], None), (2, world, c["src_cams"][0], None),
            (3, src_pt, c["src_cams"][0], None)]
