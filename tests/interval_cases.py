"""Seeded inputs shared by the interval tests on the CPU (test_interval_ref_host.py: the fp32 oracle stands in for the kernels and
the shares of live / in-range / two-valued elements are checked) and on the GPU (test_gpu_intervals.py)."""
import torch

from common import _edge_cameras
from effi_mvs_plus_amd import synth

RIGS = ["rig", "rolled", "wide", "inside", "far"]
STAGE1_SHAPES = [(37, 50, 48, 4), (16, 20, 8, 3), (9, 13, 6, 2), (20, 24, 1, 2)]       # partial 16x8 tiles, maps below one tile, D % 4 != 0


def stage1_case(kind, h, w, D, N, C=32):
    """-> feats (list of [C,h,w]), projection pairs [1,N,2,4,4], shared hypotheses [D] (the inputs of test_warpcorr_views_window_kernel)."""
    feats = [f[0] for f in synth.smooth_features(N, C, h, w, seed=300 + h)]
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"] if kind == "rig" else _edge_cameras(h, w, N, kind)
    samples = (1.0 / torch.linspace(1 / 935.0, 1 / 425.0, D)) if D > 1 else torch.tensor([600.0])
    return feats, pm, samples


def dense_grad(S, D, h, w, seed=0):
    """Upstream gradient of the similarities, dense Gaussian [S,D,h,w]."""
    return torch.randn(S, D, h, w, generator=torch.Generator().manual_seed(4000 + 10 * h + D + seed))


def seam_lattice(h, w):
    """Rows / columns on both sides of every 16 x 8 tile seam: set a = the last row / column of every tile (y = 7, 15, ..; x = 15, 31,
    ..) with the first and last of the map (its four corners), set b = the first of every tile but the first (y = 8, 16, ..; x = 16,
    32, ..) -> (ya, xa), (yb, xb).  Inside a set no two rows / columns are adjacent."""
    xa = sorted({0, w - 1} | set(range(15, w, 16)))
    ya = sorted({0, h - 1} | set(range(7, h, 8)))
    return (ya, xa), (list(range(8, h, 8)), list(range(16, w, 16)))


def sparse_grad(S, D, h, w, seed=0):
    """Upstream gradient [S,D,h,w] that is non-zero only at hypotheses {0, D - 1}, on a lattice of isolated pixels: plane 0 carries
    rows a x columns a of `seam_lattice` (the map's corners among them), plane D - 1 rows b x columns b, values of either sign with
    0.5 <= |g| < 1.5.  A stray add to a wrong pixel, view or (padded) hypothesis lands where the reference pins an exact 0."""
    g = torch.Generator().manual_seed(4100 + h + D + seed)
    G = torch.zeros(S, D, h, w)
    val = 0.5 + torch.rand(S, D, h, w, generator=g)
    val = val * (1.0 - 2.0 * (torch.rand(S, D, h, w, generator=g) < 0.5).float())
    for d, (ys, xs) in zip((0, D - 1), seam_lattice(h, w)):
        iy, ix = torch.meshgrid(torch.tensor(ys), torch.tensor(xs), indexing="ij")
        G[:, d, iy, ix] = val[:, d, iy, ix]
    return G


def lookup_bwd_case(Dp, nq, h, w, per_pixel, twice, seed=0):
    """`lookup_case` with an upstream gradient [nq,h,w]; twice: the query map at twice the volume's resolution, [nq,2h+1,2w+1] (odd:
    the last row / column is never read), the case's queries on its even pixels and another valid depth everywhere else, so that a
    read of the wrong pixel shows."""
    vol, q, dmin, dmax = lookup_case(Dp, nq, h, w, per_pixel, seed)
    g = torch.Generator().manual_seed(4200 + Dp + nq + h + seed)
    gout = torch.randn(nq, h, w, generator=g)
    if twice:
        q2 = 425.0 + 510.0 * torch.rand(nq, 2 * h + 1, 2 * w + 1, generator=g)
        q2[:, 0:2 * h:2, 0:2 * w:2] = q
        q = q2.contiguous()
    return vol, q, dmin, dmax, gout


def dyn_cameras(h, w, N, kind):
    """The stage-3 ring of cameras with the intrinsics set for an h x w map (test_warpcorr_dyn_window_form_is_bitwise_the_gather_form),
    and the edge rigs built on it like `_edge_cameras`: `rolled` = sources rotated about the optical axis, `inside` = a source camera
    moved into the depth range."""
    import math
    pm = synth.synth_cameras(8 * h, 8 * w, N)["stage3"][0].clone()
    pm[:, 1, 0, 0] = pm[:, 1, 1, 1] = 1.1 * w
    pm[:, 1, 0, 2], pm[:, 1, 1, 2] = w / 2.0, h / 2.0
    for v in range(1, N):
        E = pm[v, 0]
        if kind == "rolled":
            a = math.radians(25.0 * v)
            Rz = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
            E[:3, :3] = Rz @ E[:3, :3]
            E[:3, 3] = Rz @ E[:3, 3]
        elif kind == "inside":
            E[2, 3] = E[2, 3] - 600.0 - 40.0 * v
    return pm


def dyn_depth(h, w, name):
    """`smooth` and `noisy` of test_warpcorr_dyn_window_form_is_bitwise_the_gather_form; `clamps`: pixels whose inverse depth -+ half
    the range (interval 2e-5) meets the clamps of get_cur_depth_range_samples: 1e-4 below, 1e4 above (the 1e-5 clamp of the single
    hypothesis cannot bind once both ends are >= 1e-4; it is evaluated all the same)."""
    g = torch.Generator().manual_seed(5)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    smooth = 600.0 + 40.0 * torch.sin(xs / 17.0) + 30.0 * torch.cos(ys / 11.0)
    if name == "smooth":
        return smooth
    noisy = smooth + 25.0 * torch.randn(h, w, generator=g)
    noisy[h // 3: h // 3 + 5, :] = 430.0
    noisy[:, w // 2] = 930.0
    if name == "noisy":
        return noisy
    assert name == "clamps"
    cur = smooth.clone()
    cur[0::4, 1::3] = 9000.0           # 1/cur - half < 1e-4: the lower end sits on the clamp
    cur[1::4, 2::3] = 2.0e4            # 1/cur < 1e-4 itself
    cur[2::4, 0::3] = 5.0e-5           # 1/cur = 2e4 > 1e4: the upper end sits on its clamp BELOW the lower one, a negative step
    cur[3::4, 1::3] = 1.5e5            # both ends on 1e-4: step 0
    return cur


def softmax_logits(D, h, w, seed=9):
    """Four kinds of logits in column stripes (x % 4): 0 = 2 randn; 1 = all the mass on plane 0 (even rows) or D - 1 (odd rows), the
    padded window at both ends; 2 = two equal peaks at k - 1 and k + 1 over an exact background, so that idxf sits on the integer k to
    rounding (D < 3: the mass on plane D - 1); 3 = a spread of +-80, where the maximum subtraction matters."""
    g = torch.Generator().manual_seed(seed + D)
    out = torch.empty(D, h, w)
    out[:, :, 0::4] = (2.0 * torch.randn(D, h, w, generator=g))[:, :, 0::4]
    one = 0.5 * torch.randn(D, h, w, generator=g)
    one[0, 0::2] += 40.0
    one[D - 1, 1::2] += 40.0
    out[:, :, 1::4] = one[:, :, 1::4]
    if D >= 3:
        two = torch.full((D, h, w), -30.0)
        k = torch.randint(1, D - 1, (h, w), generator=g)
        two.scatter_(0, (k - 1).unsqueeze(0), 0.0)
        two.scatter_(0, (k + 1).unsqueeze(0), 0.0)
    else:
        two = torch.zeros(D, h, w)
        two[D - 1] += 40.0
    out[:, :, 2::4] = two[:, :, 2::4]
    out[:, :, 3::4] = (80.0 * (2.0 * torch.rand(D, h, w, generator=g) - 1.0))[:, :, 3::4]
    return out


def lookup_case(Dp, nq, h, w, per_pixel, seed=0):
    """vol [Dp,h,w], query depths [nq,h,w], dmin / dmax (one value each, or [h,w] maps): inverse depths uniform over
    [-0.25, 1.25] of the range, a sixth of them far outside ([-0.8, -0.5] and [2, 2.5] of it: the value is exactly 0 there), and queries
    exactly AT dmin / dmax (positions Dp - 1 and 0)."""
    g = torch.Generator().manual_seed(1000 * Dp + 10 * nq + h + seed)
    vol = torch.randn(Dp, h, w, generator=g)
    if per_pixel:
        dmin = 425.0 * (1.0 + 0.1 * torch.rand(h, w, generator=g))
        dmax = 935.0 * (1.0 + 0.1 * torch.rand(h, w, generator=g))
    else:
        dmin, dmax = torch.tensor([425.0]), torch.tensor([935.0])
    r = -0.25 + 1.5 * torch.rand(nq, h, w, generator=g)
    far = torch.rand(nq, h, w, generator=g)
    r = torch.where(far < 1 / 12, -0.8 + 0.3 * torch.rand(nq, h, w, generator=g), r)
    r = torch.where(far > 11 / 12, 2.0 + 0.5 * torch.rand(nq, h, w, generator=g), r)
    inv = 1.0 / dmax + (1.0 / dmin - 1.0 / dmax) * r
    q = 1.0 / inv
    lo, hi = dmin.expand(h, w), dmax.expand(h, w)
    q[0, 0::3, 0::2] = lo[0::3, 0::2]
    q[nq - 1, 1::3, 1::2] = hi[1::3, 1::2]
    return vol, q.contiguous(), dmin, dmax


def getcost_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth, seed=0):
    """Two volumes, a map of normalised inverse depth (or depth) whose nq hypotheses reach beyond both ends of the volumes' range,
    the stage's inverse-depth range and interval (half range <= a quarter of the smallest inverse depth: see GETCOST_ROUNDINGS)."""
    g = torch.Generator().manual_seed(77 * Dcur + Dreg + nq + h + seed)
    cur, reg = torch.randn(Dcur, h, w, generator=g), torch.randn(Dreg, h, w, generator=g)
    disp_range = torch.linspace(1 / 935.0, 1 / 425.0, 48)
    x = torch.rand(h, w, generator=g)                                   # normalised inverse depth over the whole range of the stage
    interval = torch.tensor([8.0e-5])
    if per_pixel:                                                       # the volumes cover a part of it: queries leave at both ends
        dmin = 470.0 * (1.0 + 0.1 * torch.rand(h, w, generator=g))
        dmax = 800.0 * (1.0 + 0.1 * torch.rand(h, w, generator=g))
    else:
        dmin, dmax = torch.tensor([470.0]), torch.tensor([800.0])
    if input_is_depth:
        x = 1.0 / (disp_range[0] + (disp_range[-1] - disp_range[0]) * x)
    return cur, reg, x.contiguous(), disp_range, interval, dmin, dmax
