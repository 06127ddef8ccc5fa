"""CPU: the interval reference of the scatter gradients (tests/scatter_ref.py) has teeth.  Torch fp32 autograd through the oracle's
warp_grid + grid_sample (and its explicit 1-D look-up) stands in for the backward kernels: every element of it lies inside its
interval with nothing left out, and mutants of it -- the defects the outlier fraction of the autograd parity tests lets through --
leave elements outside.  Each mutant prints how many ([mutant] lines: the table of DESIGN.md section 2.3).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import interval_cases as cases
import interval_ref as IR
import scatter_ref as SR
from common import check_close
from effi_mvs_plus_amd import synth
from oracle import effi_oracle as O


def _rel(pm):
    """Projection pairs [1,N,2,4,4] -> per source view (rot [1,3,3], trans [1,3,1], the twelve values)."""
    P = [O.compose_projection(pm[:, v]) for v in range(pm.shape[1])]
    out = []
    for v in range(1, len(P)):
        rot, trans = O.relative_projection(P[v], P[0])
        out.append((rot, trans, torch.cat([rot.reshape(-1), trans.reshape(-1)])))
    return out


def _sim(ref, src, rot, trans, depth, shift_px=0.0):
    """The fp32 oracle's similarity of one view [D,h,w], differentiable in ref and src (the grid carries no gradient)."""
    C, h, w = ref.shape
    D = depth.shape[0]
    dv = depth.reshape(1, D, 1, 1).expand(1, D, h, w) if depth.dim() == 1 else depth.unsqueeze(0)
    grid = O.warp_grid(rot, trans, dv, h, w).detach().clone()
    grid[..., 0] += shift_px * 2.0 / (w - 1)
    warped = F.grid_sample(src.unsqueeze(0), grid.view(1, D * h, w, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
    return (warped.view(1, C, D, h, w) * ref.view(1, C, 1, h, w)).mean(1)[0]


def _band(rot, trans, depth, h, w):
    """[D,h,w]: the sample's only tap column inside the image is a border one (ix in (-1, 0) or (W-1, W)): `drop_band` of the forward."""
    D = depth.shape[0]
    grid = O.warp_grid(rot, trans, depth.reshape(1, D, 1, 1).expand(1, D, h, w), h, w)
    ix = ((grid[..., 0] + 1) / 2 * (w - 1)).view(D, h, w)
    return ((ix > -1) & (ix < 0)) | ((ix > w - 1) & (ix < w))


def _stage1_bwd(feats, rel, samples, G, shift_px=0.0):
    """-> (grad_ref [h,w,C], [grad_src_v [h,w,C]]) by fp32 autograd."""
    leaves = [f.clone().requires_grad_(True) for f in feats]
    sims = torch.stack([_sim(leaves[0], leaves[v + 1], rel[v][0], rel[v][1], samples, shift_px) for v in range(len(rel))])
    (sims * G).sum().backward()
    return leaves[0].grad.permute(1, 2, 0).contiguous(), [l_.grad.permute(1, 2, 0).contiguous() for l_ in leaves[1:]]


@pytest.fixture(scope="module")
def stage1():
    """(rig, shape) -> inputs, the stand-in's gradients and the intervals, built on first use and kept."""
    cache = {}

    def get(kind, h, w, D, N):
        key = (kind, h, w, D, N)
        if key not in cache:
            feats, pm, samples = cases.stage1_case(kind, h, w, D, N)
            rel = _rel(pm)
            G = cases.dense_grad(N - 1, D, h, w)
            g_ref, g_src = _stage1_bwd(feats, rel, samples, G)
            iv_ref, iv_src = SR.stage1_bwd_intervals(feats, torch.stack([r[2] for r in rel]), samples, G)
            cache[key] = dict(feats=feats, rel=rel, samples=samples, G=G, g_ref=g_ref, g_src=g_src, iv_ref=iv_ref, iv_src=iv_src)
        return cache[key]
    return get


def _outside(name, got, iv):
    """How many elements of `got` are outside their interval or non-zero where they must be 0; prints the [mutant] line."""
    g = got.detach().double()
    bad = ~((g >= iv.lo - iv.tol) & (g <= iv.hi + iv.tol)) | (iv.must_be_zero & (g != 0))
    n = int(bad.sum())
    print(f"[mutant] {name:60s} outside={n} of {g.numel()}")
    with pytest.raises(AssertionError, match="outside their interval|must be exactly 0"):
        IR.check_inside(name, got, **iv.args())
    return n


# ---------------------------------------------------------------------------------------------
# stage 1: the stand-in inside every interval
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.RIGS)
@pytest.mark.parametrize("h,w,D,N", cases.STAGE1_SHAPES)
def test_stage1_autograd_lies_inside_every_interval(stage1, kind, h, w, D, N):
    c = stage1(kind, h, w, D, N)
    tag = f"[{kind} {h}x{w} D={D}]"
    s = IR.check_inside(f"autograd grad_ref {tag}", c["g_ref"], **c["iv_ref"].args(), max_left_out=0.0)
    live = [s["live"]]
    for v in range(N - 1):
        s = IR.check_inside(f"autograd grad_src{v} {tag}", c["g_src"][v], **c["iv_src"][v].args(), max_left_out=0.0)
        live.append(s["live"])
        peak = float(c["iv_src"][v].mag.max())
        print(f"[interval] widest + tol / peak {tag} view {v}: "
              f"{float((c['iv_src'][v].hi - c['iv_src'][v].lo + 2 * c['iv_src'][v].tol).max()) / max(peak, 1e-300):.3e}")
        if kind == "far":
            assert s["must_be_zero"] == s["elements"] and not c["g_src"][v].any(), "the view that looks away receives nothing"
    if kind == "far":
        assert not c["g_ref"].any()
    elif not (kind == "inside" and D == 1):
        # the forward test's rule, on grad_ref and on the source views taken together (the third view of `wide` sees nothing)
        assert live[0] >= 0.05 and sum(live[1:]) / (N - 1) >= 0.05, f"{kind}: live shares {live}"


# ---------------------------------------------------------------------------------------------
# stage 1: mutants
# ---------------------------------------------------------------------------------------------
def _without(c, mask):
    """The stand-in with the contributions of `mask` [S,D,h,w] dropped (the gradients are linear in G)."""
    return _stage1_bwd(c["feats"], c["rel"], c["samples"], c["G"] * (~mask))


def _one_contribution(c, v):
    """(d, y, x) of the contribution to drop: among the samples of view v that land inside the source image with |G| >= 1, the one
    nearest to a lattice pixel, whose weight sits on one tap (32 channels of one pixel carry nearly all of it).  (The contribution
    with the largest |G| of all sits mid-cell and moves 123 elements, 5 more than the 0.2 % of 59 200 that the present tolerance
    allows: it catches some single contributions and misses others.)"""
    feats = c["feats"]
    h, w = feats[0].shape[1:]
    px, py, _, _ = IR.project(c["rel"][v][2], c["samples"], h, w)
    inside = (px > 1) & (px < w - 2) & (py > 1) & (py < h - 2)
    assert inside.any()
    off = torch.maximum((px - px.round()).abs(), (py - py.round()).abs())
    off = torch.where(inside & (c["G"][v].abs() >= 1.0), off, torch.full_like(off, 9.0))
    d, r = divmod(int(off.flatten().argmin()), h * w)
    y, x = divmod(r, w)
    return d, y, x


@pytest.mark.parametrize("kind", ["rig", "rolled"])
def test_mutant_one_contribution_dropped_passes_the_present_tolerance(stage1, kind):
    """One (pixel, hypothesis) contribution of one view dropped at 37x50, D = 48: the tolerance of the autograd parity tests
    (rtol 1e-3, atol 2e-4 of the peak, 0.998 of the elements) accepts it; the intervals do not."""
    c = stage1(kind, 37, 50, 48, 4)
    v = 1
    d, y, x = _one_contribution(c, v)
    mask = torch.zeros_like(c["G"], dtype=torch.bool)
    mask[v, d, y, x] = True
    bad_ref, bad_src = _without(c, mask)
    peak = float(c["g_src"][v].abs().max())
    check_close(f"one contribution dropped under the present tolerance [{kind}]", bad_src[v], c["g_src"][v], rtol=1e-3, atol=2e-4 * peak,
                frac_ok=0.998)                                                              # accepted: the gap
    n = _outside(f"one contribution dropped: grad_src{v} [{kind} 37x50 D=48]", bad_src[v], c["iv_src"][v])
    assert 1 <= n <= 4 * 32
    _outside(f"one contribution dropped: grad_ref [{kind} 37x50 D=48]", bad_ref, c["iv_ref"])


@pytest.mark.parametrize("kind", ["rig", "rolled"])
def test_mutant_one_16_lane_row_of_one_hypothesis_dropped(stage1, kind):
    c = stage1(kind, 37, 50, 48, 4)
    mask = torch.zeros_like(c["G"], dtype=torch.bool)
    mask[0, 20, 18, 16:32] = True
    bad_ref, bad_src = _without(c, mask)
    _outside(f"one 16-lane row of one hypothesis dropped: grad_src0 [{kind}]", bad_src[0], c["iv_src"][0])
    _outside(f"one 16-lane row of one hypothesis dropped: grad_ref [{kind}]", bad_ref, c["iv_ref"])


@pytest.mark.parametrize("kind", ["rolled", "wide"])
def test_mutant_border_band_dropped(stage1, kind):
    c = stage1(kind, 37, 50, 48, 4)
    band = torch.stack([_band(r[0], r[1], c["samples"], 37, 50) for r in c["rel"]])
    assert band.any(), "the band must hold samples"
    _, bad_src = _without(c, band)
    n = sum(_outside(f"border band dropped: grad_src{v} [{kind}]", bad_src[v], c["iv_src"][v]) for v in range(3) if band[v].any())
    assert n > 0


@pytest.mark.parametrize("kind", ["rig", "rolled", "wide", "inside"])
def test_mutant_coordinates_shifted_by_a_hundredth_of_a_pixel(stage1, kind):
    c = stage1(kind, 16, 20, 8, 3)
    bad_ref, bad_src = _stage1_bwd(c["feats"], c["rel"], c["samples"], c["G"], shift_px=0.01)
    for v in range(2):
        n = _outside(f"coordinates shifted by 0.01 px: grad_src{v} [{kind}]", bad_src[v], c["iv_src"][v])
        if kind != "inside":
            assert n >= 0.5 * int((~c["iv_src"][v].must_be_zero).sum()), "most of what can be non-zero moves"
    _outside(f"coordinates shifted by 0.01 px: grad_ref [{kind}]", bad_ref, c["iv_ref"])


@pytest.mark.parametrize("kind", ["rig", "rolled"])
def test_mutants_scale_view_swap_and_padded_hypothesis(stage1, kind):
    c = stage1(kind, 9, 13, 6, 2)                    # D % 4 = 2: the window kernel pads its last group with hypothesis D - 1
    C = 32
    _outside(f"1/C missing: grad_src0 [{kind}]", c["g_src"][0] * C, c["iv_src"][0])
    _outside(f"1/C missing: grad_ref [{kind}]", c["g_ref"] * C, c["iv_ref"])
    # the padded hypothesis (d = D clamped to D - 1) added once: its gradient is that of the last plane
    extra = torch.zeros_like(c["G"])
    extra[:, -1] = c["G"][:, -1]
    e_ref, e_src = _stage1_bwd(c["feats"], c["rel"], c["samples"], extra)
    _outside(f"padded hypothesis added once: grad_src0 [{kind}]", c["g_src"][0] + e_src[0], c["iv_src"][0])
    _outside(f"padded hypothesis added once: grad_ref [{kind}]", c["g_ref"] + e_ref, c["iv_ref"])
    c4 = stage1(kind, 16, 20, 8, 3)
    _outside(f"two views' gradients swapped: grad_src0 [{kind}]", c4["g_src"][1], c4["iv_src"][0])
    _outside(f"two views' gradients swapped: grad_src1 [{kind}]", c4["g_src"][0], c4["iv_src"][1])


def test_sparse_gradient_pins_half_of_every_source_gradient_to_zero():
    """The sparse upstream gradient of the GPU test: its lattice hits both sides of every tile seam and the corners, and the
    reference pins at least half of each grad_src to exact 0."""
    h, w, N = 37, 50, 4
    (ya, xa), (yb, xb) = cases.seam_lattice(h, w)
    assert {0, 7, 15, 23, 31, 36} <= set(ya) and {8, 16, 24, 32} <= set(yb) and {0, 15, 31, 47, 49} <= set(xa) and {16, 32, 48} <= set(xb)
    for kind in ("rig", "rolled"):
        for D in (47, 48):
            feats, pm, samples = cases.stage1_case(kind, h, w, D, N)
            rel = _rel(pm)
            G = cases.sparse_grad(N - 1, D, h, w)
            assert set(G.abs().sum((0, 2, 3)).nonzero().flatten().tolist()) == {0, D - 1}
            g_ref, g_src = _stage1_bwd(feats, rel, samples, G)
            iv_ref, iv_src = SR.stage1_bwd_intervals(feats, torch.stack([r[2] for r in rel]), samples, G)
            IR.check_inside(f"autograd grad_ref, sparse G [{kind} D={D}]", g_ref, **iv_ref.args(), max_left_out=0.0)
            for v in range(N - 1):
                s = IR.check_inside(f"autograd grad_src{v}, sparse G [{kind} D={D}]", g_src[v], **iv_src[v].args(), max_left_out=0.0)
                assert s["must_be_zero"] >= 0.5 * s["elements"] and s["live"] > 0, s


# ---------------------------------------------------------------------------------------------
# the warped volume's backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.RIGS)
def test_homo_warp_bwd_autograd_inside(kind):
    C, h, w, D, N = 8, 9, 13, 6, 2
    feats, pm, samples = cases.stage1_case(kind, h, w, D, N, C=C)
    rot, trans, rt = _rel(pm)[0]
    gout = torch.randn(C, D, h, w, generator=torch.Generator().manual_seed(8))
    src = feats[1].clone().requires_grad_(True)
    grid = O.warp_grid(rot, trans, samples.view(1, D, 1, 1).expand(1, D, h, w), h, w)
    warped = F.grid_sample(src.unsqueeze(0), grid.view(1, D * h, w, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
    (warped.view(C, D, h, w) * gout).sum().backward()
    got = src.grad.permute(1, 2, 0)
    iv = SR.homo_warp_bwd_interval(rt, samples, gout)
    IR.check_inside(f"autograd homo_warp_bwd [{kind}]", got, **iv.args(), max_left_out=0.0)
    if kind != "far":
        _outside(f"homo_warp_bwd, channels rolled [{kind}]", got.roll(1, 2), iv)


# ---------------------------------------------------------------------------------------------
# stages 2/3
# ---------------------------------------------------------------------------------------------
def dyn_standin(feats, rel, cur, itv, view_w, shift, D, G):
    """fp32 autograd through the weighted volume -> (sim, samples, grad_ref, [grad_src], grad_view_w); grad_view_w as the kernel
    forms it: the fp32 s_vd and sim, summed in float64."""
    h, w = cur.shape
    S = len(rel)
    samples = 1.0 / O.cur_depth_range_samples(1.0 / cur.unsqueeze(0), D, itv)[0]
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    wv = view_w[:, ys >> shift, xs >> shift]
    leaves = [f.clone().requires_grad_(True) for f in feats]
    s_v = [_sim(leaves[0], leaves[v + 1], rel[v][0], rel[v][1], samples) for v in range(S)]
    den = wv.sum(0) + 1e-6
    sim = sum(wv[v] * s_v[v] for v in range(S)) / den
    (sim * G).sum().backward()
    cell = ((ys >> shift) * view_w.shape[2] + (xs >> shift)).reshape(-1)
    g_vw = torch.stack([torch.zeros(view_w[0].numel(), dtype=torch.float64).index_add(
        0, cell, (G.double() * (s_v[v].detach().double() - sim.detach().double()) / den.double()).sum(0).reshape(-1)).reshape(view_w[0].shape)
        for v in range(S)])
    return (sim.detach(), samples, leaves[0].grad.permute(1, 2, 0).contiguous(), [l_.grad.permute(1, 2, 0).contiguous() for l_ in leaves[1:]],
            g_vw.float())


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("depth", ["smooth", "noisy", "clamps"])
@pytest.mark.parametrize("kind", ["rig", "rolled", "inside"])
def test_dyn_autograd_inside_and_mutants(kind, depth, shift):
    C, D, S = 8, 4, 2
    h, w = (17, 23) if shift == 0 else (16, 24)
    feats = [f[0] for f in synth.smooth_features(S + 1, C, h, w, seed=11)]
    rel = _rel(cases.dyn_cameras(h, w, S + 1, kind).unsqueeze(0))
    view_w = 0.2 + torch.rand(S, h >> shift, w >> shift, generator=torch.Generator().manual_seed(5))
    cur, itv = cases.dyn_depth(h, w, depth), torch.tensor(2.0e-5)
    G = cases.dense_grad(1, D, h, w)[0]
    sim, samples, g_ref, g_src, g_vw = dyn_standin(feats, rel, cur, itv, view_w, shift, D, G)
    iv_ref, iv_src, iv_vw = SR.dyn_bwd_intervals(feats, torch.stack([r[2] for r in rel]), samples, view_w, shift, sim, G)
    tag = f"[{kind} {depth} {h}x{w}>>{shift}]"
    IR.check_inside(f"autograd dyn grad_ref {tag}", g_ref, **iv_ref.args(), max_left_out=0.0)
    for v in range(S):
        IR.check_inside(f"autograd dyn grad_src{v} {tag}", g_src[v], **iv_src[v].args(), max_left_out=0.0)
    IR.check_inside(f"dyn grad_view_w {tag}", g_vw, **iv_vw.args(), max_left_out=0.0)
    peak = float(torch.maximum(iv_vw.lo.abs(), iv_vw.hi.abs()).max())
    print(f"[interval] dyn grad_view_w {tag}: widest + tol / peak = {float((iv_vw.hi - iv_vw.lo + 2 * iv_vw.tol).max()) / max(peak, 1e-300):.3e}")
    _outside(f"dyn: two views' gradients swapped {tag}", g_src[1], iv_src[0])
    _outside(f"dyn: view-weight gradients swapped {tag}", g_vw.flip(0), iv_vw)


# ---------------------------------------------------------------------------------------------
# 1-D look-ups
# ---------------------------------------------------------------------------------------------
def _lookup_bwd_fp32(gout, Dp, q, dmin, dmax, swap=False):
    """The 1-D scatter written out in fp32 (volume_lookup_1d_explicit's position and weights); swap: w0 / w1 exchanged."""
    t = O.depth_to_disp(q, dmin, dmax) * (Dp - 1)
    ix = ((2 * t / (Dp - 1) - 1 + 1) / 2) * (Dp - 1)
    i0 = torch.floor(ix)
    w1, w0 = ix - i0, (i0 + 1) - ix
    if swap:
        w0, w1 = w1, w0
    i0 = i0.long()
    gvol = torch.zeros(Dp, *gout.shape[1:])
    for idx, wgt in ((i0, w0), (i0 + 1, w1)):
        ok = (idx >= 0) & (idx <= Dp - 1)
        gvol.scatter_add_(0, idx.clamp(0, Dp - 1), gout * wgt * ok)
    return gvol


@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("Dp,nq,h,w", [(2, 1, 9, 13), (8, 3, 9, 13), (8, 4, 9, 13), (2, 5, 9, 13), (48, 4, 20, 29)])
def test_lookup_bwd_autograd_inside_and_mutants(Dp, nq, h, w, per_pixel, twice):
    vol, q, dmin, dmax, gout = cases.lookup_bwd_case(Dp, nq, h, w, per_pixel, twice)
    qv = q[:, 0:2 * h:2, 0:2 * w:2] if twice else q
    leaf = vol.clone().requires_grad_(True)
    (O.volume_lookup_1d_explicit(leaf.unsqueeze(0), qv.unsqueeze(0), dmin, dmax)[0] * gout).sum().backward()
    iv = SR.lookup_bwd_interval(gout, Dp, q, dmin, dmax)
    tag = f"Dp={Dp} nq={nq} {'per-pixel' if per_pixel else 'global'} {'2x' if twice else '1x'}"
    s = IR.check_inside(f"autograd lookup bwd {tag}", leaf.grad, **iv.args(), max_left_out=0.0)
    IR.check_inside(f"explicit fp32 lookup bwd {tag}", _lookup_bwd_fp32(gout, Dp, qv, dmin, dmax), **iv.args(), max_left_out=0.0)
    assert s["must_be_zero"] > 0, "planes no query reaches are pinned to exact 0"
    # queries exactly at dmin / dmax put (all but a rounding of) their weight on the last / first plane
    t, dt = IR.lookup_box(qv, dmin, dmax, Dp)
    assert float((t[0, 0::3, 0::2] - (Dp - 1)).abs().max()) < 1e-4 and float(t[nq - 1, 1::3, 1::2].abs().max()) < 1e-4 and float(dt.max()) < 1e-3
    _outside(f"lookup index off by one {tag}", leaf.grad.roll(1, 0), iv)
    _outside(f"lookup w0 / w1 exchanged {tag}", _lookup_bwd_fp32(gout, Dp, qv, dmin, dmax, swap=True), iv)
    if twice:
        wrong = q[:, 1:2 * h + 1:2, 1:2 * w + 1:2]
        _outside(f"lookup reads the odd pixels of the 2x query map {tag}", _lookup_bwd_fp32(gout, Dp, wrong, dmin, dmax), iv)


@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("Dcur,Dreg,nq", [(8, 8, 3), (48, 8, 4), (2, 48, 3), (8, 48, 4)])
def test_getcost_bwd_autograd_inside_and_mutants(Dcur, Dreg, nq, per_pixel, input_is_depth):
    h, w = 9, 13
    cur, reg, x, disp_range, itv, dmin, dmax = cases.getcost_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth)
    gcost = torch.randn(2 * nq, h, w, generator=torch.Generator().manual_seed(3))
    depth = x if input_is_depth else O.disp_to_depth(x, 1.0 / disp_range[-1], 1.0 / disp_range[0])[1]
    lc, lr = cur.clone().requires_grad_(True), reg.clone().requires_grad_(True)
    pro = [lr.permute(1, 2, 0).reshape(h * w, 1, 1, Dreg), lc.permute(1, 2, 0).reshape(h * w, 1, 1, Dcur)]
    (O.getcost(depth.view(1, 1, h, w), pro, itv.view(1, 1), nq, dmax, dmin, [1, h, w])[0] * gcost).sum().backward()
    qd = IR.getcost_queries(O, x, disp_range, itv, nq, input_is_depth)
    iv_c, iv_r = SR.getcost_bwd_intervals(gcost, Dcur, Dreg, qd, dmin, dmax)
    tag = f"Dcur={Dcur} Dreg={Dreg} nq={nq} {'per-pixel' if per_pixel else 'global'} depth={int(input_is_depth)}"
    IR.check_inside(f"autograd getcost bwd cur {tag}", lc.grad, **iv_c.args(), max_left_out=0.0)
    IR.check_inside(f"autograd getcost bwd reg {tag}", lr.grad, **iv_r.args(), max_left_out=0.0)
    _outside(f"getcost bwd cur, index off by one {tag}", lc.grad.roll(1, 0), iv_c)
    # the two halves of the upstream gradient exchanged
    iv_x, _ = SR.getcost_bwd_intervals(torch.cat([gcost[nq:], gcost[:nq]]), Dcur, Dreg, qd, dmin, dmax)
    _outside(f"getcost bwd cur from the reg half of the gradient {tag}", lc.grad, iv_x)
