"""GPU: every element of the backward kernels that scatter -- warpcorr_views_bwd (direct and LDS-window forms), homo_warp_bwd,
warpcorr_dyn_bwd, vol_lookup1d_bwd, getcost_bwd -- inside its float64 interval (tests/scatter_ref.py): no tolerated fraction of
outliers, exact zeros where nothing can arrive, `max_left_out` 0 on every case.  One float64 reference per (rig, shape), shared by
the kernel forms.  Each check prints the share of live and must-be-zero elements, the widest interval relative to the peak and how
much of its interval the kernel uses (the table of DESIGN.md section 2.3)."""
import pytest
import torch

import interval_cases as cases
import interval_ref as IR
import scatter_ref as SR
from common import check_close, t
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FORMS = (("window", None), ("global atomics", 0), ("8 KB window", 8), ("direct", -1))


@pytest.fixture(scope="module")
def O():
    from oracle import effi_oracle
    return effi_oracle


def _check(name, got, iv):
    s = IR.check_inside(name, got, **iv.args(), max_left_out=0.0)
    peak = float(torch.maximum(iv.lo.abs(), iv.hi.abs()).max())
    s["zero_share"] = s["must_be_zero"] / max(1, s["elements"])
    s["widest_rel"] = float((iv.hi - iv.lo + 2 * iv.tol).max()) / peak if peak > 0 else 0.0
    print(f"[scatter] {name:50s} live={s['live']:.4f} must_be_zero={s['zero_share']:.4f} widest/peak={s['widest_rel']:.3e} used={s['used']:.3f}")
    return s


# ---------------------------------------------------------------------------------------------
# stage 1
# ---------------------------------------------------------------------------------------------
_STAGE1 = {}


def _stage1(kind, h, w, D, N, grad):
    """The inputs on the device and the float64 reference of one (rig, shape, upstream gradient), built once per module."""
    from effi_mvs_plus_amd import ops
    key = (kind, h, w, D, N, grad)
    if key not in _STAGE1:
        feats, pm, samples = cases.stage1_case(kind, h, w, D, N)
        G = cases.dense_grad(N - 1, D, h, w) if grad == "dense" else cases.sparse_grad(N - 1, D, h, w)
        rt = ops.compose_rel_proj(t(pm[0], DEV))
        iv_ref, iv_src = SR.stage1_bwd_intervals(feats, rt.cpu(), samples, G)
        _STAGE1[key] = (ops.to_nhwc([t(f, DEV) for f in feats]), rt, t(samples, DEV), t(G, DEV), iv_ref, iv_src)
    return _STAGE1[key]


def _stage1_forms(tag, nhwc, rt, samples, G, D, iv_ref, iv_src, forms=FORMS):
    """Every form of ops.warpcorr_views_bwd against one reference -> per form (name, statistics [grad_ref, grad_src0, ..], g_ref, g_src)."""
    from effi_mvs_plus_amd import ops
    out = []
    for form, lds in forms:
        with ops.options(warp_lds_kb=lds):
            g_ref, g_src = ops.warpcorr_views_bwd(nhwc[0], nhwc[1:], rt, samples, D, G)
            torch.cuda.synchronize()
        stats = [_check(f"stage 1 bwd {form} grad_ref {tag}", g_ref, iv_ref)]
        stats += [_check(f"stage 1 bwd {form} grad_src{v} {tag}", g_src[v], iv_src[v]) for v in range(len(g_src))]
        out.append((form, stats, g_ref, g_src))
    return out


@pytest.mark.parametrize("kind", cases.RIGS)
@pytest.mark.parametrize("h,w,D,N", cases.STAGE1_SHAPES)
def test_warpcorr_views_bwd_every_form_inside(kind, h, w, D, N):
    """C = 32, shared hypotheses, dense Gaussian upstream gradient: the default LDS window, every chunk on global atomics
    (warp_lds_kb = 0), a window that makes chunks shrink (8) and the direct kernel (-1)."""
    nhwc, rt, samples, G, iv_ref, iv_src = _stage1(kind, h, w, D, N, "dense")
    for form, stats, g_ref, g_src in _stage1_forms(f"[{kind} {h}x{w} D={D}]", nhwc, rt, samples, G, D, iv_ref, iv_src):
        if kind == "far":
            assert not g_ref.any() and not any(g.any() for g in g_src), f"{form}: the view that looks away: exact zeros everywhere"
            assert all(s["must_be_zero"] == s["elements"] for s in stats)
        elif not (kind == "inside" and D == 1):
            live_src = sum(s["live"] for s in stats[1:]) / (N - 1)
            assert stats[0]["live"] >= 0.05 and live_src >= 0.05, f"{form} [{kind}]: live shares {[s['live'] for s in stats]}"


@pytest.mark.parametrize("kind", ["rig", "rolled"])
@pytest.mark.parametrize("D", [47, 48])
def test_warpcorr_views_bwd_sparse_gradient(kind, D):
    """An upstream gradient on isolated pixels of hypotheses {0, D - 1} only, on both sides of every 16 x 8 tile seam and at the map's
    corners: at least half of every grad_src is pinned to exact 0, so a stray add to a wrong pixel, view or padded hypothesis (D = 47:
    the last group of four holds hypothesis 46 twice) has nowhere to hide."""
    h, w, N = 37, 50, 4
    nhwc, rt, samples, G, iv_ref, iv_src = _stage1(kind, h, w, D, N, "sparse")
    for form, stats, _, _ in _stage1_forms(f"sparse [{kind} {h}x{w} D={D}]", nhwc, rt, samples, G, D, iv_ref, iv_src):
        for s in stats[1:]:
            assert s["zero_share"] >= 0.5, f"{form}: only {s['zero_share']:.3f} of a source gradient is pinned to 0"
        assert sum(s["live"] for s in stats[1:]) > 0, form


@pytest.mark.parametrize("D", [256, 257])
def test_warpcorr_views_bwd_longest_window_launch_and_first_direct_one(D):
    """9x13, C = 32: D = 256 is the last launch of the window kernel (its hypothesis table is full), D = 257 the direct kernel."""
    nhwc, rt, samples, G, iv_ref, iv_src = _stage1("rig", 9, 13, D, 2, "dense")
    _stage1_forms(f"[rig 9x13 D={D}]", nhwc, rt, samples, G, D, iv_ref, iv_src, forms=FORMS[:3] if D == 256 else FORMS[:1])


@pytest.mark.parametrize("C,h,w,D,N", [(32, 16, 20, 8, 3), (16, 18, 30, 5, 5), (8, 21, 27, 6, 3)])
def test_warpcorr_views_bwd_per_pixel_hypotheses(C, h, w, D, N):
    """Per-pixel hypotheses [D,h,w] (the direct kernel whatever C) at C = 32 and the generic forms C = 16 / 8."""
    from effi_mvs_plus_amd import ops
    feats = [f[0] for f in synth.smooth_features(N, C, h, w, seed=100 + C)]
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"]
    samples = 425.0 + 510.0 * torch.rand(D, h, w, generator=torch.Generator().manual_seed(1))
    G = cases.dense_grad(N - 1, D, h, w)
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    iv_ref, iv_src = SR.stage1_bwd_intervals(feats, rt.cpu(), samples, G)
    nhwc = ops.to_nhwc([t(f, DEV) for f in feats])
    (_, stats, _, _), = _stage1_forms(f"per-pixel C={C} [{h}x{w} D={D}]", nhwc, rt, t(samples, DEV), t(G, DEV), D, iv_ref, iv_src,
                                      forms=FORMS[:1])
    assert stats[0]["live"] >= 0.5


# ---------------------------------------------------------------------------------------------
# the warped volume's backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("kind,h,w,D", [(k, 9, 13, 6) for k in cases.RIGS] + [("rig", 37, 50, 5), ("rolled", 37, 50, 5)])
def test_homo_warp_bwd_inside(O, C, kind, h, w, D):
    from effi_mvs_plus_amd import ops
    N = 2
    feats, pm, samples = cases.stage1_case(kind, h, w, D, N, C=C)
    P = [O.compose_projection(pm[:, v]) for v in range(N)]
    rt = ops.rel_proj(t(P[1][0], DEV), t(P[0][0], DEV))
    gout = torch.randn(C, D, h, w, generator=torch.Generator().manual_seed(8 + C))
    iv = SR.homo_warp_bwd_interval(rt.cpu(), samples, gout)
    got = ops.homo_warp_bwd(rt, t(samples, DEV), D, t(gout, DEV), h, w)
    s = _check(f"homo_warp_bwd C={C} [{kind} {h}x{w} D={D}]", got, iv)
    if kind == "far":
        assert not got.any() and s["must_be_zero"] == s["elements"]
    else:
        assert s["live"] >= 0.05


# ---------------------------------------------------------------------------------------------
# stages 2/3
# ---------------------------------------------------------------------------------------------
# tiles of the kernel: 8 x 4 (C = 32), 16 x 4 (C = 16), 16 x 8 (C = 8) pixels: two tiles and a partial one each way
@pytest.mark.parametrize("C,S,D,h,w,shift,kind,depth", [
    (8, 1, 8, 17, 33, 0, "rig", "smooth"), (8, 2, 8, 17, 33, 0, "rig", "smooth"), (16, 3, 4, 10, 34, 1, "rolled", "noisy"), (8, 6, 6, 18, 34, 1, "inside", "clamps"),
    (16, 10, 8, 12, 36, 2, "rig", "noisy"), (8, 3, 4, 17, 33, 0, "rolled", "clamps"), (32, 2, 4, 10, 18, 1, "rolled", "smooth")])
def test_warpcorr_dyn_bwd_inside(O, C, S, D, h, w, shift, kind, depth):
    """grad_ref, every grad_src and grad_view_w at the hypotheses the forward kernel returned for the same inputs; `sim` is the
    forward's own output, as on the training path.  With ONE view (the first case) s - sim = 1e-6 s / den: grad_view_w is all
    rounding there and its interval, twice the peak, is a sanity bound only; the same case with two views follows it, and from S = 2
    on the interval is at most 1e-3 of the peak, which the test asserts."""
    from effi_mvs_plus_amd import ops
    N = S + 1
    feats = [f[0] for f in synth.smooth_features(N, C, h, w, seed=11)]
    pm = cases.dyn_cameras(h, w, N, kind)
    nhwc = ops.to_nhwc([t(f, DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm, DEV))
    view_w = 0.2 + torch.rand(S, h >> shift, w >> shift, generator=torch.Generator().manual_seed(5))
    cur, itv = cases.dyn_depth(h, w, depth), torch.tensor([2.0e-5])
    G = cases.dense_grad(1, D, h, w)[0]
    sim, smp = ops.warpcorr_dyn(nhwc[0], nhwc[1:], rt, t(cur, DEV), t(itv, DEV), t(view_w, DEV), D)
    want_smp = 1.0 / O.cur_depth_range_samples(1.0 / cur.unsqueeze(0), D, itv[0])[0]
    check_close("dyn hypotheses", smp, want_smp, rtol=2e-6, atol=0)
    iv_ref, iv_src, iv_vw = SR.dyn_bwd_intervals(feats, rt.cpu(), smp.cpu(), view_w, shift, sim.cpu(), G)
    g_ref, g_src, g_vw = ops.warpcorr_dyn_bwd(nhwc[0], nhwc[1:], rt, t(cur, DEV), t(itv, DEV), t(view_w, DEV), D, sim, t(G, DEV))
    torch.cuda.synchronize()
    tag = f"[C={C} S={S} D={D} {h}x{w}>>{shift} {kind} {depth}]"
    s = _check(f"dyn bwd grad_ref {tag}", g_ref, iv_ref)
    assert s["live"] >= 0.05
    for v in range(S):
        _check(f"dyn bwd grad_src{v} {tag}", g_src[v], iv_src[v])
    s = _check(f"dyn bwd grad_view_w {tag}", g_vw, iv_vw)
    assert S == 1 or (s["widest_rel"] <= 1e-3 and s["live"] >= 0.5), f"grad_view_w is not meaningfully bounded: {s}"


# ---------------------------------------------------------------------------------------------
# look-ups
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("Dp,nq", [(2, 1), (2, 5), (8, 1), (8, 5)])
def test_vol_lookup1d_bwd_inside(Dp, nq, per_pixel, twice):
    """20x29 = three blocks, the last one partial.  Queries below, above and exactly at both ends of the range; the query map at the
    volume's resolution and at twice it (odd-sized: read at its even pixels)."""
    from effi_mvs_plus_amd import ops
    h, w = 20, 29
    _, q, dmin, dmax, gout = cases.lookup_bwd_case(Dp, nq, h, w, per_pixel, twice)
    iv = SR.lookup_bwd_interval(gout, Dp, q, dmin, dmax)
    got = ops.vol_lookup1d_bwd(t(gout, DEV), Dp, t(q, DEV), t(dmin, DEV), t(dmax, DEV), h, w)
    s = _check(f"vol_lookup1d_bwd Dp={Dp} nq={nq} {'per-pixel' if per_pixel else 'global'} {'2x' if twice else '1x'}", got, iv)
    if nq == 1:
        # a twelfth of the queries each lies far below / above the range: their pixels' rows are pinned to exact 0
        assert s["zero_share"] >= 0.1, "rows whose only query is far outside are pinned to exact 0"
        # a query exactly at dmin / dmax puts its whole weight on the last / first plane: to the position's rounding (lookup_box:
        # 1e-5 planes at Dp = 8), and not one bit on a plane further away
        g, o = gout[0].double(), got.double().cpu()
        for plane, (ys, xs) in ((Dp - 1, (slice(0, None, 3), slice(0, None, 2))), (0, (slice(1, None, 3), slice(1, None, 2)))):
            assert float(((o[plane] - g)[ys, xs].abs() / g[ys, xs].abs()).max()) <= 1e-4
            rest = [d for d in range(Dp) if abs(d - plane) > 1]
            assert not o[rest][:, ys, xs].any()


@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("Dcur,Dreg,nq", [(8, 8, 3), (48, 8, 4), (2, 48, 3), (8, 48, 4)])
def test_getcost_bwd_inside(O, Dcur, Dreg, nq, per_pixel, input_is_depth):
    from effi_mvs_plus_amd import ops
    h, w = 20, 29
    _, _, x, disp_range, itv, dmin, dmax = cases.getcost_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth)
    gcost = torch.randn(2 * nq, h, w, generator=torch.Generator().manual_seed(3))
    qd = IR.getcost_queries(O, x, disp_range, itv, nq, input_is_depth)
    iv_c, iv_r = SR.getcost_bwd_intervals(gcost, Dcur, Dreg, qd, dmin, dmax)
    gcur, greg = ops.getcost_bwd(t(gcost, DEV), t(x, DEV), t(disp_range, DEV), t(itv, DEV), Dcur, Dreg, t(dmin, DEV), t(dmax, DEV), nq, h, w,
                                 input_is_depth=input_is_depth)
    tag = f"Dcur={Dcur} Dreg={Dreg} nq={nq} {'per-pixel' if per_pixel else 'global'} depth={int(input_is_depth)}"
    s = _check(f"getcost_bwd cur {tag}", gcur, iv_c)
    _check(f"getcost_bwd reg {tag}", greg, iv_r)
    assert s["live"] >= 0.05


def test_getcost_bwd_refuses_a_single_hypothesis():
    """nq = 1 has no step between hypotheses: the entry refuses it, as the forward does."""
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd._lib import EffiLibraryError
    h, w = 9, 13
    _, _, x, disp_range, itv, dmin, dmax = cases.getcost_case(8, 8, 3, h, w, False, False)
    with pytest.raises(EffiLibraryError):
        ops.getcost_bwd(torch.zeros(2, h, w, device=DEV), t(x, DEV), t(disp_range, DEV), t(itv, DEV), 8, 8, t(dmin, DEV), t(dmax, DEV), 1, h, w)
