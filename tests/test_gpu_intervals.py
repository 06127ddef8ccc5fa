"""GPU: every element of the warp, look-up and soft-argmin kernels inside its float64 interval (tests/interval_ref.py): no tolerated
fraction of outliers.  An element is inside [lo - tol, hi + tol], or exactly 0 where every tap is provably outside the image, or
left out (coordinate uncertainty above a quarter pixel) -- and `max_left_out` is 0 on every case here.  Each check prints the share
of live elements, the widest interval and how much of its interval the kernel uses (the figures of DESIGN.md section 2.1)."""
import pytest
import torch

import interval_cases as cases
import interval_ref as IR
from common import check_close, t
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def O():
    from oracle import effi_oracle
    return effi_oracle


def _entropy(name, ent, sim, D):
    """The entropy output against the softmax entropy of the kernel's OWN similarities: a similarity error is not reported twice."""
    want = IR.entropy_from(sim)
    err = float((ent.detach().double().cpu() - want).abs().max())
    print(f"[interval] {name:42s} entropy max_abs={err:.3e} bound={IR.entropy_atol(D):.3e}")
    assert err <= IR.entropy_atol(D), f"{name}: entropy off by {err:.3e} (bound {IR.entropy_atol(D):.3e})"


# ---------------------------------------------------------------------------------------------
# stage 1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.RIGS)
@pytest.mark.parametrize("h,w,D,N", cases.STAGE1_SHAPES)
def test_warpcorr_views_every_form_inside(kind, h, w, D, N):
    """C = 32, shared hypotheses: the default window kernel, every chunk on global loads (warp_lds_kb = 0), a window that makes chunks
    shrink (8), the direct-gather kernel (-1) and the matrix-core form in split precision, one float64 reference for all."""
    from effi_mvs_plus_amd import ops
    feats, pm, samples = cases.stage1_case(kind, h, w, D, N)
    nhwc = ops.to_nhwc([t(f, DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    iv = IR.stack([IR.warp_sim_interval(feats[0], feats[v + 1], rt[v].cpu(), samples) for v in range(N - 1)])
    run = lambda **kw: ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D, **kw)       # noqa: E731
    live = None
    for form, lds in (("window", None), ("global loads", 0), ("8 KB window", 8), ("direct gather", -1)):
        with ops.options(warp_lds_kb=lds):
            sim, ent = run()
        s = IR.check_inside(f"stage 1 {form} [{kind} {h}x{w} D={D}]", sim, **iv.args(), max_left_out=0.0)
        _entropy(f"stage 1 {form} [{kind} {h}x{w} D={D}]", ent, sim, D)
        live = s["live"]
    before = ops.get_precision()
    try:
        ops.set_precision("split")
        sim, ent = run(x3=True)
    finally:
        ops.set_precision(before)
    IR.check_inside(f"stage 1 matrix cores [{kind} {h}x{w} D={D}]", sim, **iv.args(x3=True), max_left_out=0.0)
    _entropy(f"stage 1 matrix cores [{kind} {h}x{w} D={D}]", ent, sim, D)
    if kind == "far":
        assert live == 0.0
    elif not (kind == "inside" and D == 1):
        assert live >= 0.05, f"{kind}: only {live:.4f} of the similarities are live"


def test_warpcorr_views_shuffled_hypotheses_inside():
    from effi_mvs_plus_amd import ops
    h, w, D, N = 37, 50, 48, 4
    feats, pm, samples = cases.stage1_case("rig", h, w, D, N)
    samples = samples[torch.randperm(D, generator=torch.Generator().manual_seed(3))]
    nhwc = ops.to_nhwc([t(f, DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    iv = IR.stack([IR.warp_sim_interval(feats[0], feats[v + 1], rt[v].cpu(), samples) for v in range(N - 1)])
    sim, ent = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D)
    IR.check_inside("stage 1 window, shuffled hypotheses", sim, **iv.args(), max_left_out=0.0)
    _entropy("stage 1 window, shuffled hypotheses", ent, sim, D)
    before = ops.get_precision()
    try:
        ops.set_precision("split")
        sim, ent = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D, x3=True)
    finally:
        ops.set_precision(before)
    IR.check_inside("stage 1 matrix cores, shuffled hypotheses", sim, **iv.args(x3=True), max_left_out=0.0)
    _entropy("stage 1 matrix cores, shuffled hypotheses", ent, sim, D)


@pytest.mark.parametrize("C,h,w,D,N", [(16, 18, 30, 5, 5), (8, 21, 27, 6, 3)])
def test_warpcorr_views_generic_kernel_inside(C, h, w, D, N):
    """C = 8 / 16 with per-pixel hypotheses [D,h,w]: the generic kernel (IEEE divisions)."""
    from effi_mvs_plus_amd import ops
    feats = [f[0] for f in synth.smooth_features(N, C, h, w, seed=100 + C)]
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"]
    samples = 425.0 + 510.0 * torch.rand(D, h, w, generator=torch.Generator().manual_seed(1))
    nhwc = ops.to_nhwc([t(f, DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    iv = IR.stack([IR.warp_sim_interval(feats[0], feats[v + 1], rt[v].cpu(), samples) for v in range(N - 1)])
    sim, ent = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D)
    s = IR.check_inside(f"stage 1 generic C={C} {h}x{w} D={D}", sim, **iv.args(), max_left_out=0.0)
    assert s["live"] >= 0.5
    _entropy(f"stage 1 generic C={C}", ent, sim, D)


@pytest.mark.parametrize("kind", cases.RIGS)
def test_homo_warping_new_inside(O, kind):
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.module import homo_warping_new
    C, h, w, D, N = 8, 9, 13, 6, 2
    feats, pm, samples = cases.stage1_case(kind, h, w, D, N, C=C)
    P = [O.compose_projection(pm[:, v]) for v in range(N)]
    got = homo_warping_new(t(feats[1].unsqueeze(0), DEV), t(P[1], DEV), t(P[0], DEV), t(samples.unsqueeze(0), DEV))
    rt = ops.rel_proj(t(P[1][0], DEV), t(P[0][0], DEV))
    iv = IR.warp_interval(feats[1], rt.cpu(), samples)
    IR.check_inside(f"homo_warping_new [{kind}]", got.view(C, D, h, w), **iv.args(), max_left_out=0.0)


# ---------------------------------------------------------------------------------------------
# stages 2/3
# ---------------------------------------------------------------------------------------------
DYN_FORMS = [("default", {}), ("lanes split channels", {"dyn_form": 1}), ("exact divisions", {"dyn_setup_exact": 1}),
             ("gather", {"dyn_win": -1}), ("window off", {"dyn_win": 0}), ("48-pixel window", {"dyn_win": 48})]


@pytest.mark.parametrize("C,S,D,h,w,shift,kind,depth", [
    (8, 1, 8, 33, 47, 0, "rig", "smooth"), (16, 3, 4, 24, 40, 1, "rolled", "noisy"), (8, 6, 6, 16, 20, 1, "inside", "clamps"),
    (16, 10, 8, 24, 40, 2, "rig", "noisy"), (8, 3, 4, 33, 47, 0, "rolled", "clamps"), (16, 1, 6, 16, 20, 1, "rolled", "smooth"),
    (8, 10, 8, 16, 20, 1, "inside", "smooth"), (16, 6, 8, 33, 47, 0, "inside", "noisy")])
def test_warpcorr_dyn_every_form_inside(O, C, S, D, h, w, shift, kind, depth):
    """Every form of the stage-2/3 kernel against ONE independent reference per case: every (C, S) once, every form on every rig;
    odd maps with full-resolution view weights, even ones with half / quarter resolution; smooth, noisy and clamp-hitting depth."""
    from effi_mvs_plus_amd import ops
    N = S + 1
    feats = [f[0] for f in synth.smooth_features(N, C, h, w, seed=11)]
    pm = cases.dyn_cameras(h, w, N, kind)
    nhwc = ops.to_nhwc([t(f, DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm, DEV))
    view_w = 0.2 + torch.rand(S, h >> shift, w >> shift, generator=torch.Generator().manual_seed(5))
    cur, itv = cases.dyn_depth(h, w, depth), torch.tensor([2.0e-5])
    want_smp = 1.0 / O.cur_depth_range_samples(1.0 / cur.unsqueeze(0), D, itv[0])[0]
    iv = None
    for form, opts in DYN_FORMS:
        with ops.options(dyn_form=None, dyn_setup_exact=None, dyn_win=None), ops.options(**opts):
            sim, smp = ops.warpcorr_dyn(nhwc[0], nhwc[1:], rt, t(cur, DEV), t(itv, DEV), t(view_w, DEV), D)
            torch.cuda.synchronize()
        check_close(f"dyn hypotheses {form}", smp, want_smp, rtol=2e-6, atol=0)
        if iv is None:
            first = smp.cpu()
            iv = IR.dyn_sim_interval(feats[0], feats[1:], rt.cpu(), first, view_w, shift)
        assert torch.equal(smp.cpu(), first), "the hypotheses do not depend on the form"
        s = IR.check_inside(f"dyn {form} [C={C} S={S} D={D} {h}x{w}>>{shift} {kind} {depth}]", sim, **iv.args(), max_left_out=0.0)
        assert s["live"] >= 0.05, f"only {s['live']:.4f} of the similarities are live"


# ---------------------------------------------------------------------------------------------
# look-ups
# ---------------------------------------------------------------------------------------------
def _shares(vol, q, dmin, dmax):
    pos, _ = IR.lookup_position(q, dmin, dmax, vol.shape[0])
    inside = float(((pos >= 0) & (pos <= vol.shape[0] - 1)).double().mean())
    assert inside >= 0.5 and 1.0 - inside >= 0.05, f"queries in range: {inside:.3f}"


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("Dp,nq,h,w", [(2, 1, 9, 13), (8, 3, 9, 13), (48, 4, 20, 29), (8, 4, 20, 29), (48, 1, 9, 13), (2, 3, 20, 29)])
def test_vol_lookup1d_inside(Dp, nq, h, w, per_pixel):
    """Planar volume, the zero-copy pixel-major view of it (test_vol_lookup) and the pair launch; queries below, above and exactly at
    both ends of the range."""
    from effi_mvs_plus_amd import ops
    vol, q, dmin, dmax = cases.lookup_case(Dp, nq, h, w, per_pixel)
    vol_b = vol.flip(0).contiguous()
    _shares(vol, q, dmin, dmax)
    iv, iv_b = IR.lookup_interval(vol, q, dmin, dmax), IR.lookup_interval(vol_b, q, dmin, dmax)
    tag = f"Dp={Dp} nq={nq} {h}x{w} {'per-pixel' if per_pixel else 'global'}"
    vd, vbd, qd, lo, hi = t(vol, DEV), t(vol_b, DEV), t(q, DEV), t(dmin, DEV), t(dmax, DEV)
    s = IR.check_inside(f"vol_lookup1d planar {tag}", ops.vol_lookup1d(vd, qd, lo, hi, h, w), **iv.args())
    assert s["must_be_zero"] > 0
    pro = vd.unsqueeze(0).permute(0, 2, 3, 1).reshape(h * w, 1, 1, Dp)                 # zero-copy strided view
    assert pro.data_ptr() == vd.data_ptr()
    IR.check_inside(f"vol_lookup1d strided view {tag}", ops.vol_lookup1d(pro, qd, lo, hi, h, w), **iv.args())
    a, b = ops.vol_lookup1d_pair(vd, vbd, qd, lo, hi, h, w)
    IR.check_inside(f"vol_lookup1d_pair a {tag}", a, **iv.args())
    IR.check_inside(f"vol_lookup1d_pair b {tag}", b, **iv_b.args())


@pytest.mark.parametrize("input_is_depth", [False, True])
@pytest.mark.parametrize("Dcur,Dreg,nq,h,w,per_pixel", [(8, 8, 3, 9, 13, False), (48, 8, 4, 20, 29, True), (2, 48, 3, 9, 13, True),
                                                       (48, 48, 4, 20, 29, False)])
def test_getcost_inside(O, Dcur, Dreg, nq, h, w, per_pixel, input_is_depth):
    from effi_mvs_plus_amd import ops
    cur, reg, x, disp_range, itv, dmin, dmax = cases.getcost_case(Dcur, Dreg, nq, h, w, per_pixel, input_is_depth)
    qd = IR.getcost_queries(O, x, disp_range, itv, nq, input_is_depth)
    _shares(cur, qd, dmin, dmax)
    got = ops.getcost(t(x, DEV), t(disp_range, DEV), t(itv, DEV), t(cur, DEV), t(reg, DEV), t(dmin, DEV), t(dmax, DEV), nq, h, w,
                      input_is_depth=input_is_depth)
    for name, vol, part in (("cur", cur, got[:nq]), ("reg", reg, got[nq:])):
        iv = IR.lookup_interval(vol, qd, dmin, dmax, n_round=IR.GETCOST_ROUNDINGS)
        IR.check_inside(f"getcost {name} D={vol.shape[0]} nq={nq} {h}x{w} depth={int(input_is_depth)}", part, **iv.args())


# ---------------------------------------------------------------------------------------------
# soft-argmin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 16, 32, 48, 64, 96, 2, 3, 5, 7, 47, 97])
def test_softmax_regress_conf_inside(O, D):
    """Every register instantiation (8 .. 96) and the generic kernel, 13 x 17 = three full waves + 29 lanes, in the forms the path uses:
    plain, with the normalised inverse depth, with the replicated confidence (f = 3: scalar stores, 4: 16-byte stores), and the
    sample-batched launch with a shared (stride-0) hypothesis tensor -- all through the same set check."""
    from effi_mvs_plus_amd import ops
    h, w = 13, 17
    logits = cases.softmax_logits(D, h, w)
    cs = IR.confidence_set(logits, D)
    two = float(cs.two.double().mean())
    assert two >= 0.05 and 1.0 - two >= 0.5 and bool((cs.idx == 0).any()) and bool((cs.idx == D - 1).any())
    dv = torch.linspace(425.0, 935.0, D)
    want_d = (torch.softmax(logits.double(), 0) * dv.double().view(D, 1, 1)).sum(0)
    disp_range = torch.linspace(1 / 935.0, 1 / 425.0, 48)
    lg, dvd, rg = t(logits, DEV), t(dv, DEV), t(disp_range, DEV)

    def check(name, d, c):
        check_close(f"soft-argmin depth D={D} {name}", d, want_d, rtol=2e-6, atol=1e-3)
        IR.check_confidence(f"confidence D={D} {name}", c, cs)

    d0, c0 = ops.softmax_regress_conf(lg, dvd)
    check("plain", d0, c0)
    d, c, inv = ops.softmax_regress_conf(lg, dvd, disp_range=rg)
    check("with disp_range", d, c)
    # (the depth's own tolerance, 2e-6 relative + 1e-3 of ~600, carried through d(1/x - lo) / (hi - lo): 2.2e-6 of the unit range)
    check_close(f"normalised inverse depth D={D}", inv, O.depth_to_disp(want_d, 1.0 / disp_range[-1].double(), 1.0 / disp_range[0].double()),
                rtol=1e-5, atol=1e-5)
    for f in (3, 4):
        d, c, up = ops.softmax_regress_conf(lg, dvd, conf_up=f)
        check(f"conf_up={f}", d, c)
        assert torch.equal(up, c.repeat_interleave(f, 0).repeat_interleave(f, 1)), "the replicated confidence is the confidence"
    d, c, inv, up = ops.softmax_regress_conf(lg, dvd, disp_range=rg, conf_up=4)
    check("disp_range + conf_up=4", d, c)
    # sample batch: two samples (the second one the planes reversed), ONE hypothesis tensor shared by both
    lg2 = torch.stack([lg, lg.flip(0)]).contiguous()
    cs2 = IR.confidence_set(logits.flip(0), D)
    want_d2 = (torch.softmax(logits.flip(0).double(), 0) * dv.double().view(D, 1, 1)).sum(0)
    db, cb = ops.softmax_regress_conf(lg2, dvd)
    check("batched, sample 0", db[0], cb[0])
    check_close(f"soft-argmin depth D={D} batched, sample 1", db[1], want_d2, rtol=2e-6, atol=1e-3)
    IR.check_confidence(f"confidence D={D} batched, sample 1", cb[1], cs2)
    db, cb, ub = ops.softmax_regress_conf(lg2, dvd, conf_up=3)
    check("batched conf_up=3, sample 0", db[0], cb[0])
    IR.check_confidence(f"confidence D={D} batched conf_up=3, sample 1", cb[1], cs2)
    assert torch.equal(ub[1], cb[1].repeat_interleave(3, 0).repeat_interleave(3, 1))
