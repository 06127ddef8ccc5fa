"""GPU parity tests, kernel by kernel: HIP path (through the C ABI) vs the CPU oracle on seeded inputs
and vs the golden vectors generated from the reference.  Tolerances are written at each check; the
per-kernel bar from SURVEY.md section 8(d) is allclose(rtol=1e-4, atol=1e-5) unless a comment says why not.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from common import _edge_cameras, build_model, check_close, conv_tol, load_golden, t
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    net, sd = build_model("8,8,8", seed=7, device=DEV)       # weight seed 7 == make_golden.WSEED
    return net, sd


@pytest.fixture(scope="module")
def O():
    from oracle import effi_oracle
    return effi_oracle


def pinned(a, b):
    """The oracle reproduces the reference's CPU result: bitwise in the container that generated the
    fixtures, to a few ulp on another host CPU (different SIMD width / thread count in ATen)."""
    return torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def composed(pm):
    """[1,N,2,4,4] -> list of composed 4x4 [1,4,4] (oracle helper)."""
    from oracle import effi_oracle as Or
    return [Or.compose_projection(pm[:, v]) for v in range(pm.shape[1])]


# ---------------------------------------------------------------------------------------------
def test_library_loaded_and_version():
    from effi_mvs_plus_amd import _lib
    assert _lib.lib().effi_version() >= 100


def test_projection_algebra(O):
    from effi_mvs_plus_amd import ops
    pm = synth.synth_cameras(128, 160, 5)["stage1"]
    rt = ops.compose_rel_proj(t(pm[0], DEV)).cpu()
    P = composed(pm.double())
    for v in range(1, 5):
        rot, trans = O.relative_projection(P[v], P[0])       # fp64 ground truth
        want = torch.cat([rot.reshape(-1), trans.reshape(-1)]).float()
        # fp64 on device, rounded once: must match the fp64 oracle to fp32 rounding
        check_close(f"rel_proj view{v} (vs fp64)", rt[v - 1], want, rtol=2e-7, atol=1e-30)
    # and the reference's own fp32 result lies within its LU rounding noise of ours
    P32 = composed(pm)
    rot, trans = O.relative_projection(P32[1], P32[0])
    check_close("rel_proj view1 (vs fp32 reference algebra)", rt[0], torch.cat([rot.reshape(-1), trans.reshape(-1)]),
                rtol=2e-4, atol=1e-4)


def test_planar_to_nhwc():
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(0)
    for C, h, w in [(32, 16, 20), (16, 37, 41), (8, 64, 80)]:
        xs = [torch.randn(C, h, w, generator=g) for _ in range(3)]
        outs = ops.to_nhwc([t(x, DEV) for x in xs])
        for x, o in zip(xs, outs):
            assert torch.equal(o.cpu(), x.permute(1, 2, 0).contiguous())
    # channels-last input is passed through without a copy
    cl = t(xs[0], DEV).unsqueeze(0).contiguous(memory_format=torch.channels_last)[0]
    o = ops.to_nhwc([cl])[0]
    assert o.data_ptr() == cl.data_ptr() and torch.equal(o.cpu(), xs[0].permute(1, 2, 0))


def test_homo_warp_golden_and_oracle(O):
    from effi_mvs_plus_amd.models.module import homo_warping_new
    g = load_golden("g01_homo_warp.npz")
    proj, eproj = g["proj"], g["eproj"]
    cases = [("uniform depth", g["src1"], proj[1:2], proj[0:1], g["d2"], g["out2"]),
             ("per-pixel depth", g["src2"], proj[2:3], proj[0:1], g["d4"], g["out4"]),
             ("edge: rotated, 21% out of bounds", g["src1"], eproj[1:2], eproj[0:1], g["d2"], g["oute1"]),
             ("edge: camera inside range (z<=0)", g["src2"], eproj[2:3], eproj[0:1], g["d2"], g["oute2"])]
    for name, src, sp, rp, dv, want in cases:
        got = homo_warping_new(t(src, DEV), t(sp, DEV), t(rp, DEV), t(dv, DEV))
        # bilinear taps of O(1) features; coordinates differ from the fp32 reference by ~1e-4 px
        # (its fp32 4x4 inverse), hence atol 2e-4.  A handful of samples sit on the image border where
        # a tap flips in/out of bounds: allow 0.2 %.
        check_close("homo_warping_new " + name, got, want, rtol=1e-4, atol=2e-4, frac_ok=0.998)
        assert pinned(O.homo_warping_new(src, sp, rp, dv), want)              # oracle pinned to the reference


def _oracle_sim_views(O, feats, pm, samples):
    P = composed(pm)
    ref = feats[0]
    C = ref.shape[1]
    sims, ents = [], []
    for v in range(1, len(feats)):
        warped = O.homo_warping_new(feats[v], P[v], P[0], samples)
        D = samples.shape[1]
        warped = warped.view(1, C, D, ref.shape[2], ref.shape[3])
        sim = (warped * ref.unsqueeze(2)).mean(1)
        p = F.softmax(sim, dim=1)
        sims.append(sim[0])
        ents.append((-p * torch.log(p + 1e-7)).sum(1)[0])
    return torch.stack(sims), torch.stack(ents)


@pytest.mark.parametrize("C,h,w,D,N", [(32, 16, 20, 8, 4), (32, 21, 27, 48, 3), (16, 18, 30, 5, 5), (8, 40, 52, 16, 3)])
def test_warpcorr_views(O, C, h, w, D, N):
    from effi_mvs_plus_amd import ops
    feats = synth.smooth_features(N, C, h, w, seed=100 + C)
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"]
    g = torch.Generator().manual_seed(1)
    samples = (425.0 + 510.0 * torch.rand(1, D, h, w, generator=g)) if C == 16 else \
        torch.linspace(425.0, 935.0, D).view(1, D, 1, 1).expand(1, D, h, w)
    want_sim, want_ent = _oracle_sim_views(O, feats, pm, samples)
    nhwc = ops.to_nhwc([t(f[0], DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    sim, ent = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples[0], DEV) if C == 16 else t(samples[0, :, 0, 0], DEV), D)
    check_close(f"warpcorr_views sim C={C} D={D}", sim, want_sim, rtol=1e-4, atol=2e-4, frac_ok=0.998)
    check_close(f"warpcorr_views entropy C={C} D={D}", ent, want_ent, rtol=1e-4, atol=2e-4, frac_ok=0.998)


def _with_env(name, value, fn):
    """Run ``fn`` with the library switch that the environment variable ``name`` initialises (EFFI_X -> option x) set to ``value``
    (None = unset: the built-in rule).  The library reads the environment once per process; afterwards switches go through
    effi_set_option (ops.set_option)."""
    from effi_mvs_plus_amd import ops
    with ops.options(**{name[len("EFFI_"):].lower(): None if value is None else int(value)}):
        return fn()


@pytest.mark.parametrize("kind", ["rig", "rolled", "wide", "inside", "far"])
@pytest.mark.parametrize("h,w,D,N", [(37, 50, 48, 4), (16, 20, 8, 3), (9, 13, 6, 2), (74, 100, 96, 3), (20, 24, 1, 2)])
def test_warpcorr_views_window_kernel(O, kind, h, w, D, N):
    """The stage-1 kernel that serves its taps from an LDS window (C = 32, hypotheses shared by all pixels): (a) against the
    oracle, (b) bit for bit against itself with every chunk forced onto the global-load path (EFFI_WARP_LDS_KB=0) and with a
    window so small that chunks must shrink (8 KB), (c) against the direct-gather kernel (EFFI_WARP_LDS_KB=-1; another summation
    order, so to rounding)."""
    from effi_mvs_plus_amd import ops
    C = 32
    feats = synth.smooth_features(N, C, h, w, seed=300 + h)
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"] if kind == "rig" else _edge_cameras(h, w, N, kind)
    samples = (1.0 / torch.linspace(1 / 935.0, 1 / 425.0, D)) if D > 1 else torch.tensor([600.0])
    want_sim, want_ent = _oracle_sim_views(O, feats, pm, samples.view(1, D, 1, 1).expand(1, D, h, w))
    nhwc = ops.to_nhwc([t(f[0], DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    run = lambda: ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D)       # noqa: E731
    sim, ent = _with_env("EFFI_WARP_LDS_KB", None, run)
    sim_g, ent_g = _with_env("EFFI_WARP_LDS_KB", "0", run)
    sim_s, ent_s = _with_env("EFFI_WARP_LDS_KB", "8", run)
    sim_o, ent_o = _with_env("EFFI_WARP_LDS_KB", "-1", run)
    assert torch.equal(sim, sim_g) and torch.equal(ent, ent_g), "LDS-window and global-load paths of the kernel must agree bitwise"
    assert torch.equal(sim, sim_s) and torch.equal(ent, ent_s), "chunking must not change the result"
    tol = dict(rtol=1e-4, atol=2e-4, frac_ok=0.998)
    if kind == "inside":
        # where Z crosses zero the projection is discontinuous: coordinates near the pole are ill-conditioned in fp32
        tol = dict(rtol=1e-4, atol=2e-4, frac_ok=0.97)
    check_close(f"window kernel sim [{kind} {h}x{w} D={D}]", sim, want_sim, **tol)
    check_close(f"window kernel entropy [{kind} {h}x{w} D={D}]", ent, want_ent, **tol)
    check_close(f"window vs direct-gather kernel sim [{kind}]", sim, sim_o, rtol=1e-5, atol=2e-5, frac_ok=0.999 if kind != "inside" else 0.97)


@pytest.mark.parametrize("kind", ["rig", "rolled", "wide", "inside", "far"])
@pytest.mark.parametrize("h,w,D,N", [(37, 50, 48, 4), (16, 20, 8, 3), (9, 13, 6, 2), (74, 100, 96, 3), (20, 24, 1, 2), (148, 200, 48, 5)])
def test_warpcorr_views_matrix_core_form(O, kind, h, w, D, N):
    """Round 4: in split / bf16 precision the cascade's stage-1 similarity is evaluated CORRELATE FIRST (effi_warpcorr_views_x3_f32):
    G[reference pixel][tap pixel] = sum_c ref * src on the matrix cores (three bf16 partial products per fp32 product, fp32
    accumulation -- the arithmetic of the split convolutions), then the bilinear interpolation of the correlations.  Against the
    oracle with the split convolutions' tolerance (4e-5 of the peak on top of the exact kernel's), against the exact kernel, on the
    rigs that stress the box logic (slanted / huge / behind-the-camera / out-of-view epipolar segments: boxes that do not fit the
    wave's LDS region take the direct fp32 form), on hypotheses in any order, and bit for bit repeatable."""
    from effi_mvs_plus_amd import ops
    if h * w > 20000 and kind not in ("rig", "rolled"):
        pytest.skip("the large map runs on two rigs")
    C = 32
    feats = synth.smooth_features(N, C, h, w, seed=300 + h)
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"] if kind == "rig" else _edge_cameras(h, w, N, kind)
    samples = (1.0 / torch.linspace(1 / 935.0, 1 / 425.0, D)) if D > 1 else torch.tensor([600.0])
    want_sim, want_ent = _oracle_sim_views(O, feats, pm, samples.view(1, D, 1, 1).expand(1, D, h, w))
    nhwc = ops.to_nhwc([t(f[0], DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    before = ops.get_precision()
    try:
        ops.set_precision("split")
        sim, ent = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D, x3=True)
        sim2, ent2 = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D, x3=True)
        sim_e, ent_e = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D)
        perm = torch.randperm(D, generator=torch.Generator().manual_seed(3))
        sim_p, _ = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples[perm], DEV), D, x3=True)
        ops.set_precision("bf16")
        sim_b, ent_b = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D, x3=True)
        ops.set_precision("fp32")
        sim_f, ent_f = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D, x3=True)
    finally:
        ops.set_precision(before)
    assert torch.equal(sim, sim2) and torch.equal(ent, ent2), "repeatable bit for bit"
    assert torch.equal(sim_f, sim_e) and torch.equal(ent_f, ent_e), "exact-fp32 precision keeps the exact kernel"
    peak = float(want_sim.abs().max())
    frac = 0.97 if kind == "inside" else 0.998         # where Z crosses zero the projection is ill-conditioned in fp32 (see the test above)
    check_close(f"matrix-core sim vs oracle [{kind} {h}x{w} D={D}]", sim, want_sim, rtol=1e-4, atol=2e-4 + 4e-5 * peak, frac_ok=frac)
    check_close(f"matrix-core entropy vs oracle [{kind}]", ent, want_ent, rtol=1e-4, atol=2e-4 + 4e-4, frac_ok=frac)
    check_close(f"matrix-core vs exact kernel sim [{kind}]", sim, sim_e, rtol=1e-5, atol=2e-5 + 4e-5 * peak, frac_ok=0.999 if kind != "inside" else 0.97)
    check_close(f"shuffled hypotheses = the sorted result permuted [{kind}]", sim_p, sim.cpu()[:, perm], rtol=1e-5, atol=2e-5 + 4e-5 * peak,
                frac_ok=0.999 if kind != "inside" else 0.97)
    check_close(f"bf16 operands vs exact kernel sim [{kind}]", sim_b, sim_e, rtol=1e-2, atol=1e-2 * max(peak, 1e-3), frac_ok=0.97)


def test_warpcorr_views_window_kernel_accepts_any_order_of_hypotheses(O):
    """The reference accepts depth_values in any order (models/Effi_MVS_plus.py:32-61 never sorts them).  The window kernel bounds a
    chunk's source positions by its two END depths, which holds for monotone hypotheses only: a workgroup that finds them
    non-monotone samples every chunk from global memory.  Shuffled hypotheses: result = the monotone result permuted (the
    similarity of a hypothesis does not depend on its neighbours) and equal to the direct-gather kernel, both to rounding."""
    from effi_mvs_plus_amd import ops
    h, w, D, N, C = 37, 50, 48, 4, 32
    feats = synth.smooth_features(N, C, h, w, seed=77)
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"]
    samples = 1.0 / torch.linspace(1 / 935.0, 1 / 425.0, D)
    perm = torch.randperm(D, generator=torch.Generator().manual_seed(3))
    nhwc = ops.to_nhwc([t(f[0], DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    sim_sorted, _ = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples, DEV), D)
    sim_shuf, ent_shuf = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples[perm], DEV), D)
    # (not bitwise: a hypothesis' channel sum starts at the 8-channel group of the LANE that owns it -- position in the list mod 4)
    check_close("shuffled hypotheses = the sorted result permuted", sim_shuf, sim_sorted.cpu()[:, perm], rtol=1e-5, atol=2e-6)
    with ops.options(warp_lds_kb=-1):
        sim_direct, ent_direct = ops.warpcorr_views(nhwc[0], nhwc[1:], rt, t(samples[perm], DEV), D)
    check_close("shuffled hypotheses, window vs direct-gather kernel", sim_shuf, sim_direct, rtol=1e-5, atol=2e-5, frac_ok=0.999)
    check_close("shuffled hypotheses, entropy", ent_shuf, ent_direct, rtol=1e-4, atol=2e-4, frac_ok=0.998)
    want_sim, _ = _oracle_sim_views(O, feats, pm, samples[perm].view(1, D, 1, 1).expand(1, D, h, w))
    check_close("shuffled hypotheses vs oracle", sim_shuf, want_sim, rtol=1e-4, atol=2e-4, frac_ok=0.998)


@pytest.mark.parametrize("kind", ["rig", "rolled", "wide", "inside"])
@pytest.mark.parametrize("h,w,D,N", [(37, 50, 48, 4), (9, 13, 6, 2), (20, 24, 1, 3)])
def test_warp_correlate_backward_window_kernel(kind, h, w, D, N):
    """The stage-1 backward whose scatter is privatised in an LDS window (C = 32, shared hypotheses) against the direct kernel with
    global atomics (EFFI_WARP_LDS_KB=-1), against itself with every chunk forced onto global atomics (=0) and with windows so
    small that chunks shrink (8 KB): the same gradients to summation-order rounding."""
    from effi_mvs_plus_amd import ops
    C = 32
    feats = synth.smooth_features(N, C, h, w, seed=500 + h)
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"] if kind == "rig" else _edge_cameras(h, w, N, kind)
    samples = (1.0 / torch.linspace(1 / 935.0, 1 / 425.0, D)) if D > 1 else torch.tensor([600.0])
    g = torch.Generator().manual_seed(h)
    G = torch.randn(N - 1, D, h, w, generator=g).to(DEV)
    nhwc = ops.to_nhwc([t(f[0], DEV) for f in feats])
    rt = ops.compose_rel_proj(t(pm[0], DEV))
    run = lambda: ops.warpcorr_views_bwd(nhwc[0], nhwc[1:], rt, t(samples, DEV), D, G)       # noqa: E731
    g_ref, g_src = _with_env("EFFI_WARP_LDS_KB", None, run)
    for mode in ("-1", "0", "8"):
        o_ref, o_src = _with_env("EFFI_WARP_LDS_KB", mode, run)
        tol_ = dict(rtol=1e-4, atol=2e-5 * float(o_ref.abs().max()) + 1e-7)
        check_close(f"bwd window vs mode {mode}: grad_ref [{kind}]", g_ref, o_ref, **tol_)
        for v in range(N - 1):
            check_close(f"bwd window vs mode {mode}: grad_src{v} [{kind}]", g_src[v], o_src[v], rtol=1e-4,
                        atol=2e-5 * float(o_src[v].abs().max()) + 1e-7)


@pytest.mark.parametrize("C,h,w,D,N", [(32, 16, 20, 8, 4), (16, 18, 30, 5, 3), (8, 21, 27, 6, 3)])
def test_warp_correlate_backward_matches_torch_autograd(O, C, h, w, D, N):
    """Scope row n2, first piece: gradients of the stage-1 warp + correlation w.r.t. reference and source features from the HIP
    backward kernel (scatter-add of the bilinear weights) against torch autograd through the oracle's grid_sample formulation."""
    from effi_mvs_plus_amd import autograd as A
    feats = synth.smooth_features(N, C, h, w, seed=200 + C)
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"]
    g = torch.Generator().manual_seed(2)
    samples = (425.0 + 510.0 * torch.rand(1, D, h, w, generator=g)) if C == 16 else \
        torch.linspace(425.0, 935.0, D).view(1, D, 1, 1).expand(1, D, h, w)
    G = torch.randn(N - 1, D, h, w, generator=g)
    # oracle: autograd on the CPU
    leaves = [f.clone().requires_grad_(True) for f in feats]
    P = composed(pm)
    sims = []
    for v in range(1, N):
        warped = O.homo_warping_new(leaves[v], P[v], P[0], samples).view(1, C, D, h, w)
        sims.append((warped * leaves[0].unsqueeze(2)).mean(1)[0])
    want_sim = torch.stack(sims)
    (want_sim * G).sum().backward()
    # HIP: forward + backward kernels behind torch.autograd.Function
    dev_leaves = [f[0].to(DEV).requires_grad_(True) for f in feats]
    dv = t(samples[0], DEV) if C == 16 else t(samples[0, :, 0, 0], DEV)
    sim = A.warp_correlate(dev_leaves[0], dev_leaves[1:], t(pm[0], DEV), dv)
    check_close("warp_correlate forward", sim, want_sim.detach(), rtol=1e-4, atol=2e-4, frac_ok=0.998)
    (sim * t(G, DEV)).sum().backward()
    for v in range(N):
        want = leaves[v].grad[0]
        check_close(f"warp_correlate grad view {v}", dev_leaves[v].grad, want, rtol=1e-3, atol=2e-4 * float(want.abs().max()) + 1e-6,
                    frac_ok=0.998)


@pytest.mark.parametrize("C,h,w,D", [(32, 16, 20, 8), (16, 18, 30, 5), (8, 21, 27, 6)])
def test_homo_warping_new_is_differentiable(O, C, h, w, D):
    """``homo_warping_new`` with a source map that requires grad: HIP forward + HIP backward (scatter-add) against torch autograd
    through the oracle's grid_sample formulation."""
    from effi_mvs_plus_amd.models.module import homo_warping_new
    feats = synth.smooth_features(2, C, h, w, seed=300 + C)
    pm = synth.synth_cameras(h * 8, w * 8, 2)["stage1"]
    P = composed(pm)
    g = torch.Generator().manual_seed(3)
    samples = (425.0 + 510.0 * torch.rand(1, D, h, w, generator=g)) if C == 16 else torch.linspace(425.0, 935.0, D).view(1, D)
    G = torch.randn(1, C, D * h, w, generator=g)
    leaf = feats[1].clone().requires_grad_(True)
    want = O.homo_warping_new(leaf, P[1], P[0], samples)
    (want * G).sum().backward()
    dleaf = t(feats[1], DEV).requires_grad_(True)
    got = homo_warping_new(dleaf, t(P[1], DEV), t(P[0], DEV), t(samples, DEV))
    assert got.requires_grad
    check_close("homo_warping_new forward (autograd form)", got, want.detach(), rtol=1e-4, atol=2e-4, frac_ok=0.998)
    (got * t(G, DEV)).sum().backward()
    check_close("homo_warping_new grad", dleaf.grad, leaf.grad, rtol=1e-3, atol=2e-4 * float(leaf.grad.abs().max()) + 1e-6, frac_ok=0.998)


@pytest.mark.parametrize("form", ["mfma", "valu"])
def test_pixelwise_net(model, O, form):
    """Both kernels of the view-weight net (default: layers 2 / 3 on the fp32 matrix cores; option pixnet_mfma = 0: vector ALU) against
    the reference's vectors and the oracle, also on a map that is not a multiple of the 16 x 16 tile."""
    from effi_mvs_plus_amd import ops
    net, sd = model
    with ops.options(pixnet_mfma=0 if form == "valu" else None):
        g = load_golden("g03_pixelwise.npz")
        got = net.PixelwiseNet(t(g["entropy"], DEV))
        check_close(f"PixelwiseNet (golden, {form})", got, g["weight"], rtol=1e-4, atol=1e-5)
        check_close(f"PixelwiseNet (oracle, {form})", got, O.pixelwise_net(sd, "PixelwiseNet", g["entropy"]), rtol=1e-4, atol=1e-5)
        ent = torch.rand(3, 1, 37, 53, generator=torch.Generator().manual_seed(5)) * 3.0
        check_close(f"PixelwiseNet 37x53 (oracle, {form})", net.PixelwiseNet(t(ent, DEV)), O.pixelwise_net(sd, "PixelwiseNet", ent),
                    rtol=1e-4, atol=1e-5)


def test_view_aggregate():
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(3)
    for S in (1, 4, 10):
        sims, ws = torch.randn(S, 7, 9, 11, generator=g), torch.rand(S, 9, 11, generator=g)
        want = (sims * ws.unsqueeze(1)).sum(0) / (ws.sum(0, keepdim=True) + 1e-6)
        check_close(f"view_aggregate S={S}", ops.view_aggregate(t(sims, DEV), t(ws, DEV)), want, rtol=1e-5, atol=1e-6)


def test_depthnet_module(model, O):
    net, sd = model
    for name in ("g02_depthnet.npz", "g02e_depthnet_edge.npz"):
        g = load_golden(name)
        feats = synth.smooth_features(4, 32, 16, 20, seed=int(g["feat_seed"]))
        samples = g["depth_samples"].view(1, 8, 1, 1).expand(1, 8, 16, 20)
        out = net.depthnet([t(f, DEV) for f in feats], t(g["proj"], DEV), depth_values=samples.to(DEV), num_depth=8,
                           cost_regularization=net.cost_regularization, pixel_wise_net=net.PixelwiseNet, G=1)
        ora = O.depthnet(sd, feats, g["proj"], samples.contiguous(), 8)
        for k in ("volume", "view_weights", "reg_volume", "depth"):
            assert pinned(ora[k], g["out_" + k]) or k == "depth", k               # oracle pinned to the reference
            tol = dict(rtol=1e-4, atol=3e-4) if k != "depth" else dict(rtol=1e-5, atol=2e-2)   # depth in mm (425..935)
            check_close(f"DepthNet.{k} [{name[:4]}]", out[k], g["out_" + k], frac_ok=0.995, **tol)
        # confidence: floor() of the expected index may flip for a few pixels
        check_close(f"DepthNet.confidence [{name[:4]}]", out["photometric_confidence"], g["out_photometric_confidence"],
                    rtol=1e-4, atol=1e-4, frac_ok=0.98)


def test_depthnet_without_view_weight_net(model, O):
    """``pixel_wise_net=None`` (models/Effi_MVS_plus.py:55-58,70): plain mean over the source views, empty ``view_weights``."""
    net, sd = model
    feats = synth.smooth_features(4, 32, 16, 20, seed=2)
    _, pm, _ = synth.synth_sample(128, 160, 4, seed=7)
    proj = pm["stage1"]
    samples = (1.0 / torch.linspace(1 / 935.0, 1 / 425.0, 8)).view(1, 8, 1, 1).expand(1, 8, 16, 20).contiguous()
    out = net.depthnet([t(f, DEV) for f in feats], t(proj, DEV), depth_values=samples.to(DEV), num_depth=8,
                       cost_regularization=net.cost_regularization, pixel_wise_net=None, G=1)
    ora = O.depthnet(sd, feats, proj, samples, 8, pixelwise_prefix=None)
    assert out["view_weights"] == []
    for k in ("volume", "reg_volume", "depth"):
        tol = dict(rtol=1e-4, atol=3e-4) if k != "depth" else dict(rtol=1e-5, atol=2e-2)
        check_close(f"DepthNet(no view-weight net).{k}", out[k], ora[k], frac_ok=0.995, **tol)


# ---------------------------------------------------------------------------------------------
# 3-D convolutions
# ---------------------------------------------------------------------------------------------
def _rand_bn(bn, g):
    bn.weight.data = 0.6 + 0.8 * torch.rand(bn.weight.shape, generator=g)
    bn.bias.data = 0.1 * torch.randn(bn.bias.shape, generator=g)
    bn.running_mean.data = 0.1 * torch.randn(bn.bias.shape, generator=g)
    bn.running_var.data = 0.5 + torch.rand(bn.bias.shape, generator=g)


@pytest.mark.parametrize("cin,cout,stride,dims", [
    (1, 8, 1, (8, 16, 20)), (8, 8, 1, (12, 18, 44)), (16, 16, 1, (6, 9, 35)), (32, 32, 1, (3, 10, 13)),
    (8, 16, 2, (12, 20, 36)), (16, 32, 2, (6, 10, 18)), (8, 16, 2, (8, 14, 70)), (1, 8, (1, 2, 2), (8, 24, 40)),
    (1, 8, (1, 2, 2), (5, 18, 66)),
    # matrix-core path (cout 16/32, stride 1): aligned and unaligned rows, every rows-per-wave variant, real U-Net shapes
    (16, 16, 1, (6, 12, 40)), (32, 32, 1, (4, 8, 52)), (16, 16, 1, (24, 74, 100)), (32, 32, 1, (12, 37, 50)),
    (16, 16, 1, (48, 40, 64)), (8, 8, 1, (8, 37, 48)), (1, 8, 1, (8, 148, 200)),
    (8, 8, 1, (48, 148, 200)), (8, 16, 1, (7, 30, 52)), (16, 32, 1, (5, 20, 36)),
    # rolling-window kernel at degenerate depths / tiny maps (runs of 1..3 planes, tiles larger than the map)
    (8, 8, 1, (1, 8, 12)), (16, 8, 1, (2, 5, 8)), (16, 16, 1, (3, 9, 16)), (8, 16, 1, (5, 4, 4)),
    # stride-2 levels on the matrix cores: real U-Net shapes and odd sizes
    (8, 16, 2, (48, 148, 200)), (16, 32, 2, (24, 74, 100)), (8, 16, 2, (7, 15, 21)), (16, 32, 2, (5, 9, 34))])
def test_conv3d_block(cin, cout, stride, dims, precision):
    from effi_mvs_plus_amd.models.module import Conv3d
    g = torch.Generator().manual_seed(cin * 100 + cout)
    m = Conv3d(cin, cout, stride=stride, padding=1).eval()
    m.conv.weight.data = torch.randn(m.conv.weight.shape, generator=g) * (2.0 / (27 * cin)) ** 0.5
    _rand_bn(m.bn, g)
    x = torch.randn(1, cin, *dims, generator=g)
    want = F.relu(m.bn(m.conv(x)))
    got = m.to(DEV)(t(x, DEV))
    check_close(f"Conv3d {cin}->{cout} s={stride} {dims}", got, want, **conv_tol(precision, want, 1e-4, 1e-5))


@pytest.mark.parametrize("dims", [(8, 20, 24), (8, 74, 100), (5, 148, 200)])
def test_conv3d_two_sources(dims, precision):
    """cost_up_small.conv1 (models/module.py:513-514): the channel concatenation is read in place from two tensors."""
    from effi_mvs_plus_amd.models.module import Conv3d
    g = torch.Generator().manual_seed(dims[1])
    m = Conv3d(16, 8, padding=1).eval()
    m.conv.weight.data = torch.randn(m.conv.weight.shape, generator=g) * (2.0 / (27 * 16)) ** 0.5
    _rand_bn(m.bn, g)
    a, b = torch.randn(8, *dims, generator=g), torch.randn(8, *dims, generator=g)
    want = F.relu(m.bn(m.conv(torch.cat([a, b]).unsqueeze(0))))[0]
    got = m.to(DEV).run([t(a, DEV), t(b, DEV)])
    check_close(f"Conv3d [8+8]->8 {dims}", got, want, **conv_tol(precision, want, 1e-4, 1e-5))


@pytest.mark.parametrize("cin,cout,stride,dims,skip", [
    (32, 16, 2, (3, 5, 7), True), (16, 8, 2, (6, 10, 37), True), (16, 8, 2, (4, 9, 33), False),
    (8, 1, (1, 2, 2), (8, 12, 20), False), (8, 1, (1, 2, 2), (5, 9, 35), False),
    # real U-Net shapes (unaligned and aligned rows, both rows-per-wave variants of the matrix-core kernel)
    (32, 16, 2, (12, 37, 50), True), (16, 8, 2, (24, 74, 100), True), (16, 16, 2, (5, 13, 24), False),
    (16, 8, 2, (1, 1, 1), True), (32, 8, 2, (2, 3, 5), False), (16, 16, 2, (3, 17, 19), True)])
def test_deconv3d_block(cin, cout, stride, dims, skip, precision):
    from effi_mvs_plus_amd.models.module import Deconv3d
    g = torch.Generator().manual_seed(cin * 10 + cout)
    op = 1 if stride == 2 else (0, 1, 1)
    m = Deconv3d(cin, cout, stride=stride, padding=1, output_padding=op).eval()
    m.conv.weight.data = torch.randn(m.conv.weight.shape, generator=g) * (8.0 / (27 * cin)) ** 0.5
    _rand_bn(m.bn, g)
    x = torch.randn(1, cin, *dims, generator=g)
    want = F.relu(m.bn(m.conv(x)))
    m = m.to(DEV)
    if skip:
        sk = torch.randn(want.shape, generator=g)
        got = m.run(t(x[0], DEV), skip=t(sk[0], DEV)).unsqueeze(0)
        want = sk + want
    else:
        got = m(t(x, DEV))
    check_close(f"Deconv3d {cin}->{cout} s={stride} {dims} skip={skip}", got, want, **conv_tol(precision, want, 1e-4, 1e-5))


def test_costregnet_and_cost_up_small(model, O):
    net, sd = model
    g = load_golden("g04_costreg.npz")
    prob, pro = net.cost_regularization(t(g["vol"], DEV))
    # nine chained layers, all but the first and the last on the matrix cores in split precision (default mode): 1e-5 of the peak
    check_close("CostRegNet.prob (golden)", prob, g["prob"], rtol=1e-4, atol=6e-5)
    check_close("CostRegNet.pro (golden)", pro, g["pro"], rtol=1e-4, atol=6e-5)
    op, opro = O.cost_regnet(sd, "cost_regularization", g["vol"])
    assert pinned(op, g["prob"]) and pinned(opro, g["pro"])
    g = load_golden("g05_cost_up_small.npz")
    c2, c1 = net.CSP_R[0](t(g["x"], DEV), t(g["prior"], DEV))
    check_close("cost_up_small.conv2 (golden)", c2, g["conv2"], rtol=1e-4, atol=2e-5)
    check_close("cost_up_small.conv1 (golden)", c1, g["conv1"], rtol=1e-4, atol=2e-5)
    o2, o1 = O.cost_up_small(sd, "CSP_R.0", g["x"], g["prior"])
    assert pinned(o2, g["conv2"]) and pinned(o1, g["conv1"])


@pytest.mark.parametrize("dims", [(8, 36, 48), (8, 74, 100), (5, 20, 24)])
def test_cost_up_small_pair_equals_two_single_runs(dims):
    """CSP_R / CSP_C of a stage with every layer of the two blocks in one launch (effi_*_pair_f32) give the bits of the two
    separate runs, and so does the paired lookup."""
    import contextlib
    import io
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.module import cost_up_small
    D, h, w = dims
    g = torch.Generator().manual_seed(D * 100 + h)
    blocks = []
    for seed in (3, 4):
        with contextlib.redirect_stdout(io.StringIO()):
            m = cost_up_small(in_channels=1, base_channels=8).eval()
        m.load_state_dict(synth.randomize_state_dict(m.state_dict(), seed=seed))
        blocks.append(m.to(DEV))
    a, b = blocks
    x = torch.randn(1, D, 2 * h, 2 * w, generator=g).to(DEV)
    pa, pb = torch.randn(1, D, h, w, generator=g).to(DEV), torch.randn(1, D, h, w, generator=g).to(DEV)
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        assert cost_up_small.pairable(a, b, x, w) == (w % 4 == 0)
        if w % 4 == 0:
            (oa, ca), (ob, cb) = cost_up_small.run_pair(a, b, x, pa, pb)
            ra, rb = a.run(x, pa), b.run(x, pb)
            assert torch.equal(oa, ra[0]) and torch.equal(ca, ra[1]) and torch.equal(ob, rb[0]) and torch.equal(cb, rb[1])
    finally:
        ops.set_precision(before)


@pytest.mark.parametrize("dims,odd", [((8, 36, 48), False), ((8, 37, 52), True), ((8, 74, 100), False), ((3, 9, 20), True), ((14, 16, 16), False)])
@pytest.mark.parametrize("precision_", ["split", "bf16"])
def test_cost_up_small_generated_inputs_are_bitwise_the_three_launches(dims, odd, precision_):
    """conv0 | conv_cost generated inside conv1's rolling window (effi_csp_gen_roll_bf16x3_pair_f32, option csp_gen) against the
    three launches it replaces (effi_conv3d_k3_pair_f32 with stride (1,2,2) and (1,1,1), effi_conv3d_k3s1_roll_bf16x3_pair_f32):
    the same bits, ragged tiles, odd fine sizes (H = 2h - 1) and the largest supported depth included."""
    import contextlib
    import io
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.module import cost_up_small
    D, h, w = dims
    g = torch.Generator().manual_seed(D * 1000 + h * 10 + int(odd))
    blocks = []
    for seed in (5, 6):
        with contextlib.redirect_stdout(io.StringIO()):
            m = cost_up_small(in_channels=1, base_channels=8).eval()
        m.load_state_dict(synth.randomize_state_dict(m.state_dict(), seed=seed))
        blocks.append(m.to(DEV))
    a, b = blocks
    H, W = (2 * h - 1, 2 * w - 1) if odd else (2 * h, 2 * w)
    x = torch.randn(1, D, H, W, generator=g).to(DEV)
    pa, pb = torch.randn(1, D, h, w, generator=g).to(DEV), torch.randn(1, D, h, w, generator=g).to(DEV)
    before, gen0 = ops.get_precision(), ops.option("csp_gen")
    ops.set_precision(precision_)
    try:
        (w0a, b0a), (w0b, b0b) = a.conv0._packed(), b.conv0._packed()
        (wca, bca), (wcb, bcb) = a.conv_cost._packed(), b.conv_cost._packed()
        (w1a, b1a), (w1b, b1b) = a._roll_packed(), b._roll_packed()
        fa, fb = ops.conv3d_k3_pair(x, w0a, b0a, x, w0b, b0b, 8, sxy=2, relu=True)
        ga, gb = ops.conv3d_k3_pair(pa, wca, bca, pb, wcb, bcb, 8, sxy=1, relu=True)
        want_a, want_b = ops.conv3d_k3s1_roll_pair([fa, ga], w1a, b1a, [fb, gb], w1b, b1b, 8, relu=True)
        got_a, got_b = ops.csp_gen_roll_pair(x, pa, w0a, b0a, wca, bca, w1a, b1a, pb, w0b, b0b, wcb, bcb, w1b, b1b)
        torch.cuda.synchronize()
        assert torch.isfinite(got_a).all() and want_a.abs().max() > 0
        assert torch.equal(got_a, want_a), f"block a: {(got_a - want_a).abs().max().item():.3e}"
        assert torch.equal(got_b, want_b), f"block b: {(got_b - want_b).abs().max().item():.3e}"
        if not odd:                                   # the module path picks the fused form by default and the launches with csp_gen = 0
            (o1, c1), _ = cost_up_small.run_pair(a, b, x, pa, pb)
            ops.set_option("csp_gen", 0)
            (o0, c0), _ = cost_up_small.run_pair(a, b, x, pa, pb)
            assert torch.equal(c1, c0) and torch.equal(o1, o0) and torch.equal(c1, want_a)
    finally:
        ops.set_option("csp_gen", gen0)
        ops.set_precision(before)
    # paired lookup: same queries into two volumes
    Dp = 11
    va, vb = torch.rand(Dp, h, w, generator=g).to(DEV), torch.rand(Dp, h, w, generator=g).to(DEV)
    q = (0.002 + 0.001 * torch.rand(D, 2 * h, 2 * w, generator=g)).to(DEV)
    lo, hi = torch.tensor([1 / 0.0035]).to(DEV), torch.tensor([1 / 0.0015]).to(DEV)
    la, lb = ops.vol_lookup1d_pair(va, vb, q, lo, hi, h, w)
    assert torch.equal(la, ops.vol_lookup1d(va, q, lo, hi, h, w)) and torch.equal(lb, ops.vol_lookup1d(vb, q, lo, hi, h, w))


def test_softmax_regress_conf(O):
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(9)
    for D, h, w in [(8, 16, 20), (48, 13, 17), (5, 7, 9)]:
        logits = 2.0 * torch.randn(1, D, h, w, generator=g)
        dv = torch.linspace(425.0, 935.0, D).view(1, D, 1, 1).expand(1, D, h, w).contiguous()
        p = F.softmax(logits, dim=1)
        want_d = O.depth_regression(p, dv)
        s4 = 4 * F.avg_pool3d(F.pad(p.unsqueeze(1), pad=(0, 0, 0, 0, 1, 2)), (4, 1, 1), stride=1, padding=0).squeeze(1)
        idx = O.depth_regression(p, torch.arange(D, dtype=torch.float32)).long().clamp(0, D - 1)
        want_c = torch.gather(s4, 1, idx.unsqueeze(1)).squeeze(1)
        d, c = ops.softmax_regress_conf(t(logits[0], DEV), t(dv[0], DEV))
        check_close(f"soft-argmin depth D={D}", d, want_d[0], rtol=2e-6, atol=1e-3)
        check_close(f"confidence D={D}", c, want_c[0], rtol=1e-4, atol=1e-5, frac_ok=0.99)   # floor() flips


# ---------------------------------------------------------------------------------------------
# lookups and the dynamic volume
# ---------------------------------------------------------------------------------------------
def test_vol_lookup(O):
    from effi_mvs_plus_amd.models.Effi_MVS_plus import pro_bilinear_sampler
    g = load_golden("g07_lookup.npz")
    vol = t(g["vol"], DEV)
    h, w = vol.shape[-2:]
    pro = vol.permute(0, 2, 3, 1).reshape(h * w, 1, 1, vol.shape[1])           # zero-copy strided view
    got = pro_bilinear_sampler(pro, t(g["query"], DEV), t(g["gmin"], DEV), t(g["gmax"], DEV))
    check_close("pro_bilinear_sampler global range (golden)", got, g["out_global"], rtol=1e-4, atol=2e-5)
    got = pro_bilinear_sampler(pro.contiguous(), t(g["query"], DEV), t(g["pmin"], DEV), t(g["pmax"], DEV))
    check_close("pro_bilinear_sampler per-pixel range (golden)", got, g["out_pixel"], rtol=1e-4, atol=2e-5)
    frac_oor = float((g["out_global"] == 0).float().mean())
    assert frac_oor > 0.05, "fixture must exercise out-of-range queries"
    want = O.volume_lookup_1d_explicit(g["vol"], g["query"], g["pmin"], g["pmax"])
    check_close("explicit-lerp restatement == grid_sample form", want, g["out_pixel"], rtol=1e-5, atol=1e-6)


def test_bilinear_sampler_matches_golden_lookup(O):
    """``bilinear_sampler`` (reference Effi_MVS_plus.py:102-117) called as ``pro_bilinear_sampler`` calls it (:121-130) reproduces the
    golden lookup g07 (made by the reference), incl. its out-of-range queries; the mask follows :113."""
    from effi_mvs_plus_amd.models.Effi_MVS_plus import bilinear_sampler
    g = load_golden("g07_lookup.npz")
    vol, q = g["vol"], g["query"]
    b, D, h, w = vol.shape
    d = q.shape[1]
    pro = vol.permute(0, 2, 3, 1).reshape(b * h * w, 1, 1, D).contiguous()
    for lo, hi, want, name in ((g["gmin"], g["gmax"], g["out_global"], "global"), (g["pmin"], g["pmax"], g["out_pixel"], "per-pixel")):
        disp = O.depth_to_disp(q, lo, hi) * (D - 1)                                   # :123, plain tensor algebra on the CPU
        x0 = disp.permute(0, 2, 3, 1).reshape(b * h * w, 1, d, 1)
        coords = torch.cat([x0, torch.zeros_like(x0)], dim=-1)
        got, mask = bilinear_sampler(t(pro, DEV), t(coords, DEV), mask=True)
        assert tuple(got.shape) == (b * h * w, 1, 1, d) and tuple(mask.shape) == (b * h * w, 1, d, 1)
        got = got.reshape(b, h, w, d).permute(0, 3, 1, 2)
        check_close(f"bilinear_sampler {name} range (golden)", got, want, rtol=1e-4, atol=2e-5)
        xg = 2 * coords[..., :1] / (D - 1) - 1
        want_mask = ((xg > -1) & (xg < 1)).float()                                     # ygrid == 0 passes its two tests
        assert torch.equal(mask.cpu(), want_mask)
        assert torch.equal(bilinear_sampler(t(pro, DEV), t(coords, DEV)).cpu(), got.permute(0, 2, 3, 1).reshape(b * h * w, 1, 1, d).cpu())
    with pytest.raises(AssertionError):
        bilinear_sampler(torch.zeros(1, 1, 2, 4, device=DEV), torch.zeros(1, 1, 3, 2, device=DEV))   # H != 1: "a stereo problem"


def test_getcost_initvolume(model, O):
    net, sd = model
    g = load_golden("g06_initvolume.npz")
    N, C, h, w = int(g["N"]), int(g["C"]), int(g["h"]), int(g["w"])
    feats = synth.smooth_features(N, C, h, w, seed=int(g["feat_seed"]))
    sim, smp = net.GetCost_initvolume(t(g["cur_depth"], DEV), features=[t(f, DEV) for f in feats], proj_matrices=t(g["proj"], DEV),
                                      depth_interval=t(g["interval"], DEV), depth_max=None, depth_min=None,
                                      view_weights=t(g["view_weights"], DEV), CostNum=8, Inverse=True, G=1)
    check_close("GetCost_initvolume.samples (golden)", smp, g["samples"], rtol=2e-6, atol=0)
    check_close("GetCost_initvolume.similarity (golden)", sim, g["similarity"], rtol=1e-4, atol=3e-4, frac_ok=0.995)
    osim, osmp = O.getcost_initvolume(g["cur_depth"], feats, g["proj"], g["interval"], g["view_weights"], 8)
    assert pinned(osim, g["similarity"]) and pinned(osmp, g["samples"])
    # low-resolution view weights (what the cascade passes) give the same result as pre-upsampled ones
    vw_lo = g["view_weights"][:, :, ::2, ::2].contiguous()
    vw_up = F.interpolate(vw_lo, scale_factor=2, mode="nearest")
    a = net.GetCost_initvolume(t(g["cur_depth"], DEV), features=[t(f, DEV) for f in feats], proj_matrices=t(g["proj"], DEV),
                               depth_interval=t(g["interval"], DEV), depth_max=None, depth_min=None,
                               view_weights=t(vw_lo, DEV), CostNum=8, Inverse=True, G=1)[0]
    b = net.GetCost_initvolume(t(g["cur_depth"], DEV), features=[t(f, DEV) for f in feats], proj_matrices=t(g["proj"], DEV),
                               depth_interval=t(g["interval"], DEV), depth_max=None, depth_min=None,
                               view_weights=t(vw_up, DEV), CostNum=8, Inverse=True, G=1)[0]
    assert torch.equal(a, b)


def test_getcost_initvolume_kernel_forms_agree(model):
    """The stage-2/3 warp + correlation has a default form (a lane owns whole hypotheses, cheap projection) and switchable ones
    (option dyn_form = 1: lanes split the channels; dyn_setup_exact = 1: the reference's IEEE divisions op for op): every form
    meets the golden vectors, and the forms agree far inside that tolerance.  No form passes a tap set-up between lanes."""
    from effi_mvs_plus_amd import ops
    net, sd = model
    g = load_golden("g06_initvolume.npz")
    N, C, h, w = int(g["N"]), int(g["C"]), int(g["h"]), int(g["w"])
    feats = synth.smooth_features(N, C, h, w, seed=int(g["feat_seed"]))

    def run():
        return net.GetCost_initvolume(t(g["cur_depth"], DEV), features=[t(f, DEV) for f in feats], proj_matrices=t(g["proj"], DEV),
                                      depth_interval=t(g["interval"], DEV), depth_max=None, depth_min=None,
                                      view_weights=t(g["view_weights"], DEV), CostNum=8, Inverse=True, G=1)
    out = {}
    for name, opts in (("default", {}), ("lanes", {"dyn_form": 1}), ("exact", {"dyn_setup_exact": 1})):
        with ops.options(dyn_form=None, dyn_setup_exact=None), ops.options(**opts):
            sim, smp = run()
            torch.cuda.synchronize()
        out[name] = (sim.clone(), smp.clone())
        check_close(f"GetCost_initvolume.samples ({name})", smp, g["samples"], rtol=2e-6, atol=0)
        check_close(f"GetCost_initvolume.similarity ({name})", sim, g["similarity"], rtol=1e-4, atol=3e-4, frac_ok=0.995)
    peak = float(out["exact"][0].abs().max())
    for name in ("default", "lanes"):
        assert torch.equal(out[name][1], out["exact"][1]), "the hypotheses do not depend on the form"
        diff = float((out[name][0] - out["exact"][0]).abs().max())
        print(f"similarity, form {name} vs exact: max abs diff {diff:.3e} (peak {peak:.3e})")
        assert diff <= 2e-5 * max(peak, 1.0), (name, diff, peak)


@pytest.mark.parametrize("C,h,w,S,D", [(8, 74, 100, 4, 8), (16, 37, 50, 4, 8), (8, 64, 96, 1, 8), (16, 70, 90, 6, 8), (8, 33, 47, 10, 6),
                                        (16, 24, 40, 3, 4)])
def test_warpcorr_dyn_window_form_is_bitwise_the_gather_form(C, h, w, S, D):
    """Round 4: the stage-2/3 warp + correlation serves its taps from an LDS window per (tile, view) (warpcorr_dyn_win_kernel, the
    default for C = 8 / 16, D <= 8) instead of gathering them through the L1.  Same arithmetic in the same order: the similarities
    are BITWISE those of the gather kernel (option dyn_win = -1) -- with the full window, with a window too small for most tiles
    (dyn_win = 48: views of one tile mix LDS and global sampling), with none (dyn_win = 0), on smooth depth (every window fits) and
    on noisy depth with jumps (boxes overflow), on maps that are not multiples of the tile, from 1 to 10 source views."""
    from effi_mvs_plus_amd import ops
    N = S + 1
    pm = synth.synth_cameras(8 * h, 8 * w, N)["stage3"][0]      # the ring of cameras; intrinsics set for THIS map below
    feats = synth.smooth_features(N, C, h, w, seed=11)
    nhwc = ops.to_nhwc([f[0].to(DEV).contiguous() for f in feats])
    pmd = pm.clone()
    pmd[:, 1, 0, 0] = pmd[:, 1, 1, 1] = 1.1 * w
    pmd[:, 1, 0, 2], pmd[:, 1, 1, 2] = w / 2.0, h / 2.0
    rt = ops.compose_rel_proj(pmd.to(DEV).contiguous())
    g = torch.Generator().manual_seed(5)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    smooth = 600.0 + 40.0 * torch.sin(xs / 17.0) + 30.0 * torch.cos(ys / 11.0)
    noisy = smooth + 25.0 * torch.randn(h, w, generator=g)
    noisy[h // 3: h // 3 + 5, :] = 430.0                        # a depth jump through tiles
    noisy[:, w // 2] = 930.0
    vh, vw = (h // 2, w // 2) if h % 2 == 0 and w % 2 == 0 else (h, w)
    vweights = (0.2 + torch.rand(S, vh, vw, generator=g)).to(DEV)
    itv = torch.tensor([2.0e-5], device=DEV)
    for name, cur in (("smooth", smooth), ("noisy", noisy)):
        cur = cur.to(DEV).contiguous()
        out = {}
        for tag, val in (("gather", -1), ("window", None), ("window48", 48), ("window0", 0)):
            with ops.options(dyn_win=val):
                sim, smp = ops.warpcorr_dyn(nhwc[0], nhwc[1:], rt, cur, itv, vweights, D)
                torch.cuda.synchronize()
            out[tag] = (sim.clone(), smp.clone())
            assert torch.isfinite(sim).all()
        assert float(out["gather"][0].abs().max()) > 1e-3
        for tag in ("window", "window48", "window0"):
            nd = int((out[tag][0] != out["gather"][0]).sum())
            assert nd == 0, f"{name}: {tag} differs from the gather kernel in {nd} similarities"
            assert torch.equal(out[tag][1], out["gather"][1]), f"{name}: {tag} hypotheses differ"


# ---------------------------------------------------------------------------------------------
# GRU update block
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [1, 2, 3])
def test_update_block_parts(model, O, stage, precision):
    import sys
    import effi_mvs_plus_amd.models  # noqa: F401
    M = sys.modules["effi_mvs_plus_amd.models.Effi_MVS_plus"]     # the package attribute of that name is the class
    net, sd = model
    g = load_golden(f"g08_update_stage{stage}.npz")
    blk = net.update_block[stage - 1]
    dv = g["depth_values"]
    h, w = g["inv0"].shape[-2:]
    reg, cur = t(g["reg"], DEV), t(g["cur"], DEV)
    D = reg.shape[1]
    pro = [reg.permute(0, 2, 3, 1).reshape(h * w, 1, 1, D), cur.permute(0, 2, 3, 1).reshape(h * w, 1, 1, D)]
    dvd = t(dv, DEV)
    disp_min, disp_max = dvd[:, 0, None, None, None], dvd[:, -1, None, None, None]
    scale = functools.partial(M.disp_to_depth, min_depth=1.0 / disp_max, max_depth=1.0 / disp_min)
    scale.effi_disp_range = dvd
    costf = functools.partial(net.GetCost, pro=pro, features=[reg], proj_matrices=None, depth_interval=t(g["interval"], DEV),
                              depth_max=disp_max, depth_min=disp_min, view_weights=None, CostNum=3, Inverse=True, G=1,
                              depth_max_cur_volume=t(g["rmax"], DEV), depth_min_cur_volume=t(g["rmin"], DEV))
    inv0, h0, ctx = t(g["inv0"], DEV), t(g["net"], DEV), t(g["ctx"], DEV)
    depth0 = scale(inv0)[1]
    cost = costf(depth0, iter=0)
    check_close(f"GetCost st{stage} (golden)", cost, g["cost"], rtol=1e-4, atol=2e-5, frac_ok=0.999)
    # lookup + convc1 + ReLU in one kernel (the fused GRU path) against conv1x1 of the golden cost
    lookup = net.GetCost.make_lookup(0, disp_range=dvd, **costf.keywords)
    wc1, bc1 = blk.encoder.convc1_raw()
    cor1 = lookup.conv1x1(inv0[0], wc1, bc1, blk.encoder.convc1.out_channels)
    want_cor1 = F.relu(F.conv2d(g["cost"], sd[f"update_block.{stage - 1}.encoder.convc1.weight"],
                                sd[f"update_block.{stage - 1}.encoder.convc1.bias"]))[0]
    check_close(f"GetCost+convc1 st{stage} (golden)", cor1, want_cor1, rtol=1e-4, atol=2e-5, frac_ok=0.999)
    # ... and the one-launch form that also produces relu(convd1(inv)): the same arithmetic as the two separate kernels
    from effi_mvs_plus_amd import ops as _ops
    hd_ = blk.encoder.convc1.out_channels
    w7, b7 = blk.encoder.conv7_packed()
    both_c, both_d = lookup.encoder_inputs(inv0[0], wc1, bc1, w7, b7, hd_)
    assert torch.equal(both_c, cor1)
    assert torch.equal(both_d, _ops.conv2d_c1k7_relu(inv0[0], w7, b7, hd_))
    want_d1 = F.relu(F.conv2d(g["inv0"], sd[f"update_block.{stage - 1}.encoder.convd1.weight"],
                              sd[f"update_block.{stage - 1}.encoder.convd1.bias"], padding=3))[0]
    check_close(f"convd1 st{stage} (torch)", both_d, want_d1, rtol=1e-4, atol=2e-5)
    enc = blk.encoder(inv0, t(g["cost"], DEV), ctx)
    ct = lambda want, layers=1: conv_tol(precision, want, 1e-4, 2e-5, layers)  # noqa: E731
    check_close(f"ProjectionInput st{stage} (golden)", enc, g["enc"], **ct(g["enc"], 3))
    hnew = blk.depth_gru(h0, t(g["enc"], DEV))
    check_close(f"ConvGRU st{stage} (golden)", hnew, g["hnew"], **ct(g["hnew"], 2))
    delta = blk.depth_head(t(g["hnew"], DEV))
    check_close(f"DepthHead st{stage} (golden)", delta, g["delta"], **ct(g["delta"], 2))
    mask = blk.run_mask(t(g["hnew"][0], DEV)).unsqueeze(0)
    check_close(f"mask head st{stage} (golden)", mask, g["mask"], **ct(g["mask"], 2))
    up = M.upsample_depth(inv0, t(g["mask"], DEV), ratio=2)
    check_close(f"upsample_depth st{stage} (golden)", up, g["up"], rtol=1e-4, atol=1e-6)
    # full 3-iteration rollout through the public forward (fused path, reference-style partials)
    n_out, masks, invs = blk(h0, costf, inv0, ctx, seq_len=3, scale_inv_depth=scale)
    check_close(f"BasicUpdateBlock.net st{stage} (golden)", n_out, g["blk_net"], rtol=1e-3, atol=2e-4)
    check_close(f"BasicUpdateBlock.mask st{stage} (golden)", masks[-1], g["blk_mask"], rtol=1e-3, atol=2e-4)
    check_close(f"BasicUpdateBlock.inv st{stage} (golden)", torch.stack(invs), g["blk_inv"], **ct(g["blk_inv"], 8))
    assert masks[0] is invs[0] or torch.equal(masks[0], invs[0])            # non-final mask slots hold inv_depth
    # generic path (callables that are not ours): same kernels through GetCost.forward
    gen_scale = lambda d: M.disp_to_depth(d, 1.0 / disp_max, 1.0 / disp_min)  # noqa: E731
    n2, m2, i2 = blk(h0, lambda d, iter=0: costf(d, iter=iter), inv0, ctx, seq_len=3, scale_inv_depth=gen_scale)
    check_close(f"BasicUpdateBlock generic path st{stage}", torch.stack(i2), g["blk_inv"], **ct(g["blk_inv"], 8))
    # oracle pinned to the reference on the same fixture
    o_min, o_max = 1.0 / dv[:, -1, None, None, None], 1.0 / dv[:, 0, None, None, None]
    opro = [g["reg"].permute(0, 2, 3, 1).reshape(h * w, 1, 1, D), g["cur"].permute(0, 2, 3, 1).reshape(h * w, 1, 1, D)]
    ocost = O.getcost(O.disp_to_depth(g["inv0"], o_min, o_max)[1], opro, g["interval"], 3, g["rmax"], g["rmin"], [1, h, w])
    assert pinned(ocost, g["cost"])
    assert pinned(O.conv_gru(sd, f"update_block.{stage - 1}.depth_gru", g["net"], g["enc"]), g["hnew"])


@pytest.mark.parametrize("ks,cins,cout,act", [(3, (5,), 7, 1), (3, (16, 16), 36, 0), (1, (6,), 48, 1), (1, (36, 12), 48, 1),
                                              (3, (48,), 96, 1), (1, (96,), 36, 0), (3, (17, 3, 9), 20, 3), (3, (64,), 64, 2)])
def test_conv2d_generic(ks, cins, cout, act):
    """MFMA conv against F.conv2d for odd channel counts / image sizes / multi-source inputs."""
    from effi_mvs_plus_amd import ops, packing
    g = torch.Generator().manual_seed(ks * 1000 + cout)
    h, w = 21, 30                                     # not multiples of the 16x16 tile, w % 4 != 0
    xs = [torch.randn(c, h, w, generator=g) for c in cins]
    cin = sum(cins)
    wt = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    y = F.conv2d(torch.cat(xs).unsqueeze(0), wt, b, padding=ks // 2)[0]
    want = [y, F.relu(y), torch.sigmoid(y), torch.tanh(y)][act]
    wp, bp = packing.pack_conv2d_mfma(wt.to(DEV), b.to(DEV))
    got = ops.conv2d([t(x, DEV) for x in xs], wp, bp, cout, ks, act=act)
    check_close(f"conv2d k{ks} {cins}->{cout} act{act}", got, want, rtol=1e-4, atol=1e-5)
    # w % 4 == 0 takes the vectorised store path
    xs2 = [x[:, :, :28].contiguous() for x in xs]
    y2 = F.conv2d(torch.cat(xs2).unsqueeze(0), wt, b, padding=ks // 2)[0]
    want2 = [y2, F.relu(y2), torch.sigmoid(y2), torch.tanh(y2)][act]
    got2 = ops.conv2d([t(x, DEV) for x in xs2], wp, bp, cout, ks, act=act)
    check_close(f"conv2d k{ks} {cins}->{cout} act{act} (w=28)", got2, want2, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("h,w", [(21, 28), (130, 256), (256, 512)])      # rows-per-wave 1, 2 and 4
@pytest.mark.parametrize("cins,cout,epi", [((5,), 7, 0), ((16,), 16, 0), ((16, 16), 12, 0), ((24, 8, 12), 20, 0), ((48,), 48, 5),
                                           ((16, 16), 32, 1), ((48, 48), 96, 1), ((32, 32), 32, 2), ((64,), 64, 0)])
def test_conv2d_split_bf16(h, w, cins, cout, epi):
    """Split-precision (bf16x3) 3x3 conv against an fp64 F.conv2d: every product carries ~2^-16 relative error, so the
    result must sit within 3e-5 of the fp64 value relative to the output scale (fp32 MFMA path: ~1e-6), all epilogues."""
    from effi_mvs_plus_amd import ops, packing
    g = torch.Generator().manual_seed(cout * 100 + h)
    xs = [torch.randn(c, h, w, generator=g) for c in cins]
    cin = sum(cins)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    y = F.conv2d(torch.cat(xs).unsqueeze(0).double(), wt.double(), b.double(), padding=1)[0]
    wp, bp = packing.pack_conv2d_bf16x3(wt.to(DEV), b.to(DEV))
    dx = [t(x, DEV) for x in xs]
    tol = dict(rtol=0.0, atol=3e-5 * float(y.abs().max()))
    if epi == 0:
        got = ops.conv2d_k3_bf16x3(dx, wp, bp, cout, act=1)
        check_close("bf16x3 plain", got, F.relu(y).float(), **tol)
    elif epi == 5:
        got = ops.conv2d_k3_bf16x3(dx, wp, bp, cout, epilogue=ops.EPI_NHWC, act=0)
        check_close("bf16x3 nhwc", got, y.permute(1, 2, 0).float(), **tol)
    elif epi == 1:
        hd = cout // 2
        hprev = torch.randn(hd, h, w, generator=g)
        z, rh = ops.conv2d_k3_bf16x3(dx, wp, bp, cout, epilogue=ops.EPI_GRU_ZR, aux0=t(hprev, DEV))
        check_close("bf16x3 z", z, torch.sigmoid(y[:hd]).float(), **tol)
        check_close("bf16x3 r*h", rh, (torch.sigmoid(y[hd:]) * hprev.double()).float(), rtol=0.0,
                    atol=tol["atol"] * float(hprev.abs().max()))
    else:
        hprev = torch.randn(cout, h, w, generator=g)
        z = torch.rand(cout, h, w, generator=g)
        got = ops.conv2d_k3_bf16x3(dx, wp, bp, cout, epilogue=ops.EPI_GRU_Q, aux0=t(hprev, DEV), aux1=t(z, DEV))
        want = (1 - z.double()) * hprev.double() + z.double() * torch.tanh(y)
        check_close("bf16x3 gru q", got, want.float(), **tol)


@pytest.mark.parametrize("h,w", [(21, 28), (130, 256), (148, 200), (72, 520)])
@pytest.mark.parametrize("cins,cout1,c_extra,cout2,relu1", [((16, 16), 12, 4, 16, False), ((32, 32), 24, 8, 32, False),
                                                            ((48, 48), 36, 12, 48, False), ((16,), 16, 0, 16, False),
                                                            ((8, 8), 5, 3, 32, False),
                                                            # mask head: 3x3 + ReLU + 1x1 to 36 channels
                                                            ((16,), 32, 0, 36, True), ((32,), 64, 0, 36, True), ((48,), 96, 0, 36, True)])
def test_conv3x3_then_1x1_fused(h, w, cins, cout1, c_extra, cout2, relu1):
    """convd -> convc of the encoder, and the mask head, in one kernel (effi_conv2d_k3_k1_bf16x3_f32) against the two fp64
    convolutions."""
    from effi_mvs_plus_amd import ops, packing
    g = torch.Generator().manual_seed(cout1 * 100 + h)
    xs = [torch.randn(c, h, w, generator=g) for c in cins]
    cin = sum(cins)
    w1 = torch.randn(cout1, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b1 = 0.1 * torch.randn(cout1, generator=g)
    extra = torch.randn(c_extra, h, w, generator=g) if c_extra else None
    w2 = torch.randn(cout2, cout1 + c_extra, 1, 1, generator=g) * (2.0 / (cout1 + c_extra)) ** 0.5
    b2 = 0.1 * torch.randn(cout2, generator=g)
    mid = F.conv2d(torch.cat(xs).unsqueeze(0).double(), w1.double(), b1.double(), padding=1)
    if relu1:
        mid = F.relu(mid)
    if c_extra:
        mid = torch.cat([mid, extra.unsqueeze(0).double()], 1)
    want = F.conv2d(mid, w2.double(), b2.double())[0]
    if not relu1:
        want = F.relu(want)
    wx, bx = packing.pack_conv2d_bf16x3(w1.to(DEV), b1.to(DEV))
    w2p, b2p = packing.pack_conv1x1_after(w2.to(DEV), b2.to(DEV), cout1, c_extra)
    got = ops.conv2d_k3_k1_x3([t(x, DEV) for x in xs], wx, bx, cout1, None if extra is None else t(extra, DEV), w2p, b2p, cout2,
                              relu=not relu1, relu1=relu1)
    check_close(f"3x3+1x1 {cins}->{cout1}(+{c_extra})->{cout2} {h}x{w}", got, want.float(), rtol=0.0,
                atol=6e-5 * float(want.abs().max()))


@pytest.mark.parametrize("h,w", [(21, 28), (130, 256), (148, 200), (256, 512), (72, 520)])
@pytest.mark.parametrize("cin_a,cin_b,cout", [(16, 16, 16), (32, 32, 32), (48, 48, 48), (24, 8, 20), (64, 64, 64)])
def test_conv2d_pair_matches_two_single_launches(h, w, cin_a, cin_b, cout):
    """effi_conv2d_k3_bf16x3_pair_f32: two convolutions sharing one grid give the bits of the two single launches."""
    from effi_mvs_plus_amd import ops, packing
    g = torch.Generator().manual_seed(cout * 100 + h)
    xa, xb = t(torch.randn(cin_a, h, w, generator=g), DEV), t(torch.randn(cin_b, h, w, generator=g), DEV)
    packs = []
    for cin in (cin_a, cin_b):
        wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        packs.append(packing.pack_conv2d_bf16x3(wt.to(DEV), (0.1 * torch.randn(cout, generator=g)).to(DEV)))
    (wa, ba), (wb, bb) = packs
    ya, yb = ops.conv2d_k3_bf16x3_pair([xa], wa, ba, [xb], wb, bb, cout, act=ops.ACT_RELU)
    assert torch.equal(ya, ops.conv2d_k3_bf16x3([xa], wa, ba, cout, act=ops.ACT_RELU))
    assert torch.equal(yb, ops.conv2d_k3_bf16x3([xb], wb, bb, cout, act=ops.ACT_RELU))


def test_conv2d_split_bf16_refuses_unaligned_sources():
    """An octet of input channels must lie in one source: (17, 3) is refused by the library, and ops.conv2d keeps such
    layers on the fp32 kernel."""
    from effi_mvs_plus_amd import ops, packing
    from effi_mvs_plus_amd._lib import EffiLibraryError
    xs = [torch.randn(17, 8, 8).to(DEV), torch.randn(3, 8, 8).to(DEV)]
    wt = torch.randn(16, 20, 3, 3).to(DEV)
    wx, bx = packing.pack_conv2d_bf16x3(wt, None)
    with pytest.raises(EffiLibraryError):
        ops.conv2d_k3_bf16x3(xs, wx, bx, 16)
    w2, b2 = packing.pack_conv2d(wt, None)
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        got = ops.conv2d(xs, w2, b2, 16, 3)
    finally:
        ops.set_precision(before)
    check_close("unaligned sources fall back to fp32 MFMA", got, F.conv2d(torch.cat(xs).unsqueeze(0), wt, padding=1)[0].cpu(),
                rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("h,w", [(36, 60), (256, 256), (256, 512)])      # rows-per-wave 1, 2 and 4 of the v2 kernel
@pytest.mark.parametrize("hd,cd", [(16, 4), (48, 12)])
def test_update_convs_at_tile_configs(O, h, w, hd, cd, precision):
    """ConvGRU / encoder / heads against the oracle at image sizes that select every tiling of the
    MFMA kernel (the golden fixtures are small and only reach the 1-row-per-wave variant)."""
    import contextlib
    import io
    from effi_mvs_plus_amd.models.update import BasicUpdateBlock
    g = torch.Generator().manual_seed(hd * 1000 + h)
    with contextlib.redirect_stdout(io.StringIO()):
        blk = BasicUpdateBlock(hidden_dim=hd, cost_dim=3, ratio=2, context_dim=cd, UpMask=True, Inverse=True, cost_num=2).eval()
    sd = synth.randomize_state_dict(blk.state_dict(), seed=5)
    blk.load_state_dict(sd)
    sd = {"b." + k: v for k, v in sd.items()}
    blk = blk.to(DEV)
    net_h = torch.tanh(torch.randn(1, hd, h, w, generator=g))
    x = torch.relu(torch.randn(1, hd, h, w, generator=g))
    inv = torch.rand(1, 1, h, w, generator=g)
    cost = torch.randn(1, 6, h, w, generator=g)
    ctx = torch.relu(torch.randn(1, cd, h, w, generator=g))
    ct = lambda want, layers: conv_tol(precision, want, 1e-4, 2e-5, layers)  # noqa: E731
    want = O.conv_gru(sd, "b.depth_gru", net_h, x)
    check_close(f"ConvGRU hd={hd} {h}x{w}", blk.depth_gru(t(net_h, DEV), t(x, DEV)), want, **ct(want, 2))
    want = O.projection_input(sd, "b.encoder", inv, cost, ctx)
    check_close(f"ProjectionInput hd={hd} {h}x{w}", blk.encoder(t(inv, DEV), t(cost, DEV), t(ctx, DEV)), want, **ct(want, 3))
    want = O.depth_head(sd, "b.depth_head", net_h)
    check_close(f"DepthHead hd={hd} {h}x{w}", blk.depth_head(t(net_h, DEV)), want, **ct(want, 2))
    want = O.mask_head(sd, "b.mask", net_h)[0]
    check_close(f"mask head hd={hd} {h}x{w}", blk.run_mask(t(net_h[0], DEV)), want, **ct(want, 2))
    # fused depth-head tail: inv + tanh(conv2(relu(conv1(net)))) and the depth it scales to
    dv = torch.linspace(1 / 935.0, 1 / 425.0, 384)
    hid = blk.depth_head.run_hidden(t(net_h[0], DEV))
    inv_new, depth = blk.depth_head.run_update(hid, t(inv[0], DEV), t(dv, DEV))
    want_inv = inv + O.depth_head(sd, "b.depth_head", net_h)
    check_close(f"head update hd={hd} {h}x{w}", inv_new, want_inv[0], **ct(want_inv, 2))
    want_depth = O.disp_to_depth(want_inv, torch.tensor(425.0), torch.tensor(935.0))[1]
    check_close(f"head depth hd={hd} {h}x{w}", depth, want_depth[0], rtol=1e-4, atol=2e-2)


@pytest.mark.parametrize("h,w", [(16, 20), (9, 7), (148, 200)])
def test_split_tanh_relu(h, w):
    """tanh / relu halves of the context pyramid (models/Effi_MVS_plus.py:445-450): vectorised (h*w % 4 == 0) and scalar form."""
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(h)
    ctx = torch.randn(20, h, w, generator=g) * 2
    hid, inp = ops.split_tanh_relu(t(ctx, DEV), 16, 4)
    check_close("tanh half", hid, torch.tanh(ctx[:16]), rtol=1e-5, atol=1e-6)
    assert torch.equal(inp.cpu(), torch.relu(ctx[16:]))


@pytest.mark.parametrize("sizes", [[(8, 12), (16, 24), (32, 48)], [(9, 7), (18, 14), (36, 28)], [(5, 4)], [(4, 6), (7, 9), (8, 8), (3, 3)]])
def test_split_tanh_relu_stages(sizes):
    """All stages in one launch: float4 form (every h*w a multiple of 4) and scalar form (odd sizes), 1 to 4 maps."""
    from effi_mvs_plus_amd import ops
    hds, cds = [48, 32, 16, 8][:len(sizes)], [12, 8, 4, 3][:len(sizes)]
    g = torch.Generator().manual_seed(len(sizes) * 100 + sizes[0][0])
    ctxs = [torch.randn(hd + cd, h, w, generator=g) * 2 for (h, w), hd, cd in zip(sizes, hds, cds)]
    outs = ops.split_tanh_relu_stages([t(c, DEV) for c in ctxs], hds, cds)
    for k, (c, hd, (hid, inp)) in enumerate(zip(ctxs, hds, outs)):
        check_close(f"tanh half of map {k}", hid, torch.tanh(c[:hd]), rtol=1e-5, atol=1e-6)
        assert torch.equal(inp.cpu(), torch.relu(c[hd:])), k


@pytest.mark.parametrize("h,w", [(36, 60), (148, 200), (72, 520)])
@pytest.mark.parametrize("hd", [16, 32, 48])
def test_mask_head_fused_with_convex_upsampling(h, w, hd):
    """effi_conv2d_k3_k1_up2x_bf16x3_f32 (mask never written) against the mask-head kernel followed by effi_convex_upsample2x_f32:
    same mask values, the 9-tap softmax summed in a different order -> last-bit differences only."""
    import contextlib
    import io
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.update import BasicUpdateBlock
    g = torch.Generator().manual_seed(hd * 10 + h)
    with contextlib.redirect_stdout(io.StringIO()):
        blk = BasicUpdateBlock(hidden_dim=hd, cost_dim=3, ratio=2, context_dim=hd // 4, UpMask=True, Inverse=True, cost_num=2).eval()
    blk.load_state_dict(synth.randomize_state_dict(blk.state_dict(), seed=7))
    blk = blk.to(DEV)
    net = t(torch.tanh(torch.randn(hd, h, w, generator=g)), DEV)
    inv = t(torch.rand(1, h, w, generator=g), DEV)
    dv = t(torch.linspace(1 / 935.0, 1 / 425.0, 384), DEV)
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        assert blk.mask_upsample_fusable(net)
        depth_f, dinv_f = blk.run_mask_upsample(net, inv, dv)
        mask = blk.run_mask(net)
        _, depth_c, dinv_c = ops.convex_upsample2x(inv, mask, dv, want_inv=False, want_depth_inv=True)
    finally:
        ops.set_precision(before)
    check_close(f"fused mask+upsample depth hd={hd} {h}x{w}", depth_f, depth_c.cpu(), rtol=2e-6, atol=1e-3)
    check_close(f"fused mask+upsample inverse depth hd={hd} {h}x{w}", dinv_f, dinv_c.cpu(), rtol=0.0, atol=2e-6)


@pytest.mark.parametrize("h,w", [(36, 60), (37, 52), (148, 200), (72, 520)])
@pytest.mark.parametrize("hd", [16, 32, 48])
def test_depth_head_as_tap_projections(O, h, w, hd):
    """DepthHead.run_taps (conv1 + ReLU + the nine 1x1 tap projections of conv2 in one kernel, then effi_head_update_f32) against the
    oracle's depth head and against the two-kernel form (conv1 -> hidden map -> one-channel 3x3 conv); map edges = conv2's padding."""
    import contextlib
    import io
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.models.update import BasicUpdateBlock
    g = torch.Generator().manual_seed(hd * 7 + h)
    with contextlib.redirect_stdout(io.StringIO()):
        blk = BasicUpdateBlock(hidden_dim=hd, cost_dim=3, ratio=2, context_dim=hd // 4, UpMask=True, Inverse=True, cost_num=2).eval()
    sd = synth.randomize_state_dict(blk.state_dict(), seed=11)
    blk.load_state_dict(sd)
    sd = {"b." + k: v for k, v in sd.items()}
    blk = blk.to(DEV)
    net_h = torch.tanh(torch.randn(1, hd, h, w, generator=g))
    inv = torch.rand(1, 1, h, w, generator=g)
    dv = torch.linspace(1 / 935.0, 1 / 425.0, 384)
    net, inv_d, dv_d = t(net_h[0], DEV), t(inv[0], DEV), t(dv, DEV)
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        assert blk.depth_head.taps_fusable(net)
        scratch = torch.full((hd, h, w), float("nan"), device=DEV)
        inv_f, depth_f = blk.depth_head.run_taps(net, inv_d, dv_d, scratch)
        hid = blk.depth_head.run_hidden(net)
        inv_c, depth_c = blk.depth_head.run_update(hid, inv_d, dv_d)
    finally:
        ops.set_precision(before)
    want_inv = inv + O.depth_head(sd, "b.depth_head", net_h)
    tol = conv_tol("split", want_inv, 1e-4, 2e-5, 2)
    check_close(f"tap-projected head vs oracle hd={hd} {h}x{w}", inv_f, want_inv[0], **tol)
    check_close(f"tap-projected head vs two kernels hd={hd} {h}x{w}", inv_f, inv_c.cpu(), **tol)
    want_depth = O.disp_to_depth(want_inv, torch.tensor(425.0), torch.tensor(935.0))[1]
    check_close(f"tap-projected head depth hd={hd} {h}x{w}", depth_f, want_depth[0], rtol=1e-4, atol=2e-2)


@pytest.mark.parametrize("h,w", [(12, 16), (36, 60), (37, 52), (148, 200), (50, 520)])
@pytest.mark.parametrize("cd", [4, 8])
def test_encoder_tail_equals_the_two_launches(h, w, cd):
    """effi_encoder_tail_bf16x3_f32 (convc2 | convd2 -> convd -> convc with the two intermediate maps in LDS) against the pair launch
    followed by the fused 3x3 -> 1x1 launch: same operands, same products, same order -> bitwise equal; tiles cut by the map's
    border on every side, maps smaller than a tile."""
    from effi_mvs_plus_amd import ops, packing
    hd, cmix = 16, 16 - cd
    g = torch.Generator().manual_seed(h * 31 + cd)
    rnd = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s  # noqa: E731
    cor1, dfm1 = torch.relu(rnd(hd, h, w)), torch.relu(rnd(hd, h, w))
    ctx = torch.relu(rnd(cd, h, w))
    wc2, bc2, wd2, bd2 = rnd(hd, hd, 3, 3, s=0.1), rnd(hd, s=0.1), rnd(hd, hd, 3, 3, s=0.1), rnd(hd, s=0.1)
    wd, bd = rnd(cmix, 2 * hd, 3, 3, s=0.08), rnd(cmix, s=0.1)
    wc, bc = rnd(hd, hd, 1, 1, s=0.2), rnd(hd, s=0.1)
    d = lambda x: t(x, DEV)  # noqa: E731
    pc2, pbc2 = packing.pack_conv2d_bf16x3(d(wc2), d(bc2))
    pd2, pbd2 = packing.pack_conv2d_bf16x3(d(wd2), d(bd2))
    pd, pbd = packing.pack_conv2d_bf16x3(d(wd), d(bd))
    p2, pb2 = packing.pack_conv1x1_after(d(wc), d(bc), cmix, cd)
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        got = ops.encoder_tail(d(cor1), d(dfm1), pc2, pbc2, pd2, pbd2, pd, pbd, cmix, d(ctx), p2, pb2, hd)
        cor, dfm = ops.conv2d_k3_bf16x3_pair([d(cor1)], pc2, pbc2, [d(dfm1)], pd2, pbd2, hd, act=ops.ACT_RELU)
        want = ops.conv2d_k3_k1_x3([cor, dfm], pd, pbd, cmix, d(ctx), p2, pb2, hd, relu=True)
    finally:
        ops.set_precision(before)
    assert torch.equal(got, want), float((got - want).abs().max())
    ref = F.relu(F.conv2d(torch.cat([F.conv2d(torch.cat([F.relu(F.conv2d(cor1[None], wc2, bc2, padding=1)),
                                                             F.relu(F.conv2d(dfm1[None], wd2, bd2, padding=1))], 1), wd, bd, padding=1),
                                     ctx[None]], 1), wc, bc))[0]
    check_close(f"encoder tail vs torch {h}x{w} cd={cd}", got, ref, **conv_tol("split", ref, 1e-4, 2e-5, 3))


@pytest.mark.parametrize("h2,w2", [(6, 8), (37, 52), (74, 100)])
@pytest.mark.parametrize("co,f,ci", [(8, 64, 16), (16, 32, 8)])
@pytest.mark.parametrize("nhwc", [False, True])
def test_fpn_last_head_split_by_linearity(h2, w2, co, f, ci, nhwc):
    """packing.pack_fpn_head_split + the pixel-shuffle-add epilogues: conv3x3(up2(top) + inner(l1)) evaluated as a half-resolution
    conv with four parity groups plus a composed full-resolution conv, against torch on the CPU (borders included: the bias of the
    lateral 1x1 must vanish exactly where the 3x3 window leaves the map)."""
    from effi_mvs_plus_amd import ops, packing
    g = torch.Generator().manual_seed(h2 * 13 + co)
    top = torch.randn(f, h2, w2, generator=g)
    l1 = torch.randn(ci, 2 * h2, 2 * w2, generator=g)
    w_out = torch.randn(co, f, 3, 3, generator=g) * 0.05
    w_in, b_in = torch.randn(f, ci, 1, 1, generator=g) * 0.2, torch.randn(f, generator=g)
    want = F.conv2d(F.interpolate(top[None], scale_factor=2, mode="nearest") + F.conv2d(l1[None], w_in, b_in), w_out, padding=1)[0]
    (wu, bu), (wl, bl) = packing.pack_fpn_head_split(w_out.to(DEV), w_in.to(DEV), b_in.to(DEV))
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        ones = torch.ones(1, h2, w2, device=DEV)
        u = ops.conv2d_k3_bf16x3([t(top, DEV), ones], wu, bu, 4 * co)
        got = ops.conv2d_k3_bf16x3([t(l1, DEV)], wl, bl, co, epilogue=ops.EPI_NHWC_ADD_SHUF2 if nhwc else ops.EPI_ADD_SHUF2, aux0=u)
    finally:
        ops.set_precision(before)
    if nhwc:
        got = got.permute(2, 0, 1)
    check_close(f"split FPN head co={co} f={f} {2 * h2}x{2 * w2} nhwc={nhwc}", got, want, **conv_tol("split", want, 1e-4, 2e-5, 2))


@pytest.mark.parametrize("h,w", [(12, 16), (16, 16), (37, 52), (96, 128), (50, 520)])
@pytest.mark.parametrize("cin,cout", [(3, 8), (8, 8), (5, 6), (3, 4)])
def test_conv3x3_twice_in_one_kernel(h, w, cin, cout):
    """effi_conv2d_k3_twice_bf16x3_f32 (two one-octet 3x3 layers + ReLU, the intermediate map in LDS) against torch on the CPU and
    against two single-layer launches (same operands and products, another grouping of the K index: rounding-level differences);
    tiles cut by the border, maps smaller than a tile."""
    from effi_mvs_plus_amd import ops, packing
    g = torch.Generator().manual_seed(h * 7 + cin)
    x = torch.randn(cin, h, w, generator=g)
    cmid = 4 if cout == 4 else 8                       # the context pyramid's block is 3 -> 4 -> 4
    w1, b1 = torch.randn(cmid, cin, 3, 3, generator=g) * 0.3, torch.randn(cmid, generator=g) * 0.1
    w2, b2 = torch.randn(cout, cmid, 3, 3, generator=g) * 0.2, torch.randn(cout, generator=g) * 0.1
    want = F.relu(F.conv2d(F.relu(F.conv2d(x[None], w1, b1, padding=1)), w2, b2, padding=1))[0]
    d = lambda v: t(v, DEV)  # noqa: E731
    p1, pb1 = packing.pack_conv2d_bf16x3_oct(d(w1), d(b1))
    p2, pb2 = packing.pack_conv2d_bf16x3_oct(d(w2), d(b2))
    q1, qb1 = packing.pack_conv2d_bf16x3(d(w1), d(b1))
    q2, qb2 = packing.pack_conv2d_bf16x3(d(w2), d(b2))
    before = ops.get_precision()
    ops.set_precision("split")
    try:
        got = ops.conv2d_k3_twice(d(x), p1, pb1, p2, pb2, cout)
        mid = ops.conv2d_k3_bf16x3([d(x)], q1, qb1, cmid, act=ops.ACT_RELU)
        two = ops.conv2d_k3_bf16x3([mid], q2, qb2, cout, act=ops.ACT_RELU)
    finally:
        ops.set_precision(before)
    check_close(f"3x3 twice vs torch {cin}->{cmid}->{cout} {h}x{w}", got, want, **conv_tol("split", want, 1e-4, 2e-5, 2))
    check_close(f"3x3 twice vs two launches {cin}->{cmid}->{cout} {h}x{w}", got, two.cpu(), rtol=0.0, atol=2e-5 * float(want.abs().max()))


@pytest.mark.parametrize("hin,win", [(8, 8), (37, 52), (74, 100), (96, 520)])
@pytest.mark.parametrize("cin,cout", [(8, 16), (16, 32), (32, 64), (4, 8), (3, 24)])
def test_conv5x5_stride2_split_precision(hin, win, cin, cout):
    """effi_conv2d_k5s2_bf16x3_f32 (column parities de-interleaved in LDS, 8-channel chunks, groups of two output tiles) against torch
    on the CPU and against the fp32-MFMA kernel; odd heights, maps smaller than a tile, cin not a multiple of 8."""
    from effi_mvs_plus_amd import ops, packing
    g = torch.Generator().manual_seed(hin * 3 + cin)
    x = torch.randn(cin, hin, win, generator=g)
    wt, b = torch.randn(cout, cin, 5, 5, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1
    want = F.relu(F.conv2d(x[None], wt, b, stride=2, padding=2))[0]
    wp, bp = packing.pack_conv2d(t(wt, DEV), t(b, DEV))
    before = ops.get_precision()
    try:
        ops.set_precision("split")
        got = ops.conv2d_k5s2(t(x, DEV), wp, bp, cout, act=ops.ACT_RELU)
        ops.set_precision("fp32")
        ref = ops.conv2d_k5s2(t(x, DEV), wp, bp, cout, act=ops.ACT_RELU)
    finally:
        ops.set_precision(before)
    check_close(f"5x5 s2 split {cin}->{cout} {hin}x{win}", got, want, **conv_tol("split", want, 1e-4, 2e-5, 1))
    check_close(f"5x5 s2 fp32 {cin}->{cout} {hin}x{win}", ref, want, rtol=1e-4, atol=2e-5)


def test_cpu_tensor_fails_loudly():
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd._lib import EffiLibraryError
    with pytest.raises(EffiLibraryError):
        ops.view_aggregate(torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5))


def test_stage1_hypotheses_and_intervals():
    """effi_stage1_hypotheses_f32 on its own: D uniform inverse-depth samples between the first and last of the [384] range, inverted
    (models/module.py:578-583, models/Effi_MVS_plus.py:473-474), the three stage intervals (:424 x depth_interals_ratio :316) and
    depth_min_ / depth_max_ (:413-414)."""
    from effi_mvs_plus_amd import ops
    from oracle import effi_oracle as O
    for n_range, D, lo, hi in ((384, 48, 1 / 935.0, 1 / 425.0), (384, 96, 1 / 3.0, 1 / 0.5), (192, 8, 1e-3, 2e-3), (384, 32, 1 / 935.0, 1 / 425.0)):
        dv = torch.linspace(lo, hi, n_range, dtype=torch.float32).view(1, n_range)
        want = 1.0 / O.depth_range_samples(dv, D, None, [1, 2, 2])[0, :, 0, 0]
        depths, misc = ops.stage1_hypotheses(dv[0].to(DEV).contiguous(), D)
        assert torch.equal(depths.cpu(), want), (depths.cpu() - want).abs().max()
        base = (dv[0, -1] - dv[0, 0]) / n_range
        assert torch.equal(misc[:3].cpu(), torch.stack([base * 4, base * 2, base * 1]))
        assert misc[3].item() == (1.0 / dv[0, -1]).item() and misc[4].item() == (1.0 / dv[0, 0]).item()
    with pytest.raises(Exception):
        ops.stage1_hypotheses(torch.zeros(1, device=DEV), 8)          # n_range < 2


def test_3d_end_kernels_do_not_depend_on_what_shares_their_cu():
    """Round 4: the compiler's packed (z-pair) form of the dedicated 8 -> 1 channel kernel returned wrong low halves in lanes 48-63 --
    only while another queue ran matrix-core GEMMs on the same CUs (10-60 % of the launches; never alone, never next to element-wise
    kernels; tools/stress_c8_corun.py).  conv3d.hip is compiled without the SLP vectoriser since (csrc/Makefile).  Here: the three
    dedicated kernels next to hipBLASLt GEMMs on two more streams, every result against a quiet run, bit for bit."""
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s_: torch.randn(*s_, generator=g).to(DEV)
    D, h, w = 8, 24, 32
    x8, w81, b1 = rnd(8, D, h, w), rnd(8, 27, 1) * 0.1, rnd(1)
    x1, w18, b8 = rnd(1, D, 2 * h, 2 * w), rnd(1, 27, 8) * 0.2, rnd(8)

    def run():
        return (ops.conv3d_k3([x8], w81, None, 1, relu=False), *ops.conv3d_k3_pair(x1, w18, b8, x1, w18, b8, 8, sxy=2),
                *ops.deconv3d_k3_pair(x8, w81, b1, x8, w81, b1, 1, sz=1))

    want = [o.clone() for o in run()]
    A, B = rnd(2048, 2048).bfloat16(), rnd(2048, 2048).bfloat16()
    torch.cuda.synchronize()
    s0, s1, s2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    bad = 0
    for _ in range(80):
        outs = []
        for _ in range(6):
            with torch.cuda.stream(s1):
                A @ B
            with torch.cuda.stream(s2):
                B @ A
            with torch.cuda.stream(s0):
                outs.append(run())
        torch.cuda.synchronize()
        bad += sum(int(not all(torch.equal(a, b) for a, b in zip(o, want))) for o in outs)
    assert bad == 0, f"{bad} of 480 runs next to GEMMs differ from the quiet run"
