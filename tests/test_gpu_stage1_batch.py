"""GPU: the stage-1 cost volume of a batch of samples in batched launches.

  * every ``*_batch`` entry of the stage-1 cost volume, through its ``ops`` wrapper: sample i of a batched launch == the unbatched call
    on sample i (the 3-D convolutions in every form ``Conv3d.run`` / ``Deconv3d.run`` select, the three kernel forms of the stage-1 warp,
    the view aggregation, the soft-argmin with per-sample ranges, the view-weight net on B * S planes, the cascade's set-up);
  * ``DepthNet.forward`` and the regulariser on [B, ...] == their B = 1 calls;
  * ``Effi_MVS_plus.forward_hot`` / ``forward`` for B > 1 == the B single-sample calls, with ``conf_fused`` / ``setup_fused`` off too, and
    as a ``ForwardGraph`` replay;
  * launch counts: a batched stage 1 records ONE pass of launches for B samples (what fails without the feature);
  * mismatched sample counts raise; n = 1 through a ``_batch`` entry is the plain entry.

The bar is BITWISE (torch.equal) everywhere: both sides are this library, a batched launch offsets its pointers per sample and runs the
single-sample body, and an output's accumulation order does not depend on the tile shape a launch rule picks.
"""
import contextlib

import pytest
import torch

from common import build_model, load_golden
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (2, 3)


@pytest.fixture(params=["fp32", "split", "bf16"])
def precision3(request):
    """The ``precision`` fixture's two arithmetics plus plain bf16 operands (the *_bf16 twins of the split-precision entries)."""
    from effi_mvs_plus_amd import ops
    before = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(before)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(DEV)


def _rand_bn(bn, g):
    bn.weight.data = 0.6 + 0.8 * torch.rand(bn.weight.shape, generator=g)
    bn.bias.data = 0.1 * torch.randn(bn.bias.shape, generator=g)
    bn.running_mean.data = 0.1 * torch.randn(bn.bias.shape, generator=g)
    bn.running_var.data = 0.5 + torch.rand(bn.bias.shape, generator=g)


def _assert_samples_equal(batched, single_fn, n, what):
    assert batched.shape[0] == n, (what, batched.shape)
    for i in range(n):
        want = single_fn(i)
        assert batched[i].shape == want.shape, (what, i, batched[i].shape, want.shape)
        assert torch.equal(batched[i], want), f"{what}: sample {i} of {n} differs from the single-sample launch"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. per entry: batched == single
# ---------------------------------------------------------------------------------------------------------------------------
# (D, h, w): (9, 12, 40) has more than one 32 x 8 tile in x and y with partial tiles, more than two z groups, w % 4 == 0;
# (5, 9, 37) has unaligned rows -- the forms the split-precision layers fall back to
VOLS = [(9, 12, 40), (5, 9, 37)]
CONVS = [(1, 8, 1, True), (8, 8, 1, True), (8, 16, 2, True), (16, 16, 1, True), (16, 32, 2, True), (32, 32, 1, True), (8, 1, 1, False)]


def _conv3d_module(cin, cout, stride, relu, seed):
    from effi_mvs_plus_amd.models.module import Conv3d
    g = torch.Generator().manual_seed(seed)
    m = Conv3d(cin, cout, stride=stride, padding=1, relu=relu, bn=relu)
    m.conv.weight.data = torch.randn(m.conv.weight.shape, generator=g) * (2.0 / (27 * cin)) ** 0.5
    if m.bn is not None:
        _rand_bn(m.bn, g)
    return m.eval().to(DEV)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D,h,w", VOLS)
@pytest.mark.parametrize("cin,cout,stride,relu", CONVS)
def test_conv3d_batch_equals_single(precision3, cin, cout, stride, relu, D, h, w, n):
    """``Conv3d.run`` on [n,cin,D,h,w]: per precision and shape this is effi_conv3d_k3_f32 (the general body and the dedicated 1 -> 8 /
    8 -> 1 kernels), effi_conv3d_k3s1_mfma_f32 / _k3s2_mfma_f32, or effi_conv3d_k3s1_roll_bf16x3_f32 / _k3s1_bf16x3_f32 /
    _k3s2_bf16x3_f32 (and their _bf16 twins) -- each through its _batch entry."""
    m = _conv3d_module(cin, cout, stride, relu, seed=cin * 100 + cout)
    x = _rand(n, cin, D, h, w, seed=D + n)
    with torch.no_grad():
        got = m.run([x])
        _assert_samples_equal(got, lambda i: m.run([x[i]]), n, f"conv3d {cin}->{cout} s{stride} {D}x{h}x{w} {precision3}")
        assert torch.equal(m(x), got)                                   # Conv3d.forward takes the same launch


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D,h,w", [(3, 5, 8), (2, 6, 12)])
@pytest.mark.parametrize("cin,cout", [(32, 16), (16, 8)])
@pytest.mark.parametrize("with_skip", [False, True])
def test_deconv3d_batch_equals_single(precision3, with_skip, cin, cout, D, h, w, n):
    """``Deconv3d.run``: effi_deconv3d_k3_f32 ("fp32") / effi_deconv3d_k3s2_bf16x3_f32 (split, bf16), skip added after the ReLU."""
    from effi_mvs_plus_amd.models.module import Deconv3d
    g = torch.Generator().manual_seed(cin + cout)
    m = Deconv3d(cin, cout, stride=2, padding=1, output_padding=1)
    m.conv.weight.data = torch.randn(m.conv.weight.shape, generator=g) * (8.0 / (27 * cin)) ** 0.5
    _rand_bn(m.bn, g)
    m = m.eval().to(DEV)
    x = _rand(n, cin, D, h, w, seed=h + n)
    skip = _rand(n, cout, 2 * D, 2 * h, 2 * w, seed=5) if with_skip else None
    with torch.no_grad():
        got = m.run(x, skip=skip)
        _assert_samples_equal(got, lambda i: m.run(x[i], skip=None if skip is None else skip[i]), n,
                              f"deconv3d {cin}->{cout} {D}x{h}x{w} skip={with_skip} {precision3}")
        if not with_skip:
            assert torch.equal(m(x), got)


# Launch rules that count the workgroups of ALL samples: shapes at which ONE sample stays below a rule's threshold and n = 3 samples
# cross it, so that the batched launch and the single-sample launches it is compared with run DIFFERENT instantiations (the claim under
# test: an output's accumulation order does not depend on them).  tiles = ceil(wo/32) * ceil(ho/8), cols = ceil(wo/16).
#   1 -> 8, 8 -> 1 at (48,64,128): planes per thread 8 from tiles * ceil(D/8) * n >= 512: 32 * 6 = 192, x 3 = 576
#   8 -> 8 at (40,64,128), "fp32": slices per thread 4 from tiles * ceil(D/4) * n >= 384: 32 * 10 = 320, x 3 = 960 (split: rolling window,
#     whose (rows per wave, plane run) come from a cost model over the workgroups of all samples)
#   16 -> 16, 32 -> 32 at (12,32,64) and 8 -> 16, 16 -> 32 stride 2 INTO it: "fp32" rows per wave 2 from cols * ceil(h/8) * planes >= 512:
#     4 * 4 * 12 = 192, x 3 = 576; split / bf16: the same products against 400 (32 -> 32, the stride-2 forms), the cost model (16 -> 16)
STRADDLE = [(1, 8, 1, True, (48, 64, 128)), (8, 1, 1, False, (48, 64, 128)), (8, 8, 1, True, (40, 64, 128)), (16, 16, 1, True, (12, 32, 64)),
            (32, 32, 1, True, (12, 32, 64)), (8, 16, 2, True, (24, 64, 128)), (16, 32, 2, True, (24, 64, 128))]


@pytest.mark.parametrize("cin,cout,stride,relu,vol", STRADDLE)
def test_conv3d_batch_across_a_launch_rule_threshold(precision3, cin, cout, stride, relu, vol):
    m = _conv3d_module(cin, cout, stride, relu, seed=cin * 10 + cout)
    x = _rand(3, cin, *vol, seed=cout)
    with torch.no_grad():
        _assert_samples_equal(m.run([x]), lambda i: m.run([x[i]]), 3, f"conv3d {cin}->{cout} s{stride} {vol} {precision3}")


@pytest.mark.parametrize("with_skip", [False, True])
def test_deconv3d_batch_across_a_launch_rule_threshold(precision3, with_skip):
    """16 -> 8 from (8,48,128): "fp32" 8 output channels per workgroup from tiles * D * (cout / 8) * n >= 512 (24 * 8 = 192, x 3 = 576),
    else 4; split / bf16: rows per wave from the rounds model over the workgroups of all samples."""
    from effi_mvs_plus_amd.models.module import Deconv3d
    g = torch.Generator().manual_seed(9)
    m = Deconv3d(16, 8, stride=2, padding=1, output_padding=1)
    m.conv.weight.data = torch.randn(m.conv.weight.shape, generator=g) * (8.0 / (27 * 16)) ** 0.5
    _rand_bn(m.bn, g)
    m = m.eval().to(DEV)
    x = _rand(3, 16, 8, 48, 128, seed=2)
    skip = _rand(3, 8, 16, 96, 256, seed=3) if with_skip else None
    with torch.no_grad():
        _assert_samples_equal(m.run(x, skip=skip), lambda i: m.run(x[i], skip=None if skip is None else skip[i]), 3,
                              f"deconv3d 16->8 8x48x128 skip={with_skip} {precision3}")


def test_conv3d_batch_in_slices_of_larger_allocations(precision3):
    """Sample strides are free: the inputs are every second sample of a larger tensor, the outputs a channel range of a larger one (output
    sample stride > one sample); what lies between the samples is left untouched."""
    from effi_mvs_plus_amd import ops
    m1, m8 = _conv3d_module(1, 8, 1, True, seed=3), _conv3d_module(8, 8, 1, True, seed=4)
    D, h, w = 9, 12, 40
    for m, cin in ((m1, 1), (m8, 8)):
        wp, bp = m._packed()
        big_in = _rand(5, cin, D, h, w, seed=cin)
        x = big_in[::2]
        assert not x.is_contiguous()
        big_out = torch.full((3, 12, D, h, w), 7.0, device=DEV)
        out = big_out[:, 2:10]
        got = ops.conv3d_k3([x], wp, bp, 8, relu=True, out=out)
        assert got.data_ptr() == out.data_ptr() and out.stride(0) > out[0].numel()
        _assert_samples_equal(out, lambda i: ops.conv3d_k3([x[i].contiguous()], wp, bp, 8, relu=True), 3, f"conv3d {cin}->8 strided")
        assert bool((big_out[:, :2] == 7.0).all()) and bool((big_out[:, 10:] == 7.0).all())


def _edge_pairs(n_views):
    """The edge rig of the golden DepthNet case (projections leaving the image, z <= 0): [n_views,2,4,4], its 4 views cycled."""
    p = load_golden("g02e_depthnet_edge.npz")["proj"][0]
    return p[[v if v < 4 else 1 + (v - 1) % 3 for v in range(n_views)]].contiguous()


def _stage1_pairs(B, n_views):
    """[B,n_views,2,4,4]: the ring rig, the edge rig (sample 1), the ring rig of another image size."""
    out = []
    for b in range(B):
        if b == 1:
            out.append(_edge_pairs(n_views))
        else:
            out.append(synth.synth_cameras(128 + 16 * b, 160 + 8 * b, n_views)["stage1"][0])
    return torch.stack(out).to(DEV)


def _hyps(B, D):
    """[B,D] depth hypotheses, another range per sample."""
    return torch.stack([1.0 / torch.linspace(1 / (935.0 + 40 * b), 1 / (425.0 + 15 * b), D) for b in range(B)]).to(DEV)


@contextlib.contextmanager
def _warp_form(form):
    from effi_mvs_plus_amd import ops
    opts = {"exact": {}, "x3": {}, "lds0": {"warp_lds_kb": 0}, "gather": {"warp_lds_kb": -1}}[form]
    with ops.options(**opts):
        yield form == "x3"


@pytest.mark.parametrize("B", NS)
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("D", [8, 48])
@pytest.mark.parametrize("form", ["exact", "x3", "lds0", "gather"])
def test_warpcorr_views_batch_equals_single(precision3, form, D, S, B):
    """C = 32 on 16 x 20 maps (2 x 2 window tiles, partial in both directions): the LDS-window kernel, the same on global loads
    (warp_lds_kb = 0), the direct-gather kernel (-1) and the matrix-core form (warp_x3: split products in "split", hi * hi alone in
    "bf16" -- two instantiations, each against its own single-sample launch; the exact kernels in "fp32"), with the hypotheses given as
    [B,D], as the reference's expanded [B,D,h,w], and as one shared [D]."""
    precision = precision3
    from effi_mvs_plus_amd import ops
    h, w, C = 16, 20, 32
    feats = [torch.stack([f[0] for f in synth.smooth_features(S + 1, C, h, w, seed=30 + b)]) for b in range(B)]     # [S+1,C,h,w] each
    maps = torch.stack(feats).permute(0, 1, 3, 4, 2).contiguous().to(DEV)                                           # [B,S+1,h,w,C]
    rt = torch.stack([ops.compose_rel_proj(p) for p in _stage1_pairs(B, S + 1)])
    hyp = _hyps(B, D)
    with _warp_form(form) as x3:
        for name, dep, dep_i in (("[B,D]", hyp, lambda i: hyp[i]),
                                 ("[B,D,h,w] expanded", hyp.view(B, D, 1, 1).expand(B, D, h, w), lambda i: hyp[i].view(D, 1, 1).expand(D, h, w)),
                                 ("[D] shared", hyp[0], lambda i: hyp[0])):
            sim, ent = ops.warpcorr_views(maps[:, 0], [maps[:, 1 + v] for v in range(S)], rt, dep, D, x3=x3)
            assert tuple(sim.shape) == (B, S, D, h, w) and tuple(ent.shape) == (B, S, h, w)
            for i in range(B):
                s1, e1 = ops.warpcorr_views(maps[i, 0], [maps[i, 1 + v] for v in range(S)], rt[i], dep_i(i), D, x3=x3)
                what = f"warpcorr_views {form} D={D} S={S} hypotheses {name} {precision}: sample {i}"
                assert torch.equal(sim[i], s1), what
                assert torch.equal(ent[i], e1), what
    assert float(sim[1].abs().min()) == 0.0            # the edge rig did leave the image


@pytest.mark.parametrize("B", NS)
def test_warpcorr_views_batch_gather_form_c16_and_per_pixel_hypotheses(B):
    """C = 16 (always the direct-gather kernel) and C = 32 with per-pixel hypotheses [B,D,h,w] (the gather kernel as well)."""
    from effi_mvs_plus_amd import ops
    h, w, S, D = 16, 20, 2, 8
    rt = torch.stack([ops.compose_rel_proj(p) for p in _stage1_pairs(B, S + 1)])
    for C in (16, 32):
        maps = _rand(B, S + 1, h, w, C, seed=C)
        g = torch.Generator().manual_seed(C)
        dep = (425.0 + 510.0 * torch.rand(B, D, h, w, generator=g)).to(DEV) if C == 32 else _hyps(B, D)
        sim, ent = ops.warpcorr_views(maps[:, 0], [maps[:, 1 + v] for v in range(S)], rt, dep, D)
        for i in range(B):
            s1, e1 = ops.warpcorr_views(maps[i, 0], [maps[i, 1 + v] for v in range(S)], rt[i], dep[i], D)
            assert torch.equal(sim[i], s1) and torch.equal(ent[i], e1), (C, i)


def test_warpcorr_views_sources_at_different_strides_fall_back_to_the_loop():
    """Sources that do not share ONE sample stride are not an error: one launch per sample, same bits."""
    from effi_mvs_plus_amd import ops
    h, w, C, D, B = 16, 20, 32, 8, 2
    a, b2 = _rand(B, 2, h, w, C, seed=1), _rand(3 * B, h, w, C, seed=2)
    srcs = [a[:, 1], b2[::3]]
    assert srcs[0].stride(0) != srcs[1].stride(0)
    rt = torch.stack([ops.compose_rel_proj(p) for p in _stage1_pairs(B, 3)])
    hyp = _hyps(B, D)
    sim, ent = ops.warpcorr_views(a[:, 0], srcs, rt, hyp, D)
    for i in range(B):
        s1, e1 = ops.warpcorr_views(a[i, 0], [s_[i] for s_ in srcs], rt[i], hyp[i], D)
        assert torch.equal(sim[i], s1) and torch.equal(ent[i], e1)


@pytest.mark.parametrize("B", NS)
@pytest.mark.parametrize("S", [1, 4])
def test_view_aggregate_batch_equals_single(B, S):
    from effi_mvs_plus_amd import ops
    sims, ws = _rand(B, S, 7, 9, 11, seed=S), torch.rand(B, S, 9, 11, generator=torch.Generator().manual_seed(B)).to(DEV)
    got = ops.view_aggregate(sims, ws)
    _assert_samples_equal(got, lambda i: ops.view_aggregate(sims[i], ws[i]), B, f"view_aggregate S={S}")
    got = ops.view_aggregate(sims, None)
    _assert_samples_equal(got, lambda i: ops.view_aggregate(sims[i], None), B, f"view_aggregate S={S}, unweighted")


@pytest.mark.parametrize("B", NS)
@pytest.mark.parametrize("D", [8, 48, 5])
@pytest.mark.parametrize("conf_up", [0, 4])
def test_softmax_regress_conf_batch_equals_single(B, D, conf_up):
    """D = 8 / 48: the register kernel; D = 5: the generic one.  Hypotheses and the inverse-depth range differ per sample."""
    from effi_mvs_plus_amd import ops
    h, w = 9, 12
    logits, hyp = _rand(B, D, h, w, seed=D, scale=2.0), _hyps(B, D)
    ranges = torch.stack([torch.linspace(1 / (935.0 + 40 * b), 1 / (425.0 + 15 * b), 384) for b in range(B)]).to(DEV)
    for dep, dep_i in ((hyp, lambda i: hyp[i]), (hyp[0], lambda i: hyp[0])):
        got = ops.softmax_regress_conf(logits, dep, ranges, conf_up=conf_up)
        assert len(got) == (4 if conf_up else 3)
        for i in range(B):
            want = ops.softmax_regress_conf(logits[i], dep_i(i), ranges[i], conf_up=conf_up)
            for a, b_ in zip(got, want):
                assert torch.equal(a[i], b_), f"softmax_regress_conf D={D} conf_up={conf_up}: sample {i}"
        got = ops.softmax_regress_conf(logits, dep, None, conf_up=conf_up)
        for i in range(B):
            for a, b_ in zip(got, ops.softmax_regress_conf(logits[i], dep_i(i), None, conf_up=conf_up)):
                assert torch.equal(a[i], b_)


@pytest.fixture(scope="module")
def model8():
    return build_model("8,8,8", seed=17, device=DEV)[0]


@pytest.fixture(scope="module")
def model48():
    return build_model("48,8,8", seed=17, device=DEV)[0]


def test_pixelwise_net_on_all_planes_of_a_batch(model8):
    """The view-weight net already takes n planes: B * S planes of 13 x 17 in one launch are bitwise the per-sample launches."""
    B, S = 3, 4
    ent = 2.1 * torch.rand(B, S, 13, 17, generator=torch.Generator().manual_seed(31)).to(DEV)
    with torch.no_grad():
        got = model8.PixelwiseNet.run(ent)
        assert tuple(got.shape) == (B, S, 13, 17)
        _assert_samples_equal(got, lambda i: model8.PixelwiseNet.run(ent[i]), B, "pixelwise_net")
        assert torch.equal(model8.PixelwiseNet(ent.view(B * S, 1, 13, 17)).view(B, S, 13, 17), got)


def test_compose_rel_proj_batch_equals_single():
    """What ``DepthNet.forward`` launches for its B camera sets (it is handed the hypotheses): one launch, also on every second set
    of a larger tensor."""
    from effi_mvs_plus_amd import ops
    pairs = _stage1_pairs(5, 4)
    for p in (pairs[:3], pairs[::2], pairs[:1]):
        rt = ops.compose_rel_proj(p)
        assert tuple(rt.shape) == (p.shape[0], 3, 12)
        _assert_samples_equal(rt, lambda i: ops.compose_rel_proj(p[i]), p.shape[0], "compose_rel_proj")


def test_cascade_setup_batch_equals_single():
    from effi_mvs_plus_amd import ops
    B, N, D = 3, 5, 48
    keys = ("stage1", "stage2", "stage3")
    cams = [synth.synth_cameras(128 + 16 * b, 160 + 8 * b, N) for b in range(B)]
    pairs = [torch.cat([c[k] for c in cams]).to(DEV) for k in keys]                       # [B,N,2,4,4] per stage
    ranges = torch.stack([torch.linspace(1 / (935.0 + 40 * b), 1 / (425.0 + 15 * b), 384) for b in range(B)]).to(DEV)
    (hyp, misc), rts = ops.cascade_setup(ranges, D, pairs)
    assert tuple(hyp.shape) == (B, D) and tuple(misc.shape) == (B, 5) and len(rts) == 3 and tuple(rts[0].shape) == (B, N - 1, 12)
    for i in range(B):
        (h1, m1), r1 = ops.cascade_setup(ranges[i], D, [p[i] for p in pairs])
        assert torch.equal(hyp[i], h1) and torch.equal(misc[i], m1)
        for s in range(3):
            assert torch.equal(rts[s][i], r1[s])
    assert not torch.equal(hyp[0], hyp[1]) and not torch.equal(rts[0][0], rts[0][2])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. modules
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_net", [True, False])
def test_depthnet_forward_batch_equals_single(model8, precision3, with_net):
    """DepthNet.forward at B = 3 on 16 x 20 maps with D = 8, hypotheses as the reference passes them (expanded [B,D,h,w])."""
    net = model8
    B, N, D, h, w = 3, 4, 8, 16, 20
    feats = [torch.cat([synth.smooth_features(N, 32, h, w, seed=21 + b)[v] for b in range(B)]).to(DEV) for v in range(N)]   # N x [B,32,h,w]
    pairs = _stage1_pairs(B, N)
    samples = _hyps(B, D).view(B, D, 1, 1).expand(B, D, h, w)
    pw = net.PixelwiseNet if with_net else None
    precision = precision3
    with torch.no_grad():
        got = net.depthnet(feats, pairs, depth_values=samples, num_depth=D, cost_regularization=net.cost_regularization, pixel_wise_net=pw, G=1)
        for i in range(B):
            want = net.depthnet([f[i:i + 1] for f in feats], pairs[i:i + 1], depth_values=samples[i:i + 1], num_depth=D,
                                cost_regularization=net.cost_regularization, pixel_wise_net=pw, G=1)
            assert set(got) == set(want)
            for k in want:
                if k == "view_weights" and not with_net:
                    assert got[k] == [] and want[k] == []
                    continue
                assert got[k][i].shape == want[k][0].shape, k
                assert torch.equal(got[k][i], want[k][0]), f"DepthNet.{k}: sample {i} differs ({precision}, view-weight net {with_net})"


@pytest.mark.parametrize("shape", [(3, 1, 8, 16, 20), (2, 1, 48, 16, 20)])
def test_cost_regularization_batch_equals_single(model8, precision3, shape):
    vol = _rand(*shape, seed=shape[2], scale=0.5)
    with torch.no_grad():
        prob, pro = model8.cost_regularization(vol)
        for i in range(shape[0]):
            p1, q1 = model8.cost_regularization(vol[i:i + 1])
            assert torch.equal(prob[i], p1[0]) and torch.equal(pro[i], q1[0]), f"cost_regularization {shape} {precision3}: sample {i}"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the whole path
# ---------------------------------------------------------------------------------------------------------------------------
def _batch_inputs(B, N, H, W, seed):
    """B samples that differ in images, cameras AND depth range."""
    parts = [synth.synth_sample(H, W, N, seed=seed + b) for b in range(B)]
    imgs = torch.cat([p[0] for p in parts]).to(DEV)
    pm = {}
    for k in parts[0][1]:
        cams = torch.cat([p[1][k] for p in parts]).clone()
        for b in range(B):
            cams[b, 1:, 0, :3, 3] *= 1.0 + 0.04 * b            # another baseline per sample
            cams[b, :, 1, 0, 0] *= 1.0 + 0.01 * b              # ... and another focal length
        pm[k] = cams.to(DEV)
    dv = torch.stack([torch.linspace(1.0 / (synth.DEPTH_MAX_MM + 35 * b), 1.0 / (synth.DEPTH_MIN_MM + 12 * b), synth.NUM_DEPTH_VALUES)
                      for b in range(B)]).to(DEV)
    return imgs, pm, dv


def _features(net, imgs):
    """What ``forward`` hands ``forward_hot``."""
    B, n_views = imgs.shape[:2]
    cnet = net.cnet_depth(imgs[:, 0])
    flat = net.feature(imgs.flatten(0, 1))
    per_view = {k: t_.unflatten(0, (B, n_views)) for k, t_ in flat.items()}
    return [{k: t_[:, v] for k, t_ in per_view.items()} for v in range(n_views)], cnet


def _assert_outputs_equal(got, want, i, what):
    assert len(got["depth"]) == 13 and len(want["depth"]) == 13
    for j, (a, b_) in enumerate(zip(got["depth"], want["depth"])):
        assert torch.equal(a[i], b_[0]), f"{what}: depth map {j} of sample {i} differs"
    assert torch.equal(got["photometric_confidence"][i], want["photometric_confidence"][0]), f"{what}: confidence of sample {i}"
    if "intermediates" in want:
        assert set(got["intermediates"]) == set(want["intermediates"])
        for k, v in want["intermediates"].items():
            assert torch.equal(got["intermediates"][k][i], v[0]), f"{what}: intermediate {k} of sample {i}"


@pytest.mark.parametrize("B", NS)
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("H,W", [(128, 160), (256, 320)])
@pytest.mark.parametrize("nd", ["48,8,8", "8,8,8"])
def test_forward_batch_equals_single_samples(model8, model48, precision3, nd, H, W, N, B):
    from effi_mvs_plus_amd import ops
    precision = precision3
    net = model48 if nd == "48,8,8" else model8
    imgs, pm, dv = _batch_inputs(B, N, H, W, seed=60)
    one = lambda i: (imgs[i:i + 1], {k: v[i:i + 1] for k, v in pm.items()}, dv[i:i + 1])
    with torch.no_grad():
        for opts in ({}, {"conf_fused": 0}, {"setup_fused": 0}):
            what = f"B={B} N={N} {H}x{W} {nd} {precision} {opts}"
            with ops.options(**opts):
                got = net(imgs, pm, dv)
                feats, cnet = _features(net, imgs)
                hot = net.forward_hot(feats, cnet, pm, dv, want_intermediates=True)
                for i in range(B):
                    im, p, d = one(i)
                    _assert_outputs_equal(got, net(im, p, d), i, "forward " + what)
                    f1, c1 = _features(net, im)
                    _assert_outputs_equal(hot, net.forward_hot(f1, c1, p, d, want_intermediates=True), i, "forward_hot " + what)


@pytest.mark.parametrize("B", NS)
def test_forward_hot_with_the_matrix_core_warp(model48, precision3, B):
    """Option warp_x3 = 1: ``_stage1_batch`` routes the stage-1 warp of all samples through the matrix-core form's batched entry
    (split products / hi * hi alone / in "fp32" the exact kernel), bitwise the per-sample passes under the same option."""
    from effi_mvs_plus_amd import ops
    imgs, pm, dv = _batch_inputs(B, 3, 128, 160, seed=90)
    with torch.no_grad(), ops.options(warp_x3=1):
        feats, cnet = _features(model48, imgs)
        hot = model48.forward_hot(feats, cnet, pm, dv, want_intermediates=True)
        for i in range(B):
            f1, c1 = _features(model48, imgs[i:i + 1])
            want = model48.forward_hot(f1, c1, {k: v[i:i + 1] for k, v in pm.items()}, dv[i:i + 1], want_intermediates=True)
            _assert_outputs_equal(hot, want, i, f"forward_hot warp_x3 B={B} {precision3}")


def test_forward_graph_replay_equals_eager_at_b2(model48, precision3):
    """graph.ForwardGraph over the batched stage 1: captured once, replayed on fresh inputs, bitwise the eager pass."""
    from effi_mvs_plus_amd.graph import ForwardGraph
    samples = [_batch_inputs(2, 3, 128, 160, seed=s) for s in (71, 75)]
    with torch.no_grad():
        g = ForwardGraph(model48, *samples[0])
        for smp in (samples[1], samples[0], samples[1]):
            want = model48(*smp)
            want = ([d.clone() for d in want["depth"]], want["photometric_confidence"].clone())
            got = g(*smp)
            assert len(got["depth"]) == 13
            for a, b_ in zip(got["depth"], want[0]):
                assert torch.equal(a, b_)
            assert torch.equal(got["photometric_confidence"], want[1])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. launch counts
# ---------------------------------------------------------------------------------------------------------------------------
def _launches(fn):
    from effi_mvs_plus_amd import ops
    prof = ops.KernelProfile()
    ops.set_profile(prof)
    try:
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
    finally:
        ops.set_profile(None)
    return sum(1 for r in prof.records if r[2] is not None)


def test_depthnet_forward_records_one_pass_of_launches(model8, precision3):
    net = model8
    B, N, D, h, w = 3, 4, 8, 16, 20
    feats = [torch.cat([synth.smooth_features(N, 32, h, w, seed=21 + b)[v] for b in range(B)]).to(DEV) for v in range(N)]
    pairs = _stage1_pairs(B, N)
    samples = _hyps(B, D).view(B, D, 1, 1).expand(B, D, h, w)
    run = lambda b: net.depthnet([f[:b] for f in feats], pairs[:b], depth_values=samples[:b], num_depth=D,
                                 cost_regularization=net.cost_regularization, pixel_wise_net=net.PixelwiseNet, G=1)
    with torch.no_grad():
        run(3)                                                          # warm-up: packs the weights
    one, three = _launches(lambda: run(1)), _launches(lambda: run(3))
    assert one >= 10 and three == one, (one, three)                     # the warp + the nine layers of the regulariser at least


def test_forward_hot_records_fewer_launches_than_the_loop(model48, precision3):
    net = model48
    imgs, pm, dv = _batch_inputs(3, 5, 128, 160, seed=80)
    with torch.no_grad():
        feats, cnet = _features(net, imgs)
        f1, c1 = _features(net, imgs[:1])
        net.forward_hot(feats, cnet, pm, dv)                            # warm-up
    L1 = _launches(lambda: net.forward_hot(f1, c1, {k: v[:1] for k, v in pm.items()}, dv[:1]))
    L3 = _launches(lambda: net.forward_hot(feats, cnet, pm, dv))
    assert L3 < 3 * L1, (L1, L3)
    assert L3 <= 3 * L1 - 2 * 9, (L1, L3)                               # the nine layers of the regulariser alone


# ---------------------------------------------------------------------------------------------------------------------------
# 5. argument checks
# ---------------------------------------------------------------------------------------------------------------------------
def test_mismatched_sample_counts_raise(model8):
    from effi_mvs_plus_amd import ops
    m = _conv3d_module(8, 8, 1, True, seed=1)
    wp, bp = m._packed()
    with pytest.raises(ValueError):
        ops.conv3d_k3([_rand(2, 4, 4, 8, 8), _rand(3, 4, 4, 8, 8)], wp, bp, 8)
    with pytest.raises(ValueError):
        ops.conv3d_k3([_rand(2, 8, 4, 8, 8)], wp, bp, 8, skip=_rand(3, 8, 4, 8, 8))
    with pytest.raises(ValueError):                                       # a sample that is not contiguous itself
        ops.conv3d_k3([_rand(2, 8, 4, 8, 16)[..., ::2]], wp, bp, 8)
    with pytest.raises(ValueError):
        ops.view_aggregate(_rand(2, 3, 4, 8, 8), _rand(3, 3, 8, 8))
    with pytest.raises(ValueError):
        ops.softmax_regress_conf(_rand(2, 8, 8, 8), _hyps(3, 8))
    with pytest.raises(ValueError):
        ops.softmax_regress_conf(_rand(2, 8, 8, 8), _hyps(2, 8), torch.rand(3, 384, device=DEV))
    rt = torch.stack([ops.compose_rel_proj(p) for p in _stage1_pairs(3, 3)])
    maps = _rand(2, 3, 16, 20, 32)
    with pytest.raises(ValueError):
        ops.warpcorr_views(maps[:, 0], [maps[:, 1], maps[:, 2]], rt, _hyps(2, 8), 8)
    with pytest.raises(ValueError):
        ops.warpcorr_views(maps[:, 0], [maps[:, 1], _rand(3, 16, 20, 32)], rt[:2], _hyps(2, 8), 8)
    with pytest.raises(ValueError):
        ops.cascade_setup(torch.rand(2, 384, device=DEV), 8, [_stage1_pairs(3, 3)])


def test_mismatched_shapes_raise(model8):
    """A wrong hypothesis count would read past the hypotheses; sources of different volumes past a volume."""
    from effi_mvs_plus_amd import ops
    m = _conv3d_module(8, 8, 1, True, seed=1)
    wp, bp = m._packed()
    with pytest.raises(ValueError):
        ops.conv3d_k3([_rand(2, 4, 4, 8, 8), _rand(2, 4, 5, 8, 8)], wp, bp, 8)
    rt = torch.stack([ops.compose_rel_proj(p) for p in _stage1_pairs(2, 3)])
    maps = _rand(2, 3, 16, 20, 32)
    for dep in (_hyps(2, 7), _hyps(2, 7)[0], _hyps(2, 8).view(2, 8, 1, 1).expand(2, 8, 16, 21), _hyps(2, 8).view(2, 2, 4)):
        with pytest.raises(ValueError):
            ops.warpcorr_views(maps[:, 0], [maps[:, 1], maps[:, 2]], rt, dep, 8)
    with pytest.raises(ValueError):
        ops.softmax_regress_conf(_rand(2, 8, 8, 8), _hyps(2, 9))


def test_wrappers_take_lists_of_per_sample_tensors():
    """A list of per-sample tensors in place of [n, ...]: ONE view over them when the samples sit at a uniform stride in one allocation
    (``as_samples``, no copy), else one gathered copy -- one launch and the same bits either way."""
    from effi_mvs_plus_amd import ops
    m = _conv3d_module(8, 8, 1, True, seed=2)
    wp, bp = m._packed()
    big = _rand(5, 8, 5, 9, 37, seed=6)
    v = ops.as_samples([big[0], big[2], big[4]])
    assert v is not None and tuple(v.shape) == (3, 8, 5, 9, 37) and v.data_ptr() == big.data_ptr() and v.stride(0) == 2 * big.stride(0)
    got = ops.conv3d_k3([v], wp, bp, 8)
    _assert_samples_equal(got, lambda i: ops.conv3d_k3([big[2 * i]], wp, bp, 8), 3, "as_samples")
    assert torch.equal(ops.conv3d_k3([[big[0], big[2], big[4]]], wp, bp, 8), got)          # the wrapper takes the list itself
    got = ops.conv3d_k3([[big[0], big[1], big[3]]], wp, bp, 8)                             # not at a uniform stride: gathered
    _assert_samples_equal(got, lambda i: ops.conv3d_k3([big[(0, 1, 3)[i]]], wp, bp, 8), 3, "list of samples")
    sims, ws = _rand(3, 2, 4, 8, 8, seed=7), torch.rand(3, 2, 8, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(ops.view_aggregate(list(sims), [w_ for w_ in ws]), ops.view_aggregate(sims, ws))
    logits, hyp = _rand(2, 8, 8, 8, seed=8), _hyps(2, 8)
    for a, b_ in zip(ops.softmax_regress_conf([logits[0], logits[1]], [hyp[0], hyp[1]]), ops.softmax_regress_conf(logits, hyp)):
        assert torch.equal(a, b_)
    maps = _rand(2, 3, 16, 20, 32, seed=9)
    rt = torch.stack([ops.compose_rel_proj(p) for p in _stage1_pairs(2, 3)])
    got = ops.warpcorr_views([maps[0, 0], maps[1, 0]], [[maps[0, 1], maps[1, 1]], [maps[0, 2], maps[1, 2]]], [rt[0], rt[1]], hyp, 8)
    for a, b_ in zip(got, ops.warpcorr_views(maps[:, 0], [maps[:, 1], maps[:, 2]], rt, hyp, 8)):
        assert torch.equal(a, b_)
    assert ops.as_samples([big[0], big[1], big[3]]) is None                 # not uniform
    assert ops.as_samples([big[2], big[1]]) is None                         # descending
    assert ops.as_samples([big[0], big[1].clone()]) is None                 # two allocations
    assert tuple(ops.as_samples([big[3]]).shape) == (1, 8, 5, 9, 37)


def test_one_sample_through_a_batch_entry_is_the_plain_entry(precision3):
    """n = 1 with a leading dimension goes through the _batch entry, which launches the single-sample kernel itself."""
    from effi_mvs_plus_amd import ops
    for cin, cout, stride in ((1, 8, 1), (8, 8, 1), (8, 16, 2), (32, 32, 1)):
        m = _conv3d_module(cin, cout, stride, True, seed=cin)
        x = _rand(1, cin, 9, 12, 40, seed=cin)
        with torch.no_grad():
            assert torch.equal(m.run([x])[0], m.run([x[0]]))
    h, w, C, D = 16, 20, 32, 8
    maps = _rand(1, 3, h, w, C, seed=3)
    rt = torch.stack([ops.compose_rel_proj(p) for p in _stage1_pairs(1, 3)])
    hyp = _hyps(1, D)
    sim, ent = ops.warpcorr_views(maps[:, 0], [maps[:, 1], maps[:, 2]], rt, hyp, D)
    s1, e1 = ops.warpcorr_views(maps[0, 0], [maps[0, 1], maps[0, 2]], rt[0], hyp[0], D)
    assert torch.equal(sim[0], s1) and torch.equal(ent[0], e1)
    logits = _rand(1, D, h, w, seed=4)
    for a, b_ in zip(ops.softmax_regress_conf(logits, hyp, conf_up=4), ops.softmax_regress_conf(logits[0], hyp[0], conf_up=4)):
        assert torch.equal(a[0], b_)
    sims = _rand(1, 2, D, h, w, seed=5)
    assert torch.equal(ops.view_aggregate(sims, None)[0], ops.view_aggregate(sims[0], None))
