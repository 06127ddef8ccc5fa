"""GPU: the feature pyramid over all images of a call in batched launches (option ``fpn_batch``).

  * every ``*_batch`` entry of the library, through its ``ops`` wrapper: image i of a batched launch == the 3-D call on image i;
  * ``P_1to8_FeatureNet_Fast`` (``net.feature``, ``net.cnet_depth``) on [n,3,H,W] == the per-image passes, for every value of the option;
  * launch counts: a batched pass records as many launches for 5 images as for 1 (this is what fails without the feature);
  * the whole ``Effi_MVS_plus.forward`` and its graph replay, identical for ``fpn_batch`` 0 / 1 / 2.

The bar is BITWISE (torch.equal) everywhere: both sides are this library, a batched launch offsets its pointers per image and runs the
single-image tile body, and a pixel's accumulation order does not depend on the tile shape the launch rule picks.
"""
import pytest
import torch

from common import build_model
from effi_mvs_plus_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 2, 5)

# (h, w) of the convolution's OUTPUT map:
#   96 x 256   one row per wave on its own (96 / 192 tiles of 16 / 8 rows), n = 5 crosses mr4_min = 400 (split) and the 512 of the fp32 rule
#   104 x 256  n = 2 crosses mr2_min (208 -> 416 tiles of 8 rows); the last 16-row tile is cut by the map edge
#   52 x 72    w % 16 != 0 and the last tile of every tile height is cut in both directions (neighbour-image pixels would show)
SHAPES = [(96, 256), (104, 256), (52, 72)]


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _weights(cout, cin, ks, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(cout, cin, ks, ks, generator=g) * (1.0 / (cin * ks * ks) ** 0.5)).to(DEV), (torch.randn(cout, generator=g) * 0.1).to(DEV)


@pytest.fixture
def with_precision():
    from effi_mvs_plus_amd import ops
    before = ops.get_precision()

    def set_(p):
        ops.set_precision(p)
    yield set_
    ops.set_precision(before)


def _assert_images_equal(batched, single_fn, n, what):
    for i in range(n):
        want = single_fn(i)
        assert batched[i].shape == want.shape, (what, i, batched[i].shape, want.shape)
        assert torch.equal(batched[i], want), f"{what}: image {i} of {n} differs from the single-image launch"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. per kernel: batched == single
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("ks,cin,cout,epi", [(3, 8, 16, "plain"), (3, 16, 64, "nhwc"), (1, 32, 64, "plain"), (1, 64, 32, "nhwc"),
                                             (1, 16, 64, "add_up2")])
def test_conv2d_batch_equals_single(precision, n, h, w, ks, cin, cout, epi):
    """ops.conv2d (effi_conv2d_f32_batch in "fp32"; its 3x3 PLAIN / NHWC layers go to effi_conv2d_k3_bf16x3_f32_batch in "split")."""
    from effi_mvs_plus_amd import ops, packing
    wt, bs = _weights(cout, cin, ks, seed=cin + cout)
    wp, bp = packing.pack_conv2d(wt, bs)
    x = _rand(n, cin, h, w, seed=h + n)
    kw = {"epilogue": {"plain": ops.EPI_PLAIN, "nhwc": ops.EPI_NHWC, "add_up2": ops.EPI_ADD_UP2}[epi], "act": ops.ACT_RELU}
    aux = _rand(n, cout, h // 2, w // 2, seed=7) if epi == "add_up2" else None
    got = ops.conv2d([x], wp, bp, cout, ks, aux0=aux, **kw)
    assert tuple(got.shape) == ((n, h, w, cout) if epi == "nhwc" else (n, cout, h, w))
    _assert_images_equal(got, lambda i: ops.conv2d([x[i]], wp, bp, cout, ks, aux0=None if aux is None else aux[i], **kw), n,
                         f"conv2d k{ks} {cin}->{cout} {epi} {h}x{w} {precision}")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h,w", [(40, 46), (70, 50)])
def test_conv2d_batch_unaligned_rows(precision, n, h, w):
    """w % 4 != 0: the 16 x 16 fp32 kernel with the image in blockIdx.z (both precisions fall to it)."""
    from effi_mvs_plus_amd import ops, packing
    wt, bs = _weights(32, 16, 3, seed=3)
    wp, bp = packing.pack_conv2d(wt, bs)
    x = _rand(n, 16, h, w, seed=n)
    got = ops.conv2d([x], wp, bp, 32, 3, act=ops.ACT_RELU)
    _assert_images_equal(got, lambda i: ops.conv2d([x[i]], wp, bp, 32, 3, act=ops.ACT_RELU), n, f"conv2d unaligned {h}x{w}")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("epi", ["plain", "nhwc", "add_shuf2", "nhwc_add_shuf2"])
@pytest.mark.parametrize("prec", ["split", "bf16"])
def test_conv2d_k3_bf16x3_batch_equals_single(with_precision, prec, epi, h, w, n):
    """effi_conv2d_k3_bf16x3_f32_batch(_bf16), every epilogue of the pyramid, with the constant "ones" plane as a stride-0 source."""
    from effi_mvs_plus_amd import ops, packing
    with_precision(prec)
    cin, cout = 16, (16 if "shuf2" in epi else 32)
    wt, bs = _weights(cout, cin + 1, 3, seed=5)
    wp, bp = packing.pack_conv2d_bf16x3(wt, bs)
    x = _rand(n, cin, h, w, seed=h + 3 * n)
    ones = torch.ones(1, h, w, device=DEV)
    e = {"plain": ops.EPI_PLAIN, "nhwc": ops.EPI_NHWC, "add_shuf2": ops.EPI_ADD_SHUF2, "nhwc_add_shuf2": ops.EPI_NHWC_ADD_SHUF2}[epi]
    act = ops.ACT_NONE if "shuf2" in epi else ops.ACT_RELU
    aux = _rand(n, 4 * cout, h // 2, w // 2, seed=11) if "shuf2" in epi else None
    got = ops.conv2d_k3_bf16x3([x, ones], wp, bp, cout, epilogue=e, act=act, aux0=aux)
    assert tuple(got.shape) == ((n, h, w, cout) if "nhwc" in epi else (n, cout, h, w))
    _assert_images_equal(got, lambda i: ops.conv2d_k3_bf16x3([x[i], ones], wp, bp, cout, epilogue=e, act=act,
                                                              aux0=None if aux is None else aux[i]), n, f"k3 x3 {epi} {h}x{w} {prec}")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h,w", SHAPES + [(21, 25)])
@pytest.mark.parametrize("cin,cout", [(8, 16), (32, 64)])
@pytest.mark.parametrize("prec", ["fp32", "split", "bf16"])
def test_conv2d_k5s2_batch_equals_single(with_precision, prec, cin, cout, h, w, n):
    """effi_conv2d_k5s2_f32_batch / effi_conv2d_k5s2_bf16x3_f32_batch(_bf16); output h x w from an input 2h x 2w (21 x 25: input rows of
    50 floats, the unaligned fp32 form in every precision)."""
    from effi_mvs_plus_amd import ops, packing
    with_precision(prec)
    wt, bs = _weights(cout, cin, 5, seed=cin)
    wp, bp = packing.pack_conv2d(wt, bs)
    x = _rand(n, cin, 2 * h, 2 * w, seed=w + n)
    got = ops.conv2d_k5s2(x, wp, bp, cout)
    assert tuple(got.shape) == (n, cout, h, w)
    _assert_images_equal(got, lambda i: ops.conv2d_k5s2(x[i], wp, bp, cout), n, f"k5s2 {cin}->{cout} {h}x{w} {prec}")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h,w", [(400, 400), (52, 72), (96, 256)])
@pytest.mark.parametrize("prec", ["split", "bf16"])
def test_conv2d_k3_twice_batch_equals_single(with_precision, prec, h, w, n):
    """The persistent kernel: 400 x 400 is 625 tiles per image -- n = 2 and 5 make 1250 / 3125 (image, tile) pairs on 1024 workgroups, so
    workgroups walk 2 / 4 tiles, their runs cross image boundaries and the last workgroups get a short run."""
    from effi_mvs_plus_amd import ops, packing
    with_precision(prec)
    w1, b1 = _weights(8, 3, 3, seed=1)
    w2, b2 = _weights(8, 8, 3, seed=2)
    p1, pb1 = packing.pack_conv2d_bf16x3_oct(w1, b1)
    p2, pb2 = packing.pack_conv2d_bf16x3_oct(w2, b2)
    x = _rand(n, 3, h, w, seed=h + n)
    got = ops.conv2d_k3_twice(x, p1, pb1, p2, pb2, 8)
    assert tuple(got.shape) == (n, 8, h, w)
    _assert_images_equal(got, lambda i: ops.conv2d_k3_twice(x[i], p1, pb1, p2, pb2, 8), n, f"k3 twice {h}x{w} {prec}")


def test_batch_with_uniform_image_stride_is_accepted(precision):
    """A batch need not be contiguous: every second image of a larger tensor, or a channel range of it, has contiguous images at a
    uniform stride and is launched in place; images that are not contiguous themselves are rejected."""
    from effi_mvs_plus_amd import ops, packing
    wt, bs = _weights(16, 8, 3, seed=9)
    wp, bp = packing.pack_conv2d(wt, bs)
    big = _rand(6, 12, 52, 72, seed=4)
    for x in (big[::2, :8], big[1:4, 4:12]):
        assert not x.is_contiguous()
        got = ops.conv2d([x], wp, bp, 16, 3, act=ops.ACT_RELU)
        _assert_images_equal(got, lambda i: ops.conv2d([x[i].contiguous()], wp, bp, 16, 3, act=ops.ACT_RELU), 3, "strided batch")
    w5, b5 = _weights(16, 8, 5, seed=9)
    wp5, bp5 = packing.pack_conv2d(w5, b5)
    x = big[::2, :8]
    got = ops.conv2d_k5s2(x, wp5, bp5, 16)
    _assert_images_equal(got, lambda i: ops.conv2d_k5s2(x[i].contiguous(), wp5, bp5, 16), 3, "strided batch k5s2")
    with pytest.raises(ValueError):
        ops.conv2d([big[:, :8].transpose(-1, -2)], wp, bp, 16, 3)
    with pytest.raises(ValueError):
        ops.conv2d([big[:, :8, :, ::2]], wp, bp, 16, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. error paths
# ---------------------------------------------------------------------------------------------------------------------------
def test_mismatched_image_counts_raise():
    from effi_mvs_plus_amd import ops, packing
    wt, bs = _weights(16, 16, 3, seed=9)
    wp, bp = packing.pack_conv2d(wt, bs)
    with pytest.raises(ValueError):
        ops.conv2d([_rand(2, 8, 16, 16), _rand(3, 8, 16, 16)], wp, bp, 16, 3)
    wt1, bs1 = _weights(16, 16, 1, seed=9)
    wp1, bp1 = packing.pack_conv2d(wt1, bs1)
    with pytest.raises(ValueError):
        ops.conv2d([_rand(2, 16, 16, 16)], wp1, bp1, 16, 1, epilogue=ops.EPI_ADD_UP2, aux0=_rand(3, 16, 8, 8))
    wx, bx = packing.pack_conv2d_bf16x3(wt, bs)
    with pytest.raises(ValueError):
        ops.conv2d_k3_bf16x3([_rand(2, 8, 16, 16), _rand(4, 8, 16, 16)], wx, bx, 16)
    with pytest.raises(ValueError):                      # a shared 3-D source of another map size
        ops.conv2d_k3_bf16x3([_rand(2, 8, 16, 16), _rand(8, 16, 20)], wx, bx, 16)


@pytest.mark.parametrize("prec", ["fp32", "split"])
def test_unsupported_epilogue_for_several_images_raises(with_precision, prec):
    """The epilogues the pyramid does not use are single-image only: the library answers EFFI_ERR_UNSUPPORTED (-2) for n_img > 1 and
    runs them for n_img = 1."""
    from effi_mvs_plus_amd import ops, packing
    from effi_mvs_plus_amd._lib import EffiLibraryError, lib
    with_precision(prec)
    wt, bs = _weights(32, 16, 3, seed=2)
    wp, bp = packing.pack_conv2d(wt, bs)
    x, hst, z = _rand(2, 16, 32, 32), _rand(2, 32, 32, 32, seed=1), _rand(2, 32, 32, 32, seed=2)
    unsupported = lib().effi_error_string(-2).decode()
    with pytest.raises(EffiLibraryError) as ei:
        ops.conv2d([x], wp, bp, 32, 3, epilogue=ops.EPI_GRU_Q, aux0=hst, aux1=z)
    assert "code -2" in str(ei.value) and unsupported in str(ei.value)
    got = ops.conv2d([x[:1]], wp, bp, 32, 3, epilogue=ops.EPI_GRU_Q, aux0=hst[:1], aux1=z[:1])
    assert torch.equal(got[0], ops.conv2d([x[0]], wp, bp, 32, 3, epilogue=ops.EPI_GRU_Q, aux0=hst[0], aux1=z[0]))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the pyramid
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return build_model("8,8,8", seed=17, device=DEV)[0]


def _pyramid_equal(mod, x, what, strides=True):
    """``strides``: the batched pass presents image i exactly like the single-image pass (same per-image strides: channel-last where
    that one is); the per-image loop (fpn_batch = 0) re-stacks its maps and is only compared by value."""
    with torch.no_grad():
        got = mod(x)
        for i in range(x.shape[0]):
            want = mod(x[i:i + 1])
            assert set(got) == set(want)
            for k in want:
                assert got[k][i].shape == want[k][0].shape, (what, k)
                if strides:
                    assert got[k][i].stride() == want[k][0].stride(), (what, k, got[k][i].stride(), want[k][0].stride())
                assert torch.equal(got[k][i], want[k][0]), f"{what}: {k} of image {i} differs from the single-image pass"
    return got


@pytest.mark.parametrize("H,W", [(64, 96), (256, 320), (1184, 1600)])
@pytest.mark.parametrize("which", ["feature", "cnet_depth"])
def test_pyramid_batch_equals_per_image(model, precision, which, H, W):
    from effi_mvs_plus_amd import ops
    mod = getattr(model, which)
    x = torch.rand(5, 3, H, W, generator=torch.Generator().manual_seed(H)).to(DEV)
    for v in (0, 1, 2):
        with ops.options(fpn_batch=v):
            got = _pyramid_equal(mod, x, f"{which} {H}x{W} fpn_batch={v} {precision}", strides=v != 0)
    # what forward_hot does with the maps: per-view, per-sample slices into ops.to_nhwc (channel-last passes through without a copy
    # when W % 32 == 0, planar maps are transposed otherwise)
    with ops.options(fpn_batch=2):
        for k, t_ in got.items():
            assert t_.shape[0] == 5 and t_.dim() == 4
            maps = ops.to_nhwc([t_[i] for i in range(5)])
            for i, m in enumerate(maps):
                assert torch.equal(m, t_[i].permute(1, 2, 0))
                if which == "feature" and W % 32 == 0:
                    assert m.data_ptr() == t_[i].data_ptr()            # already channel-last: no copy
    with ops.options(fpn_batch=2, fpn_conv0_fused=0, fpn_split_head=0):
        _pyramid_equal(mod, x, f"{which} {H}x{W} unfused forms {precision}")


def test_pyramid_batch_accepts_a_strided_view_batch(model):
    """``imgs[:, 0]`` of [B,N,3,H,W] (what the context net receives): images contiguous, image stride N*3*H*W."""
    imgs = torch.rand(2, 3, 3, 64, 96, generator=torch.Generator().manual_seed(2)).to(DEV)
    _pyramid_equal(model.cnet_depth, imgs[:, 0], "strided views")
    _pyramid_equal(model.feature, imgs[:, 1], "strided views")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. launch counts
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


@pytest.mark.parametrize("H,W", [(128, 160), (256, 320)])
def test_batched_pyramid_records_one_pass_of_launches(model, precision, H, W):
    from effi_mvs_plus_amd import ops
    imgs, pm, dv = synth.synth_sample(H, W, 5, seed=3)
    imgs, pm, dv = imgs.to(DEV), {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV)
    x = imgs[0]
    with torch.no_grad():
        model(imgs, pm, dv)                                                      # packs weights, registers the workspace
    with ops.options(fpn_batch=2):
        one = _launches(lambda: model.feature(x[:1]))
        five = _launches(lambda: model.feature(x))
        whole2 = _launches(lambda: model(imgs, pm, dv))
    assert one > 0 and five == one, (one, five)
    with ops.options(fpn_batch=0):
        assert _launches(lambda: model.feature(x)) == 5 * one
        whole0 = _launches(lambda: model(imgs, pm, dv))
    assert whole0 - whole2 == 4 * one, (whole0, whole2, one)
    whole1 = _launches(lambda: model(imgs, pm, dv))                              # the default rule
    assert ops.option("fpn_batch") == 1
    assert whole1 < whole0, (whole1, whole0)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the whole forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("H,W", [(128, 160), (256, 320)])
def test_forward_is_identical_for_every_fpn_batch(model, precision, H, W, N, B):
    from effi_mvs_plus_amd import ops
    parts = [synth.synth_sample(H, W, N, seed=40 + b) for b in range(B)]
    imgs = torch.cat([p[0] for p in parts]).to(DEV)
    pm = {k: torch.cat([p[1][k] for p in parts]).to(DEV) for k in parts[0][1]}
    dv = torch.cat([p[2] for p in parts]).to(DEV)
    outs = []
    with torch.no_grad():
        for v in (0, 1, 2):
            with ops.options(fpn_batch=v):
                o = model(imgs, pm, dv)
                outs.append(([d.clone() for d in o["depth"]], o["photometric_confidence"].clone()))
    assert len(outs[0][0]) == 13
    for v in (1, 2):
        for a, b in zip(outs[v][0], outs[0][0]):
            assert a.shape[0] == B and torch.equal(a, b), f"fpn_batch={v}: a depth map differs from the per-image pyramid's"
        assert torch.equal(outs[v][1], outs[0][1])


@pytest.mark.parametrize("fpn_batch", [1, 2])
def test_forward_graph_replay_equals_eager(model, precision, fpn_batch):
    """graph.ForwardGraph over the batched pyramid: captured once, replayed with fresh inputs, bitwise the eager pass."""
    from effi_mvs_plus_amd import ops
    from effi_mvs_plus_amd.graph import ForwardGraph
    samples = []
    for seed in (51, 52):
        imgs, pm, dv = synth.synth_sample(128, 160, 3, seed=seed)
        samples.append((imgs.to(DEV), {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV)))
    with ops.options(fpn_batch=fpn_batch), torch.no_grad():
        g = ForwardGraph(model, *samples[0])
        for smp in (samples[1], samples[0], samples[1]):
            want = model(*smp)
            want = ([d.clone() for d in want["depth"]], want["photometric_confidence"].clone())
            got = g(*smp)
            assert len(got["depth"]) == 13
            for a, b in zip(got["depth"], want[0]):
                assert torch.equal(a, b)
            assert torch.equal(got["photometric_confidence"], want[1])
