"""Scope row n2 past one workgroup and at the reference's training configuration.

The operator tests of tests/test_gpu_train.py run at sizes where every training kernel keeps its one-workgroup form: one split per
channel in the per-channel reductions, one strip in the weight gradients, grid-stride loops that run once, a single workgroup of
per-pixel threads.  The cases here run the same kernels where those forms change -- the split reductions at the shapes of a
``48,8,8`` training forward at B = 4, N = 3, 512x640 (the reference's train.py configuration), forced splits at awkward small shapes,
strip-parallel weight gradients, capped grid-stride loops, per-pixel backward kernels and warps at the training maps -- and one whole
step at B = 4 with 48 stage-1 hypotheses.

Yardstick of every operator case: the same operation in torch float64 on the CPU.  e_hip = rel(hip, fp64) relative to the tensor's
peak; e_ref = rel(torch CPU float32, fp64) on identical inputs; bound max(2e-5, 4 e_ref) (the operator bound of test_gpu_train.py and
its 4 e_ref rule); warp backward cases keep their bounds of test_gpu_train.py (2e-4 similarity, 1e-3 gradients) with the same
4 e_ref escape.  Every case prints e_hip and e_ref, and asserts, through ``launch_shape``, the launch regime it is named for.
"""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from common import build_model, t
from effi_mvs_plus_amd import synth
from test_gpu_train import DLOSS, _loss_inputs, _oracle_training_pass, leaf, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_TR, W_TR, B_TR, N_TR = 512, 640, 4, 3          # reference train.py:36,55,66 / datasets/dtu_yao.py:84: batch 4, 3 views, 640x512 crops


# ---- the launch shape the library chooses --------------------------------------------------------------------------------------
TPB = 256
# wgrad_nd_kernel<KD, KS, CAB> instantiations: effi_conv_wgrad_f32 (csrc/train_ops.hip), EFFI_WG(KD, KS, CAB)
WGRAD_CAB = {(1, 1): 16, (1, 3): 8, (1, 5): 4, (1, 7): 2, (3, 3): 4}


def launch_shape(kind, **a):
    """What the library launches for one call.

    reduce    (B, n)                  -> nsplit: workgroups per channel of channel_sum / bn_train_fwd / bn_bwd (ops._reduce_split)
    wgrad     (ca, cb, na, kd, ks)    -> strips (grid z) of wgrad_nd_kernel
    plane     (n, planes)             -> (workgroups one plane needs, cap) of bn_apply_kernel / bn_bwd_apply_kernel (effi_plane_grid)
    pointwise (n)                     -> (workgroups needed, cap) of pointwise_kernel (effi_pointwise_f32)
    """
    from effi_mvs_plus_amd import ops
    if kind == "reduce":
        return ops._reduce_split(a["B"] * a["n"], 1)[1]
    if kind == "wgrad":
        # strips_for, restated from effi_conv_wgrad_f32 (csrc/train_ops.hip:576-581)
        blocks = -(-a["ca"] // WGRAD_CAB[(a["kd"], a["ks"])]) * a["cb"]
        na = a["na"]
        st = max(1, min(64, na // 8192))
        while blocks * st < 768 and na // st > 2048 and st < 64:
            st *= 2
        return st
    if kind == "plane":
        # effi_plane_grid (csrc/train_ops.hip:600-605): ~4 elements per thread, at most 16384 workgroups over all planes
        return -(-a["n"] // (4 * TPB)), max(1, 16384 // a["planes"])
    if kind == "pointwise":
        return -(-a["n"] // TPB), 16384             # effi_pointwise_f32: min(ceil(n / TPB), 16384) workgroups
    raise KeyError(kind)


def _bn_n(shape):
    return math.prod(shape[2:])


class Table:
    """Records e_hip / e_ref per compared tensor, prints them, and fails at the end with every offender named."""

    def __init__(self, case):
        self.case, self.fail = case, []

    def __call__(self, name, got, want64, ref32, floor=2e-5):
        e_hip, e_ref = rel(got, want64), rel(ref32, want64)
        bound = max(floor, 4 * e_ref)
        ok = e_hip <= bound
        print(f"[{self.case}] {name:28s} e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}{'' if ok else '   FAIL'}")
        if not ok:
            self.fail.append(f"{name}: {e_hip:.3e} > {bound:.3e} (e_ref {e_ref:.3e})")

    def fixed(self, name, got, want64, bound):
        e_hip = rel(got, want64)
        ok = e_hip <= bound
        print(f"[{self.case}] {name:28s} e_hip {e_hip:.3e}  bound {bound:.3e}{'' if ok else '   FAIL'}")
        if not ok:
            self.fail.append(f"{name}: {e_hip:.3e} > {bound:.3e}")

    def check(self):
        assert not self.fail, f"{self.case}: " + "; ".join(self.fail)


# ---- shapes of one training forward at the reference's configuration -------------------------------------------------------------
@pytest.fixture(scope="module")
def train_shapes():
    """BatchNorm input shapes and biased-convolution output shapes of ONE training-mode forward of build_model("48,8,8") at B = 4,
    N = 3, 512x640, recorded by wrapping the two autograd entries train_path calls for them."""
    from effi_mvs_plus_amd import autograd as A
    net, _ = build_model("48,8,8", seed=13, device=DEV)
    net.train()
    samples = [synth.synth_sample(H_TR, W_TR, N_TR, seed=60 + b) for b in range(B_TR)]
    imgs = torch.cat([s[0] for s in samples]).to(DEV)
    pm = {k: torch.cat([s[1][k] for s in samples]).to(DEV) for k in samples[0][1]}
    dv = torch.cat([s[2] for s in samples]).to(DEV)
    bn_shapes, bias_shapes = [], []
    bn0, conv0 = A.batch_norm_train, A.conv2d

    def bn_hook(x, bn, relu):
        bn_shapes.append(tuple(x.shape))
        return bn0(x, bn, relu)

    def conv_hook(xs, weight, bias=None, act=0):
        y = conv0(xs, weight, bias, act)
        if bias is not None:
            bias_shapes.append(tuple(y.shape))
        return y

    A.batch_norm_train, A.conv2d = bn_hook, conv_hook
    try:
        with torch.no_grad():
            net(imgs, pm, dv)
        torch.cuda.synchronize()
    finally:
        A.batch_norm_train, A.conv2d = bn0, conv0
    bn_u, bias_u = sorted(set(bn_shapes)), sorted(set(bias_shapes))
    print(f"[48,8,8 forward, B={B_TR} N={N_TR} {H_TR}x{W_TR}] {len(bn_shapes)} BatchNorm calls, {len(bn_u)} shapes (shape: nsplit):")
    for s in bn_u:
        print(f"    {s}: {launch_shape('reduce', B=s[0], n=_bn_n(s))}")
    print(f"[48,8,8 forward] {len(bias_shapes)} biased convolutions, {len(bias_u)} output shapes (shape: nsplit):")
    for s in bias_u:
        print(f"    {s}: {launch_shape('reduce', B=s[0], n=_bn_n(s))}")
    return bn_u, bias_u


def _pick(train_shapes, which):
    """One recorded shape per named regime."""
    bn_u, bias_u = train_shapes
    ns = lambda s: launch_shape("reduce", B=s[0], n=_bn_n(s))                 # noqa: E731
    if which == "fpn_conv0":              # feature pyramid conv0 at full resolution (models/module.py:239)
        cands = [s for s in bn_u if len(s) == 4 and s[2:] == (H_TR, W_TR)]
    elif which == "stage1_d48":           # stage-1 cost regularisation volume at 48 hypotheses
        cands = sorted([s for s in bn_u if len(s) == 5 and s[2] == 48], key=lambda s: -math.prod(s))
    elif which == "bn_mid":               # a split count strictly between 1 and the cap
        cands = sorted([s for s in bn_u if 1 < ns(s) < 256], key=ns)
    elif which == "bias_full":            # the largest biased-convolution output
        cands = sorted(bias_u, key=lambda s: -math.prod(s))
    elif which == "bias_mid":
        cands = sorted([s for s in bias_u if 1 < ns(s) < 256], key=ns)
    else:
        raise KeyError(which)
    assert cands, f"the 48,8,8 training forward has no shape for regime {which}"
    return cands[0]


# ---- BatchNorm forward / backward / channel sum against fp64 ----------------------------------------------------------------------
def _bn_inputs(shape, seed, offset=None):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    bs = (1, C) + (1,) * (len(shape) - 2)
    sig = 0.5 + 1.5 * torch.rand(C, generator=g)
    mu = offset * sig if offset is not None else torch.randn(C, generator=g)
    x = torch.randn(shape, generator=g) * sig.view(bs) + mu.view(bs)
    gy = torch.randn(shape, generator=g) + 0.3 * torch.randn(C, generator=g).view(bs)
    par = {"weight": 0.5 + torch.rand(C, generator=g), "bias": torch.randn(C, generator=g) * 0.2,
           "running_mean": torch.randn(C, generator=g) * 0.1, "running_var": 0.5 + torch.rand(C, generator=g)}
    return x, gy, par


def _bn_hip(x, gy, par, relu, nt0=5):
    from effi_mvs_plus_amd import ops
    d = {k: v.to(DEV) for k, v in par.items()}
    nt = torch.tensor(nt0, dtype=torch.int64, device=DEV)
    xd, gyd = x.to(DEV), gy.to(DEV)
    y, mean, invstd = ops.bn_train_fwd(xd, d["weight"], d["bias"], 1e-5, 0.1, d["running_mean"], d["running_var"], nt, relu)
    gx, s1, s2 = ops.bn_bwd(gyd, y, xd, mean, invstd, d["weight"], relu)
    cs = ops.channel_sum(gyd)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, invstd=invstd, rm=d["running_mean"], rv=d["running_var"], nt=nt, gx=gx, s1=s1, s2=s2, cs=cs)


def _bn_cpu(x, gy, par, relu, mask, dtype):
    """nn.BatchNorm in train mode on the CPU in ``dtype``; the backward is fed gy times ``mask`` (the ReLU mask of the HIP forward's
    own output: bn_bwd takes y as input, so its arithmetic is tested exactly instead of gating on ReLU flips)."""
    C = x.shape[1]
    m = (nn.BatchNorm3d if x.dim() == 5 else nn.BatchNorm2d)(C, momentum=0.1).to(dtype)
    with torch.no_grad():
        for k, v in par.items():
            getattr(m, k).copy_(v.to(dtype))
    m.train()
    xl = leaf(x.to(dtype))
    y = m(xl)
    g = gy.to(dtype) * mask.to(dtype)
    y.backward(g)
    dims = [0] + list(range(2, x.dim()))
    var, mean = torch.var_mean(x.to(dtype), dims, unbiased=False)
    return dict(y=F.relu(y) if relu else y, mean=mean, invstd=1.0 / torch.sqrt(var + m.eps), rm=m.running_mean, rv=m.running_var,
                nbt=int(m.num_batches_tracked), gx=xl.grad, s1=m.bias.grad, s2=m.weight.grad, cs=gy.to(dtype).sum(dims))


def _bn_check(case, shape, relu, seed, offset=None):
    x, gy, par = _bn_inputs(shape, seed, offset)
    hip = _bn_hip(x, gy, par, relu)
    mask = (hip["y"].cpu() > 0) if relu else torch.ones(())
    want, ref = _bn_cpu(x, gy, par, relu, mask, torch.float64), _bn_cpu(x, gy, par, relu, mask, torch.float32)
    tab = Table(case)
    for k, name in (("y", "bn_train_fwd y"), ("mean", "bn_train_fwd mean"), ("invstd", "bn_train_fwd invstd"), ("gx", "bn_bwd gx"),
                    ("s1", "bn_bwd s1 (grad beta)"), ("s2", "bn_bwd s2 (grad gamma)"), ("cs", "channel_sum")):
        tab(name, hip[k], want[k], ref[k])
    tab.fixed("running_mean", hip["rm"], want["rm"], 1e-6)         # as test_gpu_train.py::test_batch_norm_training_mode
    tab.fixed("running_var", hip["rv"], want["rv"], 1e-6)
    tab.check()
    assert int(hip["nt"]) == 6 and want["nbt"] == 1                  # num_batches_tracked advanced by exactly one
    return hip


@pytest.mark.parametrize("which", ["fpn_conv0", "stage1_d48", "bn_mid"])
def test_split_batch_norm_at_the_training_shapes(train_shapes, which):
    """Case 1: bn_train_fwd / bn_bwd / channel_sum at BatchNorm shapes of the 48,8,8 training forward (ReLU fused, as on the path)."""
    shape = _pick(train_shapes, which)
    ns = launch_shape("reduce", B=shape[0], n=_bn_n(shape))
    print(f"[{which}] shape {shape}: nsplit {ns}")
    if which == "bn_mid":
        assert 1 < ns < 256
    else:
        assert ns == 256                                            # the cap
    if which == "fpn_conv0":
        assert shape[0] * _bn_n(shape) == B_TR * H_TR * W_TR
    _bn_check(f"bn {which} {shape}", shape, True, seed=sum(shape))


@pytest.mark.parametrize("which", ["bias_full", "bias_mid"])
def test_split_channel_sum_at_the_bias_gradient_shapes(train_shapes, which):
    """Case 1: channel_sum (bias gradients) at biased-convolution output shapes of the 48,8,8 training forward."""
    from effi_mvs_plus_amd import ops
    shape = _pick(train_shapes, which)
    ns = launch_shape("reduce", B=shape[0], n=_bn_n(shape))
    print(f"[{which}] shape {shape}: nsplit {ns}")
    assert 1 < ns < 256 if which == "bias_mid" else ns > 1
    g = torch.Generator().manual_seed(sum(shape))
    bs = (1, shape[1]) + (1,) * (len(shape) - 2)
    gy = torch.randn(shape, generator=g) + 0.3 * torch.randn(shape[1], generator=g).view(bs)
    dims = [0] + list(range(2, len(shape)))
    got = ops.channel_sum(gy.to(DEV))
    tab = Table(f"channel_sum {which} {shape}")
    tab("channel_sum", got, gy.double().sum(dims), gy.sum(dims))
    tab.check()


# case 2: forced splits (reduce_chunk k) at awkward small shapes, B = 3, planes shorter than 256 elements
FORCED = [(s, k) for s in ((3, 5, 7, 11), (3, 4, 5, 6, 7), (3, 5, 9, 11), (3, 3, 13, 17)) for k in (1, 7, 64)]


def _split_layout(shape, k):
    """(nsplit, elements per split, empty trailing splits, whether a split boundary falls inside a sample) under reduce_chunk = k."""
    from effi_mvs_plus_amd import ops
    with ops.options(reduce_chunk=k):
        ns = launch_shape("reduce", B=shape[0], n=_bn_n(shape))
    total, n = shape[0] * _bn_n(shape), _bn_n(shape)
    per = -(-total // ns)
    used = -(-total // per)
    return ns, per, ns - used, any((j * per) % n for j in range(1, used))


def test_forced_split_layouts_cover_the_edges():
    """The forced-split cases together reach: more splits than half the elements (empty workgroups), split boundaries inside a
    sample, planes shorter than 256 elements, B = 3 -- and every one of them is split."""
    lay = {(s, k): _split_layout(s, k) for s, k in FORCED}
    for (s, k), (ns, per, empty, inside) in lay.items():
        print(f"[forced split] {s} reduce_chunk={k}: nsplit {ns}, {per} per split, {empty} empty, boundary inside a sample: {inside}")
        assert ns > 1 and _bn_n(s) < 256 and s[0] == 3
    assert any(ns > s[0] * _bn_n(s) / 2 and empty > 0 for (s, _), (ns, _, empty, _) in lay.items())
    assert any(inside for (_, _, _, inside) in lay.values())


@pytest.mark.parametrize("shape,k", FORCED)
@pytest.mark.parametrize("relu", [False, True])
def test_forced_split_batch_norm(shape, k, relu):
    """Case 2: the same three entries at shapes where reduce_chunk = k forces splits with ragged, empty and mid-sample boundaries."""
    from effi_mvs_plus_amd import ops
    ns, per, empty, inside = _split_layout(shape, k)
    assert ns > 1
    with ops.options(reduce_chunk=k):
        _bn_check(f"forced {shape} k={k} relu={relu} nsplit={ns} empty={empty}", shape, relu, seed=k + sum(shape))


# ---- case 3: kinks and conditioning -------------------------------------------------------------------------------------------
def test_batch_norm_relu_at_a_million_elements_per_channel():
    """relu=True at 10^6 elements per channel: some y sit within rounding of 0; the fp64 backward gets the HIP forward's own ReLU mask."""
    shape = (4, 4, 500, 500)
    assert launch_shape("reduce", B=4, n=_bn_n(shape)) == 256 and 4 * _bn_n(shape) == 10 ** 6
    _bn_check(f"bn relu {shape}", shape, True, seed=3)


def test_batch_norm_variance_with_a_large_mean_offset():
    """Every channel's mean is 10^3 times its standard deviation: the centred second pass has to remove it."""
    shape = (4, 8, 128, 160)
    assert launch_shape("reduce", B=4, n=_bn_n(shape)) == 40
    _bn_check(f"bn offset 1e3 sigma {shape}", shape, False, seed=4, offset=1e3)


# ---- case 4: bitwise repeatability of the fixed-order reductions --------------------------------------------------------------------
def _twice_equal(shape, relu, seed):
    x, gy, par = _bn_inputs(shape, seed)
    a, b = _bn_hip(x, gy, par, relu), _bn_hip(x, gy, par, relu)
    for k in ("y", "mean", "invstd", "rm", "rv", "gx", "s1", "s2", "cs"):
        assert torch.equal(a[k], b[k]), f"{shape}: {k} differs between two identical calls"


def test_fixed_order_reductions_are_bitwise_repeatable(train_shapes):
    """train_ops.hip:596-598: bn_train_fwd (y, mean, invstd, running statistics), bn_bwd (gx, s1, s2) and channel_sum give identical
    bits in two calls -- at the training shape (nsplit 256) and in a forced-split case with empty splits."""
    from effi_mvs_plus_amd import ops
    shape = _pick(train_shapes, "fpn_conv0")
    assert launch_shape("reduce", B=shape[0], n=_bn_n(shape)) == 256
    _twice_equal(shape, True, 11)
    ns, _, empty, inside = _split_layout((3, 4, 5, 6, 7), 1)
    assert ns == 256 and empty > 0 and inside
    with ops.options(reduce_chunk=1):
        _twice_equal((3, 4, 5, 6, 7), True, 12)


# ---- case 5: strip-parallel weight gradients through the autograd ops at B = 4 -----------------------------------------------------
def _grads(fn, xs, want_grad, gy, dtype, dev="cpu"):
    ls = [leaf(x.to(dtype), dev) if r else x.to(dtype).to(dev) for x, r in zip(xs, want_grad)]
    out = fn(*ls)
    out.backward(gy.to(dtype).to(dev))
    return out.detach(), [l_.grad for l_, r in zip(ls, want_grad) if r]


def _wgrad_case(case, fn_hip, fn_cpu, xs, want_grad, names, gy_shape_of, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        gy = torch.randn(gy_shape_of, generator=g)
    o64, g64 = _grads(fn_cpu, xs, want_grad, gy, torch.float64)
    o32, g32 = _grads(fn_cpu, xs, want_grad, gy, torch.float32)
    oh, gh = _grads(fn_hip, xs, want_grad, gy, torch.float32, DEV)
    tab = Table(case)
    tab("forward", oh, o64, o32)
    for n_, a, b, c in zip(names, gh, g64, g32):
        tab(n_, a, b, c)
    tab.check()


# (kind, cins, cout, stride, (D,) h, w, strips expected, what the shape is for)
WGRAD = [
    ("conv2d_k1", (6,), 20, 1, (100, 253), 24, "ragged: 25300 positions over 24 strips; ca 20 not a multiple of CAB 16"),
    ("conv2d_k3", (16, 5), 12, 1, (48, 63), 2, "2 strips; two inputs (cb_off 16); ca 12 not a multiple of CAB 8"),
    ("conv2d_k5s2", (8,), 16, 2, (512, 640), 40, "the feature pyramid's conv1.0 at 640x512"),
    ("conv2d_k7", (1,), 16, 1, (512, 512), 64, "64 strips"),
    ("conv3d", (8, 8), 1, 1, (8, 64, 80), 20, "3-D stride 1; two inputs (cb_off 8); ca 1 not a multiple of CAB 4"),
    ("conv3d", (1,), 8, 1, (8, 256, 320), 64, "the 64-strip cap (na / 8192 = 80): cost_up_small.conv0 on the stage-3 volume"),
    ("conv3d", (8,), 16, 2, (48, 64, 80), 24, "3-D stride 2 on the stage-1 volume at D = 48"),
    ("conv3d", (1,), 8, (1, 2, 2), (8, 128, 160), 20, "3-D stride (1,2,2)"),
    ("deconv3d", (16,), 8, 2, (24, 32, 40), 24, "transposed, stride 2"),
    ("deconv3d", (8,), 1, (1, 2, 2), (8, 128, 160), 80, "transposed, stride (1,2,2), one output channel"),
]


@pytest.mark.parametrize("kind,cins,cout,stride,size,strips,why", WGRAD, ids=[f"{w[0]}-{w[5]}strips-{i}" for i, w in enumerate(WGRAD)])
def test_strip_parallel_weight_gradients(kind, cins, cout, stride, size, strips, why):
    """Case 5: every wgrad_nd_kernel instantiation of the step, past one strip, through the autograd ops at B = 4 (the host's batch
    loop adds four samples into one gradient): weight, bias and input gradients against fp64."""
    from effi_mvs_plus_amd import autograd as A, ops
    B = 4
    g = torch.Generator().manual_seed(sum(cins) * 31 + cout + sum(size))
    cin = sum(cins)
    s3 = (stride,) * 3 if isinstance(stride, int) else stride
    if kind.startswith("conv2d"):
        ks = {"conv2d_k1": 1, "conv2d_k3": 3, "conv2d_k5s2": 5, "conv2d_k7": 7}[kind]
        h, w = size
        W = torch.randn(cout, cin, ks, ks, generator=g) / math.sqrt(cin * ks * ks)
        xs = [torch.randn(B, c, h, w, generator=g) for c in cins]
        if kind == "conv2d_k5s2":
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            kd, ca, cb, na = 1, cout, cin, ho * wo
            fn_hip = lambda W_, x: A.conv2d_k5s2(x, W_)                                                    # noqa: E731
            fn_cpu = lambda W_, x: F.conv2d(x, W_, None, stride=2, padding=2)                               # noqa: E731
            args, want_grad, names, gshape = [W] + xs, [True, True], ["grad weight", "grad input"], (B, cout, ho, wo)
        else:
            b = torch.randn(cout, generator=g) * 0.1
            kd, ca, cb, na = 1, cout, max(cins), h * w
            act = ops.ACT_RELU if ks == 7 else ops.ACT_NONE
            f = F.relu if ks == 7 else (lambda v: v)
            fn_hip = lambda W_, b_, *x: A.conv2d(list(x), W_, b_, act)                                       # noqa: E731
            fn_cpu = lambda W_, b_, *x: f(F.conv2d(torch.cat(x, 1), W_, b_, padding=ks // 2))                # noqa: E731
            xg = ks != 7                      # the 7x7 convolution's input is the detached inverse depth (no input gradient)
            args, want_grad = [W, b] + xs, [True, True] + [xg] * len(xs)
            names = ["grad weight", "grad bias"] + ([f"grad input {i}" for i in range(len(xs))] if xg else [])
            gshape = (B, cout, h, w)
    else:
        D, h, w = size
        ks = kd = 3
        if kind == "conv3d":
            W = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(cin * 27)
            xs = [torch.randn(B, c, D, h, w, generator=g) for c in cins]
            Do, ho, wo = (D - 1) // s3[0] + 1, (h - 1) // s3[1] + 1, (w - 1) // s3[2] + 1
            ca, cb, na = cout, max(cins), Do * ho * wo
            fn_hip = lambda W_, *x: A.conv3d(list(x), W_, stride)                                             # noqa: E731
            fn_cpu = lambda W_, *x: F.conv3d(torch.cat(x, 1), W_, None, stride=s3, padding=1)                # noqa: E731
            gshape = (B, cout, Do, ho, wo)
            names = ["grad weight"] + [f"grad input {i}" for i in range(len(xs))]
        else:
            W = torch.randn(cin, cout, 3, 3, 3, generator=g) / math.sqrt(cin * 27 / 4)
            xs = [torch.randn(B, cin, D, h, w, generator=g)]
            ca, cb, na = cin, cout, D * h * w       # transposed: A = the input, B = the output gradient
            op = (s3[0] - 1, 1, 1)
            fn_hip = lambda W_, x: A.deconv3d(x, W_, stride)                                                  # noqa: E731
            fn_cpu = lambda W_, x: F.conv_transpose3d(x, W_, None, stride=s3, padding=1, output_padding=op)  # noqa: E731
            gshape = (B, cout, D * s3[0], 2 * h, 2 * w)
            names = ["grad weight", "grad input"]
        args, want_grad = [W] + xs, [True] * (1 + len(xs))
    # one launch per sample and input (cb = that input's channels; a transposed convolution's B operand is the output gradient)
    sts = {launch_shape("wgrad", ca=ca, cb=c, na=na, kd=kd, ks=ks) for c in ((cb,) if kind == "deconv3d" else cins)}
    st = max(sts)
    print(f"[wgrad {kind} cins={cins} cout={cout} stride={stride} size={size}] na {na}, strips {sorted(sts)}: {why}")
    assert sts == {strips} and st > 1
    if "ragged" in why:
        assert na % st != 0
    if "not a multiple of CAB" in why:
        assert ca % WGRAD_CAB[(kd, ks)] != 0
    if "two inputs" in why:
        assert len(cins) == 2
    _wgrad_case(f"wgrad {kind} {size} strips={st}", fn_hip, fn_cpu, args, want_grad, names, gshape, seed=cout + cin)


# ---- case 6: grid-stride loops ------------------------------------------------------------------------------------------------------
def test_batch_norm_grid_stride_loops():
    """bn_apply_kernel / bn_bwd_apply_kernel where effi_plane_grid's cap binds: 256 planes, 64 workgroups each, 80 needed."""
    shape = (4, 64, 256, 320)
    need, cap = launch_shape("plane", n=_bn_n(shape), planes=shape[0] * shape[1])
    print(f"[bn grid stride {shape}] a plane needs {need} workgroups, cap {cap}")
    assert need > cap
    _bn_check(f"bn grid stride {shape}", shape, True, seed=6)


def test_pointwise_grid_stride_loop():
    """pointwise_kernel past its 16384-workgroup cap: GRU combine and its backward, activation backward, inv_to_depth and its
    backward on a (4, 48, 256, 320) tensor."""
    from effi_mvs_plus_amd import autograd as A, ops
    shape = (4, 48, 256, 320)
    need, cap = launch_shape("pointwise", n=math.prod(shape))
    print(f"[pointwise {shape}] {math.prod(shape)} elements: {need} workgroups needed, cap {cap}")
    assert math.prod(shape) > 4194304 and need > cap
    g = torch.Generator().manual_seed(8)
    z, h, q = (torch.rand(shape, generator=g) for _ in range(3))
    q = 3 * q - 1.5
    gy = torch.randn(shape, generator=g)
    tab = Table(f"pointwise {shape}")

    def gru(z_, h_, q_):
        return (1 - z_) * h_ + z_ * torch.tanh(q_) * h_

    o64, g64 = _grads(gru, [z, h, q], [True] * 3, gy, torch.float64)
    o32, g32 = _grads(gru, [z, h, q], [True] * 3, gy, torch.float32)
    oh, gh = _grads(lambda z_, h_, q_: A._GruCombine.apply(z_, h_, A._Mul.apply(A.activation(q_, ops.ACT_TANH), h_)), [z, h, q],
                    [True] * 3, gy, torch.float32, DEV)
    tab("GRU combine", oh, o64, o32)
    for n_, a, b, c in zip(("grad z", "grad h", "grad q (tanh backward)"), gh, g64, g32):
        tab(n_, a, b, c)
    for act, f in ((ops.ACT_RELU, F.relu), (ops.ACT_SIGMOID, torch.sigmoid)):
        nm = {ops.ACT_RELU: "relu", ops.ACT_SIGMOID: "sigmoid"}[act]
        o64, (a64,) = _grads(f, [q], [True], gy, torch.float64)
        o32, (a32,) = _grads(f, [q], [True], gy, torch.float32)
        oh, (ah,) = _grads(lambda v: A.activation(v, act), [q], [True], gy, torch.float32, DEV)
        tab(f"{nm} forward", oh, o64, o32)
        tab(f"{nm} backward", ah, a64, a32)
    lo, hi = 1 / 935.0, 1 / 425.0
    inv = z * 1.4 - 0.2

    def i2d(v):
        return 1 / (lo + (hi - lo) * v).clamp(min=1e-4)

    o64, (a64,) = _grads(i2d, [inv], [True], gy, torch.float64)
    o32, (a32,) = _grads(i2d, [inv], [True], gy, torch.float32)
    oh, (ah,) = _grads(lambda v: A.inv_to_depth(v, lo, hi), [inv], [True], gy, torch.float32, DEV)
    tab("inv_to_depth", oh, o64, o32)
    tab("inv_to_depth backward", ah, a64, a32)
    tab.check()


# ---- case 7: the 5x5 / stride-2 input gradient at 640x512 and at odd sizes ------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(3, 8), (8, 16), (16, 32)])
@pytest.mark.parametrize("h,w", [(512, 640), (509, 637)])
def test_k5s2_input_gradient_at_the_training_size(cin, cout, h, w):
    """effi_conv2d_k5s2_dgrad_f32 (vector kernel) and conv2d_k5s2_dgrad_mfma (matrix cores) against fp64 conv2d_input."""
    from effi_mvs_plus_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + h)
    W = torch.randn(cout, cin, 5, 5, generator=g) / math.sqrt(cin * 25)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gy = torch.randn(cout, ho, wo, generator=g)
    want = torch.nn.grad.conv2d_input((1, cin, h, w), W.double(), gy.double()[None], stride=2, padding=2)[0]
    ref = torch.nn.grad.conv2d_input((1, cin, h, w), W, gy[None], stride=2, padding=2)[0]
    Wd, gyd = W.to(DEV), gy.to(DEV)
    print(f"[k5s2 dgrad {cin}->{cout} {h}x{w}] vector kernel: {-(-h * w // 256)} x {-(-cin // 8)} workgroups")
    tab = Table(f"k5s2 dgrad cin={cin} {h}x{w}")
    tab("vector kernel", ops.conv2d_k5s2_dgrad(gyd, Wd, h, w), want, ref)
    tab("matrix cores", ops.conv2d_k5s2_dgrad_mfma(gyd, Wd, h, w), want, ref)
    tab.check()


# ---- case 8: per-pixel backward kernels at the training maps, B = 4 -----------------------------------------------------------------
def _pixel_case(case, fn_hip, fn_cpu, xs, want_grad, names, seed, hw):
    assert hw > TPB, "the case must span more than one workgroup of per-pixel threads"
    print(f"[{case}] {hw} pixels per sample: {-(-hw // TPB)} workgroups")
    _wgrad_case(case, fn_hip, fn_cpu, xs, want_grad, names, tuple(fn_cpu(*[x.double() for x in xs]).shape), seed)


def test_volume_lookup_backward_at_256x320():
    """vol_lookup with half-resolution queries, per-pixel ranges and queries outside the range."""
    from effi_mvs_plus_amd import autograd as A
    from oracle import effi_oracle as O
    g = torch.Generator().manual_seed(21)
    B, Dp, h, w = 4, 8, 256, 320
    vol = torch.randn(B, Dp, h, w, generator=g)
    dmax = 900.0 + 30 * torch.rand(B, 1, h, w, generator=g)
    dmin = 450.0 - 20 * torch.rand(B, 1, h, w, generator=g)
    q = 400 + 600 * torch.rand(B, 5, 2 * h, 2 * w, generator=g)               # some outside [dmin, dmax]
    assert bool(((q < 430) | (q > 930)).any())

    def cpu(v, q_, lo_, hi_):
        pro = v.permute(0, 2, 3, 1).reshape(B * h * w, 1, 1, Dp)
        return O.volume_lookup_1d(pro, F.interpolate(q_.unsqueeze(1), size=[5, h, w], mode="nearest").squeeze(1), lo_, hi_)

    _pixel_case("vol_lookup 256x320", lambda v, q_, lo_, hi_: A.vol_lookup(v, q_, lo_, hi_), cpu, [vol, q, dmin, dmax],
                [True, False, False, False], ["grad volume"], 22, h * w)


def test_getcost_backward_at_256x320():
    from effi_mvs_plus_amd import autograd as A
    from oracle import effi_oracle as O
    g = torch.Generator().manual_seed(23)
    B, h, w = 4, 256, 320
    lo, hi = 1 / 935.0, 1 / 425.0
    dv = torch.linspace(lo, hi, 384).view(1, 384).repeat(B, 1)
    cur, reg = torch.randn(B, 8, h, w, generator=g), torch.randn(B, 6, h, w, generator=g)
    inv = torch.rand(B, 1, h, w, generator=g)
    itv = torch.full((B,), (hi - lo) / 384 * 4)
    gmin, gmax = torch.full((B, 1, 1, 1), 1 / hi), torch.full((B, 1, 1, 1), 1 / lo)

    def cpu(c_, r_, inv_, itv_, gmin_, gmax_):
        depth = O.disp_to_depth(inv_, gmin_, gmax_)[1]
        pro = [r_.permute(0, 2, 3, 1).reshape(B * h * w, 1, 1, 6), c_.permute(0, 2, 3, 1).reshape(B * h * w, 1, 1, 8)]
        return O.getcost(depth, pro, itv_.view(B, 1, 1, 1), 3, gmax_, gmin_, [B, h, w])

    def hip(c_, r_, inv_, itv_, gmin_, gmax_):
        return A.getcost(c_, r_, inv_, dv.to(DEV), itv_, gmin_, gmax_, 3)

    _pixel_case("getcost 256x320", hip, cpu, [cur, reg, inv, itv, gmin, gmax], [True, True, False, False, False, False],
                ["grad cur volume", "grad reg volume"], 24, h * w)


@pytest.mark.parametrize("D,h,w", [(48, 64, 80), (8, 256, 320)])
def test_soft_argmin_backward_at_the_stage_maps(D, h, w):
    from effi_mvs_plus_amd import autograd as A
    from oracle import effi_oracle as O
    g = torch.Generator().manual_seed(D + h)
    B = 4
    lo, hi = 1 / 935.0, 1 / 425.0
    logits = torch.randn(B, D, h, w, generator=g) * 2
    hyp = (1 / torch.linspace(lo, hi, D)).view(1, D).repeat(B, 1)
    _pixel_case(f"soft_argmin D={D} {h}x{w}", lambda l_, hy: A.soft_argmin(l_, hy)[0],
                lambda l_, hy: O.depth_regression(F.softmax(l_, 1), hy), [logits, hyp], [True, False], ["grad logits"], D, h * w)


@pytest.mark.parametrize("S", [2, 12])
def test_view_aggregate_backward(S):
    """S = 2 and S = EFFI_MAX_VIEWS (12)."""
    from effi_mvs_plus_amd import autograd as A
    g = torch.Generator().manual_seed(S)
    B, D, h, w = 4, 8, 64, 80
    sv, wv = torch.randn(B, S, D, h, w, generator=g), torch.rand(B, S, h, w, generator=g)

    def cpu(s_, w_):
        return (s_ * w_.unsqueeze(2)).sum(1) / (w_.sum(1, keepdim=True) + 1e-6)

    _pixel_case(f"view_aggregate S={S}", A.view_aggregate, cpu, [sv, wv], [True, True], ["grad similarity", "grad weights"], S + 1, h * w)


def test_convex_upsample_backward_to_640x512():
    from effi_mvs_plus_amd import autograd as A
    from oracle import effi_oracle as O
    g = torch.Generator().manual_seed(25)
    B, h, w = 4, 256, 320
    inv, mask = torch.rand(B, 1, h, w, generator=g), torch.randn(B, 36, h, w, generator=g)
    _pixel_case("convex_upsample 256x320 -> 512x640", A.convex_upsample, lambda i_, m_: O.upsample_depth(i_, m_, ratio=2), [inv, mask],
                [True, True], ["grad inverse depth", "grad mask"], 26, h * w)


# ---- case 9: warp backward at the training sizes -------------------------------------------------------------------------------------
def _warp_table(case, got_sim, want, ref, g_hip, g64, g32, names):
    tab = Table(case)
    tab("similarity", got_sim, want, ref, floor=2e-4)
    for n_, a, b, c in zip(names, g_hip, g64, g32):
        tab(n_, a, b, c, floor=1e-3)
    tab.check()


def test_warp_correlate_backward_stage1_at_48_hypotheses():
    """Stage-1 warp + correlation at 64x80, C = 32, D = 48, N = 3: feature gradients against fp64 autograd through the oracle."""
    from effi_mvs_plus_amd import autograd as A
    from oracle import effi_oracle as O
    C, h, w, D, N = 32, 64, 80, 48, 3
    feats = synth.smooth_features(N, C, h, w, seed=500)
    pm = synth.synth_cameras(h * 8, w * 8, N)["stage1"]
    samples = torch.linspace(425.0, 935.0, D).view(1, D, 1, 1).expand(1, D, h, w)
    G = torch.randn(N - 1, D, h, w, generator=torch.Generator().manual_seed(5))

    def cpu(dtype):
        leaves = [leaf(f.to(dtype)) for f in feats]
        P = [O.compose_projection(pm[:, v].to(dtype)) for v in range(N)]
        sims = []
        for v in range(1, N):
            warped = O.homo_warping_new(leaves[v], P[v], P[0], samples.to(dtype)).view(1, C, D, h, w)
            sims.append((warped * leaves[0].unsqueeze(2)).mean(1)[0])
        sim = torch.stack(sims)
        (sim * G.to(dtype)).sum().backward()
        return sim.detach(), [l_.grad[0] for l_ in leaves]

    s64, g64 = cpu(torch.float64)
    s32, g32 = cpu(torch.float32)
    dl = [leaf(f[0], DEV) for f in feats]
    sim = A.warp_correlate(dl[0], dl[1:], t(pm[0], DEV), t(samples[0, :, 0, 0], DEV))
    (sim * G.to(DEV)).sum().backward()
    print(f"[warp_correlate stage 1] {h}x{w}, C {C}, D {D}, N {N}")
    _warp_table("warp_correlate stage1 D=48", sim, s64, s32, [x.grad for x in dl], g64, g32, [f"grad view {v}" for v in range(N)])


@pytest.mark.parametrize("C,h,w", [(16, 128, 160), (8, 256, 320)])
def test_warp_correlate_dyn_backward_at_the_training_maps(C, h, w):
    """Stage-2 (128x160, C 16) and stage-3 (256x320, C 8) warp + correlation at D = 8, N = 3: feature and view-weight gradients."""
    from effi_mvs_plus_amd import autograd as A
    from oracle import effi_oracle as O
    D, N = 8, 3
    key, shift = ("stage2", 1) if C == 16 else ("stage3", 2)
    feats = synth.smooth_features(N, C, h, w, seed=600 + C)
    pm = synth.synth_cameras(h * {1: 4, 2: 2}[shift], w * {1: 4, 2: 2}[shift], N)[key]
    g = torch.Generator().manual_seed(7)
    cur = 500.0 + 350.0 * torch.rand(1, 1, h, w, generator=g)
    itv = torch.full((1, 1, 1, 1), (1 / 425.0 - 1 / 935.0) / 384 * 2)
    vw = torch.rand(1, N - 1, h >> shift, w >> shift, generator=g)
    gy = torch.randn(1, D, h, w, generator=g)

    def cpu(dtype):
        fc, vc = [leaf(f.to(dtype)) for f in feats], leaf(vw.to(dtype))
        vw_up = F.interpolate(vc, scale_factor=2 ** shift, mode="nearest")
        sim, _ = O.getcost_initvolume(cur.to(dtype), fc, pm.to(dtype), itv.to(dtype), vw_up, D)
        sim.backward(gy.to(dtype))
        return sim.detach()[0], [f.grad[0] for f in fc] + [vc.grad[0]]

    s64, g64 = cpu(torch.float64)
    s32, g32 = cpu(torch.float32)
    fd, vd = [leaf(f[0], DEV) for f in feats], leaf(vw[0], DEV)
    sim, _ = A.warp_correlate_dyn(fd[0], fd[1:], vd, t(pm[0], DEV), t(cur[0, 0], DEV), t(itv.reshape(1), DEV), D)
    sim.backward(gy[0].to(DEV))
    print(f"[warp_correlate_dyn {key}] {h}x{w}, C {C}, D {D}, N {N}: {-(-h * w // TPB)} workgroups of pixels")
    _warp_table(f"warp_correlate_dyn {key} {h}x{w}", sim, s64, s32, [x.grad for x in fd] + [vd.grad], g64, g32,
                [f"grad view {v}" for v in range(N)] + ["grad view weights"])


# ---- case 10: one whole step at the reference's configuration -------------------------------------------------------------------------
def test_training_step_at_batch_4_and_48_hypotheses():
    """B = 4, N = 3, ndepths 48,8,8 at 128x160 against torch autograd through the training-mode oracle, gated with the numbers of
    test_gpu_train.py::test_training_step_matches_autograd_through_the_oracle: outputs (mean abs <= 1e-3 of the depth range), loss
    (2e-3 relative), every parameter <= max(5e-2, 2 e_ref), relative L2 distance of all gradients <= 1e-3, running statistics <= 1e-4.
    The "within 1e-3" and "above 1e-2" counts are printed, not gated (their thresholds were measured at B <= 2 with 8,8,8)."""
    from effi_mvs_plus_amd.models import mvs_loss
    H, W, B, N, nd = 128, 160, 4, 3, (48, 8, 8)
    net, sd = build_model("48,8,8", seed=13, device=DEV)
    net.train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    samples = [synth.synth_sample(H, W, N, seed=70 + b) for b in range(B)]
    imgs = torch.cat([s[0] for s in samples])
    pm = {k: torch.cat([s[1][k] for s in samples]) for k in samples[0][1]}
    dv = torch.cat([s[2] for s in samples])
    gt, mask = _loss_inputs(H, W, B, 3)
    want_out, want_loss, leaves32, sd2 = _oracle_training_pass(net, sd, imgs, pm, dv, gt, mask, nd)
    _, _, leaves64, _ = _oracle_training_pass(net, sd, imgs, pm, dv, gt, mask, nd, dtype=torch.float64)
    out = net(imgs.to(DEV), {k: v.to(DEV) for k, v in pm.items()}, dv.to(DEV))
    loss, _ = mvs_loss(out["depth"], {k: v.to(DEV) for k, v in gt.items()}, {k: v.to(DEV) for k, v in mask.items()}, DLOSS)
    loss.backward()
    assert len(out["depth"]) == 13
    rng = synth.DEPTH_MAX_MM - synth.DEPTH_MIN_MM
    for i, (a, b) in enumerate(zip(out["depth"], want_out["depth"])):
        assert tuple(a.shape) == tuple(b.shape)
        assert float((a.detach().cpu() - b.detach()).abs().mean()) / rng <= 1e-3, i
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 2e-3 * abs(float(want_loss.detach()))
    n = n_plain = n_plain_ref = n_above = 0
    num = den = 0.0
    failures = []
    for k, p_ in net.named_parameters():
        assert p_.grad is not None, f"{k}: no gradient"
        e_hip = rel(p_.grad, leaves64[k].grad)
        e_ref = rel(leaves32[k].grad, leaves64[k].grad)
        bound = max(5e-2, 2 * e_ref)
        n += 1
        n_plain += e_hip <= 1e-3
        n_plain_ref += e_ref <= 1e-3
        n_above += e_hip > 1e-2
        if e_hip > 1e-3:
            print(f"    above 1e-3: {k:55s} {e_hip:.2e}   (reference fp32 vs fp64: {e_ref:.2e})")
        num += float((p_.grad.detach().double().cpu() - leaves64[k].grad).pow(2).sum())
        den += float(leaves64[k].grad.pow(2).sum())
        if e_hip > bound:
            failures.append(f"{k}: gradient off by {e_hip:.3e} of its peak (bound {bound:.3e}; reference fp32 vs fp64: {e_ref:.3e})")
    l2 = math.sqrt(num / den)
    print(f"[training step | B={B} N={N} 48,8,8] {n} parameters, loss {float(loss.detach()):.4f} vs {float(want_loss.detach()):.4f}; "
          f"within 1e-3 of their peak: {n_plain} (the reference's own fp32 gradient: {n_plain_ref}); above 1e-2: {n_above}; "
          f"relative L2 distance of all gradients {l2:.3e}")
    assert not failures, "; ".join(failures)
    assert n > 200 and l2 <= 1e-3
    for k, v in net.state_dict().items():
        if "running_" in k:
            assert rel(v, sd2[k]) <= 1e-4, k
        if "num_batches_tracked" in k:
            assert int(v) == int(sd2[k]), k
