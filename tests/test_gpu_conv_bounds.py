"""GPU: every forward convolution entry, through the C ABI, on impulse inputs (tests/conv_bound.py).

Each case builds its impulse family (tests/conv_cases.py: isolated non-zero pixels, every input channel in every position class --
corners, borders, interior, the last pixel before and the first after every tile seam of the kernel under test), runs the product's
own wrapper or module on each member with an ``ops.KernelProfile`` installed and asserts the recorded launch key (a case that falls
back to another kernel fails instead of testing the wrong thing), then ``check_bounded``: EVERY element inside its float64 interval
-- a few 2^-16 (split) or a few 2^-24 (fp32) of the ONE product behind it -- and bit-exact where the interval is a point (0 where no
impulse reaches and the bias is 0, the activation of the fp32 bias otherwise).  Nothing is left out.  The table of DESIGN.md section
2.2 is what the module's last lines print (run with -s)."""
import pytest
import torch

import conv_bound as CB
import conv_cases as CC
from common import t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TABLE = {}          # row of the recorded table -> [checks, largest share used, pinned elements, elements]


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\n[bound-table] family | checks | largest share of the interval used | exactly pinned elements | elements")
    for row, (n, used, pinned, total) in TABLE.items():
        print(f"[bound-table] {row} | {n} | {used:.3f} | {pinned} | {total}")


class precision_:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from effi_mvs_plus_amd import ops
        self.before = ops.get_precision()
        ops.set_precision(self.mode)

    def __exit__(self, *exc):
        from effi_mvs_plus_amd import ops
        ops.set_precision(self.before)
        return False


def launch(expect, fn):
    """fn() under a KernelProfile that brackets every launch; the recorded keys must be exactly ``expect`` (a key or a list)."""
    from effi_mvs_plus_amd import ops
    prof, before = ops.KernelProfile(keys=None), ops.get_profile()
    ops.set_profile(prof)
    try:
        out = fn()
    finally:
        ops.set_profile(before)
    keys = [r[0] for r in prof.records if r[2] is not None]
    expect = [expect] if isinstance(expect, str) else list(expect)
    assert keys == expect, f"launched {keys}, the case is written for {expect}"
    return out


def bounded(row, name, got, iv, x=None, w_shape=None, stride=1, padding=1, dims=2):
    """check_bounded + the table row; a failure names the (co, ci, tap, input position) of the product behind the worst element."""
    try:
        rep = CB.check_bounded(name, got, iv.mid, iv.half, k_eff=iv.k_eff, quiet=True)
    except CB.OutOfBound as e:
        where = ""
        if x is not None and e.index is not None:
            where = f"; product behind it: {CB.locate(e.index, w_shape, x, stride, padding, dims)}"
        raise CB.OutOfBound(str(e) + where, e.index) from None
    r = TABLE.setdefault(row, [0, 0.0, 0, 0])
    r[0] += 1
    r[1] = max(r[1], rep["used"])
    r[2] += rep["pinned"]
    r[3] += rep["checked"]
    return rep


def dev_srcs(fam, x):
    return [t(s, DEV) for s in fam.sources(x)]


ACTS = ["none", "relu", "sigmoid", "tanh"]


# ---------------------------------------------------------------------------------------------
# split 3x3: conv2d_k3_bf16x3
# ---------------------------------------------------------------------------------------------
SPLIT_EPIS = [("plain", 1), ("plain", 0), ("nhwc", 0), ("plain", 2), ("plain", 3)]
# the cases that run in "bf16" precision (hi * hi only, its own C_MODE): (5,) -> 7 tanh, (24, 8, 12) -> 20 ReLU, (48,) -> 48 NHWC
SPLIT_BF16 = (4, 15, 17)
assert all(i < len(CC.split_cases()) for i in SPLIT_BF16)


def finer(mode):
    """The bf16 entries share their launch keys with the split ones, and the 7x7 wrapper records none: there the arithmetic that ran is
    pinned by the result itself.  A bf16 product is off by up to 2^-8 of itself (typically 2^-10), a split one by up to 3 * 2^-16
    (typically 2^-17), so over a family -- hundreds of products of full-significand operands -- a bf16 run must leave the split
    interval somewhere and a split run the fp32 one (3u = 2^-22.4); a run that never does took the finer arithmetic's kernel."""
    return {"bf16": "split", "split": "fp32"}[mode]


@pytest.mark.parametrize("idx", range(len(CC.split_cases())))
def test_split_3x3_every_element_bounded(idx):
    """Seams: x 16-pixel segments; y the wave's row group (MR rows, forced with ``force_mr``) and the workgroup's 4 MR rows."""
    from effi_mvs_plus_amd import ops, packing
    cins, cout, (h, w), mr = CC.split_cases()[idx]
    fam = CC.split_family(cins, (h, w), mr)
    fam.assert_full()
    (epi, act), mode = SPLIT_EPIS[idx % len(SPLIT_EPIS)], ("bf16" if idx in SPLIT_BF16 else "split")
    wt, b = CC.weights(cout, sum(cins), 3, seed=1000 + idx, bias=idx % 2)
    wp, bp = packing.pack_conv2d_bf16x3(wt.to(DEV), None if b is None else b.to(DEV))
    epilogue = ops.EPI_NHWC if epi == "nhwc" else ops.EPI_PLAIN
    key = f"conv2d_k3x3_nt{(cout + 15) // 16}_epi{epilogue}"
    row = f"split 3x3 {epi} act={ACTS[act]} ({mode})"
    left_finer = False
    with precision_(mode), ops.options(force_mr=mr):
        assert ops.launch_form("x3", h, w, nt=(cout + 15) // 16).rows == mr
        for k, x in enumerate(fam.members):
            got = launch(key, lambda: ops.conv2d_k3_bf16x3(dev_srcs(fam, x), wp, bp, cout, epilogue=epilogue, act=act))
            if epi == "nhwc":
                got = got.permute(2, 0, 1)
            iv = CB.conv_interval(x, None, wt, b, mode=mode)
            assert int(iv.k_eff.max()) == 1
            a = CB.act_interval(*iv, ACTS[act], "exact")
            a.k_eff = iv.k_eff
            bounded(row, f"split 3x3 {cins}->{cout} {h}x{w} mr={mr} {epi} act={act} member {k}", got, a, x, wt.shape)
            if mode == "bf16":
                left_finer |= CB.escapes(got, *CB.act_interval(*iv.remode(finer(mode)), ACTS[act], "exact"))
    assert mode != "bf16" or left_finer, "the bf16 case stayed inside the split interval everywhere: the split kernel ran"


@pytest.mark.parametrize("cins,cout,hw,mr,q,bias", CC.SPLIT_GRU)
def test_split_3x3_gru_epilogues_bounded(cins, cout, hw, mr, q, bias):
    """GRU_ZR (z = sigmoid, r * h) and GRU_Q ((1 - z) h + z tanh) on dense auxiliary maps: the split forms of the gates (2e-7)."""
    from effi_mvs_plus_amd import ops, packing
    h, w = hw
    fam = CC.split_family(cins, hw, mr)
    wt, b = CC.weights(cout, sum(cins), 3, seed=77 + cout + int(q), bias=bias)
    wp, bp = packing.pack_conv2d_bf16x3(wt.to(DEV), None if b is None else b.to(DEV))
    g = torch.Generator().manual_seed(cout)
    hd = cout if q else cout // 2
    hprev, z = torch.tanh(torch.randn(hd, h, w, generator=g)), torch.rand(hd, h, w, generator=g)
    hp_d, z_d = t(hprev, DEV), t(z, DEV)
    nt = (cout + 15) // 16
    with precision_("split"), ops.options(force_mr=mr):
        assert ops.launch_form("x3", h, w, nt=nt).rows == mr
        for k, x in enumerate(fam.members):
            iv = CB.conv_interval(x, None, wt, b, mode="split")
            if q:
                got = launch(f"conv2d_k3x3_nt{nt}_epi{ops.EPI_GRU_Q}",
                             lambda: ops.conv2d_k3_bf16x3(dev_srcs(fam, x), wp, bp, cout, epilogue=ops.EPI_GRU_Q, aux0=hp_d, aux1=z_d))
                bounded("split 3x3 GRU_Q", f"GRU_Q {cins}->{cout} member {k}", got, CB.act_interval(*iv, "gru_q", "split", h=hprev, z=z))
            else:
                gz, grh = launch(f"conv2d_k3x3_nt{nt}_epi{ops.EPI_GRU_ZR}",
                                 lambda: ops.conv2d_k3_bf16x3(dev_srcs(fam, x), wp, bp, cout, epilogue=ops.EPI_GRU_ZR, aux0=hp_d))
                bounded("split 3x3 GRU_ZR", f"GRU z {cins}->{cout} member {k}", gz, CB.act_interval(iv.mid[:hd], iv.half[:hd], "gru_z", "split"))
                bounded("split 3x3 GRU_ZR", f"GRU r*h {cins}->{cout} member {k}", grh,
                        CB.act_interval(iv.mid[hd:], iv.half[hd:], "gru_rh", "split", h=hprev))


def test_split_3x3_family_as_one_batch():
    """The batched twin on a whole family at once: image i is bounded like the single launch on member i."""
    from effi_mvs_plus_amd import ops, packing
    cins, cout, hw = (16,), 16, (21, 28)
    fam = CC.split_family(cins, hw, 1)
    wt, b = CC.weights(cout, 16, 3, seed=5, bias=True)
    wp, bp = packing.pack_conv2d_bf16x3(wt.to(DEV), b.to(DEV))
    xb = t(torch.stack(fam.members), DEV)
    with precision_("split"):
        got = launch(f"conv2d_k3x3_nt1_epi{ops.EPI_PLAIN}_batch", lambda: ops.conv2d_k3_bf16x3([xb], wp, bp, cout, act=ops.ACT_RELU))
    for k, x in enumerate(fam.members):
        iv = CB.conv_interval(x, None, wt, b, mode="split")
        bounded("split 3x3, family as one batch", f"batch member {k}", got[k], CB.act_interval(*iv, "relu"), x, wt.shape)


# ---------------------------------------------------------------------------------------------
# generic fp32 MFMA conv2d
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", CC.GENERIC_SHAPES)
@pytest.mark.parametrize("idx", range(len(CC.GENERIC)))
def test_generic_fp32_conv2d_bounded(idx, hw):
    """16 x 16 pixel tiles; w = 30 takes the scalar stores, w = 28 the vector stores.  Exact fp32 arithmetic: a few u of the product."""
    from effi_mvs_plus_amd import ops, packing
    ks, cins, cout, act = CC.GENERIC[idx]
    fam = CC.family(cins, hw, ks // 2, CC.fam_key(CC.GENERIC_TILES), seed=ks + sum(cins))
    fam.assert_full()
    wt, b = CC.weights(cout, sum(cins), ks, seed=2000 + idx, bias=(idx + hw[1]) % 2)
    wp, bp = packing.pack_conv2d_mfma(wt.to(DEV), None if b is None else b.to(DEV))
    key = f"conv2d_k{ks}_nt{(cout + 15) // 16}_epi{ops.EPI_PLAIN}"
    for k, x in enumerate(fam.members):
        got = launch(key, lambda: ops.conv2d(dev_srcs(fam, x), wp, bp, cout, ks, act=act))
        iv = CB.conv_interval(x, None, wt, b, 1, ks // 2, None, "fp32")
        a = CB.act_interval(*iv, ACTS[act], "exact")
        a.k_eff = iv.k_eff
        bounded(f"generic fp32 conv2d k{ks}", f"conv2d k{ks} {cins}->{cout} {hw} act={act} member {k}", got, a, x, wt.shape, 1, ks // 2)


# ---------------------------------------------------------------------------------------------
# split-resident forms
# ---------------------------------------------------------------------------------------------
def sr_value(m):
    hi, lo = m.parts()
    return hi + lo


def widen_sr(iv):
    """An output read back from a split-resident map is hi + lo of the fp32 value: 2^-16 of it more (C_MODE's derivation)."""
    return CB.Interval(iv.mid, iv.half + 2.0 ** -16 * (iv.mid.abs() + iv.half), iv.k_eff)           # still a point where the value is 0


@pytest.mark.parametrize("cins,cout,hw,bias", [((16,), 32, (37, 52), 0), ((16, 16), 32, (37, 52), 1), ((16, 16), 32, (21, 40), 1),
                                               ((32,), 32, (21, 40), 0)])
def test_split_resident_3x3_bounded(cins, cout, hw, bias):
    """conv2d_k3_sr PLAIN / GRU_ZR / GRU_Q (planar and q4 auxiliaries) and conv2d_k3_pair_sr on maps made by sr_from_planar."""
    from effi_mvs_plus_amd import ops, packing
    h, w = hw
    fam = CC.fused_family("sr", cins, hw)
    fam.assert_full()
    nt = (cout + 15) // 16
    wt, b = CC.weights(cout, sum(cins), 3, seed=300 + cout + h, bias=bias)
    wp, bp = packing.pack_conv2d_bf16x3(wt.to(DEV), None if b is None else b.to(DEV))
    g = torch.Generator().manual_seed(h)
    hq, zq = torch.tanh(torch.randn(cout, h, w, generator=g)), torch.rand(cout, h, w, generator=g)
    hz = hq[:cout // 2].contiguous()
    with precision_("split"):
        for k, x in enumerate(fam.members):
            srcs = [ops.sr_from_planar(s) for s in dev_srcs(fam, x)]
            iv = CB.conv_interval(x, None, wt, b, mode="split")
            # PLAIN: fp32 output and the split-resident one
            out0, out_sr = launch(f"conv2d_k3x3_nt{nt}_epi0", lambda: ops.conv2d_k3_sr(
                srcs, wp, bp, cout, act=ops.ACT_RELU, out0=torch.empty(cout, h, w, device=DEV)))
            a = CB.act_interval(*iv, "relu")
            bounded("split-resident 3x3 PLAIN", f"sr plain {cins}->{cout} member {k}", out0, a, x, wt.shape)
            bounded("split-resident 3x3 PLAIN", f"sr plain (SR map) member {k}", sr_value(out_sr), widen_sr(a), x, wt.shape)
            # pair: the same convolution twice, SR in, SR out
            oa, ob = ops.sr_alloc(2, cout, h, w, DEV)
            launch(f"conv2d_k3x3_pair_nt{nt}", lambda: ops.conv2d_k3_pair_sr(srcs, wp, bp, oa, srcs, wp, bp, ob, cout, act=ops.ACT_RELU))
            bounded("conv2d_k3_pair_sr", f"sr pair a member {k}", sr_value(oa), widen_sr(a), x, wt.shape)
            bounded("conv2d_k3_pair_sr", f"sr pair b member {k}", sr_value(ob), widen_sr(a), x, wt.shape)
            for q4 in (False, True):
                lay = (lambda v: ops.q4_from_planar(t(v, DEV))) if q4 else (lambda v: t(v, DEV))
                back = (lambda v, c: ops.q4_to_planar(v.view(c // 4, h, w, 4), c)) if q4 else (lambda v, c: v)
                z, rh = launch(f"conv2d_k3x3_nt{nt}_epi{ops.EPI_GRU_ZR}",
                               lambda: ops.conv2d_k3_sr(srcs, wp, bp, cout, epilogue=ops.EPI_GRU_ZR, aux0=lay(hz), q4=q4))
                hd = cout // 2
                bounded("split-resident 3x3 GRU_ZR", f"sr z q4={q4} member {k}", back(z, hd),
                        CB.act_interval(iv.mid[:hd], iv.half[:hd], "gru_z", "split"))
                bounded("split-resident 3x3 GRU_ZR", f"sr r*h q4={q4} member {k}", sr_value(rh),
                        widen_sr(CB.act_interval(iv.mid[hd:], iv.half[hd:], "gru_rh", "split", h=hz)))
                hn, _ = launch(f"conv2d_k3x3_nt{nt}_epi{ops.EPI_GRU_Q}",
                               lambda: ops.conv2d_k3_sr(srcs, wp, bp, cout, epilogue=ops.EPI_GRU_Q, aux0=lay(hq), aux1=lay(zq), q4=q4))
                bounded("split-resident 3x3 GRU_Q", f"sr q q4={q4} member {k}", back(hn, cout),
                        CB.act_interval(*iv, "gru_q", "split", h=hq, z=zq))


# ---------------------------------------------------------------------------------------------
# fused and special 2-D forms
# ---------------------------------------------------------------------------------------------
def chain(first, w2, b2, mode="split", **kw):
    """Second stage of a fused pair: the first stage's values as the kernel holds them (fp32) and its half-width as ``ex``."""
    mid32 = first.mid.float()
    return CB.conv_interval(mid32, first.half + (first.mid - mid32.double()).abs(), w2, b2, mode=mode, **kw)


@pytest.mark.parametrize("cins,hw,cout1,c_extra,cout2,relu1,bias", [
    ((16, 16), (21, 28), 12, 4, 16, False, 1), ((16,), (21, 28), 16, 0, 16, False, 0), ((8, 8), (37, 52), 5, 3, 32, False, 1),
    ((16,), (21, 28), 32, 0, 36, True, 1)])
def test_3x3_then_1x1_bounded(cins, hw, cout1, c_extra, cout2, relu1, bias):
    """conv2d_k3_k1_x3: the encoder pair (ReLU after the 1x1, with and without extra channels) and the mask head (ReLU between)."""
    from effi_mvs_plus_amd import ops, packing
    h, w = hw
    fam = CC.fused_family("k3k1", cins, hw)
    fam.assert_full()
    extras = CC.fused_family("extra", (c_extra,), hw).members if c_extra else None
    w1, b1 = CC.weights(cout1, sum(cins), 3, seed=400 + cout1, bias=bias)
    w2, b2 = CC.weights(cout2, cout1 + c_extra, 1, seed=500 + cout2, bias=bias)
    wx, bx = packing.pack_conv2d_bf16x3(w1.to(DEV), None if b1 is None else b1.to(DEV))
    w2p, b2p = packing.pack_conv1x1_after(w2.to(DEV), None if b2 is None else b2.to(DEV), cout1, c_extra)
    with precision_("split"):
        for k, x in enumerate(fam.members):
            extra = extras[k % len(extras)] if c_extra else None
            got = launch(f"conv2d_k3k1_nt{(cout1 + 15) // 16}", lambda: ops.conv2d_k3_k1_x3(
                dev_srcs(fam, x), wx, bx, cout1, None if extra is None else t(extra, DEV), w2p, b2p, cout2, relu=not relu1, relu1=relu1))
            i1 = CB.conv_interval(x, None, w1, b1, mode="split")
            if relu1:
                i1 = CB.act_interval(*i1, "relu")
            mid = i1.mid if extra is None else torch.cat([i1.mid, extra.double()])
            half = i1.half if extra is None else torch.cat([i1.half, torch.zeros_like(extra, dtype=torch.float64)])
            i2 = chain(CB.Interval(mid, half), w2, b2, padding=0)
            if not relu1:
                i2 = CB.act_interval(*i2, "relu")
            bounded("conv2d_k3_k1_x3", f"3x3+1x1 {cins}->{cout1}(+{c_extra})->{cout2} member {k}", got, i2)
            if all(c % 16 == 0 for c in cins):                       # the same pair reading split-resident maps
                srs = [ops.sr_from_planar(s) for s in dev_srcs(fam, x)]
                got = launch(f"conv2d_k3k1_nt{(cout1 + 15) // 16}", lambda: ops.conv2d_k3_k1_sr(
                    srs, wx, bx, cout1, None if extra is None else t(extra, DEV), w2p, b2p, cout2, relu=not relu1, relu1=relu1))
                bounded("conv2d_k3_k1_sr", f"3x3+1x1 (SR) {cins}->{cout1}(+{c_extra})->{cout2} member {k}", got, i2)


@pytest.mark.parametrize("cin,cmid,cout,hw,bias", [(3, 8, 8, (21, 28), 1), (8, 8, 8, (37, 52), 0), (5, 8, 6, (12, 16), 1), (3, 4, 4, (21, 28), 0)])
def test_3x3_twice_bounded(cin, cmid, cout, hw, bias):
    from effi_mvs_plus_amd import ops, packing
    fam = CC.fused_family("twice", (cin,), hw)
    fam.assert_full()
    w1, b1 = CC.weights(cmid, cin, 3, seed=600 + cin, bias=bias)
    w2, b2 = CC.weights(cout, cmid, 3, seed=700 + cout, bias=bias)
    p1, pb1 = packing.pack_conv2d_bf16x3_oct(w1.to(DEV), None if b1 is None else b1.to(DEV))
    p2, pb2 = packing.pack_conv2d_bf16x3_oct(w2.to(DEV), None if b2 is None else b2.to(DEV))
    with precision_("split"):
        for k, x in enumerate(fam.members):
            got = launch("conv2d_k3_twice", lambda: ops.conv2d_k3_twice(t(x, DEV), p1, pb1, p2, pb2, cout))
            i1 = CB.act_interval(*CB.conv_interval(x, None, w1, b1, mode="split"), "relu")
            bounded("conv2d_k3_twice", f"3x3 twice {cin}->{cmid}->{cout} {hw} member {k}", got, CB.act_interval(*chain(i1, w2, b2), "relu"))


@pytest.mark.parametrize("cd,hw,bias", [(4, (21, 28), 1), (8, (37, 52), 0)])
def test_encoder_tail_bounded(cd, hw, bias):
    """relu(convc2(cor1)) | relu(convd2(dfm1)) -> convd -> 1x1 convc over cat(., ctx) -> ReLU: three chained intervals."""
    from effi_mvs_plus_amd import ops, packing
    hd, cmix = 16, 16 - cd
    fam = CC.fused_family("tail", (hd, hd), hw)
    fam.assert_full()
    ctxs = CC.fused_family("ctx", (cd,), hw).members
    (wc2, bc2), (wd2, bd2) = CC.weights(hd, hd, 3, seed=801, bias=bias), CC.weights(hd, hd, 3, seed=802, bias=bias)
    (wd, bd), (wc, bc) = CC.weights(cmix, 2 * hd, 3, seed=803, bias=bias), CC.weights(hd, hd, 1, seed=804, bias=bias)
    d = lambda v: None if v is None else v.to(DEV)       # noqa: E731
    pc2, pbc2 = packing.pack_conv2d_bf16x3(d(wc2), d(bc2))
    pd2, pbd2 = packing.pack_conv2d_bf16x3(d(wd2), d(bd2))
    pd, pbd = packing.pack_conv2d_bf16x3(d(wd), d(bd))
    p2, pb2 = packing.pack_conv1x1_after(d(wc), d(bc), cmix, cd)
    with precision_("split"):
        for k, x in enumerate(fam.members):
            ctx = ctxs[k % len(ctxs)]
            cor1, dfm1 = fam.sources(x)
            got = launch("encoder_tail", lambda: ops.encoder_tail(t(cor1, DEV), t(dfm1, DEV), pc2, pbc2, pd2, pbd2, pd, pbd, cmix, t(ctx, DEV),
                                                                  p2, pb2, hd))
            a = CB.act_interval(*CB.conv_interval(cor1, None, wc2, bc2, mode="split"), "relu")
            b_ = CB.act_interval(*CB.conv_interval(dfm1, None, wd2, bd2, mode="split"), "relu")
            i2 = chain(CB.Interval(torch.cat([a.mid, b_.mid]), torch.cat([a.half, b_.half])), wd, bd)
            i3 = chain(CB.Interval(torch.cat([i2.mid, ctx.double()]), torch.cat([i2.half, torch.zeros_like(ctx, dtype=torch.float64)])),
                       wc, bc, padding=0)
            bounded("encoder_tail", f"encoder tail cd={cd} {hw} member {k}", got, CB.act_interval(*i3, "relu"))


@pytest.mark.parametrize("mode", ["fp32", "split"])
@pytest.mark.parametrize("cin,cout,hw,bias", [(3, 24, (21, 28), 1), (8, 16, (37, 52), 0), (32, 64, (20, 36), 1), (8, 16, (12, 20), 0)])
def test_5x5_stride2_bounded(cin, cout, hw, bias, mode):
    """Odd and even input sizes, impulses on both column / row parities; both arithmetics of the one wrapper."""
    from effi_mvs_plus_amd import ops, packing
    fam = CC.fused_family("k5s2", (cin,), hw)
    fam.assert_full()
    wt, b = CC.weights(cout, cin, 5, seed=900 + cin, bias=bias)
    wp, bp = packing.pack_conv2d(wt.to(DEV), None if b is None else b.to(DEV))
    key = f"conv2d_k5s2{'x3' if mode == 'split' else ''}_nt{(cout + 15) // 16}"
    with precision_(mode):
        for k, x in enumerate(fam.members):
            got = launch(key, lambda: ops.conv2d_k5s2(t(x, DEV), wp, bp, cout, act=ops.ACT_RELU))
            iv = CB.conv_interval(x, None, wt, b, 2, 2, None, mode)
            bounded(f"conv2d_k5s2 ({mode})", f"5x5 s2 {cin}->{cout} {hw} member {k}", got, CB.act_interval(*iv, "relu"), x, wt.shape, 2, 2)


@pytest.mark.parametrize("mode", ["fp32", "split"])
@pytest.mark.parametrize("cout,hw", [(16, (21, 28)), (48, (37, 52))])
def test_7x7_single_channel_bounded(cout, hw, mode):
    """conv2d_c1k7_relu: 32 x 8 pixel tiles (fp32 vector kernel); in split precision the same tile as 16-pixel segments with two rows
    per wave; reach 3.  The wrapper records no launch key, so the split run must leave the fp32 interval somewhere (``finer``)."""
    from effi_mvs_plus_amd import ops, packing
    fam = CC.fused_family("c1k7", (1,), hw)
    fam.assert_full()
    wt, b = CC.weights(cout, 1, 7, seed=950 + cout, bias=True)
    wp, bp = packing.pack_conv2d_c1k7(wt.to(DEV), b.to(DEV))
    left_finer = False
    with precision_(mode):
        for k, x in enumerate(fam.members):
            got = launch([], lambda: ops.conv2d_c1k7_relu(t(x, DEV), wp, bp, cout))
            iv = CB.conv_interval(x, None, wt, b, 1, 3, None, mode)
            bounded(f"conv2d_c1k7_relu ({mode})", f"7x7 1->{cout} {hw} member {k}", got, CB.act_interval(*iv, "relu"), x, wt.shape, 1, 3)
            if mode == "split":
                left_finer |= CB.escapes(got, *CB.act_interval(*iv.remode("fp32"), "relu"))
    assert mode != "split" or left_finer, "the split run stayed inside the fp32 interval everywhere: the fp32 kernel ran"


@pytest.mark.parametrize("hd,hw,bias", [(16, (37, 52), 1), (32, (29, 16), 0)])
def test_one_launch_conv_gru_bounded(hd, hw, bias):
    """gru_zr_q_fused_sr: z | r = sigmoid(conv([h, x])), q = tanh(conv([r * h, x])), h' = (1 - z) h + z q with r * h and z on chip.  The
    state h and the input x are impulses (r * h is then as sparse as h), so both convolutions see at most one product per element."""
    from effi_mvs_plus_amd import ops, packing
    h, w = hw
    fam = CC.fused_family("gru", (hd, hd), hw)
    fam.assert_full()
    wzr, bzr = CC.weights(2 * hd, 2 * hd, 3, seed=1100 + hd, bias=bias)
    wq, bq = CC.weights(hd, 2 * hd, 3, seed=1200 + hd, bias=bias)
    d = lambda v: None if v is None else v.to(DEV)       # noqa: E731
    pzr, pbzr = packing.pack_conv2d_bf16x3(d(wzr), d(bzr))
    pq, pbq = packing.pack_conv2d_bf16x3(d(wq), d(bq))
    with precision_("split"):
        for k, xm in enumerate(fam.members):
            hs, xs = fam.sources(xm)
            Hm, Xm, Ho = ops.sr_from_planar(t(hs, DEV)), ops.sr_from_planar(t(xs, DEV)), ops.sr_alloc(1, hd, h, w, DEV)[0]
            h_out, _ = launch(f"gru_fused_nt{hd // 16}", lambda: ops.gru_zr_q_fused_sr(
                Hm, Xm, t(hs, DEV), pzr, pbzr, pq, pbq, torch.empty(hd, h, w, device=DEV), Ho))
            izr = CB.conv_interval(xm, None, wzr, bzr, mode="split")
            iz = CB.act_interval(izr.mid[:hd], izr.half[:hd], "gru_z", "split")
            irh = CB.act_interval(izr.mid[hd:], izr.half[hd:], "gru_rh", "split", h=hs)
            zero = torch.zeros_like(xs, dtype=torch.float64)
            iq = chain(CB.Interval(torch.cat([irh.mid, xs.double()]), torch.cat([torch.where(hs != 0, irh.half, zero), zero])), wq, bq)
            inew = CB.act_interval(*iq, "gru_q", "split", h=hs, z=iz.mid, z_half=iz.half)
            bounded("gru_zr_q_fused_sr", f"one-launch ConvGRU hd={hd} {hw} member {k}", h_out, inew)
            bounded("gru_zr_q_fused_sr", f"one-launch ConvGRU (SR state) hd={hd} member {k}", sr_value(Ho), widen_sr(inew))


@pytest.mark.parametrize("hd,hw", [(16, (37, 52)), (32, (21, 28))])
def test_depth_head_tap_projections_bounded(hd, hw):
    """The depth head as tap projections: conv1 + ReLU + the nine 1x1 projections of conv2 (conv2d_k3_k1_x3 / conv2d_k3_k1_sr with
    packing.pack_head_taps) -- the linear part, bounded plane by plane -- then head_update and the one-launch depth_head_sr (tiles 2, 4,
    8), whose inverse depth inv + tanh(sum of the shifted planes + bias) is carried through the same algebra (its depth output is the
    existing tests')."""
    from effi_mvs_plus_amd import ops, packing
    h, w = hw
    fam = CC.fused_family("head", (hd,), hw)
    fam.assert_full()
    w1, b1 = CC.weights(hd, hd, 3, seed=1300 + hd, bias=True)
    w2, b2 = CC.weights(1, hd, 3, seed=1400 + hd, bias=True)
    g = torch.Generator().manual_seed(hd)
    inv = torch.rand(1, h, w, generator=g)
    dv = t(torch.linspace(1 / 935.0, 1 / 425.0, 384), DEV)
    p1, pb1 = packing.pack_conv2d_bf16x3(w1.to(DEV), b1.to(DEV))
    p2, pb2 = packing.pack_head_taps(w2.to(DEV), hd)
    taps = w2[0].reshape(hd, 9).t().reshape(9, hd, 1, 1)
    nt = (hd + 15) // 16
    with precision_("split"):
        for k, x in enumerate(fam.members):
            i1 = CB.act_interval(*CB.conv_interval(x, None, w1, b1, mode="split"), "relu")
            ip = chain(i1, taps, None, padding=0)
            part = launch(f"conv2d_k3k1_nt{nt}", lambda: ops.conv2d_k3_k1_x3([t(x, DEV)], p1, pb1, hd, None, p2, pb2, 9, relu=False, relu1=True))
            bounded("depth head, nine tap projections", f"head taps hd={hd} member {k}", part, ip)
            sr = ops.sr_from_planar(t(x, DEV))
            part_sr = launch(f"conv2d_k3k1_nt{nt}", lambda: ops.conv2d_k3_k1_sr([sr], p1, pb1, hd, None, p2, pb2, 9, relu=False, relu1=True))
            bounded("depth head, nine tap projections", f"head taps (SR) hd={hd} member {k}", part_sr, ip)
            # the 3x3 sum of the planes + bias (nine more additions), tanh (tanhf), + inv
            isum = chain(i1, w2, b2, n_epi=10)
            iinv = CB.act_interval(*CB.act_interval(*isum, "tanh", "exact"), "add", add=inv)
            inv_new, _ = launch("head_update", lambda: ops.head_update(part, b2.to(DEV), t(inv, DEV), dv))
            bounded("head_update", f"head update hd={hd} member {k}", inv_new, iinv)
            for tile in (2, 4, 8):
                oi, _ = launch(f"depth_head_nt{nt}", lambda: ops.depth_head_sr([sr], p1, pb1, hd, p2, pb2, b2.to(DEV), t(inv, DEV), dv, tile))
                bounded("depth_head_sr", f"one-launch depth head hd={hd} tile={tile} member {k}", oi, iinv)


def _fpn_interval(top, l1, w_out, w_in, b_in):
    """conv3x3_W(up2(top) + inner(l1)) in float64 and its half-width.  packing.pack_fpn_head_split composes the weights in fp64 and
    rounds once (u per composed weight: one more rounding per product than ACC), the two launches are split 3x3 convolutions
    (C_MODE["split"] of sum |W| (up2 |top| + |W_in| |l1| + |b_in|), which bounds the merged taps' products too), and the epilogue adds
    the pixel-shuffled coarse result (one rounding).  K_eff counts the non-zero terms of that sum (an upper bound on the kernels'
    products: merged taps are fewer), so it is 0 exactly where nothing reaches."""
    up = lambda v: v.repeat_interleave(2, -2).repeat_interleave(2, -1)      # noqa: E731
    f, ci = w_in.shape[0], w_in.shape[1]
    win = w_in.reshape(f, ci).double()

    def composite(tp, l, wi, bi, wo):
        inner = torch.einsum("fc,chw->fhw", wi, l) + bi.view(-1, 1, 1)
        return torch.nn.functional.conv2d((up(tp) + inner)[None], wo, padding=1)[0]

    mid = composite(top.double(), l1.double(), win, b_in.double(), w_out.double())
    s_abs = composite(top.double().abs(), l1.double().abs(), win.abs(), b_in.double().abs(), w_out.double().abs())
    k_eff = composite((top != 0).double(), (l1 != 0).double(), (win != 0).double(), (b_in != 0).double(), (w_out != 0).double()).round()
    roundings = torch.where(k_eff > 0, (CB.ACC["split"] + 1) * k_eff + 2, torch.zeros_like(k_eff))
    return CB.Interval(mid, CB.C_MODE["split"] * s_abs + roundings * CB.U * s_abs, k_eff)


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("co,f,ci,hw2,bias", [(8, 32, 8, (11, 16), 0), (16, 64, 16, (19, 28), 1)])
def test_split_fpn_head_bounded(co, f, ci, hw2, bias, nhwc):
    """packing.pack_fpn_head_split + the pixel-shuffle-add epilogues (ADD_SHUF2, NHWC_ADD_SHUF2): impulses in the coarse map alone, in
    the fine map alone, and in both; without a lateral bias every element nothing reaches is exactly 0."""
    from effi_mvs_plus_amd import ops, packing
    h2, w2 = hw2
    tops, l1s = CC.fused_family("fpn_top", (f,), hw2), CC.fused_family("fpn_l1", (ci,), (2 * h2, 2 * w2))
    tops.assert_full(), l1s.assert_full()
    g = torch.Generator().manual_seed(co + f)
    w_out = CB.he_weights((co, f, 3, 3), 9 * f, g)
    w_in = CB.he_weights((f, ci, 1, 1), ci, g)
    b_in = torch.randn(f, generator=g) if bias else torch.zeros(f)
    (wu, bu), (wl, bl) = packing.pack_fpn_head_split(w_out.to(DEV), w_in.to(DEV), b_in.to(DEV))
    ones = torch.ones(1, h2, w2, device=DEV)
    epilogue = ops.EPI_NHWC_ADD_SHUF2 if nhwc else ops.EPI_ADD_SHUF2
    n = max(len(tops.members), len(l1s.members))
    zt, zl = torch.zeros_like(tops.members[0]), torch.zeros_like(l1s.members[0])
    with precision_("split"):
        for k in range(n):
            top, l1 = tops.members[k % len(tops.members)], l1s.members[k % len(l1s.members)]
            top, l1 = (top, zl) if k % 3 == 0 else (zt, l1) if k % 3 == 1 else (top, l1)
            u = launch(f"conv2d_k3x3_nt{(4 * co + 15) // 16}_epi0", lambda: ops.conv2d_k3_bf16x3([t(top, DEV), ones], wu, bu, 4 * co))
            got = launch(f"conv2d_k3x3_nt{(co + 15) // 16}_epi{epilogue}",
                         lambda: ops.conv2d_k3_bf16x3([t(l1, DEV)], wl, bl, co, epilogue=epilogue, aux0=u))
            if nhwc:
                got = got.permute(2, 0, 1)
            bounded("split FPN head" + (" (NHWC)" if nhwc else ""), f"FPN head co={co} f={f} ci={ci} member {k}", got,
                    _fpn_interval(top, l1, w_out, w_in, b_in))


def _up2x_interval(imask, inv, lo, hi):
    """The mask head's interval (36 channels: 4 k + s = tap k, sub-pixel s; already scaled by 0.25) carried through the convex x2
    upsampling of conv2d_x3.hpp: ac = sum_k softmax_k(v) n_k over the 3 x 3 neighbours n_k of the inverse depth (0 outside the map),
    depth = 1 / (lo + (hi - lo) ac), and depth_to_inv(depth) = ac again.  Counted:
      * logits within +-d (d = the largest half-width of the nine): every softmax weight moves by a factor within e^(+-2d), so
        |ac' - ac| <= (e^(2d) - 1) sum_k s_k |n_k - ac|;
      * evaluation: a_k = v_k - max (u |a_k|), a_k log2(e) (u |a_k| more), v_exp_f32 (1 ulp = 2u): e_k to (2 |a_k| + 2) u = eps_k; the
        nine-term sum 8u, the refined reciprocal 2u, e_k * r one u: weight k to rho_k = eps_k + sum_j s_j eps_j + 11u; nine products
        and nine additions: 10u sum s_k |n_k|;
      * s = a + b ac with a = 1 / (1 / lo), b = 1 / (1 / hi) - a (two roundings each, one for the difference): 2u a + 5u b |ac| + the
        product's and the sum's 2u s; depth = 1 / s: u more -- depth within 1 / (s - b dac) - 1 / s, + 9u of it;
      * back: 1 / depth (u), - a (u), / (b + 1e-10) (u, and 1e-10 / b): the constants are the same in both directions, so the inverse
        depth is ac + dac + (12u s + 1e-10 |ac|) / b.
    -> (interval of the depth [2h, 2w], interval of its inverse depth)."""
    h, w = inv.shape[-2:]
    v = imask.mid.view(9, 4, h, w)
    d = imask.half.view(9, 4, h, w).max(0).values
    nb = torch.nn.functional.unfold(inv.double().view(1, 1, h, w), 3, padding=1).view(9, 1, h, w)
    a_k = v - v.max(0, keepdim=True).values
    s_k = torch.softmax(v, 0)
    ac = (s_k * nb).sum(0)
    eps = (2 * a_k.abs() + 2) * CB.U
    rho = eps + (s_k * eps).sum(0, keepdim=True) + 11 * CB.U
    dac = torch.expm1(2 * d) * (s_k * (nb - ac).abs()).sum(0) + (s_k * rho * nb.abs()).sum(0) + 10 * CB.U * (s_k * nb.abs()).sum(0)
    # a convex combination stays inside its taps' range whatever the weights are: the cap keeps s away from inv_to_depth's clamp
    dac = torch.minimum(dac, nb.max(0).values - nb.min(0).values + 10 * CB.U)
    lo, hi = float(lo), float(hi)
    s = lo + (hi - lo) * ac
    s_low = s - (hi - lo) * dac                                              # >= lo (1 - 10u) > the clamp's 1e-4: 1 / s is monotone
    assert float(s_low.min()) > 1e-4
    depth = 1.0 / s
    shuffle = lambda q: q.view(2, 2, h, w).permute(2, 0, 3, 1).reshape(2 * h, 2 * w)     # noqa: E731  (sub-pixel s = 2 py + px)
    return (CB.Interval(shuffle(depth), shuffle((1.0 / s_low - depth) + 9 * CB.U / s_low)),
            CB.Interval(shuffle(ac), shuffle(dac + (12 * CB.U * s + 1e-10 * ac.abs()) / (hi - lo))))


@pytest.mark.parametrize("hd,c1,hw", [(16, 32, (21, 28)), (32, 64, (37, 52))])
def test_mask_head_with_convex_upsampling_bounded(hd, c1, hw):
    """conv2d_k3_k1_up2x and its split-resident twin: the mask never leaves the kernel, so the bound of the mask head (3x3 + ReLU + 1x1
    to 36 channels, scaled by 0.25) is carried through the nine-tap softmax to both outputs."""
    from effi_mvs_plus_amd import ops, packing
    h, w = hw
    fam = CC.fused_family("mask", (hd,), hw)
    fam.assert_full()
    w1, b1 = CC.weights(c1, hd, 3, seed=1500 + hd, bias=True)
    w2, b2 = CC.weights(36, c1, 1, seed=1600 + hd, bias=True)
    g = torch.Generator().manual_seed(hd)
    inv = torch.rand(1, h, w, generator=g)
    dv = torch.linspace(1 / 935.0, 1 / 425.0, 384)
    p1, pb1 = packing.pack_conv2d_bf16x3(w1.to(DEV), b1.to(DEV))
    p2, pb2 = packing.pack_mask_taps_per_lane(w2.to(DEV), b2.to(DEV), c1, scale=0.25)
    key = f"conv2d_k3k1up_nt{(c1 + 15) // 16}"
    with precision_("split"):
        for k, x in enumerate(fam.members):
            i1 = CB.act_interval(*CB.conv_interval(x, None, w1, b1, mode="split"), "relu")
            imask = chain(i1, 0.25 * w2, 0.25 * b2, padding=0)                          # (the scale is a power of two: exact)
            idepth, iinv = _up2x_interval(imask, inv, dv[0], dv[-1])
            depth, dinv = launch(key, lambda: ops.conv2d_k3_k1_up2x([t(x, DEV)], p1, pb1, c1, p2, pb2, t(inv, DEV), t(dv, DEV)))
            bounded("conv2d_k3_k1_up2x", f"mask head + upsampling depth hd={hd} member {k}", depth, idepth)
            bounded("conv2d_k3_k1_up2x", f"mask head + upsampling inverse depth hd={hd} member {k}", dinv, iinv)
            sr = ops.sr_from_planar(t(x, DEV))
            depth, dinv = launch(key, lambda: ops.conv2d_k3_k1_up2x_sr([sr], p1, pb1, c1, p2, pb2, t(inv, DEV), t(dv, DEV)))
            bounded("conv2d_k3_k1_up2x_sr", f"mask head + upsampling (SR) depth hd={hd} member {k}", depth, idepth)
            bounded("conv2d_k3_k1_up2x_sr", f"mask head + upsampling (SR) inverse depth hd={hd} member {k}", dinv, iinv)


# ---------------------------------------------------------------------------------------------
# 3-D: models.module.Conv3d / Deconv3d with BatchNorm folded, every branch of their run() in each precision
# ---------------------------------------------------------------------------------------------
def _rand_bn(bn, g, zero_shift):
    bn.weight.data = 0.6 + 0.8 * torch.rand(bn.weight.shape, generator=g)
    bn.running_var.data = 0.5 + torch.rand(bn.bias.shape, generator=g)
    if zero_shift:                         # shift = bias - mean * scale is exactly 0
        bn.bias.data.zero_()
        bn.running_mean.data.zero_()
    else:
        bn.bias.data = 0.1 * torch.randn(bn.bias.shape, generator=g)
        bn.running_mean.data = 0.1 * torch.randn(bn.bias.shape, generator=g)


def _vol_module(i):
    """The module of 3-D case i on the device, and the folded fp32 weight / shift its packers hold: the fold (one fp32 product per
    weight, packing.bn_scale_shift) is evaluated with the packers' own expression on the device, so the reference convolves exactly
    the weights the kernel gets and no rounding of the fold enters the bound."""
    from effi_mvs_plus_amd import packing
    from effi_mvs_plus_amd.models.module import Conv3d, Deconv3d
    kind, cins, cout, stride, dims, relu, skip = CC.VOL_CASES[i]
    cin = sum(cins)
    g = torch.Generator().manual_seed(3000 + i)
    if kind == "conv":
        m = Conv3d(cin, cout, stride=stride, padding=1, relu=relu).eval()
    else:
        st = CB._tuple(stride, 3)
        m = Deconv3d(cin, cout, stride=stride, padding=1, output_padding=tuple(s - 1 for s in st), relu=relu).eval()
    m.conv.weight.data = CB.he_weights(tuple(m.conv.weight.shape), 27 * cin / (1 if kind == "conv" else 4), g)
    _rand_bn(m.bn, g, zero_shift=i % 2 == 0)
    m = m.to(DEV)
    with torch.no_grad():
        scale, shift = packing.bn_scale_shift(m.bn)
        wf = (m.conv.weight * (scale.view(-1, 1, 1, 1, 1) if kind == "conv" else scale.view(1, -1, 1, 1, 1))).float().cpu()
    return m, wf, shift.float().cpu()


def _vol_interval(i, x, wf, shift, mode, skip):
    kind, cins, cout, stride, dims, relu, _ = CC.VOL_CASES[i]
    st = CB._tuple(stride, 3)
    tr = None if kind == "conv" else tuple(s - 1 for s in st)
    iv = CB.conv_interval(x, None, wf, shift, st, 1, tr, mode, 3)
    a = CB.act_interval(*iv, "relu") if relu else iv
    if skip is not None:
        a = CB.act_interval(*a, "add", add=skip)
    a.k_eff = iv.k_eff
    return a


@pytest.mark.parametrize("mode", ["fp32", "split", "bf16"])
@pytest.mark.parametrize("i", range(CC.N_VOL_BRANCH_CASES))
def test_conv3d_every_branch_bounded(i, mode):
    """Seams: the union over all 3-D forms (z: every second plane -- 2, 4, 8 planes per thread and the rolling window's runs; y: 4, 8,
    16; x: 16, 32).  The launch key asserts the branch of Conv3d.run / Deconv3d.run the case is written for; the bf16 entries share
    the split ones' keys, so a bf16 run of a matrix-core form must leave the split interval somewhere (``finer``)."""
    kind, cins, cout, stride, dims, relu, skip = CC.VOL_CASES[i]
    key = CC.VOL_KEYS[i][0 if mode in ("split", "bf16") else 1]
    arith = mode if any(s in key for s in ("roll", "x3")) else "fp32"          # the vector and fp32-MFMA kernels compute exact products
    fam = CC.vol_family(i)
    fam.assert_full()
    m, wf, shift = _vol_module(i)
    g = torch.Generator().manual_seed(i)
    st = CB._tuple(stride, 3)
    oshape = [CB.out_size(dims[a], 3, st[a], 1, None if kind == "conv" else st[a] - 1) for a in range(3)]
    sk = torch.randn(cout, *oshape, generator=g) if skip else None
    row = f"{key} ({mode})"
    left_finer = False
    with precision_(mode), torch.no_grad():
        for k, x in enumerate(fam.members):
            srcs = dev_srcs(fam, x)
            kw = {} if sk is None else {"skip": t(sk, DEV)}
            got = launch(key, lambda: m.run(srcs, **kw) if kind == "conv" else m.run(srcs[0], **kw))
            bounded(row, f"{kind}3d case {i} {cins}->{cout} s={stride} {dims} member {k}", got, _vol_interval(i, x, wf, shift, arith, sk),
                    x if kind == "conv" else None, wf.shape, st, 1, 3)
            if arith == "bf16":
                left_finer |= CB.escapes(got, *_vol_interval(i, x, wf, shift, finer(arith), sk))
    assert arith != "bf16" or left_finer, "the bf16 case stayed inside the split interval everywhere: the split kernel ran"


def test_conv3d_family_as_one_batch():
    """Sample-batched form: the members of one family as ONE launch of the rolling-window kernel."""
    i = 1
    fam = CC.vol_family(i)
    m, wf, shift = _vol_module(i)
    members = fam.members[:32]
    xb = t(torch.stack(members), DEV)
    with precision_("split"), torch.no_grad():
        got = launch(CC.VOL_KEYS[i][0], lambda: m.run([xb[:, :8].contiguous(), xb[:, 8:].contiguous()]))
    for k, x in enumerate(members):
        bounded("conv3d roll, family as one batch", f"conv3d batch member {k}", got[k], _vol_interval(i, x, wf, shift, "split", None))


# ---------------------------------------------------------------------------------------------
# Tile forms of the launch rules: the forms the rules pick on the LARGE maps of the workloads (conv_cases.FORM_CASES), each reached on
# a small map -- by its option, by a 528-wide map, by a batch or a narrow map that crosses the rule's threshold.  Per case: the
# form is asserted through ops.launch_form (and, where an option forces it, that the rule alone picks another); every element of
# every member is bounded by the SAME intervals as above (a pixel's accumulation order does not depend on the tile shape); and the
# result is bitwise the one of the rule's own form on that member -- the equality the sources claim.
# ---------------------------------------------------------------------------------------------
def reach(query, options, form):
    """The options of a form case, after asserting the form it reaches."""
    from effi_mvs_plus_amd import ops
    with ops.options(**options):
        got = tuple(ops.launch_form(**query))
    assert got == tuple(form), f"the rule gives {got} for {query} under {options}; the case is written for {form}"
    if options:
        assert tuple(ops.launch_form(**query)) != tuple(form), f"{options} force the form the rule picks anyway: {form}"
    return ops.options(**options)


def same_bits(name, a, b):
    assert a.shape == b.shape and torch.equal(a, b), f"{name}: the forced form's bits differ from the rule's form in {int((a != b).sum())} elements"


def _x3_runner(epi, sr, hw, mode="split", q4s=(False, True)):
    """(row, members, run) of an X3 case: run(member) -> [(label, output, interval)] of ONE launch of the epilogue on that member."""
    from effi_mvs_plus_amd import ops, packing
    h, w = hw
    d = lambda v: None if v is None else v.to(DEV)       # noqa: E731
    cins, cout = CC.x3_channels(epi)
    nt = (cout + 15) // 16
    kind = ("split-resident" if sr else "split") + f" 3x3 {epi.replace('96', '')}, tile forms"
    g = torch.Generator().manual_seed(len(epi) + h)
    if "shuf2" in epi:
        co, f, ci, (h2, w2) = 8, 32, 8, (h // 2, w // 2)
        tops, l1s = CC.form_family((f,), (h2, w2)), CC.form_family((ci,), hw)
        w_out, w_in, b_in = CB.he_weights((co, f, 3, 3), 9 * f, g), CB.he_weights((f, ci, 1, 1), ci, g), torch.randn(f, generator=g)
        (wu, bu), (wl, bl) = packing.pack_fpn_head_split(d(w_out), d(w_in), d(b_in))
        ones = torch.ones(1, h2, w2, device=DEV)
        epilogue = ops.EPI_NHWC_ADD_SHUF2 if epi == "nhwc_shuf2" else ops.EPI_ADD_SHUF2
        zt, zl = torch.zeros_like(tops.members[0]), torch.zeros_like(l1s.members[0])
        n = max(len(tops.members), len(l1s.members))
        pairs = [(tops.members[k % len(tops.members)], l1s.members[k % len(l1s.members)]) for k in range(n)]
        members = [(tp, zl) if k % 3 == 0 else (zt, l1) if k % 3 == 1 else (tp, l1) for k, (tp, l1) in enumerate(pairs)]

        def run(m):
            top, l1 = m
            u = launch(f"conv2d_k3x3_nt{(4 * co + 15) // 16}_epi0", lambda: ops.conv2d_k3_bf16x3([t(top, DEV), ones], wu, bu, 4 * co))
            got = launch(f"conv2d_k3x3_nt1_epi{epilogue}", lambda: ops.conv2d_k3_bf16x3([t(l1, DEV)], wl, bl, co, epilogue=epilogue, aux0=u))
            return [("FPN head", got.permute(2, 0, 1) if epi == "nhwc_shuf2" else got, _fpn_interval(top, l1, w_out, w_in, b_in))]
        return kind, members, run
    fam = CC.form_family(cins, hw)
    fam.assert_full()
    srcs_of = (lambda x: [ops.sr_from_planar(s_) for s_ in dev_srcs(fam, x)]) if sr else (lambda x: dev_srcs(fam, x))
    if epi in ("plain", "nhwc"):
        wt, b = CC.weights(cout, sum(cins), 3, seed=4000 + h, bias=True)
        wp, bp = packing.pack_conv2d_bf16x3(d(wt), d(b))
        epilogue = ops.EPI_NHWC if epi == "nhwc" else ops.EPI_PLAIN

        def run(x):
            a = CB.act_interval(*CB.conv_interval(x, None, wt, b, mode=mode), "relu")
            if sr:
                out0, out_sr = launch(f"conv2d_k3x3_nt{nt}_epi0", lambda: ops.conv2d_k3_sr(
                    srcs_of(x), wp, bp, cout, act=ops.ACT_RELU, out0=torch.empty(cout, h, w, device=DEV)))
                return [("sr plain", out0, a), ("sr plain (SR map)", sr_value(out_sr), widen_sr(a))]
            got = launch(f"conv2d_k3x3_nt{nt}_epi{epilogue}", lambda: ops.conv2d_k3_bf16x3(srcs_of(x), wp, bp, cout, epilogue=epilogue,
                                                                                            act=ops.ACT_RELU))
            return [(epi, got.permute(2, 0, 1) if epi == "nhwc" else got, a)]
        return kind, fam.members, run
    if epi.startswith("gru"):
        q = epi == "gru_q"
        wt, b = CC.weights(cout, sum(cins), 3, seed=4100 + cout + h, bias=True)
        wp, bp = packing.pack_conv2d_bf16x3(d(wt), d(b))
        hd = cout if q else cout // 2
        hprev, z = torch.tanh(torch.randn(hd, h, w, generator=g)), torch.rand(hd, h, w, generator=g)
        epilogue = ops.EPI_GRU_Q if q else ops.EPI_GRU_ZR
        key = f"conv2d_k3x3_nt{nt}_epi{epilogue}"

        def run(x):
            iv = CB.conv_interval(x, None, wt, b, mode="split")
            iq = CB.act_interval(*iv, "gru_q", "split", h=hprev, z=z) if q else None
            iz = None if q else CB.act_interval(iv.mid[:hd], iv.half[:hd], "gru_z", "split")
            irh = None if q else CB.act_interval(iv.mid[hd:], iv.half[hd:], "gru_rh", "split", h=hprev)
            out = []
            if not sr:
                if q:
                    return [("GRU_Q", launch(key, lambda: ops.conv2d_k3_bf16x3(srcs_of(x), wp, bp, cout, epilogue=epilogue, aux0=t(hprev, DEV),
                                                                               aux1=t(z, DEV))), iq)]
                gz, grh = launch(key, lambda: ops.conv2d_k3_bf16x3(srcs_of(x), wp, bp, cout, epilogue=epilogue, aux0=t(hprev, DEV)))
                return [("GRU z", gz, iz), ("GRU r*h", grh, irh)]
            for q4 in q4s:                     # planar and / or q4 auxiliaries
                lay = (lambda v: ops.q4_from_planar(t(v, DEV))) if q4 else (lambda v: t(v, DEV))
                back = (lambda v, c: ops.q4_to_planar(v.view(c // 4, h, w, 4), c)) if q4 else (lambda v, c: v)
                if q:
                    hn, _ = launch(key, lambda: ops.conv2d_k3_sr(srcs_of(x), wp, bp, cout, epilogue=epilogue, aux0=lay(hprev), aux1=lay(z), q4=q4))
                    out.append((f"sr GRU_Q q4={q4}", back(hn, cout), iq))
                else:
                    gz, rh = launch(key, lambda: ops.conv2d_k3_sr(srcs_of(x), wp, bp, cout, epilogue=epilogue, aux0=lay(hprev), q4=q4))
                    out += [(f"sr GRU z q4={q4}", back(gz, hd), iz), (f"sr GRU r*h q4={q4}", sr_value(rh), widen_sr(irh))]
            return out
        return kind, fam.members, run
    w1, b1 = CC.weights(cout, sum(cins), 3, seed=4200 + cout + h, bias=True)
    p1, pb1 = packing.pack_conv2d_bf16x3(d(w1), d(b1))
    if epi == "k1":
        c_extra, cout2 = CC.K1_EXTRA, 16
        extras = CC.form_family((c_extra,), hw).members
        w2, b2 = CC.weights(cout2, cout + c_extra, 1, seed=4300 + h, bias=True)
        w2p, b2p = packing.pack_conv1x1_after(d(w2), d(b2), cout, c_extra)
        fn = ops.conv2d_k3_k1_sr if sr else ops.conv2d_k3_k1_x3
        members = [(x, extras[k % len(extras)]) for k, x in enumerate(fam.members)]

        def run(m):
            x, extra = m
            got = launch(f"conv2d_k3k1_nt{nt}", lambda: fn(srcs_of(x), p1, pb1, cout, t(extra, DEV), w2p, b2p, cout2, relu=True, relu1=False))
            i1 = CB.conv_interval(x, None, w1, b1, mode="split")
            i2 = chain(CB.Interval(torch.cat([i1.mid, extra.double()]), torch.cat([i1.half, torch.zeros_like(extra, dtype=torch.float64)])),
                       w2, b2, padding=0)
            return [("3x3+1x1", got, CB.act_interval(*i2, "relu"))]
        return kind, members, run
    assert epi == "k1up"
    w2, b2 = CC.weights(36, cout, 1, seed=4400 + h, bias=True)
    inv, dv = torch.rand(1, h, w, generator=g), torch.linspace(1 / 935.0, 1 / 425.0, 384)
    p2, pb2 = packing.pack_mask_taps_per_lane(d(w2), d(b2), cout, scale=0.25)
    fn = ops.conv2d_k3_k1_up2x_sr if sr else ops.conv2d_k3_k1_up2x

    def run(x):
        i1 = CB.act_interval(*CB.conv_interval(x, None, w1, b1, mode="split"), "relu")
        idepth, iinv = _up2x_interval(chain(i1, 0.25 * w2, 0.25 * b2, padding=0), inv, dv[0], dv[-1])
        depth, dinv = launch(f"conv2d_k3k1up_nt{nt}", lambda: fn(srcs_of(x), p1, pb1, cout, p2, pb2, t(inv, DEV), t(dv, DEV)))
        return [("mask head + upsampling depth", depth, idepth), ("mask head + upsampling inverse depth", dinv, iinv)]
    return kind, fam.members, run


def _run_form_case(row, members, run, ctx, other=None, finer_of=None):
    """Every member under the form's options (``ctx``) bounded, and bitwise the run under ``other`` (default: no option, the rule's own
    form).  ``finer_of(member, label)``: the finer arithmetic's interval -- some output must leave it (bf16 cases)."""
    import contextlib
    left = False
    for k, m in enumerate(members):
        with ctx:
            forced = run(m)
        with (other or contextlib.nullcontext()):
            ruled = run(m)
        for (label, got, iv), (_, ref, _) in zip(forced, ruled):
            bounded(row, f"{row}: {label} member {k}", got, iv)
            same_bits(f"{row}: {label} member {k}", got, ref)
            if finer_of is not None:
                left |= CB.escapes(got, *finer_of(m, label))
    assert finer_of is None or left, "the bf16 case stayed inside the split interval everywhere: the split kernel ran"


@pytest.mark.parametrize("epi,sr,f", CC.X3_CASES, ids=[f"{e}-{'sr' if s_ else 'planar'}-{f}" for e, s_, f in CC.X3_CASES])
def test_split_3x3_tile_forms_bounded(epi, sr, f):
    """launch_bf16x3 with every epilogue under 4 rows per wave, narrow (16 x 16 tiles, force_mr at 21 x 28) and wide (4 x 64 tiles, force_mr
    at 21 x 528: the rule's own w >= 512; ragged last tile of 16 columns), planar and split-resident; 2 rows per wave dealt round; the
    eight-wave SR workgroup where the rule picks it unaided ((48, 48) -> 96 at 21 x 28), against the four-wave one (sr_waves = 4)."""
    from effi_mvs_plus_amd import ops
    form, hw, opts = CC.x3_form(epi, sr, f)
    nt = (CC.x3_channels(epi)[1] + 15) // 16
    with precision_("split"):
        ctx = reach(dict(launcher="x3", h=hw[0], w=hw[1], nt=nt, sr=sr), opts, form)
        other = None
        if f == "w8":
            with ops.options(sr_waves=4):
                assert tuple(ops.launch_form("x3", hw[0], hw[1], nt=nt, sr=True)) == CC.MR1
            other = ops.options(sr_waves=4)
        # (SR GRU epilogues: the q4 layout of the auxiliaries, the product's default, everywhere; the planar one too on the 9-row maps)
        row, members, run = _x3_runner(epi, sr, hw, q4s=(False, True) if f == "wide9" else (True,))
        _run_form_case(row, members, run, ctx, other)


def test_split_3x3_wide_tiles_in_bf16_leave_the_split_interval():
    """The wide tile once more with plain bf16 operands: bounded by the bf16 interval, bitwise the narrow form, and somewhere outside
    the split interval (the split kernel did not run in its place)."""
    epi, sr, f = CC.X3_BF16
    form, hw, opts = CC.x3_form(epi, sr, f)
    cins, cout = CC.x3_channels(epi)
    wt, b = CC.weights(cout, sum(cins), 3, seed=4000 + hw[0], bias=True)         # (the weights of _x3_runner's "plain" case)
    with precision_("bf16"):
        ctx = reach(dict(launcher="x3", h=hw[0], w=hw[1], nt=1), opts, form)
        row, members, run = _x3_runner(epi, sr, hw, mode="bf16")
        _run_form_case(row + " (bf16)", members, run, ctx,
                       finer_of=lambda x, label: CB.act_interval(*CB.conv_interval(x, None, wt, b, mode="split"), "relu"))


@pytest.mark.parametrize("sr,f", CC.PAIR_CASES, ids=[f"{'sr' if s_ else 'planar'}-{f}" for s_, f in CC.PAIR_CASES])
def test_split_3x3_pair_tile_forms_bounded(sr, f):
    """launch_bf16x3_pair: 1 (the rule at 21 x 28), 2 and 4 rows per wave and the wide tile (9 x 528), planar and split-resident; two
    DIFFERENT convolutions of one member, each bitwise the single launch of the rule's form."""
    from effi_mvs_plus_amd import ops, packing
    form, (h, w), opts = CC._X3_FORM[f]
    cins, cout = (16,), 16
    fam = CC.form_family(cins, (h, w))
    fam.assert_full()
    (wa, ba), (wb, bb) = CC.weights(cout, 16, 3, seed=4500 + h, bias=True), CC.weights(cout, 16, 3, seed=4600 + h, bias=False)
    d = lambda v: None if v is None else v.to(DEV)       # noqa: E731
    (pa, pba), (pb, pbb) = packing.pack_conv2d_bf16x3(d(wa), d(ba)), packing.pack_conv2d_bf16x3(d(wb), d(bb))
    row = f"conv2d_k3 pair{' sr' if sr else ''}, tile forms"
    with precision_("split"):
        ctx = reach(dict(launcher="x3_pair", h=h, w=w, nt=1, sr=sr), opts, form)
        for k, x in enumerate(fam.members):
            ia = CB.act_interval(*CB.conv_interval(x, None, wa, ba, mode="split"), "relu")
            ib = CB.act_interval(*CB.conv_interval(x, None, wb, bb, mode="split"), "relu")
            if sr:
                srcs = [ops.sr_from_planar(s_) for s_ in dev_srcs(fam, x)]
                oa, ob = ops.sr_alloc(2, cout, h, w, DEV)
                with ctx:
                    launch("conv2d_k3x3_pair_nt1", lambda: ops.conv2d_k3_pair_sr(srcs, pa, pba, oa, srcs, pb, pbb, ob, cout, act=ops.ACT_RELU))
                ga, gb, ia, ib = sr_value(oa), sr_value(ob), widen_sr(ia), widen_sr(ib)
                ra = sr_value(launch("conv2d_k3x3_nt1_epi0", lambda: ops.conv2d_k3_sr(srcs, pa, pba, cout, act=ops.ACT_RELU)))
                rb = sr_value(launch("conv2d_k3x3_nt1_epi0", lambda: ops.conv2d_k3_sr(srcs, pb, pbb, cout, act=ops.ACT_RELU)))
            else:
                srcs = dev_srcs(fam, x)
                with ctx:
                    ga, gb = launch("conv2d_k3x3_pair_nt1", lambda: ops.conv2d_k3_bf16x3_pair(srcs, pa, pba, srcs, pb, pbb, cout, act=ops.ACT_RELU))
                ra = launch("conv2d_k3x3_nt1_epi0", lambda: ops.conv2d_k3_bf16x3(srcs, pa, pba, cout, act=ops.ACT_RELU))
                rb = launch("conv2d_k3x3_nt1_epi0", lambda: ops.conv2d_k3_bf16x3(srcs, pb, pbb, cout, act=ops.ACT_RELU))
            for name, got, iv, ref, wt in (("a", ga, ia, ra, wa), ("b", gb, ib, rb, wb)):
                bounded(row, f"{row} {f}: {name} member {k}", got, iv, x, wt.shape)
                same_bits(f"{row} {f}: {name} member {k}", got, ref)


@pytest.mark.parametrize("launcher,f", CC.BATCH_CASES, ids=[f for _, f in CC.BATCH_CASES])
def test_split_3x3_batch_tile_forms_bounded(launcher, f):
    """launch_bf16x3_batch: a whole family as ONE launch (NHWC for the odd cases); the rule counts the tiles of all images -- 48 images
    of 9 x 528 get the wide tile unaided -- and image i is bitwise the single launch on member i."""
    from effi_mvs_plus_amd import ops, packing
    form, (h, w), opts = CC._X3_FORM[f]
    opts = {} if f == "wide9" else opts
    fam = CC.form_family((16,), (h, w))
    fam.assert_full()
    wt, b = CC.weights(16, 16, 3, seed=4700 + h, bias=True)
    wp, bp = packing.pack_conv2d_bf16x3(wt.to(DEV), b.to(DEV))
    nhwc = f in ("mr2", "wide9")
    epilogue = ops.EPI_NHWC if nhwc else ops.EPI_PLAIN
    xb = t(torch.stack(fam.members), DEV)
    row = "split 3x3 batch, tile forms"
    with precision_("split"):
        with reach(dict(launcher=launcher, h=h, w=w, nt=1, count=len(fam.members)), opts, form):
            got = launch(f"conv2d_k3x3_nt1_epi{epilogue}_batch", lambda: ops.conv2d_k3_bf16x3([xb], wp, bp, 16, epilogue=epilogue, act=ops.ACT_RELU))
        for k, x in enumerate(fam.members):
            one = launch(f"conv2d_k3x3_nt1_epi{epilogue}", lambda: ops.conv2d_k3_bf16x3([xb[k]], wp, bp, 16, epilogue=epilogue, act=ops.ACT_RELU))
            gk = got[k].permute(2, 0, 1) if nhwc else got[k]
            bounded(row, f"{row} {f}: member {k}", gk, CB.act_interval(*CB.conv_interval(x, None, wt, b, mode="split"), "relu"), x, wt.shape)
            same_bits(f"{row} {f}: member {k}", got[k], one)


@pytest.mark.parametrize("f", ["mr1", "mr2", "mr4"])
def test_conv3d_z_batched_tile_forms_bounded(f):
    """The z-batched split 3-D convolution (launch_bf16x3 with ZB, VOL case 4) and its sample batch (launch_bf16x3_zb_batch) under 1
    (the rule), 2 and 4 rows per wave; samples in batches of ZB_BATCH, each bitwise the single launch of the rule's form."""
    from effi_mvs_plus_amd import ops
    i = 4
    form, _, opts = CC._X3_FORM[f]
    kind, cins, cout, stride, (D, h, w), relu, skip = CC.VOL_CASES[i]
    fam = CC.vol_family(i)
    m, wf, shift = _vol_module(i)
    key = CC.VOL_KEYS[i][0]
    n, members = CC.ZB_BATCH, fam.members
    row = "conv3d z-batched split, tile forms"
    with precision_("split"), torch.no_grad():
        one = reach(dict(launcher="x3", h=h, w=w, nt=2, planes=D, zb=True), opts, form)
        many = reach(dict(launcher="x3_zb_batch", h=h, w=w, nt=2, planes=D, count=n), opts, form)
        for s0 in [min(s0, len(members) - n) for s0 in range(0, len(members), n)]:
            xb = t(torch.stack(members[s0:s0 + n]), DEV)
            with many:
                gb = launch(key, lambda: m.run([xb]))
            for j in range(n):
                x = members[s0 + j]
                with one:
                    got = launch(key, lambda: m.run([xb[j]]))
                ref = got if not opts else launch(key, lambda: m.run([xb[j]]))
                bounded(row, f"{row} {f}: member {s0 + j}", got, _vol_interval(i, x, wf, shift, "split", None), x, wf.shape, (1, 1, 1), 1, 3)
                same_bits(f"{row} {f}: member {s0 + j}", got, ref)
                same_bits(f"{row} {f}: batched member {s0 + j}", gb[j], ref)


@pytest.mark.parametrize("idx", range(len(CC.GENERIC_FORM_CASES)))
def test_generic_fp32_tile_forms_bounded(idx):
    """launch2d / launch2d_batch have no option: the narrowest maps that cross the rule's thresholds (conv_cases.GENERIC_FORM_CASES),
    single and as batches of images.  A batch is compared bitwise with the single launches (another form: fewer tiles)."""
    from effi_mvs_plus_amd import ops, packing
    ks, cins, cout, act, (h, w), n, form = CC.GENERIC_FORM_CASES[idx]
    fam = CC.family(cins, (h, w), ks // 2, CC.fam_key(CC.GENERIC_TILES), seed=ks + sum(cins))
    fam.assert_full()
    wt, b = CC.weights(cout, sum(cins), ks, seed=4800 + idx, bias=idx % 2)
    wp, bp = packing.pack_conv2d_mfma(wt.to(DEV), None if b is None else b.to(DEV))
    nt = (cout + 15) // 16
    key = f"conv2d_k{ks}_nt{nt}_epi{ops.EPI_PLAIN}"
    row = f"generic fp32 conv2d k{ks}, tile forms"
    query = dict(launcher="conv2d", h=h, w=w, nt=nt, k1=ks == 1)
    members = fam.members

    def check(k, got):
        iv = CB.conv_interval(members[k], None, wt, b, 1, ks // 2, None, "fp32")
        a = CB.act_interval(*iv, ACTS[act], "exact")
        a.k_eff = iv.k_eff
        bounded(row, f"{row} {h}x{w} x{n}: member {k}", got, a, members[k], wt.shape, 1, ks // 2)

    with reach(dict(query, count=n), {}, form):
        if n == 1:
            for k, x in enumerate(members):
                check(k, launch(key, lambda: ops.conv2d(dev_srcs(fam, x), wp, bp, cout, ks, act=act)))
            return
        assert tuple(ops.launch_form(**dict(query, count=1))) != tuple(form), "the single image takes the same form: nothing to compare"
        for s0 in [min(s0, len(members) - n) for s0 in range(0, len(members), n)]:
            xb = t(torch.stack(members[s0:s0 + n]), DEV)
            gb = launch(key + "_batch", lambda: ops.conv2d([xb], wp, bp, cout, ks, act=act))
            for j in range(n):
                check(s0 + j, gb[j])
                same_bits(f"{row}: member {s0 + j}", gb[j], launch(key, lambda: ops.conv2d([xb[j]], wp, bp, cout, ks, act=act)))


def _roll_interval(i, x, wf, shift, mode):
    return _vol_interval(i, x, wf, shift, mode, None)


@pytest.mark.parametrize("entry,i,rp,mr,zt", CC.ROLL_CASES, ids=[f"{e}-case{i}-rp{rp}-mr{mr}-zt{zt}" for e, i, rp, mr, zt in CC.ROLL_CASES])
def test_conv3d_rolling_window_tile_forms_bounded(entry, i, rp, mr, zt):
    """launch_roll at D = 12: 2 and 4 rows per wave with one run of 12 planes, three full runs of 4 (the window refilled at every run
    boundary) and runs of 5 with a ragged last one of 2; the single, pair and sample-batched entries; the row-pair kernels (cout <=
    8) and the one-row operand (roll_rp = 0, packed under the same option; cout 16).  Bitwise the rule's own form (runs of one plane)."""
    from effi_mvs_plus_amd import ops, packing
    kind, cins, cout, stride, (D, h, w), relu, skip = CC.VOL_CASES[i]
    fam = CC.form_vol_family(i)
    fam.assert_full()
    m, wf, shift = _vol_module(i)
    opts = {"roll_mr": mr, "roll_zt": zt}
    rp_opts = {} if rp is None else {"roll_rp": rp}
    count = {"single": 1, "pair": 2, "batch": CC.ROLL_BATCH}[entry]
    key = CC.VOL_KEYS[i][0]
    row = f"conv3d roll {entry}, tile forms"
    variant = 1 if cout <= 8 and rp != 0 else 0
    with precision_("split"), torch.no_grad(), ops.options(**rp_opts):
        ctx = reach(dict(launcher="roll", h=h, w=w, nt=(cout + 15) // 16, planes=D, cout=cout, count=count, oct2=sum(cins) == 16), opts,
                    (mr, 16, 4, zt, variant))
        wp, bp = packing.pack_conv3d_roll_bf16x3(m.conv, m.bn)          # (packed under roll_rp: the operand layout follows the option)
        run1 = lambda srcs: ops.conv3d_k3s1_roll(srcs, wp, bp, cout, relu=relu)          # noqa: E731
        members = fam.members
        if entry == "batch":
            for s0 in [min(s0, len(members) - count) for s0 in range(0, len(members), count)]:
                xb = t(torch.stack(members[s0:s0 + count]), DEV)
                with ctx:
                    gb = launch(key, lambda: run1([xb]))
                for j in range(count):
                    bounded(row, f"{row}: member {s0 + j}", gb[j], _roll_interval(i, members[s0 + j], wf, shift, "split"))
                    same_bits(f"{row}: member {s0 + j}", gb[j], launch(key, lambda: run1([xb[j]])))
            return
        for k, x in enumerate(members):
            srcs = dev_srcs(fam, x)
            iv = _roll_interval(i, x, wf, shift, "split")
            ref = launch(key, lambda: run1(srcs))
            if entry == "single":
                with ctx:
                    outs = [launch(key, lambda: run1(srcs))]
            else:                                    # the pair: the same convolution on a member and on its neighbour in the family
                y = members[(k + 1) % len(members)]
                with ctx:
                    ga, gb = launch(f"conv3d_roll_pair_oct{sum(cins) // 8}", lambda: ops.conv3d_k3s1_roll_pair(
                        srcs, wp, bp, dev_srcs(fam, y), wp, bp, cout, relu=relu))
                bounded(row, f"{row}: b member {k}", gb, _roll_interval(i, y, wf, shift, "split"))
                outs = [ga]
            for got in outs:
                bounded(row, f"{row}: member {k}", got, iv, x, wf.shape, (1, 1, 1), 1, 3)
                same_bits(f"{row}: member {k}", got, ref)


def test_conv3d_rolling_window_runs_in_bf16_leave_the_split_interval():
    """4 rows per wave, runs of 5 planes, plain bf16 operands: inside the bf16 interval, bitwise the rule's form, outside the split one."""
    from effi_mvs_plus_amd import ops, packing
    entry, i, rp, mr, zt = CC.ROLL_BF16
    kind, cins, cout, stride, (D, h, w), relu, skip = CC.VOL_CASES[i]
    fam = CC.form_vol_family(i)
    m, wf, shift = _vol_module(i)
    left = False
    with precision_("bf16"), torch.no_grad():
        ctx = reach(dict(launcher="roll", h=h, w=w, planes=D, cout=cout), {"roll_mr": mr, "roll_zt": zt}, (mr, 16, 4, zt, 1))
        wp, bp = packing.pack_conv3d_roll_bf16x3(m.conv, m.bn)
        for k, x in enumerate(fam.members):
            srcs = dev_srcs(fam, x)
            with ctx:
                got = launch(CC.VOL_KEYS[i][0], lambda: ops.conv3d_k3s1_roll(srcs, wp, bp, cout, relu=relu))
            bounded("conv3d roll single, tile forms (bf16)", f"roll bf16 member {k}", got, _roll_interval(i, x, wf, shift, "bf16"))
            same_bits(f"roll bf16 member {k}", got, launch(CC.VOL_KEYS[i][0], lambda: ops.conv3d_k3s1_roll(srcs, wp, bp, cout, relu=relu)))
            left |= CB.escapes(got, *_roll_interval(i, x, wf, shift, "split"))
    assert left, "the bf16 case stayed inside the split interval everywhere: the split kernel ran"


@pytest.mark.parametrize("i,n,mr", CC.DECONV_CASES)
def test_deconv3d_split_two_rows_per_wave_bounded(i, n, mr):
    """deconv3d_s2_bf16x3 with 2 rows per wave (deconv_mr; the rule picks 1 on these maps): cout 8 with a skip on unaligned rows and cout
    16, single and as sample batches of 3 (the batched kernel), bitwise the one-row form."""
    from effi_mvs_plus_amd import ops
    kind, cins, cout, stride, (D, h, w), relu, skip = CC.VOL_CASES[i]
    fam = CC.vol_family(i)
    m, wf, shift = _vol_module(i)
    g = torch.Generator().manual_seed(i)
    sk = torch.randn(cout, 2 * D, 2 * h, 2 * w, generator=g) if skip else None
    row = "deconv3d_x3, two rows per wave"
    members = fam.members
    with precision_("split"), torch.no_grad():
        ctx = reach(dict(launcher="deconv_x3", h=h, w=w, planes=D, cout=cout, count=n), {"deconv_mr": mr}, (mr, 16, 4, 1, 0))
        for s0 in [min(s0, len(members) - n) for s0 in range(0, len(members), n)]:
            xb = t(torch.stack(members[s0:s0 + n]), DEV)
            kw = {} if sk is None else {"skip": t(sk, DEV) if n == 1 else t(torch.stack([sk] * n), DEV)}
            with ctx:
                gb = launch("deconv3d_x3", lambda: m.run(xb[0] if n == 1 else xb, **kw))
            gb = gb[None] if n == 1 else gb
            for j in range(n):
                kw1 = {} if sk is None else {"skip": t(sk, DEV)}
                bounded(row, f"{row}: case {i} member {s0 + j}", gb[j], _vol_interval(i, members[s0 + j], wf, shift, "split", sk))
                same_bits(f"{row}: case {i} member {s0 + j}", gb[j], launch("deconv3d_x3", lambda: m.run(xb[j], **kw1)))


@pytest.mark.parametrize("row,launcher,i,mode,n,form", CC.VOL_BATCH_CASES, ids=[f"{r.replace(' ', '_')}-case{i}-x{n}" for r, _, i, _, n, _ in CC.VOL_BATCH_CASES])
def test_conv3d_batch_crosses_the_rule_threshold_bounded(row, launcher, i, mode, n, form):
    """The 3-D rules without an option: the family of a VOL case, its members repeated in turn, as ONE sample batch large enough to
    cross the rule's workgroup threshold (conv_cases.VOL_BATCH_CASES states each count beside its threshold).  Every member bounded,
    bitwise the single launch (the rule's small-map form, asserted to differ) and bitwise its own repetitions."""
    from effi_mvs_plus_amd import ops
    kind, cins, cout, stride, dims, relu, skip = CC.VOL_CASES[i]
    key = CC.VOL_KEYS[i][0 if mode == "split" else 1]
    arith = mode if any(s_ in key for s_ in ("roll", "x3")) else "fp32"
    fam = CC.vol_family(i)
    m, wf, shift = _vol_module(i)
    members = fam.members
    xb = t(torch.stack([members[j % len(members)] for j in range(n)]), DEV)
    trow = f"{key} ({mode}), sample batch of {n}"
    with precision_(mode), torch.no_grad():
        assert tuple(ops.launch_form(**CC.vol_query(launcher, i, 1))) != tuple(form)
        with reach(CC.vol_query(launcher, i, n), {}, form):
            gb = launch(key, lambda: m.run([xb]) if kind == "conv" else m.run(xb))
        for j in range(n):
            k = j % len(members)
            if j == k:
                x = members[k]
                bounded(trow, f"{trow}: member {k}", gb[j], _vol_interval(i, x, wf, shift, arith, None), x if kind == "conv" else None, wf.shape,
                        CB._tuple(stride, 3), 1, 3)
                same_bits(f"{trow}: member {k}", gb[j], launch(key, lambda: m.run([xb[j]]) if kind == "conv" else m.run(xb[j])))
            else:
                same_bits(f"{trow}: sample {j}, a repetition of member {k}", gb[j], gb[k])


@pytest.mark.parametrize("mode", ["fp32", "split"])
@pytest.mark.parametrize("hw,n,form", CC.K5S2_FORM_CASES)
def test_5x5_stride2_two_rows_per_wave_bounded(hw, n, form, mode):
    """dispatch_k5s2 / launch_s2_x3 and their batched twins with 2 rows per wave: the narrowest maps that cross 512 (split: 400)
    tiles -- one image of 17 x 8192, two of 17 x 4096 (each alone takes one row per wave: the form the batch is compared with)."""
    from effi_mvs_plus_amd import ops, packing
    (cin,), cout = CC.K5S2_FORM_CHANNELS
    fam = CC.k5s2_form_family(hw)
    fam.assert_full()
    wt, b = CC.weights(cout, cin, 5, seed=4900 + hw[1], bias=True)
    wp, bp = packing.pack_conv2d(wt.to(DEV), b.to(DEV))
    launcher = "s2_x3" if mode == "split" else "k5s2"
    key = f"conv2d_k5s2{'x3' if mode == 'split' else ''}_nt{(cout + 15) // 16}"
    q = dict(launcher=launcher, h=(hw[0] - 1) // 2 + 1, w=(hw[1] - 1) // 2 + 1, nt=(cout + 15) // 16)
    row = f"conv2d_k5s2 ({mode}), two rows per wave"
    members = fam.members
    iv = lambda x: CB.act_interval(*CB.conv_interval(x, None, wt, b, 2, 2, None, mode), "relu")          # noqa: E731
    with precision_(mode), reach(dict(q, count=n), {}, form):
        if n == 1:
            for k, x in enumerate(members):
                bounded(row, f"{row}: member {k}", launch(key, lambda: ops.conv2d_k5s2(t(x, DEV), wp, bp, cout, act=ops.ACT_RELU)), iv(x), x, wt.shape, 2, 2)
            return
        assert tuple(ops.launch_form(**dict(q, count=1))) == CC.MR1
        for s0 in [min(s0, len(members) - n) for s0 in range(0, len(members), n)]:
            xb = t(torch.stack(members[s0:s0 + n]), DEV)
            gb = launch(key + "_batch", lambda: ops.conv2d_k5s2(xb, wp, bp, cout, act=ops.ACT_RELU))
            for j in range(n):
                bounded(row, f"{row}: member {s0 + j}", gb[j], iv(members[s0 + j]), members[s0 + j], wt.shape, 2, 2)
                same_bits(f"{row}: member {s0 + j}", gb[j], launch(key, lambda: ops.conv2d_k5s2(xb[j], wp, bp, cout, act=ops.ACT_RELU)))
