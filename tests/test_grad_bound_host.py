"""CPU proof that the instrument of tests/grad_bound.py is right and sharp:

* torch's float64 autograd equals ``mid`` on every family of tests/grad_cases.py;
* torch's own fp32 ``conv*_weight`` / autograd gradients and an explicit fp32 restatement of ``wgrad_nd_kernel``'s strip / thread / lane /
  wave order lie inside EVERY interval -- the bit-exact pins included -- with nothing left out;
* every coverage table is full;
* the split and bf16 arithmetics leave the fp32 interval on every route (so the GPU assertion "inside the fp32 interval under every
  ``ops.set_precision``" can fail);
* twelve mutants are caught, each by the check it is meant to trip, and the table printed by ``test_mutants`` records which of them
  the present rule -- rel <= max(2e-5, 4 e_ref) relative to the peak, on a dense Gaussian input -- accepts.  Mutant 1 (products formed
  from bf16 hi / lo halves) is accepted by it for the input gradient and for the weight gradient: the reason this file exists."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_bound as CB
import grad_bound as GB
import grad_cases as GC
from test_gpu_train_scale import launch_shape

def _conv_weight64(A, Bs, kd, ks, stride, dtype=torch.float64):
    """dW of the row by torch autograd: the convolution of the concatenated B whose output gradient is A."""
    B = torch.cat(Bs, 0).to(dtype)[None]
    st = (stride[0], stride[1], stride[1])
    W = torch.zeros(A.shape[0], B.shape[1], kd, ks, ks, dtype=dtype, requires_grad=True)
    y = F.conv3d(B, W, None, stride=st, padding=(kd // 2, ks // 2, ks // 2))
    y.backward(A.to(dtype)[None])
    return W.grad.reshape(A.shape[0], B.shape[1], -1)


def _row_interval(i, m, prior=None):
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = GC.WGRAD[i]
    fam, Bs = GC.wgrad_case(i)
    terms, off = [], 0
    for B in Bs:
        terms.append(GB.wgrad_terms(fam.members[m], B, kd, ks, stride, sum(cbs), off))
        off += B.shape[0]
    return GB.wgrad_finish(terms, prior, strips=strips)


def _restate_row(i, A, prior=None, hook=None, hook_source=None):
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = GC.WGRAD[i]
    fam, Bs = GC.wgrad_case(i)
    dw, off = prior, 0
    for s, B in enumerate(Bs):
        h = hook if (hook_source is None or hook_source == s) else None
        dw = GB.restate_wgrad(A, B, kd, ks, stride, sum(cbs), off, strips, dw, h)
        off += B.shape[0]
    return dw


# ---------------------------------------------------------------------------------------------
# the weight gradient: reference, torch fp32, the restatement, coverage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(GC.WGRAD)), ids=GC.wgrad_ids())
def test_wgrad_family_reference_torch_fp32_and_restatement(i):
    row = GC.WGRAD[i]
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = row
    assert GC.strips_of(row, launch_shape) == strips
    fam, Bs = GC.wgrad_case(i)
    fam.assert_full()
    L = len(fam.members)
    gen = torch.Generator().manual_seed(i)
    prior = CB._values(ca * sum(cbs) * kd * ks * ks, gen).view(ca, sum(cbs), -1)
    used, pinned0, pinned1 = 0.0, 0, 0
    for m in range(L):
        iv = _row_interval(i, m)
        A = fam.members[m]
        if m in (0, L // 2, L - 2, fam.few):                               # float64 autograd equals mid (a pinned mid is RN(a b))
            ref = _conv_weight64(A, Bs, kd, ks, stride)
            assert bool(((iv.mid - ref).abs() <= 1.001 * CB.U * ref.abs() + 1e-13 * iv.parts[0]).all()), f"{name} member {m}: mid"
        got32 = _conv_weight64(A, Bs, kd, ks, stride, torch.float32)
        used = max(used, CB.check_bounded(f"{name} torch fp32 member {m}", got32, *iv, k_eff=iv.k_eff, quiet=True)["used"])
        CB.check_bounded(f"{name} restatement member {m}", _restate_row(i, A), *iv, k_eff=iv.k_eff, quiet=True)
        pinned0 += int(((iv.half == 0) & (iv.k_eff == 0)).sum())
        pinned1 += int(((iv.half == 0) & (iv.k_eff == 1)).sum())
        if m in (i % (L - 1), fam.few):                                    # onto a dW that already holds values
            ivp = _row_interval(i, m, prior)
            r = CB.check_bounded(f"{name} restatement onto a prior, member {m}", _restate_row(i, A, prior), *ivp, k_eff=ivp.k_eff, quiet=True)
            used = max(used, r["used"])
    print(f"[grad-host] {name:34s} members {L:3d} strips {strips} largest share used {used:.3f}  pinned to 0: {pinned0}  to RN(ab): {pinned1}")


def test_every_coverage_table_is_full():
    cells = 0
    for i in range(len(GC.WGRAD)):
        fam, _ = GC.wgrad_case(i)
        fam.assert_full()
        req = GB.wgrad_required(fam.grid, fam.strips)
        cells += len(req) * fam.ca
        print(f"[grad-host] coverage {GC.WGRAD[i][0]:34s} {len(req):3d} classes x {fam.ca:2d} channels, fewest impulses in a cell "
              f"{min(fam.table[c][ch] for c in req for ch in range(fam.ca))}")
        per = -(-math.prod(fam.grid) // fam.strips)
        assert all(int((x != 0).sum()) == fam.ca for x in fam.members[:-1])          # one impulse per channel
        few = fam.members[-1].reshape(fam.ca, -1)
        n_few = min(fam.strips + 2, math.prod(fam.grid))
        assert all(int((few[c] != 0).sum()) == n_few for c in range(fam.ca))
        assert all(len({int(o) // per for o in few[c].nonzero()[:, 0]}) == fam.strips for c in range(fam.ca)), "one in each strip"
    for kind, i in GC.FUNC:
        geo, w, b, gfam, xfam, x_dense, g_dense = GC.func_inputs(kind, i)
        gfam.assert_full(), xfam.assert_full()
        cells += sum(len(CB.required_classes(f.spatial, f.seams, f.parities)) * sum(f.cins) for f in (gfam, xfam))
    print(f"[grad-host] coverage: {cells} (class, channel) cells over {len(GC.WGRAD)} + {2 * len(GC.FUNC)} families, none empty")


# ---------------------------------------------------------------------------------------------
# the Functions' cases through torch's own fp32 autograd: the same interval code the GPU file runs
# ---------------------------------------------------------------------------------------------
def _autograd(kind, geo, w, b, x, gy, dtype):
    leaf = lambda v: v.detach().clone().to(dtype).requires_grad_(True)          # noqa: E731
    W, bb, xx = leaf(w), None if b is None else leaf(b), leaf(x)
    y = GC.torch_forward(kind, geo, W, bb, xx)
    y.backward(gy.to(dtype))
    return y.detach(), W.grad, None if bb is None else bb.grad, xx.grad


@pytest.mark.parametrize("kind,i", GC.FUNC, ids=[f"{k}{i}" for k, i in GC.FUNC])
def test_function_cases_torch_fp32_inside_and_coarser_arithmetics_escape(kind, i):
    geo, w, b, gfam, xfam, x_dense, g_dense = GC.func_inputs(kind, i)
    cins, cout, dims, act = list(geo["cins"]), geo["cout"], geo["dims"], geo["act"]
    T = geo["ks"] ** dims
    rep = {}
    # pass F: impulses in
    xb = torch.stack(xfam.members)
    y32, w32, _, _ = _autograd(kind, geo, w, b, xb, g_dense, torch.float32)
    y64, w64, _, _ = _autograd(kind, geo, w, b, xb, g_dense, torch.float64)
    ivf = GC.fwd_interval(kind, geo, xb, w, b)
    assert float((ivf.mid - y64).abs().max()) <= 1e-12 * (1 + float(y64.abs().max()))
    rep["forward"] = CB.check_bounded(f"{kind}{i} forward", y32, *ivf, k_eff=ivf.k_eff, quiet=True)["used"]
    tr = GC.out_padding(kind, geo) if kind == "deconv3d" else None
    if act == "none":
        for mode in ("split", "bf16"):
            assert CB.escapes(CB.emulate(xb, w, b, mode, geo["stride"], geo["pad"], tr, dims), ivf.mid, ivf.half), f"forward in {mode} stays inside"
    if kind == "deconv3d":
        ivw = GC.dw_interval(kind, geo, xb, None, g_dense)
        assert float((ivw.mid - w64.reshape(ivw.mid.shape)).abs().max()) <= 1e-12 * float(ivw.parts[0].max())
        rep["weight"] = CB.check_bounded(f"{kind}{i} weight", w32.reshape(ivw.mid.shape), *ivw, k_eff=ivw.k_eff, quiet=True)["used"]
    # pass I: impulses as the output gradient
    gb = torch.stack(gfam.members)
    y32, w32, b32, x32 = _autograd(kind, geo, w, b, x_dense, gb, torch.float32)
    _, w64, b64, x64 = _autograd(kind, geo, w, b, x_dense, gb, torch.float64)
    gv, ex = GB.act_bwd(gb, y32, act)
    ivx = GC.dx_interval(kind, geo, gv, ex, w)
    scale = 1 + float(x64.abs().max())
    assert float((ivx.mid - x64).abs().max()) <= (1e-12 if act == "none" else 1e-5) * scale        # (y32, not y64, behind an activation)
    rep["input"] = CB.check_bounded(f"{kind}{i} input", x32, *ivx, k_eff=ivx.k_eff, quiet=True)["used"]
    pinned = int((ivx.half == 0).sum())
    for mode in ("split", "bf16"):                                     # the coarser arithmetics leave the fp32 interval on this route
        tr_x = None if kind == "deconv3d" else GC.out_padding(kind, geo)
        assert CB.escapes(CB.emulate(gv.float(), w, None, mode, geo["stride"], geo["pad"], tr_x, dims), ivx.mid, ivx.half), \
            f"{kind}{i}: an input gradient computed in {mode} arithmetic stays inside the fp32 interval"
    if kind != "deconv3d":
        ivw = GC.dw_interval(kind, geo, gv, ex, x_dense)
        if act == "none":
            assert float((ivw.mid - w64.reshape(ivw.mid.shape)).abs().max()) <= 1e-12 * float(ivw.parts[0].max())
        rep["weight"] = CB.check_bounded(f"{kind}{i} weight", w32.reshape(cout, sum(cins), T), *ivw, k_eff=ivw.k_eff, quiet=True)["used"]
    if b is not None:
        ns = GB.reduce_splits(gb.shape[0] * math.prod(geo["yg"]))
        ivb = GB.bias_interval(gv, ns, ex)
        rep["bias"] = CB.check_bounded(f"{kind}{i} bias", b32, *ivb, k_eff=ivb.k_eff, quiet=True)["used"]
        CB.check_bounded(f"{kind}{i} bias restated", GB.restate_channel_sum(gv.float(), ns), *ivb, quiet=True)
    print(f"[grad-host] {kind}{i} {cins}->{cout} {geo['xg']} {act}: members {len(xfam.members)} / {len(gfam.members)}, input gradient pinned to 0: "
          f"{pinned}, K_eff <= {int(ivx.k_eff.max())}; used " + ", ".join(f"{k} {v:.3f}" for k, v in rep.items()))


def test_channel_sum_restated_single_impulse_is_exact():
    g = torch.zeros(3, 5, 37 * 41)
    ns = GB.reduce_splits(g.shape[0] * g.shape[2])
    assert ns == 2
    gen = torch.Generator().manual_seed(1)
    for c in range(5):
        g[c % 3, c, 300 * c + 7] = CB._values(1, gen)[0]
    iv = GB.bias_interval(g, ns)
    assert bool((iv.half == 0).all())
    CB.check_bounded("one impulse per channel", GB.restate_channel_sum(g, ns), *iv, quiet=True)
    CB.check_bounded("torch fp32", g.sum((0, 2)), *iv, quiet=True)


# ---------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------
def rel(got, want):
    want = want.double()
    return float((got.double() - want).abs().max() / (want.abs().max() + 1e-30))


def present_accepts(got, want64, ref32):
    """The rule of tests/test_gpu_train_scale.py: rel(got, fp64) <= max(2e-5, 4 rel(torch fp32, fp64))."""
    return rel(got, want64) <= max(2e-5, 4 * rel(ref32, want64))


def _family_catches(i, hook, hook_source=None, post=None):
    """Runs the mutant restatement over the family of WGRAD[i]; -> (member, worst index) of the first failure, or None."""
    fam, Bs = GC.wgrad_case(i)
    for m, A in enumerate(fam.members):
        iv = _row_interval(i, m)
        got = _restate_row(i, A, None, hook, hook_source)
        if post is not None:
            got = post(got)
        try:
            CB.check_bounded("mutant", got, *iv, quiet=True)
        except CB.OutOfBound as e:
            return m, e.index
    return None


def _dense_wgrad(i, hook, hook_source=None, post=None, B_=4):
    """The present rule on a dense Gaussian input of the row's shape at B = 4 (the k3 row IS the shape of
    test_strip_parallel_weight_gradients): -> accepted?"""
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = GC.WGRAD[i]
    gen = torch.Generator().manual_seed(11 + i)
    ag = GC.a_grid(kd, stride, b_grid)
    got = torch.zeros(ca, sum(cbs), kd * ks * ks)
    want, ref = torch.zeros_like(got, dtype=torch.float64), torch.zeros_like(got)
    for _ in range(B_):
        A = torch.randn(ca, *ag, generator=gen)
        Bs = [torch.randn(cb, *b_grid, generator=gen) for cb in cbs]
        off = 0
        for s, B in enumerate(Bs):
            got = GB.restate_wgrad(A, B, kd, ks, stride, sum(cbs), off, strips, got, hook if hook_source in (None, s) else None)
            off += B.shape[0]
        want += _conv_weight64(A, Bs, kd, ks, stride)
        ref += _conv_weight64(A, Bs, kd, ks, stride, torch.float32)
    if post is not None:
        got = post(got)
    return present_accepts(got, want, ref)


def _k5s2_route(g, W, hin, win, mode="fp32", pxpy=False, overwrite=False):
    """conv2d_k5s2_dgrad_mfma restated: the 3x3 convolution over g whose 4 cin output channels (ci, py, px) are the parity planes
    (pack_k5s2_dgrad_kernel), launches of at most 16 input channels, then the pixel shuffle."""
    cout, cin = W.shape[:2]
    K = torch.zeros(4 * cin, cout, 3, 3)
    for py in range(2):
        for px in range(2):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ky, kx = py + 2 - 2 * dy, px + 2 - 2 * dx
                    if 0 <= ky < 5 and 0 <= kx < 5:
                        cq = 2 * px + py if pxpy else 2 * py + px
                        K[cq::4, :, dy + 1, dx + 1] = W[:, :, ky, kx].t()
    planes = torch.zeros(4 * cin, *g.shape[-2:])
    for c0 in range(0, cin, 16):
        cn = min(16, cin - c0)
        dst = 0 if (overwrite and c0) else 4 * c0
        planes[dst:dst + 4 * cn] = CB.emulate(g, K[4 * c0:4 * (c0 + cn)], None, mode, 1, 1, None, 2)
    return F.pixel_shuffle(planes[None], 2)[0][:, :hin, :win]


MUTANTS = {"1a": "input gradient: products from bf16 hi / lo halves (split arithmetic)", "1b": "weight gradient: products from hi / lo halves",
           "2": "the last position of a ragged strip dropped", "3": "the first position of strip j > 0 counted twice",
           "4": "one corner's padding tap reads the previous row's last pixel", "5": "two taps of one (a, b) pair exchanged",
           "6": "cb_off of the second source ignored", "7": "stride 2: the odd-parity tap taken from the even one",
           "8": "a transposed form's dW written as [cout][cin]", "9a": "dgrad packing without the tap flip",
           "9b": "dgrad packing with the flip but without the in / out swap", "10": "5x5 stride 2: parity planes shuffled as (px, py)",
           "11": "5x5 stride 2: the second launch's channels (16 and up) written over the first's", "12": "bias gradient missing the last split"}


def test_mutants():
    """Each mutant is caught on the impulse family, by the check it is meant to trip; the present rule's verdict on a dense Gaussian
    input is recorded beside it."""
    out = {}
    K1, K3, S2, TR = 0, 1, 8, 12                     # rows of GC.WGRAD: k1 ragged, k3 two sources, 3-D stride 2, transposed
    # 1b: split products in the weight gradient
    hit = _family_catches(K3, {"split": True})
    assert hit is not None
    out["1b"] = (True, _dense_wgrad(K3, {"split": True}))
    # 2: the member that fails holds the failing channel's impulse on the last position
    fam, _ = GC.wgrad_case(K1)
    m, idx = _family_catches(K1, {"drop_last_of_ragged": True})
    assert fam.members[m].reshape(fam.ca, -1)[idx[0], -1] != 0
    out["2"] = (True, _dense_wgrad(K1, {"drop_last_of_ragged": True}))
    # 3: ... on the first position of a strip j > 0
    m, idx = _family_catches(K1, {"double_first_of_strip": True})
    per = -(-math.prod(fam.grid) // fam.strips)
    o = int(fam.members[m].reshape(fam.ca, -1)[idx[0]].nonzero()[0, 0])
    assert o % per == 0 and o > 0
    out["3"] = (True, _dense_wgrad(K1, {"double_first_of_strip": True}))
    # 4: ... on the corner (last row, x = 0), at a tap with kx = 0
    fam3, _ = GC.wgrad_case(K3)
    m, idx = _family_catches(K3, {"corner_reads_previous_row": True})
    o = int(fam3.members[m].reshape(fam3.ca, -1)[idx[0]].nonzero()[0, 0])
    assert o == (fam3.grid[1] - 1) * fam3.grid[2] and idx[2] % 3 == 0
    out["4"] = (True, _dense_wgrad(K3, {"corner_reads_previous_row": True}))
    # 5
    m, idx = _family_catches(K3, {"swap_taps": (5, 2, 3, 4)}, hook_source=0)
    assert idx[:2] == (5, 2) and idx[2] in (3, 4)
    out["5"] = (True, _dense_wgrad(K3, {"swap_taps": (5, 2, 3, 4)}, hook_source=0))
    # 6: the second source's block lands on the first's
    m, idx = _family_catches(K3, {"ignore_cb_off": True}, hook_source=1)
    assert idx[1] < 5 or idx[1] >= 16
    out["6"] = (True, _dense_wgrad(K3, {"ignore_cb_off": True}, hook_source=1))
    # 7: 3-D stride 2: tap kx = 1 (odd parity of B's column) reads what kx = 0 reads ... of the same position
    perm = [t_ if t_ % 3 != 1 else t_ - 1 for t_ in range(27)]
    m, idx = _family_catches(S2, {"parity_tap": perm})
    assert idx[2] % 3 == 1
    out["7"] = (True, _dense_wgrad(S2, {"parity_tap": perm}, B_=1))
    # 8
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = GC.WGRAD[TR]
    post = lambda d: d.transpose(0, 1).reshape(d.shape)          # noqa: E731
    assert _family_catches(TR, None, post=post) is not None
    out["8"] = (True, _dense_wgrad(TR, None, post=post, B_=1))
    # ---- input-gradient routes: a square 3x3 case (12 -> 12) so that the un-swapped weight has a valid shape
    gen = torch.Generator().manual_seed(5)
    w = CB.he_weights((12, 12, 3, 3), 108, gen)
    gfam = GC.CC.family((12,), (21, 28), 1, GC.CC.fam_key(GC.DGRAD2D_TILES), seed=3)
    gfam.assert_full()
    gb = torch.stack(gfam.members)
    dense = torch.randn(4, 12, 48, 63, generator=gen)
    geo = dict(stride=(1, 1), pad=1, dims=2, ks=3, yg=(21, 28), xg=(21, 28))
    ivx = GC.dx_interval("conv2d", geo, gb, None, w)
    want = CB.linear(dense, w, (1, 1), (1, 1), (0, 0), 2)
    ref = F.conv_transpose2d(dense, w, None, padding=1)
    forms = {"1a": lambda g, mode="split": CB.emulate(g, w.flip(2, 3).transpose(0, 1), None, mode),
             "9a": lambda g: CB.emulate(g, w.transpose(0, 1), None, "fp32"), "9b": lambda g: CB.emulate(g, w.flip(2, 3), None, "fp32")}
    CB.check_bounded("the dgrad packing restated", CB.emulate(gb, w.flip(2, 3).transpose(0, 1), None, "fp32"), *ivx, quiet=True)
    for k, fn in forms.items():
        assert CB.escapes(fn(gb), ivx.mid, ivx.half), k
        out[k] = (True, present_accepts(fn(dense), want, ref))
    # ---- 5x5 stride 2, cin 20 on 31 x 45
    geo5, w5, _, gfam5, _, _, _ = GC.func_inputs("k5s2", 2)
    gb5 = torch.stack(gfam5.members)
    iv5 = GC.dx_interval("k5s2", geo5, gb5, None, w5)
    route = lambda g, **kw: torch.stack([_k5s2_route(gm, w5, *geo5["xg"], **kw) for gm in g])          # noqa: E731
    CB.check_bounded("the parity-plane route restated", route(gb5), *iv5, quiet=True)
    assert CB.escapes(route(gb5, mode="split"), iv5.mid, iv5.half)
    dense5 = torch.randn(2, geo5["cout"], *geo5["yg"], generator=gen)
    want5 = CB.linear(dense5, w5, (2, 2), (2, 2), GC.out_padding("k5s2", geo5), 2)
    ref5 = F.conv_transpose2d(dense5, w5, None, stride=2, padding=2, output_padding=GC.out_padding("k5s2", geo5))
    for k, kw in (("10", {"pxpy": True}), ("11", {"overwrite": True})):
        assert CB.escapes(route(gb5, **kw), iv5.mid, iv5.half), k
        out[k] = (True, present_accepts(route(dense5, **kw), want5, ref5))
    # ---- 12: the bias gradient of the first conv2d case (13 splits)
    geo2, w2, b2, gfam2, _, _, _ = GC.func_inputs("conv2d", 0)
    g2 = torch.stack(gfam2.members)
    ns = GB.reduce_splits(g2.shape[0] * math.prod(geo2["yg"]))
    assert ns > 1
    ivb = GB.bias_interval(g2, ns)
    CB.check_bounded("channel_sum restated", GB.restate_channel_sum(g2, ns), *ivb, quiet=True)
    assert CB.escapes(GB.restate_channel_sum(g2, ns, drop_last_split=True), ivb.mid, ivb.half)
    d2 = torch.randn(4, 12, 48, 63, generator=gen)
    nsd = GB.reduce_splits(4 * 48 * 63)
    out["12"] = (True, present_accepts(GB.restate_channel_sum(d2, nsd, drop_last_split=True), d2.double().sum((0, 2, 3)), d2.sum((0, 2, 3))))
    for k, (caught, acc) in out.items():
        print(f"[grad-mutant] {k:3s} {MUTANTS[k]:78s} impulse check: {'caught' if caught else 'MISSED'}   present rule: {'ACCEPTS' if acc else 'rejects'}")
    assert set(out) == set(MUTANTS)
    assert out["1a"][1] and out["1b"][1], "the present rule was measured to accept products formed from bf16 halves"
