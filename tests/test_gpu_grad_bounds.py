"""GPU: the convolutions' backward on impulse inputs (tests/grad_bound.py, tests/grad_cases.py).

1. ``ops.conv_wgrad`` directly, every ``wgrad_nd_kernel`` instantiation: A holds one impulse per channel (every channel on every
   position class: corners / edges / faces of the grid, the last position before and the first of every strip, the last position,
   lanes 0 / 63 / 64 / 255 of a workgroup's stride and a thread's second trip), B is dense, so every element of dW is ONE product and
   is pinned bit for bit to RN(a b) -- or to exactly 0 where the tap lands in the padding.  A "few products" member and a dW that
   already holds values exercise the sums.
2. The autograd Functions through ``.backward()`` with the impulse family's members as the batch: weight, bias and every input
   gradient, the launch keys of the input-gradient route asserted.
3. Each Function case under every ``ops.set_precision``: the gradients and the forward outputs stay inside the fp32 interval
   (tests/test_grad_bound_host.py shows that the split and bf16 arithmetics leave it on these inputs).
EVERY element is checked; nothing is left out.  The table of section 2.5 is what the module's last lines print (run with -s)."""
import math

import pytest
import torch

import conv_bound as CB
import grad_bound as GB
import grad_cases as GC
from common import t
from test_gpu_conv_bounds import launch, precision_
from test_gpu_train_scale import launch_shape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLE = {}          # row -> [checks, largest share used, elements pinned to 0 / the prior, elements pinned to RN(a b), elements]
KEYS = {}


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\n[grad-table] family | checks | largest share of the interval used | pinned to 0 or the prior | pinned to RN(ab) | elements | launch keys")
    for row, (n, used, p0, p1, total) in TABLE.items():
        print(f"[grad-table] {row} | {n} | {used:.3f} | {p0} | {p1} | {total} | {' '.join(sorted(KEYS.get(row.split(' | ')[0], ())))}")


def bounded(row, name, got, iv):
    rep = CB.check_bounded(name, got, iv.mid, iv.half, k_eff=iv.k_eff, quiet=True)
    r = TABLE.setdefault(row, [0, 0.0, 0, 0, 0])
    r[0] += 1
    r[1] = max(r[1], rep["used"])
    if iv.k_eff is not None and iv.k_eff.shape == iv.half.shape:
        r[2] += int(((iv.half == 0) & (iv.k_eff == 0)).sum())
        r[3] += int(((iv.half == 0) & (iv.k_eff >= 1)).sum())
    else:
        r[2] += rep["pinned"]
    r[4] += rep["checked"]
    return rep


# ---------------------------------------------------------------------------------------------
# 1. ops.conv_wgrad on every row of the table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(GC.WGRAD)), ids=GC.wgrad_ids())
def test_wgrad_every_element_is_one_product(i):
    from effi_mvs_plus_amd import ops
    row = GC.WGRAD[i]
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = row
    assert GC.strips_of(row, launch_shape) == strips
    fam, Bs = GC.wgrad_case(i)
    fam.assert_full()
    assert fam.strips == strips
    cb_total, T, L = sum(cbs), kd * ks * ks, len(fam.members)
    Bd = [t(GC.squeeze2d(B, kd), DEV) for B in Bs]
    gen = torch.Generator().manual_seed(i)
    prior = CB._values(ca * cb_total * T, gen).view(ca, cb_total, T)
    with_prior = [i % (L - 1), fam.few]
    dws = torch.zeros(L + len(with_prior), ca, cb_total, T, device=DEV)
    for k, m in enumerate(with_prior):
        dws[L + k] = prior.to(DEV)
    for slot, m in list(enumerate(range(L))) + [(L + k, m) for k, m in enumerate(with_prior)]:
        Ad, off = t(GC.squeeze2d(fam.members[m], kd), DEV), 0
        for B in Bd:
            ops.conv_wgrad(Ad, B, dws[slot], off, kd, ks, stride=stride)
            off += B.shape[0]
    got = dws.cpu()
    kind = f"conv_wgrad k{kd}x{ks} stride {stride}"
    for slot, m in list(enumerate(range(L))) + [(L + k, m) for k, m in enumerate(with_prior)]:
        terms, off = [], 0
        for B in Bs:
            terms.append(GB.wgrad_terms(fam.members[m], B, kd, ks, stride, cb_total, off))
            off += B.shape[0]
        iv = GB.wgrad_finish(terms, prior if slot >= L else None, strips=strips)
        if m != fam.few and slot < L:
            assert int(iv.k_eff.max()) == 1 and bool((iv.half == 0).all()), "an impulse member pins every element"
        sub = kind if (m != fam.few and slot < L) else kind + ": few products / onto a prior"
        bounded(sub, f"{name} member {m}{' onto a prior' if slot >= L else ''}", got[slot], iv)


# ---------------------------------------------------------------------------------------------
# the bias gradient alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,grid", [(1, 7, (12, 25)), (3, 5, (37, 41)), (4, 3, (64, 80))])
def test_channel_sum_one_impulse_is_exact(B, C, grid):
    from effi_mvs_plus_amd import ops
    n = math.prod(grid)
    ns = launch_shape("reduce", B=B, n=n)
    assert ns == GB.reduce_splits(B * n) and (ns > 1) == (B * n >= 4096)
    per = -(-(B * n) // ns)
    spots = sorted({0, B * n - 1, n - 1, n % (B * n)} | {j * per for j in range(ns)} | {j * per - 1 for j in range(1, ns)})
    gen = torch.Generator().manual_seed(B * C)
    for k in range(len(spots)):                                       # channel c on spot (k + c): every channel on every spot
        g = torch.zeros(B, C, n)
        for c in range(C):
            s = spots[(k + c) % len(spots)]
            g[s // n, c, s % n] = CB._values(1, gen)[0]
        iv = GB.bias_interval(g, ns)
        assert bool((iv.half == 0).all())
        bounded("channel_sum", f"channel_sum {B}x{C}x{grid} member {k}", ops.channel_sum(t(g.view(B, C, *grid), DEV)), iv)
    g = torch.zeros(B, C, n)                                          # n impulses: one per split and two more
    for c in range(C):
        idx = torch.tensor([j * per + (5 * c + 1) % min(per, 200) for j in range(ns)] + [B * n - 1 - c, (B * n) // 2 + c])
        for s in idx.tolist():
            g[s // n, c, s % n] = CB._values(1, gen)[0]
    bounded("channel_sum: a few values", f"channel_sum {B}x{C}x{grid} few", ops.channel_sum(t(g.view(B, C, *grid), DEV)), GB.bias_interval(g, ns))


# ---------------------------------------------------------------------------------------------
# 2. + 3. the autograd Functions, under every precision
# ---------------------------------------------------------------------------------------------
_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _apply(kind, i, W, b, xs):
    from effi_mvs_plus_amd import autograd as A, ops
    geo = GC.func_geometry(kind, i)
    if kind == "conv2d":
        code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "tanh": ops.ACT_TANH}[geo["act"]]
        return A.conv2d(xs, W, b, code)
    if kind == "k5s2":
        return A.conv2d_k5s2(xs[0], W)
    if kind == "conv3d":
        return A.conv3d(xs, W, geo["stride"])
    return A.deconv3d(xs[0], W, geo["stride"])


def _keys(kind, geo):
    """(forward key, [input-gradient keys]) per sample."""
    cin, cout, st = sum(geo["cins"]), geo["cout"], geo["stride"]
    nt = lambda c: (c + 15) // 16          # noqa: E731
    c81 = lambda c: "8" if c % 8 == 0 else "1"          # noqa: E731
    if kind == "conv2d":
        return f"conv2d_k{geo['ks']}_nt{nt(cout)}_epi0", [f"conv2d_k{geo['ks']}_nt{nt(cin)}_epi0"]
    if kind == "k5s2":
        return f"conv2d_k5s2_nt{nt(cout)}", [f"conv2d_k3_nt{nt(4 * min(16, cin - c0))}_epi0" for c0 in range(0, cin, 16)]
    if kind == "conv3d":
        fwd = f"conv3d_c{c81(cout)}_s{st[0]}{st[1]}"
        return fwd, ([f"conv3d_c{c81(cin)}_s11"] if st == (1, 1, 1) else [f"deconv3d_c{1 if cin == 1 else 8}_s{st[0]}"])
    return f"deconv3d_c{1 if cout == 1 else 8}_s{st[0]}", [f"conv3d_c{c81(cin)}_s{st[0]}{st[1]}"]


@pytest.mark.parametrize("mode", ["split", "fp32", "bf16"])
@pytest.mark.parametrize("kind,i", GC.FUNC, ids=[f"{k}{i}" for k, i in GC.FUNC])
def test_function_gradients_bounded_in_every_precision(kind, i, mode):
    from effi_mvs_plus_amd import ops
    geo, w, b, gfam, xfam, x_dense, g_dense = GC.func_inputs(kind, i)
    gfam.assert_full(), xfam.assert_full()
    fwd_key, dx_keys = _keys(kind, geo)
    cins, cout, dims, act = list(geo["cins"]), geo["cout"], geo["dims"], geo["act"]
    ks, T = geo["ks"], geo["ks"] ** dims
    row = f"{kind}{i} {cins}->{cout} k{ks} s{geo['stride']} {geo['xg']} {act}"
    KEYS.setdefault(row, set()).update([fwd_key] + dx_keys)
    leaf = lambda v: t(v, DEV).requires_grad_(True)          # noqa: E731
    with precision_(mode):
        # ---- pass F: the input is the impulse family: the forward output, sharp; the transposed form's weight gradient (A = the input)
        xb = torch.stack(xfam.members)
        Mx = xb.shape[0]
        W = leaf(w)
        bd = None if b is None else t(b, DEV)
        y = launch([fwd_key] * Mx, lambda: _apply(kind, i, W, bd, [t(s, DEV) for s in torch.split(xb, cins, 1)]))
        bounded(row + " | forward", f"{row} forward on impulses", y, memo((kind, i, "F"), lambda: GC.fwd_interval(kind, geo, xb, w, b)))
        if kind == "deconv3d":
            launch([], lambda: y.backward(t(g_dense, DEV)))
            iv = memo((kind, i, "FW"), lambda: GC.dw_interval(kind, geo, xb, None, g_dense))
            bounded(row + " | weight", f"{row} weight gradient", W.grad.view(cins[0], cout, 27), iv)
        # ---- pass I: the output gradient is the impulse family, the input dense
        gb = torch.stack(gfam.members)
        M = gb.shape[0]
        W = leaf(w) if kind != "deconv3d" else t(w, DEV)
        bl = None if b is None else leaf(b)
        xs = [leaf(s) for s in torch.split(x_dense, cins, 1)]
        y = launch([fwd_key] * M, lambda: _apply(kind, i, W, bl, xs))
        bounded(row + " | forward", f"{row} forward on a dense input", y, memo((kind, i, "Fd"), lambda: GC.fwd_interval(kind, geo, x_dense, w, b)))
        launch(dx_keys * M, lambda: y.backward(t(gb, DEV)))
        gv, ex = GB.act_bwd(gb, y, act)
        fixed = act == "none"                                           # the intervals do not depend on the run's own y
        iv = memo((kind, i, "dx"), lambda: GC.dx_interval(kind, geo, gv, ex, w)) if fixed else GC.dx_interval(kind, geo, gv, ex, w)
        assert ex is not None or int(iv.k_eff.max()) <= 1, "two impulses reach one element of the input gradient"
        off = 0
        for s, x in enumerate(xs):
            c = x.shape[1]
            sl = CB.Interval(iv.mid[:, off:off + c], iv.half[:, off:off + c], iv.k_eff[:, off:off + c])
            bounded(row + " | input", f"{row} input gradient, source {s}", x.grad, sl)
            off += c
        if kind == "k5s2":                                               # the direct vector form on the same members, same intervals
            direct = torch.stack([ops.conv2d_k5s2_dgrad(t(gb[m], DEV), t(w, DEV), *geo["xg"]) for m in range(M)])
            bounded(row + " | input, direct kernel", f"{row} conv2d_k5s2_dgrad", direct, iv)
        if kind != "deconv3d":
            wiv = lambda: GC.dw_interval(kind, geo, gv, ex, x_dense)          # noqa: E731
            bounded(row + " | weight", f"{row} weight gradient", W.grad.view(cout, sum(cins), T), memo((kind, i, "W"), wiv) if fixed else wiv())
        if bl is not None:
            ns = launch_shape("reduce", B=M, n=math.prod(geo["yg"]))
            bounded(row + " | bias", f"{row} bias gradient", bl.grad, GB.bias_interval(gv, ns, ex))
