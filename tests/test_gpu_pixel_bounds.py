"""GPU: every element of the per-pixel training kernels and of BatchNorm inside its float64 interval (tests/pixel_bound.py,
DESIGN.md section 2.6).

The kernels: bn_moment / bn_apply / bn_bwd_reduce / bn_bwd_apply, softargmin_bwd, view_aggregate and its backward, convex_upsample2x
(the ``inv`` output), its backward and gather, and every op of pointwise_kernel -- through the product's own wrappers, the
sample-batched ones through the ``autograd`` Functions with B = 2 (sample 1 has inputs of its own, so a wrong sample stride shows).
The cases are those of tests/test_pixel_bound_host.py, which proves the reference on the CPU: the smallest shapes at which the kernels'
forms change.  Every element goes through ``check_bounded``: none is left out, and a pinned element is compared bit for bit.  The table
of DESIGN.md section 2.6 is what the module's last lines print (run with -s)."""
import contextlib
import math

import pytest
import torch

import pixel_bound as PB
from conv_bound import check_bounded
from test_gpu_train_scale import launch_shape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TABLE = {}          # family -> [checks, largest share used, pinned elements, elements, widest half / |mid|]


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\n[pixel-table] family | checks | largest share of the interval used | exactly pinned elements | elements | widest half / |mid|")
    for row, (n, used, pinned, total, wide) in TABLE.items():
        print(f"[pixel-table] {row} | {n} | {used:.3f} | {pinned} | {total} | {wide:.3e}")


def bounded(row, name, got, iv):
    rep = check_bounded(name, got, iv.mid, iv.half, quiet=True)
    r = TABLE.setdefault(row, [0, 0.0, 0, 0, 0.0])
    r[0] += 1
    r[1] = max(r[1], rep["used"])
    r[2] += rep["pinned"]
    r[3] += rep["checked"]
    r[4] = max(r[4], PB.widest_relative(iv))
    return rep


def dev(x):
    return x.to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape,chunk,kind", PB.BN_CASES)
def test_batch_norm_every_element_bounded(shape, chunk, kind, relu):
    from effi_mvs_plus_amd import ops
    x, gy, par = PB.bn_inputs(shape, kind, seed=(chunk or 0) + sum(shape))
    B, n = shape[0], math.prod(shape[2:])
    with (ops.options(reduce_chunk=chunk) if chunk is not None else contextlib.nullcontext()):
        ns = launch_shape("reduce", B=B, n=n)
        assert ns == ops._reduce_split(B * n, 1)[1]
        if chunk is not None:
            assert ns > 1
        if shape == (2, 4, 40, 52):
            assert ns == 2
        d = {k: dev(v) for k, v in par.items()}
        nt = torch.tensor(5, dtype=torch.int64, device=DEV)
        xd, gyd = dev(x), dev(gy)
        y, mean, invstd = ops.bn_train_fwd(xd, d["weight"], d["bias"], 1e-5, 0.1, d["running_mean"], d["running_var"], nt, relu)
        gx, s1, s2 = ops.bn_bwd(gyd, y, xd, mean, invstd, d["weight"], relu)
        torch.cuda.synchronize()
    name = f"bn {shape} chunk={chunk} {kind} relu={relu} ns={ns}"
    fwd = PB.bn_fwd_interval(x, par["weight"], par["bias"], par["running_mean"], par["running_var"], 1e-5, 0.1, relu, ns)
    got = dict(y=y, mean=mean, invstd=invstd, rm=d["running_mean"], rv=d["running_var"])
    for k in ("y", "mean", "invstd", "rm", "rv"):
        bounded("batch norm forward", f"{name} {k}", got[k], fwd[k])
    assert int(nt) == 6                                             # the counter advanced by exactly one
    # the backward's reference takes the HIP forward's own y (the mask), mean and invstd: its inputs
    bwd = PB.bn_bwd_interval(gy, y.cpu(), x, mean.cpu(), invstd.cpu(), par["weight"], relu, ns)
    for k, v in (("gx", gx), ("s1", s1), ("s2", s2)):
        rep = bounded("batch norm backward", f"{name} {k}", v, bwd[k])
        if kind == "planted" and relu and k == "gx":
            assert rep["pinned"] == y[:, 0].numel() and bool((y[:, 0] == 0).all())


# ---------------------------------------------------------------------------------------------
# soft-argmin backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PB.SAM_CASES)))
def test_softargmin_bwd_every_element_bounded(i):
    from effi_mvs_plus_amd import autograd as A
    D, hw, hk, lk = PB.SAM_CASES[i]
    logits, hyp, g = PB.sam_inputs(D, hw, hk, lk, seed=100 + i)
    leaf = dev(logits).requires_grad_(True)
    depth, _ = A.soft_argmin(leaf, dev(hyp))
    depth.backward(dev(g))
    torch.cuda.synchronize()
    for b in range(logits.shape[0]):
        rep = bounded("soft-argmin backward", f"softargmin_bwd D={D} {hw} {hk} {lk} sample {b}", leaf.grad[b],
                      PB.softargmin_bwd_interval(logits[b], hyp[b], g[b]))
        assert (rep["pinned"] == rep["checked"]) == (D == 1)


# ---------------------------------------------------------------------------------------------
# view aggregate
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PB.VA_CASES)))
def test_view_aggregate_every_element_bounded(i):
    from effi_mvs_plus_amd import autograd as A
    from effi_mvs_plus_amd import ops
    S, D, hw, kind = PB.VA_CASES[i]
    sim, wts, g = PB.va_inputs(S, D, hw, kind, seed=200 + i)
    ls, lw = dev(sim).requires_grad_(True), dev(wts).requires_grad_(True)
    out = A.view_aggregate(ls, lw)
    out.backward(dev(g))
    plain = ops.view_aggregate(dev(sim), None)                      # weights None: one sample-batched launch
    torch.cuda.synchronize()
    name = f"view_aggregate S={S} D={D} {hw} {kind}"
    for b in range(sim.shape[0]):
        bounded("view aggregate forward", f"{name} sample {b}", out[b], PB.view_aggregate_interval(sim[b], wts[b]))
        rep = bounded("view aggregate forward", f"{name} sample {b} no weights", plain[b], PB.view_aggregate_interval(sim[b], None))
        assert (rep["pinned"] == rep["checked"]) == (S == 1)
        igs, igw = PB.view_aggregate_bwd_interval(sim[b], wts[b], g[b])
        rep = bounded("view aggregate backward", f"{name} sample {b} gsim", ls.grad[b], igs)
        bounded("view aggregate backward", f"{name} sample {b} gw", lw.grad[b], igw)
        if kind == "zero":
            assert rep["pinned"] == D * hw[0] * hw[1]


# ---------------------------------------------------------------------------------------------
# convex upsampling
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PB.CU_CASES)))
def test_convex_upsample_every_element_bounded(i):
    from effi_mvs_plus_amd import autograd as A
    hw, mk, gk = PB.CU_CASES[i]
    h, w = hw
    inv, mask, gup = PB.cu_inputs(hw, mk, gk, seed=300 + i)
    li, lm = dev(inv).requires_grad_(True), dev(mask).requires_grad_(True)
    up = A.convex_upsample(li, lm)
    up.backward(dev(gup))
    torch.cuda.synchronize()
    name = f"convex_upsample2x {hw} mask={mk} gup={gk}"
    for b in range(inv.shape[0]):
        bounded("convex upsample forward", f"{name} sample {b} inv", up[b], PB.convex_up_interval(inv[b, 0], mask[b]))
        igm, igi = PB.convex_up_bwd_interval(inv[b, 0], mask[b], gup[b])
        bounded("convex upsample backward", f"{name} sample {b} gmask", lm.grad[b], igm)
        rep = bounded("convex upsample backward", f"{name} sample {b} ginv", li.grad[b, 0], igi)
        if gk == "corners":
            assert rep["pinned"] == h * w - 16


# ---------------------------------------------------------------------------------------------
# pointwise
# ---------------------------------------------------------------------------------------------
def _pw(op, kw, n_out):
    from effi_mvs_plus_amd import ops
    args = {k: (dev(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    got = ops.pointwise(PB.PW_OPS.index(op), n_out=n_out, **args)
    torch.cuda.synchronize()
    return [got] if n_out == 1 else got


@pytest.mark.parametrize("n", PB.PW_NS)
def test_pointwise_every_element_bounded(n):
    t_ = PB.pw_inputs(n, seed=400 + n)
    for op, kw, n_out in PB.pw_calls(t_, n):
        got, ivs = _pw(op, kw, n_out), PB.pw_interval(op, **kw)
        assert len(got) == len(ivs) == n_out
        for k in range(n_out):
            bounded("pointwise", f"pointwise {op} n={n} {kw.get('inner', '')} {kw.get('C', '')} out {k}", got[k], ivs[k])


def test_pointwise_through_the_autograd_functions():
    """The same ops as the training path reaches them (autograd._Act, _Mul, _GruCombine, _InvToDepth, _ScaleChannels), [B,C,h,w] with
    B = 2."""
    from effi_mvs_plus_amd import autograd as A
    from effi_mvs_plus_amd import ops
    B, C, h, w = 2, 5, 7, 11
    t_ = {k: v.view(B, C, h, w) for k, v in PB.pw_inputs(B * C * h * w, seed=77).items()}
    lo, hi = PB.PW_RANGE
    row = "pointwise (autograd)"
    for act, name, yk in ((ops.ACT_TANH, "tanh", "y_tanh"), (ops.ACT_RELU, "relu", "y_relu"), (ops.ACT_SIGMOID, "sigmoid", "y_sig")):
        leaf = dev(t_["x"]).requires_grad_(True)
        y = A.activation(leaf, act)
        y.backward(dev(t_["g"]))
        bounded(row, f"activation {name}", y, PB.pw_interval(name, a=t_["x"])[0])
        bounded(row, f"activation {name} backward", leaf.grad, PB.pw_interval("act_bwd_" + name, a=t_["g"], b=y.detach().cpu())[0])
    z, hh, q = (dev(t_[k]).requires_grad_(True) for k in ("z", "h", "q"))
    out = A._GruCombine.apply(z, hh, q)
    out.backward(dev(t_["g"]))
    bounded(row, "gru", out, PB.pw_interval("gru", a=t_["z"], b=t_["h"], c=t_["q"])[0])
    for k, (got, iv) in enumerate(zip((z.grad, hh.grad, q.grad), PB.pw_interval("gru_bwd", a=t_["g"], b=t_["z"], c=t_["h"], d=t_["q"]))):
        bounded(row, f"gru backward out {k}", got, iv)
    a, b = dev(t_["x"]).requires_grad_(True), dev(t_["x2"]).requires_grad_(True)
    out = A._Mul.apply(a, b)
    out.backward(dev(t_["g"]))
    bounded(row, "mul", out, PB.pw_interval("mul", a=t_["x"], b=t_["x2"])[0])
    for k, (got, iv) in enumerate(zip((a.grad, b.grad), PB.pw_interval("mul_bwd", a=t_["g"], b=t_["x"], c=t_["x2"]))):
        bounded(row, f"mul backward out {k}", got, iv)
    inv = dev(t_["inv"]).requires_grad_(True)
    out = A.inv_to_depth(inv, lo, hi)
    out.backward(dev(t_["g"]))
    bounded(row, "inv_to_depth", out, PB.pw_interval("inv_to_depth", a=t_["inv"], s0=lo, s1=hi)[0])
    bounded(row, "inv_to_depth backward", inv.grad, PB.pw_interval("inv_to_depth_bwd", a=t_["g"], b=t_["inv"], s0=lo, s1=hi)[0])
    f = torch.linspace(0.5, 2.5, B * C) * 1.0000001
    xs = dev(t_["x"]).requires_grad_(True)
    out = A._ScaleChannels.apply(xs, dev(f))
    out.backward(dev(t_["g"]))
    bounded(row, "scale channels", out, PB.pw_interval("scale_ch", a=t_["x"], b=f, inner=h * w, C=B * C)[0])
    bounded(row, "scale channels backward", xs.grad, PB.pw_interval("scale_ch", a=t_["g"], b=f, inner=h * w, C=B * C)[0])


def test_inv_to_depth_on_the_clamps_threshold():
    """inv = 0 with a ``lo`` whose min_disp is exactly 1e-4f: s sits ON the threshold, the forward is 1 / 1e-4f and the backward 0, both
    pinned (s > 1e-4f is false there)."""
    lo = PB.clamp_edge_lo()
    t_ = PB.pw_inputs(257, seed=400 + 257)
    inv = t_["inv"].clone()
    inv[::5] = 0.0
    hi = PB.PW_RANGE[1]
    iv = PB.pw_interval("inv_to_depth_bwd", a=t_["g"], b=inv, s0=lo, s1=hi)[0]
    assert bool((iv.half[::5] == 0).all())
    bounded("pointwise", "inv_to_depth_bwd on the threshold", _pw("inv_to_depth_bwd", dict(a=t_["g"], b=inv, s0=lo, s1=hi), 1)[0], iv)
    bounded("pointwise", "inv_to_depth on the threshold", _pw("inv_to_depth", dict(a=inv, s0=lo, s1=hi), 1)[0],
            PB.pw_interval("inv_to_depth", a=inv, s0=lo, s1=hi)[0])
