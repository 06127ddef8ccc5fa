"""The families of tests/test_gpu_grad_bounds.py, shared with tests/test_grad_bound_host.py.  CPU only.

WGRAD: one row per direct ``ops.conv_wgrad`` case: (name, kd, ks, (sz, sxy), ca, sources of B, B's grid (D, h, w), strips, ragged).
A lives on the small grid ((n - 1) // s + 1 per strided axis).  For a convolution A = the output gradient and B = the input; for
the transposed rows A = the input and B = the output gradient (dW [cin][cout][27]): the same launch with the roles swapped.  Every
case asserts its number of strips through ``launch_shape("wgrad", ...)`` (tests/test_gpu_train_scale.py).

FUNC: the autograd Functions with the impulse family's members as the batch dimension."""
import functools
import math

import torch

import conv_bound as CB
import conv_cases as CC
import grad_bound as GB

# (name, kd, ks, stride, ca, cbs, b_grid, strips, ragged)
WGRAD = [
    ("k1 20<-6, 4 ragged strips", 1, 1, (1, 1), 20, (6,), (1, 45, 101), 4, True),
    ("k3 12<-(16,5), cb_off 16", 1, 3, (1, 1), 12, (16, 5), (1, 48, 63), 2, False),
    ("k3 16<-1", 1, 3, (1, 1), 16, (1,), (1, 17, 24), 1, False),
    ("k3 1<-8", 1, 3, (1, 1), 1, (8,), (1, 17, 24), 1, False),
    ("k5 stride 2 16<-3, odd input", 1, 5, (1, 2), 16, (3,), (1, 95, 131), 2, False),
    ("k7 16<-1", 1, 7, (1, 1), 16, (1,), (1, 50, 64), 2, False),
    ("3-D s111 1<-(8,8), cb_off 8", 3, 3, (1, 1), 1, (8, 8), (5, 20, 28), 2, False),
    ("3-D s111 8<-1", 3, 3, (1, 1), 8, (1,), (5, 20, 28), 2, False),
    ("3-D s222 16<-8", 3, 3, (2, 2), 16, (8,), (8, 48, 56), 2, False),
    ("3-D s222 8<-1", 3, 3, (2, 2), 8, (1,), (8, 48, 56), 2, False),
    ("3-D s122 16<-8", 3, 3, (1, 2), 16, (8,), (8, 48, 56), 4, False),
    ("3-D s122 8<-1", 3, 3, (1, 2), 8, (1,), (8, 48, 56), 4, False),
    ("transposed s222 16->8", 3, 3, (2, 2), 16, (8,), (8, 48, 56), 2, False),
    ("transposed s222 8->1", 3, 3, (2, 2), 8, (1,), (8, 48, 56), 2, False),
    ("transposed s122 16->8", 3, 3, (1, 2), 16, (8,), (4, 48, 56), 2, False),
    ("transposed s122 8->1", 3, 3, (1, 2), 8, (1,), (4, 48, 56), 2, False),
    # every row once more with D = 1, or h or w = 1: the "only" border class
    ("k1 h=1", 1, 1, (1, 1), 20, (6,), (1, 1, 101), 1, False),
    ("k3 12<-(16,5) w=1", 1, 3, (1, 1), 12, (16, 5), (1, 48, 1), 1, False),
    ("k3 16<-1 h=1", 1, 3, (1, 1), 16, (1,), (1, 1, 24), 1, False),
    ("k3 1<-8 w=1", 1, 3, (1, 1), 1, (8,), (1, 17, 1), 1, False),
    ("k5 stride 2 h=1", 1, 5, (1, 2), 16, (3,), (1, 1, 131), 1, False),
    ("k7 w=1", 1, 7, (1, 1), 16, (1,), (1, 50, 1), 1, False),
    ("3-D s111 1<-(8,8) D=1", 3, 3, (1, 1), 1, (8, 8), (1, 20, 28), 1, False),
    ("3-D s111 8<-1 h=1", 3, 3, (1, 1), 8, (1,), (5, 1, 28), 1, False),
    ("3-D s222 16<-8 D=1", 3, 3, (2, 2), 16, (8,), (1, 48, 56), 1, False),
    ("3-D s222 8<-1 w=1", 3, 3, (2, 2), 8, (1,), (8, 48, 1), 1, False),
    ("3-D s122 16<-8 D=1", 3, 3, (1, 2), 16, (8,), (1, 48, 56), 1, False),
    ("3-D s122 8<-1 h=1", 3, 3, (1, 2), 8, (1,), (8, 1, 56), 1, False),
    ("transposed s222 16->8 D=1", 3, 3, (2, 2), 16, (8,), (2, 48, 56), 1, False),
    ("transposed s122 8->1 D=1", 3, 3, (1, 2), 8, (1,), (1, 48, 56), 1, False),
]


def wgrad_ids():
    """Test ids of the rows: letters, digits, '-' and '_' only."""
    import re
    return [re.sub(r"[^A-Za-z0-9]+", "_", r[0].replace("<-", " from ").replace("->", " to ")).strip("_") for r in WGRAD]


def a_grid(kd, stride, b_grid):
    sz, sxy = stride
    return ((b_grid[0] - 1) // sz + 1 if kd == 3 else b_grid[0], (b_grid[1] - 1) // sxy + 1, (b_grid[2] - 1) // sxy + 1)


def strips_of(row, launch_shape):
    """The strips ``launch_shape`` reports for every source's launch of a row (the sources of a row share one number); asserts the
    regime the row is named for."""
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = row
    na = math.prod(a_grid(kd, stride, b_grid))
    got = {launch_shape("wgrad", ca=ca, cb=cb, na=na, kd=kd, ks=ks) for cb in cbs}
    assert got == {strips}, f"{name}: the library launches {got} strips, the case is written for {strips}"
    assert not ragged or na % strips != 0, f"{name}: {na} positions in {strips} strips is not ragged"
    return strips


@functools.lru_cache(maxsize=None)
def wgrad_case(i):
    """(family of A, [B per source]) of WGRAD[i]; B dense with arbitrary fp32 values (``_values``: full significands, both signs)."""
    name, kd, ks, stride, ca, cbs, b_grid, strips, ragged = WGRAD[i]
    fam = GB.wgrad_family(ca, a_grid(kd, stride, b_grid), strips, seed=300 + i)
    gen = torch.Generator().manual_seed(700 + i)
    Bs = [CB._values(cb * math.prod(b_grid), gen).view(cb, *b_grid) for cb in cbs]
    return fam, Bs


def squeeze2d(t_, kd):
    """[c, 1, h, w] -> [c, h, w] for the 2-D forms (what ops.conv_wgrad takes)."""
    return t_[:, 0] if kd == 1 else t_


# ---------------------------------------------------------------------------------------------------------------------------------
# the autograd Functions
# ---------------------------------------------------------------------------------------------------------------------------------
DGRAD2D_TILES = [(4, 8, 16), (16, 32)]        # the generic fp32 MFMA kernel's 16 x 16 tiles and the single-output-channel form's rows
# A.conv2d: (ks, cins, cout, (h, w), act, bias): (17, 3, 9): the dgrad's 29 outputs are no multiple of 16; cin = 1: the host-packed
# single-output-channel dgrad; cout 7 / 12: the dgrad's reduction dimension is no multiple of 4; one case per activation
CONV2D = [(3, (17, 3, 9), 12, (21, 28), "relu", True), (3, (1,), 7, (21, 30), "none", True), (1, (6,), 7, (21, 28), "sigmoid", True),
          (1, (16, 5), 12, (21, 30), "tanh", False)]
# A.conv2d_k5s2: (cin, cout, (hin, win)): cin 20 = two launches of 16 + 4
K5S2 = [(3, 8, (31, 45)), (8, 6, (31, 45)), (20, 8, (31, 45)), (3, 6, (32, 40)), (8, 16, (32, 40)), (20, 8, (32, 40))]
# A.conv3d: (cins, cout, stride, (D, h, w)); A.deconv3d: (cin, cout, stride, (D, h, w) of the input)
CONV3D = [((8, 8), 1, (1, 1, 1), (3, 10, 12)), ((1,), 8, (1, 1, 1), (5, 9, 12)), ((8,), 16, (2, 2, 2), (4, 10, 12)),
          ((1,), 8, (1, 2, 2), (3, 10, 12))]
DECONV3D = [(16, 8, (2, 2, 2), (2, 5, 6)), (8, 1, (1, 2, 2), (3, 5, 6))]
FUNC = ([("conv2d", i) for i in range(len(CONV2D))] + [("k5s2", i) for i in range(len(K5S2))] + [("conv3d", i) for i in range(len(CONV3D))]
        + [("deconv3d", i) for i in range(len(DECONV3D))])


def func_geometry(kind, i):
    """-> dict: cins, cout, x grid, y grid, ks, stride, padding, dims, output padding of the input gradient's transposed convolution
    (None: a plain one), act, bias, weight shape, transposed forward."""
    if kind == "conv2d":
        ks, cins, cout, hw, act, bias = CONV2D[i]
        return dict(cins=cins, cout=cout, xg=hw, yg=hw, ks=ks, stride=(1, 1), pad=ks // 2, dims=2, act=act, bias=bias,
                    wshape=(cout, sum(cins), ks, ks), tiles=DGRAD2D_TILES, par=False)
    if kind == "k5s2":
        cin, cout, (h, w) = K5S2[i]
        return dict(cins=(cin,), cout=cout, xg=(h, w), yg=((h - 1) // 2 + 1, (w - 1) // 2 + 1), ks=5, stride=(2, 2), pad=2, dims=2,
                    act="none", bias=False, wshape=(cout, cin, 5, 5), tiles=CC.GENERIC_TILES, par=True, xtiles=CC.K5S2_TILES)
    if kind == "conv3d":
        cins, cout, st, g = CONV3D[i]
        return dict(cins=cins, cout=cout, xg=g, yg=tuple((n - 1) // s + 1 for n, s in zip(g, st)), ks=3, stride=st, pad=1, dims=3,
                    act="none", bias=False, wshape=(cout, sum(cins), 3, 3, 3), tiles=CC.VOL_TILES, par=st != (1, 1, 1))
    cin, cout, st, g = DECONV3D[i]
    return dict(cins=(cin,), cout=cout, xg=g, yg=tuple(n * s for n, s in zip(g, st)), ks=3, stride=st, pad=1, dims=3, act="none",
                bias=False, wshape=(cin, cout, 3, 3, 3), tiles=CC.VOL_TILES, par=True)


def out_padding(kind, geo):
    """Output padding of the transposed convolution from the small grid of a form to its large one: the input gradient of a
    convolution (y -> x), the forward of a transposed convolution (x -> y)."""
    small, large = (geo["xg"], geo["yg"]) if kind == "deconv3d" else (geo["yg"], geo["xg"])
    return tuple(l_ - ((s_ - 1) * st - 2 * geo["pad"] + geo["ks"]) for s_, l_, st in zip(small, large, geo["stride"]))


@functools.lru_cache(maxsize=None)
def func_inputs(kind, i):
    """Deterministic inputs of a Function case: weight (He-scaled Gaussian), bias, the impulse family of the output gradient (over
    the output grid, the seams of the kernel that runs the input gradient), the impulse family of the input, and dense inputs /
    output gradients for the batch sizes of the two families."""
    geo = func_geometry(kind, i)
    gen = torch.Generator().manual_seed(900 + 17 * i + len(kind))
    fan = (sum(geo["cins"]) if kind != "deconv3d" else geo["cins"][0]) * geo["ks"] ** geo["dims"]
    w = CB.he_weights(geo["wshape"], fan, gen)
    b = 0.1 * torch.randn(geo["cout"], generator=gen) if geo["bias"] else None
    reach = 1 if kind != "conv2d" else geo["ks"] // 2
    gfam = CC.family((geo["cout"],), geo["yg"], reach, CC.fam_key(geo["tiles"]), seed=40 + i, parities=geo["par"])
    xreach = geo["ks"] // 2 if kind != "deconv3d" else 1
    xfam = CC.family(geo["cins"], geo["xg"], xreach, CC.fam_key(geo.get("xtiles", geo["tiles"])), seed=60 + i, parities=geo["par"])
    cin = sum(geo["cins"])
    x_dense = torch.randn(len(gfam.members), cin, *geo["xg"], generator=gen)
    g_dense = CB._values(len(xfam.members) * geo["cout"] * math.prod(geo["yg"]), gen).view(len(xfam.members), geo["cout"], *geo["yg"])
    return geo, w, b, gfam, xfam, x_dense, g_dense


def fwd_interval(kind, geo, x, w, b):
    """The Function's forward output on the batch x, exact fp32 products."""
    tr = out_padding(kind, geo) if kind == "deconv3d" else None
    iv = CB.conv_interval(x, None, w, b, geo["stride"], geo["pad"], tr, "fp32", geo["dims"])
    a = CB.act_interval(*iv, geo["act"], "exact")
    a.k_eff = iv.k_eff
    return a


def dx_interval(kind, geo, g, ex, w, mode="fp32"):
    """The input gradient: a transposed convolution of the output gradient with the forward weight (whose out / in axes are the
    transposed weight's in / out); of a transposed convolution: the plain strided convolution whose [out][in] weight is the
    transposed weight [cin][cout] as it stands."""
    if kind == "deconv3d":
        return CB.conv_interval(g, ex, w, None, geo["stride"], geo["pad"], None, mode, 3, n_epi=0)
    return CB.conv_interval(g, ex, w, None, geo["stride"], geo["pad"], out_padding(kind, geo), mode, geo["dims"], n_epi=0)


def wgrad_stride(geo):
    return (geo["stride"][0], geo["stride"][1]) if geo["dims"] == 3 else (1, geo["stride"][1])


def dw_interval(kind, geo, a, ex, dense):
    """The weight gradient over a batch: ``a`` the sparse operand [M, ca, ...] (the output gradient behind the activation backward,
    with its half-widths ``ex``; a transposed convolution: the input), ``dense`` the other one; K_eff counts the products of all
    samples -- the host's batch loop adds them into one dW.  -> [ca, cb_total, taps]."""
    kd, ks, st, cins = (3 if geo["dims"] == 3 else 1), geo["ks"], wgrad_stride(geo), geo["cins"]
    if kind == "deconv3d":
        return GB.wgrad_finish([GB.wgrad_terms(a, dense, kd, ks, st, geo["cout"], 0, batched=True)])
    terms, ext, o = [], [], 0
    for c in cins:
        terms.append(GB.wgrad_terms(a, dense[:, o:o + c], kd, ks, st, sum(cins), o, batched=True))
        if ex is not None:
            ext.append(GB.wgrad_terms(ex, dense[:, o:o + c].abs(), kd, ks, st, sum(cins), o, batched=True))
        o += c
    return GB.wgrad_finish(terms, None, ext)


def torch_forward(kind, geo, W, b, x):
    """The same operation in torch (any dtype): x the channel concatenation of the sources."""
    import torch.nn.functional as F
    if kind == "deconv3d":
        return F.conv_transpose3d(x, W, None, stride=geo["stride"], padding=1, output_padding=out_padding(kind, geo))
    y = (F.conv2d, F.conv3d)[geo["dims"] - 2](x, W, b, stride=geo["stride"], padding=geo["pad"])
    return {"none": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[geo["act"]](y)
