"""CPU proof that the instrument of tests/conv_bound.py is right and sharp:

* the two evaluations of the float64 reference (from the non-zeros, and torch's dense convolution) agree;
* the three arithmetics restated in torch (``emulate``) lie inside ``conv_interval`` for EVERY member of EVERY impulse family the GPU
  file uses and for one dense input per shape, nothing left out;
* every family's coverage table is full for the tile geometry it claims;
* nine mutants of the emulation are caught on the impulse family at every channel count -- and the table printed by
  ``test_mutants`` records which of them the present checks (the tolerances of tests/test_gpu_kernels.py on that test's dense
  Gaussian input) accept.  Mutant 1 (the lo half of ONE packed weight dropped) is accepted by them at cin = 48 and 96: the reason
  this file exists."""
import pytest
import torch

import conv_bound as CB
import conv_cases as CC
from common import check_close, conv_tol

MODES = ("fp32", "split", "bf16")


# ---------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,transposed,stride,spatial", [
    (2, None, 1, (21, 28)), (2, None, 2, (21, 28)), (2, None, 2, (20, 37)), (3, None, 1, (5, 9, 12)), (3, None, 2, (5, 9, 12)),
    (3, None, (1, 2, 2), (3, 8, 9)), (3, (1, 1, 1), 2, (3, 5, 6)), (3, (0, 1, 1), (1, 2, 2), (3, 5, 6))])
def test_reference_from_non_zeros_is_the_dense_convolution(dims, transposed, stride, spatial):
    g = torch.Generator().manual_seed(dims * 10 + len(spatial))
    cin, cout, k = 6, 10, (5 if dims == 2 and stride == 2 else 3)
    w = torch.randn(*((cout, cin) if transposed is None else (cin, cout)), *(k,) * dims, generator=g)
    x = torch.randn(cin, *spatial, generator=g) * (torch.rand(cin, *spatial, generator=g) < 0.06)
    args = (CB._tuple(stride, dims), (k // 2,) * dims, transposed, dims)
    a, b = CB.linear(x, w, *args, method="scatter"), CB.linear(x, w, *args, method="dense")
    assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())


def _conv_args(key):
    """(ks, stride, padding, transposed, dims, cout) of the single convolution a family is made for."""
    if key[0] == "vol":
        kind, cins, cout, stride, dims, relu, skip = CC.VOL_CASES[key[1]]
        st = CB._tuple(stride, 3)
        tr = None if kind == "conv" else tuple(s - 1 for s in st)
        return 3, st, 1, tr, 3, cout
    if key[0] == "generic":
        return key[1], 1, key[1] // 2, None, 2, 20
    if key[0] == "k5s2":
        return 5, 2, 2, None, 2, 24
    if key[0] == "c1k7":
        return 7, 1, 3, None, 2, 16
    return 3, 1, 1, None, 2, 20


def test_emulation_inside_every_interval_of_every_family():
    """Every member of every family of the GPU file, the three arithmetics, half of the families with a bias: inside, nothing left
    out, and the untouched elements bit-exact (check_bounded pins them).  K_eff <= 1 everywhere: the condition the spacing exists for."""
    worst, n = {m: 0.0 for m in MODES}, 0
    for i, (key, fam) in enumerate(CC.all_families().items()):
        ks, stride, padding, tr, dims, cout = _conv_args(key)
        w, b = CC.weights(cout, sum(fam.cins), ks, seed=i, bias=i % 2, dims=dims, transposed=tr is not None)
        for s0 in range(0, len(fam.members), 64):                        # batches of members: one evaluation of the reference each
            x = torch.stack(fam.members[s0:s0 + 64])
            iv0 = CB.conv_interval(x, None, w, b, stride, padding, tr, "fp32", dims)
            assert int(iv0.k_eff.max()) <= 1, f"{key}: two impulses reach one output element"
            for m in MODES:
                ivm = iv0.remode(m)
                rep = CB.check_bounded(f"{key} {m}", CB.emulate(x, w, b, m, stride, padding, tr, dims), *ivm, k_eff=ivm.k_eff, quiet=True)
                worst[m] = max(worst[m], rep["used"])
                n += x.shape[0]
    print(f"[bound] emulation on impulse families: {n} checks, largest share used " + ", ".join(f"{m} {worst[m]:.3f}" for m in MODES))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("dims,cin,cout,spatial,stride", [(2, 48, 20, (21, 28), 1), (2, 16, 7, (37, 52), 1), (2, 8, 16, (37, 52), 2),
                                                         (3, 8, 16, (5, 9, 12), 1), (3, 16, 8, (12, 20, 28), 2)])
def test_emulation_inside_on_a_dense_input(dims, cin, cout, spatial, stride):
    g = torch.Generator().manual_seed(cin + cout)
    ks = 5 if dims == 2 and stride == 2 else 3
    w, b = CC.weights(cout, cin, ks, seed=cin, bias=True, dims=dims)
    x = torch.randn(cin, *spatial, generator=g)
    for m in MODES:
        iv = CB.conv_interval(x, None, w, b, stride, ks // 2, None, m, dims)
        rep = CB.check_bounded(f"dense {dims}-D cin={cin} {m}", CB.emulate(x, w, b, m, stride, ks // 2, None, dims), *iv, k_eff=iv.k_eff)
        assert rep["used"] <= 1.0 and rep["pinned"] == 0


def test_emulation_inside_on_a_dense_input_of_every_shape():
    """One dense Gaussian input per family of the GPU file -- its channel count, its shape, its convolution (kernel size, stride,
    transposed or not), with a bias: the three arithmetics inside, nothing pinned, nothing left out."""
    worst = {m: 0.0 for m in MODES}
    fams = CC.all_families()
    for i, (key, fam) in enumerate(fams.items()):
        ks, stride, padding, tr, dims, cout = _conv_args(key)
        w, b = CC.weights(cout, sum(fam.cins), ks, seed=500 + i, bias=True, dims=dims, transposed=tr is not None)
        x = torch.randn(sum(fam.cins), *fam.spatial, generator=torch.Generator().manual_seed(i))
        iv0 = CB.conv_interval(x, None, w, b, stride, padding, tr, "fp32", dims)
        for m in MODES:
            iv = iv0.remode(m)
            rep = CB.check_bounded(f"dense {key} {m}", CB.emulate(x, w, b, m, stride, padding, tr, dims), *iv, k_eff=iv.k_eff, quiet=True)
            assert rep["pinned"] == 0
            worst[m] = max(worst[m], rep["used"])
    print(f"[bound] emulation on {len(fams)} dense inputs: largest share used " + ", ".join(f"{m} {worst[m]:.3f}" for m in MODES))
    assert max(worst.values()) <= 1.0


def test_chain_and_activations_inside():
    """3x3 -> ReLU -> 3x3 in split arithmetic (the first stage's half-width is the second's ``ex``), then each activation."""
    fam = CC.family((8,), (21, 28), 2, CC.fam_key(CC.FUSED_TILES), seed=5)
    w1, b1 = CC.weights(8, 8, 3, seed=1, bias=True)
    w2, b2 = CC.weights(6, 8, 3, seed=2, bias=True)
    for x in fam.members[:16]:
        i1 = CB.conv_interval(x, None, w1, b1, mode="split")
        m1 = CB.act_interval(*i1, "relu")
        y1 = CB.emulate(x, w1, b1, "split").clamp_min(0.0)
        CB.check_bounded("chain stage 1", y1, *m1, quiet=True)
        i2 = CB.conv_interval(m1.mid.float(), m1.half + (m1.mid - m1.mid.float().double()).abs(), w2, b2, mode="split")
        y2 = CB.emulate(y1, w2, b2, "split")
        CB.check_bounded("chain stage 2", y2, *i2, quiet=True)
        for act, fn in (("relu", torch.relu), ("sigmoid", torch.sigmoid), ("tanh", torch.tanh)):
            CB.check_bounded(f"chain {act}", fn(y2), *CB.act_interval(*i2, act), quiet=True)


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
def test_every_coverage_table_is_full():
    fams = CC.all_families()
    for key, fam in fams.items():
        fam.assert_full()
        assert all(int((x != 0).sum()) >= 1 for x in fam.members)
    for key in list(fams)[::9]:                                          # the table kept while generating is the recount
        assert fams[key].tabulate() == fams[key].table, key
    # the values: full significands, both signs, magnitudes over 2^-12 .. 2^12, not bf16-representable
    v = torch.cat([x[x != 0] for x in fams[("split", (16,), (21, 28), 1)].members])
    assert bool((v > 0).any()) and bool((v < 0).any()) and float(v.abs().min()) < 2.0 ** -10 and float(v.abs().max()) > 2.0 ** 10
    assert float((v.bfloat16().float() != v).double().mean()) > 0.95


def test_spacing_leaves_untouched_rows_and_columns():
    fam = CC.family((16,), (21, 28), 1, CC.fam_key(CC.split_tiles(1)), seed=16)
    w, _ = CC.weights(16, 16, 3, seed=3, bias=False)
    iv = CB.conv_interval(fam.members[0], None, w, None, mode="split")
    touched = iv.k_eff.sum(0) > 0
    assert bool((~touched).all(0).any()) and bool((~touched).all(1).any()), "a column and a row no response touches"
    assert int(((iv.half == 0) & (iv.mid == 0)).sum()) > 0


# ---------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------
def _emu64(xh, xl, wh, wl, cv):
    return cv(xh, wh) + cv(xh, wl) + cv(xl, wh)


def _mutant(k, x, w, b, cout, cv, cv_pad0, seam):
    """Mutant ``k`` of the split arithmetic -> fp32 output.  ``cv`` the float64 convolution of this case, ``cv_pad0`` the same without
    padding (mutant 6 pads by hand), ``seam`` a tile seam of the last axis."""
    (xh, xl), (wh, wl) = CB.split_hi_lo(x), CB.split_hi_lo(w)
    xh, xl, wh, wl = xh.double(), xl.double(), wh.double().clone(), wl.double().clone()
    bd = torch.zeros(cout, dtype=torch.float64) if b is None else b.double()
    co, ci = min(3, cout - 1), min(5, x.shape[0] - 1)
    centre = tuple(s // 2 for s in w.shape[2:])
    y = None
    if k == 1:
        wl[(co, ci) + centre] = 0
    elif k == 2:
        wl[co] = 0
    elif k == 3:
        wl[:, ci] = 0                                                    # the x_hi * w_lo term of one input channel
    elif k == 4:
        a, c = (co, ci) + centre[:-1] + (0,), (co, ci) + centre[:-1] + (w.shape[-1] - 1,)
        for t_ in (wh, wl):
            t_[a], t_[c] = t_[c].clone(), t_[a].clone()
    elif k == 5:
        only_h, only_l = torch.zeros_like(xh), torch.zeros_like(xl)
        only_h[ci, ..., seam - 1], only_l[ci, ..., seam - 1] = xh[ci, ..., seam - 1], xl[ci, ..., seam - 1]
        y = _emu64(xh, xl, wh, wl, cv)
        y[..., seam:] -= _emu64(only_h, only_l, wh, wl, cv)[..., seam:]
    elif k == 6:
        nd = x.dim() - 1
        pad = lambda t_: torch.nn.functional.pad(t_, (1, 1) * nd)        # noqa: E731
        ph, pl = pad(xh), pad(xl)
        inner = (slice(None),) + (slice(1, -1),) * (nd - 1)
        ph[inner + (0,)], pl[inner + (0,)] = 1e-4 * xh[..., 0], 1e-4 * xl[..., 0]
        y = _emu64(ph, pl, wh, wl, cv_pad0)
    elif k == 7:
        bd = bd.float().bfloat16().double()
    if y is None:
        y = _emu64(xh, xl, wh, wl, cv)
    y = (y + bd.view((-1,) + (1,) * (x.dim() - 1))).float()
    if k == 8:
        y[cout - 1] = y[cout - 2]
    return y


def _mutant9(x, w, b, dims):
    """Stride 2: the odd-parity columns take the weight of the even ones' tap (kx = 1 reads kx = 0's weight in a 5-tap row; in a 3-tap
    row kx = 0 reads kx = 1's)."""
    ks = w.shape[-1]
    odd = torch.zeros_like(x)
    odd[..., 1::2] = x[..., 1::2]
    wm = w.clone()
    if ks == 5:
        wm[..., 1] = w[..., 0]
    else:
        wm[..., 0] = w[..., 1]
    y = CB.emulate(x - odd, w, b, "split", 2, ks // 2, None, dims).double() + CB.emulate(odd, wm, None, "split", 2, ks // 2, None, dims).double()
    return y.float()


def _caught(fam, run, interval):
    """Whether some member of the family fails check_bounded under the mutant; -> (caught, by how much the bound is exceeded)."""
    for x in fam.members:
        iv = interval(x)
        try:
            CB.check_bounded("mutant", run(x), *iv, quiet=True)
        except CB.OutOfBound:
            err = (run(x).double() - iv.mid).abs()
            return True, float(torch.where(iv.half > 0, err / iv.half.clamp_min(1e-300), err * 1e30).max())
    return False, 0.0


def _present_accepts(name, got, want, tol):
    try:
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            check_close(name, got, want, **tol)
        return True
    except AssertionError:
        return False


MUTANTS = {1: "lo of one packed weight dropped", 2: "lo of all weights of one output channel dropped",
           3: "hi*lo term dropped for one input channel", 4: "two taps of one (co, ci) exchanged",
           5: "one halo column of one input channel read as 0 at a tile seam", 6: "a padding tap reads 1e-4 of its neighbour",
           7: "bias rounded to bf16", 8: "last channel of the ragged 16-tile written from its neighbour",
           9: "stride 2: odd-parity column takes the even one's tap"}


@pytest.mark.parametrize("dims,cin", [(2, 16), (2, 48), (2, 96), (3, 8), (3, 32)])
def test_mutants(dims, cin):
    """Each mutant fails check_bounded on the impulse family.  The present check -- 2-D: test_conv2d_split_bf16's 3e-5 * peak on a
    dense Gaussian input after ReLU (stride 2: conv_tol(1e-4, 2e-5) of test_conv5x5_stride2_split_precision); 3-D:
    test_conv3d_block's conv_tol(1e-4, 1e-5) -- is run on the same mutant and the outcome printed."""
    spatial = (21, 28) if dims == 2 else (5, 9, 20)
    tiles = CC.split_tiles(2) if dims == 2 else CC.VOL_TILES
    fam = CC.family((cin,), spatial, 1, CC.fam_key(tiles), seed=cin)
    g = torch.Generator().manual_seed(cin * 7 + dims)
    dense = torch.randn(cin, *spatial, generator=g)
    accepted = {}
    for k in range(1, 9):
        couts = (7, 12, 20, 36) if k == 8 else (cin if dims == 2 else 16,)
        for cout in couts:
            w, b = CC.weights(cout, cin, 3, seed=cin + cout, bias=True, dims=dims)
            cv = lambda a, kk: CB.linear(a, kk, (1,) * dims, (1,) * dims, None, dims)            # noqa: E731
            cv0 = lambda a, kk: CB.linear(a, kk, (1,) * dims, (0,) * dims, None, dims)           # noqa: E731
            run = lambda x, k=k, w=w, b=b, cout=cout: _mutant(k, x, w, b, cout, cv, cv0, 16)      # noqa: E731
            ok, factor = _caught(fam, run, lambda x: CB.conv_interval(x, None, w, b, mode="split", dims=dims))
            assert ok, f"mutant {k} ({MUTANTS[k]}) passes on the impulse family at cin={cin} cout={cout}"
            want = torch.relu(cv(dense, w) + b.double().view((-1,) + (1,) * dims))
            got = torch.relu(run(dense))
            tol = dict(rtol=0.0, atol=3e-5 * float(want.abs().max())) if dims == 2 else conv_tol("split", want, 1e-4, 1e-5)
            accepted[(k, cout)] = (_present_accepts("present", got, want.float(), tol), factor)
    # mutant 9 on the strided form of this dimension
    par_fam = CC.family((cin,), spatial, 2 if dims == 2 else 1, CC.fam_key(CC.K5S2_TILES if dims == 2 else CC.VOL_TILES), seed=cin, parities=True)
    ks = 5 if dims == 2 else 3
    w, b = CC.weights(16, cin, ks, seed=cin + 9, bias=True, dims=dims)
    ok, factor = _caught(par_fam, lambda x: _mutant9(x, w, b, dims), lambda x: CB.conv_interval(x, None, w, b, 2, ks // 2, None, "split", dims))
    assert ok, f"mutant 9 passes on the impulse family at cin={cin}"
    want = torch.relu(CB.linear(dense, w, (2,) * dims, (ks // 2,) * dims, None, dims) + b.double().view((-1,) + (1,) * dims))
    tol = conv_tol("split", want, 1e-4, 2e-5 if dims == 2 else 1e-5)
    accepted[(9, 16)] = (_present_accepts("present", torch.relu(_mutant9(dense, w, b, dims)), want.float(), tol), factor)
    for (k, cout), (acc, factor) in accepted.items():
        print(f"[mutant] {dims}-D cin={cin:3d} cout={cout:3d}  {k}: {MUTANTS[k]:62s} impulse check: caught (bound exceeded {factor:9.3g}-fold)"
              f"   present check: {'ACCEPTS' if acc else 'rejects'}")
    if dims == 2 and cin in (48, 96):
        assert accepted[(1, cin)][0], "the present tolerance was measured to accept mutant 1 at cin = 48 and 96"


# ---------------------------------------------------------------------------------------------
# tile forms of the launch rules (conv_cases.FORM_CASES; host only: ops.launch_form launches nothing)
# ---------------------------------------------------------------------------------------------
def test_every_form_case_reaches_its_form():
    """Each case of the table gets the form it is written for from the product's own rule under the options it sets; where an option
    forces the form, the rule alone picks another one on that map (the case is not a second copy of an existing one)."""
    from effi_mvs_plus_amd import ops
    cases = CC.form_cases()
    assert len(cases) >= 60
    for c in cases:
        with ops.options(**c.options):
            got = tuple(ops.launch_form(**c.query))
        assert got == tuple(c.form), f"{c.row}: {c.how}: the rule gives {got}, the case is written for {c.form}"
        if any(k in c.options for k in ("force_mr", "roll_mr", "roll_zt", "deconv_mr")):
            assert tuple(ops.launch_form(**c.query)) != tuple(c.form), f"{c.row}: {c.how}: the rule picks this form unaided"
    # what stays out of the table: forms only an option can force
    table = CC.forms()
    assert (1, 16, 4, 1, 1) not in table["x3 planar"] and (2, 32, 4, 1, 1) not in table["x3 planar"]         # wide with MR 1 / 2
    assert all(f[2] == 4 or f == CC.W8 for f in table["x3 sr"]) and all(f[2] == 4 for f in table["x3_pair sr"])
    assert CC.WIDE not in table["x3 z-batched"] and CC.WIDE not in table["x3_zb_batch"]


def test_workloads_take_only_forms_of_the_table():
    """The launch rule over the stage maps of the workloads bench.py names (cfg1-cfg5 at 1/8, 1/4, 1/2 and full resolution, D in 48 / 32 /
    8, 1-5 images or samples, every N-tile count): every form it returns has a bound case.  A form the workloads can take and no case
    covers fails here, without a GPU."""
    from effi_mvs_plus_amd import ops
    table, seen, missing = CC.forms(), {}, set()
    for row, query, D in CC.workload_queries():
        key = CC.table_form(row, ops.launch_form(**query), D)
        seen.setdefault(row, set()).add(key)
        if key not in table[row]:
            missing.add((row, key, tuple(sorted(query.items()))))
    assert not missing, f"forms the workloads take that no bound case launches: {sorted(missing)[:8]}"
    assert set(seen) == set(table)
    for row in table:
        print(f"[forms] {row}: the workloads take {len(seen[row])} of the table's {len(table[row])} forms")
    # the forms this work is about are ones the workloads do take: stage 2 runs 4 rows per wave, stage 3 the wide tile (2 rows with NT 2)
    assert tuple(ops.launch_form("x3", 296, 400, nt=1)) == CC.MR4 and tuple(ops.launch_form("x3", 592, 800, nt=1)) == CC.WIDE
    assert tuple(ops.launch_form("x3", 592, 800, nt=2)) == CC.MR2 and tuple(ops.launch_form("x3", 74, 100, nt=6, sr=True)) == CC.W8
