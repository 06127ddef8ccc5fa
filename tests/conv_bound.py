"""Float64 reference and bound algebra of the convolution kernels.  CPU only: nothing here imports the
HIP library or touches a GPU.

Dense inputs make every output a sum of K = 9 * cin products whose peak hides one product's worth of error.  ``impulse_inputs``
yields sparse inputs with at most one non-zero product per output element, ``conv_interval`` the float64 value and a derived
half-width per element, ``check_bounded`` the check: every element inside its interval, bit-exact where the interval is a point.

Constants (u = 2^-24, first order; each is counted here, against the kernel arithmetic it is used for):

  C_MODE["fp32"]  = 0          operands are the fp32 values themselves; the product's own rounding is counted in ACC["fp32"].
  C_MODE["split"] = 3 * 2^-16  x = xh + xl + rx with xh = bf16(x), xl = bf16(x - xh) (round to nearest even, 8 significant bits:
                               |x - xh| <= 2^-8 |x|, |rx| <= 2^-16 |x|), the same for w.  The kernel sums xh wh + xh wl + xl wh, so
                               x w - sum = xl wl + rx w + x rw (+ second order): three terms of at most 2^-16 |x w| each.  The
                               split-resident producers split once in their epilogue and the packers split the weights on the host
                               with the same two conversions: the same three terms.
  C_MODE["bf16"]  = 2 * 2^-8 + 2^-16   xh wh only: x w - xh wh = (x - xh) w + xh (w - wh) <= (2^-8 + 2^-8 (1 + 2^-8)) |x w|.

  ACC[mode] = roundings per NON-ZERO product on the way into the fp32 accumulator:
      fp32  2   the product (24 x 24 bits does not fit fp32) and its accumulation; a fused multiply-add uses one of the two.
      split 3   three partial products (each exact: 8 x 8 bits), three accumulations.
      bf16  1   one exact partial product, one accumulation.
  A zero product adds exactly 0 in every mode and is not counted: K_eff, not K.  Where K_eff = 0 the accumulator holds exactly the
  fp32 bias (0 + b and b + 0 are exact) and the interval is a point.
"""
import itertools
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_MODE = {"fp32": 0.0, "split": 3.0 * 2.0 ** -16, "bf16": 2.0 * 2.0 ** -8 + 2.0 ** -16}
ACC = {"fp32": 2, "split": 3, "bf16": 1}
# Activations' own error.  Exact forms (every kernel in "fp32" precision and the PLAIN epilogue of the split kernels):
# 1 / (1 + expf(-x)): expf <= 1 ulp = 2u relative, the addition and the division u each -> 4u of a value <= 1; tanhf <= 2 ulp = 4u
# of a value <= 1.  Split forms (GRU epilogues of the split kernels: effi_sigmoid_split / effi_tanh_split of csrc/common.hpp):
# 2e-7 absolute, as documented there.
ACT_ERR = {"exact": 4.0 * U, "split": 2.0e-7}


def _tuple(v, nd):
    return tuple(int(a) for a in v) if isinstance(v, (tuple, list)) else (int(v),) * nd


def out_size(n, k, stride, padding, transposed=None):
    """Output extent of one axis; ``transposed``: None, or that axis' output padding."""
    if transposed is None:
        return (n + 2 * padding - k) // stride + 1
    return (n - 1) * stride - 2 * padding + k + transposed


def _dense(x, w, stride, padding, transposed, dims):
    if transposed is None:
        return (F.conv2d, F.conv3d)[dims - 2](x, w, None, stride=stride, padding=padding)
    return (F.conv_transpose2d, F.conv_transpose3d)[dims - 2](x, w, None, stride=stride, padding=padding, output_padding=transposed)


def _scatter(x, w, stride, padding, transposed, dims):
    """The same linear map evaluated from the input's non-zeros: out[co, o] += w[co, ci, k] * x[ci, i] with i = o * stride - pad + k
    (transposed: o = i * stride - pad + k).  Cost ~ non-zeros x cout x taps: what makes hundreds of impulse members affordable.
    x [M, cin, *spatial] -> [M, cout, *out]."""
    ks = tuple(w.shape[2:])
    cout = w.shape[1] if transposed is not None else w.shape[0]
    osz = [out_size(x.shape[2 + a], ks[a], stride[a], padding[a], None if transposed is None else transposed[a]) for a in range(dims)]
    npix = math.prod(osz)
    out = torch.zeros(x.shape[0] * cout * npix, dtype=torch.float64)
    taps = torch.tensor(list(itertools.product(*[range(k) for k in ks])), dtype=torch.int64)            # [T, dims]
    st, pd, lim = torch.tensor(stride), torch.tensor(padding), torch.tensor(osz)
    nz_all = x.nonzero()                                                 # [N, 2 + dims]
    step = max(1, int(2.0e6 // (cout * len(taps))))                      # non-zeros per pass: bounds the contribution tensor
    for s0 in range(0, nz_all.shape[0], step):
        nz = nz_all[s0:s0 + step]
        m, ci, pos = nz[:, 0], nz[:, 1], nz[:, 2:]
        val = x[tuple(nz.t())]
        if transposed is None:
            num = pos[:, None, :] + pd - taps[None]                      # o * stride
            o = torch.div(num, st, rounding_mode="floor")
            ok = (num % st == 0).all(-1)
            wsel = w.reshape(cout, w.shape[1], -1)[:, ci, :]             # [cout, N, T]
        else:
            o = pos[:, None, :] * st - pd + taps[None]
            ok = torch.ones(o.shape[:2], dtype=torch.bool)
            wsel = w.reshape(w.shape[0], cout, -1)[ci].permute(1, 0, 2)  # [cout, N, T]
        ok &= ((o >= 0) & (o < lim)).all(-1)
        flat = torch.zeros(o.shape[:2], dtype=torch.int64)
        for a in range(dims):
            flat = flat * osz[a] + o[..., a].clamp(0, osz[a] - 1)
        index = (m[None, :, None] * cout + torch.arange(cout)[:, None, None]) * npix + flat[None]        # [cout, N, T]
        out.index_add_(0, index.reshape(-1), (wsel * (val[:, None] * ok)[None]).reshape(-1))
    return out.view(x.shape[0], cout, *osz)


def linear(x, w, stride, padding, transposed, dims, method=None):
    """The bias-free convolution in float64: x [cin, *spatial] (or a batch [M, cin, *spatial] of inputs), w [cout, cin, *k]
    ([cin, cout, *k] transposed)."""
    x, w = x.double(), w.double()
    batched = x.dim() == dims + 2
    xb = x if batched else x[None]
    if method is None:
        method = "scatter" if int((xb != 0).sum()) * 8 <= xb.numel() else "dense"
    y = (_scatter if method == "scatter" else _dense)(xb, w, stride, padding, transposed, dims)
    return y if batched else y[0]


class Interval:
    """(mid, half) in float64 plus the bookkeeping ``check_bounded`` reports: K_eff per element."""

    def __init__(self, mid, half, k_eff=None, parts=None):
        self.mid, self.half, self.k_eff, self.parts = mid, half, k_eff, parts

    def remode(self, mode):
        """The interval of the same convolution in another arithmetic (mid, sum |w||x| and K_eff do not depend on it)."""
        return Interval(self.mid, _half(mode, *self.parts), self.k_eff, self.parts)

    def __iter__(self):
        return iter((self.mid, self.half))


def _half(mode, s_abs, babs, k_eff, carried, n_epi):
    roundings = torch.where(k_eff > 0, ACC[mode] * k_eff + n_epi, torch.zeros_like(k_eff))
    half = C_MODE[mode] * s_abs + roundings * U * (s_abs + babs)
    return half if carried is None else half + carried


def conv_interval(x, ex, w, b, stride=1, padding=1, transposed=None, mode="split", dims=2, n_epi=1, method=None):
    """Float64 interval of a convolution of the fp32 values ``x`` [cin, *spatial] handed to the kernel (or of a batch [M, cin, *spatial]
    of such inputs: every array of the result then has the leading M).

    mid  = the float64 convolution (+ bias);
    half = sum |w| ex + C_MODE[mode] * sum |w| |x| + (ACC[mode] * K_eff + n_epi) * u * (sum |w| |x| + |b|), the last term only where
           K_eff > 0 (see the module docstring); ``ex`` is the half-width carried by the input (None for a test input), K_eff the
           number of non-zero products of the element (the input's non-zero mask convolved with the weight's), ``n_epi`` the roundings
           of the epilogue before any activation (1: the bias addition).
    ``transposed``: None, or the output padding (per axis) of a transposed convolution with w [cin, cout, *k]."""
    stride, padding = _tuple(stride, dims), _tuple(padding, dims)
    if transposed is not None:
        transposed = _tuple(transposed, dims)
    x, w = x.detach().double().cpu(), w.detach().double().cpu()
    lin = lambda a, k, m=method: linear(a, k, stride, padding, transposed, dims, m)      # noqa: E731
    mid = lin(x, w)
    s_abs = lin(x.abs(), w.abs())
    k_eff = lin((x != 0).double(), (w != 0).double()).round()
    shape = (-1,) + (1,) * dims
    babs = torch.zeros(mid.shape[-dims - 1], dtype=torch.float64)
    if b is not None:
        bd = b.detach().double().cpu()
        mid = mid + bd.view(shape)
        babs = bd.abs()
    carried = None if ex is None else lin(ex.detach().double().cpu(), w.abs(), "dense")
    parts = (s_abs, babs.view(shape), k_eff, carried, n_epi)
    return Interval(mid, _half(mode, *parts), k_eff, parts)


def _sig(v):
    return torch.sigmoid(v)


def act_interval(mid, half, act, form="exact", h=None, z=None, add=None, z_half=None):
    """Carry (mid, half) through an epilogue.  ``act``: "none", "relu", "sigmoid", "tanh", "gru_z" (sigmoid), "gru_rh" (sigmoid * h),
    "gru_q" ((1 - z) h + z tanh; ``z_half``: the half-width of z where it is computed, not given), "add" (value + ``add``: the additive
    skip and the ``+ up2`` epilogues).  Lipschitz constants: 1 for ReLU and tanh, 1/4 for the sigmoid; plus the activation's own error
    ACT_ERR[form] and u per further fp32 operation, relative to the magnitudes that operation combines.  ReLU of a point interval stays
    a point (max is exact)."""
    if act == "none":
        return Interval(mid, half)
    if act == "relu":
        return Interval(mid.clamp_min(0.0), half)
    e = ACT_ERR[form]
    if act in ("sigmoid", "gru_z"):
        return Interval(_sig(mid), half / 4 + e)
    if act == "tanh":
        return Interval(torch.tanh(mid), half + e)
    if act == "gru_rh":
        hd = h.detach().double().cpu()
        m = _sig(mid) * hd
        return Interval(m, (half / 4 + e) * hd.abs() + U * m.abs())                       # one product
    if act == "gru_q":
        hd, zd = h.detach().double().cpu(), z.detach().double().cpu()
        a, bq = (1.0 - zd) * hd, zd * torch.tanh(mid)
        # 1 - z, * h, z * tanh, the sum: four roundings, each at most u of |a| + |bq| (+ u |h| for 1 - z)
        width = zd.abs() * (half + e) + 4 * U * (a.abs() + bq.abs() + hd.abs())
        if z_half is not None:                # z itself is a computed gate (the one-launch ConvGRU): d/dz = tanh - h, |tanh| <= 1
            width = width + z_half * ((torch.tanh(mid) - hd).abs() + half + e)
        return Interval(a + bq, width)
    if act == "add":
        ad = add.detach().double().cpu()
        m = mid + ad
        return Interval(m, half + torch.where(ad != 0, U * m.abs(), torch.zeros_like(m)))  # + 0 is exact
    raise ValueError(act)


# ------------------------------------------------------------------------------------------------------------------------------
# impulse inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _axis_required(n, seams, parities):
    """Coordinates of one axis that some member must place an impulse on: first, last, an inside one, the last before and the first
    after every seam, and (strided forms) an inside coordinate of each parity."""
    req = {0, n - 1}
    if n >= 3:
        req.add(n // 2)
        if parities and n >= 4:
            req.add(n // 2 + 1 if n // 2 + 1 < n - 1 else n // 2 - 1)
    for s in seams:
        if 0 < s < n:
            req.update((s - 1, s))
    return sorted(req)


def _axis_phases(n, spacing, required):
    """Sets of coordinates with gaps >= spacing that together contain every required coordinate; each is filled up with further
    coordinates where there is room.  The first set holds coordinate 0 and, when the axis is long enough, the last one."""
    left, phases = list(required), []
    while left:
        order = [c for c in (0, n - 1) if c in left] + [c for c in left if c not in (0, n - 1)]
        chosen = []
        for c in order + list(range(n)):
            if all(abs(c - p) >= spacing for p in chosen):
                chosen.append(c)
        phases.append(sorted(chosen))
        left = [c for c in left if c not in chosen]
    return phases


def seam_positions(n, tile_sizes):
    """First coordinates after each seam of an axis of extent n: the multiples of every tile size of that axis."""
    return sorted({p for t in tile_sizes if t and t > 0 for p in range(t, n, t)})


def position_classes(pos, spatial, seams, parities=False):
    """Labels of an impulse position: its border class (per axis first / last / inside / only: corners, borders and the interior are
    the combinations), and per axis the seams it sits just before / just after and, for strided forms, the parity of an inside
    coordinate (axes of 4 or more)."""
    border = tuple("only" if n == 1 else "first" if p == 0 else "last" if p == n - 1 else "inside" for p, n in zip(pos, spatial))
    out = [("border",) + border]
    for a, (p, n) in enumerate(zip(pos, spatial)):
        for s in seams[a]:
            if p == s - 1:
                out.append(("seam", a, s, "before"))
            if p == s:
                out.append(("seam", a, s, "after"))
        if parities and n >= 4 and 0 < p < n - 1:                       # an INSIDE coordinate: every tap of that parity is in range
            out.append(("parity", a, p & 1))
    return out


def required_classes(spatial, seams, parities=False):
    per_axis = [["only"] if n == 1 else ["first", "last"] + (["inside"] if n >= 3 else []) for n in spatial]
    req = [("border",) + c for c in itertools.product(*per_axis)]
    for a, n in enumerate(spatial):
        for s in seams[a]:
            req += [("seam", a, s, "before"), ("seam", a, s, "after")]
        if parities and n >= 4:
            req += [("parity", a, 0), ("parity", a, 1)]
    return req


def _values(n, gen):
    """n arbitrary fp32 values: both signs, magnitudes 2^-12 .. 2^12, a full 24-bit significand (the low bits are random too)."""
    mant = 1.0 + torch.randint(0, 1 << 23, (n,), generator=gen).double() / float(1 << 23)
    expo = torch.randint(-12, 12, (n,), generator=gen).double()
    sign = 1.0 - 2.0 * torch.randint(0, 2, (n,), generator=gen).double()
    return (sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), expo)).float()


class ImpulseFamily:
    """``members``: list of fp32 tensors [cin, *spatial] (split into the sources' channel counts by ``sources``); ``table``:
    {position class: per-channel count of impulses placed in it}."""

    def __init__(self, cins, spatial, seams, parities, members, table, spacing):
        self.cins, self.spatial, self.seams, self.parities = tuple(cins), tuple(spatial), seams, parities
        self.members, self.table, self.spacing = members, table, spacing

    def sources(self, x):
        return list(torch.split(x, list(self.cins), 0))

    def missing(self):
        """(class, channel) pairs of the coverage table still empty."""
        return [(c, ch) for c in required_classes(self.spatial, self.seams, self.parities)
                for ch in range(sum(self.cins)) if c not in self.table or self.table[c][ch] == 0]

    def tabulate(self):
        """The coverage table recounted from the members themselves (the table kept while generating is the same)."""
        table = {}
        for x in self.members:
            for nz in x.nonzero().tolist():
                for c in position_classes(tuple(nz[1:]), self.spatial, self.seams, self.parities):
                    table.setdefault(c, [0] * sum(self.cins))[nz[0]] += 1
        return table

    def assert_full(self):
        miss = self.missing()
        assert not miss, f"impulse family {self.cins} {self.spatial}: {len(miss)} empty cells of the coverage table, e.g. {miss[:4]}"


def impulse_inputs(cins, spatial, reach=1, tiles=None, seed=0, parities=False):
    """A family of sparse inputs for a kernel whose output element reads inputs within ``reach`` pixels (per axis or one number).

    Spacing between impulses is 2 * reach + 2 per axis -- the kernel's extent plus 1 -- so no output element sees two of them and
    rows / columns no response touches exist.  ``tiles``: per axis, the tile sizes whose seams (their multiples) the kernel under
    test has.  Per axis the required coordinates are spread over "phases" (sets with gaps >= spacing); a combination of phases is
    kept when it adds a position class; every kept combination is repeated cin times with the channel assignment rotated by one, so
    that every position -- hence every class -- sees every input channel."""
    nd = len(spatial)
    cin = sum(cins)
    reach = _tuple(reach, nd)
    tiles = tiles if tiles is not None else [()] * nd
    seams = [seam_positions(spatial[a], tiles[a]) for a in range(nd)]
    spacing = [2 * r + 2 for r in reach]
    phases = [_axis_phases(spatial[a], spacing[a], _axis_required(spatial[a], seams[a], parities)) for a in range(nd)]
    need, kept = set(required_classes(spatial, seams, parities)), []
    for combo in itertools.product(*[range(len(p)) for p in phases]):
        grid = list(itertools.product(*[phases[a][combo[a]] for a in range(nd)]))
        cls = {c for pos in grid for c in position_classes(pos, spatial, seams, parities)}
        if cls & need:
            need -= cls
            kept.append(grid)
    gen = torch.Generator().manual_seed(seed)
    members, table = [], {}
    for grid in kept:
        pos = torch.tensor(grid, dtype=torch.int64)                      # [P, nd]
        for p_ in grid:                                                  # over the cin rotations every position sees every channel once
            for c in position_classes(p_, spatial, seams, parities):
                row = table.setdefault(c, [0] * cin)
                for ch in range(cin):
                    row[ch] += 1
        block = torch.zeros(cin, cin, *spatial)                          # one allocation for the cin rotations
        for rot in range(cin):
            x = block[rot]
            ch = (torch.arange(len(grid)) + rot) % cin
            x[(ch,) + tuple(pos.t())] = _values(len(grid), gen)
            members.append(x)
    return ImpulseFamily(cins, spatial, seams, parities, members, table, spacing)


def he_weights(shape, fan_in, gen):
    """He-scaled Gaussian weights: arbitrary fp32, not bf16-representable."""
    return torch.randn(*shape, generator=gen) * (2.0 / fan_in) ** 0.5


# ------------------------------------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------------------------------------
class OutOfBound(AssertionError):
    """``index``: the worst element (None for non-finite output)."""

    def __init__(self, message, index=None):
        super().__init__(message)
        self.index = index


def check_bounded(name, got, mid, half, k_eff=None, quiet=False):
    """Every element of ``got`` satisfies |got - mid| <= half; where half == 0 exactly, got == mid (the float64 of an fp32 value: 0
    where no impulse reaches and the bias is 0, the activation of the fp32 bias otherwise).  No element is left out.  Returns (and
    prints) the largest share of the interval used, the number of pinned elements and the largest K_eff."""
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(mid.shape), f"{name}: shape {tuple(got.shape)} vs {tuple(mid.shape)}"
    if not torch.isfinite(got).all():
        raise OutOfBound(f"{name}: non-finite values")
    err = (got - mid).abs()
    pinned = half == 0
    bad_pin = pinned & (err != 0)
    share = torch.where(pinned, torch.zeros_like(err), err / half.clamp_min(1e-300))
    bad = (~pinned & (err > half)) | bad_pin
    rep = {"used": float(share.max()) if share.numel() else 0.0, "pinned": int(pinned.sum()), "checked": got.numel(),
           "k_eff_max": int(k_eff.max()) if k_eff is not None else -1, "widest": float(half.max())}
    if not quiet:
        print(f"[bound] {name:58s} used={rep['used']:.3f} pinned={rep['pinned']}/{rep['checked']} K_eff<={rep['k_eff_max']} "
              f"widest={rep['widest']:.3e}")
    if bad.any():
        idx = torch.nonzero(bad)
        worst = idx[torch.argmax(torch.where(pinned, err, err / half.clamp_min(1e-300))[bad])]
        w_ = tuple(int(v) for v in worst)
        raise OutOfBound(f"{name}: {int(bad.sum())} of {got.numel()} elements outside their interval ({int(bad_pin.sum())} of them pinned "
                         f"elements that are not bit-exact); worst at {w_}: got {float(got[w_])!r}, mid {float(mid[w_])!r}, "
                         f"half {float(half[w_]):.3e}, err {float(err[w_]):.3e}", index=w_)
    return rep


def escapes(got, mid, half):
    """Whether some element of ``got`` lies outside (mid, half): used to pin WHICH arithmetic ran where no launch key tells -- a
    result computed in a coarser arithmetic must leave the finer one's interval somewhere in a family."""
    return bool(((got.detach().double().cpu() - mid).abs() > half).any())


def locate(idx, w_shape, x, stride=1, padding=1, dims=2):
    """(co, ci, tap, input position) of the one non-zero product behind output element ``idx`` of a forward convolution of an impulse
    member x -- what a failure report points at."""
    stride, padding = _tuple(stride, dims), _tuple(padding, dims)
    co, o = idx[0], idx[1:]
    for tap in itertools.product(*[range(k) for k in w_shape[2:]]):
        i = tuple(o[a] * stride[a] - padding[a] + tap[a] for a in range(dims))
        if all(0 <= i[a] < x.shape[1 + a] for a in range(dims)):
            ci = torch.nonzero(x[(slice(None),) + i])
            if ci.numel():
                return {"co": int(co), "ci": int(ci[0]), "tap": tap, "input": i}
    return None


# ------------------------------------------------------------------------------------------------------------------------------
# the three arithmetics restated (host test only)
# ------------------------------------------------------------------------------------------------------------------------------
def split_hi_lo(v):
    hi = v.float().bfloat16().float()
    lo = (v.float() - hi).bfloat16().float()
    return hi, lo


def emulate(x, w, b, mode, stride=1, padding=1, transposed=None, dims=2, terms=None):
    """The three arithmetics in torch on the CPU: operands rounded with ``.bfloat16()``, partial products exact (float64), one
    accumulation in float64 rounded to fp32 at the end.  ``terms``: optional hook (xh, xl, wh, wl, b) -> the same five, for mutants."""
    stride, padding = _tuple(stride, dims), _tuple(padding, dims)
    if transposed is not None:
        transposed = _tuple(transposed, dims)
    lin = lambda a, k: linear(a, k, stride, padding, transposed, dims)      # noqa: E731
    bd = None if b is None else b.double()
    if mode == "fp32":
        if terms is not None:
            x, _, w, _, bd = terms(x, None, w, None, bd)
        y = lin(x, w)
    else:
        (xh, xl), (wh, wl) = split_hi_lo(x), split_hi_lo(w)
        if terms is not None:
            xh, xl, wh, wl, bd = terms(xh, xl, wh, wl, bd)
        y = lin(xh, wh)
        if mode == "split":
            y = y + lin(xh, wl) + lin(xl, wh)
    if bd is not None:
        y = y + bd.view((-1,) + (1,) * dims)
    return y.float()
