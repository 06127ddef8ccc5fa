"""Float64 reference and bound algebra of the convolutions' backward.  CPU only: nothing here imports the HIP
library or touches a GPU.  The forward algebra, the values, the check and the input-gradient interval come from tests/conv_bound.py.

Weight gradient (``wgrad_nd_kernel``, csrc/train_ops.hip): dW[a][b][tap] = sum_o A[a][o] * B[b][o * s + tap - pad].  With ONE non-zero
position per channel of A and a dense B every element of dW is one product (exactly 0 where the tap lands in the padding), so a
dropped or doubled position, a wrong tap, a wrong row at a corner and a product formed from bf16 halves all move an element out of an
interval that is a few u wide -- or off a pinned value.

Counts (u = 2^-24), each against the kernel as written:

  K_eff = 0          every product is a * 0 or 0 * b = 0, fmaf(., ., 0) = 0, all later sums add zeros: the element is exactly the value
                     the atomic found in dW (``prior``, or 0).
  K_eff = 1, no prior  the accumulator starts at 0 and fmaf(a, b, 0) = RN(a b) is one rounding; the LDS transpose sum, the shuffle, the
                     four waves' sum and the atomic onto a zero-filled dW add exact zeros: the element IS RN(a b).  The float64
                     product of two fp32 values is exact (48 bits), so (a.double() * b.double()).float() is that value.
  otherwise          every term is rounded once (as RN(a b) by the first fmaf of a thread, or inside a later fmaf), and any tree of n
                     terms -- a thread's chain, 32 lanes in sequence, the shuffle, four waves, atomics in any order -- is off by at
                     most (n - 1) u of the sum of magnitudes: half = K_eff u sum|a||b| (1 + 2^-10) (the factor covers the second
                     order).  Onto a non-zero prior every strip's atomic rounds the RUNNING value, which is bounded by
                     |prior| + sum|a||b| and is the result itself only for the last one: + u (|mid| + (J - 1) (|prior| + sum|a||b|))
                     with J = min(K_eff, strips) atomics that add a non-zero partial sum (J = 1: u |mid|, one rounding).
  activation backward in front (``pointwise_kernel``; -ffp-contract=off, so no fused forms):
      ReLU     (y > 0) ? g : 0                an exact select on the kernel's own forward output
      sigmoid  g * (y * (1 - y))              three roundings: 3u of the value
      tanh     g * (1 - y * y)                RN(y y) is off by u y^2 and the subtraction by u |1 - y^2|: together at most u (not
                                              relative: the subtraction cancels), the product one more u: u |g| (1 + |1 - y^2|)
  bias gradient (``channel_sum_kernel`` + ``reduce_partials_kernel<1>``): threads, waves and the workgroup sum in fp64 (n 2^-53: below
      2^-30 for any n here), ONE cast to fp32 per split, then a sequential fp32 sum of the splits in which only non-zero partial sums
      round: half = (1 + ns_nonzero) u sum|g| + 2^-30 sum|g|.  One impulse per channel over the whole batch: exactly that value.
"""
import itertools
import math

import torch

import conv_bound as CB
from conv_bound import U

SLACK = 1.0 + 2.0 ** -10
TPB = 256


def _grid3(shape):
    """(D, h, w) of a [c, h, w] / [c, D, h, w] tensor's grid."""
    return (1,) * (3 - len(shape)) + tuple(int(v) for v in shape)


def _as5(t_, batched):
    """[c, *grid] or [M, c, *grid] (2-D or 3-D grid) -> [M, c, D, h, w]."""
    if not batched:
        t_ = t_[None]
    return t_.reshape(t_.shape[0], t_.shape[1], *_grid3(t_.shape[2:]))


def _taps(kd, ks):
    return torch.tensor(list(itertools.product(range(kd), range(ks), range(ks))), dtype=torch.int64)


def b_index(pos, kd, ks, stride, b_grid):
    """Where the taps of the A positions ``pos`` [N, 3] read B: -> (flat index [N, T] (clamped), in-range mask [N, T])."""
    st = torch.tensor([stride[0], stride[1], stride[1]])
    pd = torch.tensor([kd // 2, ks // 2, ks // 2])
    lim = torch.tensor(b_grid)
    p = pos[:, None, :] * st - pd + _taps(kd, ks)[None]
    ok = ((p >= 0) & (p < lim)).all(-1)
    p = torch.minimum(p.clamp_min(0), lim - 1)
    return (p[..., 0] * b_grid[1] + p[..., 1]) * b_grid[2] + p[..., 2], ok


def wgrad_terms(A, B, kd, ks, stride, cb_total=None, cb_off=0, batched=False):
    """(mid, sum |a||b|, K_eff), each [ca, cb_total, taps] in float64, of dW[a][cb_off + b][tap] = sum_o A[a][o] B[b][o s + tap - pad],
    evaluated from the non-zeros of A (cost ~ non-zeros x cb x taps).  A [ca, *small grid], B [cb, *large grid], or sample batches
    [M, ...] of both (``batched``) whose samples add into one dW (the host's batch loop)."""
    A5, B5 = _as5(A.detach().double().cpu(), batched), _as5(B.detach().double().cpu(), batched)
    M, ca = A5.shape[:2]
    cb, b_grid = B5.shape[1], tuple(B5.shape[2:])
    cb_total = cb if cb_total is None else cb_total
    T = kd * ks * ks
    out = [torch.zeros(ca, cb_total, T, dtype=torch.float64) for _ in range(3)]
    nz_all = A5.nonzero()
    Bf = B5.reshape(M, cb, -1)
    step = max(1, int(4.0e6 // (cb * T)))
    for s0 in range(0, nz_all.shape[0], step):
        nz = nz_all[s0:s0 + step]
        val = A5[tuple(nz.t())]
        flat, ok = b_index(nz[:, 2:], kd, ks, stride, b_grid)
        bsel = Bf[nz[:, 0][:, None, None], torch.arange(cb)[None, :, None], flat[:, None, :]] * ok[:, None, :]     # [N, cb, T]
        prod = val[:, None, None] * bsel
        for dst, src in zip(out, (prod, prod.abs(), (bsel != 0).double())):
            dst[:, cb_off:cb_off + cb].index_add_(0, nz[:, 1], src)
    return tuple(out)


def wgrad_finish(terms, prior=None, ex_terms=(), strips=1):
    """The interval of a dW that received the launches ``terms`` (a list of ``wgrad_terms`` results: sources, samples) on top of
    ``prior`` (None: zeros).  ``ex_terms``: ``wgrad_terms`` of the half-widths A carries (an activation backward in front);
    ``strips``: the strips of the launch, counted where a non-zero prior is added (see the module docstring)."""
    mid = sum(t_[0] for t_ in terms)
    s_abs = sum(t_[1] for t_ in terms)
    k_eff = sum(t_[2] for t_ in terms).round()
    half = k_eff * U * s_abs * SLACK
    for t_ in ex_terms:
        half = half + t_[1] * SLACK
    pin = (k_eff == 1) & (not ex_terms)
    if prior is not None:
        pr = prior.detach().double().cpu().reshape(mid.shape)
        mid = mid + pr
        atomics = k_eff.clamp_max(float(strips))                       # strips that add a non-zero partial sum to the element
        onto = U * (mid.abs() + (atomics - 1.0).clamp_min(0.0) * (pr.abs() + s_abs)) * SLACK
        half = half + torch.where((pr != 0) & (k_eff > 0), onto, torch.zeros_like(mid))
        pin = pin & (pr == 0)
    mid = torch.where(pin, mid.float().double(), mid)                 # RN(a b): the float64 product is exact, one rounding
    half = torch.where(pin | (k_eff == 0), torch.zeros_like(half), half)
    return CB.Interval(mid, half, k_eff, (s_abs,))


def wgrad_interval(A, B, kd, ks, stride, cb_total, cb_off, prior=None, strips=1):
    return wgrad_finish([wgrad_terms(A, B, kd, ks, stride, cb_total, cb_off)], prior, strips=strips)


# ------------------------------------------------------------------------------------------------------------------------------
# activation backward, bias gradient
# ------------------------------------------------------------------------------------------------------------------------------
def act_bwd(g, y, act):
    """(float64 value, half-width or None) of ``pointwise_kernel``'s activation backward on the fp32 gradient g and the fp32 forward
    output y."""
    g, y = g.detach().double().cpu(), y.detach().double().cpu()
    if act == "none":
        return g, None
    if act == "relu":
        return torch.where(y > 0, g, torch.zeros_like(g)), None
    if act == "sigmoid":
        v = g * (y * (1.0 - y))
        return v, 3.0 * U * v.abs() * SLACK
    if act == "tanh":
        d = 1.0 - y * y
        return g * d, U * g.abs() * (1.0 + d.abs()) * SLACK
    raise ValueError(act)


def reduce_splits(total, chunk=2048):
    """ops._reduce_split restated: workgroups per channel of the split per-channel reductions."""
    return int(min(256, max(1, total // chunk)))


def bias_interval(g, ns, ex=None):
    """g [B, C, *grid] (float64 values of the fp32 tensor channel_sum reads; ``ex`` their half-widths) -> Interval [C]."""
    g = g.detach().double().cpu()
    Bn, C = g.shape[:2]
    gf = g.reshape(Bn, C, -1)
    n = gf.shape[2]
    total = Bn * n
    per = -(-total // ns)
    mid, s_abs = gf.sum((0, 2)), gf.abs().sum((0, 2))
    nz = gf.nonzero()
    split = (nz[:, 0] * n + nz[:, 2]) // per
    count = torch.zeros(C, dtype=torch.float64).index_add_(0, nz[:, 1], torch.ones(nz.shape[0], dtype=torch.float64))
    used = torch.zeros(C, ns, dtype=torch.float64)
    used[nz[:, 1], split] = 1.0
    half = (1.0 + used.sum(1)) * U * s_abs + 2.0 ** -30 * s_abs
    if ex is None:
        half = torch.where(count <= 1, torch.zeros_like(half), half)    # one fp32 value: its casts are exact, the rest are zeros
    else:
        half = half + ex.detach().double().cpu().reshape(Bn, C, -1).sum((0, 2))
    return CB.Interval(mid, half, count)


# ------------------------------------------------------------------------------------------------------------------------------
# impulse families for A: flattened positions of the small grid
# ------------------------------------------------------------------------------------------------------------------------------
LANES = (0, 63, 64, 255)


def _unravel(o, grid):
    return (o // (grid[1] * grid[2]), (o // grid[2]) % grid[1], o % grid[2])


def wgrad_classes(o, grid, strips):
    """Labels of the flattened position o of A's grid (D, h, w) in a launch of ``strips`` strips (per = ceil(na / strips))."""
    na = math.prod(grid)
    per = -(-na // strips)
    pos = _unravel(o, grid)
    out = [CB.position_classes(pos, grid, [()] * 3)[0]]
    j, r = o // per, o % per
    if r == 0:
        out.append(("strip", j, "first"))
    if r == per - 1 and o + 1 < na:
        out.append(("strip", j + 1, "before"))
    if o == na - 1:
        out.append(("last",))
    if r % TPB in LANES:
        out.append(("lane", r % TPB))
    if r >= TPB:
        out.append(("second pass",))
    return out


def wgrad_required(grid, strips):
    na = math.prod(grid)
    per = -(-na // strips)
    req = list(CB.required_classes(grid, [()] * 3))
    for j in range(strips):
        req.append(("strip", j, "first"))
        if j:
            req.append(("strip", j, "before"))
    req.append(("last",))
    req += [("lane", r) for r in LANES if r < per]                     # (the first strip is a full one)
    if per > TPB:
        req.append(("second pass",))
    return req


class WgradFamily:
    """``members``: fp32 tensors [ca, D, h, w], one impulse per channel each (the last one: the "few products" member with
    strips + 2 per channel); ``table``: {class: per-channel count}, recounted from the members themselves."""

    def __init__(self, ca, grid, strips, members, few):
        self.ca, self.grid, self.strips, self.members, self.few = ca, tuple(grid), strips, members, few
        self.table = {}
        for x in members:
            for nz in x.reshape(ca, -1).nonzero().tolist():
                for c in wgrad_classes(nz[1], self.grid, strips):
                    self.table.setdefault(c, [0] * ca)[nz[0]] += 1

    def missing(self):
        return [(c, ch) for c in wgrad_required(self.grid, self.strips) for ch in range(self.ca)
                if c not in self.table or self.table[c][ch] == 0]

    def assert_full(self):
        miss = self.missing()
        assert not miss, f"wgrad family ca={self.ca} {self.grid} strips={self.strips}: {len(miss)} empty cells, e.g. {miss[:4]}"


def wgrad_family(ca, grid, strips, seed=0):
    """Positions that together hit every required class; member m puts channel c on position P[(m + c) mod len(P)], so over the
    len(P) members every position -- hence every class -- sees every channel once."""
    grid = tuple(grid)
    na = math.prod(grid)
    per = -(-na // strips)
    gen = torch.Generator().manual_seed(seed)
    need, P = list(wgrad_required(grid, strips)), []

    def take(o):
        if 0 <= o < na and o not in P:
            P.append(o)

    inside = [None if n < 3 else 1 + int(torch.randint(0, n - 2, (1,), generator=gen)) for n in grid]
    for combo in itertools.product(*[[0] if n == 1 else [0, n - 1] + ([inside[a]] if n >= 3 else []) for a, n in enumerate(grid)]):
        take((combo[0] * grid[1] + combo[1]) * grid[2] + combo[2])
    for j in range(strips):
        take(j * per), take(j * per - 1)
        if j in (0, strips - 1):                                         # the lanes, in the first and in the (ragged) last strip
            for r in LANES + (TPB + 63, TPB + 64):
                if j * per + r < min(na, (j + 1) * per):
                    take(j * per + r)
    take(na - 1)
    have = {c for o in P for c in wgrad_classes(o, grid, strips)}
    assert set(need) <= have, f"wgrad_family {grid} strips={strips}: classes without a position: {set(need) - have}"
    L = len(P)
    members = []
    for m in range(L):
        x = torch.zeros(ca, na)
        x[torch.arange(ca), torch.tensor([P[(m + c) % L] for c in range(ca)])] = CB._values(ca, gen)
        members.append(x.view(ca, *grid))
    # few products: per channel one impulse in each strip (wave 0) and two more in other waves of one strip
    few = torch.zeros(ca, na)
    for c in range(ca):
        chosen = []
        for j in range(strips):
            o0, ln = j * per, min(na, (j + 1) * per) - j * per
            chosen.append(o0 + (7 * c + 3) % min(64, ln))
        j = c % strips
        o0, ln = j * per, min(na, (j + 1) * per) - j * per
        for o in (o0 + 64 + c % 64, o0 + 192 + c % 64, o0 + ln - 1, o0 + ln - 2, o0 + ln // 2, o0 + 1, o0):
            if o0 <= o < o0 + ln and o not in chosen and len(chosen) < strips + 2:
                chosen.append(o)
        few[c, torch.tensor(chosen)] = CB._values(len(chosen), gen)
    members.append(few.view(ca, *grid))
    return WgradFamily(ca, grid, strips, members, len(members) - 1)


# ------------------------------------------------------------------------------------------------------------------------------
# wgrad_nd_kernel restated in fp32 (host test only): strip / thread / lane / wave order, with hooks for mutants
# ------------------------------------------------------------------------------------------------------------------------------
def _ordered_sum(vals, gid, n_groups, fma_b=None):
    """Sequential fp32 sums: vals [..., n] (fp32 values as float64), group ids ``gid`` [n] with the elements of a group in summation
    order; -> [..., n_groups].  ``fma_b``: vals are the a operands and fma_b the b operands of acc = fmaf(a, b, acc) (the product is
    exact in float64; the sum is rounded to float64 before fp32, which can differ from a true fmaf by one fp32 ulp on a near-tie and
    not at all where acc = 0: the pins are exact).  Adding a zero is exact, so leaving the zero terms out of ``vals`` changes nothing."""
    order = torch.argsort(gid, stable=True)
    g_sorted = gid[order]
    start = torch.searchsorted(g_sorted, g_sorted)
    rank = torch.arange(len(gid)) - start
    acc = torch.zeros(vals.shape[:-1] + (n_groups,), dtype=torch.float64)
    for i in range(int(rank.max()) + 1 if len(gid) else 0):
        sel = order[rank == i]
        g = gid[sel]
        term = vals[..., sel] if fma_b is None else vals[..., sel] * fma_b[..., sel]
        acc[..., g] = (acc[..., g] + term).float().double()
    return acc


def restate_wgrad(A, B, kd, ks, stride, cb_total, cb_off, strips, dw=None, hook=None):
    """dW after one launch of wgrad_nd_kernel<kd, ks, CAB>, in the kernel's own order: a thread's fmaf chain over its positions
    (o0 + tid + 256 k), the 32-lane sequential sums of the LDS transpose and the shuffle that joins the two halves, the four waves in
    order, one atomic per strip in strip order.  A [ca, *grid], B [cb, *grid] -> fp32 [ca, cb_total, taps].  ``hook``: dict of mutants
    (see tests/test_grad_bound_host.py)."""
    hook = hook or {}
    A5, B5 = _as5(A.detach().float().cpu(), False)[0], _as5(B.detach().float().cpu(), False)[0]
    ca, grid = A5.shape[0], tuple(A5.shape[1:])
    cb, b_grid = B5.shape[0], tuple(B5.shape[1:])
    na, T = math.prod(grid), kd * ks * ks
    per = -(-na // strips)
    Af = A5.reshape(ca, na).double()
    cols = Af.ne(0).any(0).nonzero()[:, 0]                               # positions where some channel is non-zero, ascending
    strip, r = cols // per, cols % per
    if hook.get("drop_last_of_ragged"):                                  # the ragged last strip ends one position early
        keep = cols != na - 1
        cols, strip, r = cols[keep], strip[keep], r[keep]
    if hook.get("double_first_of_strip"):                                # strip j > 0 counts its own first position twice (the
        dup = (r == 0) & (strip > 0)                                     # same thread, one more trip of its loop)
        cols, strip, r = torch.cat([cols, cols[dup]]), torch.cat([strip, strip[dup]]), torch.cat([r, r[dup] + TPB * 4096])
    pos = torch.stack(_unravel(cols, grid), 1)
    flat, ok = b_index(pos, kd, ks, stride, b_grid)
    if "corner_reads_previous_row" in hook:                              # the x = -1 tap of row y reads (y - 1, w - 1): flat index - 1
        st_x, p_x = stride[1], ks // 2
        kx = _taps(kd, ks)[:, 2]
        bx = pos[:, 2:3] * st_x - p_x + kx[None]
        by = pos[:, 1:2] * stride[1] - p_x + _taps(kd, ks)[None, :, 1]
        wrong = (bx == -1) & (by >= 1) & (by < b_grid[1]) & (pos[:, 1:2] == grid[1] - 1)
        bz = pos[:, 0:1] * stride[0] - kd // 2 + _taps(kd, ks)[None, :, 0]
        wrong &= (bz >= 0) & (bz < b_grid[0])
        flat = torch.where(wrong, (bz * b_grid[1] + by) * b_grid[2] - 1, flat)
        ok = ok | wrong
    Bsel = B5.reshape(cb, -1).double()[:, flat] * ok[None]               # [cb, n, T]
    if "parity_tap" in hook:                                             # stride 2: the odd-parity tap taken from the even one
        Bsel = Bsel[:, :, hook["parity_tap"]]
    Bsel = Bsel.permute(0, 2, 1)                                         # [cb, T, n]
    Av = Af[:, cols]                                                     # [ca, n]
    if hook.get("split"):                                                # products formed from bf16 hi / lo halves
        (ah, al), (bh, bl) = CB.split_hi_lo(Av), CB.split_hi_lo(Bsel)
        ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
    tid, k = r % TPB, r // TPB
    thread = strip * TPB + tid
    order = torch.argsort(thread * (1 << 20) + k, stable=True)           # a thread's positions in ascending k
    th_sorted = thread[order]
    uniq, inv = torch.unique(th_sorted, return_inverse=True)
    a_s = Av[:, order][:, None, None, :]
    b_s = Bsel[..., order][None]
    if hook.get("split"):
        a_h, a_l, b_h, b_l = ah[:, order][:, None, None, :], al[:, order][:, None, None, :], bh[..., order][None], bl[..., order][None]
        vals = (a_h * b_h + a_h * b_l + a_l * b_h).float().double().expand(ca, cb, T, len(cols))
        acc = _ordered_sum(vals, inv, len(uniq))
    else:
        acc = _ordered_sum(a_s.expand(ca, cb, T, len(cols)), inv, len(uniq), fma_b=b_s.expand(ca, cb, T, len(cols)))
    # LDS transpose: lanes j0 .. j0 + 31 of a half in sequence, then the shuffle
    u_strip, u_tid = uniq // TPB, uniq % TPB
    half_id = u_strip * 8 + u_tid // 32
    hu, hinv = torch.unique(half_id, return_inverse=True)
    acc = _ordered_sum(acc, hinv, len(hu))
    wave_id = hu // 2
    wu, winv = torch.unique(wave_id, return_inverse=True)
    acc = _ordered_sum(acc, winv, len(wu))
    su, sinv = torch.unique(wu // 4, return_inverse=True)
    acc = _ordered_sum(acc, sinv, len(su))                               # [ca, cb, T, strips with work]
    out = torch.zeros(ca, cb_total, T, dtype=torch.float64) if dw is None else dw.detach().double().cpu().reshape(ca, cb_total, T).clone()
    if "swap_taps" in hook:
        a_, b_, t0, t1 = hook["swap_taps"]
        acc[a_, b_, [t0, t1]] = acc[a_, b_, [t1, t0]]
    off = 0 if hook.get("ignore_cb_off") else cb_off
    for i in range(acc.shape[-1]):                                       # one atomic per strip
        out[:, off:off + cb] = (out[:, off:off + cb] + acc[..., i]).float().double()
    return out.float()


def restate_channel_sum(g, ns, drop_last_split=False):
    """channel_sum_kernel + reduce_partials_kernel<1>: fp64 sums per split, one cast each, a sequential fp32 sum of the splits."""
    Bn, C = g.shape[:2]
    gf = g.detach().double().cpu().reshape(Bn, C, -1).permute(1, 0, 2).reshape(C, -1)
    total = gf.shape[1]
    per = -(-total // ns)
    parts = [gf[:, j * per:min(total, (j + 1) * per)].sum(1).float() for j in range(ns)]
    if ns == 1:
        return parts[0]
    s = torch.zeros(C)
    for p_ in parts[:-1] if drop_last_split else parts:
        s = s + p_
    return s
