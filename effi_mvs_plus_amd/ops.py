"""Tensor-level wrappers over the C ABI.  PyTorch is used for device memory and the current stream only.

All functions take fp32 CUDA (ROCm) tensors without a batch dimension and enqueue on the current
stream.  CPU tensors raise: there is no fallback path.  The feature pyramid's convolutions (image batches) and the wrappers of the
stage-1 cost volume (sample batches, ``_sample_form`` below) also take a leading batch dimension: ONE launch, element i bitwise the
unbatched call on element i.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import threading
from typing import NamedTuple

import weakref

import torch

from . import _lib
from ._lib import EffiLibraryError, check

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
EPI_PLAIN, EPI_GRU_ZR, EPI_GRU_Q, EPI_HEAD, EPI_ADD_UP2, EPI_NHWC = 0, 1, 2, 3, 4, 5
EPI_ADD_SHUF2, EPI_NHWC_ADD_SHUF2 = 9, 10      # split-precision 3x3 entry only: + pixel-shuffled coarser map (aux0 [4*cout,h/2,w/2])
MAX_VIEWS = 12


class KernelProfile:
    """Optional per-launch timing (HIP events on the launching stream) used by bench.py for the roofline
    line: ``keys`` selects which launches are bracketed (None = all); ``records`` collects
    (key, algorithmic work, start event, end event)."""

    def __init__(self, keys=None):
        self.keys = None if keys is None else set(keys)
        self.records = []

    def busy_ms_per_mark(self):
        """Sum of the launches' own durations between consecutive ``ops.mark`` calls (name of the mark that ENDS the span -> ms):
        what the span costs when its kernels run back to back, as in a graph replay -- independent of how fast the host enqueues."""
        torch.cuda.synchronize()
        out, acc = {}, 0.0
        for key, _, e0, e1 in self.records:
            if e0 is None:
                out[key] = out.get(key, 0.0) + acc
                acc = 0.0
            else:
                acc += e0.elapsed_time(e1)
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for key, work, e0, e1 in self.records:
            if e0 is None:                      # a stage mark (see ``mark``), not a launch
                continue
            d = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += work.get("flops", 0.0)
            d["bytes"] += work.get("bytes", 0.0)
        return out


_PROF = None

# Arithmetic of the 3x3 MFMA convolutions: "split" = every fp32 product as hi*hi + hi*lo + lo*hi on the bf16 MFMA with
# fp32 accumulation (~5e-6 of the output scale), "fp32" = v_mfma_f32_16x16x4_f32 (exact products).  Everything else on the
# path (warps, 3-D regularisation, soft-argmin, lookups, epilogues) is plain fp32 in both modes.
# "bf16" = the same kernels as "split" compiled with ONLY the hi*hi term (entry points *_bf16): plain bf16 operands, fp32 accumulation --
# BASELINE.json's "bf16 (MFMA 3D-conv path)" configuration.  It is NOT fp32-grade: its own tolerance is a normalised mean depth
# error <= 1e-2; never the default, never the headline.
PRECISIONS = ("split", "fp32", "bf16")
_PRECISION = os.environ.get("EFFI_MVS_PRECISION", "split")
if _PRECISION not in PRECISIONS:
    raise ValueError(f"EFFI_MVS_PRECISION must be one of {PRECISIONS}, got {_PRECISION!r}")


def set_precision(mode):
    global _PRECISION
    if mode not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {mode!r}")
    _PRECISION = mode


def get_precision():
    return _PRECISION


def uses_split():
    """True when the 3x3 / 3-D MFMA convolutions run on the bf16 matrix cores (split-precision products or bf16 operands)."""
    return _PRECISION in ("split", "bf16")


def _x3(name):
    """The split-precision entry ``name`` of the library, or its plain-bf16-operand twin (suffix _bf16) in "bf16" precision."""
    return getattr(_lib.lib(), name + "_bf16" if _PRECISION == "bf16" else name)


# A/B switches.  Python-level ones (which fused form a module launches) live in ``_PY_OPTS``; kernel-level ones (tile rules, kernel
# forms) in the library's own table (include/effi_mvs_hip.h: effi_set_option).  Both are initialised ONCE from the environment
# (EFFI_<NAME>) and changed afterwards through ``set_option`` -- nothing on a per-call path reads the environment.
_PY_OPTION_DEFAULTS = {"warp_x3": 0, "state_q4": 1, "c1k7_mfma": 1, "k5s2_split": 1, "roll": 1, "conv3d_unaligned_split": 1, "conv3d_s2_split": 1, "fpn_conv0_fused": 1,
                       "fpn_split_head": 1, "csp_pair": 1, "head_taps": 1, "enc_tail": 0, "enc_gen": 1, "reduce_chunk": 2048, "gru_fused": 0, "csp_gen": 0,
                       # small per-pixel launches of the hot path folded into their neighbours (0 = the separate launches, bitwise the same):
                       # head_fused: the depth head's tap sum inside its convolution (1 = where the rule of
                       # BasicUpdateBlock.head_fused_tile finds it faster, 2 = everywhere); head_fused_tile: 0 = that rule, else the tile
                       # (2 / 4 / 8, effi_depth_head_bf16x3_sr); clear_fused: SR border clear inside the context split; setup_fused:
                       # hypotheses + relative projections in one launch; conf_fused: full-size confidence written by the soft-argmin
                       "head_fused": 1, "head_fused_tile": 0, "clear_fused": 1, "setup_fused": 1, "conf_fused": 1,
                       # the feature pyramid over all images of a call in batched launches (module.P_1to8_FeatureNet_Fast; bitwise the same
                       # for every value): 0 = one pass per image, 1 = the measured rule, 2 = every level batched.  Measured
                       # (profiles/fpn_batch_ab.txt): every level batched is the fastest form at 576x800 and at 1184x1600, so the rule is
                       # "every level" and 1 == 2 today
                       "fpn_batch": 1}
_PY_OPTS = {k: int(os.environ.get("EFFI_" + k.upper(), v)) for k, v in _PY_OPTION_DEFAULTS.items()}
LIB_OPTIONS = ("warp_lds_kb", "dyn_form", "dyn_setup_exact", "dyn_xchg", "pixnet_mfma", "force_mr", "mr4_min", "mr4_nt2_max", "mr2_min",
               "wide_tiles", "roll_mr", "roll_zt", "roll_rp", "deconv_mr", "sr_waves", "enc_gen_mr3", "c3_lean", "dyn_win", "roll_slide")


def option(name):
    """Current value of a Python-level switch."""
    return _PY_OPTS[name]


def get_option(name):
    """Value of any switch (None = unset library switch: the built-in rule applies)."""
    if name in _PY_OPTS:
        return _PY_OPTS[name]
    if name not in LIB_OPTIONS:
        raise KeyError(name)
    L = _lib.lib()
    v = L.effi_get_option(name.encode())
    return None if v == L.effi_option_unset() else int(v)


def set_option(name, value):
    """Set a switch (``value=None``: back to the default / unset).  Returns the previous value (for restoring)."""
    before = get_option(name)
    if name in _PY_OPTS:
        _PY_OPTS[name] = _PY_OPTION_DEFAULTS[name] if value is None else int(value)
    else:
        L = _lib.lib()
        check(L.effi_set_option(name.encode(), L.effi_option_unset() if value is None else int(value)), "effi_set_option")
    return before


class options:
    """``with ops.options(warp_lds_kb=0, head_taps=0): ...`` -- switches set for the block, restored after it."""

    def __init__(self, **kw):
        self.kw, self.before = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.before[k] = set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.before.items():
            set_option(k, v)
        return False


# launcher ids and flags of effi_launch_form (include/effi_mvs_hip.h: EFFI_LF_*)
LAUNCHERS = {"x3": 0, "x3_batch": 1, "x3_zb_batch": 2, "x3_pair": 3, "conv2d": 4, "planes3d": 5, "k5s2": 6, "s2_x3": 7, "roll": 8,
             "deconv_x3": 9, "c3_planes": 10, "deconv_k3": 11, "c3_zpt": 12}
LaunchForm = collections.namedtuple("LaunchForm", "rows cols waves planes variant")


def launch_form(launcher, h, w, nt=1, planes=1, count=1, cout=1, sr=False, zb=False, k1=False, s2=False, oct2=False):
    """The tile form the launch rule of ``launcher`` (a key of LAUNCHERS) picks for these sizes under the CURRENT options, as
    LaunchForm(rows per wave, tile columns, waves per workgroup, planes per workgroup or thread, variant): effi_launch_form.  Host
    only: launches nothing, makes no GPU call.  ``h, w``: the map whose tiles the rule counts (the output map of a strided
    convolution, the input map of a transposed one); ``planes``: D; ``count``: images / samples of a batch, 2 for a pair."""
    form = (C.c_int * 5)()
    flags = (1 if sr else 0) | (2 if zb else 0) | (4 if k1 else 0) | (8 if s2 else 0) | (16 if oct2 else 0)
    check(_lib.lib().effi_launch_form(LAUNCHERS[launcher], nt, h, w, planes, count, cout, flags, C.addressof(form)),
          "effi_launch_form")
    return LaunchForm(*form)


def set_profile(p):
    global _PROF
    _PROF = p


def get_profile():
    return _PROF


def _call(key, work, fn, *args):
    p = _PROF
    if p is None or (p.keys is not None and key not in p.keys):
        return fn(*args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn(*args)
    e1.record()
    p.records.append((key, work(), e0, e1))
    return rc


# Caller-owned per-device workspace of the C ABI (include/effi_mvs_hip.h: effi_workspace_bytes / effi_set_workspace): a small
# zero-filled block per device ordinal, allocated here through torch the first time a tensor of that device reaches an op and
# kept alive for the life of the process.  The library itself allocates nothing.
_WORKSPACES = {}
_WS_LOCK = threading.Lock()


def ensure_workspace(index):
    """Register the zero-filled workspace of device ``index`` with the library (idempotent)."""
    if index in _WORKSPACES:
        return
    with _WS_LOCK:
        if index in _WORKSPACES:
            return
        if torch.cuda.is_current_stream_capturing():
            raise EffiLibraryError(f"cuda:{index}: the device's workspace must be registered before stream capture starts "
                                   "(run one pass eagerly, or call ops.ensure_workspace(index), before capturing)")
        L = _lib.lib()
        n = int(L.effi_workspace_bytes())
        with torch.cuda.device(index):
            ws = torch.zeros((n + 3) // 4, device=torch.device("cuda", index), dtype=torch.float32)
            torch.cuda.current_stream().synchronize()       # zero-filled before ANY stream of the device can read it
        check(L.effi_set_workspace(index, C.c_void_p(ws.data_ptr()), n), "effi_set_workspace")
        _WORKSPACES[index] = ws


def _t(x: torch.Tensor, name: str, contiguous=True) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not x.is_cuda:
        raise EffiLibraryError(f"{name}: CPU tensor passed to the HIP path (no CPU fallback exists)")
    idx = x.device.index
    if idx != torch._C._cuda_getDevice():
        # kernels are enqueued on the CURRENT device's stream: a tensor of another device would be a wild pointer there
        raise EffiLibraryError(f"{name}: tensor lives on cuda:{idx} but the current device is cuda:{torch._C._cuda_getDevice()}; "
                               "call inside `with torch.cuda.device(tensor.device):` (the public modules do this themselves)")
    if idx not in _WORKSPACES:
        ensure_workspace(idx)
    if x.dtype != torch.float32:
        raise TypeError(f"{name}: fp32 only (got {x.dtype}); the reference path is fp32 (models/module.py:318)")
    if contiguous and not x.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return x


def _p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)


def _first_cuda_tensor(obj, depth=0):
    if isinstance(obj, torch.Tensor):
        return obj if obj.is_cuda else None
    if depth < 3:
        if isinstance(obj, dict):
            obj = obj.values()
        if isinstance(obj, (list, tuple)) or type(obj).__name__ == "dict_values":
            for o in obj:
                t_ = _first_cuda_tensor(o, depth + 1)
                if t_ is not None:
                    return t_
    return None


def on_tensor_device(fn):
    """Decorator of the public entry points (module ``forward``s, the reference-named functions): run with the device of the
    first CUDA tensor among the arguments as the current device, as stock PyTorch operators do.  The kernels are enqueued on the
    current device's stream, so a model on cuda:1 called while cuda:0 is current would otherwise launch against foreign
    pointers.  (Replicas of nn.DataParallel already run under their own device.)"""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        t_ = _first_cuda_tensor(args)
        if t_ is None and kwargs:
            t_ = _first_cuda_tensor(kwargs)
        if t_ is None or t_.device.index == torch._C._cuda_getDevice():
            return fn(*args, **kwargs)
        with torch.cuda.device(t_.device):
            return fn(*args, **kwargs)
    return wrapper


# Independent kernel chains (the mask head, the preparation of the stages' GRU inputs, the pyramid passes of the odd views) CAN
# be enqueued on a second HIP stream (``Branch``).  Off by default: inside a captured graph every cross-stream edge costs ~5 us
# (fork) / ~11 us (join) of idle GPU, and a graph with ANY such edge replays ~3 % slower than the linear graph of the same
# kernels (measured at 1600x1184: 2.64 -> 2.57 ms; at 800x576: 1.40 -> 1.31 ms) -- the chains that do overlap well share ONE
# grid instead (effi_encoder_inputs_f32, effi_*_pair_f32).  A second stream pays off when several views are in flight at once
# (bench.py --in-flight 3: 2.31 ms per view with branches, 2.43 without).  EFFI_MVS_BRANCHES=1 / set_branches(True) turn it on;
# results are identical either way (no atomics; every kernel sees its producers through stream events).
_BRANCHES = os.environ.get("EFFI_MVS_BRANCHES", "0") != "0"
_SIDE_STREAMS = {}


def set_branches(enabled):
    """Enable / disable the second stream (profiling passes want serial kernel durations)."""
    global _BRANCHES
    _BRANCHES = bool(enabled)


def get_branches():
    return _BRANCHES


class Branch:
    """``with Branch() as br: <enqueue the side chain>`` ... main chain ... ``br.join(outputs...)``.

    The side stream first waits for everything already enqueued on the current (main) stream; ``join`` makes the main
    stream wait for the side chain and tells the caching allocator that the given side-allocated tensors are now used on
    the main stream."""

    def __init__(self):
        self.enabled = _BRANCHES and torch.cuda.is_available()      # CPU tensors must reach the ops' own loud failure
        if self.enabled:
            self.main = torch.cuda.current_stream()
            key = (self.main.device.index, self.main.cuda_stream)
            side = _SIDE_STREAMS.get(key)
            if side is None:
                side = _SIDE_STREAMS[key] = torch.cuda.Stream(device=self.main.device)
            self.side = side
            self._ctx = None

    def __enter__(self):
        if self.enabled:
            self.side.wait_stream(self.main)
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.enabled:
            self._ctx.__exit__(*exc)
        return False

    def join(self, *tensors):
        if self.enabled:
            self.main.wait_stream(self.side)
            for t_ in tensors:
                if t_ is not None:
                    t_.record_stream(self.main)


# Optional stage markers (bench.py's "ms per cost-volume stage"): forward_hot calls mark() at the stage boundaries; events are only
# recorded while a list is installed (never during graph capture).
_MARKS = None


def set_marks(marks):
    global _MARKS
    _MARKS = marks


def mark(name):
    if _PROF is not None and _PROF.keys is None:
        _PROF.records.append((name, {}, None, None))
    if _MARKS is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        _MARKS.append((name, ev))


def _stream():
    # raw hipStream_t of torch's current stream on the current device (fast path: ~1 us instead of the
    # ~8 us of torch.cuda.current_stream().cuda_stream; this is called once per kernel launch)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _int_array(vals):
    return (C.c_int * len(vals))(*vals)


# ---------------------------------------------------------------------------------------------
def compose_rel_proj(pairs: torch.Tensor) -> torch.Tensor:
    """pairs [N,2,4,4] -> rt [N-1,12]  (K.[R|t] then P_src . P_ref^-1).  Sample batch: [n,N,2,4,4] -> [n,N-1,12], one launch."""
    pairs = _samples(pairs)
    n, ps = _in(pairs, 4, "pairs")
    nv = pairs.shape[-4]
    rt = torch.empty((() if n is None else (n,)) + (nv - 1, 12), device=pairs.device, dtype=torch.float32)
    _launch("effi_compose_rel_proj_f32", (_p(pairs), nv, _p(rt)), n, lambda: (ps, rt.stride(0)))
    return rt


def compose_rel_proj_stages(pairs_list):
    """``compose_rel_proj`` of up to 4 stages' [N,2,4,4] tensors in one launch -> list of rt [N-1,12] (views of one buffer)."""
    for p_ in pairs_list:
        _t(p_, "pairs")
    n = pairs_list[0].shape[0]
    if len(pairs_list) > 4 or any(p_.shape[0] != n for p_ in pairs_list):
        raise ValueError("compose_rel_proj_stages: up to 4 stages with the same number of views")
    rt = torch.empty(len(pairs_list), n - 1, 12, device=pairs_list[0].device, dtype=torch.float32)
    check(_lib.lib().effi_compose_rel_proj_stages_f32(_ptr_array(pairs_list), len(pairs_list), n, _p(rt), _stream()),
          "effi_compose_rel_proj_stages_f32")
    return [rt[k] for k in range(len(pairs_list))]


# ---- sample forms: a tensor argument is ONE item, or a batch [n, ...] of them ----------------------------------------------------
def _sample_form(x, nd, name):
    """Sample form of one tensor argument, read from its shape and strides alone: ``nd`` dims = ONE item (beside batched tensors:
    shared by all samples, stride 0), ``nd + 1`` dims = [n, ...] with contiguous items at ANY uniform item stride (a slice of a
    larger allocation is fine; an expanded leading dimension, or n == 1, is stride 0) -> (n or None, item stride in floats)."""
    if x.dim() == nd:
        if not x.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        return None, 0
    if x.dim() != nd + 1 or x.shape[0] < 1:
        raise ValueError(f"{name}: expected {nd} dimensions, or {nd + 1} with a leading sample dimension, got {tuple(x.shape)}")
    if not x[0].is_contiguous():
        raise ValueError(f"{name}: every sample of a batch must be contiguous (the sample stride itself is free)")
    return x.shape[0], (x.stride(0) if x.shape[0] > 1 else 0)


def _sample_count(counts, what):
    """The one sample count of a call's tensors (None entries = unbatched tensors); ValueError when they disagree."""
    ns = {c for c in counts if c is not None}
    if len(ns) > 1:
        raise ValueError(f"{what}: sample counts differ ({sorted(ns)})")
    return ns.pop() if ns else None


def _sample_forms(tensors, nd, name):
    """``_sample_form`` of several tensors of one call -> (their one sample count or None, [item strides])."""
    forms = [_sample_form(x, nd, name) for x in tensors]
    return _sample_count([f[0] for f in forms], name), [f[1] for f in forms]


def _in(x, nd, name):
    """An input tensor of a wrapper: the device / dtype / workspace check (``_t``), then its sample form."""
    _t(x, name, contiguous=False)
    return _sample_form(x, nd, name)


def _depth_strides(depth, n, D, h, w):
    """Depth hypotheses -> (tensor, hypothesis stride, pixel stride, sample stride).  Unbatched call (``n`` None): [D] (uniform),
    [D,h,w] contiguous, or an expanded [D,h,w] view.  Batched call: [D] shared by all samples, [n,D], or [n,D,h,w] (contiguous, or
    expanded over the map as the reference passes them); these are checked against ``D`` and the map size."""
    k = 0 if n is None else 1                   # position of the hypothesis dimension in the per-pixel forms
    if depth.dim() not in (1, k + 1, k + 3):
        raise ValueError("depth hypotheses: expected " + ("[D] or [D,h,w]" if n is None else "[D], [n,D] or [n,D,h,w]")
                         + f", got {tuple(depth.shape)}")
    if n is not None:
        per_pixel = depth.dim() == 4
        if depth.shape[min(1, depth.dim() - 1)] != D or (per_pixel and tuple(depth.shape[2:]) != (h, w)):
            raise ValueError(f"depth hypotheses: {tuple(depth.shape)} do not hold D = {D} hypotheses" + (f" on a {h} x {w} map" if per_pixel else ""))
        if depth.dim() > 1 and depth.shape[0] != n:
            raise ValueError(f"depth hypotheses: sample counts differ ({n} and {depth.shape[0]})")
    if depth.dim() == 1:
        return (depth if depth.is_contiguous() else depth.contiguous()), 1, 0, 0
    st = depth.stride()
    if depth.dim() == 2:
        if st[1] != 1 or st[0] < 0:
            depth = depth.contiguous()
        dds, dps = 1, 0
    elif st[k + 1] == 0 and st[k + 2] == 0 and min(st) >= 0:
        dds, dps = st[k], 0
    else:
        if not depth.is_contiguous():
            depth = depth.contiguous()
        dds, dps = h * w, 1
    return depth, dds, dps, (depth.stride(0) if n is not None and n > 1 else 0)


def _launch(name, args, n, tail, key=None, work=None, x3=False):
    """The one C call of a wrapper: the plain entry ``name`` for an unbatched call (``n`` None), else its ``_batch`` twin with the
    sample count and the strides of ``tail()`` appended.  ``key`` / ``work``: the profile record of ``_call``; ``x3``: a
    split-precision entry (``_x3``)."""
    if n is not None:
        name, args = name + "_batch", args + (n,) + tail()
    fn = _x3(name) if x3 else getattr(_lib.lib(), name)
    check(fn(*args, _stream()) if key is None else _call(key, work, fn, *args, _stream()), name)


def _long_array(vals):
    return (C.c_long * len(vals))(*[int(v) for v in vals])


def _batch_out(out, shape, dev, name):
    """Output of a batched convolution: allocated [n, ...], or the caller's (images contiguous, uniform image stride)."""
    if out is None:
        return torch.empty(shape, device=dev, dtype=torch.float32)
    _t(out, name, contiguous=False)
    if tuple(out.shape) != tuple(shape) or not out[0].is_contiguous() or (shape[0] > 1 and out.stride(0) < out[0].numel()):
        raise ValueError(f"{name}: expected {tuple(shape)} with contiguous, non-overlapping images")
    return out


def _out(n, shape, dev, out, name):
    """Output ``shape`` of a convolution: unbatched (``n`` None) the caller's ``out`` as it is, or allocated; [n, ...] in a batched
    call (``_batch_out``)."""
    if n is not None:
        return _batch_out(out, (n,) + shape, dev, name)
    return torch.empty(shape, device=dev, dtype=torch.float32) if out is None else out


def as_samples(tensors):
    """n per-sample tensors of one shape -> ONE [n, ...] view over them when they sit at a uniform sample stride inside one
    allocation (no copy), else None.  The batched wrappers pass list arguments through it (``_samples``)."""
    t0 = tensors[0]
    if len(tensors) == 1:
        return t0.unsqueeze(0)
    if any(t.shape != t0.shape or t.stride() != t0.stride() or t.dtype != t0.dtype or t.device != t0.device
           or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr() for t in tensors):
        return None
    step = tensors[1].storage_offset() - t0.storage_offset()
    if step < 0 or any(t.storage_offset() - t0.storage_offset() != i * step for i, t in enumerate(tensors)):
        return None
    return t0.as_strided((len(tensors),) + tuple(t0.shape), (step,) + tuple(t0.stride()), t0.storage_offset())


def _samples(x):
    """A wrapper's tensor argument given as a list of per-sample tensors -> [n, ...]: ``as_samples``' view when the samples sit at a
    uniform stride in one allocation, else one gathered copy (``torch.stack``).  Tensors (and None) pass through."""
    if not isinstance(x, (list, tuple)):
        return x
    if not x:
        raise ValueError("an empty list of samples")
    v = as_samples(x)
    return torch.stack(list(x)) if v is None else v


def cascade_setup(disp_range, D, pairs_list):
    """``stage1_hypotheses`` and ``compose_rel_proj_stages`` in one launch -> ((depths [D], intervals [5]), [rt [N-1,12], ...]).
    Sample batch: disp_range [n,R] and pairs [n,N,2,4,4] -> ((depths [n,D], intervals [n,5]), [rt [n,N-1,12], ...]), one launch."""
    disp_range, pairs_list = _samples(disp_range), [_samples(p_) for p_ in pairs_list]
    n, rs = _in(disp_range, 1, "disp_range")
    strides = []
    for p_ in pairs_list:
        m, ps = _in(p_, 4, "pairs")
        if m != n:
            raise ValueError(f"cascade_setup: sample counts differ ({n} ranges, {m} camera sets)")
        strides.append(ps)
    nv = pairs_list[0].shape[-4]
    if len(pairs_list) > 4 or any(p_.shape[-4] != nv for p_ in pairs_list):
        raise ValueError("cascade_setup: up to 4 stages with the same number of views")
    dev, lead = disp_range.device, () if n is None else (n,)
    depths = torch.empty(lead + (D,), device=dev, dtype=torch.float32)
    intervals = torch.empty(lead + (5,), device=dev, dtype=torch.float32)   # 3 intervals, depth_min_, depth_max_
    rt = torch.empty(lead + (len(pairs_list), nv - 1, 12), device=dev, dtype=torch.float32)
    _launch("effi_cascade_setup_f32", (_p(disp_range), disp_range.shape[-1], D, _p(depths), _p(intervals), _ptr_array(pairs_list),
                                       len(pairs_list), nv, _p(rt)), n, lambda: (rs, D, 5, _long_array(strides), rt.stride(0)))
    return (depths, intervals), [rt.select(-3, k) for k in range(len(pairs_list))]


def rel_proj(src_proj: torch.Tensor, ref_proj: torch.Tensor) -> torch.Tensor:
    _t(src_proj, "src_proj"), _t(ref_proj, "ref_proj")
    rt = torch.empty(12, device=src_proj.device, dtype=torch.float32)
    check(_lib.lib().effi_rel_proj_f32(_p(src_proj), _p(ref_proj), _p(rt), _stream()), "effi_rel_proj_f32")
    return rt


def to_nhwc(feats):
    """list of planar [C,h,w] maps -> list of channel-last [h,w,C] maps.  A map that is already channel-last in memory
    (torch.channels_last) is passed through without a copy; the others (of one shape) are transposed into ONE allocation.  Sample
    batch: [n,C,h,w] maps -> [n,h,w,C] maps (the transposed ones at one uniform sample stride, as the batched warp wants them)."""
    batched = feats[0].dim() == 4
    out, todo = [], []
    for f in feats:
        _t(f, "feature", contiguous=False)
        if f.dim() != feats[0].dim() or f.dim() not in (3, 4) or (batched and f.shape[0] != feats[0].shape[0]):
            raise ValueError("to_nhwc: expected [C,h,w] maps, or [n,C,h,w] maps of one n")
        last = f.movedim(-3, -1)
        if f.shape[-3] > 1 and (last[0] if batched else last).is_contiguous():
            out.append(last)
        else:
            todo.append(len(out))
            out.append(None)
    if not todo:
        return out
    shape = feats[todo[0]].shape
    if any(feats[i].shape != shape for i in todo):
        raise ValueError("to_nhwc: the planar feature maps of a call must share one shape")
    C_, h, w = shape[-3:]
    dst = torch.empty(tuple(shape[:-3]) + (len(todo), h, w, C_), device=feats[0].device, dtype=torch.float32)
    src_l, dst_l = [], []
    for j, i in enumerate(todo):
        out[i] = dst.select(-4, j)
        for s_, d_ in zip(feats[i] if batched else (feats[i],), out[i] if batched else (out[i],)):
            if not s_.is_contiguous():
                raise ValueError("feature map must be planar-contiguous or channels-last")
            src_l.append(s_)
            dst_l.append(d_)
    for k in range(0, len(src_l), MAX_VIEWS + 1):
        s_, d_ = src_l[k:k + MAX_VIEWS + 1], dst_l[k:k + MAX_VIEWS + 1]
        check(_lib.lib().effi_planar_to_nhwc_f32(_ptr_array(s_), _ptr_array(d_), len(s_), C_, h * w, _stream()), "effi_planar_to_nhwc_f32")
    return out


def homo_warp(src_nhwc, rt, depth, D):
    h, w, Cc = src_nhwc.shape
    _t(src_nhwc, "src_nhwc"), _t(rt, "rt"), _t(depth, "depth", contiguous=False)
    depth, dds, dps, _ = _depth_strides(depth, None, D, h, w)
    out = torch.empty(Cc, D, h, w, device=src_nhwc.device, dtype=torch.float32)
    check(_lib.lib().effi_homo_warp_f32(_p(src_nhwc), _p(rt), _p(depth), dds, dps, Cc, h, w, D, _p(out), _stream()),
          "effi_homo_warp_f32")
    return out


def homo_warp_bwd(rt, depth, D, grad_out, h, w):
    """Backward of ``homo_warp`` w.r.t. the source features: grad_out [C,D,h,w] -> grad_src [h,w,C] (scope row n2)."""
    _t(rt, "rt"), _t(depth, "depth", contiguous=False), _t(grad_out, "grad_out")
    Cc = grad_out.shape[0]
    depth, dds, dps, _ = _depth_strides(depth, None, D, h, w)
    g_src = torch.zeros(h, w, Cc, device=grad_out.device, dtype=torch.float32)
    check(_lib.lib().effi_homo_warp_bwd_f32(_p(rt), _p(depth), dds, dps, Cc, h, w, D, _p(grad_out), _p(g_src), _stream()),
          "effi_homo_warp_bwd_f32")
    return g_src


def warpcorr_views(ref_nhwc, srcs_nhwc, rt, depth, D, x3=False):
    """-> (sim_views [S,D,h,w], entropy [S,h,w]).  Sample batch: ref [n,h,w,C], sources [n,h,w,C] each, rt [n,S,12], depth [D]
    (shared), [n,D] or [n,D,h,w] -> (sim_views [n,S,D,h,w], entropy [n,S,h,w]) in ONE launch when the sources share one sample
    stride (else one launch per sample).  ``x3``: in "split" / "bf16" precision use the matrix-core form
    (``effi_warpcorr_views_x3_f32``: correlations of the tap pixels as split-precision MFMAs, then interpolated) -- inference only;
    the default is the exact fp32 kernel (what training and the exact-fp32 precision use)."""
    ref_nhwc, srcs_nhwc, rt, depth = _samples(ref_nhwc), [_samples(s_) for s_ in srcs_nhwc], _samples(rt), _samples(depth)
    n, rs = _in(ref_nhwc, 3, "ref_nhwc")
    h, w, Cc = ref_nhwc.shape[-3:]
    S = len(srcs_nhwc)
    sstr = set()
    for s_ in srcs_nhwc:
        m, ss = _in(s_, 3, "src_nhwc")
        if tuple(s_.shape[-3:]) != (h, w, Cc):
            raise ValueError("source / reference feature shapes differ")
        if m != n:
            raise ValueError(f"warpcorr_views: sample counts differ ({n} and {m})")
        sstr.add(ss)
    m, rts = _in(rt, 2, "rt")
    if m != n:
        raise ValueError(f"warpcorr_views: sample counts differ ({n} maps, {m} projection sets)")
    if rt.shape[-2] != S:
        raise ValueError("Different number of images and projection matrices")
    _t(depth, "depth", contiguous=False)
    if len(sstr) > 1:               # sources at different sample strides: not expressible as pointer list + ONE stride -> per sample
        outs = [warpcorr_views(ref_nhwc[b], [s_[b] for s_ in srcs_nhwc], rt[b], depth if depth.dim() == 1 else depth[b], D, x3=x3)
                for b in range(n)]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
    depth, dds, dps, dss = _depth_strides(depth, n, D, h, w)
    return _warpcorr_views((_p(ref_nhwc), _ptr_array(srcs_nhwc)), False, S, Cc, h, w, rt, depth, dds, dps, D, x3, n,
                           lambda sim, ent: (rs, sstr.pop(), rts, dss, sim.stride(0), ent.stride(0)))


def _warpcorr_views(views, tbl, S, Cc, h, w, rt, depth, dds, dps, D, x3, n=None, tail=None):
    """The outputs, the profile record and the one C call of ``warpcorr_views`` (``views``: reference and source pointers) and of
    ``warpcorr_views_tbl`` (``views``: the row of a ViewTable; ``tbl``).  ``n`` / ``tail(sim, ent)``: sample count and strides."""
    lead, reps = (() if n is None else (n,)), n or 1
    sim = torch.empty(lead + (S, D, h, w), device=rt.device, dtype=torch.float32)
    ent = torch.empty(lead + (S, h, w), device=rt.device, dtype=torch.float32)
    work = lambda: {"flops": reps * S * D * h * w * (10.0 * Cc + 20), "bytes": 4.0 * reps * h * w * (S * Cc + Cc + S * D + S)}
    x3 = bool(x3) and uses_split()
    _launch("effi_warpcorr_views" + ("_x3" if x3 else "") + ("_tbl" if tbl else "") + "_f32",
            views + (S, _p(rt), _p(depth), dds, dps, Cc, h, w, D, _p(sim), _p(ent)) + ((int(_PRECISION == "bf16"),) if x3 else ()),
            n, lambda: tail(sim, ent), key=f"warpcorr_views_c{Cc}", work=work)
    return sim, ent


def warpcorr_views_bwd(ref_nhwc, srcs_nhwc, rt, depth, D, grad_sim):
    """Backward of ``warpcorr_views``' similarity output (scope row n2): grad_sim [S,D,h,w] -> (grad_ref [h,w,C], [grad_src_v [h,w,C]])."""
    h, w, Cc = ref_nhwc.shape
    S = len(srcs_nhwc)
    _t(ref_nhwc, "ref_nhwc"), _t(rt, "rt"), _t(depth, "depth", contiguous=False), _t(grad_sim, "grad_sim")
    for s_ in srcs_nhwc:
        _t(s_, "src_nhwc")
    if tuple(grad_sim.shape) != (S, D, h, w):
        raise ValueError(f"grad_sim {tuple(grad_sim.shape)} does not match (S, D, h, w) = {(S, D, h, w)}")
    depth, dds, dps, _ = _depth_strides(depth, None, D, h, w)
    g_ref = torch.zeros_like(ref_nhwc)          # accumulated per source view by the windowed kernel
    g_src = [torch.zeros_like(s_) for s_ in srcs_nhwc]
    check(_lib.lib().effi_warpcorr_views_bwd_f32(_p(ref_nhwc), _ptr_array(srcs_nhwc), S, _p(rt), _p(depth), dds, dps, Cc, h, w, D,
                                                  _p(grad_sim), _p(g_ref), _ptr_array(g_src), _stream()), "effi_warpcorr_views_bwd_f32")
    return g_ref, g_src


VIEW_TABLE_ROW = MAX_VIEWS + 2        # include/effi_mvs_hip.h: EFFI_VIEW_TABLE_ROW


class ViewTable:
    """The feature maps of one reference view's (reference, sources) item as a table of device pointers the warp kernels read
    WHEN THEY RUN (``effi_warpcorr_views_tbl_f32`` / ``effi_warpcorr_dyn_tbl_f32``): ``ptrs`` int64 [n_stages, VIEW_TABLE_ROW],
    row s = channel-last maps [h_s, w_s, C_s] of the reference (entry 0) and of the sources (entries 1..S).  A captured graph of
    the hot path keeps the table's address, not the maps': ``set()`` points it at another item's cached maps with one small
    launch on the current stream (scan_eval.py) -- no 150-MB copy into static inputs.  ``shapes``: per stage (C, h, w).

    The maps are NOT kept alive by the table: whoever calls ``set`` owns them until every replay that reads them has finished
    (scan_eval.ScanFeatureCache does, per scan)."""

    def __init__(self, shapes, n_views, device, ptrs=None):
        if not 2 <= n_views <= MAX_VIEWS + 1 or not 1 <= len(shapes) <= 4:
            raise ValueError("ViewTable: 2..MAX_VIEWS+1 views, 1..4 stages")
        self.shapes = [tuple(int(v) for v in sh) for sh in shapes]
        self.n_views = int(n_views)
        self.ptrs = torch.zeros(len(shapes), VIEW_TABLE_ROW, dtype=torch.int64, device=device) if ptrs is None else ptrs
        if tuple(self.ptrs.shape) != (len(shapes), VIEW_TABLE_ROW) or self.ptrs.dtype != torch.int64 or not self.ptrs.is_contiguous():
            raise ValueError("ViewTable: ptrs must be a contiguous int64 [n_stages, VIEW_TABLE_ROW] tensor")

    def rebind(self, ptrs):
        """The same geometry over another pointer tensor (a graph slot's static copy)."""
        return ViewTable(self.shapes, self.n_views, ptrs.device, ptrs)

    def set(self, maps):
        """maps[s][v]: channel-last [h_s, w_s, C_s] fp32 map of view v (0 = reference) at stage s."""
        vals = []
        for s_, (sh, row) in enumerate(zip(self.shapes, maps)):
            if len(row) != self.n_views:
                raise ValueError(f"ViewTable.set: stage {s_} has {len(row)} maps, the table was built for {self.n_views} views")
            for m in row:
                _t(m, "feature map")
                if tuple(m.shape) != (sh[1], sh[2], sh[0]):
                    raise ValueError(f"ViewTable.set: stage {s_} map {tuple(m.shape)} is not channel-last {(sh[1], sh[2], sh[0])}")
            vals += [m.data_ptr() for m in row] + [0] * (VIEW_TABLE_ROW - len(row))
        arr = (C.c_void_p * len(vals))(*vals)
        check(_lib.lib().effi_view_table_set(C.c_void_p(self.ptrs.data_ptr()), arr, len(vals), _stream()), "effi_view_table_set")

    def row(self, s_):
        return C.c_void_p(self.ptrs.data_ptr() + 8 * VIEW_TABLE_ROW * s_)


def warpcorr_views_tbl(table, stage, rt, depth, D, x3=False):
    """``warpcorr_views`` reading its reference / source maps through row ``stage`` of a ViewTable."""
    Cc, h, w = table.shapes[stage]
    S = table.n_views - 1
    _t(rt, "rt"), _t(depth, "depth", contiguous=False)
    if rt.shape[0] != S:
        raise ValueError("Different number of images and projection matrices")
    depth, dds, dps, _ = _depth_strides(depth, None, D, h, w)
    return _warpcorr_views((table.row(stage),), True, S, Cc, h, w, rt, depth, dds, dps, D, x3)


def _vw_shift(view_w, h, w):
    """k of view weights [S, h >> k, w >> k] on an h x w map; anything else is refused (the library answers EFFI_ERR_BADARG)."""
    vh, vw = view_w.shape[1], view_w.shape[2]
    shift = 0
    while (vh << shift) < h:
        shift += 1
    if (vh << shift) != h or (vw << shift) != w:
        raise ValueError(f"view weights {vh}x{vw} are not a power-of-two downsampling of {h}x{w}")
    return shift


def _warpcorr_dyn(entry, views, S, Cc, h, w, rt, cur_depth, interval, view_w, D):
    """The body of ``warpcorr_dyn`` (``views``: reference and source pointers) and ``warpcorr_dyn_tbl`` (the row of a ViewTable)."""
    _t(rt, "rt"), _t(cur_depth, "cur_depth"), _t(interval, "interval"), _t(view_w, "view_w")
    if view_w.shape[0] != S or rt.shape[0] != S:
        raise ValueError("view weights / projections / sources disagree on the number of views")
    shift = _vw_shift(view_w, h, w)
    sim = torch.empty(D, h, w, device=rt.device, dtype=torch.float32)
    samples = torch.empty(D, h, w, device=rt.device, dtype=torch.float32)
    work = lambda: {"flops": S * D * h * w * (10.0 * Cc + 20), "bytes": 4.0 * h * w * (S * Cc + Cc + 2 * D + 1 + S / 4.0 ** shift)}
    check(_call(f"warpcorr_dyn_c{Cc}", work, getattr(_lib.lib(), entry), *views, S, _p(rt), _p(cur_depth), _p(interval), _p(view_w), shift,
                Cc, h, w, D, _p(sim), _p(samples), _stream()), entry)
    return sim, samples


def warpcorr_dyn_tbl(table, stage, rt, cur_depth, interval, view_w, D):
    """``warpcorr_dyn`` reading its reference / source maps through row ``stage`` of a ViewTable."""
    Cc, h, w = table.shapes[stage]
    return _warpcorr_dyn("effi_warpcorr_dyn_tbl_f32", (table.row(stage),), table.n_views - 1, Cc, h, w, rt, cur_depth, interval, view_w, D)


def pixelwise_net(entropy, params):
    """entropy [n,h,w] -> weights [n,h,w]; a sample batch [b,S,h,w] is the same launch on b * S planes."""
    if entropy.dim() == 4:
        _t(entropy, "entropy")
        return pixelwise_net(entropy.flatten(0, 1), params).view(entropy.shape)
    n, h, w = entropy.shape
    _t(entropy, "entropy"), _t(params, "params")
    out = torch.empty_like(entropy)
    check(_lib.lib().effi_pixelwise_net_f32(_p(entropy), _p(params), n, h, w, _p(out), _stream()),
          "effi_pixelwise_net_f32")
    return out


def view_aggregate(sim_views, weights):
    """sum_v sim_v w_v / (sum_v w_v + 1e-6); ``weights`` None = the plain mean over the views (pixel_wise_net = None).  Sample
    batch: sim_views [n,S,D,h,w], weights [n,S,h,w] or None -> [n,D,h,w], one launch."""
    sim_views, weights = _samples(sim_views), _samples(weights)
    n, ss = _in(sim_views, 4, "sim_views")
    S, D, h, w = sim_views.shape[-4:]
    ws = 0
    if weights is not None:
        m, ws = _in(weights, 3, "weights")
        if m != n or weights.shape[-3] != S:
            raise ValueError(f"view_aggregate: sample / view counts differ ({n} x {S} volumes, weights {tuple(weights.shape)})")
    out = torch.empty((() if n is None else (n,)) + (D, h, w), device=sim_views.device, dtype=torch.float32)
    _launch("effi_view_aggregate_f32", (_p(sim_views), _p(weights), S, D, h * w, _p(out)), n, lambda: (ss, ws, out.stride(0)))
    return out


def warpcorr_dyn(ref_nhwc, srcs_nhwc, rt, cur_depth, interval, view_w, D):
    """cur_depth [h,w]; interval: 1-element tensor; view_w [S,h>>k,w>>k] -> (sim [D,h,w], samples [D,h,w])."""
    h, w, Cc = ref_nhwc.shape
    _t(ref_nhwc, "ref_nhwc")
    for s in srcs_nhwc:
        _t(s, "src_nhwc")
    return _warpcorr_dyn("effi_warpcorr_dyn_f32", (_p(ref_nhwc), _ptr_array(srcs_nhwc)), len(srcs_nhwc), Cc, h, w, rt, cur_depth, interval,
                         view_w, D)


def _conv_out(size, stride):
    """Output extent of a 3-tap pad-1 (or 5-tap pad-2) convolution at ``stride``."""
    return (size - 1) // stride + 1


def _channels(srcs, axis):
    """Channel counts of a convolution's concatenated sources -> (the C array the entries take, their sum)."""
    chans = [s_.shape[axis] for s_ in srcs]
    return _int_array(chans), sum(chans)


def _vol_inputs(srcs, skip, what):
    """The [C,D,h,w] sources and the skip volume of a 3-D convolution, or sample batches [n,C,D,h,w] of them ->
    (n or None, source strides, skip stride, (D, h, w))."""
    for s_ in srcs:
        _t(s_, what + " input", contiguous=False)
    n, sstr = _sample_forms(srcs, 4, what + " input")
    if n is not None and any(s_.dim() != 5 for s_ in srcs):
        raise ValueError(f"{what}: every source of a batched call must be [n,C,D,h,w]")
    if any(s_.shape[-3:] != srcs[0].shape[-3:] for s_ in srcs):
        raise ValueError(f"{what}: the sources must share one (D, h, w), got {[tuple(s_.shape) for s_ in srcs]}")
    ks = 0
    if skip is not None:
        m, ks = _in(skip, 4, "skip")
        if m != n:
            raise ValueError(f"{what}: skip must be [n, ...] with n = {n}")
    return n, sstr, ks, tuple(srcs[0].shape[-3:])


def _vol_out(n, shape, dev, skip, out=None):
    """Output volume ``shape`` of a 3-D convolution ([n, ...] in a batched call, where it may be the caller's ``out``)."""
    out = _out(n, shape, dev, out, "conv3d output")
    if skip is not None:
        assert skip.shape == out.shape, f"skip {tuple(skip.shape)} vs out {tuple(out.shape)}"
    return out


def conv3d_k3(srcs, weight, bias, cout, stride=(1, 1, 1), relu=True, skip=None, out=None):
    """srcs: list of planar [Ci,D,h,w]; weight packed [cin,27,cout]; -> [cout,Do,ho,wo].  Sample batch (here and in the other 3-D
    convolution wrappers): sources / skip [n,...] -> [n,cout,Do,ho,wo] in one launch; ``out`` may be [n,...] slices of a larger
    allocation."""
    srcs, skip = [_samples(s_) for s_ in srcs], _samples(skip)
    n, sstr, ks, (D, h, w) = _vol_inputs(srcs, skip, "conv3d")
    if n is None and out is not None:
        raise ValueError("conv3d_k3: out= belongs to the batched call")
    sz, sxy = int(stride[0]), int(stride[1])
    Do, ho, wo = _conv_out(D, sz), _conv_out(h, sxy), _conv_out(w, sxy)
    out = _vol_out(n, (cout, Do, ho, wo), srcs[0].device, skip, out)
    chans, cin = _channels(srcs, -4)
    reps = n or 1
    work = lambda: {"flops": 2.0 * 27 * reps * cin * cout * Do * ho * wo,
                    "bytes": 4.0 * reps * (cin * D * h * w + cout * Do * ho * wo * (2 if skip is not None else 1))}
    _launch("effi_conv3d_k3_f32", (_ptr_array(srcs), chans, len(srcs), _p(weight), _p(bias), cout, D, h, w, sz, sxy, int(relu),
                                   _p(skip), _p(out)), n, lambda: (_long_array(sstr), ks, out.stride(0) if n > 1 else 0),
            key=f"conv3d_c{'8' if cout % 8 == 0 else '1'}_s{sz}{sxy}", work=work)
    return out


def _conv3d_one(x, wpack, bias, cout, relu, s, key, name, x3):
    """The 3-D convolutions of ONE planar source x [cin,D,h,w] (or [n,cin,D,h,w]) at stride (s,s,s) -> [cout,Do,ho,wo]."""
    x = _samples(x)
    n, xs = _in(x, 4, "conv3d input")
    cin, D, h, w = x.shape[-4:]
    Do, ho, wo = _conv_out(D, s), _conv_out(h, s), _conv_out(w, s)
    out = _vol_out(n, (cout, Do, ho, wo), x.device, None)
    reps = n or 1
    work = lambda: {"flops": 2.0 * 27 * reps * cin * cout * Do * ho * wo, "bytes": 4.0 * reps * (cin * D * h * w + cout * Do * ho * wo)}
    _launch(name, (_p(x), cin, _p(wpack), _p(bias), cout, D, h, w, int(relu), _p(out)), n, lambda: (xs, out.stride(0)), key=key, work=work,
            x3=x3)
    return out


def conv3d_k3s1_mfma(x, wpack, bias, cout, relu=True):
    """x planar [cin,D,h,w]; stride-1 3-D conv as z-batched 2-D MFMA convs -> [cout,D,h,w]."""
    return _conv3d_one(x, wpack, bias, cout, relu, 1, f"conv3d_mfma_nt{cout // 16}", "effi_conv3d_k3s1_mfma_f32", False)


def conv3d_k3s2_x3(x, wpack, bias, cout, relu=True):
    """x planar [cin,D,h,w] (w % 4 == 0); stride-(2,2,2) 3-D conv in split precision (``packing.pack_conv3d_s2_bf16x3``) ->
    [cout,Do,ho,wo]."""
    return _conv3d_one(x, wpack, bias, cout, relu, 2, f"conv3d_s2x3_nt{(cout + 15) // 16}", "effi_conv3d_k3s2_bf16x3_f32", True)


def conv3d_k3s2_mfma(x, wpack, bias, cout, relu=True):
    """x planar [cin,D,h,w]; stride-(2,2,2) 3-D conv as z-batched stride-2 2-D MFMA convs -> [cout,Do,ho,wo]."""
    return _conv3d_one(x, wpack, bias, cout, relu, 2, f"conv3d_mfma_s2_nt{cout // 16}", "effi_conv3d_k3s2_mfma_f32", False)


def _conv3d_s1_x3(srcs, wpack, bias, cout, relu, key, name):
    """The stride-1 split-precision 3-D convolutions of concatenated sources; ``key`` is formatted with cin // 8 and cout's tiles."""
    srcs = [_samples(s_) for s_ in srcs]
    n, sstr, _, (D, h, w) = _vol_inputs(srcs, None, "conv3d")
    chans, cin = _channels(srcs, -4)
    out = _vol_out(n, (cout, D, h, w), srcs[0].device, None)
    reps = n or 1
    work = lambda: {"flops": 2.0 * 27 * reps * cin * cout * D * h * w, "bytes": 4.0 * reps * (cin + cout) * D * h * w}
    _launch(name, (_ptr_array(srcs), chans, len(srcs), _p(wpack), _p(bias), cout, D, h, w, int(relu), _p(out)), n,
            lambda: (_long_array(sstr), out.stride(0)), key=key.format(oct=cin // 8, nt=(cout + 15) // 16), work=work, x3=True)
    return out


def conv3d_k3s1_bf16x3(srcs, wpack, bias, cout, relu=True):
    """srcs: planar [Ci,D,h,w] tensors (channel concatenation); stride-1 3-D conv as z-batched 2-D convs in split precision
    (``packing.pack_conv3d_planes_bf16x3``) -> [cout,D,h,w].  w % 4 == 0, cout <= 32."""
    return _conv3d_s1_x3(srcs, wpack, bias, cout, relu, "conv3d_x3_nt{nt}", "effi_conv3d_k3s1_bf16x3_f32")


def conv3d_k3s1_roll(srcs, wpack, bias, cout, relu=True):
    """srcs: one or two planar [Ci,D,h,w] tensors, 8 or 16 channels in total; stride-1 3-D conv with a rolling window of
    input planes in split precision (``packing.pack_conv3d_roll_bf16x3``) -> [cout,D,h,w].  w % 4 == 0, cout <= 32."""
    return _conv3d_s1_x3(srcs, wpack, bias, cout, relu, "conv3d_roll_oct{oct}_nt{nt}", "effi_conv3d_k3s1_roll_bf16x3_f32")


def _deconv3d(x, wp, bias, cout, sz, relu, skip, key, name, x3):
    """The transposed 3-D convolutions x [cin,D,h,w] (+ skip) -> [cout,sz*D,2h,2w], or sample batches of them in one launch; the
    split-precision entry is stride (2,2,2) only and takes no ``sz``."""
    x, skip = _samples(x), _samples(skip)
    n, (xs,), ks, (D, h, w) = _vol_inputs([x], skip, "deconv3d")
    cin = x.shape[-4]
    out = _vol_out(n, (cout, sz * D, 2 * h, 2 * w), x.device, skip)
    reps = n or 1
    work = lambda: {"flops": 2.0 * 27 * reps * cin * cout * D * h * w,
                    "bytes": 4.0 * reps * (cin * D * h * w + cout * sz * D * 4 * h * w * (2 if skip is not None else 1))}
    _launch(name, (_p(x), cin, _p(wp), _p(bias), cout, D, h, w) + (() if x3 else (sz,)) + (int(relu), _p(skip), _p(out)), n,
            lambda: (xs, ks, out.stride(0) if n > 1 else 0), key=key, work=work, x3=x3)
    return out


def deconv3d_k3(x, weight, bias, cout, sz=2, relu=True, skip=None):
    return _deconv3d(x, weight, bias, cout, sz, relu, skip, f"deconv3d_c{cout if cout == 1 else 8}_s{sz}", "effi_deconv3d_k3_f32", False)


def deconv3d_k3s2_x3(x, wpack, bias, cout, relu=True, skip=None):
    """Transposed 3-D conv, stride (2,2,2), on the bf16 matrix cores in split precision
    (``packing.pack_deconv3d_s2_bf16x3``): x [cin,D,h,w] -> [cout,2D,2h,2w] (+ skip after the ReLU)."""
    return _deconv3d(x, wpack, bias, cout, 2, relu, skip, "deconv3d_x3", "effi_deconv3d_k3s2_bf16x3_f32", True)


def fusion_dynamic_filter(ref_depth, src_depths, ref_cam, src_cams, ref_conf=None, prob_threshold=0.0, dh_view_num=2,
                          dist_base=4.0, rel_diff_base=1300.0, relative=False, want_points=True, want_reproj=False):
    """Scope row n3: one reference view through the dynamic geometric-consistency filter (misc/fusion.py:117-181,
    test_tank.py:466-512).  ref_depth [h,w]; src_depths [V,h,w]; ref_cam [2,4,4]; src_cams [V,2,4,4]; ref_conf [H,W] or None
    -> dict(depth [h,w], geo_mask / prob_mask / mask [h,w] uint8, points [3,h,w] or None, reproj_xyd [V,3,h,w] or None)."""
    rows = _view_inputs("fusion_dynamic_filter", ref_depth, src_depths, ref_cam, src_cams)
    return _fusion_dynamic("fusion_dynamic_filter", _lib.lib().effi_fusion_dynamic_filter_f32,
                           rows, ref_conf, prob_threshold, dh_view_num, dist_base, rel_diff_base, relative, want_points,
                           {"reproj_xyd": (rows.v_max, 3) if want_reproj else None})


def fusion_vis_filter(ref_depth, reproj_xyd, dist_base=4.0, rel_diff_base=1300.0, thres_view=2, relative=False):
    """misc/fusion.py:157-181 (vis_filter_dynamic's arithmetic): ref_depth [n,1,h,w], reproj_xyd [n,v,3,h,w] ->
    masks [n,v,v+1-thres_view,h,w] uint8."""
    _t(ref_depth, "ref_depth"), _t(reproj_xyd, "reproj_xyd")
    n, v, three, h, w = reproj_xyd.shape
    if three != 3 or tuple(ref_depth.shape) != (n, 1, h, w):
        raise ValueError("fusion_vis_filter: ref_depth [n,1,h,w], reproj_xyd [n,v,3,h,w]")
    nthr = v + 1 - int(thres_view)
    masks = torch.empty(n, v, max(nthr, 0), h, w, device=ref_depth.device, dtype=torch.uint8)
    if nthr <= 0:
        return masks
    check(_lib.lib().effi_fusion_vis_filter_f32(_p(ref_depth), _p(reproj_xyd), n, v, h, w, float(dist_base), float(rel_diff_base),
                                                int(thres_view), int(bool(relative)), _p(masks), _stream()), "effi_fusion_vis_filter_f32")
    return masks


def fusion_dtu_reproject(ref_depth, src_depth, ref_cam, src_cam, s=None, e=None, dist_base=0.5, diff_base=0.25):
    """test_dtu_dypcd.py:164-233 for one (reference, source) pair (PARITY UNPINNED): depth maps [h,w], cameras [2,4,4] ->
    (out5 [5,h,w] = depth_reprojected, x_reprojected, y_reprojected, x_src, y_src; masks [e-s,h,w] uint8 or None).  With s / e
    given the call is check_geometric_consistency (masks + zeroing under the last mask), without it reproject_with_depth."""
    for name, t_ in (("ref_depth", ref_depth), ("src_depth", src_depth), ("ref_cam", ref_cam), ("src_cam", src_cam)):
        _t(t_, name)
    h, w = ref_depth.shape
    if tuple(src_depth.shape) != (h, w) or tuple(ref_cam.shape) != (2, 4, 4) or tuple(src_cam.shape) != (2, 4, 4):
        raise ValueError("fusion_dtu_reproject: depth maps [h,w], cameras [2,4,4]")
    dev = ref_depth.device
    out5 = torch.empty(5, h, w, device=dev, dtype=torch.float32)
    masks = torch.empty(e - s, h, w, device=dev, dtype=torch.uint8) if s is not None else None
    scratch = torch.empty(104, device=dev, dtype=torch.float32)
    check(_lib.lib().effi_fusion_dtu_reproject_f32(_p(ref_depth), _p(src_depth), _p(ref_cam), _p(src_cam), h, w, int(s or 1), int(e or 2),
                                                   float(dist_base), float(diff_base), _p(scratch), _p(out5), _p(masks), _stream()),
          "effi_fusion_dtu_reproject_f32")
    return out5, masks


FUSION_IMG2CAM, FUSION_CAM2WORLD, FUSION_WORLD2CAM, FUSION_CAM2IMG = 0, 1, 2, 3


def fusion_points(mode, pts, cam, depth=None):
    """The point transforms of misc/fusion.py:23-47 with one camera per batch element.  pts [n or 1,h,w,3 or 4,1] (a leading 1 is
    broadcast over the batch, as the reference's ``@`` does), cam [n,2,4,4], depth [n,1,h,w] for FUSION_IMG2CAM -> [n,h,w,4 or 3,1]."""
    _t(pts, "points"), _t(cam, "cam")
    n = cam.shape[0]
    ni = 3 if mode == FUSION_IMG2CAM else 4
    no = 3 if mode == FUSION_CAM2IMG else 4
    if pts.dim() != 5 or pts.shape[3] != ni or pts.shape[4] != 1 or pts.shape[0] not in (1, n) or tuple(cam.shape[1:]) != (2, 4, 4):
        raise ValueError(f"fusion_points: points [n|1,h,w,{ni},1] and cam [n,2,4,4] expected, got {tuple(pts.shape)} / {tuple(cam.shape)}")
    h, w = pts.shape[1], pts.shape[2]
    if mode == FUSION_IMG2CAM:
        _t(depth, "depth")
        if tuple(depth.shape) != (n, 1, h, w):
            raise ValueError(f"fusion_points: depth {tuple(depth.shape)} is not [n,1,h,w] = {(n, 1, h, w)}")
    out = torch.empty(n, h, w, no, 1, device=pts.device, dtype=torch.float32)
    scratch = torch.empty(52 * n, device=pts.device, dtype=torch.float32)
    bstride = 0 if (pts.shape[0] == 1 and n > 1) else h * w * ni
    check(_lib.lib().effi_fusion_points_f32(int(mode), _p(pts), bstride, _p(depth), _p(cam), n, h, w, _p(scratch), _p(out), _stream()),
          "effi_fusion_points_f32")
    return out


def fusion_dtu_filter(ref_depth, src_depths, ref_cam, src_cams, confidence=None, conf_threshold=0.5, conf_keep=0.75, s=1, e=11,
                      dist_base=0.5, diff_base=0.25, want_points=True):
    """Scope row n3, DTU branch (test_dtu_dypcd.py:164-333; PARITY UNPINNED, see the header): one reference view through the dynamic
    geometric-consistency filter.  ref_depth [h,w]; src_depths [V,h,w]; ref_cam [2,4,4]; src_cams [V,2,4,4]; confidence [ch,cw] (any
    size: resized to the depth size as cv2.resize does) or None -> dict(depth [h,w], photo_mask / geo_mask / mask [h,w] uint8,
    points [3,h,w] or None)."""
    rows = _view_inputs("fusion_dtu_filter", ref_depth, src_depths, ref_cam, src_cams)
    return _fusion_dtu("fusion_dtu_filter", _lib.lib().effi_fusion_dtu_filter_f32,
                       rows, confidence, conf_threshold, conf_keep, s, e, dist_base, diff_base, want_points)


def fusion_pair_table(pair_data):
    """Host only (no GPU, no library): the ``read_pair_file`` list [(ref_view, [src_views...]), ...] (test_dtu_dypcd.py:150-160) ->
    the pair table of the scan launches, int32 CPU tensor [n_ref, 1 + v_max]: row = reference id, its source ids in order, -1 padding."""
    rows = [(int(ref), [int(v) for v in srcs]) for ref, srcs in pair_data]
    if not rows:
        raise ValueError("fusion_pair_table: no reference view")
    for ref, srcs in rows:
        if ref < 0 or not srcs or min(srcs) < 0:
            raise ValueError(f"fusion_pair_table: reference view {ref} needs a non-negative id and at least one non-negative source id")
    v_max = max(len(srcs) for _, srcs in rows)
    table = torch.full((len(rows), 1 + v_max), -1, dtype=torch.int32)
    for r, (ref, srcs) in enumerate(rows):
        table[r, 0] = ref
        table[r, 1:1 + len(srcs)] = torch.tensor(srcs, dtype=torch.int32)
    return table


class _FusionRows(NamedTuple):
    """The views of one filter launch, single-view or scan: ``head`` = the entry's leading arguments up to ``h, w`` (``keep`` holds
    the tensors it points into), ``lead`` = the outputs' leading shape, () or (n_ref,)."""
    head: tuple
    keep: tuple
    lead: tuple
    h: int
    w: int
    n_rows: int
    v_max: int
    n_src: int          # source maps read, over all rows


def _view_inputs(what, ref_depth, src_depths, ref_cam, src_cams):
    for name, t_ in (("ref_depth", ref_depth), ("src_depths", src_depths), ("ref_cam", ref_cam), ("src_cams", src_cams)):
        _t(t_, name)
    if src_depths.dim() != 3:
        raise ValueError(f"{what}: src_depths [V,h,w] expected")
    V, h, w = src_depths.shape
    if tuple(ref_depth.shape) != (h, w) or tuple(ref_cam.shape) != (2, 4, 4) or tuple(src_cams.shape) != (V, 2, 4, 4):
        raise ValueError(f"{what}: ref_depth [h,w], src_depths [V,h,w], ref_cam [2,4,4], src_cams [V,2,4,4]")
    keep = (ref_depth, src_depths, ref_cam, src_cams)
    return _FusionRows(tuple(map(_p, keep)) + (V,), keep, (), h, w, 1, V, V)


def _scan_inputs(what, depths, cams, pairs):
    _t(depths, "depths"), _t(cams, "cams")
    if depths.dim() != 3 or tuple(cams.shape) != (depths.shape[0], 2, 4, 4):
        raise ValueError(f"{what}: depths [n_views,h,w] and cams [n_views,2,4,4] expected, got {tuple(depths.shape)} / {tuple(cams.shape)}")
    if not isinstance(pairs, torch.Tensor) or pairs.is_cuda or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] < 2 \
            or pairs.shape[0] < 1:
        raise ValueError(f"{what}: pairs must be the int32 CPU table [n_ref, 1 + v_max] of ops.fusion_pair_table")
    pairs = pairs.contiguous()
    pairs_dev = pairs.to(depths.device)
    n_views, h, w = depths.shape
    n_ref, v_max = pairs.shape[0], pairs.shape[1] - 1
    return _FusionRows((_p(depths), _p(cams), n_views, _p(pairs), _p(pairs_dev), n_ref, v_max), (depths, cams, pairs, pairs_dev), (n_ref,),
                       h, w, n_ref, v_max, int((pairs[:, 1:] >= 0).sum()))


def _fusion_conf(what, name, conf, rows, resize=False):
    """A launch's confidence, [ch,cw] or for a scan [n_ref,ch,cw] in table order, or None -> the entry's (conf, ch, cw); with
    ``resize`` (DTU) brought to the depth size as cv2.resize does -> (conf,)."""
    if conf is not None:
        _t(conf, name)
        if rows.lead and (conf.dim() != 3 or conf.shape[0] != rows.n_rows):
            raise ValueError(f"{what}: {name} [n_ref,ch,cw] expected, got {tuple(conf.shape)}")
    if resize:
        if conf is not None and tuple(conf.shape[-2:]) != (rows.h, rows.w):
            conf = resize_planar(conf.reshape(rows.n_rows, *conf.shape[-2:]).contiguous(), rows.h, rows.w).reshape(*rows.lead, rows.h, rows.w)
        return (conf,)
    if conf is None:
        return None, 0, 0
    ch, cw = conf.shape[len(rows.lead):]
    return conf, ch, cw


_TT_MASKS, _DTU_MASKS = ("geo_mask", "prob_mask", "mask"), ("photo_mask", "geo_mask", "mask")      # in the entries' argument order


def _fusion_out(rows, masks, want_points, reproj=None):
    """The result dict in the entry's output order; ``reproj``: {key: leading shape or None} of a single view's by-products."""
    z = lambda *sh, dt=torch.float32: torch.empty(*sh, rows.h, rows.w, device=rows.keep[0].device, dtype=dt)
    out = {"depth": z(*rows.lead)}
    out.update((k, z(*rows.lead, dt=torch.uint8)) for k in masks)
    out["points"] = z(*rows.lead, 3) if want_points else None
    out.update((k, None if sh is None else z(*sh)) for k, sh in (reproj or {}).items())
    return out


def _fusion_launch(key, fn, rows, conf, params, out, maps, extra=0):
    """Entry ``fn`` (``effi_<key>_f32``) under the profile key ``key``; ``maps`` = fp32 maps per row besides the sources and the points,
    ``extra`` = further maps of the launch."""
    scratch = torch.empty(52 * rows.n_rows * (rows.v_max + 1), device=rows.keep[0].device, dtype=torch.float32)
    px, n = rows.h * rows.w, rows.n_rows
    work = lambda: {"flops": 0.0, "bytes": 4.0 * px * (rows.n_src + n * (maps + (0 if out["points"] is None else 3)) + extra) + 3.0 * n * px}
    check(_call(key, work, fn, *rows.head, rows.h, rows.w, _p(conf[0]), *conf[1:], *params, _p(scratch),
                *map(_p, out.values()), _stream()), f"effi_{key}_f32")
    return out


def _fusion_dynamic(key, fn, rows, ref_conf, prob_threshold, dh_view_num, dist_base, rel_diff_base, relative, want_points, reproj=None):
    conf = _fusion_conf(key, "ref_conf", ref_conf, rows)
    params = (float(prob_threshold), int(dh_view_num), float(dist_base), float(rel_diff_base), int(bool(relative)))
    return _fusion_launch(key, fn, rows, conf, params, _fusion_out(rows, _TT_MASKS, want_points, reproj), 2)


def _fusion_static(key, fn, rows, ref_conf, prob_threshold, img_dist_thresh, depth_thresh, vthresh, want_points, reproj=None, extra=0):
    conf = _fusion_conf(key, "ref_conf", ref_conf, rows)
    params = (float(prob_threshold), float(img_dist_thresh), float(depth_thresh), float(vthresh))
    return _fusion_launch(key, fn, rows, conf, params, _fusion_out(rows, _TT_MASKS, want_points, reproj), 2, extra)


def _fusion_dtu(key, fn, rows, confidence, conf_threshold, conf_keep, s, e, dist_base, diff_base, want_points):
    conf = _fusion_conf(key, "confidence", confidence, rows, resize=True)
    params = (float(conf_threshold), float(conf_keep), int(s), int(e), float(dist_base), float(diff_base))
    return _fusion_launch(key, fn, rows, conf, params, _fusion_out(rows, _DTU_MASKS, want_points), 3)


def fusion_dtu_filter_scan(depths, cams, pairs, confidence=None, conf_threshold=0.5, conf_keep=0.75, s=1, e=11, dist_base=0.5,
                           diff_base=0.25, want_points=True):
    """``fusion_dtu_filter`` for every reference view of a scan in ONE launch (test_dtu_dypcd.py:250-333).  depths [n_views,h,w] and
    cams [n_views,2,4,4] are read in place through ``pairs`` (``fusion_pair_table``: each reference view its own source count, at most
    16); confidence [n_ref,ch,cw] in table order (any size) or None -> dict(depth [n_ref,h,w], photo_mask / geo_mask / mask
    [n_ref,h,w] uint8, points [n_ref,3,h,w] or None); row r is bitwise ``fusion_dtu_filter`` on reference view r and its stacked sources."""
    rows = _scan_inputs("fusion_dtu_filter_scan", depths, cams, pairs)
    return _fusion_dtu("fusion_dtu_filter_scan", _lib.lib().effi_fusion_dtu_filter_scan_f32,
                       rows, confidence, conf_threshold, conf_keep, s, e, dist_base, diff_base, want_points)


def fusion_dynamic_filter_scan(depths, cams, pairs, ref_conf=None, prob_threshold=0.0, dh_view_num=2, dist_base=4.0,
                               rel_diff_base=1300.0, relative=False, want_points=True):
    """``fusion_dynamic_filter`` for every reference view of a scan in ONE launch (test_tank.py:466-512); arguments as
    ``fusion_dtu_filter_scan``, ref_conf [n_ref,ch,cw] in table order or None -> dict(depth [n_ref,h,w], geo_mask / prob_mask / mask
    [n_ref,h,w] uint8, points [n_ref,3,h,w] or None).  Every row needs at least ``dh_view_num`` sources."""
    rows = _scan_inputs("fusion_dynamic_filter_scan", depths, cams, pairs)
    return _fusion_dynamic("fusion_dynamic_filter_scan", _lib.lib().effi_fusion_dynamic_filter_scan_f32,
                           rows, ref_conf, prob_threshold, dh_view_num, dist_base, rel_diff_base, relative, want_points)


def fusion_static_filter(ref_depth, src_depths, ref_cam, src_cams, ref_conf=None, prob_threshold=0.0, img_dist_thresh=1.0,
                         depth_thresh=0.01, vthresh=4, want_points=True, want_reproj=False):
    """Scope row n3, the fixed-threshold visibility filter: get_reproj + vis_filter + ave_fusion (misc/fusion.py:79-115) and the
    driver's masks and points (test_tank.py:471-475,512-515) for one reference view in ONE kernel.  Arguments and result as
    ``fusion_dynamic_filter``; with ``want_reproj`` also ``in_range`` [V,h,w] (0/1 floats), get_reproj's second result."""
    rows = _view_inputs("fusion_static_filter", ref_depth, src_depths, ref_cam, src_cams)
    V = rows.v_max
    return _fusion_static("fusion_static_filter", _lib.lib().effi_fusion_static_filter_f32,
                          rows, ref_conf, prob_threshold, img_dist_thresh, depth_thresh, vthresh, want_points,
                          {"reproj_xyd": (V, 3) if want_reproj else None, "in_range": (V,) if want_reproj else None},
                          4 * V if want_reproj else 0)


def fusion_static_filter_scan(depths, cams, pairs, ref_conf=None, prob_threshold=0.0, img_dist_thresh=1.0, depth_thresh=0.01, vthresh=4,
                              want_points=True):
    """``fusion_static_filter`` for every reference view of a scan in ONE launch; arguments and result as
    ``fusion_dynamic_filter_scan``.  Every row needs at least one source; row r is bitwise the single-view launch."""
    rows = _scan_inputs("fusion_static_filter_scan", depths, cams, pairs)
    return _fusion_static("fusion_static_filter_scan", _lib.lib().effi_fusion_static_filter_scan_f32,
                          rows, ref_conf, prob_threshold, img_dist_thresh, depth_thresh, vthresh, want_points)


def fusion_project_img(src_img, dst_depth, src_cam, dst_cam, height=None, width=None):
    """misc/fusion.py:50-65: src_img [N,C,hs,ws], dst_depth [N,1,height,width], cameras [N,2,4,4] -> (warped [N,C,height,width],
    in_range [N,1,height,width] 0/1 floats).  ``height`` / ``width`` default to the source's size, as in the reference."""
    for name, t_ in (("src_img", src_img), ("dst_depth", dst_depth), ("src_cam", src_cam), ("dst_cam", dst_cam)):
        _t(t_, name)
    if src_img.dim() != 4:
        raise ValueError("fusion_project_img: src_img [N,C,hs,ws] expected")
    n, c, hs, ws = src_img.shape
    height, width = int(hs if height is None else height), int(ws if width is None else width)
    if tuple(dst_depth.shape) != (n, 1, height, width) or tuple(src_cam.shape) != (n, 2, 4, 4) or tuple(dst_cam.shape) != (n, 2, 4, 4):
        raise ValueError(f"fusion_project_img: dst_depth [N,1,height,width] = {(n, 1, height, width)} and cameras [N,2,4,4] expected, got "
                         f"{tuple(dst_depth.shape)} / {tuple(src_cam.shape)} / {tuple(dst_cam.shape)}")
    dev = src_img.device
    out = torch.empty(n, c, height, width, device=dev, dtype=torch.float32)
    in_range = torch.empty(n, 1, height, width, device=dev, dtype=torch.float32)
    scratch = torch.empty(104 * n, device=dev, dtype=torch.float32)
    work = lambda: {"flops": 0.0, "bytes": 4.0 * n * height * width * (2 + 5 * c)}
    check(_call("fusion_project_img", work, _lib.lib().effi_fusion_project_img_f32, _p(src_img), _p(dst_depth), _p(src_cam), _p(dst_cam), n,
                c, hs, ws, height, width, _p(scratch), _p(out), _p(in_range), _stream()), "effi_fusion_project_img_f32")
    return out, in_range


def fusion_static_vis_filter(ref_depth, reproj_xyd, img_dist_thresh, depth_thresh, vthresh):
    """misc/fusion.py:99-110: ref_depth [n,1,h,w], reproj_xyd [n,v,3,h,w] -> (masks [n,v,1,h,w] 0/1 floats, mask [n,1,h,w] uint8)."""
    _t(ref_depth, "ref_depth"), _t(reproj_xyd, "reproj_xyd")
    if reproj_xyd.dim() != 5 or reproj_xyd.shape[2] != 3 or tuple(ref_depth.shape) != (reproj_xyd.shape[0], 1) + tuple(reproj_xyd.shape[3:]):
        raise ValueError("fusion_static_vis_filter: ref_depth [n,1,h,w], reproj_xyd [n,v,3,h,w]")
    n, v, _, h, w = reproj_xyd.shape
    masks = torch.empty(n, v, 1, h, w, device=ref_depth.device, dtype=torch.float32)
    mask = torch.empty(n, 1, h, w, device=ref_depth.device, dtype=torch.uint8)
    work = lambda: {"flops": 0.0, "bytes": 4.0 * n * h * w * (1 + 4 * v) + 1.0 * n * h * w}
    check(_call("fusion_static_vis_filter", work, _lib.lib().effi_fusion_static_vis_filter_f32, _p(ref_depth), _p(reproj_xyd), _p(None), n,
                v, h, w, float(img_dist_thresh), float(depth_thresh), float(vthresh), _p(masks), _p(mask), _p(None), _stream()),
          "effi_fusion_static_vis_filter_f32")
    return masks, mask


def fusion_static_ave(ref_depth, reproj_xyd, masks):
    """misc/fusion.py:113-115: (sum_v d * masks + ref_depth) / (sum_v masks + 1) -> [n,1,h,w]; masks [n,v,1,h,w] fp32."""
    _t(ref_depth, "ref_depth"), _t(reproj_xyd, "reproj_xyd"), _t(masks, "masks")
    if reproj_xyd.dim() != 5 or reproj_xyd.shape[2] != 3 or tuple(ref_depth.shape) != (reproj_xyd.shape[0], 1) + tuple(reproj_xyd.shape[3:]) \
            or tuple(masks.shape) != tuple(reproj_xyd.shape[:2]) + (1,) + tuple(reproj_xyd.shape[3:]):
        raise ValueError("fusion_static_ave: ref_depth [n,1,h,w], reproj_xyd [n,v,3,h,w], masks [n,v,1,h,w]")
    n, v, _, h, w = reproj_xyd.shape
    ave = torch.empty(n, 1, h, w, device=ref_depth.device, dtype=torch.float32)
    work = lambda: {"flops": 0.0, "bytes": 4.0 * n * h * w * (2 + 2 * v)}
    check(_call("fusion_static_ave", work, _lib.lib().effi_fusion_static_vis_filter_f32, _p(ref_depth), _p(reproj_xyd), _p(masks), n, v, h,
                w, 1.0, 1.0, 0.0, _p(None), _p(None), _p(ave), _stream()), "effi_fusion_static_vis_filter_f32")
    return ave


def fusion_prob_filter(ref_prob, prob_thresh):
    """misc/fusion.py:68-76: ref_prob [n,c,1,h,w], one threshold per leading channel -> [n,1,1,h,w] uint8, the AND of
    ``ref_prob[:, [i]] > prob_thresh[i]``; no threshold -> None, as the reference."""
    _t(ref_prob, "ref_prob")
    thr = [float(p) for p in prob_thresh]
    if ref_prob.dim() < 2 or len(thr) > ref_prob.shape[1]:
        raise ValueError(f"fusion_prob_filter: {len(thr)} thresholds for ref_prob {tuple(ref_prob.shape)}")
    if not thr:
        return None
    n, c = ref_prob.shape[:2]
    hw = ref_prob[0, 0].numel()
    mask = torch.empty((n, 1) + tuple(ref_prob.shape[2:]), device=ref_prob.device, dtype=torch.uint8)
    for i, p in enumerate(thr):
        check(_lib.lib().effi_fusion_prob_filter_f32(C.c_void_p(ref_prob.data_ptr() + 4 * i * hw), c * hw, n, hw, p, int(i == 0), _p(mask),
                                                     _stream()), "effi_fusion_prob_filter_f32")
    return mask


def fusion_compact(mask, points, images, layout="hwc", pairs=None):
    """The survivors of a scan as vertex arrays in the reference's order (test_dtu_dypcd.py:327-333, test_tank.py:517-533: boolean
    indexing view by view, then np.concatenate) without leaving the device and without atomics.  mask [n_ref,h,w] uint8; points
    [n_ref,3,h,w]; images fp32 in [0,1], ``layout`` "hwc" = [n,h,w,3] (the DTU driver's) or "chw" = [n,3,h,w] (the T&T driver's); row r
    takes image r, or image ``pairs[r,0]`` when the pair table is given -> (xyz [M,3] float32, rgb [M,3] uint8 = (uint8)(c * 255),
    offsets [n_ref+1] int32: the vertices of row r are offsets[r]:offsets[r+1]).  Reading M is the only host synchronisation."""
    _t(points, "points"), _t(images, "images")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or mask.dim() != 3 \
            or mask.device != points.device:
        raise TypeError("fusion_compact: mask must be a contiguous uint8 tensor [n_ref,h,w] on the points' device")
    n_ref, h, w = mask.shape
    if layout not in ("hwc", "chw"):
        raise ValueError("fusion_compact: layout is 'hwc' or 'chw'")
    if tuple(points.shape) != (n_ref, 3, h, w) or tuple(images.shape[1:]) != ((h, w, 3) if layout == "hwc" else (3, h, w)):
        raise ValueError(f"fusion_compact: points [n_ref,3,h,w] and images {'[n,h,w,3]' if layout == 'hwc' else '[n,3,h,w]'} expected, "
                         f"got {tuple(points.shape)} / {tuple(images.shape)} for mask {tuple(mask.shape)}")
    pairs_dev, stride = None, 0
    if pairs is not None:
        if not isinstance(pairs, torch.Tensor) or pairs.is_cuda or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[0] != n_ref:
            raise ValueError("fusion_compact: pairs must be the int32 CPU table [n_ref, 1 + v_max] of ops.fusion_pair_table")
        pairs = pairs.contiguous()
        pairs_dev, stride = pairs.to(mask.device), pairs.shape[1]
    elif images.shape[0] != n_ref:
        raise ValueError(f"fusion_compact: {images.shape[0]} images for {n_ref} reference views (pass pairs to pick them by id)")
    L = _lib.lib()
    dev = mask.device
    n_blocks = L.effi_fusion_compact_blocks(n_ref, h, w)
    if n_blocks <= 0:
        raise EffiLibraryError(f"fusion_compact: n_ref*h*w = {n_ref * h * w} must stay below 2^31 and n_ref below 65536")
    base = torch.empty(n_blocks, device=dev, dtype=torch.int32)
    offsets = torch.empty(n_ref + 1, device=dev, dtype=torch.int32)
    work = lambda: {"flops": 0.0, "bytes": 1.0 * n_ref * h * w + 8.0 * n_blocks}
    check(_call("fusion_compact_count", work, L.effi_fusion_compact_count_u8, C.c_void_p(mask.data_ptr()), n_ref, h, w, _p(base),
                _p(offsets), _stream()), "effi_fusion_compact_count_u8")
    m = int(offsets[n_ref].item())                              # the path's one host synchronisation: sizes the output
    xyz = torch.empty(m, 3, device=dev, dtype=torch.float32)
    rgb = torch.empty(m, 3, device=dev, dtype=torch.uint8)
    if m:
        pix, chs = (3, 1) if layout == "hwc" else (1, h * w)
        work = lambda: {"flops": 0.0, "bytes": 1.0 * n_ref * h * w + 39.0 * m}
        check(_call("fusion_compact_scatter", work, L.effi_fusion_compact_scatter_f32, C.c_void_p(mask.data_ptr()), _p(points), _p(images),
                    images.shape[0], _p(pairs), _p(pairs_dev), stride, 3 * h * w, pix, chs, n_ref, h, w, _p(base), _p(xyz), _p(rgb),
                    _stream()), "effi_fusion_compact_scatter_f32")
    return xyz, rgb, offsets


# ---- Gipuma / fusibile fusion (csrc/gipuma.hip; the driver is effi_mvs_plus_amd/gipuma.py) ----
GIPUMA_MAX_SOURCES = 64


def gipuma_check_sources(n_views, ref, sources):
    """Host only (no GPU, no library): what ``fusion_gipuma_view`` refuses before any launch -> the source ids as a list of ints."""
    ref, srcs = int(ref), [int(s) for s in sources]
    if not 0 <= ref < n_views:
        raise ValueError(f"gipuma: reference view {ref} outside [0, {n_views})")
    if not 1 <= len(srcs) <= GIPUMA_MAX_SOURCES:
        raise ValueError(f"gipuma: reference view {ref} has {len(srcs)} sources; 1 .. {GIPUMA_MAX_SOURCES} are supported")
    for s in srcs:
        if not 0 <= s < n_views:
            raise ValueError(f"gipuma: source view {s} of reference view {ref} outside [0, {n_views})")
        if s == ref:
            raise ValueError(f"gipuma: reference view {ref} is listed as its own source")
    return srcs


def fusion_gipuma_prob(depths, confidences, prob_threshold):
    """probability_filter (misc/gipuma.py:177,188) on the device: depths where ``confidences > prob_threshold``, else 0; same shapes."""
    _t(depths, "depths"), _t(confidences, "confidences")
    if depths.shape != confidences.shape or depths.numel() < 1:
        raise ValueError(f"fusion_gipuma_prob: depths {tuple(depths.shape)} and confidences {tuple(confidences.shape)} must have one size")
    out = torch.empty_like(depths)
    n = depths.numel()
    work = lambda: {"flops": 0.0, "bytes": 12.0 * n}
    check(_call("fusion_gipuma_prob", work, _lib.lib().effi_fusion_gipuma_prob_f32, _p(depths), _p(confidences), n, float(prob_threshold),
                _p(out), _stream()), "effi_fusion_gipuma_prob_f32")
    return out


def fusion_gipuma_view(depths, cams, images, ref, sources, used, disp_threshold=0.25, num_consistent=4, depth_min=0.001,
                       depth_max=100000.0):
    """ONE reference view of the Gipuma / fusibile fusion (misc/gipuma.py:192-213 without the external program).
    depths [n_views,h,w] (probability-filtered); cams [n_views,2,4,4]; images [n_views,h,w,3] fp32 in [0,1] or None; ``sources``: the
    ordered source ids of ``ref`` (1 .. 64, none equal to ``ref``: ValueError before any launch); ``used`` [n_views,h,w] uint8, read
    and UPDATED in place -- the calls of a scan must follow each other in reference order on one stream -> dict(points [3,h,w] and
    colour [h,w,3] or None: valid where mask is set, mask [h,w] uint8, count [h,w] uint8 = consistent sources per pixel)."""
    _t(depths, "depths"), _t(cams, "cams")
    if depths.dim() != 3 or tuple(cams.shape) != (depths.shape[0], 2, 4, 4):
        raise ValueError(f"fusion_gipuma_view: depths [n_views,h,w] and cams [n_views,2,4,4] expected, got {tuple(depths.shape)} / {tuple(cams.shape)}")
    n_views, h, w = depths.shape
    if images is not None:
        _t(images, "images")
        if tuple(images.shape) != (n_views, h, w, 3):
            raise ValueError(f"fusion_gipuma_view: images [n_views,h,w,3] = {(n_views, h, w, 3)} expected, got {tuple(images.shape)}")
    if not isinstance(used, torch.Tensor) or used.dtype != torch.uint8 or used.device != depths.device or not used.is_contiguous() \
            or tuple(used.shape) != (n_views, h, w):
        raise TypeError("fusion_gipuma_view: used must be a contiguous uint8 tensor [n_views,h,w] on the depths' device")
    srcs = gipuma_check_sources(n_views, ref, sources)
    dev = depths.device
    src_host = torch.tensor(srcs, dtype=torch.int32)
    src_dev = src_host.to(dev)
    z = lambda *sh, dt=torch.float32: torch.empty(*sh, device=dev, dtype=dt)
    out = {"points": z(3, h, w), "colour": None if images is None else z(h, w, 3), "mask": z(h, w, dt=torch.uint8),
           "count": z(h, w, dt=torch.uint8)}
    scratch = z(32 * (len(srcs) + 1))
    work = lambda: {"flops": 0.0, "bytes": 4.0 * h * w * (1 + len(srcs)) + 3.0 * h * w}
    check(_call("fusion_gipuma_view", work, _lib.lib().effi_fusion_gipuma_view_f32, _p(depths), _p(cams), _p(images), n_views, int(ref),
                _p(src_host), _p(src_dev), len(srcs), h, w, float(disp_threshold), int(num_consistent), float(depth_min), float(depth_max),
                _p(scratch), C.c_void_p(used.data_ptr()), *map(_p, out.values()), _stream()), "effi_fusion_gipuma_view_f32")
    return out


# ---- DTU evaluation of a fused cloud (csrc/dtu_eval.hip; the driver is effi_mvs_plus_amd/dtu_eval.py) ----
def _dtu_points(x, name, cols=3):
    _t(x, name)
    if x.dim() != 2 or x.shape[1] != cols or x.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: [n,{cols}] fp32 with n < 2^31 expected, got {tuple(x.shape)}")
    return x


def _dtu_buffer(x, name, dtypes, n, like):
    if not isinstance(x, torch.Tensor) or x.dtype not in dtypes or x.device != like.device or not x.is_contiguous() or x.numel() != n:
        raise TypeError(f"{name}: contiguous {' / '.join(str(d) for d in dtypes)} tensor of {n} elements on {like.device} expected")
    return x


def _dtu_grid(i0, dims):
    i0, dims = [int(v) for v in i0], [int(v) for v in dims]
    if len(i0) != 3 or len(dims) != 3:
        raise ValueError("dtu grid: i0 and dims are three integers each")
    return i0, dims


def dtu_cell_keys(xyz, cell, i0, dims):
    """Cell keys of a point set on the zero-anchored uniform grid (include/effi_mvs_hip.h, "DTU evaluation"): xyz [n,3]; cell index
    floor(p / cell) - i0 per axis in fp64, key (x * ny + y) * nz + z -> int64 [n].  The neighbour grid of reducePts_haa.m:12,22 and
    MaxDistCP.m:31-32 (their KD-trees)."""
    _dtu_points(xyz, "xyz")
    i0, dims = _dtu_grid(i0, dims)
    n = xyz.shape[0]
    keys = torch.empty(n, device=xyz.device, dtype=torch.int64)
    if n:
        work = lambda: {"flops": 0.0, "bytes": 20.0 * n}
        check(_call("dtu_cell_keys", work, _lib.lib().effi_dtu_cell_keys_f32, _p(xyz), n, float(cell), *i0, *dims, _p(keys), _stream()),
              "effi_dtu_cell_keys_f32")
    return keys


def dtu_reduce_blocks(n):
    """Length of ``dtu_reduce_round``'s per-workgroup count for n points."""
    return int(_lib.lib().effi_dtu_reduce_blocks(int(n)))


def dtu_reduce_round(pts4, keys, dims, dst, state_in, state_out, block_undecided):
    """One round of reducePts_haa.m:19-31 as a fixed point.  pts4 [n,4]: the points in key order, column 3 the
    rank in the visiting order as int32 bits; keys [n] int64 sorted; state_in / state_out [n] uint8 (0 undecided, 1 kept, 2 removed),
    distinct buffers; block_undecided [dtu_reduce_blocks(n)] int32 receives the undecided points left per workgroup."""
    _dtu_points(pts4, "pts4", 4)
    n = pts4.shape[0]
    _, dims = _dtu_grid((0, 0, 0), dims)
    _dtu_buffer(keys, "keys", (torch.int64,), n, pts4)
    _dtu_buffer(state_in, "state_in", (torch.uint8,), n, pts4), _dtu_buffer(state_out, "state_out", (torch.uint8,), n, pts4)
    _dtu_buffer(block_undecided, "block_undecided", (torch.int32,), dtu_reduce_blocks(n), pts4)
    if state_in.data_ptr() == state_out.data_ptr():
        raise ValueError("dtu_reduce_round: state_out must not alias state_in (a round reads the previous round's states only)")
    if n:
        work = lambda: {"flops": 0.0, "bytes": 26.0 * n}
        check(_call("dtu_reduce_round", work, _lib.lib().effi_dtu_reduce_round_f32, _p(pts4), _p(keys), n, *dims, float(dst), _p(state_in),
                    _p(state_out), _p(block_undecided), _stream()), "effi_dtu_reduce_round_f32")


def dtu_nn_capped(src, to4, keys, cell, i0, dims, cap):
    """MaxDistCP.m:31-33 without its blocks: src [n,3]; to4 [m,4] the target points in key order (column 3 unused) with their sorted
    keys [m] int64 on the grid (cell, i0, dims) -> fp64 [n] = min(cap^2, min_j d^2(src_i, to_j)); m = 0 gives cap^2."""
    _dtu_points(src, "src"), _dtu_points(to4, "to4", 4)
    n, m = src.shape[0], to4.shape[0]
    _dtu_buffer(keys, "keys", (torch.int64,), m, src)
    i0, dims = _dtu_grid(i0, dims) if m else ((0, 0, 0), (1, 1, 1))
    out = torch.empty(n, device=src.device, dtype=torch.float64)
    if n:
        work = lambda: {"flops": 0.0, "bytes": 20.0 * n + 24.0 * m}
        check(_call("dtu_nn_capped", work, _lib.lib().effi_dtu_nn_capped_f32, _p(src), n, _p(to4) if m else _p(None),
                    _p(keys) if m else _p(None), m, float(cell), *i0, *dims, float(cap), _p(out), _stream()), "effi_dtu_nn_capped_f32")
    return out


def dtu_obs_mask(xyz, obs_mask, bb0, res):
    """PointCompareMain.m:32-40: xyz [n,3]; obs_mask [X,Y,Z] bool / uint8 on the device; bb0 = BB(1,:) (three floats); res ->
    bool [n]: every index round((q - bb0) / res + 1) (halves away from zero) lies in 1..size and the mask is set there."""
    _dtu_points(xyz, "xyz")
    if not isinstance(obs_mask, torch.Tensor) or obs_mask.dim() != 3:
        raise TypeError("dtu_obs_mask: obs_mask [X,Y,Z] expected")
    _dtu_buffer(obs_mask, "obs_mask", (torch.bool, torch.uint8), obs_mask.numel(), xyz)
    n = xyz.shape[0]
    out = torch.empty(n, device=xyz.device, dtype=torch.bool)
    if n:
        b = [float(v) for v in bb0]
        work = lambda: {"flops": 0.0, "bytes": 14.0 * n}
        check(_call("dtu_obs_mask", work, _lib.lib().effi_dtu_obs_mask_f32, _p(xyz), n, b[0], b[1], b[2], float(res), _p(obs_mask),
                    *[int(s) for s in obs_mask.shape], _p(out), _stream()), "effi_dtu_obs_mask_f32")
    return out


def dtu_above_plane(xyz, plane):
    """PointCompareMain.m:52: xyz [n,3], plane = P (four floats) -> bool [n] = ((p0 x + p1 y) + p2 z) + p3 > 0 in fp64."""
    _dtu_points(xyz, "xyz")
    n = xyz.shape[0]
    out = torch.empty(n, device=xyz.device, dtype=torch.bool)
    if n:
        p = [float(v) for v in plane]
        work = lambda: {"flops": 0.0, "bytes": 13.0 * n}
        check(_call("dtu_above_plane", work, _lib.lib().effi_dtu_above_plane_f32, _p(xyz), n, p[0], p[1], p[2], p[3], _p(out), _stream()),
              "effi_dtu_above_plane_f32")
    return out


# ---- training loss and depth metrics (csrc/metrics.hip; the callers are autograd.mvs_loss and effi_mvs_plus_amd/metrics.py) ----
LOSS_MAX_OUTPUTS, METRICS_MAX_THRES, METRICS_MAX_BANDS = 16, 8, 8


def metrics_blocks(n):
    """Workgroups (= scratch rows) the loss / metrics kernels use for n elements."""
    return int(_lib.lib().effi_metrics_blocks(int(n)))


def _metrics_scratch(blocks, n_thres, n_bands, device):
    nbytes = int(_lib.lib().effi_metrics_scratch_bytes(int(blocks), int(n_thres), int(n_bands)))
    if nbytes <= 0:
        raise ValueError(f"metrics scratch: {blocks} rows with {n_thres} thresholds / {n_bands} bands is out of range")
    return torch.empty(nbytes // 8, device=device, dtype=torch.int64)


def _mask_form(mask, name, like):
    """fp32 mask (valid where > 0.5) -> 0, bool / uint8 mask (valid where set) -> 1; same element count and device as ``like``."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.float32, torch.bool, torch.uint8):
        raise TypeError(f"{name}: fp32, bool or uint8 tensor expected")
    if mask.device != like.device or not mask.is_contiguous() or mask.numel() != like.numel():
        raise ValueError(f"{name}: contiguous, {like.numel()} elements on {like.device} expected, got {tuple(mask.shape)} on {mask.device}")
    return 0 if mask.dtype == torch.float32 else 1


def _loss_inputs(ests, gts, masks, weights):
    K = len(ests)
    if not (1 <= K <= LOSS_MAX_OUTPUTS) or len(gts) != K or len(masks) != K or len(weights) != K:
        raise ValueError(f"mvs_loss: 1..{LOSS_MAX_OUTPUTS} outputs with one gt, mask and weight each expected")
    forms = set()
    for i in range(K):
        _t(ests[i], f"est[{i}]"), _t(gts[i], f"gt[{i}]")
        if gts[i].numel() != ests[i].numel() or ests[i].numel() < 1:
            raise ValueError(f"mvs_loss: est[{i}] {tuple(ests[i].shape)} and gt[{i}] {tuple(gts[i].shape)} differ in size (or are empty)")
        forms.add(_mask_form(masks[i], f"mask[{i}]", ests[i]))
    if len(forms) != 1:
        raise TypeError("mvs_loss: the masks of one call are all fp32 or all bool / uint8")
    n = [int(e.numel()) for e in ests]
    return K, forms.pop(), n, _ptr_array(ests), _ptr_array(gts), _ptr_array(masks), (C.c_long * K)(*n), (C.c_double * K)(*[float(w) for w in weights])


def mvs_loss(ests, gts, masks, weights):
    """mvs_loss forward (models/module.py:526-552) over K <= 16 outputs: two launches.  ests / gts / masks: lists of K tensors of
    equal size per output (outputs of one stage pass the same gt / mask objects); weights: K floats.  -> (out [K + 1] fp32 with
    out[:K] the per-output means over the valid pixels and out[K] the weighted total, count [K] int64)."""
    K, u8, n, pe, pg, pm, pn, pw = _loss_inputs(ests, gts, masks, weights)
    dev = ests[0].device
    out = torch.empty(K + 1, device=dev, dtype=torch.float32)
    count = torch.empty(K, device=dev, dtype=torch.int64)
    scratch = _metrics_scratch(sum(metrics_blocks(v) for v in n), 0, 0, dev)
    work = lambda: {"flops": 6.0 * sum(n), "bytes": 12.0 * sum(n)}
    check(_call("mvs_loss", work, _lib.lib().effi_mvs_loss_f32, pe, pg, pm, pn, K, u8, pw, _p(out), _p(count),
                C.c_void_p(out.data_ptr() + 4 * K), _p(scratch), _stream()), "effi_mvs_loss_f32")
    return out, count


def mvs_loss_bwd(ests, gts, masks, weights, count, grad_total):
    """Gradients of ``mvs_loss``'s total w.r.t. the K estimates in one launch: count [K] int64 from the forward, grad_total a 0-dim
    fp32 DEVICE tensor.  -> list of K tensors shaped like the estimates (exactly 0 at the masked pixels)."""
    K, u8, n, pe, pg, pm, pn, pw = _loss_inputs(ests, gts, masks, weights)
    _t(grad_total, "grad_total")
    if grad_total.numel() != 1:
        raise ValueError("mvs_loss_bwd: grad_total is one fp32 scalar on the device")
    _dtu_buffer(count, "count", (torch.int64,), K, ests[0])
    grads = [torch.empty_like(e) for e in ests]
    work = lambda: {"flops": 4.0 * sum(n), "bytes": 16.0 * sum(n)}
    check(_call("mvs_loss_bwd", work, _lib.lib().effi_mvs_loss_bwd_f32, pe, pg, pm, pn, K, u8, pw, _p(count), _p(grad_total),
                _ptr_array(grads), _stream()), "effi_mvs_loss_bwd_f32")
    return grads


# ---- optimizer step (csrc/optim.hip; the caller is optim.FusedAdamW) ----
def adamw_max_tensors():
    """Most tensors one ``effi_adamw_multi_f32`` call takes (host-only query: needs no GPU)."""
    return int(_lib.lib().effi_adamw_max_tensors())


def _adamw_slices(n, k):
    """[(start, stop)] of the launches that cover n tensors in order, at most k per launch."""
    return [(s, min(n, s + k)) for s in range(0, n, k)]


def gradnorm_max_tensors():
    """Most gradients one ``effi_gradnorm_partial_f32`` call takes (host-only query: needs no GPU)."""
    return int(_lib.lib().effi_gradnorm_max_tensors())


def grad_norm_multi(grads, max_norm=float("inf"), clip=None, skipped=None):
    """The 2-norm over all elements of a list of fp32 device tensors and the coefficient that clips it to ``max_norm`` (what
    ``torch.nn.utils.clip_grad_norm_`` computes; the gradients are only read): one launch per ``gradnorm_max_tensors()`` tensors
    and one that finishes.  -> clip, a 4-element fp32 device tensor [norm, min(1, max_norm / (norm + 1e-6)), 1 if the norm is
    finite else 0, 0] (``clip``: such a tensor to write into).  ``skipped`` (optional one-element int64 device tensor) += 1 when
    the norm is not finite.  Deterministic: exact squares, double sums in a fixed order, no atomics (csrc/optim.hip).  An empty
    list has norm 0; it needs ``clip`` to say which device."""
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"grad_norm_multi: max_norm >= 0 expected (inf: never clip), got {max_norm}")
    n = len(grads)
    if n == 0 and clip is None:
        raise ValueError("grad_norm_multi: an empty list needs the clip tensor: it names the device")
    f32 = torch.float32
    dev = _t(grads[0] if n else clip, "grads[0]" if n else "clip").device
    idx = dev.index
    ptrs, numel = [], []
    for i, g in enumerate(grads):
        # the checks of _t, once per call instead of once per tensor; _t words the refusal
        if not isinstance(g, torch.Tensor) or g.dtype is not f32 or g.get_device() != idx or not g.is_contiguous():
            _t(g, f"grads[{i}]")
            raise ValueError(f"grad_norm_multi: grads[{i}] lives on {g.device}, grads[0] on {dev}: one device per call")
        ptrs.append(g.data_ptr())
        numel.append(g.numel())
    if clip is None:
        clip = torch.empty(4, dtype=f32, device=dev)
    else:
        _t(clip, "clip")
        if clip.numel() != 4 or clip.device != dev:
            raise ValueError("grad_norm_multi: clip is four fp32 elements on the gradients' device")
    if skipped is not None:
        if not isinstance(skipped, torch.Tensor) or skipped.dtype is not torch.int64 or skipped.numel() != 1 or skipped.device != dev:
            raise ValueError("grad_norm_multi: skipped is one int64 element on the gradients' device")
    L, st = _lib.lib(), _stream()
    total = int(L.effi_gradnorm_chunks((C.c_long * max(n, 1))(*numel), n))
    if total < 0:
        raise ValueError("grad_norm_multi: more than 2^31 - 1 chunks of 2048 elements")
    partial = torch.empty(total, dtype=torch.float64, device=dev)          # every slot is written by the launches below
    base = 0
    for s, e in _adamw_slices(n, gradnorm_max_tensors()):
        sizes = (C.c_long * (e - s))(*numel[s:e])
        # an empty tensor has no storage and the entry refuses null pointers: it gets the clip tensor's address, never read through
        arr = (C.c_void_p * (e - s))(*[p or clip.data_ptr() for p in ptrs[s:e]])
        check(L.effi_gradnorm_partial_f32(arr, sizes, e - s, C.c_void_p(partial.data_ptr() + 8 * base) if total else None, st),
              "effi_gradnorm_partial_f32")
        base += int(L.effi_gradnorm_chunks(sizes, e - s))
    check(L.effi_gradnorm_finish_f32(_p(partial) if total else None, total, max_norm, _p(clip), _p(skipped), st), "effi_gradnorm_finish_f32")
    return clip


def adamw_multi(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay, clip=None, skip_nonfinite=False):
    """One AdamW step (train.py:263,441; torch.optim.AdamW, amsgrad=False, maximize=False) IN PLACE over lists of tensors: two launches
    per ``adamw_max_tensors()`` tensors.  params / exp_avgs / exp_avg_sqs are updated, steps (0-dim fp32 device tensors, one per
    parameter) are incremented first, grads are only read.  lr: a number, or a one-element fp32 device tensor the kernel reads when
    it runs (a captured step then follows a scheduler that fills it).  ``clip`` (the tensor of ``grad_norm_multi``): every gradient
    element is read as g * clip[1]; with ``skip_nonfinite`` nothing at all is written, counters included, when clip[2] == 0."""
    if clip is None and skip_nonfinite:
        raise ValueError("adamw_multi: skip_nonfinite needs the clip tensor of grad_norm_multi")
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(steps) == n):
        raise ValueError("adamw_multi: one gradient, exp_avg, exp_avg_sq and step per parameter expected")
    if n == 0:
        return
    dev, f32 = _t(params[0], "params[0]").device, torch.float32
    idx = dev.index
    names = ("params", "grads", "exp_avgs", "exp_avg_sqs", "steps")
    pp, pg, pm, pv, ps, numel = [], [], [], [], [], []
    for i in range(n):
        five = (params[i], grads[i], exp_avgs[i], exp_avg_sqs[i], steps[i])
        for k, x in enumerate(five):
            # the checks of _t, once per call and device instead of 1,210 times per step of the model; _t words the refusal
            if not isinstance(x, torch.Tensor) or x.dtype is not f32 or x.get_device() != idx or not x.is_contiguous():
                _t(x, f"{names[k]}[{i}]")
                raise ValueError(f"adamw_multi: {names[k]}[{i}] lives on {x.device}, params[0] on {dev}: one device per call")
        p, g, m, v, c = five
        ne = p.numel()
        if g.numel() != ne or m.numel() != ne or v.numel() != ne or c.numel() != 1:
            raise ValueError(f"adamw_multi: tensor {i}: gradient and moments of the parameter's {ne} elements and a one-element step expected")
        # an empty tensor has no storage (data_ptr() == 0) and the entry refuses null pointers: it gets its step counter's address,
        # which the kernel never reads through (no chunk belongs to a tensor without elements); its counter is incremented like the others
        cp = c.data_ptr()
        pp.append(p.data_ptr() or cp), pg.append(g.data_ptr() or cp), pm.append(m.data_ptr() or cp), pv.append(v.data_ptr() or cp)
        ps.append(cp), numel.append(ne)
    lr_dev = None
    if isinstance(lr, torch.Tensor):
        lr_dev = _t(lr, "lr")
        if lr_dev.numel() != 1 or lr_dev.device != dev:
            raise ValueError("adamw_multi: a tensor lr is one fp32 element on the parameters' device")
    if clip is not None:
        _t(clip, "clip")
        if clip.numel() != 4 or clip.device != dev:
            raise ValueError("adamw_multi: clip is the four fp32 elements of grad_norm_multi on the parameters' device")
    st = _stream()
    lrv = 0.0 if lr_dev is not None else float(lr)
    for s, e in _adamw_slices(n, adamw_max_tensors()):
        arr = C.c_void_p * (e - s)
        args = (arr(*pp[s:e]), arr(*pg[s:e]), arr(*pm[s:e]), arr(*pv[s:e]), arr(*ps[s:e]), (C.c_long * (e - s))(*numel[s:e]), e - s, lrv,
                _p(lr_dev), float(beta1), float(beta2), float(eps), float(weight_decay))
        if clip is None:
            check(_lib.lib().effi_adamw_multi_f32(*args, st), "effi_adamw_multi_f32")
        else:
            check(_lib.lib().effi_adamw_multi_clip_f32(*args, _p(clip), int(bool(skip_nonfinite)), st), "effi_adamw_multi_clip_f32")


def depth_metrics(est, gt, mask, thresholds=(), bands=(), acc=None):
    """Thres_metrics / AbsDepthError_metrics (utils.py:139-160) for all thresholds and bands in one pass (two launches): est / gt /
    mask [B,H,W]; thresholds: up to 8 numbers; bands: up to 8 (lo, hi) pairs, both ends inclusive.  -> (scalars [1 + T + R] fp32 =
    [abs_mean, thres.., band..] averaged over the per-image values, counts [B, 1 + T + R] int64, sums [B, 1 + R] fp64); acc
    (optional fp64 [1 + T + R] on the device) += scalars."""
    _t(est, "est"), _t(gt, "gt")
    if est.dim() < 2 or gt.shape != est.shape or est.numel() < 1:
        raise ValueError(f"depth_metrics: est and gt [B,H,W] of one shape expected, got {tuple(est.shape)} / {tuple(gt.shape)}")
    u8 = _mask_form(mask, "mask", est)
    B = int(est.shape[0])
    n = est.numel() // B
    thr = [float(v) for v in thresholds]
    lo, hi = [float(b[0]) for b in bands], [float(b[1]) for b in bands]
    T, R = len(thr), len(lo)
    if T > METRICS_MAX_THRES or R > METRICS_MAX_BANDS:
        raise ValueError(f"depth_metrics: at most {METRICS_MAX_THRES} thresholds and {METRICS_MAX_BANDS} bands per call")
    S = 1 + T + R
    if acc is not None:
        _dtu_buffer(acc, "acc", (torch.float64,), S, est)
    dev = est.device
    scalars = torch.empty(S, device=dev, dtype=torch.float32)
    counts = torch.empty((B, S), device=dev, dtype=torch.int64)
    sums = torch.empty((B, 1 + R), device=dev, dtype=torch.float64)
    scratch = _metrics_scratch(B * metrics_blocks(n), T, R, dev)
    fa = lambda v: (C.c_float * max(1, len(v)))(*v)
    work = lambda: {"flops": (4.0 + T + 3 * R) * B * n, "bytes": 12.0 * B * n}
    check(_call("depth_metrics", work, _lib.lib().effi_depth_metrics_f32, _p(est), _p(gt), _p(mask), B, n, u8, fa(thr), T, fa(lo), fa(hi), R,
                _p(counts), _p(sums), _p(scalars), _p(acc), _p(scratch), _stream()), "effi_depth_metrics_f32")
    return scalars, counts, sums


def image_prepare(img_u8, dst_h, dst_w, out=None):
    """Scope row n4: decoded image [h,w,3] (or [h,w]) uint8 on the device -> [3,dst_h,dst_w] fp32 = cv2-style bilinear resize of
    img / 255, channel-first (datasets/general_eval.py:83-117,189)."""
    if not isinstance(img_u8, torch.Tensor) or img_u8.dtype != torch.uint8 or not img_u8.is_contiguous():
        raise TypeError("image_prepare: contiguous uint8 tensor [h,w,c] expected")
    if img_u8.dim() == 2:
        img_u8 = img_u8.unsqueeze(-1)
    if not img_u8.is_cuda:
        raise _lib.EffiLibraryError("effi_image_prepare_u8_f32 needs a tensor on the GPU (there is no CPU fallback)")
    h, w, c = img_u8.shape
    if out is None:
        out = torch.empty(c, dst_h, dst_w, device=img_u8.device, dtype=torch.float32)
    work = lambda: {"flops": 0.0, "bytes": 1.0 * h * w * c + 4.0 * c * dst_h * dst_w}
    check(_call("image_prepare", work, _lib.lib().effi_image_prepare_u8_f32, C.c_void_p(img_u8.data_ptr()), h, w, c, dst_h, dst_w,
                _p(out), _stream()), "effi_image_prepare_u8_f32")
    return out


def resize_planar(x, dst_h, dst_w, out=None):
    """[C,h,w] fp32 -> [C,dst_h,dst_w], the bilinear resize of ``image_prepare`` (datasets/general_eval.py:160-166)."""
    _t(x, "image")
    c, h, w = x.shape
    if out is None:
        out = torch.empty(c, dst_h, dst_w, device=x.device, dtype=torch.float32)
    check(_lib.lib().effi_resize_linear_f32(_p(x), c, h, w, dst_h, dst_w, _p(out), _stream()), "effi_resize_linear_f32")
    return out


# ---- training input (csrc/train_input.hip; the callers are datasets/dtu_yao.py, datasets/blend.py and GraphedTrainStep) ----
GT_STAGES = ("stage1", "stage2", "stage3", "stage4")


def _train_out(out, shape, dev, name):
    if out is None:
        return torch.empty(shape, device=dev, dtype=torch.float32)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev \
            or tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name}: contiguous fp32 {tuple(shape)} on {dev} expected")
    return out


def images_prepare(imgs_u8, out=None):
    """Decoded training images [V,h,w,3] (or [B,N,h,w,3]) uint8 on the device -> [V,3,h,w] ([B,N,3,h,w]) fp32 = x / 255, channel-first,
    all views in one launch (datasets/dtu_yao.py:70-74,186; datasets/blend.py:97-101,222; training images are never resized).
    Bitwise ``np.float32(x) / 255`` and bitwise ``image_prepare`` of every view at its own size."""
    if not isinstance(imgs_u8, torch.Tensor) or imgs_u8.dtype != torch.uint8 or not imgs_u8.is_contiguous() \
            or imgs_u8.dim() not in (4, 5) or imgs_u8.shape[-1] != 3 or imgs_u8.numel() < 1:
        raise TypeError("images_prepare: contiguous uint8 tensor [V,h,w,3] or [B,N,h,w,3] expected")
    if not imgs_u8.is_cuda:
        raise _lib.EffiLibraryError("effi_images_prepare_batch_u8_f32 needs a tensor on the GPU (there is no CPU fallback)")
    lead, (h, w) = tuple(imgs_u8.shape[:-3]), imgs_u8.shape[-3:-1]
    V = 1
    for v in lead:
        V *= int(v)
    out = _train_out(out, lead + (3, h, w), imgs_u8.device, "images_prepare: out")
    work = lambda: {"flops": 0.0, "bytes": 15.0 * V * h * w}
    check(_call("images_prepare", work, _lib.lib().effi_images_prepare_batch_u8_f32, C.c_void_p(imgs_u8.data_ptr()), V, h, w, _p(out),
                _stream()), "effi_images_prepare_batch_u8_f32")
    return out


def gt_pyramid(depth, mask_u8=None, depth_range=None, thresh=10, out=None):
    """The ground truth of a sample batch as the loss reads it, one launch: depth [B,h,w] fp32 (h, w multiples of 8) ->
    (depth_ms, mask_ms), dictionaries stage1 .. stage4 of [B, h >> (4-k), w >> (4-k)] fp32.  stage4 is a copy of ``depth``, the
    others cv2's INTER_NEAREST (source pixel (f y, f x)).  Exactly one mask source: ``mask_u8`` [B,h,w] uint8 (DTU,
    datasets/dtu_yao.py:93-106: byte > thresh) or ``depth_range`` [B,2] fp32 on the device (BlendedMVS, datasets/blend.py:215-220:
    depth_min <= d <= depth_max on each level's own depth).  ``out=(depth_ms, mask_ms)`` writes into given tensors."""
    _t(depth, "gt_pyramid: depth")
    if depth.dim() != 3 or depth.numel() < 1:
        raise ValueError(f"gt_pyramid: depth [B,h,w] expected, got {tuple(depth.shape)}")
    B, h, w = (int(v) for v in depth.shape)
    dev = depth.device
    if mask_u8 is not None:
        if not isinstance(mask_u8, torch.Tensor) or mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous() \
                or mask_u8.device != dev or mask_u8.shape != depth.shape:
            raise TypeError(f"gt_pyramid: mask_u8 is a contiguous uint8 tensor {tuple(depth.shape)} on {dev}")
    if depth_range is not None:
        _t(depth_range, "gt_pyramid: depth_range")
        if depth_range.device != dev or tuple(depth_range.shape) != (B, 2):
            raise ValueError(f"gt_pyramid: depth_range [{B},2] (depth_min, depth_max per sample) on {dev} expected")
    outs = []
    for i, ms in enumerate(out if out is not None else (None, None)):
        what = ("depth", "mask")[i]
        outs.append({k: _train_out(None if ms is None else ms[k], (B, h >> (3 - j), w >> (3 - j)), dev, f"gt_pyramid: out {what}[{k}]")
                     for j, k in enumerate(GT_STAGES)})
    depth_ms, mask_ms = outs
    work = lambda: {"flops": 0.0, "bytes": (4.0 + (1.0 if mask_u8 is not None else 0.0) + 8.0 * 85 / 64) * B * h * w}
    # the library refuses h % 8, w % 8 and both / neither mask source before it launches anything
    check(_call("gt_pyramid", work, _lib.lib().effi_gt_pyramid_f32, _p(depth), _p(mask_u8), int(thresh), _p(depth_range), B, h, w,
                _ptr_array([depth_ms[k] for k in GT_STAGES]), _ptr_array([mask_ms[k] for k in GT_STAGES]), _stream()),
          "effi_gt_pyramid_f32")
    return depth_ms, mask_ms


def softmax_regress_conf(logits, depth, disp_range=None, conf_up=0):
    """logits [D,h,w]; depth [D] / [D,h,w] -> (depth [h,w], confidence [h,w]) and, with ``disp_range``, also the regressed
    depth as normalised inverse depth (``depth_to_inv`` of it, written by the same kernel).  ``conf_up`` = f > 0: the result
    tuple ends with the confidence replicated f x f ([h*f,w*f], ``upsample_nearest`` of it) written by the same kernel.
    Sample batch: logits [n,D,h,w], depth [D] / [n,D] / [n,D,h,w], disp_range [n,R] (or one [R] for all) -> every result with a
    leading n, one launch."""
    logits, depth, disp_range = _samples(logits), _samples(depth), _samples(disp_range)
    n, ls = _in(logits, 3, "logits")
    D, h, w = logits.shape[-3:]
    _t(depth, "depth", contiguous=False)
    depth, dds, dps, dss = _depth_strides(depth, n, D, h, w)
    dev, lead = logits.device, () if n is None else (n,)
    od = torch.empty(lead + (h, w), device=dev, dtype=torch.float32)
    oc = torch.empty(lead + (h, w), device=dev, dtype=torch.float32)
    oi, n_range, rs = None, 0, 0
    if disp_range is not None:
        m, rs = _in(disp_range, 1, "disp_range")
        if m is not None and m != n:
            raise ValueError(f"softmax_regress_conf: sample counts differ ({n} volumes, {m} ranges)")
        oi, n_range = torch.empty(lead + (h, w), device=dev, dtype=torch.float32), disp_range.shape[-1]
    if conf_up:
        ou = torch.empty(lead + (h * conf_up, w * conf_up), device=dev, dtype=torch.float32)
        _launch("effi_softmax_regress_conf_up_f32", (_p(logits), _p(depth), dds, dps, D, h, w, _p(od), _p(oc), _p(disp_range), n_range,
                                                     _p(oi), _p(ou), conf_up), n, lambda: (ls, dss, h * w, h * w, rs, h * w, ou.stride(0)))
        return (od, oc, ou) if disp_range is None else (od, oc, oi, ou)
    _launch("effi_softmax_regress_conf_f32", (_p(logits), _p(depth), dds, dps, D, h * w, _p(od), _p(oc), _p(disp_range), n_range, _p(oi)),
            n, lambda: (ls, dss, h * w, h * w, rs, h * w))
    return (od, oc) if disp_range is None else (od, oc, oi)


def _vol_strides(vol, h, w):
    """Per-pixel D-vector volume as planar [D,h,w] or pixel-major [h*w,1,1,D] (the reference's `pro`)."""
    _t(vol, "volume", contiguous=False)
    if vol.dim() == 3:
        if not vol.is_contiguous():
            vol = vol.contiguous()
        return vol, h * w, 1, vol.shape[0]
    if vol.dim() == 4 and vol.shape[0] == h * w:
        return vol, vol.stride(3), vol.stride(0), vol.shape[3]
    raise ValueError(f"unsupported volume shape {tuple(vol.shape)}")


def _range_ptr(r, h, w):
    """depth-range bound: scalar-like tensor (global) or per-pixel [.., h, w] map."""
    _t(r, "range", contiguous=False)
    if r.numel() == 1:
        return r.reshape(1), 0
    if r.numel() == h * w:
        return r.reshape(h, w).contiguous(), 1
    raise ValueError(f"depth range with {r.numel()} elements does not match {h}x{w}")


def _ranges(dmin, dmax, h, w):
    """The two bounds of the depth range, both global or both per-pixel -> (dmin tensor, dmax tensor, pixel stride)."""
    dmin_t, rps = _range_ptr(dmin, h, w)
    dmax_t, rps2 = _range_ptr(dmax, h, w)
    if rps != rps2:
        raise ValueError("depth_min / depth_max must both be global or both per-pixel")
    return dmin_t, dmax_t, rps


def _query_strides(query, h, w):
    """query [nq, h', w'] with (h', w') == (h, w) or exactly 2x (read nearest-downsampled) -> (nq, plane, row, column stride)."""
    _t(query, "query")
    nq, qh, qw = query.shape
    if (qh, qw) == (h, w):
        return nq, qh * qw, qw, 1
    if (qh // 2, qw // 2) == (h, w):
        return nq, qh * qw, 2 * qw, 2   # F.interpolate(nearest) to half size picks the even samples
    raise ValueError("query resolution must equal the volume's or be twice it")


def _lookup_args(cur_vol, reg_vol, dmin, dmax, h, w):
    """The look-up block of the GetCost family as its entries take it (cur_vol, cds, cps, Dcur, reg_vol, rds, rps, Dreg, dmin, dmax,
    range_ps) -> (args, Dcur, Dreg, keep); ``keep`` holds the tensors behind the pointers in ``args`` (contiguous copies among
    them), for the caller to keep alive until it has launched."""
    cur_vol, cds, cps, Dc = _vol_strides(cur_vol, h, w)
    reg_vol, rds, rps, Dr = _vol_strides(reg_vol, h, w)
    dmin_t, dmax_t, gps = _ranges(dmin, dmax, h, w)
    return (_p(cur_vol), cds, cps, Dc, _p(reg_vol), rds, rps, Dr, _p(dmin_t), _p(dmax_t), gps), Dc, Dr, (cur_vol, reg_vol, dmin_t, dmax_t)


def _pair_outputs(srcs_a, srcs_b, what, mismatch, cout, out_dims=lambda D, h, w: (D, h, w)):
    """The two calls of a 3-D pair launch: source lists of [c,D,h,w] tensors (``what`` in their errors) with the same shapes (else
    ValueError(mismatch)) -> (out_a, out_b, cin, D, h, w): outputs [cout, *out_dims(D, h, w)], cin = the channels of a list."""
    for s in list(srcs_a) + list(srcs_b):
        _t(s, what)
    if [tuple(s.shape) for s in srcs_a] != [tuple(s.shape) for s in srcs_b]:
        raise ValueError(mismatch)
    _, D, h, w = srcs_a[0].shape
    out_a = torch.empty(cout, *out_dims(D, h, w), device=srcs_a[0].device, dtype=torch.float32)
    return out_a, torch.empty_like(out_a), sum(s.shape[0] for s in srcs_a), D, h, w


def vol_lookup1d(vol, query, dmin, dmax, h, w):
    """query [nq, h', w'] with (h', w') == (h, w) or exactly 2x (read nearest-downsampled)."""
    vol, vds, vps, Dp = _vol_strides(vol, h, w)
    nq, qds, qys, qxs = _query_strides(query, h, w)
    dmin_t, dmax_t, rps = _ranges(dmin, dmax, h, w)
    out = torch.empty(nq, h, w, device=query.device, dtype=torch.float32)
    check(_lib.lib().effi_vol_lookup1d_f32(_p(vol), vds, vps, Dp, _p(query), qds, qys, qxs, nq, _p(dmin_t),
                                            _p(dmax_t), rps, h, w, _p(out), _stream()), "effi_vol_lookup1d_f32")
    return out


def bilinear_sampler1d(img, coords, want_mask=False):
    """``bilinear_sampler`` of the reference (models/Effi_MVS_plus.py:102-117) for H == 1 images: img [N,C,1,W], coords
    [N,Ho,Wo,2] pixel (x, y) -> [N,C,Ho,Wo] (and the in-range mask [N,Ho,Wo,1] as float)."""
    _t(img, "img"), _t(coords, "coords")
    N, Cc, H, W = img.shape
    if H != 1 or coords.dim() != 4 or coords.shape[0] != N or coords.shape[-1] != 2:
        raise ValueError("bilinear_sampler1d: img [N,C,1,W] and coords [N,Ho,Wo,2]")
    Ho, Wo = coords.shape[1:3]
    out = torch.empty(N, Cc, Ho, Wo, device=img.device, dtype=torch.float32)
    mask = torch.empty(N, Ho, Wo, 1, device=img.device, dtype=torch.float32) if want_mask else None
    check(_lib.lib().effi_bilinear_sampler1d_f32(_p(img), N, Cc, W, _p(coords), Ho * Wo, _p(out), _p(mask), _stream()),
          "effi_bilinear_sampler1d_f32")
    return (out, mask) if want_mask else out


def vol_lookup1d_pair(vol_a, vol_b, query, dmin, dmax, h, w):
    """``vol_lookup1d`` into two planar volumes of the same shape with the same queries, one launch -> (out_a, out_b)."""
    vol_a, vds, vps, Dp = _vol_strides(vol_a, h, w)
    vol_b, vds_b, vps_b, Dp_b = _vol_strides(vol_b, h, w)
    if (vds, vps, Dp) != (vds_b, vps_b, Dp_b):
        raise ValueError("vol_lookup1d_pair: the two volumes must share shape and layout")
    nq, qds, qys, qxs = _query_strides(query, h, w)
    dmin_t, dmax_t, rps = _ranges(dmin, dmax, h, w)
    out_a = torch.empty(nq, h, w, device=query.device, dtype=torch.float32)
    out_b = torch.empty_like(out_a)
    check(_lib.lib().effi_vol_lookup1d_pair_f32(_p(vol_a), _p(vol_b), vds, vps, Dp, _p(query), qds, qys, qxs, nq, _p(dmin_t),
                                                 _p(dmax_t), rps, h, w, _p(out_a), _p(out_b), _stream()), "effi_vol_lookup1d_pair_f32")
    return out_a, out_b


def conv3d_k3_pair(x_a, weight_a, bias_a, x_b, weight_b, bias_b, cout, sxy=1, relu=True):
    """``conv3d_k3`` of two single-source convolutions of the same shape (cout 8, stride (1,sxy,sxy)) in one launch."""
    out_a, out_b, cin, D, h, w = _pair_outputs([x_a], [x_b], "conv3d input", "conv3d_k3_pair: the two inputs must share their shape", cout,
                                               lambda D, h, w: (D, (h - 1) // sxy + 1, (w - 1) // sxy + 1))
    ho, wo = out_a.shape[2:]
    work = lambda: {"flops": 2.0 * 2 * 27 * cin * cout * D * ho * wo, "bytes": 2 * 4.0 * (cin * D * h * w + cout * D * ho * wo)}
    check(_call(f"conv3d_pair_c8_s1{sxy}", work, _lib.lib().effi_conv3d_k3_pair_f32, _p(x_a), _p(weight_a), _p(bias_a), _p(out_a),
                _p(x_b), _p(weight_b), _p(bias_b), _p(out_b), cin, cout, D, h, w, sxy, int(relu), _stream()), "effi_conv3d_k3_pair_f32")
    return out_a, out_b


def csp_gen_roll_pair(x, prior_a, w0_a, b0_a, wc_a, bc_a, w1_a, b1_a, prior_b, w0_b, b0_b, wc_b, bc_b, w1_b, b1_b):
    """conv0 | conv_cost -> conv1 of two cross-scale blocks over one fine volume in ONE launch (``effi_csp_gen_roll_bf16x3_pair_f32``):
    x [1,D,H,W]; priors [1,D,h,w]; w0 / wc [1,27,8] packed (``Conv3d._packed``), w1 the rolling operand -> (c1_a, c1_b) [8,D,h,w].
    Bitwise ``conv3d_k3_pair`` (sxy 2 / sxy 1) + ``conv3d_k3s1_roll_pair``."""
    _t(x, "fine volume"), _t(prior_a, "prior"), _t(prior_b, "prior")
    _, D, H, W = x.shape
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if tuple(prior_a.shape) != (1, D, h, w) or tuple(prior_b.shape) != (1, D, h, w):
        raise ValueError(f"csp_gen_roll_pair: priors must be [1,{D},{h},{w}], got {tuple(prior_a.shape)} / {tuple(prior_b.shape)}")
    for t_, n_ in ((w0_a, 216), (wc_a, 216), (w0_b, 216), (wc_b, 216), (b0_a, 8), (bc_a, 8), (b0_b, 8), (bc_b, 8)):
        _t(t_, "generated layer's parameters")
        if t_.numel() != n_:
            raise ValueError("csp_gen_roll_pair: the generated layers are 1 -> 8 channels (27 x 8 weights, 8 biases)")
    out_a = torch.empty(8, D, h, w, device=x.device, dtype=torch.float32)
    out_b = torch.empty_like(out_a)
    V = D * h * w
    work = lambda: {"flops": 2 * 2.0 * 27 * (8 * 2 + 16 * 8) * V, "bytes": 4.0 * (D * H * W + 2 * V + 2 * 8 * V)}
    check(_call("csp_gen_roll_pair", work, _x3("effi_csp_gen_roll_bf16x3_pair_f32"), _p(x), D, H, W, _p(prior_a), _p(w0_a), _p(b0_a),
                _p(wc_a), _p(bc_a), _p(w1_a), _p(b1_a), _p(out_a), _p(prior_b), _p(w0_b), _p(b0_b), _p(wc_b), _p(bc_b), _p(w1_b),
                _p(b1_b), _p(out_b), _stream()), "effi_csp_gen_roll_bf16x3_pair_f32")
    return out_a, out_b


def conv3d_k3s1_roll_pair(srcs_a, wpack_a, bias_a, srcs_b, wpack_b, bias_b, cout, relu=True):
    """``conv3d_k3s1_roll`` of two convolutions with the same source split and shape in one launch."""
    out_a, out_b, cin, D, h, w = _pair_outputs(srcs_a, srcs_b, "conv3d input",
                                               "conv3d_k3s1_roll_pair: the two source lists must share their shapes", cout)
    work = lambda: {"flops": 2 * 2.0 * 27 * cin * cout * D * h * w, "bytes": 2 * 4.0 * (cin + cout) * D * h * w}
    check(_call(f"conv3d_roll_pair_oct{cin // 8}", work, _x3("effi_conv3d_k3s1_roll_bf16x3_pair_f32"), _ptr_array(srcs_a),
                _p(wpack_a), _p(bias_a), _p(out_a), _ptr_array(srcs_b), _p(wpack_b), _p(bias_b), _p(out_b),
                _int_array([s.shape[0] for s in srcs_a]), len(srcs_a), cout, D, h, w, int(relu), _stream()),
          "effi_conv3d_k3s1_roll_bf16x3_pair_f32")
    return out_a, out_b


def deconv3d_k3_pair(x_a, weight_a, bias_a, x_b, weight_b, bias_b, cout, sz=1, relu=True):
    """``deconv3d_k3`` (stride (1,2,2), cout 1) of two inputs of the same shape in one launch."""
    out_a, out_b, cin, D, h, w = _pair_outputs([x_a], [x_b], "deconv3d input", "deconv3d_k3_pair: the two inputs must share their shape", cout,
                                               lambda D, h, w: (sz * D, 2 * h, 2 * w))
    work = lambda: {"flops": 2 * 2.0 * 27 * cin * cout * D * h * w, "bytes": 2 * 4.0 * (cin * D * h * w + cout * sz * D * 4 * h * w)}
    check(_call("deconv3d_pair_c1_s1", work, _lib.lib().effi_deconv3d_k3_pair_f32, _p(x_a), _p(weight_a), _p(bias_a), _p(out_a),
                _p(x_b), _p(weight_b), _p(bias_b), _p(out_b), cin, cout, D, h, w, sz, int(relu), _stream()), "effi_deconv3d_k3_pair_f32")
    return out_a, out_b


def getcost(x, disp_range, interval, cur_vol, reg_vol, dmin, dmax, nq, h, w, input_is_depth=False, out=None):
    _t(x, "inv_depth"), _t(interval, "interval")
    look, _, _, _keep = _lookup_args(cur_vol, reg_vol, dmin, dmax, h, w)
    if out is None:
        out = torch.empty(2 * nq, h, w, device=x.device, dtype=torch.float32)
    n_range = 0 if disp_range is None else disp_range.numel()
    check(_lib.lib().effi_getcost_f32(_p(x), _p(disp_range), n_range, int(input_is_depth), _p(interval), *look, nq, h, w, _p(out), _stream()),
          "effi_getcost_f32")
    return out


def getcost_conv1x1(x, disp_range, interval, cur_vol, reg_vol, dmin, dmax, nq, h, w, weight, bias, cout, relu=True,
                    input_is_depth=False, out=None):
    """``getcost`` + 1x1 convolution (weight [2*nq, cout], bias [cout]) + ReLU in one kernel -> [cout,h,w]."""
    _t(x, "inv_depth"), _t(interval, "interval"), _t(weight, "weight"), _t(bias, "bias")
    look, Dc, Dr, _keep = _lookup_args(cur_vol, reg_vol, dmin, dmax, h, w)
    if out is None:
        out = torch.empty(cout, h, w, device=x.device, dtype=torch.float32)
    n_range = 0 if disp_range is None else disp_range.numel()
    work = lambda: {"flops": 2.0 * h * w * 2 * nq * cout, "bytes": 4.0 * h * w * (cout + 1 + Dc + Dr)}
    check(_call("getcost_conv1x1", work, _lib.lib().effi_getcost_conv1x1_f32, _p(x), _p(disp_range), n_range,
                int(input_is_depth), _p(interval), *look, nq, h, w, _p(weight), _p(bias), cout, int(relu), _p(out), _stream()),
          "effi_getcost_conv1x1_f32")
    return out


def encoder_inputs(x, disp_range, interval, cur_vol, reg_vol, dmin, dmax, nq, h, w, weight_c1, bias_c1, weight_d1, bias_d1, cout,
                   out_c1=None, out_d1=None):
    """``getcost_conv1x1`` (+ReLU) and ``conv2d_c1k7_relu`` of the same normalised inverse-depth map in one launch ->
    (relu(convc1(cost)) [cout,h,w], relu(convd1(x)) [cout,h,w]).  nq == 3, cout in {16, 32, 48}."""
    _t(x, "inv_depth"), _t(interval, "interval"), _t(disp_range, "disp_range")
    for t_ in (weight_c1, bias_c1, weight_d1, bias_d1):
        _t(t_, "encoder weights")
    look, Dc, Dr, _keep = _lookup_args(cur_vol, reg_vol, dmin, dmax, h, w)
    if out_c1 is None:
        out_c1 = torch.empty(cout, h, w, device=x.device, dtype=torch.float32)
    if out_d1 is None:
        out_d1 = torch.empty(cout, h, w, device=x.device, dtype=torch.float32)
    work = lambda: {"flops": 2.0 * h * w * (2 * nq + 49) * cout, "bytes": 4.0 * h * w * (2 * cout + 1 + Dc + Dr)}
    # split / bf16 precision: the 7x7 half on the matrix cores (EFFI_C1K7_MFMA=0: the exact-fp32 vector form, as "fp32" precision uses)
    x3 = uses_split() and _PY_OPTS["c1k7_mfma"] != 0
    fn = _lib.lib().effi_encoder_inputs_bf16x3_f32 if x3 else _lib.lib().effi_encoder_inputs_f32
    check(_call("encoder_inputs", work, fn, _p(x), _p(disp_range), disp_range.numel(), _p(interval), *look, nq, h, w,
                _p(weight_c1), _p(bias_c1), _p(weight_d1), _p(bias_d1), cout, _p(out_c1), _p(out_d1), _stream()),
          "effi_encoder_inputs_bf16x3_f32" if x3 else "effi_encoder_inputs_f32")
    return out_c1, out_d1


def conv2d_k3_bf16x3_pair(srcs_a, wpack_a, bias_a, srcs_b, wpack_b, bias_b, cout, act=ACT_NONE, out_a=None, out_b=None):
    """Two independent split-precision 3x3 convolutions of the same shape in one launch (``conv2d_k3_bf16x3`` twice)."""
    for s in list(srcs_a) + list(srcs_b):
        _t(s, "conv2d input")
    h, w = srcs_a[0].shape[-2:]
    if tuple(srcs_b[0].shape[-2:]) != (h, w):
        raise ValueError("conv2d_k3_bf16x3_pair: the two convolutions must share the map size")
    dev = srcs_a[0].device
    if out_a is None:
        out_a = torch.empty(cout, h, w, device=dev, dtype=torch.float32)
    if out_b is None:
        out_b = torch.empty(cout, h, w, device=dev, dtype=torch.float32)
    cin = sum(s.shape[0] for s in srcs_a) + sum(s.shape[0] for s in srcs_b)
    work = lambda: {"flops": 2.0 * h * w * cin * cout * 9, "bytes": 4.0 * h * w * (cin + 2 * cout)}
    check(_call(f"conv2d_k3x3_pair_nt{(cout + 15) // 16}", work, _x3("effi_conv2d_k3_bf16x3_pair_f32"), _ptr_array(srcs_a),
                _int_array([s.shape[0] for s in srcs_a]), len(srcs_a), _p(wpack_a), _p(bias_a), _p(out_a), _ptr_array(srcs_b),
                _int_array([s.shape[0] for s in srcs_b]), len(srcs_b), _p(wpack_b), _p(bias_b), _p(out_b), cout, h, w, act,
                _stream()), "effi_conv2d_k3_bf16x3_pair_f32")
    return out_a, out_b


def _conv2d_out_shape(epilogue, cout, h, w):
    """Shape of ``conv2d``'s outputs (both, where the epilogue has two) for one image."""
    if epilogue == EPI_GRU_ZR:
        return (cout // 2, h, w)
    if epilogue == EPI_HEAD:
        return (1, h, w)
    if epilogue in (EPI_NHWC, EPI_NHWC_ADD_SHUF2):
        return (h, w, cout)
    return (cout, h, w)


def _conv2d(srcs, wpack, bias, cout, ks, epilogue, act, aux0, aux1, disp_range, out0, out1, split):
    """``conv2d`` on the fp32 entry (effi_conv2d_f32) or, ``split``, ``conv2d_k3_bf16x3`` (effi_conv2d_k3_bf16x3_f32): one image, or
    n images in one launch of the entry's ``_batch`` twin."""
    h, w = srcs[0].shape[-2:]
    dev = srcs[0].device
    for s in srcs:
        _t(s, "conv2d input", contiguous=False)
        if tuple(s.shape[-2:]) != (h, w):
            raise ValueError(f"conv2d: every source of a call must be {h} x {w}, got {tuple(s.shape)}")
    n, istr = _sample_forms(srcs, 3, "conv2d input")
    if n is not None and n > 1 and aux1 is not None and (aux1.dim() != 4 or aux1.shape[0] != n):
        # (aux1 has no image stride in the library: the epilogues that read it are single-image only)
        raise ValueError(f"conv2d: aux1 of a batch must be [n, ...] with n = {n}")
    shape = _conv2d_out_shape(epilogue, cout, h, w)
    out0 = _out(n, shape, dev, out0, "conv2d output")
    if out1 is None and epilogue in (EPI_GRU_ZR, EPI_HEAD):
        out1 = torch.empty(shape if n is None else (n,) + shape, device=dev, dtype=torch.float32)
    if epilogue in (EPI_ADD_SHUF2, EPI_NHWC_ADD_SHUF2) and (aux0 is None or tuple(aux0.shape[-3:]) != (4 * cout, h // 2, w // 2) or h % 2 or w % 2):
        raise ValueError("conv2d_k3_bf16x3: the pixel-shuffled map must be [4*cout, h/2, w/2] ([n, ...] in a batch)")
    if epilogue == EPI_ADD_UP2 and (aux0 is None or tuple(aux0.shape[-3:]) != (cout, h // 2, w // 2)):
        raise ValueError("conv2d: the coarser map must be [cout, h/2, w/2] ([n, ...] in a batch)")
    aux_stride = 0
    if aux0 is not None:
        if n is None:
            _t(aux0, "conv2d aux0")
        else:
            m, aux_stride = _in(aux0, 3, "conv2d aux0")
            if m != n:
                raise ValueError(f"conv2d aux0: expected [n, ...] with n = {n}, got {tuple(aux0.shape)}")
    chans, cin = _channels(srcs, -3)
    reps, sfx = (1, "") if n is None else (n, "_batch")
    work = lambda: {"flops": 2.0 * reps * h * w * cin * cout * ks * ks, "bytes": 4.0 * reps * h * w * (cin + cout)}
    tail = lambda: (_long_array(istr), aux_stride, out0.stride(0) if n > 1 else 0)
    if split:
        _launch("effi_conv2d_k3_bf16x3_f32", (_ptr_array(srcs), chans, len(srcs), _p(wpack), _p(bias), cout, h, w, epilogue, act, _p(aux0),
                                              _p(aux1), None, 0, _p(out0), _p(out1)), n, tail,
                key=f"conv2d_k3x3_nt{(cout + 15) // 16}_epi{epilogue}{sfx}", work=work, x3=True)
    else:
        n_range = 0 if disp_range is None else disp_range.numel()
        _launch("effi_conv2d_f32", (_ptr_array(srcs), chans, len(srcs), _p(wpack), _p(bias), cout, ks, h, w, epilogue, act, _p(aux0),
                                    _p(aux1), _p(disp_range), n_range, _p(out0), _p(out1)), n, tail,
                key=f"conv2d_k{ks}_nt{(cout + 15) // 16}_epi{epilogue}{sfx}", work=work)
    return (out0, out1) if out1 is not None else out0


def _conv2d_takes_split(srcs, wpack, ks, epilogue):
    """Whether ``conv2d`` hands this call to the split-precision 3x3 entry: ONE predicate for the single-image and the batched call, so
    that image i of a batch always runs the arithmetic of the 3-D call on image i."""
    return (uses_split() and wpack.wx is not None and ks == 3 and srcs[0].shape[-1] % 4 == 0
            and epilogue in (EPI_PLAIN, EPI_NHWC, EPI_GRU_ZR, EPI_GRU_Q)
            and all(s.shape[-3] % 8 == 0 for s in srcs[:-1]))


def conv2d(srcs, wpack, bias, cout, ks, epilogue=EPI_PLAIN, act=ACT_NONE, aux0=None, aux1=None, disp_range=None,
           out0=None, out1=None):
    """2-D convolution (ks 1 or 3) of the concatenated planar sources [C,h,w].  Image batch: sources [n,C,h,w] (all the same n; a
    3-D source beside them is shared by all images), ``aux0`` [n,...], outputs [n,...] -- ONE launch, image i bitwise the 3-D call
    on image i (epilogues PLAIN, NHWC, ADD_UP2; the library reports UNSUPPORTED for the others when n > 1)."""
    if hasattr(wpack, "w32"):                 # packing.Conv2dWeights: both operand orders, pick the arithmetic here
        if _conv2d_takes_split(srcs, wpack, ks, epilogue):
            return _conv2d(srcs, wpack.wx, bias, cout, 3, epilogue, act, aux0, aux1, None, out0, out1, True)
        wpack = wpack.w32
    return _conv2d(srcs, wpack, bias, cout, ks, epilogue, act, aux0, aux1, disp_range, out0, out1, False)


def conv2d_k3_bf16x3(srcs, wpack, bias, cout, epilogue=EPI_PLAIN, act=ACT_NONE, aux0=None, aux1=None, out0=None, out1=None):
    """3x3 convolution in split precision (hi*hi + hi*lo + lo*hi on the bf16 MFMA, fp32 accumulate); ``wpack`` from
    ``packing.pack_conv2d_bf16x3``.  Same sources / epilogues as ``conv2d`` (PLAIN, NHWC, GRU_ZR, GRU_Q); w % 4 == 0 and every
    source but the last has a multiple of 8 channels (otherwise the library reports UNSUPPORTED).  Image batch as ``conv2d``
    (epilogues PLAIN, NHWC, ADD_SHUF2, NHWC_ADD_SHUF2 for n > 1)."""
    return _conv2d(srcs, wpack, bias, cout, 3, epilogue, act, aux0, aux1, None, out0, out1, True)


# =============================================================================================
# split-resident ("SR") maps of the update block: include/effi_mvs_hip.h, section "Split-resident activation maps"
# =============================================================================================
_SR = os.environ.get("EFFI_MVS_SR", "1") != "0"


def set_sr(enabled):
    """Route the update block's split-precision convolutions through split-resident maps (default) or through fp32 maps (the
    round-2 form; bitwise the same results)."""
    global _SR
    _SR = bool(enabled)


def uses_sr(pixels=None):
    """SR maps on?  ``pixels``: size of the map in question -- EFFI_MVS_SR_MAX_PX (A/B runs) keeps larger maps on the fp32 form."""
    if not (_SR and uses_split()):
        return False
    return pixels is None or pixels <= _SR_MAX_PX


_SR_MAX_PX = int(os.environ.get("EFFI_MVS_SR_MAX_PX", str(1 << 40)))


def sr_geometry(h, w):
    """(hp, wp) of an SR plane for an h x w map: effi_sr_geometry."""
    return ((h + 15) // 16) * 16 + 2, (((w + 63) // 64) * 64 if w >= 512 else ((w + 15) // 16) * 16) + 2


class SRMap:
    """One split-resident map: ``t`` is a bf16 tensor [channels/8, 2 (hi, lo), hp, wp, 8]; pixel (y, x) sits at [.., y+1, x+1, :]."""
    __slots__ = ("t", "channels", "h", "w", "hp", "wp")

    def __init__(self, t, channels, h, w):
        self.t, self.channels, self.h, self.w = t, channels, h, w
        self.hp, self.wp = t.shape[2], t.shape[3]

    def parts(self):
        """(hi, lo) as fp32 [channels, h, w] tensors (tests / debugging; plain torch)."""
        v = self.t[:, :, 1:self.h + 1, 1:self.w + 1, :].float()          # [o, 2, h, w, 8]
        v = v.permute(1, 0, 4, 2, 3).reshape(2, self.channels, self.h, self.w)
        return v[0], v[1]


def sr_alloc(n_maps, channels, h, w, device, clear=True):
    """``n_maps`` SR maps of one geometry in one allocation -> list of SRMap.  The border is zeroed here (one small launch) unless
    ``clear`` is False (the caller clears several blocks at once with ``sr_clear_border``)."""
    if channels % 8:
        raise ValueError("SR maps hold whole octets of channels")
    hp, wp = sr_geometry(h, w)
    block = torch.empty(n_maps, channels // 8, 2, hp, wp, 8, device=device, dtype=torch.bfloat16)
    maps = [SRMap(block[i], channels, h, w) for i in range(n_maps)]
    if clear:
        sr_clear_border([maps])
    return maps


def _sr(m, name):
    if not isinstance(m, SRMap):
        raise TypeError(f"{name}: expected an SRMap")
    t_ = m.t
    if not t_.is_cuda:
        raise EffiLibraryError(f"{name}: CPU tensor passed to the HIP path (no CPU fallback exists)")
    if t_.device.index != torch._C._cuda_getDevice():
        raise EffiLibraryError(f"{name}: map lives on cuda:{t_.device.index} but the current device is cuda:{torch._C._cuda_getDevice()}")
    if t_.dtype != torch.bfloat16 or not t_.is_contiguous():
        raise ValueError(f"{name}: SR maps are contiguous bf16 tensors")
    return m


def _sr_groups(groups, name):
    """(first map, plane count) of each group of SR maps: consecutive maps of ONE allocation and geometry."""
    firsts = [_sr(g[0], "SR map") for g in groups]
    planes = [2 * (g[0].channels // 8) * len(g) for g in groups]
    for g in groups:       # consecutive maps of one allocation
        step = g[0].t.numel() * 2
        if any(m.t.data_ptr() != g[0].t.data_ptr() + i * step for i, m in enumerate(g)):
            raise ValueError(f"{name}: a group must be consecutive maps of one sr_alloc block")
    return firsts, planes


def sr_clear_border(groups):
    """Zero the borders of up to 4 groups of SR maps (each group: consecutive maps of ONE allocation and geometry) in one launch."""
    if not 1 <= len(groups) <= 4:
        raise ValueError("sr_clear_border: 1..4 groups")
    firsts, planes = _sr_groups(groups, "sr_clear_border")
    check(_lib.lib().effi_sr_clear_border(_ptr_array([m.t for m in firsts]), _int_array(planes), _int_array([m.h for m in firsts]),
                                           _int_array([m.w for m in firsts]), _int_array([m.hp for m in firsts]),
                                           _int_array([m.wp for m in firsts]), len(groups), _stream()), "effi_sr_clear_border")


def sr_from_planar(x, out=None):
    """fp32 [C,h,w] -> SRMap (a block boundary of the update block: e.g. a caller-supplied hidden state)."""
    _t(x, "map")
    Cc, h, w = x.shape
    if out is None:
        out = sr_alloc(1, Cc, h, w, x.device)[0]
    check(_lib.lib().effi_sr_from_planar_f32(_p(x), Cc, h, w, _p(_sr(out, "SR map").t), out.hp, out.wp, _stream()), "effi_sr_from_planar_f32")
    return out


def split_tanh_relu_stages_sr(ctxs, hds, cds, hidden_srs, q4=None, clear=None):
    """``split_tanh_relu_stages`` that also writes each hidden state into the given SRMap -> [(hidden, inp), ...] (fp32).
    ``q4``: per stage, write the fp32 hidden state in the Q4 layout (same shape [hd,h,w] tensor, values ordered [hd/4][h][w][4]).
    ``clear``: per stage, a group of SR maps of the stage's geometry (as for ``sr_clear_border``) whose borders the same launch zeroes."""
    outs = []
    for c_, hd, cd, m in zip(ctxs, hds, cds, hidden_srs):
        _t(c_, "context"), _sr(m, "hidden SR map")
        _, h, w = c_.shape
        if (m.channels, m.h, m.w) != (hd, h, w):
            raise ValueError("split_tanh_relu_stages_sr: SR map does not match the hidden state")
        outs.append((torch.empty(hd, h, w, device=c_.device, dtype=torch.float32),
                     torch.empty(cd, h, w, device=c_.device, dtype=torch.float32)))
    if len(ctxs) > 4:
        raise ValueError("split_tanh_relu_stages_sr: up to 4 stages")
    if clear is not None:
        if len(clear) != len(ctxs) or any((g[0].h, g[0].w, g[0].hp, g[0].wp) != (m.h, m.w, m.hp, m.wp) for g, m in zip(clear, hidden_srs)):
            raise ValueError("split_tanh_relu_stages_sr: one group of maps of the stage's geometry per stage")
        firsts, planes = _sr_groups(clear, "split_tanh_relu_stages_sr")
        check(_lib.lib().effi_split_tanh_relu_stages_sr_clear_f32(
            _ptr_array(ctxs), _int_array(list(hds)), _int_array(list(cds)), _int_array([c_.shape[1] for c_ in ctxs]),
            _int_array([c_.shape[2] for c_ in ctxs]), _ptr_array([o[0] for o in outs]), _ptr_array([m.t for m in hidden_srs]),
            _int_array([m.hp for m in hidden_srs]), _int_array([m.wp for m in hidden_srs]), _ptr_array([o[1] for o in outs]),
            _int_array([int(bool(v)) for v in (q4 if q4 is not None else [0] * len(ctxs))]), _ptr_array([m.t for m in firsts]),
            _int_array(planes), len(ctxs), _stream()), "effi_split_tanh_relu_stages_sr_clear_f32")
        return outs
    check(_lib.lib().effi_split_tanh_relu_stages_sr_f32(
        _ptr_array(ctxs), _int_array(list(hds)), _int_array(list(cds)), _int_array([c_.shape[1] for c_ in ctxs]),
        _int_array([c_.shape[2] for c_ in ctxs]), _ptr_array([o[0] for o in outs]), _ptr_array([m.t for m in hidden_srs]),
        _int_array([m.hp for m in hidden_srs]), _int_array([m.wp for m in hidden_srs]), _ptr_array([o[1] for o in outs]),
        _int_array([int(bool(v)) for v in (q4 if q4 is not None else [0] * len(ctxs))]), len(ctxs),
        _stream()), "effi_split_tanh_relu_stages_sr_f32")
    return outs


def encoder_inputs_sr(x, disp_range, interval, cur_vol, reg_vol, dmin, dmax, nq, h, w, weight_c1, bias_c1, weight_d1, bias_d1, cout,
                      out_c1, out_d1):
    """``encoder_inputs`` (split precision) writing relu(convc1(cost)) and relu(convd1(x)) as SR maps."""
    _t(x, "inv_depth"), _t(interval, "interval"), _t(disp_range, "disp_range")
    for t_ in (weight_c1, bias_c1, weight_d1, bias_d1):
        _t(t_, "encoder weights")
    _sr(out_c1, "out_c1"), _sr(out_d1, "out_d1")
    look, Dc, Dr, _keep = _lookup_args(cur_vol, reg_vol, dmin, dmax, h, w)
    if (out_c1.channels, out_c1.h, out_c1.w) != (cout, h, w) or (out_d1.channels, out_d1.h, out_d1.w) != (cout, h, w):
        raise ValueError("encoder_inputs_sr: output maps must be [cout,h,w]")
    work = lambda: {"flops": 2.0 * h * w * (2 * nq + 49) * cout, "bytes": 4.0 * h * w * (2 * cout + 1 + Dc + Dr)}
    check(_call("encoder_inputs", work, _lib.lib().effi_encoder_inputs_bf16x3_sr, _p(x), _p(disp_range), disp_range.numel(),
                _p(interval), *look, nq, h, w, _p(weight_c1), _p(bias_c1), _p(weight_d1), _p(bias_d1), cout, _p(out_c1.t), _p(out_d1.t),
                out_c1.hp, out_c1.wp, _stream()), "effi_encoder_inputs_bf16x3_sr")
    return out_c1, out_d1


def encoder_pair_gen_sr(x, disp_range, interval, cur_vol, reg_vol, dmin, dmax, nq, h, w, weight_c1, bias_c1, weight_d1, bias_d1, hd,
                        wpack_c2, bias_c2, out_c2, wpack_d2, bias_d2, out_d2, cout, act=ACT_RELU):
    """``encoder_inputs_sr`` + ``conv2d_k3_pair_sr`` in one launch (models/update.py:86-91): the 1x1 / 7x7 results are generated tile by
    tile inside the 3x3 kernel.  -> (act(convc2(cor1)), act(convd2(dfm1))) as SR maps; bitwise equal to the two launches."""
    _t(x, "inv_depth"), _t(interval, "interval"), _t(disp_range, "disp_range")
    for t_ in (weight_c1, bias_c1, weight_d1, bias_d1):
        _t(t_, "encoder weights")
    g = _sr_srcs([out_c2, out_d2])
    look, Dc, Dr, _keep = _lookup_args(cur_vol, reg_vol, dmin, dmax, h, w)
    if (g.channels, g.h, g.w) != (cout, h, w) or tuple(x.shape[-2:]) != (h, w):
        raise ValueError("encoder_pair_gen_sr: output maps must be [cout,h,w]")
    work = lambda: {"flops": 2.0 * h * w * ((2 * nq + 49) * hd + 2 * 9 * hd * cout), "bytes": 4.0 * h * w * (2 * cout + 1 + Dc + Dr)}
    check(_call(f"encgen_pair_nt{(cout + 15) // 16}", work, _x3("effi_encoder_pair_gen_bf16x3_sr"), _p(x), _p(disp_range),
                disp_range.numel(), _p(interval), *look, nq,
                h, w, _p(weight_c1), _p(bias_c1), _p(weight_d1), _p(bias_d1), hd, _p(wpack_c2), _p(bias_c2), _p(out_c2.t), _p(wpack_d2),
                _p(bias_d2), _p(out_d2.t), cout, g.hp, g.wp, act, _stream()), "effi_encoder_pair_gen_bf16x3_sr")
    return out_c2, out_d2


def _sr_srcs(srcs):
    for m in srcs:
        _sr(m, "conv2d input")
        if m.channels % 16:
            raise ValueError("SR convolution sources hold multiples of 16 channels")
    g = srcs[0]
    if any((m.h, m.w, m.hp, m.wp) != (g.h, g.w, g.hp, g.wp) for m in srcs):
        raise ValueError("SR convolution sources must share one geometry")
    return g


EPI_Q4 = 0x100          # include/effi_mvs_hip.h: EFFI_EPI_Q4


def q4_from_planar(x):
    """fp32 [C,h,w] -> the same values as [C/4,h,w,4] (the "Q4" layout of EFFI_EPI_Q4; tests and callers that hold planar state)."""
    C_, h, w = x.shape
    return x.view(C_ // 4, 4, h, w).permute(0, 2, 3, 1).contiguous()


def q4_to_planar(x, channels):
    """inverse of ``q4_from_planar``: a [C/4,h,w,4] block (any view of C*h*w floats) -> planar [C,h,w]."""
    h, w = x.shape[-3:-1] if x.dim() == 4 else (None, None)
    q = x.reshape(channels // 4, -1, 4) if h is None else x
    return q.permute(0, 3, 1, 2).reshape(channels, *q.shape[1:3]).contiguous()


def conv2d_k3_sr(srcs, wpack, bias, cout, epilogue=EPI_PLAIN, act=ACT_NONE, aux0=None, aux1=None, out0=None, out_sr=None, q4=False):
    """``conv2d_k3_bf16x3`` on SR maps.  PLAIN: -> out_sr (and out0 fp32 if given); GRU_ZR: -> (z fp32, r*h SR), aux0 = h fp32;
    GRU_Q: -> (h' fp32, h' SR), aux0 = h, aux1 = z.  ``q4`` (GRU epilogues): aux0 / aux1 / out0 hold their values as
    [C/4,h,w,4] instead of planar [C,h,w] (same number of floats; EFFI_EPI_Q4: one 16-byte access per lane and map)."""
    g = _sr_srcs(srcs)
    h, w = g.h, g.w
    dev = g.t.device
    c_out_sr = cout // 2 if epilogue == EPI_GRU_ZR else cout
    if out_sr is None:
        out_sr = sr_alloc(1, c_out_sr, h, w, dev)[0]
    _sr(out_sr, "out_sr")
    if (out_sr.channels, out_sr.h, out_sr.w) != (c_out_sr, h, w):
        raise ValueError("conv2d_k3_sr: output map does not match")
    if out0 is None and epilogue in (EPI_GRU_ZR, EPI_GRU_Q):
        out0 = torch.empty(c_out_sr, h, w, device=dev, dtype=torch.float32)
    for a_ in (aux0, aux1, out0):
        if a_ is not None:
            _t(a_, "fp32 map")
    cin = sum(m.channels for m in srcs)
    work = lambda: {"flops": 2.0 * h * w * cin * cout * 9, "bytes": 4.0 * h * w * (cin + cout)}
    check(_call(f"conv2d_k3x3_nt{(cout + 15) // 16}_epi{epilogue}", work, _x3("effi_conv2d_k3_bf16x3_sr"), _ptr_array([m.t for m in srcs]),
                _int_array([m.channels for m in srcs]), len(srcs), _p(wpack), _p(bias), cout, h, w, g.hp, g.wp,
                epilogue | (EPI_Q4 if (q4 and epilogue in (EPI_GRU_ZR, EPI_GRU_Q)) else 0), act,
                _p(aux0), _p(aux1), _p(out0), _p(out_sr.t), _stream()), "effi_conv2d_k3_bf16x3_sr")
    return (out0, out_sr) if out0 is not None else out_sr


def gru_zr_q_fused_sr(H_in, X, h_in, wzr_pack, bias_zr, wq_pack, bias_q, h_out, H_out):
    """ConvGRU in one launch (csrc/gru_fused.hpp): SR maps ``H_in`` (state) and ``X`` (encoder output), fp32 state ``h_in`` ->
    (``h_out`` fp32, ``H_out`` SR); outputs must be other buffers than the inputs.  Bitwise equal to ``conv2d_k3_sr(GRU_ZR)`` +
    ``conv2d_k3_sr(GRU_Q)``."""
    g = _sr_srcs([H_in, X, H_out])
    hd, h, w = g.channels, g.h, g.w
    _t(h_in, "h"), _t(h_out, "h_out")
    if tuple(h_in.shape) != (hd, h, w) or tuple(h_out.shape) != (hd, h, w) or X.channels != hd or H_out.channels != hd:
        raise ValueError("gru_zr_q_fused_sr: state / input maps must hold hd channels of one size")
    if h_out.data_ptr() == h_in.data_ptr() or H_out.t.data_ptr() in (H_in.t.data_ptr(), X.t.data_ptr()):
        raise ValueError("gru_zr_q_fused_sr: outputs must not alias inputs")
    work = lambda: {"flops": 2.0 * h * w * 9 * (2 * hd * 2 * hd + 2 * hd * hd), "bytes": 4.0 * h * w * 5 * hd}
    check(_call(f"gru_fused_nt{hd // 16}", work, _x3("effi_gru_zr_q_fused_bf16x3_sr"), _p(H_in.t), _p(X.t), _p(h_in), _p(wzr_pack), _p(bias_zr),
                _p(wq_pack), _p(bias_q), hd, h, w, g.hp, g.wp, _p(h_out), _p(H_out.t), _stream()), "effi_gru_zr_q_fused_bf16x3_sr")
    return h_out, H_out


def conv2d_k3_pair_sr(srcs_a, wpack_a, bias_a, out_a, srcs_b, wpack_b, bias_b, out_b, cout, act=ACT_NONE):
    """``conv2d_k3_bf16x3_pair`` on SR maps (SR in, SR out)."""
    g = _sr_srcs(list(srcs_a) + list(srcs_b) + [out_a, out_b])
    h, w = g.h, g.w
    cin = sum(m.channels for m in srcs_a) + sum(m.channels for m in srcs_b)
    work = lambda: {"flops": 2.0 * h * w * cin * cout * 9, "bytes": 4.0 * h * w * (cin + 2 * cout)}
    check(_call(f"conv2d_k3x3_pair_nt{(cout + 15) // 16}", work, _x3("effi_conv2d_k3_bf16x3_pair_sr"), _ptr_array([m.t for m in srcs_a]),
                _int_array([m.channels for m in srcs_a]), len(srcs_a), _p(wpack_a), _p(bias_a), _p(out_a.t),
                _ptr_array([m.t for m in srcs_b]), _int_array([m.channels for m in srcs_b]), len(srcs_b), _p(wpack_b), _p(bias_b),
                _p(out_b.t), cout, h, w, g.hp, g.wp, act, _stream()), "effi_conv2d_k3_bf16x3_pair_sr")
    return out_a, out_b


def conv2d_k3_k1_sr(srcs, wpack, bias, cout1, extra, w2pack, bias2, cout2, relu=True, relu1=False, out=None, out_sr=None):
    """``conv2d_k3_k1_x3`` on SR inputs -> ``out_sr`` (SRMap) if given, else fp32 [cout2,h,w]."""
    g = _sr_srcs(srcs)
    h, w = g.h, g.w
    c_extra = 0
    if extra is not None:
        _t(extra, "extra channels")
        c_extra = extra.shape[0]
    if out_sr is None and out is None:
        out = torch.empty(cout2, h, w, device=g.t.device, dtype=torch.float32)
    if out_sr is not None:
        _sr(out_sr, "out_sr")
        if (out_sr.channels, out_sr.h, out_sr.w) != (cout2, h, w):
            raise ValueError("conv2d_k3_k1_sr: output map does not match")
    cin = sum(m.channels for m in srcs)
    work = lambda: {"flops": 2.0 * h * w * (cin * cout1 * 9 + (cout1 + c_extra) * cout2),
                    "bytes": 4.0 * h * w * (cin + c_extra + cout2)}
    check(_call(f"conv2d_k3k1_nt{(cout1 + 15) // 16}", work, _x3("effi_conv2d_k3_k1_bf16x3_sr"), _ptr_array([m.t for m in srcs]),
                _int_array([m.channels for m in srcs]), len(srcs), _p(wpack), _p(bias), cout1, int(relu1), _p(extra), c_extra,
                _p(w2pack), _p(bias2), cout2, int(relu), h, w, g.hp, g.wp, _p(None if out_sr is not None else out),
                _p(out_sr.t if out_sr is not None else None), _stream()), "effi_conv2d_k3_k1_bf16x3_sr")
    return out_sr if out_sr is not None else out


def depth_head_sr(srcs, wpack, bias, cout1, w2pack, bias2_taps, bias2, inv_depth, disp_range, tile):
    """``conv2d_k3_k1_sr`` with the depth head's nine tap projections + ``head_update`` in one launch (the tap planes stay in LDS)
    -> (inv_depth + tanh(conv2(relu(conv1)))), its depth), both [1,h,w].  ``tile``: 2, 4 or 8 (effi_depth_head_bf16x3_sr)."""
    g = _sr_srcs(srcs)
    _t(inv_depth, "inv_depth"), _t(disp_range, "disp_range"), _t(bias2, "bias")
    h, w = g.h, g.w
    if inv_depth.numel() != h * w:
        raise ValueError("depth_head_sr: inv_depth must hold h*w values")
    out_inv = torch.empty(1, h, w, device=g.t.device, dtype=torch.float32)
    out_depth = torch.empty(1, h, w, device=g.t.device, dtype=torch.float32)
    cin = sum(m.channels for m in srcs)
    work = lambda: {"flops": 2.0 * h * w * (cin * cout1 * 9 + cout1 * 9), "bytes": 4.0 * h * w * (cin + 3)}
    check(_call(f"depth_head_nt{(cout1 + 15) // 16}", work, _x3("effi_depth_head_bf16x3_sr"), _ptr_array([m.t for m in srcs]),
                _int_array([m.channels for m in srcs]), len(srcs), _p(wpack), _p(bias), cout1, _p(w2pack), _p(bias2_taps), _p(bias2),
                _p(inv_depth), _p(disp_range), disp_range.numel(), h, w, g.hp, g.wp, int(tile), _p(out_inv), _p(out_depth), _stream()),
          "effi_depth_head_bf16x3_sr")
    return out_inv, out_depth


def conv2d_k3_k1_up2x_sr(srcs, wpack, bias, cout1, w2pack, bias2, inv_depth, disp_range, want_depth_inv=True):
    """``conv2d_k3_k1_up2x`` on SR inputs."""
    g = _sr_srcs(srcs)
    _t(inv_depth, "inv_depth"), _t(disp_range, "disp_range")
    h, w = g.h, g.w
    dev = g.t.device
    out_depth = torch.empty(2 * h, 2 * w, device=dev, dtype=torch.float32)
    out_dinv = torch.empty(2 * h, 2 * w, device=dev, dtype=torch.float32) if want_depth_inv else None
    cin = sum(m.channels for m in srcs)
    work = lambda: {"flops": 2.0 * h * w * (cin * cout1 * 9 + cout1 * 36), "bytes": 4.0 * h * w * (cin + 1 + 8)}
    check(_call(f"conv2d_k3k1up_nt{(cout1 + 15) // 16}", work, _x3("effi_conv2d_k3_k1_up2x_bf16x3_sr"), _ptr_array([m.t for m in srcs]),
                _int_array([m.channels for m in srcs]), len(srcs), _p(wpack), _p(bias), cout1, _p(w2pack), _p(bias2), _p(inv_depth),
                _p(disp_range), disp_range.numel(), h, w, g.hp, g.wp, _p(out_depth), _p(out_dinv), _stream()),
          "effi_conv2d_k3_k1_up2x_bf16x3_sr")
    return out_depth, out_dinv


def conv2d_k3_k1_x3(srcs, wpack, bias, cout1, extra, w2pack, bias2, cout2, relu=True, out=None, relu1=False):
    """3x3 split-precision conv (ReLU if ``relu1``) + the 1x1 conv over cat(result, ``extra``) in one kernel
    (``packing.pack_conv2d_bf16x3`` / ``packing.pack_conv1x1_after``) -> [cout2,h,w]."""
    for s in srcs:
        _t(s, "conv2d input")
    h, w = srcs[0].shape[-2:]
    c_extra = 0
    if extra is not None:
        _t(extra, "extra channels")
        c_extra = extra.shape[0]
    if out is None:
        out = torch.empty(cout2, h, w, device=srcs[0].device, dtype=torch.float32)
    cin = sum(s.shape[0] for s in srcs)
    work = lambda: {"flops": 2.0 * h * w * (cin * cout1 * 9 + (cout1 + c_extra) * cout2),
                    "bytes": 4.0 * h * w * (cin + c_extra + cout2)}
    check(_call(f"conv2d_k3k1_nt{(cout1 + 15) // 16}", work, _x3("effi_conv2d_k3_k1_bf16x3_f32"), _ptr_array(srcs),
                _int_array([s.shape[0] for s in srcs]), len(srcs), _p(wpack), _p(bias), cout1, int(relu1), _p(extra), c_extra,
                _p(w2pack), _p(bias2), cout2, int(relu), h, w, _p(out), _stream()), "effi_conv2d_k3_k1_bf16x3_f32")
    return out


def conv2d_k3_twice(x, w1, b1, w2, b2, cout, out=None):
    """relu(conv3x3(relu(conv3x3(x)))) with at most 8 channels into each layer (8 between them) in one kernel, the intermediate map
    in LDS (``packing.pack_conv2d_bf16x3_oct`` weights): the pyramid's full-resolution block.  x [cin<=8,h,w] -> [cout<=8,h,w], or
    an image batch [n,cin,h,w] -> [n,cout,h,w] in one launch (image i bitwise the 3-D call on image i)."""
    n, istr = _in(x, 3, "conv input")
    cin, h, w = x.shape[-3:]
    out = _out(n, (cout, h, w), x.device, out, "conv output")
    reps, sfx = (1, "") if n is None else (n, "_batch")
    work = lambda: {"flops": 2.0 * reps * h * w * 9 * (cin * 8 + 8 * cout), "bytes": 4.0 * reps * h * w * (cin + cout)}
    _launch("effi_conv2d_k3_twice_bf16x3_f32", (_p(x), cin, _p(w1), _p(b1), _p(w2), _p(b2), cout, h, w, _p(out)), n,
            lambda: (istr, out.stride(0) if n > 1 else 0), key="conv2d_k3_twice" + sfx, work=work, x3=True)
    return out


def encoder_tail(cor1, dfm1, wc2, bc2, wd2, bd2, wd, bd, cmix, extra, w2pack, bias2, cout2, out=None):
    """relu(convc2(cor1)), relu(convd2(dfm1)) -> convd over their concatenation -> 1x1 convc over cat(., extra) + ReLU in ONE kernel
    (the two intermediate maps stay in LDS): ``conv2d_k3_bf16x3_pair`` followed by ``conv2d_k3_k1_x3``.  hd == 16 only."""
    _t(cor1, "cor1"), _t(dfm1, "dfm1"), _t(extra, "extra channels")
    hd, h, w = cor1.shape
    if dfm1.shape != cor1.shape or extra.shape[-2:] != cor1.shape[-2:]:
        raise ValueError("encoder_tail: cor1, dfm1 and the extra channels must share one map size")
    if out is None:
        out = torch.empty(cout2, h, w, device=cor1.device, dtype=torch.float32)
    c_extra = extra.shape[0]
    work = lambda: {"flops": 2.0 * h * w * (2 * hd * hd * 9 + 2 * hd * cmix * 9 + (cmix + c_extra) * cout2),
                    "bytes": 4.0 * h * w * (2 * hd + c_extra + cout2)}
    check(_call("encoder_tail", work, _x3("effi_encoder_tail_bf16x3_f32"), _p(cor1), _p(dfm1), hd, _p(wc2), _p(bc2), _p(wd2), _p(bd2),
                _p(wd), _p(bd), cmix, _p(extra), c_extra, _p(w2pack), _p(bias2), cout2, h, w, _p(out), _stream()),
          "effi_encoder_tail_bf16x3_f32")
    return out


def conv2d_k3_k1_up2x(srcs, wpack, bias, cout1, w2pack, bias2, inv_depth, disp_range, want_depth_inv=True):
    """Mask head (3x3 + ReLU + 1x1 to 36 channels) and the convex x2 upsampling it feeds in one kernel: inv_depth [1,h,w] or [h,w]
    -> (depth [2h,2w], depth_to_inv(depth) [2h,2w] or None).  cout1 in {32, 64, 96}."""
    for s_ in srcs:
        _t(s_, "conv2d input")
    _t(inv_depth, "inv_depth"), _t(disp_range, "disp_range")
    h, w = srcs[0].shape[-2:]
    dev = srcs[0].device
    out_depth = torch.empty(2 * h, 2 * w, device=dev, dtype=torch.float32)
    out_dinv = torch.empty(2 * h, 2 * w, device=dev, dtype=torch.float32) if want_depth_inv else None
    cin = sum(s_.shape[0] for s_ in srcs)
    work = lambda: {"flops": 2.0 * h * w * (cin * cout1 * 9 + cout1 * 36), "bytes": 4.0 * h * w * (cin + 1 + 8)}
    check(_call(f"conv2d_k3k1up_nt{(cout1 + 15) // 16}", work, _x3("effi_conv2d_k3_k1_up2x_bf16x3_f32"), _ptr_array(srcs),
                _int_array([s_.shape[0] for s_ in srcs]), len(srcs), _p(wpack), _p(bias), cout1, _p(w2pack), _p(bias2), _p(inv_depth),
                _p(disp_range), disp_range.numel(), h, w, _p(out_depth), _p(out_dinv), _stream()), "effi_conv2d_k3_k1_up2x_bf16x3_f32")
    return out_depth, out_dinv


def conv2d_k5s2(x, wpack, bias, cout, act=ACT_RELU):
    """5x5 stride-2 pad-2 convolution (+bias, activation): x planar [cin,hin,win] -> [cout,ceil(hin/2),ceil(win/2)], or an image
    batch [n,cin,hin,win] -> [n,cout,...] in one launch (image i bitwise the 3-D call on image i)."""
    n, istr = _in(x, 3, "conv input")
    cin, hin, win = x.shape[-3:]
    ho, wo = _conv_out(hin, 2), _conv_out(win, 2)
    out = _out(n, (cout, ho, wo), x.device, None, "conv output")
    reps, sfx = (1, "") if n is None else (n, "_batch")
    work = lambda: {"flops": 2.0 * reps * ho * wo * cin * cout * 25, "bytes": 4.0 * reps * (hin * win * cin + ho * wo * cout)}
    split = False
    if hasattr(wpack, "w32"):                 # packing.Conv2dWeights: pick the arithmetic here
        split = uses_split() and wpack.wx is not None and win % 4 == 0 and _PY_OPTS["k5s2_split"] != 0
        wpack = wpack.wx if split else wpack.w32
    _launch("effi_conv2d_k5s2_bf16x3_f32" if split else "effi_conv2d_k5s2_f32", (_p(x), cin, _p(wpack), _p(bias), cout, hin, win, act, _p(out)),
            n, lambda: (istr, out.stride(0) if n > 1 else 0), key=f"conv2d_k5s2{'x3' if split else ''}_nt{(cout + 15) // 16}{sfx}",
            work=work, x3=split)
    return out


def conv2d_c1k7_relu(x, weight, bias, cout, out=None, exact=False):
    """7x7 single-input-channel convolution + ReLU (ProjectionInput.convd1).  ``exact``: exact fp32 products whatever
    ``get_precision()`` says (the training path, whose weight gradient is taken against this output)."""
    _t(x, "conv7 input")
    h, w = x.shape[-2:]
    if out is None:
        out = torch.empty(cout, h, w, device=x.device, dtype=torch.float32)
    if not exact and uses_split() and _PY_OPTS["c1k7_mfma"] != 0:
        check(_lib.lib().effi_conv2d_c1k7_relu_bf16x3_f32(_p(x), _p(weight), _p(bias), cout, h, w, _p(out), _stream()),
              "effi_conv2d_c1k7_relu_bf16x3_f32")
        return out
    check(_lib.lib().effi_conv2d_c1k7_relu_f32(_p(x), _p(weight), _p(bias), cout, h, w, _p(out), _stream()),
          "effi_conv2d_c1k7_relu_f32")
    return out


def convex_upsample2x(inv_depth, mask, disp_range=None, want_inv=True, want_depth_inv=False):
    """-> (inv [2h,2w] or None, depth [2h,2w] or None); depth needs ``disp_range``.  ``want_depth_inv``: a third result,
    ``depth_to_inv(depth)`` (what the next stage starts from), written by the same kernel."""
    _t(inv_depth, "inv_depth"), _t(mask, "mask")
    h, w = inv_depth.shape[-2:]
    if mask.shape[0] != 36:
        raise NotImplementedError("convex upsampling is instantiated for ratio 2 (36 mask channels)")
    out_inv = torch.empty(2 * h, 2 * w, device=mask.device, dtype=torch.float32) if want_inv else None
    out_depth = None
    n_range = 0
    if disp_range is not None:
        _t(disp_range, "disp_range")
        n_range = disp_range.numel()
        out_depth = torch.empty(2 * h, 2 * w, device=mask.device, dtype=torch.float32)
    out_dinv = torch.empty(2 * h, 2 * w, device=mask.device, dtype=torch.float32) if (want_depth_inv and out_depth is not None) else None
    check(_lib.lib().effi_convex_upsample2x_f32(_p(inv_depth), _p(mask), _p(disp_range), n_range, h, w,
                                                 _p(out_inv), _p(out_depth), _p(out_dinv), _stream()), "effi_convex_upsample2x_f32")
    return (out_inv, out_depth, out_dinv) if want_depth_inv else (out_inv, out_depth)


def split_tanh_relu(ctx, hd, cd):
    _t(ctx, "context")
    _, h, w = ctx.shape
    hid = torch.empty(hd, h, w, device=ctx.device, dtype=torch.float32)
    inp = torch.empty(cd, h, w, device=ctx.device, dtype=torch.float32)
    check(_lib.lib().effi_split_tanh_relu_f32(_p(ctx), hd, cd, h * w, _p(hid), _p(inp), _stream()),
          "effi_split_tanh_relu_f32")
    return hid, inp


def split_tanh_relu_stages(ctxs, hds, cds):
    """``split_tanh_relu`` of up to 4 context maps (the stages of the cascade) in one launch -> [(hidden, inp), ...]."""
    outs, hws = [], []
    for c_, hd, cd in zip(ctxs, hds, cds):
        _t(c_, "context")
        _, h, w = c_.shape
        hws.append(h * w)
        outs.append((torch.empty(hd, h, w, device=c_.device, dtype=torch.float32),
                     torch.empty(cd, h, w, device=c_.device, dtype=torch.float32)))
    if len(ctxs) > 4:
        raise ValueError("split_tanh_relu_stages: up to 4 stages")
    check(_lib.lib().effi_split_tanh_relu_stages_f32(_ptr_array(ctxs), _int_array(list(hds)), _int_array(list(cds)), _int_array(hws),
                                                      _ptr_array([o[0] for o in outs]), _ptr_array([o[1] for o in outs]), len(ctxs),
                                                      _stream()), "effi_split_tanh_relu_stages_f32")
    return outs


def depth_to_inv(depth, disp_range):
    _t(depth, "depth"), _t(disp_range, "disp_range")
    out = torch.empty_like(depth)
    check(_lib.lib().effi_depth_to_inv_f32(_p(depth), _p(disp_range), disp_range.numel(), depth.numel(), _p(out),
                                            _stream()), "effi_depth_to_inv_f32")
    return out


def stage1_hypotheses(disp_range, D):
    _t(disp_range, "disp_range")
    depths = torch.empty(D, device=disp_range.device, dtype=torch.float32)
    intervals = torch.empty(5, device=disp_range.device, dtype=torch.float32)   # 3 intervals, depth_min_, depth_max_
    check(_lib.lib().effi_stage1_hypotheses_f32(_p(disp_range), disp_range.numel(), D, _p(depths), _p(intervals),
                                                 _stream()), "effi_stage1_hypotheses_f32")
    return depths, intervals


def upsample_nearest(x, f):
    _t(x, "map")
    Cc, h, w = x.shape
    out = torch.empty(Cc, h * f, w * f, device=x.device, dtype=torch.float32)
    check(_lib.lib().effi_upsample_nearest_f32(_p(x), Cc, h, w, f, _p(out), _stream()), "effi_upsample_nearest_f32")
    return out


def head_update(partial9, bias2, inv_depth, disp_range):
    """Tail of the depth head when conv2's nine tap projections were applied by conv1's kernel (``conv2d_k3_k1_x3`` with
    ``packing.pack_head_taps``): partial9 [9,h,w], inv_depth [1,h,w] -> (inv_depth + tanh(conv2), its depth), both [1,h,w]."""
    _t(partial9, "partial sums"), _t(bias2, "bias"), _t(inv_depth, "inv_depth"), _t(disp_range, "disp_range")
    if partial9.dim() != 3 or partial9.shape[0] != 9:
        raise ValueError("head_update: partial sums must be [9,h,w]")
    h, w = partial9.shape[-2:]
    if inv_depth.numel() != h * w:
        raise ValueError("head_update: inv_depth must hold h*w values")
    out_inv = torch.empty(1, h, w, device=partial9.device, dtype=torch.float32)
    out_depth = torch.empty(1, h, w, device=partial9.device, dtype=torch.float32)
    work = lambda: {"flops": 30.0 * h * w, "bytes": 4.0 * h * w * 12}
    check(_call("head_update", work, _lib.lib().effi_head_update_f32, _p(partial9), _p(bias2), _p(inv_depth), _p(disp_range),
                disp_range.numel(), h, w, _p(out_inv), _p(out_depth), _stream()), "effi_head_update_f32")
    return out_inv, out_depth


# =============================================================================================
# scope row n2: training kernels (csrc/train_ops.hip, warpcorr_dyn backward); thin wrappers, shapes checked here
# =============================================================================================
PW_ACT_BWD = {ACT_RELU: 0, ACT_SIGMOID: 1, ACT_TANH: 2}
PW_TANH, PW_RELU, PW_SIGMOID, PW_MUL, PW_MUL_BWD, PW_GRU, PW_GRU_BWD, PW_INV_TO_DEPTH, PW_INV_TO_DEPTH_BWD, PW_SCALE_CH = 3, 4, 5, 6, 7, 8, 9, 10, 11, 12


def conv_wgrad(a, b, dw, cb_off, kd, ks, stride=(1, 1)):
    """dw[ca][cb_off + cb][taps] += sum_o a[ca][o] * b[cb][o*stride + tap - pad]   (a on the small grid, b on the large one;
    [c,h,w] or [c,D,h,w]); see effi_conv_wgrad_f32."""
    _t(a, "wgrad a"), _t(b, "wgrad b"), _t(dw, "wgrad dw")
    if a.dim() == 3:
        a, b = a.unsqueeze(1), b.unsqueeze(1)
    ca, Da, ha, wa = a.shape
    cb, Db, hb, wb = b.shape
    sz, sxy = int(stride[0]), int(stride[1])
    if (Da, ha, wa) != ((Db - 1) // sz + 1 if kd == 3 else Db, (hb - 1) // sxy + 1, (wb - 1) // sxy + 1):
        raise ValueError(f"conv_wgrad: grids {tuple(a.shape)} / {tuple(b.shape)} do not match stride {stride}")
    if dw.shape[0] != ca or dw.numel() != ca * dw.shape[1] * kd * ks * ks:
        raise ValueError("conv_wgrad: dw shape")
    check(_lib.lib().effi_conv_wgrad_f32(_p(a), _p(b), ca, cb, dw.shape[1], cb_off, kd, ks, Da, ha, wa, Db, hb, wb, sz, sxy, _p(dw),
                                         _stream()), "effi_conv_wgrad_f32")
    return dw


def conv2d_k5s2_dgrad(grad_out, weight, hin, win):
    """Input gradient of a 5x5 / stride-2 / padding-2 convolution: grad_out [cout,ho,wo], weight [cout,cin,5,5] -> [cin,hin,win]."""
    _t(grad_out, "grad_out"), _t(weight, "weight")
    cout, cin = weight.shape[0], weight.shape[1]
    if tuple(grad_out.shape) != (cout, (hin - 1) // 2 + 1, (win - 1) // 2 + 1):
        raise ValueError("conv2d_k5s2_dgrad: grad_out shape does not match the input size")
    gx = torch.empty(cin, hin, win, device=grad_out.device, dtype=torch.float32)
    check(_lib.lib().effi_conv2d_k5s2_dgrad_f32(_p(grad_out), _p(weight), cin, cout, hin, win, _p(gx), _stream()), "effi_conv2d_k5s2_dgrad_f32")
    return gx


def conv2d_k5s2_dgrad_mfma(grad_out, weight, hin, win):
    """``conv2d_k5s2_dgrad`` on the matrix cores: one 3x3 convolution over ``grad_out`` whose 4 cin output channels are the four pixel
    parities of the input gradient (weights re-arranged on the device, effi_pack_conv2d_k5s2_dgrad_f32), then a pixel shuffle."""
    _t(grad_out, "grad_out"), _t(weight, "weight")
    cout, cin = weight.shape[0], weight.shape[1]
    ho, wo = (hin - 1) // 2 + 1, (win - 1) // 2 + 1
    if tuple(grad_out.shape) != (cout, ho, wo):
        raise ValueError("conv2d_k5s2_dgrad: grad_out shape does not match the input size")
    planes = torch.empty(4 * cin, ho, wo, device=grad_out.device, dtype=torch.float32)
    kg = (cout + 3) // 4
    for c0 in range(0, cin, 16):                       # at most 64 output channels per launch
        cn = min(16, cin - c0)
        nt = (4 * cn + 15) // 16
        if nt == 5:
            raise NotImplementedError("conv2d_k5s2_dgrad_mfma: input channels must come in groups of 4 / 8 / 12 / 16")
        buf = torch.empty(kg * 9 * nt * 64 + 16 * nt, device=grad_out.device, dtype=torch.float32)
        wp, bp = buf[:kg * 9 * nt * 64], buf[kg * 9 * nt * 64:]
        check(_lib.lib().effi_pack_conv2d_k5s2_dgrad_f32(_p(weight), cout, cin, c0, cn, _p(wp), _p(bp), _stream()),
              "effi_pack_conv2d_k5s2_dgrad_f32")
        conv2d([grad_out], wp, bp, 4 * cn, 3, out0=planes[4 * c0:4 * (c0 + cn)])
    gx = torch.nn.functional.pixel_shuffle(planes.unsqueeze(0), 2)[0]                # [cin, 2 ho, 2 wo]
    return gx if (2 * ho, 2 * wo) == (hin, win) else gx[:, :hin, :win].contiguous()


# elements per workgroup of the split per-channel reductions.  8192 left the chip short of workgroups (8 channels x 40 workgroups at
# 512x640: 1.25 per CU, 27 us for a 31-MB pass); 2048 = 8 elements per thread
# (option reduce_chunk; graph-replayed training step 28.6 -> 26.3 ms)

def _reduce_split(total, channels, k=1, device=None):
    """Workgroups per channel of the split per-channel reductions and their scratch ([C][nsplit][k] floats): ~2 K elements per
    workgroup, at most 256 per channel, none when the tensor is small.  The partial sums are added in a fixed order (second launch)."""
    nsplit = int(min(256, max(1, total // _PY_OPTS["reduce_chunk"])))
    if nsplit <= 1:
        return None, 1
    return torch.empty(channels * nsplit * k, device=device, dtype=torch.float32), nsplit


def channel_sum(g):
    """[B,C,...] -> [C] sums over batch and positions."""
    _t(g, "channel_sum input")
    B, Cc = g.shape[0], g.shape[1]
    n = g.numel() // (B * Cc)
    out = torch.empty(Cc, device=g.device, dtype=torch.float32)
    scratch, nsplit = _reduce_split(B * n, Cc, 1, g.device)
    check(_lib.lib().effi_channel_sum_f32(_p(g), B, Cc, n, _p(out), _p(scratch), nsplit, _stream()), "effi_channel_sum_f32")
    return out


def bn_moments(x):
    """[B,C,...] -> (mean [C], biased variance [C]) over batch and positions (two passes: sum, then centred squares)."""
    _t(x, "bn input")
    B, Cc = x.shape[0], x.shape[1]
    n = x.numel() // (B * Cc)
    mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
    scratch, nsplit = _reduce_split(B * n, Cc, 1, x.device)
    check(_lib.lib().effi_bn_moment_f32(_p(x), B, Cc, n, None, 1, _p(mean), _p(scratch), nsplit, _stream()), "effi_bn_moment_f32")
    mean = mean / float(B * n)
    var = torch.empty(Cc, device=x.device, dtype=torch.float32)
    check(_lib.lib().effi_bn_moment_f32(_p(x), B, Cc, n, _p(mean), 2, _p(var), _p(scratch), nsplit, _stream()), "effi_bn_moment_f32")
    return mean, var / float(B * n)


def bn_train_fwd(x, gamma, beta, eps, momentum, running_mean=None, running_var=None, n_tracked=None, relu=False):
    """nn.BatchNorm (training mode) forward in one entry: -> (y, mean [C], invstd [C]); the running statistics (and the int64 counter
    ``n_tracked``) are updated in place when given."""
    _t(x, "bn input"), _t(gamma, "bn weight"), _t(beta, "bn bias")
    B, Cc = x.shape[0], x.shape[1]
    n = x.numel() // (B * Cc)
    nsplit = int(min(256, max(1, (B * n) // _PY_OPTS["reduce_chunk"])))
    buf = torch.empty(Cc * (2 * nsplit + 2), device=x.device, dtype=torch.float32)    # scratch (two passes) | mean | invstd in one allocation
    mean, invstd = buf[2 * Cc * nsplit:Cc * (2 * nsplit + 1)], buf[Cc * (2 * nsplit + 1):]
    y = torch.empty_like(x)
    if running_mean is not None:
        _t(running_mean, "running_mean"), _t(running_var, "running_var")
    if n_tracked is not None and (n_tracked.dtype != torch.int64 or n_tracked.device != x.device):
        raise ValueError("bn_train_fwd: num_batches_tracked must be an int64 tensor on the input's device")
    check(_lib.lib().effi_bn_train_fwd_f32(_p(x), B, Cc, n, _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean),
                                           _p(running_var), _p(n_tracked), int(relu), _p(y), _p(mean), _p(invstd), _p(buf), nsplit,
                                           _stream()), "effi_bn_train_fwd_f32")
    return y, mean, invstd


_PACK_CACHE = {}


def drop_pack_cache():
    """Forget every packed weight: needed after an update the version counters do not see (a replayed graph's optimizer step,
    writes through ``p.data``)."""
    _PACK_CACHE.clear()


def pack_conv2d_mfma_dev(weight, bias=None, dgrad=False):
    """``packing.pack_conv2d_mfma`` on the device in one launch (training: every layer, every step); ``dgrad``: the weights of the
    input-gradient convolution (``weight.flip(2, 3).transpose(0, 1)`` packed).  -> (wpack, bias_pack)."""
    _t(weight, "weight")
    cout, cin, ks, _ = weight.shape
    co, ci = (cin, cout) if dgrad else (cout, cin)
    if co == 1 and ks == 3:       # single-output-channel layers carry a second (vector) weight block: host form
        from . import packing
        w = weight.flip(2, 3).transpose(0, 1).contiguous() if dgrad else weight
        return packing.pack_conv2d_mfma(w, bias)
    # a layer is applied several times per step (five images through the feature pyramid, three GRU iterations per stage): its
    # packed weights are reused until the tensor changes (``_version`` counts in-place updates: the optimizer's) or dies
    # (entries made outside a graph capture are not valid inside one -- the replay must re-pack -- and vice versa)
    key = (id(weight), bool(dgrad), torch.cuda.is_current_stream_capturing())
    hit = _PACK_CACHE.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == weight._version and hit[2] is bias and (bias is None or hit[3] == bias._version):
        return hit[4], hit[5]
    nt, kg = (co + 15) // 16, (ci + 3) // 4
    buf = torch.empty(kg * ks * ks * nt * 64 + 16 * nt, device=weight.device, dtype=torch.float32)
    wp, bp = buf[:kg * ks * ks * nt * 64].view(kg, ks * ks, nt, 64), buf[kg * ks * ks * nt * 64:]
    if bias is not None:
        _t(bias, "bias")
    check(_lib.lib().effi_pack_conv2d_mfma_f32(_p(weight), _p(bias), cout, cin, ks, int(dgrad), _p(wp), _p(bp), _stream()),
          "effi_pack_conv2d_mfma_f32")
    if len(_PACK_CACHE) > 4096:
        _PACK_CACHE.clear()
    _PACK_CACHE[key] = (weakref.ref(weight), weight._version, bias, None if bias is None else bias._version, wp, bp)
    return wp, bp


def bn_apply(x, mean, invstd, gamma, beta, relu):
    _t(x, "bn input")
    B, Cc = x.shape[0], x.shape[1]
    y = torch.empty_like(x)
    check(_lib.lib().effi_bn_apply_f32(_p(x), B, Cc, x.numel() // (B * Cc), _p(mean), _p(invstd), _p(gamma), _p(beta), int(relu), _p(y),
                                       _stream()), "effi_bn_apply_f32")
    return y


def bn_bwd(gy, y, x, mean, invstd, gamma, relu):
    """-> (gx, s1 = grad beta, s2 = grad gamma)."""
    _t(gy, "bn grad"), _t(y, "bn output"), _t(x, "bn input")
    B, Cc = x.shape[0], x.shape[1]
    s1 = torch.empty(Cc, device=x.device, dtype=torch.float32)
    s2 = torch.empty(Cc, device=x.device, dtype=torch.float32)
    gx = torch.empty_like(x)
    n = x.numel() // (B * Cc)
    scratch, nsplit = _reduce_split(B * n, Cc, 4, x.device)           # [C][nsplit][2] doubles
    check(_lib.lib().effi_bn_bwd_f32(_p(gy), _p(y), _p(x), B, Cc, n, _p(mean), _p(invstd), _p(gamma), int(relu),
                                     _p(s1), _p(s2), _p(gx), _p(scratch), nsplit, _stream()), "effi_bn_bwd_f32")
    return gx, s1, s2


def pointwise(op, a, b=None, c=None, d=None, s0=0.0, s1=0.0, inner=1, C=1, n_out=1):
    """One of the EFFI_PW_* element-wise ops over ``a.numel()`` elements -> 1..3 outputs shaped like ``a``."""
    for t_ in (a, b, c, d):
        if t_ is not None:
            _t(t_, "pointwise operand")
    outs = [torch.empty_like(a) for _ in range(n_out)]
    o = outs + [None] * (3 - n_out)
    check(_lib.lib().effi_pointwise_f32(op, _p(a), _p(b), _p(c), _p(d), float(s0), float(s1), a.numel(), inner, C, _p(o[0]), _p(o[1]),
                                        _p(o[2]), _stream()), "effi_pointwise_f32")
    return outs[0] if n_out == 1 else outs


def _ranged_args(what, inv, depth_values, g=None, out=None):
    for t_, name in ((inv, "inv"), (depth_values, "depth_values"), (g, "grad"), (out, "out")):
        if t_ is None:
            continue
        if not isinstance(t_, torch.Tensor):
            raise TypeError(f"{what}: {name}: expected a tensor")
        if t_.device != inv.device:
            raise ValueError(f"{what}: {name} lives on {t_.device}, inv on {inv.device}")
    if inv.dim() < 1 or depth_values.dim() != 2 or depth_values.shape[0] != inv.shape[0] or depth_values.shape[1] < 2:
        raise ValueError(f"{what}: inv [B,...] and depth_values [B,n_range >= 2] expected, got {tuple(inv.shape)} and "
                         f"{tuple(depth_values.shape)}")
    if inv.numel() == 0:
        raise ValueError(f"{what}: empty map")
    for t_, name in ((g, "grad"), (out, "out")):
        if t_ is not None and t_.shape != inv.shape:
            raise ValueError(f"{what}: {name} {tuple(t_.shape)} must be shaped like inv {tuple(inv.shape)}")
    _t(inv, "inv"), _t(depth_values, "depth_values")
    if g is not None:
        _t(g, "grad")
    if out is not None:
        _t(out, "out")
    B = inv.shape[0]
    return B, inv.numel() // B, depth_values.shape[1]


def inv_to_depth_ranged(inv, depth_values, out=None):
    """``scale_inv_depth`` with a depth range per sample: inv [B,...] normalised inverse depths, depth_values [B,n_range] (first / last
    = the ends of sample b's range, read on the device) -> depths shaped like ``inv`` (written to ``out`` when given).  The bits of
    ``pointwise(PW_INV_TO_DEPTH, inv[b], s0=lo_b, s1=hi_b)`` per sample."""
    B, n, n_range = _ranged_args("inv_to_depth_ranged", inv, depth_values, out=out)
    out = torch.empty_like(inv) if out is None else out
    check(_lib.lib().effi_inv_to_depth_ranged_f32(_p(inv), _p(depth_values), n_range, B, n, _p(out), _stream()),
          "effi_inv_to_depth_ranged_f32")
    return out


def inv_to_depth_ranged_bwd(g, inv, depth_values, out=None):
    """Gradient of ``inv_to_depth_ranged`` w.r.t. ``inv`` given ``g`` = the gradient of its output (both shaped like ``inv``)."""
    B, n, n_range = _ranged_args("inv_to_depth_ranged_bwd", inv, depth_values, g=g, out=out)
    out = torch.empty_like(inv) if out is None else out
    check(_lib.lib().effi_inv_to_depth_ranged_bwd_f32(_p(g), _p(inv), _p(depth_values), n_range, B, n, _p(out), _stream()),
          "effi_inv_to_depth_ranged_bwd_f32")
    return out


def vol_lookup1d_bwd(gout, Dp, query, dmin, dmax, h, w):
    """Gradient of ``vol_lookup1d`` w.r.t. a planar [Dp,h,w] volume: gout [nq,h,w] -> [Dp,h,w]."""
    _t(gout, "grad")
    nq, qds, qys, qxs = _query_strides(query, h, w)
    dmin_t, dmax_t, rps = _ranges(dmin, dmax, h, w)
    gvol = torch.zeros(Dp, h, w, device=gout.device, dtype=torch.float32)
    check(_lib.lib().effi_vol_lookup1d_bwd_f32(_p(gvol), h * w, 1, Dp, _p(query), qds, qys, qxs, nq, _p(dmin_t), _p(dmax_t), rps, h, w,
                                               _p(gout), _stream()), "effi_vol_lookup1d_bwd_f32")
    return gvol


def getcost_bwd(gcost, x, disp_range, interval, Dcur, Dreg, dmin, dmax, nq, h, w, input_is_depth=False):
    """Gradient of ``getcost`` w.r.t. planar cur [Dcur,h,w] and reg [Dreg,h,w] volumes: gcost [2nq,h,w] -> (gcur, greg)."""
    _t(gcost, "grad"), _t(x, "inv_depth"), _t(interval, "interval")
    dmin_t, dmax_t, gps = _ranges(dmin, dmax, h, w)
    gcur = torch.zeros(Dcur, h, w, device=x.device, dtype=torch.float32)
    greg = torch.zeros(Dreg, h, w, device=x.device, dtype=torch.float32)
    n_range = 0 if disp_range is None else disp_range.numel()
    check(_lib.lib().effi_getcost_bwd_f32(_p(x), _p(disp_range), n_range, int(input_is_depth), _p(interval), _p(gcur), h * w, 1, Dcur,
                                          _p(greg), h * w, 1, Dreg, _p(dmin_t), _p(dmax_t), gps, nq, h, w, _p(gcost), _stream()),
          "effi_getcost_bwd_f32")
    return gcur, greg


def softargmin_bwd(logits, hyp, gdepth):
    D, h, w = logits.shape
    _t(logits, "logits"), _t(hyp, "hypotheses", contiguous=False), _t(gdepth, "grad")
    hyp, dds, dps, _ = _depth_strides(hyp, None, D, h, w)
    gl = torch.empty_like(logits)
    check(_lib.lib().effi_softargmin_bwd_f32(_p(logits), _p(hyp), dds, dps, D, h * w, _p(gdepth), _p(gl), _stream()), "effi_softargmin_bwd_f32")
    return gl


def view_aggregate_bwd(sim_views, weights, gout):
    S, D, h, w = sim_views.shape
    _t(sim_views, "sim_views"), _t(weights, "weights"), _t(gout, "grad")
    gsim, gw = torch.empty_like(sim_views), torch.empty_like(weights)
    check(_lib.lib().effi_view_aggregate_bwd_f32(_p(sim_views), _p(weights), S, D, h * w, _p(gout), _p(gsim), _p(gw), _stream()),
          "effi_view_aggregate_bwd_f32")
    return gsim, gw


def convex_upsample2x_bwd(inv_depth, mask, gup):
    _t(inv_depth, "inv_depth"), _t(mask, "mask"), _t(gup, "grad")
    h, w = inv_depth.shape[-2:]
    gmask = torch.empty_like(mask)
    ginv = torch.empty_like(inv_depth)
    scratch = torch.empty(9, h, w, device=inv_depth.device, dtype=torch.float32)       # per-pixel contributions, gathered in a fixed order
    check(_lib.lib().effi_convex_upsample2x_bwd_f32(_p(inv_depth), _p(mask), h, w, _p(gup), _p(gmask), _p(ginv), _p(scratch), _stream()),
          "effi_convex_upsample2x_bwd_f32")
    return gmask, ginv


def warpcorr_dyn_bwd(ref_nhwc, srcs_nhwc, rt, cur_depth, interval, view_w, D, sim, grad_sim):
    """Backward of ``warpcorr_dyn``: -> (grad_ref [h,w,C], [grad_src_v [h,w,C]], grad_view_w [S,vh,vw])."""
    h, w, Cc = ref_nhwc.shape
    S = len(srcs_nhwc)
    for t_ in (ref_nhwc, rt, cur_depth, interval, view_w, sim, grad_sim):
        _t(t_, "warpcorr_dyn_bwd operand")
    shift = _vw_shift(view_w, h, w)
    g_ref = torch.empty_like(ref_nhwc)
    g_src = [torch.zeros_like(s_) for s_ in srcs_nhwc]
    g_vw = torch.zeros(view_w.shape, device=view_w.device, dtype=torch.float64)      # 64-bit atomics: the sum cancels (see the kernel)
    check(_lib.lib().effi_warpcorr_dyn_bwd_f32(_p(ref_nhwc), _ptr_array(srcs_nhwc), S, _p(rt), _p(cur_depth), _p(interval), _p(view_w), shift,
                                               Cc, h, w, D, _p(sim), _p(grad_sim), _p(g_ref), _ptr_array(g_src), _p(g_vw), _stream()),
          "effi_warpcorr_dyn_bwd_f32")
    return g_ref, g_src, g_vw.float()
