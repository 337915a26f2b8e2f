"""Operator layer: torch.autograd.Functions whose forward AND backward are
hand-written HIP kernels reached through the C ABI (michigan_amd._cabi).

Tensor convention inside this module: activations are contiguous NHWC tensors
``[N, H, W, C]`` in the compute dtype (``torch.bfloat16`` or ``torch.float32``);
parameters stay fp32 in the reference's layouts and are re-packed per call into
the GEMM-order image the kernels want (``[taps][Cout][Cin]``) with ordinary
differentiable torch ops, so autograd carries weight gradients back through the
packing (and through spectral-norm's division) without any hand-written
un-packing.

Reference call sites replaced (all ATen today):
  conv2d            nn.Conv2d            normalization.py:94-99, architecture.py:31-35,
                                         discriminator.py:84-96, architecture.py:163-178
  spade_modulate    SPADE.forward        normalization.py:101-118
  batch_stats       F.batch_norm / sync  sync_batchnorm/batchnorm.py:63-68,128-145
  instance_norm_act InstanceNorm2d+lrelu normalization.py:47-48, discriminator.py:88-93
  upsample2x / avgpool3s2 / maxpool2 / blend   generator.py:74,186 discriminator.py:46-49
"""
from __future__ import annotations

import ctypes
import math
import os
import weakref
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _cabi as C

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = C.MG_ACT_NONE, C.MG_ACT_RELU, C.MG_ACT_LRELU, C.MG_ACT_TANH

# Use the gfx950 LDS transpose-read path for bf16 weight gradients (flags bit0 of mg_wgrad_desc).
WGRAD_USE_TR = True
# Process group used to synchronise batch-norm statistics (set by michigan_amd.parallel); None = local stats.
SYNC_BN_GROUP = None
# sync-BN all-reduces: async_op=True runs them on the process group's own stream (two cross-stream hops per collective, overlap with
# the neighbouring conv), False enqueues them on the current stream (torch >= 2.8: no hop).  A/B: MG_SYNCBN_ASYNC=1.
SYNC_BN_ASYNC = os.environ.get("MG_SYNCBN_ASYNC", "0") == "1"
# Weight / bias gradients of convolutions whose parameters live in an optim.FlatAdam arena bypass autograd: the wgrad kernel
# accumulates into the arena's persistent GEMM-order buffer and one batched launch per optimiser step drains it (optim.py).
GRAD_SINK = True          # (False: every weight gradient takes the autograd path -- what parameters outside a FlatAdam arena always do; tests)
# Deterministic weight gradients (MG_DETERMINISTIC=1 or ops.set_deterministic(True)): the wgrad kernels' split-K partial sums go to
# per-split slabs that a finishing launch adds in a fixed order instead of fp32 atomics (mg_wgrad_desc.det_ws); costs one pass over
# splits x |dW| per convolution.  Everything else on the path is deterministic already (two-stage reductions, fixed-order split-K forward).
WGRAD_DETERMINISTIC = os.environ.get("MG_DETERMINISTIC") == "1"


def set_deterministic(flag: bool = True) -> bool:
    """Bit-reproducible backward passes (see WGRAD_DETERMINISTIC); returns the previous setting."""
    global WGRAD_DETERMINISTIC
    prev, WGRAD_DETERMINISTIC = WGRAD_DETERMINISTIC, bool(flag)
    return prev


# bench.py --gpus N: a list here makes every sync-BN all-reduce record a pair of HIP events on the compute stream around itself
# ((kind, start, end) tuples), so that the first run on a real node shows what the ~42 latency-bound reductions of a step cost in-stream
# (vs MG_SYNCBN_ASYNC=1) without a profiler.  None = no events.
SYNC_BN_EVENTS = None


def _sync_bn_all_reduce(t: torch.Tensor, kind: str):
    import torch.distributed as dist
    ev = SYNC_BN_EVENTS if t.is_cuda else None
    if ev is not None:
        s = torch.cuda.Event(enable_timing=True)
        s.record()
    from . import parallel
    nat = parallel.native_comm() if t.is_cuda else None
    if nat is not None:
        nat.all_reduce_stats(t)                           # include/michigan_hip.h group (iv): RCCL on the current stream, no torch.distributed call
        work = None
    else:
        work = dist.all_reduce(t, group=SYNC_BN_GROUP, async_op=SYNC_BN_ASYNC)
    if ev is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ev.append((kind, s, e))
    _count_collective(kind)
    return work


STATS_FROM_UPSAMPLE_SOURCE = True     # batch statistics of a 2x-upsampled tensor from its quarter-size source (A/B: tools/ab_pyflag.py)


def _dtype_code(dtype) -> int:
    if dtype == torch.bfloat16:
        return C.MG_BF16
    if dtype == torch.float32:
        return C.MG_F32
    raise TypeError(f"michigan_amd kernels compute in bfloat16 or float32, got {dtype}")


def _dt(t: torch.Tensor) -> int:
    return _dtype_code(t.dtype)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor):
    """The hipStream_t the launch goes to: torch's CURRENT stream of the tensor's device.  torch._C._cuda_getCurrentRawStream returns the handle
    without building a torch.cuda.Stream object (~0.4 us instead of ~5 us; ~1100 launches per step, and the step is host-bound at one image per GPU)."""
    if t.is_cuda:
        if _RAW_STREAM is not None:
            return ctypes.c_void_p(_RAW_STREAM(t.device.index))
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return None


def _roundup(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 4:
        raise ValueError(f"expected an NHWC 4-d tensor, got shape {tuple(t.shape)}")
    return t.contiguous()


def _set_taps(desc, taps: Sequence[Tuple[int, int]]):
    if not 1 <= len(taps) <= C.MG_MAX_TAPS:
        raise ValueError(f"{len(taps)} taps (max {C.MG_MAX_TAPS})")
    desc.ntaps = len(taps)
    for i, (dy, dx) in enumerate(taps):
        desc.tap_dy[i] = dy
        desc.tap_dx[i] = dx


def fwd_taps(kh: int, kw: int, pad: int, dilation: int = 1) -> List[Tuple[int, int]]:
    return [(ky * dilation - pad, kx * dilation - pad) for ky in range(kh) for kx in range(kw)]


def gemm_weight(weight: torch.Tensor, cin_pad: int) -> torch.Tensor:
    """[Cout, Cin, kh, kw] -> GEMM order [kh*kw, Cout, cin_pad] (fp32, differentiable)."""
    cout, cin, kh, kw = weight.shape
    w = weight.permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
    if cin_pad > cin:
        w = F.pad(w, (0, cin_pad - cin))
    return w


def pad_channels(x: torch.Tensor, mult: int = 8) -> torch.Tensor:
    """Zero-pad the channel (last) dim of an NHWC tensor to a multiple of `mult` (differentiable)."""
    c = x.shape[-1]
    cp = _roundup(c, mult)
    return x if cp == c else F.pad(x, (0, cp - c))


# ----------------------------------------------------------------------------
# raw launches
# ----------------------------------------------------------------------------
def _launch_conv(inp, wt, out, bias, taps, *, Hj, Wj, isy, isx, osy=1, osx=1, ooy=0, oox=0,
                 cout, cout_gemm, act=ACT_NONE, slope=0.2, resid=None,
                 spade_x=None, mean=None, rstd=None, gamma_out=None, algo_cin=None, relu_mask=None, x_up=False, mask_slope=0.0):
    d = C.ConvDesc()
    d.in_, d.wt, d.out = inp.data_ptr(), wt.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.resid = resid.data_ptr() if resid is not None else None
    d.x = spade_x.data_ptr() if spade_x is not None else (relu_mask.data_ptr() if relu_mask is not None else None)
    d.mean = mean.data_ptr() if mean is not None else None
    d.rstd = rstd.data_ptr() if rstd is not None else None
    d.gamma_out = gamma_out.data_ptr() if gamma_out is not None else None
    d.dtype = _dt(inp)
    d.N, d.Hin, d.Win, d.Cin = inp.shape
    _, d.Hout, d.Wout, _ = out.shape
    d.Cout, d.Cout_gemm, d.CoutP = cout, cout_gemm, wt.shape[1]
    d.Hj, d.Wj, d.isy, d.isx = Hj, Wj, isy, isx
    d.osy, d.osx, d.ooy, d.oox = osy, osx, ooy, oox
    d.epilogue = C.MG_EPI_SPADE if spade_x is not None else C.MG_EPI_PLAIN
    d.act, d.slope = act, slope
    d.x_up = 1 if (x_up and spade_x is not None) else 0
    d.mask_slope = float(mask_slope) if relu_mask is not None else 0.0
    _set_taps(d, taps)
    assert wt.shape[0] == len(taps) and wt.shape[2] == inp.shape[3] and wt.dtype == inp.dtype
    C.backend().mg_conv_taps(d, _stream(inp))


def _arena_epoch(p) -> int:
    """Update count of the flat optimiser arena a parameter lives in (optim.FlatAdam tags its parameters with
    `_mg_arena`); 0 for parameters torch updates itself (their version counter moves instead)."""
    arena = getattr(p, "_mg_arena", None)
    return 0 if arena is None else arena.weight_epoch


def _param_state(params):
    """What a tensor derived from `params` is valid for: per parameter, its autograd version counter and its arena's update count."""
    return [(p._version, _arena_epoch(p)) for p in params]


class _ParamCache:
    """Derived tensors of parameters, each valid until one of its source parameters changes.  An entry is keyed by the parameters'
    addresses (+ whatever else the caller puts into the key) and stamped with _param_state; it holds the parameters by weak reference."""
    PRUNE_ABOVE = 4096

    def __init__(self):
        self._entries = {}                 # key -> [state, weak references of the parameters, value]

    def get(self, key, params):
        """The value stored for these very parameters in their current state, or None."""
        ent = self._entries.get(key)
        if ent is None:
            return None
        for ref, (version, epoch), p in zip(ent[1], ent[0], params):
            # identity through weak references: a freed parameter's address (and version 0) can be re-used by a new one
            if ref() is not p or p._version != version or _arena_epoch(p) != epoch:
                return None
        return ent[2]

    def only_epoch_moved(self, key, params) -> bool:
        """Is there an entry that is stale ONLY because an arena's update count moved (the optimiser stepped), not a tensor version?"""
        ent = self._entries.get(key)
        return ent is not None and all(ref() is p and p._version == version for ref, (version, _), p in zip(ent[1], ent[0], params))

    def put(self, key, params, value):
        if len(self._entries) > self.PRUNE_ABOVE:
            self.prune()
        self._entries[key] = [_param_state(params), tuple(weakref.ref(p) for p in params), value]

    def restamp(self, key):
        """The value of this entry was refreshed in place: it is valid for its parameters' current state."""
        ent = self._entries[key]
        ent[0] = _param_state([ref() for ref in ent[1]])

    def live(self, arena):
        """(key, parameters, value) of every entry whose parameters are alive and whose first one lives in `arena`."""
        for key, (_, refs, value) in list(self._entries.items()):
            params = [ref() for ref in refs]
            if all(p is not None for p in params) and getattr(params[0], "_mg_arena", None) is arena:
                yield key, params, value

    def prune(self):
        """Drop the entries of parameters that no longer exist."""
        for key in [k for k, ent in self._entries.items() if any(ref() is None for ref in ent[1])]:
            del self._entries[key]


_PACK_CACHE = _ParamCache()           # pack_weight: (addresses, dtype, rows_p, cols_p, mode) -> GEMM image
_BIAS_PAIR_CACHE = _ParamCache()      # spade_bias_rows: (address of mlp_gamma.bias, of mlp_beta.bias) -> interleaved rows


def pack_weight(w0: torch.Tensor, w1: Optional[torch.Tensor], dtype, rows_p: int, cols_p: int, mode: int) -> torch.Tensor:
    """Reference-layout fp32 weight(s) [Cout, Cin, kh, kw] -> GEMM image [taps, rows_p, cols_p] in `dtype`
    (one HIP launch: permute + zero-pad + cast; two tensors = fused SPADE gamma/beta row interleave).
    mode 0: rows = output channels (forward / wgrad image); mode 1: rows = input channels (dgrad image).

    Packed images of registered nn.Parameters are cached until the weights change: the key carries the tensors'
    autograd version counters (bumped by every in-place torch op: init, load_state_dict, torch.optim) AND the global
    update count of the flat arena they live in, which FlatAdam.step advances because its raw-pointer HIP kernel
    updates the arena without touching the version counters.  So the discriminator (run in the G step and again, unchanged, in the D step), the VGG tower
    (three passes per step) and the in-painting net are packed once per weight state instead of once per launch.
    Tensors that are not parameters (per-forward spectral-norm products W / sigma) are never cached."""
    pre = getattr(w0, "_mg_packed", None)               # images the batched spectral-norm path produced for this very tensor
    if pre is not None:
        hit = pre.get((dtype, rows_p, cols_p, mode))
        if hit is not None:
            return hit
    origin = getattr(w0, "_mg_sn_origin", None)
    if origin is not None:                              # remember what the consumer of a spectral-normed weight asks for:
        geoms = getattr(origin, "_mg_pack_geom", None)  # the batched path (networks/spectral.py) prepares exactly these images
        if geoms is None:
            geoms = origin._mg_pack_geom = set()
        geoms.add((dtype, rows_p, cols_p, mode))
    key = None
    if isinstance(w0, torch.nn.Parameter) and (w1 is None or isinstance(w1, torch.nn.Parameter)):
        params = (w0,) if w1 is None else (w0, w1)
        key = (w0.data_ptr(), 0 if w1 is None else w1.data_ptr(), dtype, rows_p, cols_p, mode)
        hit = _PACK_CACHE.get(key, params)
        arena = getattr(w0, "_mg_arena", None)
        if (hit is None and BATCHED_PACK and arena is not None and (w1 is None or getattr(w1, "_mg_arena", None) is arena)
                and _PACK_CACHE.only_epoch_moved(key, params)):
            _repack_arena(arena)                        # the optimiser stepped: refresh every image of this arena in ONE launch
            hit = _PACK_CACHE.get(key, params)
        if hit is not None:
            return hit
    dst = _pack_weight(w0, w1, dtype, rows_p, cols_p, mode)
    if key is not None:
        _PACK_CACHE.put(key, params, dst)               # one image per slot: a stale one is replaced
        if arena is not None:
            drop_arena_pack_table(arena)                # the arena's job table has to learn about this slot
    return dst


BATCHED_PACK = True          # refresh all packed images of an optimiser arena with one mg_pack_weights launch (False: per-layer mg_pack_weight, as for parameters outside an arena; tests)
_ARENA_PACK_TABLES = weakref.WeakKeyDictionary()     # arena -> (weak references of the parameters, cache keys, job table, block map (device), nblocks, table address)


class DeviceTable:
    """A ctypes struct array that lives in pinned host memory and is mirrored to the device with one async copy."""

    def __init__(self, struct, n: int, device):
        self.n, self.struct = n, struct
        nbytes = ctypes.sizeof(struct) * n
        cuda = torch.device(device).type == "cuda"
        self.host = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=cuda)
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device) if cuda else self.host
        self.rows = (struct * n).from_address(self.host.data_ptr())
        self._event = None

    def begin_update(self):
        if self._event is not None:
            self._event.synchronize()                   # the previous upload (enqueued a forward pass ago) has finished
        return self.rows

    def upload(self):
        if self.dev is not self.host:
            self.dev.copy_(self.host, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()
        return ctypes.c_void_p(self.dev.data_ptr())


def block_map(counts, device) -> torch.Tensor:
    """int32 map workgroup -> table row for the batched kernels (row i owns counts[i] consecutive workgroups)."""
    m = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts, dtype=torch.int64))
    return m.to(device)


def _repack_arena(arena):
    """Re-pack every cached GEMM image whose source parameters live in `arena` with one batched launch (in place: the
    images keep their addresses) and stamp them with the parameters' current state.  The table holds only weak references
    to the parameters (they reference the arena, which must be able to die)."""
    ent = _ARENA_PACK_TABLES.get(arena)
    if ent is not None and any(ref() is None for ref in ent[0]):
        ent = None
    if ent is None:
        jobs = [job for job in _PACK_CACHE.live(arena) if job[1][0].shape[2] * job[1][0].shape[3] <= 49]
        if not jobs:
            return
        be = C.backend()
        dev = jobs[0][2].device
        counts = []
        table = DeviceTable(C.PackJob, len(jobs), dev)
        first = 0
        for row, (key, params, dst) in zip(table.begin_update(), jobs):
            w0, w1 = params[0], (params[1] if len(params) > 1 else None)
            _, _, dtype, rows_p, cols_p, mode = key
            taps = w0.shape[2] * w0.shape[3]
            nb = int(be.mg_pack_job_blocks(mode, w0.shape[0], w0.shape[1], taps, rows_p, cols_p))
            row.w0, row.w1, row.dst, row.sigma = w0.data_ptr(), (w1.data_ptr() if w1 is not None else None), dst.data_ptr(), None
            row.dtype = _dtype_code(dtype)
            row.cout, row.cin, row.taps = w0.shape[0], w0.shape[1], taps
            row.rows_p, row.cols_p, row.mode, row.first_block = rows_p, cols_p, mode, first
            counts.append(nb)
            first += nb
        refs = [weakref.ref(p) for _, params, _ in jobs for p in params]
        ent = _ARENA_PACK_TABLES[arena] = (refs, [key for key, _, _ in jobs], table, block_map(counts, dev), first, table.upload())
    _, keys, table, bmap, nblocks, tab_ptr = ent
    C.backend().mg_pack_weights(tab_ptr, len(keys), _p(bmap), nblocks, _stream(bmap))
    for key in keys:
        _PACK_CACHE.restamp(key)


def drop_arena_pack_table(arena):
    """Forget the batched re-pack's job table of `arena`: the set of cached images changed, or the parameters' storage moved."""
    _ARENA_PACK_TABLES.pop(arena, None)


def _pack_weight(w0, w1, dtype, rows_p, cols_p, mode):
    w0, w1 = _f32_dense(w0), _f32_dense(w1)
    cout, cin, kh, kw = w0.shape
    dst = torch.empty((kh * kw, rows_p, cols_p), dtype=dtype, device=w0.device)
    C.backend().mg_pack_weight(_p(w0), _p(w1), _p(dst), _dtype_code(dtype),
                               cout, cin, kh * kw, rows_p, cols_p, mode, _stream(w0))
    return dst


def unpack_wgrad(dw: torch.Tensor, shape, two: bool = False):
    """fp32 dW in GEMM order [taps, rows, cols] -> reference layout [Cout, Cin, kh, kw] (x2 for gamma/beta)."""
    cout, cin, kh, kw = shape
    d0 = torch.empty(shape, dtype=torch.float32, device=dw.device)
    d1 = torch.empty(shape, dtype=torch.float32, device=dw.device) if two else None
    C.backend().mg_unpack_wgrad(_p(dw), _p(d0), _p(d1), cout, cin, kh * kw, dw.shape[1], dw.shape[2], _stream(dw))
    return (d0, d1) if two else d0


FUSE_RELU_MASK = True   # fold a consumed ReLU's backward mask into the data-gradient epilogue (A/B switch)
FUSE_LRELU_MASK = os.environ.get("MG_FUSE_LRELU_MASK", "1") != "0"    # ... and a single-consumer LeakyReLU's (SPADE outputs inside a residual block)
# The LeakyReLU mask is not idempotent, so its hand-off is checked on the host by default (one set lookup per SPADE backward): a producer
# whose consumer committed to the fold at forward time raises if the gradient it receives is not the very buffer that consumer masked
# (a hook cloned it, autograd summed it with another gradient, ...), instead of masking twice in silence.  ADVICE r3.
MASK_PROTOCOL_CHECK = os.environ.get("MG_MASK_PROTOCOL_CHECK", "1") != "0"


def mark_single_consumer_lrelu(t: torch.Tensor, slope: float = 0.2) -> torch.Tensor:
    """`t` is the output of a fused LeakyReLU(slope) and goes into EXACTLY ONE conv2d: that conv's data gradient may apply the
    activation's backward mask in its epilogue (mg_conv_desc.mask_slope) and the producer then skips it (no read of `t` in its
    backward passes).  Do not mark tensors with a second consumer: the gradients would be summed after one of them was masked."""
    t._mg_lrelu_out = float(slope)
    return t


def _grad_premasked(dh: torch.Tensor, h: torch.Tensor, act: int) -> bool:
    """True when `dh` (the gradient of the activation output `h`) was already multiplied by the activation's derivative by the
    consumer's data-gradient epilogue (the record conv_dgrad left for exactly this buffer).

    Two records, both keyed by addresses of buffers that are ALIVE between the two events they connect:
      _FOLD_EXPECTED  address of h, added by the consuming conv2d at FORWARD time when it commits to folding h's LeakyReLU mask (h is saved by
                      its producer until the producer's backward): tells the producer that an un-masked gradient would be an error;
      _RELU_MASKED    address of the masked gradient -> (address of h, the gradient's version), left by conv_dgrad and popped here within
                      the same backward pass (the gradient is referenced by the autograd engine in between).
    reset_mask_protocol() (every optimiser zero_grad / trainer step) drops whatever an interrupted backward left behind."""
    if act not in (ACT_RELU, ACT_LRELU):
        return False
    hit = _take_mask_record(dh, h)
    if act == ACT_LRELU and h.data_ptr() in _FOLD_EXPECTED:
        _FOLD_EXPECTED.pop(h.data_ptr(), None)
        if MASK_PROTOCOL_CHECK and not hit and FUSE_LRELU_MASK and FUSE_RELU_MASK:
            raise RuntimeError("mask protocol: the consumer of a single-consumer LeakyReLU output folded the activation's backward mask into its "
                               "data gradient, but the gradient that reached the producer is not that buffer (cloned by a hook, accumulated with "
                               "another gradient, made contiguous by a copy): masking again would scale negative-side gradients by slope^2.  "
                               "Set MG_FUSE_LRELU_MASK=0 when gradients of SPADE outputs are intercepted.")
    return hit


def expire_fold_expectations():
    """A new generator forward in grad mode starts a new graph: expectations a previous forward left without ever running its backward
    (validation / visualisation passes outside no_grad, under an optimiser that never calls reset_mask_protocol: the drop-in's
    torch.optim.Adam) must not meet a recycled address later.  Only the error CHECK is keyed on them; the hand-off itself
    (_RELU_MASKED) is untouched.  Expectations whose GRAPH is still alive stay: each carries a weak reference to the autograd node that produced
    h (a custom Function's context, kept alive by the graph and by nothing else), so a second grad-mode generator pass inside one graph does
    not switch the check off for the first pass; entries without such a node are dropped as before."""
    for addr in [a for a, ref in _FOLD_EXPECTED.items() if ref is None or ref() is None]:
        del _FOLD_EXPECTED[addr]


def _weak_node(t):
    try:
        return weakref.ref(t.grad_fn) if t.grad_fn is not None else None
    except TypeError:                                      # a node type without weak-reference support: the entry expires at the next forward
        return None


def reset_mask_protocol():
    """Forget every pending mask hand-off (records of a backward pass that was interrupted, forward passes that never got a backward)."""
    _RELU_MASKED.clear()
    _FOLD_EXPECTED.clear()


_RELU_MASKED = {}       # address of a ReLU-masked data gradient -> (address of the ReLU output it was masked with, version)
_FOLD_EXPECTED = {}     # address of a LeakyReLU output whose (single) consumer committed to the mask fold at forward time -> weakref of its producer node
_DGRAD_CLASSES = {}     # (kh, kw, stride, pad) -> [(py, px, taps, (lo, hi))], tap order of the class-sorted weight image
_DGRAD_PERM = {}        # (kh, kw, stride, pad, device) -> index tensor that sorts the packed taps by parity class


def _leave_mask_record(g: torch.Tensor, y: torch.Tensor):
    """The gradient buffer `g` already carries the backward mask of the activation output `y`."""
    # g is already multiplied by the ReLU mask of the tensor the forward conv consumed (conv_dgrad's epilogue, the max-pool backward,
    # _ActTapFn); the producer of that tensor finds the record below and skips its activation-backward pass.  The record is keyed
    # by g's address and carries its version counter: a gradient that autograd summed out of place lives elsewhere, one it
    # accumulated in place has a bumped version -- in both cases the producer masks again (harmless: idempotent
    # for ReLU), so a skip can only happen for the very buffer that launch wrote.
    # mask_slope > 0 (LeakyReLU): masking twice is NOT harmless, so only tensors whose producer declared the conv their
    # single consumer are folded (mark_single_consumer_lrelu) -- then the buffer reaches the producer untouched and the
    # record is always found (MG_MASK_PROTOCOL_CHECK=1 makes the producer raise if it is not).
    _RELU_MASKED[g.data_ptr()] = (y.data_ptr(), g._version)


def _take_mask_record(g: torch.Tensor, y: torch.Tensor) -> bool:
    """Remove whatever record there is for the buffer `g`; True when it says that `g`, as it is now, carries the mask of `y`."""
    return _RELU_MASKED.pop(g.data_ptr(), None) == (y.data_ptr(), g._version)


def _dgrad_classes(kh: int, kw: int, stride: int, pad: int):
    key = (kh, kw, stride, pad)
    if key not in _DGRAD_CLASSES:
        classes, order = [], []
        for py in range(stride):
            for px in range(stride):
                taps, lo = [], len(order)
                for ky in range(kh):
                    if (py + pad - ky) % stride:
                        continue
                    for kx in range(kw):
                        if (px + pad - kx) % stride:
                            continue
                        taps.append(((py + pad - ky) // stride, (px + pad - kx) // stride))
                        order.append(ky * kw + kx)
                classes.append((py, px, taps, (lo, len(order))))
        _DGRAD_CLASSES[key] = (classes, order)
    return _DGRAD_CLASSES[key]


def conv_dgrad(dy: torch.Tensor, wt: torch.Tensor, kh: int, kw: int, stride: int, pad: int,
               in_hw: Tuple[int, int], cin: int, relu_mask: Optional[torch.Tensor] = None, mask_slope: float = 0.0) -> torch.Tensor:
    """Data gradient of a forward conv.  dy is [N, Ho, Wo, Cg8]; wt is the dgrad image
    [taps, roundup(cin,128), Cg8] (pack_weight mode 1).  For stride s the output pixels split into s*s
    parity classes; each class is a stride-1 gather over dy with the subset of taps whose offset is
    divisible by s (no wasted MACs).  The weight image is re-ordered once per call so that every class
    reads a contiguous slice (one gather with a cached device index; a Python index list or per-class
    copies would cost a blocking upload / a launch per class)."""
    n, ho, wo, cg8 = dy.shape
    t = kh * kw
    h, w = in_hw
    assert wt.shape[0] == t and wt.shape[2] == cg8
    classes, order = _dgrad_classes(kh, kw, stride, pad)
    # the s*s parity classes partition the input pixels; only a class without taps (kernel smaller than the stride) leaves holes
    full = all(taps for _, _, taps, _ in classes)
    dx = (torch.empty if full else torch.zeros)((n, h, w, cin), dtype=dy.dtype, device=dy.device)
    if stride > 1:
        pkey = (kh, kw, stride, pad, wt.device)
        if pkey not in _DGRAD_PERM:
            _DGRAD_PERM[pkey] = torch.tensor(order, dtype=torch.long, device=wt.device)
        wt = wt.index_select(0, _DGRAD_PERM[pkey])
    for py, px, taps, (lo, hi) in classes:
        hj, wj = len(range(py, h, stride)), len(range(px, w, stride))
        if hj == 0 or wj == 0 or not taps:
            continue
        _launch_conv(dy, wt[lo:hi], dx, None, taps, Hj=hj, Wj=wj, isy=1, isx=1,
                     osy=stride, osx=stride, ooy=py, oox=px, cout=cin, cout_gemm=cin, relu_mask=relu_mask, mask_slope=mask_slope)
    if relu_mask is not None:
        assert relu_mask.shape == dx.shape and relu_mask.dtype == dx.dtype
        _leave_mask_record(dx, relu_mask)
    return dx


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, kh: int, kw: int, stride: int, pad: int, want_bias: bool = False, out=None, beside: bool = False):
    """dW in GEMM order [T, Cg8, Cin] (fp32) of a forward conv; split-K over pixels, fp32 atomics.
    want_bias=True also returns the bias gradient [Cg8] (column sums of dy) from the same launch.
    out = (dw, dbias): accumulate into these existing buffers (the optimiser's GEMM-order arena) instead;
    beside (with out): the launch runs beside another stream's work, the 3x3 kernel keeps to one workgroup per CU (mg_wgrad_desc.flags bit 1)."""
    n, h, w, cin = x.shape
    _, hj, wj, cg8 = dy.shape
    if out is not None:
        return _wgrad_launch(x, dy, fwd_taps(kh, kw, pad), stride, want_bias, out, beside)
    if _wgrad_swapped(stride, cg8, cin):
        # Few output channels (conv_img, the discriminators' 1-channel heads): a 128-row tile would be 94 % padding.
        # dW[t][co][ci] = sum_q x[q][ci] * dy[q + (pad - k_t)][co] is the weight gradient of the mirrored problem with
        # the roles of x and dy swapped, whose tiny "Cin" takes the packed-taps path; transpose the small result.
        swapped = _wgrad_launch(dy, x, [(pad - ky, pad - kx) for ky in range(kh) for kx in range(kw)], 1, False)
        dw = swapped.transpose(1, 2).contiguous()
        return (dw, channel_sums(dy)[0, 0].float()) if want_bias else dw
    return _wgrad_launch(x, dy, fwd_taps(kh, kw, pad), stride, want_bias)


# ---- weight gradients on a side HIP stream ------------------------------------------------------------------------------------
# A weight gradient is a LEAF of the backward pass: nothing reads it before the optimiser's gradient drain.  The data-gradient chain it
# hangs off alternates MFMA-bound convolutions with HBM-bound passes (SPADE's reduce / apply, activation and pooling adjoints: ~7 ms of
# a 65 ms step) during which the matrix pipes idle, and every launch of the chain ends in a tail of half-empty CUs.  The gradient
# sink's wgrad launches therefore go to a second stream: ordered behind the producer of dy by an event, joined by the
# main stream before anything reads or re-zeroes the GEMM-order arena (FlatAdam.drain_grads / sync_grads / zero_grad), their operands
# kept referenced until their launch has finished (sink_wgrad).  Same kernels, same atomics: results are those of the in-stream order up to atomic order.
# Measured (round 5, bs 8 / 512^2 / bf16, A B A B in one process, profiles/r05_side_stream_ab.txt): 65.6 -> 63.3 ms per step, 38.7 -> 37.4
# at bs 4, 67.1 -> 65.5 with one rank and every collective forced over RCCL; the kernel trace (profiles/r05_stream_overlap.txt) has two
# queues busy 29 % of the time.  On the side stream the kernel-row 3x3 kernel keeps to ONE workgroup per CU (mg_wgrad_desc.flags bit 1:
# -0.6 / -0.55 / 0.0 ms on three boxes; the generic kernel capped the same way: +1.6 ms, not done).  What did NOT pay, same A/Bs: a
# lowest-priority side stream (same on one GPU, +16 ms per step beside RCCL collectives), SPADE's whole conditioning branch over there
# (65.0: the critical path then waits for side-stream work it used to run itself), its forward half prefetched at the top of the generator
# pass (+0.4 ms), the background encoder beside head_0 / G_middle_* (flat).  MG_WGRAD_STREAM=0 restores the single stream.
WGRAD_SIDE_STREAM = os.environ.get("MG_WGRAD_STREAM", "1") != "0"
WGRAD_HALF_CU = os.environ.get("MG_WGRAD_HALF_CU", "1") != "0"     # side-stream wgrad3x3 launches keep to one workgroup per CU (flags bit 1): -0.6 / -0.55 / 0.0 ms on three boxes
_WGRAD_STREAMS = {}            # device index -> _SideStream
# The held operands outlive their autograd nodes while the side queue lags (the case the stream is for): their bytes are BOUNDED -- past the
# budget the main stream waits for the oldest launches' events and lets go of them.  At bs 8 / 512^2 the whole backward holds
# < 3 GB this way (bench.py reports torch's peak for both settings of MG_WGRAD_STREAM under `extra.peak_memory_gb`).
WGRAD_HELD_BUDGET = int(os.environ.get("MG_WGRAD_HELD_MB", "6144")) << 20


def streams_overlap(main, cand) -> bool:
    """Do kernels on `cand` really run beside kernels on `main`?  HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by
    default) in creation order; two streams that land on one queue serialise, whatever the API says.  Probe: a ~0.4 ms element-wise pass on `main`,
    a tiny kernel on `cand` issued right behind it with no dependency; `cand` overlaps when its kernel finishes before main's does."""
    dev = main.device
    big = torch.empty(64 << 20, dtype=torch.float32, device=dev)            # 256 MiB: ~0.1 ms per pass at 5 TB/s
    small = torch.zeros(64, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    votes = 0
    for _ in range(3):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        with torch.cuda.stream(main):
            e0.record(main)
            for _ in range(4):
                big.add_(1.0)
            e1.record(main)
        with torch.cuda.stream(cand):
            small.add_(1.0)
            e2.record(cand)
        torch.cuda.synchronize(dev)
        votes += int(e0.elapsed_time(e2) < 0.6 * e0.elapsed_time(e1))
    return votes >= 2


STREAM_PROBE = os.environ.get("MG_STREAM_PROBE", "1") != "0"      # pick a second stream that is on another hardware queue than the compute stream
_STREAM_PROBE_LOG = []                                             # (device index, attempts, overlaps) of every side stream created: bench.py reports it


def _new_side_stream(device):
    """The side stream is an ordinary stream at torch's default priority.  One created at the device's LOWEST priority
    (hipStreamCreateWithPriority) measured the same single-GPU gain (65.1 -> 63.6 vs 64.6 -> 63.3 ms) but cost 16 ms per step as soon as the
    step contained RCCL collectives (one rank, every collective forced: 83.5 ms against 65.6 with this stream and 67.1 with no side stream
    at all, whichever stream the collectives were issued on: profiles/r05_side_stream_ab.txt) -- removed.
    Round 6: WHICH hardware queue a stream lands on is decided by creation order, and an RCCL communicator created in between shifts it: with
    the C ABI's communicator in the process the step ran 70.7 ms instead of 63.5 without a single collective being issued, 63.2 again under
    GPU_MAX_HW_QUEUES=8 -- and torch's own communicator showed the mirror image (83.9 ms under GPU_MAX_HW_QUEUES=8; profiles/r06_hw_queues.txt).
    So the stream is PROBED: candidates are created until one measurably overlaps the compute stream (the rejected ones stay alive -- they hold
    their queue slot); the outcome is kept for bench.py's line."""
    main = torch.cuda.current_stream(device)
    if not STREAM_PROBE:
        return torch.cuda.Stream(device=device)
    rejected = []
    for attempt in range(1, 9):
        cand = torch.cuda.Stream(device=device)
        if streams_overlap(main, cand):
            _STREAM_PROBE_LOG.append((device.index, attempt, True))
            _REJECTED_STREAMS.extend(rejected)
            return cand
        rejected.append(cand)
    _STREAM_PROBE_LOG.append((device.index, 8, False))
    _REJECTED_STREAMS.extend(rejected[1:])
    return rejected[0]


_REJECTED_STREAMS = []


class _SideStream:
    """The second stream of one device and the weight-gradient launches that may still be running on it."""

    def __init__(self, device):
        self.stream = _new_side_stream(device)
        self.dirty = False             # launches were issued to the stream since the current stream last joined it
        self.held = []                 # [(event, x, dy, bytes)], oldest first

    def hold(self, event, x, dy):
        """Keep the operands of the launch that `event` ends referenced until it has finished, within WGRAD_HELD_BUDGET."""
        # The operands stay REFERENCED until their launch has finished (or the main stream has joined).  That keeps their memory from
        # being reused -- and it keeps autograd from accumulating into dy IN PLACE: a conv's dy is also the gradient of its residual
        # input (returned as such by _ConvFn.backward), and the engine's input buffer adds the next incoming gradient into a tensor it
        # holds the only reference to.  In stream order that write came after the wgrad's reads; beside a side stream it raced them
        # (round 5: G_middle_1.conv_1's weight gradient at cosine 0.78 in tests/test_gpu_fullsize.py before this list existed).
        held = self.held
        while held and held[0][0].query():
            held.pop(0)
        held.append((event, x, dy, x.numel() * x.element_size() + dy.numel() * dy.element_size()))
        over = sum(h[3] for h in held) - WGRAD_HELD_BUDGET
        while over > 0 and len(held) > 1:                              # the main stream falls in behind the oldest launches: their operands are free again
            old = held.pop(0)
            torch.cuda.current_stream(x.device).wait_event(old[0])
            over -= old[3]

    def join(self):
        """The current stream waits for everything issued to the side stream so far; nothing has to be held any longer."""
        torch.cuda.current_stream(self.stream.device).wait_stream(self.stream)
        self.dirty = False
        self.held.clear()


def _wgrad_side(device) -> _SideStream:
    ent = _WGRAD_STREAMS.get(device.index)
    if ent is None:
        ent = _WGRAD_STREAMS[device.index] = _SideStream(device)
    return ent


def wgrad_join(device=None):
    """The current stream waits for every weight-gradient launch issued to the side stream so far (no-op when none was).  Behind the
    join the operands may be freed or rewritten by the current stream again: the references held for them are dropped."""
    for idx, ent in _WGRAD_STREAMS.items():
        if ent.dirty and (device is None or device.index == idx):
            ent.join()


def sink_wgrad(arena, slot, x, dy, kh, kw, stride, pad, need_b):
    """Weight gradient of one convolution into its slot of the optimiser's GEMM-order arena (+ the bucket bookkeeping)."""
    if WGRAD_SIDE_STREAM and x.is_cuda:
        ent = _wgrad_side(x.device)
        side = ent.stream
        side.wait_stream(torch.cuda.current_stream(x.device))          # dy (and x) were produced on the current stream
        with torch.cuda.stream(side):
            conv_wgrad(x, dy, kh, kw, stride, pad, want_bias=need_b, out=(slot[1], slot[2]), beside=WGRAD_HALF_CU)
            arena.slot_written(slot[0])                                # a bucket all-reduce it triggers is ordered behind the side stream
            ev = torch.cuda.Event()
            ev.record(side)
        ent.dirty = True
        ent.hold(ev, x, dy)
        return
    conv_wgrad(x, dy, kh, kw, stride, pad, want_bias=need_b, out=(slot[1], slot[2]))
    arena.slot_written(slot[0])


# Generator step (model.Pix2PixModel.compute_generator_loss): the losses' branches on two streams.  1 = the discriminator branch (D on fake / real,
# GAN + feature-matching losses: small 4x4-conv launches) on the side stream beside the VGG / orientation branch; autograd runs each node's backward
# on its forward's stream, so the two backward branches overlap as well.  2 (default) = also the real image's VGG features (no graph, input-only)
# on the side stream beside the generator pass.  Measured A B C C B A x 3 in one process (profiles/r05_side_stream_ab.txt): 64.51 / 63.96 / 63.22
# ms per step for 0 / 1 / 2; a second box 62.86 / 63.09 / 61.92; parity suite green in mode 2.  Needs WGRAD_SIDE_STREAM (MG_WGRAD_STREAM=0 turns
# every second-stream use off).
BRANCH_STREAMS = int(os.environ.get("MG_BRANCH_STREAMS", "2"))


def side_stream(device):
    """The second stream of the step (shared with the weight gradients)."""
    return _wgrad_side(device).stream


def _wgrad_swapped(stride: int, cg8: int, cin: int) -> bool:
    return stride == 1 and cg8 <= 8 and cin >= 32


def _wgrad_launch(x, dy, taps, stride, want_bias, out=None, beside=False):
    n, h, w, cin = x.shape
    _, hj, wj, cg8 = dy.shape
    ndw = len(taps) * cg8 * cin
    if out is not None:
        dw, dbias = out
        assert dw.shape == (len(taps), cg8, cin) and (dbias is not None or not want_bias)
        dbias = dbias if want_bias else None
    else:
        buf = torch.zeros(ndw + (cg8 if want_bias else 0), dtype=torch.float32, device=x.device)    # one fill for both atomic targets
        dw = buf[:ndw].view(len(taps), cg8, cin)
        dbias = buf[ndw:] if want_bias else None
    d = C.WgradDesc()
    d.x, d.dy, d.dw = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
    d.dbias = dbias.data_ptr() if want_bias else None
    d.dtype = _dt(x)
    d.N, d.Hin, d.Win, d.Cin = n, h, w, cin
    d.Hj, d.Wj, d.Cg = hj, wj, cg8
    d.isy = d.isx = stride
    d.splitk = 0
    d.flags = (1 if (WGRAD_USE_TR and x.dtype == torch.bfloat16) else 0) | (2 if beside else 0)
    _set_taps(d, taps)
    assert dy.dtype == x.dtype
    if WGRAD_DETERMINISTIC:
        # split-K partials into per-split slabs + an ordered sum instead of fp32 atomics: bit-reproducible weight gradients
        nbytes = int(C.backend().mg_wgrad_det_workspace(ctypes.byref(d)))
        if nbytes < 0:
            raise RuntimeError("mg_wgrad_det_workspace failed")
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
        d.det_ws, d.det_ws_bytes = ws.data_ptr(), nbytes
    C.backend().mg_conv_wgrad(d, _stream(x))
    return (dw, dbias) if want_bias else dw


def _stats_workspace(groups: int, p: int, c: int, device) -> torch.Tensor:
    """The stage-1 partial sums of a [G, P, C] column reduction (mg_stats_workspace bytes, never an empty tensor)."""
    return torch.empty(max(int(C.backend().mg_stats_workspace(groups, p, c)), 4), dtype=torch.uint8, device=device)


def channel_sums(x: torch.Tensor, groups: int = 1, shift: bool = False) -> torch.Tensor:
    """x viewed as [G, P, C] -> fp64 [G, 2, C] (sum, sum of squares); deterministic two-stage reduce (fp32 partial sums per chunk,
    fp64 across chunks: mg_norm.hip).  `shift`: accumulate x - x[g, 0, c] and un-shift in fp64 -- for STATISTICS (the variance must
    not cancel against mean^2 in fp32); off for gradient column sums, whose mean is ~0 (a sample pivot would only add error)."""
    c = x.shape[-1]
    p = x.numel() // (groups * c)
    be = C.backend()
    ws = _stats_workspace(groups, p, c, x.device)
    sums = torch.empty((groups, 2, c), dtype=torch.float64, device=x.device)
    be.mg_channel_stats(_p(x), _dt(x), groups, p, c, int(shift), _p(sums), _p(ws), _stream(x))
    return sums


def act_backward(dy: torch.Tensor, y: torch.Tensor, act: int, slope: float) -> torch.Tensor:
    if act == ACT_NONE:
        return dy
    dpre = torch.empty_like(dy)
    numel = dy.numel()
    if numel % 4:
        raise ValueError("act_backward needs numel % 4 == 0")
    C.backend().mg_act_bwd(_p(dy), _p(y), _p(dpre), _dt(dy), numel, act, slope, _stream(dy))
    return dpre


# ----------------------------------------------------------------------------
# conv2d
# ----------------------------------------------------------------------------
def _conv_forward(who, x, weight, bias, resid, stride, pad, dilation, act, slope, **launch):
    """The forward launch of `who` (conv2d / conv2d_infer, for the error text) on a dense NHWC `x` whose channels cover the weight's:
    output geometry, packed weight, fp32 bias, output, residual check.  `launch`: what only one of them passes to _launch_conv."""
    n, h, w, cx = x.shape
    cout, cin, kh, kw = weight.shape
    ho = (h + 2 * pad - dilation * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dilation * (kw - 1) - 1) // stride + 1
    wp = pack_weight(weight, None, x.dtype, _roundup(cout, 128), cx, 0)
    bp = _f32_dense(bias)
    out = torch.empty((n, ho, wo, cout), dtype=x.dtype, device=x.device)
    if resid is not None:
        resid = _nhwc(resid)
        if resid.shape != out.shape or resid.dtype != out.dtype:
            raise ValueError(f"{who}: residual must match the output")
    _launch_conv(x, wp, out, bp, fwd_taps(kh, kw, pad, dilation), Hj=ho, Wj=wo, isy=stride, isx=stride,
                 cout=cout, cout_gemm=cout, act=act, slope=slope, resid=resid, **launch)
    return out


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, resid, stride, pad, act, slope, x_relu=False, sink=None, x_mask_slope=0.0):
        ctx.sink = sink
        ctx.x_mask_slope = float(x_mask_slope)
        x = _nhwc(x)
        cx, cin = x.shape[3], weight.shape[1]
        if cx < cin or cx % 8:
            raise ValueError(f"conv2d: input has {cx} channels, weight expects {cin} (input must be >= and a multiple of 8)")
        out = _conv_forward("conv2d", x, weight, bias, resid, stride, pad, 1, act, slope, algo_cin=cin)
        ctx.save_for_backward(x, weight, out if act != ACT_NONE else None)
        ctx.cfg = (stride, pad, act, slope, bias is not None, resid is not None)
        ctx.x_relu = bool(x_relu)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, out = ctx.saved_tensors
        stride, pad, act, slope, has_bias, has_resid = ctx.cfg
        cout, cin, kh, kw = weight.shape
        cx = x.shape[3]
        dout = dout.contiguous()
        if act == ACT_RELU and _take_mask_record(dout, out):
            dpre = dout                                  # the consumer's dgrad epilogue already applied this ReLU's mask
        else:
            dpre = act_backward(dout, out, act, slope)
        dpre8 = pad_channels(dpre, 8)
        dx = dw = dbias = None
        if ctx.needs_input_grad[0]:
            wt = pack_weight(weight, None, x.dtype, _roundup(cx, 128), dpre8.shape[3], 1)
            dx = conv_dgrad(dpre8, wt, kh, kw, stride, pad, (x.shape[1], x.shape[2]), cx,
                            relu_mask=x if (ctx.x_relu and FUSE_RELU_MASK) else None, mask_slope=ctx.x_mask_slope)
        need_b = has_bias and ctx.needs_input_grad[2]
        slot = None
        if ctx.sink is not None and ctx.needs_input_grad[1] and not _wgrad_swapped(stride, dpre8.shape[3], cx):
            arena, w_leaf, b_leaf, sn = ctx.sink
            slot = arena.grad_slot(w_leaf, None, b_leaf if need_b else None, None, kh * kw, dpre8.shape[3], cx, sn)
        if slot is not None:
            # gradient sink: the wgrad kernel accumulates into the optimiser's GEMM-order arena; nothing goes through autograd
            sink_wgrad(arena, slot, x, dpre8, kh, kw, stride, pad, need_b)
        elif ctx.needs_input_grad[1]:
            res = conv_wgrad(x, dpre8, kh, kw, stride, pad, want_bias=need_b)
            if need_b:
                dbias = res[1][:cout]
            dw = unpack_wgrad(res[0] if need_b else res, weight.shape)
        elif need_b:
            dbias = channel_sums(dpre8)[0, 0, :cout].float()
        dres = dpre if (has_resid and ctx.needs_input_grad[3]) else None
        return dx, dw, dbias, dres, None, None, None, None, None, None, None


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, stride: int = 1,
           padding: int = 0, act: int = ACT_NONE, slope: float = 0.2,
           resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NHWC convolution (+bias, +residual, +activation fused in the MFMA kernel's epilogue).

    `weight` is the reference-layout fp32 parameter [Cout, Cin, kh, kw]; `x` may carry more
    (zero) channels than Cin -- the packed weight is zero-padded to match.
    """
    if x.shape[-1] < weight.shape[1]:
        raise ValueError(f"conv2d: input has {x.shape[-1]} channels < weight Cin {weight.shape[1]}")
    xp = pad_channels(x, 8)
    fold, mslope = xp is x and getattr(x, "_mg_relu_out", False), 0.0
    if xp is x and not fold and FUSE_LRELU_MASK and getattr(x, "_mg_lrelu_out", None) is not None:
        fold, mslope = True, float(x._mg_lrelu_out)             # a LeakyReLU output whose producer named this conv its only consumer
        if torch.is_grad_enabled() and x.requires_grad and FUSE_RELU_MASK:
            _FOLD_EXPECTED[x.data_ptr()] = _weak_node(x)         # this conv's data gradient WILL carry x's mask: its producer must find it so
    y = _Conv2dFn.apply(xp, weight, bias, resid, stride, padding, act, slope, fold, _sink_for(weight, bias), mslope)
    if act == ACT_RELU:
        y._mg_relu_out = True        # consumers may fold this ReLU's backward mask into their data-gradient epilogue
    return y


def _sink_for(weight, bias, weight1=None, bias1=None):
    """(arena, leaf weight, leaf bias, spectral-norm state) when this convolution's parameter gradients can take the
    optimiser's gradient sink: the weight (or, under spectral norm, the `weight_orig` it was derived from -- see
    spectral_weight) and the bias are leaf parameters of the SAME optim.FlatAdam arena.  None = autograd path."""
    if not GRAD_SINK or not torch.is_grad_enabled():
        return None
    sn = getattr(weight, "_mg_sn", None)
    leaf = sn[0] if sn is not None else weight
    arena = getattr(leaf, "_mg_arena", None)
    if arena is None or not arena.sink or not leaf.requires_grad:
        return None
    for t in (bias, weight1, bias1):
        if t is not None and (getattr(t, "_mg_arena", None) is not arena or not t.requires_grad):
            return None
    return arena, leaf, bias, (sn[1:] if sn is not None else None)


def conv2d_infer(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, stride: int = 1,
                 padding: int = 0, dilation: int = 1, act: int = ACT_NONE, slope: float = 0.2,
                 resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inference-only NHWC convolution with dilation (the frozen in-painting net's dilated residual blocks,
    generator.py:452-461): the tap list carries the dilated offsets, everything else is conv2d's forward."""
    x = _nhwc(pad_channels(x.detach(), 8))
    if x.shape[3] < weight.shape[1]:
        raise ValueError(f"conv2d_infer: input has {x.shape[3]} channels < weight Cin {weight.shape[1]}")
    return _conv_forward("conv2d_infer", x, weight, bias, resid, stride, padding, dilation, act, slope)


def conv_transpose2d_infer(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                           stride: int = 2, padding: int = 1) -> torch.Tensor:
    """Inference-only nn.ConvTranspose2d on NHWC (weight [Cin, Cout, kh, kw], generator.py:533-539): it is the
    data gradient of the strided convolution with the same weight, i.e. one stride-1 gather per output-parity class
    with that class's tap subset (conv_dgrad) -- no zero-stuffed input, no wasted MACs."""
    x = _nhwc(pad_channels(x.detach(), 8))
    n, h, w, cx = x.shape
    cin, cout, kh, kw = weight.shape
    if cx < cin or cout % 8:
        raise ValueError("conv_transpose2d_infer: input channels must cover Cin and Cout must be a multiple of 8")
    ho, wo = (h - 1) * stride - 2 * padding + kh, (w - 1) * stride - 2 * padding + kw
    wt = pack_weight(weight, None, x.dtype, _roundup(cout, 128), cx, 1)    # columns past Cin are zero
    y = conv_dgrad(x, wt, kh, kw, stride, padding, (ho, wo), cout)
    if bias is not None:
        y = y + bias.detach().to(y.dtype)
    return y


# ----------------------------------------------------------------------------
# batch statistics (sync-BN) and SPADE modulation
# ----------------------------------------------------------------------------
def batch_stats_begin(x: torch.Tensor, up: bool = False):
    """First half of batch_stats: local channel sums and, when data parallel, the all-reduce of the 2C sums launched
    ASYNCHRONOUSLY -- the caller runs work that does not need the statistics (SPADE's mlp_shared conv) before
    batch_stats_finish, so the latency-bound collective overlaps with it.  Returns an opaque pending tuple.
    up=True: the statistics of the nearest 2x upsample of x (every value occurs four times), which is never materialised."""
    with torch.no_grad():
        x = _nhwc(x)
        c = x.shape[-1]
        count = x.numel() // c * (4 if up else 1)
        src = getattr(x, "_mg_stats_src", None) if STATS_FROM_UPSAMPLE_SOURCE else None
        # x = nearest 2x upsample of src (upsample2x) / up=True: every source value occurs exactly four times, so
        # sum(x) = 4 sum(src) and sum(x^2) = 4 sum(src^2) -- reduce the quarter-size tensor (x4 is exact in fp32)
        scale = 1.0
        if up:
            scale = 4.0
        elif src is not None and src.shape[-1] == c and 4 * src.numel() == x.numel():
            x, scale = src, 4.0
        if SYNC_BN_GROUP is None and FUSED_STATS_FINALIZE:
            return ("fused", x, scale), None, count, c          # no cross-rank reduction: statistics + finalize in one entry (batch_stats_finish)
        sums = channel_sums(x, shift=True)
        if scale != 1.0:
            sums.mul_(scale)
        work = None
        if SYNC_BN_GROUP is not None:
            import torch.distributed as dist
            work = _sync_bn_all_reduce(sums, "syncbn_fwd")
            count *= dist.get_world_size(SYNC_BN_GROUP)
        return sums, work, count, c


FUSED_STATS_FINALIZE = True      # A/B switch: mg_channel_stats_finalize (2 launches) instead of stats + [x 4] + finalize (3-4)


def stats_finalize(x: torch.Tensor, groups: int, count: float, eps: float, momentum: float = 0.0, running_mean=None, running_var=None,
                   sum_scale: float = 1.0):
    """(mean, rstd, sums) of x viewed as [G, P, C] with the finalize arithmetic fused into the second reduction stage."""
    c = x.shape[-1]
    p = x.numel() // (groups * c)
    be = C.backend()
    ws = _stats_workspace(groups, p, c, x.device)
    sums = torch.empty((groups, 2, c), dtype=torch.float64, device=x.device)
    mean = torch.empty((groups, c), dtype=torch.float32, device=x.device)
    rstd = torch.empty((groups, c), dtype=torch.float32, device=x.device)
    be.mg_channel_stats_finalize(_p(x), _dt(x), groups, p, c, float(sum_scale), float(count), eps, momentum, _p(running_mean), _p(running_var),
                                 _p(sums), _p(mean), _p(rstd), _p(ws), _stream(x))
    return mean, rstd, sums


def batch_stats_finish(pending, eps: float = 1e-5, momentum: float = 0.1,
                       running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None):
    """Second half: wait for the reduction (a stream dependency, not a host block, on RCCL) and finalize."""
    sums, work, count, c = pending
    with torch.no_grad():
        if isinstance(sums, tuple):                              # ("fused", x, scale)
            mean, rstd, sums = stats_finalize(sums[1], 1, count, eps, momentum, running_mean, running_var, sums[2])
            return mean.reshape(c), rstd.reshape(c), count, sums
        if work is not None:
            work.wait()
        mean = torch.empty(c, dtype=torch.float32, device=sums.device)
        rstd = torch.empty(c, dtype=torch.float32, device=sums.device)
        C.backend().mg_norm_finalize(_p(sums), 1, c, float(count), eps, momentum, _p(running_mean), _p(running_var),
                                     _p(mean), _p(rstd), _stream(sums))
        if SYNC_BN_REFERENCE_CLAMP and work is not None:
            # the reference's N-device branch (batchnorm.py:131-145): inv_std = clamp(biased_var, eps) ** -0.5, where its one-device branch
            # (F.batch_norm, :65-68) and this repo at every N compute (biased_var + eps) ** -0.5 -- see SYNC_BN_REFERENCE_CLAMP below
            s = sums.reshape(2, c)
            m64 = s[0] / count
            rstd = (s[1] / count - m64 * m64).clamp_min(eps).rsqrt().float()
        return mean, rstd, count, sums


# The reference computes 1 / sqrt(var + eps) on one device (F.batch_norm) but clamp(var, eps) ** -0.5 in its multi-device master
# (sync_batchnorm/batchnorm.py:145): its own 1-GPU and N-GPU runs differ by eps / (2 var) = 5e-6 relative at var = 1.  This repo keeps the
# one-device formula at every world size -- an N-rank run equals the 1-rank run on the concatenated batch, which is what the
# multi-rank tests assert.  MG_SYNCBN_REFERENCE_CLAMP=1 reproduces the reference's N-device formula instead (forward statistics only; the
# backward kernels take rstd as given and are valid for both whenever var > eps); a few tiny torch launches per normalised tensor.
SYNC_BN_REFERENCE_CLAMP = os.environ.get("MG_SYNCBN_REFERENCE_CLAMP") == "1"


def batch_stats(x: torch.Tensor, eps: float = 1e-5, momentum: float = 0.1,
                running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None):
    """Per-channel batch statistics of an NHWC tensor over (N, H, W) [x all ranks of SYNC_BN_GROUP].

    Returns (mean, rstd, count, sums); rstd = 1/sqrt(biased_var + eps) as F.batch_norm computes it on one device
    (sync_batchnorm/batchnorm.py:65-68).  Three launches: two-stage channel sums, [one all-reduce of the 2C sums
    when data parallel,] finalize (which also advances the running statistics when given).  Every rank holds the
    same number of elements (equal per-GPU batch), so the global count is local count x world size -- no host
    sync.  No autograd here: the dependence of the statistics on x is handled by the consumers' backward kernels.
    """
    return batch_stats_finish(batch_stats_begin(x), eps, momentum, running_mean, running_var)


def advance_running_stats(sums: torch.Tensor, count, eps: float, momentum: float,
                          running_mean: torch.Tensor, running_var: torch.Tensor):
    """Apply the momentum update of ANOTHER norm layer that normalises the same tensor (SPADE norm_0 / norm_s share
    x, architecture.py:68-70,79): one finalize launch on the already reduced sums."""
    c = running_mean.numel()
    scratch = torch.empty(2 * c, dtype=torch.float32, device=sums.device)
    C.backend().mg_norm_finalize(_p(sums), 1, c, float(count), eps, momentum, _p(running_mean), _p(running_var),
                                 _p(scratch[:c]), _p(scratch[c:]), _stream(sums))


def _count_collective(kind: str):
    from . import parallel
    parallel.COLLECTIVES[kind] += 1


_BIAS_PLANS = weakref.WeakKeyDictionary()        # arena -> plan of ALL (mlp_gamma.bias, mlp_beta.bias) pairs living in that optimiser arena


class _BiasPlan:
    """Every SPADE layer of a network needs its two bias vectors interleaved in the fused conv's GEMM row order, and they all change
    together (one optimiser step).  Parameters of a FlatAdam arena are slices of ONE flat tensor, so all pairs are refreshed by a single
    index_select over the arena (18 layers: 18 `stack` launches per optimiser step before)."""

    def __init__(self, arena):
        self.arena = weakref.ref(arena)
        self.pairs, self.known = [], set()
        self.index = self.mask = None
        self.flat_ptr = 0

    def register(self, bg, bb):
        key = (id(bg), id(bb))
        if key not in self.known:
            self.known.add(key)
            self.pairs.append((weakref.ref(bg), weakref.ref(bb)))
            self.index = None

    def refresh(self):
        arena = self.arena()
        live = [(r0(), r1()) for r0, r1 in self.pairs]
        if arena is None or any(a is None or b is None for a, b in live):
            return False
        if self.index is None or self.flat_ptr != arena.flat.data_ptr():
            idx, msk, self.offsets, off, padded = [], [], [], 0, False
            for bg, bb in live:
                c = bg.numel()
                cr = _roundup(c, 32)
                o0, o1 = arena._span_of[id(bg)][0], arena._span_of[id(bb)][0]
                ch = torch.arange(cr).reshape(cr // 32, 1, 32)
                src = torch.cat([o0 + ch, o1 + ch], dim=1)                       # [blocks][gamma | beta][32]
                ok = (ch < c).expand(cr // 32, 2, 32)
                padded = padded or cr != c
                idx.append(torch.where(ok, src, torch.zeros_like(src)).reshape(-1))
                msk.append(ok.reshape(-1))
                self.offsets.append((off, off + 2 * cr))
                off += 2 * cr
            dev = arena.flat.device
            self.index = torch.cat(idx).to(dev)
            self.mask = torch.cat(msk).to(dev).float() if padded else None
            self.flat_ptr = arena.flat.data_ptr()
        rows = torch.index_select(arena.flat.detach(), 0, self.index)
        if self.mask is not None:
            rows = rows * self.mask
        for (bg, bb), (a, b) in zip(live, self.offsets):
            _BIAS_PAIR_CACHE.put((bg.data_ptr(), bb.data_ptr()), (bg, bb), rows[a:b])
        return True


def spade_bias_rows(bg: torch.Tensor, bb: torch.Tensor) -> torch.Tensor:
    """_interleave32 of the (mlp_gamma.bias, mlp_beta.bias) parameters, cached until either changes (tensor versions + the
    optimiser arena's update count, like pack_weight); pairs that live in a FlatAdam arena are refreshed all at once (_BiasPlan)."""
    if not (isinstance(bg, torch.nn.Parameter) and isinstance(bb, torch.nn.Parameter)):
        return _interleave32(bg.detach().float(), bb.detach().float()).contiguous()
    key, params = (bg.data_ptr(), bb.data_ptr()), (bg, bb)
    hit = _BIAS_PAIR_CACHE.get(key, params)
    if hit is not None:
        return hit
    arena = getattr(bg, "_mg_arena", None)
    if arena is not None and getattr(bb, "_mg_arena", None) is arena and hasattr(arena, "_span_of") and BATCHED_PACK:
        plan = _BIAS_PLANS.get(arena)
        if plan is None:
            plan = _BIAS_PLANS[arena] = _BiasPlan(arena)
        plan.register(bg, bb)
        if plan.refresh():
            return _BIAS_PAIR_CACHE.get(key, params)
    rows = _interleave32(bg.detach().float(), bb.detach().float()).contiguous()
    _BIAS_PAIR_CACHE.put(key, params, rows)
    return rows


def _interleave32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[C], [C] -> [2*roundup(C,32)] in the fused-SPADE GEMM row order ([32 gamma | 32 beta] blocks)."""
    c = a.numel()
    cr = _roundup(c, 32)
    if cr != c:
        a, b = F.pad(a, (0, cr - c)), F.pad(b, (0, cr - c))
    return torch.stack([a.reshape(cr // 32, 32), b.reshape(cr // 32, 32)], dim=1).reshape(2 * cr)


def _spade_branch_fwd(who, x, actv, wg, bg, wb, bb, mean, rstd, act, slope, need_g1, up=False):
    """Forward launch of one gamma|beta branch of `who` (the public function, for the error text): (out, 1 + gamma or None).
    `up`: x is the half-resolution source of the tensor that is modulated."""
    n, h, w = actv.shape[:3]
    c = x.shape[3]
    if wg.shape != wb.shape or wg.shape[0] != c or wg.shape[1] != actv.shape[3]:
        raise ValueError(f"{who}: mlp_gamma / mlp_beta weights have the wrong shape")
    kh = wg.shape[2]
    rows = 2 * _roundup(c, 32)
    wp = pack_weight(wg, wb, x.dtype, _roundup(rows, 128), actv.shape[3], 0)
    bias = spade_bias_rows(bg, bb)
    out = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device)
    # (1 + gamma) is only needed by the backward pass: the no_grad generator forward of the
    # discriminator step (pix2pix_model.py:376) does not write it
    g1 = torch.empty_like(out) if need_g1 else None
    _launch_conv(actv, wp, out, bias, fwd_taps(kh, kh, kh // 2), Hj=h, Wj=w, isy=1, isx=1, cout=c, cout_gemm=rows,
                 act=act, slope=slope, spade_x=x, mean=mean, rstd=rstd, gamma_out=g1, x_up=up)
    return out, g1


def _spade_branch_reduce(dh, h, g1, x, mean, rstd, act, slope, sums, up=False):
    """Backward reduction of one branch: the gradient dgb of the gamma|beta conv's output and, into `sums` ([2, C] fp32), the two sums of the
    batch-norm gradient.  Returns (dgb, the activation the apply pass still has to undo, h's pointer for it).  `up` (pair node only): x is the half-resolution source."""
    n, hh, ww, c = dh.shape
    p = n * hh * ww
    rows = 2 * _roundup(c, 32)
    be = C.backend()
    alloc = torch.zeros if rows != 2 * c else torch.empty      # padded gamma/beta rows must read 0
    dgb = alloc((n, hh, ww, rows), dtype=x.dtype, device=x.device)
    ws = _stats_workspace(1, p, c, x.device)
    if _grad_premasked(dh, h, act):
        act = ACT_NONE                               # conv_0 / conv_1's data-gradient epilogue already applied the LeakyReLU mask
    hp = _p(h) if act != ACT_NONE else None          # the activation's output is only read for its sign
    if up:
        be.mg_norm_bwd_reduce_up(_p(dh), hp, _p(x), _p(g1), _dt(x), n, hh, ww, c, _p(mean), _p(rstd), act, slope,
                                 _p(dgb), _p(sums), _p(ws), _stream(x))
    else:
        be.mg_norm_bwd_reduce(_p(dh), hp, _p(x), _p(g1), _dt(x), 1, p, c, _p(mean), _p(rstd), act, slope,
                              _p(dgb), _p(sums), _p(ws), _stream(x))
    return dgb, act, hp


def _spade_branch_grads(needs, sink, actv, dgb, wg, wb, actv_relu):
    """Gradients of one branch's (actv, w_gamma, b_gamma, w_beta, b_beta) from dgb; `needs`: which of the five are wanted.
    What the optimiser's gradient sink takes (`sink` = (arena, leaf weight, b_gamma, b_beta)) comes back as None."""
    hh, ww, rows = dgb.shape[1:]
    c, kh = wg.shape[0], wg.shape[2]
    pad = kh // 2
    dactv = dwg = dbg = dwb = dbb = None
    if needs[0]:
        wt = pack_weight(wg, wb, dgb.dtype, _roundup(actv.shape[3], 128), rows, 1)
        dactv = conv_dgrad(dgb, wt, kh, kh, 1, pad, (hh, ww), actv.shape[3],
                           relu_mask=actv if (actv_relu and FUSE_RELU_MASK) else None)      # mlp_shared's ReLU (normalization.py:94-99)
    need_w = needs[1] or needs[3]
    need_b = needs[2] or needs[4]
    slot = db = None
    if sink is not None and needs[1] and needs[3]:
        slot = sink[0].grad_slot(wg, wb, sink[2] if need_b else None, sink[3] if need_b else None, kh * kh, rows, actv.shape[3], None)
    if slot is not None:
        sink_wgrad(sink[0], slot, actv, dgb, kh, kh, 1, pad, need_b)
    elif need_w:
        res = conv_wgrad(actv, dgb, kh, kh, 1, pad, want_bias=need_b)
        dwg, dwb = unpack_wgrad(res[0] if need_b else res, wg.shape, two=True)
        db = res[1] if need_b else None
    elif need_b:
        db = channel_sums(dgb)[0, 0].float()
    if db is not None:
        db = db.reshape(rows // 64, 2, 32)
        dbg, dbb = db[:, 0].reshape(-1)[:c], db[:, 1].reshape(-1)[:c]
    return dactv, dwg, dbg, dwb, dbb


class _SpadeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, actv, w_gamma, b_gamma, w_beta, b_beta, mean, rstd, count, act, slope, actv_relu=False, sink=None):
        ctx.actv_relu = bool(actv_relu)
        ctx.sink = sink
        x, actv = _nhwc(x), _nhwc(actv)
        if actv.shape[:3] != x.shape[:3] or actv.dtype != x.dtype:
            raise ValueError("spade_modulate: activation map and x disagree in shape/dtype")
        out, g1 = _spade_branch_fwd("spade_modulate", x, actv, w_gamma, b_gamma, w_beta, b_beta, mean, rstd, act, slope,
                                    any(ctx.needs_input_grad))
        if g1 is not None:
            ctx.save_for_backward(x, actv, w_gamma, w_beta, out, g1, mean, rstd)
        ctx.cfg = (count, act, slope)
        return out

    @staticmethod
    def backward(ctx, dh):
        x, actv, w_gamma, w_beta, h, g1, mean, rstd = ctx.saved_tensors
        count, act, slope = ctx.cfg
        dh = dh.contiguous()
        n, hh, ww, c = x.shape
        sums = torch.empty((1, 2, c), dtype=torch.float32, device=x.device)
        dgb, act, hp = _spade_branch_reduce(dh, h, g1, x, mean, rstd, act, slope, sums)
        dx = work = None
        if ctx.needs_input_grad[0] and SYNC_BN_GROUP is not None:
            work = _sync_bn_all_reduce(sums, "syncbn_bwd")    # overlaps with the gamma/beta conv's backward below
        dactv, dwg, dbg, dwb, dbb = _spade_branch_grads(ctx.needs_input_grad[1:6], ctx.sink, actv, dgb, w_gamma, w_beta, ctx.actv_relu)
        if ctx.needs_input_grad[0]:
            if work is not None:
                work.wait()
            dx = torch.empty_like(x)
            C.backend().mg_norm_bwd_apply(_p(dh), hp, _p(x), _p(g1), _dt(x), 1, n * hh * ww, c, _p(mean), _p(rstd),
                                          _p(sums[0, 0]), _p(sums[0, 1]), 2 * c, 1.0 / float(count), act, slope, _p(dx), _stream(x))
        return dx, dactv, dwg, dbg, dwb, dbb, None, None, None, None, None, None, None


class _SpadePairFn(torch.autograd.Function):
    """Two SPADE modulations of the SAME x with shared batch statistics -- norm_0 (+LeakyReLU) and norm_s of a residual block
    with a learned shortcut (architecture.py:68-70,79) -- as one autograd node, so that the backward pass makes ONE pass for
    dx (mg_norm_bwd_apply2: both branches' terms and, when x entered through a nearest 2x upsample, the 2x2 adjoint) instead of
    two applies + autograd's add + the upsample's backward, and ONE sync-BN all-reduce for the pair.  `up`: x is the
    half-resolution source; the fused convs read it at (y >> 1, x >> 1) and the upsampled tensor never exists."""

    @staticmethod
    def forward(ctx, x, actv0, wg0, bg0, wb0, bb0, actv1, wg1, bg1, wb1, bb1, mean, rstd, count, act0, act1, slope, up, relu0, relu1, sinks):
        x, actv0, actv1 = _nhwc(x), _nhwc(actv0), _nhwc(actv1)
        n, hs, ws, c = x.shape
        h, w = (2 * hs, 2 * ws) if up else (hs, ws)
        if actv0.shape[:3] != (n, h, w) or actv1.shape[:3] != (n, h, w) or actv0.dtype != x.dtype or actv1.dtype != x.dtype:
            raise ValueError("spade_modulate_pair: activation maps and x disagree in shape / dtype")
        need = any(ctx.needs_input_grad)
        (out0, g10), (out1, g11) = (_spade_branch_fwd("spade_modulate_pair", x, actv, wg, bg, wb, bb, mean, rstd, act, slope, need, up)
                                    for actv, wg, bg, wb, bb, act in ((actv0, wg0, bg0, wb0, bb0, act0), (actv1, wg1, bg1, wb1, bb1, act1)))
        if need:
            ctx.save_for_backward(x, actv0, wg0, wb0, out0, g10, actv1, wg1, wb1, out1, g11, mean, rstd)
        ctx.cfg = (count, (act0, act1), slope, bool(up), (bool(relu0), bool(relu1)), sinks, (h, w))
        return out0, out1

    @staticmethod
    def backward(ctx, dh0, dh1):
        x, actv0, wg0, wb0, h0, g10, actv1, wg1, wb1, h1, g11, mean, rstd = ctx.saved_tensors
        count, acts, slope, up, relus, sinks, (hh, ww) = ctx.cfg
        n, _, _, c = x.shape
        need_x = ctx.needs_input_grad[0]
        sums = torch.empty((2, 2, c), dtype=torch.float32, device=x.device)          # [branch][sum dxhat | sum dxhat * xhat][C]
        branches = ((dh0.contiguous(), h0, g10, actv0, wg0, wb0, 1), (dh1.contiguous(), h1, g11, actv1, wg1, wb1, 6))
        reduced = [_spade_branch_reduce(dh, h, g1, x, mean, rstd, acts[b], slope, sums[b], up)
                   for b, (dh, h, g1, *_r) in enumerate(branches)]
        work = None
        if need_x and SYNC_BN_GROUP is not None:
            work = _sync_bn_all_reduce(sums, "syncbn_bwd")         # both branches in ONE collective; overlaps with the convs below
        grads = [None] * 11
        for b, (dh, h, g1, actv, wg, wb, base) in enumerate(branches):
            grads[base:base + 5] = _spade_branch_grads(ctx.needs_input_grad[base:base + 5], sinks[b], actv, reduced[b][0], wg, wb, relus[b])
        if need_x:
            if work is not None:
                work.wait()
            d = C.NormApply2Desc()
            for b, (dh, h, g1, *_r) in enumerate(branches):
                act = reduced[b][1]
                d.dh[b], d.g1[b], d.sums[b] = dh.data_ptr(), g1.data_ptr(), sums[b].data_ptr()
                d.h[b] = h.data_ptr() if act != ACT_NONE else None
                d.act[b], d.slope[b] = act, slope
            d.x, d.mean, d.rstd = x.data_ptr(), mean.data_ptr(), rstd.data_ptr()
            dx = torch.empty_like(x)
            d.dx, d.P, d.dtype, d.C = dx.data_ptr(), n * hh * ww, _dt(x), c
            d.up, d.H, d.W, d.inv_count = (1 if up else 0), hh, ww, 1.0 / float(count)
            C.backend().mg_norm_bwd_apply2(d, _stream(x))
            grads[0] = dx
        return tuple(grads) + (None,) * 10


def spade_pair_supported(x: torch.Tensor) -> bool:
    return bool(C.backend().mg_norm_apply2_supported(_dt(x), x.shape[-1])) and x.numel() * 4 < (1 << 32)


def spade_modulate_pair(x, mods, mean, rstd, count, *, acts, slope=0.2, up=False):
    """(h0, h1) = the two SPADE modulations `mods` = ((actv, w_gamma, b_gamma, w_beta, b_beta), ...) of the same x (or of its
    nearest 2x upsample when `up`), one fused conv launch each, ONE autograd node (see _SpadePairFn)."""
    (a0, wg0, bg0, wb0, bb0), (a1, wg1, bg1, wb1, bb1) = mods
    sk0, sk1 = _sink_for(wg0, bg0, wb0, bb0), _sink_for(wg1, bg1, wb1, bb1)
    sinks = (None if sk0 is None else (sk0[0], sk0[1], bg0, bb0), None if sk1 is None else (sk1[0], sk1[1], bg1, bb1))
    return _SpadePairFn.apply(x, a0, wg0, bg0, wb0, bb0, a1, wg1, bg1, wb1, bb1, mean, rstd, count, acts[0], acts[1], slope, bool(up),
                              getattr(a0, "_mg_relu_out", False), getattr(a1, "_mg_relu_out", False), sinks)


def spade_modulate(x, actv, w_gamma, b_gamma, w_beta, b_beta, mean, rstd, count, *, act=ACT_NONE, slope=0.2):
    """h = act( (x - mean) * rstd * (1 + conv(actv, Wg) + bg) + conv(actv, Wb) + bb ), one MFMA launch.

    gamma and beta are produced and consumed in registers (normalization.py:111-116 writes
    both to memory and makes ~12 elementwise passes).  The backward implements the full
    batch-norm gradient (statistics included), so `mean`/`rstd` enter as constants.
    """
    sk = _sink_for(w_gamma, b_gamma, w_beta, b_beta)
    return _SpadeFn.apply(x, actv, w_gamma, b_gamma, w_beta, b_beta, mean, rstd, count, act, slope,
                          getattr(actv, "_mg_relu_out", False), None if sk is None else (sk[0], sk[1], b_gamma, b_beta))


# ----------------------------------------------------------------------------
# instance norm (+ activation)
# ----------------------------------------------------------------------------
class _InstanceNormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, act, slope):
        x = _nhwc(x)
        n, h, w, c = x.shape
        p = h * w
        if FUSED_STATS_FINALIZE:
            mean, rstd, _ = stats_finalize(x, n, float(p), eps)
        else:
            sums = channel_sums(x, groups=n, shift=True)
            mean = torch.empty((n, c), dtype=torch.float32, device=x.device)
            rstd = torch.empty((n, c), dtype=torch.float32, device=x.device)
            C.backend().mg_norm_finalize(_p(sums), n, c, float(p), eps, 0.0, None, None, _p(mean), _p(rstd), _stream(x))
        y = torch.empty_like(x)
        C.backend().mg_norm_act_fwd(_p(x), _p(y), _dt(x), n, p, c, _p(mean), _p(rstd), act, slope, None, _stream(x))
        ctx.save_for_backward(x, y, mean, rstd)
        ctx.cfg = (act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd = ctx.saved_tensors
        act, slope = ctx.cfg
        dy = dy.contiguous()
        n, h, w, c = x.shape
        p = h * w
        be = C.backend()
        sums = torch.empty((n, 2, c), dtype=torch.float32, device=x.device)
        ws = _stats_workspace(n, p, c, x.device)
        be.mg_norm_bwd_reduce(_p(dy), _p(y), _p(x), None, _dt(x), n, p, c, _p(mean), _p(rstd), act, slope,
                              None, _p(sums), _p(ws), _stream(x))
        dx = torch.empty_like(x)
        be.mg_norm_bwd_apply(_p(dy), _p(y), _p(x), None, _dt(x), n, p, c, _p(mean), _p(rstd), _p(sums[0, 0]), _p(sums[0, 1]),
                             2 * c, 1.0 / float(p), act, slope, _p(dx), _stream(x))
        return dx, None, None, None


def instance_norm_act(x, *, eps: float = 1e-5, act: int = ACT_NONE, slope: float = 0.2):
    """nn.InstanceNorm2d(affine=False) followed by an optional fused activation (NHWC)."""
    return _InstanceNormActFn.apply(x, eps, act, slope)


def instance_norm_act_infer(x, *, eps: float = 1e-5, act: int = ACT_NONE, slope: float = 0.2, resid: Optional[torch.Tensor] = None):
    """Inference-only instance norm + activation [+ resid] (the frozen in-painting net: `x + IN(conv(...))`, generator.py:463):
    statistics (2 launches) and ONE apply launch that also adds the skip connection (was an extra element-wise launch per block)."""
    x = _nhwc(x.detach())
    n, h, w, c = x.shape
    mean, rstd, _ = stats_finalize(x, n, float(h * w), eps)
    if resid is not None:
        resid = _nhwc(resid.detach())
        if resid.shape != x.shape or resid.dtype != x.dtype:
            raise ValueError("instance_norm_act_infer: the residual must match x")
    y = torch.empty_like(x)
    C.backend().mg_norm_act_fwd(_p(x), _p(y), _dt(x), n, h * w, c, _p(mean), _p(rstd), act, slope, _p(resid), _stream(x))
    return y


# ----------------------------------------------------------------------------
# resampling / pooling / blending
# ----------------------------------------------------------------------------
def _geom(x):
    n, h, w, c = x.shape
    if c % 4:
        raise ValueError(f"NHWC streaming kernels need C % 4 == 0, got {c}")
    return n, h, w, c


class _Up2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _nhwc(x)
        n, h, w, c = _geom(x)
        y = torch.empty((n, 2 * h, 2 * w, c), dtype=x.dtype, device=x.device)
        C.backend().mg_upsample2x_fwd(_p(x), _p(y), _dt(x), n, h, w, c, _stream(x))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        n, h2, w2, c = dy.shape
        dx = torch.empty((n, h2 // 2, w2 // 2, c), dtype=dy.dtype, device=dy.device)
        C.backend().mg_upsample2x_bwd(_p(dy), _p(dx), _dt(dy), n, h2 // 2, w2 // 2, c, _stream(dy))
        return dx


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _nhwc(x)
        n, h, w, c = _geom(x)
        y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=x.dtype, device=x.device)
        C.backend().mg_avgpool3s2_fwd(_p(x), _p(y), _dt(x), n, h, w, c, _stream(x))
        ctx.hw = (h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        h, w = ctx.hw
        n, _, _, c = dy.shape
        dx = torch.empty((n, h, w, c), dtype=dy.dtype, device=dy.device)
        C.backend().mg_avgpool3s2_bwd(_p(dy), _p(dx), _dt(dy), n, h, w, c, _stream(dy))
        return dx


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x_relu=False):
        ctx.x_relu = bool(x_relu)
        x = _nhwc(x)
        n, h, w, c = _geom(x)
        y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
        C.backend().mg_maxpool2_fwd(_p(x), _p(y), _dt(x), n, h, w, c, _stream(x))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        n, h, w, c = x.shape
        dx = torch.empty_like(x)
        fuse = ctx.x_relu and FUSE_RELU_MASK
        C.backend().mg_maxpool2_bwd(_p(dy), _p(x), _p(dx), _dt(x), n, h, w, c, 1 if fuse else 0, _stream(x))
        if fuse:                      # dx already carries the mask of the ReLU that produced x: its conv skips act_backward
            _leave_mask_record(dx, x)
        return dx, None


class _BlendFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bg, x, hair, back, act, slope):
        bg, x = _nhwc(bg), _nhwc(x)
        if bg.shape != x.shape or bg.dtype != x.dtype:
            raise ValueError("blend: background features and x disagree")
        n, h, w, c = _geom(x)
        hair = hair.reshape(-1).float().contiguous()
        back = back.reshape(-1).float().contiguous()
        if hair.numel() != n * h * w or back.numel() != n * h * w:
            raise ValueError("blend: masks must have one value per pixel")
        y = torch.empty_like(x)
        C.backend().mg_blend_fwd(_p(bg), _p(x), _p(hair), _p(back), _p(y), _dt(x), n * h * w, c, act, slope, _stream(x))
        ctx.save_for_backward(hair, back, y if act != ACT_NONE else None)
        ctx.cfg = (act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        hair, back, y = ctx.saved_tensors
        act, slope = ctx.cfg
        dy = dy.contiguous()
        c = dy.shape[-1]
        p = dy.numel() // c
        dbg = torch.empty_like(dy) if ctx.needs_input_grad[0] else None
        dx = torch.empty_like(dy) if ctx.needs_input_grad[1] else None
        if dbg is not None or dx is not None:
            C.backend().mg_blend_bwd(_p(dy), _p(y), _p(hair), _p(back), _p(dbg), _p(dx), _dt(dy), p, c, act, slope, _stream(dy))
        return dbg, dx, None, None, None, None


class _ReflectPadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        x = _nhwc(x)
        n, h, w, c = x.shape
        y = torch.empty((n, h + 2 * p, w + 2 * p, c), dtype=x.dtype, device=x.device)
        C.backend().mg_reflect_pad_fwd(_p(x), _p(y), _dt(x), n, h, w, c, p, _stream(x))
        ctx.meta = (n, h, w, c, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, h, w, c, p = ctx.meta
        dy = dy.contiguous()
        dx = torch.empty((n, h, w, c), dtype=dy.dtype, device=dy.device)
        C.backend().mg_reflect_pad_bwd(_p(dy), _p(dx), _dt(dy), n, h, w, c, p, _stream(dy))
        return dx, None


def reflect_pad(x: torch.Tensor, p: int) -> torch.Tensor:
    """nn.ReflectionPad2d(p) on an NHWC tensor: one gather pass forward, one gather pass (adjoint) backward."""
    if p == 0:
        return x
    if x.shape[-1] % 4 or not (1 <= p < min(x.shape[1], x.shape[2])):
        raise ValueError("reflect_pad: channels must be a multiple of 4 and 1 <= p < min(H, W)")
    return _ReflectPadFn.apply(x, p)


def upsample2x(x):
    """nn.Upsample(scale_factor=2, mode='nearest') on NHWC.  The result remembers its source so that batch
    statistics of it (SPADE norm_0 / norm_s of the next block) can be reduced from the quarter-size tensor."""
    y = _Up2Fn.apply(x)
    y._mg_stats_src = x.detach()
    return y


def avgpool3s2(x):
    """F.avg_pool2d(k=3, s=2, p=1, count_include_pad=False) on NHWC."""
    return _AvgPoolFn.apply(x)


def maxpool2(x):
    """nn.MaxPool2d(2, 2) on NHWC."""
    return _MaxPoolFn.apply(x, getattr(x, "_mg_relu_out", False))


class _AssembleFn(torch.autograd.Function):
    """dst[n0:n0+N] = [planar | image[..., :cf] | 0] per pixel (mg_assemble_nhwc8); gradient to the NHWC image only."""

    @staticmethod
    def forward(ctx, image, planar, dst, n0, cf):
        n, h, w, cs = image.shape
        cp = planar.shape[1]
        C.backend().mg_assemble_nhwc8(_p(planar), cp, _p(image), cs, cf, _p(dst[n0:n0 + n]), _dt(dst), n, h * w, _stream(dst))
        ctx.meta = (n0, n, cp, cf, cs)
        ctx.mark_dirty(dst)
        return dst

    @staticmethod
    def backward(ctx, g):
        n0, n, cp, cf, cs = ctx.meta
        dimg = g[n0:n0 + n, :, :, cp:cp + cf]
        if cs != cf:
            dimg = F.pad(dimg, (0, cs - cf))
        return dimg.contiguous(), None, None, None, None


def assemble_nhwc8(dst: torch.Tensor, n0: int, planar: torch.Tensor, image: Optional[torch.Tensor] = None, cf: int = 0) -> torch.Tensor:
    """Fill dst[n0 : n0 + N] ([*, H, W, 8] NHWC, compute dtype) with [planar fp32 NCHW maps | first cf channels of the NHWC
    `image` | zeros] per pixel, one launch; differentiable w.r.t. `image`."""
    planar = _f32_dense(planar)
    if image is None:
        n, _, h, w = planar.shape
        C.backend().mg_assemble_nhwc8(_p(planar), planar.shape[1], None, 0, 0, _p(dst[n0:n0 + n]), _dt(dst), n, h * w, _stream(dst))
        return dst
    image = _nhwc(image)
    if image.dtype != dst.dtype:
        image = image.to(dst.dtype)
    if image.requires_grad and torch.is_grad_enabled():
        return _AssembleFn.apply(image, planar, dst, n0, cf)
    n, h, w, cs = image.shape
    C.backend().mg_assemble_nhwc8(_p(planar), planar.shape[1], _p(image), cs, cf, _p(dst[n0:n0 + n]), _dt(dst), n, h * w, _stream(dst))
    return dst


class _ActTapFn(torch.autograd.Function):
    """Identity on an activation's output `a` that has two consumers; returns two aliases.  Its backward adds the two incoming
    gradients AND applies the activation's derivative in one pass (mg_grad_sum_act), then tells the producing conv that its
    activation backward is done (the _RELU_MASKED record) -- instead of autograd's add followed by act_backward."""

    @staticmethod
    def forward(ctx, a, act, slope):
        ctx.save_for_backward(a)
        ctx.cfg = (act, slope)
        return a.view_as(a), a.view_as(a)

    @staticmethod
    def backward(ctx, g1, g2):
        (a,) = ctx.saved_tensors
        act, slope = ctx.cfg
        if g1 is None and g2 is None:
            return None, None, None
        if g1 is None:
            g1, g2 = g2, None
        g1 = g1.contiguous()
        # a gradient that a consumer's data-gradient epilogue / max-pool backward already masked with this ReLU stays correct
        # under a second multiplication by the same 0/1 mask; drop its record, the sum gets a new one
        _take_mask_record(g1, a)
        if g2 is not None:
            g2 = g2.contiguous()
            _take_mask_record(g2, a)
        out = torch.empty_like(a)
        C.backend().mg_grad_sum_act(_p(g1), _p(g2), _p(a), _p(out), _dt(a), a.numel(), act, slope, _stream(a))
        if act == ACT_RELU:
            _leave_mask_record(out, a)
        return out, None, None


def act_tap(a: torch.Tensor, act: int = ACT_RELU, slope: float = 0.2):
    """(a1, a2): two aliases of the activation output `a` for its two consumers (see _ActTapFn).  ReLU only: for other
    activations the producer still runs its own activation backward, so the tap must not apply the derivative."""
    if act != ACT_RELU or not (torch.is_grad_enabled() and a.requires_grad) or a.numel() % 4 or not FUSE_RELU_MASK:
        return a, a
    a1, a2 = _ActTapFn.apply(a, act, slope)
    a1._mg_relu_out = a2._mg_relu_out = getattr(a, "_mg_relu_out", False)
    return a1, a2


def blend(bg, x, hair_mask, back_mask, *, act: int = ACT_NONE, slope: float = 0.2):
    """act(bg * (1 - hair_mask) + x * (1 - back_mask)); masks are per-pixel (N*H*W values)."""
    return _BlendFn.apply(bg, x, hair_mask, back_mask, act, slope)


# Lengths, in floats, of what the scalar losses' two-stage reductions write: one row of per-workgroup partial sums per term.  The kernels
# index these buffers by their own constants; tests/test_ops_emulated.py holds each name here to the constexpr it mirrors.
L1_MEAN_BLOCKS = 1024                                  # the grid cap of mg_l1_mean_fwd (a literal in csrc/mg_pointwise.hip)
ORIENT_LOSS_BLOCKS, ORIENT_LOSS_TERMS = 1024, 3        # OL_BLOCKS (csrc/mg_glue.hip); orient, conf and the hair count
COLOR_LOSS_BLOCKS, COLOR_LOSS_TERMS = 1024, 3          # CL_BLOCKS (csrc/mg_color_loss.hip); lab, rgb, background
HAIR_LAB_BLOCKS, HAIR_LAB_TERMS = 1024, 7              # HL_BLOCKS, HL_TERMS (csrc/mg_hair_lab.hip)


def _l1_mean_launch(a, b):
    """mean |a - b| of two dense tensors of one shape and dtype as a 0-d fp32 tensor (mg_l1_mean_fwd)."""
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    ws = torch.empty(L1_MEAN_BLOCKS, dtype=torch.float32, device=a.device)
    C.backend().mg_l1_mean_fwd(_p(a), _p(b), _dt(a), a.numel(), _p(out), _p(ws), _stream(a))
    return out.reshape(())


class _L1MeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError("l1_mean: tensors must agree in shape and dtype")
        ctx.save_for_backward(a, b)
        return _l1_mean_launch(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        (g,) = _f32_grads(g)
        da = torch.empty_like(a)
        C.backend().mg_l1_mean_bwd(_p(a), _p(b), _p(g), _dt(a), a.numel(), _p(da), _stream(a))
        return da, None


class _L1HalvesFn(torch.autograd.Function):
    """mean |t[:B] - t[B:]| of a batch-stacked tensor (discriminator features of [fake | real]), gradient to the
    first half only.  Same kernels as _L1MeanFn, but the gradient is produced in the STACKED layout (real half
    zero): slicing the halves outside would make autograd materialise a zero-padded copy per feature map and add
    it with a strided kernel."""

    @staticmethod
    def forward(ctx, t):
        half = t.shape[0] // 2
        ctx.save_for_backward(t)
        return _l1_mean_launch(t[:half], t[half:])

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        half = t.shape[0] // 2
        (g,) = _f32_grads(g)
        dt = torch.empty_like(t)
        C.backend().mg_l1_mean_bwd(_p(t[:half]), _p(t[half:]), _p(g), _dt(t), t[:half].numel(), _p(dt[:half]), _stream(t))
        dt[half:].zero_()
        return dt


def l1_mean_halves(t: torch.Tensor) -> torch.Tensor:
    """mean |t[:B] - t[B:].detach()| for a batch-stacked NCHW view of NHWC memory (or a dense tensor)."""
    t = _dense_view(t)
    half = t.shape[0] // 2
    if t.shape[0] % 2 or t[:half].numel() % 4 or t.dtype not in (torch.float32, torch.bfloat16):
        return F.l1_loss(t[:half].float(), t[half:].detach().float())
    return _L1HalvesFn.apply(t)


def _dense_view(t: torch.Tensor) -> torch.Tensor:
    """A contiguous alias of t when t is an NCHW view of NHWC memory (what the networks return), else a copy."""
    if t.dim() == 4:
        v = t.permute(0, 2, 3, 1)
        if v.is_contiguous():
            return v
    return t.contiguous()


def l1_mean(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """mean |a - b| (fp32 scalar) with gradient to `a` only; one HIP pass forward, one backward."""
    a, b = _dense_view(a), _dense_view(b.detach())
    if a.dtype != b.dtype:
        b = b.to(a.dtype)
    if a.numel() % 4 or a.dtype not in (torch.float32, torch.bfloat16):
        return F.l1_loss(a.float(), b.float())
    return _L1MeanFn.apply(a, b)


# ----------------------------------------------------------------------------
# per-pixel glue around the convolutions (mg_glue.hip): one launch each instead of chains of eager element-wise ops
# ----------------------------------------------------------------------------
def _rows_dense(t: torch.Tensor) -> bool:
    """Are the rows of the [N, H, W] view `t` dense (as in a channel slice of an NCHW tensor)?  The sample stride is free."""
    return t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2]


def _plane_args(t: Optional[torch.Tensor]):
    """(pointer, sample stride in elements) of an fp32 [N, H, W] view whose rows are dense; (None, 0) for an absent plane."""
    if t is None:
        return None, 0
    if t.dtype != torch.float32 or not _rows_dense(t):
        raise ValueError("expected an fp32 [N, H, W] view with dense rows")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2])


def _f32_dense(t: Optional[torch.Tensor]):
    """`t` detached, fp32 and contiguous (None stays None): the tensor's own storage when it is all three already -- no copy, no launch."""
    return None if t is None else t.detach().float().contiguous()


def _f32_plane(t: Optional[torch.Tensor], what: str, nhw) -> torch.Tensor:
    """`t` detached and fp32 as a plane _plane_args takes: a view of its own storage when its rows are dense, a copy otherwise.
    `what` ("operator: the operand") starts the error texts; `nhw`: the (N, H, W) the plane has to have."""
    if t is None:
        raise ValueError(f"{what} is needed for the selected terms")
    t = t.detach().float()
    if tuple(t.shape) != tuple(nhw):
        raise ValueError(f"{what} {tuple(t.shape)} does not match [N, H, W] = {tuple(nhw)}")
    return t if _rows_dense(t) else t.contiguous()


def _f32_grads(*grads):
    """The scalar gradients that reach a loss's backward pass, each as fp32; an absent one (None) stays absent."""
    return [None if g is None else g.float() for g in grads]


def planes_of(t: torch.Tensor):
    """The channel planes of an NCHW fp32 tensor as [N, H, W] views (no copy when the tensor is dense)."""
    t = _f32_dense(t)
    return [t[:, c] for c in range(t.shape[1])]


def nearest_pyramid(planes, sizes, cout: int, dtype):
    """F.interpolate(cat(planes), size, mode='nearest') for every (h, w) of `sizes`, each as an NHWC [N, h, w, cout] tensor in
    `dtype` (channels beyond len(planes) zero): ONE launch for the whole pyramid.  planes: fp32 [N, H, W] views."""
    n, H, W = planes[0].shape
    if not (1 <= len(planes) <= 8 and len(planes) <= cout <= 8 and 1 <= len(sizes) <= 8):
        raise ValueError("nearest_pyramid: at most 8 planes / channels / levels")
    d = C.PyramidDesc()
    for c, pl in enumerate(planes):
        if pl.shape != planes[0].shape or pl.device != planes[0].device:
            raise ValueError("nearest_pyramid: planes disagree in shape / device")
        d.plane[c], d.nstride[c] = _plane_args(pl)
    d.nplanes, d.N, d.H, d.W, d.nlev, d.cout = len(planes), n, H, W, len(sizes), cout
    outs = []
    d.dtype = _dtype_code(dtype)
    for l, (h, w) in enumerate(sizes):
        o = torch.empty((n, int(h), int(w), cout), dtype=dtype, device=planes[0].device)
        d.h[l], d.w[l], d.out[l] = int(h), int(w), o.data_ptr()
        outs.append(o)
    C.backend().mg_nearest_pyramid(d, _stream(planes[0]))
    return outs


def pconv_mask(mask: torch.Tensor, k: int, s: int, p: int):
    """Mask half of a partial convolution: mask fp32 [N, H, W(, 1)] -> (mask_ratio * update_mask, update_mask), fp32 [N, h, w, 1]."""
    m = mask.detach()
    if m.dim() == 4:
        m = m.reshape(m.shape[0], m.shape[1], m.shape[2]) if m.shape[3] == 1 else m[:, 0]
    m = m.float().contiguous()
    n, H, W = m.shape
    h, w = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    scale = torch.empty((n, h, w, 1), dtype=torch.float32, device=m.device)
    upd = torch.empty((n, h, w, 1), dtype=torch.float32, device=m.device)
    C.backend().mg_pconv_mask(_p(m), n, H, W, k, s, p, _p(scale), _p(upd), _stream(m))
    return scale, upd


class _PixelAffineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, bias, b):
        x = _nhwc(x)
        c = x.shape[-1]
        pix = x.numel() // c
        if a.numel() != pix or a.dtype != torch.float32 or (b is not None and (b.numel() != pix or b.dtype != torch.float32)):
            raise ValueError("pixel_affine: one fp32 value per pixel expected")
        y = torch.empty_like(x)
        bf = _f32_dense(bias)
        C.backend().mg_pixel_affine(_p(x), _p(a), _p(bf), _p(b) if bias is not None else None, _dt(x), pix, c, _p(y), _stream(x))
        ctx.save_for_backward(a, b if bias is not None else None)
        ctx.bias_dtype = bias.dtype if bias is not None else None
        return y

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        c = g.shape[-1]
        dx = dbias = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(g)
            C.backend().mg_pixel_affine(_p(g), _p(a), None, None, _dt(g), g.numel() // c, c, _p(dx), _stream(g))
        if ctx.needs_input_grad[2]:
            # sum_p g[p, c] * b[p]: mask the gradient (b is the 0/1 update mask: exact in any dtype) and take the deterministic two-stage
            # channel sums -- a gemv over the [P, C] gradient ran 1.1 ms per layer in rocBLAS (P = 524288 rows)
            gm = torch.empty_like(g)
            C.backend().mg_pixel_affine(_p(g), _p(b), None, None, _dt(g), g.numel() // c, c, _p(gm), _stream(g))
            dbias = channel_sums(gm)[0, 0].to(ctx.bias_dtype)
        return dx, None, dbias, None


def pixel_affine(x: torch.Tensor, a: torch.Tensor, bias: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[p, c] = x[p, c] * a[p] (+ bias[c] * b[p]) on an NHWC tensor; a, b: fp32, one value per pixel.  Differentiable w.r.t. x and bias."""
    if x.shape[-1] % 4:
        y = x * a.reshape(x.shape[:-1] + (1,)).to(x.dtype)
        return y if bias is None else y + bias.to(x.dtype) * b.reshape(x.shape[:-1] + (1,)).to(x.dtype)
    return _PixelAffineFn.apply(x, a.contiguous(), bias, b.contiguous() if b is not None else None)


def bg_compose(image: Optional[torch.Tensor], noise: Optional[torch.Tensor], hair: torch.Tensor, k: int, mode: int, dtype):
    """Background-encoder input in one launch: (inp NHWC8 in `dtype`, back fp32 [N, 1, H, W]).  image / noise: NCHW fp32 (3 channels),
    hair: fp32 [N, H, W] view; mode 0: back = 1 - maxpool_kxk(hair), mode 1: back = hair."""
    src = image if image is not None else noise
    n, _, H, W = src.shape
    img, noi = _f32_dense(image), _f32_dense(noise)
    hp, hs = _plane_args(hair.detach())
    inp = torch.empty((n, H, W, 8), dtype=dtype, device=src.device)
    back = torch.empty((n, 1, H, W), dtype=torch.float32, device=src.device)
    C.backend().mg_bg_compose(_p(img), _p(noi), hp, hs, _dtype_code(dtype), n, H, W, int(k), int(mode),
                              _p(inp), _p(back), _stream(src))
    return inp, back


class _MaskedMeanFillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lref, ltag):
        x = _nhwc(x)
        n, h, w, c = x.shape
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
        C.backend().mg_masked_mean_fill(_p(x), _p(lref), _p(ltag), _p(lref), _dt(x), n, h * w, c, _p(out), _stream(x))
        ctx.save_for_backward(lref, ltag)
        ctx.xdtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        lref, ltag = ctx.saved_tensors
        g = g.contiguous()
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        n, h, w, c = g.shape
        dx = torch.empty((n, h, w, c), dtype=torch.float32, device=g.device)
        C.backend().mg_masked_mean_fill(_p(g), _p(ltag), _p(lref), _p(lref), _dt(g), n, h * w, c, _p(dx), _stream(g))
        return (dx if ctx.xdtype == torch.float32 else dx.to(ctx.xdtype)), None, None


def masked_mean_fill(x: torch.Tensor, lref: torch.Tensor, ltag: torch.Tensor) -> torch.Tensor:
    """ImageEncoder3's tail (encoder.py:211-220): per sample, the mean of x over the region lref (area clamped to >= 1) written over the
    region ltag: fp32 [N, H, W, C].  x NHWC; lref / ltag fp32 with one value per pixel."""
    lref = lref.detach().float().reshape(x.shape[0], -1).contiguous()
    ltag = ltag.detach().float().reshape(x.shape[0], -1).contiguous()
    if x.shape[-1] % 4 or lref.shape[1] * x.shape[-1] != x[0].numel():
        raise ValueError("masked_mean_fill: one weight per pixel and C % 4 == 0 expected")
    return _MaskedMeanFillFn.apply(x, lref, ltag)


class _OrientTailFn(torch.autograd.Function):
    """The tail of L1OLoss behind an arg-max: `fwd` / `bwd` name the two entry points (of one signature), n_out / n_ws are the lengths
    in floats of the result and partial-sum buffers they write."""

    @staticmethod
    def forward(ctx, fwd, bwd, n_out, n_ws, conf_raw, idx, label, hair):
        n, h, w = conf_raw.shape
        out = torch.empty(n_out, dtype=torch.float32, device=conf_raw.device)
        ws = torch.empty(n_ws, dtype=torch.float32, device=conf_raw.device)
        hp, hs = _plane_args(hair)
        getattr(C.backend(), fwd)(_p(conf_raw), _p(idx), _p(label), label.shape[1], label.stride(0), hp, hs, n, h * w, _p(out), _p(ws),
                                  _stream(conf_raw))
        ctx.save_for_backward(conf_raw, idx, label, hair, out)
        ctx.bwd = bwd
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_orient, g_conf):
        conf_raw, idx, label, hair, out = ctx.saved_tensors
        if g_orient is None and g_conf is None:
            return (None,) * 8
        n, h, w = conf_raw.shape
        g_orient, g_conf = _f32_grads(g_orient, g_conf)
        hp, hs = _plane_args(hair)
        d = torch.empty_like(conf_raw)
        getattr(C.backend(), ctx.bwd)(_p(conf_raw), _p(idx), _p(label), label.shape[1], label.stride(0), hp, hs, _p(g_orient), _p(g_conf),
                                      _p(out), n, h * w, _p(d), _stream(conf_raw))
        return (None,) * 4 + (d, None, None, None)


def _orient_tail(who, fwd, bwd, n_out, n_ws, conf_raw, idx, label, hair):
    return _OrientTailFn.apply(fwd, bwd, n_out, n_ws, conf_raw.contiguous(), idx.contiguous(), _f32_dense(label),
                               _f32_plane(hair, who + ": the hair plane", conf_raw.shape))


def orient_loss(conf_raw: torch.Tensor, idx: torch.Tensor, label: torch.Tensor, hair: torch.Tensor):
    """(orientation L1, confidence loss) of L1OLoss behind the Gabor arg-max (loss.py:352-385): conf_raw fp32 [N,H,W], idx u8 [N,H,W],
    label fp32 [N, 1 or 2, H, W] (0..255 angle map or (sin 2t, cos 2t) planes), hair fp32 [N, H, W] view.  Two launches forward, one backward."""
    return _orient_tail("orient_loss", "mg_orient_loss_fwd", "mg_orient_loss_bwd", ORIENT_LOSS_TERMS, ORIENT_LOSS_TERMS * ORIENT_LOSS_BLOCKS,
                        conf_raw, idx, label, hair)


ORIENT_DOG_BLOCKS, ORIENT_DOG_WS_ROWS, ORIENT_DOG_OUT = 1024, 7, 8       # MGL_ORIENT_DOG_* (include/michigan_hip/losses/orient_dog.h)


def orient_loss_dog(conf_raw: torch.Tensor, idx: torch.Tensor, label: torch.Tensor, hair: torch.Tensor):
    """(orientation L1, confidence loss) of L1OLoss behind the arg-max under the difference-of-Gaussians bank (loss.py:320-349 and the
    DoG branch of 352-385): conf_raw fp32 [N,H,W], idx u8 [N,H,W], label fp32 [N, 1 or 2, H, W] (0..255 angle map or (sin 2t, cos 2t)
    planes), hair fp32 [N, H, W] view.  The confidence is conf_raw * hair divided by its maximum over the WHOLE tensor -- across the
    samples of the batch; with no positive response under the hair anywhere both losses are NaN, as in the reference.  Under one process
    per GPU that maximum is the rank's own, which is what a replica of the reference's DataParallel computes: no collective is needed.
    Three launches forward, one backward, no read-back."""
    return _orient_tail("orient_loss_dog", "mgl_orient_dog_fwd", "mgl_orient_dog_bwd", ORIENT_DOG_OUT, ORIENT_DOG_WS_ROWS * ORIENT_DOG_BLOCKS,
                        conf_raw, idx, label, hair)


COLOR_LAB, COLOR_RGB, COLOR_BACKGROUND = 1, 2, 4      # `flags` bits of mg_color_loss_*
LAB_TABLE_BINS, HAIR_LAB_BALANCED_STATS = 256, 8      # MGC_TABLE_BINS, MGC_HAIR_STATS (include/michigan_hip/losses/lab_balance.h)


def lab_weight_table(counts, th: float = 10.0, device=None) -> torch.Tensor:
    """The weight table S of --balance_Lab, fp32 [256, 256] (rows index a, columns index b), from the histogram of hair colours over the
    a/b plane that `--weight_dir` names (cal_weight, loss.py:486-492): the counts are cast to fp32 FIRST, then in fp32 zeros become 1,
    w = max(w) / w and w = min(w, th).  Row 255 and column 255 are 0: the reference samples its weights with grid_sample(mode='nearest')
    under today's default align_corners=False, which maps bin 255 to position 255.5, rounds to 256 and reads the zero padding (the torch
    the reference was written for, align_corners=True, read w[255][..] there; this package follows the reference as it runs today).
    Refuses a shape other than 256 x 256, non-finite or negative counts and th <= 0."""
    import numpy as np
    c = counts.detach().cpu() if torch.is_tensor(counts) else torch.from_numpy(np.ascontiguousarray(counts))
    if tuple(c.shape) != (LAB_TABLE_BINS, LAB_TABLE_BINS):
        raise ValueError(f"lab_weight_table: the histogram has to be 256 x 256, got {tuple(c.shape)}")
    if c.dtype == torch.bool or c.is_complex():
        raise ValueError("lab_weight_table: the histogram has to hold counts")
    th = float(th)
    if not (th > 0 and math.isfinite(th)):
        raise ValueError(f"lab_weight_table: the cap Lab_weight_th has to be positive and finite, got {th}")
    w = c.to(torch.float32)
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("lab_weight_table: the counts have to be finite and not negative")
    w[w == 0] = 1
    w = w.max() / w
    w[w > th] = th
    w[LAB_TABLE_BINS - 1, :] = 0
    w[:, LAB_TABLE_BINS - 1] = 0
    w = w.contiguous()
    return w.to(device) if device is not None else w


def _lab_table(table: torch.Tensor, who: str, like: torch.Tensor) -> torch.Tensor:
    """The operand check of a weight table: fp32 [256, 256], dense, on the image's device; any VALUES (the kernels read what is there)."""
    if not torch.is_tensor(table) or table.dtype != torch.float32 or tuple(table.shape) != (LAB_TABLE_BINS, LAB_TABLE_BINS):
        raise ValueError(f"{who}: the weight table has to be an fp32 [256, 256] tensor (ops.lab_weight_table)")
    if table.device != like.device:
        raise ValueError(f"{who}: the weight table is on {table.device}, the image on {like.device}")
    return table.detach().contiguous()


class _ColorLossFn(torch.autograd.Function):
    """table None: mg_color_loss_*; a table: mgc_color_loss_balanced_* with (hair, table) behind the background plane."""

    @staticmethod
    def forward(ctx, img, real, back, flags, hair=None, table=None):
        img = _nhwc(img)
        n, h, w, c = img.shape
        out = torch.empty(COLOR_LOSS_TERMS, dtype=torch.float32, device=img.device)
        ws = torch.empty(COLOR_LOSS_TERMS * COLOR_LOSS_BLOCKS, dtype=torch.float32, device=img.device)
        bp, bs = _plane_args(back)
        if table is None:
            C.backend().mg_color_loss_fwd(_p(img), _p(real), real.stride(0), bp, bs, _dt(img), n, h, w, c, flags, _p(out), _p(ws), _stream(img))
        else:
            hp, hs = _plane_args(hair)
            C.backend().mgc_color_loss_balanced_fwd(_p(img), _p(real), real.stride(0), bp, bs, hp, hs, _p(table), _dt(img), n, h, w, c, flags,
                                                    _p(out), _p(ws), _stream(img))
        ctx.save_for_backward(img, real, back, hair, table)
        ctx.flags = flags
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_lab, g_rgb, g_back):
        img, real, back, hair, table = ctx.saved_tensors
        if g_lab is None and g_rgb is None and g_back is None:
            return (None,) * 6
        n, h, w, c = img.shape
        g_lab, g_rgb, g_back = _f32_grads(g_lab, g_rgb, g_back)
        bp, bs = _plane_args(back)
        d = torch.empty_like(img)
        if table is None:
            C.backend().mg_color_loss_bwd(_p(img), _p(real), real.stride(0), bp, bs, _p(g_lab), _p(g_rgb), _p(g_back), _dt(img), n, h, w, c,
                                          ctx.flags, _p(d), _stream(img))
        else:
            hp, hs = _plane_args(hair)
            C.backend().mgc_color_loss_balanced_bwd(_p(img), _p(real), real.stride(0), bp, bs, hp, hs, _p(table), _p(g_lab), _p(g_rgb), _p(g_back),
                                                    _dt(img), n, h, w, c, ctx.flags, _p(d), _stream(img))
        return (d,) + (None,) * 5


def color_losses(fake: torch.Tensor, real: torch.Tensor, back: Optional[torch.Tensor], flags: int, hair: Optional[torch.Tensor] = None,
                 table: Optional[torch.Tensor] = None):
    """(lab, rgb, background) of the generator objective (LabColorLoss loss.py:403-532, nn.L1Loss, RGBBackgroundL1Loss
    loss.py:388-400) in one pass: fake NHWC [N, H, W, C >= 3] bf16 / fp32 with RGB in channels 0..2 (`net_output.permute(0, 2, 3, 1)` is
    zero-copy), real NCHW [N, 3, H, W], back fp32 [N, H, W] view (channel 0 of the one-hot label; None unless COLOR_BACKGROUND is set).
    `flags`: COLOR_LAB | COLOR_RGB | COLOR_BACKGROUND; a term not selected is 0 and costs nothing.  Three fp32 scalars (views of one
    tensor), gradient to `fake` only.  Two launches forward, one backward.
    `table` (lab_weight_table; any fp32 [256, 256] is read as it stands) selects the --balance_Lab weighting of the Lab term: a pixel's
    |da| + |db| counts w = table[bin a][bin b] * hair times, once where that is 0, with the bins taken of the TARGET pixel's colour and
    `hair` the fp32 [N, H, W] view whose value multiplies (channel 1 of the one-hot label).  It needs `hair` and COLOR_LAB; the other two
    terms ride along unchanged, the launches stay two and one.  Without a table the call is the unbalanced one, launch for launch."""
    flags = int(flags)
    if not 1 <= flags <= 7:
        raise ValueError("color_losses: flags must select at least one of COLOR_LAB, COLOR_RGB, COLOR_BACKGROUND")
    if fake.dim() != 4 or real.dim() != 4 or real.shape[1] != 3 or fake.shape[-1] < 3 or \
            (fake.shape[0], fake.shape[1], fake.shape[2]) != (real.shape[0], real.shape[2], real.shape[3]):
        raise ValueError(f"color_losses: NHWC image {tuple(fake.shape)} does not match the NCHW target {tuple(real.shape)}")
    back = _f32_plane(back, "color_losses: the background plane", fake.shape[:3]) if flags & COLOR_BACKGROUND else None
    if table is None:
        if hair is not None:
            raise ValueError("color_losses: a hair plane without a weight table: the unbalanced Lab term does not read one")
        return _ColorLossFn.apply(fake, _f32_dense(real), back, flags, None, None)
    if not flags & COLOR_LAB:
        raise ValueError("color_losses: a weight table needs COLOR_LAB: it weights the Lab term")
    table = _lab_table(table, "color_losses", fake)
    hair = _f32_plane(hair, "color_losses: the hair plane", fake.shape[:3])
    return _ColorLossFn.apply(fake, _f32_dense(real), back, flags, hair, table)


HAIR_LAB, HAIR_BACKGROUND = 1, 2                      # `flags` bits of mg_hair_lab_*


class _HairLabLossFn(torch.autograd.Function):
    """table None: mg_hair_lab_*; a table: mgc_hair_lab_balanced_* (the table behind the background plane, a wider `stats` row)."""

    @staticmethod
    def forward(ctx, img, ref, hair_tag, hair_ref, tgt, back, flags, table=None):
        img = _nhwc(img)
        n, h, w, c = img.shape
        out = torch.empty(2, dtype=torch.float32, device=img.device)
        row = 4 if table is None else HAIR_LAB_BALANCED_STATS
        stats = torch.empty(row * n, dtype=torch.float32, device=img.device) if flags & HAIR_LAB else None
        ws = torch.empty(HAIR_LAB_TERMS * max(HAIR_LAB_BLOCKS, n), dtype=torch.float32, device=img.device)
        (fp, fs), (rp, rs), (bp, bs) = _plane_args(hair_tag), _plane_args(hair_ref), _plane_args(back)
        if table is None:
            C.backend().mg_hair_lab_fwd(_p(img), _p(ref), ref.stride(0) if ref is not None else 0, fp, fs, rp, rs,
                                        _p(tgt), tgt.stride(0) if tgt is not None else 0, bp, bs, _dt(img), n, h, w, c, flags,
                                        _p(out), _p(stats), _p(ws), _stream(img))
        else:
            C.backend().mgc_hair_lab_balanced_fwd(_p(img), _p(ref), ref.stride(0) if ref is not None else 0, fp, fs, rp, rs,
                                                  _p(tgt), tgt.stride(0) if tgt is not None else 0, bp, bs, _p(table), _dt(img), n, h, w, c, flags,
                                                  _p(out), _p(stats), _p(ws), _stream(img))
        ctx.save_for_backward(img, hair_tag, tgt, back, stats)
        ctx.flags, ctx.balanced = flags, table is not None
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_hair, g_back):
        img, hair_tag, tgt, back, stats = ctx.saved_tensors
        if g_hair is None and g_back is None:
            return (None,) * 8
        n, h, w, c = img.shape
        g_hair, g_back = _f32_grads(g_hair, g_back)
        (fp, fs), (bp, bs) = _plane_args(hair_tag), _plane_args(back)
        d = torch.empty_like(img)
        bwd = C.backend().mgc_hair_lab_balanced_bwd if ctx.balanced else C.backend().mg_hair_lab_bwd
        bwd(_p(img), fp, fs, _p(tgt), tgt.stride(0) if tgt is not None else 0, bp, bs, _p(stats),
            _p(g_hair), _p(g_back), _dt(img), n, h, w, c, ctx.flags, _p(d), _stream(img))
        return (d,) + (None,) * 7


def hair_lab_losses(fake: torch.Tensor, image_ref: Optional[torch.Tensor], hair_tag: Optional[torch.Tensor],
                    hair_ref: Optional[torch.Tensor], image_tag: Optional[torch.Tensor] = None, back: Optional[torch.Tensor] = None,
                    flags: int = HAIR_LAB, table: Optional[torch.Tensor] = None):
    """(hairAvgLab, background) of the unpaired stage's generator objective (HairAvgLabLoss loss.py:534-621,
    RGBBackgroundL1Loss loss.py:388-400; pix2pix_model.py:352-363) in one pass: fake NHWC [N, H, W, C >= 3] bf16 / fp32 with RGB in
    channels 0..2, image_ref / image_tag NCHW [N, 3, H, W], hair_tag / hair_ref / back fp32 [N, H, W] views (channel 1 of the tag label,
    channel 1 of the reference label, channel 0 of the tag label).  `flags`: HAIR_LAB | HAIR_BACKGROUND; a term not selected is 0, costs
    nothing and its operands may be None.  Two fp32 scalars (views of one tensor), gradient to `fake` only.  Two launches forward, one
    backward.
    `table` (lab_weight_table; any fp32 [256, 256] is read as it stands) selects the --balance_Lab weighting: sample n's |da| + |db|
    counts w_n = table[bin a][bin b] times, the bins taken of the REFERENCE image's mean hair colour; a zero of the table gives weight
    0 (no replacement here, unlike color_losses).  It needs HAIR_LAB.  Without a table the call is the unbalanced one."""
    flags = int(flags)
    if not 1 <= flags <= 3:
        raise ValueError("hair_lab_losses: flags must select at least one of HAIR_LAB, HAIR_BACKGROUND")
    if fake.dim() != 4 or fake.shape[-1] < 3:
        raise ValueError(f"hair_lab_losses: expected an NHWC image with at least 3 channels, got {tuple(fake.shape)}")
    n, h, w = fake.shape[0], fake.shape[1], fake.shape[2]
    if table is not None:
        if not flags & HAIR_LAB:
            raise ValueError("hair_lab_losses: a weight table needs HAIR_LAB: it weights that term")
        table = _lab_table(table, "hair_lab_losses", fake)

    def image(t, name):
        if t is None:
            raise ValueError("hair_lab_losses: %s is needed for the selected terms" % name)
        if t.dim() != 4 or tuple(t.shape) != (n, 3, h, w):
            raise ValueError(f"hair_lab_losses: NHWC image {tuple(fake.shape)} does not match the NCHW {name} {tuple(t.shape)}")
        return _f32_dense(t)

    if flags & HAIR_LAB:
        image_ref = image(image_ref, "image_ref")
        hair_tag = _f32_plane(hair_tag, "hair_lab_losses: the tag hair plane", (n, h, w))
        hair_ref = _f32_plane(hair_ref, "hair_lab_losses: the reference hair plane", (n, h, w))
    else:
        image_ref = hair_tag = hair_ref = None
    if flags & HAIR_BACKGROUND:
        image_tag, back = image(image_tag, "image_tag"), _f32_plane(back, "hair_lab_losses: the background plane", (n, h, w))
    else:
        image_tag = back = None
    return _HairLabLossFn.apply(fake, image_ref, hair_tag, hair_ref, image_tag, back, flags, table)


FEAT_STYLE, FEAT_CONTENT = 1, 2                       # `flags` bits of mg_feat_moment_loss_*


def _feat_desc(x, s, t, masks, flags, out=None, coef=None, ws=None):
    d = C.FeatMomentDesc()
    n, h, w, c = x.shape
    d.x, d.s, d.t = x.data_ptr(), (s.data_ptr() if s is not None else None), (t.data_ptr() if t is not None else None)
    for name, m in zip(("mask_x", "mask_s", "mask_t"), masks):
        ptr, stride = _plane_args(m)
        setattr(d, name, ptr)
        setattr(d, name + "_nstride", stride)
    d.P, d.dtype, d.N, d.C, d.flags = h * w, _dt(x), n, c, flags
    d.out, d.coef, d.ws = (None if out is None else out.data_ptr()), coef.data_ptr(), (None if ws is None else ws.data_ptr())
    return d


class _FeatMomentLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s, t, mask_x, mask_s, mask_t, flags):
        x = _nhwc(x)
        n, h, w, c = x.shape
        out = torch.empty(2, dtype=torch.float32, device=x.device)
        coef = torch.empty(4 * n * c, dtype=torch.float32, device=x.device)
        ws = torch.empty(int(C.backend().mg_feat_moment_workspace(n, h * w, c)), dtype=torch.uint8, device=x.device)
        C.backend().mg_feat_moment_loss_fwd(_feat_desc(x, s, t, (mask_x, mask_s, mask_t), flags, out, coef, ws), _stream(x))
        ctx.save_for_backward(x, t, mask_x, mask_t, coef)
        ctx.flags = flags
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_style, g_content):
        x, t, mask_x, mask_t, coef = ctx.saved_tensors
        if g_style is None and g_content is None:
            return (None,) * 7
        g_style, g_content = _f32_grads(g_style, g_content)
        d = torch.empty_like(x)
        C.backend().mg_feat_moment_loss_bwd(_feat_desc(x, None, t, (mask_x, None, mask_t), ctx.flags, coef=coef), _p(g_style), _p(g_content),
                                            _p(d), _stream(x))
        return (d,) + (None,) * 6


def feat_moment_loss(x: torch.Tensor, s: Optional[torch.Tensor], t: Optional[torch.Tensor] = None, mask_x: Optional[torch.Tensor] = None,
                     mask_s: Optional[torch.Tensor] = None, mask_t: Optional[torch.Tensor] = None, flags: int = FEAT_STYLE):
    """(style, content) of StyleContentLoss on ONE VGG tap (loss.py:624-694): x the fake features (gets the gradient), s the style
    features, t the content features -- NCHW [N, C, h, w] bf16 / fp32; the towers' NCHW views of NHWC storage are read in place, a plain
    contiguous NCHW tensor costs one copy.  style = MSE of the per-(sample, channel) means + MSE of the standard deviations of x and s,
    content = MSE(x, t).  mask_x / mask_s / mask_t: fp32 [N, h, w] planes at the features' resolution (`remove_background`: x under
    mask_x, s under mask_s, content under mask_t; the mask VALUE multiplies); None is the unmasked form, mask_x and mask_s come together.
    `flags`: FEAT_STYLE | FEAT_CONTENT; a term not selected is 0, costs nothing and its operands may be None.  Two fp32 scalars (views
    of one tensor), gradient to x only.  Two launches forward, one backward."""
    flags = int(flags)
    if not 1 <= flags <= 3:
        raise ValueError("feat_moment_loss: flags must select at least one of FEAT_STYLE, FEAT_CONTENT")
    if x.dim() != 4 or x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"feat_moment_loss: expected NCHW bf16 / fp32 features, got {tuple(x.shape)} {x.dtype}")
    n, c, h, w = x.shape
    if c % (8 if x.dtype == torch.bfloat16 else 4):
        raise ValueError(f"feat_moment_loss: C = {c} is not a multiple of {8 if x.dtype == torch.bfloat16 else 4} (16 bytes of channels per lane)")

    def feats(f, name):
        if f is None:
            raise ValueError("feat_moment_loss: %s is needed for the selected terms" % name)
        if tuple(f.shape) != (n, c, h, w):
            raise ValueError(f"feat_moment_loss: {name} {tuple(f.shape)} does not match the fake features {tuple(x.shape)}")
        f = f.detach()
        return _nhwc((f if f.dtype == x.dtype else f.to(x.dtype)).permute(0, 2, 3, 1))

    if flags & FEAT_STYLE:
        s = feats(s, "the style features")
        if (mask_x is None) != (mask_s is None):
            raise ValueError("feat_moment_loss: mask_x and mask_s come together")
        if mask_x is not None:
            mask_x, mask_s = _f32_plane(mask_x, "feat_moment_loss: mask_x", (n, h, w)), _f32_plane(mask_s, "feat_moment_loss: mask_s", (n, h, w))
        elif h * w < 2:
            raise ValueError("feat_moment_loss: the unbiased variance needs at least two pixels")
    else:
        s = mask_x = mask_s = None
    if flags & FEAT_CONTENT:
        t = feats(t, "the content features")
        mask_t = _f32_plane(mask_t, "feat_moment_loss: mask_t", (n, h, w)) if mask_t is not None else None
    else:
        t = mask_t = None
    return _FeatMomentLossFn.apply(x.permute(0, 2, 3, 1), s, t, mask_x, mask_s, mask_t, flags)


class _WeightedSumFn(torch.autograd.Function):
    """sum_k w_k * v_k of K scalar tensors as THREE launches forward (stack, mul, sum) and ONE backward (g * w), whatever K: the loss
    modules used to chain `total = total + val * w` -- 2 launches forward and 2 backward per term, ~100 five-microsecond
    launches per training step for the feature-matching / VGG / multi-scale GAN sums (tools/count_launches.py)."""

    @staticmethod
    def forward(ctx, wvec, *vals):
        stacked = torch.stack([v.reshape(()) for v in vals])
        if stacked.dtype != torch.float32:
            stacked = stacked.float()
        ctx.save_for_backward(wvec)
        ctx.dtypes = [v.dtype for v in vals]
        ctx.shapes = [v.shape for v in vals]
        return (stacked * wvec).sum()

    @staticmethod
    def backward(ctx, g):
        (wvec,) = ctx.saved_tensors
        gv = g * wvec                                             # one launch; the per-term gradients are views of it
        return (None,) + tuple(gv[k].reshape(sh) if dt == gv.dtype else gv[k].reshape(sh).to(dt) for k, (dt, sh) in enumerate(zip(ctx.dtypes, ctx.shapes)))


_WSUM_WEIGHTS = {}


def weighted_sum(vals, weights=None) -> torch.Tensor:
    """sum_k weights[k] * vals[k] for scalar (0-d / 1-element) tensors; weights default to 1.  fp32 result."""
    vals = list(vals)
    if len(vals) == 1 and (weights is None or float(weights[0]) == 1.0):
        return vals[0].reshape(()).float() if vals[0].dtype != torch.float32 else vals[0].reshape(())
    w = tuple(1.0 for _ in vals) if weights is None else tuple(float(x) for x in weights)
    key = (w, vals[0].device)
    wvec = _WSUM_WEIGHTS.get(key)
    if wvec is None:
        if len(_WSUM_WEIGHTS) > 256:
            _WSUM_WEIGHTS.clear()
        wvec = _WSUM_WEIGHTS[key] = torch.tensor(w, dtype=torch.float32, device=vals[0].device)
    return _WeightedSumFn.apply(wvec, *vals)


class _HingeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, mode):
        n = x.numel()
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        C.backend().mg_hinge_fwd(_p(x), _p(weight), _dt(x), n, mode, _p(out), _stream(x))
        ctx.save_for_backward(x, weight)
        ctx.mode = mode
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        (g,) = _f32_grads(g)
        dx = torch.empty_like(x)
        C.backend().mg_hinge_bwd(_p(x), _p(weight), _p(g), _dt(x), x.numel(), ctx.mode, _p(dx), _stream(x))
        return dx, None, None


HINGE_G, HINGE_D_REAL, HINGE_D_FAKE = 0, 1, 2


def hinge_loss(logits: torch.Tensor, weight: Optional[torch.Tensor], mode: int) -> torch.Tensor:
    """-mean(f(logits) * weight) of a patch discriminator's logit map (any shape, dense), one launch forward and one
    backward: f = x (HINGE_G), min(x - 1, 0) (HINGE_D_REAL), min(-x - 1, 0) (HINGE_D_FAKE)  (loss.py:96-111)."""
    x = logits if logits.is_contiguous() else _dense_view(logits)
    if weight is not None and (weight.numel() != x.numel() or weight.dtype != torch.float32):
        raise ValueError("hinge_loss: weight must be fp32 with one value per logit")
    return _HingeFn.apply(x, weight.contiguous() if weight is not None else None, mode)


def wide_edge_weight(label: torch.Tensor, h: int, w: int, wide: float, th: float = 0.06) -> torch.Tensor:
    """GANLoss.get_weight_mask (loss.py:60-89) for one logit resolution: label [N,1,Hl,Wl] in {0,1} -> fp32 [N,1,h,w]."""
    label = _f32_dense(label)
    n, c, hl, wl = label.shape
    if c != 1:
        raise ValueError("wide_edge_weight: the label must have one channel")
    k = max(1, int(h * th))
    out = torch.empty((n, 1, h, w), dtype=torch.float32, device=label.device)
    C.backend().mg_wide_edge_weight(_p(label), n, hl, wl, h, w, k, float(wide), _p(out), _stream(label))
    return out


def _rotated_grid(theta: torch.Tensor):
    """(x', y') of the 17x17 tap grid turned by each angle of `theta` (fp32 [K]): two fp32 [K, 17, 17]; x runs along rows."""
    r = torch.arange(-8, 9, dtype=torch.float32)
    x = r.view(-1, 1).expand(17, 17)
    y = r.view(1, -1).expand(17, 17)
    theta = theta.view(-1, 1, 1)
    return x * torch.cos(theta) + y * torch.sin(theta), -x * torch.sin(theta) + y * torch.cos(theta)


def gabor_bank(device=None) -> torch.Tensor:
    """The 32 oriented 17x17 Gabor kernels of the orientation loss, fp32 [32, 17, 17]
    (loss.py:215-243: sigma_x 2, sigma_y 3, lambda 4, psi 0, theta_k = pi k / 32; x runs along rows)."""
    import math
    xt, yt = _rotated_grid(math.pi * torch.arange(32, dtype=torch.float32) / 32)
    gb = torch.exp(-0.5 * (xt ** 2 / 2.0 ** 2 + yt ** 2 / 3.0 ** 2)) * torch.cos(2 * math.pi / 4.0 * xt)
    return gb.contiguous().to(device) if device is not None else gb.contiguous()


class _GaborMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, bank):
        img = _nhwc(img)
        n, h, w, c = img.shape
        conf = torch.empty((n, h, w), dtype=torch.float32, device=img.device)
        idx = torch.empty((n, h, w), dtype=torch.uint8, device=img.device)
        C.backend().mg_gabor_argmax_fwd(_p(img), _p(bank), _p(conf), _p(idx), _dt(img), n, h, w, c, _stream(img))
        ctx.save_for_backward(conf, idx, bank)
        ctx.meta = (img.dtype, c)
        ctx.mark_non_differentiable(idx)
        return conf, idx

    @staticmethod
    def backward(ctx, dconf, _didx):
        conf, idx, bank = ctx.saved_tensors
        dtype, c = ctx.meta
        n, h, w = conf.shape
        g = (dconf.float() * (conf > 0)).contiguous()                 # the clamp at 0 blocks the gradient
        dimg = torch.empty((n, h, w, c), dtype=dtype, device=conf.device)
        C.backend().mg_gabor_argmax_bwd(_p(g), _p(idx), _p(bank), _p(dimg), _dtype_code(dtype),
                                        n, h, w, c, _stream(conf))
        return dimg, None


def gabor_argmax(img_nhwc: torch.Tensor, bank: torch.Tensor):
    """(max non-negative response, first arg-max) of the 32-filter Gabor bank on the gray image; differentiable
    w.r.t. the image through the winning filter (what autograd does for the reference's max over channels)."""
    return _GaborMaxFn.apply(img_nhwc, bank)


def dog_bank(device=None) -> torch.Tensor:
    """The 32 oriented 17x17 difference-of-Gaussians kernels of dense orientation extraction, fp32 [32, 17, 17]
    (cal_orientation.py:18-44: sigma_h 1, sigma_l 2, sigma_y 2, theta_k = pi k / 32, normalised by 1/sigma_h - 1/sigma_l;
    x runs along rows).  With this bank mg_gabor_argmax_fwd is orient.calOrientation (cal_orientation.py:60-80)."""
    import math
    xt, yt = _rotated_grid(torch.tensor([math.pi * k / 32 for k in range(32)], dtype=torch.float32))    # rounded once, as the reference's
    gb = (torch.exp(-0.5 * (xt ** 2 / 1.0 ** 2 + yt ** 2 / 2.0 ** 2)) / 1.0
          - torch.exp(-0.5 * (xt ** 2 / 2.0 ** 2 + yt ** 2 / 2.0 ** 2)) / 2.0) / (1.0 / 1.0 - 1.0 / 2.0)
    return gb.contiguous().to(device) if device is not None else gb.contiguous()


def orient_trig_table() -> torch.Tensor:
    """fp32 [32, 2]: (cos, sin) of the angle filter index k stands for in the flow field, k * pi / 31 * 2, evaluated in fp32 in the
    reference's order of operations (cal_orientation.py:101-104; the 31 is the reference's own (sic): the bank steps by pi / 32)."""
    import math
    a = torch.arange(32, dtype=torch.float32) * math.pi / 31 * 2
    return torch.stack([torch.cos(a), torch.sin(a)], dim=1).contiguous()


ORIENT_RADIUS = 16                      # MG_ORIENT_RADIUS (include/michigan_hip/preprocess/dense_orient.h)
ORIENT_MAX_SIGMA = 4.0                  # the 33-tap window is cv2's for sigma = 4; a larger sigma would be truncated below 4 sigma


def gaussian_taps(sigma: float) -> torch.Tensor:
    """fp32 [33]: exp(-x^2 / (2 sigma^2)) for x = -16 .. 16, normalised in float64 -- the window of cv2.GaussianBlur(src_f32, (0, 0), 4)
    (ksize = round(sigma * 4 * 2 + 1) | 1 = 33 for a float source).  0 < sigma <= 4; below 4 the window reaches further than cv2's."""
    if not 0.0 < float(sigma) <= ORIENT_MAX_SIGMA:
        raise ValueError(f"gaussian_taps: sigma must be in (0, {ORIENT_MAX_SIGMA}], got {sigma}")
    x = torch.arange(-ORIENT_RADIUS, ORIENT_RADIUS + 1, dtype=torch.float64)
    t = torch.exp(-x * x / (2.0 * float(sigma) ** 2))
    return (t / t.sum()).float().contiguous()


_DEVICE_TABLES = {}


def _device_table(device, key, make):
    """make(): a small constant table the kernels read, built once per (device, key) and kept."""
    key = (str(device),) + key
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = make()
    return _DEVICE_TABLES[key]


def _check_nhw(who: str, shape):
    """The kernels over [N, H, W] planes index with 32-bit integers."""
    n, h, w = shape
    if n < 1 or h < 1 or w < 1 or n * h * w >= 1 << 31:
        raise ValueError(f"{who}: bad geometry {tuple(shape)} (N H W must be in [1, 2^31))")


def orient_smooth(conf: torch.Tensor, idx: torch.Tensor, mask: torch.Tensor, sigma: float = 4.0, want_angle: bool = False):
    """cal_orientation.py:101-109 in one launch (mg_orient_smooth): conf fp32 / idx u8 [N,H,W] of gabor_argmax under dog_bank, mask u8
    [N,H,W] (non-zero = hair) -> the uint8 orientation map [N,H,W] (and the fp32 angle in [0, pi] when want_angle)."""
    if conf.dim() != 3 or conf.dtype != torch.float32 or idx.dtype != torch.uint8 or mask.dtype != torch.uint8:
        raise ValueError("orient_smooth: conf must be fp32 [N,H,W], idx and mask uint8")
    if idx.shape != conf.shape or mask.shape != conf.shape:
        raise ValueError(f"orient_smooth: shapes differ: conf {tuple(conf.shape)}, idx {tuple(idx.shape)}, mask {tuple(mask.shape)}")
    n, h, w = conf.shape
    if n < 1 or h <= ORIENT_RADIUS or w <= ORIENT_RADIUS:
        raise ValueError(f"orient_smooth: H and W must be at least {ORIENT_RADIUS + 1} (one reflection reaches every tap), got {h} x {w}")
    trig, taps = _device_table(conf.device, ("orient", float(sigma)), lambda: (orient_trig_table().to(conf.device), gaussian_taps(sigma).to(conf.device)))
    conf, idx, mask = conf.contiguous(), idx.contiguous(), mask.contiguous()
    out = torch.empty((n, h, w), dtype=torch.uint8, device=conf.device)
    angle = torch.empty((n, h, w), dtype=torch.float32, device=conf.device) if want_angle else None
    C.backend().mg_orient_smooth(_p(conf), _p(idx), _p(mask), _p(trig), _p(taps), _p(out), _p(angle), n, h, w, _stream(conf))
    return (out, angle) if want_angle else out


def stroke_rgb_table() -> torch.Tensor:
    """u8 [32, 3]: the colour the stroke picture gives filter index k (cal_orient_stroke.py:112-115, 123-149): a = fp32(k) * pi / 32,
    (R, G, B) = uint8((v + 1) / 2 * 255) for v = (cos 2a, sin 2a, 0), every step in fp32 in the reference's order."""
    import math
    a = torch.arange(32, dtype=torch.float32) * math.pi / 32
    v = torch.stack([torch.cos(2 * a), torch.sin(2 * a), torch.zeros(32)], dim=1)
    return ((v + 1) / 2.0 * 255.0).to(torch.uint8).contiguous()        # np.uint8 of a value in [0, 255]: truncation


def stroke_orient(stroke: torch.Tensor, want_idx: bool = False, want_conf: bool = False, bank: Optional[torch.Tensor] = None):
    """orient().stroke_to_orient (cal_orient_stroke.py:85-121, 133-149) in one launch (mg_stroke_orient): stroke u8 [N,H,W], non-zero =
    stroke -> the RGB-coded orientation picture u8 [N,H,W,3], black outside the stroke (and the filter index u8 / the confidence
    fp32 [N,H,W] when asked for).  Tiles without a stroke pixel are not filtered.  `bank`: another fp32 [32,17,17] bank than dog_bank()."""
    if stroke.dim() != 3 or stroke.dtype != torch.uint8:
        raise ValueError(f"stroke_orient: stroke must be uint8 [N,H,W], got {stroke.dtype} {tuple(stroke.shape)}")
    n, h, w = stroke.shape
    _check_nhw("stroke_orient", stroke.shape)
    dog, table = _device_table(stroke.device, ("stroke",), lambda: (dog_bank().to(stroke.device), stroke_rgb_table().to(stroke.device)))
    if bank is None:
        bank = dog
    elif bank.dtype != torch.float32 or tuple(bank.shape) != (32, 17, 17) or bank.device != stroke.device:
        raise ValueError(f"stroke_orient: bank must be fp32 [32,17,17] on {stroke.device} (bf16 moves the arg-max), got {bank.dtype} {tuple(bank.shape)} on {bank.device}")
    bank = bank.contiguous()
    stroke = stroke.contiguous()
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=stroke.device)
    idx = torch.empty((n, h, w), dtype=torch.uint8, device=stroke.device) if want_idx else None
    conf = torch.empty((n, h, w), dtype=torch.float32, device=stroke.device) if want_conf else None
    C.backend().mg_stroke_orient(_p(stroke), _p(bank), _p(table), _p(rgb), _p(idx), _p(conf), n, h, w, _stream(stroke))
    extra = tuple(t for t in (idx, conf) if t is not None)
    return (rgb,) + extra if extra else rgb


BRUSH_MAX_THICKNESS, BRUSH_MAX_COORD, MORPH_MAX_K = 255, 8191, 64          # include/michigan_hip/editing/mask_edit.h
MORPH_DILATE, MORPH_ERODE = 0, 1


def brush_u8(canvas: torch.Tensor, segs: torch.Tensor) -> torch.Tensor:
    """demo.py:431-435 (make_mask) in one launch (mge_brush_u8): canvas u8 [N,H,W], contiguous, painted IN PLACE and returned; segs int32
    [S,8] on the canvas' device = (sample, x0, y0, x1, y1, thickness, value, 0), applied in order with the integer capsule rule of
    include/michigan_hip/editing/mask_edit.h (the package's own brush, not cv2.line's polygon).  CALLER'S OBLIGATION: every row
    of `segs` is inside the header's ranges (0 <= sample < N, |x|, |y| <= 8191, 1 <= thickness <= 255, 0 <= value <= 255).  Nothing
    here reads the device list back, so a row outside them does NOT raise: the kernel skips it silently.  inputs.brush_u8 checks the
    list while it is still on the host and raises; call this directly only with a list that went through inputs.brush_segments.
    S == 0 launches nothing."""
    if canvas.dim() != 3 or canvas.dtype != torch.uint8 or not canvas.is_contiguous():
        raise ValueError(f"brush_u8: canvas must be a contiguous uint8 [N,H,W], got {canvas.dtype} {tuple(canvas.shape)}")
    if segs.dim() != 2 or segs.shape[1] != 8 or segs.dtype != torch.int32 or segs.device != canvas.device:
        raise ValueError(f"brush_u8: segs must be int32 [S,8] on {canvas.device}, got {segs.dtype} {tuple(segs.shape)} on {segs.device}")
    n, h, w = canvas.shape
    if h > BRUSH_MAX_COORD + 1 or w > BRUSH_MAX_COORD + 1:
        raise ValueError(f"brush_u8: bad geometry {tuple(canvas.shape)} (H, W in [1, {BRUSH_MAX_COORD + 1}])")
    _check_nhw("brush_u8", canvas.shape)
    segs = segs.contiguous()
    C.backend().mge_brush_u8(_p(canvas), _p(segs), segs.shape[0], n, h, w, _stream(canvas))
    return canvas


def morph_u8(src: torch.Tensor, elem: torch.Tensor, anchor, op: int) -> torch.Tensor:
    """cv2.dilate (op MORPH_DILATE) / cv2.erode (op MORPH_ERODE) with their default border in one launch (mge_morph_u8): src u8
    [N,H,W] of any grey level, elem u8 [kh,kw] on the same device (non-zero = tap, any shape of element up to 64 x 64), anchor
    (ax, ay) inside it, cv2's (x, y) order -> a new u8 [N,H,W]."""
    if src.dim() != 3 or src.dtype != torch.uint8:
        raise ValueError(f"morph_u8: src must be uint8 [N,H,W], got {src.dtype} {tuple(src.shape)}")
    if elem.dim() != 2 or elem.dtype != torch.uint8 or elem.device != src.device:
        raise ValueError(f"morph_u8: elem must be uint8 [kh,kw] on {src.device}, got {elem.dtype} {tuple(elem.shape)} on {elem.device}")
    n, h, w = src.shape
    kh, kw = elem.shape
    ax, ay = (int(v) for v in anchor)
    if not (1 <= kh <= MORPH_MAX_K and 1 <= kw <= MORPH_MAX_K):
        raise ValueError(f"morph_u8: the element is {kh} x {kw}, at most {MORPH_MAX_K} x {MORPH_MAX_K} is supported")
    if not (0 <= ay < kh and 0 <= ax < kw):
        raise ValueError(f"morph_u8: anchor (x {ax}, y {ay}) outside the {kh} x {kw} element")
    if op not in (MORPH_DILATE, MORPH_ERODE):
        raise ValueError(f"morph_u8: op must be MORPH_DILATE or MORPH_ERODE, got {op}")
    _check_nhw("morph_u8", src.shape)
    src, elem = src.contiguous(), elem.contiguous()
    dst = torch.empty((n, h, w), dtype=torch.uint8, device=src.device)
    C.backend().mge_morph_u8(_p(src), _p(elem), kh, kw, ay, ax, op, _p(dst), n, h, w, _stream(src))
    return dst


QUALITY_TILE, QUALITY_MIN_K, QUALITY_MAX_K, QUALITY_MAX_C, QUALITY_WS_SLOTS = 16, 3, 15, 4, 6          # include/michigan_hip/evaluation/quality.h
QUALITY_INT_TERMS, QUALITY_SSIM_TERMS, ORIENT_PERIOD = 4, 2, 255


def image_quality_u8(a: torch.Tensor, b: torch.Tensor, mask: Optional[torch.Tensor], window) -> Tuple[torch.Tensor, torch.Tensor]:
    """PSNR / SSIM ingredients of two image batches in one pass (mgq_image_quality_u8, two launches): a, b u8 [N,H,W,C] NHWC, 1 <= C
    <= 4, mask u8 [N,H,W] or None (non-zero = in), window a HOST float64 array of k taps (k odd, 3 <= k <= 15, H, W >= k) ->
    (int64 [N,C,4] = sse, sse under the mask, mask count, valid-region mask count; float64 [N,C,2] = ssim sum over the valid region,
    the same under the mask), as include/michigan_hip/evaluation/quality.h defines them.  Views are made dense here; anything else
    raises ValueError before a call."""
    import numpy as np
    if a.dim() != 4 or b.shape != a.shape or a.dtype != torch.uint8 or b.dtype != torch.uint8 or b.device != a.device:
        raise ValueError(f"image_quality_u8: a and b must be uint8 [N,H,W,C] of one shape on one device, got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
    n, h, w, c = a.shape
    if not 1 <= c <= QUALITY_MAX_C:
        raise ValueError(f"image_quality_u8: {c} channels (NHWC with 1 <= C <= {QUALITY_MAX_C}); got {tuple(a.shape)}")
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (n, h, w) or mask.device != a.device):
        raise ValueError(f"image_quality_u8: mask must be uint8 {(n, h, w)} on {a.device}, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
    win = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    k = win.size
    if win.ndim != 1 or k % 2 == 0 or not QUALITY_MIN_K <= k <= QUALITY_MAX_K:
        raise ValueError(f"image_quality_u8: the window must be a vector of k taps, k odd in [{QUALITY_MIN_K}, {QUALITY_MAX_K}], got shape {win.shape}")
    if not np.isfinite(win).all():
        raise ValueError("image_quality_u8: the window holds a non-finite tap")
    if h < k or w < k:
        raise ValueError(f"image_quality_u8: the image {h} x {w} is smaller than the window k={k}")
    if n < 1 or n * h * w * c >= 1 << 31:
        raise ValueError(f"image_quality_u8: bad geometry {tuple(a.shape)} (N H W C must be in [1, 2^31))")
    a, b = a.contiguous(), b.contiguous()
    mask = None if mask is None else mask.contiguous()
    be = C.backend()
    ws = torch.empty(be.mgq_quality_workspace(n, h, w, c) // 8, dtype=torch.int64, device=a.device)
    out_int = torch.empty((n, c, QUALITY_INT_TERMS), dtype=torch.int64, device=a.device)
    out_ssim = torch.empty((n, c, QUALITY_SSIM_TERMS), dtype=torch.float64, device=a.device)
    be.mgq_image_quality_u8(_p(a), _p(b), _p(mask), ctypes.c_void_p(win.ctypes.data), k, _p(ws), _p(out_int), _p(out_ssim), n, h, w, c, _stream(a))
    return out_int, out_ssim


def orient_distance_u8(a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Agreement of two orientation maps (mgq_orient_distance_u8): a, b, mask u8 [N,H,W] -> int64 [N,2] = (sum over the pixels with
    mask != 0 of min(|a - b|, 255 - |a - b|), their count).  The coding has period 255."""
    if a.dim() != 3 or a.dtype != torch.uint8:
        raise ValueError(f"orient_distance_u8: a must be uint8 [N,H,W], got {a.dtype} {tuple(a.shape)}")
    for name, t in (("b", b), ("mask", mask)):
        if t is None or t.dtype != torch.uint8 or t.shape != a.shape or t.device != a.device:
            raise ValueError(f"orient_distance_u8: {name} must be uint8 {tuple(a.shape)} on {a.device}, got "
                             + ("None" if t is None else f"{t.dtype} {tuple(t.shape)} on {t.device}"))
    n, h, w = a.shape
    _check_nhw("orient_distance_u8", a.shape)
    a, b, mask = a.contiguous(), b.contiguous(), mask.contiguous()
    out = torch.empty((n, 2), dtype=torch.int64, device=a.device)
    C.backend().mgq_orient_distance_u8(_p(a), _p(b), _p(mask), _p(out), n, h, w, _stream(a))
    return out


def interp_nearest_table(src: int, dst: int, device=None) -> Optional[torch.Tensor]:
    """int32 [dst]: the source index F.interpolate(mode='nearest') reads for each of `dst` outputs of a `src`-long axis -- taken from
    F.interpolate itself on an arange, so it is that function's rule by construction.  None = identity (src == dst)."""
    import torch.nn.functional as F
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1 or src >= 1 << 24:
        raise ValueError(f"interp_nearest_table: bad sizes {src} -> {dst} (an index above 2^24 is not exact in fp32)")
    if src == dst:
        return None
    t = F.interpolate(torch.arange(src, dtype=torch.float32).view(1, 1, 1, src), size=(1, dst), mode="nearest").view(dst).to(torch.int32)
    return t.to(device) if device is not None else t


def _interp_table(src: int, dst: int, device):
    return _device_table(device, ("interp", int(src), int(dst)), lambda: interp_nearest_table(src, dst, device))


def _planes(name, t, c, n, h, w):
    if t.dtype != torch.float32 or tuple(t.shape) != (n, c, h, w):
        raise ValueError(f"{name} must be fp32 {(n, c, h, w)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def stroke_compose(orient_rgb: torch.Tensor, noise: torch.Tensor, hole: torch.Tensor, stroke: Optional[torch.Tensor] = None,
                   stroke_mask: Optional[torch.Tensor] = None, size=None, dtype=torch.float32) -> torch.Tensor:
    """The in-painting net's input in its own layout, in one launch (mg_stroke_compose; pix2pix_model.py:443-447, and 408-411 when
    stroke / stroke_mask are None): NCHW fp32 maps at H x W -> NHWC8 `dtype` at `size` (nearest, F.interpolate's rule), channels
    0-2 = orient_rgb (1 - hole) + noise (hole - stroke_mask) + stroke stroke_mask, 3 = hole, 4 = stroke_mask, 5-7 = 0."""
    if orient_rgb.dim() != 4 or orient_rgb.shape[1] != 3:
        raise ValueError(f"stroke_compose: orient_rgb must be [N,3,H,W], got {tuple(orient_rgb.shape)}")
    if (stroke is None) != (stroke_mask is None):
        raise ValueError("stroke_compose: stroke and stroke_mask are given together or not at all")
    n, _, h, w = orient_rgb.shape
    ho, wo = (h, w) if size is None else ((size, size) if isinstance(size, int) else tuple(size))
    orient_rgb, noise, hole = _planes("stroke_compose: orient_rgb", orient_rgb, 3, n, h, w), _planes("stroke_compose: noise", noise, 3, n, h, w), _planes("stroke_compose: hole", hole, 1, n, h, w)
    if stroke is not None:
        stroke, stroke_mask = _planes("stroke_compose: stroke", stroke, 3, n, h, w), _planes("stroke_compose: stroke_mask", stroke_mask, 1, n, h, w)
    code = _dtype_code(dtype)
    ytab, xtab = _interp_table(h, ho, orient_rgb.device), _interp_table(w, wo, orient_rgb.device)
    inp = torch.empty((n, ho, wo, 8), dtype=dtype, device=orient_rgb.device)
    C.backend().mg_stroke_compose(_p(orient_rgb), _p(noise), _p(hole), _p(stroke), _p(stroke_mask), _p(ytab), _p(xtab), code, n, h, w, ho, wo,
                                  _p(inp), _stream(orient_rgb))
    return inp


def inpaint_finish(net_out: torch.Tensor, hole: torch.Tensor, orient_rgb: torch.Tensor, mask: torch.Tensor):
    """What becomes of the in-painting net's output, in one launch (mg_inpaint_finish; pix2pix_model.py:450-463): net_out fp32
    [N,3,Ho,Wo] -> (out_rgb [N,3,H,W] = up(net_out) hole + orient_rgb (1 - hole), orient2 [N,2,H,W] = ((out_rgb[1] - 0.5) 2 mask,
    (out_rgb[0] - 0.5) 2 mask)), `up` being F.interpolate(mode='nearest') to the size of orient_rgb."""
    if orient_rgb.dim() != 4 or orient_rgb.shape[1] != 3:
        raise ValueError(f"inpaint_finish: orient_rgb must be [N,3,H,W], got {tuple(orient_rgb.shape)}")
    n, _, h, w = orient_rgb.shape
    if net_out.dim() != 4 or net_out.dtype != torch.float32 or net_out.shape[:2] != (n, 3):
        raise ValueError(f"inpaint_finish: net_out must be fp32 [{n},3,Ho,Wo], got {net_out.dtype} {tuple(net_out.shape)}")
    ho, wo = net_out.shape[2:]
    orient_rgb, hole, mask = _planes("inpaint_finish: orient_rgb", orient_rgb, 3, n, h, w), _planes("inpaint_finish: hole", hole, 1, n, h, w), _planes("inpaint_finish: mask", mask, 1, n, h, w)
    net_out = net_out.contiguous()
    ytab, xtab = _interp_table(ho, h, orient_rgb.device), _interp_table(wo, w, orient_rgb.device)
    out_rgb = torch.empty((n, 3, h, w), dtype=torch.float32, device=orient_rgb.device)
    orient2 = torch.empty((n, 2, h, w), dtype=torch.float32, device=orient_rgb.device)
    C.backend().mg_inpaint_finish(_p(net_out), _p(ytab), _p(xtab), _p(hole), _p(orient_rgb), _p(mask), n, h, w, ho, wo, _p(out_rgb), _p(orient2),
                                  _stream(orient_rgb))
    return out_rgb, orient2


def self_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[n, i] = sum_j softmax_j(q[n, i] . k[n, j]) v[n, j] over the L positions of each sample (generator.py:467-485; no 1/sqrt(d)
    scale), inference only.  q, k: [N, L, 64], v: [N, L, 256] in the compute dtype; each may be a column slice of a wider row-major
    tensor (last-dim stride 1, uniform row pitch), and so may `out` ([N, L, 256], e.g. the second half of the [x | attention]
    concatenation).  One flash-style launch: the [L, L] score matrix never exists (mg_attention.hip)."""
    n, l, dqk = q.shape
    dv = v.shape[2]
    if out is None:
        out = torch.empty((n, l, dv), dtype=v.dtype, device=v.device)

    def pitch(t, width):
        if t.shape != (n, l, width) or t.dtype != v.dtype or t.stride(2) != 1 or (n > 1 and t.stride(0) != l * t.stride(1)):
            raise ValueError("self_attention: operands must be [N, L, width] with dense channels and a uniform row pitch, same dtype")
        return t.stride(1)
    C.backend().mg_self_attention(_p(q), _p(k), _p(v), _p(out), _dt(v), n, l, dqk, dv, pitch(q, dqk), pitch(k, dqk), pitch(v, dv), pitch(out, dv),
                                  _stream(v))
    return out


class _SpectralScaleFn(torch.autograd.Function):
    """W_sn = W / sigma with sigma = u^T W v, u and v constants: dW = (g - (sum g * W_sn) u v^T) / sigma."""

    @staticmethod
    def forward(ctx, weight, u, v, sigma):
        ctx.set_materialize_grads(False)         # a consumer on the gradient sink returns no gradient: then there is nothing to do here
        w = weight.detach().contiguous()
        out = torch.empty_like(w)
        C.backend().mg_sn_scale(_p(w), _p(sigma), _p(out), w.numel(), _stream(w))
        ctx.save_for_backward(out, u, v, sigma)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        w_sn, u, v, sigma = ctx.saved_tensors
        g = g.contiguous().float()
        s = torch.dot(g.reshape(-1), w_sn.reshape(-1)).reshape(1)
        out = torch.empty_like(g)
        C.backend().mg_sn_bwd(_p(g), _p(u), _p(v), _p(s), _p(sigma), _p(out), u.numel(), v.numel(), _stream(g))
        return out, None, None, None


def spectral_weight(weight: torch.Tensor, u: torch.Tensor, v: torch.Tensor, do_power_iteration: bool, eps: float) -> torch.Tensor:
    """torch.nn.utils.spectral_norm's compute_weight (dim 0, one power iteration; `u`, `v` are the module's buffers
    and are updated in place when `do_power_iteration`): two rocBLAS gemv + three small launches forward, a dot + one
    launch backward, instead of ~16 launches forward and ~10 weight-sized autograd passes backward."""
    wm = weight.detach().reshape(weight.shape[0], -1)
    be = C.backend()
    need_grad = torch.is_grad_enabled() and weight.requires_grad
    sigma = torch.empty(1, dtype=torch.float32, device=weight.device)
    with torch.no_grad():
        if do_power_iteration:
            t1 = torch.mv(wm.t(), u)
            vc = torch.empty_like(v) if need_grad else None          # private copies for backward: the buffers change
            be.mg_sn_normalize(_p(t1), t1.numel(), eps, _p(v), _p(vc), None, _stream(weight))      # again at the next forward
            t2 = torch.mv(wm, v)
            uc = torch.empty_like(u) if need_grad else None
            be.mg_sn_normalize(_p(t2), t2.numel(), eps, _p(u), _p(uc), _p(sigma), _stream(weight))
        else:
            sigma = torch.dot(u, torch.mv(wm, v)).reshape(1)
            uc, vc = (u.clone(), v.clone()) if need_grad else (None, None)
    if need_grad:
        w_sn = _SpectralScaleFn.apply(weight, uc, vc, sigma)
        # lets a consuming convolution route its weight gradient through the optimiser's gradient sink, which applies this
        # layer's sigma-backward in the batched drain (optim.FlatAdam.drain_grads) instead of _SpectralScaleFn.backward
        w_sn._mg_sn = (weight, w_sn.detach(), uc, vc, sigma)
        w_sn._mg_sn_origin = weight
        return w_sn
    out = torch.empty_like(wm).view_as(weight)
    be.mg_sn_scale(_p(weight.detach().contiguous()), _p(sigma), _p(out), weight.numel(), _stream(weight))
    out._mg_sn_origin = weight
    return out


class _SpectralPrecomputedFn(torch.autograd.Function):
    """_SpectralScaleFn for a W / sigma that the batched path (networks/spectral.py) has already computed: `holder[0]`."""

    @staticmethod
    def forward(ctx, weight, u, v, sigma, holder):
        ctx.set_materialize_grads(False)
        out = holder[0]
        ctx.save_for_backward(out, u, v, sigma)
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        return _SpectralScaleFn.backward(ctx, g) + (None,)


def adam_step(param, grad, exp_avg, exp_avg_sq, *, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """In-place fused Adam on flat fp32 buffers (torch.optim.Adam semantics)."""
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("adam_step wants contiguous fp32 buffers")
    C.backend().mg_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(),
                             lr, beta1, beta2, eps, step, grad_scale, _stream(param))


# NCHW <-> NHWC glue for module boundaries (zero-copy when the tensor is already channels_last)
def to_nhwc(x: torch.Tensor, dtype=None) -> torch.Tensor:
    y = x.permute(0, 2, 3, 1)
    if dtype is not None and y.dtype != dtype:
        y = y.to(dtype)
    return y.contiguous()


def to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2)
