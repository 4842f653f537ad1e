"""Tensor-level wrappers over the C ABI (include/t2i_hip.h).  Each function allocates its output with torch (device
memory + caching allocator are PyTorch's job), passes raw device pointers and the current HIP stream to libt2i_hip.so
and returns.  No arithmetic happens in Python or in torch here.

CPU tensors are refused: the product path has no CPU implementation.  The only exception is ``dry_run()``, used by
the host-logic tests and by variable creation, in which launches are skipped and outputs are uninitialised
``torch.empty`` of the right shape (shape inference only — values are garbage by construction).
"""
import contextlib
import ctypes
import os

import numpy as np
import torch

from ._lib import CONSTANTS, DT_BF16, DT_F32, XFORM_HAVE, XFORM_KEEP, ConvDesc, ConvOpts, ImageDesc, check, header_values, lib

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = header_values('ACT_NONE', 'ACT_LRELU', 'ACT_RELU', 'ACT_TANH')

_DRY = [False]


@contextlib.contextmanager
def dry_run():
    """Shape-inference mode: no kernel is launched, outputs are uninitialised."""
    prev = _DRY[0]
    _DRY[0] = True
    try:
        yield
    finally:
        _DRY[0] = prev


def is_dry():
    return _DRY[0]


def _live(t):
    """True -> launch on the GPU.  False -> dry run.  CPU tensor outside dry_run -> error (no fallback)."""
    if _DRY[0]:
        return False
    if t.is_cuda:
        return True
    raise RuntimeError('text-to-image_amd kernels need a ROCm device tensor (got %s); there is no CPU path' % t.device)


def _chk(t, name='tensor', f32=False):
    """Activation tensors are float32, or bfloat16 under bf16 storage (set_storage); parameters and reduction results (f32=True)
    are always float32."""
    if t.dtype != torch.float32 and (f32 or t.dtype != torch.bfloat16):
        raise TypeError('%s must be float32%s, got %s' % (name, '' if f32 else ' or bfloat16', t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous (shape %s, strides %s)' % (name, tuple(t.shape), t.stride()))
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- workspace: one grow-only buffer per (device, lane); all users of a buffer are ordered on one stream.  Lane 0 is the
# caller's current stream; autograd's filter-gradient side stream launches under lane 1 (WS_LANE) -----------------------
WS_LANE = [0]
_STREAM_LANE = {}        # hipStream_t -> lane, for streams that run convolutions of their own (stream_lane)
_WS = {}
_WS_MIN = 64 << 20
_WS_CAPTURED = set()     # lanes whose CURRENT buffer has been handed to a kernel inside a graph capture
_WS_RETIRED = []         # outgrown buffers that captured graphs still point at: kept alive for the life of the process


PAIR_LANE = 1000          # lane + PAIR_LANE: the second workspace of a fused backward pair (kernels.conv_bwd_pair)


def workspace(device, nbytes):
    """The lane's scratch buffer, grown on demand.  A hipGraph captured while a buffer was current has that buffer's
    address baked into its kernel arguments, so once a capture has used a buffer it is never freed: a later eager call
    that needs more (the sampler at SAMPLE_NUM > BATCH_SIZE, a bigger batch) gets a NEW buffer and the old one is retired
    but kept alive — replays keep writing into memory they still own."""
    lane = WS_LANE[0]
    if lane == 0 and _STREAM_LANE and device.type == 'cuda':
        lane = _STREAM_LANE.get(torch.cuda.current_stream(device).cuda_stream, 0)
    key = (device.type, device.index, lane)
    buf = _WS.get(key)
    capturing = torch.cuda.is_available() and device.type == 'cuda' and torch.cuda.is_current_stream_capturing()
    if buf is None or buf.numel() < nbytes:
        if capturing:
            raise RuntimeError('workspace would grow during graph capture; run warm-up iterations first')
        if buf is not None and key in _WS_CAPTURED:
            _WS_RETIRED.append(buf)
            _WS_CAPTURED.discard(key)
        buf = torch.empty(max(int(nbytes), _WS_MIN), dtype=torch.uint8, device=device)
        _WS[key] = buf
    if capturing:
        _WS_CAPTURED.add(key)
    return buf


def stream_lane(stream, device=None):
    """Give the HIP stream behind `stream` its own workspace lane, sized like lane 0: launches on it never share scratch with the
    main stream's.  The lane belongs to the underlying hipStream_t (PyTorch hands out 32 pooled streams per device round-robin):
    two models whose second streams are different pool streams get different lanes; if the pool gives two models the SAME stream
    their work is ordered on it anyway, and sharing the lane is safe.  At most 32 lanes ever exist."""
    lane = _STREAM_LANE.setdefault(stream.cuda_stream, 2 + len(_STREAM_LANE))
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    main = _WS.get((dev.type, dev.index, 0))
    key = (dev.type, dev.index, lane)
    for key in (key, (dev.type, dev.index, PAIR_LANE + lane)):       # ... and the lane of conv_bwd_pair's second workspace
        if main is not None and (_WS.get(key) is None or _WS[key].numel() < main.numel()):
            if _WS.get(key) is not None and key in _WS_CAPTURED:
                _WS_RETIRED.append(_WS[key]); _WS_CAPTURED.discard(key)
            _WS[key] = torch.empty(main.numel(), dtype=torch.uint8, device=dev)


# ---- convolution geometry (TF padding rules; reference utils/ops.py:58-71 passes the string through to TF) -------------
def same_pad(in_size, k, s):
    out = -(-in_size // s)
    total = max((out - 1) * s + k - in_size, 0)
    return out, total // 2


_DESC_CACHE = {}

# Arithmetic of the conv family (t2i_conv_desc.math): 'f32' = exact fp32 matrix pipe (default, BASELINE config 2);
# 'bf16' = operands rounded to bf16 inside the kernel, bf16 MFMA with fp32 accumulation, fp32 tensors (config 3).
MATH_F32, MATH_BF16 = header_values('MATH_F32', 'MATH_BF16')
_MATH = [MATH_F32]


_MATH_CODES = {'f32': MATH_F32, 'fp32': MATH_F32, 'bf16': MATH_BF16}


def set_math(mode):
    """Select the arithmetic of every conv/deconv/dense descriptor created from now on: 'f32' or 'bf16'.  (Also forgets that a
    math_scope has been used: a new configuration starts from the process-wide rules for bf16 twins.)"""
    _MATH[0] = _MATH_CODES[str(mode).lower()]
    _MIXED[0] = False


def get_math():
    return 'bf16' if _MATH[0] == MATH_BF16 else 'f32'


# Storage of the activation tensors the wrappers allocate (ABI v6, BASELINE config 3 end to end): 'f32' (default), or 'bf16' —
# every activation / activation-gradient tensor with a multiple of 64 channels is then a torch.bfloat16 tensor, written by the
# producing kernel and read by the consuming kernel as bf16; the 3-channel image side, logits, losses, parameters, gradients of
# parameters, optimizer state and batch-norm statistics stay float32.  Needs set_math('bf16').
_STORE = [torch.float32]
_FORCE_F32 = [0]


def set_storage(mode):
    mode = {'f32': torch.float32, 'fp32': torch.float32, 'bf16': torch.bfloat16}[str(mode).lower()]
    if mode is torch.bfloat16 and _MATH[0] != MATH_BF16:
        raise ValueError("set_storage('bf16') needs set_math('bf16') first (bf16 tensors feed the bf16 matrix pipe)")
    _STORE[0] = mode
    _MIXED[0] = False          # a new configuration: the twin policy of an earlier math_scope does not carry over (see _MIXED)


def get_storage():
    return 'bf16' if _STORE[0] is torch.bfloat16 else 'f32'


@contextlib.contextmanager
def f32_outputs():
    """Inside, the wrappers allocate float32 outputs whatever the storage mode (small tensors that feed fp32-only kernels: the two
    conditioning-augmentation heads in front of t2i_ca_kl_fwd)."""
    _FORCE_F32[0] += 1
    try:
        yield
    finally:
        _FORCE_F32[0] -= 1


# Per-network arithmetic (config 3's compliant mode): a scope in which descriptors are created with another math mode and
# activations are allocated with another storage dtype than the process-wide setting.  The backward of a layer follows its forward
# (descriptors travel in the autograd context, gradients take the dtype of the tensor they are the gradient of), so entering the
# scope around a network's FORWARD is enough.  _MIXED: a scope has been used — with bf16 storage outside the scope every tensor
# that wants a bf16 image is one already, so float32 outputs (the scoped network's) get no bf16 twin.
# _MIXED is process-wide and sticky BY DESIGN within one configuration (the scoped network's backward runs outside the scope, long
# after it exited, and must still see the policy); it is cleared by set_math(), set_storage() and forget_scopes() — the models call
# the latter when they are constructed outside any scope, so a later, unscoped model in the same process starts from the plain rules.
_MIXED = [False]
_BWD_MATH = [None]
_SCOPE_GRAD = [True]     # torch.is_grad_enabled() when the innermost math_scope was entered — by model code, outside any autograd Function (inside a
                         # Function.forward grad mode is always off): "will this forward be differentiated?", for _twin_for


def forget_scopes():
    """Clear the sticky twin policy a finished math_scope left behind (no-op while a scope is open)."""
    if _BWD_MATH[0] is None:
        _MIXED[0] = False
          # arithmetic of the BACKWARD GEMMs of layers created in the current scope (None: the forward's)


@contextlib.contextmanager
def math_scope(math=None, storage=None, bwd_math=None):
    """with math_scope('f32', 'f32'): ...  — conv descriptors and activation tensors created inside use this arithmetic / storage.
    bwd_math: the input- and filter-gradient GEMMs of those layers run in this arithmetic instead (the backward is linear in the
    upstream gradient, so its rounding errors add up once; the forward's are amplified by every nonlinear term behind them)."""
    if math is None and storage is None and bwd_math is None:
        yield
        return
    pm, ps, pb, pg = _MATH[0], _STORE[0], _BWD_MATH[0], _SCOPE_GRAD[0]
    _SCOPE_GRAD[0] = torch.is_grad_enabled()
    _MIXED[0] = 'bwd_bf16' if (bwd_math is not None and _MATH_CODES[str(bwd_math).lower()] == MATH_BF16) or _MIXED[0] == 'bwd_bf16' else 'fwd'
    try:
        if math is not None:
            _MATH[0] = _MATH_CODES[str(math).lower()]
        if storage is not None:
            _STORE[0] = {'f32': torch.float32, 'fp32': torch.float32, 'bf16': torch.bfloat16}[str(storage).lower()]
        _BWD_MATH[0] = _MATH_CODES[str(bwd_math).lower()] if bwd_math is not None else None
        yield
    finally:
        _MATH[0], _STORE[0], _BWD_MATH[0], _SCOPE_GRAD[0] = pm, ps, pb, pg


# BASELINE configs[2] ("bf16 MFMA") as benchmarked and as its parity test asserts (<= 2e-2 on every tensor, tests/test_step_b64_gpu.py):
# per-network arithmetic (math, storage, backward math) handed to math_scope by the models.  Networks not named run in the
# process-wide setting (set_math('bf16') + set_storage('bf16')): the critic.  DESIGN.md 4.16.
CONFIG3_NET_MATH = {'g_net': ('f32', 'f32', 'bf16')}
# Every forward GEMM in fp32 math on fp32 tensors, every input- and filter-gradient GEMM in bf16 math (bf16 operand images, fp32 accumulate): the
# arithmetic under which the batch-normalised StackGAN Stage-II step stays inside 2e-2 (tests/test_fullsize_gpu.py)
FWD_F32_BWD_BF16 = ('f32', 'f32', 'bf16')


def bwd_geom(geom):
    """(descriptor, workspace bytes) for the backward GEMMs of a layer whose forward uses `geom`: the same geometry in the scope's
    backward arithmetic (math_scope(bwd_math=...)), or `geom` itself."""
    bm = _BWD_MATH[0]
    d = geom[0]
    if bm is None or bm == d.math:
        return geom
    key = ('bwd', id(d), bm)
    hit = _DESC_CACHE.get(key)
    if hit is None:
        d2 = ConvDesc(d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout, d.KH, d.KW, d.SH, d.SW, d.pad_t, d.pad_l, bm)
        hit = _DESC_CACHE[key] = (d2, int(lib.t2i_conv2d_workspace_bytes(ctypes.byref(d2))), d)      # (keeps d alive: id(d) is the key)
    return hit[0], hit[1]


def _act_dtype(shape, want=None):
    """dtype of a freshly allocated activation tensor of `shape`; want: the caller's explicit choice (a gradient takes the dtype of
    the tensor it is the gradient of)."""
    if want is not None:
        return want
    if _STORE[0] is torch.bfloat16 and not _FORCE_F32[0] and _MATH[0] == MATH_BF16 and shape[-1] % 64 == 0:
        n = 1
        for k in shape:
            n *= int(k)
        if n % 8 == 0:
            return torch.bfloat16
    return torch.float32


def _dt(t):
    return DT_BF16 if t.dtype == torch.bfloat16 else DT_F32


def _same_dt(*ts):
    ts = [t for t in ts if t is not None]
    if any(t.dtype != ts[0].dtype for t in ts):
        raise TypeError('activation tensors of one call must share a dtype, got %s' % [str(t.dtype) for t in ts])
    return _dt(ts[0])


def cast_f32(t):
    """bf16 activation -> float32 tensor (exact), through t2i_cast_f32."""
    if t.dtype == torch.float32:
        return t
    _chk(t, 't')
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    if _live(t):
        check(lib.t2i_cast_f32(_ptr(t), t.numel(), _ptr(out), _stream()), 't2i_cast_f32')
    return out


def conv_desc(B, H, W, Cin, Cout, KH, KW, SH, SW, padding, math=None):
    """-> (ConvDesc, workspace_bytes) for y = conv(x[B,H,W,Cin], w[KH,KW,Cin,Cout]) with a TF padding string."""
    math = _MATH[0] if math is None else math
    key = (B, H, W, Cin, Cout, KH, KW, SH, SW, padding.upper(), math)
    hit = _DESC_CACHE.get(key)
    if hit is not None:
        return hit
    p = padding.upper()
    if p == 'SAME':
        Ho, pt = same_pad(H, KH, SH)
        Wo, pl = same_pad(W, KW, SW)
    elif p == 'VALID':
        Ho, Wo, pt, pl = (H - KH) // SH + 1, (W - KW) // SW + 1, 0, 0
    else:
        raise ValueError('Invalid padding %s' % padding)
    if Ho <= 0 or Wo <= 0:
        raise ValueError('convolution output is empty for input %dx%d kernel %dx%d' % (H, W, KH, KW))
    d = ConvDesc(B, H, W, Cin, Ho, Wo, Cout, KH, KW, SH, SW, pt, pl, math)
    ws = int(lib.t2i_conv2d_workspace_bytes(ctypes.byref(d)))
    _DESC_CACHE[key] = (d, ws)
    return d, ws


def rebatch(geom, B):
    """(descriptor, workspace bytes) of the same convolution on another batch size: a slice of a stacked pass (stacked.py) is an
    ordinary pass of its own.  Geometry, padding and arithmetic are copied from `geom`'s descriptor."""
    d = geom[0]
    if d.B == B:
        return geom
    key = ('rebatch', B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout, d.KH, d.KW, d.SH, d.SW, d.pad_t, d.pad_l, d.math)
    hit = _DESC_CACHE.get(key)
    if hit is None:
        d2 = ConvDesc(B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout, d.KH, d.KW, d.SH, d.SW, d.pad_t, d.pad_l, d.math)
        hit = _DESC_CACHE[key] = (d2, int(lib.t2i_conv2d_workspace_bytes(ctypes.byref(d2))))
    return hit


def deconv_desc(B, H, W, Cin, Cout, KH, KW, SH, SW, padding, math=None):
    """Descriptor of the ADJOINT conv of a TF conv2d_transpose x[B,H,W,Cin] -> [B,Hout,Wout,Cout]: that conv maps
    [B,Hout,Wout,Cout] -> [B,H,W,Cin] with HWIO filter [KH,KW,Cout,Cin] (the TF deconv layout)."""
    p = padding.upper()
    if p == 'SAME':
        Hout, Wout = H * SH, W * SW
    elif p == 'VALID':
        Hout, Wout = (H - 1) * SH + KH, (W - 1) * SW + KW
    else:
        raise ValueError('Invalid padding %s' % padding)
    d, ws = conv_desc(B, Hout, Wout, Cout, Cin, KH, KW, SH, SW, padding, math)
    if (d.Ho, d.Wo) != (H, W):
        raise ValueError('conv2d_transpose geometry mismatch: adjoint conv gives %dx%d, input is %dx%d' % (d.Ho, d.Wo, H, W))
    return d, ws


# Optional per-launch timing hook (bench.py): an object with begin(flops) -> end_event; the wrappers record the end
# event right after the launch, on the same (current) stream.
_TIMER = [None]


def set_conv_timer(timer):
    _TIMER[0] = timer


def conv_flops(d):
    """Algorithmic FLOPs of any of the three conv primitives for descriptor d (2 x MACs incl. padded taps)."""
    return 2 * d.B * d.Ho * d.Wo * d.Cout * d.KH * d.KW * d.Cin


def _ws_args(t, nbytes):
    if nbytes == 0:
        return None, 0
    buf = workspace(t.device, nbytes)
    return _ptr(buf), buf.numel()


# bf16 math: the GEMMs read bf16 images of their activation operands.  An activation is used by up to three convs (forward,
# filter gradient, the second-order pieces of the gradient penalty), a gradient by two (input and filter gradient): the image
# is made once per tensor (and version) here, kept on the tensor object and handed to every conv that reads the tensor
# (t2i_conv_opts.a_image / b_image), instead of each entry point staging its own copy into the workspace.
_BF16_IMAGES = [True]
_H_ALGO = {}


def bf16_images(on):
    prev, _BF16_IMAGES[0] = _BF16_IMAGES[0], bool(on)
    return prev


def _h_path(d, mode):
    """does this descriptor's `mode` run the GEMM with bf16 operands in memory?"""
    if d.math != MATH_BF16 or not _BF16_IMAGES[0]:
        return False
    key = (id(d), mode)
    hit = _H_ALGO.get(key)
    if hit is None:
        hit = _H_ALGO[key] = (conv_algo(d, mode) == 'implicit_gemm_bf16_operands')
    return hit


def cast_bf16(t):
    _chk(t, 't')
    img = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    check(lib.t2i_cast_bf16(_ptr(t), t.numel(), _ptr(img), _stream()), 't2i_cast_bf16')
    return img


def _image_holder(t):
    """The tensor object the image is kept on: the base of `t` when t is a full view of it (the layout helpers of utils/ops.py hand
    the convs permuted-and-permuted-back views of the producing kernel's output: same memory, same order, another object)."""
    b = t._base
    return b if (b is not None and b.data_ptr() == t.data_ptr() and b.numel() == t.numel()) else t


def bf16_image(t):
    """The bf16 image of fp32 tensor `t` (None if it cannot have one): cached on the tensor object with the version it was made of.
    INVARIANT: the kernels of this package write through raw pointers and do not bump tensor._version, so every wrapper that
    overwrites an EXISTING tensor (the `out=` arguments of axpby, col_reduce, conv_bwd_filter) drops the cached image of that
    tensor itself (_drop_image); all other wrappers write freshly allocated outputs."""
    if t.dtype == torch.bfloat16:
        return t                       # bf16 storage: the tensor is its own image
    if t.numel() % 8 != 0 or t.data_ptr() % 16 != 0:
        return None
    h = _image_holder(t)
    c = getattr(h, '_t2i_h', None)
    cap = int(lib.t2i_capture_id(_stream()))      # an image made outside the current capture (eager, or an earlier capture) is
    if c is not None and c[0] == t._version and c[2] == t.data_ptr() and c[3] == cap:      # not part of this graph: never reused
        return c[1]
    if c is None and h is t:
        # a contiguous run of rows of a tensor that HAS an image (a part of a stacked pass, stacked.py: the producer wrote the twin of the
        # whole stacked tensor): the same rows of that image
        b = t._base
        cb = getattr(b, '_t2i_h', None) if b is not None else None
        if (cb is not None and cb[0] == t._version and cb[3] == cap and cb[2] == b.data_ptr() and t.is_contiguous() and b.is_contiguous() and
                t.dim() == b.dim() and t.shape[1:] == b.shape[1:] and t.dtype == b.dtype):
            row = t[0].numel() * t.element_size() if t.shape[0] else 0
            off = t.data_ptr() - b.data_ptr()
            if row and off % row == 0 and 0 <= off // row and off // row + t.shape[0] <= b.shape[0]:
                r0 = off // row
                part = cb[1][r0:r0 + t.shape[0]]
                if part.data_ptr() % 16 == 0:
                    return part
    img = cast_bf16(t)
    h._t2i_h = (t._version, img, t.data_ptr(), cap)
    return img


def _operand_images(opts, a, b=None):
    """Put the bf16 images of the call's activation operands into its t2i_conv_opts; the returned tensors must stay alive until
    the conv call has been issued."""
    ia = bf16_image(a) if (a is not None and a.dtype != torch.bfloat16) else None      # a bf16 tensor is passed as the operand itself
    ib = bf16_image(b) if (b is not None and b.dtype != torch.bfloat16) else None
    opts.a_image = ia.data_ptr() if ia is not None else None
    opts.b_image = ib.data_ptr() if ib is not None else None
    return ia, ib


# ... and where the tensor a conv will read comes out of one of our own kernels (activation / batch-norm apply / residual join /
# a conv epilogue with its activation fused / activation backward), that kernel writes the bf16 image as a TWIN of its fp32
# output in the same pass (the y_h arguments / t2i_conv_opts.out_image): no cast launch at all for it.
_TWINS = [True]


def bf16_twins(on):
    prev, _TWINS[0] = _TWINS[0], bool(on)
    return prev


def _twin_for(out, *inputs):
    """A buffer for the bf16 twin of `out` (bf16 math, a multiple of 64 channels: a conv reads it next), or None.  The producers
    write it on their vectorised path only, so every tensor of the call must be 16-byte aligned (the entry points refuse otherwise)."""
    want = _MATH[0] == MATH_BF16
    if _MIXED[0]:
        if _BWD_MATH[0] == MATH_BF16:            # inside a scope whose backward GEMMs read bf16 images: the saved activations get theirs here
            # (round 6: the grad mode of the scope's entry — the producers run inside autograd Functions, where torch.is_grad_enabled() is
            # always False, so the rounds 4-5 rule that asked it never made a twin and every saved activation was cast in a launch of its own)
            want = _SCOPE_GRAD[0]
        elif _STORE[0] is torch.bfloat16:        # outside the scope, bf16 storage: a float32 tensor here belongs to the scoped network's backward
            want = _MIXED[0] == 'bwd_bf16'
    if out.dtype != torch.float32 or not want or not (_TWINS[0] and _BF16_IMAGES[0]) or out.shape[-1] % 64 or out.numel() % 8:
        return None
    if any(t is not None and t.data_ptr() % 16 for t in (out,) + inputs):
        return None
    return torch.empty(out.shape, dtype=torch.bfloat16, device=out.device)


def _twin_keep(out, img, written=True):
    """Remember `img` as the bf16 image of `out` (the call that was handed it has been issued and wrote it)."""
    if img is not None and written:
        out._t2i_h = (out._version, img, out.data_ptr(), int(lib.t2i_capture_id(_stream())))


# fp32 Winograd: the forward conv of a layer and its filter gradient transform the same x.  conv_fwd(..., keep_xform=True) leaves
# the transform in a tensor it returns through `LAST_XFORM` (None if the call took another path); conv_bwd_filter(..., xform=V)
# reads it instead of transforming x again (t2i_conv2d_input_transform).
_XFORM_BYTES = {}
LAST_XFORM = [None]
_SHARE_XFORM = [True]


def share_xform(on):
    prev, _SHARE_XFORM[0] = _SHARE_XFORM[0], bool(on)
    return prev


def conv_xform_bytes(d):
    if d.math != MATH_F32 or not _SHARE_XFORM[0]:
        return 0
    n = _XFORM_BYTES.get(id(d))
    if n is None:
        n = _XFORM_BYTES[id(d)] = int(lib.t2i_conv2d_input_transform_bytes(ctypes.byref(d)))
    return n


def _xform_offer(opts, x, d, keep):
    """Offer the forward conv a buffer to leave its Winograd input transform in (t2i_conv_opts.xform, T2I_XFORM_KEEP)."""
    LAST_XFORM[0] = None
    nb = conv_xform_bytes(d) if keep else 0
    if not nb:
        return None
    V = torch.empty(nb // 4, dtype=torch.float32, device=x.device)
    opts.xform, opts.xform_bytes, opts.xform_mode = V.data_ptr(), nb, XFORM_KEEP
    return V


def _xform_taken(opts, V):
    if V is not None and opts.xform_kept:
        LAST_XFORM[0] = V


def _storage_flags(opts, a, b, out):
    opts.in_dtype = (1 if a.dtype == torch.bfloat16 else 0) | (2 if (b is not None and b.dtype == torch.bfloat16) else 0)
    opts.out_dtype = DT_BF16 if (out is not None and out.dtype == torch.bfloat16) else DT_F32


# Where the NEXT conv_fwd whose output has exactly this shape and dtype writes (one shot): the critic step lets the generator's last
# kernel put G straight into its slot of the stacked critic input [G | x | x_mismatch | x_hat] instead of concatenating afterwards.
_OUT_INTO = [None]


class output_into(object):
    def __init__(self, t):
        self.t = t

    def __enter__(self):
        self.prev, _OUT_INTO[0] = _OUT_INTO[0], self.t

    def __exit__(self, *a):
        self.taken = _OUT_INTO[0] is None
        _OUT_INTO[0] = self.prev


def _take_out(shape, dtype, device):
    t = _OUT_INTO[0]
    if t is not None and tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_contiguous() and t.device == device:
        _OUT_INTO[0] = None
        _drop_image(t)
        return t
    return None


def conv_fwd(x, w, bias, d, ws_bytes, act=ACT_NONE, alpha=0.2, keep_xform=False, out_dtype=None):
    _chk(x, 'x'); _chk(w, 'w', f32=True)
    oshape, odt = (d.B, d.Ho, d.Wo, d.Cout), _act_dtype((d.B, d.Ho, d.Wo, d.Cout), out_dtype)
    y = _take_out(oshape, odt, x.device) if _OUT_INTO[0] is not None else None
    if y is None:
        y = torch.empty(oshape, dtype=odt, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, ws_bytes)
        ev = _TIMER[0].begin(conv_flops(d), conv_algo(d, 'fwd')) if _TIMER[0] is not None else None
        opts = ConvOpts()          # every allocation happens BEFORE the call; nothing is armed on the library side
        _storage_flags(opts, x, None, y)
        keep = _operand_images(opts, x) if _h_path(d, 'fwd') else None
        twin = _twin_for(y) if (act != ACT_NONE and d.math == MATH_BF16) else None     # conv + bias + lrelu feeds the next conv directly
        opts.out_image = twin.data_ptr() if twin is not None else None
        V = _xform_offer(opts, x, d, keep_xform)
        check(lib.t2i_conv2d_fwd(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(_chk(bias, 'bias') if bias is not None else None),
                                 _ptr(y), act, alpha, ctypes.byref(opts), wsp, wsn, _stream()), 't2i_conv2d_fwd')
        _twin_keep(y, twin, opts.out_image_written)
        _xform_taken(opts, V)
        if ev is not None:
            ev.record()
    return y


# Batch-norm statistics produced by a conv epilogue, waiting for the batch norm that consumes that conv's output:
# output address -> (partials [2, chunks, C], chunks).  Filled by conv_fwd(..., stats=True), emptied by take_stats().
_STATS = {}


def take_stats(x):
    """(column sums, centred second moments sum (x - mean)^2) of `x` if the conv that produced it left its epilogue
    partials (per-tile sums and second moments about each tile's mean, merged here with Chan's update), else None."""
    hit = _STATS.pop(x.data_ptr(), None)
    if hit is None:
        return None
    part, chunks, tile_rows, shape = hit
    if tuple(x.shape) != shape:
        return None
    C = x.shape[-1]
    s0 = torch.empty(C, dtype=torch.float32, device=x.device); s1 = torch.empty_like(s0)
    check(lib.t2i_bn_stats_tiles(_ptr(part), ctypes.c_void_p(part.data_ptr() + chunks * C * 4), chunks, tile_rows, x.numel() // C, C,
                                 _ptr(s0), _ptr(s1), _stream()), 't2i_bn_stats_tiles')
    return s0, s1


def bn_train_stats(x, gamma, beta, eps, decay, moving_mean=None, moving_var=None):
    """Batch statistics of x (view [rows, C]) and the batch norm's finalize step in one chain -> (mean, rstd, scale, shift);
    moving averages updated in place when given.  Uses the producing conv's epilogue partials when it left any (take_stats)."""
    _chk(x, 'x')
    C = x.shape[-1]
    rows = x.numel() // C
    mean, rstd, scale, shift = (torch.empty(C, dtype=torch.float32, device=x.device) for _ in range(4))
    if _live(x):
        hit = _STATS.pop(x.data_ptr(), None)
        if hit is not None and tuple(x.shape) != hit[3]:
            hit = None
        if hit is not None:
            part, chunks, tile_rows, _ = hit
            check(lib.t2i_bn_train_fwd_stats(None, _ptr(part), ctypes.c_void_p(part.data_ptr() + chunks * C * 4), chunks, tile_rows, rows, C,
                                             _ptr(_chk(gamma)), _ptr(_chk(beta)), eps, decay, _ptr(mean), _ptr(rstd), _ptr(scale), _ptr(shift),
                                             _ptr(moving_mean), _ptr(moving_var), None, 0, DT_F32, _stream()), 't2i_bn_train_fwd_stats')
        else:
            wsp, wsn = _ws_args(x, int(lib.t2i_col_reduce_workspace_bytes(rows, C)))
            check(lib.t2i_bn_train_fwd_stats(_ptr(x), None, None, 0, 0, rows, C, _ptr(_chk(gamma)), _ptr(_chk(beta)), eps, decay, _ptr(mean),
                                             _ptr(rstd), _ptr(scale), _ptr(shift), _ptr(moving_mean), _ptr(moving_var), wsp, wsn, _dt(x),
                                             _stream()), 't2i_bn_train_fwd_stats')
    return mean, rstd, scale, shift


def bn_bwd_fused(dy, y, x, mean, rstd, gamma, act, alpha=0.2, dgamma_out=None, dbeta_out=None, out=None):
    """Training-mode batch-norm backward in three launches (C % 4 == 0).  y: the activation output behind the batch norm or
    None.  -> (dx, dgamma, dbeta); dgamma_out / dbeta_out: gradient-arena slots to ACCUMULATE into; out: where dx goes (a group's
    slice of a batched pass; no bf16 twin then)."""
    _chk(dy, 'dy'); _chk(x, 'x')
    C = x.shape[-1]
    rows = x.numel() // C
    if out is not None:
        assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
        _drop_image(out)
    dx = out if out is not None else torch.empty_like(x)
    gmask = torch.empty_like(x) if y is not None else None
    acc = dgamma_out is not None
    assert acc == (dbeta_out is not None)
    dgamma = dgamma_out if acc else torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = dbeta_out if acc else torch.empty(C, dtype=torch.float32, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, int(lib.t2i_bn_bwd_fused_workspace_bytes(rows, C)))
        twin = _twin_for(dx) if out is None else None     # dx is the gradient of the conv in front of the batch norm: its bwd_data / bwd_filter operand
        check(lib.t2i_bn_bwd_fused(_ptr(dy), _ptr(_chk(y, 'y') if y is not None else None), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(_chk(gamma)),
                                   rows, C, act, alpha, _ptr(gmask), _ptr(dx), _ptr(twin), _ptr(dgamma), _ptr(dbeta), 1 if acc else 0, wsp, wsn,
                                   _same_dt(dy, y, x), _stream()), 't2i_bn_bwd_fused')
        _twin_keep(dx, twin)
    return dx, dgamma, dbeta


def bn_stats(x):
    """x viewed as [rows, C] -> (sum over rows, sum over rows of (x - mean)^2), numerically stable (t2i_bn_stats)."""
    _chk(x, 'x')
    C = x.shape[-1]
    rows = x.numel() // C
    s0 = torch.empty(C, dtype=torch.float32, device=x.device); s1 = torch.empty_like(s0)
    if _live(x):
        need = int(lib.t2i_col_reduce_workspace_bytes(rows, C))
        wsp, wsn = _ws_args(x, need)
        check(lib.t2i_bn_stats(_ptr(x), rows, C, _ptr(s0), _ptr(s1), wsp, wsn, _stream()), 't2i_bn_stats')
    return s0, s1


def conv_fwd_stats(x, w, bias, d, ws_bytes, act=ACT_NONE, alpha=0.2, keep_xform=False, out_dtype=None):
    """conv_fwd whose epilogue also leaves the per-tile column sums of y, y*y for the batch norm behind it (take_stats)."""
    _chk(x, 'x'); _chk(w, 'w', f32=True)
    y = torch.empty((d.B, d.Ho, d.Wo, d.Cout), dtype=_act_dtype((d.B, d.Ho, d.Wo, d.Cout), out_dtype), device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, ws_bytes)
        nbytes = int(lib.t2i_conv2d_stats_bytes(ctypes.byref(d)))
        part = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        chunks, tile_rows = ctypes.c_int32(0), ctypes.c_int32(0)
        ev = _TIMER[0].begin(conv_flops(d), conv_algo(d, 'fwd')) if _TIMER[0] is not None else None
        opts = ConvOpts()
        _storage_flags(opts, x, None, y)
        keep = _operand_images(opts, x) if _h_path(d, 'fwd') else None
        V = _xform_offer(opts, x, d, keep_xform)
        check(lib.t2i_conv2d_fwd_stats(ctypes.byref(d), _ptr(x), _ptr(w), _ptr(_chk(bias, 'bias') if bias is not None else None),
                                       _ptr(y), act, alpha, _ptr(part), nbytes, ctypes.byref(chunks), ctypes.byref(tile_rows),
                                       ctypes.byref(opts), wsp, wsn, _stream()), 't2i_conv2d_fwd_stats')
        _xform_taken(opts, V)
        if ev is not None:
            ev.record()
        if chunks.value > 0:
            if len(_STATS) > 64:
                _STATS.clear()
            _STATS[y.data_ptr()] = (part, int(chunks.value), int(tile_rows.value), tuple(y.shape))
    return y


def conv_bwd_data(dy, w, bias, d, ws_bytes, act=ACT_NONE, alpha=0.2, out_dtype=None):
    _chk(dy, 'dy'); _chk(w, 'w', f32=True)
    dx = torch.empty((d.B, d.H, d.W, d.Cin), dtype=_act_dtype((d.B, d.H, d.W, d.Cin), out_dtype), device=dy.device)
    if _live(dy):
        wsp, wsn = _ws_args(dy, ws_bytes)
        ev = _TIMER[0].begin(conv_flops(d), conv_algo(d, 'bwd_data')) if _TIMER[0] is not None else None
        opts = ConvOpts()
        _storage_flags(opts, dy, None, dx)
        keep = _operand_images(opts, dy) if _h_path(d, 'bwd_data') else None
        twin = _twin_for(dx) if (act != ACT_NONE and d.math == MATH_BF16) else None
        opts.out_image = twin.data_ptr() if twin is not None else None
        check(lib.t2i_conv2d_bwd_data(ctypes.byref(d), _ptr(dy), _ptr(w),
                                      _ptr(_chk(bias, 'bias') if bias is not None else None), _ptr(dx), act, alpha, ctypes.byref(opts),
                                      wsp, wsn, _stream()), 't2i_conv2d_bwd_data')
        _twin_keep(dx, twin, opts.out_image_written)
        if ev is not None:
            ev.record()
    return dx


def conv_bwd_filter(x, dy, d, ws_bytes, out=None, xform=None, xform_valid_rows=0, xform_plane_rows=0, accumulate=True):
    """dw = x (*) dy.  out: an existing [KH,KW,Cin,Cout]-sized buffer to ACCUMULATE into (dw += ...), e.g. the
    optimizer's gradient arena; returns it.  xform_valid_rows (with xform): the kept transform is current for that many leading images
    only — the library regenerates the rest from x, in place in `xform` (t2i_conv_opts.xform_valid_rows)."""
    _chk(x, 'x'); _chk(dy, 'dy')
    if out is not None:
        _chk(out, 'out', f32=True)
        assert out.numel() == d.KH * d.KW * d.Cin * d.Cout
        _drop_image(out)
    dw = out if out is not None else torch.empty((d.KH, d.KW, d.Cin, d.Cout), dtype=torch.float32, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, ws_bytes)
        ev = _TIMER[0].begin(conv_flops(d), conv_algo(d, 'bwd_filter')) if _TIMER[0] is not None else None
        opts = ConvOpts()
        _storage_flags(opts, x, dy, None)
        keep = _operand_images(opts, x, dy) if _h_path(d, 'bwd_filter') else None
        if xform is not None and conv_xform_bytes(d):
            opts.xform, opts.xform_bytes, opts.xform_mode = xform.data_ptr(), xform.numel() * 4, XFORM_HAVE
            opts.xform_valid_rows = int(xform_valid_rows)
            opts.xform_plane_rows = int(xform_plane_rows)       # the transform of a larger, stacked batch whose leading images are x
        # accumulate=False with out=: the slot's FIRST contribution of a step is a plain store (optim.Arena: no zero-fill, no read)
        check(lib.t2i_conv2d_bwd_filter(ctypes.byref(d), _ptr(x), _ptr(dy), _ptr(dw), 1 if (out is not None and accumulate) else 0, ctypes.byref(opts),
                                        wsp, wsn, _stream()), 't2i_conv2d_bwd_filter')
        if ev is not None:
            ev.record()
    return dw


PAIR_FWD, PAIR_BWD_DATA = header_values('PAIR_FWD', 'PAIR_BWD_DATA')


def conv_bwd_pair(first, g, w, fx, fdy, d, ws_bytes, dw_out, out_dtype=None, accumulate=True):
    """One layer's backward pair: out1 = conv^T(g, w) (first = PAIR_BWD_DATA) or conv(g, w) (PAIR_FWD), and dw_out += fx (*) fdy
    (the gradient sink).  Same results as conv_bwd_data / conv_fwd followed by conv_bwd_filter(out=dw_out); on bf16 tensors the
    two GEMMs share one launch (t2i_conv2d_bwd_pair).  Returns out1."""
    _chk(g, 'g'); _chk(w, 'w', f32=True); _chk(fx, 'fx'); _chk(fdy, 'fdy'); _chk(dw_out, 'dw_out', f32=True)
    assert dw_out.numel() == d.KH * d.KW * d.Cin * d.Cout
    _drop_image(dw_out)
    shape = (d.B, d.H, d.W, d.Cin) if first == PAIR_BWD_DATA else (d.B, d.Ho, d.Wo, d.Cout)
    out1 = torch.empty(shape, dtype=_act_dtype(shape, out_dtype), device=g.device)
    if _live(g):
        which = 'bwd_data' if first == PAIR_BWD_DATA else 'fwd'
        ws1p, ws1n = _ws_args(g, ws_bytes)
        lane0 = WS_LANE[0]
        WS_LANE[0] = PAIR_LANE + (lane0 if lane0 else (_STREAM_LANE.get(torch.cuda.current_stream(g.device).cuda_stream, 0) if _STREAM_LANE else 0))
        try:
            ws2p, ws2n = _ws_args(g, ws_bytes)            # the pair's second workspace: both GEMMs are in flight together
        finally:
            WS_LANE[0] = lane0
        ev = _TIMER[0].begin(2 * conv_flops(d), conv_algo(d, which)) if _TIMER[0] is not None else None
        o1, o2 = ConvOpts(), ConvOpts()
        _storage_flags(o1, g, None, out1)
        keep1 = _operand_images(o1, g) if _h_path(d, which) else None
        _storage_flags(o2, fx, fdy, None)
        keep2 = _operand_images(o2, fx, fdy) if _h_path(d, 'bwd_filter') else None
        check(lib.t2i_conv2d_bwd_pair(ctypes.byref(d), first, _ptr(g), _ptr(w), _ptr(out1), ctypes.byref(o1), _ptr(fx), _ptr(fdy), _ptr(dw_out), 1 if accumulate else 0,
                                      ctypes.byref(o2), ws1p, ws1n, ws2p, ws2n, _stream()), 't2i_conv2d_bwd_pair')
        del keep1, keep2
        if ev is not None:
            ev.record()
    return out1


def col_reduce(a, b=None, want_second=False, out=None, center=None):
    """a viewed as [rows, C] (C = last dim).  -> (colsum(a), colsum(a*(b - center) or a*a) or None).
    out: an existing [C] buffer to ACCUMULATE colsum(a) into (a bias slot of the gradient arena)."""
    _chk(a, 'a')
    C = a.shape[-1]
    rows = a.numel() // C
    if out is not None:
        assert out.numel() == C and not want_second
        _drop_image(out)
    out0 = out if out is not None else torch.empty(C, dtype=torch.float32, device=a.device)
    out1 = torch.empty(C, dtype=torch.float32, device=a.device) if want_second else None
    if b is not None:
        _chk(b, 'b')
        assert b.shape == a.shape
    if _live(a):
        need = int(lib.t2i_col_reduce_workspace_bytes(rows, C))
        wsp, wsn = _ws_args(a, need)
        check(lib.t2i_col_reduce(_ptr(a), _ptr(b), _ptr(_chk(center, 'center') if center is not None else None), rows, C, _ptr(out0),
                                 _ptr(out1), 1 if out is not None else 0, wsp, wsn, _same_dt(a, b), _stream()), 't2i_col_reduce')
    return out0, out1


def bn_finalize(s, ss, n, gamma, beta, eps, decay, moving_mean=None, moving_var=None):
    """s = column sums, ss = CENTRED second moments sum (x - mean)^2 (bn_stats / take_stats)."""
    C = s.numel()
    mean, rstd, scale, shift = (torch.empty(C, dtype=torch.float32, device=s.device) for _ in range(4))
    if _live(s):
        check(lib.t2i_bn_finalize(_ptr(s), _ptr(ss), n, C, _ptr(_chk(gamma)), _ptr(_chk(beta)), eps, decay, _ptr(mean),
                                  _ptr(rstd), _ptr(scale), _ptr(shift), _ptr(moving_mean), _ptr(moving_var), _stream()),
              't2i_bn_finalize')
    return mean, rstd, scale, shift


def bn_apply(x, scale, shift, act=ACT_NONE, alpha=0.2, out=None):
    """out: a contiguous tensor (view) of x's shape and dtype to write into — one group's slice of a batched pass (no bf16 twin then)."""
    _chk(x, 'x')
    C = x.shape[-1]
    if out is not None:
        assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
        _drop_image(out)
    y = out if out is not None else torch.empty_like(x)
    if _live(x):
        twin = _twin_for(y, x, scale, shift) if out is None else None
        check(lib.t2i_bn_apply(_ptr(x), _ptr(scale), _ptr(shift), x.numel() // C, C, act, alpha, _ptr(y), _ptr(twin), _dt(x), _stream()),
              't2i_bn_apply')
        _twin_keep(y, twin)
    return y


def bn_infer(x, gamma, beta, moving_mean, moving_variance, eps=1e-5, act=ACT_NONE, alpha=0.2, residual=None, res_act=ACT_NONE, res_alpha=0.2):
    """Inference batch norm in one launch (t2i_bn_infer): res_act(residual + act(x * scale + shift)) with scale / shift formed in the
    kernel from gamma, beta and the moving statistics.  residual: None, or a tensor of x's shape and dtype."""
    _chk(x, 'x')
    C = x.shape[-1]
    for name, v in (('gamma', gamma), ('beta', beta), ('moving_mean', moving_mean), ('moving_variance', moving_variance)):
        if _chk(v, name, f32=True).numel() != C:
            raise ValueError('%s has %d entries, x has %d channels' % (name, v.numel(), C))
    if residual is not None:
        _chk(residual, 'residual')
        if residual.shape != x.shape:
            raise ValueError('residual has shape %s, x has %s' % (tuple(residual.shape), tuple(x.shape)))
    y = torch.empty_like(x)
    if _live(x):
        check(lib.t2i_bn_infer(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_variance), eps, x.numel() // C, C, act, alpha,
                               _ptr(residual), res_act, res_alpha, _ptr(y), _same_dt(x, residual), _stream()), 't2i_bn_infer')
    return y


def bn_apply_groups(x, scales, shifts, act=ACT_NONE, alpha=0.2):
    """bn_apply on a batched pass: slice g of x along the batch axis is normalised with (scales[g], shifts[g]); one output tensor.
    (A wrapper of its own so that instrumentation sees one call per batch-norm layer, like every other layer of a batched pass.)"""
    groups = len(scales)
    b = x.shape[0] // groups
    y = torch.empty_like(x)
    for g in range(groups):
        _bn_apply_one(x[g * b:(g + 1) * b], scales[g], shifts[g], act, alpha, out=y[g * b:(g + 1) * b])
    return y


def bn_train_fwd_grouped(x, gamma, beta, eps, decay, groups, act=ACT_NONE, alpha=0.2, moving_mean=None, moving_var=None, moving_updates=1,
                         moving_groups=0):
    """Training-mode batch norm in at most three launches (t2i_bn_train_fwd_grouped): x [groups * b, ..., C] with per-group statistics
    (groups = 1: the ordinary batch norm).  Uses the producing conv's epilogue partials when it left any (conv_fwd_stats).
    -> (y, mean [groups, C], rstd [groups, C]); moving averages updated in place once per group, in group order."""
    _chk(x, 'x')
    C = x.shape[-1]
    rows_g = x.numel() // C // groups
    stat = torch.empty((4, groups, C), dtype=torch.float32, device=x.device)       # mean, rstd, scale, shift
    y = torch.empty_like(x)
    if _live(x):
        hit = _STATS.pop(x.data_ptr(), None)
        if hit is not None and (tuple(x.shape) != hit[3] or (groups > 1 and rows_g % hit[2] != 0) or hit[0].data_ptr() % 16 or (hit[1] * C * 4) % 16):
            hit = None
        tsum = tm2 = None
        tchunks = trows = 0
        if hit is not None:
            part, chunks, trows, _ = hit
            tsum, tm2, tchunks = ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(part.data_ptr() + chunks * C * 4), chunks // groups
        wsp, wsn = _ws_args(x, int(lib.t2i_bn_grouped_workspace_bytes(rows_g, C, groups)))
        twin = _twin_for(y, x)
        check(lib.t2i_bn_train_fwd_grouped(_ptr(x), rows_g, C, groups, _ptr(_chk(gamma)), _ptr(_chk(beta)), eps, decay, _ptr(stat[0]), _ptr(stat[1]),
                                           _ptr(stat[2]), _ptr(stat[3]), _ptr(moving_mean), _ptr(moving_var), act, alpha, _ptr(y), _ptr(twin),
                                           tsum, tm2, tchunks, trows, int(moving_updates), int(moving_groups), wsp, wsn, _dt(x), _stream()), 't2i_bn_train_fwd_grouped')
        _twin_keep(y, twin)
    return y, stat[0], stat[1]


def bn_bwd_grouped(dy, y, x, mean, rstd, gamma, groups, act, alpha=0.2, dgamma_out=None, dbeta_out=None):
    """Backward of bn_train_fwd_grouped in three launches.  mean / rstd: [groups, C].  -> (dx, dgamma, dbeta) with dgamma / dbeta summed
    over the groups; dgamma_out / dbeta_out: gradient-arena slots to ACCUMULATE into."""
    _chk(dy, 'dy'); _chk(x, 'x')
    C = x.shape[-1]
    rows_g = x.numel() // C // groups
    dx = torch.empty_like(x)
    gmask = torch.empty_like(x) if y is not None else None
    acc = dgamma_out is not None
    assert acc == (dbeta_out is not None)
    dgamma = dgamma_out if acc else torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = dbeta_out if acc else torch.empty(C, dtype=torch.float32, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, int(lib.t2i_bn_grouped_workspace_bytes(rows_g, C, groups)))
        twin = _twin_for(dx)
        check(lib.t2i_bn_bwd_grouped(_ptr(dy), _ptr(_chk(y, 'y') if y is not None else None), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(_chk(gamma)),
                                     rows_g, C, groups, act, alpha, _ptr(gmask), _ptr(dx), _ptr(twin), _ptr(dgamma), _ptr(dbeta), 1 if acc else 0,
                                     wsp, wsn, _same_dt(dy, y, x), _stream()), 't2i_bn_bwd_grouped')
        _twin_keep(dx, twin)
    return dx, dgamma, dbeta


_bn_apply_one = bn_apply          # (instrumentation replaces the public name; the per-slice calls above are not layers of their own)


def bn_bwd(dy, x, mean, rstd, gamma, sum_dy, sum_dy_x, dgamma_out=None, dbeta_out=None):
    """sum_dy_x = colsum(dy * (x - mean)) (col_reduce / act_bwd_colsum with center=mean).
    dgamma_out / dbeta_out: gradient-arena slots to ACCUMULATE into instead of fresh tensors."""
    _chk(dy, 'dy'); _chk(x, 'x')
    C = x.shape[-1]
    dx = torch.empty_like(x)
    acc = dgamma_out is not None
    assert acc == (dbeta_out is not None)
    dgamma = dgamma_out if acc else torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = dbeta_out if acc else torch.empty(C, dtype=torch.float32, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, 3 * C * 4)
        check(lib.t2i_bn_bwd(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(_chk(gamma)), _ptr(sum_dy), _ptr(sum_dy_x),
                             x.numel() // C, C, _ptr(dx), _ptr(dgamma), _ptr(dbeta), 1 if acc else 0, wsp, wsn, _stream()),
              't2i_bn_bwd')
    return dx, dgamma, dbeta


def act_fwd(x, act, alpha=0.2):
    _chk(x, 'x')
    y = torch.empty_like(x)
    if _live(x):
        twin = _twin_for(y, x)
        check(lib.t2i_act_fwd(_ptr(x), x.numel(), act, alpha, _ptr(y), _ptr(twin), _dt(x), _stream()), 't2i_act_fwd')
        _twin_keep(y, twin)
    return y


def act_bwd(dy, y, act, alpha=0.2, out=None):
    """out: an existing contiguous tensor (a slice of a stacked buffer) to write into; no bf16 twin then."""
    _chk(dy, 'dy'); _chk(y, 'y')
    if out is not None:
        assert out.shape == dy.shape and out.dtype == dy.dtype and out.is_contiguous()
        _drop_image(out)
    dx = out if out is not None else torch.empty_like(dy)
    if _live(dy):
        twin = _twin_for(dx, dy, y) if out is None else None
        check(lib.t2i_act_bwd(_ptr(dy), _ptr(y), dy.numel(), act, alpha, _ptr(dx), _ptr(twin), _same_dt(dy, y), _stream()), 't2i_act_bwd')
        _twin_keep(dx, twin)
    return dx


def act_bwd_colsum(dy, y, act, alpha=0.2, x2=None, out=None, center=None, dx_out=None):
    """-> (dx = dy*act'(y), colsum(dx)[, colsum(dx*(x2 - center))]) in one pass: a conv layer's activation backward + bias
    gradient, or (with x2 = layer input, center = its batch mean) the masked gradient and both reductions of the batch-norm backward.
    out: gradient-arena slot to ACCUMULATE colsum(dx) into (then the second return value is `out`)."""
    _chk(dy, 'dy'); _chk(y, 'y')
    C = dy.shape[-1]
    rows = dy.numel() // C
    if dx_out is not None:              # a slice of a stacked buffer to write dx into (no bf16 twin then)
        assert dx_out.shape == dy.shape and dx_out.dtype == dy.dtype and dx_out.is_contiguous()
        _drop_image(dx_out)
    dx = dx_out if dx_out is not None else torch.empty_like(dy)
    s = out if out is not None else torch.empty(C, dtype=torch.float32, device=dy.device)
    s2 = torch.empty(C, dtype=torch.float32, device=dy.device) if x2 is not None else None
    if x2 is not None:
        _chk(x2, 'x2')
        assert out is None
    if _live(dy):
        need = int(lib.t2i_col_reduce_workspace_bytes(rows, C))
        wsp, wsn = _ws_args(dy, need)
        twin = _twin_for(dx) if (x2 is None and dx_out is None) else None        # conv bias path: dx is the next input / filter gradient's operand
        check(lib.t2i_act_bwd_colsum(_ptr(dy), _ptr(y), _ptr(x2), _ptr(_chk(center, 'center') if center is not None else None), rows, C,
                                     act, alpha, _ptr(dx), _ptr(twin), _ptr(s), _ptr(s2),
                                     1 if out is not None else 0, wsp, wsn, _same_dt(dy, y, x2), _stream()), 't2i_act_bwd_colsum')
        _twin_keep(dx, twin)
    return (dx, s) if x2 is None else (dx, s, s2)


def add_act(a, b, act=ACT_NONE, alpha=0.2):
    _chk(a, 'a'); _chk(b, 'b')
    assert a.shape == b.shape
    y = torch.empty_like(a)
    if _live(a):
        twin = _twin_for(y, a, b)
        check(lib.t2i_add_act(_ptr(a), _ptr(b), a.numel(), act, alpha, _ptr(y), _ptr(twin), _same_dt(a, b), _stream()), 't2i_add_act')
        _twin_keep(y, twin)
    return y


def _drop_image(t):
    """A wrapper wrote `t` through its raw pointer: tensor._version does not move, so a bf16 image cached on it would be stale."""
    if t is not None:
        h = _image_holder(t)
        if getattr(h, '_t2i_h', None) is not None:
            h._t2i_h = None


def axpby(a, alpha, b=None, beta=0.0, out=None):
    """out: an existing tensor to overwrite (its cached bf16 image, if any, is dropped — see bf16_image)."""
    _chk(a, 'a')
    y = torch.empty_like(a) if out is None else out
    _drop_image(out)
    if _live(a):
        check(lib.t2i_axpby(_ptr(a), alpha, _ptr(_chk(b, 'b') if b is not None else None), beta, a.numel(), _ptr(y),
                            _same_dt(a, b, y), _stream()), 't2i_axpby')
    return y


def interp(eps, g, x, out=None):
    """out: an existing contiguous tensor of g's shape to write into (the x_hat slot of the stacked critic input)."""
    _chk(g, 'g', f32=True); _chk(x, 'x', f32=True)           # the 3-channel image side is float32 in every storage mode
    eps = _chk(eps.reshape(-1), 'eps', f32=True)
    B = g.shape[0]
    assert eps.numel() == B and g.shape == x.shape
    if out is not None:
        _chk(out, 'out', f32=True)
        assert out.shape == g.shape
        _drop_image(out)
    else:
        out = torch.empty_like(g)
    if _live(g):
        check(lib.t2i_interp(_ptr(eps), _ptr(g), _ptr(x), B, g.numel() // B, _ptr(out), _stream()), 't2i_interp')
    return out


def concat_tile_fwd(feat, emb):
    """feat [B,H,W,Cf], emb [B,Ce] -> [B,H,W,Cf+Ce]"""
    _chk(feat, 'feat'); _chk(emb, 'emb')
    B, H, W, Cf = feat.shape
    Ce = emb.shape[1]
    out = torch.empty((B, H, W, Cf + Ce), dtype=feat.dtype, device=feat.device)
    if _live(feat):
        check(lib.t2i_concat_tile_fwd(_ptr(feat), _ptr(emb), B, H * W, Cf, Ce, _ptr(out), _same_dt(feat, emb), _stream()), 't2i_concat_tile_fwd')
    return out


def concat_tile_bwd(dout, Cf, Ce):
    _chk(dout, 'dout')
    B, H, W, Ct = dout.shape
    assert Ct == Cf + Ce
    dfeat = torch.empty((B, H, W, Cf), dtype=dout.dtype, device=dout.device)
    demb = torch.empty((B, Ce), dtype=dout.dtype, device=dout.device)
    if _live(dout):
        check(lib.t2i_concat_tile_bwd(_ptr(dout), B, H * W, Cf, Ce, _ptr(dfeat), _ptr(demb), _dt(dout), _stream()), 't2i_concat_tile_bwd')
    return dfeat, demb


def nchw_to_nhwc(x):
    """x physically [B,C,H,W] contiguous -> physically [B,H,W,C] contiguous"""
    _chk(x, 'x')
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device)
    if _live(x):
        check(lib.t2i_nchw_to_nhwc(_ptr(x), B, C, H * W, _ptr(y), _dt(x), _stream()), 't2i_nchw_to_nhwc')
    return y


def nhwc_to_nchw(x):
    _chk(x, 'x')
    B, H, W, C = x.shape
    y = torch.empty((B, C, H, W), dtype=x.dtype, device=x.device)
    if _live(x):
        check(lib.t2i_nhwc_to_nchw(_ptr(x), B, C, H * W, _ptr(y), _dt(x), _stream()), 't2i_nhwc_to_nchw')
    return y


def gp_slopes(g):
    _chk(g, 'g')
    B = g.shape[0]
    s = torch.empty(B, dtype=torch.float32, device=g.device)
    if _live(g):
        check(lib.t2i_gp_slopes(_ptr(g), B, g.numel() // B, _ptr(s), _dt(g), _stream()), 't2i_gp_slopes')
    return s


def row_scale(g, coef):
    _chk(g, 'g'); _chk(coef, 'coef', f32=True)
    B = g.shape[0]
    assert coef.numel() == B
    out = torch.empty_like(g)
    if _live(g):
        check(lib.t2i_row_scale(_ptr(g), _ptr(coef), B, g.numel() // B, _ptr(out), _dt(g), _stream()), 't2i_row_scale')
    return out


def row_scale_div(g, num, den):
    """out[b] = (den[b] > 0 ? num[b] / max(den[b], 1e-30) : 0) * g[b]: the slope norm's backward, coefficient formed in the kernel."""
    _chk(g, 'g'); _chk(num, 'num', f32=True); _chk(den, 'den', f32=True)
    B = g.shape[0]
    assert num.numel() == B and den.numel() == B
    out = torch.empty_like(g)
    if _live(g):
        check(lib.t2i_row_scale_div(_ptr(g), _ptr(num), _ptr(den), B, g.numel() // B, _ptr(out), _dt(g), _stream()), 't2i_row_scale_div')
    return out


def _adam_chk(w, g, m, v, beta1, ema=None):
    """What the three Adam wrappers check of their arenas (m and ema may be None)."""
    for t in (w, g, v) + ((m,) if m is not None else ()):
        _chk(t)
    if ema is not None:
        _chk(ema, 'ema', f32=True)
    assert w.numel() == g.numel() == v.numel() and (m is None or m.numel() == w.numel()) and (ema is None or ema.numel() == w.numel())
    assert m is not None or beta1 == 0.0, 'the first moment can be skipped only with beta1 == 0'


def adam_tf(w, g, m, v, lr_t, beta1, beta2, eps=1e-8, grad_scale=1.0, lr_t_dev=None):
    """In place on flat arenas.  lr_t_dev: optional device scalar that overrides lr_t (graph replay)."""
    _adam_chk(w, g, m, v, beta1)
    if _live(w):
        check(lib.t2i_adam_tf(_ptr(w), _ptr(g), _ptr(m), _ptr(v), w.numel(), lr_t, _ptr(lr_t_dev), beta1, beta2, eps, grad_scale,
                              _stream()),
              't2i_adam_tf')


def adam_tf_ema(w, g, m, v, ema, lr_t, beta1, beta2, eps=1e-8, grad_scale=1.0, ema_decay=0.999, lr_t_dev=None, ema_decay_dev=None):
    """adam_tf plus the exponential moving average of the updated weights in the same launch: ema -= (1 - decay) * (ema - w_new).
    ema_decay_dev: optional device scalar that overrides ema_decay (graph replay)."""
    _chk(ema, 'ema', f32=True)          # required here: None is an error
    _adam_chk(w, g, m, v, beta1, ema)
    if _live(w):
        check(lib.t2i_adam_tf_ema(_ptr(w), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), w.numel(), lr_t, _ptr(lr_t_dev), beta1, beta2, eps,
                                  grad_scale, ema_decay, _ptr(ema_decay_dev), _stream()),
              't2i_adam_tf_ema')


ADAM_MAX_SLOTS = CONSTANTS['T2I_ADAM_MAX_SLOTS']


def adam_tf_slots(w, g, m, v, slot_end, slot_mult, lr_t, beta1, beta2, eps=1e-8, grad_scale=1.0, ema=None, ema_decay=0.999, lr_t_dev=None,
                  ema_decay_dev=None):
    """adam_tf (ema=None) / adam_tf_ema with two multipliers per arena slot: slot s, ending at element slot_end[s] (device int64
    [n_slots], ascending multiples of 4, the last == w.numel()), steps with grad_scale * slot_mult[s, 0] and lr_t * slot_mult[s, 1]
    (device float32 [n_slots, 2]).  All ones: the bits of adam_tf / adam_tf_ema."""
    _adam_chk(w, g, m, v, beta1, ema)
    _chk(slot_mult, 'slot_mult', f32=True)
    if slot_end.dtype != torch.int64:
        raise TypeError('slot_end must be int64, got %s' % slot_end.dtype)
    if not slot_end.is_contiguous():
        raise ValueError('slot_end must be contiguous (shape %s, strides %s)' % (tuple(slot_end.shape), slot_end.stride()))
    assert slot_end.dim() == 1 and slot_mult.numel() == 2 * slot_end.numel() and slot_end.device == w.device == slot_mult.device
    if _live(w):
        check(lib.t2i_adam_tf_slots(_ptr(w), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), w.numel(), _ptr(slot_end), _ptr(slot_mult),
                                    int(slot_end.numel()), lr_t, _ptr(lr_t_dev), beta1, beta2, eps, grad_scale, ema_decay,
                                    _ptr(ema_decay_dev), _stream()),
              't2i_adam_tf_slots')


# ---- spectral normalisation of the matrices of an arena (csrc/t2i_spectral.hip) -----------------------------
SPECTRAL_MAX_SLOTS, SPECTRAL_MAX_ITEMS, SPECTRAL_MAX_ITERATIONS, SPECTRAL_COLS = header_values(
    'SPECTRAL_MAX_SLOTS', 'SPECTRAL_MAX_ITEMS', 'SPECTRAL_MAX_ITERATIONS', 'SPECTRAL_COLS')


def spectral_items(R, C):
    """(rows per work item, work items) of an [R, C] matrix: the cut of csrc/t2i_spectral.hip, a function of (R, C) alone."""
    rb = min(R, max(1, min(8192 // C, 2048)))
    return rb, (R + rb - 1) // rb


class SpectralTable(object):
    """The validated slot table of spectral_grad_ / spectral_normalize: `host` the int64 rows (off, R, C, u_off, v_off, part_off,
    iterate), `dev` their copy on the device, and the sizes the entries are told.  Made by spectral_table() only: the kernels form
    addresses from the rows, so no row reaches the device before it passed the checks there."""

    def __init__(self, host, dev, numel, nu, nv, max_items, part_floats):
        self.host, self.dev, self.numel, self.nu, self.nv, self.max_items, self.part_floats = host, dev, numel, nu, nv, max_items, part_floats
        self.max_col_blocks = max((int(C) + 63) // 64 for C in host[:, 2])
        self.n_slots = int(host.shape[0])
        self.ws_floats = (part_floats * 4 + 255) // 256 * 256 // 4          # t2i_spectral_workspace_bytes(part_floats) / 4

    def only(self, rows):
        """The same table with the power iteration advancing the given rows alone (every slot still takes part in flat = raw / sigma)."""
        host = self.host.copy()
        host[:, 6] = 0
        host[list(rows), 6] = 1
        return SpectralTable(host, torch.from_numpy(host).to(self.dev.device), self.numel, self.nu, self.nv, self.max_items, self.part_floats)


def spectral_table(slots, numel, device):
    """slots: one (offset, slot elements, R, C) per normalised variable in arena order; numel: the arena's size.  Lays u, v and the
    partial sums out in 16-byte slots and validates every row: R * C equal to the slot's element count, the slots inside the arena,
    ascending and apart, 4-element aligned."""
    name = 'spectral_table'
    slots = [tuple(int(x) for x in s) for s in slots]
    if not 1 <= len(slots) <= SPECTRAL_MAX_SLOTS:
        raise ValueError('%s: %d slots, one launch takes 1..%d' % (name, len(slots), SPECTRAL_MAX_SLOTS))
    if numel <= 0 or numel % 4:
        raise ValueError('%s: the arena has %d elements, not a positive multiple of 4' % (name, numel))
    rows, uo, vo, po, prev_end, max_items = [], 0, 0, 0, 0, 1
    for off, k, R, C in slots:
        if R < 1 or C < 1 or R >= 1 << 30 or C >= 1 << 30 or R * C != k:
            raise ValueError('%s: a slot of %d elements cannot be the matrix [%d, %d]' % (name, k, R, C))
        if off % 4 or off < prev_end or off + k > numel:
            raise ValueError('%s: the slot at %d (%d elements) is misaligned, outside the arena of %d elements, out of order or overlaps '
                             'the slot before it (which ends at %d)' % (name, off, k, numel, prev_end))
        prev_end = off + (k + 3) // 4 * 4
        items = spectral_items(R, C)[1]
        if items > SPECTRAL_MAX_ITEMS:
            raise ValueError('%s: the matrix [%d, %d] has %d work items, a launch takes at most %d' % (name, R, C, items, SPECTRAL_MAX_ITEMS))
        max_items = max(max_items, items)
        rows.append((off, R, C, uo, vo, po, 1))
        uo += (C + 3) // 4 * 4
        vo += (R + 3) // 4 * 4
        po += (items * C + items + (C + 63) // 64 + 3) // 4 * 4          # column partials, the items' |t|^2, the column blocks' |s|^2
    host = np.asarray(rows, dtype=np.int64).reshape(len(rows), SPECTRAL_COLS)
    return SpectralTable(host, torch.from_numpy(host).to(device), int(numel), uo, vo, max_items, po)


def _spectral_chk(name, tab, arenas, u, v, sigma, ws):
    if not isinstance(tab, SpectralTable):
        raise TypeError('%s: the table must come from spectral_table(), got %r' % (name, type(tab).__name__))
    for label, t in arenas + (('u', u), ('v', v), ('sigma', sigma), ('workspace', ws)):
        _chk(t, label, f32=True)
        if t.device != tab.dev.device:
            raise ValueError('%s: %s is on %s, the table on %s' % (name, label, t.device, tab.dev.device))
    for label, t in arenas:
        if t.numel() != tab.numel:
            raise ValueError('%s: %s has %d elements, the table was built for an arena of %d' % (name, label, t.numel(), tab.numel))
    if u.numel() != tab.nu or v.numel() != tab.nv or sigma.numel() != tab.n_slots or ws.numel() < tab.ws_floats:
        raise ValueError('%s: u, v, sigma and the workspace must have %d, %d, %d and at least %d elements, got %d, %d, %d and %d' % (
            name, tab.nu, tab.nv, tab.n_slots, tab.ws_floats, u.numel(), v.numel(), sigma.numel(), ws.numel()))


def spectral_grad_(grad, flat, tab, u, v, sigma, ws):
    """In place on the gradient arena: inside every slot of `tab`, grad <- (grad - <grad, flat> v u^T) / sigma — the chain rule from
    dL/dW to dL/draw of W = raw / sigma with u and v constant.  Two launches, sums in a fixed order."""
    _spectral_chk('spectral_grad_', tab, (('grad', grad), ('flat', flat)), u, v, sigma, ws)
    if _live(grad):
        check(lib.t2i_spectral_grad(_ptr(grad), _ptr(flat), tab.numel, _ptr(tab.dev), tab.n_slots, tab.max_items, _ptr(u), tab.nu, _ptr(v), tab.nv,
                                    _ptr(sigma), tab.part_floats, _ptr(ws), ws.numel() * 4, _stream()), 't2i_spectral_grad')


def spectral_normalize(flat, raw, tab, u, v, sigma, ws, iterations=1):
    """`iterations` power iterations on the matrices of `raw` that `tab` marks (u, v, sigma in place), then flat = raw / sigma inside
    every slot and flat = raw elsewhere.  iterations = 0 only rewrites flat from the stored sigma.  3 * iterations + 1 launches."""
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= SPECTRAL_MAX_ITERATIONS:
        raise ValueError('spectral_normalize: iterations must be an integer in 0..%d, got %r' % (SPECTRAL_MAX_ITERATIONS, iterations))
    _spectral_chk('spectral_normalize', tab, (('flat', flat), ('raw', raw)), u, v, sigma, ws)
    if _live(flat):
        check(lib.t2i_spectral_normalize(_ptr(flat), _ptr(raw), tab.numel, _ptr(tab.dev), tab.n_slots, tab.max_items, tab.max_col_blocks, _ptr(u), tab.nu, _ptr(v),
                                         tab.nv, _ptr(sigma), iterations, tab.part_floats, _ptr(ws), ws.numel() * 4, _stream()),
              't2i_spectral_normalize')


def device_info(device=0):
    cu, clk = ctypes.c_int32(0), ctypes.c_int32(0)
    arch = ctypes.create_string_buffer(64)
    check(lib.t2i_device_info(device, ctypes.byref(cu), ctypes.byref(clk), arch, 64), 't2i_device_info')
    return dict(cu_count=cu.value, clock_khz=clk.value, arch=arch.value.decode())


# ---- data pipeline (reference preprocess/dataset.py) --------------------------------------------------------------------
def crop_flip_normalize(src_u8, ids, row0, col0, flip, out_size):
    """src_u8 [N,S,S,3] uint8 (device); ids/row0/col0/flip int32 [B] (device) -> float32 [B,out_size,out_size,3]."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or src_u8.shape[1] != src_u8.shape[2]:
        raise ValueError('crop_flip_normalize expects a uint8 [N,S,S,3] store, got %s %s' % (src_u8.dtype, tuple(src_u8.shape)))
    B = ids.numel()
    out = torch.empty((B, out_size, out_size, 3), dtype=torch.float32, device=src_u8.device)
    if _live(src_u8):
        a, b, c, d = ids.to(torch.int32).contiguous(), row0.to(torch.int32).contiguous(), col0.to(torch.int32).contiguous(), flip.to(torch.int32).contiguous()
        check(lib.t2i_crop_flip_normalize(_ptr(src_u8.contiguous()), src_u8.shape[0], src_u8.shape[1], _ptr(a), _ptr(b), _ptr(c),
                                          _ptr(d), B, out_size, _ptr(out), _stream()), 't2i_crop_flip_normalize')
    return out


def nearest_images(src_u8, queries, row0=None, col0=None, flip=None, lo=-1.0, hi=1.0):
    """Closest stored image of each query (reference utils/visualize.py closest_image, one launch for all of them).
    src_u8 [N,S,S,3] uint8 (device); queries float32 [Q,out,out,3], clipped to [lo, hi] inside; row0/col0/flip int [Q,N]: the crop
    of image n that query q is compared with (all None: the identity crop, S == out).  -> (idx int64 [Q], dist2 float64 [Q]):
    the lowest index of minimal squared distance, accumulated in fp64."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or src_u8.shape[1] != src_u8.shape[2]:
        raise ValueError('nearest_images expects a uint8 [N,S,S,3] store, got %s %s' % (src_u8.dtype, tuple(src_u8.shape)))
    if queries.dtype != torch.float32 or queries.dim() != 4 or queries.shape[3] != 3 or queries.shape[1] != queries.shape[2]:
        raise ValueError('nearest_images expects float32 [Q,out,out,3] queries, got %s %s' % (queries.dtype, tuple(queries.shape)))
    N, S = src_u8.shape[0], src_u8.shape[1]
    Q, out = queries.shape[0], queries.shape[1]
    tables = (row0, col0, flip)
    if any(t is None for t in tables) != all(t is None for t in tables):
        raise ValueError('nearest_images: pass all three crop tables or none')
    if row0 is None and out != S:
        raise ValueError('nearest_images: without crop tables the queries must be %dx%d like the store, got %dx%d' % (S, S, out, out))
    if row0 is not None and any(tuple(t.shape) != (Q, N) for t in tables):
        raise ValueError('nearest_images: crop tables must be [Q, N] = [%d, %d], got %s' % (Q, N, [tuple(t.shape) for t in tables]))
    idx = torch.empty(Q, dtype=torch.int32, device=src_u8.device)
    dist2 = torch.empty(Q, dtype=torch.float64, device=src_u8.device)
    if _live(src_u8):
        tabs = [t.to(device=src_u8.device, dtype=torch.int32).contiguous() if t is not None else None for t in tables]
        wsp, wsn = _ws_args(src_u8, int(lib.t2i_nearest_images_workspace_bytes(Q, N)))
        check(lib.t2i_nearest_images(_ptr(src_u8.contiguous()), N, S, *[_ptr(t) for t in tabs], _ptr(queries.contiguous()), Q, out,
                                     float(lo), float(hi), _ptr(idx), _ptr(dist2), wsp, wsn, _stream()), 't2i_nearest_images')
    return idx.long(), dist2


def bytescale_nearest(x, size):
    """The reference's scipy.misc.imresize(float_image, (size, size), interp='nearest') before its / 127.5 - 1, for a batch
    (t2i_bytescale_nearest): per image scipy's bytescale of (x + 1) * 127.5 (the image's own min -> 0 and max -> 255, + 0.5,
    truncated) and Pillow's NEAREST resize, bit for bit.  x float32 [N,h,w,C] (device, finite values, C in 1..4) -> uint8
    [N,size,size,C]."""
    if x.dtype != torch.float32 or x.dim() != 4 or not 1 <= x.shape[3] <= 4:
        raise ValueError('bytescale_nearest expects a float32 [N,h,w,C] batch with C in 1..4, got %s %s' % (x.dtype, tuple(x.shape)))
    N, h, w, C = (int(s) for s in x.shape)
    size = int(size)
    if min(N, h, w) <= 0 or size <= 0:
        raise ValueError('bytescale_nearest: empty batch, image or output (x %s, size %d)' % (tuple(x.shape), size))
    y = torch.empty((N, size, size, C), dtype=torch.uint8, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, int(lib.t2i_bytescale_nearest_workspace_bytes(N, h, w, C)))
        check(lib.t2i_bytescale_nearest(_ptr(x.contiguous()), N, h, w, C, size, _ptr(y), wsp, wsn, _stream()), 't2i_bytescale_nearest')
    return y


# ---- evaluator: Inception score and FID (reference evaluation/, utils/utils.py prep_incep_img) -------------------------------
_RESAMPLE_TABLES = {}


def _resample_tables(Hi, Wi, Ho, Wo, device, filter='bilinear'):
    key = (Hi, Wi, Ho, Wo, str(device), filter)
    hit = _RESAMPLE_TABLES.get(key)
    if hit is None:
        from .evaluation import resize
        tables = {'bilinear': resize.bilinear_tables, 'bicubic': resize.bicubic_tables}[filter]
        (xb, xk), (yb, yk) = tables(Wi, Wo), tables(Hi, Ho)
        hit = _RESAMPLE_TABLES[key] = tuple(torch.from_numpy(t).to(device) for t in (xb, xk, yb, yk))
    return hit


def resample_bilinear(src, Ho, Wo, rows=None, out_u8=False, out=None):
    """Pillow's bilinear Image.resize of a batch, bit for bit, then u / 127.5 - 1 (prep_incep_img).  src [N,Hi,Wi,3]: uint8, or
    float32 generator output in [-1, 1] read as ((x + 1) * 127.5).astype(uint8) (denormalize_images).  rows int [B]: the store
    rows to take, in order (None: all N).  -> float32 [B,Ho,Wo,3] in [-1, 1], or the uint8 pixels with out_u8 (written into `out`
    if given: contiguous, that shape and dtype)."""
    if src.dtype not in (torch.uint8, torch.float32) or src.dim() != 4 or src.shape[3] != 3:
        raise ValueError('resample_bilinear expects a uint8 or float32 [N,H,W,3] store, got %s %s' % (src.dtype, tuple(src.shape)))
    if not src.is_contiguous():
        raise ValueError('resample_bilinear: the store must be contiguous')
    N, Hi, Wi = src.shape[0], src.shape[1], src.shape[2]
    B = N if rows is None else rows.numel()
    shape, dt = (B, Ho, Wo, 3), torch.uint8 if out_u8 else torch.float32
    y = torch.empty(shape, dtype=dt, device=src.device) if out is None else out
    if tuple(y.shape) != shape or y.dtype != dt or not y.is_contiguous() or y.device != src.device:
        raise ValueError('resample_bilinear: out must be a contiguous %s %s on %s' % (dt, shape, src.device))
    if _live(src) and B > 0:
        xb, xk, yb, yk = _resample_tables(Hi, Wi, Ho, Wo, src.device)
        r = rows.to(device=src.device, dtype=torch.int32).contiguous() if rows is not None else None
        wsp, wsn = _ws_args(src, int(lib.t2i_resample_bilinear_workspace_bytes(B, Hi, Wo)))
        check(lib.t2i_resample_bilinear(_ptr(src), int(src.dtype == torch.float32), N, Hi, Wi, _ptr(r), B, Ho, Wo, _ptr(xb), _ptr(xk),
                                        xk.shape[1], _ptr(yb), _ptr(yk), yk.shape[1], _ptr(y), int(out_u8), wsp, wsn, _stream()),
              't2i_resample_bilinear')
    return y


def resample_u8(src, Ho, Wo, filter='bicubic', rows=None, out=None):
    """Pillow's 8-bit Image.resize of a uint8 store [N,Hi,Wi,3] with BICUBIC (or BILINEAR) filtering, bit for bit: the
    t2i_resample_bilinear launch with the filter's tables (evaluation/resize.py; the kernel takes any tap count and clips the
    8-bit intermediate, which the negative bicubic lobes need).  rows int [B]: the store rows to take, in order (None: all N).
    -> uint8 [B,Ho,Wo,3] (written into `out` if given)."""
    if filter not in ('bicubic', 'bilinear'):
        raise ValueError("resample_u8: filter must be 'bicubic' or 'bilinear', got %r" % (filter,))
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
        raise ValueError('resample_u8 expects a uint8 [N,H,W,3] store, got %s %s' % (src.dtype, tuple(src.shape)))
    if not src.is_contiguous():
        raise ValueError('resample_u8: the store must be contiguous')
    N, Hi, Wi = src.shape[0], src.shape[1], src.shape[2]
    B = N if rows is None else rows.numel()
    shape = (B, Ho, Wo, 3)
    y = torch.empty(shape, dtype=torch.uint8, device=src.device) if out is None else out
    if tuple(y.shape) != shape or y.dtype != torch.uint8 or not y.is_contiguous() or y.device != src.device:
        raise ValueError('resample_u8: out must be a contiguous uint8 %s on %s' % (shape, src.device))
    if _live(src) and B > 0:
        xb, xk, yb, yk = _resample_tables(Hi, Wi, Ho, Wo, src.device, filter)
        r = rows.to(device=src.device, dtype=torch.int32).contiguous() if rows is not None else None
        wsp, wsn = _ws_args(src, int(lib.t2i_resample_bilinear_workspace_bytes(B, Hi, Wo)))
        check(lib.t2i_resample_bilinear(_ptr(src), 0, N, Hi, Wi, _ptr(r), B, Ho, Wo, _ptr(xb), _ptr(xk), xk.shape[1], _ptr(yb),
                                        _ptr(yk), yk.shape[1], _ptr(y), 1, wsp, wsn, _stream()), 't2i_resample_bilinear')
    return y


def pillow_tables(in_sizes, out_size, filter='bicubic', kmax=None):
    """Pillow's resize tables formed on the device in fp64 (t2i_pillow_tables): in_sizes int32 [N] (device), one axis each,
    resized to out_size -> (bounds int32 [N,out_size,2], coeffs int32 [N,out_size,kmax]), equal to evaluation/resize.py's
    bicubic_tables / bilinear_tables (coeffs zero beyond an axis' own tap count).  kmax None: what the largest axis needs."""
    if filter not in ('bicubic', 'bilinear'):
        raise ValueError("pillow_tables: filter must be 'bicubic' or 'bilinear', got %r" % (filter,))
    if in_sizes.dtype != torch.int32 or in_sizes.dim() != 1 or in_sizes.numel() == 0 or not in_sizes.is_contiguous():
        raise ValueError('pillow_tables expects a contiguous int32 [N] tensor of axis sizes, got %s %s' % (in_sizes.dtype, tuple(in_sizes.shape)))
    N, out_size = in_sizes.numel(), int(out_size)
    if out_size <= 0:
        raise ValueError('pillow_tables: out_size must be positive, got %d' % out_size)
    if kmax is None:
        from .evaluation import resize
        big = max(int(in_sizes.max()), 1)
        kmax = {'bicubic': resize.bicubic_tables, 'bilinear': resize.bilinear_tables}[filter](big, out_size)[1].shape[1]
    bounds = torch.empty((N, out_size, 2), dtype=torch.int32, device=in_sizes.device)
    coeffs = torch.empty((N, out_size, int(kmax)), dtype=torch.int32, device=in_sizes.device)
    if _live(in_sizes):
        check(lib.t2i_pillow_tables(int(filter == 'bicubic'), _ptr(in_sizes), N, out_size, _ptr(bounds), _ptr(coeffs), int(kmax),
                                    _stream()), 't2i_pillow_tables')
    return bounds, coeffs


def image_descs(rows):
    """rows: N x (offset, height, width, channels, y1, y2, x1, x2) integers -> the ctypes array t2i_preprocess_images reads."""
    rows = [tuple(int(v) for v in r) for r in rows]
    if not rows or any(len(r) != 8 for r in rows):
        raise ValueError('image_descs expects N >= 1 rows of (offset, height, width, channels, y1, y2, x1, x2)')
    return (ImageDesc * len(rows))(*[ImageDesc(*r, 0) for r in rows])


def preprocess_images(packed, descs, size):
    """The reference's load-size transform of a ragged batch in one call (t2i_preprocess_images): per image colorize and crop by
    addressing, scipy's bytescale of the crop (its own min -> 0, max -> 255) and Pillow's 8-bit BICUBIC resize to size x size, bit
    for bit with preprocess/utils.py transform.  packed: uint8 [bytes] (device), the decoded images back to back; descs: N rows
    of (offset, height, width, channels, y1, y2, x1, x2) — image n is uint8 [height, width, channels] at packed[offset:], channels
    1, 3 or 4, and rows y1:y2, columns x1:x2 of it are taken.  -> uint8 [N,size,size,3]."""
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError('preprocess_images expects a contiguous uint8 [bytes] buffer, got %s %s' % (packed.dtype, tuple(packed.shape)))
    d = descs if isinstance(descs, ctypes.Array) else image_descs(descs)
    N, size = len(d), int(size)
    if size <= 0:
        raise ValueError('preprocess_images: size must be positive, got %d' % size)
    y = torch.empty((N, size, size, 3), dtype=torch.uint8, device=packed.device)
    if _live(packed):
        rows = max(sum(r.y2 - r.y1 for r in d), 1)
        side = max(max(max(r.y2 - r.y1, r.x2 - r.x1) for r in d), 1)
        wsp, wsn = _ws_args(packed, int(lib.t2i_preprocess_images_workspace_bytes(N, rows, side, size)))
        check(lib.t2i_preprocess_images(_ptr(packed), packed.numel(), ctypes.cast(d, ctypes.c_void_p), N, size, _ptr(y), wsp, wsn,
                                        _stream()), 't2i_preprocess_images')
    return y


POOL_MAX, POOL_AVG = header_values('POOL_MAX', 'POOL_AVG')


def pool_out_size(n, k, s, padding):
    """TF's output extent of a pooling window (and of a conv)."""
    if padding.upper() == 'SAME':
        return -(-n // s)
    if padding.upper() == 'VALID':
        return (n - k) // s + 1
    raise ValueError('Invalid padding %s' % padding)


def pool2d(x, KH, KW, SH, SW, padding, op, out=None, c0=0):
    """TF max_pool / avg_pool of x [B,H,W,C] float32.  out None: a new [B,Ho,Wo,C]; else a contiguous [B,Ho,Wo,ld] float32 whose
    channels [c0, c0 + C) receive the result (one branch of a concatenation).  -> the written tensor."""
    _chk(x, 'x', f32=True)
    B, H, W, C = x.shape
    Ho, Wo = pool_out_size(H, KH, SH, padding), pool_out_size(W, KW, SW, padding)
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    elif tuple(out.shape[:3]) != (B, Ho, Wo) or out.dim() != 4 or c0 + C > out.shape[3]:
        raise ValueError('pool2d: output %s cannot take [%d,%d,%d] x %d channels at %d' % (tuple(out.shape), B, Ho, Wo, C, c0))
    _chk(out, 'out', f32=True)
    if _live(x):
        check(lib.t2i_pool2d(_ptr(x), B, H, W, C, KH, KW, SH, SW, int(padding.upper() == 'SAME'), op, _ptr(out), out.shape[3], c0,
                             _stream()), 't2i_pool2d')
    return out


def channel_slice_copy(x, out, c0):
    """x [..., C] float32 into channels [c0, c0 + C) of out [..., ld] (same leading shape): a concatenation branch."""
    _chk(x, 'x', f32=True); _chk(out, 'out', f32=True)
    C, ld = x.shape[-1], out.shape[-1]
    if tuple(x.shape[:-1]) != tuple(out.shape[:-1]) or c0 < 0 or c0 + C > ld:
        raise ValueError('channel_slice_copy: %s into channels %d.. of %s' % (tuple(x.shape), c0, tuple(out.shape)))
    rows = x.numel() // C
    if _live(x) and rows > 0:
        check(lib.t2i_channel_slice_copy(_ptr(x), rows, C, _ptr(out), ld, c0, _stream()), 't2i_channel_slice_copy')
    return out


def gram_accumulate(X, s, sum64, G64):
    """sum64 [d] += sum_k (X[k] - s) and G64 [d,d] += (X - s)^T (X - s), fp64 accumulators, X [n,d] and s [d] float32."""
    _chk(X, 'X', f32=True); _chk(s, 's', f32=True)
    n, d = X.shape
    if tuple(s.shape) != (d,) or tuple(sum64.shape) != (d,) or tuple(G64.shape) != (d, d) or sum64.dtype != torch.float64 or \
            G64.dtype != torch.float64 or not (sum64.is_contiguous() and G64.is_contiguous()):
        raise ValueError('gram_accumulate: X %s, s %s, sum %s %s, G %s %s' % (tuple(X.shape), tuple(s.shape), sum64.dtype,
                                                                           tuple(sum64.shape), G64.dtype, tuple(G64.shape)))
    if _live(X) and n > 0:
        wsp, wsn = _ws_args(X, int(lib.t2i_gram_accumulate_workspace_bytes(n, d)))
        check(lib.t2i_gram_accumulate(_ptr(X), n, d, _ptr(s), _ptr(sum64), _ptr(G64), wsp, wsn, _stream()), 't2i_gram_accumulate')
    return sum64, G64


def cosine_distance(a, b, out=None):
    """IMD's per-pair distance: a, b float32 [n, d] (rows may be strided, columns contiguous) -> float64 [n] with
    out[i] = clip(1 - a_i.b_i / sqrt(|a_i|^2 |b_i|^2), 0, 2), NaN for a zero row (scipy.spatial.distance.cosine)."""
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or tuple(a.shape) != tuple(b.shape):
        raise ValueError('cosine_distance expects two float32 [n, d] tensors of one shape, got %s %s and %s %s' % (
            a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    if a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError('cosine_distance: the columns must be contiguous (strides %s, %s)' % (a.stride(), b.stride()))
    n, d = a.shape
    y = torch.empty(n, dtype=torch.float64, device=a.device) if out is None else out
    if tuple(y.shape) != (n,) or y.dtype != torch.float64 or not y.is_contiguous() or y.device != a.device:
        raise ValueError('cosine_distance: out must be a contiguous float64 [%d] on %s' % (n, a.device))
    if _live(a) and n > 0:
        check(lib.t2i_cosine_distance(_ptr(a), a.stride(0), _ptr(b), b.stride(0), n, d, _ptr(y), _stream()), 't2i_cosine_distance')
    return y


def gather_mean(emb, ids, choice):
    """emb [N,En,D] float32; ids int32 [B]; choice int32 [B,k] -> [B,D] mean of the chosen rows, in choice order."""
    _chk(emb, 'emb')
    B, k = choice.shape
    out = torch.empty((B, emb.shape[2]), dtype=torch.float32, device=emb.device)
    if _live(emb):
        a, c = ids.to(torch.int32).contiguous(), choice.to(torch.int32).contiguous()
        check(lib.t2i_gather_mean(_ptr(emb), emb.shape[0], emb.shape[1], emb.shape[2], _ptr(a), _ptr(c), B, k, _ptr(out), _stream()),
              't2i_gather_mean')
    return out


# ---- PGGAN operators (reference utils/ops.py:74-81,100-101,109-111) ------------------------------------------------------
def pool2_sum(x, scale):
    """x [B,H,W,C] (H, W even) -> scale * 2x2 window sums [B,H/2,W/2,C]."""
    _chk(x, 'x')
    B, H, W, C = x.shape
    if H % 2 or W % 2:
        raise ValueError('pool(x, 2): odd extents %dx%d are not supported (the reference only pools powers of two)' % (H, W))
    y = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    if _live(x):
        check(lib.t2i_pool2_sum(_ptr(x), B, H, W, C, scale, _ptr(y), _stream()), 't2i_pool2_sum')
    return y


def upscale2(x, scale=1.0):
    """x [B,H,W,C] -> scale * nearest-neighbour x2 [B,2H,2W,C]."""
    _chk(x, 'x')
    B, H, W, C = x.shape
    y = torch.empty((B, 2 * H, 2 * W, C), dtype=torch.float32, device=x.device)
    if _live(x):
        check(lib.t2i_upscale2(_ptr(x), B, H, W, C, scale, _ptr(y), _stream()), 't2i_upscale2')
    return y


def row_moments(a, b=None):
    """a (and b) [B, ...] -> (sum over everything but axis 0 of a, of a*b or a*a)."""
    _chk(a, 'a')
    B = a.shape[0]
    s1 = torch.empty(B, dtype=torch.float32, device=a.device); s2 = torch.empty_like(s1)
    if _live(a):
        wsp, wsn = _ws_args(a, int(lib.t2i_row_moments_workspace_bytes(B)))
        check(lib.t2i_row_moments(_ptr(a), _ptr(_chk(b, 'b') if b is not None else None), B, a.numel() // B, _ptr(s1), _ptr(s2),
                                  wsp, wsn, _stream()), 't2i_row_moments')
    return s1, s2


def row_fma2(a, alpha, b=None, gamma=None, delta=None):
    """out[r,...] = a[r,...]*alpha[r] + b[r,...]*gamma[r] + delta[r]   (per-sample scalars; b/gamma and delta optional)."""
    _chk(a, 'a')
    B = a.shape[0]
    out = torch.empty_like(a)
    if _live(a):
        al = _chk(alpha.reshape(-1), 'alpha')
        ga = _chk(gamma.reshape(-1), 'gamma') if gamma is not None else None
        de = _chk(delta.reshape(-1), 'delta') if delta is not None else None
        assert al.numel() == B and (ga is None or ga.numel() == B) and (de is None or de.numel() == B)
        check(lib.t2i_row_fma2(_ptr(a), _ptr(_chk(b, 'b') if b is not None else None), _ptr(al), _ptr(ga), _ptr(de), B,
                               a.numel() // B, _ptr(out), _stream()), 't2i_row_fma2')
    return out


# ---- loss heads (reference models/wgancls/model.py:72-92,117-127) -------------------------------------------------------
D_HEAD_KEYS = ('D_loss', 'D_loss_real', 'D_loss_fake', 'D_loss_mismatch', 'wdist', 'wdist2', 'real_gp', 'real_gp2', 'reg_loss',
               'balance_loss', 'kt_grad', 'kt')


def wgan_d_head(logits, slopes1, slopes2, kt, gp_coeff, seed_l_into=None):
    """logits [3B] (fake | real | mismatch), slopes [B], kt: device scalar tensor or None (= 1).
    -> (scalars [12] in D_HEAD_KEYS order, dD/dlogits [3B], dD/dslopes1 [B], dD/dslopes2 [B]).  dD/dlogits depends on kt and B only
    (1/B | -(1+kt)/B | kt/B): the stacked critic step calls the head once BEFORE the slopes exist, for these seeds alone
    (seed_l_into: a contiguous float32 [3B] buffer that receives them), and once after, for the scalars and the slope seeds."""
    _chk(logits, 'logits'); _chk(slopes1, 'slopes1'); _chk(slopes2, 'slopes2')
    B = slopes1.numel()
    assert logits.numel() == 3 * B and slopes2.numel() == B
    scal = torch.empty(12, dtype=torch.float32, device=logits.device)
    if seed_l_into is not None:
        _chk(seed_l_into, 'seed_l_into', f32=True)
        assert seed_l_into.numel() == 3 * B
    sl = seed_l_into if seed_l_into is not None else torch.empty_like(logits)
    s1, s2 = torch.empty_like(slopes1), torch.empty_like(slopes2)
    if _live(logits):
        check(lib.t2i_wgan_d_head(_ptr(logits), _ptr(slopes1), _ptr(slopes2), _ptr(kt), B, gp_coeff, _ptr(sl), _ptr(s1), _ptr(s2),
                                  _ptr(scal), _stream()), 't2i_wgan_d_head')
    return scal, sl, s1, s2


def sigmoid_ce_head(logits, labels, weights, want_prob=True, seeds_into=None):
    """logits: 1-3 tensors of B logits each; labels / weights: one float per head.  -> (losses [4]: total, per head; seeds: list of
    d total / d logits_k; probs: list of sigmoid(logits_k) or None)  — t2i_sigmoid_ce_head, one launch.
    seeds_into: a flat float32 tensor of n*B elements whose slices receive the seeds (the heads of ONE batched pass)."""
    n = len(logits)
    assert 1 <= n <= 3 and len(labels) == n and len(weights) == n
    for t in logits:
        _chk(t, 'logits', f32=True)
    B = logits[0].numel()
    assert all(t.numel() == B and t.is_contiguous() for t in logits)
    losses = torch.empty(4, dtype=torch.float32, device=logits[0].device)
    if seeds_into is not None:
        _chk(seeds_into, 'seeds_into', f32=True)
        assert seeds_into.numel() == n * B
        flat = seeds_into.view(-1)
        seeds = [flat[k * B:(k + 1) * B] for k in range(n)]
    else:
        seeds = [torch.empty_like(t) for t in logits]
    probs = [torch.empty_like(t) for t in logits] if want_prob else None
    if _live(logits[0]):
        pad = lambda xs, fill: list(xs) + [fill] * (3 - n)
        lp = pad([_ptr(t) for t in logits], None)
        sp = pad([_ptr(t) for t in seeds], None)
        pp = pad([_ptr(t) for t in probs], None) if want_prob else [None] * 3
        y, w = pad([float(v) for v in labels], 0.0), pad([float(v) for v in weights], 0.0)
        check(lib.t2i_sigmoid_ce_head(lp[0], lp[1], lp[2], y[0], y[1], y[2], w[0], w[1], w[2], B, sp[0], sp[1], sp[2], pp[0], pp[1], pp[2],
                                      _ptr(losses), _stream()), 't2i_sigmoid_ce_head')
    return losses, seeds, probs


def ca_kl_fwd(mean, log_sigma, eps):
    _chk(mean, 'mean', f32=True); _chk(log_sigma, 'log_sigma', f32=True); _chk(eps, 'eps', f32=True)      # [B, 128]: kernels.f32_outputs()
    code = torch.empty_like(mean)
    kl = torch.empty(1, dtype=torch.float32, device=mean.device)
    if _live(mean):
        check(lib.t2i_ca_kl_fwd(_ptr(mean), _ptr(log_sigma), _ptr(eps), mean.numel(), _ptr(code), _ptr(kl), _stream()), 't2i_ca_kl_fwd')
    return code, kl


def ca_kl_bwd(mean, log_sigma, eps, dcode, dkl):
    dmean, dls = torch.empty_like(mean), torch.empty_like(mean)
    if _live(mean):
        check(lib.t2i_ca_kl_bwd(_ptr(mean), _ptr(log_sigma), _ptr(eps), _ptr(_chk(dcode, 'dcode') if dcode is not None else None),
                                _ptr(_chk(dkl, 'dkl') if dkl is not None else None), mean.numel(), _ptr(dmean), _ptr(dls),
                                _stream()), 't2i_ca_kl_bwd')
    return dmean, dls


ALGO_NAMES = tuple(k[len('T2I_ALGO_'):].lower() for k in sorted((k for k in CONSTANTS if k.startswith('T2I_ALGO_')), key=CONSTANTS.get))
ALGO_MAC_RATIO = (1.0, 1.0 / 2.25, 9.0 / 16.0, 1.0, 1.0)       # executed / direct-convolution multiply-adds


def conv_algo(d, which):
    """Algorithm the library picks for descriptor `d`; which: 'fwd' | 'bwd_data' | 'bwd_filter'."""
    a = int(lib.t2i_conv2d_algo(ctypes.byref(d), ('fwd', 'bwd_data', 'bwd_filter').index(which)))
    if a < 0:
        raise ValueError('invalid conv descriptor')
    return ALGO_NAMES[a]


_FC_ARENA = [None]
_FC_ON = [False]


def filter_cache(on, device=None):
    """Opt into the transformed-filter cache of the Winograd conv paths (include/t2i_hip.h: contract).  The library owns no
    device memory: the first call allocates the arena the transforms live in (T2I_FILTER_CACHE_MB, default 1024; the
    wgancls step needs 650 MB) and attaches it.  Everything in this package that writes filter memory outside t2i_adam_tf
    calls filter_cache_invalidate(): ParamStore.load, Saver.restore, optim.Arena creation, dp.broadcast_variables, hipGraph
    replays.  Returns the previous state."""
    if on and _FC_ARENA[0] is None and torch.cuda.is_available():
        import os
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        buf = torch.empty(int(os.environ.get('T2I_FILTER_CACHE_MB', '1024')) << 20, dtype=torch.uint8, device=dev)
        check(lib.t2i_filter_cache_attach(_ptr(buf), buf.numel()), 't2i_filter_cache_attach')
        _FC_ARENA[0] = buf           # kept for the life of the process: captured graphs point into it
    _FC_ON[0] = bool(on) and _FC_ARENA[0] is not None
    return bool(lib.t2i_filter_cache_enable(1 if on else 0))


def filter_cache_enabled():
    """True while the transformed-filter cache is on through filter_cache() (and has its arena)."""
    return _FC_ON[0]


def filter_cache_reset():
    """Drop every cached filter image and hand the library the same arena again, empty.  Legal only when no captured graph that
    used the cache is alive any more (bench.py calls it between two configurations, after the first model and its graphs are gone):
    slots are never moved or reused while attached, so a process that builds model after model would otherwise fill the arena with
    images of filters that no longer exist."""
    if _FC_ARENA[0] is not None:
        buf = _FC_ARENA[0]
        check(lib.t2i_filter_cache_attach(None, 0), 't2i_filter_cache_attach')
        check(lib.t2i_filter_cache_attach(_ptr(buf), buf.numel()), 't2i_filter_cache_attach')


def tuning_set(key, value):
    """Planner / diagnostic switch (include/t2i_hip.h t2i_tuning_set); drops cached descriptors, whose workspace sizes
    were computed under the old setting."""
    check(lib.t2i_tuning_set(key.encode(), float(value)), 't2i_tuning_set')
    _DESC_CACHE.clear()
    _H_ALGO.clear()
    _XFORM_BYTES.clear()


def zero_ranges(base, table):
    """base[start:start + length] = 0 for every (start, length) row of the device int64 table [n, 2], one launch (t2i_zero_ranges)."""
    _chk(base, 'base', f32=True)
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 2 and table.is_contiguous() and table.device == base.device
    if _live(base) and table.shape[0]:
        check(lib.t2i_zero_ranges(_ptr(base), _ptr(table), int(table.shape[0]), _stream()), 't2i_zero_ranges')


def trunc_normal_(t, mean=0.0, std=1.0, a=-2.0, b=2.0):
    """In place: t = mean + std * n with n ~ N(0,1) truncated to [a, b] (a, b in units of the standard normal: the reference's
    tf.truncated_normal cuts at +-2 standard deviations; with mean 0, std 1 these are torch.nn.init.trunc_normal_'s arguments).
    One launch (t2i_trunc_normal) instead of the tensor library's eight.  The Philox (seed, offset) come from — and advance — the
    device's torch generator, so torch.manual_seed / torch.cuda.manual_seed make the draws reproducible like any other."""
    _chk(t, 't', f32=True)
    if _live(t):
        gen = torch.cuda.default_generators[t.device.index if t.device.index is not None else torch.cuda.current_device()]
        seed, off = int(gen.initial_seed()) & 0xFFFFFFFFFFFFFFFF, int(gen.get_offset())
        quads = (t.numel() + 3) // 4
        gen.set_offset(off + 4 * ((quads + 3) // 4))              # (torch wants multiples of 4)
        check(lib.t2i_trunc_normal(_ptr(t), t.numel(), seed, off, float(mean), float(std), float(a), float(b), _stream()), 't2i_trunc_normal')
    return t


def kt_sgd(kt, wdist_sums, scale, lr):
    """kt -= lr * d balance_loss / d kt from the (rank-summed) batch means wdist, wdist2; in place on the device scalar."""
    _chk(wdist_sums, 'wdist_sums')
    assert wdist_sums.numel() == 2 and kt.numel() == 1
    if _live(wdist_sums):
        check(lib.t2i_kt_sgd(_ptr(kt), _ptr(wdist_sums), scale, lr, _stream()), 't2i_kt_sgd')


_FILTER_EPOCH = [0]


def filter_epoch():
    """Counts the filter writes announced from OUTSIDE a training step (checkpoint loads, broadcasts, new arenas ...): a captured
    iteration that trusts the images its previous replay left (filter_cache_assume) regenerates them eagerly when this moved."""
    return _FILTER_EPOCH[0]


def filter_cache_invalidate(t=None, external=True):
    """Drop cached transforms of the filters inside tensor `t` (None: all).  external=False: the caller is a training step's own
    replay, which left the images of the arenas it regenerates behind its updates valid in memory (only the host's bookkeeping is
    stale); every other writer of filter memory leaves the default, which also moves filter_epoch()."""
    if external:
        _FILTER_EPOCH[0] += 1
    if t is None:
        lib.t2i_filter_cache_invalidate(None, 0)
    elif t.is_cuda:
        lib.t2i_filter_cache_invalidate(_ptr(t), t.numel() * t.element_size())


def filter_cache_bytes():
    return int(lib.t2i_filter_cache_bytes())


def filter_cache_refresh(t=None):
    """Regenerate, in one launch, every cached filter image (of the filters inside tensor `t`; None = all, legal only while every
    filter the cache has seen is still allocated) that is stale in the current launch context.  t2i_adam_tf does this for its arena; graphs.StepGraphs.capture does it at the head of every graph,
    so that a graph holds ONE batched refresh instead of one small fill per filter at its first use."""
    if t is None:
        check(lib.t2i_filter_cache_refresh(None, 0, _stream()), 't2i_filter_cache_refresh')
    else:
        check(lib.t2i_filter_cache_refresh(_ptr(t), t.numel() * t.element_size(), _stream()), 't2i_filter_cache_refresh')


def filter_cache_assume(t):
    """Mark the cached images of the filters inside tensor `t` as filled for the current launch context without regenerating them
    (include/t2i_hip.h t2i_filter_cache_assume: the caller vouches that they will be current whenever the following work runs)."""
    check(lib.t2i_filter_cache_assume(_ptr(t), t.numel() * t.element_size(), _stream()), 't2i_filter_cache_assume')


def lerp_dev(a, b, t_dev, mode=0):
    """mode 0: (1-t)*a + t*b;  1: t*a;  2: (1-t)*a   with t a 1-element device tensor."""
    _chk(a, 'a')
    out = torch.empty_like(a)
    if _live(a):
        check(lib.t2i_lerp_dev(_ptr(a), _ptr(_chk(b, 'b') if b is not None else None), _ptr(_chk(t_dev, 't')), mode, a.numel(), _ptr(out),
                               _stream()), 't2i_lerp_dev')
    return out


# ---- InceptionV3 fine-tuning (t2i_incep_train.hip) ------------------------------------------------------------------------
def pool_dropout(x, keep, seed, step):
    """AvgPool_1a_8x8 + Dropout_1b: x [B, H, W, D] float32 -> (pre [B, D], mask [B, D] of 0 / 1, y = pre / keep * mask); the mask is a
    pure function of (seed, step, b, d)."""
    _chk(x, 'x', f32=True)
    B, D = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * D)
    pre, mask, y = (torch.empty((B, D), dtype=torch.float32, device=x.device) for _ in range(3))
    if _live(x):
        check(lib.t2i_pool_dropout(_ptr(x), B, HW, D, float(keep), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                   _ptr(pre), _ptr(mask), _ptr(y), _stream()), 't2i_pool_dropout')
    return pre, mask, y


def softmax_ce_head(y, W, bias, labels, dW_out=None, db_out=None, accumulate=False):
    """Logits head + mean sparse softmax cross-entropy, forward and backward (two launches).  y [B, D], W [D, C] (or the
    [1, 1, D, C] conv filter), bias [C], labels int32 [B] -> dict(logits, prob, loss [1], acc [1], dW, db, dy [B, D]).  dW_out /
    db_out: gradient-arena slots to write (accumulate: add) into."""
    _chk(y, 'y', f32=True); _chk(W, 'W', f32=True); _chk(bias, 'bias', f32=True)
    B, D = y.shape
    C = bias.numel()
    if W.numel() != D * C or labels.dtype != torch.int32 or labels.numel() != B:
        raise ValueError('softmax_ce_head: y %s, W %s, bias %s, labels %s %s' % (tuple(y.shape), tuple(W.shape), tuple(bias.shape),
                                                                                  labels.dtype, tuple(labels.shape)))
    labels = labels.contiguous()
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=y.device)       # noqa: E731
    out = dict(logits=f(B, C), prob=f(B, C), loss=f(1), acc=f(1), dy=f(B, D))
    out['dW'] = dW_out if dW_out is not None else f(D, C)
    out['db'] = db_out if db_out is not None else f(C)
    assert out['dW'].numel() == D * C and out['db'].numel() == C
    _drop_image(out['dW'])
    if _live(y):
        wsp, wsn = _ws_args(y, int(lib.t2i_softmax_ce_head_workspace_bytes(B, C)))
        check(lib.t2i_softmax_ce_head(_ptr(y), _ptr(W), _ptr(bias), _ptr(labels), B, D, C, _ptr(out['logits']), _ptr(out['prob']),
                                      _ptr(out['loss']), _ptr(out['acc']), _ptr(out['dW']), _ptr(out['db']), 1 if accumulate else 0,
                                      _ptr(out['dy']), wsp, wsn, _stream()), 't2i_softmax_ce_head')
    return out


def pooled_grad_scatter(g, mask, keep, outs, c0s, HW):
    """Backward of pool_dropout into the branches of a concatenation: outs[i] [B, H, W, C_i] (contiguous float32) =
    g[:, c0s[i]:c0s[i] + C_i] * mask / keep / HW at every pixel.  One launch."""
    _chk(g, 'g', f32=True); _chk(mask, 'mask', f32=True)
    B, D = g.shape
    n = len(outs)
    if n != len(c0s) or not 0 < n <= MAX_SCATTER_BRANCHES:
        raise ValueError('pooled_grad_scatter: %d outputs, %d offsets' % (n, len(c0s)))
    for o in outs:
        _chk(o, 'out', f32=True)
        if o.shape[0] != B or o.numel() != B * HW * o.shape[-1]:
            raise ValueError('pooled_grad_scatter: output %s for B=%d HW=%d' % (tuple(o.shape), B, HW))
    if _live(g):
        ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        c0 = (ctypes.c_int32 * n)(*[int(c) for c in c0s])
        cb = (ctypes.c_int32 * n)(*[int(o.shape[-1]) for o in outs])
        check(lib.t2i_pooled_grad_scatter(_ptr(g), _ptr(mask), B, int(HW), D, float(keep), n, ptrs, c0, cb, _stream()),
              't2i_pooled_grad_scatter')
    return outs


MAX_SCATTER_BRANCHES = CONSTANTS['T2I_MAX_SCATTER_BRANCHES']


def rmsprop_tf(w, g, ms, mom, lr, rho=0.9, momentum=0.0, eps=1e-10):
    """tf.train.RMSPropOptimizer's update in place on flat arenas, one launch."""
    for t in (w, g, ms, mom):
        _chk(t, f32=True)
    assert w.numel() == g.numel() == ms.numel() == mom.numel()
    if _live(w):
        check(lib.t2i_rmsprop_tf(_ptr(w), _ptr(g), _ptr(ms), _ptr(mom), w.numel(), float(lr), float(rho), float(momentum), float(eps),
                                 _stream()), 't2i_rmsprop_tf')


# ---- the rest of the operator surface (reference utils/ops.py:94-116,145-148; csrc/t2i_ops.hip) --------------------------


def pixel_norm_fwd(x, eps, act=ACT_NONE, alpha=0.2):
    """x [..., C] -> (y = u / sqrt(mean_c(u^2) + eps) with u = act(x), rnorm [rows] = 1 / sqrt(mean_c(u^2) + eps)); one launch."""
    _chk(x, 'x', f32=True)
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    rnorm = torch.empty(rows, dtype=torch.float32, device=x.device)
    if _live(x) and rows > 0:
        check(lib.t2i_pixel_norm_fwd(_ptr(x), rows, C, float(eps), act, alpha, _ptr(y), _ptr(rnorm), _stream()), 't2i_pixel_norm_fwd')
    return y, rnorm


def pixel_norm_bwd(g, y, rnorm, act=ACT_NONE, alpha=0.2):
    """-> dx of pixel_norm_fwd from the upstream gradient g, the output y and rnorm; one launch."""
    _chk(g, 'g', f32=True); _chk(y, 'y', f32=True); _chk(rnorm, 'rnorm', f32=True)
    assert g.shape == y.shape
    C = y.shape[-1]
    rows = y.numel() // C
    dx = torch.empty_like(y)
    if _live(y) and rows > 0:
        check(lib.t2i_pixel_norm_bwd(_ptr(g), _ptr(y), _ptr(rnorm), rows, C, act, alpha, _ptr(dx), _stream()), 't2i_pixel_norm_bwd')
    return dx


def pixel_norm_bwd2(v, g, y, rnorm, act=ACT_NONE, alpha=0.2):
    """The double backward of pixel_norm: -> (dL/dg, dL/dx) of L = <v, pixel_norm_bwd(g, y, rnorm)>; one launch."""
    for t, name in ((v, 'v'), (g, 'g'), (y, 'y'), (rnorm, 'rnorm')):
        _chk(t, name, f32=True)
    assert v.shape == y.shape and g.shape == y.shape
    C = y.shape[-1]
    rows = y.numel() // C
    dg, dx = torch.empty_like(y), torch.empty_like(y)
    if _live(y) and rows > 0:
        check(lib.t2i_pixel_norm_bwd2(_ptr(v), _ptr(g), _ptr(y), _ptr(rnorm), rows, C, act, alpha, _ptr(dg), _ptr(dx), _stream()),
              't2i_pixel_norm_bwd2')
    return dg, dx


def _ln2_args(v, gy, xhat, y, gamma):
    for t, name in ((v, 'v'), (gy, 'gy'), (xhat, 'xhat'), (gamma, 'gamma')):
        _chk(t, name, f32=True)
    if y is not None:
        _chk(y, 'y', f32=True)
    assert v.shape == xhat.shape and gy.shape == xhat.shape and (y is None or y.shape == xhat.shape)
    B, C = xhat.shape[0], xhat.shape[-1]
    assert gamma.numel() == C
    return B, xhat.numel() // B, C


def layer_norm_bwd2_sums(v, gy, xhat, y, gamma, act=ACT_NONE, alpha=0.2):
    """-> [B, 5] per-sample (sum v, sum v xhat, sum g, sum g xhat, sum v g), g = gamma_c gy act'(.): partials over up to 256 workgroups
    per sample, then their fixed-order sum (two launches)."""
    B, per, C = _ln2_args(v, gy, xhat, y, gamma)
    sums = torch.empty((B, 5), dtype=torch.float32, device=xhat.device)
    if _live(xhat) and xhat.numel() > 0:
        wsp, wsn = _ws_args(xhat, int(lib.t2i_layer_norm_bwd2_workspace_bytes(B)))
        check(lib.t2i_layer_norm_bwd2_sums(_ptr(v), _ptr(gy), _ptr(xhat), _ptr(y), _ptr(gamma), B, per, C, act, alpha, _ptr(sums), wsp, wsn,
                                           _stream()), 't2i_layer_norm_bwd2_sums')
    return sums


def layer_norm_bwd2_apply(v, gy, xhat, y, gamma, rstd, sums, act=ACT_NONE, alpha=0.2, want_hgz=False):
    """-> (dL/dgy, dL/dx, hgz or None) from the sums of layer_norm_bwd2_sums; one elementwise launch."""
    B, per, C = _ln2_args(v, gy, xhat, y, gamma)
    _chk(rstd, 'rstd', f32=True); _chk(sums, 'sums', f32=True)
    assert rstd.numel() == B and sums.numel() == 5 * B
    dgy, dx = torch.empty_like(xhat), torch.empty_like(xhat)
    hgz = torch.empty_like(xhat) if want_hgz else None
    if _live(xhat) and xhat.numel() > 0:
        check(lib.t2i_layer_norm_bwd2_apply(_ptr(v), _ptr(gy), _ptr(xhat), _ptr(y), _ptr(gamma), _ptr(rstd), _ptr(sums), B, per, C, act, alpha,
                                            _ptr(dgy), _ptr(dx), _ptr(hgz), _stream()), 't2i_layer_norm_bwd2_apply')
    return dgy, dx, hgz


def layer_norm_bwd2(v, gy, xhat, y, gamma, rstd, act=ACT_NONE, alpha=0.2, want_hgz=False):
    """The double backward of layer_norm ([B, ..., C], normalised per sample, gamma [C]; y = the activation's output or None):
    -> (dL/dgy, dL/dx, hgz or None) of L = <v, dx_first_order>; colsum(hgz) is dL/dgamma (col_reduce)."""
    sums = layer_norm_bwd2_sums(v, gy, xhat, y, gamma, act, alpha)
    return layer_norm_bwd2_apply(v, gy, xhat, y, gamma, rstd, sums, act, alpha, want_hgz)


def _mbstd_args(x, G, F):
    _chk(x, 'x', f32=True)
    assert x.dim() == 4
    B, H, W, C = x.shape
    if not (1 <= G <= 16 and B % G == 0 and F >= 1 and C % F == 0):
        raise ValueError('minibatch_stddev: group size %d (1..16) must divide the batch %d and %d statistic channels the %d channels' % (G, B, F, C))
    return B, H, W, C


def minibatch_stddev_fwd(x, G, F, eps=1e-8):
    """x [B,H,W,C] -> stat [B,F]: the mean over chunk f's columns of the standard deviation across the G contiguous samples of a
    group, the same in every row of the group (two launches: partials into the workspace, then their fixed-order sum)."""
    B, H, W, C = _mbstd_args(x, G, F)
    stat = torch.empty((B, F), dtype=torch.float32, device=x.device)
    if _live(x) and x.numel() > 0:
        wsp, wsn = _ws_args(x, int(lib.t2i_minibatch_stddev_workspace_bytes(B, H, W, C, G, F)))
        check(lib.t2i_minibatch_stddev_fwd(_ptr(x), B, H, W, C, G, F, eps, _ptr(stat), wsp, wsn, _stream()), 't2i_minibatch_stddev_fwd')
    return stat


def minibatch_stddev_bwd(gs, x, G, F, eps=1e-8):
    """dx of minibatch_stddev_fwd for the cotangent gs [B,F]; mu and sigma are recomputed from x.  One launch."""
    B, H, W, C = _mbstd_args(x, G, F)
    _chk(gs, 'gs', f32=True)
    assert tuple(gs.shape) == (B, F)
    dx = torch.empty_like(x)
    if _live(x) and x.numel() > 0:
        check(lib.t2i_minibatch_stddev_bwd(_ptr(gs), _ptr(x), B, H, W, C, G, F, eps, _ptr(dx), _stream()), 't2i_minibatch_stddev_bwd')
    return dx


def minibatch_stddev_bwd2(v, x, gs, G, F, eps=1e-8):
    """The double backward: -> (dL/dx, dL/dgs [B,F]) of L = <v, minibatch_stddev_bwd(gs, x)>; two launches."""
    B, H, W, C = _mbstd_args(x, G, F)
    _chk(v, 'v', f32=True); _chk(gs, 'gs', f32=True)
    assert v.shape == x.shape and tuple(gs.shape) == (B, F)
    dxx = torch.empty_like(x)
    dgs = torch.empty((B, F), dtype=torch.float32, device=x.device)
    if _live(x) and x.numel() > 0:
        wsp, wsn = _ws_args(x, int(lib.t2i_minibatch_stddev_workspace_bytes(B, H, W, C, G, F)))
        check(lib.t2i_minibatch_stddev_bwd2(_ptr(v), _ptr(x), _ptr(gs), B, H, W, C, G, F, eps, _ptr(dxx), _ptr(dgs), wsp, wsn, _stream()),
              't2i_minibatch_stddev_bwd2')
    return dxx, dgs


DIFFAUG_COLOR, DIFFAUG_TRANSLATION, DIFFAUG_CUTOUT = header_values('DIFFAUG_COLOR', 'DIFFAUG_TRANSLATION', 'DIFFAUG_CUTOUT')  # the policy mask of diff_augment_fwd / _adj


def _diffaug_args(x, P, policy):
    _chk(x, 'x', f32=True); _chk(P, 'params', f32=True)
    if x.dim() != 4 or tuple(P.shape) != (x.shape[0], 9) or P.device != x.device:
        raise ValueError('diff_augment: x must be [B,H,W,C] and params [B,9] on the same device, got %s on %s and %s on %s' % (
            tuple(x.shape), x.device, tuple(P.shape), P.device))
    policy = int(policy)
    if policy <= 0 or policy & ~(DIFFAUG_COLOR | DIFFAUG_TRANSLATION | DIFFAUG_CUTOUT):
        raise ValueError('diff_augment: policy must be a non-empty mask of DIFFAUG_COLOR | DIFFAUG_TRANSLATION | DIFFAUG_CUTOUT, got %d' % policy)
    return tuple(x.shape) + (policy,)


def diff_augment_fwd(x, P, policy, offset=True):
    """y = T(x) for x [B,H,W,C] and the table P [B,9] = (b, s, c, ty, tx, y0, y1, x0, x1) per sample (include/t2i_hip.h): colour,
    integer translation with zero padding, rectangular cutout, as the bits of `policy` select.  offset=False leaves the brightness
    offset b out: the linear part A of T, which is the backward of diff_augment_adj.  Two launches with DIFFAUG_COLOR (per-sample
    partial sums, then the apply kernel), else one."""
    B, H, W, C, policy = _diffaug_args(x, P, policy)
    y = torch.empty_like(x)
    if _live(x) and x.numel() > 0:
        wsp, wsn = _ws_args(x, int(lib.t2i_diff_augment_workspace_bytes(B, H, W, C, policy)))
        check(lib.t2i_diff_augment_fwd(_ptr(x), _ptr(P), B, H, W, C, policy, 1 if offset else 0, _ptr(y), wsp, wsn, _stream()),
              't2i_diff_augment_fwd')
    return y


def diff_augment_adj(g, P, policy):
    """dx = A^T g, the adjoint of the linear part of diff_augment_fwd: the cutout mask, the opposite shift, then the two (self-adjoint)
    colour blends in reverse order.  Two launches with DIFFAUG_COLOR, else one."""
    B, H, W, C, policy = _diffaug_args(g, P, policy)
    dx = torch.empty_like(g)
    if _live(g) and g.numel() > 0:
        wsp, wsn = _ws_args(g, int(lib.t2i_diff_augment_workspace_bytes(B, H, W, C, policy)))
        check(lib.t2i_diff_augment_adj(_ptr(g), _ptr(P), B, H, W, C, policy, _ptr(dx), wsp, wsn, _stream()), 't2i_diff_augment_adj')
    return dx


ADA_LOGIT, ADA_MIDPOINT = header_values('ADA_LOGIT', 'ADA_MIDPOINT')      # the threshold of diffaug_observe's statistic


def _diffaug_state(state, op):
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or tuple(state.shape) != (16,) or not state.is_contiguous():
        raise ValueError('%s: state must be a contiguous int32 tensor of 16 words (t2i_diffaug_state), got %s' % (
            op, '%s %s' % (state.dtype, tuple(state.shape)) if isinstance(state, torch.Tensor) else type(state).__name__))
    return state


def diff_augment_draw(state, out, H, W, policy):
    """Fills `out` [n, 9] with call k's parameter table of diff_augment_fwd for H x W images and advances the call counter of `state`
    (16 int32 words on out's device: include/t2i_hip.h, t2i_diffaug_state) to k + 1.  Philox4x32-10 keyed by the state's seed; each
    transform of `policy` is applied to a row with the state's probability p, else the row has its identity columns.  One launch, no
    host work: capturable, and every replay draws the next table."""
    op = 'diff_augment_draw'
    _diffaug_state(state, op)
    _chk(out, 'out', f32=True)
    if out.dim() != 2 or out.shape[1] != 9 or out.device != state.device:
        raise ValueError('%s: out must be [n, 9] on the state\'s device, got %s on %s (state on %s)' % (op, tuple(out.shape), out.device, state.device))
    policy = int(policy)
    if policy <= 0 or policy & ~(DIFFAUG_COLOR | DIFFAUG_TRANSLATION | DIFFAUG_CUTOUT):
        raise ValueError('%s: policy must be a non-empty mask of DIFFAUG_COLOR | DIFFAUG_TRANSLATION | DIFFAUG_CUTOUT, got %d' % (op, policy))
    if _live(out):
        check(lib.t2i_diff_augment_draw(_ptr(state), out.shape[0], int(H), int(W), policy, _ptr(out), _stream()), 't2i_diff_augment_draw')
    return out


def diffaug_observe(state, d_real, d_fake, mode, target, interval, ramp_images):
    """One observation of the controller of p (include/t2i_hip.h, t2i_diffaug_observe): the signs of d_real [n] against 0 (ADA_LOGIT;
    d_fake may be None) or against the midpoint of the batch means of d_real and d_fake [n] (ADA_MIDPOINT) are added to the state's
    accumulators, and on every `interval`-th call p moves by (logits seen) / ramp_images towards the statistic `target`.  One launch."""
    op = 'diffaug_observe'
    _diffaug_state(state, op)
    _chk(d_real, 'd_real', f32=True)
    if d_real.dim() != 1 or d_real.device != state.device:
        raise ValueError('%s: d_real must be a vector on the state\'s device, got %s on %s' % (op, tuple(d_real.shape), d_real.device))
    if d_fake is not None:
        _chk(d_fake, 'd_fake', f32=True)
        if d_fake.shape != d_real.shape or d_fake.device != state.device:
            raise ValueError('%s: d_fake must match d_real %s on %s, got %s on %s' % (op, tuple(d_real.shape), d_real.device,
                                                                                       tuple(d_fake.shape), d_fake.device))
    elif mode != ADA_LOGIT:
        raise ValueError('%s: d_fake may be None only under ADA_LOGIT' % op)
    if _live(d_real):
        check(lib.t2i_diffaug_observe(_ptr(state), _ptr(d_real), _ptr(d_fake), d_real.shape[0], int(mode), float(target), int(interval),
                                      float(ramp_images), _stream()), 't2i_diffaug_observe')


def resize_nearest(x, Ho, Wo):
    """x [B,H,W,C] -> [B,Ho,Wo,C], tf.image.resize_nearest_neighbor (align_corners=False)."""
    _chk(x, 'x', f32=True)
    B, H, W, C = x.shape
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    if _live(x) and y.numel() > 0:
        check(lib.t2i_resize_nearest(_ptr(x), B, H, W, C, Ho, Wo, _ptr(y), _stream()), 't2i_resize_nearest')
    return y


def resize_nearest_adj(g, H, W):
    """The adjoint of resize_nearest from [B,H,W,C]: g [B,Ho,Wo,C] -> [B,H,W,C], each input pixel the sum of its output block."""
    _chk(g, 'g', f32=True)
    B, Ho, Wo, C = g.shape
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device=g.device)
    if _live(g) and dx.numel() > 0:
        check(lib.t2i_resize_nearest_adj(_ptr(g), B, H, W, C, Ho, Wo, _ptr(dx), _stream()), 't2i_resize_nearest_adj')
    return dx


def pool_same_fwd(x, s, op, want_idx=False):
    """tf.nn.pool(window = stride = s, SAME) of x [B,H,W,C] -> (y [B,ceil(H/s),ceil(W/s),C], idx or None); idx (MAX only): int32
    window offset of the first maximum."""
    _chk(x, 'x', f32=True)
    B, H, W, C = x.shape
    y = torch.empty((B, -(-H // s), -(-W // s), C), dtype=torch.float32, device=x.device)
    idx = torch.empty(y.shape, dtype=torch.int32, device=x.device) if (want_idx and op == POOL_MAX) else None
    if _live(x) and y.numel() > 0:
        check(lib.t2i_pool_same_fwd(_ptr(x), B, H, W, C, s, op, _ptr(y), _ptr(idx), _stream()), 't2i_pool_same_fwd')
    return y, idx


def pool_same_bwd(g, idx, H, W, s, op):
    """g [B,Ho,Wo,C] -> dx [B,H,W,C]: AVG g / count of the pixel's window; MAX g where idx holds the pixel's offset, else 0."""
    _chk(g, 'g', f32=True)
    B, Ho, Wo, C = g.shape
    assert (Ho, Wo) == (-(-H // s), -(-W // s)) and (idx is None) == (op == POOL_AVG)
    if idx is not None:
        assert idx.dtype == torch.int32 and idx.shape == g.shape and idx.is_contiguous()
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device=g.device)
    if _live(g) and dx.numel() > 0:
        check(lib.t2i_pool_same_bwd(_ptr(g), _ptr(idx), B, H, W, C, s, op, _ptr(dx), _stream()), 't2i_pool_same_bwd')
    return dx


def pool_same_take(x, idx, s):
    """y[b,oh,ow,c] = x [B,H,W,C] at window offset idx[b,oh,ow,c]: MAX pooling with its offsets fixed (a linear map)."""
    _chk(x, 'x', f32=True)
    B, H, W, C = x.shape
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, -(-H // s), -(-W // s), C) and idx.is_contiguous()
    y = torch.empty(idx.shape, dtype=torch.float32, device=x.device)
    if _live(x) and y.numel() > 0:
        check(lib.t2i_pool_same_take(_ptr(x), _ptr(idx), B, H, W, C, s, _ptr(y), _stream()), 't2i_pool_same_take')
    return y


def gn_fwd(x, log_m, want_f=True):
    """-> (y = x * f, f = exp(n * log_m) or None) with n ~ N(0, 1) per element; one launch.  The Philox (seed, offset) come from — and
    advance — the device's torch generator, as in trunc_normal_ (another counter subsequence: the two never draw the same numbers).
    want_f=False skips writing the factor (no backward will ask for it); y is the same bits."""
    _chk(x, 'x', f32=True)
    y, f = torch.empty_like(x), (torch.empty_like(x) if want_f else None)
    if _live(x) and x.numel() > 0:
        gen = torch.cuda.default_generators[x.device.index if x.device.index is not None else torch.cuda.current_device()]
        seed, off = int(gen.initial_seed()) & 0xFFFFFFFFFFFFFFFF, int(gen.get_offset())
        quads = (x.numel() + 3) // 4
        gen.set_offset(off + 4 * ((quads + 3) // 4))              # (torch wants multiples of 4)
        check(lib.t2i_gn_fwd(_ptr(x), x.numel(), float(log_m), seed, off, _ptr(y), _ptr(f), _stream()), 't2i_gn_fwd')
    return y, f


def mul(a, b):
    """a * b elementwise (same shape), one launch."""
    _chk(a, 'a', f32=True); _chk(b, 'b', f32=True)
    assert a.shape == b.shape
    y = torch.empty_like(a)
    if _live(a) and a.numel() > 0:
        check(lib.t2i_mul(_ptr(a), _ptr(b), a.numel(), _ptr(y), _stream()), 't2i_mul')
    return y


# anti-aliased resampling (csrc/t2i_resample.hip)
UPFIRDN_TILE, UPFIRDN_MAX_TAPS = header_values('UPFIRDN_TILE', 'UPFIRDN_MAX_TAPS')      # outputs per tile and axis
UPFIRDN_MAX_PAD = 32768


def upfirdn2d_extent(H, u, d, p0, p1, n):
    """floor((H u + p0 + p1 - n) / d) + 1, the output extent of upfirdn2d along an axis of extent H; 0 for anything the entry refuses."""
    args = (H, u, d, p0, p1, n)
    if any(isinstance(a, bool) or int(a) != a or abs(int(a)) >= 1 << 31 for a in args):
        return 0
    return int(lib.t2i_upfirdn2d_extent(*(int(a) for a in args)))


def upfirdn2d_adjoint(H, Ho, n, u, d, p0, flip):
    """(u', d', p0', p1', flip') of the adjoint of an upfirdn2d that took extent H to Ho: the same operator, returning H exactly."""
    return d, u, n - 1 - p0, H * u - Ho * d + p0 - u + 1, not flip


def upfirdn2d(x, taps, u, d, p0, p1, flip, out=None):
    """x [B,H,W,C] -> y [B,Ho,Wo,C]: insert u - 1 zeros after every sample, pad by p0 in front and p1 behind (negative: crop), convolve
    with `taps` (n host floats, reversed first when flip) and keep every d-th sample, along H and W (include/t2i_hip.h,
    t2i_upfirdn2d).  p1 is an integer or a pair (along H, along W): the adjoint of a decimation needs one per axis when H and W leave
    different remainders.  One launch; `out` ([B,Ho,Wo,C] float32, not overlapping x) is written in place when given."""
    op = 'upfirdn2d'
    _chk(x, 'x', f32=True)
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError('%s: x must be [B,H,W,C] with every size at least 1, got %s' % (op, tuple(x.shape)))
    try:
        taps = [float(t) for t in taps]
    except (TypeError, ValueError):
        raise ValueError('%s: taps must be a sequence of numbers, got %r' % (op, taps))
    n = len(taps)
    if not 1 <= n <= UPFIRDN_MAX_TAPS:
        raise ValueError('%s: %d taps, the kernel takes 1..%d' % (op, n, UPFIRDN_MAX_TAPS))
    w = np.asarray(taps, dtype=np.float32)
    if not np.isfinite(w).all():
        raise ValueError('%s: the taps must be finite in float32, got %r' % (op, taps))
    p1h, p1w = (p1, p1) if not isinstance(p1, (tuple, list)) else p1
    for label, v in (('u', u), ('d', d), ('p0', p0), ('p1', p1h), ('p1', p1w)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('%s: %s must be an integer, got %r' % (op, label, v))
    if u not in (1, 2) or d not in (1, 2):
        raise ValueError('%s: the factors must be 1 or 2, got up %d and down %d' % (op, u, d))
    if max(abs(p0), abs(p1h), abs(p1w)) > UPFIRDN_MAX_PAD:
        raise ValueError('%s: pads (%d, %d / %d) exceed %d in magnitude' % (op, p0, p1h, p1w, UPFIRDN_MAX_PAD))
    B, H, W, C = x.shape
    Ho, Wo = upfirdn2d_extent(H, u, d, p0, p1h, n), upfirdn2d_extent(W, u, d, p0, p1w, n)
    if Ho < 1 or Wo < 1:
        raise ValueError('%s: a %dx%d map with up %d, down %d, pads (%d, %d / %d) and %d taps has no output' % (op, H, W, u, d, p0, p1h, p1w, n))
    if x.numel() >= 1 << 31 or B * Ho * Wo * C >= 1 << 31:
        raise ValueError('%s: x %s or y %s has 2^31 elements or more' % (op, tuple(x.shape), (B, Ho, Wo, C)))
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    else:
        _chk(out, 'out', f32=True)
        if tuple(out.shape) != (B, Ho, Wo, C) or out.device != x.device:
            raise ValueError('%s: out must be %s on %s, got %s on %s' % (op, (B, Ho, Wo, C), x.device, tuple(out.shape), out.device))
        x0, y0 = x.data_ptr(), out.data_ptr()
        if x0 < y0 + out.numel() * 4 and y0 < x0 + x.numel() * 4:
            raise ValueError('%s: out overlaps x' % op)
    if _live(x):
        check(lib.t2i_upfirdn2d_axes(_ptr(x), B, H, W, C, w.ctypes.data_as(ctypes.c_void_p), n, int(u), int(d), int(p0), int(p1h), int(p1w),
                                     1 if flip else 0, _ptr(out), _stream()), 't2i_upfirdn2d')
    return out


# ---- the style-based generator's layer epilogue: noise, activation, instance norm, style (csrc/t2i_style.hip) ----
ADAIN_CHUNK_ROWS = int(lib.t2i_adain_chunk_rows())      # rows of a sample per work item (include/t2i_hip.h T2I_ADAIN_CHUNK_ROWS)


def _style_rows(t, name, B, C):
    """ys / yb: float32 [B,C] with unit stride along C and rows any stride >= C apart (the halves of a dense layer's [B,2C] output)."""
    if t.dtype != torch.float32 or tuple(t.shape) != (B, C) or t.stride(1) != 1 or (B > 1 and t.stride(0) < C):
        raise ValueError('adain: %s must be a float32 [%d, %d] with unit stride along the channels, got %s %s strides %s' % (
            name, B, C, t.dtype, tuple(t.shape), t.stride()))
    return t.stride(0) if B > 1 else C


def _adain_args(x, noise, strength):
    _chk(x, 'x', f32=True)
    if x.dim() != 4 or min(x.shape) < 1 or x.numel() >= 1 << 31:
        raise ValueError('adain: x must be [B,H,W,C] with every size at least 1 and fewer than 2^31 elements, got %s' % (tuple(x.shape),))
    B, H, W, C = x.shape
    if (noise is None) != (strength is None):
        raise ValueError('adain: noise and strength come together or not at all')
    if noise is not None:
        _chk(noise, 'noise', f32=True); _chk(strength, 'strength', f32=True)
        if tuple(noise.shape) != (B, H, W) or tuple(strength.shape) != (C,):
            raise ValueError('adain: noise must be [%d, %d, %d] and strength [%d], got %s and %s' % (B, H, W, C, tuple(noise.shape), tuple(strength.shape)))
    return B, H * W, C


def adain_fwd(x, ys, yb, noise=None, strength=None, act=ACT_NONE, alpha=0.2, eps=1e-8):
    """x [B,H,W,C] -> (y, mean [B,C], rstd [B,C]) with u = act(x + strength[c] noise[b,h,w]) (u = act(x) without noise), the biased
    moments of u over (h, w) and y = (u - mean) rstd (1 + ys) + yb.  Three launches: chunk moments, their merge, apply."""
    B, R, C = _adain_args(x, noise, strength)
    sstride = _style_rows(ys, 'ys', B, C)
    if _style_rows(yb, 'yb', B, C) != sstride:
        raise ValueError('adain: ys and yb must have the same row stride, got %d and %d' % (ys.stride(0), yb.stride(0)))
    y = torch.empty_like(x)
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B, C), dtype=torch.float32, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, int(lib.t2i_adain_workspace_bytes(B, R, C)))
        check(lib.t2i_adain_stats(_ptr(x), _ptr(noise), _ptr(strength), B, R, C, act, alpha, float(eps), _ptr(mean), _ptr(rstd), wsp, wsn,
                                  _stream()), 't2i_adain_stats')
        check(lib.t2i_adain_apply(_ptr(x), _ptr(noise), _ptr(strength), _ptr(mean), _ptr(rstd), _ptr(ys), _ptr(yb), sstride, B, R, C, act, alpha,
                                  _ptr(y), _stream()), 't2i_adain_apply')
    return y, mean, rstd


def adain_bwd(g, x, ys, mean, rstd, noise=None, strength=None, act=ACT_NONE, alpha=0.2, want_strength=True):
    """The first-order backward of adain_fwd for the cotangent g of y -> (dx, dstrength [C] or None, dys [B,C], dyb [B,C]); u is
    recomputed from x.  Three launches, four with dstrength (only with noise, and only when wanted)."""
    B, R, C = _adain_args(x, noise, strength)
    _chk(g, 'g', f32=True); _chk(mean, 'mean', f32=True); _chk(rstd, 'rstd', f32=True)
    assert g.shape == x.shape and tuple(mean.shape) == (B, C) and tuple(rstd.shape) == (B, C)
    sstride = _style_rows(ys, 'ys', B, C)
    dx = torch.empty_like(x)
    dys = torch.empty((B, C), dtype=torch.float32, device=x.device)
    dyb = torch.empty((B, C), dtype=torch.float32, device=x.device)
    dstrength = torch.empty((C,), dtype=torch.float32, device=x.device) if (noise is not None and want_strength) else None
    if _live(x):
        wsp, wsn = _ws_args(x, int(lib.t2i_adain_workspace_bytes(B, R, C)))
        check(lib.t2i_adain_bwd_sums(_ptr(g), _ptr(x), _ptr(noise), _ptr(strength), _ptr(mean), _ptr(rstd), B, R, C, act, alpha, _ptr(dys),
                                     _ptr(dyb), wsp, wsn, _stream()), 't2i_adain_bwd_sums')
        check(lib.t2i_adain_bwd_apply(_ptr(g), _ptr(x), _ptr(noise), _ptr(strength), _ptr(mean), _ptr(rstd), _ptr(ys), sstride, _ptr(dys),
                                      _ptr(dyb), B, R, C, act, alpha, _ptr(dx), _ptr(dstrength), wsp, wsn, _stream()), 't2i_adain_bwd_apply')
    return dx, dstrength, dys, dyb


# ---- weight-demodulated convolutions: what surrounds the convolution (csrc/t2i_modconv.hip) -------------------------
MODCONV_CHUNK_ROWS = int(lib.t2i_modconv_chunk_rows())  # rows of a sample per work item (include/t2i_hip.h T2I_MODCONV_CHUNK_ROWS)


def _scale_rows(op, t, name, B, C):
    """s: float32 [B,C] with unit stride along C and rows any stride >= C apart (a slice of a wider dense output needs no copy)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (B, C) or t.stride(1) != 1 or (B > 1 and t.stride(0) < C):
        raise ValueError('%s: %s must be a float32 [%d, %d] with unit stride along the channels, got %s' % (
            op, name, B, C, '%s %s strides %s' % (t.dtype, tuple(t.shape), t.stride()) if isinstance(t, torch.Tensor) else type(t).__name__))
    return t.stride(0) if B > 1 else C


def _brc(op, x, name='x'):
    _chk(x, name, f32=True)
    if x.dim() != 4 or min(x.shape) < 1 or x.numel() >= 1 << 31:
        raise ValueError('%s: %s must be [B,H,W,C] with every size at least 1 and fewer than 2^31 elements, got %s' % (op, name, tuple(x.shape)))
    B, H, W, C = x.shape
    return B, H * W, C


def _filter_taps(op, w, s):
    _chk(w, 'w', f32=True)
    if w.dim() != 4 or min(w.shape) < 1 or w.numel() >= 1 << 31:
        raise ValueError('%s: w must be an HWIO filter [kh,kw,Cin,Cout] with every size at least 1, got %s' % (op, tuple(w.shape)))
    kh, kw, Cin, Cout = w.shape
    if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.shape[0] < 1:
        raise ValueError('%s: s must be [B, %d], got %s' % (op, Cin, tuple(s.shape) if isinstance(s, torch.Tensor) else type(s).__name__))
    B = s.shape[0]
    return kh * kw, Cin, Cout, B, _scale_rows(op, s, 's', B, Cin)


def demod_coef(w, s, eps=1e-8):
    """w [kh,kw,Cin,Cout], s [B,Cin] -> (d [B,Cout] = rsqrt(sum_i s^2 q + eps), q [Cin,Cout] = sum over the taps of w^2).  Two launches."""
    T, Cin, Cout, B, sstride = _filter_taps('demod_coef', w, s)
    q = torch.empty((Cin, Cout), dtype=torch.float32, device=w.device)
    d = torch.empty((B, Cout), dtype=torch.float32, device=w.device)
    if _live(w):
        check(lib.t2i_demod_coef(_ptr(w), _ptr(s), sstride, T, Cin, Cout, B, float(eps), _ptr(q), _ptr(d), _stream()), 't2i_demod_coef')
    return d, q


def demod_coef_bwd(gd, d, w, s, q, want_s=True, want_w=True, out=None, accumulate=False):
    """The backward of demod_coef for the cotangent gd of d -> (ds [B,Cin] or None, dw like w or None): a launch per wanted output.
    out: where dw goes (a flat float32 tensor of w's size: a gradient arena slot); with accumulate it is added to what out holds."""
    T, Cin, Cout, B, sstride = _filter_taps('demod_coef_bwd', w, s)
    _chk(gd, 'gd', f32=True); _chk(d, 'd', f32=True); _chk(q, 'q', f32=True)
    assert tuple(gd.shape) == (B, Cout) and tuple(d.shape) == (B, Cout) and tuple(q.shape) == (Cin, Cout)
    ds = torch.empty((B, Cin), dtype=torch.float32, device=w.device) if want_s else None
    dw = (torch.empty_like(w) if out is None else out) if want_w else None
    if dw is not None and (dw.dtype != torch.float32 or dw.numel() != w.numel() or not dw.is_contiguous()):
        raise ValueError('demod_coef_bwd: out must be a contiguous float32 tensor of %d elements' % w.numel())
    if _live(w) and (want_s or want_w):
        check(lib.t2i_demod_coef_bwd(_ptr(gd), _ptr(d), _ptr(s), sstride, _ptr(w), _ptr(q), T, Cin, Cout, B, _ptr(ds), _ptr(dw),
                                     1 if (accumulate and out is not None) else 0, _stream()), 't2i_demod_coef_bwd')
    return ds, dw


def modulate(x, s):
    """x [B,H,W,C] * s [B,C] (rows any stride >= C apart) per sample and channel.  One launch; with a cotangent in place of x, the adjoint."""
    B, R, C = _brc('modulate', x)
    sstride = _scale_rows('modulate', s, 's', B, C)
    xs = torch.empty_like(x)
    if _live(x):
        check(lib.t2i_modulate(_ptr(x), _ptr(s), sstride, B, R, C, _ptr(xs), _stream()), 't2i_modulate')
    return xs


def modulate_bwd_scale(g, x):
    """ds [B,C] = the sum over (h, w) of g * x.  Two launches: per-chunk partials, their fixed-order sum."""
    B, R, C = _brc('modulate_bwd_scale', x)
    _chk(g, 'g', f32=True)
    assert g.shape == x.shape
    ds = torch.empty((B, C), dtype=torch.float32, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, int(lib.t2i_modulate_bwd_scale_workspace_bytes(B, R, C)))
        check(lib.t2i_modulate_bwd_scale(_ptr(g), _ptr(x), B, R, C, _ptr(ds), wsp, wsn, _stream()), 't2i_modulate_bwd_scale')
    return ds


def _demod_act_args(op, c, d, bias, noise, strength):
    B, R, C = _brc(op, c, 'c')
    H, W = c.shape[1], c.shape[2]
    if (noise is None) != (strength is None):
        raise ValueError('%s: noise and strength come together or not at all' % op)
    for name, t, shape in (('d', d, (B, C)), ('bias', bias, (C,)), ('noise', noise, (B, H, W)), ('strength', strength, (C,))):
        if t is not None:
            _chk(t, name, f32=True)
            if tuple(t.shape) != shape:
                raise ValueError('%s: %s must be %s, got %s' % (op, name, list(shape), tuple(t.shape)))
    return B, R, C


def demod_act(c, d=None, bias=None, noise=None, strength=None, act=ACT_NONE, alpha=0.2):
    """act(d[b,o] c + bias[o] + strength[o] noise[b,h,w]) for c [B,H,W,C]; d, bias and the noise pair are each optional.  One launch."""
    B, R, C = _demod_act_args('demod_act', c, d, bias, noise, strength)
    out = torch.empty_like(c)
    if _live(c):
        check(lib.t2i_demod_act(_ptr(c), _ptr(d), _ptr(bias), _ptr(noise), _ptr(strength), B, R, C, act, alpha, _ptr(out), _stream()), 't2i_demod_act')
    return out


def demod_act_bwd(g, c, d=None, bias=None, noise=None, strength=None, act=ACT_NONE, alpha=0.2, want_d=True, want_bias=True, want_strength=True):
    """The backward of demod_act for the cotangent g -> (dc, dd [B,C] or None, dbias [C] or None, dstrength [C] or None); the pre-activation is
    recomputed.  One launch, two with any of the three sums."""
    B, R, C = _demod_act_args('demod_act_bwd', c, d, bias, noise, strength)
    _chk(g, 'g', f32=True)
    assert g.shape == c.shape
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=c.device)
    dc = torch.empty_like(c)
    dd = new(B, C) if (d is not None and want_d) else None
    dbias = new(C) if (bias is not None and want_bias) else None
    dstrength = new(C) if (noise is not None and want_strength) else None
    if _live(c):
        sums = dd is not None or dbias is not None or dstrength is not None
        wsp, wsn = _ws_args(c, int(lib.t2i_demod_act_bwd_workspace_bytes(B, R, C))) if sums else (None, 0)
        check(lib.t2i_demod_act_bwd(_ptr(g), _ptr(c), _ptr(d), _ptr(bias), _ptr(noise), _ptr(strength), B, R, C, act, alpha, _ptr(dc), _ptr(dd),
                                    _ptr(dbias), _ptr(dstrength), wsp, wsn, _stream()), 't2i_demod_act_bwd')
    return dc, dd, dbias, dstrength


# ---- ... and the backward of that backward -----------------------------------------------------------------------
def _dense_rows(op, t, name, B, C):
    _chk(t, name, f32=True)
    if tuple(t.shape) != (B, C):
        raise ValueError('%s: %s must be [%d, %d], got %s' % (op, name, B, C, tuple(t.shape)))


def modulate2(s, vx, x, vs):
    """The cotangent of g in the scale pass's backward (dx = g s, ds = sum over (h, w) of g x): s vx + x vs for the cotangents vx [B,H,W,C] of
    dx and vs [B,C] of ds, either of which may be None (vx comes with s, vs with x).  One launch."""
    ref = vx if vx is not None else x
    if ref is None or (vs is not None and x is None) or (vx is not None and s is None) or (vx is None and vs is None):
        raise ValueError('modulate2: vx (with s) or vs (with x) must be given')
    B, R, C = _brc('modulate2', ref, 'vx' if vx is not None else 'x')
    sstride = _scale_rows('modulate2', s, 's', B, C) if vx is not None else C
    if vs is not None:
        _dense_rows('modulate2', vs, 'vs', B, C)
        _chk(x, 'x', f32=True)
        assert x.shape == ref.shape
    gg = torch.empty_like(ref)
    if _live(ref):
        check(lib.t2i_modulate2(_ptr(s) if vx is not None else None, sstride, _ptr(vx), _ptr(x) if vs is not None else None, _ptr(vs), B, R, C,
                                _ptr(gg), _stream()), 't2i_modulate2')
    return gg


def demod_act_bwd2(g, c, d, bias, noise, strength, vc, vd, act=ACT_NONE, alpha=0.2, want_g=True, want_c=True, want_d=True):
    """The backward of demod_act_bwd for the cotangents vc [B,H,W,C] of dc and vd [B,C] of dd (either may be None) ->
    (gg = m (d vc + c vd), gc = m g vd or None, gd [B,C] = sum over (h, w) of m g vc or None), m = act'(the recomputed pre-activation).
    One launch, two with gd."""
    B, R, C = _demod_act_args('demod_act_bwd2', c, d, bias, noise, strength)
    _chk(g, 'g', f32=True)
    assert g.shape == c.shape
    if vc is None and vd is None:
        raise ValueError('demod_act_bwd2: vc or vd must be given')
    if vc is not None:
        _chk(vc, 'vc', f32=True)
        assert vc.shape == c.shape
    if vd is not None:
        if d is None:
            raise ValueError('demod_act_bwd2: vd without d')
        _dense_rows('demod_act_bwd2', vd, 'vd', B, C)
    gg = torch.empty_like(c) if want_g else None
    gc = torch.empty_like(c) if (want_c and vd is not None) else None
    gd = torch.empty((B, C), dtype=torch.float32, device=c.device) if (want_d and vc is not None and d is not None) else None
    if _live(c) and (gg is not None or gc is not None or gd is not None):
        wsp, wsn = _ws_args(c, int(lib.t2i_demod_act_bwd2_workspace_bytes(B, R, C))) if gd is not None else (None, 0)
        check(lib.t2i_demod_act_bwd2(_ptr(g), _ptr(c), _ptr(d), _ptr(bias), _ptr(noise), _ptr(strength), _ptr(vc), _ptr(vd), B, R, C, act, alpha,
                                     _ptr(gg), _ptr(gc), _ptr(gd), wsp, wsn, _stream()), 't2i_demod_act_bwd2')
    return gg, gc, gd


def demod_coef_bwd2(vs, gd, d, w, s, q, want_gd=True, want_d=True, want_w=True, out=None, accumulate=False):
    """The backward of demod_coef_bwd's ds for its cotangent vs [B,Cin] -> (-d^3 r to gd or None, -3 d^2 gd r to d or None, the term
    4 w sum_b vs s e to w or None), r = sum_i vs s q.  A launch for the first two, a launch for the third; out / accumulate as in demod_coef_bwd."""
    T, Cin, Cout, B, sstride = _filter_taps('demod_coef_bwd2', w, s)
    _chk(gd, 'gd', f32=True); _chk(d, 'd', f32=True); _chk(q, 'q', f32=True)
    _dense_rows('demod_coef_bwd2', vs, 'vs', B, Cin)
    assert tuple(gd.shape) == (B, Cout) and tuple(d.shape) == (B, Cout) and tuple(q.shape) == (Cin, Cout)
    gg_d = torch.empty_like(d) if want_gd else None
    gd_d = torch.empty_like(d) if want_d else None
    dw = (torch.empty_like(w) if out is None else out) if want_w else None
    if dw is not None and (dw.dtype != torch.float32 or dw.numel() != w.numel() or not dw.is_contiguous()):
        raise ValueError('demod_coef_bwd2: out must be a contiguous float32 tensor of %d elements' % w.numel())
    if _live(w) and (want_gd or want_d or want_w):
        check(lib.t2i_demod_coef_bwd2(_ptr(vs), _ptr(gd), _ptr(d), _ptr(s), sstride, _ptr(w), _ptr(q), T, Cin, Cout, B, _ptr(gg_d), _ptr(gd_d),
                                      _ptr(dw), 1 if (accumulate and out is not None) else 0, _stream()), 't2i_demod_coef_bwd2')
    return gg_d, gd_d, dw


# ---- sliced Wasserstein distance (csrc/t2i_swd.hip; evaluation/swd.py is the caller) -----------------------------------------
def _f32_nd(t, name, dim):
    if t.dtype != torch.float32 or t.dim() != dim or not t.is_contiguous():
        raise ValueError('%s must be a contiguous float32 tensor of %d dimensions, got %s %s' % (name, dim, t.dtype, tuple(t.shape)))
    return t


def pyramid_offsets(N, H, W, C, levels):
    """Element offsets of the levels in laplacian_pyramid's packed output, and its total element count."""
    offs, total = [], 0
    for i in range(levels):
        offs.append(total)
        total += N * (H >> i) * (W >> i) * C
    return offs, total


def laplacian_pyramid(x, levels):
    """x float32 [N,H,W,C] -> the list of `levels` Laplacian levels [N, H >> i, W >> i, C] (views of one packed buffer):
    t2i_laplacian_pyramid, the 5 x 5 binomial with scipy.ndimage's 'mirror' edges."""
    _f32_nd(x, 'laplacian_pyramid: x', 4)
    N, H, W, C = (int(s) for s in x.shape)
    levels = int(levels)
    if levels < 1 or min(N, H, W) <= 0 or not 1 <= C <= 4 or H % (1 << (levels - 1)) or W % (1 << (levels - 1)) or \
            min(H, W) >> (levels - 1) < 7:
        raise ValueError('laplacian_pyramid: %d levels of %s need C in 1..4 and sides that are multiples of 2^(levels-1) with a '
                         'coarsest side of at least 7' % (levels, tuple(x.shape)))
    offs, total = pyramid_offsets(N, H, W, C, levels)
    out = torch.empty(total, dtype=torch.float32, device=x.device)
    if _live(x):
        wsp, wsn = _ws_args(x, int(lib.t2i_laplacian_pyramid_workspace_bytes(N, H, W, C, levels)))
        check(lib.t2i_laplacian_pyramid(_ptr(x), N, H, W, C, levels, _ptr(out), wsp, wsn, _stream()), 't2i_laplacian_pyramid')
    return [out[o:o + N * (H >> i) * (W >> i) * C].view(N, H >> i, W >> i, C) for i, o in enumerate(offs)]


def swd_descriptors(level, pos, out, row0):
    """Rows row0 + n P + p of out [rows_total, 49 C] = the 7 x 7 x C neighbourhood of level [N,h,w,C] around (y, x) = pos[n, p],
    flattened (c, dy, dx).  pos: an integer array or tensor [N,P,2] on the HOST, every centre in [3, side - 3) (checked here; the
    kernel also clamps)."""
    _f32_nd(level, 'swd_descriptors: level', 4); _f32_nd(out, 'swd_descriptors: out', 2)
    N, h, w, C = (int(s) for s in level.shape)
    pos = torch.as_tensor(pos)
    if pos.is_cuda or pos.dim() != 3 or pos.shape[0] != N or pos.shape[2] != 2 or pos.shape[1] == 0 or pos.is_floating_point():
        raise ValueError('swd_descriptors: pos must be a host integer [N=%d, P, 2] table, got %s %s' % (N, pos.dtype, tuple(pos.shape)))
    P = int(pos.shape[1])
    if min(h, w) < 7 or int(pos[..., 0].min()) < 3 or int(pos[..., 0].max()) >= h - 3 or int(pos[..., 1].min()) < 3 or \
            int(pos[..., 1].max()) >= w - 3:
        raise ValueError('swd_descriptors: a centre lies outside [3, side - 3) of a %d x %d level' % (h, w))
    row0 = int(row0)
    if out.shape[1] != 49 * C or row0 < 0 or row0 + N * P > out.shape[0] or out.device != level.device:
        raise ValueError('swd_descriptors: rows %d..%d of a %s store on %s cannot take %d x %d descriptors of %d floats from %s' % (
            row0, row0 + N * P, tuple(out.shape), out.device, N, P, 49 * C, level.device))
    if _live(level):
        p = pos.to(torch.int32).contiguous().to(level.device)
        check(lib.t2i_swd_descriptors(_ptr(level), N, h, w, C, _ptr(p), P, _ptr(out), row0, out.shape[0], _stream()), 't2i_swd_descriptors')
    return out


def swd_channel_stats(A, C):
    """A float32 [rows, 49 C] -> (mean, std): float64 [C] each, per channel over all rows and its 49 columns, std with ddof 0."""
    _f32_nd(A, 'swd_channel_stats: A', 2)
    rows, C = int(A.shape[0]), int(C)
    if rows <= 0 or not 1 <= C <= 4 or A.shape[1] != 49 * C:
        raise ValueError('swd_channel_stats: A %s is not a non-empty [rows, 49 * %d] store with C in 1..4' % (tuple(A.shape), C))
    mean = torch.empty(C, dtype=torch.float64, device=A.device)
    std = torch.empty(C, dtype=torch.float64, device=A.device)
    if _live(A):
        wsp, wsn = _ws_args(A, int(lib.t2i_swd_channel_stats_workspace_bytes(rows, C)))
        check(lib.t2i_swd_channel_stats(_ptr(A), rows, C, _ptr(mean), _ptr(std), wsp, wsn, _stream()), 't2i_swd_channel_stats')
    return mean, std


def next_pow2(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def swd_project(A, mean, std, dirs, out=None):
    """out [S, rows_pad] (rows_pad = next_pow2(rows), or that of `out`) with out[s][r] = sum_j ((A[r][j] - mean_c) / std_c)
    dirs[j][s] and +inf for r >= rows.  A float32 [rows, 49 C], mean / std float64 [C], dirs float32 [49 C, S]."""
    _f32_nd(A, 'swd_project: A', 2); _f32_nd(dirs, 'swd_project: dirs', 2)
    rows, D = (int(s) for s in A.shape)
    C, S = D // 49, int(dirs.shape[1])
    if rows <= 0 or S <= 0 or D != 49 * C or not 1 <= C <= 4 or dirs.shape[0] != D:
        raise ValueError('swd_project: A %s and dirs %s are not [rows, 49 C] and [49 C, S] with C in 1..4' % (tuple(A.shape), tuple(dirs.shape)))
    for t, name in ((mean, 'mean'), (std, 'std')):
        if t.dtype != torch.float64 or tuple(t.shape) != (C,) or not t.is_contiguous() or t.device != A.device:
            raise ValueError('swd_project: %s must be a contiguous float64 [%d] on %s' % (name, C, A.device))
    if out is None:
        out = torch.empty((S, next_pow2(rows)), dtype=torch.float32, device=A.device)
    _f32_nd(out, 'swd_project: out', 2)
    rows_pad = int(out.shape[1])
    if out.shape[0] != S or rows_pad < rows or rows_pad & (rows_pad - 1) or out.device != A.device or dirs.device != A.device:
        raise ValueError('swd_project: out %s must be [%d, a power of two >= %d] on %s' % (tuple(out.shape), S, rows, A.device))
    if _live(A):
        check(lib.t2i_swd_project(_ptr(A), rows, C, _ptr(mean), _ptr(std), _ptr(dirs), S, _ptr(out), rows_pad, _stream()), 't2i_swd_project')
    return out


SORT_CHUNK = int(lib.t2i_segmented_sort_chunk())      # elements one workgroup sorts in LDS (include/t2i_hip.h T2I_SORT_CHUNK)


def segmented_sort(data):
    """Sorts every row of data float32 [segments, len] ascending, in place (len a power of two; no NaN by contract, +inf last)."""
    _f32_nd(data, 'segmented_sort: data', 2)
    segments, n = (int(s) for s in data.shape)
    if segments <= 0 or n <= 0 or n & (n - 1):
        raise ValueError('segmented_sort: %s is not [segments, a power of two]' % (tuple(data.shape),))
    if _live(data):
        check(lib.t2i_segmented_sort_f32(_ptr(data), segments, n, _stream()), 't2i_segmented_sort_f32')
    return data


def sorted_l1_mean(a, b, rows):
    """mean |a - b| over the first `rows` entries of every row of a, b float32 [segments, len] -> float64 [1] on the device."""
    _f32_nd(a, 'sorted_l1_mean: a', 2); _f32_nd(b, 'sorted_l1_mean: b', 2)
    segments, n = (int(s) for s in a.shape)
    rows = int(rows)
    if tuple(a.shape) != tuple(b.shape) or segments <= 0 or not 1 <= rows <= n or a.device != b.device:
        raise ValueError('sorted_l1_mean: a %s, b %s, rows %d' % (tuple(a.shape), tuple(b.shape), rows))
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    if _live(a):
        wsp, wsn = _ws_args(a, int(lib.t2i_sorted_l1_mean_workspace_bytes(segments, rows)))
        check(lib.t2i_sorted_l1_mean(_ptr(a), _ptr(b), segments, n, rows, _ptr(out), wsp, wsn, _stream()), 't2i_sorted_l1_mean')
    return out


# ---- multi-scale structural similarity (csrc/t2i_msssim.hip; evaluation/msssim.py is the caller) ------------------------------
SSIM_MAX_WINDOW = CONSTANTS['T2I_SSIM_MAX_WINDOW']


def msssim_window(h, w, filter_size=11, sigma=1.5):
    """The 1-D Gaussian window of a scale of size h x w: float64 [S], S = min(filter_size, h, w), sigma scaled by S / filter_size,
    g[i] = exp(-x_i^2 / 2 sigma^2) normalised to sum 1 with x_i = i - S // 2 (+ 0.5 for even S).  outer(g, g) is the 2-D normalised
    Gaussian of ms_ssim.py's _FSpecialGauss."""
    h, w, filter_size = int(h), int(w), int(filter_size)
    if min(h, w, filter_size) < 1 or not float(sigma) > 0:
        raise ValueError('msssim_window: a %d x %d scale, filter_size %d and sigma %r' % (h, w, filter_size, sigma))
    S = min(filter_size, h, w)
    sig = S * float(sigma) / filter_size
    x = np.arange(S, dtype=np.float64) - S // 2 + (0.5 if S % 2 == 0 else 0.0)
    g = np.exp(-(x * x) / (2.0 * sig * sig))
    return g / g.sum()


def ssim_scale(a, b, window, c1, c2, downsample=True):
    """One MS-SSIM scale of the pairs a[n], b[n] (device float32 [N,H,W,C], C in 1..4): -> (ssim, cs, a_half, b_half), ssim and cs
    float64 [N] on the device, a_half / b_half the next scale [N, ceil(H/2), ceil(W/2), C] (None, None without downsample).
    window: float64 [S] on the host (msssim_window), S <= min(11, H, W).  t2i_ssim_scale: every moment in fp64, fixed-order sums."""
    _f32_nd(a, 'ssim_scale: a', 4); _f32_nd(b, 'ssim_scale: b', 4)
    if tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise ValueError('ssim_scale: a %s on %s and b %s on %s must match' % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    N, H, W, C = (int(s) for s in a.shape)
    win = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
    S = int(win.size)
    if win.ndim != 1 or min(N, H, W) < 1 or not 1 <= C <= 4 or not 1 <= S <= min(SSIM_MAX_WINDOW, H, W) or N * H * W * C >= 1 << 31:
        raise ValueError('ssim_scale: %s pairs with a window of %s: C in 1..4, 1 <= S <= min(%d, H, W), fewer than 2^31 elements' % (
            tuple(a.shape), tuple(win.shape), SSIM_MAX_WINDOW))
    c1, c2 = float(c1), float(c2)
    if not (np.all(np.isfinite(win)) and np.isfinite(c1) and np.isfinite(c2) and c2 > 0):
        raise ValueError('ssim_scale: the window, c1 = %r and c2 = %r must be finite and c2 positive' % (c1, c2))
    ssim = torch.empty(N, dtype=torch.float64, device=a.device)
    cs = torch.empty(N, dtype=torch.float64, device=a.device)
    ah = bh = None
    if downsample:
        ah = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), dtype=torch.float32, device=a.device)
        bh = torch.empty_like(ah)
    if _live(a):
        wsp, wsn = _ws_args(a, int(lib.t2i_ssim_scale_workspace_bytes(N, H, W, C)))
        check(lib.t2i_ssim_scale(_ptr(a), _ptr(b), N, H, W, C, win.ctypes.data_as(ctypes.c_void_p), S, c1, c2, _ptr(ssim), _ptr(cs),
                                 _ptr(ah), _ptr(bh), wsp, wsn, _stream()), 't2i_ssim_scale')
    return ssim, cs, ah, bh


# ---- k-nearest-neighbour distances and ball counts in fp64 (csrc/t2i_knn.hip; evaluation/prdc.py is the caller) ----------------
KNN_MAX_K = CONSTANTS['T2I_KNN_MAX_K']
KNN_MAX_SEGMENTS = 65536


def _knn_sets(q, r, name, segments):
    _f32_nd(q, '%s: q' % name, 2); _f32_nd(r, '%s: r' % name, 2)
    if q.shape[1] != r.shape[1] or q.device != r.device:
        raise ValueError('%s: q %s on %s and r %s on %s must share the feature dimension and the device' % (
            name, tuple(q.shape), q.device, tuple(r.shape), r.device))
    M, D = (int(s) for s in q.shape)
    N = int(r.shape[0])
    segments = int(segments)
    if min(M, N, D) < 1 or max(M, N) * D >= 1 << 37 or not 0 <= segments <= min(N, KNN_MAX_SEGMENTS):
        raise ValueError('%s: q %s, r %s, segments %d: M, N, D >= 1, fewer than 2^37 elements per set, 0 <= segments <= min(N, %d)' % (
            name, tuple(q.shape), tuple(r.shape), segments, KNN_MAX_SEGMENTS))
    return M, N, D, segments


def knn_dist2(q, r, k, exclude_self=False, segments=0, out=None):
    """The k smallest squared distances from every row of q [M, D] to the rows of r [N, D] (device float32): float64 [M, k],
    ascending.  d2 = max(|q|^2 + |r|^2 - 2 q.r, 0) with the three sums in fp64 (t2i_knn_dist2).  exclude_self (M == N) skips candidate
    n == m by index.  segments splits the candidates over workgroups (0: the library chooses); the result does not depend on it."""
    M, N, D, segments = _knn_sets(q, r, 'knn_dist2', segments)
    k, ex = int(k), int(bool(exclude_self))
    if not 1 <= k <= KNN_MAX_K or k > N - ex or (ex and M != N):
        raise ValueError('knn_dist2: k = %d of %d candidates (exclude_self %d, %d queries): k in 1..%d, k <= N - exclude_self, '
                         'exclude_self only with M == N' % (k, N, ex, M, KNN_MAX_K))
    if out is None:
        out = torch.empty((M, k), dtype=torch.float64, device=q.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (M, k) or not out.is_contiguous() or out.device != q.device:
        raise ValueError('knn_dist2: out must be a contiguous float64 [%d, %d] tensor on %s, got %s %s on %s' % (
            M, k, q.device, out.dtype, tuple(out.shape), out.device))
    if _live(q):
        wsp, wsn = _ws_args(q, int(lib.t2i_knn_dist2_workspace_bytes(M, N, D, k, segments)))
        check(lib.t2i_knn_dist2(_ptr(q), M, _ptr(r), N, D, k, ex, segments, _ptr(out), wsp, wsn, _stream()), 't2i_knn_dist2')
    return out


def ball_counts(q, r, r2, segments=0):
    """-> (count int32 [M], dmin float64 [M]): count[m] = #{n : d2(q[m], r[n]) <= r2[n]}, dmin[m] = min_n d2(q[m], r[n]), both from
    one pass (t2i_ball_counts; d2 as in knn_dist2).  r2: device float64 [N]."""
    M, N, D, segments = _knn_sets(q, r, 'ball_counts', segments)
    if r2.dtype != torch.float64 or tuple(r2.shape) != (N,) or not r2.is_contiguous() or r2.device != q.device:
        raise ValueError('ball_counts: r2 must be a contiguous float64 [%d] tensor on %s, got %s %s on %s' % (
            N, q.device, r2.dtype, tuple(r2.shape), r2.device))
    count = torch.empty(M, dtype=torch.int32, device=q.device)
    dmin = torch.empty(M, dtype=torch.float64, device=q.device)
    if _live(q):
        wsp, wsn = _ws_args(q, int(lib.t2i_ball_counts_workspace_bytes(M, N, D, segments)))
        check(lib.t2i_ball_counts(_ptr(q), M, _ptr(r), N, D, _ptr(r2), segments, _ptr(count), _ptr(dmin), wsp, wsn, _stream()),
              't2i_ball_counts')
    return count, dmin


# ---- the kernel sums of the polynomial-kernel MMD^2 in fp64 (csrc/t2i_mmd.hip; evaluation/mmd.py is the caller) ------------------
MMD_MAX_DEGREE = 8
MMD_MAX_ITEMS = 1 << 30


def poly_mmd_items(S, m):
    """Work items (= workgroups) of poly_mmd_sums: per subset the 64 x 128 tiles of x.y and, of x.x and y.y, those that hold a pair
    i < j (row tile ti has the column tiles ti // 2 and above)."""
    nrt, nct = (m + 63) // 64, (m + 127) // 128
    a = nrt // 2                                          # row tiles 2 a' and 2 a' + 1 have nct - a' column tiles each
    sym = 2 * a * nct - a * (a - 1) + (nct - a if nrt % 2 else 0)
    return S * (2 * sym + nrt * nct)


def poly_mmd_sums(x, y, ix, iy, degree=3, gamma=None, coef0=1.0, check_indices=True):
    """-> float64 [S, 3]: per subset s the sums P_xx = sum_{i<j} k(x_i, x_j), P_yy and S_xy = sum_{i,j} k(x_i, y_j) of the polynomial
    kernel k(a, b) = (gamma a.b + coef0)^degree over the rows x[ix[s]] and y[iy[s]], i and j positions in the subset
    (t2i_poly_mmd_sums: every product in fp64, no m x m matrix, no gathered copy).  x [NX, D], y [NY, D] device float32 (they may be
    the same tensor), ix, iy device int32 [S, m]; gamma None = 1 / D.  check_indices does one device min / max over the tables and
    raises on an index out of range (a synchronisation: pass False inside a graph capture, where such an index makes its subset's
    sums NaN and is never dereferenced)."""
    name = 'poly_mmd_sums'
    _f32_nd(x, '%s: x' % name, 2); _f32_nd(y, '%s: y' % name, 2)
    if x.shape[1] != y.shape[1] or x.device != y.device:
        raise ValueError('%s: x %s on %s and y %s on %s must share the feature dimension and the device' % (
            name, tuple(x.shape), x.device, tuple(y.shape), y.device))
    for t, tn in ((ix, 'ix'), (iy, 'iy')):
        if t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous() or t.device != x.device:
            raise ValueError('%s: %s must be a contiguous int32 [S, m] tensor on %s, got %s %s on %s' % (
                name, tn, x.device, t.dtype, tuple(t.shape), t.device))
    if tuple(ix.shape) != tuple(iy.shape):
        raise ValueError('%s: ix %s and iy %s must have the same shape' % (name, tuple(ix.shape), tuple(iy.shape)))
    NX, D = (int(s) for s in x.shape)
    NY = int(y.shape[0])
    S, m = (int(s) for s in ix.shape)
    degree, coef0 = int(degree), float(coef0)
    gamma = 1.0 / max(D, 1) if gamma is None else float(gamma)
    if min(NX, NY, D, S) < 1 or m < 2 or max(NX, NY) * D >= 1 << 37 or m >= 1 << 31 or S >= 1 << 31:
        raise ValueError('%s: x %s, y %s, tables %s: NX, NY, D, S >= 1, m >= 2, fewer than 2^37 elements per set' % (
            name, tuple(x.shape), tuple(y.shape), tuple(ix.shape)))
    if not 1 <= degree <= MMD_MAX_DEGREE or not (np.isfinite(gamma) and np.isfinite(coef0)):
        raise ValueError('%s: degree %d, gamma %r, coef0 %r: degree in 1..%d, gamma and coef0 finite' % (
            name, degree, gamma, coef0, MMD_MAX_DEGREE))
    if poly_mmd_items(S, m) > MMD_MAX_ITEMS:
        raise ValueError('%s: %d subsets of %d rows are %d work items, more than 2^30: score the subsets in several calls' % (
            name, S, m, poly_mmd_items(S, m)))
    sums = torch.empty((S, 3), dtype=torch.float64, device=x.device)
    if _live(x):
        if check_indices:
            for t, tn, n in ((ix, 'ix', NX), (iy, 'iy', NY)):
                lo, hi = (int(v) for v in torch.stack(torch.aminmax(t)).cpu())
                if lo < 0 or hi >= n:
                    raise ValueError('%s: %s holds indices %d..%d, the set has rows 0..%d' % (name, tn, lo, hi, n - 1))
        wsp, wsn = _ws_args(x, int(lib.t2i_poly_mmd_sums_workspace_bytes(NX, NY, D, S, m)))
        check(lib.t2i_poly_mmd_sums(_ptr(x), NX, _ptr(y), NY, D, _ptr(ix), _ptr(iy), S, m, degree, gamma, coef0, _ptr(sums), wsp, wsn,
                                    _stream()), 't2i_poly_mmd_sums')
    return sums
