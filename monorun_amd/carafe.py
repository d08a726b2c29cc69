"""CARAFE, the NOC head trunk's upsampler (N10): ``mmcv.ops.carafe`` (``carafe``, ``CARAFEPack``) without mmcv, whose
op is a CUDA extension with no ROCm build.

The op.  Features ``x`` (N, C, H, W); up-kernel ``k`` (odd), group count ``G`` (divides C), scale ``s``; normalised masks ``w``
(N, G·k², H·s, W·s); output (N, C, H·s, W·s)::

    out[n,c,ph,pw] = Σ_{iy,ix<k} x[n, c, ph//s + iy − (k−1)/2, pw//s + ix − (k−1)/2] · w[n, (g·k + iy)·k + ix, ph, pw],   g = c // (C/G)

with taps outside the feature map contributing zero.  ``CARAFEPack.forward`` wraps it: ``m = content_encoder(channel_compressor(x))``
of shape (N, k²·G·s², H, W); ``pixel_shuffle(m, s)`` (input channel ``c·s² + dy·s + dx`` goes to output channel ``c`` at
``(h·s+dy, w·s+dx)``); a softmax over the k² taps of each group at each output pixel gives ``w``.

Hot path: :func:`carafe_pack` on CUDA fp32 runs ONE fused HIP launch forward (``mr_carafe_pack_forward``: pixel-shuffle indexing,
softmax and reassembly; the masks never reach memory) and two backward (``mr_carafe_pack_backward``; no atomics, bitwise
reproducible).  Everything else — CPU, other dtypes, no RoIs, other ``k`` / ``s``, a backward under ``create_graph=True`` — runs
:func:`carafe_pack_torch`, the torch restatement (a loop over the k² taps with shifted, zero-padded views; no ``unfold``).  The plain op
:func:`carafe` on given masks is served by the restatement on every device.  The two convolutions of :class:`CARAFEPack` are
``torch.nn.functional.conv2d``.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

MAX_KERNEL = 7          # MR_CARAFE_MAX_KERNEL of include/monorun_carafe.h
CHUNK = 32              # MR_CARAFE_CHUNK: channels a workgroup stages at a time
TILE = 16               # MR_CARAFE_TILE: source pixels per tile side
SCALES = (1, 2, 4)


def carafe(features, masks, kernel_size, group_size, scale_factor):
    """The plain op on normalised masks, as ``mmcv.ops.carafe`` exposes it: features (N, C, H, W), masks (N, G·k², H·s, W·s) ->
    (N, C, H·s, W·s).  Plain differentiable torch on any device and floating dtype: one shifted, zero-padded view of the features per
    tap, upsampled by repetition and weighted."""
    k, G, s = int(kernel_size), int(group_size), int(scale_factor)
    N, C, H, W = features.shape
    assert k >= 1 and s >= 1 and G >= 1 and C % G == 0, 'carafe: kernel_size, scale_factor >= 1 and group_size must divide the channels'
    assert masks.shape == (N, G * k * k, H * s, W * s), f'carafe: masks of shape {tuple(masks.shape)}, expected {(N, G * k * k, H * s, W * s)}'
    r = (k - 1) // 2
    xp = F.pad(features, (r, k - 1 - r, r, k - 1 - r))
    wv = masks.reshape(N, G, k * k, 1, H * s, W * s)
    out = None
    for t in range(k * k):
        iy, ix = divmod(t, k)
        tap = xp[:, :, iy:iy + H, ix:ix + W]
        tap = tap[:, :, :, None, :, None].expand(N, C, H, s, W, s).reshape(N, G, C // G, H * s, W * s)
        term = tap * wv[:, :, t]
        out = term if out is None else out + term
    return out.reshape(N, C, H * s, W * s)


def normalize_masks(m, up_kernel, up_group, scale_factor):
    """``CARAFEPack.kernel_normalizer``: the raw encoder output (N, k²·G·s², H, W) -> the normalised masks (N, G·k², H·s, W·s)."""
    k, G, s = int(up_kernel), int(up_group), int(scale_factor)
    w = F.pixel_shuffle(m, s)
    n, _, hs, ws = w.shape
    return F.softmax(w.reshape(n, G, k * k, hs, ws), dim=2).reshape(n, G * k * k, hs, ws)


def carafe_pack_torch(x, m, up_kernel, up_group, scale_factor):
    """The fused op in plain torch: pixel shuffle, softmax over the taps, reassembly.  Differentiable on any device and any floating
    dtype; same arguments and result as :func:`carafe_pack`."""
    return carafe(x, normalize_masks(m, up_kernel, up_group, scale_factor), up_kernel, up_group, scale_factor)


def hip_ok(x, m, up_kernel, up_group, scale_factor):
    """Whether the fused HIP launches cover this call: CUDA fp32 tensors on one device, N > 0, k odd and <= 7, s in {1, 2, 4}, G dividing
    C, shapes that belong together, and a RoI whose maps keep 32-bit offsets."""
    if not (isinstance(x, torch.Tensor) and isinstance(m, torch.Tensor) and x.dim() == 4 and m.dim() == 4):
        return False
    if x.device.type != 'cuda' or m.device != x.device or x.dtype != torch.float32 or m.dtype != torch.float32:
        return False
    k, G, s = int(up_kernel), int(up_group), int(scale_factor)
    N, C, H, W = x.shape
    if N == 0 or C == 0 or H == 0 or W == 0 or k < 1 or k > MAX_KERNEL or k % 2 == 0 or s not in SCALES or G < 1 or C % G != 0:
        return False
    if m.shape != (N, G * k * k * s * s, H, W):
        return False
    lim = 2 ** 31 - 1
    return C * H * s * W * s <= lim and G * k * k * s * s * H * W <= lim


def _sizes(x, k, G, s):
    N, C, H, W = x.shape
    return dict(n=N, channels=C, h=H, w=W, up_kernel=k, up_group=G, scale_factor=s)


class _CarafePackFunction(torch.autograd.Function):
    """``mr_carafe_pack_forward`` forward, ``mr_carafe_pack_backward`` for the gradients to x and m; x and m arrive contiguous fp32 on one
    CUDA device.  Only x and m are saved: the backward recomputes the softmax."""

    @staticmethod
    def forward(ctx, x, m, k, G, s):
        N, C, H, W = x.shape
        out = torch.empty(N, C, H * s, W * s, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.call('mr_carafe_pack_forward', _sizes(x, k, G, s), x=x.data_ptr(), m=m.data_ptr(), out=out.data_ptr(),
                      stream=torch.cuda.current_stream(x.device).cuda_stream)
        ctx.save_for_backward(x, m)
        ctx.cfg = (k, G, s)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, m = ctx.saved_tensors
        k, G, s = ctx.cfg
        need_x, need_m = ctx.needs_input_grad[:2]
        if torch.is_grad_enabled():
            # create_graph=True: the gradients must carry a graph themselves, which the kernels cannot give: torch differentiates the restatement
            with torch.enable_grad():
                ins = [t for t, need in ((x, need_x), (m, need_m)) if need]
                got = iter(torch.autograd.grad(carafe_pack_torch(x, m, k, G, s), ins, grad_out, create_graph=True, allow_unused=True))
            return (next(got) if need_x else None, next(got) if need_m else None, None, None, None)
        lib = _lib.load()
        sizes = _sizes(x, k, G, s)
        go = grad_out.to(torch.float32).contiguous()
        grad_x = torch.empty_like(x) if need_x else None
        grad_m = torch.empty_like(m) if need_m else None
        nbytes = lib.mr_carafe_backward_workspace_bytes(*_lib.pack('mr_carafe_backward_workspace_bytes', sizes)) if need_x else 0
        work = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32) if need_x else None
        with torch.cuda.device(x.device):
            _lib.call('mr_carafe_pack_backward', sizes, x=x.data_ptr(), m=m.data_ptr(), grad_out=go.data_ptr(), workspace=_lib.ptr(work),
                      workspace_bytes=nbytes, grad_x=_lib.ptr(grad_x), grad_m=_lib.ptr(grad_m),
                      stream=torch.cuda.current_stream(x.device).cuda_stream)
        return grad_x, grad_m, None, None, None


def carafe_pack(x, m, up_kernel, up_group, scale_factor):
    """CARAFEPack's normaliser and reassembly on the raw encoder output: x (N, C, H, W), m (N, k²·G·s², H, W) -> (N, C, H·s, W·s),
    differentiable in x (the reassembly's direct path) and m.  The fused HIP launches when :func:`hip_ok`, else
    :func:`carafe_pack_torch`."""
    k, G, s = int(up_kernel), int(up_group), int(scale_factor)
    if not hip_ok(x, m, k, G, s):
        return carafe_pack_torch(x, m, k, G, s)
    return _CarafePackFunction.apply(x.contiguous(), m.contiguous(), k, G, s)


class CARAFEPack(nn.Module):
    """mmcv's ``CARAFEPack``: same constructor arguments, parameter names (``channel_compressor.weight/bias``,
    ``content_encoder.weight/bias``) and initialisation.  ``forward``: x (N, channels, H, W) -> (N, channels, H·s, W·s)."""

    def __init__(self, channels, scale_factor, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1, compressed_channels=64):
        super().__init__()
        self.channels = channels
        self.scale_factor = scale_factor
        self.up_kernel = up_kernel
        self.up_group = up_group
        self.encoder_kernel = encoder_kernel
        self.encoder_dilation = encoder_dilation
        self.compressed_channels = compressed_channels
        self.channel_compressor = nn.Conv2d(channels, compressed_channels, 1)
        self.content_encoder = nn.Conv2d(compressed_channels, up_kernel * up_kernel * up_group * scale_factor * scale_factor, encoder_kernel,
                                         padding=int((encoder_kernel - 1) * encoder_dilation / 2), dilation=encoder_dilation, groups=1)
        self.init_weights()

    def init_weights(self):
        for conv in (self.channel_compressor, self.content_encoder):
            nn.init.xavier_uniform_(conv.weight, gain=1)
            nn.init.constant_(conv.bias, 0)
        nn.init.normal_(self.content_encoder.weight, 0, 0.001)
        nn.init.constant_(self.content_encoder.bias, 0)

    def encode(self, x):
        """The raw masks ``content_encoder(channel_compressor(x))`` (N, k²·G·s², H, W): MIOpen's convolutions."""
        cc, ce = self.channel_compressor, self.content_encoder
        return F.conv2d(F.conv2d(x, cc.weight, cc.bias), ce.weight, ce.bias, padding=ce.padding, dilation=ce.dilation)

    def kernel_normalizer(self, mask):
        return normalize_masks(mask, self.up_kernel, self.up_group, self.scale_factor)

    def feature_reassemble(self, x, mask):
        return carafe(x, mask, self.up_kernel, self.up_group, self.scale_factor)

    def forward(self, x):
        return carafe_pack(x, self.encode(x), self.up_kernel, self.up_group, self.scale_factor)
