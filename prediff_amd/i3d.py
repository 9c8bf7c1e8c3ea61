"""Inception-v1 I3D (the feature network of the Fréchet video distance) as a HIP engine.

Constructor and ``state_dict`` schema follow the reference's ``InceptionI3d`` (evaluation/fvd/pytorch_i3d.py:133-306, final endpoint
``Logits``), so ``load_state_dict(torch.load("i3d_pretrained_400.pt"))`` works unchanged; nothing here fetches a checkpoint.  ``forward``
takes the preprocessed video (B, 3, T, 224, 224) in [-1, 1] and returns the (B, num_classes) features; ``features`` takes raw frames in any
layout and runs the reference's preprocessing (pd_i3d_preprocess) in front.  Dropout is the identity (evaluation mode).

Every ``Unit3D`` is convolution + evaluation-mode BatchNorm (eps 1e-5) + ReLU: the BatchNorm is folded into the weights and a bias in fp64
before the weights are rounded, and the layer is ONE pd_igemm launch with a ReLU epilogue.  TF-style SAME padding: the front pad goes in
the launch geometry, the back pad is the kernel's bounds check.  The four branches of an Inception module write straight into their column
ranges of one buffer (pointer offset + row length): there is no concat pass.  The stem (7x7x7, stride 2, 3 channels) reads the im2col
along W that the preprocess kernel writes (21 -> 64 columns at the stem's output stride) as a KT = 7, KH = 7, KW = 1 launch.

``precision``: "fp32" (default; this is a metric: bf16 hi/lo pairs, three products), "fp16" or "bf16" (one product).
"""
from typing import Sequence

import torch
from torch import nn

from . import _lib as L
from .engine import Act, HipEngine
from .packing import pack_conv, pad64, split_bf16
from .sevir_skill import axes_of

BN_EPS = 1e-5
MAX_FRAMES_PER_PASS = 384          # videos x frames of one pass through the network (bounds the workspace: 16 videos of 24 frames)


class Unit3D(nn.Module):
    """Parameter holder of the reference's Unit3D: `conv3d` [+ `bn`]."""

    def __init__(self, in_channels, output_channels, kernel_shape=(1, 1, 1), stride=(1, 1, 1), use_batch_norm=True, use_bias=False):
        super().__init__()
        self.kernel_shape, self.stride = tuple(kernel_shape), tuple(stride)
        self.conv3d = nn.Conv3d(in_channels, output_channels, self.kernel_shape, stride=self.stride, padding=0, bias=use_bias)
        if use_batch_norm:
            self.bn = nn.BatchNorm3d(output_channels, eps=BN_EPS, momentum=0.001)

    def forward(self, *a, **k):
        raise RuntimeError("parameter holder: InceptionI3d.forward runs the HIP engine")


class InceptionModule(nn.Module):
    def __init__(self, in_channels, out_channels: Sequence[int]):
        super().__init__()
        o = out_channels
        self.in_channels, self.out_channels = in_channels, tuple(o)
        self.b0 = Unit3D(in_channels, o[0])
        self.b1a = Unit3D(in_channels, o[1])
        self.b1b = Unit3D(o[1], o[2], (3, 3, 3))
        self.b2a = Unit3D(in_channels, o[3])
        self.b2b = Unit3D(o[3], o[4], (3, 3, 3))
        self.b3b = Unit3D(in_channels, o[5])

    forward = Unit3D.forward


# (endpoint, kind, arguments) in network order: "conv" (Cin, Cout, kernel, stride), "pool" (kernel, stride), "mixed" (Cin, six widths)
ARCH = (
    ("Conv3d_1a_7x7", "stem", (64,)),
    ("MaxPool3d_2a_3x3", "pool", ((1, 3, 3), (1, 2, 2))),
    ("Conv3d_2b_1x1", "conv", (64, 64, (1, 1, 1))),
    ("Conv3d_2c_3x3", "conv", (64, 192, (3, 3, 3))),
    ("MaxPool3d_3a_3x3", "pool", ((1, 3, 3), (1, 2, 2))),
    ("Mixed_3b", "mixed", (192, (64, 96, 128, 16, 32, 32))),
    ("Mixed_3c", "mixed", (256, (128, 128, 192, 32, 96, 64))),
    ("MaxPool3d_4a_3x3", "pool", ((3, 3, 3), (2, 2, 2))),
    ("Mixed_4b", "mixed", (480, (192, 96, 208, 16, 48, 64))),
    ("Mixed_4c", "mixed", (512, (160, 112, 224, 24, 64, 64))),
    ("Mixed_4d", "mixed", (512, (128, 128, 256, 24, 64, 64))),
    ("Mixed_4e", "mixed", (512, (112, 144, 288, 32, 64, 64))),
    ("Mixed_4f", "mixed", (528, (256, 160, 320, 32, 128, 128))),
    ("MaxPool3d_5a_2x2", "pool", ((2, 2, 2), (2, 2, 2))),
    ("Mixed_5b", "mixed", (832, (256, 160, 320, 32, 128, 128))),
    ("Mixed_5c", "mixed", (832, (384, 192, 384, 48, 128, 128))),
)
VALID_ENDPOINTS = tuple(a[0] for a in ARCH) + ("Logits", "Predictions")


class InceptionI3d(nn.Module, HipEngine):
    VALID_ENDPOINTS = VALID_ENDPOINTS

    def __init__(self, num_classes=400, spatial_squeeze=True, final_endpoint="Logits", name="inception_i3d", in_channels=3,
                 dropout_keep_prob=0.5, precision: str = "fp32"):
        if final_endpoint not in self.VALID_ENDPOINTS:
            raise ValueError("Unknown final endpoint %s" % final_endpoint)
        if final_endpoint != "Logits" or not spatial_squeeze:
            raise NotImplementedError("the HIP engine runs the whole network up to the squeezed `Logits` endpoint (the FVD features)")
        super().__init__()
        self._init_engine(precision, ("fp32", "fp16", "bf16"))
        self._num_classes, self.in_channels = num_classes, in_channels
        for ep, kind, args in ARCH:
            if kind == "stem":
                m = Unit3D(in_channels, args[0], (7, 7, 7), (2, 2, 2))
            elif kind == "conv":
                m = Unit3D(args[0], args[1], args[2])
            elif kind == "mixed":
                m = InceptionModule(*args)
            else:
                continue                      # pooling layers hold no state
            self.add_module(ep, m)
        self.logits = Unit3D(1024, num_classes, use_batch_norm=False, use_bias=True)
        self.requires_grad_(False)
        self.eval()

    # ------------------------------------------------------------------------------------------------ packing
    def _params_key(self, device):
        # the BatchNorm statistics are buffers: they are part of what is folded into the packed weights
        return super()._params_key(device) + tuple((b.data_ptr(), b._version) for b in self.buffers())

    @staticmethod
    def _fold(u: Unit3D):
        """conv + evaluation-mode BatchNorm -> (weight, bias) in fp64"""
        w = u.conv3d.weight.detach().double()
        b = u.conv3d.bias.detach().double() if u.conv3d.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
        if hasattr(u, "bn"):
            s = u.bn.weight.detach().double() / torch.sqrt(u.bn.running_var.detach().double() + u.bn.eps)
            w = w * s.view(-1, 1, 1, 1, 1)
            b = (b - u.bn.running_mean.detach().double()) * s + u.bn.bias.detach().double()
        return w, b

    def _pack(self, device):
        if self.in_channels != 3:
            raise L.PrediffHipError(f"InceptionI3d: the stem's operand is built for 3 input channels; got in_channels={self.in_channels}")
        split = self.precision == "fp32"
        P = {}
        for name, u in self.named_modules():
            if not isinstance(u, Unit3D) or name == "logits":
                continue
            w, b = self._fold(u)
            w, b = w.to(device), b.to(device)
            if name == "Conv3d_1a_7x7":
                # (n, c, kt, kh, kw) -> taps (kt, kh), columns 3 kw + c: the layout pd_i3d_preprocess writes along W
                n = w.shape[0]
                ws = torch.zeros(49, n, L.I3D_STEM_LD, dtype=torch.float32, device=device)
                ws[:, :, :21] = w.permute(2, 3, 0, 4, 1).reshape(49, n, 21).float()
                P[name + ".w"] = split_bf16(ws, split, self.op_dtype)
            else:
                P[name + ".w"] = pack_conv(w.float(), split, c_pad=pad64(w.shape[1]), dtype=self.op_dtype)
            P[name + ".b"] = b.float().contiguous()
        w, b = self._fold(self.logits)
        P["logits.w32"] = w.reshape(w.shape[0], -1).float().contiguous().to(device)
        P["logits.b"] = b.float().contiguous().to(device)
        return P

    # ------------------------------------------------------------------------------------------------ layers
    def _unit(self, P, name, a: Act, B, thw, Cout, kernel=(1, 1, 1), stride=(1, 1, 1), out_f32=None, out_op=None, ld_out=None, ld_outb=None):
        """conv + folded BatchNorm + ReLU of layer `name` on the rows of `a`; returns the output (T, H, W)."""
        out_thw = tuple(L.same_out(k, s, n) for k, s, n in zip(kernel, stride, thw))
        if tuple(kernel) == (1, 1, 1) and tuple(stride) == (1, 1, 1):
            geom, taps = None, 1
        else:
            pads = tuple(L.same_pad(k, s, n) // 2 for k, s, n in zip(kernel, stride, thw))
            geom, taps = L.conv_geom(B, thw, kernel, stride=stride, pad=pads, out_thw=out_thw), kernel[0] * kernel[1] * kernel[2]
        hi, lo = out_op if out_op is not None else (None, None)
        self._gemm(P, name, a, M=B * out_thw[0] * out_thw[1] * out_thw[2], N=Cout, taps=taps, geom=geom, act="relu", out_f32=out_f32,
                   out_bf16=hi, out_bf16_lo=lo, ld_out=ld_out, ld_outb=ld_outb)
        return out_thw

    def _pool(self, name, x, B, thw, C, kernel, stride, dev, want_f32, want_op):
        """SAME max-pool of fp32 rows x (B, *thw, C) -> (fp32 rows or None, operand Act or None, output thw)"""
        out_thw = tuple(L.same_out(k, s, n) for k, s, n in zip(kernel, stride, thw))
        rows = B * out_thw[0] * out_thw[1] * out_thw[2]
        of = self._buf(name + ".f32", (rows, C), torch.float32, dev) if want_f32 else None
        hi, lo = self._bf(name + ".op", rows, pad64(C), dev) if want_op else (None, None)
        L.maxpool3d_same(x, B, thw, C, kernel, stride, out_f32=of, outb=hi, outb_lo=lo, opts=self.opts)
        return of, (Act(hi, lo, pad64(C)) if want_op else None), out_thw

    def _mixed(self, P, name, x32, a: Act, B, thw, Cin, widths, dev, want_op):
        o0, o1a, o1b, o2a, o2b, o3 = widths
        Ct = o0 + o1b + o2b + o3
        rows = B * thw[0] * thw[1] * thw[2]
        of = self._buf(name + ".f32", (rows, Ct), torch.float32, dev)
        hi, lo = self._bf(name + ".op", rows, pad64(Ct), dev) if want_op else (None, None)

        def dest(off):
            return dict(out_f32=of[:, off:], ld_out=Ct, ld_outb=pad64(Ct),
                        out_op=(hi[:, off:], lo[:, off:] if lo is not None else None) if want_op else None)

        self._unit(P, name + ".b0", a, B, thw, o0, **dest(0))
        for br, ca, cb, off in (("b1", o1a, o1b, o0), ("b2", o2a, o2b, o0 + o1b)):
            t = self._bf(name + "." + br + "a", rows, pad64(ca), dev)
            self._unit(P, name + "." + br + "a", a, B, thw, ca, out_op=t, ld_outb=pad64(ca))
            self._unit(P, name + "." + br + "b", Act(*t, pad64(ca)), B, thw, cb, kernel=(3, 3, 3), **dest(off))
        _, pa, _ = self._pool(name + ".b3a", x32, B, thw, Cin, (3, 3, 3), (1, 1, 1), dev, False, True)
        self._unit(P, name + ".b3b", pa, B, thw, o3, **dest(o0 + o1b + o2b))
        return of, (Act(hi, lo, pad64(Ct)) if want_op else None), Ct

    def _network(self, P, stem: Act, B, T, dev):
        """The network behind the preprocess kernel: `stem` = its operand rows for B videos of T frames -> (B, num_classes) fp32."""
        x32 = a = None
        thw, C = (T, L.I3D_RES, L.I3D_RES), 3
        for i, (ep, kind, args) in enumerate(ARCH):
            nxt = ARCH[i + 1][1] if i + 1 < len(ARCH) else "head"
            want_f32, want_op = nxt in ("pool", "mixed", "head"), nxt in ("conv", "mixed")
            if kind == "stem":
                To = L.same_out(7, 2, T)
                x32 = self._buf(ep + ".f32", (B * To * 112 * 112, args[0]), torch.float32, dev)
                geom = L.conv_geom(B, (T, L.I3D_RES, L.I3D_STEM_WO), (7, 7, 1), stride=(2, 2, 1),
                                   pad=(L.same_pad(7, 2, T) // 2, L.same_pad(7, 2, L.I3D_RES) // 2, 0), out_thw=(To, 112, 112))
                self._gemm(P, ep, stem, M=B * To * 112 * 112, N=args[0], taps=49, geom=geom, act="relu", out_f32=x32)
                thw, C = (To, 112, 112), args[0]
            elif kind == "pool":
                x32, a, thw = self._pool(ep, x32, B, thw, C, args[0], args[1], dev, want_f32, want_op)
            elif kind == "conv":
                Cout, kernel = args[1], args[2]
                rows = B * thw[0] * thw[1] * thw[2]
                x32 = self._buf(ep + ".f32", (rows, Cout), torch.float32, dev) if want_f32 else None
                op = self._bf(ep + ".op", rows, pad64(Cout), dev) if want_op else None
                self._unit(P, ep, a, B, thw, Cout, kernel=kernel, out_f32=x32, out_op=op, ld_outb=pad64(Cout))
                a, C = (Act(*op, pad64(Cout)) if want_op else None), Cout
            else:
                x32, a, C = self._mixed(P, ep, x32, a, B, thw, args[0], args[1], dev, want_op)
        if thw[0] < 2 or thw[1:] != (7, 7):
            raise L.PrediffHipError(f"InceptionI3d: the (2, 7, 7) average pool needs a (>= 2, 7, 7) map; got {thw} (at least 9 frames of 224 x 224)")
        pooled = self._buf("head.pooled", (B, C), torch.float32, dev)
        out = torch.empty((B, self._num_classes), dtype=torch.float32, device=dev)
        L.i3d_head(x32, P["logits.w32"], P["logits.b"], pooled, out, B, thw[0], 49, C, self._num_classes)
        return out

    # ------------------------------------------------------------------------------------------------ entry points
    def _run(self, x, layout, normalize, auto_t, rescale):
        """x: fp32 frames in `layout`, read in place through their strides, at most MAX_FRAMES_PER_PASS frames per pass"""
        dev = x.device
        sizes, strides = axes_of(layout, x)
        N, T = sizes[0], sizes[1] * (2 if auto_t else 1)
        with L.on_device(x):
            P = self._ensure_packed(dev)
            step = max(1, MAX_FRAMES_PER_PASS // T)
            outs = []
            for n0 in range(0, N, step):
                B = min(step, N - n0)
                a = self._bf("stem.a", B * T * L.I3D_RES * L.I3D_STEM_WO, L.I3D_STEM_LD, dev)
                L.i3d_preprocess(x.narrow(layout.find("N"), n0, B), [B] + list(sizes[1:]), strides, normalize, auto_t, *a, rescale=rescale, opts=self.opts)
                outs.append(self._network(P, Act(*a, L.I3D_STEM_LD), B, T, dev))
            return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def features(self, videos: torch.Tensor, layout: str = "NTCHW", normalize: bool = False, auto_t: bool = False) -> torch.Tensor:
        """I3DWrapper.forward on raw frames: values in [0, 1] (or [0, 255] with `normalize`), 1 or 3 channels, any layout of N, T, H, W, C,
        read in place; `auto_t` repeats every frame twice.  Returns (N, num_classes) fp32 features."""
        if videos.dim() != len(layout) or set(layout) - set("NTHWC") or len(set(layout)) != len(layout) or not set("NTHW") <= set(layout):
            raise ValueError(f"layout {layout!r} (N, T, H, W and optionally C, each once) does not describe a tensor of shape {tuple(videos.shape)}")
        if not videos.is_cuda:
            raise L.PrediffHipError("InceptionI3d runs on the HIP device; got a CPU tensor")
        x = videos.detach().float()
        if axes_of(layout, x)[0][4] not in (1, 3):
            raise ValueError(f"videos must have 1 or 3 channels; got {axes_of(layout, x)[0][4]}")
        return self._run(x, layout, normalize, auto_t, True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, 3, T, 224, 224) in [-1, 1] (the preprocessed video) -> (B, num_classes) features."""
        if x.dim() != 5 or x.shape[1] != 3 or tuple(x.shape[3:]) != (L.I3D_RES, L.I3D_RES):
            raise ValueError(f"InceptionI3d.forward takes (B, 3, T, 224, 224); got {tuple(x.shape)}")
        if not x.is_cuda:
            raise L.PrediffHipError("InceptionI3d runs on the HIP device; got a CPU tensor")
        return self._run(x.detach().float(), "NCTHW", False, False, False)
