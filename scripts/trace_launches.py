#!/usr/bin/env python
"""Launch trace + output hashes of seeded forwards: the tool that shows a host-side refactor changed neither what is launched nor a bit.

Every public callable of prediff_amd._lib that launches a kernel is wrapped.  For one seeded forward per case, <out>/<case>.trace gets
one line per launch: the function name and every argument after binding to the wrapper's signature (defaults included), scalars as they
are, tensors as (dtype, shape) only -- pointer values are deliberately not recorded --, a CallOpts as its _state().  <out>/hashes.txt
gets the SHA-256 of the raw bytes of each case's output, and of one 5-step ddim_sample_loop at bf16 (graph replay: hashed, not traced).

Cases: the v1 denoiser at each of its seven precisions, B = 2 (the split-K / small-grid mode) and B = 32; VAE encode and decode at bf16
and fp32.  Run it on two checkouts and `diff -r` the two output directories:
    python scripts/trace_launches.py --out /tmp/trace_a        (needs an MI355X)

--stub: the host side alone, no device.  The launching callables are replaced by stubs that bind their arguments and return; packing runs
for real, the workspace is CPU tensors of the real shapes, the forwards are entered below their is-this-a-device-tensor checks.  Traces
only (the outputs mean nothing).  The cheap CPU run also covers what the device cases do not reach: every denoiser case again with
fuse_pair, fuse_attn, fuse_ffn and fuse_ffn_rows switched off one after the other (no repack: the un-fused _attention / _ffn branches,
their e4m3 forms, the folded linears), and the VAE at fp16 and with fuse_resblock off.
"""
import argparse
import functools
import hashlib
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd import _lib as L  # noqa: E402
from prediff_amd.autoencoder_kl import AutoencoderKL  # noqa: E402
from prediff_amd.cuboid_transformer_unet import CuboidTransformerUNet  # noqa: E402
from prediff_amd.latent_diffusion import LatentDiffusion  # noqa: E402
from prediff_amd.presets import V1_LDM_KW, V1_UNET_CFG, V1_VAE_CFG  # noqa: E402
from prediff_amd.seeding import seeded_input, seeded_state_dict  # noqa: E402

PRECISIONS = ("bf16", "fp16", "fp16x2", "fp16x2_lin", "fp32", "fp8", "fp8_conv")
# public functions of _lib that launch nothing: loaders, pointer / stream helpers, geometry and capability queries, host tables
NOT_A_LAUNCH = {"lib", "stream_ptr", "on_device", "ptr", "pad64", "conv_geom", "groupnorm_nchunk", "timestep_freqs",
                "attn_ffn_pair_cuboids_per_group", "attn_ffn_pair_split_ws_floats", "ensemble_score_ws_doubles", "frame_score_ws_doubles"}


def launchers():
    return sorted(n for n, f in vars(L).items() if inspect.isfunction(f) and f.__module__ == L.__name__ and not n.startswith("_")
                  and n not in NOT_A_LAUNCH and not n.endswith("_supported"))


def describe(v):
    if isinstance(v, torch.Tensor):
        return f"<{str(v.dtype).replace('torch.', '')}{list(v.shape)}>"
    if isinstance(v, L.CallOpts):
        return "CallOpts" + describe(v._state())
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}={describe(x)}" for k, x in sorted(v.items())) + "}"
    if isinstance(v, (list, tuple)):
        return "(" + ", ".join(describe(x) for x in v) + ")"
    return repr(v)


class Tracer:
    """Context manager: while active, every launch through the module attributes of _lib appends one line to `lines`."""

    def __init__(self, stub=False):
        self.lines, self._orig, self.stub = [], {}, stub

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def traced(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            self.lines.append(name + "(" + ", ".join(f"{p}={describe(v)}" for p, v in b.arguments.items()) + ")")
            return None if self.stub else fn(*a, **k)
        return traced

    def __enter__(self):
        for n in launchers():
            self._orig[n] = getattr(L, n)
            setattr(L, n, self._wrap(n, self._orig[n]))
        return self

    def __exit__(self, *exc):
        for n, f in self._orig.items():
            setattr(L, n, f)


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def unet(precision, dev):
    net = CuboidTransformerUNet(**V1_UNET_CFG, precision=precision)
    net.load_state_dict(seeded_state_dict(net.state_dict(), 1234))
    return net.to(dev).eval()


def unet_inputs(B, dev):
    x = seeded_input("x", (B,) + tuple(V1_UNET_CFG["target_shape"]), 11).to(dev)
    cond = seeded_input("cond", (B,) + tuple(V1_UNET_CFG["input_shape"]), 12).to(dev)
    return x, torch.tensor([(37 * i + 500) % 1000 for i in range(B)], device=dev), cond


FUSE_FLAGS = ("fuse_pair", "fuse_attn", "fuse_ffn", "fuse_ffn_rows")


def stub_cases(case):
    """The host-only run: `case(name, fn)` traces fn() with every launch stubbed."""
    dev = torch.device("cpu")
    for precision in PRECISIONS:
        net = unet(precision, dev)
        for B in (2, 32):
            x, t, cond = unet_inputs(B, dev)
            case(f"unet_{precision}_B{B}", lambda: net._forward(x, t, cond))
            saved = {f: getattr(net, f) for f in FUSE_FLAGS}
            for f in FUSE_FLAGS:          # cumulative: the last case has all four off
                setattr(net, f, False)
                case(f"unet_{precision}_B{B}_no_{f}", lambda: net._forward(x, t, cond))
            for f, v in saved.items():
                setattr(net, f, v)
    for precision in ("bf16", "fp32", "fp16"):
        vae = AutoencoderKL(**V1_VAE_CFG, precision=precision)

        def cpu_input(x, dev, vae=vae):          # AutoencoderKL._input without its device check
            N, C, H, W = x.shape
            xl = vae._buf("in.nhwc", (N * H * W, C), torch.float32, dev)
            L.nchw_to_nhwc(x.contiguous().float(), xl, N, C, H * W, C)
            return xl, N, C, (H, W)
        vae._input = cpu_input
        for fuse in (True, False):
            vae.fuse_resblock = fuse
            tag = precision + ("" if fuse else "_no_fuse_resblock")
            case(f"vae_encode_{tag}", lambda: vae._encode(torch.zeros(2, 1, 128, 128)))
            case(f"vae_decode_{tag}", lambda: vae._decode_impl(torch.zeros(2, V1_VAE_CFG["latent_channels"], 16, 16)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--stub", action="store_true", help="host side only: launches are recorded, not made (no device needed; traces, no hashes)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.stub:
        total = 0

        def case(name, fn):
            nonlocal total
            with Tracer(stub=True) as tr:
                fn()
            with open(os.path.join(args.out, name + ".trace"), "w") as f:
                f.write("\n".join(tr.lines) + "\n")
            total += len(tr.lines)
            print(f"{name} launches={len(tr.lines)}", flush=True)
        stub_cases(case)
        print(f"stub run: {total} launch lines")
        return
    dev = torch.device("cuda", 0)
    hashes = []

    def case(name, fn):
        with Tracer() as tr:
            out = fn()
        torch.cuda.synchronize(dev)
        with open(os.path.join(args.out, name + ".trace"), "w") as f:
            f.write("\n".join(tr.lines) + "\n")
        hashes.append(f"{name} {sha(out)} launches={len(tr.lines)}")
        print(hashes[-1], flush=True)

    for precision in PRECISIONS:
        net = unet(precision, dev)
        for B in (2, 32):
            x, t, cond = unet_inputs(B, dev)
            case(f"unet_{precision}_B{B}", lambda: net(x, t, cond))
        del net
        torch.cuda.empty_cache()
    for precision in ("bf16", "fp32"):
        vae = AutoencoderKL(**V1_VAE_CFG, precision=precision)
        vae.load_state_dict(seeded_state_dict(vae.state_dict(), 4321))
        vae = vae.to(dev).eval()
        frames = seeded_input("frames", (2, 1, 128, 128), 13).to(dev)
        z = seeded_input("z", (2, V1_VAE_CFG["latent_channels"], 16, 16), 14).to(dev)
        case(f"vae_encode_{precision}", lambda: vae.encode(frames).parameters)
        case(f"vae_decode_{precision}", lambda: vae.decode(z))
        del vae
        torch.cuda.empty_cache()

    ldm = LatentDiffusion(torch_nn_module=unet("bf16", dev), first_stage_model=None, cond_stage_model=None, **V1_LDM_KW).to(dev).eval()
    B = 4
    cond = seeded_input("cond", (B,) + tuple(V1_UNET_CFG["input_shape"]), 15).to(dev)
    x_T = seeded_input("x_T", ldm.get_batch_latent_shape(B), 16).to(dev)
    out = ldm.ddim_sample_loop(cond, tuple(x_T.shape), ddim_steps=5, eta=0.0, x_T=x_T)
    torch.cuda.synchronize(dev)
    hashes.append(f"ddim5_bf16_B{B} {sha(out)}")
    print(hashes[-1], flush=True)
    with open(os.path.join(args.out, "hashes.txt"), "w") as f:
        f.write("\n".join(hashes) + "\n")


if __name__ == "__main__":
    main()
