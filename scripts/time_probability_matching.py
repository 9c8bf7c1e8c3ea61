"""Time rank_frames, match_cdf and probability_matched_mean (csrc/probmatch.hip) on the GPU box, next to the same three results composed
from torch.sort / scatter_ on the same device in the same process.

    python scripts/time_probability_matching.py [reps] [log path]

The v1 shape: 32 members x 1 and x 8 contexts x 6 leads of 128 x 128, storm-like frames (a few smooth cells over exact zeros: most of a
frame is ties).  match_cdf is the STEPS composition: every member frame against the one last observation of its context, threshold 16/255.
Each line: the median over `reps` single calls, each between two events, after a warm-up (GPU time of one call, launch gaps included), and
whether the two results are the same bits.  Report only: no test asserts a time, and the torch composition is the yardstick the log is
read against, not a bar.  Writes profiles/time_probability_matching.log unless told another path."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd import match_cdf, probability_matched_mean, rank_frames  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
LOG = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_probability_matching.log")
THR = 16 / 255
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
M, T, H, W = 32, 6, 128, 128
n = H * W
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(REPS):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts) * 1e3


def storms(k):
    """k frames (k, H, W): 2 .. 6 Gaussian cells of width 3 .. 10 pixels on a weak noise floor, values below 0.03 set to exact zero"""
    r = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    c = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    out = 0.04 * torch.rand((k, H, W), generator=g, device=dev)
    for i in range(6):
        on = (torch.rand((k, 1, 1), generator=g, device=dev) < (1.0 if i < 2 else 0.5)).float()
        cy, cx = (20 + 88 * torch.rand((k, 1, 1), generator=g, device=dev) for _ in range(2))
        s = 3 + 7 * torch.rand((k, 1, 1), generator=g, device=dev)
        amp = 0.4 + 0.6 * torch.rand((k, 1, 1), generator=g, device=dev)
        out += on * amp * torch.exp(-((r - cy) ** 2 + (c - cx) ** 2) / (2 * s * s))
    return torch.where(out < 0.03, torch.zeros_like(out), out)


# ---- the same three results from torch.sort / scatter_
def torch_rank(x):
    s, o = torch.sort(x.reshape(x.shape[:-3] + (n,)), dim=-1, stable=True)
    return s, o.to(torch.int32)


def torch_match(x, ref, thr):
    xf = x.reshape(x.shape[:-3] + (n,))
    order = torch.sort(xf, dim=-1, stable=True).indices
    s = torch.sort(ref.reshape(ref.shape[:-3] + (n,)), dim=-1).values.expand_as(xf)
    dry = n - (xf > thr).sum(-1, keepdim=True)
    s = torch.where((torch.arange(n, device=dev) < dry) & (s > thr), torch.full_like(s, thr), s)
    return torch.empty_like(xf).scatter_(-1, order, s).view(x.shape)


def torch_pmm(ens):
    Mm, B, Tt = ens.shape[:3]
    mean = (ens.double().sum(0) / Mm).float().reshape(B, Tt, n)
    order = torch.sort(mean, dim=-1, stable=True).indices
    P = torch.sort(ens.reshape(Mm, B, Tt, n).permute(1, 2, 0, 3).reshape(B, Tt, Mm * n), dim=-1).values
    return torch.empty_like(mean).scatter_(-1, order, P[..., Mm // 2::Mm]).view(B, Tt, H, W, 1)


def case(B):
    ens = storms(M * B * T).view(M, B, T, H, W, 1)
    last = storms(B).view(B, 1, H, W, 1)
    say(f"--- {M} members x {B} context(s) x {T} leads of {H} x {W}: {M * B * T} frames")
    for name, ours, theirs in (
            ("rank_frames", lambda: rank_frames(ens), lambda: torch_rank(ens)),
            ("match_cdf (thr 16/255, ref B x 1)", lambda: match_cdf(ens, last, threshold=THR), lambda: torch_match(ens, last, THR)),
            ("probability_matched_mean", lambda: probability_matched_mean(ens), lambda: torch_pmm(ens))):
        a, b = ours(), theirs()
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        equal = all(torch.equal(u, v) for u, v in zip(a, b))
        t_ours, t_torch = timed(ours), timed(theirs)
        say(f"{name:36} HIP {t_ours:9.1f} us/call   torch.sort composition {t_torch:9.1f} us/call   same bits: {equal}")


say(f"device {torch.cuda.get_device_name(0)}; median of {REPS} event-timed calls after 3 warm-up calls; report only")
case(1)
case(8)
with open(LOG, "w") as f:
    f.write("\n".join(lines) + "\n")
