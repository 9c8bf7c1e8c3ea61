"""Time SEVIRScaleScore.update_members (pd_scale_update: the bit-plane kernel over the target's and the members' frames plus the fold) on
the GPU box, next to SEVIRDistanceScore.update_members on the same tensors in the same run.

    python scripts/time_scale_score.py [reps]

The v1 shape: M = 32 members (32, 1, 6, 128, 128, 1) of one context against its target, storm-like frames (a few smooth cells per frame on
a weak noise floor), the six default thresholds.  Each line: after a warm-up call, the median over `reps` single calls, each between two
events (GPU time of one call, its launches included), and the mean per call over `reps` back-to-back calls between two events (launch
gaps included).  Report only: no test asserts a time.  Writes profiles/time_scale_score.log."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.distance_score import SEVIRDistanceScore  # noqa: E402
from prediff_amd.scale_score import SEVIRScaleScore  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
M, T, H, W = 32, 6, 128, 128
lines = []


def say(line):
    print(line)
    lines.append(line)


def timed(fn):
    """(median of REPS single event-timed calls, mean over REPS back-to-back calls), in ms, after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    single = []
    for _ in range(REPS):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        single.append(a.elapsed_time(b))
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return statistics.median(single), a.elapsed_time(b) / REPS


def storms(n):
    """n frames (n, H, W) in [0, 1]: 2 .. 6 Gaussian cells of width 3 .. 10 pixels each, on a weak noise floor"""
    r = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    c = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    out = 0.02 * torch.rand((n, H, W), generator=g, device=dev)
    for k in range(6):
        on = (torch.rand((n, 1, 1), generator=g, device=dev) < (1.0 if k < 2 else 0.5)).float()
        cy, cx = (20 + 88 * torch.rand((n, 1, 1), generator=g, device=dev) for _ in range(2))
        s = 3 + 7 * torch.rand((n, 1, 1), generator=g, device=dev)
        amp = 0.4 + 0.6 * torch.rand((n, 1, 1), generator=g, device=dev)
        out += on * amp * torch.exp(-((r - cy) ** 2 + (c - cx) ** 2) / (2 * s * s))
    return out.clamp_(0.0, 1.0)


frames = storms((M + 1) * T)
ens = frames[:M * T].view(M, 1, T, H, W, 1)
tgt = frames[M * T:].view(1, T, H, W, 1)
say(f"device {torch.cuda.get_device_name(0)}; {(M + 1) * T} frames of {H} x {W} per call; {REPS} calls per figure")
sc = SEVIRScaleScore(mode="1", seq_len=T)
med_s, mean_s = timed(lambda: sc.update_members(ens, tgt))
say(f"scale_score    update_members M=32, 6 thresholds: median single call {med_s * 1e3:8.1f} us, back-to-back mean "
    f"{mean_s * 1e3:8.1f} us/call")
ds = SEVIRDistanceScore(mode="1", seq_len=T)
med_d, mean_d = timed(lambda: ds.update_members(ens, tgt))
say(f"distance_score update_members M=32, 6 thresholds: median single call {med_d * 1e3:8.1f} us, back-to-back mean "
    f"{mean_d * 1e3:8.1f} us/call")
say(f"ratio scale_score / distance_score, medians: {med_s / med_d:.2f}")
sc = SEVIRScaleScore(mode="2", seq_len=T)
sc.update_members(ens, tgt)
r = sc.compute()
say("mode 2 iss per component (synthetic storms, not forecasts), threshold 16: " + " ".join(f"{v:.3f}" for v in r["iss"][0])
    + "; threshold 133: " + " ".join(f"{v:.3f}" for v in r["iss"][2]))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "time_scale_score.log"), "w") as f:
    f.write("\n".join(lines) + "\n")
