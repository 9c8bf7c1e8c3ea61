"""Time SEVIRFrameScore.update / update_members (pd_frame_score_update: the tile kernel + the fixed-order final pass, plus the two
range kernels for data_range=None) on the GPU box, next to the same formula evaluated with torch ops (five conv2d) on the same device.

    python scripts/time_frame_score.py [reps]

update: pred and target (32, 6, 128, 128, 1) fp32 in NTHWC.  update_members: M = 32 members (32, 1, 6, 128, 128, 1) of one context.
Each line: the mean per call over `reps` back-to-back calls between two events (GPU time, launch gaps included) and the best single
call (events around one call).  The bytes-moved floor is pred plus target read once at the HBM rate.  Report only: no test asserts a time."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.frame_score import SEVIRFrameScore  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    mean = a.elapsed_time(b) / REPS
    best = float("inf")
    for _ in range(10):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return mean, best


def torch_scores(pred, target, data_range):
    """The torchmetrics form with torch ops: frames as (b t) c h w, reflect padding, one grouped conv2d over the five stacked inputs with
    the 11 x 11 fp32 kernel, crop, mean per frame; plus the two error sums.  pred, target: (N, T, H, W, C)."""
    p, t = (x.permute(0, 1, 4, 2, 3).flatten(0, 1) for x in (pred, target))
    C = p.shape[1]
    d = torch.arange(-5, 6, dtype=torch.float32, device=p.device)
    k1 = torch.exp(-((d / 1.5) ** 2) / 2)
    k1 = (k1 / k1.sum()).unsqueeze(0)
    kernel = (k1.t() @ k1).expand(C, 1, 11, 11)
    pp, tp = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat((pp, tp, pp * pp, tp * tp, pp * tp)), kernel, groups=C)
    mp, mt, epp, ett, ept = out.split(p.shape[0])
    vp, vt, cov = (epp - mp * mp).clamp_min(0), (ett - mt * mt).clamp_min(0), ept - mp * mt
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * mp * mt + c1) * (2 * cov + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    ssim = s[..., 5:-5, 5:-5].reshape(s.shape[0], -1).mean(-1).sum()
    diff = p - t
    return (diff * diff).sum(), diff.abs().sum(), ssim


print(f"device {torch.cuda.get_device_name(0)}, {REPS} back-to-back calls per line")
target = torch.rand((32, 6, 128, 128, 1), generator=g, device=dev)
pred = (target + 0.1 * torch.randn(target.shape, generator=g, device=dev)).clamp(0, 1)
nbytes = 2 * pred.numel() * 4
print(f"update (32, 6, 128, 128, 1): pred + target read once = {nbytes / 1e6:.1f} MB -> floor {nbytes / HBM_BYTES_PER_S * 1e6:.1f} us at "
      f"{HBM_BYTES_PER_S / 1e12:.0f} TB/s")
for dr in (1.0, None):
    m = SEVIRFrameScore(layout="NTHWC", mode="1", seq_len=6, data_range=dr)
    mean, best = timed(lambda: m.update(pred, target))
    print(f"frame_score update data_range={dr!s:4}: {mean * 1e3:8.1f} us/update (best single {best * 1e3:8.1f} us)")
mean, best = timed(lambda: torch_scores(pred, target, 1.0))
print(f"torch ops (pad, 5-stack conv2d, crop)  : {mean * 1e3:8.1f} us/update (best single {best * 1e3:8.1f} us)")
m = SEVIRFrameScore(layout="NTHWC", mode="1", seq_len=6, data_range=1.0)
m.update(pred, target)
ref = torch_scores(pred, target, 1.0)
print(f"  ssim sum over the frames: kernel {float(m.sums[2].sum()):.9f}, torch ops (fp32) {float(ref[2]):.9f}")

tgt1 = target[:1]
ens = (tgt1.unsqueeze(0) + 0.1 * torch.randn((32,) + tuple(tgt1.shape), generator=g, device=dev)).clamp(0, 1)
nbytes = (ens.numel() + tgt1.numel()) * 4
print(f"update_members M=32 of (1, 6, 128, 128, 1): members + target read once = {nbytes / 1e6:.1f} MB -> floor "
      f"{nbytes / HBM_BYTES_PER_S * 1e6:.1f} us")
m = SEVIRFrameScore(layout="NTHWC", mode="1", seq_len=6, data_range=1.0)
mean, best = timed(lambda: m.update_members(ens, tgt1))
print(f"frame_score update_members M=32        : {mean * 1e3:8.1f} us/call   (best single {best * 1e3:8.1f} us)")


def sequential():
    for i in range(32):
        m.update(ens[i], tgt1)


mean, best = timed(sequential)
print(f"frame_score 32 sequential update calls : {mean * 1e3:8.1f} us/32 calls (best single {best * 1e3:8.1f} us)")
mean, best = timed(lambda: torch_scores(ens[:, 0], tgt1.expand(32, -1, -1, -1, -1), 1.0))
print(f"torch ops on the 32 members            : {mean * 1e3:8.1f} us/call   (best single {best * 1e3:8.1f} us)")
