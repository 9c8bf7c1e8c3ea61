"""Time SEVIRSpectralScore (pd_spectrum_update: the batched 2-D FFT with the fused radial reduce, plus the fixed-order fold) on the GPU
box, interleaved in one process with a yardstick: the same three sums per lead time computed with torch.fft.fft2 and index_add_ on the
same device.

    python scripts/time_spectrum.py [log] [reps]        (default: profiles/time_spectrum.log, 30 repeats)

Two workloads: update_members with M = 32 members of (1, 6, 128, 128, 1) fp32 frames (one context's ensemble: the LDS-resident form), and
update on (7, 6, 256, 256, 1) (the tiled canvas: the strip form).  After a warm-up of both sides, each repeat times one call of the
scorer and one call of the yardstick, alternating, each between two events with a device synchronise; the lines give the median, the
minimum and the maximum over the repeats.  Report only: no test asserts a time."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.spectrum import SEVIRSpectralScore, spectrum_bins  # noqa: E402

LOG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "time_spectrum.log")
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
SAMPLE_S = 1.07                   # README: a 12-frame rollout of 32 members takes 2.14 s end to end, two 6-frame segments: 1.07 s each
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
out = open(LOG, "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def interleaved(f, y):
    for _ in range(3):
        f(), y()
    torch.cuda.synchronize()
    tf, ty = [], []
    for _ in range(REPS):
        tf.append(once(f))
        ty.append(once(y))
    return tf, ty


def line(name, ts):
    return f"{name:46}: median {statistics.median(ts):9.1f} us  (min {min(ts):9.1f}, max {max(ts):9.1f}, {len(ts)} repeats)"


def yardstick(H, W):
    """ens (M, N, T, H, W, 1), target (N, T, H, W, 1) -> (3, T, nb) fp64 sums, with torch ops on the device"""
    bins, _, _, cells = spectrum_bins(H, W)
    nb = cells.shape[0]
    flat = torch.from_numpy(bins.reshape(-1)).to(dev)
    keep = torch.nonzero(flat < nb).squeeze(1)
    idx = flat[keep]
    s = 1.0 / (H * W)

    def run(ens, target):
        P, T = torch.fft.fft2(ens[..., 0]), torch.fft.fft2(target[..., 0]).unsqueeze(0)
        q = torch.stack([s * (P.real ** 2 + P.imag ** 2), (s * (T.real ** 2 + T.imag ** 2)).expand_as(P.real),
                         s * (P.real * T.real + P.imag * T.imag)])               # (3, M, N, T, H, W)
        q = q.sum(dim=(1, 2)).flatten(2).double()                               # (3, T, H W): linear, so members and n fold first
        return torch.zeros(q.shape[:2] + (nb,), dtype=torch.float64, device=dev).index_add_(2, idx, q[..., keep])

    return run


say(f"# python scripts/time_spectrum.py (one MI355X, gfx950); fp32 NTHWC frames; scorer and yardstick alternate in one process; report only")
say(f"device {torch.cuda.get_device_name(0)}, {REPS} repeats per line, 3 warm-up calls of each side")
for label, ens_shape in (("update_members M=32 of (1, 6, 128, 128, 1)", (32, 1, 6, 128, 128, 1)),
                         ("update of (7, 6, 256, 256, 1)", (1, 7, 6, 256, 256, 1))):
    M, N, T, H, W, _ = ens_shape
    target = torch.rand(ens_shape[1:], generator=g, device=dev)
    ens = (target.unsqueeze(0) + 0.1 * torch.randn(ens_shape, generator=g, device=dev)).clamp(0, 1)
    m = SEVIRSpectralScore(layout="NTHWC", mode="1", seq_len=T)
    f = (lambda: m.update_members(ens, target)) if M > 1 else (lambda: m.update(ens[0], target))
    ys = yardstick(H, W)
    tf, ty = interleaved(f, lambda: ys(ens, target))
    say(f"{label}: {M * N * T} pairs")
    say(line("  SEVIRSpectralScore (pd_spectrum_update)", tf))
    say(line("  torch.fft.fft2 + index_add_ (same device)", ty))
    m.reset()
    f()
    got, ref = m.sums, ys(ens, target)
    rel = float((got - ref).abs().sum() / ref.abs().sum())
    say(f"  the two agree to {rel:.1e} normwise (fp32 transforms on both sides)")
    say(f"  beside producing samples: 32 members of 6 frames end to end about {SAMPLE_S:.2f} s (README: 2.14 s for 12) -> the scorer's median is "
        f"{statistics.median(tf) / (SAMPLE_S * 1e6) * 100:.3f} % of that")
out.close()
