"""Time one SEVIREnsembleScore.update (pd_ensemble_score_update + its fixed-order final pass) and one pooled SEVIRSkillScore.update
(pd_sevir_skill_counts_pooled) on the GPU box.

    python scripts/time_ensemble_score.py [reps]

Frames of one context at SEVIR-LR size, 1 x 6 x 128 x 128 x 1, members (M, 1, 6, 128, 128, 1) fp32 in NTHWC; M in {64, 512},
pool in {1, 4, 16}.  Each line: the mean per update over `reps` back-to-back updates between two events (GPU time, launch gaps
included) and the best single update (events around one call)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.ensemble_score import SEVIREnsembleScore  # noqa: E402
from prediff_amd.sevir_skill import SEVIRSkillScore  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
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


print(f"device {torch.cuda.get_device_name(0)}, {REPS} back-to-back updates per line")
target = torch.rand((1, 6, 128, 128, 1), generator=g, device=dev)
for M in (64, 512):
    ens = (target.unsqueeze(0) + 0.1 * torch.randn((M, 1, 6, 128, 128, 1), generator=g, device=dev)).clamp(0, 1)
    for pool in (1, 4, 16):
        pre = "sevir" if pool == 1 else f"sevir_pool{pool}"
        m = SEVIREnsembleScore(layout="NTHWC", mode="1", seq_len=6, preprocess_type=pre)
        mean, best = timed(lambda: m.update(ens, target))
        mb = ens.numel() * 4 / 2 ** 20
        print(f"ensemble_score M={M:3d} pool={pool:2d}: {mean * 1e3:8.1f} us/update (best single {best * 1e3:8.1f} us), "
              f"members {mb:.1f} MiB -> {ens.numel() * 4 / (mean * 1e-3) / 1e9:.0f} GB/s")
    del ens
for N in (1, 32):
    pred = torch.rand((N, 6, 128, 128, 1), generator=g, device=dev)
    tgt = torch.rand((N, 6, 128, 128, 1), generator=g, device=dev)
    for pool in (1, 4, 16):
        pre = "sevir" if pool == 1 else f"sevir_pool{pool}"
        m = SEVIRSkillScore(layout="NTHWC", mode="1", seq_len=6, preprocess_type=pre)
        mean, best = timed(lambda: m.update(pred, tgt))
        print(f"skill_counts  N={N:2d} pool={pool:2d}: {mean * 1e3:8.1f} us/update (best single {best * 1e3:8.1f} us)")
