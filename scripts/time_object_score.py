"""Time SEVIRObjectScore.update_members (pd_sal_update: the labelling kernel over the target's and the members' frames plus the pair
kernel) on the GPU box, next to SEVIRFrameScore.update_members on the same tensors in the same run.

    python scripts/time_object_score.py [reps]

The v1 shape: M = 32 members (32, 1, 6, 128, 128, 1) of one context against its target.  Three sets of frames: storm-like (a few smooth
cells per frame: few objects, long rows of one object per wave), Bernoulli masks at density 0.45 under 4-connectivity (about 1500
winding components per frame, close to percolation: the most passes), and the checkerboard under 4-connectivity (8192 objects per frame:
16 batches of object slots).  Each line: the mean per call over `reps` back-to-back calls between two events (GPU time, launch gaps
included) and the best single call.  The time to produce the 32 samples is scripts/time_sample.py's.  Report only: no test asserts a
time."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd.frame_score import SEVIRFrameScore  # noqa: E402
from prediff_amd.object_score import SEVIRObjectScore, label_objects  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
M, T, H, W = 32, 6, 128, 128


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


def storms(n):
    """n frames (n, H, W): 2 .. 6 Gaussian cells of width 3 .. 10 pixels each, on a weak noise floor below max / 15"""
    r = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    c = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    out = 0.02 * torch.rand((n, H, W), generator=g, device=dev)
    for k in range(6):
        on = (torch.rand((n, 1, 1), generator=g, device=dev) < (1.0 if k < 2 else 0.5)).float()
        cy, cx = (20 + 88 * torch.rand((n, 1, 1), generator=g, device=dev) for _ in range(2))
        s = 3 + 7 * torch.rand((n, 1, 1), generator=g, device=dev)
        amp = 0.4 + 0.6 * torch.rand((n, 1, 1), generator=g, device=dev)
        out += on * amp * torch.exp(-((r - cy) ** 2 + (c - cx) ** 2) / (2 * s * s))
    return out


def case(label, frames, connectivity):
    """frames ((M + 1) T, H, W): the first M T are the members', the last T the target's"""
    ens = frames[:M * T].view(M, 1, T, H, W, 1)
    tgt = frames[M * T:].view(1, T, H, W, 1)
    _, n, _ = label_objects(tgt, connectivity=connectivity, max_objects=1)
    obj = SEVIRObjectScore(mode="1", seq_len=T, connectivity=connectivity)
    mean, best = timed(lambda: obj.update_members(ens, tgt))
    print(f"{label:34} objects/frame {float(n.float().mean()):7.1f}  object_score update_members M=32: {mean * 1e3:8.1f} us/call "
          f"(best single {best * 1e3:8.1f} us)")
    fs = SEVIRFrameScore(mode="1", seq_len=T, data_range=1.0)
    mean, best = timed(lambda: fs.update_members(ens, tgt))
    print(f"{'':34} {'':21}  frame_score  update_members M=32: {mean * 1e3:8.1f} us/call (best single {best * 1e3:8.1f} us)")
    obj.reset()
    obj.update_members(ens, tgt)
    r = obj.compute()
    print(f"{'':34} S {r['S'].mean():+.4f}  A {r['A'].mean():+.4f}  L {r['L'].mean():.4f}  objects pred / target "
          f"{r['n_obj_pred'].mean():.1f} / {r['n_obj_target'].mean():.1f}")


print(f"device {torch.cuda.get_device_name(0)}, {REPS} back-to-back calls per line; {(M + 1) * T} frames of {H} x {W} per call")
case("storm-like cells, 8-connectivity", storms((M + 1) * T), 8)
bern = (torch.rand(((M + 1) * T, H, W), generator=g, device=dev) < 0.45).float() * (0.2 + 0.8 * torch.rand(((M + 1) * T, H, W), generator=g, device=dev))
case("Bernoulli 0.45, 4-connectivity", bern, 4)
rr, cc = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
board = (((rr + cc) % 2 == 0).float() * 0.5).expand((M + 1) * T, H, W).contiguous()
case("checkerboard, 4-connectivity", board, 4)
