"""Time StochasticExtrapolation (pd_steps_analyse, pd_steps_evolve, pd_steps_finish) on the GPU box beside LagrangianPersistence.forecast
on the same contexts, in the same process.

    python scripts/time_steps.py [log] [reps]        (default: profiles/time_steps.log, 30 repeats)

Two workloads at the defaults (6 levels, AR(2), mask "obs", match "mean"): 32 members of 1 and of 8 contexts of 7 x 128 x 128 -> 6
frames (the v1 shape).  The noise is drawn once, outside the timed calls (``forecast(noise=...)``); ``members=32`` adds one torch.randn
and is timed beside it.  The motion field is estimated inside every forecast (pd_lk_motion), as in LagrangianPersistence.forecast, and
is timed alone too.  After three warm-up calls (the first allocates the workspace) each repeat times one call between two events with
a device synchronise; the lines give the median, the minimum and the maximum.  Report only: nothing here is a pass criterion, and there
is no earlier version to compare a time with."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd import LagrangianPersistence, StochasticExtrapolation  # noqa: E402
from prediff_amd import _lib as L  # noqa: E402

LOG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "time_steps.log")
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
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


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return [once(fn) for _ in range(REPS)]


def line(name, ts, ref=None):
    med = statistics.median(ts)
    rel = "" if ref is None else f"  |  {med / ref:6.1f} x LagrangianPersistence.forecast"
    return f"  {name:34}: median {med:9.1f} us  (min {min(ts):9.1f}, max {max(ts):9.1f}, {len(ts)} repeats){rel}"


say("# python scripts/time_steps.py (one MI355X, gfx950); fp32 NTHWC frames; default options; report only")
say(f"device {torch.cuda.get_device_name(0)}, {REPS} repeats per line, 3 warm-up calls")
with torch.no_grad():
    M, T, H, W, K = 32, 7, 128, 128, 6
    for B in (1, 8):
        lp = LagrangianPersistence(out_len=K)
        se = StochasticExtrapolation(out_len=K, motion=lp)
        # smooth fields on a dry background: a box-filtered uniform field, cut so that about a third of the frame is wet
        ctx = torch.nn.functional.avg_pool2d(torch.rand((B * T, 1, H + 8, W + 8), generator=g, device=dev), 9, stride=1)
        ctx = ((ctx - ctx.mean()) * 8 + 0.05).clamp_(0, 1).view(B, T, H, W, 1).contiguous()
        noise = torch.randn((M, B, K, H, W), generator=g, device=dev)
        mot = lp.motion(ctx)
        ws = L.steps_ws_bytes(B, M, H, W, se.levels, se.ar_order)
        say(f"{M} members x {B} contexts of {T} x {H} x {W} -> {K} frames; wet share of the last frame "
            f"{float((ctx[:, -1] > se.threshold).float().mean()):.2f}; workspace {ws / 2 ** 20:.1f} MiB; launches: analyse 1 ({B} workgroups), "
            f"evolve 1 ({M * B}), finish 1 ({M * B * K})")
        ref = statistics.median(timed(lambda: lp.forecast(ctx)))
        say(line("LagrangianPersistence.forecast", timed(lambda: lp.forecast(ctx))))
        say(line("LagrangianPersistence.motion", timed(lambda: lp.motion(ctx))))
        say(line("analyse (motion given)", timed(lambda: se.analyse(ctx, mot)), ref))
        say(line("evolve (motion given; analyse in it)", timed(lambda: se.evolve(ctx, noise, mot)), ref))
        say(line("forecast(noise), motion given", timed(lambda: se.forecast(ctx, noise=noise, motion=mot)), ref))
        say(line("forecast(noise)", timed(lambda: se.forecast(ctx, noise=noise)), ref))
        say(line("forecast(members=32)", timed(lambda: se.forecast(ctx, members=M, generator=g)), ref))
        say(line("forecast() = S-PROG, one member", timed(lambda: se.forecast(ctx)), ref))
        f = se.forecast(ctx, noise=noise)
        assert f.shape == (M, B, K, H, W, 1) and bool(torch.isfinite(f).all())
out.close()
