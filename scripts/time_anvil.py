"""Time AutoregressiveExtrapolation (pd_anvil_analyse, pd_anvil_evolve, pd_steps_finish) on the GPU box beside
LagrangianPersistence.forecast and S-PROG (StochasticExtrapolation().forecast(ctx)) on the same contexts, in the same process.

    python scripts/time_anvil.py [log] [reps]        (default: profiles/time_anvil.log, 30 repeats)

Two workloads at the defaults (6 levels, AR(2), window 16 pixels): 1 and 8 contexts of 7 x 128 x 128 -> 6 frames (the v1 shape).  The
motion field is estimated inside every forecast (pd_lk_motion), as in LagrangianPersistence.forecast, and is timed alone too; the lines
"motion given" leave it out.  analyse is pd_anvil_analyse's two launches; "evolve - analyse" and "forecast - evolve" are differences of
medians: the pointwise ARI iteration and step 10.  After three warm-up calls (the first allocates the workspace) each repeat times one
call between two events with a device synchronise; the lines give the median, the minimum and the maximum.  Report only: nothing here is
a pass criterion, and there is no earlier version to compare a time with."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prediff_amd import AutoregressiveExtrapolation, LagrangianPersistence, StochasticExtrapolation  # noqa: E402
from prediff_amd import _lib as L  # noqa: E402

LOG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "time_anvil.log")
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
    return f"  {name:38}: median {med:9.1f} us  (min {min(ts):9.1f}, max {max(ts):9.1f}, {len(ts)} repeats){rel}"


say("# python scripts/time_anvil.py (one MI355X, gfx950); fp32 NTHWC frames; default options; report only")
say(f"device {torch.cuda.get_device_name(0)}, {REPS} repeats per line, 3 warm-up calls")
with torch.no_grad():
    T, H, W, K = 7, 128, 128, 6
    for B in (1, 8):
        lp = LagrangianPersistence(out_len=K)
        ae = AutoregressiveExtrapolation(out_len=K, motion=lp)
        se = StochasticExtrapolation(out_len=K, motion=lp)
        # smooth fields on a dry background: a box-filtered uniform field, cut so that about a third of the frame is wet
        ctx = torch.nn.functional.avg_pool2d(torch.rand((B * T, 1, H + 8, W + 8), generator=g, device=dev), 9, stride=1)
        ctx = ((ctx - ctx.mean()) * 8 + 0.05).clamp_(0, 1).view(B, T, H, W, 1).contiguous()
        mot = lp.motion(ctx)
        ws = L.anvil_ws_bytes(B, H, W, ae.levels, ae.ar_order)
        say(f"{B} contexts of {T} x {H} x {W} -> {K} frames; wet share of the last frame "
            f"{float((ctx[:, -1] > ae.threshold).float().mean()):.2f}; window radius {ae._g.numel() // 2}; workspace {ws / 2 ** 20:.1f} MiB; "
            f"launches: spectra 1 ({2 * B} workgroups), cascade 1 ({ae.levels * B}), evolve 1 ({B * H * W // 1024}), finish 1 ({B * K})")
        ref = statistics.median(timed(lambda: lp.forecast(ctx)))
        say(line("LagrangianPersistence.forecast", timed(lambda: lp.forecast(ctx))))
        say(line("LagrangianPersistence.motion", timed(lambda: lp.motion(ctx))))
        t_an = timed(lambda: ae.analyse(ctx, mot))
        t_ev = timed(lambda: ae.evolve(ctx, mot))
        t_fc = timed(lambda: ae.forecast(ctx, mot))
        say(line("analyse (motion given)", t_an, ref))
        say(line("evolve (motion given; analyse in it)", t_ev, ref))
        say(line("forecast, motion given", t_fc, ref))
        say(f"  {'evolve - analyse, forecast - evolve':38}: {statistics.median(t_ev) - statistics.median(t_an):9.1f} us, "
            f"{statistics.median(t_fc) - statistics.median(t_ev):9.1f} us (differences of medians)")
        say(line("forecast", timed(lambda: ae.forecast(ctx)), ref))
        say(line("S-PROG: StochasticExtrapolation.forecast", timed(lambda: se.forecast(ctx)), ref))
        f = ae.forecast(ctx)
        assert f.shape == (B, K, H, W, 1) and bool(torch.isfinite(f).all())
out.close()
