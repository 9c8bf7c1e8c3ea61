"""Time FrechetVideoDistance.update (preprocess + I3D features + moments) on the GPU box, per precision, and split it by kernel.

    python scripts/time_fvd.py [reps]            writes profiles/time_fvd.log and profiles/time_fvd_kernel_stats.csv

Input: single-channel 128 x 128 x 12-frame videos in NTHWC (what the decoder hands to test_step), 16 and 32 videos per update, seeded I3D
weights.  Every GPU step is a child process under its own `timeout`, and the driver stops at the first step that does not end cleanly:
one step per precision ("fp32", "fp16", "bf16": videos/s, the mean over `reps` back-to-back updates between two events), then one
`rocprofv3 --kernel-trace --stats` run of three fp32 updates of 32 videos for the per-kernel split (a counter-free trace, in a run of its
own).  The cost of scoring 32 samples is printed next to the cost of producing them (README: 28.7 samples/s end to end).  Report only."""
import csv
import glob
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SAMPLES_PER_S = 28.7               # README: end-to-end sampling rate (DDIM-50 incl. the VAE) the scoring cost is set against
SHAPE = (12, 128, 128, 1)


def step(precision, reps, profile):
    import torch
    from prediff_amd import FrechetVideoDistance, InceptionI3d
    from prediff_amd.seeding import seeded_i3d_state_dict
    sd = seeded_i3d_state_dict(InceptionI3d(400).state_dict(), 4100)
    m = FrechetVideoDistance(feature=400, weights=sd, layout="NTHWC", precision=precision)
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in ((32,) if profile else (16, 32)):
        v = torch.rand((n,) + SHAPE, generator=g, device="cuda")
        m.update(v, real=True)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            m.update(v, real=False)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        print(f"{precision:5} {n:3d} videos/update: {ms:9.2f} ms/update  {n / ms * 1e3:8.1f} videos/s", flush=True)
        if n == 32:
            t_sample = 32 / SAMPLES_PER_S * 1e3
            print(f"{precision:5} scoring 32 samples {ms:.1f} ms against {t_sample:.0f} ms to produce them at {SAMPLES_PER_S} samples/s: "
                  f"{ms / t_sample * 100:.2f} % on top", flush=True)


def kernel_split(out_dir, log):
    f = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not f:
        log("no kernel_stats.csv under " + out_dir)
        return
    shutil.copyfile(f[0], os.path.join(ROOT, "profiles", "time_fvd_kernel_stats.csv"))
    rows = list(csv.DictReader(open(f[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    log(f"per-kernel split, fp32, 1 + 3 updates of 32 videos: total kernel time {tot / 1e6:.1f} ms over {sum(int(r['Calls']) for r in rows)} launches")
    for r in rows[:14]:
        log(f"{float(r['TotalDurationNs']) / tot * 100:6.2f} %  calls {int(r['Calls']):5d}  avg {float(r['AverageNs']) / 1e3:9.1f} us  {r['Name'][:100]}")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        step(sys.argv[2], int(sys.argv[3]), len(sys.argv) > 4 and sys.argv[4] == "--profile")
        return
    reps = sys.argv[1] if len(sys.argv) > 1 else "5"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def run(cmd, limit):
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return r.returncode, r.stdout

    ok = True
    for precision in ("fp32", "fp16", "bf16"):
        rc, out = run([sys.executable, os.path.abspath(__file__), "--step", precision, reps], 300)
        for s in out.splitlines():
            if s.startswith(precision):
                log(s)
        if rc != 0:
            log(f"step {precision} ended with status {rc}: stopping\n" + out[-2000:])
            ok = False
            break
    if ok:
        out_dir = os.path.join(ROOT, "build", "time_fvd_prof")          # (build/ is not tracked)
        rc, out = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "trace", "--",
                       sys.executable, os.path.abspath(__file__), "--step", "fp32", "3", "--profile"], 600)
        if rc == 0:
            kernel_split(out_dir, log)
        else:
            log(f"rocprofv3 step ended with status {rc}\n" + out[-2000:])
            ok = False
    with open(os.path.join(ROOT, "profiles", "time_fvd.log"), "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
