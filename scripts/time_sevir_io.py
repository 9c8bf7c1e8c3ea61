"""The SEVIR pixel front end against the torch op chain it replaces, one process (run on the GPU box):
  0. scripts/bench_store.py in a child process, before this process opens the GPU: the plain-copy rate of this run, the yardstick of
     the byte rates below;
  A. pd_sevir_ingest, 64 events (384, 384, 49) uint8, factors (2, 3, 3), one window of 7 + 6 frames at LR frame 12, against
     raw[..., ::2] -> reshape -> amax over the 3 x 3 blocks -> float -> scale * (x + offset) -> permute -> the two window slices made
     contiguous;
  B. pd_sevir_export, 64 x 6 frames (128 x 128), to uint8 NTHW and to uint8 NHWT, against x / scale - offset -> clamp -> round -> uint8
     (-> permute -> contiguous); the chain divides by a device scalar TENSOR: torch's division by a Python scalar on the device is a
     multiplication by the reciprocal, which is not the reference's (CPU) arithmetic;
  C. what one ensemble forecast needs: ingest of ONE event, export of 32 x 6 frames to uint8 NTHW.
Device events around LAUNCHES back-to-back calls, the two arms interleaved REPS times after untimed calls; the outputs of the two arms
are compared bit for bit.  Usage: time_sevir_io.py [REPS] [LOG]; the lines are printed and written to LOG (default
profiles/time_sevir_io.log)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
store = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_store.py")], capture_output=True, text=True, check=True).stdout
import numpy as np, torch
from prediff_amd import SEVIRFrontEnd

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LOG = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_sevir_io.log")
LAUNCHES = 20
dev = torch.device("cuda")
log = open(LOG, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def spread(v):
    return f"min {min(v):.4f} median {sorted(v)[len(v) // 2]:.4f} max {max(v):.4f}"


def event_ms(fn):
    """ms per call over LAUNCHES back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / LAUNCHES


def compare(label, arms, moved, same):
    """arms: {"kernel": fn, "torch": fn}; moved: the bytes the kernel reads and writes; same(a, b): the two results agree bit for bit"""
    for fn in arms.values():                 # untimed: code objects, the start table's upload, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    assert same(arms["kernel"](), arms["torch"]()), label
    ms = {k: [] for k in arms}
    for rep in range(REPS):
        for name, fn in arms.items():
            ms[name].append(event_ms(fn))
    for name, v in ms.items():
        say(f"{label} {name}: ms / call {spread(v)}")
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    say(f"{label} medians: kernel {med['kernel']:.4f} ms ({moved / 1e6:.1f} MB read + written: {moved / med['kernel'] / 1e9:.3f} TB/s), torch chain "
        f"{med['torch']:.4f} ms (ratio torch / kernel {med['torch'] / med['kernel']:.2f}); outputs of the two arms agree bit for bit")
    return med["kernel"]


def ingest_arms(label, N):
    fe = SEVIRFrontEnd()                                                       # 7 + 6 frames, factors (2, 3, 3), rescale "01"
    raw = torch.randint(0, 256, (N, 384, 384, 49), dtype=torch.uint8, device=dev)
    start = 12
    scale, offset = float(np.float32(fe.scale)), float(np.float32(fe.offset))

    def chain():
        x = raw[..., ::2].reshape(N, 128, 3, 128, 3, 25).amax(dim=(2, 4))      # (N, H', W', T') bytes
        x = (scale * (x.float() + offset)).permute(0, 3, 1, 2).unsqueeze(-1)   # NTHWC
        return x[:, start:start + 7].contiguous(), x[:, start + 7:start + 13].contiguous()
    arms = {"kernel": lambda: fe.ingest(raw, starts=(start,)), "torch": chain}
    moved = raw.numel() + N * 13 * 128 * 128 * 4
    t = compare(label, arms, moved, lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    del raw
    torch.cuda.empty_cache()
    return t


def export_arms(label, B, layout):
    fe = SEVIRFrontEnd()
    x = torch.rand(B, 6, 128, 128, 1, device=dev) * 1.2 - 0.1
    scale_t, offset = torch.tensor(fe.scale, dtype=torch.float32, device=dev), float(np.float32(fe.offset))

    def chain():
        v = (x / scale_t - offset).clamp(0, 255).round().to(torch.uint8)[..., 0]
        return v if layout == "NTHW" else v.permute(0, 2, 3, 1).contiguous()
    arms = {"kernel": lambda: fe.export(x, layout=layout), "torch": chain}
    return compare(label, arms, x.numel() * 5, torch.equal)


with torch.no_grad():
    say(f"{torch.cuda.get_device_name(0)}; command: python scripts/time_sevir_io.py {REPS}")
    for line in store.strip().splitlines():
        say("0 bench_store.py: " + line)
    ingest_arms("A ingest 64 events", 64)
    export_arms("B export 64 x 6 frames -> uint8 NTHW", 64, "NTHW")
    export_arms("B export 64 x 6 frames -> uint8 NHWT", 64, "NHWT")
    t_in = ingest_arms("C ingest 1 event", 1)
    t_out = export_arms("C export 32 x 6 frames -> uint8 NTHW", 32, "NTHW")
    say(f"C one ensemble of 32: ingest of the event + export of the 32 forecasts = {t_in + t_out:.4f} ms")
log.close()
