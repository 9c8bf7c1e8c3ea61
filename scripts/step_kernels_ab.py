"""Time the ten sampler-step entry points of two builds of the library in one process (run on the GPU box):
    python scripts/step_kernels_ab.py PARENT.so [NEW.so] > profiles/step_kernels_ab.txt
At the workload's shape, B = 64 trajectories x 98304 latent elements, with every optional operand present.  Three arms, interleaved
block by block: the parent, the new build, and the parent again (the run-to-run spread).  A block is BLOCK back-to-back launches between
two device events; every arm gets BLOCKS of them after a warm-up, and the figure is the median block time per launch."""
import ctypes as C
import hashlib
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, PER, BLOCK, BLOCKS = 64, 98304, 20, 50
# entry point -> its pointer operands in order (c<width>: coefficient rows)
FORMS = {"ddim_step": "zt eps noise c3 out", "ddim_step_guided": "zt eps noise shift c4 out",
         "ddim_step_held": "zt eps noise shift x0 mask hnoise c6 out", "dpmpp_2m_step": "zt eps hist c4 out",
         "dpmpp_2m_step_guided": "zt eps hist shift c5 out", "dpmpp_2m_step_held": "zt eps hist shift x0 mask hnoise c7 out",
         "dpmpp_2m_sde_step": "zt eps noise hist c5 out", "dpmpp_2m_sde_step_guided": "zt eps noise hist shift c6 out",
         "dpmpp_2m_sde_step_held": "zt eps noise hist shift x0 mask hnoise c8 out", "hold_blend": "zt x0 mask hnoise c2 out"}


def main():
    parent = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "prediff_amd", "libprediff_hip.so")
    again = os.path.join(tempfile.mkdtemp(), "parent_again.so")      # a copy under another path: loaded a second time, its own code object
    shutil.copy(parent, again)
    arms = {"parent": C.CDLL(parent), "new": C.CDLL(new), "parent again": C.CDLL(again)}
    g = torch.Generator().manual_seed(5)
    t = {k: torch.randn(B, PER, generator=g).cuda() for k in "zt eps noise hist shift x0 hnoise out".split()}
    t["mask"] = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (B, PER), generator=g)].cuda()
    for w in range(2, 9):                                  # every column 0.5: a_t in (0, 1), w, c_n and k_n not zero
        t[f"c{w}"] = torch.full((B, w), 0.5).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def block(lib, fn, n):
        ops = [C.c_void_p(t[k].data_ptr()) for k in FORMS[fn].split()]
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            assert getattr(lib, "pd_" + fn)(*ops, C.c_int(B), C.c_int64(PER), stream) == 0, fn
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / n

    print(f"# step kernels, B = {B}, per_sample = {PER}: median us per launch over {BLOCKS} blocks of {BLOCK} launches per arm, arms interleaved")
    for name, path in (("parent", parent), ("new", new)):
        with open(path, "rb") as f:
            print(f"# {name:6s} library sha256 {hashlib.sha256(f.read()).hexdigest()}")
    print(f"# {'entry point':28s} {'parent':>9s} {'new':>9s} {'parent again':>13s} {'new/parent':>11s} {'again/parent':>13s}")
    rows = []
    for fn in FORMS:
        times = {a: [] for a in arms}
        for a, lib in arms.items():
            block(lib, fn, BLOCK)
        for _ in range(BLOCKS):
            for a, lib in arms.items():
                times[a].append(block(lib, fn, BLOCK))
        p, n, p2 = (statistics.median(times[a]) for a in arms)
        rows.append((fn, n / p - 1, p2 / p - 1))
        print(f"{fn:30s} {p:9.2f} {n:9.2f} {p2:13.2f} {n / p:11.4f} {p2 / p:13.4f}", flush=True)
    spread = max(abs(r[2]) for r in rows)
    print(f"# run-to-run spread (largest |parent again / parent - 1| of the ten): {spread * 100:.2f}%")
    for fn, d, _ in rows:
        print(f"# {fn:30s} new vs parent {d * 100:+.2f}%  {'within the spread' if d <= spread else 'SLOWER than the spread'}")


if __name__ == "__main__":
    main()
