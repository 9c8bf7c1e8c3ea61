"""Record the parity figures of every GPU parity case of tests/test_spectrum.py: the kernel's normwise and per-bin deviation from the fp64
restatement beside those of torch.fft.fft2 in fp32 on the CPU, and the bound beta = 16 * 2^-24 * log2(H W).

    python scripts/spectrum_parity.py [log]        (default: profiles/spectrum_parity.log)

Runs the GPU tests of that file once; each parity case appends its line to the log through SPECTRUM_PARITY_LOG."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
log = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "spectrum_parity.log")
with open(log, "w") as f:
    f.write("# python scripts/spectrum_parity.py (one MI355X, gfx950): the three radial sums of every parity case of tests/test_spectrum.py\n"
            "# normwise: max over (sum, lead time) of sum_b |S - S_ref| / sum_b |S_ref|; per-bin: max of |S_b - S_ref,b| / (|S_ref,b| + "
            "mean_b |S_ref|); both must stay <= beta\n")
env = dict(os.environ, SPECTRUM_PARITY_LOG=log)
rc = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_spectrum.py"), "-m", "gpu", "-q", "-s",
                     "--durations=5"], cwd=ROOT, env=env).returncode
sys.exit(rc)
