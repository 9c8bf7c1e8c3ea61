"""Record the SSIM parity figures of every GPU case of tests/test_frame_score.py: e32 (the formula in fp32 torch ops on the CPU against the
fp64 restatement) and the kernel's deviation from the restatement, per lead time.

    python scripts/frame_score_parity.py [log]        (default: profiles/frame_score_parity.log)

Runs the GPU tests of that file once; each case appends its line to the log through FRAME_SCORE_PARITY_LOG."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
log = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frame_score_parity.log")
with open(log, "w") as f:
    f.write("# python scripts/frame_score_parity.py (one MI355X, gfx950): SSIM per lead time of every GPU case of tests/test_frame_score.py\n"
            "# e32: |fp32 torch ops on the CPU - fp64 restatement|; kernel deviation: |pd_frame_score_update - fp64 restatement|; "
            "bound: max(4 e32, 1e-6)\n")
env = dict(os.environ, FRAME_SCORE_PARITY_LOG=log)
rc = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_frame_score.py"), "-m", "gpu", "-q", "-s",
                     "--durations=5"], cwd=ROOT, env=env).returncode
sys.exit(rc)
