#!/usr/bin/env python3
"""Generate tests/golden/skill_score_pool.npz by IMPORTING the reference (through _ref_import.py), as gen_golden.gen_skill() does.

    python tests/golden/gen_golden_pool.py

The reference's SEVIRSkillScore with preprocess_type "sevir_pool{s}" (datasets/sevir/evaluation.py:220-231: max-pool over (H, W),
kernel = stride = s) on _inputs.skill_inputs() (3 x 6 x 32 x 32 x 1, NaNs and exact-threshold values), two updates, modes 0/1/2,
s in {4, 16} and 3 (does not divide 32: the trailing rows / columns are dropped).  Stores the counts and the compute() results.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _ref_import import import_reference  # noqa: E402
from _inputs import skill_inputs  # noqa: E402

THR = (16, 74, 133, 160, 181, 219)
POOLS = (4, 16, 3)


def gen_skill_pool():
    R = import_reference()
    pred, target = skill_inputs()
    arrs = {}
    for s in POOLS:
        for mode in ("0", "1", "2"):
            m = R.SEVIRSkillScore(layout="NTHWC", mode=mode, seq_len=6, preprocess_type=f"sevir_pool{s}", threshold_list=THR,
                                  metrics_list=("csi", "pod", "sucr", "bias"))
            m.update(pred, target)
            m.update(pred.flip(0), target)          # second, different batch
            for name in ("hits", "misses", "fas"):
                arrs[f"p{s}_{name}_{mode}"] = getattr(m, name).detach().cpu().numpy()
            res = m.compute()
            for thr in THR + ("avg",):
                for met in ("csi", "pod", "sucr", "bias"):
                    arrs[f"p{s}_score_{mode}_{thr}_{met}"] = np.asarray(res[thr][met], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "skill_score_pool.npz"), **arrs)
    print("wrote skill_score_pool", len(arrs), "arrays")


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    gen_skill_pool()
