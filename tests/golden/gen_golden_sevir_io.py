#!/usr/bin/env python3
"""Generate tests/golden/sevir_io.npz by IMPORTING the reference (through _ref_import.py), as gen_golden.py does.

    python tests/golden/gen_golden_sevir_io.py

SEVIRDataLoader's two static methods (datasets/sevir/sevir_dataloader.py): preprocess_data_dict (:610-649) on uint8 'vil' events in the
NHWT layout, to NTHWC, and process_data_dict_back (:652-681) on fp32 frames, both for rescale '01' and 'sevir'.  The offline pool
(save_downsampled_dataset) is not a static method and needs skimage and HDF5 files: it is restated in tests/_sevir_io_ref.py only.
Stored: raw (2, 4, 4, 16) uint8 holding every byte value, pre_{01,sevir} = the preprocessed events, frames (2, 3, 4, 8, 1) fp32 (values
around [0, 1], exact zeros and ones, values outside) and back_{01,sevir} = frames processed back.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF_SRC, install_stubs  # noqa: E402


def gen_sevir_io():
    install_stubs()
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    from prediff.datasets.sevir.sevir_dataloader import SEVIRDataLoader
    rng = np.random.default_rng(20)
    raw = rng.permutation(np.arange(512) % 256).astype(np.uint8).reshape(2, 4, 4, 16)
    frames = rng.uniform(-0.25, 1.25, size=(2, 3, 4, 8, 1)).astype(np.float32)
    frames.reshape(-1)[:6] = [0.0, 1.0, -1.0, 2.0, 0.5, 1e-3]
    arrs = {"raw": raw, "frames": frames}
    for rescale in ("01", "sevir"):
        pre = SEVIRDataLoader.preprocess_data_dict({"vil": torch.from_numpy(raw.copy())}, data_types=["vil"], layout="NTHWC", rescale=rescale)
        arrs[f"pre_{rescale}"] = pre["vil"].numpy()
        back = SEVIRDataLoader.process_data_dict_back({"vil": torch.from_numpy(frames.copy())}, data_types=["vil"], rescale=rescale)
        arrs[f"back_{rescale}"] = back["vil"].numpy()
        assert arrs[f"pre_{rescale}"].dtype == np.float32 and arrs[f"back_{rescale}"].dtype == np.float32
    np.savez_compressed(os.path.join(HERE, "sevir_io.npz"), **arrs)
    print("wrote sevir_io", {k: v.shape for k, v in arrs.items()})


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    gen_sevir_io()
