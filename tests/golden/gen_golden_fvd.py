"""Fixtures of the FVD path from the read-only reference (runs where the reference tree is; never on the GPU box, never in a test).

Imports the reference's pytorch_i3d.py, fvd.py and torchmetrics_wrap.py (for I3DWrapper.preprocess) by file path under a private package
name, with stand-in modules for what their imports need and this machine lacks (torchmetrics; the checkpoint downloader, which is never
called).  Copies nothing.  Writes tests/golden/i3d_schema.json (key -> shape of InceptionI3d(400)) and tests/golden/fvd.npz:
  pre_a / pre_b      I3DWrapper.preprocess of the two seeded inputs at rows / columns _i3d_ref.SUB (fp32)
  feat_a / feat_b    InceptionI3d(400) in evaluation mode, float64, on seeded_i3d_state_dict weights; feat600_b the same with 600 classes
  fd_x1, fd_x2, fd   two seeded feature sets (64, 16) and the reference's frechet_distance of them (float64)
The weights are regenerated from the seed on both sides and are not stored.

    python tests/golden/gen_golden_fvd.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _ref_import import REF_SRC, install_stubs  # noqa: E402  (tests/golden is on the path: this file runs as a script from there)

REF = os.path.join(REF_SRC, "prediff")


def _pkg(name, path=None):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    sys.modules[name] = m
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def import_reference_fvd():
    install_stubs()                                   # torchmetrics.Metric stand-in
    tm = sys.modules["torchmetrics"]
    tmm = _pkg("torchmetrics.metric")
    tmm.Metric = tm.Metric
    _pkg("torchmetrics.image")
    fid = _pkg("torchmetrics.image.fid")

    def _compute_fid(*a, **k):
        raise RuntimeError("torchmetrics stand-in: _compute_fid is not available")

    fid._compute_fid = _compute_fid
    _pkg("refprediff", REF)
    _pkg("refprediff.utils", os.path.join(REF, "utils"))
    _pkg("refprediff.evaluation", os.path.join(REF, "evaluation"))
    _pkg("refprediff.evaluation.fvd", os.path.join(REF, "evaluation", "fvd"))
    dl = _pkg("refprediff.evaluation.fvd.download")    # the downloader is never imported, let alone called

    def load_i3d_pretrained(*a, **k):
        raise RuntimeError("no checkpoint is fetched")

    dl.load_i3d_pretrained = load_i3d_pretrained
    _load("refprediff.utils.optim", os.path.join(REF, "utils", "optim.py"))
    ns = types.SimpleNamespace()
    ns.i3d = _load("refprediff.evaluation.fvd.pytorch_i3d", os.path.join(REF, "evaluation", "fvd", "pytorch_i3d.py"))
    ns.fvd = _load("refprediff.evaluation.fvd.fvd", os.path.join(REF, "evaluation", "fvd", "fvd.py"))
    ns.wrap = _load("refprediff.evaluation.fvd.torchmetrics_wrap", os.path.join(REF, "evaluation", "fvd", "torchmetrics_wrap.py"))
    return ns


def main():
    import _i3d_ref as R
    from prediff_amd.seeding import seeded_input
    ref = import_reference_fvd()
    out = {}
    net = ref.i3d.InceptionI3d(400).eval()
    with open(os.path.join(HERE, "i3d_schema.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in net.state_dict().items()}, f, indent=0)
    net.load_state_dict(R.seeded_weights(net.state_dict()))
    net = net.double()
    net600 = ref.i3d.InceptionI3d(600).eval()
    net600.load_state_dict(R.seeded_weights(net600.state_dict()))
    net600 = net600.double()
    sub = torch.tensor(R.SUB)
    for name in R.FIXTURE_INPUTS:
        v = R.fixture_input(name)
        v3 = v.repeat(1, 1, 3, 1, 1) if v.shape[2] == 1 else v            # what FrechetVideoDistance.update hands to the wrapper
        pre = ref.wrap.I3DWrapper.preprocess(v3.clone())
        out["pre_" + name] = pre[..., sub, :][..., sub].numpy()
        with torch.no_grad():
            out["feat_" + name] = net(ref.wrap.I3DWrapper.preprocess(v3.double())).numpy()
            if name == "b":
                out["feat600_" + name] = net600(ref.wrap.I3DWrapper.preprocess(v3.double())).numpy()
        print(name, out["pre_" + name].shape, out["feat_" + name].shape, flush=True)
    x1 = seeded_input("fd.x1", (64, 16), 4102).double()
    mix = seeded_input("fd.mix", (16, 16), 4102).double()
    x2 = 0.5 + seeded_input("fd.x2", (64, 16), 4102).double() @ (torch.eye(16, dtype=torch.float64) + 0.3 * mix)
    out["fd_x1"], out["fd_x2"] = x1.numpy(), x2.numpy()
    out["fd"] = np.float64(ref.fvd.frechet_distance(x1.clone(), x2.clone()))
    np.savez_compressed(os.path.join(HERE, "fvd.npz"), **out)
    print("fd", out["fd"], "size", os.path.getsize(os.path.join(HERE, "fvd.npz")))


if __name__ == "__main__":
    main()
