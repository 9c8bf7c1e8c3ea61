"""FVD, host side: the restatement tests/_i3d_ref.py against the fixtures generated from the reference (tests/golden/gen_golden_fvd.py),
the state_dict schema of InceptionI3d, and FrechetVideoDistance's argument checks, state handling and compute() -- no GPU needed."""
import json
import os

import numpy as np
import pytest
import torch

import _i3d_ref as R
from conftest import GOLDEN
from prediff_amd import FrechetVideoDistance, InceptionI3d
from prediff_amd._lib import PrediffHipError

_SD = {}


def weights(classes=400):
    if classes not in _SD:
        _SD[classes] = R.seeded_weights(InceptionI3d(classes).state_dict())
    return _SD[classes]


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_preprocess_matches_reference(golden, name):
    """fp32 bilinear on data in [-1, 1] on both sides: a few ulp of 1 (about 5e-7); bound 1e-5 absolute"""
    g = golden("fvd")
    pre = R.preprocess(R.prepare(R.fixture_input(name)))
    sub = torch.tensor(R.SUB)
    got = pre[..., sub, :][..., sub].numpy()
    err = float(np.abs(got - g["pre_" + name]).max())
    print(f"[preprocess {name}] max abs difference to the reference {err:.2e}")
    assert got.shape == g["pre_" + name].shape and err < 1e-5


@pytest.mark.parametrize("name,classes", [("a", 400), ("b", 400), ("b", 600)])
def test_restatement_features_match_reference(golden, name, classes):
    g = golden("fvd")
    want = torch.from_numpy(g[("feat_" if classes == 400 else "feat600_") + name])
    got = R.features_of(weights(classes), R.fixture_input(name))
    err = max(R.rel_l2(got, want))
    print(f"[features {name} {classes}] rel-L2 to the reference in float64 {err:.2e}")
    assert got.shape == want.shape == (R.FIXTURE_INPUTS[name][0], classes) and err < 1e-9
    assert float(want.abs().max()) > 1e-2          # the seeded network carries signal to its last layer


def test_restatement_frechet_matches_reference(golden):
    g = golden("fvd")
    fd, _ = R.frechet(torch.from_numpy(g["fd_x1"]), torch.from_numpy(g["fd_x2"]))
    assert abs(fd - float(g["fd"])) < 1e-6 * abs(float(g["fd"]))


class _Features(torch.nn.Module):
    """a custom feature extractor: (N, T, 3, H, W) -> (N, 16)"""

    def forward(self, v):
        return v.float().mean(dim=(1, 3, 4)).repeat(1, 6)[:, :16]


def test_compute_from_state_matches_reference(golden):
    """compute() from the six state tensors (eigenvalue route of torchmetrics' _compute_fid) against the reference's SVD route, which
    differs by its 1e-10 eigenvalue floor: 1e-6 relative"""
    g = golden("fvd")
    m = FrechetVideoDistance(feature=_Features())
    assert m.real_features_sum.dtype == torch.float64 and m.real_features_cov_sum.shape == (16, 16)
    assert m.fake_features_num_samples.dtype == torch.int64
    for kind, key in (("real", "fd_x1"), ("fake", "fd_x2")):
        f = torch.from_numpy(g[key])
        setattr(m, f"{kind}_features_sum", f.sum(0))
        setattr(m, f"{kind}_features_cov_sum", f.T @ f)
        setattr(m, f"{kind}_features_num_samples", torch.tensor(f.shape[0]))
    got = float(m.compute())
    assert abs(got - float(g["fd"])) < 1e-6 * abs(float(g["fd"])), (got, float(g["fd"]))


def test_schema_matches_reference():
    with open(os.path.join(GOLDEN, "i3d_schema.json")) as f:
        want = {k: tuple(v) for k, v in json.load(f).items()}
    got = {k: tuple(v.shape) for k, v in InceptionI3d(400).state_dict().items()}
    assert got == want
    assert tuple(InceptionI3d(600).state_dict()["logits.conv3d.weight"].shape) == (600, 1024, 1, 1, 1)


def test_seeded_i3d_state_dict_is_a_valid_batchnorm():
    sd = weights()
    assert all(float(v.min()) > 0 for k, v in sd.items() if k.endswith("running_var"))
    assert all(v.dtype == torch.int64 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    again = R.seeded_weights(InceptionI3d(400).state_dict())
    assert all(torch.equal(sd[k], again[k]) for k in sd)


def test_documented_errors():
    with pytest.raises(PrediffHipError, match="i3d_pretrained_400.pt"):
        FrechetVideoDistance(feature=400)
    with pytest.raises(PrediffHipError, match="i3d_pretrained_600.pt"):
        FrechetVideoDistance(feature=600)
    with pytest.raises(ValueError):
        FrechetVideoDistance(feature=500, weights={})
    with pytest.raises(TypeError):
        FrechetVideoDistance(feature="400")
    with pytest.raises(ValueError, match="precision"):
        FrechetVideoDistance(feature=400, weights=weights(), precision="fp64")
    with pytest.raises(ValueError, match="precision"):
        InceptionI3d(400, precision="tf32")
    m = FrechetVideoDistance(feature=400, weights=weights())
    with pytest.raises(ValueError, match="temporal length"):
        m.update(torch.zeros(1, 8, 1, 32, 32), real=True)
    with pytest.raises(ValueError, match="temporal length"):          # still short after the doubling
        FrechetVideoDistance(feature=_Features(), auto_t=True).update(torch.zeros(1, 4, 1, 32, 32), real=True)
    with pytest.raises(ValueError, match="channels"):
        m.update(torch.zeros(1, 9, 2, 32, 32), real=True)
    with pytest.raises(PrediffHipError):                              # no host fall-back: a CPU tensor is refused
        m.update(torch.zeros(1, 9, 1, 32, 32), real=True)


def test_weights_from_a_file(tmp_path):
    p = tmp_path / "i3d_pretrained_400.pt"
    torch.save(weights(), p)
    m = FrechetVideoDistance(feature=400, weights=str(p))
    sd = m.inception.state_dict()
    assert all(torch.equal(sd[k], weights()[k]) for k in sd)


@pytest.mark.parametrize("keep", [False, True])
def test_reset_honours_reset_real_features(keep):
    m = FrechetVideoDistance(feature=_Features(), reset_real_features=not keep)
    for kind in ("real", "fake"):
        setattr(m, f"{kind}_features_sum", torch.ones(16, dtype=torch.float64))
        setattr(m, f"{kind}_features_cov_sum", torch.ones((16, 16), dtype=torch.float64))
        setattr(m, f"{kind}_features_num_samples", torch.tensor(3))
    m.reset()
    assert float(m.fake_features_sum.sum()) == 0 and float(m.fake_features_cov_sum.sum()) == 0 and int(m.fake_features_num_samples) == 0
    assert float(m.real_features_sum.sum()) == (16 if keep else 0) and int(m.real_features_num_samples) == (3 if keep else 0)
    assert float(m.real_features_cov_sum.sum()) == (256 if keep else 0)
    m.sync()                                                           # no process group: a no-op
