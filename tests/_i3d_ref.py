"""Plain-torch restatement of the FVD path, written from the algorithm: the I3D preprocessing, Inception-v1 I3D in evaluation mode and
the Fréchet distance.  Pinned on fixtures generated from the reference (tests/golden/gen_golden_fvd.py -> fvd.npz, i3d_schema.json) by
tests/test_fvd_host.py; the GPU tests compare the HIP engine against this file.  Everything runs in the dtype of its input."""
import math

import torch
import torch.nn.functional as F

from prediff_amd.i3d import ARCH
from prediff_amd.seeding import seeded_i3d_state_dict, seeded_input

RES = 224
I3D_SEED = 4100
# the two fixture inputs, (N, T, C, H, W) with values in [0, 1]
FIXTURE_INPUTS = {"a": (2, 9, 1, 32, 48), "b": (1, 12, 3, 40, 40)}
SUB = tuple(range(0, RES, 9)) + (RES - 1,)          # rows / columns of the preprocessed frames the fixture keeps


def fixture_input(name):
    return seeded_input("fvd." + name, FIXTURE_INPUTS[name], 4101, kind="uniform")


def seeded_weights(template, seed=I3D_SEED):
    return seeded_i3d_state_dict(template, seed)


# ---------------------------------------------------------------------------------------------------- preprocessing
def prepare(videos_ntchw, normalize=False, auto_t=False):
    """FrechetVideoDistance.update's frame handling: optional frame doubling, / 255, one channel -> three."""
    v = videos_ntchw
    if auto_t:
        v = torch.repeat_interleave(v, 2, dim=1)
    if normalize:
        v = v / 255.0
    if v.shape[2] == 1:
        v = v.repeat(1, 1, 3, 1, 1)
    return v


def preprocess(v):
    """(N, T, 3, H, W) in [0, 1] -> (N, 3, T, 224, 224) in [-1, 1]: bilinear resize of the short side to 224, centre crop, 2 x - 1."""
    n, t, c, h, w = v.shape
    scale = RES / min(h, w)
    size = (RES, math.ceil(w * scale)) if h < w else (math.ceil(h * scale), RES)
    y = F.interpolate(v.reshape(n * t, c, h, w), size=size, mode="bilinear", align_corners=False)
    h0, w0 = (size[0] - RES) // 2, (size[1] - RES) // 2
    y = y[:, :, h0:h0 + RES, w0:w0 + RES].reshape(n, t, c, RES, RES).permute(0, 2, 1, 3, 4)
    return (y - 0.5) * 2


# ---------------------------------------------------------------------------------------------------- the network
def same_pads(size, kernel, stride):
    """F.pad argument (W, H, T order, front / back) of TF-style SAME padding for a (T, H, W) size"""
    pad = []
    for n, k, s in reversed(list(zip(size, kernel, stride))):
        p = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
        pad += [p // 2, p - p // 2]
    return pad


def maxpool_same(x, kernel, stride):
    """x (B, C, T, H, W): zero padding (the zeros take part in the max), then max-pool"""
    return F.max_pool3d(F.pad(x, same_pads(x.shape[2:], kernel, stride)), kernel, stride)


def unit(sd, name, x, kernel=(1, 1, 1), stride=(1, 1, 1), bn=True, relu=True):
    dt = x.dtype
    x = F.conv3d(F.pad(x, same_pads(x.shape[2:], kernel, stride)), sd[name + ".conv3d.weight"].to(dt),
                 sd[name + ".conv3d.bias"].to(dt) if name + ".conv3d.bias" in sd else None, stride=stride)
    if bn:
        g, b, m, v = (sd[f"{name}.bn.{k}"].to(dt).view(1, -1, 1, 1, 1) for k in ("weight", "bias", "running_mean", "running_var"))
        x = (x - m) / torch.sqrt(v + 1e-5) * g + b
    return F.relu(x) if relu else x


def mixed(sd, name, x):
    b0 = unit(sd, name + ".b0", x)
    b1 = unit(sd, name + ".b1b", unit(sd, name + ".b1a", x), (3, 3, 3))
    b2 = unit(sd, name + ".b2b", unit(sd, name + ".b2a", x), (3, 3, 3))
    b3 = unit(sd, name + ".b3b", maxpool_same(x, (3, 3, 3), (1, 1, 1)))
    return torch.cat([b0, b1, b2, b3], 1)


def i3d_features(sd, x, upto=None):
    """x (B, 3, T, 224, 224) in [-1, 1] -> (B, classes); `upto`: return the activations (B, C, T, H, W) behind that endpoint instead"""
    for ep, kind, args in ARCH:
        if kind == "stem":
            x = unit(sd, ep, x, (7, 7, 7), (2, 2, 2))
        elif kind == "conv":
            x = unit(sd, ep, x, args[2])
        elif kind == "pool":
            x = maxpool_same(x, args[0], args[1])
        else:
            x = mixed(sd, ep, x)
        if ep == upto:
            return x
    x = F.avg_pool3d(x, (2, 7, 7), 1)
    x = unit(sd, "logits", x, bn=False, relu=False)
    return x.squeeze(3).squeeze(3).mean(2)


def features_of(sd, videos_ntchw, dtype=torch.float64, normalize=False, auto_t=False):
    with torch.no_grad():
        return i3d_features(sd, preprocess(prepare(videos_ntchw.to(dtype), normalize, auto_t)))


# ---------------------------------------------------------------------------------------------------- the distance
def moments(f):
    f = f.double()
    n = f.shape[0]
    mu = f.mean(0)
    return mu, (f.T @ f - n * torch.outer(mu, mu)) / (n - 1)


def frechet(f1, f2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), the trace of the root as the sum of the roots of the product's eigenvalues"""
    m1, s1 = moments(f1)
    m2, s2 = moments(f2)
    tr = torch.linalg.eigvals(s1 @ s2).sqrt().real.sum()
    return float((m1 - m2).square().sum() + s1.trace() + s2.trace() - 2 * tr), float(s1.trace() + s2.trace())


def rel_l2(a, b):
    """per row: |a - b| / |b| in fp64"""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).flatten(1).norm(dim=1) / b.flatten(1).norm(dim=1)).tolist()


# ---------------------------------------------------------------------------------------------------- end-to-end inputs
def e2e_videos():
    """16 "real" and 16 "fake" single-channel videos (N, T, C, H, W) = (16, 6, 1, 32, 32) in [0, 1]: smooth drifting fields against
    noisier, brighter ones -- two distributions far enough apart that the FVD is a sizeable part of tr Sigma_r + tr Sigma_f."""
    out = []
    for kind, gain, noise, shift in (("real", 1.0, 0.0, 0.0), ("fake", 0.6, 0.25, 0.2)):
        coarse = seeded_input("e2e." + kind, (16, 1, 3, 6, 6), 4103, kind="uniform")
        v = F.interpolate(coarse, size=(6, 32, 32), mode="trilinear", align_corners=True).permute(0, 2, 1, 3, 4)
        v = gain * v + shift + noise * seeded_input("e2e.n." + kind, tuple(v.shape), 4103, kind="uniform")
        out.append(v.clamp(0, 1).contiguous())
    return out
