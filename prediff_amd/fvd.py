"""Fréchet video distance on the device: I3D features from the HIP engine, fp64 moments in a fixed order, the distance on the host.

Drop-in for the reference's ``FrechetVideoDistance`` (evaluation/fvd/torchmetrics_wrap.py:84-270) apart from two keywords: ``weights``
(the path of the reference's ``i3d_pretrained_400.pt`` / ``i3d_pretrained_600.pt``, or a ``state_dict``) and ``precision`` (of the I3D
engine, "fp32" by default).  Nothing is ever downloaded: an integer ``feature`` without ``weights`` raises and names the file to supply.

``update(videos, real)``: frames in ``layout`` with values in [0, 1] (``normalize=True``: [0, 255]), 1 or 3 channels (one channel is read
as three equal ones), at least 9 frames -- ``auto_t=True`` repeats every frame of a shorter video twice first.  The frames are read in
place, preprocessed as ``I3DWrapper.preprocess`` does (pd_i3d_preprocess) and run through ``InceptionI3d``; a custom ``nn.Module`` feature
extractor is called with the reference's (N, T, 3, H, W) tensor instead.  Either way the (n, d) features go through
pd_feature_moments_update.  State: the reference's six tensors -- fp64 sums (d), fp64 sums of outer products (d, d), int64 counts -- on the
device; ``sync(group)`` all-reduces them with SUM and is called on every rank of the group, also on ranks that made no update.

``compute()`` (host, fp64; torchmetrics' ``_compute_fid``): mu = sum / n, Sigma = (cov_sum - n mu mu^T) / (n - 1),
FVD = |mu_r - mu_f|^2 + tr Sigma_r + tr Sigma_f - 2 sum_i Re sqrt(lambda_i(Sigma_r Sigma_f)).
"""
from typing import Any, Mapping, Optional, Union

import torch
from torch import nn

from . import _lib as L
from .i3d import InceptionI3d

MIN_T = 9
_STATE = ("features_sum", "features_cov_sum", "features_num_samples")


def frechet_distance_from_moments(mu1: torch.Tensor, sigma1: torch.Tensor, mu2: torch.Tensor, sigma2: torch.Tensor) -> torch.Tensor:
    """|mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 sum_i Re sqrt(lambda_i(sigma1 sigma2)) in fp64 (torchmetrics' _compute_fid)."""
    mu1, sigma1, mu2, sigma2 = (t.detach().double().cpu() for t in (mu1, sigma1, mu2, sigma2))
    a = (mu1 - mu2).square().sum()
    c = torch.linalg.eigvals(sigma1 @ sigma2).sqrt().real.sum()
    return a + sigma1.trace() + sigma2.trace() - 2 * c


class FrechetVideoDistance(nn.Module):
    higher_is_better = False
    is_differentiable = False
    full_state_update = False
    min_t = MIN_T

    def __init__(self, feature: Union[int, nn.Module] = 400, layout: str = "NTCHW", reset_real_features: bool = True,
                 normalize: bool = False, auto_t: bool = False, weights: Union[None, str, Mapping[str, torch.Tensor]] = None,
                 precision: str = "fp32", **kwargs: Any) -> None:
        super().__init__()
        if set(layout) != set("NTCHW") or len(layout) != 5:
            raise ValueError(f"layout {layout!r}: a permutation of N, T, C, H, W")
        self.layout = layout
        if isinstance(feature, int) and not isinstance(feature, bool):
            if feature not in (400, 600):
                raise ValueError(f"Integer input to argument `feature` must be one of [400, 600], but got {feature}.")
            if weights is None:
                raise L.PrediffHipError(
                    f"FrechetVideoDistance(feature={feature}) needs the I3D weights and never downloads them: pass "
                    f"weights=<path of i3d_pretrained_{feature}.pt> (the reference's checkpoint file) or weights=<its state_dict>")
            self.inception = InceptionI3d(num_classes=feature, precision=precision)      # (an unknown precision raises here)
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") else weights
            self.inception.load_state_dict(sd)
            self.custom, num_features = False, feature
        elif isinstance(feature, nn.Module):
            self.inception, self.custom = feature, True
            dummy = torch.randint(0, 255, (1, 9, 3, 299, 299), dtype=torch.uint8)
            num_features = self.inception(dummy).shape[-1]
        else:
            raise TypeError("Got unknown input to argument `feature`")
        if not isinstance(reset_real_features, bool):
            raise ValueError("Argument `reset_real_features` expected to be a bool")
        if not isinstance(normalize, bool):
            raise ValueError("Argument `normalize` expected to be a bool")
        self.reset_real_features, self.normalize, self.auto_t = reset_real_features, normalize, auto_t
        self.num_features = num_features
        self.orig_dtype = torch.float32
        for kind in ("real", "fake"):
            self._zero(kind, torch.device("cpu"))
        self.eval()

    # ------------------------------------------------------------------------------------------------ state
    def _zero(self, kind, dev):
        d = self.num_features
        setattr(self, f"{kind}_features_sum", torch.zeros(d, dtype=torch.float64, device=dev))
        setattr(self, f"{kind}_features_cov_sum", torch.zeros((d, d), dtype=torch.float64, device=dev))
        setattr(self, f"{kind}_features_num_samples", torch.zeros((), dtype=torch.int64, device=dev))

    def _state(self, kind):
        return [getattr(self, f"{kind}_{n}") for n in _STATE]

    def _state_to(self, dev):
        for kind in ("real", "fake"):
            for n in _STATE:
                t = getattr(self, f"{kind}_{n}")
                if t.device != dev:
                    setattr(self, f"{kind}_{n}", t.to(dev))

    def reset(self) -> None:
        dev = self.real_features_sum.device
        if self.reset_real_features:
            self._zero("real", dev)
        self._zero("fake", dev)

    # ------------------------------------------------------------------------------------------------ update
    def update(self, videos: torch.Tensor, real: bool) -> None:
        if videos.dim() != 5:
            raise ValueError(f"videos must have the five axes of layout {self.layout!r}; got shape {tuple(videos.shape)}")
        T, Cn = videos.shape[self.layout.find("T")], videos.shape[self.layout.find("C")]
        double_t = False
        if T < self.min_t:
            if not self.auto_t:
                raise ValueError(f"The temporal length of the input is smaller than the minimal requirement:"
                                 f" videos.shape[1] = {T} < {self.min_t}.")
            double_t, T = True, 2 * T
            if T < self.min_t:
                raise ValueError(f"The temporal length of the input is smaller than the minimal requirement:"
                                 f" videos.shape[1] = {T} < {self.min_t}.")
        if Cn not in (1, 3):
            raise ValueError(f"videos must have 1 or 3 channels; got {Cn}")
        if not videos.is_cuda:
            raise L.PrediffHipError("FrechetVideoDistance.update runs on the HIP device the videos were decoded on; got a CPU tensor")
        dev = videos.device
        if self.custom:
            v = videos.permute(*[self.layout.find(a) for a in "NTCHW"])
            if double_t:
                v = torch.repeat_interleave(v, repeats=2, dim=1)
            v = v / 255.0 if self.normalize else v
            if Cn == 1:
                v = v.repeat(1, 1, 3, 1, 1)
            feats = self.inception(v)
        else:
            if next(self.inception.parameters()).device != dev:
                self.inception.to(dev)
            feats = self.inception.features(videos, layout=self.layout, normalize=self.normalize, auto_t=double_t)
        self.orig_dtype = feats.dtype
        if feats.dim() == 1:
            feats = feats.unsqueeze(0)
        feats = feats.detach().float().contiguous()
        self._state_to(dev)
        s, c, n = self._state("real" if real else "fake")
        with L.on_device(feats):
            L.feature_moments_update(feats, s, c)
        n += videos.shape[self.layout.find("N")]

    forward = update

    def sync(self, group=None):
        """All-reduce the six state tensors with SUM over the ranks of `group`; every rank calls it, also ranks that made no update."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        if dist.get_backend(group) == "nccl" and not self.real_features_sum.is_cuda:
            self._state_to(torch.device("cuda", torch.cuda.current_device()))
        for kind in ("real", "fake"):
            for t in self._state(kind):
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    # ------------------------------------------------------------------------------------------------ compute
    def compute(self) -> torch.Tensor:
        mom = []
        for kind in ("real", "fake"):
            s, c, n = (t.detach().cpu() for t in self._state(kind))
            n = n.double()
            mu = s / n
            mom += [mu, (c - n * torch.outer(mu, mu)) / (n - 1)]
        return frechet_distance_from_moments(*mom).to(self.orig_dtype)
