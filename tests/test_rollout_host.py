"""Rolling forecasts, host side (prediff_amd/rollout.py): RolloutPlan against the formulas and tests/_rollout_ref.py, and
what rollout_sample refuses before any draw, on modules constructed on the CPU."""
import math

import numpy as np
import pytest
import torch

import _rollout_ref as R
from prediff_amd.rollout import RolloutPlan, rollout_ensemble, rollout_sample

LENS = [(7, 6), (2, 3), (5, 2), (1, 1)]                                     # (in_len, out_len)


@pytest.mark.parametrize("in_len,out_len", LENS)
def test_plan(in_len, out_len):
    for s in range(1, out_len + 1):
        for horizon in range(1, 3 * out_len + 2):
            p = RolloutPlan(in_len, out_len, horizon, s)
            n = 1 if horizon <= out_len else math.ceil((horizon - out_len) / s) + 1
            assert p.segments == n == R.n_segments(out_len, horizon, s) == len(p.starts) == len(p.keep)
            assert (horizon <= out_len) == (n == 1)
            assert p.starts == [j * s for j in range(n)]
            assert p.starts[-1] + out_len >= horizon                         # the last segment ends at or beyond the horizon
            assert n == 1 or p.starts[-2] + out_len < horizon               # and no segment is superfluous
            src = [p.source(f) for f in range(horizon)]
            assert len(set(src)) == horizon                                  # every result frame has exactly one source
            for j in range(n):                                               # the sources of one segment are a prefix of it
                assert [t for k, t in src if k == j] == list(range(p.keep[j]))
                assert 1 <= p.keep[j] <= out_len
                for t in range(p.keep[j]):
                    assert src[p.starts[j] + t] == (j, t)
            assert p.keep == [s] * (n - 1) + [horizon - (n - 1) * s] and sum(p.keep) == horizon
            for f in range(horizon):
                assert p.source(f) == (min(f // s, n - 1), f - min(f // s, n - 1) * s)
            # the assembly of the restatement picks exactly the plan's sources
            segs = [np.arange(out_len, dtype=np.float32)[None, :] + 100 * j for j in range(n)]
            assert R.assemble(segs, out_len, horizon, s)[0].tolist() == [100 * j + t for j, t in src]
        assert RolloutPlan(in_len, out_len, 2 * out_len).stride == out_len   # the default stride


def test_plan_refusals():
    for bad in (0, 7, -1, 2.5, "2"):
        with pytest.raises(ValueError, match=r"\[1, 6\]|integer"):
            RolloutPlan(7, 6, 12, bad)
    for bad in (0, -3, 1.5, None):
        with pytest.raises(ValueError, match=r"\[1, inf\)|integer"):
            RolloutPlan(7, 6, bad)
    with pytest.raises(ValueError):
        RolloutPlan(0, 6, 12)
    with pytest.raises(ValueError):
        RolloutPlan(7, 0, 12)
    with pytest.raises(ValueError, match="frame"):
        RolloutPlan(7, 6, 12).source(12)


# ------------------------------------------------------------------------------------------------ the driver's refusals
class _NoForward(torch.nn.Module):
    def forward(self, *a):
        raise AssertionError("the denoiser must not run")

    def encode(self, *a):
        raise AssertionError("the VAE must not run")

    def decode(self, *a):
        raise AssertionError("the VAE must not run")


class _NoTape:
    def __getitem__(self, k):
        raise AssertionError("no draw may be made")


LDM_KW = dict(layout="NTHWC", data_shape=(2, 8, 8, 1), timesteps=1000, use_ema=False, latent_shape=(2, 4, 4, 1))


def _cpu_plain(**kw):
    from prediff_amd.latent_diffusion import LatentDiffusion
    return LatentDiffusion(_NoForward(), **dict(LDM_KW, **kw))


def _cpu_tiled(**kw):
    from prediff_amd.tiled import TiledLatentDiffusion
    return TiledLatentDiffusion(_NoForward(), canvas=(6, 7), stride=(2, 2), **dict(LDM_KW, **kw))


def test_refusals():
    from prediff_amd import rollout_ensemble as exported_ensemble, rollout_sample as exported_sample, RolloutPlan as ExportedPlan
    assert exported_sample is rollout_sample and exported_ensemble is rollout_ensemble and ExportedPlan is RolloutPlan
    rng = torch.get_rng_state()
    plain, tiled = _cpu_plain(), _cpu_tiled()
    cases = [(plain, torch.zeros(2, 3, 4, 4, 1)), (tiled, torch.zeros(2, 3, 6, 7, 1))]
    for ldm, zc in cases:
        ldm.set_alignment(lambda *a, **k: pytest.fail("the guidance must not run"))
        kw = dict(cond=zc, horizon=5, batch_size=2, return_decoded=False, sampler="ddim", ddim_steps=2)     # out_len 2: 3 segments
        good = [_NoTape()] * 3
        # per-segment sequences of the wrong length
        for name, bad in (("noise_tape", [_NoTape()] * 2), ("noise_tape", [_NoTape()] * 4), ("noise_tape", _NoTape()),
                          ("x_T", [torch.zeros(2, 2, 4, 4, 1)] * 2), ("x_T", torch.zeros(3, 2, 4, 4, 1)),
                          ("alignment_kwargs", [{}] * 2), ("alignment_kwargs", [{}] * 4)):
            with pytest.raises(ValueError, match=f"{name}.*3 segments"):
                rollout_sample(ldm, **dict(dict(kw, noise_tape=good), **{name: bad}))
        with pytest.raises(ValueError, match=r"stride.*\[1, 2\]"):
            rollout_sample(ldm, stride=3, noise_tape=good, **kw)
        with pytest.raises(ValueError, match=r"horizon"):
            rollout_sample(ldm, **dict(kw, horizon=0))
        shape = ldm.get_batch_latent_shape(2)
        with pytest.raises(NotImplementedError, match="mask"):
            rollout_sample(ldm, mask=torch.ones(shape), x0=torch.zeros(shape), noise_tape=good, **kw)
        with pytest.raises(NotImplementedError, match="return_intermediates"):
            rollout_sample(ldm, return_intermediates=True, noise_tape=good, **kw)
        with pytest.raises(ValueError, match="__is_first_stage__"):          # no first-stage condition to encode the decoded frames with
            rollout_sample(ldm, recondition="pixel", noise_tape=good, **kw)
        with pytest.raises(ValueError, match="recondition"):
            rollout_sample(ldm, recondition="both", noise_tape=good, **kw)
        with pytest.raises(TypeError, match="bogus"):
            rollout_sample(ldm, bogus=1, noise_tape=good, **kw)
    # a condition stage that is not the first stage cannot re-encode pixels either
    other = _cpu_plain(first_stage_model=_NoForward(), cond_stage_model=_NoForward())
    with pytest.raises(ValueError, match="__is_first_stage__"):
        rollout_sample(other, {"y": torch.zeros(2, 3, 8, 8, 1)}, 5, recondition="pixel", batch_size=2, noise_tape=[_NoTape()] * 3)
    # the tiled module keeps refusing alignment, for one segment and for several, and a context that is not the canvas
    for horizon in (2, 5):
        with pytest.raises(NotImplementedError, match="use_alignment"):
            rollout_sample(tiled, torch.zeros(2, 3, 6, 7, 1), horizon, batch_size=2, use_alignment=True, alignment_kwargs={})
    with pytest.raises(ValueError, match="latent context"):
        rollout_sample(tiled, torch.zeros(2, 3, 4, 4, 1), 5, batch_size=2)
    # the ensemble front end: the same refusals reach the caller, and it owns the noise
    with pytest.raises(ValueError, match=r"stride"):
        rollout_ensemble(plain, torch.zeros(1, 3, 4, 4, 1), 4, 5, stride=0)
    with pytest.raises(NotImplementedError, match="mask"):
        rollout_ensemble(plain, torch.zeros(1, 3, 4, 4, 1), 4, 5, mask=torch.ones(1))
    with pytest.raises(TypeError, match="noise_tape"):
        rollout_ensemble(plain, torch.zeros(1, 3, 4, 4, 1), 4, 5, noise_tape=[None] * 3)
    assert torch.equal(torch.get_rng_state(), rng)                           # refused before any draw
