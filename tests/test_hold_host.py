"""Held-region sampling, host side ("Held regions"): the hold columns of the schedule against tests/_hold_ref.py, the
order in which the loops read a noise tape (driven on the CPU with a stub denoiser and stub step kernels), what is refused before any
draw, and the conditions of the rule itself on the analytic mixture (restatement only, fp64)."""
import contextlib

import numpy as np
import pytest
import torch

import _dpmpp_ref as R
import _hold_ref as H
from oracle import diffusion as OD

T = 1000


def _ac(schedule="linear"):
    return np.cumprod(1.0 - OD.beta_schedule(schedule, T)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. the hold columns
@pytest.mark.parametrize("method,n", [("quad", 10), ("uniform", 20), ("logsnr", 15), ("quad", 50)])
def test_hold_columns(method, n):
    from prediff_amd import schedule as S
    ac = _ac()
    steps = S.make_logsnr_timesteps(n, ac) if method == "logsnr" else np.minimum(S.make_ddim_timesteps(method, n, T), T - 1)
    assert np.array_equal(steps, R.grid(n, ac, method))
    _, visited = S.make_dpmpp_2m_coefficients(ac, steps)
    runs = {"2m": (S.make_hold_coefficients(ac.astype(np.float64), steps, visited), R.visits(ac, R.grid(n, ac, method))),
            "ddim": (S.make_hold_coefficients(ac.astype(np.float64), steps), H.ddim_visits(ac, R.grid(n, ac, method), 0.0))}
    if method == "quad" and n == 50:
        assert len(runs["2m"][1]) < len(runs["ddim"][1]) == 50             # repeated grid points: the 2M loops drop them, DDIM does not
    for name, ((cols, start), vs) in runs.items():
        ref_cols, ref_start = H.hold_columns(vs)
        assert cols.dtype == np.float32 and cols.shape == (len(vs), 2) and start.dtype == np.float32 and start.shape == (2,), name
        # both sides are fp64 until the one rounding to fp32: at most one fp32 ulp apart
        assert np.allclose(cols.astype(np.float64), np.asarray(ref_cols), rtol=2.0 ** -23, atol=0), name
        assert np.allclose(start.astype(np.float64), np.asarray(ref_start), rtol=2.0 ** -23, atol=0), name
        assert cols[-1, 0] == 1.0 and cols[-1, 1] == 0.0, name              # the last step writes the known latent itself
        assert (cols[:-1, 1] > 0).all() and (cols[:, 0] > 0).all(), name
        assert np.allclose(start.astype(np.float64), [np.sqrt(vs[0]["a"]), np.sqrt(1 - vs[0]["a"])], rtol=2.0 ** -23, atol=0), name


# ------------------------------------------------------------------------------------------------ 2. tape order
class _ZeroDenoiser(torch.nn.Module):
    def forward(self, x, t, c):
        return torch.zeros_like(x)


class _RecordingTape:
    """Entry k is a tensor filled with k; reads must be consecutive (what ensemble._LazyTape / member_noise_fn assert)."""

    def __init__(self, shape):
        self.shape, self.reads = shape, []

    def __getitem__(self, k):
        assert k == len(self.reads), f"tape read at {k} after {self.reads}"
        self.reads.append(k)
        return torch.full(self.shape, float(k))


LDM_KW = dict(layout="NTHWC", data_shape=(2, 8, 8, 1), timesteps=T, use_ema=False, latent_shape=(2, 4, 4, 1))


@pytest.fixture
def host_loops(monkeypatch):
    """The loops on the CPU: every step kernel a stub that passes the latent through and records the first element (= the tape index)
    of its step noise and of its hold noise."""
    from prediff_amd import _lib as L
    from prediff_amd.latent_diffusion import LatentDiffusion
    calls = []

    def mark(x):
        return None if x is None else int(x.reshape(-1)[0])
    monkeypatch.setattr(L, "on_device", lambda t: contextlib.nullcontext())
    monkeypatch.setattr(L, "hold_blend", lambda z, x0, mask, noise, coef2, out, B, per: (calls.append(("start", mark(noise))), out.copy_(z))[1])
    monkeypatch.setattr(L, "ddim_step", lambda zt, eps, noise, coef, out, B, per: (calls.append(("step", mark(noise), None)), out.copy_(zt))[1])
    monkeypatch.setattr(L, "dpmpp_2m_step", lambda zt, eps, hist, coef, out, B, per: (calls.append(("step", None, None)), out.copy_(zt))[1])
    monkeypatch.setattr(L, "dpmpp_2m_sde_step",
                        lambda zt, eps, noise, hist, coef, out, B, per: (calls.append(("step", mark(noise), None)), out.copy_(zt))[1])
    monkeypatch.setattr(L, "ddim_step_held", lambda zt, eps, noise, shift, x0, m, hn, coef, out, B, per:
                        (calls.append(("step", mark(noise), mark(hn), coef[0, -2:].tolist())), out.copy_(zt))[1])
    monkeypatch.setattr(L, "dpmpp_2m_step_held", lambda zt, eps, hist, shift, x0, m, hn, coef, out, B, per:
                        (calls.append(("step", None, mark(hn), coef[0, -2:].tolist())), out.copy_(zt))[1])
    monkeypatch.setattr(L, "dpmpp_2m_sde_step_held", lambda zt, eps, noise, hist, shift, x0, m, hn, coef, out, B, per:
                        (calls.append(("step", mark(noise), mark(hn), coef[0, -2:].tolist())), out.copy_(zt))[1])
    return LatentDiffusion(_ZeroDenoiser(), **LDM_KW), calls


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("dpmpp_2m_sde", 0.0), ("dpmpp_2m_sde", 1.0)])
def test_tape_order(host_loops, sampler, eta):
    ldm, calls = host_loops
    B, n = 2, 6
    shape = ldm.get_batch_latent_shape(B)
    zc = torch.zeros(B, 3, 4, 4, 1)
    mask = torch.zeros(1, 2, 1, 1, 1)
    mask[:, 0] = 1.0
    kw = dict(cond=zc, batch_size=B, return_decoded=False, sampler=sampler, eta=eta, ddim_steps=n)
    plain = _RecordingTape(shape)
    ldm.sample(noise_tape=plain, **kw)
    K = sum(c[0] == "step" for c in calls)
    assert K >= 3 and not any(c[0] == "start" for c in calls)
    own = H.reads_own_draw(sampler, eta)
    assert len(plain.reads) == len(H.tape_layout(sampler, eta, K, "fixed")) == 1 + (K if own else 0)
    for hold_noise in ("fresh", "fixed"):
        calls.clear()
        tape = _RecordingTape(shape)
        rng = torch.get_rng_state()
        ldm.sample(noise_tape=tape, hold_mask=mask, hold_x0=torch.ones((1,) + shape[1:]), hold_noise=hold_noise, **kw)
        assert torch.equal(torch.get_rng_state(), rng)                      # with a tape nothing comes from a generator
        layout = H.tape_layout(sampler, eta, K, hold_noise)
        assert tape.reads == list(range(len(layout))), (hold_noise, tape.reads)
        if hold_noise == "fixed":
            assert tape.reads == plain.reads                                # the reads of the un-held run
        assert calls[0] == ("start", 0) and len(calls) == 1 + K             # x_T is the noise of the held part at the start
        for k, (_, noise, hn, (k_x, k_n)) in enumerate(calls[1:]):
            assert noise == (layout.index(f"n{k}") if own else (0 if sampler == "dpmpp_2m_sde" else None)), (hold_noise, k)
            if k < K - 1:
                assert hn == (layout.index(f"h{k}") if hold_noise == "fresh" else 0), (hold_noise, k)
                assert 0 < k_n < 1 and 0 < k_x < 1
            else:
                assert (k_x, k_n) == (1.0, 0.0)                             # the last step reads no hold noise
    # the layouts of the issue, spelled out
    assert H.tape_layout("ddim", 0.0, 3, "fresh") == ["x_T", "n0", "h0", "n1", "h1", "n2"]
    assert H.tape_layout("dpmpp_2m", 0.0, 3, "fresh") == ["x_T", "h0", "h1"]
    assert H.tape_layout("dpmpp_2m", 0.0, 3, "fixed") == ["x_T"]


def test_device_generator_order_without_a_tape(host_loops):
    """Without a tape the same draws come from the generator in the same order: x_T, then per step its own draw (eta > 0), then h_k."""
    ldm, calls = host_loops
    B, n = 2, 4
    shape = ldm.get_batch_latent_shape(B)
    mask = torch.zeros(1, 2, 1, 1, 1)
    mask[:, 0] = 1.0
    kw = dict(cond=torch.zeros(B, 3, 4, 4, 1), batch_size=B, return_decoded=False, sampler="ddim", ddim_steps=n, hold_mask=mask,
              hold_x0=torch.ones(shape))
    torch.manual_seed(3)
    ldm.sample(eta=1.0, **kw)
    drawn = torch.get_rng_state()
    torch.manual_seed(3)
    for _ in range(1 + n + (n - 1)):
        torch.randn(shape)
    assert torch.equal(torch.get_rng_state(), drawn)
    torch.manual_seed(3)
    ldm.sample(eta=0.0, hold_noise="fixed", **kw)                           # "fixed" at eta = 0 is a function of x_T alone
    drawn = torch.get_rng_state()
    torch.manual_seed(3)
    torch.randn(shape)
    assert torch.equal(torch.get_rng_state(), drawn)


# ------------------------------------------------------------------------------------------------ 3. refusals
class _NoForward(torch.nn.Module):
    def forward(self, *a):
        raise AssertionError("the denoiser must not run")

    def encode(self, *a):
        raise AssertionError("the VAE must not run")


class _NoTape:
    def __getitem__(self, k):
        raise AssertionError("no draw may be made")


def test_refusals():
    from prediff_amd.latent_diffusion import LatentDiffusion
    from prediff_amd.rollout import rollout_ensemble, rollout_sample
    from prediff_amd.tiled import TiledLatentDiffusion
    rng = torch.get_rng_state()
    plain = LatentDiffusion(_NoForward(), **LDM_KW)
    tiled = TiledLatentDiffusion(_NoForward(), canvas=(6, 7), stride=(2, 2), **LDM_KW)
    for ldm, zc in ((plain, torch.zeros(2, 3, 4, 4, 1)), (tiled, torch.zeros(2, 3, 6, 7, 1))):
        shape = ldm.get_batch_latent_shape(2)
        m, x = torch.ones(shape), torch.zeros(shape)
        for sampler in ("ddim", "dpmpp_2m", "dpmpp_2m_sde"):
            kw = dict(cond=zc, batch_size=2, return_decoded=False, sampler=sampler, ddim_steps=3, noise_tape=_NoTape())
            with pytest.raises(ValueError, match="hold_mask and hold_x0"):
                ldm.sample(hold_mask=m, **kw)
            with pytest.raises(ValueError, match="hold_mask and hold_x0"):
                ldm.sample(hold_x0=x, **kw)
            with pytest.raises(ValueError, match="hold_noise"):
                ldm.sample(hold_mask=m, hold_x0=x, hold_noise="new", **kw)
            with pytest.raises(ValueError, match="hold_x0 must be"):
                ldm.sample(hold_mask=m, hold_x0=x[:, :1], **kw)
            with pytest.raises(ValueError, match="hold_mask .* does not broadcast"):
                ldm.sample(hold_mask=torch.ones(3, 1, 1, 1, 1), hold_x0=x, **kw)
            with pytest.raises(NotImplementedError, match="inpainting"):         # the reference's keywords keep their refusal
                ldm.sample(mask=m, x0=x, **kw)
        with pytest.raises(NotImplementedError, match=r"ancestral.*mask / x0"):
            ldm.sample(cond=zc, batch_size=2, return_decoded=False, hold_mask=m, hold_x0=x, noise_tape=_NoTape())
        # rolling forecasts: out_len 2, horizon 5
        kw = dict(cond=zc, horizon=5, batch_size=2, return_decoded=False, sampler="ddim", ddim_steps=2, noise_tape=[_NoTape()] * 4)
        with pytest.raises(ValueError, match=r'overlap="hold" needs stride < out_len'):
            rollout_sample(ldm, overlap="hold", **dict(kw, noise_tape=[_NoTape()] * 3))
        with pytest.raises(ValueError, match="overlap must be"):
            rollout_sample(ldm, stride=1, overlap="blend", **kw)
        with pytest.raises(ValueError, match="hold_noise"):
            rollout_sample(ldm, stride=1, overlap="hold", hold_noise="new", **kw)
        with pytest.raises(NotImplementedError, match="hold_mask / hold_x0 are not defined for a rolling forecast"):
            rollout_sample(ldm, stride=1, overlap="hold", hold_mask=m, hold_x0=x, **kw)
        with pytest.raises(NotImplementedError, match="hold_mask / hold_x0 are not defined for a rolling forecast"):
            rollout_sample(ldm, stride=1, hold_x0=x, **kw)
        with pytest.raises(NotImplementedError, match='overlap="hold" is defined for'):
            rollout_sample(ldm, stride=1, overlap="hold", **dict(kw, sampler="ddpm"))
        with pytest.raises(NotImplementedError, match="mask"):
            rollout_sample(ldm, stride=1, overlap="hold", mask=m, x0=x, **kw)
    with pytest.raises(ValueError, match=r'overlap="hold" needs stride'):
        rollout_ensemble(plain, torch.zeros(1, 3, 4, 4, 1), 4, 5, overlap="hold")
    with pytest.raises(NotImplementedError, match="canvas"):
        tiled.hold_from_frames(torch.zeros(2, 1, 24, 28, 1))
    with pytest.raises(ValueError, match="frames must be"):
        plain.hold_from_frames(torch.zeros(2, 3, 8, 8, 1))                   # three frames into two target frames
    assert torch.equal(torch.get_rng_state(), rng)                           # refused before any draw


# ------------------------------------------------------------------------------------------------ 4. the rule on the mixture
@pytest.mark.parametrize("schedule", ["linear", "sqrt_linear"])
def test_hold_pulls_the_free_part_onto_the_held_component(schedule):
    """The analytic two-component mixture of _dpmpp_ref, d = 4096, B = 16, 3072 coordinates held at a draw m + 0.8 xi of component 1,
    hold_noise="fresh": the free quarter of EVERY sample lands on component 1 (proj > 0.7; measured over 8 seed pairs and six sampler
    settings on both schedules the worst was 0.756), where the un-held runs from the same x_T give both signs."""
    ac = _ac(schedule)
    for seed in (1, 2):
        means, M, X, x_T = H.mixture_problem(seed)
        mix = R.Mixture(np, means, R.MIXTURE_STDS)
        for sampler, eta, method in H.MIXTURE_SETTINGS:
            held = H.mixture_run(mix, ac, sampler, eta, method, x_T, M, X, 100 + seed)
            free = H.mixture_run(mix, ac, sampler, eta, method, x_T, None, None, 100 + seed)
            ph, pf = H.proj(held, means, M), H.proj(free, means, M)
            print(f"[mixture {schedule} seed {seed} {sampler} eta {eta} {method}] held proj min {ph.min():.3f}; un-held: {int((pf > 0).sum())} of "
                  f"{len(pf)} positive")
            assert np.array_equal(held[:, M == 1], X[:, M == 1])            # the last step writes the known part itself
            assert (ph > 0.7).all(), (seed, sampler, eta, method)
            assert (pf > 0).any() and (pf < 0).any(), (seed, sampler, eta, method)
