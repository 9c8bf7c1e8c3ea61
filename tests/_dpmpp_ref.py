"""CPU restatement (torch / numpy, fp64) of the DPM-Solver++(2M) sampler, written from the formulas of DESIGN.md §7 and independent of
prediff_amd.schedule: the grid comes from oracle.diffusion's DDIM helpers, everything else is spelled out step by step.

    a = ac[steps[idx]], a_prev = ac[steps[idx-1]] (ac[0] for idx = 0);  alpha = sqrt(a), sigma = sqrt(1-a), lam = log(alpha / sigma)
    visited steps: idx = n-1 .. 0 without the grid points whose a_prev == a
    h_k = lam(a_prev) - lam(a);  x0 = (z - sigma eps) / alpha;  D = x0 + w_k (x0 - x0_prev);  w_k = h_{k-1} / (2 h_k)
    z_prev = (sigma_prev / sigma) z - alpha_prev expm1(-h_k) D
    w_0 = 0; w_last = 0 with lower_order_final (default: fewer than 15 visited steps)

Also here: the analytic two-component Gaussian-mixture denoiser of the convergence tests, for any array module (numpy fp64 on the CPU,
torch fp32 on the device)."""
import math

import numpy as np
import torch

from oracle import diffusion as OD


def lam(a):
    return 0.5 * math.log(a / (1.0 - a))


def logsnr_grid(n, ac):
    """n timesteps nearest (in lam) to n + 1 levels evenly spaced in lam from t = 0 to t = T-1, without the level of t = 0."""
    lams = [lam(float(a)) for a in ac]
    out = []
    for j in range(1, n + 1):
        level = lams[0] + (lams[-1] - lams[0]) * j / n
        out.append(min(range(1, len(lams)), key=lambda t: abs(lams[t] - level)))
    return np.asarray(out, dtype=np.int64)


def grid(n, ac, method):
    """The grid of a run of n steps over the fp32 alphas_cumprod `ac`: oracle.diffusion's DDIM grid (clipped to T-1) or the lam grid."""
    T = len(ac)
    return logsnr_grid(n, ac) if method == "logsnr" else np.minimum(OD.ddim_timesteps(n, T, method), T - 1)


def visits(ac, steps, lower_order_final=None):
    """Per visited step, in visiting order: dict(idx, t, a, a_prev, h, w) in Python floats (fp64)."""
    ac = np.asarray(ac, dtype=np.float32).astype(np.float64)
    _, a, a_prev = OD.ddim_sampling_parameters(ac, np.asarray(steps), 0.0)
    out = []
    for idx in reversed(range(len(steps))):
        if a_prev[idx] == a[idx]:
            continue
        h = lam(float(a_prev[idx])) - lam(float(a[idx]))
        w = out[-1]["h"] / (2.0 * h) if out else 0.0
        out.append(dict(idx=idx, t=int(steps[idx]), a=float(a[idx]), a_prev=float(a_prev[idx]), h=h, w=w))
    if lower_order_final is None:
        lower_order_final = len(out) < 15
    if lower_order_final and out:
        out[-1]["w"] = 0.0
    return out


def bound_factor(vs):
    """1 + 2 max_k w_k: the extrapolation D = (1 + w) x0 - w x0_prev has coefficients whose absolute values sum to 1 + 2 w, so an
    error of size e in each denoiser output enters a step at most (1 + 2 w) e where the first-order step lets in e."""
    return 1.0 + 2.0 * max(v["w"] for v in vs)


def step(z, eps, x0_prev, v):
    """One step in fp64: (z_prev, x0).  x0_prev is not touched where w = 0."""
    z, eps = z.double(), eps.double()
    alpha, sigma = math.sqrt(v["a"]), math.sqrt(1.0 - v["a"])
    alpha_prev, sigma_prev = math.sqrt(v["a_prev"]), math.sqrt(1.0 - v["a_prev"])
    x0 = (z - sigma * eps) / alpha
    D = x0 + v["w"] * (x0 - x0_prev.double()) if v["w"] != 0.0 else x0
    return (sigma_prev / sigma) * z - alpha_prev * math.expm1(-v["h"]) * D, x0


def gamma_f64(logvar_clipped, steps):
    """The guidance rule of DESIGN.md §7 restated: gamma_idx = sum over J_idx = {steps[idx-1]+1 .. steps[idx]} ({0 .. steps[0]} for
    idx = 0) of exp(0.5 logvar_clipped[j]), rounded to fp32 once."""
    lv = np.asarray(logvar_clipped, dtype=np.float32).astype(np.float64)
    out = []
    for idx, t in enumerate(steps):
        lo = 0 if idx == 0 else int(steps[idx - 1]) + 1
        out.append(float(np.float32(sum(math.exp(0.5 * lv[j]) for j in range(lo, int(t) + 1)))))
    return out


def sample_loop(ac, denoiser, zc, x_T, n, method="quad", lower_order_final=None, align_fn=None, logvar_clipped=None):
    """The sampler: fp64 state, the denoiser (and the alignment function) called on the fp32 rounding of it, as the engine's see it.
    align_fn(z, t) -> shift: the guided form, z_prev -= gamma_idx * shift."""
    steps = grid(n, ac, method)
    vs = visits(ac, steps, lower_order_final)
    gamma = gamma_f64(logvar_clipped, steps) if align_fn is not None else None
    z, x0_prev = x_T.double(), None
    B = z.shape[0]
    for v in vs:
        t = torch.full((B,), v["t"], dtype=torch.long)
        with torch.no_grad():
            eps = denoiser(z.float(), t, zc)
        shift = align_fn(z.float(), t).detach() if align_fn is not None else None
        z, x0_prev = step(z, eps, x0_prev, v)
        if shift is not None:
            z = z - gamma[v["idx"]] * shift.double()
    return z


# ---------------------------------------------------------------------------------------------- the analytic denoiser
class Mixture:
    """x0 ~ 1/2 N(m1, s1^2 I) + 1/2 N(m2, s2^2 I) in d dimensions.  At level a, z ~ sum_i 1/2 N(alpha m_i, v_i I) with
    v_i = a s_i^2 + 1 - a, and eps(z, a) = -sigma * score = sigma * sum_i r_i(z) (z - alpha m_i) / v_i with the posterior weights r_i.
    `xp` is numpy or torch; `means` (2, d) and arrays passed to eps() are of that module."""

    def __init__(self, xp, means, stds):
        self.xp, self.means, self.stds = xp, means, stds

    def eps(self, z, a):
        xp = self.xp
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        d = z.shape[-1]
        logit, pull = [], []
        for m, s in zip(self.means, self.stds):
            v = a * s * s + 1.0 - a
            r = z - alpha * m
            logit.append(-0.5 * (r * r).sum(-1, keepdims=True) / v - 0.5 * d * math.log(v))
            pull.append(r / v)
        top = xp.maximum(logit[0], logit[1])
        e0, e1 = xp.exp(logit[0] - top), xp.exp(logit[1] - top)
        return sigma * (e0 * pull[0] + e1 * pull[1]) / (e0 + e1)


def mixture_means(d=4096, seed=5):
    """Means +m and -m with |m_j| = 0.6 and random signs; with both stds 0.8 every coordinate of x0 has variance 0.36 + 0.64 = 1, the
    scale the engine's latents are normalised to (scale_factor)."""
    m = 0.6 * np.sign(np.random.default_rng(seed).standard_normal(d))
    return np.stack([m, -m])


MIXTURE_STDS = (0.8, 0.8)


def ac_convergence(T=1000):
    """alphas_cumprod (fp32) of the convergence tests: the project's "sqrt_linear" beta schedule from 1e-4 to 2e-2."""
    return np.cumprod(1.0 - OD.beta_schedule("sqrt_linear", T, linear_start=1e-4, linear_end=2e-2)).astype(np.float32)
