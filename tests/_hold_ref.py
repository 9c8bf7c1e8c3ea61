"""CPU restatement (fp64) of held-region sampling, written from the rule of DESIGN.md §7 ("Held regions") and independent of
prediff_amd.schedule: the un-held steps are oracle.diffusion's DDIM step and _dpmpp_ref's 2M step, the hold is spelled out here.

    visited steps k = 0 .. K-1; a_k the level step k reads, a_prev_k the level it produces; M the mask (1 = held), X the known latent
    start :  z <- M (sqrt(a_0) X + sqrt(1 - a_0) x_T) + (1 - M) x_T
    step k:  v = the sampler's step;  u_k = a_prev_k for k < K-1, 1 for k = K-1;  z <- M (sqrt(u_k) X + sqrt(1 - u_k) h_k) + (1 - M) v
    h_k: "fresh" a new unit-normal draw per step k < K-1, "fixed" x_T
    tape, read strictly in order: x_T, then per step its own draw n_k (DDIM always; 2M-SDE when eta > 0; 2M never) followed by h_k
    ("fresh", k < K-1): DDIM [x_T, n_0, h_0, ..., n_{K-1}], 2M [x_T, h_0, ..., h_{K-2}]; "fixed" reads what the un-held run reads.
"""
import math

import numpy as np
import torch

import _dpmpp_ref as R
from oracle import diffusion as OD


def ddim_visits(ac, steps, eta):
    """DDIM's visited steps in visiting order (every grid point, the last first): dict(idx, t, a, a_prev, sigma), fp64."""
    ac = np.asarray(ac, dtype=np.float32).astype(np.float64)
    sig, a, a_prev = OD.ddim_sampling_parameters(ac, np.asarray(steps), eta)
    return [dict(idx=idx, t=int(steps[idx]), a=float(a[idx]), a_prev=float(a_prev[idx]), sigma=float(sig[idx]))
            for idx in reversed(range(len(steps)))]


def hold_levels(vs):
    """u_k of a visit list: a_prev_k, and 1 for the last step."""
    return [v["a_prev"] for v in vs[:-1]] + [1.0]


def hold_columns(vs):
    """((sqrt(u_k), sqrt(1 - u_k)) per visited step, (sqrt(a_0), sqrt(1 - a_0)))"""
    return [(math.sqrt(u), math.sqrt(1.0 - u)) for u in hold_levels(vs)], (math.sqrt(vs[0]["a"]), math.sqrt(1.0 - vs[0]["a"]))


def blend(v, M, X, h, u):
    """M (sqrt(u) X + sqrt(1 - u) h) + (1 - M) v; h is not touched where u = 1.  Works on torch and numpy arrays."""
    held = math.sqrt(u) * X
    if u != 1.0:
        held = held + math.sqrt(1.0 - u) * h
    return M * held + (1.0 - M) * v


def sde_step(z, eps, x0_prev, v, eta, noise):
    """One SDE-DPM-Solver++(2M) step in fp64: (z_prev, x0)."""
    z, eps = z.double(), eps.double()
    alpha, sigma = math.sqrt(v["a"]), math.sqrt(1.0 - v["a"])
    alpha_prev, sigma_prev = math.sqrt(v["a_prev"]), math.sqrt(1.0 - v["a_prev"])
    h = v["h"]
    x0 = (z - sigma * eps) / alpha
    D = x0 + v["w"] * (x0 - x0_prev.double()) if v["w"] != 0.0 else x0
    out = (sigma_prev / sigma) * math.exp(-eta * h) * z - alpha_prev * math.expm1(-(1.0 + eta) * h) * D
    if eta > 0:
        out = out + sigma_prev * math.sqrt(-math.expm1(-2.0 * eta * h)) * noise.double()
    return out, x0


def reads_own_draw(sampler, eta):
    return sampler == "ddim" or (sampler == "dpmpp_2m_sde" and eta > 0)


def tape_layout(sampler, eta, K, hold_noise):
    """The names of the tape entries a run of K visited steps reads, in order."""
    out = ["x_T"]
    for k in range(K):
        if reads_own_draw(sampler, eta):
            out.append(f"n{k}")
        if hold_noise == "fresh" and k < K - 1:
            out.append(f"h{k}")
    return out


def held_loop(ac, denoiser, zc, tape, n, sampler, M, X, hold_noise="fresh", eta=0.0, method=None, lower_order_final=None, align_fn=None,
              logvar_clipped=None):
    """The held sampler: fp64 state, the denoiser (and the alignment function) called on the fp32 rounding of the BLENDED latent.
    M = None: the un-held run on the same tape layout as hold_noise="fixed".  DDIM runs on the uniform grid (what sample() gives it),
    the 2M loops on `method` (default "quad").  Returns the final latent (fp64)."""
    if sampler == "ddim":
        steps = R.grid(n, ac, "uniform")
        vs = ddim_visits(ac, steps, eta)
    else:
        steps = R.grid(n, ac, method or "quad")
        vs = R.visits(ac, steps, lower_order_final)
    gamma = R.gamma_f64(logvar_clipped, steps) if align_fn is not None else None
    us = hold_levels(vs)
    pos = [0]

    def read():
        pos[0] += 1
        return tape[pos[0] - 1].double()
    x_T = read()
    z = x_T if M is None else blend(x_T, M.double(), X.double(), x_T, vs[0]["a"])
    x0_prev, B = None, x_T.shape[0]
    for k, v in enumerate(vs):
        t = torch.full((B,), v["t"], dtype=torch.long)
        with torch.no_grad():
            eps = denoiser(z.float(), t, zc)
        shift = align_fn(z.float(), t).detach() if align_fn is not None else None
        noise = read() if reads_own_draw(sampler, eta) else None
        if sampler == "ddim":
            f = lambda s: torch.full((B,), s, dtype=torch.float64)
            z = OD.ddim_step(z, eps.double(), f(v["a"]), f(v["a_prev"]), f(v["sigma"]), noise)
        elif sampler == "dpmpp_2m":
            z, x0_prev = R.step(z, eps, x0_prev, v)
        else:
            z, x0_prev = sde_step(z, eps, x0_prev, v, eta, noise)
        if shift is not None:
            z = z - gamma[v["idx"]] * shift.double()
        if M is not None:
            h = None
            if k < len(vs) - 1:
                h = read() if hold_noise == "fresh" else x_T
            z = blend(z, M.double(), X.double(), h, us[k])
    return z


# ---------------------------------------------------------------------------------------------- the mixture property
D_MIX, HELD_MIX, B_MIX = 4096, 3072, 16


def mixture_problem(seed):
    """The analytic mixture of _dpmpp_ref (means +m / -m, stds 0.8) with the first HELD_MIX coordinates held at a draw of component 1:
    (means (2, d), M (d,), X (B, d), x_T (B, d)) in numpy fp64; X is zero on the free coordinates."""
    means = R.mixture_means(D_MIX)
    rng = np.random.default_rng(seed)
    M = np.zeros(D_MIX)
    M[:HELD_MIX] = 1.0
    X = (means[0] + 0.8 * rng.standard_normal((B_MIX, D_MIX))) * M
    x_T = rng.standard_normal((B_MIX, D_MIX))
    return means, M, X, x_T


def mixture_visits(ac, sampler, eta, method, n=10):
    if sampler == "ddim":
        return ddim_visits(ac, R.grid(n, ac, "uniform"), eta)
    return R.visits(ac, R.grid(n, ac, method))


def mixture_run(mix, ac, sampler, eta, method, x_T, M, X, seed, n=10):
    """The held loop ("fresh") on the analytic denoiser in numpy fp64; M = None: the un-held run from the same x_T and step draws."""
    rng = np.random.default_rng(seed)
    vs = mixture_visits(ac, sampler, eta, method, n)
    us = hold_levels(vs)
    z = x_T if M is None else blend(x_T, M, X, x_T, vs[0]["a"])
    x0_prev = None
    for k, v in enumerate(vs):
        e = mix.eps(z, v["a"])
        noise = rng.standard_normal(x_T.shape)          # drawn for every sampler, so that held and un-held runs share their draws
        h = rng.standard_normal(x_T.shape)
        if sampler == "ddim":
            x0 = (z - math.sqrt(1 - v["a"]) * e) / math.sqrt(v["a"])
            z = math.sqrt(v["a_prev"]) * x0 + math.sqrt(max(0.0, 1 - v["a_prev"] - v["sigma"] ** 2)) * e + v["sigma"] * noise
        else:
            x0 = (z - math.sqrt(1 - v["a"]) * e) / math.sqrt(v["a"])
            D = x0 + v["w"] * (x0 - x0_prev) if v["w"] != 0.0 else x0
            z = math.sqrt(1 - v["a_prev"]) / math.sqrt(1 - v["a"]) * z - math.sqrt(v["a_prev"]) * math.expm1(-v["h"]) * D
            x0_prev = x0
        if M is not None:
            z = blend(z, M, X, h, us[k])
    return z


def proj(z, means, M):
    """Per sample: the mean over the free coordinates of z * m, over 0.36 (= |m_j|^2): +1 on component 1, -1 on component 2."""
    free = M == 0
    return (z[:, free] * means[0][free]).mean(axis=1) / 0.36


MIXTURE_SETTINGS = [("ddim", 0.0, "uniform"), ("ddim", 1.0, "uniform"), ("dpmpp_2m", 0.0, "uniform"), ("dpmpp_2m", 0.0, "quad")]
