"""Diffusion schedules (host side, float64 -> fp32 tables), same functions as the reference's
``prediff.diffusion.utils`` (make_beta_schedule :17-39, make_ddim_timesteps :42-56,
make_ddim_sampling_parameters :59-70) and ``LatentDiffusion.register_schedule`` (latent_diffusion.py:228-268)."""
from typing import Dict

import numpy as np


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3) -> np.ndarray:
    # config files written for OmegaConf carry "1e-4"-style scalars that plain YAML loaders return as str
    linear_start, linear_end, cosine_s = float(linear_start), float(linear_end), float(cosine_s)
    if schedule == "linear":
        betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2
    elif schedule == "cosine":
        ts = np.arange(n_timestep + 1, dtype=np.float64) / n_timestep + cosine_s
        alphas = np.cos(ts / (1 + cosine_s) * np.pi / 2) ** 2
        alphas = alphas / alphas[0]
        betas = np.clip(1 - alphas[1:] / alphas[:-1], a_min=0, a_max=0.999)
    elif schedule == "sqrt_linear":
        betas = np.linspace(linear_start, linear_end, n_timestep, dtype=np.float64)
    elif schedule == "sqrt":
        betas = np.linspace(linear_start, linear_end, n_timestep, dtype=np.float64) ** 0.5
    else:
        raise ValueError(f"schedule '{schedule}' unknown.")
    return betas


def schedule_tables(betas: np.ndarray, v_posterior: float = 0.0) -> Dict[str, np.ndarray]:
    """The 12 per-timestep buffers LatentDiffusion registers (float64 math, cast to fp32 last)."""
    betas = np.asarray(betas, dtype=np.float64)
    alphas = 1.0 - betas
    ac = np.cumprod(alphas, axis=0)
    ac_prev = np.append(1.0, ac[:-1])
    post_var = (1 - v_posterior) * betas * (1.0 - ac_prev) / (1.0 - ac) + v_posterior * betas
    t = {
        "betas": betas,
        "alphas_cumprod": ac,
        "alphas_cumprod_prev": ac_prev,
        "sqrt_alphas_cumprod": np.sqrt(ac),
        "sqrt_one_minus_alphas_cumprod": np.sqrt(1.0 - ac),
        "log_one_minus_alphas_cumprod": np.log(1.0 - ac),
        "sqrt_recip_alphas_cumprod": np.sqrt(1.0 / ac),
        "sqrt_recipm1_alphas_cumprod": np.sqrt(1.0 / ac - 1),
        "posterior_variance": post_var,
        "posterior_log_variance_clipped": np.log(np.maximum(post_var, 1e-20)),
        "posterior_mean_coef1": betas * np.sqrt(ac_prev) / (1.0 - ac),
        "posterior_mean_coef2": (1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac),
    }
    return {k: v.astype(np.float32) for k, v in t.items()}


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=False) -> np.ndarray:
    """The DDPM indices a DDIM run visits, each shifted up by one (so that the last one reaches the final alpha).  `verbose` is
    accepted for signature compatibility and ignored."""
    T, S = int(num_ddpm_timesteps), int(num_ddim_timesteps)
    if ddim_discr_method == "uniform":
        picked = np.arange(0, T, T // S)                          # every (T // S)-th training step
    elif ddim_discr_method == "quad":
        picked = np.square(np.linspace(0.0, np.sqrt(0.8 * T), S)).astype(int)   # quadratic spacing over the first 80 %
    else:
        raise NotImplementedError(f"unknown ddim discretization method '{ddim_discr_method}' (uniform | quad)")
    return picked + 1


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=False):
    """(sigma_t, alpha_bar_t, alpha_bar_{t-1}) on the DDIM grid; the step before the first grid point is training step 0."""
    ac = np.asarray(alphacums)
    steps = np.asarray(ddim_timesteps)
    a_t = ac[steps]
    a_before = np.concatenate([ac[:1], ac[steps[:-1]]])
    sigma = eta * np.sqrt((1 - a_before) / (1 - a_t) * (1 - a_t / a_before))
    return sigma, a_t, a_before


def _half_logsnr(a):
    """lambda = log(alpha / sigma) = 0.5 * log(a / (1 - a)) of a cumulative alpha."""
    a = np.asarray(a, dtype=np.float64)
    return 0.5 * np.log(a / (1.0 - a))


def make_logsnr_timesteps(num_steps, alphacums) -> np.ndarray:
    """`num_steps` grid points (DDPM indices, ascending, unique, the last one T-1) for the multistep solver: the timesteps nearest in
    lambda to levels evenly spaced in lambda between training steps T-1 and 0.  Step 0 itself is the last step's target (the
    convention of make_ddim_sampling_parameters), so it is not a grid point."""
    lam = _half_logsnr(np.asarray(alphacums, dtype=np.float32).astype(np.float64))       # decreasing in t
    T, S = lam.shape[0], int(num_steps)
    if not (1 <= S <= T - 1):
        raise ValueError(f"num_steps must be in [1, {T - 1}], got {num_steps}")
    levels = np.linspace(lam[0], lam[T - 1], S + 1)[1:]
    hi = np.clip(np.searchsorted(-lam, -levels), 1, T - 1)                              # lam[hi - 1] >= level >= lam[hi]
    steps = np.where(np.abs(lam[hi - 1] - levels) <= np.abs(lam[hi] - levels), hi - 1, hi)
    for i in range(S - 2, -1, -1):        # a schedule too flat in lambda for the count: the nearest timesteps that are still distinct
        steps[i] = min(steps[i], steps[i + 1] - 1)
    steps[0] = max(steps[0], 1)
    for i in range(1, S):
        steps[i] = max(steps[i], steps[i - 1] + 1)
    return steps.astype(np.int64)


def _dpmpp_2m_visits(alphacums, timesteps, lower_order_final):
    """(a, a_prev, h, w, visited) of the multistep solvers in fp64, in visiting order: the grid of make_ddim_sampling_parameters without
    the points whose a_prev == a, h_k = lambda(a_prev) - lambda(a), w_k = h_{k-1} / (2 h_k) with w_0 = 0 and, with `lower_order_final`
    (default: fewer than 15 visited steps), w_last = 0."""
    _, a, a_prev = make_ddim_sampling_parameters(np.asarray(alphacums, dtype=np.float64), timesteps, 0.0)
    visited = np.asarray([idx for idx in reversed(range(len(a))) if a_prev[idx] != a[idx]], dtype=np.int64)
    a, a_prev = a[visited], a_prev[visited]
    h = _half_logsnr(a_prev) - _half_logsnr(a)
    w = np.zeros_like(h)
    w[1:] = h[:-1] / (2.0 * h[1:])
    if lower_order_final is None:
        lower_order_final = len(visited) < 15
    if lower_order_final and len(w):
        w[-1] = 0.0
    return a, a_prev, h, w, visited


def make_dpmpp_2m_coefficients(alphacums, timesteps, lower_order_final=None):
    """DPM-Solver++(2M), data prediction (Lu et al. 2022, arXiv:2211.01095, algorithm 2), on the grid of make_ddim_sampling_parameters:
    a = alphacums[timesteps[idx]], a_prev = the grid point before it (alphacums[0] for idx = 0).  With alpha = sqrt(a),
    sigma = sqrt(1 - a), lambda = log(alpha / sigma), the k-th VISITED step (k = 0 is the largest timestep) is
        h_k = lambda(a_prev) - lambda(a);  x0 = (z - sigma eps) / alpha;  D = x0 + w_k (x0 - x0_prev);  w_k = h_{k-1} / (2 h_k)
        z_prev = (sigma_prev / sigma) z - alpha_prev expm1(-h_k) D
    w_k = 0 on the first visited step, and on the last one with `lower_order_final` (default: fewer than 15 visited steps, as in the
    published solver).  A grid point with a_prev == a (quad's repeated integers, the T-1 clamp) is the identity for an ODE solver
    (h = 0): it is dropped from the visit list and never enters h_{k-1}.
    Returns (table, visited): table[k] = (a, c_x, c_d, w_k) with c_x = sigma_prev / sigma and c_d = -alpha_prev expm1(-h_k), fp64
    from the alphacums as given, rounded to fp32 once; visited[k] = the grid index idx of the k-th visited step."""
    a, a_prev, h, w, visited = _dpmpp_2m_visits(alphacums, timesteps, lower_order_final)
    c_x = np.sqrt((1.0 - a_prev) / (1.0 - a))
    c_d = -np.sqrt(a_prev) * np.expm1(-h)
    return np.stack([a, c_x, c_d, w], axis=1).astype(np.float32), visited


def make_dpmpp_2m_sde_coefficients(alphacums, timesteps, eta, lower_order_final=None):
    """SDE-DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095) with the eta-generalisation in common use, midpoint form, on the grid,
    the visit list and the h_k, w_k of make_dpmpp_2m_coefficients.  With unit noise n per visited step:
        x0 = (z - sigma eps) / alpha;  D = x0 + w_k (x0 - x0_prev)
        z_prev = (sigma_prev / sigma) exp(-eta h_k) z - alpha_prev expm1(-(1 + eta) h_k) D + sigma_prev sqrt(-expm1(-2 eta h_k)) n
    eta = 0 is make_dpmpp_2m_coefficients' row element for element with c_n = 0; eta = 1 with w = 0 is the DDIM step at the sigma of
    make_ddim_sampling_parameters(eta=1), the ancestral posterior on the grid.
    Returns (table, visited): table[k] = (a, c_x, c_d, w_k, c_n), fp64 from the alphacums as given, rounded to fp32 once."""
    eta = float(eta)
    if not eta >= 0.0:
        raise ValueError(f"eta must be >= 0, got {eta}")
    a, a_prev, h, w, visited = _dpmpp_2m_visits(alphacums, timesteps, lower_order_final)
    c_x = np.sqrt((1.0 - a_prev) / (1.0 - a)) * np.exp(-eta * h)
    c_d = -np.sqrt(a_prev) * np.expm1(-(1.0 + eta) * h)
    c_n = np.sqrt(1.0 - a_prev) * np.sqrt(-np.expm1(-2.0 * eta * h))
    return np.stack([a, c_x, c_d, w, c_n], axis=1).astype(np.float32), visited


def make_hold_coefficients(alphacums, timesteps, visited=None):
    """The hold columns of a held-region run ("Held regions") on the grid of make_ddim_sampling_parameters.  `visited`:
    the grid indices in visiting order (default: every grid point from the last to the first, DDIM's order; the 2M loops pass the
    visit list of make_dpmpp_2m_coefficients).  After visited step k the held part is the known latent at the level the denoiser
    sees next: u_k = a_prev of step k, and u = 1 after the last step, which writes the known latent itself.
    Returns (cols, start): cols[k] = (sqrt(u_k), sqrt(1 - u_k)), the last row exactly (1, 0); start = (sqrt(a_0), sqrt(1 - a_0)) with
    a_0 the level the first step reads.  fp64 from the alphacums as given, rounded to fp32 once."""
    _, a, a_prev = make_ddim_sampling_parameters(np.asarray(alphacums, dtype=np.float64), timesteps, 0.0)
    visited = np.arange(len(a) - 1, -1, -1) if visited is None else np.asarray(visited, dtype=np.int64)
    if len(visited) == 0:
        raise ValueError("a held run needs at least one visited step")
    u = np.append(a_prev[visited[:-1]], 1.0)
    a0 = a[visited[0]]
    return (np.stack([np.sqrt(u), np.sqrt(1.0 - u)], axis=1).astype(np.float32),
            np.asarray([np.sqrt(a0), np.sqrt(1.0 - a0)]).astype(np.float32))


def make_ddim_guidance_coefficients(posterior_log_variance_clipped, ddim_timesteps) -> np.ndarray:
    """gamma per DDIM step of the knowledge-aligned DDIM sampler: step idx moves from t = steps[idx] to the alpha of
    steps[idx-1] and skips the DDPM timesteps J_idx = {steps[idx-1] + 1, ..., steps[idx]} ({0, ..., steps[0]} for idx = 0); it
    subtracts gamma_idx * g with gamma_idx = sum over J_idx of exp(0.5 * logvar_clipped[j]), the mean shifts the reference's aligned
    ancestral chain applies over those timesteps.  A repeated grid point (quad's integer rounding, the T-1 clamp) has an empty J and
    gamma 0.  fp64 from the fp32 buffer, one rounding to fp32 at the end."""
    sd = np.exp(0.5 * np.asarray(posterior_log_variance_clipped, dtype=np.float32).astype(np.float64))
    steps = np.asarray(ddim_timesteps, dtype=np.int64)
    gamma = np.zeros(len(steps), dtype=np.float64)
    lo = 0
    for idx, t in enumerate(steps):
        gamma[idx] = sd[lo:t + 1].sum()          # empty when t < lo
        lo = max(lo, int(t) + 1)
    return gamma.astype(np.float32)
