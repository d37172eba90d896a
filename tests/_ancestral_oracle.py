"""Test oracle: the two stochastic steps restated literally in float64 — Euler-ancestral (diffusers 0.25's
``EulerAncestralDiscreteScheduler.step``) and DDIM with eta > 0 (``DDIMScheduler.step`` with its ``_get_variance``) — as STATEFUL objects with
the interface of ``oracle.pipeline.denoise`` (``timesteps``, ``init_noise_sigma``, ``scale_model_input(x, i)``, ``step(eps, i, x)``).
``oracle/`` is not changed for them.

They hold the pre-drawn noise of every step (``noise[i]``: (2, C, H, W)) and add ``std * noise[i]`` as diffusers does: sigma_up / sigma_down
and the DDIM variance are written out step by step, not taken from a coefficient table, so that they check
``omg_amd.schedulers``' tables rather than repeat them.  The schedule is the SDXL-base one of ``oracle.schedulers`` ("leading" spacing,
steps_offset 1).  Parity with diffusers is unpinned (the formulas are recalled, as stated in omg_amd/schedulers.py).

``draws`` reproduces the engine's noise contract: from a fresh generator, the initial latents, then one (2, C, H, W) float32 draw per step."""
from __future__ import annotations

import numpy as np
import torch

from oracle.schedulers import alphas_cumprod, leading_timesteps


def draws(seed: int, device, latent_shape, n_steps: int, latents: bool = True):
    """(latents (1, C, H, W), [z_0 .. z_{S-1}] each (2, C, H, W) float64 numpy) as the engine draws them from
    ``torch.Generator(device).manual_seed(seed)``; the latents are NOT yet multiplied by init_noise_sigma.  ``latents=False``: a call that
    was given its latents draws the noise only (the first element is then None)."""
    g = torch.Generator(device).manual_seed(seed)
    lat = torch.randn(tuple(latent_shape), generator=g, device=device, dtype=torch.float32).cpu() if latents else None
    zs = [torch.randn((2,) + tuple(latent_shape[1:]), generator=g, device=device, dtype=torch.float32).cpu().double().numpy()
          for _ in range(n_steps)]
    return lat, zs


class EulerAncestral:
    def __init__(self, n_steps: int, noise, n_train: int = 1000):
        ac = alphas_cumprod(n_train)
        sig = ((1 - ac) / ac) ** 0.5
        self.timesteps = leading_timesteps(n_steps, n_train).astype(np.float64)
        s = np.interp(self.timesteps, np.arange(n_train), sig)
        self.sigmas = np.concatenate([s, [0.0]])
        self.init_noise_sigma = float((self.sigmas.max() ** 2 + 1) ** 0.5)   # "leading" spacing
        self.noise = noise

    def scale_model_input(self, x, i):
        return x / (self.sigmas[i] ** 2 + 1) ** 0.5

    def step(self, eps, i, x):
        sigma = self.sigmas[i]
        pred_original_sample = x - sigma * eps                                 # epsilon prediction
        sigma_from, sigma_to = self.sigmas[i], self.sigmas[i + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        derivative = (x - pred_original_sample) / sigma
        dt = sigma_down - sigma
        prev_sample = x + derivative * dt
        return prev_sample + self.noise[i] * sigma_up


class DDIMEta:
    init_noise_sigma = 1.0

    def __init__(self, n_steps: int, eta: float, noise, n_train: int = 1000):
        self.ac = alphas_cumprod(n_train)
        self.final_alpha = self.ac[0]          # set_alpha_to_one = False
        self.timesteps = leading_timesteps(n_steps, n_train)
        self.ratio = n_train // n_steps
        self.eta = eta
        self.noise = noise

    def scale_model_input(self, x, i):
        return x

    def variance(self, i):
        t = int(self.timesteps[i])
        prev = t - self.ratio
        a_t = self.ac[t]
        a_p = self.ac[prev] if prev >= 0 else self.final_alpha
        beta_t, beta_p = 1 - a_t, 1 - a_p
        return (beta_p / beta_t) * (1 - a_t / a_p)

    def step(self, eps, i, x):
        t = int(self.timesteps[i])
        prev = t - self.ratio
        a_t = self.ac[t]
        a_p = self.ac[prev] if prev >= 0 else self.final_alpha
        pred_original_sample = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
        std_dev_t = self.eta * self.variance(i) ** 0.5
        pred_sample_direction = (1 - a_p - std_dev_t ** 2) ** 0.5 * eps
        prev_sample = a_p ** 0.5 * pred_original_sample + pred_sample_direction
        if self.eta > 0:
            prev_sample = prev_sample + std_dev_t * self.noise[i]
        return prev_sample
