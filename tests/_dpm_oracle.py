"""Test oracle: DPM-Solver++ (multistep, orders 1 and 2, epsilon prediction) restated literally in float64, as a STATEFUL
``step(eps, i, x)`` with a list of model outputs — the shape of diffusers 0.25's ``DPMSolverMultistepScheduler.step`` — and not as a
coefficient table, so that it checks omg_amd.schedulers.dpm_coefficients rather than repeating it.  Plugs into
``oracle.pipeline.denoise`` (``timesteps``, ``init_noise_sigma``, ``scale_model_input(x, i)``, ``step(eps, i, x)``).

Schedule (the same recalled choices omg_amd.schedulers states; parity with diffusers is unpinned): "leading" spacing with
``ratio = n_train // (n + 1)``; without Karras sigmas sigma is interpolated at the timesteps and the final sigma is
``sigma(alphas_cumprod[0])``; with Karras sigmas (rho 7) the last sigma is repeated and the timesteps are the rounded log-sigma
interpolation.  A zero-length step (h = 0, the repeated Karras sigma) returns the sample: the limit of the formulas (the literal heun
form divides 0 by 0 there)."""
from __future__ import annotations

import numpy as np

from oracle.schedulers import alphas_cumprod


def dpm_sigmas(n: int, karras: bool = False, n_train: int = 1000, offset: int = 1):
    """(timesteps (n,), sigmas (n + 1,)) of the SDXL-base beta schedule"""
    ac = alphas_cumprod(n_train)
    sig = np.sqrt((1 - ac) / ac)
    ratio = n_train // (n + 1)
    ts = np.array([(n - i) * ratio + offset for i in range(n)], dtype=np.int64)
    if not karras:
        s = np.interp(ts.astype(np.float64), np.arange(n_train), sig)
        return ts, np.append(s, sig[0])
    rho = 7.0
    s = np.array([(sig[-1] ** (1 / rho) + k / max(n - 1, 1) * (sig[0] ** (1 / rho) - sig[-1] ** (1 / rho))) ** rho for k in range(n)])
    ts = np.round(np.interp(np.log(s), np.log(sig), np.arange(n_train))).astype(np.int64)
    return ts, np.append(s, s[-1])


class DPMSolverPP:
    init_noise_sigma = 1.0

    def __init__(self, n_steps: int, solver_order: int = 2, solver_type: str = "midpoint", lower_order_final: bool = True,
                 euler_at_final: bool = False, use_karras_sigmas: bool = False, sigmas=None):
        if sigmas is None:
            self.timesteps, self.sigmas = dpm_sigmas(n_steps, use_karras_sigmas)
        else:
            self.timesteps, self.sigmas = np.arange(n_steps)[::-1].copy(), np.asarray(sigmas, dtype=np.float64)
        self.n = n_steps
        self.solver_order, self.solver_type = solver_order, solver_type
        self.lower_order_final, self.euler_at_final = lower_order_final, euler_at_final
        self.model_outputs = []
        self.lower_order_nums = 0

    def scale_model_input(self, x, i):
        return x

    def _alpha_sigma(self, k):
        a = 1.0 / np.sqrt(self.sigmas[k] ** 2 + 1.0)
        return a, self.sigmas[k] * a

    def step(self, eps, i, x):
        if i == 0:
            self.model_outputs, self.lower_order_nums = [], 0
        alpha_s, sigma_s = self._alpha_sigma(i)
        x0 = (x - sigma_s * eps) / alpha_s                                      # convert_model_output, dpmsolver++
        self.model_outputs = (self.model_outputs + [x0])[-self.solver_order:]
        final = i == self.n - 1 and (self.euler_at_final or (self.lower_order_final and self.n < 15))
        order = 1 if (self.solver_order == 1 or self.lower_order_nums < 1 or final) else 2
        alpha_t, sigma_t = self._alpha_sigma(i + 1)
        lambda_t, lambda_s0 = np.log(alpha_t) - np.log(sigma_t), np.log(alpha_s) - np.log(sigma_s)
        h = lambda_t - lambda_s0
        if h == 0.0:
            out = x
        elif order == 1:                                                        # dpm_solver_first_order_update
            out = (sigma_t / sigma_s) * x - alpha_t * (np.exp(-h) - 1.0) * x0
        else:                                                                   # multistep_dpm_solver_second_order_update
            m0, m1 = self.model_outputs[-1], self.model_outputs[-2]
            alpha_s1, sigma_s1 = self._alpha_sigma(i - 1)
            h_0 = lambda_s0 - (np.log(alpha_s1) - np.log(sigma_s1))
            r0 = h_0 / h
            D0, D1 = m0, (1.0 / r0) * (m0 - m1)
            if self.solver_type == "midpoint":
                out = (sigma_t / sigma_s) * x - alpha_t * (np.exp(-h) - 1.0) * D0 - 0.5 * alpha_t * (np.exp(-h) - 1.0) * D1
            else:
                out = (sigma_t / sigma_s) * x - alpha_t * (np.exp(-h) - 1.0) * D0 + alpha_t * ((np.exp(-h) - 1.0) / h + 1.0) * D1
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        return out
