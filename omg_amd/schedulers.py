"""DDIM and Euler-discrete schedules for the SDXL-base scheduler config, exported as per-step
coefficient tables for the fused step kernel (``omg_fuse_cfg_step``).

Replaces ``self.scheduler.set_timesteps / scale_model_input / step`` of the reference loop
(/root/reference src/pipelines/lora_pipeline.py:390-392, :492, :615; third-party
``diffusers==0.25.0`` ``scheduling_ddim`` / ``scheduling_euler_discrete``).  For epsilon prediction
with eta = 0 both updates are linear in (sample, eps):

    sample' = cx[i] * sample + ce[i] * eps ,   model_input = cin[i] * sample

  DDIM : cx = sqrt(a_prev / a_t), ce = sqrt(1 - a_prev) - sqrt(a_prev (1 - a_t) / a_t), cin = 1
  Euler: cx = 1,                  ce = sigma[i+1] - sigma[i],                       cin = 1/sqrt(sigma[i]^2 + 1)

so the whole scheduler is a (n_steps, 4) fp32 table resident in HBM: row i = (cx_i, ce_i, cin_{i+1}, 0).
The kernel indexes it with a device-side step counter, which is what makes the loop capturable
as a hipGraph (no host read of ``t``).  Tables are computed in float64 on the host once.

BASELINE.json names DDIM; the reference never sets a scheduler, so a stock SDXL-base checkpoint
would run Euler — both are provided, DDIM is the benchmark default.

DPM-Solver++ (``DPMSolverMultistepScheduler``, the InstantID scripts' import) is not a one-step map: order 2 also reads the previous
step's data prediction.  It exports an (n_steps, 8) table (:func:`dpm_coefficients`) for ``omg_fuse_cfg_step_ms``, which keeps that
prediction in a device history buffer; see the class for the algorithm and the schedule choices it makes.

Stochastic steps (``EulerAncestralDiscreteScheduler``; ``DDIMScheduler`` with eta > 0) are the same one-step map plus cz[i] * z_i, z_i
fresh Gaussian noise the host draws from the caller's generator: column 3 of the (n_steps, 4) table holds cz, read by
``omg_fuse_cfg_step_noise`` together with the pre-drawn noise of every step.
"""
from __future__ import annotations

from types import MappingProxyType
from typing import Mapping

import numpy as np
import torch

from . import _lib as L


class _Base:
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 1):
        self.num_train_timesteps = num_train_timesteps
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.steps_offset = steps_offset
        self.timesteps = None
        self.num_inference_steps = None
        self._config = dict(_class_name=type(self).__name__, num_train_timesteps=num_train_timesteps, beta_start=beta_start,
                            beta_end=beta_end, beta_schedule="scaled_linear", steps_offset=steps_offset, timestep_spacing="leading",
                            prediction_type="epsilon")

    @property
    def config(self) -> Mapping:
        """read-only diffusers-style ``scheduler.config`` (what ``DPMSolverMultistepScheduler.from_config`` takes)"""
        return MappingProxyType(self._config)

    def _leading(self, n: int) -> np.ndarray:
        ratio = self.num_train_timesteps // n
        return (np.arange(0, n) * ratio).round()[::-1].astype(np.int64) + self.steps_offset

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        self._ts = self._leading(num_inference_steps)
        self.timesteps = torch.from_numpy(self._ts.astype(np.float32 if self.float_timesteps else np.int64)).to(device)
        self._build()

    # (n,) float64 arrays filled by _build()
    cx: np.ndarray
    ce: np.ndarray
    cin: np.ndarray

    def coef_table(self, device) -> torch.Tensor:
        """(n, 4) fp32 per-step coefficients [c_x, c_eps, c_in of the NEXT step, 0] on ``device``.  Cached per device, keyed by the BYTES of
        the host table: a re-configured scheduler (other betas / spacing / step count) gets a new table, an unchanged one costs no
        host-to-device copy per call (the table was rebuilt and copied on every pipeline call)."""
        return self._table(device, self.cx, self.ce)

    def _table(self, device, cx, ce, cz=None) -> torch.Tensor:
        """the (n, 4) table of :meth:`coef_table` with column 3 = ``cz``, the noise coefficient of a stochastic step (0 when None)"""
        n = self.num_inference_steps
        tab = np.zeros((n, 4), dtype=np.float64)
        tab[:, 0], tab[:, 1] = cx, ce
        tab[:-1, 2] = self.cin[1:]
        tab[-1, 2] = 1.0
        if cz is not None:
            tab[:, 3] = cz
        host = tab.astype(np.float32)
        key = (str(device), host.tobytes())
        cached = self.__dict__.get("_coef_cache")
        if cached is None or cached[0] != key:
            cached = (key, torch.from_numpy(host).to(device))
            self._coef_cache = cached
        return cached[1]

    def cin0(self, device) -> torch.Tensor:
        return torch.tensor([self.cin[0]], dtype=torch.float32, device=device)

    def _index(self, t) -> int:
        tv = float(t)
        idx = np.nonzero(self._ts == int(round(tv)))[0]
        if len(idx) == 0:
            raise ValueError(f"timestep {tv} is not on the schedule")
        return int(idx[0])

    # diffusers-style per-step API (host-driven use outside the fused loop)
    def scale_model_input(self, sample: torch.Tensor, t) -> torch.Tensor:
        return sample * float(self.cin[self._index(t)])

    def step(self, model_output: torch.Tensor, t, sample: torch.Tensor, return_dict: bool = False, **kw):
        i = self._index(t)
        prev = (float(self.cx[i]) * sample.float() + float(self.ce[i]) * model_output.float()).to(sample.dtype)
        return (prev,)


class DDIMScheduler(_Base):
    """DDIM; ``eta`` is an argument of :meth:`coef_table` and :meth:`step`, not configuration, as in diffusers (where it is a ``step()``
    argument).  With eta > 0 the step adds std_i * z_i, z_i fresh Gaussian noise (formulas recalled from diffusers 0.25's
    ``DDIMScheduler.step`` / ``_get_variance``, not checked against its source; parity stays unpinned):

        std_i  = eta * sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))
        x'     = sqrt(a_prev / a_t) x + (sqrt(1 - a_prev - std_i^2) - sqrt(a_prev (1 - a_t) / a_t)) eps + std_i z_i

    ``use_clipped_model_output`` is not built."""
    float_timesteps = False
    init_noise_sigma = 1.0

    def _build(self):
        n = self.num_inference_steps
        ac = self.alphas_cumprod
        ratio = self.num_train_timesteps // n
        a_t = ac[self._ts]
        prev = self._ts - ratio
        a_p = np.where(prev >= 0, ac[np.clip(prev, 0, None)], ac[0])     # set_alpha_to_one = False
        self._a_t, self._a_p = a_t, a_p
        self.cx = np.sqrt(a_p / a_t)
        self.ce = np.sqrt(1 - a_p) - np.sqrt(a_p * (1 - a_t) / a_t)
        self.cin = np.ones(n)

    def eta_coefficients(self, eta: float):
        """float64 (cx, ce, cz) per step for ``eta``; eta = 0 gives (cx, ce, 0) of the deterministic table"""
        a_t, a_p = self._a_t, self._a_p
        std = float(eta) * np.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))
        ce = np.sqrt(1 - a_p - std ** 2) - np.sqrt(a_p * (1 - a_t) / a_t)
        return self.cx, ce, std

    def coef_table(self, device, eta: float = 0.0) -> torch.Tensor:
        """(n, 4) fp32 table; eta = 0: exactly the deterministic table, eta > 0: row i = (cx_i, ce_i(eta), 1, std_i) for
        ``omg_fuse_cfg_step_noise``"""
        if float(eta) == 0.0:
            return super().coef_table(device)
        if float(eta) < 0.0:
            raise ValueError(f"DDIMScheduler: eta={eta} must be >= 0")
        return self._table(device, *self.eta_coefficients(eta))

    def step(self, model_output: torch.Tensor, t, sample: torch.Tensor, eta: float = 0.0, use_clipped_model_output: bool = False,
             generator=None, return_dict: bool = False, **kw):
        """diffusers-style step; eta > 0 draws z = ``torch.randn`` (float32, on the generator's device) from ``generator``"""
        if use_clipped_model_output:
            raise L.OmgHipError("DDIMScheduler: use_clipped_model_output=True is not implemented")
        if float(eta) == 0.0:
            return super().step(model_output, t, sample)
        i = self._index(t)
        cx, ce, cz = (float(c[i]) for c in self.eta_coefficients(eta))
        z = draw_noise(model_output.shape, generator, model_output.device)
        prev = cx * sample.double() + ce * model_output.double() + cz * z.double()
        return (prev.to(sample.dtype),)


class EulerDiscreteScheduler(_Base):
    float_timesteps = True

    def _build(self):
        n = self.num_inference_steps
        ac = self.alphas_cumprod
        sig_all = np.sqrt((1 - ac) / ac)
        s = np.interp(self._ts.astype(np.float64), np.arange(self.num_train_timesteps), sig_all)
        self.sigmas = np.concatenate([s, [0.0]])
        self.init_noise_sigma = float(np.sqrt(self.sigmas.max() ** 2 + 1))   # "leading" spacing
        self.cx = np.ones(n)
        self.ce = self.sigmas[1:] - self.sigmas[:-1]
        self.cin = 1.0 / np.sqrt(s ** 2 + 1)


# ------------------------------------------------------------------------------------------------------- DPM-Solver++ (multistep)
# columns of a row of the multistep table (``omg_fuse_cfg_step_ms``, include/omg_hip.h)
MS_A, MS_B, MS_CX, MS_CM, MS_CP, MS_CIN, MS_WIDTH = 0, 1, 2, 3, 4, 5, 8


def dpm_coefficients(sigmas, orders, solver_type: str = "midpoint") -> np.ndarray:
    """Per-step coefficients of DPM-Solver++ for epsilon prediction, float64 (n, 8), from the n + 1 sigmas of a schedule (the last one is
    the endpoint) and the solver order of each of the n steps.  Row i = [a, b, cx, cm, cp, cin_next, 0, 0]:

        m_i     = a * x_i + b * eps_i                        (a = 1 / alpha_i, b = -sigma_i: the data prediction)
        x_{i+1} = cx * x_i + cm * m_i + cp * m_{i-1}

    with alpha = 1 / sqrt(sigma^2 + 1), s = sigma * alpha, lambda = -log sigma, h = lambda_{i+1} - lambda_i, phi = sigma_{i+1} / sigma_i - 1
    (= e^-h - 1) and, for order 2, h0 = lambda_i - lambda_{i-1} (r0 = h0 / h, D1 = (m_i - m_{i-1}) / r0):

        order 1           : cx = s_{i+1} / s_i,  cm = -alpha_{i+1} phi,                          cp = 0
        order 2, midpoint : cm = -alpha_{i+1} phi (1 + h / (2 h0)),       cp = alpha_{i+1} phi h / (2 h0)
        order 2, heun     : cm = -alpha_{i+1} phi + alpha_{i+1} (phi + h) / h0,  cp = -alpha_{i+1} (phi + h) / h0

    Written with h / h0 instead of 1 / r0 and (phi + h) / h0 instead of (phi / h + 1) / r0, so that a zero-length step (h = 0: the repeated
    last Karras sigma) is the identity map, the limit of the formulas, with cp = 0.  cin_next = 1: the model input is the sample itself."""
    sig = np.asarray(sigmas, dtype=np.float64)
    orders = [int(o) for o in orders]
    n = len(orders)
    if sig.shape != (n + 1,):
        raise ValueError(f"dpm_coefficients: {n} steps need {n + 1} sigmas, got {sig.shape}")
    if solver_type not in ("midpoint", "heun"):
        raise ValueError(f"dpm_coefficients: solver_type {solver_type!r}")
    if orders and (orders[0] != 1 or any(o not in (1, 2) for o in orders)):
        raise ValueError(f"dpm_coefficients: orders must be 1 or 2 and the first one 1, got {orders}")
    alpha = 1.0 / np.sqrt(sig ** 2 + 1.0)
    s = sig * alpha
    lam = -np.log(sig)
    tab = np.zeros((n, MS_WIDTH), dtype=np.float64)
    for i, o in enumerate(orders):
        h = lam[i + 1] - lam[i]
        phi = sig[i + 1] / sig[i] - 1.0
        a1 = alpha[i + 1]
        tab[i, MS_A], tab[i, MS_B] = 1.0 / alpha[i], -sig[i]
        tab[i, MS_CX] = s[i + 1] / s[i]
        tab[i, MS_CM] = -a1 * phi
        if o == 2:
            h0 = lam[i] - lam[i - 1]
            if solver_type == "midpoint":
                tab[i, MS_CM] -= 0.5 * a1 * phi * h / h0
                tab[i, MS_CP] = 0.5 * a1 * phi * h / h0
            else:
                tab[i, MS_CM] += a1 * (phi + h) / h0
                tab[i, MS_CP] = -a1 * (phi + h) / h0
        tab[i, MS_CIN] = 1.0
    return tab


# the keys of diffusers 0.25's DPMSolverMultistepScheduler.__init__ with this class's defaults: diffusers' own, except the schedule, which
# is SDXL-base's (beta 0.00085 .. 0.012 scaled_linear, "leading", offset 1) like DDIMScheduler's and EulerDiscreteScheduler's above
_DPM_DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                     algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, euler_at_final=False,
                     use_karras_sigmas=False, use_lu_lambdas=False, lambda_min_clipped=-float("inf"), variance_type=None,
                     timestep_spacing="leading", steps_offset=1)
_DPM_SUPPORTED = dict(beta_schedule=("linear", "scaled_linear"), trained_betas=(None,), solver_order=(1, 2), prediction_type=("epsilon",),
                      thresholding=(False,), algorithm_type=("dpmsolver++",), solver_type=("midpoint", "heun"), use_lu_lambdas=(False,),
                      lambda_min_clipped=(-float("inf"),), variance_type=(None,), timestep_spacing=("leading",))


class DPMSolverMultistepScheduler:
    """DPM-Solver++ (multistep, orders 1 and 2) for epsilon prediction, after diffusers 0.25's ``DPMSolverMultistepScheduler``.

    Unlike DDIM and Euler a step is not a map of (sample, eps) alone: order 2 also needs the previous step's data prediction
    m_{i-1}.  The fused loop keeps it in a device buffer (``omg_fuse_cfg_step_ms``: m_i = a x + b eps is written back every step) and
    reads an (n, 8) table of :func:`dpm_coefficients`; an order-1 row has cp = 0 and the kernel then does not read the buffer.

    Which order runs at step i: step 0 is order 1; the last step is order 1 if ``euler_at_final`` or if ``lower_order_final`` and
    n < 15; every other step runs ``solver_order``.

    Supported: algorithm_type "dpmsolver++", solver_order 1 | 2, solver_type "midpoint" | "heun", lower_order_final, euler_at_final,
    use_karras_sigmas, timestep_spacing "leading", prediction_type "epsilon", thresholding off, a "linear" or "scaled_linear" beta
    schedule and steps_offset; any other value of a diffusers option raises OmgHipError naming it.  Without arguments it runs the
    SDXL-base schedule (``make_scheduler("dpm")``); ``from_config`` takes a checkpoint's or another scheduler's.

    Choices (diffusers' source is not at hand; these are recalled, not checked, and parity with diffusers stays UNPINNED, as for
    DDIM and Euler — DESIGN §3):
      * "leading" spacing uses step_ratio = num_train_timesteps // (n + 1): t_i = (n - i) * step_ratio + steps_offset (DDIM: // n);
      * without Karras sigmas sigma_i is interpolated at t_i and the appended final sigma is sigma(alphas_cumprod[0]), the endpoint
        DDIM uses with set_alpha_to_one=False;
      * with Karras sigmas (rho = 7, between the schedule's smallest and largest sigma) the last sigma is repeated — the last step then
        has h = 0 and is the identity map (the limit of the formulas; the heun form written with 1 / h would give 0 / 0) — and t_i is the
        log-sigma interpolation of sigma_i, rounded (duplicates are kept);
      * timesteps are not de-duplicated; the host ``step()`` counts steps from the first timestep it is called with.
    """
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, **kwargs):
        unknown = sorted(set(kwargs) - set(_DPM_DEFAULTS))
        if unknown:
            raise TypeError(f"DPMSolverMultistepScheduler: unexpected keyword argument(s) {unknown}")
        cfg = {**_DPM_DEFAULTS, **kwargs}
        for name, ok in _DPM_SUPPORTED.items():
            if cfg[name] not in ok:
                raise L.OmgHipError(f"DPMSolverMultistepScheduler: {name}={cfg[name]!r} is not implemented; supported: {list(ok)}")
        for name in ("lower_order_final", "euler_at_final", "use_karras_sigmas"):
            cfg[name] = bool(cfg[name])
        cfg["solver_order"] = int(cfg["solver_order"])
        self._config = {"_class_name": type(self).__name__, **cfg}
        T = self.num_train_timesteps = int(cfg["num_train_timesteps"])
        if cfg["beta_schedule"] == "scaled_linear":
            betas = np.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, T, dtype=np.float64) ** 2
        else:
            betas = np.linspace(cfg["beta_start"], cfg["beta_end"], T, dtype=np.float64)
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.steps_offset = int(cfg["steps_offset"])
        self.timesteps = None
        self.num_inference_steps = None

    @classmethod
    def from_config(cls, config: Mapping, **overrides) -> "DPMSolverMultistepScheduler":
        """diffusers' ``from_config``: the keys of ``config`` (e.g. another scheduler's ``.config`` or a ``scheduler_config.json``) that
        this scheduler has, then ``overrides``; other keys are ignored, as diffusers ignores them."""
        merged = {**dict(config), **overrides}
        return cls(**{k: v for k, v in merged.items() if k in _DPM_DEFAULTS})

    @property
    def config(self) -> Mapping:
        return MappingProxyType(self._config)

    def set_timesteps(self, num_inference_steps: int, device=None):
        n = self.num_inference_steps = int(num_inference_steps)
        cfg, T = self._config, self.num_train_timesteps
        ac = self.alphas_cumprod
        sig_all = np.sqrt((1 - ac) / ac)
        ratio = T // (n + 1)
        ts = (np.arange(0, n + 1) * ratio).round()[::-1][:-1].astype(np.int64) + self.steps_offset
        if cfg["use_karras_sigmas"]:
            rho = 7.0
            lo, hi = sig_all[0] ** (1 / rho), sig_all[-1] ** (1 / rho)
            s = (hi + np.linspace(0, 1, n) * (lo - hi)) ** rho
            log_all = np.log(sig_all)
            ts = np.array([self._sigma_to_t(v, log_all) for v in s]).round().astype(np.int64)
            self.sigmas = np.concatenate([s, s[-1:]])
        else:
            s = np.interp(ts.astype(np.float64), np.arange(T), sig_all)
            self.sigmas = np.concatenate([s, [sig_all[0]]])
        self._ts = ts
        self.timesteps = torch.from_numpy(ts).to(device)
        self.orders = [1 if i == 0 or (i == n - 1 and (cfg["euler_at_final"] or (cfg["lower_order_final"] and n < 15)))
                       else cfg["solver_order"] for i in range(n)]
        self.table = dpm_coefficients(self.sigmas, self.orders, cfg["solver_type"])
        self.cin = self.table[:, MS_CIN].copy()
        self._step_index = None
        self._m_prev = None

    @staticmethod
    def _sigma_to_t(sigma: float, log_sigmas: np.ndarray) -> float:
        ls = np.log(sigma)
        low = int(min(np.cumsum(ls - log_sigmas >= 0).argmax(), len(log_sigmas) - 2))
        w = np.clip((log_sigmas[low] - ls) / (log_sigmas[low] - log_sigmas[low + 1]), 0, 1)
        return (1 - w) * low + w * (low + 1)

    def coef_table(self, device) -> torch.Tensor:
        """(n, 8) fp32 multistep table (:func:`dpm_coefficients`) on ``device``, cached per device and keyed by its bytes like
        ``_Base.coef_table``: Karras / plain and midpoint / heun tables differ in their bytes."""
        host = self.table.astype(np.float32)
        key = (str(device), host.tobytes())
        cached = self.__dict__.get("_coef_cache")
        if cached is None or cached[0] != key:
            cached = (key, torch.from_numpy(host).to(device))
            self._coef_cache = cached
        return cached[1]

    def cin0(self, device) -> torch.Tensor:
        return torch.tensor([self.cin[0]], dtype=torch.float32, device=device)

    def scale_model_input(self, sample: torch.Tensor, t=None) -> torch.Tensor:
        return sample

    def step(self, model_output: torch.Tensor, t, sample: torch.Tensor, return_dict: bool = False, **kw):
        """diffusers-style STATEFUL step: the previous data prediction is kept between calls (reset by ``set_timesteps``); the first
        call finds its step from ``t``, every later one takes the next step."""
        if self._step_index is None:
            idx = np.nonzero(self._ts == int(round(float(t))))[0]
            if len(idx) == 0:
                raise ValueError(f"timestep {float(t)} is not on the schedule")
            self._step_index = int(idx[0])
        i = self._step_index
        if i >= self.num_inference_steps:
            raise ValueError("step() called more often than there are steps; call set_timesteps() again")
        a, b, cx, cm, cp = (float(v) for v in self.table[i, :MS_CIN])
        x, e = sample.double(), model_output.double()
        m = a * x + b * e
        prev = cx * x + cm * m
        if cp != 0.0:
            prev = prev + cp * self._m_prev
        self._m_prev = m
        self._step_index = i + 1
        return (prev.to(sample.dtype),)


# ------------------------------------------------------------------------------------------------------- stochastic steps
def draw_noise(shape, generator, device) -> torch.Tensor:
    """one step's Gaussian noise: ``torch.randn(shape)`` float32 from ``generator`` on the generator's device (``device`` without one),
    moved to ``device``.  diffusers draws it in the model output's dtype (fp16 in the reference's loop); float32 here, as for the initial
    latents, so the numbers differ from an fp16 draw of the same generator."""
    gen_dev = generator.device if generator is not None else device
    return torch.randn(tuple(shape), generator=generator, device=gen_dev, dtype=torch.float32).to(device)


# the keys of diffusers 0.25's EulerAncestralDiscreteScheduler.__init__ (recalled) with SDXL-base's schedule as the defaults, like _DPM_DEFAULTS
_EULER_A_DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
                         prediction_type="epsilon", timestep_spacing="leading", steps_offset=1, rescale_betas_zero_snr=False)
_EULER_A_SUPPORTED = dict(beta_schedule=("linear", "scaled_linear"), trained_betas=(None,), prediction_type=("epsilon",),
                          timestep_spacing=("leading",), rescale_betas_zero_snr=(False,))


class EulerAncestralDiscreteScheduler(_Base):
    """Euler-ancestral for epsilon prediction, after diffusers 0.25's ``EulerAncestralDiscreteScheduler`` (the usual SDXL sampler).  Per
    step i, with sigma_from = sigma_i, sigma_to = sigma_{i+1} (0 after the last step):

        sigma_up   = sqrt(sigma_to^2 (sigma_from^2 - sigma_to^2) / sigma_from^2),   sigma_down = sqrt(sigma_to^2 - sigma_up^2)
        x'         = x + (sigma_down - sigma_i) eps + sigma_up z_i

    z_i fresh Gaussian noise per step.  Table row i = (1, sigma_down - sigma_i, cin_{i+1}, sigma_up), read by ``omg_fuse_cfg_step_noise``;
    the last step has sigma_up = 0 and adds no noise.  The schedule is EulerDiscreteScheduler's: "leading" timesteps, sigma interpolated at
    them, cin = 1 / sqrt(sigma^2 + 1), init_noise_sigma = sqrt(max sigma^2 + 1).

    Supported: epsilon prediction, "leading" spacing, steps_offset, a "linear" or "scaled_linear" beta schedule; any other value of a
    diffusers option raises OmgHipError naming it.  The option names, the formulas and the schedule are recalled from diffusers 0.25, not
    checked against its source: parity stays UNPINNED, as for the other schedulers.  The host ``step()`` is stateful like
    diffusers' (the first call finds its step from ``t``) and draws its noise with :func:`draw_noise`."""
    float_timesteps = True

    def __init__(self, **kwargs):
        unknown = sorted(set(kwargs) - set(_EULER_A_DEFAULTS))
        if unknown:
            raise TypeError(f"EulerAncestralDiscreteScheduler: unexpected keyword argument(s) {unknown}")
        cfg = {**_EULER_A_DEFAULTS, **kwargs}
        for name, ok in _EULER_A_SUPPORTED.items():
            if cfg[name] not in ok:
                raise L.OmgHipError(f"EulerAncestralDiscreteScheduler: {name}={cfg[name]!r} is not implemented; supported: {list(ok)}")
        self._config = {"_class_name": type(self).__name__, **cfg}
        T = self.num_train_timesteps = int(cfg["num_train_timesteps"])
        if cfg["beta_schedule"] == "scaled_linear":
            betas = np.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, T, dtype=np.float64) ** 2
        else:
            betas = np.linspace(cfg["beta_start"], cfg["beta_end"], T, dtype=np.float64)
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.steps_offset = int(cfg["steps_offset"])
        self.timesteps = None
        self.num_inference_steps = None

    @classmethod
    def from_config(cls, config: Mapping, **overrides) -> "EulerAncestralDiscreteScheduler":
        """diffusers' ``from_config``: the keys of ``config`` this scheduler has, then ``overrides``; other keys are ignored"""
        merged = {**dict(config), **overrides}
        return cls(**{k: v for k, v in merged.items() if k in _EULER_A_DEFAULTS})

    def _build(self):
        n = self.num_inference_steps
        ac = self.alphas_cumprod
        sig_all = np.sqrt((1 - ac) / ac)
        s = np.interp(self._ts.astype(np.float64), np.arange(self.num_train_timesteps), sig_all)
        self.sigmas = np.concatenate([s, [0.0]])
        self.init_noise_sigma = float(np.sqrt(self.sigmas.max() ** 2 + 1))   # "leading" spacing
        s_from, s_to = self.sigmas[:-1], self.sigmas[1:]
        self.sigma_up = np.sqrt(s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2)
        self.sigma_down = np.sqrt(s_to ** 2 - self.sigma_up ** 2)
        self.cx = np.ones(n)
        self.ce = self.sigma_down - s_from
        self.cz = self.sigma_up
        self.cin = 1.0 / np.sqrt(s ** 2 + 1)
        self._step_index = None

    def coef_table(self, device) -> torch.Tensor:
        """(n, 4) fp32 table (1, sigma_down - sigma_i, cin_{i+1}, sigma_up), cached like ``_Base.coef_table``"""
        return self._table(device, self.cx, self.ce, self.cz)

    def step(self, model_output: torch.Tensor, t, sample: torch.Tensor, generator=None, return_dict: bool = False, **kw):
        """diffusers-style STATEFUL step (reset by ``set_timesteps``): x + (sigma_down - sigma) eps + sigma_up z, z from ``generator``"""
        if self._step_index is None:
            self._step_index = self._index(t)
        i = self._step_index
        if i >= self.num_inference_steps:
            raise ValueError("step() called more often than there are steps; call set_timesteps() again")
        z = draw_noise(model_output.shape, generator, model_output.device)
        prev = sample.double() + float(self.ce[i]) * model_output.double() + float(self.cz[i]) * z.double()
        self._step_index = i + 1
        return (prev.to(sample.dtype),)


def is_stochastic(scheduler, eta: float = 0.0) -> bool:
    """whether a step of ``scheduler`` adds fresh noise: Euler-ancestral always, DDIM when eta > 0; every other scheduler ignores eta
    (as diffusers' ``prepare_extra_step_kwargs`` passes eta only to a ``step()`` that takes it)"""
    return isinstance(scheduler, EulerAncestralDiscreteScheduler) or (isinstance(scheduler, DDIMScheduler) and float(eta) > 0.0)


def make_scheduler(name: str):
    return {"ddim": DDIMScheduler, "euler": EulerDiscreteScheduler, "dpm": DPMSolverMultistepScheduler,
            "euler_a": EulerAncestralDiscreteScheduler}[name.lower()]()
