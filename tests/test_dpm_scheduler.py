"""CPU tests (-m "not gpu"): DPM-Solver++ multistep (omg_amd.schedulers.DPMSolverMultistepScheduler) — its coefficient table
against the literal stateful restatement in tests/_dpm_oracle.py, its first-order path against DDIM, exactness on point-mass data, its
convergence order, the drop-in surface of omg_amd.compat and the C-ABI entry point of its step kernel."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from omg_amd import _lib as L
from omg_amd.schedulers import (MS_A, MS_B, MS_CM, MS_CP, MS_CX, DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler,
                                dpm_coefficients, make_scheduler)
from tests import _dpm_oracle as dpo

SDXL_SCHEDULER = {"_class_name": "EulerDiscreteScheduler", "_diffusers_version": "0.19.0.dev0", "beta_end": 0.012,
                  "beta_schedule": "scaled_linear", "beta_start": 0.00085, "clip_sample": False, "interpolation_type": "linear",
                  "num_train_timesteps": 1000, "prediction_type": "epsilon", "sample_max_value": 1.0, "set_alpha_to_one": False,
                  "skip_prk_steps": True, "steps_offset": 1, "timestep_spacing": "leading", "trained_betas": None, "use_karras_sigmas": False}


def table_run(tab, x, eps_seq):
    """the fused kernel's arithmetic in float64: m = a x + b eps ; x' = cx x + cm m + cp m_prev"""
    m_prev = None
    for row, e in zip(tab, eps_seq):
        m = row[MS_A] * x + row[MS_B] * e
        x = row[MS_CX] * x + row[MS_CM] * m + (row[MS_CP] * m_prev if row[MS_CP] != 0.0 else 0.0)
        m_prev = m
    return x


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("n", [1, 2, 3, 8, 14, 15, 25, 50])
@pytest.mark.parametrize("karras", [False, True])
def test_table_matches_the_stateful_restatement(n, karras):
    rng = np.random.default_rng(n + 100 * karras)
    x0 = rng.standard_normal((2, 3, 5))
    eps_seq = [rng.standard_normal((2, 3, 5)) for _ in range(n)]
    for order, stype, lof, eaf in itertools.product((1, 2), ("midpoint", "heun"), (False, True), (False, True)):
        sch = DPMSolverMultistepScheduler.from_config(SDXL_SCHEDULER, solver_order=order, solver_type=stype, lower_order_final=lof,
                                                      euler_at_final=eaf, use_karras_sigmas=karras)
        sch.set_timesteps(n)
        ref = dpo.DPMSolverPP(n, order, stype, lof, eaf, karras)
        assert np.array_equal(sch.timesteps.numpy(), ref.timesteps), (sch.timesteps, ref.timesteps)
        assert np.allclose(sch.sigmas, ref.sigmas, rtol=1e-13, atol=0)
        x = x0
        for i, e in enumerate(eps_seq):
            x = ref.step(e, i, x)
        got = table_run(sch.table, x0, eps_seq)
        assert rel(got, x) <= 1e-12, (order, stype, lof, eaf, rel(got, x))
        # the diffusers-style host API: stateful step() over the scheduler's own timesteps
        xs = torch.from_numpy(x0)
        for t, e in zip(sch.timesteps, eps_seq):
            xs = sch.step(torch.from_numpy(e), t, xs)[0]
        assert rel(xs.numpy(), x) <= 1e-12
        assert torch.equal(sch.scale_model_input(xs, sch.timesteps[0]), xs)


def test_orders_per_step():
    for n, lof, eaf, want_last in ((14, True, False, 1), (15, True, False, 2), (15, False, True, 1), (8, False, False, 2)):
        s = DPMSolverMultistepScheduler(lower_order_final=lof, euler_at_final=eaf)
        s.set_timesteps(n)
        assert s.orders[0] == 1 and s.orders[-1] == want_last and set(s.orders[1:-1]) <= {2}
        assert (s.table[np.array(s.orders) == 1, MS_CP] == 0).all(), "order-1 rows carry no m_{i-1} coefficient"
    s = DPMSolverMultistepScheduler(solver_order=1)
    s.set_timesteps(10)
    assert s.orders == [1] * 10


@pytest.mark.parametrize("n", [1, 5, 10, 25, 50])
def test_first_order_is_ddim(n):
    """DPM-Solver++(1) = DDIM with eta = 0: on DDIMScheduler's own timesteps and endpoint its coefficients are that class's cx / ce."""
    d = DDIMScheduler()
    d.set_timesteps(n)
    ac, ratio = d.alphas_cumprod, d.num_train_timesteps // n
    a_t = ac[d._ts]
    prev = d._ts - ratio
    a_p = np.where(prev >= 0, ac[np.clip(prev, 0, None)], ac[0])
    assert np.array_equal(a_p[:-1], a_t[1:])
    sig = np.sqrt((1 - np.append(a_t, a_p[-1])) / np.append(a_t, a_p[-1]))
    tab = dpm_coefficients(sig, [1] * n)
    cx = tab[:, MS_CX] + tab[:, MS_CM] * tab[:, MS_A]
    ce = tab[:, MS_CM] * tab[:, MS_B]
    assert np.abs(cx - d.cx).max() <= 1e-12 * np.abs(d.cx).max()
    assert np.abs(ce - d.ce).max() <= 1e-12 * np.abs(d.ce).max()


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("stype", ["midpoint", "heun"])
def test_exact_on_point_mass_data(karras, order, stype):
    """data = x0* exactly: eps = (x - alpha x0*) / s is the exact noise, m = x0* every step, and both orders land on alpha x0* + s z."""
    rng = np.random.default_rng(3)
    xs, z = rng.standard_normal(64), rng.standard_normal(64)
    sch = DPMSolverMultistepScheduler.from_config(SDXL_SCHEDULER, solver_order=order, solver_type=stype, use_karras_sigmas=karras,
                                                  lower_order_final=False)
    sch.set_timesteps(20)
    alpha = 1 / np.sqrt(sch.sigmas ** 2 + 1)
    s = sch.sigmas * alpha
    x = alpha[0] * xs + s[0] * z
    m_prev = None
    for i, row in enumerate(sch.table):
        eps = (x - alpha[i] * xs) / s[i]
        m = row[MS_A] * x + row[MS_B] * eps
        x = row[MS_CX] * x + row[MS_CM] * m + (row[MS_CP] * m_prev if m_prev is not None else 0.0)
        m_prev = m
    want = alpha[-1] * xs + s[-1] * z
    assert rel(x, want) <= 1e-12


def test_convergence_order():
    """1-D Gaussian data N(mu, s0^2) with its analytic eps on a uniform-lambda grid: the probability-flow ODE maps quantiles, so the exact
    endpoint is known.  Doubling the steps cuts the order-2 error by >= 3x, the order-1 error by about 2x."""
    mu, s0 = 0.5, 0.8
    z = np.linspace(-2.5, 2.5, 41)

    def run(n, order):
        lam = np.linspace(-np.log(10.0), -np.log(0.05), n + 1)
        sig = np.exp(-lam)
        alpha = 1 / np.sqrt(sig ** 2 + 1)
        s = sig * alpha
        tab = dpm_coefficients(sig, [1] + [order] * (n - 1))
        x = alpha[0] * mu + np.sqrt(alpha[0] ** 2 * s0 ** 2 + s[0] ** 2) * z
        m_prev = None
        for i, row in enumerate(tab):
            eps = s[i] * (x - alpha[i] * mu) / (alpha[i] ** 2 * s0 ** 2 + s[i] ** 2)
            m = row[MS_A] * x + row[MS_B] * eps
            x = row[MS_CX] * x + row[MS_CM] * m + (row[MS_CP] * m_prev if m_prev is not None else 0.0)
            m_prev = m
        want = alpha[-1] * mu + np.sqrt(alpha[-1] ** 2 * s0 ** 2 + s[-1] ** 2) * z
        return np.abs(x - want).max()

    for order, lo, hi in ((2, 3.0, 6.0), (1, 1.6, 2.5)):
        errs = [run(n, order) for n in (10, 20, 40, 80)]
        ratios = [a / b for a, b in zip(errs, errs[1:])]
        print(f"order {order}: errors {errs}, ratios {ratios}")
        assert all(lo <= r <= hi for r in ratios), (order, errs, ratios)
    # the literal restatement agrees on this custom grid too
    lam = np.linspace(-np.log(10.0), -np.log(0.05), 11)
    ref = dpo.DPMSolverPP(10, 2, "heun", sigmas=np.exp(-lam))
    rng = np.random.default_rng(0)
    x0, eps_seq = rng.standard_normal(7), [rng.standard_normal(7) for _ in range(10)]
    x = x0
    for i, e in enumerate(eps_seq):
        x = ref.step(e, i, x)
    orders = [1] + [2] * 8 + [1]                # n < 15 with lower_order_final
    assert rel(table_run(dpm_coefficients(np.exp(-lam), orders, "heun"), x0, eps_seq), x) <= 1e-12


def test_configurations_get_distinct_tables():
    """the engine's and StageCache's keys hold the scheduler class and the table BYTES: Karras vs not, midpoint vs heun, order 1 vs 2 must
    not share them"""
    tabs = {}
    for karras, stype, order in itertools.product((False, True), ("midpoint", "heun"), (1, 2)):
        s = DPMSolverMultistepScheduler.from_config(SDXL_SCHEDULER, use_karras_sigmas=karras, solver_type=stype, solver_order=order)
        s.set_timesteps(8)
        tabs[(karras, stype, order)] = s.coef_table("cpu").numpy().tobytes()
    distinct = {k: v for k, v in tabs.items() if k[2] == 2}
    assert len(set(distinct.values())) == len(distinct)
    assert tabs[(False, "midpoint", 1)] != tabs[(True, "midpoint", 1)]
    assert tabs[(False, "midpoint", 1)] == tabs[(False, "heun", 1)], "order 1 has no solver type"
    assert s.coef_table("cpu").shape == (8, 8) and s.coef_table("cpu").dtype == torch.float32


def test_from_config_of_the_sdxl_base_scheduler():
    s = DPMSolverMultistepScheduler.from_config(SDXL_SCHEDULER)
    assert isinstance(s, DPMSolverMultistepScheduler)
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2
    assert np.allclose(s.alphas_cumprod, np.cumprod(1 - betas), rtol=1e-14, atol=0)
    c = s.config
    assert (c["beta_schedule"], c["beta_start"], c["beta_end"], c["timestep_spacing"], c["steps_offset"]) == ("scaled_linear", 0.00085, 0.012, "leading", 1)
    assert (c["algorithm_type"], c["solver_order"], c["solver_type"], c["use_karras_sigmas"]) == ("dpmsolver++", 2, "midpoint", False)
    with pytest.raises(TypeError):
        c["solver_order"] = 1                                   # read-only
    s.set_timesteps(25)
    assert s.timesteps[0].item() == 25 * (1000 // 26) + 1 and s.timesteps[-1].item() == 1000 // 26 + 1
    assert s.init_noise_sigma == 1.0 and s.order == 1
    k = DPMSolverMultistepScheduler.from_config(make_scheduler("euler").config, use_karras_sigmas=True, solver_type="heun")
    assert k.config["use_karras_sigmas"] and k.config["solver_type"] == "heun" and k.config["beta_start"] == 0.00085
    assert isinstance(make_scheduler("dpm"), DPMSolverMultistepScheduler)
    for sch in (DDIMScheduler(), EulerDiscreteScheduler()):
        assert sch.config["_class_name"] == type(sch).__name__ and sch.config["beta_end"] == 0.012


@pytest.mark.parametrize("option,value", [("algorithm_type", "dpmsolver"), ("algorithm_type", "sde-dpmsolver++"), ("solver_order", 3),
                                          ("solver_type", "bh2"), ("prediction_type", "v_prediction"), ("thresholding", True),
                                          ("timestep_spacing", "trailing"), ("timestep_spacing", "linspace"), ("use_lu_lambdas", True),
                                          ("beta_schedule", "squaredcos_cap_v2"), ("trained_betas", [0.1] * 1000),
                                          ("variance_type", "learned_range"), ("lambda_min_clipped", -5.1)])
def test_unsupported_options_are_refused_by_name(option, value):
    with pytest.raises(L.OmgHipError, match=option):
        DPMSolverMultistepScheduler.from_config(SDXL_SCHEDULER, **{option: value})


def test_install_exports_the_scheduler():
    from omg_amd import compat
    compat.install()
    try:
        import diffusers
        cls = diffusers.DPMSolverMultistepScheduler
        assert cls is DPMSolverMultistepScheduler
        s = cls.from_config(diffusers.EulerDiscreteScheduler().config, use_karras_sigmas=True)
        s.set_timesteps(20)
        assert len(s.timesteps) == 20 and s.config["use_karras_sigmas"]
    finally:
        compat.uninstall()


def test_from_pretrained_maps_a_dpm_scheduler_config(tmp_path):
    from omg_amd import compat
    from tests import _fake_hub as hub
    model = hub.write_sdxl_dir(str(tmp_path / "sdxl"))
    cfg = dict(SDXL_SCHEDULER, _class_name="DPMSolverMultistepScheduler", use_karras_sigmas=True, solver_type="heun", euler_at_final=True)
    json.dump(cfg, open(os.path.join(model, "scheduler", "scheduler_config.json"), "w"))
    pipe = compat.LoraMultiConceptPipeline.from_pretrained(model, torch_dtype=torch.float16, variant="fp16")
    s = pipe.scheduler
    assert isinstance(s, DPMSolverMultistepScheduler)
    assert s.config["use_karras_sigmas"] and s.config["solver_type"] == "heun" and s.config["euler_at_final"] and s.config["steps_offset"] == 1
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, use_karras_sigmas=False)
    assert not pipe.scheduler.config["use_karras_sigmas"]
    other = hub.write_sdxl_dir(str(tmp_path / "sdxl_sde"))
    json.dump(dict(cfg, algorithm_type="sde-dpmsolver++"), open(os.path.join(other, "scheduler", "scheduler_config.json"), "w"))
    with pytest.raises(L.OmgHipError, match="algorithm_type"):
        compat.LoraMultiConceptPipeline.from_pretrained(other, torch_dtype=torch.float16, variant="fp16")
