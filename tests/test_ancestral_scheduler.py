"""CPU tests (-m "not gpu"): the stochastic steps — Euler-ancestral (omg_amd.schedulers.EulerAncestralDiscreteScheduler) and DDIM with
eta > 0 — their (n, 4) tables against the literal stateful restatement in tests/_ancestral_oracle.py, the identities of the ancestral
split, DDIM's eta = 0 table byte for byte, the host step() with a seeded generator, the options that are refused, the drop-in surface of
omg_amd.compat and the C-ABI entry point of the noise step kernel."""
import json
import os

import numpy as np
import pytest
import torch

from omg_amd import _lib as L
from omg_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                                is_stochastic, make_scheduler)
from tests import _ancestral_oracle as ao

SDXL_SCHEDULER = {"_class_name": "EulerDiscreteScheduler", "_diffusers_version": "0.19.0.dev0", "beta_end": 0.012,
                  "beta_schedule": "scaled_linear", "beta_start": 0.00085, "clip_sample": False, "interpolation_type": "linear",
                  "num_train_timesteps": 1000, "prediction_type": "epsilon", "sample_max_value": 1.0, "set_alpha_to_one": False,
                  "skip_prk_steps": True, "steps_offset": 1, "timestep_spacing": "leading", "trained_betas": None, "use_karras_sigmas": False}
NS = [1, 2, 8, 25, 50]


def table_run(cx, ce, cz, x, eps_seq, z_seq):
    """the noise step kernel's arithmetic in float64: x' = cx x + ce eps + cz z"""
    for i, (e, z) in enumerate(zip(eps_seq, z_seq)):
        x = cx[i] * x + ce[i] * e + cz[i] * z
    return x


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def sequences(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((2, 3, 5)), [rng.standard_normal((2, 3, 5)) for _ in range(n)], [rng.standard_normal((2, 3, 5)) for _ in range(n)]


@pytest.mark.parametrize("n", NS)
def test_euler_ancestral_table_matches_the_restatement(n):
    x0, eps_seq, z_seq = sequences(n, n)
    sch = EulerAncestralDiscreteScheduler.from_config(SDXL_SCHEDULER)
    sch.set_timesteps(n)
    ref = ao.EulerAncestral(n, z_seq)
    assert np.array_equal(sch.timesteps.numpy(), ref.timesteps.astype(np.float32))
    assert np.allclose(sch.sigmas, ref.sigmas, rtol=1e-14, atol=0)
    x = x0 * 3.0
    for i, e in enumerate(eps_seq):
        x = ref.step(e, i, x)
    assert rel(table_run(sch.cx, sch.ce, sch.cz, x0 * 3.0, eps_seq, z_seq), x) <= 1e-12
    tab = sch.coef_table("cpu")
    assert tab.shape == (n, 4) and tab.dtype == torch.float32
    want = np.stack([sch.cx, sch.ce, np.append(sch.cin[1:], 1.0), sch.cz], axis=1).astype(np.float32)
    assert np.array_equal(tab.numpy(), want)
    assert np.allclose(sch.cin, 1 / np.sqrt(ref.sigmas[:-1] ** 2 + 1), rtol=1e-14, atol=0)


@pytest.mark.parametrize("n", NS)
def test_ancestral_split_of_the_variance(n):
    """sigma_up^2 + sigma_down^2 = sigma_to^2 at every step, and the last step adds no noise"""
    sch = make_scheduler("euler_a")
    sch.set_timesteps(n)
    s_to = sch.sigmas[1:]
    assert np.allclose(sch.sigma_up ** 2 + sch.sigma_down ** 2, s_to ** 2, rtol=1e-12, atol=1e-15)
    assert (sch.sigma_up[:-1] > 0).all() and sch.sigma_up[-1] == 0.0 and sch.sigma_down[-1] == 0.0
    assert sch.coef_table("cpu")[-1, 3].item() == 0.0
    assert np.array_equal(sch.ce[-1:], -sch.sigmas[n - 1: n]), "the last step lands on sigma = 0: x - sigma eps"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_eta_table_matches_the_restatement(n, eta):
    x0, eps_seq, z_seq = sequences(n, 7 * n)
    sch = DDIMScheduler()
    sch.set_timesteps(n)
    ref = ao.DDIMEta(n, eta, z_seq)
    assert np.array_equal(sch.timesteps.numpy(), ref.timesteps)
    x = x0
    for i, e in enumerate(eps_seq):
        x = ref.step(e, i, x)
    cx, ce, cz = sch.eta_coefficients(eta)
    assert rel(table_run(cx, ce, cz, x0, eps_seq, z_seq), x) <= 1e-12
    assert np.array_equal(sch.coef_table("cpu", eta=eta).numpy(), np.stack([cx, ce, np.ones(n), cz], axis=1).astype(np.float32))


@pytest.mark.parametrize("n", NS)
def test_ddim_eta_zero_is_todays_table_byte_for_byte(n):
    """the deterministic table as it was built before eta existed: (cx, ce, cin_next, 0)"""
    sch = DDIMScheduler()
    sch.set_timesteps(n)
    old = np.zeros((n, 4), dtype=np.float64)
    old[:, 0], old[:, 1] = sch.cx, sch.ce
    old[:-1, 2] = sch.cin[1:]
    old[-1, 2] = 1.0
    want = old.astype(np.float32).tobytes()
    assert sch.coef_table("cpu").numpy().tobytes() == want
    assert sch.coef_table("cpu", eta=0.0).numpy().tobytes() == want
    assert sch.coef_table("cpu", eta=1.0).numpy().tobytes() != want
    assert sch.coef_table("cpu", eta=0).numpy().tobytes() == want, "back to eta = 0: the cache is keyed by the table's bytes"


def test_ddim_eta_one_variance():
    n = 25
    sch = DDIMScheduler()
    sch.set_timesteps(n)
    ref = ao.DDIMEta(n, 1.0, None)
    ac, ratio = sch.alphas_cumprod, 1000 // n
    _, ce, cz = sch.eta_coefficients(1.0)
    for i, t in enumerate(sch.timesteps.tolist()):
        a_t = ac[t]
        a_p = ac[t - ratio] if t - ratio >= 0 else ac[0]
        var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        assert abs(cz[i] ** 2 - var) <= 1e-14 and abs(cz[i] ** 2 - ref.variance(i)) <= 1e-14
        assert abs(ce[i] - (np.sqrt(1 - a_p - var) - np.sqrt(a_p * (1 - a_t) / a_t))) <= 1e-14
    # eta = 1: the step's total variance around the data prediction is the DDPM posterior's, 1 - a_prev
    assert np.all(cz > 0) and np.all(cz ** 2 < 1 - sch._a_p)


@pytest.mark.parametrize("kind", ["euler_a", "ddim_eta"])
def test_host_step_draws_from_the_generator(kind):
    """diffusers' host API: step(..., generator=g) with a seeded CPU generator equals the table applied with the same draws
    (torch.randn float32, one per step, in step order)"""
    n = 8
    sch = make_scheduler("euler_a" if kind == "euler_a" else "ddim")
    sch.set_timesteps(n)
    kw = {} if kind == "euler_a" else {"eta": 1.0}
    tab = sch.coef_table("cpu", **kw).double()
    if kind == "euler_a":
        cx, ce, cz = sch.cx, sch.ce, sch.cz
    else:
        cx, ce, cz = sch.eta_coefficients(1.0)
    gen = torch.Generator().manual_seed(11)
    rng = torch.Generator().manual_seed(12)
    x0 = torch.randn(2, 4, 6, 5, generator=rng, dtype=torch.float64)
    eps_seq = [torch.randn(2, 4, 6, 5, generator=rng, dtype=torch.float64) for _ in range(n)]
    x = x0
    for t, e in zip(sch.timesteps, eps_seq):
        x = sch.step(e, t, x, generator=gen, **kw)[0]
    g2 = torch.Generator().manual_seed(11)
    zs = [torch.randn(2, 4, 6, 5, generator=g2, dtype=torch.float32).double() for _ in range(n)]
    want = table_run(cx, ce, cz, x0.numpy(), [e.numpy() for e in eps_seq], [z.numpy() for z in zs])
    assert rel(x.numpy(), want) <= 1e-12
    assert np.allclose(tab[:, 3].numpy(), cz, rtol=1e-6)
    if kind == "euler_a":
        with pytest.raises(ValueError):                 # stateful: one call per step, then set_timesteps again
            sch.step(eps_seq[0], sch.timesteps[0], x, generator=gen)
        sch.set_timesteps(n)
        assert torch.equal(sch.scale_model_input(x0, sch.timesteps[0]), x0 * float(sch.cin[0]))


def test_init_noise_sigma_and_schedule():
    for n in NS:
        a, e = EulerAncestralDiscreteScheduler(), EulerDiscreteScheduler()
        a.set_timesteps(n); e.set_timesteps(n)
        assert a.init_noise_sigma == e.init_noise_sigma == float(np.sqrt(a.sigmas.max() ** 2 + 1))
        assert torch.equal(a.timesteps, e.timesteps) and np.array_equal(a.sigmas, e.sigmas) and np.array_equal(a.cin, e.cin)
        ref = ao.EulerAncestral(n, None)
        assert abs(a.init_noise_sigma - ref.init_noise_sigma) <= 1e-12
    c = EulerAncestralDiscreteScheduler.from_config(SDXL_SCHEDULER).config
    assert (c["_class_name"], c["beta_schedule"], c["timestep_spacing"], c["steps_offset"]) == ("EulerAncestralDiscreteScheduler", "scaled_linear", "leading", 1)
    lin = EulerAncestralDiscreteScheduler(beta_schedule="linear", beta_start=0.0001, beta_end=0.02)
    assert np.allclose(lin.alphas_cumprod, np.cumprod(1 - np.linspace(0.0001, 0.02, 1000)), rtol=1e-14, atol=0)
    with pytest.raises(TypeError):
        c["steps_offset"] = 0                                   # read-only


@pytest.mark.parametrize("option,value", [("prediction_type", "v_prediction"), ("prediction_type", "sample"),
                                          ("timestep_spacing", "trailing"), ("timestep_spacing", "linspace"),
                                          ("beta_schedule", "squaredcos_cap_v2"), ("trained_betas", [0.1] * 1000),
                                          ("rescale_betas_zero_snr", True)])
def test_unsupported_options_are_refused_by_name(option, value):
    with pytest.raises(L.OmgHipError, match=option):
        EulerAncestralDiscreteScheduler.from_config(SDXL_SCHEDULER, **{option: value})


def test_unknown_keyword_and_ddim_options():
    with pytest.raises(TypeError):
        EulerAncestralDiscreteScheduler(use_karras_sigmas=True)
    d = DDIMScheduler()
    d.set_timesteps(5)
    with pytest.raises(L.OmgHipError, match="use_clipped_model_output"):
        d.step(torch.zeros(1), d.timesteps[0], torch.zeros(1), eta=1.0, use_clipped_model_output=True)
    with pytest.raises(ValueError):
        d.coef_table("cpu", eta=-0.5)


def test_which_steps_are_stochastic():
    assert is_stochastic(make_scheduler("euler_a")) and is_stochastic(make_scheduler("euler_a"), 0.0)
    assert is_stochastic(DDIMScheduler(), 1.0) and not is_stochastic(DDIMScheduler(), 0.0)
    for other in (EulerDiscreteScheduler(), DPMSolverMultistepScheduler()):
        assert not is_stochastic(other, 1.0), "eta is ignored by a scheduler whose step() does not take it"
    assert isinstance(make_scheduler("euler_a"), EulerAncestralDiscreteScheduler)


def test_install_exports_the_scheduler():
    from omg_amd import compat
    compat.install()
    try:
        import diffusers
        cls = diffusers.EulerAncestralDiscreteScheduler
        assert cls is EulerAncestralDiscreteScheduler
        s = cls.from_config(diffusers.EulerDiscreteScheduler().config)
        s.set_timesteps(20)
        assert len(s.timesteps) == 20 and s.config["_class_name"] == "EulerAncestralDiscreteScheduler"
    finally:
        compat.uninstall()


def test_from_pretrained_maps_an_ancestral_scheduler_config(tmp_path):
    """a checkpoint whose scheduler_config.json names EulerAncestralDiscreteScheduler gets it (it used to get Euler-discrete, silently)"""
    from omg_amd import compat
    from tests import _fake_hub as hub
    model = hub.write_sdxl_dir(str(tmp_path / "sdxl"))
    cfg = dict(SDXL_SCHEDULER, _class_name="EulerAncestralDiscreteScheduler", steps_offset=2)
    json.dump(cfg, open(os.path.join(model, "scheduler", "scheduler_config.json"), "w"))
    pipe = compat.LoraMultiConceptPipeline.from_pretrained(model, torch_dtype=torch.float16, variant="fp16")
    assert isinstance(pipe.scheduler, EulerAncestralDiscreteScheduler) and pipe.scheduler.config["steps_offset"] == 2
    other = hub.write_sdxl_dir(str(tmp_path / "sdxl_v"))
    json.dump(dict(cfg, prediction_type="v_prediction"), open(os.path.join(other, "scheduler", "scheduler_config.json"), "w"))
    with pytest.raises(L.OmgHipError, match="prediction_type"):
        compat.LoraMultiConceptPipeline.from_pretrained(other, torch_dtype=torch.float16, variant="fp16")


def test_abi_exports_the_noise_step():
    import subprocess
    assert "omg_fuse_cfg_step_noise" in L.SYMBOLS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omg_hip.h")).read()
    assert "int omg_fuse_cfg_step_noise(const omg_step_args* a, const float* z, int64_t z_step_stride, void* stream);" in header
    lib = L.lib()
    assert hasattr(lib, "omg_fuse_cfg_step_noise") and lib.omg_abi_version() == 6
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert " T omg_fuse_cfg_step_noise\n" in nm
