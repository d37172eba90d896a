#!/usr/bin/env python
"""bench.py — images/sec of OMG's stage-2 denoising call on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one batch of `--images-per-step` (default 8) independent requests, each a complete stage-2 call of the
reference's pipeline at BASELINE config 2 (BASELINE configs[3] serves batch=32 over 8 GPUs, 4 per GPU; 8 per GPU makes the
tile counts of the 1280-wide layers whole rounds of 256 CUs — +3 % images/s over 4, measured);
the requests advance in lock-step through ONE batched UNet forward per denoising step, bitwise equal to running them one
at a time (tests/test_pipeline_gpu.py).  Per request:
SDXL-base UNet (2.567 B params, random init), 1024x1024 (latent 128x128), 50 DDIM steps, global batch
[unc0,unc1,cond0,cond1], prompt-to-prompt controller installed (140 attention layers), 2 concepts with
rank-64 LoRAs on every attention/FF Linear, overlapping region masks, fusion for steps i > 15
(= 200 main + 136 concept UNet sample-forwards, 2.273 PFLOP algorithmic).
Inputs are resident in HBM before the timed region.  N > 1: one process per GPU, each rank runs K steps
(weak scaling), final latents all-gathered over RCCL per step; value = N * K * images_per_step / max-over-ranks time.

Prints ONE JSON line (rank 0).  "value" is the reference's as-executed work (336 sample-forwards per image).  A plain run does
only what that figure needs: set up, W warm-up steps, the K timed steps, --dump-outputs, the line.  `--full` adds everything
else: "power" (socket power / shader clock polled during the timed region) and, after that region, "value_dedup" (the
same images with the exactly redundant sample-forwards of steps 0..15 executed once; bitwise the same latents,
tests/test_pipeline_gpu.py; timed in a second, shorter region), "roofline" (GEMM/conv kernel family, MFMA-bound, HIP-event
timed in an instrumented pass of one plain + one fused denoising step; --by-shape) and "cpu_baseline" (the fp32 oracle on the
host cores, bounded sample, extrapolated).  The --no-* switches and --dedup-steps / --by-shape select among these.

`--dump-outputs DIR` writes what the last timed step computed (rank 0's requests) as DIR/<name>.npy in float32: `latents` (requests, 2 samples,
4, h, w) and `images` (decoded images, requests x 2 samples x 3 x H x W; absent with --no-vae).  An output of more than 2^21 values is
written as a fixed, seeded sample instead: `<name>_sample` (the values) and `<name>_sample_index` (their flat indices, float64).
The inputs and weights are seeded: with the same arguments two runs compute the same things, so two builds compare output for output.

`python bench.py --gpus N` without a torch.distributed environment re-launches itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` (one rank per GPU).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

SAMPLE_FWD_TFLOP = 6.765          # algorithmic FLOPs of one UNet sample-forward @1024^2
CACHED_KV_TFLOP = 0.0525          # of which: cross-attention K / V projections of the constant 77-token context (60 blocks x 1280 + 10 x 640
                                  # channels, 4 * 77 * 2048 * C each) — computed once per call and cached, NOT executed per forward
N_MAIN, N_CONCEPT = 200, 136      # sample-forwards per stage-2 image (50 x B4 main, 34 x 2 concepts x B2)
PEAK_TFLOPS = 2500.0              # dense bf16/fp16 MFMA peak, MI355X (MI355X_MICROARCH.md)


def cpu_baseline(args):
    """Oracle (CPU restatement of the reference path) timed on the host cores: ONE fp32 UNet sample-forward at full SDXL width and
    at the workload's own shape (latent 128 = the 1024^2 image; ~45 s on the GPU box's 128 threads), extrapolated by the forward
    count to one image.  SURVEY §8d's sample (a plain + a fused full-shape step = 12 such forwards, ~9 min) does not fit a
    default run; --cpu-latent 64 times the 512^2 forward instead (~10 s, scaled by the analytic FLOP ratio)."""
    from oracle import unet as ou
    torch.manual_seed(0)
    ocfg = ou.UNetConfig.sdxl()
    sd = {}
    for k, shp in ou.param_shapes(ocfg).items():
        fan_in = 1
        for d in shp[1:]:
            fan_in *= d
        sd[k] = torch.empty(shp).normal_(0, fan_in ** -0.5) if len(shp) >= 2 else torch.ones(shp)
    L = args.cpu_latent
    x = torch.randn(1, 4, L, L)
    ctx = torch.randn(1, 77, 2048)
    te = torch.randn(1, 1280)
    tid = torch.tensor([[1024.0, 1024.0, 0, 0, 1024.0, 1024.0]])
    with torch.no_grad():
        t0 = time.perf_counter()
        ou.unet_forward(sd, ocfg, x, 981, ctx, te, tid)
        dt = time.perf_counter() - t0
    fl = {128: 6.765, 64: 1.590}.get(L)
    tf_per_s = fl / dt
    sec_per_image = (N_MAIN + N_CONCEPT) * SAMPLE_FWD_TFLOP / tf_per_s
    return {"value": 1.0 / sec_per_image, "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"1 fp32 UNet sample-forward (B=1, latent {L}x{L}, {fl} TFLOP) in {dt:.1f} s = {tf_per_s:.3f} TFLOP/s; "
                      f"extrapolated to the {N_MAIN + N_CONCEPT} x {SAMPLE_FWD_TFLOP} TFLOP of one image",
            "torch": torch.__version__}


class PowerSampler:
    """Socket power and shader clock during the timed region (rocm-smi polled from a side thread, rank 0 only): the MFMA peak
    the roofline is priced against assumes 2.4 GHz; under dense MFMA load the part sits at its power cap and clocks lower
    (profiles/r02_power_probe.log), so the line also carries the clock the kernels actually ran at."""
    def __init__(self, device_index, period=1.0):
        import threading
        self.dev, self.period, self.rows, self._stop = device_index, period, [], False
        self._th = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def parse(text):
        """One `rocm-smi -d N -c -P --showmaxpower --json` answer -> {"sclk": MHz, "w": W, "cap": W} (keys present when found)."""
        import re
        card = next(iter(json.loads(text).values()))
        row = {}
        for k, v in card.items():
            kl = k.lower()
            m = re.search(r"[-+]?\d+(\.\d+)?", str(v))
            if m is None:
                continue
            if "sclk clock speed" in kl:
                row["sclk"] = float(m.group())
            elif "max graphics package power" in kl:
                row["cap"] = float(m.group())
            elif "power (w)" in kl and "max" not in kl:
                row["w"] = float(m.group())
        return row

    def _run(self):
        import subprocess
        while not self._stop:
            try:
                o = subprocess.run(["rocm-smi", "-d", str(self.dev), "-c", "-P", "--showmaxpower", "--json"], capture_output=True, text=True, timeout=10).stdout
                row = self.parse(o)
                if row:
                    self.rows.append(row)
            except Exception:      # noqa: BLE001 - no rocm-smi, odd output: the line is simply reported without power
                pass
            time.sleep(self.period)

    def __enter__(self):
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        self._th.join(timeout=15)

    def summary(self):
        def avg(k):
            v = [r[k] for r in self.rows if k in r]
            return sum(v) / len(v) if v else None
        return {"avg_w": avg("w"), "cap_w": avg("cap"), "avg_sclk_mhz": avg("sclk"), "samples": len(self.rows), "nominal_sclk_mhz": 2400.0,
                "source": "rocm-smi -c -P polled once a second during the timed region"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per GPU (each --images-per-step requests)")
    ap.add_argument("--warmup", type=int, default=1, help="untimed warm-up steps per GPU")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp8"],
                    help="fp8 = BASELINE configs[4]'s arithmetic: the transformer Linear layers on the MX-fp8 MFMA (omg_gemm_mx8), "
                         "everything else fp16 as in the default mode; NOT the headline configuration")
    ap.add_argument("--scheduler", default="ddim", choices=["ddim", "euler"])
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--full", action="store_true", help="also measure power / clock (during the timed region), value_dedup, the roofline and the CPU "
                    "baseline (after it), each unless its --no-* switch is given; without it the run measures the headline figure only")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-latent", type=int, default=128, choices=[64, 128])
    ap.add_argument("--dedup-steps", type=int, default=-1, help="with --full: steps of the second timed region (value_dedup); -1 = min(--steps, 2), 0 = skip")
    ap.add_argument("--tiny", action="store_true", help="debug: tiny UNet (NOT a valid benchmark)")
    ap.add_argument("--images-per-step", type=int, default=8, help="independent requests run in lock-step per step (one batched UNet forward)")
    ap.add_argument("--by-shape", default="", help="with --full: also write the roofline leg's per-shape table (ms per bench step, TF/s) to this file")
    ap.add_argument("--no-vae", action="store_true", help="stop at the latents (skip the VAE decode that ends the reference's stage-2 call)")
    ap.add_argument("--vae-16bit", action="store_true", help="decode in bf16 storage instead of the reference's fp32 up blocks (faster, NOT the reference's precision)")
    ap.add_argument("--fp8-linear-only", action="store_true", help="with --dtype fp8: keep every convolution in fp16 (round-2 first fp8 line)")
    ap.add_argument("--fp8-classes", default="all", help="with --dtype fp8: which layer classes run on the MX-fp8 MFMA — a preset of omg_amd.unet.MX8_PRESETS "
                    "(all | safe | none) or a comma list of omg_amd.unet.MX8_CLASSES (profiles/r04_mx8_sensitivity.json is the per-class error table)")
    ap.add_argument("--no-power", action="store_true", help="with --full: do not poll rocm-smi for power / clock during the timed region")
    ap.add_argument("--no-graph", action="store_true", help="run the step loop eagerly instead of replaying captured hipGraphs")
    ap.add_argument("--shard", default="images", choices=["images", "concept"],
                    help="N > 1 only.  images (default, throughput, weak scaling): every rank runs its own requests, one all_gather of the final latents. "
                         "concept (LATENCY of one batch, strong scaling; north_star's 'independent per-concept UNet passes shard across the GPUs'): every "
                         "rank is handed the SAME requests, a step's forward units (main block, one [unc, cond] pair per masked concept) are split over "
                         "the ranks and one all_gather per step exchanges the noise predictions (omg_amd.parallel.ConceptShard)")
    ap.add_argument("--config3", action="store_true",
                    help="BASELINE configs[3]'s own shape: batch 32 over 8 GPUs = 4 requests per GPU and step (--images-per-step 4); the default 8 is the throughput optimum")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write the last timed step's latents and decoded images to DIR/<name>.npy "
                    "(float32; outputs above 2^21 values as a fixed, seeded sample)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full and (args.by_shape or args.dedup_steps > 0):
        ap.error("--by-shape and --dedup-steps measure beyond the headline figure: add --full")
    if args.config3:
        args.images_per_step = 4

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher (one rank per GPU over RCCL), as the N > 1 contract describes
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.execv(sys.executable, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
                                  "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:])

    from omg_amd import controller as pc, ops, parallel
    from omg_amd.pipeline import LoraMultiConceptPipeline, revise_regionally_controlnet_forward
    from omg_amd.schedulers import make_scheduler
    from omg_amd.synthetic import c2_inputs, c2_masks, make_concept_models
    from omg_amd.unet import UNet2DConditionModel, UNetConfig

    rank, world, local = parallel.init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16

    cfg = UNetConfig.tiny() if args.tiny else UNetConfig.sdxl()
    unet = UNet2DConditionModel(cfg, dtype=dt, device=dev).init_synthetic_(seed=0)
    fp8_classes = ()
    if args.dtype == "fp8":
        from omg_amd.unet import MX8_PRESETS
        fp8_classes = tuple(MX8_PRESETS[args.fp8_classes]) if args.fp8_classes in MX8_PRESETS else tuple(c for c in args.fp8_classes.split(",") if c)
        if args.fp8_linear_only:
            fp8_classes = tuple(c for c in fp8_classes if not c.startswith("conv"))
        unet.set_precision_classes(fp8_classes)
    HW = cfg.sample_size * 8
    P = "a man and a woman walking on the street"
    ctl = pc.AttentionReplace([P, P], 50, cross_replace_steps={"default_": 1.0}, self_replace_steps=0.4,
                              width=HW // 32, height=HW // 32, device=dev, dtype=dt)        # inference_lora.py:156,247
    _quiet(revise_regionally_controlnet_forward, unet, ctl)       # the installer prints like the reference's; stdout must stay ONE JSON line
    concept = make_concept_models(unet, n_concepts=2, rank=64 if not args.tiny else 8)
    pipe = LoraMultiConceptPipeline(unet, make_scheduler(args.scheduler))
    vae = None
    if not args.no_vae:           # the tail of the reference's call: vae.decode(latents / scaling_factor) + postprocess (lora_pipeline.py:635-661)
        from omg_amd.vae import AutoencoderKLDecoder, VaeConfig
        # as the reference decodes (upcast_vae, lora_pipeline.py:639-652): pipeline dtype for post_quant_conv / conv_in / mid block, fp32 up blocks;
        # --vae-16bit: everything in bf16 storage (fp32 accumulate), the labelled faster option
        vae = AutoencoderKLDecoder(VaeConfig.tiny() if args.tiny else VaeConfig.sdxl(), dtype=torch.bfloat16 if args.vae_16bit else dt, device=dev,
                                   upcast=not args.vae_16bit).init_synthetic_(seed=1)
    masks = c2_masks(HW, HW, device=dev)
    n_steps = args.warmup + args.steps
    ips = args.images_per_step
    by_concept = args.shard == "concept" and world > 1
    cshard = parallel.ConceptShard() if by_concept else None
    inputs = []
    for i in range(n_steps):                                                                       # resident in HBM
        reqs = []
        for j in range(ips):
            # images: every rank has its own requests; concept: all ranks share them (the batch is split inside the step)
            r = c2_inputs(unet, seed=((0 if by_concept else rank) * 1000 + i) * 16 + j, height=HW, width=HW)
            r["region_masks"] = masks
            reqs.append(r)
        inputs.append(reqs)

    def run_step(reqs, dedup=False, keep=None):
        """One bench step = `ips` complete stage-2 calls (independent requests batched through the UNet in lock-step).
        `keep`: a list that receives every decoded image pair (--dump-outputs)."""
        ctl.reset()                                                                   # inference_lora.py:274
        lat = pipe.generate_many(reqs, height=HW, width=HW, num_inference_steps=args.denoise_steps, guidance_scale=7.5,
                                 cross_attention_kwargs={"scale": 0.8}, controller=ctl, concept_models=concept, stage=2,
                                 lora_list=["concept0", "concept1"], styleL=False, use_graph=not args.no_graph, dedup=dedup and not by_concept,
                                 concept_shard=cshard)
        if vae is not None:                                                           # both images of every request, two at a time
            for j in (range(lat.shape[0]) if not by_concept else parallel.shard_indices(lat.shape[0], rank, world)):      # concept: the decodes are split too
                img = vae.decode_latents(lat[j])
                if keep is not None:
                    keep.append(img)
            assert img.shape[-1] == lat.shape[-1] * 2 ** (len(vae.config.block_out_channels) - 1)
        return lat

    def gather(lat):
        if by_concept:                     # every rank already holds every request's latents (replicated state): nothing to exchange
            return lat[:, 1].contiguous()
        return parallel.gather_latents(lat[:, 1].contiguous(), world * ips, rank, world)

    for i in range(args.warmup):
        lat = run_step(inputs[i])
        gather(lat)
    sampler = PowerSampler(local) if rank == 0 and args.full and not args.no_power else None
    parallel.barrier()
    torch.cuda.synchronize()
    if sampler is not None:
        sampler.__enter__()
    kept = []                                                                                    # --dump-outputs: the last step's images
    t0 = time.perf_counter()
    for i in range(args.warmup, n_steps):
        lat = run_step(inputs[i], keep=kept if args.dump_outputs and i == n_steps - 1 else None)
        allimg = gather(lat)                                                                     # the deliverable is images[1]
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    el = parallel.max_over_ranks(time.perf_counter() - t0, dev)
    if sampler is not None:
        sampler.__exit__()
    assert torch.isfinite(allimg).all()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"latents": lat, "images": torch.stack(kept) if kept else None})
    del kept
    job_images = ips if by_concept else world * ips          # concept: ONE batch is split over the ranks (strong scaling)
    value = job_images * args.steps / el

    # second timed region: the same requests with the exactly redundant forwards executed once (same barrier / sync bracket)
    n_dd = min(args.steps, 2) if args.dedup_steps < 0 else min(args.dedup_steps, n_steps)
    if by_concept or not args.full:
        n_dd = 0                                              # concept: the twin regime and the unit split are alternatives
    dedup = None
    if n_dd > 0:
        lat_full = lat
        lat_dd = run_step(inputs[n_steps - 1], dedup=True)          # warm-up of the dedup engine (captures its step graphs)
        same = bool(torch.equal(lat_dd, lat_full))                    # same inputs as the last timed step: must be the same bits
        parallel.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps - n_dd, n_steps):
            lat = run_step(inputs[i], dedup=True)
            parallel.gather_latents(lat[:, 1].contiguous(), world * ips, rank, world)
        torch.cuda.synchronize()
        parallel.barrier()
        torch.cuda.synchronize()
        el_dd = parallel.max_over_ranks(time.perf_counter() - t0, dev)
        n_twin = min(16, args.denoise_steps)                          # steps 0..15 precede the first fused step (i > 15)
        dedup = {"value": world * ips * n_dd / el_dd, "steps": n_dd, "ms_per_step": 1000.0 * el_dd / n_dd,
                 "sample_forwards_executed": N_MAIN + N_CONCEPT - 2 * n_twin, "sample_forwards_reference": N_MAIN + N_CONCEPT,
                 "latents_bitwise_equal_to_full_run": same,
                 "what": "steps 0..15 of a stage-2 call: samples 0 and 1 share latents and prompts (lora_pipeline.py:397-409, :568), so "
                         "[unc, cond] runs once per request and is written to both samples"}

    out = {"metric": "images/sec @ SDXL 1024^2 50-step, 2-concept mask fusion", "value": value, "unit": "images/sec",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * el / args.steps,
           "value_dedup": dedup["value"] if dedup else None, "dedup": dedup,
           "higher_is_better": True, "scaling": "strong" if by_concept else "weak", "vs_baseline": None,
           "dtype": ("fp8 (OCP MX e4m3 operands, fp32 accumulate) on the layer classes " + "+".join(fp8_classes)
                     + "; fp16 elsewhere; measured loop tolerance vs the fp32 oracle (50-step stage-2 trajectory, random-weight SDXL topology at reduced width: "
                       "profiles/r04_mx8_sensitivity.json, r04_error_growth_mx8.json): every class: rms error 0.10, max 0.40 of the latent rms, flat after step 10; "
                       "preset 'safe' (cross_q+cross_out+ff_out): rms 0.031, max 0.11; fp16 path: 1.5e-3 / 5.3e-3; no class dominates — the ten add in quadrature") if args.dtype == "fp8"
                    else (args.dtype + (" (storage and MFMA operands; fp32 accumulate; = the reference's own torch_dtype, inference_lora.py:153-159).  Measured tolerance per "
                                        "UNet forward at full size vs the fp32 oracle: rms 1.09e-3, max 4.9e-3 of O(1) outputs — the reference's own fp16 eager execution, "
                                        "emulated op by op in the oracle, sits at 1.23e-3 / 5.1e-3 (profiles/r04_fullsize_forward_vs_oracles.json); north_star's 1e-3 is met in rms, "
                                        "not in max, by either" if args.dtype == "fp16" else "")),
           "data": "synthetic",
           "config": {"workload": "BASELINE configs[1]: SDXL-base 1024x1024, %d %s steps, 2 concepts + 2 rank-64 LoRAs, masked "
                                  "attention fusion (i>15), p2p controller; one stage-2 call per image (masks given)" % (args.denoise_steps, args.scheduler.upper()),
                      "global_batch": job_images, "images_per_step_per_gpu": ips if not by_concept else ips / world, "main_batch": 4 * ips, "concept_batch": 4 * ips, "accounting": "stage-2 only, as executed by the reference "
                      "(200 main + 136 concept sample-forwards = 2.273 PFLOP/image; 2.255 PFLOP executed per forward pass count, the cross-attention K / V "
                      "projections of the constant text context being cached per call); no redundancy shortcuts",
                      "vae_decode": "skipped (--no-vae)" if args.no_vae else ("both 1024^2 images of every request decoded inside the timed region, "
                                     + ("bf16 storage / fp32 accumulate (--vae-16bit)" if args.vae_16bit else "as the reference's upcast decode: fp16 post_quant / conv_in / mid block, fp32 up blocks on the f32-input MFMA")
                                     + "; +10.5 TFLOP per request, not counted in the FLOP accounting"),
                      "parallelism": (f"concept-shard over {world} ranks: per step the main block and the concept pairs of the {ips} request(s) are split "
                                      f"over the ranks, one all_gather of the noise predictions per step (latency mode)") if by_concept else f"dp{world}",
                      "tiny_debug": bool(args.tiny),
                      "step_loop": "eager" if args.no_graph else "hipGraph replay (3 captured step regimes)", "lora": "merged weight slots, "
                      "main + concept samples of all requests batched per fused step (8 samples per request)"},
           "latency_s_per_batch": (el / args.steps) if by_concept else None,
           "end_to_end_tflops_per_gpu": (N_MAIN + N_CONCEPT) * SAMPLE_FWD_TFLOP * value / world if not args.tiny else None,
           # the same with the cached cross-attention K / V projections (0.78 % of a forward) taken out: what the GPU executed
           "end_to_end_tflops_per_gpu_executed": (N_MAIN + N_CONCEPT) * (SAMPLE_FWD_TFLOP - CACHED_KV_TFLOP) * value / world if not args.tiny else None}

    if sampler is not None:
        out["power"] = sampler.summary()
    if rank == 0 and args.full and not args.no_roofline:
        # instrumented eager passes: HIP events around every GEMM/conv/attention launch of 2 plain and of 2 fused denoising
        # steps, combined with the weights of the timed workload (fusion fires for steps i > 15: 16 plain + 34 fused of 50)
        def instrumented(fusion_start):
            prof = ops.KernelProfiler()
            ops.set_profiler(prof)
            ctl.reset()
            pipe.generate_many(inputs[0], height=HW, width=HW, num_inference_steps=2, guidance_scale=7.5,
                               cross_attention_kwargs={"scale": 0.8}, controller=ctl, concept_models=concept, stage=2,
                               lora_list=["concept0", "concept1"], styleL=False, fusion_start=fusion_start)
            ops.set_profiler(None)
            torch.cuda.synchronize()
            return prof.summary(), dict(prof.by_tag())
        (sp, tp), (sf, tf) = instrumented(99), instrumented(-1)
        vae_fam = None
        if vae is not None:      # the decode of one request's two images, the same way (it runs once per image pair inside the timed region)
            prof = ops.KernelProfiler()
            ops.set_profiler(prof)
            vae.decode_latents(lat[0])
            ops.set_profiler(None)
            torch.cuda.synchronize()
            vs = prof.summary()
            if "gemm_f32" in vs and vs["gemm_f32"]["ms"] > 0:
                vae_fam = {"kernel": "conv_f32_kernel (fp32 up blocks of the upcast VAE decode, v_mfma_f32_32x32x2_f32)", "achieved": vs["gemm_f32"]["flops"] / (vs["gemm_f32"]["ms"] * 1e-3) / 1e12,
                           "peak": 157.0, "unit": "TFLOP/s", "ms_per_step": vs["gemm_f32"]["ms"] * ips}
                vae_fam["frac"] = vae_fam["achieved"] / vae_fam["peak"]
        n_f = max(0, args.denoise_steps - 16)
        n_p = args.denoise_steps - n_f
        def comb(kind, key):
            return (n_p * sp[kind][key] + n_f * sf[kind][key]) / 2.0
        fam, peak = ("gemm_mx8", 5000.0) if args.dtype == "fp8" else ("gemm", PEAK_TFLOPS)
        g_ms, g_fl, g_n = comb(fam, "ms"), comb(fam, "flops"), comb(fam, "launches")
        a_ms, a_fl = comb("attn", "ms"), comb("attn", "flops")
        ach = g_fl / (g_ms * 1e-3) / 1e12
        # HBM-side bytes cannot be counted from inside this process: the committed rocprofv3 --pmc measurement of the dominant GEMM
        # shape by tools/pmc_traffic.py (method and gfx950 correction recorded in the file) is reported — the newest round's file
        traffic, traffic_note = None, "no PMC measurement committed"
        tag = "fp8" if args.dtype == "fp8" else "fp16"
        tfile = next((f for f in (f"r06_pmc_traffic_{tag}.json", f"r05_pmc_traffic_{tag}.json", f"r04_pmc_traffic_{tag}.json", f"r03_pmc_traffic_{tag}.json") if os.path.exists(os.path.join(ROOT, "profiles", f))), "")
        try:      # tools/pmc_traffic.py wrote it from rocprofv3 --pmc passes of the kernel this line's roofline names
            with open(os.path.join(ROOT, "profiles", tfile)) as f:
                pm = json.load(f)
            traffic = pm["traffic_bytes_per_launch"]
            traffic_note = ("bytes per launch of the largest GEMM (%s; %.2f GB algorithmic) from rocprofv3 --pmc FETCH_SIZE (x2 on gfx950) "
                            "+ WRITE_SIZE, separate passes: profiles/%s" % (pm["shape"], (pm["algorithmic_read_bytes"] + pm["algorithmic_write_bytes"]) / 1e9, tfile))
        except (OSError, KeyError, ValueError):
            pass
        kname = ("gemm_mx8_kernel (transformer Linear layers + resnet convolutions, MX-fp8 operands on v_mfma_scale_f32_32x32x64_f8f6f4, per-sample weight slots)"
                 if args.dtype == "fp8" else "gemm_kernel_v12 (256x256 tile, ring K loop, persistent walk) / gemm_kernel_v13 (256x320 tile) / gemm_kernel_v7 (128x320 conv tile) / gemm_kernel_v6 / gemm_kernel "
                 "(Linear + implicit-GEMM conv, per-sample weight slots)")
        out["roofline"] = {"bound": "mfma", "kernel": kname,
                           "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": traffic,
                           "traffic_note": traffic_note,
                           "launches_per_step": g_n, "avg_launch_us": 1e3 * g_ms / g_n, "avg_launch_gflop": g_fl / g_n / 1e9,
                           "gemm_ms_per_step": g_ms,
                           "sample": f"HIP events around each launch (eager), 2 plain + 2 fused denoising steps weighted {n_p}:{n_f} as in the timed workload",
                           "attn_kernel": {"achieved": a_fl / (a_ms * 1e-3) / 1e12, "ms_per_step": a_ms}}
        # every kernel family of the step, each against ITS peak (`frac` above stays the GEMM family, for continuity with rounds 1-4)
        a_ach = a_fl / (a_ms * 1e-3) / 1e12
        out["roofline"]["families"] = {
            fam: {"kernel": kname, "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "ms_per_step": g_ms, "share_of_flops": g_fl / (g_fl + a_fl)},
            "attention": {"kernel": "attn_fwd_kernel7 (self-attention: K / row-major V tiles by LDS-DMA, swapped S^T = K Q^T, probability borrowing) / attn_fwd_kernel6 "
                                    "(cross-attention: K / V^T resident, memory-bound)", "achieved": a_ach, "peak": PEAK_TFLOPS, "unit": "TFLOP/s", "frac": a_ach / PEAK_TFLOPS,
                          "ms_per_step": a_ms, "share_of_flops": a_fl / (g_fl + a_fl)}}
        if vae_fam is not None:
            out["roofline"]["families"]["vae_f32"] = vae_fam
        e2e = out.get("end_to_end_tflops_per_gpu")
        if e2e:      # algorithmic FLOPs of the whole step (2.273 PF per image) / wall time, against the 16-bit (fp8: the fp8) dense peak
            out["roofline"]["end_to_end_frac"] = e2e / peak
        sclk = (out.get("power") or {}).get("avg_sclk_mhz")
        if sclk:      # the same fraction against the MFMA peak at the clock the part held during the timed region
            out["roofline"]["frac_at_measured_clock"] = ach / (peak * sclk / 2400.0)
        if args.dtype == "fp8":      # the 16-bit GEMM family still runs the convolutions (and the K/V, embedding Linears)
            c_ms, c_fl = comb("gemm", "ms"), comb("gemm", "flops")
            out["roofline"]["fp16_gemm_family"] = {"achieved": c_fl / (c_ms * 1e-3) / 1e12, "ms_per_step": c_ms, "peak": PEAK_TFLOPS}
        if args.by_shape:
            rows = []
            for key in set(tp) | set(tf):
                z = dict(launches=0, ms=0.0, flops=0.0)
                a, b = tp.get(key, z), tf.get(key, z)
                rows.append((key, *[(n_p * a[k] + n_f * b[k]) / 2.0 for k in ("ms", "flops", "launches")]))
            rows.sort(key=lambda r: -r[1])
            tot = sum(r[1] for r in rows)
            with open(args.by_shape, "w") as f:
                f.write(f"# per bench step ({ips} images): kind, shape tag, launches, ms, share, TF/s; total {tot:.1f} ms\n")
                for key, ms, fl, n in rows:
                    f.write(f"{key[0]:5s} {str(key[1]):56s} n={n:7.0f} ms={ms:9.2f} ({100 * ms / tot:4.1f}%) {fl / ms / 1e9 if ms else 0:7.1f} TF/s\n")
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:      # the host-core baseline is reported at N = 1 only
        out["cpu_baseline"] = cpu_baseline(args)
        # BASELINE configs[0] — the reference's own CPU-runnable case (512^2, 10 DDIM steps, 1 concept, no LoRA) — timed FOR REAL at full width, no
        # extrapolation: the oracle's 10-step stage-2 call on the GPU box's host cores (tests/test_config0_fullwidth_gpu.py, ~4 minutes per stage: too long
        # for a default run, so the tracked measurement is quoted with its source; SURVEY §8(d) "time C1 end-to-end for real")
        try:
            with open(os.path.join(ROOT, "profiles", "r06_config0_fullwidth_loop.json")) as f:
                c0 = json.load(f)
            out["cpu_baseline_config0"] = dict(c0["cpu_baseline_config0"], source="profiles/r06_config0_fullwidth_loop.json (recorded by tests/test_config0_fullwidth_gpu.py "
                                               "on a GPU box of this pool; not re-timed in this run)", hip_final_error_vs_fp32_oracle=c0["final"]["hip_vs_fp32_oracle"],
                                               reference_fp16_arithmetic_vs_fp32_oracle=c0["final"]["fp16_oracle_vs_fp32_oracle"])
        except (OSError, KeyError, ValueError):
            pass
    if rank == 0:
        print(json.dumps(out))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        parallel.barrier()     # orderly shutdown: the other ranks wait for rank 0's instrumented passes, then RCCL is torn down
        torch.distributed.destroy_process_group()


DUMP_MAX_VALUES = 1 << 21       # per output: 8 MB of float32 whole, or a sample of this many values + their float64 indices (<= 48 MB for two)


def dump_outputs(dirname, outputs):
    """--dump-outputs: every output as DIR/<name>.npy in float32; one of more than DUMP_MAX_VALUES values as a fixed, seeded sample
    (the same flat indices for the same shape) in <name>_sample.npy, with the indices in <name>_sample_index.npy (float64, exact)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, t in outputs.items():
        if t is None:
            continue
        flat = t.detach().reshape(-1)
        if flat.numel() <= DUMP_MAX_VALUES:
            np.save(os.path.join(dirname, f"{name}.npy"), t.detach().float().cpu().numpy())
            continue
        idx = torch.randint(flat.numel(), (DUMP_MAX_VALUES,), generator=torch.Generator().manual_seed(0)).sort().values
        np.save(os.path.join(dirname, f"{name}_sample.npy"), flat[idx.to(flat.device)].float().cpu().numpy())
        np.save(os.path.join(dirname, f"{name}_sample_index.npy"), idx.double().numpy())


def _quiet(fn, *a):
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


if __name__ == "__main__":
    main()
