#!/usr/bin/env python3
"""Headline benchmark: user-sequences/sec of one full training step of the sequential recommender
(MovieLens-1M-shaped: V=3883 items, seq_len 200, d_model 128, 4 layers, sampled softmax / InfoNCE) on N
MI355X of one node, data-parallel over RCCL.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 8 --steps 20 --warmup 5          # launches its own 8 ranks (torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W                # ... or is launched as one of N ranks

One "step" = zero_grad -> gather+mask+BertEmbeddings -> 4 x BertLayer -> fused loss (all seven heads +
LogitsStatistics + dL/dtok, as the reference's training_step evaluates them, xfmr_rec/trainer.py:250-264) ->
encoder backward -> flat-gradient all-reduce (N > 1) -> AdamW, dropout 0.1 ON. `value` is measured with the batch
(3 x B x 200 int64) starting in page-locked HOST memory (SURVEY section 8d counts that copy into the metric: one
hipMemcpyAsync per batch on a copy stream one batch ahead, xfmr_rec_amd.data.PinnedBatchRing); `resident` repeats the
timed region on batches that already lie in HBM. Rank 0 prints ONE JSON line; see the task contract for the fields.

A plain run does only what `value` needs: set-up, the spin-up and --warmup steps, the --steps timed steps, the line.
`--full` adds the other figures (`resident`, `h2d_on_compute_stream`, `ragged`, `cold_start`, `roofline`, `cpu_baseline`),
each measured in steps of its own. `--dump-outputs DIR` writes what the last timed step handed its caller as DIR/<name>.npy
(float32): the train loss, every value the step logged and the flat parameter buffer after AdamW; the inputs are seeded,
so two builds run with the same arguments can be compared file by file.
Extra objects (--full):

  roofline     the DOMINANT kernel of the step = the one with the most GPU time per step (launch duration x launches per
               step; the top row of profiles/*_kernel_stats.md), chosen among the kernels this run times LIVE with HIP events
               on their launch stream: the four big kernels of an encoder layer (xfmr_encoder_cfg.profile_*: fused FFN
               forward, fused FFN backward dX chain, attention forward / backward; bound "hbm": ALGORITHMIC bytes per launch
               / duration against 8 TB/s) and the two passes of the fused loss (xfmr_loss_cfg.profile_*; bound "mfma":
               executed flops 2 or 4 * Np * Nd * H / duration against the dense bf16 MFMA peak). `frac` uses the duration
               with nothing beside the kernel (steps after the timed region with everything on one stream -- what a
               one-stream rocprofv3 trace shows); `*_overlapped` the duration inside the timed region. `kernels` lists all
               of them; `valu` prices the logging pass against the vector pipe it is bound by; `step` = executed flops of
               the whole step / ms_per_step; fields that come from a committed rocprof run carry a `source`.
  cpu_baseline the CPU oracle (oracle/, a restatement of the reference: 'port') timed on this host's cores on bounded
               samples: reference-faithful fp32 (the headline), bf16-autocast (the reference's default precision),
               reference-lean (train head only, GEMM-form logits) and BASELINE config 1 (ML-100K-shaped).
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import pathlib
import socket
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_HBM_TBPS = 8.0
METRIC = "user-sequences/sec (train step) MovieLens-1M seq200 d128 @1/2/4/8 GPU"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512,
                    help="sequences per GPU per step (SURVEY section 8d, config 2: per-GPU B in {32, 128, 512}; the "
                         "largest is the default -- a 288 GB part is sized for it; DESIGN.md lists all three)")
    ap.add_argument("--seq-len", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--inter", type=int, default=512)
    ap.add_argument("--items", type=int, default=3883)
    ap.add_argument("--loss", default="InfoNCELoss")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--lengths", default="dense", choices=["dense", "ml"])
    ap.add_argument("--lean", action="store_true", help="only the train head (not the reference's 7 + stats)")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ragged", action="store_true",
                    help="skip the `ragged` figures (profiling runs: rocprofv3 --pmc serialises every launch)")
    ap.add_argument("--overlap", choices=["auto", "on", "off"], default="auto",
                    help="logging heads on a side stream under the encoder backward: pays off once the logging pass is "
                         "long enough (B*L >= 51200: round 4 measured +1..2 %% at B=256, -1.3 %% at B=128); auto decides by that")
    ap.add_argument("--no-overlap", action="store_true", help=argparse.SUPPRESS)  # former default switch; no effect
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                    help="replay the step as one hipGraph (GraphedStep): auto = when the eager step would be bound by the "
                         "host's launch rate (B*L <= 32768 tokens, one process)")
    ap.add_argument("--heads", type=int, default=0, help="attention heads (default hidden/32: head size 32)")
    ap.add_argument("--negatives", default="in_batch", choices=["in_batch", "catalogue"],
                    help="catalogue = full-catalogue softmax (BASELINE config 4; SURVEY F9)")
    ap.add_argument("--preset", default=None, choices=["config1", "config2", "config3", "config4", "config5", "reference-default"],
                    help="the other BASELINE.json configs as sanity workloads (the bench line is config2, the default)")
    ap.add_argument("--spinup-steps", type=int, default=300,
                    help="untimed steps of the same workload BEFORE the --warmup steps (same count on every rank): a "
                         "fresh box can take > 100 ms of sustained load to reach its steady clocks; the cold rate "
                         "(--warmup steps only) is measured first and reported as `cold_start` (--full)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside `value` (resident / compute-stream H2D / ragged / cold-start rates, "
                         "the per-kernel roofline, the CPU baseline), each in steps of its own beside the timed region")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (loss, logged values, parameters after AdamW) as DIR/<name>.npy")
    ap.add_argument("--cpu-batch", type=int, default=4)
    ap.add_argument("--cpu-seconds", type=float, default=5.0,
                    help="time budget of EACH cpu_baseline variant beyond its 3 warm-up + 10 timed steps (up to 50 steps)")
    args = ap.parse_args(argv)
    presets = {
        # BASELINE configs[0]: MovieLens-100K-shaped, the reference's CPU-runnable case (the cpu_baseline's last variant)
        "config1": dict(items=1682, seq_len=50, hidden=64, layers=2, inter=256, batch=64),
        "config2": {},
        "config3": dict(loss="PairwiseLogisticLoss"),
        "config4": dict(items=27278, hidden=256, layers=6, inter=1024, batch=64, negatives="catalogue"),
        "config5": dict(items=1_000_000, seq_len=512, hidden=256, layers=4, inter=1024, batch=64,
                        loss="AlignmentContrastiveLoss"),
        # the reference's own config.yaml / ModelConfig defaults with the all-MiniLM (384-wide) item table
        "reference-default": dict(hidden=384, heads=12, layers=1, inter=48, seq_len=32, batch=32),
    }
    for k, v in presets.get(args.preset or "config2", {}).items():
        setattr(args, k, v)
    return args


# ----------------------------------------------------------------------------------------------- launching N ranks
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int, argv: list[str]) -> int:
    """`python bench.py --gpus N` started as ONE process: start N ranks of this script with torch.distributed.run (one
    process per GPU, rendezvous on 127.0.0.1) BEFORE anything in this process touches the GPU, relay their output
    (rank 0 prints the JSON line) and return the launcher's exit status -- non-zero if any rank failed."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(pathlib.Path(__file__).resolve()), *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.run(cmd, env=env).returncode


def dry_run(args) -> int:
    """XFMR_BENCH_DRY=1: the control flow of an N-rank run without a GPU -- rendezvous, barrier, one SUM all-reduce of
    a flat buffer, MAX-over-ranks timing, rank 0's line -- over gloo. Used by the CPU test of the self-launch."""
    import torch
    import torch.distributed as dist

    from xfmr_rec_amd import distributed as D

    rank, _local, world = D.init_process_group_from_env(backend="gloo")
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        return 2
    flat = torch.full((1000,), float(rank + 1))
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    D.allreduce_flat_grad_(flat)
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ok = bool((flat == world * (world + 1) / 2).all())
    if rank == 0:
        print(json.dumps({"metric": METRIC, "dry": True, "n_gpus": world, "allreduce_ok": ok, "value": None, "scaling": "weak",
                          "exchange": {"backend": "gloo (dry run; the GPU run uses torch.distributed 'nccl' = RCCL)",
                                       "rccl_world": world, "message_bytes": int(flat.numel()) * 4,
                                       "form": "one all-reduce after the backward"}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if ok else 1


# ----------------------------------------------------------------------------------------------------- inputs
def synth_batch(B, L, V, seed, lengths_mode):
    import torch

    g = torch.Generator().manual_seed(seed)
    if lengths_mode == "dense":
        lens = [L] * B
    else:  # MovieLens-1M-like: log-normal, clipped to [16, L]
        lens = torch.exp(torch.randn(B, generator=g) * 1.0 + 4.35).round().clamp(min(16, L), L).long().tolist()
    out = {k: torch.zeros(B, L, dtype=torch.int64) for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")}
    for b, n in enumerate(lens):
        for k in out:
            out[k][b, :n] = torch.randint(1, V + 1, (n,), generator=g)
    return out, lens


def unit_table(V, H, seed=1234):
    import torch

    g = torch.Generator().manual_seed(seed)
    t = torch.randn(V + 1, H, generator=g)
    t = t / t.norm(dim=-1, keepdim=True)
    t[0] = 0
    return t


DUMP_MAX_ELEMENTS = 8 << 20  # 32 MB of float32: the parameter buffer is the only array that can reach it


def dump_outputs(path, loss, logged, flat):
    """--dump-outputs: what the last timed step handed its caller -- the train loss, every value it logged (0-dim device
    tensors) and the flat parameter buffer after AdamW -- as float32 DIR/<name>.npy. An array above DUMP_MAX_ELEMENTS is
    written as the same sample in every run: its elements at the sorted first DUMP_MAX_ELEMENTS indices of
    torch.randperm(numel, generator seeded 0)."""
    import re

    import numpy as np
    import torch

    out = pathlib.Path(path)
    out.mkdir(parents=True, exist_ok=True)
    arrays = {"loss": loss, "params": flat}
    arrays |= {"logged_" + re.sub(r"\W", "_", k): v for k, v in logged.items()}
    for name, v in arrays.items():
        a = torch.as_tensor(v).detach().float().cpu()
        if a.numel() > DUMP_MAX_ELEMENTS:
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_MAX_ELEMENTS].sort().values
            a = a.reshape(-1)[idx]
        np.save(out / f"{name}.npy", a.numpy())


class HipEvents:
    """Timing hipEvent pairs, created once through the library (xfmr_event_create)."""

    def __init__(self, n):
        from xfmr_rec_amd import _native as N

        self.lib = N.load()
        self.pairs = []
        for _ in range(n):
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            N.check(self.lib.xfmr_event_create(ctypes.byref(a), 1), "xfmr_event_create")
            N.check(self.lib.xfmr_event_create(ctypes.byref(b), 1), "xfmr_event_create")
            self.pairs.append((a.value, b.value))

    def elapsed_ms(self, idx=None):
        out = []
        for i, (a, b) in enumerate(self.pairs):
            if idx is not None and i not in idx:
                continue
            ms = ctypes.c_float()
            if self.lib.xfmr_event_elapsed_ms(a, b, ctypes.byref(ms)) == 0:
                out.append(ms.value)
        return out


def usable_cpus() -> int:
    """Host cores this process may actually use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = pathlib.Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:  # noqa: BLE001
        pass
    return max(1, min(n, 64))


# ------------------------------------------------------------------------------------------------- CPU baseline
def _cpu_variant(args, *, B, L, H, V, layers, inter, faithful, autocast, seconds, label):
    import torch

    from oracle import encoder as enc
    from oracle import model as OM

    params = enc.init_params(H, layers, inter, L, seed=0)
    table = unit_table(V, H)
    batch, _ = synth_batch(B, L, V, 999, args.lengths)
    tr = OM.OracleTrainer(params, table, num_heads=H // 32, max_seq_length=L, train_loss=args.loss,
                          dropout_p=0.0 if args.no_dropout else 0.1, faithful=faithful)

    def step():
        if autocast:  # the reference's default precision: Lightning "bf16-mixed" = torch.autocast (trainer.py:449-455)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                tr.step(batch)
        else:
            tr.step(batch)

    # 3 warm-up steps, >= 10 timed steps, the MEDIAN reported. The time budget only extends the
    # sample beyond the 10 steps the protocol asks for (up to 50); it never cuts it short.
    for _ in range(3):
        step()
    times = []
    t_all = time.perf_counter()
    while len(times) < 10 or (len(times) < 50 and time.perf_counter() - t_all < seconds):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    times.sort()
    n = len(times)
    dt = times[n // 2] if n % 2 else 0.5 * (times[n // 2 - 1] + times[n // 2])
    return {
        "variant": label, "value": round(B / dt, 3), "unit": "sequences/s", "ms_per_step": round(dt * 1e3, 1),
        "ms_per_step_min_max": [round(times[0] * 1e3, 1), round(times[-1] * 1e3, 1)],
        "sample": f"median of {n} steps after 3 warm-up steps, B={B} x L={L} (H={H}, {layers} layers, V={V}; "
                  f"N={B * L} in-batch negatives)",
    }


def cpu_model() -> str:
    """The host CPU's model name (printed into the result beside the core count)."""
    try:
        for line in pathlib.Path("/proc/cpuinfo").read_text().splitlines():
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:  # noqa: BLE001
        pass
    import platform

    return platform.processor() or platform.machine() or "unknown"


def cpu_baseline(args):
    """The CPU oracle timed on this host (kind 'port': no reference file travels to the GPU box; the oracle is pinned to the
    reference by tests/golden). Headline = reference-faithful fp32 on the bench workload's shape: materialised
    (Np,1+N,H) candidates, 7 heads + statistics, backward, AdamW; the O(N^2 H) candidate tensor caps the CPU batch."""
    import torch

    threads = usable_cpus()
    torch.set_num_threads(threads)
    L, H, V = args.seq_len, args.hidden, args.items
    kw = dict(L=L, H=H, V=V, layers=args.layers, inter=args.inter, seconds=args.cpu_seconds)
    variants = [
        _cpu_variant(args, B=args.cpu_batch, faithful=not args.lean, autocast=False, label="reference-faithful fp32", **kw),
        _cpu_variant(args, B=args.cpu_batch, faithful=not args.lean, autocast=True,
                     label="reference-faithful bf16-autocast (the reference's default precision)", **kw),
        _cpu_variant(args, B=args.cpu_batch, faithful=False, autocast=False,
                     label="reference-lean fp32 (train head only, GEMM-form logits)", **kw),
        _cpu_variant(args, B=32, faithful=False, autocast=False,
                     label="reference-lean fp32 at the reference's default batch 32 (no O(N^2 H) tensor to cap it)", **kw),
        _cpu_variant(args, B=32, L=50, H=64, V=1682, layers=2, inter=256, faithful=True, autocast=False,
                     seconds=args.cpu_seconds, label="BASELINE config 1 (ML-100K-shaped, the reference's CPU-runnable case), faithful fp32"),
    ]
    head = variants[0]
    return {
        "value": head["value"], "unit": "sequences/s", "cores": threads, "cpu_model": cpu_model(), "kind": "port",
        "protocol": "BASELINE.md section 3: same process and host as the GPU number, torch.set_num_threads(cores), dropout on, "
                    "3 warm-up steps, >= 10 timed steps, median",
        "sample": head["sample"] + f", fp32, {'7 heads + stats' if not args.lean else 'train head only'}, "
                                   f"{head['ms_per_step']:.0f} ms/step",
        "variants": variants,
    }


# ------------------------------------------------------------------------------------------------- the benchmark
def encoder_flops_per_token(L, H, inter, layers):
    """Executed encoder flops per token of a DENSE row, forward + backward (3x forward)."""
    return 3 * layers * (8 * H * H + 4 * H * inter + 2 * (L + 1) * H)


SIMDS, CLOCK_GHZ = 1024, 2.4  # 256 CUs x 4 SIMD-32; MI355X_MICROARCH.md


def valu_roofline(v, launch_ms):
    """The dominant kernel against the VECTOR pipe (it is bound by VALU issue, not by the matrix core): wave-instructions per
    launch from the committed rocprofv3 SQ counters x cycles per wave64 instruction / (SIMDs x clock) / the launch duration
    measured in THIS run. Two prices: the microarchitecture guide's 2 cycles on a SIMD-32 (what the pipe could take from
    several waves), and the 4 x SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU cycles this kernel's instructions are measured to hold
    the pipe for (transcendentals count double)."""
    if not v or not launch_ms:
        return None
    n = float(v["wave_instructions_per_launch"])
    cyc = SIMDS * CLOCK_GHZ * 1e9 * launch_ms * 1e-3
    meas = 4.0 * float(v["active_quad_cycles_per_launch"]) / n if v.get("active_quad_cycles_per_launch") else None
    return {"wave_instructions_per_launch": n, "simds": SIMDS, "clock_ghz": CLOCK_GHZ,
            "frac_at_2_cycles_per_instruction": round(2.0 * n / cyc, 4),
            "cycles_per_instruction_measured": round(meas, 2) if meas else None,
            "frac_busy_measured": round(meas * n / cyc, 4) if meas else None,
            "source": v.get("source")}


PROFILE_ROUND = "r04"  # the round whose committed counter runs (profiles/<round>_*) describe THIS build's kernels


def static_profile(name):
    """profiles/<name> (counter figures that one bench run cannot collect itself: --pmc passes slow and serialise the
    launches) -- only when it was collected for this build's round: a file of another round is refused, `traffic` is then
    null and says why, instead of a stale number riding along silently."""
    p = ROOT / "profiles" / name
    try:
        d = json.loads(p.read_text()) if p.exists() else None
    except Exception:  # noqa: BLE001
        return None
    if d is not None and d.get("round") != PROFILE_ROUND:
        return None
    return d


def step_algorithmic_bytes(B, L, H, inter, heads, layers, n_params):
    """HBM bytes one training step must move if every tensor is read and written once (DESIGN.md sections 3 / 5; the table of
    scripts/kernel_roofline.py): bf16 for the tensors that are only ever MFMA operands, fp32 for the residual stream, its
    gradient and the LayerNorm inputs. Per layer: QKV / attention / out-proj + LN / fused FFN forward; their backward dX
    chain; the four weight-gradient GEMMs' operands. Once: gather + embedding LN and its backward, the loss's query rows
    and gradient, the split-K slabs' reduction is NOT algorithmic (a single-slab dW would not need it) and is left out."""
    T = B * L
    TH, TI, T3H = T * H, T * inter, 3 * T * H
    f32, b16 = 4, 2
    fwd = (TH * b16 + T3H * b16) + (T3H * b16 + TH * b16 + B * heads * L * f32) + (TH * b16 + 3 * TH * f32 + TH * b16) \
        + (TH * b16 + TH * f32 + 2 * TI * b16 + 2 * TH * f32 + TH * b16)
    bwd = (TH * b16 + 2 * TI * b16 + 3 * TH * f32 + TH * b16) + 2 * TH * b16 + (2 * T3H * b16 + 2 * TH * b16) \
        + (T3H * b16 + 3 * TH * f32 + TH * b16)
    dw = (TH + TI) * b16 * 2 + (TH + TH) * b16 + (T3H + TH) * b16
    once = (3 * TH * f32 + TH * b16) + (3 * TH * f32 + TH * b16 // 2) + 3 * TH * f32 + 28 * n_params
    return float(layers * (fwd + bwd + dw) + once)


def main():
    args = parse()
    if os.environ.get("XFMR_BENCH_DRY") == "1" and "WORLD_SIZE" in os.environ:
        sys.exit(dry_run(args))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # one process was asked for N GPUs: become the launcher (no HIP call has been made in this process)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if os.environ.get("XFMR_BENCH_DRY") == "1":
        sys.exit(dry_run(args))

    import torch

    import xfmr_rec_amd as X
    from xfmr_rec_amd import _native as N
    from xfmr_rec_amd import distributed as D

    rank, local, world = D.init_process_group_from_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a {world}-GPU run as "
                         f"{args.gpus} GPUs")
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (there is no CPU product path)"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    B, L, H, V = args.batch, args.seq_len, args.hidden, args.items
    catalogue = args.negatives == "catalogue"
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=args.heads or H // 32, intermediate_size=args.inter,
                             num_hidden_layers=args.layers, max_seq_length=L, train_loss=args.loss,
                             precision=args.precision, log_all_losses=not args.lean, negatives=args.negatives,
                             **(dict(target_position=None, mask_false_negatives=False) if catalogue else {}))
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V, H).to(dev))
    trainer = X.Trainer(mod, world_size=world)
    mod.train()
    if args.no_dropout:
        mod.eval()

    n_batches = 4
    KEYS = ("history_item_idx", "pos_item_idx", "neg_item_idx")
    host_batches, batches, host_lens = [], [], []
    for i in range(n_batches):
        b, lens = synth_batch(B, L, V, 1000 + rank * 97 + i, args.lengths)
        # one pinned (3, B, L) block per batch: the collate output as ONE host buffer, so the hand-over is one copy
        host_batches.append(torch.stack([b[k] for k in KEYS]).pin_memory())
        host_lens.append(torch.tensor(lens, dtype=torch.int64))  # the collate knows the rows' lengths: it padded them
        batches.append({k: v.to(dev) for k, v in b.items()})
    tokens_per_seq = sum(lens) / len(lens)

    overlap = args.overlap == "on" or (args.overlap == "auto" and B * L >= 51200)  # (= the module's own "auto" rule)

    # Host -> HBM hand-over inside the step ("H2D of the 3 index tensors -> ..."): persistent device slots,
    # pre-created events, one hipMemcpyAsync per batch on a copy stream, the copy of batch i + 1 underneath step i -- the
    # product's PinnedBatchRing (xfmr_rec_amd/data.py), what Trainer.fit feeds its steps from.
    from xfmr_rec_amd.data import PinnedBatchRing

    ring = PinnedBatchRing(dev, B, L)

    # hipGraph replay of the step (GraphedStep): "auto" MEASURES it against the eager step for small steps and keeps the
    # faster. (Round 3, MI355X: replay wins where the eager step is bound by the host's launch rate -- 0.31 vs 0.48 ms at
    # H 64 / L 50 / batch 64 -- and changes nothing where the ~80 dependent launches are GPU-latency-bound: config 2 at
    # batch 32, 0.85 vs 0.83 ms.)
    gstep, graph_tune = None, None
    if world == 1 and (args.graph == "on" or (args.graph == "auto" and B * L <= 32768)):
        mod.defer_logging = bool(overlap)
        gstep = X.GraphedStep(trainer, batches[0])
        if args.graph == "auto":
            def _time(fn, n=40):
                for i in range(10):
                    fn(i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    fn(i)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n * 1e3

            g_ms = _time(lambda i: gstep(batches[i % n_batches]))
            e_ms = _time(lambda i: trainer.fit_step(batches[i % n_batches]))
            graph_tune = {"graph_ms": round(g_ms, 4), "eager_ms": round(e_ms, 4)}
            if e_ms <= g_ms:
                gstep = None

    lib = N.load()
    ar_events = HipEvents(max(args.steps, 1)) if world > 1 else None  # around the exchange, on the compute stream

    # The four big kernels of a layer, bracketed by HIP events on their launch stream (xfmr_encoder_cfg.profile_*) -- where
    # each IS one kernel: the fused forms of d_model 128 in bf16 storage from 16 384 tokens (csrc/encoder.hip: ln_fused).
    ENC_PARTS = ((N.PROF_FFN_FWD, "ffn_fwd_fused_kernel"), (N.PROF_FFN_BWD, "ffn_bwd_dx_fused_kernel"),
                 (N.PROF_ATTN_FWD, "attn_fwd_seq_bf16_kernel"), (N.PROF_ATTN_BWD, "attn_bwd_fused_bf16_kernel"))
    ENC_LAYER = min(1, args.layers - 1)
    enc_parts_ok = (args.precision == "bf16" and H == 128 and B * L >= 16384 and L <= 256 and args.inter % 128 == 0
                    and args.inter <= 1024 and not os.environ.get("XFMR_LN_UNFUSED") and not os.environ.get("XFMR_FFN_UNFUSED")
                    and not os.environ.get("XFMR_FFN_BWD_UNFUSED") and not os.environ.get("XFMR_ATTN_BWD_SPLIT")
                    and not os.environ.get("XFMR_ATTN_FWD_SPLIT"))

    enc_flags0 = getattr(mod.model, "enc_flags", 0)

    def step(i, from_host=False, in_line=False, profile=None, enc_profile=None):
        """zero_grad -> training_step -> backward -> [all-reduce] -> optimizer.step -> on_train_batch_end: the module's
        Lightning seam in Lightning's order (= Trainer.fit_step)."""
        if from_host == "inline":  # Lightning's plain batch transfer: three copies on the compute stream itself
            batch = {k: host_batches[i % n_batches][j].to(dev, non_blocking=True) for j, k in enumerate(KEYS)}
        elif from_host:
            if ring.pending == 0:
                ring.stage(host_batches[i % n_batches], host_lens[i % n_batches])
            batch = ring.take()
            ring.stage(host_batches[(i + 1) % n_batches], host_lens[(i + 1) % n_batches])  # in flight while this step computes
        else:
            batch = batches[i % n_batches]
        if gstep is not None and not in_line and profile is None:
            return gstep(batch), mod.last_out  # one hipGraph launch: the same step, captured (GraphedStep)
        mod.model.enc_profile = enc_profile  # (kernel, layer, ev0, ev1): xfmr_encoder_cfg.profile_*
        # in line = ONE stream: the weight-gradient GEMMs too (otherwise they run beside the bracketed kernel and its
        # duration contains what they take from it)
        mod.model.enc_flags = (enc_flags0 | N.ENC_DW_INLINE) if in_line else enc_flags0
        opt = trainer.optimizer
        opt.zero_grad(set_to_none=True)
        mod.defer_logging = bool(overlap and not in_line)
        mod.profile_events = profile
        loss = mod.training_step(batch, i)
        mod.backward(loss)  # Lightning's hook: loss.backward() with the persistent unit gradient (trainer.py)
        if world > 1:
            pair = ar_events.pairs[i % len(ar_events.pairs)] if ar_events is not None else None
            if pair:
                N.check(lib.xfmr_event_record(pair[0], N.stream()), "xfmr_event_record")
            trainer.allreduce_(mod.model.flat.grad)  # two halves, the upper layers' underneath the backward (HalvedAllReduce)
            if pair:
                N.check(lib.xfmr_event_record(pair[1], N.stream()), "xfmr_event_record")
        opt.step()
        mod.on_train_batch_end(loss, batch, i)
        return loss, mod.last_out

    def timed(n_steps, events=None, from_host=False):
        """Exactly n_steps steps between barriers + device synchronisations; MAX over ranks."""
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_steps):
            prof = None
            if events is not None:  # even steps time the gradient pass, odd steps the logging pass (xfmr_loss_cfg.profile_*)
                prof = (None, events.pairs[i]) if (i & 1) else (events.pairs[i], None)
            encp = None
            if events is not None and enc_events is not None:  # one of the four encoder parts per step, layer ENC_LAYER
                encp = (ENC_PARTS[i % 4][0], ENC_LAYER) + enc_events.pairs[i]
            loss, out = step(i, from_host, profile=prof, enc_profile=encp)
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        elapsed = time.perf_counter() - t0
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        if world > 1:
            per_rank = [torch.zeros_like(t) for _ in range(world)]
            torch.distributed.all_gather(per_rank, t)
            timed.per_rank_s = [float(x.item()) for x in per_rank]
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return float(t.item()), loss, out

    if args.full:  # cold rate: what a run WITHOUT the spin-up would report (--warmup steps, then --steps steps timed)
        for i in range(args.warmup):
            step(i)
        cold_s, _, _ = timed(args.steps)
    for i in range(args.spinup_steps):  # device spin-up (clocks, caches, allocator pools): untimed, not the warmup
        step(i)
    torch.cuda.synchronize()
    for i in range(args.warmup):
        step(i)
    # per-kernel durations of the timed steps (--full; a captured step has no per-launch events: see `alone_ms`)
    ev = HipEvents(args.steps) if (args.full and gstep is None) else None
    enc_events = HipEvents(args.steps) if (args.full and gstep is None and enc_parts_ok) else None
    # THE timed region: batch in page-locked host memory -> H2D of the three index tensors -> gather ->
    # encoder -> loss -> backward -> [all-reduce] -> AdamW
    for i in range(2):
        step(i, True)
    elapsed, loss, out = timed(args.steps, ev, from_host=True)
    per_rank_ms = [round(s / args.steps * 1e3, 4) for s in getattr(timed, "per_rank_s", [elapsed])]
    ar_ms = ar_events.elapsed_ms() if ar_events is not None else []
    if args.dump_outputs and rank == 0:  # before any further step changes the parameters
        dump_outputs(args.dump_outputs, loss, gstep.logged if gstep is not None else mod.logged, mod.model.flat)
    step_ms = elapsed / args.steps * 1e3
    seqs = B * world * args.steps
    extra = {}  # the --full figures of the line
    if args.full:
        resident_s, _, _ = timed(args.steps)  # the same steps on batches that already lie in HBM
        inline_s, _, _ = timed(args.steps, None, from_host="inline")
        # SURVEY section 8(d) names two length regimes: dense rows (the roofline stress: `value`) and MovieLens-like ragged rows,
        # len ~ clip(round(exp(N(4.35, 1))), 16, L), right-padded with 0 as the reference's collate does (data.py:799-805). The
        # same timed region on ragged batches of the same (B, L) shape, beside the dense figure.
        ragged = None
        if args.lengths == "dense" and not args.no_ragged:
            while ring.pending:
                ring.take()
            ring.release()
            dense_sets = (host_batches, batches, host_lens)
            r_host, r_dev, r_lens, r_hl = [], [], [], []
            for i in range(n_batches):
                b, lens = synth_batch(B, L, V, 5000 + rank * 97 + i, "ml")
                r_host.append(torch.stack([b[k] for k in KEYS]).pin_memory())
                r_dev.append({k: v.to(dev) for k, v in b.items()})
                r_hl.append(torch.tensor(lens, dtype=torch.int64))
                r_lens += lens
            host_batches, batches, host_lens = r_host, r_dev, r_hl
            # (the packed layout's tensors have other sizes than the dense steps before them, and four different ones: the caching
            #  allocator settles over the first dozens of steps -- until then a step may pay a hipMalloc, which synchronises)
            for i in range(max(args.warmup, 80)):
                step(i, True)
            ragged_s, _, _ = timed(args.steps, None, from_host=True)
            # ... and the same batches in the reference's padded layout (XFMR_PACKED=0: the lengths are ignored)
            os.environ["XFMR_PACKED"] = "0"
            for i in range(max(args.warmup, 10)):
                step(i, True)
            ragged_padded_s, _, _ = timed(args.steps, None, from_host=True)
            os.environ.pop("XFMR_PACKED", None)
            while ring.pending:
                ring.take()
            ring.release()
            host_batches, batches, host_lens = dense_sets
            ragged = {"value": round(B * world * args.steps / ragged_s, 2), "unit": "sequences/s",
                      "ms_per_step": round(ragged_s / args.steps * 1e3, 4), "lengths": "ml",
                      "mean_tokens_per_sequence": round(sum(r_lens) / len(r_lens), 1),
                      "tokens_per_s": round(sum(r_lens) / len(r_lens) * B * world * args.steps / ragged_s, 1),
                      "layout": "packed rows (xfmr_encoder_cfg.seq_offsets): the encoder and the loss run each sequence's own rows; "
                                "the batch still arrives as the reference's right-padded (B, L) tensors, with the lengths its "
                                "collate knows",
                      "padded_layout": {"value": round(B * world * args.steps / ragged_padded_s, 2),
                                        "ms_per_step": round(ragged_padded_s / args.steps * 1e3, 4),
                                        "note": "the same batches with the padding rows computed, as the reference does (XFMR_PACKED=0)"},
                      "note": "the timed region of `value` (H2D included) on MovieLens-like ragged rows of the same (B, L) shape: "
                              "len = clip(round(exp(N(4.35, 1))), 16, L), right-padded with 0 (SURVEY section 8d, data.py:799-805)"}
        # The dominant kernel once more with nothing beside it (outside the timed region): in the timed region the logging pass
        # sits on a lowest-priority stream underneath the encoder backward, so its duration there includes the time it is held
        # back -- what a one-stream rocprofv3 trace (profiles/*_kernel_stats.md) sees is this figure.
        alone_ms, alone_grad_ms = [], []
        # in line the layer's four weight-gradient GEMMs are ONE launch (dw_ring_kernel) and can be bracketed too, and so can
        # the backward's final reduction launch
        ALONE_PARTS = ENC_PARTS + ((N.PROF_DW, "dw_ring_kernel"), (N.PROF_REDUCE, "multi_rowsum_kernel"))
        alone_enc = {k: [] for k, _ in ALONE_PARTS}
        if (overlap or gstep is not None) and not args.lean:
            n_alone = 18
            ev2 = HipEvents(n_alone)
            ev3 = HipEvents(n_alone) if enc_parts_ok else None
            for i in range(n_alone):  # even: the gradient pass, odd: the logging pass -- both on the main stream, one after the other
                encp = (ALONE_PARTS[i % 6][0], ENC_LAYER) + ev3.pairs[i] if ev3 is not None else None
                step(i, in_line=True, profile=(None, ev2.pairs[i]) if (i & 1) else (ev2.pairs[i], None), enc_profile=encp)
            torch.cuda.synchronize()
            alone_ms = ev2.elapsed_ms({i for i in range(n_alone) if i & 1})
            alone_grad_ms = ev2.elapsed_ms({i for i in range(n_alone) if not (i & 1)})
            if ev3 is not None:
                for j, (k, _) in enumerate(ALONE_PARTS):
                    alone_enc[k] = ev3.elapsed_ms({i for i in range(n_alone) if i % 6 == j})
        mod.model.enc_profile = None

        stats = out["stats/device"].tolist()
        n_valid, n_query = stats[N.STAT["n_valid"]], stats[N.STAT["n_query"]]
        n_cols = stats[N.STAT["neg_distinct"]]
        if ev is not None:
            grad_ms = ev.elapsed_ms({i for i in range(args.steps) if not (i & 1)})
            log_ms = ev.elapsed_ms({i for i in range(args.steps) if (i & 1)}) if not args.lean else []
        else:  # graph replay: the kernels are timed in the eager in-line steps after the timed region only
            grad_ms, log_ms = list(alone_grad_ms), list(alone_ms)
        grad_avg = sum(grad_ms) / max(len(grad_ms), 1)
        log_avg = sum(log_ms) / max(len(log_ms), 1)
        peak = PEAK_BF16_MFMA_TFLOPS if args.precision == "bf16" else PEAK_F32_MFMA_TFLOPS
        # Executed = algorithmic flops of THESE kernels: their columns are the distinct negative items (<= min(N, V): in-batch
        # negatives repeat items and every per-column term is a function of the item; the north star's "batch x seq x
        # item-catalogue" GEMM). The reference's materialised form scores all N sampled columns: its count is reported
        # beside it, it is not a hardware rate.
        grad_flops = 4.0 * n_query * n_cols * H
        log_flops = 2.0 * n_query * n_cols * H
        ref_form_flops = 4.0 * n_query * n_valid * H

        def kernel_entry(name, flops, avg_ms, n):
            tf = flops / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
            return {"kernel": name, "bound": "mfma", "achieved": round(tf, 2), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(tf / peak, 5), "avg_launch_ms": round(avg_ms, 4), "algorithmic_flops_per_launch": flops,
                    "launches_timed": n}

        k_grad = kernel_entry("loss_main_dma_kernel, gradient pass (logit GEMM + fused epilogue + dQ GEMM)", grad_flops,
                              grad_avg, len(grad_ms))
        k_log = kernel_entry("loss_main_dma_kernel, logging pass (six logging heads + LogitsStatistics, values only; "
                             "VALU-issue-bound: profiles/)", log_flops, log_avg, len(log_ms))
        note = ("avg_launch_ms / achieved / frac: the kernel with nothing beside it -- 6 further steps after the timed region "
                "with both loss passes on the main stream, one after the other: the figure a one-stream rocprofv3 trace "
                "(profiles/*_kernel_stats.md) shows; *_overlapped: in the timed region, where the logging pass runs on a "
                "lowest-priority stream beside the gradient pass and underneath the encoder backward (each pass's duration "
                "then includes what the others take from it)")
        for k, ms, fl in ((k_log, alone_ms, log_flops), (k_grad, alone_grad_ms, grad_flops)):
            if ms:
                a = sum(ms) / len(ms)
                tf = fl / (a * 1e-3) / 1e12
                k |= {"avg_launch_ms_overlapped": k["avg_launch_ms"], "achieved_overlapped": k["achieved"],
                      "frac_overlapped": k["frac"]}
                k |= {"avg_launch_ms": round(a, 4), "achieved": round(tf, 2), "frac": round(tf / peak, 5), "note": note}
        k_log["launches_per_step"] = k_grad["launches_per_step"] = 1
        if args.loss in ("AlignmentContrastiveLoss", "ContrastiveLoss", "PairwiseHingeLoss"):
            # hinge-type gradient weights are exactly 0 inside the margin: the gradient pass skips the dQ MFMAs of every 32 x 32
            # block without an active pair (csrc/loss_dma.inc). The algorithmic flops above still count the dQ product, so on
            # batches with few active pairs (random-init weights, a random table: none) `achieved` is up to 2 x the executed rate.
            k_grad["dq_product"] = ("skipped per 32x32 block when every gradient weight of the block is 0 (hinge-type head); "
                                    "algorithmic_flops_per_launch counts it in full")
        # The encoder's four big kernels (one launch per layer each), against HBM: ALGORITHMIC bytes per launch = what the kernel
        # must read and write once (scripts/kernel_roofline.py holds the same table) / the launch duration.
        Tt = B * L
        TH, TI = Tt * H, Tt * args.inter
        A_heads = args.heads or H // 32
        enc_model = {
            N.PROF_FFN_FWD: ("ffn_fwd_fused_kernel (FFN1 + GELU + FFN2 + dropout + residual + LayerNorm; writes u, g)",
                             TH * 2 + TH * 4 + 2 * TI * 2 + 2 * TH * 4 + TH * 2, 4.0 * Tt * args.inter * H),
            N.PROF_FFN_BWD: ("ffn_bwd_dx_fused_kernel (FFN2 dX x gelu'(u) -> dI -> FFN1 dX + LayerNorm backward)",
                             TH * 2 + 2 * TI * 2 + TH * 4 * 3 + TH * 2, 4.0 * Tt * args.inter * H),
            N.PROF_ATTN_FWD: ("attn_fwd_seq_bf16_kernel (one workgroup per (batch, head))",
                              3 * TH * 2 + TH * 2 + B * A_heads * L * 4, 4.0 * B * A_heads * L * (L + 1) / 2 * 32),
            N.PROF_ATTN_BWD: ("attn_bwd_fused_bf16_kernel (one workgroup per (batch, head): dQ, dK, dV)",
                              2 * 3 * TH * 2 + 2 * TH * 2, 10.0 * B * A_heads * L * (L + 1) / 2 * 32),
            # operands only: dy + g, dI + x1, d_lin + ctx, dQKV + x (all bf16); the split-K slabs it also writes are overhead
            N.PROF_DW: ("dw_ring_kernel (the layer's four weight-gradient GEMMs, token slabs through an LDS-DMA ring, in one launch: the in-line form)",
                        (TH + TI) * 2 * 2 + 2 * TH * 2 + (3 * TH + TH) * 2, 2.0 * Tt * (2 * H * args.inter + H * H + 3 * H * H)),
        }
        enc_entries = []
        if enc_parts_ok:
            over = {k: (enc_events.elapsed_ms({i for i in range(args.steps) if i % 4 == j}) if enc_events is not None else [])
                    for j, (k, _) in enumerate(ENC_PARTS)}
            for k, _short in ALONE_PARTS:
                ms_alone, ms_over = alone_enc.get(k) or [], over.get(k) or []
                ms = ms_alone or ms_over
                if not ms or k not in enc_model:
                    continue
                name, nbytes, flops = enc_model[k]
                avg = sum(ms) / len(ms)
                e = {"kernel": name, "bound": "hbm", "achieved": round(nbytes / (avg * 1e-3) / 1e12, 3), "peak": PEAK_HBM_TBPS,
                     "unit": "TB/s", "frac": round(nbytes / (avg * 1e-3) / 1e12 / PEAK_HBM_TBPS, 5),
                     "avg_launch_ms": round(avg, 4), "algorithmic_bytes_per_launch": float(nbytes),
                     "launches_per_step": args.layers, "launches_timed": len(ms), "layer_timed": ENC_LAYER,
                     "mfma_tflops": round(flops / (avg * 1e-3) / 1e12, 1)}
                if ms_alone and ms_over:
                    e["avg_launch_ms_overlapped"] = round(sum(ms_over) / len(ms_over), 4)
                enc_entries.append(e)
        # dominant = the kernel with the most GPU time per step (launch duration with nothing beside it x launches per step):
        # the top row of a one-stream rocprofv3 trace (profiles/*_kernel_stats.md). (The 4 x layers weight-gradient GEMMs run on
        # a side stream in many launches and are not bracketed; their sum per step is in profiles/.)
        cands = ([k_log] if log_ms else []) + [k_grad] + enc_entries
        dominant = max(cands, key=lambda e: e["avg_launch_ms"] * e["launches_per_step"])
        for e in cands:
            e["ms_per_step"] = round(e["avg_launch_ms"] * e["launches_per_step"], 4)
        # whole step: executed flops of the encoder (fwd + bwd, valid tokens) and of the two loss passes / step time
        enc_flops = n_valid * encoder_flops_per_token(tokens_per_seq, H, args.inter, args.layers)
        step_flops = enc_flops + grad_flops + (log_flops if log_ms else 0.0)
        step_tf = step_flops / (step_ms * 1e-3) / 1e12
        static = static_profile(f"{PROFILE_ROUND}_bench_static.json") or {}
        step_bytes = step_algorithmic_bytes(B, tokens_per_seq, H, args.inter, args.heads or H // 32, args.layers,
                                            int(mod.model.flat.numel()))
        if rank == 0:
            roofline = dict(dominant)
            ktraffic = static.get("kernel_hbm_bytes_per_launch") or {}
            dom_key = next((short for k, short in ALONE_PARTS if dominant["kernel"].startswith(short)), None)
            if dom_key is None:
                dom_key = "loss_logging_pass" if dominant is k_log else "loss_gradient_pass"
            dom_traffic = ktraffic.get(dom_key)
            if dom_traffic is None and dominant is k_log:
                dom_traffic = static.get("dominant_kernel_hbm_bytes_per_launch")
            roofline |= {
                "traffic": dom_traffic,
                "traffic_source": static.get("source") if dom_traffic else
                                  f"null: profiles/{PROFILE_ROUND}_bench_static.json (scripts/collect_profiles.sh {PROFILE_ROUND}) "
                                  "is missing or holds no counter run of this kernel; files of other rounds are refused",
                # step level: what the whole step moves if every tensor crosses HBM once / ms_per_step / the HBM peak
                "step_hbm": {"algorithmic_bytes": step_bytes, "achieved": round(step_bytes / (step_ms * 1e-3) / 1e12, 3),
                             "peak": PEAK_HBM_TBPS, "unit": "TB/s",
                             "frac": round(step_bytes / (step_ms * 1e-3) / 1e12 / PEAK_HBM_TBPS, 4),
                             "note": "step_algorithmic_bytes() of bench.py (per-kernel compulsory bytes, mean row length) / "
                                     "ms_per_step; the two loss passes and the attention kernels are not bound by bytes"},
                "columns": int(n_cols), "sampled_negative_columns": int(n_valid),
                "reference_form_flops_per_launch": ref_form_flops,
                "kernels": [k_grad] + ([k_log] if log_ms else []) + enc_entries,
                "step": {"executed_flops": step_flops, "achieved": round(step_tf, 1), "unit": "TFLOP/s", "peak": peak,
                         "frac": round(step_tf / peak, 4),
                         "note": "encoder fwd+bwd on valid tokens + both loss passes, / ms_per_step"},
                "reduction_launch_ms": (round(sum(alone_enc[N.PROF_REDUCE]) / len(alone_enc[N.PROF_REDUCE]), 4)
                                        if alone_enc.get(N.PROF_REDUCE) else None),
                "valu": valu_roofline(static.get("dominant_kernel_valu"), k_log["avg_launch_ms"]) if log_ms else None,
                "valu_kernel": k_log["kernel"] if log_ms else None,
                "gemm_family_tbps": static.get("gemm_family_tbps"),
                "gemm_family_tbps_source": static.get("source") if static.get("gemm_family_tbps") else None,
                "hbm_peak_tbps": PEAK_HBM_TBPS,
            }
            extra = {
                "resident": {"value": round(seqs / resident_s, 2), "ms_per_step": round(resident_s / args.steps * 1e3, 4),
                             "note": "the same timed region on batches that already lie in HBM (no copy in the step)"},
                "h2d_on_compute_stream": {"value": round(seqs / inline_s, 2), "ms_per_step": round(inline_s / args.steps * 1e3, 4),
                                          "note": "Lightning's plain batch transfer: three .to(device, non_blocking=True) copies on "
                                                  "the compute stream itself, nothing prefetched"},
                **({"ragged": ragged} if ragged else {}),
                "cold_start": {"value": round(seqs / cold_s, 2), "ms_per_step": round(cold_s / args.steps * 1e3, 4),
                               "note": f"the first {args.steps} steps after {args.warmup} warm-up steps only, before the spin-up"},
                "roofline": roofline,
            }

    if rank == 0:
        result = {
            "metric": METRIC,
            "value": round(seqs / elapsed, 2),
            "unit": "sequences/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "spinup_steps": args.spinup_steps,
            "ms_per_step": round(step_ms, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.precision,
            "data": "synthetic" if not D.rehearsal_on_one_gpu() else "synthetic (REHEARSAL: all ranks on one GPU, gloo)",
            "config": {
                "workload": (f"{'MovieLens-1M-shaped' if V == 3883 else 'synthetic'}: {V} items, seq_len={L}, "
                             f"d_model={H}, {args.layers}-layer causal BERT (heads={args.heads or H // 32}, "
                             f"ffn={args.inter}), {args.loss} over "
                             f"{'the full item catalogue' if catalogue else 'in-batch shared negatives'}, AdamW"),
                "per_gpu_batch": B, "global_batch": B * world, "seq_len": L, "lengths": args.lengths,
                "mean_tokens_per_sequence": round(tokens_per_seq, 1),
                "loss_heads_evaluated": "train head only" if args.lean else "all 7 + LogitsStatistics (reference training_step)",
                "dropout": 0.0 if args.no_dropout else 0.1, "parallelism": f"dp{world}",
                "launch": "one hipGraph replay per step (GraphedStep)" if gstep is not None else "eager launches",
                **({"graph_autotune_ms": graph_tune} if graph_tune else {}),
                "final_loss": round(float(loss.detach()), 4),
            },
            "h2d": {"included_in_value": True, "bytes_per_step": 3 * B * L * 8,
                    "how": "page-locked (3, B, L) int64 host block -> persistent device slot, ONE hipMemcpyAsync per batch on a "
                           "copy stream one batch ahead of the compute stream, pre-created events (PinnedBatchRing)"},
            **extra,
        }
        if world > 1:  # what a scaling record needs to explain itself
            be = torch.distributed.get_backend()
            result["exchange"] = {
                "backend": "rccl (torch.distributed 'nccl')" if be == "nccl" else be, "rccl_world": world,
                "message_bytes": int(mod.model.flat.numel()) * 4,
                "form": "two halves: layers >= L/2 under the lower layers' backward, the rest behind it" if trainer.exchange
                        else "one all-reduce after the backward",
                "allreduce_ms": round(sum(ar_ms) / len(ar_ms), 4) if ar_ms else None,
                "allreduce_ms_note": "HIP events on the compute stream around the exchange call of rank 0: what the step waits "
                                     "for (the overlapped half shows only as far as it is NOT hidden)",
                "ms_per_step_per_rank": per_rank_ms,
            }
        if args.full and world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(args)
        print(json.dumps(result), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
