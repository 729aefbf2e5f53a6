#!/usr/bin/env python3
"""Timing of the generic attention kernels at lengths only their key-streaming forms reach (L = 512), plus the panel and
the forced streaming form side by side at L = 256 (fp32, head size 32), through ops.attn_fwd / ops.attn_bwd with HIP
events. Per shape: us per call, algorithmic bytes as a fraction of 8 TB/s, algorithmic MFMA FLOPs as a fraction of the
policy's matrix peak (bf16 2.5 PF dense, fp32 157.3 TF). Causal, every key valid, fp32 operands in HBM (ops path).

The bf16 head-size-32 production family: 32 x 12 x 1024 in the two-kernel panel form and in the key-streaming form
(stream_keys=True) -- the one shape class where both run -- alternated over --rounds passes in one process, with the
streaming / panel ratio per round and its spread; then the lengths only the streaming form reaches (2048, 4096).
--only SUBSTRING restricts the run to the shapes whose label contains it.

  algorithmic bytes: fwd reads qkv + mask, writes ctx + lse; bwd reads qkv, ctx, lse, d_ctx, mask, writes d_qkv
  algorithmic FLOPs: fwd 2 matmuls (S = Q K^T, O = P V), bwd 5 (S, dP, dV, dK, dQ), each 2 B A L^2 dh / 2 (causal)
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    sys.path.insert(0, str(p))
import torch  # noqa: E402

from xfmr_rec_amd import ops  # noqa: E402

HBM = 8.0e12
PEAK = {"bf16": 2.5e15, "fp32": 157.3e12}
SHAPES = [  # (label, precision, B, A, dh, L, stream_keys)
    ("bf16 h64 L512", "bf16", 32, 12, 64, 512, False),
    ("fp32 h32 L512", "fp32", 32, 8, 32, 512, False),
    ("fp32 h32 L256 panel", "fp32", 32, 8, 32, 256, False),
    ("fp32 h32 L256 stream", "fp32", 32, 8, 32, 256, True),
    ("bf16 h32 L2048 stream", "bf16", 32, 12, 32, 2048, False),  # (the panel does not fit: the default is streaming)
    ("bf16 h32 L4096 stream", "bf16", 8, 12, 32, 4096, False),
]
PAIRS = [  # (label, precision, B, A, dh, L): panel and stream_keys=True alternated over --rounds
    ("bf16 h32 L1024", "bf16", 32, 12, 32, 1024),
]


def timeit(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{'shape':22s} {'pass':4s} {'us':>9s} {'bytes/8TB/s':>12s} {'flops/peak':>11s}")

    def measure(label, prec, B, A, dh, L, stream):
        H = A * dh
        qkv = torch.randn(B, L, 3 * H, device=dev, generator=g)
        mask = torch.ones(B, L, dtype=torch.uint8, device=dev)
        d_ctx = torch.randn(B, L, H, device=dev, generator=g)
        kw = dict(precision=prec, stream_keys=stream)
        ctx, lse = ops.attn_fwd(qkv, mask, A, **kw)
        t_f = timeit(lambda: ops.attn_fwd(qkv, mask, A, **kw), args.reps, args.warmup)
        t_b = timeit(lambda: ops.attn_bwd(qkv, mask, ctx, lse, d_ctx, A, **kw), args.reps, args.warmup)
        tok = B * L
        mm = 2.0 * B * A * L * L * dh / 2  # one causal L x L x dh matmul
        by_f = tok * (3 * H * 4 + 1 + H * 4) + B * A * L * 4
        by_b = tok * (3 * H * 4 + H * 4 + H * 4 + 1 + 3 * H * 4) + B * A * L * 4
        for name, t, by, fl in (("fwd", t_f, by_f, 2 * mm), ("bwd", t_b, by_b, 5 * mm)):
            s = t * 1e-6
            print(f"{label:22s} {name:4s} {t:9.1f} {by / s / HBM:12.3f} {fl / s / PEAK[prec]:11.3f}", flush=True)
        return t_f, t_b

    for label, prec, B, A, dh, L, stream in SHAPES:
        if args.only in label:
            measure(label, prec, B, A, dh, L, stream)
    for label, prec, B, A, dh, L in PAIRS:
        if args.only not in label:
            continue
        ratios = {"fwd": [], "bwd": []}
        for r in range(args.rounds):
            panel = measure(f"{label} panel #{r}", prec, B, A, dh, L, False)
            stream = measure(f"{label} stream #{r}", prec, B, A, dh, L, True)
            for name, tp, ts in zip(("fwd", "bwd"), panel, stream):
                ratios[name].append(ts / tp)
        for name, rs in ratios.items():
            print(f"{label} {name}: streaming / panel = {sum(rs) / len(rs):.3f} (rounds: "
                  f"{', '.join(f'{x:.3f}' for x in rs)}; spread {min(rs):.3f} .. {max(rs):.3f})")


if __name__ == "__main__":
    main()
