#!/usr/bin/env python3
"""Padded against packed training steps on ragged batches, at a width where attention runs its one-workgroup forms (384)
and at one where it runs the key-streaming forms (2048): compute_losses + backward of BASELINE config 2's layer shape
(H 128, 4 heads, I 512, 4 layers) at batch 128, on bench.py's MovieLens-like lengths (synth_batch(..., "ml"): len =
clip(round(exp(N(4.35, 1))), 16, width)), every batch right-padded to its OWN longest row as the collate does.

One MI355X, one process, HIP events around --steps steps after --warmup. The batch carries its rows' lengths in both
layouts; XFMR_PACKED=0 makes the step ignore them (the padded layout). The two layouts are alternated over --rounds rounds;
per width the script prints every round's ms per step, the medians and the row counts, then one JSON line.

The packed route is taken through RecommenderModel.supports_packed_rows as the trainer takes it; the script counts the
ops.pack_rows calls of every timed window, so a width whose length range the gate keeps padded is reported as such."""
import argparse
import json
import os
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    sys.path.insert(0, str(p))
import torch  # noqa: E402

import xfmr_rec_amd as X  # noqa: E402
from bench import synth_batch, unit_table  # noqa: E402
from xfmr_rec_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[384, 2048])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--items", type=int, default=3883)
    ap.add_argument("--batches", type=int, default=4, help="distinct seeded batches cycled through")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = "cuda"
    H, A, I, layers, B, V = 128, 4, 512, 4, args.batch, args.items
    calls = []
    real = ops.pack_rows
    ops.pack_rows = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    result = {"shape": dict(hidden=H, heads=A, inter=I, layers=layers, batch=B), "steps": args.steps, "widths": {}}
    for width in args.widths:
        conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=I, num_hidden_layers=layers,
                                 max_seq_length=width, precision="bf16")
        mod = X.RecommenderLightningModule(conf)
        mod.configure_model()
        mod.model.set_table(unit_table(V, H).to(dev))
        mod.train()
        batches, padded_rows, real_rows, longest = [], 0, 0, []
        for i in range(args.batches):
            b, lens = synth_batch(B, width, V, 7000 + i, "ml")
            Lb = max(lens)  # the collate pads to the batch's longest row (data.py:799-805)
            d = {k: v[:, :Lb].contiguous().to(dev) for k, v in b.items()}
            d["lengths"] = torch.tensor(lens, dtype=torch.int64)
            batches.append(d)
            padded_rows += B * Lb
            real_rows += sum(lens)
            longest.append(Lb)

        def step(i):
            mod.model.flat.grad = None
            out = mod.compute_losses(batches[i % len(batches)])
            out["loss/InfoNCELoss"].backward()

        def window(layout):
            if layout == "padded":
                os.environ["XFMR_PACKED"] = "0"
            else:
                os.environ.pop("XFMR_PACKED", None)
            for i in range(args.warmup):
                step(i)
            torch.cuda.synchronize()
            calls.clear()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.steps):
                step(i)
            b.record()
            torch.cuda.synchronize()
            os.environ.pop("XFMR_PACKED", None)
            return a.elapsed_time(b) / args.steps, len(calls)

        for layout in ("packed", "padded"):  # the allocator settles on both layouts' sizes before anything is timed
            window(layout)
        ms = {"padded": [], "packed": []}
        packs = 0
        for r in range(args.rounds):
            for layout in ("padded", "packed"):
                t, n = window(layout)
                ms[layout].append(round(t, 4))
                if layout == "packed":
                    packs += n
                else:
                    assert n == 0
                print(f"width {width} round {r} {layout:6s} {t:9.3f} ms/step", flush=True)
        took_packed = packs == args.rounds * args.steps
        assert took_packed or packs == 0
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = {"padded_rows_per_batch": padded_rows / args.batches, "real_rows_per_batch": real_rows / args.batches,
               "longest_rows": longest, "ms_per_step": ms, "median_ms": med,
               "packed_over_padded": round(med["packed"] / med["padded"], 4),
               "packed_route_taken": took_packed}
        result["widths"][str(width)] = rec
        print(f"width {width}: rows padded {rec['padded_rows_per_batch']:.0f} real {rec['real_rows_per_batch']:.0f}; median "
              f"padded {med['padded']:.3f} packed {med['packed']:.3f} ms/step (packed / padded {rec['packed_over_padded']:.3f})"
              f"{'' if took_packed else ' -- the gate kept this width PADDED: both columns are the padded layout'}", flush=True)
        del mod, batches
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
