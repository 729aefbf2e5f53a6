#!/usr/bin/env python3
"""Validation cost: `module.evaluate(rows)` against the resident `DeviceEvalSet.evaluate()`, and what a validation
pass costs inside `Trainer.fit` (bench.py is not involved).

1. The synthetic set of scripts/bench_eval.py (6 040 users, 3 900 items, the reference-default model H 384 / 12 heads /
   1 layer / I 48 / L 32 in bf16, the same seed). `DeviceEvalSet.from_rows` is timed once; then, in ONE process and after a
   warm-up of both paths, `module.evaluate(rows)` and `evalset.evaluate()` alternate --reps times each, a host clock
   around synchronised work; medians and spreads (max - min) of both, the HIP-event time of one resident pass
   (`evaluate_device`, no read-back), the largest difference between the two paths' seven means, both `num_rows`.
2. `Trainer.fit` on config-2-shaped batches (batch 512, L 200, H 128, 4 layers, bf16, dense rows) with the same users as
   the validation set of that model, a pass every 12 batches (one ML-1M epoch of 6 040 users): `elapsed` and
   `val_elapsed`; then the same loop with `module.evaluate(rows)` called by hand at the same cadence.

Prints one JSON line."""

import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd", ROOT / "scripts"):
    sys.path.insert(0, str(p))

import xfmr_rec_amd as X  # noqa: E402
from bench_eval import rows_ml1m  # noqa: E402
from xfmr_rec_amd.retrieval import METRIC_NAMES  # noqa: E402


def unit_table(V, H):
    g = torch.Generator().manual_seed(0)
    table = torch.randn(V + 1, H, generator=g)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    return table.cuda()


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_ms": round(1e3 * float(np.median(ts)), 3), "min_ms": round(1e3 * min(ts), 3),
            "max_ms": round(1e3 * max(ts), 3), "spread_ms": round(1e3 * (max(ts) - min(ts)), 3)}


def standalone(args, rows):
    V, H = args.items, 384
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=12, intermediate_size=48, num_hidden_layers=1,
                             max_seq_length=32, top_k=20)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V, H))
    mod.eval()
    t_build, es = host_timed(lambda: X.DeviceEvalSet.from_rows(mod, rows, batch_size=args.batch_size))
    for _ in range(2):  # warm-up of both paths (plans, allocator)
        mod.evaluate(rows, batch_size=args.batch_size)
        es.evaluate()
    t_old, t_new, old, new = [], [], None, None
    for _ in range(args.reps):
        t, old = host_timed(lambda: mod.evaluate(rows, batch_size=args.batch_size))
        t_old.append(t)
        t, new = host_timed(es.evaluate)
        t_new.append(t)
    ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        es.evaluate_device()
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    return {
        "packed": bool(es.packed), "chunks": len(es.plan.chunks), "tokens": int(es.plan.hist.size), "reps": args.reps,
        "from_rows_build_s": round(t_build, 4),
        "module_evaluate": stats(t_old), "evalset_evaluate": stats(t_new),
        "speedup_of_medians": round(float(np.median(t_old) / np.median(t_new)), 1),
        "resident_pass_event_ms": {"median": round(float(np.median(ev)), 3), "min": round(min(ev), 3), "max": round(max(ev), 3)},
        "max_mean_diff": max(abs(old[f"val/{n}"] - new[f"val/{n}"]) for n in METRIC_NAMES),
        "ndcg_module": old["val/retrieval_normalized_dcg"], "ndcg_evalset": new["val/retrieval_normalized_dcg"],
        "num_rows_module": old["val/num_rows"], "num_rows_evalset": new["val/num_rows"],
    }


def in_fit(args, rows):
    V, H, L, B = args.items, 128, 200, 512
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=4, intermediate_size=512, num_hidden_layers=4,
                             max_seq_length=L, top_k=20)
    table = unit_table(V, H)
    g = torch.Generator().manual_seed(1)
    batches = [{k: torch.randint(1, V + 1, (B, L), generator=g).cuda()
                for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")} for _ in range(args.fit_batches)]
    every = 12

    def module():
        mod = X.RecommenderLightningModule(conf)
        mod.configure_model()
        mod.model.set_table(table)
        return mod

    # (a) validation inside fit, resident
    mod = module()
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=args.batch_size)
    tr = X.Trainer(mod)
    tr.fit(batches[:every], val=es, val_check_interval=every)  # warm-up: plans, allocator, optimizer state
    torch.cuda.synchronize()
    t_fit, losses = host_timed(lambda: tr.fit(batches, val=es, val_check_interval=every))
    res = {"batches": len(losses), "val_every": every, "passes": len(tr.val_history), "fit_elapsed_s": round(t_fit, 4),
           "fit_val_elapsed_s": round(tr.val_elapsed, 4), "fit_val_ms_per_pass": round(1e3 * tr.val_elapsed / len(tr.val_history), 3),
           "fit_ndcg_last": tr.val_history[-1]["val/retrieval_normalized_dcg"], "val_tokens": int(es.plan.hist.size)}
    # (b) the same loop, module.evaluate(rows) by hand at the same cadence
    mod2 = module()
    tr2 = X.Trainer(mod2)
    for b in batches[:every]:
        tr2.fit_step(b)
    mod2.evaluate(rows, batch_size=args.batch_size)
    torch.cuda.synchronize()
    t_val = 0.0
    t0 = time.perf_counter()
    for i, b in enumerate(batches, 1):
        tr2.fit_step(b)
        if i % every == 0:
            torch.cuda.synchronize()
            tv = time.perf_counter()
            hand = mod2.evaluate(rows, batch_size=args.batch_size)
            t_val += time.perf_counter() - tv
    torch.cuda.synchronize()
    t_hand = time.perf_counter() - t0
    res |= {"hand_elapsed_s": round(t_hand, 4), "hand_val_elapsed_s": round(t_val, 4),
            "hand_val_ms_per_pass": round(1e3 * t_val / (len(batches) // every), 3),
            "hand_ndcg_last": hand["val/retrieval_normalized_dcg"],
            "train_s_fit": round(t_fit - tr.val_elapsed, 4), "train_s_hand": round(t_hand - t_val, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3900)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--fit-batches", type=int, default=48)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be >= 10")
    torch.cuda.set_device(0)
    rows, lens = rows_ml1m(args.users, args.items, np.random.default_rng(0))
    res = {"users": args.users, "items": args.items, "hist_len_median": float(np.median(lens)), "batch_size": args.batch_size}
    res["standalone"] = standalone(args, rows)
    if not args.skip_fit:
        res["in_fit"] = in_fit(args, rows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
