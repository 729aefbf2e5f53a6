#!/usr/bin/env python3
"""Validation cost of the rank path (`DeviceEvalSet.evaluate(cutoffs=...)`: xfmr_target_ranks + xfmr_rank_metrics_sum)
against the resident top-k pass (`DeviceEvalSet.evaluate()`: xfmr_topk_tiled + xfmr_retrieval_metrics_sum) at top_k = 20
(bench.py is not involved).

Two sets, the users of scripts/bench_eval.py (lognormal history lengths, 1-5 targets per user, seed 0) under the
reference-default model (H 384 / 12 heads / 1 layer / I 48 / L 32, bf16): 6 040 users x 3 900 items, and 4 096 users x
262 144 items. Per set, in ONE process and after a warm-up of all three, a resident pass through the top-k path, the rank
path at 1 cutoff (20) and the rank path at 5 cutoffs (5, 10, 20, 100, 500) alternate --reps times each; every pass is
timed by HIP events around the device work (no read-back). The same three are timed again from a fixed embedding (the
retrieval and metrics launches alone, the encoder left out). The two paths' seven means at cutoff 20 are compared.

Prints one JSON line."""

import argparse
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd", ROOT / "scripts"):
    sys.path.insert(0, str(p))

import xfmr_rec_amd as X  # noqa: E402
from bench_eval import rows_ml1m  # noqa: E402
from xfmr_rec_amd.retrieval import METRIC_NAMES, rank_metrics_sum, retrieval_metrics_sum  # noqa: E402

ONE, FIVE = (20,), (5, 10, 20, 100, 500)


def unit_table(V, H):
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(V + 1, H, generator=g, device="cuda")
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    return table


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_ms": round(max(ts) - min(ts), 3)}


def alternate(fns, reps):
    for _ in range(2):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(event_ms(f))
    return {k: stats(v) for k, v in ts.items()}


def one_set(users, items, args):
    H = 384
    rows, lens = rows_ml1m(users, items, np.random.default_rng(0))
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=12, intermediate_size=48, num_hidden_layers=1,
                             max_seq_length=32, top_k=20)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(items, H))
    mod.eval()
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=args.batch_size)
    csr = (es.targets, es.target_offsets)
    whole = alternate({"topk_20": es.evaluate_device, "ranks_1_cutoff": lambda: es.evaluate_ranks_device(ONE),
                       "ranks_5_cutoffs": lambda: es.evaluate_ranks_device(FIVE)}, args.reps)
    emb = es.encode()
    tail = alternate({
        "topk_20": lambda: retrieval_metrics_sum(es.recommend(emb)[0], csr, None, top_k=20),
        "ranks_1_cutoff": lambda: rank_metrics_sum(es.target_ranks(emb), csr, ONE),
        "ranks_5_cutoffs": lambda: rank_metrics_sum(es.target_ranks(emb), csr, FIVE),
    }, args.reps)
    ranks = es.target_ranks(emb)
    metrics_only = alternate({"rank_metrics_1_cutoff": lambda: rank_metrics_sum(ranks, csr, ONE),
                              "rank_metrics_5_cutoffs": lambda: rank_metrics_sum(ranks, csr, FIVE)}, args.reps)
    plain, cut = es.evaluate(), es.evaluate(cutoffs=FIVE)
    return {
        "users": users, "items": items, "H": H, "rows": len(es), "chunks": len(es.plan.chunks),
        "targets": int(es.targets.numel()), "hist_len_median": float(np.median(lens)), "reps": args.reps,
        "resident_pass": whole, "from_fixed_embedding": tail, "metrics_launches_only": metrics_only,
        "max_mean_diff_at_20": max(abs(plain[f"val/{n}"] - cut[f"val/{n}@20"]) for n in METRIC_NAMES),
        "ndcg": {str(k): cut[f"val/retrieval_normalized_dcg@{k}"] for k in FIVE},
        "recall": {str(k): cut[f"val/retrieval_recall@{k}"] for k in FIVE},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be >= 10")
    torch.cuda.set_device(0)
    res = {"batch_size": args.batch_size, "cutoffs_1": list(ONE), "cutoffs_5": list(FIVE), "sets": [one_set(6040, 3900, args)]}
    if not args.skip_large:
        res["sets"].append(one_set(4096, 262144, args))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
