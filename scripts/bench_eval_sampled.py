#!/usr/bin/env python3
"""Validation cost of the sampled-candidate protocol (`SampledEvalSet.evaluate`: xfmr_candidate_ranks +
xfmr_rank_metrics_sum, 100 negatives per row) against the full-catalogue rank pass of the same rows
(`DeviceEvalSet.evaluate(cutoffs=)`: xfmr_target_ranks + xfmr_rank_metrics_sum). bench.py is not involved.

Two sets, the users of scripts/bench_eval.py (lognormal history lengths, 1-5 targets per user, seed 0) under the
reference-default model (H 384 / 12 heads / 1 layer / I 48 / L 32, bf16): 6 040 users x 3 883 items (ML-1M) and 4 096
users x 262 144 items. Per set, in ONE process and after a warm-up of both, a sampled pass and a full pass alternate
--reps times each at cutoff 10; every pass is timed by HIP events around the device work (no read-back of the sums).
The same two are timed again from a fixed embedding (the rank and metrics launches alone), and so is the candidate
kernel alone (`ExactItemIndex.rank_among` per chunk), reported as achieved bytes/s on its algorithmic bytes
(candidates + targets) * H * 4.

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
from bench_eval_ranks import alternate, unit_table  # noqa: E402
from xfmr_rec_amd.retrieval import rank_metrics_sum  # noqa: E402

CUT = (10,)


def one_set(users, items, args):
    H = 384
    rows, lens = rows_ml1m(users, items, np.random.default_rng(0))
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=12, intermediate_size=48, num_hidden_layers=1,
                             max_seq_length=32, top_k=10)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(items, H))
    mod.eval()
    full = X.DeviceEvalSet.from_rows(mod, rows, batch_size=args.batch_size)
    t0 = time.perf_counter()
    sampled = X.SampledEvalSet.from_rows(mod, rows, num_negatives=args.negatives, seed=0, batch_size=args.batch_size)
    build_s = time.perf_counter() - t0
    csr = (full.targets, full.target_offsets)
    whole = alternate({"sampled": lambda: sampled.evaluate_ranks_device(CUT), "full": lambda: full.evaluate_ranks_device(CUT)},
                      args.reps)
    emb = full.encode()
    tail = alternate({"sampled": lambda: rank_metrics_sum(sampled.target_ranks(emb), csr, CUT),
                      "full": lambda: rank_metrics_sum(full.target_ranks(emb), csr, CUT)}, args.reps)
    kernel = alternate({"candidate_ranks": lambda: sampled.target_ranks(emb), "target_ranks": lambda: full.target_ranks(emb)},
                       args.reps)
    n_cand = int(sampled.candidate_offsets[-1] - sampled.candidate_offsets[0])
    n_tgt = int(full.target_offsets[-1] - full.target_offsets[0])
    nbytes = (n_cand + n_tgt) * H * 4
    ev_s, ev_f = sampled.evaluate(cutoffs=CUT), full.evaluate(cutoffs=CUT)
    return {
        "users": users, "items": items, "H": H, "rows": len(full), "chunks": len(full.plan.chunks), "negatives": args.negatives,
        "candidates": n_cand, "targets": n_tgt, "hist_len_median": float(np.median(lens)), "reps": args.reps,
        "sampled_set_build_s": round(build_s, 3), "resident_pass": whole, "from_fixed_embedding": tail, "rank_launches_only": kernel,
        "candidate_kernel_algorithmic_bytes": nbytes,
        "candidate_kernel_GBps": round(nbytes / (kernel["candidate_ranks"]["median_ms"] * 1e-3) / 1e9, 1),
        "hit_rate@10": {"sampled": ev_s["val/retrieval_hit_rate@10"], "full": ev_f["val/retrieval_hit_rate@10"]},
        "ndcg@10": {"sampled": ev_s["val/retrieval_normalized_dcg@10"], "full": ev_f["val/retrieval_normalized_dcg@10"]},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--negatives", type=int, default=100)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be >= 10")
    torch.cuda.set_device(0)
    res = {"batch_size": args.batch_size, "cutoffs": list(CUT), "sets": [one_set(6040, 3883, args)]}
    if not args.skip_large:
        res["sets"].append(one_set(4096, 262144, args))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
