#!/usr/bin/env python3
"""Validation cost, per row against batched, on a synthetic ML-1M-shaped set (bench.py is not involved).

1. RecommenderLightningModule.validation_step over every row (B = 1 forward + xfmr_topk + metrics per row) against
   evaluate(rows) (encode_batch + xfmr_topk_tiled + one metrics launch per pass), host clock around synchronised work;
   the two sets of means are compared.
2. xfmr_topk (scan, one workgroup per query, (B, V) workspace) against xfmr_topk_tiled at (B 6 040, V 3 900, H 384)
   and (B 4 096, V 262 144, H 384), HIP events, median of --reps; the two kernels' lists are compared (equal up to
   near-tied scores at the k-th place).

Shape: 6 040 users, 3 900 items, the reference-default model (H 384, 12 heads, 1 layer, I 48, L 32, bf16), lognormal
history lengths clamped to [20, 2 000], 1-5 targets per user. Prints one JSON line."""

import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    sys.path.insert(0, str(p))

import xfmr_rec_amd as X  # noqa: E402
from xfmr_rec_amd import _native as N  # noqa: E402
from xfmr_rec_amd.retrieval import METRIC_NAMES, ExactItemIndex  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3


def rows_ml1m(n_users, V, rng):
    lens = np.clip(np.exp(rng.normal(np.log(100), 1.0, n_users)), 20, 2000).astype(int)
    rows = []
    for n in lens:
        h = rng.integers(1, V + 1, int(n))
        t = rng.integers(1, V + 1, int(rng.integers(1, 6)))
        rows.append({"history": {"item_id": h.tolist()}, "target": {"item_id": t.tolist(), "label": [True] * len(t)}})
    return rows, lens


def timed_events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def compare_lists(a, b, ref_score, tol=1e-5):
    """rows whose sets differ, and of those how many differ only where the k-th place is a near tie."""
    ai, bi, s = a.cpu().numpy(), b.cpu().numpy(), ref_score.cpu().numpy()
    bad, near = 0, 0
    for r in range(ai.shape[0]):
        if set(ai[r].tolist()) != set(bi[r].tolist()):
            d = set(ai[r].tolist()) ^ set(bi[r].tolist())
            if len(d) <= 2 and np.isfinite(s[r, -1]):
                near += 1
            else:
                bad += 1
    return bad, near


def kernel_pair(B, V, H, k, reps, rng):
    g = torch.Generator(device="cuda").manual_seed(B + V)
    table = torch.randn(V + 1, H, generator=g, device="cuda")
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    q = torch.randn(B, H, generator=g, device="cuda")
    excl = [rng.integers(1, V + 1, int(n)).tolist() for n in rng.integers(20, 200, B)]
    idx = ExactItemIndex(table)
    scan = idx.search(q, excl, top_k=k)
    tiled = idx.search_batch(q, excl, top_k=k)
    torch.cuda.synchronize()
    bad, near = compare_lists(tiled[0], scan[0], scan[1])
    score_err = float(((tiled[1] - scan[1]).abs() / scan[1].abs().clamp(min=1.0)).nan_to_num(0.0).max())
    # kernel-only times: the host-side exclusion CSR built once, outside the timed region
    lib = N.load()
    from xfmr_rec_amd.retrieval import _csr, sorted_exclusion_csr

    ex, exo = _csr(excl, "cuda")
    f, o = sorted_exclusion_csr(excl)
    sx, sxo = torch.from_numpy(f).cuda(), torch.from_numpy(o).cuda()
    oi = torch.empty((B, k), dtype=torch.int64, device="cuda")
    os_ = torch.empty((B, k), dtype=torch.float32, device="cuda")
    nb = lib.xfmr_topk_workspace(B, V + 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    nt = lib.xfmr_topk_tiled_workspace(B, V + 1, k)
    wt = torch.empty(nt, dtype=torch.uint8, device="cuda")

    def run_scan():
        N.check(lib.xfmr_topk(N.ptr(q), N.ptr(table), N.ptr(idx.rnorm), V + 1, B, H, N.ptr(ex), N.ptr(exo), k, 0,
                              N.ptr(oi), N.ptr(os_), N.ptr(ws), nb, N.stream()), "xfmr_topk")

    def run_tiled():
        N.check(lib.xfmr_topk_tiled(N.ptr(q), N.ptr(table), N.ptr(idx.rnorm), None, V + 1, B, H, N.ptr(sx), N.ptr(sxo),
                                    k, 0, N.ptr(oi), N.ptr(os_), N.ptr(wt), nt, N.stream()), "xfmr_topk_tiled")

    run_scan(), run_tiled()
    t_scan = timed_events(run_scan, reps)
    t_tiled = timed_events(run_tiled, reps)
    flop = 2.0 * B * (V + 1) * H
    return {
        "B": B, "V": V, "H": H, "k": k, "scan_ms": round(t_scan, 3), "tiled_ms": round(t_tiled, 3),
        "speedup": round(t_scan / t_tiled, 2), "tiled_tflops": round(flop / t_tiled / 1e9, 1),
        "tiled_frac_of_peak": round(flop / t_tiled / 1e9 / PEAK_F32_MFMA_TFLOPS, 3),
        "scan_workspace_mb": round(nb / 2**20, 1), "tiled_workspace_mb": round(nt / 2**20, 2),
        "rows_sets_differ_near_tie": near, "rows_sets_differ_otherwise": bad, "max_score_err": score_err,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3900)
    ap.add_argument("--per-row-limit", type=int, default=0, help="time the per-row loop on the first N rows only")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    V, H, k = args.items, 384, 20
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=12, intermediate_size=48, num_hidden_layers=1,
                             max_seq_length=32, top_k=k)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    g = torch.Generator().manual_seed(0)
    table = torch.randn(V + 1, H, generator=g)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    mod.model.set_table(table.cuda())
    mod.eval()
    rows, lens = rows_ml1m(args.users, V, rng)
    res = {"users": args.users, "items": V, "hist_len_median": float(np.median(lens)), "packed":
           bool(mod.model.supports_packed_rows(32))}

    # warm-up both paths (plans, allocator)
    mod.evaluate(rows[:64])
    for r in rows[:8]:
        mod.validation_step(r)
    torch.cuda.synchronize()
    n_row = args.per_row_limit or len(rows)
    t0 = time.perf_counter()
    per_row = [mod.validation_step(r) for r in rows[:n_row]]
    torch.cuda.synchronize()
    t_row = time.perf_counter() - t0
    t0 = time.perf_counter()
    ev = mod.evaluate(rows[:n_row], batch_size=args.batch_size)
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    mod.evaluate(rows, batch_size=args.batch_size)
    torch.cuda.synchronize()
    t_batch_all = time.perf_counter() - t0
    means = {n: float(np.mean([float(p[f"val/{n}"]) for p in per_row if p])) for n in METRIC_NAMES}
    res |= {
        "per_row_rows": n_row, "per_row_s": round(t_row, 3), "per_row_ms_per_row": round(1e3 * t_row / n_row, 3),
        "evaluate_s_same_rows": round(t_batch, 4), "evaluate_s_all_rows": round(t_batch_all, 4),
        "validation_speedup": round(t_row / t_batch, 1),
        "ndcg_per_row": means["retrieval_normalized_dcg"], "ndcg_evaluate": ev["val/retrieval_normalized_dcg"],
        "max_mean_diff": max(abs(means[n] - ev[f"val/{n}"]) for n in METRIC_NAMES),
    }
    res["kernels"] = [kernel_pair(6040, 3900, H, k, args.reps, rng)]
    if not args.skip_large:
        res["kernels"].append(kernel_pair(4096, 262144, H, k, args.reps, rng))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
