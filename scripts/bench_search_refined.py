#!/usr/bin/env python3
"""The refined item search (`ExactItemIndex.search_refined`: bf16 MFMA shortlist + exact f32 refine + certificate) against
the exact search (`ExactItemIndex.search_batch`, xfmr_topk_tiled) of the same library in the same process. bench.py is not
involved.

Shapes (queries x items x H): 1 024 x 262 144 x 384 (the serving shape: one search per appended event of 1 024 sessions),
4 096 x 262 144 x 384 and 6 040 x 3 900 x 384; cosine, top_k 20, refine factor 4, no exclusions (their host-side CSR is
the same work on both paths). Two tables per shape: unit Gaussian rows, and clustered rows (256 unit Gaussian centres +
noise of relative size --cluster-noise, normalised; the queries are noisy copies of random items, as a user embedding
sits near the items of its history). Per table, after a warm-up of all, the paths alternate --reps times in one process;
every figure is a HIP-event time around the call:

  exact            search_batch
  refined          search_refined(exact=False): the two launches, nothing read back
  refined+fallback search_refined(exact=True): + the read-back of certified.all() and a search_batch of the rows that are
                   not certified

and the share of certified rows, the agreement of exact=True with search_batch (torch.equal) and the coarse pass's
arithmetic rate (2 x queries x items x H FLOP over the refined call's median). Prints one JSON line."""

import argparse
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd", ROOT / "scripts"):
    sys.path.insert(0, str(p))

from bench_eval_ranks import alternate, unit_table  # noqa: E402
from xfmr_rec_amd.retrieval import ExactItemIndex  # noqa: E402

SHAPES = ((1024, 262144), (4096, 262144), (6040, 3900))


def unit_rows(n, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, H, generator=g, device="cuda")
    return x / x.norm(dim=-1, keepdim=True)


def clustered(V, B, H, noise, seed):
    """(table, queries): items = normalised(centre + noise * unit Gaussian direction), queries = the same around items."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = unit_rows(256, H, seed + 1)
    which = torch.randint(0, 256, (V + 1,), generator=g, device="cuda")
    table = centres[which] + noise * unit_rows(V + 1, H, seed + 2)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    near = torch.randint(1, V + 1, (B,), generator=g, device="cuda")
    q = table[near] + noise * unit_rows(B, H, seed + 3)
    return table, q / q.norm(dim=-1, keepdim=True)


def one(table, q, args):
    index = ExactItemIndex(table, index_metric="cosine")
    index.table_bf16, index.norm_bounds  # (made once, outside the timed calls)
    kw = dict(top_k=args.top_k, refine_factor=args.refine)
    fns = {"exact": lambda: index.search_batch(q, None, top_k=args.top_k),
           "refined": lambda: index.search_refined(q, None, exact=False, **kw),
           "refined+fallback": lambda: index.search_refined(q, None, exact=True, **kw)}
    out = alternate(fns, args.reps)
    want = index.search_batch(q, None, top_k=args.top_k)
    idx, score, cert = index.search_refined(q, None, exact=True, **kw)
    ridx = index.search_refined(q, None, exact=False, **kw)[0]
    B, V, H = q.shape[0], table.shape[0], q.shape[1]
    out.update(certified_share=round(float(cert.float().mean()), 4),
               exact_true_equals_search_batch=bool(torch.equal(idx, want[0]) and torch.equal(score, want[1])),
               uncertified_rows_that_differ=int((ridx != want[0]).any(dim=1).sum()),
               coarse_tflops=round(2.0 * B * V * H / (out["refined"]["median_ms"] * 1e-3) / 1e12, 1),
               exact_tflops=round(2.0 * B * V * H / (out["exact"]["median_ms"] * 1e-3) / 1e12, 1),
               speedup_refined=round(out["exact"]["median_ms"] / out["refined"]["median_ms"], 2),
               speedup_with_fallback=round(out["exact"]["median_ms"] / out["refined+fallback"]["median_ms"], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--refine", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=384)
    ap.add_argument("--cluster-noise", type=float, default=0.5)
    ap.add_argument("--shapes", default=",".join(f"{b}x{v}" for b, v in SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    result = {"top_k": args.top_k, "refine_factor": args.refine, "H": args.hidden, "metric": "cosine", "shapes": {}}
    for shape in args.shapes.split(","):
        B, V = (int(x) for x in shape.split("x"))
        gauss = one(unit_table(V - 1, args.hidden), unit_rows(B, args.hidden, 7), args)
        table, q = clustered(V - 1, B, args.hidden, args.cluster_noise, 11)
        result["shapes"][shape] = {"unit_gaussian": gauss, "clustered": one(table, q, args)}
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
