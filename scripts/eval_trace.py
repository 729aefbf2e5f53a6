#!/usr/bin/env python3
"""What every evaluation surface computes, as JSON that two trees can be compared on byte for byte (results:
profiles/eval_path.md). The model of tests/test_gpu_evalset.py: H 64, 2 heads, 2 layers, L 24, 300 items; 40 validation
rows with histories of 0 .. 3 L ids, some without a positive target, some with unknown ids; once in bf16 (the packed
layout) and once in fp32 (the padded one). The single-query surfaces run in eval mode; the batched ones with the module in
training mode at a pinned dropout step count, which they have to leave alone (the trace ends with both).

Cases: ``recommend`` / ``predict_step`` / ``recommend_batch`` / ``predict_batch`` (an empty history, a history of unknown
ids and integer ids among them), ``model.encode`` / ``encode_batch``, ``compute_metrics`` for a row with targets and for
one without, ``evaluate`` with ``batch_size`` 16 and 1000 and with ``cutoffs=(5, 20, 500)``, and of
``DeviceEvalSet.from_rows``: ``encode``, ``recommend``, ``target_ranks``, ``evaluate()``, ``evaluate(cutoffs=...)`` and
``Trainer.validate``. Floats are written as ``float.hex()``, integer tensors as lists, embeddings as the sha256 of their
bytes, dict keys in insertion order.

    python scripts/eval_trace.py --out trace.json       # the script imports the package of the tree it lies in
"""
import argparse
import hashlib
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
H, A, L, V, N_ROWS = 64, 2, 24, 300, 40
CUTOFFS = (5, 20, 500)


def enc(v):
    """Floats as ``float.hex()``, integer tensors as lists, float tensors of more than one row as the sha256 of their
    bytes, containers element by element (dicts in insertion order)."""
    if isinstance(v, dict):
        return {str(k): enc(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [enc(x) for x in v]
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    if torch.is_tensor(v):
        v = v.detach().cpu().contiguous()
        if not v.dtype.is_floating_point:
            return v.tolist()
        if v.dim() >= 2:
            return {"shape": list(v.shape), "dtype": str(v.dtype), "sha256": hashlib.sha256(v.numpy().tobytes()).hexdigest()}
        return [float(x).hex() for x in v.reshape(-1).tolist()]
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    return float(v).hex()


def val_rows():
    rng = np.random.default_rng(3)
    rows = []
    for u in range(N_ROWS):
        n = int(rng.integers(0, 3 * L + 1))
        h = [f"i{x}" for x in rng.integers(1, V + 1, n)]
        t = [f"i{x}" for x in rng.integers(1, V + 1, int(rng.integers(1, 5)))]
        lab = (rng.random(len(t)) < 0.7).tolist()
        if u % 7 == 3:
            lab = [False] * len(t)         # no positive target
        if u % 5 == 1:
            h.insert(len(h) // 2, "unknown-a")  # unknown ids are dropped
            t.append("unknown-b")
            lab.append(True)
        if u == 11:
            h = []                         # an empty history
        if u == 12:
            h = ["unknown-c"]              # empty once the unknown id is dropped
        rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": lab}})
    return rows


def module(X, precision):
    g = torch.Generator().manual_seed(0)
    table = torch.randn(V + 1, H, generator=g)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    mod = X.RecommenderLightningModule(X.LightningConfig(
        hidden_size=H, num_attention_heads=A, intermediate_size=2 * H, num_hidden_layers=2, max_seq_length=L,
        precision=precision, top_k=20))
    mod.configure_model()
    mod.model.set_table(table.to(DEV))
    mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
    mod.eval()  # (the single-query surfaces encode in the module's own mode)
    return mod


def trace(X, precision):
    mod = module(X, precision)
    rows = val_rows()
    res = {"packed": bool(mod.model.supports_packed_rows(L))}
    with_t = next(r for r in rows if any(r["target"]["label"]) and len(r["history"]["item_id"]) > 2)
    without_t = next(r for r in rows if not any(r["target"]["label"]) and len(r["history"]["item_id"]) > 2)
    ids = list(rows[0]["history"]["item_id"]) or ["i5", "i9"]
    histories = [ids, [], ["unknown-c"], [7, 9, 11, 7], ["i3", "unknown-a", "i4"]]
    for name, h in zip(("strings", "empty", "unknown only", "integers", "mixed"), histories):
        if h and h != ["unknown-c"]:  # (the single-query encoder has no empty sequence)
            res[f"recommend | {name}"] = mod.recommend(h, top_k=7, exclude_item_ids=h[:2])
            res[f"predict_step | {name}"] = mod.predict_step({"history": {"item_id": h}})
    res["recommend | no exclusions"] = mod.recommend(ids)
    res["model.encode"] = mod.model.encode(ids + ["unknown-a"])[None, :].repeat(2, 1)
    res["compute_metrics | targets"] = mod.compute_metrics(with_t)
    res["compute_metrics | no target"] = mod.compute_metrics(without_t, stage="test")
    # from here on in training mode at a pinned dropout step count: every batched surface has to leave both alone
    mod.train()
    mod.model._step = 5
    res["recommend_batch"] = mod.recommend_batch(histories, top_k=7, exclude_item_ids=[h[:2] for h in histories])
    res["recommend_batch | no exclusions"] = mod.recommend_batch(histories)
    res["predict_batch"] = mod.predict_batch([{"history": {"item_id": h}} for h in histories])
    res["predict_batch | rows"] = mod.predict_batch(rows)
    kept = [mod._to_idx_or_empty(list(r["history"]["item_id"])) for r in rows]
    res["encode_batch"] = mod.model.encode_batch(kept)
    res["evaluate | batch 16"] = mod.evaluate(rows, batch_size=16)
    res["evaluate | batch 1000"] = mod.evaluate(rows, stage="test", batch_size=1000)
    res["evaluate | cutoffs, batch 16"] = mod.evaluate(rows, batch_size=16, cutoffs=CUTOFFS)
    res["evaluate | cutoffs, batch 1000"] = mod.evaluate(rows, batch_size=1000, cutoffs=CUTOFFS)
    res["evaluate | cutoff 20 alone"] = mod.evaluate(rows, batch_size=16, cutoffs=20)
    res["evaluate | no rows"] = mod.evaluate([], cutoffs=(5,))
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    res["evalset | kept"] = es.kept
    res["evalset | encode"] = es.encode()
    res["evalset | recommend"] = es.recommend()
    res["evalset | target_ranks"] = es.target_ranks()
    res["evalset | evaluate"] = es.evaluate()
    res["evalset | evaluate cutoffs"] = es.evaluate(stage="test", cutoffs=CUTOFFS)
    res["evalset | evaluate cutoffs 20 first"] = es.evaluate(cutoffs=(20, 5, 500))
    res["evalset | evaluate_device"] = es.evaluate_device()
    res["evalset | evaluate_ranks_device"] = es.evaluate_ranks_device(CUTOFFS).reshape(-1)
    res["Trainer.validate"] = X.Trainer(mod).validate(es)
    res["state"] = {"training": bool(mod.model.training), "step": int(mod.model._step)}
    torch.cuda.synchronize()
    return enc(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import xfmr_rec_amd as X

    print("package:", pathlib.Path(X.__file__).parent, flush=True)
    res = {}
    for precision in ("bf16", "fp32"):
        res[precision] = trace(X, precision)
        print("done:", precision, len(res[precision]), "cases", flush=True)
    assert res["bf16"]["packed"] and not res["fp32"]["packed"]
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
