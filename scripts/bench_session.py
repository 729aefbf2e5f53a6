#!/usr/bin/env python3
"""Cost of one appended event per session: the cached path (`xfmr_session_append` of one row per active session +
`xfmr_session_pool`) against what a caller has without it, `encode_batch` of the full histories -- the same library and
the same build, run as the baseline. bench.py is not involved.

BASELINE config 2's model (H 128 / 4 heads / 4 layers / I 512 / max_seq_length 200, bf16, untrained) over 3 883 items;
history lengths 50 and 200, active sessions 1, 64 and 1 024. Per shape, in ONE process and after a warm-up of all, the paths
alternate --reps times; every figure is a HIP-event time around the calls (so host time between launches counts: it is
what a caller waits for):

  append+pool    ops.session_append (every session's token at position len - 1, index tensors already on the device; the
                 call rewrites the same position each repeat, so the state stays as prefilled) + ops.session_pool
  encode_batch   model.encode_batch(histories): host packing, xfmr_encoder_infer on the packed rows, xfmr_pool_rows
  encode_packed  the device part of the same: model.sentence_embeddings on an already packed batch
  search         items_index.search_batch of the pooled embeddings, top 20, histories excluded -- once per shape, for scale

`--profile-only` runs 20 appends at 1 024 x 200 and nothing else: the shape a `rocprofv3 --kernel-trace --stats` run of its own
takes the attend kernel's time from (the bytes it must read are printed by the normal run).

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
from bench_eval_ranks import alternate, event_ms, unit_table  # noqa: E402
from xfmr_rec_amd import ops  # noqa: E402
from xfmr_rec_amd.session import SessionEncoder  # noqa: E402

H, HEADS, LAYERS, INTER, MAX_LEN, ITEMS = 128, 4, 4, 512, 200, 3883


def module():
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=HEADS, intermediate_size=INTER, num_hidden_layers=LAYERS,
                             max_seq_length=MAX_LEN, precision="bf16", top_k=20)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(ITEMS, H))
    return mod.eval()


def prefilled(mod, sessions, length, rng):
    """(encoder with every slot holding `length` items, the histories, the device tensors of the last token's append)."""
    hists = rng.integers(1, ITEMS + 1, (sessions, length)).tolist()
    enc = SessionEncoder(mod.model, sessions, max_rows_per_call=8192)
    enc.prefill(list(range(sessions)), hists)
    dev = mod.model.device
    rows = dict(item=torch.tensor([h[-1] for h in hists], dtype=torch.int64, device=dev),
                slot=torch.arange(sessions, dtype=torch.int32, device=dev),
                pos=torch.full((sessions,), length - 1, dtype=torch.int32, device=dev),
                lens=torch.full((sessions,), length, dtype=torch.int32, device=dev))
    return enc, hists, rows


def append_pool(mod, enc, rows):
    c = mod.model.config
    ops.session_append(enc.cfg, mod.model.flat.detach(), enc.state, enc.n_slots, rows["item"], rows["slot"], rows["pos"],
                       mod.model.embeddings, enc.workspace, want_tok=False)
    return ops.session_pool(enc.cfg, enc.state, enc.n_slots, rows["slot"], rows["lens"], c.pooling_mode,
                            normalize=bool(c.is_normalized))


def attend_bytes(sessions, length, plan):
    """What the attend kernels of ONE append call must read: per layer and (session, head) the K and V rows 0 .. length - 1 and
    the mask bytes, plus the query row; and write: the context row."""
    hs, es = H // HEADS, plan["kv_bytes"]
    per_pair = 2 * length * hs * es + length + 2 * hs * (2 if plan["bf16_storage"] else 4)
    return LAYERS * sessions * HEADS * per_pair


def one_shape(mod, sessions, length, reps):
    enc, hists, rows = prefilled(mod, sessions, length, np.random.default_rng(sessions * 1000 + length))
    model, dev = mod.model, mod.model.device
    lens = [length] * sessions
    hist = torch.tensor(hists, dtype=torch.int64, device=dev)
    order, offs64 = ops.length_order(lens)
    packed = ops.pack_rows(hist, hist, None, offs64.to(dev), int(offs64[-1]), order=order.to(dev)) | {"batch": sessions, "seq_len": length}

    def encode_packed():
        with torch.no_grad(), model.eval_mode():
            return model.sentence_embeddings(packed)

    t = alternate({"append+pool": lambda: append_pool(mod, enc, rows), "encode_batch": lambda: model.encode_batch(hists),
                   "encode_packed": encode_packed}, reps)
    emb = append_pool(mod, enc, rows)
    full = model.encode_batch(hists)
    err = float((emb - full).abs().max())
    mod.items_index.search_batch(emb, hists, top_k=20)
    search_ms = event_ms(lambda: mod.items_index.search_batch(emb, hists, top_k=20))
    return {"sessions": sessions, "length": length, "reps": reps, "times": t, "search_ms_once": round(search_ms, 3),
            "max_abs_diff_vs_encode_batch": err, "state_bytes_per_slot": enc.state_bytes_per_slot,
            "attend_bytes_per_call": attend_bytes(sessions, length, enc.plan),
            "ratio_encode_batch_over_append": round(t["encode_batch"]["median_ms"] / t["append+pool"]["median_ms"], 2),
            "ratio_encode_packed_over_append": round(t["encode_packed"]["median_ms"] / t["append+pool"]["median_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    mod = module()
    if args.profile_only:
        enc, _, rows = prefilled(mod, 1024, 200, np.random.default_rng(0))
        for _ in range(20):
            append_pool(mod, enc, rows)
        torch.cuda.synchronize()
        print(json.dumps({"profile_only": True, "appends": 20, "attend_launches": 20 * LAYERS,
                          "attend_bytes_per_call": attend_bytes(1024, 200, enc.plan)}))
        return
    res = {"model": dict(H=H, heads=HEADS, layers=LAYERS, inter=INTER, max_len=MAX_LEN, items=ITEMS, precision="bf16"),
           "plan": None, "shapes": []}
    for length in (50, 200):
        for sessions in (1, 64, 1024):
            res["shapes"].append(one_shape(mod, sessions, length, args.reps))
    res["plan"] = SessionEncoder(mod.model, 1, max_rows_per_call=1).plan
    print(json.dumps(res))


if __name__ == "__main__":
    main()
