#!/usr/bin/env python3
"""What a matrix of ``Trainer.fit`` calls computes, as JSON that two trees can be compared on byte for byte (results:
profiles/fit_loop.md). The model of tests/test_gpu_resume.py: H 64, L 16, one layer, 2 heads, V 200; 40 rows in batches
of 8; 12 validation rows; dropout on.

Per case: the losses as ``float.hex()``, ``val_history``, ``best_*``, ``graph_choice``, the ``loop`` dict of
``state_dict()`` without ``train_seconds``, and the sorted keys of ``last.ckpt`` where one was written. ``graph="auto"``
chooses by a clock: its case is printed (that it completed, and what it chose), not written.

    python scripts/fit_trace.py --out trace.json        # the script imports the package of the tree it lies in
"""
import argparse
import json
import pathlib
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
H, L, V, R, B = 64, 16, 200, 40, 8
OPTS = dict(gradient_clip_val=0.5, lr_scheduler={"name": "warmup_cosine", "warmup_steps": 2, "total_steps": 8},
            accumulate_grad_batches=2)
FIXED = dict(drop_last=True, fixed_width=True)


class Setup:
    def __init__(self):
        import xfmr_rec_amd as X
        from xfmr_rec_amd.data import DeviceSeqDataset, SeqDataConfig

        self.X = X
        rng = np.random.default_rng(6)
        lens = [int(x) for x in rng.integers(2, 30, R)]
        hs = [rng.integers(1, V + 1, n) for n in lens]
        ls = [np.concatenate([rng.random(n - 1) < 0.6, [True]]) for n in lens]
        self.ds = DeviceSeqDataset(SeqDataConfig(max_seq_length=L, pos_lookahead=0), hs, ls, V)
        self.conf = X.LightningConfig(hidden_size=H, num_attention_heads=2, intermediate_size=2 * H, num_hidden_layers=1,
                                      max_seq_length=L)
        table = torch.randn(V + 1, H, generator=torch.Generator().manual_seed(7))
        table = table / table.norm(dim=-1, keepdim=True)
        table[0] = 0.0
        self.table = table.to(DEV)
        self.rows = []
        for _ in range(12):
            h = [f"i{x}" for x in rng.integers(1, V + 1, int(rng.integers(1, 20)))]
            t = [f"i{x}" for x in rng.integers(1, V + 1, 3)]
            self.rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": [True, False, True]}})

    def trainer(self, other_weights=False, **kw):
        mod = self.X.RecommenderLightningModule(self.conf)
        mod.configure_model()
        mod.model.set_table(self.table)
        mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
        if other_weights:
            with torch.no_grad():
                mod.model.flat.mul_(-0.5).add_(0.01)
        return self.X.Trainer(mod, **kw)

    def loader(self, **kw):
        from xfmr_rec_amd.data import DeviceSeqLoader

        return DeviceSeqLoader(self.ds, B, **{"seed": 3, **kw})

    def evalset(self, tr):
        return self.X.DeviceEvalSet.from_rows(tr.module, self.rows, batch_size=8)

    def host_batches(self):
        """Five collated batches in host memory; the first has 4 rows, so the ring is made again for the second."""
        from xfmr_rec_amd.data import SEQ_BATCH_KEYS

        out = []
        for i, rows in enumerate([range(0, 4)] + [range(8 * j, 8 * j + 8) for j in range(1, 5)]):
            b = self.ds.sample_batch(list(rows), seed=i)
            out.append({k: b[k].cpu() for k in SEQ_BATCH_KEYS})
        return out


def record(S, tr, losses, d):
    """One call's results; paths below the case's directory ``d`` are written relative to it."""
    def rel(v):
        return v.replace(str(d), "<dir>") if isinstance(v, str) else v

    torch.cuda.synchronize()
    loop = {k: rel(v) for k, v in tr.state_dict()["loop"].items() if k != "train_seconds"}
    ck = pathlib.Path(d) / "last.ckpt"
    keys = None
    if ck.exists():
        state = S.X.read_checkpoint(ck)
        keys = sorted(state) + sorted(f"loop.{k}" for k in state["loop"])
    return {"losses": [float(v).hex() for v in losses], "val_history": tr.val_history, "best_score": tr.best_score,
            "best_step": tr.best_step, "best_model_path": rel(tr.best_model_path), "graph_choice": tr.graph_choice,
            "stopped": [tr.stopped_early, tr.stopped_on_time], "optimizer_step": tr._optimizer_steps(), "loop": loop,
            "checkpoint_keys": keys}


def run(S, source, trainer_kw=None, with_val=True, **fit_kw):
    tr = S.trainer(**(trainer_kw or {}))
    batches = S.loader(**source) if isinstance(source, dict) else source
    losses = tr.fit(batches, **fit_kw, **({"val": S.evalset(tr)} if with_val else {}))
    if isinstance(source, dict):
        batches.close()
    return tr, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    S = Setup()
    epochs = dict(max_epochs=3, val_check_interval=4)
    cases = {
        "host list (ring)": lambda d: run(S, S.host_batches(), with_val=False),
        "loader, one pass": lambda d: run(S, {}, with_val=False),
        "epochs, val every 4 batches": lambda d: run(S, {}, checkpoint_dir=d, **epochs),
        "epochs, val every 2nd epoch, 3 batches each": lambda d: run(S, {}, max_epochs=3, check_val_every_n_epoch=2,
                                                                      limit_train_batches=3),
        "graph on": lambda d: run(S, FIXED, graph="on", checkpoint_dir=d, checkpoint_every_n_steps=2, **epochs),
        # (14 of the 15 batches: state_dict() is refused between the two micro-batches of one optimizer step)
        "accumulation 2, clip, schedule": lambda d: run(S, {}, trainer_kw=OPTS, max_steps=14, **epochs),
    }
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n, (name, case) in enumerate(cases.items()):
            d = pathlib.Path(tmp) / str(n)
            d.mkdir()
            out[name] = record(S, *case(d), d)
            print("done:", name, flush=True)
        # a run cut at batch 7 (with a periodic last.ckpt in front of the final one), then resumed from the file alone
        d = pathlib.Path(tmp) / "resume"
        d.mkdir()
        tr, first = run(S, {}, max_steps=7, save_last=True, checkpoint_dir=d, checkpoint_every_n_steps=2, **epochs)
        out["interrupted at 7"] = record(S, tr, first, d)
        tr2 = S.trainer(other_weights=True)
        ld = S.loader()
        second = tr2.fit(ld, val=S.evalset(tr2), ckpt_path=d / "last.ckpt", **epochs)
        ld.close()
        out["resumed from 7"] = record(S, tr2, second, d)
        print("done: interrupted + resumed", flush=True)
        tr, losses = run(S, FIXED, with_val=False, graph="auto", graph_probe_steps=4, max_epochs=3)
        print(f"graph='auto' completed: {len(losses)} steps, chose {tr.graph_choice!r}, probe {tr.graph_probe}", flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1, sort_keys=True, default=lambda v: v.item()) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
