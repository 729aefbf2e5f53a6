#!/usr/bin/env python3
"""What a full-state checkpoint costs, beside the step it interrupts (results: profiles/checkpoint.md).

Per shape, in ONE process: the median of --reps Trainer.save_checkpoint calls (a stream sync in front, so that only the
device-to-host copies and the write are timed), the median of as many Trainer.load_checkpoint calls into a second trainer,
the file's size, and the step time of the same trainer on one resident batch (median of --steps steps by a host clock
around a synchronised step). No threshold: the table records what was measured.

    python scripts/bench_checkpoint.py [--reps 10] [--steps 30] [--dir DIR]
"""
import argparse
import pathlib
import statistics
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

DEV = "cuda"
SHAPES = {
    # BASELINE.md's configs: the MODEL is what a checkpoint holds; the batch only sets the step time beside it
    "config 2 (H 128, 4 layers, L 200)": dict(H=128, A=4, I=512, nL=4, L=200, B=512, V=3883),
    "config 4 (H 256, 6 layers, L 200)": dict(H=256, A=8, I=1024, nL=6, L=200, B=128, V=27278),
}


def trainer(s):
    import xfmr_rec_amd as X

    conf = X.LightningConfig(hidden_size=s["H"], num_attention_heads=s["A"], intermediate_size=s["I"],
                             num_hidden_layers=s["nL"], max_seq_length=s["L"])
    g = torch.Generator().manual_seed(0)
    table = torch.randn(s["V"] + 1, s["H"], generator=g)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(table.to(DEV))
    return X.Trainer(mod)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--dir", default=None, help="where the file is written (default: a temporary directory)")
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}", flush=True)
    print("| model | parameters | file | save_checkpoint ms | load_checkpoint ms | step ms (batch) | save / step |")
    print("|---|---|---|---|---|---|---|")
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for name, s in SHAPES.items():
            tr, tr2 = trainer(s), trainer(s)
            g = torch.Generator().manual_seed(1)
            batch = {k: torch.randint(1, s["V"] + 1, (s["B"], s["L"]), generator=g).to(DEV)
                     for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")}
            side = torch.cuda.Stream()
            step_ms = []
            with torch.cuda.stream(side):
                for i in range(5 + a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.fit_step(batch)
                    torch.cuda.synchronize()
                    if i >= 5:
                        step_ms.append((time.perf_counter() - t0) * 1e3)
                path = pathlib.Path(d) / "last.ckpt"
                save_ms, load_ms, size = [], [], 0
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    size = tr.save_checkpoint(path)
                    save_ms.append((time.perf_counter() - t0) * 1e3)
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr2.load_checkpoint(path)
                    torch.cuda.synchronize()
                    load_ms.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(tr2.module.model.flat, tr.module.model.flat)
            med = statistics.median
            print(f"| {name} | {tr.module.model.flat.numel():,} | {size / 2**20:.2f} MiB | {med(save_ms):.2f} "
                  f"({min(save_ms):.2f} - {max(save_ms):.2f}) | {med(load_ms):.2f} ({min(load_ms):.2f} - {max(load_ms):.2f}) | "
                  f"{med(step_ms):.3f} (B {s['B']}) | {med(save_ms) / med(step_ms):.1f} |", flush=True)
    print(f"\n(medians of {a.reps} calls, the range in brackets; the step: median of {a.steps} synchronised eager steps on one "
          "resident batch, in-batch negatives)")


if __name__ == "__main__":
    main()
