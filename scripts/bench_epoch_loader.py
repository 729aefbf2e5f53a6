#!/usr/bin/env python3
"""The epoch loop's sampler and loader, measured (results: profiles/epoch_loader.md).

(a) kernel against kernel: xfmr_seq_sample against xfmr_seq_sample_rows on the same rows of MovieLens-1M-shaped synthetic
    histories, same process, HIP events around --iters launches each, workspace bytes beside each row.
(b) loop against step: sequences/s of Trainer.fit(loader, max_epochs=1) over --steps steps, beside the same trainer
    stepping ONE resident batch as many times, with the loader's prefetch on and off.

    python scripts/bench_epoch_loader.py [--part a|b|ab] [--iters 200] [--steps 200]
"""
import argparse
import ctypes
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "transformer-recommenders_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"


def histories(users, items, rng):
    lens = np.clip(np.round(np.exp(rng.normal(4.6, 1.0, users))), 20, 2314).astype(int)  # ML-1M-like: mean ~ 165
    hs = [rng.integers(1, items + 1, n) for n in lens]
    ls = [np.concatenate([rng.random(n - 1) < 0.58, [True]]) for n in lens]
    return hs, ls


def dataset(items, seq_len, min_rows=0, users=6040, seed=0):
    from xfmr_rec_amd.data import DeviceSeqDataset, SeqDataConfig

    hs, ls = histories(users, items, np.random.default_rng(seed))
    k = max(1, -(-min_rows // users))  # the same users again, as further rows (every row has its own random stream)
    return DeviceSeqDataset(SeqDataConfig(max_seq_length=seq_len, pos_lookahead=0), hs * k, ls * k, items)


def _event(lib):
    from xfmr_rec_amd import _native as N

    e = ctypes.c_void_p()
    N.check(lib.xfmr_event_create(ctypes.byref(e), 1), "xfmr_event_create")
    return e.value


def _timed(lib, launch, iters):
    """Mean microseconds per launch: HIP events around `iters` back-to-back launches (5 untimed ones in front)."""
    from xfmr_rec_amd import _native as N

    e0, e1 = _event(lib), _event(lib)
    for i in range(5):
        launch(i)
    torch.cuda.synchronize()
    N.check(lib.xfmr_event_record(e0, N.stream()), "xfmr_event_record")
    for i in range(iters):
        launch(5 + i)
    N.check(lib.xfmr_event_record(e1, N.stream()), "xfmr_event_record")
    torch.cuda.synchronize()
    ms = ctypes.c_float()
    N.check(lib.xfmr_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "xfmr_event_elapsed_ms")
    for e in (e0, e1):
        lib.xfmr_event_destroy(e)
    return ms.value / iters * 1e3


def part_a(iters):
    from xfmr_rec_amd import _native as N

    lib = N.load()
    print("| shape | mean history | xfmr_seq_sample us | workspace | xfmr_seq_sample_rows us | workspace | rows / old |")
    print("|---|---|---|---|---|---|---|")
    for B, L, V in ((512, 200, 3883), (32, 32, 3883), (512, 200, 1_000_000)):
        ds = dataset(V, L)
        rng = np.random.default_rng(1)
        order = torch.from_numpy(rng.permutation(len(ds))[: B * 8].astype(np.int64)).to(DEV)  # 8 batches, taken in turn
        max_hist = int(ds.lengths.max())
        out = [torch.empty((B, L), dtype=torch.int64, device=DEV) for _ in range(3)]
        ln = torch.empty(B, dtype=torch.int32, device=DEV)
        ws_old = lib.xfmr_seq_sample_workspace(B, V)
        ws_new = lib.xfmr_seq_sample_rows_workspace(B, L)
        ws = torch.empty(max(ws_old, ws_new, 1), dtype=torch.uint8, device=DEV)
        base = (N.ptr(ds.items), N.ptr(ds.labels), N.ptr(ds.offsets))
        outs = (N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]))

        def old(i):
            rows = order[(i % 8) * B : (i % 8 + 1) * B]
            N.check(lib.xfmr_seq_sample(*base, N.ptr(rows), B, L, L, 0, V, max_hist, i, *outs, N.ptr(ws), ws_old,
                                        N.stream()), "xfmr_seq_sample")

        def new(i):
            N.check(lib.xfmr_seq_sample_rows(*base, len(ds), N.ptr(order), len(order), (i % 8) * B, B, L, L, 0, V, max_hist,
                                             7, i, *outs, N.ptr(ln), N.ptr(ws), ws_new, N.stream()), "xfmr_seq_sample_rows")

        t_old = [_timed(lib, old, iters) for _ in range(3)]
        t_new = [_timed(lib, new, iters) for _ in range(3)]
        mean = float(ds.lengths.mean())
        print(f"| B {B} x L {L}, V {V:,} | {mean:.0f} | {min(t_old):.1f} ({max(t_old):.1f}) | {ws_old:,} B | "
              f"{min(t_new):.1f} ({max(t_new):.1f}) | {ws_new:,} B | {min(t_new) / min(t_old):.3f} |", flush=True)
    print("\n(us per launch: best of three runs of --iters launches, the worst in brackets)")


def part_b(steps):
    import xfmr_rec_amd as X
    from xfmr_rec_amd.data import SEQ_BATCH_KEYS, DeviceSeqLoader

    shapes = {
        "config 2, B 512": dict(H=128, A=4, I=512, nL=4, L=200, B=512, V=3883, graph="off"),
        "reference default": dict(H=384, A=12, I=48, nL=1, L=32, B=32, V=3883, graph="on"),
    }
    print("| shape | graph | fit(loader), prefetch on | fit(loader), prefetch off | one resident batch | steps |")
    print("|---|---|---|---|---|---|")
    for name, s in shapes.items():
        ds = dataset(s["V"], s["L"], min_rows=steps * s["B"])
        conf = X.LightningConfig(hidden_size=s["H"], num_attention_heads=s["A"], intermediate_size=s["I"],
                                 num_hidden_layers=s["nL"], max_seq_length=s["L"])
        g = torch.Generator().manual_seed(0)
        table = torch.randn(s["V"] + 1, s["H"], generator=g)
        table = table / table.norm(dim=-1, keepdim=True)
        table[0] = 0
        mod = X.RecommenderLightningModule(conf)
        mod.configure_model()
        mod.model.set_table(table.to(DEV))
        tr = X.Trainer(mod)
        loaders = {p: DeviceSeqLoader(ds, s["B"], seed=1, drop_last=True, prefetch=p) for p in (True, False)}

        def run(batches, **kw):
            if kw:
                batches.set_epoch(0)  # (a loader stopped by max_steps would go on from where it stopped)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tr.fit(batches, max_steps=steps, graph=s["graph"], **kw)
            torch.cuda.synchronize()
            return len(out) * s["B"] / (time.perf_counter() - t0), len(out)

        run(loaders[True], max_epochs=1)  # spin-up: clocks, allocator pools, lazily made objects
        rates = {}
        for rep in range(2):
            for p, ld in loaders.items():
                rates.setdefault(p, []).append(run(ld, max_epochs=1))
            ld = loaders[False]
            ld.set_epoch(0)
            ld.fixed_width = s["graph"] != "off"
            one = next(iter(ld))
            one = {k: v.clone() if torch.is_tensor(v) else v for k, v in one.items()}
            if s["graph"] != "off":
                one = {k: one[k] for k in SEQ_BATCH_KEYS}
            ld.fixed_width = False
            ld.set_epoch(0)
            rates.setdefault("one", []).append(run([one] * steps))
        fmt = lambda rs: " / ".join(f"{r:,.0f}" for r, _ in rs)  # noqa: E731
        print(f"| {name} | {s['graph']} | {fmt(rates[True])} | {fmt(rates[False])} | {fmt(rates['one'])} | "
              f"{rates[True][0][1]} |", flush=True)
        for ld in loaders.values():
            ld.close()
    print("\n(sequences/s by a host clock around the whole fit call, its capture and warm-up steps included; two runs each)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if "a" in a.part:
        part_a(a.iters)
    if "b" in a.part:
        part_b(a.steps)


if __name__ == "__main__":
    main()
