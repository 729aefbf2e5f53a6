"""Sharded validation with two ranks: each rank's pass over its own rows against the single-process set's rows, the one
exchange per pass giving both ranks the single-process sums bit for bit, an empty shard, and ``Trainer.fit`` under two
ranks -- the same history, the same decisions, the same step count on both, the best model written by rank 0 only.

As in ``tests/test_gpu_ddp.py`` only one GPU is at hand, so both ranks run on device 0 and the collectives go over gloo
(XFMR_REHEARSE_ONE_GPU=1): everything of the W > 1 path except RCCL's transport."""

import os
import pathlib
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = pathlib.Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu
H, A, I, L, V, K = 64, 2, 128, 24, 60, 20
CUTS = (1, 5, 20)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(worker, *args, world=2, limit=180.0):
    """The workers, joined with a time limit; whatever still lives afterwards is killed (no GPU holder stays behind)."""
    ctx = mp.start_processes(worker, args=(world, _free_port()) + args, nprocs=world, join=False, start_method="spawn")
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5.0):  # (raises what a worker raised)
            if time.monotonic() > deadline:
                raise TimeoutError(f"the workers did not finish within {limit} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
        for p in ctx.processes:
            p.join(10.0)


def _rows(n=37, seed=5):
    """37 rows over V items: histories of 1 .. 40 rows (some longer than L = 24), 1-4 positive targets; four rows have no
    positive target and two an empty history, which leaves 31: 16 rows for rank 0 and 15 for rank 1."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(n):
        h = rng.integers(1, V + 1, int(rng.integers(1, 41))).tolist()
        t = rng.integers(1, V + 1, int(rng.integers(1, 5))).tolist()
        lab = [True] + (rng.random(len(t) - 1) < 0.7).tolist()
        if u % 9 == 4:
            lab = [False] * len(t)
        if u in (11, 12):
            h = []
        rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": lab}})
    rows[0]["history"]["item_id"] = rng.integers(1, V + 1, 40).tolist()
    return rows


def _start(rank, world, port):
    for p in (ROOT, ROOT / "transformer-recommenders_amd", ROOT / "tests"):
        sys.path.insert(0, str(p))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), XFMR_REHEARSE_ONE_GPU="1")
    import xfmr_rec_amd as X
    from xfmr_rec_amd import distributed as D

    r, local, w = D.init_process_group_from_env()
    assert (r, local, w) == (rank, 0, world)
    torch.cuda.set_device(0)
    return X


def _module(X, precision, layers, **kw):
    from helpers import unit_table

    conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=I, num_hidden_layers=layers,
                             max_seq_length=L, precision=precision, top_k=K, **kw)
    mod = X.RecommenderLightningModule(conf)
    mod.model = X.RecommenderModel(conf, device="cuda:0", precision=precision, seed=3)  # same seed: replicated weights
    mod.configure_model()
    mod.model.set_table(unit_table(V, H).to("cuda:0"))
    return mod


def _finish(out, out_dir, rank):
    torch.cuda.synchronize()
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _both_passes(X, mod, rows, rank, world, batch_size):
    """Everything a single-process set and this rank's shard of the same rows compute, on the host."""
    full = X.DeviceEvalSet.from_rows(mod, rows, batch_size=batch_size)
    sh = X.DeviceEvalSet.from_rows(mod, rows, batch_size=batch_size, rank=rank, world_size=world)
    assert (sh.rank, sh.world_size, full.rank, full.world_size) == (rank, world, 0, 1)
    assert len(sh) == len(full) == full.n_local == sh.n_global and sh.n_local == len(range(rank, len(full), world))
    assert sh.packed == full.packed == (mod.config.precision == "bf16")
    assert sh.hist.numel() == int(full.plan.lengths[sh.global_rows].sum())  # only the shard's histories were uploaded
    assert torch.equal(sh.targets, full.targets) and torch.equal(sh.target_offsets, full.target_offsets)
    emb_full, emb = full.encode(), sh.encode()
    (idx_full, score_full), (idx, score) = full.recommend(), sh.recommend()
    out = {
        "n_global": len(full), "n_local": sh.n_local, "chunks": (len(full.plan.chunks), len(sh.plan.chunks)),
        "global_rows": torch.from_numpy(sh.global_rows), "target_pos": torch.from_numpy(sh.plan.target_pos),
        "emb_full": emb_full, "emb": emb, "idx_full": idx_full, "idx": idx, "score_full": score_full, "score": score,
        "ranks_full": full.target_ranks(), "ranks": sh.target_ranks(),
        "sums_full": full.evaluate_device(), "sums": sh.evaluate_device(),
        "rank_sums_full": full.evaluate_ranks_device(CUTS), "rank_sums": sh.evaluate_ranks_device(CUTS),
    }
    out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
    out |= {"ev_full": full.evaluate(), "ev": sh.evaluate(), "ev_cut_full": full.evaluate(cutoffs=CUTS),
            "ev_cut": sh.evaluate(cutoffs=CUTS), "ev_test": sh.evaluate("test")}
    return out


def _check_both_passes(r, n_global, k=K):
    """``r``: the two ranks' :func:`_both_passes` results."""
    world = len(r)
    for i in range(world):
        x = r[i]
        g, tp = x["global_rows"], x["target_pos"]
        assert x["n_global"] == n_global and g.tolist() == list(range(i, n_global, world)) and x["n_local"] == g.numel()
        assert x["emb"].shape == (g.numel(), H) and x["idx"].shape == x["score"].shape == (g.numel(), k)
        assert x["idx"].dtype == torch.int64 and x["ranks"].dtype == torch.int32 and x["ranks"].shape == tp.shape
        # the local pass is the single-process pass at the rank's rows (at the targets of those rows)
        assert torch.equal(x["emb"], x["emb_full"][g])
        assert torch.equal(x["idx"], x["idx_full"][g]) and torch.equal(x["score"], x["score_full"][g])
        assert torch.equal(x["ranks"], x["ranks_full"][tp])
        # one exchange, then the single-process sums: bit for bit
        assert x["sums"].dtype == torch.float64 and x["sums"].shape == (8,) and torch.equal(x["sums"], x["sums_full"])
        assert x["rank_sums"].shape == (len(CUTS), 8) and torch.equal(x["rank_sums"], x["rank_sums_full"])
        assert float(x["sums"][7]) == n_global == x["ev"]["val/num_rows"]
        assert x["ev"] == x["ev_full"] and x["ev_cut"] == x["ev_cut_full"]
        assert f"val/retrieval_normalized_dcg@{CUTS[1]}" in x["ev_cut"] and x["ev_test"]["test/num_rows"] == n_global
    # ... and between the ranks
    for key in ("sums", "rank_sums"):
        assert torch.equal(r[0][key], r[1][key])
    for key in ("ev", "ev_cut", "ev_test"):
        assert r[0][key] == r[1][key]
    assert sorted(r[0]["global_rows"].tolist() + r[1]["global_rows"].tolist()) == list(range(n_global))


# ------------------------------------------------------------------------------------------------ 1. pass equality
def _pass_worker(rank, world, port, out_dir, precision, layers):
    X = _start(rank, world, port)
    mod = _module(X, precision, layers)
    mod.train()  # (a pass runs in eval mode and puts the flag back)
    out = _both_passes(X, mod, _rows(), rank, world, batch_size=8)
    assert mod.model.training
    _finish(out, out_dir, rank)


@pytest.mark.parametrize("precision,layers", [("bf16", 2), ("fp32", 1)])
def test_sharded_pass_equals_the_single_process_pass(tmp_path, precision, layers):
    _run(_pass_worker, str(tmp_path), precision, layers)
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=True) for i in range(2)]
    assert r[0]["n_local"] == 16 and r[1]["n_local"] == 15  # an uneven split
    assert r[0]["chunks"] == (4, 2) and r[1]["chunks"] == (4, 2)  # 8 + 8 + 8 + 7 rows against 8 + 8 and 8 + 7
    _check_both_passes(r, 31)
    assert (r[0]["ranks_full"] > 0).all() and len(set(r[0]["ranks_full"].tolist())) > 5  # (the ranks say something)


# ------------------------------------------------------------------------------------------------ 2. an empty shard
def _empty_shard_worker(rank, world, port, out_dir):
    X = _start(rank, world, port)
    mod = _module(X, "bf16", 1)
    rows = [{"history": {"item_id": [7, 3, 9]}, "target": {"item_id": [5, 2], "label": [True, False]}},
            {"history": {"item_id": [4, 4]}, "target": {"item_id": [8], "label": [False]}}]
    out = _both_passes(X, mod, rows, rank, world, batch_size=8)
    # nothing counts at all: the error of the single-process set, on every rank
    try:
        X.DeviceEvalSet.from_rows(mod, rows[1:], rank=rank, world_size=world)
        out["refused"] = False
    except ValueError as e:
        out["refused"] = "no validation row" in str(e)
    _finish(out, out_dir, rank)


def test_an_empty_shard_takes_part_in_the_exchange(tmp_path):
    _run(_empty_shard_worker, str(tmp_path))
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=True) for i in range(2)]
    assert (r[0]["n_local"], r[1]["n_local"]) == (1, 0) and r[1]["chunks"] == (1, 0)
    assert r[1]["emb"].shape == (0, H) and r[1]["idx"].shape == (0, K) and r[1]["ranks"].shape == (0,)
    _check_both_passes(r, 1)
    assert r[0]["refused"] and r[1]["refused"]


# ------------------------------------------------------------------------------------------------ 3. fit under two ranks
MONITOR = {"name": "val/retrieval_normalized_dcg@5", "mode": "max"}


def _fit_worker(rank, world, port, out_dir):
    X = _start(rank, world, port)
    from helpers import ragged_batch
    from xfmr_rec_amd import distributed as D

    rows = _rows()
    batches = []
    for i in range(8):
        b, _ = ragged_batch(8, L, V, seed=10 + i)
        mine = list(D.shard_rows(8, rank, world))
        batches.append({k: v[mine].to("cuda:0") for k, v in b.items()})
    mod = _module(X, "bf16", 2, learning_rate=0.01)
    sh = X.DeviceEvalSet.from_rows(mod, rows, batch_size=8, rank=rank, world_size=world)
    saves = []
    real_save = mod.save

    def counted_save(path):
        saves.append({k: v.detach().cpu().clone() for k, v in mod.model.encoder_state_dict().items()})
        real_save(path)

    def refused_save(path):
        raise AssertionError("only rank 0 writes the best model")

    mod.save = counted_save if rank == 0 else refused_save
    tr = X.Trainer(mod, world_size=world)
    ckpt = os.path.join(out_dir, "ckpt")
    losses = tr.fit(batches, val=sh, val_check_interval=2, early_stopping={"patience": 1, "min_delta": 0},
                    checkpoint_dir=ckpt, val_cutoffs=(5, 20), monitor=MONITOR)
    torch.cuda.synchronize()
    out = {"steps": len(losses), "val_history": tr.val_history, "best_score": tr.best_score, "best_step": tr.best_step,
           "stopped_early": tr.stopped_early, "best_model_path": tr.best_model_path, "flat": mod.model.flat.detach().cpu(),
           "n_saves": len(saves), "last_saved": saves[-1] if saves else None, "logged": float(mod.logged[MONITOR["name"]]),
           "validate": tr.validate(sh), "validate_cut": tr.validate(sh, cutoffs=(5, 20))}
    # a run whose metric cannot move: both ranks stop after the second pass, four batches before the end
    still = _module(X, "bf16", 2, learning_rate=0.0, weight_decay=0.0)
    tr2 = X.Trainer(still, world_size=world)
    sh2 = X.DeviceEvalSet.from_rows(still, rows, batch_size=8, rank=rank, world_size=world)
    n2 = len(tr2.fit(batches, val=sh2, val_check_interval=2, early_stopping={"patience": 1, "min_delta": 0}))
    out["still"] = {"steps": n2, "stopped_early": tr2.stopped_early, "best_step": tr2.best_step,
                    "history_steps": [h["step"] for h in tr2.val_history], "best_model_path": tr2.best_model_path}
    # the world check, where a process group exists: the other rank's shard, and a single-process set
    other = X.DeviceEvalSet.from_rows(still, rows, batch_size=8, rank=1 - rank, world_size=world)
    refusals = 0
    for bad in (other, X.DeviceEvalSet.from_rows(still, rows, batch_size=8)):
        try:
            tr2.validate(bad)
        except ValueError as e:
            refusals += "world_size" in str(e)
    out["refusals"] = refusals
    _finish(out, out_dir, rank)


def test_fit_under_two_ranks_takes_the_same_decisions_on_both(tmp_path):
    import xfmr_rec_amd as X

    _run(_fit_worker, str(tmp_path))
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=True) for i in range(2)]
    a, b = r
    name = MONITOR["name"]
    print(f"steps {a['steps']}, stopped_early {a['stopped_early']}, best {a['best_score']!r} at {a['best_step']}, history "
          f"{[(h['step'], round(h[name], 6)) for h in a['val_history']]}, saves {a['n_saves']}")
    for key in ("steps", "val_history", "best_score", "best_step", "stopped_early", "best_model_path", "logged", "validate",
                "validate_cut", "still", "refusals"):
        assert a[key] == b[key], key
    assert torch.equal(a["flat"], b["flat"])  # the replicas after the last step: bit for bit
    hist = a["val_history"]
    assert [h["step"] for h in hist] == list(range(2, a["steps"] + 1, 2)) and len(hist) >= 2
    assert all(h["val/num_rows"] == 31 and "val/retrieval_recall@20" in h for h in hist)
    assert a["logged"] == hist[-1][name]  # log_dict ran on every rank
    # the loop's rule, replayed on the history: strict improvements move the best; patience 1 stops at the first pass
    # that does not improve
    best, improvements, stop_at = None, [], None
    for h in hist:
        if best is None or h[name] > best:
            best = h[name]
            improvements.append(h["step"])
        elif stop_at is None:
            stop_at = h["step"]
    assert a["best_score"] == best and a["best_step"] == improvements[-1]
    assert a["stopped_early"] == (stop_at is not None) and a["steps"] == (stop_at if stop_at is not None else 8)
    # the best model: written once per improvement, by rank 0 only (rank 1's save raises), set on both ranks, loadable
    assert (a["n_saves"], b["n_saves"]) == (len(improvements), 0)
    assert a["best_model_path"] == str(tmp_path / "ckpt" / "best") and (tmp_path / "ckpt" / "best" / "model.safetensors").exists()
    loaded = X.RecommenderModel.load(a["best_model_path"], device="cuda", precision="bf16")
    state = loaded.encoder_state_dict()
    assert set(state) == set(a["last_saved"])
    for k, v in a["last_saved"].items():  # the weights rank 0 held at the last improvement
        assert torch.equal(state[k].detach().cpu(), v), k
    assert a["validate"]["val/num_rows"] == 31 and name in a["validate_cut"] and name not in a["validate"]
    assert a["still"] == {"steps": 4, "stopped_early": True, "best_step": 2, "history_steps": [2, 4], "best_model_path": None}
    assert a["refusals"] == 2
