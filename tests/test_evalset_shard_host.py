"""Host side of sharded validation (no GPU): ``shard_eval_plan`` against ``plan_eval_rows`` of the shard's rows alone, the
gather-and-reorder index in a numpy simulation, the real exchange helper on CPU tensors over gloo, and the ``Trainer``'s
check that a validation set's world is its own."""

import os
import pathlib
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = pathlib.Path(__file__).resolve().parents[1]
L = 8
WORLDS = (1, 2, 3, 8)


def _n_globals(W):
    return sorted({n for n in (1, W - 1, W, W + 1, 37) if n >= 1})


def _rows(n_kept, seed):
    """``n_kept`` rows that count -- ragged histories of 1 .. 3L items from a small range (repeats; some longer than
    L), 1-3 targets -- with rows that do not count in between: an empty history, or no positive target."""
    rng = np.random.default_rng(seed)
    hists, tgts = [], []
    for i in range(n_kept):
        if i % 4 == 1:
            hists.append([])
            tgts.append([3])
        if i % 5 == 2:
            hists.append(rng.integers(1, 12, 4).tolist())
            tgts.append([])
        n = (1, L - 1, L, L + 1, 3 * L)[i % 5] if i < 5 else int(rng.integers(1, 3 * L + 1))
        hists.append(rng.integers(1, 12, n).tolist())
        tgts.append(rng.integers(1, 12, int(rng.integers(1, 4))).tolist())
    return hists, tgts


def _same_plan_body(a, b):
    for name in ("lengths", "hist", "row_pos", "tok_offsets", "excl", "excl_offsets"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), name
    assert len(a.chunks) == len(b.chunks)
    for ca, cb in zip(a.chunks, b.chunks):
        assert (ca.row0, ca.row1, ca.tok0, ca.tok1, ca.packed_rows, ca.max_len) == \
            (cb.row0, cb.row1, cb.tok0, cb.tok1, cb.packed_rows, cb.max_len)
        assert ca.seq_offsets.dtype == cb.seq_offsets.dtype == np.int32 and ca.seq_offsets.tolist() == cb.seq_offsets.tolist()
    assert (a.max_seq_length, a.batch_size) == (b.max_seq_length, b.batch_size)


# ---------------------------------------------------------------------------------------------------- shard invariants
@pytest.mark.parametrize("bs", [3, 64])
@pytest.mark.parametrize("W", WORLDS)
def test_shards_partition_the_global_plan_and_equal_plans_of_their_rows(W, bs):
    from xfmr_rec_amd.evalset import plan_eval_rows, shard_eval_plan

    for n_global in _n_globals(W):
        hists, tgts = _rows(n_global, seed=100 * W + n_global)
        glob = plan_eval_rows(hists, tgts, L, bs)
        assert glob.kept.size == n_global == glob.n_global
        assert n_global < 3 or n_global < len(hists)  # (some input rows were dropped)
        assert glob.world_size == 1 and glob.rank == 0 and glob.global_rows.tolist() == list(range(n_global))
        assert glob.target_pos.tolist() == list(range(glob.targets.size))
        if n_global >= 5:
            assert glob.lengths.max() == L and any(len(hists[i]) > L for i in glob.kept)  # (truncation happened)
        seen = []
        for r in range(W):
            sh = shard_eval_plan(glob, r, W)
            if W == 1:
                assert sh is glob  # the identity
                assert plan_eval_rows(hists, tgts, L, bs, rank=0, world_size=1).hist.tolist() == glob.hist.tolist()
                seen += sh.global_rows.tolist()
                continue
            want_rows = list(range(r, n_global, W))
            assert sh.global_rows.dtype == np.int64 and sh.global_rows.tolist() == want_rows
            assert (sh.rank, sh.world_size, sh.n_global) == (r, W, n_global)
            assert sh.kept.dtype == np.int64 and sh.kept.tolist() == glob.kept[want_rows].tolist()
            seen += want_rows
            # the plan of just those rows, in that order
            src = sh.kept.tolist()
            alone = plan_eval_rows([hists[i] for i in src], [tgts[i] for i in src], L, bs)
            assert alone.kept.tolist() == list(range(len(src)))  # (their order is the length order already)
            _same_plan_body(sh, alone)
            # the global targets CSR rides along; the shard's own CSR is the plan's of its rows alone
            assert sh.targets is glob.targets and sh.target_offsets is glob.target_offsets
            tg, off = sh.local_targets()
            assert tg.dtype == np.int64 and off.dtype == np.int64
            assert tg.tolist() == alone.targets.tolist() and off.tolist() == alone.target_offsets.tolist()
            assert sh.target_pos.dtype == np.int64 and glob.targets[sh.target_pos].tolist() == tg.tolist()
            for j, g in enumerate(want_rows):
                assert sh.target_pos[off[j] : off[j + 1]].tolist() == list(range(glob.target_offsets[g], glob.target_offsets[g + 1]))
            # plan_eval_rows' keywords are the same shard
            kw = plan_eval_rows(hists, tgts, L, bs, rank=r, world_size=W)
            _same_plan_body(kw, sh)
            assert kw.global_rows.tolist() == want_rows and kw.target_pos.tolist() == sh.target_pos.tolist()
            if r >= n_global:  # an empty shard is well-formed
                assert sh.kept.size == 0 and sh.chunks == [] and sh.hist.size == 0 and sh.row_pos.size == 0
                assert sh.tok_offsets.tolist() == [0] and sh.excl_offsets.tolist() == [0] and sh.excl.size == 0
                assert tg.size == 0 and off.tolist() == [0] and sh.target_pos.size == 0
                assert sh.hist.dtype == np.int64 and sh.row_pos.dtype == np.int32
        assert sorted(seen) == list(range(n_global)) and len(seen) == n_global  # a partition
        if W > 1 and n_global < W:
            assert shard_eval_plan(glob, W - 1, W).kept.size == 0


def test_shard_eval_plan_refusals():
    from xfmr_rec_amd.evalset import plan_eval_rows, shard_eval_plan

    glob = plan_eval_rows(*_rows(5, seed=1), L, 2)
    for rank, W in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="world_size"):
            shard_eval_plan(glob, rank, W)
    with pytest.raises(ValueError, match="shard"):
        shard_eval_plan(shard_eval_plan(glob, 0, 2), 0, 2)  # only the global plan is sharded
    nothing = plan_eval_rows([[], [1]], [[2], []], L, 4, rank=1, world_size=2)  # no row counts at all
    assert nothing.n_global == 0 and nothing.kept.size == 0 and nothing.chunks == []


# ---------------------------------------------------------------------------------------------------- gather and reorder
def _simulate(owned, payload_of):
    """What gather_rows does, in numpy: pad every rank's local block to the longest, concatenate in rank order, index."""
    from xfmr_rec_amd.evalset import gather_index

    counts, index = gather_index(owned)
    assert counts == [len(o) for o in owned] and index.dtype == np.int64
    pad = max(counts)
    blocks = []
    for o in owned:
        local = payload_of(np.asarray(o, dtype=np.int64))
        block = np.full((pad,) + local.shape[1:], -1, dtype=np.int64)
        block[: local.shape[0]] = local
        blocks.append(block)
    return np.concatenate(blocks)[index]


@pytest.mark.parametrize("W", WORLDS)
def test_gather_index_puts_rows_and_targets_in_global_order(W):
    from xfmr_rec_amd.evalset import plan_eval_rows, shard_eval_plan

    for n_global in _n_globals(W):  # uneven shards (n % W != 0) and empty ones (n < W) included
        glob = plan_eval_rows(*_rows(n_global, seed=7 * W + n_global), L, 4)
        shards = [shard_eval_plan(glob, r, W) for r in range(W)]
        # rows: every row carries its global index (two columns, as a (n_local, k) list would)
        got = _simulate([s.global_rows for s in shards], lambda o: np.stack([o, 10 * o], axis=1))
        assert got.shape == (n_global, 2)
        assert got[:, 0].tolist() == list(range(n_global)) and got[:, 1].tolist() == [10 * i for i in range(n_global)]
        # the ragged per-target case: every target carries its position in the global flat array
        got = _simulate([s.target_pos for s in shards], lambda o: o)
        assert got.tolist() == list(range(glob.targets.size))
        if n_global % W or n_global < W:
            assert len({s.kept.size for s in shards}) > 1  # (the shards really were uneven)


def test_gather_index_refuses_what_is_no_partition():
    from xfmr_rec_amd.evalset import gather_index

    with pytest.raises(ValueError):
        gather_index([[0, 1], [1]])  # position 2 is nobody's
    with pytest.raises(ValueError):
        gather_index([[0, 3], [1]])  # out of range
    counts, index = gather_index([[0, 2], [1]])
    assert counts == [2, 1] and index.tolist() == [0, 2, 1]


# ---------------------------------------------------------------------------------------------------- the helper over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "transformer-recommenders_amd"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from xfmr_rec_amd import distributed as D
    from xfmr_rec_amd.evalset import gather_index, gather_rows, shard_rows_of

    r, _local, w = D.init_process_group_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    out = {}
    # n = 3 over two ranks: a 2 / 1 split; n = 1: rank 1's shard is empty
    for n in (3, 1):
        owned = [shard_rows_of(n, q, world) for q in range(world)]
        counts, index = gather_index(owned)
        mine = torch.from_numpy(owned[rank])
        lists = torch.stack([mine, mine + 100, mine + 200], dim=1)  # (n_local, 3) int64: each row names its global place
        out[f"rows{n}"] = gather_rows(lists, counts, torch.from_numpy(index))
    # the ragged case: rows 0, 1, 2 have 2, 1 and 3 targets (5 on rank 0, 1 on rank 1); the int32 payload is the
    # target's global position
    toff = np.asarray([0, 2, 3, 6])
    pos = [np.concatenate([np.arange(toff[g], toff[g + 1]) for g in shard_rows_of(3, q, world)]) for q in range(world)]
    counts, index = gather_index(pos)
    assert counts == [5, 1]
    out["ranks"] = gather_rows(torch.from_numpy(pos[rank]).to(torch.int32), counts, torch.from_numpy(index))
    try:
        gather_rows(torch.zeros((5, 3), dtype=torch.int64), [2, 1], torch.arange(3))  # (refused before any collective)
        out["refused"] = False
    except ValueError:
        out["refused"] = True
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_gather_rows_over_gloo_gives_both_ranks_the_global_tensor(tmp_path):
    world = 2
    mp.start_processes(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=True) for i in range(world)]
    for n in (3, 1):
        want = torch.stack([torch.arange(n), torch.arange(n) + 100, torch.arange(n) + 200], dim=1)
        for i in range(world):
            assert r[i][f"rows{n}"].dtype == torch.int64 and torch.equal(r[i][f"rows{n}"], want), (n, i)
    for i in range(world):
        assert r[i]["ranks"].dtype == torch.int32 and r[i]["ranks"].tolist() == list(range(6))
        assert r[i]["refused"]


# ---------------------------------------------------------------------------------------------------- Trainer arguments
def _trainer(**kw):
    import xfmr_rec_amd as X

    try:
        conf = X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                                 max_seq_length=8)
        return X.Trainer(X.RecommenderLightningModule(conf), **kw)
    except Exception as e:  # noqa: BLE001 - no device to build the model on
        pytest.skip(f"constructing a Trainer needs a device here: {e}")


def test_trainer_refuses_a_validation_set_of_another_world():
    def setlike(world_size, rank):  # (never evaluated: the check comes first)
        return types.SimpleNamespace(world_size=world_size, rank=rank)

    two = _trainer(world_size=2)  # (no process group here: this process is rank 0)
    for val in (setlike(1, 0), setlike(3, 0), setlike(2, 1), setlike(2, None)):
        with pytest.raises(ValueError, match="world_size"):
            two.fit([], val=val)
        with pytest.raises(ValueError, match="world_size"):
            two.validate(val)
    one = _trainer()
    for val in (setlike(2, 0), setlike(2, 1)):  # a sharded set in a single-process run
        with pytest.raises(ValueError, match="world_size"):
            one.fit([], val=val)
        with pytest.raises(ValueError, match="world_size"):
            one.validate(val)
