"""CPU, gloo: a sharded memory (streamchat_amd/sharded.py) saved after two updates by one set of processes and loaded by ANOTHER set goes on
exactly like the memory that was never interrupted: tree texts, Ref pieces, frame numbers and the rows a fetch delivers after a third
update are equal.  Every rank writes and reads only the rows of its own store (`<path>.rank<r>.safetensors`), rank 0 the manifest.
Built on the helpers of tests/test_sharded_gloo.py (streams, oracle-backed providers, ranks as spawned processes)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_sharded_gloo import MEM, QUESTION, SEGMENTS, EmbModel, EmbTok, Summarizer, Tok, _describe, _free_port, _patch_providers, _segment

UPDATES = SEGMENTS[:3]                     # 26 frames (7 chunks: a merge, k-means centroids in one rank's store), 3 frames, 13 frames


def _pieces(nodes):
    return [(list(n.centroids.pieces), _pieces(n.children)) for n in nodes]


def _update(mem, ctx, seg, rng):
    n = UPDATES[seg]
    a, b = mem.partition(n)[ctx.rank]
    return mem.update(_segment(seg, n)[a:b].contiguous(), n, Summarizer(), Tok(), rng=rng)


def _finish(mem, ctx, tree, short):
    """what is compared: the tree after the last update, and a fetch of the short memory and of the retrieved nodes"""
    from streamchat_amd import utiles as U
    wanted, texts = None, None
    if ctx.is_root:
        path, texts = U.fast_search_tree_multi_modal_with_embedding(tree, QUESTION, torch.zeros(1), EmbModel(), EmbTok(), cache=U.CaptionEmbeddingCache())
        wanted = list(short) + list(path)
    wanted = mem.broadcast_refs(wanted)
    rows = mem.fetch(wanted, dst=0, mode="allgather")
    one = mem.fetch([wanted[-1]], dst=0, mode="p2p")                       # one retrieved node on its own
    merged = [mem.fetch([nd.centroids], dst=0, mode="p2p") for nd in tree if nd.depth > 0]
    arr = lambda t: None if t is None else t.numpy().copy()
    return dict(tree=_describe(tree), pieces=_pieces(tree), short=[list(r.pieces) for r in short], frames=[mem.frames_of(r) for r in wanted],
                texts=texts, rows=arr(rows), one=arr(one), merged=[arr(t) for t in merged], seg_parts=mem.seg_parts, next_node=mem.next_node,
                store={k: tuple(v.shape) for k, v in sorted(mem.store.items())})


def _worker(rank, world, port, q, phase, path):
    try:
        import random
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        from streamchat_amd import dist as D, persistence as P, sharded as SH
        _patch_providers()
        ctx = D.init_from_env("cpu")
        mem = SH.ShardedMemory(ctx, **MEM)
        torch.manual_seed(7); random.seed(5)
        rng = np.random.RandomState(11)
        out = None
        if phase in ("full", "first"):
            for seg in range(2):
                tree, short = _update(mem, ctx, seg, rng)
            if phase == "first":
                mem.save(path, short, extra=dict(host_state=P.capture_host_state({"sampler": rng}), updates=2))
                out = dict(files=sorted(os.listdir(os.path.dirname(path))), store={k: tuple(v.shape) for k, v in sorted(mem.store.items())})
        else:
            torch.manual_seed(1234); random.seed(4321)                     # NOT the session's seeds: its state comes from the file
            rng = np.random.RandomState(99)
            tree, short, extra = mem.load(path)
            P.restore_host_state(extra["host_state"], {"sampler": rng})
            assert extra["updates"] == 2 and mem.tree is tree
        if phase != "first":
            tree, short = _update(mem, ctx, 2, rng)
            out = _finish(mem, ctx, tree, short)
            out["probe"] = (random.random(), float(torch.rand(1)), float(rng.rand()))
        q.put((rank, True, "", out))
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, False, traceback.format_exc(), None))
        raise


def _run(world, phase, path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q, phase, path)) for r in range(world)]
    [p.start() for p in ps]
    res = sorted((q.get(timeout=300) for _ in ps), key=lambda r: r[0])
    [p.join(timeout=60) for p in ps]
    for rank, ok, why, _ in res:
        assert ok, f"{phase}, world {world} rank {rank}: {why}"
    return [r[3] for r in res]


def _equal(a, b, where=""):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert a is not None and b is not None and a.dtype == b.dtype and np.array_equal(a, b), where
    elif isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            _equal(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{where}[{i}]")
    else:
        assert a == b, f"{where}: {a!r} != {b!r}"


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [2, 1])
def test_saved_and_loaded_sharded_memory_goes_on_like_the_uninterrupted_one(tmp_path, world):
    path = str(tmp_path / "ck" / "session")
    full = _run(world, "full", path)
    first = _run(world, "first", path)
    assert first[0]["files"] == sorted(["session.json"] + [f"session.rank{r}.safetensors" for r in range(world)])
    resumed = _run(world, "resumed", path)                                  # new processes
    for rank in range(world):
        _equal(resumed[rank], full[rank], f"rank {rank}")
    root = full[0]
    assert root["rows"] is not None and root["one"] is not None and len(root["merged"]) > 0 and root["texts"]
    assert any(k[0] == 1 for r in full for k in r["store"]), "no merge centroids in any store: the scenario does not cover them"
    # rows did not cross ranks: each rank's file holds exactly the tensors of its own store, with their shapes
    from safetensors import safe_open
    for rank in range(world):
        with safe_open(f"{path}.rank{rank}.safetensors", framework="pt") as f:
            on_disk = {tuple(int(x) for x in k.split(".")): tuple(f.get_slice(k).get_shape()) for k in f.keys()}
        assert on_disk == first[rank]["store"], (rank, on_disk, first[rank]["store"])


@pytest.mark.timeout(600)
def test_load_needs_the_world_size_and_settings_of_the_save(tmp_path):
    from streamchat_amd import dist as D, sharded as SH
    import streamchat_amd.ops as ops
    import streamchat_amd.utiles as U
    path = str(tmp_path / "session")
    _run(2, "first", path)
    with pytest.raises(ValueError, match="saved by 2 ranks.*has 1"):
        SH.ShardedMemory(D.DistContext(0, 1, "cpu"), **MEM).load(path)
    saved = (U.weighted_kmeans_feature, ops.sim_topk, ops.kmeans_fit_cols)
    try:
        _patch_providers()
        mem = SH.ShardedMemory(D.DistContext(0, 1, "cpu"), **MEM)
        tree, short = mem.update(_segment(0, 26), 26, Summarizer(), Tok(), rng=np.random.RandomState(0))
        mem.save(str(tmp_path / "one"), short)
        with pytest.raises(ValueError, match="chunk_size"):
            SH.ShardedMemory(D.DistContext(0, 1, "cpu"), **dict(MEM, chunk_size=8)).load(str(tmp_path / "one"))
        back = SH.ShardedMemory(D.DistContext(0, 1, "cpu"), **MEM)
        tree2, short2, _ = back.load(str(tmp_path / "one"))
        assert _pieces(tree2) == _pieces(tree) and short2 == list(short) and back.seg_parts == mem.seg_parts
        assert torch.equal(back.fetch([n.centroids for n in tree2]), mem.fetch([n.centroids for n in tree]))
        # a sharded tree handed to the single-stream saver is refused, not written without its rows
        from streamchat_amd import persistence as P
        with pytest.raises((TypeError, ValueError), match="Ref"):
            P.save_memory_tree(tree, str(tmp_path / "flat"))
        P.save_memory_tree(tree, str(tmp_path / "flat"), materialize=lambda ref: mem.fetch([ref]))
        flat, _, _ = P.load_memory_tree(str(tmp_path / "flat"), device="cpu")
        assert all(torch.equal(a.centroids, mem.fetch([b.centroids])) for a, b in zip(flat, tree))
    finally:
        U.weighted_kmeans_feature, ops.sim_topk, ops.kmeans_fit_cols = saved
