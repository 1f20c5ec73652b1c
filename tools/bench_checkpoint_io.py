#!/usr/bin/env python3
"""Wall time of a session checkpoint (`persistence.save_checkpoint`) and of the resume load (`load_checkpoint`, tensors straight to the
device) for a memory tree of a given size - by default the tree of a full C3 session: 1024 frames of 576 x 3584 fp16 rows in chunks of 40
(26 leaves, the first 10 merged under a parent of 5 centroid rows), 5 short-memory frames.  Host I/O only: the rows are random, the texts
synthetic.  Prints one JSON line; `--out FILE` also writes it there.

    python tools/bench_checkpoint_io.py [--frames 1024] [--dir DIR] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from streamchat_amd import persistence as P, synthetic, utiles as U
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--tokens", type=int, default=576)
    ap.add_argument("--width", type=int, default=3584)
    ap.add_argument("--chunk_size", type=int, default=40)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--num_clusters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the checkpoint is written (default: a temporary directory, removed afterwards)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device(a.device)
    bank = torch.randn((a.frames, a.tokens, a.width), dtype=torch.float16, device=dev)
    leaves = [U.MultimodalTreeNode(bank[s:s + a.chunk_size], synthetic.caption(i, words=100), depth=0) for i, s in enumerate(range(0, a.frames, a.chunk_size))]
    tree = leaves
    if len(leaves) >= a.interval:
        parent = U.MultimodalTreeNode(torch.randn((a.num_clusters, a.tokens, a.width), dtype=torch.float16, device=dev), synthetic.caption(999, words=200), depth=1)
        parent.children = leaves[:a.interval]
        tree = [parent] + leaves[a.interval:]
    short = [bank[i:i + 1] for i in range(a.frames - 5, a.frames)]
    settings = dict(chunk_size=a.chunk_size, num_clusters=a.num_clusters, interval=a.interval, short_window=20, remember_window=5, tau=5,
                    compress_rate=1, sample_rate=0.5)
    fp = P.settings_fingerprint(settings, (a.tokens, a.width), torch.float16)
    gens = {"answers": torch.Generator().manual_seed(1), "captions": torch.Generator().manual_seed(2)}
    d = a.dir or tempfile.mkdtemp(prefix="sc_ckpt_")
    os.makedirs(d, exist_ok=True)
    sync = (lambda: torch.cuda.synchronize(dev)) if dev.type == "cuda" else (lambda: None)
    sync()
    t_save, t_load, t_d2h = [], [], []
    try:
        for _ in range(a.reps):
            t0 = time.perf_counter()
            host = [P._host_copy(n.centroids) for n in leaves] + [P._host_copy(tree[0].centroids)]       # the device-to-host share of a save, on its own
            t_d2h.append(time.perf_counter() - t0)
            del host
            t0 = time.perf_counter()
            P.save_checkpoint(d, 0, tree, short, next_segment=1, segments=1, frames_consumed=[0, a.frames], answers=1, turns=1,
                              host_state=P.capture_host_state(gens), fingerprint=fp, extra=dict(time=60, question="q"))
            os.sync()
            t_save.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            nodes, sh, _, info = P.load_checkpoint(P.find_checkpoint(d), fp, device=dev)
            sync()
            t_load.append(time.perf_counter() - t0)
            assert torch.equal(nodes[-1].centroids, tree[-1].centroids) and torch.equal(sh[0], short[0])
            del nodes, sh
        size = os.path.getsize(os.path.join(d, "video_0.safetensors"))
        man = os.path.getsize(os.path.join(d, "video_0.json"))
        fs = next((ln.split()[2] for ln in reversed(open("/proc/mounts").read().splitlines())
                   if os.path.realpath(d).startswith(ln.split()[1].rstrip("/") + "/")), "?")
    finally:
        if a.dir is None:
            shutil.rmtree(d, ignore_errors=True)
    med = statistics.median
    rec = dict(what="session checkpoint I/O", frames=a.frames, row_bytes=a.tokens * a.width * 2, nodes=len(leaves) + (1 if tree is not leaves else 0),
               tensor_file_bytes=size, manifest_bytes=man, filesystem=fs, reps=a.reps,
               save_s=round(med(t_save), 3), save_all_s=[round(t, 3) for t in t_save], save_GBps=round(size / med(t_save) / 1e9, 2),
               d2h_share_s=round(med(t_d2h), 3),
               load_s=round(med(t_load), 3), load_all_s=[round(t, 3) for t in t_load], load_GBps=round(size / med(t_load) / 1e9, 2))
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
