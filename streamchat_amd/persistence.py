"""Persistence of the visual memory tree.  The reference only writes the answers JSON (inference_streaming_longva_v2.py:
657-675) and the dialogue `memory_{i}.json` (memory_bank/memory_utils.py:95-110); the tree of `MultimodalTreeNode`s (utiles.py:48-56) lives and
dies with the process.  Here a session's tree is saved as ONE safetensors file (every node's `.centroids`, deduplicated by storage so
a depth-0 node that is a view into the feature bank is written once) plus a JSON manifest (texts, depths, labels, children), and comes
back with identical field values, so a multi-round session can resume without re-encoding or re-captioning the stream.

A SESSION CHECKPOINT is such a pair whose `extra["resume"]` also holds what the next round reads besides the tree: where the session stands
(video, next segment, frames consumed, how many answers / dialogue turns are on disk), the host random state (`capture_host_state`) and a
fingerprint of the settings that shape the tree (`settings_fingerprint`).  `save_checkpoint` / `find_checkpoint` are what the entry
point's `--memory_tree_dir` / `--resume_memory_tree` use.

Writes are atomic: both files go to temporary names and are renamed into place, the manifest last.  The manifest and the tensor file carry
the same `save_id`; the tensor file of the previous save is kept as `<path>.prev.safetensors` until the new manifest is in place, so a
process killed anywhere inside a save leaves the previous checkpoint loadable (`load_memory_tree` picks the tensor file whose id matches)."""
import base64
import json
import os
import random
import re
import uuid

import numpy as np
import torch
from safetensors import safe_open
from safetensors.torch import load_file, save_file

from .utiles import MultimodalTreeNode

FORMAT = "streamchat-memory-tree/1"
FINGERPRINT_FIELDS = ("chunk_size", "num_clusters", "interval", "short_window", "remember_window", "tau", "compress_rate", "sample_rate",
                      "feature_row", "feature_dtype")


class ResumeError(ValueError):
    """a checkpoint that exists but cannot be resumed from (older file without resume data, other settings, other world size)"""


def _host_copy(t):
    """`t` on the host with storage of its own (safetensors refuses aliasing tensors): the device-to-host copy already is one"""
    t = t.detach()
    return t.cpu().contiguous() if t.device.type != "cpu" else t.contiguous().clone()


def _walk(nodes, tensors, seen, materialize=None, where="nodes"):
    out = []
    for i, n in enumerate(nodes):
        c = n.centroids
        key = None
        if c is not None and not torch.is_tensor(c):
            if materialize is None:
                raise TypeError(f"save_memory_tree: {where}[{i}] (depth {n.depth}, text {str(n.text)[:40]!r}) holds {type(c).__name__} centroids, "
                                f"not a tensor; pass `materialize` to turn them into rows (a sharded tree is saved by ShardedMemory.save)")
            c = materialize(c)
            if not torch.is_tensor(c):
                raise TypeError(f"save_memory_tree: `materialize` returned {type(c).__name__} for {where}[{i}], not a tensor")
        if torch.is_tensor(c):
            ident = (c.data_ptr(), tuple(c.shape), tuple(c.stride()), str(c.dtype))
            key = seen.get(ident)
            if key is None:
                key = f"t{len(tensors)}"
                seen[ident] = key
                tensors[key] = _host_copy(c)
        labels = n.labels.detach().cpu().tolist() if torch.is_tensor(n.labels) else n.labels
        out.append(dict(text=n.text, depth=int(n.depth), centroids=key, labels=labels, text_distance=n.text_distance,
                        image_distance=n.image_distance, children=_walk(n.children, tensors, seen, materialize, f"{where}[{i}].children")))
    return out


def _write_json_atomic(obj, path):
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "w", encoding="utf-8") as f:
        json.dump(obj, f, ensure_ascii=False)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def _write_tensors_atomic(tensors, path, metadata, keep_previous=None):
    """`tensors` -> `path` under a temporary name first.  keep_previous: where the file that `path` replaces is parked (its manifest still points at it)."""
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        save_file(tensors, tmp, metadata=metadata)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    if keep_previous is not None and os.path.exists(path):
        os.replace(path, keep_previous)
    os.replace(tmp, path)


def save_memory_tree(nodes, path, short_memory=None, extra=None, materialize=None, extra_tensors=None):
    """nodes: list[MultimodalTreeNode] (the long memory);  short_memory: optional list of [1,P,D] tensors;  extra: JSON-able dict.
    materialize: optional callable for `.centroids` that are not tensors (-> tensor); without it such a node raises TypeError - rows
    are never dropped silently.  extra_tensors: {name: tensor} stored beside the tree's under "x.<name>" (`load_checkpoint` returns them).
    Writes `<path>.safetensors` and `<path>.json` atomically (manifest last); returns the manifest."""
    tensors, seen = {}, {}
    for name, t in (extra_tensors or {}).items():
        tensors["x." + name] = _host_copy(t)
    save_id = uuid.uuid4().hex
    manifest = dict(format=FORMAT, save_id=save_id, nodes=_walk(nodes, tensors, seen, materialize), short=[], extra=extra or {})
    for t in short_memory or []:
        key = f"t{len(tensors)}"
        tensors[key] = _host_copy(t)
        manifest["short"].append(key)
    json.dumps(manifest, ensure_ascii=False)                # an `extra` that cannot be written fails here, before anything on disk changes
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    _settle(path)
    _write_tensors_atomic(tensors, path + ".safetensors", dict(format=FORMAT, save_id=save_id), keep_previous=path + ".prev.safetensors")
    _write_json_atomic(manifest, path + ".json")
    if os.path.exists(path + ".prev.safetensors"):
        os.remove(path + ".prev.safetensors")
    return manifest


def _tensor_file_for(path, manifest):
    """the tensor file the manifest was written with: `<path>.safetensors`, or the parked previous one when a save was cut short"""
    want = manifest.get("save_id")
    cands = [path + ".safetensors", path + ".prev.safetensors"]
    if want is None:                                         # written before save ids existed
        return cands[0]
    for c in cands:
        if os.path.exists(c):
            with safe_open(c, framework="pt") as f:
                if (f.metadata() or {}).get("save_id") == want:
                    return c
    raise ValueError(f"{path}.json: no tensor file with save id {want} beside it (looked at {', '.join(os.path.basename(c) for c in cands)})")


def _settle(path):
    """A parked tensor file means an earlier save was cut short: put the file the manifest belongs to back under its own name before
    the next save parks again (otherwise two cut saves in a row would lose it)."""
    prev = path + ".prev.safetensors"
    if not os.path.exists(prev):
        return
    try:
        with open(path + ".json", encoding="utf-8") as f:
            good = _tensor_file_for(path, json.load(f))
    except (OSError, ValueError):
        good = None
    if good == prev:
        os.replace(prev, path + ".safetensors")
    else:
        os.remove(prev)


def load_memory_tree(path, device="cuda"):
    """Returns (nodes, short_memory, extra).  Tensors are loaded straight to `device`; nodes that shared storage share it again."""
    return _load(path, device)[:3]


def _load(path, device):
    with open(path + ".json", encoding="utf-8") as f:
        manifest = json.load(f)
    if manifest.get("format") != FORMAT:
        raise ValueError(f"{path}.json: unknown memory-tree format {manifest.get('format')!r}")
    tensors = load_file(_tensor_file_for(path, manifest), device=str(device))

    def build(d):
        n = MultimodalTreeNode(tensors[d["centroids"]] if d["centroids"] is not None else None, d["text"], d["text_distance"],
                               d["image_distance"], d["labels"], depth=d["depth"])
        n.children = [build(c) for c in d["children"]]
        return n
    named = {k[2:]: v for k, v in tensors.items() if k.startswith("x.")}
    return [build(d) for d in manifest["nodes"]], [tensors[k] for k in manifest["short"]], manifest["extra"], named


# ------------------------------------------------------------------------------------------------
# what a round reads besides the tree: host random state
# ------------------------------------------------------------------------------------------------
def _b64(t):
    return base64.b64encode(t.numpy().tobytes()).decode("ascii")


def _unb64(s):
    return torch.frombuffer(bytearray(base64.b64decode(s)), dtype=torch.uint8).clone()


def capture_host_state(generators=None, which=("torch", "python", "numpy")):
    """The host random state the updater and the answer path draw from, as a JSON-able dict:
      torch   the global CPU generator (`torch.randperm`: the k-means initial rows, utiles.weighted_kmeans_feature / sharded.update)
      python  the global `random` (`random.randint`: the k-means empty-cluster reseed rows)
      numpy   the global `np.random` (`np.random.choice`: the forgetting-curve sampler, utiles.select_data_without_replacement with rng=None)
      generators: {name: torch.Generator | np.random.RandomState} - the per-role seed generators of the entry point
                  (`model.seed_generator`, `captioner.seed_generator`: llm.draw_seeds) or a caller's own sampler `rng`.
    `which` selects the globals (the entry point captures them before the look-ahead thread may draw, the answer's generator after)."""
    st = {}
    if "torch" in which:
        st["torch"] = _b64(torch.get_rng_state())
    if "python" in which:
        v, words, gauss = random.getstate()
        st["python"] = [v, list(words), gauss]
    if "numpy" in which:
        st["numpy"] = _np_state(np.random.get_state())
    gens = {}
    for name, g in (generators or {}).items():
        if isinstance(g, torch.Generator):
            if g.device.type != "cpu":
                raise TypeError(f"capture_host_state: generator {name!r} lives on {g.device}; only host generators are part of a checkpoint")
            gens[name] = dict(kind="torch", state=_b64(g.get_state()))
        elif isinstance(g, np.random.RandomState):
            gens[name] = dict(kind="numpy", state=_np_state(g.get_state()))
        else:
            raise TypeError(f"capture_host_state: generator {name!r} is a {type(g).__name__}; torch.Generator or np.random.RandomState expected")
    st["generators"] = gens
    return st


def _np_state(s):
    return [s[0], [int(x) for x in s[1]], int(s[2]), int(s[3]), float(s[4])]


def _np_tuple(s):
    return (s[0], np.asarray(s[1], dtype=np.uint32), int(s[2]), int(s[3]), float(s[4]))


def restore_host_state(state, generators=None):
    """Inverse of `capture_host_state`: sets the globals that were captured and every generator of `generators` (by name; a name the
    checkpoint does not hold is an error, so is a saved generator nobody asked for - a role that silently starts from its seed again
    would sample other tokens than the uninterrupted session)."""
    generators = generators or {}
    saved = state.get("generators", {})
    missing, unused = sorted(set(generators) - set(saved)), sorted(set(saved) - set(generators))
    if missing or unused:
        raise ResumeError(f"restore_host_state: generator names do not match the checkpoint (not saved: {missing}, saved but not given: {unused})")
    if "torch" in state:
        torch.set_rng_state(_unb64(state["torch"]))
    if "python" in state:
        v, words, gauss = state["python"]
        random.setstate((v, tuple(words), gauss))
    if "numpy" in state:
        np.random.set_state(_np_tuple(state["numpy"]))
    for name, g in generators.items():
        s = saved[name]
        if s["kind"] == "torch":
            g.set_state(_unb64(s["state"]))
        else:
            g.set_state(_np_tuple(s["state"]))


# ------------------------------------------------------------------------------------------------
# the settings that shape the tree
# ------------------------------------------------------------------------------------------------
def settings_fingerprint(settings, feature_row=None, feature_dtype=None):
    """`settings`: an argparse namespace or a dict with the memory settings.  feature_row: (P, D) of a feature row, feature_dtype: its dtype."""
    get = settings.get if isinstance(settings, dict) else (lambda k, d=None: getattr(settings, k, d))
    fp = {k: get(k) for k in FINGERPRINT_FIELDS[:-2]}
    absent = [k for k, v in fp.items() if v is None]
    if absent:
        raise ValueError(f"settings_fingerprint: no value for {', '.join(absent)}")
    fp["feature_row"] = None if feature_row is None else [int(x) for x in feature_row]
    fp["feature_dtype"] = None if feature_dtype is None else str(feature_dtype)
    return fp


def check_fingerprint(saved, current, where="checkpoint"):
    """A resume with other values than the checkpoint was written with is refused; the message names the first field that differs.
    (`feature_row` / `feature_dtype` are compared when both sides know them.)"""
    for k in FINGERPRINT_FIELDS:
        a, b = saved.get(k), current.get(k)
        if k in ("feature_row", "feature_dtype") and (a is None or b is None):
            continue
        if isinstance(a, (list, tuple)):
            a, b = list(a), (list(b) if isinstance(b, (list, tuple)) else b)
        if a != b:
            raise ResumeError(f"{where}: was written with {k} = {a!r}, this run has {k} = {b!r}; a session resumes only with the settings "
                              f"its memory tree was built with")


def tree_feature_row(nodes, short_memory=None):
    """((P, D), dtype) of the feature rows of a tree / short memory (None, None when there is no tensor)"""
    for t in list(short_memory or []) + [n.centroids for n in nodes or []]:
        if torch.is_tensor(t):
            return tuple(t.shape[1:]), t.dtype
    return None, None


# ------------------------------------------------------------------------------------------------
# session checkpoints: <dir>/video_<n>.{safetensors,json}
# ------------------------------------------------------------------------------------------------
def checkpoint_path(directory, video):
    return os.path.join(directory, f"video_{int(video)}")


def save_checkpoint(directory, video, nodes, short_memory, *, next_segment, segments, frames_consumed, answers, turns, host_state, fingerprint,
                    extra=None, materialize=None, extra_tensors=None):
    """The session after the answer of segment `next_segment - 1` of video `video` and BEFORE anything of the next segment:
    next_segment / segments  index of the segment to read next and how many the video has (equal: the video is finished);
    frames_consumed          [first, last) frame numbers of the video already read;
    answers / turns          entries of the results file / dialogue turns of this video's memory file that belong to the session so far
                             (what is on disk beyond them was written after this checkpoint and is asked again on resume);
    host_state / fingerprint `capture_host_state(...)` / `settings_fingerprint(...)`;  extra: more keys for `extra` (time, question);
    extra_tensors            named tensors that belong to the session (the entry point: the caption embeddings its retrieval has cached)."""
    ex = dict(extra or {})
    ex["resume"] = dict(version=1, video=int(video), next_segment=int(next_segment), segments=int(segments),
                        frames_consumed=[int(x) for x in frames_consumed], answers=int(answers), turns=int(turns),
                        host_state=host_state, fingerprint=fingerprint)
    return save_memory_tree(nodes, checkpoint_path(directory, video), short_memory, extra=ex, materialize=materialize, extra_tensors=extra_tensors)


def resume_info(extra, where="checkpoint"):
    """`extra["resume"]` of a loaded checkpoint; a file without it (written before sessions could resume) is refused with a message"""
    info = (extra or {}).get("resume")
    if not isinstance(info, dict) or info.get("version") != 1:
        raise ResumeError(f"{where}: holds a memory tree but no resume data (position, random state, settings); it was written by a version "
                          f"that could not resume. It still loads with load_memory_tree, but a session cannot continue from it")
    return info


def load_checkpoint(path, fingerprint=None, device="cuda"):
    """(nodes, short_memory, extra, info) of the checkpoint at `path` for RESUMING: refuses files without resume data and, with
    `fingerprint` (this run's `settings_fingerprint`), files written under other settings.  info = extra["resume"] plus
    info["tensors"], the checkpoint's named tensors on `device`."""
    nodes, short, extra, named = _load(path, device)
    info = dict(resume_info(extra, path + ".json"), tensors=named)
    if fingerprint is not None:
        check_fingerprint(info["fingerprint"], fingerprint, path + ".json")
    return nodes, short, extra, info


def find_checkpoint(directory):
    """Path (without extension) of the newest complete checkpoint in `directory`, or None.  Newest = furthest in the session (video, then
    segment).  Complete = its manifest parses and the tensor file it was written with is beside it; a manifest that is not (a copy cut
    short) is passed over for the next one.  Manifests without resume data are not candidates but are reported if nothing else is there."""
    if not directory or not os.path.isdir(directory):
        return None
    cands, old = [], []
    for name in os.listdir(directory):
        m = re.fullmatch(r"video_(\d+)\.json", name)
        if not m:
            continue
        path = os.path.join(directory, name[:-5])
        try:
            with open(path + ".json", encoding="utf-8") as f:
                manifest = json.load(f)
            if manifest.get("format") != FORMAT:
                continue
            _tensor_file_for(path, manifest)
        except (OSError, ValueError):
            continue
        info = manifest.get("extra", {}).get("resume")
        if isinstance(info, dict) and info.get("version") == 1:
            cands.append(((int(info["video"]), int(info["next_segment"])), path))
        else:
            old.append(path)
    if cands:
        return max(cands)[1]
    if old:
        resume_info(None, sorted(old)[-1] + ".json")
    return None
