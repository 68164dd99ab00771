"""The full train state of a trainer run, saved and restored (DESIGN.md
§4.16): one ``air-state-<step>.npz`` per save next to ``trainer.Saver``'s
variables file, holding what a run stopped at step N needs to continue as the
uninterrupted run does, bit for bit.

File layout (plain ``np.savez``, read with ``allow_pickle=False``):

  <variable>           every variable under its name, '/' spelled '__' (as Saver)
  adam_m__<variable>   its Adam first moment
  adam_v__<variable>   its Adam second moment
  feed_buf             the shuffle buffer (int64), when a feed was saved
  meta                 one JSON string: format version, entry point, variable
                       specs, precision, global_step, adam_t, the fp32 beta
                       powers as bit patterns, world size, per rank the noise
                       seed and Philox offset of the train and the test model,
                       the feed state, the loop state, the dataset fingerprint

The moments are stored per variable, not as the flat buffers, so a change of
padding or layout does not invalidate a file.  Loading copies into the
existing ``flat`` / ``m`` / ``v`` buffers (views, weight caches and a captured
graph keep their pointers) and checks everything before it writes anything.

This module imports without the HIP library (as records.py does): torch is
only needed once a model is passed in.
"""
from __future__ import annotations

import glob
import json
import os
import re
import warnings
from typing import Dict, List, Optional, Tuple

import numpy as np

FORMAT_VERSION = 1
STATE_PREFIX = "air-state"
KEEP = 3  # as trainer.Saver(max_to_keep=3)
_M, _V = "adam_m__", "adam_v__"
_RESERVED = ("meta", "feed_buf")
_STEP = re.compile(r"^" + STATE_PREFIX + r"-(\d+)\.npz$")
_ENTRY = {"air_model": "training_air_original", "asr_model": "train_air_pr"}


# ---------------------------------------------------------------- files ----
def key_of(name: str) -> str:
    """A variable's name inside the file (Saver's spelling)."""
    return name.replace("/", "__")


def state_path(folder: str, step: int) -> str:
    return os.path.join(folder, "%s-%d.npz" % (STATE_PREFIX, step))


def write_file(path: str, arrays: Dict[str, np.ndarray], meta: Optional[dict]) -> str:
    """Atomic write: a temporary file in the same folder, then os.replace, so
    a killed save never leaves a truncated newest file.  The temporary name
    does not end in .npz, so ``latest`` never sees it."""
    out = {k: np.asarray(v) for k, v in arrays.items()}
    for k, v in out.items():
        if v.dtype.hasobject:  # np.savez would pickle it; the files are read without pickle
            raise ValueError("%r is an object array: a state file holds plain arrays only" % k)
    if meta is not None:
        out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    tmp = "%s.tmp-%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **out)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def read_file(path: str) -> Tuple[Dict[str, np.ndarray], Optional[dict]]:
    """(arrays, meta) of a state file, or (variables, None) of one of Saver's
    variables files."""
    with np.load(path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    meta = arrays.pop("meta", None)
    if meta is not None:
        meta = json.loads(str(meta))
        if meta.get("format") != FORMAT_VERSION:
            raise ValueError("%s: state format %r, this code reads format %d" % (
                path, meta.get("format"), FORMAT_VERSION))
    return arrays, meta


def _states(folder: str) -> List[Tuple[int, str]]:
    found = []
    for p in glob.glob(os.path.join(folder, STATE_PREFIX + "-*")):
        m = _STEP.match(os.path.basename(p))
        if m:
            found.append((int(m.group(1)), p))
    return sorted(found)


def latest(folder: str) -> Optional[str]:
    """The state file of the highest step in ``folder`` (None: there is none)."""
    found = _states(folder)
    return found[-1][1] if found else None


def rotate(folder: str, keep: int = KEEP) -> None:
    """Keep the ``keep`` state files of the highest steps."""
    for _, p in _states(folder)[:-keep]:
        os.remove(p)


def resolve(path: str) -> str:
    """--restore PATH: a file, or a folder (its newest state)."""
    if os.path.isdir(path):
        found = latest(path)
        if found is None:
            raise ValueError("no %s-<step>.npz in %s" % (STATE_PREFIX, path))
        return found
    if not os.path.exists(path):
        raise ValueError("no such state file: %s" % path)
    return path


# ----------------------------------------------------------- the checks ----
def check_variables(specs, arrays: Dict[str, np.ndarray], moments: bool = False,
                    what: str = "state file") -> None:
    """ValueError naming the first variable of ``specs`` (name, shape) that
    ``arrays`` lacks or holds with another shape (``moments``: its Adam m / v
    too), or the first variable in ``arrays`` that ``specs`` does not have."""
    known = set()
    for name, shape in specs:
        for prefix in ("", _M, _V) if moments else ("",):
            k = prefix + key_of(name)
            known.add(k)
            if k not in arrays:
                raise ValueError("%s has no %r (variable %s of the model, shape %s)" % (
                    what, k, name, tuple(shape)))
            if tuple(arrays[k].shape) != tuple(shape):
                raise ValueError("%s holds variable %s with shape %s, the model's is %s" % (
                    what, name, tuple(arrays[k].shape), tuple(shape)))
    for k in arrays:
        if k in _RESERVED or k in known or k.startswith((_M, _V)):
            continue
        raise ValueError("%s holds variable %s, which the model does not have" % (
            what, k.replace("__", "/")))


def _f32_bits(v) -> int:
    return int(np.asarray(v, np.float32).reshape(1).view(np.uint32)[0])


def _bits_f32(b: int) -> np.float32:
    return np.asarray([b], np.uint32).view(np.float32)[0]


def _rank_world(ctx) -> Tuple[int, int]:
    return (0, 1) if ctx is None else (int(ctx.rank), int(ctx.world))


def _counters(train_model, test_model, ctx) -> List[dict]:
    """Per rank, the noise seed and Philox offset of each model.  Shards of
    unequal size advance the offsets differently, so every rank contributes
    its own: one small SUM all-reduce of a table that is zero outside this
    rank's row."""
    rank, world = _rank_world(ctx)
    mine = [train_model.noise_seed, train_model._noise_ctr]
    mine += [test_model.noise_seed, test_model._noise_ctr] if test_model is not None else [0, 0]
    table = np.zeros((world, 4), np.int64)
    table[rank] = mine
    if world > 1:
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(table).to(train_model.device)
        dist.all_reduce(t)
        table = t.cpu().numpy()
    return [{"train": [int(r[0]), int(r[1])],
             "test": [int(r[2]), int(r[3])] if test_model is not None else None}
            for r in table]


def _entry(model) -> str:
    kind = type(model).__module__.rsplit(".", 1)[-1]
    return _ENTRY.get(kind, kind)


def _host_vars(params, buf: str) -> Dict[str, np.ndarray]:
    host = getattr(params, buf).detach().cpu().numpy()
    out = {}
    for name, shape in params.specs:
        o = params.offsets[name]
        out[name] = host[o:o + int(np.prod(shape))].reshape(shape).copy()
    return out


# ------------------------------------------------------------- save/load ----
def save_state(path: str, train_model, test_model=None, feed=None, loop=None, ctx=None) -> str:
    """Write the train state to ``path``.  Every rank must call it (the
    per-rank counters are gathered); rank 0 writes.  ``feed``: an object with
    ``get_state()`` / ``fingerprint()`` (records.ShuffleBatcher, DeviceFeed,
    the trainer's host feed); ``loop``: the loop's JSON-serialisable state."""
    rank, world = _rank_world(ctx)
    noise = _counters(train_model, test_model, ctx)
    if rank != 0:
        return path
    p = train_model.params
    arrays = {}
    for prefix, buf in (("", "flat"), (_M, "m"), (_V, "v")):
        for name, a in _host_vars(p, buf).items():
            arrays[prefix + key_of(name)] = a
    meta = {"format": FORMAT_VERSION, "entry": _entry(train_model),
            "specs": [[name, list(shape)] for name, shape in p.specs],
            "precision": train_model.precision,
            "global_step": int(p.global_step), "adam_t": int(p.adam_t),
            "beta1_power_bits": _f32_bits(p.beta1_power),
            "beta2_power_bits": _f32_bits(p.beta2_power),
            "world": world, "noise": noise, "feed": None, "fingerprint": None,
            "loop": loop}
    if feed is not None:
        st = dict(feed.get_state())
        arrays["feed_buf"] = np.asarray(st.pop("buf"), np.int64)
        meta["feed"] = st
        meta["fingerprint"] = feed.fingerprint()
    return write_file(path, arrays, meta)


def _load_params(params, arrays, moments: bool) -> None:
    """In place: the variables (and the moments) into the existing buffers.
    What lies between the variables (alignment, padding) stays as it is."""
    import torch
    for prefix, buf in (("", "flat"), (_M, "m"), (_V, "v")) if moments else (("", "flat"),):
        t = getattr(params, buf)
        host = t.detach().cpu().numpy().copy()
        for name, shape in params.specs:
            o = params.offsets[name]
            a = np.ascontiguousarray(arrays[prefix + key_of(name)], np.float32)
            host[o:o + a.size] = a.reshape(-1)
        t.copy_(torch.from_numpy(host))
    params.version += 1


def load_variables(path: str, model) -> None:
    """The variables of a state file, or of one of Saver's variables files,
    into ``model`` (in place).  Optimizer, step, noise and feed stay as they
    are: a fresh model starts fresh."""
    arrays, meta = read_file(path)
    if meta is None:
        check_variables(model.params.specs, arrays, what=path)
    else:
        check_variables(model.params.specs, arrays, moments=True, what=path)
    _load_params(model.params, arrays, moments=False)


def load_state(path: str, train_model, test_model=None, feed=None, ctx=None,
               mode: str = "resume"):
    """Restore ``path`` into the models (which share one ParamStore: loaded
    once) and the feed; returns the saved loop state.  Every rank reads the
    same file and takes its own counters.  ``mode="weights"``: the variables
    only (load_variables).  ``feed=None`` restores no feed and checks no
    dataset fingerprint.  Every mismatch raises ValueError before anything is
    written to the models."""
    if mode not in ("resume", "weights"):
        raise ValueError("mode must be 'resume' or 'weights', got %r" % (mode,))
    if mode == "weights":
        load_variables(path, train_model)
        return None
    arrays, meta = read_file(path)
    if meta is None:
        raise ValueError("%s holds variables only: it can be loaded with mode='weights'" % path)
    p = train_model.params
    if test_model is not None and test_model.params is not p:
        raise ValueError("the train and the test model do not share their variables")
    check_variables(p.specs, arrays, moments=True, what=path)
    rank, world = _rank_world(ctx)
    if meta["world"] != world:
        raise ValueError("%s was saved by %d ranks, this run has %d" % (path, meta["world"], world))
    mine = meta["noise"][rank]
    for model, part in ((train_model, "train"), (test_model, "test")):
        if model is None:
            continue
        if mine[part] is None:
            raise ValueError("%s holds no %s model's noise counters" % (path, part))
        if mine[part][0] != model.noise_seed:
            raise ValueError("%s: the %s model of rank %d drew its noise from seed %d, this "
                             "one's noise_seed is %d" % (path, part, rank, mine[part][0],
                                                         model.noise_seed))
    if feed is not None:
        if meta["feed"] is None:
            raise ValueError("%s holds no feed state" % path)
        if meta["fingerprint"] != feed.fingerprint():
            raise ValueError("%s was saved over another dataset (%s), this one is %s" % (
                path, meta["fingerprint"], feed.fingerprint()))
    if meta["precision"] != train_model.precision:
        warnings.warn("%s was saved at precision %s and continues at %s: the parameters are "
                      "fp32 either way, but the run is no longer the uninterrupted one" % (
                          path, meta["precision"], train_model.precision))
    # ---- everything checked: write
    if feed is not None:
        feed.set_state(dict(meta["feed"], buf=arrays["feed_buf"]))
    _load_params(p, arrays, moments=True)
    p.global_step, p.adam_t = int(meta["global_step"]), int(meta["adam_t"])
    p.beta1_power = _bits_f32(meta["beta1_power_bits"])
    p.beta2_power = _bits_f32(meta["beta2_power_bits"])
    train_model._noise_ctr = int(mine["train"][1])
    if test_model is not None:
        test_model._noise_ctr = int(mine["test"][1])
    return meta["loop"]
