"""Training driver behind the kept entry points (training_air_original.py,
train_air_pr.py): results-folder handling, logging and the input pipeline
(``setup_run``, the head of both main()s), the train / test model pair sharing
one variable scope (``model_pair``), and the one iteration loop with the
reference's logging / testing / checkpoint cadence and its end-of-data
(OutOfRangeError) epilogue (``train_loop``) — training_air_original.py:18-503
and train_air_pr.py:18-400 restated around ``AIRModel.step`` / ``infer``.
What the two trainers do differently inside the loop -- how a step's numbers
are kept, the log line, what a test pass reports -- is AIR_STYLE / ASR_STYLE,
which the entry points pass by name.

Image grids (training_air_original.py:368-411, :445-490): every
IMAGE_SAVE_ITERATION iterations and at the end, the test model's
reconstruction / misclassified / generation grids are written as PNG files
under summary/ (``mog_air.visualize``).  With --summaries 1 the reference's
TensorBoard summaries (training_air_original.py:223-301) are computed on the
device and written as an event file beside them (``mog_air.summaries``,
DESIGN.md §4.19).

Checkpoints: ``Saver`` writes the variables (models/air-model-<step>.npz),
``StateSaver`` the full train state beside them (models/air-state-<step>.npz,
``mog_air.checkpoint``); ``--restore`` continues a run from such a state
(``restore``, ``LoopState``).
"""
from __future__ import annotations

import dataclasses
import glob
import logging
import operator
import os
import shutil
import time
from typing import Optional

import numpy as np

from . import checkpoint, records
from .evaluation import evaluation

EPOCHS = 300
BATCH_SIZE = 64
LOG_EACH_ITERATION = 20
TEST_EACH_ITERATION = 200
IMAGE_SAVE_ITERATION = 500  # training_air_original.py:31
NUM_IMAGES_TO_SAVE = 60     # :43
SAVE_PARAMS_EACH_ITERATIONS = 10000


def add_common_args(parser, reader_threads: int):
    """The CLI flags shared by both entry points (training_air_original.py:49-60,
    train_air_pr.py:40-61) plus this framework's options (not in the
    reference): --iterations, --precision, --test-batch, --synth-per-count,
    --write-synthetic, --device, --resident, --save-every, --restore,
    --restore-mode, --eval-only, --batch-size, --stream, --stream-seed,
    --graph, --summaries, --summary-cadence."""
    parser.add_argument("-r", "--results-folder", default="Not Valid")
    parser.add_argument("-k", "-key", "--key", default="")
    parser.add_argument("-gpu", "--gpu", default="-1")
    parser.add_argument("-data", "--data", default="mnist")
    parser.add_argument("-o", "--overwrite-results", type=int, choices=[0, 1], default=0)
    parser.add_argument("-t", "--reader-threads", type=int, default=reader_threads)
    parser.add_argument("-dn", "--dig_num", type=str, default="02")
    parser.add_argument("-dl", "--dig_location", type=str, default="")
    parser.add_argument("-ds", "--dig_surfix", type=str, default="")
    parser.add_argument("--iterations", type=int, default=0,
                        help="stop after this many train iterations (0: run all epochs)")
    parser.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    parser.add_argument("--test-batch", type=int, default=0,
                        help="test-set images per test-model launch (0: whole set)")
    parser.add_argument("--synth-per-count", type=int, default=2000,
                        help="images per object count when the dataset files are absent")
    parser.add_argument("--write-synthetic", type=int, choices=[0, 1], default=0)
    parser.add_argument("--device", default="cuda:0")
    parser.add_argument("--resident", type=int, choices=[0, 1], default=0,
                        help="1: the datasets live on the device -- batches gathered there "
                             "(records.DeviceFeed), detection metrics computed there "
                             "(evaluation.DeviceEvaluator)")
    parser.add_argument("--no-images", action="store_true",
                        help="skip the PNG grids (training_air_original.py:368-411)")
    parser.add_argument("--save-every", type=int, default=SAVE_PARAMS_EACH_ITERATIONS,
                        help="iterations between two saves of models/air-model-<step>.npz (the "
                             "variables) and models/air-state-<step>.npz (the full train state); "
                             "0: only the state at the end")
    parser.add_argument("--restore", default=None, metavar="PATH",
                        help="an air-state-<step>.npz, or a models/ folder (its newest state)")
    parser.add_argument("--restore-mode", choices=["resume", "weights"], default="resume",
                        help="resume: continue the saved run; weights: its variables only "
                             "(also from an air-model-<step>.npz), everything else fresh")
    parser.add_argument("--eval-only", type=int, choices=[0, 1], default=0,
                        help="1 (with --restore): the final test pass and grids of the restored "
                             "state, no training")
    parser.add_argument("--batch-size", type=int, default=BATCH_SIZE,
                        help="images per train step, over all ranks (the reference's 64)")
    parser.add_argument("--stream", type=int, choices=[0, 1], default=0,
                        help="1: every batch is fresh stand-in canvases made on the device "
                             "(records.StreamFeed); needs --iterations and absent dataset files")
    parser.add_argument("--stream-seed", type=int, default=12345)
    parser.add_argument("--graph", type=int, choices=[0, 1], default=0,
                        help="1: every iteration is the captured train step "
                             "(train_step_graphed) and its log row stays on the device until a "
                             "log line or a state save needs it (LogRing); one device only")
    parser.add_argument("--summaries", type=int, choices=[0, 1], default=0,
                        help="1: the reference's TensorBoard summaries, computed on the device, "
                             "as an event file under summary/ (summaries.Summaries); one "
                             "device only")
    parser.add_argument("--summary-cadence", default="50,250,500,100", metavar="NUM,VAR,IMG,GRAD",
                        help="iterations between two numeric / variable / image / gradient "
                             "summaries (training_air_original.py:33-36)")


def select_gpu(gpu: str) -> None:
    """-gpu N (training_air_original.py:64-65): must run before the HIP runtime
    starts; HIP_VISIBLE_DEVICES is the ROCm spelling of CUDA_VISIBLE_DEVICES.
    Under torch.distributed.run (WORLD_SIZE > 1) each rank takes the GPU of
    its LOCAL_RANK instead (distributed_setup)."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return
    if 0 <= int(gpu) <= 7:
        os.environ["HIP_VISIBLE_DEVICES"] = str(gpu)


class Dist:
    """Data-parallel context of one trainer process: rank,
    world, the contiguous shard of each global batch this rank trains on."""

    def __init__(self, rank: int = 0, world: int = 1):
        self.rank, self.world = rank, world

    @property
    def main(self) -> bool:
        return self.rank == 0

    def shard(self, x, k):
        """This rank's contiguous part of a global batch."""
        if self.world == 1:
            return x, k
        from .parallel import shard
        lo, hi = shard(len(k), self.rank, self.world)
        return x[lo:hi], k[lo:hi]

    def mean(self, values, device, weight: float = 1.0):
        """Weighted mean over ranks of a few host scalars (one small
        all-reduce): each rank's values are per-image means over its shard, so
        weighting by the shard size (``weight``) gives the global batch mean
        even when the shards differ in size (a global batch that does not
        divide by the world size)."""
        if self.world == 1:
            return list(values)
        import torch
        import torch.distributed as dist
        t = torch.tensor([float(v) * weight for v in values] + [float(weight)],
                         dtype=torch.float64, device=device)
        dist.all_reduce(t)
        return (t[:-1] / t[-1]).tolist()

    def barrier(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()


def distributed_setup(args) -> Dist:
    """One process per GPU under torch.distributed.run: RCCL ("nccl") process
    group, device = cuda:LOCAL_RANK (written into args.device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return Dist()
    import torch
    import torch.distributed as dist
    local = int(os.environ.get("LOCAL_RANK", "0"))
    args.device = "cuda:%d" % local
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", device_id=torch.device(args.device))
    return Dist(dist.get_rank(), world)


def attach_data_parallel(train_model, ctx: Dist) -> None:
    if ctx.world > 1:
        from .parallel import attach
        attach(train_model)


def model_pair(make, ctx: Dist, **config):
    """The train model and the test model sharing its variable scope
    (training_air_original.py:158-211): ``make(None, None, **config)`` twice,
    with independent Monte-Carlo noise per rank; the train model is attached
    to the data-parallel group."""
    models = []
    for i in range(2):
        print("Creating {0} model...".format("training" if i == 0 else "testing"))
        models.append(make(None, None, train=(i == 0), reuse=(i == 1),
                           noise_seed=1235 + ctx.rank, grad_world=ctx.world if i == 0 else 1,
                           **config))
    attach_data_parallel(models[0], ctx)
    return models


def dataset_files(args, entry: str):
    """(train file, test file, canvas size, common name), as the entry points
    derive them from -data/-dn/-dl/-ds (training_air_original.py:67-91)."""
    digits = [int(c) for c in args.dig_num]
    if args.dig_location not in ["", "right_half"]:
        raise ValueError("not valid location of digit: " + args.dig_location)
    name = args.dig_location + args.dig_surfix + "".join(str(d) for d in digits)
    if args.data.lower() == "mnist":
        folder, canvas = "./data/multi_mnist_data/", 50
    else:
        folder, canvas = "./data/multi_dsprites/", 64
    return (os.path.join(folder, f"common{name}.tfrecords"),
            os.path.join(folder, f"test{name}.tfrecords"), canvas, name, digits)


def check_feed_args(args, train_file: str, test_file: str) -> None:
    """--batch-size / --stream: refused before anything is written.  A stream
    of stand-in glyphs is not mixed with a real test file, and it never ends,
    so the run needs --iterations."""
    if getattr(args, "batch_size", BATCH_SIZE) < 1:
        raise ValueError("--batch-size must be positive")
    if not getattr(args, "stream", 0):
        return
    if os.path.exists(train_file) or os.path.exists(test_file):
        raise ValueError("--stream 1 draws the offline stand-in glyphs, but the dataset files "
                         "%s / %s exist: train from them (--stream 0) or move them away" % (
                             train_file, test_file))
    if not args.iterations > 0:
        raise ValueError("--stream 1 needs --iterations: the stream never ends")
    if not 0 <= args.stream_seed < 2 ** 63:
        raise ValueError("--stream-seed must be in [0, 2^63)")


def check_graph_args(args, ctx: Dist, annealed=()) -> None:
    """--graph 1: refused before anything is written where the captured step
    would refuse the model the entry point builds (graph.GraphCapture._graph_ok):
    more than one rank, or an annealed hyper-parameter (``annealed``: the
    names in the model's annealing_schedules) that a capture would freeze."""
    if not getattr(args, "graph", 0):
        return
    if ctx.world > 1:
        raise ValueError("--graph 1 is the single-device train step, but this run has %d ranks"
                         % ctx.world)
    frozen = [n for n in annealed if n != "z_pres_prior_log_odds"]
    if frozen:
        raise ValueError("--graph 1: annealed %s would be frozen at capture" % frozen)


def check_summary_args(args, ctx: Dist) -> None:
    """--summaries 1: refused before anything is written with a malformed
    --summary-cadence or more than one rank (the fetches read one device's
    train state)."""
    if not getattr(args, "summaries", 0):
        return
    from .summaries import parse_cadence
    parse_cadence(getattr(args, "summary_cadence", "50,250,500,100"))
    if ctx.world > 1:
        raise ValueError("--summaries 1 reads the single-device train state, but this run has "
                         "%d ranks" % ctx.world)


def results_folder(args, entry: str, name: str, main: bool = True) -> str:
    """training_air_original.py:93-115: default name, -k suffix, -o overwrite
    or the next free _N suffix; creates models/, summary/, source/ (rank 0
    only when data parallel — the other ranks write nothing)."""
    if args.results_folder == "Not Valid":
        args.results_folder = "./results/{time}-({file}_{data})_(train.{train}_test.{test})".format(
            file=entry, train=name.replace("_", "."), test=name.replace("_", "."),
            time=time.strftime("%Y-%m-%d-%H-%M"), data=args.data)
    args.results_folder += "_({})".format(args.key)
    if not main:
        return args.results_folder
    if os.path.exists(args.results_folder):
        if args.overwrite_results:
            shutil.rmtree(args.results_folder, ignore_errors=True)
        else:
            base, i = args.results_folder, 0
            args.results_folder = f"{base}_{i}"
            while os.path.exists(args.results_folder):
                i += 1
                args.results_folder = f"{base}_{i}"
    for sub in ("", "models", "summary", "source"):
        os.makedirs(os.path.join(args.results_folder, sub), exist_ok=True)
    return args.results_folder


def build_logger(folder: str, args, main: bool = True) -> logging.Logger:
    """utils/checkpoints.py:31-63: console + results-folder log file, then the
    sorted configurable parameters between '#' rules (rank 0 only when data
    parallel; the other ranks log nothing)."""
    fmt = "%(asctime)s;%(levelname)s|%(message)s"
    log = logging.getLogger("mog_air")
    log.setLevel(logging.INFO)
    log.propagate = False
    for h in list(log.handlers):
        log.removeHandler(h)
    if not main:
        log.addHandler(logging.NullHandler())
        return log
    sh = logging.StreamHandler()
    sh.setFormatter(logging.Formatter(fmt, "%H-%M-%S"))
    log.addHandler(sh)
    fh = logging.FileHandler(os.path.join(folder, "logfile{}.log".format(time.strftime("%m-%d"))))
    fh.setFormatter(logging.Formatter(fmt, "%H:%M:%S"))
    log.addHandler(fh)
    log.info("#" * 120)
    log.info("----------Configurable Parameters In this Model----------")
    for k, v in sorted(vars(args).items(), key=operator.itemgetter(0)):
        log.info("# " + ("%20s" % k) + ":\t" + str(v))
    log.info("#" * 120)
    return log


def copy_sources(folder: str, roots) -> None:
    """training_air_original.py:128-135: snapshot of the *.py sources."""
    for src in roots:
        dst = os.path.join(folder, "source", os.path.basename(os.path.normpath(src))
                           if src not in (".", "./") else "")
        os.makedirs(dst, exist_ok=True)
        for f in glob.glob(os.path.join(src, "*.py")):
            shutil.copy(f, dst)


def load_data(args, train_file, test_file, digits, log):
    """Train arrays + test tuple (read_test_data).  When the files are absent
    (the reference builds them from MNIST, which needs the network), an
    offline synthetic dataset of the same layout is generated (datasets.py)
    and optionally written to the expected paths."""
    if os.path.exists(train_file) and os.path.exists(test_file):
        log.info("Reading %s and %s", train_file, test_file)
        tr_x, tr_k = records.load_images(train_file)
        test = records.read_test_data(test_file, shift_zero_digits_images=True)
        return tr_x, tr_k, test
    from . import datasets
    log.warning("dataset files %s / %s not found: synthesizing an offline stand-in "
                "(%d images per object count)", train_file, test_file, args.synth_per_count)
    kind = "mnist" if args.data.lower() == "mnist" else "dsprites"
    sets = datasets.synthesize(kind, digits, args.synth_per_count,
                               test_set_size=min(1000, args.synth_per_count * len(digits) // 5),
                               seed=0, bbox="bbox" in args.dig_surfix)
    if args.write_synthetic:
        for path, split in ((train_file, "train"), (test_file, "test")):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            s = sets[split]
            records.write_to_records(path[:-len(".tfrecords")], s["images"], s["indices"],
                                     s["positions"], s["boxes"], s["labels"], s["digits"])
        return load_data(args, train_file, test_file, digits, log)
    tr = sets["train"]
    tr_x = np.stack([im.ravel() for im in tr["images"]]).astype(np.float32)
    tr_k = np.asarray(tr["digits"], np.int32)
    te = sets["test"]
    test = (np.stack([im.ravel() for im in te["images"]]).astype(np.float32),
            np.asarray(te["digits"], np.int32), [np.asarray(v, np.int32) for v in te["indices"]],
            [np.asarray(v, np.int32) for v in te["positions"]],
            [np.asarray(v, np.int32) for v in te["boxes"]],
            [np.asarray(v, np.int32) for v in te["labels"]])
    return tr_x, tr_k, test


def setup_run(args, entry: str, annealed=()):
    """The head of both entry points' main() (training_air_original.py:67-135):
    the argument refusals before anything is written, the results folder
    before the logger, the data before the models.  ``entry``: the entry
    point's file name; ``annealed``: see check_graph_args.  Returns (ctx,
    results folder, logger, train images, train counts, test tuple, canvas
    size, digits)."""
    train_file, test_file, canvas, name, digits = dataset_files(args, entry)
    check_feed_args(args, train_file, test_file)
    ctx = distributed_setup(args)  # one process per GPU under torch.distributed.run
    check_graph_args(args, ctx, annealed=annealed)
    check_summary_args(args, ctx)
    folder = results_folder(args, entry, name, main=ctx.main)
    log = build_logger(folder, args, main=ctx.main)
    if ctx.main:
        package = os.path.dirname(os.path.abspath(__file__))
        copy_sources(folder, [os.path.dirname(os.path.dirname(package)), package])
    log.info("Creating input pipeline...")
    if not ctx.main:
        ctx.barrier()  # rank 0 writes synthetic data first when asked to
    tr_x, tr_k, test = load_data(args, train_file, test_file, digits, log)
    if ctx.main:
        ctx.barrier()
    return ctx, folder, log, tr_x, tr_k, test, canvas, digits


class Saver:
    """tf.train.Saver(max_to_keep=3) stand-in: <folder>/<prefix>-<step>.npz
    holding every variable under its TF name."""

    def __init__(self, folder: str, prefix: str, max_to_keep: int = 3):
        self.folder, self.prefix, self.keep = folder, prefix, max_to_keep
        self.saved = []

    def save(self, params, step: int) -> str:
        path = os.path.join(self.folder, f"{self.prefix}-{step}.npz")
        np.savez(path, **{k.replace("/", "__"): v for k, v in params.state_dict().items()})
        self.saved.append(path)
        while len(self.saved) > self.keep:
            old = self.saved.pop(0)
            if os.path.exists(old):
                os.remove(old)
        return path


@dataclasses.dataclass
class LoopState:
    """What the iteration loop carries from one iteration to the next beside
    the models and the feed (saved with the train state, checkpoint.py).
    ``rows`` (AIR): the [loss, accuracy, mse] of every iteration since the
    last log line; ``logged`` (AIR-ASR): the log variables since then."""
    step: int = 0
    min_loss: float = 9999999.0
    update_flag: bool = False
    best: list = dataclasses.field(default_factory=lambda: [0.0, 0.0, 0.0, 0.0])
    rows: list = dataclasses.field(default_factory=list)
    logged: dict = dataclasses.field(default_factory=dict)

    def as_dict(self) -> dict:
        return {"step": int(self.step), "min_loss": float(self.min_loss),
                "update_flag": bool(self.update_flag), "best": [float(v) for v in self.best],
                "rows": [[float(v) for v in r] for r in self.rows],
                "logged": {n: [float(x) for x in v] for n, v in self.logged.items()}}

    @classmethod
    def from_dict(cls, d: dict) -> "LoopState":
        return cls(**{f.name: d[f.name] for f in dataclasses.fields(cls)})


class LogRing:
    """--graph 1: the log rows of the iterations since the last log line, on
    the device ([LOG_EACH_ITERATION, len(model.log_names)] fp32).  ``push``
    has the model write its last step's row into the next free one
    (``log_row_``: one launch, no host read; the row index is the host's);
    ``drain`` is the loop's only host read of step results."""

    def __init__(self, model, rows: int = LOG_EACH_ITERATION):
        import torch
        self.buf = torch.zeros((rows, len(model.log_names)), device=model.device,
                               dtype=torch.float32)
        self.n = 0

    def push(self, model) -> None:
        if self.n >= self.buf.shape[0]:
            raise RuntimeError("LogRing is full (%d rows): drain() it before the next push"
                               % self.buf.shape[0])
        model.log_row_(self.buf[self.n])
        self.n += 1

    def drain(self) -> list:
        """The pushed rows in push order as lists of Python floats (one
        device-to-host copy; none when nothing was pushed); empties the ring."""
        if self.n == 0:
            return []
        rows = self.buf[:self.n].cpu().tolist()
        self.n = 0
        return rows


class StateSaver:
    """Saver's companion: models/air-state-<step>.npz, the newest 3 kept.
    Every rank calls ``save`` (checkpoint.save_state gathers the per-rank
    noise counters); rank 0 writes and rotates."""

    def __init__(self, folder: str, train_model, test_model, feed, ctx):
        self.folder, self.ctx = folder, ctx
        self.models, self.feed = (train_model, test_model), feed

    def save(self, loop: LoopState) -> None:
        checkpoint.save_state(checkpoint.state_path(self.folder, loop.step), *self.models,
                              feed=self.feed, loop=loop.as_dict(), ctx=self.ctx)
        if self.ctx.main:
            checkpoint.rotate(self.folder)


def restore(args, train_model, test_model, feed, ctx, log) -> LoopState:
    """--restore / --restore-mode / --eval-only: the loop state to start from
    (a fresh one without --restore or with --restore-mode weights).  An
    evaluation restores no feed, so it needs no dataset of the same
    fingerprint."""
    path = getattr(args, "restore", None)
    eval_only = bool(getattr(args, "eval_only", 0))
    if path is None:
        if eval_only:
            raise ValueError("--eval-only 1 needs --restore")
        return LoopState()
    path = checkpoint.resolve(path)
    mode = getattr(args, "restore_mode", "resume")
    saved = checkpoint.load_state(path, train_model, test_model,
                                  feed=None if eval_only else feed, ctx=ctx, mode=mode)
    log.info("Restored %s (%s) at step %d", path, mode, train_model.global_step)
    return LoopState.from_dict(saved) if saved is not None else LoopState()


def resident_ok(args, tr_x, test, test_model, log) -> bool:
    """--resident 1 is taken only when both datasets fit in half of the
    device's free memory and the test set is within the metrics kernel's caps
    (boxes per image, loop steps); otherwise one warning and the host path."""
    if not getattr(args, "resident", 0):
        return False
    import torch

    from .evaluation import EVAL_CAP
    need = int(np.asarray(tr_x).nbytes) + int(np.asarray(test[0]).nbytes)
    free = torch.cuda.mem_get_info(torch.device(args.device))[0]
    boxes = max([len(p) // 2 for p in test[3]], default=0)
    why = None
    if need > free // 2:
        why = "the datasets take %d bytes, more than half of the %d free" % (need, free)
    elif boxes > EVAL_CAP or test_model.max_steps > EVAL_CAP:
        why = "%d boxes per image / %d loop steps exceed the device metrics' cap of %d" % (
            boxes, test_model.max_steps, EVAL_CAP)
    if why is not None:
        log.warning("--resident 1 not taken (%s): host feed and host metrics", why)
        return False
    return True


class _HostFeed:
    """The host input pipeline: ShuffleBatcher batches, sharded per rank."""

    def __init__(self, tr_x, tr_k, ctx, batch_size: int = BATCH_SIZE):
        self.ctx = ctx
        self.batcher = records.ShuffleBatcher(tr_x, tr_k, batch_size, EPOCHS,
                                              min_after_dequeue=min(10000, len(tr_k)))

    def next_batch(self):
        xg, kg = self.batcher.next_batch()
        x, k = self.ctx.shard(xg, kg)
        return x, k, len(kg)

    # every rank runs the same shuffle and slices its shard: one state serves all
    def get_state(self):
        return self.batcher.get_state()

    def set_state(self, state) -> None:
        self.batcher.set_state(state)

    def fingerprint(self):
        return self.batcher.fingerprint()


def stream_feed(args, ctx, batch_size: int):
    """records.StreamFeed over the glyphs load_data's stand-in test set was
    made from (datasets.synthesize with seed 0), on -data's canvas, drawing the
    object counts of -dn."""
    from . import datasets
    kind = "mnist" if args.data.lower() == "mnist" else "dsprites"
    bank, sizes, _ = datasets.glyph_bank(kind, bbox="bbox" in args.dig_surfix, seed=0)
    return records.StreamFeed(bank, sizes, [int(c) for c in args.dig_num],
                              50 if kind == "mnist" else 64, batch_size,
                              seed=getattr(args, "stream_seed", 12345), device=args.device,
                              rank=ctx.rank, world=ctx.world)


def make_feed(args, tr_x, tr_k, ctx, resident: bool):
    """(x, k, global batch size) per ``next_batch()``: this rank's shard of
    the shuffled batch, host arrays or (resident) device tensors; with
    --stream 1 fresh canvases made on the device (the train split is unused)."""
    batch_size = getattr(args, "batch_size", BATCH_SIZE)
    if getattr(args, "stream", 0):
        return stream_feed(args, ctx, batch_size)
    if not resident:
        return _HostFeed(tr_x, tr_k, ctx, batch_size)
    return records.DeviceFeed(tr_x, tr_k, batch_size, EPOCHS,
                              min_after_dequeue=min(10000, len(tr_k)), device=args.device,
                              rank=ctx.rank, world=ctx.world)


def resident_test_set(args, test, canvas: int, test_model):
    """The test images and digit counts on the device (the per-object lists
    stay on the host) and the evaluator holding the ground-truth boxes."""
    import torch

    from .evaluation import DeviceEvaluator
    dev = torch.device(args.device)
    images = torch.from_numpy(np.ascontiguousarray(test[0], np.float32)).to(dev)
    digits = torch.from_numpy(np.ascontiguousarray(test[1], np.int32)).to(dev)
    evaluator = DeviceEvaluator(test[3], test[4], canvas, dev, max_steps=test_model.max_steps)
    return (images, digits) + tuple(test[2:]), evaluator


def run_test(test_model, test, canvas: int, batch: int, evaluator=None):
    """Test-model fetches over the whole test set: (loss, accuracy, mse,
    rec_scales, rec_shifts, rec_num_digits), batched when `batch` > 0 and
    combined as the batch means the reference computes in one run.  With an
    ``evaluator`` (evaluation.DeviceEvaluator; test[0] / test[1] device
    tensors) every chunk's detections go to it in place and (loss, accuracy,
    mse, evaluator) is returned."""
    images, digits = test[0], test[1]
    n = len(digits)
    step = batch if batch > 0 else n
    loss = acc = mse = 0.0
    scales, shifts, nums = [], [], []
    T = test_model.max_steps
    for s in range(0, n, step):
        x, k = images[s:s + step], digits[s:s + step]
        test_model.infer(x, k)
        w = len(k) / n
        loss += test_model.loss * w
        acc += test_model.accuracy * w
        mse += test_model.mse_loss * w
        if evaluator is not None:
            evaluator.update(s, test_model.rec_shifts, test_model.rec_scales,
                             test_model.rec_num_digits)
            continue
        sc = np.zeros((len(k), T, 1), np.float32)
        sh = np.zeros((len(k), T, 2), np.float32)
        rs, rh = test_model.rec_scales.cpu().numpy(), test_model.rec_shifts.cpu().numpy()
        sc[:, :rs.shape[1]] = rs
        sh[:, :rh.shape[1]] = rh
        scales.append(sc)
        shifts.append(sh)
        nums.append(test_model.rec_num_digits.cpu().numpy())
    if evaluator is not None:
        return loss, acc, mse, evaluator
    return loss, acc, mse, np.concatenate(scales), np.concatenate(shifts), np.concatenate(nums)


METRICS = "test:{}\tprecision:{}\trecall:{}\tgtIoU:{:.4f}\tdetectionIoU:{:.4f}\t{}:{:.4f}"
BEST = "{} Best: elbo:{}\taccu:{}\tmse:{}\tiou:{}"


def _follow_best(log, st: LoopState, results: list) -> None:
    """After a test pass: its results are the best ones when the train loss has
    reached a new minimum since the last update."""
    if st.update_flag:
        st.update_flag = False
        st.best = results
    log.info(BEST.format("Current", *st.best))


class AirStyle:
    """What training_air_original.py:226-503 does its own way in train_loop: a
    step's [loss, accuracy, mse] is a row of LoopState.rows; the best results
    follow the periodic tests only, and the final test is tagged 'final'."""
    grids_per_count = True  # generation grids for every object count of -dn
    full_summaries = True   # --summaries 1: numeric and image summaries too

    def step_row(self, model, fetched):
        return list(fetched[:3])

    def keep(self, st, model, rows):
        st.rows.extend(rows)

    def log_line(self, st, model, mean):
        """(train loss, log line, the line's (name, mean) pairs) of the rows
        since the last log line (the last LOG_EACH_ITERATION), which are
        dropped."""
        l0, l1, l2 = mean(np.mean(st.rows, axis=0))
        st.rows = []
        return l0, ("iteration {}\ttrain loss {:.3f}\ttrain accuracy {:.2f}, "
                    "train mse {:.3f}".format(st.step, l0, l1, l2)), \
            list(zip(model.log_names, (l0, l1, l2)))

    def report(self, log, st, final, sums, detections, test_model):
        log.info("iteration {}\ttest loss {:.3f}\ttest accuracy {:.2f}, test mse {:.3f}".format(
            "final" if final else st.step, *sums))
        d = detections()
        # integer steps are padded to 6 as training_air_original.py:357 does
        log.info(METRICS.format("final" if final else "{:6d}".format(st.step), *d[:4],
                                "globaliou", d[4]))
        if not final:
            _follow_best(log, st, [*sums, d[4]])


class AsrStyle:
    """What train_air_pr.py:284-400 does its own way in train_loop: a step's
    log variables are kept per name in LoopState.logged; every test, the final
    one included, is tagged with the step (train_air_pr.py:426-430), logs the
    test model's log variables and is followed by the best results."""
    grids_per_count = False  # train_air_pr.py:362-398: the model's loop draws the counts
    full_summaries = False   # train_air_pr.py has the numeric / image summaries commented out

    def step_row(self, model, fetched):
        return list(model.log_variables.values())

    def keep(self, st, model, rows):
        for row in rows:
            for n, v in zip(model.log_names, row):
                st.logged.setdefault(n, []).append(v)

    def log_line(self, st, model, mean):
        """(TotLoss, log line, the line's (name, mean) pairs) of the variables
        since the last log line, which are dropped: the means in the model's
        order (a restored ``logged`` may list them in another)."""
        names = model.log_names
        means = mean([np.mean(st.logged[n]) for n in names])
        st.logged = {}
        return float(means[names.index("TotLoss")]), "step:{:6d}\t".format(st.step) + "".join(
            "{}:{:.4f}\t".format(n, v) for n, v in zip(names, means)), list(zip(names, means))

    def report(self, log, st, final, sums, detections, test_model):
        d = detections()
        log.info(METRICS.format("{:6d}".format(st.step), *d[:4], "global_iou", d[4]))
        lv = test_model.log_variables  # (as the test set's last chunk left them)
        log.info("test:{:6d}\t".format(st.step) +
                 "".join("{}:{:.4f}\t".format(n, v) for n, v in lv.items()))
        _follow_best(log, st, [lv["elbo"], lv["accu"], lv["mse"], d[4]])


AIR_STYLE, ASR_STYLE = AirStyle(), AsrStyle()


def train_loop(args, train_model, test_model, tr_x, tr_k, test, canvas, log, models_folder,
               ctx: Optional[Dist] = None, *, style):
    """The iteration loop of both trainers (training_air_original.py:226-503,
    train_air_pr.py:284-400): logging every 20 iterations, testing every 200,
    image grids every 500, parameters and the train state every --save-every
    (10,000); the final test when the input runs out or --iterations is
    reached.  ``style`` (AIR_STYLE / ASR_STYLE) is what the two differ in: how
    a step's numbers are kept, the log line and what a test pass reports.
    With --restore the loop starts from the saved state; --eval-only 1 runs
    the epilogue alone."""
    ctx = ctx or Dist()
    resident = resident_ok(args, tr_x, test, test_model, log)
    feed = make_feed(args, tr_x, tr_k, ctx, resident)
    test_dev, evaluator = (resident_test_set(args, test, canvas, test_model)
                           if resident and ctx.main else (None, None))
    saver = Saver(models_folder, "air-model")
    states = StateSaver(models_folder, train_model, test_model, feed, ctx)
    st = restore(args, train_model, test_model, feed, ctx, log)
    # --graph 1: the captured step; its log rows wait in the ring until a log
    # line, a state save or the end of the loop reads st.rows / st.logged
    ring = LogRing(train_model) if args.graph else None

    def drain():
        if ring is not None:
            style.keep(st, train_model, ring.drain())

    def save_state():
        drain()
        states.save(st)

    def test_pass(final=False):
        if not ctx.main:
            ctx.barrier()
            return
        if evaluator is not None:
            tl, ta, tm, _ = run_test(test_model, test_dev, canvas, args.test_batch, evaluator)
            detections = evaluator.result
        else:
            tl, ta, tm, sc, sh, nd = run_test(test_model, test, canvas, args.test_batch)

            def detections():
                return evaluation(test[3], test[4], sh, sc, nd, csize=canvas)
        ctx.barrier()
        style.report(log, st, final, (tl, ta, tm), detections, test_model)

    summary_folder = os.path.join(os.path.dirname(os.path.normpath(models_folder)), "summary")
    vis_n = args.test_batch if args.test_batch > 0 else len(test[1])
    digits = [int(c) for c in args.dig_num] if style.grids_per_count else None

    def save_images(tag, gen_tag=None):
        if not ctx.main or args.no_images:
            return
        from .visualize import save_visualizations
        save_visualizations(test_model, test[0][:vis_n], test[1][:vis_n], summary_folder, tag,
                            digits=digits, num=NUM_IMAGES_TO_SAVE, gen_tag=gen_tag)

    # --summaries 1: the reference's TensorBoard summaries into a new event
    # file (also after --restore: nothing of the writer is restored)
    summ = None
    if getattr(args, "summaries", 0) and ctx.main and not args.eval_only:
        from .summaries import Summaries, parse_cadence
        summ = Summaries(summary_folder, train_model.params, parse_cadence(args.summary_cadence),
                         full=style.full_summaries, log=log)
    summ_test = test_dev if test_dev is not None else test

    log.info("Training...\n")
    while not args.eval_only:
        pre_step = st.step
        if summ is not None:
            # training_air_original.py:252-283: before the save and the step
            summ.before_step(pre_step, test_model, summ_test[0], summ_test[1], args.test_batch,
                             vis_n=vis_n)
        if args.save_every > 0 and st.step % args.save_every == 0:
            if ctx.main:
                saver.save(train_model.params, st.step)
            save_state()
        try:
            x, k, nglobal = feed.next_batch()
        except StopIteration:  # the end of the data (the reference's OutOfRangeError)
            break
        if ring is not None:
            train_model.train_step_graphed(x, k, global_batch=nglobal)
            ring.push(train_model)
            st.step = train_model.global_step
        else:
            fetched = train_model.step(x, k, global_batch=nglobal)
            st.step = fetched[3]
            style.keep(st, train_model, [style.step_row(train_model, fetched)])
        if summ is not None and summ.wants_gradients(pre_step):
            # :290-301: the gradients this step applied, under the post-step number
            summ.gradients(train_model.params, train_model.gradient_clipping_norm, st.step)
        if st.step % LOG_EACH_ITERATION == 0:
            drain()
            # the global batch's means (shard-size weighted over ranks)
            loss, line, pairs = style.log_line(
                st, train_model, lambda v: ctx.mean(v, args.device, weight=len(k)))
            log.info(line)
            if summ is not None:
                summ.scalars([("train/" + n, v) for n, v in pairs], st.step)
            if loss < st.min_loss:
                st.update_flag, st.min_loss = True, loss
        # (train_air_pr.py:31 spells its constant TESET_EACH_ITERATION; both are 200)
        if st.step % TEST_EACH_ITERATION == 0:
            test_pass()
        if st.step % IMAGE_SAVE_ITERATION == 0:
            save_images(st.step)
        if args.iterations and st.step >= args.iterations:
            break
    drain()  # the loop's end: the rows since the last log line
    if not args.eval_only:
        # before the final test, so that an evaluation of this file draws the
        # noise the run's own final test drew
        save_state()
    test_pass(final=True)
    # the final reconstruction / misclassified grids are tagged 'final', the
    # final generation grids with the step (training_air_original.py:478-483,
    # train_air_pr.py:462-469)
    save_images("final", gen_tag=st.step)
    if summ is not None:
        summ.close()
    log.info(BEST.format("Final", *st.best))
    log.info("\ntraining has ended\n")
    return st.step
