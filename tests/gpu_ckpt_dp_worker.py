"""One rank of tests/test_gpu_checkpoint_dp.py: the AIR train / test pair on
cuda:0 under a gloo process group (as tests/gpu_dp_worker.py).

  save: two data-parallel steps on shards of unequal size (9 images: 5 + 4)
        and a test-model infer on rank + 2 images, so that every counter
        differs between the ranks; then checkpoint.save_state (every rank
        takes part, rank 0 writes <dir>/air-state-2.npz).
  load: fresh models, checkpoint.load_state of that file, and a second
        save_state into <dir>/again/.

Either way each rank writes what it holds to <dir>/<phase>_<rank>.npz.

usage: gpu_ckpt_dp_worker.py <dir> save|load"""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mog-asr_amd"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import ckpt_cases as cc  # noqa: E402
from mog_air import checkpoint, parallel, trainer  # noqa: E402
from mog_air.records import ShuffleBatcher  # noqa: E402

GLOBAL_BATCH = 9
NOISE_SEED = 40  # + rank


def feed():
    return ShuffleBatcher(np.zeros((37, 1), np.float32), (np.arange(37) % 3).astype(np.int32),
                          GLOBAL_BATCH, 3, min_after_dequeue=10, seed=5)


def held(train, test, f):
    p = train.params
    torch.cuda.synchronize()
    return dict(seeds=np.array([train.noise_seed, test.noise_seed]),
                ctrs=np.array([train._noise_ctr, test._noise_ctr]),
                step=np.array([p.global_step, p.adam_t]),
                crc=np.array([zlib.crc32(getattr(p, n).cpu().numpy().tobytes())
                              for n in ("flat", "m", "v")]),
                next_picks=f.next_indices())


def main():
    folder, phase = sys.argv[1], sys.argv[2]
    dist.init_process_group("gloo")
    try:
        rank, world = dist.get_rank(), dist.get_world_size()
        ctx = trainer.Dist(rank, world)
        train, test = cc.air_pair("fp32", f"ckdp_{phase}_{rank}", seed=21 if phase == "save" else 99,
                                  noise_seed=NOISE_SEED + rank, world=world)
        parallel.attach(train)
        f = feed()
        path = checkpoint.state_path(folder, 2)
        if phase == "save":
            lo, hi = parallel.shard(GLOBAL_BATCH, rank, world)
            for x, k in cc.batches(2, GLOBAL_BATCH):
                f.next_indices()
                train.step(x[lo:hi], k[lo:hi], global_batch=GLOBAL_BATCH)
            x, k = cc.fixed_batch()
            test.infer(x[:rank + 2], k[:rank + 2])
            checkpoint.save_state(path, train, test, feed=f, loop={"step": 2}, ctx=ctx)
        else:
            loop = checkpoint.load_state(path, train, test, feed=f, ctx=ctx)
            assert loop == {"step": 2}, loop
            checkpoint.save_state(checkpoint.state_path(os.path.join(folder, "again"), 2), train,
                                  test, feed=f, loop=loop, ctx=ctx)
        dist.barrier()
        np.savez(os.path.join(folder, f"{phase}_{rank}.npz"), **held(train, test, f))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
