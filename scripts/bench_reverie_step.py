"""ms per pre-training step on REVERIE-style object batches: today's eager path against captured obj_static batches.

    python scripts/bench_reverie_step.py [--batch 64] [--rounds 6] [--window 16] [--pool 12] [--out profiles/reverie_step_bench.txt]

BevBertConfig.reverie() (object tokens, 1000 detector classes; tasks mlm, mrc, sap, og in turn), bf16 compute, dropout
0.1, ONE model and ONE trainer.  The "dataset" is a pool of 256 ragged synthetic samples (1..7 steps, 40..80 tokens, 36..38
views, 0..20 objects per panorama -- the reference's max_objects); ``--pool`` host batches per task are collated from it
once and fed in a fixed cycle, grid features as rows of a device-resident GridFeatureStore.  Two variants run in turns:
  eager     loader.BucketManager(obj_static=False): object batches keep their own shapes and per-sample step counts in the
            bucket signature, StaticBatch.capturable is False, every step is issued from Python
  captured  loader.BucketManager(obj_static=True): every varying axis padded, object / MRC rows as loader-built tables; a
            buffer set is captured on its third use and replayed from then on
Each variant is warmed up first, in whole cycles, at most ``--max-warm-cycles``: until a cycle allocates no buffer set
and no pinned staging buffer any more (with two buffer sets per bucket the eager manager builds the second sets in its
second cycle and their staging buffers in the refills of the third and fourth), and, for the captured variant, until every
step of a cycle is a replay.  A window is ``--window`` consecutive steps of one variant between two device
synchronisations, loader work on the main thread (plan, refill) included; the median over ``--rounds`` windows per variant
is reported, with the share of the window's steps that were replays, the buckets each manager created and what the
managers allocated inside the timed windows (nothing, if the warm-up settled).  No gate."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vln_bevbert_amd import synthetic  # noqa: E402
from vln_bevbert_amd.config import BevBertConfig  # noqa: E402
from vln_bevbert_amd.feature_store import GridFeatureStore  # noqa: E402
from vln_bevbert_amd.loader import BucketManager, quiet_gc  # noqa: E402
from vln_bevbert_amd.pretrain_cmt import GlocalTextPathCMTPreTraining  # noqa: E402
from vln_bevbert_amd.train import PretrainTrainer  # noqa: E402

TASKS = ("mlm", "mrc", "sap", "og")


class Variant:
    def __init__(self, name, cfg, dev, store, obj_static, schedule):
        self.name, self.schedule, self.cursor = name, schedule, 0
        self.mgr = BucketManager(cfg, dev, depth=2, max_buckets=256, grid_store=store, obj_static=obj_static)

    def allocations(self):
        """Buffer sets and pinned staging buffers this manager has allocated so far (both are one-time costs of a set)."""
        sets = [sb for b in self.mgr.buckets.values() for sb in b["sets"]]
        return self.mgr.stats["buffer_sets_allocated"], sum(len(sb.__dict__.get("_stage", {})) for sb in sets)

    def warm_up(self, trainer, cycle, max_cycles, need_replay):
        """Whole cycles until one allocates nothing (and replays every step, if asked); returns (cycles run, settled)."""
        for k in range(1, max_cycles + 1):
            before = self.allocations()
            _, rep, _ = self.run(trainer, cycle)
            if self.allocations() == before and (rep == cycle or not need_replay):
                return k, True
        return max_cycles, False

    def run(self, trainer, n):
        """n steps from the cycle; returns (seconds between two device synchronisations, replayed steps, seconds in acquire)."""
        dev = self.mgr.device
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        replayed, t_load = 0, 0.0
        for _ in range(n):
            task, batch, keys = self.schedule[self.cursor % len(self.schedule)]
            self.cursor += 1
            ta = time.perf_counter()
            sb = self.mgr.acquire(task, batch, grid_keys=keys)
            t_load += time.perf_counter() - ta
            if sb.ready is not None:
                torch.cuda.current_stream(dev).wait_event(sb.ready)
            replayed += sb.graph is not None
            trainer.step(task, sb)
            self.mgr.release(sb)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, replayed, t_load


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--pool", type=int, default=12, help="host batches per task")
    ap.add_argument("--max-warm-cycles", type=int, default=10)
    ap.add_argument("--max-objects", type=int, default=20)
    ap.add_argument("--store-rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverie_step_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = BevBertConfig.reverie()
    torch.manual_seed(0)
    model = GlocalTextPathCMTPreTraining(cfg)
    arena = model.finalize(dev, torch.bfloat16)
    model.train()
    model.set_dropout(0.1)
    trainer = PretrainTrainer(model, arena, learning_rate=5e-5, warmup_steps=100, num_train_steps=100000)

    g = torch.Generator(device=dev).manual_seed(5)
    P = 12 * cfg.grid_hw * cfg.grid_hw
    rgbs = torch.randn(a.store_rows, P, 768, device=dev, dtype=torch.float16, generator=g)
    depths = torch.rand(a.store_rows, 12, cfg.grid_hw, cfg.grid_hw, device=dev, generator=g) * 0.6
    depths = depths * (torch.rand(depths.shape, device=dev, generator=g) > 0.05)
    sems = torch.randint(0, max(1, cfg.sem_classes), (a.store_rows, P), device=dev, generator=g).to(torch.uint8)
    store = GridFeatureStore([f"s_{i}" for i in range(a.store_rows)], rgbs, depths, sems, dev)

    rng = np.random.default_rng(11)
    samples = [synthetic.make_sample(rng, i, cfg, int(rng.integers(1, 8)), int(rng.integers(40, 81)), ragged_views=True,
                                     grid=False, max_objects=a.max_objects) for i in range(256)]
    schedule = []
    for k in range(a.pool):
        for task in TASKS:
            pick = rng.choice(len(samples), size=a.batch, replace=len(samples) < a.batch)
            batch = synthetic.collate([samples[int(i)] for i in pick], cfg, task, rng, sems_as="ids")
            keys = [f"s_{int(i)}" for i in rng.integers(0, a.store_rows, size=a.batch)]
            schedule.append((task, batch, keys))
    cycle = len(schedule)
    variants = [Variant("eager", cfg, dev, store, False, schedule), Variant("captured", cfg, dev, store, True, schedule)]

    lines = [f"bench_reverie_step: batch {a.batch}, tasks {','.join(TASKS)}, {cycle} host batches in the cycle, "
             f"0..{a.max_objects} objects per panorama, bf16, dropout 0.1, {torch.cuda.get_device_name(dev)}"]
    warm = [v.warm_up(trainer, cycle, a.max_warm_cycles, need_replay=v.name == "captured") for v in variants]
    lines.append("warm-up: " + "; ".join(f"{v.name} {k} cycles ({'settled: the last one allocated nothing' if ok else 'NOT settled'})"
                                          for v, (k, ok) in zip(variants, warm)) + f"; graph_error {trainer.graph_error}")
    quiet_gc()
    res = {v.name: [] for v in variants}
    alloc0 = [v.allocations() for v in variants]
    for r in range(a.rounds):
        for v in variants:
            sec, rep, t_load = v.run(trainer, a.window)
            res[v.name].append((1000.0 * sec / a.window, rep / a.window, 1000.0 * t_load / a.window))
            lines.append(f"round {r} {v.name:<8} {1000.0 * sec / a.window:8.2f} ms/step  replayed {rep}/{a.window}  "
                         f"acquire (plan + refill, host) {1000.0 * t_load / a.window:6.2f} ms/step")
    for v in variants:
        ms = statistics.median(x[0] for x in res[v.name])
        share = sum(x[1] for x in res[v.name]) / len(res[v.name])
        load = statistics.median(x[2] for x in res[v.name])
        st = v.mgr.stats
        lines.append(f"{v.name:<8} median {ms:8.2f} ms/step over {a.rounds} windows of {a.window} steps; share of steps replayed "
                     f"{share:.3f}; acquire {load:.2f} ms/step; buckets created {st['buckets_created']}, buffer sets "
                     f"{st['buffer_sets_allocated']}, refills {st['refills']}, captured graphs {v.mgr.captured_graphs()}")
    lines.append("allocations inside the timed windows (buffer sets, staging buffers): " + ", ".join(
        f"{v.name} {now[0] - was[0]}, {now[1] - was[1]}" for v, was, now in zip(variants, alloc0, (v.allocations() for v in variants))))
    e = statistics.median(x[0] for x in res["eager"])
    c = statistics.median(x[0] for x in res["captured"])
    lines.append(f"captured / eager = {c / e:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
