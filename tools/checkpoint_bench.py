"""What a checkpoint costs the training step: `checkpoint.Snapshot` against copying the state to the host tensor by tensor.

    python tools/checkpoint_bench.py [--iters 10] [--steps 200] [--every 25] [--out FILE]

The module and the batch are bench.py's (`build_module`, `synthetic_batch(32, 32000)`), the plan `bf16-mixed`; a few warm steps give
every parameter its Adam moments.  The state's bytes are counted from the image plan.
(a) The baseline a `state_dict()` checkpoint takes: `{k: v.detach().cpu()}` over the module's state_dict, then both optimizers'
    `exp_avg` / `exp_avg_sq` copied to the CPU tensor by tensor.  Two figures, median of `--iters`: the time the main stream is blocked
    (device events around the copies: nothing else can be queued on it meanwhile, the host sits in the blocking copies) and the wall
    time (host clock, device synchronised before and behind).
(b) `Snapshot.take`: the same two figures -- events around the call on the main stream, which holds the pack launches only -- and the
    time until the pinned image is complete (host clock from the call to the image's event); the pack launches' bytes per second (read
    plus written) beside a device-to-device torch copy of one buffer of the image's size.
(c) The mean step time of `--steps` steps with a snapshot every `--every` steps, with a snapshot and the file written from it by a
    thread (to a temporary directory), and with none; the three alternate, twice.
The one condition fixed beforehand: the stream-blocking time of (b) is below that of (a); the script exits non-zero otherwise.
Prints one JSON line per measurement and a summary; `--out` writes both to a file."""
from __future__ import annotations

import argparse
import concurrent.futures
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import bench
    from vibravox_amd import checkpoint as C

    assert torch.cuda.is_available(), "checkpoint_bench measures on an MI355X: no device, no figure"
    dev = torch.device("cuda", 0)
    mod = bench.build_module(dev, 0).set_precision("bf16-mixed")
    batch = bench.synthetic_batch(32, 32000, 1234, dev)
    for _ in range(8):
        mod.training_step(batch)
    torch.cuda.synchronize()
    lines = []

    def emit(**record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    plan = C.plan_image(C.TrainState.of(mod).tensors)
    payload = sum(e.nbytes for e in plan.entries)
    emit(what="state", tensors=len(plan.entries), bytes=payload, image_bytes=plan.image_bytes,
         largest_tensor_bytes=max(e.nbytes for e in plan.entries), tensors_below_one_block=sum(e.nbytes < 16384 for e in plan.entries))

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def baseline():
        out = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
        for opt in mod.configure_optimizers():
            for st in opt.state.values():
                out[id(st)] = (st["exp_avg"].cpu(), st["exp_avg_sq"].cpu())
        return out

    snap = C.Snapshot()

    def measure(fn, finish):
        """(ms the main stream is blocked, ms wall until `finish(result)` returns)"""
        torch.cuda.synchronize()
        e0, e1 = events()
        t0 = time.perf_counter()
        e0.record()
        result = fn()
        e1.record()
        finish(result)
        wall = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), wall

    for _ in range(2):   # warm both paths: pinned allocations, code objects
        baseline()
        snap.take(C.TrainState.of(mod)).wait()
    a, b = [], []
    for _ in range(args.iters):   # alternated
        a.append(measure(baseline, lambda r: torch.cuda.synchronize()))
        b.append(measure(lambda: snap.take(C.TrainState.of(mod)), lambda taken: taken.wait()))
    a_block, a_wall = (statistics.median(x[i] for x in a) for i in (0, 1))
    b_block, b_wall = (statistics.median(x[i] for x in b) for i in (0, 1))
    emit(what="(a) state_dict().cpu() tensor by tensor", stream_blocked_ms=round(a_block, 3), wall_ms=round(a_wall, 3),
         spread_blocked_ms=[round(min(x[0] for x in a), 3), round(max(x[0] for x in a), 3)])
    emit(what="(b) Snapshot.take", stream_blocked_ms=round(b_block, 3), pinned_image_complete_ms=round(b_wall, 3),
         spread_blocked_ms=[round(min(x[0] for x in b), 3), round(max(x[0] for x in b), 3)],
         host_gbytes_per_s=round(plan.image_bytes / b_wall / 1e6, 2))

    # the pack launches alone, against a device copy of the same bytes
    from vibravox_amd._lib import check, load, stream
    tensors = list(C.TrainState.of(mod).tensors.values())
    table, _ = C.pack_table(plan, tensors)
    image = torch.zeros(plan.image_bytes, dtype=torch.uint8, device=dev)
    other = torch.empty_like(image)

    def timed(fn, n=20):
        fn()
        torch.cuda.synchronize()
        e0, e1 = events()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    pack_ms = timed(lambda: check(load().eben_pack_tensors(table, len(plan.entries), image.data_ptr(), plan.total, image.data_ptr() + plan.total,
                                                           stream()), "pack_tensors"))
    unpack_ms = timed(lambda: check(load().eben_unpack_tensors(table, len(plan.entries), image.data_ptr(), plan.total, stream()), "unpack_tensors"))
    copy_ms = timed(lambda: other.copy_(image))
    emit(what="pack launches", ms=round(pack_ms, 4), launches=-(-len(plan.entries) // 48), read_plus_written_gbytes_per_s=round(2 * plan.total / pack_ms / 1e6, 1),
         unpack_ms=round(unpack_ms, 4), device_copy_of_the_image_ms=round(copy_ms, 4), device_copy_gbytes_per_s=round(2 * plan.image_bytes / copy_ms / 1e6, 1))

    # (c) steps with and without snapshots
    tmp = tempfile.mkdtemp(prefix="checkpoint_bench_")
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)

    def steps(mode):
        pending = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            mod.training_step(batch)
            if mode != "none" and (i + 1) % args.every == 0:
                taken = snap.take(C.TrainState.of(mod))
                if mode == "files":
                    job = pool.submit(lambda t=taken, k=i: C.write_file(t.checkpoint(), os.path.join(tmp, f"s{k % 2}.ckpt")))
                    snap.reading(taken, job)
                    pending.append(job)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        for job in pending:
            job.result()
        return ms

    try:
        runs = {"none": [], "snapshots": [], "files": []}
        for _ in range(2):
            for mode in runs:
                runs[mode].append(round(steps(mode), 4))
        emit(what=f"(c) mean step ms over {args.steps} bf16-mixed steps, a snapshot every {args.every}", **runs,
             file_bytes=os.path.getsize(os.path.join(tmp, "s0.ckpt")))
    finally:
        pool.shutdown()
        shutil.rmtree(tmp, ignore_errors=True)
    ok = b_block < a_block
    summary = (f"state {payload / 1e6:.1f} MB in {len(plan.entries)} tensors; main stream blocked {a_block:.2f} ms by the per-tensor copies, "
               f"{b_block:.3f} ms by Snapshot.take ({'below' if ok else 'NOT below'}); pinned image complete after {b_wall:.2f} ms, the per-tensor "
               f"copies after {a_wall:.2f} ms; pack {pack_ms * 1e3:.0f} us; step {statistics.mean(runs['none']):.3f} ms without, "
               f"{statistics.mean(runs['snapshots']):.3f} ms with snapshots, {statistics.mean(runs['files']):.3f} ms with files")
    lines.append(summary)
    print(summary, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
