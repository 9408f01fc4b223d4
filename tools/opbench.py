"""What the operator benches (tools/bench_select.py, _explode, _ndjson, _strcol, _filter, _arrowcol, _timecol, _dictcol) share: the
device set-up, the parsed configs[3] shard, the event-timed single execution, the interleaved rounds over a dict of legs, a
leg's record and the JSON write.  Each tool keeps its workload, its verification, its legs and its derived ratios.  Everything
is measured from ONE process on one box (boxes differ by several per cent: only numbers of the same run are compared)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
RATIOS = {"index_ratio": 4, "string_ratio": 1.0, "tape_ratio": 0.25}  # configs[3]'s, as bench.py sizes its shard


def device():
    """-> (torch device 0, a Context of 1 MiB on it, the handle of a side stream that is now torch's current one)"""
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    ctx = S.Context(0, 1 << 20)
    # handle 0 names the context's own stream in the C ABI, so torch's default stream (whose handle is 0 too) cannot carry the
    # events or order torch's own work with the calls: everything goes on a stream of its own
    side = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(side)
    assert side.cuda_stream != 0
    return dev, ctx, side.cuda_stream


def checked_step(shard, stream):
    """one step of the shard, synchronised, and check() clean: no failed document, nothing rejected -> check()'s counts"""
    import torch
    shard.step(stream)
    torch.cuda.synchronize()
    c = shard.check()
    assert c["failed_documents"] == 0 and not shard.rejected_steps, c
    return c


def parsed_shard(ctx, dev, stream, data, offs, **ratios):
    """a batch (bytes or np.uint8, and its offsets) parsed on the device -> (shard, check()'s counts)"""
    import torch
    from simdjson_java_amd import sharding
    shard = sharding.BatchShard(ctx, data if isinstance(data, bytes) else torch.from_numpy(data), offs, dev, **ratios)
    return shard, checked_step(shard, stream)


def configs_shard(ctx, dev, stream, docs):
    """the configs[3] batch (`docs` unique documents, tools/docgen.c) parsed on the device -> (data, offs, shard, check()'s counts)"""
    from tools import workloads as W
    data, offs = W.unique_docs(0, docs)
    return (data, offs) + parsed_shard(ctx, dev, stream, data, offs, **RATIOS)


def timed(fn, steps, warmup):
    """`steps` single executions of fn() behind `warmup` unmeasured ones, each between two HIP events -> their milliseconds"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def wall(fn, steps):
    """`steps` executions of a leg that works on the host, by the wall clock between two synchronisations -> their milliseconds"""
    import torch
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def leg_record(rounds_ms):
    """a leg's milliseconds, one list per round -> its record: the median of the round medians, the smallest time of all, the
    round medians, spread = (largest - smallest round median) / median -- what two repeats of the same leg differ by in this
    run -- and the number of executions"""
    meds = [statistics.median(ms) for ms in rounds_ms]
    median = statistics.median(meds)
    return {"median_ms": median, "min_ms": min(min(ms) for ms in rounds_ms), "round_medians_ms": meds,
            "spread": (max(meds) - min(meds)) / median, "steps": sum(len(ms) for ms in rounds_ms)}


def measure(legs, steps, warmup, third=(), host=(), rounds=3):
    """{leg: fn} -> {leg: leg_record}.  The legs are interleaved, round by round, so that drift of the box hits every leg alike:
    per round a leg runs steps / rounds times (at least 3), the warm-up in front of the first round, one execution in front
    of the others.  Legs named in `third` (slow yardsticks) get a third of the steps; legs named in `host` are timed by the
    wall clock, twice a round."""
    runs = {name: [] for name in legs}
    for r in range(rounds):
        for name, fn in legs.items():
            if name in host:
                runs[name].append(wall(fn, 2))
            else:
                runs[name].append(timed(fn, max(3, steps // (3 if name in third else 1) // rounds), warmup if r == 0 else 1))
    return {name: leg_record(rs) for name, rs in runs.items()}


def write(path, res):
    """the result as indented JSON into `path`, and on one line to stdout"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
