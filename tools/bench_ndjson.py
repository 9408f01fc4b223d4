"""What making the doc_offsets of an NDJSON buffer on the device costs -> profiles/r10/ndjson.json, everything from ONE process on
one box (boxes differ by several per cent: only numbers of the same run are compared).

Workloads:
  configs   the configs[3] batch (1,000,000 unique documents of about 1 KB, tools/docgen.c), one document per line;
  twitter   twitter.json's statuses minified, one per line, replicated to about 1 GB.
The offsets the call makes are first verified against the generator's own.  Then, per workload, interleaved, medians of
event-timed single executions:
  split       sjmi_ndjson_offsets_device (summaries, scan, emit: the input is read twice);
  split_size  the same call with offset_capacity 0 (how a caller sizes its array: one read);
  read        a read-only torch pass over the same bytes;
  parse       the accepted optimistic step (sjmi_parse_batch_device_optimistic) on the same buffer with the offsets the split made;
  host        what a caller does today: numpy.flatnonzero(buf == 10) into offsets on the CPU plus their H2D copy (wall clock).
  python tools/bench_ndjson.py [--workloads configs,twitter] [--docs N] [--bytes B] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(torch, S, sharding, opbench, dev, ctx, stream, data, offs, steps, warmup):
    """data: np.uint8, one document per line; offs: the generator's offsets"""
    n, n_docs = int(data.size), int(offs.size) - 1
    host = torch.from_numpy(data)
    raw = torch.zeros(n + 128, dtype=torch.uint8, device=dev)
    raw[:n] = host.to(dev)
    d_offs = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
    res = torch.zeros(3, dtype=torch.int64, device=dev)
    split = lambda: ctx.ndjson_offsets_device(raw.data_ptr(), n, d_offs.data_ptr(), n_docs + 1, res.data_ptr(), stream)
    split()
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    assert (int(r[0]), int(r[1]), int(r[2])) == (n_docs, n, 1), r
    assert np.array_equal(d_offs.cpu().numpy().view(np.uint64), offs), "the offsets differ from the generator's"
    shard = sharding.BatchShard(ctx, raw[:n], None, dev, device_offsets=d_offs, **opbench.RATIOS)
    opbench.checked_step(shard, stream)  # (nothing rejected: the timed step is the optimistic one)
    words = raw[:n // 8 * 8].view(torch.int64)
    h2d = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)

    def host_offsets():
        nl = np.flatnonzero(data == 10)
        o = np.empty(nl.size + 1, dtype=np.int64)
        o[0] = 0
        o[1:] = nl + 1
        h2d.copy_(torch.from_numpy(o))

    legs = {"split": split,
            "split_size": lambda: ctx.ndjson_offsets_device(raw.data_ptr(), n, 0, 0, res.data_ptr(), stream),
            "read": lambda: words.sum(),
            "parse": lambda: shard.step(stream),
            "host": host_offsets}
    out = {"documents": n_docs, "input_bytes": n, "tile_bytes": int(S.lib().sjmi_ndjson_tile_bytes())}
    out.update(opbench.measure(legs, steps, warmup, host={"host"}))
    sp = out["split"]["median_ms"]
    out["split_over_read"] = sp / out["read"]["median_ms"]
    out["split_size_over_read"] = out["split_size"]["median_ms"] / out["read"]["median_ms"]
    out["split_share_of_parse"] = sp / out["parse"]["median_ms"]
    out["host_over_split"] = out["host"]["median_ms"] / sp
    out["split_GBps_of_input"] = n / sp / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="configs,twitter")
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "ndjson.json"))
    a = ap.parse_args()
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import sharding
    from tests.conftest import load_fixture
    from tools import opbench
    from tools import workloads as W
    dev, ctx, stream = opbench.device()
    out = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SJMI_LIB") or "libsjmi.so"}
    todo = a.workloads.split(",")
    if "configs" in todo:
        data, offs = W.unique_docs(0, a.docs)
        out["configs"] = run(torch, S, sharding, opbench, dev, ctx, stream, np.asarray(data), np.asarray(offs, dtype=np.uint64), a.steps, a.warmup)
        del data
    if "twitter" in todo:
        statuses = json.loads(load_fixture("twitter.json"))["statuses"]
        lines = [json.dumps(s, ensure_ascii=False, separators=(",", ":")).encode("utf-8") + b"\n" for s in statuses]
        unit = b"".join(lines)
        reps = max(1, a.bytes // len(unit))
        lens = np.tile(np.array([len(l) for l in lines], dtype=np.uint64), reps)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        data = np.tile(np.frombuffer(unit, dtype=np.uint8), reps)
        out["twitter"] = run(torch, S, sharding, opbench, dev, ctx, stream, data, offs, a.steps, a.warmup)
        out["twitter"]["statuses"] = len(lines)
    opbench.write(a.out, out)
    ctx.close()


if __name__ == "__main__":
    main()
