"""What turning RFC 3339 string columns into Arrow timestamp arrays on the device costs -> profiles/r16/timecol.json, everything
from ONE process on one box (boxes differ by several per cent: only numbers of the same run are compared).

The input is made here (tools/docgen.c emits no such strings): `--docs` NDJSON documents of configs[3] size (768 .. 1280 bytes),
each with two RFC 3339 members -- "created_at" ends in Z with second precision, "updated_at" has a 6-digit fraction and an
offset --, about 1 % of each malformed and 1 % MISSING, and a string of padding.  They are parsed and selected on the device; every
leg's outputs are first compared with the Python reference of tests/timecol_common.py on a 10,000-row sample and with the counts
the generator made on all rows.  Then, interleaved, medians of single calls between HIP events, everything at MICRO:
  one_field                 created_at
  two_fields                both members
  counting                  both members as the counting call (no data block)
  two_fields_after_filter   both on the columns a filter compacted (created_at is a string), its rows taken from n_kept on the device
  string_gather             sjmi_string_column_device of the created_at column: the route there was before (and a host parse
                            would still have to follow it)
each beside ONE device-to-device copy that moves the bytes the call must at least move: 9 + the string's bytes read and 8.125
written per live cell (the counting call: 0.125 written) -- a copy of half that sum reads and writes it.  The A/B of the two
fetch forms is a program of its own, tools/ubench/timecol_ab.hip: where its binary is built it runs as a child process and its
result goes into the file under "fetch_ab".
--trace-legs K: no timing; after the verification each leg K times in a row, for a rocprofv3 --kernel-trace run of its own.
  python tools/bench_timecol.py [--docs N] [--steps K] [--warmup W] [--out PATH] [--trace-legs K] [--no-ab]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POINTERS = ["/created_at", "/updated_at", "/id"]
STRING, MISSING = ord('"'), 0


def make_documents(n, seed=20261019):
    """-> (bytes, offsets uint64 [n + 1], per column the member's text or None where it is MISSING)"""
    rng = np.random.default_rng(seed)
    secs = rng.integers(946684800, 1893456000, size=(2, n))  # 2000 .. 2030
    stamps = [np.datetime_as_string(secs[c].astype("datetime64[s]"), unit="s") for c in range(2)]
    micros, zone_h, zone_q, sign = rng.integers(0, 1000000, size=n), rng.integers(0, 14, size=n), rng.integers(0, 4, size=n), rng.integers(0, 2, size=n)
    kind = rng.integers(0, 100, size=(2, n))  # 0: malformed, 1: MISSING
    hit = rng.integers(0, 19, size=(2, n))
    lengths = rng.integers(768, 1281, size=n)
    pad = b"p" * 1280
    texts, parts, offs = [[None] * n, [None] * n], [], np.zeros(n + 1, dtype=np.uint64)
    at = 0
    for r in range(n):
        a = stamps[0][r].encode() + b"Z"
        b = b"%s.%06d%s%02d:%02d" % (stamps[1][r].encode(), micros[r], b"+-"[sign[r]:sign[r] + 1], zone_h[r], 15 * zone_q[r])
        members = [b'"id":%d' % r]
        for c, text in ((0, a), (1, b)):
            if kind[c, r] == 0:
                text = text[:hit[c, r]] + b"/" + text[hit[c, r] + 1:]  # ('/' is nowhere in the grammar)
            if kind[c, r] != 1:
                texts[c][r] = text
                members.append(b'"%s":"%s"' % ((b"created_at", b"updated_at")[c], text))
        head = b"{%s" % b",".join(members)
        doc = b'%s,"pad":"%s"}\n' % (head, pad[:max(0, int(lengths[r]) - len(head) - 11)])
        parts.append(doc)
        at += len(doc)
        offs[r + 1] = at
    return b"".join(parts), offs, texts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "timecol.json"))
    ap.add_argument("--trace-legs", type=int, default=0)
    ap.add_argument("--no-ab", action="store_true")
    a = ap.parse_args()
    import torch
    import simdjson_java_amd as S
    from tests import timecol_common as TC
    from tools import opbench
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_timecol.py measures on a GPU: none is present")
    n = a.docs
    data, offs, texts = make_documents(n)
    dev, ctx, stream = opbench.device()
    shard, _ = opbench.parsed_shard(ctx, dev, stream, data, offs, **opbench.RATIOS)
    del data
    select = S.SelectPlan(POINTERS)
    types, values = shard.select(select, stream)
    torch.cuda.synchronize()
    n_cols = len(POINTERS)

    # ---- what the generator made: per column the cells, their values at MICRO and the counts
    cell_of = lambda text: (0, False, False, False, False, False) if text is None else TC.cell_of_bytes("us", (), STRING, text)
    strings = [sum(t is not None for t in texts[col]) for col in range(2)]
    is_string = np.array([t is not None for t in texts[0]])
    plan = S.FilterPlan([(0, "type_eq", STRING)])
    _, f_types, f_values, _, f_result = shard.filter(plan, types, values, stream=stream)
    torch.cuda.synchronize()
    n_kept = int(f_result[0])
    assert n_kept == strings[0]
    kept_rows = np.flatnonzero(is_string)
    fields2 = [(0, "us"), (1, "us")]
    legs = {"one_field": (fields2[:1], types, values, None, True), "two_fields": (fields2, types, values, None, True),
            "counting": (fields2, types, values, None, False), "two_fields_after_filter": (fields2, f_types, f_values, f_result[0:1], True)}
    live_of = {name: n_kept if leg[3] is not None else n for name, leg in legs.items()}
    words = (n + 63) // 64
    out = {"data": torch.empty((2, n), dtype=torch.int64, device=dev), "validity": torch.empty((2, words), dtype=torch.int64, device=dev),
           "results": torch.empty((2, 6), dtype=torch.int64, device=dev)}

    def run_leg(name):
        fields, t, v, rc, with_data = legs[name]
        ctx.time_columns_device(fields, t.data_ptr(), v.data_ptr(), n_cols, n, n, rc.data_ptr() if rc is not None else 0, shard.sb.data_ptr(),
                                out["data"].data_ptr() if with_data else 0, n if with_data else 0, out["validity"].data_ptr(), words,
                                out["results"].data_ptr(), stream)

    # ---- every leg verified before timing: the records on all rows against the generator's counts (the reference's verdict on
    # every string it made: the malformed ones carry a '/'), data and validity against the reference on a sample of the rows
    verdicts = [[cell_of(t) for t in texts[col]] for col in range(2)]
    rng = np.random.default_rng(7)
    counts = {}
    for name, (fields, t, v, rc, with_data) in legs.items():
        live = live_of[name]
        rows_of = (lambda j: kept_rows[j]) if rc is not None else (lambda j: j)
        out["data"].fill_(-1)
        out["validity"].fill_(-1)
        run_leg(name)
        torch.cuda.synchronize()
        got = out["results"][:len(fields)].cpu().tolist()
        want = []
        for f in fields:
            cells = [verdicts[f[0]][rows_of(j)] for j in range(live)]
            want.append([live] + [sum(cell[k] for cell in cells) for k in range(1, 6)])
        assert got == want, (name, got, want)
        sample = np.sort(rng.choice(live, size=min(a.sample, live), replace=False))
        for k, f in enumerate(fields):
            validity = out["validity"][k, :(live + 63) // 64].cpu().numpy().view(np.uint64)
            data_row = out["data"][k].cpu().numpy().view(np.uint64)
            assert bool((out["validity"][k, (live + 63) // 64:] == -1).all()) and bool((out["data"][k, live if with_data else 0:] == -1).all()), (name, k)
            for j in sample.tolist():
                cell = verdicts[f[0]][rows_of(j)]
                assert bool(int(validity[j >> 6]) >> (j & 63) & 1) == cell[1], (name, k, j)
                assert not with_data or int(data_row[j]) == cell[0], (name, k, j, int(data_row[j]), cell[0])
        counts[name] = {"fields": len(fields), "live_rows": live, "n_valid": [w[1] for w in want], "n_other": [w[2] for w in want],
                        "n_malformed": [w[3] for w in want], "n_range": [w[4] for w in want], "n_inexact": [w[5] for w in want]}

    # ---- the route there was before: the string gather of the created_at column (a sizing call, then the call that is timed)
    g_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    g_validity = torch.empty(words, dtype=torch.int64, device=dev)
    g_result = torch.empty(4, dtype=torch.int64, device=dev)
    gather = lambda d, cap: ctx.string_column_device(types[0].data_ptr(), values[0].data_ptr(), n, shard.sb.data_ptr(), g_offsets.data_ptr(), g_validity.data_ptr(),
                                                     d.data_ptr() if cap else 0, cap, g_result.data_ptr(), stream)
    gather(None, 0)
    torch.cuda.synchronize()
    total_bytes = int(g_result[0])
    string_bytes = [sum(len(t) for t in texts[col] if t is not None) for col in range(2)]
    assert total_bytes == string_bytes[0] and int(g_result[1]) == strings[0]
    g_bytes = torch.empty(total_bytes, dtype=torch.uint8, device=dev)
    gather(g_bytes, total_bytes)
    torch.cuda.synchronize()
    first = next(t for t in texts[0] if t is not None)
    assert bytes(g_bytes[:len(first)].cpu().numpy()) == first

    timed_legs = {name: (lambda name=name: run_leg(name)) for name in legs}
    timed_legs["string_gather"] = lambda: gather(g_bytes, total_bytes)
    if a.trace_legs:
        for name, fn in timed_legs.items():
            for _ in range(a.trace_legs):
                fn()
            torch.cuda.synchronize()
        print(json.dumps({"traced": list(timed_legs), "calls_each": a.trace_legs, "counts": counts}))
        return

    # the least bytes a leg must move: per live cell 9 read and 8.125 (counting: 0.125) written, and the bytes of its strings
    kept_string_bytes = [sum(len(texts[col][r]) for r in kept_rows.tolist() if texts[col][r] is not None) for col in range(2)]
    least = {}
    for name, (fields, t, v, rc, with_data) in legs.items():
        sbytes = sum((kept_string_bytes if rc is not None else string_bytes)[f[0]] for f in fields)
        least[name] = int(live_of[name] * len(fields) * (9 + (8.125 if with_data else 0.125)) + sbytes)
    src = torch.zeros(max(least.values()) // 16 + 1, dtype=torch.int64, device=dev)
    dst = torch.empty_like(src)
    for name in legs:
        timed_legs[name + "_copy"] = lambda name=name: dst[:least[name] // 16].copy_(src[:least[name] // 16])
    res = {"documents": n, "input_bytes": int(offs[-1]), "paths": POINTERS, "columns": n_cols, "device": torch.cuda.get_device_name(0), "unit": "us",
           "strings": strings, "string_bytes": string_bytes, "counts": counts, "least_bytes_moved": least,
           "verified": "every leg: the records equal the Python reference's verdicts on all rows; validity bits and data words equal the "
                       "reference's on a sample of %d rows; nothing written behind the live rows" % a.sample}
    res.update(opbench.measure(timed_legs, a.steps, a.warmup))
    for name in legs:
        res[name + "_over_copy"] = res[name]["median_ms"] / res[name + "_copy"]["median_ms"]
    res["one_field_over_string_gather"] = res["one_field"]["median_ms"] / res["string_gather"]["median_ms"]
    ab = os.path.join(ROOT, "tools", "ubench", "timecol_ab")
    if not a.no_ab and os.path.exists(ab):
        torch.cuda.synchronize()
        done = subprocess.run([ab, str(n), str(a.steps)], stdout=subprocess.PIPE, timeout=300)  # (a child of its own: it opens the GPU itself)
        if done.returncode != 0:
            raise SystemExit("tools/ubench/timecol_ab failed with %d" % done.returncode)
        res["fetch_ab"] = json.loads(done.stdout.decode().strip().splitlines()[-1])
    opbench.write(a.out, res)
    plan.close()
    select.close()
    ctx.close()


if __name__ == "__main__":
    main()
