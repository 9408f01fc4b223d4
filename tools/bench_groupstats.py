"""What group statistics per dictionary key cost on the device -> profiles/r24/groupstats.json, everything from ONE process on one
box (boxes differ by several per cent: only numbers of the same run are compared).  --rows rows, 80 % of them valid, at every
--keys key count (default 8, SJMI_GROUP_LDS_KEYS, SJMI_GROUP_LDS_KEYS + 1 and 2^18), with uniform keys and with all rows in one key,
over an all-long value column and one that is half doubles.  Every leg is verified before it is timed, the legs of a
configuration are interleaved by tools/opbench.py, and every leg's spread is in its record:

  group_stats  sjmi_group_stats_device; verified against tests/groupstats_common.expected_large (every integer word equal,
               sum_double within the derived bound)
  read_only    the floor: torch reductions that only read the same 13 bytes a row (index, type byte, value word) plus the bitmap
               words -- the census's yardstick with the value column added
  torch_route  the route a user has today: boolean masks, torch.bincount, index_add_ and scatter_reduce_ (amin / amax) calls that
               give the same ten outputs per key, the int64 sums wrapping; it is GIVEN the validity as a bool tensor (it would
               have to unpack the bitmap first).  Verified against group_stats: counts, minima and maxima equal, its wrapped sum
               equal to sum_long_lo.  Where one execution takes more than 150 ms (all rows in one key) it is timed three times by
               the wall clock and left out of the interleaved rounds; more than 3 s, and that one execution is its figure
  census       sjmi_key_census_device on the same indices and type bytes: the same-box sanity leg
SJMI_LIB=<a variant built by tools/build_variant.sh> measures that library instead (the wave combine against plain atomics:
profiles/r24/README.md).  No figure is a pass mark.
  python tools/bench_groupstats.py [--rows N] [--keys a,b,..] [--steps K] [--warmup W] [--values a,b] [--out PATH]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALUES = ("all_long", "half_double")
MAX_KEYS = 1 << 20
SLOW_ROUTE_MS = 150.0  # a torch route slower than this is timed three times by the wall clock, outside the interleaved rounds


def torch_route(torch, ix, valid, ty, val, n_keys):
    """-> (n_long, n_double, n_other, sum_long (wrapping), sum_double, min_long, max_long, min_double, max_double), tensors [n_keys]"""
    idx = ix.long()
    is_l, is_d = valid & (ty == ord("l")), valid & (ty == ord("d"))
    kl, kd, ko = idx[is_l], idx[is_d], idx[valid & ~is_l & ~is_d]
    vl, vd = val[is_l], val.view(torch.float64)[is_d]
    new = lambda fill, dtype: torch.full((n_keys,), fill, dtype=dtype, device=ix.device)
    return (torch.bincount(kl, minlength=n_keys), torch.bincount(kd, minlength=n_keys), torch.bincount(ko, minlength=n_keys),
            new(0, torch.int64).index_add_(0, kl, vl), new(0.0, torch.float64).index_add_(0, kd, vd),
            new((1 << 63) - 1, torch.int64).scatter_reduce_(0, kl, vl, "amin"), new(-(1 << 63), torch.int64).scatter_reduce_(0, kl, vl, "amax"),
            new(float("inf"), torch.float64).scatter_reduce_(0, kd, vd, "amin"), new(float("-inf"), torch.float64).scatter_reduce_(0, kd, vd, "amax"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8 << 20)
    ap.add_argument("--keys", default="")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--values", default=",".join(VALUES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "groupstats.json"))
    a = ap.parse_args(argv)
    values = [s for s in a.values.split(",") if s]
    if a.rows < 1 or a.rows >= 1 << 32 or a.steps < 1 or a.warmup < 0:
        ap.error("--rows must be in [1, 2^32), --steps >= 1, --warmup >= 0")
    if not values or any(s not in VALUES for s in values):
        ap.error("--values: a list of " + ", ".join(VALUES))
    try:
        keys = [int(s) for s in a.keys.split(",") if s]
    except ValueError:
        keys = [0]
    if any(not 1 <= k <= MAX_KEYS for k in keys):
        ap.error("--keys: a list of key counts in [1, 2^20]")
    import torch
    from tests import groupstats_common as GC
    from tests.members_common import header_constant
    from tools import opbench
    lds_keys = header_constant("SJMI_GROUP_LDS_KEYS")
    keys = keys or [8, lds_keys, lds_keys + 1, 1 << 18]
    dev, ctx, stream = opbench.device()
    res = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "lds_keys": lds_keys, "library": os.environ.get("SJMI_LIB") or "libsjmi.so",
           "configurations": []}
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    for vkind in values:
        ty, va = GC.value_column(a.rows, 24, vkind)
        d_ty, d_va = up(ty), up(va)
        for n_keys in keys:
            for kind in ("uniform", "one_bin"):
                ix, words, bits = GC.keys_column(a.rows, n_keys, 24 + n_keys, kind)
                d_ix, d_words, d_valid = up(ix), up(words), up(bits)
                stats = torch.empty((n_keys, 10), dtype=torch.int64, device=dev)
                record = torch.empty(5, dtype=torch.int64, device=dev)
                counts = torch.empty((n_keys, 8), dtype=torch.int64, device=dev)
                crecord = torch.empty(4, dtype=torch.int64, device=dev)
                call = lambda: ctx.group_stats_device(d_ix.data_ptr(), d_words.data_ptr(), d_ty.data_ptr(), d_va.data_ptr(), a.rows, 0, n_keys,
                                                      stats.data_ptr(), record.data_ptr(), stream)
                census = lambda: ctx.key_census_device(d_ix.data_ptr(), d_words.data_ptr(), d_ty.data_ptr(), a.rows, 0, n_keys, counts.data_ptr(),
                                                       crecord.data_ptr(), stream)
                route = lambda: torch_route(torch, d_ix, d_valid, d_ty, d_va, n_keys)
                say = lambda text: print("%s, %d keys, %s: %s" % (vkind, n_keys, kind, text), file=sys.stderr, flush=True)
                call()
                census()
                torch.cuda.synchronize()
                say("called")
                t0 = time.perf_counter()
                theirs = [t.cpu().numpy() for t in route()]
                torch.cuda.synchronize()
                route_ms = (time.perf_counter() - t0) * 1e3
                got = stats.cpu().numpy().view(np.uint64)
                want, sums = GC.expected_large(ix, bits, ty, va, n_keys, a.rows)
                GC.check_stats(got, want, what="%s, %d keys, %s" % (vkind, n_keys, kind))
                assert record.cpu().tolist() == [a.rows, *sums, 0]
                for word, their in zip((0, 1, 2, 3, 6, 7), (theirs[0], theirs[1], theirs[2], theirs[3], theirs[5], theirs[6])):
                    assert (got[:, word] == their.astype(np.int64).view(np.uint64)).all(), (word, n_keys, kind)
                assert (got[:, 8].view(np.float64) == theirs[7]).all() and (got[:, 9].view(np.float64) == theirs[8]).all()
                assert int(counts.sum().cpu()) == sums[0] and (counts[:, 0].cpu().numpy() == got[:, 0].view(np.int64)).all()
                say("verified; the torch route's first execution took %.1f ms" % route_ms)
                legs = {"group_stats": call, "read_only": lambda: (d_ix.sum(), d_ty.sum(), d_va.sum(), d_words.sum()), "census": census}
                out = {"values": vkind, "n_keys": n_keys, "rows_in": kind, "path": "lds" if n_keys <= lds_keys else "global"}
                if route_ms <= SLOW_ROUTE_MS:
                    legs["torch_route"] = route
                else:  # (its scatter calls queue on one address: not worth dozens of executions; two more, by the wall clock)
                    ms = sorted([route_ms] + (opbench.wall(route, 2) if route_ms <= 20 * SLOW_ROUTE_MS else []))  # (seconds: the one execution)
                    out["torch_route"] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "steps": len(ms), "clock": "wall, not interleaved"}
                out.update(opbench.measure(legs, a.steps, a.warmup, third=("torch_route",)))
                for name in ("read_only", "torch_route", "census"):
                    out["group_stats_over_" + name] = out["group_stats"]["median_ms"] / out[name]["median_ms"]
                res["configurations"].append(out)
                say("group_stats %.3f ms, read_only %.3f ms, torch_route %.3f ms, census %.3f ms" % tuple(
                    out[n]["median_ms"] for n in ("group_stats", "read_only", "torch_route", "census")))
    opbench.write(a.out, res)
    ctx.close()


if __name__ == "__main__":
    main()
