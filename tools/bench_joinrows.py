"""What an inner join of two row sets on a long key costs on the device -> profiles/r32/joinrows.json, everything from ONE process
on one box (boxes differ by several per cent: only numbers of the same run are compared).  For every --rows count of LEFT rows
(default 1 Mi and 8 Mi), 95 % of the rows of both sides candidates, every --cases case:

  dim64k_100 / dim64k_10   a unique-key build side of 64 Ki rows (a dimension table), 100 % / 10 % of the left candidates match
  dim1m_100 / dim1m_10     the same with 1 Mi build rows
  zipf                     m x n: both sides draw 2^16 keys with p(k) ~ k^-1/2, 90 Ki build rows: about 4 pairs a left row
  carried                  dim64k_100 with 4 carried columns a side

Every leg is verified before it is timed, the legs of a configuration are interleaved by tools/opbench.py, and every leg's spread
is in its record:

  join_rows    sjmi_join_rows_device alone, the sorted right side given (build once, probe many); verified against
               tests/joinrows_common.expected_by_searchsorted (pairs, carried cells, offsets and record equal)
  sort_join    sjmi_sort_rows_device on the right key, then the join
  torch_route  the route a user has today: masks for the classes, torch.sort(stable=True) of the right candidates, two
               torch.searchsorted, repeat_interleave, index arithmetic, index_select of the carried columns; its .item() for the
               output size is timed, because the route needs it.  Verified against the same reference, pairs included
  pair_copy    a device copy of the 16 bytes a pair that any join must write
No figure is a pass mark.
  python tools/bench_joinrows.py [--rows a,b] [--cases a,b] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("dim64k_100", "dim64k_10", "dim1m_100", "dim1m_10", "zipf", "carried")
ZIPF_KEYS, ZIPF_BUILD = 1 << 16, 90 << 10


def _typed(keys, rng):
    """int64 keys -> (types uint8, values uint64): a twentieth of the cells nulls and strings over poison"""
    types = np.full(keys.size, ord("l"), dtype=np.uint8)
    dead = rng.random(keys.size) < 0.05
    types[dead] = rng.choice(np.frombuffer(b'n"', dtype=np.uint8), int(dead.sum()))
    values = keys.astype(np.int64).view(np.uint64).copy()
    values[dead] = 0x7FF8DEADBEEF0001
    return types, values


def bench_sides(n_left, case, seed=32, scale=1):
    """-> ((left types, left values), (right types, right values), carried columns a side).  scale divides the build sizes (tests)"""
    rng = np.random.default_rng(seed)
    if case == "zipf":
        p = np.arange(1, ZIPF_KEYS // scale + 1, dtype=np.float64) ** -0.5
        cdf = np.cumsum(p / p.sum())
        draw = lambda n: np.minimum(np.searchsorted(cdf, rng.random(n)), cdf.size - 1).astype(np.int64) * 7919 - 5
        return _typed(draw(n_left), rng), _typed(draw(ZIPF_BUILD // scale), rng), 0
    n_build = (1 << 20 if case.startswith("dim1m") else 1 << 16) // scale
    rate = 10 if case.endswith("_10") else 1
    build = rng.permutation(n_build).astype(np.int64) * 3 - n_build  # (unique, negative ones among them)
    left = rng.integers(0, n_build * rate, n_left, dtype=np.int64) * 3 - n_build
    return _typed(left, rng), _typed(build, rng), 4 if case == "carried" else 0


def torch_route(torch, lt, lv, rt, rv, l_cells=None, r_cells=None):
    """an inner join on (types uint8, values int64) key columns -> (left_rows, right_rows, left cells, right cells)"""
    ridx = (rt == ord("l")).nonzero().squeeze(1)
    rk, perm = torch.sort(rv[ridx], stable=True)
    order = ridx[perm]
    lidx = (lt == ord("l")).nonzero().squeeze(1)
    lk = lv[lidx]
    lo = torch.searchsorted(rk, lk, right=False)
    m = torch.searchsorted(rk, lk, right=True) - lo
    total = int(m.sum().item())  # (the size of the output is a device value)
    left_rows = torch.repeat_interleave(lidx, m, output_size=total)
    first = torch.repeat_interleave(lo - (torch.cumsum(m, 0) - m), m, output_size=total)  # lo[p] - off[p]
    right_rows = order[first + torch.arange(total, device=lt.device)]
    return (left_rows, right_rows, None if l_cells is None else l_cells.index_select(1, left_rows),
            None if r_cells is None else r_cells.index_select(1, right_rows))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="%d,%d" % (1 << 20, 8 << 20))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32", "joinrows.json"))
    a = ap.parse_args(argv)
    cases = [s for s in a.cases.split(",") if s]
    try:
        row_counts = [int(s) for s in a.rows.split(",") if s]
    except ValueError:
        row_counts = []
    if not row_counts or any(not 1 <= n < 1 << 32 for n in row_counts) or a.steps < 1 or a.warmup < 0:
        ap.error("--rows: a list of counts in [1, 2^32), --steps >= 1, --warmup >= 0")
    if not cases or any(s not in CASES for s in cases):
        ap.error("--cases: a list of " + ", ".join(CASES))
    import torch
    from tests import joinrows_common as JO
    from tests import toprows_common as TC
    from tools import opbench
    dev, ctx, stream = opbench.device()
    res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SJMI_LIB") or "libsjmi.so", "configurations": []}
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    for n in row_counts:
        for case in cases:
            (lt, lv), (rt, rv), n_cols = bench_sides(n, case)
            n_r = rt.size
            lref = JO.left_classes(lt, None, lv, None, n, n)
            order, sort_record, build_keys = JO.build_set(rt, None, rv)
            want_l, want_r, want_off, want = JO.expected_by_searchsorted(JO.INNER, lref, order, sort_record[1], build_keys)
            n_pairs = want[2]
            carry = [TC.carried(n_cols, rows, rows, 32 + k) if n_cols else None for k, rows in enumerate((n, n_r))]
            d_lt, d_lv, d_rt, d_rv = up(lt), up(lv), up(rt), up(rv)
            d_carry = [(up(c[0]), up(c[1])) if c else None for c in carry]
            side = lambda t, v, rows, c: (t.data_ptr(), 0, v.data_ptr(), rows, c[0].data_ptr() if c else 0, c[1].data_ptr() if c else 0, n_cols,
                                          rows if c else 0)
            ls, rs = side(d_lt, d_lv, n, d_carry[0]), side(d_rt, d_rv, n_r, d_carry[1])
            d_order, d_rec = torch.empty(n_r, dtype=torch.int64, device=dev), torch.empty(9, dtype=torch.int64, device=dev)
            out = [torch.empty(n_pairs, dtype=torch.int64, device=dev) for _ in range(2)]
            cells = [(torch.empty((n_cols, n_pairs), dtype=torch.uint8, device=dev), torch.empty((n_cols, n_pairs), dtype=torch.int64, device=dev))
                     for _ in range(2)]
            off, rec = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(9, dtype=torch.int64, device=dev)
            cp = lambda t: t.data_ptr() if n_cols and n_pairs else 0

            def sort():
                ctx.sort_rows_device(d_rt.data_ptr(), 0, d_rv.data_ptr(), n_r, 0, n_r, 0, TC.LONG, 0, 0, 0, 0, 0, d_order.data_ptr(), 0, 0, 0,
                                     d_rec.data_ptr(), stream)

            def join():
                ctx.join_rows_device(ls, 0, n, 0, rs, d_order.data_ptr(), n_r, d_rec.data_ptr(), JO.INNER, n_pairs, out[0].data_ptr(), out[1].data_ptr(),
                                     cp(cells[0][0]), cp(cells[0][1]), cp(cells[1][0]), cp(cells[1][1]), n_pairs if n_cols else 0, off.data_ptr(),
                                     rec.data_ptr(), stream)

            route = lambda: torch_route(torch, d_lt, d_lv, d_rt, d_rv, d_carry[0][1] if n_cols else None, d_carry[1][1] if n_cols else None)
            sort()
            join()
            torch.cuda.synchronize()
            same = lambda t, want: (t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint8) == want).all()
            assert d_rec.cpu().tolist() == sort_record and same(d_order[:sort_record[1]], order[:sort_record[1]])
            assert rec.cpu().tolist() == want and same(out[0], want_l) and same(out[1], want_r) and same(off, want_off)
            theirs = route()
            assert same(theirs[0], want_l) and same(theirs[1], want_r)
            for k, (c, rows, n_source) in enumerate(((carry[0], want_l, n), (carry[1], want_r, n_r))):
                if c:
                    ct, cv = JO.carried_cells(c, rows, n_source)
                    assert same(cells[k][0], ct) and same(cells[k][1], cv) and same(theirs[2 + k], cv)
            moved, landed = torch.empty(16 * n_pairs, dtype=torch.uint8, device=dev), torch.empty(16 * n_pairs, dtype=torch.uint8, device=dev)
            cfg = {"rows": n, "case": case, "build_rows": n_r, "n_build": want[1], "n_pairs": n_pairs, "pairs_per_left_row": n_pairs / n,
                   "n_matched": want[3], "carried_columns": n_cols}
            cfg.update(opbench.measure({"join_rows": join, "sort_join": lambda: (sort(), join()), "torch_route": route,
                                        "pair_copy": lambda: landed.copy_(moved)}, a.steps, a.warmup, third=("torch_route",)))
            for name in ("torch_route", "pair_copy"):
                cfg["join_rows_over_" + name] = cfg["join_rows"]["median_ms"] / cfg[name]["median_ms"]
            cfg["sort_join_over_torch_route"] = cfg["sort_join"]["median_ms"] / cfg["torch_route"]["median_ms"]
            res["configurations"].append(cfg)
            print("%d rows, %s (%d pairs): join_rows %.3f ms, sort_join %.3f ms, torch_route %.3f ms, pair_copy %.3f ms" % (
                n, case, n_pairs, cfg["join_rows"]["median_ms"], cfg["sort_join"]["median_ms"], cfg["torch_route"]["median_ms"],
                cfg["pair_copy"]["median_ms"]), file=sys.stderr, flush=True)
            del out, cells, moved, landed, theirs
    opbench.write(a.out, res)
    ctx.close()


if __name__ == "__main__":
    main()
