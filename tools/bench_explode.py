"""What exploding one array of every parsed document into rows costs on the device -> profiles/r9/explode.json, everything from
ONE process on one box (boxes differ by several per cent: only numbers of the same run are compared).

Workloads:
  configs   the configs[3] batch (1,000,000 unique documents, tools/docgen.c); base "/k2" -- a field that is an array of up to
            eight small integers in one document in ten -- and the element pointer "" (the elements are scalars);
  statuses  chunks of twitter.json's statuses reserialised as {"statuses":[...]}, replicated to about 1 GB; base "/statuses"
            and 12 element pointers;
  wide      100,000 small documents of ten elements each, and the same batch with ONE document of 100,000 elements added:
            one group walks all elements of its document, so the second batch shows what a wide array among small ones costs.
The columns are first verified against tests/explode_common.py (the oracle's tapes read by the oracle's walk).  Then, per
workload, interleaved, medians of event-timed single executions:
  explode_count   sjmi_explode_batch_device with row_capacity 0 (k_explode_count + the scan);
  explode         the full call (count, scan, k_explode_rows);
  select          k_select with a 12-path plan on the same batch: the per-document yardstick;
  read            a read-only torch pass over exactly the tape words and string-record bytes the batch made;
  d2h             the copy of those bytes into pinned memory -- what a caller without explode has to do.
  python tools/bench_explode.py [--workloads configs,statuses,wide] [--docs N] [--bytes B] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS_BASE, CONFIGS_POINTERS = "/k2", [""]
CONFIGS_SELECT = ["/k0", "/k1", "/k3/x", "/k3/y", "/k5/0", "/k2/7", "/z", "/k12", "/k20/y", "/k4/3", "/nope", "/k7"]
VERIFY_DOCS = 20000
CHUNK = 10  # statuses per document of the `statuses` workload


class Batch:
    """a parsed batch on the device, and an explode of it"""

    def __init__(self, torch, ctx, stream, shard, c):
        self.torch, self.ctx, self.shard, self.c, self.stream = torch, ctx, shard, c, stream
        self.sb_bytes, self.tape_bytes = int(self.c["string_bytes"]), 8 * int(self.c["tape_words"])

    def explode(self, plan, capacity):
        return self.shard.explode(plan, capacity, self.stream)

    def legs(self, plan, total, select_plan):
        sh, torch = self.shard, self.torch
        tape_view, sb_view = sh.tape[:self.tape_bytes // 8], sh.sb[:self.sb_bytes // 8 * 8].view(torch.int64)
        host_tape = torch.empty(self.tape_bytes // 8, dtype=torch.int64).pin_memory()
        host_sb = torch.empty(self.sb_bytes, dtype=torch.uint8).pin_memory()
        self.explode(plan, total)  # (the columns are allocated here, not inside a timed call)
        offs0 = torch.zeros(sh.n_docs + 1, dtype=torch.int64, device=sh.device)
        count_only = lambda: self.ctx.explode_batch_device(plan, sh.tape.data_ptr(), sh.tape_offsets.data_ptr(), sh.doc_errors.data_ptr(),
                                                           sh.sb.data_ptr(), sh.n_docs, offs0.data_ptr(), 0, 0, 0, self.stream)
        return {"explode_count": count_only, "explode": lambda: self.explode(plan, total), "select": lambda: sh.select(select_plan, self.stream),
                "read": lambda: (tape_view.sum(), sb_view.sum()),
                "d2h": lambda: (host_tape.copy_(tape_view, non_blocking=True), host_sb.copy_(sh.sb[:self.sb_bytes], non_blocking=True))}


def summarise(res, rows):
    ex = res["explode"]["median_ms"]
    res["rows"] = rows
    res["explode_over_select"] = ex / res["select"]["median_ms"]
    res["explode_over_read"] = ex / res["read"]["median_ms"]
    res["d2h_over_explode"] = res["d2h"]["median_ms"] / ex
    res["ns_per_row"] = ex * 1e6 / max(rows, 1)
    res["count_and_scan_share"] = res["explode_count"]["median_ms"] / ex
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="configs,statuses,wide")
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "explode.json"))
    a = ap.parse_args()
    import torch
    import simdjson_java_amd as S
    from oracle import oracle as O
    from tests import explode_common as EC
    from tests import select_common as SC
    from tools import opbench
    O.build()
    dev, ctx, stream = opbench.device()

    out = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SJMI_LIB") or "libsjmi.so"}
    todo = a.workloads.split(",")

    if "configs" in todo:
        data, offs, shard, c = opbench.configs_shard(ctx, dev, stream, a.docs)
        b = Batch(torch, ctx, stream, shard, c)
        plan, sel = S.ExplodePlan(CONFIGS_BASE, CONFIGS_POINTERS), S.SelectPlan(CONFIGS_SELECT)
        ro, _, _ = b.explode(plan, 0)
        torch.cuda.synchronize()
        total = int(ro[-1].item())
        ro, types, values = b.explode(plan, total)
        torch.cuda.synchronize()
        nv = min(VERIFY_DOCS, a.docs)
        parsed = [O.parse(bytes(data[int(offs[k]):int(offs[k + 1]) - 1])) for k in range(nv)]
        want_offs, want = EC.expected_explode(parsed, CONFIGS_BASE, CONFIGS_POINTERS)
        got_offs = ro[:nv + 1].cpu().numpy()
        assert [int(x) for x in got_offs] == want_offs
        n = want_offs[-1]
        present = SC.check_columns(types[:, :n].cpu().numpy(), values[:, :n].cpu().numpy().view(np.uint64), bytes(b.shard.sb[:b.sb_bytes].cpu().numpy()),
                                   want, "bench configs")
        res = {"documents": a.docs, "input_bytes": int(offs[-1]), "base": CONFIGS_BASE, "element_pointers": CONFIGS_POINTERS,
               "verified_documents": nv, "verified_rows": n, "verified_present": int(present), "tape_bytes": b.tape_bytes,
               "string_record_bytes": b.sb_bytes}
        res.update(opbench.measure(b.legs(plan, total, sel), a.steps, a.warmup, third={"d2h"}))
        out["configs"] = summarise(res, total)
        plan.close()
        sel.close()
        del b

    if "statuses" in todo:
        chunks = SC.reserialised("twitter.json", lambda d: [{"statuses": d["statuses"][i:i + CHUNK]} for i in range(0, len(d["statuses"]), CHUNK)])
        ptrs = SC.TWITTER_POINTERS[:12]
        unit = b"".join(c + b"\n" for c in chunks)
        reps = max(1, a.bytes // len(unit))
        lens = np.tile(np.array([len(c) + 1 for c in chunks], dtype=np.uint64), reps)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        data = np.tile(np.frombuffer(unit, dtype=np.uint8), reps)
        b = Batch(torch, ctx, stream, *opbench.parsed_shard(ctx, dev, stream, data, offs, **opbench.RATIOS))
        plan = S.ExplodePlan("/statuses", ptrs)
        sel = S.SelectPlan(["/statuses/0" + p for p in ptrs])
        parsed = [O.parse(c) for c in chunks]
        want_offs, want = EC.expected_explode(parsed, "/statuses", ptrs)
        per = want_offs[-1]
        total = per * reps
        ro, types, values = b.explode(plan, total)
        torch.cuda.synchronize()
        assert int(ro[-1].item()) == total and (np.diff(ro.cpu().numpy()) == np.tile(np.diff(want_offs), reps)).all()
        first_sb = bytes(b.shard.sb[:min(b.sb_bytes, 64 << 20)].cpu().numpy())
        present = SC.check_columns(types[:, :per].cpu().numpy(), values[:, :per].cpu().numpy().view(np.uint64), first_sb, want, "bench statuses")
        # the other copies: the same types, the same plain values, the same string lengths (their records lie elsewhere)
        t = types.cpu().numpy().reshape(len(ptrs), reps, per)
        v = values.cpu().numpy().view(np.uint64).reshape(len(ptrs), reps, per)
        assert (t == t[:, :1, :]).all()
        is_str = t == ord('"')
        assert (np.where(is_str, v >> np.uint64(32), v) == np.where(is_str[:, :1, :], v[:, :1, :] >> np.uint64(32), v[:, :1, :])).all()
        res = {"documents": len(chunks) * reps, "statuses_per_document": CHUNK, "input_bytes": int(offs[-1]), "base": "/statuses", "element_pointers": ptrs,
               "verified_rows": total, "verified_present_per_copy": int(present), "tape_bytes": b.tape_bytes, "string_record_bytes": b.sb_bytes,
               "tape_words_per_document": b.tape_bytes // 8 // (len(chunks) * reps)}
        res.update(opbench.measure(b.legs(plan, total, sel), a.steps, a.warmup, third={"d2h"}))
        out["statuses"] = summarise(res, total)
        plan.close()
        sel.close()
        del b, data, t, v

    if "wide" in todo:
        small = [b'{"id":%d,"arr":[%s]}' % (k, b",".join(b'{"a":%d,"s":"v%d"}' % (k + j, j) for j in range(10))) for k in range(100000)]
        wide = b'{"id":-1,"arr":[%s]}' % b",".join(b'{"a":%d,"s":"v%d"}' % (j, j % 10) for j in range(100000))
        ptrs = ["/a", "/s", ""]
        plan = S.ExplodePlan("/arr", ptrs)
        res = {"small_documents": len(small), "elements_per_small_document": 10, "elements_of_the_wide_document": 100000, "element_pointers": ptrs}
        for name, docs in (("small_only", small), ("with_one_wide", small[:50000] + [wide] + small[50000:])):
            blob = b"".join(d + b"\n" for d in docs)
            offs = np.concatenate([[0], np.cumsum([len(d) + 1 for d in docs])]).astype(np.uint64)
            b = Batch(torch, ctx, stream, *opbench.parsed_shard(ctx, dev, stream, blob, offs))
            ro, _, _ = b.explode(plan, 0)
            torch.cuda.synchronize()
            total = int(ro[-1].item())
            assert total == 10 * len(small) + (100000 if len(docs) > len(small) else 0)
            ro, types, values = b.explode(plan, total)
            torch.cuda.synchronize()
            at = 500000 if len(docs) > len(small) else 0  # the wide document's rows (or the first ones), against the oracle
            nv = 100000 if at else 1000
            parsed = [O.parse(docs[50000])] if at else [O.parse(d) for d in docs[:100]]
            want_offs, want = EC.expected_explode(parsed, "/arr", ptrs)
            assert want_offs[-1] == nv
            tcpu, vcpu = types[:, at:at + nv].cpu().numpy(), values[:, at:at + nv].cpu().numpy().view(np.uint64)
            for p, col in enumerate(want):
                assert (tcpu[p] == np.array([c[0] for c in col], dtype=np.uint8)).all()
                plain = np.array([c[0] != ord('"') for c in col])
                assert (vcpu[p][plain] == np.array([c[1] for c in col if c[0] != ord('"')], dtype=np.uint64)).all()
                assert ((vcpu[p][~plain] >> np.uint64(32)) == np.array([len(c[1]) for c in col if c[0] == ord('"')], dtype=np.uint64)).all()
            ms = opbench.timed(lambda: b.explode(plan, total), a.steps, a.warmup)
            res[name] = {"rows": total, "median_ms": statistics.median(ms), "min_ms": min(ms), "steps": len(ms)}
            del b
        extra = res["with_one_wide"]["median_ms"] - res["small_only"]["median_ms"]
        res["wide_document_extra_ms"] = extra
        res["wide_document_ns_per_row"] = extra * 1e6 / 100000
        res["small_only_ns_per_row"] = res["small_only"]["median_ms"] * 1e6 / res["small_only"]["rows"]
        out["wide"] = res
        plan.close()

    opbench.write(a.out, out)
    ctx.close()


if __name__ == "__main__":
    main()
