"""The row filter on the GPU (sjmi_filter_columns_device through Context.filter_columns_device and BatchShard.filter): the keep
words, the selection vector, every compacted cell below the capacity and the result record against the Python reference of
tests/filter_common.py, and canaries behind everything the call owns.  Synthetic column sets carry wild value words in the cells
that are neither strings nor numbers; the end-to-end tests take their expected cells from tests/select_common.py and
tests/explode_common.py over the oracle's parse, filtered by the reference."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import explode_common as EC
from tests import filter_common as FC
from tests import select_common as SEL
from tests import strcol_common as SC
from tests.test_gpu_batch import _pack
from tests.test_gpu_strcol import STAGE2_FAILS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 4 << 20)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def side_stream():
    """torch's work and the engine's kernels on ONE stream of their own: handle 0 names the context's stream in the C ABI, so
    torch's default stream cannot carry both"""
    import torch
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    with torch.cuda.stream(side):
        yield side.cuda_stream
    torch.cuda.synchronize()


def run(ctx, stream, case, capacity, keep=True, outs=True, type_shift=0):
    """one call into out_buffers() on the device; the type columns, the compacted types and the string buffer are slices of
    larger tensors"""
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    n_cols, stride = case.types.shape
    cells = n_cols * stride
    tstore = torch.zeros(cells + 16, dtype=torch.uint8, device=dev)
    d_types = tstore[type_shift:type_shift + cells]
    d_types.copy_(torch.from_numpy(np.ascontiguousarray(case.types, dtype=np.uint8).reshape(-1)))
    d_values = torch.from_numpy(np.ascontiguousarray(case.values, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev)
    sbstore = torch.zeros(case.sb.size + 16, dtype=torch.uint8, device=dev)
    d_sb = sbstore[5:5 + case.sb.size]
    d_sb.copy_(torch.from_numpy(np.array(case.sb, dtype=np.uint8)))
    words, rows, otypes, ovalues, res = FC.out_buffers(case.n_rows, n_cols, capacity, keep, outs)
    d_words = torch.from_numpy(words.view(np.int64)).to(dev) if keep else None
    d_res = torch.from_numpy(res.view(np.int64)).to(dev)
    if outs:
        d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
        oshift = (type_shift + 5) % 16
        ostore = torch.full((otypes.size + 16,), FC.CANARY, dtype=torch.uint8, device=dev)
        d_ot = ostore[oshift:oshift + otypes.size]
        d_ov = torch.from_numpy(ovalues.view(np.int64)).to(dev)
    plan = S.FilterPlan(case.terms)
    ctx.filter_columns_device(plan, d_types.data_ptr(), d_values.data_ptr(), n_cols, stride, case.n_rows, d_sb.data_ptr(),
                              d_words.data_ptr() if keep else 0, d_rows.data_ptr() if outs else 0, capacity, d_ot.data_ptr() if outs else 0,
                              d_ov.data_ptr() if outs else 0, d_res.data_ptr(), stream)
    torch.cuda.synchronize()
    plan.close()
    if not outs:
        return d_words.cpu().numpy() if keep else None, None, None, None, d_res.cpu().numpy()
    assert bool((ostore[:oshift] == FC.CANARY).all()) and bool((ostore[oshift + otypes.size:] == FC.CANARY).all()), "written in front of d_out_types"
    return d_words.cpu().numpy() if keep else None, d_rows.cpu().numpy(), d_ot.cpu().numpy(), d_ov.cpu().numpy(), d_res.cpu().numpy()


def check_all(ctx, stream, case, caps=None, keep=None):
    """the case at every capacity (caps=None) or at those given (None among them: n_kept), each optional output left out in turn"""
    keep = FC.reference(case) if keep is None else keep
    n_kept = int(keep.sum())
    for k, capacity in enumerate(FC.capacities(n_kept) if caps is None else [n_kept if c is None else c for c in caps]):
        got = run(ctx, stream, case, capacity, keep=k % 3 != 1, outs=capacity > 0 or k % 2 == 0, type_shift=(3 * k + 1) % 16)
        FC.check("%s, capacity %d of %d" % (case.name, capacity, n_kept), *got, case, keep, capacity)
    return n_kept


@pytest.mark.parametrize("n", FC.ROW_COUNTS)
def test_row_counts_and_capacities(ctx, side_stream, n):
    case = FC.row_count_case(n)
    n_kept = check_all(ctx, side_stream, case)
    assert n < 63 or 0 < n_kept < n


def test_keep_patterns(ctx, side_stream):
    for case in FC.keep_pattern_cases():
        check_all(ctx, side_stream, case)


def test_every_op_on_a_cell_of_every_type(ctx, side_stream):
    kept = {}
    for case in FC.op_table_cases():
        op = case.terms[0][1]
        kept[op] = kept.get(op, 0) + check_all(ctx, side_stream, case, caps=(None,))
    assert sorted(kept) == sorted(FC.ALL_OPS) and all(kept.values()), kept  # every op is true somewhere


def test_numeric_edges(ctx, side_stream):
    kept = sum(check_all(ctx, side_stream, case, caps=(None, 1)) for case in FC.numeric_edge_cases())
    assert kept > 1000


def test_string_edges(ctx, side_stream):
    kept = sum(check_all(ctx, side_stream, case, caps=(None,)) for case in FC.string_edge_cases())
    # per length and alignment EQ keeps 2 cells, NE 4 and PREFIX 3; with the empty constant 2, 1 and 3
    assert kept == 16 * (6 * 9 + 6)


def test_layouts(ctx, side_stream):
    for case in FC.layout_cases():
        n_kept = check_all(ctx, side_stream, case)
        assert case.terms == [] or 0 < n_kept < case.n_rows, case.name


def test_a_plan_of_sixteen_terms_with_long_constants(ctx, side_stream):
    """the largest launch argument: sixteen terms and 1024 bytes of constants, three of them 256 bytes long"""
    rng = np.random.default_rng(77)
    consts = [bytes(rng.integers(97, 99, size=256, dtype=np.uint8)) for _ in range(4)]
    n = 300
    buf = b"".join(consts) + consts[0][:255] + b"c"
    types = np.full((4, n + 3), FC.STRING, dtype=np.uint8)
    values = np.array([[(256 << 32) | (256 * (k if rng.random() < 0.6 else int(rng.integers(0, 5)))) for _ in range(n + 3)] for k in range(4)], dtype=np.uint64)
    terms = [(k, "string_ne", consts[(k + 1) % 4]) for k in range(3)] + [(k % 4, "string_prefix", consts[k % 4][:19]) for k in range(12)] + \
        [(3, "string_prefix", consts[3][:28])]
    assert len(terms) == 16 and sum(len(t[2]) for t in terms) == 1024
    case = FC.Case("sixteen terms", terms, types, values, n, np.frombuffer(buf, dtype=np.uint8))
    assert 0 < check_all(ctx, side_stream, case) < n


def test_the_chunk_scan_takes_a_second_slice(ctx, side_stream):
    """1024 * 1024 + 1 rows: chunk 1024 is the first of the one-workgroup scan's second slice; one LONG_GT term on 'l', 'd' and
    other cells, against the vectorised reference (like compared with like), at the capacities n_kept and 0"""
    n = 1024 * 1024 + 1
    rng = np.random.default_rng(31)
    t, v = FC.columns(rng, 2, n, n + 3, 64)
    t[1, n - 1], v[1, n - 1] = FC.LONG, 1001  # (the one row of the last chunk is kept)
    case = FC.Case("%d rows" % n, [(1, "long_gt", 1000)], t, v, n, np.zeros(64, dtype=np.uint8))
    keep = FC.reference_same_kind(case)
    assert keep[-1] and n // 20 < keep.sum() < n // 2
    sample = np.arange(0, n, 4099)
    assert np.array_equal(keep[sample], FC.reference(case._replace(types=t[:, sample], values=v[:, sample], n_rows=sample.size)))
    check_all(ctx, side_stream, case, caps=(None, 0), keep=keep)


def test_argument_errors(ctx, side_stream):
    import torch
    import simdjson_java_amd as S
    d = torch.ones(64, dtype=torch.int64, device="cuda:0")
    p = d.data_ptr()
    plain, strings = S.FilterPlan([(1, "long_gt", 0)]), S.FilterPlan([(0, "string_eq", b"a")])
    good = dict(plan=plain, d_types=p, d_values=p, n_cols=2, col_stride=4, n_rows=3, d_sb=p, d_keep=p, d_rows=p, out_capacity=3, d_out_types=p,
                d_out_values=p, d_result=p)
    for bad in (dict(n_cols=1), dict(col_stride=2), dict(d_result=0), dict(d_types=0), dict(d_values=0), dict(plan=strings, d_sb=0),
                dict(d_rows=0), dict(d_out_types=0), dict(d_out_values=0), dict(d_rows=0, d_out_types=0, d_out_values=0),
                dict(d_values=p + 4), dict(d_keep=p + 4), dict(d_rows=p + 1), dict(d_out_values=p + 2), dict(d_result=p + 4), dict(n_rows=1 << 40, col_stride=1 << 40)):
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.filter_columns_device(stream=side_stream, **dict(good, **bad))
    # legal: no rows with NULL columns; a plan without a STRING term and no string buffer; odd type pointers
    d_res = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    ctx.filter_columns_device(stream=side_stream, **dict(good, d_types=0, d_values=0, n_rows=0, col_stride=0, d_sb=0, d_keep=0, d_rows=0, d_out_types=0,
                                                          d_out_values=0, out_capacity=0, d_result=d_res.data_ptr()))
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [0, 0]
    plain.close()
    strings.close()


# ---------------------------------------------------------------------------------------------------------------------
# end to end: BatchShard.step / select / explode / check / filter / string_column on the twitter fixture
# ---------------------------------------------------------------------------------------------------------------------
def _shard(ctx, docs, stream):
    import torch
    from simdjson_java_amd import sharding
    buf, offs = _pack(docs)
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.step(stream)
    return shard


def _median_long(col):
    vals = sorted(FC.cell_object(t, p, b"") for t, p in col if t == FC.LONG)
    return vals[len(vals) // 2]


def _commonest_string(col):
    vals = [p for t, p in col if t == FC.STRING]
    return max(sorted(set(vals)), key=vals.count)


def _check_filtered(shard, types, values, n_rows, want, plans, text_column, failed_row, stream):
    """every plan through BatchShard.filter at the default capacity and at half of n_kept, the compacted text column through
    string_column; -> the kept rows per plan"""
    import torch
    import simdjson_java_amd as S
    counts = []
    for terms in plans:
        keep = FC.reference_from_cells(terms, want, n_rows)
        kept = np.flatnonzero(keep)
        n_kept = kept.size
        assert 0 < n_kept < n_rows, (terms, n_kept)  # the plan keeps a row and drops a row, by the reference
        assert failed_row is None or not keep[failed_row]
        plan = S.FilterPlan(terms)
        for capacity in (None, n_kept // 2):
            rows, ot, ov, words, res = shard.filter(plan, types, values, n_rows=n_rows, out_capacity=capacity, stream=stream)
            torch.cuda.synchronize()
            cap = n_rows if capacity is None else capacity
            m = min(n_kept, cap)
            assert rows.shape == (cap,) and ot.shape == (len(want), cap) and ov.shape == (len(want), cap) and words.numel() == (n_rows + 63) // 64
            assert res.cpu().tolist() == [n_kept, FC.OVERFLOW if n_kept > cap else 0], terms
            assert np.array_equal(words.cpu().numpy().view(np.uint64), FC.words_of(keep))
            assert np.array_equal(rows[:m].cpu().numpy(), kept[:m])
            sb = shard.sb.cpu().numpy()
            SEL.check_columns(ot[:, :m].cpu().numpy(), ov[:, :m].cpu().numpy(), sb, [[col[r] for r in kept[:m]] for col in want], "filtered by %r" % (terms,))
            # the compacted text column is a column for the string gather
            ref = SC.reference_from_cells([want[text_column][r] for r in kept[:m]])
            offsets, validity, data, result = shard.string_column(ot[text_column][:m], ov[text_column][:m], stream=stream)
            torch.cuda.synchronize()
            SC.check("text filtered by %r" % (terms,), offsets.cpu().numpy(), validity.cpu().numpy(), data.cpu().numpy(), result.cpu().numpy(), ref,
                     len(ref[2]), canaries=False)
        plan.close()
        counts.append(n_kept)
    return counts


def test_selected_statuses_filtered(ctx, side_stream):
    import torch
    import simdjson_java_amd as S
    pointers = ["/user/followers_count", "/lang", "/text", "/retweeted_status"]
    docs = SEL.reserialised("twitter.json", lambda d: d["statuses"])
    docs = docs[:7] + [STAGE2_FAILS] + docs[7:]  # one document that fails stage 2: MISSING on every path
    parsed = [O.parse(d) for d in docs]
    assert parsed[7].error and not parsed[6].error
    want = SEL.expected_columns(parsed, pointers)
    shard = _shard(ctx, docs, side_stream)
    plan = S.SelectPlan(pointers)
    types, values = shard.select(plan, side_stream)
    torch.cuda.synchronize()
    assert shard.check()["failed_documents"] == 1
    ge, eq, present = (0, "long_ge", _median_long(want[0])), (1, "string_eq", _commonest_string(want[1])), (3, "type_ne", 0)
    counts = _check_filtered(shard, types, values, len(docs), want, [[ge], [eq], [present], [ge, eq, present]], 2, 7, side_stream)
    assert counts[3] <= min(counts[:3])
    plan.close()


def test_exploded_statuses_filtered(ctx, side_stream):
    import torch
    import simdjson_java_amd as S
    name, docs, base, ptrs = EC.twitter_case()
    parsed = [O.parse(d) for d in docs]
    want_offs, want = EC.expected_explode(parsed, base, ptrs)
    total = want_offs[-1]
    assert total > 64
    shard = _shard(ctx, docs, side_stream)
    plan = S.ExplodePlan(base, ptrs)
    capacity = total + 9  # col_stride = row_capacity > n_rows
    _, et, ev = shard.explode(plan, capacity, side_stream)
    torch.cuda.synchronize()
    assert shard.check()["failed_documents"] == 0
    count, lang, name_of, text = (ptrs.index(p) for p in ("/retweet_count", "/metadata/iso_language_code", "/retweeted_status/user/name", "/text"))
    ge, eq, present = (count, "long_ge", _median_long(want[count])), (lang, "string_eq", _commonest_string(want[lang])), (name_of, "type_ne", 0)
    _check_filtered(shard, et, ev, total, want, [[ge], [eq], [present], [ge, eq, present]], text, None, side_stream)
    plan.close()
