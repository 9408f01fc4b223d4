"""tools/opbench.py, the harness under the eight operator benches: the pure aggregation of a leg's per-round milliseconds into its
record, with hand-made lists.  The measuring itself needs a GPU and runs with the tools."""
from tools import opbench


def test_leg_record_is_the_median_of_round_medians():
    rec = opbench.leg_record([[3.0, 1.0, 2.0], [10.0, 30.0, 20.0, 40.0], [5.0, 4.0, 6.0]])
    # round medians 2, 25 (an even round: the mean of the middle two) and 5; the outlier round moves neither median nor minimum
    assert rec == {"median_ms": 5.0, "min_ms": 1.0, "round_medians_ms": [2.0, 25.0, 5.0], "spread": (25.0 - 2.0) / 5.0, "steps": 10}
    assert list(rec) == ["median_ms", "min_ms", "round_medians_ms", "spread", "steps"]


def test_leg_record_of_equal_rounds_has_no_spread():
    rec = opbench.leg_record([[2.0, 2.0], [2.0, 2.0]])
    assert rec["spread"] == 0.0 and rec["median_ms"] == 2.0 and rec["steps"] == 4


def test_leg_record_of_one_round():
    rec = opbench.leg_record([[7.0, 9.0, 8.0]])
    assert rec == {"median_ms": 8.0, "min_ms": 7.0, "round_medians_ms": [8.0], "spread": 0.0, "steps": 3}


def test_measure_shares_the_steps_among_the_rounds(monkeypatch):
    """per round steps // rounds executions (at least 3), a third of them for the legs named so, two by the wall clock for a host
    leg; the warm-up in front of the first round only"""
    calls = []
    monkeypatch.setattr(opbench, "timed", lambda fn, steps, warmup: calls.append((fn, steps, warmup)) or [1.0] * steps)
    monkeypatch.setattr(opbench, "wall", lambda fn, steps: calls.append((fn, steps, None)) or [1.0] * steps)
    out = opbench.measure({"a": "A", "slow": "S", "cpu": "C"}, 30, 5, third={"slow"}, host={"cpu"})
    assert calls == [("A", 10, 5), ("S", 3, 5), ("C", 2, None)] + [("A", 10, 1), ("S", 3, 1), ("C", 2, None)] * 2
    assert {k: v["steps"] for k, v in out.items()} == {"a": 30, "slow": 9, "cpu": 6}
    calls.clear()
    assert opbench.measure({"a": "A"}, 6, 2)["a"]["steps"] == 9 and calls == [("A", 3, 2), ("A", 3, 1), ("A", 3, 1)]
