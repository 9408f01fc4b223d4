"""tests/walk_common.exact_number -- the exact (Fraction, ties to even) reference the GPU number tests compare with -- pinned on its
own, without a GPU: against Python's float() (correctly rounded) and int(), and against the reference's NumberParsingTest vectors."""
import random
import struct

from tests.conftest import number_vectors
from tests.walk_common import boundary_literal, exact_number, exact_range, random_number_literal


def _float_word(lit):
    f = float(lit)
    return ("d", struct.unpack("<Q", struct.pack("<d", f))[0])


def test_exact_reference_against_float_and_int():
    rng = random.Random(4242)
    lits = [random_number_literal(rng) for _ in range(20000)] + [boundary_literal(rng, short=False) for _ in range(3000)]
    edges = ["0.0", "-0.0", "0e999", "4.9406564584124654e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
             "2.2250738585072014e-308", "2.2250738585072011e-308", "1.7976931348623157e308", "1.7976931348623158e308",
             "1.7976931348623159e308", "-1e400", "1e-400", "9007199254740993", "9007199254740993.0", "9007199254740995.0",
             "1e23", "8.98846567431158e307", "123456789012345678901234567890e-300", "0.1", "-0.000000000000000000000001e-300"]
    floats = 0
    for lit in lits + edges:
        got = exact_number(lit)
        if any(c in lit for c in ".eE"):
            assert got == _float_word(lit), (lit, got, _float_word(lit))  # (overflow: +-infinity, as float() gives it)
            floats += 1
        else:
            v = int(lit)
            want = ("l", v & (2 ** 64 - 1)) if -2 ** 63 <= v < 2 ** 63 else None
            assert got == want, (lit, got)
    assert floats > 15000
    for bad in ["", "-", "+1", "01", "1.", ".5", "1e", "1e+", "--1", "1.0.1", "0x10", " 1", "1 ", "NaN", "Infinity", "1,"]:
        assert exact_number(bad) is None, bad
    for v in ["9223372036854775807", "-9223372036854775808"]:
        assert exact_number(v) == ("l", int(v) & (2 ** 64 - 1))
    for v in ["9223372036854775808", "-9223372036854775809", "123456789012345678901"]:
        assert exact_number(v) is None


def test_exact_reference_against_the_reference_vectors():
    n = 0
    for v in number_vectors():
        lit = v["input"][:int(v["length"])] if v.get("length") is not None else v["input"]
        got = exact_number(lit)
        if "message" in v:
            assert got is None, (lit, got)
        elif "long" in v:
            assert got == ("l", int(v["long"]) & (2 ** 64 - 1)), (lit, got)
        else:
            assert got == ("d", int(v["double_bits"])), (lit, got, v["cite"])
        n += 1
    assert n >= 158


def test_boundary_literals_are_boundary_literals():
    """The generator's literals have more than 19 significant digits and sit so close to a midpoint of two doubles that their two
    19-digit neighbours round differently (what makes the device list them for the exact comparison)."""
    rng = random.Random(4343)
    kinds = set()
    for _ in range(4000):
        lit = boundary_literal(rng)
        assert not exact_range(lit) and len(lit) <= 48, lit
        sig = lit.lstrip("-").lower().split("e")[0].replace(".", "").strip("0")
        assert len(sig) > 19, lit
        t, raw = exact_number(lit)
        assert t == "d" and (raw >> 63) == lit.startswith("-")
        e = (raw >> 52) & 0x7FF
        kinds.add("subnormal" if e == 0 else "infinity" if e == 0x7FF else "normal")
    assert kinds == {"subnormal", "infinity", "normal"}
