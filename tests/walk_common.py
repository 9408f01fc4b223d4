"""Shared by the CPU and GPU tests of the GPU walker (csrc/walk_doc.h / walk.hip)."""
NEEDS_HOST = -1


def exact_range(lit):
    """Independent statement of what the device converts itself (csrc/sj_number.h): every literal of at most 19 significant
    digits (Clinger's exact range + Eisel-Lemire), and every longer one whose two 19-digit neighbours w * 10^q and
    (w + 1) * 10^q are the same double (Python's float() is correctly rounded).  False: handed back (the reference's slow
    path, DoubleParser.java:205-330)."""
    s = lit.lstrip("-").lower()
    mant, _, e = s.partition("e")
    ip, _, fp = mant.partition(".")
    digits = ip + fp
    stripped = digits.lstrip("0")
    if len(stripped.rstrip("0")) <= 19:
        return True
    lead = len(digits) - len(stripped)
    exp = max(-10 ** 6, min(10 ** 6, int(e) if e else 0))
    w, q = int(stripped[:19]), exp + len(ip) - lead - 19
    return float("%de%d" % (w, q)) == float("%de%d" % (w + 1, q))


# more than 19 significant digits AND closer than 10^-19 (relative) to the midpoint of two doubles: neither 19-digit
# neighbour decides the rounding
AMBIGUOUS = ["9007199254740993.00000000000000000001", "9007199254740994.99999999999999999999", "1.00000000000000011102230246251565404236316680908203125",
             "1.00000000000000011102230246251565404236316680908203124", "2.4703282292062327208051355972e-324",
             "0.500000000000000166533453693773481063544750213623046875",
             str(((1 << 54) - 1) << 970) + ".0"]  # the midpoint of the largest double and 2^1024


def random_number_literal(rng):
    k = rng.random()
    if k > 0.97:  # around a rounding boundary: an exact midpoint of two doubles, nudged (or not) far behind the 19th digit
        from decimal import Decimal, getcontext
        import struct
        getcontext().prec = 1200
        bits = rng.getrandbits(52) | (rng.choice([1, 500, 1022, 1023, 1024, 1075, 1500, 2045]) << 52)
        lo = Decimal(struct.unpack("<d", struct.pack("<Q", bits))[0])
        hi = Decimal(struct.unpack("<d", struct.pack("<Q", bits + 1))[0])
        mid = (lo + hi) / 2
        text = format(mid, "f")
        if "." not in text:
            text += ".0"
        tweak = rng.choice(["", "1", "000000000001", "9"])
        if tweak == "9":  # just below: decrement the last digit, append nines
            text = text.rstrip("0")
            text = text[:-1] + str(int(text[-1]) - 1) + "9" * 12 if text[-1] not in ".0" else text + "1"
        else:
            text += tweak
        return ("-" if rng.random() < 0.3 else "") + text
    sign = "-" if rng.random() < 0.3 else ""
    if k < 0.25:
        return sign + str(rng.randrange(10 ** rng.randint(1, 18)))
    ip = str(rng.randrange(10 ** rng.randint(1, rng.choice([1, 3, 8, 16, 21, 30])))) if rng.random() < 0.8 else "0"
    fp = ""
    if rng.random() < 0.8:
        fp = "." + "".join(rng.choice("0000123456789") for _ in range(rng.randint(1, rng.choice([1, 2, 6, 12, 20, 40]))))
    ex = ""
    if rng.random() < 0.4 or not fp:
        ex = rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randrange(rng.choice([3, 10, 25, 40, 330, 400])))
    return sign + ip + fp + ex


def number_documents(rng, n):
    """-> (documents, set of indexes that must be handed back, set of indexes where either answer is right)"""
    docs, hard, either = [], set(), set()
    for k in range(n):
        lits = [random_number_literal(rng) for _ in range(rng.randint(1, 6))]
        docs.append(("[" + ", ".join(lits) + "]").encode())
        verdicts = [exact_range(x) for x in lits if any(c in x for c in ".eE")]
        if any(v is False for v in verdicts):
            hard.add(k)
    return docs, hard, either


def assert_tape_equal(got, got_strings, want, what=None):
    """A batch's tape of one document against the oracle's (`want`: oracle.parse of the document alone), word for word: every word
    bit-equal -- both root words, the back-pointers of opening and closing brackets, element counts saturated or not, numbers --
    except the payload of a '"' word, which points into a different string buffer: there both must point to the same record (4-byte
    big-endian length, then the bytes)."""
    import numpy as np
    got = np.ascontiguousarray(got).view(np.uint64)
    exp = np.ascontiguousarray(want.tape).view(np.uint64)
    assert got.size == exp.size, (what, "tape length", got.size, exp.size)
    q = (exp >> np.uint64(56)) == np.uint64(0x22)
    diff = np.nonzero((got != exp) & ~q)[0]
    if diff.size:
        i = int(diff[0])
        raise AssertionError((what, "word %d of %d" % (i, exp.size), hex(int(got[i])), hex(int(exp[i]))))
    low = np.uint64((1 << 56) - 1)
    for i in np.nonzero(q)[0]:
        g, w = int(got[i]), int(exp[i])
        assert g >> 56 == 0x22, (what, "word %d" % i, hex(g), hex(w))
        go, wo = g & int(low), w & int(low)
        ln = int.from_bytes(want.strings[wo:wo + 4], "big")
        assert got_strings[go:go + 4 + ln] == want.strings[wo:wo + 4 + ln], (what, "string word %d" % i, go, wo)


_LITERAL = None


def exact_number(lit):
    """Plain reference for one JSON number literal, exact by construction: -> ('l', raw) for an integer inside the long range,
    ('d', raw) for a floating literal (the decimal value as a Fraction, rounded to binary64 with ties to even: subnormals, and
    +-infinity past the largest double, as the reference's DoubleParser gives them), None for anything else (bad grammar, an
    integer outside [-2^63, 2^63 - 1]).  raw = the tape's second word (two's complement / IEEE bits as an unsigned 64-bit int)."""
    import re
    from fractions import Fraction
    global _LITERAL
    if _LITERAL is None:
        _LITERAL = re.compile(r"(-?)(0|[1-9][0-9]*)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?\Z")
    m = _LITERAL.match(lit)
    if not m:
        return None
    sign, ip, fp, ex = m.group(1), m.group(2), m.group(3), m.group(4)
    if fp is None and ex is None:
        v = int(sign + ip)
        return ("l", v & (2 ** 64 - 1)) if -2 ** 63 <= v < 2 ** 63 else None
    neg = 1 << 63 if sign else 0
    digits = (ip + (fp or "")).lstrip("0")
    if not digits:
        return ("d", neg)
    e10 = int(ex or "0") - len(fp or "")                # value = int(digits) * 10^e10
    lead = e10 + len(digits) - 1                        # decimal exponent of the leading digit
    if lead > 310:
        return ("d", neg | 0x7FF0000000000000)
    if lead < -330:                                     # below half the smallest subnormal (~2.47e-324)
        return ("d", neg)
    x = Fraction(int(digits)) * (Fraction(10) ** e10)
    # x = q * 2^e with 2^52 <= q < 2^53 (q a real here), e >= -1074: the quantum of the subnormals
    e = max(x.numerator.bit_length() - x.denominator.bit_length() - 53, -1074)
    while e > -1074 and x < Fraction(2 ** 52) * Fraction(2) ** e:
        e -= 1
    while x >= Fraction(2 ** 53) * Fraction(2) ** e:
        e += 1
    s = x / Fraction(2) ** e
    q, r = divmod(s.numerator, s.denominator)
    if 2 * r > s.denominator or (2 * r == s.denominator and q & 1):
        q += 1
    if q == 2 ** 53:
        q, e = q >> 1, e + 1
    if q < 2 ** 52:                                     # subnormal (or zero): e == -1074, biased exponent 0
        return ("d", neg | q)
    biased = e + 1075
    if biased >= 2047:
        return ("d", neg | 0x7FF0000000000000)
    return ("d", neg | (biased << 52) | (q - 2 ** 52))


def tape_numbers(tape):
    """The number words of a tape in order: [(type char, raw second word)] -- 'l' / 'd' words are followed by their payload."""
    out, i = [], 0
    words = [int(w) for w in tape]
    while i < len(words):
        t = words[i] >> 56
        if t in (0x6C, 0x64):
            out.append((chr(t), words[i + 1]))
            i += 2
        else:
            i += 1
    return out


def _midpoint_text(rng):
    """The exact decimal midpoint of two neighbouring doubles, as text (no sign), and whether it needs an exponent: short ones
    (between 2^52 and 2^64: an integer, or an integer + .5), the subnormals, the overflow edge."""
    from decimal import Decimal, getcontext
    getcontext().prec = 1200
    r = rng.random()
    if r < 0.85:
        e = rng.randint(0, 11)
        m = rng.randrange(2 ** 52, 2 ** 53)
        mid2 = (2 * m + 1) << e                          # twice the midpoint of m * 2^e and (m + 1) * 2^e
        return ("%d.5" % (mid2 >> 1)) if e == 0 else str(mid2 >> 1)
    if r < 0.95:                                         # subnormal: (2k + 1) * 2^-1075
        k = rng.choice([0, 1, 2, rng.randrange(2 ** 20), rng.randrange(2 ** 52)])
        return format(Decimal(2 * k + 1) / (Decimal(2) ** 1075), "f")
    # between the largest double and 2^1024 (rounds to infinity from the midpoint up), and just below the largest double
    m = (1 << 53) - rng.choice([1, 2])
    return str((2 * m + 1) << 970)                      # (m * 2^971: the largest double for m = 2^53 - 1)


def boundary_literal(rng, short=True):
    """A floating literal of more than 19 significant digits that its two 19-digit neighbours w * 10^q and (w + 1) * 10^q do
    not decide (exact_range is False: the device lists it for the exact midpoint comparison of sj_bigdec.h): an exact midpoint
    of two doubles with a nonzero tail behind it, or just below it.  short: mostly 30 .. 45 bytes."""
    while True:
        text = _midpoint_text(rng)
        if "." not in text:
            text += ".0"
        ip, fp = text.split(".")
        above = rng.random() < 0.5
        if above:                                        # just above: the midpoint, zeros, a last nonzero digit
            fp = fp + "0" * rng.randint(0, 6) + rng.choice("123456789")
        else:                                            # just below: minus one unit in the last place, then nines
            digits = str(int(ip + fp) - 1).rjust(len(ip + fp), "0")
            ip, fp = digits[:len(ip)], digits[len(ip):] + "9" * rng.randint(1, 6)
        sig = (ip + fp).lstrip("0")
        if len(sig) > 60 or rng.random() < 0.3:          # scientific form: d.ddd...e<exp>, cut after 24 .. 40 digits
            lead = len(ip.lstrip("0")) - 1 if ip.lstrip("0") else -(len(fp) - len(fp.lstrip("0")) + 1)
            cut = sig[:rng.randint(24, 40)]
            if above and len(cut) < len(sig):            # (cut short: one unit up stays above the midpoint)
                cut = str(int(cut) + 1)
            cut = cut.rstrip("0")
            if len(cut) < 21:
                continue
            lit = "%s.%se%s%d" % (cut[0], cut[1:], rng.choice(["", "+"]) if lead >= 0 else "", lead)
            if rng.random() < 0.5:
                lit = lit.replace("e", "E")
        else:
            lit = ip + "." + fp
        lit = ("-" if rng.random() < 0.4 else "") + lit
        if not exact_range(lit) and (not short or len(lit) <= 48):
            return lit
