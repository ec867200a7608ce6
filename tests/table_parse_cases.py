"""Inputs shared by tests/test_table_parse_host.py and tests/test_gpu_table_parse.py: the fields of the number-grammar table of
the table reader (DESIGN K21), built once, and helpers that write them as files."""
import random
from fractions import Fraction

HARD = ["9007199254740993", "2.2250738585072011e-308", "1.7976931348623158e308", "4.9e-324", "1e-400", "1e400", "-0",
        "9007199254740992.5", "0.30000000000000004", "1e23", "8.5e22", "1234567890123456789", "12345678901234567890",
        "2.4703282292062327e-324", "2.4703282292062328e-324", "1.7976931348623157e308", "5e-324", "123456789012345678e-340"]
SPECIAL = ["NA", "", "NaN", "Inf", "-Inf", "+Inf", "+3", ".5", "5.", "1E5", "-.5e-3", "0", "-0.0", "0e99", "007", "1e+05"]


def halfway_decimals(n, seed=5):
    """(2 m + 1) 2^(e - 1) for 53-bit m: the exact decimal of a halfway point between two doubles (a tie), and the same digits
    cut to 19 significant ones (just below the tie, within the device's 19 digits)."""
    rng = random.Random(seed)
    ties, cut = [], []
    for _ in range(n):
        m = (1 << 52) | rng.getrandbits(52)
        e = rng.randrange(-40, 60)
        v = Fraction(2 * m + 1) * Fraction(2) ** (e - 1)
        if v.denominator == 1:
            s = str(v.numerator)
        else:                                                   # denominator 2^k: k decimals print it exactly
            k = v.denominator.bit_length() - 1
            digits = str(v.numerator * 5 ** k).rjust(k + 1, "0")
            s = digits[:-k] + "." + digits[-k:]
        ties.append(s)
        sig = s.replace(".", "").lstrip("0")
        point = s.index(".") if "." in s else len(s)
        lead = len(s.replace(".", "")) - len(sig)               # leading zeros dropped from the digit string
        cut.append(f"{sig[:19]}e{point - lead - 19}")
    return ties, cut


def plain_fields(n, seed=6):
    """Integers and decimals of at most 15 significant digits with a decimal exponent within +-22: the shapes of real data."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            out.append(str(rng.randrange(0, 2000)))
        elif kind == 1:
            out.append(str(rng.randrange(0, 10 ** rng.randrange(1, 16))))
        elif kind == 2:
            out.append("%.6g" % (rng.random() * 10 ** rng.randrange(-3, 5)))     # 6 significant digits, the example data's shape
        else:
            nd = rng.randrange(1, 16)
            out.append(f"{rng.randrange(1, 10 ** nd)}e{rng.randrange(-22, 23 - nd)}" if rng.random() < 0.3 else
                       "%.*f" % (rng.randrange(0, 8), rng.random() * 10 ** rng.randrange(0, 7)))
    return out


TIES, CUT19 = halfway_decimals(40)
PLAIN = plain_fields(3000)
ADVERSARIAL = HARD + ["-" + h for h in HARD if not h.startswith("-")] + TIES + CUT19 + SPECIAL


def table_text(fields, n_cols, sep="\t", eol="\n", header_corner=False, quote_labels=False, final_newline=True, label="g"):
    """(text, row names, column names, fields per row) of a table that holds `fields` row by row, padded with 0."""
    fields = list(fields) + ["0"] * (-len(fields) % n_cols)
    rows = [fields[i:i + n_cols] for i in range(0, len(fields), n_cols)]
    cols = [f"c{j + 1}" for j in range(n_cols)]
    names = [f"{label}{i + 1}" for i in range(len(rows))]
    q = (lambda s: '"' + s + '"') if quote_labels else (lambda s: s)
    lines = [sep.join(([q("corner")] if header_corner else []) + [q(c) for c in cols])]
    lines += [sep.join([q(nm)] + r) for nm, r in zip(names, rows)]
    text = eol.join(lines) + (eol if final_newline else "")
    return text, names, cols, rows
