"""Host pieces of the matrix-file writer (DESIGN K20) that need no GPU: the restatement of the field rule against
heatmap.r_num, the generated power-of-ten table, and the kernels' digit arithmetic compiled for the CPU."""
import importlib.util
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np

import table_text_restate as ttr
from infercnv_amd import _lib
from infercnv_amd import heatmap as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "infercnv_amd", "csrc")

SPECIAL = [0.0, -0.0, 1.0, 0.1, 0.3, 2.0 / 3.0, 0.30000000000000004, 1e5, 100000.0, 1e-4, 0.0001234, 1234567.125, 2.0 ** -20,
           1e15, 1e22, 999999999999999.5, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, float("nan"), float("inf"),
           100000000000000.5, 123456789012345.5, 123456789012346.5]
EXPECT = {1e5: "1e+05", 1e-4: "1e-04", 0.0001234: "0.0001234", 123456789012345.5: "123456789012346", 123456789012346.5: "123456789012346",
          100000000000000.5: "1e+14", 999999999999999.5: "1e+15", -0.0: "0", 1e22: "1e+22", 5e-324: "4.94065645841247e-324",
          1.7976931348623157e308: "1.79769313486232e+308", 0.30000000000000004: "0.3", 2.0 ** -20: "9.5367431640625e-07"}


def test_restatement_equals_r_num_on_the_special_list():
    for v in SPECIAL:
        for x in (v, -v):
            assert ttr.field(x) == hm.r_num(x), repr(x)
            assert len(ttr.field(x)) <= 22
    for v, text in EXPECT.items():
        assert ttr.field(v) == text, repr(v)
    assert ttr.field(float("-inf")) == "-Inf" and ttr.field(-1234567.125) == "-1234567.125"


def test_restatement_equals_r_num_on_random_bit_patterns():
    bits = np.random.default_rng(20).integers(0, 2 ** 64, size=100_000, dtype=np.uint64)
    for x in bits.view(np.float64).tolist():
        assert ttr.field(x) == hm.r_num(x), repr(x)


def test_exact_ties():
    for v in (100000000000000.5, 123456789012345.5, 123456789012346.5, 999999999999999.5, 1000000000000005.0):
        assert ttr.is_exact_tie(v) and ttr.is_exact_tie(-v), repr(v)
    for v in (1.0, 0.1, 0.3, 1e22, 5e-324, 1234567.125, 123456789012345.25, float("nan"), float("inf"), 0.0):
        assert not ttr.is_exact_tie(v), repr(v)


def _generator():
    spec = importlib.util.spec_from_file_location("gen_pow10_table", os.path.join(CSRC, "gen_pow10_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_power_table_is_generated():
    r = subprocess.run([sys.executable, os.path.join(CSRC, "gen_pow10_table.py"), "--check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "up to date" in r.stdout


def test_power_table_entries_are_the_exact_floors():
    """The words in the committed header, read back, are floor(10^k / 2^q) with the top bit set, for every k."""
    gen = _generator()
    text = open(os.path.join(CSRC, "tt_pow10_table.h")).read()

    def array(name):
        body = re.search(name + r"\[\d+\] = \{(.*?)\};", text, re.S).group(1)
        return [int(t.rstrip("ul"), 0) for t in body.replace("\n", " ").split(",") if t.strip()]

    hi, lo, q = array("tt_pow10_hi"), array("tt_pow10_lo"), array("tt_pow10_q")
    n = gen.K_MAX - gen.K_MIN + 1
    assert len(hi) == len(lo) == len(q) == n and (gen.K_MIN, gen.K_MAX) == (-294, 338)
    for i in range(n):
        k = gen.K_MIN + i
        p = (hi[i] << 64) | lo[i]
        assert 2 ** 127 <= p < 2 ** 128
        exact = Fraction(10) ** k / Fraction(2) ** q[i]
        assert p <= exact < p + 1, k
        assert (p == exact) == (0 <= k <= 55), k          # 5^k fits 128 bits up to k = 55: those entries are exact


def test_digit_arithmetic_on_the_cpu(tmp_path):
    """table_text_digits.h -- the functions the kernels run -- compiled for the CPU and compared with snprintf("%.14e") on the
    special values, every power of two and of ten with its neighbours, random bit patterns, heatmap-like values and
    half-integers of 15 digits; flagged elements take the host's exact path, as in the library."""
    exe = str(tmp_path / "table_text_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(CSRC, "table_text_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) values, (\d+) flagged in all, (\d+) among the specials, (\d+) among the heatmap-like values", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 600_000 and int(m.group(4)) == 0 and int(m.group(2)) > 1000   # the half-integers are flagged, heatmap values never


def test_prototypes():
    for name in ("icnv_format_table_dev", "icnv_format_table", "icnv_table_text_stats", "icnv_table_text_stats_reset"):
        assert name in _lib.PROTOTYPES
    header = open(os.path.join(ROOT, "include", "icnv.h")).read()
    assert "ICNV_TABLE_GENE_ROWS 0" in header and "ICNV_TABLE_CELL_ROWS 1" in header
    assert (_lib.TABLE_GENE_ROWS, _lib.TABLE_CELL_ROWS) == (0, 1)
