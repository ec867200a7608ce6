"""The table reader's number arithmetic and host side without a GPU (DESIGN K21): the generated power table, the
Python-integer model of the device's certification against float(), and the stand-alone check of the host code under the
address and undefined-behaviour sanitizers."""
import importlib.util
import os
import random
import shutil
import subprocess
import sys

import pytest

import table_parse_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "infercnv_amd", "csrc")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_parse_pow10_table", os.path.join(CSRC, "gen_parse_pow10_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_generator(*args):
    return subprocess.run([sys.executable, os.path.join(CSRC, "gen_parse_pow10_table.py"), *args], capture_output=True, text=True)


def test_generator_writes_and_checks_a_header_and_k20s_is_untouched(tmp_path):
    """The header is written at build time and not kept in git, so the test works on its own copy: --check accepts what the
    generator wrote, refuses a changed file, and a header left by a build is the same text."""
    out = str(tmp_path / "tp_pow10_table.h")
    assert run_generator("--out", out).returncode == 0
    assert run_generator("--check", "--out", out).returncode == 0
    built = os.path.join(CSRC, "tp_pow10_table.h")
    if os.path.exists(built):
        assert open(built).read() == open(out).read()
    with open(out, "a") as f:
        f.write("\n")
    assert run_generator("--check", "--out", out).returncode == 1
    res = subprocess.run([sys.executable, os.path.join(CSRC, "gen_pow10_table.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_table_entries_are_floor_of_the_power(gen):
    assert (gen.K_MIN, gen.K_MAX) == (-342, 308)
    for k in range(gen.K_MIN, gen.K_MAX + 1):
        p, e = gen.TABLE[k - gen.K_MIN]
        assert 1 << 127 <= p < 1 << 128
        if k >= 0:                                   # p 2^e <= 10^k < (p + 1) 2^e
            assert p * 2 ** e <= 10 ** k < (p + 1) * 2 ** e if e >= 0 else p <= 10 ** k * 2 ** -e < p + 1
        else:
            assert p * 10 ** -k <= 2 ** -e < (p + 1) * 10 ** -k


def never_wrong(gen, fields):
    declined = 0
    for f in fields:
        got = gen.model_field(f.encode())
        assert got[0] != "bad", f
        if got[0] == "host":
            declined += 1
        else:
            assert got[1] == gen.expected_bits(f.encode()), (f, hex(got[1]))
    return declined


def test_model_never_certifies_a_wrong_value_on_random_fields(gen):
    rng = random.Random(2021)
    fields = []
    for _ in range(100000):                          # 1 .. 19 digits, exponents over the doubles' whole range and past both ends
        nd = rng.randrange(1, 20)
        w = rng.randrange(10 ** (nd - 1), 10 ** nd)
        q = rng.randrange(-345 - nd, 311)
        fields.append(f"{w}e{q}" if rng.random() < 0.7 else f"{str(w)[0]}.{str(w)[1:]}e{q + nd - 1}")
    declined = never_wrong(gen, fields)
    assert declined < len(fields) // 5               # the subnormal and out-of-range ends; the bulk is certified


def test_model_on_the_hard_cases(gen):
    assert never_wrong(gen, [f for f in cases.ADVERSARIAL]) > 0
    for tie in ["9007199254740993", "4503599627370496.5"] + cases.TIES:         # exact ties are never certified
        assert gen.model_field(tie.encode()) == ("host",), tie
    for text in ("4.9e-324", "1e-400", "1e400", "2.2250738585072011e-308"):      # subnormal, underflow, overflow: the host's
        assert gen.model_field(text.encode()) == ("host",), text
    assert gen.model_field(b"-0") == ("value", 1 << 63)
    assert gen.model_field(b"1.7976931348623158e308")[0] == "value"
    assert gen.model_field(b"NA") == gen.model_field(b"") == ("value", 0x7FF00000000007A2)
    assert gen.model_field(b"NaN") == ("value", 0x7FF8000000000000)
    for bad in ("1.2.3", "abc", '"1"', "0x10", " 1", "1 ", "1e", ".", "+", "nan", "inf", "Infinity", "-NA", "1,5"):
        assert gen.model_field(bad.encode()) == ("bad",), bad


def test_plain_fields_take_the_exact_path(gen):
    """Integers and decimals of at most 15 digits never reach the host: one exact multiply or divide (the claim behind the
    GPU test's host_parsed == 0)."""
    for f in cases.PLAIN:
        r = gen.scan_field(f.encode())
        assert r[0] in ("value", "decimal"), f
        if r[0] == "decimal":
            assert r[1] < 1 << 53 and -22 <= r[2] <= 22, (f, r)
            assert gen.convert(*r[1:]) == gen.expected_bits(f.encode())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_side_under_sanitizers(tmp_path):
    """table_parse_check.cpp: the certified conversion and the host path against strtod, then chunking, label slicing and
    strtod patching of three files through a 32-byte buffer that has to grow, under ASan and UBSan."""
    exe = tmp_path / "table_parse_check"
    assert run_generator("--out", str(tmp_path / "tp_pow10_table.h")).returncode == 0       # found through -I without a build
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(tmp_path),
                          "-o", str(exe), os.path.join(CSRC, "table_parse_check.cpp")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    files = []
    for i, (eol, final, quoted) in enumerate((("\n", True, False), ("\r\n", False, True), ("\n", False, False))):
        text, _, _, _ = cases.table_text(cases.ADVERSARIAL + cases.PLAIN[:200], 7, eol=eol, final_newline=final, quote_labels=quoted)
        body = text.split(eol, 1)[1]                 # the program reads rows; the header line is the Python reader's
        path = tmp_path / f"t{i}.tsv"
        path.write_bytes((body + (eol + eol if i == 0 else "")).encode())
        files.append(str(path))
    res = subprocess.run([str(exe), "20000", "32"] + files, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.count(" rows, ") == 3 and ", 0 refused" in res.stdout
