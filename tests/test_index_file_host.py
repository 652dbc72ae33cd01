"""The device-free side of asm_index_build_file (docs/design/mapper.md, "Reference: FASTA in, index out"): the reader's cutter
asm_fasta_cut at every offset, the parser's rules (csrc/asm_fasta.h) run serially by host/fasta_host_check.cpp under ASan + UBSan
against a parser written from the contract (tests/fasta_cases.py), and the call's argument checks with a NULL handle, whole messages
pinned in tests/golden/index_file_rejections.json."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

from tests import fasta_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "index_file_rejections.json")
CHUNKS = (1, 7, 16, 17, 64, 0)  # 0: the whole file


# ---- asm_fasta_cut ------------------------------------------------------------------------------------------------------------
def cut(asm, data: bytes, at_line_start: bool):
    lib = asm.load_library()
    in_line = ctypes.c_int(-1)
    buf = ctypes.create_string_buffer(data, len(data) + 1)
    size = lib.asm_fasta_cut(buf, len(data), 1 if at_line_start else 0, ctypes.byref(in_line))
    return int(size), int(in_line.value)


def header_spans(data: bytes):
    """[s, e): a cut at c with s < c < e lies inside a header line (e: behind its newline, or behind the file)"""
    spans, s = [], 0
    for line in data.split(b"\n"):
        if line[:1] == b">":
            spans.append((s, s + len(line) + 1))
        s += len(line) + 1
    return spans


def test_fasta_cut_at_every_offset_and_reassembly(asm):
    data = fc.ugly_file(3, 1)
    assert 250 <= len(data) <= 400
    spans = header_spans(data)
    assert len(spans) == 5

    def inside(c):
        return any(s < c < e for s, e in spans)

    for k in range(len(data) + 1):
        size, in_line = cut(asm, data[:k], True)
        assert size <= k and not inside(size), k
        assert size == k or (data[size:size + 1] == b">" and b"\n" not in data[size:k]), k  # only an unfinished header stays back
        assert in_line == (1 if size and data[size - 1:size] != b"\n" else 0), k
    for step in (1, 7, 16, 17, 64, len(data)):
        # the reader's loop: what the cut before left, then `step` more bytes; nothing shipped: more bytes; the file's end ships all
        pieces, carry, pos, at_start = [], b"", 0, True
        while pos < len(data) or carry:
            buf = carry + data[pos:pos + step]
            pos = min(pos + step, len(data))
            size, in_line = cut(asm, buf, at_start)
            if pos >= len(data):
                size = len(buf)
            elif size == 0:
                carry = buf
                continue
            pieces.append(buf[:size])
            assert not inside(sum(map(len, pieces))) or pos >= len(data), step
            at_start, carry = not in_line, buf[size:]
        assert b"".join(pieces) == data, step
    assert cut(asm, b"", True) == (0, 0) and cut(asm, b"", False) == (0, 1)
    assert cut(asm, b">abc", True) == (0, 0) and cut(asm, b">abc", False) == (4, 1)  # inside a sequence line '>' is a base
    assert cut(asm, b"AC\n>abc\n", False) == (8, 0) and cut(asm, b"AC\n>abc", False) == (3, 0)


# ---- the parser's rules on the CPU ----------------------------------------------------------------------------------------------
def san_flags():
    """SAN_FLAGS of oracle/Makefile"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        for line in fh:
            if line.startswith("SAN_FLAGS :="):
                return line.split(":=", 1)[1].split()
    raise AssertionError("oracle/Makefile has no SAN_FLAGS")


@pytest.fixture(scope="module")
def fasta_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fasta_check") / "fasta_host_check_asan")
    src = os.path.join(PKG, "host", "fasta_host_check.cpp")
    assert os.path.exists(src), "host/fasta_host_check.cpp: the host build of the FASTA parser"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_check(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=600)
    err = r.stderr.decode("latin-1")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert r.returncode == 0, (r.returncode, err[-3000:])
    return r.stdout


def expected_output(data: bytes) -> bytes:
    names, offs, text = fc.py_parse(data)
    out = b"seqs %d\n" % len(names)
    for name, off in zip(names, offs):
        out += b"seq %d %s\n" % (off, name.hex().encode())
    return out + b"text %d\n" % len(text) + text + b"\n"


def test_parser_rules_on_the_cpu_equal_python_under_sanitizers(fasta_check, tmp_path):
    rng = random.Random(41)
    files = [fc.ugly_file(3, 1), fc.ugly_file(4, 40)] + [fc.random_small_file(rng) for _ in range(200)]
    files += [b"", b"\n", b">", b">\r", b"x", b">a", b">a\nAC", b"AC\n>a\n", b">a\n" + b"ac gt" * 1700, b">" + b"n" * 5000 + b" w\nAC\n"]
    assert sum(1 for d in files if not fc.py_parse(d)[0]) >= 5  # files without a sequence are among them
    path = tmp_path / "ref.fa"
    for t, data in enumerate(files):
        path.write_bytes(data)
        got = run_check(fasta_check, [path] + list(CHUNKS))
        assert got == expected_output(data) * len(CHUNKS), (t, data[:200])


def test_text_length_limit_is_a_count_comparison(fasta_check):
    """a text of 2^32 - 1 bytes or more is refused: asm_index_build_file compares the carried count of kept bytes with this rule"""
    assert run_check(fasta_check, ["--limits"]).split() == [b"0", b"1", b"4294967294", b"1", b"4294967295", b"0", b"4294967296", b"0"]


def test_tile_constant_is_shared(asm):
    with open(asm.HEADER_PATH) as fh:
        (tile,) = re.findall(r"#define ASM_FASTA_TILE (\d+)", fh.read())
    assert int(tile) == asm.FASTA_TILE
    with open(os.path.join(PKG, "csrc", "asm_fasta.h")) as fh:
        src = fh.read()
    assert re.search(r"#define FASTA_TILE %du\b" % asm.FASTA_TILE, src) and "FASTA_TILE == ASM_FASTA_TILE" in src


# ---- rejections -------------------------------------------------------------------------------------------------------------------
def rejection_cases(asm):
    lib = asm.load_library()
    base = dict(path=b"ref.fa", k=12, chunk_bytes=0, out=True)
    cases = []

    def add(label, **kw):
        a = dict(base, **kw)

        def thunk():
            out = ctypes.c_void_p(1)  # a successful or failed call must leave NULL here
            rc = lib.asm_index_build_file(None, a["path"], a["k"], a["chunk_bytes"], ctypes.byref(out) if a["out"] else None, None)
            assert not a["out"] or out.value is None
            return rc

        cases.append((label, thunk))

    add("out=NULL", out=False)
    add("out=NULL and everything else bad", out=False, path=None, k=7, chunk_bytes=-1)
    add("fasta_path=NULL", path=None)
    add("fasta_path=NULL, k and chunk_bytes bad", path=None, k=15, chunk_bytes=-1)
    for k in (7, 15, -1):
        add("k=%d" % k, k=k)
    add("k=7 and chunk_bytes=-1", k=7, chunk_bytes=-1)
    add("chunk_bytes=-1", chunk_bytes=-1)
    add("no handle", k=8)
    add("no handle, k=14, chunk_bytes above the cap", k=14, chunk_bytes=1 << 40)
    return cases


def replay(asm):
    lib = asm.load_library()
    return [[label, int(thunk()), lib.asm_last_error(None).decode()] for label, thunk in rejection_cases(asm)]


def test_index_file_rejections_are_pinned(asm):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = replay(asm)
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert g == w
        assert g[1] == -1 and g[2].startswith("asm_index_build_file: ")
    text = {g[0]: g[2] for g in got}
    assert text["out=NULL and everything else bad"] == "asm_index_build_file: out is NULL"
    assert text["fasta_path=NULL, k and chunk_bytes bad"] == "asm_index_build_file: fasta_path is NULL"
    assert text["k=7 and chunk_bytes=-1"] == "asm_index_build_file: k must be in [8, 14]"
    assert text["chunk_bytes=-1"] == "asm_index_build_file: chunk_bytes must be >= 0"
    assert text["no handle"] == "asm_index_build_file: NULL handle"


def test_accessors_take_null_and_get_text_checks_first(asm):
    lib = asm.load_library()
    assert lib.asm_index_n_seqs(None) == 0 and lib.asm_index_seq_len(None, 0) == 0 and lib.asm_index_seq_name(None, 0) == b""
    assert lib.asm_index_get_text(None, None, 0, 0, None) == -1
    assert lib.asm_last_error(None).decode() == "asm_index_get_text: NULL argument"


if __name__ == "__main__":
    import sys

    sys.path.insert(0, ROOT)
    import approximate_string_matching_amd

    if "--record" in sys.argv:
        with open(GOLDEN, "w") as fh:
            json.dump(replay(approximate_string_matching_amd), fh, indent=1)
            fh.write("\n")
    else:
        print(json.dumps(replay(approximate_string_matching_amd), indent=1))
