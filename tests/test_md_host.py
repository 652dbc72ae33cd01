"""The device-free side of the MD:Z tag (docs/design/mapper.md, "MD tag"): the yardstick ref_md (tests/md_cases.py) against an
exhaustive check of its own, the rule the kernel compiles (csrc/asm_md.h) and the SAM formatter's MD piece (csrc/asm_sam.h) built
for the host under ASan + UBSan against ref_md, the C ABI's host helper asm_md_format and Python's md_format, and the argument
checks of asm_md_format and asm_map_set_sam_tags."""
import ctypes
import itertools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import map_cases
from tests.md_cases import MD_MAX, MD_RE, check_md, inserted, letter, md_letters, ref_md
from tests.test_map_file_host import san_flags
from tests.test_map_host import BASES, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
MD_CAP = 80  # ASM_MAP_MD_CAP


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
def paths(m, n):
    """every sequence of M, I and D columns that consumes m read and n reference bytes"""
    if m == 0 and n == 0:
        yield ""
        return
    if m and n:
        for p in paths(m - 1, n - 1):
            yield p + "M"
    if m:
        for p in paths(m - 1, n):
            yield p + "I"
    if n:
        for p in paths(m, n - 1):
            yield p + "D"


def runs_of(cols):
    return "".join("%d%s" % (len(list(g)), op) for op, g in itertools.groupby(cols))


# what a column can hold: (read byte, reference byte, is it an edit)
M_KINDS = (("A", "A", 0), ("C", "G", 1), ("N", "N", 1), ("T", "*", 1))
I_KINDS = "AN"
D_KINDS = ("T", "-")


def spell(cols, pick):
    """the read, the window and the edits of a column sequence whose t-th column holds kind pick(t, choices)"""
    q, w, edits = [], [], 0
    for t, op in enumerate(cols):
        if op == "M":
            a, b, x = M_KINDS[pick(t, len(M_KINDS))]
            q.append(a), w.append(b)
            edits += x
        elif op == "I":
            q.append(I_KINDS[pick(t, len(I_KINDS))])
            edits += 1
        else:
            w.append(D_KINDS[pick(t, len(D_KINDS))])
            edits += 1
    return "".join(q), "".join(w), edits


def test_ref_md_exhaustive_small():
    """Every column sequence with m, n <= 6; every filling of the columns for m, n <= 3, the two uniform fillings and a seeded
    one beyond.  The tag has the contract's syntax, read + CIGAR + MD give the window back (a byte outside A-Z as N), and the
    letters of the tag plus the inserted bases are the edits."""
    rng = random.Random(3)
    seen = 0
    for m in range(7):
        for n in range(7):
            for cols in paths(m, n):
                if m <= 3 and n <= 3:
                    sizes = [len(M_KINDS) if op == "M" else len(I_KINDS) if op == "I" else len(D_KINDS) for op in cols]
                    fills = [lambda t, k, c=c: c[t] for c in itertools.product(*[range(s) for s in sizes])]
                else:
                    fills = [lambda t, k: 0, lambda t, k: 1] + [lambda t, k, r=random.Random(rng.random()): r.randrange(k) for _ in range(1)]
                for pick in fills:
                    q, w, edits = spell(cols, pick)
                    cigar = runs_of(cols)
                    md = ref_md(cigar, q, w)
                    check_md(cigar, q, w, md, dist=edits)
                    seen += 1
    assert seen > 50_000


def test_ref_md_hand_cases():
    assert ref_md("5M", "ACGTA", "ACGTA") == "5"
    assert ref_md("5M", "TCGTA", "ACGTA") == "0A4" and ref_md("5M", "ACGTC", "ACGTA") == "4A0"
    assert ref_md("2M2D2M", "ACGA", "ACACTA") == "2^AC0T1"      # a mismatch right behind a deletion
    assert ref_md("3M2D2M", "ACTGA", "ACGACGA") == "2G0^AC2"    # a deletion right behind a mismatch
    assert ref_md("2I3M", "TTACG", "ACG") == "3" and ref_md("3M2I", "ACGTT", "ACG") == "3"
    assert ref_md("3M", "ANG", "ANG") == "1N1"
    assert ref_md("3M1D1M", "ACGT", "A*G-T") == "1N1^N1"


# ---- the rule and the formatter on the CPU -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def md_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("md_check") / "md_host_check_asan")
    src = os.path.join(PKG, "host", "md_host_check.cpp")
    assert os.path.exists(src), "host/md_host_check.cpp: the host build of the MD rule"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def encode(cigar):
    return [cnt << 3 | "MID".index(op) for cnt, op in map_cases.cigar_ops(cigar)]


def spaced_deletions(rng, runs):
    """single deleted reference bases between matched runs of the given lengths; a deleted base differs from both neighbours, so
    the CIGAR is the only one"""
    q, w, cigar = [], [], []
    for t, n in enumerate(runs):
        s = "".join(rng.choice(BASES) for _ in range(n))
        q.append(s), w.append(s)
        if n:
            cigar.append("%dM" % n)
        if t + 1 < len(runs):
            w.append("N")  # a letter that is no base: it can be no copy of a neighbour
            cigar.append("1D")
    return "".join(cigar), "".join(q), "".join(w)


@pytest.fixture(scope="module")
def cases():
    """(label, cigar, q_s, window, strand, dist or None).  Recipes: tests/map_cases.py's mid_edit over reference_small() at the
    lengths on both sides of every kernel width, 0, 3 and 15 edits of every kind, both strands, the CIGAR by ref_cigar.  Then the
    hand cases."""
    out = []
    seqs = [s.upper() for s in map_cases.reference_small()]
    rng = random.Random(41)
    for m in (31, 64, 65, 128, 129, 256, 257, 511):
        for x in (0, 3, 15):
            for kind in ("ins", "del", "sub"):
                for strand in (0, 1):
                    src, a = map_cases._source(rng, seqs, m + x + 2)
                    q, span = map_cases.mid_edit(rng, src[a:a + m + x + 2], m, x, kind)
                    window = src[a:a + span]
                    dist = int(map_cases.ref_matrix(q, window)[-1, -1])
                    out.append(("%s m=%d x=%d s=%d" % (kind, m, x, strand), map_cases.ref_cigar(q, window), q, window, strand, dist))
    r, a, n = map_cases.N_RUN  # a read whose tail lies over the reference's run of N: N against N, and a read with N of its own
    w = seqs[r][a - 60:a + 4]
    out.append(("N run", "64M", w, w, 0, 4))
    out.append(("N in the read", "64M", w[:10] + "N" + w[11:], w, 1, 5))
    hand = [("all match", "8M", "ACGTACGT", "ACGTACGT", 0), ("first column", "8M", "TCGTACGT", "ACGTACGT", 1),
            ("last column", "8M", "ACGTACGA", "ACGTACGT", 1), ("first and last", "8M", "CCGTACGA", "ACGTACGT", 2),
            ("deletion before a mismatch", "2M2D2M", "ACGA", "ACACTA", 3), ("deletion behind a mismatch", "3M2D2M", "ACTGA", "ACGACGA", 3),
            ("insertion at the head", "2I6M", "TTACGTAC", "ACGTAC", 2), ("insertion at the tail", "6M2I", "ACGTACTT", "ACGTAC", 2),
            ("N against N", "5M", "ACNGT", "ACNGT", 1), ("a star in the reference", "5M1D2M", "ACGTAGT", "AC*TA-GT", 2),
            ("every column a mismatch", "15M", "A" * 15, "C" * 15, 15)]
    for label, cigar, q, w, d in hand:
        for strand in (0, 1):
            out.append((label + " s=%d" % strand, cigar, q, w, strand, d))
    # the longest tags: 15 single deletions.  With m <= 511, the mapper's longest read, 16 runs cannot all have three digits
    # (that needs m >= 1600): 4 runs of 100, 11 of 10 and 1 of 1 bases, or 3 of 100 and 13 of 10, give the most digits, 35, and a
    # tag of 35 + 15 + 15 = 65 bytes.  The rule itself does not know m: 16 runs of 100 reach the bound, 78.
    rng = random.Random(43)
    out.append(("longest at m = 511",) + spaced_deletions(rng, [100, 10, 10, 100, 10, 10, 10, 100, 10, 10, 10, 100, 10, 10, 10, 1]) + (0, 15))
    out.append(("longest at m = 511, strand 1",) + spaced_deletions(rng, [10] * 6 + [100] * 3 + [10] * 7) + (1, 15))
    out.append(("the bound: 16 runs of 100",) + spaced_deletions(rng, [100] * 16) + (0, 15))
    out.append(("the bound: runs of 999",) + spaced_deletions(rng, [999] * 16) + (1, 15))
    return out


def run_md_check(exe, tmp_path, rows):
    """rows: (ops, strand, forward read, window) -> [(ok, tag, line or None)]"""
    blob = [struct.pack("<I", len(rows))]
    for ops, strand, fwd, window in rows:
        blob.append(struct.pack("<I%dH" % len(ops), len(ops), *ops))
        blob.append(struct.pack("<II", strand, len(fwd)) + fwd.encode("latin-1"))
        blob.append(struct.pack("<I", len(window)) + window.encode("latin-1"))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    data, at, out = dst.read_bytes(), 0, []
    for _ in rows:
        ok, n = struct.unpack_from("<II", data, at)
        tag = data[at + 8:at + 8 + n].decode("latin-1")
        at += 8 + n
        (size,) = struct.unpack_from("<Q", data, at)
        line = data[at + 8:at + 8 + size].decode("latin-1")
        at += 8 + size
        out.append((ok, tag, line if ok else None))
    assert at == len(data)
    return out


def py_line(cigar, qs, strand, nops, tag):
    """the line md_host_check formats: read "r" on "chr" at POS 6, dist 3, greedy_cost -2 (MAPQ 58), no QUAL"""
    return "r\t%d\tchr\t6\t58\t%s\t*\t0\t0\t%s\t*\tNM:i:3\tXG:i:-2%s\n" % (16 if strand else 0, cigar if nops <= 64 else "*", qs, "\tMD:Z:" + tag if tag else "")


def test_md_host_check_equals_ref_md(md_check, tmp_path, cases):
    rows = [(encode(cigar), strand, revcomp(q) if strand else q, w) for _, cigar, q, w, strand, _ in cases]
    got = run_md_check(md_check, tmp_path, rows)
    longest = 0
    for (label, cigar, q, w, strand, dist), (ok, tag, line) in zip(cases, got):
        want = ref_md(cigar, q, w)
        assert len(want) <= MD_MAX, (label, len(want))
        check_md(cigar, q, w, want, dist=dist)
        assert ok == 1 and tag == want, (label, cigar, tag, want)
        assert line == py_line(cigar, q, strand, len(encode(cigar)), want), label  # size = bytes at every lane, MD behind XG
        longest = max(longest, len(want))
    assert longest == MD_MAX
    assert max(len(ref_md(c, q, w)) for label, c, q, w, _, _ in cases if "m = 511" in label) == 65
    assert sum(1 for _, c, _, _, s, _ in cases if s == 1 and "D" in c and "I" not in c) >= 8


def test_md_host_check_refuses_rows_that_do_not_fit(md_check, tmp_path):
    """rows no finish kernel writes: the rule reads nothing outside the read and the window (ASan watches) and says no; a tag
    longer than the row is not stored beyond it"""
    rows = [(encode("5M"), 0, "ACGT", "ACGTA"), (encode("5M"), 0, "ACGTA", "ACGT"), (encode("4M"), 1, "ACGTA", "ACGT"),
            (encode("4M"), 0, "ACGT", "ACGTA"), (encode("2M9I"), 0, "ACGT", "AC"), (encode("2M9D"), 0, "AC", "ACGT"),
            ([4 << 3 | 3], 0, "ACGT", "ACGT"), ([8191 << 3 | 0] * 3, 0, "ACGT", "ACGT"),
            (encode("60M"), 0, "A" * 60, "C" * 60)]  # 60 mismatches: 121 bytes
    for ok, tag, line in run_md_check(md_check, tmp_path, rows):
        assert ok == 0 and tag == "" and line is None


# ---- the C ABI's host helper ---------------------------------------------------------------------------------------------------------
def c_md_format(lib, ops, q, w, cap=MD_CAP, read_len=None, ref_len=None):
    row = np.asarray(ops, np.uint16)
    out = ctypes.create_string_buffer(b"\xaa" * (cap + 16), cap + 16)
    n = lib.asm_md_format(row.ctypes.data if row.size else None, int(row.size), q.encode(), len(q) if read_len is None else read_len,
                          w.encode(), len(w) if ref_len is None else ref_len, out, cap)
    assert out.raw[cap:] == b"\xaa" * 16, "asm_md_format wrote beyond out_cap"
    return n, out.raw[:max(n, 0)].decode("latin-1"), out.raw


def test_asm_md_format_equals_ref_md(asm, cases):
    lib = asm.load_library()
    for label, cigar, q, w, strand, dist in cases:
        want = ref_md(cigar, q, w)
        n, tag, raw = c_md_format(lib, encode(cigar), q, w)
        assert n == len(want) and tag == want and raw[n] == 0, label
        assert asm.md_format(cigar, q, w) == want and asm.md_format(encode(cigar), q.encode(), w.encode()) == want, label
    # lower case on either side is the mapper's upper case
    assert asm.md_format("2M2D2M", "acga", "acacta") == "2^AC0T1"


def test_asm_md_format_rejections(asm):
    lib = asm.load_library()
    EINVAL = -1
    ops = np.asarray(encode("2M2D2M"), np.uint16)
    q, w, want = b"ACGA", b"ACACTA", b"2^AC0T1"
    out = ctypes.create_string_buffer(MD_CAP)
    good = lambda **kw: dict(dict(ops=ops.ctypes.data, nops=3, q=q, m=4, w=w, n=6, out=out, cap=MD_CAP), **kw)  # noqa: E731

    def call(a):
        return lib.asm_md_format(a["ops"], a["nops"], a["q"], a["m"], a["w"], a["n"], a["out"], a["cap"])

    assert call(good()) == len(want) and out.value == want
    for bad in (dict(ops=None), dict(q=None), dict(w=None), dict(out=None), dict(nops=-1), dict(m=-1), dict(n=-1)):
        assert call(good(**bad)) == EINVAL, bad
        assert lib.asm_last_error(None) == b"asm_md_format: bad arguments"
    for bad in (dict(m=3), dict(m=5, q=q + b"C"), dict(n=5), dict(n=7, w=w + b"A"), dict(nops=2)):
        assert call(good(**bad)) == EINVAL, bad
        assert b"consume exactly" in lib.asm_last_error(None)
    other = np.asarray([4 << 3 | 3], np.uint16)  # '=' is no operation of the mapper's rows
    assert lib.asm_md_format(other.ctypes.data, 1, b"ACGT", 4, b"ACGT", 4, out, MD_CAP) == EINVAL
    # out_cap: the tag and its NUL must fit; one byte less is refused and nothing behind out_cap is written
    n, tag, raw = c_md_format(lib, encode("2M2D2M"), "ACGA", "ACACTA", cap=len(want) + 1)
    assert n == len(want) and tag == want.decode()
    n, _, _ = c_md_format(lib, encode("2M2D2M"), "ACGA", "ACACTA", cap=len(want))
    assert n == EINVAL and lib.asm_last_error(None) == b"asm_md_format: out_cap is too small"
    assert c_md_format(lib, encode("2M2D2M"), "ACGA", "ACACTA", cap=0)[0] == EINVAL
    # nothing to align: the tag of an empty row is "0"
    assert lib.asm_md_format(None, 0, None, 0, None, 0, out, MD_CAP) == 1 and out.value == b"0"
    with pytest.raises(asm.AsmError):
        asm.md_format("4M", "ACG", "ACGT")
    with pytest.raises(ValueError):
        asm.md_format("4M1X", "ACGTA", "ACGTA")


def test_sam_tags_rejections(asm):
    lib = asm.load_library()
    assert asm.SAM_TAG_MD == 1 and asm.MAP_MD_CAP == MD_CAP
    assert lib.asm_map_set_sam_tags(None, 2) == -1
    assert lib.asm_last_error(None) == b"asm_map_set_sam_tags: mask may hold ASM_SAM_TAG_MD (1) only"
    assert lib.asm_map_set_sam_tags(None, 3) == -1 and b"mask may hold" in lib.asm_last_error(None)  # the mask is checked first
    assert lib.asm_map_set_sam_tags(None, 1) == -1 and lib.asm_last_error(None) == b"asm_map_set_sam_tags: NULL handle"
    assert lib.asm_map_set_sam_tags(None, 0) == -1
    assert lib.asm_map_get_sam_tags(None) == 0
    with open(asm.HEADER_PATH) as fh:
        header = fh.read()
    assert "#define ASM_SAM_TAG_MD 1" in header and "#define ASM_MAP_MD_CAP 80" in header


def test_letters_and_syntax_helpers():
    assert letter("a") == "N" and letter("*") == "N" and letter("R") == "R"
    assert md_letters("2^AC0T1") == 3 and inserted("2I3M1I") == 3
    assert MD_RE.fullmatch("0") and not MD_RE.fullmatch("A0") and not MD_RE.fullmatch("3^5")
