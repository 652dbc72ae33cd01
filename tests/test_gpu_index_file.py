"""asm_index_build_file / Engine.build_index_file / asm-map --ref-stream (docs/design/mapper.md, "Reference: FASTA in, index out"): a
FASTA file parsed on the device must give the names, lengths and text of a parser written from the file's contract
(tests/fasta_cases.py), whatever the chunking, and an index that maps like the one asm_index_build makes from the same sequences.
The parser can only go wrong at the edges of a thread's 16 bytes, of a tile of T bytes and of a chunk: the shapes sit there."""
import os
import random
import signal
import subprocess

import numpy as np
import pytest

from tests import fasta_cases as fc
from tests.test_gpu_map import make_reads, make_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
NAMES = ["chrA", "chrB", "chrC"]
LIMIT = 300  # seconds per test


@pytest.fixture(autouse=True)
def time_limit():
    def over(signum, frame):
        raise TimeoutError("test ran longer than %d s" % LIMIT)

    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(LIMIT)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def check(engine, path, data, chunk_bytes=0, what=None):
    """the file through build_index_file against the parser -> the stats"""
    path.write_bytes(data)
    names, offs, text = fc.py_parse(data)
    index, st = engine.build_index_file(str(path), k=8, chunk_bytes=chunk_bytes)
    try:
        assert index.names == [n.decode("latin-1") for n in names], what
        assert index.lengths == fc.lengths(offs, len(text)), what
        got = index.text(0, len(text))
        assert got == text, (what, next(i for i in range(len(text)) if got[i] != text[i]))
        assert (st["n_seqs"], st["bases"], st["bytes_in"]) == (len(names), len(text), len(data)), what
        assert st["chunks"] >= 1 and st["seconds"] >= st["seconds_index"] >= 0 and st["seconds_read"] >= 0
    finally:
        index.free()
    return st


def test_text_names_and_lengths_equal_the_parser(asm, engine, tmp_path):
    data = fc.ugly_file(5, 30)
    names, offs, text = fc.py_parse(data)
    big = sorted(fc.lengths(offs, len(text)))[-3:]
    assert len(names) == 5 and all(1000 <= n <= 3000 for n in big) and 0 in fc.lengths(offs, len(text))
    chunks = {}
    for chunk_bytes in (0, 64, 100, 1000, 7777):
        chunks[chunk_bytes] = check(engine, tmp_path / "ref.fa", data, chunk_bytes)["chunks"]
    assert chunks[0] == 1 and chunks[64] > chunks[1000] > chunks[7777] >= 1
    # parts of the text, by global offsets
    index, _ = engine.build_index_file(str(tmp_path / "ref.fa"), k=8)
    for start, n in ((0, 0), (0, 1), (len(text) - 1, 1), (len(text), 0), (offs[2] - 5, 40), (17, 4097)):
        assert index.text(start, n) == text[start:start + n]
    with pytest.raises(asm.AsmError) as err:
        index.text(len(text) - 1, 2)
    assert err.value.code == -1 and "asm_index_get_text: the range must lie inside the text" in str(err.value)


def test_accessors_on_an_index_from_sequences(engine):
    seqs = ["acgtnACGT", "", "GGGTTTAAACCC" * 3]
    index = engine.build_index(seqs, k=8)
    assert index.names == ["", "", ""] and index.lengths == [9, 0, 36]
    lib = engine.lib
    assert lib.asm_index_n_seqs(index.ptr) == 3 and [lib.asm_index_seq_len(index.ptr, r) for r in (-1, 0, 1, 2, 3)] == [0, 9, 0, 36, 0]
    assert lib.asm_index_seq_name(index.ptr, 0) == b"" and lib.asm_index_seq_name(index.ptr, 7) == b""
    assert index.text(0, 45) == "".join(seqs).upper().encode() and index.text(5, 8) == b"ACGTGGGT"


def test_line_lengths_at_the_edges(asm, engine, tmp_path):
    T = asm.FASTA_TILE
    assert T % 16 == 0
    rng = random.Random(8)
    seq = fc.bases(rng, 3 * T + 5)
    for width in (1, 15, 16, 17, 60, T - 1, T, T + 1, len(seq)):
        for eol in ("\n", "\r\n"):
            for final in (True, False):
                body = eol.join(seq[a:a + width] for a in range(0, len(seq), width)) + (eol if final else "")
                data = (">s one sequence" + eol + body).encode()
                st = check(engine, tmp_path / "ref.fa", data, 0, (width, eol, final))
                assert st["bases"] == len(seq)
    # one line of 3 T + 5 bytes in chunks of 100: the long line did not become one slot
    st = check(engine, tmp_path / "ref.fa", (">s\n" + seq + "\n").encode(), 100, "unwrapped")
    assert st["chunks"] > 1 and st["chunks"] >= len(seq) // 100
    st = check(engine, tmp_path / "ref.fa", (">s\n" + seq).encode(), T + 1, "unwrapped, chunks of T + 1")
    assert st["chunks"] == 4  # 3 T + 8 bytes


def test_headers_at_the_edges(asm, engine, tmp_path):
    T = asm.FASTA_TILE
    rng = random.Random(9)
    path = tmp_path / "ref.fa"
    for at in (15, 16, 17, T - 1, T, T + 1, 2 * T - 1, 2 * T):
        # the second header's '>' at byte `at`: the last byte of a 16-byte group, of a tile, the first of the next
        data = (">a\n" + fc.bases(rng, at - 4) + "\n>b second\n" + fc.bases(rng, 40) + "\n").encode()
        assert data[at:at + 2] == b">b"
        check(engine, path, data, 0, at)
        st = check(engine, path, data, at, (at, "the header is the first byte of a chunk"))
        assert st["chunks"] >= 2
        # the same with the junk line in front of the FIRST header of the file ending there
        data = (fc.bases(rng, at - 1) + "\n>only\n" + fc.bases(rng, 33) + "\n").encode()
        assert data[at:at + 2] == b">o"
        check(engine, path, data, 0, (at, "junk before"))
        check(engine, path, data, 50, (at, "junk before, chunks of 50"))
    # a header longer than chunk_bytes and than the slot, which grows it; its name is the first word all the same
    name = fc.bases(rng, 6000, "abcXYZ_")
    data = (">first\nACGT\n> " + name + " rest of a long header " + "x" * 3000 + "\nacgtacgt\n").encode()
    st = check(engine, path, data, 64, "long header")
    assert st["chunks"] > 1
    # two adjacent headers, a header as the last line (with and without its newline), a '>' inside a sequence line
    check(engine, path, b">a\nAC\n>empty\n>b\nGT\n", 0, "adjacent")
    check(engine, path, b">a\nAC\n>empty\n>b\nGT\n", 7, "adjacent, chunks of 7")
    check(engine, path, b">a\nAC\n>last\n", 0, "header last")
    check(engine, path, b">a\nAC\n>last", 0, "header last, no newline")
    check(engine, path, b">a\nAC\n>last", 4, "header last, no newline, chunks of 4")
    check(engine, path, b">a\nAC>GT\n >x\nTT\n", 0, "'>' inside a line")
    check(engine, path, b">a\nAC>GT\n >x\nTT\n", 3, "'>' inside a line, chunks of 3")
    check(engine, path, b">\r\n\r\nac\r\n", 0, "empty name")


def same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("k", [8, 12])
def test_the_index_is_the_same_index(engine, tmp_path, k):
    ref = make_reference()
    fa = tmp_path / "ref.fa"
    with open(fa, "w") as fh:
        for nm, s in zip(NAMES, ref):
            fh.write(">%s some description\n" % nm)
            fh.write("".join(s[a:a + 60] + "\n" for a in range(0, len(s), 60)))
    from_file, st = engine.build_index_file(str(fa), k=k, chunk_bytes=100_000)
    from_seqs = engine.build_index(ref, k=k)
    assert from_file.names == NAMES and from_file.lengths == from_seqs.lengths == [len(s) for s in ref] and st["chunks"] >= 3
    reads = make_reads(ref, 2, 200, seed=61) + ["ACGT" * 5]
    a, b = engine.map_reads(from_file, reads, 2), engine.map_reads(from_seqs, reads, 2)
    same(a, b)
    assert a["mapped"].sum() > 150 and len(set(a["seq_id"][a["mapped"]].tolist())) == 3
    a, b = engine.map_reads_all(from_file, reads, 2, max_hits=4), engine.map_reads_all(from_seqs, reads, 2, max_hits=4)
    same(a, b)
    assert (a["n_hits"] >= 1).sum() > 150


def sam_lines(path):
    with open(path) as fh:
        return fh.read().splitlines()


@pytest.mark.parametrize("mode", [[], ["--stream"]])
def test_tool_with_a_streamed_reference_writes_the_same_sam(engine, tmp_path, mode):
    assert os.path.exists(EXE), "asm-map is built by build()"
    ref = make_reference()
    rng = random.Random(3)
    fa, fq = tmp_path / "ref.fa", tmp_path / "r.fq"
    with open(fa, "w") as fh:
        fh.write("not a header\n")
        for nm, s in zip(NAMES, ref):
            fh.write(">%s\tsome description\r\n" % nm)
            fh.write("".join(s[a:a + 60] + "\r\n" for a in range(0, len(s), 60)))
    with open(fq, "w") as fh:
        for t, q in enumerate(make_reads(ref, 2, 200, seed=67)):
            fh.write("@r%d\n%s\n+\n%s\n" % (t, q, "".join(chr(rng.randrange(33, 74)) for _ in q)))
    outs = []
    for extra in ([], ["--ref-stream"]):
        sam = tmp_path / ("o%d.sam" % len(outs))
        r = subprocess.run([EXE, "-r", str(fa), "-q", str(fq), "-o", str(sam), "-e", "2", "--both-strands"] + mode + extra,
                           capture_output=True, text=True, timeout=LIMIT)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append((sam_lines(sam), r.stderr))
    (plain, err0), (streamed, err1) = outs
    assert len(plain) == len(streamed) == 200 + 5 and [ln[:3] for ln in plain[:5]] == ["@HD", "@SQ", "@SQ", "@SQ", "@PG"]
    for a, b in zip(plain, streamed):
        if a.startswith("@PG"):
            assert b.startswith("@PG") and a.split("\tCL:")[0] == b.split("\tCL:")[0] and b.endswith(" --ref-stream")
        else:
            assert a == b
    assert sum(1 for ln in plain[5:] if not int(ln.split("\t")[1]) & 4) > 150
    assert err0.splitlines()[0] == err1.splitlines()[0]  # the summary line


def test_errors_leave_the_engine_usable(asm, engine, tmp_path):
    empty, plain, missing = tmp_path / "empty.fa", tmp_path / "plain.fa", tmp_path / "missing.fa"
    empty.write_bytes(b"")
    plain.write_bytes(b"ACGTACGT\nacgt\n" * 600)
    for path, message in ((empty, "no sequence in %s" % empty), (plain, "no sequence in %s" % plain), (missing, "cannot open %s" % missing)):
        for chunk_bytes in (0, 100):
            with pytest.raises(asm.AsmError) as err:
                engine.build_index_file(str(path), k=8, chunk_bytes=chunk_bytes)
            assert err.value.code == -1 and str(err.value).endswith("asm_index_build_file: " + message)
        check(engine, tmp_path / "good.fa", b">good\nACGTACGTACGT\n", 0, path.name)
