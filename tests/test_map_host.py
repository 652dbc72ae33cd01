"""CPU checks of the read mapper's contract (docs/design/mapper.md): the test-only brute-force mapper
(tests/cxx/map_bruteforce.cpp, the yardstick of tests/test_gpu_map.py) against a tiny pure-Python DP, and argument checks of
asm_index_build / asm_map_reads that need no device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = "ACGT"


def build_bruteforce(tmp_dir):
    so = os.path.join(str(tmp_dir), "libmap_bf.so")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "cxx", "map_bruteforce.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = ctypes.CDLL(so)
    lib.map_bf.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                           ctypes.c_void_p]
    lib.map_bf.restype = ctypes.c_int
    return lib


def bf_map(lib, seqs, read, e, both=True):
    text = "".join(seqs).encode()
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    out = np.zeros(6, np.int32)
    q = read.encode() if isinstance(read, str) else read
    assert lib.map_bf(text, off.ctypes.data, len(seqs), q, len(q), e, 1 if both else 0, out.ctypes.data) == 0
    return tuple(int(v) for v in out)


def revcomp(q):
    c = {"A": "T", "T": "A", "C": "G", "G": "C"}
    return "".join(c.get(ch, ch) for ch in reversed(q))


def lev(a, b):
    """unit edit distance under the mapper's byte rule"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            same = a[i - 1] == b[j - 1] and a[i - 1] in BASES
            cur[j] = min(prev[j - 1] + (0 if same else 1), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[-1]


def py_map(seqs, read, e, both=True):
    """(mapped, s, r, i, j, d) by the tie order: d, s, r, smallest j, largest i"""
    q0 = read.upper()
    strands = [q0, revcomp(q0)] if both else [q0]
    best = None
    for s, q in enumerate(strands):
        for r, t in enumerate(seqs):
            t = t.upper()
            for j in range(len(t) + 1):
                for i in range(j, -1, -1):  # largest i first
                    d = lev(q, t[i:j])
                    key = (d, s, r, j, -i)
                    if best is None or key < best:
                        best = key
    d, s, r, j, ni = best
    return (1, s, r, -ni, j, d) if d <= e else (0, -1, -1, -1, -1, -1)


@pytest.fixture(scope="module")
def bf(tmp_path_factory):
    return build_bruteforce(tmp_path_factory.mktemp("map_bf"))


def _mutate(rng, q, edits):
    q = list(q)
    for _ in range(edits):
        kind = rng.randrange(3)
        p = rng.randrange(len(q) + (kind == 1))
        if kind == 0 and q:
            q[p % len(q)] = rng.choice(BASES + "N")
        elif kind == 1:
            q.insert(p, rng.choice(BASES))
        elif len(q) > 1:
            del q[p % len(q)]
    return "".join(q)


def test_bruteforce_agrees_with_python_dp(bf):
    rng = random.Random(7)
    cases = 0
    for _ in range(300):
        seqs = []
        for _ in range(rng.randint(1, 3)):
            n = rng.randint(0, 24)
            s = "".join(rng.choice("ACGT" * 6 + "N" + "acgt") for _ in range(n))
            if rng.random() < 0.3 and n > 6:  # a duplicated segment: ties between sequences and positions
                s = s + s[:6]
            seqs.append(s)
        if not any(seqs):
            seqs[0] = "ACGTACGT"
        e = rng.randint(0, 3)
        m = rng.randint(e + 1, 9)
        if rng.random() < 0.6:
            src = rng.choice([s for s in seqs if s] or ["ACGT"])
            a = rng.randint(0, max(0, len(src) - 1))
            read = _mutate(rng, src[a:a + m].upper() or "A", rng.randint(0, e))
            if rng.random() < 0.5:
                read = revcomp(read)
        else:
            read = "".join(rng.choice("ACGTN") for _ in range(m))
        if len(read) <= e:
            read = read + "A" * (e + 1 - len(read))
        both = rng.random() < 0.8
        assert bf_map(bf, seqs, read, e, both) == py_map(seqs, read, e, both), (seqs, read, e, both)
        cases += 1
    assert cases == 300


def test_bruteforce_byte_rule_and_ties(bf):
    # N never matches, not even N
    assert bf_map(bf, ["ACGTNACGT"], "GTNAC", 0) == (0, -1, -1, -1, -1, -1)
    assert bf_map(bf, ["ACGTNACGT"], "GTNAC", 1)[5] == 1
    # identical copies in two sequences: the first sequence wins; inside it the smallest end
    assert bf_map(bf, ["TTACGGATT", "ACGGA"], "ACGGA", 0) == (1, 0, 0, 2, 7, 0)
    # forward before reverse at the same distance (a palindrome matches on both strands)
    assert bf_map(bf, ["GGACGTCC"], "ACGT", 0)[1] == 0
    # the largest start among those reaching d at the best end: AAC vs "AAAC" -> i = 1
    assert bf_map(bf, ["GAAAC"], "AAC", 1)[3:] == (2, 5, 0)
    # lower case is upper-cased
    assert bf_map(bf, ["ttacggatt"], "ACGGA", 0) == (1, 0, 0, 2, 7, 0)


def _err(asm):
    return asm.load_library().asm_last_error(None).decode()


def test_index_build_rejects_bad_arguments(asm):
    lib = asm.load_library()
    text = b"ACGTACGTACGTACGT"
    off = np.array([0, len(text)], np.uint64)
    out = ctypes.c_void_p()
    for k in (7, 15, 0):
        assert lib.asm_index_build(None, text, off.ctypes.data, 1, k, ctypes.byref(out)) == -1 and "k must" in _err(asm)
    assert lib.asm_index_build(None, text, off.ctypes.data, 0, 12, ctypes.byref(out)) == -1 and "n_seqs" in _err(asm)
    bad = np.array([0, 10, 5], np.uint64)
    assert lib.asm_index_build(None, text, bad.ctypes.data, 2, 12, ctypes.byref(out)) == -1 and "non-decreasing" in _err(asm)
    assert lib.asm_index_build(None, text, off.ctypes.data, 1, 12, ctypes.byref(out)) == -1 and "handle" in _err(asm)
    assert out.value is None


def test_map_reads_rejects_bad_arguments(asm):
    lib = asm.load_library()
    dummy = ctypes.create_string_buffer(64)  # never dereferenced: every check below fails first
    reads = b"ACGT" * 200
    ro = np.array([0, 100], np.uint32)
    hits = np.zeros(2, asm.MAP_HIT_DTYPE)

    def call(p, ro=ro, cap=0):
        return lib.asm_map_reads(None, dummy, len(ro) - 1, reads, ro.ctypes.data, ctypes.byref(p), hits.ctypes.data, None, cap, None)

    for e in (-1, 16):
        assert call(asm.MapParams(e, 1, 0, 3)) == -1 and "max_errors" in _err(asm)
    assert call(asm.MapParams(2, 2, 0, 3)) == -1 and "both_strands" in _err(asm)
    assert call(asm.MapParams(2, 1, -1, 3)) == -1 and "max_occ" in _err(asm)
    assert call(asm.MapParams(2, 1, 0, 51)) == -1 and "greedy_k" in _err(asm)
    assert call(asm.MapParams(2, 1, 0, 3), cap=8) == -1 and "cigar" in _err(asm)
    assert call(asm.MapParams(2, 1, 0, 3), ro=np.array([0, 512], np.uint32)) == -1 and "511" in _err(asm)
    assert call(asm.MapParams(2, 1, 0, 3), ro=np.array([0, 0], np.uint32)) == -1 and "511" in _err(asm)
    assert call(asm.MapParams(2, 1, 0, 3), ro=np.array([0, 100, 50], np.uint32)) == -1 and "non-decreasing" in _err(asm)
    assert call(asm.MapParams(4, 1, 0, 3)) == -1 and "handle" in _err(asm)  # arguments fine: only the missing handle is left


def test_fasta_fastq_readers(asm, tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">chr1 first one\nACGTN\nacgt\n>chr2\n\nGGCC\n")
    assert asm.read_fasta(str(fa)) == [("chr1", "ACGTNacgt"), ("chr2", "GGCC")]
    fq = tmp_path / "reads.fq"
    fq.write_text("@r1 extra\nACGT\n+\nIIII\n@r2\nGG\n+r2\n#!\n")
    assert asm.read_fastq(str(fq)) == [("r1", "ACGT", "IIII"), ("r2", "GG", "#!")]
    assert asm.read_fastq(str(fa)) == [("chr1", "ACGTNacgt", "*"), ("chr2", "GGCC", "*")]
