"""CPU checks of the mapper's all-hits contract (docs/design/mapper.md, "All hits"): the test-only all-loci brute force
(tests/cxx/map_bruteforce_all.cpp, the yardstick of tests/test_gpu_map_all.py) against a pure-Python DP of the run rule, its
first locus against the single-best brute force, and the argument checks of asm_map_reads_all that need no device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from tests.test_map_host import BASES, _mutate, bf_map, build_bruteforce, lev, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_bruteforce_all(tmp_dir):
    so = os.path.join(str(tmp_dir), "libmap_bf_all.so")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "cxx", "map_bruteforce_all.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = ctypes.CDLL(so)
    lib.map_bf_all.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.c_void_p, ctypes.c_int]
    lib.map_bf_all.restype = ctypes.c_int
    return lib


def bf_all(lib, seqs, read, e, both=True):
    """-> every locus within e as (s, r, i, j, d), sorted by (d, s, r, j)"""
    text = "".join(seqs).encode()
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    q = read.encode() if isinstance(read, str) else read
    cap = 64
    while True:
        out = np.zeros(5 * cap, np.int32)
        n = lib.map_bf_all(text, off.ctypes.data, len(seqs), q, len(q), e, 1 if both else 0, out.ctypes.data, cap)
        if n <= cap:
            return [tuple(int(v) for v in out[5 * t:5 * t + 5]) for t in range(n)]
        cap = n


def py_all(seqs, read, e, both=True):
    """The run rule written out: D(j) by a semi-global DP, runs of consecutive ends with D <= e inside one (s, r), d = the run's
    minimum, j = its first end reaching d, i = the largest start with Lev = d."""
    q0 = read.upper()
    strands = [q0, revcomp(q0)] if both else [q0]
    loci = []
    for s, q in enumerate(strands):
        m = len(q)
        for r, t in enumerate(seqs):
            t = t.upper()
            col = list(range(m + 1))  # end 0: D = m > e
            run = None                # [d, j]
            for j in range(1, len(t) + 2):
                d = e + 1
                if j <= len(t):
                    new = [0] * (m + 1)
                    for a in range(1, m + 1):
                        same = q[a - 1] == t[j - 1] and q[a - 1] in BASES
                        new[a] = min(col[a - 1] + (0 if same else 1), col[a] + 1, new[a - 1] + 1)
                    col = new
                    d = col[m]
                if d <= e:
                    if run is None or d < run[0]:
                        run = [d, j]
                elif run is not None:
                    dd, jj = run
                    i = next(i for i in range(jj, -1, -1) if lev(q, t[i:jj]) == dd)
                    loci.append((dd, s, r, jj, i))
                    run = None
    return [(s, r, i, j, d) for d, s, r, j, i in sorted(loci)]


@pytest.fixture(scope="module")
def bf(tmp_path_factory):
    return build_bruteforce(tmp_path_factory.mktemp("map_bf_all_single"))


@pytest.fixture(scope="module")
def bfa(tmp_path_factory):
    return build_bruteforce_all(tmp_path_factory.mktemp("map_bf_all"))


# (seqs, read, e, both): the shapes the run rule has to get right
SPECIAL = [
    (["ACGTNACGTACGTNNNACGT"], "ACGTA", 1, True),                    # N runs: N never matches, not even N
    (["ttacggattACGGA"], "ACGGA", 0, True),                          # lower case, two exact copies in one sequence
    (["TTACGGATT", "ACGGA", "GGACGGA"], "ACGGA", 1, True),           # ties between sequences
    (["GGC" + "AC" * 20 + "TTG"], "ACACACAC", 1, False),              # a tandem repeat: its ends form one long run
    (["GGC" + "ACG" * 15 + "TTG"], "ACGACGAC", 2, True),              # period 3, both strands
    (["GGGGACGTAC", "ACGTACCCCC"], "ACGT", 3, False),                # a run ends on the last base of sequence 0, another
    (["TTTTTTACGT", "ACGTTTTTTT"], "ACGTAC", 2, True),               # starts on the first base of sequence 1: never merged
    (["", "NNNNNNNN", "ACGTTGCA"], "ACGTTGCA", 1, True),             # empty and N-only sequences
]


def test_bruteforce_all_agrees_with_python_dp(bfa):
    for seqs, read, e, both in SPECIAL:
        assert bf_all(bfa, seqs, read, e, both) == py_all(seqs, read, e, both), (seqs, read, e, both)
    rng = random.Random(17)
    for _ in range(250):
        seqs = []
        for _ in range(rng.randint(1, 3)):
            n = rng.randint(0, 24)
            s = "".join(rng.choice("ACGT" * 6 + "N" + "acgt") for _ in range(n))
            if rng.random() < 0.3 and n > 6:  # a duplicated segment: several loci, ties between sequences and positions
                s = s + s[:6]
            if rng.random() < 0.2:            # a short-period tandem stretch
                s = s + rng.choice(["AC", "AGT", "A"]) * rng.randint(3, 8)
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
        assert bf_all(bfa, seqs, read, e, both) == py_all(seqs, read, e, both), (seqs, read, e, both)


def test_run_rule_shapes(bfa):
    # the tandem repeat is one locus, not one per period
    assert len(bf_all(bfa, *SPECIAL[3][:3], both=False)) == 1
    # every end of both sequences is a hit end (D(10) of sequence 0 and D(1) of sequence 1 included), so the two runs touch in
    # the index text; they stay apart: one locus per sequence
    seqs = ["GGGGACGTAC", "ACGTACCCCC"]
    assert bf_all(bfa, seqs, "ACGT", 3, both=False) == [(0, 0, 4, 8, 0), (0, 1, 0, 4, 0)]
    assert min(lev("ACGT", seqs[0][i:]) for i in range(11)) <= 3 and lev("ACGT", seqs[1][:1]) <= 3
    # two exact copies, lower case: both found, the smaller end first
    assert bf_all(bfa, ["ttacggattACGGA"], "ACGGA", 0) == [(0, 0, 2, 7, 0), (0, 0, 9, 14, 0)]


def test_first_locus_is_the_best_hit(bf, bfa):
    rng = random.Random(23)
    cases = list(SPECIAL)
    for _ in range(150):
        seqs = ["".join(rng.choice("ACGT" * 4 + "N") for _ in range(rng.randint(5, 30))) for _ in range(rng.randint(1, 3))]
        e = rng.randint(0, 3)
        src = rng.choice(seqs)
        a = rng.randint(0, len(src) - 1)
        read = _mutate(rng, src[a:a + rng.randint(e + 1, 10)].upper(), rng.randint(0, e)).ljust(e + 1, "A")
        cases.append((seqs, read, e, rng.random() < 0.8))
    for seqs, read, e, both in cases:
        loci = bf_all(bfa, seqs, read, e, both)
        best = bf_map(bf, seqs, read, e, both)
        assert (best[0] == 1) == bool(loci), (seqs, read, e)
        if loci:
            assert best[1:] == loci[0], (seqs, read, e, both, best, loci[0])


def _err(asm):
    return asm.load_library().asm_last_error(None).decode()


def test_map_reads_all_rejects_bad_arguments(asm):
    lib = asm.load_library()
    dummy = ctypes.create_string_buffer(64)  # never dereferenced: every check below fails first
    reads = b"ACGT" * 200
    ro = np.array([0, 100], np.uint32)
    nh = np.zeros(2, np.uint32)
    hits = np.zeros((2, asm.MAP_MAX_HITS), asm.MAP_HIT_DTYPE)
    ops = np.zeros(2 * asm.MAP_MAX_HITS * 8, np.uint16)
    nops = np.zeros(2 * asm.MAP_MAX_HITS, np.uint8)
    ok = asm.MapParams(2, 1, 0, 3)

    def call(p=ok, ro=ro, strata=1, max_hits=4, n_hits=nh.ctypes.data, out=hits.ctypes.data, cap=0, c_ops=None, c_nops=None):
        return lib.asm_map_reads_all(None, dummy, len(ro) - 1, reads, ro.ctypes.data, ctypes.byref(p), strata, max_hits, n_hits, out,
                                     c_ops, cap, c_nops)

    for strata in (-1, 16):
        assert call(strata=strata) == -1 and "strata" in _err(asm)
    for max_hits in (0, 257):
        assert call(max_hits=max_hits) == -1 and "max_hits" in _err(asm)
    assert call(n_hits=None) == -1 and "bad arguments" in _err(asm)
    assert call(out=None) == -1 and "bad arguments" in _err(asm)
    assert call(cap=8) == -1 and "cigar" in _err(asm)
    assert call(cap=8, c_ops=ops.ctypes.data) == -1 and "cigar" in _err(asm)
    assert call(cap=-1) == -1 and "cigar" in _err(asm)
    for e in (-1, 16):
        assert call(p=asm.MapParams(e, 1, 0, 3)) == -1 and "max_errors" in _err(asm)
    assert call(p=asm.MapParams(2, 2, 0, 3)) == -1 and "both_strands" in _err(asm)
    assert call(p=asm.MapParams(2, 1, -1, 3)) == -1 and "max_occ" in _err(asm)
    assert call(p=asm.MapParams(2, 1, 0, 51)) == -1 and "greedy_k" in _err(asm)
    assert call(ro=np.array([0, 512], np.uint32)) == -1 and "511" in _err(asm)
    assert call(ro=np.array([0, 0], np.uint32)) == -1 and "511" in _err(asm)
    assert call(ro=np.array([0, 100, 50], np.uint32)) == -1 and "non-decreasing" in _err(asm)
    # arguments fine (the edges of every range included): only the missing handle is left
    for strata, max_hits in ((0, 1), (15, 256)):
        assert call(strata=strata, max_hits=max_hits, cap=8, c_ops=ops.ctypes.data, c_nops=nops.ctypes.data) == -1
        assert "handle" in _err(asm)


def test_flag_constants(asm):
    assert (asm.MAP_SECONDARY, asm.MAP_HITS_TRUNCATED, asm.MAP_MAX_HITS) == (16, 32, 256)
    flags = (asm.MAP_MAPPED, asm.MAP_TOO_SHORT, asm.MAP_SEED_CAPPED, asm.MAP_CIGAR_TRUNCATED, asm.MAP_SECONDARY, asm.MAP_HITS_TRUNCATED)
    assert sum(flags) == 63 and len(set(flags)) == 6  # distinct bits of asm_map_hit.flags (uint8)
