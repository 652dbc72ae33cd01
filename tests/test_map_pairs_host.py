"""CPU checks of the mapper's paired-end contract (docs/design/mapper.md, "Paired-end reads"): the test-only rescue brute force
(tests/cxx/map_bruteforce_rescue.cpp) against a pure-Python DP, the Python pairing reference `bf_pairs` (the yardstick of
tests/test_gpu_map_pairs.py) on handcrafted pairs, and the argument checks of asm_map_pairs that need no device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from tests.test_map_all_host import bf_all, build_bruteforce_all
from tests.test_map_host import BASES, lev, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_bruteforce_rescue(tmp_dir):
    so = os.path.join(str(tmp_dir), "libmap_bf_rescue.so")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "cxx", "map_bruteforce_rescue.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = ctypes.CDLL(so)
    lib.map_bf_rescue.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                  ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    lib.map_bf_rescue.restype = ctypes.c_int
    return lib


def bf_rescue(lib, t, read, s, jlo, jhi, R):
    """-> (s, i, j, d) of the rescued locus of `read` on strand s over the ends [jlo, jhi] of t, or None"""
    out = np.zeros(4, np.int32)
    tb = t.encode() if isinstance(t, str) else t
    q = read.encode() if isinstance(read, str) else read
    if not lib.map_bf_rescue(tb, len(tb), q, len(q), s, jlo, jhi, R, out.ctypes.data):
        return None
    return tuple(int(v) for v in out)


def py_rescue(t, read, s, jlo, jhi, R):
    """The rule written out: D(j) over all starts by a semi-global DP from column 0, the smallest (D, j) over the clipped ends
    with D <= R and D < m, the largest start reaching D."""
    q = read.upper()
    q = revcomp(q) if s else q
    t = t.upper()
    m = len(q)
    col = list(range(m + 1))
    best = None
    for j in range(1, len(t) + 1):
        new = [0] * (m + 1)
        for a in range(1, m + 1):
            same = q[a - 1] == t[j - 1] and q[a - 1] in BASES
            new[a] = min(col[a - 1] + (0 if same else 1), col[a] + 1, new[a - 1] + 1)
        col = new
        d = col[m]
        if max(jlo, 1) <= j <= min(jhi, len(t)) and d <= R and d < m and (best is None or (d, j) < best):
            best = (d, j)
    if best is None:
        return None
    d, j = best
    i = next(i for i in range(j, -1, -1) if lev(q, t[i:j]) == d)
    return (s, i, j, d)


def pair_rank(a, b):
    """pair order of loci a (mate 1) and b (mate 2), each (s, r, i, j, d): (d_A + d_B, s_A, r, j_A, j_B)"""
    return (a[4] + b[4], a[0], a[1], a[3], b[3])


def concordant(a, b, m1, m2, lo, hi):
    if a[1] != b[1] or a[0] == b[0]:
        return False
    (F, mF), R = ((a, m1), b) if a[0] == 0 else ((b, m2), a)
    return lo <= R[3] - F[3] + mF <= hi


def bf_pairs(bfa, bfr, seqs, r1, r2, e, lo, hi, rescue=-1, k=12, loci=None):
    """The paired-end contract over bf_all's loci and the rescue brute force.  -> dict: `rec` = two records (s, r, i, j, d) or
    None (mate 1, mate 2), `proper`, `rescued` (None, 0 or 1: which mate), `n_concordant`, `tlen`.  loci: the two mates' loci
    lists if already known."""
    if loci is None:
        loci = [[] if len(q) < (e + 1) * k else bf_all(bfa, seqs, q, e) for q in (r1, r2)]
    L1, L2 = loci
    m1, m2 = len(r1), len(r2)
    conc = [(pair_rank(a, b), a, b) for a in L1 for b in L2 if concordant(a, b, m1, m2, lo, hi)]
    res = {"proper": False, "rescued": None, "n_concordant": 0}
    if conc:
        best = min(conc)
        res.update(rec=[best[1], best[2]], proper=True, n_concordant=sum(1 for c in conc if c[0][0] == best[0][0]))
    else:
        rec = [L1[0] if L1 else None, L2[0] if L2 else None]
        res["rec"] = rec
        if rescue >= 0:
            cands = []
            for x in (0, 1):
                X = rec[x]
                if X is None:
                    continue
                sX, r, jX = X[0], X[1], X[3]
                mX, mb = (m1, m2) if x == 0 else (m2, m1)
                b = (r2, r1)[x]
                if sX == 0:
                    jlo, jhi = jX - mX + lo, jX - mX + hi
                else:
                    jlo, jhi = jX + mb - hi, jX + mb - lo
                y = bf_rescue(bfr, seqs[r], b, 1 - sX, jlo, jhi, rescue)
                if y is None:
                    continue
                Y = (y[0], r, y[1], y[2], y[3])
                pair = [X, Y] if x == 0 else [Y, X]
                cands.append((pair_rank(*pair), pair, 1 - x))
            if cands:
                _, pair, who = min(cands)
                res.update(rec=pair, proper=True, rescued=who)
    a, b = res["rec"]
    res["tlen"] = max(a[3], b[3]) - min(a[2], b[2]) if a is not None and b is not None and a[1] == b[1] else 0
    return res


@pytest.fixture(scope="module")
def bfr(tmp_path_factory):
    return build_bruteforce_rescue(tmp_path_factory.mktemp("map_bf_rescue"))


@pytest.fixture(scope="module")
def bfa(tmp_path_factory):
    return build_bruteforce_all(tmp_path_factory.mktemp("map_bf_all_pairs"))


def test_rescue_bruteforce_agrees_with_python_dp(bfr):
    rng = random.Random(41)
    n_found = n_clip = n_trivial = 0
    for _ in range(300):
        t = "".join(rng.choice("ACGT" * 6 + "N" + "acgt") for _ in range(rng.randint(1, 40)))
        R = rng.randint(0, 4)
        m = rng.randint(1, 9)
        if rng.random() < 0.6 and len(t) >= 2:
            a = rng.randrange(len(t))
            q = t[a:a + m].upper() or "A"
            q = "".join(rng.choice(BASES) if rng.random() < 0.15 else c for c in q)
            s = rng.randrange(2)
            if s:
                q = revcomp(q)
        else:
            q = "".join(rng.choice("ACGTN") for _ in range(m))
            s = rng.randrange(2)
        jlo = rng.randint(-10, len(t) + 3)
        jhi = jlo + rng.randint(-2, 30)
        n_clip += jlo < 1 or jhi > len(t)
        got, want = bf_rescue(bfr, t, q, s, jlo, jhi, R), py_rescue(t, q, s, jlo, jhi, R)
        assert got == want, (t, q, s, jlo, jhi, R, got, want)
        n_found += got is not None
        # the D < m rule: with R >= m every end would qualify through the empty alignment
        n_trivial += R >= len(q) and got is None and max(jlo, 1) <= min(jhi, len(t))
    assert n_found > 80 and n_clip > 80 and n_trivial > 0


def test_rescue_bruteforce_edges(bfr):
    t = "ACGTTGCAAC"
    # exact copy ending at the sequence's last base; the window reaches past it and is clipped
    assert bf_rescue(bfr, t, "GCAAC", 0, 5, 40, 0) == (0, 5, 10, 0)
    # the reverse strand: revcomp("GTTGC") = "GCAAC"
    assert bf_rescue(bfr, t, "GTTGC", 1, -5, 40, 0) == (1, 5, 10, 0)
    # an end range below 1 is empty after clipping
    assert bf_rescue(bfr, t, "ACGT", 0, -5, 0, 3) is None
    # a mate of one base: D < m leaves only D = 0, i.e. an exact base
    assert bf_rescue(bfr, t, "A", 0, 1, 10, 15) == (0, 0, 1, 0)
    assert bf_rescue(bfr, t, "N", 0, 1, 10, 15) is None
    # the smallest (D, j): two exact copies, the first end wins; a window holding only the second finds it
    assert bf_rescue(bfr, "TTACGGATTACGGA", "ACGGA", 0, 1, 14, 1) == (0, 2, 7, 0)
    assert bf_rescue(bfr, "TTACGGATTACGGA", "ACGGA", 0, 8, 14, 1) == (0, 9, 14, 0)


# ---- bf_pairs on handcrafted pairs ---------------------------------------------------------------------------------------------
def rand_seq(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def place(seq, a, piece):
    return seq[:a] + piece + seq[a + len(piece):]


@pytest.fixture(scope="module")
def hand():
    """A 3-sequence reference and the mates' sources: mate 1 = S1 (50 bp), mate 2 = revcomp(S2) (40 bp)."""
    rng = random.Random(5)
    seqs = [rand_seq(rng, 3000) for _ in range(3)]
    S1, S2 = rand_seq(rng, 50), rand_seq(rng, 40)
    return seqs, S1, S2


def test_pair_span_bounds(bfa, bfr, hand):
    seqs, S1, S2 = hand
    s0 = place(place(seqs[0], 100, S1), 300, S2)  # F = mate 1 at [100, 150), R = mate 2 at [300, 340): L = 340 - 150 + 50 = 240
    ref = [s0, seqs[1], seqs[2]]
    r1, r2 = S1, revcomp(S2)
    for lo, hi in ((240, 400), (100, 240), (240, 240), (241, 400), (100, 239), (0, 8192)):
        got = bf_pairs(bfa, bfr, ref, r1, r2, 1, lo, hi, k=12)
        assert got["proper"] == ((lo <= 240 <= hi)) and got["rescued"] is None, (lo, hi)
        if got["proper"]:
            assert got["rec"] == [(0, 0, 100, 150, 0), (1, 0, 300, 340, 0)] and got["n_concordant"] == 1 and got["tlen"] == 240
        else:
            assert got["rec"] == [(0, 0, 100, 150, 0), (1, 0, 300, 340, 0)] and got["n_concordant"] == 0
    # with mate 2 given as the forward strand (F = mate 2), the same span: L = j_R - j_F + m_F with m_F = 40
    s1 = place(place(seqs[0], 100, S2), 300, revcomp(S1))  # F = mate 2 at [100, 140), R = mate 1 at [300, 350): L = 350 - 140 + 40
    got = bf_pairs(bfa, bfr, [s1, seqs[1], seqs[2]], S1, S2, 0, 250, 250)
    assert got["proper"] and got["rec"] == [(1, 0, 300, 350, 0), (0, 0, 100, 140, 0)] and got["tlen"] == 250


def test_same_strand_and_other_sequence_are_never_concordant(bfa, bfr, hand):
    seqs, S1, S2 = hand
    same = [place(place(seqs[0], 100, S1), 300, S2)] + seqs[1:]
    got = bf_pairs(bfa, bfr, same, S1, S2, 1, 0, 8192)  # both mates forward
    assert not got["proper"] and got["rec"][0][0] == got["rec"][1][0] == 0 and got["tlen"] == 240
    other = [place(seqs[0], 100, S1), place(seqs[1], 300, S2), seqs[2]]
    got = bf_pairs(bfa, bfr, other, S1, revcomp(S2), 1, 0, 8192)
    assert not got["proper"] and got["rec"][0][1] == 0 and got["rec"][1][1] == 1 and got["tlen"] == 0


def test_pair_order_tie_breaks(bfa, bfr, hand):
    seqs, S1, S2 = hand
    r1, r2 = S1, revcomp(S2)
    # d sum first: a pair with sum 0 beats one with sum 1 found earlier in (s, r, j); n_concordant counts sum 0 only
    S2m = S2[:20] + ("A" if S2[20] != "A" else "C") + S2[21:]
    ref = [place(place(place(place(seqs[0], 100, S1), 300, S2m), 1100, S1), 1300, S2)] + seqs[1:]
    got = bf_pairs(bfa, bfr, ref, r1, r2, 1, 0, 500)
    assert got["proper"] and got["rec"] == [(0, 0, 1100, 1150, 0), (1, 0, 1300, 1340, 0)] and got["n_concordant"] == 1
    # s_A before r and j: on sequence 0 an s_A = 1 pair (F = mate 2 at [100, 140), R = mate 1 at [300, 350)), on sequence 1 an
    # s_A = 0 pair further on; the s_A = 0 pair wins
    ref = [place(place(seqs[0], 100, r2), 300, revcomp(S1)), place(place(seqs[1], 2000, S1), 2200, S2), seqs[2]]
    got = bf_pairs(bfa, bfr, ref, r1, r2, 0, 0, 500)
    assert got["proper"] and got["n_concordant"] == 2 and got["rec"] == [(0, 1, 2000, 2050, 0), (1, 1, 2200, 2240, 0)], got
    # r before j: the same pair on sequence 2 at a small position and on sequence 1 at a larger one
    ref = [seqs[0], place(place(seqs[1], 2000, S1), 2200, S2), place(place(seqs[2], 100, S1), 300, S2)]
    got = bf_pairs(bfa, bfr, ref, r1, r2, 0, 0, 500)
    assert got["proper"] and got["n_concordant"] == 2 and got["rec"] == [(0, 1, 2000, 2050, 0), (1, 1, 2200, 2240, 0)]
    # j_A: two copies of the pair on one sequence
    ref = [place(place(place(place(seqs[0], 1500, S1), 1700, S2), 100, S1), 300, S2)] + seqs[1:]
    got = bf_pairs(bfa, bfr, ref, r1, r2, 0, 0, 500)
    assert got["proper"] and got["n_concordant"] == 2 and got["rec"] == [(0, 0, 100, 150, 0), (1, 0, 300, 340, 0)]
    # j_B: one mate 1 locus, two mate 2 loci in range
    ref = [place(place(place(seqs[0], 100, S1), 400, S2), 250, S2)] + seqs[1:]
    got = bf_pairs(bfa, bfr, ref, r1, r2, 0, 0, 500)
    assert got["proper"] and got["n_concordant"] == 2 and got["rec"] == [(0, 0, 100, 150, 0), (1, 0, 250, 290, 0)]


def test_rescue_rule(bfa, bfr, hand):
    seqs, S1, S2 = hand
    # mate 2 carries 3 substitutions: beyond e = 1, found by rescue with rescue_errors >= 3 only
    S2x = "".join(("A" if c != "A" else "C") if p in (5, 18, 31) else c for p, c in enumerate(S2))
    ref = [place(place(seqs[0], 100, S1), 300, S2x)] + seqs[1:]
    r1, r2 = S1, revcomp(S2)
    assert not bf_pairs(bfa, bfr, ref, r1, r2, 1, 0, 500)["proper"]
    assert not bf_pairs(bfa, bfr, ref, r1, r2, 1, 0, 500, rescue=2)["proper"]
    got = bf_pairs(bfa, bfr, ref, r1, r2, 1, 0, 500, rescue=3)
    assert got["proper"] and got["rescued"] == 1 and got["n_concordant"] == 0
    assert got["rec"] == [(0, 0, 100, 150, 0), (1, 0, 300, 340, 3)] and got["tlen"] == 240
    # the window: mate 2's end 340 is at L = 240; a max_insert below it leaves it out
    assert not bf_pairs(bfa, bfr, ref, r1, r2, 1, 0, 239, rescue=3)["proper"]
    # anchored on the reverse mate: mate 1 is the one beyond e
    S1x = "".join(("A" if c != "A" else "C") if p in (7, 22, 40) else c for p, c in enumerate(S1))
    ref = [place(place(seqs[0], 100, S1x), 300, S2)] + seqs[1:]
    got = bf_pairs(bfa, bfr, ref, r1, r2, 1, 240, 240, rescue=4)
    assert got["proper"] and got["rescued"] == 0 and got["rec"] == [(0, 0, 100, 150, 3), (1, 0, 300, 340, 0)]
    # a mate too short to seed is rescued too
    short = S2[-20:]
    got = bf_pairs(bfa, bfr, [place(place(seqs[0], 100, S1), 300, S2)] + seqs[1:], r1, revcomp(short), 1, 0, 500, rescue=0)
    assert got["proper"] and got["rescued"] == 1 and got["rec"][1] == (1, 0, 320, 340, 0)


def _err(asm):
    return asm.load_library().asm_last_error(None).decode()


def test_map_pairs_rejects_bad_arguments(asm):
    lib = asm.load_library()
    dummy = ctypes.create_string_buffer(64)  # never dereferenced: every check below fails first
    reads = b"ACGT" * 200
    ro = np.array([0, 100, 200], np.uint32)
    hits = np.zeros((2, 2), asm.MAP_HIT_DTYPE)
    tlen = np.zeros(2, np.int32)
    nc = np.zeros(2, np.uint32)
    ops = np.zeros(2 * 2 * 8, np.uint16)
    nops = np.zeros(2 * 2, np.uint8)
    ok, pok = asm.MapParams(2, 1, 0, 3), asm.PairParams(100, 500, 4)

    def call(p=ok, pp=pok, ro1=ro, ro2=ro, out=hits.ctypes.data, tl=tlen.ctypes.data, ncc=nc.ctypes.data, cap=0, c_ops=None,
             c_nops=None):
        return lib.asm_map_pairs(None, dummy, len(ro1) - 1, reads, ro1.ctypes.data, reads, ro2.ctypes.data, ctypes.byref(p),
                                 ctypes.byref(pp), out, tl, ncc, c_ops, cap, c_nops)

    assert call(p=asm.MapParams(2, 0, 0, 3)) == -1 and "both_strands" in _err(asm)
    assert call(pp=asm.PairParams(501, 500, 4)) == -1 and "insert" in _err(asm)
    assert call(pp=asm.PairParams(-1, 500, 4)) == -1 and "insert" in _err(asm)
    assert call(pp=asm.PairParams(0, asm.MAP_MAX_INSERT + 1, 4)) == -1 and "insert" in _err(asm)
    for r in (-2, 16):
        assert call(pp=asm.PairParams(100, 500, r)) == -1 and "rescue_errors" in _err(asm)
    for bad in (np.array([0, 100, 612], np.uint32), np.array([0, 0, 100], np.uint32)):
        assert call(ro1=bad) == -1 and "511" in _err(asm)
        assert call(ro2=bad) == -1 and "511" in _err(asm)
    for kw in ({"out": None}, {"tl": None}, {"ncc": None}):
        assert call(**kw) == -1 and "bad arguments" in _err(asm)
    assert lib.asm_map_pairs(None, dummy, 2, reads, ro.ctypes.data, None, ro.ctypes.data, ctypes.byref(ok), ctypes.byref(pok),
                             hits.ctypes.data, tlen.ctypes.data, nc.ctypes.data, None, 0, None) == -1 and "bad arguments" in _err(asm)
    assert lib.asm_map_pairs(None, dummy, 2, reads, ro.ctypes.data, reads, ro.ctypes.data, ctypes.byref(ok), None,
                             hits.ctypes.data, tlen.ctypes.data, nc.ctypes.data, None, 0, None) == -1 and "bad arguments" in _err(asm)
    assert call(cap=8) == -1 and "cigar" in _err(asm)
    assert call(cap=8, c_ops=ops.ctypes.data) == -1 and "cigar" in _err(asm)
    assert call(cap=-1) == -1 and "cigar" in _err(asm)
    for e in (-1, 16):
        assert call(p=asm.MapParams(e, 1, 0, 3)) == -1 and "max_errors" in _err(asm)
    # arguments fine (the edges of every range included): only the missing handle is left
    for pp in (asm.PairParams(0, 0, -1), asm.PairParams(0, asm.MAP_MAX_INSERT, 15), asm.PairParams(8192, 8192, 0)):
        assert call(pp=pp, cap=8, c_ops=ops.ctypes.data, c_nops=nops.ctypes.data) == -1 and "handle" in _err(asm)


def test_pair_constants(asm):
    import re

    hdr = open(os.path.join(ROOT, "include", "asm_mi355x.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (ASM_MAP_[A-Z_]+) (\d+)", hdr)}
    assert (val["ASM_MAP_PROPER_PAIR"], val["ASM_MAP_RESCUED"], val["ASM_MAP_MAX_INSERT"]) == \
        (asm.MAP_PROPER_PAIR, asm.MAP_RESCUED, asm.MAP_MAX_INSERT) == (64, 128, 8192)
    flags = (asm.MAP_MAPPED, asm.MAP_TOO_SHORT, asm.MAP_SEED_CAPPED, asm.MAP_CIGAR_TRUNCATED, asm.MAP_SECONDARY, asm.MAP_HITS_TRUNCATED,
             asm.MAP_PROPER_PAIR, asm.MAP_RESCUED)
    assert sum(flags) == 255 and len(set(flags)) == 8  # all eight bits of asm_map_hit.flags (uint8)
