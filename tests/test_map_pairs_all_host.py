"""CPU checks of the mapper's secondary-pairs contract (docs/design/mapper.md, "Secondary pairs"): the Python reference
`bf_pairs_all` (the yardstick of tests/test_gpu_map_pairs_all.py, built on bf_all and bf_pairs) on handcrafted fragments, and the
argument checks of asm_map_pairs_all that need no device."""
import ctypes

import numpy as np
import pytest

from tests.test_map_all_host import bf_all, build_bruteforce_all
from tests.test_map_host import revcomp
from tests.test_map_pairs_host import bf_pairs, build_bruteforce_rescue, concordant, pair_rank, place, rand_seq


def bf_pairs_all(bfa, bfr, seqs, r1, r2, e, lo, hi, strata, max_pairs, rescue=-1, k=12, loci=None):
    """The secondary-pairs contract over bf_all's loci: bf_pairs' result (rank 0) plus `n_pairs` (the concordant pairs with
    d_A + d_B <= sum_best + strata), `pairs` (the first min(n_pairs, max_pairs) pairs in pair order, each [mate 1 locus, mate 2
    locus] as (s, r, i, j, d); [bf_pairs' records] when n_pairs is 0), `tlens` (one per listed pair) and `truncated`."""
    if loci is None:
        loci = [[] if len(q) < (e + 1) * k else bf_all(bfa, seqs, q, e) for q in (r1, r2)]
    base = bf_pairs(bfa, bfr, seqs, r1, r2, e, lo, hi, rescue, k, loci=loci)
    L1, L2 = loci
    conc = sorted((pair_rank(a, b), a, b) for a in L1 for b in L2 if concordant(a, b, len(r1), len(r2), lo, hi))
    elig = [[a, b] for rk, a, b in conc if rk[0] <= conc[0][0][0] + strata] if conc else []
    assert not elig or elig[0] == base["rec"]  # rank 0 is bf_pairs' pair
    res = dict(base)
    res["n_pairs"] = len(elig)
    res["pairs"] = [base["rec"]] + elig[1:max_pairs]
    res["tlens"] = [base["tlen"]] + [max(a[3], b[3]) - min(a[2], b[2]) for a, b in elig[1:max_pairs]]
    res["truncated"] = len(elig) > max_pairs
    return res


@pytest.fixture(scope="module")
def bfr(tmp_path_factory):
    return build_bruteforce_rescue(tmp_path_factory.mktemp("map_bf_rescue_all"))


@pytest.fixture(scope="module")
def bfa(tmp_path_factory):
    return build_bruteforce_all(tmp_path_factory.mktemp("map_bf_all_pairs_all"))


@pytest.fixture(scope="module")
def hand():
    """A 3-sequence reference and the mates' sources: S1 (50 bp), S2 (40 bp)."""
    import random

    rng = random.Random(9)
    seqs = [rand_seq(rng, 3000) for _ in range(3)]
    return seqs, rand_seq(rng, 50), rand_seq(rng, 40)


def test_ties_across_the_two_halves(bfa, bfr, hand):
    seqs, S1, S2 = hand
    r1, r2 = S1, revcomp(S2)
    # sequence 0: an s_A = 1 pair (mate 2 forward at [100, 140), mate 1 reverse at [300, 350)); sequence 1: an s_A = 0 pair.  Same
    # sum: s_A = 0 first although its r is larger
    ref = [place(place(seqs[0], 100, r2), 300, revcomp(S1)), place(place(seqs[1], 2000, S1), 2200, S2), seqs[2]]
    got = bf_pairs_all(bfa, bfr, ref, r1, r2, 0, 0, 500, 0, 16)
    assert got["n_pairs"] == got["n_concordant"] == 2 and not got["truncated"]
    assert got["pairs"] == [[(0, 1, 2000, 2050, 0), (1, 1, 2200, 2240, 0)], [(1, 0, 300, 350, 0), (0, 0, 100, 140, 0)]]
    assert got["tlens"] == [240, 250]


def test_s_a1_half_is_in_pair_order(bfa, bfr, hand):
    seqs, S1, S2 = hand
    r1, r2 = S1, revcomp(S2)
    # mate 2 forward (s = 0) at [100, 140) and [400, 440), mate 1 reverse (s = 1) at [450, 500) and [1000, 1050): all four
    # combinations are concordant in [0, 1000] (L = j_A - j_B + 40: 400, 100, 950, 650).  (r, j_B, j_A) order would list
    # (A1, B1), (A2, B1), (A1, B2), (A2, B2); pair order is (r, j_A, j_B).
    s0 = place(place(place(place(seqs[0], 100, r2), 400, r2), 450, revcomp(S1)), 1000, revcomp(S1))
    ref = [s0, seqs[1], seqs[2]]
    A1, A2, B1, B2 = (1, 0, 450, 500, 0), (1, 0, 1000, 1050, 0), (0, 0, 100, 140, 0), (0, 0, 400, 440, 0)
    got = bf_pairs_all(bfa, bfr, ref, r1, r2, 0, 0, 1000, 0, 16)
    assert got["n_pairs"] == 4 and got["pairs"] == [[A1, B1], [A1, B2], [A2, B1], [A2, B2]]
    assert got["tlens"] == [400, 100, 950, 650]
    # truncation at max_pairs: the first two, n_pairs uncapped
    got = bf_pairs_all(bfa, bfr, ref, r1, r2, 0, 0, 1000, 0, 2)
    assert got["n_pairs"] == 4 and got["truncated"] and got["pairs"] == [[A1, B1], [A1, B2]]
    got = bf_pairs_all(bfa, bfr, ref, r1, r2, 0, 0, 1000, 0, 1)
    assert got["n_pairs"] == 4 and got["truncated"] and got["pairs"] == [[A1, B1]] and got["rec"] == [A1, B1]
    got = bf_pairs_all(bfa, bfr, ref, r1, r2, 0, 0, 1000, 0, 4)
    assert got["n_pairs"] == 4 and not got["truncated"] and len(got["pairs"]) == 4


def test_several_loci_of_one_mate_and_strata(bfa, bfr, hand):
    seqs, S1, S2 = hand
    r1, r2 = S1, revcomp(S2)
    # one mate 1 locus at [100, 150), mate 2 at [250, 290), [300, 340) (one substitution) and [400, 440)
    S2m = S2[:20] + ("A" if S2[20] != "A" else "C") + S2[21:]
    ref = [place(place(place(place(seqs[0], 100, S1), 250, S2), 300, S2m), 400, S2)] + seqs[1:]
    A = (0, 0, 100, 150, 0)
    B1, B2, B3 = (1, 0, 250, 290, 0), (1, 0, 300, 340, 1), (1, 0, 400, 440, 0)
    # strata 0: the two pairs of sum 0; n_pairs == n_concordant
    got = bf_pairs_all(bfa, bfr, ref, r1, r2, 1, 0, 500, 0, 16)
    assert got["n_pairs"] == got["n_concordant"] == 2 and got["pairs"] == [[A, B1], [A, B3]]
    # strata 2e: sum 1 follows the sum-0 pairs although its j_B lies between theirs
    for strata in (1, 2):
        got = bf_pairs_all(bfa, bfr, ref, r1, r2, 1, 0, 500, strata, 16)
        assert got["n_pairs"] == 3 and got["n_concordant"] == 2 and got["pairs"] == [[A, B1], [A, B3], [A, B2]]
        assert got["tlens"] == [190, 340, 240]


def test_no_concordant_pair_means_no_secondary(bfa, bfr, hand):
    seqs, S1, S2 = hand
    # mate 2 beyond e, rescued: rank 0 is bf_pairs' rescued pair, n_pairs 0
    S2x = "".join(("A" if c != "A" else "C") if p in (5, 18, 31) else c for p, c in enumerate(S2))
    ref = [place(place(seqs[0], 100, S1), 300, S2x)] + seqs[1:]
    got = bf_pairs_all(bfa, bfr, ref, S1, revcomp(S2), 1, 0, 500, 2, 16, rescue=3)
    assert got["proper"] and got["rescued"] == 1 and got["n_pairs"] == 0 and got["pairs"] == [got["rec"]]
    # mates on different sequences: unpaired, n_pairs 0
    ref = [place(seqs[0], 100, S1), place(seqs[1], 300, S2), seqs[2]]
    got = bf_pairs_all(bfa, bfr, ref, S1, revcomp(S2), 1, 0, 8192, 2, 16)
    assert not got["proper"] and got["n_pairs"] == 0 and got["pairs"] == [got["rec"]] and got["tlens"] == [0]


def _err(asm):
    return asm.load_library().asm_last_error(None).decode()


def test_map_pairs_all_rejects_bad_arguments(asm):
    lib = asm.load_library()
    dummy = ctypes.create_string_buffer(64)  # never dereferenced: every check below fails first
    reads = b"ACGT" * 200
    ro = np.array([0, 100, 200], np.uint32)
    P = asm.MAP_MAX_HITS
    hits = np.zeros((2, P, 2), asm.MAP_HIT_DTYPE)
    tlen = np.zeros((2, P), np.int32)
    npairs = np.zeros(2, np.uint32)
    nc = np.zeros(2, np.uint32)
    ops = np.zeros(2 * P * 2 * 8, np.uint16)
    nops = np.zeros(2 * P * 2, np.uint8)
    ok, pok = asm.MapParams(2, 1, 0, 3), asm.PairParams(100, 500, 4)

    def call(p=ok, pp=pok, ro1=ro, ro2=ro, strata=4, max_pairs=16, n_pairs=npairs.ctypes.data, out=hits.ctypes.data,
             tl=tlen.ctypes.data, ncc=nc.ctypes.data, cap=0, c_ops=None, c_nops=None):
        return lib.asm_map_pairs_all(None, dummy, len(ro1) - 1, reads, ro1.ctypes.data, reads, ro2.ctypes.data, ctypes.byref(p),
                                     ctypes.byref(pp), strata, max_pairs, n_pairs, out, tl, ncc, c_ops, cap, c_nops)

    for strata in (-1, 31):
        assert call(strata=strata) == -1 and "strata" in _err(asm)
    for max_pairs in (0, 257):
        assert call(max_pairs=max_pairs) == -1 and "max_pairs" in _err(asm)
    assert call(n_pairs=None) == -1 and "n_pairs" in _err(asm)
    assert call(p=asm.MapParams(2, 0, 0, 3)) == -1 and "both_strands" in _err(asm)
    assert call(p=asm.MapParams(2, 1, -1, 3)) == -1 and "max_occ" in _err(asm)
    assert call(p=asm.MapParams(2, 1, 0, 51)) == -1 and "greedy_k" in _err(asm)
    for e in (-1, 16):
        assert call(p=asm.MapParams(e, 1, 0, 3)) == -1 and "max_errors" in _err(asm)
    for pp in (asm.PairParams(501, 500, 4), asm.PairParams(-1, 500, 4), asm.PairParams(0, asm.MAP_MAX_INSERT + 1, 4)):
        assert call(pp=pp) == -1 and "insert" in _err(asm)
    for r in (-2, 16):
        assert call(pp=asm.PairParams(100, 500, r)) == -1 and "rescue_errors" in _err(asm)
    for bad in (np.array([0, 100, 612], np.uint32), np.array([0, 0, 100], np.uint32)):
        assert call(ro1=bad) == -1 and "511" in _err(asm)
        assert call(ro2=bad) == -1 and "511" in _err(asm)
    assert call(ro1=np.array([0, 100, 50], np.uint32)) == -1 and "non-decreasing" in _err(asm)
    for kw in ({"out": None}, {"tl": None}, {"ncc": None}):
        assert call(**kw) == -1 and "bad arguments" in _err(asm)
    assert lib.asm_map_pairs_all(None, dummy, 2, reads, ro.ctypes.data, None, ro.ctypes.data, ctypes.byref(ok), ctypes.byref(pok), 4,
                                 16, npairs.ctypes.data, hits.ctypes.data, tlen.ctypes.data, nc.ctypes.data, None, 0,
                                 None) == -1 and "bad arguments" in _err(asm)
    assert lib.asm_map_pairs_all(None, dummy, 2, reads, ro.ctypes.data, reads, ro.ctypes.data, ctypes.byref(ok), None, 4, 16,
                                 npairs.ctypes.data, hits.ctypes.data, tlen.ctypes.data, nc.ctypes.data, None, 0,
                                 None) == -1 and "bad arguments" in _err(asm)
    assert call(cap=8) == -1 and "cigar" in _err(asm)
    assert call(cap=8, c_ops=ops.ctypes.data) == -1 and "cigar" in _err(asm)
    assert call(cap=-1) == -1 and "cigar" in _err(asm)
    # arguments fine (the edges of every range included): only the missing handle is left
    for strata, max_pairs in ((0, 1), (2 * asm.MAP_MAX_ERRORS, asm.MAP_MAX_HITS)):
        assert call(strata=strata, max_pairs=max_pairs, cap=8, c_ops=ops.ctypes.data, c_nops=nops.ctypes.data) == -1
        assert "handle" in _err(asm)
