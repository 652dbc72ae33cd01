"""CPU proof of the yardsticks and inputs of tests/test_gpu_map_widths.py (tests/map_cases.py), so that the GPU module can assert
on every generated read: the full-matrix CIGAR reference `ref_cigar` against the brute-force mapper's hits, hand-written ties and
an exhaustive enumeration of optimal paths; and the coverage conditions of the generated reads, judged by the brute force alone
(tests/cxx/map_bruteforce.cpp).  The conditions are not measurements: the seeds in map_cases.class_reads are frozen so that they
hold."""
import itertools
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import map_cases as mc
from tests.test_gpu_map import strand_read, walk_cigar
from tests.test_map_host import BASES, bf_map, build_bruteforce, lev

UNMAPPED = (0, -1, -1, -1, -1, -1)


@pytest.fixture(scope="module")
def bf(tmp_path_factory):
    return build_bruteforce(tmp_path_factory.mktemp("map_bf_widths"))


@pytest.fixture(scope="module")
def seqs():
    return mc.reference_small()


@pytest.fixture(scope="module")
def sweep(bf, seqs):
    """(m, e) -> [(kind, read, brute-force tuple)] for every cell of the k = 8 sweep"""
    cells = [(W, m, e) for W in mc.LENGTHS_BY_W for m, e in mc.cells_of(W)]
    reads = {}
    for W in mc.LENGTHS_BY_W:
        for e in mc.errors_of(W):
            for kind, q in mc.class_reads(seqs, W, e):
                reads.setdefault((len(q), e), []).append((kind, q))
    flat = [(m, e, kind, q) for (W, m, e) in cells for kind, q in reads[(m, e)]]
    with ThreadPoolExecutor(16) as ex:
        hits = list(ex.map(lambda x: bf_map(bf, seqs, x[3], x[1]), flat))
    out = {}
    for (m, e, kind, q), h in zip(flat, hits):
        out.setdefault((m, e), []).append((kind, q, h))
    return out


def expand(cigar):
    return "".join(op * cnt for cnt, op in mc.cigar_ops(cigar))


def test_cells_and_lengths():
    assert all(mc.width_of(m) == W for W, ms in mc.LENGTHS_BY_W.items() for m in ms)
    assert mc.errors_of(1) == [0, 1, 3, 7] and all(mc.errors_of(W) == list(mc.E_SWEEP) for W in (2, 4, 8))
    assert (128, 15) in mc.cells_of(2) and (127, 15) not in mc.cells_of(2) and (8, 0) in mc.cells_of(1)
    for k, cells in mc.EXTRA_CELLS.items():
        assert all(mc.cell_exists(m, e, k) for m, e in cells)


def test_reference_small_layout(seqs):
    assert [len(seqs[t]) for t in mc.TINY] == [40, 200] and mc.TINY[1] == mc.TINY[0] + 1
    assert len(seqs[mc.SHORT]) == 50
    r, a, n = mc.N_RUN
    assert seqs[r][a:a + n] == "N" * n and "N" not in seqs[r][:a] + seqs[r][a + n:]
    assert any(c.islower() for c in seqs[0]) and any(c.islower() for c in seqs[3])
    assert seqs[7][8_000:9_500].upper() == seqs[3][5_000:6_500].upper()
    assert mc.STRADDLE[1] == mc.STRADDLE[0] + 1


def test_ref_cigar_hand_written_ties():
    # the gap goes as far left as the ties allow: walking back from the end the diagonal is taken first
    assert mc.ref_cigar("AAC", "AAAC") == "1D3M"
    assert mc.ref_cigar("AAAA", "AAA") == "1I3M"          # a homopolymer insertion
    assert mc.ref_cigar("AACAAAAG", "AACAAAG") == "3M1I4M"  # ... and inside a read: the first A of the run
    assert mc.ref_cigar("ACG", "") == "3I"                # an empty window: column 0 is all I
    assert mc.ref_cigar("TACG", "ACG") == "1I3M"
    assert mc.ref_cigar("ACG", "TTACG") == "2D3M"         # row 0 is all D
    assert mc.ref_cigar("CA", "AC") == "2M"              # two mismatches tie with a gap pair: the diagonal wins
    # N matches nothing, not even N
    assert mc.ref_cigar("ANG", "ANG") == "3M" and walk_cigar("3M", "ANG", "ANG") == (3, 3, 1)


def all_paths(q, w):
    """every monotone path from (m, n) back to (0, 0) as (ops walking back, cost) under the byte rule"""
    def go(a, b):
        if a == 0 and b == 0:
            yield "", 0
            return
        if a and b:
            sub = 0 if (q[a - 1] == w[b - 1] and q[a - 1] in BASES) else 1
            for p, c in go(a - 1, b - 1):
                yield "M" + p, c + sub
        if a:
            for p, c in go(a - 1, b):
                yield "I" + p, c + 1
        if b:
            for p, c in go(a, b - 1):
                yield "D" + p, c + 1
    return go(len(q), len(w))


def test_ref_cigar_is_the_first_optimal_path():
    """m, n <= 6: among all paths of minimal cost, the CIGAR is the smallest walking back from the end under M < I < D"""
    rng = random.Random(3)
    rank = {"M": 0, "I": 1, "D": 2}
    n_ties = 0
    for _ in range(400):
        alpha = rng.choice(("AC", "ACG", "ACGTN"))
        q = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 6)))
        w = "".join(rng.choice(alpha) for _ in range(rng.randint(0, 6)))
        paths = list(all_paths(q, w))
        d = min(c for _, c in paths)
        assert d == lev(q, w)
        best = [p for p, c in paths if c == d]
        n_ties += len(best) > 1
        first = min(best, key=lambda p: [rank[o] for o in p])
        cig = mc.ref_cigar(q, w)
        assert expand(cig)[::-1] == first, (q, w, cig, first)
        assert walk_cigar(cig, q, w) == (len(q), len(w), d)
    assert n_ties > 200


def test_ref_cigar_walks_the_brute_force_hits(seqs, sweep):
    """on the brute force's own (s, r, i, j, d): the CIGAR consumes m and j - i bases with d edits"""
    up = [s.upper() for s in seqs]
    n = 0
    for (m, e), rows in sorted(sweep.items()):
        for t, (kind, q, h) in enumerate(rows):
            if h[0] and (t % 4 == 0 or kind == "word_edge"):
                s, r, i, j, d = h[1:]
                qs = strand_read(q, s)
                assert walk_cigar(mc.ref_cigar(qs, up[r][i:j]), qs, up[r][i:j]) == (m, j - i, d), (m, e, kind, q)
                n += 1
    assert n > 700


def test_every_cell_reaches_its_error_bound(sweep):
    """e > 0: some read maps with d = e, one with a net shift of +e and one of -e ((j - i) - m), so the traceback reaches the
    outermost diagonals the cell allows (lanes 0 and 30 of the band at e = 15)"""
    assert len(sweep) == sum(len(mc.cells_of(W)) for W in mc.LENGTHS_BY_W) == 130
    for (m, e), rows in sorted(sweep.items()):
        if e == 0:
            continue
        mapped = [h for _, _, h in rows if h[0]]
        assert any(h[5] == e for h in mapped), (m, e)
        shifts = {(h[4] - h[3]) - m for h in mapped if h[5] == e}
        assert e in shifts and -e in shifts, (m, e, sorted(shifts))


def test_only_random_reads_may_be_unmapped(seqs, sweep):
    lens = [len(s) for s in seqs]
    for (m, e), rows in sorted(sweep.items()):
        for kind, q, h in rows:
            if kind == "random" or (kind == "with_N" and e == 0):
                continue
            if kind == "straddle":
                # inside one sequence, and never the exact copy that spans the two: a hit that touches the boundary costs the
                # bases of the other side (an exact copy elsewhere, likely at m = 8, is a hit like any other)
                if h[0]:
                    spans = (h[2] == mc.STRADDLE[0] and h[4] == lens[h[2]]) or (h[2] == mc.STRADDLE[1] and h[3] == 0)
                    assert 0 <= h[3] <= h[4] <= lens[h[2]] and (h[5] > 0 or not spans), (m, e, h)
                continue
            assert h[0], (m, e, kind, q)
            assert h[5] <= e
    kinds = {kind for rows in sweep.values() for kind, _, _ in rows}
    assert kinds == set(mc.KINDS)
    # the straddle reads do map once e allows dropping the smaller half
    assert any(h[0] and h[5] > 0 for rows in sweep.values() for kind, _, h in rows if kind == "straddle")
    # half of every kind is reverse-complemented, and both strands are hit
    strands = {h[1] for rows in sweep.values() for _, _, h in rows if h[0]}
    assert strands == {0, 1}


def test_sequence_edges_are_hit(seqs, sweep):
    """seq_start / seq_end: hits that begin at 0 or end at len_r, with d = e > 0 among them (the window and lo are clipped)"""
    lens = [len(s) for s in seqs]
    at_start = [(e, h) for (m, e), rows in sweep.items() for kind, _, h in rows if kind == "seq_start" and h[0] and h[3] == 0]
    at_end = [(e, h) for (m, e), rows in sweep.items() for kind, _, h in rows if kind == "seq_end" and h[0] and h[4] == lens[h[2]]]
    assert any(e == 15 and h[5] == 15 for e, h in at_start) and any(e == 15 and h[5] == 15 for e, h in at_end)
    assert len(at_start) > 100 and len(at_end) > 100


def test_every_word_boundary_carries_a_gap(seqs, sweep):
    up = [s.upper() for s in seqs]
    for W, ms in mc.LENGTHS_BY_W.items():
        for m in ms:
            seen = set()
            for e in mc.E_SWEEP:
                for kind, q, h in sweep.get((m, e), ()):
                    if kind in ("word_edge", "tail_junk") and h[0]:
                        s, r, i, j, d = h[1:]
                        seen |= mc.crossed_boundaries(mc.ref_cigar(strand_read(q, s), up[r][i:j]), m)
            assert seen >= set(mc.word_boundaries(m)), (m, sorted(seen))
    assert mc.word_boundaries(511) == [1, 2, 3, 4, 5, 6, 7] and mc.word_boundaries(65) == [1] and mc.word_boundaries(64) == []
    assert mc.crossed_boundaries("64M1D10M", 74) == {1} and mc.crossed_boundaries("63M2I9M", 74) == {1}
    assert mc.crossed_boundaries("63M1I10M", 74) == set() and mc.crossed_boundaries("65M1D9M", 74) == set()


def test_extra_cells_generate(seqs):
    for k, cells in mc.EXTRA_CELLS.items():
        for m, e in cells:
            rows = mc.edge_reads(seqs, m, e, k, random.Random(7))
            assert all(len(q) == m for _, q in rows) and {kind for kind, _ in rows} == set(mc.KINDS)
    again = [mc.class_reads(seqs, 2, 7) for _ in range(2)]
    assert again[0] == again[1]  # seeded: the same reads in every process
    assert list(itertools.chain.from_iterable(mc.short_reads(seqs, 31, random.Random(1))))[0] == "too_short"
