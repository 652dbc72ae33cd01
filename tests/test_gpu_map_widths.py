"""The read mapper at every kernel width, at the word edges and over the whole error range (docs/design/mapper.md, "Tests").

map_with_width picks the template width W in {1, 2, 4, 8} of map_verify_kernel, map_verify_all_kernel, map_finish_kernel and
map_rescue_kernel from the longest read of the device chunk.  Every test here sends the reads of one width class per call
(tests/map_cases.py: LENGTHS_BY_W, lengths on both sides of every word edge), so that each instantiation meets the brute force
(tests/cxx/map_bruteforce*.cpp) on its own, with e over E_SWEEP = (0, 1, 3, 7, 8, 12, 15) at k = 8, and compares every CIGAR as
a string with the contract's full-matrix traceback (map_cases.ref_cigar).  tests/test_map_widths_host.py proves on the CPU that
the generated reads reach d = e, net shifts of +e and -e and a gap at every word boundary, so nothing here is skipped: every
generated read is asserted.

Cells (a length m is searchable at e when m >= (e + 1) k; the other lengths of the class are sent too and must come back
TOO_SHORT):
  k = 8   W = 1: e in {0, 1, 3, 7}   (8: e = 0; 31: e <= 1; 63: e <= 3; 64: e <= 7)
          W = 2: e in {0, 1, 3, 7, 8, 12, 15}   (65: e <= 7; 100: e <= 8; 127: e <= 12; 128: all)
          W = 4, W = 8: every e of E_SWEEP at every length
  k = 14  (m, e) = (64, 3), (128, 8), (256, 15), (511, 15)
  k = 12  (m, e) = (63, 3), (128, 8), (193, 15), (449, 15); the all-hits, rescue and file tests run at k = 12 too, on the
          references of the older modules: W = 1: e in {0, 1, 3}; W = 2: e in {0, 1, 3, 7, 8}; W = 4, W = 8: all"""
import random
import signal
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np
import pytest

from tests import map_cases as mc
from tests import test_gpu_map_all as tall
from tests import test_gpu_map_file as tfile
from tests import test_gpu_map_pairs as tpairs
from tests.map_cases import mid_edit, pair_reads
from tests.test_gpu_map import got_tuple, make_reference, strand_read, walk_cigar
from tests.test_map_all_host import build_bruteforce_all
from tests.test_map_host import BASES, bf_map, build_bruteforce, revcomp
from tests.test_map_pairs_host import build_bruteforce_rescue

pytestmark = pytest.mark.gpu
LIMIT = 600  # seconds per test
WIDTHS = (1, 2, 4, 8)
FIELDS = ("seq_id", "pos", "end", "dist", "strand", "flags", "greedy_cost")
# (W, e, k, lengths): the k = 8 sweep, then the extra cells one length at a time
CELLS = [(W, e, mc.K_SWEEP, None) for W in WIDTHS for e in mc.errors_of(W)]
CELLS += [(mc.width_of(m), e, k, (m,)) for k in sorted(mc.EXTRA_CELLS) for m, e in mc.EXTRA_CELLS[k]]
SWEEP = [c for c in CELLS if c[3] is None]
ALL_CELLS = [(W, e) for W in WIDTHS for e in mc.errors_of(W, 12)]


def cell_id(c):
    return "W%d-e%d-k%d" % c[:3] + ("-m%d" % c[3][0] if c[3] else "")


@pytest.fixture(autouse=True)
def time_limit():
    def over(signum, frame):
        raise TimeoutError("test ran longer than %d s" % LIMIT)

    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(LIMIT)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def bf(tmp_path_factory):
    return build_bruteforce(tmp_path_factory.mktemp("map_bf_widths_gpu"))


@pytest.fixture(scope="module")
def bfa(tmp_path_factory):
    return build_bruteforce_all(tmp_path_factory.mktemp("map_bf_all_widths_gpu"))


@pytest.fixture(scope="module")
def bfr(tmp_path_factory):
    return build_bruteforce_rescue(tmp_path_factory.mktemp("map_bf_rescue_widths_gpu"))


@pytest.fixture(scope="module")
def seqs():
    return mc.reference_small()


@pytest.fixture(scope="module")
def indices(engine, seqs):
    """index of reference_small() per k, built on first use"""
    built = {}

    def get(k):
        if k not in built:
            built[k] = engine.build_index(seqs, k=k)
        return built[k]

    yield get
    for ix in built.values():
        ix.free()


@pytest.fixture(scope="module")
def big():
    return make_reference()


@pytest.fixture(scope="module")
def big_index(engine, big):
    ix = engine.build_index(big, k=12)
    yield ix
    ix.free()


def upper(seqs):
    return [x.upper() for x in seqs]


@lru_cache(maxsize=None)
def cigar_of(qs, window):
    return mc.ref_cigar(qs, window)


@pytest.fixture(scope="module")
def cells(engine, indices, bf, seqs):
    """cell -> its reads with their kinds, one map_reads call over them and the brute force's answers.  Module-scoped: the mixed-call
    and cigar_cap tests compare with the very call the per-cell tests check."""
    done = {}

    def get(c):
        if c not in done:
            W, e, k, lengths = c
            rows = mc.class_reads(seqs, W, e, k, lengths)
            reads = [q for _, q in rows]
            assert all(mc.width_of(len(q)) == W for q in reads)  # the call's longest read is of this class: map_with_width picks W
            out = engine.map_reads(indices(k), reads, e)
            with ThreadPoolExecutor(16) as ex:
                want = list(ex.map(lambda q: bf_map(bf, seqs, q, e), reads))
            done[c] = {"kinds": [kind for kind, _ in rows], "reads": reads, "out": out, "want": want}
        return done[c]

    return get


def greedy_pairs(reads, up, out, idx):
    pairs = []
    for t in idx:
        s, r, i = int(out["strand"][t]), int(out["seq_id"][t]), int(out["pos"][t])
        w = i - 1 if i else 0
        pairs.append((strand_read(reads[t], s), up[r][w:min(w + len(reads[t]) + 1, len(up[r]))]))
    return pairs


@pytest.mark.parametrize("c", CELLS, ids=cell_id)
def test_each_width_equals_brute_force(asm, engine, oracle, cells, seqs, c):
    W, e, k, _ = c
    x = cells(c)
    reads, out, want = x["reads"], x["out"], x["want"]
    up = upper(seqs)
    n_mapped = 0
    for t, q in enumerate(reads):
        short = len(q) < (e + 1) * k
        assert bool(out["flags"][t] & asm.MAP_TOO_SHORT) == short, (t, len(q))
        assert not out["flags"][t] & (asm.MAP_SEED_CAPPED | asm.MAP_CIGAR_TRUNCATED)
        assert got_tuple(out, t) == ((0, -1, -1, -1, -1, -1) if short else want[t]), (t, x["kinds"][t], q, got_tuple(out, t), want[t])
        if not out["mapped"][t]:
            assert out["cigar"][t] == "" and out["cigar_nops"][t] == 0 and out["greedy_cost"][t] == -1 and out["mapq"][t] == 255
            continue
        n_mapped += 1
        s, r, i, j, d = want[t][1:]
        qs = strand_read(q, s)
        assert walk_cigar(out["cigar"][t], qs, up[r][i:j]) == (len(q), j - i, d), (t, out["cigar"][t])
    # what tests/test_map_widths_host.py proves of the inputs: only these kinds may stay unmapped
    for t, q in enumerate(reads):
        may_miss = x["kinds"][t] in ("random", "straddle", "too_short") or (x["kinds"][t] == "with_N" and e == 0)
        assert out["mapped"][t] or may_miss or len(q) < (e + 1) * k, (t, x["kinds"][t], q)
    assert n_mapped
    # Greedy on the contract's window; MAPQ = min(254, 60 + cost)
    idx = np.nonzero(out["mapped"])[0]
    costs = oracle.greedy(asm.HostBatch.from_strings(greedy_pairs(reads, up, out, idx)), k=3, mode=1)
    assert np.array_equal(out["greedy_cost"][idx], costs)
    assert np.array_equal(out["mapq"][idx], np.minimum(254, 60 + costs))


@pytest.mark.parametrize("c", SWEEP, ids=cell_id)
def test_cigar_is_the_contracts(asm, engine, indices, cells, seqs, c):
    """every CIGAR equals, as a string, the full-matrix traceback that prefers the diagonal, then I, then D"""
    W, e, k, _ = c
    x = cells(c)
    reads, out = x["reads"], x["out"]
    up = upper(seqs)
    n = 0
    for t in np.nonzero(out["mapped"])[0]:
        s, r, i, j = (int(out[key][t]) for key in ("strand", "seq_id", "pos", "end"))
        assert out["cigar"][t] == cigar_of(strand_read(reads[t], s), up[r][i:j]), (t, x["kinds"][t], reads[t])
        assert out["cigar_nops"][t] == len(mc.cigar_ops(out["cigar"][t]))
        n += 1
    assert n
    allh = engine.map_reads_all(indices(k), reads, e, max_hits=4, strata=e)
    assert allh["read"].size >= n
    for h in range(allh["read"].size):
        t, s, r, i, j = (int(allh[key][h]) for key in ("read", "strand", "seq_id", "pos", "end"))
        assert allh["cigar"][h] == cigar_of(strand_read(reads[t], s), up[r][i:j]), (h, t, reads[t])
    # both mates of map_pairs, rescued records included
    r1s, r2s = pair_reads(seqs, mc.LENGTHS_BY_W[W], e, k, seed=31 * W + e)
    pout = engine.map_pairs(indices(k), r1s, r2s, e, 0, 1400, rescue_errors=15)
    for t in range(len(r1s)):
        for y, q in enumerate((r1s[t], r2s[t])):
            if pout["mapped"][t, y]:
                s, r, i, j, d = (int(pout[key][t, y]) for key in ("strand", "seq_id", "pos", "end", "dist"))
                qs = strand_read(q, s)
                assert pout["cigar"][t][y] == cigar_of(qs, up[r][i:j]), (t, y, q)
                assert walk_cigar(pout["cigar"][t][y], qs, up[r][i:j]) == (len(q), j - i, d)
    assert pout["proper"].sum() >= len(r1s) // 3
    if e:
        assert pout["rescued"].any()


@pytest.mark.parametrize("e", [1, 7])
def test_mixed_call_equals_per_width_calls(engine, indices, cells, e):
    """all classes in one call (the short reads run in the W = 8 launch with nw < W), and in chunks that fall into different
    classes: every field and CIGAR equals the per-class call's"""
    per_class = [cells((W, e, mc.K_SWEEP, None)) for W in WIDTHS]
    reads = [q for x in per_class for q in x["reads"]]
    n1 = len(per_class[0]["reads"])
    for chunk in (None, n1, 29):
        out = engine.map_reads(indices(mc.K_SWEEP), reads, e, chunk=chunk)
        lo = 0
        for x in per_class:
            hi = lo + len(x["reads"])
            for key in FIELDS + ("mapq", "cigar_nops"):
                assert np.array_equal(out[key][lo:hi], x["out"][key]), (chunk, key)
            assert out["cigar"][lo:hi] == x["out"]["cigar"], chunk
            lo = hi


def plain_reads(seqs, lengths, e, per_length, seed):
    """reads of the given lengths from any reference: spaced substitutions, an inserted or a deleted run in the middle (e edits, at
    most m / 8),
    a random read, a read with an N; half of them reverse-complemented, some lower case"""
    rng = random.Random(seed)
    up = [s.upper() for s in seqs]
    reads = []
    for m in lengths:
        for v in range(per_length):
            kind = ("sub", "ins", "del", "random", "N", "sub")[v % 6]
            if kind == "random":
                reads.append("".join(rng.choice(BASES) for _ in range(m)))
                continue
            while True:
                r = rng.randrange(len(up))
                a = rng.randrange(len(up[r]) - m - 40)
                if "N" not in up[r][a:a + m + 40]:
                    break
            q, _ = mid_edit(rng, up[r][a:a + m + 40], m, min(e, m // 8), "sub" if kind == "N" else kind)
            if kind == "N":
                q = q[:m // 3] + "N" + q[m // 3 + 1:]
            q = revcomp(q) if rng.random() < 0.5 else q
            reads.append(q.lower() if v % 5 == 4 else q)
    return reads


def repeat_reads_at(rep, lengths, seed):
    """reads of the given lengths from the repeat reference of tests/test_gpu_map_all.py: over copies of the 500 bp element
    (with their flanks when m > 500) and inside the period-6 tandem repeat, where the hit ends of neighbouring windows merge"""
    seqs, elem = rep
    rng = random.Random(seed)
    up = [s.upper() for s in seqs]
    unit, tr, t0, copies = tall.TANDEM
    reads = []
    for m in lengths:
        for v in range(2):
            a = 2000 + 800 * rng.randrange(60) + (rng.randrange(500 - m) if m < 500 else -rng.randrange(12))
            q = up[0][a:a + m]
            reads.append(revcomp(q) if v else q)
        for v in range(2):
            a = t0 + rng.randrange(len(unit) * copies - m)
            reads.append(up[tr][a:a + m])
    return [q.replace("N", "A") for q in reads]


@pytest.fixture(scope="module")
def rep():
    return tall.make_repeat_reference()


@pytest.fixture(scope="module")
def rep_index(engine, rep):
    ix = engine.build_index(rep[0], k=12)
    yield ix
    ix.free()


@pytest.mark.parametrize("W,e", ALL_CELLS, ids=["W%d-e%d" % c for c in ALL_CELLS])
def test_all_hits_each_width(asm, engine, bfa, rep, rep_index, W, e):
    seqs, elem = rep
    k = rep_index.k
    lengths = mc.LENGTHS_BY_W[W]
    reads = plain_reads(seqs, lengths, e, 5, seed=900 + 16 * W + e) + repeat_reads_at(rep, lengths, seed=950 + 16 * W + e)
    assert mc.width_of(max(len(q) for q in reads)) == W
    want = tall.brute_force_all(bfa, seqs, reads, e)
    up = upper(seqs)
    best = engine.map_reads(rep_index, reads, e)
    n_many = 0
    for strata in sorted({0, e}):
        for max_hits in (1, 64):
            out = engine.map_reads_all(rep_index, reads, e, max_hits=max_hits, strata=strata)
            got, idx = tall.per_read(out, len(reads))
            for t, q in enumerate(reads):
                short = len(q) < (e + 1) * k
                assert bool(out["read_flags"][t] & asm.MAP_TOO_SHORT) == short, t
                nh, loci = tall.expected([] if short else want[t], e, strata, max_hits)
                assert out["n_hits"][t] == nh and out["n_reported"][t] == len(loci), (t, q, strata, max_hits, out["n_hits"][t], nh)
                assert got[t] == loci, (t, q, strata, max_hits, got[t], loci)
                n_many += nh > 1
                for rank, h in enumerate(idx[t]):
                    fl = int(out["flags"][h])
                    assert fl & asm.MAP_MAPPED and bool(fl & asm.MAP_SECONDARY) == (rank > 0)
                    assert bool(fl & asm.MAP_HITS_TRUNCATED) == (nh > max_hits)
                    s, r, i, j, d = got[t][rank]
                    assert out["cigar"][h] == cigar_of(strand_read(q, s), up[r][i:j]), (t, rank, q)
                # rank 0 is map_reads' record
                if idx[t]:
                    h = idx[t][0]
                    for key in FIELDS:
                        a = int(out[key][h]) & ~asm.MAP_HITS_TRUNCATED if key == "flags" else int(out[key][h])
                        assert a == int(best[key][t]), (t, key)
                    assert out["cigar"][h] == best["cigar"][t] and out["mapq"][h] == best["mapq"][t]
                else:
                    assert not best["mapped"][t] and out["read_flags"][t] == best["flags"][t]
    assert n_many or all(len(q) < (e + 1) * k for q in reads)


MATES = ((64, 64), (128, 128), (256, 256), (511, 511), (63, 449))


def rescue_pairs(seqs, m1, m2, f, seed):
    """12 fragments of f bases; one mate is an exact copy (the anchor), the other has 3, 8 or 15 edits as a substitution set, an
    inserted run or a deleted run and keeps its outer end, so only the rescue finds it.  A third of the fragments start within
    20 bases of a sequence's start with the reverse mate as the anchor, a third end at a sequence's end with the forward mate as
    the anchor: the allowed ends are clipped to [1, len_r]."""
    rng = random.Random(seed)
    up = [s.upper() for s in seqs]
    r1s, r2s = [], []
    for t in range(12):
        x, kind = (3, 8, 15, 15)[t // 3], ("sub", "ins", "del", "ins")[t % 4]
        where = t % 3 if t < 9 else 2
        r = (1, 2, 0)[t % 3]
        L = len(up[r])
        while True:
            a = 16 + t if where == 0 else L - f if where == 1 else rng.randrange(1000, L - f - 1000)
            if "N" not in up[r][max(0, a - 40):a + f + 40]:
                break
        edit_left = where == 0 or (where == 2 and t % 2 == 0)
        ml, mr = (m1, m2) if t % 2 else (m2, m1)  # lengths of the left (forward) and the right (reverse) mate
        mx = ml if edit_left else mr
        span = mx + (x if kind == "del" else -x if kind == "ins" else 0)
        if edit_left:  # the edited mate keeps its end a + ml
            left, _ = mid_edit(rng, up[r][a + ml - span:a + ml + 40], ml, x, kind)
            right = up[r][a + f - mr:a + f]
        else:          # the edited mate keeps its end a + f
            right, _ = mid_edit(rng, up[r][a + f - span:a + f + 40], mr, x, kind)
            left = up[r][a:a + ml]
        assert len(left) == ml and len(right) == mr
        q1, q2 = (left, revcomp(right)) if t % 2 else (revcomp(right), left)  # mate 1 is the one of m1 bases
        r1s.append(q1)
        r2s.append(q2)
    return r1s, r2s


@pytest.mark.parametrize("m1,m2", MATES, ids=["%dx%d" % m for m in MATES])
def test_rescue_each_width(asm, engine, oracle, bfa, bfr, big, big_index, m1, m2):
    """map_rescue_kernel<W> per width: rescued mates with up to 15 errors in indel runs, insert ranges of 1, 127, 128 and 129 ends
    (the tile edges) and one that is no multiple of 128, anchors near both ends of a sequence"""
    e = 2
    f = m1 + m2 + 37
    r1s, r2s = rescue_pairs(big, m1, m2, f, seed=m1 + m2)
    assert all(len(a) == m1 and len(b) == m2 for a, b in zip(r1s, r2s))
    loci = tpairs.all_loci(bfa, big, r1s + r2s, e)
    up = upper(big)
    n_resc = n_far = n_shift = 0
    for lo, hi in ((f, f), (f - 63, f + 63), (f - 64, f + 63), (f - 64, f + 64), (f - 100, f + 600)):
        assert (hi - lo + 1) in (1, 127, 128, 129, 701)
        want = tpairs.expected(bfa, bfr, big, r1s, r2s, e, 15, loci=loci, lo=lo, hi=hi)
        out = engine.map_pairs(big_index, r1s, r2s, e, lo, hi, rescue_errors=15)
        tpairs.check(asm, out, want, r1s, r2s, e, ("rescue", m1, m2, lo, hi))
        tpairs.check_alignments(asm, oracle, out, big, r1s, r2s)
        for t in range(len(r1s)):
            for y, q in enumerate((r1s[t], r2s[t])):
                if out["mapped"][t, y]:
                    s, r, i, j, d = (int(out[key][t, y]) for key in ("strand", "seq_id", "pos", "end", "dist"))
                    assert out["cigar"][t][y] == cigar_of(strand_read(q, s), up[r][i:j]), (t, y, q)
                    if out["rescued"][t, y]:
                        n_resc += 1
                        n_far += d == 15
                        n_shift += d == 15 and abs((j - i) - len(q)) == 15
    assert n_resc >= 30 and n_far >= 5 and n_shift >= 2, (n_resc, n_far, n_shift)


def test_cigar_cap_truncation(asm, engine, indices, cells):
    """cigar_cap below, at and above the number of operations R: CIGAR_TRUNCATED iff R > cap, cigar_nops = R, the first
    min(R, cap) operations are written, nothing else changes"""
    by_R = {}
    for c in ((2, 7, mc.K_SWEEP, None), (8, 15, mc.K_SWEEP, None)):
        x = cells(c)
        for t in np.nonzero(x["out"]["mapped"])[0]:
            R = int(x["out"]["cigar_nops"][t])
            if 3 <= R <= 31 and len(by_R.setdefault((c, R), [])) < 4:
                by_R[(c, R)].append(int(t))
    assert len({R for _, R in by_R}) >= 8 and max(R for _, R in by_R) == 31  # del_spread at e = 15: 16 M and 15 D
    for (c, R), ts in sorted(by_R.items()):
        x = cells(c)
        e, k = c[1], c[2]
        reads = [x["reads"][t] for t in ts]
        full = [mc.cigar_ops(x["out"]["cigar"][t]) for t in ts]
        assert all(len(ops) == R for ops in full)
        for cap in sorted({1, 2, R - 1, R, R + 1}):
            out = engine.map_reads(indices(k), reads, e, cigar_cap=cap)
            for u, t in enumerate(ts):
                assert bool(out["flags"][u] & asm.MAP_CIGAR_TRUNCATED) == (R > cap), (R, cap)
                assert out["cigar_nops"][u] == R
                assert mc.cigar_ops(out["cigar"][u]) == full[u][:min(R, cap)], (R, cap, out["cigar"][u])
                for key in FIELDS:
                    a = int(out[key][u]) & ~asm.MAP_CIGAR_TRUNCATED if key == "flags" else int(out[key][u])
                    assert a == int(x["out"][key][t]), (key, R, cap)
        # once for map_reads_all: the flag is per record
        cap = R - 1
        ref = engine.map_reads_all(indices(k), reads, e, max_hits=4, strata=e)
        out = engine.map_reads_all(indices(k), reads, e, max_hits=4, strata=e, cigar_cap=cap)
        assert np.array_equal(ref["read"], out["read"]) and np.array_equal(ref["cigar_nops"], out["cigar_nops"])
        for h in range(out["read"].size):
            ops = mc.cigar_ops(ref["cigar"][h])
            assert len(ops) == ref["cigar_nops"][h]
            assert bool(out["flags"][h] & asm.MAP_CIGAR_TRUNCATED) == (len(ops) > cap)
            assert mc.cigar_ops(out["cigar"][h]) == ops[:cap]
            for key in FIELDS:
                a = int(out[key][h]) & ~asm.MAP_CIGAR_TRUNCATED if key == "flags" else int(out[key][h])
                assert a == int(ref[key][h]), (key, h)
        assert (out["flags"][out["rank"] == 0] & asm.MAP_CIGAR_TRUNCATED).all()


def test_cigar_cap_keeps_the_next_row(asm, engine, indices, cells):
    """A truncated CIGAR must not reach into the next record's row.  Nothing the library returns shows such a store directly: the row
    after a truncated one belongs to a record whose own thread writes its first operation later (in the same wave always: that
    store follows every lane's traceback loop), or to an unmapped record whose row is not read.  So this test arranges a race the
    stray store loses: one 511 bp read with 15 operations in the last lane of the block's first wave, and 64 bp single-operation
    reads everywhere else.  The second wave does an eighth of the first wave's work, so record 64 has written its own `64M` long
    before the long read's traceback reaches its second operation; a store into row 64 after that stays visible.  A correct
    kernel passes whatever the timing."""
    e, k = 7, mc.K_SWEEP
    lng, sht = cells((8, e, k, None)), cells((1, e, k, None))
    lt = next(t for t, q in enumerate(lng["reads"]) if len(q) == 511 and lng["out"]["cigar_nops"][t] == 15)
    st = next(t for t, q in enumerate(sht["reads"]) if len(q) == 64 and sht["out"]["cigar"][t] == "64M")
    src = [(lng, lt) if u == 63 else (sht, st) for u in range(128)]
    reads = [x["reads"][t] for x, t in src]
    for cap in (1, 2, 14, 15):
        out = engine.map_reads(indices(k), reads, e, cigar_cap=cap)
        for u, (x, t) in enumerate(src):
            full = mc.cigar_ops(x["out"]["cigar"][t])
            assert out["cigar_nops"][u] == len(full) and bool(out["flags"][u] & asm.MAP_CIGAR_TRUNCATED) == (len(full) > cap)
            assert mc.cigar_ops(out["cigar"][u]) == full[:cap], (u, cap, out["cigar"][u])
            assert (out["pos"][u], out["end"][u], out["dist"][u]) == (x["out"]["pos"][t], x["out"]["end"][t], x["out"]["dist"][t])


@pytest.mark.parametrize("W", [1, 2])
def test_map_file_at_each_width(engine, big, big_index, tmp_path, W):
    """a FASTQ whose longest read is of class W: parsed, mapped and formatted on the device, byte for byte the lines formatted
    from Engine.map_reads / map_reads_all"""
    reads = plain_reads(big, mc.LENGTHS_BY_W[W], 2, 24, seed=70 + W)
    assert mc.width_of(max(len(q) for q in reads)) == W
    recs = tfile.records_for(reads, seed=W)
    fq, sam = tmp_path / "r.fq", tmp_path / "o.sam"
    tfile.write_fastq(fq, recs)
    for max_hits in (0, 3):
        for chunk_bytes in (0, 3000):
            st = engine.map_file(big_index, tfile.NAMES, str(fq), str(sam), 2, max_hits=max_hits, chunk_bytes=chunk_bytes)
            got = tfile.sam_lines(sam)
            tfile.compare(got, tfile.expected_lines(engine, big_index, recs, 2, max_hits=max_hits, strata=2 if max_hits else None))
            tfile.check_stats(st, got, recs)
            assert st["mapped"] >= len(reads) // 6
