"""GPU read mapper (asm_index_build / asm_map_reads, docs/design/mapper.md) against the test-only brute-force mapper
(tests/cxx/map_bruteforce.cpp): every read's (mapped, strand, seq, pos, end, dist) must be the brute force's, every CIGAR must
walk the read over its window with NM = d, Greedy's cost on the hit window must be the oracle's, and asm-map's SAM must carry the
same records."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.test_map_host import BASES, build_bruteforce, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (64, 100, 150, 300)
ERRORS = (0, 1, 2, 4)


def make_reference(seed=11):
    """3 sequences, ~300 kbp: a run of N, lower-case stretches and a segment copied into another sequence (ties)."""
    rng = random.Random(seed)
    seqs = ["".join(rng.choice(BASES) for _ in range(n)) for n in (120_000, 100_000, 80_000)]
    s0 = seqs[0]
    s0 = s0[:50_000] + "N" * 500 + s0[50_500:]
    s0 = s0[:70_000] + s0[70_000:72_000].lower() + s0[72_000:]
    seqs[0] = s0
    seg = seqs[1][10_000:13_000]
    seqs[2] = seqs[2][:40_000] + seg + seqs[2][43_000:]  # identical copy: reads from it tie between sequences 1 and 2
    seqs[1] = seqs[1][:60_000] + seqs[1][60_000:61_500].lower() + seqs[1][61_500:]
    return seqs


def mutate(rng, q, edits):
    q = list(q)
    for _ in range(edits):
        kind = rng.randrange(3)
        p = rng.randrange(len(q))
        if kind == 0:
            q[p] = rng.choice([b for b in BASES if b != q[p]])
        elif kind == 1:
            q.insert(p, rng.choice(BASES))
        else:
            del q[p]
    return "".join(q)


def make_reads(seqs, e, n, seed):
    rng = random.Random(seed)
    reads = []
    for t in range(n):
        m = LENGTHS[t % len(LENGTHS)]
        kind = t % 10
        if kind == 8:  # random read
            reads.append("".join(rng.choice(BASES) for _ in range(m)))
            continue
        r = rng.randrange(len(seqs))
        s = seqs[r]
        if kind == 6:    # at a sequence edge
            a = 0 if rng.random() < 0.5 else len(s) - m
        elif kind == 7:  # from the duplicated segment
            r, s = 1, seqs[1]
            a = 10_000 + rng.randrange(3000 - m)
        else:
            a = rng.randrange(len(s) - m)
        q = mutate(rng, s[a:a + m].upper(), rng.randint(0, e))
        if "N" in q:
            q = q.replace("N", "A")
        if kind == 9:  # an N inside the read
            p = rng.randrange(len(q))
            q = q[:p] + "N" + q[p + 1:]
        if rng.random() < 0.5:
            q = revcomp(q)
        if rng.random() < 0.1:
            q = q.lower()
        reads.append(q)
    return reads


@pytest.fixture(scope="module")
def bf(tmp_path_factory):
    return build_bruteforce(tmp_path_factory.mktemp("map_bf_gpu"))


@pytest.fixture(scope="module")
def ref():
    return make_reference()


@pytest.fixture(scope="module")
def index(engine, ref):
    return engine.build_index(ref, k=12)


def brute_force(bf, seqs, reads, e, both=True):
    from tests.test_map_host import bf_map

    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda q: bf_map(bf, seqs, q, e, both), reads))


def got_tuple(out, t):
    if not out["mapped"][t]:
        return (0, -1, -1, -1, -1, -1)
    return (1, int(out["strand"][t]), int(out["seq_id"][t]), int(out["pos"][t]), int(out["end"][t]), int(out["dist"][t]))


def walk_cigar(cigar, q, w):
    """-> (read bases, reference bases, edits under the byte rule)"""
    import re

    a = b = nm = 0
    for cnt, op in re.findall(r"(\d+)([MID])", cigar):
        cnt = int(cnt)
        if op == "M":
            nm += sum(1 for z in range(cnt) if not (q[a + z] == w[b + z] and q[a + z] in BASES))
            a += cnt
            b += cnt
        elif op == "I":
            a += cnt
            nm += cnt
        else:
            b += cnt
            nm += cnt
    return a, b, nm


def strand_read(q, s):
    q = q.upper()
    return revcomp(q) if s else q


@pytest.mark.parametrize("e", ERRORS)
def test_map_equals_brute_force(asm, engine, oracle, bf, ref, index, e):
    reads = make_reads(ref, e, 240, seed=100 + e)
    reads += ["ACGT" * 5, "A" * 30]  # too short for (e + 1) * k at k = 12 when e >= 2; short reads at any e
    out = engine.map_reads(index, reads, e)
    want = brute_force(bf, ref, reads, e)
    k = index.k
    up = [s.upper() for s in ref]
    n_mapped = 0
    for t, q in enumerate(reads):
        if len(q) < (e + 1) * k:
            assert not out["mapped"][t] and out["flags"][t] & asm.MAP_TOO_SHORT, t
            continue
        assert not out["flags"][t] & asm.MAP_TOO_SHORT
        assert got_tuple(out, t) == want[t], (t, q, got_tuple(out, t), want[t])
        if not out["mapped"][t]:
            assert out["cigar"][t] == "" and out["greedy_cost"][t] == -1
            continue
        n_mapped += 1
        s, r, i, j, d = want[t][1:]
        qs = strand_read(q, s)
        a, b, nm = walk_cigar(out["cigar"][t], qs, up[r][i:j])
        assert (a, b, nm) == (len(q), j - i, d), (t, out["cigar"][t])
    assert n_mapped > 150
    # Greedy on the hit windows, as mapper/main.cpp:79-95 runs it; MAPQ = min(254, 60 + cost)
    idx = np.nonzero(out["mapped"])[0]
    pairs = []
    for t in idx:
        s, r, i = int(out["strand"][t]), int(out["seq_id"][t]), int(out["pos"][t])
        w = i - 1 if i else 0
        pairs.append((strand_read(reads[t], s), up[r][w:min(w + len(reads[t]) + 1, len(up[r]))]))
    hb = asm.HostBatch.from_strings(pairs)
    costs = oracle.greedy(hb, k=3, mode=1)
    assert np.array_equal(out["greedy_cost"][idx], costs)
    assert np.array_equal(out["mapq"][idx], np.minimum(254, 60 + costs))


def test_forward_strand_only(engine, bf, ref, index):
    reads = make_reads(ref, 2, 120, seed=7)
    out = engine.map_reads(index, reads, 2, both_strands=False)
    want = brute_force(bf, ref, reads, 2, both=False)
    assert [got_tuple(out, t) for t in range(len(reads))] == want
    assert not out["strand"][out["mapped"]].any()


def test_chunking_and_rounds_do_not_change_results(asm, engine, ref, index, monkeypatch):
    reads = make_reads(ref, 4, 300, seed=5)
    base = engine.map_reads(index, reads, 4)
    again = engine.map_reads(index, reads, 4)
    split = engine.map_reads(index, reads, 4, chunk=37)
    # a second engine whose device chunks and candidate rounds are tiny: many chunks, many seeding rounds per chunk
    monkeypatch.setenv("ASM_MAP_CHUNK", "23")
    monkeypatch.setenv("ASM_MAP_CAND_CAP", "5")
    small = asm.Engine(0)
    try:
        ix2 = small.build_index(ref, k=12)
        tiny = small.map_reads(ix2, reads, 4)
        ix2.free()
    finally:
        small.close()
    for other in (again, split, tiny):
        for key in ("seq_id", "pos", "end", "dist", "strand", "flags", "greedy_cost"):
            assert np.array_equal(base[key], other[key]), key
        assert base["cigar"] == other["cigar"]


def test_other_k(engine, bf, ref):
    ix = engine.build_index(ref, k=9)
    reads = make_reads(ref, 1, 80, seed=3)
    out = engine.map_reads(ix, reads, 1)
    want = brute_force(bf, ref, reads, 1)
    assert [got_tuple(out, t) for t in range(len(reads))] == want
    ix.free()


def test_seed_cap(asm, engine, bf, ref):
    # a low-complexity stretch makes big buckets; reads spanning it seed there
    rng = random.Random(9)
    seqs = list(ref)
    seqs[2] = seqs[2][:20_000] + "ACGTACGTAC" * 300 + seqs[2][23_000:]
    ix = engine.build_index(seqs, k=10)
    reads = make_reads(seqs, 2, 160, seed=13)
    for _ in range(40):
        a = 20_000 + rng.randrange(2900)
        reads.append(mutate(rng, seqs[2][a:a + 100], rng.randint(0, 2)))
    full = engine.map_reads(ix, reads, 2)
    capped = engine.map_reads(ix, reads, 2, max_occ=20)
    want = brute_force(bf, seqs, reads, 2)
    flagged = (capped["flags"] & asm.MAP_SEED_CAPPED) != 0
    assert flagged.sum() >= 20
    up = [s.upper() for s in seqs]
    for t in range(len(reads)):
        assert got_tuple(full, t) == want[t]
        if not flagged[t]:
            assert got_tuple(capped, t) == want[t]
        elif capped["mapped"][t]:
            s, r, i, j, d = got_tuple(capped, t)[1:]
            assert d >= want[t][5]
            a, b, nm = walk_cigar(capped["cigar"][t], strand_read(reads[t], s), up[r][i:j])
            assert (a, b, nm) == (len(reads[t]), j - i, d)  # a real occurrence at that distance
    ix.free()


def test_asm_map_cli_writes_matching_sam(asm, engine, ref, index, tmp_path):
    exe = os.path.join(ROOT, "approximate-string-matching_amd", "asm-map")
    assert os.path.exists(exe), "asm-map is built by build()"
    names = ["chrA", "chrB", "chrC"]
    fa = tmp_path / "ref.fa"
    with open(fa, "w") as fh:
        for nm, s in zip(names, ref):
            fh.write(f">{nm} some description\n")
            for p in range(0, len(s), 70):
                fh.write(s[p:p + 70] + "\n")
    reads = make_reads(ref, 2, 150, seed=21) + ["ACGT" * 4]
    rng = random.Random(2)
    quals = ["".join(chr(33 + rng.randrange(40)) for _ in q) for q in reads]
    fq = tmp_path / "reads.fq"
    with open(fq, "w") as fh:
        for t, (q, ql) in enumerate(zip(reads, quals)):
            fh.write(f"@read{t} x\n{q}\n+\n{ql}\n")
    sam = tmp_path / "out.sam"
    r = subprocess.run([exe, "-r", str(fa), "-q", str(fq), "-o", str(sam), "-e", "2", "--both-strands", "--chunk", "40"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = sam.read_text().splitlines()
    head = [ln for ln in lines if ln.startswith("@")]
    body = [ln.split("\t") for ln in lines if not ln.startswith("@")]
    assert head[0] == "@HD\tVN:1.6\tSO:unsorted"
    assert head[1:4] == [f"@SQ\tSN:{nm}\tLN:{len(s)}" for nm, s in zip(names, ref)]
    assert head[4].startswith("@PG\tID:asm-map")
    assert len(body) == len(reads)
    out = engine.map_reads(index, reads, 2)
    for t, f in enumerate(body):
        assert f[0] == f"read{t}"
        q = reads[t].upper()
        if not out["mapped"][t]:
            assert f[1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"] and f[9] == q and f[10] == quals[t]
            continue
        s = int(out["strand"][t])
        assert int(f[1]) == (16 if s else 0)
        assert f[2] == names[out["seq_id"][t]] and int(f[3]) == out["pos"][t] + 1 and int(f[4]) == out["mapq"][t]
        assert f[5] == out["cigar"][t] and f[6:9] == ["*", "0", "0"]
        assert f[9] == (revcomp(q) if s else q) and f[10] == (quals[t][::-1] if s else quals[t])
        assert f[11] == f"NM:i:{out['dist'][t]}" and f[12] == f"XG:i:{out['greedy_cost'][t]}"
    assert any(f[1] == "16" for f in body) and any(f[1] == "0" for f in body) and any(f[1] == "4" for f in body)


def test_smoke_sized_index_build(engine):
    """Empty and N-only sequences index and map without hits."""
    ix = engine.build_index(["", "N" * 100, "ACGTTGCAACGTAGGA" * 4], k=8)
    out = engine.map_reads(ix, ["ACGTTGCAACGTAGGA" * 2, "N" * 40], 0)
    assert out["mapped"][0] and out["seq_id"][0] == 2 and out["dist"][0] == 0 and not out["mapped"][1]
    ix.free()
