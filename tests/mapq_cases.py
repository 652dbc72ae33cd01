"""The mapping-quality model of docs/design/mapper.md ("Mapping quality") stated in Python, and the small corpus its tests share
(tests/test_mapq_host.py proves both on the CPU, tests/test_gpu_mapq.py runs the corpus on the device).  A plain helper module:
everything is seeded with random.Random, nothing is read from a file.

mapq_ref_* take what the brute forces of the older modules already give: a read's loci as bf_all lists them, (s, r, i, j, d) in
(d, s, r, j) order, and for pairs the two mates' loci lists and bf_pairs' answer."""
import random

from tests.test_map_host import BASES, revcomp
from tests.test_map_pairs_host import concordant, pair_rank

E_SWEEP = (0, 2, 4)
K_SWEEP = (8, 12)
M = 100              # read length
SEG = 120            # planted segment length
INSERT = (200, 400)  # the pairs' window; fragments are 300 bp
FRAG = 300
CAPPED = 20

# (sequence, start) of every copy of each planted family; `sub` = substitutions at these segment offsets in the LAST copy
FAMILIES = {
    "two": dict(at=[(0, 500), (0, 3000)], sub=()),
    "three": dict(at=[(0, 1000), (0, 5000), (1, 1000)], sub=()),
    "five": dict(at=[(0, 1500), (0, 4000), (0, 7000), (1, 2000), (1, 5000)], sub=()),
    "near1": dict(at=[(0, 2000), (0, 8000)], sub=(40,)),
    "near2": dict(at=[(0, 2500), (1, 3000)], sub=(40, 80)),
    "cross": dict(at=[(0, 9000), (1, 6000)], sub=()),
}
FRAG_TWICE = [(0, 10_000), (1, 7000)]  # a 400 bp stretch planted twice: both mates repeat, two concordant placements


def table(n, g):
    """T(n, g)"""
    if n <= 0:
        return 0
    if n == 1:
        return min(60, 20 * g) if g >= 1 else 0
    return 3 if n == 2 else 1 if n <= 4 else 0


def read_fold(ds, e):
    """(d1, n1, d2) of a read's loci distances; without loci (e + 1, 0, e + 1)"""
    if not ds:
        return e + 1, 0, e + 1
    d1 = min(ds)
    rest = [d for d in ds if d > d1]
    return d1, ds.count(d1), min(rest) if rest else e + 1


def read_quality(loci, e, capped=False):
    """Q_read"""
    d1, n1, d2 = read_fold([l[4] for l in loci], e)
    q = table(n1, d2 - d1)
    return min(q, CAPPED) if capped else q


def mapq_ref_read(loci, e, capped=False):
    """the MAPQ of every locus of one read, in the order of `loci` (rank order): Q_read at d1, 0 above it"""
    q = read_quality(loci, e, capped)
    d1 = min([l[4] for l in loci], default=None)
    return [q if l[4] == d1 else 0 for l in loci]


def _q_locus(rec, loci, e, capped):
    return read_quality(loci, e, capped) if rec is not None and loci and rec[4] == min(l[4] for l in loci) else 0


def mapq_ref_pair(L1, L2, m1, m2, lo, hi, e, res, capped=(False, False)):
    """One fragment.  res: bf_pairs' answer for it.  -> dict: `primary` (MAPQ of mate 1, mate 2 of the pair's answer), `Q_pair`,
    `Q_locus` (the two single-end values of the answer's records), `fold` (S1, N1, S2) and `pairs`: every concordant pair in pair
    order as (a, b, (MAPQ of a, MAPQ of b)); Q_pair, fold and pairs only where there is a concordant pair."""
    out = {"Q_pair": None, "fold": None, "pairs": []}
    a, b = res["rec"]
    ql = (_q_locus(a, L1, e, capped[0]), _q_locus(b, L2, e, capped[1]))
    conc = sorted((pair_rank(x, y), x, y) for x in L1 for y in L2 if concordant(x, y, m1, m2, lo, hi))
    if conc:
        S1 = conc[0][0][0]
        N1 = sum(1 for c in conc if c[0][0] == S1)
        above = [c[0][0] for c in conc if c[0][0] > S1]
        S2 = min(above) if above else None
        g = e + 1 - max(conc[0][1][4], conc[0][2][4])
        if S2 is not None:
            g = min(g, S2 - S1)
        qp = table(N1, g)
        if capped[0] or capped[1]:
            qp = min(qp, CAPPED)
        for rank, x, y in conc:
            both = (max(_q_locus(x, L1, e, capped[0]), qp), max(_q_locus(y, L2, e, capped[1]), qp)) if rank[0] == S1 else (0, 0)
            out["pairs"].append((x, y, both))
        out.update(Q_pair=qp, fold=(S1, N1, S2), primary=out["pairs"][0][2])
        ql = (_q_locus(conc[0][1], L1, e, capped[0]), _q_locus(conc[0][2], L2, e, capped[1]))
    elif res["rescued"] is not None:
        who = res["rescued"]
        qa = ql[1 - who]  # the anchor keeps its single-end Q_read
        prim = [0, 0]
        prim[1 - who], prim[who] = qa, min(qa, CAPPED)
        out["primary"] = tuple(prim)
    else:
        out["primary"] = ql
    out["Q_locus"] = ql
    return out


def _rand(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def _sub(rng, q, positions):
    q = list(q)
    for p in positions:
        q[p] = rng.choice([c for c in BASES if c != q[p]])
    return "".join(q)


def reference(seed=2024):
    """about 20 kbp in two sequences with the families planted"""
    rng = random.Random(seed)
    seqs = [list(_rand(rng, 12_000)), list(_rand(rng, 8_000))]
    for name in sorted(FAMILIES):
        fam = FAMILIES[name]
        seg = _rand(rng, SEG)
        for t, (r, a) in enumerate(fam["at"]):
            piece = _sub(rng, seg, fam["sub"]) if fam["sub"] and t == len(fam["at"]) - 1 else seg
            seqs[r][a:a + SEG] = piece
    frag = _rand(rng, 400)
    for r, a in FRAG_TWICE:
        seqs[r][a:a + 400] = frag
    return ["".join(s) for s in seqs]


# starts of stretches that hold no planted copy; the pairs draw on the first six only
UNIQUE = [(0, 200), (0, 3300), (0, 6000), (0, 11_000), (1, 200), (1, 4000), (0, 6500), (0, 11_500), (1, 500), (1, 4500)]


def reads(seqs, e, seed=5):
    """the single-end reads of one e: [(label, read)]"""
    rng = random.Random(1000 * seed + e)
    out = []
    for x in range(e + 1):  # unique places with 0..e substitutions, both strands
        for t, (r, a) in enumerate(UNIQUE):
            q = _sub(rng, seqs[r][a + 7 * x:a + 7 * x + M], [int((u + 0.5) * M / max(x, 1)) for u in range(x)])
            out.append(("unique%d" % x, revcomp(q) if t % 2 else q))
    for name in sorted(FAMILIES):  # every family: from its first and its last copy, both strands, exact; one with an edit
        at = FAMILIES[name]["at"]
        for t, (r, a) in enumerate((at[0], at[-1], at[0], at[-1])):
            q = seqs[r][a + 10:a + 10 + M]
            if t >= 2 and e >= 1:
                q = _sub(rng, q, [5])
            out.append((name, revcomp(q) if t % 2 else q))
    for _ in range(4):
        out.append(("random", _rand(rng, M)))
    for t, (r, a) in enumerate(UNIQUE[:4]):  # an N costs one edit
        q = seqs[r][a + 50:a + 50 + M]
        out.append(("with_N", q[:30 + t] + "N" + q[31 + t:]))
    r, a = FAMILIES["five"]["at"][1]
    q = seqs[r][a + 10:a + 10 + M]
    out.append(("five_N", q[:60] + "N" + q[61:]))
    return out


def _fr(seq, a, m=M, f=FRAG):
    """the FR pair of the fragment seq[a, a + f): mate 1 forward at its start, mate 2 reverse at its end"""
    return seq[a:a + m], revcomp(seq[a + f - m:a + f])


def pairs(seqs, e, seed=9):
    """the pairs of one e: [(label, mate 1, mate 2)]; rescue pairs carry e + 2 substitutions in mate 2"""
    rng = random.Random(1000 * seed + e)
    out = []
    for r, a in UNIQUE[:4]:
        q1, q2 = _fr(seqs[r], a)
        out.append(("unique", q1, q2))
    for t, (r, a) in enumerate(FAMILIES["five"]["at"][:4]):  # mate 1 inside a copy of the 5-copy family, mate 2 unique
        q1, q2 = _fr(seqs[r], a + 10)
        out.append(("five_unique", q1, q2) if t % 2 == 0 else ("five_unique", q2, q1))
    for t, (r, a) in enumerate(FRAG_TWICE + FRAG_TWICE):  # both mates repeat, two concordant placements
        q1, q2 = _fr(seqs[r], a + 20 + 10 * t)
        out.append(("both_twice", q1, q2))
    for t, (r, a) in enumerate(UNIQUE[2:6]):  # mate 2 lies beyond e: left to the rescue
        q1, q2 = _fr(seqs[r], a + 400)
        q2 = _sub(rng, q2, [int((u + 0.5) * M / (e + 2)) for u in range(e + 2)])
        out.append(("rescue", q1, q2) if t % 2 == 0 else ("rescue", q2, q1))
    r, a = FAMILIES["five"]["at"][0]  # the anchor of a rescue inside the 5-copy family
    q1, q2 = _fr(seqs[r], a + 10)
    out.append(("rescue_five", q1, _sub(rng, q2, [int((u + 0.5) * M / (e + 2)) for u in range(e + 2)])))
    return out


def rescue_errors(e):
    return e + 3
