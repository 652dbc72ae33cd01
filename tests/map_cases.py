"""Inputs and the CIGAR yardstick of the mapper's width / word-edge / error-range tests (tests/test_map_widths_host.py proves them
on the CPU, tests/test_gpu_map_widths.py runs them on the device).  A plain helper module: everything is seeded with
random.Random, nothing is read from a file.

The kernels of csrc/asm_map.h are templates over the number of 64-bit words W in {1, 2, 4, 8}; the launch's W comes from the
longest read of the call's device chunk.  LENGTHS_BY_W holds, per W, read lengths on both sides of every word edge of that class;
E_SWEEP spans the whole contract range of max_errors at k = 8, the only k at which a 128 bp read is searchable with 15 errors
(a read is searchable when m >= (e + 1) * k)."""
import random

import numpy as np

from tests.test_map_host import BASES, revcomp

# W = 1: 8 = one k-mer, 31 = below half a word, 63 / 64 = the last bit of the only word (last_bit = 62, 63).
# W = 2: 65 = one bit in the second word, 127 / 128 = the last bit of the last word; 100 = the length of every published number.
# W = 4: 129 = one bit in word 2, 191 / 192 / 193 = nw = 3 inside a W = 4 launch and its two neighbours, 255 / 256 = full.
# W = 8: 257 and 321 = one bit in a new word, 320 = nw = 5 full, 447 / 448 / 449 = around the edge of word 6, 510 / 511 = the
#        longest reads the contract allows (512 is rejected by the argument checks).
LENGTHS_BY_W = {1: (8, 31, 63, 64), 2: (65, 100, 127, 128), 4: (129, 191, 192, 193, 255, 256), 8: (257, 320, 321, 447, 448, 449, 510, 511)}
E_SWEEP = (0, 1, 3, 7, 8, 12, 15)
K_SWEEP = 8
# cells at the other legal k: the largest k (14) and the k of the index the older modules share (12)
EXTRA_CELLS = {14: ((64, 3), (128, 8), (256, 15), (511, 15)), 12: ((63, 3), (128, 8), (193, 15), (449, 15))}
KINDS = ("sub_spread", "ins_run_head", "ins_run_tail", "del_run_head", "del_run_tail", "word_edge", "one_piece", "in_piece",
         "seq_start", "seq_end", "straddle", "with_N", "lower", "random", "del_spread", "tail_junk")

# layout of reference_small(): indices of its sequences
BIG = (0, 3, 7)          # the sequences reads are sampled from
TINY = (1, 2)            # 40 and 200 bp, next to each other
SHORT = 4                # 50 bp: shorter than most reads
STRADDLE = (5, 6)        # a 100 bp stretch: its first half ends sequence 5, its second half starts sequence 6
N_RUN = (0, 15_000, 300)  # sequence, start, length of the run of N


def width_of(m):
    """the template width a call whose longest read has m bytes must pick"""
    return 1 if m <= 64 else 2 if m <= 128 else 4 if m <= 256 else 8


def cell_exists(m, e, k=K_SWEEP):
    """searchable: every one of the e + 1 pigeonhole pieces holds a k-mer"""
    return m >= (e + 1) * k


def cells_of(W, k=K_SWEEP):
    """the (m, e) cells of one width class"""
    return [(m, e) for m in LENGTHS_BY_W[W] for e in E_SWEEP if cell_exists(m, e, k)]


def errors_of(W, k=K_SWEEP):
    """the e of E_SWEEP at which at least one length of the class is searchable"""
    return [e for e in E_SWEEP if any(cell_exists(m, e, k) for m in LENGTHS_BY_W[W])]


def _rand(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def reference_small(seed=71):
    """~97 kbp in 8 sequences with the ingredients of tests/test_gpu_map.py::make_reference (a run of N, lower-case stretches, a
    segment copied into another sequence) plus: two short sequences next to each other (40 and 200 bp), one sequence shorter than
    most reads (50 bp), and a 100 bp stretch cut in two by a sequence boundary (STRADDLE)."""
    rng = random.Random(seed)
    b0, b1, b2 = (_rand(rng, n) for n in (40_000, 30_000, 20_000))
    seq, a, n = N_RUN
    b0 = b0[:a] + "N" * n + b0[a + n:]
    b0 = b0[:20_000] + b0[20_000:21_000].lower() + b0[21_000:]
    b2 = b2[:8_000] + b1[5_000:6_500] + b2[9_500:]  # identical copy: reads from it tie between sequences 3 and 7
    b1 = b1[:12_000] + b1[12_000:12_800].lower() + b1[12_800:]
    stretch = _rand(rng, 100)
    left, right = _rand(rng, 3_000) + stretch[:50], stretch[50:] + _rand(rng, 3_000)
    return [b0, _rand(rng, 40), _rand(rng, 200), b1, _rand(rng, 50), left, right, b2]


def _other(rng, *avoid):
    return rng.choice([b for b in BASES if b not in avoid])


def _source(rng, seqs, span, ok=lambda s, a: True):
    """a big sequence (upper case) and a start of `span` bases free of N, at least 40 bases from both ends"""
    for _ in range(1000):
        r = rng.choice(BIG)
        s = seqs[r].upper()
        a = rng.randrange(40, len(s) - span - 40)
        if "N" not in s[a - 20:a + span + 20] and ok(s, a):
            return s, a
    raise AssertionError("no source found")


def _substitute(q, positions, rng):
    q = list(q)
    for p in positions:
        q[p] = _other(rng, q[p])
    return "".join(q)


def _ins_run(rng, e, avoid):
    """e inserted bases, none of them one of `avoid` (so that the run cannot be read as a copy of its neighbours)"""
    return "".join(_other(rng, *avoid) for _ in range(e))


def _word_offsets(m):
    return [p for p in (62, 63, 64, 65) if p < m] + list(range(128, m, 64))


def word_boundaries(m):
    """the t with 0 < 64 t <= m - 1: the word boundaries inside a read of m bases.  A D op in front of the read's last base never
    survives the smallest-end rule (mismatching or dropping that base costs the same and ends earlier), so at 64 t = m - 1 (the
    lengths with one bit in a new word: 65, 129, 193, 257, 321, 449) the gap is the I run of `tail_junk`, which holds the read
    offsets 64 t - 1 and 64 t."""
    return [t for t in range(1, 8) if 64 * t <= m - 1]


def _word_edge(seqs, m, e, rng, first):
    """min(e, all) edits at the read offsets _word_offsets(m)[first:first + e] (cyclic): a deleted reference base in front of every
    offset that is a multiple of 64 and at most m - 2 (a D op at the word boundary; its neighbours differ from it, so the traceback
    cannot move it), a substitution at the others."""
    offs = _word_offsets(m)
    if not offs or e == 0:
        s, a = _source(rng, seqs, m)
        return s[a:a + m]
    pick = {offs[(first + t) % len(offs)] for t in range(min(e, len(offs)))}
    gaps = {p for p in pick if p % 64 == 0 and p <= m - 2}
    pick = sorted(p for p in pick if p in gaps or not ({p - 1, p + 1} & gaps))  # an edit next to a gap would let the gap move
    for _ in range(500):
        s, a = _source(rng, seqs, m + e + 2)
        q, x, good = [], a, True  # x: the next source base
        for p in pick:
            while len(q) < p:
                q.append(s[x])
                x += 1
            if p % 64 == 0 and p <= m - 2:
                good = good and s[x] != s[x - 1] and s[x] != s[x + 1]
                x += 1
            else:
                q.append(_other(rng, s[x]))
                x += 1
        if not good:
            continue
        while len(q) < m:
            q.append(s[x])
            x += 1
        return "".join(q)
    raise AssertionError("no word_edge source found")


def _one(seqs, kind, m, e, k, rng, variant):
    """one forward read of exactly m bases"""
    if kind == "random":
        return _rand(rng, m)
    if kind == "sub_spread":
        s, a = _source(rng, seqs, m)
        return _substitute(s[a:a + m], [int((t + 0.5) * m / e) for t in range(e)], rng)
    if kind == "ins_run_head":
        s, a = _source(rng, seqs, m)
        return (s[a] + _ins_run(rng, e, (s[a], s[a + 1])) + s[a + 1:a + m])[:m]
    if kind == "ins_run_tail":
        s, a = _source(rng, seqs, m)
        z = a + m - e - 1  # the source base that stays last
        return s[a:z] + _ins_run(rng, e, (s[z - 1], s[z])) + s[z] if m > e + 1 else s[a:a + m]
    if kind in ("del_run_head", "del_run_tail"):
        h = max(1, min(m // 3, 3 * e + 6))  # far enough from the end that mismatching the short side costs more than the gap
        s, a = _source(rng, seqs, m + e)
        cut = a + h if kind == "del_run_head" else a + m - h
        return s[a:cut] + s[cut + e:a + m + e]
    if kind == "word_edge":
        return _word_edge(seqs, m, e, rng, variant * max(e, 1))
    if kind == "one_piece":  # a substitution in the middle of every pigeonhole piece but one: exactly one piece seeds
        s, a = _source(rng, seqs, m)
        L = m // (e + 1)
        clean = rng.randrange(e + 1)
        return _substitute(s[a:a + m], [p * L + L // 2 for p in range(e + 1) if p != clean], rng)
    if kind == "in_piece":  # all the edits inside one piece (as many as fit): every other piece seeds the same diagonal
        s, a = _source(rng, seqs, m)
        L = m // (e + 1)
        p0 = rng.randrange(e + 1) * L
        return _substitute(s[a:a + m], range(p0, p0 + min(e, L)), rng)
    if kind in ("seq_start", "seq_end"):
        r = rng.choice(BIG + STRADDLE)
        s = seqs[r].upper()
        if variant < 2:  # the read hangs e bases over the sequence's edge: j - m - d < 0 at the start, the window is clipped
            junk = _ins_run(rng, e, (s[0], s[-1]))
            return junk + s[:m - e] if kind == "seq_start" else s[len(s) - (m - e):] + junk
        h = max(1, min(m // 3, 3 * e + 6))  # e reference bases deleted: the occurrence is T[0, m + e), so lo = j - m - d is 0
        if kind == "seq_start":
            return s[:h] + s[h + e:m + e]
        t = s[len(s) - (m + e):]
        return t[:m - h] + t[m - h + e:]
    if kind == "straddle":  # the exact copy spans two sequences; inside one of them the read costs the h bases of the other
        left, right = seqs[STRADDLE[0]].upper(), seqs[STRADDLE[1]].upper()
        h = max(1, (e + 1) // 2)
        h = h if variant % 2 == 0 else m - h
        return left[len(left) - h:] + right[:m - h]
    if kind == "with_N":
        if variant < 2:  # an N in the read (it costs one edit) and e - 1 substitutions
            s, a = _source(rng, seqs, m)
            q = _substitute(s[a:a + m], [int((t + 0.5) * m / e) for t in range(max(e - 1, 0))], rng)
            p = m // 2 + 1
            return q[:p] + "N" + q[p + 1:]
        r, a, n = N_RUN  # the read's tail lies over the reference's run of N: every N costs an edit, N against N included
        x = min(max(1, e // 2), m - 1)
        s = seqs[r].upper()
        return s[a + x - m:a + x]
    if kind == "del_spread":  # e single deleted reference bases near spaced read offsets: a CIGAR of 2 e + 1 operations
        s, a = _source(rng, seqs, m + e)
        q, x = [], a
        for p in [int((t + 0.5) * m / e) for t in range(e)]:
            while len(q) < p or s[x] == s[x - 1] or s[x] == s[x + 1]:  # a gap between two bases that differ from it cannot move
                q.append(s[x])
                x += 1
            x += 1
        return ("".join(q) + s[x:x + m])[:m]
    if kind == "tail_junk":  # the last min(e, 2) bases are no copy of the reference: ...M2I ends earliest, so the I run wins
        s, a = _source(rng, seqs, m)
        x = min(e, 2)
        z = a + m - x
        return s[a:z] + _ins_run(rng, x, (s[z - 1], s[z], s[z + 1]))
    if kind == "lower":
        s, a = _source(rng, seqs, m)
        return _substitute(s[a:a + m], [int((t + 0.5) * m / (e // 2)) for t in range(e // 2)], rng).lower()
    raise ValueError(kind)


def edge_reads(seqs, m, e, k, rng, variants=2):
    """The reads of one (m, e) cell over reference_small(): `variants` reads of every kind in KINDS, each with its label;
    odd variants are reverse-complemented, `seq_start`, `seq_end` and `with_N` get twice as many (two recipes each).  Every read
    has exactly m bytes: an edited read takes more or fewer source bases.

    `one_piece` leaves exactly one pigeonhole piece clean (one substitution in each of the others); `in_piece` is the other
    reading of "all edits in one piece": as many substitutions as fit next to each other inside a single piece."""
    assert cell_exists(m, e, k), (m, e, k)
    out = []
    for kind in KINDS:
        for v in range(variants * (2 if kind in ("seq_start", "seq_end", "with_N") else 1)):
            q = _one(seqs, kind, m, e, k, rng, v)
            assert len(q) == m, (kind, m, e, len(q))
            if v % 2:  # revcomp knows upper case only
                q = revcomp(q.upper()).lower() if q.islower() else revcomp(q)
            out.append((kind, q))
    return out


def short_reads(seqs, m, rng):
    """exact copies for a length that is not searchable at the cell's e: they must come back TOO_SHORT"""
    out = []
    for v in range(2):
        s, a = _source(rng, seqs, m)
        out.append(("too_short", revcomp(s[a:a + m]) if v else s[a:a + m]))
    return out


def class_reads(seqs, W, e, k=K_SWEEP, lengths=None):
    """every read of one width class at e: edge_reads for the searchable lengths, short_reads for the others"""
    out = []
    for m in (lengths or LENGTHS_BY_W[W]):
        rng = random.Random(100_000 * k + 100 * m + e)
        out += edge_reads(seqs, m, e, k, rng) if cell_exists(m, e, k) else short_reads(seqs, m, rng)
    return out


def mid_edit(rng, src, m, x, kind):
    """a forward read of m bases from the start of src (upper case, at least m + x long) with x edits in its middle: a run of
    inserted bases, a run of deleted reference bases, or spaced substitutions; -> (read, reference bases spanned)"""
    h = m // 2
    if kind == "ins":
        ins = "".join(rng.choice([b for b in BASES if b not in (src[h - 1], src[h])]) for _ in range(x))
        return src[:h] + ins + src[h:m - x], m - x
    if kind == "del":
        return src[:h] + src[h + x:m + x], m + x
    q = list(src[:m])
    for t in range(x):
        p = int((t + 0.5) * m / x)
        q[p] = rng.choice([b for b in BASES if b != q[p]])
    return "".join(q), m


def pair_reads(seqs, lengths, e, k, seed):
    """FR pairs with mates of one length each: mate 1 an exact copy, mate 2 with e edits (concordant), with more than e edits or
    too short to seed (left to the rescue)"""
    rng = random.Random(seed)
    up = [s.upper() for s in seqs]
    r1s, r2s = [], []
    for m in lengths:
        if m < (e + 1) * k:
            continue
        for v in range(6):
            r = BIG[v % 3]
            f = 2 * m + 40 + rng.randrange(60)
            a = rng.randrange(1000, len(up[r]) - f - 1000)
            x = e if v < 3 else min(15, e + 2)
            kind = ("ins", "del", "sub")[v % 3]
            span = m + (x if kind == "del" else -x if kind == "ins" else 0)  # mate 2 keeps its end a + f
            q2, _ = mid_edit(rng, up[r][a + f - span:a + f + 40], m, x, kind)
            if v == 5:
                q2 = q2[:max(8, min(m, (e + 1) * k - 1))]  # too short to seed when e > 0
            q1, q2 = up[r][a:a + m], revcomp(q2)
            if "N" in up[r][a - 40:a + f + 40]:
                continue
            r1s.append(q1 if v % 2 else q2)
            r2s.append(q2 if v % 2 else q1)
    return r1s, r2s


def _is_base(c):
    return c in BASES


def ref_matrix(qs, window):
    """the full (m + 1) x (n + 1) edit-distance matrix of q_s against the window under the byte rule (A, C, G, T match only
    themselves, every other byte mismatches everything); row 0 is 0..n, column 0 is 0..m"""
    m, n = len(qs), len(window)
    q = np.frombuffer(qs.encode("latin-1"), np.uint8)
    w = np.frombuffer(window.encode("latin-1"), np.uint8)
    ar = np.arange(n + 1, dtype=np.int32)
    D = np.empty((m + 1, n + 1), np.int32)
    D[0] = ar
    cand = np.empty(n + 1, np.int32)
    for a in range(1, m + 1):
        cost = (w != q[a - 1]).astype(np.int32) if _is_base(qs[a - 1]) else np.ones(n, np.int32)
        cand[0] = a
        np.minimum(D[a - 1, :-1] + cost, D[a - 1, 1:] + 1, out=cand[1:])
        # the left neighbour: D[a][b] = min over b' <= b of cand[b'] + (b - b')
        D[a] = np.minimum.accumulate(cand - ar) + ar
    return D


def ref_cigar(qs, window):
    """The contract's CIGAR of q_s against the window (docs/design/mapper.md, "Alignment"): a full-matrix DP under the byte rule and
    a traceback from (m, n) that prefers the diagonal (M), then up (I: a read base absent from the reference), then left (D).
    Column 0 is all I and row 0 is all D.

    Why this equals the kernel's banded traceback (31 diagonals, values saturated above d): a traceback only visits cells (a, b)
    with D[a][b] + (cost of the path from there to (m, n)) = d, so every visited cell has D[a][b] <= d.  D[a][b] >= |b - a|, so such
    a cell lies inside the band |b - a| <= d <= 15.  By induction over the cells, the banded value of a cell whose true value is
    <= d is the true value: its optimal predecessor has a true value <= d too, lies in the band and is exact.  A predecessor
    whose banded value differs from its true value has a true value > d, so it offers more than d and can neither win nor tie at a
    visited cell.  Hence at every visited cell the band sees the same three offers wherever they matter, and with the same
    preference both tracebacks take the same step."""
    m, n = len(qs), len(window)
    D = ref_matrix(qs, window)
    a, b = m, n
    ops = []
    while a > 0 or b > 0:
        if a == 0:
            op = "D"
        elif b == 0:
            op = "I"
        else:
            sub = 0 if (qs[a - 1] == window[b - 1] and _is_base(qs[a - 1])) else 1
            v = D[a, b]
            op = "M" if v == D[a - 1, b - 1] + sub else "I" if v == D[a - 1, b] + 1 else "D"
        ops.append(op)
        if op != "D":
            a -= 1
        if op != "I":
            b -= 1
    ops.reverse()
    out, t = [], 0
    while t < len(ops):
        u = t
        while u < len(ops) and ops[u] == ops[t]:
            u += 1
        out.append("%d%s" % (u - t, ops[t]))
        t = u
    return "".join(out)


def cigar_ops(cigar):
    """'3M1I' -> [(3, 'M'), (1, 'I')]"""
    import re

    return [(int(c), o) for c, o in re.findall(r"(\d+)([MID])", cigar)]


def crossed_boundaries(cigar, m):
    """the word boundaries t (read offset 64 t, 0 < 64 t < m) at which the CIGAR has a gap: a D op at read offset 64 t, or an I op
    that holds read offsets 64 t - 1 and 64 t"""
    hit = set()
    a = 0
    for cnt, op in cigar_ops(cigar):
        if op == "D" and a % 64 == 0 and 0 < a < m:
            hit.add(a // 64)
        if op == "I":
            for t in range(1, (m - 1) // 64 + 1):
                if a <= 64 * t - 1 and 64 * t < a + cnt:
                    hit.add(t)
        if op != "D":
            a += cnt
    return hit
