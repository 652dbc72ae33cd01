"""A structured corpus for the pair aligners: repeats, shifted copies, block gaps, edits on word edges and unrelated pairs.

The other inputs of the suite (asm.generate_pairs, tests/util.random_ragged_batch) are uniform random text with scattered edits: an
extension off the main diagonal runs about 1.3 characters there, a match mask is never all ones, a gap is one character, and few
cells tie.  The kinds below make every diagonal extend over several words, drive the carry of the bit-parallel NW through a whole
column, put one gap of k - 1, k and k + 1 characters at a string's ends and word edges, and fill the matrix with ties.

Deterministic from the seed; nothing is read from disk.  A batch carries, beside the HostBatch fields, `kinds` (numpy array of
the kind's name per pair) and `meta` (one dict per pair: what was built, for the tests that prove the corpus is what it claims).
"""
import numpy as np

EDGES = (31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512)
KINDS = ("homopolymer", "tandem", "shifted", "rotated_repeat", "block_gap", "edge_edits", "unrelated", "dirty_repeat")
REPEAT_KINDS = ("homopolymer", "tandem", "rotated_repeat")
EDIT_POSITIONS = (0, 30, 31, 32, 62, 63, 64, 126, 127, 128)  # and L - 1
PLACEMENTS = ("start", "end", "word_edge", "random")
N = 1061  # two full 512-pair workgroups of the widest kernels and a ragged tail of 37, as in test_gpu_dispatch.py
ZONE = 6  # random edits of the repeat kinds stay within this many characters of a string's ends (see _end_edits)
DIRTY = np.frombuffer(b"NnacgtRY-*", np.uint8)
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMPLEMENT = {ord("A"): ord("C"), ord("C"): ord("A"), ord("G"): ord("T"), ord("T"): ord("G")}


def _random(rng, L):
    return list(_ACGT[rng.integers(0, 4, L)])


def _other(rng, c):
    """A base that is not c."""
    return _ACGT[(int(np.searchsorted(_ACGT, c)) + int(rng.integers(1, 4))) % 4]


def _unit(rng, period):
    """A repeat unit that has no shorter period (so that a rotation by less than the period is a real shift)."""
    while True:
        u = _random(rng, period)
        if all(any(u[i] != u[(i + q) % period] for i in range(period)) for q in range(1, period)):
            return u


def _tandem(unit, L, phase=0):
    return [unit[(i + phase) % len(unit)] for i in range(L)]


def _plan_edits(rng, count, bound):
    """`count` edits as (type S / D / I, at the head or at the tail); neither the running net length change nor the part of it
    made at the head (the shift of the string's middle) ever leaves [-bound, bound]."""
    ops, net, shift = [], 0, 0
    for _ in range(count):
        op, head = "SDI"[int(rng.integers(0, 3))], bool(rng.random() < 0.5)
        step = {"S": 0, "D": -1, "I": 1}[op]
        if abs(net + step) > bound or (head and abs(shift + step) > bound):
            op, step = "S", 0
        net, shift = net + step, shift + (step if head else 0)
        ops.append((op, head))
    return ops, net


def _end_edits(rng, a, ops, fill):
    """b = a after `ops`, every one of them within ZONE characters of an end of a: the middle of a repeat stays a run of equal
    characters on every diagonal, L - 2 ZONE - |shift - d| long, whatever the edits do.  `fill(i)`: the repeat's own character
    at i, so that an insertion lengthens the repeat rather than breaking it."""
    L = len(a)
    head, mid, tail = list(a[:ZONE]), list(a[ZONE:L - ZONE]), list(a[L - ZONE:])
    for op, at_head in ops:
        part = head if at_head else tail
        if op == "S":
            p = int(rng.integers(0, len(part)))
            part[p] = _other(rng, part[p])
        elif op == "D":
            del part[int(rng.integers(0, len(part)))]
        else:
            p = int(rng.integers(0, len(part) + 1))
            part.insert(p, fill(p) if rng.random() < 0.5 else _ACGT[rng.integers(0, 4)])
    return head + mid + tail


WORD_EDGES = (31, 32, 63, 64, 95, 96, 127, 128, 191, 192, 255, 256)


def _scattered_edits(rng, a, ops, fill):
    """b = a after `ops` anywhere in the string: every other edit on a 32-bit word edge, the rest at random places (the middle of
    the repeat included), so that a repeat's long extensions and its ties break inside the string and on word edges too."""
    b = list(a)
    for op, _ in ops:
        edges = [w for w in WORD_EDGES if w < len(b)]
        p = edges[int(rng.integers(0, len(edges)))] if edges and rng.random() < 0.5 else int(rng.integers(0, len(b)))
        if op == "S":
            b[p] = _other(rng, b[p])
        elif op == "D":
            del b[p]
        else:
            b.insert(p, fill(p) if rng.random() < 0.5 else _ACGT[rng.integers(0, 4)])
    return b


def _repeat_edits(rng, j, a, ops, fill):
    """Rounds of six variants take turns: edits at the ends only (the middle keeps its run on every diagonal), edits anywhere."""
    where = "scattered" if (j // 6) % 2 else "ends"
    return (_scattered_edits if where == "scattered" else _end_edits)(rng, a, ops, fill), where


def _lengths(rng, lo, hi, count, variants):
    """The longer string's length per pair: the first third (at least three rounds) cycles through EDGES inside [lo, hi], one
    step further whenever edges and variants have come round together, so that a variant meets more than one edge; then uniform in [lo, hi]."""
    edges = [L for L in EDGES if lo <= L <= hi] or [hi]
    cut = max(3 * len(edges), count // 3)
    block = int(np.lcm(len(edges), variants))
    return [edges[(j + j // block) % len(edges)] if j < cut else int(rng.integers(lo, hi + 1)) for j in range(count)]


def gap_lengths(k, max_diff=None):
    """block_gap's g: 1, k - 1, k, k + 1, at least 1 and capped at max_diff where a comparison bounds the length difference."""
    cap = max_diff if max_diff is not None else k + 1
    return [max(1, min(g, cap)) for g in (1, k - 1, k, k + 1)]


def _gap_position(rng, placement, L, g):
    """Where a gap of g starts in a string of L (the deleted characters are [p, p + g))."""
    if placement == "start":
        return 0
    if placement == "end":
        return L - g
    if placement == "word_edge":
        inside = [w for w in (32, 64, 96, 128, 192, 256, 384) if w + g <= L]
        return inside[int(rng.integers(0, len(inside)))] if inside else max(0, L - g) // 2
    return int(rng.integers(0, L - g + 1))


def _pair(rng, kind, j, L, hi, k, bound, max_diff):
    """One pair of `kind`, variant j, whose longer string has exactly L characters (hi: the longest the class allows); bound:
    the most the lengths may differ."""
    meta = {"kind": kind, "L": L}
    if kind == "homopolymer":
        c = _ACGT[j % 4]
        ops, net = _plan_edits(rng, j % 6, bound)
        a = [c] * (L - max(net, 0))
        b, where = _repeat_edits(rng, j, a, ops, lambda p: c)
        meta.update(letter=chr(c), period=1, edits=where)
    elif kind in ("tandem", "dirty_repeat"):
        period = 2 + j % 6
        unit = _unit(rng, period)
        ops, net = _plan_edits(rng, j % 6, bound)
        # every other pair: one whole period deleted or inserted as well, where the bound on the length difference allows it
        whole = 0
        if j % 2:
            whole = period if (j // 2) % 2 else -period
            if max_diff is not None and abs(net + whole) > max_diff:
                whole = 0
        a = _tandem(unit, L - max(net + whole, 0))
        b, where = _repeat_edits(rng, j, a, ops, lambda p: unit[p % period])
        if whole:
            p = period + ZONE + int(rng.integers(0, max(1, len(b) - 2 * (ZONE + period))))
            b = b[:p] + b[p - period:p] + b[p:] if whole > 0 else b[:p] + b[p + period:]
        meta.update(period=period, whole_period=whole, edits=where)
    elif kind == "shifted":
        s = 1 + (j // 2) % (k + 1)
        s = min(s, L - 1)
        a = _random(rng, L)
        b = a[s:] + _random(rng, s) if j % 2 == 0 else _random(rng, s) + a[:L - s]
        meta.update(shift=s if j % 2 else -s)
    elif kind == "rotated_repeat":
        s = 1 + j % (k + 1)  # every rotation within k + 1 pairs; the period moves on one step more per round of rotations
        period = 2 + (j % (k + 1) + j // (k + 1)) % 6
        unit = _unit(rng, period)
        a, b = _tandem(unit, L), _tandem(unit, L, s)
        meta.update(period=period, rotation=s)
    elif kind == "block_gap":
        gaps = gap_lengths(k, max_diff)
        g = min(gaps[j % 4], L - 1)
        insertion = (j // 4) % 2 == 1
        placement = PLACEMENTS[(j // 8) % 4]
        a = _random(rng, L)
        p = _gap_position(rng, placement, L, g)
        b = a[:p] + a[p + g:]
        if insertion:  # the same gap seen from the other side: g random characters inserted into the shorter string
            a, b = b, b[:p] + _random(rng, g) + b[p:]
        meta.update(gap=g, insertion=insertion, placement=placement, at=p)
    elif kind == "edge_edits":
        # every listed position below the class's longest string, and the last character; a string too short for its
        # position is made the longest of the class
        w = (EDIT_POSITIONS + (None,))[(j // 3) % (len(EDIT_POSITIONS) + 1)]
        if w is None or w >= hi:
            w = L - 1
        elif w >= L:
            L = hi
            meta["L"] = L
        form = ("substitution", "deletion", "insertion")[j % 3]
        a = _random(rng, L)
        if form == "substitution":
            b = a[:w] + [_other(rng, a[w])] + a[w + 1:]
        elif form == "deletion":
            b = a[:w] + a[w + 1:]
        else:
            b = a[:w] + a[w + 1:]
            a, b = b, a  # the longer string is the one with the inserted character at w
        meta.update(at=w, form=form)
    elif kind == "unrelated":
        a = _random(rng, L)
        if j % 2:
            b = [_COMPLEMENT[int(c)] for c in a]
        else:
            b = _random(rng, L)
        meta.update(complement=bool(j % 2))
    else:
        raise ValueError(kind)
    if kind in REPEAT_KINDS + ("dirty_repeat", "unrelated") and j % 4 >= 2:
        a, b = b, a  # either string may be the read
    return a, b, meta


def _dirty(rng, s):
    s = np.array(s, np.uint8)
    hit = rng.random(s.size) < 0.01
    s[hit] = rng.choice(DIRTY, int(hit.sum()))
    return s, int(hit.sum())


def _build(asm, specs, lo, hi, k, seed, max_diff):
    """specs: (kind, variant index, length) per pair, in batch order."""
    rng = np.random.default_rng(seed)
    bound = k if max_diff is None else min(k, max_diff)
    reads, refs, metas = [], [], []
    for kind, j, L in specs:
        a, b, meta = _pair(rng, kind, j, L, hi, k, bound, max_diff)
        a, b = np.array(a, np.uint8), np.array(b, np.uint8)
        if kind == "dirty_repeat":
            (a, da), (b, db) = _dirty(rng, a), _dirty(rng, b)
            meta.update(kind=kind, dirty=da + db)
        assert lo <= max(len(a), len(b)) <= hi, (meta, len(a), len(b))
        assert max_diff is None or abs(min(len(a), 128) - min(len(b), 128)) <= max_diff, meta
        reads.append(a), refs.append(b), metas.append(meta)
    ro = np.zeros(len(specs) + 1, np.uint32)
    fo = np.zeros(len(specs) + 1, np.uint32)
    ro[1:] = np.cumsum([len(a) for a in reads])
    fo[1:] = np.cumsum([len(b) for b in refs])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    hb = asm.HostBatch(cat(reads), ro, cat(refs), fo)
    hb.kinds = np.array([m["kind"] for m in metas])
    hb.meta = metas
    return hb


def _variants(kind, k):
    return {"homopolymer": 12, "tandem": 12, "dirty_repeat": 12, "shifted": 2 * (k + 1), "rotated_repeat": 6 * (k + 1), "block_gap": 32,
            "edge_edits": 33, "unrelated": 2}[kind]


def structured_batch(asm, kind, lo, hi, k, n, seed, max_diff=None):
    """n pairs of one kind whose longer string lies in [lo, hi], so that the dispatch arm is known.  k: the band the batch is
    meant for (shifts 1 .. k + 1, gaps 1, k - 1, k, k + 1; the random edits of the repeat kinds change the length by at most
    k).  max_diff: where given (a Greedy comparison passes k), no pair's lengths, each cut at 128 as Greedy cuts them,
    differ by more — gaps and whole-period indels are capped to it — so that tests/util.greedy_defined leaves the pairs in."""
    rng = np.random.default_rng([seed, lo, hi, k, KINDS.index(kind)])
    lengths = _lengths(rng, lo, hi, n, _variants(kind, k))
    return _build(asm, [(kind, j, lengths[j]) for j in range(n)], lo, hi, k, int(rng.integers(0, 2 ** 31)), max_diff)


def all_kinds_batch(asm, lo, hi, k, n=N, seed=0, max_diff=None, kinds=KINDS):
    """The kinds interleaved pair by pair, so that neighbouring lanes of a wavefront — and, where a thread takes two pairs, the
    two halves of one thread — hold different kinds.  A kind named more than once in `kinds` takes that many of the turns."""
    rng = np.random.default_rng([seed, lo, hi, k, 99])
    turns = [kinds[i % len(kinds)] for i in range(n)]
    lengths = {kind: _lengths(rng, lo, hi, turns.count(kind), _variants(kind, k)) for kind in dict.fromkeys(kinds)}
    seen, specs = dict.fromkeys(kinds, 0), []
    for kind in turns:
        specs.append((kind, seen[kind], lengths[kind][seen[kind]]))
        seen[kind] += 1
    return _build(asm, specs, lo, hi, k, int(rng.integers(0, 2 ** 31)), max_diff)


# Three turns in eight for the pairs that no banded or windowed pass can answer, for the cases whose subject is the fallback behind
# those passes; the repeats and the gaps stay in, next to them.
FAR_HEAVY = ("unrelated", "homopolymer", "block_gap", "unrelated", "tandem", "shifted", "unrelated", "rotated_repeat")


def removed_share_by_kind(hb, keep):
    """Share of each kind's pairs that a predicate (`keep`: bool per pair) leaves out."""
    return {kind: float(1.0 - keep[hb.kinds == kind].mean()) for kind in np.unique(hb.kinds)}


def assert_predicate_leaves_most(hb, keep, what):
    """Every test that applies greedy_defined or leap_defined: at most 10 % of each kind may go."""
    shares = removed_share_by_kind(hb, keep)
    assert max(shares.values()) <= 0.10, (what, shares)
    return shares


def diagonal_runs(a, b, k):
    """{d: longest run of equal characters a[i] == b[i + d] that crosses a multiple of 32 (in a's or in b's index)} for every
    diagonal d in [-k, k] that exists for the two lengths."""
    a, b = np.frombuffer(a.encode(), np.uint8), np.frombuffer(b.encode(), np.uint8)
    out = {}
    for d in range(-k, k + 1):
        i0, i1 = max(0, -d), min(len(a), len(b) - d)
        if i1 <= i0:
            continue
        eq = a[i0:i1] == b[i0 + d:i1 + d]
        edge = np.flatnonzero(np.concatenate(([True], ~eq, [True])))  # run r covers eq[edge[r] : edge[r + 1] - 1]
        best = 0
        for s, e in zip(edge[:-1], edge[1:] - 1):
            if e > s:
                first, last = i0 + s, i0 + e - 1  # a's indices of the run; b's are + d
                crosses = (first // 32 != last // 32) or ((first + d) // 32 != (last + d) // 32)
                if crosses:
                    best = max(best, int(e - s))
        out[d] = best
    return out


def as_packed(asm, hb):
    """The batch as the pack kernel's planes hold it: every byte but C, G and T is code 00, the same as A (the rule Greedy's and
    the filters' oracle applies byte by byte; the oracle's LEAP and NW compare characters and are given this batch)."""
    as_a = np.full(256, ord("A"), np.uint8)
    as_a[[ord("C"), ord("G"), ord("T")]] = [ord("C"), ord("G"), ord("T")]
    seen = asm.HostBatch(as_a[hb.reads], hb.read_off, as_a[hb.refs], hb.ref_off)
    seen.kinds, seen.meta = hb.kinds, hb.meta
    return seen
