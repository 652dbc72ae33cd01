"""The payload corpus of the deflate container's tests (docs/design/mapper.md, "Deflate"), shared by tests/test_deflate_host.py and
tests/test_gpu_deflate.py, and what both check on a container: every block inflates to its payload with the right CRC and ISIZE
(bam_cases.bgzf_blocks), none is longer than its stored form, and the cut is the one of the stored container.  check_tokens reads
the contract back from every block's tokens with the decoder of tests/inflate_cases.py; adversarial() is a second corpus, of inputs
built for one edge of the encoder each.

Two measured ratios bound the encoder's output from above.  Against zlib level 1 on the record fill: 0.9844, cap 1.083
(test_deflate_host.test_record_fill_against_zlib).  dfl_lengths' code against the package-merge optimum where the length limit
binds, on Fibonacci, power-of-two and flat weights (test_deflate_host.test_lengths_under_the_limit):

    limit   cases where it binds   worst ratio   at             cap = worst + (worst - 1) / 10
    7       33                     1.11004       fibonacci 19   1.1211
    15      811                    1.00266       fibonacci 27   1.00293

and the emitted blocks of the adversarial corpus where a limit binds, token bits against package-merge (the table at OPTIMALITY_CAP):
worst 1.000349, cap 1.000384.
"""
import gzip
import random
import struct

from tests import bam_cases as bc
from tests import inflate_cases as ic

P = bc.PAYLOAD
SIZES = (1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 1023, 1024, 1025, P - 1, P, P + 1, 2 * P + 1)
PERIODS = (1, 2, 3, 63, 64, 65, 258, 259, 1023, 1025, 32767, 32768, 32769)
FILLS = ("zeros", "random", "records", "text")
COMPRESSIBLE = ("zeros", "records", "text")     # every full block must come out smaller than stored


def _records(n, rng):
    out, t = [], 0
    while sum(len(r) for r in out) < n:
        seq = "".join(rng.choice("ACGT") for _ in range(100))
        out.append(bc.encode_record(ref_id=t % 3, pos=1000 + 37 * t, mapq=rng.choice((0, 3, 58, 60)), flag=rng.choice((0, 16)), next_id=-1,
                                    next_pos=-1, tlen=0, name="read.%07d" % t, cigar=[(100, "M")], seq=seq,
                                    qual=bytes(rng.randrange(2, 41) for _ in range(100)),
                                    tags=[("NM", "C", rng.randrange(3)), ("XG", "c", -rng.randrange(9)), ("MD", "Z", "100")]))
        t += 1
    return b"".join(out)[:n]


def _text(n, rng):
    out, t = [], 0
    while sum(len(r) for r in out) < n:
        seq = "".join(rng.choice("ACGT") for _ in range(100))
        qual = "".join(chr(33 + rng.randrange(2, 41)) for _ in range(100))
        out.append(("read.%07d\t%d\tchr%d\t%d\t60\t100M\t*\t0\t0\t%s\t%s\tNM:i:%d\n" % (t, rng.choice((0, 16)), t % 3, 1000 + 37 * t, seq, qual,
                                                                                     rng.randrange(3))).encode())
        t += 1
    return b"".join(out)[:n]


def fill(kind, n, seed=7):
    rng = random.Random(seed * 1000003 + n)
    return {"zeros": lambda: bytes(n), "random": lambda: rng.randbytes(n), "records": lambda: _records(n, rng),
            "text": lambda: _text(n, rng)}[kind]()


def corpus():
    """-> {name: payload}; built once per process"""
    if not _CORPUS:
        for kind in FILLS:
            for n in SIZES:
                _CORPUS["%s %d" % (kind, n)] = fill(kind, n)
        rng = random.Random(23)
        letters = b"ACGTNacgtn0123456789\t:"
        for p in PERIODS:
            unit = bytes(rng.choice(letters) for _ in range(p))
            _CORPUS["period %d" % p] = (unit * (P // p + 1))[:P]
        half = rng.randbytes(32769)
        _CORPUS["copy at 32769"] = (half + half)[:P]        # every repeat lies one byte further back than deflate can reach
        _CORPUS["all bytes"] = bytes(t & 255 for t in range(P))
        _CORPUS["one byte"] = b"Q"
        _CORPUS["long run"] = rng.randbytes(700) + b"\xa5" * 3000 + rng.randbytes(700)     # far more than 258 equal bytes
    return _CORPUS


_CORPUS = {}


def check_container(data, src, eof=True):
    """the container of src at level 1 -> its data blocks; checks what every such container must satisfy"""
    blocks = bc.bgzf_blocks(data)
    if eof:
        assert blocks and data.endswith(bc.EOF_BLOCK) and blocks[-1]["payload"] == b""
        blocks = blocks[:-1]
    assert [b["payload"] for b in blocks] == [src[a:a + P] for a in range(0, len(src), P)], "the cut is the stored container's"
    assert gzip.decompress(data) == src if data else src == b""
    for b in blocks:
        assert b["bsize"] <= len(b["payload"]) + 31, "a block of %d bytes for %d" % (b["bsize"], len(b["payload"]))
        assert b["deflate"][0] & 1 == 1, "BFINAL"
        if btype(b) == 0:
            assert b["bsize"] == len(b["payload"]) + 31
    return blocks


def btype(block):
    return (block["deflate"][0] >> 1) & 3


def decode(data: bytes) -> bytes:
    """bam_cases.decode for a container at any level: bam_cases.parse_bam insists on stored blocks"""
    stream = b"".join(b["payload"] for b in bc.bgzf_blocks(data))
    assert data.endswith(bc.EOF_BLOCK) and gzip.decompress(data) == stream
    text, refs, at = bc.parse_header(stream)
    names = [n for n, _ in refs]
    return text + "".join(bc.sam_line(r, names) for r in bc.records_of(stream, at)).encode("latin-1")


def header_bytes(data: bytes) -> int:
    """the bytes of the blocks that hold the BAM header of a file (the header goes in blocks of its own)"""
    blocks = bc.bgzf_blocks(data)
    stream = b"".join(b["payload"] for b in blocks)
    _, _, at = bc.parse_header(stream)
    seen = size = 0
    for b in blocks:
        if seen >= at:
            break
        seen += len(b["payload"])
        size += b["bsize"]
    assert seen == at
    return size


def u16(data, at):
    return struct.unpack_from("<H", data, at)[0]


# ---- the contract, read back from the tokens ------------------------------------------------------------------------------------------
SLICE = 64
TOO_FAR = 4096
_CHECKED = {}


def check_tokens(block, payload, counts=None):
    """One block (an entry of bam_cases.bgzf_blocks) of `payload` against the contract of docs/design/mapper.md, "Deflate", read
    back by the decoder of tests/inflate_cases.py: the match rules, the code lengths, the header's fields and runs, the choice of the
    type, BSIZE and the padding.  counts: the (fixed, dynamic) bit counts of the host checker's `counts` form, which a
    stored block and, for the dynamic count, a fixed block do not show in their bytes; without them that part of the choice is not
    checked (the device's bytes are held against the host's, which are).  For a fixed block the rule "fixed <= dynamic" rests on the
    encoder's own dynamic count, bounded from below only by the tokens' Huffman cost and the smallest header there is (17 bits of
    fields, four code-length lengths); a dynamic count that is wrong above that floor and still leaves the block fixed is not seen
    here.  -> the decoded block"""
    key = (bytes(block["deflate"]), block["bsize"], counts)
    if key in _CHECKED:
        assert _CHECKED[key]["payload"] == payload
        return _CHECKED[key]
    data = block["deflate"]
    inf = ic.inflate(data)
    assert inf["payload"] == payload and block["payload"] == payload, "the decoder, zlib and the payload agree"
    n, typ, end = len(payload), inf["btype"], inf["end_bit"]
    stored = 40 + 8 * n
    # padding: the stream ends in the byte of the last bit, and what that byte has left is zero
    assert len(data) == (end + 7) // 8, (len(data), end)
    assert end % 8 == 0 or data[-1] >> (end % 8) == 0, "padding bits"
    assert block["bsize"] == 18 + (end + 7) // 8 + 8
    if typ == 0:
        assert end == stored
        if counts is not None:
            assert stored <= counts[0] and stored <= counts[1], ("stored was not the cheapest", stored, counts)
        _CHECKED[key] = inf
        return inf
    # the match rules
    at = 0
    for t in inf["tokens"]:
        assert t[0] == at, "the tokens tile the payload"
        if len(t) == 2:
            at += 1
            continue
        _, length, dist = t
        assert 3 <= length <= SLICE and 1 <= dist <= 32768, t
        assert at // SLICE == (at + length - 1) // SLICE, ("a match across a slice's end", t)
        assert length > 3 or dist <= TOO_FAR, ("three bytes from too far back", t)
        at += length
    assert at == n
    fixed = 3 + ic.token_bits(inf["tokens"], ic.FIXED_LL, ic.FIXED_D)
    if typ == 1:
        assert end == fixed
        assert fixed < stored, ("fixed chosen over a cheaper stored block", fixed, stored)
        if counts is not None:
            ll, d = ic.histograms(inf["tokens"])
            floor = 3 + 14 + 3 * 4 + ic.cost(ll, ic.huffman_lengths(ll)) + ic.cost(d, ic.huffman_lengths(d))     # no dynamic block has fewer
            assert counts[0] == fixed and fixed <= counts[1] and counts[1] >= floor, ("fixed was not the cheapest", fixed, counts)
        _CHECKED[key] = inf
        return inf
    # the code lengths
    ll, d, cl = inf["ll_lens"], inf["d_lens"], inf["cl_lens"]
    assert max(ll) <= 15 and max(d) <= 15 and max(cl) <= 7
    assert ic.kraft(ll) == 1 << 15 and ic.kraft(d) == 1 << 15 and ic.kraft(cl) == 1 << 15, "a complete code, the dummies counted"
    dyn = inf["head_bits"] + ic.token_bits(inf["tokens"], ll + [0] * (286 - len(ll)), d + [0] * (30 - len(d)))    # asserts nonzero lengths
    assert all(cl[s] for s, _ in inf["head_syms"])
    # the header
    assert inf["hlit"] == max(257, max(s for s, v in enumerate(ll) if v) + 1), "HLIT"
    assert inf["hdist"] == max(1, max(s for s, v in enumerate(d) if v) + 1), "HDIST"
    assert inf["hclen"] == max(4, max(i for i, s in enumerate(ic.CL_ORDER) if cl[s]) + 1), "HCLEN"
    check_head_runs(inf["head_syms"])
    # the choice
    assert end == dyn
    assert dyn < stored and dyn < fixed, ("dynamic chosen over a cheaper type", stored, fixed, dyn)
    if counts is not None:
        assert counts == (fixed, dyn), (counts, fixed, dyn)
    _CHECKED[key] = inf
    return inf


def check_head_runs(syms):
    """the header's symbols: 16 covers 3 to 6, 17 covers 3 to 10, 18 covers 11 to 138 (their extra bits say no more than that), a 16
    has a length in front of it, and no stretch of plain symbols spells out what a repeat symbol could have covered: three zeros, or
    three lengths behind an equal one"""
    last, zeros, repeats = None, 0, 0
    for s, x in syms:
        if s == 16:
            assert 0 <= x <= 3 and last not in (None, 0), "a repeat of nothing or of zero"
            zeros = repeats = 0
        elif s >= 17:
            assert 0 <= x <= (7 if s == 17 else 127)
            last, zeros, repeats = 0, 0, 0
        elif s == 0:
            last, zeros, repeats = 0, zeros + 1, 0
            assert zeros < 3, "three zeros spelled out"
        else:
            repeats = repeats + 1 if s == last else 0
            last, zeros = s, 0
            assert repeats < 3, "three lengths behind an equal one spelled out"


# ---- the adversarial corpus -------------------------------------------------------------------------------------------------------------
# Inputs built for one edge of the encoder each.  An entry is (payload, property): the property takes the decoded blocks
# (check_tokens' results) and asserts that the payload reached its edge, so an input that drifts away from it fails and does not pass
# unnoticed.  The names start with the letter of their group.
#
# Two building blocks make the tokens predictable under this encoder's two-candidate match finder:
#   planted()  strings in a background of zeros: a zero run is matched against the window's first zeros, a planted string against
#              its only earlier copy, and nothing else repeats
#   tails()    slices of 62 zeros and two bytes: a match needs three bytes inside its slice, so the bytes at offsets 62 and 63 of a
#              slice are literals whatever they are, in exactly the counts that were asked for
W = 1024


def planted(n, strings):
    out = bytearray(n)
    for at, s in strings.items():
        assert 0 <= at and at + len(s) <= n and not any(out[at:at + len(s)])
        out[at:at + len(s)] = s
    return bytes(out)


def tails(counts, marker, seed):
    """a full block of slices [62 zeros, x, y]: x = marker in the first slice of every window (the slice every zero run of the window
    is matched against, so the match ends in front of x), every other x and y drawn without replacement from counts {byte: count};
    what is left over stays zero"""
    slots = [(s, o) for s in range(P // SLICE) for o in (62, 63) if not (o == 62 and s % (W // SLICE) == 0)]
    pool = [b for b, c in sorted(counts.items()) for _ in range(c)]
    assert len(pool) <= len(slots) and marker not in counts and 0 not in counts
    random.Random(seed).shuffle(slots)
    out = bytearray(P)
    for s in range(0, P // SLICE, W // SLICE):
        out[SLICE * s + 62] = marker
    for b, (s, o) in zip(pool, slots):
        out[SLICE * s + o] = b
    return bytes(out)


def de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence of order n over k letters (Fredricksen, Kessler and Maiorana): every n-gram
    occurs once, so no prefix of it repeats one"""
    a, out = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return out


def matches(inf):
    return [t for t in inf["tokens"] if len(t) == 3]


def token_at(inf, at):
    hit = [t for t in inf["tokens"] if t[0] == at]
    assert hit, "no token starts at %d" % at
    return hit[0]


def head_runs(inf):
    """the header's symbols by the place they start at in the lengths (literal/length first, distances behind HLIT):
    {place: (symbol, how many lengths it stands for)}"""
    out, at = {}, 0
    for s, x in inf["head_syms"]:
        n = 1 if s < 16 else 3 + x if s in (16, 17) else 11 + x
        out[at] = (s, n)
        at += n
    return out


def _unique_text(symbols, n, seed):
    """n bytes over `symbols` with no 4-gram twice: a de Bruijn sequence's prefix, its letters mapped through a seeded permutation"""
    order = list(symbols)
    random.Random(seed).shuffle(order)
    seq = de_bruijn(len(order), 4)
    assert n <= len(seq)
    start = len(seq) // 3                                                     # past the first, nearly constant stretch
    return bytes(order[v] for v in (seq + seq[:3])[start:start + n])


def adversarial():
    """-> {name: (payload, property)}; built once per process"""
    if _ADVERSARIAL:
        return _ADVERSARIAL
    add = _ADVERSARIAL.__setitem__

    # (d) header run edges.  The first occurrence of a byte value is always a literal, so the used literals are the payload's byte set
    # and the zero runs between them are its gaps.
    def gaps_entry(gaps, seed):
        used, at = [], 0
        for g in gaps:
            used += list(range(at, at + 5))
            at += 5 + g
        used += list(range(at, min(at + 5, 256)))
        assert at < 256
        starts, at = [], 0
        for g in gaps:
            starts.append(at + 5)
            at += 5 + g
        src = _unique_text(used, 3000, seed)

        def prop(infs):
            inf, = infs
            assert inf["btype"] == 2
            runs, want = head_runs(inf), []
            for g, at in zip(gaps, starts):
                spell, left, place = [], g, at
                while left >= 11:
                    spell.append((place, (18, min(left, 138))))
                    place, left = place + min(left, 138), left - min(left, 138)
                if left >= 3:
                    spell.append((place, (17, left)))
                    place, left = place + left, 0
                spell += [(place + i, (0, 1)) for i in range(left)]
                for where, what in spell:
                    assert runs.get(where) == what, (g, where, what, runs.get(where))
                want.append((g, [w for _, w in spell]))
            print("header zero runs:", want)
        return src, prop
    add("d zero runs 2 3 10 11 12", gaps_entry((2, 3, 10, 11, 12), 1))
    add("d zero run 138", gaps_entry((138,), 2))
    add("d zero run 139", gaps_entry((139,), 3))
    add("d zero run 149", gaps_entry((149,), 4))

    src = _unique_text(range(48, 64), 3000, 5)
    # Without a match the distance alphabet is the two dummies, symbols 0 and 1 with one bit each, so HDIST is 2: the floor of 1
    # cannot be reached by any payload, as in zlib.
    add("d no match", (src, lambda infs: _no_match(infs)))
    add("d one match at distance 1", (src[:1500] + b"\xee" * 9 + src[1500:], lambda infs: _one_match(infs)))
    add("d literal 255 and length 64", (src[:1472] + b"\xff" + bytes(63 + 128) + src[1472:], lambda infs: _hlit_277(infs)))
    add("d distance symbol 29", (planted(P, {100: src[:40], 100 + 30000: src[:40]}), lambda infs: _dist_29(infs)))
    _more(add, src)
    _deep(add)
    return _ADVERSARIAL


def cl_histogram(inf):
    out = [0] * 19
    for s, _ in inf["head_syms"]:
        out[s] += 1
    return out


def optimality(inf):
    """(c) a dynamic block's token bits under its own two codes over the same tokens' bits under package-merge lengths of at most 15
    bits for the same histograms (the optimum; the extra bits are the same on both sides and left out)"""
    ll, d = ic.histograms(inf["tokens"])
    own = ic.cost(ll, inf["ll_lens"] + [0] * 30) + ic.cost(d, inf["d_lens"] + [0] * 30)
    best = ic.cost(ll, ic.package_merge_lengths(ll, 15)) + ic.cost(d, ic.package_merge_lengths(d, 15))
    return own / best


# (c) measured on the host build over the (a) and (b) entries, every dynamic block:
#
#   entry                         ratio to package-merge
#   a records 65280 seed 1        1.000260
#   a records 65280 seed 18       1.000266
#   a records 65279 seed 14       1.000280
#   a records 65279 seed 23       1.000349   (the worst)
#   b records 65279 seed 7        1.000000   (the literal/length limit does not bind there)
#
# cap = worst + (worst - 1) / 10 = 1.000384
OPTIMALITY_CAP = 1.000384


def _deep(add):
    # (a) deep codes.  Shuffled Fibonacci and 2^i byte histograms do not get there (the match finder takes the frequent bytes' repeats
    # away: depths 10, 13, 14, 14), but the record fill does: its length symbols and rare quality bytes sit below thousands of base
    # letters.  Found by a seeded search over fill("records", n, seed); the seeds and sizes are the ones below.
    def deep(infs):
        inf, = infs
        ll, _ = ic.histograms(inf["tokens"])
        depth, ratio = max(ic.huffman_lengths(ll)), optimality(inf)
        print("unlimited literal/length depth %d, longest code %d, to package-merge %.6f" % (depth, max(inf["ll_lens"]), ratio))
        assert inf["btype"] == 2 and depth > 15 and max(inf["ll_lens"]) == 15
        assert ic.cost(ll, ic.package_merge_lengths(ll, 15)) > ic.cost(ll, ic.huffman_lengths(ll)), "the limit costs bits: it binds"
        assert 1.0 <= ratio <= OPTIMALITY_CAP, ratio
    for n, seed in ((P, 1), (P, 18), (P - 1, 14), (P - 1, 23)):
        add("a records %d seed %d" % (n, seed), (fill("records", n, seed), deep))

    # (b) limit 7: the header of this record fill has a code-length histogram of unlimited depth 8
    def deep_header(infs):
        inf, = infs
        depth, ratio = max(ic.huffman_lengths(cl_histogram(inf))), optimality(inf)
        print("unlimited code-length depth %d, longest code %d, to package-merge %.6f" % (depth, max(inf["cl_lens"]), ratio))
        assert inf["btype"] == 2 and depth > 7 and max(inf["cl_lens"]) == 7
        assert 1.0 <= ratio <= OPTIMALITY_CAP, ratio
    add("b records %d seed 7" % (P - 1), (fill("records", P - 1, 7), deep_header))

    # (g) the widest token: a length code, 3 extra bits, a distance code and 13 extra bits.  12 000 bytes of records and 14 000 of text
    # hold few distances beyond 24 576, so distance symbol 29 has a long code; the copy of a whole slice from 128 to 25 792 is the one
    # match of 64 bytes that far back.  (Seed 1 of a seeded search over the two fills' seeds and sizes.)
    src = bytearray(fill("records", 12000, 1) + fill("text", 14000, 1) + fill("records", 2000, 101))
    src[25792:25792 + 64] = src[128:192]

    def widest(infs):
        inf, = infs
        t, k = token_at(inf, 25792), [x[0] for x in inf["tokens"]].index(25792)
        print("the token %s takes %d bits" % (t, inf["widths"][k]))
        assert inf["btype"] == 2 and t == (25792, 64, 25664) and inf["widths"][k] >= 40 and max(inf["widths"]) <= 48
    add("g widest token", (bytes(src), widest))


def _lit(inf, at, n=1):
    for k in range(n):
        assert len(token_at(inf, at + k)) == 2, ("not a literal", token_at(inf, at + k))


def _is(at, length, dist, longer=False):
    """the property: the token at `at` is the match (length, dist); longer: at least that long (zeros follow both copies)"""
    def prop(infs):
        t = token_at(infs[0], at)
        assert len(t) == 3 and t[2] == dist and (t[1] >= length if longer else t[1] == length), t
        assert all(m[2] <= 32768 for inf in infs for m in matches(inf))
    return prop


def _more(add, text):
    s8, rng = bytes(text[8:16]), random.Random(41)
    assert len(set(s8[k:k + 4] for k in range(5))) == 5

    # (d) equal-length runs of exactly 9, 7, 6, 4, 3 and 2 among the used literals, from exact literal counts
    sizes, weights, counts, groups, at = (9, 7, 6, 4, 3, 2), (5, 12, 28, 90, 150, 400), {}, [], 10
    for r, c in zip(sizes, weights):
        groups.append((at, r))
        counts.update({b: c for b in range(at, at + r)})
        at += r + 1

    def equal_runs(infs):
        inf, = infs
        runs, spelled = head_runs(inf), {9: [1, 6, 1, 1], 7: [1, 6], 6: [1, 5], 4: [1, 3], 3: [1, 1, 1], 2: [1, 1]}
        for a, r in groups:
            v = inf["ll_lens"][a]
            assert v and inf["ll_lens"][a - 1:a + r + 1] == [0] + [v] * r + [0], (a, r, inf["ll_lens"][a - 1:a + r + 1])
            place = a
            for k, n in enumerate(spelled[r]):
                assert runs.get(place) == ((16 if n >= 3 else v), n), (a, r, place, runs.get(place))
                place += n
        print("header length runs:", [(r, spelled[r]) for _, r in groups])
    add("d equal length runs", (tails(counts, 200, 3), equal_runs))

    # (e) match-rule edges, planted in zeros
    def lits_at(at, n):
        def prop(infs):
            _lit(infs[0], at, n)
            assert all(m[2] <= 32768 and (m[1] > 3 or m[2] <= TOO_FAR) for m in matches(infs[0]))
        return prop
    add("e 3 bytes at 4096 taken", (planted(P, {253: s8[:5], 4349: s8[:5]}), _is(4349, 3, 4096)))
    add("e 3 bytes at 4097 dropped", (planted(P, {252: s8[:5], 4349: s8[:5]}), lits_at(4349, 3)))
    add("e 4 bytes at 4097 taken", (planted(P, {251: s8[:5], 4348: s8[:5]}), _is(4348, 4, 4097)))
    add("e 4 bytes at 32768 taken", (planted(P, {300: s8[:4], 33068: s8[:4]}), _is(33068, 4, 32768, longer=True)))
    add("e 4 bytes at 32769 not taken", (planted(P, {300: s8[:4], 33069: s8[:4]}), lits_at(33069, 4)))
    add("e stale far entry", (planted(P, {300: s8, 40300: s8}), lits_at(40300, 8)))

    def stale_and_near(infs):
        _lit(infs[0], 40300, 8)
        _is(40500, 8, 200, longer=True)(infs)
    add("e stale far entry, near copy", (planted(P, {300: s8, 40300: s8, 40500: s8}), stale_and_near))

    def straddle(infs):
        t = token_at(infs[0], 2048)                          # zeros follow both copies, so the second match runs on
        assert token_at(infs[0], 2038) == (2038, 10, 1838) and len(t) == 3 and t[1] >= 10 and t[2] == 1838, t
    s20 = bytes(text[100:120])
    add("e repeat across a slice end", (planted(P, {200: s20, 2038: s20}), straddle))

    def remainder(p, n):
        def prop(infs):
            _lit(infs[0], p, n)
            t = token_at(infs[0], p + n)
            assert len(t) == 3 and t[1] >= 8 - n and t[2] == 1912, t
        return prop
    add("e remainder 2 in the slice", (planted(P, {200 - 2: s8, 2110: s8}), remainder(2110, 2)))
    add("e remainder 1 in the slice", (planted(P, {200 - 1: s8, 2111: s8}), remainder(2111, 1)))
    # both copies agree for 20 bytes (the slice's end): the one in this window, 100 back, wins over the one 4 900 back
    add("e nearer of two equal", (planted(P, {200: s8, 5000: s8, 5100: s8}), _is(5100, 20, 100)))

    # (f) window and table edges
    for d in (1023, 1024, 1025):
        add("f copy at %d over the window seam" % d, (planted(P, {2036: s8, 2036 + d: s8}), _is(2036 + d, 8, d, longer=True)))
    add("f copy from the window's last slice", (planted(P, {2032: s8, 2048: s8}), _is(2048, 8, 16, longer=True)))
    add("f source across the window seam", (planted(P, {2046: s8, 3072: s8}), _is(3072, 8, 1026, longer=True)))
    grams = rng.randbytes(20000)

    def crowded(infs):
        """more distinct 4-grams in front of the repeat than `prev` has entries, so entries are overwritten.  The repeat at 20 000 has
        its copy 19 960 back: `prev` names the latest earlier-window place of its hash, so it is the match (8, 19960) if no later
        4-gram of the first 19 windows took that entry, and literals if one did; which, the bytes decide, and the rule is checked
        here from the bytes"""
        assert len(set(grams[k:k + 4] for k in range(19997))) > 4096
        assert infs[0]["btype"] == 0, "random bytes: the block is stored, and the host's bytes are the device's"
    add("f crowded tables", (grams + grams[40:48] + rng.randbytes(100), crowded))
    # the same crowding in a block that is not stored: 5 000 random 4-grams over 16 letters, the repeat of an early one behind them
    low = bytes(48 + (v & 15) for v in grams)
    crowd = low[:20000] + b"\xf0" + low[40:60] + b"\xf1" + low[20000:]

    def crowded_low(infs):
        inf, = infs
        assert len(set(low[k:k + 4] for k in range(19997))) > 4096 and inf["btype"] == 2
        t = token_at(inf, 20001)                             # behind the literal 0xf0, which no match can cover
        h = lambda x: (int.from_bytes(x, "little") * 0x9e3779b1 & 0xffffffff) >> 20      # the contract's 12-bit table
        later = [q for q in range(41, 19 * W) if h(low[q:q + 4]) == h(low[40:44]) and q + 4 <= len(crowd)]
        if later:                # a later place took the entry: whatever is found there, it is not the copy 19 961 back
            assert len(t) == 2 or t[2] != 19961, t
        else:
            assert len(t) == 3 and t[2] == 19961 and t[1] >= 4, t
        print("crowded tables: %d later places share the entry; the token at the repeat is %s" % (len(later), t))
    add("f crowded tables, low entropy", (crowd, crowded_low))

    def whole_windows(n):
        def prop(infs):
            inf, = infs
            assert inf["btype"] == 2 and len(inf["payload"]) == n
            last = [t for t in inf["tokens"] if t[0] >= (n - 1) // W * W]
            assert last and sum(1 if len(t) == 2 else t[1] for t in last) == n - last[0][0], "the last window's tokens end the payload"
        return prop
    for k in (1, 2, 63):
        for n in (W * k - 1, W * k, W * k + 1):
            add("f length %d" % n, (fill("text", n, seed=11), whole_windows(n)))
    for n in (2001, 2002, 2003):
        add("f match to the last byte of %d" % n, (planted(n, {100: s8[:6], n - 6: s8[:6]}), _is(n - 6, 6, n - 106)))
        add("f match at the last hashed place of %d" % n, (planted(n, {100: s8[:4], n - 4: s8[:4]}), _is(n - 4, 4, n - 104)))
    for n in (5, 6, 7):
        # a run: one literal and a match at distance 1 that ends at the last byte (n - 1 >= 4 bytes are hashed at place 1)
        add("f length %d" % n, (b"Q" * n, lambda infs, n=n: _short(infs, [(0, 81), (1, n - 1, 1)])))
        add("f length %d, distinct" % n, (bytes(range(65, 65 + n)), lambda infs, n=n: _short(infs, [(k, 65 + k) for k in range(n)])))

    # the choice: 30 distinct bytes of 9 bits make the fixed form 3 + 270 + 7 = 280 bits, the stored form's 40 + 8 * 30; stored wins
    # the tie (a dynamic header alone costs more than the 40 bits)
    tie = rng.sample(range(144, 256), 30)

    def stored(infs):
        assert infs[0]["btype"] == 0
    add("c stored ties with fixed", (bytes(tie), stored))


def mixed_blocks():
    """(h) the eight distinct payload blocks of the mixed container and the order of its 300 blocks (indices into them; the short
    tail last)"""
    rng = random.Random(59)
    adv = adversarial()
    seven = bytes(rng.choice(b"ACGTN\t\n") for _ in range(P))
    blocks = [fill("random", P), bytes(P), fill("text", P), fill("records", P), adv["a records %d seed 1" % P][0],
              adv["d equal length runs"][0], seven, fill("text", 40)]
    assert all(len(b) == P for b in blocks[:7])
    order = [rng.randrange(7) for _ in range(299)]
    order[:7] = range(7)
    rng.shuffle(order)
    return blocks, order + [7]


def _short(infs, tokens):
    assert infs[0]["btype"] == 1 and infs[0]["tokens"] == tokens, infs[0]["tokens"]


def _no_match(infs):
    inf, = infs
    assert inf["btype"] == 2 and not matches(inf), matches(inf)[:5]
    assert inf["hlit"] == 257 and inf["hdist"] == 2 and inf["d_lens"] == [1, 1]
    print("no match: HLIT %d, HDIST %d, distance lengths %s" % (inf["hlit"], inf["hdist"], inf["d_lens"]))


def _one_match(infs):
    inf, = infs
    assert inf["btype"] == 2 and [t[1:] for t in matches(inf)] == [(8, 1)], matches(inf)[:5]
    assert inf["hdist"] == 2 and inf["d_lens"] == [1, 1], "distance symbol 0 and one dummy"


def _hlit_277(infs):
    inf, = infs
    assert inf["btype"] == 2 and inf["hlit"] == 277 and inf["ll_lens"][255] and inf["ll_lens"][276]
    assert any(t[1] == 64 for t in matches(inf))


def _dist_29(infs):
    inf, = infs
    assert inf["btype"] == 2 and inf["hdist"] == 30 and inf["d_lens"][29]
    t = token_at(inf, 30100)
    assert len(t) == 3 and t[1] >= 40 and t[2] == 30000, t


_ADVERSARIAL = {}
