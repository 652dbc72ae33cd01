"""A byte-level reference parser of the harness's `>read\\n<ref\\n` text and a corpus of texts built for the edges of the device parser
(csrc/asm_ingest.h) and of the streamed path around it (asm_stream_seq_file in csrc/asm_capi.hip, PairsFill in csrc/asm_host.h).

The other ingest inputs of the suite (asm.generate_pairs, tests/util.random_ragged_batch written out line by line) put a newline
wherever it happens to fall, start every line with a marker and fill every chunk with about as many pairs as the one before.  The
builders below put newlines on the edges of the parser's 16-byte thread slices, 1,024-byte waves and 4,096-byte tiles, fill whole
tiles with newlines, end the text on those edges, put the lengths at which the gather kernel's 64-lane stride turns next to one
another, put bytes into the strings that are not bases, move the longest pair beyond the maximum kernel's first grid pass, and step
the pairs per byte up in the middle of a file.

Deterministic; nothing is read from disk and nothing needs a GPU.  A builder returns a Case: it unpacks as `(text, name)`, and
`.facts` holds what the builder promises, for the tests that prove it from the text (tests/test_seq_text_host.py).
"""
import functools

import numpy as np

SLICE, WAVE, TILE = 16, 1024, 4096  # bytes per thread, per wavefront and per workgroup of seq_count_kernel / seq_index_kernel
MAX_GRID_THREADS = 1024 * 256       # seq_max_kernel's launch: beyond that many pairs its grid-stride loop takes a second pass
LEAP_MAX, MAX_LENGTH = 256, 512
_ACGT = np.frombuffer(b"ACGT", np.uint8)


class Case(tuple):
    """(text, name) with the builder's facts beside it."""

    def __new__(cls, text, name, **facts):
        self = super().__new__(cls, (bytes(text), name))
        self.facts = facts
        return self

    text = property(lambda self: self[0])
    name = property(lambda self: self[1])


# ---- the reference parser ------------------------------------------------------------------------------------------------------
def _lines(text):
    """(bytes as uint8, start of every line, end of every line): line l is buf[start[l]:end[l]], split on byte 0x0a only; an
    unterminated last line counts."""
    buf = np.frombuffer(bytes(text), np.uint8)
    end = np.flatnonzero(buf == 0x0A).astype(np.int64)
    if buf.size and buf[-1] != 0x0A:
        end = np.append(end, buf.size)
    start = np.concatenate(([0], end[:-1] + 1)).astype(np.int64) if end.size else end
    return buf, start, end


def _gather(buf, first, length):
    off = np.zeros(length.size + 1, np.int64)
    off[1:] = np.cumsum(length)
    idx = np.repeat(first - off[:-1], length) + np.arange(off[-1], dtype=np.int64)
    return buf[idx].copy(), off.astype(np.uint32)


def parse(text):
    """`benchmark::read_string_file` (benchmark_utils.h:325-352) as this project implements it, byte for byte: the text is split on
    byte 0x0a only (CR, NUL and bytes >= 0x80 stay in the strings, as std::getline keeps them); an unterminated last line
    counts; line 2i is read i and line 2i + 1 reference i, each without its first byte, whatever that byte is; a read without a
    reference line (an odd line count) gets an empty reference.

    A line of zero bytes is an empty string: that is the project's rule (csrc/asm_ingest.h, seq_lengths_kernel:
    `a1 - a0 > 1 ? a1 - a0 - 1 : 0`), not the reference's, whose `line.substr(1)` throws std::out_of_range on an empty line.
    Everything else is the reference's behaviour.  -> HostBatch"""
    import approximate_string_matching_amd as asm

    buf, start, end = _lines(text)
    if start.size & 1:
        start, end = np.append(start, buf.size), np.append(end, buf.size)
    first = np.minimum(start + 1, end)
    length = end - first
    reads, read_off = _gather(buf, first[0::2], length[0::2])
    refs, ref_off = _gather(buf, first[1::2], length[1::2])
    return asm.HostBatch(reads, read_off, refs, ref_off)


def appended_newlines(text):
    """What asm_batch_from_text and PairsFill put behind the text: one newline for an open last line, one more for an odd line count."""
    text = bytes(text)
    open_line = bool(text) and not text.endswith(b"\n")
    lines = text.count(b"\n") + (1 if open_line else 0)
    return (1 if open_line else 0) + (lines & 1)


def shipped_bytes(text):
    """asm_stream_stats.bytes of the whole file: the text and the newlines appended to it."""
    return len(text) + appended_newlines(text)


def chunk_cuts(text, chunk, max_pairs=0):
    """The chunks asm_stream_seq_file ships (PairsFill, csrc/asm_host.h): chunk c holds what the chunk before left behind its last
    whole pair and `chunk` more file bytes, and is cut behind its last whole pair; the end of the file closes an open line and an
    odd line count; max_pairs > 0 ends the stream inside the chunk that reaches it.
    -> [(first byte, bytes, pairs, carried bytes)], chunks without a whole pair included (pairs = 0, never shipped)."""
    text = bytes(text)
    closed = text + b"\n" * appended_newlines(text)
    nl = np.flatnonzero(np.frombuffer(closed, np.uint8) == 0x0A)
    boundary = nl[1::2] + 1  # the byte behind pair j
    out, at, done, read = [], 0, 0, 0
    while True:
        carried = read - at
        read = min(len(text), read + chunk)
        eof = read >= len(text)
        have = len(closed) if eof else read
        upto = int(np.searchsorted(boundary, have, side="right"))
        if max_pairs > 0 and upto >= max_pairs:
            upto, eof = max_pairs, True
        stop = int(boundary[upto - 1]) if upto else 0
        stop = max(stop, at)
        out.append((at, stop - at, upto - done, carried))
        at, done = stop, upto
        if eof:
            return out


# ---- building blocks -----------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20240607, *key])


def _acgt(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def _related(rng, s, n):
    """n characters that go on from s: s with a substitution every 20 or so characters and, one time in three, one character
    dropped or doubled near the middle; cut to n, or lengthened by random characters."""
    b = bytearray(s)
    for p in np.flatnonzero(rng.random(len(b)) < 0.05):
        b[p] = int(_ACGT[rng.integers(0, 4)])
    if len(b) > 4 and rng.random() < 1 / 3:
        p = len(b) // 2
        if rng.random() < 0.5:
            del b[p]
        else:
            b.insert(p, b[p])
    b = b[:n]
    return bytes(b) + _acgt(rng, n - len(b))


def _content(rng, index, size, partner):
    """The bytes of line `index` without its newline, `size` of them: a marker and size - 1 characters, or nothing at all; the
    characters of a reference line go on from the read line before it."""
    if size == 0:
        return b"", b""
    string = _related(rng, partner, size - 1) if index & 1 else _acgt(rng, size - 1)
    return (b"<" if index & 1 else b">") + string, string


class _Text:
    """Lines in order; `pos` is where the next line starts."""

    def __init__(self, rng):
        self.rng, self.parts, self.pos, self.lines, self.last = rng, [], 0, 0, b""

    def line(self, size, newline=True):
        content, string = _content(self.rng, self.lines, size, self.last)
        self.last = string
        self.raw(content, newline)

    def raw(self, content, newline=True):
        self.parts.append(content + (b"\n" if newline else b""))
        self.pos += len(content) + (1 if newline else 0)
        self.lines += 1

    def bytes(self):
        return b"".join(self.parts)


# ---- the builders --------------------------------------------------------------------------------------------------------------
def default_targets():
    """Where newline_grid's newlines must be: both sides of every tile edge of five tiles, both sides of the wave edges inside
    tiles 0 and 2, and bytes 0 and 1, 15 and the next slice's 0, and 14 and 15 of slices in the middle of a wave."""
    t = set()
    for tile in range(1, 6):
        t.update((TILE * tile - 1, TILE * tile))
    for wave in (1, 2, 3, 9, 10, 11):
        t.update((WAVE * wave - 1, WAVE * wave))
    for s in (21, 83, 300, 517, 700, 1000):  # slices well inside a wave
        t.update((SLICE * s, SLICE * s + 1, SLICE * (s + 3) + 15, SLICE * (s + 4), SLICE * (s + 7) + 14, SLICE * (s + 7) + 15))
    return sorted(t)


def newline_grid(targets=None):
    """About five tiles of lines of 0 to 256 random characters whose lengths are chosen so that a newline sits on every byte of
    `targets` (default_targets()).  Two targets next to each other leave a line of zero bytes between them."""
    targets = default_targets() if targets is None else sorted(targets)
    rng = _rng(1)
    t = _Text(rng)
    for target in targets:
        while target - t.pos > LEAP_MAX + 1:
            t.line(int(rng.integers(0, LEAP_MAX + 2)))
        t.line(target - t.pos)
    for _ in range(4):
        t.line(int(rng.integers(40, 90)))
    return Case(t.bytes(), "newline_grid", targets=targets)


def dense(n_lines=13000):
    """Two runs of n_lines bare newlines (an even number; 13,000: every run covers at least two whole tiles of 4,096 newlines,
    wherever it starts) with a line of 300 characters in front of, between and behind them: slices that are all newlines, slices
    that hold none, and a read, a reference and a read without reference line of 300 characters next to empty strings."""
    assert n_lines % 2 == 0
    rng = _rng(2)
    t = _Text(rng)
    for run in range(3):
        t.line(301)
        if run < 2:
            t.raw(b"\n" * (n_lines - 1))  # n_lines lines of zero bytes
            t.lines += n_lines - 1
    return Case(t.bytes(), "dense", n_lines=n_lines, long=300)


def ends(total, open_line, odd):
    """A text of exactly `total` bytes of lines of 0 to 256 characters; open_line: the last line has no newline; odd: the number of
    lines is odd.  total on a slice or tile edge (or one byte short of it) puts the newlines that the library appends on the
    first bytes of the next slice or tile."""
    rng = _rng(3, total, int(open_line), int(odd))
    t = _Text(rng)
    while total - t.pos > 400:
        t.line(int(rng.integers(0, LEAP_MAX + 2)))
    more = 2 if (t.lines & 1) == (1 if odd else 0) else 3
    left = total - t.pos - (more - 1 if open_line else more)
    for q in range(more):
        t.line(left // more + (1 if q < left % more else 0), newline=not (open_line and q == more - 1))
    text = t.bytes()
    assert len(text) == total
    return Case(text, f"ends_{total}_{'open' if open_line else 'closed'}_{'odd' if odd else 'even'}", total=total, open_line=open_line,
                odd=odd)


ENDS_TOTALS = (TILE - 1, TILE, TILE + 1, 2 * TILE, SLICE * 1283 - 1, SLICE * 1283)
MIX = (-1, 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 511, 512)  # -1: a line of zero bytes; 0: a marker alone


def lengths_mix():
    """Every length of MIX as a read next to every length of MIX as a reference, 169 pairs, the reference going on from the read."""
    t = _Text(_rng(4))
    for a in MIX:
        for b in MIX:
            t.line(a + 1)
            t.line(b + 1)
    return Case(t.bytes(), "lengths_mix", lengths=MIX)


DIRTY_KINDS = ("plain", "nul", "high", "markers_inside", "lower", "mixed")


def _soil(rng, s, kind):
    b = bytearray(s)
    hit = np.flatnonzero(rng.random(len(b)) < 0.08)
    for p in hit:
        if kind == "nul":
            b[p] = 0
        elif kind == "high":
            b[p] = int(rng.integers(0x80, 0x100))
        elif kind == "markers_inside":
            b[p] = b"><"[int(rng.integers(0, 2))]
        elif kind == "mixed":
            b[p] = (0, int(rng.integers(0x80, 0x100)), ord(">"), ord("<"), ord("\t"), ord("n"))[int(rng.integers(0, 6))]
    if kind == "lower" or (kind == "mixed" and rng.random() < 0.3):
        b = bytearray(bytes(b).lower())
    return bytes(b)


def dirty():
    """A CRLF text, 240 pairs: every line ends in `\\r\\n`, so every string ends in `\\r`; the strings (0 to 255 characters in front
    of the `\\r`) hold, by turns, plain bases, NUL, bytes 0x80-0xff, `>` and `<`, lower case, and all of these; the markers of the
    "mixed" pairs are NUL and 0xff."""
    rng = _rng(5)
    t = _Text(rng)
    special = (0, 1, 62, 63, 64, 254, 255)
    for i in range(240):
        kind = DIRTY_KINDS[i % len(DIRTY_KINDS)]
        n = special[i // len(DIRTY_KINDS)] if i < len(special) * len(DIRTY_KINDS) else int(rng.integers(0, 256))
        a = _acgt(rng, n)
        b = _related(rng, a, max(0, min(255, n + int(rng.integers(-2, 3)))))
        marks = (b"\x00", b"\xff") if kind == "mixed" else (b">", b"<")
        t.raw(marks[0] + _soil(rng, a, kind) + b"\r")
        t.raw(marks[1] + _soil(rng, b, kind) + b"\r")
    return Case(t.bytes(), "dirty", pairs=240)


def far_max(n=300_000, at=280_000):
    """n pairs of two bare newlines, except pair `at`, whose strings have 300 characters: with at >= 262,144 only a thread of
    seq_max_kernel that is in its second grid pass sees the longest string."""
    rng = _rng(6)
    a = _acgt(rng, 300)
    long_pair = b">" + a + b"\n<" + _related(rng, a, 300) + b"\n"
    return Case(b"\n\n" * at + long_pair + b"\n\n" * (n - at - 1), "far_max", n=n, at=at, long=300)


def density_step(chunk=1 << 16):
    """200 pairs of 512 characters (three chunks of `chunk` bytes), then 60,000 pairs of 0 to 3 characters, then 50 pairs of 512
    again: the result staging that asm_stream_seq_file sizes from the first chunk's pairs per byte is too small for the chunks of
    the middle part.  facts: the chunks as the library cuts them, the first chunk's and the densest chunk's pairs and bytes."""
    rng = _rng(7)
    t = _Text(rng)
    for _ in range(2 * 200):
        t.line(513)
    for _ in range(2 * 60_000):
        t.line(int(rng.integers(0, 5)))  # 0: a line of zero bytes; 1: a marker alone; up to 3 characters
    for _ in range(2 * 50):
        t.line(513)
    text = t.bytes()
    cuts = chunk_cuts(text, chunk)
    densest = max(cuts, key=lambda c: c[2])
    return Case(text, "density_step", chunk=chunk, cuts=cuts, first_pairs=cuts[0][2], first_bytes=cuts[0][1], densest_pairs=densest[2],
                densest_bytes=densest[1], densest_index=cuts.index(densest))


FIXED_SHIFTS = (0, 1, 32, 63)
FIXED_PAIRS = 384  # 24 KiB: six 4,096-byte chunks exactly at shift 0, so the last chunk ends with the file


def fixed_width(shift):
    """384 pairs of 64 bytes, two lines of 32 (a marker, 30 characters, a newline), behind a first pair whose read line is
    (64 - shift) % 64 bytes longer: every 4,096-byte chunk then ends `shift` bytes behind a pair boundary and carries them into
    the next.  shift 0: nothing is carried; 32: every chunk ends between a read line and its reference line."""
    rng = _rng(8, shift)
    t = _Text(rng)
    t.line(31 + (64 - shift) % 64)
    t.line(31)
    for _ in range(2 * (FIXED_PAIRS - 1)):
        t.line(31)
    return Case(t.bytes(), f"fixed_width_{shift}", shift=shift, pairs=FIXED_PAIRS, chunk=TILE)


@functools.lru_cache(maxsize=None)
def corpus():
    """Every text, in a fixed order."""
    cases = [newline_grid(), dense()]
    cases += [ends(total, open_line, odd) for total in ENDS_TOTALS for open_line in (False, True) for odd in (False, True)]
    cases += [lengths_mix(), dirty(), far_max(), density_step()]
    cases += [fixed_width(shift) for shift in FIXED_SHIFTS]
    return tuple(cases)


NAMES = (("newline_grid", "dense")
         + tuple(f"ends_{t}_{o}_{p}" for t in ENDS_TOTALS for o in ("closed", "open") for p in ("even", "odd"))
         + ("lengths_mix", "dirty", "far_max", "density_step") + tuple(f"fixed_width_{s}" for s in FIXED_SHIFTS))
BEYOND_LEAP = {"lengths_mix", "density_step", "dense", "far_max"}  # the texts with a string above 256 characters


def case(name):
    return next(c for c in corpus() if c.name == name)


@functools.lru_cache(maxsize=None)
def parsed(name):
    """parse() of a corpus text, made once and shared: do not modify it."""
    return parse(case(name).text)


def packed(hb):
    """The batch as the pack kernel's planes hold it (tests/structured_cases.as_packed): what the oracle's NW and LEAP are given."""
    import approximate_string_matching_amd as asm

    from tests import structured_cases

    if not hasattr(hb, "kinds"):
        hb.kinds = hb.meta = None
    return structured_cases.as_packed(asm, hb)
