"""Paired FASTQ texts and the ways they are cut into BGZF members, for the tests of the compressed paired file call
(docs/design/mapper.md, "Compressed input for pairs"): tests/test_bgzf_pair_fill_host.py and tests/test_gpu_map_pairs_file_gz.py.
Containers are built with tests/bgzf_in_cases.py's helpers, so zlib is the encoder unless a test says otherwise."""
import itertools
import random

from tests import bgzf_in_cases as bi

BGZIP = (65280,)            # what bgzip writes
SMALL = (1, 7, 4099)        # members of these text sizes in rotation


def container(text, sizes=BGZIP, eof=True, empties=0, level=6):
    """text in members of `sizes` text bytes in rotation; empties: every that many members an empty member and an EOF block stand in
    the middle"""
    out, at, k = [], 0, 0
    for size in itertools.cycle(sizes):
        if at >= len(text):
            break
        part = text[at:at + size]
        out.append(bi.good_member(bi.deflate(part, level=level), part))
        at += size
        k += 1
        if empties and k % empties == 0:
            out.append(bi.good_member(bi.deflate(b"", level=0), b"") + bi.EOF_BLOCK)
    return b"".join(out) + (bi.EOF_BLOCK if eof else b"")


def mates(n, len1=36, len2=150, seed=5, crlf=(False, False), names=None, long_every=0, long_len=6000):
    """n pairs of random bases -> (text of file 1, text of file 2); long_every: every that many pairs mate 2 has long_len bases, a
    record of three chunks of 4 096 bytes (and a read longer than the mapper takes: the pair comes out unmapped)"""
    rng = random.Random(seed)
    out = ([], [])
    for k in range(n):
        for x, ln in enumerate((len1, long_len if long_every and k % long_every == long_every - 1 else len2)):
            nl = "\r\n" if crlf[x] else "\n"
            name = names(k, x) if names else "p%d/%d" % (k, x + 1)
            out[x].append("@%s%s%s%s+%s%s%s" % (name, nl, "".join(rng.choice("ACGT") for _ in range(ln)), nl, nl, "I" * ln, nl))
    return "".join(out[0]).encode(), "".join(out[1]).encode()


def records(text):
    """the whole records of a FASTQ text (a last line without its newline counts as a line) -> (records, lines behind the last one)"""
    lines = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    return lines // 4, lines % 4


def whole_records(text, n):
    """the first n records of a text whose last line may lack its newline, with that newline"""
    closed = text if not text or text.endswith(b"\n") else text + b"\n"
    at = 0
    for _ in range(4 * n):
        at = closed.index(b"\n", at) + 1
    return closed[:at]
