"""The payload corpus of the deflate container's tests (docs/design/mapper.md, "Deflate"), shared by tests/test_deflate_host.py and
tests/test_gpu_deflate.py, and what both check on a container: every block inflates to its payload with the right CRC and ISIZE
(bam_cases.bgzf_blocks), none is longer than its stored form, and the cut is the one of the stored container."""
import gzip
import random
import struct

from tests import bam_cases as bc

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
