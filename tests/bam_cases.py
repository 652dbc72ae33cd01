"""A BAM reader for the tests of the file calls' BAM output (docs/design/mapper.md, "BAM output"), on gzip, zlib and struct only.
bgzf_blocks walks the BGZF blocks of a file, parse_bam the header and the records of the uncompressed stream, sam_line prints a
record as the line sam_format writes (integer tags as :i:), and every record's stored bin is checked against reg2bin of its POS and
CIGAR.  encode_record is the writer of the hand-made records the reader is tested on first (tests/test_bam_host.py)."""
import gzip
import struct
import zlib

PAYLOAD = 65280
BASES16 = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FIXED = bytes.fromhex("1f8b08040000000000ff060042430200")  # everything in front of BSIZE


def bgzf_bound(n, eof):
    """the bytes of n payload bytes in stored blocks of PAYLOAD: 31 per block, and the EOF block"""
    return n + 31 * ((n + PAYLOAD - 1) // PAYLOAD) + (28 if eof else 0)


def bgzf_blocks(data: bytes):
    """-> [dict(at, bsize, head (the 18 header bytes), deflate (what lies between header and CRC), payload, crc, isize)]; every
    block's header bytes, CRC and ISIZE are checked here"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 16] == FIXED, "block at %d: header %s" % (at, data[at:at + 16].hex())
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert at + bsize <= len(data), "block at %d runs past the file" % at
        deflate = data[at + 18:at + bsize - 8]
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        payload = zlib.decompress(deflate, wbits=-15)
        assert zlib.crc32(payload) == crc, "block at %d: CRC %08x, payload has %08x" % (at, crc, zlib.crc32(payload))
        assert len(payload) == isize
        out.append(dict(at=at, bsize=bsize, head=data[at:at + 18], deflate=deflate, payload=payload, crc=crc, isize=isize))
        at += bsize
    assert at == len(data)
    return out


def check_stored(blocks, eof=True, full=True):
    """the structure the library writes: stored blocks (01 LEN ~LEN, then the payload as it is), every payload full except the
    last one in front of the EOF block (full=False: a whole file, where the header's last block may be short too), and the EOF
    block's bytes; -> the data blocks"""
    body = blocks[:-1] if eof else blocks
    if eof:
        assert blocks and blocks[-1]["head"] + blocks[-1]["deflate"] + struct.pack("<II", 0, 0) == EOF_BLOCK
    for t, b in enumerate(body):
        n = len(b["payload"])
        assert 1 <= n <= PAYLOAD and b["bsize"] == n + 31
        assert b["deflate"] == b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + b["payload"]
        assert not full or n == PAYLOAD or t == len(body) - 1, "block %d of %d holds %d bytes" % (t, len(body), n)
    return body


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def parse_header(stream: bytes):
    """-> (text, [(name, length)], offset of the first record)"""
    assert stream[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, at)[0]
        name = stream[at + 4:at + 4 + l_name]
        assert name[-1:] == b"\0"
        refs.append((name[:-1].decode("latin-1"), struct.unpack_from("<i", stream, at + 4 + l_name)[0]))
        at += 8 + l_name
    return text, refs, at


def parse_record(rec: bytes):
    """the bytes behind block_size -> dict; the stored bin must be reg2bin of POS and the CIGAR"""
    ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_id, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
    at = 32
    name = rec[at:at + l_name]
    assert l_name >= 1 and name[-1:] == b"\0" and b"\0" not in name[:-1]
    at += l_name
    cigar = [(v >> 4, CIGAR_OPS[v & 15]) for v in struct.unpack_from("<%dI" % n_cigar, rec, at)]
    at += 4 * n_cigar
    packed = rec[at:at + (l_seq + 1) // 2]
    seq = "".join(BASES16[packed[t >> 1] >> 4 if t % 2 == 0 else packed[t >> 1] & 15] for t in range(l_seq))
    if l_seq % 2:
        assert packed[-1] & 15 == 0
    at += (l_seq + 1) // 2
    qual = rec[at:at + l_seq]
    assert len(qual) == l_seq
    at += l_seq
    tags = []
    while at < len(rec):
        tag, typ = rec[at:at + 2].decode("latin-1"), chr(rec[at + 2])
        at += 3
        if typ == "Z":
            end = rec.index(b"\0", at)
            tags.append((tag, "Z", rec[at:end].decode("latin-1")))
            at = end + 1
        else:
            fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ]
            tags.append((tag, typ, struct.unpack_from(fmt, rec, at)[0]))
            at += struct.calcsize(fmt)
    assert at == len(rec)
    ref_len = sum(n for n, op in cigar if op in "MDN=X")
    want_bin = reg2bin(pos, pos + ref_len if cigar else pos + 1)
    assert bin_ == want_bin, "bin %d, reg2bin gives %d (pos %d, cigar %s)" % (bin_, want_bin, pos, cigar)
    return dict(ref_id=ref_id, pos=pos, mapq=mapq, bin=bin_, flag=flag, next_id=next_id, next_pos=next_pos, tlen=tlen,
                name=name[:-1].decode("latin-1"), cigar=cigar, seq=seq, qual=qual, tags=tags)


def smallest_type(v):
    """htslib's type for an integer tag"""
    if v >= 0:
        return "C" if v <= 255 else "S" if v <= 65535 else "I"
    return "c" if v >= -128 else "s" if v >= -32768 else "i"


def sam_line(r, names):
    """the record as sam_format writes it; integer tags must be of the smallest type and print as :i:"""
    rname = "*" if r["ref_id"] < 0 else names[r["ref_id"]]
    rnext = "*" if r["next_id"] < 0 else "=" if r["next_id"] == r["ref_id"] else names[r["next_id"]]
    cigar = "".join("%d%s" % c for c in r["cigar"]) or "*"
    qual = "*" if not r["qual"] or r["qual"] == b"\xff" * len(r["qual"]) else bytes(q + 33 for q in r["qual"]).decode("latin-1")
    cols = [r["name"], str(r["flag"]), rname, str(r["pos"] + 1), str(r["mapq"]), cigar, rnext, str(r["next_pos"] + 1), str(r["tlen"]),
            r["seq"] or "*", qual]
    for tag, typ, v in r["tags"]:
        if typ == "Z":
            cols.append("%s:Z:%s" % (tag, v))
        else:
            assert typ == smallest_type(v), "%s:%s:%d is not the smallest type" % (tag, typ, v)
            cols.append("%s:i:%d" % (tag, v))
    return "\t".join(cols) + "\n"


def records_of(stream: bytes, at=0):
    """the records of stream[at:] -> [dict]"""
    out = []
    while at < len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        assert size >= 32 and at + 4 + size <= len(stream)
        out.append(parse_record(stream[at + 4:at + 4 + size]))
        at += 4 + size
    return out


def parse_bam(data: bytes, eof=True):
    """a whole file -> (header text, [(name, length)], [record dict], blocks); the container's structure is checked on the way"""
    blocks = bgzf_blocks(data)
    check_stored(blocks, eof, full=False)
    stream = b"".join(b["payload"] for b in blocks)
    assert gzip.decompress(data) == stream
    text, refs, at = parse_header(stream)
    return text, refs, records_of(stream, at), blocks


def decode(data: bytes) -> bytes:
    """a BAM file as the SAM file of the same call: the header text, then every record's line"""
    text, refs, recs, _ = parse_bam(data)
    names = [n for n, _ in refs]
    return text + "".join(sam_line(r, names) for r in recs).encode("latin-1")


# ---- the writer of the hand-made records ---------------------------------------------------------------------------------------------
def encode_record(ref_id, pos, mapq, flag, next_id, next_pos, tlen, name, cigar, seq, qual, tags, bin_=None):
    """one record with its block_size, written field by field from SAM spec 4.2; cigar: [(n, op)], qual: bytes of Phred values or
    None, tags: [(tag, type, value)]"""
    ref_len = sum(n for n, op in cigar if op in "MDN=X")
    if bin_ is None:
        bin_ = reg2bin(pos, pos + ref_len if cigar else pos + 1)
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, mapq, bin_, len(cigar), flag, len(seq), next_id, next_pos, tlen)
    body += name.encode("latin-1") + b"\0"
    body += b"".join(struct.pack("<I", n << 4 | CIGAR_OPS.index(op)) for n, op in cigar)
    codes = [BASES16.index(ch) for ch in seq] + [0]
    body += bytes(codes[t] << 4 | codes[t + 1] for t in range(0, len(seq), 2))
    body += qual if qual is not None else b"\xff" * len(seq)
    for tag, typ, v in tags:
        body += tag.encode("latin-1") + typ.encode("latin-1")
        body += v.encode("latin-1") + b"\0" if typ == "Z" else struct.pack(
            {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ], v)
    return struct.pack("<i", len(body)) + body


def encode_header(text: bytes, refs):
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode("latin-1") + b"\0" + struct.pack("<i", length)
    return out


def frame_stored(stream: bytes, eof=True):
    """stream in stored BGZF blocks, by zlib's CRC"""
    out = b""
    for at in range(0, len(stream), PAYLOAD):
        p = stream[at:at + PAYLOAD]
        out += FIXED + struct.pack("<H", len(p) + 30) + b"\x01" + struct.pack("<HH", len(p), len(p) ^ 0xffff) + p
        out += struct.pack("<II", zlib.crc32(p), len(p))
    return out + (EOF_BLOCK if eof else b"")


# name, sequences, and hand-made records with the SAM line each must print as
HAND_REFS = [("chrA", 5000), ("chrB", 70000)]
HAND_RECORDS = [
    (dict(ref_id=0, pos=99, mapq=60, flag=0, next_id=-1, next_pos=-1, tlen=0, name="r0", cigar=[(3, "M"), (1, "I"), (2, "M")],
          seq="ACGTNA", qual=bytes([0, 1, 40, 41, 2, 3]), tags=[("NM", "C", 1), ("XG", "c", -4), ("MD", "Z", "5")]),
     "r0\t0\tchrA\t100\t60\t3M1I2M\t*\t0\t0\tACGTNA\t!\"IJ#$\tNM:i:1\tXG:i:-4\tMD:Z:5\n"),
    (dict(ref_id=-1, pos=-1, mapq=0, flag=4, next_id=-1, next_pos=-1, tlen=0, name="un", cigar=[], seq="ACG", qual=None, tags=[]),
     "un\t4\t*\t0\t0\t*\t*\t0\t0\tACG\t*\n"),
    (dict(ref_id=1, pos=16383, mapq=254, flag=163, next_id=1, next_pos=16500, tlen=217, name="p", cigar=[(2, "="), (1, "X"), (1, "D"), (2, "M")],
          seq="", qual=b"", tags=[("XP", "S", 256), ("XH", "I", 65536), ("XG", "s", -129), ("XQ", "i", -32769)]),
     "p\t163\tchrB\t16384\t254\t2=1X1D2M\t=\t16501\t217\t*\t*\tXP:i:256\tXH:i:65536\tXG:i:-129\tXQ:i:-32769\n"),
    (dict(ref_id=0, pos=10, mapq=3, flag=97, next_id=1, next_pos=0, tlen=-5, name="q", cigar=[(1, "M")], seq="=RYKMSWBDHVN",
          qual=bytes(range(12)), tags=[]),
     "q\t97\tchrA\t11\t3\t1M\tchrB\t1\t-5\t=RYKMSWBDHVN\t!\"#$%&'()*+,\n"),
]
