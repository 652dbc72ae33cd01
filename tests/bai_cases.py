"""The BAM index of the tests (docs/design/mapper.md, "BAM index"), on tests/bam_cases.py, struct and zlib only: build() writes the
canonical form from a block walk and the parsed records, parse() reads an index and checks its structure, query() is the SAM
specification's query algorithm (section 5.3: reg2bins, the candidate chunks, the linear index's lower bound, seeking by virtual
offset, filtering by overlap) and scan() the full scan it must agree with."""
import bisect
import struct

from tests import bam_cases as bc

PSEUDO_BIN = 37450
MAGIC = b"BAI\x01"


_LAYOUTS = {}


def layout(data: bytes):
    """a BAM file -> (blocks, stream, refs, [(offset in the stream, size with block_size, record dict)]); the last few files' are
    kept, since build, parse and Reader walk the same file"""
    if data not in _LAYOUTS:
        if len(_LAYOUTS) >= 4:
            _LAYOUTS.pop(next(iter(_LAYOUTS)))
        _LAYOUTS[data] = _layout(data)
    return _LAYOUTS[data]


def _layout(data: bytes):
    blocks = bc.bgzf_blocks(data)
    stream = b"".join(b["payload"] for b in blocks)
    _, refs, at = bc.parse_header(stream)
    recs = []
    while at < len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        assert size >= 32 and at + 4 + size <= len(stream)
        recs.append((at, 4 + size, bc.parse_record(stream[at + 4:at + 4 + size])))
        at += 4 + size
    return blocks, stream, refs, recs


class Voffsets:
    """the virtual offset of a stream offset: the block that holds the byte; behind the last byte the first of the empty blocks at
    the file's end (the EOF block), or the file's end when there is none"""

    def __init__(self, blocks, file_bytes):
        self.blocks, self.file_bytes = blocks, file_bytes
        self.ends, total = [], 0
        for b in blocks:
            total += len(b["payload"])
            self.ends.append(total)
        self.total = total
        self.by_at = {b["at"]: k for k, b in enumerate(blocks)}

    def __call__(self, at):
        k = bisect.bisect_right(self.ends, at)           # the first block whose end lies behind at
        if k < len(self.blocks):
            start = self.ends[k] - len(self.blocks[k]["payload"])
            return self.blocks[k]["at"] << 16 | (at - start)
        assert at == self.total
        e = len(self.blocks)
        while e > 0 and not self.blocks[e - 1]["payload"]:
            e -= 1
        return (self.blocks[e]["at"] if e < len(self.blocks) else self.file_bytes) << 16

    def stream_offset(self, v):
        """back: the stream offset a virtual offset points at (the block must start there)"""
        if v >> 16 == self.file_bytes:
            assert v & 0xffff == 0
            return self.total
        k = self.by_at[v >> 16]
        assert v & 0xffff < max(len(self.blocks[k]["payload"]), 1)
        return self.ends[k] - len(self.blocks[k]["payload"]) + (v & 0xffff)


def span(r):
    """[beg, end) of a placed record"""
    ref_len = sum(n for n, op in r["cigar"] if op in "MDN=X")
    return r["pos"], r["pos"] + (ref_len or 1)


def build(data: bytes) -> bytes:
    """the canonical index of a coordinate-sorted BAM file"""
    blocks, stream, refs, recs = layout(data)
    voff = Voffsets(blocks, len(data))
    out = MAGIC + struct.pack("<i", len(refs))
    per_ref = [[] for _ in refs]
    no_coor = 0
    for at, size, r in recs:
        if r["ref_id"] < 0:
            no_coor += 1
        else:
            per_ref[r["ref_id"]].append((voff(at), voff(at + size), r))
    keys = [(len(refs) if r["ref_id"] < 0 else r["ref_id"], r["pos"] if r["ref_id"] >= 0 else 0) for _, _, r in recs]
    assert keys == sorted(keys), "the file is not coordinate-sorted"
    for own in per_ref:
        if not own:
            out += struct.pack("<ii", 0, 0)
            continue
        bins, last_bin = {}, None
        windows = {}
        max_end = 0
        for v, v_end, r in own:
            beg, end = span(r)
            b = bc.reg2bin(beg, end)
            assert b == r["bin"]
            if b == last_bin:
                bins[b][-1][1] = v_end                     # the run goes on
            else:
                bins.setdefault(b, []).append([v, v_end])
            last_bin = b
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                windows[w] = min(windows.get(w, v), v)
            max_end = max(max_end, end)
        out += struct.pack("<i", len(bins) + 1)
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b])
        mapped = sum(1 for _, _, r in own if not r["flag"] & 4)
        out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, own[0][0], own[-1][1], mapped, len(own) - mapped)
        n_intv = ((max_end - 1) >> 14) + 1
        lin, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            nxt = windows.get(w, nxt)
            lin[w] = nxt
        out += struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *lin)
    return out + struct.pack("<Q", no_coor)


def parse(bai: bytes, data: bytes = None):
    """-> dict(refs=[dict(bins={bin: [(beg, end)]}, pseudo=(v_first, v_end, n_mapped, n_unmapped) or None, ioffset=[...])],
    no_coor, bins, chunks, intervals); the structure is checked, and with the BAM file every virtual offset must point at a record's
    start or at the end of the stream"""
    assert bai[:4] == MAGIC
    n_ref = struct.unpack_from("<i", bai, 4)[0]
    at = 8
    starts = None
    if data is not None:
        blocks, stream, _, recs = layout(data)
        voff = Voffsets(blocks, len(data))
        starts = {voff(a) for a, _, _ in recs} | {voff(len(stream))}
    refs, n_bins, n_chunks, n_intervals = [], 0, 0, 0
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, at)[0]
        at += 4
        bins, pseudo, order = {}, None, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", bai, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
            order.append(b)
            if b == PSEUDO_BIN:
                assert n_chunk == 2
                pseudo = chunks[0] + chunks[1]
                assert pseudo[0] < pseudo[1]
                continue
            assert b < PSEUDO_BIN and n_chunk >= 1 and b not in bins
            for c, (beg, end) in enumerate(chunks):
                assert beg < end, "chunk %d of bin %d is empty" % (c, b)
                assert c == 0 or chunks[c - 1][1] <= beg, "the chunks of bin %d overlap or descend" % b
            bins[b] = chunks
            n_bins += 1
            n_chunks += n_chunk
        assert order == sorted(order) and (not order or order[-1] == PSEUDO_BIN), "bins ascend, 37450 last"
        n_intv = struct.unpack_from("<i", bai, at)[0]
        ioffset = list(struct.unpack_from("<%dQ" % n_intv, bai, at + 4))
        at += 4 + 8 * n_intv
        assert ioffset == sorted(ioffset)
        assert (n_bin == 0) == (n_intv == 0)
        n_intervals += n_intv
        if starts is not None:
            for v in [x for ch in bins.values() for c in ch for x in c] + list(pseudo[:2] if pseudo else ()) + ioffset:
                assert v in starts, "virtual offset %x points at no record" % v
        refs.append(dict(bins=bins, pseudo=pseudo, ioffset=ioffset))
    no_coor = struct.unpack_from("<Q", bai, at)[0]
    assert at + 8 == len(bai)
    return dict(refs=refs, no_coor=no_coor, bins=n_bins, chunks=n_chunks, intervals=n_intervals)


def reg2bins(beg, end):
    """SAM spec 5.3"""
    end -= 1
    out = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class Reader:
    """a BAM file ready for queries: the records by stream offset"""

    def __init__(self, data: bytes):
        self.blocks, self.stream, self.refs, self.recs = layout(data)
        self.voff = Voffsets(self.blocks, len(data))
        self.at = [a for a, _, _ in self.recs]
        # for scan(): per sequence the records in file order, which is ascending beg, and the longest span among them
        self.by_tid = {}
        for k, (_, _, r) in enumerate(self.recs):
            if r["ref_id"] >= 0:
                begs, rows, longest = self.by_tid.setdefault(r["ref_id"], ([], [], [0]))
                beg, end = span(r)
                begs.append(beg), rows.append((beg, end, k))
                longest[0] = max(longest[0], end - beg)

    def from_to(self, v_beg, v_end):
        """the records whose first byte lies in [v_beg, v_end)"""
        lo = bisect.bisect_left(self.at, self.voff.stream_offset(v_beg))
        hi = bisect.bisect_left(self.at, self.voff.stream_offset(v_end))
        return range(lo, hi)


def query(index, reader: Reader, tid, beg, end):
    """the indices of the records the spec's algorithm finds for [beg, end) of tid; index: parse()'s"""
    ref = index["refs"][tid]
    w = beg >> 14
    if w >= len(ref["ioffset"]):
        return []                                          # n_intv says that no record reaches the window
    min_off = ref["ioffset"][w]                            # no record that overlaps the window starts in front of it
    found = set()
    for b in reg2bins(beg, end):
        for c_beg, c_end in ref["bins"].get(b, ()):
            if c_end <= min_off:
                continue
            for k in reader.from_to(max(c_beg, min_off), c_end):
                r = reader.recs[k][2]
                r_beg, r_end = span(r)
                if r["ref_id"] == tid and r_beg < end and r_end > beg:
                    found.add(k)
    return sorted(found)


def scan(reader: Reader, tid, beg, end):
    """the full scan: every record of tid that overlaps [beg, end); a record that starts at or below beg - (the longest span) cannot
    reach beg, and one that starts at or behind end does not overlap, so only the records between them are looked at"""
    if tid not in reader.by_tid:
        return []
    begs, rows, longest = reader.by_tid[tid]
    lo, hi = bisect.bisect_right(begs, beg - longest[0]), bisect.bisect_left(begs, end)
    return [k for r_beg, r_end, k in rows[lo:hi] if r_beg < end and r_end > beg]


def idxstats(index):
    """(n_mapped, n_unmapped) per reference from the pseudo-bins, and n_no_coor"""
    return [tuple(r["pseudo"][2:]) if r["pseudo"] else (0, 0) for r in index["refs"]], index["no_coor"]
