"""The corpus of the BGZF decoder's tests (docs/design/mapper.md, "Compressed input"): containers that must decode to zlib's bytes and
containers that must be refused, built with zlib and struct alone.  zlib.decompress(raw, wbits=-15) per member is the reference; every
good member is checked against it where it is built.  Every size is the smallest that reaches its edge."""
import functools
import random
import struct
import zlib

# the status classes of csrc/asm_inflate.h
(OK, E_EOF, E_BTYPE, E_STORED, E_HEADER, E_CODELEN, E_REPEAT, E_LITLEN, E_DISTCODE, E_SYMBOL, E_DIST, E_OVERRUN, E_ISIZE, E_CRC, E_SLACK,
 E_TABLE) = range(16)
IN_OK, IN_MAGIC, IN_NO_BC, IN_BSIZE, IN_PAST_END, IN_ISIZE = range(6)

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
PAYLOADS = (0, 1, 2, 3, 63, 64, 65, 258, 259, 65279, 65280, 65536)
PERIODS = (1, 2, 3, 63, 64, 65, 257, 258, 259)


# ---- the container -----------------------------------------------------------------------------------------------------------------
def member(raw, payload, before=b"", after=b"", crc=None, isize=None, bsize=None):
    """one BGZF member around a raw deflate stream; `before` / `after`: whole extra subfields around BC"""
    extra = before + b"BC" + struct.pack("<H", 2) + b"\0\0" + after
    size = 12 + len(extra) + len(raw) + 8
    assert bsize is not None or size <= 65536, size
    extra = before + b"BC" + struct.pack("<HH", 2, (size - 1 if bsize is None else bsize) & 0xffff) + after
    head = bytes.fromhex("1f8b08040000000000ff") + struct.pack("<H", len(extra)) + extra
    return head + raw + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush=zlib.Z_SYNC_FLUSH):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return z.compress(data) + z.flush()
    out = b""
    for at in range(0, len(data), flush_every):
        out += z.compress(data[at:at + flush_every]) + z.flush(flush)
    return out + z.flush()


def good_member(raw, payload, **kw):
    assert zlib.decompress(raw, wbits=-15) == payload
    return member(raw, payload, **kw)


def split_members(data):
    """[(offset, member bytes)] by BSIZE, for containers whose BC subfield comes first"""
    out, at = [], 0
    while at < len(data):
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        extra, k, size = data[at + 12:at + 12 + xlen], 0, None
        while k + 4 <= len(extra):
            slen = struct.unpack_from("<H", extra, k + 2)[0]
            if extra[k:k + 2] == b"BC" and slen == 2 and size is None:
                size = struct.unpack_from("<H", extra, k + 4)[0] + 1
            k += 4 + slen
        out.append((at, data[at:at + size]))
        at += size
    return out


def reference(data):
    """zlib's bytes of a sound container"""
    out = b""
    for _, m in split_members(data):
        xlen = struct.unpack_from("<H", m, 10)[0]
        out += zlib.decompress(m[12 + xlen:-8], wbits=-15)
    return out


# ---- text sources ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fastq_text(n=200_000, seed=7):
    rng, out, k = random.Random(seed), [], 0
    while sum(map(len, out)) < n:
        ln = rng.randint(30, 150)
        out.append("@read%d/%d\n%s\n+\n%s\n" % (k, ln, "".join(rng.choice("ACGT") for _ in range(ln)),
                                                 "".join(chr(33 + min(40, int(rng.expovariate(0.08)))) for _ in range(ln))))
        k += 1
    return "".join(out).encode()[:n]


def source(kind, n):
    if kind == "fastq":
        return (fastq_text() * (n // len(fastq_text()) + 1))[:n]
    if kind == "bytes":
        return (bytes(range(256)) * (n // 256 + 1))[:n]
    if kind == "run":
        return b"G" * n
    if kind == "random":
        return random.Random(n + 11).randbytes(n)
    if kind.startswith("period"):
        p = int(kind[6:])
        return (random.Random(p).randbytes(p) * (n // p + 1))[:n]
    raise KeyError(kind)


ENCODERS = {
    "level0": dict(level=0), "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9),
    "fixed": dict(strategy=zlib.Z_FIXED), "huffman": dict(strategy=zlib.Z_HUFFMAN_ONLY), "rle": dict(strategy=zlib.Z_RLE),
    "sync": dict(flush_every=97, flush=zlib.Z_SYNC_FLUSH), "full": dict(level=9, flush_every=1021, flush=zlib.Z_FULL_FLUSH),
}


# ---- hand-assembled streams --------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):            # as the header's fields and the extra bits go: lowest bit first
        self.acc |= value << self.n
        self.n += nbits

    def code(self, code, nbits):            # a Huffman code: its first bit first
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def raw(self, data):
        self.align()
        self.acc |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """{symbol: (code, length)} of the canonical code, over-subscribed and incomplete ones included (as far as codes exist)"""
    code, out = 0, {}
    for ln in range(1, 16):
        for sym, v in enumerate(lens):
            if v == ln:
                out[sym] = (code, ln)
                code += 1
        code <<= 1
    return out


LEN_BASE = [(3 + i, 0) for i in range(8)] + [(11 + 2 * i, 1) for i in range(4)] + [(19 + 4 * i, 2) for i in range(4)] + \
    [(35 + 8 * i, 3) for i in range(4)] + [(67 + 16 * i, 4) for i in range(4)] + [(131 + 32 * i, 5) for i in range(4)] + [(258, 0)]
DIST_BASE = [(1, 0), (2, 0), (3, 0), (4, 0)] + [((2 + (d & 1) << (d // 2 - 1)) + 1, d // 2 - 1) for d in range(4, 30)]


def length_symbol(n):
    if n == 258:
        return 285, 0, 0
    sym = max(i for i, (base, _) in enumerate(LEN_BASE[:28]) if base <= n)
    return 257 + sym, n - LEN_BASE[sym][0], LEN_BASE[sym][1]


def distance_symbol(d):
    sym = max(i for i, (base, _) in enumerate(DIST_BASE) if base <= d)
    return sym, d - DIST_BASE[sym][0], DIST_BASE[sym][1]


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def put_tokens(b, tokens, ll_lens, d_lens):
    """tokens: an int is a literal, (length, distance) a match, ("ll", symbol) / ("d", symbol) a bare code; then the end-of-block code"""
    ll, d = canonical(ll_lens), canonical(d_lens)
    for t in list(tokens) + [("ll", 256)]:
        if isinstance(t, int):
            b.code(*ll[t])
        elif t[0] == "ll":
            b.code(*ll[t[1]])
        elif t[0] == "d":
            b.code(*d[t[1]])
        else:
            sym, extra, nbits = length_symbol(t[0])
            b.code(*ll[sym])
            b.put(extra, nbits)
            sym, extra, nbits = distance_symbol(t[1])
            b.code(*d[sym])
            b.put(extra, nbits)


def fixed_block(b, tokens, final=True):
    b.put(int(final), 1)
    b.put(1, 2)
    put_tokens(b, tokens, FIXED_LL, FIXED_D)


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def dynamic_header(b, ll_lens, d_lens, final=True, cl_lens=None, cl_symbols=None, hlit=None, hdist=None):
    """The header of a dynamic block.  By default the code-length code gives 4 bits to each of the lengths 0 to 15 and uses no repeat
    symbol; cl_lens / cl_symbols replace the code and the symbols sent (an int, or (16 | 17 | 18, repeat field))."""
    b.put(int(final), 1)
    b.put(2, 2)
    b.put((len(ll_lens) if hlit is None else hlit) - 257, 5)
    b.put((len(d_lens) if hdist is None else hdist) - 1, 5)
    cl_lens = [4] * 16 + [0] * 3 if cl_lens is None else cl_lens
    b.put(19 - 4, 4)
    for sym in CL_ORDER:
        b.put(cl_lens[sym], 3)
    cl = canonical(cl_lens)
    for s in (list(ll_lens) + list(d_lens) if cl_symbols is None else cl_symbols):
        if isinstance(s, int):
            b.code(*cl[s])
        else:
            b.code(*cl[s[0]])
            b.put(s[1], {16: 2, 17: 3, 18: 7}[s[0]])


def dynamic_block(b, tokens, ll_lens, d_lens, final=True, **kw):
    dynamic_header(b, ll_lens, d_lens, final, **kw)
    put_tokens(b, tokens, ll_lens, d_lens)


def ll_lens_of(codes, n=257):
    """literal/length code lengths from {symbol: length}"""
    n = max(n, max(codes) + 1)
    return [codes.get(s, 0) for s in range(n)]


def hand_assembled():
    """{name: (raw deflate, payload)}: streams no encoder writes"""
    out = {}
    b = Bits()
    fixed_block(b, [ord("a"), (258, 1)])
    out["literal then 258 at distance 1"] = (b.bytes(), b"a" * 259)
    far = random.Random(32768).randbytes(32768)
    b = Bits()
    b.put(0, 1), b.put(0, 2)
    b.raw(struct.pack("<HH", 32768, 32768 ^ 0xffff) + far)
    fixed_block(b, [(100, 32768), (3, 32768), (258, 32768)])
    out["distance 32768"] = (b.bytes(), far + far[:100] + far[100:103] + far[103:361])
    b = Bits()
    dynamic_block(b, [97, 97, 97, (3, 1)], ll_lens_of({97: 1, 256: 2, 257: 2}), [1])
    out["distance code of one symbol"] = (b.bytes(), b"a" * 6)
    b = Bits()
    dynamic_block(b, [97, 98, 97], ll_lens_of({97: 1, 98: 2, 256: 2}), [0])
    out["distance code of no symbol"] = (b.bytes(), b"aba")
    # overlapping copies around the wave's width, in one batch with their sources
    b = Bits()
    fixed_block(b, [120, 121, 122] + [(n, d) for d in (1, 2, 3) for n in (3, 63, 64, 65, 129, 258)])
    raw = b.bytes()
    out["overlapping copies"] = (raw, zlib.decompress(raw, wbits=-15))
    # more than one batch of 64 tokens, a match of the second reaching into the first, and 15-bit codes with subtables
    b = Bits()
    lens = ll_lens_of({**{s: 15 for s in range(0, 64)}, **{s: 14 for s in range(64, 96)}, 256: 15, 257: 15})
    lens, k = list(lens), 96
    kraft = sum(1 << (15 - v) for v in lens if v)
    for ln in range(1, 15):                     # complete the code with shorter ones
        while kraft + (1 << (15 - ln)) <= 1 << 15 and k < 256:
            lens[k], kraft, k = ln, kraft + (1 << (15 - ln)), k + 1
    assert kraft == 1 << 15, kraft
    toks = list(range(0, 96)) + list(range(96, k)) + [(3, 70), (3, 1)] + list(range(0, 64))
    dynamic_block(b, toks, lens, [1] + [0] * 11 + [1])      # distances 1 and 65 to 96
    raw = b.bytes()
    out["15-bit codes over two batches"] = (raw, zlib.decompress(raw, wbits=-15))
    return out


# ---- the good corpus ---------------------------------------------------------------------------------------------------------------
def fits(raw):
    return len(raw) + 26 <= 65536


@functools.lru_cache(maxsize=None)
def good():
    """{name: container}: one or a few members each, with or without the EOF block; reference() gives the expected bytes"""
    out = {}
    for enc, kw in ENCODERS.items():
        for n in PAYLOADS:
            for kind in ("fastq", "random"):
                src = source(kind, n)
                raw = deflate(src, **kw)
                if fits(raw) and not (kind == "random" and 3 < n < 65279 and enc not in ("level6", "level0")):
                    out["%s %s %d" % (enc, kind, n)] = good_member(raw, src) + EOF_BLOCK
    for kind in ["bytes", "run"] + ["period%d" % p for p in PERIODS]:
        for enc in ("level1", "level9", "rle", "fixed"):
            src = source(kind, 3000 if kind != "run" else 65536)
            out["%s %s" % (enc, kind)] = good_member(deflate(src, **ENCODERS[enc]), src) + EOF_BLOCK
    for name, (raw, payload) in hand_assembled().items():
        out[name] = good_member(raw, payload) + EOF_BLOCK
    text = fastq_text()
    parts = [text[a:a + 65280] for a in range(0, len(text), 65280)]
    out["fastq in bgzip members"] = b"".join(good_member(deflate(p), p) for p in parts) + EOF_BLOCK
    out["no EOF block"] = b"".join(good_member(deflate(p), p) for p in parts[:2])
    out["empty members"] = EOF_BLOCK + good_member(deflate(parts[0]), parts[0]) + EOF_BLOCK + EOF_BLOCK + good_member(deflate(parts[1]), parts[1]) + \
        good_member(deflate(b"", level=0), b"") + EOF_BLOCK
    out["only the EOF block"] = EOF_BLOCK
    out["nothing"] = b""
    small = text[:700]
    out["extra subfields"] = good_member(deflate(small), small, before=b"AB" + struct.pack("<H", 3) + b"xyz",
                                         after=b"ZZ" + struct.pack("<H", 0) + b"BC" + struct.pack("<H", 2) + b"\x01\x02") + EOF_BLOCK
    out["a BC subfield of another size first"] = good_member(deflate(small), small, before=b"BC" + struct.pack("<H", 1) + b"q") + EOF_BLOCK
    return out


def own_encoder(asm):
    """{name: container} written by this project's encoder: deflate and stored"""
    out = {}
    for kind, n in (("fastq", 0), ("fastq", 1), ("fastq", 65280), ("fastq", 2 * 65280 + 1), ("random", 65281), ("period3", 5000), ("run", 70000)):
        for level in (asm.BGZF_DEFLATE, asm.BGZF_STORED):
            out["own level %d %s %d" % (level, kind, n)] = asm.bgzf_compress_host(source(kind, n), eof=True, level=level)
    return out


def as_one(containers):
    """the containers as one, their EOF blocks kept as empty members -> container"""
    return b"".join(containers)


# ---- the corrupt corpus ------------------------------------------------------------------------------------------------------------
def _raw(build):
    b = Bits()
    build(b)
    return b.bytes()


@functools.lru_cache(maxsize=None)
def corrupt():
    """{name: (container, "member" | "container", index of the bad member, class)}.  A sound member stands in front of every bad one,
    so that the index reported is not 0 by default."""
    text = fastq_text()[:900]
    sound = good_member(deflate(text), text)
    raw = deflate(text)
    out = {}

    def bad(name, rawbytes, payload=text, cls=None, **kw):
        out[name] = (sound + member(rawbytes, payload, **kw) + EOF_BLOCK, "member", 1, cls)

    bad("stream cut short", raw[:-2], cls=E_EOF)
    bad("block type 3", _raw(lambda b: (b.put(1, 1), b.put(3, 2))), b"", cls=E_BTYPE)
    bad("stored LEN is not ~NLEN", b"\x01\x05\x00\x00\x00hello", b"hello", cls=E_STORED)
    bad("HLIT 288", _raw(lambda b: (b.put(1, 1), b.put(2, 2), b.put(31, 5), b.put(0, 5), b.put(0, 4), b.put(0, 64))), b"", cls=E_HEADER)
    bad("HDIST 31", _raw(lambda b: (b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(30, 5), b.put(0, 4), b.put(0, 64))), b"", cls=E_HEADER)
    ll = ll_lens_of({97: 1, 256: 2, 257: 2})
    bad("code-length code over-subscribed", _raw(lambda b: (dynamic_header(b, ll, [1], cl_lens=[1] * 19), b.put(0, 64))), b"", cls=E_CODELEN)
    bad("code-length code incomplete", _raw(lambda b: (dynamic_header(b, [], [], cl_lens=[1] + [0] * 18, cl_symbols=[0] * 258, hlit=257, hdist=1),
                                                      b.put(0, 64))), b"", cls=E_CODELEN)
    rep = [4] * 15 + [0] + [4, 0, 0]    # the lengths 0 to 14 and symbol 16 at 4 bits each
    bad("repeat with no previous length", _raw(lambda b: (dynamic_header(b, [], [], cl_lens=rep, cl_symbols=[(16, 0)] + [0] * 255, hlit=257, hdist=1),
                                                         b.put(0, 64))), b"", cls=E_REPEAT)
    bad("repeat past the last length", _raw(lambda b: (dynamic_header(b, [], [], cl_lens=rep, cl_symbols=[1] * 256 + [(16, 3)], hlit=257, hdist=1),
                                                      b.put(0, 64))), b"", cls=E_REPEAT)
    bad("literal/length code over-subscribed", _raw(lambda b: (dynamic_header(b, ll_lens_of({97: 1, 98: 1, 256: 1}), [1]), b.put(0, 64))), b"",
        cls=E_LITLEN)
    bad("literal/length code incomplete", _raw(lambda b: (dynamic_header(b, ll_lens_of({97: 2, 256: 2}), [1]), b.put(0, 64))), b"", cls=E_LITLEN)
    bad("no end-of-block code", _raw(lambda b: (dynamic_header(b, ll_lens_of({97: 1, 98: 1}), [1]), b.put(0, 64))), b"", cls=E_LITLEN)
    bad("literal/length code of one symbol", _raw(lambda b: dynamic_block(b, [], ll_lens_of({256: 1}), [0])), b"", cls=E_LITLEN)
    bad("distance code over-subscribed", _raw(lambda b: (dynamic_header(b, ll, [1, 1, 1]), b.put(0, 64))), b"", cls=E_DISTCODE)
    bad("distance code of two symbols incomplete", _raw(lambda b: (dynamic_header(b, ll, [2, 2]), b.put(0, 64))), b"", cls=E_DISTCODE)
    bad("distance code of one symbol of two bits", _raw(lambda b: (dynamic_header(b, ll, [2]), b.put(0, 64))), b"", cls=E_DISTCODE)
    bad("length symbol 286", _raw(lambda b: fixed_block(b, [97, ("ll", 286)])), b"a", cls=E_SYMBOL)
    bad("distance symbol 30", _raw(lambda b: fixed_block(b, [97, ("ll", 257), ("d", 30)])), b"a", cls=E_SYMBOL)

    def unused(b):
        dynamic_header(b, ll, [1])
        b.code(*canonical(ll)[97]), b.code(*canonical(ll)[257]), b.put(1, 1), b.put(0, 64)
    bad("the unused code of a one-symbol distance code", _raw(unused), b"a", cls=E_SYMBOL)
    bad("a distance in a block with no distance code",
        _raw(lambda b: (dynamic_header(b, ll, [0]), b.code(*canonical(ll)[97]), b.code(*canonical(ll)[257]), b.put(0, 64))), b"a", cls=E_SYMBOL)
    bad("first token a match at distance 1", _raw(lambda b: fixed_block(b, [(258, 1)])), b"a" * 258, cls=E_DIST)
    bad("distance one past the output", _raw(lambda b: fixed_block(b, [97, 98, (3, 3)])), b"ab" + b"aba", cls=E_DIST)
    bad("ISIZE one short", raw, isize=len(text) - 1, cls=E_OVERRUN)
    bad("ISIZE one short, ending in a match", _raw(lambda b: fixed_block(b, [97, (258, 1)])), b"a" * 259, isize=258, cls=E_OVERRUN)
    bad("ISIZE one long", raw, isize=len(text) + 1, cls=E_ISIZE)
    bad("stored block past ISIZE", deflate(text, level=0), isize=len(text) - 1, cls=E_OVERRUN)
    bad("stored block past the end", deflate(text, level=0)[:-1], cls=E_EOF)
    bad("CRC off by one", raw, crc=zlib.crc32(text) ^ 1, cls=E_CRC)
    bad("CRC off in its top bit", raw, crc=zlib.crc32(text) ^ 0x80000000, cls=E_CRC)
    bad("a byte behind the final block", raw + b"\0", cls=E_SLACK)

    whole = sound + sound + EOF_BLOCK
    cut = len(sound)
    out["BSIZE past the file"] = (sound + member(raw, text, bsize=len(sound) + len(EOF_BLOCK)) + EOF_BLOCK, "container", 1, IN_PAST_END)
    out["last member cut short"] = (whole[:2 * cut - 5], "container", 1, IN_PAST_END)
    out["header cut short"] = (sound + sound[:9], "container", 1, IN_PAST_END)
    out["trailing bytes"] = (whole + b"\0\0\0\0", "container", 3, IN_MAGIC)
    out["bad magic"] = (sound + b"\x1f\x8b\x08\x00" + sound[4:], "container", 1, IN_MAGIC)
    out["no BC subfield"] = (sound + member(raw, text).replace(b"BC", b"BD", 1) + EOF_BLOCK, "container", 1, IN_NO_BC)
    out["BSIZE below the header"] = (sound + member(raw, text, bsize=20) + EOF_BLOCK, "container", 1, IN_BSIZE)
    out["ISIZE 65537"] = (sound + member(raw, text, isize=65537) + EOF_BLOCK, "container", 1, IN_ISIZE)
    return out


def long_corrupt():
    """several bad members far apart in one container of about 800 members -> (container, index of the first bad one, its class)"""
    sound = good()["fastq in bgzip members"]
    bad = [corrupt()[n][0] for n in ("CRC off by one", "stream cut short", "first token a match at distance 1")]
    return sound * 100 + bad[0] + sound * 100 + bad[1] + bad[2], len(split_members(sound)) * 100 + 1, E_CRC


def bad_offset(name):
    """the file offset of a corrupt() entry's bad member: behind the one sound member, or where the trailing bytes begin"""
    data, _, index, _ = corrupt()[name]
    text = fastq_text()[:900]
    return len(data) - 4 if index == 3 else len(good_member(deflate(text), text))


@functools.lru_cache(maxsize=None)
def seeded():
    """32 single-byte corruptions of one dynamic member's deflate stream -> [(container, zlib's bytes or None)]"""
    text = fastq_text()[:3000]
    raw = deflate(text, level=9)
    assert raw[0] & 6 == 4      # a dynamic block
    rng, out = random.Random(1951), []
    for _ in range(32):
        at, flip = rng.randrange(len(raw)), 1 << rng.randrange(8)
        hit = raw[:at] + bytes([raw[at] ^ flip]) + raw[at + 1:]
        try:
            d = zlib.decompressobj(wbits=-15)
            ref = d.decompress(hit)
            ref = ref if d.eof and not d.unused_data else None
        except zlib.error:
            ref = None
        out.append((member(hit, text) + EOF_BLOCK, ref))
    return out


# ---- code-length sets that use the most subtable entries ---------------------------------------------------------------------------
def table_cases(nsyms, root):
    """complete codes of at most nsyms symbols and 15 bits with many and large subtables under `root`: chains (one code of every length from
    a depth on, two of the last) hung below as many root indexes as the symbols pay for"""
    cases = []
    for depth in range(root + 1, 16):
        per = depth - root + 1                          # symbols of a chain that fills a subtable of depth - root bits
        for chains in range(1, nsyms // per + 1):
            # `chains` root indexes carry a chain; the rest of the root is filled with codes of `root` bits or shorter
            if chains > 1 << root:
                break
            lens = []
            for _ in range(chains):
                lens += list(range(root + 1, depth)) + [depth, depth]
            free = (1 << root) - chains                 # root indexes left, to be covered by short codes
            short = []
            for ln in range(1, root + 1):               # greedy: the fewest codes that cover `free` indexes
                while free >= 1 << (root - ln):
                    short.append(ln)
                    free -= 1 << (root - ln)
            if len(lens) + len(short) <= nsyms:
                cases.append(sorted(lens + short))
    return cases
