"""A token-level deflate decoder, written from RFC 1951 alone, and the two code builders the deflate tests measure against: plain
Huffman lengths and package-merge length-limited lengths (Larmore and Hirschberg).  Pure Python, standard library only.  It does not
share a line or a table with csrc/asm_deflate.h: the tables below are the RFC's, section 3.2.5 to 3.2.7.

inflate(stream) decodes one deflate block with BFINAL = 1 (what one BGZF block holds) and keeps what zlib throws away: the header's
fields and symbols, every token with its place and its width, and where the bits end.  tests/test_inflate_cases.py checks it against
zlib on zlib's own output; deflate_cases.check_tokens checks it against zlib on every block it reads."""
import heapq
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8           # 288 lengths; 286 and 287 take part in the code and never occur
FIXED_D = [5] * 32                                              # 30 and 31 likewise


def len_symbol(length):
    """-> (symbol, extra bits) of a match length in [3, 258]"""
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= length:
            assert length - LEN_BASE[s] < (1 << LEN_EXTRA[s]) or (LEN_EXTRA[s] == 0 and length == LEN_BASE[s])
            return 257 + s, LEN_EXTRA[s]
    raise AssertionError(length)


def dist_symbol(dist):
    """-> (symbol, extra bits) of a distance in [1, 32 768]"""
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= dist:
            assert dist - DIST_BASE[s] < (1 << DIST_EXTRA[s])
            return s, DIST_EXTRA[s]
    raise AssertionError(dist)


class Bits:
    """the stream's bits, least significant bit of each byte first (RFC 1951, 3.1.1)"""

    def __init__(self, data):
        self.data = bytes(data) + bytes(8)
        self.n = 8 * len(data)
        self.at = 0

    def peek(self, n):                                        # n <= 24
        at = self.at
        return (int.from_bytes(self.data[at >> 3:(at >> 3) + 4], "little") >> (at & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.at += n
        assert self.at <= self.n, "the stream ends inside a field"
        return v


def decoder(lengths):
    """the canonical code of RFC 1951, 3.2.2 for `lengths` -> (table, width): table[the next `width` bits as they lie in the stream]
    = (symbol, length), or None where no code begins (an incomplete code)"""
    width = max(lengths)
    assert 0 < width <= 15
    count = [0] * (width + 1)
    for v in lengths:
        count[v] += 1
    count[0] = 0
    code, nxt = 0, [0] * (width + 1)
    for b in range(1, width + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    assert sum(c << (width - b) for b, c in enumerate(count) if b) <= 1 << width, "an oversubscribed code"
    table = [None] * (1 << width)
    for s, v in enumerate(lengths):
        if v:
            c = nxt[v]
            nxt[v] += 1
            r = int(format(c, "0%db" % v)[::-1], 2)             # Huffman codes are packed most significant bit first
            for hi in range(1 << (width - v)):
                table[r | (hi << v)] = (s, v)
    return table, width


def symbol(bits, dec):
    table, width = dec
    e = table[bits.peek(width)]
    assert e is not None, "bits that no code starts with, at bit %d" % bits.at
    bits.at += e[1]
    assert bits.at <= bits.n
    return e


def inflate(stream, history=b"", at=0, final=1):
    """one deflate block, by default the whole stream's only one with BFINAL = 1 (what a BGZF block holds); for zlib's streams of
    several blocks: the block at bit `at` behind the payload `history`, final: the BFINAL it must have, or None -> dict:
      final                    BFINAL
      btype
      hlit, hdist, hclen       the counts themselves (257.., 1.., 4..), BTYPE 2 only, as are the next four
      cl_lens                  the 19 lengths of the code-length alphabet, by symbol
      ll_lens, d_lens          hlit and hdist lengths
      head_syms                [(symbol of the code-length alphabet, its extra bits' value)]
      tokens                   [(start, byte)] and [(start, length, distance)], in order
      widths                   every token's bits
      head_bits                the bits in front of the first token, the three of BFINAL and BTYPE included
      end_bit                  the bit behind the end-of-block symbol (BTYPE 0: behind the last byte)
      payload                  rebuilt from the tokens
    """
    bits = Bits(stream)
    bits.at = at
    bfinal = bits.take(1)
    assert final is None or bfinal == final, "BFINAL"
    out = dict(final=bfinal, btype=bits.take(2), tokens=[], widths=[])
    assert out["btype"] != 3
    if out["btype"] == 0:
        pad = bits.take(-bits.at % 8)
        assert pad == 0, "padding in front of LEN"
        n, nn = bits.take(16), bits.take(16)
        assert n ^ nn == 0xffff, "LEN and NLEN"
        assert bits.at + 8 * n <= bits.n
        out.update(head_bits=bits.at, payload=bytes(stream[bits.at // 8:bits.at // 8 + n]), end_bit=bits.at + 8 * n)
        return out
    if out["btype"] == 1:
        ll, d = FIXED_LL, FIXED_D
    else:
        hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
        assert hlit <= 286 and hdist <= 30
        cl = [0] * 19
        for i in range(hclen):
            cl[CL_ORDER[i]] = bits.take(3)
        dec, lens, syms = decoder(cl), [], []
        while len(lens) < hlit + hdist:
            s, _ = symbol(bits, dec)
            if s < 16:
                syms.append((s, 0))
                lens.append(s)
            elif s == 16:
                assert lens, "a repeat with nothing in front of it"
                x = bits.take(2)
                syms.append((s, x))
                lens += [lens[-1]] * (3 + x)
            else:
                x = bits.take(3 if s == 17 else 7)
                syms.append((s, x))
                lens += [0] * ((3 if s == 17 else 11) + x)
        assert len(lens) == hlit + hdist, "a run past the end of the lengths"
        ll, d = lens[:hlit], lens[hlit:]
        assert ll[256], "no code for the end of the block"
        out.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl, ll_lens=ll, d_lens=d, head_syms=syms)
    out["head_bits"] = bits.at
    dec_ll = decoder(ll)
    dec_d = decoder(d) if any(d) else None
    buf, tokens, widths, base = bytearray(history), out["tokens"], out["widths"], len(history)
    while True:
        at = bits.at
        s, _ = symbol(bits, dec_ll)
        if s < 256:
            tokens.append((len(buf) - base, s))
            buf.append(s)
        elif s == 256:
            break
        else:
            assert s <= 285, "length symbol %d" % s
            length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
            assert dec_d is not None, "a match without a distance code"
            ds, _ = symbol(bits, dec_d)
            assert ds <= 29, "distance symbol %d" % ds
            dist = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
            assert dist <= len(buf), "a distance in front of the block"
            tokens.append((len(buf) - base, length, dist))
            for _ in range(length):
                buf.append(buf[-dist])
        widths.append(bits.at - at)
    out.update(end_bit=bits.at, payload=bytes(buf[base:]))
    return out


def inflate_checked(stream):
    """inflate, with the payload held against zlib's"""
    out = inflate(stream)
    assert out["payload"] == zlib.decompress(stream, wbits=-15)
    return out


def histograms(tokens):
    """-> (literal/length counts with the end-of-block symbol, 286; distance counts, 30)"""
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if len(t) == 2:
            ll[t[1]] += 1
        else:
            ll[len_symbol(t[1])[0]] += 1
            d[dist_symbol(t[2])[0]] += 1
    return ll, d


def token_bits(tokens, ll_lens, d_lens):
    """the tokens' bits under the two codes, extra bits and the end-of-block symbol included"""
    n = ll_lens[256]
    for t in tokens:
        if len(t) == 2:
            assert ll_lens[t[1]]
            n += ll_lens[t[1]]
        else:
            (ls, lx), (ds, dx) = len_symbol(t[1]), dist_symbol(t[2])
            assert ll_lens[ls] and d_lens[ds]
            n += ll_lens[ls] + lx + d_lens[ds] + dx
    return n


# ---- code builders ------------------------------------------------------------------------------------------------------------------
def huffman_lengths(weights):
    """plain Huffman lengths of the used symbols (weight > 0) -> lengths by symbol.  Among equal weights the shallower subtree is merged
    first, which gives the tree of the least depth among the optimal ones."""
    used = [s for s, w in enumerate(weights) if w]
    out = [0] * len(weights)
    if len(used) == 1:
        out[used[0]] = 1
    if len(used) < 2:
        return out
    heap = [(weights[s], 0, s, (s,)) for s in used]
    heapq.heapify(heap)
    tick = len(weights)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[3] + b[3]:
            out[s] += 1
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick, a[3] + b[3]))
        tick += 1
    return out


def package_merge_lengths(weights, limit):
    """optimal lengths of at most `limit` bits for the used symbols -> lengths by symbol"""
    used = sorted((w, s) for s, w in enumerate(weights) if w)
    out = [0] * len(weights)
    if len(used) == 1:
        out[used[0][1]] = 1
    if len(used) < 2:
        return out
    assert len(used) <= 1 << limit
    leaves = [(w, (s,)) for w, s in used]
    row = list(leaves)
    for _ in range(limit - 1):
        packed = [(row[i][0] + row[i + 1][0], row[i][1] + row[i + 1][1]) for i in range(0, len(row) - 1, 2)]
        row = sorted(leaves + packed, key=lambda it: it[0])
    for _, syms in row[:2 * len(used) - 2]:
        for s in syms:
            out[s] += 1
    return out


def cost(weights, lengths):
    return sum(w * v for w, v in zip(weights, lengths))


def kraft(lengths, limit=15):
    """the code's Kraft sum in units of 2^-limit: 1 << limit for a complete code"""
    return sum(1 << (limit - v) for v in lengths if v)
