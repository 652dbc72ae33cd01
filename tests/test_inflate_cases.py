"""tests/inflate_cases.py against zlib on zlib's own output, so that a mistake in the decoder cannot hide behind the encoder it is
used to check; and its package-merge lengths against plain Huffman where the limit does not bind."""
import random
import zlib

import pytest

from tests import deflate_cases as dc
from tests import inflate_cases as ic

PAYLOADS = ("text 1025", "records 65280", "zeros 1024", "random 257", "period 259", "long run", "all bytes", "one byte")


def blocks_of(stream):
    """every block of a zlib stream: BFINAL on the last one only, and a match may reach into the blocks in front"""
    out, at, done = [], 0, b""
    while True:
        inf = ic.inflate(stream, history=done, at=at, final=None)
        out.append(inf)
        at, done = inf["end_bit"], done + inf["payload"]
        if inf["final"]:
            return out, at


@pytest.mark.parametrize("level", [1, 6, 9])
def test_decoder_against_zlib(level):
    seen = set()
    for name in PAYLOADS:
        src = dc.corpus()[name]
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED):
            z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
            stream = z.compress(src) + z.flush()
            blocks, end = blocks_of(stream)
            assert b"".join(b["payload"] for b in blocks) == src == zlib.decompress(stream, wbits=-15), (name, level)
            assert (end + 7) // 8 == len(stream)
            for b in blocks:
                seen.add(b["btype"])
                at = 0
                for t in b["tokens"]:
                    assert t[0] == at
                    at += 1 if len(t) == 2 else t[1]
                assert at == len(b["payload"]) or b["btype"] == 0
                if b["btype"] == 2:
                    assert ic.kraft(b["ll_lens"]) <= 1 << 15 and len(b["ll_lens"]) == b["hlit"] and len(b["d_lens"]) == b["hdist"]
                    assert b["end_bit"] - b["head_bits"] == ic.token_bits(b["tokens"], b["ll_lens"] + [0] * 30, b["d_lens"] + [0] * 30)
                    assert sum(b["widths"]) + b["ll_lens"][256] == b["end_bit"] - b["head_bits"]
                    ll, d = ic.histograms(b["tokens"])
                    assert all(b["ll_lens"][s] for s, w in enumerate(ll) if w) and all(b["d_lens"][s] for s, w in enumerate(d) if w)
                if b["btype"] == 1:
                    assert b["end_bit"] - b["head_bits"] == ic.token_bits(b["tokens"], ic.FIXED_LL, ic.FIXED_D)
    assert {1, 2} <= seen


def test_stored_block():
    src = dc.corpus()["random 257"]
    z = zlib.compressobj(0, wbits=-15)
    inf = ic.inflate_checked(z.compress(src) + z.flush())
    assert inf["btype"] == 0 and inf["payload"] == src and inf["end_bit"] == 40 + 8 * len(src)


def test_symbols_are_the_rfc_tables():
    assert ic.len_symbol(3) == (257, 0) and ic.len_symbol(10) == (264, 0) and ic.len_symbol(11) == (265, 1) and ic.len_symbol(64) == (276, 3)
    assert ic.len_symbol(257) == (284, 5) and ic.len_symbol(258) == (285, 0)
    assert ic.dist_symbol(1) == (0, 0) and ic.dist_symbol(4) == (3, 0) and ic.dist_symbol(5) == (4, 1) and ic.dist_symbol(4096) == (23, 10)
    assert ic.dist_symbol(24577) == (29, 13) and ic.dist_symbol(32768) == (29, 13)


def test_package_merge_is_huffman_where_the_limit_does_not_bind():
    rng = random.Random(3)
    for trial in range(60):
        w = [rng.choice((0, 0, 1, 2, 3, 5, 40, 900)) * rng.randrange(1, 4) for _ in range(rng.randrange(2, 60))]
        h = ic.huffman_lengths(w)
        if sum(1 for v in w if v) < 2:
            continue
        assert ic.kraft(h, 40) == 1 << 40
        for limit in (max(h), max(h) + 1, 15 if max(h) <= 15 else max(h)):
            pm = ic.package_merge_lengths(w, limit)
            assert ic.cost(w, pm) == ic.cost(w, h) and max(pm) <= limit and ic.kraft(pm, 40) == 1 << 40, (w, limit)


def test_package_merge_under_a_binding_limit():
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    h = ic.huffman_lengths(fib)
    assert max(h) == 19
    last = None
    for limit in (19, 15, 10, 7, 5):
        pm = ic.package_merge_lengths(fib, limit)
        assert max(pm) == limit and ic.kraft(pm, 40) == 1 << 40
        assert all(pm[i] >= pm[i + 1] for i in range(19)), "a rarer symbol never has the shorter code"
        assert last is None or ic.cost(fib, pm) > last, "a tighter limit costs bits"
        last = ic.cost(fib, pm)
    # four symbols in two bits: only the flat code
    assert ic.package_merge_lengths([1, 2, 4, 100], 2) == [2, 2, 2, 2]
    # brute force over every complete code of six symbols in at most three bits
    w = [1, 2, 3, 5, 8, 40]
    import itertools
    best = min(ic.cost(w, c) for c in itertools.product((1, 2, 3), repeat=6) if ic.kraft(c, 3) == 8)
    assert ic.cost(w, ic.package_merge_lengths(w, 3)) == best
