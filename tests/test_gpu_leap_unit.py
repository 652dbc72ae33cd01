"""leap_unit_kernel and leap_unit_hint_kernel around the per-pair core of csrc/asm_leapunit.h: batches at the hint kernel's
workgroup edge (256 pairs) and with a tail workgroup, lengths at the word edges of the one-granule form, k = 1, 2, 3,
un-hinted, hinted by the NW penalties and hinted by an all-zero estimate; and one batch of 129-192 bases, the three-word
width the one-granule form does not touch.  Everything is compared with the oracle, exactly.  The host logic is in
test_leap_unit_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = (1, 2, 3, 4, 62, 63, 64, 65, 66, 99, 100, 101, 126, 127, 128)
BATCHES = (1, 255, 256, 257, 513)


def edge_length_pairs(rng, count, k):
    """Reads of the edge lengths against themselves after 0-8 edits; the reference's length stays within k of an edge length
    or not, as the edits fall."""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for i in range(count):
        a = list(acgt[rng.integers(0, 4, EDGE_LENGTHS[int(rng.integers(0, len(EDGE_LENGTHS)))])])
        b = list(a)
        for _ in range(int(rng.integers(0, 9))):
            u = rng.random()
            if u < 0.6 or (len(b) <= 1 and u < 0.8):
                b[int(rng.integers(0, len(b)))] = acgt[rng.integers(0, 4)]
            elif u < 0.8 or len(b) >= 128:
                del b[int(rng.integers(0, len(b)))]
            else:
                b.insert(int(rng.integers(0, len(b) + 1)), acgt[rng.integers(0, 4)])
        pairs.append((bytes(bytearray(int(c) for c in a)).decode(), bytes(bytearray(int(c) for c in b)).decode()))
    return pairs


def three_ways(asm, engine, hb, params, want):
    n = hb.n
    batch = engine.upload(hb)
    d_nw, d_leap = engine.malloc(4 * n), engine.malloc(4 * n)
    try:
        engine.memset_async(d_leap, 0xff, 4 * n)
        engine.align_async(batch, asm.LEAP, params, d_leap)
        assert np.array_equal(engine.to_host(d_leap, n), want), "un-hinted"
        engine.align_async(batch, asm.NW, params, d_nw)
        engine.memset_async(d_leap, 0xff, 4 * n)
        engine.align_hinted_async(batch, asm.LEAP, params, d_nw, d_leap)
        assert np.array_equal(engine.to_host(d_leap, n), want), "hinted by NW"
        engine.memset_async(d_nw, 0, 4 * n)
        engine.memset_async(d_leap, 0xff, 4 * n)
        engine.align_hinted_async(batch, asm.LEAP, params, d_nw, d_leap)
        assert np.array_equal(engine.to_host(d_leap, n), want), "hinted by zeros"
    finally:
        engine.free(d_nw), engine.free(d_leap)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n", BATCHES)
def test_word_edge_lengths_at_the_workgroup_edge(asm, engine, oracle, n, k):
    rng = np.random.default_rng(1000 * k + n)
    hb = asm.HostBatch.from_strings(edge_length_pairs(rng, n, k))
    three_ways(asm, engine, hb, asm.Params.default(k=k, x=1, o=1, e=1), oracle.leap(hb, k=k))


def test_three_word_width_is_untouched(asm, engine, oracle):
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for i in range(513):
        a = acgt[rng.integers(0, 4, int(rng.integers(129, 193)))]
        b = a.copy()
        hit = rng.random(len(b)) < 0.04
        b[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        b = b[:max(129, len(b) - int(rng.integers(0, 3)))]
        pairs.append((bytes(a).decode(), bytes(b).decode()))
    hb = asm.HostBatch.from_strings(pairs)
    three_ways(asm, engine, hb, asm.Params.default(k=3, x=1, o=1, e=1), oracle.leap(hb, k=3))
