"""pack_kernel at the edges of its range loop and of the cut: planes and lens read back bit for bit against the numpy packer of
test_gpu_pack_planes.py (and, with the tails argument set, against the oracle's views as test_gpu_tail_planes.py does).

The kernel converts a workgroup's two byte ranges vector by vector, a wave's 64 vectors always on one side, and cuts each string out
at its byte offset: so batches of 1, 255, 256, 257 and 513 pairs (a partial workgroup, one workgroup, a seam), lengths drawn from
0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128 mixed within a batch (ranges and strings start at every alignment, the sides'
vector counts fall on both sides of a multiple of 64), empty strings at the start, the middle and the end of a workgroup's range,
non-base bytes at vector edges, the bucketed layout, and strings long enough that a workgroup converts in rounds."""
import numpy as np
import pytest

from tests.test_gpu_pack_planes import _batch, _check
from tests.test_gpu_tail_planes import _compare

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _strings(rng, lens):
    return [ACGT[rng.integers(0, 4, int(k))].tobytes() for k in lens]


def _mixed(rng, n):
    return [LENGTHS[int(i)] for i in rng.integers(0, len(LENGTHS), n)]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_mixed_lengths_at_workgroup_edges(asm, engine, n):
    rng = np.random.default_rng(100 + n)
    _check(engine, _batch(asm, _strings(rng, _mixed(rng, n)), _strings(rng, _mixed(rng, n))))


@pytest.mark.parametrize("n", [1, 256, 513])
def test_every_length_uniform(asm, engine, n):
    """One length per batch, reads one character shorter than refs where there is one: each side's range ends at its own alignment."""
    rng = np.random.default_rng(7)
    for length in (1, 17, 100, 128):
        _check(engine, _batch(asm, _strings(rng, [length - 1] * n), _strings(rng, [length] * n)))


def test_empty_strings_at_the_start_middle_and_end_of_a_range(asm, engine):
    rng = np.random.default_rng(11)
    n = 513
    la, lb = _mixed(rng, n), _mixed(rng, n)
    for at in (0, 1, 127, 128, 254, 255, 256, 257, 400, 511, 512):  # both workgroups' first, middle and last pairs, and the seam
        la[at] = 0
        lb[at] = 0 if at % 2 else lb[at]
    _check(engine, _batch(asm, _strings(rng, la), _strings(rng, lb)))
    _check(engine, _batch(asm, _strings(rng, [0] * 257), _strings(rng, [0] * 257)))  # nothing to convert at all
    _check(engine, _batch(asm, _strings(rng, [0] * 300), _strings(rng, _mixed(rng, 300))))  # one side empty


def test_non_base_bytes_at_vector_edges(asm, engine):
    """Positions 0, 15, 16, 31 of a workgroup's range (and of later vectors) hold bytes that are no base: lower case, N, NUL, 0xFF and
    the bytes one bit away from a base."""
    rng = np.random.default_rng(13)
    n = 300
    la, lb = [100] * n, [100] * n
    reads = np.frombuffer(b"".join(_strings(rng, la)), np.uint8).copy()
    refs = np.frombuffer(b"".join(_strings(rng, lb)), np.uint8).copy()
    odd = np.array(list(b"Nnacgt") + [0x00, 0xff, 0x40, 0x45, 0x4f, 0x53, 0x55, 0x44, 0x14, 0xc3, 0x03, 0x07], np.uint8)
    for text in (reads, refs):
        for v in (0, 1, 63, 64, 100, 1599, 1600, 1601):  # vectors of the first and of the second workgroup's range
            for p in (0, 15, 16, 31):
                text[16 * v + p] = odd[rng.integers(0, odd.size)]
    off = np.arange(n + 1, dtype=np.uint32) * 100
    _check(engine, asm.HostBatch(reads, off, refs, off.copy()))


def test_tails_in_sequential_mode(asm, engine, oracle):
    rng = np.random.default_rng(17)
    n = 513
    hb = _batch(asm, _strings(rng, _mixed(rng, n)), _strings(rng, _mixed(rng, n)))
    _compare(hb, oracle.greedy_views(hb, 0), engine.upload(hb, asm.GREEDY_SEQUENTIAL), "mixed lengths, sequential")


def test_bucketed_layout(asm, engine):
    """Lengths of all four width classes in one batch, enough pairs that it is bucketed."""
    rng = np.random.default_rng(19)
    n = 6000
    pool = LENGTHS + [129, 160, 255, 256, 257, 384, 385, 512]
    la = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    lb = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    order = _check(engine, _batch(asm, _strings(rng, la), _strings(rng, lb)))
    assert not np.array_equal(order, np.arange(order.size))


@pytest.mark.parametrize("n,length", [(256, 264), (257, 272)])
def test_rounds(asm, engine, n, length):
    """256 strings of 264 characters per side are the least for which a workgroup's plane arrays, 2 * (pdA + pdB) = 8452 dwords, exceed
    the 8448 the host gives it (33 KiB): each side is then converted in rounds.  263 characters (8420 dwords) still fit."""
    rng = np.random.default_rng(23)
    _check(engine, _batch(asm, _strings(rng, [length] * n), _strings(rng, [length] * n)))
