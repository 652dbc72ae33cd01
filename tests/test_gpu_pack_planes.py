"""pack_kernel's output read back bit for bit: the uint4[4][w4][bn] bucketed planes and the lens words, against a numpy packer
written from the rule (A=00 C=01 G=10 T=11; any byte other than exactly 'C', 'G', 'T' is 00; bits at and beyond a string's
length are 0).  Clean mode only: the sequential-mode tails are read back the same way in test_gpu_tail_planes.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LUT = np.zeros(256, np.uint8)
LUT[ord("C")], LUT[ord("G")], LUT[ord("T")] = 1, 2, 3


def _side_bits(text, off, idx, w4):
    """(len(idx), 2, w4, 4) uint32: plane p of the strings idx of one side, granule g, dword w."""
    text = np.concatenate([np.asarray(text, np.uint8), np.zeros(w4 * 128, np.uint8)])
    L = (off[idx + 1] - off[idx]).astype(np.int64)
    col = np.arange(w4 * 128)
    codes = LUT[text[off[idx].astype(np.int64)[:, None] + col[None, :]]]
    codes[col[None, :] >= L[:, None]] = 0
    out = np.empty((len(idx), 2, w4, 4), np.uint32)
    for p in range(2):
        bits = ((codes >> p) & 1).astype(np.uint8)
        out[:, p] = np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(len(idx), w4, 4)
    return out


def _expected(hb, order, planes_entries):
    n = hb.n
    ro, fo = hb.read_off.astype(np.int64), hb.ref_off.astype(np.int64)
    m, nn = ro[1:] - ro[:-1], fo[1:] - fo[:-1]
    maxlen = int(max(m.max(initial=0), nn.max(initial=0)))
    wmax = 1 if maxlen <= 128 else (maxlen + 127) // 128
    if planes_entries == 4 * wmax * max(n, 1) or n == 0:
        buckets = [(0, n, wmax)]
    else:  # several width classes, in class order
        cls = np.minimum((np.maximum(np.maximum(m, nn), 1)[order] + 127) // 128 - 1, 3)
        assert np.all(np.diff(cls) >= 0)
        buckets = [(int(np.searchsorted(cls, c)), int(np.searchsorted(cls, c, "right")), c + 1) for c in np.unique(cls)]
    planes = np.zeros((planes_entries, 4), np.uint32)
    base = 0
    for lo, hi, w4 in buckets:
        bn, idx = hi - lo, order[lo:hi].astype(np.int64)
        for s, (text, off) in enumerate(((hb.reads, hb.read_off), (hb.refs, hb.ref_off))):
            bits = _side_bits(text, off.astype(np.int64), idx, w4)
            for p in range(2):
                for g in range(w4):
                    at = base + ((2 * s + p) * w4 + g) * bn
                    planes[at:at + bn] = bits[:, p, g]
        base += 4 * w4 * bn
    lens = (m | (nn << 16)).astype(np.uint32)[order]
    return planes, lens


def _check(engine, hb):
    batch = engine.upload(hb)
    planes, lens, order = batch.download_planes()
    assert np.array_equal(np.sort(order), np.arange(hb.n, dtype=np.uint32))
    want_planes, want_lens = _expected(hb, order.astype(np.int64), planes.shape[0])
    bad = np.nonzero(lens != want_lens)[0]
    assert bad.size == 0, f"lens: {bad.size} slots differ, first {bad[:5]}"
    bad = np.nonzero((planes != want_planes).any(axis=1))[0]
    assert bad.size == 0, f"planes: {bad.size} of {planes.shape[0]} entries differ, first {bad[:5]}"
    return order


def _batch(asm, reads_list, refs_list):
    def cat(strs):
        off = np.zeros(len(strs) + 1, np.uint32)
        off[1:] = np.cumsum([len(s) for s in strs])
        text = np.frombuffer(b"".join(strs), np.uint8) if off[-1] else np.zeros(0, np.uint8)
        return text.copy(), off
    (ra, ro), (fa, fo) = cat(reads_list), cat(refs_list)
    return asm.HostBatch(ra, ro, fa, fo)


def test_pack_planes_c2(asm, engine):
    cfg, _, _ = asm.workload("C2")
    _check(engine, asm.generate_pairs(cfg, 0, 100000))


def test_pack_planes_dirty_alphabet(asm, engine):
    rng = np.random.default_rng(3)
    pool = np.array(list(b"ACGTACGTACGTNnacgt-*BDEFHU@") + [0, 1, 2, 0x42, 0x44, 0x53, 0x55, 0x7f, 0x80, 0xc3, 0xd4, 0xff],
                    np.uint8)
    n = 4000
    la, lb = rng.integers(0, 200, n), rng.integers(0, 200, n)
    reads = [pool[rng.integers(0, pool.size, int(k))].tobytes() for k in la]
    refs = [pool[rng.integers(0, pool.size, int(k))].tobytes() for k in lb]
    _check(engine, _batch(asm, reads, refs))


@pytest.mark.parametrize("n", [3001, 256, 1])
def test_pack_planes_edge_lengths(asm, engine, n):
    """Lengths at and around the 32-bit words and 128-position granules, at every byte alignment; n not a multiple of 256."""
    rng = np.random.default_rng(n)
    edges = [0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 511, 512]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    la = [edges[int(i)] for i in rng.integers(0, len(edges), n)]
    lb = [edges[int(i)] for i in rng.integers(0, len(edges), n)]
    reads = [acgt[rng.integers(0, 4, k)].tobytes() for k in la]
    refs = [acgt[rng.integers(0, 4, k)].tobytes() for k in lb]
    _check(engine, _batch(asm, reads, refs))


def test_pack_planes_c5_bucketed(asm, engine):
    """Mixed lengths: several width classes, pairs routed through the pos permutation."""
    cfg, _, _ = asm.workload("C5")
    order = _check(engine, asm.generate_pairs(cfg, 17, 12000))
    assert not np.array_equal(order, np.arange(order.size))


def test_pack_planes_long_strings_take_rounds(asm, engine):
    """Blocks of 256 strings of 300-512 characters: both sides' planes exceed the workgroup's LDS, so each side is packed in
    its own round; ragged, so that the rounds start at every byte alignment."""
    rng = np.random.default_rng(7)
    n = 1300
    acgt = np.frombuffer(b"ACGTN", np.uint8)
    la, lb = rng.integers(300, 513, n), rng.integers(300, 513, n)
    reads = [acgt[rng.integers(0, 5, int(k))].tobytes() for k in la]
    refs = [acgt[rng.integers(0, 4, int(k))].tobytes() for k in lb]
    _check(engine, _batch(asm, reads, refs))
