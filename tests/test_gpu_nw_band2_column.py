"""nw_banded2_kernel with the repriced column of nw_band2x16 (csrc/asm_nwband.h) on the GPU, penalties bit for bit against
the oracle: pair counts around a thread without a partner, a partly filled workgroup and the seam at base + 256, each with the
benchmark's 100-base pairs and with the block-edge lengths of test_nw_band2_column_host.py (which checks the column's state on the
CPU), and one batch in which about one pair in a hundred leaves the 16-row window for the cascade."""
import numpy as np
import pytest

from tests.test_nw_band2_column_host import edge_pairs
from tests.test_nw_pair2_host import edited_pairs

pytestmark = pytest.mark.gpu
COUNTS = [1, 2, 255, 256, 257, 511, 512, 513, 1025]


@pytest.fixture(scope="module")
def sets(asm, oracle):
    """1025 pairs of either kind and the oracle's penalties, computed once; the smaller batches are prefixes."""
    rng = np.random.default_rng(17)
    c2 = edited_pairs(rng, 1025, 100, 100, 10, 10, 0.96)
    edge = edge_pairs()
    edge = [edge[i] for i in rng.permutation(len(edge))[:1025]]  # shuffled: a prefix holds every length class
    return {name: (pairs, oracle.nw(asm.HostBatch.from_strings(pairs))) for name, pairs in (("c2", c2), ("edge", edge))}


def nw(asm, eng, hb):
    _, _, params = asm.workload("C2")
    return eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.NW, params)


@pytest.mark.parametrize("kind", ["c2", "edge"])
@pytest.mark.parametrize("n", COUNTS)
def test_counts_and_shapes(asm, engine, sets, n, kind):
    pairs, want = sets[kind]
    got = nw(asm, engine, asm.HostBatch.from_strings(pairs[:n]))
    assert np.array_equal(got, want[:n])


def test_one_in_a_hundred_takes_the_cascade(asm, engine, oracle):
    """4096 pairs of 100 bases, 10 edits, every hundredth with 40: those are beyond 14 - |n-m| and go on to the wider windows
    in their thread while the partner's half is settled."""
    rng = np.random.default_rng(23)
    pairs = edited_pairs(rng, 4096, 100, 100, 10, 10, 0.96)
    far = edited_pairs(rng, 41, 100, 100, 40, 40, 0.9)
    for j, p in enumerate(far):
        pairs[100 * j + 7] = p
    hb = asm.HostBatch.from_strings(pairs)
    want = oracle.nw(hb)
    m, n = hb.lengths()
    beyond = (want > 14 - np.abs(n - m)).mean()
    assert 0.005 < beyond < 0.02, beyond
    assert np.array_equal(nw(asm, engine, hb), want)
