"""nw_banded2_kernel on the GPU: unit-cost NW of one-granule batches with two pairs per thread (16-row windows side by side in
one dword, csrc/asm_nwband.h), bit for bit against the oracle and against the one-pair-per-thread kernel (ASM_NW_PAIR2=0).
The sweep's own logic is checked on the CPU in test_nw_pair2_host.py; here: the thread-to-pair mapping at workgroup edges,
threads without a partner, couples of different lengths, and the cascade for halves the 16-row window does not settle."""
import os

import numpy as np
import pytest

from tests.test_nw_pair2_host import edited_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_one_pair(asm, engine):
    """A second handle created with ASM_NW_PAIR2=0 (the switch is read once, at creation): the parent's launch."""
    old = os.environ.get("ASM_NW_PAIR2")
    os.environ["ASM_NW_PAIR2"] = "0"
    try:
        eng = asm.Engine(0)
    finally:
        if old is None:
            del os.environ["ASM_NW_PAIR2"]
        else:
            os.environ["ASM_NW_PAIR2"] = old
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def mixed(asm, oracle):
    """1025 pairs of lengths 1-128 with 0-20 edits, and the oracle's penalties; prefixes of it are the small batches."""
    rng = np.random.default_rng(5)
    pairs = edited_pairs(rng, 1025, 1, 128, 0, 20, 0.7)
    return pairs, oracle.nw(asm.HostBatch.from_strings(pairs))


def nw(asm, eng, hb):
    _, _, params = asm.workload("C2")
    return eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.NW, params)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 512, 513, 1025])
def test_counts_at_the_workgroup_edges(asm, engine, engine_one_pair, mixed, n):
    """An odd count, a thread without a partner (n <= 256 and 512 < n <= 768: nobody or only some have one), full and
    partly filled workgroups of 512 pairs; lengths 1-128 mixed, so the two halves of a dword end at different columns."""
    pairs, want = mixed
    hb = asm.HostBatch.from_strings(pairs[:n])
    got = nw(asm, engine, hb)
    assert np.array_equal(got, want[:n])
    assert np.array_equal(nw(asm, engine_one_pair, hb), got)


def test_c2_pairs(asm, engine, engine_one_pair, oracle):
    """The benchmark's shape: 4096 generated C2 pairs (100 bases, 10 edits), all settled by the 16-row pass."""
    cfg, _, _ = asm.workload("C2")
    hb = asm.generate_pairs(cfg, 0, 4096)
    got = nw(asm, engine, hb)
    assert np.array_equal(got, oracle.nw(hb))
    assert np.array_equal(nw(asm, engine_one_pair, hb), got)


def test_halves_that_take_the_cascade(asm, engine, engine_one_pair, oracle):
    """100 bases with 20 edits: most distances are above 14 - |n-m|, so most halves go on to the 32-row window in the same
    thread, often only one of a thread's two."""
    rng = np.random.default_rng(9)
    hb = asm.HostBatch.from_strings(edited_pairs(rng, 2048, 100, 100, 20, 20, 0.8))
    want = oracle.nw(hb)
    m, n = hb.lengths()
    beyond = want > 14 - np.abs(n - m)
    assert 0.5 < beyond.mean() < 1.0  # both kinds are present
    got = nw(asm, engine, hb)
    assert np.array_equal(got, want)
    assert np.array_equal(nw(asm, engine_one_pair, hb), got)
