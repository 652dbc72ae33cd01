"""The filter kernels at their seams, against the CPU oracle: pair counts on both sides of every workgroup size (16 pairs of the
four-threads-per-pair affine kernel, 16 / 32 / 64 threads of the thread-per-pair one, SIMD_ED_THREADS = 128, ASM_BLOCK = 256), string
lengths on both sides of every plane word and of the 256-character cut with references shorter than, equal to and longer than the
read, thresholds on both sides of the register forms' limit (8 | 9), at SHD's limit (16) and at the maximum (32), every ED_mode, and
a batch packed for Greedy's sequential mode, whose stale tails meet the shared clip.  Small batches: the parity tests in
test_gpu_parity.py carry the volume."""
import numpy as np
import pytest

from tests.oracle_binding import SIMD_WARM_STATE
from tests.test_filter_host import edge_batch
from tests.util import check

pytestmark = pytest.mark.gpu

COUNTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
AFFINE = ((3, 60, 2, 3, 1), (8, 100, 4, 6, 2), (32, 200, 15, 15, 15))  # the last: 16 threads per workgroup in the thread-per-pair kernel


@pytest.fixture(scope="module")
def pools(asm):
    """name -> shuffled list of pairs over the edge lengths: 'short' (both strings <= 128: one bucket, the quad kernel), 'long' (the longer
    one in 129..256: one bucket, the thread-per-pair kernel), 'mixed' (everything, reads of 257 and 300 included: several buckets)"""
    pairs = []
    for seed in (11, 12, 13):
        hb = edge_batch(asm, seed)
        pairs += [hb.pair(i) for i in range(hb.n)]
    order = np.random.default_rng(3).permutation(len(pairs))
    pairs = [pairs[int(i)] for i in order]
    top = [max(len(a), len(b)) for a, b in pairs]
    out = {"short": [p for p, t in zip(pairs, top) if t <= 128], "long": [p for p, t in zip(pairs, top) if 128 < t <= 256], "mixed": pairs}
    assert all(len(v) >= max(COUNTS) for v in out.values())
    return out


def batches(asm, engine, pools, n, mode=None):
    for name in ("short", "long") if n != max(COUNTS) else ("short", "long", "mixed"):
        hb = asm.HostBatch.from_strings(pools[name][:n])
        yield f"{name} n={n}", hb, engine.upload(hb, asm.GREEDY_CLEAN if mode is None else mode)


def lev_cases():
    for t in (1, 8, 9, 16, 32):
        for shd in (True, False) if t <= 16 else (False,):
            yield t, shd, 0
    for ed_mode in (1, 2, 3):
        for t in (8, 9):
            yield t, True, ed_mode


@pytest.mark.parametrize("n", COUNTS)
def test_levenshtein_at_block_edges(asm, engine, oracle, pools, n):
    for name, hb, batch in batches(asm, engine, pools, n):
        for t, shd, ed_mode in lev_cases():
            for mode in (asm.FILTER_CLEAN, asm.FILTER_SEQUENTIAL):
                want, _, _ = oracle.simd_ed(hb, t, shd, mode, SIMD_WARM_STATE, ed_mode=ed_mode)
                got = engine.simd_ed(batch, t, shd, mode, SIMD_WARM_STATE, ed_mode=ed_mode)
                check(f"{name} T={t} shd={shd} ed_mode={ed_mode} mode={mode}", got, want, hb)


@pytest.mark.parametrize("n", COUNTS)
def test_sequential_state_at_block_edges(asm, engine, oracle, pools, n):
    """The state a sequential call returns, by what it does: the same batch filtered again from it gives the second half of the
    oracle's verdicts for the batch twice over."""
    for name, hb, batch in batches(asm, engine, pools, n):
        a, b = zip(*[hb.pair(i) for i in range(hb.n)])
        twice = asm.HostBatch.from_strings(list(zip(a + a, b + b)))
        d = engine.malloc(4 * n)
        try:
            for t, shd, ed_mode in ((8, True, 0), (9, True, 0), (9, False, 2), (32, False, 0)):
                want, _, _ = oracle.simd_ed(twice, t, shd, asm.FILTER_SEQUENTIAL, SIMD_WARM_STATE, ed_mode=ed_mode)
                state = engine.simd_ed_async(batch, t, d, shd, asm.FILTER_SEQUENTIAL, SIMD_WARM_STATE, ed_mode)
                check(f"{name} T={t} first pass", engine.to_host(d, n), want[:n], hb)
                engine.simd_ed_async(batch, t, d, shd, asm.FILTER_SEQUENTIAL, state, ed_mode)
                check(f"{name} T={t} from the returned state {state}", engine.to_host(d, n), want[n:], hb)
        finally:
            engine.free(d)


@pytest.mark.parametrize("n", COUNTS)
def test_affine_at_block_edges(asm, engine, oracle, pools, n):
    for name, hb, batch in batches(asm, engine, pools, n):
        for g, af, x, o, e in AFFINE:
            for st in (None, 0, min(g, 16)):
                for mode in (0, 1, 2, 3):
                    want, _ = oracle.simd_ed_affine(hb, g, af, x, o, e, shd_t=st, mode=mode)
                    got = engine.simd_ed_affine(batch, g, af, x, o, e, shd_threshold=st, mode=mode)
                    check(f"{name} {(g, af, x, o, e)} shd={st} mode={mode}", got, want, hb)


@pytest.mark.parametrize("n", COUNTS)
def test_shd_at_block_edges(asm, engine, oracle, pools, n):
    for name, hb, batch in batches(asm, engine, pools, n):
        for max_error in (0, 1, 16):
            check(f"{name} e={max_error}", engine.shd_filter(batch, max_error), oracle.shd(hb, max_error), hb)


def test_stale_tails_meet_the_clip_at_a_block_edge(asm, engine, oracle, pools):
    """GREEDY_SEQUENTIAL packing keeps the reference's stale buffer tails beyond each string's end: no filter may see them."""
    for name, hb, batch in batches(asm, engine, pools, max(COUNTS), asm.GREEDY_SEQUENTIAL):
        for t in (8, 9):
            want, _, _ = oracle.simd_ed(hb, t, True, asm.FILTER_CLEAN, (0, 0, 0))
            check(f"{name} simd_ed T={t}", engine.simd_ed(batch, t, True, asm.FILTER_CLEAN), want, hb)
        for st in (None, 3):
            want, _ = oracle.simd_ed_affine(hb, 6, 80, 2, 3, 1, shd_t=st)
            check(f"{name} affine shd={st}", engine.simd_ed_affine(batch, 6, 80, 2, 3, 1, shd_threshold=st), want, hb)
        check(f"{name} shd", engine.shd_filter(batch, 5), oracle.shd(hb, 5), hb)
