"""The structured corpus (tests/structured_cases.py: homopolymers, tandem repeats, shifted copies, rotations, block gaps, edits on
word edges, unrelated pairs, repeats with non-base bytes) through every pair-aligner kernel, bit for bit against the oracle —
which tests/test_structured_host.py pins to the compiled reference on these very batches.  The other GPU modules reach every
dispatch arm with uniform random text; this one reaches the arms with inputs on which every diagonal extends over several
words, carries run through whole columns, one gap has the band's width, and almost every cell ties.

Every case is one all_kinds_batch of 1,061 pairs (neighbouring lanes hold different kinds), made once per (class, band).  The
oracle's Greedy and filters apply the pack kernel's code-00 rule byte by byte; its LEAP and NW compare characters and are
given the batch as packed (structured_cases.as_packed).  No comparison here leaves a pair out."""
import numpy as np
import pytest

from tests import structured_cases as sc
from tests.oracle_binding import SIMD_WARM_STATE
from tests.test_gpu_dispatch import engine_full_height, engine_no_length_sort  # noqa: F401  (fixtures)
from tests.util import check, engine_with

pytestmark = pytest.mark.gpu

UNIT = (1, 1, 1)


@pytest.fixture(scope="module")
def batches(asm):
    """(batch, batch as packed) by (lo, hi, k, capped), made on first use.  capped: the lengths differ by at most k (Greedy)."""
    made = {}

    def get(lo, hi, k, capped=False, n=sc.N, kinds=sc.KINDS):
        key = (lo, hi, k, capped, n, kinds)
        if key not in made:
            hb = sc.all_kinds_batch(asm, lo, hi, k, n=n, max_diff=k if capped else None, kinds=kinds)
            made[key] = (hb, sc.as_packed(asm, hb))
        return made[key]

    return get


def _second_engine(asm, switch):
    eng = engine_with(asm, switch)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_slow_greedy(asm, engine):
    yield from _second_engine(asm, "ASM_GREEDY_FAST")


@pytest.fixture(scope="module")
def engine_no_wave(asm, engine):
    yield from _second_engine(asm, "ASM_WAVE")


@pytest.fixture(scope="module")
def engine_full_matrix(asm, engine):
    yield from _second_engine(asm, "ASM_NW_WFA")


def check_strings(name, got, want, hb):
    bad = [i for i in range(hb.n) if got[i] != want[i]]
    assert not bad, (f"{name}: {len(bad)}/{hb.n} differ; first {bad[:5]} got {got[bad[0]]} want {want[bad[0]]} "
                     f"kind {hb.kinds[bad[0]]} pair {hb.pair(bad[0])}")


# ---- Greedy ----
def greedy_case(asm, eng, oracle, hb, k, pen, label, cigars=False):
    """Global and semi-global, clean and sequential uploads (the sequential one resolves a pair's stale tail from what the pair
    before it — a homopolymer, a repeat — left in the buffers); with `cigars`, greedy_with_cigar CIGAR for CIGAR."""
    x, o, e = pen
    for mode in (asm.GREEDY_CLEAN, asm.GREEDY_SEQUENTIAL):
        batch = eng.upload(hb, mode)
        try:
            for semi in (False, True):
                params = asm.Params.default(k=k, x=x, o=o, e=e, alignment_type=asm.ALIGN_SEMI_GLOBAL if semi else asm.ALIGN_GLOBAL)
                want, want_cig = oracle.greedy(hb, k, x, o, e, mode=mode, cigars=True, semi=semi)
                name = f"greedy {label} k={k} {pen} mode={mode} semi={semi}"
                check(name, eng.align(batch, asm.GREEDY, params), want, hb)
                if cigars:
                    cost, cig, nops = eng.greedy_with_cigar(batch, params, cap=128)
                    check(name + " cigar cost", cost, want, hb)
                    assert int(nops.max()) <= 128
                    check_strings(name + " CIGAR", cig, want_cig, hb)
        finally:
            batch.free()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 12, 16, 17, 31, 32, 39, 40])
def test_greedy_unit_penalties(asm, engine, oracle, batches, k):
    """k <= 3: greedy_fast_kernel; 4 .. 16 the thread-per-pair ladder; 17, 31 a wave per pair; 32, 39 sixteen threads per pair;
    40 the two-wavefront kernel."""
    hb, _ = batches(100, 128, k, True)
    greedy_case(asm, engine, oracle, hb, k, UNIT, "default", cigars=k in (3, 12, 17, 32, 40))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_greedy_narrow_bands_on_the_fp64_kernel(asm, engine_slow_greedy, oracle, batches, k):
    hb, _ = batches(100, 128, k, True)
    greedy_case(asm, engine_slow_greedy, oracle, hb, k, UNIT, "ASM_GREEDY_FAST=0", cigars=k == 3)


@pytest.mark.parametrize("k", [3, 16, 17, 32, 39, 40])
def test_greedy_general_penalties(asm, engine, oracle, batches, k):
    hb, _ = batches(100, 128, k, True)
    greedy_case(asm, engine, oracle, hb, k, (2, 3, 1), "default", cigars=k in (3, 17, 32, 40))


@pytest.mark.parametrize("k", [17, 40])
def test_greedy_workgroup_per_pair_fallback(asm, engine_no_wave, oracle, batches, k):
    hb, _ = batches(100, 128, k, True)
    greedy_case(asm, engine_no_wave, oracle, hb, k, UNIT, "ASM_WAVE=0", cigars=k == 17)
    greedy_case(asm, engine_no_wave, oracle, hb, k, (2, 3, 1), "ASM_WAVE=0", cigars=True)


# ---- LEAP ----
LEAP_SHORT = (31, 128)


@pytest.mark.parametrize("k", [1, 3, 5, 6, 10, 11, 30])
def test_leap_unit_penalties_one_granule(asm, engine, oracle, batches, k):
    hb, seen = batches(*LEAP_SHORT, k)
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k))
    check(f"leap k={k}", got, oracle.leap(seen, k=k), hb)


@pytest.mark.parametrize("k,lo,hi", [(k, lo, hi) for k in (1, 5, 6) for lo, hi in ((129, 192), (193, 256))] +
                         [(6, 257, 320), (6, 321, 384), (6, 385, 512)])
def test_leap_unit_penalties_by_length_class(asm, engine, oracle, batches, k, lo, hi):
    """Up to 256 every string is within LEAP's length; beyond, the oracle's LEAP is compared on every pair, as
    test_gpu_dispatch.py compares those classes."""
    hb, seen = batches(lo, hi, k)
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k))
    check(f"leap k={k} {lo}-{hi}", got, oracle.leap(seen, k=k), hb)


@pytest.mark.parametrize("pen", [(2, 3, 1), (4, 6, 2)])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_leap_general_penalties_every_thread_band(asm, engine, oracle, batches, k, pen):
    hb, seen = batches(*LEAP_SHORT, k)
    x, o, e = pen
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k, x=x, o=o, e=e))
    check(f"leap k={k} {pen}", got, oracle.leap(seen, k, x, o, e), hb)


@pytest.mark.parametrize("pen", [(2, 3, 1), (4, 6, 2)])
@pytest.mark.parametrize("k", [5, 6])
def test_leap_general_penalties_beyond_one_granule(asm, engine, oracle, batches, k, pen):
    hb, seen = batches(129, 256, k)
    x, o, e = pen
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k, x=x, o=o, e=e))
    check(f"leap k={k} {pen} 129-256", got, oracle.leap(seen, k, x, o, e), hb)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("k", [3, 10])
def test_leap_ed_modes(asm, engine, oracle, batches, k, mode):
    hb, seen = batches(*LEAP_SHORT, k)
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k, leap_mode=mode))
    check(f"leap k={k} ED mode {mode}", got, oracle.leap(seen, k, mode=mode), hb)


@pytest.mark.parametrize("k,lo,hi,pen", [(3, 31, 128, UNIT), (10, 31, 128, UNIT), (6, 129, 256, UNIT), (12, 31, 128, (2, 3, 1))])
def test_leap_scheduled_by_a_work_hint(asm, engine, oracle, batches, k, lo, hi, pen):
    """align_hinted_async with the NW penalties and with junk: sorting by work puts a homopolymer's long extension next to an
    unrelated pair's short one."""
    hb, seen = batches(lo, hi, k)
    x, o, e = pen
    params = asm.Params.default(k=k, x=x, o=o, e=e)
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    want = oracle.leap(seen, k, x, o, e)
    d_hint, d_leap = engine.malloc(4 * hb.n), engine.malloc(4 * hb.n)
    try:
        engine.align_async(batch, asm.NW, params, d_hint)
        engine.align_hinted_async(batch, asm.LEAP, params, d_hint, d_leap)
        check(f"leap k={k} hinted by NW", engine.to_host(d_leap, hb.n), want, hb)
        junk = ((np.arange(hb.n, dtype=np.int64) * 7919) % 300 - 50).astype(np.int32)
        engine._chk(engine.lib.asm_memcpy_h2d(engine.h, d_hint, junk.ctypes.data, 4 * hb.n))
        engine.memset_async(d_leap, 0xff, 4 * hb.n)
        engine.align_hinted_async(batch, asm.LEAP, params, d_hint, d_leap)
        check(f"leap k={k} hinted by junk", engine.to_host(d_leap, hb.n), want, hb)
    finally:
        engine.free(d_hint), engine.free(d_leap)


# ---- NW ----
@pytest.fixture(scope="module")
def nw_inputs(asm, oracle, batches):
    """One batch per width class w4 = 1..4 (w4 = 1 is nw_banded2_kernel: neighbouring pairs, of different kinds, are the two
    halves of one thread) and a 1-512 batch of 4 x 1,061 pairs, which the library splits into the four classes and marks mixed."""
    out = {}
    for name, key in (("w4=1", (31, 128, 6)), ("w4=2", (129, 256, 6)), ("w4=3", (257, 384, 6)), ("w4=4", (385, 512, 6)),
                      ("mixed", (31, 512, 6, False, 4 * sc.N))):
        hb, seen = batches(*key)
        out[name] = (hb, oracle.nw(seen))
    return out


@pytest.mark.parametrize("name", ["w4=1", "w4=2", "w4=3", "w4=4", "mixed"])
def test_nw_unit_penalties_every_width_class(asm, engine, engine_full_height, engine_no_length_sort, nw_inputs, name):
    hb, want = nw_inputs[name]
    m, n = hb.lengths()
    if name == "mixed":
        assert set(np.unique((np.maximum(m, n) + 127) // 128)) == {1, 2, 3, 4}
    else:
        assert (hb.kinds[0:-1:2] != hb.kinds[1::2]).all()
    params = asm.Params.default()
    for label, eng in (("default", engine), ("ASM_NW_BANDED=0", engine_full_height), ("ASM_NW_BYLEN=0", engine_no_length_sort)):
        check(f"nw {name} {label}", eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.NW, params), want, hb)


NW_WFA_REACH = 15  # csrc/asm_kernels.h: the widest banded affine pass (|d| <= 15 up to 128 bases, 7 beyond)


MIXES = {"all kinds": sc.KINDS, "far-heavy": sc.FAR_HEAVY}  # far-heavy: three turns in eight are unrelated pairs
FALLBACK_SHARE = 0.3                                        # the bar test_gpu_parity.py sets for its noisy coverage cases


@pytest.mark.parametrize("mix", sorted(MIXES))
@pytest.mark.parametrize("lo,hi", [(31, 128), (129, 256)])
@pytest.mark.parametrize("pen", [(2, 3, 1), (4, 6, 2), (1, 1, 0), (0, 2, 1)])
def test_nw_affine(asm, engine, engine_full_matrix, oracle, batches, pen, lo, hi, mix):
    """nw_wfa_kernel, nw_oct_kernel and nw_affine_kernel behind them, and the full matrix alone (ASM_NW_WFA=0: every pair, the
    repeats and block gaps included).  A banded pass proves a result s only when s <= 2 o + (2 K - |n - m|) e: the pairs above
    that bound at the widest K were answered by the full-matrix kernel behind the banded passes, and the far-heavy batch must
    hold more than 0.3 of them.  With a zero penalty the dispatch (asm_capi.hip, `positive`) sends the whole batch to the full
    matrix at once, so there is no share to assert."""
    hb, seen = batches(lo, hi, 16, kinds=MIXES[mix])
    x, o, e = pen
    want = oracle.nw(seen, x, o, e)
    if min(pen) >= 1:
        share = float((want > 2 * o + 2 * NW_WFA_REACH * e).mean())
        print(f"affine NW {pen} {lo}-{hi} {mix}: {share:.3f} of the pairs beyond the banded passes")
        assert mix != "far-heavy" or share > FALLBACK_SHARE, share
    params = asm.Params.default(x=x, o=o, e=e)
    for label, eng in (("default", engine), ("ASM_NW_WFA=0", engine_full_matrix)):
        check(f"nw {pen} {lo}-{hi} {mix} {label}", eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.NW, params), want, hb)


# ---- traceback and coverage ----
@pytest.mark.parametrize("mix,k", [("all kinds", 3), ("far-heavy", 16)])
@pytest.mark.parametrize("window,pen", [(32, UNIT), (64, UNIT), (64, (2, 3, 1)), (64, (1, 1, 0))])
def test_coverage_and_nw_traceback(asm, engine, oracle, batches, window, pen, mix, k):
    """In a repeat almost every cell ties, and the traceback's tie-break decides the CIGAR: NW CIGAR for CIGAR, the cover verdict
    pair for pair, nothing undetermined.  With unit penalties, what the windowed pass cannot answer (distance above
    window / 2 - 3) goes through the full matrix with stored directions: more than 0.3 of the far-heavy batch (unrelated pairs,
    and at window 32 the block gaps and shifts of 14 to 17).  Other penalties take the full Gotoh matrix for every pair, so
    there is no share to assert."""
    hb, seen = batches(100, 128, k, True, kinds=MIXES[mix])
    x, o, e = pen
    params = asm.Params.default(k=k, x=x, o=o, e=e)
    got = engine.coverage(engine.upload(hb, asm.GREEDY_CLEAN), params, window=window, cap=255, want_nw_cigars=True)
    gcost, gcig = oracle.greedy(hb, k, x, o, e, mode=1, cigars=True)
    pen_nw, ncig = oracle.nw_cigar(seen, x, o, e)
    want = oracle.coverage(seen, gcig, 1, ncig, 3)
    if pen == UNIT:
        share = float((pen_nw > window // 2 - 3).mean())
        print(f"coverage window {window} {mix}: {share:.3f} of the pairs beyond the windowed pass")
        assert mix != "far-heavy" or share > FALLBACK_SHARE, share
    assert got["undetermined"] == 0 and not (got["cover"] == 2).any()
    assert got["covered"] == int((got["cover"] == 1).sum())
    check("coverage greedy cost", got["greedy_cost"], gcost, hb)
    check_strings(f"nw CIGAR window {window} {pen} {mix}", got["nw_cigars"], ncig, hb)
    check(f"cover window {window} {pen} {mix}", got["cover"], want, hb)


# ---- filters ----
FILTER_CLASSES = [(31, 128), (129, 256)]


@pytest.mark.parametrize("lo,hi", FILTER_CLASSES)
@pytest.mark.parametrize("ed_t", [1, 3, 8, 9, 16, 25])
def test_simd_ed(asm, engine, oracle, batches, ed_t, lo, hi):
    hb, _ = batches(lo, hi, 3)
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    for shd in ((False, True) if ed_t <= 16 else (False,)):
        for mode in (asm.FILTER_CLEAN, asm.FILTER_SEQUENTIAL):  # sequential: each pair from the state the pair before left
            want, _, want_pass = oracle.simd_ed(hb, ed_t, shd, mode, SIMD_WARM_STATE)
            got = engine.simd_ed(batch, ed_t, shd, mode, SIMD_WARM_STATE)
            check(f"simd_ed T={ed_t} shd={shd} mode={mode} {lo}-{hi}", got, want, hb)
            assert ((got >= 0) == (want_pass == 1)).all()


@pytest.mark.parametrize("lo,hi", FILTER_CLASSES)
def test_shd(asm, engine, oracle, batches, lo, hi):
    hb, _ = batches(lo, hi, 3)
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    passed = []
    for max_error in (0, 1, 3, 7, 16):
        want = oracle.shd(hb, max_error)
        check(f"shd e={max_error} {lo}-{hi}", engine.shd_filter(batch, max_error), want, hb)
        passed.append(float(want.mean()))
    assert 0 < passed[0] < passed[-1] < 1  # rejection at every threshold, and never of everything


@pytest.mark.parametrize("lo,hi", FILTER_CLASSES)
@pytest.mark.parametrize("setting", [(3, 60, 2, 3, 1), (12, 120, 4, 6, 2)])
def test_simd_ed_affine(asm, engine, oracle, batches, setting, lo, hi):
    hb, _ = batches(lo, hi, 3)
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    for shd_t in (None, 2):
        for mode in (0, 1, 2, 3):
            want, _ = oracle.simd_ed_affine(hb, *setting, shd_t=shd_t, mode=mode)
            got = engine.simd_ed_affine(batch, *setting, shd_threshold=shd_t, mode=mode)
            check(f"simd_ed_affine {setting} shd_t={shd_t} mode={mode} {lo}-{hi}", got, want, hb)


# ---- the whole step ----
def test_the_whole_step(asm, engine, oracle, batches):
    """run_benchmark_async in stream order (repack = True) and as overlapped calls (repack = 3, two sets of outputs, one join):
    the three aligners' outputs and the four accuracy counters, the latter against counts made from the oracle's answers."""
    k = 3
    hb, seen = batches(100, 128, k, True)
    n = hb.n
    params = asm.Params.default(k=k)
    nw, leap, greedy = oracle.nw(seen), oracle.leap(seen, k), oracle.greedy(hb, k, mode=1)
    counts = [n, n, int((leap == nw).sum()), int((greedy == nw).sum())]
    assert 0 < counts[2] < n and 0 < counts[3] < n
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    sets = [[engine.malloc(4 * n) for _ in range(3)] for _ in range(2)]
    d_cnt = engine.malloc(32)
    try:
        engine.memset_async(d_cnt, 0, 32)
        engine.run_benchmark_async(batch, params, *sets[0], d_cnt, repack=True)
        for name, d, want in zip(("nw", "leap", "greedy"), sets[0], (nw, leap, greedy)):
            check(f"step {name}", engine.to_host(d, n), want, hb)
        assert engine.to_host(d_cnt, 4, np.uint64).tolist() == counts
        for s in sets:
            for d in s:
                engine.memset_async(d, 0xff, 4 * n)
        engine.memset_async(d_cnt, 0, 32)
        calls = 5
        for c in range(calls):
            engine.run_benchmark_async(batch, params, *sets[c & 1], d_cnt, repack=3)
        engine.pipeline_join_async()
        for s in sets:
            for name, d, want in zip(("nw", "leap", "greedy"), s, (nw, leap, greedy)):
                check(f"overlapped step {name}", engine.to_host(d, n), want, hb)
        assert engine.to_host(d_cnt, 4, np.uint64).tolist() == [calls * c for c in counts]
    finally:
        engine.synchronize()
        for d in sets[0] + sets[1] + [d_cnt]:
            engine.free(d)
