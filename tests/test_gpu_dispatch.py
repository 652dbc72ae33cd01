"""The arms of the pair aligners' dispatch (csrc/asm_plan.h decides, csrc/asm_align_host.h launches) that the other GPU modules do
not pin, bit for bit against the oracle.  The cases are the rows of tests/dispatch_cases.py, which name the kernel family and the
template constants each one reaches; tests/test_plan_host.py holds the dispatch to those names on the CPU.  The arms differ in template constants, not in scale:
every case is 1,061 pairs, two full 512-pair workgroups of the widest kernels and a ragged tail of 37.  One-granule cases use
the C2 configuration (100 bp); a length class is random_ragged_batch with its lengths inside the class, so that the batch's
longest string, which picks the kernel, is known."""
import numpy as np
import pytest

from tests import dispatch_cases as dc
from tests.oracle_binding import SIMD_WARM_STATE
from tests.util import check, engine_with, random_ragged_batch

pytestmark = pytest.mark.gpu

N = dc.N
ERR = 0.12  # random_ragged_batch's default: ceil(L * ERR) edits per pair, each of which may be an insertion


def class_batch(asm, lo, hi, n=N):
    """n ragged pairs whose longer string is in [lo, hi]: reads of lo .. L with L + ceil(L * ERR) <= hi, so that no reference
    grows beyond hi; the generator's fixed lengths put a read of L into the batch, and L >= lo for every class used here."""
    top = max(L for L in range(lo, hi + 1) if L + int(np.ceil(L * ERR)) <= hi)
    hb = random_ragged_batch(asm, 1000 + hi + n, n, lo, top, err=ERR)
    m, r = hb.lengths()
    assert lo <= max(m.max(), r.max()) <= hi
    return hb


@pytest.fixture(scope="module")
def inputs(asm):
    """Host batches by name, made on first use and shared by the cases: "c2", or a length class (lo, hi)."""
    made = {}

    def get(key):
        if key not in made:
            if key == "c2":
                cfg, _, _ = asm.workload("C2")
                made[key] = asm.generate_pairs(cfg, 53, N)
            else:
                made[key] = class_batch(asm, *key)
        return made[key]

    return get


@pytest.fixture(scope="module")
def engine_full_height(asm, engine):
    eng = engine_with(asm, "ASM_NW_BANDED")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_no_length_sort(asm, engine):
    eng = engine_with(asm, "ASM_NW_BYLEN")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_no_wave_kernels(asm, engine):
    eng = engine_with(asm, "ASM_WAVE")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_full_matrix(asm, engine):
    eng = engine_with(asm, "ASM_NW_WFA")
    yield eng
    eng.close()


@pytest.mark.parametrize("k", [r.k for r in dc.GREEDY_UNIT])
def test_greedy_unit_penalties(asm, engine, oracle, inputs, k):
    """The top of the thread-per-pair ladder (k <= 16), the first and the last wave-per-pair band (17, 31), both ends of the
    sixteen-threads-per-pair range (32, 39) and the first band beyond it."""
    hb = inputs("c2")
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.GREEDY, asm.Params.default(k=k))
    check(f"greedy k={k}", got, oracle.greedy(hb, k=k, mode=1), hb)


@pytest.mark.parametrize("k", [r.k for r in dc.GREEDY_GENERAL])
def test_greedy_general_penalties(asm, engine, oracle, inputs, k):
    """(2, 3, 1): greedy_persist_kernel<K, false>, greedy_wave_kernel<false>, the group kernel and the two-wavefront kernel."""
    hb = inputs("c2")
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.GREEDY, asm.Params.default(k=k, x=2, o=3, e=1))
    check(f"greedy k={k} (2,3,1)", got, oracle.greedy(hb, k, 2, 3, 1, mode=1), hb)


@pytest.mark.parametrize("k,lo,hi", sorted((r.k, *r.key) for r in dc.LEAP_UNIT_BY_CLASS))
def test_leap_unit_penalties_by_length_class(asm, engine, oracle, inputs, k, lo, hi):
    """k = 1, 5: leap_unit_kernel<K, 3..6>, one word count per class up to 384.  k = 6: four threads per pair on 6, 8, 12, 12 and
    16 words of 32 bits, ring entries of one byte up to 253 characters and of two beyond."""
    hb = inputs((lo, hi))
    (row,) = [r for r in dc.LEAP_UNIT_BY_CLASS if (r.k, r.key) == (k, (lo, hi))]
    if row.span:  # the part of the class in which the row's word count holds
        assert row.span[0] <= max(a.max() for a in hb.lengths()) <= row.span[1]
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k))
    check(f"leap k={k} {lo}-{hi}", got, oracle.leap(hb, k=k), hb)


@pytest.mark.parametrize("k", [r.k for r in dc.LEAP_UNIT_EDGE])
def test_leap_unit_penalties_last_thread_band_and_first_quad_band(asm, engine, oracle, inputs, k):
    hb = inputs("c2")
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k))
    check(f"leap k={k}", got, oracle.leap(hb, k=k), hb)


@pytest.mark.parametrize("k", [r.k for r in dc.LEAP_GENERAL])
def test_leap_general_penalties_every_thread_band(asm, engine, oracle, inputs, k):
    """(2, 3, 1) at 100 bp: leap_general_kernel<1..8, 2>."""
    hb = inputs("c2")
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k, x=2, o=3, e=1))
    check(f"leap k={k} (2,3,1)", got, oracle.leap(hb, k, 2, 3, 1), hb)


@pytest.mark.parametrize("k", [r.k for r in dc.LEAP_GENERAL_LONG])
def test_leap_general_penalties_beyond_one_granule(asm, engine, oracle, inputs, k):
    """(2, 3, 1) at 129-256: leap_general_kernel<5, 4>, and at k = 6 the four-threads-per-pair kernel."""
    hb = inputs((129, 256))
    got = engine.align(engine.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=k, x=2, o=3, e=1))
    check(f"leap k={k} (2,3,1) 129-256", got, oracle.leap(hb, k, 2, 3, 1), hb)


@pytest.fixture(scope="module")
def nw_inputs(asm, oracle):
    """Unit-cost NW inputs with the oracle's penalties.  A batch below 4096 pairs is one width class (that of its longest string)
    and is not `mixed`, so beside the ragged 1-512 batch of N pairs there is one batch of N per width class w4 = 1..4, and one
    ragged 1-512 batch of 4 N pairs, which the library splits into the four classes and marks `mixed`."""
    batches = {"ragged": class_batch(asm, 1, 512), "mixed": class_batch(asm, 1, 512, 4 * N)}
    for w4 in (1, 2, 3, 4):
        batches[f"w4={w4}"] = class_batch(asm, 128 * (w4 - 1) + 1, 128 * w4)
    return {name: (hb, oracle.nw(hb)) for name, hb in batches.items()}


@pytest.mark.parametrize("name", list(dc.NW_UNIT_BUCKETS))
def test_nw_unit_penalties_every_width_class(asm, engine, engine_full_height, engine_no_length_sort, nw_inputs, name):
    """nw_banded_kernel<4 w4, 32 | 64, false> (nw_banded2_kernel at w4 = 1) and, for the classes of the mixed batch, <.., true> on
    the default engine; nw_unit_kernel<2 w4> with ASM_NW_BANDED=0; the mixed batch without the length sort with ASM_NW_BYLEN=0."""
    hb, want = nw_inputs[name]
    if name == "mixed":
        m, n = hb.lengths()
        assert set(np.unique((np.maximum(np.maximum(m, n), 1) + 127) // 128)) == {1, 2, 3, 4}
    params = asm.Params.default()
    for label, eng in (("default", engine), ("ASM_NW_BANDED=0", engine_full_height), ("ASM_NW_BYLEN=0", engine_no_length_sort)):
        check(f"nw {name} {label}", eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.NW, params), want, hb)


@pytest.mark.parametrize("key", ["c2", (129, 256)])
@pytest.mark.parametrize("ed_t", sorted({t for t, _, _ in dc.SIMD_ED}))
def test_simd_ed_last_register_form_and_first_lds_form(asm, engine, oracle, inputs, ed_t, key):
    hb = inputs(key)
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    for shd in (False, True):
        want, _, want_pass = oracle.simd_ed(hb, ed_t, shd, asm.FILTER_CLEAN, SIMD_WARM_STATE)
        got = engine.simd_ed(batch, ed_t, shd, asm.FILTER_CLEAN, SIMD_WARM_STATE)
        check(f"simd_ed T={ed_t} shd={shd} {key}", got, want, hb)
        assert ((got >= 0) == (want_pass == 1)).all()


@pytest.mark.parametrize("key", [key for key, _ in dc.SIMD_ED_AFFINE])
def test_simd_ed_affine_quad_kernel_and_thread_per_pair_kernel(asm, engine, oracle, inputs, key):
    """A one-granule bucket goes to simd_ed_affine_quad_kernel, a longer one to simd_ed_affine_kernel<4>, the only thread-per-pair
    instantiation there is."""
    hb = inputs(key)
    want, _ = oracle.simd_ed_affine(hb, *dc.SIMD_ED_AFFINE_ARGS)
    check(f"simd_ed_affine {key}", engine.simd_ed_affine(engine.upload(hb, asm.GREEDY_CLEAN), *dc.SIMD_ED_AFFINE_ARGS), want, hb)


def test_workgroup_per_pair_kernels_without_wave_kernels(asm, engine_no_wave_kernels, oracle, inputs):
    """ASM_WAVE=0: greedy_wide_kernel at k = 20 and leap_wide_kernel<2> at k = 12, the kernels that take any band."""
    eng, hb = engine_no_wave_kernels, inputs("c2")
    (g,), (l,) = dc.GREEDY_WIDE, dc.LEAP_WIDE
    check(f"greedy k={g.k} ASM_WAVE=0", eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.GREEDY, asm.Params.default(k=g.k)),
          oracle.greedy(hb, k=g.k, mode=1), hb)
    check(f"leap k={l.k} ASM_WAVE=0", eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.LEAP, asm.Params.default(k=l.k)), oracle.leap(hb, k=l.k), hb)


def test_nw_general_penalties_wavefront_and_full_matrix(asm, engine, engine_full_matrix, oracle, inputs):
    """(2, 3, 1) at 100 bp: nw_wfa_kernel<7, 2>, nw_oct_kernel and nw_affine_kernel over the rest on the default engine;
    nw_affine_kernel<2, 128> over every pair with ASM_NW_WFA=0."""
    hb = inputs("c2")
    x, o, e = dc.NW_AFFINE[0].pen
    want = oracle.nw(hb, x, o, e)
    for label, eng in (("default", engine), ("ASM_NW_WFA=0", engine_full_matrix)):
        check(f"nw (2,3,1) {label}", eng.align(eng.upload(hb, asm.GREEDY_CLEAN), asm.NW, asm.Params.default(x=x, o=o, e=e)), want, hb)
