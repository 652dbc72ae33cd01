"""The cases of tests/test_gpu_dispatch.py, each with the kernel family and the template constants it is there to reach
(csrc/asm_plan.h: AlignPlan's fields by name).  tests/test_plan_host.py asserts the plan of every row on the CPU, so a threshold
edit that reroutes a case fails there; test_gpu_dispatch.py runs the same rows bit for bit against the oracle.

A row's input is "c2" (the C2 configuration: 100 bp, one granule, at most 128 characters) or a length class (lo, hi): a ragged
batch whose longest string lies in [lo, hi], so the plan is asserted at both ends of the class and a row names only what the
whole class shares; `span` narrows the lengths where a constant holds for part of a class only, and the GPU test asserts
that its batch's longest string lies there.  `off` is the one switch a row turns off (an environment variable of the library), or None."""
from collections import namedtuple

N = 1061  # two full 512-thread workgroups of the widest kernel plus a ragged tail of 37

Row = namedtuple("Row", "aligner k pen key off family want span")
SWITCH_BITS = {"ASM_WAVE": 1, "ASM_NW_BANDED": 2, "ASM_NW_BYLEN": 4, "ASM_NW_PAIR2": 8, "ASM_NW_WFA": 16, "ASM_GREEDY_FAST": 32,
               "ASM_LEAP_HINT": 64, "ASM_LEAP_SORT": 128}  # the order of AlignSwitches
UNIT, GENERAL = (1, 1, 1), (2, 3, 1)


def _row(aligner, band, pen, key, family, off=None, span=None, **want):
    return Row(aligner, band, pen, key, off, family, want, span)


# the top of the thread-per-pair ladder (k <= 16), the first and the last wave-per-pair band (17, 31), both ends of the
# sixteen-threads-per-pair range (32, 39) and the first band beyond it
GREEDY_UNIT = ([_row("greedy", 3, UNIT, "c2", "GREEDY_FAST", k=3)] +
               [_row("greedy", k, UNIT, "c2", "GREEDY_PERSIST", k=k, unit=1) for k in (12, 13, 14, 15, 16)] +
               [_row("greedy", k, UNIT, "c2", "GREEDY_WAVE", unit=1) for k in (17, 31)] +
               [_row("greedy", k, UNIT, "c2", "GREEDY_GROUP") for k in (32, 39)] + [_row("greedy", 40, UNIT, "c2", "GREEDY_WAVE2")])
# (2, 3, 1): greedy_persist_kernel<K, false>, greedy_wave_kernel<false>, the group kernel and the two-wavefront kernel
GREEDY_GENERAL = [_row("greedy", 16, GENERAL, "c2", "GREEDY_PERSIST", k=16, unit=0), _row("greedy", 17, GENERAL, "c2", "GREEDY_WAVE", unit=0),
                  _row("greedy", 32, GENERAL, "c2", "GREEDY_GROUP"), _row("greedy", 39, GENERAL, "c2", "GREEDY_GROUP"),
                  _row("greedy", 40, GENERAL, "c2", "GREEDY_WAVE2")]
# the workgroup-per-pair kernel: what ASM_WAVE=0 leaves of the bands above 16
GREEDY_WIDE = [_row("greedy", 20, UNIT, "c2", "GREEDY_WIDE", off="ASM_WAVE")]

LEAP_CLASSES = [(129, 192), (193, 256), (257, 320), (321, 384)]
# k = 1, 5: leap_unit_kernel<K, 3..6>, one word count per class up to 384.  k = 6: four threads per pair on 6, 8, 12, 12 and 16
# words of 32 bits, ring entries of one byte up to 253 characters and of two beyond
LEAP_UNIT_BY_CLASS = ([_row("leap", k, UNIT, c, "LEAP_UNIT", k=k, words=3 + q, hinted=0) for k in (1, 5) for q, c in enumerate(LEAP_CLASSES)] +
                      [_row("leap", 6, UNIT, (129, 192), "LEAP_QUAD", span=(161, 192), words=6, entry=1, unit=1), _row("leap", 6, UNIT, (193, 256), "LEAP_QUAD", words=8, unit=1),
                       _row("leap", 6, UNIT, (257, 320), "LEAP_QUAD", words=12, entry=2, unit=1),
                       _row("leap", 6, UNIT, (321, 384), "LEAP_QUAD", words=12, entry=2, unit=1),
                       _row("leap", 6, UNIT, (385, 512), "LEAP_QUAD", words=16, entry=2, unit=1)])
# the last thread-per-pair band of one granule and the first four-threads-per-pair band
LEAP_UNIT_EDGE = [_row("leap", 10, UNIT, "c2", "LEAP_UNIT", k=10, words=2), _row("leap", 11, UNIT, "c2", "LEAP_QUAD", words=4, entry=1, unit=1)]
# (2, 3, 1) at 100 bp: leap_general_kernel<1..8, 2>
LEAP_GENERAL = [_row("leap", k, GENERAL, "c2", "LEAP_GENERAL", k=k, words=2) for k in range(1, 9)]
# (2, 3, 1) at 129-256: leap_general_kernel<5, 4>, and at k = 6 the four-threads-per-pair kernel
LEAP_GENERAL_LONG = [_row("leap", 5, GENERAL, (129, 256), "LEAP_GENERAL", k=5, words=4), _row("leap", 6, GENERAL, (129, 256), "LEAP_QUAD", unit=0)]
# the workgroup-per-pair kernel: what ASM_WAVE=0 leaves of the bands above the thread-per-pair kernels
LEAP_WIDE = [_row("leap", 12, UNIT, "c2", "LEAP_WIDE", off="ASM_WAVE", words=2)]

# Unit-cost NW by batch name (test_gpu_dispatch.nw_inputs): (w4, mixed) of the buckets a batch is made of, and the family under the
# default switches, with ASM_NW_BANDED=0 and with ASM_NW_BYLEN=0
NW_UNIT_BUCKETS = {"ragged": [(4, False)], "w4=1": [(1, False)], "w4=2": [(2, False)], "w4=3": [(3, False)], "w4=4": [(4, False)],
                   "mixed": [(1, True), (2, True), (3, True), (4, True)]}


def nw_unit_want(w4, mixed, off):
    if off == "ASM_NW_BANDED":
        return "NW_UNIT_FULL", dict(words=2 * w4)
    if mixed and off != "ASM_NW_BYLEN":
        return "NW_BANDED_BYLEN", dict(words=4 * w4, window=32 if w4 == 1 else 64)
    if w4 == 1:
        return "NW_PAIR2", dict(words=4)
    return "NW_BANDED", dict(words=4 * w4, window=64)


# (2, 3, 1): the banded wavefront passes, and the full matrix over every pair with ASM_NW_WFA=0
NW_AFFINE = [_row("nw", 0, GENERAL, "c2", "NW_WFA", k=7, words=2, entry=1, oct_entry=1),
             _row("nw", 0, GENERAL, "c2", "NW_AFFINE_FULL", off="ASM_NW_WFA", words=2)]

ALIGNER_ROWS = (GREEDY_UNIT + GREEDY_GENERAL + GREEDY_WIDE + LEAP_UNIT_BY_CLASS + LEAP_UNIT_EDGE + LEAP_GENERAL + LEAP_GENERAL_LONG + LEAP_WIDE +
                NW_AFFINE)

# SIMD_ED: the last register form and the first LDS form, on two and on four words
SIMD_ED = [(ed_t, key, dict(reg_t=ed_t if ed_t <= 8 else 0, words=2 if key == "c2" else 4)) for key in ("c2", (129, 256)) for ed_t in (8, 9)]
# a one-granule bucket goes to simd_ed_affine_quad_kernel, a longer one to simd_ed_affine_kernel<4>, the only thread-per-pair
# instantiation there is: (gap threshold, affine threshold, x, o, e)
SIMD_ED_AFFINE_ARGS = (3, 60, 2, 3, 1)
SIMD_ED_AFFINE = [("c2", dict(quad=1, refused=0)), ((129, 256), dict(quad=0, refused=0))]
