"""The pair aligners' and the filters' dispatch (csrc/asm_plan.h) on the CPU: host/plan_host_check.cpp, built under ASan + UBSan, prints
the plan of every query of a grid, and every plan must equal what `parent_*` below gives.  Those functions are a transcription of the
dispatch as it stood before asm_plan.h existed: align_bucket, the launch_* functions, launch_simd_ed_events and simd_ed_affine_launch
of csrc/asm_capi.hip and the launchers that stood beside the kernels in asm_wave.h, asm_wide.h and asm_group.h, condition by condition
in their order.  They are never derived from asm_plan.h; a deliberate change of the dispatch changes them in the same commit.

Over the same grid: every plan's template constants are ones the launchers instantiate, LDS stays within what the dispatch compares
against (64 KiB, 150 KiB for the affine filter), a ring entry is one byte only where every stored position + 2 fits, and grid x block
covers the bucket.  And every row of tests/dispatch_cases.py reaches the kernel family and the constants it names.  No GPU needed."""
import itertools
import os
import subprocess

import pytest

from tests import dispatch_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
NW, LEAP, GREEDY = 0, 1, 2
ALIGNER = {"nw": NW, "leap": LEAP, "greedy": GREEDY}
ALL_ON = 255
SWITCH_SETS = [ALL_ON] + [ALL_ON & ~bit for bit in dc.SWITCH_BITS.values()]  # all on, and each switch off alone
MAXLENS = [1, 31, 32, 63, 64, 65, 127, 128, 129, 192, 193, 253, 254, 256, 257, 320, 321, 384, 385, 512]  # 513 is beyond ASM_MAX_LENGTH
N = dc.N
KIB = 1024
# limits of the kernels (csrc/asm_limits.h)
BLOCK, G3_THREADS, GEN_THREADS, QUAD_PAIRS, QUAD_THREADS, HINT_PAIRS, SORT_PAIRS, OCT_PAIRS, WIDE_THREADS = 256, 512, 128, 16, 64, 256, 256, 8, 128
EXACT, PER_CU, OCCUPANCY = 0, 1, 2


def san_flags():
    """SAN_FLAGS of oracle/Makefile"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        for line in fh:
            if line.startswith("SAN_FLAGS :="):
                return line.split(":=", 1)[1].split()
    raise AssertionError("oracle/Makefile has no SAN_FLAGS")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """queries -> the program's output lines"""
    exe = str(tmp_path_factory.mktemp("plan_check") / "plan_host_check_asan")
    src = os.path.join(PKG, "host", "plan_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(queries):
        p = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = p.stdout.splitlines()
        assert len(lines) == len(queries)
        return lines

    return run


# ---- the dispatch before asm_plan.h ---------------------------------------------------------------------------------------------------
def blocks(n, per):
    return (n + per - 1) // per


def first_of(v, ascending):
    """with_const_of: the first listed C with v <= C; a value above the last takes the last"""
    return next((c for c in ascending if v <= c), ascending[-1])


def pow2_above(v):
    g = 2
    while g <= v:
        g <<= 1
    return g


def rings_pow2(x, o, e):
    return pow2_above(max(x, o)), pow2_above(e)


def rings_exact(x, o, e):
    return max(x, o) + 1, e + 1


def ring_bytes(rg, rows, columns, elem):
    return ((rg[0] + 2 * rg[1]) * rows * columns * elem + 3) & ~3


def quad_lds(rg, pairs, w32, half_band, elem):
    return pairs * (4 * (w32 + 1) + 1) * 4 + ring_bytes(rg, 2 * half_band + 3, pairs, elem)


def plan(family, block, grid, **kw):
    d = dict(family=family, k=0, words=0, window=0, entry=0, gm=0, gi=0, unit=0, hinted=0, waves=0, sort=0, sort_div=0, oct_entry=0, oct_lds=0,
             block=block, grid=grid, grid_rule=EXACT, grid_arg=0, lds=0)
    assert set(kw) <= set(d)
    d.update(kw)
    return d


def parent_greedy(k, x, o, e, semi, n, sw):
    wave, fast = bool(sw & 1), bool(sw & 32)
    unit = (x, o, e) == (1, 1, 1)
    if 1 <= k <= 16:  # launch_greedy<K>
        if k <= 3 and fast and unit and not semi:  # ... and g3_prepare, which the plan leaves to the launcher
            return plan("GREEDY_FAST", G3_THREADS, blocks(n, G3_THREADS), k=k, unit=1, grid_rule=PER_CU, grid_arg=1,
                        lds=129 * 32 * 8 + (2 * k + 1) * G3_THREADS * 16 + 4096 * 2)
        return plan("GREEDY_PERSIST", BLOCK, blocks(n, BLOCK), k=k, unit=int(unit and not semi), grid_rule=OCCUPANCY, grid_arg=0)
    if wave and 32 <= k <= 39 and o + 110 * e < 16000:
        return plan("GREEDY_GROUP", BLOCK, blocks(n * 16, BLOCK), grid_rule=OCCUPANCY, grid_arg=4)
    if k <= 31 and wave and unit and not semi:
        return plan("GREEDY_WAVE", BLOCK, blocks(n, 4), unit=1, grid_rule=OCCUPANCY, grid_arg=8)
    if k <= 31 and wave and o + 62 * e < 16000:
        return plan("GREEDY_WAVE", BLOCK, blocks(n, 4), unit=0, grid_rule=OCCUPANCY, grid_arg=8)
    if wave and o + 100 * e < 16000:
        return plan("GREEDY_WAVE2", 128, n, grid_rule=PER_CU, grid_arg=16)
    return plan("GREEDY_WIDE", WIDE_THREADS, min(n, 256 * 32))


def parent_leap_wide(n, w4):
    maxw = 2 * w4
    return plan("LEAP_WIDE", WIDE_THREADS, min(n, 256 * 32), words=2 if maxw <= 2 else 4 if maxw <= 4 else 8)


def parent_leap(k, x, o, e, mode, n, maxlen, w4, hint, sw):
    wave, leap_hint, leap_sort = bool(sw & 1), bool(sw & 64), bool(sw & 128)
    unit = (x, o, e) == (1, 1, 1)
    quad_rg = (2, 0) if unit else rings_pow2(x, o, e)
    if mode != 0:
        return parent_leap_wide(n, w4)
    if unit and k >= 1 and ((k <= 5 and maxlen <= 384) or (k <= 10 and maxlen <= 128)):
        wmax = 6 if k <= 5 else 2
        assert maxlen <= 64 * wmax  # the guard launch_leap_unit carried
        hinted = hint and leap_hint
        return plan("LEAP_UNIT", BLOCK, blocks(n, HINT_PAIRS if hinted else BLOCK), k=k, words=min(max((maxlen + 63) // 64, 2), wmax), hinted=int(hinted))
    if (not unit and k >= 1 and ((k <= 5 and maxlen <= 256) or (k <= 8 and maxlen <= 128)) and wave and
            ring_bytes(rings_pow2(x, o, e), 2 * k + 1, GEN_THREADS, 2) <= 64 * KIB):
        gmax = 2 if k <= 5 else 1
        assert maxlen <= 128 * gmax  # the guard launch_leap_general carried
        rg = rings_pow2(x, o, e)
        entry = 1 if maxlen + 4 <= 255 and ring_bytes(rg, 2 * k + 1, GEN_THREADS, 2) > 20 * KIB else 2
        return plan("LEAP_GENERAL", GEN_THREADS, blocks(n, GEN_THREADS), k=k, words=2 * min(max((maxlen + 127) // 128, 1), gmax), entry=entry, gm=rg[0],
                    gi=rg[1], lds=ring_bytes(rg, 2 * k + 1, GEN_THREADS, entry))
    en = 1 if maxlen + 2 <= 255 else 2
    if wave and maxlen <= 512 and quad_lds(quad_rg, QUAD_PAIRS, (maxlen + 31) // 32, k, en) <= 64 * KIB:
        qhint = hint and leap_hint
        sort = bool(qhint and leap_sort and (maxlen > 128 or not unit))
        w32 = first_of((maxlen + 31) // 32, (4, 5, 6, 8, 12, 16))
        lds1 = quad_lds(quad_rg, QUAD_PAIRS, w32, k, en)  # launch_leap_quad<W32, EnT>
        waves = 4 if qhint and not sort and 4 * lds1 + 512 <= 64 * KIB else 1
        return plan("LEAP_QUAD", waves * QUAD_THREADS, blocks(n, waves * QUAD_PAIRS), words=w32, entry=en, gm=quad_rg[0], gi=quad_rg[1], unit=int(unit),
                    hinted=int(qhint), waves=waves, sort=int(sort), sort_div=1 if unit else min(e, x), lds=waves * lds1)
    return parent_leap_wide(n, w4)


def parent_nw(x, o, e, n, maxlen, w4, mixed, sw):
    banded, bylen, pair2, wfa = bool(sw & 2), bool(sw & 4), bool(sw & 8), bool(sw & 16)
    if (x, o, e) == (1, 1, 1):
        w = min(max(w4, 1), 4)  # with_const<1, 4>(b.w4, ...)
        window = 32 if w == 1 else 64
        if not banded:
            return plan("NW_UNIT_FULL", BLOCK, blocks(n, BLOCK), words=2 * w)
        if mixed and bylen:
            return plan("NW_BANDED_BYLEN", BLOCK, blocks(n, SORT_PAIRS), words=4 * w, window=window)
        if w4 == 1 and pair2:
            return plan("NW_PAIR2", BLOCK, blocks(n, 2 * BLOCK), words=4, window=16)
        return plan("NW_BANDED", BLOCK, blocks(n, BLOCK), words=4 * w, window=window)
    positive = x >= 1 and o >= 1 and e >= 1
    rg = rings_exact(x, o, e)
    if wfa and positive and maxlen <= 256 and ring_bytes(rg, 15, GEN_THREADS, 2) <= 64 * KIB:
        w64 = first_of((maxlen + 63) // 64, (2, 4))
        entry = 1 if w64 == 2 else 2
        en = 1 if maxlen + 2 <= 255 else 2
        oct_lds = quad_lds(rg, OCT_PAIRS, 2 * w64, 15, en)
        oct_on = oct_lds <= 64 * KIB
        return plan("NW_WFA", GEN_THREADS, blocks(n, GEN_THREADS), k=7, words=w64, entry=entry, gm=rg[0], gi=rg[1], lds=ring_bytes(rg, 15, GEN_THREADS, entry),
                    oct_entry=en if oct_on else 0, oct_lds=oct_lds if oct_on else 0)
    return plan("NW_AFFINE_FULL", 64, blocks(n, 64), words=2 if maxlen <= 128 else 4 if maxlen <= 256 else 8)


def parent_simd_ed(T, ed_mode, n, maxlen):
    words = first_of((maxlen + 63) // 64, (2, 4))
    if T <= 8 and ed_mode not in (1, 2):
        return dict(reg_t=T, words=words, block=128, grid=blocks(n, 128), lds=0)
    return dict(reg_t=0, words=words, block=128, grid=blocks(n, 128), lds=2 * (2 * T + 3) * 128 * 2)


def parent_simd_ed_affine(gap, x, o, e, n, maxlen):
    rg = rings_pow2(x, o, e)
    rows, threads = 2 * gap + 3, 64
    while threads > 16 and ring_bytes(rg, rows, threads, 2) > 150 * KIB:
        threads >>= 1
    lds = ring_bytes(rg, rows, threads, 2)
    d = dict(refused=int(lds > 150 * KIB), quad=int(maxlen <= 128), gm=rg[0], gi=rg[1])
    if maxlen <= 128:
        d.update(block=64, grid=blocks(n, 16), lds=quad_lds(rg, 16, 5, gap, 1))
    else:
        d.update(block=threads, grid=blocks(n, threads), lds=lds)
    return d


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
GREEDY_PENALTIES = [(1, 1, 1), (2, 3, 1), (1, 2, 2), (15, 15, 1), (4, 6, 2), (0, 0, 0)] + [
    (1, 16000 - m * e - d, e) for m in (62, 100, 110) for e in (1, 7) for d in (0, 1)]  # both sides of o + 62e, o + 100e, o + 110e = 16000
LEAP_PENALTIES = [(1, 1, 1), (2, 3, 1), (1, 2, 2), (15, 15, 1), (4, 6, 2), (15, 15, 15)]
NW_PENALTIES = [(1, 1, 1), (2, 3, 1), (1, 2, 2), (15, 15, 1), (4, 6, 2), (0, 3, 1), (2, 0, 0), (2, 3, 0), (9000, 9000, 1), (4000, 1, 4000)]


def w4_of(maxlen):
    return (max(maxlen, 1) + 127) // 128


def aligner_grid():
    """(query line, expected plan)"""
    for k, (x, o, e), semi, sw, n in itertools.product(range(51), GREEDY_PENALTIES, (0, 1), SWITCH_SETS, (N, 8, 10 ** 7)):
        for maxlen, mixed in ((100, 0), (512, 1)):  # Greedy's choice reads neither
            yield f"A {GREEDY} {k} {x} {o} {e} {semi} 0 {n} {maxlen} {w4_of(maxlen)} {mixed} 0 {sw}", parent_greedy(k, x, o, e, semi, n, sw)
    for k, (x, o, e), mode, maxlen, hint, sw in itertools.product(range(64), LEAP_PENALTIES, range(4), MAXLENS, (0, 1), SWITCH_SETS):
        for n, mixed in ((N, 0), (10 ** 7, 1)) if sw == ALL_ON else ((N, 0),):
            yield (f"A {LEAP} {k} {x} {o} {e} 0 {mode} {n} {maxlen} {w4_of(maxlen)} {mixed} {hint} {sw}",
                   parent_leap(k, x, o, e, mode, n, maxlen, w4_of(maxlen), hint, sw))
    for (x, o, e), maxlen, mixed, sw, n in itertools.product(NW_PENALTIES, MAXLENS, (0, 1), SWITCH_SETS, (N, 8, 10 ** 7)):
        for w4 in {w4_of(maxlen), 4}:  # a batch below 4096 pairs is one class of the widest kernel's width
            yield f"A {NW} 3 {x} {o} {e} 0 0 {n} {maxlen} {w4} {mixed} 0 {sw}", parent_nw(x, o, e, n, maxlen, w4, mixed, sw)


def parse(line):
    family, *fields = line.split()
    return dict({"family": family}, **{k: int(v) for k, v in (f.split("=") for f in fields)})


@pytest.fixture(scope="module")
def aligner_plans(plan_check):
    """[(query, plan of asm_plan.h, plan of the dispatch before it)] over the whole grid, computed once"""
    queries, want = zip(*aligner_grid())
    return list(zip(queries, map(parse, plan_check(queries)), want))


def test_aligner_plans_equal_the_dispatch_they_replace(aligner_plans):
    assert len(aligner_plans) > 300000
    bad = [(q, got, want) for q, got, want in aligner_plans if got != want]
    assert not bad, (len(bad), bad[:3])
    assert {got["family"] for _, got, _ in aligner_plans} == {
        "GREEDY_FAST", "GREEDY_PERSIST", "GREEDY_GROUP", "GREEDY_WAVE", "GREEDY_WAVE2", "GREEDY_WIDE", "LEAP_UNIT", "LEAP_GENERAL", "LEAP_QUAD", "LEAP_WIDE",
        "NW_UNIT_FULL", "NW_BANDED", "NW_BANDED_BYLEN", "NW_PAIR2", "NW_WFA", "NW_AFFINE_FULL"}


# what the launchers of csrc/asm_align_host.h instantiate, per family: (k, words) -> allowed, and the ring entries
INSTANTIATED = {
    "GREEDY_FAST": lambda p: 1 <= p["k"] <= 3, "GREEDY_PERSIST": lambda p: 1 <= p["k"] <= 16,
    "GREEDY_GROUP": lambda p: True, "GREEDY_WAVE": lambda p: True, "GREEDY_WAVE2": lambda p: True, "GREEDY_WIDE": lambda p: True,
    "LEAP_UNIT": lambda p: (1 <= p["k"] <= 5 and 2 <= p["words"] <= 6) or (6 <= p["k"] <= 10 and p["words"] == 2),
    "LEAP_GENERAL": lambda p: ((1 <= p["k"] <= 5 and p["words"] in (2, 4)) or (6 <= p["k"] <= 8 and p["words"] == 2)) and p["entry"] in (1, 2),
    "LEAP_QUAD": lambda p: p["words"] in (4, 5, 6, 8, 12, 16) and p["entry"] in (1, 2) and p["waves"] in (1, 4),
    "LEAP_WIDE": lambda p: p["words"] in (2, 4, 8),
    "NW_UNIT_FULL": lambda p: p["words"] in (2, 4, 6, 8),
    "NW_BANDED": lambda p: (p["words"], p["window"]) in ((4, 32), (8, 64), (12, 64), (16, 64)),
    "NW_BANDED_BYLEN": lambda p: (p["words"], p["window"]) in ((4, 32), (8, 64), (12, 64), (16, 64)),
    "NW_PAIR2": lambda p: p["words"] == 4,
    "NW_WFA": lambda p: p["k"] == 7 and (p["words"], p["entry"]) in ((2, 1), (4, 2)) and p["oct_entry"] in (0, 1, 2),
    "NW_AFFINE_FULL": lambda p: p["words"] in (2, 4, 8),
}
BITS_PER_WORD = {"LEAP_UNIT": 64, "LEAP_GENERAL": 64, "LEAP_QUAD": 32, "LEAP_WIDE": 64, "NW_WFA": 64, "NW_AFFINE_FULL": 64}
PAIRS_PER_BLOCK = {"GREEDY_GROUP": 16, "GREEDY_WAVE": 4, "NW_PAIR2": 512}  # else: one pair per thread; the strided and persistent kernels cover any n


def test_aligner_plan_invariants(aligner_plans):
    for q, p, _ in aligner_plans:
        f = q.split()
        aligner, n, maxlen, w4 = int(f[1]), int(f[8]), int(f[9]), int(f[10])
        fam = p["family"]
        assert INSTANTIATED[fam](p), (q, p)
        if fam in BITS_PER_WORD:  # the strings fit the words the kernel is instantiated with
            assert BITS_PER_WORD[fam] * p["words"] >= (128 * w4 if fam == "LEAP_WIDE" else maxlen), (q, p)
        if fam.startswith("NW_") and fam not in BITS_PER_WORD:
            words_of_64 = p["words"] // (1 if fam == "NW_UNIT_FULL" else 2)
            assert 64 * words_of_64 >= 128 * min(w4, 4), (q, p)
        # LDS within the 64 KiB the dispatch compares against; the fast Greedy kernel states its size and asks for it (launch_on)
        if fam == "LEAP_QUAD":  # compared per wave, on the words the strings need
            assert p["lds"] // p["waves"] <= 64 * KIB or first_of((maxlen + 31) // 32, (4, 5, 6, 8, 12, 16)) > (maxlen + 31) // 32, (q, p)
            assert p["waves"] == 1 or p["lds"] + 512 <= 64 * KIB, (q, p)
        elif fam != "GREEDY_FAST":
            assert p["lds"] <= 64 * KIB and p["oct_lds"] <= 64 * KIB, (q, p)
        # a byte holds every stored position + 2
        if fam in ("LEAP_GENERAL", "LEAP_QUAD") and p["entry"] == 1:
            assert maxlen + 2 <= 255, (q, p)
        if fam == "NW_WFA" and (p["entry"] == 1 or p["oct_entry"] == 1):
            assert maxlen + 2 <= 255, (q, p)
        # grid x block covers n, or the kernel strides
        if p["grid_rule"] == EXACT and fam not in ("GREEDY_WIDE", "LEAP_WIDE"):
            per_block = PAIRS_PER_BLOCK.get(fam, p["block"] // 4 if fam == "LEAP_QUAD" else p["block"])
            assert p["grid"] * per_block >= n and (p["grid"] - 1) * per_block < n, (q, p)
        else:
            assert 1 <= p["grid"] <= max(n, blocks(n * 16, BLOCK)), (q, p)
        assert p["sort"] <= p["hinted"] and (aligner == LEAP or not p["hinted"]), (q, p)


def test_filter_plans_equal_the_dispatch_they_replace_and_hold_their_invariants(plan_check):
    shapes = [(n, maxlen) for n in (N, 8, 10 ** 7) for maxlen in (1, 63, 64, 65, 127, 128, 129, 192, 193, 256)]
    ed = [(T, mode, n, maxlen) for T in range(1, 33) for mode in range(4) for n, maxlen in shapes]
    got = plan_check([f"E {T} {mode} {n} {maxlen}" for T, mode, n, maxlen in ed])
    for args, line in zip(ed, got):
        p = parse("E " + line)
        del p["family"]
        assert p == parent_simd_ed(*args), (args, p)
        assert p["words"] in (2, 4) and 64 * p["words"] >= args[3] and 0 <= p["reg_t"] <= 8 and p["lds"] <= 64 * KIB and p["grid"] * p["block"] >= args[2]
    pens = [(x, o, e) for x in (1, 2, 7, 8, 15) for o in (1, 3, 7, 8, 15) for e in (1, 2, 3, 4, 7, 8, 15) if e <= o]
    af = [(gap, x, o, e, n, maxlen) for gap in range(1, 33) for x, o, e in pens for n, maxlen in shapes]
    got = plan_check([f"F {gap} {x} {o} {e} {n} {maxlen}" for gap, x, o, e, n, maxlen in af])
    refused = 0
    for args, line in zip(af, got):
        p = parse("F " + line)
        del p["family"]
        assert p == parent_simd_ed_affine(*args), (args, p)
        refused += p["refused"]
        if not p["refused"]:
            pairs = 16 if p["quad"] else p["block"]
            assert p["lds"] <= 150 * KIB and p["block"] in (16, 32, 64) and p["grid"] * pairs >= args[4], (args, p)
    assert refused == 0  # with the penalties the entry accepts (at most 15) the rings of 16 threads are 100.5 KiB at the most


def test_dispatch_cases_reach_the_kernels_they_name(plan_check):
    """Every row of tests/dispatch_cases.py, at both ends of its length class, under its switch."""
    queries, want = [], []

    def ends(key):
        return (100, 128) if key == "c2" else key

    for r in dc.ALIGNER_ROWS:
        sw = ALL_ON & ~dc.SWITCH_BITS[r.off] if r.off else ALL_ON
        for maxlen in r.span or ends(r.key):
            x, o, e = r.pen
            queries.append(f"A {ALIGNER[r.aligner]} {r.k} {x} {o} {e} 0 0 {dc.N} {maxlen} {w4_of(maxlen)} 0 0 {sw}")
            want.append((r.family, r.want))
    for name, buckets in dc.NW_UNIT_BUCKETS.items():
        for (w4, mixed), off in itertools.product(buckets, (None, "ASM_NW_BANDED", "ASM_NW_BYLEN")):
            sw = ALL_ON & ~dc.SWITCH_BITS[off] if off else ALL_ON
            for maxlen in (128 * (w4 - 1) + 1, 128 * w4) if name != "ragged" else (385, 512):
                queries.append(f"A {NW} 3 1 1 1 0 0 {dc.N} {maxlen} {w4} {int(mixed)} 0 {sw}")
                want.append(dc.nw_unit_want(w4, mixed, off))
    for line, q, (family, fields) in zip(plan_check(queries), queries, want):
        p = parse(line)
        assert p["family"] == family and {k: p[k] for k in fields} == fields, (q, p, family, fields)
    for T, key, fields in dc.SIMD_ED:
        for shd_mode, maxlen in itertools.product((0,), ends(key)):
            (line,) = plan_check([f"E {T} {shd_mode} {dc.N} {maxlen}"])
            p = parse("E " + line)
            assert {k: p[k] for k in fields} == fields, (T, key, p)
    gap, _, x, o, e = dc.SIMD_ED_AFFINE_ARGS
    for key, fields in dc.SIMD_ED_AFFINE:
        for maxlen in ends(key):
            (line,) = plan_check([f"F {gap} {x} {o} {e} {dc.N} {maxlen}"])
            p = parse("F " + line)
            assert {k: p[k] for k in fields} == fields, (key, p)
    # every family has a row, under the default switches or with one switch off
    assert {family for family, _ in want} == set(INSTANTIATED)


CHECKS = [  # (aligner, k, x, o, e, alignment_type, leap_mode, p_match, p_mismatch, p_indel, maxlen) -> code, message
    ((GREEDY, 3, 1, 1, 1, 0, 0, .8, .1, .1, 512), (0, "")),
    ((GREEDY, 3, -1, 1, 1, 0, 0, .8, .1, .1, 512), (-1, "penalties must be non-negative")),
    ((GREEDY, 51, 1, 1, 1, 0, 0, .8, .1, .1, 512), (-1, "Greedy: k must be in [0, 50] (MAX_K, hurdle_matrix.h:8)")),
    ((GREEDY, 3, 1, 1, 1, 0, 0, .8, 0, .1, 512), (-1, "Greedy: probabilities must be positive")),
    ((GREEDY, 3, 1, 1, 1, 2, 0, .8, .1, .1, 512),
     (-4, "Greedy: alignment type must be GLOBAL or SEMI_GLOBAL (LOCAL is unsupported in the reference too, hurdle_matrix.h:467)")),
    ((LEAP, 64, 1, 1, 1, 0, 0, .8, .1, .1, 512), (-1, "LEAP: k out of range")),
    ((LEAP, 3, 1, 1, 2, 0, 0, .8, .1, .1, 512), (-1, "LEAP: need x >= 1, o >= e >= 1 (LV_BAG.cpp:165-166)")),
    ((LEAP, 3, 16, 1, 1, 0, 0, .8, .1, .1, 512), (-4, "LEAP: penalties above the compiled history depth")),
    ((LEAP, 3, 1, 1, 1, 0, 4, .8, .1, .1, 512), (-1, "LEAP: leap_mode must be one of ASM_LEAP_GLOBAL/LOCAL/SEMI_FREE_BEGIN/SEMI_FREE_END")),
    ((LEAP, 3, 1, 1, 1, 0, 1, .8, .1, .1, 513), (-4, "LEAP: the non-GLOBAL modes are built for strings up to 512 characters")),
    ((LEAP, 3, 1, 1, 1, 0, 0, .8, .1, .1, 513), (0, "")),
    ((NW, 3, 1, 10001, 1, 0, 0, .8, .1, .1, 1),
     (-4, "NW: penalties too large for this batch's longest sequence (need 2*(o + (maxlen-1)*e) + o < 30000 and x, o, e <= 10000)")),
    ((NW, 3, 1, 10, 29, 0, 0, .8, .1, .1, 512), (0, "")),  # 2 * (10 + 511 * 29) + 10 = 29668
    ((NW, 3, 1, 10, 30, 0, 0, .8, .1, .1, 512),
     (-4, "NW: penalties too large for this batch's longest sequence (need 2*(o + (maxlen-1)*e) + o < 30000 and x, o, e <= 10000)")),
    ((7, 3, 1, 1, 1, 0, 0, .8, .1, .1, 512), (-1, "unknown aligner id")),
]


def test_parameter_rules_keep_their_codes_and_messages(plan_check):
    got = plan_check(["C " + " ".join(str(v) for v in args) for args, _ in CHECKS])
    for line, (args, (code, msg)) in zip(got, CHECKS):
        assert line == f"{code} {msg}".rstrip() or line == f"{code} {msg}", (args, line)
