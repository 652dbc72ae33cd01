"""The structured corpus (tests/structured_cases.py) on the CPU: that the corpus is what it claims to be, that the oracle agrees
with the compiled reference and with the committed goldens on it, and that the host-buildable per-thread cores (the fast Greedy
pass, the unit-penalty LEAP core, the banded NW sweeps) give the oracle's results on it.  No GPU needed; the kernels are in
test_gpu_structured.py."""
import json
import os

import numpy as np
import pytest

from tests import oracle_binding
from tests import structured_cases as sc
from tests.golden.make_golden import digest, inputs_sha
from tests.golden.make_golden_structured import case_batch
from tests.test_greedy3_host import g3, run as g3_run  # noqa: F401  (g3, leaph, nwh: the modules' library fixtures)
from tests.test_leap_unit_host import CORE, GENERIC, check_all_forms, leaph, run as leap_run  # noqa: F401
from tests.test_nw_pair2_host import band, cascade, check_halves, full, half16, nwh, pair2  # noqa: F401
from tests.util import greedy_defined, leap_defined

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_reference = pytest.mark.skipif(not oracle_binding.have_reference(), reason="oracle/_ref not built (no reference tree)")
needs_reference_simd = pytest.mark.skipif(not oracle_binding.have_reference_simd(), reason="oracle/_ref/libasm_ref_simd.so not built")
PENALTIES = ((1, 1, 1), (2, 3, 1), (4, 6, 2))
BANDS = (1, 3, 6, 10, 16, 30)


@pytest.fixture(scope="module")
def batches(asm):
    """all_kinds_batch by (lo, hi, k, capped), made on first use."""
    made = {}

    def get(lo, hi, k, capped=False):
        key = (lo, hi, k, capped)
        if key not in made:
            made[key] = sc.all_kinds_batch(asm, lo, hi, k, max_diff=k if capped else None)
        return made[key]

    return get


# ---- the corpus proves what it claims, from the strings alone ----
def test_batches_are_deterministic_and_interleaved(asm):
    a, b = sc.all_kinds_batch(asm, 100, 128, 3, seed=5), sc.all_kinds_batch(asm, 100, 128, 3, seed=5)
    assert inputs_sha(a) == inputs_sha(b) and inputs_sha(a) != inputs_sha(sc.all_kinds_batch(asm, 100, 128, 3, seed=6))
    assert a.n == sc.N and list(a.kinds[:8]) == list(sc.KINDS) and (a.kinds[:-1] != a.kinds[1:]).all()
    one = sc.structured_batch(asm, "tandem", 129, 192, 5, 200, 1)
    assert one.n == 200 and set(one.kinds) == {"tandem"}


@pytest.mark.parametrize("lo,hi", [(31, 128), (100, 128), (129, 192), (193, 256), (129, 256), (257, 320), (321, 384), (385, 512), (1, 512)])
def test_lengths_stay_in_the_class_and_visit_its_edges(asm, lo, hi):
    """The longer string of every pair is inside [lo, hi], and each kind meets every word and granule edge of the class."""
    hb = sc.all_kinds_batch(asm, max(lo, 31), hi, 6)
    longer = np.maximum(*hb.lengths())
    assert longer.min() >= max(lo, 31) and longer.max() <= hi
    for kind in sc.KINDS:
        assert set(L for L in sc.EDGES if max(lo, 31) <= L <= hi) <= set(longer[hb.kinds == kind]), kind


# Half of the repeat pairs take their random edits within ZONE characters of the ends (the other half anywhere, word edges
# included).  The run such a pair keeps on diagonal d is L - 2 ZONE - |shift - d| with |shift| and |d| up to k
# (structured_cases._end_edits): 64 characters need L >= 64 + 2 ZONE + 2 k, so the statement is made for the classes and bands that
# allow it.  A tandem pair can only match on the diagonals of one residue modulo its period, and a rotation's long diagonals are
# those congruent to the rotation.
@pytest.mark.parametrize("lo,hi,k", [(100, 128, 1), (100, 128, 3), (100, 128, 12), (129, 192, 6), (129, 192, 16), (193, 256, 30)])
def test_repeats_extend_every_diagonal_across_word_edges(asm, lo, hi, k):
    assert lo >= 64 + 2 * sc.ZONE + 2 * k
    for kind in sc.REPEAT_KINDS:
        hb = sc.structured_batch(asm, kind, lo, hi, k, 133, 3, max_diff=k)
        off_main = checked = beyond = scattered_on_edge = 0
        for i in range(hb.n):
            a, b = hb.pair(i)
            meta = hb.meta[i]
            if meta.get("edits") == "scattered":  # edits inside the repeat: no run is promised, but the edits must be there
                scattered_on_edge += any(a[w:w + 1] != b[w:w + 1] for w in sc.WORD_EDGES)
                continue
            runs = sc.diagonal_runs(a, b, k)
            assert set(runs) == set(d for d in range(-k, k + 1) if -len(a) < d < len(b))
            long_ones = sorted(d for d, r in runs.items() if r >= 64)
            if kind == "rotated_repeat" and meta["rotation"] == k + 1 and not long_ones:
                beyond += 1  # the rotation just beyond the band, where the period brings no diagonal of its residue back inside
                continue
            checked += 1
            assert long_ones, (kind, a, b)
            want = [d for d in runs if (d - long_ones[0]) % meta["period"] == 0]
            assert long_ones == sorted(want), (kind, meta, long_ones, a, b)
            off_main += any(d != 0 for d in long_ones)
        # one rotation in k + 1 is the one beyond the band: no more pairs than that may go unchecked
        assert beyond <= -(-hb.n // (k + 1)), (kind, beyond)
        if kind == "rotated_repeat":
            assert checked == hb.n - beyond
        else:
            assert checked >= hb.n // 2 - 6 and hb.n - checked >= hb.n // 2 - 6, (kind, checked)
            assert scattered_on_edge >= (hb.n - checked) // 4, (kind, scattered_on_edge)  # edits that sit on word edges
        # a homopolymer: every diagonal; a repeat of period p: off the main diagonal when p <= k or its middle is shifted
        assert off_main >= (checked if kind == "homopolymer" else checked // 4), (kind, off_main)


@pytest.mark.parametrize("k", [1, 3, 16, 40])
def test_every_rotation_and_shift_up_to_one_beyond_the_band(asm, k):
    """In the 133 pairs a kind has in an all_kinds_batch: rotations and shifts 1 .. k + 1, shifts in both directions, and at a
    narrow band every period with every rotation."""
    hb = sc.all_kinds_batch(asm, 100, 128, k, max_diff=k)
    rotated = [m for m in hb.meta if m["kind"] == "rotated_repeat"]
    assert set(m["rotation"] for m in rotated) == set(range(1, k + 2))
    if 6 * (k + 1) <= len(rotated):
        assert set((m["period"], m["rotation"]) for m in rotated) == set((p, r) for p in range(2, 8) for r in range(1, k + 2))
    assert set(m["period"] for m in rotated) == set(range(2, 8))
    assert set(m["shift"] for m in hb.meta if m["kind"] == "shifted") == set(range(-k - 1, 0)) | set(range(1, k + 2))


@pytest.mark.parametrize("k,capped", [(1, True), (3, True), (3, False), (6, False), (16, True), (40, True)])
def test_block_gaps_of_every_length_and_placement(asm, k, capped):
    hb = sc.structured_batch(asm, "block_gap", 100, 128, k, 133, 4, max_diff=k if capped else None)
    want = set(sc.gap_lengths(k, k if capped else None))
    assert want == set(max(1, min(g, k if capped else k + 1)) for g in (1, k - 1, k, k + 1))
    seen = set()
    for i, meta in enumerate(hb.meta):
        a, b = hb.pair(i)
        assert abs(len(a) - len(b)) == meta["gap"]
        short, long_ = (a, b) if len(a) < len(b) else (b, a)
        p, g = meta["at"], meta["gap"]
        assert long_[:p] == short[:p] and long_[p + g:] == short[p:]  # one gap of g at p and nothing else
        assert {"start": p == 0, "end": p + g == len(long_), "word_edge": p % 32 == 0 and p > 0, "random": True}[meta["placement"]]
        seen.add((g, meta["insertion"], meta["placement"]))
    assert seen == set((g, ins, pl) for g in want for ins in (False, True) for pl in sc.PLACEMENTS)


@pytest.mark.parametrize("lo,hi", [(31, 128), (100, 128), (129, 192), (129, 256), (385, 512)])
def test_edge_edits_sit_on_every_word_edge(asm, lo, hi):
    """Every listed position below the longest string of the class, and the last character, each as a substitution, a deletion
    and an insertion — in a batch of the kind and in the 133 pairs the kind has in an all_kinds_batch."""
    forms = ("substitution", "deletion", "insertion")
    mixed = sc.all_kinds_batch(asm, lo, hi, 3)
    for hb in (sc.structured_batch(asm, "edge_edits", lo, hi, 3, 133, 5), mixed):
        seen, last = set(), set()
        for i, meta in enumerate(hb.meta):
            if meta["kind"] != "edge_edits":
                continue
            a, b = hb.pair(i)
            w, L = meta["at"], meta["L"]
            assert max(len(a), len(b)) == L and w < L and a[:w] == b[:w]
            if meta["form"] == "substitution":
                assert a[w] != b[w] and a[w + 1:] == b[w + 1:], (meta, a, b)
            else:
                assert a[w + 1:] == b[w:] if meta["form"] == "deletion" else a[w:] == b[w + 1:], (meta, a, b)
            seen.add((w, meta["form"]))
            if w == L - 1:
                last.add(meta["form"])
        assert seen >= set((w, f) for w in sc.EDIT_POSITIONS if w < hi for f in forms), (lo, hi, sorted(seen))
        assert last == set(forms)


@pytest.mark.parametrize("lo,hi", [(31, 128), (100, 128), (129, 256), (385, 512)])
def test_unrelated_pairs_are_far_apart(asm, oracle, lo, hi):
    hb = sc.structured_batch(asm, "unrelated", lo, hi, 3, 133, 6)
    assert (oracle.nw(hb) > np.maximum(*hb.lengths()) / 3).mean() >= 0.9
    m, n = hb.lengths()
    assert (m == n).all() and sum(meta["complement"] for meta in hb.meta) >= hb.n // 2 - 1
    for i in np.flatnonzero([meta["complement"] for meta in hb.meta])[:20]:
        a, b = hb.pair(int(i))
        assert all(x != y for x, y in zip(a, b))  # a solid mismatch block over the whole length


def test_dirty_repeats_hold_non_bases(asm):
    hb = sc.structured_batch(asm, "dirty_repeat", 100, 128, 3, 133, 7)
    dirty = np.isin(hb.reads, sc.DIRTY).sum() + np.isin(hb.refs, sc.DIRTY).sum()
    assert dirty == sum(meta["dirty"] for meta in hb.meta) and 0.005 < dirty / (hb.reads.size + hb.refs.size) < 0.02
    seen = sc.as_packed(asm, hb)
    assert not np.isin(seen.reads, sc.DIRTY[:-2]).any() and (seen.reads != hb.reads).sum() > 0


GREEDY_CELLS = [(100, 128, k, True) for k in (1, 2, 3, 4, 6, 10, 12, 16, 17, 30, 31, 32, 39, 40)]
OTHER_CELLS = [(31, 128, k, False) for k in (1, 3, 5, 6, 10, 11, 30)] + [(129, 192, k, False) for k in (1, 5, 6)] + \
              [(193, 256, k, False) for k in (1, 5, 6)] + [(129, 256, k, False) for k in (3, 5, 6, 10, 16, 30)]


@pytest.mark.parametrize("lo,hi,k,capped", GREEDY_CELLS + OTHER_CELLS)
def test_the_predicates_leave_the_corpus_in(batches, lo, hi, k, capped):
    """greedy_defined on the batches the Greedy comparisons use and leap_defined on those the LEAP comparisons use remove at
    most a tenth of any kind (as built: nothing)."""
    hb = batches(lo, hi, k, capped)
    if capped:
        sc.assert_predicate_leaves_most(hb, greedy_defined(hb, k), ("greedy_defined", lo, hi, k))
    sc.assert_predicate_leaves_most(hb, leap_defined(hb), ("leap_defined", lo, hi, k))


# ---- the oracle against the compiled reference ----
@needs_reference
@pytest.mark.parametrize("k", BANDS)
def test_oracle_equals_reference_greedy_and_leap(batches, oracle, k):
    """Greedy cost and CIGAR in both buffer-tail modes, global and SEMI_GLOBAL, and LEAP, for three penalty sets."""
    ref = oracle_binding.load_reference()
    hb = batches(100, 128, k, True)
    gd = greedy_defined(hb, k)
    sc.assert_predicate_leaves_most(hb, gd, "greedy_defined")
    for x, o, e in PENALTIES:
        for semi in (False, True):
            for mode in (0, 1):
                oc, ocig = oracle.greedy(hb, k, x, o, e, mode=mode, cigars=True, semi=semi)
                rc, rcig = ref.greedy(hb, k, x, o, e, mode=mode, cigars=True, semi=semi)
                bad = np.flatnonzero((oc != rc) & gd)
                assert bad.size == 0, (k, x, o, e, mode, semi, hb.kinds[bad[0]], hb.pair(int(bad[0])), oc[bad[0]], rc[bad[0]])
                bad = [i for i in np.flatnonzero(gd) if ocig[i] != rcig[i]]
                assert not bad, (k, x, o, e, mode, semi, "CIGAR", hb.kinds[bad[0]], hb.pair(int(bad[0])), ocig[bad[0]], rcig[bad[0]])
        for lo, hi in ((31, 128), (129, 256)):
            hl = batches(lo, hi, k)
            ld = leap_defined(hl)
            sc.assert_predicate_leaves_most(hl, ld, "leap_defined")
            got, want = oracle.leap(hl, k, x, o, e), ref.leap(hl, k, x, o, e)
            bad = np.flatnonzero((got != want) & ld)
            assert bad.size == 0, ("leap", k, x, o, e, hl.kinds[bad[0]], hl.pair(int(bad[0])), got[bad[0]], want[bad[0]])


@needs_reference
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_oracle_equals_reference_leap_ed_modes(batches, oracle, mode):
    ref = oracle_binding.load_reference()
    for lo, hi in ((31, 128), (129, 256)):
        for k, x, o, e in ((3, 1, 1, 1), (5, 2, 3, 1), (10, 1, 1, 1), (8, 4, 6, 2)):
            hb = batches(lo, hi, k)
            ld = leap_defined(hb)
            sc.assert_predicate_leaves_most(hb, ld, "leap_defined")
            got = oracle.leap(hb, k, x, o, e, mode)
            for clean in (True, False):
                want = ref.leap_mode(hb, k, x, o, e, mode, clean=clean)
                bad = np.flatnonzero((got != want) & ld)
                assert bad.size == 0, (mode, k, x, o, e, clean, hb.kinds[bad[0]], hb.pair(int(bad[0])), got[bad[0]], want[bad[0]])


@needs_reference_simd
@pytest.mark.parametrize("lo,hi", [(31, 128), (100, 128), (129, 256)])
def test_oracle_equals_reference_filters(batches, oracle, lo, hi):
    """SIMD_ED at six thresholds with and without SHD, SHD at five, affine SIMD_ED at two settings in every ED mode."""
    ref = oracle_binding.load_reference_simd()
    hb = batches(lo, hi, 3)
    for t in (1, 3, 8, 9, 16, 25):
        for shd in ((False, True) if t <= 16 else (False,)):
            r_ed, r_ps = ref.simd_ed(hb, t, shd)
            _, o_raw, o_ps = oracle.simd_ed(hb, t, shd, 0, oracle_binding.SIMD_WARM_STATE)
            bad = np.flatnonzero((r_ps != o_ps) | (r_ed != o_raw))
            assert bad.size == 0, (t, shd, hb.kinds[bad[0]], hb.pair(int(bad[0])), o_raw[bad[0]], r_ed[bad[0]])
    for me in (0, 1, 3, 7, 16):
        assert np.array_equal(ref.shd(hb, me), oracle.shd(hb, me)), me
    for g, af, x, o, e in ((3, 60, 2, 3, 1), (12, 120, 4, 6, 2)):
        for shd_t in (None, 2):
            for mode in (0, 1, 2, 3):
                o_ed, o_ps = oracle.simd_ed_affine(hb, g, af, x, o, e, shd_t=shd_t, mode=mode)
                r_ed, r_ps = ref.simd_ed_affine(hb, g, af, x, o, e, shd_t=shd_t, mode=mode)
                bad = np.flatnonzero((o_ps != r_ps) | (o_ed != np.where(r_ps == 1, r_ed, -1)))
                assert bad.size == 0, (g, af, x, o, e, shd_t, mode, hb.kinds[bad[0]], hb.pair(int(bad[0])), o_ed[bad[0]], r_ed[bad[0]])


# ---- the committed goldens: the same pin where the reference is absent ----
with open(os.path.join(GOLDEN, "structured_index.json")) as _fh:
    STRUCTURED_INDEX = json.load(_fh)


@pytest.mark.parametrize("name", sorted(STRUCTURED_INDEX["cases"]))
def test_oracle_matches_reference_goldens(oracle, name):
    case = STRUCTURED_INDEX["cases"][name]
    k, x, o, e = case["k"], case["x"], case["o"], case["e"]
    hb = case_batch(case["lo"], case["hi"], k, case["capped"])
    assert hb.n == case["n"] and inputs_sha(hb) == case["inputs_sha256"], "the corpus changed: regenerate with make_golden_structured.py"
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    gd, ld = greedy_defined(hb, k), leap_defined(hb)
    if case["capped"]:
        sc.assert_predicate_leaves_most(hb, gd, "greedy_defined")
    sc.assert_predicate_leaves_most(hb, ld, "leap_defined")
    for mode, tag in ((0, "seq"), (1, "clean")):
        cost, cig = oracle.greedy(hb, k, x, o, e, mode=mode, cigars=True)
        assert np.array_equal(cost[gd], gold[f"greedy_{tag}_cost"][gd]), (name, tag)
        assert np.array_equal(digest(cig)[gd], gold[f"greedy_{tag}_cigar"][gd]), (name, tag, "CIGAR")
    assert np.array_equal(oracle.leap(hb, k, x, o, e)[ld], gold["leap_ed"][ld]), name
    for t, shd in STRUCTURED_INDEX["simd_settings"]:
        _, raw, ps = oracle.simd_ed(hb, t, bool(shd), 0, tuple(STRUCTURED_INDEX["warm_state"]))
        assert np.array_equal(ps, gold[f"pass_t{t}_shd{shd}"]) and np.array_equal(raw, gold[f"ed_t{t}_shd{shd}"]), (name, t, shd)
    for me in STRUCTURED_INDEX["shd_errors"]:
        assert np.array_equal(oracle.shd(hb, me), gold[f"shd_e{me}"]), (name, me)
    for g, af, ax, ao, ae in STRUCTURED_INDEX["affine_settings"]:
        ed, ps = oracle.simd_ed_affine(hb, g, af, ax, ao, ae)
        r_ps, r_ed = gold[f"af_pass_g{g}_a{af}_x{ax}o{ao}e{ae}"], gold[f"af_ed_g{g}_a{af}_x{ax}o{ao}e{ae}"]
        assert np.array_equal(ps, r_ps) and np.array_equal(ed, np.where(r_ps == 1, r_ed, -1)), (name, g, af)
    first = hb.slice(0, case["nw_first"])
    assert np.array_equal(oracle.nw(first, x, o, e), gold["nw_first"]), name


# ---- the host-buildable cores: the per-thread code of the kernels, against the oracle ----
def _first_bad(hb, got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else (bad.size, hb.kinds[bad[0]], hb.pair(int(bad[0])), int(got[bad[0]]), int(want[bad[0]]))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_fast_greedy_pass_on_the_corpus(g3, batches, oracle, k):  # noqa: F811
    """g3_setup / g3_pass at k = 1..3, clean and sequential views (a homopolymer's stale tail under the next pair), on the class
    the kernel is timed on and on every length down to 31."""
    slow_seen = 0
    for lo, hi, capped in ((100, 128, True), (31, 128, False)):
        hb = batches(lo, hi, k, capped)
        for mode in (1, 0):
            got, passes, slow = g3_run(g3, oracle, hb, k, mode=mode)
            assert _first_bad(hb, got, oracle.greedy(hb, k=k, mode=mode)) is None, (lo, hi, mode, _first_bad(hb, got, oracle.greedy(hb, k=k, mode=mode)))
            assert passes.min() >= 1
            slow_seen += slow
    assert slow_seen > 0  # the complement pairs push hurdles + switches past the rank table: the FP64 path ran too


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_leap_unit_core_on_the_corpus(leaph, asm, batches, oracle, k):  # noqa: F811
    """Every form at two words of 64 bits (generic, core, and the one-granule form with its clamp check on every lane step), and
    generic and core at three words, on strings up to 128 and, at three words, up to 192."""
    hb = batches(31, 128, k)
    want = check_all_forms(leaph, oracle, hb, k, seen_as=sc.as_packed(asm, hb))
    for form in (GENERIC, CORE):
        assert _first_bad(hb, leap_run(leaph, hb, k, form, w64=3)[0], want) is None, (form, "three words")
    assert (want <= k).sum() > 100 and (want > k).sum() > 100  # pairs within the band, and generations beyond the first k
    long_ = batches(129, 192, k)
    want = oracle.leap(sc.as_packed(asm, long_), k=k)
    for form in (GENERIC, CORE):
        got = leap_run(leaph, long_, k, form, w64=3)[0]
        assert _first_bad(long_, got, want) is None, (form, _first_bad(long_, got, want))


@pytest.mark.parametrize("lo,hi,k", [(31, 128, 3), (100, 128, 6), (100, 128, 16), (31, 128, 30)])
def test_banded_nw_sweeps_on_the_corpus(nwh, asm, batches, oracle, lo, hi, k):  # noqa: F811
    """nw_band<4, 32>, nw_band<4, 64>, nw_band2x16<4> with neighbouring pairs (of different kinds) in the two halves of a dword,
    and the cascade the kernel stores: a window reports only the distance and only within its bound; the cascade is the oracle's."""
    hb = sc.as_packed(asm, batches(lo, hi, k))  # the sweeps work on the planes; the host check's last stage compares characters
    want = oracle.nw(hb)
    m, n = hb.lengths()
    h16 = half16(nwh, hb)
    told = check_halves(hb, h16, want)
    assert told.mean() > 0.3
    for W in (32, 64):
        got = band(nwh, hb, W)
        ok = got >= 0
        assert _first_bad(hb, got[ok], want[ok]) is None, (W, hb.kinds[np.flatnonzero(ok)[np.flatnonzero(got[ok] != want[ok])[:1]]])
        assert (got[ok] <= W - 2 - np.abs(n - m)[ok]).all()
        assert ok[(want <= W - 2 - np.abs(n - m)) & (np.abs(n - m) < W // 2)].all()  # nothing within the bound is turned away
    assert _first_bad(hb, full(nwh, hb), want) is None
    assert _first_bad(hb, cascade(nwh, hb, h16), want) is None


def test_a_half_never_sees_a_homopolymer_partner(nwh, asm, batches, oracle):  # noqa: F811
    """Carry isolation on the corpus: every pair gives the same 16-row result next to each of the homopolymers (Eq and VP all
    ones: the longest carry chains of the add) as next to itself, in either half."""
    hb = sc.as_packed(asm, batches(100, 128, 3))
    homo = np.flatnonzero(hb.kinds == "homopolymer")[:12]
    idx = np.arange(hb.n)
    alone = pair2(nwh, hb, idx, idx)
    assert np.array_equal(alone[0], alone[1])
    for h in homo:
        partner = np.full(hb.n, h)
        low, q = pair2(nwh, hb, idx, partner)
        p, high = pair2(nwh, hb, partner, idx)
        assert np.array_equal(low, alone[0]) and np.array_equal(high, alone[0]), hb.pair(int(h))
        assert (q == alone[0][h]).all() and (p == alone[0][h]).all(), hb.pair(int(h))
