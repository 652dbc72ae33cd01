"""tests/tail_cases.py proved on the host, with the oracle alone: the inputs of test_gpu_tail_planes.py carry old bytes across
every seam of the stale-tail resolver, and `expected_planes` agrees with an independent packer where one exists.

The seam counterfactual.  A seam pair t is the first pair behind a boundary of the resolver (every multiple of 40 pairs = chunk,
of 5120 = workgroup, and of the carry kernel's segment where it folds several workgroups per thread).  On a side, t's *writer*
p is the nearest earlier pair that rewrote that whole buffer (128 characters or more: a plant).  Replacing p by an empty pair
must change what t's conversion sees in at least 64 of the 128 slots of every active side: 122 slots survive coasting pairs,
and the bytes of the plant before p (codes 1..3 against codes 1..3) coincide in about a third of them.  Where p lies before
the previous seam of the same kind, those bytes have crossed a whole chunk / workgroup / segment through the scans; the cases
that have such seams are listed in LONG_RANGE.  A seam pair that is itself a plant sees no stale byte on that side and is left
out.  In the eroding batch mid-length pairs overwrite part of a plant's bytes: there the 64 slots are required at the seams
with no such pair on that side between p and t, and every kind of seam must also have pairs behind a partial overwrite that
still see bytes of p."""
import numpy as np
import pytest

from tests import tail_cases as tc

MIN_SLOTS = 64
# (case, n): kinds of seam that old bytes must cross from before the previous seam of the same kind
LONG_RANGE = {("A", 400): ("chunk",), ("B", 10241): ("chunk",), ("B-far", 10241): ("chunk", "workgroup"),
              ("B-far", 15361): ("chunk", "workgroup"), ("C", 163840): ("chunk", "workgroup"),
              ("C", 163841): ("chunk", "workgroup", "segment"), ("C", 327681): ("chunk", "workgroup", "segment"),
              ("D-eroding", tc.N_D): ("chunk", "workgroup", "segment"),
              ("D-reads-empty", tc.N_D): ("chunk", "workgroup", "segment"),
              ("D-refs-empty", tc.N_D): ("chunk", "workgroup", "segment")}
CASES = ([("A", n) for n in tc.SIZES_A] + [("B", n) for n in tc.SIZES_B] + [("B-far", n) for n in tc.SIZES_B_FAR]
         + [("C", n) for n in tc.SIZES_C] + [("D-eroding", tc.N_D), ("D-reads-empty", tc.N_D), ("D-refs-empty", tc.N_D)])


def _state_before(views, t):
    """The two buffers before pair t's strings are copied in: pair t - 1's view, permuted (zeros before the first pair)."""
    return np.zeros(256, np.uint8) if t == 0 else views[t - 1][:, tc.SRC].reshape(-1)


def _seam_report(oracle, hb):
    """For every side, seam kind and seam pair: (t, writer p, slots that differ without p, mid-length pairs between)."""
    views = oracle.greedy_views(hb, 0)
    lengths = hb.lengths()
    out = {}
    for s in range(2):
        L = lengths[s]
        full, mid = np.nonzero(L >= 128)[0], np.nonzero((L > 2) & (L < 128))[0]
        if full.size == 0:
            continue                                            # an inactive side: nothing is ever planted on it
        differ = np.full(hb.n, -1, np.int64)                   # per pair t: slots of side s that change without t's writer
        for i, p in enumerate(full):
            end = int(full[i + 1]) if i + 1 < full.size else hb.n
            oracle.set_initial_buffers(_state_before(views, int(p)))
            try:
                alt = oracle.greedy_views(tc.with_empty_pair(hb.slice(int(p), end), 0), 0)
            finally:
                oracle.set_initial_buffers(None)
            differ[p + 1:end] = (alt[1:, s] != views[p + 1:end, s]).sum(axis=1)
        for kind, period in tc.seam_pairs(hb.n).items():
            rows = []
            for t in range(period, hb.n, period):
                if L[t] >= 128:
                    continue
                p = int(full[np.searchsorted(full, t) - 1])
                between = int(np.searchsorted(mid, t) - np.searchsorted(mid, p))
                rows.append((t, p, int(differ[t]), between, p < t - period))
            out[s, kind] = rows
    return out


@pytest.mark.parametrize("case,n", CASES)
def test_seam_counterfactual(oracle, case, n):
    hb = tc.case_batch(case, n)
    report = _seam_report(oracle, hb)
    assert report or not tc.seam_pairs(n), "a batch with seams and no active side"
    for (s, kind), rows in report.items():
        weak = [(t, p, d) for t, p, d, between, _ in rows if between == 0 and d < MIN_SLOTS]
        assert not weak, f"{case} n={n} side {s}: {kind} seam pairs (t, writer, slots) below {MIN_SLOTS}: {weak[:5]}"
        if kind in LONG_RANGE.get((case, n), ()):
            far = [r for r in rows if r[4] and r[2] > 0]
            assert far, f"{case} n={n} side {s}: no {kind} seam sees a writer from before the previous {kind} seam"
        if case == "D-eroding":
            eroded = [r for r in rows if r[3] > 0 and 0 < r[2]]
            assert eroded, f"{case} side {s}: no {kind} seam behind a partial overwrite still sees its writer"
    if case.startswith("D-re"):
        assert {s for s, _ in report} == {1 if case == "D-reads-empty" else 0}


def test_orbit_facts():
    """What the builders rely on, from the permutation's definition alone."""
    assert sorted(tc.SRC.tolist()) == list(range(128))
    sizes = sorted(len(o) for o in tc.orbits())
    assert sizes == [1] * 4 + [2] * 2 + [5] * 12 + [10] * 6
    power, order = tc.SRC.copy(), 1
    while not np.array_equal(power, np.arange(128)):
        power, order = tc.SRC[power], order + 1
    assert order == 10                                           # chunks of a multiple of 10 pairs start in the same slot frame
    assert len(tc.survivors(2)) == 122 and len(tc.survivors(1)) == 127 and len(tc.survivors(0)) == 128
    # 100 bp data: two fixed points and one 2-cycle lie wholly at or above slot 100, and nothing is ever written there
    assert tc.survivors(100) == [109, 111, 125, 127]
    assert len(tc.survivors(128)) == 0


def test_coasting_keeps_a_plant_visible(oracle):
    """The survivor count seen through the oracle: 5000 coasting pairs after a plant, and at least the 122 surviving slots
    still hold the plant's non-zero codes (slots 0 and 1 and their orbits hold whatever the coasting pairs wrote)."""
    hb = tc.plant_and_coast(5001, (0,), seed=1)
    views = oracle.greedy_views(hb, 0)
    plant = views[0]
    assert np.all(tc.LUT[plant] != 0) and not np.array_equal(plant[0], plant[1])
    frame = np.arange(128)
    for t in range(1, hb.n):
        frame = frame[tc.SRC]                                     # slot q of pair t's buffer holds what slot frame[q] held at pair 0
        if t in (1, 7, 40, 4999, 5000):
            keep = np.isin(frame, tc.survivors(2))
            assert keep.sum() == 122
            for s in range(2):
                assert np.array_equal(views[t, s, keep], plant[s, frame[keep]]), (t, s)


@pytest.mark.parametrize("bucketed", [False, True])
def test_expected_planes_equals_the_clean_packer(asm, oracle, bucketed):
    """On clean views (every stale byte zero) expected_planes must be test_gpu_pack_planes's packer, which works from the
    strings and the rule alone; ragged 0-200 as one bucket, and 0-300 over three width classes in bucket order."""
    from tests.test_gpu_pack_planes import _expected
    from tests.util import random_ragged_batch

    hb = random_ragged_batch(asm, 5, 3000, 0, 300 if bucketed else 200)
    order, entries = tc.host_order(hb, bucketed)
    if bucketed:
        assert not np.array_equal(order, np.arange(hb.n)) and len(tc.bucket_layout(*hb.lengths(), order, entries)) == 3
    got_planes, got_lens = tc.expected_planes(hb, oracle.greedy_views(hb, 1), order, entries)
    want_planes, want_lens = _expected(hb, order, entries)
    assert np.array_equal(got_lens, want_lens)
    assert np.array_equal(got_planes, want_planes)
    # and the sequential views differ from the clean ones in granule 0 only
    seq_planes, _ = tc.expected_planes(hb, oracle.greedy_views(hb, 0), order, entries)
    changed = np.nonzero((seq_planes != want_planes).any(axis=1))[0]
    assert changed.size > 0
    assert {tc.locate_entry(hb, order, entries, int(e))[3] for e in changed} == {0}


def test_locate_entry_inverts_the_layout(asm):
    from tests.util import random_ragged_batch

    hb = random_ragged_batch(asm, 6, 500, 0, 300)
    order, entries = tc.host_order(hb, True)
    seen = {tc.locate_entry(hb, order, entries, e) for e in range(entries)}
    assert len(seen) == entries and {k[0] for k in seen} == set(range(hb.n))


def test_shard_chain_on_the_host(asm, oracle):
    """Case G without the device: summaries folded shard after shard by asm_tail_state_advance, each shard's views run from
    the folded state, equal the whole batch's views; the last state is the whole batch's final buffers."""
    from tests import oracle_binding as ob

    hb = tc.case_batch("C", sum(tc.CUTS_G))
    whole = oracle.greedy_views(hb, 0)
    want_final = tc.LUT[oracle.final_buffers()]
    state, lo = np.zeros(256, np.uint8), 0
    for n in tc.CUTS_G:
        part = hb.slice(lo, lo + n)
        oracle.set_initial_buffers(ob.codes_to_buffers(state))
        try:
            views = oracle.greedy_views(part, 0)
        finally:
            oracle.set_initial_buffers(None)
        assert np.array_equal(tc.LUT[views], tc.LUT[whole[lo:lo + n]]), f"shard [{lo}, {lo + n})"
        state = asm.tail_state_advance(state, oracle.tail_summary(part), n)
        lo += n
    assert lo == hb.n and np.array_equal(state, want_final)
