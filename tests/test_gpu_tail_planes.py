"""The stale-tail resolver (csrc/asm_tails.h) read back bit for bit: every entry of a sequential-mode batch's packed planes against
the bytes the oracle's buffer model says each conversion sees (tests/tail_cases.py: expected_planes), on inputs that carry old
bytes across every seam of the three passes -- 40-pair chunks, 5120-pair workgroups, and the carry kernel's segments of 1, 2
and 3 workgroups (n > 163 840, n > 327 680).  tests/test_tail_cases_host.py proves on the host that the inputs do so.  A wrong
tail bit rarely changes a Greedy penalty, so the penalties of test_gpu_parity.py cannot stand in for this."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import tail_cases as tc
from tests.util import greedy_defined, random_ragged_batch

pytestmark = pytest.mark.gpu

_views = {}


def _whole_c(oracle):
    """Batch C at its largest size with its views: shared by the plain case and the shard chain, never modified."""
    if "C" not in _views:
        hb = tc.case_batch("C", sum(tc.CUTS_G))
        _views["C"] = (hb, oracle.greedy_views(hb, 0))
    return _views["C"]


def _views_from(oracle, hb, state=None):
    oracle.set_initial_buffers(None if state is None else ob.codes_to_buffers(state))
    try:
        return oracle.greedy_views(hb, 0)
    finally:
        oracle.set_initial_buffers(None)


def _compare(hb, views, batch, what=""):
    planes, lens, order = batch.download_planes()
    assert np.array_equal(np.sort(order), np.arange(hb.n, dtype=np.uint32)), f"{what}: order is no permutation"
    want_planes, want_lens = tc.expected_planes(hb, views, order, planes.shape[0])
    bad = np.nonzero(lens != want_lens)[0]
    assert bad.size == 0, f"{what}: lens: {bad.size} slots differ, first {bad[:5]}"
    if not np.array_equal(planes, want_planes):
        pytest.fail(f"{what}: " + tc.describe_mismatch(hb, order, planes, want_planes))
    return planes


def _check_upload(asm, engine, oracle, hb, views=None, what=""):
    views = oracle.greedy_views(hb, 0) if views is None else views
    batch = engine.upload(hb, asm.GREEDY_SEQUENTIAL)
    _compare(hb, views, batch, what)
    return batch


def _check_greedy(asm, engine, oracle, hb, batch):
    """The planes tied to what the aligner reads: penalties where the reference defines them (|n - m| <= k)."""
    got, want = engine.align(batch, asm.GREEDY, asm.Params.default(k=3)), oracle.greedy(hb, 3, mode=0)
    ok = greedy_defined(hb, 3)
    assert ok.sum() > hb.n // 2
    bad = np.nonzero((got != want) & ok)[0]
    assert bad.size == 0, f"greedy: {bad.size} differ; first {bad[:5]} got {got[bad[:5]]} want {want[bad[:5]]}"


@pytest.mark.parametrize("n", tc.SIZES_A)
def test_a_chunk_seams(asm, engine, oracle, n):
    """Plants on both sides of the first two chunk seams; sizes at every phase of the slot frame (n mod 10), with a ragged last
    chunk (the cnt mod 10 fix-up of pass 1), a last chunk of one pair, and leftovers of the TAIL_AHEAD loop."""
    _check_upload(asm, engine, oracle, tc.case_batch("A", n), what=f"A n={n}")


@pytest.mark.parametrize("case,n", [("B", n) for n in tc.SIZES_B] + [("B-far", n) for n in tc.SIZES_B_FAR])
def test_b_workgroup_seams(asm, engine, oracle, case, n):
    """The scan over a workgroup's 128 chunks in LDS, loc / grp, a last workgroup of one pair; B-far plants nothing behind pair
    5119, so that its bytes reach the third and fourth workgroup through gcarry."""
    _check_upload(asm, engine, oracle, tc.case_batch(case, n), what=f"{case} n={n}")


@pytest.mark.parametrize("n", tc.SIZES_C)
def test_c_carry_segments(asm, engine, oracle, n):
    """tails_carry_kernel with 1, 2 and 3 workgroups per segment and empty trailing segments."""
    if n == sum(tc.CUTS_G):
        hb, views = _whole_c(oracle)
    else:
        hb, views = tc.case_batch("C", n), None
    batch = _check_upload(asm, engine, oracle, hb, views, what=f"C n={n}")
    _check_greedy(asm, engine, oracle, hb, batch)


@pytest.mark.parametrize("case", ["D-eroding", "D-reads-empty", "D-refs-empty"])
def test_d_partial_overwrites_and_one_side(asm, engine, oracle, case):
    """Partial overwrites of many ages across every kind of seam; one side that nothing is ever written on (the 'nothing
    written' identity all the way through both scans) next to a side that carries, either way round."""
    hb = tc.case_batch(case, tc.N_D)
    views = oracle.greedy_views(hb, 0)
    if case.startswith("D-re"):
        assert not views[:, 0 if case == "D-reads-empty" else 1].any()
    batch = _check_upload(asm, engine, oracle, hb, views, what=case)
    _check_greedy(asm, engine, oracle, hb, batch)


@pytest.mark.parametrize("n", [1, 10, 11, 5121, 163841])
@pytest.mark.parametrize("start", ["random", "none"])
def test_e_empty_batch_permutes_the_state(asm, engine, oracle, n, start):
    """Empty strings only: every pair sees the initial state, permuted -- the carry-in alone, through s_init's ballot layout."""
    hb = tc.all_empty(n)
    state = np.random.default_rng(n).integers(0, 4, 256).astype(np.uint8) if start == "random" else None
    views = _views_from(oracle, hb, state)
    if state is not None:
        assert np.array_equal(tc.LUT[views[0].reshape(-1)], state) and (state != 0).sum() > 128
        if n > 1:
            assert np.array_equal(views[1], views[0][:, tc.SRC])
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    engine.resolve_tails(batch, state)
    _compare(hb, views, batch, f"E n={n} state={start}")


@pytest.mark.parametrize("kind", ["ragged", "bucketed"])
def test_f_tails_meet_bucketed_planes(asm, engine, oracle, kind):
    """Tails are made in input order and ORed in where pos sends the pair: several width classes; granules >= 1 stay clean;
    strings beyond 128 characters take no tail."""
    if kind == "ragged":
        hb = random_ragged_batch(asm, 41, 12000, 0, 200)
    else:
        hb = asm.generate_pairs(asm.workload("C5")[0], 41, 12000)
    batch = engine.upload(hb, asm.GREEDY_SEQUENTIAL)
    _, _, order = batch.download_planes()
    assert not np.array_equal(order, np.arange(hb.n))         # really bucketed
    _compare(hb, oracle.greedy_views(hb, 0), batch, f"F {kind}")


def test_g_shard_chain_at_scale(asm, engine, oracle):
    """Batch C cut into shards: summary per shard on the device, folded on the host, each shard resolved from the folded
    state; every shard's planes are the whole batch's rows."""
    hb, whole = _whole_c(oracle)
    state, lo = np.zeros(256, np.uint8), 0
    for n in tc.CUTS_G:
        part = hb.slice(lo, lo + n)
        batch = engine.upload(part, asm.GREEDY_CLEAN)
        summary = engine.tail_summary(batch)
        assert np.array_equal(summary, oracle.tail_summary(part)), f"summary of [{lo}, {lo + n})"
        engine.resolve_tails(batch, state)
        if n:
            _compare(part, whole[lo:lo + n], batch, f"G shard [{lo}, {lo + n})")
        state = asm.tail_state_advance(state, summary, n)
        lo += n
    _views_from(oracle, hb)
    assert lo == hb.n and np.array_equal(state, tc.LUT[oracle.final_buffers()])


@pytest.mark.parametrize("wl", ["mixed", "C5"])
def test_h_device_generator(asm, engine, oracle, wl):
    """A batch generated on the device goes through the same resolver: mixed lengths in one bucket, and C5 in several."""
    cfg = asm.GenConfig.exact(32, 30, 0.10, length_hi=128) if wl == "mixed" else asm.workload("C5")[0]
    hb = asm.generate_pairs(cfg, 17, 12000)
    views = oracle.greedy_views(hb, 0)
    _compare(hb, views, engine.generate(cfg, 17, hb.n, asm.GREEDY_SEQUENTIAL), f"H {wl} generate")
    _compare(hb, views, engine.upload(hb, asm.GREEDY_SEQUENTIAL), f"H {wl} upload")


def test_i_repacking_accumulates_nothing(asm, engine, oracle):
    hb = tc.case_batch("B", 5121)
    batch = _check_upload(asm, engine, oracle, hb, what="I")
    first = batch.download_planes()[0]
    for _ in range(2):
        engine.pack_async(batch)
    engine.synchronize()
    assert np.array_equal(batch.download_planes()[0], first)
    _compare(hb, oracle.greedy_views(hb, 0), batch, "I repacked")
