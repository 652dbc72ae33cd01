"""The pair aligners' fixed-width CIGAR rows on the device, full and overfull: every producer (CigarSink in the six Greedy families,
nw_trace_cover_kernel<.., 32|64>, nw_trace_affine_kernel) at caps below, at and above the run counts R of its input, and the reader
of the Greedy rows (cover_verdict) on rows that did not fit.

Every expectation is the oracle's CIGAR string cut at cap (tests/cigar_row_cases.py: the first min(R, cap) entries, nops =
min(R, 255)); the inputs and what they must deliver are checked without a GPU in tests/test_cigar_rows_host.py.  The rows and counts
live in caller-owned buffers between guard zones filled with a byte no entry can equal (0xA5: op 5 does not exist), so a store
past a full row shows in the next pair's row (compared) or in a guard (compared byte for byte).

Not tested here, because no input can reach it: a Greedy row that saturates the count (see cigar_row_cases), and a banded
traceback that leaves its window after writing part of a row (a distance inside the margin C - 3 keeps the path, and the cells the
walk inspects, inside the window) — the pairs handed over here are refused by the banded pass before it writes."""
import ctypes

import numpy as np
import pytest

from tests import cigar_row_cases as cr
from tests.util import engine_with

pytestmark = pytest.mark.gpu

GUARD = 512  # bytes before and after each buffer
FILL = 0xA5
FILL16 = 0xA5A5


class Guarded:
    """A device buffer of nbytes between two guard zones, all of it filled with FILL"""

    def __init__(self, eng, nbytes):
        self.eng, self.nbytes = eng, int(nbytes)
        self.total = self.nbytes + 2 * GUARD
        self.base = eng.malloc(self.total)
        self.ptr = self.base + GUARD
        self.refill()

    def refill(self):
        self.eng.memset_async(self.base, FILL, self.total)

    def read(self, dtype, count):
        """(payload as dtype[count], number of guard bytes that changed)"""
        raw = self.eng.to_host(self.base, self.total, np.uint8)
        body = raw[GUARD:GUARD + self.nbytes]
        spoiled = int((raw[:GUARD] != FILL).sum() + (raw[GUARD + self.nbytes:] != FILL).sum())
        used = count * np.dtype(dtype).itemsize
        assert used <= self.nbytes
        spoiled += int((body[used:] != FILL).sum())  # slack behind the payload of this run counts as guard
        return body[:used].view(dtype).copy(), spoiled

    def free(self):
        self.eng.free(self.base)


@pytest.fixture(scope="module")
def inputs(asm):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = cr.INPUTS[key](asm)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def known(oracle, inputs):
    """The oracle's answers, computed once per (input, penalties[, k, mode]) and shared, never changed"""
    cache = {}

    def memo(key, fn):
        if key not in cache:
            cache[key] = fn()
        return cache[key]

    class Known:
        def greedy(self, source, k, pen, mode=1):
            """(costs, CIGAR strings, rows uint16[n][max R], R)"""
            def make():
                cost, cig = oracle.greedy(inputs(source), k, *pen, mode=mode, cigars=True)
                return (cost, cig) + cr.expect_matrix(cig)
            return memo(("greedy", source, k, pen, mode), make)

        def nw(self, source, pen):
            """(penalties, CIGAR strings, rows in traceback order, R)"""
            def make():
                p, cig = cr.nw_cigar_wide(oracle, inputs(source), *pen)
                return (p, cig) + cr.expect_matrix(cig, reverse=True)
            return memo(("nw", source, pen), make)

        def cover(self, source, pen):
            """the verdicts, or None where a CIGAR string is longer than the binding's coverage call holds (767 characters)"""
            def make():
                gcig, ncig = self.greedy(source, cr.COVER_K, pen)[1], self.nw(source, pen)[1]
                return oracle.coverage(inputs(source), gcig, 1, ncig, 3) if max(len(c) for c in ncig) < 760 else None
            return memo(("cover", source, pen), make)

    return Known()


@pytest.fixture(scope="module")
def wide_engine(asm):
    eng = engine_with(asm, "ASM_WAVE")
    yield eng
    eng.close()


def check_rows(ctx, ops, nops, full, R, cap):
    """nops == min(R, 255) and the first min(R, cap) entries are the oracle's, for every pair"""
    n = R.size
    want_nops = np.minimum(R, cr.NOPS_MAX)
    bad = np.nonzero(nops.astype(np.int64) != want_nops)[0]
    assert bad.size == 0, (ctx, "nops", bad.size, bad[:5], nops[bad[:5]], want_nops[bad[:5]])
    width = min(cap, full.shape[1])
    keep = np.arange(width)[None, :] < np.minimum(R, cap)[:, None]
    diff = (ops.reshape(n, cap)[:, :width] != full[:, :width]) & keep
    bad = np.nonzero(diff.any(axis=1))[0]
    assert bad.size == 0, (ctx, "entries", bad.size, bad[:5], ops.reshape(n, cap)[bad[0], :width], full[bad[0], :width])


# ---------------------------------------------------------------------------------------------------------------------------
# Greedy rows, every family
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", cr.GREEDY_INPUTS)
@pytest.mark.parametrize("case", cr.GREEDY_CASES, ids=[c[0] for c in cr.GREEDY_CASES])
def test_greedy_rows_at_every_cap(asm, engine, wide_engine, known, inputs, case, source):
    cid, k, (x, o, e), mode, switch = case
    eng = wide_engine if switch == "ASM_WAVE" else engine
    hb = inputs(source)
    n = hb.n
    want_cost, _, full, R = known.greedy(source, k, (x, o, e), mode)
    ladder = cr.cap_ladder(R)
    cut, whole = cr.split_at(R, int(np.median(R)))
    assert cut >= 0.25 and whole >= 0.25  # (tests/test_cigar_rows_host.py pins this on the CPU)
    params = asm.Params.default(k=k, x=x, o=o, e=e)
    batch = eng.upload(hb, mode)
    d_pen, d_ops, d_nops = Guarded(eng, 4 * n), Guarded(eng, 2 * n * max(ladder)), Guarded(eng, n)
    try:
        for cap in ladder:
            for g in (d_pen, d_ops, d_nops):
                g.refill()
            eng.greedy_cigar_async(batch, params, d_pen.ptr, d_ops.ptr, cap, d_nops.ptr)
            cost, s0 = d_pen.read(np.int32, n)
            ops, s1 = d_ops.read(np.uint16, n * cap)
            nops, s2 = d_nops.read(np.uint8, n)
            ctx = (cid, source, "cap", cap)
            bad = np.nonzero(cost != want_cost)[0]
            assert bad.size == 0, (ctx, "cost", bad.size, bad[:5], cost[bad[:5]], want_cost[bad[:5]])
            check_rows(ctx, ops, nops, full, R, cap)
            assert (s0, s1, s2) == (0, 0, 0), (ctx, "guard bytes changed behind penalties / rows / counts", s0, s1, s2)
            # what a producer does not store it does not touch: the row's tail still holds the fill
            tail = np.arange(cap)[None, :] >= np.minimum(R, cap)[:, None]
            assert (ops.reshape(n, cap)[tail] == FILL16).all(), (ctx, "entries behind the last run were written")
    finally:
        for g in (d_pen, d_ops, d_nops):
            g.free()


# ---------------------------------------------------------------------------------------------------------------------------
# NW rows, both tracebacks and both windows
# ---------------------------------------------------------------------------------------------------------------------------
def run_coverage(eng, batch, params, n, window, greedy_cap, nw_cap, bufs):
    """Greedy rows at greedy_cap, then asm_coverage with NW rows at nw_cap, all in guarded caller buffers.  -> dict"""
    for g in bufs.values():
        g.refill()
    eng.memset_async(bufs["cnt"].ptr, 0, 16)
    eng.greedy_cigar_async(batch, params, bufs["pen"].ptr, bufs["gops"].ptr, greedy_cap, bufs["gn"].ptr)
    eng._chk(eng.lib.asm_coverage(eng.h, batch.ptr, ctypes.byref(params), bufs["gops"].ptr, greedy_cap, bufs["gn"].ptr, window, bufs["cov"].ptr,
                                  bufs["nwo"].ptr, nw_cap, bufs["nwn"].ptr, bufs["cnt"].ptr))
    out, spoiled = {}, {}
    for key, dtype, count in (("pen", np.int32, n), ("gops", np.uint16, n * greedy_cap), ("gn", np.uint8, n), ("cov", np.uint8, n),
                              ("nwo", np.uint16, n * nw_cap), ("nwn", np.uint8, n), ("cnt", np.uint64, 2)):
        out[key], spoiled[key] = bufs[key].read(dtype, count)
    out["spoiled"] = spoiled
    return out


def coverage_buffers(eng, n, greedy_cap_max, nw_cap_max):
    return {"pen": Guarded(eng, 4 * n), "gops": Guarded(eng, 2 * n * greedy_cap_max), "gn": Guarded(eng, n), "cov": Guarded(eng, n),
            "nwo": Guarded(eng, 2 * n * nw_cap_max), "nwn": Guarded(eng, n), "cnt": Guarded(eng, 16)}


GREEDY_CAP_WHOLE = 128  # above every Greedy run count of these inputs (cigar_row_cases.GREEDY_MAX_R_FOUND), below 255


@pytest.mark.parametrize("case", cr.NW_CASES, ids=[c[0] for c in cr.NW_CASES])
def test_nw_rows_at_every_cap(asm, engine, known, inputs, case):
    cid, source, (x, o, e), window = case
    hb = inputs(source)
    n = hb.n
    _, _, full, R = known.nw(source, (x, o, e))
    ladder = cr.cap_ladder(R)
    if cid.startswith("comb511"):
        assert int(R.min()) == 511
        ladder = sorted(set(ladder) | {254, 255, 256})  # around the saturated count: nops == 255 at each, the prefix cap long
    params = asm.Params.default(k=cr.COVER_K, x=x, o=o, e=e)
    gcost = known.greedy(source, cr.COVER_K, (x, o, e))[0]
    want_cover = known.cover(source, (x, o, e))  # (None for the 511-run rows: they go without the verdict comparison)
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    bufs = coverage_buffers(engine, n, GREEDY_CAP_WHOLE, max(ladder))
    try:
        for cap in ladder:
            got = run_coverage(engine, batch, params, n, window, GREEDY_CAP_WHOLE, cap, bufs)
            ctx = (cid, "window", window, "nw_cap", cap)
            assert np.array_equal(got["pen"], gcost), (ctx, "Greedy cost")
            check_rows(ctx, got["nwo"], got["nwn"], full, R, cap)
            assert not any(got["spoiled"].values()), (ctx, "guard bytes changed", got["spoiled"])
            # the NW cap does not touch the verdicts: the Greedy rows are whole
            assert int(got["cnt"][1]) == 0 and int(got["cnt"][0]) == int((got["cov"] == 1).sum()) and not (got["cov"] == 2).any(), ctx
            if want_cover is not None:
                assert np.array_equal(got["cov"], want_cover), (ctx, "verdicts")
            if cid.startswith("comb511") and cap in (254, 255, 256):
                assert (got["nwn"] == 255).all() and (got["nwo"].reshape(n, cap) != FILL16).all(), ctx
    finally:
        for g in bufs.values():
            g.free()


# ---------------------------------------------------------------------------------------------------------------------------
# Coverage on truncated Greedy rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.COVER_CASES, ids=[c[0] for c in cr.COVER_CASES])
def test_coverage_of_truncated_greedy_rows_is_unknown(asm, engine, known, inputs, case):
    """A pair whose Greedy row did not fit gets COVER_UNKNOWN and counts in counters[1], not a verdict from the stored prefix; every
    other pair of the same launch gets the oracle's verdict; with a sufficient cap nothing is unknown."""
    cid, source, (x, o, e), window = case
    hb = inputs(source)
    n = hb.n
    _, _, gfull, RG = known.greedy(source, cr.COVER_K, (x, o, e))
    _, _, nfull, RN = known.nw(source, (x, o, e))
    want = known.cover(source, (x, o, e))
    params = asm.Params.default(k=cr.COVER_K, x=x, o=o, e=e)
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    median_cap, nw_cap = int(np.median(RG)), int(RN.max()) + 1
    bufs = coverage_buffers(engine, n, GREEDY_CAP_WHOLE, nw_cap)
    try:
        for greedy_cap in (median_cap, GREEDY_CAP_WHOLE):
            got = run_coverage(engine, batch, params, n, window, greedy_cap, nw_cap, bufs)
            ctx = (cid, "window", window, "greedy_cap", greedy_cap)
            check_rows(ctx, got["gops"], got["gn"], gfull, RG, greedy_cap)
            check_rows(ctx, got["nwo"], got["nwn"], nfull, RN, nw_cap)  # every pair keeps its NW row, known-truncated or not
            assert not any(got["spoiled"].values()), (ctx, "guard bytes changed", got["spoiled"])
            gn = got["gn"].astype(np.int64)
            cut = (gn > greedy_cap) | ((gn == 255) & (greedy_cap >= 255))
            assert np.array_equal(cut, RG > greedy_cap)
            cover = got["cov"]
            print(ctx, "known truncated", int(cut.sum()), "of", n, "cover==2", int((cover == 2).sum()), "counters", got["cnt"].tolist(),
                  "verdicts differing from the oracle among the rest", int((cover[~cut] != want[~cut]).sum()))
            bad = np.nonzero(cover[cut] != 2)[0]
            assert bad.size == 0, (ctx, "truncated rows with a verdict", bad.size, "of", int(cut.sum()), cover[cut][bad[:8]])
            bad = np.nonzero(cover[~cut] != want[~cut])[0]
            assert bad.size == 0, (ctx, "verdicts", bad.size, bad[:5])
            assert int(got["cnt"][0]) == int((cover == 1).sum()) and int(got["cnt"][1]) == int((cover == 2).sum()) == int(cut.sum()), \
                (ctx, got["cnt"].tolist(), int((cover == 1).sum()), int((cover == 2).sum()))
            if greedy_cap == median_cap:
                assert cut.mean() >= 0.25 and (~cut).mean() >= 0.25
            else:
                assert not cut.any() and np.array_equal(cover, want)
    finally:
        for g in bufs.values():
            g.free()


def test_coverage_of_a_saturated_greedy_count_is_unknown(asm, engine, known, inputs):
    """greedy_cap >= 255: a count of 255 means "255 or more", so such a row is known truncated whatever the cap.  No Greedy input
    saturates the count (cigar_row_cases), so the rows are the device's own with some counts set to 255 by hand: those pairs, and
    only those, become unknown — through the banded verdict and through the full matrix's."""
    hb = inputs("noisy_c2")
    n = hb.n
    marked = np.zeros(n, bool)
    marked[::5] = True
    for pen, window in (((1, 1, 1), 64), ((1, 1, 1), 32), ((2, 3, 1), 64)):
        x, o, e = pen
        want = known.cover("noisy_c2", pen)
        params = asm.Params.default(k=cr.COVER_K, x=x, o=o, e=e)
        batch = engine.upload(hb, asm.GREEDY_CLEAN)
        for cap in (255, 256):
            d_pen, d_ops, d_nops, d_cov, d_cnt = (engine.malloc(s) for s in (4 * n, 2 * n * cap, n, n, 16))
            try:
                engine.greedy_cigar_async(batch, params, d_pen, d_ops, cap, d_nops)
                nops = engine.to_host(d_nops, n, np.uint8)
                assert int(nops.max()) < 255
                nops[marked] = 255
                engine._chk(engine.lib.asm_memcpy_h2d(engine.h, d_nops, nops.ctypes.data, n))
                engine.memset_async(d_cnt, 0, 16)
                engine._chk(engine.lib.asm_coverage(engine.h, batch.ptr, ctypes.byref(params), d_ops, cap, d_nops, window, d_cov, None, 0,
                                                    None, d_cnt))
                cover, cnt = engine.to_host(d_cov, n, np.uint8), engine.to_host(d_cnt, 2, np.uint64)
                assert (cover[marked] == 2).all() and np.array_equal(cover[~marked], want[~marked]), (pen, window, cap)
                assert cnt.tolist() == [int((cover == 1).sum()), int(marked.sum())], (pen, window, cap, cnt.tolist())
            finally:
                for p in (d_pen, d_ops, d_nops, d_cov, d_cnt):
                    engine.free(p)


def test_engine_coverage_marks_and_nw_cap(asm, engine, oracle, known, inputs):
    """Engine.coverage: nw_cap apart from cap; a truncated row is None in the decoded lists, never a shortened string; and
    greedy_with_cigar raises where a row did not fit.  asm_cigar_format refuses the same rows."""
    hb = inputs("noisy_c2")
    params = asm.Params.default(k=cr.COVER_K)
    gcost, gcig, _, RG = known.greedy("noisy_c2", cr.COVER_K, (1, 1, 1))
    _, ncig, _, RN = known.nw("noisy_c2", (1, 1, 1))
    want = known.cover("noisy_c2", (1, 1, 1))
    batch = engine.upload(hb, asm.GREEDY_CLEAN)
    cap, nw_cap = int(np.median(RG)), int(np.median(RN))
    got = engine.coverage(batch, params, window=64, cap=cap, want_nw_cigars=True, nw_cap=nw_cap)
    assert np.array_equal(got["greedy_nops"], RG) and np.array_equal(got["nw_nops"], RN)
    assert got["greedy_cigars"] == [c if r <= cap else None for c, r in zip(gcig, RG)]
    assert got["nw_cigars"] == [c if r <= nw_cap else None for c, r in zip(ncig, RN)]
    assert np.array_equal(got["cover"], np.where(RG > cap, 2, want)) and got["undetermined"] == int((RG > cap).sum())
    assert got["covered"] == int((got["cover"] == 1).sum())
    whole = engine.coverage(batch, params, window=64, cap=64, want_nw_cigars=True)  # nw_cap defaults to cap
    assert whole["greedy_cigars"] == gcig and whole["nw_cigars"] == ncig and np.array_equal(whole["cover"], want)
    assert whole["undetermined"] == 0
    with pytest.raises(ValueError, match="truncated"):
        engine.greedy_with_cigar(batch, params, cap=cap)
    cost, cig, nops = engine.greedy_with_cigar(batch, params, cap=int(RG.max()))
    assert cig == gcig and np.array_equal(cost, gcost)
    # asm_cigar_format on a device row that saturated (subst_comb(511): R = 511) and on one that is whole
    comb = inputs("comb511")
    sub = asm.HostBatch.from_strings([comb.pair(i) for i in range(3)])
    text = ctypes.create_string_buffer(8192)
    for nw in (255, 256, 600):
        out = engine.coverage(engine.upload(sub, asm.GREEDY_CLEAN), params, window=64, cap=64, want_nw_cigars=True, nw_cap=nw)
        assert out["nw_nops"].tolist() == [255] * 3 and out["nw_cigars"] == [None] * 3
        row = np.array(cr.expect_row(cr.nw_cigar_wide(oracle, sub)[1][0], nw, reverse=True)[0], np.uint16)
        rc = engine.lib.asm_cigar_format(row.ctypes.data, 255, nw, text, len(text))
        assert rc == -4, (nw, rc)  # ASM_EUNSUPPORTED
    row = np.array(cr.encode("1=1X" * 127), np.uint16)
    assert engine.lib.asm_cigar_format(row.ctypes.data, 254, 254, text, len(text)) == 0 and text.value.decode() == "1=1X" * 127
