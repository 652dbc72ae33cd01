"""tests/cigar_row_cases.py on the CPU: the helpers on hand-written strings, and — with the oracle alone — that every input builder
delivers what tests/test_gpu_cigar_rows.py relies on: run counts below, at and above each cap of the ladder, at least a quarter of
the Greedy rows truncated and a quarter not at the median cap, R >= 256 for subst_comb(511), NW distances inside the band margin
C - 3 where the banded pass is meant to answer and beyond it where the full matrix is.  Also the search for a Greedy input that
saturates the byte count (none: see the module docstring of cigar_row_cases), and decode_cigars' refusal of rows not known whole."""
import numpy as np
import pytest

from tests import cigar_row_cases as cr


def E(count, op):
    return count << 3 | "MID=X".index(op)


def test_encode_and_expect_row():
    assert cr.encode("22M1D50M1D28M") == [E(22, "M"), E(1, "D"), E(50, "M"), E(1, "D"), E(28, "M")]
    assert cr.encode("3=1X2I4D100=") == [E(3, "="), E(1, "X"), E(2, "I"), E(4, "D"), E(100, "=")]
    assert cr.encode("") == [] and cr.encode("128M") == [1024] and cr.encode("1I") == [9]
    for bad in ("M", "3", "3S", "3M4", "3M 4I", "-3M", "0M", "9000M"):
        with pytest.raises(ValueError):
            cr.encode(bad)
    c = "5M1I7M2D9M"
    full = [E(5, "M"), E(1, "I"), E(7, "M"), E(2, "D"), E(9, "M")]
    assert cr.expect_row(c, 1) == ([E(5, "M")], 5) and cr.expect_row(c, 4) == (full[:4], 5)
    assert cr.expect_row(c, 5) == (full, 5) and cr.expect_row(c, 6) == (full, 5) and cr.expect_row("", 3) == ([], 0)
    assert cr.expect_row(c, 2, reverse=True) == ([E(9, "M"), E(2, "D")], 5) and cr.expect_row(c, 9, reverse=True) == (full[::-1], 5)
    comb = "1=1X" * 150  # 300 runs: the count saturates, the prefix is cap long
    for cap in (254, 255, 256, 300, 301):
        row, nops = cr.expect_row(comb, cap)
        assert nops == 255 and len(row) == min(cap, 300) and row[:2] == [E(1, "="), E(1, "X")]
    assert cr.expect_row("1=1X" * 127, 255) == ([E(1, "="), E(1, "X")] * 127, 254)
    assert cr.expect_row("1=1X" * 127 + "1=", 255)[1] == 255  # 255 runs read as "255 or more"
    full, R = cr.expect_matrix(["5M1I7M", "", "3="], reverse=True)
    assert R.tolist() == [3, 0, 1] and full.tolist() == [[E(7, "M"), E(1, "I"), E(5, "M")], [0, 0, 0], [E(3, "="), 0, 0]]
    assert cr.cap_ladder([1, 5, 9, 12, 31]) == [1, 2, 9, 30, 31, 32] and cr.cap_ladder([1, 1]) == [1, 2]
    assert cr.split_at([1, 2, 3, 4], 2) == (0.5, 0.5)


def test_decode_cigars_refuses_rows_not_known_whole(asm):
    ops = np.zeros((3, 4), np.uint16)
    ops[0, :2] = [E(5, "M"), E(1, "I")]
    ops[1] = [E(1, "="), E(1, "X"), E(2, "="), E(1, "D")]
    ops[2, :1] = [E(9, "M")]
    nops = np.array([2, 6, 1], np.uint8)
    assert asm.cigar_rows_truncated(nops, 4).tolist() == [False, True, False]
    assert asm.cigar_rows_truncated(np.array([254, 255], np.uint8), 255).tolist() == [False, True]
    assert asm.cigar_rows_truncated(np.array([254, 255], np.uint8), 300).tolist() == [False, True]
    with pytest.raises(ValueError, match="truncated"):
        asm.decode_cigars(ops, nops, 4)
    assert asm.decode_cigars(ops, nops, 4, truncated="none") == ["5M1I", None, "9M"]
    assert asm.decode_cigars(ops, nops, 4, truncated="prefix") == ["5M1I", "1=1X2=1D", "9M"]
    assert asm.decode_cigars(ops, nops, 4, reverse=True, truncated="prefix")[1] == "1D2=1X1="
    nops[1] = 4
    assert asm.decode_cigars(ops, nops, 4) == ["5M1I", "1=1X2=1D", "9M"]
    # the saturated count, at a cap that holds 255 entries and at one that holds more
    for cap in (255, 256):
        wide = np.full((2, cap), E(1, "="), np.uint16)
        with pytest.raises(ValueError, match="255"):
            asm.decode_cigars(wide, np.array([254, 255], np.uint8), cap)
        got = asm.decode_cigars(wide, np.array([254, 255], np.uint8), cap, truncated="none")
        assert got[0] == "1=" * 254 and got[1] is None
    with pytest.raises(ValueError):
        asm.decode_cigars(ops, nops, 4, truncated="whatever")


def _greedy_R(oracle, hb, k, pen, mode):
    x, o, e = pen
    return np.array([cr.run_count(c) for c in oracle.greedy(hb, k, x, o, e, mode=mode, cigars=True)[1]])


def _consumes(cigar, ops):
    return sum(v >> 3 for v in cr.encode(cigar) if "MID=X"[v & 7] in ops)


@pytest.mark.parametrize("name", cr.GREEDY_INPUTS)
def test_greedy_inputs_fill_their_rows(asm, oracle, name):
    """Every Greedy case of the GPU test: rows below, at and above each cap of its ladder, and the quarter / quarter split at the
    median cap"""
    hb = cr.INPUTS[name](asm)
    assert hb.n == cr.N_PAIRS == 2 * 512 + 37
    for cid, k, pen, mode, _ in cr.GREEDY_CASES:
        R = _greedy_R(oracle, hb, k, pen, mode)
        ladder = cr.cap_ladder(R)
        med, top = int(np.median(R)), int(R.max())
        assert ladder == [1, 2, med, top - 1, top, top + 1] and top < 255, (cid, ladder)
        cut, whole = cr.split_at(R, med)
        assert cut >= 0.25 and whole >= 0.25, (cid, med, cut, whole)
        for cap in ladder:  # below, at and above, as far as a cap next to the maximum can have them
            assert (R < cap).any() or cap == 1, (cid, cap)
            assert (R == cap).any() or cap in (top - 1, top + 1), (cid, cap)
            assert (R > cap).any() or cap >= top, (cid, cap)


def test_coverage_inputs_split_and_reach_both_verdict_paths(asm, oracle):
    for cid, source, pen, window in cr.COVER_CASES:
        hb = cr.INPUTS[source](asm)
        R = _greedy_R(oracle, hb, cr.COVER_K, pen, 1)
        cut, whole = cr.split_at(R, int(np.median(R)))
        assert cut >= 0.25 and whole >= 0.25, (cid, cut, whole)
        dist = cr.nw_cigar_wide(oracle, hb)[0]  # unit-cost distance: what the banded pass looks at
        if pen != (1, 1, 1):
            continue  # every pair through the full matrix
        banded = dist <= window // 2 - 3
        if "banded" in cid:
            assert banded.mean() >= 0.25, (cid, float(banded.mean()))
        if cid == "noisy_c2_w32":
            assert (~banded).mean() >= 0.9  # and here nearly all are handed over
        # truncated rows on both sides of the hand-over where both exist
        if 0.05 < banded.mean() < 0.95:
            assert (R[banded] > np.median(R)).any() and (R[~banded] > np.median(R)).any(), cid


def test_indel_comb_spreads_run_counts(asm, oracle):
    hb = cr.INPUTS["indel_comb"](asm)
    m, n = hb.lengths()
    assert int(np.abs(m.astype(int) - n.astype(int)).max()) <= 1  # inside the smallest band
    for k in (1, 3):
        R = _greedy_R(oracle, hb, k, (1, 1, 1), 1)
        med, top = int(np.median(R)), int(R.max())
        cut, whole = cr.split_at(R, med)
        assert cut >= 0.25 and whole >= 0.25 and top >= 15, (k, med, top)
        for cap in (1, med):  # (no row of this input has two runs: its switches sit between runs)
            assert (R == cap).any() and (R > cap).any(), (k, cap)
        cigs = oracle.greedy(hb, k, mode=1, cigars=True)[1]
        assert sum("I" in c and "D" in c for c in cigs) > hb.n // 2


def test_nw_inputs(asm, oracle):
    """subst_comb: R = length exactly (>= 256 at 511); sparse_subst: inside the margin of the window meant to answer, outside the
    other's; every oracle CIGAR consumes both strings whole (nothing was cut from a long string)"""
    for cid, source, pen, window in cr.NW_CASES:
        hb = cr.INPUTS[source](asm)
        dist, cig = cr.nw_cigar_wide(oracle, hb, *pen)
        m, n = hb.lengths()
        for i in range(0, hb.n, 7):
            assert (_consumes(cig[i], "=XI"), _consumes(cig[i], "=XD")) == (int(m[i]), int(n[i])), (cid, i)
        R = np.array([cr.run_count(c) for c in cig])
        margin = window // 2 - 3
        if cid.startswith("comb"):
            L = int(m[0])
            assert (R == L).all() and (dist == L // 2).all() and all(c == ("1=1X" * L)[:2 * L] for c in cig[:50]), cid
        if cid == "comb511_w64":
            assert int(R.min()) == 511 >= 256
        if cid == "sparse12_w32":
            assert int(dist.max()) <= 12 <= margin == 13 and (R == 25).all()
        if cid == "sparse28_w64":
            assert int(dist.max()) <= 28 <= margin == 29 and int(R.max()) == 57
        if cid == "sparse28_w32_handed_over":
            assert int(dist.min()) > margin == 13
        if cid.startswith("ragged"):
            assert int(m.min()) == 129 and int(m.max()) == 256 and (dist <= margin).any() and (dist > margin).any()
            med = int(np.median(R))
            assert (R < med).any() and (R == med).any() and (R > med).any() and (R == 1).any(), cid
        if cid == "noisy_c2_231":
            assert int(R.min()) >= 3 and len(set(R.tolist())) > 10


def test_no_greedy_input_saturates_the_count(asm, oracle):
    """The search the module docstring of cigar_row_cases reports: full combs at periods 1..8, four lengths, eight bands."""
    best = (0, None)
    for length in (100, 128, 200, 511):
        for period in range(1, 9):
            hb = cr.indel_comb(asm, length, period, n=64, seed=period, ragged=False)
            for k in (1, 2, 3, 5, 10, 17, 32, 40):
                top = int(_greedy_R(oracle, hb, k, (1, 1, 1), 1).max())
                if top > best[0]:
                    best = (top, (length, period, k))
    assert best[0] == cr.GREEDY_MAX_R_FOUND < 255, best


def test_cigar_format_refuses_rows_not_known_whole(asm):
    """asm_cigar_format (host helper, no device): ASM_EUNSUPPORTED (-4) when nops > cap or nops == 255; the stored entries are
    written either way"""
    import ctypes

    lib = asm.load_library()
    text = ctypes.create_string_buffer(8192)
    comb = "1=1X" * 300
    for cap in (254, 255, 256, 600):
        row, nops = cr.expect_row(comb, cap)
        arr = np.array(row, np.uint16)
        assert nops == 255 and lib.asm_cigar_format(arr.ctypes.data, nops, cap, text, len(text)) == -4, cap
        assert text.value.decode() == comb[:2 * min(cap, 255)]
    row, nops = cr.expect_row("1=1X" * 127, 254)
    arr = np.array(row, np.uint16)
    assert nops == 254 and lib.asm_cigar_format(arr.ctypes.data, nops, 254, text, len(text)) == 0 and text.value.decode() == "1=1X" * 127
    assert lib.asm_cigar_format(arr.ctypes.data, 9, 5, text, len(text)) == -4 and text.value.decode() == "1=1X1=1X1="
