"""The ingest corpus (tests/seq_text_cases.py) on the CPU: that the reference parser reads the harness's format as the project
defines it, and that every text holds the edge it was built for — proven from the text itself, so that a builder changed later
cannot quietly stop reaching the slice, wave and tile edges of csrc/asm_ingest.h or the staging branch of asm_stream_seq_file.
No GPU needed; the device parser and the streamed path are in test_gpu_ingest_edges.py."""
import numpy as np
import pytest

from tests import seq_text_cases as stc
from tests.seq_text_cases import SLICE, TILE, WAVE
from tests.util import leap_defined, random_ragged_batch


def _pairs(hb):
    return [(hb.reads[hb.read_off[i]:hb.read_off[i + 1]].tobytes(), hb.refs[hb.ref_off[i]:hb.ref_off[i + 1]].tobytes())
            for i in range(hb.n)]


def _newlines(text):
    return np.flatnonzero(np.frombuffer(text, np.uint8) == 0x0A)


def _same(got, want):
    assert got.n == want.n
    assert np.array_equal(got.read_off, want.read_off) and np.array_equal(got.ref_off, want.ref_off)
    assert np.array_equal(got.reads, want.reads) and np.array_equal(got.refs, want.refs)


# ---- the parser ----
def test_parse_equals_the_package_reader_on_lf_files_with_markers(asm, tmp_path):
    hb = random_ragged_batch(asm, 3, 500, 0, 300)
    path = str(tmp_path / "ragged.seq")
    hb.write_seq_file(path)
    with open(path, "rb") as fh:
        text = fh.read()
    _same(stc.parse(text), asm.HostBatch.read_seq_file(path))
    _same(stc.parse(text), hb)
    _same(stc.parse(text[:-1]), hb)  # without the final newline
    cfg, _, _ = asm.workload("C5")
    hb = asm.generate_pairs(cfg, 0, 300)
    hb.write_seq_file(path)
    with open(path, "rb") as fh:
        _same(stc.parse(fh.read()), asm.HostBatch.read_seq_file(path))


@pytest.mark.parametrize("text,want,appended", [
    (b"", [], 0),
    (b"\n", [(b"", b"")], 1),                                 # one line of zero bytes: an empty read, no reference line
    (b"\n\n\n", [(b"", b""), (b"", b"")], 1),                 # three lines: the second read has no reference line
    (b">ACGT\n<ACGA\n>TTTT", [(b"ACGT", b"ACGA"), (b"TTTT", b"")], 2),
    (b">AC\r\n<AG\r\n", [(b"AC\r", b"AG\r")], 0),             # CRLF: the CR stays in the string
    (b">\n<\n", [(b"", b"")], 0),                             # markers alone
    (b"xA\x00\xffC\n>>a<\n", [(b"A\x00\xffC", b">a<")], 0),   # any first byte is the marker; the rest is kept as it is
    (b">ACGT\n<ACGA", [(b"ACGT", b"ACGA")], 1),               # an open last line, an even number of lines
])
def test_parse_by_hand(text, want, appended):
    hb = stc.parse(text)
    assert _pairs(hb) == want
    assert hb.read_off.dtype == np.uint32 and hb.reads.dtype == np.uint8 and hb.read_off.size == len(want) + 1
    assert stc.appended_newlines(text) == appended and stc.shipped_bytes(text) == len(text) + appended


def test_corpus_is_deterministic_and_named():
    assert tuple(c.name for c in stc.corpus()) == stc.NAMES and len(set(stc.NAMES)) == len(stc.NAMES)
    again = stc.newline_grid()
    assert again.text == stc.case("newline_grid").text
    text, name = again
    assert name == "newline_grid" and text == again.text


def test_corpus_sizes_and_string_lengths(asm):
    """No string is longer than the library takes (512).  Above LEAP's 256 — where the suite's rule tests.util.leap_defined leaves a
    pair out of the LEAP comparison — are lengths_mix and density_step, by design, and the 300-character lines of dense and
    far_max, which are counted here: three pairs and one pair.  Every other text keeps every pair in every comparison."""
    beyond = {}
    for text, name in stc.corpus():
        hb = stc.parsed(name)
        m, n = hb.lengths()
        longest = int(max(m.max(), n.max()))
        assert longest <= stc.MAX_LENGTH, name
        assert len(text) <= (1 << 20) + 4096, name
        if longest > stc.LEAP_MAX:
            beyond[name] = int((~leap_defined(hb)).sum())
        else:
            assert leap_defined(hb).all(), name
    assert set(beyond) == stc.BEYOND_LEAP
    assert beyond["dense"] == 3 and beyond["far_max"] == 1
    assert max(len(c.text) for c in stc.corpus()) >= 600_000 and stc.parsed("far_max").n == 300_000


# ---- every builder places what it promises ----
def test_newline_grid_hits_every_edge():
    case = stc.case("newline_grid")
    nl = _newlines(case.text)
    assert set(case.facts["targets"]) <= set(nl.tolist())
    assert 5 * TILE < len(case.text) < 5 * TILE + 1024
    assert {0, 1, 14, 15} <= set((nl % SLICE).tolist())
    for residue, period in ((WAVE - 1, WAVE), (0, WAVE), (TILE - 1, TILE), (0, TILE)):
        tiles = set((nl[nl % period == residue] // TILE).tolist())
        assert len(tiles - {0} if residue == 0 else tiles) >= 2, (residue, period, tiles)
    # a newline on the last byte of a wave and on the first byte of the next one, inside one tile; the same across a tile edge
    have = set(nl.tolist())
    assert any(p % WAVE == WAVE - 1 and p % TILE != TILE - 1 and p + 1 in have for p in have)
    assert sum(1 for p in have if p % TILE == TILE - 1 and p + 1 in have) >= 2
    # bytes 15 and 0 of neighbouring slices in the middle of a wave
    assert any(p % SLICE == SLICE - 1 and p % WAVE not in (WAVE - 1,) and p + 1 in have for p in have)
    m, n = stc.parsed("newline_grid").lengths()
    assert min(m.min(), n.min()) == 0 and max(m.max(), n.max()) <= 256


def test_dense_fills_whole_tiles_and_whole_slices():
    case = stc.case("dense")
    buf = np.frombuffer(case.text, np.uint8)
    whole = buf[:buf.size // TILE * TILE].reshape(-1, TILE)
    full_tiles = np.flatnonzero((whole == 0x0A).all(axis=1))
    assert full_tiles.size >= 4 and (np.diff(full_tiles) == 1).any(), full_tiles       # 4,096 newlines in a tile, two tiles running
    per_slice = (buf[:buf.size // SLICE * SLICE].reshape(-1, SLICE) == 0x0A).sum(axis=1)
    assert (per_slice == SLICE).sum() > 2 * TILE // SLICE and (per_slice == 0).sum() >= 3 * (300 // SLICE - 1)
    assert ((per_slice > 0) & (per_slice < SLICE)).any()                                 # and a slice that a run starts or ends in
    hb = stc.parsed("dense")
    m, n = hb.lengths()
    assert hb.n == case.facts["n_lines"] + 2 and sorted(m[m > 0].tolist() + n[n > 0].tolist()) == [300, 300, 300]
    assert m[0] == 300 and n[0] == 0 and n[n > 0].size == 1 and m[-1] == 300            # read, reference, read without reference


@pytest.mark.parametrize("total", stc.ENDS_TOTALS)
def test_ends_stop_where_they_claim(total):
    for open_line in (False, True):
        for odd in (False, True):
            case = stc.ends(total, open_line, odd)
            text = case.text
            assert len(text) == total and text.endswith(b"\n") != open_line
            lines = text.count(b"\n") + (1 if open_line else 0)
            assert lines % 2 == (1 if odd else 0)
            assert stc.appended_newlines(text) == int(open_line) + int(odd)
            assert stc.parsed(case.name).n == (lines + 1) // 2
    assert set(stc.ENDS_TOTALS) >= {4095, 4096, 4097, 8192} and any(t % SLICE == 0 and t % TILE for t in stc.ENDS_TOTALS)
    assert any(t % SLICE == SLICE - 1 and t % TILE != TILE - 1 for t in stc.ENDS_TOTALS)


def test_ends_4095_open_odd_appends_across_the_tile_edge():
    text = stc.case("ends_4095_open_odd").text
    assert len(text) == TILE - 1 and stc.appended_newlines(text) == 2  # the appended newlines are bytes 4,095 and 4,096
    hb = stc.parsed("ends_4095_open_odd")
    assert hb.lengths()[1][-1] == 0 and hb.lengths()[0][-1] > 0


def test_lengths_mix_puts_every_length_next_to_every_other():
    hb = stc.parsed("lengths_mix")
    want = [max(v, 0) for v in stc.MIX]
    m, n = hb.lengths()
    assert hb.n == len(want) ** 2
    assert m.tolist() == [a for a in want for _ in want] and n.tolist() == [b for _ in want for b in want]
    assert {0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 511, 512} == set(want)
    text = stc.case("lengths_mix").text
    assert text.startswith(b"\n\n") and b"\n>\n" in text and b"\n<\n" in text      # lines of zero bytes and markers alone, both sides
    assert b"\n\n<" in text and b"\n>\n\n" in text


def test_dirty_holds_the_bytes_it_names():
    case = stc.case("dirty")
    text = case.text
    lines = text.split(b"\n")
    assert lines[-1] == b"" and all(line.endswith(b"\r") for line in lines[:-1]) and len(lines) - 1 == 2 * case.facts["pairs"]
    hb = stc.parsed("dirty")
    assert hb.n == case.facts["pairs"]
    pairs = _pairs(hb)
    assert all(a.endswith(b"\r") and b.endswith(b"\r") for a, b in pairs)
    for side in (hb.reads, hb.refs):
        seen = set(side.tolist())
        assert 0 in seen and sum(1 for v in seen if v >= 0x80) >= 64
        assert {ord(">"), ord("<"), ord("a"), ord("c"), ord("g"), ord("t"), ord("\r")} <= seen and 0x0A not in seen
    m, n = hb.lengths()
    assert {1, 2, 63, 64, 65, 255, 256} <= set(m.tolist()) and max(m.max(), n.max()) == 256
    assert {line[:1] for line in lines[:-1]} == {b">", b"<", b"\x00", b"\xff"}


def test_far_max_is_beyond_the_first_grid_pass():
    case = stc.case("far_max")
    hb = stc.parsed("far_max")
    m, n = hb.lengths()
    at = case.facts["at"]
    assert hb.n == case.facts["n"] and at >= stc.MAX_GRID_THREADS == 262_144
    assert np.flatnonzero(m).tolist() == [at] and np.flatnonzero(n).tolist() == [at] and m[at] == 300 and n[at] == 300
    assert len(case.text) < (1 << 20)  # one chunk when streamed in chunks of 1 MiB


def test_density_step_overflows_the_staging_of_its_first_chunk():
    """The library's bound, restated: csrc/asm_capi.hip, asm_stream_seq_file, process(), `if (n > pen_cap)`:
    `full = n / shipped * slot_cap + 1` and `cap = max(full, n) + max(full, n) / 8 + 1024` with `slot_cap = chunk + (4 << 20)`,
    taken from the first chunk.  A chunk with more pairs than that takes the branch that harvests both buffers and reallocates the
    staging; test_gpu_ingest_edges.py relies on this text reaching it.  If the library's sizing changes, change this with it."""
    case = stc.case("density_step")
    f = case.facts
    chunk = f["chunk"]
    assert chunk == 1 << 16
    per_byte = f["first_pairs"] / f["first_bytes"]
    bound = 9 / 8 * (per_byte * (chunk + (4 << 20))) + 1024
    assert f["densest_pairs"] > bound + 8, (f["densest_pairs"], bound)  # + 8: the library's integer roundings
    assert f["densest_index"] >= 3 and f["first_pairs"] == 63
    # the same cut rule for both counts, checked against the text: whole pairs, the carry of the chunk before in front
    cuts = f["cuts"]
    assert cuts == stc.chunk_cuts(case.text, chunk)
    hb = stc.parsed("density_step")
    assert sum(c[2] for c in cuts) == hb.n == 200 + 60_000 + 50 and sum(c[1] for c in cuts) == len(case.text)
    nl = _newlines(case.text)
    for k, (first, nbytes, pairs, carried) in enumerate(cuts):
        assert first + nbytes <= min(len(case.text), chunk * (k + 1)) and carried == (chunk * k - first if k else 0)
        assert int(((nl >= first) & (nl < first + nbytes)).sum()) == 2 * pairs
    m, n = hb.lengths()
    assert m[:200].min() == 512 and m[200:60_200].max() <= 3 and m[60_200:].min() == 512 and n[200:60_200].max() <= 3
    assert (m[200:60_200] == 0).any() and b"\n\n\n" in case.text  # lines of zero bytes among the short ones


@pytest.mark.parametrize("shift", stc.FIXED_SHIFTS)
def test_fixed_width_cuts_fall_where_claimed(shift):
    case = stc.case(f"fixed_width_{shift}")
    text, n = case.text, case.facts["pairs"]
    hb = stc.parsed(case.name)
    m, nn = hb.lengths()
    assert hb.n == n and (m[1:] == 30).all() and (nn == 30).all() and len(text) == 64 * n + (64 - shift) % 64
    cuts = stc.chunk_cuts(text, TILE)
    whole = [c for c in cuts if c[0] + c[1] < len(text)]  # every chunk but the one that ends with the file
    assert len(whole) >= 5
    for k, (first, nbytes, pairs, carried) in enumerate(whole):
        end = first + nbytes
        assert TILE * (k + 1) - end == shift and (carried == shift or k == 0)
        read_so_far = text[end:TILE * (k + 1)]
        assert read_so_far.count(b"\n") == (1 if shift >= 32 else 0)  # shift 32: the read line is in, its reference line is not
    if shift == 0:
        assert cuts[0][2] == 64 and all(c[3] == 0 for c in cuts) and len(text) % TILE == 0 and len(cuts) == len(text) // TILE
    if shift == 32:
        assert all(text[c[0] + c[1]:TILE * (k + 1)].endswith(b"\n") for k, c in enumerate(whole))
    for max_pairs in (1, 64, 65, n, n + 5):
        cut = stc.chunk_cuts(text, TILE, max_pairs)
        assert sum(c[2] for c in cut) == min(max_pairs, n)
