"""The device parser of the harness's text (csrc/asm_ingest.h) and the streamed file path around it (asm_stream_seq_file) at their
edges, on the corpus of tests/seq_text_cases.py: newlines on slice, wave and tile edges, tiles full of newlines, texts that end on
those edges, lines of zero bytes, the gather's lane-stride lengths side by side, bytes that are no bases, the longest pair beyond
the maximum kernel's first grid pass, a chunk that outgrows the result staging, fixed chunk carries, the wrapper's default capacity
and an error in a late chunk.  The reference is the byte-level parser of that module and the oracle run over its batch; every
comparison is exact.  tests/test_seq_text_host.py proves on the CPU that each text holds its edge."""
import os

import numpy as np
import pytest

from tests import seq_text_cases as stc
from tests.util import leap_defined, random_ragged_batch

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(oracle, name, what):
    """The oracle's answer for a corpus text, computed once and shared: do not modify it.  NW and LEAP see the batch through the
    code-00 mapping of the pack kernel, Greedy sees the raw bytes."""
    key = (name, what)
    if key not in _WANT:
        hb = stc.parsed(name)
        if what == "nw":
            _WANT[key] = oracle.nw(stc.packed(hb))
        elif what == "nw231":
            _WANT[key] = oracle.nw(stc.packed(hb), 2, 3, 1)
        elif what == "leap":
            _WANT[key] = oracle.leap(stc.packed(hb), 3)
        elif what == "greedy_clean":
            _WANT[key] = oracle.greedy(hb, 3, mode=1)
        elif what == "greedy_sequential":
            _WANT[key] = oracle.greedy(hb, 3, mode=0)
        else:
            raise KeyError(what)
    return _WANT[key]


def _strings(hb, i):
    return (hb.reads[hb.read_off[i]:hb.read_off[i + 1]].tobytes(), hb.refs[hb.ref_off[i]:hb.ref_off[i + 1]].tobytes())


def _same_batch(got, want, what):
    assert got.n == want.n, (what, got.n, want.n)
    for side in ("read_off", "ref_off"):
        bad = np.flatnonzero(getattr(got, side) != getattr(want, side))
        assert bad.size == 0, f"{what}: {side} differs first at pair {bad[0]}: got {getattr(got, side)[bad[:4]]} want {getattr(want, side)[bad[:4]]}"
    for side, off in (("reads", "read_off"), ("refs", "ref_off")):
        g, w = getattr(got, side), getattr(want, side)
        assert g.size == w.size, (what, side, g.size, w.size)
        bad = np.flatnonzero(g != w)
        if bad.size:
            i = int(np.searchsorted(getattr(want, off), bad[0], side="right")) - 1
            raise AssertionError(f"{what}: {side} differ in {bad.size} bytes, first in pair {i}: got {_strings(got, i)} want {_strings(want, i)}")


def _equal(what, got, want, hb, keep=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want) & (True if keep is None else keep))
    assert bad.size == 0, (f"{what}: {bad.size}/{hb.n} differ; first {bad[:5]} got {got[bad[:5]]} want {want[bad[:5]]} "
                           f"pair {_strings(hb, int(bad[0]))}")


def _file(tmp_path, text, name="pairs.seq"):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(text)
    return path


def _longest(hb):
    m, n = hb.lengths()
    return int(max(m.max(), n.max())) if hb.n else 0


@pytest.mark.parametrize("name", stc.NAMES)
def test_text_is_parsed_like_the_reference_parser(asm, engine, oracle, tmp_path, name):
    """asm_batch_from_text gives the parser's offsets and bytes on both sides; the same text as a file, streamed in chunks of
    4,096 bytes (every text has several; each carries the tail of the one before), gives the parser's pair count, the text's bytes
    (with the newlines the reader appends) and the longest string, and NW's penalties equal the oracle's on the parser's batch."""
    text = stc.case(name).text
    want = stc.parsed(name)
    batch = engine.batch_from_text(text)
    assert batch.n == want.n and batch.max_length == _longest(want)
    _same_batch(batch.download(), want, name)
    batch.free()
    got, st = engine.stream_seq_file(_file(tmp_path, text), asm.Params.default(), asm.GREEDY_CLEAN, aligners=(asm.NW,), chunk_bytes=4096)
    assert (st.pairs, st.bytes, st.max_length) == (want.n, stc.shipped_bytes(text), _longest(want))
    assert st.chunks == sum(1 for c in stc.chunk_cuts(text, 4096) if c[2] > 0)
    _equal(f"{name} streamed nw", got[asm.NW], _want(oracle, name, "nw"), want)


@pytest.mark.parametrize("name", stc.NAMES)
def test_aligners_on_the_parsed_text_equal_the_oracle(asm, engine, oracle, name):
    """NW (unit costs and (2, 3, 1)) and Greedy (clean, k = 3) on every pair; LEAP (k = 3) on every pair with both strings within 256
    (tests.util.leap_defined: all pairs, except in lengths_mix and density_step and the 300-character pairs of dense and far_max)."""
    hb = stc.parsed(name)
    batch = engine.batch_from_text(stc.case(name).text, asm.GREEDY_CLEAN)
    p = asm.Params.default(k=3)
    _equal(f"{name} nw", engine.align(batch, asm.NW, p), _want(oracle, name, "nw"), hb)
    _equal(f"{name} nw (2, 3, 1)", engine.align(batch, asm.NW, asm.Params.default(k=3, x=2, o=3, e=1)), _want(oracle, name, "nw231"), hb)
    _equal(f"{name} greedy", engine.align(batch, asm.GREEDY, p), _want(oracle, name, "greedy_clean"), hb)
    keep = leap_defined(hb)
    assert keep.all() or name in stc.BEYOND_LEAP
    _equal(f"{name} leap", engine.align(batch, asm.LEAP, p), _want(oracle, name, "leap"), hb, keep)
    batch.free()


def test_longest_pair_beyond_the_first_grid_pass(asm, engine, oracle, tmp_path):
    """300,000 pairs in one chunk: seq_max_kernel's threads take a second pass, and only there is a string longer than zero."""
    case = stc.case("far_max")
    hb, at = stc.parsed("far_max"), case.facts["at"]
    got, st = engine.stream_seq_file(_file(tmp_path, case.text), asm.Params.default(), asm.GREEDY_CLEAN, aligners=(asm.NW,),
                                     chunk_bytes=1 << 20)
    assert st.pairs == hb.n and st.chunks == 1 and st.max_length == 300
    nw = got[asm.NW]
    assert nw.size == hb.n and nw[at] == _want(oracle, "far_max", "nw")[at] and nw[at] > 0
    assert np.count_nonzero(nw) == 1


def test_chunk_that_outgrows_the_result_staging(asm, engine, oracle, tmp_path):
    """density_step in chunks of 64 KiB: the first chunk holds 63 pairs of 512 characters, the middle chunks more than 9,000 short
    ones — more than the staging sized from the first chunk holds (test_seq_text_host.py restates the library's bound and proves
    it on the CPU; nothing here observes which branch ran).  Every penalty of all three aligners equals the oracle over the whole
    file, Greedy in sequential mode with its chain through every chunk, and the counters equal a host recount; then once more on
    the same engine with LEAP and Greedy alone, which finds the pinned staging of the first call on the handle."""
    case = stc.case("density_step")
    hb = stc.parsed("density_step")
    path = _file(tmp_path, case.text)
    p = asm.Params.default(k=3)
    nw, leap, greedy = (_want(oracle, "density_step", w) for w in ("nw", "leap", "greedy_sequential"))
    keep = leap_defined(hb)
    got, st = engine.stream_seq_file(path, p, asm.GREEDY_SEQUENTIAL, chunk_bytes=case.facts["chunk"])
    assert st.pairs == hb.n and st.bytes == len(case.text) and st.max_length == 512
    assert st.chunks == sum(1 for c in case.facts["cuts"] if c[2] > 0)
    _equal("nw", got[asm.NW], nw, hb)
    _equal("leap", got[asm.LEAP], leap, hb, keep)
    _equal("greedy", got[asm.GREEDY], greedy, hb)
    assert list(st.counters) == [hb.n, hb.n, int((got[asm.LEAP] == nw).sum()), int((greedy == nw).sum())]
    two, st2 = engine.stream_seq_file(path, p, asm.GREEDY_SEQUENTIAL, aligners=(asm.LEAP, asm.GREEDY), chunk_bytes=case.facts["chunk"])
    assert st2.pairs == hb.n and set(two) == {asm.LEAP, asm.GREEDY}
    _equal("leap, second call", two[asm.LEAP], leap, hb, keep)
    _equal("greedy, second call", two[asm.GREEDY], greedy, hb)


@pytest.mark.parametrize("shift", stc.FIXED_SHIFTS)
def test_fixed_carry_on_every_chunk(asm, engine, oracle, tmp_path, shift):
    """Pairs of 64 bytes in chunks of 4,096: no carry, a carry of 1 and of 63 bytes, and a cut between a read line and its
    reference line on every chunk; max_pairs at 1, at the first chunk's end, one behind it, at the file's end and beyond it."""
    name = f"fixed_width_{shift}"
    case, hb = stc.case(name), stc.parsed(name)
    path = _file(tmp_path, case.text)
    p = asm.Params.default(k=3)
    got, st = engine.stream_seq_file(path, p, asm.GREEDY_SEQUENTIAL, chunk_bytes=4096)
    assert st.pairs == hb.n and st.bytes == len(case.text) and st.chunks == len(stc.chunk_cuts(case.text, 4096))
    _equal("nw", got[asm.NW], _want(oracle, name, "nw"), hb)
    _equal("leap", got[asm.LEAP], _want(oracle, name, "leap"), hb)
    _equal("greedy", got[asm.GREEDY], _want(oracle, name, "greedy_sequential"), hb)
    n = hb.n
    for max_pairs in (1, 64, 65, n, n + 5):
        cut = min(max_pairs, n)
        part, st = engine.stream_seq_file(path, p, asm.GREEDY_CLEAN, chunk_bytes=4096, max_pairs=max_pairs)
        assert st.pairs == cut and all(v.size == cut for v in part.values()), (max_pairs, st.pairs)
        assert st.bytes == sum(c[1] for c in stc.chunk_cuts(case.text, 4096, max_pairs))
        _equal(f"nw, max_pairs {max_pairs}", part[asm.NW], _want(oracle, name, "nw")[:cut], hb)
        _equal(f"leap, max_pairs {max_pairs}", part[asm.LEAP], _want(oracle, name, "leap")[:cut], hb)
        _equal(f"greedy, max_pairs {max_pairs}", part[asm.GREEDY], _want(oracle, name, "greedy_clean")[:cut], hb)


def test_ragged_text_with_empty_strings_streamed_sequentially(asm, engine, oracle, tmp_path):
    """Lengths 0 to 300 mixed, empty strings among them, in chunks of 4,096 bytes: Greedy's stale-tail chain through every chunk
    boundary equals the oracle's sequential mode on every pair."""
    hb = random_ragged_batch(asm, 29, 3000, 0, 300)
    m, n = hb.lengths()
    assert (m == 0).any() and (n == 0).any()
    path = str(tmp_path / "ragged.seq")
    hb.write_seq_file(path)
    got, st = engine.stream_seq_file(path, asm.Params.default(k=3), asm.GREEDY_SEQUENTIAL, chunk_bytes=4096)
    assert st.pairs == hb.n and st.bytes == os.path.getsize(path) and st.max_length == int(max(m.max(), n.max()))
    _equal("greedy", got[asm.GREEDY], oracle.greedy(hb, 3, mode=0), hb)
    _equal("nw", got[asm.NW], oracle.nw(hb), hb)


def test_default_capacity_holds_a_file_of_bare_newlines(asm, engine, tmp_path):
    """A pair costs as little as two bytes — two lines of zero bytes — so 2,000 newlines are 1,000 pairs, and the arrays that
    Engine.stream_seq_file sizes by itself must hold them all."""
    got, st = engine.stream_seq_file(_file(tmp_path, b"\n" * 2000), asm.Params.default())
    assert st.pairs == 1000
    for a in (asm.NW, asm.LEAP, asm.GREEDY):
        assert got[a].shape == (1000,) and not got[a].any(), (a, got[a].shape)
    got, st = engine.stream_seq_file(_file(tmp_path, b"\n" * 1999, "odd.seq"), asm.Params.default())
    assert st.pairs == 1000 and got[asm.NW].shape == (1000,)
    got, st = engine.stream_seq_file(_file(tmp_path, b"\n", "one.seq"), asm.Params.default())
    assert st.pairs == 1 and got[asm.NW].tolist() == [0]


def _late_line(rng_key, length):
    """Five chunks of 64-byte pairs, then a pair whose read has `length` characters (in the sixth 4,096-byte chunk), then 20 more."""
    case = stc.fixed_width(0)
    lines = case.text.split(b"\n")[:-1]
    head, tail = lines[:2 * 320], lines[2 * 320:2 * 340]
    long_read = b">" + bytes(b"ACGT"[(i * 7 + rng_key) % 4] for i in range(length))
    text = b"\n".join(head + [long_read, b"<" + long_read[1:length - 2]] + tail) + b"\n"
    assert 5 * 4096 == sum(len(x) + 1 for x in head) and 5 * 4096 + length + 2 < 6 * 4096
    return text


def test_error_in_a_late_chunk_leaves_the_engine_usable(asm, engine, oracle, tmp_path):
    """A line of 513 characters in the sixth chunk is refused with an error, after five chunks have gone through; the same engine
    then streams newline_grid correctly; a line of 512 characters in the same place is taken."""
    p = asm.Params.default(k=3)
    with pytest.raises(asm.AsmError):
        engine.stream_seq_file(_file(tmp_path, _late_line(1, 513), "long.seq"), p, asm.GREEDY_SEQUENTIAL, chunk_bytes=4096)
    name = "newline_grid"
    hb = stc.parsed(name)
    got, st = engine.stream_seq_file(_file(tmp_path, stc.case(name).text, "grid.seq"), p, asm.GREEDY_CLEAN, chunk_bytes=4096)
    assert st.pairs == hb.n
    _equal("nw after the error", got[asm.NW], _want(oracle, name, "nw"), hb)
    _equal("leap after the error", got[asm.LEAP], _want(oracle, name, "leap"), hb)
    _equal("greedy after the error", got[asm.GREEDY], _want(oracle, name, "greedy_clean"), hb)
    text = _late_line(1, 512)
    hb = stc.parse(text)
    got, st = engine.stream_seq_file(_file(tmp_path, text, "fits.seq"), p, asm.GREEDY_CLEAN, chunk_bytes=4096)
    assert st.pairs == hb.n == 341 and st.max_length == 512
    _equal("nw, 512 in the sixth chunk", got[asm.NW], oracle.nw(hb), hb)
    _equal("greedy, 512 in the sixth chunk", got[asm.GREEDY], oracle.greedy(hb, 3, mode=1), hb)
