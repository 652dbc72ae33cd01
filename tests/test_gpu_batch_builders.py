"""Equal pairs give an equal batch, whichever constructor made it: asm_batch_upload, asm_batch_from_text, asm_batch_generate,
asm_batch_from_hits and the chunks of asm_stream_seq_file, on the smallest pair lists at which a constructor can go wrong (no pair,
one pair, empty strings, the width-class edges, a mixed batch below and at the bucketing threshold, seed-hit windows clipped at the
end of the reference), and every refusal of theirs that Python can reach, with its code and its call's name.

The reference of every comparison is the uploaded batch of the same pairs; every comparison is exact.  LEAP (k = 3) is compared on
the pairs on which it is defined (tests.util.leap_defined: both strings within 256).  asm_batch_from_hits reports a bound as its
maximum, longest read + 1: its planes are compared only where that equals the uploaded batch's measured maximum.

Not tested here: the 4 GiB refusals of asm_batch_generate and asm_batch_from_text, which need inputs that do not fit a test."""
import ctypes

import numpy as np
import pytest

from tests.util import leap_defined

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
EDGES = (127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512)
_LISTS = {}


def _mutated(rng, s, edits):
    s = list(s)
    for _ in range(edits):
        op, at = int(rng.integers(0, 3)), int(rng.integers(0, max(len(s), 1)))
        if op == 0 and s:
            s[at] = "ACGT"[int(rng.integers(0, 4))]
        elif op == 1 and s:
            del s[at]
        else:
            s.insert(at, "ACGT"[int(rng.integers(0, 4))])
    return "".join(s)


def _random(rng, length):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, length))


def _edge_pairs(L):
    """40 pairs whose longest string has exactly L characters: the read, the reference, or both."""
    rng = np.random.default_rng(1000 + L)
    pairs = []
    for i in range(40):
        a = _random(rng, L)
        b = _mutated(rng, a, int(rng.integers(0, 5)))[:L]
        pairs.append((a, b) if i % 3 else (b, a))
    pairs[7] = (pairs[7][0], pairs[7][0])
    pairs[11] = (_random(rng, L), "")
    return pairs


def _mixed_pairs(n):
    """Classes 0 and 1 side by side, every eleventh pair and the last one in class 1."""
    rng = np.random.default_rng(n)
    pairs = []
    for i in range(n):
        a = _random(rng, int(rng.integers(130, 200)) if i % 11 == 5 or i == n - 1 else int(rng.integers(0, 60)))
        pairs.append((a, _mutated(rng, a, int(rng.integers(0, 4)))))
    return pairs


def _pairs(name):
    """The pair lists, built once and shared: do not modify them."""
    if name not in _LISTS:
        if name == "n0":
            _LISTS[name] = []
        elif name == "n1":
            _LISTS[name] = [("ACGTACGTTGCA", "ACGAACGTTGC")]
        elif name == "empties":
            _LISTS[name] = [("", "ACGT"), ("ACGT", ""), ("", ""), ("ACGTAC", "ACTTAC"), ("", ""), ("G", ""), ("", "T")]
        elif name.startswith("edge"):
            _LISTS[name] = _edge_pairs(int(name[4:]))
        elif name.startswith("mixed"):
            _LISTS[name] = _mixed_pairs(int(name[5:]))
        else:
            raise KeyError(name)
    return _LISTS[name]


def _seq_text(pairs):
    return "".join(f">{a}\n<{b}\n" for a, b in pairs).encode("ascii")


def _observed(asm, engine, batch, hb, planes=True):
    """Everything a caller can see of a batch."""
    d = batch.download()
    seen = {"read_off": d.read_off, "ref_off": d.ref_off, "reads": d.reads, "refs": d.refs,
            "sizes": np.array([batch.n, batch.max_length, batch.ascii_bytes])}
    if planes:
        seen["planes"], seen["lens"], seen["order"] = batch.download_planes()
        if batch.n == 0:
            seen["planes"] = seen["planes"][:0]  # the one entry an empty batch allocates is never written
    p = asm.Params.default(k=3)
    keep = leap_defined(hb)
    for a, name in ((asm.NW, "nw"), (asm.LEAP, "leap"), (asm.GREEDY, "greedy")):
        pen = engine.align(batch, a, p)
        seen[name] = np.where(keep, pen, 0) if a == asm.LEAP else pen
    return seen


def _same(what, got, want, skip=()):
    for key, w in want.items():
        if key in skip or key not in got:
            continue
        g = got[key]
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1)) if g.size else np.zeros(0, int)
        assert bad.size == 0, f"{what}: {key} differs in {bad.size} entries, first at {bad[:5]}: got {g[bad[:3]]} want {w[bad[:3]]}"


def _check_constructors(asm, engine, tmp_path, pairs, what, chunk_bytes=0):
    """upload, from_text and one streamed run of the same pairs, in both Greedy modes.  -> the uploaded batches' observations"""
    hb = asm.HostBatch.from_strings(pairs)
    text = _seq_text(pairs)
    want = {}
    for mode, tag in ((asm.GREEDY_CLEAN, "clean"), (asm.GREEDY_SEQUENTIAL, "sequential")):
        up = engine.upload(hb, mode)
        m, n = hb.lengths()
        assert (up.n, up.max_length, up.ascii_bytes) == (hb.n, int(max(m.max(), n.max())) if hb.n else 0, int(m.sum() + n.sum()))
        want[mode] = _observed(asm, engine, up, hb)
        up.free()
        tx = engine.batch_from_text(text, mode)
        _same(f"{what}: from_text, {tag}", _observed(asm, engine, tx, hb), want[mode])
        tx.free()
    path = str(tmp_path / "pairs.seq")
    with open(path, "wb") as fh:
        fh.write(text)
    got, st = engine.stream_seq_file(path, asm.Params.default(k=3), asm.GREEDY_SEQUENTIAL, chunk_bytes=chunk_bytes)
    assert (st.pairs, st.max_length) == (hb.n, int(want[asm.GREEDY_SEQUENTIAL]["sizes"][1]))
    keep = leap_defined(hb)
    streamed = {"nw": got[asm.NW], "leap": np.where(keep, got[asm.LEAP], 0), "greedy": got[asm.GREEDY]}
    _same(f"{what}: streamed", streamed, {k: want[asm.GREEDY_SEQUENTIAL][k] for k in streamed})
    return hb, want


@pytest.mark.parametrize("name", ["n0", "n1", "empties"] + [f"edge{L}" for L in EDGES])
def test_small_lists_give_one_batch_through_every_constructor(asm, engine, tmp_path, name):
    """No pair, one pair, empty strings on either side and on both, and a few dozen pairs at each width-class edge."""
    pairs = _pairs(name)
    hb, want = _check_constructors(asm, engine, tmp_path, pairs, name)
    if name.startswith("edge"):
        L = int(name[4:])
        assert want[asm.GREEDY_CLEAN]["sizes"][1] == L
        assert want[asm.GREEDY_CLEAN]["planes"].shape[0] == 4 * ((L + 127) // 128) * hb.n  # one bucket of the batch's class
    if name == "n0":
        assert want[asm.GREEDY_CLEAN]["sizes"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("n", [4095, 4096])
def test_mixed_classes_below_and_at_the_bucketing_threshold(asm, engine, tmp_path, n):
    """Two width classes in one batch: at n = 4095 one bucket in input order, at n = 4096 sorted by class, stable inside a class.  The
    streamed run cuts the text into several chunks."""
    hb, want = _check_constructors(asm, engine, tmp_path, _pairs(f"mixed{n}"), f"mixed{n}", chunk_bytes=65536)
    m, r = hb.lengths()
    cls = (np.maximum(np.maximum(m, r), 1) + 127) // 128 - 1
    assert set(cls.tolist()) == {0, 1}
    for mode in (asm.GREEDY_CLEAN, asm.GREEDY_SEQUENTIAL):
        order, planes = want[mode]["order"], want[mode]["planes"]
        if n < 4096:
            assert np.array_equal(order, np.arange(n)) and planes.shape[0] == 4 * 2 * n
        else:
            assert np.array_equal(order, np.argsort(cls, kind="stable"))
            assert planes.shape[0] == 4 * (int((cls == 0).sum()) + 2 * int((cls == 1).sum()))


@pytest.mark.parametrize("config,n", [("C5", 4096), ("C2", 1)])
def test_device_generator_gives_the_uploaded_batch(asm, engine, config, n):
    """asm_batch_generate against the host generator's pairs, uploaded: planes included, both Greedy modes."""
    cfg = asm.workload(config)[0]
    hb = asm.generate_pairs(cfg, 77, n)
    for mode in (asm.GREEDY_CLEAN, asm.GREEDY_SEQUENTIAL):
        up = engine.upload(hb, mode)
        want = _observed(asm, engine, up, hb)
        up.free()
        dev = engine.generate(cfg, 77, n, mode)
        _same(f"{config} generate, mode {mode}", _observed(asm, engine, dev, hb), want)
        dev.free()


def _windows(genome, reads, pos):
    """The pairs asm_batch_from_hits must build: read i against genome[start, start + len_i + 1), start = pos - 1 (0 for pos 0),
    clipped at the genome's end."""
    pairs = []
    for r, p in zip(reads, pos):
        start = int(p) - 1 if p else 0
        pairs.append((r, genome[start:start + len(r) + 1]))
    return pairs


def _check_hits(asm, engine, genome, reads, pos, what):
    pairs = _windows(genome, reads, pos)
    hb = asm.HostBatch.from_strings(pairs)
    ref = engine.upload_reference(genome)
    longest = max((len(r) for r in reads), default=0)
    for mode in (asm.GREEDY_CLEAN, asm.GREEDY_SEQUENTIAL):
        up = engine.upload(hb, mode)
        want = _observed(asm, engine, up, hb)
        up.free()
        hits = engine.batch_from_hits(ref, hb.reads, hb.read_off, np.asarray(pos, np.uint64), mode)
        assert hits.max_length == longest + 1, (what, hits.max_length, longest)
        same_max = hits.max_length == int(want["sizes"][1])
        got = _observed(asm, engine, hits, hb, planes=same_max)
        assert got["sizes"][[0, 2]].tolist() == want["sizes"][[0, 2]].tolist()
        _same(f"{what}: from_hits, mode {mode}", got, want, skip=("sizes",) + (() if same_max else ("planes", "lens", "order")))
        hits.free()
    ref.free()
    return hb


def test_seed_hit_windows_inside_a_text(asm, engine, tmp_path):
    """Windows of a text through all constructors: reads of many lengths, hits all over a reference of 700 bases, a read of 511 bytes
    among them (its window of 512 is the batch's measured maximum, so the planes are compared too)."""
    rng = np.random.default_rng(5)
    genome = _random(rng, 700)
    reads, pos = [], []
    for i in range(60):
        length = 511 if i == 17 else int(rng.integers(0, 150))
        p = int(rng.integers(0, len(genome) - length - 1))
        reads.append(_mutated(rng, genome[p:p + length], int(rng.integers(0, 3)))[:length].ljust(length, "A"))
        pos.append(p)
    hb = _check_hits(asm, engine, genome, reads, pos, "windows")
    assert int(max(hb.lengths()[1])) == 512
    _check_constructors(asm, engine, tmp_path, _windows(genome, reads, pos), "windows")


def test_seed_hit_windows_at_the_ends_of_the_reference(asm, engine):
    """Hits at 0, 1, len - 1, len and len + 5 of a reference of 300 bases, reads of 0, 1, 2 and 10 bytes at each: a start at len - 2
    clips the window to 2 bytes, at len - 1 to 1, at or beyond the end to none.  Then the same with every window clipped: the maximum
    stays the bound, longest read + 1."""
    rng = np.random.default_rng(6)
    genome = _random(rng, 300)
    ends = [0, 1, 299, 300, 305]
    reads = [_random(rng, length) for _ in ends for length in (0, 1, 2, 10)]
    pos = [p for p in ends for _ in range(4)]
    hb = _check_hits(asm, engine, genome, reads, pos, "ends")
    win = hb.lengths()[1].reshape(5, 4)
    assert win[2].tolist() == [1, 2, 2, 2] and win[3].tolist() == [1, 1, 1, 1] and win[4].tolist() == [0, 0, 0, 0]
    assert win[0].tolist() == [1, 2, 3, 11] and win[1].tolist() == [1, 2, 3, 11]
    clipped = [(r, p) for r, p in zip(reads, pos) if p >= 299]
    hb = _check_hits(asm, engine, genome, [r for r, _ in clipped], [p for _, p in clipped], "all clipped")
    assert int(max(hb.lengths()[1])) == 2


def _still_works(asm, engine):
    hb = asm.HostBatch.from_strings([("ACGTACGT", "ACGTACGT"), ("ACGTACGT", "ACGAACGT"), ("ACGT", "AGT")])
    b = engine.upload(hb)
    assert engine.align(b, asm.NW, asm.Params.default(k=3)).tolist() == [0, 1, 1]
    assert engine.align(b, asm.GREEDY, asm.Params.default(k=3)).tolist() == [0, 1, 1]
    b.free()


def test_refusals_keep_code_text_and_call_name(asm, engine, tmp_path):
    """Every argument and size refusal of the constructors that Python can reach; after each one the engine builds and aligns."""
    lib, h = engine.lib, engine.h
    ok = asm.HostBatch.from_strings([("ACGT", "ACGT"), ("AC", "AG")])
    ref = engine.upload_reference("ACGT" * 200)
    out = ctypes.c_void_p()
    cfg = asm.workload("C2")[0]

    def raw(rc):
        engine._chk(rc)

    cases = [
        # bad arguments
        (EINVAL, ("asm_batch_upload: bad arguments",),
         lambda: raw(lib.asm_batch_upload(h, -1, ok.reads.ctypes.data, ok.read_off.ctypes.data, ok.refs.ctypes.data,
                                          ok.ref_off.ctypes.data, asm.GREEDY_CLEAN, ctypes.byref(out)))),
        (EINVAL, ("asm_batch_upload: bad arguments",),
         lambda: raw(lib.asm_batch_upload(h, 2, None, ok.read_off.ctypes.data, ok.refs.ctypes.data, ok.ref_off.ctypes.data,
                                          asm.GREEDY_CLEAN, ctypes.byref(out)))),
        (EINVAL, ("asm_batch_generate: bad arguments",), lambda: engine.generate(cfg, -1, 4)),
        (EINVAL, ("asm_batch_generate: bad arguments",), lambda: engine.generate(cfg, 0, -4)),
        (EINVAL, ("asm_batch_from_hits: bad arguments",),
         lambda: raw(lib.asm_batch_from_hits(h, None, 2, ok.reads.ctypes.data, ok.read_off.ctypes.data, None, asm.GREEDY_CLEAN,
                                             ctypes.byref(out)))),
        (EINVAL, ("asm_batch_from_text: bad argument",),
         lambda: raw(lib.asm_batch_from_text(h, None, 10, asm.GREEDY_CLEAN, ctypes.byref(out)))),
        # unknown greedy_mode, behind the call's own argument check
        (EINVAL, ("asm_batch_upload: unknown greedy_mode",), lambda: engine.upload(ok, 7)),
        (EINVAL, ("asm_batch_generate: unknown greedy_mode",), lambda: engine.generate(cfg, 0, 4, 7)),
        (EINVAL, ("asm_batch_from_hits: unknown greedy_mode",),
         lambda: engine.batch_from_hits(ref, ok.reads, ok.read_off, np.array([0, 4], np.uint64), 7)),
        (EINVAL, ("asm_batch_from_text: unknown greedy_mode",), lambda: engine.batch_from_text(b">AC\n<AC\n", 7)),
        (EINVAL, ("asm_stream_seq_file: unknown greedy_mode",),
         lambda: engine.stream_seq_file(_seq_file(tmp_path, [("AC", "AC")]), asm.Params.default(k=3), 7)),
        # offsets
        (EINVAL, ("asm_batch_upload: offsets must be non-decreasing",),
         lambda: engine.upload(asm.HostBatch(ok.reads, np.array([0, 5, 4], np.uint32), ok.refs, ok.ref_off))),
        (EINVAL, ("asm_batch_upload: offsets must be non-decreasing",),
         lambda: engine.upload(asm.HostBatch(ok.reads, ok.read_off, ok.refs, np.array([3, 2, 6], np.uint32)))),
        (EINVAL, ("asm_batch_from_hits: offsets must be non-decreasing",),
         lambda: engine.batch_from_hits(ref, ok.reads, np.array([0, 5, 4], np.uint32), np.array([0, 4], np.uint64))),
        # a decreasing offset wins over a string that is too long
        (EINVAL, ("asm_batch_upload: offsets must be non-decreasing",),
         lambda: engine.upload(asm.HostBatch(np.zeros(600, np.uint8) + 65, np.array([0, 600, 599], np.uint32), ok.refs, ok.ref_off))),
        # lengths
        (EUNSUPPORTED, ("asm_batch_upload: a sequence is longer than ASM_MAX_LENGTH",),
         lambda: engine.upload(asm.HostBatch.from_strings([("ACGT", "ACGT"), ("A" * 513, "ACGT")]))),
        (EUNSUPPORTED, ("asm_batch_upload: a sequence is longer than ASM_MAX_LENGTH",),
         lambda: engine.upload(asm.HostBatch.from_strings([("ACGT", "C" * 513)]))),
        (EUNSUPPORTED, ("streamed file: a sequence is longer than ASM_MAX_LENGTH",),
         lambda: engine.batch_from_text(_seq_text([("ACGT", "ACGT"), ("ACGT", "A" * 513)]))),
        (EUNSUPPORTED, ("streamed file: a sequence is longer than ASM_MAX_LENGTH",),
         lambda: engine.stream_seq_file(_seq_file(tmp_path, [("A" * 513, "ACGT")]), asm.Params.default(k=3))),
        (EUNSUPPORTED, ("asm_batch_from_hits: a read is longer than ASM_MAX_LENGTH - 1",),
         lambda: engine.batch_from_hits(ref, np.zeros(512, np.uint8) + 65, np.array([0, 512], np.uint32), np.array([3], np.uint64))),
        (EUNSUPPORTED, ("asm_batch_generate: a generated sequence exceeds ASM_MAX_LENGTH",),
         lambda: engine.generate(asm.GenConfig.per_base(3, 512, 0.01, 0.2, 0.0), 0, 64)),
    ]
    for code, words, call in cases:
        with pytest.raises(asm.AsmError) as ei:
            call()
        assert ei.value.code == code and all(w in str(ei.value) for w in words), (code, words, ei.value.code, str(ei.value))
        _still_works(asm, engine)
    # the strings at the limit are accepted
    b = engine.upload(asm.HostBatch.from_strings([("A" * 512, "C" * 512)]))
    assert b.max_length == 512
    b.free()
    b = engine.batch_from_hits(ref, np.zeros(511, np.uint8) + 65, np.array([0, 511], np.uint32), np.array([3], np.uint64))
    assert b.max_length == 512 and b.download().ref_off.tolist() == [0, 512]
    b.free()
    ref.free()


def _seq_file(tmp_path, pairs):
    path = str(tmp_path / "refusal.seq")
    with open(path, "wb") as fh:
        fh.write(_seq_text(pairs))
    return path
