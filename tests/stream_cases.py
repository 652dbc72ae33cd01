"""Helpers of tests/test_gpu_stream_order.py: the gate (a bounded spin the caller enqueues on its stream), the ordering pattern
around one library call, and the table of enqueue-only calls.

An ordering case on stream S, every buffer a torch tensor handed over by data_ptr():
  1. inputs hold a stale value, outputs the first sentinel; the device is idle.
  2. on S: gate | torch writes the real input and the first sentinel into the outputs once more | the library call | torch copies
     the outputs away | torch overwrites the outputs with the second sentinel.
  3. S is synchronised and the copies are compared with the CPU oracle.
A call that escaped S runs while the gate still spins: it reads the stale input, and what it writes is overwritten by the sentinel
fill behind the gate, so the copy shows a sentinel or a result of the stale input.  A call that runs late leaves the first sentinel
in the copy; the second sentinel keeps a late writer from repairing it.

Gate lengths.  A gate is at least GATE_FACTOR times the ungated time of the work behind it (events on the stream around one
ungated run, which is also the warm-up), never below GATE_FLOOR_MS (the host needs about a millisecond to enqueue a pattern) and
never above GATE_CAP_MS.  The ungated times and gate lengths of every case are measured where the module runs and printed as
`GATE <case> <ungated ms> <gate ms> <ratio>` lines (pytest -s); the table below the constants holds one such run, and none of its
ratios is below GATE_FACTOR.

What the module was seen to catch (three libraries with one contract broken each, the module run once against each) is in the
notes at the end of this file.
"""
import random

import numpy as np

GATE_FACTOR = 20.0
GATE_FLOOR_MS = 20.0
GATE_CAP_MS = 200.0
SENT1 = {"int32": 0x7F7F7F7F, "int64": 0x7F7F7F7F7F7F7F7F, "int16": 0x7F7F, "uint8": 0x7F}  # no aligner, filter or counter gives these
SENT2 = {"int32": 0x3C3C3C3C, "int64": 0x3C3C3C3C3C3C3C3C, "int16": 0x3C3C, "uint8": 0x3C}
INT32_MIN = -(2 ** 31)

# Measured on one MI355X (the run of the whole module, 89 tests in 14.1 s): ungated ms of the work behind the gate, gate ms,
# ratio.  E, F and the reset half of C.5 use GATE_CAP_MS, whatever the work.
# case                                           ungated     gate    ratio
# A/nw_unit_pair2/stream                          0.0918    20.00    218.0
# A/nw_unit_pair2/default                         0.0204    20.00    982.3
# A/nw_affine_todo/stream                         3.2135    64.27     20.0
# A/nw_affine_todo/default                        3.3490    66.98     20.0
# A/leap_k3_hinted/stream                         0.0262    20.00    764.5
# A/leap_k3_hinted/default                        0.0152    20.00   1319.3
# A/leap_k30_sorted/stream                        0.1188    20.00    168.3
# A/leap_k30_sorted/default                       0.0847    20.00    236.2
# A/greedy_k3_rank_table/stream                   0.6091    20.00     32.8
# A/greedy_k3_rank_table/default                  0.0469    20.00    426.3
# A/greedy_k17_pair_queue/stream                  0.0919    20.00    217.6
# A/greedy_k17_pair_queue/default                 0.0707    20.00    283.0
# A/greedy_k40_wide/stream                        0.0238    20.00    838.9
# A/greedy_k40_wide/default                       0.0195    20.00   1024.5
# A/greedy_cigar_k17/stream                       0.0758    20.00    263.7
# A/greedy_cigar_k17/default                      0.0762    20.00    262.3
# A/simd_ed_clean_t8_shd/stream                   0.0356    20.00    561.8
# A/simd_ed_clean_t8_shd/default                  0.0172    20.00   1165.5
# A/simd_ed_affine/stream                         0.6231    20.00     32.1
# A/simd_ed_affine/default                        0.5765    20.00     34.7
# A/shd_e3/stream                                 0.0204    20.00    978.5
# A/shd_e3/default                                0.0133    20.00   1501.5
# A/pack_then_nw_bucketed/stream                  0.1052    20.00    190.1
# A/pack_then_nw_bucketed/default                 0.0926    20.00    215.9
# A/count_equal/stream                            0.0160    20.00   1253.1
# A/count_equal/default                           0.0084    20.00   2369.7
# A/accuracy_answers/stream                       0.0186    20.00   1075.2
# A/accuracy_answers/default                      0.0103    20.00   1945.5
# B/nw_leap_greedy/repack0/stream                 0.1856    20.00    107.8
# B/nw_leap_greedy/repack1/stream                 0.1769    20.00    113.1
# B/nw_leap_greedy/repack2/stream                 0.2406    20.00     83.1
# B/nw_leap_greedy/repack3/stream                 0.2362    20.00     84.7
# B/leap_greedy_first/repack0/stream              0.3591    20.00     55.7
# B/leap_greedy_first/repack1/stream              0.3607    20.00     55.4
# B/leap_greedy_first/repack2/stream              0.4162    20.00     48.0
# B/leap_greedy_first/repack3/stream              0.3870    20.00     51.7
# B/greedy_only/repack0/stream                    0.0853    20.00    234.5
# B/greedy_only/repack1/stream                    0.0901    20.00    222.0
# B/greedy_only/repack2/stream                    0.1262    20.00    158.5
# B/greedy_only/repack3/stream                    0.2304    20.00     86.8
# B/nw_leap_greedy/repack0/default                0.1386    20.00    144.3
# B/nw_leap_greedy/repack1/default                0.1413    20.00    141.5
# B/nw_leap_greedy/repack2/default                0.1855    20.00    107.8
# B/nw_leap_greedy/repack3/default                0.2088    20.00     95.8
# C1/second_stream                                0.0161    20.00   1240.7
# C1/own_stream                                   0.0149    20.00   1340.5
# C2/upload                                       0.0148    20.00   1347.7
# C2/generate                                     0.0171    20.00   1171.0
# C3/leap_k30_d_sort                              0.0788    20.00    253.8
# C3/nw_affine_d_todo                             3.2404    64.81     20.0
# C3/greedy_k17_d_pair_queue                      0.0675    20.00    296.4
# C4/overlapped                                   0.3455    20.00     57.9
# C5/set_twice                                    0.0192    20.00   1043.8
# D/handle1                                       0.1696    20.00    117.9
# D/handle2                                       3.1906    63.81     20.0


def _key(t):
    return str(t.dtype).replace("torch.", "")


def sentinel1(*tensors):
    for t in tensors:
        t.fill_(SENT1[_key(t)])


def sentinel2(*tensors):
    for t in tensors:
        t.fill_(SENT2[_key(t)])


class Gate:
    """torch.cuda._sleep(cycles) on the current stream, calibrated once with two timing events around it."""

    def __init__(self, torch):
        self.torch = torch
        torch.cuda._sleep(1_000_000)  # the first launch loads the kernel
        torch.cuda.synchronize()
        rate = 1_000_000 / self._time(1_000_000)
        want = int(rate * 20.0)       # ... and the rate is taken from a spin of about the shortest gate
        self.cycles_per_ms = want / self._time(want)
        self.log = []

    def _time(self, cycles):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(int(cycles))
        b.record()
        b.synchronize()
        return max(a.elapsed_time(b), 1e-3)

    def start(self, ms):
        """a spin of `ms` on torch's current stream; bounded, waits for nothing"""
        assert 0.0 < ms <= GATE_CAP_MS
        self.torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def length(self, case, ungated_ms):
        ms = min(GATE_CAP_MS, max(GATE_FLOOR_MS, GATE_FACTOR * ungated_ms))
        self.log.append((case, ungated_ms, ms))
        print("GATE %-44s %9.4f %8.2f %8.1f" % (case, ungated_ms, ms, ms / max(ungated_ms, 1e-6)), flush=True)
        return ms


def timed(torch, stream, fn):
    """fn() enqueued on `stream` between two events -> ms on the device (ungated: the stream is idle before)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def ordered(torch, gate, stream, name, stale, produce, call, outs, after=None, gate_ms=None):
    """The pattern of the module docstring around `call` on `stream` (torch's current stream is set to it here).  stale(): torch ops
    that put the stale value into the inputs; produce(): torch ops that write the real input; outs: the tensors the call writes.
    after(): further library calls behind `call` that belong to it (a join).  -> the copies of outs as numpy arrays."""
    copies = [torch.empty_like(o) for o in outs]
    with torch.cuda.stream(stream):
        def once():
            call()
            if after:
                after()
        stale()
        sentinel1(*outs)
        produce()
        ungated = timed(torch, stream, once)
        if gate_ms is None:
            gate_ms = gate.length(name, ungated)
        stale()
        sentinel1(*outs)
        torch.cuda.synchronize()
        gate.start(gate_ms)
        sentinel1(*outs)
        produce()
        once()
        for c, o in zip(copies, outs):
            c.copy_(o)
        sentinel2(*outs)
        stream.synchronize()
    return [c.cpu().numpy() for c in copies]


def assert_equal(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    if bad.size:
        g, w = got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]]
        s1 = int((got.reshape(-1) == SENT1.get(str(got.dtype), None)).sum()) if str(got.dtype) in SENT1 else -1
        raise AssertionError("%s: %d of %d entries differ (first at %s: got %s, want %s; %d entries hold the first sentinel)"
                             % (name, bad.size, got.size, bad[:5].tolist(), g.tolist(), w.tolist(), s1))


class Cases:
    """Batches, oracle answers and device tensors shared by the tests of one engine: made once, never changed."""

    def __init__(self, asm, oracle, torch, eng):
        self.asm, self.oracle, self.torch, self.eng = asm, oracle, torch, eng
        self._hb, self._batch, self._want, self._dev = {}, {}, {}, {}

    def hb(self, wl, n, seed=0):
        key = (wl, n, seed)
        if key not in self._hb:
            self._hb[key] = self.asm.generate_pairs(self.asm.workload(wl)[0], 1000 * seed, n)
        return self._hb[key]

    def batch(self, wl, n, seed=0):
        """resident on self.eng (upload is synchronous: call it with no gate pending)"""
        key = (wl, n, seed)
        if key not in self._batch:
            self._batch[key] = self.eng.upload(self.hb(wl, n, seed), self.asm.GREEDY_CLEAN)
        return self._batch[key]

    def want(self, what, wl, n, seed=0, **kw):
        key = (what, wl, n, seed, tuple(sorted(kw.items())))
        if key not in self._want:
            hb, o = self.hb(wl, n, seed), self.oracle
            if what == "nw":
                v = o.nw(hb, kw.get("x", 1), kw.get("o", 1), kw.get("e", 1))
            elif what == "leap":
                v = o.leap(hb, k=kw["k"])
            elif what == "greedy":
                v = o.greedy(hb, k=kw["k"], mode=1, **({"probs": kw["probs"]} if "probs" in kw else {}))
            elif what == "greedy_cigar":
                v = o.greedy(hb, k=kw["k"], mode=1, cigars=True)
            elif what == "simd_ed":
                v = o.simd_ed(hb, kw["t"], True, self.asm.FILTER_CLEAN, (0, 0, 0))[0]
            elif what == "simd_ed_affine":
                v = o.simd_ed_affine(hb, *kw["setting"])[0]
            elif what == "shd":
                v = o.shd(hb, kw["e"])
            else:
                raise KeyError(what)
            self._want[key] = v
        return self._want[key]

    def dev(self, name, array):
        """a device copy of a host array, made once (with no gate pending)"""
        if name not in self._dev:
            self._dev[name] = self.torch.from_numpy(np.ascontiguousarray(array)).cuda()
            self.torch.cuda.synchronize()
        return self._dev[name]

    def close(self):
        for b in self._batch.values():
            b.free()
        self._batch.clear()
        self._dev.clear()


def i32(torch, n):
    return torch.empty(max(n, 1), dtype=torch.int32, device="cuda")


def answers_for(nw):
    """read_answer_file's integers for `accuracy`: INT32_MIN ("use the NW penalty") except on every third pair, where the answer
    is the NW penalty + 1 — different from NW there, by construction"""
    ans = np.full(nw.size, INT32_MIN, np.int32)
    ans[::3] = nw[::3] + 1
    return ans


def counters_for(n, nw=None, leap=None, greedy=None, answers=None):
    """{total_tests, nw_correct, LEAP_correct, greedy_correct} of benchmark_utils.h:238,249-255 from host arrays"""
    if nw is None and answers is None:
        return np.array([n, 0, 0, 0], np.int64)
    ans = np.full(n, INT32_MIN, np.int64) if answers is None else answers.astype(np.int64)
    if nw is not None:
        ans = np.where(ans == INT32_MIN, nw.astype(np.int64), ans)
    hit = lambda a: 0 if a is None else int(((a.astype(np.int64) == ans) & (ans != INT32_MIN)).sum())  # noqa: E731
    return np.array([n, hit(nw), hit(leap), hit(greedy)], np.int64)


# ---- the enqueue-only entry points over a resident batch (group A; group F makes the same calls) ----
# name -> (workload, n, what the call writes, maker); maker(cases) -> dict(outs, stale, produce, call, check)
CIGAR_CAP = 48


def _plain(aligner, wl, n, want_what, params_kw=None, want_kw=None):
    def make(cs):
        asm, torch = cs.asm, cs.torch
        batch, out = cs.batch(wl, n), i32(torch, n)
        params = asm.Params.default(**(params_kw or {}))
        want = cs.want(want_what, wl, n, **(want_kw or {}))
        return dict(outs=[out], stale=lambda: None, produce=lambda: None,
                    call=lambda: cs.eng.align_async(batch, aligner, params, out.data_ptr()),
                    check=lambda got, name: assert_equal(name, got[0][:n], want))
    return make


def _hinted_leap(wl, n, k):
    def make(cs):
        asm, torch = cs.asm, cs.torch
        batch, out, hint = cs.batch(wl, n), i32(torch, n), i32(torch, n)
        nw_dev = cs.dev(("nw", wl, n), cs.want("nw", wl, n))
        params = asm.Params.default(k=k)
        want = cs.want("leap", wl, n, k=k)
        return dict(outs=[out], stale=lambda: hint.zero_(), produce=lambda: hint.copy_(nw_dev),
                    call=lambda: cs.eng.align_hinted_async(batch, asm.LEAP, params, hint.data_ptr(), out.data_ptr()),
                    check=lambda got, name: assert_equal(name, got[0][:n], want))
    return make


def _greedy_cigar(wl, n, k):
    def make(cs):
        asm, torch = cs.asm, cs.torch
        batch = cs.batch(wl, n)
        pen = i32(torch, n)
        ops = torch.empty(n * CIGAR_CAP, dtype=torch.int16, device="cuda")
        nops = torch.empty(n, dtype=torch.uint8, device="cuda")
        params = asm.Params.default(k=k)
        want_cost, want_cigars = cs.want("greedy_cigar", wl, n, k=k)

        def check(got, name):
            assert_equal(name + " cost", got[0][:n], want_cost)
            rows, counts = got[1].view(np.uint16).reshape(n, CIGAR_CAP), got[2]
            assert int(counts.max()) <= CIGAR_CAP, (name, int(counts.max()))  # also: no sentinel (0x7f) left in the counts
            cig = asm.decode_cigars(rows, counts, CIGAR_CAP)
            bad = [i for i in range(n) if cig[i] != want_cigars[i]]
            assert not bad, (name, len(bad), bad[:3], [cig[i] for i in bad[:3]], [want_cigars[i] for i in bad[:3]])
        return dict(outs=[pen, ops, nops], stale=lambda: None, produce=lambda: None,
                    call=lambda: cs.eng.greedy_cigar_async(batch, params, pen.data_ptr(), ops.data_ptr(), CIGAR_CAP, nops.data_ptr()),
                    check=check)
    return make


def _filter(kind, wl, n, **kw):
    def make(cs):
        asm, torch = cs.asm, cs.torch
        batch, out = cs.batch(wl, n), i32(torch, n)
        if kind == "simd_ed":
            want = cs.want("simd_ed", wl, n, t=kw["t"])
            call = lambda: cs.eng.simd_ed_async(batch, kw["t"], out.data_ptr(), shd=True, mode=asm.FILTER_CLEAN)  # noqa: E731
        elif kind == "simd_ed_affine":
            want = cs.want("simd_ed_affine", wl, n, setting=kw["setting"])
            g, af, x, o, e = kw["setting"]
            call = lambda: cs.eng.simd_ed_affine_async(batch, g, af, x, o, e, out.data_ptr())  # noqa: E731
        else:
            want = cs.want("shd", wl, n, e=kw["e"])
            call = lambda: cs.eng.shd_filter_async(batch, kw["e"], out.data_ptr())  # noqa: E731
        return dict(outs=[out], stale=lambda: None, produce=lambda: None, call=call,
                    check=lambda got, name: assert_equal(name, got[0][:n], want))
    return make


def _pack_then_nw(wl, n):
    def make(cs):
        asm, torch = cs.asm, cs.torch
        batch, out = cs.batch(wl, n), i32(torch, n)
        assert batch.download_planes()[2].tolist() != list(range(n)), "the batch is meant to be bucketed by width class"
        params = asm.Params.default()
        want = cs.want("nw", wl, n)

        def call():
            cs.eng.pack_async(batch)
            cs.eng.align_async(batch, asm.NW, params, out.data_ptr())
        return dict(outs=[out], stale=lambda: None, produce=lambda: None, call=call,
                    check=lambda got, name: assert_equal(name, got[0][:n], want))
    return make


def _count_equal(wl, n):
    def make(cs):
        torch = cs.torch
        nw, leap = cs.want("nw", wl, n), cs.want("leap", wl, n, k=3)
        assert 0 < int((nw == leap).sum()) < n  # the stale fill (all pairs equal) gives another count
        nw_dev, leap_dev = cs.dev(("nw", wl, n), nw), cs.dev(("leap3", wl, n), leap)
        a, b = i32(torch, n), i32(torch, n)
        count = torch.empty(1, dtype=torch.int64, device="cuda")

        def stale():
            a.zero_(), b.zero_()

        def produce():
            a.copy_(nw_dev), b.copy_(leap_dev), count.zero_()
        return dict(outs=[count], stale=stale, produce=produce,
                    call=lambda: cs.eng.count_equal_async(a.data_ptr(), b.data_ptr(), n, count.data_ptr()),
                    check=lambda got, name: assert_equal(name, got[0], np.array([int((nw == leap).sum())], np.int64)))
    return make


def _accuracy(wl, n):
    def make(cs):
        torch = cs.torch
        assert n % 4
        nw, leap, greedy = cs.want("nw", wl, n), cs.want("leap", wl, n, k=3), cs.want("greedy", wl, n, k=3)
        ans = answers_for(nw)
        want = counters_for(n, nw, leap, greedy, ans)
        assert (want != counters_for(n, nw, leap, greedy, None)).any()  # the stale answers give other counters
        d = [cs.dev((w, wl, n), v) for w, v in (("nw", nw), ("leap3", leap), ("greedy3", greedy))]
        ans_dev = cs.dev(("answers", wl, n), ans)
        answers, counters = i32(torch, n), torch.empty(4, dtype=torch.int64, device="cuda")

        def produce():
            answers.copy_(ans_dev), counters.zero_()
        return dict(outs=[counters], stale=lambda: answers.fill_(INT32_MIN), produce=produce,
                    call=lambda: cs.eng.accuracy_async(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, counters.data_ptr(),
                                                       answers.data_ptr()),
                    check=lambda got, name: assert_equal(name, got[0], want))
    return make


ASYNC_CASES = {
    "nw_unit_pair2": _plain(0, "C2", 4099, "nw"),
    "nw_affine_todo": _plain(0, "C5", 3001, "nw", dict(x=2, o=3, e=1), dict(x=2, o=3, e=1)),
    "leap_k3_hinted": _hinted_leap("C2", 4099, 3),
    "leap_k30_sorted": _hinted_leap("C3", 1500, 30),
    "greedy_k3_rank_table": _plain(2, "C2", 4099, "greedy", dict(k=3), dict(k=3)),
    "greedy_k17_pair_queue": _plain(2, "C2", 2051, "greedy", dict(k=17), dict(k=17)),
    "greedy_k40_wide": _plain(2, "C2", 1027, "greedy", dict(k=40), dict(k=40)),
    "greedy_cigar_k17": _greedy_cigar("C2", 2051, 17),
    "simd_ed_clean_t8_shd": _filter("simd_ed", "C2", 4099, t=8),
    "simd_ed_affine": _filter("simd_ed_affine", "C5", 3001, setting=(12, 120, 4, 6, 2)),
    "shd_e3": _filter("shd", "C2", 4099, e=3),
    "pack_then_nw_bucketed": _pack_then_nw("C5", 4611),
    "count_equal": _count_equal("C2", 4099),
    "accuracy_answers": _accuracy("C2", 4099),
}


# ---- reads for the mapper rows of the synchronous group ----
def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def simple_reads(seqs, n, seed, m=100, frag=300):
    """n mates pairs from the long sequences of map_cases.reference_small(): fragments of `frag` bases in FR orientation, up to two
    substitutions per mate -> (mate 1 list, mate 2 list)"""
    rng = random.Random(seed)
    big = [s.upper() for s in seqs if len(s) >= 10 * frag]
    r1, r2 = [], []
    for _ in range(n):
        s = rng.choice(big)
        a = rng.randrange(len(s) - frag)
        f = s[a:a + frag].replace("N", "A")
        mates = [f[:m], revcomp(f[-m:])]
        for q in range(2):
            t = list(mates[q])
            for _ in range(rng.randrange(3)):
                p = rng.randrange(m)
                t[p] = rng.choice([c for c in "ACGT" if c != t[p]])
            mates[q] = "".join(t)
        r1.append(mates[0]), r2.append(mates[1])
    return r1, r2


def write_fastq(path, reads, seed=5):
    rng = random.Random(seed)
    with open(path, "w") as fh:
        for t, q in enumerate(reads):
            fh.write("@r%d\n%s\n+\n%s\n" % (t, q, "".join(chr(rng.randrange(33, 74)) for _ in q)))


def write_fasta(path, seqs, width=70):
    with open(path, "w") as fh:
        for r, s in enumerate(seqs):
            fh.write(">seq%d some text\n" % r)
            for a in range(0, len(s), width):
                fh.write(s[a:a + width] + "\n")


# What the module was seen to catch.  Three libraries with one contract broken each, the module run once against each on one
# MI355X.  A process there has four hardware queues, and two streams that share a queue run in submission order, which can hide
# an escaped launch; the switch cases therefore repeat over several second streams (test_gpu_stream_order._targets).
#   1. asm_set_stream keeps launching on the handle's own stream: 52 of 89 fail: all 28 of A, 15 of 16 of B (greedy_only with
#      repack 3 passes), C.4, C.5, D, and of E upload/download, download_planes, simd_ed, the tails and both in-memory mappers.
#      The other six rows of E pass: coverage, the four file-mapper rows and build_index_file spend more host time than the
#      200 ms of the longest gate even after a warm-up call, so the event behind the gate is complete when they return whether
#      they waited or not.  For these six only the equality with a fresh engine is tested, not the waiting.
#   2. switch_stream without the wait on ev_switch: C.1 (both), C.2 (both) and the Greedy k = 17 row of C.3 (d_pair_queue) fail,
#      the last on the first second stream: the pairs of one call are never computed.  The LEAP k = 30 (d_sort) and affine NW
#      (d_todo) rows of C.3 pass on all four second streams, with the second call starting 0, 1/4, 1/2 and 3/4 of a call behind the
#      first: no wrong number came out of these two scratch buffers.  Those two rows pin the results across a switch; they were
#      not seen to catch the missing order.
#   3. switch_stream without pipe.join_into: C.4 fails, on the first second stream: the counters copied there hold one of the two
#      calls (1500, 1500, 1263, 219 against 3000, 3000, 2526, 438).  C.4 runs the wide-band workload (C3, k = 30, all three
#      outputs: 0.38 ms of overlapped work); with the 0.2 ms of the C2 workload the copies came out right under this mutation.
