"""The caller-stream contract of include/asm_mi355x.h and INTEGRATION.md ("Streams"): after asm_set_stream everything the library
enqueues is ordered with the caller's work on that stream; NULL is HIP's legacy default stream, which is torch's default stream;
a switch orders the new stream behind everything queued on the old one (pool blocks, handle scratch and overlapped calls
included); and the calls the header marks "Enqueue only" return while earlier work of the stream is still running.

Every ordering case holds the library's work back behind a gate (a bounded spin the caller enqueues on its stream, see
tests/stream_cases.py) and compares what a torch copy on the same stream sees with the CPU oracle.  The groups: A every
enqueue-only entry point on one caller stream and on torch's default stream, B asm_run_benchmark_async in its four repack forms,
C switches, D two handles on two streams, E the synchronous calls, F the host side of "enqueue only".

The engines here are the module's own; the session-wide `engine` fixture stays on its own stream."""
import types

import numpy as np
import pytest

from tests import map_cases
from tests import stream_cases as sc
from tests.oracle_binding import SIMD_WARM_STATE

pytestmark = pytest.mark.gpu


def _context(asm, oracle):
    import torch

    if asm.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests must run on the GPU box; there is no CPU fallback")
    eng = asm.Engine(0)
    return types.SimpleNamespace(asm=asm, oracle=oracle, torch=torch, eng=eng, cs=sc.Cases(asm, oracle, torch, eng), made={},
                                 S=torch.cuda.Stream(), S2=torch.cuda.Stream(), index=None, seqs=None)


def _close(c):
    c.torch.cuda.synchronize()
    c.made.clear()
    if c.index is not None:
        c.index.free()
    c.cs.close()
    c.eng.close()


@pytest.fixture(scope="module")
def gate():
    import torch

    return sc.Gate(torch)


@pytest.fixture(scope="module")
def ctx(asm, oracle, gate):
    """the engine whose stream the tests switch, with two caller streams"""
    c = _context(asm, oracle)
    c.gate = gate
    yield c
    _close(c)


@pytest.fixture(scope="module")
def other(asm, oracle, gate):
    """a second handle for group D"""
    c = _context(asm, oracle)
    c.gate = gate
    yield c
    _close(c)


@pytest.fixture(scope="module")
def plain(asm, oracle):
    """a fresh engine that stays on its own stream: what the synchronous calls of group E must return"""
    c = _context(asm, oracle)
    yield c
    _close(c)


@pytest.fixture(scope="module")
def pool_engine(asm):
    """an engine whose pool holds nothing but what case C.2 puts there"""
    eng = asm.Engine(0)
    yield eng
    eng.close()


def use(c, which):
    """puts c.eng on the caller's stream of this variant -> the torch stream"""
    torch = c.torch
    if which == "default":
        if torch.cuda.default_stream().cuda_stream != 0:
            pytest.skip("torch's default stream is not HIP's legacy default stream here: cuda_stream = %d"
                        % torch.cuda.default_stream().cuda_stream)
        c.eng.set_stream(None)
        return torch.cuda.default_stream()
    c.eng.set_stream(c.S.cuda_stream)
    return c.S


def made(c, name, which, stream):
    """the tensors and closures of one row of stream_cases.ASYNC_CASES, allocated under the stream they are used on"""
    key = (name, which)
    if key not in c.made:
        with c.torch.cuda.stream(stream):
            c.made[key] = sc.ASYNC_CASES[name](c.cs)
        c.torch.cuda.synchronize()
    return c.made[key]


def test_torch_default_stream_is_hips_legacy_default_stream(ctx):
    """asm_set_stream(NULL) is torch's default stream because that stream's handle is 0"""
    assert ctx.torch.cuda.default_stream().cuda_stream == 0
    with ctx.torch.cuda.stream(ctx.S):
        assert ctx.torch.cuda.current_stream().cuda_stream == ctx.S.cuda_stream != 0


# ---- A: one caller stream, every enqueue-only entry point ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["stream", "default"])
@pytest.mark.parametrize("name", list(sc.ASYNC_CASES))
def test_a_call_is_ordered_with_the_callers_work(ctx, name, which):
    S = use(ctx, which)
    case = made(ctx, name, which, S)
    got = sc.ordered(ctx.torch, ctx.gate, S, "A/%s/%s" % (name, which), case["stale"], case["produce"], case["call"], case["outs"])
    case["check"](got, name)


# ---- B: asm_run_benchmark_async ------------------------------------------------------------------------------------------------
MASKS = {"nw_leap_greedy": ("C2", 4099, 3, (True, True, True)), "leap_greedy_first": ("C3", 1500, 30, (False, True, True)),
         "greedy_only": ("C2", 4099, 3, (False, False, True)),
         "wide_band_all": ("C3", 1500, 30, (True, True, True))}  # C.4 only: the longest chain of overlapped work


def _bench_case(c, mask, which, stream):
    key = ("bench", mask, which)
    if key not in c.made:
        torch, cs = c.torch, c.cs
        wl, n, k, on = MASKS[mask]
        with torch.cuda.stream(stream):
            sets = [[sc.i32(torch, n) if q else None for q in on] for _ in range(2)]
            counters = torch.empty(4, dtype=torch.int64, device="cuda")
        want = [cs.want("nw", wl, n) if on[0] else None, cs.want("leap", wl, n, k=k) if on[1] else None,
                cs.want("greedy", wl, n, k=k) if on[2] else None]
        c.made[key] = types.SimpleNamespace(batch=cs.batch(wl, n), n=n, params=c.asm.Params.default(k=k), sets=sets, counters=counters,
                                            want=want, want_counters=2 * sc.counters_for(n, *want),
                                            outs=[t for s in sets for t in s if t is not None] + [counters])
        torch.cuda.synchronize()
    return c.made[key]


def _bench_call(c, b, s, repack):
    p = [None if t is None else t.data_ptr() for t in b.sets[s]]
    c.eng.run_benchmark_async(b.batch, b.params, p[0], p[1], p[2], b.counters.data_ptr(), repack=repack)


def _bench_check(b, got, name):
    it = iter(got)
    for s in range(2):
        for q, w in enumerate(b.want):
            if w is not None:
                sc.assert_equal("%s set %d %s" % (name, s, ("nw", "leap", "greedy")[q]), next(it)[:b.n], w)
    sc.assert_equal(name + " counters", next(it), b.want_counters)


@pytest.mark.parametrize("repack", [0, 1, 2, 3])
@pytest.mark.parametrize("mask,which", [(m, "stream") for m in MASKS if m != "wide_band_all"] + [("nw_leap_greedy", "default")])
def test_b_two_benchmark_calls_behind_one_gate(ctx, mask, which, repack):
    S = use(ctx, which)
    b = _bench_case(ctx, mask, which, S)
    overlapped = repack == 3 and mask != "leap_greedy_first"  # the Greedy-first shape runs as repack = 2 (asm_mi355x.h)

    def call():
        _bench_call(ctx, b, 0, repack)
        _bench_call(ctx, b, 1, repack)
        if overlapped:  # the misuse guard: the previous overlapped call's arrays again, without a join
            with pytest.raises(ctx.asm.AsmError) as err:
                _bench_call(ctx, b, 1, repack)
            assert err.value.code == -1

    got = sc.ordered(ctx.torch, ctx.gate, S, "B/%s/repack%d/%s" % (mask, repack, which), lambda: None, b.counters.zero_, call, b.outs,
                     after=ctx.eng.pipeline_join_async if repack == 3 else None)
    _bench_check(b, got, "%s repack=%d" % (mask, repack))


# ---- C: switching streams ------------------------------------------------------------------------------------------------------
def _gate_for(c, name, stream, fn):
    with c.torch.cuda.stream(stream):
        return c.gate.length(name, sc.timed(c.torch, stream, fn))


@pytest.mark.parametrize("to", ["second_stream", "own_stream"])
def test_c1_results_are_visible_across_a_switch(ctx, to):
    torch, eng, cs, asm = ctx.torch, ctx.eng, ctx.cs, ctx.asm
    wl, n = "C2", 4099
    batch, params = cs.batch(wl, n), asm.Params.default()
    want = cs.dev(("nw", wl, n), cs.want("nw", wl, n))
    eng.set_stream(ctx.S.cuda_stream)
    with torch.cuda.stream(ctx.S):
        out, count = sc.i32(torch, n), torch.zeros(1, dtype=torch.int64, device="cuda")
    ms = _gate_for(ctx, "C1/%s" % to, ctx.S, lambda: eng.align_async(batch, asm.NW, params, out.data_ptr()))
    try:
        with torch.cuda.stream(ctx.S):
            sc.sentinel1(out)
            torch.cuda.synchronize()
            ctx.gate.start(ms)
            eng.align_async(batch, asm.NW, params, out.data_ptr())
        if to == "second_stream":
            eng.set_stream(ctx.S2.cuda_stream)
            eng.count_equal_async(out.data_ptr(), want.data_ptr(), n, count.data_ptr())
            ctx.S2.synchronize()
        else:
            eng.reset_stream()
            eng.count_equal_async(out.data_ptr(), want.data_ptr(), n, count.data_ptr())
            eng.synchronize()
        got = int(count.cpu()[0])
    finally:
        torch.cuda.synchronize()
    assert got == n, "%d of %d penalties were there when the new stream compared them" % (got, n)


@pytest.mark.parametrize("how,n", [("upload", 4099), ("generate", 6151)])
def test_c2_pool_blocks_survive_a_switch(ctx, pool_engine, how, n):
    """batch A is freed while its kernel is still queued behind the gate on S1; batch B, made under S2, gets A's blocks"""
    torch, asm, eng = ctx.torch, ctx.asm, pool_engine
    cfg, _, params = asm.workload("C2")
    first = {"A": 7000, "B": 9000}
    hb = {q: asm.generate_pairs(cfg, first[q], n) for q in first}
    want = {q: ctx.oracle.nw(hb[q]) for q in first}
    make = (lambda q: eng.upload(hb[q])) if how == "upload" else (lambda q: eng.generate(cfg, first[q], n))
    eng.set_stream(ctx.S.cuda_stream)
    with torch.cuda.stream(ctx.S):
        out = {q: sc.i32(torch, n) for q in first}
    a = make("A")
    b = None
    ms = _gate_for(ctx, "C2/%s" % how, ctx.S, lambda: eng.align_async(a, asm.NW, params, out["A"].data_ptr()))
    try:
        with torch.cuda.stream(ctx.S):
            sc.sentinel1(*out.values())
            torch.cuda.synchronize()
            ctx.gate.start(ms)
            eng.align_async(a, asm.NW, params, out["A"].data_ptr())
        a.free()  # its blocks go idle while its kernel is still queued
        eng.set_stream(ctx.S2.cuda_stream)
        b = make("B")
        eng.align_async(b, asm.NW, params, out["B"].data_ptr())
        ctx.S.synchronize()
        ctx.S2.synchronize()
        got = {q: out[q].cpu().numpy() for q in first}
    finally:
        torch.cuda.synchronize()
        a.free()  # a no-op when it was freed above
        if b is not None:
            b.free()
        eng.reset_stream()
    for q in first:
        sc.assert_equal("batch %s (%s)" % (q, how), got[q][:n], want[q])


SCRATCH = {"leap_k30_d_sort": ("C3", 1500, "leap", dict(k=30), dict(k=30)), "nw_affine_d_todo": ("C5", 3001, "nw", dict(x=2, o=3, e=1), dict(x=2, o=3, e=1)),
           "greedy_k17_d_pair_queue": ("C2", 2051, "greedy", dict(k=17), dict(k=17))}


def _targets(c, fresh):
    """the streams a switch case switches to: the module's second stream and `fresh` new ones.  The runtime deals streams out over
    the process's hardware queues as they are created, and two streams on one queue run in submission order whatever the library
    does; over several targets some do not share a queue with the streams the case is about.  The case must hold on every one."""
    return [c.S2] + [c.torch.cuda.Stream() for _ in range(fresh)]


@pytest.mark.parametrize("name", list(SCRATCH))
def test_c3_handle_scratch_survives_a_switch(ctx, name):
    """the same call on two batches, the first behind a gate on S1, the second under S2.  S2 holds a gate of its own, started
    right behind the first and longer by a part of the call's ungated time: without the order a switch sets up the second call
    starts while the first is under way, on one set of handle scratch.  Repeated over several second streams (_targets), each with
    another part: started together the two calls can both come out right (the todo lists then hold the slots of both, the work
    sort any valid order), what breaks the first is a reset of the scratch that lands between its kernels."""
    torch, eng, cs, asm = ctx.torch, ctx.eng, ctx.cs, ctx.asm
    wl, n, what, pkw, wkw = SCRATCH[name]
    aligner = {"nw": asm.NW, "leap": asm.LEAP, "greedy": asm.GREEDY}[what]
    params = asm.Params.default(**pkw)
    batches = [cs.batch(wl, n, seed) for seed in (0, 1)]
    want = [cs.want(what, wl, n, seed, **wkw) for seed in (0, 1)]
    hints = [cs.dev(("nw", wl, n, seed), cs.want("nw", wl, n, seed)) if what == "leap" else None for seed in (0, 1)]
    eng.set_stream(ctx.S.cuda_stream)
    with torch.cuda.stream(ctx.S):
        outs = [sc.i32(torch, n), sc.i32(torch, n)]

    def call(q):
        eng.align_hinted_async(batches[q], aligner, params, None if hints[q] is None else hints[q].data_ptr(), outs[q].data_ptr())

    call(1)  # warm-up of the second batch (its first Greedy call may block)
    with torch.cuda.stream(ctx.S):
        ungated = sc.timed(torch, ctx.S, lambda: call(0))
    ms = ctx.gate.length("C3/%s" % name, ungated)
    for t, second in enumerate(_targets(ctx, 3)):
        later = min(ms + (0.0, 0.5, 0.25, 0.75)[t] * ungated, sc.GATE_CAP_MS)
        eng.set_stream(ctx.S.cuda_stream)
        try:
            sc.sentinel1(*outs)
            torch.cuda.synchronize()
            with torch.cuda.stream(ctx.S):
                ctx.gate.start(ms)
            with torch.cuda.stream(second):
                ctx.gate.start(later)
            call(0)
            eng.set_stream(second.cuda_stream)
            call(1)
            ctx.S.synchronize()
            second.synchronize()
            got = [o.cpu().numpy() for o in outs]
        finally:
            torch.cuda.synchronize()
        for q in range(2):
            sc.assert_equal("%s batch %d, second stream %d" % (name, q, t), got[q][:n], want[q])


def test_c4_a_switch_joins_the_overlapped_calls(ctx):
    """two repack = 3 calls behind a gate on S1, then set_stream(S2) without asm_pipeline_join_async: what S2 copies is complete.
    Repeated over several second streams (_targets): the calls end on streams of the library, and a second stream that shares a
    hardware queue with those sees their results whether the switch joined them or not."""
    torch, eng = ctx.torch, ctx.eng
    eng.set_stream(ctx.S.cuda_stream)
    b = _bench_case(ctx, "wide_band_all", "switch", ctx.S)
    copies = [torch.empty_like(o) for o in b.outs]

    def two():
        _bench_call(ctx, b, 0, 3)
        _bench_call(ctx, b, 1, 3)

    def joined():
        two()
        eng.pipeline_join_async()

    ms = _gate_for(ctx, "C4/overlapped", ctx.S, joined)
    for t, second in enumerate(_targets(ctx, 5)):
        eng.set_stream(ctx.S.cuda_stream)
        try:
            with torch.cuda.stream(ctx.S):
                sc.sentinel1(*b.outs)
                torch.cuda.synchronize()
                ctx.gate.start(ms)
                sc.sentinel1(*b.outs)
                b.counters.zero_()
                two()
            eng.set_stream(second.cuda_stream)
            with torch.cuda.stream(second):
                for c, o in reversed(list(zip(copies, b.outs))):  # what the calls finish last is copied first
                    c.copy_(o)
                sc.sentinel2(*b.outs)
            second.synchronize()
            got = [c.cpu().numpy() for c in copies]
        finally:
            torch.cuda.synchronize()
            eng.pipeline_join_async()  # ends the run of overlapped calls: these arrays are filled with torch again next
            eng.synchronize()
        _bench_check(b, got, "overlapped calls across a switch, second stream %d" % t)


def test_c5_current_stream_again_and_reset(ctx):
    torch, eng, cs, asm = ctx.torch, ctx.eng, ctx.cs, ctx.asm
    wl, n = "C2", 4099
    batch, params, want = cs.batch(wl, n), asm.Params.default(), cs.want("nw", wl, n)
    S = use(ctx, "stream")
    eng.set_stream(S.cuda_stream)  # the stream already current: accepted, and nothing changes
    case = made(ctx, "nw_unit_pair2", "stream", S)
    got = sc.ordered(torch, ctx.gate, S, "C5/set_twice", case["stale"], case["produce"], case["call"], case["outs"])
    case["check"](got, "after set_stream with the current stream")
    # after reset_stream a call no longer waits for what the former stream gets LATER
    eng.reset_stream()
    eng.reset_stream()
    out = sc.i32(torch, n)
    # Two streams that the runtime put on one hardware queue run in submission order whatever the library does, and a process
    # has few queues: the former stream of this case is one that is SEEN to run beside the handle's own stream, with a short
    # gate and a memset of the library.
    candidates = [S] + [torch.cuda.Stream() for _ in range(8)]
    former = None
    for cand in candidates:
        torch.cuda.synchronize()
        probe = torch.cuda.Event()
        with torch.cuda.stream(cand):
            ctx.gate.start(sc.GATE_FLOOR_MS)
            probe.record(cand)
        eng.memset_async(out.data_ptr(), 0, 4 * n)
        eng.synchronize()
        beside = not probe.query()
        torch.cuda.synchronize()
        if beside:
            former = cand
            break
    assert former is not None, "none of %d torch streams runs beside the handle's own stream" % len(candidates)
    eng.set_stream(former.cuda_stream)
    eng.reset_stream()
    sc.sentinel1(out)
    torch.cuda.synchronize()
    behind = torch.cuda.Event()
    try:
        with torch.cuda.stream(former):
            ctx.gate.start(sc.GATE_CAP_MS)
            behind.record(former)
        eng.align_async(batch, asm.NW, params, out.data_ptr())
        eng.synchronize()
        still_spinning = not behind.query()
        got = eng.to_host(out.data_ptr(), n)
    finally:
        torch.cuda.synchronize()
    assert still_spinning, "asm_synchronize returned only after a gate queued later on the former stream"
    sc.assert_equal("nw on the handle's own stream", got, want)


# ---- D: two handles, two streams -----------------------------------------------------------------------------------------------
def test_d_two_handles_interleaved_on_two_streams(ctx, other):
    torch, asm = ctx.torch, ctx.asm
    e1, e2, s1, s2 = ctx.eng, other.eng, ctx.S, ctx.S2
    e1.set_stream(s1.cuda_stream)
    e2.set_stream(s2.cuda_stream)
    probs = (0.85, 0.05, 0.10)
    p_other = asm.Params.default(k=3, p_match=probs[0], p_mismatch=probs[1], p_indel=probs[2])
    p_aff = asm.Params.default(x=2, o=3, e=1)
    shared = ctx.cs.batch("C2", 2051)  # made by e1, aligned through e2
    jobs = [  # (engine, stream, batch, aligner, params, hint, want)
        (e1, s1, ctx.cs.batch("C2", 4099), asm.GREEDY, asm.Params.default(k=3), None, ctx.cs.want("greedy", "C2", 4099, k=3)),
        (e2, s2, other.cs.batch("C2", 4099, 1), asm.GREEDY, p_other, None, other.cs.want("greedy", "C2", 4099, 1, k=3, probs=probs)),
        (e1, s1, ctx.cs.batch("C3", 1500), asm.LEAP, asm.Params.default(k=30), ctx.cs.dev(("nw", "C3", 1500), ctx.cs.want("nw", "C3", 1500)),
         ctx.cs.want("leap", "C3", 1500, k=30)),
        (e2, s2, other.cs.batch("C5", 3001), asm.NW, p_aff, None, other.cs.want("nw", "C5", 3001, x=2, o=3, e=1)),
        (e1, s1, ctx.cs.batch("C2", 2051), asm.GREEDY, asm.Params.default(k=17), None, ctx.cs.want("greedy", "C2", 2051, k=17)),
        (e2, s2, shared, asm.NW, asm.Params.default(), None, ctx.cs.want("nw", "C2", 2051)),
    ]
    outs = []
    for eng, s, batch, *_ in jobs:
        with torch.cuda.stream(s):
            outs.append(sc.i32(torch, batch.n))
    copies = [torch.empty_like(o) for o in outs]

    def run(q):
        eng, _, batch, aligner, params, hint, _ = jobs[q]
        eng.align_hinted_async(batch, aligner, params, None if hint is None else hint.data_ptr(), outs[q].data_ptr())

    for q in range(len(jobs)):  # warm-up: a first Greedy parameter set blocks
        run(q)
    torch.cuda.synchronize()
    ms1 = _gate_for(ctx, "D/handle1", s1, lambda: [run(q) for q in (0, 2, 4)])
    ms2 = min(sc.GATE_CAP_MS, 1.5 * _gate_for(ctx, "D/handle2", s2, lambda: [run(q) for q in (1, 3, 5)]))
    try:
        sc.sentinel1(*outs)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            ctx.gate.start(ms1)
        with torch.cuda.stream(s2):
            ctx.gate.start(ms2)
        for q in range(len(jobs)):
            with torch.cuda.stream(jobs[q][1]):
                sc.sentinel1(outs[q])
                run(q)
        for q in range(len(jobs)):
            with torch.cuda.stream(jobs[q][1]):
                copies[q].copy_(outs[q])
                sc.sentinel2(outs[q])
        s1.synchronize()
        s2.synchronize()
        got = [c.cpu().numpy() for c in copies]
    finally:
        torch.cuda.synchronize()
    for q, job in enumerate(jobs):
        sc.assert_equal("job %d (handle %d)" % (q, 1 + q % 2), got[q][:job[2].n], job[-1])


# ---- E: synchronous calls on a caller's stream --------------------------------------------------------------------------------
def gated(c, stream, fn, warm=True):
    """fn() with a gate pending on `stream`: it must have waited for the gate when it returns -> what fn returned.  The gate is the
    longest one (GATE_CAP_MS) and, with warm, fn() has run once before (first-use allocations, pinned buffers, file cache), so
    that the host side of the call is short beside the gate: an event behind the gate that is complete at return then means the
    call waited.  Which rows were seen to fail here with a library that ignores asm_set_stream is in stream_cases.py."""
    torch = c.torch
    if warm:
        fn()
    behind = torch.cuda.Event()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(stream):
            c.gate.start(sc.GATE_CAP_MS)
            behind.record(stream)
            result = fn()
            waited = behind.query()
    finally:
        torch.cuda.synchronize()
    assert waited, "the call returned while earlier work of its stream was still running"
    return result


def same(name, got, want):
    if isinstance(want, dict):
        assert set(got) == set(want), name
        for key in want:
            same("%s[%s]" % (name, key), got[key], want[key])
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), name
    elif isinstance(want, (tuple, list)) and want and isinstance(want[0], np.ndarray):
        assert len(got) == len(want), name
        for q, (g, w) in enumerate(zip(got, want)):
            same("%s[%d]" % (name, q), g, w)
    else:
        assert got == want, name


def _index(c):
    if c.index is None:
        c.seqs = map_cases.reference_small()
        c.index = c.eng.build_index(c.seqs, k=12)
    return c.index


def test_e_upload_then_download(ctx, plain):
    S = use(ctx, "stream")
    hb = ctx.cs.hb("C5", 4611, 3)
    batch = gated(ctx, S, lambda: ctx.eng.upload(hb), warm=False)
    try:
        got = gated(ctx, S, batch.download)
    finally:
        batch.free()
    for f in ("reads", "read_off", "refs", "ref_off"):
        same(f, getattr(got, f), getattr(hb, f))
    ref = plain.eng.upload(hb)
    try:
        back = ref.download()
    finally:
        ref.free()
    for f in ("reads", "read_off", "refs", "ref_off"):
        same(f, getattr(got, f), getattr(back, f))


def test_e_download_planes(ctx, plain):
    S = use(ctx, "stream")
    batch = ctx.cs.batch("C5", 4611)
    same("planes", gated(ctx, S, batch.download_planes), plain.cs.batch("C5", 4611).download_planes())


def test_e_coverage(ctx, plain):
    S = use(ctx, "stream")
    params = ctx.asm.Params.default()
    batch = ctx.cs.batch("C2", 2051)  # made with no gate pending: upload would take the wait on itself
    got = gated(ctx, S, lambda: ctx.eng.coverage(batch, params))
    same("coverage", got, plain.eng.coverage(plain.cs.batch("C2", 2051), params))


def test_e_simd_ed_sequential(ctx, plain):
    S = use(ctx, "stream")
    asm = ctx.asm
    run = lambda c: c.eng.simd_ed(c.cs.batch("C2", 4099), 3, True, asm.FILTER_SEQUENTIAL, SIMD_WARM_STATE)  # noqa: E731
    ctx.cs.batch("C2", 4099)  # made with no gate pending
    got = gated(ctx, S, lambda: run(ctx))
    same("simd_ed sequential", got, run(plain))
    sc.assert_equal("simd_ed sequential", got, ctx.oracle.simd_ed(ctx.cs.hb("C2", 4099), 3, True, asm.FILTER_SEQUENTIAL, SIMD_WARM_STATE)[0])


def test_e_tail_summary_then_resolve_tails(ctx, plain):
    S = use(ctx, "stream")
    asm = ctx.asm
    params = asm.Params.default()
    hb = ctx.cs.hb("C2", 4099, 5)  # a batch of its own: resolve_tails turns it into a sequential-mode batch

    def resolved(c):
        c.eng.resolve_tails(c.cs.batch("C2", 4099, 5), None)
        return c.eng.align(c.cs.batch("C2", 4099, 5), asm.GREEDY, params)

    tb = ctx.cs.batch("C2", 4099, 5)  # made with no gate pending
    summary = gated(ctx, S, lambda: ctx.eng.tail_summary(tb))
    got = gated(ctx, S, lambda: resolved(ctx))
    same("summary", summary, plain.eng.tail_summary(plain.cs.batch("C2", 4099, 5)))
    same("summary (oracle)", summary, ctx.oracle.tail_summary(hb))
    same("greedy after resolve_tails", got, resolved(plain))
    sc.assert_equal("greedy after resolve_tails", got, ctx.oracle.greedy(hb, k=3, mode=0))


@pytest.mark.parametrize("call", ["map_reads", "map_pairs"])
def test_e_in_memory_mappers(ctx, plain, call):
    S = use(ctx, "stream")
    r1, r2 = sc.simple_reads(map_cases.reference_small(), 500, 17)

    def run(c):
        if call == "map_reads":
            return c.eng.map_reads(_index(c), r1, 3)
        return c.eng.map_pairs(_index(c), r1, r2, 3, 100, 600, rescue_errors=5)

    _index(ctx)
    got = gated(ctx, S, lambda: run(ctx))
    assert int(got["mapped"].sum()) > 400
    same(call, got, run(plain))


@pytest.mark.parametrize("fmt", ["sam", "bam"])
@pytest.mark.parametrize("sort", [False, True], ids=["map_file", "map_file_sorted"])
def test_e_file_mappers(ctx, plain, tmp_path, sort, fmt):
    S = use(ctx, "stream")
    reads, _ = sc.simple_reads(map_cases.reference_small(), 2000, 23)
    fq = str(tmp_path / "reads.fq")
    sc.write_fastq(fq, reads)
    names = ["seq%d" % r for r in range(len(map_cases.reference_small()))]
    header = "@HD\tVN:1.6\n"

    def run(c, path):
        c.eng.set_output_format(fmt)
        try:
            stats = c.eng.map_file(_index(c), names, fq, path, 3, header=header, sort=sort)
        finally:
            c.eng.set_output_format("sam")
        with open(path, "rb") as fh:
            return stats["reads"], stats["mapped"], fh.read()

    _index(ctx)
    got = gated(ctx, S, lambda: run(ctx, str(tmp_path / "gated.out")))
    want = run(plain, str(tmp_path / "plain.out"))
    assert got[0] == 2000 and got[1] > 1600
    assert got == want


def test_e_build_index_file(ctx, plain, tmp_path):
    S = use(ctx, "stream")
    seqs = map_cases.reference_small()
    fa = str(tmp_path / "ref.fa")
    sc.write_fasta(fa, seqs)
    total = sum(len(s) for s in seqs)

    def run(c):
        index, _ = c.eng.build_index_file(fa, k=12)
        try:
            return list(index.lengths), list(index.names), index.text(0, total)
        finally:
            index.free()

    got = gated(ctx, S, lambda: run(ctx))
    assert got[0] == [len(s) for s in seqs] and got[2] == "".join(seqs).upper().encode()
    assert got == run(plain)


# ---- F: "enqueue only" means the host returns ------------------------------------------------------------------------------------
def _host_calls(c, S):
    """name -> closure, for every call include/asm_mi355x.h marks "Enqueue only" (sequential-mode simd_ed is documented as
    returning after its scans and the first use of a Greedy parameter set as blocking: the warm-up call takes that away)"""
    asm, eng, cs = c.asm, c.eng, c.cs
    calls = {name: made(c, name, "stream", S)["call"] for name in sc.ASYNC_CASES}
    b = _bench_case(c, "nw_leap_greedy", "stream", S)
    for repack in (0, 1, 2):
        calls["run_benchmark_repack%d" % repack] = lambda repack=repack: _bench_call(c, b, 0, repack)

    def overlapped():
        _bench_call(c, b, 0, 3)
        _bench_call(c, b, 1, 3)
        eng.pipeline_join_async()
    calls["run_benchmark_repack3_and_pipeline_join"] = overlapped
    calls["pack"] = lambda: eng.pack_async(cs.batch("C2", 4099))
    calls["resolve_tails"] = lambda: eng.resolve_tails(cs.batch("C2", 4099, 5), None)
    out = made(c, "simd_ed_affine", "stream", S)["outs"][0]
    c5 = cs.batch("C5", 3001)
    calls["simd_ed_affine_shd"] = lambda: eng.simd_ed_affine_async(c5, 12, 120, 4, 6, 2, out.data_ptr(), shd_threshold=5)
    calls["simd_ed_affine_mode"] = lambda: eng.simd_ed_affine_async(c5, 12, 120, 4, 6, 2, out.data_ptr(), shd_threshold=5, mode=asm.LEAP_LOCAL)
    return calls


HOST_CALLS = list(sc.ASYNC_CASES) + ["run_benchmark_repack%d" % r for r in (0, 1, 2)] + [
    "run_benchmark_repack3_and_pipeline_join", "pack", "resolve_tails", "simd_ed_affine_shd", "simd_ed_affine_mode"]


@pytest.mark.parametrize("name", HOST_CALLS)
def test_f_enqueue_only_call_returns_while_the_stream_is_busy(ctx, name):
    torch = ctx.torch
    S = use(ctx, "stream")
    call = _host_calls(ctx, S)[name]
    behind = torch.cuda.Event()
    try:
        with torch.cuda.stream(S):
            call()  # warm-up with the same arguments
            torch.cuda.synchronize()
            ctx.gate.start(sc.GATE_CAP_MS)
            behind.record(S)
            call()
            returned_early = not behind.query()
    finally:
        torch.cuda.synchronize()
        ctx.eng.synchronize()
    assert returned_early, "%s came back only after the %d ms of earlier work on its stream" % (name, sc.GATE_CAP_MS)
