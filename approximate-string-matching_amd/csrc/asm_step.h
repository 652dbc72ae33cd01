// The step scheduler: asm_run_benchmark_async orders pack, NW, LEAP, Greedy and the counters of a call over the caller's stream
// and the library's three (StepPipe, asm_capi.hip).  Each schedule is one function: a linear list of waits, stages and records.
// With it asm_pipeline_join_async and asm_profile_enable / asm_profile_read.  Included by asm_capi.hip inside its extern "C" block.
#pragma once

extern "C++" {

/* repack = 2/3: the other set of planes becomes the batch's current one.  Its own inverse: a call whose pack fails flips back. */
static void batch_flip_planes(asm_batch* b) {
    std::swap(b->d_planes, b->d_planes_alt);
    std::swap(b->d_lens, b->d_lens_alt);
    b->cur ^= 1;
    for (int q = 0; q < b->nb; q++) {
        b->bk[q].planes = b->d_planes + b->pb.plane_off[q];
        b->bk[q].lens = b->d_lens + b->pb.start[q];
    }
}

/* asm_run_benchmark_async reaches its other streams through the ordinary entry points, which launch on h->stream: for the life
 * of this object that is `s`, and afterwards what it was before, on every way out of the scope. */
struct StreamBorrow {
    asm_handle* const h;
    const hipStream_t back;
    StreamBorrow(asm_handle* handle, hipStream_t s) : h(handle), back(handle->stream) { h->stream = s; }
    StreamBorrow(const StreamBorrow&) = delete;
    StreamBorrow& operator=(const StreamBorrow&) = delete;
    ~StreamBorrow() { h->stream = back; }
};

/* One asm_run_benchmark_async call past its checks: its arguments, the caller's stream, the stages as the schedules name them, and
 * the schedules.  `slot`: optional per-kernel timing inside the caller's timed region (asm_profile_enable) — begin and end events
 * of pack, NW, LEAP, Greedy, or null when profiling is off or used up; the mask of the stages launched is filed on every way out. */
struct Step {
    asm_handle* const h;
    StepPipe& pp;
    asm_batch* const b;
    const asm_params* const p;
    const int repack; /* after the downgrade of a call that cannot overlap */
    int32_t *const d_nw, *const d_leap, *const d_greedy;
    const int32_t* const d_answers;
    unsigned long long* const d_counters;
    const hipStream_t main; /* the caller's stream */
    hipEvent_t* const slot;
    unsigned mask = 0u;
    bool pipelined = false; /* the pack of this call went to the pack stream */
    ~Step() { if (slot) h->prof_mask.push_back(mask); }

    /* One timed stage (q: 0 pack, 1 NW, 2 LEAP, 3 Greedy): `run` enqueues it through the ordinary entry points on stream s.  A
     * selected stage is bracketed by the slot's events on that stream; its mask bit is set with the begin event, and a stage that
     * failed gets no end event.  Returns the first error. */
    template <class F> int stage(int q, hipStream_t s, F&& run) {
        const bool timed = slot && (h->prof_select & (1u << q));
        if (timed) {
            HIPCHK(h, hipEventRecord(slot[2 * q], s));
            mask |= 1u << q;
        }
        const auto borrowed = [&] { StreamBorrow on(h, s); return run(); };
        const int rc = s == h->stream ? run() : borrowed();
        if (timed && !rc) HIPCHK(h, hipEventRecord(slot[2 * q + 1], s));
        return rc;
    }
    int nw(hipStream_t s) { return stage(1, s, [&] { return asm_align_batch_async(h, b, ASM_NW, p, d_nw); }); }
    int leap(hipStream_t s, const int32_t* d_hint) { return stage(2, s, [&] { return asm_align_batch_hinted_async(h, b, ASM_LEAP, p, d_hint, d_leap); }); }
    int greedy(hipStream_t s) { return stage(3, s, [&] { return asm_align_batch_async(h, b, ASM_GREEDY, p, d_greedy); }); }
    int counters(hipStream_t s) { /* not timed */
        StreamBorrow on(h, s);
        return d_counters ? asm_accuracy_async(h, d_nw, d_leap, d_greedy, d_answers, b->n, d_counters) : ASM_OK;
    }
    int pack_pipelined();
    int tail_overlapped();
    int tail_in_order(bool greedy_first);
};

/* (a) Pipelined pack, repack 2 and 3: pack fills the OTHER set of planes on its own stream, so it runs beside the aligners of the
 * previous call (which read the current set) instead of behind them; this call's aligners wait for it.  The set it fills was last
 * read two calls ago (ev_consumed).  The caller guarantees that nothing enqueued since the previous call changes what pack reads
 * (the resident ASCII, the tails).  On every error return the batch points at a plane set that has been packed. */
int Step::pack_pipelined() {
    HIPCHK(h, hipSetDevice(h->device));
    if (!b->d_planes_alt) HIPCHK(h, batch_alloc(b, &b->d_planes_alt, sizeof(uint4) * b->planes_total));
    if (!b->d_lens_alt) HIPCHK(h, batch_alloc(b, &b->d_lens_alt, sizeof(uint32_t) * (size_t)b->n));
    if (!b->ev_consumed[1]) {
        for (hipEvent_t& ev : b->ev_consumed)
            if (!ev) HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(b->ev_consumed[0], main)); /* everything enqueued so far (the batch's creation) */
        HIPCHK(h, hipEventRecord(b->ev_consumed[1], main));
    }
    HIPCHK(h, hipStreamWaitEvent(pp.pack_stream, b->ev_consumed[b->cur ^ 1], 0));
    /* Overlapped calls on DIFFERENT batches (a caller rotating over several resident batches): the plane set of this batch
     * was consumed long ago, so nothing above holds the pack back, and the pack chain would run as many calls ahead as the
     * host has enqueued — thousands of short pack workgroups dispatched beside every persistent Greedy kernel (0.258 ms per
     * step against 0.218 on one batch).  Pace it as one batch paces itself: the pack of call c behind the counters of call
     * c - 2 (the event that also frees that call's output arrays). */
    if (repack == 3 && pp.calls3 >= 2) HIPCHK(h, hipStreamWaitEvent(pp.pack_stream, pp.ev_out[pp.calls3 & 1u], 0));
    if (!pp.pipe_prev) { /* first of a run of pipelined calls: behind whatever the caller's stream holds so far */
        HIPCHK(h, hipEventRecord(pp.ev_fork, main));
        HIPCHK(h, hipStreamWaitEvent(pp.pack_stream, pp.ev_fork, 0));
    }
    /* ... and not before the previous call's persistent Greedy kernel is resident everywhere: pack's thousands of short
     * workgroups, dispatched at the same moment, keep Greedy's 122 KB-LDS workgroups off the CUs (0.280 ms/step); behind
     * the previous NW they find Greedy running and take the slots NW left (0.238).  With overlapped calls (repack = 3) the
     * pack chain runs a call ahead and meets no Greedy launch: no gate there (0.229 against 0.251 gated) */
    if (pp.gate_set && repack == 2) HIPCHK(h, hipStreamWaitEvent(pp.pack_stream, pp.ev_gate, 0));
    pipelined = true;
    const int rc = stage(0, pp.pack_stream, [&] {
        batch_flip_planes(b);
        const int packed = asm_batch_pack_async(h, b);
        if (packed) batch_flip_planes(b); /* nothing enqueued: back to the set that is packed */
        return packed;
    });
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(pp.ev_packed, pp.pack_stream));
    HIPCHK(h, hipStreamWaitEvent(main, pp.ev_packed, 0));
    return ASM_OK;
}

/* (b) OVERLAPPED calls, repack 3 behind its pipelined pack: nothing of this call waits for the previous call's Greedy, and the
 * caller's stream is not joined here (asm_pipeline_join_async does that).  Three chains run through consecutive calls — NW ->
 * LEAP -> counters -> NW -> ... on a stream of the library, Greedy -> Greedy on the side stream, pack -> pack on the pack stream; a
 * call's counters wait for its Greedy, and their event also frees the call's plane set for the pack two calls later (and, with
 * the caller alternating output arrays, says those arrays may be written again). */
int Step::tail_overlapped() {
    pp.last3_out[0] = d_nw, pp.last3_out[1] = d_leap, pp.last3_out[2] = d_greedy, pp.last3_valid = true;
    /* the output arrays were last written two calls ago (the caller alternates): behind that call's counters.  For calls
     * on ONE batch ev_packed already implies it; calls on different batches have nothing else that orders them. */
    const hipEvent_t out_free = pp.ev_out[pp.calls3 & 1u];
    if (pp.calls3 >= 2) {
        HIPCHK(h, hipStreamWaitEvent(main, out_free, 0));
        if (d_greedy) HIPCHK(h, hipStreamWaitEvent(pp.side_stream, out_free, 0));
    }
    if (d_greedy) {
        /* one side stream: Greedy kernels of consecutive calls in a row.  Alternating two streams, so that the next call's
         * workgroups move in as the previous call's leave, was measured at 0.273 ms/step against 0.233 — two persistent
         * kernels that each want a CU's LDS keep each other out */
        HIPCHK(h, hipStreamWaitEvent(pp.side_stream, pp.ev_packed, 0));
        if (int rc = greedy(pp.side_stream)) return rc;
        HIPCHK(h, hipEventRecord(pp.ev_join, pp.side_stream));
    }
    /* NW -> LEAP -> counters of a call, then the next call's NW, in a row on ONE stream (when all three are asked for).
     * Rounds 3-4 launched NW on the caller's stream and LEAP + counters on a stream of the library; under torch the two
     * shared a hardware queue (the runtime spreads streams over four, the handle's idle own stream holds one), which
     * serialised them in exactly this order — and that order is the fast one: with GPU_MAX_HW_QUEUES=8, where the next NW
     * really starts beside this call's LEAP and counters, a step takes 0.219 ms against 0.204.  Saying so explicitly makes
     * the step independent of how the host's streams happen to map to queues (same box: 0.206 at four queues, 0.208 at
     * eight). */
    const hipStream_t chain = (d_nw && d_leap) ? pp.acc_stream : main;
    if (chain != main) HIPCHK(h, hipStreamWaitEvent(chain, pp.ev_packed, 0));
    if (int rc = d_nw ? nw(chain) : ASM_OK) return rc;
    if (int rc = d_leap ? leap(chain, d_nw) : ASM_OK) return rc;
    HIPCHK(h, hipEventRecord(pp.ev_leap, chain));
    HIPCHK(h, hipStreamWaitEvent(pp.acc_stream, pp.ev_leap, 0));
    if (d_greedy) HIPCHK(h, hipStreamWaitEvent(pp.acc_stream, pp.ev_join, 0));
    if (int rc = counters(pp.acc_stream)) return rc;
    HIPCHK(h, hipEventRecord(b->ev_consumed[b->cur], pp.acc_stream));
    HIPCHK(h, hipEventRecord(out_free, pp.acc_stream));
    pp.calls3++;
    HIPCHK(h, hipEventRecord(pp.ev_tail, pp.acc_stream));
    pp.tail_set = pp.pipe_prev = true;
    return ASM_OK;
}

/* (c) In-order tail, repack 0, 1 and 2: everything is back on the caller's stream when the call returns. */
int Step::tail_in_order(bool greedy_first) {
    if (int rc = greedy_first ? greedy(main) : ASM_OK) return rc;
    // Greedy depends only on the packed planes, NW -> LEAP form their own chain (LEAP is scheduled by the NW penalties):
    // run Greedy on a side stream so that the two chains fill each other's launch gaps and tail waves.
    const bool fork = h->overlap && d_greedy && (d_nw || d_leap) && !greedy_first;
    if (fork) {
        HIPCHK(h, hipEventRecord(pp.ev_fork, main));
        HIPCHK(h, hipStreamWaitEvent(pp.side_stream, pp.ev_fork, 0));
        if (int rc = greedy(pp.side_stream)) return rc;
        HIPCHK(h, hipEventRecord(pp.ev_join, pp.side_stream));
    }
    if (d_nw) {
        if (int rc = nw(main)) return rc;
        if (repack == 2) { /* the next call's pack starts behind this point (pack_pipelined) */
            HIPCHK(h, hipEventRecord(pp.ev_gate, main));
            pp.gate_set = true;
        }
    }
    /* LEAP is scheduled by the NW penalties just computed (same work, sorted inside each workgroup) */
    if (int rc = d_leap ? leap(main, greedy_first ? d_greedy : d_nw) : ASM_OK) return rc;
    if (fork) HIPCHK(h, hipStreamWaitEvent(main, pp.ev_join, 0));
    if (int rc = d_greedy && !fork && !greedy_first ? greedy(main) : ASM_OK) return rc; /* or last */
    if (pipelined) HIPCHK(h, hipEventRecord(b->ev_consumed[b->cur], main)); /* Greedy's stream has joined above */
    return counters(main);
}

}  // extern "C++"

int asm_run_benchmark_async(asm_handle* h, asm_batch* b, const asm_params* p, int repack, int32_t* d_nw, int32_t* d_leap,
                            int32_t* d_greedy, const int32_t* d_answers, unsigned long long* d_counters) {
    if (!h || !b || !p) return fail(h, ASM_EINVAL, "asm_run_benchmark_async: NULL argument");
    /* the aligners check again; these checks come before anything is enqueued or flipped */
    int rc = d_nw ? check_params(h, ASM_NW, p, b->maxlen) : ASM_OK;
    if (!rc && d_leap) rc = check_params(h, ASM_LEAP, p, b->maxlen);
    if (!rc && d_greedy) rc = check_params(h, ASM_GREEDY, p, b->maxlen);
    if (rc) return rc;
    // Without NW in the mask, wide-band LEAP (four threads per pair, asm_wave.h) is scheduled by the Greedy penalties:
    // Greedy first, on the same stream — at wide bands both kernels are VALU-bound and side by side they gain nothing (C3:
    // 23.8 ms against 23.6 in a row), while the work-sorted LEAP saves a quarter of its time.
    const bool greedy_first = d_greedy && d_leap && !d_nw && p->k > 5 && h->leap_hint && h->wave_kernels;
    /* A call that asks for overlapped steps but has the Greedy-first shape (or no pairs) runs as a pipelined-pack call: it is
     * ordered like one (behind every earlier overlapped call), and the bookkeeping of the overlapped form starts afresh. */
    if (repack == 3 && (b->n <= 0 || greedy_first)) repack = 2;
    StepPipe& pp = h->pipe;
    /* the contract of repack = 3: consecutive overlapped calls write different arrays (the previous call's counters may still be
     * reading its own).  A caller that forgets is told so instead of getting a race. */
    if (repack == 3 && pp.names_previous_outputs(d_nw, d_leap, d_greedy))
        return fail(h, ASM_EINVAL, "asm_run_benchmark_async: repack = 3 needs output arrays that alternate between two sets (these "
                                   "were the previous call's); asm_pipeline_join_async first to reuse them");
    if (repack != 3) {
        pp.end_overlapped_run();
        if (pp.tail_set) { /* earlier overlapped calls: everything of theirs before anything of this one */
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, pp.join_into(h->stream));
            pp.tail_set = false;
        }
    }
    hipEvent_t* const slot = (int)h->prof_mask.size() < h->prof_cap ? &h->prof_ev[8 * h->prof_mask.size()] : nullptr;
    Step s{h, pp, b, p, repack, d_nw, d_leap, d_greedy, d_answers, d_counters, h->stream, slot};
    if ((repack == 2 || repack == 3) && b->n > 0)
        rc = s.pack_pipelined();
    else if (repack)
        rc = s.stage(0, s.main, [&] { return asm_batch_pack_async(h, b); });
    if (!rc && repack == 3 && s.pipelined) return s.tail_overlapped(); /* sets pipe_prev itself, where the call is complete */
    if (!rc) rc = s.tail_in_order(greedy_first);
    pp.pipe_prev = s.pipelined;
    return rc;
}

int asm_pipeline_join_async(asm_handle* h) {
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_pipeline_join_async: NULL handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, h->pipe.join_into(h->stream));
    h->pipe.rejoin_caller();
    return ASM_OK;
}

int asm_profile_enable(asm_handle* h, int max_calls, unsigned kernel_mask) {
    if (!h || max_calls < 0) return fail(h, ASM_EINVAL, "asm_profile_enable: bad argument");
    h->prof_select = kernel_mask & 0xfu;
    HIPCHK(h, hipSetDevice(h->device));
    for (hipEvent_t ev : h->prof_ev) (void)hipEventDestroy(ev);
    h->prof_ev.clear();
    h->prof_mask.clear();
    h->prof_cap = 0;
    for (int i = 0; i < 8 * max_calls; i++) {
        hipEvent_t ev;
        HIPCHK(h, hipEventCreate(&ev));
        h->prof_ev.push_back(ev);
    }
    h->prof_cap = max_calls;
    return ASM_OK;
}

int asm_profile_read(asm_handle* h, float* ms, int cap_calls, int* n_calls) {
    if (!h || !n_calls || (cap_calls > 0 && !ms)) return fail(h, ASM_EINVAL, "asm_profile_read: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (hipStream_t s : {h->pipe.side_stream, h->pipe.pack_stream, h->pipe.acc_stream})
        if (s) HIPCHK(h, hipStreamSynchronize(s));
    const int n = (int)h->prof_mask.size();
    *n_calls = n;
    for (int c = 0; c < n && c < cap_calls; c++)
        for (int q = 0; q < 4; q++) {
            float v = -1.0f;
            if (h->prof_mask[(size_t)c] & (1u << q))
                HIPCHK(h, hipEventElapsedTime(&v, h->prof_ev[(size_t)(8 * c + 2 * q)], h->prof_ev[(size_t)(8 * c + 2 * q + 1)]));
            ms[4 * c + q] = v;
        }
    return ASM_OK;
}
