// Device side of the streamed-file calls (asm_stream_seq_file, asm_map_file, asm_map_pairs_file): their error path and the input
// pipeline — reader thread (asm_host.h) -> pinned slots -> copy-in stream -> two device buffers -> the caller's processing on the
// handle's stream.  ("Scalars back, one wait", hipcub's scratch and scans and the newline index of a chunk of text in HBM: asm_batch.h.)
// asm_capi.hip includes this file inside its extern "C" block.
#pragma once

extern "C++" {

/* the one error path of both calls: `who` is the call's name */
#define STREAM_TRY(who, call)                                                                    \
    do {                                                                                         \
        hipError_t _e = (call);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(h, _e == hipErrorOutOfMemory ? ASM_ENOMEM : ASM_ENODEVICE,               \
                        std::string(who) + ": " + #call + ": " + hipGetErrorString(_e));         \
    } while (0)

/* The input side of one streamed call: the file, the copy-in stream, three pinned slots in rotation (the reader thread fills them),
 * two device buffers that the handle's stream reads, and the events between them.  The destructor waits for the streams and gives
 * everything back, on every path; declare the reader after it, so that its thread is joined before.
 * The two callers differ in three ways, which open_device and the pinned slots take as they are:
 *   pinned slots  borrowed (asm_stream_seq_file keeps them on the handle between calls) or owned (asm_map_file: per call, growing)
 *   fixed_raw     d_raw[q] allocated once for a whole slot, or on demand with the chunk that needs it
 *   gate_each     the copy-in stream waits for the handle's stream once, before the first copy (d_raw[q] is then reused only after
 *                 this thread has waited for the parse of the chunk before), or before every copy */
struct StreamInput {
    asm_handle* h;
    const char* who;
    int fd = -1;
    hipStream_t s_in = nullptr;
    char* pin[3] = {nullptr, nullptr, nullptr};
    bool own_pin = false;
    char* d_raw[2] = {nullptr, nullptr};
    size_t d_raw_cap[2] = {0, 0};
    size_t slot_cap = 0;
    bool gate_each = false;
    hipEvent_t ev_shipped[3] = {nullptr, nullptr, nullptr}; /* the copy out of pinned slot q is over */
    hipEvent_t ev_h2d[2] = {nullptr, nullptr};              /* d_raw[q] holds its chunk */
    hipEvent_t ev_gate = nullptr;                           /* everything enqueued on the handle's stream so far */
    StreamInput(asm_handle* owner, const char* call) : h(owner), who(call) {}
    StreamInput(const StreamInput&) = delete;
    StreamInput& operator=(const StreamInput&) = delete;
    ~StreamInput() {
        (void)hipSetDevice(h->device);
        if (s_in) (void)hipStreamSynchronize(s_in);
        (void)hipStreamSynchronize(h->stream);
        for (hipEvent_t ev : {ev_shipped[0], ev_shipped[1], ev_shipped[2], ev_h2d[0], ev_h2d[1], ev_gate})
            if (ev) (void)hipEventDestroy(ev);
        if (s_in) (void)hipStreamDestroy(s_in);
        for (char* q : pin)
            if (q && own_pin) (void)hipHostFree(q);
        for (char* q : d_raw) pool_free(h, q);
        if (fd >= 0) close(fd);
    }
    int open_file(const char* path, size_t* file_bytes) {
        fd = open(path, O_RDONLY);
        if (fd < 0) return fail(h, ASM_EINVAL, std::string(who) + ": cannot open " + path); /* benchmark_utils.h:350 */
        struct stat st;
        if (fstat(fd, &st) != 0) return fail(h, ASM_EINVAL, std::string(who) + ": fstat failed");
        *file_bytes = (size_t)st.st_size;
        return ASM_OK;
    }
    hipError_t gate() { /* the copy-in stream waits for what the handle's stream holds now */
        hipError_t e = hipEventRecord(ev_gate, h->stream);
        return e != hipSuccess ? e : hipStreamWaitEvent(s_in, ev_gate, 0);
    }
    hipError_t reserve_raw(int q, size_t bytes) {
        if (d_raw_cap[q] >= bytes + 64) return hipSuccess;
        pool_free(h, d_raw[q]);
        d_raw[q] = nullptr, d_raw_cap[q] = 0;
        const size_t want = std::max(bytes + bytes / 4, slot_cap) + 64;
        const hipError_t e = pool_alloc(h, (void**)&d_raw[q], want);
        if (e == hipSuccess) d_raw_cap[q] = want;
        return e;
    }
    hipError_t open_device(size_t slot_bytes, bool fixed_raw, bool gate_every_copy) {
        slot_cap = slot_bytes, gate_each = gate_every_copy;
        hipError_t e = hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking);
        for (hipEvent_t* ev : {&ev_shipped[0], &ev_shipped[1], &ev_shipped[2], &ev_h2d[0], &ev_h2d[1], &ev_gate})
            if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        for (int q = 0; q < 2 && fixed_raw; q++)
            if (e == hipSuccess) e = reserve_raw(q, 0);
        /* d_raw comes from the pool, whose blocks are recycled in the order of the HANDLE's stream: kernels still queued there may
         * read the block's previous life.  The copy stream is non-blocking and would not wait for them by itself. */
        if (e == hipSuccess && !gate_each) e = gate();
        return e;
    }
    /* SHIP chunk c: pinned slot c % 3 -> d_raw[c & 1] on the copy-in stream */
    int ship(int c, const asm_host::ChunkSlot& s) {
        const int q = c & 1;
        STREAM_TRY(who, reserve_raw(q, s.bytes));
        /* d_raw[q] held chunk c - 2, whose kernels are all enqueued on the handle's stream (and a block fresh from the pool may
         * still be read by work queued there): the copy waits for them */
        if (gate_each) STREAM_TRY(who, gate());
        STREAM_TRY(who, hipMemcpyAsync(d_raw[q], s.buf, s.bytes, hipMemcpyHostToDevice, s_in));
        STREAM_TRY(who, hipEventRecord(ev_shipped[c % 3], s_in));
        STREAM_TRY(who, hipEventRecord(ev_h2d[q], s_in));
        return ASM_OK;
    }
    /* For a reader's policy, on the reader's thread, when the pinned slots are owned: a unit longer than slot q gets a larger pinned
     * one, with the first `keep` bytes of the old one.  No copy reads the old one now: the reader has waited for the one out of it. */
    bool grow_pin(asm_host::ChunkSlot* slots, int q, size_t cap, size_t keep) {
        (void)hipSetDevice(h->device);
        char* bigger = nullptr;
        if (hipHostMalloc((void**)&bigger, cap + 64, hipHostMallocDefault) != hipSuccess) return false;
        if (keep) memcpy(bigger, pin[q], keep);
        (void)hipHostFree(pin[q]);
        pin[q] = bigger;
        slots[q].buf = bigger, slots[q].cap = cap;
        return true;
    }
    std::function<void(int)> wait_shipped() { /* for the reader: the copy out of slot q is over */
        return [this](int q) {
            (void)hipSetDevice(h->device);
            (void)hipEventSynchronize(ev_shipped[q]);
        };
    }
    /* The caller's thread.  Two stages per iteration, one chunk apart: SHIP chunk c and only then PROCESS chunk c - 1.  Processing
     * blocks this thread (the parser's totals), so with the stages the other way round the transfer of the next chunk could not
     * start before the current one was parsed, and the copy engine idled through every parse.
     * accept(slot, first_unit) sees every chunk before it is shipped; process(q, bytes, units, first_unit) runs behind the copy into
     * d_raw[q], for every chunk that holds a unit; first_unit: the file's units before the chunk.  read_failed: the reader's message.
     * hold_slots: a chunk's pinned slot goes back to the reader after the chunk has been processed instead of after its copy has been
     * started, for a process() that reads the slot (two slots are then held while the reader fills the third). */
    template <class Reader, class Accept, class Process>
    int run(Reader& rd, const std::string& read_failed, Accept accept, Process process, bool hold_slots = false) {
        struct {
            bool valid = false;
            size_t bytes = 0;
            int64_t units = 0, first = 0;
        } pend[2];
        auto flush = [&](int q) -> int {
            if (!pend[q].valid) return ASM_OK;
            pend[q].valid = false;
            if (pend[q].units <= 0) return ASM_OK;
            STREAM_TRY(who, hipStreamWaitEvent(h->stream, ev_h2d[q], 0));
            return process(q, pend[q].bytes, pend[q].units, pend[q].first);
        };
        int64_t seen = 0;
        bool last = false;
        for (int c = 0; !last; c++) {
            asm_host::ChunkSlot* s = rd.wait_ready(c);
            if (!s) return fail(h, ASM_EINVAL, read_failed);
            const int q = c & 1;
            last = s->last;
            if (const int rc = accept(*s, seen)) return rc;
            if (s->units > 0)
                if (const int rc = ship(c, *s)) return rc;
            pend[q].valid = true, pend[q].bytes = s->bytes, pend[q].units = s->units, pend[q].first = seen;
            seen += s->units;
            if (!hold_slots) rd.consumed(c, s->units > 0); /* the reader may refill the slot once ev_shipped has fired */
            if (const int rc = flush(q ^ 1)) return rc;
            if (hold_slots && c > 0) rd.consumed(c - 1, true);
        }
        for (int q = 0; q < 2; q++) /* the last chunk shipped (only one of the two is pending) */
            if (const int rc = flush(q)) return rc;
        return ASM_OK;
    }
};

} /* extern "C++" */
