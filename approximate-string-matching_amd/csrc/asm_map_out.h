// The output side of a file call (asm_map_file.h, asm_map_pairs_file.h; the sorted calls' slabs: asm_sam_sort.h): MapOutput owns the
// file, the copy-out stream, the rotation of three output slots, the writer thread and, under ASM_OUT_BAM, the BGZF record stream.
// MapOutput::put is the one way payload bytes reach the file.  asm_capi.hip includes this file inside its extern "C" block, behind
// asm_bgzf.h and in front of asm_sam_sort.h.
#pragma once

extern "C++" {

/* the file the call writes could not be written: named by the handle's output format */
static int map_out_failed(asm_handle* h, const char* who) {
    return fail(h, ASM_EINVAL, std::string(who) + (h->out_format == ASM_OUT_BAM ? ": writing the BAM file failed" : ": writing the SAM file failed"));
}

/* What one file call (`who`) owns of its output: the file, the copy-out stream, three pinned buffers and three device buffers in
 * rotation with the events between them, the writer thread, the BAM call's record stream (asm_bgzf.h), the count of the writer's jobs
 * and of the bytes they hold.  open() once, put() per unsorted chunk or sorted slab, finish() after the last.
 * The destructor runs on every path, in this order: the writer thread is joined before any pinned buffer is freed; the copy-out
 * stream and the handle's stream are synchronised before events, stream, pinned buffers and pool blocks go back; the file is closed
 * last.  Declare it behind the call's input side (StreamInput), which then goes after it. */
struct MapOutput {
    asm_handle* h;
    const char* who;
    FILE* file = nullptr;
    hipStream_t s_out = nullptr;
    char* pin_out[3] = {nullptr, nullptr, nullptr};
    size_t pin_out_cap[3] = {0, 0, 0};
    char* d_out[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fmt[3] = {nullptr, nullptr, nullptr};    /* d_out[o] holds its bytes */
    hipEvent_t ev_copied[3] = {nullptr, nullptr, nullptr}; /* pin_out[o] holds them */
    std::unique_ptr<asm_host::ChunkWriter> writer;
    std::unique_ptr<BgzfStream> bam; /* ASM_OUT_BAM: the payload is BAM records and leaves through the BGZF record stream */
    int64_t jobs = 0;                /* handed to the writer so far */
    int64_t bytes_out = 0;           /* in those jobs: the file's bytes behind its head */
    size_t head_bytes = 0;           /* the file's head */
    MapOutput(asm_handle* owner, const char* call) : h(owner), who(call) {}
    MapOutput(const MapOutput&) = delete;
    MapOutput& operator=(const MapOutput&) = delete;
    ~MapOutput() {
        writer.reset();
        (void)hipSetDevice(h->device);
        if (s_out) (void)hipStreamSynchronize(s_out);
        (void)hipStreamSynchronize(h->stream);
        for (hipEvent_t ev : {ev_fmt[0], ev_fmt[1], ev_fmt[2], ev_copied[0], ev_copied[1], ev_copied[2]})
            if (ev) (void)hipEventDestroy(ev);
        if (s_out) (void)hipStreamDestroy(s_out);
        for (char* q : pin_out)
            if (q) (void)hipHostFree(q);
        for (char* q : d_out) pool_free(h, q);
        bam.reset();
        if (file) fclose(file);
    }

    /* head: what the file starts with, the SAM header's text or the BAM header in BGZF blocks of its own */
    int open(const char* path, const std::vector<uint8_t>& head) {
        file = fopen(path, "wb");
        if (!file) return fail(h, ASM_EINVAL, std::string(who) + ": cannot write " + path);
        head_bytes = head.size();
        if (!head.empty() && fwrite(head.data(), 1, head.size(), file) != head.size()) return map_out_failed(h, who);
        STREAM_TRY(who, hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
        for (hipEvent_t* ev : {&ev_fmt[0], &ev_fmt[1], &ev_fmt[2], &ev_copied[0], &ev_copied[1], &ev_copied[2]})
            STREAM_TRY(who, hipEventCreateWithFlags(ev, hipEventDisableTiming));
        if (h->out_format == ASM_OUT_BAM) {
            bam.reset(new BgzfStream(h));
            STREAM_TRY(who, bam->open());
        }
        writer.reset(new asm_host::ChunkWriter(file, [this](int o) {
            (void)hipSetDevice(h->device);
            return hipEventSynchronize(ev_copied[o]) == hipSuccess;
        }));
        return ASM_OK;
    }

    /* n payload bytes (SAM text, or BAM records) are about to be produced on the handle's stream: fill(dst), a callable that gives a
     * hipError_t, launches what writes exactly dst[0, n).  SAM: dst is the slot and the n bytes leave as they are.  BAM: the records
     * go behind the stream's carry in a staging block, and what leaves is the whole BGZF blocks framed from it; the slot has room
     * for their stored form. */
    template <class Fill>
    int put(size_t n, Fill fill) {
        Scratch<char> d_stage(h);
        return job(bam ? bam->framed(n) : n, [&](char* slot, size_t* bytes) {
            if (!bam) return fill(slot);
            char* fresh = nullptr;
            hipError_t e = bam->stage(n, d_stage, &fresh);
            if (e == hipSuccess) e = fill(fresh);
            return e == hipSuccess ? bam->frame(d_stage, n, slot, bytes) : e;
        });
    }

    /* after the last put: under BAM what it left of the record stream and the EOF block; then the file complete on disk */
    int finish(double* seconds_write) {
        if (bam)
            if (const int rc = job(bam->tail_bytes(), [&](char* slot, size_t* bytes) { return bam->tail(slot, bytes); })) return rc;
        if (!writer->finish() || fflush(file) != 0) return map_out_failed(h, who);
        *seconds_write = writer->write_seconds();
        return ASM_OK;
    }

private:
    /* One job of the rotation.  The next slot gets room for `room` bytes: the writer is done with the job that used it three jobs
     * ago, so its copy out of d_out is over too.  write(slot, &bytes) enqueues on the handle's stream what fills the slot and may
     * lower bytes from `room` to what it wrote.  Then d_out[o][0, bytes) is complete in the handle's stream order: the copy out
     * starts on the copy-out stream and the write is queued.  The only place that counts bytes_out. */
    template <class Write>
    int job(size_t room, Write write) {
        const int o = (int)(jobs % 3);
        writer->wait_idle(o);
        if (writer->failed()) return map_out_failed(h, who);
        pool_free(h, d_out[o]);
        d_out[o] = nullptr;
        if (pin_out_cap[o] < room) {
            if (pin_out[o]) (void)hipHostFree(pin_out[o]);
            pin_out[o] = nullptr, pin_out_cap[o] = 0;
            const size_t want = room + room / 4 + 4096;
            STREAM_TRY(who, hipHostMalloc((void**)&pin_out[o], want, hipHostMallocDefault));
            pin_out_cap[o] = want;
        }
        STREAM_TRY(who, pool_alloc(h, (void**)&d_out[o], room + 64));
        size_t bytes = room;
        STREAM_TRY(who, write(d_out[o], &bytes));
        STREAM_TRY(who, hipEventRecord(ev_fmt[o], h->stream));
        STREAM_TRY(who, hipStreamWaitEvent(s_out, ev_fmt[o], 0));
        if (bytes) STREAM_TRY(who, hipMemcpyAsync(pin_out[o], d_out[o], bytes, hipMemcpyDeviceToHost, s_out));
        STREAM_TRY(who, hipEventRecord(ev_copied[o], s_out));
        writer->push(o, pin_out[o], bytes);
        jobs++, bytes_out += (int64_t)bytes;
        return ASM_OK;
    }
};

} /* extern "C++" */
