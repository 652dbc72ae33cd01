// The output side that the file calls share (asm_map_file.h: MapFilePipe and the unsorted chunks; asm_sam_sort.h: the sorted slabs):
// the report of a failed write and the rotation of three output slots.  asm_capi.hip includes this file inside its extern "C"
// block, in front of asm_sam_sort.h.
#pragma once

extern "C++" {

/* the file the call writes could not be written: named by the handle's output format */
static int map_out_failed(asm_handle* h, const char* who) {
    return fail(h, ASM_EINVAL, std::string(who) + (h->out_format == ASM_OUT_BAM ? ": writing the BAM file failed" : ": writing the SAM file failed"));
}

/* The output rotation of a file call (Pipe: MapFilePipe, asm_map_file.h), for the unsorted call's chunks and the sorted call's slabs.
 * map_out_slot: the next slot with room for `bytes`; the writer is done with the job that used it three jobs ago, so its copy out
 * of d_out is over too.  map_out_ship: d_out[o][0, bytes) is complete in the handle's stream order; the copy out starts on the
 * copy-out stream and the write is queued. */
template <class Pipe>
static int map_out_slot(asm_handle* h, const char* who, Pipe& pp, asm_host::ChunkWriter& writer, int64_t out_seq, size_t bytes, int* slot) {
    const int o = (int)(out_seq % 3);
    writer.wait_idle(o);
    if (writer.failed()) return map_out_failed(h, who);
    pool_free(h, pp.d_out[o]);
    pp.d_out[o] = nullptr;
    if (pp.pin_out_cap[o] < bytes) {
        if (pp.pin_out[o]) (void)hipHostFree(pp.pin_out[o]);
        pp.pin_out[o] = nullptr, pp.pin_out_cap[o] = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        STREAM_TRY(who, hipHostMalloc((void**)&pp.pin_out[o], want, hipHostMallocDefault));
        pp.pin_out_cap[o] = want;
    }
    STREAM_TRY(who, pool_alloc(h, (void**)&pp.d_out[o], bytes + 64));
    *slot = o;
    return ASM_OK;
}
template <class Pipe>
static int map_out_ship(asm_handle* h, const char* who, Pipe& pp, asm_host::ChunkWriter& writer, int64_t& out_seq, int o, size_t bytes) {
    STREAM_TRY(who, hipEventRecord(pp.ev_fmt[o], h->stream));
    STREAM_TRY(who, hipStreamWaitEvent(pp.s_out, pp.ev_fmt[o], 0));
    if (bytes) STREAM_TRY(who, hipMemcpyAsync(pp.pin_out[o], pp.d_out[o], bytes, hipMemcpyDeviceToHost, pp.s_out));
    STREAM_TRY(who, hipEventRecord(pp.ev_copied[o], pp.s_out));
    writer.push(o, pp.pin_out[o], bytes);
    out_seq++;
    return ASM_OK;
}

} /* extern "C++" */
