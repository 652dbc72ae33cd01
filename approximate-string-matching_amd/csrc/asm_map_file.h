// asm_map_file: a FASTQ file in, a SAM file out, parsed, mapped and formatted on the device (kernels: asm_fastq.h, asm_sam.h and the
// mapper's own; stages: asm_map_host.h; input pipeline: asm_stream.h; reader and writer threads: asm_host.h; design:
// docs/design/mapper.md, "Files: FASTQ in, SAM out").  asm_capi.hip includes this file inside its extern "C" block, behind
// asm_map_host.h.
#pragma once

extern "C++" {

#define MAP_FILE_TRY(call) STREAM_TRY("asm_map_file", call)

/* What one call owns besides its threads: the input side (StreamInput, asm_stream.h) and on top of it the SAM file, the copy-out
 * stream, three pinned output buffers in rotation, the device buffers of the SAM bytes and the events between them.  The destructor
 * waits for the streams and gives everything back, on every path; the threads are declared after it, so they are joined before. */
struct MapFilePipe {
    asm_handle* h;
    StreamInput in;
    FILE* out = nullptr;
    hipStream_t s_out = nullptr;
    char* pin_out[3] = {nullptr, nullptr, nullptr};
    size_t pin_out_cap[3] = {0, 0, 0};
    char* d_out[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fmt[3] = {nullptr, nullptr, nullptr};    /* d_out[o] holds its SAM bytes */
    hipEvent_t ev_copied[3] = {nullptr, nullptr, nullptr}; /* pin_out[o] holds them */
    explicit MapFilePipe(asm_handle* owner, const char* who = "asm_map_file") : h(owner), in(owner, who) {}
    hipError_t open_device(size_t slot_cap) {
        hipError_t e = in.open_device(slot_cap, false, true);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking);
        for (hipEvent_t* ev : {&ev_fmt[0], &ev_fmt[1], &ev_fmt[2], &ev_copied[0], &ev_copied[1], &ev_copied[2]})
            if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        return e;
    }
    ~MapFilePipe() { /* the input side goes after this */
        (void)hipSetDevice(h->device);
        if (in.s_in) (void)hipStreamSynchronize(in.s_in);
        if (s_out) (void)hipStreamSynchronize(s_out);
        (void)hipStreamSynchronize(h->stream);
        for (hipEvent_t ev : {ev_fmt[0], ev_fmt[1], ev_fmt[2], ev_copied[0], ev_copied[1], ev_copied[2]})
            if (ev) (void)hipEventDestroy(ev);
        if (s_out) (void)hipStreamDestroy(s_out);
        for (char* q : pin_out)
            if (q) (void)hipHostFree(q);
        for (char* q : d_out) pool_free(h, q);
        if (out) fclose(out);
    }
};

/* The output side of one device chunk, for both file calls: a's sizes and offsets are there and `total` is their sum.  Takes the
 * next output slot of the rotation (the writer is done with the chunk that used it three chunks ago, so its copy out of d_out is
 * over too), emits the nlines lines into it, starts the copy out on the copy-out stream and queues the write. */
template <bool PAIRED>
static int map_file_hand_over(MapFilePipe& pp, asm_host::ChunkWriter& writer, int64_t& out_seq, SamArgs& a, int64_t nlines,
                              unsigned long long total) {
    asm_handle* h = pp.h;
    const char* who = pp.in.who;
    const int o = (int)(out_seq % 3);
    writer.wait_idle(o);
    if (writer.failed()) return fail(h, ASM_EINVAL, std::string(who) + ": writing the SAM file failed");
    pool_free(h, pp.d_out[o]);
    pp.d_out[o] = nullptr;
    if (pp.pin_out_cap[o] < total) {
        if (pp.pin_out[o]) (void)hipHostFree(pp.pin_out[o]);
        pp.pin_out[o] = nullptr, pp.pin_out_cap[o] = 0;
        const size_t want = (size_t)total + (size_t)total / 4 + 4096;
        STREAM_TRY(who, hipHostMalloc((void**)&pp.pin_out[o], want, hipHostMallocDefault));
        pp.pin_out_cap[o] = want;
    }
    STREAM_TRY(who, pool_alloc(h, (void**)&pp.d_out[o], (size_t)total + 64));
    a.out = pp.d_out[o];
    hipLaunchKernelGGL(sam_emit_kernel<PAIRED>, dim3(map_grid((uint64_t)nlines * 64, h)), dim3(256), 0, h->stream, a);
    STREAM_TRY(who, hipGetLastError());
    STREAM_TRY(who, hipEventRecord(pp.ev_fmt[o], h->stream));
    STREAM_TRY(who, hipStreamWaitEvent(pp.s_out, pp.ev_fmt[o], 0));
    if (total) STREAM_TRY(who, hipMemcpyAsync(pp.pin_out[o], pp.d_out[o], (size_t)total, hipMemcpyDeviceToHost, pp.s_out));
    STREAM_TRY(who, hipEventRecord(pp.ev_copied[o], pp.s_out));
    writer.push(o, pp.pin_out[o], (size_t)total);
    out_seq++;
    return ASM_OK;
}

struct MapFileJob { /* what every chunk of a call shares */
    asm_handle* h;
    const asm_index* ix;
    const asm_map_params* p;
    int max_hits, strata;
    const char* d_names;
    const uint32_t* d_name_off;
    MapFilePipe* pipe;
    asm_host::ChunkWriter* writer;
    asm_map_file_stats st = {};
    int64_t out_seq = 0; /* device chunks handed to the writer so far */
};

/* Records [r0, r0 + rn) of the file chunk whose bytes are d_raw and whose newline positions are d_nl: one device chunk, from the
 * record kernel to the writer's queue.  first_record: the file's records before r0 (for the message of a malformed one). */
static int map_file_chunk(MapFileJob& j, const char* d_raw, const uint32_t* d_nl, int64_t r0, int64_t rn, int64_t first_record) {
    asm_handle* h = j.h;
    const asm_index* ix = j.ix;
    const asm_map_params* p = j.p;
    const size_t cnt = (size_t)rn + 1;
    MapTmp tmp(h);
    /* the records, and which of them go to the mapper */
    Scratch<SamRec> d_recs(h);
    Scratch<uint32_t> d_send(h), d_mlen(h), d_rd(h), d_mo(h);
    Scratch<int32_t> d_rec_read(h);
    Scratch<FastqCounts> d_counts(h);
    Scratch<unsigned long long> d_start(h);
    MAP_FILE_TRY(d_recs.alloc(sizeof(SamRec) * (size_t)rn));
    for (Scratch<uint32_t>* x : {&d_send, &d_mlen, &d_rd, &d_mo}) MAP_FILE_TRY(x->alloc(sizeof(uint32_t) * cnt));
    MAP_FILE_TRY(d_rec_read.alloc(sizeof(int32_t) * (size_t)rn));
    MAP_FILE_TRY(d_counts.alloc(sizeof(FastqCounts)));
    MAP_FILE_TRY(hipMemsetAsync(&d_counts.p->bad_min, 0xff, sizeof(uint32_t), h->stream));
    MAP_FILE_TRY(hipMemsetAsync(&d_counts.p->too_long, 0, sizeof(uint32_t), h->stream));
    hipLaunchKernelGGL(fastq_record_kernel, dim3(grid_for(rn + 1)), dim3(ASM_BLOCK), 0, h->stream, d_raw, d_nl, (long)r0, (long)rn,
                       (uint32_t)ASM_MAP_MAX_READ, d_recs.p, d_send.p, d_mlen.p, d_counts.p);
    MAP_FILE_TRY(hipGetLastError());
    MAP_FILE_TRY(map_exclusive_sum(h, tmp, d_send.p, d_rd.p, (int64_t)cnt));
    MAP_FILE_TRY(map_exclusive_sum(h, tmp, d_mlen.p, d_mo.p, (int64_t)cnt));
    uint32_t tot[2] = {0, 0};
    FastqCounts counts = {FASTQ_NO_RECORD, 0};
    MAP_FILE_TRY(hipMemcpyAsync(&tot[0], d_rd.p + rn, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    MAP_FILE_TRY(hipMemcpyAsync(&tot[1], d_mo.p + rn, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    MAP_FILE_TRY(hipMemcpyAsync(&counts, d_counts.p, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
    MAP_FILE_TRY(hipStreamSynchronize(h->stream));
    if (counts.bad_min != FASTQ_NO_RECORD)
        return fail(h, ASM_EINVAL, "asm_map_file: record " + std::to_string(first_record + counts.bad_min + 1) +
                                       " is malformed (line 1 of a record starts with '@', line 3 with '+')");
    const int64_t ns = tot[0]; /* library reads */
    /* compact and gather: the reads in HBM, numbered in file order */
    MapFront f(h);
    MAP_FILE_TRY(f.d_reads.alloc((size_t)tot[1] + 16));
    MAP_FILE_TRY(f.d_roff.alloc(sizeof(uint32_t) * ((size_t)ns + 1)));
    MAP_FILE_TRY(d_start.alloc(sizeof(unsigned long long) * ((size_t)ns + 1)));
    hipLaunchKernelGGL(fastq_compact_kernel, dim3(grid_for(rn + 1)), dim3(ASM_BLOCK), 0, h->stream, (const SamRec*)d_recs.p,
                       (const uint32_t*)d_send.p, (const uint32_t*)d_rd.p, (const uint32_t*)d_mo.p, (long)rn, d_rec_read.p, f.d_roff.p,
                       d_start.p);
    MAP_FILE_TRY(hipGetLastError());
    /* map: the library's stages, fed from device memory; the records, ops and nops stay there */
    Scratch<unsigned long long> d_keys(h);
    MapAllItems ai(h);
    MapFinish fin(h);
    std::vector<uint32_t> n_hits;
    int64_t nlines = rn;
    if (ns > 0) {
        hipLaunchKernelGGL(seq_gather_kernel, dim3((unsigned)std::min<int64_t>((ns + 3) / 4, 256 * 16)), dim3(ASM_BLOCK), 0, h->stream,
                           d_raw, (const unsigned long long*)d_start.p, (const uint32_t*)f.d_roff.p, (long)ns, f.d_reads.p);
        MAP_FILE_TRY(hipGetLastError());
        f.roff.resize((size_t)ns + 1);
        f.bytes = tot[1];
        MAP_FILE_TRY(hipMemcpyAsync(f.roff.data(), f.d_roff.p, sizeof(uint32_t) * ((size_t)ns + 1), hipMemcpyDeviceToHost, h->stream));
        MAP_FILE_TRY(hipStreamSynchronize(h->stream));
        if (const int rc = map_front_seed(h, ix, ns, p, f)) return rc;
        if (j.max_hits == 0) {
            if (const int rc = map_best_keys(h, ix, ns, p, f, d_keys)) return rc;
            if (const int rc = map_finish_launch(h, ix, p, f, ns, d_keys.p, nullptr, nullptr, f.bytes + (size_t)ns, SAM_CIGAR_CAP, fin))
                return rc;
        } else {
            n_hits.resize((size_t)ns);
            if (const int rc = map_all_items(h, ix, ns, p, j.strata, j.max_hits, f, n_hits.data(), ai, "asm_map_file")) return rc;
            if (const int rc = map_finish_launch(h, ix, p, f, ai.ni, ai.d_ikey.p, ai.d_iread.p, ai.d_idirs.p, ai.dwords, SAM_CIGAR_CAP, fin))
                return rc;
            nlines = (rn - ns) + ai.ni; /* the item list is in read-then-rank order, which is SAM order */
        }
        if (const int rc = map_finish_device(h, ix, p, f, fin)) return rc;
    }
    if (nlines > (int64_t)INT32_MAX) return fail(h, ASM_EUNSUPPORTED, "asm_map_file: more than 2^31 - 1 SAM lines in a chunk");
    /* format: the line list, every line's size, its offset, the bytes */
    Scratch<uint32_t> d_lcnt(h), d_lbase(h), d_lrec(h), d_litem(h);
    Scratch<unsigned long long> d_size(h), d_off(h), d_nmapped(h);
    MAP_FILE_TRY(d_lcnt.alloc(sizeof(uint32_t) * cnt));
    MAP_FILE_TRY(d_lbase.alloc(sizeof(uint32_t) * cnt));
    MAP_FILE_TRY(d_lrec.alloc(sizeof(uint32_t) * (size_t)nlines));
    MAP_FILE_TRY(d_litem.alloc(sizeof(uint32_t) * (size_t)nlines));
    MAP_FILE_TRY(d_size.alloc(sizeof(unsigned long long) * ((size_t)nlines + 1)));
    MAP_FILE_TRY(d_off.alloc(sizeof(unsigned long long) * ((size_t)nlines + 1)));
    MAP_FILE_TRY(d_nmapped.alloc(sizeof(unsigned long long)));
    MAP_FILE_TRY(hipMemsetAsync(d_nmapped.p, 0, sizeof(unsigned long long), h->stream));
    SamArgs a = {};
    a.raw = d_raw, a.recs = d_recs.p, a.rec_read = d_rec_read.p, a.nrec = (long)rn, a.nlines = (long)nlines;
    a.line_rec = d_lrec.p, a.line_item = d_litem.p, a.hits = fin.d_hits.p, a.ops = fin.d_ops.p, a.nops = fin.d_nops.p;
    a.ibase = (j.max_hits > 0 && ns > 0) ? ai.d_ibase.p : nullptr, a.n_hits = ai.d_nh.p;
    a.names = j.d_names, a.name_off = j.d_name_off, a.line_cnt = d_lcnt.p, a.line_base = d_lbase.p, a.size = d_size.p, a.off = d_off.p;
    a.n_mapped = d_nmapped.p;
    hipLaunchKernelGGL(sam_line_count_kernel, dim3(grid_for(rn + 1)), dim3(ASM_BLOCK), 0, h->stream, a);
    MAP_FILE_TRY(hipGetLastError());
    MAP_FILE_TRY(map_exclusive_sum(h, tmp, d_lcnt.p, d_lbase.p, (int64_t)cnt));
    hipLaunchKernelGGL(sam_line_fill_kernel, dim3(grid_for(rn)), dim3(ASM_BLOCK), 0, h->stream, a, d_lrec.p, d_litem.p);
    hipLaunchKernelGGL(sam_size_kernel<false>, dim3(grid_for(nlines + 1)), dim3(ASM_BLOCK), 0, h->stream, a);
    MAP_FILE_TRY(hipGetLastError());
    MAP_FILE_TRY(map_exclusive_sum(h, tmp, d_size.p, d_off.p, nlines + 1));
    unsigned long long total = 0, n_mapped = 0;
    MAP_FILE_TRY(hipMemcpyAsync(&total, d_off.p + nlines, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    MAP_FILE_TRY(hipMemcpyAsync(&n_mapped, d_nmapped.p, sizeof(n_mapped), hipMemcpyDeviceToHost, h->stream));
    MAP_FILE_TRY(hipStreamSynchronize(h->stream));
    if (const int rc = map_file_hand_over<false>(*j.pipe, *j.writer, j.out_seq, a, nlines, total)) return rc;
    j.st.reads += rn, j.st.mapped += (int64_t)n_mapped, j.st.too_long += counts.too_long, j.st.records += nlines;
    j.st.chunks++, j.st.bytes_out += (int64_t)total;
    return ASM_OK;
}

/* One file chunk (nrec whole records in d_raw[0, nbytes)): the newline index, then its device chunks of at most map_chunk records */
static int map_file_process(MapFileJob& j, const char* d_raw, size_t nbytes, int64_t nrec, int64_t first_record) {
    asm_handle* h = j.h;
    Scratch<uint32_t> d_nl(h);
    MapTmp tmp(h);
    MAP_FILE_TRY(d_nl.alloc(sizeof(uint32_t) * (4 * (size_t)nrec + 2)));
    MAP_FILE_TRY(newline_index(h, tmp, d_raw, nbytes, (long)(4 * nrec), d_nl.p));
    /* the run key of asm_map_reads_all holds the read in its top 31 bits */
    return map_chunks(nrec, std::min<int64_t>(h->map_chunk, (int64_t)1 << 30), [&](int64_t r0, int64_t rn) {
        return map_file_chunk(j, d_raw, d_nl.p, r0, rn, first_record + r0);
    });
}

/* the RNAME table on the device: the names back to back and their n_seqs + 1 offsets */
static int map_file_names(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* who, Scratch<char>& d_names,
                          Scratch<uint32_t>& d_name_off) {
    std::string names;
    std::vector<uint32_t> name_off(1, 0u);
    for (int32_t r = 0; r < ix->n_seqs; r++) {
        if (!seq_names[r]) return fail(h, ASM_EINVAL, std::string(who) + ": seq_names[" + std::to_string(r) + "] is NULL");
        names += seq_names[r];
        name_off.push_back((uint32_t)names.size());
    }
    STREAM_TRY(who, d_names.alloc(names.size() + 16));
    STREAM_TRY(who, d_name_off.alloc(sizeof(uint32_t) * name_off.size()));
    STREAM_TRY(who, hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, h->stream));
    STREAM_TRY(who, hipMemcpyAsync(d_name_off.p, name_off.data(), sizeof(uint32_t) * name_off.size(), hipMemcpyHostToDevice, h->stream));
    STREAM_TRY(who, hipStreamSynchronize(h->stream));
    return ASM_OK;
}

static int map_file_run(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq_path, const char* sam_path,
                        const char* header, const asm_map_params* p, int max_hits, int strata, size_t chunk, asm_map_file_stats* stats) {
    const auto t_begin = std::chrono::steady_clock::now();
    MapFilePipe pipe(h);
    StreamInput& in = pipe.in;
    size_t file_bytes = 0;
    if (const int rc = in.open_file(fastq_path, &file_bytes)) return rc;
    char first = 0;
    if (file_bytes && pread(in.fd, &first, 1, 0) != 1) return fail(h, ASM_EINVAL, std::string("asm_map_file: cannot read ") + fastq_path);
    if (first == '>') return fail(h, ASM_EUNSUPPORTED, "asm_map_file: FASTA reads are not supported (the file starts with '>')");
    pipe.out = fopen(sam_path, "wb");
    if (!pipe.out) return fail(h, ASM_EINVAL, std::string("asm_map_file: cannot write ") + sam_path);
    if (header && *header && fwrite(header, 1, strlen(header), pipe.out) != strlen(header))
        return fail(h, ASM_EINVAL, "asm_map_file: writing the SAM file failed");
    Scratch<char> d_names(h);
    Scratch<uint32_t> d_name_off(h);
    if (const int rc = map_file_names(h, ix, seq_names, "asm_map_file", d_names, d_name_off)) return rc;
    /* chunks ramp up from an eighth, so that the device starts after an eighth of a chunk has been read */
    const size_t slot_cap = chunk + chunk / 4 + 4096, first_chunk = chunk >= ((size_t)8 << 20) ? chunk / 8 : chunk;
    MAP_FILE_TRY(pipe.open_device(slot_cap));
    in.own_pin = true;
    for (char*& q : in.pin) MAP_FILE_TRY(hipHostMalloc((void**)&q, slot_cap + 64, hipHostMallocDefault));
    asm_host::ChunkReader<asm_host::FastqFill> rd(
        chunk, first_chunk, in.wait_shipped(), in.fd, file_bytes, chunk,
        [&](int q, size_t cap, size_t keep) { /* a record longer than the buffer: a larger pinned one (no copy reads the old one now) */
            (void)hipSetDevice(h->device);
            char* bigger = nullptr;
            if (hipHostMalloc((void**)&bigger, cap + 64, hipHostMallocDefault) != hipSuccess) return false;
            if (keep) memcpy(bigger, in.pin[q], keep);
            (void)hipHostFree(in.pin[q]);
            in.pin[q] = bigger;
            rd.slot[q].buf = bigger, rd.slot[q].cap = cap;
            return true;
        });
    for (int q = 0; q < 3; q++) rd.slot[q].buf = in.pin[q], rd.slot[q].cap = slot_cap;
    asm_host::ChunkWriter writer(pipe.out, [&](int o) {
        (void)hipSetDevice(h->device);
        return hipEventSynchronize(pipe.ev_copied[o]) == hipSuccess;
    });
    MapFileJob j = {h, ix, p, max_hits, strata, d_names.p, d_name_off.p, &pipe, &writer};
    rd.start();
    const int rc = in.run(
        rd, std::string("asm_map_file: reading ") + fastq_path + " failed",
        [&](const asm_host::ChunkSlot& s, int64_t records_seen) {
            if (s.extra_lines)
                return fail(h, ASM_EINVAL, "asm_map_file: record " + std::to_string(records_seen + s.units + 1) +
                                               " is truncated (the file's line count is not a multiple of 4)");
            if (s.bytes >= 0xfffffff0ull) return fail(h, ASM_EUNSUPPORTED, "asm_map_file: a chunk of 4 GiB or more; lower chunk_bytes");
            j.st.bytes_in += (int64_t)s.bytes;
            return ASM_OK;
        },
        [&](int q, size_t bytes, int64_t records, int64_t first_record) {
            return map_file_process(j, in.d_raw[q], bytes, records, first_record);
        });
    if (rc) return rc;
    rd.stop();
    if (!writer.finish() || fflush(pipe.out) != 0) return fail(h, ASM_EINVAL, "asm_map_file: writing the SAM file failed");
    j.st.seconds_read = rd.read_seconds(), j.st.seconds_write = writer.write_seconds();
    j.st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = j.st;
    return ASM_OK;
}

} /* extern "C++" */

int asm_map_file(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq_path, const char* sam_path,
                 const char* header, const asm_map_params* p, int max_hits, int strata, int64_t chunk_bytes, asm_map_file_stats* stats) {
    if (!p || !ix || !seq_names || !fastq_path || !sam_path) return fail(h, ASM_EINVAL, "asm_map_file: bad arguments");
    if (max_hits < 0 || max_hits > ASM_MAP_MAX_HITS) return fail(h, ASM_EINVAL, "asm_map_file: max_hits must be in [0, 256]");
    if (chunk_bytes < 0) return fail(h, ASM_EINVAL, "asm_map_file: chunk_bytes must be >= 0");
    if (const int rc = map_check_args(h, ix, "asm_map_file", "read",
                                      {0, p, {nullptr, nullptr}, nullptr, max_hits ? "max_hits" : nullptr, strata, ASM_MAP_MAX_ERRORS,
                                       max_hits, {nullptr, 0, nullptr}}))
        return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t chunk = chunk_bytes == 0 ? (size_t)16 << 20 : (size_t)std::min<int64_t>(chunk_bytes, (int64_t)1 << 30);
    return map_file_run(h, ix, seq_names, fastq_path, sam_path, header, p, max_hits, strata, chunk, stats);
}

size_t asm_fastq_cut(const char* buf, size_t nbytes, int64_t* records) {
    if (!buf) nbytes = 0;
    return asm_host::fastq_cut(buf, nbytes, records);
}
