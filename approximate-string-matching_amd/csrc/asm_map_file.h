// asm_map_file: a FASTQ file in, a SAM file out, parsed, mapped and formatted on the device (kernels: asm_fastq.h, asm_sam.h and the
// mapper's own; stages: asm_map_host.h; input pipeline: asm_stream.h; reader and writer threads: asm_host.h; design:
// docs/design/mapper.md, "Files: FASTQ in, SAM out"; output side: MapOutput of asm_map_out.h).  First what it shares with
// asm_map_pairs_file.h: the session of one call (MapFileSession), the gather stage and the format tail of a device chunk
// (map_file_gather, map_file_format<PAIRED>); then asm_map_file's own chunk function and entry point.  asm_capi.hip includes this
// file inside its extern "C" block, behind asm_sam_sort.h.
#pragma once

extern "C++" {

/* One file call, asm_map_file or asm_map_pairs_file (`who`), above its input side (StreamInput, asm_stream.h) and its output side
 * (MapOutput, asm_map_out.h): everything the two calls set up, run and tear down in the same way.  open() probes the input files for
 * FASTA, opens the output with the header, puts the RNAME table on the device and sizes and pins the input slots; grow() is the
 * reader's way to a larger pinned slot; run() drives the input pipeline; finish() completes the output and fills the fields the two
 * stats structs share.  The call itself keeps what differs: its files, its reader policy, what it accepts and how a chunk is
 * processed.  Declare the reader after the session, so that its thread is joined first.  Members go in reverse order of their
 * declaration: what the sorted call holds, then the output side (its writer thread first), then the input side; the destructor
 * waits for the copy-in stream in front of them all. */
struct MapFileSession {
    asm_handle* h;
    const char* who;
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    StreamInput in;
    MapOutput out;
    Scratch<char> d_names; /* the RNAME table: the names back to back and their n_seqs + 1 offsets */
    Scratch<uint32_t> d_name_off;
    /* chunks ramp up from an eighth, so that the device starts after an eighth of a chunk has been read */
    const size_t chunk, slot_cap = chunk + chunk / 4 + 4096, first_chunk = chunk >= ((size_t)8 << 20) ? chunk / 8 : chunk;
    asm_host::ChunkSlot* slots = nullptr; /* the reader's, from run() on */
    struct {
        int64_t chunks, bytes_in, records;
        double seconds_read;
    } st = {};
    std::function<size_t(const asm_host::ChunkSlot&)> text_bytes; /* set: a chunk's share of bytes_in is not the bytes it ships (BGZF) */
    std::unique_ptr<SamSortHold> sort; /* the sorted calls: the formatted chunks stay on the device until finish() (asm_sam_sort.h) */
    std::vector<uint32_t> ref_len;     /* a sorted BAM call that writes an index (asm_bai.h): the sequences' lengths, and its path */
    std::string bai_path;
    MapFileSession(asm_handle* owner, const char* call, size_t chunk_bytes)
        : h(owner), who(call), in(owner, call), out(owner, call), d_names(owner), d_name_off(owner), chunk(chunk_bytes) {}
    ~MapFileSession() {
        (void)hipSetDevice(h->device);
        if (in.s_in) (void)hipStreamSynchronize(in.s_in);
    }

    int bad(const std::string& text, int code = ASM_EINVAL) { return fail(h, code, std::string(who) + ": " + text); }

    /* fds, file_bytes, paths: the n_files input files, open */
    int open(const asm_index* ix, const char* const* seq_names, int n_files, const int* fds, const size_t* file_bytes,
             const char* const* paths, const char* sam_path, const char* header) {
        for (int f = 0; f < n_files; f++) {
            char first = 0;
            if (file_bytes[f] && pread(fds[f], &first, 1, 0) != 1) return bad(std::string("cannot read ") + paths[f]);
            if (first == '>')
                return bad("FASTA reads are not supported (" + (n_files > 1 ? "file " + std::to_string(f + 1) : std::string("the file")) +
                               " starts with '>')",
                           ASM_EUNSUPPORTED);
        }
        std::string names;
        std::vector<uint32_t> name_off(1, 0u);
        for (int32_t r = 0; r < ix->n_seqs; r++) {
            if (!seq_names[r]) return bad("seq_names[" + std::to_string(r) + "] is NULL");
            names += seq_names[r];
            name_off.push_back((uint32_t)names.size());
        }
        std::vector<uint8_t> head; /* what the file starts with: the header as it is, or the BAM header in BGZF blocks of its own */
        if (h->out_format == ASM_OUT_BAM) {
            const size_t l_text = header ? strlen(header) : 0;
            if (l_text > 0x7fffffffull) return bad("a header of 2 GiB or more cannot be a BAM header", ASM_EUNSUPPORTED);
            std::vector<uint32_t> lengths;
            for (int32_t r = 0; r < ix->n_seqs; r++) lengths.push_back((uint32_t)asm_index_seq_len(ix, r));
            const std::vector<uint8_t> text = bam_header_bytes(header, l_text, seq_names, lengths.data(), lengths.size());
            bgzf_compress_host(text.data(), text.size(), 0, h->bgzf_level, head, nullptr);
        } else if (header) {
            head.assign(header, header + strlen(header));
        }
        if (sort && sort->index) {
            for (int32_t r = 0; r < ix->n_seqs; r++) ref_len.push_back((uint32_t)asm_index_seq_len(ix, r));
            bai_path = std::string(sam_path) + ".bai";
        }
        if (const int rc = out.open(sam_path, head)) return rc;
        STREAM_TRY(who, d_names.alloc(names.size() + 16));
        STREAM_TRY(who, d_name_off.alloc(sizeof(uint32_t) * name_off.size()));
        STREAM_TRY(who, hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, h->stream));
        STREAM_TRY(who, hipMemcpyAsync(d_name_off.p, name_off.data(), sizeof(uint32_t) * name_off.size(), hipMemcpyHostToDevice, h->stream));
        STREAM_TRY(who, hipStreamSynchronize(h->stream));
        STREAM_TRY(who, in.open_device(slot_cap, false, true));
        in.own_pin = true;
        for (char*& q : in.pin) STREAM_TRY(who, hipHostMalloc((void**)&q, slot_cap + 64, hipHostMallocDefault));
        return ASM_OK;
    }

    /* For the reader's policy: a record (or pair) longer than slot q gets a larger pinned one (StreamInput::grow_pin) */
    std::function<bool(int, size_t, size_t)> grow() {
        return [this](int q, size_t cap, size_t keep) { return in.grow_pin(slots, q, cap, keep); };
    }

    /* The reader (built on first_chunk, chunk and grow()) through the input pipeline, from its start to its stop: accept sees every
     * chunk first, then the size check and the byte count that both calls share; process is StreamInput::run's. */
    template <class Reader, class Accept, class Process>
    int run(Reader& rd, const std::string& read_failed, Accept accept, Process process) {
        slots = rd.slot;
        for (int q = 0; q < 3; q++) slots[q].buf = in.pin[q], slots[q].cap = slot_cap;
        rd.start();
        const int rc = in.run(
            rd, read_failed,
            [&](const asm_host::ChunkSlot& s, int64_t seen) {
                if (const int ra = accept(s, seen)) return ra;
                if (s.bytes >= 0xfffffff0ull) return bad("a chunk of 4 GiB or more; lower chunk_bytes", ASM_EUNSUPPORTED);
                st.bytes_in += (int64_t)(text_bytes ? text_bytes(s) : s.bytes);
                return (int)ASM_OK;
            },
            process);
        if (rc) return rc;
        rd.stop();
        st.seconds_read = rd.read_seconds();
        return ASM_OK;
    }

    /* after run() and the call's own last checks: the output file complete (a sorted call writes all of it here, in slabs of at most
     * a chunk), and the shared fields of the call's stats.  bytes_out is what the output's jobs shipped; for sorted SAM that is the
     * slabs' bytes, which add up to the chunks' totals. */
    template <class Stats>
    int finish(Stats& stats) {
        if (sort)
            if (const int rc = sort->flush(out, chunk)) return rc;
        if (const int rc = out.finish(&stats.seconds_write)) return rc;
        if (sort && sort->index) /* the BAM file is complete: its index, from what the sort left on the device */
            if (const int rc = bai_index_device(*sort, out.head_bytes, ref_len, bai_path)) return rc;
        stats.chunks = st.chunks, stats.bytes_in = st.bytes_in, stats.bytes_out = out.bytes_out, stats.records = st.records;
        stats.seconds_read = st.seconds_read;
        stats.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        return ASM_OK;
    }
};

struct MapFileJob { /* what every chunk of a file call shares; each call derives its own with its parameters and stats */
    MapFileSession& ss;
    const asm_index* ix;
    const asm_map_params* p;
};

/* the report of a chunk's smallest malformed record (1-based in its file); file: 1 or 2, 0 for the call that reads one */
static int map_file_bad_record(MapFileSession& ss, int64_t record, int file, const char* what) {
    return ss.bad("record " + std::to_string(record) + (file ? " of file " + std::to_string(file) : std::string()) + what);
}
static int map_file_malformed(MapFileSession& ss, int64_t record, int file) {
    return map_file_bad_record(ss, record, file, " is malformed (line 1 of a record starts with '@', line 3 with '+')");
}

/* ASM_OUT_BAM, behind a chunk's malformed records and in front of its other errors: the chunk's smallest record whose QNAME no BAM
 * record can hold (d_recs: the chunk's rn records; PAIRED: [2][rn], file 1 before file 2), reported as a malformed one is.  Under
 * ASM_OUT_SAM nothing is launched. */
template <bool PAIRED>
static int map_file_bam_names(MapFileSession& ss, const char* d_raw, const SamRec* d_recs, int64_t rn, int64_t first_record) {
    if (!ss.out.bam || rn == 0) return ASM_OK;
    asm_handle* h = ss.h;
    Scratch<uint32_t> d_long(h);
    uint32_t min_long[2] = {FASTQ_NO_RECORD, FASTQ_NO_RECORD};
    STREAM_TRY(ss.who, d_long.alloc(sizeof min_long));
    STREAM_TRY(ss.who, hipMemsetAsync(d_long.p, 0xff, sizeof min_long, h->stream));
    STREAM_TRY(ss.who, launch(h, bam_name_check_kernel<PAIRED>, grid_for((PAIRED ? 2 : 1) * rn), ASM_BLOCK, d_raw, d_recs, (long)rn, d_long.p));
    STREAM_TRY(ss.who, fetch(h, {fetched(min_long, (const uint32_t*)d_long.p, 2)}));
    for (int f = 0; f < 2; f++)
        if (min_long[f] != FASTQ_NO_RECORD)
            return map_file_bad_record(ss, first_record + min_long[f] + 1, PAIRED ? f + 1 : 0,
                                       " has a QNAME of more than 254 bytes, which a BAM record cannot hold");
    return ASM_OK;
}

/* The gather stage of one device chunk, for both file calls: n library reads of `bytes` bytes in all.  compact(d_start) launches
 * the call's compact kernel, which writes every read's start in d_raw and f.d_roff; then the reads are gathered into f.d_reads,
 * numbered in file order, and f.roff and f.bytes are filled. */
template <class C>
static int map_file_gather(MapFileSession& ss, const char* d_raw, int64_t n, size_t bytes, MapFront& f, C compact) {
    asm_handle* h = ss.h;
    Scratch<unsigned long long> d_start(h);
    f.bytes = bytes;
    STREAM_TRY(ss.who, f.d_reads.alloc(bytes + 16));
    STREAM_TRY(ss.who, f.d_roff.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    STREAM_TRY(ss.who, d_start.alloc(sizeof(unsigned long long) * ((size_t)n + 1)));
    STREAM_TRY(ss.who, compact(d_start.p));
    if (n == 0) return ASM_OK;
    STREAM_TRY(ss.who, launch_text_gather(h, d_raw, d_start.p, f.d_roff.p, n, f.d_reads.p));
    f.roff.resize((size_t)n + 1);
    STREAM_TRY(ss.who, fetch(h, {fetched(f.roff.data(), f.d_roff.p, (size_t)n + 1)}));
    return ASM_OK;
}

/* The format tail of one device chunk, for both file calls: a holds the chunk's records, results, line list and nlines; the
 * RNAME table, size, off and the counters are set here.  Every line's size and offset, then the total and the call's counters n
 * (mapped; paired: proper and rescued too) in one wait.  Then the lines are emitted: into the output (MapOutput::put), or for a
 * sorted call into a block that stays on the device. */
template <bool PAIRED>
static int map_file_format(MapFileSession& ss, MapTmp& tmp, SamArgs& a, unsigned long long* n) {
    asm_handle* h = ss.h;
    const char* who = ss.who;
    const int64_t nlines = a.nlines;
    constexpr size_t NC = PAIRED ? 3 : 1;
    Scratch<unsigned long long> d_size(h), d_off(h), d_n(h);
    STREAM_TRY(who, d_size.alloc(sizeof(unsigned long long) * ((size_t)nlines + 1)));
    STREAM_TRY(who, d_off.alloc(sizeof(unsigned long long) * ((size_t)nlines + 1)));
    STREAM_TRY(who, d_n.alloc(sizeof(unsigned long long) * NC));
    STREAM_TRY(who, hipMemsetAsync(d_n.p, 0, sizeof(unsigned long long) * NC, h->stream));
    a.names = ss.d_names.p, a.name_off = ss.d_name_off.p, a.size = d_size.p, a.off = d_off.p, a.n_mapped = d_n.p;
    if (PAIRED) a.n_proper = d_n.p + 1, a.n_rescued = d_n.p + 2;
    const bool bam = ss.out.bam != nullptr;
    const LineKernels k = line_kernels<PAIRED>(bam);
    STREAM_TRY(who, launch(h, k.size, grid_for(nlines + 1), ASM_BLOCK, a));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_size.p, d_off.p, nlines + 1));
    unsigned long long total = 0;
    STREAM_TRY(who, fetch(h, {fetched(&total, d_off.p + nlines), fetched(n, d_n.p, NC)}));
    ss.st.records += nlines, ss.st.chunks++;
    if (ss.sort) return ss.sort->hold<PAIRED>(a, total, bam); /* nothing is written yet */
    return ss.out.put((size_t)total, [&](char* dst) {
        a.out = dst;
        return launch(h, k.emit, map_grid((uint64_t)nlines * 64, h), 256, a);
    });
}

/* One file chunk (`lines` lines of whole records in d_raw[0, nbytes)), for both file calls: the newline index, then
 * one(d_nl, r0, rn) for each of its device chunks of at most `step` out of `units` */
template <class F>
static int map_file_device_chunks(MapFileSession& ss, const char* d_raw, size_t nbytes, int64_t lines, int64_t units, int64_t step, F one) {
    asm_handle* h = ss.h;
    Scratch<uint32_t> d_nl(h);
    MapTmp tmp(h);
    STREAM_TRY(ss.who, d_nl.alloc(sizeof(uint32_t) * ((size_t)lines + 2)));
    STREAM_TRY(ss.who, newline_index(h, tmp, d_raw, nbytes, (long)lines, d_nl.p));
    return map_chunks(units, step, [&](int64_t r0, int64_t rn) { return one((const uint32_t*)d_nl.p, r0, rn); });
}

/* chunk_bytes as both entry points take it: 0 is 16 MiB, and 1 GiB is the most */
static int map_file_chunk_bytes(asm_handle* h, const char* who, int64_t chunk_bytes, size_t* chunk) {
    if (chunk_bytes < 0) return fail(h, ASM_EINVAL, std::string(who) + ": chunk_bytes must be >= 0");
    *chunk = chunk_bytes == 0 ? (size_t)16 << 20 : (size_t)std::min<int64_t>(chunk_bytes, (int64_t)1 << 30);
    return ASM_OK;
}

/* ---- asm_map_file's own ---------------------------------------------------------------------------------------------------------- */
struct MapReadsFileJob : MapFileJob {
    int max_hits, strata;
    asm_map_file_stats st = {};
};

/* Records [r0, r0 + rn) of the file chunk whose bytes are d_raw and whose newline positions are d_nl: one device chunk, from the
 * record kernel to the writer's queue.  first_record: the file's records before r0 (for the message of a malformed one). */
static int map_file_chunk(MapReadsFileJob& j, const char* d_raw, const uint32_t* d_nl, int64_t r0, int64_t rn, int64_t first_record) {
    MapFileSession& ss = j.ss;
    asm_handle* h = ss.h;
    const char* who = ss.who;
    const asm_index* ix = j.ix;
    const asm_map_params* p = j.p;
    const size_t cnt = (size_t)rn + 1;
    MapTmp tmp(h);
    /* the records, and which of them go to the mapper */
    Scratch<SamRec> d_recs(h);
    Scratch<uint32_t> d_send(h), d_mlen(h), d_rd(h), d_mo(h);
    Scratch<int32_t> d_rec_read(h);
    Scratch<FastqCounts> d_counts(h);
    STREAM_TRY(who, d_recs.alloc(sizeof(SamRec) * (size_t)rn));
    for (Scratch<uint32_t>* x : {&d_send, &d_mlen, &d_rd, &d_mo}) STREAM_TRY(who, x->alloc(sizeof(uint32_t) * cnt));
    STREAM_TRY(who, d_rec_read.alloc(sizeof(int32_t) * (size_t)rn));
    STREAM_TRY(who, d_counts.alloc(sizeof(FastqCounts)));
    STREAM_TRY(who, hipMemsetAsync(&d_counts.p->bad_min, 0xff, sizeof(uint32_t), h->stream));
    STREAM_TRY(who, hipMemsetAsync(&d_counts.p->too_long, 0, sizeof(uint32_t), h->stream));
    STREAM_TRY(who, launch(h, fastq_record_kernel, grid_for(rn + 1), ASM_BLOCK, d_raw, d_nl, (long)r0, (long)rn, (uint32_t)ASM_MAP_MAX_READ,
                           d_recs.p, d_send.p, d_mlen.p, d_counts.p));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_send.p, d_rd.p, (int64_t)cnt));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_mlen.p, d_mo.p, (int64_t)cnt));
    uint32_t tot[2] = {0, 0};
    FastqCounts counts = {FASTQ_NO_RECORD, 0};
    STREAM_TRY(who, fetch(h, {fetched(&tot[0], d_rd.p + rn), fetched(&tot[1], d_mo.p + rn), fetched(&counts, d_counts.p)}));
    if (counts.bad_min != FASTQ_NO_RECORD) return map_file_malformed(ss, first_record + counts.bad_min + 1, 0);
    if (const int rc = map_file_bam_names<false>(ss, d_raw, d_recs.p, rn, first_record)) return rc;
    const int64_t ns = tot[0]; /* library reads */
    /* compact and gather: the reads in HBM, numbered in file order */
    MapFront f(h);
    if (const int rc = map_file_gather(ss, d_raw, ns, tot[1], f, [&](unsigned long long* d_start) {
            return launch(h, fastq_compact_kernel, grid_for(rn + 1), ASM_BLOCK, (const SamRec*)d_recs.p, (const uint32_t*)d_send.p,
                          (const uint32_t*)d_rd.p, (const uint32_t*)d_mo.p, (long)rn, d_rec_read.p, f.d_roff.p, d_start);
        }))
        return rc;
    /* map: the library's stages, fed from device memory; the records, ops and nops stay there */
    Scratch<unsigned long long> d_keys(h);
    MapAllItems ai(h);
    MapFinish fin(h);
    MapRuns runs(h);
    MapMapq mm(h); /* ASM_MAPQ_GAP: the items' MAPQ bytes, which stay on the device like the records */
    const bool gap = h->mapq_model == ASM_MAPQ_GAP;
    std::vector<uint32_t> n_hits;
    int64_t nlines = rn;
    if (ns > 0) {
        if (const int rc = map_front_seed(h, ix, ns, p, f)) return rc;
        if (j.max_hits == 0) {
            if (const int rc = gap ? map_best_keys_gap(h, ix, ns, p, f, who, runs, mm, d_keys) : map_best_keys(h, ix, ns, p, f, d_keys)) return rc;
            if (const int rc = map_finish_launch(h, ix, p, f, ns, d_keys.p, nullptr, nullptr, f.bytes + (size_t)ns, SAM_CIGAR_CAP, fin))
                return rc;
        } else {
            n_hits.resize((size_t)ns);
            if (const int rc = map_all_items(h, ix, ns, p, j.strata, j.max_hits, f, n_hits.data(), ai, who)) return rc;
            if (gap)
                if (const int rc = map_mapq_reads(h, ix, f, ai.runs, ns, p->max_errors, mm, nullptr, ai.d_ibase.p, ai.d_ikey.p, ai.ni)) return rc;
            if (const int rc = map_finish_launch(h, ix, p, f, ai.ni, ai.d_ikey.p, ai.d_iread.p, ai.d_idirs.p, ai.dwords, SAM_CIGAR_CAP, fin))
                return rc;
            nlines = (rn - ns) + ai.ni; /* the item list is in read-then-rank order, which is SAM order */
        }
        if (const int rc = map_finish_device(h, ix, p, f, fin)) return rc;
    }
    if (nlines > (int64_t)INT32_MAX) return ss.bad("more than 2^31 - 1 SAM lines in a chunk", ASM_EUNSUPPORTED);
    /* format: the line list here, the rest in the tail */
    Scratch<uint32_t> d_lcnt(h), d_lbase(h), d_lrec(h), d_litem(h);
    STREAM_TRY(who, d_lcnt.alloc(sizeof(uint32_t) * cnt));
    STREAM_TRY(who, d_lbase.alloc(sizeof(uint32_t) * cnt));
    STREAM_TRY(who, d_lrec.alloc(sizeof(uint32_t) * (size_t)nlines));
    STREAM_TRY(who, d_litem.alloc(sizeof(uint32_t) * (size_t)nlines));
    SamArgs a = {};
    a.raw = d_raw, a.recs = d_recs.p, a.rec_read = d_rec_read.p, a.nrec = (long)rn, a.nlines = (long)nlines;
    a.line_rec = d_lrec.p, a.line_item = d_litem.p;
    a.mapq = mm.d_item, a.md = fin.d_md.p, a.md_len = fin.d_md_len.p;
    a.hits = fin.d_hits.p, a.ops = fin.d_ops.p, a.nops = fin.d_nops.p, a.ibase = (j.max_hits > 0 && ns > 0) ? ai.d_ibase.p : nullptr;
    a.n_hits = ai.d_nh.p, a.line_cnt = d_lcnt.p, a.line_base = d_lbase.p;
    /* the line list reads nrec, rec_read, ibase, line_cnt and line_base of a; what the tail sets (names, size, off, n_mapped) it does not */
    STREAM_TRY(who, launch(h, sam_line_count_kernel, grid_for(rn + 1), ASM_BLOCK, a));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_lcnt.p, d_lbase.p, (int64_t)cnt));
    STREAM_TRY(who, launch(h, sam_line_fill_kernel, grid_for(rn), ASM_BLOCK, a, d_lrec.p, d_litem.p));
    unsigned long long n_mapped = 0;
    if (const int rc = map_file_format<false>(ss, tmp, a, &n_mapped)) return rc;
    j.st.reads += rn, j.st.mapped += (int64_t)n_mapped, j.st.too_long += counts.too_long;
    return ASM_OK;
}

/* ---- a BGZF-compressed FASTQ file (docs/design/mapper.md, "Compressed input") ---------------------------------------------------- */
struct BgzfCutOut {
    unsigned long long lines; /* the text's newlines, an appended one included */
    unsigned long long cut;   /* the bytes of the text's whole records: behind newline 4 * (lines / 4) - 1 */
    uint32_t appended;        /* a newline was appended behind the text (the end of the file) */
    uint32_t pad;
};
/* One wavefront, every lane the same answer: the byte behind newline k (counted from 0) of text[0, nbytes), which holds more than k.
 * tile_base[0 .. ntiles]: the exclusive sums of seq_count_kernel's tile counts, from any origin (tile_base[0] newlines lie in front of
 * the text).  The newline's tile is found by bisection, the newline in it by ballots over 64 bytes at a time. */
ASM_DEV unsigned long long seq_behind_newline(const char* __restrict__ text, unsigned long long nbytes, const uint32_t* __restrict__ tile_base,
                                              uint32_t ntiles, uint32_t k, uint32_t lane) {
    k += tile_base[0];
    uint32_t lo = 0u, hi = ntiles - 1u; /* the last tile with tile_base <= k */
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (tile_base[mid] <= k) lo = mid;
        else hi = mid - 1u;
    }
    uint32_t left = k - tile_base[lo]; /* newlines of the tile in front of it */
    const unsigned long long t0 = (unsigned long long)lo * SEQ_TILE;
    for (uint32_t i = 0; i < SEQ_TILE; i += 64u) {
        const unsigned long long at = t0 + i + lane;
        const unsigned long long mask = __ballot(at < nbytes && text[at] == '\n');
        const uint32_t c = (uint32_t)__popcll(mask);
        if (left < c) {
            unsigned long long m = mask;
            for (uint32_t d = 0; d < left; d++) m &= m - 1u;
            return t0 + i + (uint32_t)__builtin_ctzll(m) + 1u;
        }
        left -= c;
    }
    return 0ull; /* not reached: the tile holds the newline */
}

/* One wavefront, behind seq_count_kernel and the exclusive sum of its tile counts (tile_base[ntiles]: all newlines): the record cut
 * of text[0, nbytes).  is_last: a text that does not end in a newline gets one at text[nbytes] (the buffer has room). */
__global__ __launch_bounds__(64) void bgzf_cut_kernel(char* __restrict__ text, unsigned long long nbytes, const uint32_t* __restrict__ tile_base,
                                                      uint32_t ntiles, int is_last, BgzfCutOut* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const unsigned long long counted = ntiles ? tile_base[ntiles] : 0ull;
    const bool append = is_last && nbytes > 0 && text[nbytes - 1] != '\n';
    const unsigned long long lines = counted + (append ? 1u : 0u), need = lines / 4u * 4u;
    unsigned long long cut = 0;
    if (need > counted) cut = nbytes + 1u; /* the appended newline closes the last record */
    else if (need > 0) cut = seq_behind_newline(text, nbytes, tile_base, ntiles, (uint32_t)(need - 1u), lane);
    if (lane == 0u) {
        if (append) text[nbytes] = '\n';
        out->lines = lines, out->cut = cut, out->appended = append ? 1u : 0u, out->pad = 0u;
    }
}

/* The device side of a BGZF input: the text left over behind a chunk's last whole record stays in `carry` on the device and leads
 * the next chunk's text, as BgzfStream does on the output side. */
struct BgzfInput {
    asm_handle* h;
    Scratch<char> carry;
    size_t carry_len = 0, carry_cap = 0;
    int64_t records_seen = 0;
    asm_host::BgzfChunkInfo pend[2]; /* what the reader said of the chunks in flight, by device buffer */
    bool pend_last[2] = {false, false};
    explicit BgzfInput(asm_handle* owner) : h(owner), carry(owner) {}
};
static int map_file_member_error(MapFileSession& ss, size_t member, size_t offset, const char* what) {
    return ss.bad("BGZF member " + std::to_string(member) + " at offset " + std::to_string(offset) + ": " + what);
}

/* One file chunk of compressed members in d_src: inflated behind the carry, cut into records on the device (one wait: the line
 * count, the cut, the first failed member), handed to map_file_device_chunks / map_file_chunk as a plain chunk is; the rest of the
 * text is the next carry. */
static int map_file_gz_chunk(MapReadsFileJob& j, BgzfInput& gz, const char* d_src, const asm_host::BgzfChunkInfo& ci, bool is_last) {
    MapFileSession& ss = j.ss;
    asm_handle* h = ss.h;
    const char* who = ss.who;
    typedef unsigned long long u64;
    const size_t nbytes = gz.carry_len + ci.text;
    if (nbytes >= 0xfffffff0ull) return ss.bad("a chunk of 4 GiB or more of text; lower chunk_bytes", ASM_EUNSUPPORTED);
    Scratch<char> d_text(h);
    Scratch<InfMember> d_members(h);
    Scratch<u64> d_bad(h);
    Scratch<BgzfCutOut> d_cut(h);
    Scratch<uint32_t> d_tile(h), d_tbase(h);
    MapTmp tmp(h);
    const uint32_t ntiles = (uint32_t)((nbytes + SEQ_TILE - 1) / SEQ_TILE);
    STREAM_TRY(who, d_text.alloc(nbytes + 64));
    STREAM_TRY(who, d_members.alloc(sizeof(InfMember) * (ci.members.size() + 1)));
    STREAM_TRY(who, d_bad.alloc(sizeof(u64)));
    STREAM_TRY(who, d_cut.alloc(sizeof(BgzfCutOut)));
    STREAM_TRY(who, d_tile.alloc(sizeof(uint32_t) * ((size_t)ntiles + 1)));
    STREAM_TRY(who, d_tbase.alloc(sizeof(uint32_t) * ((size_t)ntiles + 1)));
    if (gz.carry_len) STREAM_TRY(who, hipMemcpyAsync(d_text.p, gz.carry.p, gz.carry_len, hipMemcpyDeviceToDevice, h->stream));
    if (!ci.members.empty())
        STREAM_TRY(who, hipMemcpyAsync(d_members.p, ci.members.data(), sizeof(InfMember) * ci.members.size(), hipMemcpyHostToDevice, h->stream));
    STREAM_TRY(who, bgzf_inflate_device(h, (const uint8_t*)d_src, d_members.p, ci.members.size(), (uint8_t*)d_text.p + gz.carry_len, d_bad.p));
    STREAM_TRY(who, hipMemsetAsync(d_tile.p, 0, sizeof(uint32_t) * ((size_t)ntiles + 1), h->stream));
    if (ntiles) {
        STREAM_TRY(who, launch(h, seq_count_kernel, ntiles, 256, (const char*)d_text.p, (long)nbytes, d_tile.p));
        STREAM_TRY(who, map_exclusive_sum(h, tmp, d_tile.p, d_tbase.p, (int64_t)ntiles + 1));
    }
    STREAM_TRY(who, launch(h, bgzf_cut_kernel, 1u, 64u, d_text.p, (u64)nbytes, (const uint32_t*)d_tbase.p, ntiles, is_last ? 1 : 0, d_cut.p));
    u64 bad = INF_NONE_BAD;
    BgzfCutOut cut = {};
    STREAM_TRY(who, fetch(h, {fetched(&bad, (const u64*)d_bad.p), fetched(&cut, (const BgzfCutOut*)d_cut.p)}));
    if (bad != INF_NONE_BAD) {
        const size_t k = (size_t)(bad >> 8);
        return map_file_member_error(ss, (size_t)ci.first_member + k, ci.file_base + (size_t)ci.members[k].src_off, inf_status_text((uint32_t)(bad & 0xffu)));
    }
    if (ci.err.status != BGZF_IN_OK) return map_file_member_error(ss, ci.err.member, ci.err.offset, bgzf_in_text(ci.err.status));
    const int64_t records = (int64_t)(cut.lines / 4u);
    if (is_last && (cut.lines & 3u))
        return ss.bad("record " + std::to_string(gz.records_seen + records + 1) + " is truncated (the file's line count is not a multiple of 4)");
    const size_t text_end = nbytes + cut.appended;
    if (records > 0) {
        const int64_t first_record = gz.records_seen;
        const char* d_raw = d_text.p;
        if (const int rc = map_file_device_chunks(ss, d_raw, (size_t)cut.cut, 4 * records, records, std::min<int64_t>(h->map_chunk, (int64_t)1 << 30),
                                                  [&](const uint32_t* d_nl, int64_t r0, int64_t rn) {
                                                      return map_file_chunk(j, d_raw, d_nl, r0, rn, first_record + r0);
                                                  }))
            return rc;
        gz.records_seen += records;
    }
    const size_t rest = text_end - (size_t)cut.cut;
    if (rest > gz.carry_cap) { /* the old carry has been copied into d_text, in stream order */
        pool_free(h, gz.carry.p);
        gz.carry.p = nullptr, gz.carry_cap = 0;
        STREAM_TRY(who, gz.carry.alloc(rest + rest / 2 + 65536));
        gz.carry_cap = rest + rest / 2 + 65536;
    }
    if (rest) STREAM_TRY(who, hipMemcpyAsync(gz.carry.p, d_text.p + cut.cut, rest, hipMemcpyDeviceToDevice, h->stream));
    gz.carry_len = rest;
    return ASM_OK;
}

/* What an input file starts with: *gzip = a gzip member, which is BGZF or refused here as plain gzip; else text (or nothing).  The
 * file calls probe at open and nowhere else; MapFileSession::open's first-byte probe (FASTA) stays apart. */
static int map_file_probe(MapFileSession& ss, int fd, size_t file_bytes, const char* path, bool* gzip) {
    uint8_t probe[4096];
    const size_t probed = file_bytes ? (size_t)std::max<ssize_t>(pread(fd, probe, std::min(file_bytes, sizeof probe), 0), 0) : 0;
    *gzip = probed >= 2 && probe[0] == 0x1fu && probe[1] == 0x8bu;
    if (*gzip && bgzf_is_plain_gzip(probe, probed))
        return ss.bad(std::string(path) + " is plain gzip, not BGZF (no BC subfield in its first member): recompress it with bgzip",
                      ASM_EUNSUPPORTED);
    return ASM_OK;
}

/* map_file_run for a file that starts with a BGZF member */
static int map_file_run_gz(MapFileSession& ss, MapReadsFileJob& j, const char* fastq_path, size_t file_bytes) {
    asm_handle* h = ss.h;
    StreamInput& in = ss.in;
    BgzfInput gz(h);
    asm_host::ChunkReader<asm_host::BgzfFill> rd(ss.chunk, ss.first_chunk, in.wait_shipped(), in.fd, file_bytes, ss.grow());
    /* info[q] is read while the reader runs: slot q's hand-over (ready under the reader's mutex, refilled only after consumed())
     * orders it, as it orders the slot's bytes */
    const asm_host::BgzfFill& fill = rd.policy();
    ss.text_bytes = [&](const asm_host::ChunkSlot& s) { return fill.info[(&s - rd.slot)].text; };
    bool header_error = false; /* a bad header in a chunk without members: reported behind the chunks in front of it */
    asm_host::BgzfChunkInfo bad_chunk;
    int c = 0;
    const int rc = ss.run(
        rd, std::string(ss.who) + ": reading " + fastq_path + " failed",
        [&](const asm_host::ChunkSlot& s, int64_t) {
            const asm_host::BgzfChunkInfo& ci = fill.info[&s - rd.slot];
            if (s.units > 0) gz.pend[c & 1] = ci, gz.pend_last[c & 1] = s.last;
            else if (ci.err.status != BGZF_IN_OK) header_error = true, bad_chunk = ci;
            c++;
            return (int)ASM_OK;
        },
        [&](int q, size_t, int64_t, int64_t) { return map_file_gz_chunk(j, gz, in.d_raw[q], gz.pend[q], gz.pend_last[q]); });
    rd.stop();
    ss.text_bytes = nullptr; /* it refers to the reader, which ends here */
    if (rc) return rc;
    if (header_error) return map_file_member_error(ss, bad_chunk.err.member, bad_chunk.err.offset, bgzf_in_text(bad_chunk.err.status));
    return ASM_OK;
}

/* sort_cap: NULL for asm_map_file, max_device_bytes for asm_map_file_sorted */
static int map_file_run(asm_handle* h, const char* who, const asm_index* ix, const char* const* seq_names, const char* fastq_path,
                        const char* sam_path, const char* header, const asm_map_params* p, int max_hits, int strata, size_t chunk,
                        asm_map_file_stats* stats, const int64_t* sort_cap, asm_sam_sort_stats* sort_stats) {
    MapFileSession ss(h, who, chunk);
    if (sort_cap) ss.sort.reset(new SamSortHold(h, who, ix->n_seqs, (size_t)*sort_cap));
    StreamInput& in = ss.in;
    size_t file_bytes = 0;
    if (const int rc = in.open_file(fastq_path, &file_bytes)) return rc;
    /* the first bytes: a BGZF member (the compressed path), plain gzip (refused), or text, which goes on as before */
    bool gzip = false;
    if (const int rc = map_file_probe(ss, in.fd, file_bytes, fastq_path, &gzip)) return rc;
    if (const int rc = ss.open(ix, seq_names, 1, &in.fd, &file_bytes, &fastq_path, sam_path, header)) return rc;
    MapReadsFileJob j = {{ss, ix, p}, max_hits, strata};
    if (gzip) {
        if (const int rc = map_file_run_gz(ss, j, fastq_path, file_bytes)) return rc;
        if (const int rf = ss.finish(j.st)) return rf;
        if (stats) *stats = j.st;
        if (sort_stats && ss.sort) *sort_stats = ss.sort->st;
        return ASM_OK;
    }
    asm_host::ChunkReader<asm_host::FastqFill> rd(chunk, ss.first_chunk, in.wait_shipped(), in.fd, file_bytes, chunk, ss.grow());
    const int rc = ss.run(
        rd, std::string(who) + ": reading " + fastq_path + " failed",
        [&](const asm_host::ChunkSlot& s, int64_t records_seen) {
            if (s.extra_lines)
                return ss.bad("record " + std::to_string(records_seen + s.units + 1) +
                              " is truncated (the file's line count is not a multiple of 4)");
            return (int)ASM_OK;
        },
        [&](int q, size_t bytes, int64_t records, int64_t first_record) {
            /* the run key of asm_map_reads_all holds the read in its top 31 bits */
            return map_file_device_chunks(ss, in.d_raw[q], bytes, 4 * records, records, std::min<int64_t>(h->map_chunk, (int64_t)1 << 30),
                                          [&](const uint32_t* d_nl, int64_t r0, int64_t rn) {
                                              return map_file_chunk(j, in.d_raw[q], d_nl, r0, rn, first_record + r0);
                                          });
        });
    if (rc) return rc;
    if (const int rf = ss.finish(j.st)) return rf;
    if (stats) *stats = j.st;
    if (sort_stats && ss.sort) *sort_stats = ss.sort->st;
    return ASM_OK;
}

/* max_device_bytes of the two sorted calls: checked behind chunk_bytes */
static int map_file_sort_cap(asm_handle* h, const char* who, const int64_t* sort_cap) {
    return sort_cap && *sort_cap < 0 ? fail(h, ASM_EINVAL, std::string(who) + ": max_device_bytes must be >= 0") : (int)ASM_OK;
}

/* A sorted BAM call under ASM_BAM_INDEX_BAI, behind the other argument checks: BAI holds coordinates below 2^29 */
static int map_file_index_check(asm_handle* h, const char* who, const asm_index* ix, const char* const* seq_names, const int64_t* sort_cap) {
    if (!sort_cap || h->out_format != ASM_OUT_BAM || h->bam_index != ASM_BAM_INDEX_BAI) return ASM_OK;
    for (int32_t r = 0; r < asm_index_n_seqs(ix); r++)
        if (asm_index_seq_len(ix, r) > ((uint64_t)1 << 29))
            return fail(h, ASM_EUNSUPPORTED, std::string(who) + ": sequence " + std::to_string(r) + " (" + (seq_names[r] ? seq_names[r] : "") + ") has " +
                                                 std::to_string(asm_index_seq_len(ix, r)) +
                                                 " bases; a .bai index holds coordinates below 2^29: such a reference needs a .csi index");
    return ASM_OK;
}

/* asm_map_file and asm_map_file_sorted (`who`): the argument checks, then the call */
static int map_file_call(const char* who, asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq_path,
                         const char* sam_path, const char* header, const asm_map_params* p, int max_hits, int strata, int64_t chunk_bytes,
                         asm_map_file_stats* stats, const int64_t* sort_cap, asm_sam_sort_stats* sort_stats) {
    const std::string name = who;
    if (!p || !ix || !seq_names || !fastq_path || !sam_path) return fail(h, ASM_EINVAL, name + ": bad arguments");
    if (max_hits < 0 || max_hits > ASM_MAP_MAX_HITS) return fail(h, ASM_EINVAL, name + ": max_hits must be in [0, 256]");
    size_t chunk = 0;
    if (const int rc = map_file_chunk_bytes(h, who, chunk_bytes, &chunk)) return rc;
    if (const int rc = map_file_sort_cap(h, who, sort_cap)) return rc;
    if (const int rc = map_check_args(h, ix, who, "read",
                                      {0, p, {nullptr, nullptr}, nullptr, max_hits ? "max_hits" : nullptr, strata, ASM_MAP_MAX_ERRORS,
                                       max_hits, {nullptr, 0, nullptr}}))
        return rc;
    if (const int rc = map_file_index_check(h, who, ix, seq_names, sort_cap)) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (sort_stats) memset(sort_stats, 0, sizeof *sort_stats);
    HIPCHK(h, hipSetDevice(h->device));
    return map_file_run(h, who, ix, seq_names, fastq_path, sam_path, header, p, max_hits, strata, chunk, stats, sort_cap, sort_stats);
}

} /* extern "C++" */

int asm_map_file(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq_path, const char* sam_path,
                 const char* header, const asm_map_params* p, int max_hits, int strata, int64_t chunk_bytes, asm_map_file_stats* stats) {
    return map_file_call("asm_map_file", h, ix, seq_names, fastq_path, sam_path, header, p, max_hits, strata, chunk_bytes, stats, nullptr,
                         nullptr);
}

int asm_map_file_sorted(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq_path, const char* sam_path,
                        const char* header, const asm_map_params* p, int max_hits, int strata, int64_t chunk_bytes,
                        int64_t max_device_bytes, asm_map_file_stats* stats, asm_sam_sort_stats* sort_stats) {
    return map_file_call("asm_map_file_sorted", h, ix, seq_names, fastq_path, sam_path, header, p, max_hits, strata, chunk_bytes, stats,
                         &max_device_bytes, sort_stats);
}

size_t asm_fastq_cut(const char* buf, size_t nbytes, int64_t* records) {
    if (!buf) nbytes = 0;
    return asm_host::fastq_cut(buf, nbytes, records);
}
