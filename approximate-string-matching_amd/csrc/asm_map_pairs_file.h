// asm_map_pairs_file: two FASTQ files in, a paired SAM file out, parsed, paired, mapped and formatted on the device (design:
// docs/design/mapper.md, "Files: two FASTQ files in, paired SAM out").  The reader keeps the two files in step (FastqPairFill,
// asm_host.h); a chunk holds the mate-1 records and then as many mate-2 records in one buffer, so the input pipeline, the newline
// index and the record kernel are asm_map_file's, as are the output rotation and the writer (MapFilePipe, map_file_hand_over); the
// mapper's stages are asm_map_pairs' (map_pairs_front_seed) and the finish stage stays on the device (map_finish_device).
// asm_capi.hip includes this file inside its extern "C" block, behind asm_map_file.h.
#pragma once

extern "C++" {

#define MAP_PAIRS_FILE_TRY(call) STREAM_TRY("asm_map_pairs_file", call)

struct MapPairsFileJob { /* what every chunk of a call shares */
    asm_handle* h;
    const asm_index* ix;
    const asm_map_params* p;
    const asm_pair_params* pp;
    const char* d_names;
    const uint32_t* d_name_off;
    MapFilePipe* pipe;
    asm_host::ChunkWriter* writer;
    asm_map_pairs_file_stats st = {};
    int64_t out_seq = 0;
};

/* Pairs [r0, r0 + rn) of a file chunk of R pairs (record r of d_raw is mate 1 of pair r, record R + r its mate 2; d_nl: the 8 R
 * newline positions): one device chunk, from the record kernel to the writer's queue.  first_record: the files' records before r0. */
static int map_pairs_file_chunk(MapPairsFileJob& j, const char* d_raw, const uint32_t* d_nl, int64_t R, int64_t r0, int64_t rn,
                                int64_t first_record) {
    asm_handle* h = j.h;
    const asm_index* ix = j.ix;
    const asm_map_params* p = j.p;
    const size_t cnt = (size_t)rn + 1;
    MapTmp tmp(h);
    /* the records of both mates, the pairs and which of them go to the mapper */
    Scratch<SamRec> d_recs(h);
    Scratch<uint32_t> d_send1(h), d_send2(h), d_mlen1(h), d_mlen2(h), d_psend(h), d_len1(h), d_len2(h), d_rd(h), d_mo1(h), d_mo2(h);
    Scratch<int32_t> d_rec_read(h);
    Scratch<FastqCounts> d_counts(h);
    Scratch<FastqPairCounts> d_pcounts(h);
    Scratch<unsigned long long> d_start(h);
    MAP_PAIRS_FILE_TRY(d_recs.alloc(sizeof(SamRec) * 2 * (size_t)rn));
    for (Scratch<uint32_t>* x : {&d_send1, &d_send2, &d_mlen1, &d_mlen2, &d_psend, &d_len1, &d_len2, &d_rd, &d_mo1, &d_mo2})
        MAP_PAIRS_FILE_TRY(x->alloc(sizeof(uint32_t) * cnt));
    MAP_PAIRS_FILE_TRY(d_rec_read.alloc(sizeof(int32_t) * (size_t)rn));
    MAP_PAIRS_FILE_TRY(d_counts.alloc(sizeof(FastqCounts) * 2));
    MAP_PAIRS_FILE_TRY(d_pcounts.alloc(sizeof(FastqPairCounts)));
    /* bad_min and name_min start as FASTQ_NO_RECORD; the record kernel's too_long counts are not read here (unsent covers them) */
    MAP_PAIRS_FILE_TRY(hipMemsetAsync(d_counts.p, 0xff, sizeof(FastqCounts) * 2, h->stream));
    MAP_PAIRS_FILE_TRY(hipMemsetAsync(&d_pcounts.p->name_min, 0xff, sizeof(uint32_t), h->stream));
    MAP_PAIRS_FILE_TRY(hipMemsetAsync(&d_pcounts.p->unsent, 0, sizeof(uint32_t), h->stream));
    hipLaunchKernelGGL(fastq_record_kernel, dim3(grid_for(rn + 1)), dim3(ASM_BLOCK), 0, h->stream, d_raw, d_nl, (long)r0, (long)rn,
                       (uint32_t)ASM_MAP_MAX_READ, d_recs.p, d_send1.p, d_mlen1.p, d_counts.p);
    hipLaunchKernelGGL(fastq_record_kernel, dim3(grid_for(rn + 1)), dim3(ASM_BLOCK), 0, h->stream, d_raw, d_nl, (long)(R + r0), (long)rn,
                       (uint32_t)ASM_MAP_MAX_READ, d_recs.p + rn, d_send2.p, d_mlen2.p, d_counts.p + 1);
    MAP_PAIRS_FILE_TRY(hipGetLastError());
    hipLaunchKernelGGL(fastq_pair_kernel, dim3(grid_for(rn + 1)), dim3(ASM_BLOCK), 0, h->stream, d_raw, (const SamRec*)d_recs.p, (long)rn,
                       (const uint32_t*)d_send1.p, (const uint32_t*)d_send2.p, (const uint32_t*)d_mlen1.p, (const uint32_t*)d_mlen2.p,
                       d_psend.p, d_len1.p, d_len2.p, d_pcounts.p);
    MAP_PAIRS_FILE_TRY(hipGetLastError());
    MAP_PAIRS_FILE_TRY(map_exclusive_sum(h, tmp, d_psend.p, d_rd.p, (int64_t)cnt));
    MAP_PAIRS_FILE_TRY(map_exclusive_sum(h, tmp, d_len1.p, d_mo1.p, (int64_t)cnt));
    MAP_PAIRS_FILE_TRY(map_exclusive_sum(h, tmp, d_len2.p, d_mo2.p, (int64_t)cnt));
    uint32_t tot[3] = {0, 0, 0};
    FastqCounts counts[2] = {{FASTQ_NO_RECORD, 0u}, {FASTQ_NO_RECORD, 0u}};
    FastqPairCounts pcounts = {FASTQ_NO_RECORD, 0u};
    MAP_PAIRS_FILE_TRY(hipMemcpyAsync(&tot[0], d_rd.p + rn, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    MAP_PAIRS_FILE_TRY(hipMemcpyAsync(&tot[1], d_mo1.p + rn, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    MAP_PAIRS_FILE_TRY(hipMemcpyAsync(&tot[2], d_mo2.p + rn, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    MAP_PAIRS_FILE_TRY(hipMemcpyAsync(counts, d_counts.p, sizeof counts, hipMemcpyDeviceToHost, h->stream));
    MAP_PAIRS_FILE_TRY(hipMemcpyAsync(&pcounts, d_pcounts.p, sizeof pcounts, hipMemcpyDeviceToHost, h->stream));
    MAP_PAIRS_FILE_TRY(hipStreamSynchronize(h->stream));
    for (int f = 0; f < 2; f++)
        if (counts[f].bad_min != FASTQ_NO_RECORD)
            return fail(h, ASM_EINVAL, "asm_map_pairs_file: record " + std::to_string(first_record + counts[f].bad_min + 1) + " of file " +
                                           std::to_string(f + 1) + " is malformed (line 1 of a record starts with '@', line 3 with '+')");
    if (pcounts.name_min != FASTQ_NO_RECORD)
        return fail(h, ASM_EINVAL, "asm_map_pairs_file: the mates of record " + std::to_string(first_record + pcounts.name_min + 1) +
                                       " have different names (QNAME is the first word without a trailing /1 or /2)");
    const int64_t ns = tot[0]; /* sent pairs: library reads [0, ns) are their mates 1, [ns, 2 ns) their mates 2 */
    MapPairFront pf(h);
    MapFront& f = pf.f;
    MapFinish fin(h);
    f.bytes = (size_t)tot[1] + tot[2];
    MAP_PAIRS_FILE_TRY(f.d_reads.alloc(f.bytes + 16));
    MAP_PAIRS_FILE_TRY(f.d_roff.alloc(sizeof(uint32_t) * (2 * (size_t)ns + 1)));
    MAP_PAIRS_FILE_TRY(d_start.alloc(sizeof(unsigned long long) * (2 * (size_t)ns + 1)));
    hipLaunchKernelGGL(fastq_pair_compact_kernel, dim3(grid_for(rn + 1)), dim3(ASM_BLOCK), 0, h->stream,
                       (const SamRec*)d_recs.p, (const uint32_t*)d_psend.p, (const uint32_t*)d_rd.p, (const uint32_t*)d_mo1.p,
                       (const uint32_t*)d_mo2.p, (long)rn, d_rec_read.p, f.d_roff.p, d_start.p);
    MAP_PAIRS_FILE_TRY(hipGetLastError());
    if (ns > 0) {
        hipLaunchKernelGGL(seq_gather_kernel, dim3((unsigned)std::min<int64_t>((2 * ns + 3) / 4, 256 * 16)), dim3(ASM_BLOCK), 0, h->stream,
                           d_raw, (const unsigned long long*)d_start.p, (const uint32_t*)f.d_roff.p, (long)(2 * ns), f.d_reads.p);
        MAP_PAIRS_FILE_TRY(hipGetLastError());
        f.roff.resize(2 * (size_t)ns + 1);
        MAP_PAIRS_FILE_TRY(hipMemcpyAsync(f.roff.data(), f.d_roff.p, sizeof(uint32_t) * (2 * (size_t)ns + 1), hipMemcpyDeviceToHost, h->stream));
        MAP_PAIRS_FILE_TRY(hipStreamSynchronize(h->stream));
        /* map: asm_map_pairs' stages on reads that are in HBM already; records, ops, nops and the pair state stay there */
        if (const int rc = map_pairs_front_seed(h, ix, ns, p, j.pp, "asm_map_pairs_file", pf)) return rc;
        if (const int rc = map_finish_launch(h, ix, p, f, 2 * ns, pf.d_ikey.p, nullptr, nullptr, f.bytes + 2 * (size_t)ns, SAM_CIGAR_CAP, fin))
            return rc;
        if (const int rc = map_finish_device(h, ix, p, f, fin)) return rc;
    }
    /* format: line 2q + x is mate x of pair q; every line's size, its offset, the bytes */
    const int64_t nlines = 2 * rn;
    Scratch<unsigned long long> d_size(h), d_off(h), d_n(h);
    MAP_PAIRS_FILE_TRY(d_size.alloc(sizeof(unsigned long long) * ((size_t)nlines + 1)));
    MAP_PAIRS_FILE_TRY(d_off.alloc(sizeof(unsigned long long) * ((size_t)nlines + 1)));
    MAP_PAIRS_FILE_TRY(d_n.alloc(sizeof(unsigned long long) * 3));
    MAP_PAIRS_FILE_TRY(hipMemsetAsync(d_n.p, 0, sizeof(unsigned long long) * 3, h->stream));
    SamArgs a = {};
    a.raw = d_raw, a.recs = d_recs.p, a.rec_read = d_rec_read.p, a.nrec = (long)rn, a.nlines = (long)nlines;
    a.hits = fin.d_hits.p, a.ops = fin.d_ops.p, a.nops = fin.d_nops.p, a.names = j.d_names, a.name_off = j.d_name_off;
    a.size = d_size.p, a.off = d_off.p, a.n_mapped = d_n.p, a.n_proper = d_n.p + 1, a.n_rescued = d_n.p + 2;
    a.pair_state = pf.d_state.p, a.n_conc = pf.d_nconc.p, a.n_sent = (long)ns;
    hipLaunchKernelGGL(sam_size_kernel<true>, dim3(grid_for(nlines + 1)), dim3(ASM_BLOCK), 0, h->stream, a);
    MAP_PAIRS_FILE_TRY(hipGetLastError());
    MAP_PAIRS_FILE_TRY(map_exclusive_sum(h, tmp, d_size.p, d_off.p, nlines + 1));
    unsigned long long total = 0, n[3] = {0, 0, 0};
    MAP_PAIRS_FILE_TRY(hipMemcpyAsync(&total, d_off.p + nlines, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    MAP_PAIRS_FILE_TRY(hipMemcpyAsync(n, d_n.p, sizeof n, hipMemcpyDeviceToHost, h->stream));
    MAP_PAIRS_FILE_TRY(hipStreamSynchronize(h->stream));
    if (const int rc = map_file_hand_over<true>(*j.pipe, *j.writer, j.out_seq, a, nlines, total)) return rc;
    j.st.pairs += rn, j.st.proper += (int64_t)n[1], j.st.rescued += (int64_t)n[2], j.st.unsent += pcounts.unsent;
    j.st.records += nlines, j.st.chunks++, j.st.bytes_out += (int64_t)total;
    return ASM_OK;
}

/* One file chunk (R pairs: 2 R whole records in d_raw[0, nbytes)): the newline index, then its device chunks */
static int map_pairs_file_process(MapPairsFileJob& j, const char* d_raw, size_t nbytes, int64_t R, int64_t first_record) {
    asm_handle* h = j.h;
    Scratch<uint32_t> d_nl(h);
    MapTmp tmp(h);
    MAP_PAIRS_FILE_TRY(d_nl.alloc(sizeof(uint32_t) * (8 * (size_t)R + 2)));
    MAP_PAIRS_FILE_TRY(newline_index(h, tmp, d_raw, nbytes, (long)(8 * R), d_nl.p));
    return map_chunks(R, map_pair_step(h), [&](int64_t r0, int64_t rn) {
        return map_pairs_file_chunk(j, d_raw, d_nl.p, R, r0, rn, first_record + r0);
    });
}

static int map_pairs_file_run(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* const path[2],
                              const char* sam_path, const char* header, const asm_map_params* p, const asm_pair_params* pp, size_t chunk,
                              asm_map_pairs_file_stats* stats) {
    const auto t_begin = std::chrono::steady_clock::now();
    MapFilePipe pipe(h, "asm_map_pairs_file");
    StreamInput& in = pipe.in;
    struct Fd { /* file 2 (file 1 is the input side's) */
        int fd = -1;
        ~Fd() {
            if (fd >= 0) close(fd);
        }
    } second;
    size_t file_bytes[2] = {0, 0};
    if (const int rc = in.open_file(path[0], &file_bytes[0])) return rc;
    second.fd = open(path[1], O_RDONLY);
    struct stat st2;
    if (second.fd < 0 || fstat(second.fd, &st2) != 0) return fail(h, ASM_EINVAL, std::string("asm_map_pairs_file: cannot open ") + path[1]);
    file_bytes[1] = (size_t)st2.st_size;
    const int fds[2] = {in.fd, second.fd};
    for (int f = 0; f < 2; f++) {
        char first = 0;
        if (file_bytes[f] && pread(fds[f], &first, 1, 0) != 1) return fail(h, ASM_EINVAL, std::string("asm_map_pairs_file: cannot read ") + path[f]);
        if (first == '>')
            return fail(h, ASM_EUNSUPPORTED, "asm_map_pairs_file: FASTA reads are not supported (file " + std::to_string(f + 1) + " starts with '>')");
    }
    pipe.out = fopen(sam_path, "wb");
    if (!pipe.out) return fail(h, ASM_EINVAL, std::string("asm_map_pairs_file: cannot write ") + sam_path);
    if (header && *header && fwrite(header, 1, strlen(header), pipe.out) != strlen(header))
        return fail(h, ASM_EINVAL, "asm_map_pairs_file: writing the SAM file failed");
    Scratch<char> d_names(h);
    Scratch<uint32_t> d_name_off(h);
    if (const int rc = map_file_names(h, ix, seq_names, "asm_map_pairs_file", d_names, d_name_off)) return rc;
    /* chunks ramp up from an eighth, as asm_map_file's do */
    const size_t slot_cap = chunk + chunk / 4 + 4096, first_chunk = chunk >= ((size_t)8 << 20) ? chunk / 8 : chunk;
    MAP_PAIRS_FILE_TRY(pipe.open_device(slot_cap));
    in.own_pin = true;
    for (char*& q : in.pin) MAP_PAIRS_FILE_TRY(hipHostMalloc((void**)&q, slot_cap + 64, hipHostMallocDefault));
    asm_host::ChunkReader<asm_host::FastqPairFill> rd(
        chunk, first_chunk, in.wait_shipped(), fds[0], fds[1], file_bytes[0], file_bytes[1], chunk,
        [&](int q, size_t cap, size_t keep) { /* a pair longer than the buffer: a larger pinned one (no copy reads the old one now) */
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
    MapPairsFileJob j = {h, ix, p, pp, d_names.p, d_name_off.p, &pipe, &writer};
    rd.start();
    const int rc = in.run(
        rd, std::string("asm_map_pairs_file: reading ") + path[0] + " or " + path[1] + " failed",
        [&](const asm_host::ChunkSlot& s, int64_t) {
            if (s.bytes >= 0xfffffff0ull) return fail(h, ASM_EUNSUPPORTED, "asm_map_pairs_file: a chunk of 4 GiB or more; lower chunk_bytes");
            j.st.bytes_in += (int64_t)s.bytes;
            return ASM_OK;
        },
        [&](int q, size_t bytes, int64_t pairs, int64_t first_record) {
            return map_pairs_file_process(j, in.d_raw[q], bytes, pairs, first_record);
        });
    if (rc) return rc;
    rd.stop();
    /* the ends of the two files, after every pair in front of them has been looked at */
    const asm_host::FastqPairFill& end = rd.policy();
    for (int f = 0; f < 2; f++)
        if (end.extra_lines[f])
            return fail(h, ASM_EINVAL, "asm_map_pairs_file: record " + std::to_string(end.records[f] + 1) + " of file " + std::to_string(f + 1) +
                                           " is truncated (the file's line count is not a multiple of 4)");
    for (int f = 0; f < 2; f++)
        if (end.more[f])
            return fail(h, ASM_EINVAL, "asm_map_pairs_file: record " + std::to_string(end.records[1 - f] + 1) + " of file " + std::to_string(f + 1) +
                                           " has no mate (the two files hold different numbers of records)");
    if (!writer.finish() || fflush(pipe.out) != 0) return fail(h, ASM_EINVAL, "asm_map_pairs_file: writing the SAM file failed");
    j.st.carry_peak = (int64_t)end.carry_peak;
    j.st.seconds_read = rd.read_seconds(), j.st.seconds_write = writer.write_seconds();
    j.st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = j.st;
    return ASM_OK;
}

} /* extern "C++" */

int asm_map_pairs_file(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq1_path, const char* fastq2_path,
                       const char* sam_path, const char* header, const asm_map_params* p, const asm_pair_params* pp, int64_t chunk_bytes,
                       asm_map_pairs_file_stats* stats) {
    if (!p || !pp || !ix || !seq_names || !fastq1_path || !fastq2_path || !sam_path)
        return fail(h, ASM_EINVAL, "asm_map_pairs_file: bad arguments");
    if (chunk_bytes < 0) return fail(h, ASM_EINVAL, "asm_map_pairs_file: chunk_bytes must be >= 0");
    if (const int rc = map_check_args(h, ix, "asm_map_pairs_file", "mate", {0, p, {nullptr, nullptr}, pp, nullptr, 0, 0, 0, {nullptr, 0, nullptr}}))
        return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t chunk = chunk_bytes == 0 ? (size_t)16 << 20 : (size_t)std::min<int64_t>(chunk_bytes, (int64_t)1 << 30);
    const char* const path[2] = {fastq1_path, fastq2_path};
    return map_pairs_file_run(h, ix, seq_names, path, sam_path, header, p, pp, chunk, stats);
}

size_t asm_fastq_cut_n(const char* buf, size_t nbytes, int64_t max_records, int64_t* records) {
    if (!buf) nbytes = 0;
    return asm_host::fastq_cut_n(buf, nbytes, max_records < 0 ? 0 : max_records, records);
}
