// asm_map_pairs_file: two FASTQ files in, a paired SAM file out, parsed, paired, mapped and formatted on the device (design:
// docs/design/mapper.md, "Files: two FASTQ files in, paired SAM out").  The reader keeps the two files in step (FastqPairFill,
// asm_host.h); a chunk holds the mate-1 records and then as many mate-2 records in one buffer, so the session, the newline index,
// the record kernel, the gather stage and the format tail are asm_map_file's (MapFileSession, map_file_device_chunks,
// map_file_gather, map_file_format<true>); the mapper's stages are asm_map_pairs' (map_pairs_front_seed) and the finish stage
// stays on the device (map_finish_device).  Here: the second file, the pairing kernels' chunk function and the ends of the files.
// asm_capi.hip includes this file inside its extern "C" block, behind asm_map_file.h.
#pragma once

extern "C++" {

struct MapPairsFileJob : MapFileJob {
    const asm_pair_params* pp;
    asm_map_pairs_file_stats st = {};
};

/* Pairs [r0, r0 + rn) of a file chunk of R pairs (record r of d_raw is mate 1 of pair r, record R + r its mate 2; d_nl: the 8 R
 * newline positions): one device chunk, from the record kernel to the writer's queue.  first_record: the files' records before r0. */
static int map_pairs_file_chunk(MapPairsFileJob& j, const char* d_raw, const uint32_t* d_nl, int64_t R, int64_t r0, int64_t rn,
                                int64_t first_record) {
    MapFileSession& ss = j.ss;
    asm_handle* h = ss.h;
    const char* who = ss.who;
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
    STREAM_TRY(who, d_recs.alloc(sizeof(SamRec) * 2 * (size_t)rn));
    for (Scratch<uint32_t>* x : {&d_send1, &d_send2, &d_mlen1, &d_mlen2, &d_psend, &d_len1, &d_len2, &d_rd, &d_mo1, &d_mo2})
        STREAM_TRY(who, x->alloc(sizeof(uint32_t) * cnt));
    STREAM_TRY(who, d_rec_read.alloc(sizeof(int32_t) * (size_t)rn));
    STREAM_TRY(who, d_counts.alloc(sizeof(FastqCounts) * 2));
    STREAM_TRY(who, d_pcounts.alloc(sizeof(FastqPairCounts)));
    /* bad_min and name_min start as FASTQ_NO_RECORD; the record kernel's too_long counts are not read here (unsent covers them) */
    STREAM_TRY(who, hipMemsetAsync(d_counts.p, 0xff, sizeof(FastqCounts) * 2, h->stream));
    STREAM_TRY(who, hipMemsetAsync(&d_pcounts.p->name_min, 0xff, sizeof(uint32_t), h->stream));
    STREAM_TRY(who, hipMemsetAsync(&d_pcounts.p->unsent, 0, sizeof(uint32_t), h->stream));
    STREAM_TRY(who, launch(h, fastq_record_kernel, grid_for(rn + 1), ASM_BLOCK, d_raw, d_nl, (long)r0, (long)rn, (uint32_t)ASM_MAP_MAX_READ,
                           d_recs.p, d_send1.p, d_mlen1.p, d_counts.p));
    STREAM_TRY(who, launch(h, fastq_record_kernel, grid_for(rn + 1), ASM_BLOCK, d_raw, d_nl, (long)(R + r0), (long)rn,
                           (uint32_t)ASM_MAP_MAX_READ, d_recs.p + rn, d_send2.p, d_mlen2.p, d_counts.p + 1));
    STREAM_TRY(who, launch(h, fastq_pair_kernel, grid_for(rn + 1), ASM_BLOCK, d_raw, (const SamRec*)d_recs.p, (long)rn,
                           (const uint32_t*)d_send1.p, (const uint32_t*)d_send2.p, (const uint32_t*)d_mlen1.p, (const uint32_t*)d_mlen2.p,
                           d_psend.p, d_len1.p, d_len2.p, d_pcounts.p));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_psend.p, d_rd.p, (int64_t)cnt));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_len1.p, d_mo1.p, (int64_t)cnt));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_len2.p, d_mo2.p, (int64_t)cnt));
    uint32_t tot[3] = {0, 0, 0};
    FastqCounts counts[2] = {{FASTQ_NO_RECORD, 0u}, {FASTQ_NO_RECORD, 0u}};
    FastqPairCounts pcounts = {FASTQ_NO_RECORD, 0u};
    STREAM_TRY(who, fetch(h, {fetched(&tot[0], d_rd.p + rn), fetched(&tot[1], d_mo1.p + rn), fetched(&tot[2], d_mo2.p + rn),
                              fetched(counts, d_counts.p, 2), fetched(&pcounts, d_pcounts.p)}));
    for (int f = 0; f < 2; f++)
        if (counts[f].bad_min != FASTQ_NO_RECORD) return map_file_malformed(ss, first_record + counts[f].bad_min + 1, f + 1);
    if (const int rc = map_file_bam_names<true>(ss, d_raw, d_recs.p, rn, first_record)) return rc;
    if (pcounts.name_min != FASTQ_NO_RECORD)
        return ss.bad("the mates of record " + std::to_string(first_record + pcounts.name_min + 1) +
                      " have different names (QNAME is the first word without a trailing /1 or /2)");
    const int64_t ns = tot[0]; /* sent pairs: library reads [0, ns) are their mates 1, [ns, 2 ns) their mates 2 */
    MapPairFront pf(h);
    MapFront& f = pf.f;
    MapFinish fin(h);
    if (const int rc = map_file_gather(ss, d_raw, 2 * ns, (size_t)tot[1] + tot[2], f, [&](unsigned long long* d_start) {
            return launch(h, fastq_pair_compact_kernel, grid_for(rn + 1), ASM_BLOCK, (const SamRec*)d_recs.p, (const uint32_t*)d_psend.p,
                          (const uint32_t*)d_rd.p, (const uint32_t*)d_mo1.p, (const uint32_t*)d_mo2.p, (long)rn, d_rec_read.p, f.d_roff.p,
                          d_start);
        }))
        return rc;
    if (ns > 0) {
        /* map: asm_map_pairs' stages on reads that are in HBM already; records, ops, nops and the pair state stay there */
        if (const int rc = map_pairs_front_seed(h, ix, ns, p, j.pp, who, pf)) return rc;
        if (const int rc = map_finish_launch(h, ix, p, f, 2 * ns, pf.d_ikey.p, nullptr, nullptr, f.bytes + 2 * (size_t)ns, SAM_CIGAR_CAP, fin))
            return rc;
        if (const int rc = map_finish_device(h, ix, p, f, fin)) return rc;
    }
    /* format: line 2q + x is mate x of pair q */
    SamArgs a = {};
    a.raw = d_raw, a.recs = d_recs.p, a.rec_read = d_rec_read.p, a.nrec = (long)rn, a.nlines = (long)(2 * rn);
    a.hits = fin.d_hits.p, a.ops = fin.d_ops.p, a.nops = fin.d_nops.p, a.mapq = pf.d_mapq.p;
    a.md = fin.d_md.p, a.md_len = fin.d_md_len.p;
    a.pair_state = pf.d_state.p, a.n_conc = pf.d_nconc.p, a.n_sent = (long)ns;
    unsigned long long n[3] = {0, 0, 0}; /* mapped, proper, rescued */
    if (const int rc = map_file_format<true>(ss, tmp, a, n)) return rc;
    j.st.pairs += rn, j.st.proper += (int64_t)n[1], j.st.rescued += (int64_t)n[2], j.st.unsent += pcounts.unsent;
    return ASM_OK;
}

/* sort_cap: NULL for asm_map_pairs_file, max_device_bytes for asm_map_pairs_file_sorted */
static int map_pairs_file_run(asm_handle* h, const char* who, const asm_index* ix, const char* const* seq_names, const char* const path[2],
                              const char* sam_path, const char* header, const asm_map_params* p, const asm_pair_params* pp, size_t chunk,
                              asm_map_pairs_file_stats* stats, const int64_t* sort_cap, asm_sam_sort_stats* sort_stats) {
    MapFileSession ss(h, who, chunk);
    if (sort_cap) ss.sort.reset(new SamSortHold(h, who, ix->n_seqs, (size_t)*sort_cap));
    StreamInput& in = ss.in;
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
    if (second.fd < 0 || fstat(second.fd, &st2) != 0) return ss.bad(std::string("cannot open ") + path[1]);
    file_bytes[1] = (size_t)st2.st_size;
    const int fds[2] = {in.fd, second.fd};
    if (const int rc = ss.open(ix, seq_names, 2, fds, file_bytes, path, sam_path, header)) return rc;
    asm_host::ChunkReader<asm_host::FastqPairFill> rd(chunk, ss.first_chunk, in.wait_shipped(), fds[0], fds[1], file_bytes[0], file_bytes[1],
                                                      chunk, ss.grow());
    MapPairsFileJob j = {{ss, ix, p}, pp};
    const int rc = ss.run(
        rd, std::string(who) + ": reading " + path[0] + " or " + path[1] + " failed",
        [](const asm_host::ChunkSlot&, int64_t) { return (int)ASM_OK; },
        [&](int q, size_t bytes, int64_t R, int64_t first_record) {
            return map_file_device_chunks(ss, in.d_raw[q], bytes, 8 * R, R, map_pair_step(h), [&](const uint32_t* d_nl, int64_t r0, int64_t rn) {
                return map_pairs_file_chunk(j, in.d_raw[q], d_nl, R, r0, rn, first_record + r0);
            });
        });
    if (rc) return rc;
    /* the ends of the two files, after every pair in front of them has been looked at */
    const asm_host::FastqPairFill& end = rd.policy();
    for (int f = 0; f < 2; f++)
        if (end.extra_lines[f])
            return ss.bad("record " + std::to_string(end.records[f] + 1) + " of file " + std::to_string(f + 1) +
                          " is truncated (the file's line count is not a multiple of 4)");
    for (int f = 0; f < 2; f++)
        if (end.more[f])
            return ss.bad("record " + std::to_string(end.records[1 - f] + 1) + " of file " + std::to_string(f + 1) +
                          " has no mate (the two files hold different numbers of records)");
    if (const int rf = ss.finish(j.st)) return rf;
    j.st.carry_peak = (int64_t)end.carry_peak;
    if (stats) *stats = j.st;
    if (sort_stats && ss.sort) *sort_stats = ss.sort->st;
    return ASM_OK;
}

/* asm_map_pairs_file and asm_map_pairs_file_sorted (`who`): the argument checks, then the call */
static int map_pairs_file_call(const char* who, asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq1_path,
                               const char* fastq2_path, const char* sam_path, const char* header, const asm_map_params* p,
                               const asm_pair_params* pp, int64_t chunk_bytes, asm_map_pairs_file_stats* stats, const int64_t* sort_cap,
                               asm_sam_sort_stats* sort_stats) {
    if (!p || !pp || !ix || !seq_names || !fastq1_path || !fastq2_path || !sam_path)
        return fail(h, ASM_EINVAL, std::string(who) + ": bad arguments");
    size_t chunk = 0;
    if (const int rc = map_file_chunk_bytes(h, who, chunk_bytes, &chunk)) return rc;
    if (const int rc = map_file_sort_cap(h, who, sort_cap)) return rc;
    if (const int rc = map_check_args(h, ix, who, "mate", {0, p, {nullptr, nullptr}, pp, nullptr, 0, 0, 0, {nullptr, 0, nullptr}})) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (sort_stats) memset(sort_stats, 0, sizeof *sort_stats);
    HIPCHK(h, hipSetDevice(h->device));
    const char* const path[2] = {fastq1_path, fastq2_path};
    return map_pairs_file_run(h, who, ix, seq_names, path, sam_path, header, p, pp, chunk, stats, sort_cap, sort_stats);
}

} /* extern "C++" */

int asm_map_pairs_file(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq1_path, const char* fastq2_path,
                       const char* sam_path, const char* header, const asm_map_params* p, const asm_pair_params* pp, int64_t chunk_bytes,
                       asm_map_pairs_file_stats* stats) {
    return map_pairs_file_call("asm_map_pairs_file", h, ix, seq_names, fastq1_path, fastq2_path, sam_path, header, p, pp, chunk_bytes, stats,
                               nullptr, nullptr);
}

int asm_map_pairs_file_sorted(asm_handle* h, const asm_index* ix, const char* const* seq_names, const char* fastq1_path,
                              const char* fastq2_path, const char* sam_path, const char* header, const asm_map_params* p,
                              const asm_pair_params* pp, int64_t chunk_bytes, int64_t max_device_bytes, asm_map_pairs_file_stats* stats,
                              asm_sam_sort_stats* sort_stats) {
    return map_pairs_file_call("asm_map_pairs_file_sorted", h, ix, seq_names, fastq1_path, fastq2_path, sam_path, header, p, pp,
                               chunk_bytes, stats, &max_device_bytes, sort_stats);
}

size_t asm_fastq_cut_n(const char* buf, size_t nbytes, int64_t max_records, int64_t* records) {
    if (!buf) nbytes = 0;
    return asm_host::fastq_cut_n(buf, nbytes, max_records < 0 ? 0 : max_records, records);
}
