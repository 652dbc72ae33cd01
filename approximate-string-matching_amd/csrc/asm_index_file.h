// asm_index_build_file: a FASTA file in, a k-mer index out (kernels: asm_fasta.h; reader: FastaFill of asm_host.h; input pipeline:
// asm_stream.h; index stage: map_index_stage of asm_map_host.h; design: docs/design/mapper.md, "Reference: FASTA in, index out").
// The file is read at disk speed into pinned slots and copied up as it is; the device drops the line structure and writes the
// upper-cased text where the index keeps it.  asm_capi.hip includes this file inside its extern "C" block, behind asm_map_file.h.
#pragma once

extern "C++" {

#define INDEX_FILE_INLINE_HEADERS 64 /* header records that come down with the carried state, in the chunk's one download */

/* What the chunks of one call share: the index under construction, the carried state on the device, and the host's lists */
struct IndexFileJob {
    asm_handle* h;
    const char* who;
    const char* path;
    asm_index* ix;
    uint64_t text_cap;
    Scratch<FastaCarry> d_carry;
    FastaCarry carry = {};
    std::vector<FastaHeader> recs;
    int64_t chunks = 0;
    IndexFileJob(asm_handle* owner, const char* call, const char* fasta_path, asm_index* index, uint64_t cap)
        : h(owner), who(call), path(fasta_path), ix(index), text_cap(cap), d_carry(owner) {}
};

/* One file chunk: d_raw[0, nbytes) with `lines` newlines; pin: the same bytes in the pinned slot, which the host still holds */
static int index_file_chunk(IndexFileJob& j, const char* d_raw, const char* pin, size_t nbytes, int64_t lines) {
    asm_handle* h = j.h;
    const char* who = j.who;
    const size_t ntiles = (nbytes + FASTA_TILE - 1) / FASTA_TILE, cnt = ntiles + 1;
    const uint32_t hdr_cap = (uint32_t)std::min<int64_t>(lines + 1, (int64_t)MAP_MAX_SEQS); /* a header line begins a line */
    MapTmp tmp(h);
    Scratch<uint32_t> d_nl(h), d_tbase(h), d_thdr(h), d_tcand(h), d_tafter(h), d_tkept(h), d_hbase(h), d_kbase(h);
    Scratch<FastaHeader> d_hdr(h);
    STREAM_TRY(who, d_nl.alloc(sizeof(uint32_t) * ((size_t)lines + 2)));
    for (Scratch<uint32_t>* x : {&d_thdr, &d_tcand, &d_tafter, &d_tkept, &d_hbase, &d_kbase}) STREAM_TRY(who, x->alloc(sizeof(uint32_t) * cnt));
    STREAM_TRY(who, d_hdr.alloc(sizeof(FastaHeader) * (size_t)hdr_cap));
    STREAM_TRY(who, newline_index(h, tmp, d_raw, nbytes, (long)lines, d_nl.p, d_tbase));
    const FastaChunk c = {d_raw, (uint32_t)nbytes, d_nl.p, (uint32_t)lines, d_tbase.p, j.d_carry.p};
    STREAM_TRY(who, launch(h, fasta_count_kernel, (unsigned)cnt, 256, c, d_thdr.p, d_tcand.p, d_tafter.p));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_thdr.p, d_hbase.p, (int64_t)cnt));
    STREAM_TRY(who, launch(h, fasta_resolve_kernel, (unsigned)((cnt + 255) / 256), 256, (const FastaCarry*)j.d_carry.p, (const uint32_t*)d_hbase.p,
                           (const uint32_t*)d_tcand.p, (const uint32_t*)d_tafter.p, (uint32_t)cnt, d_tkept.p));
    STREAM_TRY(who, map_exclusive_sum(h, tmp, d_tkept.p, d_kbase.p, (int64_t)cnt));
    STREAM_TRY(who, launch(h, fasta_scatter_kernel, (unsigned)ntiles, 256, c, (const uint32_t*)d_hbase.p, (const uint32_t*)d_kbase.p, j.ix->d_text,
                           j.text_cap, d_hdr.p, hdr_cap));
    STREAM_TRY(who, launch(h, fasta_carry_kernel, 1u, 64u, c, (const uint32_t*)d_hbase.p + ntiles, (const uint32_t*)d_kbase.p + ntiles, j.d_carry.p));
    /* the chunk's one download: the carried state and the first header records; more only when the chunk holds more */
    const uint32_t first = std::min<uint32_t>(hdr_cap, INDEX_FILE_INLINE_HEADERS);
    j.recs.resize(first);
    STREAM_TRY(who, fetch(h, {fetched(&j.carry, (const FastaCarry*)j.d_carry.p), fetched(j.recs.data(), (const FastaHeader*)d_hdr.p, first)}));
    j.chunks++;
    if (j.carry.n_seqs >= (uint32_t)MAP_MAX_SEQS) return fail(h, ASM_EINVAL, std::string(who) + ": 2^26 sequences or more in " + j.path);
    if (!fasta_text_fits(j.carry.text_len)) return fail(h, ASM_EUNSUPPORTED, std::string(who) + ": total reference length must be below 2^32");
    const uint32_t nh = j.carry.chunk_seqs;
    j.recs.resize(nh);
    if (nh > first) STREAM_TRY(who, fetch(h, {fetched(j.recs.data() + first, (const FastaHeader*)d_hdr.p + first, nh - first)}));
    for (const FastaHeader& r : j.recs) {
        j.ix->names.emplace_back(pin + r.name, r.name_len);
        j.ix->seq_off.push_back(r.text_off);
    }
    return ASM_OK;
}

static int index_file_run(asm_handle* h, const char* path, int k, size_t chunk, asm_index** out, asm_index_file_stats* stats) {
    const char* who = "asm_index_build_file";
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    std::unique_ptr<asm_index> ix(new asm_index); /* freed after the streams below have been waited for */
    ix->device = h->device, ix->k = k;
    StreamInput in(h, who);
    size_t file_bytes = 0;
    if (const int rc = in.open_file(path, &file_bytes)) return rc;
    /* the text is no longer than the file; the index keeps this block */
    const uint64_t text_cap = std::min<uint64_t>(file_bytes, (uint64_t)1 << 32);
    STREAM_TRY(who, big_malloc(h, (void**)&ix->d_text, text_cap + 16));
    IndexFileJob j(h, who, path, ix.get(), text_cap);
    STREAM_TRY(who, j.d_carry.alloc(sizeof(FastaCarry)));
    STREAM_TRY(who, hipMemsetAsync(j.d_carry.p, 0, sizeof(FastaCarry), h->stream)); /* no text, no sequence, FASTA_FRESH */
    /* chunks ramp up from an eighth, as asm_map_file's do */
    const size_t slot_cap = chunk + chunk / 4 + 4096, first_chunk = chunk >= ((size_t)8 << 20) ? chunk / 8 : chunk;
    STREAM_TRY(who, in.open_device(slot_cap, false, true));
    in.own_pin = true;
    for (char*& q : in.pin) STREAM_TRY(who, hipHostMalloc((void**)&q, slot_cap + 64, hipHostMallocDefault));
    asm_host::ChunkSlot* slots = nullptr;
    asm_host::ChunkReader<asm_host::FastaFill> rd(chunk, first_chunk, in.wait_shipped(), in.fd, file_bytes, chunk,
                                                  [&](int q, size_t cap, size_t keep) { return in.grow_pin(slots, q, cap, keep); });
    slots = rd.slot;
    for (int q = 0; q < 3; q++) slots[q].buf = in.pin[q], slots[q].cap = slot_cap;
    rd.start();
    const char* held[2] = {nullptr, nullptr}; /* the pinned bytes of the chunk in d_raw[q] */
    int64_t accepted = 0, bytes_in = 0;
    const int rc = in.run(
        rd, std::string(who) + ": reading " + path + " failed",
        [&](const asm_host::ChunkSlot& s, int64_t) {
            if (s.bytes >= 0xfffffff0ull) return fail(h, ASM_EUNSUPPORTED, std::string(who) + ": a chunk of 4 GiB or more; lower chunk_bytes");
            held[accepted++ & 1] = s.buf;
            bytes_in += (int64_t)s.bytes;
            return (int)ASM_OK;
        },
        [&](int q, size_t bytes, int64_t units, int64_t) { return index_file_chunk(j, in.d_raw[q], held[q], bytes, units - 1); },
        /* hold_slots */ true);
    if (rc) return rc;
    rd.stop();
    if (j.carry.n_seqs == 0) return fail(h, ASM_EINVAL, std::string(who) + ": no sequence in " + path);
    ix->n_seqs = (int32_t)j.carry.n_seqs, ix->len = j.carry.text_len;
    ix->seq_off.push_back(ix->len);
    const auto t_index = std::chrono::steady_clock::now();
    STREAM_TRY(who, big_malloc(h, (void**)&ix->d_seq_off, sizeof(unsigned long long) * ix->seq_off.size()));
    STREAM_TRY(who, hipMemcpyAsync(ix->d_seq_off, ix->seq_off.data(), sizeof(uint64_t) * ix->seq_off.size(), hipMemcpyHostToDevice, h->stream));
    if (const int rs = map_index_stage(h, ix.get())) return rs;
    if (stats) {
        stats->n_seqs = ix->n_seqs, stats->bases = (int64_t)ix->len, stats->bytes_in = bytes_in, stats->chunks = j.chunks;
        stats->seconds_index = since(t_index), stats->seconds_read = rd.read_seconds(), stats->seconds = since(t_begin);
    }
    *out = ix.release();
    return ASM_OK;
}

} /* extern "C++" */

int asm_index_build_file(asm_handle* h, const char* fasta_path, int k, int64_t chunk_bytes, asm_index** out, asm_index_file_stats* stats) {
    const char* who = "asm_index_build_file";
    if (!out) return fail(h, ASM_EINVAL, std::string(who) + ": out is NULL");
    *out = nullptr;
    if (!fasta_path) return fail(h, ASM_EINVAL, std::string(who) + ": fasta_path is NULL");
    if (k < ASM_MAP_MIN_K || k > ASM_MAP_MAX_K) return fail(h, ASM_EINVAL, std::string(who) + ": k must be in [8, 14]");
    size_t chunk = 0;
    if (const int rc = map_file_chunk_bytes(h, who, chunk_bytes, &chunk)) return rc;
    if (!h) return fail(h, ASM_EINVAL, std::string(who) + ": NULL handle");
    if (stats) memset(stats, 0, sizeof *stats);
    HIPCHK(h, hipSetDevice(h->device));
    return index_file_run(h, fasta_path, k, chunk, out, stats);
}

size_t asm_fasta_cut(const char* buf, size_t nbytes, int at_line_start, int* ends_in_line) {
    if (!buf) nbytes = 0;
    return asm_host::fasta_cut(buf, nbytes, at_line_start, ends_in_line);
}
