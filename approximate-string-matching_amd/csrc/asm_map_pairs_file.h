// asm_map_pairs_file: two FASTQ files in, a paired SAM file out, parsed, paired, mapped and formatted on the device (design:
// docs/design/mapper.md, "Files: two FASTQ files in, paired SAM out").  The reader keeps the two files in step (FastqPairFill,
// asm_host.h); a chunk holds the mate-1 records and then as many mate-2 records in one buffer, so the session, the newline index,
// the record kernel, the gather stage and the format tail are asm_map_file's (MapFileSession, map_file_device_chunks,
// map_file_gather, map_file_format<true>); the mapper's stages are asm_map_pairs' (map_pairs_front_seed) and the finish stage
// stays on the device (map_finish_device).  Here: the second file, the pairing kernels' chunk function and the ends of the files;
// and the same call on two BGZF-compressed files (BgzfPairFill, asm_host.h; pair_cut_kernel and pair_move_kernel here), which puts
// the same chunk in front of the same chunk function.
// asm_capi.hip includes this file inside its extern "C" block, behind asm_map_file.h.
#pragma once

extern "C++" {

#include "asm_pair_cut.h"

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

/* ---- two BGZF-compressed FASTQ files (docs/design/mapper.md, "Compressed input for pairs") ---------------------------------------- */
/* One wavefront, behind seq_count_kernel over both texts and one exclusive sum of their tile counts laid back to back (tile_base[0 ..
 * ntiles1] text 1's, tile_base[ntiles1 .. ntiles1 + ntiles2] text 2's): the pair cut (pair_cut_plan, asm_pair_cut.h) and the byte
 * behind newline 4 R - 1 of each text (seq_behind_newline).  last: the text reaches its file's end, so one that does not end in a
 * newline gets one at text[nbytes] (the buffers have room). */
__global__ __launch_bounds__(64) void pair_cut_kernel(char* __restrict__ text1, char* __restrict__ text2, unsigned long long nbytes1,
                                                      unsigned long long nbytes2, const uint32_t* __restrict__ tile_base, uint32_t ntiles1,
                                                      uint32_t ntiles2, int last1, int last2, PairCutOut* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    char* const text[2] = {text1, text2};
    const uint32_t* const tb[2] = {tile_base, tile_base + ntiles1};
    const uint32_t ntiles[2] = {ntiles1, ntiles2};
    const int last[2] = {last1, last2};
    PairCutText t[2] = {{0ull, nbytes1, 0u, 0u}, {0ull, nbytes2, 0u, 0u}};
#pragma unroll
    for (int x = 0; x < 2; x++) {
        t[x].counted = ntiles[x] ? (unsigned long long)(tb[x][ntiles[x]] - tb[x][0]) : 0ull;
        t[x].open_end = last[x] && t[x].nbytes > 0 && text[x][t[x].nbytes - 1] != '\n' ? 1u : 0u;
    }
    PairCutOut o;
    uint32_t how[2];
    pair_cut_plan(t, &o, how);
#pragma unroll
    for (int x = 0; x < 2; x++)
        if (how[x] == PAIR_CUT_FIND) o.f[x].cut = seq_behind_newline(text[x], t[x].nbytes, tb[x], ntiles[x], (uint32_t)(4u * o.pairs - 1u), lane);
    if (lane == 0u) {
#pragma unroll
        for (int x = 0; x < 2; x++)
            if (o.f[x].appended) text[x][t[x].nbytes] = '\n';
        *out = o;
    }
}

/* dst[0, n) = src[0, n) for ranges that do not overlap: file 2's records to behind file 1's.  16-byte stores on dst's own 16-byte
 * grid (dst starts anywhere: file 1's cut), the loads as the offset between the two allows; the bytes in front of the grid and behind
 * its last whole group one by one. */
__global__ __launch_bounds__(256) void pair_move_kernel(char* __restrict__ dst, const char* __restrict__ src, unsigned long long n) {
    const unsigned long long lead = (16u - (unsigned long long)((uintptr_t)dst & 15u)) & 15u, head = lead < n ? lead : n;
    const unsigned long long groups = (n - head) / 16u, tail = head + 16u * groups;
    const unsigned long long tid = (unsigned long long)blockIdx.x * 256u + threadIdx.x, stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long g = tid; g < groups; g += stride) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16u * g, 16);
        *reinterpret_cast<uint4*>(dst + head + 16u * g) = v;
    }
    if (tid < head) dst[tid] = src[tid];
    if (tid < n - tail) dst[tail + tid] = src[tail + tid];
}

/* The device side of two BGZF inputs: per file, the text behind a chunk's last whole pair stays in a carry on the device and leads
 * that file's text in the next chunk (BgzfInput's carry, twice). */
struct BgzfPairInput {
    asm_handle* h;
    Scratch<char> carry1, carry2;
    Scratch<char>* const carry[2] = {&carry1, &carry2};
    size_t carry_len[2] = {0, 0}, carry_cap[2] = {0, 0}, carry_peak = 0;
    int64_t pairs_seen = 0, chunk_no = 0;
    asm_host::BgzfPairChunkInfo pend[2]; /* what the reader said of the chunks in flight, by device buffer */
    size_t pend_bytes1[2] = {0, 0};
    explicit BgzfPairInput(asm_handle* owner) : h(owner), carry1(owner), carry2(owner) {}
};
static int map_pairs_file_member_error(MapFileSession& ss, int file, size_t member, size_t offset, const char* what) {
    return ss.bad("file " + std::to_string(file) + ": BGZF member " + std::to_string(member) + " at offset " + std::to_string(offset) + ": " + what);
}
static int map_pairs_file_truncated(MapFileSession& ss, int64_t record, int file) {
    return map_file_bad_record(ss, record, file, " is truncated (the file's line count is not a multiple of 4)");
}
static int map_pairs_file_no_mate(MapFileSession& ss, int64_t record, int file) {
    return map_file_bad_record(ss, record, file, " has no mate (the two files hold different numbers of records)");
}

/* One file chunk of compressed members in d_src, file 1's in front of file 2's (bytes1): each file's members inflated behind its carry
 * into a text of its own in one launch, both counted, the pair cut (one wait: the cut and the first failed member), file 2's records moved to
 * behind file 1's, and that chunk handed to map_file_device_chunks / map_pairs_file_chunk as a plain one is; what lies behind the two
 * cuts are the next carries, and the policy hears of their lengths.  Behind the pairs of the chunk that shows them, the ends of the files. */
static int map_pairs_file_gz_chunk(MapPairsFileJob& j, BgzfPairInput& gz, asm_host::BgzfPairFill& fill, const char* d_src,
                                   const asm_host::BgzfPairChunkInfo& pi, size_t bytes1) {
    MapFileSession& ss = j.ss;
    asm_handle* h = ss.h;
    const char* who = ss.who;
    typedef unsigned long long u64;
    const size_t nb[2] = {gz.carry_len[0] + pi.f[0].text, gz.carry_len[1] + pi.f[1].text};
    if (nb[0] + nb[1] >= 0xfffffff0ull) return ss.bad("a chunk of 4 GiB or more of text; lower chunk_bytes", ASM_EUNSUPPORTED);
    /* d_text: [text 1][room for text 2's records behind text 1's cut][text 2], so that the move never overlaps its source */
    const size_t room[2] = {(nb[0] + 64 + 15) & ~(size_t)15, (nb[1] + 64 + 15) & ~(size_t)15}, off2 = room[0] + room[1];
    const size_t nm[2] = {pi.f[0].members.size(), pi.f[1].members.size()};
    const uint32_t ntiles[2] = {(uint32_t)((nb[0] + SEQ_TILE - 1) / SEQ_TILE), (uint32_t)((nb[1] + SEQ_TILE - 1) / SEQ_TILE)};
    const size_t nt = (size_t)ntiles[0] + ntiles[1];
    Scratch<char> d_text(h);
    Scratch<InfMember> d_members(h);
    Scratch<u64> d_bad(h);
    Scratch<PairCutOut> d_cut(h);
    Scratch<uint32_t> d_tile(h), d_tbase(h);
    MapTmp tmp(h);
    STREAM_TRY(who, d_text.alloc(off2 + room[1]));
    STREAM_TRY(who, d_members.alloc(sizeof(InfMember) * (nm[0] + nm[1] + 1)));
    STREAM_TRY(who, d_bad.alloc(sizeof(u64)));
    STREAM_TRY(who, d_cut.alloc(sizeof(PairCutOut)));
    STREAM_TRY(who, d_tile.alloc(sizeof(uint32_t) * (nt + 1)));
    STREAM_TRY(who, d_tbase.alloc(sizeof(uint32_t) * (nt + 1)));
    char* const text[2] = {d_text.p, d_text.p + off2};
    STREAM_TRY(who, hipMemsetAsync(d_tile.p, 0, sizeof(uint32_t) * (nt + 1), h->stream));
    /* one launch over both member tables, file 1's in front: a launch lasts as long as its slowest member, so two would take twice
     * as long; file 2's output offsets are moved to its text, and the smallest failed index is the error the contract names */
    std::vector<InfMember> members(pi.f[0].members);
    members.insert(members.end(), pi.f[1].members.begin(), pi.f[1].members.end());
    for (size_t k = nm[0]; k < members.size(); k++) members[k].out_off += (u64)(off2 + gz.carry_len[1] - gz.carry_len[0]);
    if (!members.empty())
        STREAM_TRY(who, hipMemcpyAsync(d_members.p, members.data(), sizeof(InfMember) * members.size(), hipMemcpyHostToDevice, h->stream));
    for (int x = 0; x < 2; x++)
        if (gz.carry_len[x]) STREAM_TRY(who, hipMemcpyAsync(text[x], gz.carry[x]->p, gz.carry_len[x], hipMemcpyDeviceToDevice, h->stream));
    STREAM_TRY(who, bgzf_inflate_device(h, (const uint8_t*)d_src, d_members.p, members.size(), (uint8_t*)text[0] + gz.carry_len[0], d_bad.p));
    for (int x = 0; x < 2; x++)
        if (ntiles[x])
            STREAM_TRY(who, launch(h, seq_count_kernel, ntiles[x], 256, (const char*)text[x], (long)nb[x], d_tile.p + (x ? ntiles[0] : 0u)));
    if (nt) STREAM_TRY(who, map_exclusive_sum(h, tmp, d_tile.p, d_tbase.p, (int64_t)nt + 1));
    STREAM_TRY(who, launch(h, pair_cut_kernel, 1u, 64u, text[0], text[1], (u64)nb[0], (u64)nb[1], (const uint32_t*)d_tbase.p, ntiles[0], ntiles[1],
                           pi.done[0] ? 1 : 0, pi.done[1] ? 1 : 0, d_cut.p));
    u64 bad = INF_NONE_BAD;
    PairCutOut cut = {};
    STREAM_TRY(who, fetch(h, {fetched(&cut, (const PairCutOut*)d_cut.p), fetched(&bad, (const u64*)d_bad.p)}));
    for (int x = 0; x < 2; x++) { /* file 1's failed member, its bad header, then file 2's */
        const asm_host::BgzfChunkInfo& ci = pi.f[x];
        const size_t k = (size_t)(bad >> 8) - (x ? nm[0] : 0);
        if (bad != INF_NONE_BAD && (x == 1 || (size_t)(bad >> 8) < nm[0]))
            return map_pairs_file_member_error(ss, x + 1, (size_t)ci.first_member + k, ci.file_base + (size_t)ci.members[k].src_off - (x ? bytes1 : 0),
                                               inf_status_text((uint32_t)(bad & 0xffu)));
        if (ci.err.status != BGZF_IN_OK) return map_pairs_file_member_error(ss, x + 1, ci.err.member, ci.err.offset, bgzf_in_text(ci.err.status));
    }
    const int64_t R = (int64_t)cut.pairs, first_record = gz.pairs_seen;
    size_t rest[2];
    bool end = pi.done[0] && pi.done[1]; /* the files' ends are looked at behind this chunk's pairs */
    for (int x = 0; x < 2; x++) {
        rest[x] = nb[x] + cut.f[x].appended - (size_t)cut.f[x].cut;
        if (pi.done[x] && !cut.f[x].more && cut.f[1 - x].more) end = true; /* file x holds no further record and its mate's file does */
    }
    gz.pairs_seen += R;
    fill.feedback(gz.chunk_no++, rest[0], rest[1], gz.pairs_seen);
    if (!end && rest[0] + rest[1] > gz.carry_peak) gz.carry_peak = rest[0] + rest[1];
    /* the carries leave first: file 2's records move onto what lies behind file 1's cut */
    for (int x = 0; x < 2 && !end; x++) {
        if (rest[x] > gz.carry_cap[x]) { /* the old carry has been copied into its text, in stream order */
            pool_free(h, gz.carry[x]->p);
            gz.carry[x]->p = nullptr, gz.carry_cap[x] = 0;
            STREAM_TRY(who, gz.carry[x]->alloc(rest[x] + rest[x] / 2 + 65536));
            gz.carry_cap[x] = rest[x] + rest[x] / 2 + 65536;
        }
        if (rest[x]) STREAM_TRY(who, hipMemcpyAsync(gz.carry[x]->p, text[x] + cut.f[x].cut, rest[x], hipMemcpyDeviceToDevice, h->stream));
        gz.carry_len[x] = rest[x];
    }
    if (R > 0) {
        const u64 n2 = cut.f[1].cut, groups = n2 / 16u + 1u;
        STREAM_TRY(who, launch(h, pair_move_kernel, (unsigned)std::min<u64>((groups + 255u) / 256u, 2048u), 256u, d_text.p + cut.f[0].cut,
                               (const char*)text[1], n2));
        const char* d_raw = d_text.p;
        if (const int rc = map_file_device_chunks(ss, d_raw, (size_t)(cut.f[0].cut + cut.f[1].cut), 8 * R, R, map_pair_step(h),
                                                  [&](const uint32_t* d_nl, int64_t r0, int64_t rn) {
                                                      return map_pairs_file_chunk(j, d_raw, d_nl, R, r0, rn, first_record + r0);
                                                  }))
            return rc;
    }
    if (!end) return ASM_OK;
    /* the ends of the two files, as the plain call words them */
    for (int x = 0; x < 2; x++)
        if (pi.done[x] && cut.f[x].extra_lines) return map_pairs_file_truncated(ss, first_record + (int64_t)(cut.f[x].lines / 4u) + 1, x + 1);
    for (int x = 0; x < 2; x++)
        if (cut.f[x].more) return map_pairs_file_no_mate(ss, first_record + (int64_t)(cut.f[1 - x].lines / 4u) + 1, x + 1);
    return ASM_OK;
}

/* map_pairs_file_run for two files that start with BGZF members */
static int map_pairs_file_run_gz(MapFileSession& ss, MapPairsFileJob& j, const char* const path[2], const int fds[2], const size_t file_bytes[2]) {
    StreamInput& in = ss.in;
    BgzfPairInput gz(ss.h);
    asm_host::ChunkReader<asm_host::BgzfPairFill> rd(ss.chunk, ss.first_chunk, in.wait_shipped(), fds[0], fds[1], file_bytes[0], file_bytes[1],
                                                     ss.grow());
    /* info[q] is read while the reader runs: slot q's hand-over orders it, as in map_file_run_gz */
    asm_host::BgzfPairFill& fill = rd.policy();
    ss.text_bytes = [&](const asm_host::ChunkSlot& s) { return fill.info[&s - rd.slot].f[0].text + fill.info[&s - rd.slot].f[1].text; };
    int c = 0;
    const int rc = ss.run(
        rd, std::string(ss.who) + ": reading " + path[0] + " or " + path[1] + " failed",
        [&](const asm_host::ChunkSlot& s, int64_t) {
            gz.pend[c & 1] = fill.info[&s - rd.slot], gz.pend_bytes1[c & 1] = s.bytes1;
            c++;
            return (int)ASM_OK;
        },
        [&](int q, size_t, int64_t, int64_t) { return map_pairs_file_gz_chunk(j, gz, fill, in.d_raw[q], gz.pend[q], gz.pend_bytes1[q]); });
    rd.stop();
    ss.text_bytes = nullptr; /* it refers to the reader, which ends here */
    j.st.carry_peak = (int64_t)gz.carry_peak;
    return rc;
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
    /* the first bytes of each file: BGZF members (the compressed path), plain gzip (refused), or text, which goes on as before */
    bool gzip[2] = {false, false};
    for (int f = 0; f < 2; f++)
        if (const int rc = map_file_probe(ss, fds[f], file_bytes[f], path[f], &gzip[f])) return rc;
    for (int f = 0; f < 2; f++)
        if (gzip[f] && !gzip[1 - f] && file_bytes[1 - f] > 0)
            return ss.bad("file " + std::to_string(f + 1) + " (" + path[f] + ") is BGZF and file " + std::to_string(2 - f) + " (" + path[1 - f] +
                              ") is plain text: both files must be of one kind",
                          ASM_EUNSUPPORTED);
    if (const int rc = ss.open(ix, seq_names, 2, fds, file_bytes, path, sam_path, header)) return rc;
    if (gzip[0] || gzip[1]) {
        MapPairsFileJob jz = {{ss, ix, p}, pp};
        if (const int rc = map_pairs_file_run_gz(ss, jz, path, fds, file_bytes)) {
            if (stats) stats->carry_peak = jz.st.carry_peak; /* what a failed call held: the one field it leaves behind */
            return rc;
        }
        if (const int rf = ss.finish(jz.st)) return rf;
        if (stats) *stats = jz.st;
        if (sort_stats && ss.sort) *sort_stats = ss.sort->st;
        return ASM_OK;
    }
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
    if (const int rc = map_file_index_check(h, who, ix, seq_names, sort_cap)) return rc;
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
