// Device-side parser of four-line FASTQ for asm_map_file (contract: docs/design/mapper.md, "Files: FASTQ in, SAM out").  The raw
// bytes of a chunk are indexed by asm_ingest.h's seq_count_kernel / seq_index_kernel (position of every newline); record i is
// lines 4i .. 4i+3 by line number alone.
//   fastq_record_kernel   one thread per record: where QNAME, SEQ and QUAL lie, whether the record is malformed, whether it is
//                         sent to the mapper (1 <= m <= 511)
//   (exclusive scans over the sent flags and the sent lengths)
//   fastq_compact_kernel  the sent records numbered as library reads: read offsets and source positions
//   text_gather_kernel    (asm_ingest.h) the reads' bytes, one wave per read
// Two files in step (asm_map_pairs_file): the chunk holds the mate-1 records and then as many mate-2 records, fastq_record_kernel
// runs over each half, and
//   fastq_pair_kernel          one thread per pair: sent when both mates are, the two QNAMEs compared without /1 and /2
//   (exclusive scans over the sent flags and over each mate's sent lengths)
//   fastq_pair_compact_kernel  mate 1 of sent pair q = library read q, mate 2 = read ns + q: read offsets and source positions
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "asm_bits.h"
#include "asm_sam.h"

#define FASTQ_NO_RECORD 0xffffffffu

struct FastqCounts {
    uint32_t bad_min;  /* smallest malformed record of the range, FASTQ_NO_RECORD: none */
    uint32_t too_long; /* records longer than max_read */
};

/* records [first, first + n) of the chunk; nl = the chunk's newline positions (4 per record); every read of raw is at a position
 * below a newline's, so inside the chunk */
__global__ __launch_bounds__(256) void fastq_record_kernel(const char* __restrict__ raw, const uint32_t* __restrict__ nl, long first,
                                                           long n, uint32_t max_read, SamRec* __restrict__ recs,
                                                           uint32_t* __restrict__ send, uint32_t* __restrict__ mlen,
                                                           FastqCounts* __restrict__ counts) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { /* so that the exclusive scans over n + 1 entries yield the totals */
        send[n] = 0u, mlen[n] = 0u;
        return;
    }
    const long r = first + i;
    uint32_t b[4], e[4]; /* the four lines, CR stripped */
#pragma unroll
    for (int q = 0; q < 4; q++) {
        b[q] = (r == 0 && q == 0) ? 0u : nl[4 * r + q - 1] + 1u;
        e[q] = nl[4 * r + q];
        if (e[q] > b[q] && raw[e[q] - 1u] == '\r') e[q]--;
    }
    const bool bad = e[0] == b[0] || raw[b[0]] != '@' || e[2] == b[2] || raw[b[2]] != '+';
    SamRec rec;
    uint32_t a = bad ? e[0] : b[0] + 1u;
    while (a < e[0] && (raw[a] == ' ' || raw[a] == '\t')) a++;
    uint32_t z = a;
    while (z < e[0] && raw[z] != ' ' && raw[z] != '\t') z++;
    rec.name = a, rec.name_len = z - a;
    rec.seq = b[1], rec.seq_len = e[1] - b[1];
    rec.qual = b[3], rec.qual_len = e[3] - b[3];
    recs[i] = rec;
    const bool sent = rec.seq_len >= 1u && rec.seq_len <= max_read;
    send[i] = sent ? 1u : 0u;
    mlen[i] = sent ? rec.seq_len : 0u;
    if (bad) atomicMin(&counts->bad_min, (uint32_t)i);
    const unsigned long long lm = __ballot(rec.seq_len > max_read);
    if ((threadIdx.x & 63) == 0 && lm) atomicAdd(&counts->too_long, (uint32_t)__popcll(lm));
}

/* rd = exclusive scan of send, mo = exclusive scan of mlen (n + 1 entries each; entry n = the totals) */
__global__ __launch_bounds__(256) void fastq_compact_kernel(const SamRec* __restrict__ recs, const uint32_t* __restrict__ send,
                                                            const uint32_t* __restrict__ rd, const uint32_t* __restrict__ mo, long n,
                                                            int32_t* __restrict__ rec_read, uint32_t* __restrict__ roff,
                                                            unsigned long long* __restrict__ start) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        roff[rd[n]] = mo[n];
        return;
    }
    const bool sent = send[i] != 0u;
    rec_read[i] = sent ? (int32_t)rd[i] : -1;
    if (sent) roff[rd[i]] = mo[i], start[rd[i]] = recs[i].seq;
}

struct FastqPairCounts {
    uint32_t name_min; /* smallest pair of the range whose mates' names differ, FASTQ_NO_RECORD: none */
    uint32_t unsent;   /* pairs with an empty or too long mate */
};

/* pairs [0, n) of a device chunk: recs = [2][n] (mate 1 of every pair, then mate 2), send1 / send2 and mlen1 / mlen2 what
 * fastq_record_kernel left for the two halves (n + 1 entries each).  psend, len1 and len2 get n + 1 entries, the last 0. */
__global__ __launch_bounds__(256) void fastq_pair_kernel(const char* __restrict__ raw, const SamRec* __restrict__ recs, long n,
                                                         const uint32_t* __restrict__ send1, const uint32_t* __restrict__ send2,
                                                         const uint32_t* __restrict__ mlen1, const uint32_t* __restrict__ mlen2,
                                                         uint32_t* __restrict__ psend, uint32_t* __restrict__ len1,
                                                         uint32_t* __restrict__ len2, FastqPairCounts* __restrict__ counts) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool unsent = false;
    if (i == n) psend[n] = 0u, len1[n] = 0u, len2[n] = 0u;
    if (i < n) {
        const SamRec a = recs[i], b = recs[n + i];
        const bool sent = send1[i] != 0u && send2[i] != 0u;
        psend[i] = sent ? 1u : 0u;
        len1[i] = sent ? mlen1[i] : 0u;
        len2[i] = sent ? mlen2[i] : 0u;
        unsent = !sent;
        const uint32_t la = sam_pair_name_len(raw, a), lb = sam_pair_name_len(raw, b);
        bool same = la == lb;
        for (uint32_t t = 0; same && t < la; t++) same = raw[a.name + t] == raw[b.name + t];
        if (!same) atomicMin(&counts->name_min, (uint32_t)i);
    }
    const unsigned long long um = __ballot(unsent);
    if ((threadIdx.x & 63) == 0 && um) atomicAdd(&counts->unsent, (uint32_t)__popcll(um));
}

/* rd = exclusive scan of psend, mo1 / mo2 = exclusive scans of len1 / len2 (n + 1 entries each; entry n = the totals): the reads of
 * the chunk's ns sent pairs in map_pairs_front's layout, the mates 1 and then the mates 2 */
__global__ __launch_bounds__(256) void fastq_pair_compact_kernel(const SamRec* __restrict__ recs, const uint32_t* __restrict__ psend,
                                                                 const uint32_t* __restrict__ rd, const uint32_t* __restrict__ mo1,
                                                                 const uint32_t* __restrict__ mo2, long n, int32_t* __restrict__ rec_read,
                                                                 uint32_t* __restrict__ roff, unsigned long long* __restrict__ start) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const uint32_t ns = rd[n], bytes1 = mo1[n];
    if (i == n) {
        roff[2u * ns] = bytes1 + mo2[n];
        return;
    }
    const bool sent = psend[i] != 0u;
    rec_read[i] = sent ? (int32_t)rd[i] : -1;
    if (sent) {
        roff[rd[i]] = mo1[i], start[rd[i]] = recs[i].seq;
        roff[ns + rd[i]] = bytes1 + mo2[i], start[ns + rd[i]] = recs[n + i].seq;
    }
}
