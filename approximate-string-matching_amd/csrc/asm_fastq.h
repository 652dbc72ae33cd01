// Device-side parser of four-line FASTQ for asm_map_file (contract: docs/design/mapper.md, "Files: FASTQ in, SAM out").  The raw
// bytes of a chunk are indexed by asm_ingest.h's seq_count_kernel / seq_index_kernel (position of every newline); record i is
// lines 4i .. 4i+3 by line number alone.
//   fastq_record_kernel   one thread per record: where QNAME, SEQ and QUAL lie, whether the record is malformed, whether it is
//                         sent to the mapper (1 <= m <= 511)
//   (exclusive scans over the sent flags and the sent lengths)
//   fastq_compact_kernel  the sent records numbered as library reads: read offsets and source positions
//   seq_gather_kernel     (asm_ingest.h) the reads' bytes, one wave per read
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
