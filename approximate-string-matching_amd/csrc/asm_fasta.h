// Device-side FASTA parser of asm_index_build_file (contract: docs/design/mapper.md, "Reference: FASTA in, index out").  A chunk of
// the file lies in HBM as it was read; it may begin and end anywhere except inside a header line.  The work is byte-parallel: a
// thread takes FASTA_GROUP consecutive bytes, no thread owns a line, and what a thread does never depends on a line's length.
//   seq_count_kernel / seq_index_kernel  (asm_ingest.h) the position of every newline of the chunk
//   fasta_count_kernel    per tile of FASTA_TILE bytes: header lines, kept bytes if a header came before the tile, kept bytes if not
//   (exclusive scan of the header counts)
//   fasta_resolve_kernel  per tile: which of the two kept counts holds
//   (exclusive scan of the kept counts)
//   fasta_scatter_kernel  the kept bytes, upper-cased, to text[carried length + tile base + rank]; one record per header line
//   fasta_carry_kernel    the state the next chunk starts from (FastaCarry stays on the device; the host only reads it)
// The rules — which bytes are kept, what kind a line is, where a name lies — stand once, above the kernels, and hold no HIP:
// host/fasta_host_check.cpp compiles them with plain g++ under ASan + UBSan and runs them chunk by chunk in the kernels' order
// (tests/test_index_file_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FASTA_HD __host__ __device__ inline
#else
#define FASTA_HD inline
#endif

#define FASTA_GROUP 16u   /* bytes per thread: one 128-bit load */
#define FASTA_TILE 4096u  /* bytes per workgroup: 256 threads */

/* the kind of the line in progress where a chunk ends */
enum { FASTA_FRESH = 0 /* none: the next byte begins a line */, FASTA_JUNK = 1 /* a line before the first header */, FASTA_HEADER = 2, FASTA_SEQ = 3 };

struct FastaCarry { /* what the chunks before left behind */
    uint64_t text_len;   /* kept bytes so far */
    uint32_t n_seqs;     /* header lines so far */
    uint32_t kind;       /* FASTA_* */
    uint32_t chunk_seqs; /* header lines of the last chunk */
    uint32_t pad;
};

struct FastaHeader {     /* one header line */
    uint32_t line;       /* its '>' in the chunk */
    uint32_t name, name_len; /* the first word behind it */
    uint32_t pad;
    uint64_t text_off;   /* where its sequence begins in the text */
};

/* ---- byte class -------------------------------------------------------------------------------------------------------------------- */
FASTA_HD int fasta_kept(uint32_t c) { return c != ' ' && c != '\t' && c != '\r' && c != '\n'; } /* a byte of a sequence line */
FASTA_HD char fasta_upper(uint32_t c) { return (char)((c >= 'a' && c <= 'z') ? c - 32u : c); }
FASTA_HD uint32_t fasta_byte(const uint32_t w[4], uint32_t q) { return (w[q >> 2] >> (8u * (q & 3u))) & 0xffu; } /* byte q of a group */
FASTA_HD int fasta_text_fits(uint64_t len) { return len < 0xffffffffull; } /* the index addresses the text with 32 bits */

/* ---- line kind ---------------------------------------------------------------------------------------------------------------------- */
struct FastaEnter { /* the line a group's first byte lies in */
    int line_start; /* the byte begins it */
    int in_header;  /* it is a header line */
};

/* base: the group's first byte; j: the chunk's newlines before it; nl: their positions.  One lookup, whatever the line's length. */
FASTA_HD FastaEnter fasta_enter(const char* raw, const uint32_t* nl, uint32_t j, uint32_t base, uint32_t carry_kind) {
    if (j == 0u && carry_kind != FASTA_FRESH) return FastaEnter{0, carry_kind == FASTA_HEADER}; /* the carried line goes on */
    const uint32_t s = j ? nl[j - 1u] + 1u : 0u;
    return FastaEnter{s == base, raw[s] == '>'};
}

struct FastaGroup { /* bit q: byte q of the group ... */
    uint32_t nl;    /* is a newline */
    uint32_t hdr;   /* is the '>' of a header line */
    uint32_t cand;  /* lies in another line and is no blank, tab, CR or LF: kept once a header has been seen */
};

FASTA_HD FastaGroup fasta_group(const uint32_t w[4], uint32_t valid, FastaEnter in) {
    FastaGroup g = {0u, 0u, 0u};
    int start = in.line_start, hdr = in.in_header;
    for (uint32_t q = 0; q < FASTA_GROUP; q++) {
        if (q >= valid) break;
        const uint32_t c = fasta_byte(w, q);
        if (start) {
            hdr = c == '>';
            if (hdr) g.hdr |= 1u << q;
        }
        start = c == '\n';
        if (start) g.nl |= 1u << q;
        if (!hdr && fasta_kept(c)) g.cand |= 1u << q;
    }
    return g;
}

/* the group's kept bytes; seen: a header line lies before the group (in this chunk or an earlier one).  Lines before the file's
 * first header are ignored. */
FASTA_HD uint32_t fasta_keep_mask(FastaGroup g, int seen) {
    if (seen) return g.cand;
    return g.hdr ? g.cand & ~((g.hdr & (0u - g.hdr)) - 1u) : 0u; /* from the group's first header on */
}

FASTA_HD uint32_t fasta_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}

/* ---- name span ----------------------------------------------------------------------------------------------------------------------- */
/* the header line whose '>' is raw[p]; jn: the chunk's newlines before p, so nl[jn] ends the line when jn < lines; else the chunk
 * ends it (the file's last line).  The name: blanks and tabs skipped, then up to a blank, a tab or the line's end without its CR. */
FASTA_HD FastaHeader fasta_header(const char* raw, uint32_t nbytes, const uint32_t* nl, uint32_t lines, uint32_t p, uint32_t jn,
                                  uint64_t text_off) {
    uint32_t end = jn < lines ? nl[jn] : nbytes;
    if (end > p + 1u && raw[end - 1u] == '\r') end--;
    uint32_t a = p + 1u;
    while (a < end && (raw[a] == ' ' || raw[a] == '\t')) a++;
    uint32_t z = a;
    while (z < end && raw[z] != ' ' && raw[z] != '\t') z++;
    return FastaHeader{p, a, z - a, 0u, text_off};
}

/* ---- carried state ------------------------------------------------------------------------------------------------------------------ */
/* after a chunk of nbytes with `lines` newlines, `kept` kept bytes and `hdrs` header lines */
FASTA_HD void fasta_carry_next(FastaCarry* c, const char* raw, uint32_t nbytes, const uint32_t* nl, uint32_t lines, uint32_t kept,
                               uint32_t hdrs) {
    c->text_len += kept, c->n_seqs += hdrs, c->chunk_seqs = hdrs;
    if (!nbytes) return;
    if (raw[nbytes - 1u] == '\n') {
        c->kind = FASTA_FRESH;
    } else if (lines || c->kind == FASTA_FRESH) { /* else the carried line goes on */
        const uint32_t s = lines ? nl[lines - 1u] + 1u : 0u;
        c->kind = raw[s] == '>' ? FASTA_HEADER : c->n_seqs ? FASTA_SEQ : FASTA_JUNK;
    }
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/asm_mi355x.h"
#include "asm_ingest.h"

static_assert(FASTA_TILE == SEQ_TILE && FASTA_TILE == ASM_FASTA_TILE && FASTA_TILE == 256u * FASTA_GROUP, "one tile for the newline index and the parser");

/* exclusive prefix of v over the workgroup's 256 threads and the sum of all of them; s_wave: 4 words, free again after the call */
__device__ inline uint32_t fasta_block_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if ((int)(threadIdx.x & 63) >= off) incl += up;
    }
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - v, all = 0u;
    for (int w = 0; w < 4; w++) {
        if (w < (int)(threadIdx.x >> 6)) before += s_wave[w];
        all += s_wave[w];
    }
    __syncthreads();
    *total = all;
    return before;
}

struct FastaChunk { /* one chunk on the device */
    const char* raw;
    uint32_t nbytes;          /* raw holds FASTA_GROUP spare bytes behind them */
    const uint32_t* nl;       /* the newlines' positions */
    uint32_t lines;           /* how many */
    const uint32_t* nl_base;  /* per tile: the newlines before it */
    const FastaCarry* carry;
};

/* what a thread knows about its group: the same in the count and in the scatter kernel.  j: the chunk's newlines before the group;
 * eh: the tile's header lines before it; *tile_hdr: all of the tile's */
__device__ inline FastaGroup fasta_thread_group(const FastaChunk& c, uint32_t base, uint32_t w[4], uint32_t* s_wave, uint32_t* j, uint32_t* eh,
                                                uint32_t* tile_hdr) {
    const uint32_t valid = base < c.nbytes ? (c.nbytes - base < FASTA_GROUP ? c.nbytes - base : FASTA_GROUP) : 0u;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (valid) v = *reinterpret_cast<const uint4*>(c.raw + base);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    uint32_t unused;
    *j = c.nl_base[blockIdx.x] + fasta_block_scan((uint32_t)__popc(seq_newline_mask(v, (long)base, (long)c.nbytes)), s_wave, &unused);
    FastaGroup g = {0u, 0u, 0u};
    if (valid) g = fasta_group(w, valid, fasta_enter(c.raw, c.nl, *j, base, c.carry->kind));
    *eh = fasta_block_scan(fasta_popc(g.hdr), s_wave, tile_hdr);
    return g;
}

/* one workgroup per tile, and one more behind the last tile that leaves zeros (the scans then end in the totals).  tile_cand: the
 * tile's kept bytes if a header came before the tile; tile_after: if none did */
__global__ __launch_bounds__(256) void fasta_count_kernel(FastaChunk c, uint32_t* __restrict__ tile_hdr, uint32_t* __restrict__ tile_cand,
                                                          uint32_t* __restrict__ tile_after) {
    __shared__ uint32_t s_wave[4];
    if ((uint64_t)blockIdx.x * FASTA_TILE >= c.nbytes) {
        if (threadIdx.x == 0) tile_hdr[blockIdx.x] = 0u, tile_cand[blockIdx.x] = 0u, tile_after[blockIdx.x] = 0u;
        return;
    }
    const uint32_t base = blockIdx.x * FASTA_TILE + threadIdx.x * FASTA_GROUP;
    uint32_t w[4], j, eh, nh, both;
    const FastaGroup g = fasta_thread_group(c, base, w, s_wave, &j, &eh, &nh);
    /* both counts in one scan: a tile holds at most 4096 of either */
    (void)fasta_block_scan(fasta_popc(g.cand) | (fasta_popc(fasta_keep_mask(g, eh > 0u)) << 16), s_wave, &both);
    if (threadIdx.x == 0) tile_hdr[blockIdx.x] = nh, tile_cand[blockIdx.x] = both & 0xffffu, tile_after[blockIdx.x] = both >> 16;
}

/* hbase: the exclusive scan of tile_hdr; n: tiles + 1 */
__global__ __launch_bounds__(256) void fasta_resolve_kernel(const FastaCarry* __restrict__ carry, const uint32_t* __restrict__ hbase,
                                                            const uint32_t* __restrict__ tile_cand, const uint32_t* __restrict__ tile_after,
                                                            uint32_t n, uint32_t* __restrict__ tile_kept) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) tile_kept[t] = (carry->n_seqs + hbase[t] > 0u) ? tile_cand[t] : tile_after[t];
}

/* one workgroup per tile.  kbase: the exclusive scan of tile_kept.  Nothing is written at or behind text[text_cap] or
 * headers[hdr_cap]. */
__global__ __launch_bounds__(256) void fasta_scatter_kernel(FastaChunk c, const uint32_t* __restrict__ hbase, const uint32_t* __restrict__ kbase,
                                                            char* __restrict__ text, uint64_t text_cap, FastaHeader* __restrict__ headers,
                                                            uint32_t hdr_cap) {
    __shared__ uint32_t s_wave[4];
    const uint32_t base = blockIdx.x * FASTA_TILE + threadIdx.x * FASTA_GROUP;
    uint32_t w[4], j, eh, nh, unused;
    const FastaGroup g = fasta_thread_group(c, base, w, s_wave, &j, &eh, &nh);
    const uint32_t keep = fasta_keep_mask(g, c.carry->n_seqs + hbase[blockIdx.x] + eh > 0u);
    const uint32_t ek = fasta_block_scan(fasta_popc(keep), s_wave, &unused);
    const uint64_t first = c.carry->text_len + kbase[blockIdx.x] + ek; /* the group's first kept byte */
    uint64_t dst = first;
    for (uint32_t m = keep; m; m &= m - 1u, dst++) {
        const uint32_t q = (uint32_t)__builtin_ctz(m);
        if (dst < text_cap) text[dst] = fasta_upper(fasta_byte(w, q));
    }
    uint32_t idx = hbase[blockIdx.x] + eh;
    for (uint32_t m = g.hdr; m; m &= m - 1u, idx++) {
        const uint32_t q = (uint32_t)__builtin_ctz(m), below = (1u << q) - 1u;
        if (idx < hdr_cap)
            headers[idx] = fasta_header(c.raw, c.nbytes, c.nl, c.lines, base + q, j + fasta_popc(g.nl & below), first + fasta_popc(keep & below));
    }
}

/* totals: hbase[tiles] and kbase[tiles] */
__global__ void fasta_carry_kernel(FastaChunk c, const uint32_t* __restrict__ hdr_total, const uint32_t* __restrict__ kept_total,
                                   FastaCarry* __restrict__ carry) {
    if (blockIdx.x == 0 && threadIdx.x == 0) fasta_carry_next(carry, c.raw, c.nbytes, c.nl, c.lines, *kept_total, *hdr_total);
}
#endif /* __HIPCC__ */
