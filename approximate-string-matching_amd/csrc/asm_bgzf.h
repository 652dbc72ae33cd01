// The BGZF container of the file calls' BAM output (contract: docs/design/mapper.md, "BAM output"): stored deflate blocks, what
// `samtools view -u` writes.  A block is 18 header bytes (1f 8b 08 04 00000000 00 ff 0600 42 43 0200 BSIZE), the stored-block header
// 01 LEN ~LEN, up to BGZF_PAYLOAD payload bytes, CRC-32 and ISIZE: payload + 31 bytes.  The only work is the CRC.
//
// bgzf_frame_kernel, one workgroup per block: thread t takes the fixed slice [64 t, 64 t + 64) of the payload, loads it once
// (4 x 16 bytes), stores it into place and folds it into a CRC state of its own (slice-by-4 tables in LDS).  CRC is linear: the
// state after the whole block is the XOR of every slice's state times x^(8 * bytes behind the slice) mod P.  The slices in front of
// the last one are a whole number of slices plus the last slice's length away from the block's end, so each multiplies by a
// precomputed x^(512 m), the products are XOR-reduced, and one more multiplication by x^(8 * last slice's length) brings the sum to
// the end.
//
// At ASM_BGZF_DEFLATE the blocks are deflate blocks instead: asm_deflate.h, which this file includes behind its first part, holds the
// encoder, its kernel and the compaction; the device entry (bgzf_deflate_device), the record stream and the C entry points are here.
//
// The first part holds no HIP: the tables, the slice width, a slice's CRC, load and store, the multiplication and the block's fixed
// bytes.  The host frames the BAM header's blocks with it (bgzf_frame_host runs the same per-slice code serially), and
// host/bam_host_check.cpp compiles it with plain g++ under ASan + UBSan (tests/test_bam_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "asm_sam.h" /* SAM_HD, sam_funnel */

extern "C++" {

#define BGZF_PAYLOAD 65280u /* uncompressed bytes per block: htslib's value, ASM_BGZF_PAYLOAD */
#define BGZF_FRONT 23u      /* the bytes in front of the payload: gzip header with the BC field, stored-block header */
#define BGZF_BACK 8u        /* CRC-32, ISIZE */
#define BGZF_BLOCK (BGZF_FRONT + BGZF_PAYLOAD + BGZF_BACK)
#define BGZF_EOF 28u
#define BGZF_SLICE 64u                            /* payload bytes per thread */
#define BGZF_SLICES (BGZF_PAYLOAD / BGZF_SLICE)   /* 1020 */
#define BGZF_THREADS 1024u
#define BGZF_SRC_PAD 16u /* the source is read in whole 16-byte pieces: it starts 16-byte aligned and may be read to the next multiple */
#define BGZF_POLY 0xedb88320u

/* a * b mod P in CRC-32's reflected form, where bit 31 is x^0 (zlib's multmodp) */
SAM_HD constexpr uint32_t bgzf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0u;
    for (uint32_t m = 0x80000000u; m != 0u; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ BGZF_POLY : b >> 1;
    }
    return p;
}

struct BgzfTables {
    uint32_t t[4][256];               /* slice-by-4: t[k][v] = the state after byte v and k zero bytes */
    uint32_t pow_slices[BGZF_SLICES]; /* x^(8 * BGZF_SLICE * m) mod P */
    uint32_t pow_bytes[BGZF_SLICE + 1u]; /* x^(8 r) mod P */
};
constexpr BgzfTables bgzf_make_tables() {
    BgzfTables T{};
    for (uint32_t v = 0; v < 256u; v++) {
        uint32_t c = v;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ BGZF_POLY : c >> 1;
        T.t[0][v] = c;
    }
    for (uint32_t k = 1; k < 4u; k++)
        for (uint32_t v = 0; v < 256u; v++) T.t[k][v] = (T.t[k - 1u][v] >> 8) ^ T.t[0][T.t[k - 1u][v] & 0xffu];
    uint32_t p = 0x80000000u;
    for (uint32_t r = 0; r <= BGZF_SLICE; r++) T.pow_bytes[r] = p, p = bgzf_mul(p, 0x00800000u /* x^8 */);
    p = 0x80000000u;
    for (uint32_t m = 0; m < BGZF_SLICES; m++) T.pow_slices[m] = p, p = bgzf_mul(p, T.pow_bytes[BGZF_SLICE]);
    return T;
}

typedef uint32_t BgzfCrcTable[4][256];

/* the state after the four bytes of w, lowest first, and after one byte */
SAM_HD uint32_t bgzf_crc_word(const BgzfCrcTable& t, uint32_t s, uint32_t w) {
    s ^= w;
    return t[3][s & 0xffu] ^ t[2][(s >> 8) & 0xffu] ^ t[1][(s >> 16) & 0xffu] ^ t[0][s >> 24];
}
SAM_HD uint32_t bgzf_crc_byte(const BgzfCrcTable& t, uint32_t s, uint32_t b) { return t[0][(s ^ b) & 0xffu] ^ (s >> 8); }

/* One slice in registers: its 16 dwords and a zero behind them.  Loaded in 16-byte pieces, only those that hold one of its nbytes. */
struct BgzfSlice {
    uint32_t w[BGZF_SLICE / 4u + 1u];
};
SAM_HD BgzfSlice bgzf_load_slice(const uint8_t* s, uint32_t nbytes) {
    BgzfSlice v = {};
#pragma unroll
    for (uint32_t j = 0; j < BGZF_SLICE / 16u; j++)
        if (16u * j < nbytes) __builtin_memcpy(&v.w[4u * j], (const uint8_t*)__builtin_assume_aligned(s + 16u * j, 16), 16);
    return v;
}
/* the state s after the slice's first nbytes <= BGZF_SLICE bytes */
SAM_HD uint32_t bgzf_crc_slice(const BgzfCrcTable& t, uint32_t s, const BgzfSlice& v, uint32_t nbytes) {
    uint32_t last = 0u;
#pragma unroll
    for (uint32_t j = 0; j < BGZF_SLICE / 4u; j++) {
        if (4u * j + 4u <= nbytes) s = bgzf_crc_word(t, s, v.w[j]);
        else if (j == nbytes >> 2) last = v.w[j];
    }
    for (uint32_t b = 0; b < (nbytes & 3u); b++) s = bgzf_crc_byte(t, s, (last >> (8u * b)) & 0xffu);
    return s;
}
/* the slice's first nbytes bytes to d[0, nbytes), d aligned anyhow: up to 3 single bytes to the next dword, then whole dwords cut
 * out of neighbouring registers (sam_funnel), then up to 3 single bytes.  Writes nothing else. */
SAM_HD void bgzf_store_slice(uint8_t* d, const BgzfSlice& v, uint32_t nbytes) {
    const uint32_t to_edge = (4u - (uint32_t)((uintptr_t)d & 3u)) & 3u, head = to_edge < nbytes ? to_edge : nbytes;
#pragma unroll
    for (uint32_t b = 0; b < 3u; b++)
        if (b < head) d[b] = (uint8_t)(v.w[0] >> (8u * b));
    const uint32_t nmid = (nbytes - head) >> 2, ntail = nbytes - head - 4u * nmid;
    uint32_t last = 0u;
#pragma unroll
    for (uint32_t j = 0; j < BGZF_SLICE / 4u; j++) {
        const uint32_t x = sam_funnel(v.w[j + 1u], v.w[j], head);
        if (j < nmid) __builtin_memcpy(__builtin_assume_aligned(d + head + 4u * j, 4), &x, 4);
        else if (j == nmid) last = x;
    }
#pragma unroll
    for (uint32_t b = 0; b < 3u; b++)
        if (b < ntail) d[head + 4u * nmid + b] = (uint8_t)(last >> (8u * b));
}

/* how a block of len >= 1 payload bytes is cut: slices [0, last) are whole, slice `last` has last_len in [1, BGZF_SLICE] bytes */
struct BgzfCut {
    uint32_t last, last_len;
};
SAM_HD BgzfCut bgzf_cut(uint32_t len) {
    const uint32_t last = (len - 1u) / BGZF_SLICE;
    return {last, len - BGZF_SLICE * last};
}
SAM_HD uint32_t bgzf_slice_bytes(const BgzfCut& c, uint32_t t) { return t < c.last ? BGZF_SLICE : t == c.last ? c.last_len : 0u; }
/* the CRC register a slice starts from: the block's first slice carries CRC-32's initial value */
SAM_HD uint32_t bgzf_slice_init(uint32_t t) { return t == 0u ? 0xffffffffu : 0u; }
/* the block's CRC-32 from the XOR of (state of slice t) * pow_slices[last - 1 - t] over t < last, and the last slice's state */
SAM_HD uint32_t bgzf_crc_finish(uint32_t front, uint32_t pow_last_len, uint32_t last_state) {
    return ~(bgzf_mul(front, pow_last_len) ^ last_state);
}

/* the fixed bytes: i < BGZF_FRONT in front of a payload of len bytes, i < BGZF_BACK behind it, i < BGZF_EOF of the EOF block */
SAM_HD uint8_t bgzf_front_byte(uint32_t i, uint32_t len) {
    const uint64_t a = 0x0000000004088b1full, b = 0x000243420006ff00ull;
    const uint32_t bsize = len + BGZF_FRONT + BGZF_BACK - 1u;
    if (i < 8u) return (uint8_t)(a >> (8u * i));
    if (i < 16u) return (uint8_t)(b >> (8u * (i - 8u)));
    if (i < 18u) return (uint8_t)(bsize >> (8u * (i - 16u)));
    if (i == 18u) return 1u; /* BFINAL, BTYPE 00 */
    return (uint8_t)((i < 21u ? len : ~len) >> (8u * ((i - 19u) & 1u)));
}
SAM_HD uint8_t bgzf_back_byte(uint32_t i, uint32_t crc, uint32_t len) { return (uint8_t)((i < 4u ? crc : len) >> (8u * (i & 3u))); }
SAM_HD uint8_t bgzf_eof_byte(uint32_t i) { return i < 16u ? bgzf_front_byte(i, 0u) : i == 16u ? 0x1bu : i == 18u ? 3u : 0u; }

inline size_t bgzf_blocks(size_t n) { return (n + BGZF_PAYLOAD - 1u) / BGZF_PAYLOAD; }
inline size_t bgzf_bound(size_t n, int with_eof) { return n + (BGZF_FRONT + BGZF_BACK) * bgzf_blocks(n) + (with_eof ? BGZF_EOF : 0u); }

inline const BgzfTables& bgzf_host_tables() {
    static constexpr BgzfTables T = bgzf_make_tables();
    return T;
}
/* the CRC-32 of p[0, len), len in [1, BGZF_PAYLOAD], and the payload copied to out, slice by slice as bgzf_frame_kernel's threads do
 * it; p is 16-byte aligned and readable up to the next multiple of 16 */
inline uint32_t bgzf_block_host(const uint8_t* p, uint32_t len, uint8_t* out) {
    const BgzfTables& T = bgzf_host_tables();
    const BgzfCut c = bgzf_cut(len);
    uint32_t front = 0u, last_state = 0u;
    for (uint32_t t = 0; t <= c.last; t++) {
        const uint32_t nbytes = bgzf_slice_bytes(c, t);
        const BgzfSlice v = bgzf_load_slice(p + BGZF_SLICE * t, nbytes);
        const uint32_t s = bgzf_crc_slice(T.t, bgzf_slice_init(t), v, nbytes);
        if (out) bgzf_store_slice(out + BGZF_SLICE * t, v, nbytes);
        if (t < c.last) front ^= bgzf_mul(s, T.pow_slices[c.last - 1u - t]);
        else last_state = s;
    }
    return bgzf_crc_finish(front, T.pow_bytes[c.last_len], last_state);
}
/* src[0, n) framed onto the end of out, as bgzf_frame_kernel frames it */
inline void bgzf_frame_host(const void* src, size_t n, int with_eof, std::vector<uint8_t>& out) {
    std::vector<uint32_t> aligned((BGZF_PAYLOAD + BGZF_SRC_PAD) / 4u + 4u);
    uint8_t* const stage = (uint8_t*)(((uintptr_t)aligned.data() + 15u) & ~(uintptr_t)15u);
    for (size_t at = 0; at < n; at += BGZF_PAYLOAD) {
        const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD ? n - at : BGZF_PAYLOAD);
        memcpy(stage, (const uint8_t*)src + at, len);
        const size_t blk = out.size();
        out.resize(blk + BGZF_FRONT + len + BGZF_BACK);
        for (uint32_t i = 0; i < BGZF_FRONT; i++) out[blk + i] = bgzf_front_byte(i, len);
        const uint32_t crc = bgzf_block_host(stage, len, out.data() + blk + BGZF_FRONT);
        for (uint32_t i = 0; i < BGZF_BACK; i++) out[blk + BGZF_FRONT + len + i] = bgzf_back_byte(i, crc, len);
    }
    if (with_eof)
        for (uint32_t i = 0; i < BGZF_EOF; i++) out.push_back(bgzf_eof_byte(i));
}

#if defined(__HIPCC__)
__device__ const BgzfTables bgzf_device_tables = bgzf_make_tables();
#endif

#include "asm_deflate.h"

#if defined(__HIPCC__)

/* Workgroup b < nblocks frames src[b * BGZF_PAYLOAD, ...) (the last block: what is left of n) into dst + b * BGZF_BLOCK; workgroup
 * nblocks, when the grid has one, writes the EOF block behind them.  src: 16-byte aligned, readable to the next multiple of 16
 * behind n (BGZF_SRC_PAD).  Writes dst[0, bgzf_bound(n, grid > nblocks)) and nothing else. */
__global__ __launch_bounds__(BGZF_THREADS) void bgzf_frame_kernel(const uint8_t* __restrict__ src, unsigned long long n, uint32_t nblocks,
                                                                 uint8_t* __restrict__ dst) {
    __shared__ BgzfCrcTable table;
    __shared__ uint32_t wave_front[BGZF_THREADS / 64u];
    __shared__ uint32_t last_state;
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    if (b >= nblocks) { /* the whole workgroup: no barrier is skipped.  The EOF block lies behind the last block, which may be short */
        if (t < BGZF_EOF) dst[n + (size_t)(BGZF_FRONT + BGZF_BACK) * nblocks + t] = bgzf_eof_byte(t);
        return;
    }
    uint8_t* const blk = dst + (size_t)b * BGZF_BLOCK;
    (&table[0][0])[t] = (&bgzf_device_tables.t[0][0])[t]; /* 4 x 256 entries, one per thread */
    const unsigned long long at = (unsigned long long)b * BGZF_PAYLOAD;
    const uint32_t len = (uint32_t)(n - at < BGZF_PAYLOAD ? n - at : BGZF_PAYLOAD);
    const BgzfCut c = bgzf_cut(len);
    const uint32_t nbytes = bgzf_slice_bytes(c, t);
    const BgzfSlice v = bgzf_load_slice(src + at + BGZF_SLICE * t, nbytes);
    if (t < BGZF_FRONT) blk[t] = bgzf_front_byte(t, len);
    bgzf_store_slice(blk + BGZF_FRONT + BGZF_SLICE * t, v, nbytes);
    __syncthreads();
    const uint32_t s = bgzf_crc_slice(table, bgzf_slice_init(t), v, nbytes);
    uint32_t front = t < c.last ? bgzf_mul(s, bgzf_device_tables.pow_slices[c.last - 1u - t]) : 0u;
    if (t == c.last) last_state = s;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) front ^= __shfl_xor(front, off);
    if ((t & 63u) == 0u) wave_front[t >> 6] = front;
    __syncthreads();
    if (t < BGZF_BACK) {
        uint32_t all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < BGZF_THREADS / 64u; w++) all ^= wave_front[w];
        blk[BGZF_FRONT + len + t] = bgzf_back_byte(t, bgzf_crc_finish(all, bgzf_device_tables.pow_bytes[c.last_len], last_state), len);
    }
}
/* src[0, n) on the device (BGZF_SRC_PAD) framed into dst, with the EOF block behind it when with_eof; dst holds bgzf_bound(n,
 * with_eof) bytes.  On the handle's stream; nothing to frame launches nothing. */
static hipError_t bgzf_frame_device(asm_handle* h, const char* src, size_t n, int with_eof, char* dst) {
    const size_t nblocks = bgzf_blocks(n);
    if (nblocks + (with_eof ? 1 : 0) == 0) return hipSuccess;
    return launch(h, bgzf_frame_kernel, (unsigned)(nblocks + (with_eof ? 1 : 0)), BGZF_THREADS, (const uint8_t*)src, (unsigned long long)n,
                  (uint32_t)nblocks, (uint8_t*)dst);
}

/* bgzf_frame_kernel's blocks of n payload bytes: their sizes in the file, for the sorted BAM call's index (asm_bai.h) */
__global__ __launch_bounds__(256) void bgzf_stored_sizes_kernel(unsigned long long* __restrict__ size, uint32_t nblocks, unsigned long long n) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    const unsigned long long left = n - (unsigned long long)b * BGZF_PAYLOAD;
    size[b] = (left < BGZF_PAYLOAD ? left : BGZF_PAYLOAD) + BGZF_FRONT + BGZF_BACK;
}

/* The same at ASM_BGZF_DEFLATE: the blocks encoded at a fixed stride (bgzf_deflate_kernel), their sizes summed, the blocks moved
 * together into dst (bgzf_compact_kernel) with the EOF block behind them when with_eof, and the bytes written read back into *total
 * (one wait).  dst holds bgzf_bound(n, with_eof) bytes.  Nothing to encode launches nothing and waits for nothing.  keep: NULL, or room
 * on the device for the blocks' sizes, copied there in stream order. */
static hipError_t bgzf_deflate_device(asm_handle* h, const char* src, size_t n, int with_eof, char* dst, size_t* total,
                                      unsigned long long* keep = nullptr) {
    typedef unsigned long long u64;
    const size_t nblocks = bgzf_blocks(n);
    *total = 0;
    if (nblocks + (with_eof ? 1 : 0) == 0) return hipSuccess;
    Scratch<uint8_t> d_tmp(h);
    Scratch<u64> d_size(h), d_off(h);
    MapTmp tmp(h);
    hipError_t e = d_tmp.alloc(nblocks * DFL_STRIDE + 16);
    if (e == hipSuccess) e = d_size.alloc(sizeof(u64) * (nblocks + 1));
    if (e == hipSuccess) e = d_off.alloc(sizeof(u64) * (nblocks + 1));
    if (e == hipSuccess) e = hipMemsetAsync(d_size.p + nblocks, 0, sizeof(u64), h->stream);
    if (e == hipSuccess && nblocks)
        e = launch(h, bgzf_deflate_kernel, (unsigned)nblocks, BGZF_THREADS, (const uint8_t*)src, (u64)n, (uint32_t)nblocks, d_tmp.p, d_size.p);
    if (e == hipSuccess && keep && nblocks) e = hipMemcpyAsync(keep, d_size.p, sizeof(u64) * nblocks, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = map_exclusive_sum(h, tmp, d_size.p, d_off.p, (int64_t)nblocks + 1);
    if (e == hipSuccess)
        e = launch(h, bgzf_compact_kernel, (unsigned)(nblocks + (with_eof ? 1 : 0)), BGZF_THREADS, (const uint8_t*)d_tmp.p, (const u64*)d_size.p,
                   (const u64*)d_off.p, (uint32_t)nblocks, (uint8_t*)dst);
    u64 end = 0;
    if (e == hipSuccess) e = fetch(h, {fetched(&end, (const u64*)d_off.p + nblocks)});
    *total = (size_t)end + (with_eof ? BGZF_EOF : 0u);
    return e;
}
/* src framed into dst at `level`; *total: the bytes written (ASM_BGZF_STORED: the bound, with no wait); keep: NULL, or room on the
 * device for the size of every block framed */
static hipError_t bgzf_level_device(asm_handle* h, int level, const char* src, size_t n, int with_eof, char* dst, size_t* total,
                                    unsigned long long* keep = nullptr) {
    if (level == ASM_BGZF_DEFLATE) return bgzf_deflate_device(h, src, n, with_eof, dst, total, keep);
    *total = bgzf_bound(n, with_eof);
    if (keep && n)
        if (const hipError_t e = launch(h, bgzf_stored_sizes_kernel, (unsigned)((bgzf_blocks(n) + 255u) / 256u), 256u, keep, (uint32_t)bgzf_blocks(n),
                                        (unsigned long long)n))
            return e;
    return bgzf_frame_device(h, src, n, with_eof, dst);
}

/* The record stream of one BAM file call.  It is cut every BGZF_PAYLOAD bytes counted from its first byte, whatever the device
 * chunks or sorted slabs are that bring it: what a chunk leaves behind its last whole block stays in `carry` on the device and leads
 * the next one.  Per chunk: stage(n) gives a buffer with the carry in front and room for the chunk's n bytes; the caller fills those
 * and calls frame(), which writes at most framed(n) bytes of whole blocks and keeps the rest.  tail() frames what is left and the EOF
 * block, at most tail_bytes().  Both give the bytes they wrote: the bound at ASM_BGZF_STORED, what the encoder made of it at
 * ASM_BGZF_DEFLATE (read back with one wait).  keep: NULL, or a device table with room for the size in the file of every block of the
 * stream, in order (the sorted call's index, asm_bai.h); kept counts them. */
struct BgzfStream {
    asm_handle* h;
    Scratch<char> carry;
    size_t carry_len = 0;
    unsigned long long* keep = nullptr;
    size_t kept = 0;
    const int level;
    explicit BgzfStream(asm_handle* owner) : h(owner), carry(owner), level(owner->bgzf_level) {}
    hipError_t open() { return carry.alloc(BGZF_PAYLOAD + BGZF_SRC_PAD); }
    size_t framed(size_t n) const { return (carry_len + n) / BGZF_PAYLOAD * BGZF_BLOCK; }
    size_t tail_bytes() const { return bgzf_bound(carry_len, 1); }
    hipError_t stage(size_t n, Scratch<char>& buf, char** fresh) {
        if (const hipError_t e = buf.alloc(carry_len + n + BGZF_SRC_PAD)) return e;
        *fresh = buf.p + carry_len;
        return carry_len ? hipMemcpyAsync(buf.p, carry.p, carry_len, hipMemcpyDeviceToDevice, h->stream) : hipSuccess;
    }
    hipError_t frame(const Scratch<char>& buf, size_t n, char* dst, size_t* written) {
        const size_t whole = (carry_len + n) / BGZF_PAYLOAD * BGZF_PAYLOAD, rest = carry_len + n - whole;
        if (const hipError_t e = bgzf_level_device(h, level, buf.p, whole, 0, dst, written, keep ? keep + kept : nullptr)) return e;
        carry_len = rest, kept += whole / BGZF_PAYLOAD;
        return rest ? hipMemcpyAsync(carry.p, buf.p + whole, rest, hipMemcpyDeviceToDevice, h->stream) : hipSuccess;
    }
    hipError_t tail(char* dst, size_t* written) {
        const hipError_t e = bgzf_level_device(h, level, carry.p, carry_len, 1, dst, written, keep ? keep + kept : nullptr);
        kept += bgzf_blocks(carry_len), carry_len = 0;
        return e;
    }
};

#endif /* __HIPCC__ */

} /* extern "C++" */

#if defined(__HIPCC__)
static_assert(ASM_BGZF_PAYLOAD == BGZF_PAYLOAD, "the ABI's ASM_BGZF_PAYLOAD is the payload of asm_bgzf.h");

size_t asm_bgzf_bound(size_t n, int with_eof) { return bgzf_bound(n, with_eof); }

static int bgzf_level_check(asm_handle* h, const std::string& who, int level) {
    if (level != ASM_BGZF_STORED && level != ASM_BGZF_DEFLATE)
        return fail(h, ASM_EINVAL, who + ": level must be ASM_BGZF_STORED (0) or ASM_BGZF_DEFLATE (1)");
    return ASM_OK;
}
int asm_map_set_bgzf_level(asm_handle* h, int level) {
    if (const int rc = bgzf_level_check(h, "asm_map_set_bgzf_level", level)) return rc;
    if (!h) return fail(h, ASM_EINVAL, "asm_map_set_bgzf_level: NULL handle");
    h->bgzf_level = level;
    return ASM_OK;
}
int asm_map_get_bgzf_level(const asm_handle* h) { return h ? h->bgzf_level : ASM_BGZF_STORED; }

/* asm_bgzf_frame and asm_bgzf_compress (`name`) */
static int bgzf_frame_call(const char* name, asm_handle* h, const void* src, size_t n, int with_eof, int level, void* dst, size_t dst_cap,
                           size_t* dst_len) {
    const char* who = name;
    const std::string call = name;
    if (const int rc = bgzf_level_check(h, call, level)) return rc;
    if (!h || (n && !src) || !dst_len) return fail(h, ASM_EINVAL, call + ": NULL argument");
    const size_t need = bgzf_bound(n, with_eof);
    if (dst_cap < need || (need && !dst)) return fail(h, ASM_EINVAL, call + ": dst_cap is below asm_bgzf_bound (" + std::to_string(need) + " bytes)");
    if (bgzf_blocks(n) >= 0xffffffffull) return fail(h, ASM_EUNSUPPORTED, call + ": 2^32 blocks or more");
    *dst_len = 0;
    HIPCHK(h, hipSetDevice(h->device));
    Scratch<char> d_src(h), d_dst(h);
    STREAM_TRY(who, d_src.alloc(n + BGZF_SRC_PAD));
    STREAM_TRY(who, d_dst.alloc(need + 1));
    if (n) STREAM_TRY(who, hipMemcpyAsync(d_src.p, src, n, hipMemcpyHostToDevice, h->stream));
    size_t written = 0;
    STREAM_TRY(who, bgzf_level_device(h, level, d_src.p, n, with_eof, d_dst.p, &written));
    if (written) STREAM_TRY(who, hipMemcpyAsync(dst, d_dst.p, written, hipMemcpyDeviceToHost, h->stream));
    STREAM_TRY(who, hipStreamSynchronize(h->stream));
    *dst_len = written;
    return ASM_OK;
}
int asm_bgzf_frame(asm_handle* h, const void* src, size_t n, int with_eof, void* dst, size_t dst_cap, size_t* dst_len) {
    return bgzf_frame_call("asm_bgzf_frame", h, src, n, with_eof, ASM_BGZF_STORED, dst, dst_cap, dst_len);
}
int asm_bgzf_compress(asm_handle* h, const void* src, size_t n, int with_eof, int level, void* dst, size_t dst_cap, size_t* dst_len) {
    return bgzf_frame_call("asm_bgzf_compress", h, src, n, with_eof, level, dst, dst_cap, dst_len);
}
int asm_bgzf_compress_host(const void* src, size_t n, int with_eof, int level, void* dst, size_t dst_cap, size_t* dst_len) {
    const std::string call = "asm_bgzf_compress_host";
    if (const int rc = bgzf_level_check(nullptr, call, level)) return rc;
    if ((n && !src) || !dst_len) return fail(nullptr, ASM_EINVAL, call + ": NULL argument");
    const size_t need = bgzf_bound(n, with_eof);
    if (dst_cap < need || (need && !dst)) return fail(nullptr, ASM_EINVAL, call + ": dst_cap is below asm_bgzf_bound (" + std::to_string(need) + " bytes)");
    *dst_len = 0;
    std::vector<uint8_t> out;
    bgzf_compress_host(src, n, with_eof, level, out, nullptr);
    if (!out.empty()) memcpy(dst, out.data(), out.size());
    *dst_len = out.size();
    return ASM_OK;
}
#endif /* __HIPCC__ */
