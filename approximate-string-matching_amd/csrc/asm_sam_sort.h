// Coordinate-sorted SAM from the file calls (asm_map_file_sorted, asm_map_pairs_file_sorted; contract and design:
// docs/design/mapper.md, "Sorted output").  A sorted call formats every device chunk as the unsorted call does, but keeps the
// formatted block on the device with one (key, source address, size) entry per line; after the last chunk the keys are sorted
// (stable, so equal keys keep the unsorted order), the sizes are permuted and scanned into output offsets, and
// sam_line_gather_kernel copies the lines in sorted order into output slabs that leave as the unsorted call's chunks do, one
// MapOutput::put each (asm_map_out.h).  The key itself is sam_sort_key (asm_sam.h), the slab cutter sam_slab_cuts (asm_host.h).
// The part above the kernels holds no HIP: host/sort_host_check.cpp compiles the per-lane copy with plain g++ under ASan + UBSan
// (tests/test_sam_sort_host.py).  asm_capi.hip includes this file inside its extern "C" block, between asm_map_out.h and
// asm_map_file.h.
#pragma once
#include <stdint.h>

#include "asm_sam.h"

extern "C++" {

/* Lanes that copy one line.  Lines are mostly 200-700 bytes with a tail to about 1.2 KB: a group of 16 lanes moves 256 bytes per
 * step (two 128-byte lines of the cache per store instruction), so such a line takes 1-3 steps and a wave works on four lines at
 * once; a whole wave per line would leave most of its 64 x 16 bytes idle on all but the longest lines, and one thread per line
 * would store 16 bytes per instruction to 64 unrelated places. */
#define SAM_GATHER_LANES 16u
/* bytes behind a held block's text that may be read (the copy's loads look up to 4 bytes past a line), as MapOutput pads a slot */
#define SAM_SORT_PAD 64u

struct alignas(4) SamQuad {
    uint32_t w[4];
};

/* Lane g of SAM_GATHER_LANES copies its share of src[0, len) to dst[0, len); source and destination are byte-aligned independently.
 * Up to 15 head bytes bring the destination to a 16-byte boundary, one byte per lane; then 16-byte stores, lane g the chunks g, g +
 * 16, ...; then up to 15 tail bytes, one per lane.  A chunk's 16 source bytes lie anywhere: they are cut out of the five aligned
 * dwords that hold them (one 16-byte and one 4-byte load, then four funnel shifts by the source's offset inside a dword).
 * Reads [src - 3, src + len + 4) rounded to dwords inside it: the source block starts dword-aligned and has SAM_SORT_PAD bytes
 * behind its text.  Writes dst[0, len) and nothing else.  Src: const char*, which the kernel qualifies as global memory (an address
 * that comes out of a table is otherwise loaded from with flat instructions). */
template <class Src>
SAM_HD void sam_gather_line(char* dst, Src src, uint64_t len, uint32_t g) {
    const uint64_t to_edge = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    const uint64_t head = to_edge < len ? to_edge : len;
    if (g < head) dst[g] = src[g];
    const uint64_t nmid = (len - head) >> 4, tail = head + (nmid << 4);
    const uint32_t r = (uint32_t)((uintptr_t)(src + head) & 3u);
    const Src s = src + head - r; /* dword-aligned */
    char* d = dst + head;           /* 16-byte-aligned */
    for (uint64_t c = g; c < nmid; c += SAM_GATHER_LANES) {
        SamQuad q, v;
        uint32_t next;
        __builtin_memcpy(&q, (Src)__builtin_assume_aligned(s + 16u * c, 4), 16);
        __builtin_memcpy(&next, (Src)__builtin_assume_aligned(s + 16u * c + 16u, 4), 4);
        v.w[0] = sam_funnel(q.w[1], q.w[0], r), v.w[1] = sam_funnel(q.w[2], q.w[1], r);
        v.w[2] = sam_funnel(q.w[3], q.w[2], r), v.w[3] = sam_funnel(next, q.w[3], r);
        __builtin_memcpy(__builtin_assume_aligned(d + 16u * c, 16), &v, 16);
    }
    if (tail + g < len) dst[tail + g] = src[tail + g];
}

#if defined(__HIPCC__)

/* one thread per line of a held chunk, behind its line_size_kernel and scan: the line's key, where its bytes lie and how many */
template <bool PAIRED>
__global__ __launch_bounds__(256) void sam_sort_key_kernel(SamArgs a, int32_t n_seqs, unsigned long long* __restrict__ key,
                                                           unsigned long long* __restrict__ src, unsigned long long* __restrict__ size) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.nlines) return;
    key[l] = sam_sort_key(sam_load<PAIRED>(a, l), n_seqs);
    src[l] = (unsigned long long)(uintptr_t)(a.out + a.off[l]);
    size[l] = a.size[l];
}

/* the sort's values: the global line numbers */
__global__ __launch_bounds__(256) void sam_sort_iota_kernel(uint32_t* __restrict__ idx, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}

/* output line i is input line idx[i]: its source and its size, and a last size of 0 for the scan's total */
__global__ __launch_bounds__(256) void sam_sort_permute_kernel(const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ src,
                                                               const unsigned long long* __restrict__ size, unsigned long long n,
                                                               unsigned long long* __restrict__ psrc, unsigned long long* __restrict__ psize) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) psrc[i] = src[idx[i]], psize[i] = size[idx[i]];
    else if (i == n) psize[i] = 0ull;
}

/* The lines [0, n) of one output slab (src and off point at the slab's first line; off[n] is read): line i goes from its held
 * block to out + off[i] - slab_base, SAM_GATHER_LANES lanes per line (sam_gather_line). */
typedef const __attribute__((address_space(1))) char* SamGlobalSrc;
__global__ __launch_bounds__(256) void sam_line_gather_kernel(const unsigned long long* __restrict__ src, const unsigned long long* __restrict__ off,
                                                              long n, unsigned long long slab_base, char* __restrict__ out) {
    const uint32_t g = threadIdx.x & (SAM_GATHER_LANES - 1u);
    const long group = ((long)blockIdx.x * blockDim.x + threadIdx.x) / SAM_GATHER_LANES;
    const long ngroups = ((long)gridDim.x * blockDim.x) / SAM_GATHER_LANES;
    for (long i = group; i < n; i += ngroups) {
        const unsigned long long at = off[i];
        sam_gather_line(out + (at - slab_base), (SamGlobalSrc)(uintptr_t)src[i], off[i + 1] - at, g);
    }
}

/* What a sorted call holds on the device, and its two steps: hold() in place of a chunk's copy-out, flush() after the last chunk.
 * Every allocation of the hold (the held text, the line tables, the sort's arrays) is counted against max_device_bytes first (cap;
 * 0: none); the blocks go back to the pool with the session.  Not counted, as in the unsorted call: the output slots of the rotation
 * (at most a slab each) and, under ASM_OUT_BAM, a slab's staging block (the stream's carry of less than a BGZF block plus the
 * slab), which lives for one slab.
 * index: a BAM call under ASM_BAM_INDEX_BAI.  flush() then keeps the sources and offsets in output order and gives the record stream a
 * table for its blocks' sizes; bai_index_device (asm_bai.h) builds the index from them when the output is finished, in allocations of
 * this hold. */
struct SamSortHold {
    asm_handle* h;
    const char* who;
    const int32_t n_seqs;
    const size_t cap;
    const bool index;
    unsigned long long *psrc = nullptr, *off = nullptr; /* [lines], [lines + 1]: set by flush() */
    unsigned long long* blk_size = nullptr;             /* index: [nblk + 1], the last one 0 */
    size_t nblk = 0;
    size_t used = 0, reached = 0;
    struct Chunk { /* one held device chunk: its SAM bytes and its line tables */
        char* text;
        unsigned long long *key, *src, *size;
        int64_t nlines;
    };
    std::vector<Chunk> chunks;
    std::vector<void*> owned; /* everything to give back */
    asm_sam_sort_stats st = {};
    SamSortHold(asm_handle* owner, const char* call, int32_t seqs, size_t max_device_bytes)
        : h(owner), who(call), n_seqs(seqs), cap(max_device_bytes),
          index(owner->out_format == ASM_OUT_BAM && owner->bam_index == ASM_BAM_INDEX_BAI) {}
    SamSortHold(const SamSortHold&) = delete;
    SamSortHold& operator=(const SamSortHold&) = delete;
    ~SamSortHold() {
        for (void* p : owned) pool_free(h, p);
    }

    int no_memory(size_t wanted) {
        return fail(h, ASM_ENOMEM,
                    std::string(who) + ": sorted output keeps the whole SAM text on the device: " + std::to_string(used + wanted) +
                        " bytes reached" + (cap ? " (max_device_bytes = " + std::to_string(cap) + ")" : std::string(" (the device is full)")));
    }
    template <class T>
    int alloc(T** p, size_t bytes) {
        if (cap && used + bytes > cap) return no_memory(bytes);
        void* q = nullptr;
        const hipError_t e = pool_alloc(h, &q, bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return no_memory(bytes);
        }
        STREAM_TRY(who, e);
        owned.push_back(q);
        used += bytes, reached = std::max(reached, used);
        *p = (T*)q;
        return ASM_OK;
    }
    void release(void* p, size_t bytes) { /* in stream order, like every block of the pool */
        owned.erase(std::find(owned.begin(), owned.end(), p));
        pool_free(h, p);
        used -= bytes;
    }

    /* A chunk's `total` SAM bytes (bam: BAM record bytes), sized and scanned (a.size, a.off): emitted into a block that stays, with
     * the chunk's line tables */
    template <bool PAIRED>
    int hold(SamArgs& a, unsigned long long total, bool bam) {
        const int64_t nlines = a.nlines;
        if ((uint64_t)st.lines + (uint64_t)nlines >= ((uint64_t)1 << 32)) return fail(h, ASM_EUNSUPPORTED, std::string(who) + ": 2^32 SAM lines or more");
        const size_t table = sizeof(unsigned long long) * (size_t)std::max<int64_t>(nlines, 1);
        Chunk c = {nullptr, nullptr, nullptr, nullptr, nlines};
        if (const int rc = alloc(&c.text, (size_t)total + SAM_SORT_PAD)) return rc;
        for (unsigned long long** t : {&c.key, &c.src, &c.size})
            if (const int rc = alloc(t, table)) return rc;
        a.out = c.text;
        STREAM_TRY(who, launch(h, line_kernels<PAIRED>(bam).emit, map_grid((uint64_t)nlines * 64, h), 256, a));
        if (nlines) STREAM_TRY(who, launch(h, sam_sort_key_kernel<PAIRED>, grid_for(nlines), ASM_BLOCK, a, n_seqs, c.key, c.src, c.size));
        chunks.push_back(c);
        st.lines += nlines, st.bytes_held += (int64_t)total;
        return ASM_OK;
    }

    /* After the last chunk: sort, offsets, and the lines gathered slab by slab (at most slab_cap bytes, or one line), one put each.
     * The output still has to be finished by the caller. */
    int flush(MapOutput& out, size_t slab_cap) {
        const auto t0 = std::chrono::steady_clock::now();
        const size_t n = (size_t)st.lines;
        if (n == 0) return ASM_OK;
        typedef unsigned long long u64;
        const size_t table = sizeof(u64) * n;
        /* the chunks' tables back to back; a chunk's own go back at once */
        u64 *key = nullptr, *src = nullptr, *size = nullptr;
        for (u64** t : {&key, &src, &size})
            if (const int rc = alloc(t, table)) return rc;
        size_t at = 0;
        for (Chunk& c : chunks) {
            const size_t bytes = sizeof(u64) * (size_t)c.nlines;
            u64* const from[3] = {c.key, c.src, c.size};
            u64* const to[3] = {key + at, src + at, size + at};
            for (int t = 0; t < 3; t++) {
                if (bytes) STREAM_TRY(who, hipMemcpyAsync(to[t], from[t], bytes, hipMemcpyDeviceToDevice, h->stream));
                release(from[t], sizeof(u64) * (size_t)std::max<int64_t>(c.nlines, 1));
            }
            c.key = c.src = c.size = nullptr;
            at += (size_t)c.nlines;
        }
        /* stable sort of (key, line number) over the key bits in use: POS and the bits of tid <= n_seqs */
        MapTmp tmp(h);
        u64* key_sorted = nullptr;
        uint32_t *idx = nullptr, *idx_sorted = nullptr;
        if (const int rc = alloc(&key_sorted, table)) return rc;
        if (const int rc = alloc(&idx, sizeof(uint32_t) * n)) return rc;
        if (const int rc = alloc(&idx_sorted, sizeof(uint32_t) * n)) return rc;
        STREAM_TRY(who, launch(h, sam_sort_iota_kernel, grid_for((int64_t)n), ASM_BLOCK, idx, (u64)n));
        int tid_bits = 0;
        while (((uint64_t)n_seqs >> tid_bits) != 0) tid_bits++;
        STREAM_TRY(who, map_sort_pairs(h, tmp, key, key_sorted, idx, idx_sorted, (uint32_t)n, 32 + tid_bits));
        release(key, table), release(key_sorted, table), release(idx, sizeof(uint32_t) * n);
        /* sources and sizes in output order, then the 64-bit output offsets (the scan's own count is 64-bit here: n + 1 may pass 2^31) */
        u64* psize = nullptr;
        if (const int rc = alloc(&psrc, table)) return rc;
        if (const int rc = alloc(&psize, table + sizeof(u64))) return rc;
        if (const int rc = alloc(&off, table + sizeof(u64))) return rc;
        STREAM_TRY(who, launch(h, sam_sort_permute_kernel, grid_for((int64_t)n + 1), ASM_BLOCK, (const uint32_t*)idx_sorted, (const u64*)src,
                               (const u64*)size, (u64)n, psrc, psize));
        size_t scan_bytes = 0;
        STREAM_TRY(who, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, psize, off, n + 1, h->stream));
        STREAM_TRY(who, tmp.reserve(scan_bytes));
        STREAM_TRY(who, hipcub::DeviceScan::ExclusiveSum(tmp.s.p, scan_bytes, psize, off, n + 1, h->stream));
        release(src, table), release(size, table), release(idx_sorted, sizeof(uint32_t) * n), release(psize, table + sizeof(u64));
        std::vector<uint64_t> h_off(n + 1);
        STREAM_TRY(who, fetch(h, {fetched((u64*)h_off.data(), (const u64*)off, n + 1)}));
        if (index) { /* the sizes of the record stream's blocks, as the stream frames them */
            nblk = bgzf_blocks((size_t)h_off[n]);
            if (const int rc = alloc(&blk_size, sizeof(u64) * (nblk + 1))) return rc;
            STREAM_TRY(who, hipMemsetAsync(blk_size, 0, sizeof(u64) * (nblk + 1), h->stream));
            out.bam->keep = blk_size;
        }
        const std::vector<size_t> cuts = asm_host::sam_slab_cuts(h_off.data(), n, slab_cap);
        for (size_t s = 0; s + 1 < cuts.size(); s++) {
            const size_t i0 = cuts[s], cnt = cuts[s + 1] - i0;
            const size_t bytes = (size_t)(h_off[cuts[s + 1]] - h_off[i0]);
            if (const int rc = out.put(bytes, [&](char* to) {
                    return launch(h, sam_line_gather_kernel, map_grid((uint64_t)cnt * SAM_GATHER_LANES, h), 256, (const u64*)psrc + i0,
                                  (const u64*)off + i0, (long)cnt, (u64)h_off[i0], to);
                }))
                return rc;
            st.slabs++;
        }
        st.seconds_sort = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return ASM_OK;
    }
};

#endif /* __HIPCC__ */

} /* extern "C++" */
