// The device-resident batch (asm_batch) and everything that makes, finishes, inspects and frees one: "scalars back, one wait" and
// hipcub's scratch, scan and sort (which the mapper and the file calls use too), the batch and its ownership, the pack launch, the
// tail resolver's host side, the bucket table, the one builder behind the five constructors (asm_batch_upload, asm_batch_generate,
// asm_batch_from_hits, batch_from_device_text for asm_batch_from_text and asm_stream_seq_file, map_greedy of asm_map_host.h) and the
// C ABI entries of batches and references.  asm_capi.hip includes this file inside an extern "C" block, behind the handle, the
// pool, the error path and the launch.
#pragma once

extern "C++" {

/* One copy of fetch(): `bytes` from device memory into host memory */
struct Fetch {
    void* dst;
    const void* src;
    size_t bytes;
};
template <class T>
static Fetch fetched(T* dst, const T* src, size_t count = 1) {
    return {dst, src, sizeof(T) * count};
}
/* "Scan, then read the totals": the copies to the host on the handle's stream, in order, and then one wait for all of them */
static hipError_t fetch(asm_handle* h, std::initializer_list<Fetch> what) {
    for (const Fetch& f : what)
        if (const hipError_t e = hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyDeviceToHost, h->stream)) return e;
    return hipStreamSynchronize(h->stream);
}

/* hipcub's temporary storage: grows to the largest request; the old block goes back to the pool in stream order */
struct MapTmp {
    Scratch<void> s;
    size_t cap = 0;
    explicit MapTmp(asm_handle* h) : s(h) {}
    hipError_t reserve(size_t bytes) {
        if (s.p && bytes <= cap) return hipSuccess;
        pool_free(s.h, s.p);
        s.p = nullptr, cap = bytes;
        return s.alloc(bytes + 16);
    }
};

/* hipcub's two-phase calls on the handle's stream: query the temporary size, reserve it, run */
template <class T>
static hipError_t map_exclusive_sum(asm_handle* h, MapTmp& tmp, T* in, T* out, int64_t n) {
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, h->stream);
    if (e == hipSuccess) e = tmp.reserve(bytes);
    return e != hipSuccess ? e : hipcub::DeviceScan::ExclusiveSum(tmp.s.p, bytes, in, out, (int)n, h->stream);
}
template <class K, class V, class N> /* stable: equal keys keep their order */
static hipError_t map_sort_pairs(asm_handle* h, MapTmp& tmp, K* key_in, K* key_out, V* val_in, V* val_out, N n, int end_bit) {
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, key_in, key_out, val_in, val_out, n, 0, end_bit, h->stream);
    if (e == hipSuccess) e = tmp.reserve(bytes);
    return e != hipSuccess ? e : hipcub::DeviceRadixSort::SortPairs(tmp.s.p, bytes, key_in, key_out, val_in, val_out, n, 0, end_bit, h->stream);
}

/* One width class of a batch: pairs whose longer string needs `w4` granules of 128 positions. */
struct asm_bucket {
    int64_t n = 0;
    int w4 = 1;
    int maxlen = 0;
    uint4* planes = nullptr;    /* uint4[4][w4][n], inside asm_batch::d_planes */
    uint32_t* lens = nullptr;   /* uint32[n],       inside asm_batch::d_lens   */
    uint32_t* order = nullptr;  /* bucket slot -> pair index; null when the batch is one bucket in input order */
    bool mixed = false;         /* one of several width classes of a mixed-length batch */
};

struct asm_batch {
    asm_handle* owner = nullptr; /* whose pool the device blocks come from */
    unsigned long long owner_serial = 0;
    int64_t n = 0;
    int maxlen = 0;              /* the longest string, or a bound on it: see BatchBuild */
    int greedy_mode = ASM_GREEDY_CLEAN;
    size_t reads_bytes = 0, refs_bytes = 0;
    char* d_reads = nullptr;
    char* d_refs = nullptr;
    uint32_t* d_read_off = nullptr;
    uint32_t* d_ref_off = nullptr;
    uint4* d_planes = nullptr;  /* all buckets back to back */
    uint32_t* d_lens = nullptr; /* in bucketed order */
    uint32_t* d_order = nullptr; /* bucketed slot -> pair index (null: identity) */
    uint32_t* d_pos = nullptr;   /* pair index -> bucketed slot (null: identity) */
    /* pipelined repack (asm_run_benchmark_async, repack = 2): a second set of planes/lens that the next call's pack fills
     * while this call's aligners still read the current one */
    uint4* d_planes_alt = nullptr;
    uint32_t* d_lens_alt = nullptr;
    size_t planes_total = 0;     /* uint4 entries in d_planes */
    hipEvent_t ev_consumed[2] = {nullptr, nullptr}; /* aligners of the call that used buffer q are done */
    int cur = 0;
    uint4* d_tails = nullptr;    /* sequential mode: stale-tail planes, uint4[4][n] in input order */
    uint4* d_tail_g0 = nullptr;  /* tail resolver scratch (asm_tails.h), allocated on first use: clean granule 0 in input order, */
    uint32_t* d_tail_l0 = nullptr; /* its lengths, */
    uint8_t* d_tail_chunks = nullptr; /* per-chunk prefixes, per-workgroup totals and carries + the 256-byte summary */
    int nb = 1;
    asm_bucket bk[4];
    PackBuckets pb;
};

struct asm_reference {
    char* d_text = nullptr;
    size_t len = 0;
};

/* The only place that frees a batch's device blocks (its owner is live). */
static void batch_release(asm_batch* b) {
    if (!b) return;
    asm_handle* const o = b->owner;
    /* the pool hands blocks out again in the order of o->stream; overlapped calls that were never joined may still read these
     * on the library's own streams */
    (void)o->pipe.join_into(o->stream);
    for (void* p : {(void*)b->d_reads, (void*)b->d_refs, (void*)b->d_read_off, (void*)b->d_ref_off, (void*)b->d_planes, (void*)b->d_lens,
                    (void*)b->d_planes_alt, (void*)b->d_lens_alt, (void*)b->d_order, (void*)b->d_pos, (void*)b->d_tails,
                    (void*)b->d_tail_g0, (void*)b->d_tail_l0, (void*)b->d_tail_chunks})
        pool_free(o, p);
    for (hipEvent_t ev : b->ev_consumed)
        if (ev) (void)hipEventDestroy(ev);
    delete b;
}

struct BatchRelease {
    void operator()(asm_batch* b) const { batch_release(b); }
};
using BatchPtr = std::unique_ptr<asm_batch, BatchRelease>; /* a batch under construction, or a streamed chunk's */

/* A new, empty batch of n pairs whose device blocks will come from h's pool. */
static int batch_new(asm_handle* h, int64_t n, int greedy_mode, const char* who, BatchPtr& b) {
    if (greedy_mode != ASM_GREEDY_CLEAN && greedy_mode != ASM_GREEDY_SEQUENTIAL)
        return fail(h, ASM_EINVAL, std::string(who) + ": unknown greedy_mode");
    b.reset(new asm_batch);
    b->owner = h, b->owner_serial = h->serial;
    b->n = n;
    b->greedy_mode = greedy_mode;
    return ASM_OK;
}

/* Every device block a batch owns comes from its owner's pool, whichever handle the call came through: batch_release returns
 * it there. */
template <typename T>
static hipError_t batch_alloc(asm_batch* b, T** p, size_t bytes) {
    return pool_alloc(b->owner, (void**)p, bytes);
}

static hipError_t launch_pack(asm_handle* h, const asm_batch* b, const uint4* tails, uint4* planes, uint32_t* lens,
                              const PackBuckets& pb, const uint32_t* pos) {
    int wmax = 1;
    for (int q = 0; q < pb.nb; q++) wmax = pb.w4[q] > wmax ? pb.w4[q] : wmax;
    // LDS: the plane arrays of both sides of 256 strings of the batch's longest length (+ alignment slack), capped; at least
    // one string's (the rounds path then makes progress)
    const auto side_dwords = [](size_t bytes) { return (size_t)2 * (size_t)(((bytes + 15) / 16 + 1) / 2 + 1); };
    size_t dw = 2 * side_dwords((size_t)PACK_BLOCK * (size_t)b->maxlen + 15);
    if (dw > PACK_LDS_MAX / 4) dw = PACK_LDS_MAX / 4;
    if (dw < side_dwords((size_t)b->maxlen + 30)) dw = side_dwords((size_t)b->maxlen + 30);
    return with_const<1, 4>(wmax, [&](auto w) {
        return launch_lds(h, pack_kernel<decltype(w)::value>, (unsigned)((b->n + PACK_BLOCK - 1) / PACK_BLOCK), PACK_BLOCK, dw * 4,
                          b->d_reads, b->d_read_off, b->d_refs, b->d_ref_off, tails, planes, lens, (long)b->n, pb, pos, (uint32_t)dw);
    });
}

/* The bucket table of n pairs of which counts[c] are in width class c (c + 1 granules): what the pack kernel reads (pb), the
 * buckets without their pointers, their number and the planes' uint4 entries.  An empty batch has one empty bucket of class 0. */
struct BucketTable {
    PackBuckets pb{};
    asm_bucket bk[4];
    int nb = 0;
    size_t planes_total = 0;
};
static BucketTable bucket_table(const unsigned int (&counts)[4], int64_t n, int maxlen) {
    BucketTable t;
    int64_t slot = 0;
    for (int c = 0; c < 4; c++) {
        if (!counts[c] && !(n == 0 && c == 0)) continue;
        asm_bucket& k = t.bk[t.nb];
        k.n = counts[c], k.w4 = c + 1, k.maxlen = std::min(maxlen, 128 * (c + 1));
        t.pb.w4[t.nb] = k.w4, t.pb.start[t.nb] = slot, t.pb.plane_off[t.nb] = (long)t.planes_total;
        t.planes_total += (size_t)4 * (size_t)k.w4 * (size_t)k.n;
        slot += k.n, t.nb++;
    }
    t.pb.nb = t.nb, t.pb.start[t.nb] = slot;
    return t;
}

} /* extern "C++" */

int asm_batch_pack_async(asm_handle* h, asm_batch* b) {
    if (!h || !b) return fail(h, ASM_EINVAL, "asm_batch_pack_async: NULL argument");
    if (b->n == 0) return ASM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_pack(h, b, b->d_tails, b->d_planes, b->d_lens, b->pb, b->d_pos));
    return ASM_OK;
}

/* ASM_GREEDY_SEQUENTIAL: derive the stale buffer tails on the device (asm_tails.h).  The resolver walks the pairs
 * in INPUT order and only needs granule 0, so it works on a temporary clean-mode, unbucketed, one-granule packing.
 * init256 (host, optional): buffer codes before the batch's first pair; summary256 (host, optional): the batch's effect on
 * the buffers (see tails_carry_kernel); emit = false stops after the summary (b->d_tails untouched). */
static int batch_resolve_tails(asm_handle* h, asm_batch* b, const uint8_t* init256, uint8_t* summary256, bool emit) {
    if (summary256) memset(summary256, TAIL_NONE, 256);
    if (b->n == 0) return ASM_OK;
    const long nchunks = (b->n + TAIL_CHUNK - 1) / TAIL_CHUNK;
    const long ngroups = (nchunks + TAIL_GROUP - 1) / TAIL_GROUP;
    TailState init;
    if (init256) memcpy(init.code, init256, 256);
    else memset(init.code, 0, 256);
    /* scratch lives with the batch: a streamed file re-resolves every chunk, a bench step every iteration */
    if (emit && !b->d_tails) HIPCHK(h, batch_alloc(b, &b->d_tails, sizeof(uint4) * 4 * (size_t)b->n));
    const size_t loc_bytes = (size_t)ngroups * TAIL_GROUP * 2 * sizeof(TailOp), grp_bytes = (size_t)ngroups * 2 * sizeof(TailOp);
    const size_t carry_bytes = (size_t)ngroups * 2 * 2 * sizeof(uint4);
    if (!b->d_tail_g0) HIPCHK(h, batch_alloc(b, &b->d_tail_g0, sizeof(uint4) * 4 * (size_t)b->n));
    if (!b->d_tail_l0) HIPCHK(h, batch_alloc(b, &b->d_tail_l0, sizeof(uint32_t) * (size_t)b->n));
    if (!b->d_tail_chunks) HIPCHK(h, batch_alloc(b, &b->d_tail_chunks, loc_bytes + grp_bytes + carry_bytes + 256)); /* loc, grp, gcarry, summary[256] */
    TailOp* const d_loc = (TailOp*)b->d_tail_chunks;
    TailOp* const d_grp = (TailOp*)(b->d_tail_chunks + loc_bytes);
    uint4* const d_carry = (uint4*)(b->d_tail_chunks + loc_bytes + grp_bytes);
    uint8_t* const d_sum = b->d_tail_chunks + loc_bytes + grp_bytes + carry_bytes;
    const unsigned int one_class[4] = {(unsigned int)b->n, 0, 0, 0};
    HIPCHK(h, launch_pack(h, b, nullptr, b->d_tail_g0, b->d_tail_l0, bucket_table(one_class, b->n, b->maxlen).pb, nullptr));
    HIPCHK(h, launch(h, tails_chunk_kernel, (unsigned)ngroups, 2 * TAIL_GROUP, b->d_tail_g0, b->d_tail_l0, (long)b->n, d_loc, d_grp));
    HIPCHK(h, launch(h, tails_carry_kernel, 1, 8 * TAIL_CARRY_SEGS, (const uint32_t*)d_grp, (uint32_t*)d_carry, ngroups, init,
                     summary256 ? d_sum : (uint8_t*)nullptr));
    if (emit)
        HIPCHK(h, launch(h, tails_emit_kernel, (unsigned)ngroups, 2 * TAIL_GROUP, b->d_tail_g0, b->d_tail_l0, (long)b->n,
                         (const TailOp*)d_loc, (const uint4*)d_carry, b->d_tails));
    if (summary256) HIPCHK(h, fetch(h, {fetched(summary256, (const uint8_t*)d_sum, 256)}));
    return ASM_OK;
}

/* Common tail of every constructor once ASCII + offsets are resident and b->maxlen is known: group the pairs into width
 * classes (only when the batch really mixes classes), allocate the packed form, resolve tails, pack. */
static int batch_finish(asm_handle* h, asm_batch* b) {
    const int64_t n = b->n;
    const int wmax = b->maxlen <= 128 ? 1 : (b->maxlen + 127) / 128;
    unsigned int counts[4] = {0, 0, 0, 0};
    bool bucketed = false;
    if (wmax > 1 && n >= 4096 && h->bucketing) {
        Scratch<uint8_t> d_cls(h), d_cls2(h);
        Scratch<uint32_t> d_idx(h);
        Scratch<unsigned int> d_counts(h);
        MapTmp tmp(h);
        HIPCHK(h, d_cls.alloc((size_t)n));
        HIPCHK(h, d_cls2.alloc((size_t)n));
        HIPCHK(h, d_idx.alloc(sizeof(uint32_t) * (size_t)n));
        HIPCHK(h, d_counts.alloc(16));
        HIPCHK(h, hipMemsetAsync(d_counts.p, 0, 16, h->stream));
        HIPCHK(h, launch(h, classify_kernel, grid_for(n), ASM_BLOCK, b->d_read_off, b->d_ref_off, (long)n, d_cls.p, d_idx.p, d_counts.p));
        HIPCHK(h, fetch(h, {fetched(counts, (const unsigned int*)d_counts.p, 4)}));
        bucketed = (counts[0] != 0) + (counts[1] != 0) + (counts[2] != 0) + (counts[3] != 0) > 1;
        if (bucketed) {
            HIPCHK(h, batch_alloc(b, &b->d_order, sizeof(uint32_t) * (size_t)n));
            HIPCHK(h, batch_alloc(b, &b->d_pos, sizeof(uint32_t) * (size_t)n));
            HIPCHK(h, map_sort_pairs(h, tmp, d_cls.p, d_cls2.p, d_idx.p, b->d_order, (int)n, 2)); /* stable: input order is kept inside a class */
            HIPCHK(h, launch(h, invert_order_kernel, grid_for(n), ASM_BLOCK, b->d_order, (long)n, b->d_pos));
        }
    }
    if (!bucketed) {
        counts[0] = counts[1] = counts[2] = counts[3] = 0;
        counts[wmax - 1] = (unsigned int)n;
    }
    const BucketTable t = bucket_table(counts, n, b->maxlen);
    b->pb = t.pb, b->nb = t.nb;
    b->planes_total = std::max<size_t>(t.planes_total, 1);
    HIPCHK(h, batch_alloc(b, &b->d_planes, sizeof(uint4) * b->planes_total));
    HIPCHK(h, batch_alloc(b, &b->d_lens, sizeof(uint32_t) * (size_t)std::max<int64_t>(n, 1)));
    for (int q = 0; q < b->nb; q++) {
        b->bk[q] = t.bk[q];
        b->bk[q].planes = b->d_planes + b->pb.plane_off[q];
        b->bk[q].lens = b->d_lens + b->pb.start[q];
        b->bk[q].order = b->d_order ? b->d_order + b->pb.start[q] : nullptr;
        b->bk[q].mixed = bucketed;
    }
    int rc = b->greedy_mode == ASM_GREEDY_SEQUENTIAL ? batch_resolve_tails(h, b, nullptr, nullptr, true) : ASM_OK;
    if (!rc) rc = asm_batch_pack_async(h, b);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ASM_OK;
}

/* ---- The builder: what every constructor runs between its argument checks and its fill step -------------------------------------
 * A constructor is its argument checks, its lengths step, these calls in this order, its fill step and batch_finish:
 *   bound(maxlen)                  only where the caller knows a bound on the longest string; refused at once when too long
 *   offsets_from_host(side, off)   the caller's n + 1 offsets (checked by host_offsets_ok), uploaded; the side's bytes = off[n]
 *   offsets_from_lengths(side, l)  a device array of lengths, scanned into the side's offsets
 *   totals()                       both totals, and the measured maximum where no bound was given, with ONE wait on the stream
 *                                  (asm_batch_upload knows everything on the host and skips it)
 *   text_blocks()                  the refusal of a maximum above ASM_MAX_LENGTH, then d_reads and d_refs: their bytes + 16 of slack
 * Lengths convention: a device length array holds n + 1 entries and the last one is ZERO, so that the exclusive scan over n + 1
 * entries leaves the total in offsets[n]; the lengths step writes that zero.
 * b->maxlen selects the width class, the plane layout and the kernel instantiation.  It is one of two things, and stays what the
 * constructor made it: MEASURED, the longest string of either side (upload, generate, text: seq_max_kernel over both length
 * arrays, or the host loop), or a BOUND that the caller passes to bound(): longest read + 1 for the seed-hit windows of
 * asm_batch_from_hits and map_greedy, whose windows may all be shorter (clipped at the end of the reference). */
enum { BATCH_READS = 0, BATCH_REFS = 1 };
struct BatchBuild {
    asm_handle* h;
    asm_batch* b;
    int refuse_code; /* the constructor's own code and text for a string longer than ASM_MAX_LENGTH */
    const char* refuse_text;
    MapTmp tmp;
    const uint32_t* d_len[2] = {nullptr, nullptr}; /* the scanned sides' lengths: their totals are still on the device */
    bool bounded = false;
    BatchBuild(asm_handle* handle, asm_batch* batch, int code, const char* text)
        : h(handle), b(batch), refuse_code(code), refuse_text(text), tmp(handle) {}
    int refuse() const { return b->maxlen > ASM_MAX_LENGTH ? fail(h, refuse_code, refuse_text) : ASM_OK; }
    int bound(int maxlen) {
        b->maxlen = maxlen, bounded = true;
        return refuse();
    }
    int offsets_from_host(int side, const uint32_t* host_off) {
        uint32_t*& d_off = side == BATCH_READS ? b->d_read_off : b->d_ref_off;
        const size_t bytes = sizeof(uint32_t) * ((size_t)b->n + 1);
        HIPCHK(h, batch_alloc(b, &d_off, bytes));
        HIPCHK(h, hipMemcpyAsync(d_off, host_off, bytes, hipMemcpyHostToDevice, h->stream));
        (side == BATCH_READS ? b->reads_bytes : b->refs_bytes) = b->n ? host_off[b->n] : 0;
        return ASM_OK;
    }
    int offsets_from_lengths(int side, uint32_t* lens) {
        uint32_t*& d_off = side == BATCH_READS ? b->d_read_off : b->d_ref_off;
        HIPCHK(h, batch_alloc(b, &d_off, sizeof(uint32_t) * ((size_t)b->n + 1)));
        HIPCHK(h, map_exclusive_sum(h, tmp, lens, d_off, b->n + 1));
        d_len[side] = lens;
        return ASM_OK;
    }
    int totals() { /* measuring needs both sides' lengths on the device: every constructor without a bound has them */
        Scratch<uint32_t> d_max(h);
        uint32_t tot[2] = {0, 0}, mx = 0;
        const Fetch t0 = fetched(&tot[0], (const uint32_t*)b->d_read_off + b->n), t1 = fetched(&tot[1], (const uint32_t*)b->d_ref_off + b->n);
        if (bounded) {
            HIPCHK(h, fetch(h, {t0, t1}));
        } else {
            HIPCHK(h, d_max.alloc(16));
            HIPCHK(h, hipMemsetAsync(d_max.p, 0, 16, h->stream));
            if (b->n > 0)
                HIPCHK(h, launch(h, seq_max_kernel, (unsigned)std::min(grid_for(b->n), 1024), ASM_BLOCK, d_len[0], d_len[1], (long)b->n, d_max.p));
            HIPCHK(h, fetch(h, {t0, t1, fetched(&mx, (const uint32_t*)d_max.p)}));
            b->maxlen = (int)mx;
        }
        if (d_len[BATCH_READS]) b->reads_bytes = tot[0];
        if (d_len[BATCH_REFS]) b->refs_bytes = tot[1];
        return ASM_OK;
    }
    int text_blocks() {
        if (const int rc = refuse()) return rc;
        HIPCHK(h, batch_alloc(b, &b->d_reads, b->reads_bytes + 16));
        HIPCHK(h, batch_alloc(b, &b->d_refs, b->refs_bytes + 16));
        return ASM_OK;
    }
};

/* The caller's n + 1 offsets of one side: non-decreasing?  maxlen is raised to the longest string. */
static bool host_offsets_ok(const uint32_t* off, int64_t n, int& maxlen) {
    for (int64_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return false;
        maxlen = std::max(maxlen, (int)(off[i + 1] - off[i]));
    }
    return true;
}

/* The last step of a public constructor: finish the batch and only then hand it to the caller. */
static int batch_finish_into(asm_handle* h, BatchPtr& b, asm_batch** out) {
    if (const int rc = batch_finish(h, b.get())) return rc;
    *out = b.release();
    return ASM_OK;
}

/* out[off[i], off[i + 1]) = text[start[i], ...) for n strings (text_gather_kernel, asm_ingest.h): one wave per string, four per
 * workgroup, at most 4096 workgroups */
static hipError_t launch_text_gather(asm_handle* h, const char* text, const unsigned long long* start, const uint32_t* off, int64_t n,
                                     char* out) {
    if (n <= 0) return hipSuccess;
    return launch(h, text_gather_kernel, (unsigned)std::min<int64_t>((n + 3) / 4, 256 * 16), ASM_BLOCK, text, start, off, (long)n, out);
}

int asm_batch_upload(asm_handle* h, int64_t n, const char* reads, const uint32_t* read_off, const char* refs,
                     const uint32_t* ref_off, int greedy_mode, asm_batch** out) {
    if (!h || !out || n < 0 || !read_off || !ref_off || (n > 0 && (!reads || !refs)))
        return fail(h, ASM_EINVAL, "asm_batch_upload: bad arguments");
    BatchPtr b;
    int rc = batch_new(h, n, greedy_mode, "asm_batch_upload", b);
    if (rc) return rc;
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    int maxlen = 0;
    if (!host_offsets_ok(read_off, n, maxlen) || !host_offsets_ok(ref_off, n, maxlen))
        return fail(h, ASM_EINVAL, "asm_batch_upload: offsets must be non-decreasing");
    BatchBuild bb(h, b.get(), ASM_EUNSUPPORTED, "asm_batch_upload: a sequence is longer than ASM_MAX_LENGTH");
    rc = bb.bound(maxlen); /* measured on the host: the bound is the maximum */
    if (!rc) rc = bb.offsets_from_host(BATCH_READS, read_off);
    if (!rc) rc = bb.offsets_from_host(BATCH_REFS, ref_off);
    if (!rc) rc = bb.text_blocks();
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(b->d_reads, reads, b->reads_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(b->d_refs, refs, b->refs_bytes, hipMemcpyHostToDevice, h->stream));
    return batch_finish_into(h, b, out);
}

int asm_batch_generate(asm_handle* h, const asm_gen_config* cfg, int64_t first, int64_t n, int greedy_mode,
                       asm_batch** out) {
    if (!h || !out || n < 0 || first < 0) return fail(h, ASM_EINVAL, "asm_batch_generate: bad arguments");
    std::string err;
    int rc = asm_host::check_gen(cfg, err);
    if (rc) return fail(h, rc, err);
    BatchPtr b;
    rc = batch_new(h, n, greedy_mode, "asm_batch_generate", b);
    if (rc) return rc;
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    BatchBuild bb(h, b.get(), ASM_EUNSUPPORTED, "asm_batch_generate: a generated sequence exceeds ASM_MAX_LENGTH");
    Scratch<uint32_t> d_m(h), d_n(h);
    HIPCHK(h, d_m.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    HIPCHK(h, d_n.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    HIPCHK(h, hipMemsetAsync(d_m.p + n, 0, sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d_n.p + n, 0, sizeof(uint32_t), h->stream));
    if (n > 0) HIPCHK(h, launch(h, gen_lengths_kernel, grid_for(n), ASM_BLOCK, *cfg, (long)first, (long)n, d_m.p, d_n.p));
    rc = bb.offsets_from_lengths(BATCH_READS, d_m.p);
    if (!rc) rc = bb.offsets_from_lengths(BATCH_REFS, d_n.p);
    if (!rc) rc = bb.totals();
    if (rc) return rc;
    /* 32-bit offsets: the host-side bound (n * worst length) must stay below 4 GiB */
    if ((double)n * (double)(cfg->len_hi * 2 + 2) >= 4294967295.0 && (double)n * (double)b->maxlen >= 4294967295.0)
        return fail(h, ASM_EUNSUPPORTED, "asm_batch_generate: batch exceeds 4 GiB of text; split it");
    rc = bb.text_blocks();
    if (rc) return rc;
    if (n > 0)
        HIPCHK(h, launch(h, gen_fill_kernel, (unsigned)((n + 63) / 64), 64, *cfg, (long)first, (long)n, b->d_read_off, b->d_ref_off,
                         b->d_reads, b->d_refs));
    return batch_finish_into(h, b, out);
}

int asm_reference_upload(asm_handle* h, const char* text, size_t len, asm_reference** out) {
    if (!h || !out || (!text && len)) return fail(h, ASM_EINVAL, "asm_reference_upload: bad argument");
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    asm_reference* r = new asm_reference;
    r->len = len;
    if (big_malloc(h, (void**)&r->d_text, len + 16) != hipSuccess) {
        delete r;
        return fail(h, ASM_ENOMEM, "asm_reference_upload: hipMalloc failed");
    }
    if (len && hipMemcpy(r->d_text, text, len, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(r->d_text);
        delete r;
        return fail(h, ASM_ENODEVICE, "asm_reference_upload: copy failed");
    }
    *out = r;
    return ASM_OK;
}

int asm_reference_free(asm_handle* h, asm_reference* r) {
    if (h) (void)hipSetDevice(h->device);
    if (r) {
        (void)hipFree(r->d_text);
        delete r;
    }
    return ASM_OK;
}

int asm_batch_from_hits(asm_handle* h, const asm_reference* ref, int64_t n, const char* reads, const uint32_t* read_off,
                        const uint64_t* hit_pos, int greedy_mode, asm_batch** out) {
    if (!h || !ref || !out || n < 0 || !read_off || (n > 0 && (!reads || !hit_pos)))
        return fail(h, ASM_EINVAL, "asm_batch_from_hits: bad arguments");
    BatchPtr b;
    int rc = batch_new(h, n, greedy_mode, "asm_batch_from_hits", b);
    if (rc) return rc;
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    int maxlen = 0;
    if (!host_offsets_ok(read_off, n, maxlen)) return fail(h, ASM_EINVAL, "asm_batch_from_hits: offsets must be non-decreasing");
    BatchBuild bb(h, b.get(), ASM_EUNSUPPORTED, "asm_batch_from_hits: a read is longer than ASM_MAX_LENGTH - 1");
    rc = bb.bound(maxlen + 1); /* the window is one base longer than the read (mapper/main.cpp:80) */
    if (!rc) rc = bb.offsets_from_host(BATCH_READS, read_off);
    if (rc) return rc;
    Scratch<unsigned long long> d_pos(h), d_start(h);
    Scratch<uint32_t> d_wl(h);
    HIPCHK(h, d_pos.alloc(sizeof(unsigned long long) * ((size_t)n + 1)));
    HIPCHK(h, d_start.alloc(sizeof(unsigned long long) * ((size_t)n + 1)));
    HIPCHK(h, d_wl.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    if (n) HIPCHK(h, hipMemcpyAsync(d_pos.p, hit_pos, sizeof(unsigned long long) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch(h, hit_window_lengths_kernel, grid_for(n + 1), ASM_BLOCK, b->d_read_off, d_pos.p, (unsigned long long)ref->len,
                     (long)n, d_wl.p, d_start.p));
    rc = bb.offsets_from_lengths(BATCH_REFS, d_wl.p);
    if (!rc) rc = bb.totals();
    if (!rc) rc = bb.text_blocks();
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(b->d_reads, reads, b->reads_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_text_gather(h, ref->d_text, d_start.p, b->d_ref_off, n, b->d_refs));
    return batch_finish_into(h, b, out);
}

extern "C++" {
/* d_nl[l] = the position of the l-th newline of d_raw[0, nbytes), for the first `lines` of them (asm_ingest.h); d_tbase: per tile of
 * SEQ_TILE bytes, the newlines before it */
static hipError_t newline_index(asm_handle* h, MapTmp& tmp, const char* d_raw, size_t nbytes, long lines, uint32_t* d_nl,
                                Scratch<uint32_t>& d_tbase) {
    const long ntiles = (long)((nbytes + SEQ_TILE - 1) / SEQ_TILE);
    Scratch<uint32_t> d_tile(h);
    hipError_t e = d_tile.alloc(sizeof(uint32_t) * ((size_t)ntiles + 1));
    if (e == hipSuccess) e = d_tbase.alloc(sizeof(uint32_t) * ((size_t)ntiles + 1));
    if (e == hipSuccess) e = launch(h, seq_count_kernel, (unsigned)ntiles, 256, d_raw, (long)nbytes, d_tile.p);
    if (e == hipSuccess) e = map_exclusive_sum(h, tmp, d_tile.p, d_tbase.p, (int64_t)ntiles);
    if (e != hipSuccess) return e;
    return launch(h, seq_index_kernel, (unsigned)ntiles, 256, d_raw, (long)nbytes, (const uint32_t*)d_tbase.p, d_nl, lines);
}
static hipError_t newline_index(asm_handle* h, MapTmp& tmp, const char* d_raw, size_t nbytes, long lines, uint32_t* d_nl) {
    Scratch<uint32_t> d_tbase(h);
    return newline_index(h, tmp, d_raw, nbytes, lines, d_nl, d_tbase);
}
} /* extern "C++" */

/* Fills batch b (n pairs = 2n lines, every line ending in '\n') out of raw text already in HBM: a `>read\n<ref\n` text
 * (benchmark_utils.h:325-352), parsed on the device (asm_ingest.h). */
static int batch_from_device_text(asm_handle* h, const char* d_raw, size_t nbytes, asm_batch* b) {
    const int64_t n = b->n;
    const size_t cnt = (size_t)n + 1;
    BatchBuild bb(h, b, ASM_EUNSUPPORTED, "streamed file: a sequence is longer than ASM_MAX_LENGTH");
    Scratch<uint32_t> d_nl(h), d_m(h), d_n(h);
    Scratch<unsigned long long> d_sa(h), d_sb(h);
    HIPCHK(h, d_m.alloc(sizeof(uint32_t) * cnt));
    HIPCHK(h, d_n.alloc(sizeof(uint32_t) * cnt));
    HIPCHK(h, d_sa.alloc(sizeof(unsigned long long) * cnt));
    HIPCHK(h, d_sb.alloc(sizeof(unsigned long long) * cnt));
    HIPCHK(h, d_nl.alloc(sizeof(uint32_t) * (2 * (size_t)n + 2)));
    if (n > 0) HIPCHK(h, newline_index(h, bb.tmp, d_raw, nbytes, (long)(2 * n), d_nl.p));
    HIPCHK(h, launch(h, seq_lengths_kernel, grid_for(n + 1), ASM_BLOCK, (const uint32_t*)d_nl.p, (long)n, d_m.p, d_n.p, d_sa.p, d_sb.p));
    int rc = bb.offsets_from_lengths(BATCH_READS, d_m.p);
    if (!rc) rc = bb.offsets_from_lengths(BATCH_REFS, d_n.p);
    if (!rc) rc = bb.totals();
    if (!rc) rc = bb.text_blocks();
    if (rc) return rc;
    HIPCHK(h, launch_text_gather(h, d_raw, d_sa.p, b->d_read_off, n, b->d_reads));
    HIPCHK(h, launch_text_gather(h, d_raw, d_sb.p, b->d_ref_off, n, b->d_refs));
    return batch_finish(h, b);
}

int asm_batch_from_text(asm_handle* h, const char* text, size_t nbytes, int greedy_mode, asm_batch** out) {
    if (!h || !out || (!text && nbytes)) return fail(h, ASM_EINVAL, "asm_batch_from_text: bad argument");
    BatchPtr b;
    int rc = batch_new(h, 0, greedy_mode, "asm_batch_from_text", b);
    if (rc) return rc;
    if (nbytes >= 0xfffffff0ull) return fail(h, ASM_EUNSUPPORTED, "asm_batch_from_text: more than 4 GiB of text; split it");
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    const bool open_line = nbytes && text[nbytes - 1] != '\n';
    int64_t lines = asm_host::scan_newlines(text, nbytes, 8).count + (open_line ? 1 : 0);
    const bool odd = (lines & 1) != 0; /* a read without its reference line: the reference gets an empty string there */
    const size_t total = nbytes + (open_line ? 1 : 0) + (odd ? 1 : 0);
    lines += odd ? 1 : 0;
    Scratch<char> d_raw(h);
    HIPCHK(h, d_raw.alloc(total + 32));
    if (nbytes) HIPCHK(h, hipMemcpyAsync(d_raw.p, text, nbytes, hipMemcpyHostToDevice, h->stream));
    if (total > nbytes) HIPCHK(h, hipMemsetAsync(d_raw.p + nbytes, '\n', total - nbytes, h->stream));
    b->n = lines / 2;
    rc = batch_from_device_text(h, d_raw.p, total, b.get());
    if (rc) return rc;
    *out = b.release();
    return ASM_OK;
}

/* ---- Greedy sequential mode across batches: shards of one file on several GPUs, or chunks of a streamed file ---- */
int asm_batch_tail_summary(asm_handle* h, const asm_batch* b, uint8_t* summary) {
    if (!h || !b || !summary) return fail(h, ASM_EINVAL, "asm_batch_tail_summary: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    return batch_resolve_tails(h, const_cast<asm_batch*>(b), nullptr, summary, false);
}

int asm_tail_state_advance(uint8_t* state, const uint8_t* summary, int64_t n_pairs) {
    std::string err;
    const int rc = asm_host::tail_state_advance(state, summary, n_pairs, err);
    return rc ? fail(nullptr, rc, err) : ASM_OK;
}

int asm_batch_resolve_tails(asm_handle* h, asm_batch* b, const uint8_t* state) {
    if (!h || !b) return fail(h, ASM_EINVAL, "asm_batch_resolve_tails: NULL argument");
    if (state)
        for (int q = 0; q < 256; q++)
            if (state[q] > 3) return fail(h, ASM_EINVAL, "asm_batch_resolve_tails: state entries are 2-bit codes (0..3)");
    HIPCHK(h, hipSetDevice(h->device));
    b->greedy_mode = ASM_GREEDY_SEQUENTIAL;
    int rc = batch_resolve_tails(h, b, state, nullptr, true);
    if (!rc) rc = asm_batch_pack_async(h, b);
    return rc;
}

int asm_batch_free(asm_handle* h, asm_batch* b) {
    if (!b) return ASM_OK;
    /* The device blocks belong to the pool of the handle that created the batch, whichever handle is named here (h may be NULL):
     * they go back THERE.  The owner is named by (address, serial): if that handle is gone — asm_destroy has released every
     * block of its pool, this batch's included — only the record is left, also when a NEW handle lives at the old address.
     * Look-up and release happen under one lock, so the owner cannot be destroyed in between. */
    (void)h;
    std::lock_guard<std::mutex> lk(g_live_mu);
    if (!owner_is_live_locked(b->owner, b->owner_serial)) {
        for (hipEvent_t ev : b->ev_consumed) /* events belong to the device context, not to the handle */
            if (ev) (void)hipEventDestroy(ev);
        delete b;
        return ASM_OK;
    }
    (void)hipSetDevice(b->owner->device);
    batch_release(b);
    return ASM_OK;
}

int64_t asm_batch_size(const asm_batch* b) { return b ? b->n : 0; }
int asm_batch_max_length(const asm_batch* b) { return b ? b->maxlen : 0; }
int64_t asm_batch_text_bytes(const asm_batch* b) { return b ? (int64_t)(b->reads_bytes + b->refs_bytes) : 0; }

int asm_batch_download(asm_handle* h, const asm_batch* b, uint32_t* read_off, uint32_t* ref_off, char* reads,
                       size_t reads_cap, char* refs, size_t refs_cap) {
    if (!h || !b) return fail(h, ASM_EINVAL, "asm_batch_download: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (read_off) HIPCHK(h, hipMemcpy(read_off, b->d_read_off, sizeof(uint32_t) * (size_t)(b->n + 1), hipMemcpyDeviceToHost));
    if (ref_off) HIPCHK(h, hipMemcpy(ref_off, b->d_ref_off, sizeof(uint32_t) * (size_t)(b->n + 1), hipMemcpyDeviceToHost));
    if (reads) {
        if (reads_cap < b->reads_bytes) return fail(h, ASM_EINVAL, "asm_batch_download: reads buffer too small");
        HIPCHK(h, hipMemcpy(reads, b->d_reads, b->reads_bytes, hipMemcpyDeviceToHost));
    }
    if (refs) {
        if (refs_cap < b->refs_bytes) return fail(h, ASM_EINVAL, "asm_batch_download: refs buffer too small");
        HIPCHK(h, hipMemcpy(refs, b->d_refs, b->refs_bytes, hipMemcpyDeviceToHost));
    }
    return ASM_OK;
}

int64_t asm_batch_planes_size(const asm_batch* b) { return b ? (int64_t)b->planes_total : 0; }

int asm_batch_download_planes(asm_handle* h, const asm_batch* b, uint32_t* planes, size_t planes_cap, uint32_t* lens,
                              uint32_t* order) {
    if (!h || !b) return fail(h, ASM_EINVAL, "asm_batch_download_planes: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t n = (size_t)b->n;
    if (planes) {
        if (planes_cap < 4 * b->planes_total) return fail(h, ASM_EINVAL, "asm_batch_download_planes: planes buffer too small");
        HIPCHK(h, hipMemcpy(planes, b->d_planes, sizeof(uint4) * b->planes_total, hipMemcpyDeviceToHost));
    }
    if (lens && n) HIPCHK(h, hipMemcpy(lens, b->d_lens, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    if (order && n) {
        if (b->d_order) HIPCHK(h, hipMemcpy(order, b->d_order, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        else
            for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    }
    return ASM_OK;
}
