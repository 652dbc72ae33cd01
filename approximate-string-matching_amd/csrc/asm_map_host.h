// Host side of the read mapper (kernels: asm_map.h; design: docs/design/mapper.md): the index, the stages every mapping call is
// made of (check -> front -> seeding rounds -> runs -> select / pair -> finish stage -> scatter) and the C ABI entry points.
// asm_capi.hip includes this file inside its extern "C" block: the stages (templates among them) get C++ linkage below, the entry
// points after them C linkage.
#pragma once

static_assert(sizeof(MapHit) == sizeof(asm_map_hit) && offsetof(MapHit, dist) == offsetof(asm_map_hit, dist) &&
                  offsetof(MapHit, greedy_cost) == offsetof(asm_map_hit, greedy_cost),
              "MapHit must have the layout of asm_map_hit");

struct asm_index {
    int device = 0;
    int k = 0;
    int32_t n_seqs = 0;
    uint64_t len = 0;
    std::vector<uint64_t> seq_off;          /* host copy, n_seqs + 1 */
    std::vector<std::string> names;         /* asm_index_build_file: n_seqs names; asm_index_build: none */
    char* d_text = nullptr;                 /* upper case */
    unsigned long long* d_seq_off = nullptr;
    uint32_t* d_off = nullptr;              /* 4^k + 1 bucket offsets */
    uint32_t* d_pos = nullptr;              /* positions sorted by k-mer (ascending inside a bucket) */
    ~asm_index() {
        (void)hipSetDevice(device);
        for (void* p : {(void*)d_text, (void*)d_seq_off, (void*)d_off, (void*)d_pos})
            if (p) (void)hipFree(p);
    }
};

extern "C++" {

static unsigned map_grid(uint64_t n, const asm_handle* h) { /* grid-stride kernels: at most 8 workgroups per CU */
    const uint64_t want = (n + 255) / 256, cap = (uint64_t)h->num_cus * 8;
    return (unsigned)(want < 1 ? 1 : want > cap ? cap : want);
}

/* (launch: asm_capi.hip; fetch, hipcub's scratch MapTmp, map_exclusive_sum and map_sort_pairs: asm_batch.h, which the batch builder shares) */

/* fn(std::integral_constant<int, W>) with W = the 64-bit words a read of maxm bases needs, rounded up to 1, 2, 4 or 8: the one
 * place where a read length picks an instantiation of the <W> kernels */
template <class F>
static hipError_t map_with_width(int maxm, F fn) {
    return with_const_of<1, 2, 4, 8>((maxm + 63) / 64, fn);
}

/* one(first, count) for every chunk of at most step out of n */
template <class F>
static int map_chunks(int64_t n, int64_t step, F one) {
    for (int64_t c0 = 0; c0 < n; c0 += step)
        if (const int rc = one(c0, std::min(n, c0 + step) - c0)) return rc;
    return ASM_OK;
}

/* the caller's CIGAR arrays: cap operations and one count per record; cap = 0: none wanted */
struct MapCigars {
    uint16_t* ops;
    int cap;
    uint8_t* nops;
    MapCigars at(size_t rec) const { return cap > 0 ? MapCigars{ops + rec * cap, cap, nops + rec} : MapCigars{nullptr, 0, nullptr}; }
};

/* What the argument checks of the four mapping calls look at.  off[1] and pp are NULL for the single-end calls, cap_name for the
 * calls without strata and a cap. */
struct MapArgs {
    int64_t n;
    const asm_map_params* p;
    const uint32_t* off[2];
    const asm_pair_params* pp;
    const char* cap_name; /* "max_hits" / "max_pairs" */
    int strata, strata_max, cap;
    MapCigars cg;
};

/* Every check after the call's own "bad arguments", in the order in which they win.  Nothing is read through h or ix before the
 * last two, so that the checks can be tested without a device. */
static int map_check_args(asm_handle* h, const asm_index* ix, const char* who, const char* noun, const MapArgs& a) {
    auto bad = [&](const std::string& text, int code = ASM_EINVAL) { return fail(h, code, std::string(who) + ": " + text); };
    const asm_map_params* p = a.p;
    if (p->max_errors < 0 || p->max_errors > ASM_MAP_MAX_ERRORS) return bad("max_errors must be in [0, 15]");
    if (a.pp ? p->both_strands != 1 : (p->both_strands != 0 && p->both_strands != 1))
        return bad(a.pp ? "both_strands must be 1" : "both_strands must be 0 or 1");
    if (p->max_occ < 0) return bad("max_occ must be >= 0");
    if (p->greedy_k < 0 || p->greedy_k > ASM_GREEDY_MAX_K) return bad("greedy_k must be in [0, 50]");
    if (a.pp && (a.pp->min_insert < 0 || a.pp->min_insert > a.pp->max_insert || a.pp->max_insert > ASM_MAP_MAX_INSERT))
        return bad("need 0 <= min_insert <= max_insert <= 8192");
    if (a.pp && (a.pp->rescue_errors < -1 || a.pp->rescue_errors > ASM_MAP_MAX_ERRORS))
        return bad("rescue_errors must be -1 (off) or in [0, 15]");
    if (a.cap_name && (a.strata < 0 || a.strata > a.strata_max)) return bad("strata must be in [0, " + std::to_string(a.strata_max) + "]");
    if (a.cap_name && (a.cap < 1 || a.cap > ASM_MAP_MAX_HITS)) return bad(std::string(a.cap_name) + " must be in [1, 256]");
    if (a.cg.cap < 0 || (a.cg.cap > 0 && (!a.cg.ops || !a.cg.nops))) return bad("cigar_cap > 0 needs cigar_ops and cigar_nops");
    for (const uint32_t* ro : a.off)
        for (int64_t i = 0; ro && i < a.n; i++) {
            if (ro[i + 1] < ro[i]) return bad("read offsets must be non-decreasing");
            const uint32_t m = ro[i + 1] - ro[i];
            if (m < 1 || m > ASM_MAP_MAX_READ) return bad(std::string("every ") + noun + " must have 1 to 511 bytes");
        }
    if (a.pp && a.n > 0 && (uint64_t)(a.off[0][a.n] - a.off[0][0]) + (a.off[1][a.n] - a.off[1][0]) >= 0xffffffffull)
        return bad("both mates' bytes must stay below 2^32", ASM_EUNSUPPORTED);
    if (!h) return bad("NULL handle");
    if (ix->device != h->device) return bad("the index lives on another device");
    return ASM_OK;
}

/* Greedy on the windows of the mapped items of one chunk (d_list: their indices into d_hits; d_iread: each item's read, NULL when
 * item i is read i); costs into d_cost[q] */
static int map_greedy(asm_handle* h, const asm_index* ix, const char* d_reads, const uint32_t* d_roff, const MapHit* d_hits,
                      const uint32_t* d_iread, const uint32_t* d_list, int64_t nl, int maxm, int greedy_k, int32_t* d_cost) {
    BatchPtr b;
    int rc = batch_new(h, nl, ASM_GREEDY_CLEAN, "asm_map_reads", b);
    if (rc) return rc;
    BatchBuild bb(h, b.get(), ASM_EUNSUPPORTED, "asm_map_reads: a read is longer than ASM_MAX_LENGTH - 1"); /* map_check_args: <= 511 */
    rc = bb.bound(maxm + 1); /* the window is at most one base longer than the read */
    if (rc) return rc;
    Scratch<uint32_t> qlen(h), wlen(h);
    HIPCHK(h, qlen.alloc(sizeof(uint32_t) * ((size_t)nl + 1)));
    HIPCHK(h, wlen.alloc(sizeof(uint32_t) * ((size_t)nl + 1)));
    HIPCHK(h, launch(h, map_greedy_lengths_kernel, grid_for(nl + 1), ASM_BLOCK, d_list, d_iread, (long)nl, d_roff, d_hits,
                     (const unsigned long long*)ix->d_seq_off, qlen.p, wlen.p));
    rc = bb.offsets_from_lengths(BATCH_READS, qlen.p);
    if (!rc) rc = bb.offsets_from_lengths(BATCH_REFS, wlen.p);
    if (!rc) rc = bb.totals();
    if (!rc) rc = bb.text_blocks();
    if (rc) return rc;
    HIPCHK(h, launch(h, map_greedy_gather_kernel, map_grid((uint64_t)nl * 64, h), 256, d_list, d_iread, (long)nl, d_reads, d_roff, d_hits,
                     (const char*)ix->d_text, (const unsigned long long*)ix->d_seq_off, (const uint32_t*)b->d_read_off,
                     (const uint32_t*)b->d_ref_off, b->d_reads, b->d_refs));
    rc = batch_finish(h, b.get());
    if (rc) return rc;
    asm_params gp;
    asm_default_params(&gp);
    gp.k = greedy_k, gp.x = gp.o = gp.e = 1, gp.alignment_type = ASM_ALIGN_GLOBAL;
    return asm_align_batch_async(h, b.get(), ASM_GREEDY, &gp, d_cost);
}

/* The front of a chunk, shared by all mapping calls: reads in HBM (uploaded, or gathered there by asm_map_file) and upper-cased, per-read flags cleared, every work item's
 * candidates counted (map_seed_count_kernel) and numbered (exclusive scan); total = all candidates of the chunk. */
struct MapFront {
    std::vector<uint32_t> roff;
    int maxm = 0;
    size_t bytes = 0;
    int64_t nw = 0;
    unsigned long long total = 0;
    MapSeedArgs sa = {};
    Scratch<char> d_reads;
    Scratch<uint32_t> d_roff, d_flags;
    Scratch<unsigned long long> d_cnt, d_base;
    explicit MapFront(asm_handle* h) : d_reads(h), d_roff(h), d_flags(h), d_cnt(h), d_base(h) {}
    int len(size_t i) const { return (int)(roff[i + 1] - roff[i]); }
};

/* the chunk's reads: one or more runs of reads (asm_map_pairs: the mates 1, then the mates 2), numbered in that order */
struct MapReadsIn {
    const char* reads;
    const uint32_t* read_off; /* n + 1 */
    int64_t n;
};

/* The front once the reads are in HBM: f.d_reads (f.bytes bytes, any case), f.d_roff and its host copy f.roff are filled */
static int map_front_seed(asm_handle* h, const asm_index* ix, int64_t n, const asm_map_params* p, MapFront& f) {
    const int S = p->both_strands ? 2 : 1, P = p->max_errors + 1;
    f.maxm = 0;
    for (int64_t i = 0; i < n; i++) f.maxm = std::max(f.maxm, f.len((size_t)i));
    const size_t bytes = f.bytes;
    const int64_t nw = f.nw = n * S * P;
    HIPCHK(h, f.d_flags.alloc(sizeof(uint32_t) * (size_t)n));
    HIPCHK(h, f.d_cnt.alloc(sizeof(unsigned long long) * (size_t)nw));
    HIPCHK(h, f.d_base.alloc(sizeof(unsigned long long) * (size_t)nw));
    HIPCHK(h, hipMemsetAsync(f.d_flags.p, 0, sizeof(uint32_t) * (size_t)n, h->stream));
    HIPCHK(h, launch(h, map_upper_kernel, map_grid(bytes, h), 256, f.d_reads.p, (unsigned long long)bytes));
    MapSeedArgs& sa = f.sa;
    sa.reads = f.d_reads.p, sa.roff = f.d_roff.p, sa.n = (long)n, sa.S = S, sa.P = P, sa.k = ix->k, sa.e = p->max_errors;
    sa.max_occ = p->max_occ, sa.text = ix->d_text, sa.ix_off = ix->d_off, sa.ix_pos = ix->d_pos;
    sa.seq_off = (const unsigned long long*)ix->d_seq_off, sa.n_seqs = (uint32_t)ix->n_seqs;
    HIPCHK(h, launch(h, map_seed_count_kernel, map_grid((uint64_t)nw, h), 256, sa, f.d_cnt.p, f.d_flags.p));
    MapTmp tmp(h);
    HIPCHK(h, map_exclusive_sum(h, tmp, f.d_cnt.p, f.d_base.p, nw));
    unsigned long long last[2] = {0, 0};
    HIPCHK(h, fetch(h, {fetched(&last[0], f.d_base.p + nw - 1), fetched(&last[1], f.d_cnt.p + nw - 1)}));
    f.total = last[0] + last[1];
    return ASM_OK;
}

/* The runs of reads numbered and uploaded: f.d_reads, f.d_roff, f.roff and f.bytes */
static int map_front_upload(asm_handle* h, const MapReadsIn* in, int n_in, MapFront& f) {
    int64_t n = 0;
    for (int t = 0; t < n_in; t++) n += in[t].n;
    f.roff.assign(1, 0u);
    f.roff.reserve((size_t)n + 1);
    for (int t = 0; t < n_in; t++) {
        const uint32_t o = f.roff.back(), *ro = in[t].read_off;
        for (int64_t i = 1; i <= in[t].n; i++) f.roff.push_back(o + (ro[i] - ro[0]));
    }
    const size_t bytes = f.bytes = f.roff[(size_t)n];
    HIPCHK(h, f.d_reads.alloc(bytes + 16));
    HIPCHK(h, f.d_roff.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    for (int64_t t = 0, o = 0; t < n_in; o += in[t].read_off[in[t].n] - in[t].read_off[0], t++)
        HIPCHK(h, hipMemcpyAsync(f.d_reads.p + o, in[t].reads + in[t].read_off[0], in[t].read_off[in[t].n] - in[t].read_off[0],
                                 hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(f.d_roff.p, f.roff.data(), sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, h->stream));
    return ASM_OK;
}

/* The front from host arrays: the upload, then map_front_seed */
static int map_front(asm_handle* h, const asm_index* ix, const MapReadsIn* in, int n_in, const asm_map_params* p, MapFront& f) {
    if (const int rc = map_front_upload(h, in, n_in, f)) return rc;
    return map_front_seed(h, ix, (int64_t)f.roff.size() - 1, p, f);
}

/* The seeding rounds of a chunk, of at most map_cand_cap candidates each: every round sees every work item, emits the part of it
 * that falls in [c0, c1) and hands those candidates to verify(cand, count) */
template <class V>
static int map_seed_rounds(asm_handle* h, const MapFront& f, V verify) {
    Scratch<MapCand> d_cand(h);
    const unsigned long long cap = std::min<unsigned long long>(f.total, (unsigned long long)h->map_cand_cap);
    if (f.total) HIPCHK(h, d_cand.alloc(sizeof(MapCand) * cap));
    for (unsigned long long c0 = 0; c0 < f.total; c0 += cap) {
        const unsigned long long c1 = std::min(f.total, c0 + cap);
        HIPCHK(h, launch(h, map_seed_emit_kernel, map_grid((uint64_t)f.nw, h), 256, f.sa, (const unsigned long long*)f.d_base.p,
                         (const unsigned long long*)f.d_cnt.p, c0, c1, d_cand.p));
        if (const int rc = verify((const MapCand*)d_cand.p, c1 - c0)) return rc;
    }
    return ASM_OK;
}

/* asm_map_reads: the best end of every read into keys (64-bit atomicMin per candidate) */
static hipError_t map_launch_verify(asm_handle* h, const asm_index* ix, const MapFront& f, int e, const MapCand* cand,
                                    unsigned long long nc, unsigned long long* keys) {
    return map_with_width(f.maxm, [&](auto w) {
        return launch(h, map_verify_kernel<decltype(w)::value>, map_grid(nc, h), 256, cand, nc, (const char*)f.d_reads.p,
                      (const uint32_t*)f.d_roff.p, (const char*)ix->d_text, (const unsigned long long*)ix->d_seq_off, e, keys);
    });
}

/* the other calls: every candidate's run records appended to key / val [0, cap); *counter counts all of them, kept or not */
static hipError_t map_launch_verify_all(asm_handle* h, const asm_index* ix, const MapFront& f, int e, const MapCand* cand,
                                        unsigned long long nc, unsigned long long* counter, unsigned long long cap,
                                        unsigned long long* key, uint32_t* val) {
    return map_with_width(f.maxm, [&](auto w) {
        return launch(h, map_verify_all_kernel<decltype(w)::value>, map_grid(nc, h), 256, cand, nc, (const char*)f.d_reads.p,
                      (const uint32_t*)f.d_roff.p, (const char*)ix->d_text, e, counter, cap, key, val);
    });
}

/* The finish stage, used by all four calls.  Launch: one item per packed key (iread / idirs: each item's read and dirs offset;
 * NULL for the identity list, item i = read i) gets its start, traceback, CIGAR and hit record on the device.  Collect: the records
 * to the host, Greedy on the mapped items, greedy_cost into the host records.  Work may be enqueued between the two halves. */
struct MapFinish {
    int64_t n = 0;
    int ocap = 0;
    const uint32_t* d_iread = nullptr;
    Scratch<uint64_t> d_dirs;
    Scratch<MapHit> d_hits;
    Scratch<uint16_t> d_ops;
    Scratch<uint8_t> d_nops;
    Scratch<char> d_md;        /* ASM_SAM_TAG_MD, the file calls: the items' MD rows and their lengths (map_finish_device), else NULL */
    Scratch<uint8_t> d_md_len;
    explicit MapFinish(asm_handle* h) : d_dirs(h), d_hits(h), d_ops(h), d_nops(h), d_md(h), d_md_len(h) {}
};

static int map_finish_launch(asm_handle* h, const asm_index* ix, const asm_map_params* p, const MapFront& f, int64_t n,
                             const unsigned long long* keys, const uint32_t* iread, const unsigned long long* idirs,
                             unsigned long long dir_words, int cigar_cap, MapFinish& s) {
    s.n = n, s.ocap = cigar_cap > 0 ? cigar_cap : 0, s.d_iread = iread;
    HIPCHK(h, s.d_dirs.alloc(sizeof(uint64_t) * dir_words));
    HIPCHK(h, s.d_hits.alloc(sizeof(MapHit) * (size_t)n));
    HIPCHK(h, s.d_ops.alloc(sizeof(uint16_t) * ((size_t)n * s.ocap + 1)));
    HIPCHK(h, s.d_nops.alloc((size_t)n));
    MapFinishArgs fa = {};
    fa.reads = f.d_reads.p, fa.roff = f.d_roff.p, fa.n = (long)n, fa.e = p->max_errors, fa.P = p->max_errors + 1, fa.k = ix->k;
    fa.cap = s.ocap, fa.text = ix->d_text, fa.seq_off = (const unsigned long long*)ix->d_seq_off, fa.keys = keys;
    fa.flags = f.d_flags.p, fa.iread = iread, fa.idirs = idirs, fa.dirs = s.d_dirs.p, fa.hits = s.d_hits.p, fa.ops = s.d_ops.p;
    fa.nops = s.d_nops.p;
    const hipError_t launched = map_with_width(f.maxm, [&](auto w) {
        constexpr int W = decltype(w)::value;
        return launch(h, iread ? map_finish_kernel<W, true> : map_finish_kernel<W, false>, map_grid((uint64_t)n, h), 256, fa);
    });
    HIPCHK(h, launched);
    return ASM_OK;
}

/* hits[n], ops[n][ocap], nops[n]: host memory, the caller's own arrays or a MapItems.  all_mapped_maxm >= 0: the caller knows that
 * every item is mapped and no read of theirs is longer than that, which saves the pass over the flags and the wait before it. */
static int map_finish_collect(asm_handle* h, const asm_index* ix, const asm_map_params* p, const MapFront& f, MapFinish& s,
                              asm_map_hit* hits, uint16_t* ops, uint8_t* nops, int all_mapped_maxm = -1) {
    const size_t n = (size_t)s.n;
    HIPCHK(h, hipMemcpyAsync(hits, s.d_hits.p, sizeof(MapHit) * n, hipMemcpyDeviceToHost, h->stream));
    if (s.ocap) {
        HIPCHK(h, hipMemcpyAsync(ops, s.d_ops.p, sizeof(uint16_t) * n * s.ocap, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(nops, s.d_nops.p, n, hipMemcpyDeviceToHost, h->stream));
    }
    std::vector<uint32_t> list, iread;
    int maxmap = all_mapped_maxm;
    if (all_mapped_maxm >= 0) {
        list.resize(n);
        for (size_t q = 0; q < n; q++) list[q] = (uint32_t)q;
    } else {
        if (s.d_iread) {
            iread.resize(n);
            HIPCHK(h, hipMemcpyAsync(iread.data(), s.d_iread, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        maxmap = 0;
        for (size_t q = 0; q < n; q++)
            if (hits[q].flags & ASM_MAP_MAPPED) {
                list.push_back((uint32_t)q);
                maxmap = std::max(maxmap, f.len(s.d_iread ? iread[q] : q));
            }
    }
    if (list.empty()) return ASM_OK;
    const size_t nl = list.size();
    Scratch<uint32_t> d_list(h);
    Scratch<int32_t> d_cost(h);
    HIPCHK(h, d_list.alloc(sizeof(uint32_t) * nl));
    HIPCHK(h, d_cost.alloc(sizeof(int32_t) * nl));
    HIPCHK(h, hipMemcpyAsync(d_list.p, list.data(), sizeof(uint32_t) * nl, hipMemcpyHostToDevice, h->stream));
    if (const int rc = map_greedy(h, ix, f.d_reads.p, f.d_roff.p, s.d_hits.p, s.d_iread, d_list.p, (int64_t)nl, maxmap, p->greedy_k, d_cost.p))
        return rc;
    std::vector<int32_t> cost(nl);
    HIPCHK(h, hipMemcpyAsync(cost.data(), d_cost.p, sizeof(int32_t) * nl, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t q = 0; q < nl; q++) hits[list[q]].greedy_cost = cost[q];
    return ASM_OK;
}

/* The collect half for a caller that formats on the device (asm_map_file): the records, ops and nops stay in s; the mapped items
 * are listed on the device, Greedy runs on them and a small kernel puts its costs into the device records.  Every read of the chunk
 * bounds the mapped ones' length. */
static int map_finish_device(asm_handle* h, const asm_index* ix, const asm_map_params* p, const MapFront& f, MapFinish& s) {
    const size_t n = (size_t)s.n;
    if ((h->sam_tags & ASM_SAM_TAG_MD) && n) { /* the items' MD rows: they need the records' pos, end and strand, not their costs */
        HIPCHK(h, s.d_md.alloc(n * MD_ROW_CAP));
        HIPCHK(h, s.d_md_len.alloc(n));
        MapMdArgs ma = {};
        ma.reads = f.d_reads.p, ma.roff = f.d_roff.p, ma.n = (long)n, ma.iread = s.d_iread, ma.hits = s.d_hits.p, ma.ops = s.d_ops.p;
        ma.nops = s.d_nops.p, ma.cap = s.ocap, ma.text = ix->d_text, ma.seq_off = (const unsigned long long*)ix->d_seq_off;
        ma.md = s.d_md.p, ma.md_len = s.d_md_len.p;
        HIPCHK(h, launch(h, map_md_kernel, grid_for((int64_t)n), ASM_BLOCK, ma));
    }
    Scratch<uint32_t> d_flag(h), d_slot(h), d_list(h);
    Scratch<int32_t> d_cost(h);
    MapTmp tmp(h);
    HIPCHK(h, d_flag.alloc(sizeof(uint32_t) * (n + 1)));
    HIPCHK(h, d_slot.alloc(sizeof(uint32_t) * (n + 1)));
    HIPCHK(h, launch(h, map_mapped_flag_kernel, grid_for((int64_t)n + 1), ASM_BLOCK, (const MapHit*)s.d_hits.p, (long)n, d_flag.p));
    HIPCHK(h, map_exclusive_sum(h, tmp, d_flag.p, d_slot.p, (int64_t)n + 1));
    uint32_t nl = 0;
    HIPCHK(h, fetch(h, {fetched(&nl, d_slot.p + n)}));
    if (!nl) return ASM_OK;
    HIPCHK(h, d_list.alloc(sizeof(uint32_t) * nl));
    HIPCHK(h, d_cost.alloc(sizeof(int32_t) * nl));
    HIPCHK(h, launch(h, map_mapped_list_kernel, grid_for((int64_t)n), ASM_BLOCK, (const uint32_t*)d_flag.p, (const uint32_t*)d_slot.p,
                     (long)n, d_list.p));
    if (const int rc = map_greedy(h, ix, f.d_reads.p, f.d_roff.p, s.d_hits.p, s.d_iread, d_list.p, (int64_t)nl, f.maxm, p->greedy_k, d_cost.p))
        return rc;
    HIPCHK(h, launch(h, map_cost_kernel, grid_for((int64_t)nl), ASM_BLOCK, (const uint32_t*)d_list.p, (const int32_t*)d_cost.p, (long)nl,
                     s.d_hits.p));
    return ASM_OK;
}

/* the host copy of finished items, for the calls that scatter them into the caller's slots */
struct MapItems {
    std::vector<asm_map_hit> hits;
    std::vector<uint16_t> ops;
    std::vector<uint8_t> nops;
    int ocap;
    MapItems(int64_t n, int ocap_) : hits((size_t)n), ops((size_t)n * ocap_), nops((size_t)n), ocap(ocap_) {}
    void cigar_to(const MapCigars& cg, size_t rec, size_t item) const { /* item's CIGAR row into the caller's record rec */
        if (!ocap) return;
        std::copy(ops.begin() + item * ocap, ops.begin() + (item + 1) * ocap, cg.ops + rec * ocap);
        cg.nops[rec] = nops[item];
    }
};

static const asm_map_hit MAP_UNUSED_SLOT = MAP_HIT_UNMAPPED;

/* asm_map_reads' keys of a fronted chunk: the seeding rounds with map_verify_kernel<W>, every read's best end in d_keys */
static int map_best_keys(asm_handle* h, const asm_index* ix, int64_t n, const asm_map_params* p, const MapFront& f,
                         Scratch<unsigned long long>& d_keys) {
    HIPCHK(h, d_keys.alloc(sizeof(unsigned long long) * (size_t)n));
    HIPCHK(h, hipMemsetAsync(d_keys.p, 0xff, sizeof(unsigned long long) * (size_t)n, h->stream));
    return map_seed_rounds(h, f, [&](const MapCand* cand, unsigned long long nc) -> int {
        HIPCHK(h, map_launch_verify(h, ix, f, p->max_errors, cand, nc, d_keys.p));
        return ASM_OK;
    });
}

/* The run records of one chunk (every call but asm_map_reads), sorted by (read, s, lo): the seeding rounds with
 * map_verify_all_kernel<W>, then a radix sort.  n < 2^31 reads, so that read << 33 fits the 64-bit run key. */
struct MapRuns {
    unsigned long long nr = 0;
    Scratch<unsigned long long> key;
    Scratch<uint32_t> val;
    explicit MapRuns(asm_handle* h) : key(h), val(h) {}
};

static int map_runs(asm_handle* h, const asm_index* ix, int64_t n, const asm_map_params* p, MapFront& f, MapRuns& out,
                    const char* who) {
    Scratch<unsigned long long> d_counter(h), d_rkey(h);
    Scratch<uint32_t> d_rval(h);
    unsigned long long rcap = 0, nr = 0;
    HIPCHK(h, d_counter.alloc(sizeof(unsigned long long)));
    HIPCHK(h, hipMemsetAsync(d_counter.p, 0, sizeof(unsigned long long), h->stream));
    auto grow = [&](unsigned long long ncap) -> int { /* the run buffer to ncap records, keeping [0, nr) */
        Scratch<unsigned long long> k2(h);
        Scratch<uint32_t> v2(h);
        HIPCHK(h, k2.alloc(sizeof(unsigned long long) * ncap));
        HIPCHK(h, v2.alloc(sizeof(uint32_t) * ncap));
        if (nr) {
            HIPCHK(h, hipMemcpyAsync(k2.p, d_rkey.p, sizeof(unsigned long long) * nr, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(v2.p, d_rval.p, sizeof(uint32_t) * nr, hipMemcpyDeviceToDevice, h->stream));
        }
        std::swap(d_rkey.p, k2.p);
        std::swap(d_rval.p, v2.p);
        rcap = ncap;
        return ASM_OK;
    };
    /* Before each round's verify, the buffer gets room for min(ASM_MAP_RUN_CAP, the round's candidates) more records (a window
     * mostly gives one interval or none); after it, the run counter tells whether the buffer held the round's records.  If not,
     * the buffer grows (keeping the earlier rounds' records), the counter goes back and the verify runs again. */
    const int rc = map_seed_rounds(h, f, [&](const MapCand* cand, unsigned long long nc) -> int {
        const unsigned long long want = nr + std::min(nc, (unsigned long long)h->map_run_cap);
        if (want > rcap)
            if (const int rg = grow(std::max(want, rcap + rcap / 2))) return rg;
        for (;;) {
            HIPCHK(h, map_launch_verify_all(h, ix, f, p->max_errors, cand, nc, d_counter.p, rcap, d_rkey.p, d_rval.p));
            unsigned long long got = 0;
            HIPCHK(h, fetch(h, {fetched(&got, d_counter.p)}));
            if (got <= rcap) {
                nr = got;
                return ASM_OK;
            }
            if (const int rg = grow(std::max(got, 2 * rcap))) return rg;
            HIPCHK(h, hipMemcpyAsync(d_counter.p, &nr, sizeof(nr), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream)); /* nr is read by the copy above before it may change */
        }
    });
    if (rc) return rc;
    if (nr > (unsigned long long)INT32_MAX)
        return fail(h, ASM_EUNSUPPORTED, std::string(who) + ": more than 2^31 - 1 run records in a chunk");
    /* sort by (read, s, lo): only the bits in use (read < n) */
    int rbits = 0;
    while (rbits < 31 && (1ull << rbits) < (unsigned long long)n) rbits++;
    HIPCHK(h, out.key.alloc(sizeof(unsigned long long) * (nr + 1)));
    HIPCHK(h, out.val.alloc(sizeof(uint32_t) * (nr + 1)));
    MapTmp tmp(h);
    if (nr) HIPCHK(h, map_sort_pairs(h, tmp, d_rkey.p, out.key.p, d_rval.p, out.val.p, (int)nr, MAP_RUN_READ_SHIFT + rbits));
    out.nr = nr;
    return ASM_OK;
}

/* what map_select_count_kernel / map_select_emit_kernel / map_loci_emit_kernel read of a chunk's sorted runs */
static MapSelectArgs map_select_args(const asm_index* ix, const MapFront& f, const MapRuns& runs, int64_t n, int e, int strata,
                                     int max_hits, uint32_t* n_hits, uint32_t* d_best) {
    MapSelectArgs sel = {};
    sel.rkey = runs.key.p, sel.rval = runs.val.p, sel.nr = runs.nr, sel.n = (long)n, sel.e = e, sel.strata = strata, sel.max_hits = max_hits;
    sel.seq_off = (const unsigned long long*)ix->d_seq_off, sel.n_seqs = (uint32_t)ix->n_seqs, sel.roff = f.d_roff.p;
    sel.n_hits = n_hits, sel.d_best = d_best;
    return sel;
}

/* Mapping quality under ASM_MAPQ_GAP (the model: docs/design/mapper.md, "Mapping quality"; the rules: asm_map_core.h).  Per read
 * Q_read and d1, and per item of a call its MAPQ byte, next to the device records. */
struct MapMapq {
    Scratch<uint8_t> rq, rd1, item, pq, ps1, sec;
    const uint8_t* d_item = nullptr; /* per item of the finish stage: item.p, or rq.p where item i is read i with its best hit */
    explicit MapMapq(asm_handle* h) : rq(h), rd1(h), item(h), pq(h), ps1(h), sec(h) {}
};

/* map_mapq_kernel over a chunk's sorted runs: rq and rd1; best: every read's best key (NULL: not wanted); ibase / ikey / ni: the
 * items of asm_map_reads_all, whose bytes go to m.item (ibase NULL: none) */
static int map_mapq_reads(asm_handle* h, const asm_index* ix, const MapFront& f, const MapRuns& runs, int64_t n, int e, MapMapq& m,
                          unsigned long long* best, const uint32_t* ibase, const unsigned long long* ikey, int64_t ni) {
    HIPCHK(h, m.rq.alloc((size_t)n + 1));
    HIPCHK(h, m.rd1.alloc((size_t)n + 1));
    if (ibase) HIPCHK(h, m.item.alloc((size_t)ni + 1));
    MapMapqArgs a = {};
    a.rkey = runs.key.p, a.rval = runs.val.p, a.nr = runs.nr, a.n = (long)n, a.e = e;
    a.seq_off = (const unsigned long long*)ix->d_seq_off, a.n_seqs = (uint32_t)ix->n_seqs, a.flags = f.d_flags.p;
    a.rq = m.rq.p, a.rd1 = m.rd1.p, a.best = best, a.ibase = ibase, a.ikey = ikey, a.mapq = m.item.p;
    HIPCHK(h, launch(h, map_mapq_kernel, map_grid((uint64_t)n, h), 256, a));
    m.d_item = ibase ? m.item.p : m.rq.p;
    return ASM_OK;
}

/* the reference model's value of host records: what every in-memory call leaves for asm_map_last_mapq under ASM_MAPQ_REFERENCE */
static void map_mapq_from_records(const asm_map_hit* out, size_t count, uint8_t* mq) {
    for (size_t t = 0; t < count; t++) mq[t] = (uint8_t)map_mapq_reference((out[t].flags & ASM_MAP_MAPPED) != 0, out[t].greedy_cost);
}

/* An in-memory mapping call's body with the handle's MAPQ slots around it: `count` record slots, valid once the call succeeded */
template <class F>
static int map_mapq_call(asm_handle* h, size_t count, F body) {
    h->last_mapq_valid = false;
    h->last_mapq.assign(count, 0);
    const int rc = body();
    h->last_mapq_valid = rc == ASM_OK;
    return rc;
}

/* asm_map_reads' keys under ASM_MAPQ_GAP, where the fold needs every locus: the sorted runs of the other calls instead of the
 * atomicMin, then map_mapq_kernel, which leaves every read's best key (rank 0 of asm_map_reads_all: the same hit) and its MAPQ */
static int map_best_keys_gap(asm_handle* h, const asm_index* ix, int64_t n, const asm_map_params* p, MapFront& f, const char* who,
                             MapRuns& runs, MapMapq& mm, Scratch<unsigned long long>& d_keys) {
    HIPCHK(h, d_keys.alloc(sizeof(unsigned long long) * (size_t)n));
    if (const int rc = map_runs(h, ix, n, p, f, runs, who)) return rc;
    return map_mapq_reads(h, ix, f, runs, n, p->max_errors, mm, d_keys.p, nullptr, nullptr, 0);
}

/* asm_map_reads on one chunk: everything on the device, results straight into the caller's host arrays */
static int map_chunk(asm_handle* h, const asm_index* ix, int64_t n, const char* reads, const uint32_t* read_off,
                     const asm_map_params* p, asm_map_hit* out, MapCigars cg, uint8_t* mq) {
    MapFront f(h);
    Scratch<unsigned long long> d_keys(h);
    const MapReadsIn in = {reads, read_off, n};
    if (const int rc = map_front(h, ix, &in, 1, p, f)) return rc;
    MapRuns runs(h);
    MapMapq mm(h);
    if (h->mapq_model == ASM_MAPQ_GAP) {
        if (const int rc = map_best_keys_gap(h, ix, n, p, f, "asm_map_reads", runs, mm, d_keys)) return rc;
    } else if (const int rc = map_best_keys(h, ix, n, p, f, d_keys)) {
        return rc;
    }
    MapFinish fin(h);
    if (const int rc2 = map_finish_launch(h, ix, p, f, n, d_keys.p, nullptr, nullptr, f.bytes + (size_t)n, cg.cap, fin)) return rc2;
    if (mm.d_item) HIPCHK(h, hipMemcpyAsync(mq, mm.d_item, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (const int rc = map_finish_collect(h, ix, p, f, fin, out, cg.ops, cg.nops)) return rc;
    if (!mm.d_item) map_mapq_from_records(out, (size_t)n, mq);
    return ASM_OK;
}

/* asm_map_reads_all's items of a fronted chunk: the sorted run records, the loci selected per read (n_hits: host, n entries) and
 * listed as items in read-then-rank order, max(1, min(n_hits, max_hits)) per read */
struct MapAllItems {
    MapRuns runs;
    Scratch<uint32_t> d_nh, d_dbest, d_ibase, d_iread;
    Scratch<unsigned long long> d_dbase, d_ikey, d_idirs;
    std::vector<uint32_t> ibase;           /* n + 1 */
    std::vector<unsigned long long> dbase; /* the upload's source: lives as long as the items */
    unsigned long long dwords = 0;
    int64_t ni = 0;
    explicit MapAllItems(asm_handle* h) : runs(h), d_nh(h), d_dbest(h), d_ibase(h), d_iread(h), d_dbase(h), d_ikey(h), d_idirs(h) {}
};

static int map_all_items(asm_handle* h, const asm_index* ix, int64_t n, const asm_map_params* p, int strata, int max_hits, MapFront& f,
                         uint32_t* n_hits, MapAllItems& it, const char* who) {
    if (const int rc = map_runs(h, ix, n, p, f, it.runs, who)) return rc;
    /* loci per read: count, then (host) the item layout, then emit */
    HIPCHK(h, it.d_nh.alloc(sizeof(uint32_t) * (size_t)n));
    HIPCHK(h, it.d_dbest.alloc(sizeof(uint32_t) * (size_t)n));
    MapSelectArgs sel = map_select_args(ix, f, it.runs, n, p->max_errors, strata, max_hits, it.d_nh.p, it.d_dbest.p);
    HIPCHK(h, launch(h, map_select_count_kernel, map_grid((uint64_t)n, h), 256, sel));
    HIPCHK(h, fetch(h, {fetched(n_hits, it.d_nh.p, (size_t)n)}));
    /* items: max(1, min(n_hits, max_hits)) per read, in read-then-rank order; dirs: (m + 1) words per item */
    std::vector<uint32_t>& ibase = it.ibase;
    ibase.assign((size_t)n + 1, 0u);
    std::vector<unsigned long long>& dbase = it.dbase;
    dbase.assign((size_t)n, 0ull);
    unsigned long long dwords = 0;
    for (int64_t i = 0; i < n; i++) {
        const uint32_t ni = n_hits[i] ? std::min<uint32_t>(n_hits[i], (uint32_t)max_hits) : 1u;
        ibase[(size_t)i + 1] = ibase[(size_t)i] + ni;
        dbase[(size_t)i] = dwords;
        dwords += (unsigned long long)ni * (f.len((size_t)i) + 1u);
    }
    const int64_t ni = it.ni = ibase[(size_t)n];
    it.dwords = dwords;
    HIPCHK(h, it.d_ibase.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    HIPCHK(h, it.d_dbase.alloc(sizeof(unsigned long long) * (size_t)n));
    HIPCHK(h, it.d_iread.alloc(sizeof(uint32_t) * (size_t)ni));
    HIPCHK(h, it.d_ikey.alloc(sizeof(unsigned long long) * (size_t)ni));
    HIPCHK(h, it.d_idirs.alloc(sizeof(unsigned long long) * (size_t)ni));
    HIPCHK(h, hipMemcpyAsync(it.d_ibase.p, ibase.data(), sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(it.d_dbase.p, dbase.data(), sizeof(unsigned long long) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    sel.ibase = it.d_ibase.p, sel.dbase = it.d_dbase.p, sel.iread = it.d_iread.p, sel.ikey = it.d_ikey.p, sel.idirs = it.d_idirs.p;
    HIPCHK(h, launch(h, map_select_emit_kernel, map_grid((uint64_t)n, h), 256, sel));
    return ASM_OK;
}

/* asm_map_reads_all on one chunk: the front, the items, the finish stage on them, then the scatter into the caller's
 * [n][max_hits] slots */
static int map_chunk_all(asm_handle* h, const asm_index* ix, int64_t n, const char* reads, const uint32_t* read_off,
                         const asm_map_params* p, int strata, int max_hits, uint32_t* n_hits, asm_map_hit* out, MapCigars cg,
                         uint8_t* mq) {
    MapFront f(h);
    const MapReadsIn in = {reads, read_off, n};
    if (const int rc = map_front(h, ix, &in, 1, p, f)) return rc;
    MapAllItems ai(h);
    if (const int rc = map_all_items(h, ix, n, p, strata, max_hits, f, n_hits, ai, "asm_map_reads_all")) return rc;
    const std::vector<uint32_t>& ibase = ai.ibase;
    const int64_t ni = ai.ni;
    MapFinish fin(h);
    if (const int rc = map_finish_launch(h, ix, p, f, ni, ai.d_ikey.p, ai.d_iread.p, ai.d_idirs.p, ai.dwords, cg.cap, fin)) return rc;
    MapItems it(ni, fin.ocap);
    MapMapq mm(h);
    std::vector<uint8_t> imq; /* ASM_MAPQ_GAP: per item */
    if (h->mapq_model == ASM_MAPQ_GAP) {
        if (const int rc = map_mapq_reads(h, ix, f, ai.runs, n, p->max_errors, mm, nullptr, ai.d_ibase.p, ai.d_ikey.p, ni)) return rc;
        imq.resize((size_t)ni);
        HIPCHK(h, hipMemcpyAsync(imq.data(), mm.d_item, (size_t)ni, hipMemcpyDeviceToHost, h->stream));
    }
    if (const int rc = map_finish_collect(h, ix, p, f, fin, it.hits.data(), it.ops.data(), it.nops.data())) return rc;
    /* into the caller's [n][max_hits] slots (a read's items are contiguous); the flags that depend on the rank are set here.  The
     * CIGAR rows of unused slots are not written: their cigar_nops is 0. */
    const int ocap = fin.ocap;
    for (int64_t i = 0; i < n; i++) {
        const uint32_t q0 = ibase[(size_t)i], cnt = ibase[(size_t)i + 1] - q0;
        const size_t o = (size_t)i * max_hits;
        std::copy(it.hits.begin() + q0, it.hits.begin() + q0 + cnt, out + o);
        for (uint32_t t = 1; t < cnt; t++) out[o + t].flags |= ASM_MAP_SECONDARY;
        if (n_hits[i] > (uint32_t)max_hits)
            for (uint32_t t = 0; t < cnt; t++) out[o + t].flags |= ASM_MAP_HITS_TRUNCATED;
        std::fill(out + o + cnt, out + o + max_hits, MAP_UNUSED_SLOT);
        if (ocap) {
            std::copy(it.ops.begin() + (size_t)q0 * ocap, it.ops.begin() + (size_t)(q0 + cnt) * ocap, cg.ops + o * ocap);
            std::copy(it.nops.begin() + q0, it.nops.begin() + q0 + cnt, cg.nops + o);
            std::fill(cg.nops + o + cnt, cg.nops + o + max_hits, (uint8_t)0);
        }
        if (!imq.empty()) std::copy(imq.begin() + q0, imq.begin() + q0 + cnt, mq + o); /* unused slots stay 0 */
    }
    if (imq.empty()) map_mapq_from_records(out, (size_t)n * max_hits, mq);
    return ASM_OK;
}

/* The paired calls' front on one chunk of np pairs (mate 1 of pair p = read p, mate 2 = read np + p): the sorted run records, each
 * read's loci listed (count, scan, emit), the pairing and the rescue of pairs without a concordant pair. */
struct MapPairFront {
    MapFront f;
    MapRuns runs;
    Scratch<uint32_t> d_nh, d_dbest, d_lbase, d_lsplit, d_nconc, d_anchors, d_nanch;
    Scratch<unsigned long long> d_lkey, d_lbest, d_ikey, d_rslot;
    Scratch<uint8_t> d_state, d_mapq; /* d_mapq: ASM_MAPQ_GAP, per read: the MAPQ of its record in the pair's answer */
    MapMapq mm;
    MapPairMapqArgs ma = {};
    MapPairArgs pa = {};
    explicit MapPairFront(asm_handle* h)
        : f(h), runs(h), d_nh(h), d_dbest(h), d_lbase(h), d_lsplit(h), d_nconc(h), d_anchors(h), d_nanch(h), d_lkey(h), d_lbest(h),
          d_ikey(h), d_rslot(h), d_state(h), d_mapq(h), mm(h) {}
};

struct MapPairsIn { /* the two mates of a chunk's pairs */
    const char* reads1;
    const uint32_t* off1;
    const char* reads2;
    const uint32_t* off2;
    MapPairsIn at(int64_t c0) const { return {reads1, off1 + c0, reads2, off2 + c0}; }
};

/* The paired front once the 2 np reads are in HBM (pf.f.d_reads, d_roff, roff and bytes are filled: uploaded by map_pairs_front,
 * or gathered there by asm_map_pairs_file) */
static int map_pairs_front_seed(asm_handle* h, const asm_index* ix, int64_t np, const asm_map_params* p, const asm_pair_params* pp,
                                const char* who, MapPairFront& pf) {
    const int64_t n = 2 * np;
    MapFront& f = pf.f;
    if (const int rc = map_front_seed(h, ix, n, p, f)) return rc;
    const int e = p->max_errors;
    if (const int rc = map_runs(h, ix, n, p, f, pf.runs, who)) return rc;
    /* each read's loci (strata = e: all of them), listed in walk order */
    HIPCHK(h, pf.d_nh.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    HIPCHK(h, pf.d_dbest.alloc(sizeof(uint32_t) * (size_t)n));
    HIPCHK(h, pf.d_lbase.alloc(sizeof(uint32_t) * ((size_t)n + 1)));
    const MapSelectArgs sel = map_select_args(ix, f, pf.runs, n, e, e, 1, pf.d_nh.p, pf.d_dbest.p);
    HIPCHK(h, hipMemsetAsync(pf.d_nh.p + n, 0, sizeof(uint32_t), h->stream));
    HIPCHK(h, launch(h, map_select_count_kernel, map_grid((uint64_t)n, h), 256, sel));
    MapTmp tmp(h);
    HIPCHK(h, map_exclusive_sum(h, tmp, pf.d_nh.p, pf.d_lbase.p, n + 1));
    uint32_t nloci = 0;
    HIPCHK(h, fetch(h, {fetched(&nloci, pf.d_lbase.p + n)}));
    HIPCHK(h, pf.d_lkey.alloc(sizeof(unsigned long long) * ((size_t)nloci + 1)));
    HIPCHK(h, pf.d_lsplit.alloc(sizeof(uint32_t) * (size_t)n));
    HIPCHK(h, pf.d_lbest.alloc(sizeof(unsigned long long) * (size_t)n));
    HIPCHK(h, launch(h, map_loci_emit_kernel, map_grid((uint64_t)n, h), 256, sel, (const uint32_t*)pf.d_lbase.p, pf.d_lkey.p, pf.d_lsplit.p,
                     pf.d_lbest.p));
    /* pairing */
    HIPCHK(h, pf.d_ikey.alloc(sizeof(unsigned long long) * (size_t)n));
    HIPCHK(h, pf.d_nconc.alloc(sizeof(uint32_t) * (size_t)np));
    HIPCHK(h, pf.d_state.alloc((size_t)np));
    HIPCHK(h, pf.d_nanch.alloc(sizeof(uint32_t)));
    HIPCHK(h, hipMemsetAsync(pf.d_nanch.p, 0, sizeof(uint32_t), h->stream));
    const bool rescue = pp->rescue_errors >= 0;
    if (rescue) {
        HIPCHK(h, pf.d_anchors.alloc(sizeof(uint32_t) * (size_t)n));
        HIPCHK(h, pf.d_rslot.alloc(sizeof(unsigned long long) * (size_t)n));
        HIPCHK(h, hipMemsetAsync(pf.d_rslot.p, 0xff, sizeof(unsigned long long) * (size_t)n, h->stream));
    }
    MapPairArgs& pa = pf.pa;
    pa.np = (long)np, pa.roff = f.d_roff.p, pa.lbase = pf.d_lbase.p, pa.lsplit = pf.d_lsplit.p, pa.lbest = pf.d_lbest.p;
    pa.lkey = pf.d_lkey.p, pa.min_insert = pp->min_insert, pa.max_insert = pp->max_insert, pa.rescue = pp->rescue_errors;
    pa.ikey = pf.d_ikey.p, pa.n_conc = pf.d_nconc.p, pa.state = pf.d_state.p, pa.anchors = pf.d_anchors.p, pa.n_anchors = pf.d_nanch.p;
    pa.rslot = pf.d_rslot.p, pa.seq_off = (const unsigned long long*)ix->d_seq_off;
    HIPCHK(h, launch(h, map_pair_kernel, map_grid((uint64_t)np, h), 256, pa));
    if (rescue) {
        /* one thread per (anchor, tile of ends); grid-stride over the anchor count the pair kernel left on the device (<= 2 np) */
        const uint32_t ntile = (uint32_t)((pp->max_insert - pp->min_insert + MAP_RESCUE_TILE) / MAP_RESCUE_TILE);
        const hipError_t launched = map_with_width(f.maxm, [&](auto w) {
            return launch(h, map_rescue_kernel<decltype(w)::value>, map_grid((uint64_t)(2 * pa.np) * ntile, h), 256, pa,
                          (const char*)f.d_reads.p, (const char*)ix->d_text, ntile, pf.d_rslot.p);
        });
        HIPCHK(h, launched);
        HIPCHK(h, launch(h, map_rescue_pick_kernel, map_grid((uint64_t)np, h), 256, pa));
    }
    if (h->mapq_model == ASM_MAPQ_GAP) { /* the states are final: every read folded, then every pair */
        if (const int rc = map_mapq_reads(h, ix, f, pf.runs, n, e, pf.mm, nullptr, nullptr, nullptr, 0)) return rc;
        HIPCHK(h, pf.d_mapq.alloc((size_t)n + 1));
        HIPCHK(h, pf.mm.pq.alloc((size_t)np + 1));
        HIPCHK(h, pf.mm.ps1.alloc((size_t)np + 1));
        MapPairMapqArgs& ma = pf.ma;
        ma.pa = pa, ma.e = e, ma.flags = f.d_flags.p, ma.rq = pf.mm.rq.p, ma.rd1 = pf.mm.rd1.p, ma.mapq = pf.d_mapq.p;
        ma.pq = pf.mm.pq.p, ma.ps1 = pf.mm.ps1.p;
        HIPCHK(h, launch(h, map_pair_mapq_kernel, map_grid((uint64_t)np, h), 256, ma));
    }
    return ASM_OK;
}

/* The paired front from host arrays: the mates 1 and then the mates 2 uploaded, then map_pairs_front_seed */
static int map_pairs_front(asm_handle* h, const asm_index* ix, int64_t np, const MapPairsIn& m, const asm_map_params* p,
                           const asm_pair_params* pp, const char* who, MapPairFront& pf) {
    const MapReadsIn in[2] = {{m.reads1, m.off1, np}, {m.reads2, m.off2, np}};
    if (const int rc = map_front_upload(h, in, 2, pf.f)) return rc;
    return map_pairs_front_seed(h, ix, np, p, pp, who, pf);
}

/* asm_map_pairs' answer after map_pairs_front: the finish stage on the identity list (one item per read), then pair q's two records
 * into out[2 q slots + 0, 1] with the pair flags, tlen[q slots], n_concordant[q] and the CIGAR rows of those records (slots:
 * records per mate and pair in the caller's arrays, 1 for asm_map_pairs) */
static int map_pairs_primary(asm_handle* h, const asm_index* ix, int64_t np, const asm_map_params* p, MapPairFront& pf, int slots,
                             asm_map_hit* out, int32_t* tlen, uint32_t* n_concordant, MapCigars cg, uint8_t* mq) {
    const int64_t n = 2 * np;
    MapFront& f = pf.f;
    MapFinish fin(h);
    std::vector<uint8_t> imq; /* ASM_MAPQ_GAP: per read */
    if (pf.d_mapq.p) {
        imq.resize((size_t)n);
        HIPCHK(h, hipMemcpyAsync(imq.data(), pf.d_mapq.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    }
    if (const int rc = map_finish_launch(h, ix, p, f, n, pf.d_ikey.p, nullptr, nullptr, f.bytes + (size_t)n, cg.cap, fin)) return rc;
    MapItems it(n, fin.ocap);
    std::vector<uint8_t> state((size_t)np);
    HIPCHK(h, hipMemcpyAsync(state.data(), pf.d_state.p, (size_t)np, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(n_concordant, pf.d_nconc.p, sizeof(uint32_t) * (size_t)np, hipMemcpyDeviceToHost, h->stream));
    if (const int rc = map_finish_collect(h, ix, p, f, fin, it.hits.data(), it.ops.data(), it.nops.data())) return rc;
    /* into the caller's records; the pair flags and tlen are set here */
    for (int64_t q = 0; q < np; q++) {
        const size_t r0 = (size_t)(2 * q) * slots; /* pair q's first record */
        asm_map_hit* o = out + r0;
        o[0] = it.hits[(size_t)q], o[1] = it.hits[(size_t)(np + q)];
        const uint8_t st = state[(size_t)q];
        if (st == MAP_PAIR_CONCORDANT || st == MAP_PAIR_RESCUED1 || st == MAP_PAIR_RESCUED2) {
            o[0].flags |= ASM_MAP_PROPER_PAIR, o[1].flags |= ASM_MAP_PROPER_PAIR;
            if (st == MAP_PAIR_RESCUED1) o[0].flags |= ASM_MAP_RESCUED;
            if (st == MAP_PAIR_RESCUED2) o[1].flags |= ASM_MAP_RESCUED;
        }
        const bool same = (o[0].flags & ASM_MAP_MAPPED) && (o[1].flags & ASM_MAP_MAPPED) && o[0].seq_id == o[1].seq_id;
        tlen[(size_t)q * slots] = same ? (int32_t)(std::max(o[0].end, o[1].end) - std::min(o[0].pos, o[1].pos)) : 0;
        it.cigar_to(cg, r0, (size_t)q), it.cigar_to(cg, r0 + 1, (size_t)(np + q));
        if (!imq.empty()) mq[r0] = imq[(size_t)q], mq[r0 + 1] = imq[(size_t)(np + q)];
        else map_mapq_from_records(o, 2, mq + r0);
    }
    return ASM_OK;
}

/* asm_map_pairs on one chunk of np pairs: the front, then the primary answer */
static int map_chunk_pairs(asm_handle* h, const asm_index* ix, int64_t np, const MapPairsIn& m, const asm_map_params* p,
                           const asm_pair_params* pp, asm_map_hit* out, int32_t* tlen, uint32_t* n_concordant, MapCigars cg,
                           uint8_t* mq) {
    MapPairFront pf(h);
    if (const int rc = map_pairs_front(h, ix, np, m, p, pp, "asm_map_pairs", pf)) return rc;
    return map_pairs_primary(h, ix, np, p, pf, 1, out, tlen, n_concordant, cg, mq);
}

/* host threads that fill the slots beyond rank 0 of asm_map_pairs_all's arrays as unused while the device works; joined by
 * join() or at scope exit */
struct MapSlotFill {
    std::vector<std::thread> t;
    MapSlotFill(int64_t np, int max_pairs, asm_map_hit* out, int32_t* tlen, MapCigars cg) {
        const int64_t nt = max_pairs > 1 ? std::min<int64_t>(4, std::max<int64_t>(1, np / 4096)) : 0;
        for (int64_t k = 0; k < nt; k++)
            t.emplace_back([=]() {
                for (int64_t q = np * k / nt; q < np * (k + 1) / nt; q++) {
                    const size_t o = (size_t)q * max_pairs;
                    std::fill(out + 2 * (o + 1), out + 2 * (o + max_pairs), MAP_UNUSED_SLOT);
                    std::fill(tlen + o + 1, tlen + o + max_pairs, 0);
                    if (cg.cap > 0) std::fill(cg.nops + 2 * (o + 1), cg.nops + 2 * (o + max_pairs), (uint8_t)0);
                }
            });
    }
    void join() {
        for (std::thread& x : t) x.join();
        t.clear();
    }
    ~MapSlotFill() { join(); }
};

/* asm_map_pairs_all on one chunk of np pairs: the front, the eligible pairs counted, ranks >= 1 listed as items (mate 1, mate 2 per
 * pair) in pair order and their finish kernel enqueued; then, while the device works on it, the primary answer of asm_map_pairs
 * (rank 0); then the secondary items collected and scattered into the caller's [np][max_pairs][2] slots. */
static int map_chunk_pairs_all(asm_handle* h, const asm_index* ix, int64_t np, const MapPairsIn& m, const asm_map_params* p,
                               const asm_pair_params* pp, int strata, int max_pairs, uint32_t* n_pairs, asm_map_hit* out,
                               int32_t* tlen, uint32_t* n_concordant, MapCigars cg, uint8_t* mq) {
    MapSlotFill fill(np, max_pairs, out, tlen, cg);
    MapPairFront pf(h);
    if (const int rc = map_pairs_front(h, ix, np, m, p, pp, "asm_map_pairs_all", pf)) return rc;
    MapFront& f = pf.f;
    /* eligible pairs per pair, and the layout of the secondary items (device scans) */
    Scratch<uint32_t> d_np(h), d_sums(h), d_iread(h);
    Scratch<unsigned long long> d_nitem(h), d_ndirs(h), d_ibase(h), d_dbase(h), d_ikey(h), d_idirs(h);
    HIPCHK(h, d_np.alloc(sizeof(uint32_t) * (size_t)np));
    HIPCHK(h, d_sums.alloc(sizeof(uint32_t) * (size_t)np));
    for (Scratch<unsigned long long>* x : {&d_nitem, &d_ndirs, &d_ibase, &d_dbase})
        HIPCHK(h, x->alloc(sizeof(unsigned long long) * ((size_t)np + 1)));
    HIPCHK(h, hipMemsetAsync(d_nitem.p + np, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(d_ndirs.p + np, 0, sizeof(unsigned long long), h->stream));
    MapPairAllArgs aa = {};
    aa.pa = pf.pa, aa.strata = strata, aa.max_pairs = max_pairs, aa.n_pairs = d_np.p, aa.sums = d_sums.p, aa.nitem = d_nitem.p;
    aa.ndirs = d_ndirs.p, aa.ibase = d_ibase.p, aa.dbase = d_dbase.p;
    HIPCHK(h, launch(h, map_pair_count_kernel, map_grid((uint64_t)np, h), 256, aa));
    MapTmp tmp(h);
    HIPCHK(h, map_exclusive_sum(h, tmp, d_nitem.p, d_ibase.p, np + 1));
    HIPCHK(h, map_exclusive_sum(h, tmp, d_ndirs.p, d_dbase.p, np + 1));
    unsigned long long tot[2] = {0, 0};
    HIPCHK(h, fetch(h, {fetched(n_pairs, d_np.p, (size_t)np), fetched(&tot[0], d_ibase.p + np), fetched(&tot[1], d_dbase.p + np)}));
    const int64_t ni = (int64_t)tot[0];
    /* ranks >= 1: items, finish kernel (the item-list instantiation of asm_map_reads_all) */
    MapFinish fin(h);
    if (ni) {
        HIPCHK(h, d_iread.alloc(sizeof(uint32_t) * (size_t)ni));
        HIPCHK(h, d_ikey.alloc(sizeof(unsigned long long) * (size_t)ni));
        HIPCHK(h, d_idirs.alloc(sizeof(unsigned long long) * (size_t)ni));
        aa.iread = d_iread.p, aa.ikey = d_ikey.p, aa.idirs = d_idirs.p;
        HIPCHK(h, launch(h, map_pair_emit_kernel, map_grid((uint64_t)np, h), 256, aa));
        if (const int rc = map_finish_launch(h, ix, p, f, ni, d_ikey.p, d_iread.p, d_idirs.p, tot[1], cg.cap, fin)) return rc;
    }
    std::vector<uint8_t> imq; /* ASM_MAPQ_GAP: per secondary item */
    if (ni && h->mapq_model == ASM_MAPQ_GAP) {
        HIPCHK(h, pf.mm.sec.alloc((size_t)ni));
        MapPairMapqArgs ma = pf.ma;
        ma.ni = (long)ni, ma.iread = d_iread.p, ma.ikey = d_ikey.p, ma.imapq = pf.mm.sec.p;
        HIPCHK(h, launch(h, map_pair_item_mapq_kernel, map_grid((uint64_t)ni / 2, h), 256, ma));
        imq.resize((size_t)ni);
        HIPCHK(h, hipMemcpyAsync(imq.data(), pf.mm.sec.p, (size_t)ni, hipMemcpyDeviceToHost, h->stream));
    }
    /* rank 0: asm_map_pairs' answer */
    if (const int rc = map_pairs_primary(h, ix, np, p, pf, max_pairs, out, tlen, n_concordant, cg, mq)) return rc;
    for (int64_t q = 0; q < np; q++)
        if (n_pairs[q] > (uint32_t)max_pairs) {
            out[(size_t)q * 2 * max_pairs].flags |= ASM_MAP_HITS_TRUNCATED;
            out[(size_t)q * 2 * max_pairs + 1].flags |= ASM_MAP_HITS_TRUNCATED;
        }
    fill.join();
    if (!ni) return ASM_OK;
    /* every secondary item is mapped: Greedy on all of them, in item order */
    int maxmap = 0;
    for (int64_t q = 0; q < np; q++)
        if (n_pairs[q] >= 2) maxmap = std::max(maxmap, std::max(f.len((size_t)q), f.len((size_t)(np + q))));
    MapItems it(ni, fin.ocap);
    if (const int rc = map_finish_collect(h, ix, p, f, fin, it.hits.data(), it.ops.data(), it.nops.data(), maxmap)) return rc;
    /* into the caller's slots: items 2 (t - 1) and 2 (t - 1) + 1 of a pair are rank t's mates 1 and 2 */
    size_t item = 0;
    for (int64_t q = 0; q < np; q++) {
        const uint32_t want = std::min<uint32_t>(n_pairs[q], (uint32_t)max_pairs);
        const uint8_t extra = ASM_MAP_PROPER_PAIR | ASM_MAP_SECONDARY | (n_pairs[q] > (uint32_t)max_pairs ? ASM_MAP_HITS_TRUNCATED : 0);
        for (uint32_t t = 1; t < want; t++, item += 2) {
            const size_t o = ((size_t)q * max_pairs + t) * 2;
            for (int x = 0; x < 2; x++) {
                out[o + x] = it.hits[item + x];
                out[o + x].flags |= extra;
                it.cigar_to(cg, o + x, item + x);
                mq[o + x] = imq.empty() ? (uint8_t)map_mapq_reference(true, out[o + x].greedy_cost) : imq[item + x];
            }
            tlen[(size_t)q * max_pairs + t] = (int32_t)(std::max(out[o].end, out[o + 1].end) - std::min(out[o].pos, out[o + 1].pos));
        }
    }
    return ASM_OK;
}

/* pairs per chunk: at most map_chunk / 2; the run key holds the read (2 per pair) in its top 31 bits */
static int64_t map_pair_step(const asm_handle* h) { return std::max<int64_t>(1, std::min<int64_t>(h->map_chunk, (int64_t)1 << 30) / 2); }

/* The index stage of asm_index_build and asm_index_build_file: ix holds its text in HBM (d_text, len; any case) and its sequence
 * offsets (d_seq_off, seq_off, n_seqs), the copies into them queued on the handle's stream.  The k-mer keys, the stable sort (positions
 * ascend inside a bucket) and the bucket offsets; d_off and d_pos are allocated here, when the text length is known.  Waits for the
 * stream. */
static int map_index_stage(asm_handle* h, asm_index* ix) {
    const uint64_t len = ix->len;
    const int k = ix->k;
    const uint32_t nb = (1u << (2 * k)) + 1u;
    HIPCHK(h, big_malloc(h, (void**)&ix->d_off, sizeof(uint32_t) * nb));
    HIPCHK(h, big_malloc(h, (void**)&ix->d_pos, sizeof(uint32_t) * (len ? len : 1)));
    if (len) {
        Scratch<uint32_t> keys(h), keys2(h), vals(h);
        MapTmp tmp(h);
        HIPCHK(h, keys.alloc(sizeof(uint32_t) * len));
        HIPCHK(h, keys2.alloc(sizeof(uint32_t) * len));
        HIPCHK(h, vals.alloc(sizeof(uint32_t) * len));
        HIPCHK(h, launch(h, map_upper_kernel, map_grid(len, h), 256, ix->d_text, (unsigned long long)len));
        HIPCHK(h, launch(h, map_kmer_key_kernel, map_grid(len, h), 256, (const char*)ix->d_text, (unsigned long long)len,
                         (const unsigned long long*)ix->d_seq_off, (uint32_t)ix->n_seqs, k, keys.p, vals.p));
        HIPCHK(h, map_sort_pairs(h, tmp, keys.p, keys2.p, vals.p, ix->d_pos, (uint32_t)len, 2 * k + 1));
        HIPCHK(h, launch(h, map_bucket_offsets_kernel, map_grid(nb, h), 256, (const uint32_t*)keys2.p, (unsigned long long)len, nb, ix->d_off));
    } else {
        HIPCHK(h, hipMemsetAsync(ix->d_off, 0, sizeof(uint32_t) * nb, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ASM_OK;
}

} /* extern "C++" */

int asm_index_build(asm_handle* h, const char* text, const uint64_t* seq_off, int32_t n_seqs, int k, asm_index** out) {
    if (!out || !seq_off) return fail(h, ASM_EINVAL, "asm_index_build: NULL argument");
    *out = nullptr;
    if (n_seqs < 1 || n_seqs >= MAP_MAX_SEQS) return fail(h, ASM_EINVAL, "asm_index_build: n_seqs must be in [1, 2^26)");
    if (k < ASM_MAP_MIN_K || k > ASM_MAP_MAX_K) return fail(h, ASM_EINVAL, "asm_index_build: k must be in [8, 14]");
    if (seq_off[0] != 0) return fail(h, ASM_EINVAL, "asm_index_build: seq_off[0] must be 0");
    for (int32_t r = 0; r < n_seqs; r++)
        if (seq_off[r + 1] < seq_off[r]) return fail(h, ASM_EINVAL, "asm_index_build: seq_off must be non-decreasing");
    const uint64_t len = seq_off[n_seqs];
    if (len >= 0xffffffffull) return fail(h, ASM_EUNSUPPORTED, "asm_index_build: total reference length must be below 2^32");
    if (len && !text) return fail(h, ASM_EINVAL, "asm_index_build: text is NULL");
    if (!h) return fail(h, ASM_EINVAL, "asm_index_build: NULL handle");
    HIPCHK(h, hipSetDevice(h->device));
    std::unique_ptr<asm_index> ix(new asm_index);
    ix->device = h->device, ix->k = k, ix->n_seqs = n_seqs, ix->len = len;
    ix->seq_off.assign(seq_off, seq_off + n_seqs + 1);
    HIPCHK(h, big_malloc(h, (void**)&ix->d_text, len + 16));
    HIPCHK(h, big_malloc(h, (void**)&ix->d_seq_off, sizeof(unsigned long long) * (size_t)(n_seqs + 1)));
    if (len) HIPCHK(h, hipMemcpyAsync(ix->d_text, text, len, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ix->d_seq_off, seq_off, sizeof(uint64_t) * (size_t)(n_seqs + 1), hipMemcpyHostToDevice, h->stream));
    if (const int rc = map_index_stage(h, ix.get())) return rc;
    *out = ix.release();
    return ASM_OK;
}

int asm_index_free(asm_handle* h, asm_index* ix) {
    (void)h;
    delete ix;
    return ASM_OK;
}

int32_t asm_index_n_seqs(const asm_index* ix) { return ix ? ix->n_seqs : 0; }

uint64_t asm_index_seq_len(const asm_index* ix, int32_t r) {
    return ix && r >= 0 && r < ix->n_seqs ? ix->seq_off[(size_t)r + 1] - ix->seq_off[(size_t)r] : 0;
}

const char* asm_index_seq_name(const asm_index* ix, int32_t r) {
    return ix && r >= 0 && (size_t)r < ix->names.size() ? ix->names[(size_t)r].c_str() : "";
}

int asm_index_get_text(asm_handle* h, const asm_index* ix, uint64_t start, uint64_t n, char* dst) {
    if (!ix || (n && !dst)) return fail(h, ASM_EINVAL, "asm_index_get_text: NULL argument");
    if (start > ix->len || n > ix->len - start) return fail(h, ASM_EINVAL, "asm_index_get_text: the range must lie inside the text");
    if (!h) return fail(h, ASM_EINVAL, "asm_index_get_text: NULL handle");
    if (ix->device != h->device) return fail(h, ASM_EINVAL, "asm_index_get_text: the index lives on another device");
    HIPCHK(h, hipSetDevice(h->device));
    if (n) HIPCHK(h, hipMemcpyAsync(dst, ix->d_text + start, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ASM_OK;
}

int asm_map_reads(asm_handle* h, const asm_index* ix, int64_t n, const char* reads, const uint32_t* read_off,
                  const asm_map_params* p, asm_map_hit* out, uint16_t* cigar_ops, int cigar_cap, uint8_t* cigar_nops) {
    if (!p || !ix || n < 0 || !read_off || (n > 0 && (!reads || !out))) return fail(h, ASM_EINVAL, "asm_map_reads: bad arguments");
    const MapCigars cg = {cigar_ops, cigar_cap, cigar_nops};
    if (const int rc = map_check_args(h, ix, "asm_map_reads", "read", {n, p, {read_off, nullptr}, nullptr, nullptr, 0, 0, 0, cg}))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    /* under ASM_MAPQ_GAP the run key holds the read in its top 31 bits */
    const int64_t step = h->mapq_model == ASM_MAPQ_GAP ? std::min<int64_t>(h->map_chunk, (int64_t)1 << 30) : h->map_chunk;
    return map_mapq_call(h, (size_t)n, [&] {
        return map_chunks(n, step, [&](int64_t c0, int64_t cn) {
            return map_chunk(h, ix, cn, reads, read_off + c0, p, out + c0, cg.at((size_t)c0), h->last_mapq.data() + c0);
        });
    });
}

int asm_map_reads_all(asm_handle* h, const asm_index* ix, int64_t n, const char* reads, const uint32_t* read_off,
                      const asm_map_params* p, int strata, int max_hits, uint32_t* n_hits, asm_map_hit* out, uint16_t* cigar_ops,
                      int cigar_cap, uint8_t* cigar_nops) {
    if (!p || !ix || n < 0 || !read_off || (n > 0 && (!reads || !out || !n_hits)))
        return fail(h, ASM_EINVAL, "asm_map_reads_all: bad arguments");
    const MapCigars cg = {cigar_ops, cigar_cap, cigar_nops};
    if (const int rc = map_check_args(h, ix, "asm_map_reads_all", "read",
                                      {n, p, {read_off, nullptr}, nullptr, "max_hits", strata, ASM_MAP_MAX_ERRORS, max_hits, cg}))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    /* the run key holds the read in its top 31 bits */
    return map_mapq_call(h, (size_t)n * max_hits, [&] {
        return map_chunks(n, std::min<int64_t>(h->map_chunk, (int64_t)1 << 30), [&](int64_t c0, int64_t cn) {
            const size_t o = (size_t)c0 * max_hits;
            return map_chunk_all(h, ix, cn, reads, read_off + c0, p, strata, max_hits, n_hits + c0, out + o, cg.at(o),
                                 h->last_mapq.data() + o);
        });
    });
}

int asm_map_pairs(asm_handle* h, const asm_index* ix, int64_t n, const char* reads1, const uint32_t* off1, const char* reads2,
                  const uint32_t* off2, const asm_map_params* p, const asm_pair_params* pp, asm_map_hit* out, int32_t* tlen,
                  uint32_t* n_concordant, uint16_t* cigar_ops, int cigar_cap, uint8_t* cigar_nops) {
    if (!p || !pp || !ix || n < 0 || !off1 || !off2 || (n > 0 && (!reads1 || !reads2 || !out || !tlen || !n_concordant)))
        return fail(h, ASM_EINVAL, "asm_map_pairs: bad arguments");
    const MapCigars cg = {cigar_ops, cigar_cap, cigar_nops};
    if (const int rc = map_check_args(h, ix, "asm_map_pairs", "mate", {n, p, {off1, off2}, pp, nullptr, 0, 0, 0, cg})) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const MapPairsIn m = {reads1, off1, reads2, off2};
    return map_mapq_call(h, 2 * (size_t)n, [&] {
        return map_chunks(n, map_pair_step(h), [&](int64_t c0, int64_t cn) {
            return map_chunk_pairs(h, ix, cn, m.at(c0), p, pp, out + 2 * c0, tlen + c0, n_concordant + c0, cg.at((size_t)c0 * 2),
                                   h->last_mapq.data() + 2 * c0);
        });
    });
}

int asm_map_pairs_all(asm_handle* h, const asm_index* ix, int64_t n, const char* reads1, const uint32_t* off1, const char* reads2,
                      const uint32_t* off2, const asm_map_params* p, const asm_pair_params* pp, int strata, int max_pairs,
                      uint32_t* n_pairs, asm_map_hit* out, int32_t* tlen, uint32_t* n_concordant, uint16_t* cigar_ops, int cigar_cap,
                      uint8_t* cigar_nops) {
    if (!p || !pp || !ix || n < 0 || !off1 || !off2 || (n > 0 && (!reads1 || !reads2 || !out || !tlen || !n_concordant)))
        return fail(h, ASM_EINVAL, "asm_map_pairs_all: bad arguments");
    if (n > 0 && !n_pairs) return fail(h, ASM_EINVAL, "asm_map_pairs_all: n_pairs is NULL");
    const MapCigars cg = {cigar_ops, cigar_cap, cigar_nops};
    if (const int rc = map_check_args(h, ix, "asm_map_pairs_all", "mate",
                                      {n, p, {off1, off2}, pp, "max_pairs", strata, 2 * ASM_MAP_MAX_ERRORS, max_pairs, cg}))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const MapPairsIn m = {reads1, off1, reads2, off2};
    return map_mapq_call(h, 2 * (size_t)n * max_pairs, [&] {
        return map_chunks(n, map_pair_step(h), [&](int64_t c0, int64_t cn) {
            const size_t o = (size_t)c0 * max_pairs;
            return map_chunk_pairs_all(h, ix, cn, m.at(c0), p, pp, strata, max_pairs, n_pairs + c0, out + 2 * o, tlen + o,
                                       n_concordant + c0, cg.at(2 * o), h->last_mapq.data() + 2 * o);
        });
    });
}

int asm_map_set_mapq_model(asm_handle* h, int model) { /* the model is checked first, so that the check needs no device */
    if (model != ASM_MAPQ_REFERENCE && model != ASM_MAPQ_GAP)
        return fail(h, ASM_EINVAL, "asm_map_set_mapq_model: model must be ASM_MAPQ_REFERENCE (0) or ASM_MAPQ_GAP (1)");
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_map_set_mapq_model: NULL handle");
    h->mapq_model = model;
    return ASM_OK;
}

int asm_map_get_mapq_model(const asm_handle* h) { return h ? h->mapq_model : ASM_MAPQ_REFERENCE; }

static_assert(ASM_MAP_MD_CAP == MD_ROW_CAP, "the ABI's ASM_MAP_MD_CAP is the MD row of asm_md.h");

int asm_map_set_sam_tags(asm_handle* h, unsigned mask) { /* the mask is checked first, so that the check needs no device */
    if (mask & ~(unsigned)ASM_SAM_TAG_MD) return fail(h, ASM_EINVAL, "asm_map_set_sam_tags: mask may hold ASM_SAM_TAG_MD (1) only");
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_map_set_sam_tags: NULL handle");
    h->sam_tags = mask;
    return ASM_OK;
}

unsigned asm_map_get_sam_tags(const asm_handle* h) { return h ? h->sam_tags : 0u; }

int asm_map_set_output_format(asm_handle* h, int format) { /* the value is checked first, so that the check needs no device */
    if (format != ASM_OUT_SAM && format != ASM_OUT_BAM)
        return fail(h, ASM_EINVAL, "asm_map_set_output_format: format must be ASM_OUT_SAM (0) or ASM_OUT_BAM (1)");
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_map_set_output_format: NULL handle");
    h->out_format = format;
    return ASM_OK;
}

int asm_map_get_output_format(const asm_handle* h) { return h ? h->out_format : ASM_OUT_SAM; }

int asm_md_format(const uint16_t* ops, int nops, const char* read_on_strand, int read_len, const char* ref_window, int ref_len,
                  char* out, size_t out_cap) {
    if (nops < 0 || read_len < 0 || ref_len < 0 || (nops > 0 && !ops) || (read_len > 0 && !read_on_strand) || (ref_len > 0 && !ref_window) ||
        !out)
        return fail(nullptr, ASM_EINVAL, "asm_md_format: bad arguments");
    MdRowSink o{out, out_cap > 0x7fffffffull ? 0x7fffffffu : (uint32_t)out_cap}; /* the length is returned as an int */
    /* upper case on both sides, as the mapper holds its reads and its text */
    const bool ok = md_format(ops, (uint32_t)nops, [&](uint32_t p) { return sam_upper(read_on_strand[p]); }, (uint32_t)read_len,
                              [&](uint32_t p) { return sam_upper(ref_window[p]); }, (uint32_t)ref_len, o);
    if (!ok)
        return fail(nullptr, ASM_EINVAL, "asm_md_format: the row must hold M, I and D only and consume exactly read_len read and ref_len reference bases");
    if (o.cur >= o.cap) return fail(nullptr, ASM_EINVAL, "asm_md_format: out_cap is too small");
    out[o.cur] = 0;
    return (int)o.cur;
}

int asm_map_last_mapq(asm_handle* h, uint8_t* dst, int64_t count) {
    if (count < 0) return fail(h, ASM_EINVAL, "asm_map_last_mapq: count must be >= 0");
    if (count > 0 && !dst) return fail(h, ASM_EINVAL, "asm_map_last_mapq: dst is NULL");
    if (!h) return fail(nullptr, ASM_EINVAL, "asm_map_last_mapq: NULL handle");
    if (!h->last_mapq_valid) return fail(h, ASM_EINVAL, "asm_map_last_mapq: no in-memory mapping call has succeeded on this handle");
    if ((uint64_t)count != h->last_mapq.size())
        return fail(h, ASM_EINVAL, "asm_map_last_mapq: count must be the last call's record slots (" + std::to_string(h->last_mapq.size()) + ")");
    std::copy(h->last_mapq.begin(), h->last_mapq.end(), dst);
    return ASM_OK;
}
