// The device-free part of the C ABI's host side: everything in libasm_mi355x.so that runs on the CPU and never calls HIP —
// the seeded generator's host loop (asm_generate_pairs), the stale-tail state arithmetic (asm_tail_state_advance), the CIGAR
// formatter (asm_cigar_format), and the host threads of the two streamed-file calls: the three-slot hand-over between a reader
// thread and the caller's thread (ChunkReader) with its fill policies — asm_stream_seq_file's newline scanning over the
// persistent reader pool (PairsFill), asm_map_file's FASTQ chunk cutter (asm_fastq_cut, FastqFill), asm_map_pairs_file's two
// files in step (asm_fastq_cut_n, FastqPairFill) and asm_index_build_file's FASTA cutter (asm_fasta_cut, FastaFill), with the BGZF
// forms of the two FASTQ policies (BgzfFill, BgzfPairFill) — and the SAM writer (ChunkWriter).
//
// Kept in a header without any HIP include so that the SAME code is compiled twice: into the product by hipcc (asm_capi.hip),
// and by plain g++ under -fsanitize=thread / address,undefined into host/asm_host_check.cpp (`make -C oracle asan`,
// tests/test_sanitizers.py).  GPU AddressSanitizer is not available on the target pool; this is the part of the library a CPU
// sanitizer can see.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/types.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/asm_mi355x.h"
#include "asm_gen.h"
#include "asm_bgzf_walk.h"

namespace asm_host {

// ---- generator (benchmark_dataset.h:85-253 restated over a counter-based stream, asm_gen.h) ---------------------------------
inline int check_gen(const asm_gen_config* cfg, std::string& err) {
    if (!cfg) return err = "generator: cfg is NULL", ASM_EINVAL;
    if (cfg->len_lo < 1 || cfg->len_hi < cfg->len_lo || cfg->len_hi > ASM_MAX_LENGTH)
        return err = "generator: need 1 <= len_lo <= len_hi <= ASM_MAX_LENGTH", ASM_EINVAL;
    if (cfg->kind == ASM_GEN_EXACT_ERRORS || cfg->kind == ASM_GEN_UP_TO_ERRORS) {
        /* benchmark_dataset.h:192-204 */
        if (!(cfg->err >= 0.f && cfg->err <= 0.7f)) return err = "generator: err must be in [0, 0.7]", ASM_EINVAL;
        if (!(cfg->mismatch_rate >= 0.f && cfg->mismatch_rate <= 1.f)) return err = "generator: mismatch_rate must be in [0, 1]", ASM_EINVAL;
    } else if (cfg->kind == ASM_GEN_PER_BASE) {
        if (!(cfg->p_sub >= 0.f && cfg->p_ins >= 0.f && cfg->p_del >= 0.f && cfg->p_sub + cfg->p_del <= 1.f && cfg->p_ins <= 1.f))
            return err = "generator: per-base rates out of range", ASM_EINVAL;
    } else {
        return err = "generator: unknown kind", ASM_EINVAL;
    }
    return ASM_OK;
}

inline int generate_pairs(const asm_gen_config* cfg, int64_t first, int64_t n, uint32_t* read_off, uint32_t* ref_off, char* reads,
                          size_t reads_cap, char* refs, size_t refs_cap, std::string& err) {
    int rc = check_gen(cfg, err);
    if (rc) return rc;
    if (n < 0 || first < 0 || !read_off || !ref_off) return err = "asm_generate_pairs: bad arguments", ASM_EINVAL;
    uint64_t ra = 0, rb = 0;
    for (int64_t i = 0; i < n; i++) {
        int m, nn;
        asm_gen_lengths(cfg, (uint64_t)(first + i), &m, &nn);
        read_off[i] = (uint32_t)ra;
        ref_off[i] = (uint32_t)rb;
        ra += (uint64_t)m;
        rb += (uint64_t)nn;
        if (ra > 0xffffffffull || rb > 0xffffffffull) return err = "asm_generate_pairs: batch exceeds 4 GiB of text; split it", ASM_EUNSUPPORTED;
    }
    read_off[n] = (uint32_t)ra;
    ref_off[n] = (uint32_t)rb;
    if (!reads || !refs) return ASM_OK; /* sizing pass */
    if (reads_cap < ra || refs_cap < rb) return err = "asm_generate_pairs: output buffers too small", ASM_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) {
        char rd[ASM_MAX_LENGTH + 8], tx[ASM_GEN_MAX_TEXT];
        int m, nn;
        asm_gen_pair(cfg, (uint64_t)(first + i), rd, tx, &m, &nn);
        memcpy(reads + read_off[i], rd, (size_t)m);
        memcpy(refs + ref_off[i], tx, (size_t)nn);
    }
    return ASM_OK;
}

// ---- Greedy's stale tails: the host side of the chain across batches (hurdle_matrix.h:136-137,630-631) -----------------------
#define TAIL_NONE 0xFFu
// Where the trajectory that starts in `slot` sits after n pairs: every conversion leaves buf'[q] = buf[SRC[q]],
// SRC[q] = 8 * (q & 15) + P[q >> 4] (bit_convert.cpp:265-330), and SRC has order 10.
static inline int tail_slot_after(int slot, long long n) {
    for (int i = 0, r = (int)(n % 10); i < r; i++) {
        const int v = slot & 7, low2 = v & 3;
        const int pv = (low2 == 1 || low2 == 2) ? (v ^ 3) : v;
        slot = (pv << 4) | (slot >> 3);
    }
    return slot;
}

// The same step on all 128 slots of a buffer at once, one bit per slot (bit q of w[q >> 5] = slot q): what the resolver's
// device passes run per pair and plane (csrc/asm_tails.h).  after[q] = before[SRC[q]] reads the buffer as 16 bytes of 8 bits and
// leaves 8 halfwords of 16 bits: halfword j, bit r = byte r, bit P[j] — two 8x8 bit transposes (bytes 0-7, bytes 8-15), then
// byte (P[j]) of the first next to byte (P[j]) of the second.  constexpr: clang compiles these for host and device alike, and
// the static_assert below checks the permutation against its definition for every slot while the library is being compiled.
struct TailBits {
    uint32_t w[4];
};
constexpr uint32_t tail_bfi(uint32_t m, uint32_t x, uint32_t y) { return (x & m) | (y & ~m); } /* v_bfi_b32 */
constexpr void tail_transpose8(uint32_t& lo, uint32_t& hi) { /* bytes 0-3 in lo, 4-7 in hi: byte c, bit r <- byte r, bit c */
    lo = tail_bfi(0xAA55AA55u, lo, tail_bfi(0x00AA00AAu, lo >> 7, lo << 7));
    hi = tail_bfi(0xAA55AA55u, hi, tail_bfi(0x00AA00AAu, hi >> 7, hi << 7));
    lo = tail_bfi(0xCCCC3333u, lo, tail_bfi(0x0000CCCCu, lo >> 14, lo << 14));
    hi = tail_bfi(0xCCCC3333u, hi, tail_bfi(0x0000CCCCu, hi >> 14, hi << 14));
    const uint32_t l2 = tail_bfi(0x0F0F0F0Fu, lo, hi << 4);
    hi = tail_bfi(0xF0F0F0F0u, hi, lo >> 4);
    lo = l2;
}
constexpr TailBits tail_permute(TailBits v) {
    uint32_t a0 = v.w[0], a1 = v.w[1], b0 = v.w[2], b1 = v.w[3];
    tail_transpose8(a0, a1);
    tail_transpose8(b0, b1);
    TailBits o{};
    o.w[0] = tail_bfi(0x00FF00FFu, a0, b0 << 8);      /* halfwords 0, 1: bytes P[0] = 0 and P[1] = 2 of both transposes */
    o.w[1] = tail_bfi(0x00FF00FFu, a0 >> 8, b0);      /* halfwords 2, 3: bytes 1, 3 */
    o.w[2] = tail_bfi(0x00FF00FFu, a1, b1 << 8);      /* halfwords 4, 5: bytes 4, 6 */
    o.w[3] = tail_bfi(0x00FF00FFu, a1 >> 8, b1);      /* halfwords 6, 7: bytes 5, 7 */
    return o;
}
constexpr uint32_t tail_prefix_word(uint32_t len, uint32_t lo) { /* the bits of [0, len) that fall into slots [lo, lo + 32) */
    return len >= lo + 32u ? 0xFFFFFFFFu : (len > lo ? (1u << ((len - lo) & 31u)) - 1u : 0u);
}
constexpr TailBits tail_prefix(uint32_t len) { /* slots [0, len), len <= 128 */
    return TailBits{{tail_prefix_word(len, 0u), tail_prefix_word(len, 32u), tail_prefix_word(len, 64u), tail_prefix_word(len, 96u)}};
}
constexpr bool tail_permute_selfcheck() {
    for (int q = 0; q < 128; q++) { /* a byte in slot s moves to tail_slot_after(s, 1) */
        TailBits one{};
        one.w[q >> 5] = 1u << (q & 31);
        const TailBits got = tail_permute(one);
        const int v = q & 7, low2 = v & 3, pv = (low2 == 1 || low2 == 2) ? (v ^ 3) : v, to = (pv << 4) | (q >> 3);
        for (int d = 0; d < 4; d++)
            if (got.w[d] != ((to >> 5) == d ? 1u << (to & 31) : 0u)) return false;
    }
    return true;
}
static_assert(tail_permute_selfcheck(), "tail_permute does not move slot s to SRC^-1[s]");

inline int tail_state_advance(uint8_t* state, const uint8_t* summary, int64_t n_pairs, std::string& err) {
    if (!state || !summary || n_pairs < 0) return err = "asm_tail_state_advance: bad argument", ASM_EINVAL;
    uint8_t next[256];
    for (int side = 0; side < 2; side++)
        for (int s = 0; s < 128; s++) {
            const uint8_t w = summary[side * 128 + s];
            if (w != TAIL_NONE && w > 3) return err = "asm_tail_state_advance: summary entries are 0..3 or 0xFF", ASM_EINVAL;
            next[side * 128 + tail_slot_after(s, (long long)n_pairs)] = w != TAIL_NONE ? w : state[side * 128 + s];
        }
    memcpy(state, next, 256);
    return ASM_OK;
}

// ---- CIGAR rows -> text (hurdle_matrix::_update_CIGAR, hurdle_matrix.h:238-251; '=' and 'X' come from the NW traceback) -----
inline int cigar_format(const uint16_t* ops, int nops, int cap, char* out, size_t out_cap) {
    if (!ops || !out || out_cap == 0) return ASM_EINVAL;
    size_t len = 0;
    out[0] = 0;
    const int cnt = nops < cap ? nops : cap;
    for (int i = 0; i < cnt; i++) {
        const char op = "MID=X???"[ops[i] & 7];
        const int w = snprintf(out + len, out_cap - len, "%d%c", (int)(ops[i] >> 3), op);
        if (w < 0 || len + (size_t)w >= out_cap) return ASM_EINVAL;
        len += (size_t)w;
    }
    /* truncated row, or one that may be: the producers' counts are bytes that saturate, 255 = "255 or more" */
    return nops > cap || nops >= 255 ? ASM_EUNSUPPORTED : ASM_OK;
}

// ---- `>read\n<ref\n` files (benchmark_utils.h:325-352): newline scanning and the reader side of the streaming ingest ---------
/* newlines in [p, p+len): count and the positions (relative to p) of the last two */
struct NlScan {
    int64_t count = 0;
    int64_t last = -1, prev = -1;
};

inline void nl_merge(NlScan& tot, const NlScan& r) { /* append a later segment's summary (positions on one common base) */
    if (!r.count) return;
    tot.count += r.count;
    if (r.count >= 2) tot.prev = r.prev;
    else tot.prev = tot.last; /* the segment's only newline: the one before it is the running last */
    tot.last = r.last;
}

inline NlScan scan_range(const char* base, size_t a, size_t b) { /* newlines of base[a, b), positions relative to base */
    NlScan r;
    const char* q = base + a;
    const char* end = base + (a < b ? b : a);
    while (q < end) {
        const char* hit = (const char*)memchr(q, '\n', (size_t)(end - q));
        if (!hit) break;
        r.count++, r.prev = r.last, r.last = (int64_t)(hit - base);
        q = hit + 1;
    }
    return r;
}

inline NlScan scan_newlines(const char* p, size_t len, int threads) {
    if (threads < 1) threads = 1;
    std::vector<NlScan> part((size_t)threads);
    std::vector<std::thread> pool;
    const size_t step = (len + (size_t)threads - 1) / (size_t)threads;
    auto work = [&](int t) {
        const size_t a = (size_t)t * step, b = a + step < len ? a + step : len;
        part[(size_t)t] = scan_range(p, a, b);
    };
    for (int t = 1; t < threads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    NlScan tot;
    for (const NlScan& r : part) nl_merge(tot, r);
    return tot;
}

/* Worker threads that live as long as one asm_stream_seq_file call: a chunk is read AND scanned for newlines by the same
 * workers in one go (each its own slice: pread into the pinned buffer, then memchr over the bytes it has just written).
 * Round 2 started 2 x 8 threads per chunk — half a millisecond of every 64 MB chunk — and passed over the data twice. */
class StreamWorkers {
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_work_, cv_done_;
    std::function<void(int)> job_;
    int generation_ = 0, pending_ = 0;
    bool quit_ = false;

public:
    explicit StreamWorkers(int n) {
        for (int t = 0; t < n; t++)
            threads_.emplace_back([this, t]() {
                int seen = 0;
                for (;;) {
                    std::function<void(int)> job;
                    {
                        std::unique_lock<std::mutex> lk(mu_);
                        cv_work_.wait(lk, [&] { return quit_ || generation_ != seen; });
                        if (quit_) return;
                        seen = generation_;
                        job = job_;
                    }
                    job(t);
                    {
                        std::lock_guard<std::mutex> lk(mu_);
                        if (--pending_ == 0) cv_done_.notify_all();
                    }
                }
            });
    }
    int size() const { return (int)threads_.size(); }
    void run(const std::function<void(int)>& job) { /* job(t) on every worker t; returns when all are done */
        std::unique_lock<std::mutex> lk(mu_);
        job_ = job;
        pending_ = (int)threads_.size();
        generation_++;
        cv_work_.notify_all();
        cv_done_.wait(lk, [&] { return pending_ == 0; });
    }
    ~StreamWorkers() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_work_.notify_all();
        for (auto& th : threads_) th.join();
    }
};

/* buf[0, head) is already there (the carry of the chunk before); reads `len` file bytes behind it and returns the newline
 * summary of buf[0, head + len) */
inline NlScan read_and_scan(StreamWorkers& pool, int fd, char* buf, size_t head, size_t len, off_t off, std::atomic<bool>& failed) {
    const int threads = pool.size();
    std::vector<NlScan> part((size_t)threads + 1);
    const size_t step = ((len + (size_t)threads - 1) / (size_t)threads + 4095) & ~(size_t)4095;
    part[0] = scan_range(buf, 0, head);
    pool.run([&](int t) {
        /* read and scan in blocks of 1 MB: the scan then finds the bytes the copy has just written still in the core's cache
         * (scanning an 8 MB slice after reading all of it fetched every byte from DRAM a second time) */
        const size_t a0 = (size_t)t * step, b = a0 + step < len ? a0 + step : len;
        NlScan mine;
        for (size_t a = a0; a < b;) {
            const size_t blk_end = a + ((size_t)1 << 20) < b ? a + ((size_t)1 << 20) : b;
            const size_t blk_a = a;
            while (a < blk_end) {
                const ssize_t got = pread(fd, buf + head + a, blk_end - a, off + (off_t)a);
                if (got <= 0) {
                    failed = true;
                    return;
                }
                a += (size_t)got;
            }
            nl_merge(mine, scan_range(buf, head + blk_a, head + blk_end));
        }
        part[(size_t)t + 1] = mine;
    });
    NlScan tot;
    for (const NlScan& r : part) nl_merge(tot, r);
    return tot;
}

struct ChunkSlot { /* one (pinned) host buffer */
    char* buf = nullptr;
    size_t cap = 0;          /* usable bytes */
    size_t bytes = 0;        /* raw bytes to ship: whole units only */
    size_t bytes1 = 0;       /* two files in step: the bytes of file 1's records, in front of file 2's */
    int64_t units = 0;       /* pairs, or FASTQ records */
    int64_t extra_lines = 0; /* FASTQ, last chunk: lines behind the last whole record (a truncated record) */
    bool last = false;
    bool ready = false;     /* filled by the reader, not yet taken by the consumer */
    bool in_flight = false; /* the consumer has started an asynchronous copy out of it; wait_shipped(slot) tells when it is over */
};

struct ChunkCut { /* what a fill policy reports: buf[0, have) is there, buf[0, boundary) are `units` whole units */
    size_t have = 0, boundary = 0, bytes1 = 0;
    int64_t units = 0, extra_lines = 0;
    bool eof = false;
};

/* The reader thread of a streamed file and its hand-over to the caller's thread.  Three slots in rotation: the reader fills slot
 * c % 3 with chunk c and marks it ready; the consumer takes the chunks in order (wait_ready), starts its copy out of the buffer
 * and gives the slot back (consumed), after which the reader may refill it once wait_shipped(slot) says the copy is over.
 * How a slot is filled and cut is the policy's: fill(slot, q, carry, want, cut) puts the carry (what the chunk before left behind
 * its boundary) and about `want` more file bytes into slot q and reports the cut; false: reading failed. */
template <class Fill>
class ChunkReader {
    Fill fill_;
    const size_t chunk_, first_chunk_;
    const std::function<void(int)> wait_shipped_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::atomic<bool> failed_{false}, stop_{false};
    double read_seconds_ = 0;
    std::thread reader_;

    void loop() {
        std::vector<char> carry;
        for (int c = 0; !stop_; c++) {
            ChunkSlot& s = slot[c % 3];
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !s.ready; });
                if (stop_) return;
            }
            if (s.in_flight) { /* the copy out of this buffer (three chunks ago) must be over before it is overwritten */
                wait_shipped_(c % 3);
                s.in_flight = false;
            }
            const auto t0 = std::chrono::steady_clock::now();
            /* chunk c takes first_chunk << c file bytes until that reaches `chunk`: the consumer's pipeline (ship, parse, align) starts
             * after the FIRST chunk is in memory, so a small first chunk shortens the fill of the pipeline and the large later ones
             * keep the per-chunk costs rare */
            const size_t want = c < 30 && (first_chunk_ << c) < chunk_ ? first_chunk_ << c : chunk_;
            ChunkCut cut;
            const bool ok = fill_(s, c % 3, carry, want, cut);
            carry.clear();
            if (ok && !cut.eof) carry.assign(s.buf + cut.boundary, s.buf + cut.have);
            read_seconds_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (!ok) failed_ = true;
            {
                std::lock_guard<std::mutex> lk(mu_);
                s.bytes = cut.boundary, s.bytes1 = cut.bytes1, s.units = cut.units, s.extra_lines = cut.extra_lines, s.last = cut.eof, s.ready = true;
            }
            cv_.notify_all();
            if (!ok || cut.eof) return;
        }
    }

public:
    ChunkSlot slot[3]; /* the caller sets buf and cap (usable bytes; allocate cap + 64) before start() */

    /* first_chunk: file bytes of chunk 0 (0 or >= chunk: every chunk takes `chunk`); fill_args: the policy's constructor's */
    template <class... A>
    ChunkReader(size_t chunk, size_t first_chunk, std::function<void(int)> wait_shipped, A&&... fill_args)
        : fill_(std::forward<A>(fill_args)...), chunk_(chunk), first_chunk_(first_chunk > 0 && first_chunk < chunk ? first_chunk : chunk),
          wait_shipped_(std::move(wait_shipped)) {}
    ~ChunkReader() { stop(); }
    void start() { reader_ = std::thread([this] { loop(); }); }
    /* consumer: chunk c (in order, c = 0, 1, ...); nullptr when reading failed */
    ChunkSlot* wait_ready(int c) {
        ChunkSlot& s = slot[c % 3];
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return s.ready || failed_.load(); });
        }
        return failed_ ? nullptr : &s;
    }
    /* consumer: done with chunk c's slot, apart from an asynchronous copy out of it when `in_flight` */
    void consumed(int c, bool in_flight) {
        ChunkSlot& s = slot[c % 3];
        s.in_flight = in_flight;
        {
            std::lock_guard<std::mutex> lk(mu_);
            s.ready = false; /* the reader may refill it once wait_shipped has returned */
        }
        cv_.notify_all();
    }
    void stop() {
        {   /* under the mutex: the reader evaluates its wait predicate under it, and a store between its test and its block
               would otherwise be a lost wake-up */
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (reader_.joinable()) reader_.join();
    }
    bool failed() const { return failed_.load(); }
    double read_seconds() const { return read_seconds_; } /* after stop() */
    /* what the policy keeps for its caller: after the last chunk or stop(); what it keeps per slot (BgzfFill::info) goes with the
     * slot's hand-over: written before the slot is ready, read before consumed() */
    const Fill& policy() const { return fill_; }
    Fill& policy() { return fill_; } /* for what the consumer hands back to it (BgzfPairFill::feedback) */
};

/* asm_stream_seq_file's policy: `want` more file bytes through the reader pool (reads stop at cap - 8), cut behind the last
 * complete pair; at the end of the file a missing final newline and, for an odd line count, an empty reference line are appended;
 * max_pairs > 0 ends the stream inside the chunk that reaches it.  A pair longer than a whole slot is a failure. */
struct PairsFill {
    const int fd;
    const size_t file_bytes;
    const int reader_threads;
    int64_t pairs_left;
    size_t file_off = 0;
    std::optional<StreamWorkers> workers; /* started by the reader thread with its first chunk */
    std::atomic<bool> failed{false};
    PairsFill(int fd_, size_t file_bytes_, int reader_threads_, int64_t max_pairs)
        : fd(fd_), file_bytes(file_bytes_), reader_threads(reader_threads_), pairs_left(max_pairs > 0 ? max_pairs : INT64_MAX) {}

    bool operator()(ChunkSlot& s, int, const std::vector<char>& carry, size_t want, ChunkCut& cut) {
        if (!workers) workers.emplace(reader_threads);
        size_t have = carry.size();
        if (have) memcpy(s.buf, carry.data(), have);
        if (file_off + want > file_bytes) want = file_bytes - file_off;
        if (have + want > s.cap - 8) want = s.cap - 8 - have;
        NlScan sc = read_and_scan(*workers, fd, s.buf, have, want, (off_t)file_off, failed);
        if (failed) return false;
        file_off += want;
        have += want;
        bool eof = file_off >= file_bytes;
        if (eof && have && s.buf[have - 1] != '\n') { /* a last line without its newline */
            s.buf[have++] = '\n';
            sc.prev = sc.last, sc.last = (int64_t)have - 1, sc.count++;
        }
        if (eof && (sc.count & 1)) { /* a read line without its reference line: an empty reference */
            s.buf[have++] = '\n';
            sc.prev = sc.last, sc.last = (int64_t)have - 1, sc.count++;
        }
        int64_t lines = sc.count & ~(int64_t)1;
        size_t boundary = lines == 0 ? 0 : (size_t)((lines == sc.count ? sc.last : sc.prev) + 1);
        if (lines / 2 > pairs_left) { /* max_pairs cuts inside this chunk: find the boundary of the pairs_left-th pair */
            const int64_t need = 2 * pairs_left;
            const char* q = s.buf;
            for (int64_t l = 0; l < need; l++) q = (const char*)memchr(q, '\n', (size_t)(s.buf + have - q)) + 1;
            boundary = (size_t)(q - s.buf), lines = need;
            eof = true;
        }
        /* (the two bytes appended above stay inside the slot: reads stop at cap - 8 and every slot is allocated with cap + 64) */
        if (!eof && boundary == 0 && have >= s.cap - 8) return false; /* one pair longer than a whole chunk */
        pairs_left -= lines / 2;
        cut.have = have, cut.boundary = boundary, cut.units = lines / 2, cut.eof = eof || pairs_left <= 0;
        return true;
    }
};

// ---- four-line FASTQ (asm_map_file): chunk cutting and the reader thread --------------------------------------------------------
/* the longest prefix of buf[0, nbytes) made of whole records (four lines each, every line ending in '\n'): its length, and how
 * many records it holds; *lines (may be NULL) = all newlines of buf */
inline size_t fastq_cut(const char* buf, size_t nbytes, int64_t* records, int64_t* lines = nullptr) {
    int64_t count = 0;
    size_t boundary = 0;
    const char* q = buf;
    const char* end = buf + nbytes;
    while (q < end) {
        const char* hit = (const char*)memchr(q, '\n', (size_t)(end - q));
        if (!hit) break;
        q = hit + 1;
        if ((++count & 3) == 0) boundary = (size_t)(q - buf);
    }
    if (records) *records = count / 4;
    if (lines) *lines = count;
    return boundary;
}

/* the first max_records whole records of buf[0, nbytes), or all of them when there are fewer: their length and how many they are */
inline size_t fastq_cut_n(const char* buf, size_t nbytes, int64_t max_records, int64_t* records) {
    int64_t count = 0;
    size_t boundary = 0;
    const char* q = buf;
    const char* end = buf + nbytes;
    while (q < end && count < 4 * max_records) {
        const char* hit = (const char*)memchr(q, '\n', (size_t)(end - q));
        if (!hit) break;
        q = hit + 1;
        if ((++count & 3) == 0) boundary = (size_t)(q - buf);
    }
    if (records) *records = count / 4;
    return boundary;
}

/* asm_map_file's policy: one pread loop, cut behind the last whole record (fastq_cut); when that leaves no record at all the chunk
 * takes `chunk` more bytes, and the slot grows through grow(slot, capacity, keep) (the owner of the buffers moves the first `keep`
 * bytes into a larger one and sets slot[q].buf and cap; false: out of memory).  extra_lines is reported with the last chunk, and
 * an empty file is one last, empty chunk. */
struct FastqFill {
    const int fd;
    const size_t file_bytes, chunk;
    const std::function<bool(int, size_t, size_t)> grow;
    size_t file_off = 0;
    FastqFill(int fd_, size_t file_bytes_, size_t chunk_, std::function<bool(int, size_t, size_t)> grow_)
        : fd(fd_), file_bytes(file_bytes_), chunk(chunk_), grow(std::move(grow_)) {}

    bool operator()(ChunkSlot& s, int q, const std::vector<char>& carry, size_t want, ChunkCut& cut) {
        size_t have = carry.size();
        if (have + 8 > s.cap && !grow(q, have + 8 + chunk, 0)) return false;
        if (have) memcpy(s.buf, carry.data(), have);
        int64_t lines = 0;
        for (;;) {
            if (want > file_bytes - file_off) want = file_bytes - file_off;
            if (have + want + 8 > s.cap && !grow(q, have + want + 8 + (have + want) / 4, have)) return false;
            for (size_t a = 0; a < want;) {
                const ssize_t got = pread(fd, s.buf + have + a, want - a, (off_t)(file_off + a));
                if (got <= 0) return false;
                a += (size_t)got;
            }
            file_off += want, have += want;
            cut.eof = file_off >= file_bytes;
            if (cut.eof && have && s.buf[have - 1] != '\n') s.buf[have++] = '\n'; /* a last line without its newline */
            cut.boundary = fastq_cut(s.buf, have, &cut.units, &lines);
            if (cut.units > 0 || cut.eof) break;
            want = chunk; /* one record longer than the chunk: take more */
        }
        cut.have = have, cut.extra_lines = cut.eof ? lines - 4 * cut.units : 0;
        return true;
    }
};

/* asm_map_file's policy for a BGZF-compressed file (asm_bgzf_walk.h; docs/design/mapper.md, "Compressed input"): whole members into
 * the slot until their ISIZE sum reaches `want`, which stays text bytes; units are members.  Every member's header is checked (magic, CM 8,
 * FLG 4, the XLEN walk to BC, BSIZE + 1 >= 26 and within the file, ISIZE <= 65 536).  At most 64 KiB are read behind the member at
 * hand, so the carry (a member cut by the chunk's end, still compressed) is at most 64 KiB.  The text cannot be cut into records
 * here: that is the device's.  info[q] goes with slot q: the members (offsets in the slot, output offsets the exclusive sum of
 * ISIZE), their text bytes, the file's members before them, and a bad header (its member's index in the file and file offset),
 * which ends the stream behind the members in front of it. */
struct BgzfChunkInfo {
    std::vector<InfMember> members;
    size_t text = 0;
    int64_t first_member = 0;
    size_t file_base = 0; /* the file offset of the slot's first byte */
    BgzfWalkError err;
};
/* One BGZF file under a fill policy: where the reader stands in it */
struct BgzfFile {
    int fd;
    size_t file_bytes;
    size_t file_off = 0;
    int64_t members_seen = 0;
};
/* The per-member loop both BGZF policies share.  s.buf[base, base + have) holds file f's bytes already (a compressed carry; ci.file_base
 * is set); whole members are taken behind them, at least one, until the ISIZE sum of ci reaches `want`.  Members enter ci with their
 * offsets in the slot (base included).  at: the bytes of [base, base + have) that are whole members; eof: the file ends behind them, or
 * a bad header does (ci.err).  false: reading failed or the slot could not grow. */
inline bool bgzf_fill_members(BgzfFile& f, ChunkSlot& s, int q, const std::function<bool(int, size_t, size_t)>& grow, size_t base,
                              size_t want, BgzfChunkInfo& ci, size_t& have, size_t& at, bool& eof) {
    at = 0, eof = false;
    for (;;) {
        /* the member at `at` whole: 64 KiB behind `at`, or up to the end of the file */
        size_t need = have - at < 65536 ? 65536 - (have - at) : 0;
        if (need > f.file_bytes - f.file_off) need = f.file_bytes - f.file_off;
        if (base + have + need + 8 > s.cap && !grow(q, base + have + need + 8 + (base + have + need) / 4, base + have)) return false;
        for (size_t a = 0; a < need;) {
            const ssize_t got = pread(f.fd, s.buf + base + have + a, need - a, (off_t)(f.file_off + a));
            if (got <= 0) return false;
            a += (size_t)got;
        }
        f.file_off += need, have += need;
        if (at == have) { /* the end of the file behind a whole member */
            eof = true;
            break;
        }
        const uint8_t* m = (const uint8_t*)s.buf + base + at;
        uint32_t csize = 0, dstart = 0;
        uint32_t st = bgzf_member_header(m, have - at, &csize, &dstart);
        if (st == BGZF_IN_OK && csize > have - at) st = BGZF_IN_PAST_END;
        uint32_t crc = 0, isize = 0;
        if (st == BGZF_IN_OK) {
            const uint8_t* t = m + csize - 8u;
            crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
            if (isize > INF_MAX_ISIZE) st = BGZF_IN_ISIZE;
        }
        if (st != BGZF_IN_OK) {
            ci.err.status = st, ci.err.member = (size_t)f.members_seen + ci.members.size(), ci.err.offset = ci.file_base + at;
            eof = true;
            break;
        }
        ci.members.push_back(InfMember{(unsigned long long)(base + at), (unsigned long long)ci.text, csize, dstart, isize, crc});
        at += csize, ci.text += isize;
        if (ci.text >= want) {
            eof = at == have && f.file_off >= f.file_bytes;
            break;
        }
    }
    f.members_seen += (int64_t)ci.members.size();
    return true;
}
struct BgzfFill {
    BgzfFile file;
    const std::function<bool(int, size_t, size_t)> grow;
    BgzfChunkInfo info[3];
    BgzfFill(int fd_, size_t file_bytes_, std::function<bool(int, size_t, size_t)> grow_) : file{fd_, file_bytes_}, grow(std::move(grow_)) {}

    bool operator()(ChunkSlot& s, int q, const std::vector<char>& carry, size_t want, ChunkCut& cut) {
        BgzfChunkInfo& ci = info[q];
        ci = BgzfChunkInfo();
        ci.first_member = file.members_seen;
        size_t have = carry.size(), at = 0;
        if (have + 8 > s.cap && !grow(q, have + 8 + 65536, 0)) return false;
        if (have) memcpy(s.buf, carry.data(), have);
        ci.file_base = file.file_off - have;
        if (!bgzf_fill_members(file, s, q, grow, 0, want, ci, have, at, cut.eof)) return false;
        cut.have = have, cut.boundary = at, cut.units = (int64_t)ci.members.size();
        return true;
    }
};

/* asm_map_pairs_file's policy for two BGZF-compressed files (docs/design/mapper.md, "Compressed input for pairs").  A slot holds whole
 * members of file 1 and then whole members of file 2, bytes1 the length of the first region; info[q].f[x] is BgzfFill's table for region
 * x (its members' offsets count from the slot's start), done[x]: file x is read to its end with this chunk.  What a file has behind its
 * last whole member (at most 64 KiB, still compressed) stays in a carry of the policy's own, as FastqPairFill's does (have == boundary).
 * Records cannot be counted here, so `want` text bytes are split by bytes: s1 + s2 = want with
 *     (avail1 + s1) / b1 = (avail2 + s2) / b2,   each clamped to [0, want],
 * avail: the text bytes of the file that have been handed out and are not yet paired, b: its text bytes per record.  Until the consumer has
 * reported a pair, avail is all text handed out and b the compressed bytes the file has left, which splits `want` in proportion to
 * those; from then on both come from feedback(): after chunk k, left[x] text bytes of file x lay behind the cut and `pairs` had been cut
 * in all, so avail = left + what has been handed out since chunk k, exactly, and b = (handed out up to k - left) / pairs.  The split
 * leans towards the file that is behind by as much as it is behind, whatever is in flight between reader and consumer.  A file takes
 * whole members until its share is reached (none for a share of 0), so it overshoots by less than one member.  A file that is read goes
 * without a share, and the stream ends when both are, or behind a bad header.  units: the slot's members and one for the chunk itself, so
 * that a chunk without members reaches the consumer too, which checks the ends of the files. */
struct BgzfPairChunkInfo {
    BgzfChunkInfo f[2];
    bool done[2] = {false, false};
};
struct BgzfPairFill {
    BgzfFile file[2];
    const std::function<bool(int, size_t, size_t)> grow;
    std::vector<char> carry[2];
    bool done[2];
    BgzfPairChunkInfo info[3];
    static constexpr int HIST = 16; /* chunks whose hand-outs are remembered; the reader is at most 4 ahead of the feedback */
    size_t issued[2] = {0, 0}, issued_at[HIST][2] = {};
    int64_t chunk_no = 0;
    std::mutex fb_mu; /* the consumer's report */
    int64_t fb_chunk = -1, fb_pairs = 0;
    size_t fb_left[2] = {0, 0};
    BgzfPairFill(int fd1, int fd2, size_t bytes1, size_t bytes2, std::function<bool(int, size_t, size_t)> grow_)
        : file{{fd1, bytes1}, {fd2, bytes2}}, grow(std::move(grow_)), done{bytes1 == 0, bytes2 == 0} {}

    /* consumer: chunk `chunk` (0, 1, ...) has been cut; left: the text bytes of each file behind the cut, pairs: all pairs cut so far */
    void feedback(int64_t chunk, size_t left1, size_t left2, int64_t pairs) {
        std::lock_guard<std::mutex> lk(fb_mu);
        fb_chunk = chunk, fb_left[0] = left1, fb_left[1] = left2, fb_pairs = pairs;
    }
    /* how many of `want` text bytes file 1 takes */
    size_t share1(size_t want) {
        if (done[0] || done[1]) return done[0] ? 0 : want;
        int64_t k, pairs;
        size_t left[2];
        {
            std::lock_guard<std::mutex> lk(fb_mu);
            k = fb_chunk, pairs = fb_pairs, left[0] = fb_left[0], left[1] = fb_left[1];
        }
        long double avail[2], b[2];
        const bool known = k >= 0 && chunk_no - k <= HIST && pairs > 0;
        for (int x = 0; x < 2; x++) {
            const size_t upto = known ? issued_at[k % HIST][x] : 0;
            avail[x] = (long double)(known ? left[x] + (issued[x] - upto) : issued[x]);
            b[x] = known ? (long double)(upto - left[x]) / (long double)pairs
                         : (long double)(file[x].file_bytes - file[x].file_off + carry[x].size());
        }
        if (!(b[0] > 0) || !(b[1] > 0)) return b[0] > 0 ? want : b[1] > 0 ? 0 : want / 2;
        const long double s = (b[0] * (avail[1] + (long double)want) - b[1] * avail[0]) / (b[0] + b[1]);
        return s <= 0 ? 0 : s >= (long double)want ? want : (size_t)s;
    }

    bool operator()(ChunkSlot& s, int q, const std::vector<char>&, size_t want, ChunkCut& cut) {
        BgzfPairChunkInfo& pi = info[q];
        pi = BgzfPairChunkInfo();
        const size_t s1 = share1(want);
        const size_t share[2] = {s1, want - s1};
        size_t base = 0;
        bool bad = false;
        for (int x = 0; x < 2; x++) {
            BgzfChunkInfo& ci = pi.f[x];
            ci.first_member = file[x].members_seen;
            ci.file_base = file[x].file_off - carry[x].size();
            /* a share of 0 takes nothing, unless the other file is read or takes nothing either */
            const bool other_idle = done[1 - x] || share[1 - x] == 0;
            if (!done[x] && !bad && (share[x] > 0 || other_idle)) {
                size_t have = carry[x].size(), at = 0;
                bool eof = false;
                if (base + have + 8 > s.cap && !grow(q, base + have + 8 + 65536, base)) return false;
                if (have) memcpy(s.buf + base, carry[x].data(), have);
                if (!bgzf_fill_members(file[x], s, q, grow, base, share[x], ci, have, at, eof)) return false;
                carry[x].assign(s.buf + base + at, s.buf + base + have);
                done[x] = eof;
                bad = ci.err.status != BGZF_IN_OK;
                base += at;
                issued[x] += ci.text;
            }
            pi.done[x] = done[x];
            if (x == 0) cut.bytes1 = base;
        }
        issued_at[chunk_no % HIST][0] = issued[0], issued_at[chunk_no % HIST][1] = issued[1];
        chunk_no++;
        cut.have = cut.boundary = base;
        cut.units = (int64_t)(pi.f[0].members.size() + pi.f[1].members.size()) + 1;
        cut.eof = bad || (done[0] && done[1]);
        return true;
    }
};

/* asm_map_pairs_file's policy: two FASTQ files in step.  A slot holds [R whole records of file 1][R whole records of file 2] with
 * the same R, bytes1 = the length of the first region; what a file has behind its R-th record stays in a carry of the policy's own
 * (have == boundary: the reader's generic carry stays empty).  The chunk's `want` bytes are split between the files in proportion
 * to what each has left (carry included), so the files reach their ends together and neither carry grows with the file:
 * carry_peak = the largest sum of the two carries.  No pair in reach (a record longer than the chunk): `chunk` more bytes, the slot
 * grows through grow().  The stream ends when both files are read, or when one of them is and holds no further record while the
 * other does.  For the caller, after the last chunk: records[f] = the whole records seen of file f, extra_lines[f] = the lines
 * behind the last one of a file read to its end (a truncated record), more[f] = file f holds records beyond the last pair. */
struct FastqPairFill {
    const int fd[2];
    const size_t file_bytes[2], chunk;
    const std::function<bool(int, size_t, size_t)> grow;
    size_t file_off[2] = {0, 0};
    std::vector<char> carry[2];
    bool closed[2] = {false, false}; /* the file's last line has its newline */
    int64_t records[2] = {0, 0}, extra_lines[2] = {0, 0};
    bool more[2] = {false, false};
    size_t carry_peak = 0;
    FastqPairFill(int fd1, int fd2, size_t bytes1, size_t bytes2, size_t chunk_, std::function<bool(int, size_t, size_t)> grow_)
        : fd{fd1, fd2}, file_bytes{bytes1, bytes2}, chunk(chunk_), grow(std::move(grow_)) {}

    bool operator()(ChunkSlot& s, int q, const std::vector<char>&, size_t want, ChunkCut& cut) {
        for (bool again = false;; again = true) {
            /* how many bytes of each file the slot should hold */
            const size_t left[2] = {file_bytes[0] - file_off[0], file_bytes[1] - file_off[1]};
            const long double rest[2] = {(long double)(left[0] + carry[0].size()), (long double)(left[1] + carry[1].size())};
            size_t take[2];
            for (int f = 0; f < 2; f++) {
                const size_t share = rest[0] + rest[1] > 0 ? (size_t)((long double)want * rest[f] / (rest[0] + rest[1])) : 0;
                take[f] = again ? share + 1 : share > carry[f].size() ? share - carry[f].size() : 0; /* again: progress in both */
                if (take[f] > left[f]) take[f] = left[f];
            }
            const size_t need = carry[0].size() + take[0] + carry[1].size() + take[1] + 16;
            if (need > s.cap && !grow(q, need + need / 4, 0)) return false;
            size_t at[2], have[2], cutat[2];
            int64_t n[2], lines[2];
            for (int f = 0; f < 2; f++) {
                char* dst = s.buf + (f ? have[0] : 0);
                at[f] = (size_t)(dst - s.buf), have[f] = carry[f].size();
                if (have[f]) memcpy(dst, carry[f].data(), have[f]);
                for (size_t a = 0; a < take[f];) {
                    const ssize_t got = pread(fd[f], dst + have[f] + a, take[f] - a, (off_t)(file_off[f] + a));
                    if (got <= 0) return false;
                    a += (size_t)got;
                }
                file_off[f] += take[f], have[f] += take[f];
                if (file_off[f] >= file_bytes[f] && !closed[f]) { /* a last line without its newline */
                    if (have[f] && dst[have[f] - 1] != '\n') dst[have[f]++] = '\n';
                    closed[f] = true;
                }
                cutat[f] = fastq_cut(dst, have[f], &n[f], &lines[f]);
            }
            const bool done[2] = {file_off[0] >= file_bytes[0], file_off[1] >= file_bytes[1]};
            const int64_t R = n[0] < n[1] ? n[0] : n[1];
            const bool dry[2] = {done[0] && n[0] == 0, done[1] && n[1] == 0}; /* the file holds no further record */
            const bool eof = (done[0] && done[1]) || (dry[0] && n[1] > 0) || (dry[1] && n[0] > 0);
            if (R == 0 && !eof) { /* no whole pair yet: keep everything and take more */
                for (int f = 0; f < 2; f++) carry[f].assign(s.buf + at[f], s.buf + at[f] + have[f]);
                want = chunk;
                continue;
            }
            for (int f = 0; f < 2; f++)
                if (n[f] > R) cutat[f] = fastq_cut_n(s.buf + at[f], have[f], R, nullptr);
            if (eof)
                for (int f = 0; f < 2; f++)
                    records[f] += n[f], extra_lines[f] = done[f] ? lines[f] - 4 * n[f] : 0, more[f] = !done[f] || n[f] > R;
            else
                records[0] += R, records[1] += R;
            for (int f = 0; f < 2; f++) carry[f].assign(s.buf + at[f] + cutat[f], s.buf + at[f] + have[f]);
            if (!eof && carry[0].size() + carry[1].size() > carry_peak) carry_peak = carry[0].size() + carry[1].size();
            if (cutat[1] && at[1] != cutat[0]) memmove(s.buf + cutat[0], s.buf + at[1], cutat[1]); /* file 2's records behind file 1's */
            cut.have = cut.boundary = cutat[0] + cutat[1], cut.bytes1 = cutat[0], cut.units = R, cut.eof = eof;
            return true;
        }
    }
};

/* ---- FASTA (asm_index_build_file): chunk cutting and the reader thread ---------------------------------------------------------- */
/* How much of buf[0, nbytes) to ship: a chunk may end anywhere except inside a header line, so all of it, unless its last line is a
 * header line without its newline yet: then what lies in front of that line's '>'.  at_line_start: buf[0] begins a line (else it goes
 * on with a sequence line).  *ends_in_line: the shipped prefix ends inside a line, so the next buffer starts with at_line_start = 0.
 * Only the last line is looked at: a sequence line of any length is cut like any other bytes. */
inline size_t fasta_cut(const char* buf, size_t nbytes, int at_line_start, int* ends_in_line) {
    const char* nl = nbytes ? (const char*)memrchr(buf, '\n', nbytes) : nullptr;
    const size_t s = nl ? (size_t)(nl - buf) + 1 : 0; /* where the last line begins */
    const size_t cut = (s < nbytes && (nl || at_line_start) && buf[s] == '>') ? s : nbytes;
    if (ends_in_line) *ends_in_line = cut ? buf[cut - 1] != '\n' : !at_line_start;
    return cut;
}

/* asm_index_build_file's policy: one pread loop, cut by fasta_cut; the end of the file ends the last line.  Only a header line
 * longer than the slot takes `chunk` more bytes and grows the slot through grow() (FastqFill's hook).  units = the shipped lines,
 * whole or not (newlines + 1), so that the consumer can size the chunk's newline index; an empty file is one last, empty chunk. */
struct FastaFill {
    const int fd;
    const size_t file_bytes, chunk;
    const std::function<bool(int, size_t, size_t)> grow;
    size_t file_off = 0;
    int at_line_start = 1;
    FastaFill(int fd_, size_t file_bytes_, size_t chunk_, std::function<bool(int, size_t, size_t)> grow_)
        : fd(fd_), file_bytes(file_bytes_), chunk(chunk_), grow(std::move(grow_)) {}

    bool operator()(ChunkSlot& s, int q, const std::vector<char>& carry, size_t want, ChunkCut& cut) {
        size_t have = carry.size();
        if (have + 8 > s.cap && !grow(q, have + 8 + chunk, 0)) return false;
        if (have) memcpy(s.buf, carry.data(), have);
        int in_line = 0;
        for (;;) {
            if (want > file_bytes - file_off) want = file_bytes - file_off;
            if (have + want + 8 > s.cap && !grow(q, have + want + 8 + (have + want) / 4, have)) return false;
            for (size_t a = 0; a < want;) {
                const ssize_t got = pread(fd, s.buf + have + a, want - a, (off_t)(file_off + a));
                if (got <= 0) return false;
                a += (size_t)got;
            }
            file_off += want, have += want;
            cut.eof = file_off >= file_bytes;
            cut.boundary = cut.eof ? have : fasta_cut(s.buf, have, at_line_start, &in_line);
            if (cut.boundary > 0 || cut.eof) break;
            want = chunk; /* one header line longer than the chunk: take more */
        }
        at_line_start = !in_line;
        int64_t newlines = 0;
        for (size_t a = 0; a < cut.boundary; a++) newlines += s.buf[a] == '\n'; /* (vectorised by the compiler) */
        cut.have = have, cut.units = cut.boundary ? newlines + 1 : 0;
        return true;
    }
};

/* The writer thread of asm_map_file: jobs (a buffer and its length) are written in the order they were given; before(job) waits for
 * the bytes to be there (the copy out of the device), after(job) gives the buffer back. */
class ChunkWriter {
    FILE* f_;
    struct Job {
        int slot;
        const char* buf;
        size_t bytes;
    };
    const std::function<bool(int)> before_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Job> queue_;
    bool busy_[3] = {false, false, false};
    bool quit_ = false, failed_ = false;
    double write_seconds_ = 0;
    std::thread writer_;

    void loop() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return quit_ || !queue_.empty(); });
                if (queue_.empty()) return;
                j = queue_.front();
                queue_.pop_front();
            }
            bool ok = before_(j.slot);
            const auto t0 = std::chrono::steady_clock::now();
            if (ok && j.bytes) ok = fwrite(j.buf, 1, j.bytes, f_) == j.bytes;
            write_seconds_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            {
                std::lock_guard<std::mutex> lk(mu_);
                busy_[j.slot] = false;
                if (!ok) failed_ = true;
            }
            cv_.notify_all();
        }
    }

public:
    ChunkWriter(FILE* f, std::function<bool(int)> before) : f_(f), before_(std::move(before)) { writer_ = std::thread([this] { loop(); }); }
    ~ChunkWriter() { finish(); }
    void wait_idle(int slot) { /* the job that used this slot (three jobs ago) is on disk */
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !busy_[slot]; });
    }
    void push(int slot, const char* buf, size_t bytes) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            busy_[slot] = true;
            queue_.push_back({slot, buf, bytes});
        }
        cv_.notify_all();
    }
    bool finish() { /* writes what is queued, joins; false when a write failed */
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        if (writer_.joinable()) writer_.join();
        return !failed_;
    }
    bool failed() {
        std::lock_guard<std::mutex> lk(mu_);
        return failed_;
    }
    double write_seconds() const { return write_seconds_; } /* after finish() */
};

/* The output slabs of the sorted file calls (asm_sam_sort.h): off[0 .. n] are the byte offsets of n lines laid back to back and
 * off[n] their total.  -> the cuts c[0] = 0 < c[1] < ... < c[k] = n: slab s holds the lines [c[s], c[s + 1]), as many as fit into
 * `cap` bytes and always at least one, so a slab is longer than cap only when it is a single line that is.  n = 0 gives {0}. */
inline std::vector<size_t> sam_slab_cuts(const uint64_t* off, size_t n, uint64_t cap) {
    std::vector<size_t> cuts(1, 0);
    for (size_t at = 0; at < n;) {
        size_t end = at + 1;
        while (end < n && off[end + 1] - off[at] <= cap) end++;
        cuts.push_back(end);
        at = end;
    }
    return cuts;
}

}  // namespace asm_host
