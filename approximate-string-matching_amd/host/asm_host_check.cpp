// TEST PROGRAM for CPU sanitizers (`make -C oracle asan`; tests/test_sanitizers.py runs the two builds): the device-free host
// side of the C ABI — csrc/asm_host.h, the very code libasm_mi355x.so compiles — exercised without a GPU:
//   * the generator's host loop and the `>read\n<ref\n` text it stands for,
//   * the streaming reader (ChunkReader: the three-slot hand-over) against a consumer that "ships" each chunk asynchronously on a
//     thread of its own, the way the copy stream does, with both of its fill policies: asm_stream_seq_file's (PairsFill, the reader
//     pool) — every byte of the file must come out once, in order, cut at pair boundaries, for several chunk sizes, reader counts
//     and max_pairs cuts, incl. files that end without a newline or on a read line — and asm_map_file's (FastqFill), against a
//     plain line splitter: chunk sizes with and without ramp, CRLF, truncated records, records longer than a slot, an early stop —
//     and asm_map_pairs_file's (FastqPairFill: two files in step): equal record counts in both regions of every chunk, both files
//     restored, the carry bounded by the chunk, a longer file and a truncated record in either file,
//   * asm_map_file's writer thread (ChunkWriter): order, wait_idle, and failures that must not hang,
//   * the stale-tail state arithmetic and the CIGAR formatter at their edges.
// Built twice: -fsanitize=thread (races in the hand-overs / the pool) and -fsanitize=address,undefined (buffer edges).
// Usage: asm_host_check <scratch directory>.  Prints "host check ok" and exits 0, or says what differed and exits 1.
//        asm_host_check --pairs r1.fq r2.fq <chunk bytes> <out>: the chunks FastqPairFill makes of two files, for a test to read.
#include <sys/stat.h>

#include <cstdlib>
#include <deque>
#include <future>
#include <string>
#include <vector>

#include "../csrc/asm_host.h"

using namespace asm_host;

static int g_fail = 0;
#define EXPECT(cond, ...)                                      \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                      \
            fprintf(stderr, "\n");                             \
            g_fail++;                                          \
        }                                                      \
    } while (0)

static std::string make_text(const asm_gen_config& cfg, int64_t first, int64_t n, int64_t* pairs_out) {
    std::string err;
    std::vector<uint32_t> ro((size_t)n + 1), fo((size_t)n + 1);
    int rc = generate_pairs(&cfg, first, n, ro.data(), fo.data(), nullptr, 0, nullptr, 0, err);
    EXPECT(rc == ASM_OK, "sizing pass: %s", err.c_str());
    std::vector<char> reads(ro.back() + 1), refs(fo.back() + 1);
    rc = generate_pairs(&cfg, first, n, ro.data(), fo.data(), reads.data(), reads.size(), refs.data(), refs.size(), err);
    EXPECT(rc == ASM_OK, "fill pass: %s", err.c_str());
    std::string text;
    for (int64_t i = 0; i < n; i++) {
        text += '>';
        text.append(reads.data() + ro[(size_t)i], ro[(size_t)i + 1] - ro[(size_t)i]);
        text += "\n<";
        text.append(refs.data() + fo[(size_t)i], fo[(size_t)i + 1] - fo[(size_t)i]);
        text += '\n';
    }
    *pairs_out = n;
    return text;
}

/* Streams `text` (written to `path`) through ChunkReader<PairsFill>; returns what the consumer received, concatenated. */
static std::string stream_file(const std::string& path, const std::string& text, size_t chunk, int readers, int64_t max_pairs,
                               int64_t* pairs_seen, int* chunks_seen, bool* failed, size_t slack = (size_t)4 << 10, size_t first_chunk = 0) {
    FILE* f = fopen(path.c_str(), "wb");
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
    const int fd = open(path.c_str(), O_RDONLY);
    const size_t cap = chunk + slack;
    std::vector<std::vector<char>> bufs(3, std::vector<char>(cap + 64));
    std::future<void> copy[3]; /* the "copy stream": an asynchronous reader of the slot's buffer */
    ChunkReader<PairsFill> rd(chunk, first_chunk, [&](int q) {
        if (copy[q].valid()) copy[q].wait();
    }, fd, text.size(), readers, max_pairs);
    for (int q = 0; q < 3; q++) rd.slot[q].buf = bufs[(size_t)q].data(), rd.slot[q].cap = cap;
    rd.start();
    std::deque<std::string> parts; /* a deque: elements stay where they are while asynchronous copies write into them */
    *pairs_seen = 0, *chunks_seen = 0, *failed = false;
    bool last = false;
    for (int c = 0; !last; c++) {
        ChunkSlot* s = rd.wait_ready(c);
        if (!s) {
            *failed = true;
            break;
        }
        last = s->last;
        parts.emplace_back();
        std::string* dst = &parts.back();
        const char* src = s->buf;
        const size_t bytes = s->bytes;
        *pairs_seen += s->units, *chunks_seen += 1;
        /* the slot's previous copy (three chunks ago) was awaited by the reader before it refilled the buffer */
        copy[c % 3] = std::async(std::launch::async, [dst, src, bytes] { dst->assign(src, bytes); });
        rd.consumed(c, true);
        if (c % 2) std::this_thread::yield();
    }
    for (auto& fu : copy)
        if (fu.valid()) fu.wait();
    rd.stop();
    close(fd);
    std::string out;
    for (const std::string& p : parts) out += p;
    return out;
}

static std::string first_pairs(const std::string& text, int64_t pairs) { /* the text of the first `pairs` pairs */
    size_t pos = 0;
    for (int64_t l = 0; l < 2 * pairs; l++) {
        const size_t nl = text.find('\n', pos);
        if (nl == std::string::npos) return text;
        pos = nl + 1;
    }
    return text.substr(0, pos);
}

static void write_file(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

/* n four-line records; lengths vary, record `big` (if any) has a sequence of big_len bases */
static std::string make_fastq(int n, const char* eol = "\n", int big = -1, int big_len = 0) {
    std::string text;
    for (int i = 0; i < n; i++) {
        const size_t len = i == big ? (size_t)big_len : (size_t)(30 + (i * 37) % 120);
        text += "@read" + std::to_string(i) + eol + std::string(len, "ACGT"[i & 3]) + eol + "+" + eol + std::string(len, (char)('!' + i % 40)) + eol;
    }
    return text;
}

/* the plain line splitter the FASTQ reader is compared with: whole records of four lines, and the lines behind the last one */
static std::string fastq_whole_records(const std::string& text, int64_t* records, int64_t* extra_lines) {
    std::vector<size_t> ends; /* one past every line (a last line without its newline gets one) */
    for (size_t pos = 0; pos < text.size();) {
        const size_t nl = text.find('\n', pos);
        pos = nl == std::string::npos ? text.size() : nl + 1;
        ends.push_back(pos);
    }
    *records = (int64_t)ends.size() / 4, *extra_lines = (int64_t)ends.size() % 4;
    std::string out = text.substr(0, *records ? ends[(size_t)(4 * *records) - 1] : 0);
    if (*records && *extra_lines == 0 && text.back() != '\n') out += '\n';
    return out;
}

struct FastqRun {
    std::string bytes;
    int64_t records = 0, extra_lines = 0;
    int chunks = 0, grown = 0;
    bool failed = false, extra_before_last = false;
};

/* Streams `text` through ChunkReader<FastqFill>, slots of chunk + slack bytes that grow on demand (unless !may_grow); stop_at >= 0:
 * takes that many chunks, lets the reader fill every slot, and stops it */
static FastqRun stream_fastq(const std::string& path, const std::string& text, size_t chunk, size_t first_chunk, size_t slack,
                             bool may_grow = true, int stop_at = -1) {
    write_file(path, text);
    const int fd = open(path.c_str(), O_RDONLY);
    FastqRun r;
    std::vector<std::vector<char>> bufs(3, std::vector<char>(chunk + slack + 64));
    std::future<void> copy[3];
    ChunkReader<FastqFill> rd(
        chunk, first_chunk,
        [&](int q) {
            if (copy[q].valid()) copy[q].wait();
        },
        fd, text.size(), chunk,
        [&](int q, size_t cap, size_t keep) { /* the reader has waited for the slot's copy before it fills it */
            if (!may_grow) return false;
            std::vector<char> bigger(cap + 64);
            if (keep) memcpy(bigger.data(), bufs[(size_t)q].data(), keep);
            bufs[(size_t)q].swap(bigger);
            rd.slot[q].buf = bufs[(size_t)q].data(), rd.slot[q].cap = cap;
            r.grown++;
            return true;
        });
    for (int q = 0; q < 3; q++) rd.slot[q].buf = bufs[(size_t)q].data(), rd.slot[q].cap = chunk + slack;
    rd.start();
    std::deque<std::string> parts;
    bool last = false;
    for (int c = 0; !last && c != stop_at; c++) {
        ChunkSlot* s = rd.wait_ready(c);
        if (!s) {
            r.failed = true;
            break;
        }
        last = s->last;
        if (!last && s->extra_lines) r.extra_before_last = true;
        r.records += s->units, r.extra_lines += s->extra_lines, r.chunks++;
        parts.emplace_back();
        std::string* dst = &parts.back();
        const char* src = s->buf;
        const size_t bytes = s->bytes;
        copy[c % 3] = std::async(std::launch::async, [dst, src, bytes] { dst->assign(src, bytes); });
        rd.consumed(c, true);
        if (c % 2) std::this_thread::yield();
    }
    if (stop_at >= 0) std::this_thread::sleep_for(std::chrono::milliseconds(20)); /* the reader fills what is free and blocks */
    rd.stop();
    for (auto& fu : copy)
        if (fu.valid()) fu.wait();
    close(fd);
    for (const std::string& p : parts) r.bytes += p;
    return r;
}

static void expect_fastq(const char* what, const FastqRun& r, const std::string& text) {
    int64_t records = 0, extra = 0;
    const std::string want = fastq_whole_records(text, &records, &extra);
    EXPECT(!r.failed, "%s: stream failed", what);
    EXPECT(r.records == records && r.extra_lines == extra && !r.extra_before_last, "%s: %lld records + %lld lines, want %lld + %lld", what,
           (long long)r.records, (long long)r.extra_lines, (long long)records, (long long)extra);
    EXPECT(r.bytes == want, "%s: bytes differ (%zu against %zu)", what, r.bytes.size(), want.size());
}

static void check_fastq_reader(const std::string& path) {
    const std::string text = make_fastq(3000);
    FastqRun flat, ramp;
    for (size_t chunk : {(size_t)600, (size_t)4096, (size_t)65536, (size_t)1 << 20}) {
        flat = stream_fastq(path, text, chunk, 0, chunk / 4 + 4096);
        expect_fastq("flat chunks", flat, text);
        ramp = stream_fastq(path, text, chunk, chunk / 8, chunk / 4 + 4096);
        expect_fastq("ramped chunks", ramp, text);
        EXPECT(chunk >= text.size() || ramp.chunks > flat.chunks, "chunk %zu: ramp %d chunks against %d", chunk, ramp.chunks, flat.chunks);
    }
    expect_fastq("CRLF", stream_fastq(path, make_fastq(500, "\r\n"), 5000, 0, 4096), make_fastq(500, "\r\n"));
    expect_fastq("missing final newline", stream_fastq(path, text.substr(0, text.size() - 1), 30000, 0, 4096), text.substr(0, text.size() - 1));
    for (int extra = 1; extra <= 3; extra++) { /* a truncated last record: its first `extra` lines are there */
        std::string cut = make_fastq(200);
        const std::string more = make_fastq(1);
        size_t pos = 0;
        for (int l = 0; l < extra; l++) pos = more.find('\n', pos) + 1;
        cut += more.substr(0, pos);
        const FastqRun r = stream_fastq(path, cut, 3000, 0, 4096);
        expect_fastq("truncated record", r, cut);
        EXPECT(r.extra_lines == extra, "truncated record: %lld extra lines, want %d", (long long)r.extra_lines, extra);
    }
    {   /* a record longer than the chunk and the slot: the chunk takes more bytes and the slot grows; a grow that refuses fails */
        const std::string big = make_fastq(40, "\n", 17, 20000);
        FastqRun r = stream_fastq(path, big, 1024, 0, 64);
        expect_fastq("long record", r, big);
        EXPECT(r.grown > 0, "long record: the slot did not grow");
        r = stream_fastq(path, big, 1024, 0, 64, false);
        EXPECT(r.failed, "a grow that refuses must fail the stream");
    }
    {   /* an empty file is one last, empty chunk */
        const FastqRun r = stream_fastq(path, "", 4096, 0, 4096);
        EXPECT(!r.failed && r.chunks == 1 && r.records == 0 && r.extra_lines == 0 && r.bytes.empty(), "empty file: %d chunks", r.chunks);
    }
    {   /* stop() while every slot is full and the reader waits for one */
        const FastqRun r = stream_fastq(path, text, 2000, 0, 4096, true, 2);
        EXPECT(!r.failed && r.chunks == 2 && r.bytes == text.substr(0, r.bytes.size()), "early stop: %d chunks", r.chunks);
    }
}

struct PairChunk {
    std::string bytes;
    size_t bytes1 = 0;
    int64_t units = 0;
};
struct PairRun {
    std::deque<PairChunk> chunks;
    bool failed = false;
    int grown = 0;
    size_t carry_peak = 0;
    int64_t records[2] = {0, 0}, extra_lines[2] = {0, 0};
    bool more[2] = {false, false};
};

/* Streams the two files through ChunkReader<FastqPairFill>, slots of chunk + slack bytes that grow on demand */
static PairRun stream_fastq_pairs(const std::string& path1, const std::string& path2, size_t chunk, size_t first_chunk, size_t slack) {
    PairRun r;
    const int fd1 = open(path1.c_str(), O_RDONLY), fd2 = open(path2.c_str(), O_RDONLY);
    struct stat st1, st2;
    if (fd1 < 0 || fd2 < 0 || fstat(fd1, &st1) != 0 || fstat(fd2, &st2) != 0) {
        r.failed = true;
        return r;
    }
    std::vector<std::vector<char>> bufs(3, std::vector<char>(chunk + slack + 64));
    std::future<void> copy[3];
    ChunkReader<FastqPairFill> rd(
        chunk, first_chunk,
        [&](int q) {
            if (copy[q].valid()) copy[q].wait();
        },
        fd1, fd2, (size_t)st1.st_size, (size_t)st2.st_size, chunk,
        [&](int q, size_t cap, size_t keep) {
            std::vector<char> bigger(cap + 64);
            if (keep) memcpy(bigger.data(), bufs[(size_t)q].data(), keep);
            bufs[(size_t)q].swap(bigger);
            rd.slot[q].buf = bufs[(size_t)q].data(), rd.slot[q].cap = cap;
            r.grown++;
            return true;
        });
    for (int q = 0; q < 3; q++) rd.slot[q].buf = bufs[(size_t)q].data(), rd.slot[q].cap = chunk + slack;
    rd.start();
    bool last = false;
    for (int c = 0; !last; c++) {
        ChunkSlot* s = rd.wait_ready(c);
        if (!s) {
            r.failed = true;
            break;
        }
        last = s->last;
        r.chunks.emplace_back();
        PairChunk* dst = &r.chunks.back();
        dst->bytes1 = s->bytes1, dst->units = s->units;
        const char* src = s->buf;
        const size_t bytes = s->bytes;
        copy[c % 3] = std::async(std::launch::async, [dst, src, bytes] { dst->bytes.assign(src, bytes); });
        rd.consumed(c, true);
        if (c % 2) std::this_thread::yield();
    }
    rd.stop();
    for (auto& fu : copy)
        if (fu.valid()) fu.wait();
    const FastqPairFill& pol = rd.policy();
    r.carry_peak = pol.carry_peak;
    for (int f = 0; f < 2; f++) r.records[f] = pol.records[f], r.extra_lines[f] = pol.extra_lines[f], r.more[f] = pol.more[f];
    close(fd1), close(fd2);
    return r;
}

/* `asm_host_check --pairs f1 f2 chunk out` (tests/test_map_pairs_file_host.py): every chunk as u64 units, bytes1, bytes and the
 * bytes, then u64 0xffffffffffffffff, failed, carry_peak, records[2], extra_lines[2], more[2] */
static int dump_fastq_pairs(const char* f1, const char* f2, size_t chunk, const char* out_path) {
    const PairRun r = stream_fastq_pairs(f1, f2, chunk, chunk >= 8192 ? chunk / 8 : 0, chunk / 4 + 4096);
    FILE* out = fopen(out_path, "wb");
    if (!out) return 2;
    auto put = [&](uint64_t v) { fwrite(&v, 8, 1, out); };
    for (const PairChunk& c : r.chunks) {
        put((uint64_t)c.units), put(c.bytes1), put(c.bytes.size());
        fwrite(c.bytes.data(), 1, c.bytes.size(), out);
    }
    put(~0ull), put(r.failed), put(r.carry_peak);
    for (int f = 0; f < 2; f++) put((uint64_t)r.records[f]);
    for (int f = 0; f < 2; f++) put((uint64_t)r.extra_lines[f]);
    for (int f = 0; f < 2; f++) put(r.more[f]);
    return fclose(out) == 0 ? 0 : 2;
}

/* the first n records of a FASTQ text */
static std::string first_records(const std::string& text, int64_t n) {
    size_t pos = 0;
    for (int64_t l = 0; l < 4 * n; l++) pos = text.find('\n', pos) + 1;
    return text.substr(0, pos);
}

static void expect_pairs(const char* what, const PairRun& r, const std::string& t1, const std::string& t2, int64_t pairs, size_t chunk) {
    EXPECT(!r.failed, "%s: stream failed", what);
    std::string got[2];
    int64_t units = 0;
    for (const PairChunk& c : r.chunks) {
        int64_t n1 = 0, n2 = 0, l1 = 0, l2 = 0;
        const size_t b1 = fastq_cut(c.bytes.data(), c.bytes1, &n1, &l1);
        const size_t b2 = fastq_cut(c.bytes.data() + c.bytes1, c.bytes.size() - c.bytes1, &n2, &l2);
        EXPECT(c.bytes1 <= c.bytes.size() && b1 == c.bytes1 && b2 == c.bytes.size() - c.bytes1 && n1 == c.units && n2 == c.units && l1 == 4 * n1 &&
                   l2 == 4 * n2,
               "%s: a chunk of %lld units holds %lld and %lld records", what, (long long)c.units, (long long)n1, (long long)n2);
        got[0].append(c.bytes, 0, c.bytes1), got[1].append(c.bytes, c.bytes1, std::string::npos);
        units += c.units;
    }
    EXPECT(units == pairs, "%s: %lld pairs, want %lld", what, (long long)units, (long long)pairs);
    const std::string w1 = first_records(t1, pairs), w2 = first_records(t2, pairs);
    EXPECT(got[0] == w1 && got[1] == w2, "%s: bytes differ (%zu, %zu against %zu, %zu)", what, got[0].size(), got[1].size(), w1.size(), w2.size());
    EXPECT(chunk == 0 || r.carry_peak <= chunk, "%s: carry peak %zu above the chunk %zu", what, r.carry_peak, chunk);
}

static std::string make_mates(int n, int len_lo, int len_step, int len_mod, const char* eol = "\n") {
    std::string text;
    for (int i = 0; i < n; i++) {
        const size_t len = (size_t)(len_lo + (i * len_step) % len_mod);
        text += "@frag" + std::to_string(i) + eol + std::string(len, "ACGT"[i & 3]) + eol + "+" + eol + std::string(len, (char)('!' + i % 40)) + eol;
    }
    return text;
}

static void check_fastq_pair_reader(const std::string& dir) {
    const std::string p1 = dir + "/asm_host_check.r1.fq", p2 = dir + "/asm_host_check.r2.fq";
    const std::string t1 = make_mates(2000, 30, 7, 31), t2 = make_mates(2000, 200, 13, 101);
    write_file(p1, t1), write_file(p2, t2);
    for (size_t chunk : {(size_t)4096, (size_t)65536, (size_t)1 << 20}) {
        expect_pairs("flat chunks", stream_fastq_pairs(p1, p2, chunk, 0, chunk / 4 + 4096), t1, t2, 2000, chunk);
        const PairRun ramp = stream_fastq_pairs(p1, p2, chunk, chunk / 8, chunk / 4 + 4096);
        expect_pairs("ramped chunks", ramp, t1, t2, 2000, chunk);
        EXPECT(ramp.records[0] == 2000 && ramp.records[1] == 2000 && !ramp.more[0] && !ramp.more[1] && !ramp.extra_lines[0] && !ramp.extra_lines[1],
               "ramped chunks: the end of the stream");
    }
    {   /* CRLF in one file, no final newline in the other */
        const std::string c1 = make_mates(300, 40, 1, 1, "\r\n"), c2 = t2.substr(0, first_records(t2, 300).size() - 1);
        write_file(p1, c1), write_file(p2, c2);
        expect_pairs("CRLF and a missing final newline", stream_fastq_pairs(p1, p2, 5000, 0, 4096), c1, c2 + "\n", 300, 5000);
    }
    {   /* records longer than chunk and slot: more bytes are taken and the slot grows */
        const std::string b1 = make_fastq(40, "\n", 17, 20000), b2 = make_fastq(40, "\n", 3, 9000);
        write_file(p1, b1), write_file(p2, b2);
        const PairRun r = stream_fastq_pairs(p1, p2, 1024, 0, 64);
        expect_pairs("long records", r, b1, b2, 40, 0);
        EXPECT(r.grown > 0, "long records: the slot did not grow");
    }
    {   /* two empty files: one last, empty chunk */
        write_file(p1, ""), write_file(p2, "");
        const PairRun r = stream_fastq_pairs(p1, p2, 4096, 0, 4096);
        EXPECT(!r.failed && r.chunks.size() == 1 && r.chunks[0].units == 0 && r.chunks[0].bytes.empty() && !r.more[0] && !r.more[1], "two empty files");
    }
    for (int longer = 0; longer < 2; longer++) { /* one file holds more records: the pairs come through, then more[] says which */
        const std::string a = first_records(t1, 700 + 300 * (longer == 0)), b = first_records(t2, 700 + 300 * (longer == 1));
        write_file(p1, a), write_file(p2, b);
        const PairRun r = stream_fastq_pairs(p1, p2, 8192, 0, 4096);
        expect_pairs("a longer file", r, a, b, 700, 0);
        EXPECT(r.more[longer] && !r.more[1 - longer] && r.records[1 - longer] == 700 && r.records[longer] > 700 && !r.extra_lines[0] && !r.extra_lines[1],
               "a longer file: more %d %d", (int)r.more[0], (int)r.more[1]);
    }
    for (int f = 0; f < 2; f++)
        for (int extra = 1; extra <= 3; extra++) { /* a truncated last record in file f */
            std::string a = first_records(t1, 200), b = first_records(t2, 200);
            std::string& cut = f ? b : a;
            size_t pos = cut.size();
            for (int l = 0; l < 4 - extra; l++) pos = cut.rfind('\n', pos - 2) + 1;
            cut.resize(pos);
            write_file(p1, a), write_file(p2, b);
            const PairRun r = stream_fastq_pairs(p1, p2, 3000, 0, 4096);
            expect_pairs("a truncated record", r, a, b, 199, 0);
            EXPECT(r.extra_lines[f] == extra && r.extra_lines[1 - f] == 0 && r.records[f] == 199 && r.records[1 - f] == 200,
                   "a truncated record in file %d: %lld extra lines, want %d", f + 1, (long long)r.extra_lines[f], extra);
        }
    remove(p1.c_str()), remove(p2.c_str());
}

static void check_chunk_writer(const std::string& path) {
    {   /* bytes arrive in push order through three rotating slots, whatever `before` takes; wait_idle waits for the job */
        FILE* f = fopen(path.c_str(), "wb");
        std::atomic<int> befores{0};
        std::string bufs[3], want;
        {
            ChunkWriter w(f, [&](int o) {
                std::this_thread::sleep_for(std::chrono::milliseconds(o + 1));
                befores++;
                return true;
            });
            for (int i = 0; i < 40; i++) {
                const int o = i % 3;
                w.wait_idle(o); /* the job that used the buffer three jobs ago is written */
                EXPECT(befores >= i - 2, "wait_idle returned before job %d was written", i - 3);
                bufs[o] = "chunk " + std::to_string(i) + std::string((size_t)(i * 97 % 5000), (char)('a' + i % 26)) + "\n";
                want += bufs[o];
                w.push(o, bufs[o].data(), i == 7 ? 0 : bufs[o].size()); /* an empty job still goes through before() */
                if (i == 7) want.resize(want.size() - bufs[o].size());
            }
            w.wait_idle(0), w.wait_idle(1), w.wait_idle(2);
            EXPECT(befores == 40 && !w.failed(), "writer: %d jobs went through", befores.load());
            EXPECT(w.finish(), "writer: finish");
        }
        fclose(f);
        std::string got;
        f = fopen(path.c_str(), "rb");
        char block[4096];
        for (size_t k; (k = fread(block, 1, sizeof block, f)) > 0;) got.append(block, k);
        fclose(f);
        EXPECT(got == want, "writer: file differs (%zu bytes against %zu)", got.size(), want.size());
    }
    {   /* a failing before(): the job is dropped, the slot is given back, finish() says so */
        FILE* f = fopen(path.c_str(), "wb");
        ChunkWriter w(f, [](int o) { return o != 1; });
        const std::string text = "some bytes\n";
        for (int o = 0; o < 3; o++) w.push(o, text.data(), text.size());
        for (int o = 0; o < 3; o++) w.wait_idle(o);
        EXPECT(w.failed(), "writer: a failing before() went unnoticed");
        EXPECT(!w.finish(), "writer: finish() after a failing before()");
        fclose(f);
    }
    {   /* a file whose writes fail (unbuffered, so that fwrite itself reports it) */
        FILE* f = fopen("/dev/full", "wb");
        if (!f) f = fopen(path.c_str(), "rb"); /* no such device here: a stream that is not open for writing */
        setvbuf(f, nullptr, _IONBF, 0);
        ChunkWriter w(f, [](int) { return true; });
        const std::string text(10000, 'x');
        for (int i = 0; i < 5; i++) {
            w.wait_idle(i % 3);
            w.push(i % 3, text.data(), text.size());
        }
        EXPECT(!w.finish() && w.failed(), "writer: failing writes went unnoticed");
        fclose(f);
    }
}

int main(int argc, char** argv) {
    if (argc == 6 && std::string(argv[1]) == "--pairs") return dump_fastq_pairs(argv[2], argv[3], (size_t)atoll(argv[4]), argv[5]);
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    const std::string path = dir + "/asm_host_check.seq";
    asm_gen_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.seed = 7, cfg.kind = ASM_GEN_EXACT_ERRORS, cfg.len_lo = 64, cfg.len_hi = 300, cfg.err = 0.10f, cfg.mismatch_rate = 0.96f;
    int64_t n = 0;
    const std::string text = make_text(cfg, 123, 6000, &n);
    {   /* the same pairs whichever slice of the stream asks for them */
        int64_t n2 = 0;
        const std::string tail = make_text(cfg, 123 + 5000, 1000, &n2);
        EXPECT(text.size() > tail.size() && text.compare(text.size() - tail.size(), tail.size(), tail) == 0, "generator: slices disagree");
        std::string err;
        asm_gen_config bad = cfg;
        bad.err = 0.9f;
        uint32_t off[2];
        EXPECT(generate_pairs(&bad, 0, 1, off, off, nullptr, 0, nullptr, 0, err) == ASM_EINVAL, "generator accepted err 0.9");
    }
    EXPECT(scan_newlines(text.data(), text.size(), 5).count == 2 * n, "scan_newlines count");

    struct Case {
        size_t chunk;
        int readers;
        int64_t max_pairs;
    };
    const Case cases[] = {{4096, 1, 0}, {4096, 4, 0}, {65536, 3, 0}, {1 << 20, 8, 0}, {8192, 2, 777}, {4 << 20, 4, 0}, {50000, 5, 5999}};
    for (const Case& c : cases) {
        int64_t pairs = 0;
        int chunks = 0;
        bool failed = false;
        const std::string got = stream_file(path, text, c.chunk, c.readers, c.max_pairs, &pairs, &chunks, &failed);
        const int64_t want_pairs = c.max_pairs > 0 && c.max_pairs < n ? c.max_pairs : n;
        EXPECT(!failed, "stream failed (chunk %zu)", c.chunk);
        EXPECT(pairs == want_pairs, "chunk %zu readers %d: %lld pairs, want %lld", c.chunk, c.readers, (long long)pairs, (long long)want_pairs);
        EXPECT(got == first_pairs(text, want_pairs), "chunk %zu readers %d: bytes differ (%zu against %zu)", c.chunk, c.readers, got.size(),
               first_pairs(text, want_pairs).size());
    }
    {   /* chunks that ramp up from a small first one: the same bytes, more chunks than the full size alone would give */
        int64_t pairs = 0;
        int chunks_flat = 0, chunks_ramp = 0;
        bool failed = false;
        std::string got = stream_file(path, text, 1 << 19, 3, 0, &pairs, &chunks_flat, &failed);
        EXPECT(!failed && pairs == n && got == text, "flat 512 KB chunks");
        got = stream_file(path, text, 1 << 19, 3, 0, &pairs, &chunks_ramp, &failed, (size_t)4 << 10, 1 << 15);
        EXPECT(!failed && pairs == n && got == text, "ramped chunks: %lld pairs", (long long)pairs);
        EXPECT(chunks_ramp > chunks_flat, "ramp: %d chunks against %d", chunks_ramp, chunks_flat);
        got = stream_file(path, text, 1 << 19, 2, 4321, &pairs, &chunks_ramp, &failed, (size_t)4 << 10, 600); /* a first chunk of barely a pair */
        EXPECT(!failed && pairs == 4321 && got == first_pairs(text, 4321), "ramp from 600 bytes: %lld pairs", (long long)pairs);
    }
    {   /* a last line without its newline; a file that ends on a read line (the reference gets an empty string there) */
        int64_t pairs = 0;
        int chunks = 0;
        bool failed = false;
        std::string open_end = text.substr(0, text.size() - 1);
        std::string got = stream_file(path, open_end, 30000, 3, 0, &pairs, &chunks, &failed);
        EXPECT(!failed && pairs == n && got == text, "missing final newline: %lld pairs", (long long)pairs);
        std::string odd = text + ">ACGT\n";
        got = stream_file(path, odd, 30000, 3, 0, &pairs, &chunks, &failed);
        EXPECT(!failed && pairs == n + 1 && got == odd + "\n", "odd line count: %lld pairs", (long long)pairs);
        /* a pair longer than a whole slot is refused, not cut */
        got = stream_file(path, text, 256, 2, 0, &pairs, &chunks, &failed, 16);
        EXPECT(failed, "a chunk smaller than one pair must fail");
    }
    check_fastq_reader(path);
    check_fastq_pair_reader(dir);
    check_chunk_writer(path);
    {   /* stale-tail state: advancing over a + b untouched pairs = advancing over a, then b; a write lands where its slot goes */
        std::string err;
        uint8_t none[256], st1[256], st2[256];
        memset(none, TAIL_NONE, sizeof none);
        for (int q = 0; q < 256; q++) st1[q] = st2[q] = (uint8_t)(q & 3);
        EXPECT(tail_state_advance(st1, none, 7, err) == ASM_OK && tail_state_advance(st1, none, 14, err) == ASM_OK, "advance");
        EXPECT(tail_state_advance(st2, none, 21, err) == ASM_OK, "advance");
        EXPECT(memcmp(st1, st2, 256) == 0, "tail_state_advance is not additive over untouched pairs");
        for (int s = 0; s < 128; s++) EXPECT(tail_slot_after(tail_slot_after(s, 3), 7) == s, "SRC does not have order 10 at slot %d", s);
        uint8_t sum[256];
        memset(sum, TAIL_NONE, sizeof sum);
        sum[5] = 2, sum[128 + 127] = 1;
        EXPECT(tail_state_advance(st2, sum, 1, err) == ASM_OK, "advance with writes");
        EXPECT(st2[tail_slot_after(5, 1)] == 2 && st2[128 + tail_slot_after(127, 1)] == 1, "a written code did not land on its trajectory");
        sum[9] = 17;
        EXPECT(tail_state_advance(st2, sum, 1, err) == ASM_EINVAL, "summary entry 17 accepted");
        EXPECT(tail_state_advance(nullptr, sum, 1, err) == ASM_EINVAL, "NULL state accepted");
    }
    {   /* the resolver's bit-plane step (tail_permute, tail_prefix: what csrc/asm_tails.h runs per pair) against the byte buffer
           it stands for: copy the first L codes in, then after[q] = before[8 * (q & 15) + P[q >> 4]] (bit_convert.cpp:265-330) */
        static const int P[8] = {0, 2, 1, 3, 4, 6, 5, 7};
        uint8_t buf[128] = {0};
        TailBits s0{}, s1{};
        uint64_t rng = 88172645463325252ull;
        auto next = [&rng] { return rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17, (uint32_t)(rng >> 11); };
        int bad = 0;
        for (int t = 0; t < 2000 && !bad; t++) {
            const uint32_t L = t % 7 == 0 ? (t % 14 ? 128u : 0u) : next() % 129u;
            TailBits a0{}, a1{};
            for (uint32_t q = 0; q < L; q++) {
                const uint8_t code = (uint8_t)(next() & 3u);
                buf[q] = code;
                a0.w[q >> 5] |= (uint32_t)(code & 1u) << (q & 31), a1.w[q >> 5] |= (uint32_t)(code >> 1) << (q & 31);
            }
            const TailBits m = tail_prefix(L);
            for (uint32_t q = 0; q < 128; q++) { /* what the conversion sees: the string, then the stale codes */
                const uint32_t want = buf[q], bit = 1u << (q & 31);
                const uint32_t t0 = q < L ? a0.w[q >> 5] : (s0.w[q >> 5] & ~m.w[q >> 5]), t1 = q < L ? a1.w[q >> 5] : (s1.w[q >> 5] & ~m.w[q >> 5]);
                if ((((t0 & bit) ? 1u : 0u) | ((t1 & bit) ? 2u : 0u)) != want) bad++;
            }
            uint8_t after[128];
            for (int q = 0; q < 128; q++) after[q] = buf[8 * (q & 15) + P[q >> 4]];
            memcpy(buf, after, 128);
            TailBits n0{}, n1{};
            for (int d = 0; d < 4; d++) n0.w[d] = tail_bfi(m.w[d], a0.w[d], s0.w[d]), n1.w[d] = tail_bfi(m.w[d], a1.w[d], s1.w[d]);
            s0 = tail_permute(n0), s1 = tail_permute(n1);
        }
        EXPECT(bad == 0, "bit-plane buffer step differs from the byte buffer");
        TailBits x{{0x12345678u, 0x9abcdef0u, 0x0fedcba9u, 0x87654321u}}, y = x;
        for (int r = 0; r < 10; r++) y = tail_permute(y);
        EXPECT(memcmp(&x, &y, sizeof x) == 0, "tail_permute does not have order 10");
    }
    {   /* CIGAR rows: formatting, truncated rows, output buffers of every size down to one byte */
        const uint16_t ops[5] = {(uint16_t)(22 << 3 | 0), (uint16_t)(1 << 3 | 2), (uint16_t)(50 << 3 | 0), (uint16_t)(1 << 3 | 1), (uint16_t)(128 << 3 | 4)};
        char out[64];
        EXPECT(cigar_format(ops, 5, 8, out, sizeof out) == ASM_OK && std::string(out) == "22M1D50M1I128X", "cigar text: %s", out);
        EXPECT(cigar_format(ops, 9, 5, out, sizeof out) == ASM_EUNSUPPORTED && std::string(out) == "22M1D50M1I128X", "truncated row");
        EXPECT(cigar_format(ops, 0, 5, out, sizeof out) == ASM_OK && out[0] == 0, "empty row");
        {   /* the count saturates: 255 is "255 or more" at any cap, 254 is a whole row where the cap holds it */
            std::vector<uint16_t> wide(300, (uint16_t)(1 << 3 | 3));
            std::vector<char> text(4096);
            EXPECT(cigar_format(wide.data(), 254, 254, text.data(), text.size()) == ASM_OK && strlen(text.data()) == 2 * 254, "254 of 254");
            for (int cap : {254, 255, 256, 300}) {
                const int rc = cigar_format(wide.data(), 255, cap, text.data(), text.size());
                EXPECT(rc == ASM_EUNSUPPORTED && strlen(text.data()) == 2 * (size_t)(cap < 255 ? cap : 255), "saturated count at cap %d: rc %d", cap, rc);
            }
        }
        for (size_t cap = 1; cap <= 15; cap++) {
            std::vector<char> small(cap); /* exactly `cap` bytes on the heap: an overrun is an ASan report */
            const int rc = cigar_format(ops, 5, 8, small.data(), cap);
            EXPECT(rc == (cap >= 15 ? ASM_OK : ASM_EINVAL), "out_cap %zu: rc %d", cap, rc);
        }
        EXPECT(cigar_format(nullptr, 1, 1, out, sizeof out) == ASM_EINVAL && cigar_format(ops, 1, 1, out, 0) == ASM_EINVAL, "bad arguments");
    }
    remove(path.c_str());
    if (g_fail) {
        fprintf(stderr, "%d host checks failed\n", g_fail);
        return 1;
    }
    printf("host check ok\n");
    return 0;
}
