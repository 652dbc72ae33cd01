// Host build of asm_map_pairs_file's fill policy for two BGZF files (csrc/asm_host.h: BgzfPairFill, device-free) and of the pair cut's
// rule (csrc/asm_pair_cut.h), for the CPU test-suite (tests/test_bgzf_pair_fill_host.py): plain g++, run under ASan + UBSan.
//
//   bgzf_pair_fill_host_check <file 1> <file 2> <want> <out>
// streams the two files through ChunkReader<BgzfPairFill>, every chunk asking for <want> text bytes, and plays the device's part of
// map_pairs_file_gz_chunk on the host: each region's members are inflated behind that file's carry by the decoder the kernel runs
// (bgzf_inflate_host), the newlines are counted, pair_cut_plan says how many pairs R the two texts hold and which newline ends them (a
// scan finds its byte, and asm_fastq_cut_n must find the same one), what lies behind the cuts are the next carries, and their lengths
// go back to the policy before the slot does.  <out> gets, per chunk, the u64s R, done1, done2, members1, members2, len1, len2 and the
// len1 + len2 bytes of the two regions' records; then the u64s ~0, status (0 sound, 1 reading failed, 2 a bad member or header),
// carry_peak, records[2], extra_lines[2], more[2] with FastqPairFill's meanings, the chunks with R = 0 in front of the end, and the
// largest text handed out in one chunk.  Exit status 5: the rule and asm_fastq_cut_n disagree, or the policy broke its own layout.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>

#include "../csrc/asm_inflate.h"
#include "../csrc/asm_host.h"
#include "../csrc/asm_pair_cut.h"

using namespace asm_host;

static size_t behind_newline(const char* text, size_t nbytes, unsigned long long k) { /* the byte behind newline k (from 0) */
    const char* q = text;
    for (unsigned long long l = 0; l <= k; l++) q = (const char*)memchr(q, '\n', (size_t)(text + nbytes - q)) + 1;
    return (size_t)(q - text);
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const int fd1 = open(argv[1], O_RDONLY), fd2 = open(argv[2], O_RDONLY);
    struct stat st1, st2;
    if (fd1 < 0 || fd2 < 0 || fstat(fd1, &st1) != 0 || fstat(fd2, &st2) != 0) return 2;
    const size_t want = (size_t)strtoull(argv[3], nullptr, 10);
    FILE* out = fopen(argv[4], "wb");
    if (!out || want == 0) return 2;
    auto put = [&](uint64_t v) { fwrite(&v, 8, 1, out); };

    const size_t cap0 = 4096;
    std::vector<std::vector<char>> bufs(3, std::vector<char>(cap0 + 64));
    ChunkReader<BgzfPairFill> rd(
        want, 0, [](int) {}, fd1, fd2, (size_t)st1.st_size, (size_t)st2.st_size, [&](int q, size_t cap, size_t keep) {
            std::vector<char> bigger(cap + 64);
            if (keep) memcpy(bigger.data(), bufs[(size_t)q].data(), keep);
            bufs[(size_t)q].swap(bigger);
            rd.slot[q].buf = bufs[(size_t)q].data(), rd.slot[q].cap = cap;
            return true;
        });
    for (int q = 0; q < 3; q++) rd.slot[q].buf = bufs[(size_t)q].data(), rd.slot[q].cap = cap0;
    BgzfPairFill& fill = rd.policy();
    rd.start();

    std::vector<char> text[2]; /* each file's carry, then its chunk's text, then room for the appended newline */
    size_t carry_len[2] = {0, 0}, carry_peak = 0, text_peak = 0;
    int64_t pairs_seen = 0, records[2] = {0, 0}, extra_lines[2] = {0, 0}, empty_chunks = 0;
    bool more[2] = {false, false};
    int status = 0, rc = 0;
    bool last = false;
    for (int c = 0; !last && !status && !rc; c++) {
        ChunkSlot* s = rd.wait_ready(c);
        if (!s) {
            status = 1;
            break;
        }
        last = s->last;
        const BgzfPairChunkInfo& pi = fill.info[c % 3];
        const size_t nm[2] = {pi.f[0].members.size(), pi.f[1].members.size()};
        if (s->units != (int64_t)(nm[0] + nm[1]) + 1 || s->bytes1 > s->bytes) rc = 5;
        PairCutText t[2];
        for (int x = 0; x < 2 && !rc; x++) {
            const BgzfChunkInfo& ci = pi.f[x];
            for (const InfMember& m : ci.members) /* whole members of region x, inside the slot */
                if (m.src_off < (x ? s->bytes1 : 0) || m.src_off + m.csize > (x ? s->bytes : s->bytes1)) rc = 5;
            text[x].resize(carry_len[x] + ci.text + 1);
            if (!rc && bgzf_inflate_host((const uint8_t*)s->buf, ci.members, (uint8_t*)text[x].data() + carry_len[x]) != INF_NONE_BAD) status = 2;
            if (ci.err.status != BGZF_IN_OK) status = 2;
            const size_t nb = carry_len[x] + ci.text;
            int64_t lines = 0;
            fastq_cut(text[x].data(), nb, nullptr, &lines);
            t[x].counted = (unsigned long long)lines, t[x].nbytes = nb, t[x].pad = 0u;
            t[x].open_end = pi.done[x] && nb > 0 && text[x][nb - 1] != '\n' ? 1u : 0u;
        }
        if (pi.f[0].text + pi.f[1].text > text_peak) text_peak = pi.f[0].text + pi.f[1].text;
        if (rc || status) break;
        PairCutOut o;
        uint32_t how[2];
        pair_cut_plan(t, &o, how);
        size_t rest[2];
        bool end = pi.done[0] && pi.done[1];
        for (int x = 0; x < 2; x++) {
            if (o.f[x].appended) text[x][t[x].nbytes] = '\n';
            const size_t len = (size_t)t[x].nbytes + o.f[x].appended;
            if (how[x] == PAIR_CUT_FIND) o.f[x].cut = behind_newline(text[x].data(), (size_t)t[x].nbytes, 4u * o.pairs - 1u);
            int64_t n = 0;
            if (fastq_cut_n(text[x].data(), len, (int64_t)o.pairs, &n) != o.f[x].cut || n != (int64_t)o.pairs) rc = 5;
            rest[x] = len - (size_t)o.f[x].cut;
            if (pi.done[x] && !o.f[x].more && o.f[1 - x].more) end = true;
        }
        if (rc) break;
        put(o.pairs), put(pi.done[0]), put(pi.done[1]), put(nm[0]), put(nm[1]), put(o.f[0].cut), put(o.f[1].cut);
        for (int x = 0; x < 2; x++) fwrite(text[x].data(), 1, (size_t)o.f[x].cut, out);
        pairs_seen += (int64_t)o.pairs;
        fill.feedback(c, rest[0], rest[1], pairs_seen);
        if (!end) {
            if (rest[0] + rest[1] > carry_peak) carry_peak = rest[0] + rest[1];
            if (o.pairs == 0) empty_chunks++;
        }
        for (int x = 0; x < 2; x++) {
            memmove(text[x].data(), text[x].data() + o.f[x].cut, rest[x]);
            carry_len[x] = rest[x];
        }
        rd.consumed(c, false);
        if (end) {
            for (int x = 0; x < 2; x++)
                records[x] = pairs_seen - (int64_t)o.pairs + (int64_t)(o.f[x].lines / 4u), extra_lines[x] = pi.done[x] ? o.f[x].extra_lines : 0,
                more[x] = o.f[x].more != 0;
            if (!last && !more[0] && !more[1]) rc = 5; /* only a missing mate ends the call in front of the stream's end */
            break;
        }
        if (last) rc = 5; /* the stream's end is the files' */
    }
    rd.stop();
    put(~0ull), put((uint64_t)status), put(carry_peak);
    for (int x = 0; x < 2; x++) put((uint64_t)records[x]);
    for (int x = 0; x < 2; x++) put((uint64_t)extra_lines[x]);
    for (int x = 0; x < 2; x++) put(more[x]);
    put((uint64_t)empty_chunks), put(text_peak);
    close(fd1), close(fd2);
    if (fclose(out) != 0) return 2;
    return rc;
}
