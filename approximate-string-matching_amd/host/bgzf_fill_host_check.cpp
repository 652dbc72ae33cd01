// Host build of asm_map_file's BGZF fill policy (csrc/asm_host.h: BgzfFill, device-free), for the CPU test-suite
// (tests/test_inflate_host.py): plain g++, run under ASan + UBSan.
//
//   bgzf_fill_host_check <file> <want> [<slot bytes>]
// drives the policy as ChunkReader does, chunk after chunk with its carry, every chunk asking for <want> text bytes, in slots that
// start at <slot bytes> (default 4096) and grow through the policy's grow().  One line per chunk, `chunk <members> <text bytes>
// <compressed bytes> <carry bytes> <eof>`, one per member, `<index in the file> <file offset> <csize> <isize> <crc>`, and for a bad
// header `error <status> <member> <offset>`.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>

#include "../csrc/asm_host.h"

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 2;
    const int fd = open(argv[1], O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) return 2;
    const size_t want = (size_t)strtoull(argv[2], nullptr, 10), cap0 = argc == 4 ? (size_t)strtoull(argv[3], nullptr, 10) : 4096u;
    asm_host::ChunkSlot slot[3];
    std::vector<std::vector<char>> mem(3);
    for (int q = 0; q < 3; q++) mem[q].resize(cap0 + 64), slot[q].buf = mem[q].data(), slot[q].cap = cap0;
    asm_host::BgzfFill fill(fd, (size_t)st.st_size, [&](int q, size_t cap, size_t keep) {
        std::vector<char> bigger(cap + 64);
        if (keep) memcpy(bigger.data(), mem[q].data(), keep);
        mem[q].swap(bigger);
        slot[q].buf = mem[q].data(), slot[q].cap = cap;
        return true;
    });
    std::vector<char> carry;
    for (int c = 0;; c++) {
        asm_host::ChunkCut cut;
        const int q = c % 3;
        if (!fill(slot[q], q, carry, want, cut)) return 3;
        const asm_host::BgzfChunkInfo& ci = fill.info[q];
        if (cut.units != (int64_t)ci.members.size() || cut.boundary > cut.have || cut.have > slot[q].cap) return 5;
        if (!cut.eof && cut.have - cut.boundary > 65536u) return 5; /* the carry: a member cut by the chunk's end */
        printf("chunk %zu %zu %zu %zu %d\n", ci.members.size(), ci.text, cut.boundary, cut.eof ? (size_t)0 : cut.have - cut.boundary, (int)cut.eof);
        for (size_t k = 0; k < ci.members.size(); k++)
            printf("%lld %zu %u %u %u\n", (long long)ci.first_member + (long long)k, ci.file_base + (size_t)ci.members[k].src_off, ci.members[k].csize,
                   ci.members[k].isize, ci.members[k].crc);
        if (ci.err.status) printf("error %u %zu %zu\n", ci.err.status, ci.err.member, ci.err.offset);
        carry.clear();
        if (cut.eof) break;
        carry.assign(slot[q].buf + cut.boundary, slot[q].buf + cut.have);
    }
    close(fd);
    return 0;
}
