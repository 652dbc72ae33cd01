// Host build of the BAM index's core (csrc/asm_bai.h: the record-field reader, the virtual-offset rule, the layout arithmetic and the
// byte emitters that the index kernels compile, walked serially by bai_build_host), for the CPU test-suite (tests/test_bai_host.py):
// plain g++, run under ASan + UBSan.
//
//   bai_host_check <in.bam> <out.bai>
// walks and inflates the container with the host decoder (csrc/asm_inflate.h), builds the index of the coordinate-sorted BAM stream and
// writes it.  Prints `ok <refs> <bins> <chunks> <intervals> <no_coor> <bytes>` and exits 0; a corrupt container prints `container
// <status> <member> <offset>` or `member <index> <status>` and exits 3; a stream that cannot be indexed prints `refused <class> <text>`
// (class: BAI_E_MALFORMED 1, BAI_E_ORDER 2, BAI_E_COORD 3) and exits 4, and <out.bai> is not written.  The inflated stream lies in a
// buffer of exactly its size, so that a read behind it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_inflate.h"
#include "../csrc/asm_bai.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint8_t> src;
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, in)) > 0;) src.insert(src.end(), buf, buf + got);
    fclose(in);
    std::vector<InfMember> members;
    size_t total = 0;
    const BgzfWalkError err = bgzf_walk(src.data(), src.size(), &members, &total);
    if (err.status != BGZF_IN_OK) {
        printf("container %u %zu %zu\n", err.status, err.member, err.offset);
        return 3;
    }
    std::vector<uint8_t> stream(total);
    const unsigned long long bad = bgzf_inflate_host(src.data(), members, stream.data());
    if (bad != INF_NONE_BAD) {
        printf("member %llu %u\n", bad >> 8, (unsigned)(bad & 0xffu));
        return 3;
    }
    std::vector<uint8_t> img;
    const BaiHostResult r = bai_build_host(stream.data(), total, members, src.size(), img);
    if (r.status != BAI_OK) {
        printf("refused %d %s\n", r.status, r.what.c_str());
        return 4;
    }
    printf("ok %lld %lld %lld %lld %lld %zu\n", (long long)r.refs, (long long)r.bins, (long long)r.chunks, (long long)r.intervals,
           (long long)r.no_coor, img.size());
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (!img.empty()) fwrite(img.data(), 1, img.size(), out);
    return fclose(out) == 0 ? 0 : 5;
}
