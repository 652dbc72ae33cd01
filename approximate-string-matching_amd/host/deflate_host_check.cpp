// Host build of the BGZF container's deflate encoder (csrc/asm_deflate.h behind csrc/asm_bgzf.h), for the CPU test-suite
// (tests/test_deflate_host.py): plain g++, run under ASan + UBSan.
//
//   deflate_host_check <in> <out> <with_eof>
// writes the bytes of <in> to <out> as the container of ASM_BGZF_DEFLATE, with bgzf_compress_host (the per-position match, parse,
// count and emit code that bgzf_deflate_kernel's threads run, serially), and prints one line per block: the payload's length, the
// block's BTYPE and the block's bytes.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../csrc/asm_bgzf.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint8_t> src, framed;
    std::vector<uint32_t> types;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, in)) > 0;) src.insert(src.end(), buf, buf + got);
    fclose(in);
    const int with_eof = atoi(argv[3]);
    bgzf_compress_host(src.data(), src.size(), with_eof, 1, framed, &types);
    if (framed.size() > bgzf_bound(src.size(), with_eof) || types.size() != bgzf_blocks(src.size())) return 5;
    size_t at = 0;
    for (size_t b = 0; b < types.size(); b++) {
        const size_t done = b * (size_t)BGZF_PAYLOAD, len = src.size() - done < BGZF_PAYLOAD ? src.size() - done : BGZF_PAYLOAD;
        if (at + DFL_HEAD > framed.size()) return 5;
        const size_t block = (size_t)framed[at + 16] + 256u * framed[at + 17] + 1u;
        printf("%zu %u %zu\n", len, types[b], block);
        at += block;
    }
    if (at + (with_eof ? BGZF_EOF : 0u) != framed.size()) return 5;
    fwrite(framed.data(), 1, framed.size(), out);
    return fclose(out) == 0 ? 0 : 4;
}
