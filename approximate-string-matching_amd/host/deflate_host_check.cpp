// Host build of the BGZF container's deflate encoder (csrc/asm_deflate.h behind csrc/asm_bgzf.h), for the CPU test-suite
// (tests/test_deflate_host.py): plain g++, run under ASan + UBSan.
//
//   deflate_host_check <in> <out> <with_eof> [counts]
// writes the bytes of <in> to <out> as the container of ASM_BGZF_DEFLATE, with bgzf_compress_host (the per-position match, parse,
// count and emit code that bgzf_deflate_kernel's threads run, serially), and prints one line per block: the payload's length, the
// block's BTYPE and the block's bytes; with `counts` also the bits dfl_choose counted for the fixed-Huffman and for the dynamic
// form (a stored block shows neither in its bytes).
//
//   deflate_host_check lengths <limit> w0 w1 ...
//   deflate_host_check lengths @<file>          one case per line of <file>: <limit> w0 w1 ...
// prints dfl_lengths' code lengths of the weights w (0: an unused symbol) under `limit`, ranked by dfl_rank as the encoder ranks
// them; one line per case.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../csrc/asm_bgzf.h"

static int lengths_case(uint32_t limit, const std::vector<uint32_t>& w) {
    const uint32_t n = (uint32_t)w.size();
    if (limit < 1u || limit > 15u || n < 1u) return 2;
    std::vector<uint32_t> order(n), a(n), len(n);
    uint32_t used = 0u;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t r = dfl_rank(w.data(), n, i);
        if (r != DFL_NONE) order[r] = i, used++;
    }
    if (used > (1u << limit)) return 2; /* no code of that limit exists */
    dfl_lengths(w.data(), order.data(), used, limit, a.data(), len.data(), n);
    for (uint32_t i = 0; i < n; i++) printf(i + 1u < n ? "%u " : "%u\n", len[i]);
    return 0;
}

static int lengths_mode(int argc, char** argv) {
    if (argc == 3 && argv[2][0] == '@') {
        FILE* in = fopen(argv[2] + 1, "r");
        if (!in) return 2;
        std::string text;
        char buf[4096];
        for (size_t got; (got = fread(buf, 1, sizeof buf, in)) > 0;) text.append(buf, got);
        fclose(in);
        std::istringstream lines(text);
        for (std::string line; std::getline(lines, line);) {
            std::istringstream fields(line);
            uint32_t limit = 0u;
            std::vector<uint32_t> w;
            if (!(fields >> limit)) continue;
            for (uint32_t v; fields >> v;) w.push_back(v);
            if (const int rc = lengths_case(limit, w)) return rc;
        }
        return 0;
    }
    if (argc < 4) return 2;
    std::vector<uint32_t> w;
    for (int i = 3; i < argc; i++) w.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
    return lengths_case((uint32_t)atoi(argv[2]), w);
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "lengths") == 0) return lengths_mode(argc, argv);
    const bool with_counts = argc == 5 && strcmp(argv[4], "counts") == 0;
    if (argc != 4 && !with_counts) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint8_t> src, framed;
    std::vector<uint32_t> types, counts;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, in)) > 0;) src.insert(src.end(), buf, buf + got);
    fclose(in);
    const int with_eof = atoi(argv[3]);
    bgzf_compress_host(src.data(), src.size(), with_eof, 1, framed, &types, &counts);
    if (framed.size() > bgzf_bound(src.size(), with_eof) || types.size() != bgzf_blocks(src.size()) || counts.size() != 2u * types.size()) return 5;
    size_t at = 0;
    for (size_t b = 0; b < types.size(); b++) {
        const size_t done = b * (size_t)BGZF_PAYLOAD, len = src.size() - done < BGZF_PAYLOAD ? src.size() - done : BGZF_PAYLOAD;
        if (at + DFL_HEAD > framed.size()) return 5;
        const size_t block = (size_t)framed[at + 16] + 256u * framed[at + 17] + 1u;
        if (with_counts) printf("%zu %u %zu %u %u\n", len, types[b], block, counts[2 * b], counts[2 * b + 1]);
        else printf("%zu %u %zu\n", len, types[b], block);
        at += block;
    }
    if (at + (with_eof ? BGZF_EOF : 0u) != framed.size()) return 5;
    fwrite(framed.data(), 1, framed.size(), out);
    return fclose(out) == 0 ? 0 : 4;
}
