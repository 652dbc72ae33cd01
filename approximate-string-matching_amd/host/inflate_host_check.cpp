// Host build of the BGZF container's decoder (csrc/asm_inflate.h: the walk, and per member the code that bgzf_inflate_kernel's wave
// runs, its 64 lanes as a loop), for the CPU test-suite (tests/test_inflate_host.py): plain g++, run under ASan + UBSan.
//
//   inflate_host_check <in> <out>        <in>: a file, or - for stdin
// walks the container and prints `container <status> <member> <offset> <total>` (status 0: <member> members of <total> output bytes;
// else the BGZF_IN_* class of the first bad member, its index and its file offset, and nothing more is done).  Then every member is
// decoded by itself, out of a copy that ends with the member, so that a read behind it is a sanitizer report: one line
// `<index> <offset> <csize> <isize> <status>` each, status an INF_* class.  The sound members' bytes go to <out>, each at its offset
// (a failed member leaves zeros), and the whole container is decoded once more in one piece, which must give the same bytes and the
// first failed member.  Exit status 0 whatever the statuses are; 5 when the two decodings differ.
//
//   inflate_host_check tables <root> <cap> @<file>      one code per line of <file>: its lengths
// builds each code's table with inf_build and prints the result (INF_CODE_*) and the entries the table takes; a table above <cap>
// stops the program in inf_build's assert.
//
//   inflate_host_check classes
// prints every status class: `member <k> <text>` for the INF_* classes, `container <k> <text>` for the BGZF_IN_* classes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../csrc/asm_inflate.h"

static bool read_all(const char* path, std::vector<uint8_t>& data) {
    FILE* in = strcmp(path, "-") == 0 ? stdin : fopen(path, "rb");
    if (!in) return false;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, in)) > 0;) data.insert(data.end(), buf, buf + got);
    if (in != stdin) fclose(in);
    return true;
}

static int tables_mode(int argc, char** argv) {
    if (argc != 5 || argv[4][0] != '@') return 2;
    const uint32_t root = (uint32_t)atoi(argv[2]), cap = (uint32_t)atoi(argv[3]);
    if (root < 1u || root > 15u || cap < (1u << root) || cap > 65536u) return 2;
    std::vector<uint8_t> text;
    if (!read_all(argv[4] + 1, text)) return 2;
    std::istringstream lines(std::string(text.begin(), text.end()));
    for (std::string line; std::getline(lines, line);) {
        std::istringstream fields(line);
        std::vector<uint8_t> lens;
        for (uint32_t v; fields >> v;) {
            if (v > 15u) return 2;
            lens.push_back((uint8_t)v);
        }
        if (lens.empty()) continue;
        std::vector<uint16_t> tab(cap, 0xeeeeu);
        uint16_t count[16], next[16];
        const uint32_t kind = inf_build(tab.data(), root, cap, lens.data(), (uint32_t)lens.size(), count, next);
        size_t used = 0;
        if (kind == INF_CODE_COMPLETE) {
            /* every entry the builder placed is written: a complete code leaves no hole */
            used = 1u << root;
            for (uint32_t i = 0; i < (1u << root); i++)
                if (tab[i] & INF_LINK) used += 1u << (tab[i] & 15u);
            for (size_t i = 0; i < used; i++)
                if (tab[i] == 0xeeeeu || (tab[i] & 15u) == 0u) return 5;
        }
        printf("%u %zu\n", kind, used);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "tables") == 0) return tables_mode(argc, argv);
    if (argc == 2 && strcmp(argv[1], "classes") == 0) {
        for (uint32_t k = 0; k < INF_E_CLASSES; k++) printf("member %u %s\n", k, inf_status_text(k));
        for (uint32_t k = 0; k < BGZF_IN_CLASSES; k++) printf("container %u %s\n", k, bgzf_in_text(k));
        return 0;
    }
    if (argc != 3) return 2;
    std::vector<uint8_t> src;
    if (!read_all(argv[1], src)) return 2;
    std::vector<InfMember> members;
    size_t total = 0;
    const BgzfWalkError err = bgzf_walk(src.data(), src.size(), &members, &total);
    if (err.status != BGZF_IN_OK) {
        printf("container %u %zu %zu 0\n", err.status, err.member, err.offset);
        return 0;
    }
    printf("container 0 %zu %zu %zu\n", members.size(), members.size() ? (size_t)members.back().src_off : (size_t)0, total);
    std::vector<uint8_t> apart(total), whole(total);
    unsigned long long first = INF_NONE_BAD;
    for (size_t k = 0; k < members.size(); k++) {
        const InfMember& m = members[k];
        const std::vector<uint8_t> own(src.begin() + (ptrdiff_t)m.src_off, src.begin() + (ptrdiff_t)(m.src_off + m.csize));
        InfMember alone = m;
        alone.src_off = 0;
        const unsigned long long bad = bgzf_inflate_host(own.data(), std::vector<InfMember>(1, alone), apart.data());
        const uint32_t status = bad == INF_NONE_BAD ? 0u : (uint32_t)(bad & 0xffu);
        if (status && first == INF_NONE_BAD) first = (unsigned long long)k << 8 | status;
        printf("%zu %llu %u %u %u\n", k, m.src_off, m.csize, m.isize, status);
    }
    if (bgzf_inflate_host(src.data(), members, whole.data()) != first || whole != apart) return 5;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (!apart.empty()) fwrite(apart.data(), 1, apart.size(), out);
    return fclose(out) == 0 ? 0 : 4;
}
