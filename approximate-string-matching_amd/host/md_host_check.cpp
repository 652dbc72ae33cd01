// Host build of the MD:Z rule (csrc/asm_md.h) and of the SAM formatter's MD piece (csrc/asm_sam.h), for the CPU test-suite
// (tests/test_md_host.py): plain g++, run under ASan + UBSan.  Reads cases from argv[1] and does for each what the device does:
//   the rule   md_format over the read on its strand (map_read_byte, as map_md_kernel) into a heap row of exactly MD_ROW_CAP
//              bytes through the bounded sink: a byte beyond the row is a heap overflow
//   the line   sam_format of a mapped line that carries the row, through both sinks: sam_line_size, then sam_line_emit for lanes
//              0..63 in turn into a buffer of exactly that size
// and writes the results to argv[2].
//
// Case (little endian): u32 nops, u16 each; u32 strand; u32 m, the read's bytes (forward, upper case); u32 n, the window's bytes.
// The file starts with u32 = number of cases.  Output per case: u32 ok (the row consumed the read and the window exactly and the tag
// fits the row), u32 len, the tag's bytes; u64 size, the line's bytes (size 0 and no bytes when ok is 0).  The line is that of read
// "r" on sequence "chr" at pos 6 with dist 3 and greedy_cost -2, QUAL '*'; the test formats the same line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../csrc/asm_map_core.h"
#include "../csrc/asm_md.h"
#include "../csrc/asm_sam.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!get(in, &ncases, 4)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t nops = 0, strand = 0, m = 0, n = 0;
        if (!get(in, &nops, 4)) return 3;
        std::vector<uint16_t> ops(nops);
        if (!get(in, ops.data(), 2 * (size_t)nops) || !get(in, &strand, 4) || !get(in, &m, 4)) return 3;
        std::vector<char> q(m);
        if (!get(in, q.data(), m) || !get(in, &n, 4)) return 3;
        std::vector<char> w(n);
        if (!get(in, w.data(), n)) return 3;

        char* row = (char*)malloc(MD_ROW_CAP); /* exactly the device's row */
        MdRowSink o{row, (uint32_t)MD_ROW_CAP};
        const char* wp = w.data();
        const char* qp = q.data();
        const bool walked = md_format(ops.data(), nops, [&](uint32_t p) { return map_read_byte(qp, m, strand, p); }, m, [&](uint32_t p) { return wp[p]; }, n, o);
        const uint32_t ok = walked && o.cur <= (uint32_t)MD_ROW_CAP, len = ok ? o.cur : 0u;
        fwrite(&ok, 4, 1, out);
        fwrite(&len, 4, 1, out);
        fwrite(row, 1, len, out);

        uint64_t size = 0;
        char* line = nullptr;
        if (ok) {
            std::string raw = "r";
            raw.append(q.data(), m);
            SamLine l = {};
            l.raw = raw.data();
            l.rec.name = 0, l.rec.name_len = 1, l.rec.seq = 1, l.rec.seq_len = m;
            l.mapped = 1, l.seq_id = 0, l.pos = 5, l.dist = 3, l.greedy_cost = -2, l.strand = strand;
            l.mapq = map_mapq_reference(true, l.greedy_cost);
            l.ops = ops.data(), l.nops = nops, l.rname = "chr", l.rname_len = 3;
            l.md = row, l.md_len = len;
            size = sam_line_size(l);
            line = (char*)calloc(size ? size : 1, 1); /* exactly the size: a byte too many is a heap overflow */
            for (uint32_t lane = 0; lane < SAM_LANES; lane++) sam_line_emit(l, line, lane);
        }
        fwrite(&size, 8, 1, out);
        if (size) fwrite(line, 1, size, out);
        free(line);
        free(row);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
