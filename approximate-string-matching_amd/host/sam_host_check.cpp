// Host build of asm_map_file's SAM formatter (csrc/asm_sam.h), for the CPU test-suite (tests/test_map_file_host.py): plain g++,
// run under ASan + UBSan.  Reads cases from argv[1], formats each the way the kernels do — sam_line_size, then sam_line_emit for
// lanes 0..63 in turn into a buffer of exactly that size — and writes size and bytes to argv[2].
//
// Case (little endian): u32 raw_len, raw bytes; 6 x u32 SamRec; i32 mapped, i32 seq_id, u32 pos, i32 dist, i32 greedy_cost,
// u32 strand, u32 rank, u32 nops, u32 all, u32 n_reported, u32 n_hits; u32 stored ops (<= 64), u16 each; u32 rname_len, bytes.
// The file starts with u32 = number of cases.  Output per case: u64 size, bytes.
// With a third argument `--pairs` (tests/test_map_pairs_file_host.py) every case goes on with the paired fields: u32 paired, u32 mate,
// u32 proper, u32 rescued, u32 mate_mapped, i32 mate_seq_id, u32 mate_pos, u32 mate_strand, u32 tlen, u32 n_concordant; u32
// mate_rname_len, bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_map_core.h"
#include "../csrc/asm_sam.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    const bool pairs = argc == 4 && strcmp(argv[3], "--pairs") == 0;
    if (argc != 3 && !pairs) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!get(in, &ncases, 4)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t raw_len = 0, u[11], stored = 0, rname_len = 0;
        if (!get(in, &raw_len, 4)) return 3;
        std::vector<char> raw(raw_len);
        SamLine l = {};
        if (!get(in, raw.data(), raw_len) || !get(in, &l.rec, sizeof l.rec) || !get(in, u, sizeof u) || !get(in, &stored, 4)) return 3;
        std::vector<uint16_t> ops(stored);
        if (stored > SAM_CIGAR_CAP || !get(in, ops.data(), 2 * (size_t)stored) || !get(in, &rname_len, 4)) return 3;
        std::vector<char> rname(rname_len);
        if (!get(in, rname.data(), rname_len)) return 3;
        l.raw = raw.data();
        l.mapped = (int)u[0], l.seq_id = (int32_t)u[1], l.pos = u[2], l.dist = (int32_t)u[3], l.greedy_cost = (int32_t)u[4];
        l.strand = u[5], l.rank = u[6], l.nops = u[7], l.all = (int)u[8], l.n_reported = u[9], l.n_hits = u[10];
        l.ops = ops.data(), l.rname = rname.data(), l.rname_len = rname_len;
        l.mapq = map_mapq_reference(l.mapped != 0, l.greedy_cost); /* the cases carry no MAPQ of their own: the reference model's */
        uint32_t v[10], mate_rname_len = 0;
        std::vector<char> mate_rname;
        if (pairs) {
            if (!get(in, v, sizeof v) || !get(in, &mate_rname_len, 4)) return 3;
            mate_rname.resize(mate_rname_len);
            if (!get(in, mate_rname.data(), mate_rname_len)) return 3;
            l.paired = (int)v[0], l.mate = v[1], l.proper = (int)v[2], l.rescued = (int)v[3], l.mate_mapped = (int)v[4];
            l.mate_seq_id = (int32_t)v[5], l.mate_pos = v[6], l.mate_strand = v[7], l.tlen = v[8], l.n_concordant = v[9];
            l.mate_rname = mate_rname.data(), l.mate_rname_len = mate_rname_len;
        }
        const uint64_t size = sam_line_size(l);
        char* line = (char*)calloc(size ? size : 1, 1); /* exactly the size: a byte too many is a heap overflow */
        for (uint32_t lane = 0; lane < SAM_LANES; lane++) sam_line_emit(l, line, lane);
        fwrite(&size, 8, 1, out);
        fwrite(line, 1, size, out);
        free(line);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
