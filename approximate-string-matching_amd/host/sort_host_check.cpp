// Host build of the device-free parts of the sorted file calls (asm_map_file_sorted, asm_map_pairs_file_sorted), for the CPU
// test-suite (tests/test_sam_sort_host.py): plain g++, run under ASan + UBSan.  Three modes:
//
//   sort_host_check keys CASES OUT    sam_sort_key and the line sam_format writes, for every case (csrc/asm_sam.h).
//       CASES (little endian): u32 number of cases, u32 n_seqs; then per case the fields of host/sam_host_check.cpp's paired
//       format: u32 raw_len, raw bytes; 6 x u32 SamRec; i32 mapped, i32 seq_id, u32 pos, i32 dist, i32 greedy_cost, u32 strand,
//       u32 rank, u32 nops, u32 all, u32 n_reported, u32 n_hits; u32 stored ops (<= 64), u16 each; u32 rname_len, bytes; u32 paired,
//       u32 mate, u32 proper, u32 rescued, u32 mate_mapped, i32 mate_seq_id, u32 mate_pos, u32 mate_strand, u32 tlen,
//       u32 n_concordant; u32 mate_rname_len, bytes.  OUT per case: u64 key, u64 size, the line's bytes.
//   sort_host_check slabs LISTS OUT   sam_slab_cuts (csrc/asm_host.h).
//       LISTS: u32 number of lists; per list u64 cap, u64 n, n x u64 line sizes.  OUT per list: u64 number of cuts, the cuts as u64.
//   sort_host_check gather            sam_gather_line (csrc/asm_sam_sort.h), what sam_line_gather_kernel runs per lane: every
//       destination alignment with every source alignment and the lengths around every edge of the copy, the source in a block
//       with 4 bytes behind its text (what the copy may read; a held block has SAM_SORT_PAD) and the destination ending with its
//       allocation, lanes 0..15 in turn.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_host.h"
#include "../csrc/asm_sam_sort.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int keys(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0, n_seqs = 0;
    if (!get(in, &ncases, 4) || !get(in, &n_seqs, 4)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t raw_len = 0, u[11], stored = 0, rname_len = 0, v[10], mate_rname_len = 0;
        if (!get(in, &raw_len, 4)) return 3;
        std::vector<char> raw(raw_len);
        SamLine l = {};
        if (!get(in, raw.data(), raw_len) || !get(in, &l.rec, sizeof l.rec) || !get(in, u, sizeof u) || !get(in, &stored, 4)) return 3;
        std::vector<uint16_t> ops(stored);
        if (stored > SAM_CIGAR_CAP || !get(in, ops.data(), 2 * (size_t)stored) || !get(in, &rname_len, 4)) return 3;
        std::vector<char> rname(rname_len);
        if (!get(in, rname.data(), rname_len) || !get(in, v, sizeof v) || !get(in, &mate_rname_len, 4)) return 3;
        std::vector<char> mate_rname(mate_rname_len);
        if (!get(in, mate_rname.data(), mate_rname_len)) return 3;
        l.raw = raw.data();
        l.mapped = (int)u[0], l.seq_id = (int32_t)u[1], l.pos = u[2], l.dist = (int32_t)u[3], l.greedy_cost = (int32_t)u[4];
        l.strand = u[5], l.rank = u[6], l.nops = u[7], l.all = (int)u[8], l.n_reported = u[9], l.n_hits = u[10];
        l.ops = ops.data(), l.rname = rname.data(), l.rname_len = rname_len;
        l.paired = (int)v[0], l.mate = v[1], l.proper = (int)v[2], l.rescued = (int)v[3], l.mate_mapped = (int)v[4];
        l.mate_seq_id = (int32_t)v[5], l.mate_pos = v[6], l.mate_strand = v[7], l.tlen = v[8], l.n_concordant = v[9];
        l.mate_rname = mate_rname.data(), l.mate_rname_len = mate_rname_len;
        const uint64_t key = sam_sort_key(l, (int32_t)n_seqs), size = sam_line_size(l);
        char* line = (char*)calloc(size ? size : 1, 1);
        for (uint32_t lane = 0; lane < SAM_LANES; lane++) sam_line_emit(l, line, lane);
        fwrite(&key, 8, 1, out);
        fwrite(&size, 8, 1, out);
        fwrite(line, 1, size, out);
        free(line);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}

static int slabs(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    uint32_t nlists = 0;
    if (!get(in, &nlists, 4)) return 3;
    for (uint32_t t = 0; t < nlists; t++) {
        uint64_t cap = 0, n = 0;
        if (!get(in, &cap, 8) || !get(in, &n, 8)) return 3;
        std::vector<uint64_t> size(n), off(n + 1, 0); /* exactly n + 1 offsets: a read of off[n + 1] is a heap overflow */
        if (!get(in, size.data(), 8 * (size_t)n)) return 3;
        for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + size[i];
        const std::vector<size_t> cuts = asm_host::sam_slab_cuts(off.data(), (size_t)n, cap);
        const uint64_t k = cuts.size();
        fwrite(&k, 8, 1, out);
        for (size_t c : cuts) {
            const uint64_t v = c;
            fwrite(&v, 8, 1, out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}

static int gather() {
    const uint64_t lens[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 19, 20, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 255, 256, 257, 271, 272,
                             273, 300, 511, 512, 513, 527, 700, 1200};
    long checked = 0;
    for (uint64_t len : lens)
        for (uint32_t da = 0; da < 16; da++)
            for (uint32_t sa = 0; sa < 16; sa++) {
                /* the source line at offset sa of a block whose text ends with the line; the destination at offset da, ending with
                 * its allocation, behind da bytes that must stay as they are */
                const size_t src_bytes = sa + len + 4, dst_bytes = da + len;
                void *src_block = nullptr, *dst_block = nullptr;
                if (posix_memalign(&src_block, 64, src_bytes) != 0 || posix_memalign(&dst_block, 16, dst_bytes ? dst_bytes : 1) != 0) return 5;
                char *src = (char*)src_block, *dst = (char*)dst_block;
                for (size_t i = 0; i < src_bytes; i++) src[i] = (char)(1 + (i * 131 + len * 7 + sa) % 251);
                memset(dst, 0, dst_bytes ? dst_bytes : 1);
                for (uint32_t g = 0; g < SAM_GATHER_LANES; g++) sam_gather_line(dst + da, (const char*)(src + sa), len, g);
                if (memcmp(dst + da, src + sa, len) != 0) {
                    fprintf(stderr, "gather: len %llu dst %u src %u: bytes differ\n", (unsigned long long)len, da, sa);
                    return 1;
                }
                for (uint32_t i = 0; i < da; i++)
                    if (dst[i] != 0) {
                        fprintf(stderr, "gather: len %llu dst %u src %u: wrote in front of the line\n", (unsigned long long)len, da, sa);
                        return 1;
                    }
                free(src), free(dst);
                checked++;
            }
    printf("gather ok %ld\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "keys") == 0) return keys(argv[2], argv[3]);
    if (argc == 4 && strcmp(argv[1], "slabs") == 0) return slabs(argv[2], argv[3]);
    if (argc == 2 && strcmp(argv[1], "gather") == 0) return gather();
    return 2;
}
