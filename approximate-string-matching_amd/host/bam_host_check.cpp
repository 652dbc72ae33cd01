// Host build of the BAM record (csrc/asm_bam.h) and of the BGZF container's host-buildable part (csrc/asm_bgzf.h), for the CPU
// test-suite (tests/test_bam_host.py): plain g++, run under ASan + UBSan.
//
//   bam_host_check records <cases> <out>
// reads cases from <cases>, formats each the way the kernels do — the size sink, then the lane sink for lanes 0..63 in turn into a
// buffer of exactly that size — once as the SAM line and once as the BAM record, and writes both to <out>.
// Case (little endian): u32 raw_len, raw bytes; 6 x u32 SamRec; i32 mapped, i32 seq_id, u32 pos, i32 dist, i32 greedy_cost, u32 strand,
// u32 rank, u32 nops, u32 all, u32 n_reported, u32 n_hits; u32 stored ops (<= 64), u16 each; u32 rname_len, bytes; u32 paired, u32
// mate, u32 proper, u32 rescued, u32 mate_mapped, i32 mate_seq_id, u32 mate_pos, u32 mate_strand, u32 tlen, u32 n_concordant; u32
// mate_rname_len, bytes; i32 mapq; u32 md_len, bytes.  The file starts with u32 = number of cases.
// Output per case: u64 size, the SAM line; u64 size, the BAM record.
//
//   bam_host_check bgzf <in> <out> <with_eof>
// frames the bytes of <in> into <out> with bgzf_frame_host (the per-slice CRC, the combine and the slice copy that bgzf_frame_kernel's
// threads run) and prints one line per block: the payload's length and its CRC-32 in hex, as the block carries it.
//
//   bam_host_check header <in> <out>
// builds the BAM header with bam_header_bytes and writes it to <out>.  <in> (little endian): u32 l_text, the text; u32 n_ref; per
// reference sequence u32 name length, the name, u32 length.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../csrc/asm_bam.h"
#include "../csrc/asm_bgzf.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool get_bytes(FILE* f, std::vector<char>& v) {
    uint32_t n = 0;
    if (!get(f, &n, 4)) return false;
    v.resize(n);
    return get(f, v.data(), n);
}

static int records(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    if (!get(in, &ncases, 4)) return 3;
    for (uint32_t c = 0; c < ncases; c++) {
        std::vector<char> raw, rname, mate_rname, md;
        uint32_t u[11], v[10], stored = 0;
        int32_t mapq = 0;
        SamLine l = {};
        if (!get_bytes(in, raw) || !get(in, &l.rec, sizeof l.rec) || !get(in, u, sizeof u) || !get(in, &stored, 4)) return 3;
        std::vector<uint16_t> ops(stored);
        if (stored > SAM_CIGAR_CAP || !get(in, ops.data(), 2 * (size_t)stored) || !get_bytes(in, rname)) return 3;
        if (!get(in, v, sizeof v) || !get_bytes(in, mate_rname) || !get(in, &mapq, 4) || !get_bytes(in, md)) return 3;
        l.raw = raw.data();
        l.mapped = (int)u[0], l.seq_id = (int32_t)u[1], l.pos = u[2], l.dist = (int32_t)u[3], l.greedy_cost = (int32_t)u[4];
        l.strand = u[5], l.rank = u[6], l.nops = u[7], l.all = (int)u[8], l.n_reported = u[9], l.n_hits = u[10];
        l.ops = ops.data(), l.rname = rname.data(), l.rname_len = (uint32_t)rname.size();
        l.paired = (int)v[0], l.mate = v[1], l.proper = (int)v[2], l.rescued = (int)v[3], l.mate_mapped = (int)v[4];
        l.mate_seq_id = (int32_t)v[5], l.mate_pos = v[6], l.mate_strand = v[7], l.tlen = v[8], l.n_concordant = v[9];
        l.mate_rname = mate_rname.data(), l.mate_rname_len = (uint32_t)mate_rname.size();
        l.mapq = mapq, l.md = md.data(), l.md_len = (uint32_t)md.size();
        for (int bam = 0; bam < 2; bam++) {
            const uint64_t size = bam ? bam_record_size(l) : sam_line_size(l);
            char* bytes = (char*)calloc(size ? size : 1, 1); /* exactly the size: a byte too many is a heap overflow */
            for (uint32_t lane = 0; lane < SAM_LANES; lane++) {
                if (bam) bam_record_emit(l, bytes, lane);
                else sam_line_emit(l, bytes, lane);
            }
            fwrite(&size, 8, 1, out);
            fwrite(bytes, 1, size, out);
            free(bytes);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}

static int bgzf(const char* in_path, const char* out_path, int with_eof) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    std::vector<uint8_t> src, framed;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, in)) > 0;) src.insert(src.end(), buf, buf + got);
    fclose(in);
    bgzf_frame_host(src.data(), src.size(), with_eof, framed);
    if (framed.size() != bgzf_bound(src.size(), with_eof)) return 5;
    size_t at = 0;
    for (size_t done = 0; done < src.size();) {
        const size_t len = src.size() - done < BGZF_PAYLOAD ? src.size() - done : BGZF_PAYLOAD;
        uint32_t crc = 0;
        memcpy(&crc, framed.data() + at + BGZF_FRONT + len, 4);
        printf("%zu %08x\n", len, crc);
        at += BGZF_FRONT + len + BGZF_BACK, done += len;
    }
    fwrite(framed.data(), 1, framed.size(), out);
    return fclose(out) == 0 ? 0 : 4;
}

static int header(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    std::vector<char> text;
    uint32_t n_ref = 0;
    if (!get_bytes(in, text) || !get(in, &n_ref, 4)) return 3;
    std::vector<std::vector<char>> names(n_ref);
    std::vector<const char*> name_ptr(n_ref);
    std::vector<uint32_t> lengths(n_ref);
    for (uint32_t r = 0; r < n_ref; r++) {
        if (!get_bytes(in, names[r]) || !get(in, &lengths[r], 4)) return 3;
        names[r].push_back('\0');
        name_ptr[r] = names[r].data();
    }
    fclose(in);
    /* an empty text comes as NULL, as a call without a header gives it */
    const std::vector<uint8_t> bytes = bam_header_bytes(text.empty() ? nullptr : text.data(), text.size(), name_ptr.data(), lengths.data(), n_ref);
    fwrite(bytes.data(), 1, bytes.size(), out);
    return fclose(out) == 0 ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "records") == 0) return records(argv[2], argv[3]);
    if (argc == 5 && strcmp(argv[1], "bgzf") == 0) return bgzf(argv[2], argv[3], atoi(argv[4]));
    if (argc == 4 && strcmp(argv[1], "header") == 0) return header(argv[2], argv[3]);
    return 2;
}
