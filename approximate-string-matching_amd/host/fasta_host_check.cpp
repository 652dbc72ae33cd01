// Host build of asm_index_build_file's FASTA parser: the rules of csrc/asm_fasta.h (byte class, line kind, name span, carried state)
// and the reader's cutter (fasta_cut of csrc/asm_host.h), run serially in the order of the kernels — newline positions, per-tile
// counts, the two scans, the scatter, the carried state — chunk by chunk, groups of 16 bytes in tiles of FASTA_TILE.  Plain g++;
// tests/test_index_file_host.py builds it under ASan + UBSan and compares its output with a parser written there.
//   fasta_host_check FILE CHUNK_BYTES...   (0: the whole file as one chunk)
// prints, for each chunk size in turn, "seqs N", then per sequence "seq OFFSET NAME-IN-HEX", then "text LEN", the text's bytes and a newline.
//   fasta_host_check --limits           prints which text lengths the index takes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../csrc/asm_fasta.h"
#include "../csrc/asm_host.h"

struct Parsed {
    FastaCarry carry = {};
    std::string text;
    std::vector<uint64_t> off;
    std::vector<std::string> names;
};

/* one chunk, as index_file_chunk runs it: raw holds FASTA_GROUP spare bytes behind nbytes */
static void chunk(Parsed& out, const char* raw, uint32_t nbytes) {
    std::vector<uint32_t> nl;
    for (uint32_t p = 0; p < nbytes; p++)
        if (raw[p] == '\n') nl.push_back(p);
    const uint32_t lines = (uint32_t)nl.size(), ntiles = (nbytes + FASTA_TILE - 1) / FASTA_TILE;
    const FastaCarry carry = out.carry;
    struct Thread {
        FastaGroup g;
        uint32_t w[4], j, eh;
    };
    std::vector<Thread> th((size_t)ntiles * (FASTA_TILE / FASTA_GROUP));
    std::vector<uint32_t> tile_hdr(ntiles + 1, 0), tile_kept(ntiles + 1, 0), hbase(ntiles + 1, 0), kbase(ntiles + 1, 0);
    /* fasta_count_kernel, then the scan of the header counts and fasta_resolve_kernel */
    uint32_t j = 0;
    std::vector<uint32_t> tile_cand(ntiles + 1, 0), tile_after(ntiles + 1, 0);
    for (uint32_t t = 0; t < ntiles; t++)
        for (uint32_t x = 0, eh = 0; x < FASTA_TILE / FASTA_GROUP; x++) {
            Thread& me = th[(size_t)t * (FASTA_TILE / FASTA_GROUP) + x];
            const uint32_t base = t * FASTA_TILE + x * FASTA_GROUP;
            const uint32_t valid = base < nbytes ? (nbytes - base < FASTA_GROUP ? nbytes - base : FASTA_GROUP) : 0u;
            memset(me.w, 0, sizeof me.w);
            if (valid) memcpy(me.w, raw + base, FASTA_GROUP);
            me.j = j, me.eh = eh, me.g = FastaGroup{0u, 0u, 0u};
            if (valid) me.g = fasta_group(me.w, valid, fasta_enter(raw, nl.data(), j, base, carry.kind));
            j += fasta_popc(me.g.nl), eh += fasta_popc(me.g.hdr);
            tile_hdr[t] += fasta_popc(me.g.hdr), tile_cand[t] += fasta_popc(me.g.cand);
            tile_after[t] += fasta_popc(fasta_keep_mask(me.g, me.eh > 0u));
        }
    for (uint32_t t = 0; t < ntiles; t++) hbase[t + 1] = hbase[t] + tile_hdr[t];
    for (uint32_t t = 0; t <= ntiles; t++) tile_kept[t] = carry.n_seqs + hbase[t] > 0u ? tile_cand[t] : tile_after[t];
    for (uint32_t t = 0; t < ntiles; t++) kbase[t + 1] = kbase[t] + tile_kept[t];
    /* fasta_scatter_kernel */
    out.text.resize((size_t)carry.text_len + kbase[ntiles]);
    std::vector<FastaHeader> headers(hbase[ntiles]);
    for (uint32_t t = 0; t < ntiles; t++)
        for (uint32_t x = 0, ek = 0; x < FASTA_TILE / FASTA_GROUP; x++) {
            const Thread& me = th[(size_t)t * (FASTA_TILE / FASTA_GROUP) + x];
            const uint32_t base = t * FASTA_TILE + x * FASTA_GROUP;
            const uint32_t keep = fasta_keep_mask(me.g, carry.n_seqs + hbase[t] + me.eh > 0u);
            const uint64_t first = carry.text_len + kbase[t] + ek;
            uint64_t dst = first;
            for (uint32_t m = keep; m; m &= m - 1u, dst++) out.text.at((size_t)dst) = fasta_upper(fasta_byte(me.w, (uint32_t)__builtin_ctz(m)));
            uint32_t idx = hbase[t] + me.eh;
            for (uint32_t m = me.g.hdr; m; m &= m - 1u, idx++) {
                const uint32_t q = (uint32_t)__builtin_ctz(m), below = (1u << q) - 1u;
                headers.at(idx) = fasta_header(raw, nbytes, nl.data(), lines, base + q, me.j + fasta_popc(me.g.nl & below), first + fasta_popc(keep & below));
            }
            ek += fasta_popc(keep);
        }
    /* fasta_carry_kernel, and the host's lists */
    fasta_carry_next(&out.carry, raw, nbytes, nl.data(), lines, kbase[ntiles], hbase[ntiles]);
    for (const FastaHeader& r : headers) {
        out.names.emplace_back(raw + r.name, r.name_len);
        out.off.push_back(r.text_off);
    }
}

/* FastaFill's loop: the carry, then `step` more bytes, cut by fasta_cut; a header line longer than that takes more */
static int run(const std::string& file, size_t step) {
    Parsed out;
    std::string buf;
    int at_line_start = 1;
    for (size_t pos = 0; pos < file.size() || !buf.empty();) {
        size_t cut = 0;
        int in_line = 0;
        for (;;) {
            buf.append(file, pos, step);
            pos = pos + step < file.size() ? pos + step : file.size();
            cut = pos >= file.size() ? buf.size() : asm_host::fasta_cut(buf.data(), buf.size(), at_line_start, &in_line);
            if (cut || pos >= file.size()) break;
        }
        at_line_start = !in_line;
        std::vector<char> raw(buf.begin(), buf.begin() + (long)cut); /* an exact copy, so that a read behind the spare bytes is caught */
        raw.resize(cut + FASTA_GROUP, 0);
        if (cut) chunk(out, raw.data(), (uint32_t)cut);
        buf.erase(0, cut);
    }
    printf("seqs %u\n", out.carry.n_seqs);
    for (size_t r = 0; r < out.names.size(); r++) {
        printf("seq %llu ", (unsigned long long)out.off[r]);
        for (unsigned char ch : out.names[r]) printf("%02x", ch);
        printf("\n");
    }
    printf("text %llu\n", (unsigned long long)out.carry.text_len);
    fwrite(out.text.data(), 1, out.text.size(), stdout);
    printf("\n");
    return out.text.size() == out.carry.text_len && out.names.size() == out.carry.n_seqs ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--limits")) {
        for (uint64_t len : {0ull, 0xfffffffeull, 0xffffffffull, 0x100000000ull}) printf("%llu %d\n", (unsigned long long)len, fasta_text_fits(len));
        return 0;
    }
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::string file;
    char tmp[4096];
    for (size_t n; (n = fread(tmp, 1, sizeof tmp, f)) > 0;) file.append(tmp, n);
    fclose(f);
    int bad = 0;
    for (int a = 2; a < argc; a++) bad |= run(file, atol(argv[a]) > 0 ? (size_t)atol(argv[a]) : file.size() + 1);
    return bad;
}
