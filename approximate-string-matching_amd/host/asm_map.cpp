// asm-map: read mapper over the C ABI's read-mapping section (include/asm_mi355x.h; contract: docs/design/mapper.md), the
// counterpart of the reference's `my-mapper` (GASMA/mapper/main.cpp) without its on-disk index: the k-mer index is built in HBM
// at start-up.
//   asm-map -r ref.fa -q reads.fq [-o out.sam] [-e N] [--k 12] [--both-strands] [--max-occ N] [--chunk N]
//           [--all-hits N [--strata S]]
// --all-hits N writes up to N loci per read in rank order (asm_map_reads_all, strata S, default e): the primary record as without
// it, then the secondary ones (FLAG 256, SEQ and QUAL '*'), each with NH:i:<reported> HI:i:<rank + 1> XH:i:<all loci> after NM
// and XG.  Reads may be FASTQ or FASTA (QUAL '*').  Reads are processed in chunks of --chunk records, so the read file's size is not
// bounded by memory.  Reads longer than ASM_MAP_MAX_READ are written unmapped.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "asm_mi355x.h"

static void usage() {
    fprintf(stderr, "usage: asm-map -r ref.fa -q reads.fq [-o out.sam] [-e N] [--k 12] [--both-strands] [--max-occ N] [--chunk N] "
                    "[--all-hits N [--strata S]]\n");
    exit(2);
}

static std::string first_word(const std::string& s) {
    size_t a = 0;
    while (a < s.size() && (s[a] == ' ' || s[a] == '\t')) a++;
    size_t b = a;
    while (b < s.size() && s[b] != ' ' && s[b] != '\t') b++;
    return s.substr(a, b - a);
}

static bool get_line(FILE* f, std::string& line) {
    line.clear();
    int c;
    bool any = false;
    while ((c = fgetc(f)) != EOF) {
        any = true;
        if (c == '\n') break;
        line.push_back((char)c);
    }
    if (!line.empty() && line.back() == '\r') line.pop_back();
    return any;
}

static char up(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
static char comp(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

struct Record {
    std::string name, seq, qual;
};

/* FASTQ or FASTA records, one at a time */
struct ReadFile {
    FILE* f = nullptr;
    bool fasta = false;
    std::string pending; /* FASTA: the header line already read */
    bool next(Record& r) {
        std::string line;
        if (fasta) {
            if (pending.empty()) {
                while (get_line(f, line))
                    if (!line.empty() && line[0] == '>') break;
                if (line.empty() || line[0] != '>') return false;
                pending = line;
            }
            r.name = first_word(pending.substr(1)), r.seq.clear(), r.qual = "*";
            pending.clear();
            while (get_line(f, line)) {
                if (!line.empty() && line[0] == '>') {
                    pending = line;
                    break;
                }
                r.seq += line;
            }
            return true;
        }
        do {
            if (!get_line(f, line)) return false;
        } while (line.empty());
        r.name = first_word(line.substr(1));
        get_line(f, r.seq);
        get_line(f, line);
        get_line(f, r.qual);
        return true;
    }
};

int main(int argc, char** argv) {
    std::string ref_path, read_path, out_path = "out.sam";
    asm_map_params p = {0, 0, 0, 3};
    int k = 12;
    long chunk = 262144;
    int all_hits = 0, strata = -1; /* all_hits 0: the best hit only */
    std::string cl = "asm-map";
    for (int a = 1; a < argc; a++) cl += std::string(" ") + argv[a];
    for (int a = 1; a < argc; a++) {
        const std::string s = argv[a];
        auto val = [&]() -> const char* {
            if (a + 1 >= argc) usage();
            return argv[++a];
        };
        if (s == "-r") ref_path = val();
        else if (s == "-q") read_path = val();
        else if (s == "-o") out_path = val();
        else if (s == "-e") p.max_errors = atoi(val());
        else if (s == "--k") k = atoi(val());
        else if (s == "--both-strands") p.both_strands = 1;
        else if (s == "--max-occ") p.max_occ = atoi(val());
        else if (s == "--chunk") chunk = atol(val());
        else if (s == "--all-hits") all_hits = atoi(val());
        else if (s == "--strata") strata = atoi(val());
        else usage();
    }
    if (ref_path.empty() || read_path.empty() || chunk < 1 || all_hits < 0 || (strata >= 0 && !all_hits)) usage();
    if (strata < 0) strata = p.max_errors;
    const int slots = all_hits ? all_hits : 1; /* records per read in the library's output */

    /* reference: name = first word of the header */
    std::vector<std::string> names;
    std::vector<uint64_t> off(1, 0);
    std::string text;
    {
        FILE* f = fopen(ref_path.c_str(), "r");
        if (!f) {
            fprintf(stderr, "asm-map: cannot open %s\n", ref_path.c_str());
            return 1;
        }
        std::string line;
        while (get_line(f, line)) {
            if (!line.empty() && line[0] == '>') {
                if (!names.empty()) off.push_back(text.size());
                names.push_back(first_word(line.substr(1)));
            } else if (!names.empty()) {
                for (char c : line)
                    if (c != ' ' && c != '\t') text.push_back(up(c));
            }
        }
        fclose(f);
        if (names.empty()) {
            fprintf(stderr, "asm-map: no sequence in %s\n", ref_path.c_str());
            return 1;
        }
        off.push_back(text.size());
    }
    FILE* rf = fopen(read_path.c_str(), "r");
    if (!rf) {
        fprintf(stderr, "asm-map: cannot open %s\n", read_path.c_str());
        return 1;
    }
    ReadFile reads;
    reads.f = rf;
    {
        int c = fgetc(rf);
        reads.fasta = c == '>';
        if (c != EOF) ungetc(c, rf);
    }
    FILE* out = fopen(out_path.c_str(), "w");
    if (!out) {
        fprintf(stderr, "asm-map: cannot write %s\n", out_path.c_str());
        return 1;
    }
    asm_handle* h = nullptr;
    asm_index* ix = nullptr;
    int rc = asm_create(&h, 0);
    if (!rc) rc = asm_index_build(h, text.data(), off.data(), (int32_t)names.size(), k, &ix);
    if (rc) {
        fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
        return 1;
    }
    fprintf(out, "@HD\tVN:1.6\tSO:unsorted\n");
    for (size_t r = 0; r < names.size(); r++)
        fprintf(out, "@SQ\tSN:%s\tLN:%llu\n", names[r].c_str(), (unsigned long long)(off[r + 1] - off[r]));
    fprintf(out, "@PG\tID:asm-map\tPN:asm-map\tVN:%s\tCL:%s\n", asm_version(), cl.c_str());

    const int cap = 64;
    std::vector<Record> recs;
    std::vector<char> buf;
    std::vector<uint32_t> ro;
    std::vector<int64_t> slot; /* record -> index in the library call, -1 = not sent (too long) */
    std::vector<asm_map_hit> hits;
    std::vector<uint16_t> ops;
    std::vector<uint8_t> nops;
    std::vector<uint32_t> n_hits;
    long long n_total = 0, n_mapped = 0, n_long = 0;
    bool more = true;
    while (more) {
        recs.clear();
        Record r;
        while ((long)recs.size() < chunk && (more = reads.next(r))) recs.push_back(r);
        if (recs.empty()) break;
        buf.clear(), ro.assign(1, 0), slot.assign(recs.size(), -1);
        for (size_t q = 0; q < recs.size(); q++) {
            for (char& c : recs[q].seq) c = up(c);
            const size_t m = recs[q].seq.size();
            if (m < 1 || m > ASM_MAP_MAX_READ) {
                n_long += m > 0;
                continue;
            }
            slot[q] = (int64_t)ro.size() - 1;
            buf.insert(buf.end(), recs[q].seq.begin(), recs[q].seq.end());
            ro.push_back((uint32_t)buf.size());
        }
        const int64_t n = (int64_t)ro.size() - 1;
        hits.assign((size_t)(n + 1) * slots, asm_map_hit{});
        ops.assign((size_t)(n + 1) * slots * cap, 0);
        nops.assign((size_t)(n + 1) * slots, 0);
        n_hits.assign((size_t)n + 1, 0);
        if (all_hits)
            rc = asm_map_reads_all(h, ix, n, buf.data(), ro.data(), &p, strata, all_hits, n_hits.data(), hits.data(), ops.data(), cap,
                                   nops.data());
        else
            rc = asm_map_reads(h, ix, n, buf.data(), ro.data(), &p, hits.data(), ops.data(), cap, nops.data());
        if (rc) {
            fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
            return 1;
        }
        for (size_t q = 0; q < recs.size(); q++) {
            const Record& rec = recs[q];
            n_total++;
            const asm_map_hit* hp = slot[q] >= 0 ? &hits[(size_t)slot[q] * slots] : nullptr;
            if (!hp || !(hp->flags & ASM_MAP_MAPPED)) {
                fprintf(out, "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n", rec.name.c_str(), rec.seq.empty() ? "*" : rec.seq.c_str(),
                        rec.qual.empty() ? "*" : rec.qual.c_str());
                continue;
            }
            n_mapped++;
            std::string seq = rec.seq, qual = rec.qual;
            if (hp->strand) {
                seq.assign(rec.seq.rbegin(), rec.seq.rend());
                for (char& c : seq) c = comp(c);
                if (qual != "*") qual.assign(rec.qual.rbegin(), rec.qual.rend());
            }
            /* rank 0 is the primary record; with --all-hits, ranks 1.. follow as secondary records */
            const uint32_t nh = all_hits ? n_hits[(size_t)slot[q]] : 1u, nrep = nh < (uint32_t)slots ? nh : (uint32_t)slots;
            for (uint32_t t = 0; t < nrep; t++) {
                const size_t o = (size_t)slot[q] * slots + t;
                const asm_map_hit& hr = hits[o];
                char cigar[4096];
                const int nn = nops[o];
                if (asm_cigar_format(&ops[o * cap], nn, cap, cigar, sizeof(cigar)) != 0 || nn > cap) strcpy(cigar, "*");
                const int mapq = hr.greedy_cost + 60 < 254 ? hr.greedy_cost + 60 : 254;
                fprintf(out, "%s\t%d\t%s\t%u\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tXG:i:%d", rec.name.c_str(),
                        (hr.strand ? 16 : 0) | (t ? 256 : 0), names[(size_t)hr.seq_id].c_str(), hr.pos + 1, mapq, cigar,
                        t ? "*" : seq.c_str(), t || qual.empty() ? "*" : qual.c_str(), (int)hr.dist, hr.greedy_cost);
                if (all_hits) fprintf(out, "\tNH:i:%u\tHI:i:%u\tXH:i:%u", nrep, t + 1, nh);
                fputc('\n', out);
            }
        }
    }
    fclose(out);
    fclose(rf);
    asm_index_free(h, ix);
    asm_destroy(h);
    fprintf(stderr, "asm-map: %lld reads, %lld mapped, %lld longer than %d (unmapped)\n", n_total, n_mapped, n_long, ASM_MAP_MAX_READ);
    return 0;
}
