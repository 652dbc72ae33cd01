// asm-map: read mapper over the C ABI's read-mapping section (include/asm_mi355x.h; contract: docs/design/mapper.md), the
// counterpart of the reference's `my-mapper` (GASMA/mapper/main.cpp) without its on-disk index: the k-mer index is built in HBM
// at start-up.
//   asm-map -r ref.fa -q reads.fq [-o out.sam] [-e N] [--k 12] [--both-strands] [--max-occ N] [--chunk N]
//           [--all-hits N [--strata S]]
//   asm-map -r ref.fa -1 r1.fq -2 r2.fq [-o out.sam] -e N --insert MIN,MAX [--rescue E] [--k 12] [--max-occ N] [--chunk N]
//           [--all-hits N [--strata S]]
//   asm-map -r ref.fa -q reads.fq --stream [--chunk-bytes N] [-o out.sam] [-e N] [--k 12] [--both-strands] [--max-occ N]
//           [--all-hits N [--strata S]]
// --stream hands the FASTQ file and the SAM path to asm_map_file, which parses, maps and formats on the device while it reads and
// writes (four-line FASTQ only; the same lines as without it); --chunk-bytes N: file bytes per chunk (default: the library's).
// --stream-pairs does the same for paired mode through asm_map_pairs_file (two four-line FASTQ files; the lines of -1 / -2 without
// --all-hits); --stream together with -2 is a usage error.  Both take bgzip-compressed (BGZF) files as they are: the library probes
// each file's first bytes and inflates on the device; the other modes parse their reads here and take text only.
// --ref-stream (any mode) builds the index with asm_index_build_file, which reads and parses the reference on the device, and takes
// the names and lengths for @SQ and RNAME from the index; without it the reference is parsed here.  The SAM is the same.
// --sort (any mapping mode) writes the same lines in coordinate order: ascending (index of RNAME among the reference's sequences, POS),
// '*' behind every sequence, lines with equal keys in the order they have without --sort; the header's first line then reads
// SO:coordinate.  With --stream / --stream-pairs the library sorts on the device (asm_map_file_sorted, asm_map_pairs_file_sorted;
// --sort-mem BYTES: the most device memory the held SAM text and its tables may take, default no cap); without them the lines are
// built as always and sorted here, by the key read from their text.  The two ways give the same file.
// --mapq reference|gap (any mapping mode; default reference) picks the model of column 5 (asm_map_set_mapq_model): reference is
// min(254, 60 + greedy_cost), gap the repeat- and pair-aware value of docs/design/mapper.md, "Mapping quality".  The streamed modes
// let the library format it; the others read it with asm_map_last_mapq, so both ways write the same file under either model.
// --md (any mapping mode) adds MD:Z:<tag> behind XG:i:<n> on every line that shows a CIGAR (docs/design/mapper.md, "MD tag").  The
// streamed modes set the handle's tag mask (asm_map_set_sam_tags) and the library builds the tag on the device; the others call
// asm_md_format per record, on the reference window from the text parsed here or, under --ref-stream, from asm_index_get_text.  Both
// ways write the same file.
// --bam (--stream and --stream-pairs only, with or without --sort) makes the library write BAM to -o (asm_map_set_output_format;
// docs/design/mapper.md, "BAM output"): the same records, encoded and BGZF-framed in stored blocks on the device.  The header text
// and every other option are as for SAM.  With any other mode it is a usage error.  --bam-level 0|1 (with --bam; default 0) is the
// container's level (asm_map_set_bgzf_level; docs/design/mapper.md, "Deflate"): 1 deflates every block on the device.
// --bai (with --bam --sort under --stream or --stream-pairs) makes the library write the BAI index <out>.bai beside the BAM file
// (asm_map_set_bam_index; docs/design/mapper.md, "BAM index"), built on the device.  Anywhere else it is a usage error.
//   asm-map -r ref.fa --bench-ref N [--k 12]
// maps nothing: it builds the index N times each way, alternately, and prints the seconds of every build.
// --all-hits N writes up to N loci per read in rank order (asm_map_reads_all, strata S, default e): the primary record as without
// it, then the secondary ones (FLAG 256, SEQ and QUAL '*'), each with NH:i:<reported> HI:i:<rank + 1> XH:i:<all loci> after NM
// and XG.  Reads may be FASTQ or FASTA (QUAL '*').  Reads are processed in chunks of --chunk records, so the read file's size is not
// bounded by memory.  Reads longer than ASM_MAP_MAX_READ are written unmapped.
// Paired mode (-1 / -2, asm_map_pairs: FR pairs with a projected span in [MIN, MAX], mate rescue with E errors) searches both
// strands and writes mate 1 then mate 2.  QNAME is the first word without a trailing /1 or /2; the two files must name the pairs
// alike.  FLAG = 1 | 2 (proper) | 4 / 8 (self / mate unmapped) | 16 / 32 (self / mate reverse) | 64 / 128 (mate 1 / 2); an
// unmapped mate of a mapped mate takes its RNAME and POS; RNEXT is '=' on the same sequence and '*' when the mate is unmapped;
// PNEXT is the mate's POS; TLEN is +tlen on the mate with the smaller POS (mate 1 when equal) and -tlen on the other.  Proper
// pairs carry XP:i:<n_concordant>, rescued records XR:i:1.  A mate longer than ASM_MAP_MAX_READ (or empty) leaves its pair
// unmapped.
// Paired --all-hits N writes up to N concordant pairs per fragment in rank order (asm_map_pairs_all, pair strata S on the d sum,
// default 2e), mate 1 then mate 2 for each: rank 0 as without it, then the secondary pairs (FLAG 1 | 2 | 256 | 16 / 32 | 64 / 128,
// SEQ and QUAL '*', RNEXT '=', PNEXT the POS of the other mate of that pair, TLEN that pair's +-tlen by the rule above, tags NM and
// XG).  Every record of a fragment with at least one concordant pair ends with NH:i:<reported pairs> HI:i:<rank + 1>
// XH:i:<eligible pairs>; both mates of a pair share HI.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

#include "asm_mi355x.h"

static void usage() {
    fprintf(stderr, "usage: asm-map -r ref.fa -q reads.fq [-o out.sam] [-e N] [--k 12] [--both-strands] [--max-occ N] [--chunk N] "
                    "[--all-hits N [--strata S]]\n"
                    "       asm-map -r ref.fa -1 r1.fq -2 r2.fq [-o out.sam] -e N --insert MIN,MAX [--rescue E] [--k 12] [--max-occ N] "
                    "[--chunk N] [--all-hits N [--strata S]]\n"
                    "       asm-map -r ref.fa -q reads.fq --stream [--chunk-bytes N] [-o out.sam] [-e N] [--k 12] [--both-strands] "
                    "[--max-occ N] [--all-hits N [--strata S]]\n"
                    "       asm-map -r ref.fa -1 r1.fq -2 r2.fq --stream-pairs [--chunk-bytes N] [-o out.sam] -e N --insert MIN,MAX "
                    "[--rescue E] [--k 12] [--max-occ N]\n"
                    "       --stream takes reads.fq.gz, --stream-pairs r1.fq.gz and r2.fq.gz, as bgzip writes them (BGZF), inflated on the device\n"
                    "       any of them with --ref-stream: the reference is read and parsed by the library\n"
                    "       any of them with --mapq reference|gap: the model of the MAPQ column (default reference)\n"
                    "       any of them with --md: MD:Z on every line that shows a CIGAR\n"
                    "       --stream, --stream-pairs with --bam: BAM output (BGZF with stored blocks), encoded on the device\n"
                    "       --bam with --bam-level 0|1: 0 (default) stored blocks, 1 deflate blocks compressed on the device\n"
                    "       --bam --sort with --bai: the BAI index <out>.bai beside the BAM file, built on the device\n"
                    "       any of them with --sort: coordinate-sorted output (--stream, --stream-pairs: on the device, [--sort-mem BYTES])\n");
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

static std::string pair_name(const std::string& n) {
    if (n.size() >= 2 && n[n.size() - 2] == '/' && (n.back() == '1' || n.back() == '2')) return n.substr(0, n.size() - 2);
    return n;
}

static std::string revcomp(const std::string& q) {
    std::string o(q.rbegin(), q.rend());
    for (char& c : o) c = comp(c);
    return o;
}

/* --md without --stream: "\tMD:Z:<tag>" of one record ("" without --md and for a row of more than cap operations, whose CIGAR
 * column is '*'); text: the upper-cased reference, parsed here or, under --ref-stream, read back from the index; seq: the read as
 * the file holds it, upper case */
struct MdSource {
    bool on;
    const std::string* text;
    const std::vector<uint64_t>* off;
    std::string tag(const asm_map_hit& hr, const uint16_t* ops, int nn, int cap, const std::string& seq) const {
        if (!on || nn > cap) return "";
        char md[ASM_MAP_MD_CAP];
        const std::string qs = hr.strand ? revcomp(seq) : seq;
        if (asm_md_format(ops, nn, qs.data(), (int)qs.size(), text->data() + (*off)[(size_t)hr.seq_id] + hr.pos, (int)(hr.end - hr.pos), md,
                          sizeof md) < 0) {
            fprintf(stderr, "asm-map: %s\n", asm_last_error(nullptr));
            exit(1);
        }
        return std::string("\tMD:Z:") + md;
    }
};

static int write_pairs(FILE* out, asm_handle* h, asm_index* ix, const std::vector<std::string>& names, ReadFile& f1, ReadFile& f2,
                       const asm_map_params& p, const asm_pair_params& pp, long chunk, int all_hits, int strata, const MdSource& mds) {
    const int cap = 64;
    const int slots = all_hits ? all_hits : 1; /* pairs per fragment in the library's output */
    std::vector<Record> a, b;
    std::vector<char> buf1, buf2;
    std::vector<uint32_t> ro1, ro2;
    std::vector<int64_t> slot;
    std::vector<asm_map_hit> hits;
    std::vector<int32_t> tlen;
    std::vector<uint32_t> nconc, npairs;
    std::vector<uint16_t> ops;
    std::vector<uint8_t> nops, mq;
    long long n_pairs = 0, n_proper = 0, n_rescued = 0, n_secondary = 0;
    bool more = true;
    while (more) {
        a.clear(), b.clear();
        Record r1, r2;
        while ((long)a.size() < chunk) {
            const bool g1 = f1.next(r1), g2 = f2.next(r2);
            if (g1 != g2) {
                fprintf(stderr, "asm-map: the two read files hold different numbers of records\n");
                return 1;
            }
            if (!(more = g1)) break;
            if (pair_name(r1.name) != pair_name(r2.name)) {
                fprintf(stderr, "asm-map: mate names differ: %s and %s\n", r1.name.c_str(), r2.name.c_str());
                return 1;
            }
            a.push_back(r1), b.push_back(r2);
        }
        if (a.empty()) break;
        buf1.clear(), buf2.clear(), ro1.assign(1, 0), ro2.assign(1, 0), slot.assign(a.size(), -1);
        for (size_t q = 0; q < a.size(); q++) {
            for (char& c : a[q].seq) c = up(c);
            for (char& c : b[q].seq) c = up(c);
            const size_t m1 = a[q].seq.size(), m2 = b[q].seq.size();
            if (m1 < 1 || m1 > ASM_MAP_MAX_READ || m2 < 1 || m2 > ASM_MAP_MAX_READ) continue;
            slot[q] = (int64_t)ro1.size() - 1;
            buf1.insert(buf1.end(), a[q].seq.begin(), a[q].seq.end());
            buf2.insert(buf2.end(), b[q].seq.begin(), b[q].seq.end());
            ro1.push_back((uint32_t)buf1.size()), ro2.push_back((uint32_t)buf2.size());
        }
        const int64_t n = (int64_t)ro1.size() - 1;
        hits.assign((size_t)(n + 1) * 2 * slots, asm_map_hit{});
        tlen.assign((size_t)(n + 1) * slots, 0), nconc.assign((size_t)n + 1, 0), npairs.assign((size_t)n + 1, 0);
        ops.assign((size_t)(n + 1) * 2 * slots * cap, 0), nops.assign((size_t)(n + 1) * 2 * slots, 0);
        const int rc = all_hits ? asm_map_pairs_all(h, ix, n, buf1.data(), ro1.data(), buf2.data(), ro2.data(), &p, &pp, strata, all_hits,
                                                    npairs.data(), hits.data(), tlen.data(), nconc.data(), ops.data(), cap, nops.data())
                                : asm_map_pairs(h, ix, n, buf1.data(), ro1.data(), buf2.data(), ro2.data(), &p, &pp, hits.data(),
                                                tlen.data(), nconc.data(), ops.data(), cap, nops.data());
        mq.assign((size_t)(n + 1) * 2 * slots, 0);
        if (rc || asm_map_last_mapq(h, mq.data(), n * 2 * slots)) {
            fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
            return 1;
        }
        const asm_map_hit none = {-1, 0, 0, -1, 0, 0, -1};
        for (size_t q = 0; q < a.size(); q++) {
            n_pairs++;
            const Record* rec[2] = {&a[q], &b[q]};
            const asm_map_hit* hr[2] = {&none, &none};
            if (slot[q] >= 0) hr[0] = &hits[(size_t)slot[q] * 2 * slots], hr[1] = &hits[(size_t)slot[q] * 2 * slots + 1];
            const bool mapped[2] = {(hr[0]->flags & ASM_MAP_MAPPED) != 0, (hr[1]->flags & ASM_MAP_MAPPED) != 0};
            const bool proper = (hr[0]->flags & ASM_MAP_PROPER_PAIR) != 0;
            n_proper += proper;
            /* RNAME / POS of each record: its own, else its mapped mate's */
            int rid[2];
            long long pos[2];
            for (int x = 0; x < 2; x++) {
                const int y = mapped[x] ? x : mapped[1 - x] ? 1 - x : -1;
                rid[x] = y < 0 ? -1 : hr[y]->seq_id;
                pos[x] = y < 0 ? 0 : (long long)hr[y]->pos + 1;
            }
            const long long tl = slot[q] >= 0 ? tlen[(size_t)slot[q] * slots] : 0;
            /* with --all-hits: NH / HI / XH on every record of a fragment with a concordant pair */
            const uint32_t nh = all_hits && slot[q] >= 0 ? npairs[(size_t)slot[q]] : 0u, nrep = nh < (uint32_t)slots ? nh : (uint32_t)slots;
            const int plus = pos[0] <= pos[1] ? 0 : 1; /* the mate whose TLEN is positive */
            for (int x = 0; x < 2; x++) {
                const asm_map_hit& m = *hr[x];
                const int y = 1 - x;
                int flag = 1 | (proper ? 2 : 0) | (mapped[x] ? 0 : 4) | (mapped[y] ? 0 : 8) | (x ? 128 : 64);
                if (mapped[x] && m.strand) flag |= 16;
                if (mapped[y] && hr[y]->strand) flag |= 32;
                std::string seq = rec[x]->seq, qual = rec[x]->qual;
                char cigar[4096];
                strcpy(cigar, "*");
                int mapq = 0;
                std::string md;
                if (mapped[x]) {
                    if (m.strand) {
                        seq = revcomp(rec[x]->seq);
                        if (qual != "*") qual.assign(rec[x]->qual.rbegin(), rec[x]->qual.rend());
                    }
                    const size_t o = (size_t)slot[q] * 2 * slots + x;
                    const int nn = nops[o];
                    if (asm_cigar_format(&ops[o * cap], nn, cap, cigar, sizeof(cigar)) != 0 || nn > cap) strcpy(cigar, "*");
                    mapq = mq[o];
                    md = mds.tag(m, &ops[o * cap], nn, cap, rec[x]->seq);
                }
                const char* rnext = !mapped[y] ? "*" : rid[y] == rid[x] ? "=" : names[(size_t)rid[y]].c_str();
                fprintf(out, "%s\t%d\t%s\t%lld\t%d\t%s\t%s\t%lld\t%lld\t%s\t%s", pair_name(rec[x]->name).c_str(), flag,
                        rid[x] < 0 ? "*" : names[(size_t)rid[x]].c_str(), pos[x], mapq, cigar, rnext, pos[y], x == plus ? tl : -tl,
                        seq.empty() ? "*" : seq.c_str(), qual.empty() ? "*" : qual.c_str());
                if (mapped[x]) fprintf(out, "\tNM:i:%d\tXG:i:%d%s", (int)m.dist, m.greedy_cost, md.c_str());
                if (proper) fprintf(out, "\tXP:i:%u", nconc[(size_t)slot[q]]);
                if (m.flags & ASM_MAP_RESCUED) {
                    fprintf(out, "\tXR:i:1");
                    n_rescued++;
                }
                if (nh) fprintf(out, "\tNH:i:%u\tHI:i:1\tXH:i:%u", nrep, nh);
                fputc('\n', out);
            }
            /* secondary pairs, rank 1.., both mates mapped on one sequence */
            for (uint32_t t = 1; t < nrep; t++) {
                const size_t o = ((size_t)slot[q] * slots + t) * 2;
                const asm_map_hit* sr[2] = {&hits[o], &hits[o + 1]};
                const long long stl = tlen[(size_t)slot[q] * slots + t];
                const int splus = sr[0]->pos <= sr[1]->pos ? 0 : 1;
                n_secondary++;
                for (int x = 0; x < 2; x++) {
                    const asm_map_hit& m = *sr[x];
                    const int flag = 1 | 2 | 256 | (m.strand ? 16 : 0) | (sr[1 - x]->strand ? 32 : 0) | (x ? 128 : 64);
                    char cigar[4096];
                    const int nn = nops[o + x];
                    if (asm_cigar_format(&ops[(o + x) * cap], nn, cap, cigar, sizeof(cigar)) != 0 || nn > cap) strcpy(cigar, "*");
                    const int mapq = mq[o + x];
                    fprintf(out, "%s\t%d\t%s\t%u\t%d\t%s\t=\t%u\t%lld\t*\t*\tNM:i:%d\tXG:i:%d%s\tNH:i:%u\tHI:i:%u\tXH:i:%u\n",
                            pair_name(rec[x]->name).c_str(), flag, names[(size_t)m.seq_id].c_str(), m.pos + 1, mapq, cigar,
                            sr[1 - x]->pos + 1, x == splus ? stl : -stl, (int)m.dist, m.greedy_cost,
                            mds.tag(m, &ops[(o + x) * cap], nn, cap, rec[x]->seq).c_str(), nrep, t + 1, nh);
                }
            }
        }
    }
    fprintf(stderr, "asm-map: %lld pairs, %lld proper, %lld mates rescued\n", n_pairs, n_proper, n_rescued);
    if (all_hits) fprintf(stderr, "asm-map: %lld secondary pairs\n", n_secondary);
    return 0;
}

/* --sort without --stream: the SAM lines text[0, len), as the modes below built them, in coordinate order.  The key is read from a
 * line's own RNAME and POS columns: (index of RNAME in names, names.size() for '*' or a name that is none of them) << 32 | POS. */
static bool write_sorted(FILE* file, const char* text, size_t len, const std::vector<std::string>& names) {
    std::unordered_map<std::string, uint64_t> tid;
    for (size_t r = 0; r < names.size(); r++) tid.emplace(names[r], (uint64_t)r);
    struct Line {
        uint64_t key;
        const char* at;
        size_t bytes;
    };
    std::vector<Line> lines;
    for (size_t a = 0; a < len;) {
        const char* nl = (const char*)memchr(text + a, '\n', len - a);
        const size_t end = nl ? (size_t)(nl - text) + 1 : len;
        size_t tab[4], ntab = 0;
        for (size_t i = a; i < end && ntab < 4; i++)
            if (text[i] == '\t') tab[ntab++] = i;
        uint64_t key = (uint64_t)names.size() << 32;
        if (ntab == 4) {
            const auto it = tid.find(std::string(text + tab[1] + 1, tab[2] - tab[1] - 1));
            key = (it == tid.end() ? (uint64_t)names.size() : it->second) << 32 | strtoull(text + tab[2] + 1, nullptr, 10);
        }
        lines.push_back({key, text + a, end - a});
        a = end;
    }
    std::stable_sort(lines.begin(), lines.end(), [](const Line& x, const Line& y) { return x.key < y.key; });
    for (const Line& l : lines)
        if (fwrite(l.at, 1, l.bytes, file) != l.bytes) return false;
    return true;
}

/* the report line of --sort with --stream or --stream-pairs */
static void report_index(const asm_bam_index_stats& st) {
    fprintf(stderr, "asm-map: index of %lld bytes: %lld bins, %lld chunks, %lld windows, %lld records without coordinates, %.3f s\n",
            (long long)st.bytes, (long long)st.bins, (long long)st.chunks, (long long)st.intervals, (long long)st.no_coor, st.seconds_index);
}
static void report_sorted(const asm_sam_sort_stats& st) {
    fprintf(stderr, "asm-map: sorted %lld lines, %lld bytes held on the device, %lld slabs, %.3f s\n", (long long)st.lines,
            (long long)st.bytes_held, (long long)st.slabs, st.seconds_sort);
}

/* the second report line of --stream and --stream-pairs: what the two calls' stats share */
template <class Stats>
static void report_streamed(const Stats& st) {
    fprintf(stderr, "asm-map: streamed %lld chunks, %lld bytes in, %lld bytes out, %.3f s (reader busy %.3f s, writer busy %.3f s)\n",
            (long long)st.chunks, (long long)st.bytes_in, (long long)st.bytes_out, st.seconds, st.seconds_read, st.seconds_write);
}

/* the reference, parsed here: name = first word of the header; off starts as {0} */
static bool parse_reference(const std::string& ref_path, std::vector<std::string>& names, std::vector<uint64_t>& off, std::string& text) {
    FILE* f = fopen(ref_path.c_str(), "r");
    if (!f) {
        fprintf(stderr, "asm-map: cannot open %s\n", ref_path.c_str());
        return false;
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
        return false;
    }
    off.push_back(text.size());
    return true;
}

/* --bench-ref N: the two ways from the reference file to its index, alternately in one process, N times each; one line of seconds
 * per build on stdout (tools/bench_index_file.py reads them) */
static int bench_reference(const std::string& ref_path, int k, int reps) {
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double>(b - a).count();
    };
    asm_handle* h = nullptr;
    if (asm_create(&h, 0)) {
        fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
        return 1;
    }
    for (int rep = 0; rep < reps; rep++) {
        asm_index* ix = nullptr;
        {
            std::vector<std::string> names;
            std::vector<uint64_t> off(1, 0);
            std::string text;
            const auto t0 = now();
            if (!parse_reference(ref_path, names, off, text)) return 1;
            const auto t1 = now();
            const int rc = asm_index_build(h, text.data(), off.data(), (int32_t)names.size(), k, &ix);
            const auto t2 = now();
            if (rc) {
                fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
                return 1;
            }
            printf("host seconds %.6f parse %.6f index_build %.6f bases %llu\n", secs(t0, t2), secs(t0, t1), secs(t1, t2),
                   (unsigned long long)text.size());
            asm_index_free(h, ix);
        }
        asm_index_file_stats st;
        const auto t0 = now();
        const int rc = asm_index_build_file(h, ref_path.c_str(), k, 0, &ix, &st);
        const auto t1 = now();
        if (rc) {
            fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
            return 1;
        }
        printf("file seconds %.6f reader_busy %.6f index_stage %.6f chunks %lld bases %lld\n", secs(t0, t1), st.seconds_read, st.seconds_index,
               (long long)st.chunks, (long long)st.bases);
        asm_index_free(h, ix);
    }
    asm_destroy(h);
    return 0;
}

int main(int argc, char** argv) {
    std::string ref_path, read_path, read2_path, out_path = "out.sam";
    asm_pair_params pp = {-1, -1, -1};
    asm_map_params p = {0, 0, 0, 3};
    int k = 12;
    long chunk = 262144;
    int all_hits = 0, strata = -1; /* all_hits 0: the best hit only */
    bool stream = false, stream_pairs = false, ref_stream = false, sort = false, md = false, bam = false, bai = false;
    int bam_level = -1; /* --bam-level: not given */
    int bench_ref = 0;
    long long chunk_bytes = 0, sort_mem = -1;
    int mapq_model = ASM_MAPQ_REFERENCE;
    std::string cl = "asm-map";
    for (int a = 1; a < argc; a++) cl += std::string(" ") + argv[a];
    for (int a = 1; a < argc; a++) {
        const std::string s = argv[a];
        auto val = [&]() -> const char* {
            if (a + 1 >= argc) usage();
            return argv[++a];
        };
        if (s == "-r") ref_path = val();
        else if (s == "-q" || s == "-1") read_path = val();
        else if (s == "-2") read2_path = val();
        else if (s == "--insert") {
            if (sscanf(val(), "%d,%d", &pp.min_insert, &pp.max_insert) != 2) usage();
        } else if (s == "--rescue") pp.rescue_errors = atoi(val());
        else if (s == "-o") out_path = val();
        else if (s == "-e") p.max_errors = atoi(val());
        else if (s == "--k") k = atoi(val());
        else if (s == "--both-strands") p.both_strands = 1;
        else if (s == "--max-occ") p.max_occ = atoi(val());
        else if (s == "--chunk") chunk = atol(val());
        else if (s == "--all-hits") all_hits = atoi(val());
        else if (s == "--strata") strata = atoi(val());
        else if (s == "--stream") stream = true;
        else if (s == "--stream-pairs") stream_pairs = true;
        else if (s == "--ref-stream") ref_stream = true;
        else if (s == "--bench-ref") bench_ref = atoi(val());
        else if (s == "--chunk-bytes") chunk_bytes = atoll(val());
        else if (s == "--sort") sort = true;
        else if (s == "--md") md = true;
        else if (s == "--bam") bam = true;
        else if (s == "--bai") bai = true;
        else if (s == "--bam-level") {
            const std::string v = val();
            if (v != "0" && v != "1") usage();
            bam_level = v == "1" ? ASM_BGZF_DEFLATE : ASM_BGZF_STORED;
        }
        else if (s == "--mapq") {
            const std::string m = val();
            if (m != "reference" && m != "gap") usage();
            mapq_model = m == "gap" ? ASM_MAPQ_GAP : ASM_MAPQ_REFERENCE;
        }
        else if (s == "--sort-mem") {
            if ((sort_mem = atoll(val())) < 0) usage();
        }
        else usage();
    }
    if (ref_path.empty() || (read_path.empty() && bench_ref < 1) || chunk < 1 || all_hits < 0 || (strata >= 0 && !all_hits)) usage();
    const bool paired = !read2_path.empty();
    if (chunk_bytes < 0 || (chunk_bytes > 0 && !stream && !stream_pairs) || (stream && paired)) usage(); /* paired: --stream-pairs */
    if (stream_pairs && (!paired || all_hits || stream)) usage(); /* secondary pairs from files: not there */
    if (bam && !stream && !stream_pairs) {
        fprintf(stderr, "asm-map: --bam needs --stream or --stream-pairs (the library writes BAM from the streamed modes only)\n");
        usage();
    }
    if (bai && (!bam || !sort || (!stream && !stream_pairs))) {
        fprintf(stderr, "asm-map: --bai needs --bam --sort with --stream or --stream-pairs (the index is of a sorted BAM file the library writes)\n");
        usage();
    }
    if (bam_level >= 0 && !bam) {
        fprintf(stderr, "asm-map: --bam-level needs --bam (the level is the BAM container's)\n");
        usage();
    }
    if (sort_mem >= 0 && (!sort || (!stream && !stream_pairs))) usage(); /* --sort-mem: the device-side sort's */
    if (paired && (pp.min_insert < 0 || pp.max_insert < 0)) usage(); /* paired: --insert needed */
    if (!paired && (pp.min_insert >= 0 || pp.rescue_errors >= 0)) usage();
    if (paired) p.both_strands = 1;
    if (strata < 0) strata = paired ? 2 * p.max_errors : p.max_errors; /* paired: strata on the d sum of a pair */
    const int slots = all_hits ? all_hits : 1; /* records per read in the library's output */

    if (bench_ref > 0) return bench_reference(ref_path, k, bench_ref);
    std::vector<std::string> names;
    std::vector<uint64_t> off(1, 0);
    std::string text;
    if (!ref_stream && !parse_reference(ref_path, names, off, text)) return 1;
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
    if (stream && reads.fasta) {
        fprintf(stderr, "asm-map: --stream needs FASTQ reads\n");
        return 1;
    }
    if (stream_pairs) { /* both files must be FASTQ */
        bool fasta2 = false;
        if (FILE* f2 = fopen(read2_path.c_str(), "r")) {
            fasta2 = fgetc(f2) == '>';
            fclose(f2);
        } else {
            fprintf(stderr, "asm-map: cannot open %s\n", read2_path.c_str());
            return 1;
        }
        if (reads.fasta || fasta2) {
            fprintf(stderr, "asm-map: --stream-pairs needs FASTQ reads\n");
            return 1;
        }
    }
    const bool library_writes = stream || stream_pairs;
    /* the modes below write their lines to `out`: the file itself, or with --sort a buffer that finish_output sorts into the file */
    FILE* file = library_writes ? nullptr : fopen(out_path.c_str(), "w");
    char* held = nullptr;
    size_t held_bytes = 0;
    FILE* out = sort && file ? open_memstream(&held, &held_bytes) : file;
    if (!out && !library_writes) {
        fprintf(stderr, "asm-map: cannot write %s\n", out_path.c_str());
        return 1;
    }
    auto finish_output = [&](int rc) {
        fclose(out);
        if (!sort) return rc;
        if (!rc && !write_sorted(file, held, held_bytes, names)) {
            fprintf(stderr, "asm-map: writing %s failed\n", out_path.c_str());
            rc = 1;
        }
        free(held);
        fclose(file);
        return rc;
    };
    asm_handle* h = nullptr;
    asm_index* ix = nullptr;
    int rc = asm_create(&h, 0);
    if (!rc) rc = asm_map_set_mapq_model(h, mapq_model);
    if (!rc && md && (stream || stream_pairs)) rc = asm_map_set_sam_tags(h, ASM_SAM_TAG_MD);
    if (!rc && bam) rc = asm_map_set_output_format(h, ASM_OUT_BAM);
    if (!rc && bam_level >= 0) rc = asm_map_set_bgzf_level(h, bam_level);
    if (!rc && bai) rc = asm_map_set_bam_index(h, ASM_BAM_INDEX_BAI);
    if (!rc)
        rc = ref_stream ? asm_index_build_file(h, ref_path.c_str(), k, 0, &ix, nullptr)
                        : asm_index_build(h, text.data(), off.data(), (int32_t)names.size(), k, &ix);
    if (rc) {
        fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
        return 1;
    }
    if (ref_stream) /* the index knows its sequences */
        for (int32_t r = 0; r < asm_index_n_seqs(ix); r++) {
            names.push_back(asm_index_seq_name(ix, r));
            off.push_back(off.back() + asm_index_seq_len(ix, r));
        }
    std::string header = sort ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unsorted\n";
    for (size_t r = 0; r < names.size(); r++)
        header += "@SQ\tSN:" + names[r] + "\tLN:" + std::to_string((unsigned long long)(off[r + 1] - off[r])) + "\n";
    header += std::string("@PG\tID:asm-map\tPN:asm-map\tVN:") + asm_version() + "\tCL:" + cl + "\n";
    if (stream) { /* the library reads, maps, formats and writes */
        fclose(rf);
        std::vector<const char*> name_ptr;
        for (const std::string& nm : names) name_ptr.push_back(nm.c_str());
        asm_map_file_stats st;
        asm_sam_sort_stats sst;
        rc = sort ? asm_map_file_sorted(h, ix, name_ptr.data(), read_path.c_str(), out_path.c_str(), header.c_str(), &p, all_hits, strata,
                                        chunk_bytes, sort_mem < 0 ? 0 : sort_mem, &st, &sst)
                  : asm_map_file(h, ix, name_ptr.data(), read_path.c_str(), out_path.c_str(), header.c_str(), &p, all_hits, strata,
                                 chunk_bytes, &st);
        if (rc) fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
        asm_index_free(h, ix);
        asm_bam_index_stats ist = {};
        if (!rc && bai) (void)asm_map_last_bam_index(h, &ist);
        asm_destroy(h);
        if (rc) return 1;
        if (bai) report_index(ist);
        fprintf(stderr, "asm-map: %lld reads, %lld mapped, %lld longer than %d (unmapped)\n", (long long)st.reads, (long long)st.mapped,
                (long long)st.too_long, ASM_MAP_MAX_READ);
        report_streamed(st);
        if (sort) report_sorted(sst);
        return 0;
    }
    if (stream_pairs) { /* the library reads both files, pairs, maps, formats and writes */
        fclose(rf);
        std::vector<const char*> name_ptr;
        for (const std::string& nm : names) name_ptr.push_back(nm.c_str());
        asm_map_pairs_file_stats st;
        asm_sam_sort_stats sst;
        rc = sort ? asm_map_pairs_file_sorted(h, ix, name_ptr.data(), read_path.c_str(), read2_path.c_str(), out_path.c_str(),
                                              header.c_str(), &p, &pp, chunk_bytes, sort_mem < 0 ? 0 : sort_mem, &st, &sst)
                  : asm_map_pairs_file(h, ix, name_ptr.data(), read_path.c_str(), read2_path.c_str(), out_path.c_str(), header.c_str(), &p,
                                       &pp, chunk_bytes, &st);
        if (rc) fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
        asm_index_free(h, ix);
        asm_bam_index_stats ist = {};
        if (!rc && bai) (void)asm_map_last_bam_index(h, &ist);
        asm_destroy(h);
        if (rc) return 1;
        if (bai) report_index(ist);
        fprintf(stderr, "asm-map: %lld pairs, %lld proper, %lld mates rescued\n", (long long)st.pairs, (long long)st.proper,
                (long long)st.rescued);
        report_streamed(st);
        if (sort) report_sorted(sst);
        return 0;
    }
    fputs(header.c_str(), file);
    if (md && ref_stream) { /* the index holds the only copy of the text */
        text.resize((size_t)off.back());
        if (asm_index_get_text(h, ix, 0, off.back(), &text[0])) {
            fprintf(stderr, "asm-map: %s\n", asm_last_error(h));
            return 1;
        }
    }
    const MdSource mds = {md, &text, &off};
    if (paired) {
        FILE* rf2 = fopen(read2_path.c_str(), "r");
        if (!rf2) {
            fprintf(stderr, "asm-map: cannot open %s\n", read2_path.c_str());
            return 1;
        }
        ReadFile reads2;
        reads2.f = rf2;
        {
            int c = fgetc(rf2);
            reads2.fasta = c == '>';
            if (c != EOF) ungetc(c, rf2);
        }
        rc = finish_output(write_pairs(out, h, ix, names, reads, reads2, p, pp, chunk, all_hits, strata, mds));
        fclose(rf);
        fclose(rf2);
        asm_index_free(h, ix);
        asm_destroy(h);
        return rc;
    }

    const int cap = 64;
    std::vector<Record> recs;
    std::vector<char> buf;
    std::vector<uint32_t> ro;
    std::vector<int64_t> slot; /* record -> index in the library call, -1 = not sent (too long) */
    std::vector<asm_map_hit> hits;
    std::vector<uint16_t> ops;
    std::vector<uint8_t> nops, mq;
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
        mq.assign((size_t)(n + 1) * slots, 0);
        if (!rc) rc = asm_map_last_mapq(h, mq.data(), n * slots);
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
                const int mapq = mq[o];
                fprintf(out, "%s\t%d\t%s\t%u\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tXG:i:%d%s", rec.name.c_str(),
                        (hr.strand ? 16 : 0) | (t ? 256 : 0), names[(size_t)hr.seq_id].c_str(), hr.pos + 1, mapq, cigar,
                        t ? "*" : seq.c_str(), t || qual.empty() ? "*" : qual.c_str(), (int)hr.dist, hr.greedy_cost,
                        mds.tag(hr, &ops[o * cap], nn, cap, rec.seq).c_str());
                if (all_hits) fprintf(out, "\tNH:i:%u\tHI:i:%u\tXH:i:%u", nrep, t + 1, nh);
                fputc('\n', out);
            }
        }
    }
    rc = finish_output(0);
    fclose(rf);
    asm_index_free(h, ix);
    asm_destroy(h);
    fprintf(stderr, "asm-map: %lld reads, %lld mapped, %lld longer than %d (unmapped)\n", n_total, n_mapped, n_long, ASM_MAP_MAX_READ);
    return rc;
}
