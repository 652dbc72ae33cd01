// Test-only brute force of asm_map_reads_all (docs/design/mapper.md, "All hits"): for every strand s and sequence r, a plain
// semi-global DP under the mapper's byte rule gives D(j) = min_i Lev(q_s, T_r[i, j)) at every end j (Ukkonen's cut-off: rows
// above e are not computed, which keeps D exact wherever D <= e).  A locus is a maximal run of consecutive ends with D <= e; its
// d is the run's minimum, its j the smallest end reaching d, its i the largest start with Lev(q_s, T_r[i, j)) = d (reversed DP).
//   map_bf_all(text, seq_off, n_seqs, read, m, e, both, out, cap) -> number of loci; the first min(that, cap) are written to
//   out[5 * t ..] = {s, r, i, j, d}, sorted by (d, s, r, j).
#include <stdint.h>

#include <algorithm>
#include <array>
#include <string>
#include <vector>

static bool is_base(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
static char upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
static char comp(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
static int sub(char a, char b) { return (a == b && is_base(a)) ? 0 : 1; }

/* the largest start i with Lev(q, T[i, j)) = d: a plain DP over the reversed strings, the first length reaching d */
static int64_t start_of(const std::string& q, const char* t, int64_t j, int d) {
    const int m = (int)q.size();
    const int64_t lo = std::max<int64_t>(0, j - m - d);
    std::vector<int> P(m + 1), Q(m + 1);
    for (int i = 0; i <= m; i++) P[i] = i;
    for (int64_t L = 1; L <= j - lo; L++) {
        const char tc = upper(t[j - L]);
        Q[0] = (int)L;
        for (int i = 1; i <= m; i++) Q[i] = std::min({P[i - 1] + sub(q[m - i], tc), P[i] + 1, Q[i - 1] + 1});
        std::swap(P, Q);
        if (P[m] == d) return j - L;
    }
    return -1;
}

extern "C" int map_bf_all(const char* text, const uint64_t* seq_off, int n_seqs, const char* read, int m, int e, int both, int32_t* out,
                          int cap) {
    std::string q0(read, read + m);
    for (char& c : q0) c = upper(c);
    std::string q1(q0.rbegin(), q0.rend());
    for (char& c : q1) c = comp(c);
    const int INF = e + 1;
    std::vector<std::array<int64_t, 5>> loci; /* d, s, r, j, i */
    std::vector<int> C(m + 1), N(m + 1);
    for (int s = 0; s < (both ? 2 : 1); s++) {
        const std::string& q = s ? q1 : q0;
        for (int r = 0; r < n_seqs; r++) {
            const int64_t s0 = (int64_t)seq_off[r], len = (int64_t)seq_off[r + 1] - s0;
            for (int i = 0; i <= m; i++) C[i] = std::min(i, INF);
            int top = std::min(m, e), touchedC = m, touchedN = m; /* rows > top hold INF; touched*: the highest row written */
            for (int i = 0; i <= m; i++) N[i] = INF;
            int run_d = INF;   /* the open run's minimum (INF: no run open) */
            int64_t run_j = 0; /* its smallest end reaching run_d */
            for (int64_t t = 0; t <= len; t++) {
                int d = INF;
                if (t < len) {
                    const char tc = upper(text[s0 + t]);
                    N[0] = 0;
                    int i = 1;
                    const int lim = std::min(m, top + 1);
                    for (; i <= lim; i++) N[i] = std::min({C[i - 1] + sub(q[i - 1], tc), C[i] + 1, N[i - 1] + 1, INF});
                    for (; i <= m && N[i - 1] < INF; i++) N[i] = std::min({C[i - 1] + sub(q[i - 1], tc), C[i] + 1, N[i - 1] + 1, INF});
                    const int last = i - 1;
                    for (int z = last + 1; z <= touchedN; z++) N[z] = INF;
                    touchedN = last;
                    top = last;
                    while (top > 0 && N[top] >= INF) top--;
                    d = last == m ? N[m] : INF;
                    std::swap(C, N);
                    std::swap(touchedC, touchedN);
                }
                if (d <= e) { /* end t + 1 is a hit end */
                    if (d < run_d) run_d = d, run_j = t + 1;
                } else if (run_d <= e) { /* the run closes (also at the sequence's end) */
                    loci.push_back({run_d, s, r, run_j, start_of(q, text + s0, run_j, run_d)});
                    run_d = INF;
                }
            }
        }
    }
    std::sort(loci.begin(), loci.end(), [](const std::array<int64_t, 5>& a, const std::array<int64_t, 5>& b) {
        return a[0] != b[0] ? a[0] < b[0] : a[1] != b[1] ? a[1] < b[1] : a[2] != b[2] ? a[2] < b[2] : a[3] < b[3];
    });
    for (size_t t = 0; t < loci.size() && (int64_t)t < cap; t++) {
        int32_t* o = out + 5 * t;
        o[0] = (int32_t)loci[t][1], o[1] = (int32_t)loci[t][2], o[2] = (int32_t)loci[t][4], o[3] = (int32_t)loci[t][3];
        o[4] = (int32_t)loci[t][0];
    }
    return (int)loci.size();
}
