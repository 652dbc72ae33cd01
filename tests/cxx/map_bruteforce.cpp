// Test-only brute-force read mapper: scans every sequence and strand with a plain semi-global DP under the mapper's byte rule
// (A, C, G, T match only themselves; every other byte mismatches everything) and applies the tie order of
// docs/design/mapper.md.  No index, no pigeonhole.  Ukkonen's cut-off (rows whose value exceeds e are not computed) keeps it
// exact for d <= e.
//   map_bf(text, seq_off, n_seqs, read, m, e, both, out) -> out = {mapped, s, r, i, j, d}
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

static bool is_base(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
static char upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
static char comp(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
static int sub(char a, char b) { return (a == b && is_base(a)) ? 0 : 1; }

extern "C" int map_bf(const char* text, const uint64_t* seq_off, int n_seqs, const char* read, int m, int e, int both, int32_t* out) {
    std::string q0(read, read + m);
    for (char& c : q0) c = upper(c);
    std::string q1(q0.rbegin(), q0.rend());
    for (char& c : q1) c = comp(c);
    const int INF = e + 1;
    int best_d = INF, best_s = -1, best_r = -1;
    int64_t best_j = -1;
    std::vector<int> C(m + 1), N(m + 1);
    for (int s = 0; s < (both ? 2 : 1); s++) {
        const std::string& q = s ? q1 : q0;
        for (int r = 0; r < n_seqs; r++) {
            const int64_t s0 = (int64_t)seq_off[r], len = (int64_t)seq_off[r + 1] - s0;
            for (int i = 0; i <= m; i++) C[i] = std::min(i, INF);
            int touchedC = m, top = std::min(m, e);  /* rows > top hold INF */
            int touchedN = m;
            for (int i = 0; i <= m; i++) N[i] = INF;
            for (int64_t t = 0; t < len; t++) {
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
                const int d = last == m ? N[m] : INF;
                if (d < best_d) best_d = d, best_s = s, best_r = r, best_j = t + 1;
                std::swap(C, N);
                std::swap(touchedC, touchedN);
            }
        }
    }
    out[0] = 0, out[1] = out[2] = out[3] = out[4] = out[5] = -1;
    if (best_d > e) return 0;
    /* start: the largest i with Lev(q_s, T[i, j)) = d, by a plain DP over the reversed strings */
    const std::string& q = best_s ? q1 : q0;
    const int64_t s0 = (int64_t)seq_off[best_r], j = best_j, lo = std::max<int64_t>(0, j - m - best_d);
    std::vector<int> P(m + 1), Q(m + 1);
    for (int i = 0; i <= m; i++) P[i] = i;
    int64_t start = -1;
    for (int64_t L = 1; L <= j - lo; L++) {
        const char tc = upper(text[s0 + j - L]);
        Q[0] = (int)L;
        for (int i = 1; i <= m; i++) Q[i] = std::min({P[i - 1] + sub(q[m - i], tc), P[i] + 1, Q[i - 1] + 1});
        std::swap(P, Q);
        if (P[m] == best_d) {
            start = j - L;
            break;
        }
    }
    out[0] = 1, out[1] = best_s, out[2] = best_r, out[3] = (int32_t)start, out[4] = (int32_t)j, out[5] = best_d;
    return 0;
}
