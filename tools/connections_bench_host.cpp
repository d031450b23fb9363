// tools/connections_bench_host.cpp — the host side of tools/connections_bench.py: KeyFrame::UpdateConnections restated over the arrays of one map of
// planar_local_map / planar_covis_graph, run over a list in order by ONE thread (compiled -O2 by the tool).  The graph starts empty: no weights, every key frame
// unconnected, mnId = index.  Input (int32 stream): S SS PS OC nk npts reps, kf_rank [S], n_slots [S], kf_pts [S][SS], pt_bad [PS], obs_off [PS + 1], obs_kf [OC],
// L, entry_kf [L].  Output (int32 stream): microseconds of each repetition [reps], then conn_w [S][S], ord_n [S], ord_kf [S][S], parent [S] of the last one.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

struct Graph {
    int S;
    std::vector<int32_t> conn, ord_n, ord_kf, ord_w, parent;
    std::vector<uint8_t> first;
    explicit Graph(int s) : S(s), conn((size_t)s * s, 0), ord_n(s, 0), ord_kf((size_t)s * s, -1), ord_w((size_t)s * s, 0), parent(s, -1), first(s, 1) {}
};

static void list_row(Graph& g, const int32_t* rank, const std::vector<int32_t>& byrank, int x, int nk) {
    std::vector<std::pair<int, int>> v;
    for (int k = 0; k < nk; k++)
        if (g.conn[(size_t)x * g.S + k] > 0) v.push_back({g.conn[(size_t)x * g.S + k], rank[k]});
    std::sort(v.begin(), v.end());
    g.ord_n[x] = (int32_t)v.size();
    for (size_t i = 0; i < v.size(); i++) {
        g.ord_kf[(size_t)x * g.S + i] = byrank[v[v.size() - 1 - i].second];
        g.ord_w[(size_t)x * g.S + i] = v[v.size() - 1 - i].first;
    }
}

static void add_connection(Graph& g, const int32_t* rank, const std::vector<int32_t>& byrank, int x, int j, int w, int nk) {
    if (g.conn[(size_t)x * g.S + j] == w) return;
    g.conn[(size_t)x * g.S + j] = w;
    list_row(g, rank, byrank, x, nk);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<int32_t> in(bytes / 4);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    const int32_t* p = in.data();
    const int S = p[0], SS = p[1], PS = p[2], OC = p[3], nk = p[4], reps = p[6];
    p += 7;
    const int32_t* rank = p; p += S;
    const int32_t* n_slots = p; p += S;
    const int32_t* kf_pts = p; p += (size_t)S * SS;
    const int32_t* pt_bad = p; p += PS;
    const int32_t* obs_off = p; p += PS + 1;
    const int32_t* obs_kf = p; p += OC;
    const int L = *p++;
    const int32_t* entry = p;
    std::vector<int32_t> byrank(nk), out;
    for (int k = 0; k < nk; k++) byrank[rank[k]] = k;
    Graph last(S);
    for (int rep = 0; rep < reps; rep++) {
        Graph g(S);
        std::vector<int32_t> counter(S);
        const auto t0 = std::chrono::steady_clock::now();
        for (int l = 0; l < L; l++) {
            const int j = entry[l];
            std::fill(counter.begin(), counter.end(), 0);
            for (int s = 0; s < n_slots[j]; s++) {
                const int pt = kf_pts[(size_t)j * SS + s];
                if (pt < 0 || pt_bad[pt]) continue;
                for (int o = obs_off[pt]; o < obs_off[pt + 1]; o++)
                    if (obs_kf[o] != j) counter[obs_kf[o]]++;
            }
            int nmax = 0, kmax = -1;
            std::vector<std::pair<int, int>> targets;
            for (int r = 0; r < nk; r++) {
                const int k = byrank[r], c = counter[k];
                if (c > nmax) { nmax = c; kmax = k; }
                if (c >= 15) { targets.push_back({c, r}); add_connection(g, rank, byrank, k, j, c, nk); }
            }
            if (kmax < 0) continue;
            if (targets.empty()) { targets.push_back({nmax, rank[kmax]}); add_connection(g, rank, byrank, kmax, j, nmax, nk); }
            std::sort(targets.begin(), targets.end());
            std::copy(counter.begin(), counter.end(), g.conn.begin() + (size_t)j * S);
            g.ord_n[j] = (int32_t)targets.size();
            for (size_t i = 0; i < targets.size(); i++) {
                g.ord_kf[(size_t)j * S + i] = byrank[targets[targets.size() - 1 - i].second];
                g.ord_w[(size_t)j * S + i] = targets[targets.size() - 1 - i].first;
            }
            if (g.first[j] && j != 0) { g.parent[j] = g.ord_kf[(size_t)j * S]; g.first[j] = 0; }
        }
        const auto t1 = std::chrono::steady_clock::now();
        out.push_back((int32_t)std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count());
        if (rep == reps - 1) last = g;
    }
    out.insert(out.end(), last.conn.begin(), last.conn.end());
    out.insert(out.end(), last.ord_n.begin(), last.ord_n.end());
    out.insert(out.end(), last.ord_kf.begin(), last.ord_kf.end());
    out.insert(out.end(), last.parent.begin(), last.parent.end());
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
