// Driver of tools/gen_golden_connections.py: builds the stand-in key frames and map points of one case from the int32 stream tests/connections_cases.py::stream
// writes, calls the reference's KeyFrame::UpdateConnections (compiled from the real lines ahead of this file) on the listed key frames in order and writes the
// connection state of every key frame as int32.  The key frames of a map live in ONE array and key frame k sits at position kf_rank[k], so pointer order - the
// order of std::map<KeyFrame*, int> and of the sort on pair<int, KeyFrame*> - is the case's rank.
//   ref_connections in.bin out.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace Planar_SLAM;

static std::vector<int32_t> in;
static size_t at = 0;
static int32_t next() { if (at >= in.size()) { fprintf(stderr, "short input\n"); exit(2); } return in[at++]; }
static std::vector<int32_t> take(size_t n) { std::vector<int32_t> v(n); for (size_t i = 0; i < n; i++) v[i] = next(); return v; }

struct OneMap {
    int nk = 0, npts = 0;
    std::unique_ptr<KeyFrame[]> store;
    std::vector<MapPoint> pts;
    std::vector<KeyFrame*> kf;
    std::vector<int32_t> id_at;      // array position -> key-frame id
    int id(KeyFrame* p) const { return p ? id_at[p - store.get()] : -1; }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    in.resize(bytes / 4);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);

    const int G = next();
    std::vector<OneMap> maps(G);
    for (OneMap& m : maps) {
        m.nk = next(); m.npts = next();
        const int nk = m.nk;
        const std::vector<int32_t> rank = take(nk), mnid = take(nk), first = take(nk), parent = take(nk);
        m.store.reset(new KeyFrame[nk]);
        m.pts.resize(m.npts);
        m.kf.resize(nk); m.id_at.resize(nk);
        for (int k = 0; k < nk; k++) { m.kf[k] = &m.store[rank[k]]; m.id_at[rank[k]] = k; }
        for (int k = 0; k < nk; k++) {
            m.kf[k]->mnId = (long unsigned int)mnid[k];
            m.kf[k]->mbFirstConnection = first[k] != 0;
            m.kf[k]->mpParent = parent[k] >= 0 ? m.kf[parent[k]] : NULL;
        }
        {
            const std::vector<int32_t> n = take(nk);
            for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int p = next(); m.kf[k]->mvpMapPoints.push_back(p < 0 ? NULL : &m.pts[p]); }
        }
        for (int p = 0; p < m.npts; p++) m.pts[p].bad = next() != 0;
        {
            const std::vector<int32_t> n = take(m.npts);
            for (int p = 0; p < m.npts; p++) for (int i = 0; i < n[p]; i++) m.pts[p].observations[m.kf[next()]] = (size_t)i;
        }
        {
            const std::vector<int32_t> n = take(nk);
            for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int o = next(), w = next(); m.kf[k]->mConnectedKeyFrameWeights[m.kf[o]] = w; }
        }
        {
            const std::vector<int32_t> n = take(nk);
            for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) {
                const int o = next(), w = next();
                m.kf[k]->mvpOrderedConnectedKeyFrames.push_back(m.kf[o]); m.kf[k]->mvOrderedWeights.push_back(w);
            }
        }
    }
    const int L = next();
    std::vector<int32_t> new_parent(L, -1);
    for (int l = 0; l < L; l++) {
        const int g = next(), j = next();
        KeyFrame* kf = maps[g].kf[j];
        const bool was_first = kf->mbFirstConnection;
        kf->UpdateConnections();
        if (was_first && !kf->mbFirstConnection) new_parent[l] = maps[g].id(kf->mpParent);
    }
    if (at != in.size()) { fprintf(stderr, "long input\n"); return 2; }

    std::vector<int32_t> out;
    for (OneMap& m : maps)
        for (int k = 0; k < m.nk; k++) {
            KeyFrame* kf = m.kf[k];
            out.push_back((int32_t)kf->mConnectedKeyFrameWeights.size());
            for (auto& e : kf->mConnectedKeyFrameWeights) { out.push_back(m.id(e.first)); out.push_back(e.second); }
            out.push_back((int32_t)kf->mvpOrderedConnectedKeyFrames.size());
            if (kf->mvpOrderedConnectedKeyFrames.size() != kf->mvOrderedWeights.size()) return 3;
            for (KeyFrame* p : kf->mvpOrderedConnectedKeyFrames) out.push_back(m.id(p));
            for (int w : kf->mvOrderedWeights) out.push_back(w);
            out.push_back(m.id(kf->mpParent));
            out.push_back(kf->mbFirstConnection);
            out.push_back((int32_t)kf->mspChildrens.size());
            for (KeyFrame* p : kf->mspChildrens) out.push_back(m.id(p));
        }
    for (int32_t p : new_parent) out.push_back(p);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
