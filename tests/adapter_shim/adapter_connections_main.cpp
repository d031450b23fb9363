// tests/adapter_shim/adapter_connections_main.cpp — TEST INFRASTRUCTURE.  KeyFrame::UpdateConnections of include/planar_adapters.hpp
// (PLANAR_ADAPTERS_WITH_CONNECTIONS) executed on stand-in classes that hold what the adapter reads.  Same input and output as the fixture generator's driver
// (tools/connections_golden/ref_connections_main.cpp; the int32 stream of tests/connections_cases.py stream): the maps of a case and its list, run in order.
// The key frames of a map live in one array, key frame k at position kf_rank[k], so pointer order is the case's rank.  AddConnection and AddChild are the
// stand-in's own statement of what the reference's do.
//   adapter_connections <in.bin> <out.bin>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>

namespace Planar_SLAM {
class KeyFrame;
class MapPoint {
public:
    bool bad = false;
    std::map<KeyFrame*, size_t> observations;
    bool isBad() { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() { return observations; }
};
class KeyFrame {
public:
    void UpdateConnections();
    // a changed or new weight re-lists the whole row by (weight, pointer), largest first; an unchanged one does nothing
    void AddConnection(KeyFrame* pKF, const int& weight) {
        std::unique_lock<std::mutex> lock(mMutexConnections);
        auto it = mConnectedKeyFrameWeights.find(pKF);
        if (it != mConnectedKeyFrameWeights.end() && it->second == weight) return;
        mConnectedKeyFrameWeights[pKF] = weight;
        std::vector<std::pair<int, KeyFrame*>> v;
        for (const auto& kv : mConnectedKeyFrameWeights) v.push_back(std::make_pair(kv.second, kv.first));
        std::sort(v.begin(), v.end());
        std::reverse(v.begin(), v.end());
        mvpOrderedConnectedKeyFrames.clear(); mvOrderedWeights.clear();
        for (const auto& e : v) { mvpOrderedConnectedKeyFrames.push_back(e.second); mvOrderedWeights.push_back(e.first); }
    }
    void AddChild(KeyFrame* pKF) {
        std::unique_lock<std::mutex> lock(mMutexConnections);
        mspChildrens.insert(pKF);
    }
    long unsigned int mnId = 0;
    std::vector<MapPoint*> mvpMapPoints;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true;
    KeyFrame* mpParent = NULL;
    std::set<KeyFrame*> mspChildrens;
    std::mutex mMutexConnections, mMutexFeatures;
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_CONNECTIONS
#include "planar_adapters.hpp"

using namespace Planar_SLAM;

namespace {
std::vector<int32_t> in;
size_t at = 0;
int32_t next() { if (at >= in.size()) std::exit(4); return in[at++]; }
std::vector<int32_t> take(size_t n) { std::vector<int32_t> v(n); for (size_t i = 0; i < n; i++) v[i] = next(); return v; }

struct OneMap {
    int nk = 0, npts = 0;
    std::unique_ptr<KeyFrame[]> store;
    std::vector<MapPoint> pts;
    std::vector<KeyFrame*> kf;
    std::vector<int32_t> id_at;      // array position -> key-frame id
    int id(KeyFrame* p) const { return p ? id_at[p - store.get()] : -1; }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END); const long bytes = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    in.resize(bytes / 4);
    if (std::fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    std::fclose(f);
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
        { const std::vector<int32_t> n = take(nk); for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int p = next(); m.kf[k]->mvpMapPoints.push_back(p < 0 ? NULL : &m.pts[p]); } }
        for (int p = 0; p < m.npts; p++) m.pts[p].bad = next() != 0;
        { const std::vector<int32_t> n = take(m.npts); for (int p = 0; p < m.npts; p++) for (int i = 0; i < n[p]; i++) m.pts[p].observations[m.kf[next()]] = (size_t)i; }
        { const std::vector<int32_t> n = take(nk); for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int o = next(), w = next(); m.kf[k]->mConnectedKeyFrameWeights[m.kf[o]] = w; } }
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
    if (at != in.size()) return 4;
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
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
