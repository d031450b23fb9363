// tests/adapter_shim/adapter_local_map_main.cpp — TEST INFRASTRUCTURE.  Tracking::UpdateLocalMap of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_LOCAL_MAP)
// executed on stand-in classes that hold what the adapter reads.  Same input as the fixture generator's driver (tools/local_map_golden/ref_local_map_main.cpp; the
// int32 stream of tests/local_map_cases.py frame_stream): one map and one frame.  The key frames live in one array, key frame k at position kf_rank[k], so pointer
// order is the case's rank; Map::GetAllKeyFrames() hands them out in id order.
//   adapter_local_map <in.bin> <out.bin>
// out.bin (int32): n, the local key frames; mpReferenceKF, mCurrentFrame.mpReferenceKF (-1 = NULL); n, the local points; n, the local lines; the frame's map points.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
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
class MapLine {
public:
    bool bad = false;
    bool isBad() { return bad; }
};
class KeyFrame {
public:
    bool bad = false;
    std::vector<KeyFrame*> covisible;
    std::set<KeyFrame*> children;
    KeyFrame* parent = NULL;
    std::vector<MapPoint*> points;
    std::vector<MapLine*> lines;
    bool isBad() { return bad; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        return (int)covisible.size() < N ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
    }
    std::set<KeyFrame*> GetChilds() { return children; }
    KeyFrame* GetParent() { return parent; }
    std::vector<MapPoint*> GetMapPointMatches() { return points; }
    std::vector<MapLine*> GetMapLineMatches() { return lines; }
};
class Frame {
public:
    int N = 0;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    KeyFrame* mpReferenceKF = NULL;
};
class Map {
public:
    std::vector<KeyFrame*> kfs;
    std::vector<MapPoint*> pts;
    std::vector<MapLine*> mls;
    int reference_sets = 0;
    std::vector<KeyFrame*> GetAllKeyFrames() { return kfs; }
    std::vector<MapPoint*> GetAllMapPoints() { return pts; }
    std::vector<MapLine*> GetAllMapLines() { return mls; }
    void SetReferenceMapPoints(const std::vector<MapPoint*>&) { reference_sets++; }
    void SetReferenceMapLines(const std::vector<MapLine*>&) { reference_sets++; }
};
class Tracking {
public:
    void UpdateLocalMap();
    Frame mCurrentFrame;
    std::vector<KeyFrame*> mvpLocalKeyFrames;
    std::vector<MapPoint*> mvpLocalMapPoints;
    std::vector<MapLine*> mvpLocalMapLines;
    KeyFrame* mpReferenceKF = NULL;
    Map* mpMap = NULL;
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_LOCAL_MAP
#include "planar_adapters.hpp"

using namespace Planar_SLAM;

namespace {
std::vector<int32_t> in;
size_t at = 0;
int32_t next() { if (at >= in.size()) std::exit(4); return in[at++]; }
std::vector<int32_t> take(size_t n) { std::vector<int32_t> v(n); for (size_t i = 0; i < n; i++) v[i] = next(); return v; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END); const long bytes = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    in.resize(bytes / 4);
    if (std::fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    std::fclose(f);
    const int nk = next(), npts = next(), nml = next();
    const std::vector<int32_t> kf_bad = take(nk), kf_rank = take(nk), covis = take((size_t)nk * 10), parent = take(nk);
    std::vector<KeyFrame> store(nk);
    std::vector<MapPoint> pts(npts);
    std::vector<MapLine> mls(nml);
    Map map;
    for (int k = 0; k < nk; k++) map.kfs.push_back(&store[kf_rank[k]]);
    for (int p = 0; p < npts; p++) map.pts.push_back(&pts[p]);
    for (int l = 0; l < nml; l++) map.mls.push_back(&mls[l]);
    std::vector<KeyFrame*>& kf = map.kfs;
    for (int k = 0; k < nk; k++) {
        kf[k]->bad = kf_bad[k] != 0;
        for (int t = 0; t < 10; t++) if (covis[(size_t)k * 10 + t] >= 0) kf[k]->covisible.push_back(kf[covis[(size_t)k * 10 + t]]);
        if (parent[k] >= 0) kf[k]->parent = kf[parent[k]];
    }
    { const std::vector<int32_t> n = take(nk); for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) kf[k]->children.insert(kf[next()]); }
    { const std::vector<int32_t> n = take(nk); for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int p = next(); kf[k]->points.push_back(p < 0 ? NULL : &pts[p]); } }
    { const std::vector<int32_t> n = take(nk); for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int l = next(); kf[k]->lines.push_back(l < 0 ? NULL : &mls[l]); } }
    for (int p = 0; p < npts; p++) pts[p].bad = next() != 0;
    { const std::vector<int32_t> n = take(npts); for (int p = 0; p < npts; p++) for (int i = 0; i < n[p]; i++) pts[p].observations[kf[next()]] = (size_t)i; }
    for (int l = 0; l < nml; l++) mls[l].bad = next() != 0;
    // a bad key frame leaves the reference's map (KeyFrame::SetBadFlag erases it): the adapter must still find a bad parent
    {
        std::vector<KeyFrame*> kept;
        for (int k = 0; k < nk; k++) if (!kf_bad[k]) kept.push_back(kf[k]);
        std::vector<KeyFrame*> all = kf;
        map.kfs = kept;
        Tracking tr;
        tr.mpMap = &map;
        const int N = next();
        tr.mCurrentFrame.N = N;
        for (int i = 0; i < N; i++) { const int p = next(); tr.mCurrentFrame.mvpMapPoints.push_back(p < 0 ? NULL : &pts[p]); }
        const int NL = next();
        for (int i = 0; i < NL; i++) { const int l = next(); tr.mCurrentFrame.mvpMapLines.push_back(l < 0 ? NULL : &mls[l]); }
        const int nin = next();
        for (int i = 0; i < nin; i++) tr.mvpLocalKeyFrames.push_back(all[next()]);
        tr.UpdateLocalMap();
        if (map.reference_sets != 2) return 3;
        std::vector<int32_t> id_at(nk), out;
        for (int k = 0; k < nk; k++) id_at[kf_rank[k]] = k;
        out.push_back((int32_t)tr.mvpLocalKeyFrames.size());
        for (KeyFrame* p : tr.mvpLocalKeyFrames) out.push_back(id_at[p - store.data()]);
        out.push_back(tr.mpReferenceKF ? id_at[tr.mpReferenceKF - store.data()] : -1);
        out.push_back(tr.mCurrentFrame.mpReferenceKF ? id_at[tr.mCurrentFrame.mpReferenceKF - store.data()] : -1);
        out.push_back((int32_t)tr.mvpLocalMapPoints.size());
        for (MapPoint* p : tr.mvpLocalMapPoints) out.push_back((int32_t)(p - pts.data()));
        out.push_back((int32_t)tr.mvpLocalMapLines.size());
        for (MapLine* p : tr.mvpLocalMapLines) out.push_back((int32_t)(p - mls.data()));
        for (MapPoint* p : tr.mCurrentFrame.mvpMapPoints) out.push_back(p ? (int32_t)(p - pts.data()) : -1);
        f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
        std::fclose(f);
    }
    return 0;
}
