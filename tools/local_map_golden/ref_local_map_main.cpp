// Driver of tools/gen_golden_local_map.py: builds the stand-in objects of one frame from the int32 stream tests/local_map_cases.py::frame_stream writes, runs the
// reference's Tracking::UpdateLocalMap, SearchLocalPoints and SearchLocalLines (compiled from the real lines ahead of this file) and writes the lists as int32.
// The key frames live in ONE array and key frame k sits at position kf_rank[k], so pointer order - the order of std::map<KeyFrame*, int> and of the children's
// std::set<KeyFrame*> - is the case's rank.
//   ref_local_map in.bin out.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>

using namespace Planar_SLAM;

static std::vector<int32_t> in;
static size_t at = 0;
static int32_t next() { if (at >= in.size()) { fprintf(stderr, "short input\n"); exit(2); } return in[at++]; }
static std::vector<int32_t> take(size_t n) { std::vector<int32_t> v(n); for (size_t i = 0; i < n; i++) v[i] = next(); return v; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    in.resize(bytes / 4);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);

    const int nk = next(), npts = next(), nml = next();
    const std::vector<int32_t> kf_bad = take(nk), kf_rank = take(nk), covis = take((size_t)nk * 10), parent = take(nk);
    std::vector<KeyFrame> store(nk);
    std::vector<MapPoint> pts(npts);
    std::vector<MapLine> mls(nml);
    std::vector<KeyFrame*> kf(nk);
    for (int k = 0; k < nk; k++) kf[k] = &store[kf_rank[k]];
    for (int k = 0; k < nk; k++) {
        kf[k]->bad = kf_bad[k] != 0;
        // a -1 entry is skipped: a vector<KeyFrame*> has no holes, and where the -1 stood does not change which entry comes first
        for (int t = 0; t < 10; t++) if (covis[(size_t)k * 10 + t] >= 0) kf[k]->covisible.push_back(kf[covis[(size_t)k * 10 + t]]);
        if (parent[k] >= 0) kf[k]->parent = kf[parent[k]];
    }
    {
        const std::vector<int32_t> n = take(nk);
        for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) kf[k]->children.insert(kf[next()]);
    }
    {
        const std::vector<int32_t> n = take(nk);
        for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int p = next(); kf[k]->points.push_back(p < 0 ? NULL : &pts[p]); }
    }
    {
        const std::vector<int32_t> n = take(nk);
        for (int k = 0; k < nk; k++) for (int i = 0; i < n[k]; i++) { const int l = next(); kf[k]->lines.push_back(l < 0 ? NULL : &mls[l]); }
    }
    for (int p = 0; p < npts; p++) pts[p].bad = next() != 0;
    {
        const std::vector<int32_t> n = take(npts);
        for (int p = 0; p < npts; p++) for (int i = 0; i < n[p]; i++) pts[p].observations[kf[next()]] = (size_t)i;
    }
    for (int l = 0; l < nml; l++) mls[l].bad = next() != 0;

    Map map;
    Tracking tr;
    tr.mpMap = &map;
    tr.mCurrentFrame.mnId = 7;
    tr.mnLastRelocFrameId = 0;
    const int N = next();
    tr.mCurrentFrame.N = N;
    for (int i = 0; i < N; i++) { const int p = next(); tr.mCurrentFrame.mvpMapPoints.push_back(p < 0 ? NULL : &pts[p]); }
    const int NL = next();
    for (int i = 0; i < NL; i++) { const int l = next(); tr.mCurrentFrame.mvpMapLines.push_back(l < 0 ? NULL : &mls[l]); }
    const int nin = next();
    for (int i = 0; i < nin; i++) tr.mvpLocalKeyFrames.push_back(kf[next()]);

    tr.UpdateLocalMap();
    tr.SearchLocalPoints();
    tr.SearchLocalLines();

    std::vector<int32_t> out;
    std::vector<int32_t> id_at(nk);                       // array position -> key-frame id
    for (int k = 0; k < nk; k++) id_at[kf_rank[k]] = k;
    out.push_back((int32_t)tr.mvpLocalKeyFrames.size());
    for (KeyFrame* p : tr.mvpLocalKeyFrames) out.push_back(id_at[p - store.data()]);
    out.push_back(tr.mpReferenceKF ? id_at[tr.mpReferenceKF - store.data()] : -1);
    out.push_back(tr.mCurrentFrame.mpReferenceKF ? id_at[tr.mCurrentFrame.mpReferenceKF - store.data()] : -1);
    out.push_back((int32_t)tr.mvpLocalMapPoints.size());
    for (MapPoint* p : tr.mvpLocalMapPoints) out.push_back((int32_t)(p - pts.data()));
    for (MapPoint* p : tr.mvpLocalMapPoints) out.push_back(p->mnLastFrameSeen == tr.mCurrentFrame.mnId);
    out.push_back((int32_t)tr.mvpLocalMapLines.size());
    for (MapLine* p : tr.mvpLocalMapLines) out.push_back((int32_t)(p - mls.data()));
    for (MapLine* p : tr.mvpLocalMapLines) out.push_back(p->mnLastFrameSeen == tr.mCurrentFrame.mnId);
    for (MapPoint* p : tr.mCurrentFrame.mvpMapPoints) out.push_back(p ? (int32_t)(p - pts.data()) : -1);
    for (MapLine* p : tr.mCurrentFrame.mvpMapLines) out.push_back(p ? (int32_t)(p - mls.data()) : -1);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
