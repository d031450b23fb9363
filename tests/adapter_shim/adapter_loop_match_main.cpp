// tests/adapter_shim/adapter_loop_match_main.cpp — TEST INFRASTRUCTURE.  The four ORBmatcher members of include/planar_adapters.hpp
// (PLANAR_ADAPTERS_WITH_LOOP_MATCHERS) executed on stand-in key frames and map points that hold what the adapter reads and accept the edits it makes.  Same input as the
// fixture generator's driver (tools/loop_match_golden/ref_loop_match_main.cpp; written by tests/loop_match_cases.py) and the same output blocks, so the result is
// compared with tests/golden/loop_match_ref.npz.
//   adapter_loop_match <bow|sim3|proj|fuse> <in.bin> <out.bin>
#include <map>
#include <set>
#include <string>

#include "adapter_io.hpp"

namespace Planar_SLAM {
class KeyFrame;
class MapPoint {
public:
    cv::Mat pos, normal, desc;
    bool bad = false;
    float mfMinDistance = 0, mfMaxDistance = 0;
    std::map<KeyFrame*, int> index_in;
    int added_at = -1;
    bool isBad() { return bad; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    cv::Mat GetNormal() { return normal.clone(); }
    cv::Mat GetDescriptor() { return desc.clone(); }
    void GetDistanceRange(float& mn, float& mx) { mn = mfMinDistance; mx = mfMaxDistance; }
    int GetIndexInKeyFrame(KeyFrame* kf) { auto it = index_in.find(kf); return it == index_in.end() ? -1 : it->second; }
    void AddObservation(KeyFrame* kf, size_t i) { added_at = (int)i; index_in[kf] = (int)i; }
};
class KeyFrame {
public:
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors, Tcw;
    std::map<unsigned, std::vector<unsigned>> mFeatVec;
    std::vector<MapPoint*> mps;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mb = 0, mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0,
          mfLogScaleFactor = 0;
    int mnScaleLevels = 0;
    std::vector<float> mvScaleFactors;
    cv::Mat GetPose() { return Tcw.clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mps; }
    std::set<MapPoint*> GetMapPoints() { std::set<MapPoint*> r; for (MapPoint* p : mps) if (p) r.insert(p); return r; }
    MapPoint* GetMapPoint(const size_t& i) { return mps[i]; }
    void AddMapPoint(MapPoint* p, const size_t& i) { mps[i] = p; }
};
class ORBmatcher {
public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12);
    int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12, const cv::Mat& t12, const float th);
    int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th);
    int Fuse(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint);
protected:
    float mfNNratio;
    bool mbCheckOrientation;
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_LOOP_MATCHERS
#include "planar_adapters.hpp"

using namespace Planar_SLAM;
using namespace adapter_io;

namespace {
void set_view(KeyFrame& kf, const KP7* k, int N, const uint8_t* desc, const float* intr, const float* sf, size_t nl) {
    kf.N = N; to_keypoints(k, N, kf.mvKeysUn); kf.mDescriptors = desc_mat(N, desc);
    kf.mnMinX = intr[0]; kf.mnMaxX = intr[1]; kf.mnMinY = intr[2]; kf.mnMaxY = intr[3]; kf.mfGridElementWidthInv = intr[4]; kf.mfGridElementHeightInv = intr[5];
    kf.fx = intr[6]; kf.fy = intr[7]; kf.cx = intr[8]; kf.cy = intr[9]; kf.mfLogScaleFactor = intr[10];
    kf.mnScaleLevels = (int)nl; kf.mvScaleFactors.assign(sf, sf + nl);
    kf.mps.assign(N, nullptr);
}

void fill(KeyFrame& kf, std::vector<MapPoint>& mps, Blocks& in) {
    size_t n, nl;
    const KP7* k = in.get<KP7>(&n);
    const uint8_t* desc = in.get<uint8_t>();
    const float* intr = in.get<float>();
    const float* sf = in.get<float>(&nl);
    const float* Tcw = in.get<float>();
    const uint8_t* usable = in.get<uint8_t>();
    const float *xw = in.get<float>(), *min_d = in.get<float>(), *max_d = in.get<float>();
    const uint8_t* mdesc = in.get<uint8_t>();
    const int N = (int)n;
    set_view(kf, k, N, desc, intr, sf, nl);
    kf.Tcw = mat_f32(4, 4, Tcw);
    mps.assign(N, MapPoint());
    for (int i = 0; i < N; i++) {
        if (!usable[i] && !(i & 1)) continue;   // NULL slot; odd ones become isBad() points instead
        mps[i].bad = !usable[i];
        mps[i].pos = mat_f32(3, 1, xw + 3 * i); mps[i].desc = desc_mat(1, mdesc + 32 * (size_t)i);
        mps[i].mfMinDistance = min_d[i]; mps[i].mfMaxDistance = max_d[i];
        kf.mps[i] = &mps[i];
    }
}

int run_sim3(Blocks& in, FILE* out) {
    const float* prm = in.get<float>();   // {th, s12, R12[9], t12[3]}
    KeyFrame kf1, kf2;
    std::vector<MapPoint> mps1, mps2;
    fill(kf1, mps1, in);
    fill(kf2, mps2, in);
    const int32_t* entry = in.get<int32_t>();
    const int N1 = kf1.N;
    std::vector<MapPoint> before(N1);
    std::vector<MapPoint*> vpMatches12(N1, nullptr);
    for (int i = 0; i < N1; i++)
        if (entry[i] != -1) { before[i].index_in[&kf2] = entry[i]; vpMatches12[i] = &before[i]; }
    ORBmatcher matcher(0.75f, true);
    const float s12 = prm[1];
    const int nFound = matcher.SearchBySim3(&kf1, &kf2, vpMatches12, s12, mat_f32(3, 3, prm + 2), mat_f32(3, 1, prm + 11), prm[0]);
    std::vector<int32_t> match(N1, -1);
    for (int i = 0; i < N1; i++) {
        MapPoint* p = vpMatches12[i];
        if (!p) continue;
        match[i] = p == &before[i] ? entry[i] : (int32_t)(p - mps2.data());
    }
    write_block(out, match.data(), (size_t)N1); write_block(out, &nFound, 1);
    return 0;
}

int run_bow(Blocks& in, FILE* out) {
    const float* prm = in.get<float>();
    KeyFrame kf[2];
    std::vector<MapPoint> mps[2];
    for (int s = 0; s < 2; s++) {
        size_t n;
        const KP7* k = in.get<KP7>(&n);
        const int N = (int)n;
        const uint8_t* desc = in.get<uint8_t>();
        const int32_t* node = in.get<int32_t>();
        const uint8_t* usable = in.get<uint8_t>();
        kf[s].N = N; kf[s].mvKeysUn.resize(N); kf[s].mDescriptors = desc_mat(N, desc);
        mps[s].assign(N, MapPoint()); kf[s].mps.assign(N, nullptr);
        for (int i = 0; i < N; i++) {
            kf[s].mvKeysUn[i] = to_keypoint(k[i]);
            if (node[i] >= 0) kf[s].mFeatVec[(unsigned)node[i]].push_back((unsigned)i);
            if (!usable[i] && !(i & 1)) continue;
            mps[s][i].bad = !usable[i];
            kf[s].mps[i] = &mps[s][i];
        }
    }
    ORBmatcher matcher(prm[0], prm[1] != 0);
    std::vector<MapPoint*> vpMatches12;
    const int nm = matcher.SearchByBoW(&kf[0], &kf[1], vpMatches12);
    std::vector<int32_t> match(kf[0].N, -1);
    for (int i = 0; i < kf[0].N && i < (int)vpMatches12.size(); i++) if (vpMatches12[i]) match[i] = (int32_t)(vpMatches12[i] - mps[1].data());
    write_block(out, match.data(), match.size()); write_block(out, &nm, 1);
    return 0;
}

struct ScwProblem {
    KeyFrame kf;
    std::vector<MapPoint> pts, holders;
    std::vector<MapPoint*> vp;
    const uint8_t *state, *usable, *flag;
    cv::Mat Scw;
    float th;
    int N, NP;
    void load(Blocks& in) {
        th = in.get<float>()[0];
        size_t n, nl, np;
        const KP7* k = in.get<KP7>(&n);
        N = (int)n;
        const uint8_t* desc = in.get<uint8_t>();
        const float* intr = in.get<float>();
        const float* sf = in.get<float>(&nl);
        Scw = mat_f32(4, 4, in.get<float>());
        state = in.get<uint8_t>();
        usable = in.get<uint8_t>(&np);
        NP = (int)np;
        flag = in.get<uint8_t>();
        const float *xw = in.get<float>(), *nrm = in.get<float>(), *min_d = in.get<float>(), *max_d = in.get<float>();
        const uint8_t* pdesc = in.get<uint8_t>();
        set_view(kf, k, N, desc, intr, sf, nl);
        pts.assign(NP, MapPoint()); vp.assign(NP, nullptr);
        for (int j = 0; j < NP; j++) {
            pts[j].pos = mat_f32(3, 1, xw + 3 * j); pts[j].normal = mat_f32(3, 1, nrm + 3 * j); pts[j].desc = desc_mat(1, pdesc + 32 * (size_t)j);
            pts[j].mfMinDistance = min_d[j]; pts[j].mfMaxDistance = max_d[j];
            vp[j] = &pts[j];
        }
        holders.assign(N, MapPoint());
    }
};

int run_proj(Blocks& in, FILE* out) {
    ScwProblem q;
    q.load(in);
    std::vector<MapPoint*> vpMatched(q.N, nullptr);
    for (int i = 0; i < q.N; i++) if (q.state[i]) vpMatched[i] = &q.holders[i];
    int next = 0;
    for (int j = 0; j < q.NP; j++) {
        q.pts[j].bad = !q.usable[j];
        if (!q.flag[j]) continue;
        while (next < q.N && !q.state[next]) next++;
        if (next == q.N) return 3;
        vpMatched[next++] = &q.pts[j];
    }
    ORBmatcher matcher(0.75f, true);
    const int nm = matcher.SearchByProjection(&q.kf, q.Scw, q.vp, vpMatched, (int)q.th);
    std::vector<int32_t> match(q.N, -1);
    for (int i = 0; i < q.N; i++) if (!q.state[i] && vpMatched[i]) match[i] = (int32_t)(vpMatched[i] - q.pts.data());
    write_block(out, match.data(), match.size()); write_block(out, &nm, 1);
    return 0;
}

// out: vpReplacePoint (per point: -1 NULL, j' >= 0 a point of the list, -2 - idx the point the key frame held in slot idx on entry), the slot AddObservation got
// per point (-1 none), the key frame's slots after the call, the return value
int run_fuse(Blocks& in, FILE* out) {
    ScwProblem q;
    q.load(in);
    for (int i = 0; i < q.N; i++) if (q.state[i]) { q.holders[i].bad = q.state[i] == 2; q.kf.mps[i] = &q.holders[i]; }
    int next = 0;
    for (int j = 0; j < q.NP; j++) {
        if (q.usable[j]) continue;
        if (!(j & 1)) {
            while (next < q.N && q.state[next] != 1) next++;
            if (next < q.N) { q.kf.mps[next++] = &q.pts[j]; continue; }
        }
        q.pts[j].bad = true;
    }
    std::vector<MapPoint*> vpReplacePoint(q.NP, nullptr);
    ORBmatcher matcher(0.8f, true);
    const int nFused = matcher.Fuse(&q.kf, q.Scw, q.vp, q.th, vpReplacePoint);
    std::vector<int32_t> rep(q.NP, -1), added(q.NP, -1), slots(q.N, -1);
    for (int j = 0; j < q.NP; j++) {
        added[j] = q.pts[j].added_at;
        MapPoint* r = vpReplacePoint[j];
        if (!r) continue;
        if (r >= q.pts.data() && r < q.pts.data() + q.NP) rep[j] = (int32_t)(r - q.pts.data());
        else rep[j] = -2 - (int32_t)(r - q.holders.data());
    }
    for (int i = 0; i < q.N; i++) if (!q.state[i] && q.kf.mps[i]) slots[i] = (int32_t)(q.kf.mps[i] - q.pts.data());
    write_block(out, rep.data(), rep.size()); write_block(out, added.data(), added.size()); write_block(out, slots.data(), slots.size()); write_block(out, &nFused, 1);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: adapter_loop_match <bow|sim3|proj|fuse> <in.bin> <out.bin>\n"); return 2; }
    Blocks in;
    if (!in.load(argv[2])) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    const std::string mode = argv[1];
    const int rc = mode == "bow" ? run_bow(in, out) : mode == "sim3" ? run_sim3(in, out) : mode == "proj" ? run_proj(in, out) : mode == "fuse" ? run_fuse(in, out) : 2;
    std::fclose(out);
    return rc;
}
