// tools/loop_match_golden/ref_loop_match_main.cpp — fixture generator, not product code.  Driver for the REAL reference's four loop-closing matchers,
// ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (src/ORBmatcher.cc:526-659), SearchBySim3 (:1106-1330), SearchByProjection(KeyFrame*, Scw, vpPoints,
// vpMatched, th) (:294-407) and Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:981-1104), compiled by tools/gen_golden_loop_match.py from the reference tree
// where it lies (never copied) against loop_match_standins.hpp, with the flags and sources of oracle/Makefile's ref_match recipe.
//   ref_loop_match <bow|sim3|proj|fuse> <in.bin> <out.bin>      in/out: sequences of blocks {int64 nbytes; bytes}
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ORBmatcher.h"

using namespace Planar_SLAM;

float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY, Frame::mfGridElementWidthInv,
    Frame::mfGridElementHeightInv;

namespace {
struct Blocks {
    std::vector<std::vector<uint8_t>> b;
    size_t next = 0;
    bool load(const char* path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) return false;
        int64_t n;
        while (std::fread(&n, 8, 1, f) == 1) { b.emplace_back((size_t)n); if (n && std::fread(b.back().data(), 1, (size_t)n, f) != (size_t)n) return false; }
        std::fclose(f);
        return true;
    }
    template <typename T> const T* get(size_t* count = nullptr) { auto& v = b.at(next++); if (count) *count = v.size() / sizeof(T); return (const T*)v.data(); }
};
struct KP7 { float x, y, size, angle, response; int32_t octave, class_id; };
cv::Mat mat_f32(int r, int c, const float* src) { cv::Mat m(r, c, CV_32F); std::memcpy(m.data, src, sizeof(float) * r * c); return m; }
cv::Mat desc_mat(int n, const uint8_t* src) { cv::Mat m(n, 32, CV_8UC1); if (n) std::memcpy(m.data, src, (size_t)n * 32); return m; }

// blocks of one key frame: keys, desc, intr {min_x, max_x, min_y, max_y, grid_w_inv, grid_h_inv, fx, fy, cx, cy, mfLogScaleFactor}, scale factors, Tcw,
// usable, xw, min_dist, max_dist, map-point descriptors
void fill(KeyFrame& kf, std::vector<MapPoint>& mps, Blocks& in) {
    size_t n, nl;
    const KP7* k = in.get<KP7>(&n);
    const int N = (int)n;
    const uint8_t* desc = in.get<uint8_t>();
    const float* intr = in.get<float>();
    const float* sf = in.get<float>(&nl);
    const float* Tcw = in.get<float>();
    const uint8_t* usable = in.get<uint8_t>();
    const float *xw = in.get<float>(), *min_d = in.get<float>(), *max_d = in.get<float>();
    const uint8_t* mdesc = in.get<uint8_t>();
    // the grid is the frame's (src/KeyFrame.cc:56-63): built by the reference's own Frame::AssignFeaturesToGrid under this key frame's bounds
    Frame F;
    F.N = N; F.mvKeysUn.resize(N);
    kf.mFeatVec.clear();
    for (int i = 0; i < N; i++) F.mvKeysUn[i] = cv::KeyPoint(k[i].x, k[i].y, k[i].size, k[i].angle, k[i].response, k[i].octave, k[i].class_id);
    Frame::mnMinX = intr[0]; Frame::mnMaxX = intr[1]; Frame::mnMinY = intr[2]; Frame::mnMaxY = intr[3];
    Frame::mfGridElementWidthInv = intr[4]; Frame::mfGridElementHeightInv = intr[5];
    F.AssignFeaturesToGrid();
    kf.N = N; kf.mvKeysUn = F.mvKeysUn; kf.mvKeys = F.mvKeysUn; kf.mvuRight.assign(N, -1.f); kf.mDescriptors = desc_mat(N, desc);
    kf.mnMinX = intr[0]; kf.mnMaxX = intr[1]; kf.mnMinY = intr[2]; kf.mnMaxY = intr[3];
    kf.mfGridElementWidthInv = intr[4]; kf.mfGridElementHeightInv = intr[5];
    kf.fx = intr[6]; kf.fy = intr[7]; kf.cx = intr[8]; kf.cy = intr[9];
    kf.mfLogScaleFactor = intr[10]; kf.mnScaleLevels = (int)nl; kf.mvScaleFactors.assign(sf, sf + nl);
    kf.mGrid.resize(kf.mnGridCols);
    for (int i = 0; i < kf.mnGridCols; i++) { kf.mGrid[i].resize(kf.mnGridRows); for (int j = 0; j < kf.mnGridRows; j++) kf.mGrid[i][j] = F.mGrid[i][j]; }
    kf.SetPose(mat_f32(4, 4, Tcw));
    mps.assign(N, MapPoint());
    kf.mps.assign(N, nullptr);
    for (int i = 0; i < N; i++) {
        if (!usable[i] && !(i & 1)) continue;   // NULL slot; odd ones become isBad() points instead
        mps[i].bad = !usable[i];
        mps[i].pos = mat_f32(3, 1, xw + 3 * i); mps[i].desc = desc_mat(1, mdesc + 32 * (size_t)i);
        mps[i].mfMinDistance = min_d[i]; mps[i].mfMaxDistance = max_d[i]; mps[i].index = i;
        kf.mps[i] = &mps[i];
    }
}
void put(FILE* out, const void* p, size_t bytes) { int64_t nb = (int64_t)bytes; std::fwrite(&nb, 8, 1, out); if (bytes) std::fwrite(p, 1, bytes, out); }

int run_sim3(Blocks& in, FILE* out) {
    const float* prm = in.get<float>();   // {th, s12, R12[9], t12[3]}
    KeyFrame kf1, kf2;
    std::vector<MapPoint> mps1, mps2;
    fill(kf1, mps1, in);
    fill(kf2, mps2, in);
    const int32_t* entry = in.get<int32_t>();   // vpMatches12 on entry: -1 NULL, else GetIndexInKeyFrame(pKF2) of a point matched before
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
    put(out, match.data(), (size_t)N1 * 4); put(out, &nFound, 4);
    return 0;
}

// blocks: {nn_ratio, check_orientation}, then per key frame: keys, desc, node ids, usable
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
            kf[s].mvKeysUn[i] = cv::KeyPoint(k[i].x, k[i].y, k[i].size, k[i].angle, k[i].response, k[i].octave, k[i].class_id);
            if (node[i] >= 0) kf[s].mFeatVec.addFeature((DBoW2::NodeId)node[i], (unsigned)i);
            if (!usable[i] && !(i & 1)) continue;   // NULL slot; odd ones become isBad() points instead
            mps[s][i].bad = !usable[i]; mps[s][i].index = i;
            kf[s].mps[i] = &mps[s][i];
        }
    }
    ORBmatcher matcher(prm[0], prm[1] != 0);
    std::vector<MapPoint*> vpMatches12;
    const int nm = matcher.SearchByBoW(&kf[0], &kf[1], vpMatches12);
    std::vector<int32_t> match(kf[0].N, -1);
    for (int i = 0; i < kf[0].N && i < (int)vpMatches12.size(); i++) if (vpMatches12[i]) match[i] = (int32_t)(vpMatches12[i] - mps[1].data());
    put(out, match.data(), match.size() * 4); put(out, &nm, 4);
    return 0;
}

// the key frame of the two Scw entries (no map points of its own yet) and the list vpPoints.  blocks: prm {th}, keys, desc, intr, scale factors, Scw,
// slot state, then the points: usable, flag, xw, normal, min_dist, max_dist, desc
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
        Frame F;
        F.N = N; F.mvKeysUn.resize(N);
        for (int i = 0; i < N; i++) F.mvKeysUn[i] = cv::KeyPoint(k[i].x, k[i].y, k[i].size, k[i].angle, k[i].response, k[i].octave, k[i].class_id);
        Frame::mnMinX = intr[0]; Frame::mnMaxX = intr[1]; Frame::mnMinY = intr[2]; Frame::mnMaxY = intr[3];
        Frame::mfGridElementWidthInv = intr[4]; Frame::mfGridElementHeightInv = intr[5];
        F.AssignFeaturesToGrid();
        kf.N = N; kf.mvKeysUn = F.mvKeysUn; kf.mvKeys = F.mvKeysUn; kf.mvuRight.assign(N, -1.f); kf.mDescriptors = desc_mat(N, desc);
        kf.mnMinX = intr[0]; kf.mnMaxX = intr[1]; kf.mnMinY = intr[2]; kf.mnMaxY = intr[3];
        kf.mfGridElementWidthInv = intr[4]; kf.mfGridElementHeightInv = intr[5];
        kf.fx = intr[6]; kf.fy = intr[7]; kf.cx = intr[8]; kf.cy = intr[9];
        kf.mfLogScaleFactor = intr[10]; kf.mnScaleLevels = (int)nl; kf.mvScaleFactors.assign(sf, sf + nl);
        kf.mGrid.resize(kf.mnGridCols);
        for (int i = 0; i < kf.mnGridCols; i++) { kf.mGrid[i].resize(kf.mnGridRows); for (int j = 0; j < kf.mnGridRows; j++) kf.mGrid[i][j] = F.mGrid[i][j]; }
        kf.mps.assign(N, nullptr);
        pts.assign(NP, MapPoint()); vp.assign(NP, nullptr);
        for (int j = 0; j < NP; j++) {
            pts[j].pos = mat_f32(3, 1, xw + 3 * j); pts[j].normal = mat_f32(3, 1, nrm + 3 * j); pts[j].desc = desc_mat(1, pdesc + 32 * (size_t)j);
            pts[j].mfMinDistance = min_d[j]; pts[j].mfMaxDistance = max_d[j]; pts[j].index = j;
            vp[j] = &pts[j];
        }
        holders.assign(N, MapPoint());
    }
};

// proj: state[idx] = vpMatched[idx] != NULL on entry; usable[j] = !isBad(); flag[j] = the point is in vpMatched on entry (it takes the next matched slot)
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
        if (next == q.N) { std::fprintf(stderr, "more found points than matched slots\n"); return 3; }
        vpMatched[next++] = &q.pts[j];
    }
    ORBmatcher matcher(0.75f, true);
    const int nm = matcher.SearchByProjection(&q.kf, q.Scw, q.vp, vpMatched, (int)q.th);
    std::vector<int32_t> match(q.N, -1);
    for (int i = 0; i < q.N; i++) if (!q.state[i] && vpMatched[i]) match[i] = (int32_t)(vpMatched[i] - q.pts.data());
    put(out, match.data(), match.size() * 4); put(out, &nm, 4);
    return 0;
}

// fuse: state[idx] = 0 NULL, 1 a map point, 2 a bad one; usable[j] = 0: the point is bad (odd j) or already in the key frame (even j: it takes the next slot of
// state 1, or is bad when none is left)
int run_fuse(Blocks& in, FILE* out) {
    ScwProblem q;
    q.load(in);
    for (int i = 0; i < q.N; i++) if (q.state[i]) { q.holders[i].bad = q.state[i] == 2; q.holders[i].index = -2 - i; q.kf.mps[i] = &q.holders[i]; }
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
    fuse_log().clear();
    ORBmatcher matcher(0.8f, true);
    const int nFused = matcher.Fuse(&q.kf, q.Scw, q.vp, q.th, vpReplacePoint);
    // the slot of every fused point: KeyFrame::GetMapPoint(bestIdx) is called exactly once per fused point, right after GetDescriptor of that point
    std::vector<int32_t> idx(q.NP, -1), owner(q.NP, -9);
    for (auto& e : fuse_log()) if (e.first >= 0) idx[e.first] = e.second;
    for (int j = 0; j < q.NP; j++) {
        if (idx[j] < 0) continue;
        MapPoint* r = vpReplacePoint[j];
        if (q.pts[j].fuse_idx >= 0) owner[j] = j;                                        // AddObservation
        else if (r && r >= q.pts.data() && r < q.pts.data() + q.NP && q.usable[r - q.pts.data()]) owner[j] = (int32_t)(r - q.pts.data());
        else owner[j] = -1;                                                              // a point of the key frame on entry, or a bad one (nothing recorded)
    }
    // the key frame's slots after the call: the point of the list now there, -1 otherwise
    std::vector<int32_t> slots(q.N, -1);
    for (int i = 0; i < q.N; i++) if (!q.state[i] && q.kf.mps[i]) slots[i] = (int32_t)(q.kf.mps[i] - q.pts.data());
    put(out, idx.data(), idx.size() * 4); put(out, owner.data(), owner.size() * 4); put(out, slots.data(), slots.size() * 4); put(out, &nFused, 4);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: ref_loop_match <bow|sim3|proj|fuse> <in.bin> <out.bin>\n"); return 2; }
    Blocks in;
    if (!in.load(argv[2])) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    const std::string mode = argv[1];
    const int rc = mode == "bow" ? run_bow(in, out) : mode == "sim3" ? run_sim3(in, out) : mode == "proj" ? run_proj(in, out) : mode == "fuse" ? run_fuse(in, out) : 2;
    std::fclose(out);
    return rc;
}
