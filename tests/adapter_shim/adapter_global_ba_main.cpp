// tests/adapter_shim/adapter_global_ba_main.cpp — TEST INFRASTRUCTURE.  Optimizer::GlobalBundleAdjustemnt and Optimizer::BundleAdjustment of
// include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_GLOBAL_BA, over libplanar_hip.so) on the stand-in map objects of oracle/shim/opt_standins.hpp
// (-DSTANDINS_NO_REFERENCE: no reference headers needed).
//   adapter_global_ba run <in.bin> <out.bin> <nLoopKF>
// The input is the fixture generator's (tools/global_ba_golden/ref_global_ba_main.cpp, written by tests/global_ba_cases.py reference_blocks) and the output has the
// same two blocks, so the result is compared with tests/golden/global_ba_ref.npz.  On top of the fixture's map this program adds what the adapter must filter: a bad
// key frame inside the map's list and a key frame outside it with mnId > maxKFid, both observing landmarks of the map (a point, a line, a plane through each of its
// three observation maps) with measurements that would wreck the solve; a bad map point, a bad map line and a bad map plane, which must come back untouched; and it
// lists the key frames in descending mnId.  nLoopKF == 0 reads the results from the poses and world positions; nLoopKF != 0 from mTcwGBA / mPosGBA, and checks that
// mnBAGlobalForKF is nLoopKF on what was optimised (0 on a landmark without an edge) and that no pose or world position moved.  Exit 3: one of these checks failed.
#include <string>

#include "adapter_io.hpp"

namespace Planar_SLAM {
class Optimizer {
public:
    void static BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, const std::vector<MapLine*>& vpML,
                                 const std::vector<MapPlane*>& vpMPL, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                                 const bool bRobust = true);                                                                            // include/Optimizer.h:22-24
    void static GlobalBundleAdjustemnt(Map* pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);   // :26-27
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_GLOBAL_BA
#include "planar_adapters.hpp"

float Planar_SLAM::Frame::fx, Planar_SLAM::Frame::fy, Planar_SLAM::Frame::cx, Planar_SLAM::Frame::cy;
std::mutex Planar_SLAM::MapPoint::mGlobalMutex, Planar_SLAM::MapLine::mGlobalMutex, Planar_SLAM::MapPlane::mGlobalMutex;

using namespace Planar_SLAM;
using namespace adapter_io;

static bool same(const cv::Mat& a, const cv::Mat& b, int n) { for (int i = 0; i < n; i++) if (a.at<float>(i) != b.at<float>(i)) return false; return true; }

static int run(const char* in, const char* out, unsigned long nLoopKF) {
    Blocks bl;
    if (!bl.load(in) || bl.size() != 11) { std::fprintf(stderr, "cannot read 11 blocks from %s\n", in); return 2; }
    const int32_t* hdr = (const int32_t*)bl[0].data();
    const int K = hdr[0], NLM = hdr[1], NE = hdr[2], iterations = hdr[3];
    const bool robust = hdr[4] != 0;
    const float* cam = (const float*)bl[1].data();
    const double* cfg = (const double*)bl[2].data();
    auto& t = Config::table();
    t["Plane.AngleInfo"] = cfg[0]; t["Plane.DistanceInfo"] = cfg[1]; t["Plane.ParallelInfo"] = cfg[2]; t["Plane.VerticalInfo"] = cfg[3]; t["Plane.Chi"] = cfg[4];
    t["Plane.VPChi"] = cfg[5];
    const float* kf_Tcw = (const float*)bl[3].data();
    const uint8_t* lm_type = bl[4].data();
    const double* lm_init = (const double*)bl[5].data();
    const int32_t* e_kf = (const int32_t*)bl[6].data(); const int32_t* e_lm = (const int32_t*)bl[7].data();
    const uint8_t* e_type = bl[8].data();
    const double* e_meas = (const double*)bl[9].data();
    const float* e_is2 = (const float*)bl[10].data();

    std::vector<KeyFrame> kfs(K + 2);                        // [K]: bad, inside the map's list; [K + 1]: good, outside it (mnId > maxKFid)
    Map map;
    for (int k = 0; k < K + 2; k++) {
        KeyFrame& kf = kfs[k];
        kf.mnId = (unsigned long)k;
        kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3]; kf.mbf = cam[4];
        kf.pose = mat_f32(4, 4, kf_Tcw + (size_t)(k < K ? k : 0) * 16);
    }
    kfs[K].bad = true;
    for (int k = K; k >= 0; k--) map.kfs.push_back(&kfs[k]);     // GetAllKeyFrames() in no particular order: the adapter ranks by mnId
    std::vector<int> lm_obj(NLM, -1);
    std::vector<char> is_line_pt(NLM, 0), is_end(NLM, 0);
    for (int e = 0; e + 1 < NE; e++)
        if (e_type[e] == 2) { is_line_pt[e_lm[e]] = 1; is_line_pt[e_lm[e + 1]] = 1; is_end[e_lm[e + 1]] = 1; e++; }
    int n_pt = 0, n_ln = 0, n_pl = 0;
    for (int l = 0; l < NLM; l++) {
        if (lm_type[l] == 1) lm_obj[l] = n_pl++;
        else if (is_line_pt[l]) { if (is_end[l]) lm_obj[l] = lm_obj[l - 1]; else lm_obj[l] = n_ln++; }
        else lm_obj[l] = n_pt++;
    }
    std::vector<MapPoint> mps(n_pt + 1);                     // the last of each: a bad one
    std::vector<MapLine> mls(n_ln + 1);
    std::vector<MapPlane> mpls(n_pl + 1);
    for (int l = 0; l < NLM; l++) {
        const double* v = lm_init + (size_t)l * 4;
        if (lm_type[l] == 1) {
            MapPlane& p = mpls[lm_obj[l]]; p.mnId = (unsigned long)lm_obj[l];
            const float c[4] = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
            p.mWorldPos = mat_f32(4, 1, c);
            map.mpls.push_back(&p);
        } else if (is_line_pt[l]) {
            MapLine& m = mls[lm_obj[l]];
            if (!is_end[l]) { m.mnId = (unsigned long)lm_obj[l]; for (int j = 0; j < 3; j++) m.mWorldPos[j] = v[j]; map.mls.push_back(&m); }
            else for (int j = 0; j < 3; j++) m.mWorldPos[3 + j] = v[j];
        } else {
            MapPoint& p = mps[lm_obj[l]]; p.mnId = (unsigned long)lm_obj[l];
            const float c[3] = {(float)v[0], (float)v[1], (float)v[2]};
            p.mWorldPos = mat_f32(3, 1, c);
            map.mps.push_back(&p);
        }
    }
    for (int e = 0; e < NE; e++) {
        KeyFrame& kf = kfs[e_kf[e]];
        const int l = e_lm[e];
        const double* m = e_meas + (size_t)e * 4;
        switch (e_type[e]) {
            case 0: case 1: {
                cv::KeyPoint kp; kp.pt.x = (float)m[0]; kp.pt.y = (float)m[1]; kp.octave = (int)kf.mvKeysUn.size();
                kf.mvKeysUn.push_back(kp);
                kf.mvuRight.push_back(e_type[e] == 1 ? (float)m[2] : -1.f);
                kf.mvInvLevelSigma2.push_back(e_is2[e]);
                kf.mps.push_back(&mps[lm_obj[l]]);
                mps[lm_obj[l]].mObservations[&kf] = kf.mvKeysUn.size() - 1;
                break;
            }
            case 2: {
                if (is_end[l]) break;
                kf.mvKeyLineFunctions.push_back(Eigen::Vector3d(m[0], m[1], m[2]));
                kf.mls.push_back(&mls[lm_obj[l]]);
                mls[lm_obj[l]].mObservations[&kf] = kf.mvKeyLineFunctions.size() - 1;
                break;
            }
            default: {
                const float c[4] = {(float)m[0], (float)m[1], (float)m[2], (float)m[3]};
                kf.mvPlaneCoefficients.push_back(mat_f32(4, 1, c));
                MapPlane& p = mpls[lm_obj[l]];
                const size_t idx = kf.mvPlaneCoefficients.size() - 1;
                if (e_type[e] == 3) { p.mObservations[&kf] = idx; kf.mpls.push_back(&p); }
                else if (e_type[e] == 4) p.mVerObservations[&kf] = idx;
                else p.mParObservations[&kf] = idx;
                break;
            }
        }
    }
    // what must be filtered: the bad key frame and the outsider observe the first point, line and plane that have observations, with absurd measurements
    for (int x = K; x < K + 2; x++) {
        KeyFrame& kf = kfs[x];
        cv::KeyPoint kp; kp.pt.x = 5.f; kp.pt.y = 470.f; kp.octave = 0;
        kf.mvKeysUn.push_back(kp); kf.mvuRight.push_back(1.f); kf.mvInvLevelSigma2.push_back(1.f);
        kf.mvKeyLineFunctions.push_back(Eigen::Vector3d(0.6, 0.8, -300.0));
        const float c[4] = {1.f, 0.f, 0.f, 9.f};
        kf.mvPlaneCoefficients.push_back(mat_f32(4, 1, c));
        for (int i = 0; i < n_pt; i++) if (!mps[i].mObservations.empty()) { mps[i].mObservations[&kf] = 0; break; }
        for (int i = 0; i < n_ln; i++) if (!mls[i].mObservations.empty()) { mls[i].mObservations[&kf] = 0; break; }
        for (int i = 0; i < n_pl; i++) if (!mpls[i].mObservations.empty()) { mpls[i].mObservations[&kf] = 0; mpls[i].mVerObservations[&kf] = 0; mpls[i].mParObservations[&kf] = 0; break; }
    }
    // bad landmarks, observed by key frame 1: skipped, left as they are
    const float far3[3] = {9, 9, 9}, far4[4] = {0, 0, 1, 9};
    mps[n_pt].bad = true; mps[n_pt].mWorldPos = mat_f32(3, 1, far3); mps[n_pt].mObservations[&kfs[K > 1 ? 1 : 0]] = 0; map.mps.push_back(&mps[n_pt]);
    mls[n_ln].bad = true; for (int j = 0; j < 6; j++) mls[n_ln].mWorldPos[j] = 9; mls[n_ln].mObservations[&kfs[K > 1 ? 1 : 0]] = 0; map.mls.push_back(&mls[n_ln]);
    mpls[n_pl].bad = true; mpls[n_pl].mWorldPos = mat_f32(4, 1, far4); mpls[n_pl].mObservations[&kfs[K > 1 ? 1 : 0]] = 0; map.mpls.push_back(&mpls[n_pl]);

    std::vector<cv::Mat> pose0(K);
    for (int k = 0; k < K; k++) pose0[k] = kfs[k].pose.clone();
    bool stop = false;
    Optimizer::GlobalBundleAdjustemnt(&map, iterations, &stop, nLoopKF, robust);

    if (mps[n_pt].mWorldPos.at<float>(0) != 9.f || mls[n_ln].mWorldPos[0] != 9 || mpls[n_pl].mWorldPos.at<float>(3) != 9.f) return 3;
    if (mps[n_pt].mnBAGlobalForKF != 0 || kfs[K].mnBAGlobalForKF != 0 || kfs[K + 1].mnBAGlobalForKF != 0) return 3;
    std::vector<float> po(16 * (size_t)K);
    std::vector<double> lo(4 * (size_t)NLM, 0.0);
    std::vector<char> seen(NLM, 0);
    for (int e = 0; e < NE; e++) seen[e_lm[e]] = 1;
    for (int k = 0; k < K; k++) {
        if (nLoopKF) {
            if (!same(kfs[k].pose, pose0[k], 16) || kfs[k].mnBAGlobalForKF != nLoopKF) return 3;
            std::memcpy(&po[16 * (size_t)k], kfs[k].mTcwGBA.data, 64);
        } else std::memcpy(&po[16 * (size_t)k], kfs[k].pose.data, 64);
    }
    for (int l = 0; l < NLM; l++) {
        double* v = &lo[4 * (size_t)l];
        const double* v0 = lm_init + (size_t)l * 4;
        const bool gba = nLoopKF != 0 && seen[l];            // a landmark without an edge carries no mPosGBA: it is reported as it is in the map
        if (lm_type[l] == 1) {
            MapPlane& p = mpls[lm_obj[l]];
            if (nLoopKF && (p.mnBAGlobalForKF != (seen[l] ? nLoopKF : 0) || p.mWorldPos.at<float>(3) != (float)v0[3])) return 3;
            const cv::Mat c = gba ? p.mPosGBA : p.mWorldPos;
            for (int j = 0; j < 4; j++) v[j] = c.at<float>(j);
        } else if (is_line_pt[l]) {
            MapLine& m = mls[lm_obj[l]];
            const int o = is_end[l] ? 3 : 0;
            if (nLoopKF && (m.mnBAGlobalForKF != nLoopKF || m.mWorldPos[o] != v0[0])) return 3;
            for (int j = 0; j < 3; j++) v[j] = gba ? (double)m.mPosGBA.at<float>(o + j) : m.mWorldPos[o + j];
        } else {
            MapPoint& p = mps[lm_obj[l]];
            if (nLoopKF && (p.mnBAGlobalForKF != (seen[l] ? nLoopKF : 0) || p.mWorldPos.at<float>(0) != (float)v0[0])) return 3;
            const cv::Mat c = gba ? p.mPosGBA : p.mWorldPos;
            for (int j = 0; j < 3; j++) v[j] = c.at<float>(j);
        }
    }
    FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    write_block(f, po.data(), po.size()); write_block(f, lo.data(), lo.size());
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && std::string(argv[1]) == "run") return run(argv[2], argv[3], std::stoul(argv[4]));
    std::fprintf(stderr, "usage: %s run <in.bin> <out.bin> <nLoopKF>\n", argv[0]);
    return 2;
}
