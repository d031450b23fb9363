// tools/global_ba_golden/ref_global_ba_main.cpp — TEST INFRASTRUCTURE: runs the REAL Optimizer::GlobalBundleAdjustemnt (reference src/Optimizer.cc:35-548) on one
// map.  Linked by tools/gen_golden_global_ba.py against the objects `make -C oracle _ref/ref_opt` leaves in oracle/_ref/obj_opt (the reference's Optimizer.cc,
// Converter.cc and its vendored g2o, compiled where they lie) minus that program's main.o, with oracle/shim/opt_standins.hpp force-included as the recipe of
// oracle/Makefile does.  Nothing here computes: it stores the flat arrays of a planar_ba_problem in the stand-in KeyFrame / MapPoint / MapLine / MapPlane / Map
// objects and writes what the function left in them.  nLoopKF = 0, so the results come back through SetPose / SetWorldPos.
//   in : blocks {int64 nbytes; bytes}: hdr i32[6] = n_kf, n_lm, n_edges, iterations, robust, reverse; cam f32[5]; cfg f64[6] (AngleInfo, DistanceInfo, ParallelInfo,
//        VerticalInfo, Chi, VPChi); kf_Tcw f32[n_kf][16]; lm_type u8[n_lm]; lm_init f64[n_lm][4]; e_kf i32; e_lm i32; e_type u8; e_meas f64[n_edges][4];
//        e_inv_sigma2 f32.  Key frame k has mnId k (mnId 0 is the fixed one); line landmarks come in (start, end) pairs, their two edges of an observation
//        consecutive, on the observing key frame.
//        reverse = 1 allocates the key-frame objects in descending address order, so every std::map<KeyFrame*, size_t> of observations iterates the other way:
//        a different summation order, nothing else.
//   out: blocks: kf_Tcw f32[n_kf][16]; lm f64[n_lm][4] (points and planes are the float32 values the reference keeps, widened)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Optimizer.h"

using namespace Planar_SLAM;

float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
std::mutex MapPoint::mGlobalMutex, MapLine::mGlobalMutex, MapPlane::mGlobalMutex;

namespace {

std::vector<std::vector<unsigned char>> read_blocks(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<std::vector<unsigned char>> out;
    int64_t k;
    while (fread(&k, 8, 1, f) == 1) {
        out.emplace_back((size_t)k);
        if (k && fread(out.back().data(), 1, (size_t)k, f) != (size_t)k) { fprintf(stderr, "short block\n"); exit(2); }
    }
    fclose(f);
    return out;
}
template <class T> void write_block(FILE* f, const T* p, size_t n) {
    const int64_t k = (int64_t)(n * sizeof(T));
    fwrite(&k, 8, 1, f);
    if (n) fwrite(p, sizeof(T), n, f);
}
cv::Mat mat_f32(int r, int c, const float* p) { cv::Mat m(r, c, CV_32F); memcpy(m.data, p, sizeof(float) * r * c); return m; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    const auto bl = read_blocks(argv[1]);
    if (bl.size() != 11) { fprintf(stderr, "11 blocks expected, got %zu\n", bl.size()); return 2; }
    const int32_t* hdr = (const int32_t*)bl[0].data();
    const int K = hdr[0], NLM = hdr[1], NE = hdr[2], iterations = hdr[3];
    const bool robust = hdr[4] != 0, reverse = hdr[5] != 0;
    const float* cam = (const float*)bl[1].data();
    const double* cfg = (const double*)bl[2].data();
    auto& t = Config::table();
    t["Plane.AngleInfo"] = cfg[0]; t["Plane.DistanceInfo"] = cfg[1]; t["Plane.ParallelInfo"] = cfg[2]; t["Plane.VerticalInfo"] = cfg[3]; t["Plane.Chi"] = cfg[4];
    t["Plane.VPChi"] = cfg[5];
    const float* kf_Tcw = (const float*)bl[3].data();
    const unsigned char* lm_type = bl[4].data();
    const double* lm_init = (const double*)bl[5].data();
    const int32_t* e_kf = (const int32_t*)bl[6].data(); const int32_t* e_lm = (const int32_t*)bl[7].data();
    const unsigned char* e_type = bl[8].data();
    const double* e_meas = (const double*)bl[9].data();
    const float* e_is2 = (const float*)bl[10].data();

    std::vector<KeyFrame> store(K);
    auto kf_of = [&](int k) -> KeyFrame& { return store[reverse ? K - 1 - k : k]; };
    Map map;
    for (int k = 0; k < K; k++) {
        KeyFrame& kf = kf_of(k);
        kf.mnId = (unsigned long)k;
        kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3]; kf.mbf = cam[4];
        kf.pose = mat_f32(4, 4, kf_Tcw + (size_t)k * 16);
        map.kfs.push_back(&kf);
    }
    // landmark objects: a plane per type-1 landmark, a line per (start, end) pair of type-0 landmarks that carry line edges, a point per other type-0 landmark
    std::vector<int> lm_obj(NLM, -1);
    std::vector<char> is_line_pt(NLM, 0), is_end(NLM, 0);
    for (int e = 0; e + 1 < NE; e++)
        if (e_type[e] == 2) {
            if (e_type[e + 1] != 2 || e_lm[e + 1] != e_lm[e] + 1 || e_kf[e + 1] != e_kf[e]) { fprintf(stderr, "edge %d: a line observation is a (start, end) pair of edges\n", e); return 3; }
            is_line_pt[e_lm[e]] = 1; is_line_pt[e_lm[e + 1]] = 1; is_end[e_lm[e + 1]] = 1;
            e++;
        }
    int n_pt = 0, n_ln = 0, n_pl = 0;
    for (int l = 0; l < NLM; l++) {
        if (lm_type[l] == 1) lm_obj[l] = n_pl++;
        else if (is_line_pt[l]) { if (is_end[l]) lm_obj[l] = lm_obj[l - 1]; else lm_obj[l] = n_ln++; }
        else lm_obj[l] = n_pt++;
    }
    std::vector<MapPoint> mps(n_pt);
    std::vector<MapLine> mls(n_ln);
    std::vector<MapPlane> mpls(n_pl);
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
    // observations: one feature slot per edge in its key frame
    for (int e = 0; e < NE; e++) {
        KeyFrame& kf = kf_of(e_kf[e]);
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
                if (is_end[l]) break;                    // the end-point edge shares the observation of the start-point edge
                kf.mvKeyLineFunctions.push_back(Eigen::Vector3d(m[0], m[1], m[2]));      // the observer's own line function (:232)
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
    bool stop = false;
    Optimizer::GlobalBundleAdjustemnt(&map, iterations, &stop, 0, robust);
    std::vector<float> po(16 * (size_t)K);
    std::vector<double> lo(4 * (size_t)NLM, 0.0);
    for (int k = 0; k < K; k++) memcpy(&po[16 * (size_t)k], kf_of(k).pose.data, 64);
    for (int l = 0; l < NLM; l++) {
        double* v = &lo[4 * (size_t)l];
        if (lm_type[l] == 1) { cv::Mat c = mpls[lm_obj[l]].mWorldPos; for (int j = 0; j < 4; j++) v[j] = c.at<float>(j); }
        else if (is_line_pt[l]) { const int o = is_end[l] ? 3 : 0; for (int j = 0; j < 3; j++) v[j] = mls[lm_obj[l]].mWorldPos[o + j]; }
        else { cv::Mat c = mps[lm_obj[l]].mWorldPos; for (int j = 0; j < 3; j++) v[j] = c.at<float>(j); }
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    write_block(f, po.data(), po.size());
    write_block(f, lo.data(), lo.size());
    fclose(f);
    return 0;
}
