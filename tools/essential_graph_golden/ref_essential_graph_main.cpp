// tools/essential_graph_golden/ref_essential_graph_main.cpp — TEST INFRASTRUCTURE: runs the REAL Optimizer::OptimizeEssentialGraph (reference
// src/Optimizer.cc:2680-2991) on one graph.  Linked by tools/gen_golden_essential_graph.py against the objects `make -C oracle _ref/ref_opt` leaves in
// oracle/_ref/obj_opt (the reference's Optimizer.cc, Converter.cc, types_seven_dof_expmap.cpp and its vendored g2o, compiled where they lie) minus that program's
// main.o, with oracle/shim/opt_standins.hpp force-included as the recipe of oracle/Makefile does.  Nothing here computes: it stores what it reads in the stand-in
// KeyFrame / MapPoint / MapLine / MapPlane / Map objects and writes what the function left.  The stand-in key frame has no parent, no loop edge and weight 0, so
// normal edges come from its `covisible` list and the only loop connection that passes the weight gate is (current, loop); a stand-in landmark has no reference key
// frame, so every landmark carries mnCorrectedByKF = pCurKF->mnId and its reference id in mnCorrectedReference.
//   in : blocks {int64 nbytes; bytes}: hdr i32[4] = n, fixed (pLoopKF), cur (pCurKF), fix_scale; poses f32[n][16]; corrected f64[n][8]; corr_mask u8[n];
//        noncorrected f64[n][8]; nc_mask u8[n]; covisible counts i32[n]; covisible ids i32[sum]; points f32[np][3]; point refs i32[np]; lines f64[nl][6];
//        line refs i32[nl]; planes f32[npl][4]; plane refs i32[npl]
//   out: blocks: poses f32[n][16], points f32[np][3], lines f64[nl][6], planes f32[npl][4] (the generator does not store the planes: the cv::Mat stand-in of this
//        build does not write `m.rowRange(0, 3).col(0) = expr` through the view, so they are not what the reference computes with OpenCV)
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
g2o::Sim3 sim3_of(const double* p) { g2o::Sim3 S; for (int k = 0; k < 8; k++) S[k] = p[k]; return S; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    const auto bl = read_blocks(argv[1]);
    if (bl.size() != 14) { fprintf(stderr, "14 blocks expected, got %zu\n", bl.size()); return 2; }
    const int32_t* hdr = (const int32_t*)bl[0].data();
    const int n = hdr[0], fixed = hdr[1], cur = hdr[2];
    const bool fix_scale = hdr[3] != 0;
    const float* poses = (const float*)bl[1].data();
    const double* corr = (const double*)bl[2].data(); const unsigned char* corr_mask = bl[3].data();
    const double* nc = (const double*)bl[4].data(); const unsigned char* nc_mask = bl[5].data();
    const int32_t* cnt = (const int32_t*)bl[6].data(); const int32_t* ids = (const int32_t*)bl[7].data();
    std::vector<KeyFrame> kfs(n);
    Map map;
    LoopClosing::KeyFrameAndPose NonCorrected, Corrected;
    for (int i = 0, at = 0; i < n; i++) {
        kfs[i].mnId = (long unsigned)i;
        kfs[i].pose = mat_f32(4, 4, poses + 16 * i);
        for (int k = 0; k < cnt[i]; k++) kfs[i].covisible.push_back(&kfs[ids[at + k]]);
        at += cnt[i];
        map.kfs.push_back(&kfs[i]);
        if (corr_mask[i]) Corrected[&kfs[i]] = sim3_of(corr + 8 * i);
        if (nc_mask[i]) NonCorrected[&kfs[i]] = sim3_of(nc + 8 * i);
    }
    std::map<KeyFrame*, std::set<KeyFrame*>> LoopConnections;
    LoopConnections[&kfs[cur]].insert(&kfs[fixed]);
    const int np = (int)(bl[8].size() / 12), nl = (int)(bl[10].size() / 48), npl = (int)(bl[12].size() / 16);
    std::vector<MapPoint> pts(np); std::vector<MapLine> lines(nl); std::vector<MapPlane> planes(npl);
    for (int i = 0; i < np; i++) {
        pts[i].mWorldPos = mat_f32(3, 1, (const float*)bl[8].data() + 3 * i);
        pts[i].mnCorrectedByKF = (long unsigned)cur; pts[i].mnCorrectedReference = (long unsigned)((const int32_t*)bl[9].data())[i];
        map.mps.push_back(&pts[i]);
    }
    for (int i = 0; i < nl; i++) {
        for (int k = 0; k < 6; k++) lines[i].mWorldPos(k) = ((const double*)bl[10].data())[6 * i + k];
        lines[i].mnCorrectedByKF = (long unsigned)cur; lines[i].mnCorrectedReference = (long unsigned)((const int32_t*)bl[11].data())[i];
        map.mls.push_back(&lines[i]);
    }
    for (int i = 0; i < npl; i++) {
        planes[i].mWorldPos = mat_f32(4, 1, (const float*)bl[12].data() + 4 * i);
        planes[i].mnCorrectedByKF = (long unsigned)cur; planes[i].mnCorrectedReference = (long unsigned)((const int32_t*)bl[13].data())[i];
        map.mpls.push_back(&planes[i]);
    }
    Optimizer::OptimizeEssentialGraph(&map, &kfs[fixed], &kfs[cur], NonCorrected, Corrected, LoopConnections, fix_scale);
    std::vector<float> po(16 * (size_t)n), pp(3 * (size_t)np), ppl(4 * (size_t)npl);
    std::vector<double> pl(6 * (size_t)nl);
    for (int i = 0; i < n; i++) { const cv::Mat T = kfs[i].GetPose(); for (int k = 0; k < 16; k++) po[16 * i + k] = T.at<float>(k / 4, k % 4); }
    for (int i = 0; i < np; i++) { const cv::Mat P = pts[i].GetWorldPos(); for (int k = 0; k < 3; k++) pp[3 * i + k] = P.at<float>(k, 0); }
    for (int i = 0; i < nl; i++) for (int k = 0; k < 6; k++) pl[6 * i + k] = lines[i].mWorldPos(k);
    for (int i = 0; i < npl; i++) { const cv::Mat P = planes[i].GetWorldPos(); for (int k = 0; k < 4; k++) ppl[4 * i + k] = P.at<float>(k, 0); }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    write_block(f, po.data(), po.size());
    write_block(f, pp.data(), pp.size());
    write_block(f, pl.data(), pl.size());
    write_block(f, ppl.data(), ppl.size());
    fclose(f);
    return 0;
}
