// tests/adapter_shim/adapter_essential_graph_main.cpp — TEST INFRASTRUCTURE.  Optimizer::OptimizeEssentialGraph of include/planar_adapters.hpp
// (PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH) on the stand-in map objects of oracle/shim/opt_standins.hpp (-DSTANDINS_NO_REFERENCE: no reference headers needed).
//   adapter_essential_graph run <in.bin> <out.bin>   the adapter through the reference's signature; same input as the fixture generator's driver
//                                                     (tools/essential_graph_golden/ref_essential_graph_main.cpp, written by tests/essential_graph_cases.py) and the
//                                                     same output blocks, so the result is compared with tests/golden/essential_graph_ref.npz
//   adapter_essential_graph edges <in.txt>           planar_adapter::essential_graph_edges on plain arrays, no key frame and no device: "n cur loop", parent[n], then
//                                                     three lists (loop edges, covisible, loop connections), each n rows "count (index weight)*"; prints "v0 v1 kind" lines
#include <set>
#include <string>

#include "g2o_sim3_standin.hpp"
#include "adapter_io.hpp"

namespace Planar_SLAM {
class LoopClosing {
public:
    typedef std::map<KeyFrame*, g2o::Sim3> KeyFrameAndPose;
};
class Optimizer {
public:
    void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections,
                                       const bool& bFixScale);   // include/Optimizer.h
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH
#include "planar_adapters.hpp"

float Planar_SLAM::Frame::fx, Planar_SLAM::Frame::fy, Planar_SLAM::Frame::cx, Planar_SLAM::Frame::cy;
std::mutex Planar_SLAM::MapPoint::mGlobalMutex, Planar_SLAM::MapLine::mGlobalMutex, Planar_SLAM::MapPlane::mGlobalMutex;

using namespace Planar_SLAM;
using namespace adapter_io;

static int run_edges(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    int n, cur, loop;
    if (std::fscanf(f, "%d %d %d", &n, &cur, &loop) != 3) return 2;
    std::vector<int32_t> parent(n), off[3], idx[3], w[3];
    for (int i = 0; i < n; i++) if (std::fscanf(f, "%d", &parent[i]) != 1) return 2;
    for (int l = 0; l < 3; l++) {
        off[l].push_back(0);
        for (int i = 0; i < n; i++) {
            int c;
            if (std::fscanf(f, "%d", &c) != 1) return 2;
            for (int k = 0; k < c; k++) { int a, b; if (std::fscanf(f, "%d %d", &a, &b) != 2) return 2; idx[l].push_back(a); w[l].push_back(b); }
            off[l].push_back((int32_t)idx[l].size());
        }
    }
    std::fclose(f);
    planar_adapter::EssGraphLists L[3];
    for (int l = 0; l < 3; l++) L[l] = planar_adapter::EssGraphLists{off[l].data(), idx[l].data(), w[l].data()};
    const std::vector<int32_t> e = planar_adapter::essential_graph_edges(n, parent.data(), L[0], L[1], L[2], cur, loop);
    for (size_t k = 0; k < e.size(); k += 3) std::printf("%d %d %d\n", e[k], e[k + 1], e[k + 2]);
    return 0;
}

static g2o::Sim3 sim3_of(const double* p) { g2o::Sim3 S; for (int k = 0; k < 8; k++) S[k] = p[k]; return S; }

static int run_adapter(const char* in, const char* out) {
    Blocks bl;
    if (!bl.load(in) || bl.size() != 14) { std::fprintf(stderr, "cannot read 14 blocks from %s\n", in); return 2; }
    const int32_t* hdr = (const int32_t*)bl[0].data();
    const int n = hdr[0], fixed = hdr[1], cur = hdr[2];
    const float* poses = (const float*)bl[1].data();
    const double* corr = (const double*)bl[2].data(); const uint8_t* corr_mask = bl[3].data();
    const double* nc = (const double*)bl[4].data(); const uint8_t* nc_mask = bl[5].data();
    const int32_t* cnt = (const int32_t*)bl[6].data(); const int32_t* ids = (const int32_t*)bl[7].data();
    std::vector<KeyFrame> kfs(n);
    Map map;
    LoopClosing::KeyFrameAndPose NonCorrected, Corrected;
    for (int i = 0, at = 0; i < n; i++) {
        kfs[i].mnId = (long unsigned)i;
        kfs[i].pose = mat_f32(4, 4, poses + 16 * i);
        for (int k = 0; k < cnt[i]; k++) kfs[i].covisible.push_back(&kfs[ids[at + k]]);
        at += cnt[i];
        if (corr_mask[i]) Corrected[&kfs[i]] = sim3_of(corr + 8 * i);
        if (nc_mask[i]) NonCorrected[&kfs[i]] = sim3_of(nc + 8 * i);
    }
    for (int i = n - 1; i >= 0; i--) map.kfs.push_back(&kfs[i]);      // GetAllKeyFrames() in no particular order: the adapter ranks by mnId
    std::map<KeyFrame*, std::set<KeyFrame*> > LoopConnections;
    LoopConnections[&kfs[cur]].insert(&kfs[fixed]);
    const int np = (int)(bl[8].size() / 12), nl = (int)(bl[10].size() / 48), npl = (int)(bl[12].size() / 16);
    std::vector<MapPoint> pts(np + 1); std::vector<MapLine> lines(nl); std::vector<MapPlane> planes(npl);
    for (int i = 0; i < np; i++) {
        pts[i].mWorldPos = mat_f32(3, 1, (const float*)bl[8].data() + 3 * i);
        pts[i].mnCorrectedByKF = (long unsigned)cur; pts[i].mnCorrectedReference = (long unsigned)((const int32_t*)bl[9].data())[i];
        map.mps.push_back(&pts[i]);
    }
    const float far_away[3] = {9, 9, 9};
    pts[np].mWorldPos = mat_f32(3, 1, far_away); pts[np].bad = true; map.mps.push_back(&pts[np]);      // a bad point: skipped, left as it is
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
    Optimizer::OptimizeEssentialGraph(&map, &kfs[fixed], &kfs[cur], NonCorrected, Corrected, LoopConnections, hdr[3] != 0);
    if (pts[np].mWorldPos.at<float>(0) != 9.f) return 3;
    std::vector<float> po(16 * (size_t)n), pp(3 * (size_t)np), ppl(4 * (size_t)npl);
    std::vector<double> pl(6 * (size_t)nl);
    for (int i = 0; i < n; i++) { const cv::Mat T = kfs[i].GetPose(); for (int k = 0; k < 16; k++) po[16 * i + k] = T.at<float>(k / 4, k % 4); }
    for (int i = 0; i < np; i++) { const cv::Mat P = pts[i].GetWorldPos(); for (int k = 0; k < 3; k++) pp[3 * i + k] = P.at<float>(k, 0); }
    for (int i = 0; i < nl; i++) for (int k = 0; k < 6; k++) pl[6 * i + k] = lines[i].mWorldPos(k);
    for (int i = 0; i < npl; i++) { const cv::Mat P = planes[i].GetWorldPos(); for (int k = 0; k < 4; k++) ppl[4 * i + k] = P.at<float>(k, 0); }
    FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    write_block(f, po.data(), po.size()); write_block(f, pp.data(), pp.size()); write_block(f, pl.data(), pl.size()); write_block(f, ppl.data(), ppl.size());
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "edges") return run_edges(argv[2]);
    if (argc == 4 && std::string(argv[1]) == "run") return run_adapter(argv[2], argv[3]);
    std::fprintf(stderr, "usage: %s run <in.bin> <out.bin> | edges <in.txt>\n", argv[0]);
    return 2;
}
