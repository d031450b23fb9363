// tools/new_lines_golden/new_lines_standins.hpp — fixture generator, not product code.
// What oracle/shim (frozen) lacks for the REAL LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:800-1037), KeyFrame::obtain3DLine / AddMapLine / GetMapLine /
// lineDescriptorMAD (src/KeyFrame.cc:738-747, 781-785, 852-856, 858-883) and MapLine's constructor and UpdateAverageDir (src/MapLine.cpp:16-29, 320-367), whose text
// tools/gen_golden_new_lines.py extracts into a temporary translation unit at generation time.  This header is force-included into that unit, into the driver and into
// src/LSDmatcher.cpp, which is compiled where it lies.  The reference's text is not edited; two names are redirected by macros at the end of this header:
//   KeyFrame -> KeyFrameX   (all three units) the shim's KeyFrame plus mvLines3D, mvDepthLine, mK, invfx, invfy, mfScaleFactor, mnFrameId and the four functions above,
//                           declared here with the reference's bodies: the shim's AddMapLine is a no-op and its lineDescriptorMAD a restatement, so LSDmatcher.cpp
//                           must call these (through KeyFrameX*) for an accepted idx1 to be occupied at the later neighbours and for the MAD to be the reference's
//   MapLine  -> NewLine     (the extracted unit and the driver only: -DNEW_LINES_EXTRACT) the shim's MapLine plus what the constructor and UpdateAverageDir touch.
//                           LSDmatcher.cpp keeps the shim's MapLine; KeyFrameX::GetMapLine hands it a NewLine*, which it only tests against NULL.
// SearchByDescriptor(KeyFrame*, KeyFrame*) reads GetMapLineMatches(), the shim's copy of `mls`: the driver fills both on entry.
#pragma once
#include <list>
#include <map>

#include "match_standins.hpp"

// The Eigen expressions of MapLine::UpdateAverageDir that oracle/shim/eigenshim.hpp lacks (head, tail, norm, +, -, scalar *), coefficient-wise and in the order
// oracle/shim/minieigen restates them (norm: the squares summed first to last).  Unpinned: Eigen is absent.  Vector3d / Vector6d are redirected to these in the
// extracted unit and the driver only.
namespace nl_shim {
struct V3X : Eigen::Vector3d {
    V3X() {}
    V3X(double x, double y, double z) : Eigen::Vector3d(x, y, z) {}
    V3X(const Eigen::Vector3d& o) : Eigen::Vector3d(o) {}
    double norm() const { double s = d[0] * d[0]; s += d[1] * d[1]; s += d[2] * d[2]; return std::sqrt(s); }
};
inline V3X operator+(const Eigen::Vector3d& a, const Eigen::Vector3d& b) { return V3X(a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2]); }
inline V3X operator-(const Eigen::Vector3d& a, const Eigen::Vector3d& b) { return V3X(a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2]); }
inline V3X operator*(double s, const Eigen::Vector3d& a) { return V3X(s * a.d[0], s * a.d[1], s * a.d[2]); }
struct V6X : Eigen::Matrix<double, 6, 1> {
    V6X() {}
    V6X(const Eigen::Matrix<double, 6, 1>& o) : Eigen::Matrix<double, 6, 1>(o) {}
    V3X head(int) const { return V3X(d[0], d[1], d[2]); }
    V3X tail(int) const { return V3X(d[3], d[4], d[5]); }
};
}  // namespace nl_shim
namespace Eigen { using nl_shim::operator+; using nl_shim::operator-; using nl_shim::operator*; }

namespace Planar_SLAM {
using nl_shim::V3X;
using nl_shim::V6X;

class KeyFrameX;
class NewLine;

class Map {
public:
    void AddMapLine(MapLine*) {}
    std::mutex mMutexPointCreation;
};

class KeyFrameX : public KeyFrame {
public:
    std::vector<V6X> mvLines3D;
    std::vector<float> mvDepthLine;
    std::vector<NewLine*> mvpMapLines;
    CopyableMutex mMutexFeatures;
    cv::Mat mK;
    float invfx = 0, invfy = 0, mfScaleFactor = 0;
    long unsigned int mnFrameId = 0;
    int slot = -1;                                   // harness: -1 the current key frame, k a neighbour
    std::vector<KeyFrameX*> neighbours;
    std::vector<KeyFrameX*> GetBestCovisibilityKeyFrames(const int& N) { (void)N; return neighbours; }
    float ComputeSceneMedianDepth(const int) { return 1.f; }   // the monocular branch (:847) is compiled, never taken
    // bodies: src/KeyFrame.cc, extracted
    V6X obtain3DLine(const int& i);
    void AddMapLine(NewLine* pML, const size_t& idx);
    void AddMapLine(MapLine* pML, const size_t& idx) { KeyFrame::AddMapLine(pML, idx); }   // LSDmatcher::Fuse's call, on the shim's MapLine: not run here
    NewLine* GetMapLine(const size_t& idx);
    void lineDescriptorMAD(std::vector<std::vector<cv::DMatch>> line_matches, double& nn_mad, double& nn12_mad) const;
};

class NewLine : public MapLine {
public:
    NewLine(V6X& Pos, KeyFrameX* pRefKF, Map* pMap);   // body: src/MapLine.cpp:16-29, extracted
    void UpdateAverageDir();                                 // body: src/MapLine.cpp:320-367, extracted
    void AddObservation(KeyFrameX* pKF, size_t idx) {        // src/MapLine.cpp: mObservations[pKF] = idx
        mObservations[pKF] = idx;
        if (pKF->slot < 0) idx1 = (int)idx; else { neigh = pKF->slot; idx2 = (int)idx; }
    }
    void ComputeDistinctiveDescriptors() {}
    // what the two bodies touch (include/MapLine.h)
    long int mnFirstKFid, mnFirstFrame;
    int nObs;
    long unsigned int mnTrackReferenceForFrame, mnLastFrameSeen, mnBALocalForKF, mnFuseCandidateForKF, mnLoopLineForKF, mnCorrectedByKF, mnCorrectedReference, mnBAGlobalForKF;
    KeyFrameX* mpRefKF;
    int mnVisible, mnFound;
    bool mbBad;
    NewLine* mpReplaced;
    Map* mpMap;
    V6X mWorldPos;
    V3X mNormalVector;
    std::map<KeyFrameX*, size_t> mObservations;
    CopyableMutex mMutexFeatures;
    static long unsigned int nNextId;
    int neigh = -1, idx1 = -1, idx2 = -1;                    // harness
};

class LocalMapping {
public:
    void CreateNewMapLines2();
    cv::Mat ComputeF12(KeyFrameX*& pKF1, KeyFrameX*& pKF2) { (void)pKF1; (void)pKF2; return cv::Mat(); }   // its result is unused by the line path
    bool CheckNewKeyFrames() { return false; }
    bool mbMonocular = false;
    KeyFrameX* mpCurrentKeyFrame = nullptr;
    Map* mpMap = nullptr;
    std::list<NewLine*> mlpRecentAddedMapLines;
};

}  // namespace Planar_SLAM

namespace Planar_SLAM { typedef MapLine ShimMapLine; }
#define KeyFrame KeyFrameX
#include "LSDmatcher.h"   // the reference's own, declared over KeyFrameX and the shim's MapLine in every unit
#ifdef NEW_LINES_EXTRACT
#define MapLine NewLine
#define Vector3d V3X
#define Vector6d V6X
#endif
