// tools/horn_ransac_golden/standins.hpp — TEST INFRASTRUCTURE.  Data-holder stand-ins for the reference's KeyFrame and MapPoint, an empty ORBmatcher.h and
// DUtils/Random.h, so that the REAL src/Sim3Solver.cc and include/Sim3Solver.h compile where they lie and run in oracle/_ref/ref_horn_ransac.  Force-included
// (-include) with the real headers' include guards pre-defined.  Only the members Sim3Solver.cc touches exist; they carry the real declarations' names and types
// (include/KeyFrame.h, MapPoint.h) and return what the harness stored.  Nothing here computes, except RandomInt, which is the reference's own expression
// (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) over the C library's rand().
#pragma once
#define MAPPOINT_H
#define KEYFRAME_H
#define ORBMATCHER_H
#define __D_RANDOM__
#include <cstdlib>
#include <map>
#include <vector>

#include "horn_cv.hpp"

namespace Eigen {}   // src/Sim3Solver.cc:35 names it and uses nothing of it

namespace DUtils {
class Random {
public:
    static int RandomInt(int min, int max) {
        int d = max - min + 1;
        return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
    }
};
}  // namespace DUtils

namespace Planar_SLAM {
class KeyFrame;
class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return bad; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    // harness data
    cv::Mat mWorldPos;
    bool bad = false;
    std::map<KeyFrame*, size_t> mObservations;
};
class KeyFrame {
public:
    cv::Mat GetRotation() { return pose.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return pose.rowRange(0, 3).col(3).clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mps; }
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    cv::Mat mK;
    // harness data
    cv::Mat pose;
    std::vector<MapPoint*> mps;
};
}  // namespace Planar_SLAM
