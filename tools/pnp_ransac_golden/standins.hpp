// tools/pnp_ransac_golden/standins.hpp — TEST INFRASTRUCTURE.  Data-holder stand-ins for the reference's Frame and MapPoint and for DUtils/Random.h, so that the
// REAL src/PnPsolver.cc and include/PnPsolver.h compile where they lie and run in oracle/_ref/ref_pnp_ransac.  Force-included (-include) with the real headers'
// include guards pre-defined.  Only the members PnPsolver.cc touches exist; they carry the real declarations' names and types (include/Frame.h, MapPoint.h) and
// return what the harness stored.  Nothing here computes, except RandomInt, which is the reference's own expression (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) over
// the C library's rand().
#pragma once
#define MAPPOINT_H
#define FRAME_H
#define __D_RANDOM__
#include <cstdlib>
#include <vector>

#include "pnp_cv.hpp"

using namespace std;   // include/PnPsolver.h names vector unqualified, on the strength of the using-directive in the real Frame.h

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
class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return bad; }
    // harness data
    cv::Mat mWorldPos;
    bool bad = false;
};
class Frame {
public:
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<float> mvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0;   // static in the real class
};
}  // namespace Planar_SLAM
