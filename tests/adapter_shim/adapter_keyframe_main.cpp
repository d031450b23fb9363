// tests/adapter_shim/adapter_keyframe_main.cpp — TEST INFRASTRUCTURE.  Tracking::NeedNewKeyFrame and Tracking::CreateNewKeyFrame of include/planar_adapters.hpp
// (PLANAR_ADAPTERS_WITH_KEYFRAME) executed on the stand-in classes of tools/keyframe_golden/keyframe_standins.hpp, by the fixture generator's own driver
// (tools/keyframe_golden/ref_keyframe_main.cpp; the int32 stream of tests/keyframe_cases.py stream), so input and output are those of the fixture.  What the
// generator compiles from the reference's lines is here either the adapter (the two functions under test) or the stand-in's own statement of what the reference's
// do: the two AddObservation, the count of mnMatchesInliers that Track() runs before the decision.  The clean step is left EMPTY on purpose: the cleaned matches the
// fixture holds must then come from the adapter's call.
//   adapter_keyframe <in.bin> <out.bin>
#include <opencv2/core/core.hpp>
#define KEYFRAME_STANDINS_HAVE_CV_MAT
#include "../../tools/keyframe_golden/keyframe_standins.hpp"

namespace Planar_SLAM {
// one entry per key frame; two counts for an observation with a right coordinate, one otherwise
void MapPoint::AddObservation(KeyFrame* pKF, size_t idx) {
    if (!mObservations.insert(std::make_pair(pKF, idx)).second) return;
    nObs += pKF->mvuRight[idx] >= 0 ? 2 : 1;
}
void MapLine::AddObservation(KeyFrame* pKF, size_t idx) {
    if (mObservations.insert(std::make_pair(pKF, idx)).second) nObs += 1;
}
// matched, not an outlier and, unless only tracking, observed
void Tracking::CountInliers() {
    mnMatchesInliers = 0;
    for (int i = 0; i < mCurrentFrame.N; i++) {
        MapPoint* p = mCurrentFrame.mvpMapPoints[i];
        if (p && !mCurrentFrame.mvbOutlier[i] && (mbOnlyTracking || p->Observations() > 0)) mnMatchesInliers++;
    }
    for (int i = 0; i < mCurrentFrame.NL; i++) {
        MapLine* p = mCurrentFrame.mvpMapLines[i];
        if (p && !mCurrentFrame.mvbLineOutlier[i] && (mbOnlyTracking || p->Observations() > 0)) mnMatchesInliers++;
    }
}
void Tracking::CleanVOMatches() {}
void LocalMapping::ProcessNewKeyFrameHead() { std::fprintf(stderr, "the head of ProcessNewKeyFrame has no adapter\n"); std::exit(4); }
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_KEYFRAME
#include "planar_adapters.hpp"

#include "../../tools/keyframe_golden/ref_keyframe_main.cpp"
