// Stand-ins for the classes the reference's key-frame insertion touches: the end of Tracking::Track (src/Tracking.cc:1973-2003, :321-336), NeedNewKeyFrame
// (:2049-2137), CreateNewKeyFrame (:2139-2285), the head of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:123-157), KeyFrame::TrackedMapPoints
// (src/KeyFrame.cc:259-284), MapPoint::AddObservation (src/MapPoint.cc:103-114) and MapLine::AddObservation (src/MapLine.cpp:91-100).  Exactly the members those
// lines use, nothing of the reference's own text.  Force-included ahead of the extracted lines by tools/gen_golden_keyframe.py.  mnPlaneNum is 0: the plane loop of
// CreateNewKeyFrame compiles and does not run.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <vector>

using namespace std;

#ifndef KEYFRAME_STANDINS_HAVE_CV_MAT   // tests/adapter_shim/adapter_keyframe_main.cpp brings the test image's stand-in of OpenCV
namespace cv { struct Mat {}; }
#endif
struct Vector6d {};

namespace Planar_SLAM {

class KeyFrame;
class Map;
class Frame;

struct System { enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 }; };
class KeyFrameDatabase {};
class PointCloudMapping { public: void print() {} };

class MapPoint {
public:
    MapPoint() {}
    MapPoint(const cv::Mat&, KeyFrame*, Map*) {}
    void AddObservation(KeyFrame* pKF, size_t idx);
    int Observations() { return nObs; }
    bool isBad() { return bad; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    void IncreaseFound(int n = 1) {}
    void ComputeDistinctiveDescriptors() {}
    void UpdateNormalAndDepth() {}
    bool bad = false;
    int nObs = 0;
    map<KeyFrame*, size_t> mObservations;
    mutex mMutexFeatures;
};

class MapLine {
public:
    MapLine() {}
    MapLine(const Vector6d&, KeyFrame*, Map*) {}
    void AddObservation(KeyFrame* pKF, size_t idx);
    int Observations() { return nObs; }
    bool isBad() { return bad; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    void IncreaseFound(int n = 1) {}
    void ComputeDistinctiveDescriptors() {}
    void UpdateAverageDir() {}
    bool bad = false;
    int nObs = 0;
    map<KeyFrame*, size_t> mObservations;
    mutex mMutexFeatures;
};

class MapPlane {
public:
    MapPlane(const cv::Mat&, KeyFrame*, Map*) {}
    void AddObservation(KeyFrame*, int) {}
    void AddParObservation(KeyFrame*, int) {}
    void AddVerObservation(KeyFrame*, int) {}
    void UpdateCoefficientsAndPoints() {}
};

class Map {
public:
    long unsigned int KeyFramesInMap() { return n_key_frames; }
    void AddMapPoint(MapPoint* p) { new_points.push_back(p); }
    void AddMapLine(MapLine* p) { new_lines.push_back(p); }
    void AddMapPlane(MapPlane*) {}
    long unsigned int MapPlanesInMap() { return 0; }
    long unsigned int n_key_frames = 0;
    vector<MapPoint*> new_points;
    vector<MapLine*> new_lines;
};

class Frame {
public:
    void UpdatePoseMatrices() {}
    cv::Mat UnprojectStereo(const int&) { return cv::Mat(); }
    Vector6d obtain3DLine(const int&) { return Vector6d(); }
    cv::Mat ComputePlaneWorldCoeff(const int&) { return cv::Mat(); }
    long unsigned int mnId = 0;
    int N = 0, NL = 0, mnPlaneNum = 0;
    bool mbNewPlane = false;
    KeyFrame* mpReferenceKF = NULL;
    vector<MapPoint*> mvpMapPoints;
    vector<bool> mvbOutlier;
    vector<float> mvDepth, mvuRight;
    vector<MapLine*> mvpMapLines;
    vector<bool> mvbLineOutlier;
    vector<float> mvDepthLine;
    vector<MapPlane*> mvpMapPlanes, mvpParallelPlanes, mvpVerticalPlanes;
    vector<bool> mvbPlaneOutlier;
};

class KeyFrame {
public:
    KeyFrame() {}
    KeyFrame(Frame& F, Map*, KeyFrameDatabase*) : N(F.N), mvuRight(F.mvuRight), mvpMapPoints(F.mvpMapPoints), mvpMapLines(F.mvpMapLines) {}
    // a key frame made with `new` lands where the driver wants it, so that pointer order is the case's kf_rank
    static void* next_slot;
    static void* operator new(size_t) { return next_slot; }
    static void* operator new(size_t, void* p) { return p; }
    static void operator delete(void*) {}
    int TrackedMapPoints(const int& minObs);
    void AddMapPoint(MapPoint* p, const size_t& idx) { mvpMapPoints[idx] = p; }
    void AddMapLine(MapLine* p, const size_t& idx) { mvpMapLines[idx] = p; }
    void AddMapPlane(MapPlane*, const int&) {}
    vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    vector<MapLine*> GetMapLineMatches() { return mvpMapLines; }
    vector<MapPlane*> GetMapPlaneMatches() { return vector<MapPlane*>(); }
    void ComputeBoW() {}
    int N = 0;
    vector<float> mvuRight;
    vector<MapPoint*> mvpMapPoints;
    vector<MapLine*> mvpMapLines;
    mutex mMutexFeatures;
};

class LocalMapping {
public:
    bool isStopped() { return stopped; }
    bool stopRequested() { return false; }
    bool AcceptKeyFrames() { return accepts; }
    void InterruptBA() { interrupted = true; }
    int KeyframesInQueue() { return queued; }
    bool SetNotStop(bool) { return true; }
    void InsertKeyFrame(KeyFrame* pKF) { inserted = pKF; }
    void ProcessNewKeyFrameHead();
    bool stopped = false, accepts = false, interrupted = false;
    int queued = 0;
    KeyFrame* inserted = NULL;
    KeyFrame* mpCurrentKeyFrame = NULL;
    list<MapPoint*> mlpRecentAddedMapPoints;
    list<MapLine*> mlpRecentAddedMapLines;
};

class Tracking {
public:
    void CountInliers();
    void CleanVOMatches();
    bool NeedNewKeyFrame();
    void CreateNewKeyFrame();
    int mSensor = System::RGBD;
    bool mbOnlyTracking = false;
    Frame mCurrentFrame;
    LocalMapping* mpLocalMapper = NULL;
    Map* mpMap = NULL;
    KeyFrameDatabase* mpKeyFrameDB = NULL;
    KeyFrame* mpReferenceKF = NULL;
    KeyFrame* mpLastKeyFrame = NULL;
    shared_ptr<PointCloudMapping> mpPointCloudMapping = make_shared<PointCloudMapping>();
    int mMinFrames = 0, mMaxFrames = 0;
    float mThDepth = 0;
    int mnMatchesInliers = 0;
    unsigned int mnLastKeyFrameId = 0, mnLastRelocFrameId = 0;
};

}  // namespace Planar_SLAM
