// Stand-ins for the classes Tracking::UpdateLocalMap (reference src/Tracking.cc:2394-2552), SearchLocalPoints (:2287-2330) and SearchLocalLines (:2332-2377) touch:
// exactly the members those lines use, nothing of the reference's own text.  Force-included ahead of the extracted lines by tools/gen_golden_local_map.py.
// Frame::isInFrustum answers false and the two matchers record nothing: only the lists matter.
#pragma once
#include <cstddef>
#include <iostream>
#include <map>
#include <set>
#include <vector>

using namespace std;

namespace Planar_SLAM {

class KeyFrame;

class MapPoint {
public:
    bool bad = false;
    map<KeyFrame*, size_t> observations;
    long unsigned int mnTrackReferenceForFrame = 0, mnLastFrameSeen = 0;
    bool mbTrackInView = false;
    int visible = 0;
    bool isBad() { return bad; }
    map<KeyFrame*, size_t> GetObservations() { return observations; }
    void IncreaseVisible(int n = 1) { visible += n; }
};

class MapLine {
public:
    bool bad = false;
    long unsigned int mnTrackReferenceForFrame = 0, mnLastFrameSeen = 0;
    bool mbTrackInView = false;
    int visible = 0;
    bool isBad() { return bad; }
    void IncreaseVisible(int n = 1) { visible += n; }
};

class MapPlane {
public:
    bool isBad() { return false; }
    void IncreaseVisible(int n = 1) {}
};

class KeyFrame {
public:
    bool bad = false;
    long unsigned int mnTrackReferenceForFrame = 0;
    vector<KeyFrame*> covisible;
    set<KeyFrame*> children;
    KeyFrame* parent = NULL;
    vector<MapPoint*> points;
    vector<MapLine*> lines;
    bool isBad() { return bad; }
    vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) { return (int)covisible.size() <= N ? covisible : vector<KeyFrame*>(covisible.begin(), covisible.begin() + N); }
    set<KeyFrame*> GetChilds() { return children; }
    KeyFrame* GetParent() { return parent; }
    vector<MapPoint*> GetMapPointMatches() { return points; }
    vector<MapLine*> GetMapLineMatches() { return lines; }
};

class Frame {
public:
    long unsigned int mnId = 0;
    int N = 0;
    vector<MapPoint*> mvpMapPoints;
    vector<MapLine*> mvpMapLines;
    vector<MapPlane*> mvpMapPlanes;
    KeyFrame* mpReferenceKF = NULL;
    bool isInFrustum(MapPoint*, float) { return false; }
    bool isInFrustum(MapLine*, float) { return false; }
};

class Map {
public:
    void SetReferenceMapPoints(const vector<MapPoint*>&) {}
    void SetReferenceMapLines(const vector<MapLine*>&) {}
};

class System {
public:
    enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 };
};

class ORBmatcher {
public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) {}
    int SearchByProjection(Frame&, const vector<MapPoint*>&, const float) { return 0; }
};

class LSDmatcher {
public:
    int SearchByProjection(Frame&, const vector<MapLine*>&, const float) { return 0; }
};

class Tracking {
public:
    void SearchLocalPoints();
    void SearchLocalLines();
    void UpdateLocalMap();
    void UpdateLocalLines();
    void UpdateLocalPoints();
    void UpdateLocalKeyFrames();
    Frame mCurrentFrame;
    vector<KeyFrame*> mvpLocalKeyFrames;
    vector<MapPoint*> mvpLocalMapPoints;
    vector<MapLine*> mvpLocalMapLines;
    KeyFrame* mpReferenceKF = NULL;
    Map* mpMap = NULL;
    int mSensor = System::RGBD;
    unsigned int mnLastRelocFrameId = 0;
};

}  // namespace Planar_SLAM
