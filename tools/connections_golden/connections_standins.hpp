// Stand-ins for the classes KeyFrame::UpdateConnections (reference src/KeyFrame.cc:298-432), AddConnection (:132-145), UpdateBestCovisibles (:147-166) and AddChild
// (:434-438) touch: exactly the members those lines use, nothing of the reference's own text.  Force-included ahead of the extracted lines by
// tools/gen_golden_connections.py.
#pragma once
#include <algorithm>
#include <cstddef>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <vector>

using namespace std;

namespace Planar_SLAM {

class KeyFrame;

class MapPoint {
public:
    bool bad = false;
    map<KeyFrame*, size_t> observations;
    bool isBad() { return bad; }
    map<KeyFrame*, size_t> GetObservations() { return observations; }
};

class MapLine {};
class MapPlane {};

class KeyFrame {
public:
    void AddConnection(KeyFrame* pKF, const int& weight);
    void UpdateBestCovisibles();
    void UpdateConnections();
    void AddChild(KeyFrame* pKF);

    long unsigned int mnId = 0;
    vector<MapPoint*> mvpMapPoints;
    vector<MapLine*> mvpMapLines;
    vector<MapPlane*> mvpMapPlanes;
    map<KeyFrame*, int> mConnectedKeyFrameWeights;
    vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    vector<int> mvOrderedWeights;
    bool mbFirstConnection = true;
    KeyFrame* mpParent = NULL;
    set<KeyFrame*> mspChildrens;
    mutex mMutexConnections, mMutexFeatures;
};

}  // namespace Planar_SLAM
