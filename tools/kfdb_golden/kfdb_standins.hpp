// tools/kfdb_golden/kfdb_standins.hpp — TEST INFRASTRUCTURE for tools/gen_golden_kfdb.py.  Force-included in front of the reference's src/KeyFrameDatabase.cc, which is
// compiled where it lies with its own include/KeyFrameDatabase.h and include/ORBVocabulary.h: the include guards of KeyFrame.h and Frame.h are defined here, so the
// two classes below stand in for them.  They hold what the database reads and writes: mBowVec, mnId, the six query members (zero-initialised; the reference leaves
// mLoopScore and mRelocScore uninitialised), GetConnectedKeyFrames and GetBestCovisibilityKeyFrames.
#pragma once
#define KEYFRAME_H
#define FRAME_H
#include <list>
#include <mutex>
#include <set>
#include <vector>

#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

using namespace std;   // include/KeyFrameDatabase.h names list<> without std::, as the real KeyFrame.h lets it

namespace Planar_SLAM {

class KeyFrame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
    std::set<KeyFrame*> connected;        // GetConnectedKeyFrames()
    std::vector<KeyFrame*> covisible;     // mvpOrderedConnectedKeyFrames
    std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        if ((int)covisible.size() < N) return covisible;
        return std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
    }
};

class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};

}  // namespace Planar_SLAM
