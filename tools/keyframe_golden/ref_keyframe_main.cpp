// Driver of tools/gen_golden_keyframe.py: builds the stand-in maps and frames of one case from the int32 stream tests/keyframe_cases.py::stream writes (floats as
// their bits), runs the reference's lines (compiled from the real text ahead of this file) and writes what they left as int32.  The key frames of a map live in ONE
// array and key frame k sits at position kf_rank[k] (one further up where a new key frame is to land at or below it), so pointer order - the order of
// std::map<KeyFrame*, size_t> - is the case's rank; KeyFrame::operator new puts the key frame CreateNewKeyFrame makes at new_rank.
//   ref_keyframe in.bin out.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>

using namespace Planar_SLAM;

void* KeyFrame::next_slot = nullptr;

static std::vector<int32_t> in, out;
static size_t at = 0;
static int32_t next() { if (at >= in.size()) { fprintf(stderr, "short input\n"); exit(2); } return in[at++]; }
static float nextf() { const int32_t v = next(); float f; memcpy(&f, &v, 4); return f; }

struct OneMap {
    int nk = 0, npt = 0, nm = 0, new_rank = -1;
    KeyFrame* store = nullptr;
    std::vector<KeyFrame*> kf;
    std::deque<MapPoint> pts;
    std::deque<MapLine> mls;
    Map map;
    int kf_id(KeyFrame* p) const { for (size_t k = 0; k < kf.size(); k++) if (kf[k] == p) return (int)k; return -9; }
    int pt_id(MapPoint* p) const {
        if (!p) return -1;
        for (int i = 0; i < npt; i++) if (&pts[i] == p) return i;
        for (size_t i = 0; i < map.new_points.size(); i++) if (map.new_points[i] == p) return npt + (int)i;
        return -9;
    }
    int ml_id(MapLine* p) const {
        if (!p) return -1;
        for (int i = 0; i < nm; i++) if (&mls[i] == p) return i;
        for (size_t i = 0; i < map.new_lines.size(); i++) if (map.new_lines[i] == p) return nm + (int)i;
        return -9;
    }
};

static void read_map(OneMap& m) {
    m.nk = next(); m.npt = next(); m.nm = next(); m.new_rank = next();
    m.store = (KeyFrame*)::operator new(sizeof(KeyFrame) * (m.nk + 1));
    m.pts.resize(m.npt); m.mls.resize(m.nm);
    m.kf.resize(m.nk);
    for (int k = 0; k < m.nk; k++) {
        const int r = next();
        m.kf[k] = new (&m.store[r + (m.new_rank >= 0 && r >= m.new_rank)]) KeyFrame();
    }
    for (int k = 0; k < m.nk; k++) {
        const int ns = next();
        m.kf[k]->N = ns;
        for (int i = 0; i < ns; i++) { const int p = next(); m.kf[k]->mvpMapPoints.push_back(p < 0 ? NULL : &m.pts[p]); }
        m.kf[k]->mvuRight.assign(ns, 1.f);
        const int nls = next();
        for (int i = 0; i < nls; i++) { const int p = next(); m.kf[k]->mvpMapLines.push_back(p < 0 ? NULL : &m.mls[p]); }
    }
    for (int p = 0; p < m.npt; p++) m.pts[p].bad = next() != 0;
    for (int p = 0; p < m.npt; p++) m.pts[p].nObs = next();
    for (int p = 0; p < m.npt; p++) { const int n = next(); for (int i = 0; i < n; i++) m.pts[p].mObservations[m.kf[next()]] = 0; }
    for (int p = 0; p < m.nm; p++) m.mls[p].bad = next() != 0;
    for (int p = 0; p < m.nm; p++) m.mls[p].nObs = next();
    for (int p = 0; p < m.nm; p++) { const int n = next(); for (int i = 0; i < n; i++) m.mls[p].mObservations[m.kf[next()]] = 0; }
    m.map.n_key_frames = (long unsigned int)m.nk;
}

static void read_points(OneMap& m, Frame& F, bool outliers, bool uright) {
    F.N = next();
    for (int i = 0; i < F.N; i++) { const int p = next(); F.mvpMapPoints.push_back(p < 0 ? NULL : &m.pts[p]); }
    F.mvbOutlier.assign(F.N, false);
    if (outliers) for (int i = 0; i < F.N; i++) F.mvbOutlier[i] = next() != 0;
    for (int i = 0; i < F.N; i++) F.mvDepth.push_back(nextf());
    F.mvuRight.assign(F.N, 1.f);
    if (uright) for (int i = 0; i < F.N; i++) F.mvuRight[i] = nextf();
}

static void read_lines(OneMap& m, Frame& F, bool outliers, bool depth) {
    F.NL = next();
    for (int i = 0; i < F.NL; i++) { const int p = next(); F.mvpMapLines.push_back(p < 0 ? NULL : &m.mls[p]); }
    F.mvbLineOutlier.assign(F.NL, false);
    if (outliers) for (int i = 0; i < F.NL; i++) F.mvbLineOutlier[i] = next() != 0;
    F.mvDepthLine.assign(F.NL, -1.f);
    if (depth) for (int i = 0; i < F.NL; i++) F.mvDepthLine[i] = nextf();
}

static void write_lists(OneMap& m) {
    for (int p = 0; p < m.npt; p++) {
        out.push_back(m.pts[p].nObs); out.push_back((int32_t)m.pts[p].mObservations.size());
        for (auto& e : m.pts[p].mObservations) out.push_back(m.kf_id(e.first));
    }
    for (int p = 0; p < m.nm; p++) {
        out.push_back(m.mls[p].nObs); out.push_back((int32_t)m.mls[p].mObservations.size());
        for (auto& e : m.mls[p].mObservations) out.push_back(m.kf_id(e.first));
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    in.resize(bytes / 4);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);

    const int kind = next(), G = next();
    std::vector<OneMap> maps(G);
    for (OneMap& m : maps) read_map(m);
    const int n = next();
    for (int b = 0; b < n; b++) {
        OneMap& m = maps[next()];
        LocalMapping mapper;
        if (kind == 0) {                                             // the end of Track: count, clean, decide
            Tracking t;
            t.mpLocalMapper = &mapper; t.mpMap = &m.map;
            t.mpReferenceKF = m.kf[next()];
            Frame& F = t.mCurrentFrame;
            read_points(m, F, true, false);
            read_lines(m, F, true, false);
            const uint32_t lo = (uint32_t)next(), hi = (uint32_t)next();
            F.mnId = ((long unsigned int)hi << 32) | lo;
            t.mnLastRelocFrameId = (unsigned int)next(); t.mnLastKeyFrameId = (unsigned int)next(); t.mMaxFrames = next(); t.mMinFrames = next();
            t.mThDepth = nextf();
            m.map.n_key_frames = (long unsigned int)next();
            const int planes = next(), flags = next();
            mapper.queued = next();
            t.mbOnlyTracking = (flags & 1) != 0; mapper.stopped = (flags & 2) != 0; mapper.accepts = (flags & 4) != 0; F.mbNewPlane = (flags & 8) != 0;
            t.CountInliers();
            t.mnMatchesInliers += planes;
            t.CleanVOMatches();
            const bool need = t.NeedNewKeyFrame();
            out.push_back(need); out.push_back(mapper.interrupted); out.push_back(t.mnMatchesInliers);
            for (int i = 0; i < F.N; i++) out.push_back(m.pt_id(F.mvpMapPoints[i]));
            for (int i = 0; i < F.N; i++) out.push_back(F.mvbOutlier[i]);
            for (int i = 0; i < F.NL; i++) out.push_back(m.ml_id(F.mvpMapLines[i]));
            for (int i = 0; i < F.NL; i++) out.push_back(F.mvbLineOutlier[i]);
        } else if (kind == 1) {                                      // CreateNewKeyFrame
            Tracking t;
            t.mpLocalMapper = &mapper; t.mpMap = &m.map;
            Frame& F = t.mCurrentFrame;
            read_points(m, F, false, true);
            read_lines(m, F, false, true);
            t.mThDepth = nextf();
            F.mnId = (long unsigned int)next();
            KeyFrame::next_slot = &m.store[m.new_rank];
            t.CreateNewKeyFrame();
            KeyFrame* k = mapper.inserted;
            out.push_back(k == (KeyFrame*)&m.store[m.new_rank] && t.mpReferenceKF == k && F.mpReferenceKF == k && t.mpLastKeyFrame == k &&
                          t.mnLastKeyFrameId == (unsigned int)F.mnId);
            if (!k) return 3;
            for (int i = 0; i < F.N; i++) out.push_back(m.pt_id(F.mvpMapPoints[i]));
            for (int i = 0; i < F.N; i++) out.push_back(m.pt_id(k->mvpMapPoints[i]));
            out.push_back((int32_t)m.map.new_points.size());
            for (MapPoint* p : m.map.new_points) {
                out.push_back(p->mObservations.count(k) ? (int32_t)p->mObservations[k] : -1); out.push_back(p->nObs); out.push_back((int32_t)p->mObservations.size());
            }
            for (int i = 0; i < F.NL; i++) out.push_back(m.ml_id(F.mvpMapLines[i]));
            for (int i = 0; i < F.NL; i++) out.push_back(m.ml_id(k->mvpMapLines[i]));
            out.push_back((int32_t)m.map.new_lines.size());
            for (MapLine* p : m.map.new_lines) {
                out.push_back(p->mObservations.count(k) ? (int32_t)p->mObservations[k] : -1); out.push_back(p->nObs); out.push_back((int32_t)p->mObservations.size());
            }
        } else {                                                     // the head of ProcessNewKeyFrame
            KeyFrame* k = m.kf[next()];
            const int ns = next();
            if (ns != (int)k->mvpMapPoints.size()) return 3;
            for (int i = 0; i < ns; i++) k->mvuRight[i] = nextf();
            mapper.mpCurrentKeyFrame = k;
            mapper.ProcessNewKeyFrameHead();
            write_lists(m);
            out.push_back((int32_t)mapper.mlpRecentAddedMapPoints.size());
            for (MapPoint* p : mapper.mlpRecentAddedMapPoints) out.push_back(m.pt_id(p));
            out.push_back((int32_t)mapper.mlpRecentAddedMapLines.size());
            for (MapLine* p : mapper.mlpRecentAddedMapLines) out.push_back(m.ml_id(p));
        }
    }
    if (at != in.size()) { fprintf(stderr, "long input\n"); return 2; }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
