// planar_adapters.hpp — drop-in C++ classes / member functions with the reference's own signatures over the C ABI (planar_abi.h).
//
// Build PlanarSLAM with these instead of src/ORBextractor.cc, src/PlaneExtractor.cpp, src/LSDextractor.cpp, src/ORBmatcher.cc,
// src/LSDmatcher.cpp, src/PlaneMatcher.cpp and the two pose functions of src/Optimizer.cc, and link libplanar_hip.so.
//   Planar_SLAM::ORBextractor   <- include/ORBextractor.h:45-112, src/ORBextractor.cc                 (always)
//   PlaneDetection              <- include/PlaneExtractor.h:36-56, src/PlaneExtractor.cpp             (always)
//   Planar_SLAM::LineSegment    <- include/LSDextractor.h:344-352, src/LSDextractor.cpp               (PLANAR_ADAPTERS_WITH_LINES)
//   ORBmatcher::Fuse / LSDmatcher::Fuse (search on the device, map edits as in the reference)         (PLANAR_ADAPTERS_WITH_FUSE, needs one accessor, see there)
//   LocalMapping::CreateNewMapPoints up to the candidate list (planar_adapter::CreateNewMapPoints)   (PLANAR_ADAPTERS_WITH_NEW_POINTS)
//   Planar_SLAM::KeyFrameDatabase <- include/KeyFrameDatabase.h:42-70, src/KeyFrameDatabase.cc         (PLANAR_ADAPTERS_WITH_KFDB)
//   Tracking::UpdateLocalMap                                                                          (PLANAR_ADAPTERS_WITH_LOCAL_MAP)
//   KeyFrame::UpdateConnections                                                                       (PLANAR_ADAPTERS_WITH_CONNECTIONS)
//   Tracking::NeedNewKeyFrame / Tracking::CreateNewKeyFrame                                           (PLANAR_ADAPTERS_WITH_KEYFRAME)
//   ORBmatcher::SearchByBoW(KF, KF) / SearchBySim3 / SearchByProjection(KF, Scw) / Fuse(KF, Scw)      (PLANAR_ADAPTERS_WITH_LOOP_MATCHERS)
//   Optimizer::OptimizeSim3                                                                           (PLANAR_ADAPTERS_WITH_SIM3_OPT)
//   Planar_SLAM::Sim3Solver <- include/Sim3Solver.h, src/Sim3Solver.cc                                  (PLANAR_ADAPTERS_WITH_SIM3_SOLVER)
//   Planar_SLAM::PnPsolver  <- include/PnPsolver.h, src/PnPsolver.cc                                    (PLANAR_ADAPTERS_WITH_PNP_SOLVER)
//   Optimizer::OptimizeEssentialGraph                                                                 (PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH)
//   Optimizer::BundleAdjustment / GlobalBundleAdjustemnt                                              (PLANAR_ADAPTERS_WITH_GLOBAL_BA)
//   ORBmatcher / LSDmatcher / PlaneMatcher / Optimizer member functions                                (PLANAR_ADAPTERS_WITH_TRACKING:
//       include this header AFTER the reference's Frame.h, KeyFrame.h, MapPoint.h, MapLine.h, MapPlane.h, ORBmatcher.h, LSDmatcher.h,
//       PlaneMatcher.h and Optimizer.h; it then DEFINES the member functions those headers declare - gather the Frame fields into flat
//       arrays, call the ABI, scatter the result back)
//
// Threading and lifetime.  The reference starts three std::threads per Frame (src/Frame.cc:90-95: ExtractLSD / ExtractORB / ComputePlanes),
// copies Frames (and the PlaneDetection inside them) by value (src/Tracking.cc:177) and calls LineSegment::ExtractLineSegment through a
// pointer it never initialises (include/Frame.h:123, src/Frame.cc:172).  Therefore NO adapter object owns a device resource: contexts and
// plans live in one process-wide runtime (planar_adapter::Runtime), one context + stream + mutex per ROLE (points, lines, planes,
// tracking), so the three extraction threads run concurrently and nothing is created or leaked per frame or per thread; plans are cached
// by image size (and ORB parameters).  The adapter classes hold only host data and are freely copyable.
//
// Shared parts (namespace planar_adapter, right below the runtime; every section is composed of them):
//   on_lane(role, "planar_xxx", call)      the one locked call: the role's lane, its mutex, the call on its context, the report through ok()
//   mat_to_array / array_to_mat / rt_to_array / vec3_to_array, copy_scale_factors, copy_desc_rows, copy_keypoints    poses, scale tables, descriptor rows, key points
//   ViewGather                             owner of one planar_frame_view and its storage, filled by parts (add_keys, add_desc, add_u_right, add_pose, ...): a part that
//                                          names a member of a reference class is a template and is instantiated only by the sections that read that member
//   PointGather                            a list of MapPoint* as usable / xw, plus normals, descriptors and distance range where a section asks for them
//   tri_camera, plane_pose_params, sim3_entry_matches, apply_fuse_edits, UNTOUCHED / NOT_IN_KF2
#pragma once
#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "planar_abi.h"

namespace planar_adapter {

enum Role { POINTS = 0, LINES = 1, PLANES = 2, TRACKING = 3, NROLES = 4 };

class Runtime {
public:
    static Runtime& get() { static Runtime r; return r; }           // destroyed at process exit: plans first, then contexts
    static void complain(const char* what) { std::fprintf(stderr, "planar (%s): %s\n", what, planar_last_error()); }
    struct Lane { std::mutex mu; planar_ctx* ctx = nullptr; };
    // the role's context (created on first use) - hold lane(role).mu while a call on it is in flight
    Lane& lane(Role r) {
        Lane& l = lanes_[r];
        std::lock_guard<std::mutex> g(create_mu_);
        if (!l.ctx && planar_ctx_create(&l.ctx, device_) != PLANAR_OK) { l.ctx = nullptr; complain("planar_ctx_create"); }   // (no exceptions: this runs on the threads Frame's constructor spawns; the calls on a null context fail and degrade)
        return l;
    }
    typedef std::tuple<int, int, int, int, int, int, int> OrbKey;   // w, h, nfeatures, scale * 1e6, nlevels, ini, min
    planar_orb* orb(const planar_orb_params& p, int w, int h) {     // call with lane(POINTS).mu held
        const OrbKey k(w, h, p.nfeatures, (int)(p.scale_factor * 1e6f), p.nlevels, p.ini_th_fast, p.min_th_fast);
        auto it = orbs_.find(k);
        if (it != orbs_.end()) return it->second;
        planar_orb* o = nullptr;
        if (planar_orb_create(lanes_[POINTS].ctx, &p, w, h, 1, &o) != PLANAR_OK) { complain("planar_orb_create"); return nullptr; }
        return orbs_[k] = o;
    }
    planar_lsd* lsd(int w, int h) {                                 // call with lane(LINES).mu held
        auto it = lsds_.find({w, h});
        if (it != lsds_.end()) return it->second;
        planar_lsd* o = nullptr;
        if (planar_lsd_create(lanes_[LINES].ctx, w, h, 1, &o) != PLANAR_OK) { complain("planar_lsd_create"); return nullptr; }
        return lsds_[{w, h}] = o;
    }
    planar_peac* peac(int w, int h) {                               // call with lane(PLANES).mu held
        auto it = peacs_.find({w, h});
        if (it != peacs_.end()) return it->second;
        planar_peac* o = nullptr;
        // (a size the plane path does not support - more than ~10 900 blocks of 10x10: 1280x720 fits since round 6, 1920x1080 does not - is reported ONCE: the failed size is
        //  remembered as a null handle, later frames of that size track without planes without repeating the message; INTEGRATION.md "Frame sizes")
        if (planar_peac_create(lanes_[PLANES].ctx, w, h, 1, &o) != PLANAR_OK) { complain("planar_peac_create"); o = nullptr; }
        return peacs_[{w, h}] = o;
    }
    planar_plane_clouds* clouds(int w, int h) {                     // call with lane(PLANES).mu held
        auto it = clouds_.find({w, h});
        if (it != clouds_.end()) return it->second;
        planar_plane_clouds* o = nullptr;
        // 8192 voxels of 0.1 m per pass (a frame with more goes plane by plane); frames of more than 2^19 pixels (1280x720) carry 20 bits of pixel in a sort word: 4096 voxels per pass
        const int max_voxels = (long long)w * h > (1ll << 19) ? 4096 : 8192;
        if (planar_plane_clouds_create(lanes_[PLANES].ctx, w, h, 1, max_voxels, &o) != PLANAR_OK) { complain("planar_plane_clouds_create"); o = nullptr; }   // (sizes beyond 2^20 pixels: reported once)
        return clouds_[{w, h}] = o;
    }
    void set_device(int d) { device_ = d; }
private:
    Runtime() {}
    ~Runtime() {
        for (auto& kv : orbs_) planar_orb_destroy(kv.second);
        for (auto& kv : lsds_) planar_lsd_destroy(kv.second);
        for (auto& kv : peacs_) planar_peac_destroy(kv.second);
        for (auto& kv : clouds_) planar_plane_clouds_destroy(kv.second);
        for (Lane& l : lanes_) if (l.ctx) planar_ctx_destroy(l.ctx);
    }
    Runtime(const Runtime&) = delete;
    Runtime& operator=(const Runtime&) = delete;
    int device_ = 0;
    std::mutex create_mu_;
    Lane lanes_[NROLES];
    std::map<OrbKey, planar_orb*> orbs_;
    std::map<std::pair<int, int>, planar_lsd*> lsds_;
    std::map<std::pair<int, int>, planar_peac*> peacs_;
    std::map<std::pair<int, int>, planar_plane_clouds*> clouds_;
};

// The reference's convention is no exceptions: its extractors run on threads Frame's constructor spawns, its matchers / optimisers on the tracking and
// local-mapping threads, none with a handler - a throw would end in std::terminate.  A failing call says so on stderr and the adapter degrades to "nothing
// found" (no key points / lines / planes / matches, the pose left alone), which the reference's own state machine handles (tracking lost -> relocalisation).
inline bool ok(int rc, const char* where) {
    if (rc == PLANAR_OK) return true;
    std::fprintf(stderr, "planar (%s): %s - degraded to \"nothing found\"\n", where, planar_last_error());
    return false;
}

// The one locked call: the role's lane, then its mutex, then the call on the lane's context, reported through ok() under the name `where`.
template <class Call> inline bool on_lane(Role role, const char* where, Call call) {
    Runtime::Lane& L = Runtime::get().lane(role);
    std::lock_guard<std::mutex> g(L.mu);
    return ok(call(L.ctx), where);
}

const int32_t UNTOUCHED = -2;      // a match slot the call did not write
const int32_t NOT_IN_KF2 = -2;     // vpMatches12[i] is set but is no (usable) feature of pKF2: takes i out of the search, nothing else

// ---- poses, scale tables, descriptor rows, key points ----
inline void mat_to_array(const cv::Mat& T, float* a) { for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) a[4 * r + c] = T.at<float>(r, c); }   // 4x4
inline cv::Mat array_to_mat(const float* a, int rows = 4, int cols = 4) { cv::Mat M(rows, cols, CV_32F); std::memcpy(M.data, a, sizeof(float) * rows * cols); return M; }
// R (3x3) to Ra[ld * r + c], t (3x1) to ta[tstep * r]: R[9] and t[3] with (3, 1), the upper rows of a 4x4 with (Tcw, 4, Tcw + 3, 4)
inline void rt_to_array(const cv::Mat& R, const cv::Mat& t, float* Ra, int ld, float* ta, int tstep) {
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Ra[ld * r + c] = R.at<float>(r, c); ta[tstep * r] = t.at<float>(r); }
}
inline void vec3_to_array(const cv::Mat& x, float* a) { for (int k = 0; k < 3; k++) a[k] = x.at<float>(k); }
inline void copy_scale_factors(float* dst, const std::vector<float>& v) { for (size_t l = 0; l < v.size() && l < PLANAR_MAX_LEVELS; l++) dst[l] = v[l]; }
inline void copy_desc_rows(uint8_t* dst, const cv::Mat& d, int rows) { for (int i = 0; i < rows; i++) std::memcpy(dst + (size_t)i * 32, d.ptr(i), 32); }
inline void copy_keypoints(void* dst, const void* src, size_t count) {      // cv::KeyPoint <-> planar_keypoint, either way
    static_assert(sizeof(cv::KeyPoint) == sizeof(planar_keypoint), "cv::KeyPoint layout");
    if (count) std::memcpy(dst, src, count * sizeof(planar_keypoint));
}

// ---- one planar_frame_view and the storage behind it, filled by parts.  Nothing is set that no part set: a view without add_keys has n = keys_un = NULL and
//      stride 1 (LSDmatcher::Fuse), one without add_pose has Tcw = NULL.  Arrays are padded to stride = max(n, 1); padded u_right is -1, everything else 0.  A copy
//      points into its own storage. ----
struct ViewGather {
    int32_t n;
    std::vector<planar_keypoint> keys;
    std::vector<float> ur;
    std::vector<uint8_t> desc, blocked;
    float Tcw[16];
    planar_frame_view view;

    ViewGather() : n(0) { std::memset(&view, 0, sizeof(view)); view.B = 1; view.stride = 1; }
    ViewGather(const ViewGather& o) { *this = o; }
    ViewGather& operator=(const ViewGather& o) {
        n = o.n; keys = o.keys; ur = o.ur; desc = o.desc; blocked = o.blocked; view = o.view;
        std::memcpy(Tcw, o.Tcw, sizeof(Tcw));
        return bind();
    }
    ViewGather& bind() {      // the view's pointers follow the storage (after a part filled it, after a copy)
        view.n = keys.empty() ? nullptr : &n; view.keys_un = keys.empty() ? nullptr : keys.data();
        view.u_right = ur.empty() ? nullptr : ur.data(); view.desc = desc.empty() ? nullptr : desc.data(); view.blocked = blocked.empty() ? nullptr : blocked.data();
        if (view.Tcw) view.Tcw = Tcw;
        return *this;
    }
    ViewGather& add_keys(const std::vector<cv::KeyPoint>& k, int count) {          // mvKeysUn; the first part: it sets n and the stride
        n = count; keys.resize(n > 0 ? n : 1); view.stride = (int32_t)keys.size();
        copy_keypoints(keys.data(), k.data(), n > 0 ? n : 0);
        return bind();
    }
    ViewGather& add_desc(const cv::Mat& d) { desc.assign((size_t)view.stride * 32, 0); copy_desc_rows(desc.data(), d, n); return bind(); }              // mDescriptors
    ViewGather& add_u_right(const std::vector<float>& v) {                          // mvuRight; -1 where it is empty
        ur.assign(view.stride, -1.f);
        if (!v.empty() && n > 0) std::copy(v.begin(), v.begin() + n, ur.begin());
        return bind();
    }
    ViewGather& add_blocked() { blocked.assign(view.stride, 0); return bind(); }    // all free; the section sets the flags
    template <class MapPointT> ViewGather& add_blocked_observed(const std::vector<MapPointT*>& mps) {       // mvpMapPoints[i] && ->Observations() > 0
        add_blocked();
        for (int i = 0; i < n; i++) if (mps[i] && mps[i]->Observations() > 0) blocked[i] = 1;
        return *this;
    }
    ViewGather& add_pose(const cv::Mat& T) { if (!T.empty()) { mat_to_array(T, Tcw); view.Tcw = Tcw; } return *this; }     // F.mTcw or pKF->GetPose()
    ViewGather& add_pose(const cv::Mat& R, const cv::Mat& t) {                      // [R | t] of GetRotation() / GetTranslation()
        rt_to_array(R, t, Tcw, 4, Tcw + 3, 4);
        Tcw[12] = Tcw[13] = Tcw[14] = 0.f; Tcw[15] = 1.f; view.Tcw = Tcw;
        return *this;
    }
    template <class T> ViewGather& add_bounds(const T& o) { view.min_x = o.mnMinX; view.max_x = o.mnMaxX; view.min_y = o.mnMinY; view.max_y = o.mnMaxY; return *this; }
    template <class T> ViewGather& add_grid(const T& o) { view.grid_w_inv = o.mfGridElementWidthInv; view.grid_h_inv = o.mfGridElementHeightInv; return *this; }
    template <class T> ViewGather& add_intrinsics(const T& o) { view.fx = o.fx; view.fy = o.fy; view.cx = o.cx; view.cy = o.cy; return *this; }
    template <class T> ViewGather& add_stereo(const T& o) { view.bf = o.mbf; view.b = o.mb; return *this; }
    ViewGather& add_intrinsics_K(const cv::Mat& K) { view.fx = K.at<float>(0, 0); view.fy = K.at<float>(1, 1); view.cx = K.at<float>(0, 2); view.cy = K.at<float>(1, 2); return *this; }
    ViewGather& add_scales(const std::vector<float>& v, bool ones_first) {          // mvScaleFactors; the two solvers fill all levels with 1.f first
        if (ones_first) std::fill_n(view.scale_factors, (int)PLANAR_MAX_LEVELS, 1.f);
        copy_scale_factors(view.scale_factors, v);
        return *this;
    }
};

// ---- a list of map points as the arrays of the entries, by parts.  add_points: `count` slots (padded to max(count, 1)), usable = v[j] != NULL && !isBad() &&
//      !excluded(v[j]), xw of the usable; a slot past the end of v counts as NULL.  The other parts fill their array for the usable points and leave zeros elsewhere;
//      kp names only the arrays that were added.  A copy points into its own storage. ----
struct NoExclusion { template <class P> bool operator()(P*) const { return false; } };
struct PointGather {
    std::vector<uint8_t> usable, desc;
    std::vector<float> xw, nrm, mn, mx;
    planar_kf_points kp;

    PointGather() { std::memset(&kp, 0, sizeof(kp)); }
    PointGather(const PointGather& o) { *this = o; }
    PointGather& operator=(const PointGather& o) { usable = o.usable; desc = o.desc; xw = o.xw; nrm = o.nrm; mn = o.mn; mx = o.mx; return bind(); }
    PointGather& bind() {
        kp.usable = usable.empty() ? nullptr : usable.data(); kp.xw = xw.empty() ? nullptr : xw.data(); kp.desc = desc.empty() ? nullptr : desc.data();
        kp.min_dist = mn.empty() ? nullptr : mn.data(); kp.max_dist = mx.empty() ? nullptr : mx.data();
        return *this;
    }
    template <class MapPointT, class Excluded> PointGather& add_points(const std::vector<MapPointT*>& v, size_t count, Excluded excluded) {
        usable.assign(count ? count : 1, 0); xw.assign(usable.size() * 3, 0.f);
        for (size_t j = 0; j < count && j < v.size(); j++) {
            MapPointT* p = v[j];
            if (!p || p->isBad() || excluded(p)) continue;
            usable[j] = 1;
            vec3_to_array(p->GetWorldPos(), &xw[3 * j]);
        }
        return bind();
    }
    template <class MapPointT> PointGather& add_points(const std::vector<MapPointT*>& v) { return add_points(v, v.size(), NoExclusion()); }
    template <class MapPointT> PointGather& add_normals(const std::vector<MapPointT*>& v) {      // GetNormal()
        nrm.assign(usable.size() * 3, 0.f);
        for (size_t j = 0; j < v.size() && j < usable.size(); j++) if (usable[j]) vec3_to_array(v[j]->GetNormal(), &nrm[3 * j]);
        return *this;
    }
    template <class MapPointT> PointGather& add_desc(const std::vector<MapPointT*>& v) {         // GetDescriptor()
        desc.assign(usable.size() * 32, 0);
        for (size_t j = 0; j < v.size() && j < usable.size(); j++) if (usable[j]) copy_desc_rows(&desc[j * 32], v[j]->GetDescriptor(), 1);
        return bind();
    }
    template <class MapPointT> PointGather& add_range(const std::vector<MapPointT*>& v) {        // GetDistanceRange(): the unscaled mfMinDistance / mfMaxDistance
        mn.assign(usable.size(), 0.f); mx.assign(usable.size(), 0.f);
        for (size_t j = 0; j < v.size() && j < usable.size(); j++) if (usable[j]) v[j]->GetDistanceRange(mn[j], mx[j]);
        return bind();
    }
};

// ---- smaller pieces ----
// the camera of CreateNewMapPoints / CreateNewMapLines, off the current key frame
template <class KeyFrameT> inline planar_tri_camera tri_camera(KeyFrameT* pKF) {
    planar_tri_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.fx = pKF->fx; cam.fy = pKF->fy; cam.cx = pKF->cx; cam.cy = pKF->cy; cam.invfx = pKF->invfx; cam.invfy = pKF->invfy; cam.scale_factor = pKF->mfScaleFactor;
    cam.n_levels = (int32_t)pKF->mvScaleFactors.size();
    copy_scale_factors(cam.scale_factors, pKF->mvScaleFactors);
    copy_scale_factors(cam.level_sigma2, pKF->mvLevelSigma2);
    return cam;
}

// the intrinsics and the six Plane.* values Config::Get<double> returns (ConfigT = Planar_SLAM::Config)
template <class ConfigT> inline planar_pose_params plane_pose_params(float fx, float fy, float cx, float cy, float bf) {
    planar_pose_params prm;
    prm.fx = fx; prm.fy = fy; prm.cx = cx; prm.cy = cy; prm.bf = bf;
    prm.angle_info = ConfigT::template Get<double>("Plane.AngleInfo"); prm.distance_info = ConfigT::template Get<double>("Plane.DistanceInfo");
    prm.parallel_info = ConfigT::template Get<double>("Plane.ParallelInfo"); prm.vertical_info = ConfigT::template Get<double>("Plane.VerticalInfo");
    prm.plane_chi = ConfigT::template Get<double>("Plane.Chi"); prm.vp_chi = ConfigT::template Get<double>("Plane.VPChi");
    return prm;
}

// vpMatches (of pKF1's features) as the entry's match array over `stride1` slots: -1 = NULL, i2 = GetIndexInKeyFrame(pKF2) where that is a feature of pKF2 and the
// matched point is not bad, NOT_IN_KF2 otherwise.  usable2 describes pKF2's own slot, so a match makes slot i2 of `side2` usable with the matched point's position.
template <class KeyFrameT, class MapPointT>
inline std::vector<int32_t> sim3_entry_matches(const std::vector<MapPointT*>& vpMatches, int n1, size_t stride1, KeyFrameT* pKF2, int n2, PointGather& side2) {
    std::vector<int32_t> match(stride1, -1);
    const int N = (int)vpMatches.size() < n1 ? (int)vpMatches.size() : n1;
    for (int i = 0; i < N; i++) {
        if (!vpMatches[i]) continue;
        const int i2 = vpMatches[i]->GetIndexInKeyFrame(pKF2);
        match[i] = (i2 >= 0 && i2 < n2 && !vpMatches[i]->isBad()) ? i2 : NOT_IN_KF2;
        if (match[i] >= 0) { side2.usable[i2] = 1; vec3_to_array(vpMatches[i]->GetWorldPos(), &side2.xw[3 * i2]); }
    }
    return match;
}

// the map edits of the two Fuse functions (src/ORBmatcher.cc:953-974, src/LSDmatcher.cpp:993-1010) on the reference's own objects: landmark j found feature idx[j];
// in_kf(i) is GetMapPoint / GetMapLine, add_to_kf(p, i) is AddMapPoint / AddMapLine
template <class KeyFrameT, class LandmarkT, class InKF, class AddToKF>
inline void apply_fuse_edits(KeyFrameT* pKF, const std::vector<LandmarkT*>& v, const std::vector<int32_t>& idx, InKF in_kf, AddToKF add_to_kf) {
    for (size_t j = 0; j < v.size(); j++) {
        if (idx[j] < 0) continue;
        LandmarkT* p = v[j];
        LandmarkT* held = in_kf(idx[j]);
        if (held) {
            if (!held->isBad()) {
                if (held->Observations() > p->Observations()) p->Replace(held);
                else held->Replace(p);
            }
        } else {
            p->AddObservation(pKF, idx[j]);
            add_to_kf(p, idx[j]);
        }
    }
}

}  // namespace planar_adapter

namespace Planar_SLAM {

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
        : nfeatures(nfeatures), scaleFactor(scaleFactor), nlevels(nlevels), iniThFAST(iniThFAST), minThFAST(minThFAST) {
        mvImagePyramid.resize(nlevels);
    }

    // Same contract as the reference operator() (src/ORBextractor.cc:1043-1105); mask is ignored there too.
    void operator()(cv::InputArray _image, cv::InputArray /*mask*/, std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors) {
        if (_image.empty()) return;
        cv::Mat image = _image.getMat();
        assert(image.type() == CV_8UC1);   // src/ORBextractor.cc:1050
        std::vector<planar_keypoint> kps;
        std::vector<uint8_t> desc;
        int32_t n = 0;
        const bool done = planar_adapter::on_lane(planar_adapter::POINTS, "ORBextractor", [&](planar_ctx*) -> int {
            planar_orb* orb = planar_adapter::Runtime::get().orb(params(), image.cols, image.rows);
            if (!orb) return PLANAR_OK;            // (said at create: no key points, the pyramid left alone)
            const int cap = planar_orb_max_keypoints(orb);
            kps.resize(cap); desc.resize((size_t)cap * 32);
            const int rc = planar_orb_extract(orb, image.data, 1, (int)image.step, (int64_t)image.step * image.rows, kps.data(), desc.data(), &n);
            for (int l = 0; l < nlevels; l++) {      // public member of the reference class (include/ORBextractor.h:85)
                int w, h;
                planar_orb_level_size(orb, l, &w, &h);
                mvImagePyramid[l].create(h, w, CV_8UC1);
                planar_orb_read_level(orb, 0, l, mvImagePyramid[l].data);
            }
            return rc;
        });
        if (!done) n = 0;
        _keypoints.resize(n);
        planar_adapter::copy_keypoints((void*)_keypoints.data(), kps.data(), n);
        if (n == 0) { _descriptors.release(); return; }
        _descriptors.create(n, 32, CV_8U);
        cv::Mat d = _descriptors.getMat();
        for (int i = 0; i < n; i++) std::memcpy(d.ptr(i), &desc[(size_t)i * 32], 32);
    }

    int GetLevels() { return nlevels; }
    float GetScaleFactor() { return (float)scaleFactor; }
    std::vector<float> GetScaleFactors() { return factors(0); }
    std::vector<float> GetInverseScaleFactors() { return factors(1); }
    std::vector<float> GetScaleSigmaSquares() { return factors(2); }
    std::vector<float> GetInverseScaleSigmaSquares() { return factors(3); }

    std::vector<cv::Mat> mvImagePyramid;

protected:
    planar_orb_params params() const { return planar_orb_params{nfeatures, (float)scaleFactor, nlevels, iniThFAST, minThFAST}; }
    std::vector<float> factors(int which) {
        // the scale tables depend only on the constructor arguments; any cached plan with these parameters can answer
        std::vector<float> v[4];
        for (auto& x : v) x.resize(nlevels);
        planar_adapter::on_lane(planar_adapter::POINTS, "ORBextractor", [&](planar_ctx*) -> int {
            planar_orb_get_scale_factors(planar_adapter::Runtime::get().orb(params(), 640, 480), v[0].data(), v[1].data(), v[2].data(), v[3].data());
            return PLANAR_OK;
        });
        return v[which];
    }
    int nfeatures; double scaleFactor; int nlevels, iniThFAST, minThFAST;
};

}  // namespace Planar_SLAM

// ---- PlaneDetection (include/PlaneExtractor.h:36-56).  Frame::ComputePlanes (src/Frame.cc:647-672) reads plane_num_,
// plane_vertices_[i], cloud.vertices[j] and plane_filter.extractedPlanes[i]->normal/center; the same members exist here.
// A PlaneDetection is a by-value member of every Frame and is copied with it: it owns no device handle, and its
// extractedPlanes pointers are re-seated on copy.
struct PlanarPlaneSeg { double normal[3], center[3], mse; int N; };
struct PlanarPlaneFilter {
    std::vector<PlanarPlaneSeg*> extractedPlanes;
    std::vector<PlanarPlaneSeg> storage;
    PlanarPlaneFilter() {}
    PlanarPlaneFilter(const PlanarPlaneFilter& o) : storage(o.storage) { reseat(); }
    PlanarPlaneFilter& operator=(const PlanarPlaneFilter& o) { if (this != &o) { storage = o.storage; reseat(); } return *this; }
    void reseat() { extractedPlanes.resize(storage.size()); for (size_t i = 0; i < storage.size(); i++) extractedPlanes[i] = &storage[i]; }
};
struct PlanarVertex { double v[3]; double operator[](int i) const { return v[i]; } };
struct ImagePointCloud { std::vector<PlanarVertex> vertices; int w = 0, h = 0; };

class PlaneDetection {
public:
    ImagePointCloud cloud;
    PlanarPlaneFilter plane_filter;
    std::vector<std::vector<int>> plane_vertices_;
    cv::Mat seg_img_, color_img_;
    int plane_num_ = 0;

    bool readColorImage(cv::Mat RGBImg) { color_img_ = RGBImg; return !(color_img_.empty() || color_img_.depth() != CV_8U); }

    // src/PlaneExtractor.cpp:26-57: keeps the depth and the intrinsics; the XYZ cloud is produced with the same FP64 arithmetic.
    bool readDepthImage(cv::Mat depthImg, cv::Mat& K, float kScaleFactor) {
        if (depthImg.empty() || depthImg.depth() != CV_16U) { std::printf("WARNING: cannot read depth image. No such a file, or the image format is not 16UC1\n"); return false; }
        depth_ = depthImg; factor_ = kScaleFactor;
        fx_ = K.at<float>(0, 0); fy_ = K.at<float>(1, 1); cx_ = K.at<float>(0, 2); cy_ = K.at<float>(1, 2);
        cloud.w = depthImg.cols; cloud.h = depthImg.rows;
        cloud.vertices.resize((size_t)cloud.w * cloud.h);
        for (int i = 0; i < depthImg.rows; i++)
            for (int j = 0; j < depthImg.cols; j++) {
                const double z = (double)depthImg.at<unsigned short>(i, j) * kScaleFactor;
                PlanarVertex& p = cloud.vertices[(size_t)i * cloud.w + j];
                p.v[0] = ((double)j - cx_) * z / fx_; p.v[1] = ((double)i - cy_) * z / fy_; p.v[2] = z;
            }
        return true;
    }

    void runPlaneDetection(int H, int W) {   // src/PlaneExtractor.cpp:59-65
        std::vector<int32_t>& labels = labels_;
        std::vector<double>& planes = planes_;
        labels.assign((size_t)W * H, -1);
        planes.assign((size_t)planar_peac_max_planes() * 8, 0.0);
        int32_t n = 0;
        if (!planar_adapter::on_lane(planar_adapter::PLANES, "PlaneDetection", [&](planar_ctx*) -> int {
                planar_peac* pp = planar_adapter::Runtime::get().peac(W, H);
                if (!pp) return PLANAR_OK;                                     // (unsupported frame size: said once, at create; no planes)
                return planar_peac_segment(pp, (const uint16_t*)depth_.data, 1, (int)(depth_.step / 2), (int64_t)(depth_.step / 2) * H, fx_, fy_, cx_, cy_, factor_,
                                           labels.data(), planes.data(), &n);
            })) { n = 0; labels.assign((size_t)W * H, -1); }
        plane_num_ = n;
        plane_vertices_.assign(n, std::vector<int>());
        for (size_t i = 0; i < labels.size(); i++) if (labels[i] >= 0) plane_vertices_[labels[i]].push_back((int)i);   // raster order, as :362-372
        plane_filter.storage.resize(n);
        for (int i = 0; i < n; i++) {
            PlanarPlaneSeg& s = plane_filter.storage[i];
            const double* p = &planes[(size_t)i * 8];
            s.N = (int)p[0]; for (int k = 0; k < 3; k++) { s.normal[k] = p[1 + k]; s.center[k] = p[4 + k]; } s.mse = p[7];
        }
        plane_filter.reseat();
        seg_img_ = cv::Mat(H, W, CV_8UC3);   // visualisation only (colours are out of scope)
    }

    // NOT a member of the reference class: the loop of Frame::ComputePlanes over the detected planes (src/Frame.cc:655-692: pcl::VoxelGrid(0.1) of every
    // plane's points, coefficient (n, -n.c), Frame::MaxPointDistanceFromPlane with its pcl::SACSegmentation refit) as one call.  In Frame::ComputePlanes:
    //     planeDetector.ComputePlaneClouds(Config::Get<double>("Plane.DistanceThreshold"), mvPlanePoints, mvPlaneCoefficients);
    // CloudT: pcl::PointCloud<pcl::PointXYZRGB> or anything with a `points` vector whose elements have float x, y, z.  Returns mnPlaneNum.
    template <class CloudT>
    int ComputePlaneClouds(double disTh, std::vector<CloudT>& planePoints, std::vector<cv::Mat>& planeCoefficients, float leaf = 0.1f) {
        const int W = cloud.w, H = cloud.h, PS = planar_peac_max_planes(), MP = 8192;
        std::vector<float> coef((size_t)PS * 4), pts((size_t)MP * 3);
        std::vector<int32_t> src(PS), off(PS + 1);
        int32_t n_in = plane_num_, n_out = 0;
        auto append = [&](int k, const float* cf, const int32_t* of, const float* pt) {     // kept plane k of a call's outputs -> mvPlanePoints / mvPlaneCoefficients
            CloudT c;
            c.points.resize(of[k + 1] - of[k]);
            for (int i = of[k]; i < of[k + 1]; i++) { auto& p = c.points[i - of[k]]; p.x = pt[(size_t)i * 3]; p.y = pt[(size_t)i * 3 + 1]; p.z = pt[(size_t)i * 3 + 2]; }
            planePoints.push_back(c);
            cv::Mat m(4, 1, CV_32F);
            for (int t = 0; t < 4; t++) m.at<float>(t, 0) = cf[(size_t)k * 4 + t];
            planeCoefficients.push_back(m);
        };
        int total = -1;                                                       // >= 0: the frame went through plane by plane, this many were kept
        const bool done = planar_adapter::on_lane(planar_adapter::PLANES, "ComputePlaneClouds", [&](planar_ctx*) -> int {
            planar_plane_clouds* pc = planar_adapter::Runtime::get().clouds(W, H);
            if (!pc) { total = 0; return PLANAR_OK; }                         // (unsupported frame size: said once, at create)
            // one call; *st = the frame's result code where the table was too small (3 = more voxels than it holds), not the message's text
            auto compute = [&](int32_t* n_kept, int32_t* st) {
                const int rc = planar_plane_clouds_compute(pc, (const uint16_t*)depth_.data, 1, (int)(depth_.step / 2), (int64_t)(depth_.step / 2) * H, fx_, fy_, cx_, cy_,
                                                           factor_, labels_.data(), planes_.data(), &n_in, disTh, leaf, n_kept, coef.data(), src.data(), off.data(),
                                                           pts.data(), nullptr, nullptr, nullptr);
                *st = 0;
                if (rc == PLANAR_ECAPACITY) planar_plane_clouds_last_status(pc, 1, st);
                return rc;
            };
            int32_t fst = 0;
            const int rc = compute(&n_out, &fst);
            if (!(rc == PLANAR_ECAPACITY && fst == 3)) return rc;
            // pcl::VoxelGrid has no voxel cap (src/Frame.cc:674-679); the frame's voxel table here has (8192 for all planes together).  The frame goes through once
            // more PLANE BY PLANE (planar_plane_clouds_set_plane_window), results appended in plane order - the very sequence of Frame::ComputePlanes' loop, every
            // plane's cloud and refit what the one-pass call would have produced.  Only a single plane of more than 8192 voxels (> 80 m^2 at the 0.1 m leaf) is
            // beyond the structure: it alone is dropped, with a message (this runs on the thread Frame's constructor spawned: no exception may leave it).
            total = 0;
            for (int i = 0; i < n_in; i++) {
                int32_t n1 = 0, pst = 0;
                planar_plane_clouds_set_plane_window(pc, i, 1);
                const int rc1 = compute(&n1, &pst);
                if (rc1 == PLANAR_ECAPACITY && pst == 3) {
                    std::fprintf(stderr, "planar: plane %d of this frame alone has more than %d voxels: dropped (%s)\n", i, MP, planar_last_error());
                    continue;
                }
                if (!planar_adapter::ok(rc1, "ComputePlaneClouds (plane by plane)")) { total = 0; planePoints.clear(); planeCoefficients.clear(); break; }
                if (n1 == 1) { append(0, coef.data(), off.data(), pts.data()); total++; }
            }
            planar_plane_clouds_set_plane_window(pc, 0, -1);
            return PLANAR_OK;
        });
        if (!done) return 0;
        if (total >= 0) return total;
        for (int k = 0; k < n_out; k++) append(k, coef.data(), off.data(), pts.data());
        return n_out;
    }

private:
    cv::Mat depth_;
    float factor_ = 0, fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
    std::vector<int32_t> labels_;       // what planar_peac_segment delivered (plane_vertices_ / plane_filter are views of these)
    std::vector<double> planes_;
};

// ---- LineSegment (reference include/LSDextractor.h:344-352, src/LSDextractor.cpp:12-39).  Opt-in: define PLANAR_ADAPTERS_WITH_LINES
//      before including this header in a build that has opencv_contrib's line_descriptor and Eigen (the types of the signature). ------
#ifdef PLANAR_ADAPTERS_WITH_LINES
#include <opencv2/line_descriptor/descriptor.hpp>
#include <eigen3/Eigen/Core>
namespace Planar_SLAM {
class LineSegment {   // no data members: Frame calls this through an uninitialised pointer (include/Frame.h:123), which only works for a method that never touches `this`
public:
    // scale / numOctaves are accepted for signature compatibility; the reference passes 1.2f -> (int)1 and 1 (one octave, full resolution)
    void ExtractLineSegment(const cv::Mat& img, std::vector<cv::line_descriptor::KeyLine>& keylines, cv::Mat& ldesc,
                            std::vector<Eigen::Vector3d>& keylineFunctions, float scale = 1.2, int numOctaves = 1) {
        (void)scale; (void)numOctaves;
        static_assert(sizeof(cv::line_descriptor::KeyLine) == sizeof(planar_keyline), "cv::line_descriptor::KeyLine layout");
        static_assert(sizeof(Eigen::Vector3d) == 3 * sizeof(double), "Eigen::Vector3d layout");
        assert(img.type() == CV_8UC1);
        const int W = img.cols, H = img.rows;
        const int lsdNFeatures = 40;                                   // src/LSDextractor.cpp:18
        keylines.resize(lsdNFeatures);
        std::vector<unsigned char> desc((size_t)lsdNFeatures * 32);
        const size_t first = keylineFunctions.size();                  // the reference push_backs
        keylineFunctions.resize(first + lsdNFeatures);
        int32_t n = 0;
        if (!planar_adapter::on_lane(planar_adapter::LINES, "LineSegment", [&](planar_ctx*) {
                return planar_lsd_extract(planar_adapter::Runtime::get().lsd(W, H), img.data, 1, (int)img.step, (int64_t)img.step * H, lsdNFeatures,
                                          (planar_keyline*)keylines.data(), desc.data(), (double*)(keylineFunctions.data() + first), &n);
            })) n = 0;
        keylines.resize(n);
        keylineFunctions.resize(first + n);
        if (n) { ldesc = cv::Mat(n, 32, CV_8UC1); std::memcpy(ldesc.data, desc.data(), (size_t)n * 32); }   // BinaryDescriptor::compute leaves ldesc untouched when there are no lines
    }
};
}  // namespace Planar_SLAM
#endif

// ---- matchers and pose optimisers: definitions of the member functions the reference headers declare -----------------------------------
#ifdef PLANAR_ADAPTERS_WITH_TRACKING
namespace planar_adapter {

// a Frame as the guided matchers read it: every part, the pose from F.mTcw (where it is set), blocked = the feature holds an observed map point.
// (For a KeyFrame compose the parts yourself, with add_pose(pKF->GetPose()): ORBmatcher::Fuse below does.)
template <class FrameT> inline ViewGather frame_view(FrameT& F) {
    ViewGather g;
    g.add_keys(F.mvKeysUn, F.N).add_u_right(F.mvuRight).add_desc(F.mDescriptors).add_blocked_observed(F.mvpMapPoints).add_pose(F.mTcw);
    g.add_bounds(F).add_grid(F).add_intrinsics(F).add_stereo(F).add_scales(F.mvScaleFactors, false);
    return g;
}

}  // namespace planar_adapter

namespace Planar_SLAM {

// ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)  (src/ORBmatcher.cc:1396-1535)
inline int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono) {
    using namespace planar_adapter;
    const ViewGather cur = frame_view(CurrentFrame);
    const int NL = LastFrame.N;
    int32_t nl = NL;
    std::vector<uint8_t> usable(NL > 0 ? NL : 1, 0), observed(usable.size(), 0), mpd(usable.size() * 32, 0);
    std::vector<float> xw(usable.size() * 3, 0.f), ang(usable.size(), 0.f);
    std::vector<int32_t> oct(usable.size(), 0);
    float Tl[16];
    mat_to_array(LastFrame.mTcw, Tl);
    for (int i = 0; i < NL; i++) {
        MapPoint* pMP = LastFrame.mvpMapPoints[i];
        oct[i] = LastFrame.mvKeys[i].octave; ang[i] = LastFrame.mvKeysUn[i].angle;
        if (pMP && !LastFrame.mvbOutlier[i]) {
            usable[i] = 1;
            vec3_to_array(pMP->GetWorldPos(), &xw[3 * i]);
            copy_desc_rows(&mpd[(size_t)i * 32], pMP->GetDescriptor(), 1);
            observed[i] = pMP->Observations() > 0;
        }
    }
    planar_last_frame_view last;
    last.stride = (int32_t)usable.size(); last.n = &nl; last.Tcw = Tl; last.usable = usable.data(); last.xw = xw.data(); last.octave = oct.data(); last.angle = ang.data();
    last.mp_desc = mpd.data(); last.mp_observed = observed.data();
    std::vector<int32_t> match(cur.keys.size(), UNTOUCHED);
    int32_t nmatches = 0;
    if (!on_lane(TRACKING, "planar_search_by_projection_frame", [&](planar_ctx* ctx) {
            return planar_search_by_projection_frame(ctx, &cur.view, &last, th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0, match.data(), &nmatches);
        })) return 0;
    for (int i = 0; i < CurrentFrame.N; i++) {
        if (match[i] == UNTOUCHED) continue;
        CurrentFrame.mvpMapPoints[i] = match[i] >= 0 ? LastFrame.mvpMapPoints[match[i]] : static_cast<MapPoint*>(NULL);
    }
    return nmatches;
}

// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)  (src/ORBmatcher.cc:46-130)
inline int ORBmatcher::SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th) {
    using namespace planar_adapter;
    const ViewGather fr = frame_view(F);
    const size_t M = vpMapPoints.size();
    int32_t nm = (int32_t)M;
    std::vector<uint8_t> inview(M ? M : 1, 0), obs(inview.size(), 0), desc(inview.size() * 32, 0);
    std::vector<float> px(inview.size(), 0.f), py(inview.size(), 0.f), pxr(inview.size(), 0.f), vc(inview.size(), 0.f);
    std::vector<int32_t> lvl(inview.size(), 0);
    for (size_t j = 0; j < M; j++) {
        MapPoint* p = vpMapPoints[j];
        if (!p->mbTrackInView || p->isBad()) continue;
        inview[j] = 1; px[j] = p->mTrackProjX; py[j] = p->mTrackProjY; pxr[j] = p->mTrackProjXR; lvl[j] = p->mnTrackScaleLevel; vc[j] = p->mTrackViewCos;
        copy_desc_rows(&desc[j * 32], p->GetDescriptor(), 1);
        obs[j] = p->Observations() > 0;
    }
    planar_map_probes pr;
    pr.stride = (int32_t)inview.size(); pr.n = &nm; pr.in_view = inview.data(); pr.proj_x = px.data(); pr.proj_y = py.data(); pr.proj_xr = pxr.data(); pr.level = lvl.data();
    pr.view_cos = vc.data(); pr.desc = desc.data(); pr.observed = obs.data();
    std::vector<int32_t> match(fr.keys.size(), UNTOUCHED);
    int32_t nmatches = 0;
    if (!on_lane(TRACKING, "planar_search_by_projection_map", [&](planar_ctx* ctx) {
            return planar_search_by_projection_map(ctx, &fr.view, &pr, th, mfNNratio, match.data(), &nmatches);
        })) return 0;
    for (int i = 0; i < F.N; i++) if (match[i] >= 0) F.mvpMapPoints[i] = vpMapPoints[match[i]];
    return nmatches;
}

// ORBmatcher::MatchORBPoints(Frame&, const Frame&)  (src/ORBmatcher.cc:1332-1394)
inline int ORBmatcher::MatchORBPoints(Frame& CurrentFrame, const Frame& LastFrame) {
    using namespace planar_adapter;
    int32_t nc = CurrentFrame.N, nl = LastFrame.N;
    std::vector<uint8_t> cd((size_t)(nc > 0 ? nc : 1) * 32), ld((size_t)(nl > 0 ? nl : 1) * 32), has(nl > 0 ? nl : 1, 0), outl(has.size(), 0);
    copy_desc_rows(cd.data(), CurrentFrame.mDescriptors, nc);
    copy_desc_rows(ld.data(), LastFrame.mDescriptors, nl);
    for (int j = 0; j < nl; j++) {
        has[j] = LastFrame.mvpMapPoints[j] != NULL;
        outl[j] = (size_t)j < LastFrame.mvbOutlier.size() && LastFrame.mvbOutlier[j];
    }
    std::vector<int32_t> match(nc > 0 ? nc : 1, UNTOUCHED);
    int32_t npair = 0;
    if (!on_lane(TRACKING, "planar_match_orb_points", [&](planar_ctx* ctx) {
            return planar_match_orb_points(ctx, cd.data(), &nc, nc > 0 ? nc : 1, ld.data(), &nl, nl > 0 ? nl : 1, has.data(), outl.data(), 1, match.data(), &npair);
        })) return 0;
    for (int i = 0; i < nc; i++) if (match[i] >= 0) CurrentFrame.mvpMapPoints[i] = LastFrame.mvpMapPoints[match[i]];
    return npair;
}

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)  (src/ORBmatcher.cc:160-292).  A DBoW2::FeatureVector maps node id ->
// feature indices; every feature is in at most one node, so it is passed as one node id per feature.
inline int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches) {
    const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
    vpMapPointMatches = std::vector<MapPoint*>(F.N, static_cast<MapPoint*>(NULL));
    int32_t nk = (int32_t)vpMapPointsKF.size(), nf = F.N;
    if (nk == 0 || nf == 0) return 0;
    std::vector<int32_t> knode(nk, -1), fnode(nf, -1);
    for (const auto& kv : pKF->mFeatVec) for (unsigned int i : kv.second) if ((int)i < nk) knode[i] = (int32_t)kv.first;
    for (const auto& kv : F.mFeatVec) for (unsigned int i : kv.second) if ((int)i < nf) fnode[i] = (int32_t)kv.first;
    std::vector<uint8_t> kus(nk, 0), kd((size_t)nk * 32), fd((size_t)nf * 32);
    std::vector<float> kang(nk), fang(nf);
    for (int i = 0; i < nk; i++) { kus[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad(); kang[i] = pKF->mvKeysUn[i].angle; }
    for (int i = 0; i < nf; i++) fang[i] = F.mvKeys[i].angle;
    planar_adapter::copy_desc_rows(kd.data(), pKF->mDescriptors, nk);
    planar_adapter::copy_desc_rows(fd.data(), F.mDescriptors, nf);
    std::vector<int32_t> match(nf, -1);
    int32_t nmatches = 0;
    if (!planar_adapter::on_lane(planar_adapter::TRACKING, "planar_search_by_bow", [&](planar_ctx* ctx) {
            return planar_search_by_bow(ctx, 1, &nk, nk, knode.data(), kus.data(), kang.data(), kd.data(), &nf, nf, fnode.data(), fang.data(), fd.data(), mfNNratio,
                                        mbCheckOrientation ? 1 : 0, match.data(), &nmatches);
        })) return 0;
    for (int i = 0; i < nf; i++) if (match[i] >= 0) vpMapPointMatches[i] = vpMapPointsKF[match[i]];
    return nmatches;
}

// LSDmatcher::SearchByDescriptor(KeyFrame*, Frame&, vector<MapLine*>&)  (src/LSDmatcher.cpp:242-279)
inline int LSDmatcher::SearchByDescriptor(KeyFrame* pKF, Frame& currentF, std::vector<MapLine*>& vpMapLineMatches) {
    const std::vector<MapLine*> vpMapLinesKF = pKF->GetMapLineMatches();
    int32_t nk = pKF->mLineDescriptors.rows, nc = currentF.mLdesc.rows;
    vpMapLineMatches = std::vector<MapLine*>(currentF.NL, static_cast<MapLine*>(NULL));
    if (nk == 0 || nc == 0) return 0;
    std::vector<uint8_t> kd((size_t)nk * 32), cd((size_t)nc * 32), has(nk, 0);
    planar_adapter::copy_desc_rows(kd.data(), pKF->mLineDescriptors, nk);
    planar_adapter::copy_desc_rows(cd.data(), currentF.mLdesc, nc);
    for (int i = 0; i < nk; i++) has[i] = vpMapLinesKF[i] != NULL;
    std::vector<int32_t> match(nc, -1);
    int32_t nmatches = 0;
    if (!planar_adapter::on_lane(planar_adapter::TRACKING, "planar_lsd_search_by_descriptor", [&](planar_ctx* ctx) {
            return planar_lsd_search_by_descriptor(ctx, kd.data(), &nk, nk, cd.data(), &nc, nc, has.data(), 1, match.data(), &nmatches);
        })) return 0;
    for (int i = 0; i < nc && i < currentF.NL; i++) if (match[i] >= 0) vpMapLineMatches[i] = vpMapLinesKF[match[i]];
    return nmatches;
}

// LSDmatcher::SearchByProjection(Frame&, const vector<MapLine*>&, th)  (src/LSDmatcher.cpp:141-211)
inline int LSDmatcher::SearchByProjection(Frame& F, const std::vector<MapLine*>& vpMapLines, const float th) {
    int32_t nl = F.NL, nm = (int32_t)vpMapLines.size();
    if (nl == 0 || nm == 0) return 0;
    static_assert(sizeof(cv::line_descriptor::KeyLine) == sizeof(planar_keyline), "KeyLine layout");
    std::vector<uint8_t> ldesc((size_t)nl * 32), blocked(nl, 0), inview(nm, 0), obs(nm, 0), mdesc((size_t)nm * 32, 0);
    std::vector<float> proj((size_t)nm * 4, 0.f), vc(nm, 0.f);
    std::vector<int32_t> lvl(nm, 0);
    planar_adapter::copy_desc_rows(ldesc.data(), F.mLdesc, nl);
    for (int i = 0; i < nl; i++) blocked[i] = F.mvpMapLines[i] && F.mvpMapLines[i]->Observations() > 0;
    for (int j = 0; j < nm; j++) {
        MapLine* p = vpMapLines[j];
        if (!p || p->isBad() || !p->mbTrackInView) continue;
        inview[j] = 1; proj[4 * j] = p->mTrackProjX1; proj[4 * j + 1] = p->mTrackProjY1; proj[4 * j + 2] = p->mTrackProjX2; proj[4 * j + 3] = p->mTrackProjY2;
        lvl[j] = p->mnTrackScaleLevel; vc[j] = p->mTrackViewCos;
        planar_adapter::copy_desc_rows(&mdesc[(size_t)j * 32], p->GetDescriptor(), 1);
        obs[j] = p->Observations() > 0;
    }
    std::vector<int32_t> match(nl, planar_adapter::UNTOUCHED);
    int32_t nmatches = 0;
    if (!planar_adapter::on_lane(planar_adapter::TRACKING, "planar_lsd_search_by_projection", [&](planar_ctx* ctx) {
            return planar_lsd_search_by_projection(ctx, 1, &nl, nl, (const planar_keyline*)F.mvKeylinesUn.data(), ldesc.data(), blocked.data(), &nm, nm, inview.data(), proj.data(),
                                                   lvl.data(), vc.data(), mdesc.data(), obs.data(), F.mvScaleFactors.data(), (int)F.mvScaleFactors.size(), th, mfNNratio,
                                                   match.data(), &nmatches);
        })) return 0;
    for (int i = 0; i < nl; i++) if (match[i] >= 0) F.mvpMapLines[i] = vpMapLines[match[i]];
    return nmatches;
}

// ---- Fuse (LocalMapping::SearchInNeighbors).  Enabled with PLANAR_ADAPTERS_WITH_FUSE: the search needs the UNSCALED invariance distances of a map point / line
//      (MapPoint::PredictScale divides mfMaxDistance; GetMaxDistanceInvariance() returns 1.2f * it), which include/MapPoint.h / MapLine.h keep protected - add
//          void GetDistanceRange(float& mn, float& mx) { unique_lock<mutex> lock(mMutexPos); mn = mfMinDistance; mx = mfMaxDistance; }
//      to both classes.  The search half runs on the device; the map edits are the reference's own statements on its own objects.
#ifdef PLANAR_ADAPTERS_WITH_FUSE
// ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)  (src/ORBmatcher.cc:829-979)
inline int ORBmatcher::Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const float th) {
    const int M = (int)vpMapPoints.size(), N = pKF->N;
    if (M == 0) return 0;
    using namespace planar_adapter;
    // the key frame's side: every part of a Frame's view but `blocked`; KeyFrame keeps the bounds / grid constants per object and the pose behind GetPose()
    ViewGather kf;
    kf.add_keys(pKF->mvKeysUn, N).add_u_right(pKF->mvuRight).add_desc(pKF->mDescriptors).add_pose(pKF->GetPose());
    kf.add_bounds(*pKF).add_grid(*pKF).add_intrinsics(*pKF).add_stereo(*pKF).add_scales(pKF->mvScaleFactors, false);
    // the map points' side: not NULL, not bad, not in the key frame yet (:849-853)
    PointGather pts;
    pts.add_points(vpMapPoints, (size_t)M, [&](MapPoint* p) { return p->IsInKeyFrame(pKF); }).add_normals(vpMapPoints).add_desc(vpMapPoints).add_range(vpMapPoints);
    std::vector<int32_t> idx(M, -1);
    int32_t m = M, nFused = 0;
    if (!on_lane(TRACKING, "planar_fuse_search", [&](planar_ctx* ctx) {
            return planar_fuse_search(ctx, &kf.view, pKF->mvInvLevelSigma2.data(), pKF->mfLogScaleFactor, pKF->mnScaleLevels, &m, M, 0, pts.usable.data(), pts.xw.data(),
                                      pts.nrm.data(), pts.mn.data(), pts.mx.data(), pts.desc.data(), th, idx.data(), nullptr, &nFused);
        })) return 0;
    apply_fuse_edits(pKF, vpMapPoints, idx, [&](int i) { return pKF->GetMapPoint(i); }, [&](MapPoint* p, int i) { pKF->AddMapPoint(p, i); });
    return nFused;
}

// LSDmatcher::Fuse(KeyFrame*, const vector<MapLine*>&, th)  (src/LSDmatcher.cpp:884-1015)
inline int LSDmatcher::Fuse(KeyFrame* pKF, const std::vector<MapLine*>& vpMapLines, const float th) {
    const int M = (int)vpMapLines.size();
    int32_t nl = (int32_t)pKF->mvKeyLines.size();
    if (M == 0 || nl == 0) return 0;
    static_assert(sizeof(cv::line_descriptor::KeyLine) == sizeof(planar_keyline), "KeyLine layout");
    using namespace planar_adapter;
    std::vector<uint8_t> ldesc((size_t)nl * 32);
    copy_desc_rows(ldesc.data(), pKF->mLineDescriptors, nl);
    ViewGather kf;                                                                  // no key points: the pose, the bounds, the camera and the scale table
    kf.add_pose(pKF->GetPose()).add_bounds(*pKF).add_intrinsics(*pKF).add_stereo(*pKF).add_scales(pKF->mvScaleFactors, false);
    const int n_levels = (int)std::min<size_t>(pKF->mvScaleFactors.size(), PLANAR_MAX_LEVELS);
    std::vector<uint8_t> usable(M, 0), desc((size_t)M * 32, 0);
    std::vector<double> xw6((size_t)M * 6, 0.0), nrm((size_t)M * 3, 0.0);
    std::vector<float> mn(M, 0.f), mx(M, 0.f);
    for (int j = 0; j < M; j++) {
        MapLine* p = vpMapLines[j];
        if (!p || p->isBad()) continue;                                             // :906-907
        usable[j] = 1;
        const Vector6d P = p->GetWorldPos();
        const Eigen::Vector3d Pn = p->GetNormal();
        for (int k = 0; k < 6; k++) xw6[6 * j + k] = P(k);
        for (int k = 0; k < 3; k++) nrm[3 * j + k] = Pn(k);
        copy_desc_rows(&desc[(size_t)j * 32], p->GetDescriptor(), 1);
        p->GetDistanceRange(mn[j], mx[j]);
    }
    std::vector<int32_t> idx(M, -1);
    int32_t m = M, nFused = 0;
    if (!on_lane(TRACKING, "planar_lsd_fuse_search", [&](planar_ctx* ctx) {
            return planar_lsd_fuse_search(ctx, &kf.view, pKF->mfLogScaleFactor, n_levels, &nl, nl, (const planar_keyline*)pKF->mvKeyLines.data(), ldesc.data(), &m, M, 0, usable.data(),
                                          xw6.data(), nrm.data(), mn.data(), mx.data(), desc.data(), th, idx.data(), nullptr, &nFused);
        })) return 0;
    apply_fuse_edits(pKF, vpMapLines, idx, [&](int i) { return pKF->GetMapLine(i); }, [&](MapLine* p, int i) { pKF->AddMapLine(p, i); });
    return nFused;
}
#endif   // PLANAR_ADAPTERS_WITH_FUSE

// PlaneMatcher::SearchMapByCoefficients(Frame&, const vector<MapPlane*>&)  (src/PlaneMatcher.cpp:10-66)
inline int PlaneMatcher::SearchMapByCoefficients(Frame& pF, const std::vector<MapPlane*>& vpMapPlanes) {
    pF.mbNewPlane = false;
    int32_t np = pF.mnPlaneNum, nm = (int32_t)vpMapPlanes.size();
    if (np == 0) return 0;
    std::vector<float> coef((size_t)np * 4), T(16), mcoef((size_t)(nm ? nm : 1) * 4, 0.f);
    for (int i = 0; i < np; i++) for (int k = 0; k < 4; k++) coef[4 * i + k] = pF.mvPlaneCoefficients[i].template at<float>(k);
    planar_adapter::mat_to_array(pF.mTcw, T.data());
    std::vector<uint8_t> valid(nm ? nm : 1, 0);
    std::vector<int32_t> npts(nm ? nm : 1, 0);
    int maxp = 1;
    for (int j = 0; j < nm; j++) if (!vpMapPlanes[j]->isBad() && vpMapPlanes[j]->mvPlanePoints) maxp = std::max(maxp, (int)vpMapPlanes[j]->mvPlanePoints->points.size());
    std::vector<float> pts((size_t)(nm ? nm : 1) * maxp * 3, 0.f);
    for (int j = 0; j < nm; j++) {
        MapPlane* p = vpMapPlanes[j];
        if (p->isBad()) continue;
        valid[j] = 1;
        cv::Mat c = p->GetWorldPos();
        for (int k = 0; k < 4; k++) mcoef[4 * j + k] = c.at<float>(k);
        if (p->mvPlanePoints) {
            npts[j] = (int32_t)p->mvPlanePoints->points.size();
            for (int k = 0; k < npts[j]; k++) { const auto& q = p->mvPlanePoints->points[k]; float* o = &pts[((size_t)j * maxp + k) * 3]; o[0] = q.x; o[1] = q.y; o[2] = q.z; }
        }
    }
    const float th[4] = {dTh, aTh, verTh, parTh};
    std::vector<int32_t> a(np, -1), v(np, -1), par(np, -1);
    int32_t nmatches = 0;
    if (!planar_adapter::on_lane(planar_adapter::TRACKING, "planar_plane_search_by_coefficients", [&](planar_ctx* ctx) {
            return planar_plane_search_by_coefficients(ctx, 1, &np, np, coef.data(), T.data(), 0, &nm, nm ? nm : 1, valid.data(), mcoef.data(), npts.data(), maxp, pts.data(), th,
                                                       a.data(), v.data(), par.data(), &nmatches);
        })) return 0;
    for (int i = 0; i < np; i++) {
        if (a[i] >= 0) pF.mvpMapPlanes[i] = vpMapPlanes[a[i]];
        if (v[i] >= 0) pF.mvpVerticalPlanes[i] = vpMapPlanes[v[i]];
        if (par[i] >= 0) pF.mvpParallelPlanes[i] = vpMapPlanes[par[i]];
    }
    return nmatches;
}

// Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:550-1275) / TranslationOptimization(Frame*) (:2995-3738).  cfg = the six Plane.* values
// Config::Get<double> returns (Plane.AngleInfo, DistanceInfo, ParallelInfo, VerticalInfo, Chi, VPChi).
namespace planar_detail {
template <class FrameT> inline int pose_opt(FrameT* pFrame, int mode) {
    const int N = pFrame->N, NL = pFrame->NL, M = pFrame->mnPlaneNum;
    const int MP = N > 0 ? N : 1, ML = NL > 0 ? NL : 1, MM = M > 0 ? M : 1;
    int32_t n_points = N, n_lines = NL, n_planes = M, n_inliers = 0;
    std::vector<uint8_t> pt_valid(MP, 0), ln_valid(ML, 0), pl_valid((size_t)MM * 3, 0), pt_out(MP, 0), ln_out(ML, 0), pl_out((size_t)MM * 3, 0);
    std::vector<float> pt_xw((size_t)MP * 3, 0.f), pt_obs((size_t)MP * 3, 0.f), pt_is2(MP, 1.f), pl_meas((size_t)MM * 4, 0.f), pl_world((size_t)MM * 12, 0.f), Tin(16), Tout(16);
    std::vector<double> ln_obs((size_t)ML * 3, 0.0), ln_xw((size_t)ML * 6, 0.0);
    for (int i = 0; i < N; i++) {
        const cv::KeyPoint& kp = pFrame->mvKeysUn[i];
        pt_obs[3 * i] = kp.pt.x; pt_obs[3 * i + 1] = kp.pt.y; pt_obs[3 * i + 2] = pFrame->mvuRight[i];
        pt_is2[i] = pFrame->mvInvLevelSigma2[kp.octave];
        if (MapPoint* p = pFrame->mvpMapPoints[i]) { pt_valid[i] = 1; planar_adapter::vec3_to_array(p->GetWorldPos(), &pt_xw[3 * i]); }
    }
    for (int i = 0; i < NL; i++) {
        for (int k = 0; k < 3; k++) ln_obs[3 * i + k] = pFrame->mvKeyLineFunctions[i][k];
        if (MapLine* p = pFrame->mvpMapLines[i]) { ln_valid[i] = 1; for (int k = 0; k < 6; k++) ln_xw[6 * i + k] = p->mWorldPos[k]; }
    }
    for (int i = 0; i < M; i++) {
        for (int k = 0; k < 4; k++) pl_meas[4 * i + k] = pFrame->mvPlaneCoefficients[i].template at<float>(k);
        MapPlane* three[3] = {pFrame->mvpMapPlanes[i], pFrame->mvpParallelPlanes[i], pFrame->mvpVerticalPlanes[i]};
        for (int j = 0; j < 3; j++) if (three[j]) { pl_valid[3 * i + j] = 1; cv::Mat c = three[j]->GetWorldPos(); for (int k = 0; k < 4; k++) pl_world[(3 * i + j) * 4 + k] = c.at<float>(k); }
    }
    planar_adapter::mat_to_array(pFrame->mTcw, Tin.data());
    planar_pose_batch pb;
    std::memset(&pb, 0, sizeof(pb));
    pb.B = 1; pb.max_points = MP; pb.max_lines = ML; pb.max_planes = MM;
    pb.n_points = &n_points; pb.n_lines = &n_lines; pb.n_planes = &n_planes; pb.pt_valid = pt_valid.data(); pb.pt_xw = pt_xw.data(); pb.pt_obs = pt_obs.data();
    pb.pt_inv_sigma2 = pt_is2.data(); pb.ln_valid = ln_valid.data(); pb.ln_obs = ln_obs.data(); pb.ln_xw = ln_xw.data(); pb.pl_meas = pl_meas.data(); pb.pl_valid = pl_valid.data();
    pb.pl_world = pl_world.data(); pb.Tcw_in = Tin.data(); pb.Tcw_out = Tout.data(); pb.pt_outlier = pt_out.data(); pb.ln_outlier = ln_out.data(); pb.pl_outlier = pl_out.data();
    pb.n_inliers = &n_inliers; pb.lm_iters = nullptr;
    const planar_pose_params prm = planar_adapter::plane_pose_params<Config>(pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy, pFrame->mbf);
    if (!planar_adapter::on_lane(planar_adapter::TRACKING, "planar_pose_opt", [&](planar_ctx* ctx) { return planar_pose_opt(ctx, &pb, &prm, mode, 4, 10); })) return 0;
    // the reference writes the flags of the correspondences it used and the pose through Frame::SetPose
    for (int i = 0; i < N; i++) if (pt_valid[i]) pFrame->mvbOutlier[i] = pt_out[i] != 0;
    for (int i = 0; i < NL; i++) if (ln_valid[i]) pFrame->mvbLineOutlier[i] = ln_out[i] != 0;
    for (int i = 0; i < M; i++) {
        if (pl_valid[3 * i]) pFrame->mvbPlaneOutlier[i] = pl_out[3 * i] != 0;
        if (mode == PLANAR_POSE_FULL) {
            if (pl_valid[3 * i + 1]) pFrame->mvbParPlaneOutlier[i] = pl_out[3 * i + 1] != 0;
            if (pl_valid[3 * i + 2]) pFrame->mvbVerPlaneOutlier[i] = pl_out[3 * i + 2] != 0;
        }
    }
    pFrame->SetPose(planar_adapter::array_to_mat(Tout.data()));
    return n_inliers;
}
}  // namespace planar_detail
inline int Optimizer::PoseOptimization(Frame* pFrame) { return planar_detail::pose_opt(pFrame, PLANAR_POSE_FULL); }
inline int Optimizer::TranslationOptimization(Frame* pFrame) { return planar_detail::pose_opt(pFrame, PLANAR_POSE_TRANSLATION); }

}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_TRACKING

// ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:309-540), everything up to "Triangulation is succesfull".  Enabled with PLANAR_ADAPTERS_WITH_NEW_POINTS.
//      Takes the current key frame and its neighbours (GetBestCovisibilityKeyFrames' order; pass fewer to mirror the CheckNewKeyFrames() return), packs them, calls
//      planar_create_new_map_points and returns the candidates in the reference's creation order.  The caller keeps the reference's own statements for each of them:
//          MapPoint* pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpMap); pMP->AddObservation(mpCurrentKeyFrame, idx1); pMP->AddObservation(vpNeighKFs[neighbour], idx2);
//          mpCurrentKeyFrame->AddMapPoint(pMP, idx1); vpNeighKFs[neighbour]->AddMapPoint(pMP, idx2); ComputeDistinctiveDescriptors(); UpdateNormalAndDepth(); ...
//      A failing call degrades to "no new points".  KeyFrameT is Planar_SLAM::KeyFrame (a template only so that a test can pass a stand-in): N, mvKeysUn, mvKeys,
//      mvuRight, mvDepth, mDescriptors, mFeatVec, GetMapPoint, GetPose, GetPoseInverse, mb, mbf, fx fy cx cy invfx invfy, mfScaleFactor, mvScaleFactors, mvLevelSigma2 are read.
#ifdef PLANAR_ADAPTERS_WITH_NEW_POINTS
namespace planar_adapter {

struct NewPointCandidate {
    int neighbour;        // index into vpNeighKFs
    int idx1, idx2;       // feature of the current key frame, feature of the neighbour
    float x3D[3];         // the position handed to MapPoint's constructor
};

namespace detail {
// the arrays of `count` key frames behind one planar_tri_keyframes
struct TriPack {
    int32_t stride;
    std::vector<int32_t> n, node;
    std::vector<planar_keypoint> keys_un, keys;
    std::vector<float> u_right, depth, cos_stereo, Tcw, Twc, mb, mbf;
    std::vector<uint8_t> desc, occupied;
    TriPack(size_t count, int32_t s) : stride(s), n(count, 0), node(count * s, -1), keys_un(count * s), keys(count * s), u_right(count * s, -1.f), depth(count * s, -1.f),
                                       cos_stereo(count * s, 0.f), Tcw(count * 16, 0.f), Twc(count * 16, 0.f), mb(count, 0.f), mbf(count, 0.f), desc(count * s * 32, 0),
                                       occupied(count * s, 0) {}
    template <class KeyFrameT> void put(size_t e, KeyFrameT* kf) {
        const size_t o = e * stride;
        const int N = kf->N;
        n[e] = N; mb[e] = kf->mb; mbf[e] = kf->mbf;
        copy_keypoints(&keys_un[o], kf->mvKeysUn.data(), N > 0 ? N : 0);
        copy_keypoints(&keys[o], kf->mvKeys.data(), N > 0 ? N : 0);
        copy_desc_rows(&desc[o * 32], kf->mDescriptors, N);
        for (int i = 0; i < N; i++) {
            u_right[o + i] = kf->mvuRight[i];
            depth[o + i] = kf->mvDepth[i];
            // src/LocalMapping.cc:411, :413 in the host's float libm: the value decides a branch, so it is not left to the device
            cos_stereo[o + i] = std::cos(2 * std::atan2(kf->mb / 2, kf->mvDepth[i]));
            occupied[o + i] = kf->GetMapPoint(i) != NULL;
        }
        for (const auto& kv : kf->mFeatVec) for (unsigned int i : kv.second) if ((int)i < N) node[o + i] = (int32_t)kv.first;
        mat_to_array(kf->GetPose(), &Tcw[e * 16]);
        mat_to_array(kf->GetPoseInverse(), &Twc[e * 16]);
    }
    planar_tri_keyframes view() const {
        planar_tri_keyframes v;
        v.count = (int32_t)n.size(); v.stride = stride; v.n = n.data(); v.keys_un = keys_un.data(); v.u_right = u_right.data(); v.desc = desc.data(); v.node = node.data();
        v.occupied = occupied.data(); v.Tcw = Tcw.data(); v.keys = keys.data(); v.depth = depth.data(); v.cos_stereo = cos_stereo.data(); v.Twc = Twc.data();
        v.mb = mb.data(); v.mbf = mbf.data();
        return v;
    }
};
}  // namespace detail

template <class KeyFrameT>
inline std::vector<NewPointCandidate> CreateNewMapPoints(KeyFrameT* pKF, const std::vector<KeyFrameT*>& vpNeighKFs) {
    std::vector<NewPointCandidate> out;
    const int K = (int)vpNeighKFs.size();
    if (!pKF || pKF->N <= 0 || K == 0) return out;
    if (K > PLANAR_TRI_MAX_NEIGHBOURS) { std::fprintf(stderr, "planar (CreateNewMapPoints): more than %d neighbours - degraded to \"nothing found\"\n", PLANAR_TRI_MAX_NEIGHBOURS); return out; }
    int32_t stride = pKF->N;
    for (KeyFrameT* kf : vpNeighKFs) if (kf->N > stride) stride = kf->N;
    const planar_tri_camera cam = tri_camera(pKF);
    detail::TriPack cur(1, stride), nb((size_t)K, stride);
    cur.put(0, pKF);
    for (int k = 0; k < K; k++) nb.put((size_t)k, vpNeighKFs[k]);
    const planar_tri_keyframes vc = cur.view(), vn = nb.view();
    std::vector<int32_t> kk(stride, -1), i1(stride, -1), i2(stride, -1);
    std::vector<float> x((size_t)stride * 3, 0.f);
    int32_t n_neigh = K, n_new = 0;
    if (!on_lane(TRACKING, "planar_create_new_map_points", [&](planar_ctx* ctx) {
            return planar_create_new_map_points(ctx, &cam, &vc, &vn, &n_neigh, K, &n_new, kk.data(), i1.data(), i2.data(), x.data());
        })) return out;
    out.resize(n_new);
    for (int j = 0; j < n_new; j++) { out[j].neighbour = kk[j]; out[j].idx1 = i1[j]; out[j].idx2 = i2[j]; for (int c = 0; c < 3; c++) out[j].x3D[c] = x[3 * j + c]; }
    return out;
}

}  // namespace planar_adapter
#endif   // PLANAR_ADAPTERS_WITH_NEW_POINTS

// ---- LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:800-1037), everything up to "new MapLine", and LSDmatcher::SearchForTriangulation
//      (src/LSDmatcher.cpp:334-367).  Enabled with PLANAR_ADAPTERS_WITH_NEW_LINES.  CreateNewMapLines takes the current key frame and its neighbours
//      (GetBestCovisibilityKeyFrames' order; pass fewer to mirror the CheckNewKeyFrames() return), packs them, calls planar_create_new_map_lines and returns the
//      candidates in the reference's creation order.  The caller keeps the reference's own statements for each of them:
//          MapLine* pML = new MapLine(line3D, mpCurrentKeyFrame, mpMap); pML->AddObservation(mpCurrentKeyFrame, idx1); pML->AddObservation(vpNeighKFs[neighbour], idx2);
//          mpCurrentKeyFrame->AddMapLine(pML, idx1); vpNeighKFs[neighbour]->AddMapLine(pML, idx2); ComputeDistinctiveDescriptors(); UpdateAverageDir(); ...
//      A failing call, more than PLANAR_TRI_MAX_NEIGHBOURS neighbours or a key frame with more than PLANAR_MAX_KEYFRAME_LINES lines degrades to "no new lines".
//      KeyFrameT is Planar_SLAM::KeyFrame (a template only so that a test can pass a stand-in): mvKeyLines, mLineDescriptors, mvDepthLine, mvLines3D, GetMapLine,
//      GetPose, GetPoseInverse, mb, fx fy cx cy invfx invfy, mfScaleFactor, mvScaleFactors, mvLevelSigma2 are read.  Kept as the reference has them: bStereo2 reads the
//      current key frame's mvDepthLine at the neighbour's index, two lines may take one idx2, F12 is not computed (its result is unused by the line path).
//      With PLANAR_ADAPTERS_LSDMATCHER_TRIANGULATION as well (after the reference's LSDmatcher.h) LSDmatcher::SearchForTriangulation itself is defined here.
#ifdef PLANAR_ADAPTERS_WITH_NEW_LINES
#include <opencv2/line_descriptor/descriptor.hpp>
namespace planar_adapter {

struct NewLineCandidate {
    int neighbour;        // index into vpNeighKFs
    int idx1, idx2;       // line of the current key frame, line of the neighbour
    double line3D[6];     // the Vector6d handed to MapLine's constructor: floats widened to double
};

namespace detail {
// the arrays of `count` key frames behind one planar_tri_line_keyframes
struct TriLinePack {
    int32_t stride;
    std::vector<int32_t> n;
    std::vector<planar_keyline> keylines;
    std::vector<uint8_t> ldesc_store, occupied;
    std::vector<float> depth_line, Tcw, Twc, mb;
    std::vector<double> lines3d;
    uint8_t* ldesc;       // 16-byte aligned inside ldesc_store
    TriLinePack(size_t count, int32_t s) : stride(s), n(count, 0), keylines(count * s), ldesc_store(count * s * 32 + 16, 0), occupied(count * s, 0), depth_line(count * s, -1.f),
                                           Tcw(count * 16, 0.f), Twc(count * 16, 0.f), mb(count, 0.f), lines3d(count * s * 6, 0.0) {
        std::memset(keylines.data(), 0, keylines.size() * sizeof(planar_keyline));
        ldesc = ldesc_store.data() + ((16 - ((uintptr_t)ldesc_store.data() & 15)) & 15);
    }
    // what the two searches read (n, ldesc, occupied)
    template <class KeyFrameT> void put_search(size_t e, KeyFrameT* kf) {
        static_assert(sizeof(cv::line_descriptor::KeyLine) == sizeof(planar_keyline), "KeyLine layout");
        const size_t o = e * stride;
        const int N = kf->mLineDescriptors.rows;
        n[e] = N;
        copy_desc_rows(ldesc + o * 32, kf->mLineDescriptors, N);
        for (int i = 0; i < N; i++) occupied[o + i] = kf->GetMapLine(i) != NULL;
    }
    template <class KeyFrameT> void put(size_t e, KeyFrameT* kf) {
        put_search(e, kf);
        const size_t o = e * stride;
        int N = n[e];
        // the reference keeps mvKeyLines, mvDepthLine and mvLines3D as long as mLineDescriptors has rows; a shorter one leaves its lines without depth (-1, zeros)
        if ((size_t)N > kf->mvKeyLines.size()) N = (int)kf->mvKeyLines.size();
        if ((size_t)N > kf->mvDepthLine.size()) N = (int)kf->mvDepthLine.size();
        if ((size_t)N > kf->mvLines3D.size()) N = (int)kf->mvLines3D.size();
        mb[e] = kf->mb;
        for (int i = 0; i < N; i++) {
            std::memcpy(&keylines[o + i], &kf->mvKeyLines[i], sizeof(planar_keyline));
            depth_line[o + i] = kf->mvDepthLine[i];
            for (int c = 0; c < 6; c++) lines3d[(o + i) * 6 + c] = kf->mvLines3D[i](c);
        }
        mat_to_array(kf->GetPose(), &Tcw[e * 16]);
        mat_to_array(kf->GetPoseInverse(), &Twc[e * 16]);
    }
    planar_tri_line_keyframes view(bool search) const {
        planar_tri_line_keyframes v;
        std::memset(&v, 0, sizeof(v));
        v.count = (int32_t)n.size(); v.stride = stride; v.n = n.data(); v.ldesc = ldesc; v.occupied = occupied.data();
        if (!search) { v.keylines = keylines.data(); v.depth_line = depth_line.data(); v.lines3d = lines3d.data(); v.Tcw = Tcw.data(); v.Twc = Twc.data(); v.mb = mb.data(); }
        return v;
    }
};
}  // namespace detail

template <class KeyFrameT>
inline std::vector<NewLineCandidate> CreateNewMapLines(KeyFrameT* pKF, const std::vector<KeyFrameT*>& vpNeighKFs) {
    std::vector<NewLineCandidate> out;
    const int K = (int)vpNeighKFs.size();
    if (!pKF || pKF->mLineDescriptors.rows <= 0 || K == 0) return out;
    if (K > PLANAR_TRI_MAX_NEIGHBOURS) { std::fprintf(stderr, "planar (CreateNewMapLines): more than %d neighbours - degraded to \"nothing found\"\n", PLANAR_TRI_MAX_NEIGHBOURS); return out; }
    int32_t stride = pKF->mLineDescriptors.rows;
    for (KeyFrameT* kf : vpNeighKFs) if (kf->mLineDescriptors.rows > stride) stride = kf->mLineDescriptors.rows;
    if (stride > PLANAR_MAX_KEYFRAME_LINES) { std::fprintf(stderr, "planar (CreateNewMapLines): more than %d lines in a key frame - degraded to \"nothing found\"\n", PLANAR_MAX_KEYFRAME_LINES); return out; }
    const planar_tri_camera cam = tri_camera(pKF);
    detail::TriLinePack cur(1, stride), nb((size_t)K, stride);
    cur.put(0, pKF);
    for (int k = 0; k < K; k++) nb.put((size_t)k, vpNeighKFs[k]);
    const planar_tri_line_keyframes vc = cur.view(false), vn = nb.view(false);
    std::vector<int32_t> kk(stride, -1), i1(stride, -1), i2(stride, -1);
    std::vector<double> x((size_t)stride * 6, 0.0);
    int32_t n_neigh = K, n_new = 0;
    if (!on_lane(TRACKING, "planar_create_new_map_lines", [&](planar_ctx* ctx) {
            return planar_create_new_map_lines(ctx, &cam, &vc, &vn, &n_neigh, K, &n_new, kk.data(), i1.data(), i2.data(), x.data());
        })) return out;
    out.resize(n_new);
    for (int j = 0; j < n_new; j++) { out[j].neighbour = kk[j]; out[j].idx1 = i1[j]; out[j].idx2 = i2[j]; for (int c = 0; c < 6; c++) out[j].line3D[c] = x[6 * j + c]; }
    return out;
}

// LSDmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs): the pairs in ascending qdx, the count returned.  A failing call gives no pairs.
template <class KeyFrameT>
inline int SearchLinesForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs) {
    vMatchedPairs.clear();
    const int32_t n1 = pKF1->mLineDescriptors.rows, n2 = pKF2->mLineDescriptors.rows;
    const int32_t stride = n1 > n2 ? n1 : n2;
    if (n1 <= 0 || n2 < 2) return 0;   // the reference would index lmatches[i][1]
    if (stride > PLANAR_MAX_KEYFRAME_LINES) { std::fprintf(stderr, "planar (SearchForTriangulation): more than %d lines in a key frame - degraded to \"nothing found\"\n", PLANAR_MAX_KEYFRAME_LINES); return 0; }
    detail::TriLinePack a(1, stride), b(1, stride);
    a.put_search(0, pKF1);
    b.put_search(0, pKF2);
    const planar_tri_line_keyframes va = a.view(true), vb = b.view(true);
    std::vector<int32_t> match(stride, -1);
    int32_t nmatches = 0;
    if (!on_lane(TRACKING, "planar_lsd_search_for_triangulation", [&](planar_ctx* ctx) {
            return planar_lsd_search_for_triangulation(ctx, &va, &vb, match.data(), &nmatches, NULL, NULL);
        })) return 0;
    for (int q = 0; q < n1; q++) if (match[q] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)q, (size_t)match[q]));
    return nmatches;
}

}  // namespace planar_adapter
#ifdef PLANAR_ADAPTERS_LSDMATCHER_TRIANGULATION
namespace Planar_SLAM {
inline int LSDmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs) {
    return planar_adapter::SearchLinesForTriangulation(pKF1, pKF2, vMatchedPairs);
}
}  // namespace Planar_SLAM
#endif
#endif   // PLANAR_ADAPTERS_WITH_NEW_LINES

// ---- KeyFrameDatabase (include/KeyFrameDatabase.h:42-70, src/KeyFrameDatabase.cc): add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates with
//      the reference's signatures.  Enabled with PLANAR_ADAPTERS_WITH_KFDB, after the reference's KeyFrame.h, Frame.h and ORBVocabulary.h.  The class keeps a HOST
//      mirror (no device resource): one slot per key frame ever added, with a copy of its mBowVec, whether it is in the inverted file, the order of its add() and the
//      two score members (mRelocScore / mLoopScore live HERE and start at 0: the reference never initialises them).  A query packs the mirror, asks every present
//      key frame for GetBestCovisibilityKeyFrames(10), calls planar_kfdb_detect (the host flavour) and maps the slots back to pointers.  Of a key frame
//      mBowVec (begin / end, ->first, ->second), GetBestCovisibilityKeyFrames and, of the query, mBowVec and GetConnectedKeyFrames are read; the members
//      mnRelocQuery / mnRelocWords / mnLoopQuery / mnLoopWords of the key frames are NOT written (nothing else in the reference reads them).  A failing call, more
//      than PLANAR_KFDB_MAX_KEYFRAMES slots or a BowVector of more than PLANAR_KFDB_MAX_WORDS words gives an empty vector.  add() of a key frame that is already in
//      the database (the reference would list it twice) is ignored.
#ifdef PLANAR_ADAPTERS_WITH_KFDB
#include <list>
#include <set>
namespace planar_adapter {

template <class KeyFrameT, class FrameT, class VocabularyT>
class KeyFrameDatabaseT {
public:
    explicit KeyFrameDatabaseT(const VocabularyT&) {}    // the vocabulary is not read: the score is L1Scoring's, ORBvoc.txt's configuration
    void add(KeyFrameT* pKF) {
        std::lock_guard<std::mutex> g(mMutex);
        auto it = slot_of_.find(pKF);
        if (it == slot_of_.end()) { it = slot_of_.insert(std::make_pair(pKF, (int)slots_.size())).first; slots_.push_back(Slot()); slots_.back().kf = pKF; }
        Slot& s = slots_[it->second];
        if (s.present) return;
        s.words.clear(); s.values.clear();
        for (auto vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; ++vit) { s.words.push_back((int32_t)vit->first); s.values.push_back((double)vit->second); }
        s.present = 1; s.add_seq = next_seq_++;
    }
    void erase(KeyFrameT* pKF) {
        std::lock_guard<std::mutex> g(mMutex);
        auto it = slot_of_.find(pKF);
        if (it != slot_of_.end()) slots_[it->second].present = 0;
    }
    void clear() {
        std::lock_guard<std::mutex> g(mMutex);
        slots_.clear(); slot_of_.clear(); next_seq_ = 0;
    }
    std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) {
        std::set<KeyFrameT*> connected = pKF->GetConnectedKeyFrames();
        return detect(1, pKF->mBowVec, &connected, minScore);
    }
    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) { return detect(0, F->mBowVec, (const std::set<KeyFrameT*>*)NULL, 0.f); }

protected:
    struct Slot {
        KeyFrameT* kf = NULL;
        uint8_t present = 0;
        int32_t add_seq = 0;
        std::vector<int32_t> words;
        std::vector<double> values;
        float score[2] = {0.f, 0.f};     // mRelocScore, mLoopScore
    };
    template <class BowT>
    std::vector<KeyFrameT*> detect(int mode, const BowT& bow, const std::set<KeyFrameT*>* connected, float minScore) {
        std::vector<KeyFrameT*> out;
        std::lock_guard<std::mutex> g(mMutex);
        const size_t n = slots_.size();
        if (n == 0) return out;
        std::vector<int32_t> qw;
        std::vector<double> qv;
        for (auto vit = bow.begin(), vend = bow.end(); vit != vend; ++vit) { qw.push_back((int32_t)vit->first); qv.push_back((double)vit->second); }
        size_t W = 1;
        for (const Slot& s : slots_) if (s.present && s.words.size() > W) W = s.words.size();
        if (n > PLANAR_KFDB_MAX_KEYFRAMES || W > PLANAR_KFDB_MAX_WORDS || qw.size() > PLANAR_KFDB_MAX_WORDS) {
            std::fprintf(stderr, "planar (KeyFrameDatabase): more than %d key frames or %d words - degraded to \"nothing found\"\n", PLANAR_KFDB_MAX_KEYFRAMES, PLANAR_KFDB_MAX_WORDS);
            return out;
        }
        const size_t QW = qw.size() ? qw.size() : 1;
        qw.resize(QW, 0); qv.resize(QW, 0.0);
        std::vector<uint8_t> present(n), excluded(n, 0);
        std::vector<int32_t> add_seq(n), bow_n(n, 0), bow_word(n * W, 0), covis(n * 10, -1), common(n, 0), cand(n, -1);
        std::vector<double> bow_value(n * W, 0.0);
        std::vector<float> score(n);
        for (size_t j = 0; j < n; j++) {
            const Slot& s = slots_[j];
            present[j] = s.present; add_seq[j] = s.add_seq; score[j] = s.score[mode];
            if (!s.present) continue;
            bow_n[j] = (int32_t)s.words.size();
            std::copy(s.words.begin(), s.words.end(), bow_word.begin() + j * W);
            std::copy(s.values.begin(), s.values.end(), bow_value.begin() + j * W);
            const std::vector<KeyFrameT*> neigh = s.kf->GetBestCovisibilityKeyFrames(10);
            for (size_t t = 0; t < neigh.size() && t < 10; t++) { const auto it = slot_of_.find(neigh[t]); if (it != slot_of_.end()) covis[j * 10 + t] = it->second; }
            if (connected && connected->count(s.kf)) excluded[j] = 1;
        }
        planar_kf_database db;
        db.kf_stride = (int32_t)n; db.word_stride = (int32_t)W;
        const int32_t n_kf = (int32_t)n, q_db = 0, q_n = (int32_t)bow.size();
        db.n_kf = &n_kf; db.present = present.data(); db.add_seq = add_seq.data(); db.bow_n = bow_n.data(); db.bow_word = bow_word.data(); db.bow_value = bow_value.data();
        db.covis = covis.data();
        int32_t n_cand = 0, n_scored = 0;
        if (!on_lane(TRACKING, "planar_kfdb_detect", [&](planar_ctx* ctx) {
                return planar_kfdb_detect(ctx, mode, &db, 1, &q_db, &q_n, qw.data(), qv.data(), (int)QW, mode ? excluded.data() : NULL, mode ? &minScore : NULL, score.data(),
                                          common.data(), &n_cand, cand.data(), &n_scored);
            })) return out;
        for (size_t j = 0; j < n; j++) slots_[j].score[mode] = score[j];
        out.reserve(n_cand);
        for (int i = 0; i < n_cand; i++) out.push_back(slots_[cand[i]].kf);
        return out;
    }
    std::vector<Slot> slots_;
    std::map<KeyFrameT*, int> slot_of_;
    int32_t next_seq_ = 0;
    std::mutex mMutex;
};

}  // namespace planar_adapter
namespace Planar_SLAM {
typedef planar_adapter::KeyFrameDatabaseT<KeyFrame, Frame, ORBVocabulary> KeyFrameDatabase;
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_KFDB

// ---- Tracking::UpdateLocalMap (src/Tracking.cc:2394-2552).  Enabled with PLANAR_ADAPTERS_WITH_LOCAL_MAP, after the reference's Tracking.h, Map.h, KeyFrame.h,
//      MapPoint.h and MapLine.h; leave that body of src/Tracking.cc (with UpdateLocalKeyFrames / UpdateLocalPoints / UpdateLocalLines, which it alone calls) out.
//      This form RE-PACKS THE MAP ON EVERY CALL: mpMap->GetAllKeyFrames() / GetAllMapPoints() / GetAllMapLines() name the objects (ids are positions in those
//      vectors; an object they do not hold but a key frame, an observation or the frame refers to - a bad parent, for one - is appended behind them), kf_rank is
//      std::less<KeyFrame*> over the pointers, children come in the std::set's own order, covis from GetBestCovisibilityKeyFrames(10), observations from
//      GetObservations().  It is the correctness path; the throughput path is planar_update_local_map_dev on a resident map.  The gathered rows
//      (positions, normals, descriptors) are not needed here and are passed as zeros.  The call runs with B = 1 on the tracking lane; a failing call, or a map of
//      more than PLANAR_LOCALMAP_MAX_KEYFRAMES key frames, changes nothing and reports on stderr.  As in the reference, the frame's bad map points become NULL
//      (:2470); its bad map lines are left to SearchLocalLines.
#ifdef PLANAR_ADAPTERS_WITH_LOCAL_MAP
#include <set>
namespace Planar_SLAM {
inline void Tracking::UpdateLocalMap() {
    mpMap->SetReferenceMapPoints(mvpLocalMapPoints);      // This is for visualization (:2396-2397)
    mpMap->SetReferenceMapLines(mvpLocalMapLines);
    std::vector<KeyFrame*> K = mpMap->GetAllKeyFrames();
    std::vector<MapPoint*> P = mpMap->GetAllMapPoints();
    std::vector<MapLine*> ML = mpMap->GetAllMapLines();
    std::map<KeyFrame*, int32_t> kf_id;
    std::map<MapPoint*, int32_t> pt_id;
    std::map<MapLine*, int32_t> ml_id;
    for (size_t i = 0; i < K.size(); i++) kf_id[K[i]] = (int32_t)i;
    for (size_t i = 0; i < P.size(); i++) pt_id[P[i]] = (int32_t)i;
    for (size_t i = 0; i < ML.size(); i++) ml_id[ML[i]] = (int32_t)i;
    auto kf_of = [&](KeyFrame* p) -> int32_t {
        if (!p) return -1;
        auto it = kf_id.find(p);
        if (it != kf_id.end()) return it->second;
        K.push_back(p);
        return kf_id[p] = (int32_t)K.size() - 1;
    };
    auto pt_of = [&](MapPoint* p) -> int32_t {
        if (!p) return -1;
        auto it = pt_id.find(p);
        if (it != pt_id.end()) return it->second;
        P.push_back(p);
        return pt_id[p] = (int32_t)P.size() - 1;
    };
    auto ml_of = [&](MapLine* p) -> int32_t {
        if (!p) return -1;
        auto it = ml_id.find(p);
        if (it != ml_id.end()) return it->second;
        ML.push_back(p);
        return ml_id[p] = (int32_t)ML.size() - 1;
    };
    // the frame and the incoming list first, then every key frame and point reached, until nothing new turns up
    const int N = mCurrentFrame.N, NL = (int)mCurrentFrame.mvpMapLines.size();
    std::vector<int32_t> frame_match(N > 0 ? N : 1, -1), frame_line_match(NL > 0 ? NL : 1, -1), local_in;
    for (int i = 0; i < N; i++) frame_match[i] = pt_of(mCurrentFrame.mvpMapPoints[i]);
    for (int i = 0; i < NL; i++) frame_line_match[i] = ml_of(mCurrentFrame.mvpMapLines[i]);
    for (KeyFrame* pKF : mvpLocalKeyFrames) local_in.push_back(kf_of(pKF));
    std::vector<std::vector<int32_t>> covis_of, child_of, slots_of, lslots_of, obs_of;
    std::vector<int32_t> parent_of;
    size_t kdone = 0, pdone = 0;
    while (kdone < K.size() || pdone < P.size()) {
        for (; kdone < K.size() && K.size() <= PLANAR_LOCALMAP_MAX_KEYFRAMES; kdone++) {
            KeyFrame* pKF = K[kdone];
            std::vector<int32_t> c, ch, sl, ls;
            const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (size_t t = 0; t < vNeighs.size() && t < 10; t++) c.push_back(kf_of(vNeighs[t]));
            const std::set<KeyFrame*> spChilds = pKF->GetChilds();
            for (KeyFrame* pChild : spChilds) ch.push_back(kf_of(pChild));
            const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
            for (MapPoint* pMP : vpMPs) sl.push_back(pt_of(pMP));
            const std::vector<MapLine*> vpMLs = pKF->GetMapLineMatches();
            for (MapLine* pML : vpMLs) ls.push_back(ml_of(pML));
            parent_of.push_back(kf_of(pKF->GetParent()));
            covis_of.push_back(c); child_of.push_back(ch); slots_of.push_back(sl); lslots_of.push_back(ls);
        }
        if (K.size() > PLANAR_LOCALMAP_MAX_KEYFRAMES) {
            std::fprintf(stderr, "planar (UpdateLocalMap): more than %d key frames - the local map is left as it is\n", PLANAR_LOCALMAP_MAX_KEYFRAMES);
            return;
        }
        for (; pdone < P.size(); pdone++) {
            std::vector<int32_t> o;
            const std::map<KeyFrame*, size_t> observations = P[pdone]->GetObservations();
            for (const auto& kv : observations) o.push_back(kf_of(kv.first));
            obs_of.push_back(o);
        }
    }
    const size_t nk = K.size(), np = P.size(), nl = ML.size();
    if (nk == 0) return;
    const size_t S = nk, PS = np ? np : 1, LS = nl ? nl : 1;
    size_t SS = 1, LSS = 1, OC = 1, CC = 1;
    for (size_t k = 0; k < nk; k++) { SS = std::max(SS, slots_of[k].size()); LSS = std::max(LSS, lslots_of[k].size()); }
    std::vector<uint8_t> kf_bad(S), pt_bad(PS, 0), ml_bad(LS, 0), ml_observed(LS, 1);
    std::vector<int32_t> kf_rank(S), covis(S * 10, -1), parent(parent_of), child_off(S + 1, 0), child, n_slots(S), kf_pts(S * SS, -1), n_lslots(S), kf_lines(S * LSS, -1),
        obs_off(PS + 1, 0), obs_kf;
    {
        int32_t r = 0;
        for (const auto& kv : kf_id) kf_rank[kv.second] = r++;      // std::map<KeyFrame*, ...>: std::less<KeyFrame*>, the order of the reference's keyframeCounter
    }
    for (size_t k = 0; k < nk; k++) {
        kf_bad[k] = K[k]->isBad();
        std::copy(covis_of[k].begin(), covis_of[k].end(), covis.begin() + k * 10);
        child.insert(child.end(), child_of[k].begin(), child_of[k].end());
        child_off[k + 1] = (int32_t)child.size();
        n_slots[k] = (int32_t)slots_of[k].size(); std::copy(slots_of[k].begin(), slots_of[k].end(), kf_pts.begin() + k * SS);
        n_lslots[k] = (int32_t)lslots_of[k].size(); std::copy(lslots_of[k].begin(), lslots_of[k].end(), kf_lines.begin() + k * LSS);
    }
    for (size_t p = 0; p < np; p++) {
        pt_bad[p] = P[p]->isBad();
        obs_kf.insert(obs_kf.end(), obs_of[p].begin(), obs_of[p].end());
        obs_off[p + 1] = (int32_t)obs_kf.size();
    }
    for (size_t p = np; p < PS; p++) obs_off[p + 1] = obs_off[np];
    for (size_t l = 0; l < nl; l++) ml_bad[l] = ML[l]->isBad();
    OC = std::max(OC, obs_kf.size()); CC = std::max(CC, child.size());
    obs_kf.resize(OC, 0); child.resize(CC, 0);
    // the rows the next calls would read are not needed here: zeros
    std::vector<float> zf(std::max(PS * 3, LS), 0.f);
    std::vector<double> zd(LS * 6, 0.0);
    std::vector<uint8_t> zb(std::max(PS, LS) * 32, 0);
    planar_local_map m;
    m.n_maps = 1; m.kf_stride = (int32_t)S; m.slot_stride = (int32_t)SS; m.line_slot_stride = (int32_t)LSS; m.pt_stride = (int32_t)PS; m.ml_stride = (int32_t)LS;
    m.obs_cap = (int32_t)OC; m.child_cap = (int32_t)CC;
    const int32_t n_kf = (int32_t)nk, n_pts = (int32_t)np, n_ml = (int32_t)nl, map_of = 0, n_frame = N > 0 ? N : 0, n_frame_lines = NL;
    m.n_kf = &n_kf; m.kf_bad = kf_bad.data(); m.kf_rank = kf_rank.data(); m.covis = covis.data(); m.parent = parent.data(); m.child_off = child_off.data();
    m.child = child.data(); m.n_slots = n_slots.data(); m.kf_pts = kf_pts.data(); m.n_line_slots = n_lslots.data(); m.kf_lines = kf_lines.data(); m.n_pts = &n_pts;
    m.pt_bad = pt_bad.data(); m.obs_off = obs_off.data(); m.obs_kf = obs_kf.data(); m.pt_xw = zf.data(); m.pt_normal = zf.data(); m.pt_min_dist = zf.data();
    m.pt_max_dist = zf.data(); m.pt_desc = zb.data(); m.n_ml = &n_ml; m.ml_bad = ml_bad.data(); m.ml_observed = ml_observed.data(); m.ml_xw6 = zd.data();
    m.ml_normal = zd.data(); m.ml_min_dist = zf.data(); m.ml_max_dist = zf.data(); m.ml_desc = zb.data();
    // every point / line can be listed at most once, every key frame too
    std::vector<int32_t> local_kf(S, -1), lp_id(PS, -1), ll_id(LS, -1);
    std::copy(local_in.begin(), local_in.begin() + std::min(local_in.size(), S), local_kf.begin());
    int32_t n_local_kf = (int32_t)std::min(local_in.size(), S), ref_kf = -1, n_lp = 0, n_ll = 0, status = 0;
    std::vector<uint8_t> lp_u8(PS * 2), ll_u8(LS * 2), lp_desc(PS * 32), ll_desc(LS * 32);
    std::vector<float> lp_f(PS * 8), ll_f(LS * 2);
    std::vector<double> ll_d(LS * 9);
    std::vector<int32_t> line_match_copy(frame_line_match);       // the lines' nulling is SearchLocalLines' (:2339); the frame's own vector is not touched here
    const bool done = planar_adapter::on_lane(planar_adapter::TRACKING, "planar_update_local_map", [&](planar_ctx* ctx) -> int {
        planar_local_map_ws* ws = nullptr;
        int rc = planar_local_map_ws_create(ctx, 1, (int)S, (int)PS, (int)LS, &ws);
        if (rc != PLANAR_OK) return rc;
        rc = planar_update_local_map(ws, &m, 1, &map_of, &n_frame, frame_match.data(), (int)frame_match.size(), &n_frame_lines, line_match_copy.data(),
                                     (int)line_match_copy.size(), local_kf.data(), &n_local_kf, (int)S, &ref_kf, lp_id.data(), &n_lp, lp_u8.data(), lp_f.data(),
                                     lp_f.data() + PS * 3, lp_f.data() + PS * 6, lp_f.data() + PS * 7, lp_desc.data(), lp_u8.data() + PS, (int)PS, ll_id.data(), &n_ll,
                                     ll_u8.data(), ll_d.data(), ll_d.data() + LS * 6, ll_f.data(), ll_f.data() + LS, ll_desc.data(), ll_u8.data() + LS, (int)LS, &status);
        planar_local_map_ws_destroy(ws);
        return rc;
    });
    if (!done) return;
    if (status != 0 && status != 1) {
        std::fprintf(stderr, "planar (UpdateLocalMap): frame status %d - the local map is left as it is\n", (int)status);
        return;
    }
    for (int i = 0; i < N; i++)
        if (frame_match[i] < 0 && mCurrentFrame.mvpMapPoints[i]) mCurrentFrame.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);     // :2470
    if (status == 0) {                                                                                                             // :2481-2499, :2548-2551
        mvpLocalKeyFrames.clear();
        for (int i = 0; i < n_local_kf; i++) mvpLocalKeyFrames.push_back(K[local_kf[i]]);
        if (ref_kf >= 0) { mpReferenceKF = K[ref_kf]; mCurrentFrame.mpReferenceKF = mpReferenceKF; }
    }
    mvpLocalMapPoints.clear();
    for (int i = 0; i < n_lp; i++) mvpLocalMapPoints.push_back(P[lp_id[i]]);
    mvpLocalMapLines.clear();
    for (int i = 0; i < n_ll; i++) mvpLocalMapLines.push_back(ML[ll_id[i]]);
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_LOCAL_MAP

// ---- KeyFrame::UpdateConnections (src/KeyFrame.cc:298-432).  Enabled with PLANAR_ADAPTERS_WITH_CONNECTIONS, after the reference's KeyFrame.h and MapPoint.h; leave
//      that body of src/KeyFrame.cc out (AddConnection, UpdateBestCovisibles and AddChild stay the reference's).  The key frame's map points are copied under
//      mMutexFeatures and their isBad() / GetObservations() gathered into a ONE-ENTRY problem: key frame ids are places in std::less<KeyFrame*> order of the key
//      frames met (so kf_rank is the identity), only this key frame has slots, and the graph comes in empty apart from this key frame's mbFirstConnection and
//      whether its mnId is 0.  planar_update_connections runs with L = 1 on the tracking lane; from its result come the counter (row j), the key frame's ordered
//      list (exactly the targets, sorted) and the parent.  The targets' own state is the reference's: AddConnection(this, w) is called on each, as :397 / :404 do.
//      It is the correctness path; the throughput path is planar_update_connections_dev on a resident map.  A failing call, or more than
//      PLANAR_LOCALMAP_MAX_KEYFRAMES key frames met, changes nothing and reports on stderr.
#ifdef PLANAR_ADAPTERS_WITH_CONNECTIONS
#include <map>
#include <mutex>
namespace Planar_SLAM {
inline void KeyFrame::UpdateConnections() {
    std::vector<MapPoint*> vpMP;
    {
        std::unique_lock<std::mutex> lockMPs(mMutexFeatures);
        vpMP = mvpMapPoints;
    }
    std::map<MapPoint*, int32_t> pt_id;
    std::vector<std::map<KeyFrame*, size_t>> obs_of;
    std::vector<uint8_t> pt_bad;
    std::map<KeyFrame*, int32_t> kf_id;                  // std::less<KeyFrame*>: the order of the reference's KFcounter
    kf_id[this] = 0;
    std::vector<int32_t> kf_pts(vpMP.size() ? vpMP.size() : 1, -1);
    for (size_t i = 0; i < vpMP.size(); i++) {
        MapPoint* pMP = vpMP[i];
        if (!pMP) continue;
        auto it = pt_id.find(pMP);
        if (it == pt_id.end()) {
            it = pt_id.emplace(pMP, (int32_t)pt_bad.size()).first;
            const bool bad = pMP->isBad();
            pt_bad.push_back(bad);
            obs_of.push_back(bad ? std::map<KeyFrame*, size_t>() : pMP->GetObservations());
            for (const auto& kv : obs_of.back()) kf_id[kv.first] = 0;
        }
        kf_pts[i] = it->second;
    }
    if (kf_id.size() > PLANAR_LOCALMAP_MAX_KEYFRAMES) {
        std::fprintf(stderr, "planar (UpdateConnections): more than %d key frames - the connections are left as they are\n", PLANAR_LOCALMAP_MAX_KEYFRAMES);
        return;
    }
    std::vector<KeyFrame*> K;
    for (auto& kv : kf_id) { kv.second = (int32_t)K.size(); K.push_back(kv.first); }
    const size_t S = K.size(), PS = pt_bad.size() ? pt_bad.size() : 1;
    const int32_t j = kf_id[this];
    // a self observation is skipped on mnId, not on the pointer (:329): a key frame that shares this one's mnId must not count either
    std::vector<int32_t> obs_off(PS + 1, 0), obs_kf;
    for (size_t p = 0; p < obs_of.size(); p++) {
        for (const auto& kv : obs_of[p])
            if (kv.first->mnId != mnId) obs_kf.push_back(kf_id[kv.first]);
        obs_off[p + 1] = (int32_t)obs_kf.size();
    }
    for (size_t p = obs_of.size(); p < PS; p++) obs_off[p + 1] = obs_off[obs_of.size()];
    if (obs_kf.empty()) obs_kf.push_back(0);
    pt_bad.resize(PS, 0);
    const size_t SS = kf_pts.size();
    std::vector<int32_t> kf_rank(S), n_slots(S, 0), slots(S * SS, -1);
    for (size_t k = 0; k < S; k++) kf_rank[k] = (int32_t)k;
    n_slots[j] = (int32_t)vpMP.size();
    std::copy(kf_pts.begin(), kf_pts.end(), slots.begin() + (size_t)j * SS);
    planar_local_map m{};
    m.n_maps = 1; m.kf_stride = (int32_t)S; m.slot_stride = (int32_t)SS; m.line_slot_stride = 1; m.pt_stride = (int32_t)PS; m.ml_stride = 1;
    m.obs_cap = (int32_t)obs_kf.size(); m.child_cap = 1;
    const int32_t n_kf = (int32_t)S, n_pts = (int32_t)obs_of.size();
    m.n_kf = &n_kf; m.kf_rank = kf_rank.data(); m.n_slots = n_slots.data(); m.kf_pts = slots.data(); m.n_pts = &n_pts; m.pt_bad = pt_bad.data();
    m.obs_off = obs_off.data(); m.obs_kf = obs_kf.data();
    std::vector<int32_t> conn_w(S * S, 0), ord_n(S, 0), ord_kf(S * S, -1), ord_w(S * S, 0), kf_mnid(S, 1), parent(S, -1), covis(S * 10, -1);
    std::vector<uint8_t> first(S, 0);
    {
        std::unique_lock<std::mutex> lockCon(mMutexConnections);
        first[j] = mbFirstConnection;
    }
    kf_mnid[j] = mnId != 0;
    planar_covis_graph gr;
    gr.conn_w = conn_w.data(); gr.ord_n = ord_n.data(); gr.ord_kf = ord_kf.data(); gr.ord_w = ord_w.data(); gr.first_connection = first.data();
    gr.kf_mnid = kf_mnid.data(); gr.parent = parent.data(); gr.covis = covis.data();
    const int32_t entry_map = 0, entry_kf = j;
    int32_t new_parent = -1, status = -1;
    const bool done = planar_adapter::on_lane(planar_adapter::TRACKING, "planar_update_connections", [&](planar_ctx* ctx) -> int {
        planar_connections_ws* ws = nullptr;
        int rc = planar_connections_ws_create(ctx, 1, 1, (int)S, &ws);
        if (rc != PLANAR_OK) return rc;
        rc = planar_update_connections(ws, &m, &gr, 1, &entry_map, &entry_kf, &new_parent, &status);
        planar_connections_ws_destroy(ws);
        return rc;
    });
    if (!done) return;
    if (status == 1) return;                             // This should not happen (:376)
    if (status != 0) {
        std::fprintf(stderr, "planar (UpdateConnections): entry status %d - the connections are left as they are\n", (int)status);
        return;
    }
    const int n = ord_n[j];
    std::map<KeyFrame*, int> KFcounter;
    for (size_t k = 0; k < S; k++)
        if (conn_w[(size_t)j * S + k] > 0) KFcounter[K[k]] = conn_w[(size_t)j * S + k];
    std::vector<KeyFrame*> vpOrdered;
    std::vector<int> vOrderedWeights;
    for (int i = 0; i < n; i++) { vpOrdered.push_back(K[ord_kf[(size_t)j * S + i]]); vOrderedWeights.push_back(ord_w[(size_t)j * S + i]); }
    for (int i = 0; i < n; i++) vpOrdered[i]->AddConnection(this, vOrderedWeights[i]);      // the key frame's ordered list is exactly the targets (:394-405)
    {
        std::unique_lock<std::mutex> lockCon(mMutexConnections);
        mConnectedKeyFrameWeights = KFcounter;
        mvpOrderedConnectedKeyFrames = vpOrdered;
        mvOrderedWeights = vOrderedWeights;
        if (mbFirstConnection && mnId != 0 && new_parent >= 0) {
            mpParent = K[new_parent];
            mpParent->AddChild(this);
            mbFirstConnection = false;
        }
    }
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_CONNECTIONS

// ---- Tracking::NeedNewKeyFrame (src/Tracking.cc:2049-2137) and Tracking::CreateNewKeyFrame (:2139-2285).  Enabled with PLANAR_ADAPTERS_WITH_KEYFRAME, after the
//      reference's Tracking.h, Frame.h, KeyFrame.h, MapPoint.h, MapLine.h, MapPlane.h, Map.h and LocalMapping.h; leave those two bodies of src/Tracking.cc out.
//      Both pack the current frame into a ONE-FRAME problem on a one-map planar_map_edit and call the host form with B = 1 on the tracking lane: the correctness
//      path; the throughput path is the _dev calls on a resident map.  Map points and lines are numbered as the frame (and, for the
//      decision, the reference key frame) meets them; their Observations() are pt_nobs / ml_nobs.
//      NeedNewKeyFrame: the only key frame of the packed map is mpReferenceKF; the call counts and cleans again what Track() counted and cleaned before it
//      (:1973-2003, :321-336), which changes nothing on a frame that went through those, and the member mnMatchesInliers is handed through: n_plane_inliers is
//      what the member holds beyond the point and line inliers the call counts.  InterruptBA() is called where the reference calls it.
//      CreateNewKeyFrame: the packed map has no key frame yet (new_rank 0) and no rows worth copying; the call gives the key points and lines that create, in
//      creation order, and new MapPoint / AddObservation / AddMapPoint / ... run on the objects in that order, as the reference's walk does.  The plane loop
//      works on MapPlane objects and stays on the host.  A failing call creates no point and no line (the key frame is still inserted) and reports on stderr.
#ifdef PLANAR_ADAPTERS_WITH_KEYFRAME
#include <iostream>
#include <map>
namespace planar_adapter {
// the frame's matches as ids, with the Observations() of every object met; ids are handed out in the order of meeting
template <class T> struct ObjectIds {
    std::map<T*, int32_t> id;
    std::vector<T*> object;
    std::vector<int32_t> nobs;
    std::vector<uint8_t> bad;
    int32_t of(T* p) {
        if (!p) return -1;
        auto it = id.find(p);
        if (it != id.end()) return it->second;
        id[p] = (int32_t)object.size();
        object.push_back(p); nobs.push_back(p->Observations()); bad.push_back(p->isBad());
        return (int32_t)object.size() - 1;
    }
};
template <class V> inline V* data_or_one(std::vector<V>& v) { if (v.empty()) v.resize(1); return v.data(); }
}  // namespace planar_adapter

namespace Planar_SLAM {
inline bool Tracking::NeedNewKeyFrame() {
    Frame& F = mCurrentFrame;
    const int N = F.N, NL = F.NL;
    planar_adapter::ObjectIds<MapPoint> pts;
    planar_adapter::ObjectIds<MapLine> mls;
    std::vector<int32_t> match(N > 0 ? N : 1, -1), lmatch(NL > 0 ? NL : 1, -1);
    std::vector<uint8_t> outl(match.size(), 0), loutl(lmatch.size(), 0);
    std::vector<float> depth(match.size(), -1.f);
    int counted = 0;                                     // what the call will count itself of mnMatchesInliers
    for (int i = 0; i < N; i++) {
        match[i] = pts.of(F.mvpMapPoints[i]); outl[i] = F.mvbOutlier[i]; depth[i] = F.mvDepth[i];
        if (match[i] >= 0 && !outl[i] && (mbOnlyTracking || pts.nobs[match[i]] > 0)) counted++;
    }
    for (int i = 0; i < NL; i++) {
        lmatch[i] = mls.of(F.mvpMapLines[i]); loutl[i] = F.mvbLineOutlier[i];
        if (lmatch[i] >= 0 && !loutl[i] && (mbOnlyTracking || mls.nobs[lmatch[i]] > 0)) counted++;
    }
    const std::vector<MapPoint*> ref = mpReferenceKF->GetMapPointMatches();
    std::vector<int32_t> slots(ref.size() ? ref.size() : 1, -1);
    for (size_t i = 0; i < ref.size(); i++) slots[i] = pts.of(ref[i]);
    planar_map_edit m{};
    m.n_maps = 1; m.kf_stride = 1; m.slot_stride = (int32_t)slots.size(); m.line_slot_stride = 1; m.pt_stride = (int32_t)(pts.object.size() ? pts.object.size() : 1);
    m.ml_stride = (int32_t)(mls.object.size() ? mls.object.size() : 1); m.obs_cap = 1; m.ml_obs_cap = 1;
    int32_t n_kf = 1, n_slots = (int32_t)ref.size(), n_pts = (int32_t)pts.object.size(), n_ml = (int32_t)mls.object.size();
    m.n_kf = &n_kf; m.n_slots = &n_slots; m.kf_pts = slots.data(); m.n_pts = &n_pts; m.pt_bad = planar_adapter::data_or_one(pts.bad);
    m.pt_nobs = planar_adapter::data_or_one(pts.nobs); m.n_ml = &n_ml; m.ml_nobs = planar_adapter::data_or_one(mls.nobs);
    planar_kf_frames fr{};
    const int32_t map_of = 0, ref_kf = 0;
    fr.B = 1; fr.frame_stride = (int32_t)match.size(); fr.frame_line_stride = (int32_t)lmatch.size();
    fr.map_of = &map_of; fr.n_frame = &N; fr.frame_match = match.data(); fr.outlier = outl.data(); fr.depth = depth.data();
    fr.n_frame_lines = &NL; fr.frame_line_match = lmatch.data(); fr.line_outlier = loutl.data();
    planar_need_kf_params prm{};
    prm.frame_id = F.mnId; prm.last_reloc_frame_id = mnLastRelocFrameId; prm.last_kf_frame_id = mnLastKeyFrameId; prm.max_frames = mMaxFrames; prm.min_frames = mMinFrames;
    prm.th_depth = mThDepth; prm.n_kfs_in_map = (int32_t)mpMap->KeyFramesInMap(); prm.n_plane_inliers = mnMatchesInliers - counted;
    prm.flags = (mbOnlyTracking ? PLANAR_NEEDKF_ONLY_TRACKING : 0) | ((mpLocalMapper->isStopped() || mpLocalMapper->stopRequested()) ? PLANAR_NEEDKF_MAPPER_STOPPED : 0) |
                (mpLocalMapper->AcceptKeyFrames() ? PLANAR_NEEDKF_MAPPER_ACCEPTS : 0) | (F.mbNewPlane ? PLANAR_NEEDKF_NEW_PLANE : 0);
    prm.keyframes_in_queue = mpLocalMapper->KeyframesInQueue();
    int32_t out[PLANAR_NEEDKF_NOUT] = {0};
    const bool done = planar_adapter::on_lane(planar_adapter::TRACKING, "planar_need_new_key_frame", [&](planar_ctx* ctx) -> int {
        planar_keyframe_ws* ws = nullptr;
        int rc = planar_keyframe_ws_create(ctx, 1, 1, m.pt_stride, m.ml_stride, 1, 1, &ws);
        if (rc != PLANAR_OK) return rc;
        rc = planar_need_new_key_frame(ws, &m, &fr, &ref_kf, &prm, out);
        planar_keyframe_ws_destroy(ws);
        return rc;
    });
    if (!done || out[PLANAR_NEEDKF_STATUS] != 0) return false;
    for (int i = 0; i < N; i++) {                        // the clean step's result; nothing changes on a frame Track() cleaned already
        if (match[i] < 0) F.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
        F.mvbOutlier[i] = outl[i] != 0;
    }
    for (int i = 0; i < NL; i++) {
        if (lmatch[i] < 0) F.mvpMapLines[i] = static_cast<MapLine*>(NULL);
        F.mvbLineOutlier[i] = loutl[i] != 0;
    }
    if (out[PLANAR_NEEDKF_INTERRUPT_BA]) mpLocalMapper->InterruptBA();
    return out[PLANAR_NEEDKF_NEED] != 0;
}

inline void Tracking::CreateNewKeyFrame() {
    if (!mpLocalMapper->SetNotStop(true)) return;
    KeyFrame* pKF = new KeyFrame(mCurrentFrame, mpMap, mpKeyFrameDB);
    mpReferenceKF = pKF;
    mCurrentFrame.mpReferenceKF = pKF;
    if (mSensor != System::MONOCULAR) {
        Frame& F = mCurrentFrame;
        F.UpdatePoseMatrices();
        const int N = F.N, NL = F.NL;
        planar_adapter::ObjectIds<MapPoint> pts;
        planar_adapter::ObjectIds<MapLine> mls;
        const size_t FS = N > 0 ? N : 1, FLS = NL > 0 ? NL : 1;
        std::vector<int32_t> match(FS, -1), lmatch(FLS, -1);
        std::vector<float> depth(FS, -1.f), u_right(FS, -1.f), depth_line(FLS, -1.f);
        for (int i = 0; i < N; i++) { match[i] = pts.of(F.mvpMapPoints[i]); depth[i] = F.mvDepth[i]; u_right[i] = F.mvuRight[i]; }
        for (int i = 0; i < NL; i++) { lmatch[i] = mls.of(F.mvpMapLines[i]); depth_line[i] = F.mvDepthLine[i]; }
        // a one-map problem without a key frame: room for one, and for every key point and line to create
        const int32_t np0 = (int32_t)pts.object.size(), nl0 = (int32_t)mls.object.size();
        const size_t PS = np0 + FS, LS = nl0 + FLS;
        int32_t n_kf = 0, n_pts = np0, n_ml = nl0, kf_rank = 0, parent = -1, n_slots = 0, n_line_slots = 0, child_off[2] = {0, 0}, covis[10];
        uint8_t kf_bad = 0;
        std::vector<int32_t> kf_pts(FS, -1), kf_lines(FLS, -1), obs_off(PS + 1, 0), obs_kf(FS, 0), pt_nobs(PS, 0), ml_obs_off(LS + 1, 0), ml_obs_kf(FLS, 0), ml_nobs(LS, 0);
        std::vector<uint8_t> pt_bad(PS, 0), ml_bad(LS, 0), ml_observed(LS, 0), pt_desc(PS * 32, 0), ml_desc(LS * 32, 0), desc(FS * 32, 0), line_desc(FLS * 32, 0);
        std::vector<float> pt_xw(PS * 3, 0.f), pt_normal(PS * 3, 0.f), pt_min(PS, 0.f), pt_max(PS, 0.f), ml_min(LS, 0.f), ml_max(LS, 0.f), xw(FS * 3, 0.f), normal(FS * 3, 0.f),
            fmin_(FS, 0.f), fmax_(FS, 0.f), lmin(FLS, 0.f), lmax(FLS, 0.f);
        std::vector<double> ml_xw6(LS * 6, 0.0), ml_normal(LS * 3, 0.0), xw6(FLS * 6, 0.0), line_normal(FLS * 3, 0.0);
        for (int32_t p = 0; p < np0; p++) { pt_nobs[p] = pts.nobs[p]; pt_bad[p] = pts.bad[p]; }
        for (int32_t p = 0; p < nl0; p++) { ml_nobs[p] = mls.nobs[p]; ml_bad[p] = mls.bad[p]; ml_observed[p] = mls.nobs[p] > 0; }
        planar_map_edit m{};
        m.n_maps = 1; m.kf_stride = 1; m.slot_stride = (int32_t)FS; m.line_slot_stride = (int32_t)FLS; m.pt_stride = (int32_t)PS; m.ml_stride = (int32_t)LS;
        m.obs_cap = (int32_t)FS; m.ml_obs_cap = (int32_t)FLS;
        m.n_kf = &n_kf; m.kf_bad = &kf_bad; m.kf_rank = &kf_rank; m.parent = &parent; m.covis = covis; m.child_off = child_off; m.n_slots = &n_slots; m.kf_pts = kf_pts.data();
        m.n_line_slots = &n_line_slots; m.kf_lines = kf_lines.data(); m.n_pts = &n_pts; m.pt_bad = pt_bad.data(); m.obs_off = obs_off.data(); m.obs_kf = obs_kf.data();
        m.pt_nobs = pt_nobs.data(); m.pt_xw = pt_xw.data(); m.pt_normal = pt_normal.data(); m.pt_min_dist = pt_min.data(); m.pt_max_dist = pt_max.data();
        m.pt_desc = pt_desc.data(); m.n_ml = &n_ml; m.ml_bad = ml_bad.data(); m.ml_observed = ml_observed.data(); m.ml_obs_off = ml_obs_off.data();
        m.ml_obs_kf = ml_obs_kf.data(); m.ml_nobs = ml_nobs.data(); m.ml_xw6 = ml_xw6.data(); m.ml_normal = ml_normal.data(); m.ml_min_dist = ml_min.data();
        m.ml_max_dist = ml_max.data(); m.ml_desc = ml_desc.data();
        planar_kf_frames fr{};
        const int32_t map_of = 0, new_rank = 0, mnid = 0;
        const uint8_t create = 1;
        const float th = mThDepth;
        fr.B = 1; fr.frame_stride = (int32_t)FS; fr.frame_line_stride = (int32_t)FLS;
        fr.map_of = &map_of; fr.n_frame = &N; fr.frame_match = match.data(); fr.depth = depth.data(); fr.u_right = u_right.data(); fr.xw = xw.data();
        fr.normal = normal.data(); fr.min_dist = fmin_.data(); fr.max_dist = fmax_.data(); fr.desc = desc.data(); fr.n_frame_lines = &NL;
        fr.frame_line_match = lmatch.data(); fr.depth_line = depth_line.data(); fr.xw6 = xw6.data(); fr.line_normal = line_normal.data(); fr.line_min_dist = lmin.data();
        fr.line_max_dist = lmax.data(); fr.line_desc = line_desc.data();
        std::vector<int32_t> created_pt(FS, -1), created_ml(FLS, -1);
        int32_t new_kf = -1, n_created_pt = 0, n_created_ml = 0, status = -1;
        const bool done = planar_adapter::on_lane(planar_adapter::TRACKING, "planar_create_new_key_frame", [&](planar_ctx* ctx) -> int {
            planar_keyframe_ws* ws = nullptr;
            int rc = planar_keyframe_ws_create(ctx, 1, 1, m.pt_stride, m.ml_stride, m.obs_cap, m.ml_obs_cap, &ws);
            if (rc != PLANAR_OK) return rc;
            rc = planar_create_new_key_frame(ws, &m, &fr, &create, &th, &new_rank, &mnid, &new_kf, created_pt.data(), &n_created_pt, created_ml.data(), &n_created_ml, &status);
            planar_keyframe_ws_destroy(ws);
            return rc;
        });
        if (done && status != 0) std::fprintf(stderr, "planar (CreateNewKeyFrame): frame status %d - no map point and no map line is created\n", (int)status);
        if (done && status == 0) {
            for (int c = 0; c < n_created_pt; c++) {     // in creation order: the order of the reference's sorted walk
                const int i = created_pt[c];
                cv::Mat x3D = F.UnprojectStereo(i);
                MapPoint* pNewMP = new MapPoint(x3D, pKF, mpMap);
                pNewMP->AddObservation(pKF, i);
                pKF->AddMapPoint(pNewMP, i);
                pNewMP->ComputeDistinctiveDescriptors();
                pNewMP->UpdateNormalAndDepth();
                mpMap->AddMapPoint(pNewMP);
                F.mvpMapPoints[i] = pNewMP;
            }
            for (int c = 0; c < n_created_ml; c++) {
                const int i = created_ml[c];
                Vector6d line3D = F.obtain3DLine(i);
                MapLine* pNewML = new MapLine(line3D, pKF, mpMap);
                pNewML->AddObservation(pKF, i);
                pKF->AddMapLine(pNewML, i);
                pNewML->ComputeDistinctiveDescriptors();
                pNewML->UpdateAverageDir();
                mpMap->AddMapLine(pNewML);
                F.mvpMapLines[i] = pNewML;
            }
        }
        // the planes: observations of the matched ones, a new MapPlane for an unmatched inlier, an unmatched outlier forgiven (:2248-2272)
        for (int i = 0; i < F.mnPlaneNum; ++i) {
            const bool inlier = !F.mvbPlaneOutlier[i];
            if (inlier && F.mvpParallelPlanes[i]) F.mvpParallelPlanes[i]->AddParObservation(pKF, i);
            if (inlier && F.mvpVerticalPlanes[i]) F.mvpVerticalPlanes[i]->AddVerObservation(pKF, i);
            if (F.mvpMapPlanes[i]) {
                F.mvpMapPlanes[i]->AddObservation(pKF, i);
            } else if (!inlier) {
                F.mvbPlaneOutlier[i] = false;
            } else {
                cv::Mat p3D = F.ComputePlaneWorldCoeff(i);
                MapPlane* pNewPlane = new MapPlane(p3D, pKF, mpMap);
                pNewPlane->AddObservation(pKF, i);
                pKF->AddMapPlane(pNewPlane, i);
                pNewPlane->UpdateCoefficientsAndPoints();
                mpMap->AddMapPlane(pNewPlane);
            }
        }
        mpPointCloudMapping->print();
        std::cout << "New map created with " << mpMap->MapPlanesInMap() << " planes" << std::endl;
    }
    mpLocalMapper->InsertKeyFrame(pKF);
    mpLocalMapper->SetNotStop(false);
    mnLastKeyFrameId = mCurrentFrame.mnId;
    mpLastKeyFrame = pKF;
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_KEYFRAME

// ---- Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*)  (src/Optimizer.cc:1853-2680): the graph the reference assembles from the covisibility
//      list and the observation maps becomes a planar_ba_problem, planar_local_ba solves it, the erase lists and the optimised values go back.
//      Define PLANAR_ADAPTERS_WITH_LOCAL_BA after including KeyFrame.h, MapPoint.h, MapLine.h, MapPlane.h, Map.h, Optimizer.h, Config.h. --------------
#ifdef PLANAR_ADAPTERS_WITH_LOCAL_BA
#include <list>
namespace Planar_SLAM {
inline void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap) {
    // local key frames, local landmarks, fixed cameras: the reference's traversal (:1855-1974), marks included
    std::vector<KeyFrame*> kfs;
    kfs.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    for (KeyFrame* k : pKF->GetVectorCovisibleKeyFrames()) { k->mnBALocalForKF = pKF->mnId; if (!k->isBad()) kfs.push_back(k); }
    const size_t n_local = kfs.size();
    std::vector<MapPoint*> pts; std::vector<MapLine*> lns; std::vector<MapPlane*> pls;
    for (size_t i = 0; i < n_local; i++) {
        for (MapPoint* p : kfs[i]->GetMapPointMatches()) if (p && !p->isBad() && p->mnBALocalForKF != pKF->mnId) { pts.push_back(p); p->mnBALocalForKF = pKF->mnId; }
    }
    for (size_t i = 0; i < n_local; i++) {
        for (MapLine* p : kfs[i]->GetMapLineMatches()) if (p && !p->isBad() && p->mnBALocalForKF != pKF->mnId) { lns.push_back(p); p->mnBALocalForKF = pKF->mnId; }
    }
    for (size_t i = 0; i < n_local; i++) {
        for (MapPlane* p : kfs[i]->GetMapPlaneMatches()) if (p && !p->isBad() && p->mnBALocalForKF != pKF->mnId) { pls.push_back(p); p->mnBALocalForKF = pKF->mnId; }
    }
    auto fix_observers = [&](const std::map<KeyFrame*, size_t>& obs) {
        for (const auto& o : obs) {
            KeyFrame* k = o.first;
            if (k->mnBALocalForKF != pKF->mnId && k->mnBAFixedForKF != pKF->mnId) { k->mnBAFixedForKF = pKF->mnId; if (!k->isBad()) kfs.push_back(k); }
        }
    };
    for (MapPoint* p : pts) fix_observers(p->GetObservations());
    for (MapLine* p : lns) fix_observers(p->GetObservations());
    for (MapPlane* p : pls) fix_observers(p->GetObservations());
    const int K = (int)kfs.size();
    std::map<KeyFrame*, int> kf_index;
    std::vector<float> kf_Tcw((size_t)K * 16);
    std::vector<uint8_t> kf_fixed(K);
    unsigned long maxKFid = 0;
    for (int k = 0; k < K; k++) {
        kf_index[kfs[k]] = k;
        planar_adapter::mat_to_array(kfs[k]->GetPose(), &kf_Tcw[(size_t)k * 16]);
        kf_fixed[k] = (size_t)k >= n_local || kfs[k]->mnId == 0;
        if (kfs[k]->mnId > maxKFid) maxKFid = kfs[k]->mnId;
    }
    // landmarks and edges
    std::vector<uint8_t> lm_type, e_type;
    std::vector<double> lm_init, e_meas;
    std::vector<int32_t> e_kf, e_lm;
    std::vector<float> e_is2;
    struct Assoc { KeyFrame* kf; void* lm; };                 // what an erased edge removes
    std::vector<Assoc> assoc;
    auto add_lm = [&](int type, double a, double b, double c, double d) { lm_type.push_back((uint8_t)type); lm_init.insert(lm_init.end(), {a, b, c, d}); return (int32_t)lm_type.size() - 1; };
    auto add_edge = [&](int kf, int lm, int type, double m0, double m1, double m2, double m3, float is2, KeyFrame* okf, void* olm) {
        e_kf.push_back(kf); e_lm.push_back(lm); e_type.push_back((uint8_t)type); e_meas.insert(e_meas.end(), {m0, m1, m2, m3}); e_is2.push_back(is2); assoc.push_back(Assoc{okf, olm});
    };
    std::vector<int32_t> pt_lm(pts.size()), ln_lm(lns.size()), pl_lm(pls.size());
    for (size_t i = 0; i < pts.size(); i++) {
        cv::Mat X = pts[i]->GetWorldPos();
        pt_lm[i] = add_lm(0, X.at<float>(0), X.at<float>(1), X.at<float>(2), 0);
        const std::map<KeyFrame*, size_t> obs = pts[i]->GetObservations();
        for (const auto& o : obs) {
            KeyFrame* k = o.first;
            if (k->isBad()) continue;
            const cv::KeyPoint& kp = k->mvKeysUn[o.second];
            const float ur = k->mvuRight[o.second], is2 = k->mvInvLevelSigma2[kp.octave];
            if (ur < 0) add_edge(kf_index.at(k), pt_lm[i], PLANAR_BA_MONO, kp.pt.x, kp.pt.y, 0, 0, is2, k, pts[i]);
            else add_edge(kf_index.at(k), pt_lm[i], PLANAR_BA_STEREO, kp.pt.x, kp.pt.y, ur, 0, is2, k, pts[i]);
        }
    }
    for (size_t i = 0; i < lns.size(); i++) {
        const auto W = lns[i]->GetWorldPos();                  // Vector6d: start xyz, end xyz
        ln_lm[i] = add_lm(0, W[0], W[1], W[2], 0);
        add_lm(0, W[3], W[4], W[5], 0);
        const std::map<KeyFrame*, size_t> obs = lns[i]->GetObservations();
        for (const auto& o : obs) {
            if (o.first->isBad()) continue;
            // both end-point edges hang on the CURRENT key frame's vertex and use its line function at the observer's slot (:2170-2194)
            const auto f = pKF->mvKeyLineFunctions[o.second];
            add_edge(0, ln_lm[i], PLANAR_BA_LINE, f[0], f[1], f[2], 0, 1.f, o.first, lns[i]);
            add_edge(0, ln_lm[i] + 1, PLANAR_BA_LINE, f[0], f[1], f[2], 0, 1.f, o.first, lns[i]);
        }
    }
    for (size_t i = 0; i < pls.size(); i++) {
        cv::Mat C = pls[i]->GetWorldPos();
        pl_lm[i] = add_lm(1, C.at<float>(0), C.at<float>(1), C.at<float>(2), C.at<float>(3));
        auto plane_edges = [&](const std::map<KeyFrame*, size_t>& obs, int type) {
            for (const auto& o : obs) {
                KeyFrame* k = o.first;
                if (k->isBad() || k->mnId > maxKFid) continue;
                auto it = kf_index.find(k);
                if (it == kf_index.end()) continue;            // (the reference would dereference a null vertex here)
                const cv::Mat& m = k->mvPlaneCoefficients[o.second];
                add_edge(it->second, pl_lm[i], type, m.at<float>(0), m.at<float>(1), m.at<float>(2), m.at<float>(3), 1.f, k, pls[i]);
            }
        };
        plane_edges(pls[i]->GetObservations(), PLANAR_BA_PLANE);
        plane_edges(pls[i]->GetVerObservations(), PLANAR_BA_VERTICAL);
        plane_edges(pls[i]->GetParObservations(), PLANAR_BA_PARALLEL);
    }
    if (pbStopFlag && *pbStopFlag) return;
    const int NL = (int)lm_type.size(), NE = (int)e_type.size();
    std::vector<float> out_T((size_t)K * 16);
    std::vector<double> out_lm((size_t)std::max(NL, 1) * 4);
    std::vector<uint8_t> out_e(std::max(NE, 1));
    planar_ba_problem P{K, kf_Tcw.data(), kf_fixed.data(), NL, lm_type.data(), lm_init.data(), NE, e_kf.data(), e_lm.data(), e_type.data(), e_meas.data(), e_is2.data()};
    planar_ba_result R{out_T.data(), out_lm.data(), out_e.data(), 0, 0};
    const planar_pose_params prm = planar_adapter::plane_pose_params<Config>(pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf);
    static_assert(sizeof(bool) == 1, "bool* pbStopFlag is passed as a byte flag");
    if (!planar_adapter::on_lane(planar_adapter::TRACKING, "planar_local_ba", [&](planar_ctx* ctx) {
            return planar_local_ba(ctx, &P, &prm, 5, 10, &R, reinterpret_cast<const volatile unsigned char*>(pbStopFlag), nullptr);
        })) return;
    // erase lists (:2471-2620) and write-back (:2622-2680) under the map mutex
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (int e = 0; e < NE; e++) {
        if (!out_e[e]) continue;
        KeyFrame* k = assoc[e].kf;
        switch (e_type[e]) {
            case PLANAR_BA_MONO: case PLANAR_BA_STEREO: { MapPoint* p = (MapPoint*)assoc[e].lm; if (p->isBad()) break; k->EraseMapPointMatch(p); p->EraseObservation(k); break; }
            case PLANAR_BA_LINE: {
                if (e > 0 && e_type[e - 1] == PLANAR_BA_LINE && assoc[e - 1].lm == assoc[e].lm && assoc[e - 1].kf == k && e_lm[e - 1] + 1 == e_lm[e]) break;   // the end-point twin
                MapLine* p = (MapLine*)assoc[e].lm; if (p->isBad()) break; k->EraseMapLineMatch(p); p->EraseObservation(k); break;
            }
            case PLANAR_BA_PLANE: { MapPlane* p = (MapPlane*)assoc[e].lm; if (p->isBad()) break; k->EraseMapPlaneMatch(p); p->EraseObservation(k); break; }
            case PLANAR_BA_VERTICAL: { MapPlane* p = (MapPlane*)assoc[e].lm; if (p->isBad()) break; k->EraseMapVerticalPlaneMatch(p); p->EraseVerObservation(k); break; }
            default: { MapPlane* p = (MapPlane*)assoc[e].lm; if (p->isBad()) break; k->EraseMapParallelPlaneMatch(p); p->EraseParObservation(k); break; }
        }
    }
    for (size_t k = 0; k < n_local; k++) kfs[k]->SetPose(planar_adapter::array_to_mat(&out_T[k * 16]));
    for (size_t i = 0; i < pts.size(); i++) {
        cv::Mat X(3, 1, CV_32F);
        for (int j = 0; j < 3; j++) X.at<float>(j) = (float)out_lm[(size_t)pt_lm[i] * 4 + j];
        pts[i]->SetWorldPos(X); pts[i]->UpdateNormalAndDepth();
    }
    for (size_t i = 0; i < lns.size(); i++) {
        auto W = lns[i]->GetWorldPos();
        for (int j = 0; j < 3; j++) { W[j] = (double)(float)out_lm[(size_t)ln_lm[i] * 4 + j]; W[3 + j] = (double)(float)out_lm[(size_t)(ln_lm[i] + 1) * 4 + j]; }   // through Converter::toCvMat (float)
        lns[i]->SetWorldPos(W); lns[i]->UpdateAverageDir();
    }
    for (size_t i = 0; i < pls.size(); i++) {
        cv::Mat C(4, 1, CV_32F);
        for (int j = 0; j < 4; j++) C.at<float>(j) = (float)out_lm[(size_t)pl_lm[i] * 4 + j];
        pls[i]->SetWorldPos(C); pls[i]->UpdateCoefficientsAndPoints();
    }
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_LOCAL_BA


// ---- The loop thread's matchers (LoopClosing::ComputeSim3, SearchAndFuse): DEFINITIONS of the four ORBmatcher members with the reference's signatures
//          int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12)                                        src/ORBmatcher.cc:526-659
//          int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12,
//                           const cv::Mat& t12, const float th)                                                                        src/ORBmatcher.cc:1106-1330
//          int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th)   :294-407
//          int Fuse(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint)          :981-1104
//      Enabled with PLANAR_ADAPTERS_WITH_LOOP_MATCHERS, after the reference's ORBmatcher.h, KeyFrame.h and MapPoint.h; leave src/ORBmatcher.cc's four bodies out.  Each
//      call gathers the key frames and map points into arrays, runs the host flavour with B = 1 on the tracking context and performs the reference's own edit
//      statements on its own objects: SearchBySim3 translates vpMatches12 through MapPoint::GetIndexInKeyFrame, Fuse performs AddObservation / AddMapPoint and fills
//      vpReplacePoint in the order of the points from `owner`.  Needs MapPoint::GetDistanceRange, the accessor of PLANAR_ADAPTERS_WITH_FUSE.  A failing call returns 0
//      and changes nothing.
#ifdef PLANAR_ADAPTERS_WITH_LOOP_MATCHERS
#include <set>
namespace planar_adapter {

// the key frame's side: key points, descriptors, bounds, grid constants, intrinsics, scale factors.  No pose: a caller that needs it adds add_pose(pKF->GetPose())
template <class KeyFrameT> inline ViewGather keyframe_view(KeyFrameT* pKF) {
    ViewGather g;
    g.add_keys(pKF->mvKeysUn, pKF->N).add_desc(pKF->mDescriptors);
    g.add_bounds(*pKF).add_grid(*pKF).add_intrinsics(*pKF).add_stereo(*pKF).add_scales(pKF->mvScaleFactors, false);
    return g;
}
// a list of map points for the searches: usable, xw, descriptor, distance range
template <class MapPointT> inline PointGather search_points(const std::vector<MapPointT*>& v) {
    PointGather p;
    p.add_points(v).add_desc(v).add_range(v);
    return p;
}

template <class KeyFrameT, class MapPointT>
int SearchByBoWKF(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12, float nn_ratio, bool check_orientation) {
    KeyFrameT* kf[2] = {pKF1, pKF2};
    std::vector<MapPointT*> mps[2] = {pKF1->GetMapPointMatches(), pKF2->GetMapPointMatches()};
    ViewGather g1 = keyframe_view(pKF1), g2 = keyframe_view(pKF2);
    std::vector<int32_t> node[2];
    std::vector<uint8_t> usable[2];
    for (int s = 0; s < 2; s++) {
        const size_t S = s ? g2.keys.size() : g1.keys.size();
        node[s].assign(S, -1); usable[s].assign(S, 0);
        for (auto it = kf[s]->mFeatVec.begin(); it != kf[s]->mFeatVec.end(); ++it)
            for (size_t k = 0; k < it->second.size(); k++) if (it->second[k] < S) node[s][it->second[k]] = (int32_t)it->first;
        for (size_t i = 0; i < mps[s].size() && i < S; i++) usable[s][i] = mps[s][i] && !mps[s][i]->isBad();
    }
    std::vector<int32_t> match(g1.keys.size(), -1);
    int32_t nmatches = 0;
    if (!on_lane(TRACKING, "planar_search_by_bow_kf", [&](planar_ctx* ctx) {
            return planar_search_by_bow_kf(ctx, 1, &g1.n, g1.view.stride, node[0].data(), usable[0].data(), g1.keys.data(), g1.desc.data(), &g2.n, g2.view.stride, node[1].data(),
                                           usable[1].data(), g2.keys.data(), g2.desc.data(), nn_ratio, check_orientation ? 1 : 0, match.data(), &nmatches);
        })) return 0;
    vpMatches12 = std::vector<MapPointT*>(mps[0].size(), static_cast<MapPointT*>(NULL));
    for (size_t i = 0; i < mps[0].size(); i++) if (match[i] >= 0) vpMatches12[i] = mps[1][match[i]];
    return nmatches;
}

template <class KeyFrameT, class MapPointT>
int SearchBySim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12, float s12, const cv::Mat& R12, const cv::Mat& t12, float th) {
    const std::vector<MapPointT*> mps1 = pKF1->GetMapPointMatches(), mps2 = pKF2->GetMapPointMatches();
    const int N1 = (int)mps1.size(), N2 = (int)mps2.size();
    ViewGather g1 = keyframe_view(pKF1), g2 = keyframe_view(pKF2);
    g1.add_pose(pKF1->GetPose());
    g2.add_pose(pKF2->GetPose());
    const PointGather p1 = search_points(mps1), p2 = search_points(mps2);
    std::vector<int32_t> entry(g1.keys.size(), -1);                                     // NOT_IN_KF2 here: matched, index not in pKF2, which blocks i1 only (:1143)
    for (int i = 0; i < N1; i++)
        if (vpMatches12[i]) { const int idx2 = vpMatches12[i]->GetIndexInKeyFrame(pKF2); entry[i] = idx2 >= 0 && idx2 < N2 ? idx2 : NOT_IN_KF2; }
    std::vector<int32_t> match = entry;
    float R[9], t[3];
    rt_to_array(R12, t12, R, 3, t, 1);
    int32_t nFound = 0;
    if (!on_lane(TRACKING, "planar_search_by_sim3", [&](planar_ctx* ctx) {
            return planar_search_by_sim3(ctx, &g1.view, &p1.kp, pKF1->mfLogScaleFactor, pKF1->mnScaleLevels, &g2.view, &p2.kp, pKF2->mfLogScaleFactor, pKF2->mnScaleLevels, &s12, R, t,
                                         th, match.data(), &nFound);
        })) return 0;
    for (int i = 0; i < N1; i++) if (match[i] != entry[i]) vpMatches12[i] = mps2[match[i]];      // :1323
    return nFound;
}

template <class KeyFrameT, class MapPointT>
int SearchByProjectionScw(KeyFrameT* pKF, const cv::Mat& Scw, const std::vector<MapPointT*>& vpPoints, std::vector<MapPointT*>& vpMatched, int th) {
    const int M = (int)vpPoints.size();
    if (M == 0) return 0;
    ViewGather g = keyframe_view(pKF);
    g.add_blocked();                                                                    // a feature that holds a match on entry
    std::vector<uint8_t> found(M, 0);
    for (size_t i = 0; i < vpMatched.size() && i < g.blocked.size(); i++) g.blocked[i] = vpMatched[i] != NULL;
    std::set<MapPointT*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(static_cast<MapPointT*>(NULL));
    PointGather pts = search_points(vpPoints);
    pts.add_normals(vpPoints);
    for (int j = 0; j < M; j++) found[j] = spAlreadyFound.count(vpPoints[j]) ? 1 : 0;
    float S[16];
    mat_to_array(Scw, S);
    std::vector<int32_t> match(g.keys.size(), -1);
    int32_t m = M, nmatches = 0;
    if (!on_lane(TRACKING, "planar_search_by_projection_sim3", [&](planar_ctx* ctx) {
            return planar_search_by_projection_sim3(ctx, &g.view, S, pKF->mfLogScaleFactor, pKF->mnScaleLevels, &m, M, 0, pts.usable.data(), found.data(), pts.xw.data(),
                                                    pts.nrm.data(), pts.mn.data(), pts.mx.data(), pts.desc.data(), th, match.data(), &nmatches);
        })) return 0;
    for (size_t i = 0; i < vpMatched.size() && i < match.size(); i++) if (match[i] >= 0) vpMatched[i] = vpPoints[match[i]];   // :400
    return nmatches;
}

template <class KeyFrameT, class MapPointT>
int FuseScw(KeyFrameT* pKF, const cv::Mat& Scw, const std::vector<MapPointT*>& vpPoints, float th, std::vector<MapPointT*>& vpReplacePoint) {
    const int M = (int)vpPoints.size();
    if (M == 0) return 0;
    const ViewGather g = keyframe_view(pKF);
    const std::set<MapPointT*> spAlreadyFound = pKF->GetMapPoints();                     // :997
    const std::vector<MapPointT*> inKF = pKF->GetMapPointMatches();
    std::vector<uint8_t> slot(g.keys.size(), 0);
    for (size_t i = 0; i < inKF.size() && i < slot.size(); i++) slot[i] = !inKF[i] ? 0 : inKF[i]->isBad() ? 2 : 1;
    PointGather pts = search_points(vpPoints);
    pts.add_normals(vpPoints);
    for (int j = 0; j < M; j++) if (pts.usable[j] && spAlreadyFound.count(vpPoints[j])) pts.usable[j] = 0;
    float S[16];
    mat_to_array(Scw, S);
    std::vector<int32_t> idx(M, -1), owner(M, -1);
    int32_t m = M, nFused = 0;
    if (!on_lane(TRACKING, "planar_fuse_sim3", [&](planar_ctx* ctx) {
            return planar_fuse_sim3(ctx, &g.view, S, slot.data(), pKF->mfLogScaleFactor, pKF->mnScaleLevels, &m, M, 0, pts.usable.data(), pts.xw.data(), pts.nrm.data(),
                                    pts.mn.data(), pts.mx.data(), pts.desc.data(), th, idx.data(), owner.data(), &nFused);
        })) return 0;
    for (int j = 0; j < M; j++) {                                                       // :1086-1100, in the order of the points
        if (idx[j] < 0) continue;
        MapPointT* pMP = vpPoints[j];
        if (owner[j] == j) { pMP->AddObservation(pKF, idx[j]); pKF->AddMapPoint(pMP, idx[j]); }
        else if (owner[j] >= 0) vpReplacePoint[j] = vpPoints[owner[j]];
        else { MapPointT* pMPinKF = pKF->GetMapPoint(idx[j]); if (pMPinKF && !pMPinKF->isBad()) vpReplacePoint[j] = pMPinKF; }
    }
    return nFused;
}

}  // namespace planar_adapter

namespace Planar_SLAM {
inline int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12) {
    return planar_adapter::SearchByBoWKF(pKF1, pKF2, vpMatches12, mfNNratio, mbCheckOrientation);
}
inline int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12, const cv::Mat& t12, const float th) {
    return planar_adapter::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th);
}
inline int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th) {
    return planar_adapter::SearchByProjectionScw(pKF, Scw, vpPoints, vpMatched, th);
}
inline int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint) {
    return planar_adapter::FuseScw(pKF, Scw, vpPoints, th, vpReplacePoint);
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_LOOP_MATCHERS


// ---- Optimizer::OptimizeSim3: the DEFINITION of the static member with the reference's signature
//          int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2, const bool bFixScale)   src/Optimizer.cc:3739-3934
//      Enabled with PLANAR_ADAPTERS_WITH_SIM3_OPT, after the reference's Optimizer.h, KeyFrame.h, MapPoint.h and g2o's types/sim3.h; leave that body of src/Optimizer.cc out.
//      The call gathers what the function reads (mK, GetRotation() / GetTranslation(), mvKeysUn, mvScaleFactors, GetMapPointMatches(), isBad(), GetWorldPos(),
//      GetIndexInKeyFrame) with the packing of the loop matchers above, runs planar_optimize_sim3 with B = 1 on the tracking context, sets vpMatches1[i] = NULL where the
//      entry cleared the match and writes g2oS12 through g2o::Sim3::operator[].  A failing call returns 0 and changes nothing.
#if defined(PLANAR_ADAPTERS_WITH_SIM3_OPT) || defined(PLANAR_ADAPTERS_WITH_SIM3_SOLVER)
namespace planar_adapter {

struct Sim3OptSide {   // one key frame as planar_optimize_sim3 and planar_horn_ransac read it: freely copyable, a copy's views point into the copy
    ViewGather g;      // key points, [R | t], the camera of mK, the scale table over ones
    PointGather p;     // slot i = the key frame's map point i: usable, xw
    template <class KeyFrameT, class MapPointT> Sim3OptSide(KeyFrameT* pKF, const std::vector<MapPointT*>& mps) {
        g.add_keys(pKF->mvKeysUn, (int)pKF->mvKeysUn.size()).add_pose(pKF->GetRotation(), pKF->GetTranslation());
        g.add_intrinsics_K(pKF->mK).add_scales(pKF->mvScaleFactors, true);
        p.add_points(mps, (size_t)g.n, NoExclusion());
    }
};

}  // namespace planar_adapter
#endif

#ifdef PLANAR_ADAPTERS_WITH_SIM3_OPT
namespace planar_adapter {

template <class KeyFrameT, class MapPointT, class Sim3T>
int OptimizeSim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, float th2, bool bFixScale) {
    const std::vector<MapPointT*> mps1 = pKF1->GetMapPointMatches(), mps2 = pKF2->GetMapPointMatches();
    Sim3OptSide s1(pKF1, mps1), s2(pKF2, mps2);
    if (s1.g.n > PLANAR_MAX_FRAME_KEYS || s2.g.n > PLANAR_MAX_FRAME_KEYS) return 0;
    const int N = (int)vpMatches1.size() < s1.g.n ? (int)vpMatches1.size() : s1.g.n;
    std::vector<int32_t> match = sim3_entry_matches(vpMatches1, s1.g.n, (size_t)s1.g.view.stride, pKF2, s2.g.n, s2.p);      // NOT_IN_KF2: skipped (:3807)
    const std::vector<int32_t> entry = match;
    double S[8];
    for (int k = 0; k < 8; k++) S[k] = g2oS12[k];
    int32_t nIn = 0;
    if (!on_lane(TRACKING, "planar_optimize_sim3", [&](planar_ctx* ctx) {
            return planar_optimize_sim3(ctx, &s1.g.view, &s1.p.kp, &s2.g.view, &s2.p.kp, S, th2, bFixScale ? 1 : 0, match.data(), &nIn, NULL);
        })) return 0;
    for (int i = 0; i < N; i++) if (match[i] != entry[i]) vpMatches1[i] = static_cast<MapPointT*>(NULL);
    for (int k = 0; k < 8; k++) g2oS12[k] = S[k];      // untouched on the early return: the entry leaves S as it was
    return nIn;
}

}  // namespace planar_adapter

namespace Planar_SLAM {
inline int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2, const bool bFixScale) {
    return planar_adapter::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_SIM3_OPT

// ---- Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc): the class LoopClosing::ComputeSim3 constructs per candidate (src/LoopClosing.cc:274-301), with the
//      reference's signatures.  Enabled with PLANAR_ADAPTERS_WITH_SIM3_SOLVER, after the reference's KeyFrame.h and MapPoint.h and INSTEAD of its Sim3Solver.h; leave
//      src/Sim3Solver.cc out.  The constructor gathers what Optimizer::OptimizeSim3's adapter gathers (mK, GetRotation() / GetTranslation(), mvKeysUn, mvScaleFactors,
//      GetMapPointMatches(), isBad(), GetWorldPos(), GetIndexInKeyFrame); iterate() runs planar_horn_ransac with B = 1 on the tracking context and carries the state
//      (mnIterations, mnBestInliers, the best R, t, s) in the object.  The draws come from this solver's own glibc stream, srand(seed) with the seed of SetSeed (0 unless
//      set): the reference's solvers share the process's rand().  A failing call returns an empty matrix with bNoMore set.
#ifdef PLANAR_ADAPTERS_WITH_SIM3_SOLVER
namespace Planar_SLAM {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true)
        : mN1((int)vpMatched12.size()), mSide1(pKF1, pKF1->GetMapPointMatches()), mSide2(pKF2, pKF2->GetMapPointMatches()), mnIterations(0), mnBestInliers(0), mBestScale(0.f),
          mbFixScale(bFixScale), mSeed(0) {
        mvMatch = planar_adapter::sim3_entry_matches(vpMatched12, mSide1.g.n, (size_t)mSide1.g.view.stride, pKF2, mSide2.g.n, mSide2.p);      // NOT_IN_KF2: skipped (:82)
        for (int k = 0; k < 9; k++) mBestR[k] = 0.f;
        for (int k = 0; k < 3; k++) mBestt[k] = 0.f;
        SetRansacParameters();
    }
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability; mRansacMinInliers = minInliers; mRansacMaxIts = maxIterations;
        mnIterations = 0;
    }
    void SetSeed(unsigned seed) { mSeed = seed; }
    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }
    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        using namespace planar_adapter;
        Sim3OptSide &s1 = mSide1, &s2 = mSide2;
        bNoMore = true;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (s1.g.n > PLANAR_MAX_FRAME_KEYS || s2.g.n > PLANAR_MAX_FRAME_KEYS) return cv::Mat();
        int32_t found = 0, no_more = 1, n_inl = 0;
        std::vector<uint8_t> inl((size_t)s1.g.view.stride, 0);
        float R[9], t[3], s = 0.f;
        if (!on_lane(TRACKING, "planar_horn_ransac", [&](planar_ctx* ctx) {
                return planar_horn_ransac(ctx, &s1.g.view, &s1.p.kp, &s2.g.view, &s2.p.kp, mvMatch.data(), mRansacProb, mRansacMinInliers, mRansacMaxIts, mbFixScale ? 1 : 0,
                                          nIterations, &mSeed, &mnIterations, &mnBestInliers, mBestR, mBestt, &mBestScale, &found, &no_more, &n_inl, inl.data(), R, t, &s,
                                          NULL, NULL);
            })) return cv::Mat();
        bNoMore = no_more != 0;
        if (!found) return cv::Mat();
        nInliers = n_inl;
        for (int i = 0; i < mN1 && i < s1.g.n; i++) vbInliers[i] = inl[i] != 0;
        const float T[16] = {R[0] * s, R[1] * s, R[2] * s, t[0], R[3] * s, R[4] * s, R[5] * s, t[1], R[6] * s, R[7] * s, R[8] * s, t[2], 0.f, 0.f, 0.f, 1.f};
        return array_to_mat(T);                                                             // mBestT12: [s R | t]
    }
    cv::Mat GetEstimatedRotation() { return mnIterations <= 0 ? cv::Mat() : planar_adapter::array_to_mat(mBestR, 3, 3); }   // empty until an iteration has run
    cv::Mat GetEstimatedTranslation() { return mnIterations <= 0 ? cv::Mat() : planar_adapter::array_to_mat(mBestt, 3, 1); }
    float GetEstimatedScale() { return mBestScale; }

protected:
    int mN1;
    planar_adapter::Sim3OptSide mSide1, mSide2;                                              // (by value: a copied solver's views point into its own sides)
    std::vector<int32_t> mvMatch;
    int32_t mnIterations, mnBestInliers;
    float mBestR[9], mBestt[3], mBestScale;
    bool mbFixScale;
    uint32_t mSeed;
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
};

}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_SIM3_SOLVER

// ---- PnPsolver (reference include/PnPsolver.h, src/PnPsolver.cc): the class Tracking::Relocalization constructs per candidate key frame (src/Tracking.cc:2590-2625),
//      with the reference's signatures.  Enabled with PLANAR_ADAPTERS_WITH_PNP_SOLVER, after the reference's Frame.h and MapPoint.h and INSTEAD of its PnPsolver.h; leave
//      src/PnPsolver.cc out.  The constructor gathers what the reference's does (F.mvKeysUn, F.mvScaleFactors, whose squares are mvLevelSigma2, F.fx fy cx cy, isBad(),
//      GetWorldPos()): key point i is matched to "feature" i of a candidate that holds vpMapPointMatches[i].  iterate() runs planar_pnp_ransac with B = 1 on the tracking
//      context and carries the state (mnIterations, mnBestInliers, mvbBestInliers, mBestTcw) in the object.  SetRansacParameters evaluates the reference's chain for
//      mRansacMinInliers and mRansacMaxIts (:129-152), the same libm doubles as the library's table, because find() is iterate(mRansacMaxIts).  The draws come from this
//      solver's own glibc stream, srand(seed) with the seed of SetSeed (0 unless set): the reference's solvers share the process's rand().  A failing call returns an
//      empty matrix with bNoMore set.
#ifdef PLANAR_ADAPTERS_WITH_PNP_SOLVER
namespace Planar_SLAM {

class PnPsolver {
public:
    PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches) : mnIterations(0), mnBestInliers(0), N(0), mSeed(0) {
        mnMatches = vpMapPointMatches.size();
        const int mn = (int)(mnMatches < F.mvKeysUn.size() ? mnMatches : F.mvKeysUn.size());
        mView.add_keys(F.mvKeysUn, mn).add_intrinsics(F).add_scales(F.mvScaleFactors, true);
        mPoints.add_points(vpMapPointMatches, (size_t)mn, planar_adapter::NoExclusion());
        mvMatch.assign((size_t)mView.view.stride, -1); mvbBestInliers.assign((size_t)mView.view.stride, 0);
        for (int i = 0; i < mn; i++) {                                                      // a bad point is matched (match = i) but not usable
            if (vpMapPointMatches[i]) mvMatch[i] = i;
            N += mPoints.usable[i];
        }
        for (int k = 0; k < 16; k++) mBestTcw[k] = 0.f;
        SetRansacParameters();
    }
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991) {
        mRansacProb = probability; mRansacMinSet = minSet; mRansacEpsilon = epsilon; mRansacTh = th2;
        mMinInliersGiven = minInliers; mMaxItsGiven = maxIterations;
        int nMinInliers = N * epsilon;
        if (nMinInliers < minInliers) nMinInliers = minInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        if (epsilon < (float)mRansacMinInliers / N) epsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N) nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
            nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);   // what x86-64's conversion gives where the double is no int
        }
        const int m = nIterations < maxIterations ? nIterations : maxIterations;
        mRansacMaxIts = m > 1 ? m : 1;
    }
    void SetSeed(unsigned seed) { mSeed = seed; }
    cv::Mat find(std::vector<bool>& vbInliers, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }
    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        using namespace planar_adapter;
        bNoMore = true;
        vbInliers.clear();
        nInliers = 0;
        const int mn = mView.n;
        if (mn > PLANAR_MAX_FRAME_KEYS) return cv::Mat();
        int32_t found = 0, no_more = 1, n_inl = 0;
        std::vector<uint8_t> inl((size_t)mView.view.stride, 0);
        float T[16];
        if (!on_lane(TRACKING, "planar_pnp_ransac", [&](planar_ctx* ctx) {
                return planar_pnp_ransac(ctx, &mView.view, mPoints.usable.data(), mPoints.xw.data(), mView.view.stride, mvMatch.data(), mRansacProb, mMinInliersGiven,
                                         mMaxItsGiven, mRansacMinSet, mRansacEpsilon, mRansacTh, nIterations, &mSeed, &mnIterations, &mnBestInliers, mvbBestInliers.data(),
                                         mBestTcw, &found, &no_more, &n_inl, inl.data(), T);
            })) return cv::Mat();
        bNoMore = no_more != 0;
        if (!found) return cv::Mat();
        nInliers = n_inl;
        vbInliers = std::vector<bool>(mnMatches, false);
        for (int i = 0; i < mn; i++) vbInliers[i] = inl[i] != 0;
        return array_to_mat(T);
    }

protected:
    size_t mnMatches;
    planar_adapter::ViewGather mView;                                                      // key points (mView.n of them), fx fy cx cy, the scale table over ones
    planar_adapter::PointGather mPoints;                                                   // slot i = vpMapPointMatches[i]: usable, xw
    std::vector<uint8_t> mvbBestInliers;
    std::vector<int32_t> mvMatch;
    int32_t mnIterations, mnBestInliers;
    float mBestTcw[16];
    int N;
    uint32_t mSeed;
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts, mRansacMinSet, mMinInliersGiven, mMaxItsGiven;
    float mRansacEpsilon, mRansacTh;
};

}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_PNP_SOLVER


// ---- Optimizer::OptimizeEssentialGraph: the DEFINITION of the static member with the reference's signature
//          void OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
//                                      const LoopClosing::KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections,
//                                      const bool& bFixScale)                                                                       src/Optimizer.cc:2680-2991
//      Enabled with PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH, after the reference's Optimizer.h, LoopClosing.h, Map.h, KeyFrame.h, MapPoint.h, MapLine.h and MapPlane.h;
//      leave that body of src/Optimizer.cc out.  The key frames of Map::GetAllKeyFrames() are numbered by the rank of their mnId; essential_graph_edges applies the
//      reference's selection rules to plain arrays (so they can be tested without a KeyFrame); planar_optimize_essential_graph runs with B = 1 on the tracking
//      context; SetPose, then SetWorldPos of points, lines and planes follow in the reference's order with its UpdateNormalAndDepth /
//      ComputeDistinctiveDescriptors / UpdateAverageDir / UpdateCoefficientsAndPoints calls.  A failing call, or a map of more than PLANAR_ESSGRAPH_MAX_KF key
//      frames, changes nothing.  Precondition (the reference's own): no bad key frame in GetAllKeyFrames().
#ifdef PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH
#include <algorithm>
#include <set>
namespace planar_adapter {

// A list per key frame: item k of key frame i is idx[off[i] + k] (and weight[off[i] + k] where the list has weights); off has n + 1 entries.
struct EssGraphLists { const int32_t* off; const int32_t* idx; const int32_t* weight; };

// The edge list of OptimizeEssentialGraph over key frames 0 .. n - 1 in mnId order -> (vertex 0, vertex 1, kind) triples in the reference's order of insertion.
//   parent[i]: index of GetParent() or -1.            loop_edges: GetLoopEdges() of i (no weights).
//   covisible: GetVectorCovisibleKeyFrames() of i in its order, with GetWeight(); the function applies minFeat = 100 as GetCovisiblesByWeight(minFeat) does.
//   loop_connections: LoopConnections[i] with pKF->GetWeight(connection) as weight; a key frame without an entry has an empty list.
// std::set<KeyFrame*> iterates in pointer order, which no array can carry: lists are taken in the order given.  That order only decides the order of the sums.
inline std::vector<int32_t> essential_graph_edges(int n, const int32_t* parent, const EssGraphLists& loop_edges, const EssGraphLists& covisible,
                                                  const EssGraphLists& loop_connections, int cur, int loop) {
    const int minFeat = 100;                                                                                   // :2707
    std::vector<int32_t> e;
    std::set<std::pair<int, int> > inserted;                                                                   // sInsertedEdges
    auto add = [&](int v0, int v1, int kind) { e.push_back(v0); e.push_back(v1); e.push_back(kind); };
    for (int i = 0; i < n; i++)                                                                                // loop connections (:2748-2774)
        for (int k = loop_connections.off[i]; k < loop_connections.off[i + 1]; k++) {
            const int j = loop_connections.idx[k];
            if ((i != cur || j != loop) && loop_connections.weight[k] < minFeat) continue;                     // the (current, loop) exemption (:2757)
            add(i, j, PLANAR_ESSGRAPH_LOOP);
            inserted.insert(std::make_pair(std::min(i, j), std::max(i, j)));
        }
    for (int i = 0; i < n; i++) {                                                                              // normal edges (:2777-2866)
        if (parent[i] >= 0) add(i, parent[i], PLANAR_ESSGRAPH_NORMAL);                                         // spanning tree (:2792-2813): no exclusion applies
        auto is_loop_edge = [&](int j) { for (int k = loop_edges.off[i]; k < loop_edges.off[i + 1]; k++) if (loop_edges.idx[k] == j) return true; return false; };
        for (int k = loop_edges.off[i]; k < loop_edges.off[i + 1]; k++)                                        // old loop edges towards lower ids (:2816-2836)
            if (loop_edges.idx[k] < i) add(i, loop_edges.idx[k], PLANAR_ESSGRAPH_NORMAL);
        for (int k = covisible.off[i]; k < covisible.off[i + 1]; k++) {                                        // covisibility (:2839-2865)
            const int j = covisible.idx[k];
            if (covisible.weight[k] < minFeat) continue;                                                       // GetCovisiblesByWeight(minFeat)
            if (j == parent[i] || parent[j] == i || is_loop_edge(j)) continue;                                 // != pParentKF, !hasChild, !sLoopEdges.count (:2841)
            if (!(j < i)) continue;                                                                            // mnId ordering (:2842)
            if (inserted.count(std::make_pair(std::min(i, j), std::max(i, j)))) continue;                      // :2843
            add(i, j, PLANAR_ESSGRAPH_NORMAL);
        }
    }
    return e;
}

template <class MapT, class KeyFrameT, class PoseMapT, class ConnMapT>
void OptimizeEssentialGraph(MapT* pMap, KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const PoseMapT& NonCorrectedSim3, const PoseMapT& CorrectedSim3,
                            const ConnMapT& LoopConnections, bool bFixScale) {
    std::vector<KeyFrameT*> vpKFs = pMap->GetAllKeyFrames();
    const auto vpMPs = pMap->GetAllMapPoints();
    const auto vpMLs = pMap->GetAllMapLines();
    const auto vpMPLs = pMap->GetAllMapPlanes();
    const int n = (int)vpKFs.size();
    if (n < 1 || n > PLANAR_ESSGRAPH_MAX_KF) { std::fprintf(stderr, "planar (OptimizeEssentialGraph): %d key frames, 1 .. %d supported - nothing optimised\n", n, PLANAR_ESSGRAPH_MAX_KF); return; }
    std::vector<KeyFrameT*> order = vpKFs;
    std::sort(order.begin(), order.end(), [](KeyFrameT* a, KeyFrameT* b) { return a->mnId < b->mnId; });
    std::map<KeyFrameT*, int> index;
    std::map<unsigned long, int> index_of_id;
    for (int i = 0; i < n; i++) { index[order[i]] = i; index_of_id[order[i]->mnId] = i; }
    auto at = [&](KeyFrameT* k) { auto it = index.find(k); return it == index.end() ? -1 : it->second; };
    if (at(pLoopKF) < 0 || at(pCurKF) < 0) return;
    std::vector<float> poses(16 * (size_t)n);
    std::vector<double> corr(8 * (size_t)n, 0.0), nc(8 * (size_t)n, 0.0);
    std::vector<uint8_t> cm(n, 0), nm(n, 0);
    std::vector<int32_t> parent(n, -1), le_off(1, 0), le_idx, cv_off(1, 0), cv_idx, cv_w, lc_off(1, 0), lc_idx, lc_w;
    for (int i = 0; i < n; i++) {
        KeyFrameT* pKF = order[i];
        mat_to_array(pKF->GetPose(), &poses[16 * (size_t)i]);
        auto ic = CorrectedSim3.find(pKF);
        if (ic != CorrectedSim3.end()) { cm[i] = 1; for (int k = 0; k < 8; k++) corr[8 * (size_t)i + k] = ic->second[k]; }
        auto in = NonCorrectedSim3.find(pKF);
        if (in != NonCorrectedSim3.end()) { nm[i] = 1; for (int k = 0; k < 8; k++) nc[8 * (size_t)i + k] = in->second[k]; }
        KeyFrameT* par = pKF->GetParent();
        parent[i] = par ? at(par) : -1;
        for (KeyFrameT* l : pKF->GetLoopEdges()) if (at(l) >= 0) le_idx.push_back(at(l));
        le_off.push_back((int32_t)le_idx.size());
        for (KeyFrameT* c : pKF->GetCovisiblesByWeight(100)) if (c && at(c) >= 0 && !c->isBad()) { cv_idx.push_back(at(c)); cv_w.push_back(100); }   // the list is already cut at minFeat
        cv_off.push_back((int32_t)cv_idx.size());
        auto il = LoopConnections.find(pKF);
        if (il != LoopConnections.end()) for (KeyFrameT* c : il->second) if (at(c) >= 0) { lc_idx.push_back(at(c)); lc_w.push_back(pKF->GetWeight(c)); }
        lc_off.push_back((int32_t)lc_idx.size());
    }
    const int cur = at(pCurKF), loop = at(pLoopKF);
    std::vector<int32_t> edges = essential_graph_edges(n, parent.data(), EssGraphLists{le_off.data(), le_idx.data(), NULL}, EssGraphLists{cv_off.data(), cv_idx.data(), cv_w.data()},
                                                       EssGraphLists{lc_off.data(), lc_idx.data(), lc_w.data()}, cur, loop);
    // landmarks that are not bad, with the reference key frame of :2897-2903
    auto ref_of = [&](unsigned long by, unsigned long ref, KeyFrameT* rk) {
        const unsigned long id = by == pCurKF->mnId ? ref : rk->mnId;
        auto it = index_of_id.find(id);
        return it == index_of_id.end() ? -1 : it->second;
    };
    std::vector<float> pts, pls; std::vector<double> lns; std::vector<int32_t> pt_ref, ln_ref, pl_ref;
    std::vector<size_t> pt_of, ln_of, pl_of;
    bool refs_ok = true;
    for (size_t i = 0; i < vpMPs.size(); i++) {
        auto* p = vpMPs[i];
        if (p->isBad()) continue;
        const int r = ref_of(p->mnCorrectedByKF, p->mnCorrectedReference, p->mnCorrectedByKF == pCurKF->mnId ? (KeyFrameT*)NULL : p->GetReferenceKeyFrame());
        refs_ok = refs_ok && r >= 0;
        const cv::Mat P = p->GetWorldPos();
        for (int k = 0; k < 3; k++) pts.push_back(P.at<float>(k));
        pt_ref.push_back(r); pt_of.push_back(i);
    }
    for (size_t i = 0; i < vpMLs.size(); i++) {
        auto* p = vpMLs[i];
        if (p->isBad()) continue;
        const int r = ref_of(p->mnCorrectedByKF, p->mnCorrectedReference, p->mnCorrectedByKF == pCurKF->mnId ? (KeyFrameT*)NULL : p->GetReferenceKeyFrame());
        refs_ok = refs_ok && r >= 0;
        const auto P = p->GetWorldPos();
        for (int k = 0; k < 6; k++) lns.push_back(P(k));
        ln_ref.push_back(r); ln_of.push_back(i);
    }
    for (size_t i = 0; i < vpMPLs.size(); i++) {
        auto* p = vpMPLs[i];
        if (p->isBad()) continue;
        const int r = ref_of(p->mnCorrectedByKF, p->mnCorrectedReference, p->mnCorrectedByKF == pCurKF->mnId ? (KeyFrameT*)NULL : p->GetReferenceKeyFrame());
        refs_ok = refs_ok && r >= 0;
        const cv::Mat P = p->GetWorldPos();
        for (int k = 0; k < 4; k++) pls.push_back(P.at<float>(k));
        pl_ref.push_back(r); pl_of.push_back(i);
    }
    if (!refs_ok) { std::fprintf(stderr, "planar (OptimizeEssentialGraph): a landmark's reference key frame is not in the map - nothing optimised\n"); return; }
    const int32_t n_kf = n, n_e = (int32_t)(edges.size() / 3), n_pt = (int32_t)pt_ref.size(), n_ln = (int32_t)ln_ref.size(), n_pl = (int32_t)pl_ref.size();
    if (edges.empty()) edges.resize(3, 0);
    planar_essgraph g;
    std::memset(&g, 0, sizeof g);
    g.B = 1; g.kf_stride = n; g.edge_stride = n_e > 0 ? n_e : 1; g.point_stride = n_pt; g.line_stride = n_ln; g.plane_stride = n_pl;
    g.n_kf = &n_kf; g.poses = poses.data(); g.corrected = corr.data(); g.corrected_mask = cm.data(); g.noncorrected = nc.data(); g.noncorrected_mask = nm.data();
    g.fixed = &loop; g.n_edges = &n_e; g.edges = edges.data();
    if (n_pt) { g.n_points = &n_pt; g.points = pts.data(); g.point_ref = pt_ref.data(); }
    if (n_ln) { g.n_lines = &n_ln; g.lines = lns.data(); g.line_ref = ln_ref.data(); }
    if (n_pl) { g.n_planes = &n_pl; g.planes = pls.data(); g.plane_ref = pl_ref.data(); }
    std::vector<double> sim3(8 * (size_t)n), lns_out(lns.size());
    std::vector<float> poses_out(16 * (size_t)n), pts_out(pts.size()), pls_out(pls.size());
    double info[5];
    if (!on_lane(TRACKING, "planar_optimize_essential_graph", [&](planar_ctx* ctx) {
            return planar_optimize_essential_graph(ctx, &g, bFixScale ? 1 : 0, 20, sim3.data(), poses_out.data(), n_pt ? pts_out.data() : NULL, n_ln ? lns_out.data() : NULL,
                                                   n_pl ? pls_out.data() : NULL, info);
        })) return;
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (KeyFrameT* pKFi : vpKFs) pKFi->SetPose(array_to_mat(&poses_out[16 * (size_t)index[pKFi]]));
    for (size_t k = 0; k < pt_of.size(); k++) { auto* p = vpMPs[pt_of[k]]; p->SetWorldPos(array_to_mat(&pts_out[3 * k], 3, 1)); p->UpdateNormalAndDepth(); }
    for (size_t k = 0; k < ln_of.size(); k++) {
        auto* p = vpMLs[ln_of[k]];
        auto P = p->GetWorldPos();
        for (int c = 0; c < 6; c++) P(c) = lns_out[6 * k + c];
        p->SetWorldPos(P); p->ComputeDistinctiveDescriptors(); p->UpdateAverageDir();
    }
    for (size_t k = 0; k < pl_of.size(); k++) { auto* p = vpMPLs[pl_of[k]]; p->SetWorldPos(array_to_mat(&pls_out[4 * k], 4, 1)); p->UpdateCoefficientsAndPoints(); }
}

}  // namespace planar_adapter

namespace Planar_SLAM {
inline void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                              const LoopClosing::KeyFrameAndPose& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections,
                                              const bool& bFixScale) {
    planar_adapter::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale);
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_ESSENTIAL_GRAPH


// ---- Optimizer::BundleAdjustment / Optimizer::GlobalBundleAdjustemnt (src/Optimizer.cc:35-548, called from LoopClosing::RunGlobalBundleAdjustment,
//      src/LoopClosing.cc:650): DEFINITIONS with the reference's signatures.  The map becomes a planar_ba_problem, planar_global_ba solves it, the values go back as
//      :451-547 put them back.  Enabled with PLANAR_ADAPTERS_WITH_GLOBAL_BA, after the reference's Optimizer.h, Map.h, KeyFrame.h, MapPoint.h, MapLine.h, MapPlane.h and
//      Config.h; leave those two bodies of src/Optimizer.cc out.
//      What is gathered: the key frames that are not bad, by ascending mnId (mnId 0 fixed); maxKFid over them; every map point, line and plane that is not bad; of
//      their observations (for a plane its three maps: plane, vertical, parallel) those whose key frame is not bad and has mnId <= maxKFid.  (An observing key frame
//      that passes both tests but is not in vpKFs has no vertex in the reference, which then dereferences a null pointer; here the observation is skipped.)  A line
//      observation reads the OBSERVING key frame's mvKeyLineFunctions (:232).  A landmark left without an observation is the reference's vbNotIncluded*: untouched.
//      Write-back: nLoopKF == 0: SetPose / SetWorldPos with UpdateNormalAndDepth / UpdateAverageDir / UpdateCoefficientsAndPoints, in the reference's order (key frames,
//      points, lines, planes); otherwise mTcwGBA / mPosGBA (float, as Converter::toCvMat leaves them) and mnBAGlobalForKF = nLoopKF.  Intrinsics are the first key
//      frame's (the reference copies each key frame's own into its edges; one camera per map is what the library takes).  A failing call, or a map of more than
//      PLANAR_GBA_MAX_KF key frames, writes a message to stderr and changes nothing.
#ifdef PLANAR_ADAPTERS_WITH_GLOBAL_BA
#include <algorithm>
namespace Planar_SLAM {
inline void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, const std::vector<MapLine*>& vpML,
                                        const std::vector<MapPlane*>& vpMPL, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
    std::vector<KeyFrame*> kfs;
    for (KeyFrame* k : vpKFs) if (k && !k->isBad()) kfs.push_back(k);
    std::sort(kfs.begin(), kfs.end(), [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; });
    const int K = (int)kfs.size();
    if (K < 1) return;
    if (K > PLANAR_GBA_MAX_KF) { std::fprintf(stderr, "planar (BundleAdjustment): %d key frames, 1 .. %d supported - nothing optimised\n", K, PLANAR_GBA_MAX_KF); return; }
    std::map<KeyFrame*, int> kf_index;
    std::vector<float> kf_Tcw((size_t)K * 16);
    std::vector<uint8_t> kf_fixed(K);
    unsigned long maxKFid = 0;
    for (int k = 0; k < K; k++) {
        kf_index[kfs[k]] = k;
        planar_adapter::mat_to_array(kfs[k]->GetPose(), &kf_Tcw[(size_t)k * 16]);
        kf_fixed[k] = kfs[k]->mnId == 0;
        if (kfs[k]->mnId > maxKFid) maxKFid = kfs[k]->mnId;
    }
    std::vector<uint8_t> lm_type, e_type;
    std::vector<double> lm_init, e_meas;
    std::vector<int32_t> e_kf, e_lm;
    std::vector<float> e_is2;
    auto add_lm = [&](int type, double a, double b, double c, double d) { lm_type.push_back((uint8_t)type); lm_init.insert(lm_init.end(), {a, b, c, d}); return (int32_t)lm_type.size() - 1; };
    auto add_edge = [&](int kf, int lm, int type, double m0, double m1, double m2, double m3, float is2) {
        e_kf.push_back(kf); e_lm.push_back(lm); e_type.push_back((uint8_t)type); e_meas.insert(e_meas.end(), {m0, m1, m2, m3}); e_is2.push_back(is2);
    };
    // the vertex of an observing key frame, or -1 where the observation is filtered (:116, :227, :317, :346, :372)
    auto observer = [&](KeyFrame* k) { if (k->isBad() || k->mnId > maxKFid) return -1; auto it = kf_index.find(k); return it == kf_index.end() ? -1 : it->second; };
    std::vector<int32_t> pt_lm(vpMP.size(), -1), ln_lm(vpML.size(), -1), pl_lm(vpMPL.size(), -1);
    for (size_t i = 0; i < vpMP.size(); i++) {
        MapPoint* p = vpMP[i];
        if (!p || p->isBad()) continue;
        cv::Mat X = p->GetWorldPos();
        pt_lm[i] = add_lm(0, X.at<float>(0), X.at<float>(1), X.at<float>(2), 0);
        const std::map<KeyFrame*, size_t> obs = p->GetObservations();
        for (const auto& o : obs) {
            const int v = observer(o.first);
            if (v < 0) continue;
            KeyFrame* k = o.first;
            const cv::KeyPoint& kp = k->mvKeysUn[o.second];
            const float ur = k->mvuRight[o.second], is2 = k->mvInvLevelSigma2[kp.octave];
            if (ur < 0) add_edge(v, pt_lm[i], PLANAR_BA_MONO, kp.pt.x, kp.pt.y, 0, 0, is2);
            else add_edge(v, pt_lm[i], PLANAR_BA_STEREO, kp.pt.x, kp.pt.y, ur, 0, is2);
        }
    }
    for (size_t i = 0; i < vpML.size(); i++) {
        MapLine* p = vpML[i];
        if (!p || p->isBad()) continue;
        const auto W = p->GetWorldPos();                       // Vector6d: start xyz, end xyz
        ln_lm[i] = add_lm(0, W[0], W[1], W[2], 0);
        add_lm(0, W[3], W[4], W[5], 0);
        const std::map<KeyFrame*, size_t> obs = p->GetObservations();
        for (const auto& o : obs) {
            const int v = observer(o.first);
            if (v < 0) continue;
            const auto f = o.first->mvKeyLineFunctions[o.second];     // the observer's own line function, both end points on the observer's vertex
            add_edge(v, ln_lm[i], PLANAR_BA_LINE, f[0], f[1], f[2], 0, 1.f);
            add_edge(v, ln_lm[i] + 1, PLANAR_BA_LINE, f[0], f[1], f[2], 0, 1.f);
        }
    }
    for (size_t i = 0; i < vpMPL.size(); i++) {
        MapPlane* p = vpMPL[i];
        if (!p || p->isBad()) continue;
        cv::Mat C = p->GetWorldPos();
        pl_lm[i] = add_lm(1, C.at<float>(0), C.at<float>(1), C.at<float>(2), C.at<float>(3));
        auto plane_edges = [&](const std::map<KeyFrame*, size_t>& obs, int type) {
            for (const auto& o : obs) {
                const int v = observer(o.first);
                if (v < 0) continue;
                const cv::Mat& m = o.first->mvPlaneCoefficients[o.second];
                add_edge(v, pl_lm[i], type, m.at<float>(0), m.at<float>(1), m.at<float>(2), m.at<float>(3), 1.f);
            }
        };
        plane_edges(p->GetObservations(), PLANAR_BA_PLANE);
        plane_edges(p->GetVerObservations(), PLANAR_BA_VERTICAL);
        plane_edges(p->GetParObservations(), PLANAR_BA_PARALLEL);
    }
    const int NL = (int)lm_type.size(), NE = (int)e_type.size();
    std::vector<float> out_T((size_t)K * 16);
    std::vector<double> out_lm((size_t)std::max(NL, 1) * 4);
    std::vector<uint8_t> out_inc(std::max(NL, 1));
    planar_ba_problem P{K, kf_Tcw.data(), kf_fixed.data(), NL, lm_type.data(), lm_init.data(), NE, e_kf.data(), e_lm.data(), e_type.data(), e_meas.data(), e_is2.data()};
    planar_gba_result R{out_T.data(), out_lm.data(), out_inc.data(), 0, 0, 0, 0, 0.0, 0.0};
    const planar_pose_params prm = planar_adapter::plane_pose_params<Config>(kfs[0]->fx, kfs[0]->fy, kfs[0]->cx, kfs[0]->cy, kfs[0]->mbf);
    static_assert(sizeof(bool) == 1, "bool* pbStopFlag is passed as a byte flag");
    if (!planar_adapter::on_lane(planar_adapter::TRACKING, "planar_global_ba", [&](planar_ctx* ctx) {
            return planar_global_ba(ctx, &P, &prm, nIterations, bRobust ? 1 : 0, &R, reinterpret_cast<const volatile unsigned char*>(pbStopFlag));
        })) return;
    // Recover optimized data (:451-547)
    for (int k = 0; k < K; k++) {
        const cv::Mat T = planar_adapter::array_to_mat(&out_T[(size_t)k * 16]);
        if (nLoopKF == 0) kfs[k]->SetPose(T);
        else { kfs[k]->mTcwGBA.create(4, 4, CV_32F); T.copyTo(kfs[k]->mTcwGBA); kfs[k]->mnBAGlobalForKF = nLoopKF; }
    }
    for (size_t i = 0; i < vpMP.size(); i++) {
        if (pt_lm[i] < 0 || !out_inc[pt_lm[i]]) continue;
        float x[3];
        for (int j = 0; j < 3; j++) x[j] = (float)out_lm[(size_t)pt_lm[i] * 4 + j];
        const cv::Mat X = planar_adapter::array_to_mat(x, 3, 1);
        if (nLoopKF == 0) { vpMP[i]->SetWorldPos(X); vpMP[i]->UpdateNormalAndDepth(); }
        else { vpMP[i]->mPosGBA.create(3, 1, CV_32F); X.copyTo(vpMP[i]->mPosGBA); vpMP[i]->mnBAGlobalForKF = nLoopKF; }
    }
    for (size_t i = 0; i < vpML.size(); i++) {
        if (ln_lm[i] < 0 || !out_inc[ln_lm[i]]) continue;
        const double* s = &out_lm[(size_t)ln_lm[i] * 4];
        const double* e = &out_lm[(size_t)(ln_lm[i] + 1) * 4];
        if (nLoopKF == 0) {
            auto W = vpML[i]->GetWorldPos();
            for (int j = 0; j < 3; j++) { W[j] = s[j]; W[3 + j] = e[j]; }                 // linePos << vStartPoint->estimate(), vEndPoint->estimate(): doubles
            vpML[i]->SetWorldPos(W); vpML[i]->UpdateAverageDir();
        } else {
            const float x[6] = {(float)s[0], (float)s[1], (float)s[2], (float)e[0], (float)e[1], (float)e[2]};
            vpML[i]->mPosGBA.create(6, 1, CV_32F); planar_adapter::array_to_mat(x, 6, 1).copyTo(vpML[i]->mPosGBA); vpML[i]->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (size_t i = 0; i < vpMPL.size(); i++) {
        if (pl_lm[i] < 0 || !out_inc[pl_lm[i]]) continue;
        float c[4];
        for (int j = 0; j < 4; j++) c[j] = (float)out_lm[(size_t)pl_lm[i] * 4 + j];
        const cv::Mat C = planar_adapter::array_to_mat(c, 4, 1);
        if (nLoopKF == 0) { vpMPL[i]->SetWorldPos(C); vpMPL[i]->UpdateCoefficientsAndPoints(); }
        else { vpMPL[i]->mPosGBA.create(4, 1, CV_32F); C.copyTo(vpMPL[i]->mPosGBA); vpMPL[i]->mnBAGlobalForKF = nLoopKF; }
    }
}
inline void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
    BundleAdjustment(pMap->GetAllKeyFrames(), pMap->GetAllMapPoints(), pMap->GetAllMapLines(), pMap->GetAllMapPlanes(), nIterations, pbStopFlag, nLoopKF, bRobust);
}
}  // namespace Planar_SLAM
#endif   // PLANAR_ADAPTERS_WITH_GLOBAL_BA
