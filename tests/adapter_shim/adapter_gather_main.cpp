// tests/adapter_shim/adapter_gather_main.cpp — TEST INFRASTRUCTURE.  The two shared gathers of include/planar_adapters.hpp (planar_adapter::ViewGather and
// PointGather) run part by part on stand-in Frame / KeyFrame / MapPoint objects built from known arrays; every field of the resulting views is compared with the
// arrays it came from.  No device call is made and libplanar_hip.so is not linked: an unused inline function is not emitted.  Exit status 0 = all equal; the
// first difference prints its line and exits 1.
//   adapter_gather
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvshim.hpp"
#include "planar_adapters.hpp"

using planar_adapter::PointGather;
using planar_adapter::ViewGather;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "adapter_gather_main.cpp:%d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {
struct KeyFrame;
struct MapPoint {
    cv::Mat pos, normal, desc;
    bool bad = false, in_kf = false;
    int obs = 0;
    float mn = 0, mx = 0;
    bool isBad() { return bad; }
    cv::Mat GetWorldPos() { return pos.clone(); }
    cv::Mat GetNormal() { return normal.clone(); }
    cv::Mat GetDescriptor() { return desc.clone(); }
    void GetDistanceRange(float& a, float& b) { a = mn; b = mx; }
    int Observations() { return obs; }
    bool IsInKeyFrame(KeyFrame*) { return in_kf; }
};
struct Frame {      // bounds, grid constants and camera are statics, as in the reference's Frame
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvScaleFactors;
    cv::Mat mDescriptors, mTcw;
    std::vector<MapPoint*> mvpMapPoints;
    float mbf = 40.f, mb = 0.08f;
    static float fx, fy, cx, cy, mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
};
float Frame::fx = 535.4f, Frame::fy = 539.2f, Frame::cx = 320.1f, Frame::cy = 247.6f, Frame::mnMinX = -3.f, Frame::mnMaxX = 643.f, Frame::mnMinY = -2.f, Frame::mnMaxY = 481.f,
      Frame::mfGridElementWidthInv = 0.1f, Frame::mfGridElementHeightInv = 0.0625f;
struct KeyFrame {   // the same members per object, the pose behind accessors
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvScaleFactors;
    cv::Mat mDescriptors, Tcw, mK;
    float fx = 517.3f, fy = 516.5f, cx = 318.6f, cy = 255.3f, mbf = 41.f, mb = 0.09f, mnMinX = 1.f, mnMaxX = 639.f, mnMinY = 2.f, mnMaxY = 478.f, mfGridElementWidthInv = 0.2f,
          mfGridElementHeightInv = 0.125f;
    cv::Mat GetPose() { return Tcw.clone(); }
    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
};

cv::KeyPoint key(int i) { return cv::KeyPoint(10.5f + i, 20.25f + 2 * i, 31.f, 45.f * i, 7.f + i, i % 4, i); }
uint8_t desc_byte(int i, int j) { return (uint8_t)(1 + 37 * i + j); }
float pose_value(int k) { return 0.5f + 0.25f * k; }
template <class T> void fill(T& o, int n, bool with_u_right, int n_levels) {
    o.N = n;
    o.mvKeysUn.resize(n); o.mDescriptors = cv::Mat(n, 32, CV_8UC1);
    for (int i = 0; i < n; i++) { o.mvKeysUn[i] = key(i); for (int j = 0; j < 32; j++) o.mDescriptors.ptr(i)[j] = desc_byte(i, j); }
    o.mvuRight.clear();
    if (with_u_right) for (int i = 0; i < n; i++) o.mvuRight.push_back(100.f + i);
    o.mvScaleFactors.clear();
    for (int l = 0; l < n_levels; l++) o.mvScaleFactors.push_back(1.f + 0.2f * l);
}
cv::Mat pose() { cv::Mat T(4, 4, CV_32F); for (int k = 0; k < 16; k++) T.at<float>(k / 4, k % 4) = pose_value(k); return T; }

// keys, descriptors, u_right and the padding of a view gathered from `o`
template <class T> int check_arrays(const ViewGather& g, T& o, int n, bool with_u_right) {
    const int S = n > 0 ? n : 1;
    CHECK(g.view.B == 1 && g.view.stride == S && g.view.n == &g.n && *g.view.n == n);
    CHECK(g.view.keys_un == g.keys.data() && g.view.keys_un && (int)g.keys.size() == S);
    CHECK(g.view.desc == g.desc.data() && g.view.desc && (int)g.desc.size() == S * 32);
    CHECK(g.view.u_right == g.ur.data() && g.view.u_right && (int)g.ur.size() == S);
    for (int i = 0; i < n; i++) {
        CHECK(std::memcmp(&g.view.keys_un[i], &o.mvKeysUn[i], sizeof(planar_keypoint)) == 0);
        for (int j = 0; j < 32; j++) CHECK(g.view.desc[32 * i + j] == desc_byte(i, j));
        CHECK(g.view.u_right[i] == (with_u_right ? 100.f + i : -1.f));
    }
    if (n == 0) {       // the padded slot
        const planar_keypoint zero = planar_keypoint();
        CHECK(std::memcmp(&g.view.keys_un[0], &zero, sizeof(zero)) == 0 && g.view.u_right[0] == -1.f);
        for (int j = 0; j < 32; j++) CHECK(g.view.desc[j] == 0);
    }
    return 0;
}
int check_pose(const ViewGather& g) {
    CHECK(g.view.Tcw == g.Tcw);
    for (int k = 0; k < 16; k++) CHECK(g.view.Tcw[k] == pose_value(k));
    return 0;
}
int check_scales(const ViewGather& g, int n_levels, bool ones_first) {
    for (int l = 0; l < PLANAR_MAX_LEVELS; l++) CHECK(g.view.scale_factors[l] == (l < n_levels ? 1.f + 0.2f * l : ones_first ? 1.f : 0.f));
    return 0;
}

int frame_cases(int n, bool with_u_right) {
    Frame F;
    fill(F, n, with_u_right, 20);         // 20 levels: 16 are copied
    F.mTcw = pose();
    std::vector<MapPoint> mps(3);
    mps[1].obs = 2;                       // feature 0: a point nobody observes, 1: an observed one, 2: none
    F.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n && i < 2; i++) F.mvpMapPoints[i] = &mps[i];
    ViewGather g;
    g.add_keys(F.mvKeysUn, F.N).add_u_right(F.mvuRight).add_desc(F.mDescriptors).add_blocked_observed(F.mvpMapPoints).add_pose(F.mTcw);
    g.add_bounds(F).add_grid(F).add_intrinsics(F).add_stereo(F).add_scales(F.mvScaleFactors, false);
    if (check_arrays(g, F, n, with_u_right) || check_pose(g) || check_scales(g, 20, false)) return 1;
    CHECK(g.view.blocked == g.blocked.data() && g.view.blocked && (int)g.blocked.size() == g.view.stride);
    for (int i = 0; i < g.view.stride; i++) CHECK(g.view.blocked[i] == (i == 1 && n > 1 ? 1 : 0));
    CHECK(g.view.min_x == -3.f && g.view.max_x == 643.f && g.view.min_y == -2.f && g.view.max_y == 481.f);
    CHECK(g.view.grid_w_inv == 0.1f && g.view.grid_h_inv == 0.0625f);
    CHECK(g.view.fx == 535.4f && g.view.fy == 539.2f && g.view.cx == 320.1f && g.view.cy == 247.6f && g.view.bf == 40.f && g.view.b == 0.08f);
    // blocked off, no pose yet (an empty mTcw sets none)
    ViewGather h;
    h.add_keys(F.mvKeysUn, F.N).add_desc(F.mDescriptors).add_pose(cv::Mat());
    CHECK(h.view.blocked == nullptr && h.view.u_right == nullptr && h.view.Tcw == nullptr && h.view.keys_un == h.keys.data() && h.view.desc == h.desc.data());
    // a copy points into its own storage and holds the same values; so does an assigned one, and neither follows the original afterwards
    ViewGather c(g), a;
    a = g;
    g.n = -7; g.keys[0].angle = -1.f; g.ur[0] = 9.f; g.desc[0] = 255; g.blocked[0] = 9; g.Tcw[0] = -1.f;
    for (const ViewGather* v : {&c, &a}) {
        CHECK(v->view.n == &v->n && v->view.keys_un == v->keys.data() && v->view.u_right == v->ur.data() && v->view.desc == v->desc.data());
        CHECK(v->view.blocked == v->blocked.data() && v->view.Tcw == v->Tcw && v->view.keys_un != g.keys.data());
        if (check_arrays(*v, F, n, with_u_right) || check_pose(*v) || check_scales(*v, 20, false)) return 1;
        CHECK(v->view.fx == 535.4f && v->view.max_y == 481.f && v->view.blocked[0] == 0);
    }
    return 0;
}

int keyframe_cases(int n) {
    KeyFrame K;
    fill(K, n, true, 5);
    K.Tcw = pose();
    const float Km[9] = {525.f, 0, 319.5f, 0, 526.f, 239.5f, 0, 0, 1};
    K.mK = cv::Mat(3, 3, CV_32F);
    std::memcpy(K.mK.data, Km, sizeof(Km));
    // the pose from GetPose(), per-object bounds / grid / camera, 5 levels over zeros
    ViewGather g;
    g.add_keys(K.mvKeysUn, K.N).add_u_right(K.mvuRight).add_desc(K.mDescriptors).add_pose(K.GetPose());
    g.add_bounds(K).add_grid(K).add_intrinsics(K).add_stereo(K).add_scales(K.mvScaleFactors, false);
    if (check_arrays(g, K, n, true) || check_pose(g) || check_scales(g, 5, false)) return 1;
    CHECK(g.view.blocked == nullptr);
    CHECK(g.view.min_x == 1.f && g.view.max_x == 639.f && g.view.min_y == 2.f && g.view.max_y == 478.f && g.view.grid_w_inv == 0.2f && g.view.grid_h_inv == 0.125f);
    CHECK(g.view.fx == 517.3f && g.view.fy == 516.5f && g.view.cx == 318.6f && g.view.cy == 255.3f && g.view.bf == 41.f && g.view.b == 0.09f);
    // the pose from [R | t], the camera from mK, 5 levels over ones; nothing else is set
    ViewGather s;
    s.add_keys(K.mvKeysUn, (int)K.mvKeysUn.size()).add_pose(K.GetRotation(), K.GetTranslation()).add_intrinsics_K(K.mK).add_scales(K.mvScaleFactors, true);
    CHECK(s.view.Tcw == s.Tcw && s.view.stride == (n > 0 ? n : 1) && *s.view.n == n);
    for (int k = 0; k < 12; k++) CHECK(s.view.Tcw[k] == pose_value(k));
    CHECK(s.view.Tcw[12] == 0.f && s.view.Tcw[13] == 0.f && s.view.Tcw[14] == 0.f && s.view.Tcw[15] == 1.f);
    CHECK(s.view.fx == 525.f && s.view.fy == 526.f && s.view.cx == 319.5f && s.view.cy == 239.5f && s.view.bf == 0.f && s.view.b == 0.f);
    CHECK(s.view.u_right == nullptr && s.view.desc == nullptr && s.view.blocked == nullptr && s.view.min_x == 0.f && s.view.grid_w_inv == 0.f);
    if (check_scales(s, 5, true)) return 1;
    // no key points at all (the line fuse's view): n and keys_un stay NULL over one slot; free `blocked` flags for the section to set
    ViewGather l;
    l.add_pose(K.GetPose()).add_bounds(K).add_blocked();
    CHECK(l.view.B == 1 && l.view.stride == 1 && l.view.n == nullptr && l.view.keys_un == nullptr && l.view.blocked == l.blocked.data() && l.blocked.size() == 1);
    return check_pose(l);
}

int point_cases() {
    const int M = 4;                      // NULL, bad, good, good but already in the key frame
    std::vector<MapPoint> mp(M);
    for (int j = 0; j < M; j++) {
        const float x[3] = {1.f + j, 2.f + j, 3.f + j}, nv[3] = {0.1f * j, 0.2f, -0.3f};
        mp[j].pos = cv::Mat(3, 1, CV_32F); mp[j].normal = cv::Mat(3, 1, CV_32F); mp[j].desc = cv::Mat(1, 32, CV_8UC1);
        std::memcpy(mp[j].pos.data, x, 12); std::memcpy(mp[j].normal.data, nv, 12);
        for (int k = 0; k < 32; k++) mp[j].desc.ptr(0)[k] = desc_byte(j, k);
        mp[j].mn = 0.5f + j; mp[j].mx = 8.f + j;
    }
    mp[1].bad = true; mp[3].in_kf = true;
    const std::vector<MapPoint*> v = {nullptr, &mp[1], &mp[2], &mp[3]};
    for (int excl = 0; excl < 2; excl++) {
        for (int extras = 0; extras < 2; extras++) {
            PointGather p;
            if (excl) p.add_points(v, v.size(), [](MapPoint* q) { return q->IsInKeyFrame(nullptr); });
            else p.add_points(v);
            if (extras) p.add_normals(v).add_desc(v).add_range(v);
            const PointGather c(p);       // and its copy, which must point into itself
            p.usable[2] = 7;
            CHECK(c.kp.usable == c.usable.data() && c.kp.xw == c.xw.data() && c.usable.size() == 4 && c.xw.size() == 12 && c.kp.usable != p.usable.data());
            for (int j = 0; j < M; j++) {
                const bool use = j == 2 || (j == 3 && !excl);
                CHECK(c.kp.usable[j] == (use ? 1 : 0));
                for (int k = 0; k < 3; k++) CHECK(c.kp.xw[3 * j + k] == (use ? 1.f + k + j : 0.f));
                if (!extras) continue;
                for (int k = 0; k < 3; k++) CHECK(c.nrm[3 * j + k] == (!use ? 0.f : k == 0 ? 0.1f * j : k == 1 ? 0.2f : -0.3f));
                for (int k = 0; k < 32; k++) CHECK(c.kp.desc[32 * j + k] == (use ? desc_byte(j, k) : 0));
                CHECK(c.kp.min_dist[j] == (use ? 0.5f + j : 0.f) && c.kp.max_dist[j] == (use ? 8.f + j : 0.f));
            }
            if (extras) CHECK(c.kp.desc == c.desc.data() && c.kp.min_dist == c.mn.data() && c.kp.max_dist == c.mx.data() && c.nrm.size() == 12 && c.desc.size() == 128);
            else CHECK(c.kp.desc == nullptr && c.kp.min_dist == nullptr && c.kp.max_dist == nullptr && c.nrm.empty() && c.desc.empty() && c.mn.empty());
        }
    }
    // more slots than the list is long (a key frame with more features than map-point slots): the rest counts as NULL; no slot at all pads to one
    PointGather six, none;
    six.add_points(v, 6, planar_adapter::NoExclusion());
    CHECK(six.usable.size() == 6 && six.xw.size() == 18 && six.usable[2] == 1 && six.usable[3] == 1 && six.usable[4] == 0 && six.usable[5] == 0 && six.xw[17] == 0.f);
    none.add_points(std::vector<MapPoint*>());
    CHECK(none.usable.size() == 1 && none.usable[0] == 0 && none.xw.size() == 3 && none.kp.usable == none.usable.data() && none.kp.xw == none.xw.data());
    return 0;
}
}  // namespace

int main() {
    for (int n : {0, 3})
        for (int with_u_right = 0; with_u_right < 2; with_u_right++)
            if (frame_cases(n, with_u_right != 0)) return 1;
    for (int n : {0, 3}) if (keyframe_cases(n)) return 1;
    if (point_cases()) return 1;
    std::printf("adapter_gather: all equal\n");
    return 0;
}
