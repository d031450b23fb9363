/* planar_abi.h — C ABI of libplanar_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for PlanarSLAM's per-frame extract -> match -> pose-optimise
 * hot path.  POD only: plain pointers and sizes, no OpenCV /
 * Eigen / torch types.  Every entry point cites the reference interface it
 * replaces (paths relative to the PlanarSLAM tree).
 *
 * Conventions
 *  - return 0 (PLANAR_OK) on success, a negative PLANAR_E* code otherwise;
 *    never throws, never exits.  planar_last_error() gives a message (per thread).
 *  - "_dev" entry points take DEVICE pointers and only enqueue work on the
 *    context's stream (results valid after planar_ctx_sync / a stream sync);
 *    entry points without the suffix take HOST pointers, are synchronous, and
 *    are what the reference-signature adapters call.
 *  - the caller owns every buffer; a context is not re-entrant (one per host
 *    thread, as the reference's ORBextractor instance is, include/ORBextractor.h:85).
 *  - a batch is B independent frames; frame b of a per-frame array starts at
 *    b * <documented stride>.
 */
#ifndef PLANAR_ABI_H
#define PLANAR_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLANAR_OK 0
#define PLANAR_EINVAL (-1)   /* bad argument (null pointer, size out of range) */
#define PLANAR_ENOMEM (-2)   /* device/host allocation failed */
#define PLANAR_EDEVICE (-3)  /* HIP runtime error (no device, launch failure) */
#define PLANAR_ECAPACITY (-4) /* output capacity too small */
#define PLANAR_ESTATE (-5)   /* call out of order */

typedef struct planar_ctx planar_ctx;

/* Same 28-byte layout as cv::KeyPoint (pt.x, pt.y, size, angle, response, octave, class_id),
 * so an adapter can memcpy into std::vector<cv::KeyPoint>. */
typedef struct planar_keypoint {
    float x, y;       /* level-0 pixel coordinates (level coords * scale[octave]), ORBextractor.cc:1094-1100 */
    float size;       /* (int)(31 * scale[octave]),                                  ORBextractor.cc:835,845 */
    float angle;      /* IC_Angle, degrees [0,360),                                  ORBextractor.cc:77-104 */
    float response;   /* FAST-9/16 corner score                                                              */
    int32_t octave;   /* pyramid level                                                                       */
    int32_t class_id; /* -1                                                                                  */
} planar_keypoint;

/* ---- context ------------------------------------------------------------------------- */
/* Creates a context on HIP device `device` with its own stream. */
int planar_ctx_create(planar_ctx** out, int device);
void planar_ctx_destroy(planar_ctx* ctx);
/* Use an external hipStream_t (e.g. torch's current stream) for all subsequent work; NULL
 * restores the context's own stream. */
int planar_ctx_set_stream(planar_ctx* ctx, void* hip_stream);
/* CU partition for the extractors' one-wavefront-per-frame kernels (no reference counterpart: the reference runs its three extractors on three CPU threads,
 * src/Frame.cc:90-95; this is the device-side analogue of pinning the sequential ones to some cores).  planar_cu_stream_create makes a HIP stream whose kernels
 * run only on the compute units whose bit is set in cu_mask (n_words x 32 bits, bit i = CU i in the driver's round-robin-over-XCDs numbering:
 * hipExtStreamCreateWithCUMask); planar_ctx_set_seq_stream(ctx, s) makes the context launch the PEAC clustering kernel and LSD's region-growing kernel on s
 * (forked from / joined into the context's stream by events, so results and ordering are unchanged); s = NULL restores the single-stream behaviour (default).
 * One such stream may be shared by several contexts.  The caller destroys it after the contexts.  The context must be idle when planar_ctx_set_seq_stream is called. */
int planar_cu_stream_create(int device, const uint32_t* cu_mask, int n_words, void** out_stream);
void planar_cu_stream_destroy(void* stream);
int planar_ctx_set_seq_stream(planar_ctx* ctx, void* stream);
void* planar_ctx_get_stream(planar_ctx* ctx);
int planar_ctx_sync(planar_ctx* ctx);
const char* planar_last_error(void);
/* Library/ABI version: major*10000 + minor*100 + patch. */
int planar_abi_version(void);

/* ---- ORB extractor (replaces Planar_SLAM::ORBextractor, include/ORBextractor.h:45-112) -- */
typedef struct planar_orb planar_orb;

typedef struct planar_orb_params {
    int32_t nfeatures;    /* ORBextractor.nFeatures   (1000) */
    float scale_factor;   /* ORBextractor.scaleFactor (1.2)  */
    int32_t nlevels;      /* ORBextractor.nLevels     (8)    */
    int32_t ini_th_fast;  /* ORBextractor.iniThFAST   (20)   */
    int32_t min_th_fast;  /* ORBextractor.minThFAST   (7)    */
} planar_orb_params;

/* ORBextractor::ORBextractor (src/ORBextractor.cc:410-470) + all device workspace for
 * batches of up to max_batch frames of width x height 8-bit gray. */
int planar_orb_create(planar_ctx* ctx, const planar_orb_params* params, int width, int height, int max_batch,
                      planar_orb** out);
void planar_orb_destroy(planar_orb* orb);
/* Upper bound on keypoints per frame (nfeatures + small octree overshoot); the per-frame
 * stride of `kps`/`desc` below. */
int planar_orb_max_keypoints(const planar_orb* orb);
/* Getters of the reference class (include/ORBextractor.h:63-83): out[nlevels]. */
int planar_orb_get_scale_factors(const planar_orb* orb, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2);
int planar_orb_level_size(const planar_orb* orb, int level, int* w, int* h);
int planar_orb_features_per_level(const planar_orb* orb, int32_t* out);

/* ORBextractor::operator() (src/ORBextractor.cc:1043-1105) on B frames.
 *   gray   : B frames, row pitch `pitch` bytes, frame stride `frame_stride` bytes
 *   kps    : [B][planar_orb_max_keypoints]           desc : [B][max_keypoints][32]
 *   n_out  : [B] keypoints found per frame
 * Host-pointer version: copies in, runs, copies out, synchronous. */
int planar_orb_extract(planar_orb* orb, const uint8_t* gray, int B, int pitch, int64_t frame_stride,
                       planar_keypoint* kps, uint8_t* desc, int32_t* n_out);
/* Device-pointer version: enqueues on the context stream and returns. */
int planar_orb_extract_dev(planar_orb* orb, const uint8_t* d_gray, int B, int pitch, int64_t frame_stride,
                           planar_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n_out);

/* Synchronises; PLANAR_ECAPACITY if a FAST cell produced more non-max-suppressed corners than its candidate slots since the last check
 * (the slot count is the mathematical bound on strict 8-neighbour maxima, so this reports a broken invariant, not a tuning limit).
 * The host-pointer entry point calls it itself. */
int planar_orb_check(planar_orb* orb);

/* Stage read-back for parity tests and for the adapter's public mvImagePyramid member
 * (include/ORBextractor.h:85).  Valid after an extract call; host output buffers. */
int planar_orb_read_level(planar_orb* orb, int frame, int level, uint8_t* out /* w*h */);
int planar_orb_read_blurred(planar_orb* orb, int frame, int level, uint8_t* out /* w*h */);
/* FAST survivors of one level in the reference's emission order (ORBextractor.cc:789-826):
 * out = n x {x, y, score} relative to (minBorderX, minBorderY); returns n or a negative code. */
int planar_orb_read_candidates(planar_orb* orb, int frame, int level, int32_t* out, int cap);

/* Per-launch timing with HIP events on the context stream (bench.py's roofline leg).
 * set_profiling(1) starts recording an event before/after every kernel launch of each
 * extract call; get_profile synchronises, returns the summed milliseconds per launch slot
 * (total_ms[planar_orb_profile_num_launches]) and the number of recorded calls, and resets. */
int planar_orb_set_profiling(planar_orb* orb, int enable);
int planar_orb_profile_num_launches(const planar_orb* orb);
const char* planar_orb_profile_launch_name(const planar_orb* orb, int i);
int planar_orb_get_profile(planar_orb* orb, double* total_ms, int64_t* calls);

/* ---- pose optimisation (replaces Optimizer::PoseOptimization, src/Optimizer.cc:550-1275, and
 *      Optimizer::TranslationOptimization, :2995-3738; include/Optimizer.h:37,43) ------------ */
#define PLANAR_POSE_FULL 0         /* PoseOptimization: point/line/plane/parallel/vertical edges, 6-DoF */
#define PLANAR_POSE_TRANSLATION 1  /* TranslationOptimization: ...OnlyTranslation edges, rotation kept  */

typedef struct planar_pose_params {
    float fx, fy, cx, cy, bf;      /* Frame::fx, fy, cx, cy, mbf                                         */
    /* raw Config values (src/Optimizer.cc:771-783): Plane.AngleInfo, Plane.DistanceInfo,
     * Plane.ParallelInfo, Plane.VerticalInfo, Plane.Chi, Plane.VPChi                                    */
    double angle_info, distance_info, parallel_info, vertical_info, plane_chi, vp_chi;
} planar_pose_params;

/* B frames, structure-of-arrays with per-frame strides max_points / max_lines / max_planes.
 * Inputs mirror the Frame fields the reference reads:                            */
typedef struct planar_pose_batch {
    int32_t B, max_points, max_lines, max_planes;
    const int32_t* n_points;       /* [B]  Frame::N                                                      */
    const int32_t* n_lines;        /* [B]  Frame::NL                                                     */
    const int32_t* n_planes;       /* [B]  Frame::mnPlaneNum                                             */
    const uint8_t* pt_valid;       /* [B][max_points]      mvpMapPoints[i] != NULL                       */
    const float* pt_xw;            /* [B][max_points][3]   MapPoint::GetWorldPos() (float32)             */
    const float* pt_obs;           /* [B][max_points][3]   mvKeysUn[i].pt.x, .pt.y, mvuRight[i] (<0: mono) */
    const float* pt_inv_sigma2;    /* [B][max_points]      mvInvLevelSigma2[mvKeysUn[i].octave]          */
    const uint8_t* ln_valid;       /* [B][max_lines]       mvpMapLines[i] != NULL                        */
    const double* ln_obs;          /* [B][max_lines][3]    mvKeyLineFunctions[i]                         */
    const double* ln_xw;           /* [B][max_lines][6]    MapLine::mWorldPos (start xyz, end xyz)       */
    const float* pl_meas;          /* [B][max_planes][4]   mvPlaneCoefficients[i]                        */
    const uint8_t* pl_valid;       /* [B][max_planes][3]   mvpMapPlanes / mvpParallelPlanes / mvpVerticalPlanes[i] != NULL */
    const float* pl_world;         /* [B][max_planes][3][4] GetWorldPos() of those three map planes      */
    const float* Tcw_in;           /* [B][16]              Frame::mTcw, row-major 4x4 float32            */
    /* outputs */
    float* Tcw_out;                /* [B][16]              pose passed to Frame::SetPose                 */
    uint8_t* pt_outlier;           /* [B][max_points]      mvbOutlier      (written only where pt_valid) */
    uint8_t* ln_outlier;           /* [B][max_lines]       mvbLineOutlier  (written only where ln_valid) */
    uint8_t* pl_outlier;           /* [B][max_planes][3]   mvbPlaneOutlier / mvbParPlaneOutlier / mvbVerPlaneOutlier (written only where pl_valid, see below) */
    int32_t* n_inliers;            /* [B]                  the reference function's return value         */
    int32_t* lm_iters;             /* [B] or NULL          LM iterations run (diagnostic)                */
} planar_pose_batch;

/* rounds = 4, its = 10 reproduce the reference protocol (4 x optimize(10) with outlier
 * re-classification, src/Optimizer.cc:990-1000).  All pointers in `batch` are HOST pointers for
 * planar_pose_opt (synchronous) and DEVICE pointers for planar_pose_opt_dev (enqueue only; the
 * struct itself is always host memory, passed by value to the kernel).
 *
 * What is written when (the reference's own statements, src/Optimizer.cc:593-985 / :3034-3270): a flag is written only where its valid byte is
 * set and its index is below the frame's count; every other entry keeps the caller's value.  pl_outlier[i][kind] is written only where
 * pl_valid[i][kind]; kinds 1 and 2 (parallel, vertical) never in translation mode, whose edges for them are commented out (:3370, :3413); and no
 * plane flag at all when TranslationOptimization returns early (fewer than 3 valid points, :3199, which stands before the plane edges are built;
 * point and line flags are already cleared where valid by then).  PoseOptimization's early return (:985) comes after all flags are cleared.
 * n_inliers may be negative in translation mode: planes count towards the outliers subtracted but not towards the correspondences.
 *
 * Defined where the reference is not: n_points[b] is clamped to [0, max_points] and n_lines[b] to [0, max_lines]; a negative n_planes[b] is 0;
 * n_planes[b] > max_planes gives n_inliers[b] = -1, Tcw_out = Tcw_in and lm_iters[b] = 0, with point and line flags as an early return leaves
 * them (cleared where valid) and no plane array of that frame read or written.  Nothing outside a frame's own rows is touched.
 * PLANAR_EINVAL (nothing launched): a null argument or array whose stride is > 0, B < 1, a negative stride, max_planes > 32, a mode other than
 * the two above, rounds outside [1, 4], its < 1, or strides that need more than 160 KiB of LDS per frame. */
int planar_pose_opt(planar_ctx* ctx, const planar_pose_batch* batch, const planar_pose_params* params, int mode, int rounds, int its);
int planar_pose_opt_dev(planar_ctx* ctx, const planar_pose_batch* d_batch, const planar_pose_params* params, int mode, int rounds, int its);

/* ---- descriptor matchers ------------------------------------------------------------------
 * Descriptors are 32-byte rows (cv::Mat N x 32 CV_8U: Frame::mDescriptors, Frame::mLdesc).
 * Batched over B frame pairs: pair b uses rows [b*stride, b*stride + n[b]).                      */

/* cv::BFMatcher(cv::NORM_HAMMING).match (k = 1) / .knnMatch(..., 2) (k = 2), as called at
 * src/ORBmatcher.cc:1346-1347 and src/LSDmatcher.cpp:249-254.  idx/dist: [B][q_stride][k], ascending
 * distance, lowest train index on ties; a missing neighbour is idx -1 / dist INT32_MAX. */
int planar_hamming_knn(planar_ctx* ctx, const uint8_t* q, const int32_t* nq, int q_stride, const uint8_t* t, const int32_t* nt,
                       int t_stride, int B, int k, int32_t* idx, int32_t* dist);
int planar_hamming_knn_dev(planar_ctx* ctx, const uint8_t* d_q, const int32_t* d_nq, int q_stride, const uint8_t* d_t,
                           const int32_t* d_nt, int t_stride, int B, int k, int32_t* d_idx, int32_t* d_dist);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:259-324) for n_points map points at once: point p observes the descriptors
 * desc[off[p] .. off[p + 1]) (the rows pKF->mDescriptors.row(idx) of its non-bad key frames, in the order of the observation map); best[p] = index within that
 * list of the descriptor with the least median Hamming distance to all of them (first minimum; -1 without observations), median[p] (or NULL) that median.
 * _dev: max_obs = an upper bound of the observations per point (<= 2047; a point with more gets best = -2). */
/* MapLine::ComputeDistinctiveDescriptors (src/MapLine.cpp:241) is the same computation on LBD rows (32 bytes, the median at (n - 1) / 2): pass mLineDescriptors rows. */
int planar_distinctive_descriptors(planar_ctx* ctx, int n_points, const uint8_t* desc, const int32_t* off, int32_t* best, int32_t* median);
int planar_distinctive_descriptors_dev(planar_ctx* ctx, int n_points, const uint8_t* d_desc, const int32_t* d_off, int max_obs, int32_t* d_best, int32_t* d_median);

/* ORBmatcher::MatchORBPoints(Frame& Current, const Frame& Last) (src/ORBmatcher.cc:1332-1394).
 *   last_has_mp[j]   LastFrame.mvpMapPoints[j] != NULL        last_outlier[j]  LastFrame.mvbOutlier[j]
 *   cur_match[q]     (in/out) index j of the last-frame keypoint whose MapPoint the reference copies into
 *                    CurrentFrame.mvpMapPoints[q]; entries the reference does not assign keep their value
 *   npair[b]         the function's return value (number of good matches)                           */
int planar_match_orb_points(planar_ctx* ctx, const uint8_t* cur, const int32_t* n_cur, int cur_stride, const uint8_t* last,
                            const int32_t* n_last, int last_stride, const uint8_t* last_has_mp, const uint8_t* last_outlier, int B,
                            int32_t* cur_match, int32_t* npair);
int planar_match_orb_points_dev(planar_ctx* ctx, const uint8_t* d_cur, const int32_t* d_n_cur, int cur_stride, const uint8_t* d_last,
                                const int32_t* d_n_last, int last_stride, const uint8_t* d_last_has_mp, const uint8_t* d_last_outlier,
                                int B, int32_t* d_cur_match, int32_t* d_npair);

/* LSDmatcher::SearchByDescriptor(KeyFrame*, Frame&, vector<MapLine*>&) (src/LSDmatcher.cpp:242-279).
 *   kf_has_ml[i]     pKF->GetMapLineMatches()[i] != NULL
 *   cur_match[t]     (out) keyframe line index whose MapLine lands in vpMapLineMatches[t], or -1
 *   nmatches[b]      the function's return value                                                    */
int planar_lsd_search_by_descriptor(planar_ctx* ctx, const uint8_t* kf, const int32_t* n_kf, int kf_stride, const uint8_t* cur,
                                    const int32_t* n_cur, int cur_stride, const uint8_t* kf_has_ml, int B, int32_t* cur_match,
                                    int32_t* nmatches);
int planar_lsd_search_by_descriptor_dev(planar_ctx* ctx, const uint8_t* d_kf, const int32_t* d_n_kf, int kf_stride, const uint8_t* d_cur,
                                        const int32_t* d_n_cur, int cur_stride, const uint8_t* d_kf_has_ml, int B, int32_t* d_cur_match,
                                        int32_t* d_nmatches);

/* ---- guided (projection / vocabulary-node / coefficient) matchers ---------------------------
 * These reproduce the reference's SEQUENTIAL assignment semantics exactly: probes (map points, last-frame
 * points, key-frame features) are resolved in the reference's loop order and every assignment updates the
 * "already matched" state later probes see.  All arrays are batched over B independent frames with fixed
 * per-frame strides; pointers are HOST pointers for the plain entry points and DEVICE pointers for *_dev
 * (the view structs themselves are always host memory). */
#define PLANAR_MAX_LEVELS 16
#define PLANAR_GRID_COLS 64 /* FRAME_GRID_COLS include/Frame.h:38 */
#define PLANAR_GRID_ROWS 48 /* FRAME_GRID_ROWS include/Frame.h:37 */
#define PLANAR_MAX_FRAME_KEYS 4096 /* limit on Frame::N / probes per frame for the guided matchers */

/* The fields of the Frame being matched INTO that the guided matchers read (include/Frame.h). */
typedef struct planar_frame_view {
    int32_t B, stride;               /* frames, per-frame capacity of the arrays below                     */
    const int32_t* n;                /* [B]             Frame::N                                            */
    const planar_keypoint* keys_un;  /* [B][stride]     mvKeysUn (pt, angle, octave are read)               */
    const float* u_right;            /* [B][stride]     mvuRight                                            */
    const uint8_t* desc;             /* [B][stride][32] mDescriptors                                        */
    const uint8_t* blocked;          /* [B][stride]     mvpMapPoints[i] != NULL && ->Observations() > 0 on entry (NULL = none) */
    const float* Tcw;                /* [B][16]         mTcw (frame-to-frame variant only)                  */
    float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY (src/Frame.cc:117-123)              */
    float grid_w_inv, grid_h_inv;    /* mfGridElementWidthInv / mfGridElementHeightInv                      */
    float fx, fy, cx, cy, bf, b;     /* Frame::fx.. , mbf, mb                                               */
    float scale_factors[PLANAR_MAX_LEVELS]; /* mvScaleFactors                                              */
} planar_frame_view;

/* LastFrame side of ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono). */
typedef struct planar_last_frame_view {
    int32_t stride;
    const int32_t* n;            /* [B]             LastFrame.N                                              */
    const float* Tcw;            /* [B][16]         LastFrame.mTcw                                           */
    const uint8_t* usable;       /* [B][stride]     mvpMapPoints[i] != NULL && !mvbOutlier[i]                */
    const float* xw;             /* [B][stride][3]  mvpMapPoints[i]->GetWorldPos()                           */
    const int32_t* octave;       /* [B][stride]     mvKeys[i].octave                                         */
    const float* angle;          /* [B][stride]     mvKeysUn[i].angle                                        */
    const uint8_t* mp_desc;      /* [B][stride][32] mvpMapPoints[i]->GetDescriptor()                         */
    const uint8_t* mp_observed;  /* [B][stride]     mvpMapPoints[i]->Observations() > 0                      */
} planar_last_frame_view;

/* ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) (src/ORBmatcher.cc:1396-1535).
 *   cur_match[b][i2] (in/out): index i of the LAST-frame keypoint whose MapPoint the reference stores in
 *       CurrentFrame.mvpMapPoints[i2]; -1 where the rotation check resets it to NULL; untouched otherwise.
 *   nmatches[b]: the function's return value. */
int planar_search_by_projection_frame(planar_ctx* ctx, const planar_frame_view* cur, const planar_last_frame_view* last, float th,
                                      int mono, int check_orientation, int32_t* cur_match, int32_t* nmatches);
int planar_search_by_projection_frame_dev(planar_ctx* ctx, const planar_frame_view* d_cur, const planar_last_frame_view* d_last, float th,
                                          int mono, int check_orientation, int32_t* d_cur_match, int32_t* d_nmatches);

/* The MapPoint tracking fields written by Frame::isInFrustum (src/Frame.cc:312-367) and read by
 * ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:46-130). */
typedef struct planar_map_probes {
    int32_t stride;
    const int32_t* n;            /* [B]             vpMapPoints.size()                                       */
    const uint8_t* in_view;      /* [B][stride]     mbTrackInView && !isBad()                                */
    const float* proj_x;         /* [B][stride]     mTrackProjX                                              */
    const float* proj_y;         /* [B][stride]     mTrackProjY                                              */
    const float* proj_xr;        /* [B][stride]     mTrackProjXR                                             */
    const int32_t* level;        /* [B][stride]     mnTrackScaleLevel                                        */
    const float* view_cos;       /* [B][stride]     mTrackViewCos                                            */
    const uint8_t* desc;         /* [B][stride][32] GetDescriptor()                                          */
    const uint8_t* observed;     /* [B][stride]     Observations() > 0                                       */
} planar_map_probes;

/* match[b][idx] (in/out): index iMP of the map point stored in F.mvpMapPoints[idx]. nn_ratio = mfNNratio. */
int planar_search_by_projection_map(planar_ctx* ctx, const planar_frame_view* frame, const planar_map_probes* probes, float th,
                                    float nn_ratio, int32_t* match, int32_t* nmatches);
int planar_search_by_projection_map_dev(planar_ctx* ctx, const planar_frame_view* d_frame, const planar_map_probes* d_probes, float th,
                                        float nn_ratio, int32_t* d_match, int32_t* d_nmatches);

/* Key-frame side of ORBmatcher::SearchByProjection(Frame&, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:1537-1663), the relocalisation search.  Entry i is pKF->GetMapPointMatches()[i]. */
typedef struct planar_keyframe_probes {
    int32_t stride;
    const int32_t* n;            /* [B]             vpMPs.size()                                             */
    const uint8_t* usable;       /* [B][stride]     vpMPs[i] != NULL && !isBad()                             */
    const uint8_t* found;        /* [B][stride]     sAlreadyFound.count(vpMPs[i]) (NULL = empty set)         */
    const float* xw;             /* [B][stride][3]  GetWorldPos()                                            */
    const float* min_dist;       /* [B][stride]     mfMinDistance (the 0.8 of GetMinDistanceInvariance is applied here) */
    const float* max_dist;       /* [B][stride]     mfMaxDistance (1.2 of GetMaxDistanceInvariance; PredictScale reads it bare) */
    const float* angle;          /* [B][stride]     pKF->mvKeysUn[i].angle                                   */
    const uint8_t* desc;         /* [B][stride][32] GetDescriptor()                                          */
} planar_keyframe_probes;

/* ORBmatcher(nnratio, check_orientation)::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), batched over B (frame, key frame)
 * pairs.  cur: keys_un, desc, Tcw, bounds, grid, fx fy cx cy, scale_factors are read; blocked[i2] = CurrentFrame.mvpMapPoints[i2] != NULL on
 * entry (NULL = none); u_right is not read (this overload has no stereo gate).  log_scale_factor / n_levels = CurrentFrame.mfLogScaleFactor /
 * mnScaleLevels (MapPoint::PredictScale, src/MapPoint.cc:419-434).  Kept as the reference has them: no depth test before the projection, no
 * ratio test, bestDist starts at 256 and bestDist <= ORBdist decides; key-frame points are resolved in index order and a match is written into
 * mvpMapPoints at once, so later points skip that keypoint; ComputeThreeMaxima's removal runs last.  orb_dist < 256 is required (the reference
 * writes mvpMapPoints[-1] otherwise).
 *   cur_match[b][i2] (in/out): key-frame index i of the map point the reference stores in CurrentFrame.mvpMapPoints[i2]; -1 where the rotation
 *       check resets it to NULL; untouched otherwise.
 *   nmatches[b]: the function's return value. */
int planar_search_by_projection_keyframe(planar_ctx* ctx, const planar_frame_view* cur, const planar_keyframe_probes* kf, float log_scale_factor,
                                         int n_levels, float th, int orb_dist, int check_orientation, int32_t* cur_match, int32_t* nmatches);
int planar_search_by_projection_keyframe_dev(planar_ctx* ctx, const planar_frame_view* d_cur, const planar_keyframe_probes* d_kf,
                                             float log_scale_factor, int n_levels, float th, int orb_dist, int check_orientation,
                                             int32_t* d_cur_match, int32_t* d_nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBmatcher.cc:160-292).
 * The DBoW2 FeatureVectors (node id -> feature indices) are passed as one node id per feature (-1: feature
 * is in no node), which is what DBoW2's transform(..., levelsup) produces (each feature falls in one node).
 *   kf_usable[i]  vpMapPointsKF[i] != NULL && !isBad()         kf_angle[i]  pKF->mvKeysUn[i].angle
 *   f_angle[i]    F.mvKeys[i].angle
 *   match[b][iF]  (out) index of the key-frame feature whose MapPoint lands in vpMapPointMatches[iF], else -1 */
int planar_search_by_bow(planar_ctx* ctx, int B, const int32_t* n_kf, int kf_stride, const int32_t* kf_node, const uint8_t* kf_usable,
                         const float* kf_angle, const uint8_t* kf_desc, const int32_t* n_f, int f_stride, const int32_t* f_node,
                         const float* f_angle, const uint8_t* f_desc, float nn_ratio, int check_orientation, int32_t* match,
                         int32_t* nmatches);
int planar_search_by_bow_dev(planar_ctx* ctx, int B, const int32_t* d_n_kf, int kf_stride, const int32_t* d_kf_node,
                             const uint8_t* d_kf_usable, const float* d_kf_angle, const uint8_t* d_kf_desc, const int32_t* d_n_f,
                             int f_stride, const int32_t* d_f_node, const float* d_f_angle, const uint8_t* d_f_desc, float nn_ratio,
                             int check_orientation, int32_t* d_match, int32_t* d_nmatches);

/* ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:309-540): epipolar BoW search + triangulation ---------------------------- */
#define PLANAR_TRI_MAX_NEIGHBOURS 32 /* limit on the neighbours per current key frame (the reference asks for 10, 20 when monocular) */

/* What the key frames of one call share (include/KeyFrame.h): intrinsics, mfScaleFactor, mvScaleFactors, mvLevelSigma2. */
typedef struct planar_tri_camera {
    float fx, fy, cx, cy, invfx, invfy;         /* KeyFrame::fx .. invfy, as the key frame stores them; mK = [fx 0 cx; 0 fy cy; 0 0 1] */
    float scale_factor;                         /* mfScaleFactor (ratioFactor = 1.5f * mfScaleFactor)                                 */
    int32_t n_levels;                           /* mnScaleLevels, 1 .. PLANAR_MAX_LEVELS; key-point octaves must lie below it         */
    float scale_factors[PLANAR_MAX_LEVELS];     /* mvScaleFactors                                                                     */
    float level_sigma2[PLANAR_MAX_LEVELS];      /* mvLevelSigma2                                                                      */
} planar_tri_camera;

/* `count` key frames, [count][stride] arrays.  The second group is read by planar_create_new_map_points only (NULL for the search). */
typedef struct planar_tri_keyframes {
    int32_t count, stride;           /* stride <= PLANAR_MAX_FRAME_KEYS                                                     */
    const int32_t* n;                /* [count]             KeyFrame::N                                                      */
    const planar_keypoint* keys_un;  /* [count][stride]     mvKeysUn (pt, angle, octave are read)                            */
    const float* u_right;            /* [count][stride]     mvuRight (>= 0: stereo)                                          */
    const uint8_t* desc;             /* [count][stride][32] mDescriptors; the array must start on a 16-byte boundary (read as 16-byte words) */
    const int32_t* node;             /* [count][stride]     mFeatVec as planar_bow_transform writes it: node id, -1 = none   */
    const uint8_t* occupied;         /* [count][stride]     GetMapPoint(i) != NULL on entry                                  */
    const float* Tcw;                /* [count][16]         Tcw; Ow is derived as KeyFrame::SetPose does (src/KeyFrame.cc:79-93) */
    const planar_keypoint* keys;     /* [count][stride]     mvKeys: KeyFrame::UnprojectStereo reads the DISTORTED point      */
    const float* depth;              /* [count][stride]     mvDepth (> 0 wherever u_right >= 0)                              */
    const float* cos_stereo;         /* [count][stride]     cos(2 * atan2(mb / 2, mvDepth[i])) in float, by the HOST's libm  */
    const float* Twc;                /* [count][16]         Twc as the key frame holds it (UnprojectStereo)                  */
    const float* mb;                 /* [count]             KeyFrame::mb                                                     */
    const float* mbf;                /* [count]             KeyFrame::mbf                                                    */
} planar_tri_keyframes;

/* ORBmatcher(., check_orientation)::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (src/ORBmatcher.cc:661-827) with
 * F12 = LocalMapping::ComputeF12(pKF1, pKF2) (src/LocalMapping.cc:1141-1157), for kf1->count (key frame 1, key frame 2) pairs: pair b is
 * entry b of both views.  Kept as the reference has them: vbMatched2 is never set, so two features of key frame 1 may take the same feature of
 * key frame 2; the smallest distance <= 50 among the candidates that pass every gate wins and the LAST such candidate (ascending idx2) on a tie.
 *   match12[b][idx1] (out, idx1 < n): vMatches12[idx1], the index in key frame 2 or -1; vMatchedPairs is its ascending-idx1 read.
 *   nmatches[b]: the function's return value. */
int planar_search_for_triangulation(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* kf1, const planar_tri_keyframes* kf2,
                                    int only_stereo, int check_orientation, int32_t* match12, int32_t* nmatches);
int planar_search_for_triangulation_dev(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* d_kf1,
                                        const planar_tri_keyframes* d_kf2, int only_stereo, int check_orientation, int32_t* d_match12,
                                        int32_t* d_nmatches);

/* LocalMapping::CreateNewMapPoints for cur->count current key frames (RGB-D / stereo: mbMonocular == false).  Current key frame b has
 * n_neigh[b] <= max_neigh neighbours, GetBestCovisibilityKeyFrames' order, at entries b * max_neigh + k of `neigh`.  The reference leaves
 * the loop when CheckNewKeyFrames() turns true (:341): a caller that wants to stop early passes fewer neighbours.
 *   n_new[b]            how many points the reference creates (at most n[b]: an accepted feature is occupied for the later neighbours)
 *   new_neigh / new_idx1 / new_idx2 [b][j], new_x3d [b][j][3], j < n_new[b]: the neighbour slot k, the two feature indices and the
 *       position handed to MapPoint's constructor, in the reference's creation order (k ascending, then idx1 ascending).  Entries at and
 *       beyond n_new[b] are not written.  The capacity is cur->stride per key frame.
 * Input the reference would fault on creates no point instead: a stereo feature (u_right >= 0) whose depth is not > 0 when UnprojectStereo is its
 * source; an octave outside [0, PLANAR_MAX_LEVELS) is taken modulo PLANAR_MAX_LEVELS.  `cam` is a HOST pointer in both flavours.
 * new MapPoint, AddObservation, AddMapPoint, ComputeDistinctiveDescriptors and UpdateNormalAndDepth stay with the caller
 * (planar_distinctive_descriptors, planar_update_normal_and_depth). */
int planar_create_new_map_points(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* cur, const planar_tri_keyframes* neigh,
                                 const int32_t* n_neigh, int max_neigh, int32_t* n_new, int32_t* new_neigh, int32_t* new_idx1, int32_t* new_idx2,
                                 float* new_x3d);
int planar_create_new_map_points_dev(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_keyframes* d_cur,
                                     const planar_tri_keyframes* d_neigh, const int32_t* d_n_neigh, int max_neigh, int32_t* d_n_new,
                                     int32_t* d_new_neigh, int32_t* d_new_idx1, int32_t* d_new_idx2, float* d_new_x3d);

/* ---- LocalMapping::CreateNewMapLines2 (src/LocalMapping.cc:800-1037): key-frame / key-frame LBD search + depth lines + gates ---------- */
#define PLANAR_MAX_KEYFRAME_LINES 256 /* limit on the line stride of a key-frame view (the extractor keeps the top 40 lines by default) */

/* `count` key frames, [count][stride] arrays, as planar_lsd_extract and planar_is_line_good leave them.  The two searches read n, ldesc and
 * occupied only (the rest may be NULL). */
struct planar_keyline;
typedef struct planar_tri_line_keyframes {
    int32_t count, stride;           /* stride <= PLANAR_MAX_KEYFRAME_LINES                                                         */
    const int32_t* n;                /* [count]             the number of key lines (mLineDescriptors.rows)                          */
    const struct planar_keyline* keylines; /* [count][stride] mvKeyLines, the struct below (start_x/y, end_x/y and octave are read)        */
    const uint8_t* ldesc;            /* [count][stride][32] mLineDescriptors; must start on a 16-byte boundary (else PLANAR_EINVAL) */
    const uint8_t* occupied;         /* [count][stride]     GetMapLine(i) != NULL on entry                                           */
    const float* depth_line;         /* [count][stride]     mvDepthLine, exactly as planar_is_line_good writes it (> 0: a 3-D line)  */
    const double* lines3d;           /* [count][stride][6]  mvLines3D (camera frame), exactly as planar_is_line_good writes it      */
    const float* Tcw;                /* [count][16]         Tcw; Ow is derived as KeyFrame::SetPose does                             */
    const float* Twc;                /* [count][16]         Twc as the key frame holds it (KeyFrame::obtain3DLine)                   */
    const float* mb;                 /* [count]             KeyFrame::mb                                                             */
} planar_tri_line_keyframes;

/* LSDmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs) (src/LSDmatcher.cpp:334-367) for kf1->count pairs; pair b is entry b of both
 * views.  BFMatcher(NORM_HAMMING).knnMatch(k = 2) over ALL lines of both key frames (occupied ones included; the lowest train index wins a
 * tie), KeyFrame::lineDescriptorMAD (src/KeyFrame.cc:858-883) over all those matches, nn12_dist_th = 0.1 * nn12_mad; query qdx is kept when
 * neither it nor its best target is occupied and double(d1 - d0) > nn12_dist_th.
 *   match12[b][qdx] (out, qdx < n1): the target index or -1; vMatchedPairs is its ascending-qdx read.   nmatches[b]: the return value.
 *   nn_mad / nn12_mad [b] (may be NULL): what lineDescriptorMAD returned, before the factor; 0 where no match exists.
 * Input the reference would fault on gives no matches: n1 == 0, and n2 < 2 (lmatches[i][1] does not exist). */
int planar_lsd_search_for_triangulation(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* match12,
                                        int32_t* nmatches, double* nn_mad, double* nn12_mad);
int planar_lsd_search_for_triangulation_dev(planar_ctx* ctx, const planar_tri_line_keyframes* d_kf1, const planar_tri_line_keyframes* d_kf2,
                                            int32_t* d_match12, int32_t* d_nmatches, double* d_nn_mad, double* d_nn12_mad);
/* LSDmatcher::SearchByDescriptor(KeyFrame* pKF, KeyFrame* pKF2, vpMapLineMatches) (src/LSDmatcher.cpp:281-314): the same knn and the same
 * function of the same matches (pKF2->lineDescriptorMAD), factor 0.5; query qdx is kept when double(d1 - d0) > nn12_dist_th and its best
 * target has a map line (kf2->occupied).  match12[b][qdx]: the target whose map line vpMapLineMatches[qdx] becomes, or -1. */
int planar_lsd_search_by_descriptor_kf(planar_ctx* ctx, const planar_tri_line_keyframes* kf1, const planar_tri_line_keyframes* kf2, int32_t* match12,
                                       int32_t* nmatches);
int planar_lsd_search_by_descriptor_kf_dev(planar_ctx* ctx, const planar_tri_line_keyframes* d_kf1, const planar_tri_line_keyframes* d_kf2,
                                           int32_t* d_match12, int32_t* d_nmatches);

/* LocalMapping::CreateNewMapLines2 for cur->count current key frames (mbMonocular == false); neighbours as planar_create_new_map_points takes
 * them (entries b * max_neigh + k of `neigh`, GetBestCovisibilityKeyFrames' order).  Per neighbour: the baseline gate, SearchForTriangulation,
 * then per kept pair the 3-D segment of KeyFrame::obtain3DLine (src/KeyFrame.cc:738-747), the four depth signs, the four reprojection gates at
 * 5.991 * sigma2[octave], the zero distances and the two-sided scale test on both end points.  ComputeF12's result is unused by the reference's
 * line path and is not computed.  Kept as the reference has them: bStereo2 reads the CURRENT key frame's depth_line at the NEIGHBOUR's index
 * (:885); two lines of the current key frame may take the same idx2; an accepted idx1 is occupied for the later neighbours.
 *   n_new[b]; new_neigh / new_idx1 / new_idx2 [b][j], new_line [b][j][6], j < n_new[b]: the neighbour slot, the two line indices and the six
 *       floats handed to MapLine's constructor, widened to double as its Vector6d holds them, in creation order (k ascending, then idx1
 *       ascending).  Nothing is written at or beyond n_new[b].  The capacity is cur->stride per key frame.
 * Input the reference would fault on: n1 == 0 or a neighbour with fewer than 2 lines gives no pair; idx2 >= n1 in the bStereo2 read (past the end
 * of mvDepthLine) counts as not stereo; an octave outside the levels is taken modulo PLANAR_MAX_LEVELS; n_neigh[b] == 0 gives n_new[b] == 0.
 * `cam` is a HOST pointer in both flavours.  new MapLine, AddObservation, AddMapLine, ComputeDistinctiveDescriptors and UpdateAverageDir stay
 * with the caller (planar_distinctive_descriptors, planar_update_average_dir). */
int planar_create_new_map_lines(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_line_keyframes* cur, const planar_tri_line_keyframes* neigh,
                                const int32_t* n_neigh, int max_neigh, int32_t* n_new, int32_t* new_neigh, int32_t* new_idx1, int32_t* new_idx2,
                                double* new_line);
int planar_create_new_map_lines_dev(planar_ctx* ctx, const planar_tri_camera* cam, const planar_tri_line_keyframes* d_cur,
                                    const planar_tri_line_keyframes* d_neigh, const int32_t* d_n_neigh, int max_neigh, int32_t* d_n_new,
                                    int32_t* d_new_neigh, int32_t* d_new_idx1, int32_t* d_new_idx2, double* d_new_line);

/* MapLine::UpdateAverageDir (src/MapLine.cpp:320-367) for G groups of map lines; group g = the lines whose reference key frame has the pose
 * ref_Tcw[g], shaped like planar_update_normal_and_depth.
 *   n [G], xw6 [G][stride][6] (mWorldPos: start xyz, end xyz), valid [G][stride] or NULL (0 = no line: its outputs are left alone)
 *   ref_octave [G][stride]: the octave of the line's key line in the reference key frame (modulo PLANAR_MAX_LEVELS)
 *   obs_off [G * stride + 1], obs_ow [.][3]: camera centres (float, as GetCameraCenter gives them) of the observing key frames in observation-map
 *            order; both NULL: every line is observed by its reference key frame only
 *   scale_factors [n_levels] (mvScaleFactors) is a HOST pointer in both flavours
 *   normal [G][stride][3] (mNormalVector: the mean of the unit vectors from the camera centres to the mid point, in double),
 *   min_dist / max_dist [G][stride] (mfMinDistance / mfMaxDistance); a line without observations keeps its values */
int planar_update_average_dir(planar_ctx* ctx, int G, const int32_t* n, int stride, const double* xw6, const uint8_t* valid, const float* ref_Tcw,
                              const int32_t* ref_octave, const int32_t* obs_off, const float* obs_ow, const float* scale_factors, int n_levels,
                              double* normal, float* min_dist, float* max_dist);
int planar_update_average_dir_dev(planar_ctx* ctx, int G, const int32_t* d_n, int stride, const double* d_xw6, const uint8_t* d_valid,
                                  const float* d_ref_Tcw, const int32_t* d_ref_octave, const int32_t* d_obs_off, const float* d_obs_ow,
                                  const float* scale_factors, int n_levels, double* d_normal, float* d_min_dist, float* d_max_dist);

/* Frame::isInFrustum(MapPoint*, viewingCosLimit) (src/Frame.cc:312-367) for every local map point of B frames: fills the tracking
 * fields SearchByProjection(F, vpMapPoints, th) reads (the non-const twins of planar_map_probes' arrays).
 *   frame: Tcw, fx fy cx cy bf, min/max bounds are read (mRcw, mtcw, mOw are derived as Frame::UpdatePoseMatrices does, :301-306)
 *   log_scale_factor = Frame::mfLogScaleFactor, n_levels = mnScaleLevels (MapPoint::PredictScale, src/MapPoint.cc:419-434)
 *   valid[j] = vpMapPoints[j] usable; xw = GetWorldPos(), normal = GetNormal(), min_dist / max_dist = mfMinDistance / mfMaxDistance
 *   (GetMin/MaxDistanceInvariance apply the 0.8 / 1.2 factors, src/MapPoint.cc:390-400) */
int planar_is_in_frustum_points(planar_ctx* ctx, const planar_frame_view* frame, float log_scale_factor, int n_levels, const int32_t* n, int stride,
                                const uint8_t* valid, const float* xw, const float* normal, const float* min_dist, const float* max_dist,
                                float viewing_cos_limit, uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr, int32_t* level,
                                float* view_cos);
int planar_is_in_frustum_points_dev(planar_ctx* ctx, const planar_frame_view* d_frame, float log_scale_factor, int n_levels, const int32_t* d_n,
                                    int stride, const uint8_t* d_valid, const float* d_xw, const float* d_normal, const float* d_min_dist,
                                    const float* d_max_dist, float viewing_cos_limit, uint8_t* d_in_view, float* d_proj_x, float* d_proj_y,
                                    float* d_proj_xr, int32_t* d_level, float* d_view_cos);
/* Frame::isInFrustum(MapLine*, viewingCosLimit) (src/Frame.cc:369-438): xw6 = MapLine::GetWorldPos() (Vector6d: start xyz, end xyz),
 * normal = GetNormal() (Vector3d), level = MapLine::PredictScale (src/MapLine.cpp:381-390, NOT clamped to the pyramid, as in the reference);
 * proj[j] = {mTrackProjX1, Y1, X2, Y2}. */
int planar_is_in_frustum_lines(planar_ctx* ctx, const planar_frame_view* frame, float log_scale_factor, const int32_t* n, int stride,
                               const uint8_t* valid, const double* xw6, const double* normal, const float* min_dist, const float* max_dist,
                               float viewing_cos_limit, uint8_t* in_view, float* proj, int32_t* level, float* view_cos);
int planar_is_in_frustum_lines_dev(planar_ctx* ctx, const planar_frame_view* d_frame, float log_scale_factor, const int32_t* d_n, int stride,
                                   const uint8_t* d_valid, const double* d_xw6, const double* d_normal, const float* d_min_dist,
                                   const float* d_max_dist, float viewing_cos_limit, uint8_t* d_in_view, float* d_proj, int32_t* d_level,
                                   float* d_view_cos);

/* ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th) (src/ORBmatcher.cc:829-979), the SEARCH half: for every map point the
 * keypoint of the key frame it would be fused with (:847-951: projection, KeyFrame::IsInImage src/KeyFrame.cc:715-718, distance / viewing-angle
 * gates, MapPoint::PredictScale, KeyFrame::GetFeaturesInArea src/KeyFrame.cc:639-678, level / chi-square gates, smallest Hamming distance, TH_LOW).
 * The map edits that follow (:953-974: Replace / AddObservation / AddMapPoint) stay with the caller's map: a point's gates read only its own state
 * on entry, so they do not feed back into the search.  Batched over B key frames (LocalMapping::SearchInNeighbors fuses the same list into every
 * neighbour key frame: points_shared = 1).
 *   kf: keys_un, u_right, desc, Tcw, bounds, grid, fx fy cx cy bf, scale_factors are read (blocked is ignored)
 *   inv_level_sigma2[n_levels] = KeyFrame::mvInvLevelSigma2; log_scale_factor / n_levels = mfLogScaleFactor / mnScaleLevels
 *   usable[j] = vpMapPoints[j] != NULL && !isBad() && !IsInKeyFrame(pKF); xw / normal / desc = GetWorldPos() / GetNormal() / GetDescriptor();
 *   min_dist / max_dist = mfMinDistance / mfMaxDistance (the 0.8 / 1.2 factors of GetMin/MaxDistanceInvariance are applied here)
 *   fuse_idx[b][j] = bestIdx where bestDist <= TH_LOW (the reference then counts the point in its return value), else -1;
 *   fuse_dist[b][j] (may be NULL) = bestDist (256: no candidate); rows j >= n[b] read -1 / 256; n_fused[b] = the function's return value. */
int planar_fuse_search(planar_ctx* ctx, const planar_frame_view* kf, const float* inv_level_sigma2, float log_scale_factor, int n_levels,
                       const int32_t* n, int stride, int points_shared, const uint8_t* usable, const float* xw, const float* normal,
                       const float* min_dist, const float* max_dist, const uint8_t* desc, float th, int32_t* fuse_idx, int32_t* fuse_dist,
                       int32_t* n_fused);
int planar_fuse_search_dev(planar_ctx* ctx, const planar_frame_view* d_kf, const float* inv_level_sigma2 /* host */, float log_scale_factor, int n_levels,
                           const int32_t* d_n, int stride, int points_shared, const uint8_t* d_usable, const float* d_xw, const float* d_normal,
                           const float* d_min_dist, const float* d_max_dist, const uint8_t* d_desc, float th, int32_t* d_fuse_idx,
                           int32_t* d_fuse_dist, int32_t* d_n_fused);

/* cv::line_descriptor::KeyLine (opencv_contrib line_descriptor/descriptor.hpp), same field order, 68 bytes. */
typedef struct planar_keyline {
    float angle;
    int32_t class_id, octave;
    float pt_x, pt_y, response, size;
    float start_x, start_y, end_x, end_y;
    float s_oct_x, s_oct_y, e_oct_x, e_oct_y;
    float line_length;
    int32_t num_pixels;
} planar_keyline;

/* LSDmatcher::SearchByProjection(Frame& F, const vector<MapLine*>&, th) (src/LSDmatcher.cpp:141-211) with
 * Frame::GetLinesInArea (src/Frame.cc:491-524).
 *   keylines[b][i] mvKeylinesUn, ldesc mLdesc, blocked[i] = mvpMapLines[i] && ->Observations() > 0 on entry
 *   ml_in_view[j] = pML && !isBad() && mbTrackInView;  ml_proj[j] = {mTrackProjX1, Y1, X2, Y2};
 *   ml_level mnTrackScaleLevel, ml_view_cos mTrackViewCos, ml_desc GetDescriptor(), ml_observed Observations() > 0
 *   match[b][i] (in/out) index j of the map line stored in F.mvpMapLines[i] */
int planar_lsd_search_by_projection(planar_ctx* ctx, int B, const int32_t* n_lines, int line_stride, const planar_keyline* keylines,
                                    const uint8_t* ldesc, const uint8_t* blocked, const int32_t* n_ml, int ml_stride,
                                    const uint8_t* ml_in_view, const float* ml_proj, const int32_t* ml_level, const float* ml_view_cos,
                                    const uint8_t* ml_desc, const uint8_t* ml_observed, const float* scale_factors, int n_levels, float th,
                                    float nn_ratio, int32_t* match, int32_t* nmatches);
int planar_lsd_search_by_projection_dev(planar_ctx* ctx, int B, const int32_t* d_n_lines, int line_stride, const planar_keyline* d_keylines,
                                        const uint8_t* d_ldesc, const uint8_t* d_blocked, const int32_t* d_n_ml, int ml_stride,
                                        const uint8_t* d_ml_in_view, const float* d_ml_proj, const int32_t* d_ml_level,
                                        const float* d_ml_view_cos, const uint8_t* d_ml_desc, const uint8_t* d_ml_observed,
                                        const float* scale_factors /* host */, int n_levels, float th, float nn_ratio, int32_t* d_match,
                                        int32_t* d_nmatches);

/* LSDmatcher::Fuse(KeyFrame* pKF, const vector<MapLine*>& vpMapLines, th) (src/LSDmatcher.cpp:884-1015), the SEARCH half (:904-991): projection of both
 * end points, image-bounds / distance / viewing-angle gates, MapLine::PredictScale (src/MapLine.cpp:381-390, not clamped), KeyFrame::GetLinesInArea
 * (src/KeyFrame.cc:680-712), level gate, smallest Hamming distance, TH_LOW.  The map edits (:993-1010) stay with the caller, as for planar_fuse_search.
 *   kf: only B, Tcw, fx fy cx cy, min/max bounds and scale_factors are read (the key-point arrays may be NULL)
 *   keylines / ldesc = pKF->mvKeyLines / mLineDescriptors; usable[j] = vpMapLines[j] != NULL && !isBad(); xw6 / normal = GetWorldPos() / GetNormal()
 *   (doubles); min_dist / max_dist = mfMinDistance / mfMaxDistance.  A predicted level outside [0, n_levels) indexes mvScaleFactors out of
 *   bounds in the reference (undefined); such a line is skipped here.
 *   fuse_idx[b][j] = bestIdx where bestDist <= TH_LOW else -1; fuse_dist (may be NULL) = bestDist (INT_MAX: no candidate); rows j >= n_ml[b] read -1 / INT_MAX. */
int planar_lsd_fuse_search(planar_ctx* ctx, const planar_frame_view* kf, float log_scale_factor, int n_levels, const int32_t* n_lines, int line_stride,
                           const planar_keyline* keylines, const uint8_t* ldesc, const int32_t* n_ml, int ml_stride, int lines_shared,
                           const uint8_t* usable, const double* xw6, const double* normal, const float* min_dist, const float* max_dist,
                           const uint8_t* ml_desc, float th, int32_t* fuse_idx, int32_t* fuse_dist, int32_t* n_fused);
int planar_lsd_fuse_search_dev(planar_ctx* ctx, const planar_frame_view* d_kf, float log_scale_factor, int n_levels, const int32_t* d_n_lines, int line_stride,
                               const planar_keyline* d_keylines, const uint8_t* d_ldesc, const int32_t* d_n_ml, int ml_stride, int lines_shared,
                               const uint8_t* d_usable, const double* d_xw6, const double* d_normal, const float* d_min_dist, const float* d_max_dist,
                               const uint8_t* d_ml_desc, float th, int32_t* d_fuse_idx, int32_t* d_fuse_dist, int32_t* d_n_fused);

/* ---- the loop thread's matchers (LoopClosing::ComputeSim3, src/LoopClosing.cc:323) ----
 * pKF->GetMapPointMatches() of the key frame a planar_frame_view describes: entry i belongs to key point i, the arrays have the view's B and stride. */
typedef struct planar_kf_points {
    const uint8_t* usable;       /* [B][stride]     vpMapPoints[i] != NULL && !isBad()                                                 */
    const float* xw;             /* [B][stride][3]  GetWorldPos()                                                                      */
    const float* min_dist;       /* [B][stride]     mfMinDistance (the 0.8 of GetMinDistanceInvariance is applied here)                 */
    const float* max_dist;       /* [B][stride]     mfMaxDistance (1.2 of GetMaxDistanceInvariance; PredictScale reads it bare)         */
    const uint8_t* desc;         /* [B][stride][32] GetDescriptor()                                                                    */
} planar_kf_points;

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1106-1330), batched over B independent key-frame pairs: the
 * map points of pKF1 are searched in pKF2 under the similarity and those of pKF2 in pKF1, and a pair is stored where both searches agree.
 *   kf1, kf2: n, keys_un, desc, Tcw (GetRotation() / GetTranslation() are its blocks), bounds, grid and scale_factors are read, u_right and blocked are
 *       not; fx fy cx cy are taken from kf1 in BOTH directions, as the reference does (:1109-1112).  Both views have the same B.
 *   log_scale_factor / n_levels 1, 2 = pKF1's and pKF2's mfLogScaleFactor / mnScaleLevels (MapPoint::PredictScale(dist, pKF), src/MapPoint.cc:402-417,
 *       is called with the key frame searched).
 *   s12 [B], R12 [B][9] row-major, t12 [B][3].
 *   match12[b][i1] (in/out, stride of kf1): on entry -1 = vpMatches12[i1] is NULL; a value in [0, n2[b]) = GetIndexInKeyFrame(pKF2) of the point matched
 *       before, which takes both key point i1 of pKF1 and that key point of pKF2 out of the search; any other value = matched, the point is not in pKF2,
 *       which takes out i1 only (:1136-1146).  On exit i2 where the reference stores vpMapPoints2[i2]; every other entry keeps its value.
 *   n_found[b]: the function's return value.
 * Kept as the reference has them: 1.0 / z is a double division narrowed to float; dist3D is the norm of the CAMERA-frame point; the level gate is
 * [level - 1, level]; bestDist starts at INT_MAX, the first best in KeyFrame::GetFeaturesInArea order wins, bestDist <= TH_HIGH decides; no ratio test, no
 * orientation check.  A batch is over independent pairs; each problem has the semantics of one call on the state at entry.
 * Defined where the reference is not: n[b] is clamped to [0, stride] and n == 0 on either side gives n_found[b] = 0; a predicted level cannot leave
 * mvScaleFactors because n_levels above PLANAR_MAX_LEVELS is PLANAR_EINVAL, as are a stride above PLANAR_MAX_FRAME_KEYS, views of different B, a null
 * array and log_scale_factor == 0; s12 == 0 gives infinite or NaN coordinates, which fail the image gate (the reference does the same).
 * The _dev flavour keeps vnMatch1 / vnMatch2 in the context's scratch block. */
int planar_search_by_sim3(planar_ctx* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, float log_scale_factor1, int n_levels1,
                          const planar_frame_view* kf2, const planar_kf_points* mp2, float log_scale_factor2, int n_levels2, const float* s12, const float* R12,
                          const float* t12, float th, int32_t* match12, int32_t* n_found);
int planar_search_by_sim3_dev(planar_ctx* ctx, const planar_frame_view* d_kf1, const planar_kf_points* d_mp1, float log_scale_factor1, int n_levels1,
                              const planar_frame_view* d_kf2, const planar_kf_points* d_mp2, float log_scale_factor2, int n_levels2, const float* d_s12,
                              const float* d_R12, const float* d_t12, float th, int32_t* d_match12, int32_t* d_n_found);

/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:3739-3934), batched over B independent key-frame pairs: step 4 of
 * LoopClosing::ComputeSim3, after planar_search_by_sim3 and with its views, so the calls chain on the device.  One free VertexSim3Expmap, an EdgeSim3ProjectXYZ and
 * an EdgeInverseSim3ProjectXYZ per correspondence with g2o's numeric Jacobians, Huber with delta = sqrt(th2), Levenberg on the dense 7x7: optimize(5), classify,
 * optimize(nBad > 0 ? 10 : 5) on the inliers, classify.
 *   kf1, kf2: n, keys_un (pt and octave), Tcw, fx fy cx cy (each view's own: K1 and K2) and scale_factors (mvInvLevelSigma2[octave] = 1.0f / (sf * sf)) are read;
 *       mp1, mp2: usable and xw.  Nothing else is read and may be NULL.  Both views have the same B.
 *   S12 [B][8] (in/out, double): quaternion x, y, z, w, then t, then s: g2o::Sim3::operator[] order.  The quaternion is taken as it is (g2o does not normalise it).
 *   th2, fix_scale: th2 and bFixScale.
 *   match12[b][i] (in/out, stride of kf1), with the entry meaning planar_search_by_sim3 documents: -1 = vpMatches1[i] is NULL; a value in [0, n2[b]) = i2 =
 *       GetIndexInKeyFrame(pKF2) of the matched point; any other value = a match whose point is not in pKF2 (i2 < 0), which is skipped and keeps its value.  i is a
 *       correspondence where usable1[i] and usable2[i2] are set too.  On exit -1 exactly where the reference sets vpMatches1[i] = NULL: the outliers of the first pass
 *       (also on the early return) and those of the second.
 *   n_inliers[b]: the function's return value.   lm_iters[b][2] (may be NULL): the Levenberg iterations the two optimize calls ran.
 * Kept as the reference has them: P3D1c / P3D2c are float products widened to double; a classification reads chi2() of g2o's last evaluation, which may be a
 * rejected trial; fewer than 10 correspondences left after the first pass returns 0 with S12 untouched.
 * Defined where the reference is not: n[b] is clamped to [0, stride]; a pair without a correspondence returns 0 with S12 untouched; an octave outside the levels is
 * taken modulo PLANAR_MAX_LEVELS.  PLANAR_EINVAL: a null array, views of different B, B < 1, a stride outside [1, PLANAR_MAX_FRAME_KEYS]. */
int planar_optimize_sim3(planar_ctx* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, const planar_frame_view* kf2, const planar_kf_points* mp2,
                         double* S12, float th2, int fix_scale, int32_t* match12, int32_t* n_inliers, int32_t* lm_iters);
int planar_optimize_sim3_dev(planar_ctx* ctx, const planar_frame_view* d_kf1, const planar_kf_points* d_mp1, const planar_frame_view* d_kf2,
                             const planar_kf_points* d_mp2, double* d_S12, float th2, int fix_scale, int32_t* d_match12, int32_t* d_n_inliers, int32_t* d_lm_iters);

/* Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) (src/Optimizer.cc:2680-2991, called from
 * LoopClosing::CorrectLoop, src/LoopClosing.cc:567), batched over B independent pose graphs with ragged sizes: one VertexSim3Expmap per key frame (array index =
 * rank of mnId), an EdgeSim3 with identity information and g2o's numeric Jacobians per edge, BlockSolver_7_3 + Levenberg with setUserLambdaInit(1e-16), then the
 * SE3 recovery and the correction of points, lines and planes.  The system (7 rows per free key frame) is factored on the device in tiles of 8 key frames.
 *   g: the graphs (below).  Arrays are [B][stride] rows; what lies beyond a graph's count is not read, and the matching output rows are not written.
 *   fix_scale, iterations: bFixScale and the argument of optimize() (the reference passes 20), 0 <= iterations <= PLANAR_ESSGRAPH_MAX_ITERATIONS.
 *   sim3_out [B][kf_stride][8] (double): the optimised vertex estimates Siw in g2o::Sim3::operator[] order (quaternion x y z w, t, s).
 *   poses_out [B][kf_stride][16] (float): Tiw = [R | t / s], what SetPose receives.
 *   points_out / lines_out / planes_out: the corrected landmarks in the layout of their inputs, correctedSwr.map(Srw.map(P)) in double for points and for both end
 *       points of a line, the float cv::Mat algebra with its two d < 0 sign flips for planes.  May be NULL where the input array is NULL.
 *   info [B][5] (double): Levenberg iterations run, trials, final chi2, final lambda, status (PLANAR_ESSGRAPH_*).
 * UpdateNormalAndDepth, ComputeDistinctiveDescriptors, UpdateAverageDir and UpdateCoefficientsAndPoints stay with the caller, as does every map edit of CorrectLoop.
 * Preconditions taken from the reference: no bad key frame among the inputs (the reference dereferences a null vertex there), landmarks not bad.
 * Launch budget: iterations + PLANAR_ESSGRAPH_EXTRA_TRIALS trial slots are enqueued with no host decision between them; an iteration costs one and so does each
 * rejected trial.  A graph whose protocol has not ended by then reports PLANAR_ESSGRAPH_RUNNING and the estimates of its last accepted trial.
 * PLANAR_EINVAL (nothing written): a null required argument, B < 1, kf_stride outside [1, PLANAR_ESSGRAPH_MAX_KF], edge_stride < 1, a Sim3 array without its mask,
 * a landmark array without its count, references, stride or output, iterations out of range; and, in the host flavour, n_kf[b] outside [1, kf_stride], n_edges[b]
 * outside [0, edge_stride], a fixed index outside [0, n_kf), an edge naming a vertex outside [0, n_kf) or the same vertex twice, a landmark count beyond its stride
 * or a reference key frame outside [0, n_kf).  The _dev flavour cannot read those without a copy: such a graph gets status PLANAR_ESSGRAPH_INVALID and no other
 * output, the other graphs of the batch run, and a landmark with a reference out of range is left unwritten. */
#define PLANAR_ESSGRAPH_MAX_KF 256          /* key frames per graph */
#define PLANAR_ESSGRAPH_MAX_ITERATIONS 100
#define PLANAR_ESSGRAPH_EXTRA_TRIALS 20     /* trial slots beyond one per iteration */
#define PLANAR_ESSGRAPH_LOOP 0              /* edge kind: loop connection (:2748-2774), both measurement ends from the start estimates */
#define PLANAR_ESSGRAPH_NORMAL 1            /* edge kind: spanning tree, old loop edge, covisibility (:2777-2866), each end from noncorrected where present */
#define PLANAR_ESSGRAPH_RUNNING 0           /* status: the launch budget ran out first */
#define PLANAR_ESSGRAPH_MAX_ITERATIONS_RUN 1 /* status: optimize() ran all its iterations */
#define PLANAR_ESSGRAPH_TERMINATED 2        /* status: ten rejected trials, rho == 0 or the _nBad >= 3 stop */
#define PLANAR_ESSGRAPH_NOTHING 3           /* status: no free vertex or no edge */
#define PLANAR_ESSGRAPH_INVALID (-1)        /* status (_dev flavour): see PLANAR_EINVAL above */
typedef struct planar_essgraph {
    int32_t B, kf_stride, edge_stride, point_stride, line_stride, plane_stride;
    const int32_t* n_kf;               /* [B] */
    const float* poses;                /* [B][kf_stride][16] Tcw of GetPose(), row-major */
    const double* corrected;           /* [B][kf_stride][8] CorrectedSim3 in g2o::Sim3::operator[] order, or NULL */
    const uint8_t* corrected_mask;     /* [B][kf_stride] non-zero where the key frame is in CorrectedSim3 */
    const double* noncorrected;        /* NonCorrectedSim3, the same way, or NULL */
    const uint8_t* noncorrected_mask;
    const int32_t* fixed;              /* [B] index of pLoopKF */
    const int32_t* n_edges;            /* [B] */
    const int32_t* edges;              /* [B][edge_stride][3]: vertex 0, vertex 1, kind; planar_adapter::essential_graph_edges (planar_adapters.hpp) builds the reference's list */
    const int32_t* n_points;  const float* points;  const int32_t* point_ref;   /* [B], [B][point_stride][3], [B][point_stride] reference key-frame index; or NULL */
    const int32_t* n_lines;   const double* lines;  const int32_t* line_ref;    /* [B][line_stride][6] start and end point */
    const int32_t* n_planes;  const float* planes;  const int32_t* plane_ref;   /* [B][plane_stride][4] */
} planar_essgraph;
int planar_optimize_essential_graph(planar_ctx* ctx, const planar_essgraph* g, int fix_scale, int iterations, double* sim3_out, float* poses_out, float* points_out,
                                    double* lines_out, float* planes_out, double* info);
int planar_optimize_essential_graph_dev(planar_ctx* ctx, const planar_essgraph* d_g, int fix_scale, int iterations, double* d_sim3_out, float* d_poses_out,
                                        float* d_points_out, double* d_lines_out, float* d_planes_out, double* d_info);

/* Sim3Solver (src/Sim3Solver.cc), batched over B independent key-frame pairs: step 2 of LoopClosing::ComputeSim3 (src/LoopClosing.cc:274-301), between
 * planar_search_by_bow_kf and planar_search_by_sim3 and on the views of the latter, so the calls chain on the device.  Each pair has the semantics of one
 * Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale), SetRansacParameters(prob, min_inliers, max_its) and ONE iterate(n_iterations, bNoMore, vbInliers, nInliers); the
 * solver's state is passed in and out, so a later call is the same solver's next iterate.
 *   kf1, kf2: n, keys_un (the octave), Tcw, fx fy cx cy (each view's own: mK1 and mK2) and scale_factors (mvLevelSigma2[octave] = sf * sf) are read; mp1, mp2:
 *       usable and xw.  Nothing else is read and may be NULL.  Both views have the same B.
 *   match12[b][i1] (stride of kf1; not written, and not the array match12_inl), with the entry meaning planar_search_by_sim3 documents: -1 = vpMatched12[i1] is
 *       NULL; a value in [0, n2[b]) = i2 = GetIndexInKeyFrame(pKF2); any other value = a point that is not in pKF2, skipped as indexKF2 < 0 is (:82).  i1 is a
 *       correspondence where usable1[i1] and usable2[i2] are set too.  Correspondences are numbered in ascending i1: that order decides what a draw picks.
 *   prob, min_inliers, max_its, fix_scale: the arguments of SetRansacParameters and bFixScale.  n_iterations: that of iterate.
 *   seeds[b]: the pair's draws are glibc's rand() after srand(seeds[b]).  The reference's stream is process-global and shared by every solver; a stream per item is
 *       the rule planar_is_line_good set.  Iteration k (counted from the solver's construction) uses draws 3k .. 3k + 2, so the place in the stream follows from
 *       its_done.  A draw is DUtils::Random::RandomInt(0, size - 1) = int(((double)rand() / ((double)RAND_MAX + 1.0)) * size) (Random.cpp:47-50), and the three picks
 *       follow the swap-with-back rule of :170-181.
 *   State of the solver, [B] each, in/out (zero for a new solver): its_done = mnIterations; best_inliers = mnBestInliers; best_R [B][9], best_t [B][3], best_s [B] =
 *       mBestRotation, mBestTranslation, mBestScale, written whenever mnInliersi >= mnBestInliers, so the last such iteration wins.
 *   found[b]: 1 where the reference returns a non-empty mBestT12.  no_more[b]: bNoMore.  n_inliers[b]: nInliers.  inliers[b][i1] (stride of kf1): vbInliers.
 *   R12 [B][9] row-major, t12 [B][3], s12 [B]: GetEstimatedRotation / Translation / Scale of a pair that was found, in the layout planar_search_by_sim3 takes; zero
 *       where found is 0.
 *   match12_inl[b][i1] (may be NULL): match12 with every entry that is no inlier set to -1, as LoopClosing.cc:313-318 builds vpMapPointMatches before SearchBySim3.
 *   S12 [B][8] (may be NULL, double): g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) as LoopClosing.cc:325 builds gScm, in
 *       g2o::Sim3::operator[] order (quaternion x y z w, t, s): what planar_optimize_sim3 takes.  Eigen's matrix-to-quaternion rule; that constructor does not
 *       normalise (sim3.h:64-67).  Zero where found is 0.
 * mRansacMaxIts = max(1, min(ceil(log(1 - prob) / log(1 - pow((float)min_inliers / N, 3))), max_its)), and 1 where min_inliers == N, is host libm arithmetic that a
 * ceil can tip: the library evaluates the reference's expression on the host for every N, keeps the table in the context per (prob, min_inliers, max_its) and the
 * kernel reads it.  Where the double is no int (NaN, overflow) the reference's conversion is undefined; x86-64 gives INT_MIN, hence 1, and so does the table.
 * Kept as the reference has them: iterate clears vbInliers and nInliers on every call; N < mRansacMinInliers is tested before a draw; the rotation angle is
 * atan2(norm(vec), w) in double; vec = 2 * ang * vec / norm(vec) is NaN when the imaginary part of the eigenvector is exactly zero (two identical point sets),
 * every comparison of CheckInliers then fails and the hypothesis has 0 inliers; 1 / z has no positivity gate; mvnMaxError1 / 2 are std::vector<size_t>
 * (Sim3Solver.h:78-79), so 9.210 * sigma2 is a double product TRUNCATED to an integer and compared as a float; ms12i = nom / den is a double quotient narrowed to
 * float.  A hypothesis of 0 inliers still replaces the best of a new solver (0 >= 0).
 * Defined where the reference is not: n[b] is clamped to [0, stride]; an octave outside the levels is taken modulo PLANAR_MAX_LEVELS; N < max(min_inliers, 3) gives
 * no_more = 1, found = 0 and leaves the state untouched; a negative its_done counts as 0.
 * PLANAR_EINVAL, before any device call: a null required array, views of different B, B < 1, a stride outside [1, PLANAR_MAX_FRAME_KEYS], n_iterations < 1, max_its
 * outside [1, PLANAR_HORN_MAX_ITS] (the draws and counts of one call are kept on chip; the reference passes 300), prob outside (0, 1).
 * The _dev flavour keeps the correspondences of key frames above 512 key points in the context's scratch block. */
#define PLANAR_HORN_MAX_ITS 1024
int planar_horn_ransac(planar_ctx* ctx, const planar_frame_view* kf1, const planar_kf_points* mp1, const planar_frame_view* kf2, const planar_kf_points* mp2,
                       const int32_t* match12, double prob, int min_inliers, int max_its, int fix_scale, int n_iterations, const uint32_t* seeds, int32_t* its_done,
                       int32_t* best_inliers, float* best_R, float* best_t, float* best_s, int32_t* found, int32_t* no_more, int32_t* n_inliers, uint8_t* inliers,
                       float* R12, float* t12, float* s12, int32_t* match12_inl, double* S12);
int planar_horn_ransac_dev(planar_ctx* ctx, const planar_frame_view* d_kf1, const planar_kf_points* d_mp1, const planar_frame_view* d_kf2, const planar_kf_points* d_mp2,
                           const int32_t* d_match12, double prob, int min_inliers, int max_its, int fix_scale, int n_iterations, const uint32_t* d_seeds,
                           int32_t* d_its_done, int32_t* d_best_inliers, float* d_best_R, float* d_best_t, float* d_best_s, int32_t* d_found, int32_t* d_no_more,
                           int32_t* d_n_inliers, uint8_t* d_inliers, float* d_R12, float* d_t12, float* d_s12, int32_t* d_match12_inl, double* d_S12);

/* PnPsolver (src/PnPsolver.cc: EPnP inside a RANSAC), batched over B independent (lost frame, candidate key frame) problems: step 3 of Tracking::Relocalization
 * (src/Tracking.cc:2554-2698), between planar_search_by_bow, whose match array it takes as written, and planar_pose_opt.  Each problem has the semantics of one
 * PnPsolver(F, vpMapPointMatches), SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2) and ONE iterate(n_iterations, bNoMore, vbInliers, nInliers);
 * the solver's state is passed in and out, so a later call is the same solver's next iterate.
 *   fr: the lost frames: n, keys_un (pt and octave), fx fy cx cy and scale_factors (mvLevelSigma2[octave] = sf * sf) are read; nothing else is and may be NULL.
 *   kf_usable [B][kf_stride], kf_xw [B][kf_stride][3]: the candidate's map points by key-frame feature: whether it holds a point that is not bad, and GetWorldPos().
 *   match [B][fr->stride]: exactly what planar_search_by_bow writes: the key-frame feature matched to key point i of the frame, or -1.  i is a correspondence where
 *       0 <= match[i] < kf_stride and kf_usable[match[i]] is set.  Correspondences are numbered in ascending i (mvKeyPointIndices): that order decides what a draw picks.
 *   seeds[b]: the problem's draws are glibc's rand() after srand(seeds[b]) (the reference's stream is process-global; a stream per item is the rule
 *       planar_is_line_good set).  Iteration k, counted from the solver's construction, uses draws 4k .. 4k + 3, so the place in the stream follows from its_done.  A draw
 *       is DUtils::Random::RandomInt(0, size - 1) and the four picks follow the swap-with-back rule of :191-201.
 *   State of the solver, in/out (zero for a new solver): its_done [B] = mnIterations; best_inliers [B] = mnBestInliers; best_set [B][fr->stride] = mvbBestInliers, by key
 *       point of the frame (only entries of correspondences are ever written); best_Tcw [B][16] = mBestTcw.  Refine()'s outcome on the best set is no state: it
 *       depends on that set alone and is computed again when a later call first needs it.
 *   found[b]: 1 where the reference returns a non-empty matrix.  no_more[b]: bNoMore.  n_inliers[b]: nInliers.  inliers[b][i]: vbInliers, by key point of the frame; the
 *       first n[b] entries of a row are written (zero unless found), the rest is left alone.  Tcw [B][16] row-major float: mRefinedTcw or mBestTcw, mRi / mti narrowed as
 *       convertTo(CV_32F) does; zero where found is 0.
 * mRansacMinInliers = max(int(N * epsilon), min_inliers, min_set), epsilon = max(epsilon, (float)mRansacMinInliers / N) and mRansacMaxIts = max(1, min(ceil(log(1 - prob)
 * / log(1 - pow(epsilon, 3))), max_its)) (the exponent is 3 although the minimal set is 4), 1 where mRansacMinInliers == N, are host libm arithmetic: the library
 * evaluates the reference's expressions on the host for every N, keeps the table in the context per (prob, min_inliers, max_its, epsilon) and the kernel reads it.
 * Kept as the reference has them: the loop runs while mnIterations < mRansacMaxIts OR this call has run fewer than n_iterations, so the first call of a solver runs
 * max(mRansacMaxIts, n_iterations) iterations unless a Refine returns, and find() is n_iterations = mRansacMaxIts; N < mRansacMinInliers gives no_more before any
 * draw; the best is replaced on strict >; Refine() runs whenever mnInliersi >= mRansacMinInliers, on the best set, and returns on strict mnInliersi >
 * mRansacMinInliers; at the end the best is returned when mnIterations >= mRansacMaxIts and mnBestInliers >= mRansacMinInliers (found = 1 with no_more = 1);
 * maxError = sigma2 * th2 is a float product; CheckInliers narrows Xc, Yc, 1 / Zc to float, has ue, ve in double and distX, distY, error2 in float, and no positivity
 * gate on Zc.  EPnP itself runs in double through OpenCV's JacobiSVD and SVBackSubst as restated in csrc/epnp_arith.h, the RNG(0x12345678) tail for a zero singular
 * value included (coplanar sets reach it).  qr_solve's early return on a singular A leaves X as it was; the reference's X is uninitialised there, here it is the
 * previous step's or zero.
 * Defined where the reference is not: n[b] is clamped to [0, stride]; an octave outside the levels is taken modulo PLANAR_MAX_LEVELS; a negative its_done counts as 0 and one above
 * PLANAR_PNP_MAX_ITS_DONE as that value (one thread walks 4 * its_done values of the stream before the call's first draw, about 10 ns each, so a solver resumed
 * after thousands of iterations pays for them again on every call).
 * PLANAR_EINVAL, before any device call: a null required array, B < 1, fr->stride or kf_stride outside [1, PLANAR_MAX_FRAME_KEYS], n_iterations or max_its outside
 * [1, PLANAR_PNP_MAX_ITS] (the draws and counts of one call are kept on chip; the reference passes 300 and 5), prob outside (0, 1), min_set != 4 (the only value the
 * reference passes; EPnP on another minimal set is simply not built).
 * The _dev flavour keeps the correspondences of frames above 512 key points in the context's scratch block. */
#define PLANAR_PNP_MAX_ITS 1024
#define PLANAR_PNP_MAX_ITS_DONE (1 << 20)
int planar_pnp_ransac(planar_ctx* ctx, const planar_frame_view* fr, const uint8_t* kf_usable, const float* kf_xw, int kf_stride, const int32_t* match, double prob,
                      int min_inliers, int max_its, int min_set, float epsilon, float th2, int n_iterations, const uint32_t* seeds, int32_t* its_done,
                      int32_t* best_inliers, uint8_t* best_set, float* best_Tcw, int32_t* found, int32_t* no_more, int32_t* n_inliers, uint8_t* inliers, float* Tcw);
int planar_pnp_ransac_dev(planar_ctx* ctx, const planar_frame_view* d_fr, const uint8_t* d_kf_usable, const float* d_kf_xw, int kf_stride, const int32_t* d_match,
                          double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2, int n_iterations, const uint32_t* d_seeds,
                          int32_t* d_its_done, int32_t* d_best_inliers, uint8_t* d_best_set, float* d_best_Tcw, int32_t* d_found, int32_t* d_no_more,
                          int32_t* d_n_inliers, uint8_t* d_inliers, float* d_Tcw);

/* ORBmatcher(nn_ratio, check_orientation)::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (src/ORBmatcher.cc:526-659), batched
 * over B independent key-frame pairs (LoopClosing::ComputeSim3 calls it with ORBmatcher(0.75, true), once per candidate).  Both FeatureVectors are passed as one
 * node id per feature (-1: in no node), as planar_search_by_bow takes them.  Probes are key frame 1's features in (node ascending, feature index ascending)
 * order, which is the order of the reference's walk over the common nodes.
 *   usable1[i] / usable2[i] = GetMapPointMatches()[i] != NULL && !isBad();  keys_un1 / keys_un2 = mvKeysUn (the angle is read);  desc = mDescriptors
 *   match12[b][idx1] (stride1) = idx2 where the reference stores vpMapPoints2[idx2], else -1; entries at and beyond n1[b] keep their value
 *   nmatches[b]: the function's return value.
 * Kept as the reference has them: both sides need a usable map point; vbMatched2 is set at once and seen by later probes; bestDist1 < TH_LOW is strict here
 * (the (KeyFrame*, Frame&) overload has <=); the float ratio test; the orientation histogram on the mvKeysUn angles of both sides, whose removal clears the
 * match but not vbMatched2.  n[b] is clamped to [0, stride]; n == 0 on either side gives no match.  PLANAR_EINVAL: a null array, B < 1, a stride outside
 * [1, PLANAR_MAX_FRAME_KEYS]. */
int planar_search_by_bow_kf(planar_ctx* ctx, int B, const int32_t* n1, int stride1, const int32_t* node1, const uint8_t* usable1, const planar_keypoint* keys_un1,
                            const uint8_t* desc1, const int32_t* n2, int stride2, const int32_t* node2, const uint8_t* usable2, const planar_keypoint* keys_un2,
                            const uint8_t* desc2, float nn_ratio, int check_orientation, int32_t* match12, int32_t* nmatches);
int planar_search_by_bow_kf_dev(planar_ctx* ctx, int B, const int32_t* d_n1, int stride1, const int32_t* d_node1, const uint8_t* d_usable1,
                                const planar_keypoint* d_keys_un1, const uint8_t* d_desc1, const int32_t* d_n2, int stride2, const int32_t* d_node2,
                                const uint8_t* d_usable2, const planar_keypoint* d_keys_un2, const uint8_t* d_desc2, float nn_ratio, int check_orientation,
                                int32_t* d_match12, int32_t* d_nmatches);

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th)
 * (src/ORBmatcher.cc:294-407): the loop map points projected into the current key frame under the similarity Scw, batched over B (key frame, Scw, list)
 * problems.  The list has no length limit (mvpLoopMapPoints is the union over a loop key frame's covisibles); points_shared = 1: one list [1][stride] for all.
 *   kf: n, keys_un, desc, bounds, grid, fx fy cx cy and scale_factors are read; blocked[b][idx] = vpMatched[idx] != NULL on entry (NULL = none); u_right and Tcw
 *       are not read.  Scw [B][16] row-major.  log_scale_factor / n_levels = pKF->mfLogScaleFactor / mnScaleLevels.
 *   usable[j] = !vpPoints[j]->isBad(); found[b][j] (always [B][stride]; NULL = none) = spAlreadyFound.count(vpPoints[j]), fixed on entry;
 *   xw / normal / desc = GetWorldPos() / GetNormal() / GetDescriptor(); min_dist / max_dist = mfMinDistance / mfMaxDistance (0.8 / 1.2 applied here).
 *   kf_match[b][idx] (in/out, stride of kf) = iMP where the reference stores vpMatched[idx] = vpPoints[iMP]; untouched where nothing new is stored.
 *   nmatches[b]: the function's return value.
 * Kept as the reference has them: scw = (float)sqrt(row0.dot(row0)), Rcw = sRcw / scw, tcw = t / scw, Ow = -Rcw.t() * tcw; the gates z < 0, IsInImage,
 * 0.8 * min / 1.2 * max, PO.dot(Pn) < 0.5 * dist in double; 1 / z in float; radius = th * mvScaleFactors[level] with an int th; a candidate whose vpMatched
 * entry is non-null NOW is skipped, so a match written earlier in the call blocks its key point; bestDist starts at 256 and bestDist <= TH_LOW decides; no
 * ratio test, no orientation check.  Each problem has the semantics of one call on the state at entry.
 * Defined where the reference is not: n[b] is clamped to [0, stride]; scw == 0 gives NaN coordinates, which fail the image gate: nothing matches.
 * PLANAR_EINVAL: a null array, B < 1, kf->stride outside [1, PLANAR_MAX_FRAME_KEYS], stride < 1, n_levels outside [1, PLANAR_MAX_LEVELS] (a predicted level
 * could leave mvScaleFactors), log_scale_factor == 0. */
int planar_search_by_projection_sim3(planar_ctx* ctx, const planar_frame_view* kf, const float* Scw, float log_scale_factor, int n_levels, const int32_t* n, int stride,
                                     int points_shared, const uint8_t* usable, const uint8_t* found, const float* xw, const float* normal, const float* min_dist,
                                     const float* max_dist, const uint8_t* desc, int th, int32_t* kf_match, int32_t* nmatches);
int planar_search_by_projection_sim3_dev(planar_ctx* ctx, const planar_frame_view* d_kf, const float* d_Scw, float log_scale_factor, int n_levels, const int32_t* d_n,
                                         int stride, int points_shared, const uint8_t* d_usable, const uint8_t* d_found, const float* d_xw, const float* d_normal,
                                         const float* d_min_dist, const float* d_max_dist, const uint8_t* d_desc, int th, int32_t* d_kf_match, int32_t* d_nmatches);

/* ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint) (src/ORBmatcher.cc:981-1104):
 * the loop map points fused into a corrected key frame (LoopClosing::SearchAndFuse, ORBmatcher(0.8), th = 4), batched over B key frames.  Unlike
 * planar_fuse_search this entry returns the WHOLE outcome, because the reference's edits feed back inside the call: AddMapPoint (:1097) fills a slot that a
 * later point then finds occupied (:1088).  A point's best key point does not depend on that, so every point is evaluated on its own and the lowest j that
 * chose an empty slot owns it.
 *   kf, Scw, log_scale_factor, n_levels, the point arrays and points_shared: as planar_search_by_projection_sim3 (kf->blocked is not read);
 *   usable[b][j] (always [B][stride]) = !isBad() && !pKF->GetMapPoints().count(vpPoints[j]), the set taken on entry;
 *   kf_slot[b][idx] (stride of kf) = pKF->GetMapPoint(idx) on entry: 0 NULL, 1 a map point that is not bad, 2 a bad map point.
 *   fuse_idx[b][j] = the slot chosen (bestDist <= TH_LOW), or -1 where nothing was fused.
 *   owner[b][j], written where fuse_idx[b][j] >= 0 and untouched elsewhere:
 *       -1       the slot held a point on entry: kf_slot 1 means vpReplacePoint[j] = that point; kf_slot 2 means nothing is recorded, yet it counts in nFused
 *       j        the point took the empty slot: AddObservation / AddMapPoint
 *       j' < j   an earlier point of this call took it: vpReplacePoint[j] = vpPoints[j']
 *   n_fused[b]: the function's return value.  Entries at and beyond n[b] keep their value.
 * Kept as the reference has them: the gates of the projection search minus "already matched"; 1.0 / z is a double division narrowed to float; bestDist starts at
 * INT_MAX; no chi-square or stereo gates.  A batch is over INDEPENDENT maps and each problem has the semantics of one call on the state at entry:
 * LoopClosing::SearchAndFuse applies the replacements between the key frames of one map, which is the caller's business, as with planar_fuse_search.
 * Undefined input and PLANAR_EINVAL as for planar_search_by_projection_sim3. */
int planar_fuse_sim3(planar_ctx* ctx, const planar_frame_view* kf, const float* Scw, const uint8_t* kf_slot, float log_scale_factor, int n_levels, const int32_t* n,
                     int stride, int points_shared, const uint8_t* usable, const float* xw, const float* normal, const float* min_dist, const float* max_dist,
                     const uint8_t* desc, float th, int32_t* fuse_idx, int32_t* owner, int32_t* n_fused);
int planar_fuse_sim3_dev(planar_ctx* ctx, const planar_frame_view* d_kf, const float* d_Scw, const uint8_t* d_kf_slot, float log_scale_factor, int n_levels,
                         const int32_t* d_n, int stride, int points_shared, const uint8_t* d_usable, const float* d_xw, const float* d_normal, const float* d_min_dist,
                         const float* d_max_dist, const uint8_t* d_desc, float th, int32_t* d_fuse_idx, int32_t* d_owner, int32_t* d_n_fused);

/* PlaneMatcher::SearchMapByCoefficients(Frame&, const vector<MapPlane*>&) (src/PlaneMatcher.cpp:10-66) with
 * Frame::ComputePlaneWorldCoeff (src/Frame.cc:815-820) and PointDistanceFromPlane (:67-79).
 *   pl_coef [B][pl_stride][4]  mvPlaneCoefficients[i] (camera frame)      Tcw [B][16]
 *   mp_*: the map planes seen by frame b (b = 0 for every frame when map_shared != 0):
 *     mp_valid !isBad(); mp_coef GetWorldPos() [4]; mp_pts mvPlanePoints xyz float, [.][mp_stride][pts_stride][3]
 *   th[4] = {dTh, aTh, verTh, parTh} (PlaneMatcher ctor, include/PlaneMatcher.h:19)
 *   match / ver / par [B][pl_stride] (in/out): index of the map plane stored in mvpMapPlanes[i] /
 *   mvpVerticalPlanes[i] / mvpParallelPlanes[i]; untouched where the reference does not assign. */
int planar_plane_search_by_coefficients(planar_ctx* ctx, int B, const int32_t* n_planes, int pl_stride, const float* pl_coef,
                                        const float* Tcw, int map_shared, const int32_t* n_mp, int mp_stride, const uint8_t* mp_valid,
                                        const float* mp_coef, const int32_t* mp_npts, int pts_stride, const float* mp_pts,
                                        const float* th, int32_t* match, int32_t* ver, int32_t* par, int32_t* nmatches);
int planar_plane_search_by_coefficients_dev(planar_ctx* ctx, int B, const int32_t* d_n_planes, int pl_stride, const float* d_pl_coef,
                                            const float* d_Tcw, int map_shared, const int32_t* d_n_mp, int mp_stride,
                                            const uint8_t* d_mp_valid, const float* d_mp_coef, const int32_t* d_mp_npts, int pts_stride,
                                            const float* d_mp_pts, const float* th /* host */, int32_t* d_match, int32_t* d_ver,
                                            int32_t* d_par, int32_t* d_nmatches);

/* ---- line extractor (replaces LineSegment::ExtractLineSegment, src/LSDextractor.cpp:12-39 /
 *      include/LSDextractor.h:344-352: cv::line_descriptor::LSDDetector::detect (1 octave, LSD_REFINE_ADV) +
 *      sort by response, keep max_lines + cv::line_descriptor::BinaryDescriptor::compute + line equations) --- */
typedef struct planar_lsd planar_lsd;
int planar_lsd_create(planar_ctx* ctx, int width, int height, int max_batch, planar_lsd** out);
void planar_lsd_destroy(planar_lsd* lsd);
int planar_lsd_max_segments(void);   /* raw LSD segments kept per frame before the top-`max_lines` cut (2048) */
int planar_lsd_scaled_size(planar_lsd* lsd, int* w, int* h);   /* the 0.8x working resolution */
int planar_lsd_set_tie_order(planar_lsd* lsd, int tie_order);   /* 0 (default): libstdc++ std::sort order, 1: raster order */
/* 1: the NFA stage (rect_improve) only for the regions that can end among the max_lines key lines LineSegment::ExtractLineSegment keeps (reference src/LSDextractor.cpp:17-27:
 * sort by response, resize to 40): the longest regions first, the rest only where that cannot settle the frame (fewer than max_lines + 1 accepted, a shorter region could still
 * reach the kept ones, or equal responses among them).  Key lines, descriptors and equations are those of the default mode, bit for bit; what planar_lsd_read_stage(.., 3, ..) returns
 * (the raw segments) is then only the part that was evaluated.  0 (default): every region. */
int planar_lsd_set_top_only(planar_lsd* lsd, int enable);
/* gray     : B frames of 8-bit gray (the `img` argument), pitch / frame_stride in bytes
 * max_lines: lsdNFeatures (40 in the reference); per-frame stride of the outputs
 * keylines : [B][max_lines] cv::line_descriptor::KeyLine records   ldesc: [B][max_lines][32] LBD bytes
 * line_eq  : [B][max_lines][3] keylineFunctions (sp x ep, normalised)   n_lines: [B] keylines.size()
 * Pixels of equal gradient bin are visited in the order libstdc++'s std::sort leaves them, as in the reference library
 * (lsd.cpp sorts with std::sort); planar_lsd_set_tie_order(lsd, 1) selects raster order inside a bin instead (the original
 * LSD's list order). */
int planar_lsd_extract(planar_lsd* lsd, const uint8_t* gray, int B, int pitch, int64_t frame_stride, int max_lines, planar_keyline* keylines,
                       uint8_t* ldesc, double* line_eq, int32_t* n_lines);
int planar_lsd_extract_dev(planar_lsd* lsd, const uint8_t* d_gray, int B, int pitch, int64_t frame_stride, int max_lines,
                           planar_keyline* d_keylines, uint8_t* d_ldesc, double* d_line_eq, int32_t* d_n_lines);
/* The same work as planar_lsd_extract_dev in two enqueues on the context's stream, for callers that overlap the sequential
 * detector with other stages: preprocess = Gaussians, 0.8x resample + gradients, Sobel, pixel ordering (throughput kernels);
 * detect = region growing / NFA, KeyLines, LBD.  planar_lsd_detect_dev returns PLANAR_ESTATE without a matching preprocess. */
int planar_lsd_preprocess_dev(planar_lsd* lsd, const uint8_t* d_gray, int B, int pitch, int64_t frame_stride);
int planar_lsd_detect_dev(planar_lsd* lsd, int B, int max_lines, planar_keyline* d_keylines, uint8_t* d_ldesc, double* d_line_eq, int32_t* d_n_lines);
/* Per-frame status of the last detect / extract call (synchronises the context's stream).  n_lines is never negative: a frame whose workspace overflowed (more
 * regions / segments than it holds) or whose std::sort order could not be reproduced delivers ZERO lines, and this call (which planar_lsd_extract makes itself)
 * returns PLANAR_ECAPACITY naming the frame; planar_last_error() has the reason.  The device entry points never synchronise: their callers check when they read back. */
int planar_lsd_check(planar_lsd* lsd, int B);
/* diagnostics (tests / profiling; stage 5 = cycle counters, see lsd.hip): stage 0 level-line angle float deg [w*h] (-1024 undefined), 1 squared gradient u32 [w*h],
 * 2 visiting order int32 (returns n), 3 raw segments 40 B each {x1,y1,x2,y2 float; width,p,nfa double} (returns count),
 * 4 number of grown regions int32[1], 7 rare paths of the region kernel int32[2]: regions grown again by refine(), rounds of reduce_region_radius */
int planar_lsd_read_stage(planar_lsd* lsd, int frame, int stage, void* out, int64_t out_bytes);
/* Per-launch timing with HIP events on the context stream (bench.py's roofline leg), as planar_peac_set_profiling: get_profile synchronises and returns the
 * summed milliseconds of the recorded calls, total_ms[4] = preprocessing (blurs, gradient, Sobel), lsd_sort, lsd_detect, the rest, their number, and resets. */
int planar_lsd_set_profiling(planar_lsd* lsd, int enable);
int planar_lsd_get_profile(planar_lsd* lsd, double* total_ms, int64_t* calls);
#ifdef PLANAR_TEST_HOOKS
/* test hook, exported by the TEST build only (libplanar_hip_paranoid.so, `make paranoid`): device emulation of libstdc++ std::sort with the sort_lines_by_response
 * comparator (include/auxiliar.h:43-48) on raw keys */
int planar_debug_std_sort_desc(planar_ctx* ctx, float* keys, int32_t* perm, int n);
#endif

/* ---- plane extractor (replaces PlaneDetection::readDepthImage + runPlaneDetection,
 *      src/PlaneExtractor.cpp:26-65 / include/PlaneExtractor.h:36-56, i.e. ahc::PlaneFitter::run with
 *      PlanarSLAM's defaults, include/peac/AHCPlaneFitter.hpp:154-158,211) ------------------------- */
typedef struct planar_peac planar_peac;
int planar_peac_create(planar_ctx* ctx, int width, int height, int max_batch, planar_peac** out);
void planar_peac_destroy(planar_peac* peac);
int planar_peac_max_planes(void);   /* per-frame stride of `planes` (128) */
/* depth  : B frames of 16-bit depth (cv::Mat CV_16U as passed to readDepthImage), pitch / frame stride in PIXELS
 * fx..cy : K.at<float>(0,0), (1,1), (0,2), (1,2);   depth_factor : kScaleFactor (mDepthMapFactor, 1/5000)
 * labels : [B][H*W] int32, plane id of every pixel in the order of plane_vertices_ (= extractedPlanes), -1 = none;
 *          plane_vertices_[i] is the raster-ordered list of pixels with label i (src/Frame.cc:652-656)
 * planes : [B][max_planes][8] doubles: N, normal[3], center[3], mse of extractedPlanes[i] (src/Frame.cc:663-669)
 * n_planes : [B] plane_num_                                                                             */
int planar_peac_segment(planar_peac* peac, const uint16_t* depth, int B, int pitch_px, int64_t frame_stride_px, float fx, float fy,
                        float cx, float cy, float depth_factor, int32_t* labels, double* planes, int32_t* n_planes);
int planar_peac_segment_dev(planar_peac* peac, const uint16_t* d_depth, int B, int pitch_px, int64_t frame_stride_px, float fx, float fy,
                            float cx, float cy, float depth_factor, int32_t* d_labels, double* d_planes, int32_t* d_n_planes);
/* Synchronises and returns PLANAR_ECAPACITY if any of the last B frames overflowed an internal capacity
 * (more than max_planes planes, flood-fill queue, neighbour pool); the host-pointer entry point calls it itself. */
/* Debug aids (tools/peac_ab.py; not part of the drop-in surface): workspace layout {frame_bytes, NB, NB2, off_stats, off_geo, off_N, off_dsp, off_dss,
 * off_rid, off_nouse, off_hand, off_crec} and a raw read of one frame's workspace after the last call. */
int planar_peac_debug_layout(planar_peac* peac, int64_t* out /* [12] */);
int planar_peac_debug_read(planar_peac* peac, int frame, int64_t offset, int64_t bytes, void* out);
int planar_peac_check(planar_peac* peac, int B);
/* A/B aid (tools/peac_ab.py and the tests; nothing in the product calls it, and no environment variable selects a kernel): clustering 0 = product (fast attempt +
 * exact redo), 1 = exact heap only (anything else: PLANAR_EINVAL); wide_below = batch size up to which the refinement runs 1024 threads per frame (< 0: keep).
 * Every variant returns the same labels and planes. */
int planar_peac_set_variant(planar_peac* peac, int clustering, int wide_below);
/* Per-launch timing with HIP events on the context stream (bench.py's roofline leg), as planar_orb_set_profiling: get_profile synchronises and returns the
 * summed milliseconds of the four launches of the recorded calls (total_ms[4] = peac_blocks, peac_ahc, peac_order, peac_refine), their number, and resets. */
int planar_peac_set_profiling(planar_peac* peac, int enable);
int planar_peac_get_profile(planar_peac* peac, double* total_ms, int64_t* calls);
/* Profiling aid: per-frame record of the last call, out[B][48] (100 MHz ticks since kernel entry:
 * [1] graph edges, [2] heap built, [3] ahCluster, [4] seeds, [5] floodFill, [6] end; [7] evaluation phases << 40 | nodes evaluated << 20 | valid-record pops;
 * [8] flood-fill queue entries, [9] nodes, [10] pops of nodes whose bag lives in the pool; [16..39] shader-cycle buckets of the clustering kernel, zero
 * unless the library was built with -DPLANAR_PEAC_TIMING: tools/peac_ab.py names them). */
int planar_peac_read_timing(planar_peac* peac, int B, int64_t* out);

/* ---- local bundle adjustment (replaces the numerical core of Optimizer::LocalBundleAdjustment,
 *      src/Optimizer.cc:1853-2680 / include/Optimizer.h:35: optimize(5) -> outlier levels -> optimize(10) -> erase lists) ---- */
/* RCCL communicator for the one exchange step on the path: the all-reduce of the reduced camera system when landmarks
 * are partitioned over GPUs.  Rank 0 creates an id, every rank gets it out of band (e.g. a
 * torch.distributed broadcast), then all ranks call planar_comm_create. */
typedef struct planar_comm planar_comm;
typedef struct planar_comm_id { char internal[128]; } planar_comm_id;   /* == ncclUniqueId */
int planar_comm_unique_id(planar_comm_id* out);
int planar_comm_create(planar_ctx* ctx, const planar_comm_id* id, int nranks, int rank, planar_comm** out);
/* The same exchange over a transport the embedding program owns (MPI, gloo, shared memory ...): the library stages the buffer
 * through host memory and calls allreduce(user, buf, n, op) (op 0 = sum, 1 = max; in place; 0 = success) on every rank.
 * It is how several PROCESSES that share ONE GPU (which RCCL refuses) run the partitioned solve - tests/test_ba_gpu.py does that
 * with torch.distributed/gloo on the 1-GPU box - and a way to use the library where RCCL is not wanted. */
typedef int (*planar_allreduce_fn)(void* user, double* buf, size_t n, int op);
int planar_comm_create_hosted(planar_ctx* ctx, planar_allreduce_fn allreduce, void* user, int nranks, int rank, planar_comm** out);
void planar_comm_destroy(planar_comm* comm);

#define PLANAR_BA_MONO 0      /* g2o::EdgeSE3ProjectXYZ        (types_six_dof_expmap.cpp:103-139)  meas = u, v            */
#define PLANAR_BA_STEREO 1    /* g2o::EdgeStereoSE3ProjectXYZ  (:188-235)                          meas = u, v, ur        */
#define PLANAR_BA_LINE 2      /* EdgeLineProjectXYZ            (include/EdgeLine.h:53-153)         meas = line a, b, c    */
#define PLANAR_BA_PLANE 3     /* g2o::EdgePlane                (g2oAddition/EdgePlane.h:25-126)    meas = plane coeffs    */
#define PLANAR_BA_VERTICAL 4  /* g2o::EdgeVerticalPlane        (g2oAddition/EdgeVerticalPlane.h:21) meas = plane coeffs   */
#define PLANAR_BA_PARALLEL 5  /* g2o::EdgeParallelPlane        (g2oAddition/EdgeParallelPlane.h:21) meas = plane coeffs   */

/* The graph the reference assembles at src/Optimizer.cc:1985-2350, as arrays (all HOST pointers).  Keyframes in
 * ascending mnId; landmarks are 3-dof vertices: MapPoints and the two endpoints of every MapLine (type 0,
 * VertexSBAPointXYZ) and MapPlanes (type 1, VertexPlane).  The two edges of a line observation (start, end) must be
 * consecutive.  With a communicator every rank passes ITS landmarks and their edges (keyframes replicated). */
typedef struct planar_ba_problem {
    int32_t n_kf;
    const float* kf_Tcw;          /* [n_kf][16]  KeyFrame::GetPose(), row-major float32                              */
    const uint8_t* kf_fixed;      /* [n_kf]      setFixed(): mnId == 0 or a fixed camera (:1994, :2007)               */
    int32_t n_lm;
    const uint8_t* lm_type;       /* [n_lm]      0 = XYZ vertex, 1 = plane vertex                                    */
    const double* lm_init;        /* [n_lm][4]   x, y, z, 0  |  plane coefficients (GetWorldPos())                    */
    int32_t n_edges;
    const int32_t* e_kf;          /* [n_edges]   keyframe index (vertex 1)                                           */
    const int32_t* e_lm;          /* [n_edges]   landmark index (vertex 0)                                           */
    const uint8_t* e_type;        /* [n_edges]   PLANAR_BA_*                                                         */
    const double* e_meas;         /* [n_edges][4]                                                                    */
    const float* e_inv_sigma2;    /* [n_edges]   mvInvLevelSigma2[octave] for point edges (ignored otherwise)        */
} planar_ba_problem;

typedef struct planar_ba_result {
    float* kf_Tcw;                /* [n_kf][16]  optimised poses (what the reference passes to KeyFrame::SetPose)    */
    double* lm;                   /* [n_lm][4]   optimised landmarks                                                 */
    uint8_t* e_outlier;           /* [n_edges]   1 = the observation lands in the reference's erase lists (:2471-2575) */
    int32_t lm_iterations;        /* LM iterations run                                                               */
    int32_t stopped;              /* 1 if *stop_flag was seen (pbStopFlag, :1982-1983)                               */
} planar_ba_result;

/* its1 = 5, its2 = 10 reproduce the reference.  `params` supplies fx, fy, cx, cy, bf and the Plane.* configuration.
 * stop_flag (or NULL) is the reference's `bool* pbStopFlag` (one byte; the host samples it when LM steps are enqueued - with a flag at most two steps per chunk, so
 * a flag raised while the GPU is solving is seen at most two LM steps later - and once more between optimize(its1) and optimize(its2), as the reference's bDoMore
 * does; with several ranks every decision is taken on the all-reduced value).  comm may be NULL (single GPU).  Synchronous.
 * With the flag already up on entry nothing is optimised (lm_iterations == 0, stopped == 1): the poses and landmarks come back as given (poses through a quaternion,
 * planes normalised) and e_outlier holds the verdicts of :2471-2575 on the errors of that entry estimate, computed once.  (The reference leaves these verdicts
 * undefined there: with the flag up g2o never calls computeActiveErrors.)
 * Non-fixed key frames: any number up to 128 (PLANAR_ECAPACITY above); up to 20 the reduced camera system stays in LDS, above that it is accumulated and
 * factorised in global memory (slower per LM step, same results): Optimizer::LocalBundleAdjustment has no cap on the covisible key frames. */
int planar_local_ba(planar_ctx* ctx, const planar_ba_problem* problem, const planar_pose_params* params, int its1, int its2,
                    planar_ba_result* result, const volatile unsigned char* stop_flag, planar_comm* comm);

/* ---- Global bundle adjustment (replaces the numerical core of Optimizer::BundleAdjustment, src/Optimizer.cc:44-548, as Optimizer::GlobalBundleAdjustemnt calls it
 *      from LoopClosing::RunGlobalBundleAdjustment: ONE optimize(iterations) over every key frame and landmark of the map, no outlier levels, no erase lists) ----
 * The same planar_ba_problem as the local BA: key frames in ascending mnId, kf_fixed = (mnId == 0) in the reference (any pattern is accepted, none fixed and all
 * fixed included), line edges in consecutive (start, end) pairs with e_kf the OBSERVING key frame (:225-236 read that key frame's own line function; the local
 * BA's quirk of hanging them on the central key frame does not exist here), identity information on both line edges, angleInfo on both the vertical and the
 * parallel edges.  Huber kernels by edge kind: mono sqrt(5.99) (5.99 here, 5.991 in the local BA), stereo and line sqrt(7.815), each rounded through float, and
 * only when `robust` is set; plane, vertical and parallel edges always carry theirs (sqrt(Plane.Chi), sqrt(Plane.VPChi)).
 * A landmark without an edge is not optimised (the reference's vbNotIncluded*): lm_included is 0 and lm is lm_init, bit for bit.  A landmark whose edges all sit
 * on fixed key frames is optimised.  stop_flag (or NULL) is sampled as planar_local_ba samples it; with the flag up on entry nothing is optimised (status
 * PLANAR_GBA_STOPPED, poses through a quaternion, planes normalised).  No edges at all: nothing to optimise, status PLANAR_GBA_CONVERGED, the same pass-through.
 * Up to PLANAR_GBA_MAX_KF key frames, fixed ones included: one more is PLANAR_ECAPACITY and writes nothing.  PLANAR_EINVAL (nothing launched, nothing written) on
 * the conditions planar_local_ba checks: a null argument or array, negative sizes, an edge that names a key frame, landmark or kind out of range, a line edge
 * without its partner.  There is no communicator argument: single GPU only.  Synchronous.  Two calls on the same input return the same bits (no floating-point
 * atomics anywhere; every sum has one owner and a fixed order). */
#define PLANAR_GBA_MAX_KF 256          /* = PLANAR_ESSGRAPH_MAX_KF: the call that follows the essential graph takes what the essential graph takes */
#define PLANAR_GBA_CONVERGED 1         /* g2o's own stop rules: ten failed trials in an iteration, rho == 0, or three iterations without gain */
#define PLANAR_GBA_MAX_ITERATIONS 2
#define PLANAR_GBA_STOPPED 3           /* the stop flag */
typedef struct planar_gba_result {
    float* kf_Tcw;                /* [n_kf][16]  optimised poses                                                     */
    double* lm;                   /* [n_lm][4]   optimised landmarks                                                 */
    uint8_t* lm_included;         /* [n_lm]      0 where the reference would skip the landmark (no edge)             */
    int32_t lm_iterations;        /* LM iterations run                                                               */
    int32_t trials;               /* LM trials run (an iteration has one, plus one per rejected step)                */
    int32_t stopped;              /* 1 if *stop_flag was seen                                                        */
    int32_t status;               /* PLANAR_GBA_*                                                                    */
    double chi2;                  /* robust chi2 of the returned estimate                                            */
    double lambda;                /* the damping the solve ended with                                                */
} planar_gba_result;
int planar_global_ba(planar_ctx* ctx, const planar_ba_problem* problem, const planar_pose_params* params, int iterations, int robust,
                     planar_gba_result* result, const volatile unsigned char* stop_flag);

/* ---- DBoW2 vocabulary transform (replaces ORBVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) as Frame::ComputeBoW and
 *      KeyFrame::ComputeBoW call it with levelsup = 4; Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1124-1180, :1203-1250; include/ORBVocabulary.h:31) ----
 * The vocabulary arrives as the rows of the text format TemplatedVocabulary::loadFromTextFile reads (ORBvoc.txt): for node 1..n in file order its
 * parent id, isLeaf flag, 32 descriptor bytes and weight; header values k and L.  TF_IDF weighting with L1 normalisation (header "k L 0 0").
 *   word / weight [B][stride]: WordId and idf weight of every feature (the per-feature transform);  node [B][stride]: the id of its ancestor at level
 *   L - levelsup (0 = root when levelsup >= L), -1 for a stopped word (weight 0), i.e. the FeatureVector as one node id per feature - the form
 *   planar_search_by_bow takes;  bow_word / bow_value [B][stride] + bow_n [B]: the BowVector, ascending word id, L1-normalised. */
typedef struct planar_vocab planar_vocab;
int planar_vocab_create(planar_ctx* ctx, int k, int L, int n_nodes, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc /* [n][32] */,
                        const double* weight, planar_vocab** out);
void planar_vocab_destroy(planar_vocab* voc);
int planar_vocab_words(const planar_vocab* voc);
int planar_bow_transform(planar_vocab* voc, const uint8_t* desc, const int32_t* n, int B, int stride, int levelsup, int32_t* word, double* weight,
                         int32_t* node, int32_t* bow_word, double* bow_value, int32_t* bow_n);
/* the three BowVector outputs may be NULL together (FeatureVector only) */
int planar_bow_transform_dev(planar_vocab* voc, const uint8_t* d_desc, const int32_t* d_n, int B, int stride, int levelsup, int32_t* d_word,
                             double* d_weight, int32_t* d_node, int32_t* d_bow_word, double* d_bow_value, int32_t* d_bow_n);

/* ---- key-frame database: BoW scores, relocalisation and loop candidates (replaces KeyFrameDatabase::DetectRelocalizationCandidates(Frame*),
 *      src/KeyFrameDatabase.cc:199-309, as src/Tracking.cc:2561 calls it, KeyFrameDatabase::DetectLoopCandidates(KeyFrame*, float minScore), :76-197, as
 *      src/LoopClosing.cc:141 calls it, and ORBVocabulary::score = L1Scoring::score, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68, src/LoopClosing.cc:134) ----
 * A database is the key frames that KeyFrameDatabase::add() was called with, one per slot; the inverted file is not stored: the order of a word's list is the
 * order of the add() calls (add_seq) among the key frames still present.  Limits (PLANAR_EINVAL beyond them): */
#define PLANAR_KFDB_MAX_WORDS 4096     /* word_stride, q_word_stride: words of one BowVector, the feature limit of the key-frame views (PLANAR_MAX_FRAME_KEYS) */
#define PLANAR_KFDB_MAX_KEYFRAMES 1024 /* kf_stride: slots of one database                                                                                    */
typedef struct planar_kf_database {          /* G databases, padded like every other view */
    int32_t kf_stride, word_stride;
    const int32_t* n_kf;        /* [G]                          slots in use                                         */
    const uint8_t* present;     /* [G][kf_stride]               in the inverted file (add()ed, not erase()d)         */
    const int32_t* add_seq;     /* [G][kf_stride]               order of KeyFrameDatabase::add, unique per database  */
    const int32_t* bow_n;       /* [G][kf_stride]                                                                    */
    const int32_t* bow_word;    /* [G][kf_stride][word_stride]  mBowVec keys, ascending                              */
    const double*  bow_value;   /* [G][kf_stride][word_stride]  must start on an 8-byte boundary                     */
    const int32_t* covis;       /* [G][kf_stride][10]  GetBestCovisibilityKeyFrames(10) as slot indices, -1 = none / not in this database */
} planar_kf_database;
/* mode 0: DetectRelocalizationCandidates, mode 1: DetectLoopCandidates, for B queries.  `db` is a HOST pointer in both flavours (its arrays are device arrays
 * in the _dev one).  Query b runs against database q_db[b] (several queries may share one; the host flavour stages databases 0 .. max(q_db)); its BowVector is
 * q_bow_word / q_bow_value [B][q_word_stride] + q_bow_n [B], the layout planar_bow_transform_dev writes, so that call's output feeds this one without a copy.
 *   excluded [B][kf_stride]   spConnectedKeyFrames.count(pKFi)      min_score [B]   the minScore argument       (loop mode only; may be NULL in mode 0)
 *   score [B][kf_stride]  in/out: on entry what mRelocScore / mLoopScore held, on exit overwritten exactly where the reference assigns it (the key frames it
 *       scores: more common words than minCommonWords).  In reloc mode a covisible neighbour that shares a word but is not scored contributes its STALE
 *       mRelocScore, a member the reference never initialises: here that value is the caller's input (the adapter starts it at 0).
 *   common_words [B][kf_stride]  mnRelocWords / mnLoopWords of the key frames that enter lKFsSharingWords, 0 for every other slot of the row
 *   cand [B][kf_stride], n_cand [B]  the returned vector as slot indices, in its order; nothing is written beyond n_cand[b]
 *   n_scored [B]  nscores (0 when no key frame shares a word)
 * Kept as the reference has it: lKFsSharingWords in first-encounter order (ascending smallest common word, then add_seq); minCommonWords =
 * (int)(maxCommonWords * 0.8f) and `>`; si = (float)score, accScore a float sum in neighbour order, bestScore on `>`; minScoreToRetain = 0.75f * bestAccScore and
 * `>`, bestAccScore from 0 (reloc) or minScore (loop); loop mode: si < minScore is not listed but counts as a neighbour, an excluded key frame is neither;
 * candidates deduplicated on pBestKF, first occurrence.  Left out: a query whose mnId is 0 meeting key frames whose constructor set mnRelocQuery / mnLoopQuery to 0
 * (they would count as already seen); query ids are taken as unique.  B * kf_stride must stay below 2^31. */
int planar_kfdb_detect(planar_ctx* ctx, int mode, const planar_kf_database* db, int B, const int32_t* q_db, const int32_t* q_bow_n, const int32_t* q_bow_word,
                       const double* q_bow_value, int q_word_stride, const uint8_t* excluded, const float* min_score, float* score, int32_t* common_words,
                       int32_t* n_cand, int32_t* cand, int32_t* n_scored);
int planar_kfdb_detect_dev(planar_ctx* ctx, int mode, const planar_kf_database* db, int B, const int32_t* d_q_db, const int32_t* d_q_bow_n,
                           const int32_t* d_q_bow_word, const double* d_q_bow_value, int q_word_stride, const uint8_t* d_excluded, const float* d_min_score,
                           float* d_score, int32_t* d_common_words, int32_t* d_n_cand, int32_t* d_cand, int32_t* d_n_scored);
/* L1Scoring::score(a, b) for P pairs of BowVectors ([P][a_stride] / [P][b_stride], strides up to PLANAR_KFDB_MAX_WORDS): the terms fabs(vi - wi) - fabs(vi) -
 * fabs(wi) of the common words added in ascending word id as one FP64 chain, then -score / 2.0 (-0.0 without a common word).  out [P] is the double; the
 * caller narrows it to float and takes its minimum as src/LoopClosing.cc:134 does. */
int planar_bow_score(planar_ctx* ctx, int P, const int32_t* a_bow_n, const int32_t* a_bow_word, const double* a_bow_value, int a_stride, const int32_t* b_bow_n,
                     const int32_t* b_bow_word, const double* b_bow_value, int b_stride, double* out);
int planar_bow_score_dev(planar_ctx* ctx, int P, const int32_t* d_a_bow_n, const int32_t* d_a_bow_word, const double* d_a_bow_value, int a_stride,
                         const int32_t* d_b_bow_n, const int32_t* d_b_bow_word, const double* d_b_bow_value, int b_stride, double* d_out);

/* ---- the local map of a tracked frame (replaces Tracking::UpdateLocalMap, src/Tracking.cc:2394-2405, the first statement of TrackLocalMap, :1954: UpdateLocalKeyFrames
 *      :2458-2552, UpdateLocalPoints :2434-2455, UpdateLocalLines :2407-2432, and the head loops of SearchLocalPoints :2289-2312 / SearchLocalLines :2334-2358) ----
 * A map is what the tracking thread reads of Map / KeyFrame / MapPoint / MapLine, as indices: key frames, map points and map lines are named by their position in
 * the map's arrays, -1 = NULL / none.  G maps, padded like every other view; frame b of a call reads map map_of[b] (several frames may share one).  Limit: */
#define PLANAR_LOCALMAP_MAX_KEYFRAMES 1024 /* kf_stride: key frames of one map (= PLANAR_KFDB_MAX_KEYFRAMES) */
typedef struct planar_local_map {
    int32_t n_maps;              /* G */
    int32_t kf_stride, slot_stride, line_slot_stride, pt_stride, ml_stride, obs_cap, child_cap;
    const int32_t* n_kf;         /* [G]                              key frames in use                                                             */
    const uint8_t* kf_bad;       /* [G][kf_stride]                   KeyFrame::isBad()                                                             */
    const int32_t* kf_rank;      /* [G][kf_stride]                   position of the key frame in std::less<KeyFrame*> order: a permutation of [0, n_kf) */
    const int32_t* covis;        /* [G][kf_stride][10]               GetBestCovisibilityKeyFrames(10), -1 = none                                   */
    const int32_t* parent;       /* [G][kf_stride]                   GetParent(), -1 = none                                                        */
    const int32_t* child_off;    /* [G][kf_stride + 1]               GetChilds() of key frame k = child[g][child_off[k] .. child_off[k + 1])       */
    const int32_t* child;        /* [G][child_cap]                   in the std::set's own (pointer) order                                         */
    const int32_t* n_slots;      /* [G][kf_stride]                   GetMapPointMatches().size()                                                   */
    const int32_t* kf_pts;       /* [G][kf_stride][slot_stride]      GetMapPointMatches(): map-point ids, -1 = NULL                                */
    const int32_t* n_line_slots; /* [G][kf_stride]                   GetMapLineMatches().size()                                                    */
    const int32_t* kf_lines;     /* [G][kf_stride][line_slot_stride] map-line ids, -1 = NULL                                                       */
    const int32_t* n_pts;        /* [G]                              map points in use                                                             */
    const uint8_t* pt_bad;       /* [G][pt_stride]                   MapPoint::isBad()                                                             */
    const int32_t* obs_off;      /* [G][pt_stride + 1]               GetObservations() of point p = obs_kf[g][obs_off[p] .. obs_off[p + 1])        */
    const int32_t* obs_kf;       /* [G][obs_cap]                     the observing key frames                                                      */
    const float* pt_xw;          /* [G][pt_stride][3]                GetWorldPos()                                                                 */
    const float* pt_normal;      /* [G][pt_stride][3]                GetNormal()                                                                   */
    const float* pt_min_dist;    /* [G][pt_stride]                   mfMinDistance                                                                 */
    const float* pt_max_dist;    /* [G][pt_stride]                   mfMaxDistance                                                                 */
    const uint8_t* pt_desc;      /* [G][pt_stride][32]               GetDescriptor(); must start on a 4-byte boundary                              */
    const int32_t* n_ml;         /* [G]                              map lines in use                                                              */
    const uint8_t* ml_bad;       /* [G][ml_stride]                   MapLine::isBad()                                                              */
    const uint8_t* ml_observed;  /* [G][ml_stride]                   Observations() > 0                                                            */
    const double* ml_xw6;        /* [G][ml_stride][6]                GetWorldPos(); the doubles must start on an 8-byte boundary                   */
    const double* ml_normal;     /* [G][ml_stride][3]                GetNormal()                                                                   */
    const float* ml_min_dist;    /* [G][ml_stride]                                                                                                 */
    const float* ml_max_dist;    /* [G][ml_stride]                                                                                                 */
    const uint8_t* ml_desc;      /* [G][ml_stride][32]               GetDescriptor(); must start on a 4-byte boundary                              */
} planar_local_map;
/* The per-batch workspace: per frame the local key-frame list and two per-key-frame prefix counts (12 * kf_stride bytes), a position mark and an "already in the
 * frame" byte per map point and per map line (5 * pt_stride + 5 * ml_stride bytes) and 32 bytes of state, i.e. 12 * kf_stride + 5 * (pt_stride + ml_stride) + 32
 * bytes per frame of max_batch, allocated by the first call on the handle (creating it touches no device).  A call on maps with larger strides than the
 * workspace was made for is PLANAR_EINVAL. */
typedef struct planar_local_map_ws planar_local_map_ws;
int planar_local_map_ws_create(planar_ctx* ctx, int max_batch, int kf_stride, int pt_stride, int ml_stride, planar_local_map_ws** out);
void planar_local_map_ws_destroy(planar_local_map_ws* ws);
/* HIP-event timing of the launches of planar_update_local_map_dev, as planar_plane_clouds_set_profiling: total_ms [5] = the two memsets, localmap_keyframes,
 * localmap_mark, localmap_count, localmap_gather (points and lines) over `calls` recorded calls (tools/local_map_bench.py reads them) */
int planar_local_map_ws_set_profiling(planar_local_map_ws* ws, int enable);
int planar_local_map_ws_get_profile(planar_local_map_ws* ws, double* total_ms, int64_t* calls);
/* Tracking::UpdateLocalMap for B frames.  `map` is a HOST pointer in both flavours (its arrays are device arrays in the _dev one); every other array follows the
 * flavour.  The arrays of frame b:
 *   n_frame [B], frame_match [B][frame_stride]   in/out: mCurrentFrame.N and mvpMapPoints as map-point ids; a bad point's entry becomes -1 (:2470, :2294)
 *   n_frame_lines [B], frame_line_match [B][frame_line_stride]   in/out: NL and mvpMapLines likewise (:2339)
 *   local_kf [B][local_kf_stride], n_local_kf [B]   in/out: mvpLocalKeyFrames; rewritten unless the vote is empty
 *   ref_kf [B]   mpReferenceKF = pKFmax, or -1: keep the one you have (empty vote, or every voted key frame bad)
 *   lp_id [B][lp_stride], n_lp [B]   mvpLocalMapPoints as ids, in the reference's order, and per listed point j the inputs of the next two calls in their layouts:
 *       lp_valid, lp_xw [..][3], lp_normal [..][3], lp_min_dist, lp_max_dist  ->  planar_is_in_frustum_points_dev (n = n_lp, stride = lp_stride)
 *       lp_desc [..][32], lp_observed (GetObservations() non-empty)           ->  planar_map_probes
 *       lp_valid[j] = 0 where the frame holds the point already (frame_match names it once the bad ones are nulled): mnLastFrameSeen == mCurrentFrame.mnId (:2309)
 *   ll_id [B][ll_stride], n_ll [B], ll_valid, ll_xw6 [..][6], ll_normal [..][3] (double), ll_min_dist, ll_max_dist, ll_desc [..][32], ll_observed: mvpLocalMapLines
 *       likewise, for planar_is_in_frustum_lines_dev and planar_lsd_search_by_projection_dev; ll_valid honours frame_line_match (:2356)
 *   status [B]   0 ok; 1 empty vote, the list that came in was kept; 3 an output list was longer than its stride: its count reports the full length and nothing is
 *       written at or beyond the stride; 2 an index read from the map or the frame was out of range: the frame's lists are empty (n_lp = n_ll = 0), local_kf /
 *       n_local_kf are left as they came in, ref_kf = -1 (matches nulled before the index was met stay nulled).  Nothing is ever read or written out of bounds.
 * Kept as the reference has it:
 *   vote       every key point with a match >= 0 whose point is not bad gives +1 to each key frame of the point's observation list (:2460-2473)
 *   empty vote no key frame got a vote (bad ones count here, it is keyframeCounter.empty()): return, the previous mvpLocalKeyFrames stays (:2475) and the points
 *              and lines are still rebuilt from it
 *   voted list std::map<KeyFrame*, int> iterates in pointer order = ascending kf_rank; a bad key frame is neither listed, nor marked, nor a candidate for the
 *              maximum; pKFmax on `>` from 0: the first of equal counts wins (:2485-2499)
 *   expansion  over the VOTED entries only (the end iterator is taken once, :2503): `size > 80` at the top of an iteration ends the loop, on the live size, so the
 *              list can end at 83; per key frame the first covis entry that is neither bad nor marked, then the first such child, then the parent if it is not
 *              marked - isBad() is not asked of the parent, and appending the parent ends the WHOLE loop (the break of :2542 sits in the outer for)
 *   lists      local key frames in list order, slots in slot order; a point / line is kept at its first occurrence if it is neither NULL nor bad
 * A mark (mnTrackReferenceForFrame == mCurrentFrame.mnId) is per frame of the call: frames of one batch that share a map do not see each other's marks, nor does
 * the next call.  IncreaseVisible and the other counters of SearchLocalPoints / SearchLocalLines stay the caller's.
 * PLANAR_EINVAL before any HIP call: a null argument or map array, B < 1 or above the workspace's max_batch, kf_stride outside [1, PLANAR_LOCALMAP_MAX_KEYFRAMES],
 * any other stride or capacity < 1 (slot strides above 2^20), strides above the workspace's, misaligned descriptor / double arrays.  The host-pointer flavour also
 * walks the maps 0 .. n_maps - 1 and the frames on the host and returns PLANAR_EINVAL, before it touches a device, for every index the kernels could meet out of
 * range (observation key frames, slot contents, covis, children, parent, kf_rank, map_of, frame_match, frame_line_match, the incoming local_kf, the counts). */
int planar_update_local_map(planar_local_map_ws* ws, const planar_local_map* map, int B, const int32_t* map_of, const int32_t* n_frame, int32_t* frame_match,
                            int frame_stride, const int32_t* n_frame_lines, int32_t* frame_line_match, int frame_line_stride, int32_t* local_kf, int32_t* n_local_kf,
                            int local_kf_stride, int32_t* ref_kf, int32_t* lp_id, int32_t* n_lp, uint8_t* lp_valid, float* lp_xw, float* lp_normal, float* lp_min_dist,
                            float* lp_max_dist, uint8_t* lp_desc, uint8_t* lp_observed, int lp_stride, int32_t* ll_id, int32_t* n_ll, uint8_t* ll_valid, double* ll_xw6,
                            double* ll_normal, float* ll_min_dist, float* ll_max_dist, uint8_t* ll_desc, uint8_t* ll_observed, int ll_stride, int32_t* status);
int planar_update_local_map_dev(planar_local_map_ws* ws, const planar_local_map* map, int B, const int32_t* d_map_of, const int32_t* d_n_frame, int32_t* d_frame_match,
                                int frame_stride, const int32_t* d_n_frame_lines, int32_t* d_frame_line_match, int frame_line_stride, int32_t* d_local_kf,
                                int32_t* d_n_local_kf, int local_kf_stride, int32_t* d_ref_kf, int32_t* d_lp_id, int32_t* d_n_lp, uint8_t* d_lp_valid, float* d_lp_xw,
                                float* d_lp_normal, float* d_lp_min_dist, float* d_lp_max_dist, uint8_t* d_lp_desc, uint8_t* d_lp_observed, int lp_stride,
                                int32_t* d_ll_id, int32_t* d_n_ll, uint8_t* d_ll_valid, double* d_ll_xw6, double* d_ll_normal, float* d_ll_min_dist,
                                float* d_ll_max_dist, uint8_t* d_ll_desc, uint8_t* d_ll_observed, int ll_stride, int32_t* d_status);

/* ---- the covisibility graph of the maps of a planar_local_map (replaces KeyFrame::UpdateConnections, src/KeyFrame.cc:298-432, with AddConnection :132-145 and
 *      UpdateBestCovisibles :147-166; the one author of the covis and parent rows planar_update_local_map reads) ----
 * The connection state of every key frame of the G maps, in the map's kf_stride (S below).  Every array but kf_mnid is in/out. */
typedef struct planar_covis_graph {
    int32_t* conn_w;           /* [G][S][S]   row x = mConnectedKeyFrameWeights of key frame x; 0 = absent (the reference stores no weight below 1)      */
    int32_t* ord_n;            /* [G][S]      mvpOrderedConnectedKeyFrames.size()                                                                        */
    int32_t* ord_kf;           /* [G][S][S]   mvpOrderedConnectedKeyFrames                                                                               */
    int32_t* ord_w;            /* [G][S][S]   mvOrderedWeights                                                                                           */
    uint8_t* first_connection; /* [G][S]      mbFirstConnection                                                                                          */
    const int32_t* kf_mnid;    /* [G][S]      mnId (only `!= 0` is asked); input                                                                         */
    int32_t* parent;           /* [G][S]      mpParent, -1 = none; may be the array planar_local_map.parent points at                                    */
    int32_t* covis;            /* [G][S][10]  the first ten of the ordered list, -1 = none; may be the array planar_local_map.covis points at            */
} planar_covis_graph;
/* The per-call workspace: a counter row of kf_stride ints and 16 bytes of state per entry of max_entries, and the place in the list of every key frame of
 * max_maps maps (4 * (max_entries * (kf_stride + 4) + max_maps * kf_stride) bytes), allocated by the first call on the handle (creating it touches no device).  A
 * call with more entries, more maps or a larger kf_stride than the workspace was made for is PLANAR_EINVAL. */
typedef struct planar_connections_ws planar_connections_ws;
int planar_connections_ws_create(planar_ctx* ctx, int max_entries, int max_maps, int kf_stride, planar_connections_ws** out);
void planar_connections_ws_destroy(planar_connections_ws* ws);
/* HIP-event timing of the launches of planar_update_connections_dev, as planar_local_map_ws_set_profiling: total_ms [3] = the memset with connections_register,
 * connections_count, connections_apply over `calls` recorded calls (tools/connections_bench.py reads them) */
int planar_connections_ws_set_profiling(planar_connections_ws* ws, int enable);
int planar_connections_ws_get_profile(planar_connections_ws* ws, double* total_ms, int64_t* calls);
/* The state the reference reaches by calling UpdateConnections() on the L key frames (entry_map[l], entry_kf[l]) IN LIST ORDER.  `map` and `graph` are HOST
 * structs in both flavours (their arrays are device arrays in the _dev one); the four arrays [L] follow the flavour.  Of the map the call reads only n_kf, kf_rank,
 * n_slots, kf_pts, n_pts, pt_bad, obs_off and obs_kf (and n_maps, kf_stride, slot_stride, pt_stride, obs_cap); the other arrays may be null.
 *   new_parent [L]  the parent key frame l was given in this call (the caller inserts l among its children), else -1
 *   status [L]      0 ok; 1 the counter was empty: nothing changed; 2 (_dev only) an index the entry met was out of range (entry_map, entry_kf, n_kf, n_pts,
 *                   n_slots, slot contents, obs_off, obs_kf, kf_rank), or the list names its key frame twice: the entry has no effect
 * Kept as the reference has it:
 *   count      every slot of the key frame whose point is neither NULL nor bad gives +1 to each key frame of the point's observation list but the key frame
 *              itself (:315-333): a point in two slots counts twice, a point whose list lacks the key frame counts; lines and planes do not vote
 *   targets    the key frames with count >= 15; if none, the maximum on `>` from 0 in pointer order (ascending kf_rank: the first of equals)
 *   AddConnection(j, w) on target x: nothing if conn_w[x][j] == w already; else the weight is set and x's ordered list becomes ALL of its row
 *   own state  row j = the whole counter (stale entries vanish), j's ordered list = the targets only
 *   order      sort on (weight, KeyFrame*) ascending, reversed: descending weight, ties in DESCENDING pointer order
 *   parent     if first_connection[j] and kf_mnid[j] != 0: parent[j] = the front of j's list, the flag clears
 *   covis      rewritten (first ten, padded with -1) for every key frame whose ordered list was written
 * Entries of different maps are independent.  The list may not name a (map, key frame) twice: the host flavour answers PLANAR_EINVAL, in the _dev flavour every
 * entry naming it gets status 2.  Entries with status 2 count as not listed.
 * PLANAR_EINVAL before any HIP call: a null argument, a null array of the graph or of the eight the map must hold, L < 1 or above the workspace's max_entries,
 * kf_stride outside [1, PLANAR_LOCALMAP_MAX_KEYFRAMES], n_maps / slot_stride / pt_stride / obs_cap < 1 (slot_stride above 2^20), kf_stride or n_maps above the
 * workspace's.  The host-pointer flavour also walks the maps and the list on the host and returns PLANAR_EINVAL, before it touches a device, for every index the
 * kernels could meet out of range.  Nothing is ever read or written out of bounds. */
int planar_update_connections(planar_connections_ws* ws, const planar_local_map* map, const planar_covis_graph* graph, int L, const int32_t* entry_map,
                              const int32_t* entry_kf, int32_t* new_parent, int32_t* status);
int planar_update_connections_dev(planar_connections_ws* ws, const planar_local_map* map, const planar_covis_graph* graph, int L, const int32_t* d_entry_map,
                                  const int32_t* d_entry_kf, int32_t* d_new_parent, int32_t* d_status);

/* ---- key-frame insertion into the maps of a planar_local_map (replaces the end of Tracking::Track, src/Tracking.cc:1973-2003 and :321-336, NeedNewKeyFrame
 *      :2049-2137, CreateNewKeyFrame :2139-2285 without its plane loop, and the head of LocalMapping::ProcessNewKeyFrame, src/LocalMapping.cc:123-157) ----
 * The arrays of the G maps that these calls write, in the layout of planar_local_map and, like parent / covis of planar_covis_graph, possibly the very arrays a
 * planar_local_map points at.  Three arrays are new: the observation counters and the observation lists of the lines. */
typedef struct planar_map_edit {
    int32_t n_maps;              /* G */
    int32_t kf_stride, slot_stride, line_slot_stride, pt_stride, ml_stride, obs_cap, ml_obs_cap;
    int32_t* n_kf;               /* [G]                                                                                                            */
    uint8_t* kf_bad;             /* [G][kf_stride]                                                                                                 */
    int32_t* kf_rank;            /* [G][kf_stride]                   a permutation of [0, n_kf)                                                    */
    int32_t* parent;             /* [G][kf_stride]                                                                                                 */
    int32_t* covis;              /* [G][kf_stride][10]                                                                                             */
    int32_t* child_off;          /* [G][kf_stride + 1]                                                                                             */
    int32_t* n_slots;            /* [G][kf_stride]                                                                                                 */
    int32_t* kf_pts;             /* [G][kf_stride][slot_stride]                                                                                    */
    int32_t* n_line_slots;       /* [G][kf_stride]                                                                                                 */
    int32_t* kf_lines;           /* [G][kf_stride][line_slot_stride]                                                                               */
    int32_t* n_pts;              /* [G]                                                                                                            */
    uint8_t* pt_bad;             /* [G][pt_stride]                                                                                                 */
    int32_t* obs_off;            /* [G][pt_stride + 1]               obs_off[0] = 0, ascending; obs_off[n_pts] entries of obs_kf are in use        */
    int32_t* obs_kf;             /* [G][obs_cap]                     each list in ascending kf_rank (std::map<KeyFrame*, size_t>)                  */
    int32_t* pt_nobs;            /* [G][pt_stride]                   MapPoint::nObs = Observations(): +2 per observation with mvuRight >= 0, else +1 */
    float* pt_xw;                /* [G][pt_stride][3]                                                                                              */
    float* pt_normal;            /* [G][pt_stride][3]                                                                                              */
    float* pt_min_dist;          /* [G][pt_stride]                                                                                                 */
    float* pt_max_dist;          /* [G][pt_stride]                                                                                                 */
    uint8_t* pt_desc;            /* [G][pt_stride][32]               4-byte aligned                                                                */
    int32_t* n_ml;               /* [G]                                                                                                            */
    uint8_t* ml_bad;             /* [G][ml_stride]                                                                                                 */
    uint8_t* ml_observed;        /* [G][ml_stride]                   Observations() > 0                                                            */
    int32_t* ml_obs_off;         /* [G][ml_stride + 1]               the observation lists of the lines, as obs_off / obs_kf                       */
    int32_t* ml_obs_kf;          /* [G][ml_obs_cap]                                                                                                */
    int32_t* ml_nobs;            /* [G][ml_stride]                   MapLine::nObs: +1 per observation                                             */
    double* ml_xw6;              /* [G][ml_stride][6]                8-byte aligned                                                                */
    double* ml_normal;           /* [G][ml_stride][3]                                                                                              */
    float* ml_min_dist;          /* [G][ml_stride]                                                                                                 */
    float* ml_max_dist;          /* [G][ml_stride]                                                                                                 */
    uint8_t* ml_desc;            /* [G][ml_stride][32]               4-byte aligned                                                                */
    const planar_covis_graph* graph; /* optional (a HOST pointer in both flavours); its arrays MUST be laid out in this view's n_maps and kf_stride, as
                                  * planar_update_connections asks of its graph: the struct carries no sizes of its own, so nothing can check it, and a graph
                                  * packed with another stride is written out of bounds.  planar_create_new_key_frame initialises the row of the key frame k it
                                  * appends: conn_w[k][x] = conn_w[x][k] = 0 for x <= k, ord_n[k] = 0, first_connection[k] = 1, kf_mnid[k] = mnid, parent[k] =
                                  * -1, covis[k][*] = -1 */
} planar_map_edit;
/* The tracked frames of a call, B of them, padded like every other view.  planar_need_new_key_frame reads map_of, the counts, the matches, the outlier flags and
 * the depths (the others may be null); planar_create_new_key_frame reads all but the outlier flags. */
typedef struct planar_kf_frames {
    int32_t B, frame_stride, frame_line_stride;
    const int32_t* map_of;       /* [B]                          the frame's map                                                                     */
    const int32_t* n_frame;      /* [B]                          mCurrentFrame.N                                                                     */
    int32_t* frame_match;        /* [B][frame_stride]            in/out: mvpMapPoints as map-point ids, -1 = NULL                                    */
    uint8_t* outlier;            /* [B][frame_stride]            in/out: mvbOutlier                                                                  */
    const float* depth;          /* [B][frame_stride]            mvDepth                                                                             */
    const float* u_right;        /* [B][frame_stride]            mvuRight (planar_stereo_from_rgbd_dev)                                              */
    const float* xw;             /* [B][frame_stride][3]         UnprojectStereo(i) (planar_stereo_from_rgbd_dev)                                    */
    const float* normal;         /* [B][frame_stride][3]         planar_update_normal_and_depth_dev on the frame's single observation                */
    const float* min_dist;       /* [B][frame_stride]                                                                                                */
    const float* max_dist;       /* [B][frame_stride]                                                                                                */
    const uint8_t* desc;         /* [B][frame_stride][32]        mDescriptors, 4-byte aligned                                                        */
    const int32_t* n_frame_lines; /* [B]                         NL                                                                                  */
    int32_t* frame_line_match;   /* [B][frame_line_stride]       in/out: mvpMapLines                                                                 */
    uint8_t* line_outlier;       /* [B][frame_line_stride]       in/out: mvbLineOutlier                                                              */
    const float* depth_line;     /* [B][frame_line_stride]       mvDepthLine                                                                         */
    const double* xw6;           /* [B][frame_line_stride][6]    obtain3DLine(i), 8-byte aligned                                                     */
    const double* line_normal;   /* [B][frame_line_stride][3]                                                                                        */
    const float* line_min_dist;  /* [B][frame_line_stride]                                                                                           */
    const float* line_max_dist;  /* [B][frame_line_stride]                                                                                           */
    const uint8_t* line_desc;    /* [B][frame_line_stride][32]   4-byte aligned                                                                      */
} planar_kf_frames;
/* What NeedNewKeyFrame reads from outside the frame and the map, per frame (48 bytes) */
typedef struct planar_need_kf_params {
    uint64_t frame_id;                              /* mCurrentFrame.mnId (long unsigned)                                       */
    uint32_t last_reloc_frame_id, last_kf_frame_id; /* mnLastRelocFrameId, mnLastKeyFrameId (unsigned int: their sums with the int below wrap as the reference's) */
    int32_t max_frames, min_frames;                 /* mMaxFrames, mMinFrames                                                   */
    float th_depth;                                 /* mThDepth                                                                 */
    int32_t n_kfs_in_map;                           /* Map::KeyFramesInMap()                                                    */
    int32_t n_plane_inliers;                        /* what the plane loops (:2005 ff.) add to mnMatchesInliers                 */
    int32_t flags;                                  /* PLANAR_NEEDKF_*                                                          */
    int32_t keyframes_in_queue;                     /* LocalMapping::KeyframesInQueue()                                         */
    int32_t reserved;
} planar_need_kf_params;
#define PLANAR_NEEDKF_ONLY_TRACKING 1    /* mbOnlyTracking */
#define PLANAR_NEEDKF_MAPPER_STOPPED 2   /* isStopped() || stopRequested() */
#define PLANAR_NEEDKF_MAPPER_ACCEPTS 4   /* AcceptKeyFrames() */
#define PLANAR_NEEDKF_NEW_PLANE 8        /* mCurrentFrame.mbNewPlane */
/* the row of int32 planar_need_new_key_frame writes per frame */
#define PLANAR_NEEDKF_NOUT 12
enum { PLANAR_NEEDKF_NEED = 0, PLANAR_NEEDKF_INTERRUPT_BA, PLANAR_NEEDKF_MATCHES_INLIERS, PLANAR_NEEDKF_REF_MATCHES, PLANAR_NEEDKF_MAP, PLANAR_NEEDKF_TOTAL,
       PLANAR_NEEDKF_NON_TRACKED_CLOSE, PLANAR_NEEDKF_C1A, PLANAR_NEEDKF_C1B, PLANAR_NEEDKF_C1C, PLANAR_NEEDKF_C2, PLANAR_NEEDKF_STATUS };
#define PLANAR_KEYFRAME_MAX_KEYS 2048    /* frame_stride and frame_line_stride of planar_create_new_key_frame: a frame's sort keys stay within a sixth of a CU's LDS */
/* The workspace: one int per map of max_maps (the frame or entry that names it), a mark per map point and per map line and a second observation buffer per map
 * (4 * (1 + pt_stride + ml_stride + obs_cap + ml_obs_cap) bytes per map), allocated by the first call on the handle (creating it touches no device).  A call with
 * more frames than max_batch, more maps than max_maps or larger strides / capacities than the workspace was made for is PLANAR_EINVAL. */
typedef struct planar_keyframe_ws planar_keyframe_ws;
int planar_keyframe_ws_create(planar_ctx* ctx, int max_batch, int max_maps, int pt_stride, int ml_stride, int obs_cap, int ml_obs_cap, planar_keyframe_ws** out);
void planar_keyframe_ws_destroy(planar_keyframe_ws* ws);
/* HIP-event timing, as planar_connections_ws_set_profiling: total_ms [3] = keyframe_need; keyframe_register with keyframe_create; keyframe_register
 * with keyframe_add (the 4-byte-per-map memset ahead of the last two is enqueued before the first event), each over the `calls` recorded calls of ITS entry point (calls [3]) */
int planar_keyframe_ws_set_profiling(planar_keyframe_ws* ws, int enable);
int planar_keyframe_ws_get_profile(planar_keyframe_ws* ws, double* total_ms, int64_t* calls);
/* The end of Tracking::Track for the B frames of `fr` (RGB-D sensor); frames may share a map, the map is only read.  `map` and `fr` are HOST structs in both
 * flavours (their arrays are device arrays in the _dev one); ref_kf [B] (mpReferenceKF), params [B] and out [B][PLANAR_NEEDKF_NOUT] follow the flavour.  In order:
 *   count   mnMatchesInliers (:1973-2003): the matched key points and lines that are not outliers and, unless only_tracking, whose Observations() > 0, plus
 *           n_plane_inliers; outlier entries are not nulled (that is the STEREO sensor's)
 *   clean   "Clean VO matches" (:321-336): a match whose point or line has Observations() < 1 becomes -1 and its outlier flag 0
 *   decide  NeedNewKeyFrame line for line on the cleaned frame: nRefMatches = TrackedMapPoints(nKFs <= 2 ? 2 : 3) over the slots of ref_kf (not NULL, not bad,
 *           pt_nobs >= nMinObs); nMap / nTotal / nNonTrackedClose over 0 < depth < th_depth; ratioMap = (float)((double)(float)nMap / fmax(1.0, nTotal));
 *           mnMatchesInliers < nRefMatches * 0.25 in double, < nRefMatches * thRefRatio in float; the early returns (only_tracking, a stopped mapper, too close
 *           to a relocalisation) give need = 0 with the counters and condition bits still reported
 *   out     need, interrupt_ba (InterruptBA() was called), the five counters, c1a, c1b, c1c, c2, status: 0 ok; 2 (_dev only) an index was out of range (map_of,
 *           ref_kf, the counts, a match, a slot of ref_kf): need = 0, the other entries 0, the frame's arrays untouched
 * PLANAR_EINVAL before any HIP call: a null argument or required array, B < 1 or above max_batch, strides < 1 or above the workspace's; the host-pointer
 * flavour also walks every index on the host first. */
int planar_need_new_key_frame(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const int32_t* ref_kf,
                              const planar_need_kf_params* params, int32_t* out);
int planar_need_new_key_frame_dev(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const int32_t* d_ref_kf,
                                  const planar_need_kf_params* d_params, int32_t* d_out);
/* Tracking::CreateNewKeyFrame (RGB-D, planes left to the caller) for the frames b of `fr` with create[b] != 0, at most one per map and call.  Per frame: th_depth,
 * new_rank (the new key frame's place in pointer order, in [0, n_kf]; every kf_rank >= it moves up by one) and mnid.
 *   selection  the pairs (z, i) with z > 0 sorted as std::pair<float, int>; the walk's break (`z > mThDepth && nPoints > 100`, nPoints counting both branches)
 *              processes the first min(M, max(100, c) + 1) of the M candidates, c of which have z <= th_depth; lines: the first min(ML, 51)
 *   creation   a processed key point creates a map point iff its match is -1 or its point has pt_nobs < 1; the new point's id is n_pts plus the number of
 *              creators before it in sorted order; its rows are copies of the frame's (the descriptor too: ComputeDistinctiveDescriptors over one observation
 *              returns it), pt_bad = 0, one observation (the new key frame), pt_nobs = u_right[i] >= 0 ? 2 : 1; lines likewise with ml_nobs = 1, ml_observed = 1
 *   key frame  k = n_kf appended: kf_bad = 0, parent = -1, covis = -1, child_off[k + 1] = child_off[k], n_slots = N, slots = frame_match as it came in with the
 *              created ids over it, lines likewise, kf_rank[k] = new_rank, the optional graph row
 *   frame      frame_match / frame_line_match get the new ids
 *   new_kf [B] k, or -1; created_pt [B][frame_stride], n_created_pt [B], created_ml [B][frame_line_stride], n_created_ml [B]: the key-point (line) index of each
 *              creation in creation order
 *   status [B] 0 ok (also a frame not chosen); 2 (_dev only) an index was out of range or the map is named twice (then for every frame naming it); 3 a capacity
 *              (kf_stride, pt_stride, ml_stride, obs_cap, ml_obs_cap, a slot stride below N / NL) would be exceeded.  With 2 or 3 the frame changes nothing.
 * PLANAR_EINVAL as above, and frame_stride or frame_line_stride above PLANAR_KEYFRAME_MAX_KEYS; the host-pointer flavour answers it for a map named twice. */
int planar_create_new_key_frame(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const uint8_t* create, const float* th_depth,
                                const int32_t* new_rank, const int32_t* mnid, int32_t* new_kf, int32_t* created_pt, int32_t* n_created_pt, int32_t* created_ml,
                                int32_t* n_created_ml, int32_t* status);
int planar_create_new_key_frame_dev(planar_keyframe_ws* ws, const planar_map_edit* map, const planar_kf_frames* fr, const uint8_t* d_create, const float* d_th_depth,
                                    const int32_t* d_new_rank, const int32_t* d_mnid, int32_t* d_new_kf, int32_t* d_created_pt, int32_t* d_n_created_pt,
                                    int32_t* d_created_ml, int32_t* d_n_created_ml, int32_t* d_status);
/* The head of LocalMapping::ProcessNewKeyFrame for L entries (entry_map[l], entry_kf[l]), at most one per map and call.  Every slot of the key frame whose point is
 * neither NULL nor bad and does not list the key frame gives the point one observation: the key frame is inserted into the point's list at its place in ascending
 * kf_rank and pt_nobs grows by 2 if u_right[l][slot] >= 0, else by 1; a point in two slots gains one observation and its first slot decides.  Lines likewise with
 * increment 1 and ml_observed = 1.
 *   u_right [L][slot_stride]  mvuRight of the key frame
 *   added_pt [L][slot_stride], added_ml [L][line_slot_stride]  bytes, written for the slots in use: 1 = the slot gave its point the observation
 *   status [L]  0 ok; 2 (_dev only) an index out of range or the map named twice; 3 obs_cap or ml_obs_cap would be exceeded.  With 2 or 3 nothing changes.
 * PLANAR_EINVAL as above. */
int planar_add_observations(planar_keyframe_ws* ws, const planar_map_edit* map, int L, const int32_t* entry_map, const int32_t* entry_kf, const float* u_right,
                            uint8_t* added_pt, uint8_t* added_ml, int32_t* status);
int planar_add_observations_dev(planar_keyframe_ws* ws, const planar_map_edit* map, int L, const int32_t* d_entry_map, const int32_t* d_entry_kf,
                                const float* d_u_right, uint8_t* d_added_pt, uint8_t* d_added_ml, int32_t* d_status);

/* ---- 3-D line back-projection (replaces Frame::isLineGood, src/Frame.cc:189-267, with compPt3dCov / extract3dline_mahdist / verify3dLine /
 *      mah_dist3d_pt_line / computeLine3d_svd of src/LineExtractor.cpp:1157-1470) ----
 * keylines [B][ln_stride] = Frame::mvKeylinesUn, depth = the u16 depth image (imDepth = value * depth_factor), fx.. = Frame::fx.. (K(0,0) of compPt3dCov is fx).
 * seeds [B]: line i of frame b draws from the glibc rand() stream of srand(seeds[b] + i) - the reference uses the process-global rand() state, which
 * is not reproducible; with this seeding a CPU run of the reference that calls srand(seed + i) before line i gives the same draws.
 *   depth_line [B][ln_stride] float   mvDepthLine (-1: no reliable 3-D line)          lines3d [B][ln_stride][6]  mvLines3D (A xyz, B xyz; zeros if none)
 *   good [B][ln_stride] u8            the line was pushed to mVF3DLines                 direction [B][ln_stride][3] FrameLine::direction
 *   n_inliers [B][ln_stride]          tmpLine.pts.size()
 *   packed_dirs [B][ln_stride][3] (or NULL in the _dev form) + n_good [B]: the directions of the good lines in line order = mVF3DLines, the
 *   line_dirs / n_lines arguments of planar_track_manhattan_frame. */
int planar_is_line_good(planar_ctx* ctx, int B, const planar_keyline* keylines, const int32_t* n_lines, int ln_stride, const uint16_t* depth, int width,
                        int height, int pitch_px, int64_t frame_stride_px, float depth_factor, float fx, float fy, float cx, float cy, const uint32_t* seeds,
                        float* depth_line, double* lines3d, uint8_t* good, double* direction, int32_t* n_inliers, double* packed_dirs, int32_t* n_good);
int planar_is_line_good_dev(planar_ctx* ctx, int B, const planar_keyline* d_keylines, const int32_t* d_n_lines, int ln_stride, const uint16_t* d_depth,
                            int width, int height, int pitch_px, int64_t frame_stride_px, float depth_factor, float fx, float fy, float cx, float cy,
                            const uint32_t* d_seeds, float* d_depth_line, double* d_lines3d, uint8_t* d_good, double* d_direction, int32_t* d_n_inliers,
                            double* d_packed_dirs, int32_t* d_n_good);

/* ---- surface normals (replaces the tail of Frame::ComputePlanes, src/Frame.cc:694-751: the depth image sampled every 3rd pixel ->
 *      pcl::IntegralImageNormalEstimation(AVERAGE_3D_GRADIENT, MaxDepthChangeFactor 0.05, NormalSmoothingSize 10) -> vSurfaceNormal) ----
 * Output per frame: planar_normals_count() entries in the reference's push_back order (odd rows m, odd columns n of the
 * ceil(W/3) x ceil(H/3) grid, row-major; 8 560 for 640x480): normals[b][i] = SurfaceNormal::normal (NaN where PCL yields none),
 * points[b][i] = SurfaceNormal::cameraPosition (or NULL); FramePosition is (3n, 3m).  The normals array is what
 * planar_track_manhattan_frame takes (n_normals = count, sn_stride = out_stride). */
typedef struct planar_normals planar_normals;
int planar_normals_create(planar_ctx* ctx, int width, int height, int max_batch, planar_normals** out);
void planar_normals_destroy(planar_normals* nrm);
int planar_normals_count(const planar_normals* nrm);
int planar_normals_grid(const planar_normals* nrm, int* grid_w, int* grid_h, int* out_w, int* out_h);
int planar_normals_compute(planar_normals* nrm, const uint16_t* depth, int B, int pitch_px, int64_t frame_stride_px, float fx, float fy, float cx,
                           float cy, float depth_factor, float* normals /* [B][count][3] */, float* points /* [B][count][3] or NULL */);
int planar_normals_compute_dev(planar_normals* nrm, const uint16_t* d_depth, int B, int pitch_px, int64_t frame_stride_px, float fx, float fy,
                               float cx, float cy, float depth_factor, float* d_normals, float* d_points, int out_stride);

/* ---- Manhattan-frame tracking (replaces Tracking::TrackManhattanFrame, src/Tracking.cc:963-1138, with its helpers
 *      ProjectSN2Conic :886-953, ProjectSN2MF :757-884 and MeanShift :1140-1157; called once per frame by Tracking::Track, :248) ----
 * R_last   : [B][9]   row-major 3x3 float, mLastRcm (camera <- Manhattan frame)
 * normals  : [B][sn_stride][3] float, Frame::vSurfaceNormal[i].normal; n_normals[b] of them are valid
 * line_dirs: [B][ln_stride][3] double, Frame::mVF3DLines[i].direction; n_lines[b] valid
 * R_out    : [B][9]   the returned rotation (U * Vt of the updated axes; the input, possibly with one column replaced, if fewer
 *                     than two directions were found - the reference returns that too)
 * member   : [B][sn_stride + ln_stride] or NULL: bit a-1 set iff the element was pushed to Frame::vSurfaceNormalx/y/z resp.
 *            vVanishingLinex/y/z by ProjectSN2MF for axis a (surface normals first, vanishing directions from offset sn_stride)
 * info     : [B][8] or NULL: numDirectionFound, found mask (bit a-1), numInCone[3], points given to MeanShift per axis [3]
 * density  : [B][3] or NULL: s_j_density of the axes that were found                                                            */
int planar_track_manhattan_frame(planar_ctx* ctx, int B, const float* R_last, const float* normals, const int32_t* n_normals, int sn_stride,
                                 const double* line_dirs, const int32_t* n_lines, int ln_stride, float* R_out, uint8_t* member, int32_t* info,
                                 float* density);
int planar_track_manhattan_frame_dev(planar_ctx* ctx, int B, const float* d_R_last, const float* d_normals, const int32_t* d_n_normals, int sn_stride,
                                     const double* d_line_dirs, const int32_t* d_n_lines, int ln_stride, float* d_R_out, uint8_t* d_member,
                                     int32_t* d_info, float* d_density);

/* ---- plane post-processing (planepost.hip; replaces the head of Frame::ComputePlanes, src/Frame.cc:652-692, with
 *      Frame::MaxPointDistanceFromPlane, src/Frame.cc:755-812) -----------------------------------------------------------------------
 * For every plane PlaneDetection extracted (labels / planes / n_planes exactly as planar_peac_segment delivers them): the member pixels' camera points
 * as float -> pcl::VoxelGrid(leaf) centroids -> coefficient (n, -n.c) in float -> a plane with a centroid farther than dist_th
 * (Plane.DistanceThreshold) is dropped -> pcl::SACSegmentation (plane, RANSAC, optimised coefficients, threshold dist_th) refits the coefficient.
 *   n_out  [B]                     Frame::mnPlaneNum: planes kept
 *   coef   [B][pl_stride][4]       mvPlaneCoefficients (pl_stride = planar_peac_max_planes())
 *   src    [B][pl_stride]          index of the detector plane each kept plane came from
 *   pt_off [B][pl_stride + 1]      mvPlanePoints[k] = points[b][pt_off[k] .. pt_off[k + 1])
 *   points [B][max_points][3]      the kept planes' voxel centroids, concatenated, each plane in PCL's output order
 *   status [B] (_dev only)         0, or 3 = more than max_points voxels / voxel coordinate out of range, 4 = sampler table exhausted: the frame's
 *                                  outputs are then empty; the host-pointer entry point turns it into PLANAR_ECAPACITY
 *   state / nvox / info (optional, per DETECTOR plane, stride pl_stride / pl_stride / pl_stride * 12): 0 kept, 1 distance, 2 no inliers; voxels;
 *                                  {RANSAC iterations, best count, best sample[3], inliers, inliers after the refit, sampler draws, model[4] bits}  */
typedef struct planar_plane_clouds planar_plane_clouds;
int planar_plane_clouds_create(planar_ctx* ctx, int width, int height, int max_batch, int max_points /* voxels per frame: a power of two <= 8192; the kernel holds 36 KB of LDS up to 4096, 64 KB at 8192; the key table is in the workspace */, planar_plane_clouds** out);
void planar_plane_clouds_destroy(planar_plane_clouds* pc);
int planar_plane_clouds_stride(const planar_plane_clouds* pc, int* pl_stride, int* max_points);
/* Plane window: the compute calls that follow only process the detector planes [first, first + count) of every frame (count < 0: all planes again).  pcl::VoxelGrid
 * has no voxel cap (reference src/Frame.cc:674-679); a frame's voxel table here holds max_points (<= 8192) voxels for all its planes together, and a compute call
 * reports PLANAR_ECAPACITY (frame status 3) beyond that.  Such a frame goes through once more plane by plane (window (i, 1) for every plane i, results appended in
 * plane order: exactly the sequence of Frame::ComputePlanes' loop) - include/planar_adapters.hpp and planarslam_amd.planes.PlaneClouds.compute do so; only a SINGLE
 * plane of more than max_points voxels (> 80 m^2 of surface at the 0.1 m leaf) is beyond the structure and is dropped with a message. */
int planar_plane_clouds_set_plane_window(planar_plane_clouds* pc, int first, int count);
/* HIP-event timing of the launches of planar_plane_clouds_compute_dev (bench.py's roofline leg), as planar_peac_set_profiling: total_ms [6] = plane_voxels,
 * plane_items, plane_sort_global, plane_sort_lds, plane_sort_heap, plane_tail over `calls` recorded calls */
int planar_plane_clouds_set_profiling(planar_plane_clouds* pc, int enable);
int planar_plane_clouds_get_profile(planar_plane_clouds* pc, double* total_ms, int64_t* calls);
/* diagnostics (synchronises): per frame of the last call, out [B][4] = {ranges that went through libstdc++'s heap-sort fallback (std::sort of
 * pcl::VoxelGrid::applyFilter on a plane whose introsort depth budget ran out), their elements, the longest, LDS-tier sort blocks} */
int planar_plane_clouds_sort_stats(planar_plane_clouds* pc, int B, int64_t* out);
/* Profiling aid, as planar_peac_read_timing: per-frame phase timestamps of the last call, out[B][16] (100 MHz ticks: [0] entry, [1] table cleared, [2] voxel sums,
 * [3] sorted + centroids, [4] refit, [5] end; [6] voxels, [7] planes; [8..11] shader-clock cycles of wavefront 0 in the voxel-sum phase: row loops, tile ends,
 * executions of the parked-run insertion and the cycles in it). */
int planar_plane_clouds_set_timing(planar_plane_clouds* pc, int enable);
int planar_plane_clouds_read_timing(planar_plane_clouds* pc, int B, int64_t* out);
int planar_plane_clouds_compute(planar_plane_clouds* pc, const uint16_t* depth, int B, int pitch_px, int64_t frame_stride_px, float fx, float fy, float cx,
                                float cy, float depth_factor, const int32_t* labels, const double* planes, const int32_t* n_planes, double dist_th, float leaf,
                                int32_t* n_out, float* coef, int32_t* src, int32_t* pt_off, float* points, int32_t* state, int32_t* nvox, int32_t* info);
int planar_plane_clouds_compute_dev(planar_plane_clouds* pc, const uint16_t* d_depth, int B, int pitch_px, int64_t frame_stride_px, float fx, float fy,
                                    float cx, float cy, float depth_factor, const int32_t* d_labels, const double* d_planes, const int32_t* d_n_planes,
                                    double dist_th, float leaf, int32_t* d_n_out, float* d_coef, int32_t* d_src, int32_t* d_pt_off, float* d_points,
                                    int32_t* d_status, int32_t* d_state, int32_t* d_nvox, int32_t* d_info);
/* Per-frame result codes of the last planar_plane_clouds_compute call on this handle (host-pointer entry point; the _dev entry point delivers them in d_status): 0 ok,
 * 3 = the frame's planes together hold more voxels than max_points (or a voxel index out of range) - pcl::VoxelGrid has no cap (src/Frame.cc:674-679), so callers redo
 * exactly those frames plane by plane (planar_plane_clouds_set_plane_window) -, 4 = sampler table exhausted, 5 = std::sort order not reproducible.  out [B]. */
int planar_plane_clouds_last_status(planar_plane_clouds* pc, int B, int32_t* out);
/* Frame::MaxPointDistanceFromPlane on given clouds (host pointers): planes [n_clouds][4] in/out (written when state == 0), cloud q = points[pt_off[q] ..
 * pt_off[q + 1]); state / info as above. */
int planar_plane_refit(planar_plane_clouds* pc, int n_clouds, const float* points, const int32_t* pt_off, double dist_th, float* planes, int32_t* state,
                       int32_t* info);
/* Map::FlagMatchedPlanePoints (src/Map.cc:366-393): flags[b][j] = 1 for every map point j within 0.5 of the WORLD coefficient (Frame::ComputePlaneWorldCoeff)
 * of a plane i < n_planes[b] with matched[b][i] != 0 (mvpMapPlanes[i] non-null).  xw: [B or 1][n_points][3]; flags are only ever set; n_matches (or NULL): nMatches. */
int planar_flag_matched_plane_points(planar_ctx* ctx, int B, const float* Tcw, const float* coef, const uint8_t* matched, const int32_t* n_planes, int pl_stride,
                                     const float* xw, int n_points, int points_shared, uint8_t* flags, int32_t* n_matches);
int planar_flag_matched_plane_points_dev(planar_ctx* ctx, int B, const float* d_Tcw, const float* d_coef, const uint8_t* d_matched, const int32_t* d_n_planes,
                                         int pl_stride, const float* d_xw, int n_points, int points_shared, uint8_t* d_flags, int32_t* d_n_matches);
/* The cloud half of MapPlane::UpdateCoefficientsAndPoints (src/MapPlane.cc:335-352): the frame plane's points through Twc (row-major 4x4 double, what
 * Converter::toSE3Quat(mTcw).inverse() yields; pcl::transformPointCloud: double arithmetic, float store), the map plane's points appended, VoxelGrid(leaf). */
int planar_merge_plane_points(planar_plane_clouds* pc, const double* Twc, const float* frame_points, int n_frame, const float* map_points, int n_map, float leaf,
                              float* out_points, int out_cap, int32_t* n_out);

/* ---- Frame-side glue of Tracking::Track (frame.hip) ---------------------------------------------------------------------------
 * Frame::ComputeStereoFromRGBD (src/Frame.cc:603-621) + Frame::UnprojectStereo (:623-634) for every keypoint of B frames.
 *   keys / keys_un : [B][stride] mvKeys (the depth image is read at the DISTORTED position, truncated to int) / mvKeysUn
 *   depth          : B frames of 16-bit depth, row pitch `pitch_px`, frame stride `frame_stride_px` (pixels); the float image the
 *                    reference indexes is depth * depth_factor in float (imDepth.convertTo(CV_32F, mDepthMapFactor), src/Tracking.cc:174)
 *   Tcw            : [B][16] the pose UnprojectStereo uses (mRwc, mOw are derived as Frame::UpdatePoseMatrices does)
 *   u_right, depth_out : [B][stride] mvuRight / mvDepth (-1 where the depth is not positive)
 *   xw             : [B][stride][3] UnprojectStereo(i) (zeros where it returns an empty Mat), valid[B][stride] = depth > 0          */
int planar_stereo_from_rgbd(planar_ctx* ctx, int B, const planar_keypoint* keys, const planar_keypoint* keys_un, const int32_t* n, int stride,
                            const uint16_t* depth, int pitch_px, int64_t frame_stride_px, float depth_factor, float fx, float fy, float cx, float cy,
                            float bf, const float* Tcw, float* u_right, float* depth_out, float* xw, uint8_t* valid);
int planar_stereo_from_rgbd_dev(planar_ctx* ctx, int B, const planar_keypoint* d_keys, const planar_keypoint* d_keys_un, const int32_t* d_n, int stride,
                                const uint16_t* d_depth, int pitch_px, int64_t frame_stride_px, float depth_factor, float fx, float fy, float cx,
                                float cy, float bf, const float* d_Tcw, float* d_u_right, float* d_depth_out, float* d_xw, uint8_t* d_valid);

/* MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:347-388) for G groups of map points; group g = the points whose reference key frame (mpRefKF) has the pose
 * ref_Tcw[g] - e.g. the back-projected keypoints of one frame.  Its camera centre is formed as KeyFrame::SetPose does (src/KeyFrame.cc:85-86).
 *   n [G], xw [G][stride][3] (GetWorldPos), valid [G][stride] or NULL (0 = no point: its outputs are left alone)
 *   keys_un [G][stride]: the point's keypoint in the reference key frame (its octave selects mvScaleFactors[level])
 *   obs_off [G * stride + 1], obs_ow [obs_off[G * stride]][3]: camera centres of the key frames observing each point, in observation-map order; both NULL:
 *            every point is observed by its reference key frame only
 *   normal [G][stride][3] (mNormalVector), min_dist / max_dist [G][stride] (mfMinDistance / mfMaxDistance); a point without observations keeps its values */
int planar_update_normal_and_depth(planar_ctx* ctx, int G, const int32_t* n, int stride, const float* xw, const uint8_t* valid, const float* ref_Tcw,
                                   const planar_keypoint* keys_un, const int32_t* obs_off, const float* obs_ow, const float* scale_factors, int n_levels,
                                   float* normal, float* min_dist, float* max_dist);
int planar_update_normal_and_depth_dev(planar_ctx* ctx, int G, const int32_t* d_n, int stride, const float* d_xw, const uint8_t* d_valid, const float* d_ref_Tcw,
                                       const planar_keypoint* d_keys_un, const int32_t* d_obs_off, const float* d_obs_ow, const float* scale_factors,
                                       int n_levels, float* d_normal, float* d_min_dist, float* d_max_dist);

/* What Optimizer::PoseOptimization / TranslationOptimization read from the Frame once the matchers have filled mvpMapPoints / mvpMapLines /
 * mvpMapPlanes / mvpParallelPlanes / mvpVerticalPlanes (src/Optimizer.cc:593-668, 689-745, 859-981), as match INDICES into the arrays of
 * the matched-against objects.  -1 = no association.                                                                                 */
typedef struct planar_track_matches {
    int32_t B;
    /* points */
    int32_t stride, mp_stride, n_levels;
    const int32_t* n;                /* [B]                 Frame::N                                                              */
    const planar_keypoint* keys_un;  /* [B][stride]         mvKeysUn                                                              */
    const float* u_right;            /* [B][stride]         mvuRight                                                              */
    const int32_t* pt_match;         /* [B][stride]         index of the matched map point (what the matchers wrote), -1 = NULL   */
    const float* mp_xw;              /* [B][mp_stride][3]   GetWorldPos() of the candidate map points                             */
    const uint8_t* mp_valid;         /* [B][mp_stride] or NULL: the map point exists (e.g. planar_stereo_from_rgbd's `valid`)      */
    float inv_level_sigma2[PLANAR_MAX_LEVELS]; /* mvInvLevelSigma2                                                                 */
    /* lines (n_lines == NULL: no lines) */
    int32_t ln_stride, ml_stride;
    const int32_t* n_lines;          /* [B]                 Frame::NL                                                             */
    const double* line_eq;           /* [B][ln_stride][3]   mvKeyLineFunctions                                                    */
    const int32_t* ln_match;         /* [B][ln_stride]      index of the matched map line                                         */
    const double* ml_xw6;            /* [B][ml_stride][6]   MapLine::mWorldPos                                                    */
    /* planes (n_planes == NULL: no planes) */
    int32_t pl_stride, mpl_stride, mpl_shared;   /* mpl_shared != 0: one map-plane array for all frames                            */
    const int32_t* n_planes;         /* [B]                 Frame::mnPlaneNum                                                     */
    const float* pl_coef;            /* [B][pl_stride][4]   mvPlaneCoefficients                                                   */
    const int32_t* pl_match;         /* [3][B][pl_stride]   matched / parallel / vertical map plane (PlaneMatcher's three outputs) */
    const float* mpl_coef;           /* [B or 1][mpl_stride][4] MapPlane::GetWorldPos()                                           */
    const float* Tcw;                /* [B][16]             Frame::mTcw the optimiser starts from                                 */
} planar_track_matches;
/* Fills the INPUT arrays of `out` (n_points .. Tcw_in; they are written although the struct declares them const) for planar_pose_opt.
 * Frame b gets min(n[b], out->max_points) points, likewise lines / planes.  Host pointers / device pointers as usual.              */
int planar_pose_assemble(planar_ctx* ctx, const planar_track_matches* matches, const planar_pose_batch* out);
int planar_pose_assemble_dev(planar_ctx* ctx, const planar_track_matches* d_matches, const planar_pose_batch* d_out);

/* The loop that follows the optimiser in Tracking::TranslationWithMotionModel / TrackLocalMap (src/Tracking.cc:1784-1812): a match whose
 * outlier flag is set is dropped (match = -1, flag cleared); kept[b] (or NULL) = matches left.  outlier has row stride flag_stride.  */
int planar_discard_outliers(planar_ctx* ctx, int B, const int32_t* n, int stride, int flag_stride, int32_t* match, uint8_t* outlier, int32_t* kept);
int planar_discard_outliers_dev(planar_ctx* ctx, int B, const int32_t* d_n, int stride, int flag_stride, int32_t* d_match, uint8_t* d_outlier,
                                int32_t* d_kept);

/* ---- element-wise glue between the stages of Tracking::Track (src/Tracking.cc:240-253, 1739-1790, 1954-2040), enqueue-only on the context's stream: with these a
 *      host drives the whole per-frame chain through this header alone (planarslam_amd/track.py launches nothing else inside the timed region).
 *   reset_matches      fill(mvpMapPoints.begin(), mvpMapPoints.end(), NULL): every entry -1
 *   blocked_mask       mask[i] = match[i] >= 0                       (key points / lines that already have a map point are skipped by SearchByProjection)
 *   merge_matches      out = first >= 0 ? first : (second >= 0 ? second + offset : second)   (one index space for PoseOptimization: [last frame | older frame])
 *   manhattan_pose     Tcw_out = Tcw_in with its rotation block replaced by mRotation_wc = (Rotation_cm * MF_can^T)^T (:250-253), as :1778 does before
 *                      TranslationOptimization; Rcm_new = TrackManhattanFrame's result, Rcm0 = the stream's Rotation_cm; [B][9] / [B][16] row-major float32
 *   keypoint_fields    KeyPoint::octave / ::angle of n key points into flat arrays
 *   add_scalar_i32     dst = src + value (per-line rand() seeds of Frame::isLineGood: base + step offset)
 *   copy_rows          pitched device-to-device row copy */
/* Frame::UndistortKeyPoints (reference src/Frame.cc:545-573: cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK), five iterations in double): keys [B][stride]
 * -> keys_un [B][stride] (every field copied, pt undistorted); dist_coef: host array k1, k2, p1, p2, k3 (Camera.k1 .. Camera.k3 of the reference's yaml files);
 * k1 == 0 copies, as :546-549.  Frame::ComputeImageBounds (:575-598) is the same call on the four image corners. */
int planar_undistort_keypoints(planar_ctx* ctx, int B, const planar_keypoint* keys, const int32_t* n, int stride, float fx, float fy, float cx, float cy, const float* dist_coef,
                               planar_keypoint* keys_un);
int planar_undistort_keypoints_dev(planar_ctx* ctx, int B, const planar_keypoint* d_keys, const int32_t* d_n, int stride, float fx, float fy, float cx, float cy,
                                   const float* dist_coef, planar_keypoint* d_keys_un);
int planar_reset_matches_dev(planar_ctx* ctx, int32_t* d_match, int64_t n);
int planar_blocked_mask_dev(planar_ctx* ctx, const int32_t* d_match, int64_t n, uint8_t* d_mask);
int planar_merge_matches_dev(planar_ctx* ctx, const int32_t* d_first, const int32_t* d_second, int offset, int64_t n, int32_t* d_out);
int planar_manhattan_pose_dev(planar_ctx* ctx, int B, const float* d_Rcm_new, const float* d_Rcm0, const float* d_Tcw_in, float* d_Tcw_out);
int planar_keypoint_fields_dev(planar_ctx* ctx, const planar_keypoint* d_keys, int64_t n, int32_t* d_octave, float* d_angle);
int planar_add_scalar_i32_dev(planar_ctx* ctx, const int32_t* d_src, int64_t n, int32_t value, int32_t* d_dst);
int planar_copy_rows_dev(planar_ctx* ctx, void* d_dst, int64_t dst_pitch, const void* d_src, int64_t src_pitch, int64_t row_bytes, int64_t rows);


#ifdef __cplusplus
}
#endif
#endif /* PLANAR_ABI_H */
