// mi355_gms.hpp -- header-only C++ face of the C ABI (include/gms.h) with the reference's exact signature:
//
//   cv::xfeatures2d::matchGMS(const Size&, const Size&, const std::vector<KeyPoint>&, const std::vector<KeyPoint>&,
//                             const std::vector<DMatch>&, std::vector<DMatch>&, bool = false, bool = false, double = 6.0)
//
// (reference call sites: SfM-GMS/SfM-GMS/FeatureMatchUtil.cpp:69, DisparityUtil.cpp:149, :299), and likewise
//
//   cv::xfeatures2d::matchLOGOS(const std::vector<KeyPoint>&, const std::vector<KeyPoint>&, const std::vector<int>&,
//                               const std::vector<int>&, std::vector<DMatch>&)
//
// (FeatureMatchUtil.cpp:86-131).
// With OpenCV headers present the cv:: types are used directly (cv::KeyPoint and cv::DMatch are
// layout-identical to gms_keypoint / gms_dmatch); without them the same-shaped PODs below stand in, so the
// call sites compile unchanged apart from the namespace. Link with libgms_hip.so.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "gms.h"

#if defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
#define MI355_GMS_HAVE_OPENCV 1
#endif
#endif

namespace mi355 {

#ifdef MI355_GMS_HAVE_OPENCV
using Size = cv::Size;
using KeyPoint = cv::KeyPoint;
using DMatch = cv::DMatch;
#else
struct Size {
    int width = 0, height = 0;
    Size() = default;
    Size(int w, int h) : width(w), height(h) {}
};
struct Point2f {
    float x = 0, y = 0;
};
struct KeyPoint {  // cv::KeyPoint
    Point2f pt;
    float size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};
struct DMatch {  // cv::DMatch
    int queryIdx = -1, trainIdx = -1, imgIdx = -1;
    float distance = 0;
};
#endif

static_assert(sizeof(KeyPoint) == sizeof(gms_keypoint), "KeyPoint must be 28 bytes like cv::KeyPoint");
static_assert(sizeof(DMatch) == sizeof(gms_dmatch), "DMatch must be 16 bytes like cv::DMatch");

// Same arguments, same output contract (matchesGMS is cleared, then receives the surviving matches verbatim and in
// input order). Where the reference has undefined behaviour (bad indices, points outside the image) or where no
// GPU is available this throws instead; there is no CPU fallback.
inline void matchGMS(const Size& size1, const Size& size2, const std::vector<KeyPoint>& keypoints1,
                     const std::vector<KeyPoint>& keypoints2, const std::vector<DMatch>& matches1to2,
                     std::vector<DMatch>& matchesGMS, const bool withRotation = false, const bool withScale = false,
                     const double thresholdFactor = 6.0)
{
    std::vector<DMatch> out(matches1to2.size());
    int n_out = 0;
    const int rc = gms_match(reinterpret_cast<const gms_keypoint*>(keypoints1.data()), (int)keypoints1.size(), size1.width,
                             size1.height, reinterpret_cast<const gms_keypoint*>(keypoints2.data()),
                             (int)keypoints2.size(), size2.width, size2.height,
                             reinterpret_cast<const gms_dmatch*>(matches1to2.data()), (int)matches1to2.size(),
                             withRotation ? 1 : 0, withScale ? 1 : 0, thresholdFactor,
                             reinterpret_cast<gms_dmatch*>(out.data()), &n_out);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::matchGMS: ") + gms_error_string(rc));
    out.resize((size_t)n_out);
    matchesGMS.swap(out);
}

// The same filter for a whole sequence in one call: what a caller looping `matchGMS` over image pairs (FeatureMatchUtil.cpp:66-69
// once per pair) switches to for throughput. keypoints[f] / sizes[f] describe frame f; pair p filters matches1to2[p] between frames
// pairs[p].first (query side) and pairs[p].second (train side); matchesGMS[p] receives the survivors. Host vectors in, host vectors
// out: the library stages them through pinned memory on two streams (gms_filter_host_batch) and keeps the frames resident on the GPU
// for the duration of the call. Pairs the reference has undefined behaviour on come back empty with ok[p] = false (if given).
inline void matchGMSBatch(const std::vector<Size>& sizes, const std::vector<std::vector<KeyPoint>>& keypoints,
                          const std::vector<std::pair<int, int>>& pairs, const std::vector<std::vector<DMatch>>& matches1to2,
                          std::vector<std::vector<DMatch>>& matchesGMS, const bool withRotation = false, const bool withScale = false,
                          const double thresholdFactor = 6.0, std::vector<bool>* ok = nullptr)
{
    if (sizes.size() != keypoints.size() || pairs.size() != matches1to2.size()) throw std::invalid_argument("mi355::matchGMSBatch: sizes");
    static gms_ctx* ctx = nullptr;  // one context per process, created on first use (by exactly one of the threads that race here)
    static int ctx_rc = GMS_OK;
    static std::once_flag ctx_once;
    std::call_once(ctx_once, [] { ctx_rc = gms_ctx_create(0, &ctx); });
    if (ctx_rc != GMS_OK || !ctx) throw std::runtime_error(std::string("mi355::matchGMSBatch: ") + gms_error_string(ctx_rc));
    std::vector<int64_t> frame_off(keypoints.size() + 1, 0);
    std::vector<int32_t> wh(2 * keypoints.size());
    for (size_t f = 0; f < keypoints.size(); ++f) {
        frame_off[f + 1] = frame_off[f] + (int64_t)keypoints[f].size();
        wh[2 * f] = sizes[f].width;
        wh[2 * f + 1] = sizes[f].height;
    }
    std::vector<KeyPoint> kp_all((size_t)frame_off.back());
    for (size_t f = 0; f < keypoints.size(); ++f) std::copy(keypoints[f].begin(), keypoints[f].end(), kp_all.begin() + frame_off[f]);
    std::vector<gms_pair> prs(pairs.size());
    int64_t total = 0;
    for (size_t p = 0; p < pairs.size(); ++p) {
        prs[p] = gms_pair{pairs[p].first, pairs[p].second, (int32_t)matches1to2[p].size(), 0, total};
        total += (int64_t)matches1to2[p].size();
    }
    std::vector<DMatch> m_all((size_t)total), out_all((size_t)total);
    for (size_t p = 0; p < pairs.size(); ++p) std::copy(matches1to2[p].begin(), matches1to2[p].end(), m_all.begin() + prs[p].match_off);
    std::vector<gms_pair_result> res(pairs.size());
    const int rc = gms_filter_host_batch(ctx, reinterpret_cast<const gms_keypoint*>(kp_all.data()), frame_off.data(), wh.data(),
                                         (int)keypoints.size(), prs.data(), (int)prs.size(), reinterpret_cast<const gms_dmatch*>(m_all.data()),
                                         withRotation ? 1 : 0, withScale ? 1 : 0, thresholdFactor,
                                         reinterpret_cast<gms_dmatch*>(out_all.data()), res.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::matchGMSBatch: ") + gms_error_string(rc));
    matchesGMS.assign(pairs.size(), std::vector<DMatch>());
    if (ok) ok->assign(pairs.size(), true);
    for (size_t p = 0; p < pairs.size(); ++p) {
        if (res[p].status != GMS_OK) {
            if (ok) (*ok)[p] = false;
            continue;
        }
        matchesGMS[p].assign(out_all.begin() + prs[p].match_off, out_all.begin() + prs[p].match_off + res[p].n_inliers);
    }
}

static_assert(sizeof(int) == sizeof(int32_t), "visual words travel as int32");

// Same arguments, same output as the reference: matches1to2 is cleared, then receives the survivors (queryIdx, trainIdx, imgIdx -1,
// distance 0), queryIdx ascending, then trainIdx. nn1 / nn2 hold the visual word of each keypoint. Throws where the reference has
// undefined behaviour or no GPU is available; there is no CPU fallback.
inline void matchLOGOS(const std::vector<KeyPoint>& keypoints1, const std::vector<KeyPoint>& keypoints2, const std::vector<int>& nn1,
                       const std::vector<int>& nn2, std::vector<DMatch>& matches1to2)
{
    if (nn1.size() != keypoints1.size() || nn2.size() != keypoints2.size())
        throw std::invalid_argument("mi355::matchLOGOS: one label per keypoint");
    // survivors rarely outnumber the larger frame; on overflow the call reports the count it needs and runs once more with it
    int64_t cap = (int64_t)std::max<size_t>(std::max(keypoints1.size(), keypoints2.size()), 1);
    for (int attempt = 0;; ++attempt) {
        std::vector<DMatch> out((size_t)cap);
        int64_t n = 0;
        const int rc = gms_logos_match(reinterpret_cast<const gms_keypoint*>(keypoints1.data()), (int)keypoints1.size(),
                                       reinterpret_cast<const gms_keypoint*>(keypoints2.data()), (int)keypoints2.size(),
                                       reinterpret_cast<const int32_t*>(nn1.data()), reinterpret_cast<const int32_t*>(nn2.data()),
                                       reinterpret_cast<gms_dmatch*>(out.data()), cap, &n, nullptr);
        if (rc == GMS_ERR_CAPACITY && attempt == 0 && n > cap) {
            cap = n;
            continue;
        }
        if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::matchLOGOS: ") + gms_error_string(rc));
        out.resize((size_t)n);
        matches1to2.swap(out);
        return;
    }
}

// The LOGOS filter for a whole sequence in one call, on a context (gms_logos_host_batch): keypoints[f] / words[f] describe frame f
// (words in [0, n_words)), pair p filters frames pairs[p].first (query side) and pairs[p].second; matches1to2[p] receives what
// matchLOGOS would. Each frame's neighbours and word buckets are worked out once for all its pairs. Pairs the library refuses (a word
// out of range, or a keypoint whose x, y or angle is not finite or whose |angle| exceeds 3600 degrees: GMS_ERR_DOMAIN) come back empty with ok[p] = false (if given).
inline void matchLOGOSBatch(const std::vector<std::vector<KeyPoint>>& keypoints, const std::vector<std::vector<int>>& words, int n_words,
                            const std::vector<std::pair<int, int>>& pairs, std::vector<std::vector<DMatch>>& matches1to2,
                            std::vector<bool>* ok = nullptr)
{
    if (keypoints.size() != words.size()) throw std::invalid_argument("mi355::matchLOGOSBatch: one word list per frame");
    static gms_ctx* ctx = nullptr;  // one context per process, created on first use
    static int ctx_rc = GMS_OK;
    static std::once_flag ctx_once;
    std::call_once(ctx_once, [] { ctx_rc = gms_ctx_create(0, &ctx); });
    if (ctx_rc != GMS_OK || !ctx) throw std::runtime_error(std::string("mi355::matchLOGOSBatch: ") + gms_error_string(ctx_rc));
    const size_t nf = keypoints.size();
    std::vector<int64_t> frame_off(nf + 1, 0);
    for (size_t f = 0; f < nf; ++f) {
        if (words[f].size() != keypoints[f].size()) throw std::invalid_argument("mi355::matchLOGOSBatch: one word per keypoint");
        frame_off[f + 1] = frame_off[f] + (int64_t)keypoints[f].size();
    }
    std::vector<KeyPoint> kp_all((size_t)frame_off.back());
    std::vector<int32_t> w_all((size_t)frame_off.back());
    for (size_t f = 0; f < nf; ++f) {
        std::copy(keypoints[f].begin(), keypoints[f].end(), kp_all.begin() + frame_off[f]);
        std::copy(words[f].begin(), words[f].end(), w_all.begin() + frame_off[f]);
    }
    std::vector<int64_t> cap(pairs.size());
    for (size_t p = 0; p < pairs.size(); ++p) {
        const int a = pairs[p].first, b = pairs[p].second;
        if (a < 0 || b < 0 || (size_t)a >= nf || (size_t)b >= nf) throw std::invalid_argument("mi355::matchLOGOSBatch: frame index");
        cap[p] = std::max(keypoints[a].size(), keypoints[b].size());
    }
    std::vector<gms_pair> prs(pairs.size());
    std::vector<gms_logos_result> res(pairs.size());
    std::vector<DMatch> out_all;
    for (int attempt = 0; attempt < 2; ++attempt) {
        int64_t total = 0;
        for (size_t p = 0; p < pairs.size(); ++p) {
            prs[p] = gms_pair{pairs[p].first, pairs[p].second, (int32_t)cap[p], 0, total};
            total += cap[p];
        }
        out_all.assign((size_t)total, DMatch());
        const int rc = gms_logos_host_batch(ctx, reinterpret_cast<const gms_keypoint*>(kp_all.data()), frame_off.data(), (int)nf,
                                            w_all.data(), n_words, prs.data(), (int)prs.size(),
                                            reinterpret_cast<gms_dmatch*>(out_all.data()), res.data());
        if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::matchLOGOSBatch: ") + gms_error_string(rc));
        bool again = false;
        for (size_t p = 0; p < pairs.size(); ++p)
            if (res[p].status == GMS_ERR_CAPACITY) {
                if (res[p].n_out > INT32_MAX) throw std::runtime_error("mi355::matchLOGOSBatch: too many survivors");
                cap[p] = res[p].n_out;
                again = true;
            }
        if (!again) break;
    }
    matches1to2.assign(pairs.size(), std::vector<DMatch>());
    if (ok) ok->assign(pairs.size(), true);
    for (size_t p = 0; p < pairs.size(); ++p) {
        if (res[p].status != GMS_OK) {
            if (ok) (*ok)[p] = false;
            continue;
        }
        matches1to2[p].assign(out_all.begin() + prs[p].match_off, out_all.begin() + prs[p].match_off + res[p].n_out);
    }
}

// The dictionary the reference builds with BOWKMeansTrainer(n_words).cluster(desc1) (FeatureMatchUtil.cpp:100-104), trained on the
// GPU (gms_logos_dict_train): k-means with k-means++ seeding, `attempts` restarts, at most `max_iters` assignments. Not OpenCV's
// rows -- cv::kmeans draws from a global RNG and sums in float -- but the same bytes on every run for the same rows and seed. The
// shim has no cv::Mat: descriptors are flat row-major vectors of 128 floats (finite, |x| <= 4096) or 32 bytes per row, and so is
// the dictionary returned (n_words rows). labels (optional) gets the word of every row; result (optional) the record. Too few rows
// (fewer than n_words) or rows outside the domain throw.
namespace detail {
inline void train_dict(int kind, const void* desc, size_t n, void* dict, int n_words, int attempts, int max_iters,
                       uint64_t seed, std::vector<int>* labels, gms_logos_dict_result* result)
{
    const int64_t off[2] = {0, (int64_t)n};
    std::vector<int32_t> lab(std::max<size_t>(n, 1), -1);
    gms_logos_dict_result res{};
    int rc = gms_logos_dict_train(kind, n ? desc : nullptr, off, 1, n_words, attempts, max_iters, seed, dict, &res, lab.data());
    if (rc == GMS_OK) rc = res.status;
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::trainLogosDictionary: ") + gms_error_string(rc));
    if (labels) labels->assign(lab.begin(), lab.begin() + (std::ptrdiff_t)n);
    if (result) *result = res;
}
}  // namespace detail

inline std::vector<float> trainLogosDictionary(const std::vector<float>& descriptors, int n_words = 50, int attempts = 3,
                                               int max_iters = 100, uint64_t seed = 0, std::vector<int>* labels = nullptr,
                                               gms_logos_dict_result* result = nullptr)
{
    if (descriptors.size() % 128 || n_words < 1) throw std::invalid_argument("mi355::trainLogosDictionary: rows of 128 floats, n_words >= 1");
    std::vector<float> dict((size_t)n_words * 128);
    detail::train_dict(GMS_DESC_L2_F32X128, descriptors.data(), descriptors.size() / 128, dict.data(), n_words, attempts, max_iters, seed,
                       labels, result);
    return dict;
}

inline std::vector<uint8_t> trainLogosDictionary(const std::vector<uint8_t>& descriptors, int n_words = 50, int attempts = 3,
                                                 int max_iters = 100, uint64_t seed = 0, std::vector<int>* labels = nullptr,
                                                 gms_logos_dict_result* result = nullptr)
{
    if (descriptors.size() % 32 || n_words < 1) throw std::invalid_argument("mi355::trainLogosDictionary: rows of 32 bytes, n_words >= 1");
    std::vector<uint8_t> dict((size_t)n_words * 32);
    detail::train_dict(GMS_DESC_HAMMING256, descriptors.data(), descriptors.size() / 32, dict.data(), n_words, attempts, max_iters, seed,
                       labels, result);
    return dict;
}

// The reference's bruteForceMatch (FeatureMatchUtil.cpp:20-31): BFMatcher(norm, crossCheck).match(desc1, desc2), std::sort by
// distance (MSVC's order among equal distances), then the matches within distance_coef times the smallest distance, at most
// max_size. The shim has no cv::Mat: descriptors come as flat row-major vectors -- 128 floats per row (SIFT, NORM_L2) or 32 bytes
// per row (ORB, NORM_HAMMING). matches receives (queryIdx, trainIdx, imgIdx 0, distance). An empty frame throws (the reference reads
// front() of an empty vector there).
namespace detail {
inline void bf_match(int kind, const void* d1, size_t n1, const void* d2, size_t n2, std::vector<DMatch>& matches, bool cross_check,
                     double distance_coef, int max_size)
{
    const int64_t cap = (int64_t)std::max<size_t>(std::min<size_t>(n1, (size_t)std::max(max_size, 0)), 1);
    std::vector<DMatch> out((size_t)cap);
    int64_t n = 0;
    const int rc = gms_bf_match_select(kind, n1 ? d1 : nullptr, (int)n1, n2 ? d2 : nullptr, (int)n2, cross_check ? 1 : 0, distance_coef,
                                       max_size, reinterpret_cast<gms_dmatch*>(out.data()), cap, &n, nullptr);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::bruteForceMatch: ") + gms_error_string(rc));
    out.resize((size_t)n);
    matches.swap(out);
}
}  // namespace detail

inline void bruteForceMatch(const std::vector<float>& desc1, const std::vector<float>& desc2, std::vector<DMatch>& matches,
                            bool cross_check = true, double distance_coef = 4.0, int max_size = 500)
{
    if (desc1.size() % 128 || desc2.size() % 128) throw std::invalid_argument("mi355::bruteForceMatch: rows of 128 floats");
    detail::bf_match(GMS_DESC_L2_F32X128, desc1.data(), desc1.size() / 128, desc2.data(), desc2.size() / 128, matches, cross_check,
                     distance_coef, max_size);
}

inline void bruteForceMatch(const std::vector<uint8_t>& desc1, const std::vector<uint8_t>& desc2, std::vector<DMatch>& matches,
                            bool cross_check = true, double distance_coef = 4.0, int max_size = 500)
{
    if (desc1.size() % 32 || desc2.size() % 32) throw std::invalid_argument("mi355::bruteForceMatch: rows of 32 bytes");
    detail::bf_match(GMS_DESC_HAMMING256, desc1.data(), desc1.size() / 32, desc2.data(), desc2.size() / 32, matches, cross_check,
                     distance_coef, max_size);
}

// bruteForceMatch for a whole sequence in one call, on a context (gms_bf_select_host_batch): descriptors[f] holds frame f's rows
// (flat, T = float: 128 per row; T = uint8_t: 32 per row), pair p matches frames pairs[p].first (query) and pairs[p].second;
// matches1to2[p] receives what bruteForceMatch would. Pairs the library refuses (an empty frame) come back empty with ok[p] = false.
template <typename T>
inline void bruteForceMatchBatch(const std::vector<std::vector<T>>& descriptors, const std::vector<std::pair<int, int>>& pairs,
                                 std::vector<std::vector<DMatch>>& matches1to2, bool cross_check = true, double distance_coef = 4.0,
                                 int max_size = 500, std::vector<bool>* ok = nullptr)
{
    static_assert(std::is_same<T, float>::value || std::is_same<T, uint8_t>::value, "rows of float (SIFT) or uint8_t (ORB)");
    const int kind = std::is_same<T, float>::value ? GMS_DESC_L2_F32X128 : GMS_DESC_HAMMING256;
    const size_t width = std::is_same<T, float>::value ? 128 : 32;
    static gms_ctx* ctx = nullptr;  // one context per process, created on first use
    static int ctx_rc = GMS_OK;
    static std::once_flag ctx_once;
    std::call_once(ctx_once, [] { ctx_rc = gms_ctx_create(0, &ctx); });
    if (ctx_rc != GMS_OK || !ctx) throw std::runtime_error(std::string("mi355::bruteForceMatchBatch: ") + gms_error_string(ctx_rc));
    const size_t nf = descriptors.size();
    std::vector<int64_t> frame_off(nf + 1, 0);
    for (size_t f = 0; f < nf; ++f) {
        if (descriptors[f].size() % width) throw std::invalid_argument("mi355::bruteForceMatchBatch: whole rows per frame");
        frame_off[f + 1] = frame_off[f] + (int64_t)(descriptors[f].size() / width);
    }
    std::vector<T> all((size_t)frame_off.back() * width);
    for (size_t f = 0; f < nf; ++f) std::copy(descriptors[f].begin(), descriptors[f].end(), all.begin() + frame_off[f] * (int64_t)width);
    std::vector<gms_pair> prs(pairs.size());
    int64_t total = 0;
    for (size_t p = 0; p < pairs.size(); ++p) {
        const int a = pairs[p].first, b = pairs[p].second;
        if (a < 0 || b < 0 || (size_t)a >= nf || (size_t)b >= nf) throw std::invalid_argument("mi355::bruteForceMatchBatch: frame index");
        const int64_t cap = std::min<int64_t>(frame_off[a + 1] - frame_off[a], std::max(max_size, 0));  // K never exceeds it
        prs[p] = gms_pair{a, b, (int32_t)cap, 0, total};
        total += cap;
    }
    std::vector<DMatch> out_all((size_t)std::max<int64_t>(total, 1));
    std::vector<gms_bf_result> res(pairs.size());
    const int rc = gms_bf_select_host_batch(ctx, kind, all.empty() ? nullptr : all.data(), frame_off.data(), (int)nf, prs.data(),
                                            (int)prs.size(), cross_check ? 1 : 0, distance_coef, max_size,
                                            reinterpret_cast<gms_dmatch*>(out_all.data()), res.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::bruteForceMatchBatch: ") + gms_error_string(rc));
    matches1to2.assign(pairs.size(), std::vector<DMatch>());
    if (ok) ok->assign(pairs.size(), true);
    for (size_t p = 0; p < pairs.size(); ++p) {
        if (res[p].status != GMS_OK) {
            if (ok) (*ok)[p] = false;
            continue;
        }
        matches1to2[p].assign(out_all.begin() + prs[p].match_off, out_all.begin() + prs[p].match_off + res[p].n_out);
    }
}

// The reference's stereo_match (DisparityUtil.cpp:22-49): StereoBM with its parameters (GMS_STEREO_BM_PARAMS_REFERENCE), then
// normalize(NORM_MINMAX, 0..255, CV_8U) and every 0 -> 255. The shim has no cv::Mat: images are flat row-major 8-bit grey vectors of
// width * height bytes, and so is disparity8. stereoBM gives StereoBM::compute's int16 map (4 fractional bits) for any accepted
// parameter set (include/gms.h). Both run one pair synchronously on the current HIP device (gms_stereo_bm).
inline gms_stereo_bm_params stereo_bm_reference_params()
{
    const gms_stereo_bm_params p = GMS_STEREO_BM_PARAMS_REFERENCE;
    return p;
}

namespace detail {
inline void stereo_check(const std::vector<uint8_t>& left, const std::vector<uint8_t>& right, int width, int height)
{
    if (width <= 0 || height <= 0 || left.size() != (size_t)width * (size_t)height || right.size() != left.size())
        throw std::invalid_argument("mi355::stereo_match: two width * height 8-bit images");
}
}  // namespace detail

inline void stereoBM(const std::vector<uint8_t>& left, const std::vector<uint8_t>& right, int width, int height,
                     const gms_stereo_bm_params& params, std::vector<int16_t>& disparity16)
{
    detail::stereo_check(left, right, width, height);
    disparity16.assign((size_t)width * (size_t)height, 0);
    const int rc = gms_stereo_bm(&params, left.data(), right.data(), width, height, width, disparity16.data(), nullptr, nullptr);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::stereoBM: ") + gms_error_string(rc));
}

inline void stereo_match(const std::vector<uint8_t>& left, const std::vector<uint8_t>& right, int width, int height,
                         const gms_stereo_bm_params& params, std::vector<uint8_t>& disparity8)
{
    detail::stereo_check(left, right, width, height);
    disparity8.assign((size_t)width * (size_t)height, 0);
    const int rc = gms_stereo_bm(&params, left.data(), right.data(), width, height, width, nullptr, nullptr, disparity8.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::stereo_match: ") + gms_error_string(rc));
}

inline void stereo_match(const std::vector<uint8_t>& left, const std::vector<uint8_t>& right, int width, int height,
                         std::vector<uint8_t>& disparity8)
{
    stereo_match(left, right, width, height, stereo_bm_reference_params(), disparity8);
}

// Semi-global matching on StereoBM's costs (include/gms.h) -- the library's own definition, not cv::StereoSGBM.
// stereoSGM gives the int16 map (4 fractional bits), stereo_match_sgm the 8-bit map in stereo_match's form (normalised, 0 -> 255);
// images and maps as above. Both run one pair synchronously on the current HIP device (gms_stereo_sgm).
inline gms_stereo_sgm_params stereo_sgm_reference_params()
{
    const gms_stereo_sgm_params p = GMS_STEREO_SGM_PARAMS_REFERENCE;
    return p;
}

inline void stereoSGM(const std::vector<uint8_t>& left, const std::vector<uint8_t>& right, int width, int height,
                      const gms_stereo_sgm_params& params, std::vector<int16_t>& disparity16)
{
    detail::stereo_check(left, right, width, height);
    disparity16.assign((size_t)width * (size_t)height, 0);
    const int rc = gms_stereo_sgm(&params, left.data(), right.data(), width, height, width, disparity16.data(), nullptr, nullptr);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::stereoSGM: ") + gms_error_string(rc));
}

inline void stereo_match_sgm(const std::vector<uint8_t>& left, const std::vector<uint8_t>& right, int width, int height,
                             const gms_stereo_sgm_params& params, std::vector<uint8_t>& disparity8)
{
    detail::stereo_check(left, right, width, height);
    disparity8.assign((size_t)width * (size_t)height, 0);
    const int rc = gms_stereo_sgm(&params, left.data(), right.data(), width, height, width, nullptr, nullptr, disparity8.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::stereo_match_sgm: ") + gms_error_string(rc));
}

inline void stereo_match_sgm(const std::vector<uint8_t>& left, const std::vector<uint8_t>& right, int width, int height,
                             std::vector<uint8_t>& disparity8)
{
    stereo_match_sgm(left, right, width, height, stereo_sgm_reference_params(), disparity8);
}

// Many two-view results into one frame (include/gms.h) -- the library's own step behind the batched two-view stage.
// frame_off: n_frames + 1 keypoint offsets; pairs, matches, mask, points3d (3 doubles per match slot) and two_view as the stage leaves
// them, laid out by the pairs' match_off. Runs synchronously on the current HIP device (gms_sfm_register). The cloud arrays are cut to
// the tracks they hold. Loop closure is not done; re-triangulation over all views and bundle adjustment are bundleAdjust's, below.
struct Registration {
    std::vector<gms_sfm_view> views;            // one per frame
    std::vector<gms_sfm_pair_reg> pairs;        // one per pair
    std::vector<double> points_world;           // 3 per match slot; 0 where a slot holds no point
    std::vector<int32_t> track;                 // per match slot; -1 without a track
    std::vector<double> cloud, cloud_spread;    // 3 per track; 1 per track
    std::vector<int32_t> cloud_id, cloud_obs, cloud_est;
    gms_sfm_summary summary;
};

namespace detail {
// registerViews with (gms_sfm_register_keep) or without (gms_sfm_register) a keep plane
inline Registration register_views(const std::vector<int64_t>& frame_off, const std::vector<gms_pair>& pairs, const std::vector<gms_dmatch>& matches,
                                   const std::vector<uint8_t>& mask, const std::vector<double>& points3d, const std::vector<gms_two_view>& two_view,
                                   const std::vector<uint8_t>* keep, int root, int min_links)
{
    size_t total = 0;
    for (const gms_pair& p : pairs)
        if (p.m > 0 && p.match_off >= 0) total = std::max(total, (size_t)p.match_off + (size_t)p.m);
    if (frame_off.size() < 2 || two_view.size() != pairs.size() || matches.size() < total || mask.size() < total || points3d.size() < 3 * total)
        throw std::invalid_argument("mi355::registerViews: offsets of at least one frame, one two-view record per pair, arrays that cover every pair's match range");
    if (keep && keep->size() < total) throw std::invalid_argument("mi355::registerViews: a keep plane that covers every pair's match range");
    const int n_frames = (int)frame_off.size() - 1;
    const size_t cap = frame_off.back() > 0 ? (size_t)frame_off.back() / 2 : 0;
    Registration r;
    r.views.resize((size_t)n_frames);
    r.pairs.resize(pairs.size());
    r.points_world.assign(3 * total, 0.0);
    r.track.assign(total, -1);
    r.cloud.assign(3 * cap, 0.0);
    r.cloud_spread.assign(cap, 0.0);
    r.cloud_id.assign(cap, 0);
    r.cloud_obs.assign(cap, 0);
    r.cloud_est.assign(cap, 0);
    const int rc = keep ? gms_sfm_register_keep(frame_off.data(), n_frames, pairs.data(), (int)pairs.size(), matches.data(), mask.data(),
                                                points3d.data(), two_view.data(), root, min_links, r.views.data(), r.pairs.data(),
                                                r.points_world.data(), r.track.data(), (int64_t)cap, r.cloud.data(), r.cloud_id.data(),
                                                r.cloud_obs.data(), r.cloud_est.data(), r.cloud_spread.data(), &r.summary, keep->data())
                        : gms_sfm_register(frame_off.data(), n_frames, pairs.data(), (int)pairs.size(), matches.data(), mask.data(), points3d.data(),
                                           two_view.data(), root, min_links, r.views.data(), r.pairs.data(), r.points_world.data(), r.track.data(),
                                           (int64_t)cap, r.cloud.data(), r.cloud_id.data(), r.cloud_obs.data(), r.cloud_est.data(),
                                           r.cloud_spread.data(), &r.summary);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::registerViews: ") + gms_error_string(rc));
    const size_t n = std::min(cap, (size_t)r.summary.n_tracks);
    r.cloud.resize(3 * n);
    r.cloud_spread.resize(n);
    r.cloud_id.resize(n);
    r.cloud_obs.resize(n);
    r.cloud_est.resize(n);
    return r;
}
}  // namespace detail

inline Registration registerViews(const std::vector<int64_t>& frame_off, const std::vector<gms_pair>& pairs, const std::vector<gms_dmatch>& matches,
                                  const std::vector<uint8_t>& mask, const std::vector<double>& points3d, const std::vector<gms_two_view>& two_view,
                                  int root = 0, int min_links = 8)
{
    return detail::register_views(frame_off, pairs, matches, mask, points3d, two_view, nullptr, root, min_links);
}

// One-to-one matches per pair (include/gms.h): per match slot one byte, 1 where the match is live (inside the pair's
// count, a non-zero mask byte, both indices inside their frames) and the best of the live matches on its train keypoint and of those
// on its query keypoint (distance, then position). mask and two_view may be empty: then every slot below a pair's m is live. counts,
// when given, gets {live, kept} per pair. Runs synchronously on the current HIP device (gms_match_unique). Not a maximum matching.
inline std::vector<uint8_t> uniqueMatches(const std::vector<int64_t>& frame_off, const std::vector<gms_pair>& pairs,
                                          const std::vector<gms_dmatch>& matches, const std::vector<uint8_t>& mask = {},
                                          const std::vector<gms_two_view>& two_view = {}, std::vector<int32_t>* counts = nullptr)
{
    size_t total = 0;
    for (const gms_pair& p : pairs)
        if (p.m > 0 && p.match_off >= 0) total = std::max(total, (size_t)p.match_off + (size_t)p.m);
    if (frame_off.size() < 2 || matches.size() < total || (!mask.empty() && mask.size() < total) || (!two_view.empty() && two_view.size() != pairs.size()))
        throw std::invalid_argument("mi355::uniqueMatches: offsets of at least one frame, arrays that cover every pair's match range, one two-view record per pair or none");
    std::vector<uint8_t> keep(total, 0);
    std::vector<int32_t> cnt(2 * pairs.size(), 0);
    const int rc = gms_match_unique(frame_off.data(), (int)frame_off.size() - 1, pairs.data(), (int)pairs.size(), matches.data(),
                                    mask.empty() ? nullptr : mask.data(), two_view.empty() ? nullptr : two_view.data(), keep.data(), cnt.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::uniqueMatches: ") + gms_error_string(rc));
    if (counts) *counts = cnt;
    return keep;
}

// registerViews on a keep plane (uniqueMatches'): a match whose byte is 0 feeds no track; views, pairs and points_world are the bytes
// of the call without the plane (gms_sfm_register_keep).
inline Registration registerViews(const std::vector<int64_t>& frame_off, const std::vector<gms_pair>& pairs, const std::vector<gms_dmatch>& matches,
                                  const std::vector<uint8_t>& mask, const std::vector<double>& points3d, const std::vector<gms_two_view>& two_view,
                                  const std::vector<uint8_t>& keep, int root = 0, int min_links = 8)
{
    return detail::register_views(frame_off, pairs, matches, mask, points3d, two_view, &keep, root, min_links);
}

// Bundle adjustment behind registerViews (include/gms.h): refines the views and the cloud over all the keypoints a
// track chains together. keypoints: all frames back to back (frame_off); pairs, matches and mask as registerViews took them; reg: its
// result. Runs synchronously on the current HIP device (gms_sfm_ba). The outputs have one entry per view and per cloud entry of reg.
struct BundleAdjustment {
    std::vector<gms_sfm_view> views;      // one per frame
    std::vector<double> cloud;            // 3 per cloud entry
    std::vector<int32_t> track_status;    // 0 refined, 1 two keypoints of a frame, 2 fewer than two observations, 3 kept its cloud point
    gms_sfm_ba_summary summary;
};

inline gms_sfm_ba_params bundle_default_params()
{
    gms_sfm_ba_params p = {};
    p.lambda0 = 1e-3;
    p.cg_tol = 1e-8;
    p.ftol = 1e-10;
    p.huber_px = 2.0;
    p.n_iters = 10;
    p.n_cg = 50;
    p.retriangulate = 1;
    return p;
}

inline BundleAdjustment bundleAdjust(const std::vector<gms_keypoint>& keypoints, const std::vector<int64_t>& frame_off,
                                     const std::vector<gms_pair>& pairs, const std::vector<gms_dmatch>& matches, const std::vector<uint8_t>& mask,
                                     const Registration& reg, const gms_camera& camera, const gms_sfm_ba_params& params = bundle_default_params())
{
    size_t total = 0;
    for (const gms_pair& p : pairs)
        if (p.m > 0 && p.match_off >= 0) total = std::max(total, (size_t)p.match_off + (size_t)p.m);
    const size_t cap = reg.cloud_id.size();
    if (frame_off.size() < 2 || frame_off.back() < 0 || keypoints.size() < (size_t)frame_off.back() || reg.views.size() != frame_off.size() - 1 ||
        reg.pairs.size() != pairs.size() || matches.size() < total || mask.size() < total || reg.track.size() < total || reg.cloud.size() != 3 * cap)
        throw std::invalid_argument("mi355::bundleAdjust: keypoints that cover every frame, arrays that cover every pair's match range, and the registration of the same frames and pairs");
    const int n_frames = (int)frame_off.size() - 1;
    BundleAdjustment r;
    r.views.resize((size_t)n_frames);
    r.cloud.assign(3 * cap, 0.0);
    r.track_status.assign(cap, 0);
    const int rc = gms_sfm_ba(&camera, &params, keypoints.data(), frame_off.data(), n_frames, pairs.data(), (int)pairs.size(), matches.data(),
                              mask.data(), reg.views.data(), reg.pairs.data(), reg.track.data(), (int64_t)cap, reg.cloud.data(), reg.cloud_id.data(),
                              reg.summary.n_tracks, r.views.data(), r.cloud.data(), r.track_status.data(), &r.summary);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::bundleAdjust: ") + gms_error_string(rc));
    return r;
}

// Pair records from views (include/gms.h): for any frame pairs (a, b) of a view array -- registerViews' views or
// bundleAdjust's -- the two-view records (R, unit t, status) and registration records (S, status) that the dense stage and the fusion
// read, so that they run on those poses, also for pairs the sparse stage never matched. A pair the views cannot pose (an index out of
// range, a == b, a frame that is not registered, coincident centres) gets status GMS_ERR_NO_MODEL and zeros. Runs synchronously on the
// current HIP device (gms_sfm_pair_poses).
struct PairPoses {
    std::vector<gms_pair> pairs;             // frame_a, frame_b; m and match_off 0
    std::vector<gms_two_view> two_view;      // one per pair
    std::vector<gms_sfm_pair_reg> reg;       // one per pair
};

inline PairPoses pairPosesFromViews(const std::vector<gms_sfm_view>& views, const std::vector<std::pair<int, int>>& frame_pairs)
{
    if (views.empty()) throw std::invalid_argument("mi355::pairPosesFromViews: at least one view");
    PairPoses r;
    r.pairs.resize(frame_pairs.size());
    for (size_t i = 0; i < frame_pairs.size(); ++i) {
        r.pairs[i] = gms_pair{};
        r.pairs[i].frame_a = frame_pairs[i].first;
        r.pairs[i].frame_b = frame_pairs[i].second;
    }
    r.two_view.resize(frame_pairs.size());
    r.reg.resize(frame_pairs.size());
    const int rc = gms_sfm_pair_poses(views.data(), (int)views.size(), r.pairs.data(), (int)r.pairs.size(), r.two_view.data(), r.reg.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::pairPosesFromViews: ") + gms_error_string(rc));
    return r;
}

// The image tail of the reference's createPortraitMode (DisparityUtil.cpp:317-412): img = the photograph as flat row-major BGR bytes
// (3 * width * height, cv::Mat's layout after imread), disparity = an 8-bit map with 255 = no value (what gms_disparity_device and
// stereo_match write); out receives the portrait image in img's layout. medianBlur is cv::medianBlur for 1 or 3 interleaved channels
// (ksize odd in 3..31). Both run one image synchronously on the current HIP device (gms_portrait, gms_median_blur).
inline gms_portrait_params portrait_reference_params()
{
    const gms_portrait_params p = GMS_PORTRAIT_PARAMS_REFERENCE;
    return p;
}

inline void createPortraitMode(const std::vector<uint8_t>& img, const std::vector<uint8_t>& disparity, int width, int height,
                               const gms_portrait_params& params, std::vector<uint8_t>& out)
{
    if (width <= 0 || height <= 0 || disparity.size() != (size_t)width * (size_t)height || img.size() != 3 * disparity.size())
        throw std::invalid_argument("mi355::createPortraitMode: a 3 * width * height BGR image and a width * height disparity map");
    out.assign(img.size(), 0);
    const int rc = gms_portrait(&params, img.data(), disparity.data(), width, height, out.data(), nullptr, nullptr, nullptr);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::createPortraitMode: ") + gms_error_string(rc));
}

inline void createPortraitMode(const std::vector<uint8_t>& img, const std::vector<uint8_t>& disparity, int width, int height,
                               std::vector<uint8_t>& out)
{
    createPortraitMode(img, disparity, width, height, portrait_reference_params(), out);
}

inline void medianBlur(const std::vector<uint8_t>& src, int width, int height, int channels, int ksize, std::vector<uint8_t>& dst)
{
    if (width <= 0 || height <= 0 || (channels != 1 && channels != 3) || src.size() != (size_t)width * (size_t)height * (size_t)channels)
        throw std::invalid_argument("mi355::medianBlur: a width * height image of 1 or 3 interleaved channels");
    dst.assign(src.size(), 0);
    const int rc = gms_median_blur(src.data(), width, height, channels, ksize, dst.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::medianBlur: ") + gms_error_string(rc));
}

// The image transforms of the reference's main() (main.cpp:36, :44, :114-120) on flat row-major 8-bit images of 1 or 3 interleaved
// channels: cv::resize (INTER_LINEAR), cv::warpAffine (INTER_LINEAR, BORDER_CONSTANT 0; M = the forward 2 x 3 matrix, 6 doubles
// row-major) and img_rotate (the rotation by `angle` degrees about (width / 2., height / 2.), same size). Each runs one image
// synchronously on the current HIP device (gms_resize, gms_warp_affine, gms_img_rotate).
inline void warp_check_image(const char* who, const std::vector<uint8_t>& src, int width, int height, int channels)
{
    if (width <= 0 || height <= 0 || (channels != 1 && channels != 3) || src.size() != (size_t)width * (size_t)height * (size_t)channels)
        throw std::invalid_argument(std::string(who) + ": a width * height image of 1 or 3 interleaved channels");
}

inline void resize(const std::vector<uint8_t>& src, int width, int height, int channels, int dst_width, int dst_height,
                   std::vector<uint8_t>& dst)
{
    warp_check_image("mi355::resize", src, width, height, channels);
    if (dst_width <= 0 || dst_height <= 0) throw std::invalid_argument("mi355::resize: a positive destination size");
    dst.assign((size_t)dst_width * (size_t)dst_height * (size_t)channels, 0);
    const int rc = gms_resize(src.data(), width, height, channels, dst.data(), dst_width, dst_height);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::resize: ") + gms_error_string(rc));
}

inline std::array<double, 6> getRotationMatrix2D(double center_x, double center_y, double angle, double scale)
{
    std::array<double, 6> M;
    gms_rotation_matrix_2d(center_x, center_y, angle, scale, M.data());
    return M;
}

inline void warpAffine(const std::vector<uint8_t>& src, int width, int height, int channels, const std::array<double, 6>& M, int dst_width,
                       int dst_height, std::vector<uint8_t>& dst)
{
    warp_check_image("mi355::warpAffine", src, width, height, channels);
    if (dst_width <= 0 || dst_height <= 0) throw std::invalid_argument("mi355::warpAffine: a positive destination size");
    dst.assign((size_t)dst_width * (size_t)dst_height * (size_t)channels, 0);
    const int rc = gms_warp_affine(src.data(), width, height, channels, M.data(), dst.data(), dst_width, dst_height);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::warpAffine: ") + gms_error_string(rc));
}

inline void img_rotate(const std::vector<uint8_t>& src, int width, int height, int channels, double angle, std::vector<uint8_t>& dst)
{
    warp_check_image("mi355::img_rotate", src, width, height, channels);
    dst.assign(src.size(), 0);
    const int rc = gms_img_rotate(src.data(), width, height, channels, angle, dst.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::img_rotate: ") + gms_error_string(rc));
}

// ---- a dense cloud from a posed pair ----------------------------------------------------------------------------------
// stereoRectify: the plan of X2 = R X1 + t (R 9 doubles row-major, t 3), host arithmetic; out_width / out_height <= 0: the default
// size. undistort: cv::undistort with the new camera equal to the camera. denseStereo: the plan, both images rectified, semi-global
// matching (params NULL: GMS_STEREO_SGM_PARAMS_DENSE) and every matched pixel reprojected into camera 1's frame in the unit of t.
// Images are flat row-major 8-bit, 1 or 3 interleaved channels; each call runs synchronously on the current HIP device.
inline gms_rectify_plan stereoRectify(const gms_camera& camera, const std::array<double, 9>& R, const std::array<double, 3>& t, int width,
                                      int height, int out_width = 0, int out_height = 0)
{
    gms_rectify_plan plan;
    const int rc = gms_rectify_plan_host(&camera, R.data(), t.data(), width, height, out_width, out_height, &plan);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::stereoRectify: ") + gms_error_string(rc));
    return plan;
}

inline void undistort(const std::vector<uint8_t>& src, int width, int height, int channels, const gms_camera& camera, std::vector<uint8_t>& dst)
{
    warp_check_image("mi355::undistort", src, width, height, channels);
    dst.assign(src.size(), 0);
    const int rc = gms_undistort(&camera, src.data(), width, height, channels, dst.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::undistort: ") + gms_error_string(rc));
}

struct DenseCloud {
    gms_rectify_plan plan{};
    std::vector<float> points;      // [k][3]
    std::vector<uint8_t> colors;    // [k][channels]
    std::vector<int32_t> pixel;     // [k]: v * plan.out_w + u, raster order
    std::vector<int16_t> disp16;    // [plan.out_h][plan.out_w], 4 fractional bits
    std::vector<uint8_t> rect1, rect2, valid;   // grey, [plan.out_h][plan.out_w]
    int32_t count = 0;              // all the points, also beyond cap
};

// Throws std::runtime_error with "not rectifiable" when the plan's status is GMS_ERR_NO_MODEL. cap < 0: every pixel.
inline DenseCloud denseStereo(const std::vector<uint8_t>& img1, const std::vector<uint8_t>& img2, int width, int height, int channels,
                              const gms_camera& camera, const std::array<double, 9>& R, const std::array<double, 3>& t, int min_disp16 = 16,
                              int cap = -1, const gms_stereo_sgm_params* params = nullptr)
{
    warp_check_image("mi355::denseStereo", img1, width, height, channels);
    warp_check_image("mi355::denseStereo", img2, width, height, channels);
    DenseCloud out;
    out.plan = stereoRectify(camera, R, t, width, height);
    if (out.plan.status != GMS_OK) throw std::runtime_error("mi355::denseStereo: the pair is not rectifiable");
    const size_t px = (size_t)out.plan.out_w * (size_t)out.plan.out_h;
    const int k = cap < 0 ? (int)px : cap;
    out.points.assign(3 * (size_t)k, 0.f);
    out.colors.assign((size_t)channels * (size_t)k, 0);
    out.pixel.assign((size_t)k, 0);
    out.disp16.assign(px, 0);
    out.rect1.assign(px, 0);
    out.rect2.assign(px, 0);
    out.valid.assign(px, 0);
    const int rc = gms_dense_pair(&camera, params, img1.data(), img2.data(), width, height, channels, R.data(), t.data(), out.plan.out_w,
                                  out.plan.out_h, min_disp16, &out.plan, out.rect1.data(), out.rect2.data(), out.valid.data(), nullptr,
                                  out.disp16.data(), k, out.points.data(), out.colors.data(), out.pixel.data(), &out.count);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::denseStereo: ") + gms_error_string(rc));
    const size_t n = (size_t)(out.count < k ? out.count : k);
    out.points.resize(3 * n);
    out.colors.resize((size_t)channels * n);
    out.pixel.resize(n);
    return out;
}

// ---- the speckle filter -----------------------------------------------------------------------------------------------
// cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) for a CV_16S map, in cv's argument order: disp is a flat row-major int16
// map [height][width], filtered in place by gms_filter_speckles, synchronously on the current HIP device. maxDiff is in the map's
// own units (sixteenths of a pixel for stereoBM's and stereoSGM's maps, whose newVal is (min_disparity - 1) * 16). Returns the number
// of pixels changed.
inline int filterSpeckles(std::vector<int16_t>& disp, int width, int height, int newVal, int maxSpeckleSize, int maxDiff)
{
    if (width <= 0 || height <= 0 || disp.size() != (size_t)width * (size_t)height)
        throw std::invalid_argument("mi355::filterSpeckles: a width * height int16 map");
    int32_t removed = 0;
    const int rc = gms_filter_speckles(disp.data(), width, height, newVal, maxSpeckleSize, maxDiff, &removed);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::filterSpeckles: ") + gms_error_string(rc));
    return removed;
}

// ---- the clouds of several posed pairs fused into one by depth consistency --------------------------------------------
// A source is one pair's output of the dense stage (what denseStereo returns holds plan, points, colors, disp16 and valid), with the
// view of the pair's frame_a (x_camera = R x_world + t) and the pair's registration when the clouds were made in a world frame.
// fuseDense runs gms_dense_fuse on them, synchronously on the current HIP device: a point is kept once, by the lowest source whose own
// map agrees with it, with the number of sources that agree (support) and disagree (conflict). neighbors: [n][n_nb] source indices
// (-1: empty), empty: every other source, which needs at most 33 sources. fused_cap < 0: room for all.
struct FuseSource {
    gms_rectify_plan plan{};
    int width = 0, height = 0;      // the maps' size; 0: plan.out_w, plan.out_h
    std::vector<int16_t> disp16;    // [height][width]
    std::vector<uint8_t> valid;     // [height][width]
    std::vector<float> points;      // [cap][3]
    std::vector<uint8_t> colors;    // [cap][channels], or empty
    int32_t count = -1;             // < 0: every point of `points`
    int filtered16 = -16, min_disp16 = 16;
    bool has_view = false, has_reg = false;
    gms_sfm_view view{};
    gms_sfm_pair_reg reg{};
};
struct FusedCloud {
    std::vector<float> points;      // [k][3]
    std::vector<uint8_t> colors;    // [k][channels]
    std::vector<int32_t> source, index;   // [k]: the source and the point's index in it
    std::vector<uint8_t> support, conflict;
    std::vector<int32_t> counts;    // [n + 1]: kept per source, then the total (also beyond fused_cap)
};

inline FusedCloud fuseDense(const std::vector<FuseSource>& sources, int channels = 1, int tol16 = 16, int min_support = 1, long long fused_cap = -1,
                            const std::vector<int32_t>& neighbors = {}, int n_nb = 0)
{
    const size_t n = sources.size();
    if (n == 0) throw std::runtime_error("mi355::fuseDense: at least one source");
    std::vector<int32_t> nb = neighbors;
    if (nb.empty()) {
        if (n > 33) throw std::runtime_error("mi355::fuseDense: more than 33 sources need a neighbour table");
        n_nb = n > 1 ? (int)n - 1 : 1;
        nb.assign(n * (size_t)n_nb, -1);
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0, q = 0; j < n; ++j)
                if (j != i) nb[i * (size_t)n_nb + q++] = (int32_t)j;
    }
    if (n_nb < 1 || nb.size() != n * (size_t)n_nb) throw std::runtime_error("mi355::fuseDense: neighbors: [n][n_nb]");
    std::vector<gms_dense_fuse_src> tab(n);
    std::vector<int32_t> counts_in(n);
    long long total_cap = 0;
    for (size_t i = 0; i < n; ++i) {
        const FuseSource& s = sources[i];
        const int w = s.width > 0 ? s.width : s.plan.out_w, h = s.height > 0 ? s.height : s.plan.out_h;
        const size_t px = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0), cap = s.points.size() / 3;
        if (px == 0 || s.disp16.size() != px || s.valid.size() != px || s.points.size() != 3 * cap ||
            (!s.colors.empty() && s.colors.size() != (size_t)channels * cap))
            throw std::runtime_error("mi355::fuseDense: a source's arrays do not fit its size");
        counts_in[i] = s.count < 0 ? (int32_t)cap : s.count;
        tab[i] = {s.disp16.data(), s.valid.data(), &s.plan, s.points.data(), s.colors.empty() ? nullptr : s.colors.data(), &counts_in[i],
                  s.has_view ? &s.view : nullptr, s.has_reg ? &s.reg : nullptr, w, h, s.filtered16, s.min_disp16, (int32_t)cap, 0};
        total_cap += (long long)cap;
    }
    const long long k = fused_cap < 0 ? total_cap : fused_cap;
    if (k > 2147483647LL) throw std::runtime_error("mi355::fuseDense: fused_cap");
    FusedCloud out;
    out.points.assign(3 * (size_t)k + 3, 0.f);
    out.colors.assign((size_t)channels * (size_t)k + 3, 0);
    out.source.assign((size_t)k + 1, 0);
    out.index.assign((size_t)k + 1, 0);
    out.support.assign((size_t)k + 1, 0);
    out.conflict.assign((size_t)k + 1, 0);
    out.counts.assign(n + 1, 0);
    const int rc = gms_dense_fuse(tab.data(), (int)n, nb.data(), n_nb, channels, tol16, min_support, (int)k, out.points.data(), out.colors.data(),
                                  out.source.data(), out.index.data(), out.support.data(), out.conflict.data(), out.counts.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::fuseDense: ") + gms_error_string(rc));
    const size_t kept = (size_t)(out.counts[n] < k ? out.counts[n] : k);
    out.points.resize(3 * kept);
    out.colors.resize((size_t)channels * kept);
    out.source.resize(kept);
    out.index.resize(kept);
    out.support.resize(kept);
    out.conflict.resize(kept);
    return out;
}

// ---- camera calibration from chessboard photographs (main.cpp:53-68, CalibrationUtil.cpp:3-53) --------------------------
// The library's own corner finder (NOT OpenCV's quad-based one), OpenCV 4.5.2's cornerSubPix in fp64, and calibrateCamera with
// flags = 0, on flat 8-bit grey images (dense rows). Points are doubles, so that nothing is rounded between the steps.
struct ImagePoint { double x = 0, y = 0; };
struct ObjectPoint { double x = 0, y = 0, z = 0; };
struct CameraCalibration {
    std::array<double, 9> K{};       // row-major
    std::array<double, 5> dist{};    // k1, k2, p1, p2, k3
    std::vector<std::array<double, 3>> rvecs, tvecs;
    double rms = 0;
};

inline void calib_check_image(const char* who, const std::vector<uint8_t>& grey, int width, int height)
{
    if (width <= 0 || height <= 0 || grey.size() != (size_t)width * (size_t)height)
        throw std::invalid_argument(std::string(who) + ": width * height grey bytes");
}

// findChessboardCorners(image, Size(nx, ny), corners): true and nx * ny corners in its order (row by row), or false
inline bool findChessboardCorners(const std::vector<uint8_t>& grey, int width, int height, const Size& patternSize, std::vector<ImagePoint>& corners)
{
    calib_check_image("mi355::findChessboardCorners", grey, width, height);
    const long long n = (long long)patternSize.width * patternSize.height;
    if (patternSize.width < 2 || patternSize.height < 2 || n > GMS_CHESS_MAX_CANDIDATES)
        throw std::invalid_argument("mi355::findChessboardCorners: a pattern of at least 2 x 2 and at most 4096 points");
    std::vector<float> pts((size_t)(2 * n));
    int found = 0;
    const int rc = gms_find_chessboard_corners(grey.data(), width, height, patternSize.width, patternSize.height, &found, pts.data());
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::findChessboardCorners: ") + gms_error_string(rc));
    corners.clear();
    if (found)
        for (long long i = 0; i < n; ++i) corners.push_back({pts[(size_t)(2 * i)], pts[(size_t)(2 * i + 1)]});
    return found != 0;
}

// cornerSubPix(image, corners, Size(5, 5), Size(-1, -1), TermCriteria(MAX_ITER + EPS, max_iter, eps)), in place
inline void cornerSubPix(const std::vector<uint8_t>& grey, int width, int height, std::vector<ImagePoint>& corners, const Size& win = Size(5, 5),
                         int max_iter = 30, double eps = 0.1)
{
    calib_check_image("mi355::cornerSubPix", grey, width, height);
    if (win.width != 5 || win.height != 5) throw std::invalid_argument("mi355::cornerSubPix: win (5, 5)");
    static_assert(sizeof(ImagePoint) == 2 * sizeof(double), "ImagePoint is two doubles");
    const int rc = gms_corner_subpix(grey.data(), width, height, corners.empty() ? nullptr : &corners[0].x, (int)corners.size(), 5, max_iter, eps, nullptr);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::cornerSubPix: ") + gms_error_string(rc));
}

// calibrateCamera(objectPoints, imagePoints, imageSize, K, dist, rvecs, tvecs) with flags = 0; the RMS reprojection error is .rms
inline CameraCalibration calibrateCamera(const std::vector<std::vector<ObjectPoint>>& objectPoints, const std::vector<std::vector<ImagePoint>>& imagePoints,
                                         const Size& imageSize)
{
    if (objectPoints.empty() || objectPoints.size() != imagePoints.size()) throw std::invalid_argument("mi355::calibrateCamera: one point set per view");
    static_assert(sizeof(ObjectPoint) == 3 * sizeof(double), "ObjectPoint is three doubles");
    std::vector<double> obj, img;
    std::vector<int32_t> counts;
    for (size_t v = 0; v < objectPoints.size(); ++v) {
        if (objectPoints[v].size() != imagePoints[v].size()) throw std::invalid_argument("mi355::calibrateCamera: as many image as object points");
        counts.push_back((int32_t)objectPoints[v].size());
        for (const ObjectPoint& o : objectPoints[v]) obj.insert(obj.end(), {o.x, o.y, o.z});
        for (const ImagePoint& i : imagePoints[v]) img.insert(img.end(), {i.x, i.y});
    }
    CameraCalibration c;
    const size_t n = counts.size();
    std::vector<double> rv(3 * n), tv(3 * n);
    const int rc = gms_calibrate_camera(obj.data(), img.data(), counts.data(), (int)n, imageSize.width, imageSize.height, c.K.data(), c.dist.data(),
                                        rv.data(), tv.data(), &c.rms);
    if (rc != GMS_OK) throw std::runtime_error(std::string("mi355::calibrateCamera: ") + gms_error_string(rc));
    for (size_t v = 0; v < n; ++v) {
        c.rvecs.push_back({rv[3 * v], rv[3 * v + 1], rv[3 * v + 2]});
        c.tvecs.push_back({tv[3 * v], tv[3 * v + 1], tv[3 * v + 2]});
    }
    return c;
}

// The reference's addChessboardPoints (CalibrationUtil.cpp:3-53) on equally sized grey images: per image findChessboardCorners, then
// cornerSubPix((5, 5), (-1, -1), (30, 0.1)); images without a board are skipped; object point i * nx + j is (i, j, 0). Returns the successes.
inline int addChessboardPoints(const std::vector<std::vector<uint8_t>>& images, int width, int height, const Size& boardSize,
                               std::vector<std::vector<ObjectPoint>>& objPtr, std::vector<std::vector<ImagePoint>>& imgPtr)
{
    std::vector<ObjectPoint> objectCorners;
    for (int i = 0; i < boardSize.height; ++i)
        for (int j = 0; j < boardSize.width; ++j) objectCorners.push_back({(double)i, (double)j, 0.0});
    int successes = 0;
    for (const std::vector<uint8_t>& image : images) {
        std::vector<ImagePoint> corners;
        if (!findChessboardCorners(image, width, height, boardSize, corners)) continue;
        cornerSubPix(image, width, height, corners, Size(5, 5), 30, 0.1);
        imgPtr.push_back(corners);
        objPtr.push_back(objectCorners);
        ++successes;
    }
    return successes;
}

}  // namespace mi355
