// capi_detect.cpp -- the C ABI of the keypoint sources (detect_kernels.hip, grad_desc_kernels.hip, dog_kernels.hip) and of the ingest
// kernels that turn photographs and per-image keypoint blocks into the tables (ingest_kernels.hip).
#include "capi_common.h"
#include "gms_kernels.h"

extern "C" {

size_t gms_detect_workspace_bytes(int width, int height, int n_images, int max_keypoints)
{
    return gms::detect_workspace_bytes(width, height, n_images, max_keypoints);
}

static bool detect_image_ok(int width, int height)
{
    return width > 2 * GMS_DETECT_BORDER && height > 2 * GMS_DETECT_BORDER && width <= 65535 && height <= 65535;
}

int gms_detect_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                            void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors, int32_t* d_counts)
{
    if (!c || n_images < 0 || max_keypoints < 0 || threshold < 0 || threshold > 254 || !detect_image_ok(width, height)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_workspace || !d_counts || (max_keypoints > 0 && (!d_keypoints || !d_descriptors))) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < gms::detect_workspace_bytes(width, height, n_images, max_keypoints)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_detect(d_images, n_images, width, height, threshold, max_keypoints, d_workspace, d_keypoints, d_descriptors, d_counts,
                                  c->stream);
    });
}

int gms_describe_device(gms_ctx* c, const uint8_t* d_image, int width, int height, gms_keypoint* d_keypoints, int n,
                        void* d_workspace, size_t workspace_bytes, uint8_t* d_descriptors, int32_t* d_status)
{
    if (!c || n < 0 || !detect_image_ok(width, height) || !d_image || !d_workspace || !d_status) return GMS_ERR_BAD_ARG;
    if (n > 0 && (!d_keypoints || !d_descriptors)) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < gms::detect_workspace_bytes(width, height, 1, 0)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_describe(d_image, width, height, d_keypoints, n, d_workspace, d_descriptors, d_status, c->stream); });
}

// ---- pyramid keypoint source (detect_kernels.hip) -------------------------------------------------------------------------------
int gms_pyramid_level_sizes(int width, int height, int n_levels, int32_t* widths, int32_t* heights)
{
    if (n_levels < 1 || n_levels > GMS_PYRAMID_MAX_LEVELS || !detect_image_ok(width, height) || !widths || !heights) return GMS_ERR_BAD_ARG;
    return gms::pyramid_level_sizes(width, height, n_levels, widths, heights);
}

int gms_pyramid_build_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int n_levels, uint8_t* d_levels,
                             size_t levels_bytes)
{
    if (!c || n_images < 0 || n_levels < 1 || n_levels > GMS_PYRAMID_MAX_LEVELS || !detect_image_ok(width, height)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    const size_t need = gms::pyramid_bytes(width, height, n_images, n_levels);
    if (!d_images || levels_bytes < need || (need > 0 && !d_levels)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_pyramid_build(d_images, n_images, width, height, n_levels, d_levels, c->stream); });
}

// what the batch calls of the keypoint source check first: the context, the counts, the detector's strength and the image size
static bool detect_scalars_ok(const gms_ctx* c, int n_images, int width, int height, int strength, int max_strength)
{
    return c && n_images >= 0 && strength >= 0 && strength <= max_strength && detect_image_ok(width, height);
}

static bool rows128_ok(const float* d_rows128) { return d_rows128 && !misaligned(d_rows128, 8); }   // the 128-float rows are stored two floats at a time

static size_t pyramid_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels, bool refined)
{
    return detect_image_ok(width, height) ? gms::detect_pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, refined) : 0;
}

// The four pyramid calls. max_strength: the bound of run.strength. rows128_bad: the caller's own rule for d_rows128 refuses it (looked at
// behind the early return of an empty batch, like every pointer).
static int detect_pyramid(gms_ctx* c, const gms::PyramidRun& run, int max_strength, const uint8_t* d_images, int n_images, int width, int height,
                          int max_keypoints, int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints,
                          uint8_t* d_descriptors, int32_t* d_counts, int32_t* d_level_counts, float* d_rows128, bool rows128_bad)
{
    if (!detect_scalars_ok(c, n_images, width, height, run.strength, max_strength) || max_keypoints < 0) return GMS_ERR_BAD_ARG;
    if (n_levels < 1 || n_levels > GMS_PYRAMID_MAX_LEVELS) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_workspace || !d_counts || !d_level_counts || rows128_bad) return GMS_ERR_BAD_ARG;
    if (max_keypoints > 0 && (!d_keypoints || !d_descriptors)) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, run.refined)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_detect_pyramid(run, d_images, n_images, width, height, max_keypoints, n_levels, d_workspace, d_keypoints, d_descriptors,
                                          max_keypoints > 0 ? d_rows128 : nullptr, d_counts, d_level_counts, c->stream);
    });
}

size_t gms_detect_pyramid_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, false);
}

int gms_detect_pyramid_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                                    int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                    int32_t* d_counts, int32_t* d_level_counts)
{
    return detect_pyramid(c, {gms::PyramidRun::kFast, threshold, false}, 254, d_images, n_images, width, height, max_keypoints, n_levels, d_workspace,
                          workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, nullptr, false);
}

// ---- gradient descriptor (grad_desc_kernels.hip): fused into the pyramid call, no workspace region of its own ----------------------
size_t gms_detect_pyramid_grad_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, false);
}

int gms_detect_pyramid_grad_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                                         int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                         int32_t* d_counts, int32_t* d_level_counts, float* d_rows128)
{
    const bool rows128_bad = max_keypoints > 0 && !rows128_ok(d_rows128);   // required, but only where a row can be written
    return detect_pyramid(c, {gms::PyramidRun::kFast, threshold, false}, 254, d_images, n_images, width, height, max_keypoints, n_levels, d_workspace,
                          workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, d_rows128, rows128_bad);
}

int gms_describe_grad_device(gms_ctx* c, const uint8_t* d_image, int width, int height, gms_keypoint* d_keypoints, int n, void* d_workspace,
                             size_t workspace_bytes, float* d_rows128, int32_t* d_status)
{
    if (!c || n < 0 || !detect_image_ok(width, height) || !d_image || !d_workspace || !d_status) return GMS_ERR_BAD_ARG;
    if (n > 0 && (!d_keypoints || !rows128_ok(d_rows128))) return GMS_ERR_BAD_ARG;
    if (workspace_bytes < gms::detect_workspace_bytes(width, height, 1, 0)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_describe_grad(d_image, width, height, d_keypoints, n, d_workspace, d_rows128, d_status, c->stream); });
}

// ---- difference-of-Gaussians detector (dog_kernels.hip): d_rows128 is optional, but never misaligned -------------------------------
size_t gms_detect_dog_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, false);   // the kernel is fused: no region of its own
}

int gms_detect_dog_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, int max_keypoints,
                                int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                int32_t* d_counts, int32_t* d_level_counts, float* d_rows128)
{
    return detect_pyramid(c, {gms::PyramidRun::kDog, contrast, false}, GMS_DOG_MAX_CONTRAST, d_images, n_images, width, height, max_keypoints, n_levels,
                          d_workspace, workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, d_rows128, misaligned(d_rows128, 8));
}

size_t gms_detect_dog_refined_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels)
{
    return pyramid_workspace_bytes(width, height, n_images, max_keypoints, n_levels, true);   // + the plane of refinement codes
}

int gms_detect_dog_refined_batch_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, int max_keypoints,
                                        int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                        int32_t* d_counts, int32_t* d_level_counts, float* d_rows128)
{
    return detect_pyramid(c, {gms::PyramidRun::kDog, contrast, true}, GMS_DOG_MAX_CONTRAST, d_images, n_images, width, height, max_keypoints, n_levels,
                          d_workspace, workspace_bytes, d_keypoints, d_descriptors, d_counts, d_level_counts, d_rows128, misaligned(d_rows128, 8));
}

int gms_dog_offsets_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, uint16_t* d_codes)
{
    if (!detect_scalars_ok(c, n_images, width, height, contrast, GMS_DOG_MAX_CONTRAST)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_codes || misaligned(d_codes, 2)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_dog_maps(d_images, n_images, width, height, contrast, nullptr, nullptr, nullptr, d_codes, c->stream); });
}

int gms_dog_candidates_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int contrast, uint8_t* d_cand)
{
    if (!detect_scalars_ok(c, n_images, width, height, contrast, GMS_DOG_MAX_CONTRAST)) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_images || !d_cand) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_dog_maps(d_images, n_images, width, height, contrast, d_cand, nullptr, nullptr, nullptr, c->stream); });
}

// ---- from photographs to the tables (ingest_kernels.hip) ----------------------------------------------------------------------------
int gms_bgr_to_gray_device(gms_ctx* c, const uint8_t* d_bgr, int n_images, int width, int height, uint8_t* d_gray)
{
    if (!c || n_images < 0 || width <= 0 || height <= 0 || width > 65535 || height > 65535) return GMS_ERR_BAD_ARG;
    if (n_images == 0) return GMS_OK;
    if (!d_bgr || !d_gray) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_bgr_to_gray(d_bgr, n_images, width, height, d_gray, c->stream); });
}

int gms_detect_pack_device(gms_ctx* c, const gms_keypoint* d_keypoint_blocks, const uint8_t* d_rows32_blocks, const float* d_rows128_blocks,
                           const int32_t* d_counts, int n_images, int max_keypoints, gms_keypoint* d_keypoints, uint8_t* d_rows32,
                           float* d_rows128, int64_t* d_frame_off)
{
    if (!c || n_images < 1 || n_images > 65535 || max_keypoints < 0 || !d_counts || !d_frame_off) return GMS_ERR_BAD_ARG;
    if ((d_rows32_blocks == nullptr) != (d_rows32 == nullptr) || (d_rows128_blocks == nullptr) != (d_rows128 == nullptr)) return GMS_ERR_BAD_ARG;
    if (max_keypoints > 0 && (!d_keypoint_blocks || !d_keypoints)) return GMS_ERR_BAD_ARG;
    for (const void* p : {(const void*)d_keypoint_blocks, (const void*)d_rows32_blocks, (const void*)d_rows128_blocks, (const void*)d_counts,
                          (const void*)d_keypoints, (const void*)d_rows32, (const void*)d_rows128})
        if (misaligned(p, 4)) return GMS_ERR_BAD_ARG;
    if (misaligned(d_frame_off, 8)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_detect_pack(d_keypoint_blocks, d_rows32_blocks, d_rows128_blocks, d_counts, n_images, max_keypoints, d_keypoints, d_rows32,
                                       d_rows128, d_frame_off, c->stream);
    });
}

}  // extern "C"
