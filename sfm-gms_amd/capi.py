"""ctypes binding of include/gms.h -> csrc/libgms_hip.so. Fails loudly if the library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))

vp, i32, i64, u64, sz, dbl, cstr, P = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_double, C.c_char_p, C.POINTER

# Every function include/gms.h declares: name -> (restype, argtypes). tests/test_host.py checks the table against the header's
# prototypes and that the built library exports every name.
SIGNATURES = {
    "gms_match": (i32, [vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, i32, i32, dbl, vp, P(i32)]),
    "gms_match_ctx": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, i32, vp, i32, i32, i32, dbl, vp, P(i32), vp]),
    "gms_ctx_create": (i32, [i32, P(vp)]),
    "gms_ctx_destroy": (i32, [vp]),
    "gms_ctx_set_stream": (i32, [vp, vp]),
    "gms_ctx_synchronize": (i32, [vp]),
    "gms_ctx_reserve": (i32, [vp, i32, i32, i32, i32]),
    "gms_ctx_query": (i32, [vp, i32, P(i64)]),
    "gms_ctx_set_option": (i32, [vp, i32, i32]),
    "gms_frame_table_bytes": (i64, [i64]),
    "gms_normalize_device": (i32, [vp, vp, vp, vp, i32, i64, vp]),
    "gms_ctx_read_side_records": (i32, [vp, vp, sz, P(i32)]),
    "gms_filter_device": (i32, [vp, vp, vp, i32, vp, i32, i32, vp, i32, i32, dbl, vp, vp, vp]),
    "gms_filter_host_batch": (i32, [vp, vp, vp, vp, i32, vp, i32, vp, i32, i32, dbl, vp, vp]),
    "gms_bf_prepared_bytes": (i64, [i32, i64, i32]),
    "gms_bf_prepare_device": (i32, [vp, i32, vp, vp, i32, i64, vp]),
    "gms_bfmatch_device": (i32, [vp, i32, vp, vp, i64, vp, i32, vp, i32, i32, vp]),
    "gms_disparity_device": (i32, [vp, vp, i32, vp, i32, vp, vp, i32, i32, i32, vp, i32, vp, vp, vp]),
    "gms_gather_points_device": (i32, [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp]),
    "gms_triangulate_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
    "gms_recover_pose_device": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
    "gms_gather_points_batch_device": (i32, [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]),
    "gms_find_essential_batch_device": (i32, [vp, vp, dbl, dbl, i32, vp, i32, vp, vp, vp, vp]),
    "gms_recover_pose_batch_device": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, vp]),
    "gms_triangulate_batch_device": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp]),
    "gms_two_view_batch_device": (i32, [vp, vp, dbl, dbl, i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "gms_disparity_batch_device": (i32, [vp, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, i64, i32, vp, i64, vp, vp]),
    "gms_sfm_plan": (i32, [vp, i32, i32, i32, vp]),
    "gms_sfm_register_workspace_bytes": (sz, [i32, i32, i64, i64]),
    "gms_sfm_register_device": (i32, [vp, vp, i32, i64, vp, vp, i32, i32, i64, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp, vp, vp, i64, vp, vp, vp,
                                      vp, vp, vp]),
    "gms_sfm_register": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
    "gms_match_unique_workspace_bytes": (sz, [i32, i64, i64]),
    "gms_match_unique_device": (i32, [vp, vp, i32, i64, vp, i32, i32, i64, vp, vp, vp, vp, sz, vp, vp]),
    "gms_match_unique": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, vp]),
    "gms_sfm_register_keep_device": (i32, [vp, vp, i32, i64, vp, vp, i32, i32, i64, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp, vp, vp, i64, vp, vp,
                                           vp, vp, vp, vp, vp]),
    "gms_sfm_register_keep": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    "gms_sfm_ba_workspace_bytes": (sz, [i32, i32, i64, i64]),
    "gms_sfm_ba_device": (i32, [vp, vp, vp, vp, vp, i32, i64, vp, i32, i64, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, sz, vp, vp, vp, vp]),
    "gms_sfm_ba": (i32, [vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]),
    "gms_sfm_pair_poses_device": (i32, [vp, vp, i32, vp, i32, vp, vp]),
    "gms_sfm_pair_poses": (i32, [vp, i32, vp, i32, vp, vp]),
    "gms_dataset_write": (i32, [cstr, vp]),
    "gms_dataset_read": (i32, [cstr, vp]),
    "gms_dataset_free": (None, [vp]),
    "gms_max_matches": (i32, []),
    "gms_last_hip_error": (i32, []),
    "gms_error_string": (cstr, [i32]),
    "gms_version": (cstr, []),
    "gms_selftest_threshold": (i32, [vp, vp, vp, vp, dbl, i32, vp]),
    "gms_selftest_five_point": (i32, [vp, vp, i32, vp, vp]),
    "gms_detect_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "gms_detect_batch_device": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp]),
    "gms_describe_device": (i32, [vp, vp, i32, i32, vp, i32, vp, sz, vp, vp]),
    "gms_logos_match": (i32, [vp, i32, vp, i32, vp, vp, vp, i64, P(i64), vp]),
    "gms_logos_table_bytes": (i64, [i64, i32, i32]),
    "gms_logos_workspace_bytes": (sz, [i64, i32, i64]),
    "gms_logos_prepare_device": (i32, [vp, vp, vp, i32, i64, vp, i32, vp, sz, vp]),
    "gms_logos_filter_device": (i32, [vp, vp, vp, i32, vp, sz, vp, vp, vp]),
    "gms_logos_words_device": (i32, [vp, i32, vp, i64, vp, i32, vp]),
    "gms_logos_host_batch": (i32, [vp, vp, vp, i32, vp, i32, vp, i32, vp, vp]),
    "gms_bf_select_workspace_bytes": (sz, [i32, i32, i64]),
    "gms_bf_select_device": (i32, [vp, i32, vp, vp, i64, vp, i32, vp, i32, i32, i32, dbl, i32, vp, sz, vp, vp, vp]),
    "gms_bf_match_select": (i32, [i32, vp, i32, vp, i32, i32, dbl, i32, vp, i64, P(i64), vp]),
    "gms_bf_select_host_batch": (i32, [vp, i32, vp, vp, i32, vp, i32, i32, dbl, i32, vp, vp]),
    "gms_stereo_bm_workspace_bytes": (sz, [i32, i32, i32, vp]),
    "gms_stereo_bm_device": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp]),
    "gms_stereo_bm_normalize_device": (i32, [vp, vp, i32, i32, i32, vp]),
    "gms_stereo_bm": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "gms_stereo_sgm_workspace_bytes": (sz, [i32, i32, i32, vp]),
    "gms_stereo_sgm_device": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp]),
    "gms_stereo_sgm": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "gms_portrait_workspace_bytes": (sz, [i32, i32, i32, vp]),
    "gms_portrait_device": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp]),
    "gms_median_blur_device": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "gms_portrait": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "gms_portrait_profile_device": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp, vp]),
    "gms_median_blur": (i32, [vp, i32, i32, i32, i32, vp]),
    "gms_resize_device": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, i32]),
    "gms_warp_affine_device": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, i32, i32]),
    "gms_rotation_matrix_2d": (i32, [dbl, dbl, dbl, dbl, vp]),
    "gms_resize": (i32, [vp, i32, i32, i32, vp, i32, i32]),
    "gms_warp_affine": (i32, [vp, i32, i32, i32, vp, vp, i32, i32]),
    "gms_img_rotate": (i32, [vp, i32, i32, i32, dbl, vp]),
    "gms_rectify_plan_host": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "gms_rectify_plan_device": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "gms_rectify_q": (i32, [vp, vp]),
    "gms_rectify_device": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, i32, i32, i32, vp]),
    "gms_rectify": (i32, [vp, vp, i32, vp, i32, i32, i32, vp, vp]),
    "gms_undistort": (i32, [vp, vp, i32, i32, i32, vp]),
    "gms_dense_cloud_workspace_bytes": (sz, [i32, i32, i32]),
    "gms_dense_cloud_device": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, i32, vp, sz, i32, vp, vp, vp, vp]),
    "gms_dense_pairs_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32, vp]),
    "gms_dense_pairs_device": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, sz, vp, vp, vp, vp, vp, vp,
                                     i32, vp, vp, vp, vp]),
    "gms_dense_pair": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    "gms_dense_fuse_workspace_bytes": (sz, [i32, i32]),
    "gms_dense_fuse_device": (i32, [vp, vp, i32, i32, vp, i32, i32, i32, i32, vp, sz, i32, vp, vp, vp, vp, vp, vp, vp]),
    "gms_dense_fuse": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "gms_filter_speckles_workspace_bytes": (sz, [i32, i32, i32]),
    "gms_filter_speckles_device": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
    "gms_filter_speckles": (i32, [vp, i32, i32, i32, i32, i32, vp]),
    "gms_dense_pairs_filtered_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32, vp]),
    "gms_dense_pairs_filtered_device": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, sz, vp, vp, vp, vp, vp,
                                              vp, i32, vp, vp, vp, vp, i32, i32, vp]),
    "gms_dense_pair_filtered": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32,
                                      vp]),
    "gms_chess_candidates_workspace_bytes": (sz, [i32, i32, i32]),
    "gms_chess_candidates_device": (i32, [vp, vp, i32, i32, i32, i32, vp, sz, vp, vp]),
    "gms_corner_subpix_device": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, dbl, vp]),
    "gms_find_chessboard_corners": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    "gms_order_chessboard": (i32, [vp, i32, i32, vp, vp]),
    "gms_corner_subpix": (i32, [vp, i32, i32, vp, i32, i32, i32, dbl, vp]),
    "gms_calibrate_camera": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "gms_pyramid_level_sizes": (i32, [i32, i32, i32, vp, vp]),
    "gms_detect_pyramid_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
    "gms_detect_pyramid_batch_device": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp]),
    "gms_pyramid_build_device": (i32, [vp, vp, i32, i32, i32, i32, vp, sz]),
    "gms_detect_pyramid_grad_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
    "gms_detect_pyramid_grad_batch_device": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp, vp]),
    "gms_describe_grad_device": (i32, [vp, vp, i32, i32, vp, i32, vp, sz, vp, vp]),
    "gms_detect_dog_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
    "gms_detect_dog_batch_device": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp, vp]),
    "gms_dog_candidates_device": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "gms_detect_dog_refined_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
    "gms_detect_dog_refined_batch_device": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp, vp]),
    "gms_dog_offsets_device": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "gms_bgr_to_gray_device": (i32, [vp, vp, i32, i32, i32, vp]),
    "gms_detect_pack_device": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "gms_logos_dict_workspace_bytes": (sz, [i32, i64, i32, i32, i32, i32]),
    "gms_logos_dict_train_device": (i32, [vp, i32, vp, vp, i32, i64, i32, i32, i32, u64, vp, sz, vp, vp, vp]),
    "gms_logos_dict_train": (i32, [i32, vp, vp, i32, i32, i32, i32, u64, vp, vp, vp]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)

_lib = None


def library_path():
    return os.path.join(_HERE, "csrc", "libgms_hip.so")


def load_library():
    """Load the HIP extension. No fallback: a missing .so is an error (build with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: the HIP extension is not built "
                          f"(run `python -c 'import __graft_entry__ as g; g.build()'`)")
    # torch (used by batch.py for device memory and streams) ships its own copy of the HIP runtime; it
    # must be the first one loaded in a process that uses both, or torch finds "no HIP GPUs". Nothing of
    # torch is called here.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib
