"""MI355X-native GMS match filter -- host-side mirror of the reference's boundary.

The reference's hot path is one call, ``cv::xfeatures2d::matchGMS`` (call sites
``SfM-GMS/SfM-GMS/FeatureMatchUtil.cpp:69`` and ``DisparityUtil.cpp:149,299``). This package is the
Python face of the C ABI in ``include/gms.h``; every compute call goes through
``csrc/libgms_hip.so`` (hand-written HIP for gfx950). There is no CPU fallback: importing works
without a GPU, computing does not.

The directory name has a dash (it is fixed by the project layout), so load it with
``importlib.import_module("sfm-gms_amd")``.
"""
from .types import (KEYPOINT_DTYPE, DMATCH_DTYPE, PAIR_DTYPE, RESULT_DTYPE, LOGOS_RESULT_DTYPE, LOGOS_DICT_RESULT_DTYPE, BF_RESULT_DTYPE, GmsError,  # noqa: F401
                    GMS_DESC_HAMMING256, GMS_DESC_L2_F32X128, GMS_DETECT_BORDER, STEREO_BM_PARAMS_DTYPE, stereo_bm_params,
                    STEREO_SGM_PARAMS_DTYPE, stereo_sgm_params,
                    PORTRAIT_PARAMS_DTYPE, portrait_params)
from .capi import load_library, library_path, EXPORTED_SYMBOLS  # noqa: F401
from .api import matchGMS, matchLOGOS, trainLogosDictionary, bruteForceMatch, stereoBM, stereo_match, stereoSGM, stereo_match_sgm, portraitMode, medianBlur, structureFromMotion, GmsContext  # noqa: F401
from .api import resize, warpAffine, getRotationMatrix2D, imgRotate  # noqa: F401
from .api import findChessboardCorners, cornerSubPix, calibrateCamera, addChessboardPoints, chessboardObjectPoints  # noqa: F401
from .types import CHESS_CANDIDATE_DTYPE  # noqa: F401
from .api import structureFromMotionMulti, registerViews, sfm_plan, uniqueMatches  # noqa: F401
from .types import SFM_PLAN_DTYPE, SFM_VIEW_DTYPE, SFM_PAIR_REG_DTYPE, SFM_SUMMARY_DTYPE, GMS_SFM_SKIPPED  # noqa: F401
from .api import bundleAdjust  # noqa: F401
from .api import stereoRectify, rectifyQ, rectify, undistort, denseStereo, denseFuse, filterSpeckles  # noqa: F401
from .types import DENSE_FUSE_SRC_DTYPE, dense_fuse_neighbors  # noqa: F401
from .types import RECTIFY_PLAN_DTYPE, RectifyPlan  # noqa: F401
from .types import (SFM_BA_PARAMS_DTYPE, SFM_BA_SUMMARY_DTYPE, SFM_BA_REFINED, SFM_BA_MULTI, SFM_BA_FEW, SFM_BA_KEPT, SFM_BA_DEFAULTS,  # noqa: F401
                    sfm_ba_params)
from .sharding import all_pairs_count, pair_from_index, shard_range  # noqa: F401

__all__ = [
    "KEYPOINT_DTYPE", "DMATCH_DTYPE", "PAIR_DTYPE", "RESULT_DTYPE", "LOGOS_RESULT_DTYPE", "BF_RESULT_DTYPE", "GmsError",
    "load_library", "library_path", "EXPORTED_SYMBOLS", "matchGMS", "matchLOGOS", "trainLogosDictionary", "LOGOS_DICT_RESULT_DTYPE", "bruteForceMatch", "stereoBM", "stereo_match",
    "STEREO_BM_PARAMS_DTYPE", "stereo_bm_params", "GmsContext",
    "stereoSGM", "stereo_match_sgm", "STEREO_SGM_PARAMS_DTYPE", "stereo_sgm_params",
    "portraitMode", "medianBlur", "structureFromMotion", "resize", "warpAffine", "getRotationMatrix2D", "imgRotate", "PORTRAIT_PARAMS_DTYPE", "portrait_params",
    "findChessboardCorners", "cornerSubPix", "calibrateCamera", "addChessboardPoints", "chessboardObjectPoints", "CHESS_CANDIDATE_DTYPE",
    "structureFromMotionMulti", "registerViews", "sfm_plan", "uniqueMatches", "SFM_PLAN_DTYPE", "SFM_VIEW_DTYPE", "SFM_PAIR_REG_DTYPE", "SFM_SUMMARY_DTYPE",
    "GMS_SFM_SKIPPED", "bundleAdjust", "SFM_BA_PARAMS_DTYPE", "SFM_BA_SUMMARY_DTYPE", "SFM_BA_REFINED", "SFM_BA_MULTI", "SFM_BA_FEW",
    "SFM_BA_KEPT", "SFM_BA_DEFAULTS", "sfm_ba_params",
    "stereoRectify", "rectifyQ", "rectify", "undistort", "denseStereo", "denseFuse", "filterSpeckles", "DENSE_FUSE_SRC_DTYPE", "dense_fuse_neighbors", "RECTIFY_PLAN_DTYPE", "RectifyPlan",
    "all_pairs_count", "pair_from_index", "shard_range", "GMS_DESC_HAMMING256", "GMS_DESC_L2_F32X128", "GMS_DETECT_BORDER",
]
