"""apex_camera_models -- MI355X-native drop-in for the reference crate's hot path.

Module layout mirrors the reference crate (`apex_camera_models::camera`,
`::util`, and apex-solver's `factors`).  Every numeric operation runs in the
HIP kernels of libacm.so (gfx950) through its C-ABI (include/acm.h); importing
this package loads that library and raises if it is missing.
"""
from . import _lib

_lib.load()  # fail loudly at import if the HIP extension is not built

from . import camera, factors, util  # noqa: E402
from .camera import (CameraModel, CameraModelError, DoubleSphereModel, EucmModel,  # noqa: E402
                     FovModel, Intrinsics, KannalaBrandtModel, PinholeModel, RadTanModel,
                     Resolution, UcmModel)
from .util import (ImageQualityMetrics, calculate_psnr, calculate_ssim,  # noqa: E402
                   compute_image_quality_metrics)
from .optimizer import (CalibrationConfig, CalibrationResult, Pose, PoseBatchConfig,  # noqa: E402
                        PoseBatchResult, TriangulationConfig, calibrate,
                        TriangulationResult, alternate_bundle_adjustment, refine_pose,
                        refine_poses, tracks_by_view, tracks_from_dense, triangulate)
from .optimizer import (PoseEstimateConfig, PoseEstimateResult, estimate_poses,  # noqa: E402
                        p3p)
from .optimizer import (RelativePoseConfig, RelativePoseResult,  # noqa: E402
                        estimate_relative_poses, relative_pose_8pt, two_view_tracks)
from .optimizer import (HomographyConfig, HomographyResult,  # noqa: E402
                        estimate_homographies, homography_4pt)
from .optimizer import (SimilarityConfig, SimilarityResult, apply_similarity,  # noqa: E402
                        estimate_similarities, similarity_3pt, similarity_compose,
                        similarity_inverse, similarity_transform_poses)

__all__ = [
    "camera", "factors", "util", "CameraModel", "CameraModelError", "DoubleSphereModel",
    "EucmModel", "FovModel", "Intrinsics", "KannalaBrandtModel", "PinholeModel", "RadTanModel",
    "Resolution", "UcmModel", "ImageQualityMetrics", "calculate_psnr", "calculate_ssim",
    "compute_image_quality_metrics", "Pose", "refine_pose", "triangulate", "tracks_from_dense",
    "TriangulationConfig", "TriangulationResult", "PoseBatchConfig", "PoseBatchResult",
    "CalibrationConfig", "CalibrationResult", "calibrate",
    "refine_poses", "tracks_by_view", "alternate_bundle_adjustment",
    "PoseEstimateConfig", "PoseEstimateResult", "estimate_poses", "p3p",
    "RelativePoseConfig", "RelativePoseResult", "estimate_relative_poses", "relative_pose_8pt",
    "two_view_tracks",
    "HomographyConfig", "HomographyResult", "estimate_homographies", "homography_4pt",
    "SimilarityConfig", "SimilarityResult", "estimate_similarities", "similarity_3pt",
    "apply_similarity", "similarity_transform_poses", "similarity_compose", "similarity_inverse",
]
