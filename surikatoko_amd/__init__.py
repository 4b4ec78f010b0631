"""surikatoko_amd -- MI355X-native bundle-adjustment core (drop-in for suriko's BundleAdjustmentKanatani).

Only the hot path lives here: csrc/ (HIP kernels + the C ABI of include/srk_ba.h) and a thin Python
mirror of the reference's operator interface (ba.py) used by the tests and bench.py.  There is no CPU
fallback: every compute entry point needs libsrk_ba.so and a HIP device.
"""
from ._lib import lib, library_path, build_library, LibraryNotBuilt  # noqa: F401
from .ba import (BundleAdjustmentKanatani, BundleAdjustmentKanataniTermCriteria, Report, Scene,  # noqa: F401
                 normalize_scene_inplace, check_world_is_normalized, status_string, device_count, revert_covariances,
                 revert_cross_covariances, marginalize_dense, revert_marginalization_prior, marginalization_landmarks)
from .triangulate import (triangulate_tracks, tri_status_names, default_tri_options, TRI_FEW_VIEWS, TRI_DEGENERATE,  # noqa: F401
                          TRI_BEHIND, TRI_LOW_PARALLAX, TRI_NOT_CONVERGED)
from .resect import (resect_frames, resect_status_names, default_resect_options, RESECT_FEW_POINTS, RESECT_DEGENERATE,  # noqa: F401
                     RESECT_BEHIND, RESECT_NOT_CONVERGED)
from .locate import (locate_frames, locate_status_names, default_locate_options, ransac_hypotheses, LocateResult,  # noqa: F401
                     LOCATE_FEW_POINTS, LOCATE_NO_MODEL)
from .relate import (relate_frames, relate_status_names, default_relate_options, two_view_scene, RelateResult, TwoViewScene,  # noqa: F401
                     RELATE_FEW_POINTS, RELATE_NO_MODEL)
from .pair import (refine_pairs, relative_pose_factor, pair_status_names, default_pair_options, PairResult,  # noqa: F401
                   PAIR_FEW_POINTS, PAIR_DEGENERATE, PAIR_NOT_CONVERGED)
from .align import (align_points, apply_similarity, align_status_names, default_align_options, AlignResult,  # noqa: F401
                    ALIGN_FEW_POINTS, ALIGN_NO_MODEL)
from .homography import (relate_homography, apply_homography, decompose_homography, homography_status_names,  # noqa: F401
                         default_homography_options, HomographyResult, HomographyPoses, HOMOGRAPHY_FEW_POINTS, HOMOGRAPHY_NO_MODEL)
from .fundamental import (relate_uncalibrated, epipolar_lines, pose_from_fundamental, fundamental_status_names,  # noqa: F401
                          default_fundamental_options, FundamentalResult, FUNDAMENTAL_FEW_POINTS, FUNDAMENTAL_NO_MODEL)
from .scene import (SceneSpec, generate_scene, config_scene, drop_observations, renumber_frames, loop_scene,  # noqa: F401
                    CONFIGS)
