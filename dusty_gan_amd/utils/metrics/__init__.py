"""Validation metrics on MI355X -- reference: utils/metrics/ (SURVEY.md §8f row 3)."""
from .cov_mmd_1nna import compute_cov_mmd_1nna  # noqa: F401
from .distance import (ChamferDistance, ChamferDistanceFunction, EarthMoverDistance, EarthMoverDistanceFunction,  # noqa: F401
                       chamfer_backward, chamfer_dir, chamfer_distance, chamfer_distance_matrix, chamfer_paired, compute_cd,
                       earth_mover_distance, earth_mover_distance_grad, emd_distance_matrix)
from .jsd import compute_jsd  # noqa: F401
from .swd import compute_swd  # noqa: F401
