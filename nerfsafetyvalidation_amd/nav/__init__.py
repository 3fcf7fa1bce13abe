"""The reference's trajectory planner (nav/quad_plot.py, nav/quad_helpers.py), with the collision term of its cost as a fused
HIP kernel (density_query), and its NeRF state estimator (nav/estimator_helpers.py) with a HIP keypoint detector."""
from .math_utils import rot_matrix_to_vec, skew_matrix, vec_to_rot_matrix
from .quad_helpers import astar, next_rotation
from .estimator import Estimator, estimator_config
from .quad_plot import DensityQuery, Planner, density_query

__all__ = ["DensityQuery", "Estimator", "Planner", "estimator_config", "astar", "density_query", "next_rotation", "rot_matrix_to_vec", "skew_matrix", "vec_to_rot_matrix"]
