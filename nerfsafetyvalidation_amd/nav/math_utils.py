"""The SO(3) helpers of nav/math_utils.py the planner needs.  They are the rollout's (rollout.py), which mirror the same functions;
`rot_matrix_to_vec` there selects the two branches of the reference's clamped arccos with torch.where instead of boolean-mask
assignment: the same values and gradients, without the host reads of boolean indexing."""
from ..rollout import rot_matrix_to_vec, skew as skew_matrix, vec_to_rot_matrix

__all__ = ["rot_matrix_to_vec", "skew_matrix", "vec_to_rot_matrix"]
