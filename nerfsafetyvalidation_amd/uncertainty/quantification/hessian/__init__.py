from .HessianApproximator import HessianApproximator
from .methods import RankOneHessian, levenberg_marquardt
