"""Dispatcher of the Hessian approximations (reference: uncertainty/quantification/hessian/HessianApproximator.py:4-42).

Only 'levenberg_marquardt' is built: it is the one method the reference's BayesianLaplace constructs (bayesian_laplace.py:33).  The
other four names the reference knows are refused by name; anything else is the reference's ValueError."""
from .methods import levenberg_marquardt

_NOT_BUILT = ("finite_difference", "bfgs", "regression_gradient", "regression_gradient_regularized")


class HessianApproximator:
    def __init__(self, func, method="finite_difference", epsilon=1e-8, delta=1e-6, alpha=0.1, lmbda=0.01, grad_fn=None, max_iter=200, solver="dense"):
        """func: x -> loss.  grad_fn: x -> d loss / d x as the caller defines it (None: autograd of func)."""
        self.func, self.method, self.epsilon, self.delta, self.alpha, self.lmbda = func, method, epsilon, delta, alpha, lmbda
        self.grad_fn, self.max_iter, self.solver = grad_fn, max_iter, solver

    def compute(self, x):
        if self.method == "levenberg_marquardt":
            return levenberg_marquardt(x, self.func, lmbda=self.lmbda, max_iter=self.max_iter, grad_fn=self.grad_fn, solver=self.solver)
        if self.method in _NOT_BUILT:
            raise NotImplementedError(f"Hessian method '{self.method}' is not built: the Bayesian-Laplace fit only reaches 'levenberg_marquardt'")
        raise ValueError(f"Unknown method: {self.method}")
