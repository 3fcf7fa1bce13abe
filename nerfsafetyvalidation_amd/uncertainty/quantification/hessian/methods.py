"""Levenberg-Marquardt "Hessian" of the reference (uncertainty/quantification/hessian/methods.py:158-188), same control flow:

    x = x0;  repeat max_iter times:
        g  = d func / d x  at x
        dx = solve(outer(g, g) + lambda I, -g);   hessian = outer(g, g)
        if allclose(dx, 0): break
        x = x + dx
        lambda /= 10 if func(x) < func(x0) else lambda *= 10
    return hessian                                   (outer(g, g) of the LAST iteration, not a Hessian of func)

outer(g, g) + lambda I is a rank-one update of a multiple of the identity, so in exact arithmetic the solve is dx = -g / (lambda + g.g)
(Sherman-Morrison): solver='closed_form' evaluates that and forms no n x n matrix.  The default solver='dense' repeats the
reference's float32 solve instead (see levenberg_marquardt).  The result is a RankOneHessian that materialises outer(g, g) on request.  func(x0) does not change between iterations and is evaluated once.  The comparison is made on float32 values, as the
reference's tensors are."""
import contextlib

import numpy as np
import torch


@contextlib.contextmanager
def single_thread_lapack():
    """The dense float32 solve / inverse of the reference are round-off once lambda is small, and that round-off depends on how the
    host LAPACK splits the matrix among threads: the same inputs give trace 130.4 on 8 threads and 99.97 on 1 or 4.  On one thread the
    result is a function of the inputs alone, so the dense arithmetic runs on one thread (torch's and numpy's BLAS both).
    torch.set_num_threads is a setting of the process: other host threads' CPU operators run single-threaded meanwhile."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        try:
            from threadpoolctl import threadpool_limits
        except ImportError as e:                 # numpy's BLAS would keep its own thread count, and the inverse its own round-off
            raise RuntimeError("lm_solver='dense' needs threadpoolctl to pin numpy's BLAS to one thread; "
                               "use lm_solver='closed_form' without it") from e
        with threadpool_limits(limits=1):
            yield
    finally:
        torch.set_num_threads(n)


class RankOneHessian:
    """outer(g, g) kept as g, with the closed forms of what the Bayesian-Laplace code does with it."""

    def __init__(self, g, x, branches, lambdas, dense=False):
        self.g, self.x, self.dense_arithmetic = g, x, dense
        self.branches, self.lambdas = branches, lambdas     # per iteration: func(x) < func(x0), and lambda after the update

    @property
    def shape(self):
        return (self.g.numel(), self.g.numel())

    def dense(self):
        return torch.outer(self.g, self.g)

    def regularized_inverse_f32(self, reg=1e-2):
        """np.linalg.inv of the float32 matrix outer(g, g) + reg I, as bayesian_laplace.py:91-94 computes it (float32 LAPACK on the host)"""
        g = self.g.detach().float().cpu()
        with single_thread_lapack():
            return np.linalg.inv((torch.outer(g, g) + torch.eye(g.numel()) * reg).numpy())

    def regularized_inverse_diag(self, reg=1e-2):
        """diag of inv(outer(g, g) + reg I) = (1 - g_i^2 / (reg + g.g)) / reg, float64 numpy"""
        g = self.g.detach().double().cpu().numpy()
        return (1.0 - g * g / (reg + float(g @ g))) / reg

    def regularized_inverse(self, reg=1e-2):
        """inv(outer(g, g) + reg I) = (I - outer(g, g) / (reg + g.g)) / reg, float64 numpy [n, n]"""
        g = self.g.detach().double().cpu().numpy()
        return (np.eye(g.size) - np.outer(g, g) / (reg + float(g @ g))) / reg


def _f32(v):
    return float(np.float32(float(v)))


def levenberg_marquardt(x0, func, lmbda=0.01, max_iter=200, grad_fn=None, solver="dense"):
    """solver 'dense' (default): the reference's arithmetic -- outer(g, g) + lambda I as a float32 matrix on the host and
    torch.linalg.solve, a RuntimeError of the solve multiplying lambda by 10.  Once lambda is small that solve is dominated by
    float32 round-off (condition (lambda + g.g) / lambda), and what the reference returns IS that round-off: only the same
    arithmetic reproduces it.  solver 'closed_form': dx = -g / (lambda + g.g), exact arithmetic, no matrix."""
    if solver not in ("dense", "closed_form"):
        raise ValueError(f"Unknown solver: {solver}")
    if grad_fn is None:
        def grad_fn(x):
            xg = x.detach().requires_grad_(True)
            with torch.enable_grad():
                return torch.autograd.grad(func(xg), xg)[0]
    x = x0.detach().clone()
    f0 = None
    g = torch.zeros_like(x)
    branches, lambdas = [], []
    for _ in range(max_iter):
        g_new = grad_fn(x).detach()
        if solver == "dense":
            gh = g_new.float().cpu()
            try:
                with single_thread_lapack():
                    dx = torch.linalg.solve(torch.outer(gh, gh) + lmbda * torch.eye(gh.numel()), -gh)
                dx = dx.to(x.device, x.dtype)
                g = g_new
            except RuntimeError:
                lmbda *= 10
                continue
        else:
            g = g_new
            gd = g.double()
            dx = (-gd / (lmbda + float(gd @ gd))).to(x.dtype)
        if torch.allclose(dx, torch.zeros_like(dx)):
            break
        x = x + dx
        if f0 is None:
            f0 = _f32(func(x0))
        better = _f32(func(x)) < f0
        lmbda = lmbda / 10 if better else lmbda * 10
        branches.append(bool(better))
        lambdas.append(lmbda)
    return RankOneHessian(g, x, branches, lambdas, dense=solver == "dense")
