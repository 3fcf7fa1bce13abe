"""Bayesian-Laplace approximation of the sigma net's posterior (reference: uncertainty/quantification/bayesian_laplace.py:18-123,
called from uncertain.py:181-231 with X = rays_o + rays_d and y = aggregated_density of a render).

    L(theta) = 0.5 sum (theta - prior_mean)^2 / prior_std^2 + 0.5 sum_i (y_i - sigma(X_i; theta))^2

is minimised by Adam (StepLR 100 / 0.1) from a random theta over `num_perturbations` noisy copies of X; Levenberg-Marquardt on the
unperturbed X then yields the "Hessian" whose regularised inverse is the posterior covariance.  DESIGN.md "Bayesian-Laplace" lists
what the reference really computes; with `likelihood_gradient=False` (the default) this class computes the same:
  * the likelihood enters through the loss VALUE only: log_likelihood writes theta into the model with `param.data.copy_`, so the
    gradient of the loss with respect to theta is the prior term (theta - prior_mean) / prior_std^2, for Adam and for LM alike;
  * `minTheta = theta` aliases the tensor Adam updates in place: the posterior mean is the FINAL theta of the last perturbation in
    which some step lowered the running minimum, not the theta at that minimum.
`likelihood_gradient=True` follows the gradient of the whole posterior instead (trunc_exp's clamped backward included).

Two paths.  The torch path evaluates `model.density` with theta substituted for `model.sigma_net.parameters()` (functional_call:
the model's weights are never written) on any device and backbone.  The fused path -- the fp32 nn.Linear 32 -> 64 -> 16 sigma net
on a HIP device outside autocast, the conditions of NeRFNetwork.fused_model() with f32 -- encodes X once per perturbation through
the grid encoder and runs every evaluation and optimiser step as launches of csrc/sigma_fit.hip; the host reads the loss history and
the improvement flag once per perturbation."""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from .hessian import HessianApproximator

_FUSED_SHAPES = [(64, 32), (16, 64)]
MODE_LOSS, MODE_PRIOR_GRAD, MODE_FULL_GRAD = 0, 1, 2


def step_lrs(lr, n_steps, step_size=100, gamma=0.1):
    """the learning rate of every step under StepLR(step_size, gamma): multiplied recursively, as torch's scheduler does"""
    out, cur = [], float(lr)
    for k in range(n_steps):
        out.append(cur)
        if (k + 1) % step_size == 0:
            cur = cur * gamma
    return out


class _Density(nn.Module):
    """model.density as a Module's forward, so that torch.func.functional_call can substitute the sigma net's parameters"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model.density(x)["sigma"]


def sigma_fit_eval(features, y, theta, prior_mean, prior_std, mode, max_workgroups=0):
    """csrc/sigma_fit.hip on device tensors: features [n,32], y [n], theta [3072] (float32) -> (loss float64 0-dim tensor, grad [3072] or None)"""
    n = features.shape[0]
    if features.dtype != torch.float32 or features.shape[1:] != (32,) or y.dtype != torch.float32 or y.numel() != n or theta.dtype != torch.float32 or theta.numel() != 3072:
        raise RuntimeError("sigma_fit_eval: features float32 [n,32], y float32 [n], theta float32 [3072]")
    if not (features.is_contiguous() and y.is_contiguous() and theta.is_contiguous()) or not (features.device == y.device == theta.device):
        raise RuntimeError("sigma_fit_eval: features, y and theta must be contiguous tensors on one device")
    work, wbytes = _lib.workspace("sigma_fit", n, max_workgroups, device=features.device)
    if work is None:                  # a max_workgroups the library refuses: a buffer all the same, so that its message names the reason
        work = torch.empty(8, dtype=torch.uint8, device=features.device)
    loss = torch.empty((), dtype=torch.float64, device=features.device)
    grad = torch.empty(3072, dtype=torch.float32, device=features.device) if mode != MODE_LOSS else None
    _lib.call("sigma_fit_eval", features, y, n, theta, float(prior_mean), float(prior_std) ** 2, mode, max_workgroups, work, wbytes, loss,
              grad)
    return loss, grad


class BayesianLaplace:
    def __init__(self, model, prior_mean, prior_std, lr, likelihood_gradient=False):
        self.model = model
        self.prior_mean, self.prior_std, self.lr = float(prior_mean), float(prior_std), lr
        self.likelihood_gradient = bool(likelihood_gradient)
        self.hessian_approximator = HessianApproximator(self.negative_log_posterior_hessian_wrapper, method="levenberg_marquardt",
                                                        grad_fn=self._hessian_grad)
        self.X = self.y = None
        self._names = [n for n, _ in model.sigma_net.named_parameters()]
        self._shapes = [tuple(p.shape) for p in model.sigma_net.parameters()]
        self._density = _Density(model)
        self._feat = None          # fused path: encoder features of self.X

    # ---- the objective ---------------------------------------------------------------------------------------------------
    def num_params(self):
        return sum(int(np.prod(s)) for s in self._shapes)

    def _device(self):
        return next(self.model.sigma_net.parameters()).device

    def _params(self, theta):
        out, start = {}, 0
        for name, shape in zip(self._names, self._shapes):
            end = start + int(np.prod(shape))
            out["model.sigma_net." + name] = theta[start:end].view(shape)
            start = end
        return out

    def _prior(self, theta):
        d = theta - self.prior_mean
        return 0.5 * torch.sum(d ** 2 / self.prior_std ** 2), d / self.prior_std ** 2

    def loss_and_grad(self, theta, X, y):
        """torch path: (L(theta) as a 0-dim tensor, the gradient Adam and LM are handed).  The density is always evaluated under autograd
        with theta requiring a gradient, so that a model with a fused inference path takes its operators (which see theta) and not a
        snapshot of its own weights."""
        theta = theta.detach()
        prior, prior_grad = self._prior(theta)
        th = theta.clone().requires_grad_(True)
        with torch.enable_grad():
            sigma = torch.func.functional_call(self._density, self._params(th), (X,)).reshape(-1).float()
            lik = 0.5 * torch.sum((y.reshape(-1) - sigma) ** 2)
        if self.likelihood_gradient:
            grad = prior_grad + torch.autograd.grad(lik, th)[0]
        else:
            grad = prior_grad                      # the reference's graph ends at the model's parameters, not at theta
        return (prior + lik.detach()), grad

    def negative_log_posterior(self, theta, X, y):
        if isinstance(theta, np.ndarray):
            theta = torch.from_numpy(theta).to(self._device())
        return self.loss_and_grad(theta, X, y)[0]

    def log_posterior(self, theta, X, y):
        return -self.negative_log_posterior(theta, X, y)

    def negative_log_posterior_hessian_wrapper(self, xt):
        if self._feat is not None:
            return sigma_fit_eval(self._feat, self.y, xt.contiguous(), self.prior_mean, self.prior_std, MODE_LOSS)[0]
        return self.negative_log_posterior(xt, self.X, self.y)

    def _hessian_grad(self, xt):
        if not self.likelihood_gradient:
            return (xt - self.prior_mean) / self.prior_std ** 2
        if self._feat is not None:
            return sigma_fit_eval(self._feat, self.y, xt.contiguous(), self.prior_mean, self.prior_std, MODE_FULL_GRAD)[1]
        return self.loss_and_grad(xt, self.X, self.y)[1]

    # ---- path selection --------------------------------------------------------------------------------------------------
    def uses_fused_path(self, X):
        m = self.model
        if not X.is_cuda or torch.is_autocast_enabled("cuda") or not hasattr(m, "fused_model") or not hasattr(m, "encoder"):
            return False
        ps = list(m.sigma_net.parameters())
        if [tuple(p.shape) for p in ps] != _FUSED_SHAPES or any(p.dtype != torch.float32 for p in ps) or not getattr(m, "fused", True):
            return False
        fm = m.fused_model()
        return fm is not None and bool(fm.f32)

    def _encode(self, X):
        with torch.no_grad():
            return self.model.encoder(X.reshape(-1, 3), bound=self.model.bound).float().contiguous()

    # ---- the fit ---------------------------------------------------------------------------------------------------------
    def fit(self, X, y, theta_init=None, perturbations=None, generator=None, n_steps=1000, num_perturbations=3, perturbation_scale=0.3,
            lm_max_iter=200, lm_solver="dense"):
        dev = self._device()
        X = torch.as_tensor(X, dtype=torch.float32).to(dev)
        y = torch.as_tensor(y, dtype=torch.float32).to(dev)
        n = X.numel() // 3
        if y.numel() != n:
            raise ValueError(f"BayesianLaplace.fit: y holds {y.numel()} values for {n} points")
        P = self.num_params()
        # the reference's draws, in its order (bayesian_laplace.py:58,65): theta ~ N(0, 1), then the perturbations ~ N(0, 1) * scale
        if theta_init is None:
            theta_init = torch.randn(P, device=dev, generator=generator)
        theta_init = torch.as_tensor(theta_init, dtype=torch.float32).to(dev).reshape(P).clone()
        if perturbations is None:
            perturbations = torch.randn((num_perturbations,) + tuple(X.shape), device=dev, generator=generator) * perturbation_scale
        perturbations = torch.as_tensor(perturbations, dtype=torch.float32).to(dev)
        X_perturbed = X.unsqueeze(0) + perturbations
        fused = self.uses_fused_path(X)
        self.fused = fused
        y_flat = y.reshape(-1).contiguous()
        min_loss = torch.full((), float("inf"), dtype=torch.float32, device=dev)
        lrs = step_lrs(self.lr, n_steps)
        history, chosen, min_theta = [], -1, theta_init
        for p, X_p in enumerate(X_perturbed):
            run = self._fit_fused if fused else self._fit_torch
            theta, hist, improved, min_loss = run(X_p, y_flat, theta_init, lrs, min_loss)
            history.append(hist)
            if improved:                           # `minTheta = theta`: the tensor the optimiser went on updating (:79-81)
                chosen, min_theta = p, theta
        self.loss_history = np.stack(history) if history else np.zeros((0, n_steps), np.float32)
        self.chosen_perturbation = chosen
        self.min_loss = float(min_loss)
        self.posterior_mean = min_theta.detach().cpu().numpy()
        self.X, self.y = X, y_flat
        self._feat = self._encode(X) if fused else None
        self.hessian_approximator.max_iter, self.hessian_approximator.solver = lm_max_iter, lm_solver
        self.hessian = self.hessian_approximator.compute(min_theta.detach())
        self._posterior_cov = None
        return self

    def _fit_torch(self, X_p, y, theta_init, lrs, min_loss):
        theta = theta_init.clone().detach().requires_grad_(True)
        optimizer = torch.optim.Adam([theta], lr=self.lr)
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=100, gamma=0.1)
        hist = torch.empty(len(lrs), dtype=torch.float32, device=theta.device)
        improved = torch.zeros((), dtype=torch.bool, device=theta.device)
        for k in range(len(lrs)):
            loss, grad = self.loss_and_grad(theta, X_p, y)
            theta.grad = grad
            optimizer.step()
            scheduler.step()
            loss = loss.float()
            hist[k] = loss
            better = loss < min_loss               # on the loss before the step (:75-81); no host read inside the loop
            min_loss = torch.where(better, loss, min_loss)
            improved = improved | better
        return theta.detach(), hist.cpu().numpy(), bool(improved), min_loss

    def _fit_fused(self, X_p, y, theta_init, lrs, min_loss):
        dev = theta_init.device
        feat = self._encode(X_p)
        n = feat.shape[0]
        theta = theta_init.clone().contiguous()
        grad, m, v = torch.empty_like(theta), torch.zeros_like(theta), torch.zeros_like(theta)
        hist = torch.empty(len(lrs), dtype=torch.float32, device=dev)
        improved = torch.zeros(1, dtype=torch.int32, device=dev)
        min_loss = min_loss.clone()
        work, wbytes = _lib.workspace("sigma_fit", n, 0, device=dev)
        mode = MODE_FULL_GRAD if self.likelihood_gradient else MODE_PRIOR_GRAD
        args = (feat, y, n, theta, self.prior_mean, self.prior_std ** 2, mode, 0, work, wbytes, grad, m, v)
        for k, lr in enumerate(lrs):               # launches only; the one read-back follows the loop
            _lib.call("sigma_fit_step", *args, lr, k + 1, min_loss, improved, hist, k)
        return theta, hist.cpu().numpy(), bool(int(improved.item())), min_loss

    # ---- results ---------------------------------------------------------------------------------------------------------
    def predict(self, X):
        return self.model.forward(X)

    def get_posterior_mean(self):
        return self.posterior_mean

    def get_posterior_cov(self):
        """inv(outer(g, g) + 1e-2 I) of :91-94 [n, n]: the reference's float32 inverse after its dense LM, the closed form (float64)
        after lm_solver='closed_form'"""
        if self._posterior_cov is None:
            h = self.hessian
            self._posterior_cov = h.regularized_inverse_f32(1e-2) if h.dense_arithmetic else h.regularized_inverse(1e-2)
        return self._posterior_cov

    def covariance_summary(self):
        """uncertain.py:199-212: diagonal clamped at 0, trace / n, sqrt(mean(diag)) / n (from the diagonal alone in the closed form)"""
        if self.hessian.dense_arithmetic:
            cov = self.get_posterior_cov().copy()
            n = cov.shape[0]
            idx = np.diag_indices(n)
            cov[idx] = np.maximum(0, cov[idx])
            return float(np.trace(cov) / n), float(np.sqrt(np.mean(np.diag(cov))) / n)
        diag = np.maximum(0, self.hessian.regularized_inverse_diag(1e-2))
        n = diag.size
        return float(diag.sum() / n), float(np.sqrt(diag.mean()) / n)
