"""uncertainty(method, ...) of the reference's uncertain.py:20-247, online branch (what NerfSimulator.step calls every step,
validation/simulators/NerfSimulator.py:110), for both values of envConfig.json's `uq_method`.

    rendered_output = (render result dict, rays_o, rays_d)        Estimator.render_for_uncertainty

"Gaussian Approximation" -> (mu_d_opt, sigma_d_opt); "Bayesian Laplace Approximation" -> (trace, root_mean_variance) of the posterior
covariance with prior N(0, 1) (uncertain.py:181-231).  X = rays_o + rays_d; the reference reshapes the rays with a hard-coded
H = W = 800, which only fixes X's shape -- the points are taken from the rays as they are.  The model's weights are not touched (the
reference overwrites and restores them).  The offline image-folder branch and the plots are not built."""
import torch

from .uncertainty.quantification.bayesian_laplace import BayesianLaplace
from .uncertainty.quantification.gaussian_approximation_density_uncertainty import GaussianApproximationDensityUncertainty

GAUSSIAN, LAPLACE = "Gaussian Approximation", "Bayesian Laplace Approximation"
NUM_PERTURBATIONS = 3          # bayesian_laplace.py:63, and the factor of NerfSimulator.reward (:172,179)


def uncertainty(method, rendered_output=None, model_to_use=None, lr=None, **fit_kwargs):
    """fit_kwargs (Bayesian Laplace only): BayesianLaplace.fit's keywords and `likelihood_gradient`."""
    if method == GAUSSIAN:
        out = rendered_output[0]
        c, d = out["rgbs"], out["sigmas"]
        if c.dim() == 2:            # run_cuda's last-iteration tensors [M,3] / [M]: one sample per row
            c = c[:, None, :]
        return GaussianApproximationDensityUncertainty(c, d.reshape(-1), out["image"]).optimize()
    if method == LAPLACE:
        if model_to_use is None or lr is None:
            raise ValueError("uncertainty: the Bayesian Laplace Approximation needs model_to_use and lr")
        d = rendered_output[0]["aggregated_density"]
        rays_o, rays_d = rendered_output[1].reshape(-1, 3), rendered_output[2].reshape(-1, 3)
        X = (rays_o + rays_d).unsqueeze(-2)                      # [n,1,3] (uncertain.py:187-189)
        lg = fit_kwargs.pop("likelihood_gradient", False)
        bl = BayesianLaplace(model_to_use, 0.0, 1.0, lr, likelihood_gradient=lg)
        with torch.autocast("cuda", enabled=False):
            bl.fit(X.detach().float(), d.detach().float(), **fit_kwargs)
        return bl.covariance_summary()
    raise ValueError(f"Unrecognized uncertainty quantification method {method}")
