from .posterior import LeafPosterior, fit_posterior  # noqa: F401
from .scores import loo_scores, predictive_scores  # noqa: F401
from .tree_gps import (  # noqa: F401
    BARKModel,
    forest_predict,
    mixture_of_gaussians_as_normal,
    posterior_sample_dim,
    posterior_samples,
)
