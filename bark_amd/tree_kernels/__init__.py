from .posterior import (LeafPaths, LeafPosterior, fit_posterior, forest_weights, path_list, paths_plan,  # noqa: F401
                        systematic_index)
from .scores import loo_scores, predictive_scores  # noqa: F401
from .tree_gps import (  # noqa: F401
    BARKModel,
    forest_predict,
    mixture_of_gaussians_as_normal,
    posterior_sample_dim,
    posterior_samples,
)
