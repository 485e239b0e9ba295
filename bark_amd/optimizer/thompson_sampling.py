"""thompson_sampling.py:10-27 `generate_fstar_samples` on the numpy model triple.

The reference draws joint samples of the latent function at the training inputs from a gpytorch `BARKGP` (which no
longer exists) and keeps the min (or max) of each draw.  Here the draws come from the leaf-space
posterior (`posterior_samples`), whose covariance is the true scale K - K K_s^-1 K, so no non-PD warning needs
silencing, and the reduction over the sample sites runs on the device (`reduce=`)."""

from __future__ import annotations

from ..tree_kernels.tree_gps import posterior_samples


def generate_fstar_samples(model, data, domain, num_samples: int = 10, maximise: bool = False, generator=None):
    """-> (B, num_samples): the min (max with `maximise`) over the training inputs of each joint posterior draw of each
    forest sample.  model: (forest, noise, scale); data: (train_x, train_y); `domain` may be feat_types; generator: a
    torch.Generator, an int seed or None (see `posterior_samples`).  Torch train_x gives a device tensor, numpy a numpy
    array."""
    train_x, _ = data
    values, _ = posterior_samples(model, data, train_x, domain, num_samples, generator=generator,
                                  reduce="max" if maximise else "min")
    return values
