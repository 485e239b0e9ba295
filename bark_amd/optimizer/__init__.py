"""Drop-in for the sampling helpers of `bark.optimizer` (reference: src/bark/optimizer/), built on the leaf-space
posterior draws of `bark_amd.tree_kernels.posterior_samples`."""
