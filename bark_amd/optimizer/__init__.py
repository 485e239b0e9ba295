"""Drop-in for the sampling helpers of `bark.optimizer` (reference: src/bark/optimizer/), built on the leaf-space
posterior draws of `bark_amd.tree_kernels.posterior_samples`, and the acquisition scan over a candidate set that stands
in for the reference's solver-based `propose` (`acquisition`)."""

from .acquisition import (acquisition_plan, acquisition_scan, propose_batch_from_candidates,  # noqa: F401
                          propose_from_candidates, propose_mes_from_candidates)
