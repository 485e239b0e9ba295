"""Drop-in for the sampling helpers of `bark.optimizer` (reference: src/bark/optimizer/), built on the leaf-space
posterior draws of `bark_amd.tree_kernels.posterior_samples`, the acquisition scan over a candidate set (`acquisition`) and
the search over the whole domain that stands in for the reference's solver-based `propose` (`domain`)."""

from .acquisition import (acquisition_plan, acquisition_scan, propose_batch_from_candidates,  # noqa: F401
                          propose_from_candidates, propose_mes_from_candidates)
from .constraints import LinearConstraints  # noqa: F401
from .domain import (CellBoxes, CellTable, cell_boxes, domain_candidates, domain_neighbours, domain_plan,  # noqa: F401
                     domain_repair, propose_from_domain, split_table)
from .fidelity import (fidelity_information_gain, fstar_at_fidelity, information_gain,  # noqa: F401
                       propose_fidelity_information_based, with_fidelity)
from .thompson_sampling import (propose_thompson_from_candidates, propose_thompson_from_domain,  # noqa: F401
                                thompson_forests)
