from .mll import batched_kernel_inverse, batched_mll, mll, schedule_plan  # noqa: F401
from . import quick_inverse  # noqa: F401
from .incremental import ChainBatch, ChainState, sweep_plan  # noqa: F401,E402
from .leafchain import LeafChainBatch, leafchain_plan  # noqa: F401,E402
from . import noise_scale_proposals  # noqa: F401,E402
from .tree_proposals import TreeProposalEnum, propose_trees, tree_proposals_plan  # noqa: F401,E402
from .bark_sampler import BARKTrainParams, run_bark_sampler  # noqa: F401,E402
