"""Host-side checks of the leaf-space posterior draws: the public names exist, the workspace query of
bark_posterior_samples_hip answers without a GPU, and the product path refuses to run without one."""
import numpy as np
import pytest

from bark_amd import _lib, synthetic

from conftest import load_golden


def test_public_names_import():
    from bark_amd.optimizer.thompson_sampling import generate_fstar_samples
    from bark_amd.tree_kernels import posterior_sample_dim, posterior_samples

    assert callable(posterior_samples) and callable(posterior_sample_dim) and callable(generate_fstar_samples)
    assert (_lib.SAMPLE_FULL, _lib.SAMPLE_MAX, _lib.SAMPLE_MIN) == (0, 1, 2)


def test_workspace_query_grows_with_chunk_and_draws():
    q = _lib.lib().bark_posterior_samples_workspace_bytes
    base = q(512, 150, 50, 4, 1000, 16)
    assert base > 0
    assert q(512, 150, 50, 8, 1000, 16) > base
    assert q(512, 150, 50, 4, 1000, 200) > base
    assert q(512, 150, 50, 4, 1000, 0) == 0 and q(512, 150, 50, 4, 0, 16) == 0


def test_sample_dim_is_the_packed_leaf_width():
    from bark_amd.tree_kernels import posterior_sample_dim

    X, y, bounds, ft = synthetic.mixed_problem(64, seed=3)
    F = synthetic.sample_prior_forests(3, 20, bounds, ft, seed=3)
    R = posterior_sample_dim(F, ft)
    assert isinstance(R, int) and R >= 20  # at least one leaf per tree
    assert posterior_sample_dim(F[:1], ft) <= R  # the widest forest sets it


def test_product_path_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bark_amd.tree_kernels import posterior_samples

    g = load_golden("g6_predict")
    from oracle import oracle as orc

    forest = orc.nodes_from_raw(g["forest"]).reshape(-1, 50, 100)
    model = (forest, g["noise"].reshape(-1), g["scale"].reshape(-1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        posterior_samples(model, (g["X"], g["y"]), g["cand"], g["feat_types"], 4)
    with pytest.raises(ValueError, match="num_samples"):
        posterior_samples(model, (g["X"], g["y"]), g["cand"], g["feat_types"], 0)
    assert np.all(g["noise"] > 0)
