"""The byte queries of the leaf-space entry points and of the calls on a fitted state, replayed against a table recorded from
the library before its host drivers were reorganised (tests/golden/leaf_workspace_bytes.json).  A layout is the sum of its
areas, so a query that still answers every row of the table still carves the same workspace.  No GPU.

`python tests/test_workspace_layout_cpu.py` rewrites the table from the library that is built: only for a change that means
to alter a layout."""
import itertools
import json
import os

import pytest

from bark_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leaf_workspace_bytes.json")

N, R, M, BC, B = [1, 200], [1, 31, 32, 33, 141, 8192], [1, 13, 64], [1, 3], [1, 5]
C, P, Q, FLAG, VARIANT = [1, 256, 65536, 65537], [0, 1, 64], [0, 16], [0, 1], [0, 1, 2]
# query -> the values each of its arguments takes, in the order of its signature; a query is asked at their product, the last
# argument running fastest
GRID = {
    "bark_mll_leafspace_workspace_bytes": [N, R, M, BC, [0] + C],
    "bark_kernel_inverse_leafspace_workspace_bytes": [N, R, M, BC],
    "bark_posterior_samples_workspace_bytes": [N, R, M, BC, C, [1, 7]],
    "bark_noise_scale_step_chains_workspace_bytes": [N, R, M, BC],
    "bark_acquisition_scan_workspace_bytes": [N, R, M, BC, C],
    "bark_acquisition_scan_pending_workspace_bytes": [N, R, M, BC, C, P],
    "bark_acquisition_scan_targets_workspace_bytes": [N, R, M, BC, C, P],
    "bark_predictive_scores_workspace_bytes": [N, R, M, BC, C],
    "bark_leaf_posterior_bytes": [R, M, B],
    "bark_leaf_posterior_fit_workspace_bytes": [N, R, M, BC],
    "bark_acquisition_scan_fitted_workspace_bytes": [R, M, BC, C, P, VARIANT],
    "bark_acquisition_scan_fitted_weighted_workspace_bytes": [R, M, BC, C, P, VARIANT],
    "bark_leaf_posterior_condition_workspace_bytes": [R, M, BC, P],
    "bark_leaf_posterior_observe_workspace_bytes": [R, M, BC, P],
    "bark_fidelity_gain_fitted_workspace_bytes": [R, M, BC, C, [1, 1024]],
    "bark_leaf_posterior_predict_workspace_bytes": [R, M, B, BC, C, Q, FLAG, FLAG, VARIANT],
    "bark_leaf_posterior_paths_workspace_bytes": [[1, 31, 32, 33, 141, 2048], M, B, [1, 64], FLAG],
    "bark_path_scan_workspace_bytes": [[1, 31, 32, 33, 141, 2048], M, [1, 64], C, VARIANT],
}
# one shape per query that it must refuse
REFUSED = {
    "bark_mll_leafspace_workspace_bytes": (200, 141, 13, 3, -1),
    "bark_kernel_inverse_leafspace_workspace_bytes": (0, 141, 13, 3),
    "bark_posterior_samples_workspace_bytes": (200, 141, 13, 3, 256, 0),
    "bark_noise_scale_step_chains_workspace_bytes": (200, 141, 13, 0),
    "bark_acquisition_scan_workspace_bytes": (200, 141, 13, 3, 0),
    "bark_acquisition_scan_pending_workspace_bytes": (200, 141, 13, 3, 256, 65),
    "bark_acquisition_scan_targets_workspace_bytes": (200, 141, 13, 3, 256, -1),
    "bark_predictive_scores_workspace_bytes": (200, 0, 13, 3, 256),
    "bark_leaf_posterior_bytes": (8193, 13, 5),
    "bark_leaf_posterior_fit_workspace_bytes": (200, 141, 65, 3),
    "bark_acquisition_scan_fitted_workspace_bytes": (141, 13, 3, (1 << 24) + 1, 1, 0),
    "bark_acquisition_scan_fitted_weighted_workspace_bytes": (141, 13, 3, 256, 1, 3),
    "bark_leaf_posterior_condition_workspace_bytes": (141, 13, 3, 65),
    "bark_leaf_posterior_observe_workspace_bytes": (141, 65, 3, 1),
    "bark_fidelity_gain_fitted_workspace_bytes": (141, 13, 3, 65537, 1),
    "bark_leaf_posterior_predict_workspace_bytes": (141, 13, 5, 3, 256, 17, 0, 0, 0),
    "bark_leaf_posterior_paths_workspace_bytes": (2049, 13, 5, 1, 0),
    "bark_path_scan_workspace_bytes": (141, 13, 4097, 256, 0),
}


def ask(lib, name):
    q = getattr(lib, name)
    return [int(q(*args)) for args in itertools.product(*GRID[name])]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_of_this_grid(golden):
    assert golden["grid"] == GRID and sorted(golden["bytes"]) == sorted(GRID) == sorted(REFUSED)


@pytest.mark.parametrize("name", sorted(GRID))
def test_query_answers_as_recorded(golden, name):
    lib = _lib.lib()
    got, want = ask(lib, name), golden["bytes"][name]
    assert len(got) == len(want)
    wrong = [(args, g, w) for args, g, w in zip(itertools.product(*GRID[name]), got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])
    assert any(want) and all(w % 256 == 0 for w in want)
    assert getattr(lib, name)(*REFUSED[name]) == 0


if __name__ == "__main__":
    table = {"grid": GRID, "bytes": {name: ask(_lib.lib(), name) for name in sorted(GRID)}}
    with open(GOLDEN, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(GOLDEN, sum(len(v) for v in table["bytes"].values()), "values")
