"""The host reference of the front end (tests/frontend_ref.py) pinned without a device: the Gram rebuilt from the reference CODES is
the oracle's Gram bit for bit on every row and on goldens g3, g5 and g10; the shift / scale / noise values make the order of the
steps and their separate roundings visible; every row reaches the variant it is named for and every variant has a row; and the
wire-format reader agrees with a plain depth-first numbering on a scrambled container.  No GPU."""
import numpy as np
import pytest

import frontend_ref as fr
from conftest import load_golden
from oracle import oracle as orc


class _Inputs(dict):
    def __missing__(self, name):
        self[name] = fr.make_inputs(name)
        return self[name]


INPUTS = _Inputs()


def gram_from_reference_codes(F, X1, X2, ft):
    info, packed = fr.pack(F, ft)
    tables = fr.leaf_tables(packed, F.shape[2])
    c1, c2 = fr.reference_codes(F, X1, ft, info, tables), fr.reference_codes(F, X2, ft, info, tables)
    assert not c1[:, :, X1.shape[0]:].any() and not c2[:, :, X2.shape[0]:].any()  # the padding of every plane is zero
    bits = fr._lib.lib().bark_leaf_encoding(info) == 1
    m = F.shape[1]
    return np.stack([fr.gram_from_counts(fr.agree_from_codes(c1[b], c2[b], X1.shape[0], X2.shape[0], m, bits), m) for b in range(F.shape[0])])


@pytest.mark.parametrize("name", list(fr.CASES))
def test_gram_from_reference_codes_is_the_oracle(name):
    inp = INPUTS[name]
    F = inp.distinct
    got = gram_from_reference_codes(F, inp.X1, inp.X2, inp.ft)
    want = orc.batched_forest_gram_matrix(F, inp.X1, inp.X2, inp.ft)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    for b in range(F.shape[0]):  # and the index route of the Gram reference
        i1, i2 = orc.pass_through_forest(F[b], inp.X1, inp.ft), orc.pass_through_forest(F[b], inp.X2, inp.ft)
        assert np.array_equal(fr.gram_from_counts(fr.agree_from_indices(i1, i2), F.shape[1]).view(np.uint64), want[b].view(np.uint64))


@pytest.mark.parametrize("gname", ["g3_prior_mixed_n257", "g5_boundaries", "g10_mcmc_posterior_forests"])
def test_gram_from_reference_codes_on_the_goldens(gname):
    g = load_golden(gname)
    F = orc.nodes_from_raw(g["forest"])
    F = F.reshape(-1, *F.shape[-2:])
    X, ft = g["X"], g["feat_types"]
    got = gram_from_reference_codes(F, X, X, ft)
    assert np.array_equal(got.view(np.uint64), g["K"].reshape(got.shape).view(np.uint64)), gname


@pytest.mark.parametrize("name", list(fr.CASES))
def test_row_reaches_its_variant(name):
    print(name, sorted(fr.check_shape(name, INPUTS[name])))


def test_every_variant_has_a_row():
    walk, gram = set(), set()
    for name, case in fr.CASES.items():
        reached = fr.check_shape(name, INPUTS[name])
        if isinstance(case, fr.WalkCase):
            walk |= {case.variant}
        else:
            gram |= reached
    assert walk == fr.WALK_VARIANTS, sorted(fr.WALK_VARIANTS - walk)
    assert gram == fr.GRAM_VARIANTS, sorted(fr.GRAM_VARIANTS - gram)
    assert len(fr.WALK_VARIANTS) == 2 * 2 + 2 * 3 and len(fr.GRAM_VARIANTS) == 3 * 2 * 2
    cases = [c for c in fr.CASES.values() if isinstance(c, fr.WalkCase) and c.indices]
    assert {c.m for c in cases} >= {1, 31, 32, 33, 64, 65} and {c.N for c in cases} >= {1, 255, 256, 257} and {c.d for c in cases} == {15, 16}
    grams = [c for c in fr.CASES.values() if isinstance(c, fr.GramCase)]
    assert {c.N for c in grams} >= {1, 31, 32, 33, 63, 64, 65} and {c.M for c in grams} >= {1, 2, 63, 64, 65, 127, 128, 129}
    assert {c.m % 4 for c in grams if c.variant.startswith("bytes")} == {0, 1, 2, 3}
    assert {c.m for c in grams if c.params} == {3, 7, 13}
    # each walk variant has a row with a categorical feature (the fault test runs on those)
    assert {c.variant for c in fr.CASES.values() if isinstance(c, fr.WalkCase) and c.mixed and c.d >= 4} == fr.WALK_VARIANTS


@pytest.mark.parametrize("name", [n for n in fr.GRAM_CASES if fr.CASES[n].params])
def test_order_and_separate_roundings_are_visible(name):
    """For every combination of shift / scale / noise and every forest of the row: at least one entry of the documented result
    differs from the result with shift and scale in the other order, from `inv_m * count - shift` rounded once (a fused
    multiply-add), and from `scale * val + jitter` rounded once — else the row would pass a kernel that does any of these."""
    inp = INPUTS[name]
    case = inp.case
    for combo in fr.PARAM_COMBOS:
        par, counts = fr.gram_params(inp, combo)
        for b in range(case.B):
            count = counts[b]
            p = {k: (None if v is None else float(v[b])) for k, v in par.items()}
            ref = fr.gram_from_counts(count, case.m, **p)
            for kind, rows in fr.gram_variants_exact(count, case.m, p["shift"], p["scale"], p["noise"]).items():
                for c, on_diag, doc, _wrong in rows:  # the exact-arithmetic restatement is the numpy reference
                    k = np.arange(min(count.shape))
                    mask = np.zeros(count.shape, bool)
                    mask[k, k] = True
                    sel = (count == c) & (mask if (on_diag and p["noise"] is not None) else ~mask if p["noise"] is not None else True)
                    assert sel.any() and (ref[sel] == doc).all(), (name, combo, b, kind, c)
                if rows:
                    assert any(doc != wrong for _, _, doc, wrong in rows), (name, combo, b, kind)
                else:
                    assert (kind == "swapped" and not {"shift", "scale"} <= set(combo)) or (kind == "fma_shift" and "shift" not in combo) \
                        or (kind == "fma_jitter" and (not {"scale", "noise"} <= set(combo) or (case.same and "shift" not in combo))), (name, combo, kind)


@pytest.mark.parametrize("name", [n for n in fr.WALK_CASES if fr.CASES[n].mixed and fr.CASES[n].d >= 4 and fr.CASES[n].m >= 8])
def test_invalid_category_at_the_last_point_raises_in_the_oracle(name):
    """what tests/test_gpu_frontend.py::test_categorical_fault_in_the_last_block plants is a fault in the reference"""
    inp = INPUTS[name]
    for bad in (np.nan, -1.0, np.inf):
        X = inp.X1[-1:].copy()
        X[0, inp.ft == fr.CAT] = bad
        with pytest.raises(ValueError):
            for F in inp.distinct:
                orc.pass_through_forest(F, X, inp.ft)
    for F in inp.distinct:
        orc.pass_through_forest(F, inp.X1, inp.ft)  # the clean input walks


def _dfs_tables(F):
    """dense id and bit position of every reachable leaf by a plain recursive depth-first numbering, left child first"""
    B, m, L = F.shape
    ids, bits = np.full((B, m, L), -1, dtype=np.int64), np.full((B, m, L), -1, dtype=np.int64)
    for b in range(B):
        base = 0
        for t in range(m):
            count = [0]

            def visit(k):
                node = F[b, t, k]
                if node["is_leaf"]:
                    ids[b, t, k], bits[b, t, k] = count[0], base + count[0]
                    count[0] += 1
                else:
                    visit(int(node["left"]))
                    visit(int(node["right"]))

            visit(0)
            base += count[0]
    return ids, bits


def test_wire_format_reader_on_a_scrambled_container():
    from test_gpu_parity import _scrambled_forest

    rng = np.random.default_rng(5)
    ft = np.array([2, 2, 1, 0, 2, 0, 1, 2])
    F = np.stack([_scrambled_forest(rng, 9, 60, ft, max_leaves=14) for _ in range(3)])
    info, packed = fr.pack(F, ft)
    ids, bits = fr.leaf_tables(packed, 60)
    want_ids, want_bits = _dfs_tables(F)
    assert np.array_equal(ids, want_ids) and np.array_equal(bits, want_bits)
    assert info.max_bits == int(bits.max()) + 1 and info.max_leaves == int(ids.max()) + 1
    for name in ("walk_grouped_lds_bits_mixed", "gram_bytes8_comb129"):
        inp = INPUTS[name]
        i2, b2 = _dfs_tables(inp.distinct)
        assert np.array_equal(inp.tables[0], i2) and np.array_equal(inp.tables[1], b2)
