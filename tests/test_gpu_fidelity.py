"""The fidelity information gain on the device (LeafPosterior.information_gain and bark_amd.optimizer.fidelity;
bark_fidelity_gain_fitted_hip) against tests/fidelity_ref.py within the propagated posterior bar, and bit for bit wherever the
contract says so: the same point against the scan's "mes", chunks, repeats, weights against a subset.

The cases are fidelity_ref.GPU_CASES (those that pass its precheck; tests/test_fidelity_cpu.py holds the list).  Everything
beyond them runs on `wave_edge`: B = 3 forests of 5 trees, C = 65 pairs (one past a wave), S = 7 targets, both kinds of pairs."""
import ctypes

import numpy as np
import pytest

import fidelity_ref as fr

pytestmark = pytest.mark.gpu

BASE = "wave_edge"


class Fitted:
    def __init__(self, name):
        import torch

        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from bark_amd.tree_kernels import fit_posterior

        self.inp = fr.make_inputs(name)
        self.case = self.inp.case
        self.ref = fr.reference(name)
        self.post = fit_posterior(self.inp.model, self.inp.data, self.inp.ft, chunk=self.case.chunk)

    def gain(self, **kw):
        return self.post.information_gain(self.inp.query, self.inp.target, self.ref.targets, **kw)


_fitted = {}


def fitted(name) -> Fitted:
    if name not in _fitted:
        _fitted[name] = Fitted(name)
    return _fitted[name]


@pytest.fixture(scope="module")
def base():
    return fitted(BASE)


@pytest.mark.parametrize("name", fr.GPU_CASES)
def test_case_within_the_bar(name):
    f = fitted(name)
    gain, rows = f.gain(per_forest=True, chunk=f.case.chunk)
    assert gain.shape == (f.case.C,) and rows.shape == (f.case.B, f.case.C)
    used, used_rows = fr.bar_used(gain, f.ref.gain, f.ref.bar), fr.bar_used(rows, f.ref.pf, f.ref.pf_bar)
    print(f"{name}: bar used {used:.3g} (gain), {used_rows:.3g} (per forest); separated {int((~f.ref.same).sum())} of {f.ref.same.size}")
    assert used <= 1.0
    assert used_rows <= 1.0
    best, decided = fr.index_gap(f.ref)
    if decided:
        assert int(np.argmax(gain)) == best


def test_same_point_is_the_scan_mes(base):
    t = base.ref.targets
    for pts in (base.inp.target, base.inp.query):
        gain = base.post.information_gain(pts, pts, t)
        assert np.array_equal(gain, -base.post.scan(pts, kind="mes", targets=t, return_values=True)[2])


def test_chunk_changes_no_bit(base):
    want = base.gain(per_forest=True)
    for chunk in (1, 2):
        got = base.gain(per_forest=True, chunk=chunk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    f = fitted("chunks")  # five forests: three chunks of two, five of one, one of five
    want = f.gain(per_forest=True, chunk=5)
    for chunk in (1, 2):
        got = f.gain(per_forest=True, chunk=chunk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_two_runs_give_the_same_bits(base):
    one, two = base.gain(per_forest=True), base.gain(per_forest=True)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])


def test_weights_against_a_subset(base):
    w = np.array([1.0, 0.0, 1.0]) / 2
    gain, rows = base.gain(per_forest=True, weights=w)
    sub = base.post.subset([0, 2])
    want, want_rows = sub.information_gain(base.inp.query, base.inp.target, base.ref.targets[[0, 2]], per_forest=True)
    assert np.array_equal(gain, want)
    assert np.array_equal(rows[[0, 2]], want_rows) and np.isnan(rows[1]).all()
    # the state's own weights are honoured, and None switches them off
    post = base.post._copy()
    post.reweight_(np.array([0.0, -np.inf, 0.0]))
    by_state = post.information_gain(base.inp.query, base.inp.target, base.ref.targets, per_forest=True)[1]
    assert np.array_equal(by_state[[0, 2]], want_rows) and np.isnan(by_state[1]).all()  # the dead forest was skipped
    assert np.array_equal(post.information_gain(base.inp.query, base.inp.target, base.ref.targets, weights=None), base.gain())


def test_torch_inputs_give_device_tensors(base):
    import torch

    want = base.gain(per_forest=True)
    q, x0, t = (torch.from_numpy(np.ascontiguousarray(a)) for a in (base.inp.query, base.inp.target, base.ref.targets))
    gain, rows = base.post.information_gain(q, x0, t, per_forest=True)
    assert gain.is_cuda and rows.is_cuda and gain.dtype == torch.float64
    assert np.array_equal(gain.cpu().numpy(), want[0]) and np.array_equal(rows.cpu().numpy(), want[1])


def test_fidelity_information_gain_rows(base):
    from bark_amd.optimizer import fidelity_information_gain, with_fidelity

    x, t = base.inp.x, base.ref.targets
    gains = fidelity_information_gain(base.post, x, fidelity_feature=fr.FID, fidelities=[0, 1, 2], targets=t)
    assert gains.shape == (3, base.case.C)
    x0 = with_fidelity(x, fr.FID, 0)
    assert np.array_equal(x0, base.inp.target)
    assert np.array_equal(gains[0], base.post.information_gain(x0, x0, t))
    for k in (1, 2):
        assert np.array_equal(gains[k], base.post.information_gain(with_fidelity(x, fr.FID, k), x0, t))
    # the case's own pairs are rows 1 and 2, picked by the fidelity column of x
    picked = np.where(x[:, fr.FID] == 1, gains[1], gains[2])
    assert np.array_equal(picked, base.gain())


def host_argmax(gains, costs):
    """per column the first t with the largest gain / cost among those that are not NaN; -1 without one"""
    out = []
    for c in range(gains.shape[1]):
        best, arg = None, -1
        for k in range(gains.shape[0]):
            v = gains[k, c] / costs[k]
            if not np.isnan(v) and (best is None or v > best):
                best, arg = v, k
        out.append(arg)
    return np.array(out, dtype=np.int64)


def test_propose_fidelity(base):
    from bark_amd.optimizer import propose_fidelity_information_based

    x, t = base.inp.x, base.ref.targets
    kw = dict(fidelity_feature=fr.FID, fidelities=[0, 1, 2], targets=t)
    index, gains = propose_fidelity_information_based(base.post, x, [1.0, 1.0, 1.0], **kw)
    assert index.dtype == np.int64 and index.shape == (base.case.C,) and gains.shape == (3, base.case.C)
    assert np.array_equal(index, host_argmax(gains, [1.0, 1.0, 1.0]))
    # a candidate whose two best fidelities have positive gains; the runner-up's cost puts it at 3/4 of the winner's ratio
    order = np.argsort(-gains, axis=0)
    runner = gains[order[1], np.arange(base.case.C)]
    c = int(np.argmax(runner))
    w, r = int(order[0, c]), int(order[1, c])
    assert gains[r, c] > 0
    costs = np.ones(3)
    costs[r] = gains[r, c] / (0.75 * gains[w, c])
    first = propose_fidelity_information_based(base.post, x, costs, **kw)[0]
    assert first[c] == w
    costs[w] *= 2.0
    second, again = propose_fidelity_information_based(base.post, x, costs, **kw)
    assert second[c] == r and np.array_equal(again, gains)
    assert np.array_equal(second, host_argmax(gains, costs))
    # without targets the draws come from the sites
    index, gains = propose_fidelity_information_based(base.post, x[:5], [1.0, 2.0, 4.0], fidelity_feature=fr.FID, fidelities=[0, 1, 2],
                                                      sites=base.inp.X, num_samples=4, seed=3)
    assert np.array_equal(index, host_argmax(gains, [1.0, 2.0, 4.0])) and gains.shape == (3, 5)


def test_fstar_at_fidelity(base):
    from bark_amd.optimizer import fstar_at_fidelity, with_fidelity

    S = 6
    kw = dict(fidelity_feature=fr.FID, target=0, num_samples=S, seed=11)
    f = fstar_at_fidelity(base.post, base.inp.X, **kw)
    assert f.is_cuda and tuple(f.shape) == (base.case.B, S)
    assert np.array_equal(f.cpu().numpy(), fstar_at_fidelity(base.post, base.inp.X, **kw).cpu().numpy())
    assert not np.array_equal(f.cpu().numpy(), fstar_at_fidelity(base.post, base.inp.X, **{**kw, "seed": 12}).cpu().numpy())
    values = base.post.sample_paths(S, seed=11).evaluate(with_fidelity(base.inp.X, fr.FID, 0))  # (B S, N)
    assert (f.cpu().numpy().reshape(-1, 1) <= values).all()
    assert np.array_equal(f.cpu().numpy().reshape(-1), values.min(axis=1))


def test_invalid_category(base):
    import torch

    from bark_amd import _lib
    from bark_amd.fitting.mll import _clear_fault

    bad = base.inp.query.copy()
    bad[:, fr.FID] = -1.0
    with pytest.raises(ValueError, match="categorical"):
        base.post.information_gain(bad, base.inp.target, base.ref.targets)
    post, lib = base.post, _lib.lib()
    C, S = base.case.C, base.case.S
    q, x0, t = (_lib.to_device(a, torch.float64) for a in (bad, base.inp.target, base.ref.targets))
    gain = torch.empty(C, dtype=torch.float64, device=q.device)
    info = torch.zeros(post.B, dtype=torch.int32, device=q.device)
    ws = _lib.workspace(int(lib.bark_fidelity_gain_fitted_workspace_bytes(post.R, post.m, post.B, C, S)))
    lo, hi, n_a, pad, G = fr.GRID
    rc = lib.bark_fidelity_gain_fitted_hip(_lib.ctx(), _lib.ptr(post.packed.packed), post.packed.info_ref, post.d, _lib.ptr(post.noise),
                                           _lib.ptr(post.scale), _lib.ptr(post.state), post.nbytes, _lib.ptr(q), _lib.ptr(x0), C,
                                           _lib.ptr(t), S, None, lo, hi, n_a, pad, G, _lib.ptr(gain), None, _lib.ptr(info), _lib.ptr(ws),
                                           ws.numel(), post.B, _lib.stream_ptr())
    assert rc == 0
    assert (info.cpu().numpy() == -1).all() and np.isnan(gain.cpu().numpy()).all()
    _clear_fault()
    assert not post.info.cpu().numpy().any()  # the state is only read
    assert np.array_equal(base.gain(), base.post.information_gain(base.inp.query, base.inp.target, base.ref.targets))


def test_after_observe(base):
    inp, ref = base.inp, base.ref
    x_new = inp.target[:1].copy()
    y_new = np.array([float(inp.y.min()) - 0.5])
    post = base.post.observe(x_new, y_new)
    gain = post.information_gain(inp.query, inp.target, ref.targets)
    before = base.gain()
    assert not np.array_equal(gain, before)
    refit = fr.reference_of(inp.model, (np.concatenate([inp.X, x_new]), np.concatenate([inp.y.reshape(-1), y_new]).reshape(-1, 1)),
                            inp.query, inp.target, inp.ft, targets=ref.targets)
    assert np.isfinite(refit.gain).all() and np.isfinite(refit.bar).all() and (refit.bar > 0).all()
    assert np.abs(refit.gain - ref.gain).max() > 10 * refit.bar.max()  # the observation moved the reference too
    used = fr.bar_used(gain, refit.gain, refit.bar)
    print(f"after observe_: bar used {used:.3g}")
    assert used <= 1.0
    assert np.array_equal(base.gain(), before)  # `observe` worked on a copy
