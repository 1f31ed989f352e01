"""Conditions on the inputs of tests/test_gpu_vjp.py, held on the reference alone (no device):

1. for every case x pattern with a nonzero gradient the float32 oracle stays within the floor on every tensor, max |g32 - g64| <=
   GRAD_FLOOR x max |g64|: the bar of sharp_cases.check_bar can then never exceed five floors (1e-3 of the largest gradient);
2. the weight patterns have the features they are named for;
3. the bar tells right from wrong: under the signed pattern (and onehot_last) the fp64 gradient under four wrong readings of the
   weights (all ones; rolled by one position; the ragged tile's weights taken from the first tile; in the rows form the weight at
   rows[b] % B) differs from the reference on at least one tensor by 20 x the bar's maximum, 0.02 x max |g64|;
4. onehot_last is the per-sample fp64 gradient of the last row.
"""
import numpy as np
import pytest

import sharp_cases as SC
import vjp_cases as VC

_SHAPES = sorted({(c.name, c.B) for c in VC.SMALL})
_FORMS = [False, True]
_ids = lambda v: "rows" if v is True else "direct" if v is False else str(v)


def _forms(pattern):
    return _FORMS if pattern in VC.BOTH_FORMS else [False]


def _check_floor(label, ospec, r):
    gmax = np.abs(r.g64).max()
    assert gmax > 0, label
    worst = max(VC.tensor_max(ospec, r.g32 - r.g64).items(), key=lambda kv: kv[1])
    print(f"VJPCASE {label}: max |g64| {gmax:.3e} worst tensor {worst[0]} |g32 - g64| {worst[1]:.3e} = {worst[1] / gmax:.2e} of it")
    assert worst[1] <= SC.GRAD_FLOOR * gmax, (label, worst, gmax)


def _check_wrong(label, ospec, name, B, rows_form, w, scale, g64, readings, asserted=True):
    gmax = np.abs(g64).max()
    for kind, ww in readings.items():
        gw, _ = VC.grads_for(name, B, rows_form, ww, scale)
        far = max(VC.tensor_max(ospec, gw - g64).values())
        print(f"VJPCASE {label} wrong reading {kind}: max tensor difference {far / gmax:.3f} of max |g64|")
        if asserted:
            assert not np.array_equal(ww, w), (label, kind)
            assert far >= VC.WRONG_MIN * gmax, (label, kind, far, gmax)


@pytest.mark.parametrize("name,B", _SHAPES)
def test_fp32_oracle_stays_within_the_floor(name, B):
    """Condition 1 on the parameter gradient (and printed for the context gradient)."""
    for pattern in ("uniform", "signed", "onehot_last"):
        for rows_form in _forms(pattern):
            ospec = VC.inputs(name, B, rows_form).ospec
            for sk in VC.SCALES:
                r = VC.reference(name, B, rows_form, pattern, sk)
                _check_floor(f"{name}-{B} {pattern} {_ids(rows_form)} {sk}", ospec, r)
                assert np.isfinite(r.loss32).all() and np.abs(r.loss32 - r.loss64).max() < SC.LOGP_FLOOR


@pytest.mark.parametrize("B", sorted({c.B for c in VC.SMALL + VC.LARGE}))
def test_weight_patterns_have_their_features(B):
    """Condition 2 (the patterns depend on the case's name only through their seed: every name at this B is checked)."""
    for name in sorted({c.name for c in VC.SMALL + VC.LARGE if c.B == B}):
        tl = VC.tiles(B)
        assert len(tl) >= 3 and 0 < B % VC.TILE, "two full tiles and a ragged one"
        u = VC.weights(name, B, "uniform")
        assert u.dtype == np.float32 and (u >= 0.5).all() and (u <= 1.5).all() and u.std() > 0.2
        s = VC.weights(name, B, "signed")
        assert (s == 0).mean() >= 0.2
        zt = VC.zero_tile(B)
        assert 0 <= zt < len(tl) - 1 and (s[tl[zt]] == 0).all() and len(s[tl[zt]]) == VC.TILE
        for t, sl in enumerate(tl):
            if t != zt:
                assert VC._both_signs(s[sl]) and (len(s[sl]) == 1 or ((s[sl] > 0).any() and (s[sl] < 0).any())), (name, B, t)
        o = VC.weights(name, B, "onehot_last")
        assert o[B - 1] == 1 and o.sum() == 1 and (B - 1) // VC.TILE == len(tl) - 1
        assert not VC.weights(name, B, "zeros").any()
        for a in (u, s):
            assert not np.array_equal(a, VC.weights(name + "x", B, "uniform" if a is u else "signed"))


@pytest.mark.parametrize("name,B", _SHAPES)
def test_rows_of_the_rows_form(name, B):
    i = VC.inputs(name, B, True)
    assert i.theta.shape[0] == VC.N_TRAIN and i.rows.shape == (B,) and i.rows.dtype == np.int64
    assert len(np.unique(i.rows)) < B and (np.diff(i.rows) < 0).any() and (np.diff(i.rows) > 0).any()
    assert (i.rows % B != np.arange(B)).mean() > 0.9
    assert np.array_equal(i.theta_b, i.theta[i.rows]) and np.array_equal(i.x_b, i.x[i.rows])


@pytest.mark.parametrize("rows_form", _FORMS, ids=_ids)
@pytest.mark.parametrize("name,B", _SHAPES)
def test_wrong_readings_of_the_weights_are_far_from_the_reference(name, B, rows_form):
    """Condition 3, asserted on the patterns made to discriminate: signed, and onehot_last where it runs.  Under the control pattern
    a wrong reading cannot be far: the weights are within 0.5 of each other and of 1, so that every misreading moves the gradient by a
    few percent of its largest entry (and the single ragged row of B = 513 by 1 / 513 of it); its distances are printed."""
    i = VC.inputs(name, B, rows_form)
    for pattern in ("signed", "onehot_last", "uniform"):
        if rows_form and pattern not in VC.BOTH_FORMS:
            continue
        w = VC.weights(name, B, pattern)
        r = VC.reference(name, B, rows_form, pattern, "sum")
        readings = VC.wrong_readings(w, i.rows)
        assert set(readings) == {"ones", "rolled", "ragged_from_first"} | ({"by_gathered_row"} if rows_form else set())
        _check_wrong(f"{name}-{B} {pattern} {_ids(rows_form)}", i.ospec, name, B, rows_form, w, 1.0, r.g64, readings,
                     asserted=pattern != "uniform")


@pytest.mark.parametrize("name,B", _SHAPES)
def test_onehot_last_is_the_gradient_of_the_last_row(name, B):
    """Condition 4."""
    for sk in VC.SCALES:
        r = VC.reference(name, B, False, "onehot_last", sk)
        g = VC.per_sample_gradient(name, B, False, B - 1, VC.grad_scale(B, sk))
        assert np.abs(g).max() > 0
        assert np.abs(r.g64 - g).max() <= 1e-10 * np.abs(g).max(), (name, B, sk, np.abs(r.g64 - g).max(), np.abs(g).max())
        # the context gradient reaches that row alone
        assert not r.dx64[:B - 1].any() and r.dx64[B - 1].any()


@pytest.mark.parametrize("case", VC.LARGE, ids=VC.case_id)
def test_large_batches(case):
    """Conditions 1 and 3 (the rolled reading) at the batches that reach a second chunk of a persistent workgroup."""
    i = VC.inputs(case.name, case.B, False)
    w = VC.weights(case.name, case.B, "signed")
    for sk in VC.SCALES:
        r = VC.reference(case.name, case.B, False, "signed", sk)
        _check_floor(f"{VC.case_id(case)} signed {sk}", i.ospec, r)
    r = VC.reference(case.name, case.B, False, "signed", "sum")
    _check_wrong(f"{VC.case_id(case)} signed", i.ospec, case.name, case.B, False, w, 1.0, r.g64, {"rolled": np.roll(w, 1)})
