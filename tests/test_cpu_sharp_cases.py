"""What keeps tests/test_gpu_sharp.py from being vacuous or from hiding a failure, checked on the reference alone (no GPU).

* caps: the fp32 oracle's own distance to the fp64 oracle on every sharp case -- the bar of the GPU tests is 4 x that + the floor, so
  a cap on it bounds what a device defect can hide behind;
* coverage: the oracle's splines really see every bin, both tails, narrow bins, steep and flat bins, extreme knot derivatives; the
  affine maps see scales far from 1;
* the numpy twin of the device's spline backward agrees with autograd on the sharp rows;
* the fp32 oracle meets the draw-for-draw rule against the fp64 oracle on the sharp lampe flows;
* sensitivity: three one-line mistakes in a spline move log p far beyond the bar on the sharp inputs.

The tests print what they measure (run with -s)."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import sharp_cases as SC
from cases import make_case
from oracle import flows as OF
from oracle import posterior as OP
from spline_bwd_model import spline_fwd_bwd

SHARP = SC.SHARP
SPLINE = [n for n in SHARP if n.startswith("nsf")]
AFFINE = [n for n in SHARP if n.startswith("maf")]


@pytest.mark.parametrize("name", SHARP)
def test_reference_error_caps(name):
    """e_ref max <= 1e-3 in log p (any device defect >= 4e-3 + floor on a single row is caught), <= 1e-4 of max(sigma, |theta - mean|)
    for the inverse, <= 1e-4 of max |g| on every tensor of the gradient."""
    c = SC.sharp_case(name)
    lp = SC.case_budget(name, "logp")
    e_lp = np.abs(lp["f32"] - lp["f64"]).max()
    inv = SC.case_budget(name, "inverse")
    e_th = (np.abs(inv["f32"][0] - inv["f64"][0]) / SC.theta_scale(c.ospec, inv["f64"][0])).max()
    g = SC.case_budget(name, "grad", 512)
    g64, g32 = g["f64"][1], g["f32"][1]
    e_g = max(np.abs(g32[o:o + int(np.prod(s))] - g64[o:o + int(np.prod(s))]).max() for _, s, o in OF.param_layout(c.ospec)) / np.abs(g64).max()
    print(f"{name} (gain {c.gain}, {len(c.theta)} rows): e_ref max log p {e_lp:.2e}, theta {e_th:.2e}, gradient {e_g:.2e}; "
          f"log p in [{lp['f64'].min():.0f}, {lp['f64'].max():.0f}]")
    assert c.gain < 10
    assert np.isfinite(lp["f64"]).all() and np.isfinite(lp["f32"]).all() and np.isfinite(inv["f32"][0]).all()
    assert e_lp <= 1e-3 and e_th <= 1e-4 and e_g <= 1e-4, (e_lp, e_th, e_g)


def _trace(c):
    fl = torch.as_tensor(np.array(c.flat)).double()
    th, x, z = (torch.as_tensor(np.array(a)).double() for a in (c.theta, c.x, c.z))
    with SC.spline_trace() as tr, torch.no_grad():
        OF.log_prob(c.ospec, fl, th, x)
        OF.inverse_transform(c.ospec, fl, z, x)
    return tr


@pytest.mark.parametrize("name", SPLINE)
def test_spline_coverage(name):
    c = SC.sharp_case(name)
    o = c.ospec
    tr = _trace(c)
    met = dict(narrow=False, slopes=False, der=False)
    for inverse in (False, True):
        for t in range(o.T):
            (cl,) = tr.of(t, inverse)
            inside = ~(cl["low"] | cl["high"])
            cnt = np.bincount(cl["idx"][inside].ravel(), minlength=o.K)
            lo, hi = cl["low"].mean(), cl["high"].mean()
            print(f"{name} t{t} {'inverse' if inverse else 'forward'}: rarest bin {cnt.min()} rows, tails {lo:.3f} / {hi:.3f}, w/2B "
                  f"{cl['w'][0]:.4f}..{cl['w'][1]:.2f}, h/w {cl['slope'][0]:.3f}..{cl['slope'][1]:.1f}, knot derivative "
                  f"{cl['der'][0]:.5f}..{cl['der'][1]:.1f}")
            assert cnt.min() >= 1, (t, inverse, cnt)                 # every bin index is hit
            assert lo >= 0.02 and hi >= 0.02, (t, inverse, lo, hi)   # each tail holds >= 2 % of the rows
            met["narrow"] |= cl["w"][0] < 0.03
            met["slopes"] |= cl["slope"][1] > 5 and cl["slope"][0] < 0.2
            if o.kind == "nsf" and o.D > 1:      # coupling NSF: the derivative floor itself
                met["der"] |= cl["der"][0] <= 1.01 * o.min_derivative
            elif name == "nsfar_cfg1":
                # zuko's soft clip exp(d / (1 + |d| / 6.9)) needs a raw logit of -5.3 for 0.05 and of +2.1 for 5.  Of ~150 scanned
                # (gain, seed) pairs of this case none reached 0.05 while the fp32 oracle stayed inside test_reference_error_caps
                # (from gain 2.25 up its inverse or gradient error passes 1e-4 on most seeds); the caps win and the gain is 2.  Held
                # here: raw logits beyond 2.1 on BOTH sides (0.2 / 5); reached: 0.16 / 9.4.  nsfar_small, nsfar_d1 and nsfar_33
                # meet 0.05 through the same device spline.
                met["der"] |= cl["der"][0] < 0.2 and cl["der"][1] > 5
            else:                                # zuko, and the context-only spline of a one-parameter NSF
                met["der"] |= cl["der"][0] < 0.05 and cl["der"][1] > 5
    assert all(met.values()), met


@pytest.mark.parametrize("name", AFFINE)
def test_affine_scale_coverage(name):
    c = SC.sharp_case(name)
    s = np.concatenate([a[2].ravel() for a in _trace(c).scales])
    print(f"{name}: scales {s.min():.4f} .. {s.max():.2f}")
    # sigmoid(a + 2) + eps never exceeds 1.001: its far end is saturation
    assert s.min() < 0.2 and s.max() > (0.99 if c.ospec.scale_fn == "sigmoid2" else 5.0), (s.min(), s.max())


def test_edge_rows():
    for name in ("nsf_d1", "nsfar_d1"):
        c = SC.sharp_case(name)
        b = np.float32(c.ospec.tail_bound)
        K1 = c.ospec.K + 1
        assert c.n_edge == 7 + 6 * K1 and len(c.theta) == len(c.z) == len(c.x)
        e = c.theta[-c.n_edge:, 0]
        assert set(e[:7]) == {b, -b, np.nextafter(b, np.float32(9)), np.nextafter(-b, np.float32(-9)), np.nextafter(b, np.float32(0)),
                              np.nextafter(-b, np.float32(0)), np.float32(0)}
        assert np.all(np.diff(e[7:7 + K1]) > 0) and e[7] == -b and e[7 + K1 - 1] == b       # a row's knots
        tr = _trace(c)
        (fwd,), (inv,) = tr.of(0, False), tr.of(c.ospec.T - 1, True)
        # u = theta exactly: the first spline of each direction meets the values as given
        assert np.array_equal(fwd["v"][-c.n_edge:, 0], e) and np.array_equal(inv["v"][-c.n_edge:, 0], c.z[-c.n_edge:, 0])
        lp = SC.case_budget(name, "logp")
        assert np.isfinite(lp["f64"][-c.n_edge:]).all() and np.isfinite(lp["f32"][-c.n_edge:]).all()


def test_numpy_twin_of_the_spline_backward_on_sharp_rows():
    """tests/spline_bwd_model.py (the device's hand-derived backward) against autograd, tolerances of test_cpu_spline_backward.py,
    on rows of the sharp nsf_cfg3: every bin of every transform, both tails, the narrowest bin's rows."""
    c = SC.sharp_case("nsf_cfg3")
    o = c.ospec
    tr = _trace(c)
    rng = np.random.default_rng(0)
    n = 0
    for t in range(o.T):
        (cl,) = tr.of(t, False)
        picks = []
        inside = ~(cl["low"] | cl["high"])
        for k in range(o.K):
            r, d = np.nonzero(inside & (cl["idx"] == k))
            picks += list(zip(r[:2], d[:2]))
        for m in (cl["low"], cl["high"]):
            r, d = np.nonzero(m)
            picks += list(zip(r[:1], d[:1]))
        for r, d in picks:
            q, v = cl["q"][r, d], float(cl["v"][r, d])
            Go, Gl = rng.normal(), rng.normal()
            qt = torch.tensor(q[None, None, :], requires_grad=True)
            vt = torch.tensor([[v]], dtype=torch.float64, requires_grad=True)
            out, lad = OF.rq_spline(o, vt, qt, inverse=False)
            (Go * out + Gl * lad).sum().backward()
            ov, lv, dv, dq = spline_fwd_bwd(q, v, Go, Gl, o.K, o.H)
            assert abs(ov - out.item()) < 1e-10 and abs(lv - lad.item()) < 1e-9
            assert abs(dv - vt.grad.item()) < 1e-8 * max(1, abs(vt.grad.item())), (t, r, d, dv, vt.grad.item())
            ref = qt.grad[0, 0].numpy()
            assert np.abs(dq - ref).max() < 1e-8 * max(1.0, np.abs(ref).max()), (t, r, d)
            n += 1
    assert n >= o.T * (o.K + 2)


@pytest.mark.parametrize("name", ["nsfar_small", "nsfar_cfg1"])
def test_fp32_oracle_meets_the_draw_for_draw_rule(name):
    """The rule of tests/test_gpu_parity.py::_draw_for_draw, fp32 oracle against fp64 oracle, on the inputs the device test uses: if
    the reference's own fp32 evaluation could not meet it, no fp32 kernel could be asked to."""
    c = SC.sharp_case(name, B=6, gain=SC.DRAW_GAINS[name], spread=0.2)
    o, flat, x = c.ospec, torch.as_tensor(np.array(c.flat)), np.array(c.x)
    S, seed = 257, 2025
    free, _ = OP.sample(o, flat, x, 400, 99, dtype=torch.float32)
    lo = np.quantile(free.reshape(-1, o.D), 0.03, axis=0).astype(np.float32)
    hi = np.quantile(free.reshape(-1, o.D), 0.97, axis=0).astype(np.float32)
    got, nd = OP.sample(o, flat, x, S, seed, lo, hi, dtype=torch.float32)
    ref, rnd = OP.sample(o, flat, x, S, seed, lo, hi, dtype=torch.float64)
    err = np.abs((got - ref) / (hi - lo).astype(np.float64)).max(-1)
    bad_g, off_g = (err > 1e-4).sum(1), np.abs(nd - rnd)
    print(f"{name}: max err / box {err.max():.2e}, mismatching draws {bad_g.sum()}, attempt counts off by {off_g.sum()} of {rnd.sum()}")
    assert np.isfinite(got).all()
    assert (bad_g <= off_g).all(), (bad_g, off_g, err.max())
    assert off_g.sum() <= max(3, 0.01 * rnd.sum())
    assert (nd >= S).all() and nd.sum() > S * len(x)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
def _rq_forward(spec, v, q, swap=False):
    """The density direction of OF.rq_spline, restated so that one line can be got wrong: ``swap`` exchanges d_k and d_{k+1}."""
    K, B = spec.K, spec.tail_bound
    const = math.log(math.exp(1.0 - spec.min_derivative) - 1.0)
    ud = q[..., 2 * K:]
    ud = torch.cat([torch.full_like(ud[..., :1], const), ud, torch.full_like(ud[..., :1], const)], dim=-1)
    cw, w = OF._knots(spec, q[..., :K] / math.sqrt(spec.H), spec.min_bin_width)
    ch, hh = OF._knots(spec, q[..., K:2 * K] / math.sqrt(spec.H), spec.min_bin_height)
    der = spec.min_derivative + torch.nn.functional.softplus(ud)
    inside = (v >= -B) & (v <= B)
    vc = torch.clamp(v, -B, B)
    idx = ((vc[..., None] >= cw[..., :-1]).sum(-1) - 1).clamp(0, K - 1)[..., None]
    g = lambda a: a.gather(-1, idx)[..., 0]
    x_k, w_k, y_k, h_k, s_k, d_k, d_k1 = g(cw), g(w), g(ch), g(hh), g(hh / w), g(der), g(der[..., 1:])
    if swap:
        d_k, d_k1 = d_k1, d_k
    xi = (vc - x_k) / w_k
    om = xi * (1 - xi)
    den = s_k + (d_k + d_k1 - 2 * s_k) * om
    out = y_k + h_k * (s_k * xi * xi + d_k * om) / den
    lad = torch.log(s_k * s_k * (d_k1 * xi * xi + 2 * s_k * om + d_k * (1 - xi) * (1 - xi))) - 2 * torch.log(den)
    return torch.where(inside, out, v), torch.where(inside, lad, torch.zeros_like(lad))


def _log_prob_with(ospec, flat, theta, x, spline):
    saved = OF.rq_spline
    OF.rq_spline = spline
    try:
        with torch.no_grad():
            return OF.log_prob(ospec, torch.as_tensor(np.array(flat)).double(), torch.as_tensor(np.array(theta)).double(),
                               torch.as_tensor(np.array(x)).double()).numpy()
    finally:
        OF.rq_spline = saved


def test_one_line_mistakes_are_seen_on_the_sharp_inputs():
    """Three mistakes a kernel could make -- no minimum bin width / height, d_k and d_{k+1} exchanged, no minimum derivative -- move
    log p of the sharp nsf_cfg3 far beyond the bar (4 e_ref + floor); printed next to what they do to make_case's inputs."""
    rq = OF.rq_spline
    wrong = {
        "restated spline, nothing wrong": lambda s, v, q, inverse: _rq_forward(s, v, q),
        "no minimum bin width / height": lambda s, v, q, inverse: rq(dataclasses.replace(s, min_bin_width=0.0, min_bin_height=0.0), v, q, inverse),
        "d_k and d_k+1 exchanged": lambda s, v, q, inverse: _rq_forward(s, v, q, swap=True),
        "no minimum derivative": lambda s, v, q, inverse: rq(dataclasses.replace(s, min_derivative=0.0), v, q, inverse),
    }
    c = SC.sharp_case("nsf_cfg3")
    b = SC.case_budget("nsf_cfg3", "logp")
    e_ref = np.abs(b["f32"] - b["f64"])
    o2, _, flat2, theta2, x2 = make_case("nsf_cfg3", B=512)
    base2 = _log_prob_with(o2, flat2, theta2, x2, rq)
    for what, fn in wrong.items():
        d_sharp = np.abs(_log_prob_with(c.ospec, c.flat, c.theta, c.x, fn) - b["f64"])
        d_old = np.abs(_log_prob_with(o2, flat2, theta2, x2, fn) - base2)
        print(f"{what}: |d log p| sharp median {np.median(d_sharp):.2e} p99 {np.quantile(d_sharp, 0.99):.2e} max {d_sharp.max():.2e} | "
              f"make_case median {np.median(d_old):.2e} p99 {np.quantile(d_old, 0.99):.2e} max {d_old.max():.2e}")
        if what.endswith("nothing wrong"):
            assert d_sharp.max() < 1e-9 and d_old.max() < 1e-9
            continue
        # seen: beyond the bar at the maximum by a factor of ten and more
        assert d_sharp.max() > 10 * (SC.FACTOR * e_ref.max() + SC.LOGP_FLOOR), (what, d_sharp.max(), e_ref.max())


def test_plain_log_of_one_plus_exp_shows_only_on_the_sharp_maf():
    """softplus as log(1 + e^a) in fp32 -- what sf_softplus was before these tests -- against log1p(e^a): the MAF inverse of the fp32
    oracle moves away from the fp64 oracle by an order of magnitude on the sharp maf_cfg1 (scales down to 2e-3, where 1 + e^a keeps
    five digits of e^a) and not at all on make_case's inputs (scales near 1).  Printed; the assertion is the order of magnitude."""
    plain = lambda spec, a: torch.log(1 + torch.exp(a)) + spec.maf_eps
    c = SC.sharp_case("maf_cfg1")
    o2, _, flat2, theta2, x2 = make_case("maf_cfg1", B=512)
    z2 = np.random.default_rng(5).normal(size=theta2.shape).astype(np.float32)
    worse = {}
    for label, (o, flat, theta, x, z) in (("sharp", (c.ospec, c.flat, c.theta, c.x, c.z)), ("make_case", (o2, flat2, theta2, x2, z2))):
        ref = SC.budget(o, flat, theta, x, z, "inverse")
        saved = OF._scale_from_unconstrained
        OF._scale_from_unconstrained = plain
        try:
            got = SC.budget(o, flat, theta, x, z, "inverse")["f32"]
        finally:
            OF._scale_from_unconstrained = saved
        sc = SC.theta_scale(o, ref["f64"][0])
        e_plain, e_ref = np.abs(got[0] - ref["f64"][0]) / sc, np.abs(ref["f32"][0] - ref["f64"][0]) / sc
        l_plain, l_ref = np.abs(got[1] - ref["f64"][1]), np.abs(ref["f32"][1] - ref["f64"][1])
        print(f"{label}: theta error max {e_plain.max():.2e} (log1p form {e_ref.max():.2e}), p99 ratio "
              f"{np.quantile(e_plain, 0.99) / np.quantile(e_ref, 0.99):.1f}; logdet error max {l_plain.max():.2e} ({l_ref.max():.2e})")
        worse[label] = np.quantile(e_plain, 0.99) / np.quantile(e_ref, 0.99)
    assert worse["sharp"] > 8 and worse["make_case"] < 2, worse
