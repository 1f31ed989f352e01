"""Sharp flows for the conformance tests: head weights scaled up until the splines have bins of half a percent of the interval,
bin slopes and knot derivatives between the floor and ~15, and a good share of rows in the linear tails; affine scales far from 1.

Helper module, no tests in it.  ``sharp_case`` builds the inputs, ``spline_trace`` reports what the oracle's splines saw,
``budget`` / ``case_budget`` evaluate the oracle in fp64 and in fp32 on the same inputs and ``check_bar`` holds the one rule every
comparison uses:

    quantile_q(|kernel - oracle64|) <= 4 * quantile_q(|oracle32 - oracle64|) + floor      for q in 0.5, 0.99, 1.0

The right-hand side is measured on the reference at run time, never on the kernel.  Factor 4: kernel and fp32 oracle are two fp32
evaluations of the same conditioning in a different operation order; the suite already allows 3x between two of its own fp32 paths
(test_sampler_arithmetic_from_given_noise), the fourth is for comparing extreme quantiles of ~512 rows.  The floor is the suite's
bar for the quantity in the near-identity regime (1e-4 on log p, 1e-4 of max(sigma, |theta - mean|) on theta, 2e-4 of max |g| on
gradients): where the reference's own fp32 error is below it, the old bar still holds.
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from cases import CASES, make_case
from oracle import flows as OF

FACTOR = 4.0
QUANTILES = (0.5, 0.99, 1.0)
LOGP_FLOOR = 1e-4        # tests/test_gpu_parity.py LOGP_TOL
THETA_FLOOR = 1e-4       # test_sampler_arithmetic_from_given_noise: 1e-4 of the parameter scale on every row
GRAD_FLOOR = 2e-4        # tests/test_gpu_train.py: 2e-4 of max |g|
ROUNDTRIP_FLOOR = 5e-4   # test_inverse_from_noise_matches_oracle: log p(inverse(z)) against log N(z) - logdet

# Head gain per case.  Chosen on the CPU (tests/test_cpu_sharp_cases.py holds the conditions): large enough for the coverage
# conditions, small enough that the fp32 oracle itself stays within 1e-3 of the fp64 oracle in log p.  At gain 10 and above the fp32
# oracle is off by more than 1e-2 and a MAF inverse overflows: not a regime fp32 code can be held to.
_KIND_GAIN = {"nsf": 3.0, "nsf_ar": 3.0, "maf": 2.0, "maf_ar": 1.5}
# name -> (gain, seed of make_case and sharpen, random rows).  Where the kind's starting gain and seed 0 met every condition they are
# kept; elsewhere a scanned (gain, seed) at which the reference met all of them with room to spare: the fp32 oracle's maximum error
# over the rows moves by tens of percent with the host's summation order, so the caps are met with about a factor of two in hand.
# nsfar_cfg1 is the one case LOWERED: from gain 2.25 up its fp32 inverse or gradient error passes 1e-4 on most seeds.  The one-parameter flows need
# more rows: their spline parameters depend on the context alone, so the rarest bin of a later transform is reached a few times in
# thousands of rows.
TUNED = {
    "nsf_d2": (3.0, 1, 512),
    "nsf_nb1": (4.0, 0, 512),
    "nsf_d1": (5.0, 0, 2048),
    "nsfar_small": (4.0, 1, 512),
    "nsfar_33": (5.0, 1, 512),
    "nsfar_d1": (3.75, 1, 2048),
    "nsfar_cfg1": (2.0, 0, 512),
    "maf_cfg1": (4.0, 0, 512),
    "maf_sig2": (4.0, 1, 512),
    "maf_span6": (4.5, 0, 512),
    "maf_nb3": (5.0, 3, 512),
    "mafar_small": (4.0, 1, 512),
}
# the draw-for-draw runs (six context rows, weights spread 0.2 as in tests/test_gpu_parity.py)
DRAW_GAINS = {"nsfar_small": 3.0, "nsfar_cfg1": 2.0}

# one representative per kernel / template path (tests/test_gpu_sharp.py)
SHARP = ["nsf_cfg3", "nsf_k16", "nsf_odd", "nsf_d2", "nsf_nb1", "nsf_d1",
         "nsfar_small", "nsfar_cfg1", "nsfar_d1", "nsfar_33",
         "maf_cfg1", "maf_sig2", "maf_span6", "maf_nb3", "mafar_small"]

SharpCase = namedtuple("SharpCase", "ospec spec flat theta x z n_edge gain")


def tuned(name: str):
    return TUNED.get(name, (_KIND_GAIN[CASES[name][0]], 0, 512))


def _is_head(ospec, name: str) -> str:
    """'W' / 'b' for the weight / bias of the layer that emits the spline or affine parameters, '' otherwise."""
    leaf = name.split(".", 1)[1]
    heads = {"maf": ("Wf", "bf"), "nsf": ("csm.W2", "csm.b2") if ospec.nsf_1d else ("Wout", "bout"),
             "nsf_ar": (f"ar.W{ospec.NB}", f"ar.b{ospec.NB}"), "maf_ar": (f"ar.W{ospec.NB}", f"ar.b{ospec.NB}")}[ospec.kind]
    return "W" if leaf == heads[0] else "b" if leaf == heads[1] else ""


def sharpen(ospec, flat, gain: float, seed: int = 0) -> np.ndarray:
    """Head weights x gain, head biases ~ N(0, (gain / 2)^2), LULinear's triangles ~ N(0, 0.3^2); the rest as make_case gives it."""
    rng = np.random.default_rng(seed + 4242)
    out = np.array(flat, dtype=np.float64)
    for name, shape, off in OF.param_layout(ospec):
        n = int(np.prod(shape))
        h = _is_head(ospec, name)
        if h == "W":
            out[off:off + n] *= gain
        elif h == "b":
            out[off:off + n] = rng.normal(size=n) * (gain / 2.0)
        elif name.endswith(("lu.lower", "lu.upper")):
            out[off:off + n] = rng.normal(size=n) * 0.3
    return out.astype(np.float32)


def _first_knots(ospec, flat, x, t: int):
    """fp32 knots (horizontal, vertical) of transform t of a one-parameter flow for the context rows x: [n, K + 1] each.  The
    spline parameters of such a flow depend on the context alone."""
    with torch.no_grad():
        fl = torch.as_tensor(flat, dtype=torch.float32)
        P = OF.views(ospec, fl)
        e = OF.embed_context(ospec, torch.as_tensor(x, dtype=torch.float32))
        if ospec.kind == "nsf":
            q = OF._context_spline_map(ospec, P, t, e)
            cw, _ = OF._knots(ospec, q[..., :ospec.K] / math.sqrt(ospec.H), ospec.min_bin_width)
            ch, _ = OF._knots(ospec, q[..., ospec.K:2 * ospec.K] / math.sqrt(ospec.H), ospec.min_bin_height)
        else:
            q = OF._ar_hyper(ospec, P, t, torch.zeros(len(x), 1), e)[:, 0]
            cw, ch, _ = OF._ar_knots(ospec, q)
    return cw.numpy(), ch.numpy()


@functools.lru_cache(maxsize=None)
def sharp_case(name: str, B: int | None = None, gain: float | None = None, spread: float = 0.5, seed: int | None = None) -> SharpCase:
    """make_case(name) with sharpened heads, theta = mean + sigma * s * N(0, 1) and given noise z = 0.8 * s * N(0, 1), s = 3 on
    every fourth row and 1 elsewhere.

    The one-parameter spline flows (nsf_d1, nsfar_d1) are built with theta_mean = 0 and theta_std = 1, so that the first spline
    sees u = theta exactly, and get edge rows APPENDED (``n_edge`` of them, after the B random rows): theta in {+-bound, the
    neighbouring floats on both sides, 0}, and the oracle's own fp32 knots of transform 0 for three context rows, as theta
    (horizontal knots: the density direction meets them first) and as z (vertical knots; the sampling direction meets transform
    T - 1 first, so that transform's vertical knots are given as z as well).  The splines are C1 at every knot and at +-bound (the
    end derivatives are exactly 1), so log p, theta and the log-determinant need no exemption there; the parameter gradient of
    the log-determinant is NOT continuous across a knot, so the gradient tests use the random rows only."""
    t_gain, t_seed, t_rows = tuned(name)
    B, gain, seed = B or t_rows, t_gain if gain is None else gain, t_seed if seed is None else seed
    ospec, spec, flat, _, x = make_case(name, seed=seed, B=B, spread=spread)
    one_d = ospec.D == 1 and ospec.kind in ("nsf", "nsf_ar")
    if one_d:
        ospec = dataclasses.replace(ospec, theta_mean=np.zeros(1), theta_std=np.ones(1))
        spec = dataclasses.replace(spec, theta_mean=np.zeros(1, np.float32), theta_std=np.ones(1, np.float32))
    flat = sharpen(ospec, flat, gain, seed)
    rng = np.random.default_rng(seed + 977)
    # 3 sigma on every fourth row puts ~2.4 % of the rows beyond EACH end of a spline on [-3, 3]; the zuko splines live on [-5, 5],
    # where 3 sigma would leave 0.6 % there: the wide rows scale with the bound, so the same share sits in the tails
    wide = 3.0 * (ospec.tail_bound / 3.0 if ospec.kind == "nsf_ar" else 1.0)
    s = np.where(np.arange(B) % 4 == 3, wide, 1.0)[:, None]
    theta = (np.asarray(ospec.theta_mean) + np.asarray(ospec.theta_std) * s * rng.normal(size=(B, ospec.D))).astype(np.float32)
    z = (0.8 * s * rng.normal(size=(B, ospec.D))).astype(np.float32)
    n_edge = 0
    if one_d:
        b = np.float32(ospec.tail_bound)
        inf = np.float32(np.inf)
        ends = [b, -b, np.nextafter(b, inf), np.nextafter(-b, -inf), np.nextafter(b, np.float32(0)), np.nextafter(-b, np.float32(0)),
                np.float32(0)]
        cw0, ch0 = _first_knots(ospec, flat, x[:3], 0)
        _, chl = _first_knots(ospec, flat, x[:3], ospec.T - 1)
        K1 = ospec.K + 1
        te = np.concatenate([ends, cw0.reshape(-1), np.zeros(3 * K1)]).astype(np.float32)
        ze = np.concatenate([ends, ch0.reshape(-1), chl.reshape(-1)]).astype(np.float32)
        xe = np.concatenate([x[:len(ends)], np.repeat(x[:3], K1, 0), np.repeat(x[:3], K1, 0)])
        n_edge = len(te)
        theta = np.concatenate([theta, te[:, None]])
        z = np.concatenate([z, ze[:, None]])
        x = np.concatenate([x, xe]).astype(np.float32)
    for a in (flat, theta, x, z):
        a.setflags(write=False)
    return SharpCase(ospec, spec, flat, theta, x, z, n_edge, gain)


def sharp_factory(gain: float | None = None):
    """A make_case-shaped factory (name, B, spread) -> (ospec, spec, flat, theta, x) of sharpened flows."""
    def make(name, B=200, spread=0.5, seed=None):
        c = sharp_case(name, B=B, gain=gain, spread=spread, seed=seed)
        return c.ospec, c.spec, np.array(c.flat), np.array(c.theta), np.array(c.x)
    return make


# ---------------------------------------------------------------------------------------------------------------------------
# what the oracle's splines and affine maps saw
# ---------------------------------------------------------------------------------------------------------------------------
class Trace:
    """``calls``: one dict per spline call -- t, inverse, final (False for the first D - 1 sweeps of an autoregressive inverse,
    whose inputs are not yet those of the finished iterate), idx [B, d] (bin index; meaningless where a tail holds the row), low /
    high [B, d] (tail membership), and (min, max) of w / (2 bound), h / w and the knot derivative over every row, dimension and bin;
    the inputs v [B, d] and, for the nflows spline, the raw parameters q [B, d, 3K - 1].
    ``scales``: (t, inverse, scale [B, D]) per affine call of a MAF / zuko MAF."""

    def __init__(self):
        self.calls, self.scales = [], []

    def of(self, t, inverse):
        return [c for c in self.calls if c["t"] == t and c["inverse"] == inverse and c["final"]]


def _mm(a):
    return float(a.min()), float(a.max())


@contextlib.contextmanager
def spline_trace():
    """Wraps OF.rq_spline, OF.ar_spline, OF.ar_affine and OF._scale_from_unconstrained for the duration of the block.  Transform
    numbers are counted per direction: run one log_prob and / or one inverse_transform of ONE flow inside a block."""
    tr = Trace()
    n = {False: 0, True: 0}
    saved = (OF.rq_spline, OF.ar_spline, OF.ar_affine, OF._scale_from_unconstrained)

    def place(spec, inverse, sweeps):
        i = n[inverse]
        n[inverse] += 1
        per = sweeps if inverse else 1
        t = (i // per) % spec.T
        return (spec.T - 1 - t if inverse else t), (i % per == per - 1)

    def rq(spec, v, q, inverse):
        out = saved[0](spec, v, q, inverse)
        with torch.no_grad():
            K, B = spec.K, spec.tail_bound
            cw, w = OF._knots(spec, q[..., :K] / math.sqrt(spec.H), spec.min_bin_width)
            ch, h = OF._knots(spec, q[..., K:2 * K] / math.sqrt(spec.H), spec.min_bin_height)
            der = spec.min_derivative + torch.nn.functional.softplus(q[..., 2 * K:])
            loc = ch if inverse else cw
            idx = ((v[..., None] >= loc[..., :-1]).sum(-1) - 1).clamp(0, K - 1)
            t, final = place(spec, inverse, 1)
            tr.calls.append(dict(t=t, inverse=inverse, final=final, idx=idx.numpy(), low=(v < -B).numpy(), high=(v > B).numpy(),
                                 w=_mm(w / (2 * B)), slope=_mm(h / w), der=_mm(der), v=v.detach().numpy(), q=q.detach().numpy()))
        return out

    def ar(spec, v, q, inverse):
        out = saved[1](spec, v, q, inverse)
        with torch.no_grad():
            K, B = spec.K, spec.tail_bound
            hor, ver, der = OF._ar_knots(spec, q)
            loc = ver if inverse else hor
            idx = ((v[..., None] >= loc[..., :-1]).sum(-1) - 1).clamp(0, K - 1)
            w, h = hor[..., 1:] - hor[..., :-1], ver[..., 1:] - ver[..., :-1]
            t, final = place(spec, inverse, spec.D)
            tr.calls.append(dict(t=t, inverse=inverse, final=final, idx=idx.numpy(), low=(v < -B).numpy(), high=(v > B).numpy(),
                                 w=_mm(w / (2 * B)), slope=_mm(h / w), der=_mm(der[..., 1:-1]), v=v.detach().numpy()))
        return out

    def aff(spec, v, q, inverse):
        out = saved[2](spec, v, q, inverse)
        t, final = place(spec, inverse, spec.D)
        if final:
            tr.scales.append((t, inverse, torch.exp(out[1].detach() * (-1 if inverse else 1)).numpy()))
        return out

    def scale(spec, a):
        s = saved[3](spec, a)
        tr.scales.append((None, None, s.detach().numpy()))
        return s

    OF.rq_spline, OF.ar_spline, OF.ar_affine, OF._scale_from_unconstrained = rq, ar, aff, scale
    try:
        yield tr
    finally:
        OF.rq_spline, OF.ar_spline, OF.ar_affine, OF._scale_from_unconstrained = saved


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's own fp32 error
# ---------------------------------------------------------------------------------------------------------------------------
def _std_normal_logp(z):
    z = np.asarray(z, dtype=np.float64)
    return -0.5 * (z * z).sum(1) - 0.5 * z.shape[1] * OF.LOG_2PI


def budget(ospec, flat, theta, x, z, quantity: str):
    """{'f64': ..., 'f32': ...}: the oracle in both precisions on the same inputs (every output as float64 numpy).
      logp     log p(theta | x) [B]
      inverse  (theta [B, D], logdet [B], round trip [B]) of the given noise z; round trip = the oracle's own
               log p(inverse(z)) - (log N(z) - logdet) in that precision
      grad     (loss rows [B], d mean(-log p) / d flat) by autograd
      dctx     d sum(-log p) / d x [B, C] by autograd
      dtheta   (log p [B], d log p / d theta [B, D]) by autograd"""
    out = {}
    for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
        fl = torch.as_tensor(np.array(flat)).to(dt)
        th, xx = torch.as_tensor(np.array(theta)).to(dt), torch.as_tensor(np.array(x)).to(dt)
        if quantity == "logp":
            with torch.no_grad():
                out[key] = OF.log_prob(ospec, fl, th, xx).double().numpy()
        elif quantity == "inverse":
            with torch.no_grad():
                t_, ld = OF.inverse_transform(ospec, fl, torch.as_tensor(np.array(z)).to(dt), xx)
                # (the device round trip feeds float32 theta back: so does this one)
                lp = OF.log_prob(ospec, fl, t_.float().to(dt), xx).double().numpy()
            t_, ld = t_.double().numpy(), ld.double().numpy()
            out[key] = (t_, ld, lp - (_std_normal_logp(z) - ld))
        elif quantity == "grad":
            p = fl.clone().requires_grad_(True)
            loss = -OF.log_prob(ospec, p, th, xx)
            loss.mean().backward()
            out[key] = (loss.detach().double().numpy(), p.grad.double().numpy())
        elif quantity == "dctx":
            xg = xx.clone().requires_grad_(True)
            (-OF.log_prob(ospec, fl, th, xg).sum()).backward()
            out[key] = xg.grad.double().numpy()
        elif quantity == "dtheta":
            tg = th.clone().requires_grad_(True)
            lp = OF.log_prob(ospec, fl, tg, xx)
            (g,) = torch.autograd.grad(lp.sum(), tg)
            out[key] = (lp.detach().double().numpy(), g.double().numpy())
        else:
            raise ValueError(quantity)
    return out


@functools.lru_cache(maxsize=None)
def case_budget(name: str, quantity: str, rows: int | None = None, rows_per_x: int = 1):
    """budget() of sharp_case(name), once per session; ``rows``: the first rows only (the gradient batches); ``rows_per_x``: that many
    consecutive rows share a context row (row b sees x[b // rows_per_x], as in sf_flow_log_prob_grad)."""
    c = sharp_case(name)
    n = len(c.theta) if rows is None else rows
    x = c.x[np.arange(n) // rows_per_x]
    return budget(c.ospec, c.flat, c.theta[:n], x, c.z[:n], quantity)


def theta_scale(ospec, theta_ref):
    """max(sigma, |theta_ref - mean|) per element: the unit of the theta bar."""
    return np.maximum(np.asarray(ospec.theta_std), np.abs(theta_ref - np.asarray(ospec.theta_mean)))


def ratios(e_kernel, e_ref):
    """e_kernel / e_ref at the three quantiles (inf where the reference's error is zero and the kernel's is not)."""
    out = []
    for q in QUANTILES:
        k, r = np.quantile(e_kernel, q), np.quantile(e_ref, q)
        out.append(float(k / r) if r > 0 else (0.0 if k == 0 else float("inf")))
    return out


def check_bar(label: str, e_kernel, e_ref, floor: float, factor: float = FACTOR):
    """Prints the three ratios, then asserts quantile_q(e_kernel) <= factor * quantile_q(e_ref) + floor at q = 0.5, 0.99, 1."""
    e_kernel, e_ref = np.abs(np.asarray(e_kernel, dtype=np.float64)).ravel(), np.abs(np.asarray(e_ref, dtype=np.float64)).ravel()
    assert e_kernel.shape == e_ref.shape and e_kernel.size
    assert np.isfinite(e_ref).all(), label
    rs = ratios(e_kernel, e_ref)
    worst = int(np.argmax(e_kernel))
    print(f"SHARP {label}: ratio med/p99/max {rs[0]:.2f} {rs[1]:.2f} {rs[2]:.2f} | kernel max {e_kernel.max():.3e} (element {worst}) "
          f"ref max {e_ref.max():.3e} floor {floor:.1e}")
    assert np.isfinite(e_kernel).all(), (label, "non-finite kernel output")
    for q in QUANTILES:
        k, r = np.quantile(e_kernel, q), np.quantile(e_ref, q)
        assert k <= factor * r + floor, (label, q, k, r, floor)
    return rs
