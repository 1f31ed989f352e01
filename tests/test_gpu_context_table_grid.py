"""The per-galaxy context table of the 16-row MAF sampler (k_maf_ctab16) is built with one wave per (16 galaxies, transform):
galaxies along grid x, transforms along grid y.

A table row must not depend on where its galaxy sits in the launch: which workgroup and wave computed it, how many galaxies
the catalogue has, or which lanes of its wave are padding.  The sampler's draws are keyed by (catalogue row, slot, attempt) and
keep the lowest accepted attempt, so given the same table rows they are bit-identical however the work was scheduled.  Hence the
check: a galaxy sampled ALONE (a table of one row, built by lane 0 of one wave per transform) with its catalogue row as the
random streams' row offset gives exactly the draws and attempt counts it gets inside a ragged catalogue of 131 galaxies (three
workgroups along x, the last one with a single wave of 3 valid lanes).  Shapes: the fused-first-layer kernels (c0 and c0' rows),
one and two hidden blocks, eight transforms, the straddling placement, and a context wider than one 16-column block.
"""
import numpy as np
import pytest
import torch

from cases import make_case
from oracle import flows as OF
from oracle import posterior as OP
from synference_amd.engine import HipFlow
from synference_amd.spec import FlowSpec

pytestmark = pytest.mark.gpu

M, S = 131, 24
PROBES = (0, 15, 16, 63, 64, 127, 128, 130)   # first / last lane of a wave, first / last wave of a workgroup, the ragged end


def _wide_context_case():
    """D = 5, H = 50, T = 3 with C = 37 context columns: three 16-column blocks of the context product, the last one ragged."""
    D, C, H, T = 5, 37, 50, 3
    rng = np.random.default_rng(537)
    perms = OF.random_perms(D, T, 5)
    st = dict(theta_mean=rng.normal(size=D).astype(np.float32), theta_std=rng.uniform(0.5, 2, size=D).astype(np.float32),
              x_mean=rng.normal(size=C).astype(np.float32), x_std=rng.uniform(0.5, 2, size=C).astype(np.float32))
    ospec = OF.FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, **{k: v.astype(np.float64) for k, v in st.items()})
    spec = FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, **st)
    flat = OF.init_params(ospec, 12)
    flat = (flat + 0.2 * rng.normal(size=flat.shape) * np.abs(flat).mean()).astype(np.float32)
    x = (rng.normal(size=(M, C)) * st["x_std"] + st["x_mean"]).astype(np.float32)
    return ospec, spec, flat, x


def _case(name):
    if name == "wide_context":
        return _wide_context_case()
    ospec, spec, flat, _, x = make_case(name, B=M, spread=0.2)
    return ospec, spec, flat, x


@pytest.mark.parametrize("name", ["maf_cfg1", "maf_t8", "maf_nb1", "maf_span6", "maf_cli", "wide_context"])
def test_a_galaxys_draws_do_not_depend_on_its_place_in_the_table_launch(name):
    ospec, spec, flat, x = _case(name)
    D = spec.D
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x[:8], 200, 5, dtype=torch.float32)
    lo = np.quantile(free.reshape(-1, D), 0.1, axis=0).astype(np.float32)
    hi = np.quantile(free.reshape(-1, D), 0.9, axis=0).astype(np.float32)
    f = HipFlow(spec, "cuda:0")
    assert f.describe()["m16_ok"], f.describe()      # really the 16-row path and its table kernel
    f.set_params(torch.as_tensor(flat))
    f.set_sample_time_limit(20)
    whole, nd = f.sample(x, S, lo, hi, seed=17, return_counts=True)
    whole, nd = whole.cpu().numpy(), nd.cpu().numpy()
    assert f.last_unfilled == 0 and np.isfinite(whole).all()
    assert ((whole >= lo) & (whole <= hi)).all()
    try:
        for g in PROBES:
            f.set_sample_row_offset(g)
            alone, nda = f.sample(x[g:g + 1], S, lo, hi, seed=17, return_counts=True)
            assert f.last_unfilled == 0
            assert np.array_equal(alone.cpu().numpy()[0], whole[g]), (name, g)
            assert int(nda.cpu().numpy()[0]) == int(nd[g]), (name, g)
    finally:
        f.set_sample_row_offset(0)
    # different galaxies really have different rows (a table that ignored the galaxy would pass the comparison above)
    assert not np.array_equal(whole[0], whole[64]) and not np.array_equal(whole[128], whole[130])


def test_ragged_catalogue_meets_the_oracle():
    """131 galaxies of the benchmarked shape against the CPU oracle, at the bars of the unrolled-shape test: fewer than 1 % of
    the draws off by more than 5e-4 of the box width, attempt counts within max(3, 2 %)."""
    ospec, spec, flat, x = _case("maf_cfg1")
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x[:8], 200, 5, dtype=torch.float32)
    lo = np.quantile(free.reshape(-1, spec.D), 0.1, axis=0).astype(np.float32)
    hi = np.quantile(free.reshape(-1, spec.D), 0.9, axis=0).astype(np.float32)
    f = HipFlow(spec, "cuda:0")
    f.set_params(torch.as_tensor(flat))
    f.set_sample_time_limit(20)
    got, nd = f.sample(x, S, lo, hi, seed=3, return_counts=True)
    got, nd = got.cpu().double().numpy(), nd.cpu().numpy()
    ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x, S, 3, lo, hi, dtype=torch.float32)
    assert f.last_unfilled == 0 and np.isfinite(got).all()
    err = np.abs((got - ref) / (hi - lo).astype(np.float64)).max(-1)
    assert (err > 5e-4).mean() < 0.01, ((err > 5e-4).mean(), err.max())
    assert np.abs(nd - rnd).sum() <= max(3, 0.02 * rnd.sum())
