"""GPU: the fused-first-layer sampler kernels (sf_maf16.hip, PREC 2: first layer as rank-1 updates in degree order, draw state
handed to the passes by degree) fed GIVEN noise through the parity hook, against the fp64 oracle, on every shape they serve:
D = 3, 4, 5 (one degree group per hidden tile) x one / two hidden blocks x both scale parametrisations, with random
permutations between the transforms."""
import numpy as np
import pytest
import torch

from cases import oracle_inverse
from oracle import flows as OF
from synference_amd.spec import FlowSpec

pytestmark = pytest.mark.gpu

# D -> H with one degree group of 12-14 units per 16-row tile (the unrolled kernels' placement)
SHAPES = {3: 26, 4: 40, 5: 50}


def _case(D, NB, scale_fn, seed, B, C=7, T=4):
    H = SHAPES[D]
    rng = np.random.default_rng(seed)
    perms = OF.random_perms(D, T, seed)
    st = dict(theta_mean=rng.normal(size=D).astype(np.float32),
              theta_std=rng.uniform(0.5, 2.0, size=D).astype(np.float32),
              x_mean=rng.normal(size=C).astype(np.float32),
              x_std=rng.uniform(0.5, 2.0, size=C).astype(np.float32))
    extra = dict(NB=NB, scale_fn=scale_fn)
    ospec = OF.FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, **extra,
                        **{k: v.astype(np.float64) for k, v in st.items()})
    spec = FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, **extra, **st)
    flat = OF.init_params(ospec, seed + 1)
    flat = (flat + 0.5 * rng.normal(size=flat.shape) * np.abs(flat).mean()).astype(np.float32)
    x = (rng.normal(size=(B, C)) * st["x_std"] + st["x_mean"]).astype(np.float32)
    z = rng.normal(size=(B, D)).astype(np.float32)
    return ospec, spec, flat, x, z


@pytest.mark.parametrize("scale_fn", ["softplus", "sigmoid2"])
@pytest.mark.parametrize("NB", [1, 2])
@pytest.mark.parametrize("D", [3, 4, 5])
def test_fused_sampler_from_given_noise(D, NB, scale_fn):
    from synference_amd.engine import HipFlow
    seed = 100 * D + 10 * NB + (scale_fn == "sigmoid2")
    ospec, spec, flat, x, z = _case(D, NB, scale_fn, seed, B=2051)   # ragged: not a multiple of the 128-row workgroup
    f = HipFlow(spec, "cuda:0")
    f.set_params(torch.as_tensor(flat))
    rth, _ = oracle_inverse(ospec, flat, z, x, torch.float64)
    scale = np.asarray(ospec.theta_std)
    th, _ = f.inverse_sampler(z, x)
    assert f.last_sampler_rc == 3, f.last_sampler_rc   # the fused pass functions, not a fallback
    th = th.cpu().double().numpy()
    assert np.isfinite(th).all()
    err = np.abs((th - rth) / scale).max()
    th32, _ = f.inverse(z, x)   # the generic all-fp32 hook on the same rows
    err32 = np.abs((th32.cpu().double().numpy() - rth) / scale).max()
    assert err <= 1e-4, err
    assert err <= max(3.0 * err32, 2e-5), (err, err32)
    # a second parameter set on the same handle: W' follows the parameters
    flat2 = (flat * 0.9).astype(np.float32)
    f.set_params(torch.as_tensor(flat2))
    rth2, _ = oracle_inverse(ospec, flat2, z, x, torch.float64)
    th2, _ = f.inverse_sampler(z, x)
    assert f.last_sampler_rc == 3
    err2 = np.abs((th2.cpu().double().numpy() - rth2) / scale).max()
    assert err2 <= 1e-4, err2
    print(f"D={D} NB={NB} {scale_fn}: max |dtheta|/sigma fused {err:.2e} (second parameters {err2:.2e}), generic fp32 hook {err32:.2e}")
