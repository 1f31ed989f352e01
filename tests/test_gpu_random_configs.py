"""Randomised configuration sweep (fixed seeds): every supported shape family against the fp64 oracle --
log_prob, inverse-from-noise, flat gradient and context gradient.  Catches layout / padding / staging
corner cases that the named cases do not hit (multi-tile contexts, HT = 1..4, D up to 16, K 2..16)."""
import numpy as np
import pytest
import torch

from oracle import flows as OF
from sweep_cases import _configs, _configs_other_kinds, build_case, flow_or_lds_refusal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,D,C,H,T,K,NB,seed", _configs())
def test_random_config_matches_oracle(kind, D, C, H, T, K, NB, seed):
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x, z, st = build_case((kind, D, C, H, T, K, NB, seed))
    B = len(theta)
    f = HipFlow(spec, "cuda:0")
    f.set_params(torch.as_tensor(flat))
    pt = torch.tensor(flat, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lp_ref = OF.log_prob(ospec, pt, torch.as_tensor(theta).double(), xt)
    (-lp_ref).mean().backward()
    lp = f.log_prob(theta, x).cpu().double().numpy()
    assert np.abs(lp - lp_ref.detach().numpy()).max() < 1e-4 * max(1.0, D / 4)
    with torch.no_grad():
        th_ref, ld_ref = OF.inverse_transform(ospec, pt.detach(), torch.as_tensor(z).double(), xt.detach())
    th, ld = f.inverse(z, x)
    scale = np.maximum(np.abs(th_ref.numpy()), st["theta_std"])
    assert np.abs((th.cpu().double().numpy() - th_ref.numpy()) / scale).max() < 5e-4
    assert np.abs(ld.cpu().double().numpy() - ld_ref.numpy()).max() < 5e-4 * max(1.0, D / 4)
    dctx = torch.empty(B, C, device="cuda")
    _, grad = f.loss_grad(torch.as_tensor(flat), theta, x, 1.0 / B, dctx_out=dctx)
    g, rg = grad.cpu().double().numpy(), pt.grad.numpy()
    assert np.abs(g - rg).max() < 3e-4 * max(np.abs(rg).max(), 1e-6)
    rd = xt.grad.numpy()
    assert np.abs(dctx.cpu().double().numpy() - rd).max() < 3e-4 * max(np.abs(rd).max(), 1e-6)
    # sampler: finite and reproducible (its draws against the oracle's: tests/test_gpu_sweep_sampler.py, over these same configs)
    s1 = f.sample(x[:3], 40, seed=5).cpu().numpy()
    s2 = f.sample(x[:3], 40, seed=5).cpu().numpy()
    assert np.isfinite(s1).all() and np.array_equal(s1, s2)


@pytest.mark.parametrize("kind,D,C,H,T,K,seed", _configs_other_kinds())
def test_random_config_of_the_other_flow_kinds_matches_oracle(kind, D, C, H, T, K, seed):
    ospec, spec, flat, theta, x, z, st = build_case((kind, D, C, H, T, K, seed))
    B = len(theta)   # (77: two waves of the thread-per-sample kernels, the second ragged)
    f = flow_or_lds_refusal(spec)   # a wave's rows must fit the CU's LDS: shapes beyond that are refused at creation, by name
    if f is None:
        return
    f.set_params(torch.as_tensor(flat))
    pt = torch.tensor(flat, dtype=torch.float64, requires_grad=True)
    lp_ref = OF.log_prob(ospec, pt, torch.as_tensor(theta).double(), torch.as_tensor(x).double())
    (-lp_ref).mean().backward()
    lp = f.log_prob(theta, x).cpu().double().numpy()
    assert np.abs(lp - lp_ref.detach().numpy()).max() < 1e-4 * max(1.0, D / 4)
    with torch.no_grad():
        th_ref, ld_ref = OF.inverse_transform(ospec, pt.detach(), torch.as_tensor(z).double(), torch.as_tensor(x).double())
    th, ld = f.inverse(z, x)
    scale = np.maximum(np.abs(th_ref.numpy()), st["theta_std"])
    assert np.abs((th.cpu().double().numpy() - th_ref.numpy()) / scale).max() < 5e-4
    assert np.abs(ld.cpu().double().numpy() - ld_ref.numpy()).max() < 5e-4 * max(1.0, D / 4)
    loss, grad = f.loss_grad(torch.as_tensor(flat), theta, x, 1.0 / B)
    assert np.abs(loss.cpu().double().numpy() + lp_ref.detach().numpy()).max() < 1e-4 * max(1.0, D / 4)
    g, rg = grad.cpu().double().numpy(), pt.grad.numpy()
    assert np.abs(g - rg).max() < 3e-4 * max(np.abs(rg).max(), 1e-6)
    with pytest.raises(RuntimeError):
        f.loss_grad(torch.as_tensor(flat), theta, x, 1.0 / B, dctx_out=torch.empty(B, C, device="cuda"))
    s1 = f.sample(x[:3], 40, seed=5).cpu().numpy()
    s2 = f.sample(x[:3], 40, seed=5).cpu().numpy()
    assert np.isfinite(s1).all() and np.array_equal(s1, s2)
