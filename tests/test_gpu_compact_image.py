"""GPU: the compact fused image of the fp32 16-row sampler (sf_layout.h: packed16c; sf_maf16.hip: sf_stage16c) as
k_maf_samp16 / k_maf_find16s, PREC 2, stage and read it -- one contiguous block per transform holding exactly what the fused
passes read, rebuilt on the device whenever the parameters change.

Every shape the unrolled fused kernels serve (D = 3, 4, 5 with one degree group per hidden tile x one / two hidden blocks) at
T = 1, 2 and 5 transforms.

Bars: given noise against the fp64 oracle as in test_gpu_fused_first_layer.py (1e-4 of sigma, and no worse than three times the
generic fp32 hook or 2e-5); catalogues against the oracle sampler as in test_gpu_context_table_grid.py (fewer than 1 % of the
draws off by more than 5e-4 of the box width, counts within max(3, 2 %)); everything else bit for bit."""
import numpy as np
import pytest
import torch

from cases import oracle_inverse
from oracle import flows as OF
from oracle import posterior as OP
from synference_amd.spec import FlowSpec

pytestmark = pytest.mark.gpu

SHAPES = {3: 24, 4: 36, 5: 50}   # D -> H: every degree group fills one 16-row tile (12-13 units)
GRID = [(D, NB, T) for D in (3, 4, 5) for NB in (1, 2) for T in (1, 2, 5)]
S = 130                          # draws per galaxy: more than one 128-item iteration, and ragged
C = 7


def _case(D, NB, T, M):
    seed = 1000 * D + 100 * NB + T
    H = SHAPES[D]
    rng = np.random.default_rng(seed)
    perms = OF.random_perms(D, T, seed)
    st = dict(theta_mean=rng.normal(size=D).astype(np.float32),
              theta_std=rng.uniform(0.5, 2.0, size=D).astype(np.float32),
              x_mean=rng.normal(size=C).astype(np.float32),
              x_std=rng.uniform(0.5, 2.0, size=C).astype(np.float32))
    ospec = OF.FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, NB=NB,
                        **{k: v.astype(np.float64) for k, v in st.items()})
    spec = FlowSpec(kind="maf", D=D, C=C, H=H, T=T, K=10, perms=perms, NB=NB, **st)
    flat = OF.init_params(ospec, seed + 1)
    flat = (flat + 0.5 * rng.normal(size=flat.shape) * np.abs(flat).mean()).astype(np.float32)
    x = (rng.normal(size=(M, C)) * st["x_std"] + st["x_mean"]).astype(np.float32)
    return ospec, spec, flat, x, rng


def _flow(spec, flat):
    from synference_amd.engine import HipFlow
    f = HipFlow(spec, "cuda:0")
    d = f.describe()
    assert d["c16_fix"] == 1 and d["t16c_stride"] % 256 == 0, d   # the compact image exists with the hard-wired offsets
    f.set_params(torch.as_tensor(flat))
    f.set_sample_time_limit(20)
    return f


def _assert_fused(f, x):
    """The persistent sampler and the find / resolve launches over these rows take the fused PREC 2 kernels on the compact image
    (asked with the context table attached, as at a launch): not the two-layer fp32 kernels the plan falls back to without it."""
    xt = torch.as_tensor(x, dtype=torch.float32, device="cuda:0").contiguous()
    f.prepare_context(xt)
    try:
        assert f.sampler_fused()
    finally:
        f.release_context()
    assert not f.sampler_fused()   # (no table, no fused kernels: the query really looks at the run-time state)


def _box(ospec, flat, x_rows, q, n=400):
    free, _ = OP.sample(ospec, torch.as_tensor(flat), x_rows, n, 5, dtype=torch.float32)
    free = free.reshape(-1, ospec.D)
    return np.quantile(free, q, axis=0).astype(np.float32), np.quantile(free, 1.0 - q, axis=0).astype(np.float32)


def _meets_oracle(got, ref, lo, hi):
    off = np.abs((got - ref) / (hi - lo)).max(-1) > 5e-4
    return float(off.mean())


@pytest.mark.parametrize("D,NB,T", GRID)
def test_given_noise_through_the_compact_image(D, NB, T):
    """k_maf_find16s in its given-noise mode: one row (three waves without an item still copy and meet the barrier) and 3 x 130
    rows (four workgroups, the last one ragged)."""
    ospec, spec, flat, x, rng = _case(D, NB, T, 3 * S)
    z = rng.normal(size=(3 * S, D)).astype(np.float32)
    f = _flow(spec, flat)
    rth, _ = oracle_inverse(ospec, flat, z, x, torch.float64)
    scale = np.asarray(ospec.theta_std)
    th32, _ = f.inverse(z, x)   # the generic all-fp32 hook on the same rows
    err32 = np.abs((th32.cpu().double().numpy() - rth) / scale).max()
    for n in (1, 3 * S):
        th, _ = f.inverse_sampler(z[:n], x[:n])
        assert f.last_sampler_rc == 3, f.last_sampler_rc   # the fused pass functions, not a fallback
        th = th.cpu().double().numpy()
        assert np.isfinite(th).all()
        err = np.abs((th - rth[:n]) / scale).max()
        print(f"D={D} NB={NB} T={T} rows={n}: max |dtheta|/sigma fused {err:.2e}, generic fp32 hook {err32:.2e}")
        assert err <= 1e-4, err
        assert err <= max(3.0 * err32, 2e-5), (err, err32)


@pytest.mark.parametrize("D,NB,T", GRID)
def test_catalogues_through_the_persistent_sampler(D, NB, T):
    """k_maf_samp16: 3 galaxies x 130 draws against the oracle sampler; each galaxy alone and the single draw of a 1 x 1
    catalogue equal their place in it bit for bit; after set_params with other weights the handle samples what a fresh one
    with those weights does."""
    ospec, spec, flat, x, rng = _case(D, NB, T, 3)
    lo, hi = _box(ospec, flat, x, 0.1)
    f = _flow(spec, flat)
    _assert_fused(f, x)
    whole, nd = f.sample(x, S, lo, hi, seed=17, return_counts=True)
    whole, nd = whole.cpu().numpy(), nd.cpu().numpy()
    assert f.last_unfilled == 0 and np.isfinite(whole).all()
    assert ((whole >= lo) & (whole <= hi)).all()
    ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x, S, 17, lo, hi, dtype=torch.float32)
    bad = _meets_oracle(whole.astype(np.float64), ref, lo, hi)
    print(f"D={D} NB={NB} T={T}: draws off the oracle {bad:.4f}, attempts {nd.tolist()} oracle {np.asarray(rnd).tolist()}")
    assert bad < 0.01, bad
    assert (np.abs(nd - rnd) <= np.maximum(3, 0.02 * rnd)).all(), (nd, rnd)
    try:
        for g in range(3):
            f.set_sample_row_offset(g)
            alone = f.sample(x[g:g + 1], S, lo, hi, seed=17).cpu().numpy()
            assert f.last_unfilled == 0
            assert np.array_equal(alone[0], whole[g]), g
    finally:
        f.set_sample_row_offset(0)
    one = f.sample(x[:1], 1, lo, hi, seed=17).cpu().numpy()   # slot 0 of both catalogues: the same random stream
    assert f.last_unfilled == 0 and np.array_equal(one[0, 0], whole[0, 0])
    # stale image: the compact image follows the parameters
    flat2 = (flat * 0.9).astype(np.float32)
    f.set_params(torch.as_tensor(flat2))
    _assert_fused(f, x)
    second = f.sample(x, S, lo, hi, seed=17).cpu().numpy()
    assert f.last_unfilled == 0
    fresh = _flow(spec, flat2).sample(x, S, lo, hi, seed=17).cpu().numpy()
    assert np.array_equal(second, fresh)
    assert not np.array_equal(second, whole)


@pytest.mark.parametrize("D,NB,T", GRID)
def test_tight_box_retries_and_acceptance_counts(D, NB, T):
    """A box that a first attempt meets about one time in ten: most slots are retried (the tail iterations run with several
    attempts per entry), and the acceptance counts run on k_maf_find16s with Philox noise.  Two near-identical galaxies, so
    that both see that box."""
    ospec, spec, flat, x, rng = _case(D, NB, T, 1)
    x = np.concatenate([x, x * np.float32(1.01)]).astype(np.float32)
    q = 0.5 * (1.0 - 0.1 ** (1.0 / D))   # central fraction 0.1^(1/D) per dimension
    lo, hi = _box(ospec, flat, x[:1], q)
    f = _flow(spec, flat)
    _assert_fused(f, x)
    n = 2000
    acc = f.acceptance(x, n, lo, hi, seed=3).cpu().double().numpy()   # fractions of the n draws
    racc = OP.acceptance(ospec, torch.as_tensor(flat), x, n, 3, lo, hi, dtype=torch.float32)
    print(f"D={D} NB={NB} T={T}: first-attempt acceptance {acc} oracle {racc}")
    assert (np.abs(acc - racc) * n <= max(3, 0.02 * n * racc.max())).all(), (acc * n, racc * n)
    assert 0.02 < racc[0] < 0.4, racc   # (the test's own set-up: "about 0.1")
    whole, nd = f.sample(x, S, lo, hi, seed=29, return_counts=True)
    whole, nd = whole.cpu().numpy(), nd.cpu().numpy()
    assert f.last_unfilled == 0 and np.isfinite(whole).all()
    assert ((whole >= lo) & (whole <= hi)).all()
    assert (nd > 2 * S).all(), nd   # retries really ran
    ref, rnd = OP.sample(ospec, torch.as_tensor(flat), x, S, 29, lo, hi, dtype=torch.float32)
    bad = _meets_oracle(whole.astype(np.float64), ref, lo, hi)
    print(f"D={D} NB={NB} T={T}: draws off the oracle {bad:.4f}, attempts {nd.tolist()} oracle {np.asarray(rnd).tolist()}")
    assert bad < 0.01, bad
    assert (np.abs(nd - rnd) <= np.maximum(3, 0.02 * rnd)).all(), (nd, rnd)
    try:
        for g in range(2):
            f.set_sample_row_offset(g)
            alone = f.sample(x[g:g + 1], S, lo, hi, seed=29).cpu().numpy()
            assert f.last_unfilled == 0
            assert np.array_equal(alone[0], whole[g]), g
    finally:
        f.set_sample_row_offset(0)


@pytest.mark.parametrize("D,NB,T", GRID)
def test_narrow_box_reaches_the_find_and_resolve_launches(D, NB, T):
    """A box that an attempt meets about once in a thousand: some slots use up the persistent launch's first window of 1 024
    attempts and are filled by the find / resolve launches of the deep tail (k_maf_find16s in its best / att_list modes, 32 or
    more attempts per survivor side by side).  Every slot keeps its lowest accepted attempt, so a galaxy sampled alone still
    equals its place in the catalogue bit for bit."""
    ospec, spec, flat, x, rng = _case(D, NB, T, 1)
    x = np.concatenate([x, x * np.float32(1.01)]).astype(np.float32)
    q = 0.5 * (1.0 - 1e-3 ** (1.0 / D))   # central fraction 1e-3^(1/D) per dimension
    lo, hi = _box(ospec, flat, x[:1], q, n=4000)
    f = _flow(spec, flat)
    _assert_fused(f, x)
    whole, nd = f.sample(x, S, lo, hi, seed=31, return_counts=True)
    whole, nd = whole.cpu().numpy(), nd.cpu().numpy()
    print(f"D={D} NB={NB} T={T}: rounds {f.last_sample_stats['rounds']}, attempts per slot {(nd / S).tolist()}")
    assert f.last_unfilled == 0 and np.isfinite(whole).all()
    assert ((whole >= lo) & (whole <= hi)).all()
    assert f.last_sample_stats["rounds"] >= 3   # the persistent launch and at least one find / resolve pair
    try:
        for g in range(2):
            f.set_sample_row_offset(g)
            alone, nda = f.sample(x[g:g + 1], S, lo, hi, seed=31, return_counts=True)
            assert f.last_unfilled == 0
            assert np.array_equal(alone.cpu().numpy()[0], whole[g]), g
            assert int(nda.cpu().numpy()[0]) == int(nd[g]), g
    finally:
        f.set_sample_row_offset(0)
