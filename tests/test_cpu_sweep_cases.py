"""No GPU: the sampler sweep (tests/sweep_cases.py) on the reference alone.

* The fp32 oracle against the fp64 oracle, per config, under the rule the device is held to in tests/test_gpu_sweep_sampler.py
  (sweep_cases.compare_draws) and a decade tighter: 1e-5 of the box width on every draw whose slot took the same number of attempts
  in both precisions.  The device's bar of 1e-4 is then ten times the reference's own fp32 error, not a figure read off a kernel.
* The sweep box accepts 0.5 .. 0.75 of the proposals at every D, and every unbounded draw is finite.
* Coverage: which sampler families the union of the configs reaches, from describe() of a handle per config (creating a handle
  needs no GPU).  A later edit of the sweep that loses a family fails here, by name."""
import numpy as np
import pytest
import torch

import sweep_cases as SW
from oracle import posterior as OP

M, S, SEED = 4, 65, 2025


@pytest.mark.parametrize("cfg", SW.sweep_configs(), ids=SW.config_id)
def test_fp32_oracle_meets_the_device_rule_against_the_fp64_oracle(cfg):
    c = SW.sweep_case(cfg)
    x, flat = c.x[:M], torch.as_tensor(np.array(c.flat))
    free, _ = OP.sample(c.ospec, flat, x, S, SEED, dtype=torch.float32)
    assert np.isfinite(free).all()
    lo, hi = SW.case_box(cfg, M)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()
    slots = np.arange(M * S, dtype=np.uint64)
    th32, n32 = OP.sample_slots(c.ospec, flat, x, slots, S, SEED, lo, hi, dtype=torch.float32)
    th64, n64 = OP.sample_slots(c.ospec, flat, x, slots, S, SEED, lo, hi, dtype=torch.float64)
    D = c.ospec.D
    worst, flips = SW.compare_draws(th32.reshape(M, S, D), n32.reshape(M, S).sum(1), th64.reshape(M, S, D), n64.reshape(M, S).sum(1),
                                    lo, hi, S)
    same = n32 == n64
    err = np.abs((th32 - th64) / (hi - lo).astype(np.float64)).max(-1)
    acc = M * S / n64.sum()
    print(f"SWEEP {SW.config_id(cfg)}: fp32 oracle worst {err[same].max():.2e} of the box width, slots with other counts "
          f"{int((~same).sum())} of {M * S}, attempts {int(n64.sum())}, acceptance {acc:.3f}")
    assert same.any() and err[same].max() <= 1e-5, err[same].max()
    assert 0.5 <= acc <= 0.75, acc


def _describe(cfg):
    from synference_amd.engine import HipFlow
    return HipFlow(SW.sweep_case(cfg).spec).describe()   # creating a handle needs no GPU


def _families(configs):
    """Family name -> the configs that reach it."""
    want = {}
    for ht in (1, 2, 3, 4):
        want[f"MAF 32-row sampler (m16_ok = 0), HT = {ht}"] = lambda d, ht=ht: d["kind_"] == "maf" and not d["m16_ok"] and d["HT"] == ht
    for nb in (1, 2, 3, 4):
        want[f"MAF 32-row sampler (m16_ok = 0), NB = {nb}"] = lambda d, nb=nb: d["kind_"] == "maf" and not d["m16_ok"] and d["NB"] == nb
    want["MAF image not LDS-resident (n_parts = 0)"] = lambda d: d["kind_"] == "maf" and d["n_parts"] == 0
    for sp in (0, 1):
        want[f"MAF 16-row sampler (m16_ok = 1), m16_span = {sp}"] = lambda d, sp=sp: d["kind_"] == "maf" and d["m16_ok"] and d["m16_span"] == sp
    for pt in (2, 3):
        want[f"NSF PT = {pt}"] = lambda d, pt=pt: d["kind_"] == "nsf" and d["PT"] == pt
    for nb in (1, 2, 3, 4):
        want[f"NSF NB = {nb}"] = lambda d, nb=nb: d["kind_"] == "nsf" and d["NB"] == nb
    for ok in (0, 1):
        want[f"NSF nsf_split_sampler = {ok}"] = lambda d, ok=ok: d["kind_"] == "nsf" and d["nsf_split_sampler"] == ok
    for n in (1, 2, 4):
        want[f"NSF n_parts = {n}"] = lambda d, n=n: d["kind_"] == "nsf" and d["n_parts"] == n
    for D in (2, 16):
        want[f"NSF D = {D}"] = lambda d, D=D: d["kind_"] == "nsf" and d["D"] == D
    reached = {name: [] for name in want}
    for cfg in configs:
        if len(cfg) != 8:        # the flows outside the two tile engines have one sampler each
            continue
        d = _describe(cfg)
        d["kind_"] = cfg[0]
        for name, hit in want.items():
            if hit(d):
                reached[name].append(cfg)
    return reached


def test_the_sweep_reaches_every_sampler_family():
    reached = _families(SW.sweep_configs())
    for name, cfgs in reached.items():
        print(f"{name}: {len(cfgs)} configs, first {cfgs[0] if cfgs else None}")
    missing = [name for name, cfgs in reached.items() if not cfgs]
    assert not missing, "the sampler sweep no longer reaches: " + "; ".join(missing)
    # and so does the short list that runs the second geometry (several galaxies per wave)
    missing = [name for name, cfgs in _families(SW.DENSE_WAVE_CONFIGS).items() if not cfgs]
    assert not missing, "sweep_cases.DENSE_WAVE_CONFIGS no longer reaches: " + "; ".join(missing)


def test_the_lds_refusal_is_predicted_for_the_lampe_configs():
    """flow_or_lds_refusal: a handle for every lampe config that fits, the named refusal for the others (no GPU needed)."""
    n = 0
    for cfg in SW.sweep_configs():
        spec = SW.sweep_case(cfg).spec
        if spec.kind in ("nsf_ar", "maf_ar"):
            f = SW.flow_or_lds_refusal(spec)
            assert (f is None) == SW.lampe_lds_refused(spec)
            n += f is not None
    assert n >= 10, n
