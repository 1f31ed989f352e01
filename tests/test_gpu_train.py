"""GPU parity of the training kernels: loss and flat gradient vs torch.autograd on the fp64 oracle."""
import numpy as np
import pytest
import torch

from cases import CASES, make_case
from oracle import flows as OF

pytestmark = pytest.mark.gpu
import os as _os
ROOT_DIR = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))


def oracle_loss_grad(ospec, flat, theta, x):
    p = torch.tensor(flat, dtype=torch.float64, requires_grad=True)
    lp = OF.log_prob(ospec, p, torch.as_tensor(theta).double(), torch.as_tensor(x).double())
    loss = -lp
    loss.mean().backward()
    return loss.detach().numpy(), p.grad.numpy()


def masked_reference(ospec, g):
    """MADE-masked entries never receive gradient; the oracle applies W*M so autograd already
    returns exact zeros there -- nothing to do, kept for clarity."""
    return g


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("B", [37, 256])
def test_loss_grad_matches_autograd(name, B):
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=B)
    f = HipFlow(spec, "cuda:0")
    loss, grad = f.loss_grad(torch.as_tensor(flat), theta, x, 1.0 / B)
    loss, grad = loss.cpu().double().numpy(), grad.cpu().double().numpy()
    rloss, rgrad = oracle_loss_grad(ospec, flat, theta, x)
    assert np.abs(loss - rloss).max() < 1e-4, np.abs(loss - rloss).max()
    denom = np.abs(rgrad).max()
    err = np.abs(grad - rgrad).max() / denom
    assert err < 2e-4, (err, denom)
    # per-tensor check so a wrong small tensor cannot hide behind a big one
    for n, s, o in OF.param_layout(ospec):
        k = int(np.prod(s))
        d = np.abs(grad[o:o + k] - rgrad[o:o + k]).max()
        assert d < 2e-4 * max(denom, 1e-12) + 1e-7, (n, d, np.abs(rgrad[o:o + k]).max())
    # the forward image was refreshed by loss_grad: log_prob must now agree with -loss
    lp = f.log_prob(theta, x).cpu().double().numpy()
    assert np.abs(lp + rloss).max() < 1e-4


def test_adam_step_matches_torch():
    from synference_amd import _lib
    import ctypes as C
    lib = _lib.load()
    n = 10007
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g)
    for decoupled, wd in ((0, 0.0), (1, 0.01)):
        p_ref = torch.nn.Parameter(p0.clone().double())
        opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p_ref], lr=1e-3, weight_decay=wd)
        p = p0.clone().cuda()
        d = _lib.sf_adam_desc(1e-3, 0.9, 0.999, 1e-8, wd, decoupled)
        h = C.c_void_p()
        _lib.check(lib.sf_opt_create(n, C.byref(d), C.byref(h)))
        norm = torch.zeros(1, device="cuda")
        for step in range(5):
            gr = torch.randn(n, generator=g) * (3.0 if step % 2 else 0.01)
            p_ref.grad = gr.double().clone()
            tn = torch.nn.utils.clip_grad_norm_([p_ref], 5.0)
            opt.step()
            gd = gr.cuda()
            _lib.check(lib.sf_adam_step(h, C.c_void_p(p.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_float(5.0),
                                        C.c_void_p(norm.data_ptr()), None))
            torch.cuda.synchronize()
            assert abs(norm.item() - tn.item()) / tn.item() < 1e-5
            assert (p.cpu().double() - p_ref.detach()).abs().max() < 2e-6
        lib.sf_opt_destroy(h)


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3", "nsf_odd", "maf_wide"])
def test_context_gradient_matches_autograd(name):
    """dctx = d(sum_b w_b * -log p_b)/dx, the gradient an embedding net in front of the flow receives."""
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=70)
    w = np.random.default_rng(3).uniform(0.5, 1.5, size=70).astype(np.float32)
    f = HipFlow(spec, "cuda:0")
    dctx = torch.empty(70, spec.C, device="cuda")
    f.loss_grad(torch.as_tensor(flat), theta, x, 1.0, weights=torch.as_tensor(w), dctx_out=dctx)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lp = OF.log_prob(ospec, torch.tensor(flat).double(), torch.as_tensor(theta).double(), xt)
    (-(lp * torch.as_tensor(w).double()).sum()).backward()
    ref = xt.grad.numpy()
    err = np.abs(dctx.cpu().double().numpy() - ref).max() / max(np.abs(ref).max(), 1e-12)
    assert err < 2e-4, err


def test_torch_embedding_net_trains_through_the_hip_flow():
    """Any nn.Module embedding: forward in torch, flow + context gradient in HIP, joint gradients equal
    the oracle's (same module in fp64 in front of the oracle flow)."""
    import copy
    from synference_amd.estimator import build_flow
    rng = np.random.default_rng(0)
    B, D, C = 96, 4, 12
    theta = rng.normal(size=(B, D)).astype(np.float32)
    x = (rng.normal(size=(B, C)) * 3 + 1).astype(np.float32)
    torch.manual_seed(0)
    emb = torch.nn.Sequential(torch.nn.Linear(C, 16), torch.nn.SiLU(), torch.nn.Linear(16, 6))
    est = build_flow("nsf", theta, x, hidden_features=24, num_transforms=2, num_bins=6,
                     embedding_net=copy.deepcopy(emb), device="cuda:0",
                     generator=torch.Generator().manual_seed(1)).to("cuda")
    assert est.spec.C == 6 and est.has_embedding
    losses = est.loss(torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda())
    losses.mean().backward()
    # oracle twin
    s = est.spec
    ospec = OF.FlowSpec(kind="nsf", D=D, C=6, H=24, T=2, K=6, theta_mean=s.theta_mean.astype(np.float64),
                        theta_std=s.theta_std.astype(np.float64))
    emb64 = copy.deepcopy(emb).double()
    p = est.flat.detach().cpu().double().requires_grad_(True)
    xs = (torch.as_tensor(x).double() - est.x_mean_raw.cpu().double()) / est.x_std_raw.cpu().double()
    ref_loss = -OF.log_prob(ospec, p, torch.as_tensor(theta).double(), emb64(xs))
    ref_loss.mean().backward()
    assert (losses.detach().cpu().double() - ref_loss.detach()).abs().max() < 1e-4
    g = est.flat.grad.cpu().double()
    assert (g - p.grad).abs().max() < 2e-4 * p.grad.abs().max()
    for (n, q), (_, r) in zip(est.embedding_net.named_parameters(), emb64.named_parameters()):
        assert (q.grad.cpu().double() - r.grad).abs().max() < 2e-4 * max(r.grad.abs().max().item(), 1e-9), n
    # and the runner trains it (generic autograd path) and samples through it
    from synference_amd.posterior import FlowPosterior
    from synference_amd.runner import train_flow
    out = train_flow(est, torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda(), batch_size=32,
                     learning_rate=5e-3, stop_after_epochs=3, max_num_epochs=6, seed=0, log_every=0)
    assert out["training_loss"][-1] < out["training_loss"][0]
    smp = FlowPosterior(est, None).sample_catalogue(x[:5], 40, seed=1)
    assert smp.shape == (5, 40, D) and torch.isfinite(smp).all()


@pytest.mark.parametrize("widths,act,n_in", [([32, 16], "SiLU", 10), ([64, 50, 8], "ReLU", 37), ([20], "Tanh", 5),
                                              ([100, 64, 32, 12], "SiLU", 70)])
def test_hip_fcn_forward_backward_match_torch(widths, act, n_in):
    """The HIP embedding MLP vs the same MLP in torch fp64 (ili FCN semantics: no activation after the last layer)."""
    from synference_amd.embedding import FCN
    g = torch.Generator().manual_seed(0)
    m = FCN(widths, act, n_input=n_in, generator=g).to("cuda")
    x = torch.randn(75, n_in, generator=g) * 2
    layers, n_prev = [], n_in
    T = m.named_tensors()
    for l, w in enumerate(widths):
        lin = torch.nn.Linear(n_prev, w).double()
        lin.weight.data.copy_(T[f"layers.{l}.weight"].cpu().double()); lin.bias.data.copy_(T[f"layers.{l}.bias"].cpu().double())
        layers.append(lin)
        if l + 1 < len(widths):
            layers.append({"SiLU": torch.nn.SiLU(), "ReLU": torch.nn.ReLU(), "Tanh": torch.nn.Tanh()}[act])
        n_prev = w
    ref = torch.nn.Sequential(*layers)
    out = m(x.cuda())
    rout = ref(x.double())
    assert out.shape == (75, widths[-1])
    assert (out.cpu().double() - rout).abs().max() < 1e-4 * max(1.0, rout.abs().max().item())
    gout = torch.randn(75, widths[-1], generator=g)
    (out * gout.cuda()).sum().backward()
    (rout * gout.double()).sum().backward()
    lay, _ = m.layout()
    gflat = m.flat.grad.cpu().double()
    for name, shape, off in lay:
        l = int(name.split(".")[1])
        lin = [q for q in ref if isinstance(q, torch.nn.Linear)][l]
        rg = (lin.weight.grad if name.endswith("weight") else lin.bias.grad).reshape(-1)
        k = rg.numel()
        assert (gflat[off:off + k] - rg).abs().max() < 2e-4 * max(rg.abs().max().item(), 1e-9), name


def test_hip_fcn_embedding_in_front_of_the_flow_end_to_end():
    from synference_amd import FCN, SBI_Fitter
    from synference_amd.synthetic import make_catalogue
    x, theta, names = make_catalogue(3000, 10, 5, seed=5)
    f = SBI_Fitter("fcn", names, [f"F{i}" for i in range(10)], feature_array=x, parameter_array=theta)
    post, stats = f.run_single_sbi(model_type="maf", hidden_features=50, num_transforms=3, training_batch_size=256,
                                   learning_rate=2e-3, stop_after_epochs=2, max_num_epochs=8, random_seed=2,
                                   save_model=False, verbose=False, embedding_net=FCN([32, 8]))
    est = post.posteriors[0].posterior_estimator
    assert est.has_embedding and est.spec.C == 8
    assert stats[0]["training_loss"][-1] < stats[0]["training_loss"][0] - 0.3
    s = f.sample_posterior(f._X_test[:8], num_samples=64, seed=1)
    assert s.shape == (8, 64, 5) and np.isfinite(s).all()
    lp = f.log_prob(f._X_test[:8], f._y_test[:8], norm_posterior=False)
    assert np.isfinite(lp).all()


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3"])
def test_fused_epoch_equals_the_per_step_loop(name):
    """sf_flow_train_epoch (row gather fused into the kernel, loss summed on the device, no host round trip per
    step) reproduces the per-step path: loss_grad on gathered rows + clip + Adam.  f32 atomics may reorder sums."""
    from synference_amd.engine import HipFlow
    from synference_amd.runner import HipAdam, HipTrainOps
    ospec, spec, flat0, theta, x = make_case(name, B=900)
    dev = torch.device("cuda:0")
    T = torch.as_tensor(theta, dtype=torch.float32, device=dev).contiguous()
    X = torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    g = torch.Generator().manual_seed(3)
    order = torch.randperm(900, generator=g).to(dev)
    nb, bs = 7, 96                                   # ragged: 96 is not a multiple of the 32-row tile... it is; 7*96 < 900

    def run(fused):
        f = HipFlow(spec, dev)
        flat = torch.as_tensor(flat0, dtype=torch.float32, device=dev).clone()
        opt = HipAdam(flat, lr=3e-3)
        grad = torch.empty_like(flat)
        tl = torch.zeros((), dtype=torch.float64, device=dev)
        if fused:
            class E:  # minimal estimator stand-in for HipTrainOps
                flow = f
            # two epochs (the second continues the Adam step count of the first)
            ops = HipTrainOps(E)
            ops.train_epoch(flat, T, X, order, nb, bs, 1.0 / bs, opt, 5.0, grad, tl)
            ops.train_epoch(flat, T, X, order, nb, bs, 1.0 / bs, opt, 5.0, grad, tl)
        else:
            for ep in range(2):
                for b in range(nb):
                    idx = order[b * bs:(b + 1) * bs]
                    loss, _ = f.loss_grad(flat, T[idx], X[idx], 1.0 / bs, grad_out=grad)
                    opt.step(grad, 5.0)
                    tl += loss.double().sum()
        return flat.cpu().double().numpy(), float(tl.item()), opt.step_count

    fa, la, sa = run(False)
    fb, lb, sb = run(True)
    assert sa == sb == 2 * nb
    assert abs(la - lb) < 1e-3 * max(1.0, abs(la)), (la, lb)
    assert np.abs(fa - np.asarray(flat0, dtype=np.float64)).max() > 1e-3       # the parameters really moved
    assert np.abs(fa - fb).max() < 2e-4, np.abs(fa - fb).max()


def test_loss_grad_rows_equals_gathered_loss_grad():
    import ctypes as C
    from synference_amd import _lib
    from synference_amd.engine import HipFlow
    ospec, spec, flat0, theta, x = make_case("nsf_odd", B=300)
    dev = torch.device("cuda:0")
    f = HipFlow(spec, dev)
    flat = torch.as_tensor(flat0, dtype=torch.float32, device=dev)
    T = torch.as_tensor(theta, dtype=torch.float32, device=dev).contiguous()
    X = torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    rows = torch.tensor([5, 299, 0, 17, 17, 123] * 9 + [42], device=dev, dtype=torch.int64)   # duplicates, B = 55 (ragged)
    B = rows.numel()
    loss_ref, grad_ref = f.loss_grad(flat, T[rows], X[rows], 1.0 / B)
    grad_ref = grad_ref.clone()
    loss = torch.empty(B, device=dev); grad = torch.empty_like(flat)
    lsum = torch.zeros((), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().sf_flow_loss_grad_rows(f.handle, p(flat), p(T), p(X), p(rows), B, C.c_float(1.0 / B), None,
                                                  p(loss), p(lsum), p(grad), None, st))
    assert torch.allclose(loss, loss_ref, atol=1e-6)
    assert abs(float(lsum.item()) - float(loss_ref.double().sum().item())) < 1e-3
    assert (grad - grad_ref).abs().max().item() < 1e-5 * max(1.0, grad_ref.abs().max().item())


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3", "nsfar_cfg1", "mafar_cfg1"])
def test_training_losses_equal_the_density_kernel_at_a_full_chip_batch(name):
    """The per-row losses of the training kernel are -log_prob of another kernel: at 20 000 rows -- every CU holds workgroups of the
    training kernel side by side where its LDS and registers allow -- they must agree row by row.  (The lampe training kernel missed a
    barrier between the loss and the backward sweep: every small-batch gradient test passed, and with two workgroups per CU thousands of
    these rows were wrong: csrc/sf_nsfar.hip.)"""
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=20000)
    f = HipFlow(spec, "cuda:0")
    fl = torch.as_tensor(flat)
    f.set_params(fl.cuda())
    T, X = torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda()
    ref = -f.log_prob(T, X)
    for _ in range(2):
        loss, _g = f.loss_grad(fl, T, X, 1.0 / 20000)
        assert (loss - ref).abs().max().item() < 2e-4


def test_lampe_gradient_partials_and_atomics_agree(tmp_path):
    """sf_nsfar_loss_grad: every 64-row chunk stores its own gradient partial and k_ar_gather sums them in chunk order while the
    partials fit 512 MiB; f32 atomics into the one gradient beyond (or SF_AR_GRAD=atomic).  40 000 rows against the sum of the two
    halves, and against the atomic form of the same kernel in a child process."""
    import os, subprocess, sys
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case("nsfar_cfg1", B=40000)
    f = HipFlow(spec, "cuda:0")
    fl = torch.as_tensor(flat)
    T, X = torch.as_tensor(theta).cuda(), torch.as_tensor(x).cuda()
    la, ga = f.loss_grad(fl, T[:20000], X[:20000], 1.0 / 40000)
    la, ga = la.clone(), ga.clone()
    l2, g2 = f.loss_grad(fl, T[:20000], X[:20000], 1.0 / 40000)
    # no global atomics -- what is left of the hardware's order is the LDS adds of the hidden deltas inside a workgroup (four waves add
    # their dimensions' shares into the same rows): equal to rounding, and the losses bit for bit
    assert torch.equal(la, l2) and (ga - g2).abs().max().item() <= 2e-6 * ga.abs().max().item()
    lb, gb = f.loss_grad(fl, T[20000:], X[20000:], 1.0 / 40000)
    lb, gb = lb.clone(), gb.clone()
    lw, gw = f.loss_grad(fl, T, X, 1.0 / 40000)
    ref = (ga.double() + gb.double())
    assert (gw.double() - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    assert torch.equal(lw[:20000], la) and torch.equal(lw[20000:], lb)
    out = tmp_path / "atomic.npy"
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from cases import make_case; from synference_amd.engine import HipFlow\n"
            "ospec, spec, flat, theta, x = make_case('nsfar_cfg1', B=40000)\n"
            "f = HipFlow(spec, 'cuda:0'); l, g = f.loss_grad(torch.as_tensor(flat), theta, x, 1.0 / 40000)\n"
            "np.save(%r, g.cpu().numpy())\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), str(out))
    env = dict(os.environ, SF_AR_GRAD="atomic")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    g_at = np.load(out).astype(np.float64)
    assert np.abs(g_at - gw.cpu().double().numpy()).max() < 2e-5 * np.abs(g_at).max()


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3"])
def test_small_batch_gradients_are_bitwise_reproducible(name):
    """Up to 16 tiles (batch 512) every tile owns a gradient-image replica that the gather sums in tile order:
    the same inputs give the same bits, call after call (larger batches use f32 atomics unless SF_DETERMINISTIC=1)."""
    from synference_amd.engine import HipFlow
    ospec, spec, flat, theta, x = make_case(name, B=500)
    f = HipFlow(spec, "cuda:0")
    fl = torch.as_tensor(flat)
    l0, g0 = f.loss_grad(fl, theta, x, 1.0 / 500)
    g0 = g0.clone(); l0 = l0.clone()
    for _ in range(3):
        l1, g1 = f.loss_grad(fl, theta, x, 1.0 / 500)
        assert torch.equal(g0, g1) and torch.equal(l0, l1)
    # and they are right
    rloss, rgrad = oracle_loss_grad(ospec, flat, theta[:300], x[:300])
    _, g300 = f.loss_grad(fl, theta[:300], x[:300], 1.0 / 300)
    assert np.abs(g300.cpu().double().numpy() - rgrad).max() < 2e-4 * np.abs(rgrad).max()


@pytest.mark.parametrize("name", ["maf_cfg1", "nsf_cfg3", "nsfar_cfg1"])
def test_rccl_epoch_at_one_rank_is_the_plain_epoch(name):
    """SURVEY 8e / VERDICT r4 item 3: sf_flow_train_epoch_dp keeps the fused epoch loop under data parallelism -- prep -> flow
    -> gather -> ncclAllReduce (RCCL, on the library's stream) -> clip + Adam.  At nranks = 1 the exchange is the identity, so
    the parameters must equal the plain epoch's: bit for bit while the clip is inactive (the only other difference between
    the two calls is WHO sums |grad|^2 for the clip), to rounding with an active clip.  This is real RCCL on cuda:0: the
    communicator is created from a unique id, the all-reduce executes."""
    from synference_amd.comm import RcclComm, library_info
    from synference_amd.engine import HipFlow
    from synference_amd.runner import HipAdam, HipTrainOps
    info = library_info()
    assert "rccl" in info["path"] and info["version"] > 0
    ospec, spec, flat0, theta, x = make_case(name, B=900)
    dev = torch.device("cuda:0")
    T = torch.as_tensor(theta, dtype=torch.float32, device=dev)
    X = torch.as_tensor(x, dtype=torch.float32, device=dev)
    order = torch.randperm(900, generator=torch.Generator().manual_seed(3)).to(dev)
    comm = RcclComm.create(dev, 1, 0)
    assert (comm.nranks, comm.rank) == (1, 0)
    v = torch.arange(1000, dtype=torch.float32, device=dev)
    assert torch.equal(comm.all_reduce_(v.clone()), v)

    def run(with_comm, max_norm):
        f = HipFlow(spec, dev)
        flat = torch.as_tensor(flat0, dtype=torch.float32, device=dev).clone()
        opt = HipAdam(flat, lr=3e-3)
        grad = torch.empty_like(flat)
        tl = torch.zeros((), dtype=torch.float64, device=dev)

        class E:
            flow = f
        ops = HipTrainOps(E)
        for ep in range(2):
            ops.train_epoch(flat, T, X, order, 9, 96, 1.0 / 96, opt, max_norm, grad, tl, comm=(comm if with_comm else None))
        torch.cuda.synchronize()
        return flat.cpu(), float(tl.item()), opt.step_count, float(opt.scratch[1].item())

    a, b = run(False, 1e9), run(True, 1e9)
    assert a[2] == b[2] == 18
    # (the lampe flows' hidden deltas are summed with LDS float adds in the hardware's order: gradients agree to rounding call to call,
    #  and 18 Adam steps turn a rounding-level difference of a near-zero gradient into up to a few 1e-4 of a parameter -- 4.5e-4 seen
    #  under the schedule-fuzz build, scripts/fuzz_sched.sh, a few 1e-6 on the product build)
    tol = 2e-3 if name == "nsfar_cfg1" else 1e-4
    if name != "nsfar_cfg1":
        assert torch.equal(a[0], b[0]) and a[1] == b[1]
    else:
        assert (a[0] - b[0]).abs().max().item() < tol and abs(a[1] - b[1]) < 1e-5 * abs(a[1])
    c, d = run(False, 0.5), run(True, 0.5)            # the clip bites (|grad| of a random-init flow is far above 0.5)
    assert c[3] > 0.5 and abs(c[3] - d[3]) < 1e-4 * c[3]
    # (18 Adam steps at lr 3e-3 turn a last-bit difference of the clip factor into ~1e-5 on a few parameters)
    assert (c[0] - d[0]).abs().max().item() < tol
    comm.close()
