"""Gradient-norm clipping and weight EMA inside the fused AdamW step (FlatTrainer(max_grad_norm=..., ema_decay=...)): the
sum-of-squares kernel against fp64, the clipped step against torch clip_grad_norm_ + torch.optim.AdamW, bitwise identity when
the clip does not bind, the EMA against its fp64 recurrence and through ema_weights() / ema_state_dict(), clipping once under
no_sync() accumulation, checkpoints, and a captured step with both features replayed against eager steps."""
import math
import os
import subprocess
import sys
import textwrap

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def M():
    import image_restoration_amd as m
    return m


def _restormer_base_flat_total():
    from image_restoration_amd.configs import RESTORMER_BASE
    from image_restoration_amd.trainer import ALIGN
    net = M().Restormer(**RESTORMER_BASE)
    return sum((p.numel() + ALIGN - 1) // ALIGN * ALIGN for p in net.parameters() if p.requires_grad)


def _tiny(seed=3):
    from image_restoration_amd.configs import RESTORMER_TINY
    torch.manual_seed(seed)
    return M().Restormer(**RESTORMER_TINY).to(DEV)


def _batch(seed, dtype=torch.float32, b=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((b, 3, 64, 64), generator=g)
    y = torch.rand((b, 3, 64, 64), generator=g)
    return x.to(DEV).to(dtype), y.to(DEV).to(dtype)


def _loss(net, x, y):
    return (net(x).float() - y.float()).abs().mean()


# ----------------------------------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("n", [1, 3, 4, 1023, (1 << 20) + 5, "restormer_base"])
def test_grad_sumsq_matches_fp64_and_is_reproducible(n):
    from image_restoration_amd import ops
    if n == "restormer_base":
        n = _restormer_base_flat_total()
        assert 26_000_000 < n < 26_300_000
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000)).to(DEV)
    ref = float(x.double().square().sum())
    a = ops.grad_sumsq(x)
    b = ops.grad_sumsq(x)
    assert a.shape == (1,) and a.dtype == torch.float32
    assert torch.equal(a, b), "two calls differ"
    assert abs(float(a) - ref) <= 1e-6 * ref, (float(a), ref)
    assert math.sqrt(float(a)) == pytest.approx(math.sqrt(ref), rel=1e-6)


def test_grad_sumsq_zero_inf_nan():
    from image_restoration_amd import ops
    z = torch.zeros(4099, device=DEV)
    assert float(ops.grad_sumsq(z)) == 0.0
    for pos in (0, 4098):                               # in the f32x4 body and in the n % 4 tail
        t = z.clone()
        t[pos] = float("inf")
        assert math.isinf(float(ops.grad_sumsq(t)))
        t[pos] = float("nan")
        assert math.isnan(float(ops.grad_sumsq(t)))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.grad_sumsq(torch.zeros(8))


def _adamw_ex_fp64(p, g, m, v, ema, lr, step, b1, b2, eps, wd, gscale, max_norm, decay):
    """fp64 restatement of the fused step: torch clip_grad_norm_ (error_if_nonfinite=False) then AdamW then BasicSR's EMA.  The
    hyper-parameters are the fp32 values the kernel receives (1 - fp32(0.999) differs from 0.001 by 5e-5 relative)."""
    p, g, m, v, ema = (t.double().cpu() for t in (p, g, m, v, ema))
    lr, b1, b2, eps, wd, gscale, decay = (float(torch.tensor(x, dtype=torch.float32)) for x in (lr, b1, b2, eps, wd, gscale, decay))
    g = g * gscale
    norm = float(g.square().sum().sqrt())
    coef = min(max_norm / (norm + 1e-6), 1.0)
    g = g * coef
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** step) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    ema = ema * decay + p * (1 - decay)
    return p, m, v, ema, norm


@pytest.mark.parametrize("n,max_norm", [(1023, 0.5), ((1 << 16) + 3, 1e9)])
def test_adamw_step_ex_against_fp64(n, max_norm):
    from image_restoration_amd import ops
    gen = torch.Generator().manual_seed(n)
    p, g, ema = (torch.randn(n, generator=gen) for _ in range(3))
    m = torch.randn(n, generator=gen) * 0.01
    v = torch.rand(n, generator=gen) * 1e-4
    args = dict(lr=1e-3, step=3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, gscale=0.5, max_norm=max_norm, decay=0.99)
    want = _adamw_ex_fp64(p, g, m, v, ema, **args)
    P, G, Mm, V, E = (t.to(DEV) for t in (p, g, m, v, ema))
    ws = ops.grad_sumsq_workspace(n, DEV)
    ss = ops.grad_sumsq(G, workspace=ws)
    norm = torch.zeros((), device=DEV)
    ops.adamw_step_ex(P, G, Mm, V, 1e-3, 3, (0.9, 0.999), 1e-8, 1e-2, 0.5, None, sumsq=ss, max_norm=max_norm, norm_out=norm,
                      ema=E, ema_decay=0.99)
    for got, w in zip((P, Mm, V, E), want[:4]):
        err = float((got.double().cpu() - w).abs().max() / w.abs().max())
        assert err < 2e-6, err
    assert float(norm) == pytest.approx(want[4], rel=1e-6)


def test_adamw_step_ex_nonfinite_norm_propagates_like_torch():
    """An inf gradient: norm inf, coefficient 0, inf * 0 = NaN in the update (torch clip_grad_norm_ does the same)."""
    from image_restoration_amd import ops
    n = 64
    p, m, v = torch.ones(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    g = torch.full((n,), 0.1, device=DEV)
    g[5] = float("inf")
    norm = torch.zeros((), device=DEV)
    ops.adamw_step_ex(p, g, m, v, 1e-3, 1, sumsq=ops.grad_sumsq(g), max_norm=1.0, norm_out=norm)
    assert math.isinf(float(norm)) and torch.isnan(p[5]) and torch.isfinite(p[:5]).all()
    # torch's own answer for the same gradient
    t = torch.nn.Parameter(torch.ones(n))
    t.grad = g.cpu()
    assert math.isinf(float(torch.nn.utils.clip_grad_norm_([t], 1.0)))
    assert torch.isnan(t.grad[5]) and torch.equal(t.grad[:5], torch.zeros(5))


# ----------------------------------------------------------------------------------------------------------- 2. clipped step
def test_clipped_step_matches_torch_clip_and_adamw():
    from image_restoration_amd.trainer import FlatTrainer
    net = _tiny()
    lr = 1e-3
    tr = FlatTrainer(net, lr=lr, max_grad_norm=0.01)
    try:
        ref_p = torch.nn.Parameter(tr.flat_p.detach().cpu().clone())
        opt = torch.optim.AdamW([ref_p], lr=lr, betas=tr.betas, eps=tr.eps, weight_decay=tr.wd)
        for step in range(3):
            x, y = _batch(100 + step)
            tr.zero_grad()
            _loss(net, x, y).backward()
            tr.reduce_gradients()
            g = tr.flat_g.clone()
            tr.optimizer_step()
            ref_p.grad = g.cpu()
            norm = torch.nn.utils.clip_grad_norm_([ref_p], 0.01)
            opt.step()
            assert float(norm) > 0.01, "the clip must bind for this test to mean anything"
            assert float(tr.grad_norm) == pytest.approx(float(g.double().norm()), rel=2e-6)
            # torch's fp32 CPU norm sums in fp32: 1.6e-5 relative off the fp64 norm at this size
            assert float(tr.grad_norm) == pytest.approx(float(norm), rel=1e-4)
            assert tr.grad_norm.is_cuda and tr.grad_norm.dim() == 0
            dp = (tr.flat_p.cpu() - ref_p.detach()).abs().max()
            assert float(dp) <= 1e-3 * lr, (step, float(dp))
            m_ref = opt.state[ref_p]["exp_avg"]        # scales with the clip coefficient: a missing clip shows here
            assert float((tr.flat_m.cpu() - m_ref).abs().max() / m_ref.abs().max()) < 1e-4
    finally:
        tr.close()


# ----------------------------------------------------------------------------------------------------------- 3. non-binding
def test_non_binding_clip_is_bitwise_the_default_step():
    from image_restoration_amd.trainer import FlatTrainer

    def run(**kw):
        net = _tiny()
        tr = FlatTrainer(net, lr=1e-3, **kw)
        try:
            for step in range(3):
                x, y = _batch(200 + step, torch.bfloat16)
                tr.zero_grad()
                _loss(net, x, y).backward()
                tr.optimizer_step()
            return tr.flat_p.clone(), tr.flat_m.clone(), tr.flat_v.clone(), float(tr.grad_norm)
        finally:
            tr.close()
    p1, m1, v1, n1 = run(max_grad_norm=1e9)
    p0, m0, v0, _ = run()
    assert 0 < n1 < 1e9
    assert torch.equal(p1, p0) and torch.equal(m1, m0) and torch.equal(v1, v0)


# ----------------------------------------------------------------------------------------------------------- 4. EMA
def test_ema_recurrence_state_dict_and_swap():
    from image_restoration_amd.configs import RESTORMER_TINY
    from image_restoration_amd.trainer import FlatTrainer
    decay = 0.9
    net = _tiny()
    tr = FlatTrainer(net, lr=1e-3, ema_decay=decay)
    try:
        ema = tr.flat_p.double().cpu()
        assert torch.equal(tr.flat_ema, tr.flat_p)
        for step in range(4):
            x, y = _batch(300 + step, torch.bfloat16)
            tr.zero_grad()
            _loss(net, x, y).backward()
            tr.optimizer_step()
            ema = ema * decay + tr.flat_p.double().cpu() * (1 - decay)
            err = float((tr.flat_ema.double().cpu() - ema).abs().max() / ema.abs().max())
            assert err < 1e-6, (step, err)
        sd = tr.ema_state_dict()
        assert list(sd) == list(net.state_dict())
        x, _ = _batch(399, torch.bfloat16)
        net.eval()
        with torch.no_grad():
            y_pre = net(x).float()
            with tr.ema_weights():
                y_ema = net(x).float()
                with pytest.raises(RuntimeError, match="ema_weights"):
                    tr.optimizer_step()
            y_post = net(x).float()
            twin = M().Restormer(**RESTORMER_TINY).to(DEV)
            twin.load_state_dict(sd)
            twin.eval()
            y_twin = twin(x).float()
        assert not torch.equal(y_ema, y_pre), "the EMA did not differ from the weights"
        assert torch.equal(y_ema, y_twin), float((y_ema - y_twin).abs().max())
        assert torch.equal(y_post, y_pre), float((y_post - y_pre).abs().max())
    finally:
        tr.close()


# ----------------------------------------------------------------------------------------------------------- 5. accumulation
def test_clip_runs_once_on_the_accumulated_gradient():
    from image_restoration_amd.trainer import FlatTrainer
    net = _tiny()
    tr = FlatTrainer(net, lr=1e-3, max_grad_norm=0.01)
    try:
        (x1, y1), (x2, y2) = _batch(500, torch.bfloat16), _batch(501, torch.bfloat16)
        tr.zero_grad()
        with tr.no_sync():
            _loss(net, x1, y1).backward()
        tr.grads_ready()
        g1 = tr.flat_g.clone()
        _loss(net, x2, y2).backward()
        tr.reduce_gradients()
        g = tr.flat_g.clone()
        tr.optimizer_step()
        norm = float(g.double().norm())
        assert float(tr.grad_norm) == pytest.approx(norm, rel=1e-5)
        assert abs(float(g1.double().norm()) - norm) > 1e-3 * norm       # the norm of one micro-batch alone differs
        coef = 0.01 / (norm + 1e-6)
        m_ref = 0.1 * coef * g.double()                                   # first step: exp_avg = (1 - beta1) * clipped grad
        assert float((tr.flat_m.double() - m_ref).abs().max() / m_ref.abs().max()) < 1e-5
    finally:
        tr.close()


# ----------------------------------------------------------------------------------------------------------- 6. checkpoints
def test_checkpoint_round_trip_with_ema():
    from image_restoration_amd.trainer import FlatTrainer
    net = _tiny()
    tr = FlatTrainer(net, lr=1e-3, ema_decay=0.99, max_grad_norm=0.05)
    try:
        for step in range(2):
            x, y = _batch(600 + step, torch.bfloat16)
            tr.zero_grad()
            _loss(net, x, y).backward()
            tr.optimizer_step()
        sd, msd = tr.state_dict(), {k: v.clone() for k, v in net.state_dict().items()}
        ema = tr.flat_ema.clone()
    finally:
        tr.close()
    assert sd["ema_decay"] == 0.99 and sd["max_grad_norm"] == 0.05 and torch.equal(sd["ema"], ema)
    net2 = _tiny(seed=11)
    tr2 = FlatTrainer(net2, lr=1e-3, ema_decay=0.5, max_grad_norm=1.0)
    try:
        net2.load_state_dict(msd)
        tr2.load_state_dict(sd)
        assert torch.equal(tr2.flat_ema, ema) and tr2.ema_decay == 0.99 and tr2.max_grad_norm == 0.05 and tr2.step_count == 2
        old = dict(sd)
        for k in ("ema", "ema_decay", "max_grad_norm"):
            old.pop(k)
        tr2.load_state_dict(old)                        # an older state without EMA: the average restarts at the weights
        assert torch.equal(tr2.flat_ema, tr2.flat_p)
    finally:
        tr2.close()
    net3 = _tiny()
    tr3 = FlatTrainer(net3, lr=1e-3)
    try:
        assert not {"ema", "ema_decay", "max_grad_norm"} & set(tr3.state_dict())
        with pytest.raises(ValueError, match="EMA"):
            tr3.load_state_dict(sd)
    finally:
        tr3.close()


# ----------------------------------------------------------------------------------------------------------- 7. capture
CHILD = textwrap.dedent(r'''
    import os, sys, torch
    sys.path.insert(0, os.getcwd())
    import image_restoration_amd as m
    from image_restoration_amd import configs
    from image_restoration_amd.trainer import FlatTrainer
    torch.manual_seed(0)
    net = m.Restormer(**configs.RESTORMER_TINY).to("cuda")
    x = torch.rand(2, 3, 64, 64, device="cuda").to(torch.bfloat16)
    y = torch.rand(2, 3, 64, 64, device="cuda").to(torch.bfloat16)
    lr = 1e-4
    tr = FlatTrainer(net, lr=lr, max_grad_norm=0.01, ema_decay=0.9)
    def step():
        tr.zero_grad()
        loss = (net(x).float() - y.float()).abs().mean()
        loss.backward()
        tr.reduce_gradients()
        tr.optimizer_step(use_dev_scalars=True)
    graph = tr.capture_step(step, warmup=2)
    assert tr.step_count == 2, tr.step_count             # the two warm-up steps ran; the captured one did not
    snap = [t.clone() for t in (tr.flat_p, tr.flat_m, tr.flat_v, tr.flat_ema)]
    n0 = tr.step_count
    for _ in range(3):
        tr.replay_step(graph)
    torch.cuda.synchronize()
    rep = dict(p=tr.flat_p.clone(), ema=tr.flat_ema.clone(), norm=float(tr.grad_norm), step=tr.step_count)
    assert float((rep["p"] - snap[0]).abs().max()) > 0, "replays did not update the parameters"
    for dst, src in zip((tr.flat_p, tr.flat_m, tr.flat_v, tr.flat_ema), snap):
        dst.copy_(src)
    tr.step_count = n0
    tr.weights_changed()
    for _ in range(3):
        tr.set_step_scalars(tr.step_count + 1)
        step()
    torch.cuda.synchronize()
    assert rep["step"] == tr.step_count == n0 + 3, (rep["step"], tr.step_count)
    dp = float((rep["p"] - tr.flat_p).abs().max())
    de = float((rep["ema"] - tr.flat_ema).abs().max())
    assert dp <= 1e-3 * lr and de <= 1e-3 * lr, (dp, de)
    assert abs(rep["norm"] - float(tr.grad_norm)) <= 1e-5 * float(tr.grad_norm), (rep["norm"], float(tr.grad_norm))
    assert rep["norm"] > 0.01
    print("CAPTURE_CLIP_EMA_OK", dp, de, rep["norm"])
''')


def test_captured_step_with_clip_and_ema_replays_like_eager_steps(tmp_path):
    """Three replays of a captured Restormer-tiny step with clipping and EMA equal three eager steps from the same state (flat
    parameters, EMA, step_count, grad_norm).  Before the step_count fix in capture_step every replay used the next step's bias
    corrections.  A fresh child process, as the other capture tests (a failed capture takes the process down); the deferred
    sums are off so that eager and captured steps launch the same reductions."""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ)
    env["MI_DEFER_MB"] = "0"
    res = subprocess.run([sys.executable, str(script)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert res.returncode == 0 and "CAPTURE_CLIP_EMA_OK" in res.stdout, res.stdout[-3000:]
