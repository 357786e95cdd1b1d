"""DRSformer's MEFC (``subnet``) and whole network on the MI355X: the native modules against the reference fixtures and against
the fp64 restatement (tests/drs_net_ref.py) fed the device's own ReLU decisions (and, for the network, the STBs' top-k masks),
determinism, no_grad, accumulation, refusals, FlatTrainer training (eager and captured) and DRSformer base at 256^2."""
import importlib.util
import os
import subprocess
import sys
import textwrap

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import drs_net_ref as R  # noqa: E402
import drs_ref as D  # noqa: E402
from oracle.fixtures import load, seeded_input  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {torch.float32: 5e-5, torch.bfloat16: 3e-2}      # the bars of tests/test_gpu_drsformer.py


def N():
    from image_restoration_amd import drsformer
    return drsformer


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_drs_net", os.path.join(ROOT, "tools", "capture_golden_drs_net.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build_subnet(dim, layer_num, steps, seed):
    sd = D.make_state(R.subnet_shapes(dim, layer_num, steps), seed)
    mod = N().subnet(dim, layer_num, steps)
    mod.load_state_dict(sd)
    return mod.to(DEV), sd


def _cpu_masks(masks):
    return [{k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in m.items()} for m in masks]


def run_native(mod, x, cot, dtype):
    mod.zero_grad(set_to_none=True)
    mod.record_masks = True
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    y = mod(xg)
    y.backward(cot.to(DEV).to(dtype))
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
    return y.detach(), xg.grad.detach(), grads, _cpu_masks(mod.relu_masks)


def run_oracle(sd, x, cot, layer_num, steps, masks):
    ps = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    y, ws = R.subnet(xr, ps, layer_num, steps, masks)
    y.backward(cot.double())
    return y.detach(), xr.grad, {k: v.grad for k, v in ps.items()}, [w.detach() for w in ws]


def _parity(dim, layer_num, steps, bhw, dtype, seed):
    mod, sd = build_subnet(dim, layer_num, steps, seed)
    B, H, W = bhw
    x, cot = seeded_input((B, dim, H, W), 3000 + seed), seeded_input((B, dim, H, W), 4000 + seed)
    if dtype == torch.bfloat16:           # the oracle sees the same (rounded) input and cotangent
        x, cot = x.to(dtype).float(), cot.to(dtype).float()
    y, dx, grads, masks = run_native(mod, x, cot, dtype)
    yr, dxr, gr, wr = run_oracle(sd, x, cot, layer_num, steps, masks)
    errs = {"y": rel(y, yr), "dx": rel(dx, dxr)}
    errs.update({f"w{i}": rel(m["w"], wr[i]) for i, m in enumerate(masks)})
    errs.update({"g_" + k: rel(g, gr[k]) for k, g in grads.items()})
    worst = max(errs, key=errs.get)
    print(f"PARITY mefc C{dim} L{layer_num} S{steps} {bhw} {dtype}: max-rel {worst} {errs[worst]:.2e}; y {errs['y']:.2e} "
          f"dx {errs['dx']:.2e} w {max(v for k, v in errs.items() if k[0] == 'w'):.2e}")
    assert errs[worst] < TOL[dtype], (worst, errs[worst], {k: v for k, v in errs.items() if v >= TOL[dtype]})
    return errs


# (dim, layer_num, steps, (B, H, W)); tiles are 32 x 32, a 6-pixel halo
PARITY = [
    (48, 1, 4, (2, 40, 70)),      # tiles_x 3 (last 6 wide) x 2 rows (last 8 tall)
    (96, 1, 4, (2, 33, 97)),      # tiles_x 4 (last 1 wide) x 2 rows (last 1 tall)
    (48, 1, 4, (1, 70, 200)),     # 7 x 3 = 21 tiles: the weight-gradient splits (16) walk two tiles or one
    (48, 1, 4, (2, 1, 1)),        # one pixel: every tap but the centre falls outside
    (96, 1, 4, (3, 5, 9)),        # B = 3 on a plane smaller than the 13 x 13 dilated footprint
    (48, 2, 2, (2, 12, 20)),      # two layer pairs of two steps
    (96, 2, 2, (2, 7, 9)),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", PARITY, ids=[f"C{c[0]}_L{c[1]}S{c[2]}_B{c[3][0]}_{c[3][1]}x{c[3][2]}" for c in PARITY])
def test_mefc_parity_with_device_masks(case, dtype):
    dim, layer_num, steps, bhw = case
    _parity(dim, layer_num, steps, bhw, dtype, seed=dim + 10 * layer_num + bhw[1] + bhw[2])


@pytest.mark.parametrize("name", ["drs_net_mefc_c16", "drs_net_mefc_c12_l2s2"])
def test_native_subnet_matches_reference_fixtures(name):
    """fp32 against the fixtures captured from the reference (its own fp64 ReLU decisions)."""
    kind, dim, layer_num, steps, bhw, seed = G.CASES[name]
    mod, _ = build_subnet(dim, layer_num, steps, seed)
    x, cot = G.case_io(kind, dim, bhw, seed)
    y, dx, grads, masks = run_native(mod, x, cot, torch.float32)
    gold = load(name)
    R.check_packed("y", y, gold, 1e-4, what=name + " ")
    R.check_packed("dx", dx, gold, 1e-4, what=name + " ")
    for i, m in enumerate(masks):
        R.check_packed(f"w{i}", m["w"], gold, 1e-4, what=name + " ")
    R.check_grads(grads, gold, 1e-4, what=name + " ")


# ---------------------------------------------------------------- the whole network
def build_net(cfg, seed):
    sd = D.make_state(R.drsformer_shapes(cfg), seed)
    net = N().DRSformer(**cfg)
    net.load_state_dict(sd)
    return net.to(DEV), sd


def _record(net, on=True):
    for m in net.modules():
        if isinstance(m, N().TransformerBlock):
            m.attn.record_scores = on
            m.ffn.record_masks = on
        elif isinstance(m, N().subnet):
            m.record_masks = on


def _net_masks(net):
    stb, mefc = {}, {}
    for name, m in net.named_modules():
        if isinstance(m, N().TransformerBlock):
            stb[name] = (D.topk_masks(m.attn.scores.cpu().double()), [t.cpu() for t in m.ffn.relu_masks])
        elif isinstance(m, N().subnet):
            mefc[name] = _cpu_masks(m.relu_masks)
    return stb, mefc


def _group_scalars(grads, dtype):
    """The STBs' one-element parameters are compared as groups, as in tests/test_gpu_drsformer.py: each block's four mixing weights
    attn1..4 as one tensor [4], and in bf16 every block's per-head temperatures as one vector.  Each is a sum of signed terms over
    every (image, head, row, column) and can cancel to near 0; in bf16 the input of a deep block already differs from the fp64
    path by ~1e-2, so a cancelled temperature gradient alone has no relative precision to hold."""
    for blk in sorted({k.rsplit(".attn.", 1)[0] for k in grads if ".attn.attn1" in k}):
        keys = [f"{blk}.attn.attn{m}" for m in range(1, 5)]
        grads[blk + ".attn.attn1..4"] = torch.cat([grads.pop(k).reshape(-1) for k in keys])
    if dtype == torch.bfloat16:
        keys = sorted(k for k in grads if k.endswith(".attn.temperature"))
        grads["*.attn.temperature"] = torch.cat([grads.pop(k).reshape(-1) for k in keys])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_tiny_network_parity_with_device_masks(dtype):
    from image_restoration_amd import configs
    cfg = configs.DRSFORMER_TINY
    net, sd = build_net(cfg, 201)
    x, cot = seeded_input((2, 3, 32, 48), 201), seeded_input((2, 3, 32, 48), 202)
    if dtype == torch.bfloat16:
        x, cot = x.to(dtype).float(), cot.to(dtype).float()
    _record(net)
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    y = net(xg)
    y.backward(cot.to(DEV).to(dtype))
    torch.cuda.synchronize()
    stb, mefc = _net_masks(net)
    ps = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    yr = R.drsformer(xr, ps, cfg, stb, mefc)
    yr.backward(cot.double())
    got = {k: p.grad for k, p in net.named_parameters()}
    ref = {k: ps[k].grad for k in got}
    _group_scalars(got, dtype)
    _group_scalars(ref, dtype)
    errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad)}
    errs.update({"g_" + k: rel(g, ref[k]) for k, g in got.items()})
    nerrs = {"g_" + k: nrel(g, ref[k]) for k, g in got.items()}
    top = sorted(errs, key=errs.get, reverse=True)[:4]
    ntop = sorted(nerrs, key=nerrs.get, reverse=True)[:4]
    mefc = {k: v for k, v in errs.items() if k.startswith(("g_encoder_level0.", "g_refinement."))}
    mw = max(mefc, key=mefc.get)
    print(f"PARITY DRSformer-tiny {dtype}: y {errs['y']:.2e} dx {errs['dx']:.2e}; max-rel " +
          ", ".join(f"{k} {errs[k]:.2e}" for k in top) + f"; MEFC max-rel {mw} {mefc[mw]:.2e}; norm-rel " +
          ", ".join(f"{k} {nerrs[k]:.2e}" for k in ntop))
    assert errs["y"] < TOL[dtype] and errs["dx"] < TOL[dtype], (errs["y"], errs["dx"])
    assert mefc[mw] < TOL[dtype], (mw, mefc[mw])
    if dtype == torch.float32:
        assert errs[top[0]] < TOL[dtype], (top[0], errs[top[0]])
    else:
        # bf16 through the whole U-Net: the STBs of the deep levels (8 x 12 and 4 x 6 planes here) see inputs that already differ
        # from the fp64 path by ~1e-2, and their weight gradients are sums over a few hundred pixels with cancellation (0.12 of
        # the norm at worst, in encoder_level3 / decoder_level3; fp32 holds 2e-5).  The network's gradients are held as vectors
        # at the whole-network bar of test_gpu_configs.py (Restormer base, bf16: every gradient norm 1.5e-1); the MEFC's own
        # gradients and the output and input gradient keep the per-module bar above.
        assert nerrs[ntop[0]] < 1.5e-1, (ntop[0], nerrs[ntop[0]])
    with torch.no_grad():                     # the no_grad forward gives the training forward's output
        y0 = net(x.to(DEV).to(dtype))
    assert torch.equal(y0, y.detach())


def test_tiny_network_matches_reference_fixture():
    from image_restoration_amd import configs
    kind, dim, layer_num, steps, bhw, seed = G.CASES["drs_net_tiny"]
    net, _ = build_net(configs.DRSFORMER_TINY, seed)
    x, cot = G.case_io(kind, dim, bhw, seed)
    xg = x.to(DEV).requires_grad_(True)
    y = net(xg)
    y.backward(cot.to(DEV))
    gold = load("drs_net_tiny")
    R.check_packed("y", y, gold, 1e-4, what="tiny ")
    R.check_packed("dx", xg.grad, gold, 1e-4, what="tiny ")
    R.check_grads({k: p.grad for k, p in net.named_parameters()}, gold, 1e-4, what="tiny ")


# ---------------------------------------------------------------- determinism and behaviour
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_is_bitwise_reproducible(dtype):
    mod, _ = build_subnet(48, 1, 4, 301)
    x, cot = seeded_input((2, 48, 40, 70), 301), seeded_input((2, 48, 40, 70), 302)
    y1, dx1, g1, _ = run_native(mod, x, cot, dtype)
    y2, dx2, g2, _ = run_native(mod, x, cot, dtype)
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_no_grad_output_equals_grad_mode_output(dtype):
    mod, _ = build_subnet(96, 2, 2, 311)
    x = seeded_input((3, 96, 33, 40), 311).to(DEV).to(dtype)
    with torch.no_grad():
        y0 = mod(x)
    y1 = mod(x.clone().requires_grad_(True))
    assert torch.equal(y0, y1.detach())


def test_ops_backward_accumulates_onto_existing_gradients():
    """accumulate=True adds onto what the gradient buffers hold: G0 + g_a + g_b after two calls."""
    from image_restoration_amd import ops
    mod, _ = build_subnet(48, 1, 4, 321)
    params = mod.pair_params(0)
    x = seeded_input((3, 48, 37, 40), 321).to(DEV)
    ca, cb = seeded_input((3, 48, 37, 40), 322).to(DEV), seeded_input((3, 48, 37, 40), 323).to(DEV)
    out, saved = ops.mefc_fwd(x, params, 4, True)
    ga, gb = ([torch.empty_like(p) for p in params] for _ in range(2))
    dxa = ops.mefc_bwd(x, out, ca, params, 4, saved, ga, False)
    dxb = ops.mefc_bwd(x, out, cb, params, 4, saved, gb, False)
    g = torch.Generator().manual_seed(324)
    g0 = [(torch.randn(p.shape, generator=g) * float(a.abs().max())).to(DEV) for p, a in zip(params, ga)]
    acc = [t.clone() for t in g0]
    dxa2 = ops.mefc_bwd(x, out, ca, params, 4, saved, acc, True)
    dxb2 = ops.mefc_bwd(x, out, cb, params, 4, saved, acc, True)
    torch.cuda.synchronize()
    assert torch.equal(dxa, dxa2) and torch.equal(dxb, dxb2)
    for i, t in enumerate(acc):
        ref = g0[i].double() + ga[i].double() + gb[i].double()
        assert rel(t, ref) <= 1e-6, (i, rel(t, ref))
        assert rel(g0[i], ref) > 1e-3, i


def test_cpu_tensors_are_refused():
    mod, _ = build_subnet(48, 1, 4, 331)
    with pytest.raises(RuntimeError, match="MI355X only"):
        mod(torch.zeros(1, 48, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        N().subnet(48)(torch.zeros(1, 48, 8, 8, device=DEV))          # CPU parameters


def test_unsupported_shapes_fail_the_library_check():
    for dim, steps in ((260, 1), (16, 17)):
        mod = N().subnet(dim, 1, steps).to(DEV)
        with pytest.raises(RuntimeError, match="mefc"):
            mod(torch.zeros(1, dim, 8, 8, device=DEV))
    with pytest.raises(TypeError):
        N().subnet(16).to(DEV)(torch.zeros(1, 16, 8, 8, device=DEV, dtype=torch.float16))


# ---------------------------------------------------------------- training
def test_training_steps_follow_the_oracle_trajectory():
    """Three FlatTrainer steps (main_grad accumulation, fused AdamW) of the tiny network against the fp64 oracle plus
    torch.optim.AdamW, fp32.  The oracle uses each step's device top-k and ReLU decisions."""
    from image_restoration_amd import configs
    from image_restoration_amd.trainer import FlatTrainer
    cfg = configs.DRSFORMER_TINY
    net, sd0 = build_net(cfg, 401)
    x, tgt = seeded_input((2, 3, 32, 32), 401), seeded_input((2, 3, 32, 32), 402)
    lr = 1e-3
    net = net.train()
    _record(net)
    tr = FlatTrainer(net, lr=lr, weight_decay=0.01)
    losses, masks = [], []
    try:
        xd, td = x.to(DEV), tgt.to(DEV)
        for _ in range(3):
            tr.zero_grad()
            loss = (net(xd) - td).abs().mean()
            masks.append(_net_masks(net))
            loss.backward()
            tr.reduce_gradients()
            tr.optimizer_step()
            losses.append(float(loss.detach()))
        got = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    finally:
        tr.close()
    ps = {k: v.double().clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.AdamW(list(ps.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    for step in range(3):
        opt.zero_grad()
        loss = (R.drsformer(x.double(), ps, cfg, *masks[step]) - tgt.double()).abs().mean()
        loss.backward()
        opt.step()
        lr_ = float(loss.detach())
        assert abs(losses[step] - lr_) < 1e-4 * lr_, (step, losses[step], lr_)
    for k, v in ps.items():
        w0 = sd0[k].double()
        a, r = got[k].double(), v.detach()
        d = (a - r).abs()
        ua, ur = (a - w0).flatten(), (r - w0).flatten()
        if float(ur.norm()) == 0.0:
            assert float(ua.norm()) == 0.0, k
            continue
        cos = float((ua @ ur) / (ua.norm() * ur.norm()).clamp_min(1e-30))
        assert cos >= 0.9995, (k, cos)
        # (Adam's first steps move an element by about lr sign(g): where a gradient element sits near 0 the two sides may step
        #  opposite ways, 2 lr apart per step, so single elements are bounded by 6 lr over three steps; the mean holds them)
        assert float(d.mean()) <= 0.02 * lr and float(d.max()) <= 6.0 * lr, (k, float(d.mean()) / lr, float(d.max()) / lr)


CHILD = textwrap.dedent(r'''
    import os, sys, torch
    sys.path.insert(0, os.getcwd())
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import drs_net_ref as R, drs_ref as D
    from image_restoration_amd import configs
    from image_restoration_amd import drsformer as N
    from image_restoration_amd.trainer import FlatTrainer
    dev = "cuda"
    cfg = configs.DRSFORMER_TINY
    sd = D.make_state(R.drsformer_shapes(cfg), 91)
    g = torch.Generator().manual_seed(91)
    x = torch.randn(2, 3, 32, 32, generator=g).to(dev).to(torch.bfloat16)
    t = torch.randn(2, 3, 32, 32, generator=g).to(dev).to(torch.bfloat16)

    def make():
        net = N.DRSformer(**cfg)
        net.load_state_dict(sd)
        net = net.to(dev).train()
        tr = FlatTrainer(net, lr=1e-3)
        losses = []
        def step():
            tr.zero_grad()
            loss = (net(x).float() - t.float()).abs().mean()
            loss.backward()
            tr.reduce_gradients()
            tr.optimizer_step(use_dev_scalars=True)
            losses.append(loss.detach())
        return tr, step, losses

    tr_e, step_e, loss_e = make()
    for _ in range(5):
        tr_e.set_step_scalars(tr_e.step_count + 1)
        step_e()
    torch.cuda.synchronize()
    tr_c, step_c, loss_c = make()
    graph = tr_c.capture_step(step_c, warmup=2)
    for _ in range(3):
        tr_c.replay_step(graph)
    torch.cuda.synchronize()
    pe, pc = tr_e.flat_p.float(), tr_c.flat_p.float()
    err = float((pe - pc).abs().max() / pe.abs().max())
    le = [float(v) for v in loss_e]
    lc = [float(v) for v in loss_c]
    print("losses", le, lc[:2] + [float(lc[2])], "param err", err)
    assert torch.isfinite(pc).all() and err < 1e-5, err
    assert all(abs(a - b) <= 1e-5 * abs(a) for a, b in zip(le[:2], lc[:2])), (le, lc)
    tr_e.close(); tr_c.close()
    print("CAPTURE_OK")
''')


def test_captured_training_step_replays_equal_to_eager_steps(tmp_path):
    """The tiny network, bf16 activations: 2 warm-up steps + a captured step replayed 3 times against 5 eager steps from the same
    weights, in a fresh child process with a timeout (a failed capture takes its process down)."""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ)
    env.pop("MI_DEFER_MB", None)
    res = subprocess.run([sys.executable, str(script)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert res.returncode == 0 and "CAPTURE_OK" in res.stdout, res.stdout[-3000:]


# ---------------------------------------------------------------- full size
def test_drsformer_base_at_256_trains_in_bf16_and_its_mefc_matches():
    """DRSformer base, batch 1, 256^2, bf16: forward and backward with finite gradients.  Then its refinement MEFC (C = 96) on
    that plane, forward, against the oracle with the device's ReLU decisions, compared on a 64 x 64 crop and in its routing."""
    from image_restoration_amd import configs
    torch.manual_seed(0)
    net = N().DRSformer(**configs.DRSFORMER_BASE).to(DEV)
    x = seeded_input((1, 3, 256, 256), 501).to(DEV).to(torch.bfloat16).requires_grad_(True)
    y = net(x)
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all() and torch.isfinite(x.grad.float()).all()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    del y, x
    mod = net.refinement
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    h = seeded_input((1, 96, 256, 256), 502).to(torch.bfloat16).float()
    mod.record_masks = True
    yd = mod(h.to(DEV).to(torch.bfloat16).requires_grad_(True))
    torch.cuda.synchronize()
    masks = _cpu_masks(mod.relu_masks)
    with torch.no_grad():
        yr, ws = R.subnet(h.double(), {k: v.double() for k, v in sd.items()}, 1, 4, masks)
    crop = (slice(None), slice(None), slice(96, 160), slice(96, 160))
    e, ew = rel(yd[crop], yr[crop]), rel(masks[0]["w"], ws[0])
    print(f"MEFC C96 256^2 bf16: crop max-rel {e:.2e}, routing {ew:.2e}, whole plane {rel(yd, yr):.2e}")
    assert e < TOL[torch.bfloat16] and ew < TOL[torch.bfloat16]
