"""DarkIR's dilated-gate decoder block on the MI355X: the native DBlock against the reference fixtures and against the fp64
restatement (tests/darkir_ref.py) under bounds derived on the host, the stencil primitives on their own (one exact integer
case), determinism, no_grad, and FlatTrainer training.

Bounds of the block parity (test_block_matches_restatement): 4x the error of the restatement evaluated on the host in the device's
storage precision against fp64, per case, dtype and tensor (tests/golden/darkir_bounds.npz, written by tools/darkir_bounds.py;
the table is in DESIGN.md).  The primitives' bounds are formed the same way inside their tests."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import darkir_ref as D  # noqa: E402
from oracle.fixtures import check, load, seeded_input  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 4.0
TAGS = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def N():
    from image_restoration_amd import darkir
    return darkir


def O():
    from image_restoration_amd import ops
    return ops


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_darkir", os.path.join(ROOT, "tools", "capture_golden_darkir.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


def build(c, dil, extra, sd):
    mod = N().DBlock(c, dilations=list(dil), extra_depth_wise=extra)
    mod.load_state_dict(sd)
    return mod.to(DEV)


def run_native(mod, x, cot, dtype):
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    y = mod(xg)
    y.backward(cot.to(DEV).to(dtype))
    torch.cuda.synchronize()
    out = {"y": y.detach().cpu(), "dx": xg.grad.detach().cpu()}
    out.update({"g." + k: p.grad.detach().cpu() for k, p in mod.named_parameters()})
    return out


# ------------------------------------------------------------------ 1. the reference fixtures
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_native_block_matches_reference_fixtures(name):
    """fp32 against the fixtures captured from the reference, the bar of test_native_modules_match_reference_fixtures."""
    c, dil, extra, bhw, seed = G.CASES[name]
    sd = D.make_state(D.dblock_shapes(c, len(dil), extra), seed)
    x, cot = G.case_io(c, bhw, seed)
    got = run_native(build(c, dil, extra, sd), x, cot, torch.float32)
    gold = load(name)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-3, what=name + " ")


# ------------------------------------------------------------------ 2. the whole block against the fp64 restatement
@functools.lru_cache(maxsize=None)
def _bounds():
    return load("darkir_bounds")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(D.PARITY_CASES))
def test_block_matches_restatement(name, dtype):
    """Per tensor max |delta| / max |ref| against the fp64 restatement (which sees the same rounded input and cotangent), within
    4x the host-side error of the same storage precision.

    Measured on the MI355X: all 22 cases pass; the worst tensor sits at 0.72 x its bound in fp32 and 0.38 x in bf16 (the bf16 1x1
    products run on split weights: with plain bf16 weights conv1.bias' gradient was at 1.18 x and 1.09 x in two cases).
    See DESIGN.md section 7k."""
    (B, c, H, W), dil, extra = D.PARITY_CASES[name]
    sd, x, cot, _ = D.parity_io(name)
    x, cot = D.storage_io(x, cot, dtype)
    ref = D.run(x, cot, sd, dil)
    got = run_native(build(c, dil, extra, sd), x, cot, dtype)
    assert set(got) == set(ref)
    bounds, bad = _bounds(), []
    for k in ref:
        err, bound = D.rel_err(got[k], ref[k]), MARGIN * float(bounds[f"{name}.{TAGS[dtype]}.{k}"])
        print(f"{name} {TAGS[dtype]} {k}: err {err:.3e} bound {bound:.3e} ({err / bound:.2f})")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


# ------------------------------------------------------------------ 3. the primitives alone
def _branch_state(c, dil, seed, integer=False):
    rng = np.random.default_rng(seed)
    sd = {}
    for i in range(len(dil)):
        if integer:
            w, b = rng.integers(-1, 2, (2 * c, 1, 3, 3)), rng.integers(-1, 2, (2 * c,))
        else:
            w, b = rng.standard_normal((2 * c, 1, 3, 3)) / 3, 0.1 * rng.standard_normal((2 * c,))
        sd[f"branches.{i}.branch.0.weight"] = torch.from_numpy(np.asarray(w, dtype=np.float32))
        sd[f"branches.{i}.branch.0.bias"] = torch.from_numpy(np.asarray(b, dtype=np.float32))
    return sd


def _dilgate_ref(x, dg, add, sd, dil, dtype):
    """g, pool, dx and the branch gradients of the restatement's piece in ``dtype``; the pooled path's gradient enters as add."""
    p = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = x.to(dtype).requires_grad_(True)
    g, pool = D.dilgate(xr, p, dil)
    (g * (dg.to(dtype) + add.to(dtype)[:, :, None, None])).sum().backward()
    out = {"g": g.detach(), "pool": pool.detach(), "dx": xr.grad}
    out.update({"g." + k: v.grad for k, v in p.items()})
    return out


def _dilgate_native(x, dg, add, sd, dil, dtype, accumulate, base=None):
    ops = O()
    n = len(dil)
    ws = [sd[f"branches.{i}.branch.0.weight"].to(DEV) for i in range(n)]
    bs = [sd[f"branches.{i}.branch.0.bias"].to(DEV) for i in range(n)]
    xd = x.to(DEV).to(dtype)
    g, pool = ops.dilgate_fwd(xd, ws, bs, dil)
    gw = [torch.full_like(w, float("nan")) if base is None else base[f"g.branches.{i}.branch.0.weight"].to(DEV).clone()
          for i, w in enumerate(ws)]
    gb = [torch.full_like(b, float("nan")) if base is None else base[f"g.branches.{i}.branch.0.bias"].to(DEV).clone()
          for i, b in enumerate(bs)]
    dx = ops.dilgate_bwd(dg.to(DEV).to(dtype), None if add is None else add.to(DEV), xd, ws, bs, dil, gw, gb, accumulate)
    torch.cuda.synchronize()
    out = {"g": g.cpu(), "pool": pool.cpu(), "dx": dx.cpu()}
    for i in range(n):
        out[f"g.branches.{i}.branch.0.weight"], out[f"g.branches.{i}.branch.0.bias"] = gw[i].cpu(), gb[i].cpu()
    return out


DILGATE_CASES = [((3, 5, 37, 100), (1, 4, 9)), ((2, 3, 5, 7), (16, 16, 2, 1)), ((1, 4, 70, 1), (9,))]


@pytest.mark.parametrize("shape,dil", DILGATE_CASES, ids=["seams", "sub_halo_4_branches", "column"])
def test_dilgate_alone_matches_restatement(shape, dil):
    """mi_dilgate_fwd / _bwd in fp32 with a non-zero dg_add, overwrite and accumulate; bound: 4x the fp32 host error."""
    B, c, H, W = shape
    sd = _branch_state(c, dil, 7)
    x, dg = seeded_input((B, 2 * c, H, W), 71), seeded_input((B, c, H, W), 72)
    add = seeded_input((B, c), 73)
    ref = _dilgate_ref(x, dg, add, sd, dil, torch.float64)
    host = _dilgate_ref(x, dg, add, sd, dil, torch.float32)
    got = _dilgate_native(x, dg, add, sd, dil, torch.float32, accumulate=False)
    bad = []
    for k in ref:
        err, bound = D.rel_err(got[k], ref[k]), MARGIN * D.rel_err(host[k], ref[k])
        print(f"dilgate {shape} {dil} {k}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad
    # accumulate: the same gradients on top of a base; one fp32 addition of the overwrite result per element
    base = {k: seeded_input(tuple(v.shape), 74) for k, v in ref.items() if k.startswith("g.")}
    acc = _dilgate_native(x, dg, add, sd, dil, torch.float32, accumulate=True, base=base)
    for k in base:
        assert torch.equal(acc[k], base[k] + got[k]), k
    assert torch.equal(acc["dx"], got["dx"])
    # no addend = an addend of zeros
    z = _dilgate_native(x, dg, torch.zeros(B, c), sd, dil, torch.float32, accumulate=False)
    nz = _dilgate_native(x, dg, None, sd, dil, torch.float32, accumulate=False)
    assert all(torch.equal(z[k], nz[k]) for k in z)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_dilgate_is_exact_on_integers(dtype):
    """Small integer inputs and weights: every sum stays below 2^24 (and every stored value below 2^8 where it is bf16), so the
    output, the pool sums and every gradient equal the restatement exactly - a wrong tap or tile seam cannot hide in a tolerance.
    Two tile columns, two tile rows, ragged in both; dilations 1, 4, 9 and a repeated 4."""
    B, c, H, W, dil = 2, 3, 37, 70, (1, 4, 9, 4)
    rng = np.random.default_rng(5)
    sd = _branch_state(c, dil, 8, integer=True)
    small = dtype == torch.bfloat16          # bf16 stores g, dz and dx: keep them below 256
    x = torch.from_numpy(rng.integers(-1 if small else -2, 2 if small else 3, (B, 2 * c, H, W))).float()
    if small:
        for k in sd:
            if k.endswith("weight"):
                sd[k] = sd[k] * (torch.from_numpy(rng.random(tuple(sd[k].shape))) < 0.25).float()
    dg = torch.from_numpy(rng.integers(-1 if small else -2, 2 if small else 3, (B, c, H, W))).float()
    add = torch.from_numpy(rng.integers(0 if small else -1, 2, (B, c))).float()
    ref = _dilgate_ref(x, dg, add, sd, dil, torch.float64)
    z = D.dilated_sum(x.double(), {k: v.double() for k, v in sd.items()}, dil)
    dz = torch.cat([z[:, c:], z[:, :c]], 1) * (dg.double() + add.double()[:, :, None, None]).repeat(1, 2, 1, 1)
    lim = 256 if small else 2 ** 24
    assert ref["g"].abs().max() < lim and dz.abs().max() < lim and ref["dx"].abs().max() < lim
    assert max(v.abs().max() for v in ref.values()) < 2 ** 24
    got = _dilgate_native(x, dg, add, sd, dil, dtype, accumulate=False)
    for k in ref:
        assert torch.equal(got[k].double(), ref[k]), (k, float((got[k].double() - ref[k]).abs().max()))


@pytest.mark.parametrize("shape", [(3, 5, 37, 100), (2, 3, 5, 7), (1, 2, 1, 33)], ids=["seams", "tiny", "row"])
def test_pairconv3x3_alone_matches_restatement(shape):
    B, c, H, W = shape
    rng = np.random.default_rng(9)
    w = torch.from_numpy(rng.standard_normal((2 * c, 2, 3, 3)) / 4).float()
    b = torch.from_numpy(0.1 * rng.standard_normal((2 * c,))).float()
    x, dy = seeded_input((B, 2 * c, H, W), 91), seeded_input((B, 2 * c, H, W), 92)

    def ref_in(dtype):
        xr, wr, br = (t.to(dtype).requires_grad_(True) for t in (x, w, b))
        y = D.pairconv(xr, wr, br)
        y.backward(dy.to(dtype))
        return {"y": y.detach(), "dx": xr.grad, "dw": wr.grad, "db": br.grad}

    ref, host = ref_in(torch.float64), ref_in(torch.float32)
    ops = O()
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    dw, db = torch.full_like(wd, float("nan")), torch.full_like(bd, float("nan"))
    y = ops.pairconv3x3_fwd(xd, wd, bd)
    dx = ops.pairconv3x3_bwd(dy.to(DEV), xd, wd, dw, db, False)
    got = {"y": y.cpu(), "dx": dx.cpu(), "dw": dw.cpu(), "db": db.cpu()}
    bad = []
    for k in ref:
        err, bound = D.rel_err(got[k], ref[k]), MARGIN * D.rel_err(host[k], ref[k])
        print(f"pairconv {shape} {k}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad
    dw2, db2 = dw.clone(), db.clone()
    ops.pairconv3x3_bwd(dy.to(DEV), xd, wd, dw2, db2, True)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)
    # without a bias: forward and backward
    y0 = ops.pairconv3x3_fwd(xd, wd, None).cpu()
    r0, h0 = D.pairconv(x.double(), w.double(), None), D.pairconv(x, w, None)
    assert D.rel_err(y0, r0) <= MARGIN * D.rel_err(h0, r0)
    dw3 = torch.full_like(wd, float("nan"))
    assert torch.equal(ops.pairconv3x3_bwd(dy.to(DEV), xd, wd, dw3, None, False), dx) and torch.equal(dw3, dw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 32, 9, 11), (1, 256, 8, 8), (2, 64, 32, 64)], ids=["odd", "c256", "aligned"])
def test_ln_fwd_eps(shape, dtype):
    """mi_ln_fwd_eps at 1e-5 is bitwise mi_ln_fwd (output and statistics); at 1e-6 it follows the fp64 LayerNorm2d.  The input
    has near-constant pixels, where eps decides the result."""
    ops = O()
    B, c, H, W = shape
    x = seeded_input(shape, 95)
    x[:, :, 0, :] = 1.0 + 1e-2 * x[:, :, 0, :]
    w, b = 1.0 + 0.1 * seeded_input((c,), 96), 0.1 * seeded_input((c,), 97)
    xd, wd, bd = x.to(DEV).to(dtype), w.to(DEV), b.to(DEV)
    y5, m5, r5 = ops.ln_fwd(xd, wd, bd, True)
    e5, em5, er5 = ops.ln_fwd_eps(xd, wd, bd, True, 1e-5)
    assert torch.equal(y5, e5) and torch.equal(m5, em5) and torch.equal(r5, er5)
    y6, _, r6 = ops.ln_fwd_eps(xd, wd, bd, True, 1e-6)
    assert not torch.equal(r5, r6)
    xs = xd.float().cpu()
    ref = D.layer_norm2d(xs.double(), w.double(), b.double())
    host = D.layer_norm2d(xs, w, b).to(dtype)
    err, bound = D.rel_err(y6.cpu(), ref), MARGIN * D.rel_err(host, ref)
    print(f"ln_fwd_eps {shape} {TAGS[dtype]}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------ 4. bitwise reproducibility
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_block_is_bitwise_reproducible(dtype):
    (B, c, H, W), dil, extra = D.PARITY_CASES["seams_b3"]
    sd, x, cot, _ = D.parity_io("seams_b3")
    mod = build(c, dil, extra, sd)
    a = run_native(mod, x, cot, dtype)
    b = run_native(mod, x, cot, dtype)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------ 5. no_grad, CPU tensors
def test_no_grad_output_equals_grad_mode_and_cpu_is_refused():
    (B, c, H, W), dil, extra = D.PARITY_CASES["seams_c64"]
    sd, x, _, _ = D.parity_io("seams_c64")
    mod = build(c, dil, extra, sd)
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(DEV).to(dtype)
        y = mod(xd.clone().requires_grad_(True))
        with torch.no_grad():
            y0 = mod(xd)
        assert y.requires_grad and not y0.requires_grad
        assert torch.equal(y.detach(), y0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        mod(torch.zeros(1, c, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        N().LayerNorm2d(c)(torch.zeros(1, c, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        N().SimpleGate()(torch.zeros(1, c, 8, 8))


def test_simple_gate_and_layernorm2d_modules():
    """The two small modules on their own kernels, forward and backward, fp32 against fp64 (bound: 4x the fp32 host error)."""
    x, cot = seeded_input((2, 12, 9, 11), 98), seeded_input((2, 6, 9, 11), 99)
    xg = x.to(DEV).requires_grad_(True)
    y = N().SimpleGate()(xg)
    y.backward(cot.to(DEV))
    assert torch.equal(y.detach().cpu(), x[:, :6] * x[:, 6:])
    assert torch.equal(xg.grad.cpu(), torch.cat([cot * x[:, 6:], cot * x[:, :6]], 1))
    ln = N().LayerNorm2d(12).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.1 * seeded_input((12,), 1))
        ln.bias.copy_(0.1 * seeded_input((12,), 2))
    cot = seeded_input((2, 12, 9, 11), 3)
    xg = x.to(DEV).requires_grad_(True)
    ln(xg).backward(cot.to(DEV))

    def ref_in(dtype):
        xr, w, b = x.to(dtype).requires_grad_(True), ln.weight.detach().cpu().to(dtype).requires_grad_(True), \
            ln.bias.detach().cpu().to(dtype).requires_grad_(True)
        D.layer_norm2d(xr, w, b).backward(cot.to(dtype))
        return {"dx": xr.grad, "dw": w.grad, "db": b.grad}

    ref, host = ref_in(torch.float64), ref_in(torch.float32)
    got = {"dx": xg.grad.cpu(), "dw": ln.weight.grad.cpu(), "db": ln.bias.grad.cpu()}
    for k in ref:
        assert D.rel_err(got[k], ref[k]) <= MARGIN * D.rel_err(host[k], ref[k]), k


# ------------------------------------------------------------------ 6. training
def test_training_steps_follow_the_oracle_trajectory():
    """Three FlatTrainer steps (main_grad accumulation, deferred sums, fused AdamW) of a stack of two DBlocks against the fp64
    restatement plus torch.optim.AdamW, fp32; the displacement-in-lr bar of the DRSformer trajectory test."""
    from image_restoration_amd.trainer import FlatTrainer
    c, dil = 32, (1, 4, 9)
    net = torch.nn.Sequential(N().DBlock(c, dilations=list(dil), extra_depth_wise=True),
                              N().DBlock(c, dilations=list(dil), extra_depth_wise=True))
    sd0 = D.make_state({f"{i}.{k}": v for i in range(2) for k, v in D.dblock_shapes(c, 3, True).items()}, 81)
    net.load_state_dict(sd0)
    x, tgt = seeded_input((2, c, 32, 32), 81), seeded_input((2, c, 32, 32), 82)
    lr = 1e-3
    net = net.to(DEV).train()
    tr = FlatTrainer(net, lr=lr, weight_decay=0.01)
    losses = []
    try:
        xd, td = x.to(DEV), tgt.to(DEV)
        for _ in range(3):
            tr.zero_grad()
            loss = (net(xd) - td).abs().mean()
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
        h = D.dblock_stack(x.double(), [{k[2:]: v for k, v in ps.items() if k.startswith(f"{i}.")} for i in range(2)], dil)
        loss = (h - tgt.double()).abs().mean()
        loss.backward()
        opt.step()
        assert abs(losses[step] - float(loss)) < 1e-4 * float(loss), (step, losses[step], float(loss))
    for k, v in ps.items():
        w0 = sd0[k].double()
        a, r = got[k].double(), v.detach()
        d = (a - r).abs()
        ua, ur = (a - w0).flatten(), (r - w0).flatten()
        cos = float((ua @ ur) / (ua.norm() * ur.norm()).clamp_min(1e-30))
        assert cos >= 0.9995, (k, cos)
        assert float(d.mean()) <= 0.02 * lr and float(d.max()) <= 2.0 * lr, (k, float(d.mean()) / lr, float(d.max()) / lr)
