"""DarkIR's FreMLP on the MI355X: the native module against the reference fixtures and against the fp64 restatement
(tests/fremlp_ref.py) under bounds derived on the host, the two transforms on their own (exact integer cases, the c2r convention),
the zero-spectrum convention, accumulate, poisoned buffers, determinism, no_grad, and FlatTrainer training.

Bounds of the parity (test_fremlp_matches_restatement): 4x the error of the DENSE form of the restatement evaluated on the host in
the device's storage precision against the fp64 torch.fft form, per case, dtype and tensor (tests/golden/fremlp_bounds.npz,
written by tools/fremlp_bounds.py; the table is in DESIGN.md).  The transforms' bounds are formed the same way inside their tests."""
import functools
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import fremlp_ref as R  # noqa: E402
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
    spec = importlib.util.spec_from_file_location("capture_golden_fremlp", os.path.join(ROOT, "tools", "capture_golden_fremlp.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


def build(nc, expand, sd):
    mod = N().FreMLP(nc, expand)
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
def test_native_fremlp_matches_reference_fixtures(name):
    """fp32 against the fixtures captured from the reference, the bar of test_native_block_matches_reference_fixtures."""
    nc, expand, bhw, seed = G.CASES[name]
    sd = R.make_state(R.fremlp_shapes(nc, expand), seed)
    x, cot = G.case_io(nc, bhw, seed)
    got = run_native(build(nc, expand, sd), x, cot, torch.float32)
    gold = load(name)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-3, what=name + " ")


# ------------------------------------------------------------------ 2. parity against the fp64 restatement
@functools.lru_cache(maxsize=None)
def _bounds():
    return load("fremlp_bounds")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_fremlp_matches_restatement(name, dtype):
    """Per tensor max |delta| / max |ref| against the fp64 restatement (which sees the same rounded input and cotangent), within
    4x the host-side error of the dense form in the same storage precision.  Precondition on the input, not a tolerance: the
    fp64 spectrum keeps min |Z| >= 2e-4 rms |Z| (the phase gradient divides by |Z|).

    Measured on the MI355X: all 20 cases pass; the worst tensor sits at 0.63 x its bound in fp32 (plane256, process1.0.weight) and
    0.90 x in bf16 (max, process1.0.weight); y and dx in bf16 sit at 0.25 x (the one rounding the host model makes too).
    See DESIGN.md section 7l."""
    (B, nc, H, W), expand, _ = R.PARITY_CASES[name]
    sd, x, cot, _ = R.parity_io(name)
    x, cot = R.storage_io(x, cot, dtype)
    floor = R.spectrum_floor(x)
    assert floor >= R.FLOOR, (name, floor)
    ref = R.run(x, cot, sd)
    got = run_native(build(nc, expand, sd), x, cot, dtype)
    assert set(got) == set(ref)
    bounds, bad = _bounds(), []
    for k in ref:
        err, bound = R.rel_err(got[k], ref[k]), MARGIN * float(bounds[f"{name}.{TAGS[dtype]}.{k}"])
        # (a bound may be 0: at 2 x 2 in bf16 storage the host sums are exact, and so must the device's be)
        print(f"{name} {TAGS[dtype]} {k}: err {err:.3e} bound {bound:.3e} ({err / max(bound, 1e-300):.2f})")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


# ------------------------------------------------------------------ 3. the transforms alone
@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("W", [2, 4])
def test_r2c_is_exact_on_small_integers(H, W):
    """Every twiddle of a 2- or 4-point DFT is 0 or +-1 and the tables hold them exactly, so small-integer inputs transform
    exactly: equal to torch.fft.rfft2, bit for bit."""
    g = torch.Generator().manual_seed(10 * H + W)
    x = torch.randint(-8, 9, (3, 5, H, W), generator=g).float()
    ref = torch.fft.rfft2(x)
    zre, zim = O().dft2_r2c(x.to(DEV))
    assert torch.equal(zre.cpu(), ref.real) and torch.equal(zim.cpu(), ref.imag)
    zre, zim = O().dft2_r2c(x.to(DEV).bfloat16())
    assert torch.equal(zre.cpu(), ref.real) and torch.equal(zim.cpu(), ref.imag)


@pytest.mark.parametrize("name", ["odd", "seams"])
def test_transforms_alone_match_torch_fft(name):
    """mi_dft2_r2c against rfft2 and mi_dft2_c2r against irfft2 (fp64), each within 4x the fp32 host error of the dense form.
    The c2r input is NOT Hermitian: random imaginary parts in columns 0 and W/2, which irfft2 drops and so must the kernel."""
    (B, nc, H, W), _, seed = R.PARITY_CASES[name]
    K = W // 2 + 1
    x = seeded_input((B, nc, H, W), seed + 1)
    ref = torch.fft.rfft2(x.double())
    hre, him = R.r2c_dense(x)
    zre, zim = O().dft2_r2c(x.to(DEV))
    for tag, got, host, want in (("re", zre, hre, ref.real), ("im", zim, him, ref.imag)):
        err, bound = R.rel_err(got.cpu(), want), MARGIN * R.rel_err(host, want)
        print(f"r2c {name} {tag}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound
    yre, yim = seeded_input((B, nc, H, K), seed + 2), seeded_input((B, nc, H, K), seed + 3)
    assert float(yim[..., 0].abs().min()) > 0 and (W % 2 or float(yim[..., W // 2].abs().min()) > 0)
    want = torch.fft.irfft2(torch.complex(yre.double(), yim.double()), s=(H, W))
    host = R.c2r_dense(yre, yim, W)
    got = O().dft2_c2r(yre.to(DEV), yim.to(DEV), W)
    err, bound = R.rel_err(got.cpu(), want), MARGIN * R.rel_err(host, want)
    print(f"c2r {name}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    # bf16 output: the same values rounded once
    assert torch.equal(O().dft2_c2r(yre.to(DEV), yim.to(DEV), W, torch.bfloat16), got.bfloat16())


# ------------------------------------------------------------------ 4. the zero spectrum
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_zero_sample_on_the_device(dtype):
    """A sample of zeros has Z = 0 everywhere: u = (1, 0), so out = m delta at pixel (0, 0) with m = W2 LeakyReLU(b1) + b2; its dx
    is exactly 0; and the other sample of the batch is what it is without the zero sample, bit for bit."""
    name = "expand3"
    (B, nc, H, W), expand, _ = R.PARITY_CASES[name]
    sd, x, cot, _ = R.parity_io(name)
    x, cot = R.storage_io(x, cot, dtype)
    x[1] = 0
    mod = build(nc, expand, sd)
    got = run_native(mod, x, cot, dtype)
    p = {k: v.double() for k, v in sd.items()}
    m = p["process1.2.weight"].flatten(1) @ torch.nn.functional.leaky_relu(p["process1.0.bias"], 0.1) + p["process1.2.bias"]
    want = torch.zeros(nc, H, W, dtype=torch.float64)
    want[:, 0, 0] = m
    bound = MARGIN * float(_bounds()[f"{name}.{TAGS[dtype]}.y"])
    err = R.rel_err(got["y"][1], want)
    print(f"zero sample {TAGS[dtype]}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(got["dx"][1], torch.zeros(nc, H, W, dtype=dtype))
    assert all(float(got[k].abs().max()) > 0 for k in got if k.startswith("g."))
    alone = run_native(mod, x[:1], cot[:1], dtype)
    assert torch.equal(alone["y"][0], got["y"][0]) and torch.equal(alone["dx"][0], got["dx"][0])


# ------------------------------------------------------------------ 5. accumulate, poisoned buffers
def _raw(name, dtype, grads, accumulate):
    (B, nc, H, W), expand, _ = R.PARITY_CASES[name]
    sd, x, cot, _ = R.parity_io(name)
    params = [sd[k].to(DEV) for k in R.fremlp_shapes(nc, expand)]
    out, saved = O().fremlp_fwd(x.to(DEV).to(dtype), params, True)
    dx = O().fremlp_bwd(cot.to(DEV).to(dtype), params, saved, grads, accumulate)
    torch.cuda.synchronize()
    return out, dx


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_accumulate_and_poisoned_buffers(dtype):
    """Overwrite into NaN-filled gradient buffers leaves no NaN; accumulate on top of a base is base + the overwrite result, one
    fp32 addition per element; dx does not depend on the flag."""
    name = "seams"
    (B, nc, H, W), expand, _ = R.PARITY_CASES[name]
    shapes = R.fremlp_shapes(nc, expand)
    over = [torch.full(s, float("nan"), device=DEV) for s in shapes.values()]
    out, dx = _raw(name, dtype, over, False)
    assert all(bool(torch.isfinite(g).all()) for g in over) and bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dx.float()).all())
    base = [seeded_input(s, 74 + i).to(DEV) for i, s in enumerate(shapes.values())]
    acc = [b.clone() for b in base]
    out2, dx2 = _raw(name, dtype, acc, True)
    for a, b, g in zip(acc, base, over):
        assert torch.equal(a, b + g)
    assert torch.equal(out, out2) and torch.equal(dx, dx2)


# ------------------------------------------------------------------ 6. bitwise reproducibility, no_grad, CPU tensors
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fremlp_is_bitwise_reproducible_and_no_grad_equals_grad_mode(dtype):
    name = "seams"
    (B, nc, H, W), expand, _ = R.PARITY_CASES[name]
    sd, x, cot, _ = R.parity_io(name)
    mod = build(nc, expand, sd)
    a = run_native(mod, x, cot, dtype)
    b = run_native(mod, x, cot, dtype)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    xd = x.to(DEV).to(dtype)
    y = mod(xd.clone().requires_grad_(True))
    with torch.no_grad():
        y0 = mod(xd)
    assert y.requires_grad and not y0.requires_grad
    assert torch.equal(y.detach(), y0) and torch.equal(y0.cpu(), a["y"])
    with pytest.raises(RuntimeError, match="MI355X only"):
        mod(torch.zeros(1, nc, 8, 8))
    with pytest.raises(NotImplementedError, match="outside the supported"):
        mod(torch.zeros(1, nc, 1, 8, device=DEV))
    with pytest.raises(NotImplementedError, match="outside the supported"):
        mod(torch.zeros(1, nc, 8, 513, device=DEV))


# ------------------------------------------------------------------ 7. training
def test_training_steps_follow_the_oracle_trajectory():
    """Three FlatTrainer steps (main_grad accumulation, deferred sums, fused AdamW) of Sequential(LayerNorm2d, FreMLP) against the
    fp64 restatement plus torch.optim.AdamW, fp32; the bars of the DBlock trajectory test."""
    from image_restoration_amd.trainer import FlatTrainer
    import darkir_ref as D
    c = 16
    net = torch.nn.Sequential(N().LayerNorm2d(c), N().FreMLP(c))
    shapes = {"0.weight": (c,), "0.bias": (c,)}
    shapes.update({"1." + k: v for k, v in R.fremlp_shapes(c).items()})
    sd0 = R.make_state(shapes, 83)
    sd0["0.weight"] = 1.0 + 0.1 * seeded_input((c,), 84)
    net.load_state_dict(sd0)
    x, tgt = seeded_input((2, c, 32, 32), 85), seeded_input((2, c, 32, 32), 86)
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
        h = R.fremlp(D.layer_norm2d(x.double(), ps["0.weight"], ps["0.bias"]), {k[2:]: v for k, v in ps.items() if k.startswith("1.")})
        loss = (h - tgt.double()).abs().mean()
        loss.backward()
        opt.step()
        want = float(loss.detach())
        assert abs(losses[step] - want) < 1e-4 * want, (step, losses[step], want)
    for k, v in ps.items():
        w0 = sd0[k].double()
        a, r = got[k].double(), v.detach()
        d = (a - r).abs()
        ua, ur = (a - w0).flatten(), (r - w0).flatten()
        cos = float((ua @ ur) / (ua.norm() * ur.norm()).clamp_min(1e-30))
        assert cos >= 0.9995, (k, cos)
        assert float(d.mean()) <= 0.02 * lr and float(d.max()) <= 2.0 * lr, (k, float(d.mean()) / lr, float(d.max()) / lr)
