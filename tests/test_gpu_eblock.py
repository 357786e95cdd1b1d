"""DarkIR's encoder block and the whole network on the MI355X: the native EBlock against the reference fixtures and against the
fp64 restatement (tests/eblock_ref.py) under bounds derived on the host, the tail kernels (mi_fregate_*) on their own with one
exact integer case, determinism, no_grad, an all-zero sample, the DarkIR network, and FlatTrainer training.

Bounds of the parity tests: 4x the error of the restatement evaluated on the host in the device's storage precision (FreMLP in its
dense form) against fp64, per case, dtype and tensor (tests/golden/eblock_bounds.npz, written by tools/eblock_bounds.py; the table
is in DESIGN.md section 7m).  Every case first asserts the spectral floor of its FreMLP inputs on the fp64 evaluation."""
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
import eblock_ref as E  # noqa: E402
from oracle.fixtures import check, load, seeded_input  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 4.0
TAGS = {torch.float32: "fp32", torch.bfloat16: "bf16"}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def N():
    from image_restoration_amd import darkir
    return darkir


def O():
    from image_restoration_amd import ops
    return ops


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_eblock", os.path.join(ROOT, "tools", "capture_golden_eblock.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


def build(c, dil, extra, sd):
    mod = N().EBlock(c, dilations=list(dil), extra_depth_wise=extra)
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


@functools.lru_cache(maxsize=None)
def _bounds():
    return load("eblock_bounds")


def _within_bounds(case, dtype, got, ref):
    assert set(got) == set(ref)
    bounds, bad, worst = _bounds(), [], 0.0
    for k in ref:
        err, bound = D.rel_err(got[k], ref[k]), MARGIN * float(bounds[f"{case}.{TAGS[dtype]}.{k}"])
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))    # (a sum of bf16 values can be exact in fp32)
        print(f"{case} {TAGS[dtype]} {k}: err {err:.3e} bound {bound:.3e} ({ratio:.2f})")
        worst = max(worst, ratio)
        if not err <= bound:
            bad.append((k, err, bound))
    print(f"{case} {TAGS[dtype]}: worst ratio to the bound {worst:.2f}")
    assert not bad, bad


# ------------------------------------------------------------------ 1. the reference fixtures
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_native_block_matches_reference_fixtures(name):
    """fp32 against the fixtures captured from the reference's EBlock, the bar of test_gpu_darkir.py."""
    c, dil, extra, bhw, seed = G.CASES[name]
    sd = E.make_state(E.eblock_shapes(c, len(dil), extra), seed)
    x, cot = G.case_io(c, bhw, seed)
    got = run_native(build(c, dil, extra, sd), x, cot, torch.float32)
    gold = load(name)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        check(k, v, gold, 1e-3, what=name + " ")


# ------------------------------------------------------------------ 2. the whole block against the fp64 restatement
@DTYPES
@pytest.mark.parametrize("name", list(E.PARITY_CASES))
def test_block_matches_restatement(name, dtype):
    """Per tensor max |delta| / max |ref| against the fp64 restatement (which sees the same rounded input and cotangent), within
    4x the host-side error of the same storage precision; the FreMLP input keeps the spectral floor.

    Measured on the MI355X: all 16 cases pass; the worst tensor sits at 0.74 x its bound in fp32 (plane128, norm2.bias) and
    0.69 x in bf16 (max_dil, conv1.bias).  That tensor was at 1.04 x while the restatement rounded the gradient at y once: the
    device also stores the residual's share on its own (mi_fregate_bwd writes it, mi_ln_bwd adds it), which eblock_ref.eblock
    now models.  See DESIGN.md section 7m."""
    (B, c, H, W), dil, extra, _ = E.PARITY_CASES[name]
    sd, x, cot, _ = E.parity_io(name)
    x, cot = E.storage_io(x, cot, dtype)
    probe = []
    ref = E.run(x, cot, sd, dil, probe=probe)
    assert E.floor_margin(probe) >= E.FLOOR, E.floor_margin(probe)
    got = run_native(build(c, dil, extra, sd), x, cot, dtype)
    _within_bounds(name, dtype, got, ref)


# ------------------------------------------------------------------ 3. the tail kernels alone
def _fregate_ref(y, f, gamma, dout, dtype, rnd=E._id):
    yr, fr, gr = (t.detach().to(dtype).clone().requires_grad_(True) for t in (y, f, gamma))
    out = rnd(E.fregate(yr, fr, gr))
    out.backward(dout.to(dtype))
    # the kernel's two data gradients: through f, and the residual's share (everything that reaches y directly)
    return {"out": out.detach(), "df": rnd(fr.grad), "dyr": rnd(yr.grad), "dgamma": gr.grad}


def _fregate_native(y, f, gamma, dout, dtype, accumulate, base=None):
    ops = O()
    yd, fd, dd = (t.to(DEV).to(dtype) for t in (y, f, dout))
    gd = gamma.to(DEV)
    out = ops.fregate_fwd(yd, fd, gd)
    dg = torch.full_like(gd, float("nan")) if base is None else base.to(DEV).clone()
    df, dyr = ops.fregate_bwd(dd, yd, fd, gd, dg, accumulate)
    torch.cuda.synchronize()
    return {"out": out.cpu(), "df": df.cpu(), "dyr": dyr.cpu(), "dgamma": dg.cpu()}


FREGATE_SHAPES = [(2, 4, 2, 2), (3, 5, 3, 3), (2, 8, 33, 65)]


@DTYPES
@pytest.mark.parametrize("shape", FREGATE_SHAPES, ids=["n4", "odd_unaligned", "vectors_and_tail"])
def test_fregate_alone_matches_restatement(shape, dtype):
    """mi_fregate_fwd / _bwd against fp64, overwrite and accumulate; bound: 4x the host error of the same storage precision.
    (3, 5, 3, 3): N = 9 is odd, so the planes start at every alignment the dtype has; (2, 8, 33, 65): vectors, head and tail."""
    B, c, H, W = shape
    y, f, dout = (E.storage_io(seeded_input(shape, 60 + i), seeded_input(shape, 60 + i), dtype)[0] for i in range(3))
    gamma = 0.5 + 0.2 * seeded_input((c,), 64)
    ref = _fregate_ref(y, f, gamma, dout, torch.float64)
    host = _fregate_ref(y, f, gamma, dout, torch.float32, E._id if dtype == torch.float32 else E.round_bf16)
    got = _fregate_native(y, f, gamma, dout, dtype, accumulate=False)
    bad = []
    for k in ref:
        err, bound = D.rel_err(got[k], ref[k]), MARGIN * D.rel_err(host[k], ref[k])
        print(f"fregate {shape} {TAGS[dtype]} {k}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad
    base = seeded_input((c,), 65)
    acc = _fregate_native(y, f, gamma, dout, dtype, accumulate=True, base=base)
    assert torch.equal(acc["dgamma"], base + got["dgamma"])             # one fp32 addition of the overwrite result
    assert all(torch.equal(acc[k], got[k]) for k in ("out", "df", "dyr"))
    again = _fregate_native(y, f, gamma, dout, dtype, accumulate=False)
    assert all(torch.equal(again[k], got[k]) for k in got)              # bitwise over two runs


@DTYPES
@pytest.mark.parametrize("shape", FREGATE_SHAPES, ids=["n4", "odd_unaligned", "vectors_and_tail"])
def test_fregate_is_exact_on_integers(shape, dtype):
    """Small integers: every product and sum is exact in fp32 and every stored value is below 2^8, so out, df, dyr and dgamma equal
    the fp64 result exactly in both dtypes - a wrong head, tail or channel index cannot hide in a tolerance."""
    B, c, H, W = shape
    rng = np.random.default_rng(66)
    y, f, dout = (torch.from_numpy(rng.integers(-3, 4, shape)).float() for _ in range(3))
    gamma = torch.from_numpy(rng.integers(-2, 3, (c,))).float()
    ref = _fregate_ref(y, f, gamma, dout, torch.float64)
    assert max(float(ref[k].abs().max()) for k in ("out", "df", "dyr")) < 256 and float(ref["dgamma"].abs().max()) < 2 ** 24
    for accumulate in (False, True):
        base = torch.from_numpy(rng.integers(-5, 6, (c,))).float() if accumulate else None
        got = _fregate_native(y, f, gamma, dout, dtype, accumulate, base)
        for k in ("out", "df", "dyr"):
            assert torch.equal(got[k].double(), ref[k]), (k, accumulate)
        assert torch.equal(got["dgamma"].double(), ref["dgamma"] + (base.double() if accumulate else 0)), accumulate


def test_fregate_takes_misaligned_views():
    """Tensors whose bases disagree modulo 16 bytes take the scalar form; the result is bitwise that of the vector form."""
    ops = O()
    shape = (2, 3, 5, 8)
    n = int(np.prod(shape))
    y, f, dout = (seeded_input(shape, 67 + i).to(DEV).to(torch.bfloat16) for i in range(3))
    gamma = (0.5 + 0.2 * seeded_input((3,), 70)).to(DEV)

    def shifted(t, k):
        buf = torch.empty(n + 8, dtype=t.dtype, device=DEV)
        v = buf[k:k + n].view(shape)
        v.copy_(t)
        return v

    dg0, dg1 = torch.empty_like(gamma), torch.empty_like(gamma)
    out0 = ops.fregate_fwd(y, f, gamma)
    df0, dyr0 = ops.fregate_bwd(dout, y, f, gamma, dg0, False)
    ys, fs, ds = shifted(y, 1), shifted(f, 3), shifted(dout, 0)
    out1 = ops.fregate_fwd(ys, fs, gamma)
    df1, dyr1 = ops.fregate_bwd(ds, ys, fs, gamma, dg1, False)
    assert torch.equal(out0, out1) and torch.equal(df0, df1) and torch.equal(dyr0, dyr1)
    # the sum's grouping differs between the two forms: one rounding of an fp32 sum of 80 terms
    assert torch.allclose(dg0, dg1, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ 4. block behaviour
@DTYPES
def test_block_is_bitwise_reproducible(dtype):
    (B, c, H, W), dil, extra, _ = E.PARITY_CASES["seams_b3"]
    sd, x, cot, _ = E.parity_io("seams_b3")
    mod = build(c, dil, extra, sd)
    a = run_native(mod, x, cot, dtype)
    b = run_native(mod, x, cot, dtype)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_no_grad_output_equals_grad_mode_and_zero_sample_is_finite():
    (B, c, H, W), dil, extra, _ = E.PARITY_CASES["net_level"]
    sd, x, cot, _ = E.parity_io("net_level")
    mod = build(c, dil, extra, sd)
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(DEV).to(dtype)
        y = mod(xd.clone().requires_grad_(True))
        with torch.no_grad():
            y0 = mod(xd)
        assert y.requires_grad and not y0.requires_grad
        assert torch.equal(y.detach(), y0)
        # an all-zero sample: LayerNorm gives its bias on every pixel, a spectrum with one live bin per channel; FreMLP's
        # zero-bin rule (u = (1, 0), no gradient) has to survive LayerNorm in front of it and the gate behind it
        xz = x.clone()
        xz[0] = 0
        got = run_native(mod, xz, cot, dtype)
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), (TAGS[dtype], k)
    with pytest.raises(RuntimeError, match="MI355X only"):
        mod(torch.zeros(1, c, 8, 8))
    with pytest.raises(NotImplementedError, match="not covered"):
        mod(torch.zeros(1, c, 1, 8, device=DEV))


FIRST_HALF = ("norm1.", "conv1.", "branches.", "sca.1.", "conv3.", "beta")


@DTYPES
@pytest.mark.parametrize("name", ["tiny", "max_dil"])
def test_first_half_is_dblocks_first_half_bitwise(name, dtype):
    """The two blocks' first halves are one function (csrc/darkir.hip runs one launch sequence for both).  Without extra_conv and
    with gamma = 0 both tails are the identity on y and hand dout back unchanged as the gradient at y: DBlock's 0 . W5 gives exact
    zeros and 0 + dres is exact; EBlock's fma(0, f, 1) is 1 and a zero cotangent through FreMLP above its spectral floor stays
    zero.  So out, dinp and the gradient of every first-half parameter of an EBlock and of a DBlock that shares its first-half
    parameters (norm2 / conv4 / conv5 random) are equal bit for bit."""
    (B, c, H, W), dil, extra, seed = E.PARITY_CASES[name]
    assert not extra
    sd, x, cot, _ = E.parity_io(name)
    sd = dict(sd, gamma=torch.zeros_like(sd["gamma"]))
    dsd = D.make_state(D.dblock_shapes(c, len(dil), False), seed + 60)
    dsd.update({k: v for k, v in sd.items() if k.startswith(FIRST_HALF)}, gamma=sd["gamma"])
    e = run_native(build(c, dil, False, sd), x, cot, dtype)
    dmod = N().DBlock(c, dilations=list(dil), extra_depth_wise=False)
    dmod.load_state_dict(dsd)
    d = run_native(dmod.to(DEV), x, cot, dtype)
    keys = ["y", "dx"] + ["g." + k for k in sd if k.startswith(FIRST_HALF)]
    assert len(keys) == 2 + 9 + 2 * len(dil)
    diff = [k for k in keys if not torch.equal(e[k], d[k])]
    assert not diff, diff


# ------------------------------------------------------------------ 5. the network
def _run_net_native(net, x, cots, dtype):
    net.zero_grad(set_to_none=True)
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    side, y = net(xg, side_loss=True)
    torch.autograd.backward([side, y], [cots[0].to(DEV).to(dtype), cots[1].to(DEV).to(dtype)])
    torch.cuda.synchronize()
    out = {"side": side.detach().cpu(), "y": y.detach().cpu(), "dx": xg.grad.detach().cpu()}
    out.update({"g." + k: p.grad.detach().cpu() for k, p in net.named_parameters()})
    return out


@DTYPES
def test_small_network_matches_restatement_and_fixture(dtype):
    """DarkIR(width 8, enc [1, 1], dec [1, 1], middle 1 / 1) on (2, 3, 18, 27) with side_loss=True (padded to 20 x 28): both
    outputs, dx and every parameter gradient against the fp64 restatement under the host model's bounds; fp32 also against the
    fixture captured from the reference at 1e-3.

    Measured on the MI355X: worst ratio 0.66 x in fp32, 0.60 x in bf16 (downs.1.bias).  With the glue convolutions' weights
    rounded to bf16 by the MFMA path five bias gradients of the deeper levels sat at 1.06 - 1.50 x (reproduced on the host);
    with bf16 activations they run on split weights now.  See DESIGN.md section 7m."""
    sd, x, cots = E.net_io()
    x, c1 = E.storage_io(x, cots[1], dtype)
    c0 = cots[0].to(dtype).float()
    probe = []
    ref = E.run_net(x, (c0, c1), sd, E.SMALL_NET, probe=probe)
    assert len(probe) == 3 and E.floor_margin(probe) >= E.FLOOR, E.floor_margin(probe)
    net = N().DarkIR(**E.SMALL_NET)
    net.load_state_dict(sd)
    got = _run_net_native(net.to(DEV), x, (c0, c1), dtype)
    assert got["y"].shape == x.shape and got["side"].shape == c0.shape
    _within_bounds("net", dtype, got, ref)
    if dtype == torch.float32:
        gold = load(G.NET_CASE)
        assert {k[:-4] for k in gold.files if k.endswith(".sub")} == set(got)
        for k, v in got.items():
            check(k, v, gold, 1e-3, what="net ")


def test_default_network_runs_in_bf16():
    """DarkIR-m (width 32, c up to 256) at (1, 3, 32, 32) in bf16: loads the recorded key list, forward and backward finite."""
    net = N().DarkIR()
    keys = load("darkir_net_keys")
    shapes = E.net_shapes(E.net_config())
    assert list(shapes) == [str(k) for k in keys["darkir_m.keys"]]
    net.load_state_dict(E.make_state(shapes, 7), strict=True)
    net = net.to(DEV)
    x = seeded_input((1, 3, 32, 32), 8).to(DEV).to(torch.bfloat16).requires_grad_(True)
    out = net(x)
    assert out.shape == x.shape
    out.float().abs().mean().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())
    missing = [k for k, p in net.named_parameters() if p.grad is None and not k.startswith("side_out")]
    assert not missing, missing
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    with pytest.raises(NotImplementedError, match="512"):
        net(torch.zeros(1, 3, 8, 520, device=DEV))


# ------------------------------------------------------------------ 6. training
def test_training_steps_follow_the_oracle_trajectory():
    """Three FlatTrainer steps (main_grad accumulation, deferred sums, fused AdamW) of Sequential(EBlock, DBlock) against the fp64
    restatement plus torch.optim.AdamW, fp32, with the bars of test_gpu_darkir's trajectory test.  The seed was picked on the CPU
    so that the fp32 host restatement meets those bars (tests/test_eblock_golden.py checks it): they test the device."""
    from image_restoration_amd.trainer import FlatTrainer
    c = E.TRAIN_C
    net = torch.nn.Sequential(N().EBlock(c, extra_depth_wise=True),
                              N().DBlock(c, dilations=list(E.TRAIN_DIL), extra_depth_wise=True))
    sd0, x, tgt = E.train_io()
    net.load_state_dict(sd0)
    net = net.to(DEV).train()
    tr = FlatTrainer(net, lr=E.TRAIN_LR, weight_decay=E.TRAIN_WD)
    losses = []
    try:
        xd, td = x.to(DEV), tgt.to(DEV)
        for _ in range(E.TRAIN_STEPS):
            tr.zero_grad()
            loss = (net(xd) - td).abs().mean()
            loss.backward()
            tr.reduce_gradients()
            tr.optimizer_step()
            losses.append(float(loss.detach()))
        got = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    finally:
        tr.close()
    ref_losses, ref = E.train_reference(sd0, x, tgt)
    misses = E.trajectory_misses(losses, got, ref_losses, ref, sd0)
    assert not misses, misses
