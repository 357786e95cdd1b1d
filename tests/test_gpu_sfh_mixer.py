"""SFHformer's TokenMixer_For_Gloal and Mixer on the MI355X: the native modules against the reference fixtures and against the fp64
restatement (tests/sfh_mixer_ref.py) under bounds derived on the host, accumulate, poisoned buffers, determinism, no_grad, the
running statistics, and FlatTrainer training.

Bounds of the parity (test_modules_match_restatement): 4x the error of the DEVICE form of the restatement evaluated on the host in
the device's storage precision against the fp64 form, per case, dtype and tensor (tests/golden/sfh_mixer_bounds.npz, written by
tools/sfh_mixer_bounds.py; the table is in DESIGN.md section 7s); a host error below 2^-24, one fp32 ulp of the tensor's maximum, is
taken as 2^-24.  MARGIN is test_gpu_sfh_ffn.py's."""
import ctypes as C
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

import sfh_mixer_ref as R  # noqa: E402
from oracle.fixtures import load, seeded_input  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 4.0
ULP = 2.0 ** -24
TAGS = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def N():
    from image_restoration_amd import sfhformer
    return sfhformer


def O():
    from image_restoration_amd import ops
    return ops


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_sfh_mixer", os.path.join(ROOT, "tools", "capture_golden_sfh_mixer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


def build(kind, dim, sd, training=True):
    mod = getattr(N(), G.CLASSES[kind])(dim)
    mod.load_state_dict(R.module_state(kind, sd), strict=True)
    return mod.to(DEV).train(training)


def run_native(mod, kind, x, cot, dtype):
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    y = mod(xg)
    y.backward(cot.to(DEV).to(dtype))
    torch.cuda.synchronize()
    sd = mod.state_dict()
    out = {"y": y.detach().cpu(), "dx": xg.grad.detach().cpu(), "rm": sd[R.RM[kind]].cpu().clone(), "rv": sd[R.RV[kind]].cpu().clone()}
    out.update({"g." + k: p.grad.detach().cpu() for k, p in mod.named_parameters()})
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    """The fp64 restatement of a parity case on the input and cotangent as ``dtype`` stores them: computed once, shared, unchanged."""
    kind, sd, x, cot, training = R.parity_io(name)
    x, cot = R.storage_io(x, cot, dtype)
    return R.run(kind, x, cot, sd, training)


# ------------------------------------------------------------------ 1. the reference fixtures
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_native_modules_match_reference_fixtures(name):
    """fp32 against the fixtures captured from the reference, the bar of the FFN's fixture test: output, dx, every parameter
    gradient and the running statistics after the call."""
    kind, dim, bhw, seed, training = G.CASES[name]
    x, cot = G.case_io(dim, bhw, seed)
    got = run_native(build(kind, dim, G.case_state(kind, dim, seed, training), training), kind, x, cot, torch.float32)
    gold = load(name)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        R.check(k, v, gold, 1e-3, what=name + " ")


# ------------------------------------------------------------------ 2. parity against the fp64 restatement
@functools.lru_cache(maxsize=None)
def _bounds():
    return load("sfh_mixer_bounds")


def _compare(name, dtype, got, ref):
    bounds, bad, worst = _bounds(), [], 0.0
    for k in ref:
        assert got[k].shape == ref[k].shape and bool(torch.isfinite(got[k].float()).all()), k
        err, bound = R.rel_err(got[k], ref[k]), MARGIN * max(float(bounds[f"{name}.{TAGS[dtype]}.{k}"]), ULP)
        worst = max(worst, err / bound)
        print(f"{name} {TAGS[dtype]} {k}: err {err:.3e} bound {bound:.3e} ({err / bound:.2f})")
        if not err <= bound:
            bad.append((k, err, bound))
    print(f"{name} {TAGS[dtype]} WORST {worst:.2f}")
    return bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_modules_match_restatement(name, dtype):
    """Per tensor max |delta| / max |ref| against the fp64 restatement (which sees the same rounded input and cotangent), within 4x
    the host-side error of the device form in the same storage precision (never less than 4 x 2^-24): output, dx, every parameter
    gradient and the running statistics; every element of every tensor.  The preconditions of the case list (tests/sfh_mixer_ref.py)
    are on the host model, not on the device.

    Measured on the MI355X: all 28 cases pass.  Worst device-to-bound ratio per case, fp32 / bf16: tiny 0.65 / 0.25, odd 0.40 / 0.25,
    tile_plus_1 0.78 / 0.27, b3 0.59 / 0.27, ragged 0.43 / 0.26, pool2 0.72 / 0.26, deep 0.41 / 0.25, wide 0.39 / 0.28, odd_eval 0.40 /
    0.25, b3_eval 0.37 / 0.25, glo_odd 0.88 / 0.25, glo_b3 0.45 / 0.25, glo_wide 0.40 / 0.25, glo_eval 0.29 / 0.25.  See DESIGN.md section
    7s (and there what the host model first missed: the order in which the per-image Gram is summed)."""
    kind, (B, dim, H, W), _, _ = R.PARITY_CASES[name]
    kind, sd, x, cot, training = R.parity_io(name)
    x, cot = R.storage_io(x, cot, dtype)
    ref = _reference(name, dtype)
    got = run_native(build(kind, dim, sd, training), kind, x, cot, dtype)
    assert set(got) == set(ref) == R.tensors(kind)
    bad = _compare(name, dtype, got, ref)
    assert not bad, bad


# ------------------------------------------------------------------ 3. accumulate, poisoned buffers
def _raw(name, dtype, grads, accumulate, poison):
    """One forward and backward straight through the C-ABI on buffers of the test's own: workspace, saved blob, out and dx filled
    with 0xff bytes (NaN in either dtype) first when ``poison``."""
    from image_restoration_amd import _lib as L
    kind, (B, dim, H, W), _, _ = R.PARITY_CASES[name]
    kind, sd, x, cot, training = R.parity_io(name)
    ops, lib = O(), L.lib()
    params = [sd[k].to(DEV).contiguous() for k in R.PARAMS[kind]]
    rm, rv = sd[R.RM[kind]].to(DEV).clone(), sd[R.RV[kind]].to(DEV).clone()
    fill = 0xFF if poison else 0
    xd, cd = x.to(DEV).to(dtype), cot.to(DEV).to(dtype)
    out = torch.full((xd.numel() * xd.element_size(),), fill, dtype=torch.uint8, device=DEV).view(dtype).view_as(xd)
    dx = torch.full((xd.numel() * xd.element_size(),), fill, dtype=torch.uint8, device=DEV).view(dtype).view_as(xd)
    st = ops._stream()
    s = L.SfhMixerShape(B, dim, H, W, ops._dtype_code(dtype), int(training), 1e-5, 0.1)
    mix = kind == "mixer"
    sizes = (lib.mi_sfh_mixer_workspace, lib.mi_sfh_mixer_saved_bytes) if mix else (lib.mi_sfh_global_workspace, lib.mi_sfh_global_saved_bytes)
    fwd, bwd = (lib.mi_sfh_mixer_fwd, lib.mi_sfh_mixer_bwd) if mix else (lib.mi_sfh_global_fwd, lib.mi_sfh_global_bwd)
    ws = torch.full((sizes[0](C.byref(s)),), fill, dtype=torch.uint8, device=DEV)
    saved = torch.full((sizes[1](C.byref(s)),), fill, dtype=torch.uint8, device=DEV)
    pp = (L.SfhMixerParams if mix else L.SfhGlobalParams)(*[p.data_ptr() for p in params])
    gg = (L.SfhMixerGrads if mix else L.SfhGlobalGrads)(*[g.data_ptr() for g in grads], int(accumulate))
    L.check(fwd(C.byref(s), C.byref(pp), xd.data_ptr(), out.data_ptr(), rm.data_ptr(), rv.data_ptr(), saved.data_ptr(), ws.data_ptr(), st), "fwd")
    ws.fill_(fill)
    L.check(bwd(C.byref(s), C.byref(pp), xd.data_ptr(), cd.data_ptr(), dx.data_ptr(), C.byref(gg), saved.data_ptr(), ws.data_ptr(), st), "bwd")
    torch.cuda.synchronize()
    return out, dx


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["odd", "b3", "ragged", "glo_odd"])
def test_accumulate_and_poisoned_buffers(name, dtype):
    """Workspace, saved blob, out, dx and the gradient buffers NaN-filled before an overwriting call: no NaN comes out, and the
    results equal those on zero-filled buffers bit for bit (nothing is read before it is written).  Accumulate on top of a base is
    base + the overwrite result, one fp32 addition per element; out and dx do not depend on the flag."""
    kind, (B, dim, H, W), _, _ = R.PARITY_CASES[name]
    shapes = [tuple(R.parity_io(name)[1][k].shape) for k in R.PARAMS[kind]]
    over = [torch.full(s, float("nan"), device=DEV) for s in shapes]
    out, dx = _raw(name, dtype, over, False, True)
    assert all(bool(torch.isfinite(g).all()) for g in over)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dx.float()).all())
    assert all(float(g.abs().max()) > 0 for g in over)
    clean = [torch.zeros(s, device=DEV) for s in shapes]
    out0, dx0 = _raw(name, dtype, clean, False, False)
    for a, b in zip(over, clean):
        assert torch.equal(a, b)
    base = [seeded_input(s, 74 + i).to(DEV) for i, s in enumerate(shapes)]
    acc = [b.clone() for b in base]
    out2, dx2 = _raw(name, dtype, acc, True, True)
    for a, b, g in zip(acc, base, over):
        assert torch.equal(a, b + g)
    for a, b, c_ in ((out, out0, out2), (dx, dx0, dx2)):
        assert torch.equal(a, b) and torch.equal(a, c_)


# ------------------------------------------------------------------ 4. bitwise reproducibility, no_grad, running statistics
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["ragged", "glo_b3"])
def test_modules_are_bitwise_reproducible_and_no_grad_equals_grad_mode(name, dtype):
    kind, (B, dim, H, W), _, _ = R.PARITY_CASES[name]
    kind, sd, x, cot, training = R.parity_io(name)
    a = run_native(build(kind, dim, sd), kind, x, cot, dtype)
    b = run_native(build(kind, dim, sd), kind, x, cot, dtype)
    assert set(a) == R.tensors(kind)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    xd = x.to(DEV).to(dtype)
    mod = build(kind, dim, sd)
    with torch.no_grad():
        y0 = mod(xd)                                   # saved == NULL: nothing is kept
    assert not y0.requires_grad and y0.grad_fn is None and torch.equal(y0.cpu(), a["y"])
    after = mod.state_dict()                           # ... yet the running statistics moved, exactly as in grad mode
    assert torch.equal(after[R.RM[kind]].cpu(), a["rm"]) and torch.equal(after[R.RV[kind]].cpu(), a["rv"])
    assert not torch.equal(a["rm"], sd[R.RM[kind]])
    assert int(after[R.RM[kind].replace("running_mean", "num_batches_tracked")]) == 1
    with pytest.raises(RuntimeError, match="MI355X only"):
        mod(torch.zeros(1, dim, 8, 8))
    for wrong in (dim + 2, dim + 1):                   # (an odd count too: not the library's "dim is odd" refusal)
        with pytest.raises(ValueError, match="do not fit"):
            mod(torch.zeros(1, wrong, 8, 8, device=DEV))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_training_forwards_each_match_their_own_restatement(dtype):
    """Two consecutive training forwards with different inputs through ONE module: each output, and the running statistics after
    each, match the restatement fed the statistics the previous call left (the per-image folded weights and the pool are not reused
    from the first call); num_batches_tracked counts."""
    name = "b3"
    kind, (B, dim, H, W), _, _ = R.PARITY_CASES[name]
    kind, sd, x, cot, training = R.parity_io(name)
    x, cot = R.storage_io(x, cot, dtype)
    x2 = R.storage_io(seeded_input(tuple(x.shape), 75), cot, dtype)[0]
    mod = build(kind, dim, sd)
    ref1 = _reference(name, dtype)
    got1 = run_native(mod, kind, x, cot, dtype)
    assert not _compare(name, dtype, got1, ref1)
    sd2 = dict(sd)
    sd2[R.RM[kind]], sd2[R.RV[kind]] = ref1["rm"].float(), ref1["rv"].float()
    ref2 = R.run(kind, x2, cot, sd2, training)
    got2 = run_native(mod, kind, x2, cot, dtype)
    assert not _compare(name, dtype, got2, ref2)          # the bounds of the case: same shapes, same parameters
    assert not torch.equal(got1["y"], got2["y"])
    assert int(mod.state_dict()[R.RM[kind].replace("running_mean", "num_batches_tracked")]) == 2


# ------------------------------------------------------------------ 5. training
def test_flat_trainer_takes_two_steps_and_moves_every_parameter():
    """Mixer(8) flattened into a FlatTrainer (main_grad accumulation, deferred sums, fused AdamW): two steps, every parameter
    finite and moved, the first loss within 1e-4 relative of the restatement's."""
    from image_restoration_amd.trainer import FlatTrainer
    kind, dim = "mixer", 8
    sd0 = R.make_state(kind, dim, 91)
    net = build(kind, dim, sd0)
    x, tgt = seeded_input((2, dim, 16, 20), 92), seeded_input((2, dim, 16, 20), 93)
    tr = FlatTrainer(net, lr=1e-3, weight_decay=0.01)
    losses = []
    try:
        xd, td = x.to(DEV), tgt.to(DEV)
        for _ in range(2):
            tr.zero_grad()
            loss = (net(xd) - td).abs().mean()
            loss.backward()
            tr.reduce_gradients()
            tr.optimizer_step()
            losses.append(float(loss.detach()))
        got = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    finally:
        tr.close()
    assert all(l == l and abs(l) < 1e6 for l in losses)
    for k in R.PARAMS[kind]:
        assert bool(torch.isfinite(got[k]).all()), k
        assert float((got[k] - sd0[k]).abs().max()) > 0, k          # (a hidden unit that is off for every image has zero gradients)
    want = float((R.run(kind, x, x, sd0)["y"] - tgt.double()).abs().mean())
    assert abs(losses[0] - want) < 1e-4 * want, (losses[0], want)
