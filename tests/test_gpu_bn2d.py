"""The SFHformer Block's BatchNorm2d and scaled residual on the MI355X: the native module and function against the fp64 restatement
(tests/bn2d_ref.py) under bounds derived on the host, the exact properties (a constant channel, scale = 0, the two seams kept for the
Block, bitwise reproducibility), poisoned buffers and guard bands, accumulate, the refusal of one value per channel, no_grad, and
FlatTrainer training.

Bounds of the parity (test_native_matches_restatement): 4x the error of the DEVICE form of the restatement evaluated on the host in
the device's storage precision against the fp64 formulas, per case, dtype, mode and tensor (tests/golden/bn2d_bounds.npz, written by
tools/bn2d_bounds.py; the table is in DESIGN.md section 7t); a host error below 2^-24, one fp32 ulp of the tensor's maximum, is taken
as 2^-24.  MARGIN is test_gpu_sfh_ffn.py's."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import bn2d_ref as R  # noqa: E402
import eblock_ref as E  # noqa: E402  (the trajectory bars of DESIGN.md section 7m)
from oracle.fixtures import load, seeded_input  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 4.0
ULP = 2.0 ** -24
TAGS = {torch.float32: "fp32", torch.bfloat16: "bf16"}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
MODES = pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
SMALL = ["odd", "ch_p1", "ragged", "const"]          # narrow and 16-byte forms, one and several chunks, ragged tails


def N():
    from image_restoration_amd import sfhformer
    return sfhformer


def O():
    from image_restoration_amd import ops
    return ops


def build(io, training=True):
    C_ = io["x"].shape[1]
    bn = N().BatchNorm2d(C_, eps=R.EPS, momentum=R.MOMENTUM)
    bn.load_state_dict({"weight": io["w"], "bias": io["b"], "running_mean": io["rm"], "running_var": io["rv"],
                        "num_batches_tracked": torch.tensor(0)}, strict=True)
    return bn.to(DEV).train(training)


def run_native(io, dtype, training, scale_shape=None):
    """BatchNorm2d and scaled_residual, forward and backward, on one case's tensors -> {name: CPU tensor} over R.TENSORS."""
    C_ = io["x"].shape[1]
    bn = build(io, training)
    dev = lambda k: io[k].to(DEV).to(dtype)   # noqa: E731
    x, f, xr = (dev(k).requires_grad_(True) for k in ("x", "f", "x"))
    scale = torch.nn.Parameter(io["scale"].to(DEV).view(scale_shape or (1, C_, 1, 1)))
    cot = dev("cot")
    y = bn(x)
    y.backward(cot)
    out = N().scaled_residual(f, xr, scale)
    out.backward(cot)
    torch.cuda.synchronize()
    assert torch.equal(xr.grad, cot)                     # the gradient towards x is the cotangent itself
    assert int(bn.num_batches_tracked) == int(training)  # what torch.nn.BatchNorm2d counts (tests/test_bn2d_golden.py)
    assert scale.grad.shape == scale.shape
    got = {"y": y.detach(), "dx": x.grad, "dw": bn.weight.grad, "db": bn.bias.grad, "rm": bn.running_mean, "rv": bn.running_var,
           "out": out.detach(), "df": f.grad, "ds": scale.grad.reshape(-1)}
    return {k: v.detach().cpu().clone() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, training):
    """The fp64 restatement of a parity case on the activations as ``dtype`` stores them: computed once, shared, unchanged."""
    return R.run(R.stored(R.parity_io(name), dtype), training)


@functools.lru_cache(maxsize=None)
def _bounds():
    return load("bn2d_bounds")


def _bound(name, dtype, training, k):
    return MARGIN * max(float(_bounds()[f"{name}.{TAGS[dtype]}.{'train' if training else 'eval'}.{k}"]), ULP)


def _compare(name, dtype, training, got, ref, keys=R.TENSORS):
    bad, worst = [], 0.0
    for k in keys:
        assert got[k].shape == ref[k].shape and bool(torch.isfinite(got[k].float()).all()), k
        err, bound = R.rel_err(got[k], ref[k]), _bound(name, dtype, training, k)
        worst = max(worst, err / bound)
        print(f"{name} {TAGS[dtype]} {'train' if training else 'eval'} {k}: err {err:.3e} bound {bound:.3e} ({err / bound:.2f})")
        if not err <= bound:
            bad.append((k, err, bound))
    print(f"{name} {TAGS[dtype]} {'train' if training else 'eval'} WORST {worst:.2f}")
    return bad


# ------------------------------------------------------------------ 1. parity against the fp64 restatement
@MODES
@DTYPES
@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_native_matches_restatement(name, dtype, training):
    """Per tensor max |delta| / max |ref| against the fp64 restatement (which sees the same rounded activations and cotangent), within
    4x the host-side error of the device form in the same storage precision (never less than 4 x 2^-24): y, dx, dw, db, the running
    statistics after the call, and out, df, ds; every element of every tensor.  "const": the constant channel normalises to exactly
    b[c] in training mode (its chunk means are exactly 2.0, so x - mu is exactly 0).

    Measured on the MI355X: all 88 runs pass, and the worst device-to-bound ratio is 0.25 in every case, dtype and mode: the device's
    error equals the host model's, whose operations and summation order are the kernels' (floating-point contraction is off in
    csrc/bn2d.hip).  See DESIGN.md section 7t for the table."""
    io = R.stored(R.parity_io(name), dtype)
    ref = _reference(name, dtype, training)
    got = run_native(io, dtype, training)
    assert set(got) == set(ref) == set(R.TENSORS)
    bad = _compare(name, dtype, training, got, ref)
    assert not bad, bad
    if R.PARITY_CASES[name][2] == "const" and training:
        want = io["b"][1].to(dtype).float()
        assert bool((got["y"][:, 1].float() == want).all())
        assert not torch.equal(got["rm"], io["rm"])


# ------------------------------------------------------------------ 2. exact properties
@DTYPES
@pytest.mark.parametrize("name", ["odd", "ragged"])
def test_scale_zero_returns_x_itself(name, dtype):
    """The reference initialises beta and gamma to 0: out is x bit for bit, df is 0, and ds = sum f dout keeps the parity bound.
    Also a scale of shape (C,)."""
    io = dict(R.stored(R.parity_io(name), dtype))
    io["scale"] = torch.zeros_like(io["scale"])
    got = run_native(io, dtype, True, scale_shape=(io["x"].shape[1],))
    assert torch.equal(got["out"], io["x"].to(dtype))
    assert float(got["df"].float().abs().max()) == 0.0
    ref = R.run(io, True)
    assert float(ref["ds"].abs().max()) > 0
    assert not _compare(name, dtype, True, got, ref, keys=("ds",))


@DTYPES
@pytest.mark.parametrize("name", SMALL)
def test_forward_seam_part_in_equals_own_statistics(name, dtype):
    """scale_res_fwd(..., want_part) writes the BatchNorm pairs of out as stored; bn2d_fwd(out, part_in) then skips its statistics
    pass and gives y, stat and both running statistics bit for bit as bn2d_fwd(out) does on its own."""
    io, ops = R.parity_io(name), O()
    f, x = io["f"].to(DEV).to(dtype), io["x"].to(DEV).to(dtype)
    w, b, s = (io[k].to(DEV) for k in ("w", "b", "scale"))
    out, part = ops.scale_res_fwd(f, x, s, want_part=True)
    plain = ops.scale_res_fwd(f, x, s)
    assert torch.equal(out, plain) and part.numel() * 4 == ops.bn2d_plan(*x.shape, dtype)["pair_bytes"]
    res = []
    for part_in in (part, None):
        rm, rv = io["rm"].to(DEV).clone(), io["rv"].to(DEV).clone()
        y, stat = ops.bn2d_fwd(out, w, b, rm, rv, True, True, R.EPS, R.MOMENTUM, part_in=part_in)
        res.append((y, stat, rm, rv))
    torch.cuda.synchronize()
    for a, c in zip(*res):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, c)
    assert not torch.equal(res[0][2].cpu(), io["rm"])


@MODES
@DTYPES
@pytest.mark.parametrize("name", SMALL)
def test_backward_seam_dres(name, dtype, training):
    """bn2d_bwd(..., dres) writes dx + dres, added in fp32 and rounded once: in fp32 that is bn2d_bwd(...) followed by + dres bit for
    bit; in bf16 it keeps dx's parity bound against the fp64 sum (the bound of the case's dx: the same single rounding).  dw and db
    do not depend on dres."""
    io, ops = R.stored(R.parity_io(name), dtype), O()
    x, cot, dres = io["x"].to(DEV).to(dtype), io["cot"].to(DEV).to(dtype), io["f"].to(DEV).to(dtype)
    w, b = io["w"].to(DEV), io["b"].to(DEV)
    rm, rv = io["rm"].to(DEV).clone(), io["rv"].to(DEV).clone()
    _, stat = ops.bn2d_fwd(x, w, b, rm, rv, training, True, R.EPS, R.MOMENTUM)
    g0, g1 = [torch.empty_like(w), torch.empty_like(w)], [torch.empty_like(w), torch.empty_like(w)]
    dx = ops.bn2d_bwd(x, cot, w, stat, g0, False, training, R.EPS, R.MOMENTUM)
    both = ops.bn2d_bwd(x, cot, w, stat, g1, False, training, R.EPS, R.MOMENTUM, dres=dres)
    torch.cuda.synchronize()
    assert torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])
    if dtype == torch.float32:
        assert torch.equal(both, dx + dres)
    want = _reference(name, dtype, training)["dx"] + io["f"].double()
    err, bound = R.rel_err(both.cpu(), want), _bound(name, dtype, training, "dx")
    assert err <= bound, (err, bound)


@MODES
@DTYPES
@pytest.mark.parametrize("name", ["odd", "ragged"])
def test_every_entry_point_is_bitwise_reproducible(name, dtype, training):
    io, ops = R.parity_io(name), O()

    def once():
        x, f, cot = (io[k].to(DEV).to(dtype) for k in ("x", "f", "cot"))
        w, b, s = (io[k].to(DEV) for k in ("w", "b", "scale"))
        rm, rv = io["rm"].to(DEV).clone(), io["rv"].to(DEV).clone()
        y, stat = ops.bn2d_fwd(x, w, b, rm, rv, training, True, R.EPS, R.MOMENTUM)
        dw, db, ds = torch.empty_like(w), torch.empty_like(w), torch.empty_like(s)
        dx = ops.bn2d_bwd(x, cot, w, stat, (dw, db), False, training, R.EPS, R.MOMENTUM, dres=f)
        out, part = ops.scale_res_fwd(f, x, s, want_part=True)
        df = ops.scale_res_bwd(f, cot, s, ds, False)
        torch.cuda.synchronize()
        return y, stat, rm, rv, dx, dw, db, out, part, df, ds

    for a, c in zip(once(), once()):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, c)


# ------------------------------------------------------------------ 3. poisoned buffers, guard bands, accumulate
GUARD = 256


def _filled(nbytes, fill, guard=GUARD):
    t = torch.full((nbytes + guard,), fill, dtype=torch.uint8, device=DEV)
    t[nbytes:] = 0xA5
    return t


def _raw(name, dtype, training, grads, accumulate, fill):
    """All four entry points straight through the C-ABI on buffers of the test's own: workspaces, stat, y, dx, out and df filled with
    ``fill`` bytes first (0xff: NaN in either dtype), a guard band of 0xa5 bytes behind each workspace and behind stat."""
    from image_restoration_amd import _lib as L
    io, ops, lib = R.parity_io(name), O(), L.lib()
    B, C_, H, W = io["x"].shape
    x, f, cot = (io[k].to(DEV).to(dtype) for k in ("x", "f", "cot"))
    w, b, sc = (io[k].to(DEV) for k in ("w", "b", "scale"))
    rm, rv = io["rm"].to(DEV).clone(), io["rv"].to(DEV).clone()
    s = L.Bn2dShape(B, C_, H, W, ops._dtype_code(dtype), int(training), R.EPS, R.MOMENTUM)
    nb = x.numel() * x.element_size()
    ws_bytes, ws2_bytes = lib.mi_bn2d_workspace(C.byref(s)), lib.mi_scale_res_workspace(C.byref(s))
    ws, ws2, stat = _filled(ws_bytes, fill), _filled(ws2_bytes, fill), _filled(8 * C_, fill)
    y, dx, out, df = (_filled(nb, fill, 0).view(dtype).view_as(x) for _ in range(4))
    dw, db, ds = grads
    st = ops._stream()
    p = lambda t: t.data_ptr()   # noqa: E731
    L.check(lib.mi_bn2d_fwd(C.byref(s), p(w), p(b), p(x), p(y), p(rm), p(rv), p(stat), None, p(ws), st), "fwd")
    ws[:ws_bytes] = fill
    L.check(lib.mi_bn2d_bwd(C.byref(s), p(w), p(x), p(cot), None, p(dx), p(dw), p(db), int(accumulate), p(stat), p(ws), st), "bwd")
    L.check(lib.mi_scale_res_fwd(C.byref(s), p(sc), p(f), p(x), p(out), None, st), "res fwd")
    L.check(lib.mi_scale_res_bwd(C.byref(s), p(sc), p(f), p(cot), p(df), p(ds), int(accumulate), p(ws2), st), "res bwd")
    torch.cuda.synchronize()
    for t, n in ((ws, ws_bytes), (ws2, ws2_bytes), (stat, 8 * C_)):
        assert bool((t[n:] == 0xA5).all()), "a guard band was written"
    return y, dx, out, df, rm, rv, stat[:8 * C_].view(torch.float32).clone()


@MODES
@DTYPES
@pytest.mark.parametrize("name", ["odd", "ch_p1", "ragged"])
def test_poisoned_buffers_guard_bands_and_accumulate(name, dtype, training):
    """Workspaces, stat, y, dx, out, df and the gradient buffers NaN-filled before an overwriting call: no NaN comes out, every
    output is fully written, the guard bands behind the workspaces and behind stat are untouched, and the results equal those on
    zero-filled buffers bit for bit (nothing is read before it is written).  accumulate = 1 on top of a base is base + the overwrite
    result, one fp32 addition per element; the activations do not depend on the flag."""
    C_ = R.PARITY_CASES[name][0][1]
    over = [torch.full((C_,), float("nan"), device=DEV) for _ in range(3)]
    res = _raw(name, dtype, training, over, False, 0xFF)
    assert all(bool(torch.isfinite(t.float()).all()) for t in (*res, *over))
    assert all(float(g.abs().max()) > 0 for g in over)
    clean = [torch.zeros(C_, device=DEV) for _ in range(3)]
    res0 = _raw(name, dtype, training, clean, False, 0)
    base = [seeded_input((C_,), 84 + i).to(DEV) for i in range(3)]
    acc = [t.clone() for t in base]
    res2 = _raw(name, dtype, training, acc, True, 0xFF)
    for a, c, g in zip(acc, base, over):
        assert torch.equal(a, c + g)
    for a, c in zip(over, clean):
        assert torch.equal(a, c)
    for a, c, d in zip(res, res0, res2):
        assert torch.equal(a, c) and torch.equal(a, d)


# ------------------------------------------------------------------ 4. refusals, grad mode
@DTYPES
def test_one_value_per_channel_trains_nowhere_and_evaluates(dtype):
    """Training with B H W = 1 is refused, as torch refuses it (no variance); eval mode at that shape runs and matches the formula."""
    io = R.parity_io("n2")
    io = {k: (v[:1] if k in ("x", "f", "cot") else v) for k, v in io.items()}
    x = io["x"].to(DEV).to(dtype)
    bn = build(io, True)
    with pytest.raises(NotImplementedError, match="B\\*H\\*W = 1"):
        bn(x)
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean.cpu(), io["rm"])
    with pytest.raises(ValueError):
        torch.nn.BatchNorm2d(3).train()(torch.zeros(1, 3, 1, 1))
    bn.eval()
    y = bn(x)
    want = R.batch_norm(x.cpu().double(), *(io[k].double() for k in ("w", "b", "rm", "rv")), False)[0]
    host = R.batch_norm_device(x.cpu().float(), *(io[k] for k in ("w", "b", "rm", "rv")), False,
                               R._id if dtype == torch.float32 else R.round_bf16, R.vec_width(dtype))[0]
    assert R.rel_err(y.cpu(), want) <= MARGIN * max(R.rel_err(host, want), ULP)      # the parity's rule, on this shape's own host error
    with pytest.raises(ValueError, match="does not fit"):
        bn(torch.zeros(2, 4, 2, 2, device=DEV, dtype=dtype))
    with pytest.raises(ValueError, match="does not fit"):
        N().scaled_residual(x, x, torch.zeros(4, device=DEV))


@DTYPES
@pytest.mark.parametrize("name", ["odd", "ragged"])
def test_no_grad_saves_nothing_and_still_updates_the_running_statistics(name, dtype):
    io = R.parity_io(name)
    a = run_native(io, dtype, True)
    bn = build(io, True)
    x, f = io["x"].to(DEV).to(dtype), io["f"].to(DEV).to(dtype)
    scale = torch.nn.Parameter(io["scale"].to(DEV).view(1, -1, 1, 1))
    with torch.no_grad():
        y0 = bn(x)                                     # stat == NULL: nothing is kept
        out0 = N().scaled_residual(f, x, scale)
    assert not y0.requires_grad and y0.grad_fn is None and out0.grad_fn is None
    assert torch.equal(y0.cpu(), a["y"]) and torch.equal(out0.cpu(), a["out"])
    assert torch.equal(bn.running_mean.cpu(), a["rm"]) and torch.equal(bn.running_var.cpu(), a["rv"])
    assert not torch.equal(a["rm"], io["rm"]) and int(bn.num_batches_tracked) == 1
    bn.eval()
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    y1 = bn(x.requires_grad_(True))
    y1.sum().backward()
    assert all(torch.equal(v, bn.state_dict()[k]) for k, v in before.items()) and x.grad is not None


# ------------------------------------------------------------------ 5. training
def test_training_steps_follow_the_oracle_trajectory():
    """Three FlatTrainer steps (main_grad accumulation, fused AdamW) of Sequential(Conv2d 1x1, BatchNorm2d) at (2, 4, 8, 8), fp32,
    against the fp64 restatement plus torch.optim.AdamW under the bars of the EBlock / DBlock trajectory test (DESIGN.md section 7m:
    eblock_ref.trajectory_misses).  The conv has no bias: BatchNorm removes a per-channel shift, so that bias has an exactly zero
    gradient, and AdamW would normalise its rounding noise into a step of random sign on both sides."""
    from image_restoration_amd.trainer import FlatTrainer
    Cn, shape = 4, (2, 4, 8, 8)
    x, tgt = seeded_input(shape, 94), seeded_input(shape, 95)
    sd0 = {"0.weight": 0.5 * seeded_input((Cn, Cn, 1, 1), 96), "1.weight": 1.0 + 0.3 * seeded_input((Cn,), 97),
           "1.bias": 0.1 * seeded_input((Cn,), 98)}
    net = torch.nn.Sequential(torch.nn.Conv2d(Cn, Cn, 1, bias=False), N().BatchNorm2d(Cn))
    net.load_state_dict(sd0, strict=False)
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
    ps = {k: v.double().clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.AdamW(list(ps.values()), lr=E.TRAIN_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=E.TRAIN_WD)
    rm, rv, ref_losses = torch.zeros(Cn, dtype=torch.float64), torch.ones(Cn, dtype=torch.float64), []
    for _ in range(E.TRAIN_STEPS):
        opt.zero_grad()
        h = torch.nn.functional.conv2d(x.double(), ps["0.weight"])
        y, rm, rv = R.batch_norm(h, ps["1.weight"], ps["1.bias"], rm, rv, True)
        loss = (y - tgt.double()).abs().mean()
        loss.backward()
        opt.step()
        ref_losses.append(float(loss.detach()))
    misses = E.trajectory_misses(losses, got, ref_losses, {k: v.detach() for k, v in ps.items()}, sd0)
    assert not misses, misses
    assert int(got["1.num_batches_tracked"]) == E.TRAIN_STEPS
    assert not torch.equal(got["1.running_mean"], torch.zeros(Cn)) and not torch.equal(got["1.running_var"], torch.ones(Cn))
