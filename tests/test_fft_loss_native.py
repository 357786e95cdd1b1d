"""The native FFT loss (mi_fft_l1_loss, csrc/fftloss.hip; FFTLoss(native=True)): rfft2 L1 and its gradient as dense-DFT
GEMMs on the fp32 MFMA, against the reference's goldens, the fp64 oracle and today's rocFFT path.

CPU part: workspace sizing, argument errors and the plan query (the plan the launcher itself follows).  GPU part: values and
gradients.  The gradient is a sum of signs of spectrum coefficients, so every GPU case that is not a reference golden builds its
inputs FROM a spectrum whose non-structural coefficients have magnitude in [1, 2]: no coefficient sits within rounding of zero,
and a flipped sign is then a kernel error, not noise.  Tolerances: the fp32 cases hold the bars tests/test_train_tail.py holds
the rocFFT path to (1e-4 on the loss, 1e-4 on the relative gradient norm; an fp32 dense DFT with exact quadrant twiddles lands
near 1e-7 on both); the bf16 cases hold the bars of test_losses_on_gpu_against_oracle (2e-3 / 2e-2: dpred is stored in bf16)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import train_tail_ref as T

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


# --------------------------------------------------------------------------- CPU: sizing, errors, the plan
SECTION_ORDER = ("cos_w", "sin_w", "cos_wt", "sin_wt", "cos_h", "sin_h", "T", "S", "partials", "reduce_scratch")


def test_workspace_sizing_without_gpu(lib):
    from image_restoration_amd import ops
    L = lib.lib()
    for shape in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, -1), (-2, 3, 16, 16)):
        assert L.mi_fft_l1_workspace(*shape) == 0, shape
    for shape in ((1, 1, 2, 2), (1, 3, 15, 21), (2, 3, 128, 128), (1, 1, 512, 512), (7, 1, 16, 32), (32, 3, 256, 256)):
        n = L.mi_fft_l1_workspace(*shape)
        assert n > 0 and n % 256 == 0, shape
        for want_grad in (True, False):
            plan = ops.fft_l1_plan(*shape, torch.float32, want_grad)
            off, size = plan["sections"][SECTION_ORDER[-1]]
            assert max(o + b for o, b in plan["sections"].values()) == off + size      # the last section ends last
            assert n == plan["workspace"] == (off + size + 255) // 256 * 256, (shape, want_grad)
    # past the size limit there is no workspace either
    assert L.mi_fft_l1_workspace(1, 1, 513, 16) == 0 and L.mi_fft_l1_workspace(1, 1, 16, 1) == 0


def test_argument_errors_without_gpu(lib):
    """Every refusal returns before anything is launched: the host buffers standing in for device memory are never touched."""
    L = lib.lib()
    buf = [C.create_string_buffer(64) for _ in range(5)]
    pred, target, dpred, loss, ws = [C.cast(b, C.c_void_p) for b in buf]
    ok = dict(pred=pred, target=target, dpred=dpred, loss=loss, B=1, C=1, H=4, W=4, lw=1.0, dtype=lib.MI_F32, ws=ws)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.mi_fft_l1_loss(a["pred"], a["target"], a["dpred"], a["loss"], a["B"], a["C"], a["H"], a["W"], a["lw"], a["dtype"],
                              a["ws"], None)
        return rc, L.mi_last_error()

    for name in ("pred", "target", "loss", "ws"):
        rc, msg = call(**{name: None})
        assert rc < 0 and b"null pointer" in msg, name
    for kw in (dict(H=1), dict(W=1), dict(H=513), dict(W=513)):
        rc, msg = call(**kw)
        assert rc < 0 and b"outside the supported 2..512" in msg, kw
    rc, msg = call(dtype=7)
    assert rc < 0 and b"bad dtype 7" in msg
    rc, msg = call(B=0)
    assert rc < 0 and len(msg) > 0
    assert all(b.raw == bytes(64) for b in buf)
    # the plan query refuses the same things
    out = (C.c_int64 * 40)()
    assert L.mi_fft_l1_plan(1, 3, 16, 16, lib.MI_F32, 1, None) < 0 and b"null pointer" in L.mi_last_error()
    assert L.mi_fft_l1_plan(1, 3, 513, 16, lib.MI_F32, 1, out) < 0 and b"outside the supported" in L.mi_last_error()
    assert L.mi_fft_l1_plan(1, 3, 16, 1, lib.MI_F32, 1, out) < 0
    assert L.mi_fft_l1_plan(1, 3, 16, 16, 7, 1, out) < 0 and b"bad dtype 7" in L.mi_last_error()
    assert L.mi_fft_l1_plan(0, 3, 16, 16, lib.MI_F32, 1, out) < 0


def _sections(*sizes):
    """(offset, bytes) of consecutive sections, each starting on a 256-byte boundary."""
    out, o = {}, 0
    for name, n in zip(SECTION_ORDER, sizes):
        out[name] = (o, n)
        o = (o + n + 255) // 256 * 256
    return out, o


def _expected_plan(B, Cc, H, W, l_block, x_block, want_grad):
    """The plan from first principles: 64-row tiles, the pinned block widths, one loss partial per stage-2 workgroup, a second
    reduction launch past 128 partials (csrc/common.h reduce_rows_two_stage)."""
    P, K = B * Cc, W // 2 + 1
    cd = lambda a, b: (a + b - 1) // b
    lb, xb, mf, mp = cd(K, l_block), cd(W, x_block), cd(P * H, 64), cd(H, 64)
    g2 = P * mp * lb
    red = 2 if g2 > 128 else 1
    sec, total = _sections(*([4 * W * K] * 4), *([4 * H * H] * 2), *([8 * P * H * K] * 2), 4 * g2, 4 * 32)
    return {"planes": P, "K": K, "tile_m": 64, "tile_k": 16, "l_block": l_block, "l_blocks": lb, "x_block": x_block,
            "x_blocks": xb, "m_tiles_folded": mf, "m_tiles_plane": mp, "grid_tables": cd(W * K + H * H, 256),
            "grid_stage1": mf * lb, "grid_stage2": g2, "grid_stage3": g2 if want_grad else 0,
            "grid_stage4": mf * xb if want_grad else 0, "block": 256, "partials": g2, "reduce_launches": red,
            "launches": 3 + red + (2 if want_grad else 0), "sections": sec, "workspace": total}


# shape -> (l block width, x block width): the widths (48 / 64 / 80 columns) that pad K and W the least, the wider on a tie
PINNED = {(1, 3, 15, 21): (48, 48), (2, 3, 128, 128): (80, 64), (1, 1, 512, 512): (48, 64), (32, 3, 256, 256): (48, 64)}


@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("shape", list(PINNED))
def test_plan_is_pinned_without_gpu(lib, shape, want_grad):
    from image_restoration_amd import ops
    plan = ops.fft_l1_plan(*shape, torch.bfloat16, want_grad)
    assert plan == _expected_plan(*shape, *PINNED[shape], want_grad)
    assert plan == ops.fft_l1_plan(*shape, torch.float32, want_grad)           # the dtype picks an instantiation, not a plan
    assert plan["l_blocks"] * plan["l_block"] >= plan["K"] and plan["x_blocks"] * plan["x_block"] >= shape[3]
    spans = sorted(plan["sections"].values())
    assert all(o % 256 == 0 for o, _ in spans)
    assert all(o0 + b0 <= o1 for (o0, b0), (o1, _) in zip(spans, spans[1:])), "workspace sections overlap"
    # a few absolute figures, so that the helper above cannot drift with the code
    if shape == (32, 3, 256, 256):
        assert (plan["grid_stage1"], plan["grid_stage2"], plan["grid_stage4"]) == (1152, 1152, 1536 if want_grad else 0)
        assert plan["launches"] == (7 if want_grad else 5) and plan["workspace"] == 51782400
    if shape == (1, 3, 15, 21):
        assert plan["launches"] == (6 if want_grad else 4) and plan["workspace"] == 14848 and plan["K"] == 11


def test_cpu_tensors_are_refused_and_old_signature_stays(lib):
    from image_restoration_amd.losses import FFTLoss
    old = FFTLoss(0.5, "mean")
    assert old.loss_weight == 0.5 and old.native is False and FFTLoss().native is False
    with pytest.raises(RuntimeError, match="MI355X only"):
        FFTLoss(native=True)(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        FFTLoss(reduction="sum", native=True)


# --------------------------------------------------------------------------- inputs built from their spectrum
def _structural(H, W):
    """Mask [H, K] of the bins whose imaginary part is identically zero for real input."""
    K = W // 2 + 1
    m = torch.zeros(H, K, dtype=torch.bool)
    ks = [0] + ([H // 2] if H % 2 == 0 else [])
    ls = [0] + ([W // 2] if W % 2 == 0 else [])
    for k in ks:
        for l in ls:
            m[k, l] = True
    return m


@functools.lru_cache(maxsize=None)
def _case(shape, dtype=torch.float32, seed=0, same_plane=-1):
    """pred / target (in `dtype`) whose difference has a spectrum with every non-structural |Re|, |Im| in [1, 2] (before
    rounding), and the fp64 reference loss (loss_weight 1) and gradient on the ROUNDED inputs.  same_plane >= 0: that plane
    (of B*C) has pred == target.  Shared by the tests below and never modified."""
    B, Cc, H, W = shape
    K = W // 2 + 1
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    mag = lambda: (1.0 + torch.rand((B, Cc, H, K), generator=g, dtype=torch.float64)) * \
        (torch.randint(0, 2, (B, Cc, H, K), generator=g).double() * 2 - 1)
    Z = torch.complex(mag(), mag())
    self_conj = [0] + ([H // 2] if H % 2 == 0 else [])
    for l in [0] + ([W // 2] if W % 2 == 0 else []):
        for k in range(H // 2 + 1, H):
            Z[..., k, l] = Z[..., (-k) % H, l].conj()
        for k in self_conj:
            Z[..., k, l] = torch.complex(Z[..., k, l].real, torch.zeros_like(Z[..., k, l].real))
    d = torch.fft.irfft2(Z, s=(H, W))
    target = torch.rand((B, Cc, H, W), generator=g, dtype=torch.float64)
    pred = (target + d).to(dtype)
    target = target.to(dtype)
    if same_plane >= 0:
        pred.view(B * Cc, H, W)[same_plane] = target.view(B * Cc, H, W)[same_plane]
    # the rounded inputs still keep every non-structural coefficient away from zero
    spec = torch.fft.rfft2(pred.double() - target.double())
    keep = torch.ones(B * Cc, dtype=torch.bool)
    if same_plane >= 0:
        keep[same_plane] = False
    spec = spec.view(B * Cc, H, K)[keep]
    free_im = spec.imag.abs()[:, ~_structural(H, W)]                  # (empty at 2 x 2: every bin is structural there)
    floor = min([float(spec.real.abs().min())] + ([float(free_im.min())] if free_im.numel() else []))
    p = pred.double().requires_grad_(True)
    ref = T.fft_loss(p, target.double(), 1.0)
    ref.backward()
    return pred, target, float(ref.detach()), p.grad.detach(), floor


def _native(pred, target, loss_weight=1.0):
    from image_restoration_amd.losses import FFTLoss
    dev = torch.device("cuda:0")
    p = pred.to(dev).requires_grad_(True)
    out = FFTLoss(loss_weight=loss_weight, native=True)(p, target.to(dev))
    out.backward()
    return out.item(), p.grad


def _check(shape, dtype, loss_tol, grad_tol, seed=0):
    pred, target, ref, dref, floor = _case(shape, dtype, seed)
    print(f"{shape} {dtype}: smallest non-structural coefficient {floor:.4f}")
    assert floor >= 0.5
    loss, grad = _native(pred, target)
    assert grad.dtype == dtype and grad.shape == pred.shape
    e_loss = abs(loss - ref) / max(1.0, abs(ref))
    e_grad = float((grad.double().cpu() - dref).norm() / dref.norm())
    print(f"{shape} {dtype}: loss error {e_loss:.3e}, relative gradient error {e_grad:.3e}")
    assert e_loss <= loss_tol
    assert e_grad <= grad_tol


# --------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_native_fft_loss_against_reference_golden():
    """FFTLoss(native=True) against what the reference's FFTLoss class produced, at the bars the rocFFT path is held to."""
    z = np.load(os.path.join(GOLD, "fft_loss.npz"))
    for name in ("a", "b", "c", "odd"):
        lw = float(z[name + "_args"][4])
        loss, grad = _native(torch.from_numpy(z[name + "_pred"]).float(), torch.from_numpy(z[name + "_target"]).float(), lw)
        gl, gd = float(z[name + "_loss"]), torch.from_numpy(z[name + "_dpred"]).double()
        e_loss, e_grad = abs(loss - gl) / max(1.0, abs(gl)), float((grad.double().cpu() - gd).norm() / gd.norm())
        print(f"golden {name}: loss error {e_loss:.3e}, relative gradient error {e_grad:.3e}")
        assert e_loss <= 1e-4, name
        assert e_grad <= 1e-4, name


SEAMS = [(1, 1, 2, 2), (1, 2, 15, 21), (1, 3, 37, 50), (7, 1, 16, 32), (2, 3, 96, 160), (1, 3, 128, 128), (1, 1, 256, 256),
         (1, 1, 512, 512), (1, 1, 511, 509)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SEAMS, ids=lambda s: "x".join(map(str, s)))
def test_native_fft_loss_at_tile_seams_vs_fp64(shape):
    _check(shape, torch.float32, 1e-4, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 24, 40), (1, 3, 37, 50)], ids=lambda s: "x".join(map(str, s)))
def test_native_fft_loss_bf16_vs_fp64(shape):
    _check(shape, torch.bfloat16, 2e-3, 2e-2)


@pytest.mark.gpu
def test_native_agrees_with_the_rocfft_path():
    from image_restoration_amd.losses import FFTLoss
    pred, target, _, _, floor = _case((2, 3, 64, 96))
    assert floor >= 0.5
    dev = torch.device("cuda:0")
    loss, grad = _native(pred, target, 0.1)
    p = pred.to(dev).requires_grad_(True)
    old = FFTLoss(loss_weight=0.1)(p, target.to(dev))
    old.backward()
    assert abs(loss - old.item()) <= 1e-4 * max(1.0, abs(old.item()))
    assert float((grad - p.grad).norm()) <= 1e-4 * float(p.grad.norm())


@pytest.mark.gpu
def test_native_autograd_plumbing():
    from image_restoration_amd import ops
    from image_restoration_amd.losses import FFTLoss
    dev = torch.device("cuda:0")
    pred, target, _, _, _ = _case((1, 2, 15, 21))
    loss, grad = _native(pred, target, 0.7)
    p, t = pred.to(dev).requires_grad_(True), target.to(dev).requires_grad_(True)
    fn = FFTLoss(loss_weight=0.7, native=True)
    out = fn(p, t)
    assert out.item() == loss
    (3 * out).backward()
    assert torch.equal(p.grad, 3 * grad)
    assert torch.equal(t.grad, -p.grad)
    # a target that alone needs a gradient
    t2 = target.to(dev).requires_grad_(True)
    fn(pred.to(dev), t2).backward()
    assert torch.equal(t2.grad, -grad)
    # no gradient wanted: the adjoint stages are skipped, the loss is the same bit for bit
    with torch.no_grad():
        assert fn(pred.to(dev), target.to(dev)).item() == loss
    assert fn(pred.to(dev), target.to(dev)).item() == loss
    l0, d0 = ops.fft_l1_loss(pred.to(dev), target.to(dev), 0.7, want_grad=False)
    l1, d1 = ops.fft_l1_loss(pred.to(dev), target.to(dev), 0.7, want_grad=True)
    assert d0 is None and l0.item() == l1.item() == loss and torch.equal(d1, grad)
    # mixed dtypes are widened to fp32
    mixed = fn(pred.to(dev).bfloat16(), target.to(dev))
    both32 = fn(pred.to(dev).bfloat16().float(), target.to(dev))
    assert mixed.item() == both32.item()
    with pytest.raises(TypeError):
        ops.fft_l1_loss(pred.to(dev).bfloat16(), target.to(dev))
    with pytest.raises(RuntimeError, match="outside the supported"):
        fn(torch.zeros(1, 1, 513, 8, device=dev), torch.zeros(1, 1, 513, 8, device=dev))


@pytest.mark.gpu
def test_native_exact_zeros():
    dev = torch.device("cuda:0")
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.rand((2, 3, 24, 40), generator=torch.Generator().manual_seed(3)).to(dtype)
        loss, grad = _native(x, x.clone())
        assert loss == 0.0 and grad.dtype == dtype and not grad.any()
    # one identical plane among others: its gradient is exactly zero, the rest match the reference
    shape, same = (2, 3, 24, 40), 4
    pred, target, ref, dref, floor = _case(shape, torch.float32, 0, same)
    assert floor >= 0.5 and not dref.view(6, 24, 40)[same].any()
    loss, grad = _native(pred, target)
    assert not grad.view(6, 24, 40)[same].any()
    assert abs(loss - ref) <= 1e-4 * max(1.0, abs(ref))
    assert float((grad.double().cpu() - dref).norm()) <= 1e-4 * float(dref.norm())


@pytest.mark.gpu
def test_native_is_bitwise_reproducible():
    pred, target, _, _, _ = _case((2, 3, 96, 160))
    l0, g0 = _native(pred, target)
    l1, g1 = _native(pred, target)
    assert l0 == l1 and torch.equal(g0, g1)


@pytest.mark.gpu
def test_native_takes_a_non_contiguous_view():
    from image_restoration_amd.losses import FFTLoss
    dev = torch.device("cuda:0")
    pred, target, _, _, _ = _case((1, 3, 37, 50))
    wide = torch.zeros((1, 6, 37, 50), device=dev)
    wide[:, ::2] = pred.to(dev)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    fn = FFTLoss(native=True)
    v = view.requires_grad_(True)
    out = fn(v, target.to(dev))
    out.backward()
    loss, grad = _native(pred, target)
    assert out.item() == loss and torch.equal(v.grad, grad)
