"""The pixel-space loss terms on native kernels (csrc/losses.hip: mi_ssim_loss, mi_edge_loss, mi_focal_l1_loss; losses.SSIMloss,
SSIM, EdgeLoss, FocalL1Loss) against fp64 restatements written here as plain torch on the CPU, gradients by autograd.

The EdgeLoss and FocalL1Loss restatements are pinned on the reference's own classes (tests/golden/pixel_losses.npz,
tools/capture_golden_losses.py).  The SSIM restatement is pytorch_msssim.ssim with its defaults written out; that package is
not installed, so it stays unpinned, and its closed-form gradient (the one the kernel implements) is checked against autograd.

GPU inputs are drawn in fp64, rounded to the case's dtype and handed to the oracle as those rounded values: what is left is
fp32 arithmetic and the rounding of dpred.  Bars: edge and focal in fp32 hold the bars of tests/test_train_tail.py (1e-4
relative on the loss, 1e-4 on |dpred - oracle| / |oracle|); SSIM in fp32 holds 1e-4 * loss_weight ABSOLUTE on the loss (1 - m
cancels; fp32 torch on the CPU is off by 1.1e-5 on the hardest input here) and 3e-4 on the gradient norm; bf16 holds the bars
of test_losses_on_gpu_against_oracle (2e-3 on the loss - absolute, times loss_weight, for SSIM - and 2e-2 on the gradient
norm: storing dpred in bf16 alone costs 1.7e-3)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pixel_losses.npz")
F64 = torch.float64
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
BARS = {"f32": (1e-4, 1e-4), "bf16": (2e-3, 2e-2)}                  # (loss, gradient norm)
SSIM_BARS = {"f32": (1e-4, 3e-4), "bf16": (2e-3, 2e-2)}             # (loss: absolute, per unit of loss_weight; gradient norm)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


# --------------------------------------------------------------------------- fp64 restatements
@functools.lru_cache(None)
def _blur5():
    k = torch.tensor([[.05, .25, .4, .25, .05]])           # fp32, and the outer product taken in fp32, as the reference builds it
    return torch.matmul(k.t(), k).to(F64)


def _conv_gauss(img):
    c = img.shape[1]
    return F.conv2d(F.pad(img, (2, 2, 2, 2), mode="replicate"), _blur5().expand(c, 1, 5, 5), groups=c)


def laplacian_ref(x):
    z = torch.zeros_like(x)
    z[:, :, ::2, ::2] = 4 * _conv_gauss(x)[:, :, ::2, ::2]
    return x - _conv_gauss(z)


def edge_ref(pred, target, loss_weight=1.0, criterion="l2"):
    e = laplacian_ref(pred) - laplacian_ref(target)
    return loss_weight * (e.abs().mean() if criterion == "l1" else (e * e).mean())


def focal_ref(pred, target, gamma=2.0, epsilon=1e-6, alpha=0.1):
    a = (pred - target).abs() / alpha
    return (torch.log1p(a + epsilon) ** gamma * a).mean()


@functools.lru_cache(None)
def _window():
    g = torch.exp(-(torch.arange(11, dtype=F64) - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def _win_valid(x):
    c, g = x.shape[1], _window()
    x = F.conv2d(x, g.view(1, 1, 11, 1).expand(c, 1, 11, 1), groups=c)
    return F.conv2d(x, g.view(1, 1, 1, 11).expand(c, 1, 1, 11), groups=c)


def _win_full(m):
    """The zero-extended correlation with the same window: the adjoint of _win_valid."""
    c, g = m.shape[1], _window()
    m = F.conv_transpose2d(m, g.view(1, 1, 11, 1).expand(c, 1, 11, 1), groups=c)
    return F.conv_transpose2d(m, g.view(1, 1, 1, 11).expand(c, 1, 1, 11), groups=c)


def _ssim_parts(x, y, data_range):
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = _win_valid(x), _win_valid(y)
    s1, s2, s12 = _win_valid(x * x) - mu1 * mu1, _win_valid(y * y) - mu2 * mu2, _win_valid(x * y) - mu1 * mu2
    A1, A2, B1, B2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    return mu1, mu2, A1, A2, B1, B2, A1 * A2 / (B1 * B2)


def ssim_ref(pred, target, data_range=1.0):
    """Mean SSIM as pytorch_msssim.ssim computes it with its defaults (11-tap Gaussian, sigma 1.5, valid, per channel)."""
    return _ssim_parts(pred, target, data_range)[-1].mean()


def ssim_mean_grad_closed(pred, target, data_range=1.0):
    """d (mean SSIM) / d pred in the closed form the kernel implements (include/mi_restore.h)."""
    mu1, mu2, A1, A2, B1, B2, S = _ssim_parts(pred, target, data_range)
    dmu = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * S / B1
    dsg, ds12 = -S / B2, 2 * A1 / (B1 * B2)
    ga, gb, gc = dmu - 2 * mu1 * dsg - mu2 * ds12, 2 * dsg, ds12
    return (_win_full(ga) + pred * _win_full(gb) + target * _win_full(gc)) / S.numel()


def _with_grad(fn, pred, *args, **kw):
    p = pred.clone().requires_grad_(True)
    loss = fn(p, *args, **kw)
    loss.backward()
    return float(loss.detach()), p.grad


def _rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-300))


# --------------------------------------------------------------------------- CPU: the restatements
def _golden_cases():
    z = np.load(GOLD)
    for name in sorted(k[:-5] for k in z.files if k.endswith("/loss")):
        shape, prec, kind = name.split("/")
        yield name, shape, prec, kind


GOLDEN = list(_golden_cases())
EDGE_KINDS = {"edge_l2_w1": ("l2", 1.0), "edge_l1_w1": ("l1", 1.0), "edge_l2_w005": ("l2", 0.05), "edge_l1_w005": ("l1", 0.05)}
FOCAL_KINDS = {"focal_default": (2.0, 1e-6, 0.1), "focal_cgir": (0.5, 1e-6, 1.0)}


def _golden(name, shape):
    z = np.load(GOLD)
    return (torch.from_numpy(z[shape + "/pred"]).to(F64), torch.from_numpy(z[shape + "/target"]).to(F64), float(z[name + "/loss"]),
            torch.from_numpy(z[name + "/dpred"]).to(F64))


def _oracle_of_kind(kind, pred, target):
    if kind in EDGE_KINDS:
        crit, lw = EDGE_KINDS[kind]
        return _with_grad(edge_ref, pred, target, lw, crit)
    return _with_grad(focal_ref, pred, target, *FOCAL_KINDS[kind])


def test_golden_file_holds_every_kind_in_both_precisions():
    kinds = {(prec, kind) for _, _, prec, kind in GOLDEN}
    assert kinds == {(p, k) for p in ("f64", "f32") for k in list(EDGE_KINDS) + list(FOCAL_KINDS)}
    assert {s for _, s, _, _ in GOLDEN} == {"2x3x16x16", "1x3x15x21", "1x3x24x40"}
    assert os.path.getsize(GOLD) < 200 * 1024


@pytest.mark.parametrize("name,shape,prec,kind", GOLDEN, ids=[g[0] for g in GOLDEN])
def test_restatements_reproduce_the_reference_classes(name, shape, prec, kind):
    pred, target, loss, dpred = _golden(name, shape)
    got, grad = _oracle_of_kind(kind, pred, target)
    tol = 1e-12 if prec == "f64" else 1e-5
    assert abs(got - loss) <= tol * abs(loss), (got, loss)
    assert _rel(grad, dpred) <= tol
    if prec == "f64":
        assert float((grad - dpred).abs().max()) <= tol * float(dpred.abs().max())


@pytest.mark.parametrize("shape,data_range", [((1, 1, 11, 11), 1.0), ((2, 3, 19, 27), 1.0), ((1, 2, 24, 13), 255.0)])
def test_ssim_closed_form_gradient_is_autograd_of_the_restatement(shape, data_range):
    g = torch.Generator().manual_seed(7)
    target = torch.rand(shape, generator=g, dtype=F64) * data_range
    pred = (target + 0.05 * data_range * torch.randn(shape, generator=g, dtype=F64))
    _, auto = _with_grad(ssim_ref, pred, target, data_range)
    closed = ssim_mean_grad_closed(pred, target, data_range)
    assert float((closed - auto).abs().max()) <= 1e-10 * float(auto.abs().max())


# --------------------------------------------------------------------------- CPU: the ABI surface
def test_workspace_queries_without_gpu(lib):
    L = lib.lib()
    for shape in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, -1), (-2, 3, 16, 16)):
        assert L.mi_ssim_loss_workspace(*shape) == 0 and L.mi_edge_loss_workspace(*shape) == 0, shape
    assert L.mi_focal_l1_workspace(0) == 0 and L.mi_focal_l1_workspace(-5) == 0
    for shape in ((1, 1, 11, 11), (1, 3, 11, 40), (2, 3, 43, 75), (32, 3, 256, 256)):
        n = L.mi_ssim_loss_workspace(*shape)
        B, Cc, H, W = shape
        assert n > 0 and n % 256 == 0 and n >= 3 * 4 * B * Cc * (H - 10) * (W - 10), shape
    for shape in ((1, 1, 2, 3), (1, 3, 5, 5), (2, 3, 37, 40), (32, 3, 256, 256)):
        n = L.mi_edge_loss_workspace(*shape)
        assert n > 0 and n % 256 == 0 and n >= 4 * int(np.prod(shape)), shape
    for n in (1, 63, 64 * 1024 + 5, 2 ** 33):
        w = L.mi_focal_l1_workspace(n)
        assert w > 0 and w % 256 == 0
    for shape in ((1, 3, 10, 40), (1, 3, 40, 10), (1, 3, 10, 10)):
        assert L.mi_ssim_loss_workspace(*shape) == 0, shape
    assert L.mi_edge_loss_workspace(1, 3, 1, 8) == 0 and L.mi_edge_loss_workspace(1, 3, 8, 1) == 0
    header = open(os.path.join(ROOT, "include", "mi_restore.h")).read()
    assert int(re.search(r"#define MI_SSIM_TILE (\d+)", header).group(1)) == lib.MI_SSIM_TILE


def test_argument_refusals_without_gpu(lib):
    """Every refusal returns < 0 with a message before anything is launched: the host buffers standing in for device memory
    are never touched."""
    L = lib.lib()
    buf = [C.create_string_buffer(64) for _ in range(5)]
    pred, target, dpred, loss, ws = [C.cast(b, C.c_void_p) for b in buf]
    ptrs = dict(pred=pred, target=target, dpred=dpred, loss=loss, ws=ws)

    def ssim(**kw):
        a = {**dict(ptrs, B=1, C=1, H=11, W=11, lw=1.0, dr=1.0, dtype=lib.MI_F32), **kw}
        return L.mi_ssim_loss(a["pred"], a["target"], a["dpred"], a["loss"], a["B"], a["C"], a["H"], a["W"], a["lw"], a["dr"],
                              a["dtype"], a["ws"], None), L.mi_last_error()

    def edge(**kw):
        a = {**dict(ptrs, B=1, C=1, H=4, W=4, lw=1.0, crit=0, dtype=lib.MI_F32), **kw}
        return L.mi_edge_loss(a["pred"], a["target"], a["dpred"], a["loss"], a["B"], a["C"], a["H"], a["W"], a["lw"], a["crit"],
                              a["dtype"], a["ws"], None), L.mi_last_error()

    def focal(**kw):
        a = {**dict(ptrs, n=4, gamma=2.0, eps=1e-6, alpha=0.1, scale=1.0, dtype=lib.MI_F32), **kw}
        return L.mi_focal_l1_loss(a["pred"], a["target"], a["dpred"], a["loss"], a["n"], a["gamma"], a["eps"], a["alpha"],
                                  a["scale"], a["dtype"], a["ws"], None), L.mi_last_error()

    for call in (ssim, edge, focal):
        for name in ("pred", "target", "loss", "ws"):
            rc, msg = call(**{name: None})
            assert rc < 0 and b"null pointer" in msg, (call.__name__, name)
        rc, msg = call(dtype=7)
        assert rc < 0 and b"bad dtype 7" in msg, call.__name__
    for call, kw in ((ssim, dict(B=0)), (edge, dict(B=0)), (ssim, dict(C=0)), (edge, dict(C=-1)), (focal, dict(n=0)),
                     (ssim, dict(H=10)), (ssim, dict(W=10)), (ssim, dict(dr=0.0)), (edge, dict(W=1)), (edge, dict(H=1)),
                     (edge, dict(crit=2)), (edge, dict(crit=-1)), (focal, dict(alpha=0.0)), (focal, dict(alpha=-0.1)),
                     (focal, dict(gamma=-1.0))):
        rc, msg = call(**kw)
        assert rc < 0 and len(msg) > 0, (call.__name__, kw)
    assert b"criterion" in edge(crit=2)[1] and b"alpha" in focal(alpha=0.0)[1] and b"window" in ssim(H=10)[1]
    assert all(b.raw == bytes(64) for b in buf)


def test_modules_refuse_cpu_tensors_and_other_reductions(lib):
    from image_restoration_amd import losses
    x = torch.zeros(1, 3, 16, 16)
    for mod in (losses.FocalL1Loss(), losses.SSIMloss(), losses.SSIM(), losses.EdgeLoss(), losses.EdgeLoss(criterion="l1"),
                losses.FocalL1Loss(gamma=0.5, alpha=1.0), losses.SSIMloss(loss_weight=0.2, data_range=255.)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            mod(x, x)
    for reduction in ("sum", "none"):
        with pytest.raises(ValueError):
            losses.EdgeLoss(reduction=reduction)
    with pytest.raises(NotImplementedError):
        losses.EdgeLoss(criterion="huber")
    for cls in (losses.SSIMloss, losses.SSIM):
        with pytest.raises(RuntimeError, match="with respect to the target"):
            cls()(x, x.clone().requires_grad_(True))
    # the reference's constructor signatures, positionally
    f, s, e = losses.FocalL1Loss(0.5, 1e-6, 1.0), losses.SSIMloss(0.3, 255.), losses.EdgeLoss(0.05, "l1", "mean")
    assert (f.gamma, f.epsilon, f.alpha, s.loss_weight, s.data_range, e.weight, e.criterion) == (0.5, 1e-6, 1.0, 0.3, 255., 0.05, "l1")


# --------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


def _rounded(t64, dtype):
    """(device tensor in dtype, the same values in fp64 on the host)"""
    t = t64.to(dtype)
    return t.cuda(), t.to(F64)


def _ssim_inputs(kind, shape, data_range, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        target = torch.rand(shape, generator=g, dtype=F64)
        pred = (target + 0.1 * torch.randn(shape, generator=g, dtype=F64)).clamp(0, 1)
    elif kind == "smooth":                                    # a smooth sinusoid image and a slightly noisy prediction
        B, Cc, H, W = shape
        yy, xx = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
        ph = torch.arange(B * Cc, dtype=F64).view(B, Cc, 1, 1)
        target = 0.5 + 0.4 * torch.sin(0.13 * yy + 0.7 * ph) * torch.cos(0.09 * xx - 0.3 * ph)
        pred = target + 0.02 * torch.randn(shape, generator=g, dtype=F64)
    else:                                                     # flat: 0.5 plus sigma = 0.004 noise, the variance terms cancel hardest
        target = 0.5 + 0.004 * torch.randn(shape, generator=g, dtype=F64)
        pred = 0.5 + 0.004 * torch.randn(shape, generator=g, dtype=F64)
    return pred * data_range, target * data_range


def _ssim_cases():
    from image_restoration_amd._lib import MI_SSIM_TILE as T
    return [("one_element", "random", (1, 1, 11, 11), 1.0, 1.0), ("one_row", "random", (1, 3, 11, 40), 1.0, 0.2),
            ("one_column", "random", (1, 3, 40, 11), 255.0, 1.0), ("seams", "random", (2, 3, 43, 75), 1.0, 1.0),
            ("seams_255", "random", (2, 3, 43, 75), 255.0, 0.2),
            ("map_tile_plus_one", "random", (1, 1, T + 11, T + 11), 1.0, 1.0), ("image_tile_plus_one", "random", (1, 2, T + 1, T + 1), 1.0, 0.2),
            ("smooth", "smooth", (2, 3, 64, 64), 1.0, 1.0), ("smooth_255", "smooth", (2, 3, 64, 64), 255.0, 0.2),
            ("flat", "flat", (2, 3, 64, 64), 1.0, 1.0), ("flat_255", "flat", (2, 3, 64, 64), 255.0, 0.2)]


SSIM_CASES = _ssim_cases()


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", SSIM_CASES, ids=[c[0] for c in SSIM_CASES])
def test_ssim_against_fp64(lib, case, dt):
    from image_restoration_amd import losses, ops
    _, kind, shape, data_range, lw = case
    p64, t64 = _ssim_inputs(kind, shape, data_range, seed=11)
    (pred, p64), (target, t64) = _rounded(p64, DTYPES[dt]), _rounded(t64, DTYPES[dt])
    m, dm = _with_grad(ssim_ref, p64, t64, data_range)
    bar_l, bar_g = SSIM_BARS[dt]
    out, dpred = ops.ssim_loss(pred, target, lw, data_range)
    out = out.double().cpu()
    err_l, err_m, err_g = abs(float(out[0]) - lw * (1 - m)), abs(float(out[1]) - m), _rel(dpred, -lw * dm)
    print(f"ssim {case[0]} {dt}: m {m:.6f} |loss err| {err_l:.2e} |m err| {err_m:.2e} grad {err_g:.2e}")
    assert dpred.dtype == DTYPES[dt] and bool(torch.isfinite(dpred).all())
    assert err_l <= bar_l * lw and err_m <= bar_l and err_g <= bar_g
    # the modules: SSIMloss is loss[0] with that gradient, SSIM is loss_weight * m with the negative of it
    pa, pb = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    la, lb = losses.SSIMloss(lw, data_range)(pa, target), losses.SSIM(lw, data_range)(pb, target)
    la.backward()
    lb.backward()
    assert torch.equal(la.detach(), out[0].float().cuda()) and torch.equal(pa.grad, dpred) and torch.equal(pb.grad, -dpred)
    assert abs(float(lb.detach()) - lw * m) <= bar_l * lw


# uniform inputs rounded to bf16 (exact in fp32 too); for these seeds no element of the oracle's Laplacian difference is within
# 1e-5 of zero, so sign() is the same in every precision and a flipped sign is a kernel error
EDGE_SHAPES = {(1, 1, 2, 3): 0, (1, 3, 5, 5): 0, (2, 3, 37, 40): 4, (1, 3, 64, 65): 0, (1, 2, 33, 130): 4}      # shape: seed


def _edge_inputs(shape):
    torch.manual_seed(EDGE_SHAPES[shape])
    return torch.rand(shape, dtype=F64).to(torch.bfloat16).to(F64), torch.rand(shape, dtype=F64).to(torch.bfloat16).to(F64)


def _check_edge(ops, pred, target, p64, t64, lw, crit, dt, what):
    if crit == "l1":
        e = laplacian_ref(p64) - laplacian_ref(t64)
        assert float(e.abs().min()) > 1e-5, "the case's seed leaves an element of e at zero: choose another"
    want, dwant = _with_grad(edge_ref, p64, t64, lw, crit)
    loss, dpred = ops.edge_loss(pred, target, lw, crit)
    err_l, err_g = abs(float(loss) - want) / abs(want), _rel(dpred, dwant)
    print(f"edge {what} {crit} {dt}: loss {want:.6e} rel err {err_l:.2e} grad {err_g:.2e}")
    assert dpred.dtype == pred.dtype and err_l <= BARS[dt][0] and err_g <= BARS[dt][1]


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("crit,lw", [("l2", 1.0), ("l1", 0.05)])
@pytest.mark.parametrize("shape", list(EDGE_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_edge_against_fp64(lib, shape, crit, lw, dt):
    from image_restoration_amd import ops
    p64, t64 = _edge_inputs(shape)
    (pred, p64), (target, t64) = _rounded(p64, DTYPES[dt]), _rounded(t64, DTYPES[dt])
    _check_edge(ops, pred, target, p64, t64, lw, crit, dt, "x".join(map(str, shape)))


EDGE_GOLDEN = [g for g in GOLDEN if g[3] in EDGE_KINDS]
FOCAL_GOLDEN = [g for g in GOLDEN if g[3] in FOCAL_KINDS]


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name,shape,prec,kind", EDGE_GOLDEN, ids=[g[0] for g in EDGE_GOLDEN])
def test_edge_against_the_reference_goldens(lib, name, shape, prec, kind, dt):
    """The golden inputs sit on a 2^-8 grid: exact in bf16 and fp32, so both dtypes start from the reference's own numbers."""
    from image_restoration_amd import ops
    p64, t64, loss, dpred = _golden(name, shape)
    crit, lw = EDGE_KINDS[kind]
    got, grad = ops.edge_loss(p64.to(DTYPES[dt]).cuda(), t64.to(DTYPES[dt]).cuda(), lw, crit)
    assert abs(float(got) - loss) <= BARS[dt][0] * abs(loss) and _rel(grad, dpred) <= BARS[dt][1]


@gpu
def test_edge_border_adjoint(lib):
    """An impulse at each corner and at one edge midpoint of a 9 x 9 plane: the 'l2' gradient, 2/N L^T L d, to 1e-6 absolute.
    A wrong adjoint of the replicate padding (the taps clamped onto a border pixel) shows here."""
    from image_restoration_amd import ops
    for y, x in ((0, 0), (0, 8), (8, 0), (8, 8), (0, 4), (4, 8)):
        p64, t64 = torch.zeros(1, 1, 9, 9, dtype=F64), torch.zeros(1, 1, 9, 9, dtype=F64)
        p64[0, 0, y, x] = 1.0
        want, dwant = _with_grad(edge_ref, p64, t64, 1.0, "l2")
        loss, dpred = ops.edge_loss(p64.float().cuda(), t64.float().cuda(), 1.0, "l2")
        assert float((dpred.double().cpu() - dwant).abs().max()) <= 1e-6, (y, x)
        assert abs(float(loss) - want) <= 1e-4 * want


FOCAL_PARAMS = [(2.0, 0.1), (0.5, 1.0), (1.0, 0.5)]
FOCAL_SHAPES = [(1,), (63,), (64 * 1024 + 5,), (2, 3, 37, 40)]


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("gamma,alpha", FOCAL_PARAMS)
@pytest.mark.parametrize("shape", FOCAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_focal_against_fp64(lib, shape, gamma, alpha, dt):
    from image_restoration_amd import ops
    g = torch.Generator().manual_seed(3)
    t64 = torch.rand(shape, generator=g, dtype=F64)
    p64 = torch.rand(shape, generator=g, dtype=F64)
    tie = (torch.arange(t64.numel()) % 10 == 9).view(shape)           # exact ties on a tenth of the elements
    p64 = torch.where(tie, t64, p64)
    (pred, p64), (target, t64) = _rounded(p64, DTYPES[dt]), _rounded(t64, DTYPES[dt])
    want, dwant = _with_grad(focal_ref, p64, t64, gamma, 1e-6, alpha)
    loss, dpred = ops.focal_l1_loss(pred, target, gamma, 1e-6, alpha)
    err_l, err_g = abs(float(loss) - want) / abs(want), _rel(dpred, dwant)
    print(f"focal {shape} gamma {gamma} alpha {alpha} {dt}: loss {want:.6e} rel err {err_l:.2e} grad {err_g:.2e}")
    assert bool(torch.isfinite(dpred).all()) and bool((dpred.cpu()[p64 == t64] == 0).all())
    assert bool((dwant[tie] == 0).all())
    assert err_l <= BARS[dt][0] and err_g <= BARS[dt][1]
    half, dhalf = ops.focal_l1_loss(pred, target, gamma, 1e-6, alpha, scale=0.5)            # scale folds into both
    assert abs(float(half) - 0.5 * want) <= BARS[dt][0] * 0.5 * want and _rel(dhalf, 0.5 * dwant) <= BARS[dt][1]


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name,shape,prec,kind", FOCAL_GOLDEN, ids=[g[0] for g in FOCAL_GOLDEN])
def test_focal_against_the_reference_goldens(lib, name, shape, prec, kind, dt):
    from image_restoration_amd import ops
    p64, t64, loss, dpred = _golden(name, shape)
    got, grad = ops.focal_l1_loss(p64.to(DTYPES[dt]).cuda(), t64.to(DTYPES[dt]).cuda(), *FOCAL_KINDS[kind])
    assert abs(float(got) - loss) <= BARS[dt][0] * abs(loss) and _rel(grad, dpred) <= BARS[dt][1]


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
def test_bitwise_reproducible_and_the_loss_without_a_gradient(lib, dt):
    from image_restoration_amd import ops
    g = torch.Generator().manual_seed(5)
    shape = (2, 3, 43, 75)
    pred, target = torch.rand(shape, generator=g).to(DTYPES[dt]).cuda(), torch.rand(shape, generator=g).to(DTYPES[dt]).cuda()
    for fn in (lambda **k: ops.ssim_loss(pred, target, 0.2, 1.0, **k), lambda **k: ops.edge_loss(pred, target, 0.05, "l2", **k),
               lambda **k: ops.edge_loss(pred, target, 1.0, "l1", **k), lambda **k: ops.focal_l1_loss(pred, target, 0.5, 1e-6, 1.0, **k)):
        l0, d0 = fn()
        l0, d0 = l0.clone(), d0.clone()
        l1, d1 = fn()
        assert torch.equal(l0, l1) and torch.equal(d0, d1)
        l2, d2 = fn(want_grad=False)
        assert d2 is None and torch.equal(l0, l2)


@gpu
def test_modules_under_autograd(lib):
    """0.3 SSIMloss + 0.05 EdgeLoss + FocalL1Loss + L1Loss on one prediction in bf16, against the fp64 oracle of the same sum;
    then one mixed-dtype call (bf16 prediction, fp32 target), which runs the fp32 path."""
    from image_restoration_amd import losses
    g = torch.Generator().manual_seed(9)
    shape = (2, 3, 32, 32)
    t64 = torch.rand(shape, generator=g, dtype=F64)
    p64 = (t64 + 0.1 * torch.randn(shape, generator=g, dtype=F64)).clamp(0, 1)
    (pred, p64), (target, t64) = _rounded(p64, torch.bfloat16), _rounded(t64, torch.bfloat16)
    terms = (losses.SSIMloss(0.3), losses.EdgeLoss(0.05), losses.FocalL1Loss(), losses.L1Loss())

    def oracle(p):
        return 0.3 * (1 - ssim_ref(p, t64)) + edge_ref(p, t64, 0.05, "l2") + focal_ref(p, t64) + (p - t64).abs().mean()

    want, dwant = _with_grad(oracle, p64)
    p = pred.clone().requires_grad_(True)
    loss = sum(m(p, target) for m in terms)
    loss.backward()
    assert p.grad.dtype == torch.bfloat16
    assert abs(float(loss.detach()) - want) <= BARS["bf16"][0] * abs(want) and _rel(p.grad, dwant) <= BARS["bf16"][1]
    # a target that asks for a gradient gets the negative (focal, edge)
    tq, pq = target.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    (losses.EdgeLoss(0.05, "l1")(pq, tq) + losses.FocalL1Loss(0.5, 1e-6, 1.0)(pq, tq)).backward()
    assert torch.equal(tq.grad, -pq.grad)
    # mixed dtypes: both are widened to fp32
    for mod in terms[:3]:
        pm, pf = pred.clone().requires_grad_(True), pred.float().requires_grad_(True)
        lm, lf = mod(pm, target.float()), mod(pf, target.float())
        lm.backward()
        lf.backward()
        assert torch.equal(lm, lf) and pm.grad.dtype == torch.bfloat16 and torch.equal(pm.grad, pf.grad.to(torch.bfloat16))
