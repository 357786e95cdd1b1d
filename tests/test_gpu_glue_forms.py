"""The 3x3 U-Net glue bit for bit: the implicit-GEMM convolution (csrc/conv3x3.hip) and the layout kernels (csrc/glue.hip) on the
case tables of tests/glue_forms.py.  Every case first asserts from the plan query that the call reaches the instance, the loop
state and the alignment form its row names, then runs the kernel on small integers inside NaN-guarded buffers and compares with
torch.equal against F.conv2d / F.conv_transpose2d / autograd in float64, F.pad + slicing, F.pixel_shuffle / F.pixel_unshuffle and
plain indexing.  No comparison here carries a tolerance."""
import pytest
import torch
import torch.nn.functional as F

import glue_forms as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(table, r):
    from image_restoration_amd import ops
    c = T.BUILD[table](ops, r, DEV)
    T.reach(ops, r, getattr(c, "aligned", None))
    T.RUN[table](ops, c)
    torch.cuda.synchronize()
    c.check()
    return c


@pytest.mark.parametrize("r", T.CONV_CASES, ids=T.case_id)
def test_conv3x3_forward_and_data_gradient_exact(r):
    """All nine c3_kernel<MT, TWP> at every tile seam, height, chunk count, channel tail, batch, epilogue; transpose=True rows run
    the same kernels on the flipped, transposed pack."""
    _run("conv", r)


@pytest.mark.parametrize("r", T.WGRAD_CASES, ids=T.case_id)
def test_conv3x3_weight_gradient_exact(r):
    """c3_wgrad_kernel<TWP> with either operand in the 64-row role, every tile / split state; overwrite into NaN, accumulate on an
    integer base."""
    _run("wgrad", r)


@pytest.mark.parametrize("r", T.IM2COL_CASES, ids=T.case_id)
def test_im2col3x3_exact(r):
    _run("im2col", r)


@pytest.mark.parametrize("r", T.COL2IM_CASES, ids=T.case_id)
def test_col2im3x3_exact(r):
    _run("col2im", r)


@pytest.mark.parametrize("r", T.SHUFFLE_CASES, ids=T.case_id)
def test_pixel_shuffle2_exact(r):
    _run("shuffle", r)


@pytest.mark.parametrize("r", T.COPY_CASES, ids=T.case_id)
def test_copy_rows_exact(r):
    _run("copy", r)


MODULE_CASES = [r for r in T.CONV_CASES if T.module_route(r)]


def _module_reference(r):
    """Output and every gradient of conv2d(x; w) (+ bias) (+ residual) under the cotangent dy, float64 autograd on the CPU."""
    h = T._conv_host(r["B"], r["M"], r["K"], r["H"], r["W"], False)
    x, w, b, res = (h[k].double().requires_grad_(True) for k in ("x", "w", "bias", "res"))
    y = F.conv2d(x, w, b if r["bias"] else None, padding=1) + (res if r["res"] else 0)
    y.backward(h["dy"].double())
    ref = {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad if r["bias"] else None, "dres": res.grad if r["res"] else None}
    for k, v in ref.items():
        if v is not None:
            T.precondition(v, torch.float32 if k in ("dw", "db") else torch.bfloat16, f"{T.case_id(r)}: {k}")
    return h, ref


@pytest.mark.parametrize("r", MODULE_CASES, ids=T.case_id)
def test_glue_conv_module_both_routes_exact(r, monkeypatch):
    """restormer._conv2d (the door the models use) on the rows _Conv3x3Fn hands to the implicit GEMM: output, dx, dW, db and the
    residual gradient equal float64 autograd bit for bit, and with MI_NO_CONV3_IMPLICIT=1 the im2col / col2im route (the layout
    kernels around the 1x1 GEMM and the Gram) gives the same bits."""
    from image_restoration_amd import ops, restormer
    h, ref = _module_reference(r)
    T.reach(ops, r)
    for route in ("implicit", "im2col"):
        if route == "im2col":
            monkeypatch.setenv("MI_NO_CONV3_IMPLICIT", "1")
        else:
            monkeypatch.delenv("MI_NO_CONV3_IMPLICIT", raising=False)
        conv = torch.nn.Conv2d(r["K"], r["M"], 3, padding=1, bias=r["bias"])
        with torch.no_grad():
            conv.weight.copy_(h["w"])
            if r["bias"]:
                conv.bias.copy_(h["bias"])
        conv = conv.to(DEV)
        x = h["x"].to(DEV, torch.bfloat16).requires_grad_(True)
        res = h["res"].to(DEV, torch.bfloat16).requires_grad_(True) if r["res"] else None
        y = restormer._conv2d(x, conv, res)
        y.backward(h["dy"].to(DEV, torch.bfloat16))
        torch.cuda.synchronize()
        got = {"y": y.detach(), "dx": x.grad, "dw": conv.weight.grad, "db": conv.bias.grad if r["bias"] else None,
               "dres": res.grad if r["res"] else None}
        for k, want in ref.items():
            if want is None:
                continue
            g = got[k].cpu().double()
            n = int((g != want).sum())
            assert torch.equal(g, want), f"{T.case_id(r)}: {route} route, {k}: {n} of {want.numel()} elements differ"
