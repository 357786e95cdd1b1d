"""Host-only checks of the FreMLP / dense-DFT entry points: the symbols and their signatures, mi_fremlp_plan against the two
sizing calls over a sweep of shapes, every refusal (no device is touched), the module's state_dict against the reference's
recorded key list, and the CPU-tensor refusal."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import fremlp_ref as R  # noqa: E402
from plan_checks import sections_tile  # noqa: E402
from oracle.fixtures import load  # noqa: E402

SYMBOLS = ("mi_fremlp_workspace", "mi_fremlp_saved_bytes", "mi_fremlp_plan", "mi_fremlp_fwd", "mi_fremlp_bwd", "mi_dft2_workspace",
           "mi_dft2_r2c", "mi_dft2_c2r")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


def test_symbols_exist_with_their_signatures(lib):
    handle = lib.lib()
    header = open(os.path.join(ROOT, "include", "mi_restore.h")).read()
    for name in SYMBOLS:
        assert name in lib.SIGNATURES and name + "(" in header, name
        fn = getattr(handle, name)
        res, args = lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert C.sizeof(lib.FremlpShape) == 6 * C.sizeof(C.c_int)
    # pointer counts of the two launchers: shape, 4 parameters, x, out, saved, ws, stream / shape, 3 parameters, dout, dx, 4 gradients,
    # the flag, saved, ws, stream
    assert len(lib.SIGNATURES["mi_fremlp_fwd"][1]) == 10 and len(lib.SIGNATURES["mi_fremlp_bwd"][1]) == 14


SWEEP = [(1, 1, 1, 2, 2), (2, 4, 2, 2, 2), (2, 16, 2, 2, 70), (2, 16, 2, 70, 2), (2, 8, 2, 5, 7), (3, 5, 2, 100, 130), (1, 256, 2, 8, 8),
         (2, 12, 1, 9, 16), (2, 12, 3, 9, 16), (1, 4, 2, 256, 256), (1, 2, 2, 512, 512), (8, 32, 2, 256, 256), (8, 64, 2, 128, 128),
         (8, 128, 2, 64, 64), (8, 256, 2, 32, 32), (1, 1, 512, 3, 3), (5, 3, 7, 33, 65)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_plan_is_consistent_with_the_sizing_calls(lib, dtype):
    from image_restoration_amd import ops
    for B, nc, expand, H, W in SWEEP:
        p = ops.fremlp_plan(B, nc, expand, H, W, dtype)
        saved, ws = ops.fremlp_sizes(B, nc, expand, H, W, dtype)
        assert (p["saved_bytes"], p["workspace"]) == (saved, ws) and saved > 0 and ws > 0
        K, P, hc = W // 2 + 1, B * nc, expand * nc
        bins = P * H * K
        assert (p["planes"], p["K"], p["hidden"]) == (P, K, hc)
        assert p["tile_m"] == 64 and p["block"] == 256 and p["l_block"] in (48, 64, 80) and p["x_block"] in (48, 64, 80)
        assert p["l_blocks"] == -(-K // p["l_block"]) and p["x_blocks"] == -(-W // p["x_block"])
        assert p["m_tiles_folded"] == -(-P * H // 64) and p["m_tiles_plane"] == -(-H // 64)
        assert p["grid_rows_k"] == p["m_tiles_folded"] * p["l_blocks"] and p["grid_rows_w"] == p["m_tiles_folded"] * p["x_blocks"]
        assert p["grid_planes"] == P * p["m_tiles_plane"] * p["l_blocks"]
        assert p["grid_bins"] == -(-bins // 256) and p["grid_hidden"] == -(-B * hc * H * K // 256)
        assert p["grid_tables"] == -(-(W * K + H * H) // 256)
        # the blob: Z (two floats per bin), then the hidden activations (expand floats per bin); nothing else
        assert p["saved_hidden_offset"] >= 8 * bins and saved >= p["saved_hidden_offset"] + 4 * expand * bins
        assert saved < (2 + expand) * 4 * bins + 512
        # sections lie in order, 256-byte aligned, inside the workspace, and hold what the launcher puts there
        sec = p["sections"]
        assert sections_tile(sec)[0] <= ws
        for name in ("cos_w", "sin_w", "cos_wt", "sin_wt", "wcos_w", "wsin_w", "wcos_wt", "wsin_wt"):
            assert sec[name][1] == 4 * W * K
        assert sec["cos_h"][1] == sec["sin_h"][1] == 4 * H * H
        assert sec["T"][1] == sec["U"][1] == sec["Z"][1] == 8 * bins and sec["m1"][1] == sec["m2"][1] == 4 * bins
        assert sec["hidden"][1] == 4 * expand * bins
        # the transforms alone need the tables and one complex intermediate
        assert 0 < lib.lib().mi_dft2_workspace(B, nc, H, W) <= sec["U"][0]
    # the size does not depend on the activation dtype (everything in the workspace and the blob is fp32)
    assert ops.fremlp_sizes(2, 8, 2, 5, 7, torch.float32) == ops.fremlp_sizes(2, 8, 2, 5, 7, torch.bfloat16)


def test_every_refusal_returns_before_a_launch(lib):
    """No device exists in this test: a call that tried to launch would fail differently (or crash on the null pointers)."""
    L, handle = lib, lib.lib()
    out = (L.c_i64 * 64)()

    def shape(B=2, nc=8, expand=2, H=8, W=8, dtype=0):
        return L.FremlpShape(B, nc, expand, H, W, dtype)

    assert handle.mi_fremlp_plan(C.byref(shape()), out) == 0
    bad = [(dict(H=1), b"H=1"), (dict(W=1), b"W=1"), (dict(H=513), b"H=513"), (dict(W=513), b"W=513"), (dict(nc=0), b"nc=0"),
           (dict(nc=257, expand=1), b"nc=257"), (dict(nc=171, expand=3), b"expand=3"), (dict(nc=1, expand=513), b"expand=513"),
           (dict(expand=0), b"expand=0"), (dict(B=0), b"B=0"), (dict(dtype=7), b"bad dtype 7")]
    for kw, msg in bad:
        s = shape(**kw)
        assert handle.mi_fremlp_plan(C.byref(s), out) != 0, kw
        assert msg in handle.mi_last_error(), (kw, handle.mi_last_error())
        assert handle.mi_fremlp_workspace(C.byref(s)) == 0 and handle.mi_fremlp_saved_bytes(C.byref(s)) == 0
        p = C.cast(256, C.c_void_p)        # never dereferenced: the shape is refused first
        fp = C.cast(256, C.POINTER(C.c_float))
        assert handle.mi_fremlp_fwd(C.byref(s), fp, fp, fp, fp, p, p, p, p, None) != 0, kw
        assert handle.mi_fremlp_bwd(C.byref(s), fp, fp, fp, p, p, fp, fp, fp, fp, 0, p, p, None) != 0, kw
    assert 171 * 3 == 513
    assert handle.mi_fremlp_plan(None, out) != 0 and handle.mi_fremlp_plan(C.byref(shape()), None) != 0
    assert handle.mi_fremlp_workspace(None) == 0 and handle.mi_fremlp_saved_bytes(None) == 0
    # null tensors with a good shape
    assert handle.mi_fremlp_fwd(C.byref(shape()), None, None, None, None, None, None, None, None, None) != 0
    assert b"null" in handle.mi_last_error()
    assert handle.mi_fremlp_bwd(C.byref(shape()), None, None, None, None, None, None, None, None, None, 0, None, None, None) != 0
    # the transforms
    for H, W in ((1, 8), (8, 1), (513, 8), (8, 513)):
        assert handle.mi_dft2_workspace(2, 3, H, W) == 0
        fp = C.cast(256, C.POINTER(C.c_float))
        p = C.cast(256, C.c_void_p)
        assert handle.mi_dft2_r2c(p, fp, fp, 2, 3, H, W, 0, p, None) != 0 and b"outside the supported" in handle.mi_last_error()
        assert handle.mi_dft2_c2r(fp, fp, p, 2, 3, H, W, 0, p, None) != 0
    fp, p = C.cast(256, C.POINTER(C.c_float)), C.cast(256, C.c_void_p)
    assert handle.mi_dft2_r2c(p, fp, fp, 2, 3, 8, 8, 7, p, None) != 0 and b"bad dtype 7" in handle.mi_last_error()
    assert handle.mi_dft2_c2r(fp, fp, p, 0, 3, 8, 8, 0, p, None) != 0
    assert handle.mi_dft2_r2c(None, None, None, 2, 3, 8, 8, 0, None, None) != 0 and b"null" in handle.mi_last_error()
    assert handle.mi_dft2_workspace(2, 300, 8, 8) > 0          # the transforms have no channel limit


def test_module_has_reference_keys_and_refuses_cpu_and_uncovered_shapes(lib):
    from image_restoration_amd import darkir as N, ops
    import image_restoration_amd
    assert image_restoration_amd.FreMLP is N.FreMLP and "FreMLP" in N.__all__ and "FreMLP" in image_restoration_amd.__all__
    keys = load("darkir_fremlp_keys")
    for tag, args in (("nc32", dict(nc=32)), ("nc8_e3", dict(nc=8, expand=3))):
        mod = N.FreMLP(**args)
        sd = mod.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]]
        mod.load_state_dict(R.make_state(R.fremlp_shapes(args["nc"], args.get("expand", 2)), seed=5))
    assert list(sd) == ["process1.0.weight", "process1.0.bias", "process1.2.weight", "process1.2.bias"]
    assert isinstance(mod.process1[1], torch.nn.LeakyReLU) and mod.process1[1].negative_slope == 0.1
    with pytest.raises(RuntimeError, match="MI355X only"):
        mod(torch.zeros(1, 8, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.dft2_r2c(torch.zeros(1, 8, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.dft2_c2r(torch.zeros(1, 8, 8, 5), torch.zeros(1, 8, 8, 5), 8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.fremlp_bwd(torch.zeros(1, 8, 8, 8), list(mod.parameters()), torch.zeros(8), [torch.zeros_like(p) for p in mod.parameters()], False)
    for bad in (dict(nc=0), dict(nc=257, expand=1), dict(nc=171, expand=3), dict(nc=8, expand=0)):
        with pytest.raises(NotImplementedError, match="not covered"):
            N.FreMLP(**bad)
    N.FreMLP(256, 2), N.FreMLP(512 // 3, 3), N.FreMLP(1, 512)
