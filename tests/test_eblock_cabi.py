"""CPU checks of the mi_eblock_* / mi_fregate_* entry points: symbols and signatures, mi_eblock_plan against both sizing calls over
a sweep, and every refusal - all host-only: no device is touched."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

SYMBOLS = ("mi_fregate_fwd", "mi_fregate_bwd_workspace", "mi_fregate_bwd", "mi_eblock_saved_bytes", "mi_eblock_workspace",
           "mi_eblock_plan", "mi_eblock_fwd", "mi_eblock_bwd")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


def test_symbols_signatures_and_struct_layout(lib):
    handle = C.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mi_restore.h")).read()
    for s in SYMBOLS:
        assert hasattr(handle, s) and s in lib.SIGNATURES and s + "(" in header, s
    assert lib.SIGNATURES["mi_eblock_fwd"][1][:2] == [C.POINTER(lib.EblockShape), C.POINTER(lib.EblockParams)]
    assert len(lib.SIGNATURES["mi_fregate_bwd"][1]) == 14 and len(lib.SIGNATURES["mi_fregate_fwd"][1]) == 9
    # the ctypes structs follow the header's field order: 12 single pointers and two arrays of four in front of gamma
    names = [n for n, _ in lib.EBLOCK_FIELDS]
    assert names == ["norm1_w", "norm1_b", "extra_w", "extra_b", "conv1_w", "conv1_b", "br_w", "br_b", "sca_w", "sca_b", "conv3_w",
                     "conv3_b", "beta", "norm2_w", "norm2_b", "fre_w1", "fre_b1", "fre_w2", "fre_b2", "gamma"]
    for n in names:
        assert f"const float* {n}" in header and f"float* {n}" in header, n
    assert C.sizeof(lib.EblockParams) == 26 * C.sizeof(C.c_void_p)
    assert C.sizeof(lib.EblockGrads) == 27 * C.sizeof(C.c_void_p)          # + accumulate, padded
    assert C.sizeof(lib.EblockShape) == 11 * C.sizeof(C.c_int)


def test_plan_agrees_with_both_sizing_calls_over_a_sweep(lib):
    from image_restoration_amd import ops
    seen = 0
    for dtype in (torch.float32, torch.bfloat16):
        es = 4 if dtype == torch.float32 else 2
        for B, c, H, W in ((1, 1, 2, 2), (2, 4, 2, 2), (2, 8, 5, 7), (3, 6, 40, 70), (1, 256, 8, 8), (8, 32, 256, 256), (8, 256, 32, 32),
                           (1, 4, 512, 512), (2, 12, 9, 16)):
            for dil, extra in (((1,), True), ((1,), False), ((16, 16, 1, 2), True)):
                p = ops.eblock_plan(B, c, H, W, dtype, dil, extra)
                saved, ws = ops.eblock_sizes(B, c, H, W, dtype, dil, extra)
                assert (p["saved_bytes"], p["workspace"]) == (saved, ws) and saved > 0 and ws > 0
                plane = B * c * H * W * es
                up = lambda n: -(-n // 256) * 256  # noqa: E731
                assert p["x0_bytes"] == p["g_bytes"] == p["y_bytes"] == p["f_bytes"] == up(plane)
                assert p["x1_bytes"] == up(2 * plane) and p["xe_bytes"] == (up(plane) if extra else 0)
                assert p["stats_bytes"] == 4 * up(B * H * W * 4)
                assert p["fremlp_blob_bytes"] == ops.fremlp_sizes(B, c, 2, H, W, dtype)[0]
                sections = ("x0", "xe", "x1", "g", "y", "f", "stats", "small", "fremlp_blob")
                assert sum(p[k + "_bytes"] for k in sections) == saved
                assert ws >= ops.fremlp_sizes(B, c, 2, H, W, dtype)[1] + 3 * up(2 * plane)
                fre = ops.fremlp_plan(B, c, 2, H, W, dtype)
                assert p["calls_fwd"] > fre["kernels_fwd"] + fre["lib_calls_fwd"] + 6
                assert p["calls_bwd"] > fre["kernels_bwd"] + fre["lib_calls_bwd"] + 12
                vec = 16 // es
                assert p["fregate_bwd_slices"] == min(-(-(H * W) // (256 * vec * 4)), 64)
                seen += 1
    assert seen == 54
    # the FreMLP blob dominates what a bf16 block keeps: about four times its input (the fp32 half spectrum and the hidden layer)
    p = ops.eblock_plan(8, 32, 256, 256, torch.bfloat16, (1,), True)
    assert 3.9 < p["fremlp_blob_bytes"] / p["x0_bytes"] < 4.2 and p["fremlp_blob_bytes"] > 0.3 * p["saved_bytes"]


def test_every_refusal_without_a_device(lib):
    from image_restoration_amd import ops
    L = lib.lib()
    ok = dict(B=2, Cc=32, H=20, W=24, dtype=torch.float32, dilations=(1,), extra=True)
    assert ops.eblock_sizes(**ok)[0] > 0
    for bad, msg in ((dict(Cc=257), b"C=257"), (dict(Cc=0), b"C=0"), (dict(B=0), b"bad shape"), (dict(H=1), b"plane 1 x 24"),
                     (dict(W=1), b"plane 20 x 1"), (dict(H=513), b"plane 513 x 24"), (dict(W=513), b"plane 20 x 513"),
                     (dict(dilations=(1, 17)), b"dilation 17"), (dict(dilations=(0,)), b"dilation 0"), (dict(dilations=()), b"n_dil=0"),
                     (dict(dilations=(1, 2, 3, 4, 5)), b"n_dil=5")):
        args = dict(ok)
        args.update(bad)
        assert ops.eblock_sizes(**args) == (0, 0), bad
        assert msg in L.mi_last_error(), (bad, L.mi_last_error())
        with pytest.raises(RuntimeError):
            ops.eblock_plan(**{("Cc" if k == "Cc" else k): v for k, v in args.items()})
    # (2 C H W < 2^31 cannot be reached inside the other limits: 2 * 256 * 512 * 512 = 2^27)
    assert ops.eblock_sizes(1, 256, 512, 512, torch.bfloat16, (1,), True)[0] > 0
    # FreMLP's own size condition: B expand nc H K below 2^31
    assert ops.eblock_sizes(64, 256, 512, 256, torch.bfloat16, (1,), True) == (0, 0)
    s = ops._eblock_shape(2, 32, 20, 24, 7, (1,), True)
    assert L.mi_eblock_workspace(C.byref(s)) == 0 and b"bad dtype 7" in L.mi_last_error()
    assert L.mi_eblock_saved_bytes(None) == 0 and L.mi_eblock_workspace(None) == 0
    out = (lib.c_i64 * 16)()
    s = ops._eblock_shape(2, 32, 20, 24, lib.MI_F32, (1,), True)
    assert L.mi_eblock_plan(C.byref(s), None) == -1 and L.mi_eblock_plan(None, out) == -1
    # null pointers are refused with an error code, not a crash
    assert L.mi_eblock_fwd(C.byref(s), None, None, None, None, None, None) == -1 and b"null parameter" in L.mi_last_error()
    pp = lib.EblockParams()
    assert L.mi_eblock_fwd(C.byref(s), C.byref(pp), None, None, None, None, None) == -1
    assert L.mi_eblock_bwd(C.byref(s), C.byref(pp), None, None, None, None, None, None, None) == -1
    assert L.mi_fregate_fwd(None, None, None, None, 2, 4, 16, lib.MI_F32, None) == -1 and b"null pointer" in L.mi_last_error()
    assert L.mi_fregate_bwd(None, None, None, None, None, None, None, 2, 4, 16, 0, lib.MI_F32, None, None) == -1
    buf = C.create_string_buffer(256)
    for B, c, n, dt, msg in ((0, 4, 16, lib.MI_F32, b"bad shape"), (2, 0, 16, lib.MI_F32, b"bad shape"), (2, 4, 0, lib.MI_F32, b"bad shape"),
                             (70000, 4, 16, lib.MI_F32, b"bad shape"), (2, 4, 16, 7, b"bad dtype 7")):
        assert L.mi_fregate_fwd(buf, buf, C.cast(buf, lib.fp), buf, B, c, n, dt, None) == -1 and msg in L.mi_last_error(), (B, c, n, dt)
    assert L.mi_fregate_bwd_workspace(2, 4, 16) >= 2 * 4 * 4 and L.mi_fregate_bwd_workspace(0, 4, 16) == 0
    # the Python layer: CPU tensors, parameter dtype, shapes outside the limits
    from image_restoration_amd import darkir as N
    blk = N.EBlock(8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        blk(torch.zeros(1, 8, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.fregate_fwd(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), torch.zeros(8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.fregate_bwd(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), torch.zeros(8), torch.zeros(8), False)
