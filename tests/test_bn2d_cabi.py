"""Host-only checks of the BatchNorm2d / scaled-residual entry points: the symbols and their signatures, the two plan queries
against the sizing calls over a sweep of shapes, every refusal (no device is touched), and the CPU-tensor refusals."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import bn2d_ref as R  # noqa: E402
from plan_checks import sections_tile, up256 as up  # noqa: E402
from test_sfh_fu_cabi import _exported  # noqa: E402  (the ELF dynamic-symbol reader)

SYMBOLS = {p: tuple(f"mi_{p}_{n}" for n in ("workspace", "plan", "fwd", "bwd")) for p in ("bn2d", "scale_res")}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


def test_symbols_exist_with_their_signatures(lib):
    handle = lib.lib()
    header = open(os.path.join(ROOT, "include", "mi_restore.h")).read()
    dynsym = _exported(lib.LIB_PATH)
    for p, names in SYMBOLS.items():
        prefix = f"mi_{p}_"
        declared = set(re.findall(r"\b(" + prefix + r"\w+)\(", header))
        exported = {n for n in dynsym if n.startswith(prefix)}
        table = {k for k in lib.SIGNATURES if k.startswith(prefix)}
        assert declared == exported == table == set(names), prefix
        for name in names:
            fn = getattr(handle, name)
            res, args = lib.SIGNATURES[name]
            assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert C.sizeof(lib.Bn2dShape) == 6 * C.sizeof(C.c_int) + 2 * C.sizeof(C.c_float)
    # shape, w, b, x, y, running_mean, running_var, stat, part_in, ws, stream / shape, w, x, dy, dres, dx, dw, db, accumulate, stat, ws, stream
    assert [len(lib.SIGNATURES[f"mi_bn2d_{n}"][1]) for n in ("fwd", "bwd")] == [11, 12]
    # shape, scale, f, x, out, part_out, stream / shape, scale, f, dout, df, dscale, accumulate, ws, stream
    assert [len(lib.SIGNATURES[f"mi_scale_res_{n}"][1]) for n in ("fwd", "bwd")] == [7, 9]
    # the file adds these eight names and nothing else: kernels, helpers and the plan stay internal
    internal = ("bn_stats", "bn_finish", "bn_apply", "bn_bwd", "sr_fwd", "sr_bwd", "sr_finish", "chunk_stats", "chunk_ld", "chunk_st",
                "bn_check", "bn_plan_out", "bn_vec", "block_sum", "BnPlan")
    assert not any(name in n for name in internal for n in dynsym)
    assert {n for n in dynsym if "bn2d" in n or "scale_res" in n} == set(SYMBOLS["bn2d"]) | set(SYMBOLS["scale_res"])


# B, C, H, W: the three workload levels, every parity shape, the limits
SWEEP = sorted({(8, 32, 256, 256), (8, 64, 128, 128), (8, 128, 64, 64), (1, 1, 1, 2), (2, 1, 1, 1), (5, 10, 7, 7), (1, 4096, 16, 16),
                (1, 1, 32768, 32768 - 1), (7, 3, 640, 480)} | {c[0] for c in R.PARITY_CASES.values()})


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_plans_are_consistent_with_the_sizing_calls(lib, dtype):
    from image_restoration_amd import ops
    assert ops.BN2D_MAX_C == 4096
    V = R.vec_width(dtype)
    for B, Cn, H, W in SWEEP:
        N = H * W
        nchunk = -(-N // R.CHUNK)
        for training in (True, False):
            p = ops.bn2d_plan(B, Cn, H, W, dtype, training)
            assert (p["B"], p["C"], p["N"], p["dtype"], p["training"]) == (B, Cn, N, ops._dtype_code(dtype), int(training))
            assert (p["block"], p["chunk"]) == (R.THREADS, R.CHUNK) and R.CHUNK == R.THREADS * R.SLOTS
            assert (p["chunks_per_plane"], p["partials_per_channel"], p["chunks"]) == (nchunk, B * nchunk, B * Cn * nchunk)
            assert p["vector_width"] == (V if N % V == 0 else 1)
            assert p["grid_chunks"] == min(B * Cn * nchunk, 1 << 20) and p["grid_channels"] == -(-Cn // 256)
            assert (p["launches_fwd"], p["launches_fwd_part_in"], p["launches_bwd"]) == ((3, 2, 3) if training else (1, 1, 3))
            assert p["workspace"] == ops.bn2d_workspace(B, Cn, H, W, dtype, training) > 0
            assert p["stat_bytes"] == 8 * Cn and p["pair_bytes"] == 8 * B * Cn * nchunk
            sec = p["sections"]
            assert list(sec) == list(ops._BN_SECTIONS)
            end, total = sections_tile(sec)
            assert up(end) == p["workspace"] == total
            assert [n for _, n in sec.values()] == [p["pair_bytes"], 8 * Cn, 8 * Cn]
        q = ops.scale_res_plan(B, Cn, H, W, dtype)
        assert all(q[k] == p[k] for k in ("B", "C", "N", "block", "chunk", "chunks_per_plane", "partials_per_channel", "vector_width", "chunks",
                                          "grid_chunks", "grid_channels", "pair_bytes"))      # the seam: one chunking for both
        assert (q["launches_fwd"], q["launches_fwd_part_in"], q["launches_bwd"]) == (1, 1, 2)
        assert [n for _, n in q["sections"].values()] == [4 * B * Cn * nchunk, 0, 0]
        assert q["workspace"] == ops.scale_res_workspace(B, Cn, H, W, dtype) == up(4 * B * Cn * nchunk)


def test_every_refusal_returns_before_a_launch(lib):
    """No device exists in this test: a call that tried to launch would fail differently (or crash on the null pointers)."""
    L, handle = lib, lib.lib()
    out = (L.c_i64 * 64)()
    p = C.cast(256, C.c_void_p)            # never dereferenced: the shape is refused first

    def shape(B=2, Cn=8, H=8, W=8, dtype=0, training=1, eps=1e-5, momentum=0.1):
        return L.Bn2dShape(B, Cn, H, W, dtype, training, eps, momentum)

    both = [(dict(Cn=0), b"C=0"), (dict(Cn=4097), b"C=4097"), (dict(Cn=-2), b"C=-2"), (dict(H=0), b"H=0"), (dict(W=0), b"W=0"),
            (dict(W=-3), b"W=-3"), (dict(B=0), b"B=0"), (dict(dtype=7), b"bad dtype 7"), (dict(B=64, Cn=4096, H=128, W=64), b"beyond the 2^31"),
            (dict(B=1 << 20, Cn=1 << 11, H=1, W=1), b"beyond the 2^31")]
    bn_only = [(dict(eps=0.0), b"eps"), (dict(eps=-1e-5), b"eps"), (dict(momentum=1.5), b"momentum"), (dict(momentum=-0.1), b"momentum"),
               (dict(B=1, H=1, W=1), b"B*H*W = 1"), (dict(B=1, Cn=4096, H=1, W=1), b"B*H*W = 1")]
    calls = {
        "bn2d": (lambda s: handle.mi_bn2d_fwd(s, p, p, p, p, p, p, p, None, p, None),
                 lambda s: handle.mi_bn2d_bwd(s, p, p, p, None, p, p, p, 0, p, p, None)),
        "scale_res": (lambda s: handle.mi_scale_res_fwd(s, p, p, p, p, None, None),
                      lambda s: handle.mi_scale_res_bwd(s, p, p, p, p, p, 0, p, None)),
    }
    for kind, bad in (("bn2d", both + bn_only), ("scale_res", both)):
        ws, plan = getattr(handle, f"mi_{kind}_workspace"), getattr(handle, f"mi_{kind}_plan")
        assert plan(C.byref(shape()), out) == 0 and ws(C.byref(shape())) > 0
        assert plan(C.byref(shape(B=1, Cn=4096, H=1, W=2, dtype=1)), out) == 0
        for kw, msg in bad:
            s = shape(**kw)
            assert plan(C.byref(s), out) != 0, (kind, kw)
            assert msg in handle.mi_last_error(), (kind, kw, handle.mi_last_error())
            assert ws(C.byref(s)) == 0, (kind, kw)
            assert all(call(C.byref(s)) != 0 for call in calls[kind]), (kind, kw)
        assert plan(None, out) != 0 and b"null shape" in handle.mi_last_error()
        assert plan(C.byref(shape()), None) != 0 and ws(None) == 0
    # what BatchNorm refuses and the scaled residual takes: it reads neither eps, momentum nor training
    for kw, _ in bn_only:
        assert handle.mi_scale_res_plan(C.byref(shape(**kw)), out) == 0, kw
    # eval mode at one value per channel is a shape like any other
    assert handle.mi_bn2d_plan(C.byref(shape(B=1, H=1, W=1, training=0)), out) == 0 and out[13] == 1
    # null tensors with a good shape
    good = C.byref(shape())
    for call in (lambda: handle.mi_bn2d_fwd(good, p, p, None, p, p, p, p, None, p, None),
                 lambda: handle.mi_bn2d_fwd(good, p, p, p, p, p, p, None, None, None, None),
                 lambda: handle.mi_bn2d_bwd(good, p, p, p, None, p, p, p, 0, None, p, None),
                 lambda: handle.mi_bn2d_bwd(good, p, p, p, None, p, None, p, 0, p, p, None),
                 lambda: handle.mi_scale_res_fwd(good, None, p, p, p, None, None),
                 lambda: handle.mi_scale_res_bwd(good, p, p, p, p, None, 0, p, None),
                 lambda: handle.mi_scale_res_bwd(good, p, p, p, p, p, 0, None, None)):
        assert call() != 0 and b"null" in handle.mi_last_error()


def test_ops_and_modules_refuse_cpu_tensors_and_misfits(lib):
    from image_restoration_amd import ops, sfhformer as N
    x, v, st = torch.zeros(2, 8, 4, 4), torch.ones(8), torch.zeros(16)
    for call in (lambda: ops.bn2d_fwd(x, v, v, v, v, True, True), lambda: ops.bn2d_bwd(x, x, v, st, (v, v), False, True),
                 lambda: ops.bn2d_bwd(x, x, v, st, (v, v), False, True, dres=x), lambda: ops.scale_res_fwd(x, x, v),
                 lambda: ops.scale_res_fwd(x, x, v, want_part=True), lambda: ops.scale_res_bwd(x, x, v, v, False)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    bn = N.BatchNorm2d(8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        bn(x)
    assert int(bn.num_batches_tracked) == 0
    with pytest.raises(ValueError, match="expected 4D input"):
        bn(torch.zeros(2, 8, 4))
    for scale in (v, v.view(1, 8, 1, 1)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            N.scaled_residual(x, x, scale)
    bn.momentum = None
    with pytest.raises(NotImplementedError, match="fixed momentum"):
        bn(x)
    assert ops.bn2d_workspace(1, 8, 1, 1, torch.float32, True) == 0 and ops.bn2d_workspace(1, 8, 1, 1, torch.float32, False) > 0
    assert ops.bn2d_workspace(2, 4097, 4, 4, torch.float32) == 0 and ops.scale_res_workspace(2, 4097, 4, 4, torch.bfloat16) == 0
    with pytest.raises(RuntimeError, match="B\\*H\\*W = 1"):
        ops.bn2d_plan(1, 8, 1, 1)
