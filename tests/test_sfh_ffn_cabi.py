"""Host-only checks of the SFHformer FFN / TokenMixer_For_Local entry points: the symbols and their signatures, the two plan
queries against the sizing calls over a sweep of shapes, the byte conditions on what is saved and on the workspace, every refusal
(no device is touched), and the CPU-tensor refusal."""
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

from plan_checks import sections_tile  # noqa: E402
from test_sfh_fu_cabi import _exported  # noqa: E402  (the ELF dynamic-symbol reader)

FFN_SYMBOLS = ("mi_sfh_ffn_workspace", "mi_sfh_ffn_saved_bytes", "mi_sfh_ffn_plan", "mi_sfh_ffn_fwd", "mi_sfh_ffn_bwd")
LOCAL_SYMBOLS = ("mi_sfh_local_workspace", "mi_sfh_local_plan", "mi_sfh_local_fwd", "mi_sfh_local_bwd")


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
    for prefix, symbols in (("mi_sfh_ffn_", FFN_SYMBOLS), ("mi_sfh_local_", LOCAL_SYMBOLS)):
        declared = set(re.findall(r"\b(" + prefix + r"\w+)\(", header))
        exported = {n for n in dynsym if n.startswith(prefix)}
        table = {k for k in lib.SIGNATURES if k.startswith(prefix)}
        assert declared == exported == table == set(symbols), prefix
        for name in symbols:
            fn = getattr(handle, name)
            res, args = lib.SIGNATURES[name]
            assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert C.sizeof(lib.SfhFfnShape) == C.sizeof(lib.SfhLocalShape) == 5 * C.sizeof(C.c_int)
    assert C.sizeof(lib.SfhFfnParams) == 10 * C.sizeof(C.c_void_p) and C.sizeof(lib.SfhFfnGrads) == 11 * C.sizeof(C.c_void_p)
    assert C.sizeof(lib.SfhLocalParams) == 4 * C.sizeof(C.c_void_p) and C.sizeof(lib.SfhLocalGrads) == 5 * C.sizeof(C.c_void_p)
    # shape, parameters, x, out, saved, ws, stream / shape, parameters, x, dout, dx, gradients, saved, ws, stream; the local mixer
    # has no saved blob
    assert [len(lib.SIGNATURES[n][1]) for n in ("mi_sfh_ffn_fwd", "mi_sfh_ffn_bwd", "mi_sfh_local_fwd", "mi_sfh_local_bwd")] == [7, 9, 6, 8]
    # the kernel launchers stay internal
    assert not any("sf_fwd" in n or "sf_bwd" in n or "sf_check" in n or "block_sum4" in n for n in dynsym)


# B, dim, H, W
SWEEP = [(1, 2, 1, 1), (1, 2, 2, 2), (2, 6, 9, 33), (8, 32, 256, 256), (8, 64, 128, 128), (8, 128, 64, 64), (1, 256, 4, 6), (1, 4, 16, 64),
         (1, 4, 17, 65), (1, 4, 83, 136), (3, 4, 9, 33), (2, 2, 83, 134), (5, 10, 7, 7), (1, 64, 8, 8)]
TAPS = {"ffn": ((1, 1), (3, 1), (5, 1), (7, 1)), "local": ((3, 1), (3, 2))}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_plans_are_consistent_with_the_sizing_calls(lib, dtype):
    from image_restoration_amd import ops
    el = 4 if dtype == torch.float32 else 2
    for B, dim, H, W in SWEEP:
        for kind in ("ffn", "local"):
            p = (ops.sfh_ffn_plan if kind == "ffn" else ops.sfh_local_plan)(B, dim, H, W, dtype)
            S, s = len(TAPS[kind]), dim // 2
            assert (p["tile_w"], p["tile_h"], p["block"], p["segments"], p["segment_width"]) == (64, 16, 256, S, s)
            assert p["halo"] == tuple(d * (k - 1) // 2 for k, d in TAPS[kind])
            tiles = (-(-W // 64), -(-H // 16))
            assert (p["tiles_x"], p["tiles_y"]) == tiles
            assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (tiles[0] * tiles[1], S * s, B)
            assert p["splits"] == min(tiles[0] * tiles[1], 16) and p["partial_rows"] == B * p["splits"]
            assert p["partial_cols"] == sum(s * (k * k + 1) for k, _ in TAPS[kind] if k > 1)
            assert p["lds_fwd"] == 4 * 22 * 72 and p["lds_bwd"] == 4 * (2 * 22 * 72 + 200) and p["lds_bwd"] <= 64 * 1024
            sec = p["sections"]
            assert sections_tile(sec, unplaced_empty=True)[0] <= p["workspace"] and p["workspace"] > 0
            assert sec["partials"][1] == 4 * p["partial_rows"] * p["partial_cols"]
            plane = B * 2 * dim * H * W
            if kind == "ffn":
                saved, ws = ops.sfh_ffn_sizes(B, dim, H, W, dtype)
                assert (p["saved_bytes"], p["workspace"]) == (saved, ws)
                # saved: h and u in the activation dtype and nothing else
                assert 2 * plane * el <= saved <= 2 * plane * el + 512 and plane * el <= p["saved_u_offset"] < plane * el + 256
                assert sec["g"][1] == sec["dg"][1] == sec["dh"][1] == plane * el
                assert (p["kernels_fwd"], p["kernels_bwd"], p["lib_calls_fwd"], p["lib_calls_bwd"]) == (1, 7, 2, 6)
                # no section exceeds one fp32 plane of h, B 2dim H W 4 bytes: the three planes always; the packed 1x1 weights, the Gram
                # partials and the partial rows, whose sizes do not shrink with the plane, from 16384 elements on.  The library sizes
                # a Gram workspace as its partial tiles [splits][dim][2dim] PLUS sumsq rows [splits][dim + 2dim] that it reserves
                # whether asked for or not (mi_gram_workspace): the partial tiles are held to the plane, the reservation on top of
                # them is at most their 1/dim + 1/(2 dim).
                for name, (_, nbytes) in sec.items():
                    limit = plane * 4 * (1 + 1 / dim + 1 / (2 * dim)) if name == "gram_ws" else plane * 4
                    assert nbytes <= limit or (plane < 16384 and name not in ("g", "dg", "dh")), (name, nbytes, plane)
            else:
                s_ = lib.SfhLocalShape(B, dim, H, W, ops._dtype_code(dtype))
                assert p["workspace"] == lib.lib().mi_sfh_local_workspace(C.byref(s_))
                assert (p["saved_bytes"], p["kernels_fwd"], p["kernels_bwd"], p["lib_calls_fwd"], p["lib_calls_bwd"]) == (0, 1, 3, 0, 0)
                assert all(n == 0 for k, (_, n) in sec.items() if k != "partials")


def test_every_refusal_returns_before_a_launch(lib):
    """No device exists in this test: a call that tried to launch would fail differently (or crash on the null pointers)."""
    L, handle = lib, lib.lib()
    out = (L.c_i64 * 64)()
    p = C.cast(256, C.c_void_p)            # never dereferenced: the shape is refused first
    bad = [(dict(dim=5), b"dim=5 is odd: not covered"), (dict(dim=0), b"dim=0"), (dict(dim=258), b"dim=258"), (dict(H=0), b"H=0"),
           (dict(W=0), b"W=0"), (dict(dtype=7), b"bad dtype 7"), (dict(B=0), b"B=0"), (dict(dim=-2), b"dim=-2"),
           (dict(B=1024, dim=256, H=4096, W=4096), b"beyond the 2^31")]
    for Shape, plan, sizes, fwd, bwd, Params, Grads in (
            (L.SfhFfnShape, handle.mi_sfh_ffn_plan, (handle.mi_sfh_ffn_workspace, handle.mi_sfh_ffn_saved_bytes),
             lambda s, pp: handle.mi_sfh_ffn_fwd(s, pp, p, p, p, p, None),
             lambda s, pp, gg: handle.mi_sfh_ffn_bwd(s, pp, p, p, p, gg, p, p, None), L.SfhFfnParams, L.SfhFfnGrads),
            (L.SfhLocalShape, handle.mi_sfh_local_plan, (handle.mi_sfh_local_workspace,),
             lambda s, pp: handle.mi_sfh_local_fwd(s, pp, p, p, p, None),
             lambda s, pp, gg: handle.mi_sfh_local_bwd(s, pp, p, p, p, gg, p, None), L.SfhLocalParams, L.SfhLocalGrads)):

        def shape(B=2, dim=8, H=8, W=8, dtype=0):
            return Shape(B, dim, H, W, dtype)

        pp, gg = Params(), Grads()
        assert plan(C.byref(shape()), out) == 0
        assert plan(C.byref(shape(dim=2, H=1, W=1)), out) == 0 and plan(C.byref(shape(dim=256, dtype=1)), out) == 0
        for kw, msg in bad:
            s = shape(**kw)
            assert plan(C.byref(s), out) != 0, kw
            assert msg in handle.mi_last_error(), (kw, handle.mi_last_error())
            assert all(f(C.byref(s)) == 0 for f in sizes), kw
            assert fwd(C.byref(s), C.byref(pp)) != 0 and bwd(C.byref(s), C.byref(pp), C.byref(gg)) != 0, kw
        assert plan(None, out) != 0 and b"null shape" in handle.mi_last_error()
        assert plan(C.byref(shape()), None) != 0
        assert all(f(None) == 0 for f in sizes)
        # null tensors with a good shape
        good = shape()
        for call in (lambda: fwd(C.byref(good), C.byref(pp)), lambda: bwd(C.byref(good), C.byref(pp), C.byref(gg)),
                     lambda: fwd(C.byref(good), None)):
            assert call() != 0 and b"null" in handle.mi_last_error()
    assert handle.mi_sfh_ffn_fwd(C.byref(L.SfhFfnShape(2, 8, 8, 8, 0)), C.byref(L.SfhFfnParams()), None, None, None, None, None) != 0
    assert handle.mi_sfh_local_bwd(C.byref(L.SfhLocalShape(2, 8, 8, 8, 0)), C.byref(L.SfhLocalParams()), None, None, None,
                                   C.byref(L.SfhLocalGrads()), None, None) != 0


def test_modules_refuse_what_the_kernels_do_not_cover_and_cpu_tensors(lib):
    from image_restoration_amd import ops, sfhformer as N
    assert ops.SFH_FFN_MAX_DIM == 256
    for cls in (N.FFN, N.TokenMixer_For_Local):
        for bad in (5, 0, 258, 1, -2, 4.0):
            with pytest.raises(NotImplementedError, match="not covered"):
                cls(bad)
        cls(2), cls(256), cls(6)
        mod = cls(8)
        with pytest.raises(RuntimeError, match="MI355X only"):
            mod(torch.zeros(1, 8, 8, 8))
        params = list(mod.parameters())
        grads = [torch.zeros_like(q) for q in params]
        x = torch.zeros(1, 8, 8, 8)
        if cls is N.FFN:
            calls = (lambda: ops.sfh_ffn_fwd(x, params, False), lambda: ops.sfh_ffn_bwd(x, x, params, torch.zeros(8), grads, False))
        else:
            calls = (lambda: ops.sfh_local_fwd(x, params), lambda: ops.sfh_local_bwd(x, x, params, grads, False))
        for call in calls:
            with pytest.raises(RuntimeError, match="MI355X only"):
                call()
    assert ops.sfh_ffn_sizes(1, 5, 8, 8, torch.float32) == (0, 0)
