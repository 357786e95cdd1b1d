"""Host-only checks of the SFHformer Block entry points (csrc/sfh_block.hip): the symbols and their signatures, every refusal (no
device is touched), and for every in-range case the carving of the workspace and of the saved blob - aligned, disjoint, inside the
totals, each part's section at least what that part's own sizing call asks for - so that a mis-carved buffer shows before anything
runs on a device."""
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

import sfh_block_ref as R  # noqa: E402
from plan_checks import sections_tile  # noqa: E402
from test_sfh_fu_cabi import _exported  # noqa: E402  (the ELF dynamic-symbol reader)

SYMBOLS = tuple(f"mi_sfh_block_{n}" for n in ("workspace", "saved_bytes", "plan", "fwd", "bwd"))


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
    prefix = "mi_sfh_block_"
    declared = set(re.findall(r"\b(" + prefix + r"\w+)\(", header))
    exported = {n for n in dynsym if n.startswith(prefix)}
    table = {k for k in lib.SIGNATURES if k.startswith(prefix)}
    assert declared == exported == table == set(SYMBOLS)
    for name in SYMBOLS:
        fn = getattr(handle, name)
        res, args = lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # shape, parameters, x, out, statistics, part_in, part_out, saved, ws, stream / shape, parameters, x, dout, dx, gradients, saved, ws,
    # stream
    assert [len(lib.SIGNATURES[prefix + n][1]) for n in ("fwd", "bwd")] == [10, 9]
    ptr, i = C.sizeof(C.c_void_p), C.sizeof(C.c_int)
    assert C.sizeof(lib.SfhBlockParams) == R_PARAMS * ptr and C.sizeof(lib.SfhBlockStats) == 6 * ptr
    # the two embedded gradient structs end in an int each (padded to a pointer), then the Block's own `accumulate`
    assert C.sizeof(lib.SfhBlockGrads) == (R_PARAMS + 3) * ptr and lib.SfhBlockGrads.accumulate.size == i
    # nothing of the file but the five entry points is exported
    assert not any("sb_check" in n or "SbPlan" in n for n in dynsym)


R_PARAMS = len(R.BLOCK_PARAMS)

# B, dim, H, W: the three workload levels, the fixture cases, the limits
SWEEP = sorted({(8, 32, 256, 256), (8, 64, 128, 128), (8, 128, 64, 64), (1, 2, 2, 2), (5, 10, 7, 7), (2, 128, 512, 16), (1, 2, 512, 512),
                (2, 4, 9, 11), (2, 6, 8, 10), (1, 32, 12, 16), (1, 4, 72, 64), (2, 8, 8, 10), (2, 16, 4, 5)})
PLANES = ("y1", "m", "x1", "y2", "f")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sections_are_aligned_disjoint_inside_the_totals_and_hold_the_parts(lib, dtype, training):
    from image_restoration_amd import ops
    el = 4 if dtype == torch.float32 else 2
    for B, dim, H, W in SWEEP:
        p = ops.sfh_block_plan(B, dim, H, W, dtype, training)
        N, plane = H * W, B * dim * H * W * el
        bn = ops.bn2d_plan(B, dim, H, W, dtype, training)
        sr = ops.scale_res_plan(B, dim, H, W, dtype)
        mx = ops.sfh_mixer_plan(B, dim, H, W, dtype)
        ff = ops.sfh_ffn_plan(B, dim, H, W, dtype)
        assert (p["B"], p["dim"], p["N"]) == (B, dim, N) and p["chunks_per_plane"] == bn["chunks_per_plane"] == -(-N // 4096)
        assert (p["lib_calls_fwd"], p["lib_calls_fwd_part_in"], p["lib_calls_bwd"]) == (6, 6, 6)
        mid = mx["kernels_fwd"] + ff["kernels_fwd"] + 2 * sr["launches_fwd"]
        assert p["kernels_fwd"] == bn["launches_fwd"] + bn["launches_fwd_part_in"] + mid         # norm2 always has the pairs of x1
        assert p["kernels_fwd_part_in"] == 2 * bn["launches_fwd_part_in"] + mid
        assert p["kernels_fwd"] - p["kernels_fwd_part_in"] == (1 if training else 0)             # the statistics pass the producer saves
        assert p["kernels_bwd"] == 2 * bn["launches_bwd"] + 2 * sr["launches_bwd"] + mx["kernels_bwd"] + ff["kernels_bwd"]
        assert (p["sub_lib_calls_fwd"], p["sub_lib_calls_bwd"]) == (mx["lib_calls_fwd"] + ff["lib_calls_fwd"], mx["lib_calls_bwd"] + ff["lib_calls_bwd"])
        assert (p["saved_bytes"], p["workspace"]) == ops.sfh_block_sizes(B, dim, H, W, dtype, training) and p["workspace"] > 0
        assert p["pair_bytes"] == bn["pair_bytes"] == B * dim * bn["chunks_per_plane"] * 8
        # the workspace: aligned, in order, not overlapping, inside the total
        sec = p["sections"]
        assert list(sec) == list(ops._SB_SECTIONS)
        end, _ = sections_tile(sec)
        assert end <= p["workspace"] < end + 256
        # the parts run one after the other on one stream and share one region: it holds each of them
        mixer_saved, mixer_ws = ops.sfh_mixer_sizes(B, dim, H, W, dtype)
        ffn_saved, ffn_ws = ops.sfh_ffn_sizes(B, dim, H, W, dtype)
        parts = (ops.bn2d_workspace(B, dim, H, W, dtype, training), ops.scale_res_workspace(B, dim, H, W, dtype), mixer_ws, ffn_ws)
        assert all(n > 0 for n in parts) and sec["sub_ws"][1] == max(parts)
        assert sec["p1"][1] == (p["pair_bytes"] if training else 0)
        assert sec["d0"][1] == sec["d1"][1] == sec["d2"][1] == plane
        # the saved blob: five planes, the two stats, the parts' blobs, each at least what the part asks for; the sum of the sections
        sv = p["saved_sections"]
        assert list(sv) == list(ops._SB_SAVED)
        assert all(sv[k][1] == plane for k in PLANES) and sv["stat1"][1] == sv["stat2"][1] == bn["stat_bytes"] == 2 * dim * 4
        assert sv["mixer_blob"][1] == mixer_saved > 0 and sv["ffn_blob"][1] == ffn_saved > 0
        end, total = sections_tile(sv)
        assert p["saved_bytes"] == total and end <= total
        # the scratch of a forward without a blob holds the planes and the stats at the blob's own offsets
        assert sec["scratch"][1] == sv["mixer_blob"][0] >= sv["stat2"][0] + sv["stat2"][1]


def test_every_refusal_returns_before_a_launch(lib):
    """No device exists in this test: a call that tried to launch would fail differently (or crash on the null pointers)."""
    L, handle = lib, lib.lib()
    out = (L.c_i64 * 64)()
    p = C.cast(256, C.c_void_p)            # never dereferenced: the shape is refused first
    ws, sv, plan, fwd_, bwd_ = (getattr(handle, n) for n in SYMBOLS)

    def shape(B=2, dim=8, H=8, W=8, dtype=0, training=1, eps=1e-5, momentum=0.1):
        return L.SfhMixerShape(B, dim, H, W, dtype, training, eps, momentum)

    pp, gg, st = L.SfhBlockParams(), L.SfhBlockGrads(), L.SfhBlockStats()

    def fwd(s):
        return fwd_(s, C.byref(pp), p, p, C.byref(st), None, None, p, p, None)

    def bwd(s):
        return bwd_(s, C.byref(pp), p, p, p, C.byref(gg), p, p, None)

    assert plan(C.byref(shape()), out) == 0 and out[60] == ws(C.byref(shape())) > 0 and out[61] == sv(C.byref(shape())) > 0
    assert plan(C.byref(shape(dim=2, H=2, W=2)), out) == 0 and plan(C.byref(shape(dim=128, dtype=1)), out) == 0
    assert plan(C.byref(shape(B=1, H=2, W=2, training=1)), out) == 0
    bad = [(dict(dim=5), b"dim=5 is odd"), (dict(dim=130), b"dim=130"), (dict(dim=0), b"dim=0"), (dict(H=1), b"H=1"), (dict(H=513), b"H=513"),
           (dict(W=1), b"W=1"), (dict(W=514), b"W=514"), (dict(B=1, H=1, W=1), b"H=1"), (dict(dtype=7), b"bad dtype 7"), (dict(B=0), b"B=0"),
           (dict(B=65536), b"B=65536"), (dict(B=1024, dim=128, H=512, W=512), b"beyond the 2^31"), (dict(eps=0.0), b"eps"),
           (dict(momentum=1.5), b"momentum")]
    for kw, msg in bad:
        s = shape(**kw)
        assert plan(C.byref(s), out) != 0, kw
        assert msg in handle.mi_last_error(), (kw, handle.mi_last_error())
        assert ws(C.byref(s)) == 0 and sv(C.byref(s)) == 0, kw
        assert fwd(C.byref(s)) != 0 and bwd(C.byref(s)) != 0, kw
    assert plan(None, out) != 0 and b"null shape" in handle.mi_last_error()
    assert plan(C.byref(shape()), None) != 0
    assert ws(None) == 0 and sv(None) == 0
    # null tensors, parameters, statistics and gradient buffers with a good shape
    good = C.byref(shape())
    for call in (lambda: fwd(good), lambda: bwd(good), lambda: fwd_(good, None, p, p, C.byref(st), None, None, p, p, None),
                 lambda: fwd_(good, C.byref(pp), p, p, None, None, None, p, p, None)):
        assert call() != 0 and b"null" in handle.mi_last_error()


def test_the_wrappers_refuse_cpu_tensors_and_misfits(lib):
    from image_restoration_amd import ops, sfhformer as N
    blk = N.Block(8)
    params = list(N._block_params(blk))
    stats = [t for bn in N._block_norms(blk) for t in (bn.running_mean, bn.running_var)]
    grads = [torch.zeros_like(q) for q in params]
    x = torch.zeros(1, 8, 8, 8)
    for call in (lambda: ops.sfh_block_fwd(x, params, stats, True, False),
                 lambda: ops.sfh_block_bwd(x, x, params, torch.zeros(8), grads, False, True)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    assert ops.sfh_block_sizes(1, 5, 8, 8, torch.float32) == (0, 0) and ops.sfh_block_sizes(1, 8, 1, 8, torch.float32) == (0, 0)
    assert ops.sfh_block_sizes(1, 130, 8, 8, torch.bfloat16) == (0, 0) and ops.sfh_block_sizes(1, 8, 513, 8, torch.float32) == (0, 0)
    with pytest.raises(RuntimeError, match="odd"):
        ops.sfh_block_plan(1, 5, 8, 8)
