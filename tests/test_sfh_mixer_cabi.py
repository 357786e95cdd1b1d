"""Host-only checks of the SFHformer TokenMixer_For_Gloal / Mixer entry points: the symbols and their signatures, the two plan
queries against the sizing calls over a sweep of shapes, the byte conditions on what is saved and on the workspace, every refusal
(no device is touched), the per-image ca_conv product's plan, and the CPU-tensor refusal."""
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

import sfh_mixer_ref as R  # noqa: E402
from plan_checks import sections_tile  # noqa: E402
from test_sfh_fu_cabi import _exported  # noqa: E402  (the ELF dynamic-symbol reader)

KINDS = ("global", "mixer")
SYMBOLS = {k: tuple(f"mi_sfh_{k}_{n}" for n in ("workspace", "saved_bytes", "plan", "fwd", "bwd")) for k in KINDS}


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
    for kind in KINDS:
        prefix = f"mi_sfh_{kind}_"
        declared = set(re.findall(r"\b(" + prefix + r"\w+)\(", header))
        exported = {n for n in dynsym if n.startswith(prefix)}
        table = {k for k in lib.SIGNATURES if k.startswith(prefix)}
        assert declared == exported == table == set(SYMBOLS[kind]), prefix
        for name in SYMBOLS[kind]:
            fn = getattr(handle, name)
            res, args = lib.SIGNATURES[name]
            assert fn.restype is res and list(fn.argtypes) == list(args), name
        # shape, parameters, x, out, the two running statistics, saved, ws, stream / shape, parameters, x, dout, dx, gradients, saved,
        # ws, stream
        assert [len(lib.SIGNATURES[prefix + n][1]) for n in ("fwd", "bwd")] == [9, 9]
    assert C.sizeof(lib.SfhMixerShape) == 6 * C.sizeof(C.c_int) + 2 * C.sizeof(C.c_float)
    assert C.sizeof(lib.SfhGlobalParams) == 12 * C.sizeof(C.c_void_p) and C.sizeof(lib.SfhGlobalGrads) == 13 * C.sizeof(C.c_void_p)
    assert C.sizeof(lib.SfhMixerParams) == 24 * C.sizeof(C.c_void_p) and C.sizeof(lib.SfhMixerGrads) == 25 * C.sizeof(C.c_void_p)
    assert len(lib.SFH_MIXER_FIELDS) == len(R.MIXER_PARAMS) and len(lib.SFH_GLOBAL_FIELDS) == len(R.GLOBAL_PARAMS)
    # the kernels, launchers and the plan stay internal
    internal = ("sm_ew", "sm_tail", "sm_ca_kernel", "sm_gate", "sm_check", "sm_plan", "glo_fwd", "glo_bwd", "tail_in", "chan_attn")
    assert not any(name in n for name in internal for n in dynsym)


# B, dim, H, W: the three workload levels, every parity shape, the limits
SWEEP = sorted({(8, 32, 256, 256), (8, 64, 128, 128), (8, 128, 64, 64), (1, 2, 2, 2), (5, 10, 7, 7), (2, 128, 512, 16), (1, 2, 512, 512)} |
               {c[1] for c in R.PARITY_CASES.values()})
WS_PLANES = {"p": 2, "f": 2}                      # sections that are [B, k dim, N] planes in either module
SAVED_PLANES = {"global": {"a": 0, "b": 0, "l": 0, "u1": 2, "r": 2, "u2": 1}, "mixer": {"a": 1, "b": 1, "l": 1, "u1": 2, "r": 2, "u2": 1}}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_plans_are_consistent_with_the_sizing_calls(lib, dtype):
    from image_restoration_amd import ops
    el = 4 if dtype == torch.float32 else 2
    for B, dim, H, W in SWEEP:
        for kind in KINDS:
            if kind == "mixer" and dim % 2:
                continue
            plan, sizes = (ops.sfh_mixer_plan, ops.sfh_mixer_sizes) if kind == "mixer" else (ops.sfh_global_plan, ops.sfh_global_sizes)
            p = plan(B, dim, H, W, dtype)
            N, mix = H * W, kind == "mixer"
            assert (p["mode"], p["B"], p["dim"], p["channels"], p["N"], p["block"]) == (int(mix), B, dim, 2 * dim, N, 256)
            assert p["pool"] == min(-(-N // 4096), 16)
            assert (p["kernels_fwd"], p["kernels_bwd"], p["lib_calls_fwd"], p["lib_calls_bwd"]) == ((4, 6, 6, 12) if mix else (3, 2, 3, 3))
            assert (p["saved_bytes"], p["workspace"]) == sizes(B, dim, H, W, dtype) and p["workspace"] > 0
            # the workspace: aligned, in order, not overlapping
            sec = p["sections"]
            assert list(sec) == list(ops._SM_SECTIONS)
            end, _ = sections_tile(sec)
            assert end <= p["workspace"] < end + 256
            plane = B * dim * N * el
            for name, k in WS_PLANES.items():
                assert sec[name][1] == k * plane, name
            assert sec["g"][1] == (2 * plane if mix else 0)
            small = sum(-(-n // 64) * 64 for n in (2 * B * dim, B * dim, 2 * B * dim, 2 * B * dim, B * dim, 2 * B * dim)) * 4
            assert sec["small"][1] == (small if mix else 0)
            assert sec["fold"][1] == sec["gram_out"][1] == (B * dim * 2 * dim * 4 if mix else 0)
            assert sec["pool_partials"][1] == (B * 2 * dim * p["pool"] * 4 if mix else 0)
            fu_saved, fu_ws = ops.fourier_unit_sizes(B, 2 * dim, 4, H, W, dtype)
            assert sec["fu_ws"][1] == fu_ws
            assert sec["local_ws"][1] == (ops.sfh_local_plan(B, dim, H, W, dtype)["workspace"] if mix else 0)
            # saved: the documented planes in the activation dtype, then the FourierUnit's blob; the sum of the sections
            sv = p["saved_sections"]
            assert list(sv) == list(ops._SM_SAVED)
            for name, (_, nbytes) in sv.items():
                assert nbytes == (fu_saved if name == "fu_blob" else SAVED_PLANES[kind][name] * plane), (kind, name)
            assert p["saved_bytes"] == sections_tile(sv)[1]
            # the scratch holds the inference copy of the saved planes (not of the FourierUnit's blob, which a forward without a
            # blob never writes) or the backward's planes (e, dl, du2, da, db), whichever is larger
            bwd = sum(-(-k * plane // 256) * 256 for k in ((2, 1, 1, 1, 1) if mix else (1,)))
            assert p["bwd_scratch_bytes"] == bwd and sec["scratch"][1] == max(sv["fu_blob"][0], bwd) < p["saved_bytes"] + bwd


def test_every_refusal_returns_before_a_launch(lib):
    """No device exists in this test: a call that tried to launch would fail differently (or crash on the null pointers)."""
    L, handle = lib, lib.lib()
    out = (L.c_i64 * 64)()
    p = C.cast(256, C.c_void_p)            # never dereferenced: the shape is refused first
    f = C.cast(256, C.POINTER(C.c_float))
    common = [(dict(dim=0), b"dim=0"), (dict(dim=130), b"dim=130"), (dict(dim=-2), b"dim=-2"), (dict(H=1), b"H=1"), (dict(H=513), b"H=513"),
              (dict(W=1), b"W=1"), (dict(W=514), b"W=514"), (dict(dtype=7), b"bad dtype 7"), (dict(B=0), b"B=0"), (dict(B=65536), b"B=65536"),
              (dict(B=1024, dim=128, H=512, W=512), b"beyond the 2^31"), (dict(eps=0.0), b"eps"), (dict(momentum=1.5), b"momentum")]
    bad = {"global": common, "mixer": common + [(dict(dim=5), b"dim=5 is odd"), (dict(dim=1), b"dim=1 outside")]}
    for kind, Params, Grads in (("global", L.SfhGlobalParams, L.SfhGlobalGrads), ("mixer", L.SfhMixerParams, L.SfhMixerGrads)):
        ws, sv, plan, fwd_, bwd_ = (getattr(handle, n) for n in SYMBOLS[kind])
        sizes = (ws, sv)

        def fwd(s, pp):
            return fwd_(s, pp, p, p, f, f, p, p, None)

        def bwd(s, pp, gg):
            return bwd_(s, pp, p, p, p, gg, p, p, None)

        def shape(B=2, dim=8, H=8, W=8, dtype=0, training=1, eps=1e-5, momentum=0.1):
            return L.SfhMixerShape(B, dim, H, W, dtype, training, eps, momentum)

        pp, gg = Params(), Grads()
        assert plan(C.byref(shape()), out) == 0
        assert plan(C.byref(shape(dim=2, H=2, W=2)), out) == 0 and plan(C.byref(shape(dim=128, dtype=1)), out) == 0
        for kw, msg in bad[kind]:
            s = shape(**kw)
            assert plan(C.byref(s), out) != 0, kw
            assert msg in handle.mi_last_error(), (kw, handle.mi_last_error())
            assert all(fn(C.byref(s)) == 0 for fn in sizes), kw
            assert fwd(C.byref(s), C.byref(pp)) != 0 and bwd(C.byref(s), C.byref(pp), C.byref(gg)) != 0, kw
        assert plan(None, out) != 0 and b"null shape" in handle.mi_last_error()
        assert plan(C.byref(shape()), None) != 0
        assert all(fn(None) == 0 for fn in sizes)
        # null tensors with a good shape
        good = shape()
        for call in (lambda: fwd(C.byref(good), C.byref(pp)), lambda: bwd(C.byref(good), C.byref(pp), C.byref(gg)),
                     lambda: fwd(C.byref(good), None)):
            assert call() != 0 and b"null" in handle.mi_last_error()
    assert handle.mi_sfh_global_plan(C.byref(L.SfhMixerShape(2, 3, 8, 8, 0, 1, 1e-5, 0.1)), out) == 0       # an odd dim: the global mixer only


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_per_image_ca_conv_product_is_never_cached(lib, dtype):
    """ca_conv runs as one product with one folded matrix per image (w_bs != 0), forward and transposed: the 1x1 plan marks such
    weights as not cacheable, so a second call with other s_b cannot meet the first call's packed image."""
    from image_restoration_amd import ops
    for B, dim, H, W in SWEEP:
        if dim % 2:
            continue
        fwd = ops.pw_probe(dim, 2 * dim, H * W, dtype, B=B, per_image=True)
        bwd = ops.pw_probe(2 * dim, dim, H * W, dtype, B=B, per_image=True, transposed=True)
        assert fwd.w_bs == bwd.w_bs == 2 * dim * dim
        assert not ops.pw_plan(fwd)["cacheable"] and not ops.pw_plan(bwd)["cacheable"], (B, dim, H, W)
        need = max(ops.pw_plan(fwd)["workspace"], ops.pw_plan(bwd)["workspace"])
        assert ops.sfh_mixer_plan(B, dim, H, W, dtype)["sections"]["pw_ws"][1] >= need


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_grouped_conv_init_plans_as_a_half_product(lib, dtype):
    """Mixer.conv_init runs as ONE product of two groups that read the same x (x1_gs = 0) and write a and b apart.  That choice was
    made by the 1x1 plan: at the three levels of the network it gives the grouped descriptor the instance it gives a product of
    one half (family, tile rows, K chunks, workgroup, LDS, weight source) over twice the grid z: the two products in one launch.
    Where the planner sees enough work it hands a wave more pixel tiles and shrinks grid x to match (bf16 at dim 32: two tiles per
    wave on half the columns), so what is held equal is the instance and the pixel tiles covered."""
    from image_restoration_amd import ops
    same = ("family", "tm", "kb", "block", "lds", "tpb", "weights")
    for B, dim, H, W in ((8, 32, 256, 256), (8, 64, 128, 128), (8, 128, 64, 64)):
        N = H * W
        half = ops.pw_plan(ops.pw_probe(dim, dim, N, dtype, B=B))
        d = ops.pw_probe(dim, dim, N, dtype, B=B, groups=2)
        gap = ops.sfh_mixer_plan(B, dim, H, W, dtype)["saved_sections"]["b"][0] // (4 if dtype == torch.float32 else 2)
        d.x1_bs, d.x1_gs, d.y_bs, d.y_gs, d.bias_gs = dim * N, 0, dim * N, gap, dim
        grouped = ops.pw_plan(d)
        assert [grouped[k] for k in same] == [half[k] for k in same], (dim, grouped, half)
        assert grouped["grid"][1:] == (half["grid"][1], 2 * half["grid"][2]), (dim, grouped, half)
        assert grouped["grid"][0] * max(grouped["tpw"], 1) == half["grid"][0] * max(half["tpw"], 1), (dim, grouped, half)
        assert grouped["workspace"] <= ops.sfh_mixer_plan(B, dim, H, W, dtype)["sections"]["pw_ws"][1]


def test_modules_refuse_what_the_kernels_do_not_cover_and_cpu_tensors(lib):
    from image_restoration_amd import ops, sfhformer as N
    assert ops.SFH_MIXER_MAX_DIM == 128
    for bad in (5, 0, 130, 1, -2, 4.0):
        with pytest.raises(NotImplementedError, match="not covered"):
            N.Mixer(bad)
    for bad in (0, 129, -2, 4.0):
        with pytest.raises(NotImplementedError, match="not covered"):
            N.TokenMixer_For_Gloal(bad)
    N.Mixer(2), N.Mixer(6), N.TokenMixer_For_Gloal(1), N.TokenMixer_For_Gloal(3)
    for cls, fwd, bwd in ((N.Mixer, ops.sfh_mixer_fwd, ops.sfh_mixer_bwd), (N.TokenMixer_For_Gloal, ops.sfh_global_fwd, ops.sfh_global_bwd)):
        mod = cls(8)
        with pytest.raises(RuntimeError, match="MI355X only"):
            mod(torch.zeros(1, 8, 8, 8))
        assert int(mod.state_dict()[[k for k in mod.state_dict() if k.endswith("num_batches_tracked")][0]]) == 0
        params = list(mod.parameters())
        grads = [torch.zeros_like(q) for q in params]
        x, rm, rv = torch.zeros(1, 8, 8, 8), torch.zeros(32), torch.ones(32)
        for call in (lambda: fwd(x, params, rm, rv, True, False), lambda: bwd(x, x, params, torch.zeros(8), grads, False, True)):
            with pytest.raises(RuntimeError, match="MI355X only"):
                call()
        bn = (mod.mixer_gloal if cls is N.Mixer else mod).FFC.bn
        bn.momentum = None
        with pytest.raises(NotImplementedError, match="fixed momentum"):
            mod(torch.zeros(1, 8, 8, 8))
    assert ops.sfh_mixer_sizes(1, 5, 8, 8, torch.float32) == (0, 0) and ops.sfh_global_sizes(1, 5, 8, 8, torch.float32)[0] > 0
    assert ops.sfh_global_sizes(1, 8, 1, 8, torch.float32) == (0, 0)
