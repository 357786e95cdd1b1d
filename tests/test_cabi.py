"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/mi_restore.h declares, the ctypes table matches the header, sizing entry points work without a GPU,
the modules keep the reference's state_dict, and CPU tensors are refused (no fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "mi_restore.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(lib):
    handle = C.CDLL(lib.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 24
    for s in syms:
        assert hasattr(handle, s), f"{s} declared in include/mi_restore.h but not exported"
    assert set(syms) == set(lib.SIGNATURES), "ctypes table and header disagree"
    assert lib.lib().mi_version() == 100


def test_unknown_dtype_code_is_refused_without_gpu(lib):
    # the dtype dispatch returns before anything is launched: the buffers are never touched
    src, dst = C.create_string_buffer(64), C.create_string_buffer(64)
    assert lib.lib().mi_cast(src, lib.MI_F32, dst, 7, 16, None) == -1
    assert b"bad dtype 7" in lib.lib().mi_last_error()


def test_sizing_and_argument_errors_without_gpu(lib):
    L = lib
    s = L.MdtaShape(2, 48, 1, 16, 16, L.MI_F32, 3)
    assert L.lib().mi_mdta_saved_bytes(C.byref(s)) > 2 * 2 * 144 * 256 * 4
    assert L.lib().mi_mdta_workspace(C.byref(s)) > 0
    g = L.GdfnShape(2, 48, 127, 16, 16, L.MI_BF16, 3)
    # conv input (2h planes) + gate output (h planes); the conv output is recomputed in backward for 3x3 on 16-pixel rows
    assert L.lib().mi_gdfn_saved_bytes(C.byref(g)) >= 2 * (254 + 127) * 256 * 2
    bad = L.MdtaShape(2, 50, 4, 16, 16, L.MI_F32, 3)   # 50 channels not divisible by 4 heads
    assert L.lib().mi_mdta_saved_bytes(C.byref(bad)) == 0
    assert b"divisible" in L.lib().mi_last_error()
    # null pointers are rejected with an error code, not a crash
    assert L.lib().mi_ln_fwd(None, None, None, None, None, None, 1, 4, 16, 1, 0, None) == -1
    assert L.lib().mi_ln_bwd_workspace(8, 48, 65536) > 0
    assert L.lib().mi_dwconv_bwd_workspace(8, 144, 256, 256, 3) > 0


def test_state_dict_matches_reference_and_cpu_is_refused(lib):
    import image_restoration_amd as m
    from oracle import restormer_ref as R
    from oracle.fixtures import load
    net = m.Restormer()
    keys = [str(k) for k in load("restormer_base_keys")["keys"]]
    sd = net.state_dict()
    assert list(sd) == keys
    shapes = R.restormer_param_shapes(R.RESTORMER_BASE)
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert sum(p.numel() for p in net.parameters()) == 26126644
    tiny = m.Restormer(**{k: v for k, v in R.RESTORMER_TINY.items()})
    tiny.load_state_dict(R.make_restormer_state(R.RESTORMER_TINY, seed=1))
    blk = m.TransformerBlock(48, 1, 2.66, True, "BiasFree")
    assert "norm1.body.bias" not in blk.state_dict() and "attn.qkv.bias" in blk.state_dict()
    with pytest.raises(RuntimeError, match="MI355X only"):
        blk(torch.zeros(1, 48, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.LayerNorm(48, "WithBias")(torch.zeros(1, 48, 8, 8))


def test_moce_and_adair_state_dict_keys_match_reference(lib):
    """Key lists captured from the reference modules (tools/capture_golden_moce.py) vs the drop-in modules."""
    import image_restoration_amd.adair as ad
    import image_restoration_amd.moce_ir as mo
    from oracle.fixtures import load
    gold = load("moce_keys")
    db = mo.DecoderBlock(dim=48, num_heads=1, ffn_expansion_factor=2, bias=False, LayerNorm_type="WithBias",
                         expert_layer=mo.FFTAttention, complexity_scale="max", rank=2, num_experts=4, top_k=1,
                         depth_type="constant", rank_type="spread", stage_depth=1, freq_dim=64, with_complexity=True)
    assert list(db.state_dict()) == [str(k) for k in gold["decoder"]]
    assert list(mo.EncoderBlock(48, 2, 2, True, "WithBias").state_dict()) == [str(k) for k in gold["encoder"]]
    assert list(mo.CrossAttention(48, 1, True).state_dict()) == [str(k) for k in gold["cross"]]
    assert list(ad.Chanel_Cross_Attention(48, 4, False).state_dict()) == [str(k) for k in gold["adair_cross"]]
    with pytest.raises(RuntimeError, match="MI355X only"):
        mo.CrossAttention(48, 1, True)(torch.zeros(1, 48, 8, 8), torch.zeros(1, 48, 8, 8))
    # AdaIR: the whole network and its frequency module (tools/capture_golden_adair.py), MoCE-IR whole network
    from image_restoration_amd import configs
    from oracle import adair_ref as A
    akeys = load("adair_keys")
    net = ad.AdaIR(**configs.ADAIR_BASE)
    assert list(net.state_dict()) == [str(k) for k in akeys["adair_base"]]
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == A.adair_param_shapes(configs.ADAIR_BASE)
    assert list(ad.FreModule(48, 4, False).state_dict()) == [str(k) for k in akeys["fre"]]
    with pytest.raises(RuntimeError):
        ad.FreModule(32, 2, False)(torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 8, 8))      # CPU tensors: no fallback


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "image_restoration_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f"{f} imports the oracle"


def test_env_switches_are_read_once_and_reloadable(lib, monkeypatch):
    """The launch planners' MI_* switches come from a table filled at first use; mi_env_reload() / reload_env() re-read it."""
    import image_restoration_amd as m
    from image_restoration_amd import ops
    assert lib.lib().mi_env_reload() == 0
    os.environ["MI_NO_LN_HEAD"] = "1"          # behind the package's back: not seen until a reload
    try:
        ops.reload_env()
        assert ops.env("MI_NO_LN_HEAD") == "1"
        os.environ.pop("MI_NO_LN_HEAD")
        assert ops.env("MI_NO_LN_HEAD") == "1"  # cached
        m.reload_env()
        assert ops.env("MI_NO_LN_HEAD") is None
    finally:
        os.environ.pop("MI_NO_LN_HEAD", None)
        m.reload_env()
    monkeypatch.setenv("MI_TORCH_OPS", "0")    # the conftest fixture reloads after monkeypatch.setenv
    assert ops.env("MI_TORCH_OPS") == "0"


def test_torch_library_custom_ops_are_registered(lib):
    """north_star: 'registers PyTorch-ROCm custom ops over a thin C-ABI'.  Without a GPU: the eight mi_restore:: ops exist with
    the documented schemas, have an Autograd registration, and their fake (meta) implementations produce the real ops' output
    structure (run under FakeTensorMode: no kernel is touched).  The GPU suite runs torch.library.opcheck on real inputs."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from image_restoration_amd import torch_ops
    from oracle import restormer_ref as R
    for name in ("layernorm", "mdta", "gdfn", "transformer_block"):
        for sfx in ("_fwd", "_bwd"):
            op = getattr(torch.ops.mi_restore, name + sfx).default
            assert str(op._schema).endswith("-> Tensor[]")
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"mi_restore::{name}_fwd", "Autograd")
    sch = str(torch.ops.mi_restore.transformer_block_fwd.default._schema)
    assert "Tensor x, int heads, Tensor n1_w, Tensor? n1_b, Tensor temperature, Tensor qkv_w, Tensor? qkv_b" in sch and "bool need" in sch
    c, heads = 48, 1
    sd = R.make_block_state(c, heads, 2.66, False, "WithBias", seed=1)
    order = ["norm1.body.weight", "norm1.body.bias", "attn.temperature", "attn.qkv.weight", "attn.qkv.bias",
             "attn.qkv_dwconv.weight", "attn.qkv_dwconv.bias", "attn.project_out.weight", "attn.project_out.bias",
             "norm2.body.weight", "norm2.body.bias", "ffn.project_in.weight", "ffn.project_in.bias", "ffn.dwconv.weight",
             "ffn.dwconv.bias", "ffn.project_out.weight", "ffn.project_out.bias"]
    with FakeTensorMode() as mode:
        params = [mode.from_tensor(sd[k]) if k in sd else None for k in order]
        x = mode.from_tensor(torch.zeros(2, c, 16, 16))
        outs = torch.ops.mi_restore.transformer_block_fwd(x, heads, *params, True)
        assert len(outs) == 10 and tuple(outs[0].shape) == (2, c, 16, 16)
        assert tuple(outs[4].shape) == (2, 256) and outs[4].dtype == torch.float32        # LayerNorm statistics
        assert outs[8].dtype == torch.uint8 and outs[8].numel() > 2 * 2 * 3 * c * 256 * 4  # the MDTA saved blob (mi_mdta_saved_bytes)
        res = torch.ops.mi_restore.transformer_block_bwd(outs[0], x, heads, *params, list(outs[1:]), False)
        assert len(res) == 18 and tuple(res[0].shape) == (2, c, 16, 16)
        assert tuple(res[4].shape) == tuple(sd["attn.qkv.weight"].shape) and res[5].dtype == torch.int8   # qkv.bias absent (bias=False)
        nog = torch.ops.mi_restore.transformer_block_fwd(x, heads, *params, False)
        assert all(t.dtype == torch.int8 for t in nog[1:])          # placeholders for absent saved tensors
        y = torch.ops.mi_restore.layernorm_fwd(x, params[0], params[1], True)
        assert len(y) == 3 and tuple(y[1].shape) == (2, 256)
        a = torch.ops.mi_restore.mdta_fwd(x, heads, *params[2:9], True)
        f = torch.ops.mi_restore.gdfn_fwd(x, *params[11:17], True)
        assert len(a) == 2 and len(f) == 2 and a[1].dtype == torch.uint8 and f[1].dtype == torch.uint8


def test_glue_has_no_vendor_fallback(lib):
    """Round-2 verdict (weak #5): planes outside the wave-streaming kernels' set used to leave the native path silently.  Now
    every H, W is native (mi_glue3x3_ok) and the Python glue has no F.conv2d / F.pixel_shuffle / torch.cat / torch.fft path left;
    anything the native kernels do not implement raises."""
    import torch.nn as nn
    import image_restoration_amd.restormer as rs
    for hw in ((8, 8), (16, 16), (512, 512), (1024, 1024), (7, 9)):
        assert lib.lib().mi_glue3x3_ok(*hw) == 1
    for f in ("restormer.py", "moce_ir.py", "adair.py"):
        text = open(os.path.join(ROOT, "image_restoration_amd", f)).read()
        for banned in ("F.conv2d", "F.pixel_shuffle", "F.pixel_unshuffle", "torch.fft", "import torch.nn.functional"):
            assert banned not in text, (f, banned)
    with pytest.raises(NotImplementedError, match="3x3"):
        rs._conv2d(torch.zeros(1, 4, 8, 8), nn.Conv2d(4, 4, 5, padding=2))
    with pytest.raises(RuntimeError, match="MI355X only"):
        rs._conv2d(torch.zeros(1, 4, 8, 8), nn.Conv2d(4, 4, 3, padding=1))
    with pytest.raises(RuntimeError, match="MI355X only"):
        rs._shuffle(torch.zeros(1, 4, 8, 8), False)


def test_ln_plan_query_and_its_argument_errors(lib, monkeypatch):
    """mi_ln_plan reports what mi_ln_fwd / mi_ln_bwd launch (the launchers call the same plan functions) without a GPU."""
    from image_restoration_amd import ops
    monkeypatch.delenv("MI_LN_FORM", raising=False)
    f32, bf16 = torch.float32, torch.bfloat16
    assert ops.ln_plan(2, 48, 130, bf16, False) == {"family": "wave", "CB": 48, "WS": 1, "NW": 4, "vec": 2, "tiles": 4, "gx": 1,
                                                    "rows": 0, "two_stage": False}
    assert ops.ln_plan(3, 49, 130, f32, True) == {"family": "wave", "CB": 24, "WS": 4, "NW": 4, "vec": 1, "tiles": 1, "gx": 3,
                                                  "rows": 9, "two_stage": False}
    # an odd pixel count or a misaligned pointer: one bf16 pixel per lane, and with it the block family
    for kw in ({"N": 129}, {"N": 130, "aligned": False}):
        assert ops.ln_plan(3, 96, dtype=bf16, backward=True, **kw) == {"family": "block", "waves": 8, "CPT": 12, "vec": 1, "tiles": 1,
                                                                      "gx": 3, "rows": 9, "two_stage": False}
    assert ops.ln_plan(1, 768, 64, f32, True)["family"] == "block" and ops.ln_plan(1, 768, 64, f32, True)["CPT"] == 48
    assert ops.ln_plan(3, 16, 2753, f32, True)["rows"] == 132 and ops.ln_plan(3, 16, 2753, f32, True)["two_stage"]
    assert ops.ln_plan(2, 16, 4033, f32, True)["rows"] == 128 and not ops.ln_plan(2, 16, 4033, f32, True)["two_stage"]
    monkeypatch.setenv("MI_LN_FORM", "block")
    assert ops.ln_plan(2, 48, 130, bf16, False) == {"family": "block", "waves": 8, "CPT": 6, "vec": 2, "tiles": 1, "gx": 2,
                                                    "rows": 0, "two_stage": False}
    monkeypatch.setenv("MI_LN_FORM", "wave")
    assert ops.ln_plan(2, 384, 130, f32, False)["WS"] == 4 and ops.ln_plan(2, 385, 130, f32, False)["family"] == "block"
    out = (C.c_int * 9)()
    assert lib.lib().mi_ln_plan(1, 769, 64, lib.MI_F32, 0, 1, out) == -1 and b"769" in lib.lib().mi_last_error()
    assert lib.lib().mi_ln_plan(1, 769, 64, lib.MI_BF16, 1, 1, out) == -1
    assert lib.lib().mi_ln_plan(1, 48, 64, 7, 0, 1, out) == -1 and b"bad dtype 7" in lib.lib().mi_last_error()
    assert lib.lib().mi_ln_plan(1, 48, 64, lib.MI_F32, 0, 1, None) == -1
    assert lib.lib().mi_ln_plan(0, 48, 64, lib.MI_F32, 0, 1, out) == -1


def test_ln_case_lists_reach_every_plan(lib, monkeypatch):
    """Every kernel instance the LayerNorm dispatch can choose - over C = 1..768, both dtypes, both directions, aligned or not,
    even or odd pixel counts and the three MI_LN_FORM settings - is run by a case of tests/test_gpu_ln.py.  A threshold that
    moves in ln.hip shows up here as the plan that lost its case."""
    import test_gpu_ln as T
    possible = {}
    for form in T.FORMS:
        T.set_form(monkeypatch, form)
        for c in range(1, 769):
            for d in ("f32", "bf16"):
                for n in (130, 65):
                    for aligned in (True, False):
                        pf, pb = T.plans(3, c, n, d, aligned)
                        for key in (T.plan_key("fwd", d, pf), T.plan_key("bwd", d, pb)):
                            possible.setdefault(key, (form, c, n, aligned))
    reached = T.reached_plans(monkeypatch)
    missing = {k: v for k, v in possible.items() if k not in reached}
    assert not missing, "plans without a test case (plan: first (MI_LN_FORM, C, N, aligned) that takes it): %r" % missing
    assert len(possible) >= 40 and reached <= set(possible)


# --------------------------------------------------------------------------- the 1x1 GEMM plan (mi_pw_plan)
from pw_forms import PW_INSTANCES, PW_SWITCHES, PW_WAVE_FORMS, key as pw_key      # shared with tests/test_gpu_pw_forms.py

PW_MS = (16, 48, 49, 64, 96, 97, 144, 192, 254, 256, 288, 510, 1021, 2042)
PW_KS = (16, 33, 48, 96, 97, 128, 129, 192, 193, 384, 576, 1020)
PW_NS = (35, 64, 256, 4096)


def _pw_switches(monkeypatch, **env):
    for k in PW_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _pw_sweep():
    import itertools
    from image_restoration_amd import ops
    for M, K, N, dtype, groups, per_image, transposed in itertools.product(PW_MS, PW_KS, PW_NS, (torch.float32, torch.bfloat16),
                                                                         (1, 2), (False, True), (False, True)):
        yield dtype, ops.pw_probe(M, K, N, dtype, B=2, groups=groups, per_image=per_image, transposed=transposed)


def test_pw_plan_pinned_for_every_family(lib, monkeypatch):
    """ops.pw_plan, every field, for one descriptor per kernel family (batch 2, bias + residual).  Kernel instance, grid and
    block are what a kernel trace of these calls showed BEFORE the plan became the one place of decision (the trace reports
    static LDS only: the dynamic LDS bytes, the counts and the workspace follow the formulas of that launcher; planes this small
    leave one pixel tile per wave / workgroup)."""
    from image_restoration_amd import ops
    f32, bf16 = torch.float32, torch.bfloat16

    def plan(M, K, N, dtype, env={}, **kw):
        _pw_switches(monkeypatch, **env)
        return ops.pw_plan(ops.pw_probe(M, K, N, dtype, residual=True, **{"B": 2, **kw}))

    def want(family, tm, kb, grid, block, lds, workspace, **kw):
        base = {"family": family, "tm": tm, "kb": kb, "f8": False, "ln": False, "grid": grid, "block": block, "lds": lds, "tpw": 0,
                "tpb": 0, "n_slabs": 0, "slabs_per": 0, "xcd_map": False, "weights": "pack", "cacheable": True, "workspace": workspace}
        return {**base, **kw}

    assert plan(48, 48, 35, f32) == want("chunked", 48, 2, (1, 1, 2), 256, 0, 16640)
    assert plan(144, 48, 256, bf16, {"MI_PW_WAVE": "0"}) == want("resident", 64, 2, (4, 3, 2), 256, 30720, 49408, tpb=1)
    assert plan(144, 48, 256, bf16, {"MI_PW_DMA": "1"}) == want("dma", 64, 2, (4, 3, 2), 256, 36864, 49408)
    assert plan(254, 48, 256, bf16) == want("xres", 64, 2, (1, 1, 2), 512, 77824, 65792, tpw=1)
    assert plan(96, 510, 256, bf16) == want("stream", 96, 16, (1, 1, 2), 512, 159744, 131328, tpw=1)
    assert plan(64, 160, 256, bf16) == want("stream", 64, 5, (1, 1, 2), 512, 62464, 41216, tpw=1)
    assert plan(48, 127, 256, bf16) == want("stream", 48, 4, (1, 1, 2), 512, 52224, 16640, tpw=1)
    assert plan(510, 128, 256, bf16) == want("xwide", 64, 4, (1, 8, 2), 512, 77824, 262400, tpw=1, n_slabs=8, slabs_per=1)
    assert plan(510, 192, 256, bf16) == want("xwide", 64, 6, (1, 8, 2), 512, 98304, 393472, tpw=1, n_slabs=8, slabs_per=1)
    assert plan(1021, 384, 256, bf16) == want("lds", 256, 6, (4, 1, 2), 512, 67584, 786432, cacheable=False)
    # a pointer off the 16-byte grid, or pixel rows that are no multiple of 8: the chunked kernel
    assert plan(144, 48, 256, bf16, misalign=2) == want("chunked", 64, 2, (4, 3, 2), 256, 0, 49408)
    assert plan(144, 48, 35, bf16) == want("chunked", 64, 2, (1, 3, 2), 256, 0, 49408)
    # beyond the traced calls: a plane large enough for the per-wave / per-workgroup counts to leave 1, and the per-image weight sources
    assert plan(510, 96, 65536, bf16, B=32)["tpw"] == 4 and plan(254, 48, 65536, bf16, B=32)["tpw"] == 2
    assert plan(144, 48, 65536, bf16, {"MI_PW_WAVE": "0"})["tpb"] == 3
    _pw_switches(monkeypatch)
    d = ops.pw_probe(96, 96, 256, bf16, B=2, per_image=True)
    assert (ops.pw_plan(d)["weights"], ops.pw_plan(d)["cacheable"]) == ("pack", False)
    d.w_b16, d.w_b16_sm = ops.PW_PROBE, 96
    assert ops.pw_plan(d)["weights"] == "b16"
    d.w_b16 = None
    _pw_switches(monkeypatch, MI_PW_DIRECT="1")
    assert ops.pw_plan(d)["weights"] == "f32"


def test_pw_predicates_and_workspace_follow_the_plan(lib, monkeypatch):
    """mi_pw_gemm_ln_ok / _split_ok / _f8_ok say what the plan of the same descriptor says, and mi_pw_gemm_workspace covers the
    plan for aligned and for unaligned pointers, over every shape class of the sweep."""
    from image_restoration_amd import ops
    _pw_switches(monkeypatch)
    L, n = lib.lib(), 0

    def family_with(d, **feature):                    # the family of the same call with one optional feature switched on
        for k, v in feature.items():
            setattr(d, k, v)
        fam = ops.pw_plan(d)["family"]
        for k in feature:
            setattr(d, k, 0)
        return fam

    for dtype, d in _pw_sweep():
        p = ops.pw_plan(d)
        ln = d.groups == 1 and (family_with(d, ln_mode=1) == "xres" or (family_with(d, ln_mode=1) == "xwide" and d.k1 <= 128))
        assert bool(L.mi_pw_gemm_ln_ok(C.byref(d))) == ln, (p, d.m, d.k1, d.n)
        for ok, fam in ((L.mi_pw_gemm_split_ok, family_with(d, y2=ops.PW_PROBE)), (L.mi_pw_gemm_f8_ok, family_with(d, f8=1))):
            assert bool(ok(C.byref(d))) == (dtype == torch.bfloat16 and fam in PW_WAVE_FORMS), (p, fam, d.m, d.k1, d.n)
        ws = L.mi_pw_gemm_workspace(C.byref(d))
        d.y += 2                                      # the same call with an unaligned output
        q = ops.pw_plan(d)
        assert q["family"] == "chunked" and ws >= p["workspace"] and ws >= q["workspace"], (p, q, ws)
        n += 1
    assert n == 14 * 12 * 4 * 2 * 2 * 2 * 2


def test_pw_every_family_and_instance_is_reachable(lib, monkeypatch):
    """The sweep under the default switches and under each A/B switch reaches all seven families and every kernel instance (with
    fp8 operands and LayerNorm on load wherever the predicates allow them).  A threshold that strands an instance shows up here."""
    from image_restoration_amd import ops

    def key(dtype, d, p):
        return pw_key(dtype, p)

    reached = set()
    for env in ({}, {"MI_PW_WAVE": "0"}, {"MI_PW_CHUNKED": "1"}, {"MI_PW_DMA": "1"}, {"MI_PW_XWIDE": "0"}, {"MI_PW_WAVE_WIDE": "0"},
                {"MI_PW_LDS": "all"}):
        _pw_switches(monkeypatch, **env)
        for dtype, d in _pw_sweep():
            p = ops.pw_plan(d)
            reached.add(key(dtype, d, p))
            if p["family"] in PW_WAVE_FORMS:
                ln_ok = bool(lib.lib().mi_pw_gemm_ln_ok(C.byref(d)))
                for f8, ln in ((1, 0), (0, 1), (1, 1)):
                    if ln and not ln_ok:
                        continue
                    d.f8, d.ln_mode = f8, ln
                    q = ops.pw_plan(d)
                    assert q["family"] == p["family"] and q["f8"] == bool(f8) and q["ln"] == bool(ln)
                    reached.add(key(dtype, d, q))
                d.f8, d.ln_mode = 0, 0
    assert reached == PW_INSTANCES, (sorted(PW_INSTANCES - reached, key=str), sorted(reached - PW_INSTANCES, key=str))
    assert {k[0] for k in reached} == set(ops.PW_FAMILIES)


def test_pw_case_tables_reach_every_instance_and_loop_state(lib, monkeypatch):
    """The GPU case tables of tests/pw_forms.py, planned here on probe descriptors of the rows' shapes, strides and features: every
    row reaches the instance and loop state it names (a row nobody can reach fails here, without a GPU), the union of the tables
    is every kernel instance, and the loop states the default plans of small planes never take are each there at least once."""
    import pw_forms as P
    from image_restoration_amd import ops
    reached, states, ids = set(), set(), set()
    for table, rows in P.TABLES.items():
        for r in rows:
            assert (table, P.case_id(r)) not in ids, f"{table}: two rows named {P.case_id(r)}"
            ids.add((table, P.case_id(r)))
            P.set_switches(monkeypatch, r["env"])
            p = P.reach(ops, r, P.probe(ops, r))
            reached.add(P.key(P.DTYPES[r["dtype"]], p))
            states |= P.loop_state(r, p)
            if r["replaced"]:
                P.set_switches(monkeypatch, r["replaced"])
                assert ops.pw_plan(P.probe(ops, r))["family"] != r["key"][0], (P.case_id(r), r["replaced"])
    assert reached == PW_INSTANCES, (sorted(PW_INSTANCES - reached, key=str), sorted(reached - PW_INSTANCES, key=str))
    want = ({(s, f) for s in ("tpw_ragged", "tpw_idle") for f in ("xres", "stream")}             # the wave forms' tile loop
            | {("tpb_ragged",), ("resident_partial_tile",), ("xcd_map",)}
            | {("slabs", "one"), ("slabs", "some_ragged"), ("slabs", "all")}                     # the X-wide slab pipeline
            | {("weights", src, f) for src in ops.PW_WEIGHTS for f in PW_WAVE_FORMS} | {("split", f) for f in PW_WAVE_FORMS}
            | {("ln", inst, mode) for inst in (("xres", 1), ("xres", 2), ("xres", 3), ("xwide", 4)) for mode in (1, 2)}
            | {("strided", f) for f in ops.PW_FAMILIES})
    assert want <= states, sorted(want - states, key=str)


def test_pw_ln_bar_admits_the_model_and_catches_four_faults(lib):
    """The LayerNorm-on-load bar of tests/pw_forms.py (e_gpu <= 1.5 e_model + 2^-8) on the CPU, at every shape, mode and operand
    type of the table: it passes the model of the kernel's roundings evaluated in the opposite summation order, and each of four
    faults - the K tail counted in the statistics, gamma / beta one channel off, beta in the wrong mode, the statistics of the
    previous pixel tile - lands at least 3 x over it.  Likewise the NaN guard: a store one row past M and a skipped tile are caught."""
    import pw_forms as P
    from image_restoration_amd import ops
    seen = set()
    for r in P.LN_CASES:
        sig = (r["M"], r["K"], r["ln"], r["f8"])
        if sig in seen:
            continue
        seen.add(sig)
        h = P._host((r["B"], 1, r["M"], r["K"], 0, r["N"], False, True))
        ref, mu, rstd = P.ln_model(h, r["ln"], "fp64")
        bar = P.ln_bar(P.rel_err(P.ln_model(h, r["ln"], "kernel", f8=r["f8"])[0], ref))
        other, mu32, rstd32 = P.ln_model(h, r["ln"], "kernel", f8=r["f8"], flip=True)
        assert P.rel_err(other, ref) <= bar, (sig, P.rel_err(other, ref), bar)
        assert P.rel_err(mu32, mu) < P.BAR_STATS and P.rel_err(rstd32, rstd) < P.BAR_STATS
        for fault in P.LN_FAULTS:
            if fault == "k_tail" and r["K"] % 32 == 0:          # no tail: not a fault
                continue
            e = P.rel_err(P.ln_model(h, r["ln"], "kernel", f8=r["f8"], fault=fault)[0], ref)
            assert e >= 3 * bar, f"{sig}: fault {fault} at {e:.3e} is within 3 x the bar {bar:.3e}"
    assert len(seen) == 11
    r = next(r for r in P.WAVE_LOOP_CASES if r["key"] == ("xres", 2, False) and r["tpw"] == 2)
    call = P.build(ops, r, "cpu")
    P.fake_store(call)
    call.check_guards()
    assert torch.equal(call.result(), call.ref)
    for fault, msg in (("row_past_m", "outside the output were written"), ("skipped_tile", "never written")):
        call.reset_outputs()
        P.fake_store(call, fault)
        with pytest.raises(AssertionError, match=msg):
            call.check_guards()


def test_pw_plan_argument_errors(lib):
    from image_restoration_amd import ops
    L, out = lib.lib(), (C.c_int64 * 18)()
    d = ops.pw_probe(48, 48, 64, torch.float32)
    assert L.mi_pw_plan(None, out) == -1 and b"null pointer" in L.mi_last_error()
    assert L.mi_pw_plan(C.byref(d), None) == -1 and b"pw_plan: null pointer" in L.mi_last_error()
    d.dtype = 7
    assert L.mi_pw_plan(C.byref(d), out) == -1 and b"bad dtype 7" in L.mi_last_error()


# --------------------------------------------------------------------------- the Gram plan (mi_gram_plan)
GRAM_SWITCHES = ("MI_GRAM_LDS", "MI_GRAM_STREAM_ALL", "MI_GRAM_RECT", "MI_GRAM_FOLD", "MI_GRAM_WANT")
GRAM_MS = (16, 30, 48, 64, 65, 96, 97, 128, 129, 144, 192, 193, 254, 288, 384, 385, 510, 1021, 2042)
GRAM_NS = (35, 64, 1024, 4096, 65536)
GRAM_SWEEP_CASES = 19 * 19 * 5 * 2 * 3 * 2 * 3


def _gram_switches(monkeypatch, **env):
    for k in GRAM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _gram_sweep():
    """(dtype, descriptor) over the shape classes; sumsq only where legal (not with sum_batch)."""
    import itertools
    from image_restoration_amd import ops
    for ma, mb, N, dtype, B, groups, (sum_batch, sumsq) in itertools.product(
            GRAM_MS, GRAM_MS, GRAM_NS, (torch.float32, torch.bfloat16), (1, 2, 32), (1, 2), ((False, False), (False, True), (True, False))):
        yield dtype, ops.gram_probe(ma, mb, N, dtype, B=B, groups=groups, sum_batch=sum_batch, sumsq=sumsq)


def test_gram_plan_pinned_for_every_family_and_finish(lib, monkeypatch):
    """ops.gram_plan, every field, for one descriptor per family, tile and finish kind.  The values are what the launchers decided
    BEFORE the plan became the one place of decision.  Family, tile (the kernel instance's fragment counts and its sumsq flag),
    grid, block, fold, vec_ok and the reduce kernel that follows come from that commit's own planners and launch branches, asked
    through a debug export of a build of it (which agreed with mi_gram_plan on every one of these fields over the whole sweep
    below, aligned and not, accumulating and not).  What no launch shows follows the formulas of that launcher: unit = 32 pixels
    (fp32) / 64, units = ceil(n / unit) (folded: batch * n / unit), the split rule (512 / tiles workgroups, LDS; 768 / tiles
    capped at units / 32 and rounded up to 4 steps, streaming), part_bytes = splits * Z * ma * mb floats and ss_bytes = splits *
    Z * (ma + mb) floats, each rounded up to 256; workspace = part_bytes + ss_bytes."""
    from image_restoration_amd import ops
    f32, bf16 = torch.float32, torch.bfloat16
    _gram_switches(monkeypatch)

    def plan(ma, mb, N, dtype, **kw):
        return ops.gram_plan(ops.gram_probe(ma, mb, N, dtype, **kw))

    def want(family, fa, fb, unit, units, per_split, splits, tiles, Z, part, ss, finish, **kw):
        base = {"family": family, "fa": fa, "fb": fb, "sumsq": False, "unit": unit, "units": units, "per_split": per_split,
                "splits": splits, "tiles_a": tiles[0], "tiles_b": tiles[1], "Z": Z, "fold": 0, "vec_ok": True,
                "grid": (splits, tiles[0] * tiles[1], Z), "block": 256, "part_bytes": part, "ss_bytes": ss, "finish": finish,
                "deferrable": False, "workspace": part + ss}
        return {**base, **kw}

    # the LDS-staged tiles: fp32 2 x 2 and 4 x 4, bf16 3 x 3 with sumsq, the three rectangular ones (folded weight gradients)
    assert plan(48, 48, 1024, f32, B=2, sumsq=True) == want("lds", 2, 2, 32, 32, 1, 32, (1, 1), 2, 589824, 24576, "general", sumsq=True)
    assert plan(144, 48, 1024, f32, B=2, sum_batch=True) == want("lds", 4, 4, 32, 32, 1, 32, (2, 1), 2, 1769472, 49152, "general")
    assert plan(96, 96, 1024, bf16, B=2, sumsq=True) == want("lds", 3, 3, 64, 16, 1, 16, (1, 1), 2, 1179648, 24576, "few16", sumsq=True)
    assert plan(96, 255, 1024, bf16, B=2, sum_batch=True) == want("lds", 3, 8, 64, 32, 1, 32, (1, 1), 1, 3133440, 45056, "few16", fold=16)
    assert plan(576, 192, 1024, bf16, B=2, sum_batch=True) == want("lds", 4, 6, 64, 32, 1, 32, (5, 1), 1, 14155776, 98304, "few16", fold=16)
    assert plan(192, 510, 1024, bf16, B=2, sum_batch=True) == want("lds", 6, 4, 64, 32, 1, 32, (1, 4), 1, 12533760, 89856, "few16", fold=16)
    # streaming: one tile (per image, two heads, sumsq), several tiles (summed per image), folded
    assert plan(48, 48, 4096, bf16, B=2, groups=2, sumsq=True) == want("stream", 3, 3, 64, 64, 32, 2, (1, 1), 4, 73728, 3072, "few4", sumsq=True)
    assert plan(254, 48, 4096, bf16, B=2, sum_batch=True) == want("stream", 4, 3, 64, 64, 32, 2, (4, 1), 2, 195072, 4864, "few4")
    assert plan(144, 48, 1024, bf16, B=4, sum_batch=True) == want("stream", 3, 3, 64, 64, 32, 2, (3, 1), 1, 55296, 1536, "few4", fold=16)
    # the finish kinds: straight into the output; deferrable; reduce few<4> / few<16> / general
    assert plan(48, 48, 64, bf16, B=2) == want("lds", 2, 2, 64, 1, 1, 1, (1, 1), 2, 18432, 768, "direct")
    assert plan(48, 48, 1024, bf16, B=2, sum_batch=True, accumulate=True) == want("lds", 2, 2, 64, 32, 1, 32, (1, 1), 1, 294912, 12288,
                                                                                 "general", fold=16, deferrable=True)
    assert plan(48, 48, 256, bf16, B=2) == want("lds", 2, 2, 64, 4, 1, 4, (1, 1), 2, 73728, 3072, "few4")
    assert plan(48, 48, 256, bf16, B=2, sum_batch=True) == want("lds", 2, 2, 64, 8, 1, 8, (1, 1), 1, 73728, 3072, "few16", fold=4)
    assert plan(48, 48, 1024, f32, B=5, sum_batch=True) == want("lds", 2, 2, 32, 32, 1, 32, (1, 1), 5, 1474560, 61440, "general")
    # a column block of a wider gradient (out_ld > mb) is summed at once, never deferred
    assert plan(144, 48, 1024, bf16, B=2, sum_batch=True, accumulate=True, out_ld=96) == want("lds", 4, 4, 64, 32, 1, 32, (2, 1), 1, 884736,
                                                                                            24576, "general", fold=16)
    # a pointer off the 16-byte grid, or pixel rows that are no multiple of 8: the LDS-staged kernel with scalar loads
    assert plan(48, 48, 4096, bf16, B=2, misalign=2) == want("lds", 2, 2, 64, 64, 1, 64, (1, 1), 2, 1179648, 49152, "general", vec_ok=False)
    assert plan(48, 48, 35, bf16, B=2) == want("lds", 2, 2, 64, 1, 1, 1, (1, 1), 2, 18432, 768, "direct", vec_ok=False)


def test_gram_workspace_follows_the_plan(lib, monkeypatch):
    """mi_gram_workspace covers the plan of the descriptor as given and of the same call with `a` off the 16-byte grid, over
    every shape class of the sweep."""
    from image_restoration_amd import ops
    _gram_switches(monkeypatch)
    L, n = lib.lib(), 0
    for dtype, d in _gram_sweep():
        ws = L.mi_gram_workspace(C.byref(d))
        p = ops.gram_plan(d)
        d.a += 2
        q = ops.gram_plan(d)
        assert q["family"] == "lds" and not q["vec_ok"] and ws >= p["workspace"] and ws >= q["workspace"], (p, q, ws)
        n += 1
    assert n == GRAM_SWEEP_CASES


# every instance the launcher's tables hold: (family, dtype, fa, fb, sumsq).  The rectangular LDS tiles go to calls without sumsq only.
GRAM_INSTANCES = (
    {("lds", dt, f, f, ss) for dt, fs in (("f32", (2, 4)), ("bf16", (2, 3, 4))) for f in fs for ss in (False, True)} |
    {("lds", "bf16", fa, fb, False) for fa, fb in ((3, 8), (4, 6), (6, 4))} |
    {("stream", "bf16", fa, fb, ss) for fa in (3, 4, 6) for fb in (3, 4, 6) if (fa, fb) != (6, 6) for ss in (False, True)})


def test_gram_every_instance_is_reachable_and_none_unknown(lib, monkeypatch):
    """The sweep under the default switches and under each A/B switch reaches every kernel instance of the launcher's two tables
    and names none outside them.  A threshold that strands an instance, or a plan the launcher would refuse, shows up here."""
    from image_restoration_amd import ops
    reached = set()
    for env in ({}, {"MI_GRAM_LDS": "1"}, {"MI_GRAM_STREAM_ALL": "1"}, {"MI_GRAM_RECT": "0"}, {"MI_GRAM_FOLD": "0"}, {"MI_GRAM_FOLD": "2"}):
        _gram_switches(monkeypatch, **env)
        n = 0
        for dtype, d in _gram_sweep():
            p = ops.gram_plan(d)
            reached.add((p["family"], "bf16" if dtype == torch.bfloat16 else "f32", p["fa"], p["fb"], p["sumsq"]))
            n += 1
        assert n == GRAM_SWEEP_CASES
    assert reached == GRAM_INSTANCES, "stranded: %r; unknown to the launcher: %r" % (
        sorted(GRAM_INSTANCES - reached, key=str), sorted(reached - GRAM_INSTANCES, key=str))
    assert len(GRAM_INSTANCES) == 29 and {k[0] for k in reached} == set(ops.GRAM_FAMILIES)


def test_gram_plan_argument_errors_and_the_32_bit_guard(lib, monkeypatch):
    from image_restoration_amd import ops
    _gram_switches(monkeypatch)
    L, out = lib.lib(), (C.c_int64 * 22)()
    bf16 = torch.bfloat16
    d = ops.gram_probe(48, 48, 64, torch.float32)
    assert L.mi_gram_plan(None, out) == -1 and b"null pointer" in L.mi_last_error()
    assert L.mi_gram_plan(C.byref(d), None) == -1 and b"gram_plan: null pointer" in L.mi_last_error()
    for field, value, msg in (("dtype", 7, b"bad dtype 7"), ("ma", 0, b"bad shape"), ("out_ld", 47, b"out_ld < mb"), ("a", None, b"null pointer")):
        e = ops.gram_probe(48, 48, 64, torch.float32)
        setattr(e, field, value)
        assert L.mi_gram_plan(C.byref(e), out) == -1 and msg in L.mi_last_error(), field
    e = ops.gram_probe(48, 48, 64, torch.float32, sum_batch=True, sumsq=True)
    assert L.mi_gram_plan(C.byref(e), out) == -1 and b"sumsq with sum_batch" in L.mi_last_error()
    # the streaming kernel addresses a slice with 32-bit element offsets: max(ma, mb) * n < 2^31, beyond it the LDS-staged form
    # (64-bit addressing) - also under the switch that streams everything
    N = 4096 * 4096
    assert ops.gram_plan(ops.gram_probe(127, 48, N, bf16))["family"] == "stream"                 # 127 * 2^24 < 2^31
    assert ops.gram_plan(ops.gram_probe(128, 48, N, bf16))["family"] == "lds"                    # = 2^31
    assert ops.gram_plan(ops.gram_probe(48, 128, N, bf16))["family"] == "lds"
    big = ops.gram_plan(ops.gram_probe(254, 48, N, bf16))
    assert (big["family"], big["fa"], big["fb"], big["vec_ok"]) == ("lds", 4, 4, True)
    _gram_switches(monkeypatch, MI_GRAM_STREAM_ALL="1")
    assert ops.gram_plan(ops.gram_probe(254, 48, N, bf16))["family"] == "lds"
    assert ops.gram_plan(ops.gram_probe(127, 48, N, bf16))["family"] == "stream"


# --------------------------------------------------------------------------- the backward tail's plan (mi_bwd_tail_plan)
BT_FORMS = ((48, 1, 192, 4, 3, 512), (48, 193, 256, 4, 4, 512), (96, 1, 384, 8, 3, 256), (96, 385, 512, 8, 4, 256))   # C, M from..to, waves, fragments, grid


def _bt_switches(monkeypatch, **env):
    for k in ("MI_BT_WIDE", "MI_BT_DEBUG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_bwd_tail_plan_sweep(lib, monkeypatch):
    """ops.bwd_tail_plan over M = 1..520 for covered and uncovered C: the table of forms read from csrc/bwd_tail.hip, agreement
    with mi_bwd_tail_ok and mi_bwd_tail_workspace everywhere, MI_BT_WIDE, and workgroups / passes around the grid."""
    from image_restoration_amd import ops
    L, bf16, f32 = lib.lib(), torch.bfloat16, torch.float32
    _bt_switches(monkeypatch)
    zeros = dict.fromkeys(ops.BWD_TAIL_PLAN_FIELDS, 0)
    zeros.update(covered=False, pays=False)
    plans = {}
    for C_ in (48, 96, 64, 192):
        form = [f for f in BT_FORMS if f[0] == C_]
        for M in range(1, 521):
            p = plans[(C_, M)] = ops.bwd_tail_plan(M, C_, 2, 576, bf16)
            assert p["covered"] == bool(L.mi_bwd_tail_ok(M, C_, 576, lib.MI_BF16)), (C_, M)
            row = [f for f in form if f[1] <= M <= f[2] and M >= 16]
            if not row:                              # M < 16, M above the cap, another C
                assert p == zeros and L.mi_bwd_tail_workspace(M, C_) == 0, (C_, M, p)
                continue
            _, _, _, waves, frags, grid = row[0]
            assert p == {"covered": True, "pays": True, "waves": waves, "fragments": frags, "rows_per_wave": 16 * frags,
                         "mpad": 16 * frags * waves, "workgroups": 18, "tiles": 18, "passes": 1, "active_waves": -(-M // (16 * frags)),
                         "lds": {48: 76736, 96: 153472}[C_], "workspace": L.mi_bwd_tail_workspace(M, C_)}, (C_, M, p)
            assert M <= p["mpad"] and 1 <= p["active_waves"] <= waves      # (LDS: 3 and 4 fragments both take two 32-row patch steps)
            assert p["workspace"] >= 4 * grid * M * (C_ + 1)                       # a partial [M][C + 1] per workgroup of the full grid
            for N, dt in ((577, bf16), (96, bf16), (576, f32)):                    # no multiple of the tile; fp32
                assert ops.bwd_tail_plan(M, C_, 2, N, dt) == zeros
                assert not L.mi_bwd_tail_ok(M, C_, N, lib.MI_BF16 if dt == bf16 else lib.MI_F32)
            # workgroups and passes around the grid
            if M in (16, 17, 192, 193, 256, 384, 385, 512):
                for tiles, wgs, passes in ((1, 1, 1), (grid - 1, grid - 1, 1), (grid, grid, 1), (grid + 1, grid, 2), (2 * grid + 1, grid, 3)):
                    for B, tpi in ((1, tiles), (tiles, 1)):
                        q = ops.bwd_tail_plan(M, C_, B, 64 * tpi, bf16)
                        assert (q["tiles"], q["workgroups"], q["passes"]) == (tiles, wgs, passes), (C_, M, B, tpi, q)
                        assert {k: v for k, v in q.items() if k not in ("tiles", "workgroups", "passes")} == \
                               {k: v for k, v in p.items() if k not in ("tiles", "workgroups", "passes")}
    # MI_BT_WIDE=0 switches the C = 96 four-fragment form off for the module entry points, and nothing else
    _bt_switches(monkeypatch, MI_BT_WIDE="0")
    for (C_, M), p in plans.items():
        q = ops.bwd_tail_plan(M, C_, 2, 576, bf16)
        assert q == {**p, "pays": p["pays"] and not (C_ == 96 and p["fragments"] == 4)}, (C_, M)
    _bt_switches(monkeypatch, MI_BT_WIDE="1")
    assert all(ops.bwd_tail_plan(M, C_, 2, 576, bf16) == p for (C_, M), p in plans.items())


def test_bwd_tail_plan_argument_errors(lib):
    L, out = lib.lib(), (C.c_int64 * 12)()
    assert L.mi_bwd_tail_plan(144, 48, 2, 576, lib.MI_BF16, None) == -1 and b"bwd_tail_plan: null pointer" in L.mi_last_error()
    assert L.mi_bwd_tail_plan(144, 48, 2, 576, 7, out) == -1 and b"bad dtype 7" in L.mi_last_error()
    for M, B, N in ((0, 2, 576), (144, 0, 576), (144, 2, 0), (-1, 2, 576), (144, -3, 576), (144, 2, -64)):
        assert L.mi_bwd_tail_plan(M, 48, B, N, lib.MI_BF16, out) == -1 and b"bwd_tail_plan: bad shape" in L.mi_last_error(), (M, B, N)
    assert L.mi_bwd_tail_plan(144, 64, 2, 576, lib.MI_BF16, out) == 0 and list(out) == [0] * 12      # uncovered: no error
    assert L.mi_bwd_tail_plan(144, 48, 2, 576, lib.MI_BF16, out) == 0 and out[0] == 1


def test_tail_case_lists_reach_every_plan(lib, monkeypatch):
    """The case lists of tests/test_gpu_bwd_tail.py reach every form of the kernel with one, two and at least three passes of
    the persistent loop, with and without a row tail, with idle waves, with dres given and absent, accumulating and not."""
    from image_restoration_amd import ops
    import test_gpu_bwd_tail as T
    _bt_switches(monkeypatch)
    seen = {}
    for case in T.EXACT_CASES:
        C_, f, M, B, tpi, passes, dres, accumulate, narrow = case
        p = T.assert_plan(C_, f, M, B, tpi, passes)
        for tag in ("passes %d" % min(p["passes"], 3), "tail" if M % 16 else "no tail", "dres" if dres else "no dres",
                    "accumulate" if accumulate else "overwrite") + (("idle waves",) if p["active_waves"] < p["waves"] else ()):
            seen.setdefault((C_, p["fragments"]), set()).add(tag)
    assert set(seen) == set(T.FORMS)
    every = {"passes 1", "passes 2", "passes 3", "tail", "no tail", "dres", "no dres", "accumulate", "overwrite"}
    for form, tags in seen.items():
        assert tags >= every | ({"idle waves"} if form[1] == 3 else set()), (form, every - tags)   # a 4-fragment form has rows for every wave
    for form, ms in T.ROW_MS.items():                        # the row counts at the borders of each form
        lo, hi = next((f[1], f[2]) for f in BT_FORMS if (f[0], f[4]) == form)
        assert max(lo, 16) in ms and hi in ms and all(ops.bwd_tail_plan(M, form[0], 2, 576, torch.bfloat16)["fragments"] == form[1] for M in ms)
    for case in T.MODEL_CASES:
        assert T.assert_plan(*case)["passes"] == 1 and case[2] % 16
    assert {c[:2] for c in T.MODEL_CASES} == set(T.FORMS)


def _tail_host_cases(T):
    """One Family-A and one Family-B case per C, small enough for the host: (inputs, fp64 reference)."""
    out = []
    for C_, f, M, B, tpi in ((48, 4, 254, 2, 9), (96, 4, 510, 1, 7)):
        s = T.exact_inputs(C_, M, B, tpi)
        r = T.reference(s, *T.exact_operands(s))
        T.assert_exact_preconditions(s, r, 5.0)
        m = T.float_inputs(C_, M, B, tpi, stats="cpu")
        out.append((C_, f, s, r, m, T.reference(m, *T.model_operands(m))))
    return out


def test_tail_bounds_admit_a_correct_fp32_evaluation(lib, monkeypatch):
    """The tail evaluated in torch fp32 on the CPU, in a permuted summation order, passes the assertions of both families of
    tests/test_gpu_bwd_tail.py: the bounds ask nothing that correct fp32 arithmetic cannot give."""
    import test_gpu_bwd_tail as T
    _bt_switches(monkeypatch)
    for C_, f, s, r, m, rm in _tail_host_cases(T):
        plan = T.assert_plan(C_, f, s.M, s.B, s.tpi)
        for wgs, accumulate, seed in ((plan["workgroups"], False, 0), (4, True, 1)):       # one pass; three passes of four workgroups
            ratio, equal = T.assert_exact(T.evaluate_fp32(s, wgs, accumulate, seed=seed), s, r, plan, accumulate, "fp32 on the host")
            assert ratio <= 1.0 and equal > 0.98
        T.assert_model_near_statement(m, rm)
        assert max(T.assert_model(T.evaluate_fp32(m, 4, seed=2), m, rm, plan, "fp32 on the host")) <= 1.0


def test_tail_assertions_catch_four_deliberate_faults(lib, monkeypatch):
    """Four faults of the kind the tail's masking, pipelining and partial sums can have, applied to the fp32 evaluation on the
    CPU: each fails Family A's assertions, and the modelled bounds of Family B see the dropped row on float data too.

    Contrast with the max-norm bars that guarded the kernel before (tests/test_gpu_fused.py: 2e-2 of max|dx|, 1e-2 for the
    parameter gradients), on random float data with real statistics.  Measured here, error / max|ref| of (dx, dW, dgamma):
        the last valid dY row left out of W^T dY    0.051 .. 0.136, unchanged, unchanged   (C, M, pixels) = (96, 510, 448) .. (48, 144, 2048)
        two pixels' rstd swapped                    0.0145, 0.0020, 0.0027                 (96, 510, 3072)
    A wholly dropped row is NOT under the old dx bar: its worst element is a product of two tail values against a maximum that
    grows with sqrt(M) only, 5 % of it and more (1 / sqrt(510) = 4 % relates typical values).  The old tests miss it where they
    never go - the row counts at a form's borders, a third pass, dres absent, a small call after a large one.  Where the bar
    itself is blind is a statistic read for the wrong pixel: real rstd varies little between pixels, and the swap stays under
    all three bars while Family A (rstd drawn from {0.5, 1, 2} per pixel) and the modelled bounds both fail it."""
    import test_gpu_bwd_tail as T
    _bt_switches(monkeypatch)
    for C_, f, s, r, m, rm in _tail_host_cases(T):
        plan = T.assert_plan(C_, f, s.M, s.B, s.tpi)
        for fault, what in zip(T.FAULTS, ("dx off", "dw differs", "dx off", "dw differs")):      # (a statistic enters xh, so G too)
            with pytest.raises(AssertionError, match=what):
                T.assert_exact(T.evaluate_fp32(s, 4, fault=fault), s, r, plan, False, fault)
        T.assert_exact(T.evaluate_fp32(s, 4), s, r, plan, False, "no fault")
        pure = T.assert_model_near_statement(m, rm)
        got = T.evaluate_fp32(m, 4, fault="drop_last_row")
        assert T.max_norm(got[0], pure.dx) > T.MAX_NORM_DX                                 # the old bar sees a whole row ...
        with pytest.raises(AssertionError, match="dx off"):                                # ... and so do the modelled bounds
            T.assert_model(got, m, rm, plan, "dropped row")
    C_, f, M, B, tpi = 96, 4, 510, 2, 24
    m, plan = T.float_inputs(C_, M, B, tpi, stats="cpu"), T.assert_plan(C_, f, M, B, tpi)
    rm = T.reference(m, *T.model_operands(m))
    pure = T.assert_model_near_statement(m, rm)
    got = T.evaluate_fp32(m, 4, fault="swap_rstd")
    assert T.max_norm(got[0], pure.dx) < T.MAX_NORM_DX                                     # unseen by the old bars
    assert max(T.max_norm(g_, getattr(pure, n)) for n, g_ in zip(("dw", "dgamma", "dbeta"), got[1:])) < T.MAX_NORM_PARAM
    with pytest.raises(AssertionError, match="off at"):
        T.assert_model(got, m, rm, plan, "swapped rstd")
    assert max(T.assert_model(T.evaluate_fp32(m, 4), m, rm, plan, "no fault")) <= 1.0


# --------------------------------------------------------------------------- the fused forwards' plans (mi_gdfn_fused_plan, mi_mdta_fused_plan)
FUSED_CS, FUSED_HS, FUSED_WS = (48, 96, 192), tuple(range(8, 73, 8)) + (20,), (32, 64, 128, 192)
FUSED_BS = (1, 2, 8, 32, 52, 86, 300)
FUSED_HIDDEN = {48: (127, 96), 96: (255, 192), 192: (510,)}


def _fg_layout_bytes(C_, hidden, pc):
    """Bytes of the tile sections of the pack for one chunk width (fg_pack_layout in csrc/fused_gdfn.hip)."""
    up = lambda v: -(-v // 256) * 256
    nch = -(-hidden // pc)
    return up(nch * 2 * pc * (C_ + 8) * 2) + up(nch * C_ * (pc + 8) * 2) + up(nch * pc * 20 * 4) + up(C_ * 4)


def test_gdfn_fused_plan_sweep(lib, monkeypatch):
    """ops.gdfn_fused_plan over shapes, batches, entries and every switch string the GPU cases use: covered agrees with the _ok
    predicates, grid = B * S with 1 <= S <= tiles, the tiles cover the image, LDS within 160 KiB, the pack holds the tile
    sections of either chunk width, xcd_pairs only on 32-wide tiles with a multiple of 16 of them, uncovered = all zeros."""
    from image_restoration_amd import ops
    import fused_forms as FF
    L = lib.lib()
    zeros = dict.fromkeys(ops.GDFN_FUSED_PLAN_FIELDS, 0)
    zeros.update(covered=False, save=False, f8=False, xcd_pairs=False, family=None)
    rows = FF.ladder_rows()
    n = 0
    for cfg in FF.GDFN_SWITCHES:
        for noxcd in (False, True):
            FF.set_switches(monkeypatch, cfg, noxcd=noxcd)
            for C_ in FUSED_CS:
                for H in FUSED_HS:
                    for W in FUSED_WS:
                        for B in FUSED_BS:
                            hidden = FUSED_HIDDEN[C_][(H // 8 + B) % len(FUSED_HIDDEN[C_])]
                            s = lib.GdfnFusedShape(B, C_, hidden, H, W, 1)
                            shape_ok = C_ in (48, 96) and H % 8 == 0 and W % 64 == 0
                            plans = {e: ops.gdfn_fused_plan((B, C_, H, W), hidden, e) for e in ops.GDFN_FUSED_ENTRIES}
                            assert plans["inference"]["covered"] == bool(L.mi_gdfn_fused_ok(C.byref(s))) == shape_ok
                            assert plans["train"]["covered"] == bool(L.mi_gdfn_fused_fwd_train_ok(C.byref(s)))
                            assert L.mi_gdfn_fused_pack_bytes(C.byref(s)) == plans["inference"]["pack_bytes"]
                            for e, p in plans.items():
                                n += 1
                                if not p["covered"]:
                                    assert p == zeros, (cfg, e, p)
                                    continue
                                tiles = p["tiles_x"] * p["tiles_y"]
                                assert p["tiles_x"] * p["tw"] == W and p["tiles_y"] * p["th"] == H and p["C"] == C_
                                assert 1 <= p["S"] <= tiles and p["grid"] == B * p["S"] and p["block"] == 64 * p["waves"]
                                assert 0 < p["lds"] <= 160 * 1024
                                assert p["save"] == (e == "train") and p["f8"] == (e == "f8")
                                assert p["pack_bytes"] >= max(_fg_layout_bytes(C_, hidden, 16), _fg_layout_bytes(C_, hidden, 32))
                                assert p["pack_pc"] in (16, 32) and p["pack_pc"] == plans["inference"]["pack_pc"]
                                if p["family"] == "tile":
                                    assert p["S"] == tiles and p["nch"] == -(-hidden // p["pc"]) and p["pc"] == p["pack_pc"] and p["ngr"] == 0
                                    assert (C_, p["th"], p["tw"], p["pc"], p["waves"]) in rows[e], (cfg, e, p)
                                    assert p["xcd_pairs"] == (p["tw"] == 32 and (B * tiles) % 16 == 0 and not noxcd)
                                else:
                                    assert e != "f8" and (p["th"], p["tw"], p["waves"]) == (8, 32, 8) and not p["xcd_pairs"]
                                    assert p["S"] == max(1, min(256 // B, tiles // 2)) and p["ngr"] % 2 == 0 and 32 * p["ngr"] >= hidden
                                if p["xcd_pairs"]:
                                    assert p["tw"] == 32 and (B * tiles) % 16 == 0
    assert n == len(FF.GDFN_SWITCHES) * 2 * 3 * len(FUSED_HS) * 4 * 7 * 3
    # the example of the plan's contract: training under w64,pc16 at C = 96 has no kernel, inference has
    FF.set_switches(monkeypatch, "w64,pc16")
    assert ops.gdfn_fused_plan((2, 96, 24, 128), 255, "train") == zeros
    assert FF.instance_of(ops.gdfn_fused_plan((2, 96, 24, 128), 255, "inference")) == FF.tile(96, 8, 64, 16, 8)
    out = (C.c_int64 * 20)()
    s = lib.GdfnFusedShape(2, 96, 255, 24, 128, 1)
    assert L.mi_gdfn_fused_plan(None, 0, out) == -1 and L.mi_gdfn_fused_plan(C.byref(s), 0, None) == -1
    assert L.mi_gdfn_fused_plan(C.byref(s), 3, out) == -1 and b"bad entry 3" in L.mi_last_error()
    assert L.mi_gdfn_fused_plan(C.byref(lib.GdfnFusedShape(0, 96, 255, 24, 128, 1)), 0, out) == -1 and b"bad shape" in L.mi_last_error()


def test_mdta_fused_plan_sweep(lib, monkeypatch):
    """ops.mdta_fused_plan over the same shapes under both MI_FM_CFG settings: covered agrees with mi_mdta_fused_ok, pays with
    mi_mdta_fused_pays, the workspace and pack sizes with their entry points, and the partials' arena holds part_mult * S
    partials per image."""
    from image_restoration_amd import ops
    import fused_forms as FF
    L = lib.lib()
    zeros = dict.fromkeys(ops.MDTA_FUSED_PLAN_FIELDS, 0)
    zeros.update(covered=False, pays=False, kind=None, form=None)
    for cfg in ("", "v2"):
        FF.set_switches(monkeypatch, fm_cfg=cfg)
        for C_, heads in ((48, 1), (96, 1), (96, 2), (96, 4), (48, 2), (192, 4)):
            for H in FUSED_HS:
                for W in FUSED_WS:
                    for B in FUSED_BS:
                        s = lib.MdtaShape(B, C_, heads, H, W, lib.MI_BF16, 3)
                        p = ops.mdta_fused_plan((B, C_, H, W), heads)
                        kind = {(48, 1): "48_1", (96, 2): "96_2", (96, 1): "96_1"}.get((C_, heads))
                        assert p["covered"] == bool(L.mi_mdta_fused_ok(C.byref(s))) == (kind is not None and H % 8 == 0 and W % 64 == 0)
                        assert p["pays"] == bool(L.mi_mdta_fused_pays(C.byref(s)))
                        assert p["workspace"] == L.mi_mdta_fused_workspace(C.byref(s)) and p["pack_bytes"] == L.mi_mdta_fused_pack_bytes(C.byref(s))
                        if not p["covered"]:
                            assert p == zeros
                            continue
                        tiles = p["tiles_x"] * p["tiles_y"]
                        assert p["kind"] == kind and p["form"] == ("fourth" if kind == "48_1" and not cfg else "round3")
                        assert p["th"] == 8 and tiles == (H // 8) * (W // 32) and p["S"] == max(1, min(256 // B, tiles // 4))
                        assert 1 <= p["S"] <= tiles and p["grid"] == B * p["S"] and p["block"] == 64 * p["waves"] == 512
                        assert 0 < p["lds"] <= 160 * 1024 and p["pays"] == (p["grid"] >= 192)
                        assert p["part_mult"] == (8 if p["form"] == "fourth" else 1)
                        partial = 4 * (C_ * (C_ // heads) + 2 * C_)                  # heads x c x c Gram + 2 C sums of squares, fp32
                        assert p["workspace"] > p["part_bytes"] >= B * p["S"] * p["part_mult"] * partial
        for dt, ks in ((torch.float32, 3), (torch.bfloat16, 5)):                     # fp32 and 5x5 stay on the chain
            assert ops.mdta_fused_plan((2, 48, 16, 64), 1, ks, dt) == zeros
    monkeypatch.setenv("MI_NO_FUSED_MDTA", "1")                                      # the module paths' off switch answers _ok, not the plan
    s = lib.MdtaShape(32, 48, 1, 128, 128, lib.MI_BF16, 3)
    assert ops.mdta_fused_plan((32, 48, 128, 128), 1)["pays"] and not L.mi_mdta_fused_ok(C.byref(s)) and not L.mi_mdta_fused_pays(C.byref(s))
    out = (C.c_int64 * 16)()
    assert L.mi_mdta_fused_plan(None, out) == -1 and L.mi_mdta_fused_plan(C.byref(s), None) == -1
    assert L.mi_mdta_fused_plan(C.byref(lib.MdtaShape(2, 48, 1, 0, 64, lib.MI_BF16, 3)), out) == -1 and b"bad shape" in L.mi_last_error()


def test_fused_case_tables_reach_every_instance(lib, monkeypatch):
    """The GPU case tables of tests/fused_forms.py, evaluated through the plan on the host, reach every instance the dispatch
    lists of csrc/fused_gdfn.hip can select - each row of FG_INFER_ROWS, FG_TRAIN_ROWS and FG_F8_ROWS, the fourth form with SAVE on
    and off at both widths - each with a ragged and an exact last chunk, bias on and off, both LayerNorm kinds; both MDTA forms
    for every kind that has them; and the launch-plan branches (relabelling on / off, fg4 with S = 1, S = tiles / 2 and an uneven
    capped S, uneven MDTA ranges).  A row added to a list without a case fails here."""
    from image_restoration_amd import ops
    import fused_forms as FF
    want = {FF.tile(*r, SAVE=(e == "train"), F8=(e == "f8")) for e, rows in FF.ladder_rows().items() for r in rows}
    want |= {FF.fourth(c, s) for c in (48, 96) for s in (False, True)}
    seen, splits = {}, set()
    for inst, entry, cfg, shape, pset in FF.GDFN_CASES:
        FF.set_switches(monkeypatch, cfg)
        chunk, bias, kind = FF.PARAMS[pset]
        hidden = FF.HIDDEN[(shape[1], chunk)]
        p = FF.reach(ops, inst, entry, shape, hidden)
        width = 16 if inst[0] == "fourth" else p["pc"]
        assert (hidden % width != 0) == (chunk == "ragged")
        assert shape[0] == 2 or (inst, shape[0]) in ((FF.tile(96, 8, 32, 16, 4), 1),)
        seen.setdefault(inst, set()).update({chunk, "bias" if bias else "no bias", kind})
        if shape[0] == 2 and shape[2] > 8:
            assert p["tiles_x"] >= 2 and p["tiles_y"] >= 2 and shape[3] == 2 * p["tw"] and shape[2] in ((24,) if p["th"] == 8 else (32, 48))
        if inst[0] == "fourth":
            tiles = p["tiles_x"] * p["tiles_y"]
            splits.add("one" if p["S"] == 1 else "half" if p["S"] == tiles // 2 else "other")
        elif p["tw"] == 32 and not cfg and p["grid"] % 16:
            splits.add("no relabelling")
    assert set(seen) == want, (want - set(seen), set(seen) - want)
    for inst, tags in seen.items():
        assert tags >= {"ragged", "exact", "bias", "no bias", "WithBias", "BiasFree"}, (inst, tags)
    assert splits >= {"one", "half", "no relabelling"}
    for inst, shape, pset in FF.XCD_CASES:
        for noxcd in (False, True):
            FF.set_switches(monkeypatch, "", noxcd=noxcd)
            p = FF.reach(ops, inst, "train" if inst[6] else "inference", shape, FF.HIDDEN[(shape[1], FF.PARAMS[pset][0])])
            assert p["xcd_pairs"] == (not noxcd) and p["grid"] % 16 == 0
    assert {s[0] * (s[2] // i[2]) * (s[3] // i[3]) for i, s, _ in FF.XCD_CASES} >= {16, 32}
    inst, cfg, shape, pset, S, tiles = FF.FG4_RANGES
    FF.set_switches(monkeypatch, cfg)
    p = FF.reach(ops, inst, "inference", shape, FF.HIDDEN[(shape[1], FF.PARAMS[pset][0])])
    assert p["S"] == S == 256 // shape[0] < tiles // 2 and p["tiles_x"] * p["tiles_y"] == tiles and tiles % S
    for entry, cfg, shape, hidden in FF.GDFN_REFUSALS:
        FF.set_switches(monkeypatch, cfg)
        assert not ops.gdfn_fused_plan(shape, hidden, entry)["covered"] and ops.gdfn_fused_plan(shape, hidden, "inference")["covered"]
    assert {r[0] for r in FF.GDFN_REFUSALS} == {"train", "f8"}       # (inference has a kernel under every switch string: its refusals are shapes)
    forms, uneven = set(), set()
    for kind, c, heads, cfg, form, shape, bias, ln, (tiles, S) in FF.MDTA_CASES:
        FF.set_switches(monkeypatch, fm_cfg=cfg)
        p = ops.mdta_fused_plan(shape, heads)
        assert (p["kind"], p["form"], p["tiles_x"] * p["tiles_y"], p["S"]) == (kind, form, tiles, S)
        forms.add((kind, form))
        if tiles % S:
            uneven.add((kind, form))
    assert forms == uneven == {("48_1", "fourth"), ("48_1", "round3"), ("96_2", "round3"), ("96_1", "round3")}
    for shape, heads in FF.MDTA_REFUSALS:
        assert not ops.mdta_fused_plan(shape, heads)["covered"]


def test_fused_assertions_pass_on_bf16_arithmetic_and_catch_five_faults(lib):
    """The assertion helper of the GPU tests (fused_forms.assert_half_block, assert_saved) on the CPU, for every distinct
    (C, parameters, shape, tile) of the case tables:
      * it passes on a CPU evaluation of the documented arithmetic (fused_forms.model_half_block, mode "fused") held against the
        modelled chain, and that evaluation stays under HALF of each bar;
      * it fails on each of five injected faults: an interior corner halo pixel dropped per tile, the right-halo column dropped,
        the last hidden channel dropped from project_out, the padding holding b' = W' LN(0) + b instead of 0, the gate halves
        swapped;
      * the cap: every fault, evaluated in pure fp64, exceeds the bar it is meant to trip (fused_forms.FAULT_BAR) by at least 3 x.
        This is what fused_forms.BIAS_SCALE / BETA are chosen for: with the stock 0.1 N biases and 0.2 N beta the padding fault
        moves the branch by 5 - 7 % against its 4 % bar.
    Reference-only figures (pure fp64, worst and best over the table) are in DESIGN.md next to the measured ones."""
    import fused_forms as FF
    figures = {f: [] for f in FF.FAULTS}
    table = FF.fault_table()
    assert len(table) >= 20
    for C_, pset, shape, thw in table:
        sd, kind, hidden = FF.gdfn_state(C_, pset)
        y = FF.gdfn_input(shape)
        ref = FF._oracle_half_block(y, sd, kind)
        assert FF.rel(FF.model_half_block(y, sd, kind, "fp64", thw)[0], ref) < 1e-12       # the model states the oracle's operation
        chain, h0_c, g_c = FF.model_half_block(y, sd, kind, "chain", thw)
        clean, h0, g = FF.model_half_block(y, sd, kind, "fused", thw)
        e_out, e_branch, _ = FF.assert_half_block(clean, chain, y, ref, f"model {C_} {pset} {shape}")
        assert e_out < FF.BAR_OUT / 2 and e_branch < FF.BAR_BRANCH / 2, (C_, pset, shape, e_out, e_branch)
        FF.assert_saved(h0, g, h0_c, g_c, FF.oracle_h0(y, sd, kind))     # (a bf16 ulp of the largest entry apart: inside the bars, not half)
        for fault in FF.FAULTS:
            if fault == "corner" and shape[2] <= thw[0]:
                continue                                             # one tile row: no tile has a diagonal neighbour
            pure = dict(zip(("out", "branch"), FF.errors(FF.model_half_block(y, sd, kind, "fp64", thw, fault)[0], y, ref)))
            bar = {"out": FF.BAR_OUT, "branch": FF.BAR_BRANCH}[FF.FAULT_BAR[fault]]
            figures[fault].append(pure[FF.FAULT_BAR[fault]])
            assert pure[FF.FAULT_BAR[fault]] > 3 * bar, (fault, C_, pset, shape, thw, pure)
            with pytest.raises(AssertionError, match="off the fp64 oracle"):
                FF.assert_half_block(FF.model_half_block(y, sd, kind, "fused", thw, fault)[0], chain, y, ref, fault)
    for fault, v in figures.items():
        print(f"{fault}: {FF.FAULT_BAR[fault]} moved by {min(v):.3f} .. {max(v):.3f} (pure fp64)")


# --------------------------------------------------------------------------- the attention c x c side and chan_sum (mi_attn_small_plan, mi_chan_sum_plan)
ATTN_BS = (1, 2, 8, 32, 160)


def _attn_formulas(B, C_, heads):
    """The launchers' decisions, read from csrc/attn_small.hip."""
    c = C_ // heads
    ct0 = -(-c // 16)
    ct = {5: 6, 7: 8}.get(ct0, ct0)
    cp, rch, Z = 16 * ct, -(-C_ // 16), B * heads
    rpw = min(max(Z * rch // 768, 1), min(8, rch))
    gy = -(-rch // rpw)
    fold = 4 * (cp * (cp + 1) + 2 * cp + rpw * 16 * (cp + 1))
    bwd = 4 * max(2 * 32 * (cp + 1) + 16 * cp + 2 * cp + 8, cp * (cp + 1) + 64 * (cp + 1))
    return {"instance": ct, "promoted": ct != ct0, "padded": cp, "rpw": rpw, "fold_grid_x": Z, "fold_grid_y": gy,
            "last_chunks": rch - (gy - 1) * rpw, "fold_lds": fold, "fold_raised": fold > 65536, "bwd_grid_x": Z,
            "bwd_grid_y": 1 + -(-C_ // 64), "bwd_lds": bwd, "bwd_raised": bwd > 65536, "row_blocks": -(-ct // 4),
            "mtb_vector": C_ % 4 == 0, "wd_vector": c % 4 == 0}


def test_attn_small_plan_sweep(lib):
    """ops.attn_small_plan over C = 1..768, every head count with c <= 128 and five batch sizes: each field is the launcher's
    formula, the LDS fits the 160 KiB of a CU, rpw stays within 1..min(8, chunks), the fold's row groups cover the chunks with a
    non-empty last group, and the instance holds c.  ops.chan_sum_plan likewise over a grid of C and N."""
    from image_restoration_amd import ops
    seen, n = set(), 0
    for C_ in range(1, 769):
        for heads in range(1, C_ + 1):
            if C_ % heads or C_ // heads > 128:
                continue
            for B in ATTN_BS:
                p = ops.attn_small_plan(B, C_, heads)
                assert p == _attn_formulas(B, C_, heads), (B, C_, heads, p)
                rch = -(-C_ // 16)
                assert p["instance"] in (1, 2, 3, 4, 6, 8) and p["padded"] - (32 if p["promoted"] else 16) < C_ // heads <= p["padded"]
                assert max(p["fold_lds"], p["bwd_lds"]) <= 160 * 1024
                assert 1 <= p["rpw"] <= min(8, rch) and 1 <= p["last_chunks"] <= p["rpw"]
                assert (p["fold_grid_y"] - 1) * p["rpw"] + p["last_chunks"] == rch and p["bwd_grid_y"] * 64 - 64 >= C_
                seen.add((p["instance"], p["rpw"], p["fold_raised"], p["bwd_raised"]))
                n += 1
    assert n > 20000 and {s[0] for s in seen} == {1, 2, 3, 4, 6, 8} and {s[1] for s in seen} == set(range(1, 9))
    assert (6, 5, True, False) in seen and (6, 4, False, False) in seen and not any(s[3] for s in seen if s[0] < 8)
    for dt, V in ((torch.float32, 4), (torch.bfloat16, 8)):
        for C_ in (1, 3, 48, 100, 511, 512, 513, 600):
            for N in (1, 7, 1023, 1024, 1025, 4096, 4099, 5000, 5004, 65536, 1 << 20):
                for aligned in (True, False):
                    p = ops.chan_sum_plan(2, C_, N, dt, aligned)
                    splits = max(1, min(512 // C_, -(-N // 1024)))
                    per = -(-(-(-N // splits)) // 8) * 8
                    assert p == {"splits": splits, "per_split": per, "vector": aligned and N % V == 0,
                                 "workspace": lib.lib().mi_chan_sum_workspace(C_, N)}, (C_, N, dt, aligned, p)
                    assert per % 8 == 0 and (splits - 1) * per < N <= splits * per and p["workspace"] >= 4 * splits * C_


def test_attn_small_and_chan_sum_argument_errors(lib):
    """c > 128, C % heads != 0, non-positive extents and null pointers: -1 with their message from the plan and from both entry
    points, before anything touches a GPU (the buffers here are host memory, never read)."""
    L, out = lib.lib(), (C.c_int64 * 16)()
    buf = C.create_string_buffer(64)
    ptr = C.cast(buf, C.c_void_p).value
    assert L.mi_attn_small_plan(2, 48, 1, None) == -1 and b"attn_small_plan: null pointer" in L.mi_last_error()
    for B, C_, heads, msg in ((1, 129, 1, b"channels per head 129 unsupported (1..128)"), (1, 774, 6, b"channels per head 129 unsupported"),
                              (2, 50, 4, b"channels per head 12 unsupported"), (2, 3, 4, b"channels per head 0 unsupported"),
                              (0, 48, 1, b"bad shape B=0 C=48 heads=1"), (2, 0, 1, b"bad shape"), (2, 48, 0, b"bad shape"),
                              (2, 48, -2, b"bad shape"), (-1, 48, 1, b"bad shape")):
        assert L.mi_attn_small_plan(B, C_, heads, out) == -1 and msg in L.mi_last_error(), (B, C_, heads, L.mi_last_error())
        fwd = L.mi_attn_small_fwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, C_, heads, None)
        assert fwd == -1 and msg in L.mi_last_error(), (B, C_, heads)
        bwd = L.mi_attn_small_bwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, C_, heads, None)
        assert bwd == -1 and msg in L.mi_last_error(), (B, C_, heads)
    assert L.mi_attn_small_plan(1, 128, 1, out) == 0 and out[0] == 8 and L.mi_attn_small_plan(2, 48, 1, out) == 0 and out[0] == 3
    for k in range(8):                                   # each required pointer of the fold; Mb and Mtb may be NULL
        a = [ptr] * 10
        a[k] = None
        assert L.mi_attn_small_fwd(*a, 2, 48, 1, None) == -1 and b"mdta: null pointer in the attention fold" in L.mi_last_error(), k
    for k in range(9):                                   # each required pointer of the backward; wdb may be NULL
        a = [ptr] * 10
        a[k] = None
        assert L.mi_attn_small_bwd(*a, 2, 48, 1, None) == -1 and b"mdta: null pointer in the attention backward" in L.mi_last_error(), k
    o4 = (C.c_int64 * 4)()
    assert L.mi_chan_sum_plan(2, 48, 4096, lib.MI_F32, 1, None) == -1 and b"chan_sum_plan: null pointer" in L.mi_last_error()
    assert L.mi_chan_sum_plan(2, 48, 4096, 7, 1, o4) == -1 and b"chan_sum_plan: bad dtype 7" in L.mi_last_error()
    for B, C_, N in ((0, 48, 4096), (2, 0, 4096), (2, 48, 0), (-1, 48, 4096), (2, -48, 4096), (2, 48, -8)):
        assert L.mi_chan_sum_plan(B, C_, N, lib.MI_BF16, 1, o4) == -1 and b"chan_sum_plan: bad shape" in L.mi_last_error(), (B, C_, N)
    assert L.mi_chan_sum_plan(2, 48, 4096, lib.MI_BF16, 1, o4) == 0 and list(o4) == [4, 1024, 1, 768]
    assert L.mi_chan_sum(None, ptr, 2, 48, 4096, lib.MI_F32, 0, ptr, None) == -1 and b"chan_sum: null pointer" in L.mi_last_error()


def test_attn_case_tables_reach_every_plan(lib):
    """The tables of tests/attn_forms.py together reach every instance at an exact and at a padded width and both promotions,
    rpw 1, 2, 3, 5, 7, 8 with a partial last group and the cap at the chunk count, both raised-LDS fold launches and the raised
    backward, both values of each vector-store flag, every row tail the issue names, clamped norms on every third row, and every
    chan_sum plan for each dtype.  Each row names its plan: a threshold that moves in the launcher is a row that lost it."""
    from image_restoration_amd import ops
    import attn_forms as T
    fit, rpws, promoted, raised, flags, partial = set(), set(), set(), set(), set(), set()
    for case in T.ALL_CASES:
        (B, C_, heads), _ = case
        p, c = T.assert_plan(ops, case), C_ // heads
        fit.add((p["instance"], "exact" if c == p["padded"] else "padded"))
        rpws.add(p["rpw"])
        if p["promoted"]:
            promoted.add(p["instance"])
        if p["fold_raised"]:
            raised.add(("fold", p["instance"]))
        if p["bwd_raised"]:
            raised.add(("bwd", p["instance"]))
        if p["last_chunks"] < p["rpw"]:
            partial.add(p["rpw"])
        flags |= {("mtb", p["mtb_vector"]), ("wd", p["wd_vector"])}
    assert {C_ // h for (B, C_, h), _ in T.WIDTH_CASES} == {1, 10, 16, 17, 24, 32, 33, 40, 48, 49, 64, 65, 80, 81, 96, 97, 112, 120, 127, 128}
    assert all(B <= 3 and 1 <= h <= 3 for (B, C_, h), _ in T.WIDTH_CASES)
    assert fit == {(ct, f) for ct in (1, 2, 3, 4, 6, 8) for f in ("exact", "padded")} and promoted == {6, 8}
    assert rpws == {1, 2, 3, 5, 7, 8} and partial >= {3, 5, 7}
    assert raised == {("fold", 6), ("fold", 8), ("bwd", 8)}
    assert flags == {("mtb", True), ("mtb", False), ("wd", True), ("wd", False)}
    (B, C_, heads), _ = T.CHUNK_CASES[-1]                                          # the cap: more asked for than there are chunks
    assert B * heads * -(-C_ // 16) // 768 > -(-C_ // 16) == ops.attn_small_plan(B, C_, heads)["rpw"]
    assert T.CHUNK_CASES[3][0] == (32, 384, 8)                                     # the benchmark's deepest level, batch 32
    cs = [C_ for (B, C_, h), _ in T.WIDTH_CASES]
    assert any(x % 16 for x in cs) and any(x % 4 for x in cs) and any(x % 32 and not x % 4 for x in cs) and 72 in cs
    assert any(T.is_clamp_case(k) and (k[0][1] // k[0][2]) % 16 for k in T.ALL_CASES)           # a clamped row inside a padded fragment
    assert sum(map(T.is_clamp_case, T.ALL_CASES)) == 9 and any(T.is_clamp_case(k) for k in T.CHUNK_CASES)
    assert all(v <= 5e-5 for v in T.BOUND.values()) and all(T.BOUND[k] == 8 * T.MEASURED[k] for k in T.BOUND)
    plans = {}
    for (B, C_, N), per_dtype in T.CHAN_SUM_CASES:
        for dt in per_dtype:
            for aligned in (True, False):
                p = T.assert_chan_sum_plan(ops, B, C_, N, dt, aligned)
                plans.setdefault(dt, set()).add((p["splits"] > 1, p["vector"]))
    assert all(v == {(False, True), (False, False), (True, True), (True, False)} for v in plans.values()) and len(plans) == 2


def test_attn_bounds_admit_a_correct_fp32_evaluation(lib):
    """On every row of both tables: Reference 1 agrees with fp64 autograd (Reference 2) to 1e-10, and autograd rejects the
    projection terms D1 / D2 on a clamped norm; the kernels' arithmetic evaluated in torch fp32 on the CPU, with every contraction
    in a permuted order, passes Family B's assertions and Family A's bit for bit.  The bounds ask nothing that correct fp32
    arithmetic cannot give, and Family A's expected values are what the formulas give."""
    from image_restoration_amd import ops
    import attn_forms as T
    worst = {}
    for n, case in enumerate(T.ALL_CASES):
        plan, who = T.assert_plan(ops, case), T.case_id(case)
        assert max(T.reference_gap(case).values()) <= T.REFERENCE_GAP, who
        if T.is_clamp_case(case) and case[0][1] // case[0][2] >= 4:
            assert max(T.reference_gap(case, d_on_clamp=True).values()) > 1e3 * T.REFERENCE_GAP, who
        s = T.float_inputs(case)
        got = T.evaluate_fp32(s, plan, seed=n)
        for ratios, _ in (T.assert_float_fwd(got, s, who), T.assert_float_bwd(got, s, who)):
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
        e = T.exact_inputs(case)
        got = T.evaluate_fp32(e, plan, seed=n)
        T.assert_exact_fwd(got, e, who)
        T.assert_exact_bwd(got, e, who)
    assert set(worst) == set(T.BOUND) and max(worst.values()) <= 1.0, worst
    assert max(worst.values()) >= 1.0 / 16, worst          # (and the bounds are of the arithmetic's own size, not idle)


def test_attn_assertions_catch_five_deliberate_faults(lib):
    """Five faults of the kind the kernels' padding, row groups, clamps and store tails can have, applied to the fp32 evaluation
    on the CPU, on every row of the tables where each can occur: each fails its assertion.

    Contrast with the bar that guarded these kernels before (test_attention_small_kernels_at_padded_and_wide_heads: one
    max-over-tensor ratio of 5e-5 per tensor, behind two Grams, three GEMMs and LayerNorm, at rpw = 1 and unclamped norms only):
    the partial row group and the clamp branch were never run, and the bf16 copies never read back."""
    from image_restoration_amd import ops
    import attn_forms as T
    caught = dict.fromkeys(T.FAULTS, 0)
    for case in T.ALL_CASES:
        (B, C_, heads), _ = case
        plan, who, c = T.assert_plan(ops, case), T.case_id(case), C_ // heads
        s = T.float_inputs(case)
        applicable = {"pad_in_softmax": c % 16 != 0, "partial_group_unwritten": plan["last_chunks"] < plan["rpw"],
                      "d_on_clamp": s.clamp and c >= 4, "g1t_shift": c % 4 != 0 and c >= 4, "mtb_tail": C_ % 4 != 0}
        match = {"pad_in_softmax": "A off", "partial_group_unwritten": "M has elements never written",
                 "d_on_clamp": "D1 / D2 not zero on a clamped norm", "g1t_shift": "lower-right block is not G1 transposed",
                 "mtb_tail": "Mtb is not Mb transposed"}
        for fault in T.FAULTS:
            if not applicable[fault]:
                continue
            got = T.evaluate_fp32(s, plan, fault=fault)
            with pytest.raises(AssertionError, match=match[fault]):
                T.assert_float_fwd(got, s, who)
                T.assert_float_bwd(got, s, who)
            caught[fault] += 1
    assert min(caught.values()) >= 3, caught


# --------------------------------------------------------------------------- the 3x3 glue (mi_conv3x3_plan, mi_glue3x3_plan, mi_pixel_shuffle2_plan, mi_copy_rows_plan)
def _cdiv(a, b):
    return -(-a // b)


def _conv3x3_formulas(B, M, K, H, W):
    """The launchers' decisions, read from csrc/conv3x3.hip."""
    mt = 1 if M <= 16 else 2 if M <= 32 else 4
    twp = 64 if W > 32 else 32 if W > 16 else 16
    tr = 256 // twp
    tx, ty, cot, ch = _cdiv(W, twp), _cdiv(H, tr), _cdiv(M, 16 * mt), _cdiv(K, 16)
    swap = _cdiv(K, 64) * 64 * _cdiv(M, 16) * 16 < _cdiv(M, 64) * 64 * _cdiv(K, 16) * 16
    rows, cols = (K, M) if swap else (M, K)
    gx, gy = _cdiv(cols, 16), _cdiv(rows, 64)
    splits = min(max(min(_cdiv(1024, gx * gy), B * tx * ty // 2), 1), 4096)
    return {"mt": mt, "twp": twp, "tr": tr, "tiles_x": tx, "tiles_y": ty, "co_tiles": cot, "chunks": ch,
            "pack_bytes": cot * ch * 5 * mt * 512 * 2, "w_swap": swap, "w_rows": rows, "w_cols": cols, "w_splits": splits,
            "w_grid_x": gx, "w_grid_y": gy, "w_workspace": splits * M * K * 36}


def test_glue_plans_from_first_principles(lib):
    """The four plan queries against the launchers' rules written out here, over grids of shapes, against the sizing entry points
    that existed before them, and at a few absolute figures so that this helper cannot drift with the code."""
    from image_restoration_amd import ops
    L = lib.lib()
    seen = set()
    for B in (1, 2, 3, 18):
        for M in (1, 3, 16, 17, 32, 33, 48, 64, 65, 96, 512):
            for K in (1, 3, 15, 16, 17, 33, 48, 64, 96, 256):
                for H, W in ((1, 8), (15, 16), (17, 16), (8, 24), (9, 32), (4, 40), (5, 72), (7, 128), (256, 256)):
                    p = ops.conv3x3_plan(B, M, K, H, W)
                    assert p == _conv3x3_formulas(B, M, K, H, W), (B, M, K, H, W, p)
                    assert p["pack_bytes"] == L.mi_conv3x3_pack_bytes(M, K) and p["w_workspace"] == L.mi_conv3x3_wgrad_workspace(B, M, K, H, W)
                    assert p["tiles_x"] * p["twp"] >= W > (p["tiles_x"] - 1) * p["twp"] and p["tiles_y"] * p["tr"] >= H > (p["tiles_y"] - 1) * p["tr"]
                    assert p["co_tiles"] * 16 * p["mt"] >= M and p["chunks"] * 16 >= K and {p["w_rows"], p["w_cols"]} == {M, K}
                    assert 1 <= p["w_splits"] <= max(1, B * p["tiles_x"] * p["tiles_y"] // 2)
                    seen.add((p["mt"], p["twp"], p["w_swap"]))
    assert len(seen) == 18
    # absolute figures: Restormer's patch embedding (3 -> 48 at 128 x 128, batch 2) and a Downsample body (48 -> 24)
    assert ops.conv3x3_plan(2, 48, 3, 128, 128) == {
        "mt": 4, "twp": 64, "tr": 4, "tiles_x": 2, "tiles_y": 32, "co_tiles": 1, "chunks": 1, "pack_bytes": 20480, "w_swap": False,
        "w_rows": 48, "w_cols": 3, "w_splits": 64, "w_grid_x": 1, "w_grid_y": 1, "w_workspace": 64 * 48 * 3 * 36}
    p = ops.conv3x3_plan(18, 512, 256, 1, 8)
    assert (p["w_splits"], p["w_grid_x"], p["w_grid_y"], p["w_swap"], p["twp"], p["tr"]) == (8, 16, 8, False, 16, 16)
    p = ops.conv3x3_plan(1, 16, 64, 8, 32)
    assert (p["w_swap"], p["w_rows"], p["w_cols"], p["mt"], p["twp"], p["chunks"], p["w_splits"]) == (True, 64, 16, 1, 32, 4, 1)

    for dt in (torch.float32, torch.bfloat16):
        for planes in (1, 3, 9, 96, 2048, 4096):
            for H in (1, 7, 8, 9, 17, 33, 256):
                for W in (1, 3, 8, 16, 20, 32, 64, 128, 256, 500, 512):
                    for aligned in (True, False):
                        p = ops.glue3x3_plan(planes, H, W, dt, aligned)
                        fast = aligned and W in (16, 32, 64, 128, 256)
                        if fast:
                            G = 64 // (W // 4)
                            band = 32 if planes * _cdiv(H, 32) // G >= 4096 else 16 if planes * _cdiv(H, 16) // G >= 4096 else 8
                            blocks = _cdiv(planes * _cdiv(H, band), 4 * G)
                            want = {"fast": True, "lpr": W // 4, "band": band, "bands": _cdiv(H, band), "blocks_im2col": blocks, "blocks_col2im": blocks}
                        else:
                            n = planes * H * W
                            want = {"fast": False, "lpr": 0, "band": 0, "bands": 0, "blocks_im2col": min(9 * n // 256 + 1, 65536),
                                    "blocks_col2im": min(n // 256 + 1, 65536)}
                        assert p == want, (planes, H, W, dt, aligned, p)
    assert ops.glue3x3_plan(2048, 17, 256, torch.bfloat16) == {"fast": True, "lpr": 64, "band": 16, "bands": 2, "blocks_im2col": 1024, "blocks_col2im": 1024}
    assert ops.glue3x3_plan(2048, 33, 256, torch.bfloat16)["band"] == 32 and ops.glue3x3_plan(2047, 33, 256, torch.bfloat16)["band"] == 16
    assert ops.glue3x3_plan(6, 128, 128, torch.float32) == {"fast": True, "lpr": 32, "band": 8, "bands": 16, "blocks_im2col": 12, "blocks_col2im": 12}
    assert ops.glue3x3_plan(8, 500, 500, torch.bfloat16) == {"fast": False, "lpr": 0, "band": 0, "bands": 0, "blocks_im2col": 65536, "blocks_col2im": 7813}

    for dt, V in ((torch.float32, 4), (torch.bfloat16, 8)):
        for W in (1, 4, 6, 8, 12, 16, 601):
            for bs_in in (0, 4 * 3 * 5 * W + 8, 4 * 3 * 5 * W + 1):
                for bs_out in (0, 4 * 3 * 5 * W + 16, 4 * 3 * 5 * W + 4):
                    for aligned in (True, False):
                        dense = 4 * 3 * 5 * W
                        v = V if aligned and W % V == 0 and (bs_in or dense) % V == 0 and (bs_out or dense) % V == 0 else 1
                        total = 2 * 3 * 2 * 5 * (W // v)
                        assert ops.pixel_shuffle2_plan(2, 3, 5, W, bs_in, bs_out, dt, aligned) == \
                            {"vector": v, "total": total, "blocks": min(_cdiv(total, 256), 16384)}, (dt, W, bs_in, bs_out, aligned)
                        rs_in, rs_out = bs_in and bs_in // 4, bs_out and bs_out // 4          # copy_rows: rows of L = 15 W
                        Ln = 15 * W
                        v = V if aligned and Ln % V == 0 and (rs_in or Ln) % V == 0 and (rs_out or Ln) % V == 0 else 1
                        assert ops.copy_rows_plan(7, Ln, rs_in, rs_out, dt, aligned) == \
                            {"vector": v, "total": 7 * (Ln // v), "blocks": min(_cdiv(7 * (Ln // v), 256), 16384)}, (dt, Ln, rs_in, rs_out, aligned)
    assert ops.pixel_shuffle2_plan(2, 3, 600, 601, 0, 0, torch.bfloat16) == {"vector": 1, "total": 4327200, "blocks": 16384}
    assert ops.pixel_shuffle2_plan(32, 48, 64, 64, 0, 0, torch.bfloat16) == {"vector": 8, "total": 1572864, "blocks": 6144}
    assert ops.copy_rows_plan(32, 96 * 128 * 128, 192 * 128 * 128, 0, torch.bfloat16) == {"vector": 8, "total": 6291456, "blocks": 16384}
    assert ops.copy_rows_plan(2, 45, 90, 90, torch.float32) == {"vector": 1, "total": 90, "blocks": 1}


def test_glue_plan_argument_errors(lib):
    """Null pointers, bad dtype codes and bad shapes: -1 with their message, nothing launched."""
    L = lib.lib()
    o = (C.c_int64 * 16)()
    assert L.mi_conv3x3_plan(2, 48, 3, 16, 16, None) == -1 and b"conv3x3_plan: null pointer" in L.mi_last_error()
    for B, M, K in ((0, 48, 3), (2, 0, 3), (2, 48, 0), (-1, 48, 3)):
        assert L.mi_conv3x3_plan(B, M, K, 16, 16, o) == -1 and b"conv3x3_plan: bad shape" in L.mi_last_error(), (B, M, K)
    for H, W in ((0, 16), (16, 0), (16, 12), (16, 4), (-1, 16)):                 # where mi_conv3x3_ok refuses
        assert not L.mi_conv3x3_ok(H, W, lib.MI_BF16)
        assert L.mi_conv3x3_plan(2, 48, 3, H, W, o) == -1 and b"conv3x3_plan: plane not covered" in L.mi_last_error(), (H, W)
    assert L.mi_conv3x3_plan(2, 48, 3, 1, 8, o) == 0 and list(o)[:7] == [4, 16, 16, 1, 1, 1, 1]
    assert L.mi_glue3x3_plan(3, 8, 16, lib.MI_BF16, 1, None) == -1 and b"glue3x3_plan: null pointer" in L.mi_last_error()
    assert L.mi_glue3x3_plan(3, 8, 16, 7, 1, o) == -1 and b"glue3x3_plan: bad dtype 7" in L.mi_last_error()
    for planes, H, W in ((0, 8, 16), (3, 0, 16), (3, 8, 0), (-3, 8, 16)):
        assert L.mi_glue3x3_plan(planes, H, W, lib.MI_F32, 1, o) == -1 and b"glue3x3_plan: bad shape" in L.mi_last_error(), (planes, H, W)
    assert L.mi_glue3x3_plan(3, 8, 16, lib.MI_F32, 1, o) == 0 and list(o)[:6] == [1, 4, 8, 1, 1, 1]
    assert L.mi_pixel_shuffle2_plan(2, 3, 5, 16, 0, 0, lib.MI_BF16, 1, None) == -1 and b"pixel_shuffle2_plan: null pointer" in L.mi_last_error()
    assert L.mi_pixel_shuffle2_plan(2, 3, 5, 16, 0, 0, 9, 1, o) == -1 and b"pixel_shuffle2_plan: bad dtype 9" in L.mi_last_error()
    for a in ((0, 3, 5, 16, 0, 0), (2, 0, 5, 16, 0, 0), (2, 3, 0, 16, 0, 0), (2, 3, 5, 0, 0, 0), (2, 3, 5, 16, -8, 0), (2, 3, 5, 16, 0, -8)):
        assert L.mi_pixel_shuffle2_plan(*a, lib.MI_BF16, 1, o) == -1 and b"pixel_shuffle2_plan: bad shape" in L.mi_last_error(), a
    assert L.mi_copy_rows_plan(2, 16, 0, 0, lib.MI_BF16, 1, None) == -1 and b"copy_rows_plan: null pointer" in L.mi_last_error()
    assert L.mi_copy_rows_plan(2, 16, 0, 0, 3, 1, o) == -1 and b"copy_rows_plan: bad dtype 3" in L.mi_last_error()
    for a in ((0, 16, 0, 0), (2, 0, 0, 0), (2, 16, -1, 0), (2, 16, 0, -1)):
        assert L.mi_copy_rows_plan(*a, lib.MI_F32, 1, o) == -1 and b"copy_rows_plan: bad shape" in L.mi_last_error(), a
    assert L.mi_copy_rows_plan(2, 16, 0, 0, lib.MI_F32, 1, o) == 0 and list(o)[:3] == [4, 8, 1]


def test_glue_case_tables_reach_every_instance(lib):
    """The tables of tests/glue_forms.py reach every instance the launchers can select and nothing unknown, each value of each
    dimension at each instance, and every loop state; each row names its plan, so a threshold that moves is a row that lost it."""
    from image_restoration_amd import ops
    import glue_forms as T
    seen = {t: {} for t in T.TABLES}
    for t, rows in T.TABLES.items():
        for r in rows:
            seen[t].setdefault(T.instance(r, T.reach(ops, r)), []).append(r)
    conv = seen["conv"]
    assert set(conv) == T.C3_INSTANCES
    for (mt, twp), rows in conv.items():
        tr = 256 // twp
        assert {r["wkind"] for r in rows} == {k for k, _ in T.C3_W[twp]} and {r["W"] for r in rows} == {w for _, w in T.C3_W[twp]}
        assert {r["H"] for r in rows} == {1, tr - 1, tr, tr + 1, 2 * tr + 1} and {r["K"] for r in rows if not r["transpose"]} == {1, 3, 15, 16, 17, 33}
        assert {r["M"] for r in rows} == set(T.C3_M[mt]) and {r["B"] for r in rows} == {1, 3}
        assert {(r["bias"], r["res"]) for r in rows} == set(T.EPILOGUES)
        assert sum(r["transpose"] and r["M"] != r["K"] for r in rows) >= 2
    assert {r["W"] for r in conv[(4, 64)]} == {64, 40, 72, 128} and {r["W"] for r in conv[(1, 16)]} == {16, 8} and {r["W"] for r in conv[(2, 32)]} == {32, 24}
    assert {(r["mt"], r["twp"]) for r in T.CONV_CASES if T.module_route(r)} == T.C3_INSTANCES      # the module route runs all nine too
    wg = seen["wgrad"]
    assert set(wg) == T.C3W_INSTANCES
    for (twp, swap), rows in wg.items():
        assert {r["rows"] for r in rows} >= ({17, 33, 64, 65} if swap else {1, 16, 17, 33, 64, 65}) and {r["cols"] for r in rows} >= {1, 15, 16, 17}
        assert {(r["tiles"], r["splits"]) for r in rows} >= {(1, 1), (3, 1), (4, 2), (5, 2), (7, 3), (6, 3), (2, 1)}
        assert any(r["loop"] == "3x2/3" and r["B"] == 3 for r in rows)                 # 3 images x 2 tiles: each split alternates images
        assert any(r["loop"] == "past_h" and r["H"] % (256 // twp) for r in rows) and sum(r["accumulate"] for r in rows) >= 2
    assert not any(ops.conv3x3_plan(1, c, r, 8, 16)["w_swap"] for r in (1, 16) for c in range(1, 65))   # (no swap puts <= 16 rows in the row role)
    by_blocks = [r for r in T.WGRAD_CASES if r["loop"] == "by_blocks"]
    assert len(by_blocks) == 1 and by_blocks[0]["splits"] == 8 < by_blocks[0]["tiles"] // 2
    for t in ("im2col", "col2im"):
        g = seen[t]
        assert set(g) == T.G3_STREAM | T.G3_BANDS | {("general", "f32"), ("general", "bf16")}, t
        for lpr in (4, 8, 16, 32, 64):
            rows = [r for k in T.G3_STREAM if k[0] == lpr for r in g[k]]
            assert {r["H"] for r in rows} == {1, 7, 8, 9, 17} and all(r["idle"] and r["band"] == 8 and r["W"] == 4 * lpr for r in rows)
        assert all(r["dtype"] == "bf16" and r["device_ref"] and r["B"] * r["C"] == 2048 for k in T.G3_BANDS for r in g[k])
        assert ops.glue3x3_plan(2047, 17, 256, torch.bfloat16)["band"] == 8                 # 2048 is the smallest plane count for both
        gen = g[("general", "f32")] + g[("general", "bf16")]
        assert {(r["W"], r["H"]) for r in gen} >= {(W, H) for W in (1, 3, 8, 20, 24) for H in (1, 2, 5)}
        assert {(r["dtype"], r["x_off"], r["out_off"]) for r in gen if r["W"] == 64} == {(d, a, b) for d in T.DTYPES for a, b in ((1, 0), (0, 1))}
        assert sum(r["trips"] == 2 for r in gen) == 1
    assert {(r["bias"], r["res"]) for r in T.COL2IM_CASES if r["form"] == "stream"} == set(T.EPILOGUES)
    assert {(r["bias"], r["res"]) for r in T.COL2IM_CASES if r["form"] == "general"} == set(T.EPILOGUES)
    assert all(r["C"] > 1 for r in T.COL2IM_CASES) and any(r["B"] > 1 and r["bias"] for r in T.COL2IM_CASES)
    sh = seen["shuffle"]
    assert set(sh) == T.PS_INSTANCES
    for (form, un, dt), rows in sh.items():
        if form == "element":
            assert {r["why"] for r in rows} == {"width", "in_ptr", "out_ptr", "stride"}
    assert sum(r["trips"] == 2 for r in T.SHUFFLE_CASES) == 1
    cr = seen["copy"]
    assert set(cr) == T.CR_INSTANCES
    assert all({r["why"] for r in rows} == {"tail", "in_ptr", "out_ptr", "stride"} for (form, dt), rows in cr.items() if form == "element")


def _glue_calls(tables):
    from image_restoration_amd import ops
    import glue_forms as T
    for t in tables:
        for r in T.TABLES[t]:
            if not r.get("device_ref"):
                yield t, r, T.BUILD[t](ops, r, "cpu")


def test_glue_rows_meet_the_integer_precondition(lib):
    """Every expected value of every row is an integer its output dtype holds exactly (the builders assert it on the reference
    alone; none is skipped), the operands lie inside NaN and a result equal to the reference passes the comparison and the guards.
    The rows whose reference is computed on the device (the two tall-band cases and the grid-cap cases) are bounded by their
    ranges: a tap of x in [-2, 2], or nine z in [-3, 3] plus a bias and a residual in [-8, 8], at most 43."""
    import glue_forms as T
    n, peak = 0, {}
    for t, r, c in _glue_calls(T.TABLES):
        T.precondition(c.ref, c.out.dtype, T.case_id(r))
        peak[t] = max(peak.get(t, 0.0), float(c.ref.abs().max()))
        assert bool(c.out_buf.isnan().all())
        c.reset()
        c.out.copy_(c.ref)
        c.check()
        n += 1
    big = [r for rows in T.TABLES.values() for r in rows if r.get("device_ref")]
    assert n + len(big) == sum(map(len, T.TABLES.values())) and len(big) == 6
    assert all(r["dtype"] == "bf16" and 9 * 3 + 8 + 8 <= 256 for r in big)
    assert peak["conv"] <= 256 and peak["wgrad"] < 2 ** 24 and peak["col2im"] <= 43, peak


def test_glue_assertions_catch_deliberately_wrong_results(lib):
    """Eight alterations of the kind these kernels can have - a halo column at a tile seam read as zero, a row-end neighbour taken
    from the adjacent row, taps 0 and 8 exchanged, the last partial channel chunk dropped, one split's partial sum left out of dw,
    the column phases of a shuffle exchanged, a band's halo row read as zero, the bias of another plane - applied to the reference
    of every row where each can occur: the comparison fails each time.  And one stray write fails the guard check.

    Contrast with the bar these kernels had (tests/test_gpu_conv3x3.py: one scalar, max|delta| / max|ref| < 1e-2 on random normal
    data, at five of the nine forward instances; the layout kernels behind whole modules only): any error under a hundredth of
    the largest output passes it, and it names no element; here one unit in one element fails, with its tile, chunk or band."""
    import glue_forms as T
    caught = dict.fromkeys(T.FAULTS, 0)
    for t, r, c in _glue_calls({tb for tb, _ in T.FAULTS.values()}):
        for name, (table, fault) in T.FAULTS.items():
            if table != t or not T.fault_applies(name, r, c.plan):
                continue
            wrong = fault(c)
            assert wrong.shape == c.ref.shape
            c.reset()
            c.out.copy_(wrong)
            with pytest.raises(AssertionError, match="elements differ; first at"):
                c.check()
            caught[name] += 1
    assert min(caught.values()) >= 3, caught
    _, r, c = next(_glue_calls(["conv"]))
    c.reset()
    c.out.copy_(c.ref)
    c.check()
    c.out_buf[c.out.storage_offset() - 1] = 1.0                                # one element, in the guard channel before image 0
    with pytest.raises(AssertionError, match="1 elements outside the output were written"):
        c.check()
    c.reset()
    c.out.copy_(c.ref)
    c.out[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 elements of the output were never written"):
        c.check()
