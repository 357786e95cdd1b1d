"""CPU checks of DRSformer's transformer block: the fp64 restatement (tests/drs_ref.py) against the fixtures captured from the
reference (tools/capture_golden_drs.py), the native modules' state_dict against the reference's, and the TKSA / MSFN sizing
entry points without a GPU."""
import ctypes as C
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import drs_ref as D  # noqa: E402
from oracle.fixtures import check, load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_drs", os.path.join(ROOT, "tools", "capture_golden_drs.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import _lib
    return _lib


def run_ref(name, masks=None):
    kind, dim, heads, factor, bias, ln_type, bhw, seed = G.CASES[name]
    shapes = G.case_shapes(kind, dim, heads, factor, bias, ln_type)
    sd = {k: v.double().requires_grad_(True) for k, v in D.make_state(shapes, seed).items()}
    x, cot = G.case_io(dim, bhw, seed)
    x = x.double().requires_grad_(True)
    if kind == "tksa":
        y, _ = D.tksa(x, sd, heads, masks)
    elif kind == "msfn":
        y = D.msfn(x, sd)
    else:
        y, _ = D.stb(x, sd, heads, masks)
    y.backward(cot.double())
    return y, x.grad, {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name):
    gold = load(name)
    y, dx, grads = run_ref(name)
    check("y", y, gold, 1e-9, what=name + " ")
    check("dx", dx, gold, 1e-9, what=name + " ")
    names = {k[2:-4] for k in gold.files if k.startswith("g.") and k.endswith(".sub")}
    assert names == set(grads), f"{name}: gradient set differs from the fixture"
    for k, g in grads.items():
        check("g." + k, g, gold, 1e-9, what=name + " ")
    if G.CASES[name][0] != "msfn":
        assert {f"attn{m}" for m in range(1, 5)} <= {k.split(".")[-1] for k in grads}


def test_topk_sizes_are_the_reference_expressions():
    from image_restoration_amd import ops
    assert D.topk_sizes(48) == (24, 32, 36, 38) == ops.tksa_topk(48)
    assert D.topk_sizes(96) == (48, 64, 72, 76) == ops.tksa_topk(96)


def test_topk_masks_rank_ties_by_lower_index():
    S = torch.tensor([[[[1.0, 3.0, 3.0, 2.0, 3.0]]]], dtype=torch.float64)
    m = D.topk_masks(S, (1, 2, 3, 4))
    assert m[0].tolist() == [[[[False, True, False, False, False]]]]
    assert m[1].tolist() == [[[[False, True, True, False, False]]]]
    assert m[2].tolist() == [[[[False, True, True, False, True]]]]
    assert m[3].tolist() == [[[[False, True, True, True, True]]]]


def test_native_modules_have_reference_keys_and_refuse_cpu(lib):
    from image_restoration_amd import drsformer as N
    keys = load("drs_stb_keys")
    for tag, args in (("withbias", (48, 1, 2.66, False, "WithBias")), ("biasfree_bias", (96, 2, 2.66, True, "BiasFree"))):
        blk = N.TransformerBlock(*args)
        sd = blk.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]]
        blk.load_state_dict(D.make_state(D.stb_shapes(*args), seed=5))
    with pytest.raises(RuntimeError, match="MI355X only"):
        blk(torch.zeros(1, 96, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        N.Attention(48, 1, False)(torch.zeros(1, 48, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        N.FeedForward(48, 2.66, False)(torch.zeros(1, 48, 8, 8))


def test_sizing_entry_points_without_gpu(lib):
    from image_restoration_amd import ops
    L = lib
    saved, ws = ops.tksa_sizes(2, 48, 1, 16, 16, torch.float32, (24, 32, 36, 38))
    # qkv0 and qkv (3C planes each) plus the c x c scores the masks are ranked from
    assert saved >= 2 * 2 * 144 * 256 * 4 + 2 * 48 * 48 * 4 and ws > 0
    assert ops.tksa_sizes(2, 240, 2, 16, 16, torch.bfloat16, ops.tksa_topk(120))[0] > 0
    assert ops.tksa_sizes(2, 121, 1, 16, 16, torch.float32, (60, 80, 90, 96)) == (0, 0)
    assert b"channels per head 121" in L.lib().mi_last_error()
    for bad in ((0, 32, 36, 38), (24, 32, 36, 49)):
        assert ops.tksa_sizes(2, 48, 1, 16, 16, torch.float32, bad) == (0, 0)
        assert b"outside 1..c" in L.lib().mi_last_error()
    assert ops.tksa_sizes(2, 50, 4, 16, 16, torch.float32, (6, 8, 9, 10)) == (0, 0)
    s = L.MsfnShape(2, 48, 127, 16, 16, L.MI_BF16)
    # h0, a, b and y: 2h planes each
    assert L.lib().mi_msfn_saved_bytes(C.byref(s)) >= 4 * 2 * 254 * 256 * 2
    assert L.lib().mi_msfn_workspace(C.byref(s)) > 0
    assert L.lib().mi_msfn_saved_bytes(C.byref(L.MsfnShape(2, 48, 0, 16, 16, L.MI_F32))) == 0
