"""CPU checks of the SFHformer FFN / TokenMixer_For_Local restatement (tests/sfh_ffn_ref.py): both of its forms against the fixtures
captured from the reference (tools/capture_golden_sfh_ffn.py), its device form (one segmented tensor, stencils as sums of shifted
planes) against the formula form in fp64, the key lists against the modules' state_dicts, and the committed bounds table against
what tools/sfh_ffn_bounds.py computes."""
import importlib.util
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import sfh_ffn_ref as R  # noqa: E402
from oracle.fixtures import load  # noqa: E402


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_golden_sfh_ffn", os.path.join(ROOT, "tools", "capture_golden_sfh_ffn.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _capture_module()


@pytest.mark.parametrize("device", [False, True], ids=["formula", "device"])
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_matches_reference_fixture(name, device):
    """Both forms on the float32 state and inputs, at 1e-9 evaluated in fp64 and at 1e-4 in float32 arithmetic; every tensor of the
    fixture (y, dx and every parameter gradient) is present and non-zero."""
    kind, dim, bhw, seed = G.CASES[name]
    gold = load(name)
    x, cot = G.case_io(dim, bhw, seed)
    sd = G.case_state(kind, dim, seed)
    got = R.run(kind, x, cot, sd, device=device)
    names = {k[:-4] for k in gold.files if k.endswith(".sub")}
    assert names == set(got) == R.tensors(kind), f"{name}: tensor set differs from the fixture"
    for k, v in got.items():
        R.check(k, v, gold, 1e-9, what=name + " ")
    assert all(float(v.abs().max()) > 0 for v in got.values())
    for k, v in R.run(kind, x, cot, sd, torch.float32, device=device).items():
        R.check(k, v, gold, 1e-4, what=name + " fp32 ")


def test_the_fixtures_are_the_cases_the_issue_names():
    want = {"sfh_ffn_d4": ("ffn", 4, (2, 9, 11)), "sfh_ffn_d6": ("ffn", 6, (1, 8, 34)), "sfh_ffn_d32": ("ffn", 32, (1, 16, 12)),
            "sfh_local_d4": ("local", 4, (2, 9, 11)), "sfh_local_d6": ("local", 6, (1, 5, 34))}
    assert {k: v[:3] for k, v in G.CASES.items()} == want
    biggest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.startswith("sfh_fu_") and "bounds" not in f)
    for name in want:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= biggest, name


@pytest.mark.parametrize("name", list(R.PARITY_CASES))
def test_device_form_equals_formula_form_in_fp64(name):
    """Every parity case: the device form IS the function, to 1e-11 in every tensor."""
    kind, sd, x, cot = R.parity_io(name)
    a, b = R.run(kind, x, cot, sd), R.run(kind, x, cot, sd, device=True)
    assert set(a) == set(b) == R.tensors(kind)
    for k in a:
        assert R.rel_err(b[k], a[k]) <= 1e-11, (name, k, R.rel_err(b[k], a[k]))


def test_the_parity_cases_cover_the_tile_seams_of_the_kernels_built():
    """The case list against the plan the library reports (no GPU): the tile it was stated for, one-tile, one-past, more tiles than
    splits in both row forms, planes under every halo, s = 1 and an odd s."""
    import __graft_entry__ as g
    g.build()
    from image_restoration_amd import ops
    plans = {n: (ops.sfh_ffn_plan if k == "ffn" else ops.sfh_local_plan)(*shape) for n, (k, shape, _) in R.PARITY_CASES.items()}
    assert all((p["tile_w"], p["tile_h"]) == (64, 16) for p in plans.values())
    assert (plans["tile"]["tiles_x"], plans["tile"]["tiles_y"]) == (1, 1) and R.PARITY_CASES["tile"][1][2:] == (16, 64)
    assert (plans["tile_plus_1"]["tiles_x"], plans["tile_plus_1"]["tiles_y"]) == (2, 2)
    for n in ("ragged", "loc_ragged"):
        p, (H, W) = plans[n], R.PARITY_CASES[n][1][2:]
        assert p["tiles_x"] == 3 and W % 64 and H % 16 and p["tiles_x"] * p["tiles_y"] > p["splits"] == 16
    assert R.PARITY_CASES["ragged"][1][3] % 4 == 0 and R.PARITY_CASES["loc_ragged"][1][3] % 4
    assert plans["tiny"]["halo"] == (0, 1, 2, 3) and plans["loc_tiny"]["halo"] == (1, 2)
    assert {plans[n]["segment_width"] for n in ("dim2", "dim6", "wide")} == {1, 3, 32}
    assert R.PARITY_CASES["k7"][1][2:] == (7, 7) and R.PARITY_CASES["b3"][1][0] == 3


def test_modules_have_the_reference_keys_and_load_a_checkpoint_slice():
    from image_restoration_amd import sfhformer as N
    import image_restoration_amd
    for cls in ("FFN", "TokenMixer_For_Local"):
        assert getattr(image_restoration_amd, cls) is getattr(N, cls) and cls in image_restoration_amd.__all__ and cls in N.__all__
    keys = load("sfh_ffn_keys")
    assert len(G.KEY_CASES) == 4
    for tag, kind, args in G.KEY_CASES:
        mod = getattr(N, G.CLASSES[kind])(**args)
        sd = mod.state_dict()
        assert list(sd) == [str(k) for k in keys[tag + ".keys"]]
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in keys[tag + ".shapes"]]
        assert [k for k, _ in mod.named_buffers()] == [str(k) for k in keys[tag + ".buffers"]] == []
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_dict_layout(kind, args["dim"])
        state = R.make_state(kind, args["dim"], 5)
        mod.load_state_dict(state, strict=True)
        assert all(torch.equal(mod.state_dict()[k], v) for k, v in state.items())
    assert list(N.FFN(4).state_dict()) == list(R.FFN_PARAMS) and list(N.TokenMixer_For_Local(4).state_dict()) == list(R.LOCAL_PARAMS)


def test_bounds_table_is_the_host_error_of_the_device_form():
    """The committed bounds are what tools/sfh_ffn_bounds.py computes (three cheap cases recomputed here), one entry per case, dtype
    and tensor; fp32 entries are of fp32 size, bf16 storage costs y and dx 2^-9-sized errors."""
    bounds = load("sfh_ffn_bounds")
    for name in ("tiny", "row", "dim6"):
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            errs, _ = R.host_errors(name, dtype)
            for k, v in errs.items():
                assert v / 3 <= float(bounds[f"{name}.{tag}.{k}"]) <= 3 * v, (name, tag, k)   # (summation order varies by host)
    n = 0
    for name, (kind, _, _) in R.PARITY_CASES.items():
        for k in R.tensors(kind):
            assert 0 <= float(bounds[f"{name}.fp32.{k}"]) < 1e-5, (name, k)
            assert 0 <= float(bounds[f"{name}.bf16.{k}"]) < 0.1, (name, k)
            n += 2
        assert 1e-3 < float(bounds[f"{name}.bf16.y"]) < 2e-2 and 1e-3 < float(bounds[f"{name}.bf16.dx"]) < 2e-2, name
    assert len(bounds.files) == n
